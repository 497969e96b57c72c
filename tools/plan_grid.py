"""Dispatch grid of the host side: which kernel kn_spmm would launch for which call, as text.

Loads the library named by KEYNET_HIP_LIB (default: the product library) through keynet_amd/_capi.py WITHOUT torch, creates a fixed list of operators and
prints, per operator, kn_nnz / kn_nnz_expanded / a hash of kn_export_csr and one line per (n_vecs, ldx = ldy, flags) with the text of kn_spmm_plan; the
batches include 1, 2, 3, 4, 8 and 9 columns and the flags the three narrow ones (KN_FLAG_NARROW, _MFMA, _ROWS).  Float32 CSR operators close the list: three at every flag word, then (csr_cases) the shapes that reach
every launch site of the three CSR sources, a kn_tiled_create operator and a kn_chain_create handle, at the flags a CSR handle reads (--csr: these alone); last
(chain_cases) the operator stacks the whole-net kernel's GPU tests run, as kn_chain_create handles (--chain: these alone; the KN_CHAIN_NO_* knobs of a -DKN_ABLATION
build are set in the environment of the whole run), and (conv_cases) the conv-taps operators that reach every launch site of the matrix-core and narrow regimes, also at
leading dimensions beyond 32-bit offsets and under KN_FLAG_NARROW32 (--conv: these alone).  Nothing is
launched, so the KN_HOST_PACK_ONLY build answers on a machine without a GPU.  Two builds of the library dispatch alike when their outputs are byte-identical:

    KEYNET_HIP_LIB=/path/to/libkeynet_hip.so python tools/plan_grid.py > grid.txt
"""
import ctypes
import hashlib
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ['KEYNET_HIP_NO_TORCH'] = '1'
spec = importlib.util.spec_from_file_location('kn_capi_plan_grid', os.path.join(ROOT, 'keynet_amd', '_capi.py'))
capi = importlib.util.module_from_spec(spec)
spec.loader.exec_module(capi)
GOLD = os.path.join(ROOT, 'tests', 'golden')

BATCHES = (1, 2, 3, 4, 8, 9, 64, 128, 130, 256, 384, 1024, 4096)
FLAGS = (0, capi.KN_FLAG_RELU, capi.KN_FLAG_EXACT, capi.KN_FLAG_EXACT | capi.KN_FLAG_RELU, capi.KN_FLAG_BF16X3)
# the three narrow flags as the Python host sets them (KeyedLayer.kernel), at every batch: beyond 8 columns the library ignores them
FLAGS += (capi.KN_FLAG_NARROW, capi.KN_FLAG_NARROW | capi.KN_FLAG_EXACT | capi.KN_FLAG_RELU, capi.KN_FLAG_NARROW | capi.KN_FLAG_BF16X3, capi.KN_FLAG_NARROW_MFMA,
          capi.KN_FLAG_NARROW_MFMA | capi.KN_FLAG_RELU, capi.KN_FLAG_NARROW_ROWS | capi.KN_FLAG_EXACT, capi.KN_FLAG_NARROW_ROWS | capi.KN_FLAG_EXACT | capi.KN_FLAG_RELU)
SWITCHES = (('KN_NO_SPTR', '1'), ('KN_NO_SMALLK_PIPE', '1'), ('KN_NO_EXACT_TABLE', '1'), ('KN_NO_FILL_EXACT', '1'), ('KN_NO_FILL_TILES2', '1'), ('KN_TABLE_NRB', '2'))
EXPORT_MAX_NNZ = 1 << 22


def report(name, op, out, export=True, flags=None):
    L = capi.lib()
    nx = op.nnz_expanded()
    digest = '-'
    if nx <= EXPORT_MAX_NNZ and export:
        try:
            h = hashlib.sha256()
            for a in op.export_csr():
                h.update(np.ascontiguousarray(a).tobytes())
            digest = h.hexdigest()[:16]
        except capi.KeynetHipError as e:
            digest = str(e)
    out.write('%s shape=%s nnz=%d nnz_expanded=%d csr=%s\n' % (name, op.shape(), op.nnz(), nx, digest))
    buf = ctypes.create_string_buffer(4096)
    for n in BATCHES:
        for ld in (n, n + 1):
            for fl in (flags or FLAGS):
                rc = L.kn_spmm_plan(op.handle, n, ld, ld, fl, buf, 4096)
                text = buf.value.decode() if rc == 0 else 'rc=%d %s' % (rc, L.kn_last_error().decode())
                out.write('%s n=%d ld=%d flags=%d: %s\n' % (name, n, ld, fl, text))


def with_switches(name, make, out):
    """`make()` on a fresh handle under the defaults and under each environment switch (read once, when an operator is created)."""
    report(name, make(), out)
    for (k, v) in SWITCHES:
        os.environ[k] = v
        try:
            op = make()
        finally:
            del os.environ[k]
        report('%s[%s=%s]' % (name, k, v), op, out)


def golden_conv2dtiled(out):
    for fname in sorted(f for f in os.listdir(GOLD) if f.endswith('.npz')):
        z = np.load(os.path.join(GOLD, fname), allow_pickle=False)
        if 'layer_names' in z.files:
            prefixes = ['L.%s.' % str(n) for n in z['layer_names']]
        elif fname == 'tiled_cases.npz':
            prefixes = ['C.%s.' % c for c in sorted(set(k.split('.')[1] for k in z.files if k.startswith('C.')))]
        else:
            continue
        for p in prefixes:
            if str(z[p + 'kind']) != 'conv2dtiled':
                continue

            def make(p=p, z=z):
                return capi.Operator.conv2dtiled(tuple(int(v) for v in z[p + 'shape']), z[p + 'inshape'], z[p + 'outshape'], z[p + 'blocks'], z[p + 'tile_keys'],
                                                 z[p + 'tile_isbias'].astype(np.uint8), z[p + 'tile_chan'], z[p + 'tile_bias'])
            with_switches('%s:%s' % (fname, p.rstrip('.')), make, out)


def factored(cin, cout, hw, ntaps=9, per_pixel=9, coef=False, last=True, dup=False, zero_entry=False, drop=False, seed=0):
    """A keyed-conv-like factored operator: `per_pixel` entries per output pixel on scattered input pixels (dup: on three input pixels only)."""
    rng = np.random.RandomState(seed)
    HW = hw * hw
    (eo, ei, et) = ([], [], [])
    for o in range(HW):
        for k in range(per_pixel):
            eo.append(o)
            ei.append((o % 3) if dup else (o + 7 * k) % HW)
            et.append(k % ntaps)
    taps = rng.randn(ntaps, cout, cin).astype(np.float32)
    if zero_entry:
        taps[0, 0, 0] = 0.0
    ec = (rng.rand(len(eo)).astype(np.float32) + 0.5) if coef else None
    lc = np.concatenate((rng.randn(cout * HW), [1.0])).astype(np.float32) if last else None
    op = capi.Operator.convtaps((cin, hw, hw), (cout, hw, hw), taps, np.array(eo, np.int32), np.array(ei, np.int32), np.array(et, np.int32), ec, lc)
    return op.drop_zero_entries() if drop else op


# ---- float32 CSR operators: every launch site of kn_csr.hip, kn_csr_mfma.hip and kn_csr_narrow.hip (the thresholds: csr_build_groups, csr_choice) ----
# the flags a CSR handle reads: ReLU and KN_FLAG_NARROW_ROWS
CSR_FLAGS = (0, capi.KN_FLAG_RELU, capi.KN_FLAG_NARROW_ROWS | capi.KN_FLAG_EXACT, capi.KN_FLAG_NARROW_ROWS | capi.KN_FLAG_EXACT | capi.KN_FLAG_RELU)


def csr_from_rows(row_cols, n_cols, seed, shuffle=True):
    """A CSR operator from per-row column sequences (stored order = the order given), N(0, 1) values, the rows in a fixed random order."""
    rng = np.random.RandomState(seed)
    if shuffle:
        row_cols = [row_cols[i] for i in rng.permutation(len(row_cols))]
    indptr = np.concatenate(([0], np.cumsum([len(c) for c in row_cols]))).astype(np.int32)
    indices = (np.concatenate(row_cols) if indptr[-1] else np.zeros(0)).astype(np.int32)
    return ((len(row_cols), n_cols), indptr, indices, rng.randn(len(indices)).astype(np.float32))


def groups(rng, n_cols, sizes, seq_len):
    """One pattern group per entry of `sizes`: that many rows over one random sequence of `seq_len` distinct columns."""
    rows = []
    for n in sizes:
        seq = rng.choice(n_cols, seq_len, replace=False)
        rows += [seq] * n
    return rows


def ragged(rng, n_cols, n_rows, lo, hi):
    """Rows no other row shares a sequence with (almost surely): lo .. hi distinct random columns each."""
    return [rng.choice(n_cols, rng.randint(lo, hi + 1), replace=False) for _ in range(n_rows)]


def csr_cases():
    """(name, (shape, indptr, indices, data), environment switches that change its plan)."""
    empty = [np.zeros(0, np.int64)] * 3
    rng = np.random.RandomState(11)
    # 42 chunks of 32 member rows over 256-column sequences: the matrix-pipe lists at 4 096 columns (n_mf * 16 * 4 >= 2 048); groups of 64 / 96 members fill the
    # 2- and 3-block chunks under KN_MF_NRB; five small groups (the ws list behind the matrix-pipe launch), loose and empty rows
    mf = groups(rng, 4096, [32] * 30 + [64, 64, 96, 96, 40], 256) + groups(rng, 4096, [2, 5, 9, 16, 23], 64) + ragged(rng, 4096, 10, 5, 30) + empty
    yield ('csr matrix-pipe groups', csr_from_rows(mf, 4096, 12), (('KN_MF_NRB', '2'), ('KN_MF_NRB', '3'), ('KN_GROUP_MFMA', '0'), ('KN_NO_GROUP_PIPE', '1')))
    # conv-like groups with short sequences: the rule keeps them on the vector ALU (pipelined kernel, 16 rows per wavefront), KN_GROUP_MFMA=1 moves them
    rng = np.random.RandomState(13)
    yield ('csr conv-like groups', csr_from_rows(groups(rng, 1024, [32] * 64, 28), 1024, 14), (('KN_GROUP_MFMA', '1'), ('KN_NO_GROUP_PIPE', '1')))
    # groups that leave 16-row bundles half empty (8 rows per wavefront of the pipelined kernel) and loose rows behind them
    rng = np.random.RandomState(15)
    yield ('csr thin groups', csr_from_rows(groups(rng, 1024, [9] * 300, 28) + ragged(rng, 1024, 50, 3, 12), 1024, 16), (('KN_NO_GROUP_PIPE', '1'),))
    # a keyed Linear: one big group; 32 chunks of 16 rows reach the matrix pipe by rule at 4 096 columns (n_mf16 * 64 >= 2 048)
    rng = np.random.RandomState(17)
    yield ('csr linear 512x2100', csr_from_rows(groups(rng, 2100, [512], 2100), 2100, 18, shuffle=False),
           (('KN_BIG_MFMA16', '0'), ('KN_BIG_MFMA16', '1'), ('KN_NO_BIG_GROUPS', '1')))
    # patched rows: groups of 12 members over 40 columns, and single rows that are a group's sequence minus 1 .. 4 entries
    rng = np.random.RandomState(19)
    rows = []
    for g in range(4):
        seq = rng.choice(512, 40, replace=False)
        rows += [seq] * 12 + [np.delete(seq, rng.choice(40, miss, replace=False)) for miss in (1, 2, 3, 4)]
    yield ('csr patched rows', csr_from_rows(rows + ragged(rng, 512, 6, 2, 9), 512, 20), ())
    # long ungrouped rows (>= 1 024 entries): three of them take the deep-queue role, 64 the row kernel at 4 096 columns (64 * 16 tiles >= 1 024)
    rng = np.random.RandomState(21)
    yield ('csr long rows few', csr_from_rows(ragged(rng, 2048, 3, 1024, 1500) + ragged(rng, 2048, 20, 4, 40), 2048, 22), (('KN_NO_BIG_GROUPS', '1'),))
    yield ('csr long rows many', csr_from_rows(ragged(rng, 2048, 64, 1024, 1100) + groups(rng, 2048, [20], 48), 2048, 23), ())
    # 4 096 short loose rows (overlapping 3-column windows): the locality order, csr_rows_pair_kernel at 128 and 384 columns
    yield ('csr pool 4096x4100', csr_from_rows([np.arange(r, r + 3) for r in range(4096)], 4100, 24), ())
    # a bit of everything, and loose rows too long for a lane of the row-lane kernel (> 64 entries)
    rng = np.random.RandomState(25)
    seq = rng.choice(3000, 48, replace=False)
    rows = [seq] * 30 + [np.delete(seq, [7])] + groups(rng, 3000, [3, 17], 20) + ragged(rng, 3000, 2, 1024, 1030) + ragged(rng, 3000, 12, 70, 100) + empty
    yield ('csr mixed', csr_from_rows(rows, 3000, 26), (('KN_NO_BIG_GROUPS', '1'),))


def csr_operators(out):
    for (name, (shape, ip, ix, dt), switches) in csr_cases():
        for (k, v) in ((None, None),) + tuple(switches):
            if k:
                os.environ[k] = v
            try:
                op = capi.Operator.csr(shape, ip, ix, dt)
            finally:
                if k:
                    del os.environ[k]
            report(name + ('[%s=%s]' % (k, v) if k else ''), op, out, export=False, flags=CSR_FLAGS)
    # kn_tiled_create: a block-diagonal tiled operator (expanded to CSR on the host, packed like one)
    rng = np.random.RandomState(27)
    tile = rng.randn(8, 8).astype(np.float32)
    (tr, tc) = np.nonzero(np.ones((8, 8)))
    blocks = np.array([[8 * i, 8 * i, 0] for i in range(40)], np.int64)
    report('tiled 320x320', capi.Operator.tiled((320, 320), blocks, np.array([0, 64], np.int64), tr.astype(np.int32), tc.astype(np.int32), tile.ravel()), out, flags=CSR_FLAGS)
    # kn_chain_create over the CSR layers of the LeNet golden key-net: its plan names the LDS and operator bytes of the packed layout
    z = np.load(os.path.join(GOLD, 'lenet_perm.npz'), allow_pickle=False)
    ops = []
    for lname in [str(n) for n in z['layer_names']]:
        p = 'L.%s.' % lname
        if str(z[p + 'kind']) == 'csr':
            ops.append(capi.Operator.csr(tuple(int(v) for v in z[p + 'shape']), z[p + 'indptr'], z[p + 'indices'], z[p + 'data'].astype(np.float32)))
    report('chain lenet_perm', capi.Operator.chain(ops, [capi.KN_FLAG_RELU] * (len(ops) - 1) + [0]), out, export=False, flags=CSR_FLAGS)


# ---- kn_chain_create handles: every layer decision of kn_chain.hip's packer (chain_choose_walk, chain_place_staging) ----
CHAIN_BATCHES = (1, 3, 4, 5, 37, 1024)          # the plan text depends on the batch through the grid alone


def _csr_arrays(row_cols, rng, row_vals=None):
    """(indptr, indices, data) from per-row column sequences, stored order as given; N(0, 1) values unless `row_vals` gives them."""
    indptr = np.concatenate(([0], np.cumsum([len(c) for c in row_cols]))).astype(np.int32)
    indices = (np.concatenate(row_cols) if indptr[-1] else np.zeros(0)).astype(np.int32)
    data = np.concatenate(row_vals).astype(np.float32) if row_vals is not None else rng.randn(len(indices)).astype(np.float32)
    return (indptr, indices, data)


def chain_grouped(rng, rows, cols, group, nnz, tail_loose):
    """Conv-like: groups of `group` rows over one unsorted sequence of `nnz` columns (duplicates allowed), `tail_loose` short rows of their own at the end."""
    (rc, shared) = ([], None)
    for r in range(rows):
        if r >= rows - tail_loose:
            rc.append(rng.randint(0, cols, size=rng.randint(1, 6)))
        else:
            if r % group == 0:
                shared = rng.randint(0, cols, size=nnz)
            rc.append(shared)
    return _csr_arrays(rc, rng)


def chain_dense(rng, rows, cols, n_other=0, seq_len=None):
    """A keyed Linear: `rows - n_other` rows over one sequence of `seq_len` (default: all) distinct columns, `n_other` rows of 1 .. 3 columns of their own behind them."""
    perm = rng.permutation(cols)[:seq_len]
    return _csr_arrays([perm] * (rows - n_other) + [rng.choice(cols, size=rng.randint(1, 4), replace=False) for _ in range(n_other)], rng)


def chain_random(rng, rows, cols, kind):
    """The layers of the random stack: 'grouped' (a new sequence of 1 .. 39 columns every 7 rows), 'dense' (one permutation, a row in eleven an entry short),
    'loose' (0 .. 13 random columns per row, duplicates and empty rows among them)."""
    (rc, shared) = ([], None)
    for r in range(rows):
        if kind == 'grouped':
            if r % 7 == 0:
                shared = rng.randint(0, cols, size=rng.randint(1, 40))
            rc.append(shared)
        elif kind == 'dense':
            if shared is None:
                shared = rng.permutation(cols)
            rc.append(shared if r % 11 else shared[:-1])
        else:
            rc.append(rng.randint(0, cols, size=(0 if r % 13 == 5 else rng.randint(1, 14))))
    return _csr_arrays(rc, rng)


def chain_pixels(rng, shared_values, pixels=600, ch=8, nnz=22, cols=500):
    """`pixels` column sequences of `ch` rows each, the rows in a random order; shared_values: every pixel carries the same `ch` value sequences, permuted per pixel."""
    base_vals = rng.randn(ch, nnz).astype(np.float32)
    order = rng.permutation(pixels * ch)
    pat = [rng.randint(0, cols, size=nnz) for _ in range(pixels)]
    rows = [None] * (pixels * ch)
    for p in range(pixels):
        perm_ch = rng.permutation(ch)
        for c in range(ch):
            rows[order[p * ch + c]] = (pat[p], base_vals[perm_ch[c]] if shared_values else rng.randn(nnz).astype(np.float32))
    return _csr_arrays([r[0] for r in rows], rng, [r[1] for r in rows])


def chain_cases():
    """(name, [((rows, cols), (indptr, indices, data), relu), ...]): the operator stacks of tests/test_parity_gpu.py's test_whole_net_kernel_* tests, restated."""
    rng = np.random.RandomState(103)
    yield ('chain random', [((r, c), chain_random(rng, r, c, kind), relu)
                            for (r, c, kind, relu) in ((301, 97, 'grouped', 1), (150, 301, 'loose', 0), (70, 150, 'dense', 1), (33, 70, 'dense', 1), (9, 33, 'dense', 0))])
    rng = np.random.RandomState(7)
    (G, D) = (lambda *a: chain_grouped(rng, *a), lambda *a: chain_dense(rng, *a))
    yield ('chain pattern pools', [((645, 200), G(645, 200, 6, 11, 5), 1), ((130, 645), G(130, 645, 16, 50, 2), 0), ((70, 130), D(70, 130), 1), ((10, 70), D(10, 70), 0)])
    yield ('chain keyed linears', [((645, 200), G(645, 200, 6, 11, 5), 1), ((131, 645), G(131, 645, 16, 50, 2), 0), ((121, 131), D(121, 131, 1), 1), ((85, 121), D(85, 121, 3), 1),
                                   ((11, 85), D(11, 85, 1), 0)])
    yield ('chain linear first', [((70, 130), D(70, 130), 1), ((10, 70), D(10, 70, 1), 0)])
    yield ('chain pool does not fit', [((4100, 4200), G(4100, 4200, 6, 110, 2), 1), ((64, 4100), G(64, 4100, 8, 9, 0), 0)])
    yield ('chain two rows per lane 6 16', [((2051, 300), G(2051, 300, 6, 11, 5), 1), ((1300, 2051), G(1300, 2051, 1, 7, 0), 0), ((1609, 1300), G(1609, 1300, 16, 50, 9), 1),
                                            ((90, 1609), D(90, 1609), 1), ((10, 90), D(10, 90), 0)])
    yield ('chain two rows per lane 11', [((1500, 257), G(1500, 257, 11, 13, 1), 0), ((33, 1500), D(33, 1500), 0)])
    yield ('chain linear 336x2184 first', [((336, 2184), D(336, 2184, 9), 0), ((50, 336), D(50, 336, 1), 1)])
    # a thin first operator whose two pool copies do not fit beside 9 000 + 70 + 1 activations: 704 quads twice = 22.5 KB against 18.7 KB of room (at 8 600 columns they fit)
    yield ('chain thin pool does not fit', [((70, 9000), D(70, 9000, 0, 2800), 0)])
    yield ('chain thin pool fits', [((70, 8600), D(70, 8600, 0, 2800), 0)])
    # two rows per lane tried and dropped: 64 rows of one 400-column pattern fill a slice of their own at one row per lane; at two they leave half of it to 32 four-column
    # patterns, each then stored at 100 quads -- 4 772 quads against 3 175 of room, where the one-row pool takes 1 604
    yield ('chain two rows per lane do not fit', [((3064, 4000), _csr_arrays([rng.randint(0, 4000, size=400)] * 64 + [c for c in rng.randint(0, 4000, size=(1500, 4)) for _ in range(2)], rng), 1)])
    # two pattern pools that fit beside the activations one at a time only: the second is staged at the start of its own layer
    yield ('chain pool staged late', [((2000, 3000), G(2000, 3000, 8, 40, 0), 1), ((400, 2000), G(400, 2000, 8, 240, 0), 0)])
    rng = np.random.RandomState(21)
    for shared_values in (True, False):
        yield ('chain pixels shared_values=%d' % shared_values, [((4800, 500), chain_pixels(rng, shared_values), 1)])
    rng = np.random.RandomState(29)
    yield ('chain 0 rows', [((0, 7), _csr_arrays([], rng), 0)])
    yield ('chain empty rows', [((5, 7), _csr_arrays([np.zeros(0, np.int64)] * 5, rng), 1)])


def chain_operators(out):
    L = capi.lib()
    buf = ctypes.create_string_buffer(4096)
    for (name, layers) in chain_cases():
        try:
            ops = [capi.Operator.csr(shape, ip, ix, dt) for (shape, (ip, ix, dt), relu) in layers]
            chain = capi.Operator.chain(ops, [capi.KN_FLAG_RELU if relu else 0 for (shape, csr, relu) in layers])
        except capi.KeynetHipError as e:
            out.write('%s: %s\n' % (name, e))
            continue
        out.write('%s shape=%s nnz=%d\n' % (name, chain.shape(), chain.nnz()))
        for n in CHAIN_BATCHES:
            rc = L.kn_spmm_plan(chain.handle, n, n, n, capi.KN_FLAG_EXACT, buf, 4096)
            out.write('%s n=%d: %s\n' % (name, n, buf.value.decode() if rc == 0 else 'rc=%d %s' % (rc, L.kn_last_error().decode())))


# ---- conv-taps handles: every launch site of the matrix-core and the narrow regimes (mfma_choice / narrow_choice in kn_conv.hip) ----
N32 = capi.KN_FLAG_NARROW32
# leading dimensions that cross the 32-bit offset tests of a 36-pixel operator: the wave-uniform pointers of the 128-column tiles (1 << 21), the straight-line loaders
# and the narrow kernels' size rule (1 << 22), everything (1 << 26)
BIG_LDS = (1 << 21, 1 << 22, 1 << 26)


def conv_cases():
    """(name, make, [(n_vecs, flags), ...], environment switches that change its plan): the smallest operators that reach each site.  Sites only the occupancy
    query decides (tail_split, occ_cap, the grid of the persistent small-K kernel) show on a machine with a GPU; the CPU-only build answers that query with 0."""
    (NARROW, MFMA, BF16X3, EXACT) = (capi.KN_FLAG_NARROW, capi.KN_FLAG_NARROW_MFMA, capi.KN_FLAG_BF16X3, capi.KN_FLAG_EXACT)
    wide = [(n, fl) for n in (128, 130, 256) for fl in (0, BF16X3)]
    narrow = [(n, fl) for fl in (NARROW, MFMA, NARROW | EXACT) for n in (1, 2, 3, 4, 5, 8)] + [(n, fl | N32) for fl in (NARROW, MFMA) for n in (9, 16, 17, 24, 32)]
    # small-K: the persistent kernel (one 64-channel tile), the one-shot kernel under KN_NO_SMALLK_PIPE and at two channel tiles; at 128 columns the KC = 4 tiles
    yield ('conv cin=3 cout=64', lambda: factored(3, 64, 6), wide + narrow, (('KN_NO_SMALLK_PIPE', '1'),))
    yield ('conv cin=3 cout=128', lambda: factored(3, 128, 6), wide, ())
    # ten slots x 3 channels exceed the small-K contraction: the KC = 4 tiles with straight-line loaders (Cin < 4) at whole tiles, generic ones else
    yield ('conv cin=3 cout=64 slots10', lambda: factored(3, 64, 6, per_pixel=10), wide, ())
    yield ('conv cin=3 cout=128 slots10', lambda: factored(3, 128, 6, per_pixel=10), wide, ())
    yield ('conv cin=5 cout=128', lambda: factored(5, 128, 6), wide, ())
    # the KC = 16 tiles: wave-uniform pointers, per-thread pointers under KN_NO_SPTR, generic loaders at 130 columns and with coefficients under KN_NO_SPTR; bf16x3
    for (cin, cout) in ((16, 64), (16, 128), (32, 128)):
        for coef in (False, True):
            yield ('conv cin=%d cout=%d coef=%d' % (cin, cout, coef), lambda: factored(cin, cout, 6, coef=coef), wide + (narrow if cin == 16 else []), (('KN_NO_SPTR', '1'),))
    # more than 64 slots per pixel: slot groups
    yield ('conv slots70 cin=32 cout=64', lambda: factored(32, 64, 9, per_pixel=70), wide, (('KN_NO_SPTR', '1'),))
    yield ('conv slots70 cin=32 cout=128', lambda: factored(32, 128, 9, per_pixel=70), wide, (('KN_NO_SPTR', '1'),))
    # several slots on one pixel pair: the narrow kernels that sum stored values (at most 16 columns per block beyond 8)
    for coef in (False, True):
        yield ('conv dup cin=16 cout=64 coef=%d' % coef, lambda: factored(16, 64, 6, coef=coef, dup=True), narrow, ())
    # 2.4 MB of taps: the 9 .. 32 column kernel keeps the width's form (16 | 32 columns per block) on a small layer
    yield ('conv cin=256 cout=256', lambda: factored(256, 256, 6), narrow, ())


def conv_operators(out):
    L = capi.lib()
    buf = ctypes.create_string_buffer(4096)
    for (name, make, calls, switches) in conv_cases():
        for (k, v) in ((None, None),) + tuple(switches):
            if k:
                os.environ[k] = v
            try:
                op = make()
            finally:
                if k:
                    del os.environ[k]
            tag = name + ('[%s=%s]' % (k, v) if k else '')
            for (n, fl) in calls:
                for ld in (n, n + 1) + BIG_LDS:
                    rc = L.kn_spmm_plan(op.handle, n, ld, ld, fl, buf, 4096)
                    out.write('%s n=%d ld=%d flags=%d: %s\n' % (tag, n, ld, fl, buf.value.decode() if rc == 0 else 'rc=%d %s' % (rc, L.kn_last_error().decode())))


def main():
    out = sys.stdout
    if '--conv' in sys.argv[1:]:
        return conv_operators(out)
    if '--csr' in sys.argv[1:]:
        return csr_operators(out)
    if '--chain' in sys.argv[1:]:
        return chain_operators(out)
    golden_conv2dtiled(out)
    for cin in (3, 5, 16, 32, 64):
        for cout in (7, 64, 128, 192):
            for coef in (False, True):
                for last in (False, True):
                    name = 'factored cin=%d cout=%d coef=%d last=%d' % (cin, cout, coef, last)
                    with_switches(name, lambda: factored(cin, cout, 6, coef=coef, last=last), out)
    for (cin, cout) in ((5, 7), (32, 64), (16, 192)):
        for coef in (False, True):
            with_switches('dup cin=%d cout=%d coef=%d' % (cin, cout, coef), lambda: factored(cin, cout, 6, coef=coef, dup=True), out)
            with_switches('slots70 cin=%d cout=%d coef=%d' % (cin, cout, coef), lambda: factored(cin, cout, 9, per_pixel=70, coef=coef), out)
            with_switches('taps25 cin=%d cout=%d coef=%d' % (cin, cout, coef), lambda: factored(cin, cout, 6, ntaps=25, per_pixel=25, coef=coef), out)
            with_switches('dup taps25 cin=%d cout=%d coef=%d' % (cin, cout, coef), lambda: factored(cin, cout, 6, ntaps=25, per_pixel=25, coef=coef, dup=True), out)
    for (cin, cout, hw) in ((3, 64, 9), (16, 64, 6), (16, 128, 8), (32, 192, 12), (64, 96, 6)):
        for last in (False, True):
            with_switches('dropzero cin=%d cout=%d hw=%d last=%d' % (cin, cout, hw, last), lambda: factored(cin, cout, hw, last=last, zero_entry=True, drop=True), out)
    for coef in (False, True):             # enough (pixel, channel bundle) rows for 16 channels per wavefront of the order-preserving pipeline
        with_switches('wide cin=16 cout=192 hw=20 coef=%d' % coef, lambda: factored(16, 192, 20, coef=coef), out)
    with_switches('dropzero coef cin=16 cout=64', lambda: factored(16, 64, 6, coef=True, zero_entry=True, drop=True), out)
    with_switches('dropzero dup cin=16 cout=64', lambda: factored(16, 64, 6, dup=True, zero_entry=True, drop=True), out)
    rng = np.random.RandomState(1)
    D = rng.randn(37, 513).astype(np.float32)
    D[-1, :] = 0
    D[-1, -1] = 1
    with_switches('dense 37x513', lambda: capi.Operator.dense(D), out)
    # float32 CSR operators (KN_FLAG_NARROW_ROWS): scattered rows, a pool-like operator (loose rows only), a keyed-Linear-like one with a big pattern group
    import scipy.sparse
    pool = scipy.sparse.kron(scipy.sparse.identity(40), np.full((1, 4), 0.25)).tocsr()
    for (name, M) in (('csr random 300x257', scipy.sparse.random(300, 257, density=0.1, format='csr', random_state=2)), ('csr pool 40x160', pool),
                      ('csr linear 300x2100', scipy.sparse.csr_matrix(rng.randn(300, 2100)))):
        M = M.astype(np.float32)
        report(name, capi.Operator.csr(M.shape, M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data), out, export=False)
    csr_operators(out)
    chain_operators(out)
    conv_operators(out)


if __name__ == '__main__':
    main()
