"""The bit-exact contract at the edges of float32 (tests/value_classes.py): every order-preserving kernel family against the CPU oracle under bits_equal -- the
uint32 patterns, so the sign of a zero, the sign of an Inf and a flushed subnormal all count -- with subnormal operands and results, products that underflow, sums that
cross the normal / subnormal boundary or overflow on the way, 120 binades in one block, neighbouring batch columns of different classes, and integer data full of
-0.0; the float64 kernel where its two conversions and its one rounding matter; the screen slot's bit pattern; and, for the kernels that run under the float-key
tolerance, exact covariance with a power-of-two scale.

One row per launch site (FAMILIES; the plan of kn_spmm_plan must name it), inside a row a loop over the seven regimes with ReLU off and on.  The operators are the
smallest ones the neighbouring modules already use to reach a site (their builders take the operator-value variant of a regime as an optional argument).  Half of the
rows run on a column window (ld = n + 8, first column 4) of a block that is NaN outside the window, into a sentinel-filled block that must stay one outside.

Columns.  The reference treats every batch column on its own, and the oracle's subnormal arithmetic is slow on a CPU (tens of ns per product).  A batch wider than
32 columns therefore holds 29 distinct columns, column c a copy of column c mod 29 (29 is odd: a lane of four or two columns sees every position of every source
column), and the reference block is the oracle's 29 columns laid out the same way: every element of the output is still compared.

Shares.  Every (row, regime) checks the regime's floors on the class shares of the REFERENCE (value_classes.REGIMES) before anything is launched: a case that misses
its floor is an error of the generator.  Run with -s for the per-case shares.

A build with -fgpu-flush-denormals-to-zero (a scratch variant, keynet_amd.build.build(out=..., extra=[...]) loaded through KEYNET_HIP_LIB; never committed) fails the
`subnormal`, `boundary` or `underflow` case of every family row and of the float64 rows, and passes `overflow`, `wide` and the covariance cases.

Measured on an MI355X: the module's 96 cases take 14 s from its first case to its last (19 s for the pytest process; the slowest case, the 256 -> 256 channel operator of
convtaps_narrow32_kernel<NV=16>, 3.7 s, most of it the oracle); the module prints its wall time at teardown (run with -s).
"""
import time

import numpy as np
import pytest
import torch

import oracle
import value_classes as vc
from keynet_amd import io as kio
from keynet_amd import sparse as ksp
from keynet_amd import _capi
from keynet_amd.layer import KeyedLayer
from narrow_helpers import _spmm, SENTINEL
from test_parity_gpu import _chain_dense, _chain_dense_plus, _chain_grouped, dev
import test_conv_choice_gpu as cc
import test_large_offsets_gpu as lo
import test_narrow_fill_gpu as nf

pytestmark = pytest.mark.gpu

C = _capi
(RELU, EXACT, BF16X3, NARROW, MFMA, N32, N64, ROWS, LINEAR, TAPS, TAPS32, FILL) = (
    C.KN_FLAG_RELU, C.KN_FLAG_EXACT, C.KN_FLAG_BF16X3, C.KN_FLAG_NARROW, C.KN_FLAG_NARROW_MFMA, C.KN_FLAG_NARROW32, C.KN_FLAG_NARROW64, C.KN_FLAG_NARROW_ROWS,
    C.KN_FLAG_NARROW_LINEAR, C.KN_FLAG_NARROW_TAPS, C.KN_MODIFIER_NARROW_TAPS32, C.KN_MODIFIER_NARROW_FILL)
DISTINCT = 29                      # distinct columns of a batch wider than 32 (module docstring)
_T0 = [None]


@pytest.fixture(scope='module', autouse=True)
def _wall():
    _T0[0] = time.time()
    yield
    torch.cuda.synchronize()
    print('\ntest_value_classes_gpu: wall %.1f s' % (time.time() - _T0[0]))
    for b in (lo.conv, lo.dropped_zero_conv, lo.grouped_csr, lo.loose_csr, lo.long_rows_csr, lo.linear_csr, lo.f64_csr, lo.patched_csr):
        b.cache_clear()
    for k in [k for k in cc._ops if k[2] is not None]:
        del cc._ops[k]
    for k in [k for k in nf._built if k[1] is not None]:
        del nf._built[k]
    torch.cuda.empty_cache()


# ---- operators: maker(variant) -> (handle, (shape, indptr, indices, data) for the oracle, homogeneous row?) ---------------------------------------------

def _lo(builder, *args, **kw):
    def make(variant):
        c = builder(*args, values=variant, **kw)
        c = c[0] if isinstance(c, tuple) else c                      # (patched_csr returns the rows it patched as well)
        return (c.op, (c.shape, c.ip, c.ix, c.dt), c.has_last)
    return make


def _cc(name):
    def make(variant):
        (op, csr) = cc._operator(name, None, variant)
        return (op, csr, True)
    return make


def _nf(case):
    def make(variant):
        (W, M, _, _) = nf._build(case, values=variant)
        with torch.cuda.device(dev()):
            op = W._device_op(dev())
        return (op, (M.shape, M.indptr, M.indices, M.data.astype(np.float32)), bool(case[2][-1]))
    return make


MF = (('KN_GROUP_MFMA', '1'),)
# (id, maker, n_vecs, flags, what the plan must name, column window[, distinct columns, regimes])
FAMILIES = [
    # CSR
    ('csr_rows<4>-loose', _lo(lo.loose_csr), 256, EXACT, ['csr_rows_kernel<vec=4>'], False),
    ('csr_rows<1>-loose', _lo(lo.loose_csr), 8, EXACT, ['csr_rows_kernel<vec=1>'], True),
    ('csr_rows_pair', _lo(lo.loose_csr), 128, EXACT, ['csr_rows_pair_kernel'], True),
    ('csr_rows<4>-long-rows', _lo(lo.long_rows_csr), 256, EXACT, ['csr_rows_kernel<vec=4> (long rows)'], False),        # (needs 1 024 long rows at 256 columns)
    ('csr_rows-long-deep-role', _lo(lo.long_rows_csr, long_rows=40), 64, EXACT, ['csr_big_group_kernel'], False),
    ('csr_group', _lo(lo.grouped_csr), 100, EXACT, ['csr_group_kernel<vec=2'], True),
    ('csr_group_pipe', _lo(lo.grouped_csr), 256, EXACT, ['csr_group_pipe_kernel'], False),
    ('csr_big_group', _lo(lo.linear_csr, 257, 2048, env=(('KN_BIG_MFMA16', '0'),)), 64, EXACT, ['csr_big_group_kernel'], True),
    ('csr_group_mfma16', _lo(lo.linear_csr, 257, 2048, env=(('KN_BIG_MFMA16', '1'),)), 64, EXACT, ['csr_group_mfma16_kernel'], False),
    ('csr_group_mfma', _lo(lo.grouped_csr, 96, 200, 1024, env=MF), 256, EXACT, ['csr_group_mfma_kernel<row blocks=1>'], False),
    ('csr_group_mfma-window', _lo(lo.grouped_csr, 96, 200, 1024, env=MF), 128, EXACT, ['csr_group_mfma_kernel<row blocks=1>'], True),
    ('csr_group_mfma-taps-table', _lo(lo.dropped_zero_conv), 128, EXACT, ['csr_group_mfma_kernel<row blocks=1,taps>', 'convtaps_zero_guard_kernel', 'conv_lastrow_kernel'], False),
    ('csr_patch_guard', _lo(lo.patched_csr), 37, EXACT, ['csr_patch_guard_kernel<27 patched rows>', 'csr_group_kernel'], True),
    ('csr_narrow-1', _lo(lo.loose_csr), 1, EXACT | ROWS, ['csr_narrow_kernel<nv=1'], False),
    ('csr_narrow-3', _lo(lo.loose_csr), 3, EXACT | ROWS, ['csr_narrow_kernel<nv=4,masked to 3'], True),
    ('csr_narrow-8', _lo(lo.loose_csr), 8, EXACT | ROWS, ['csr_narrow_kernel<nv=8'], False),
    ('csr_stream_group-8', _lo(lo.linear_csr, 257, 2048), 8, EXACT | LINEAR, ['csr_stream_group_kernel<W=8,NV=1>'], True),
    ('csr_stream_group-32', _lo(lo.linear_csr, 257, 2048), 32, EXACT | LINEAR, ['csr_stream_group_kernel<W=8,NV=4>'], False),
    # conv-taps
    ('convtaps_exact', _lo(lo.conv, 4, 32, 8, 3, 1, False, True, env=(('KN_NO_FILL_EXACT', '1'),)), 64, EXACT, ['convtaps_exact_kernel<vec=1>', 'conv_lastrow_kernel'], True),
    ('convtaps_exact-zero-guard', _lo(lo.dropped_zero_conv), 64, EXACT, ['convtaps_exact_kernel<vec=1>', 'convtaps_zero_guard_kernel', 'conv_lastrow_kernel'], False),
    ('convtaps_exact_pipe-4-per-lane', _cc('c16-o64'), 256, EXACT, ['convtaps_exact_pipe_kernel<8>', 'conv_lastrow_kernel'], False),
    ('convtaps_exact_pipe-128-tiles', _cc('c16-o64'), 128, EXACT, ['convtaps_exact_pipe_kernel<8,128-column tiles>'], True),
    ('convtaps_exact_pipe-coef', _cc('c16-o64-coef'), 128, EXACT, ['convtaps_exact_pipe_kernel<8,coef,128-column tiles>'], False),
    ('convtaps_exact_pipe64', _cc('c16-o64'), 64, EXACT | NARROW | N32 | N64, ['convtaps_exact_pipe64_kernel'], False),
    ('convtaps_exact_pipe64-33', _cc('c16-o64'), 33, EXACT | NARROW | N32 | N64, ['convtaps_exact_pipe64_kernel'], True),
    ('convtaps_exact_fill', _cc('c16-o64-dup'), 64, EXACT, ['convtaps_exact_fill_kernel<taps in registers>'], True),
    ('convtaps_exact_fill-coef', _lo(lo.conv, 4, 32, 8, 3, 1, False, True), 64, EXACT, ['convtaps_exact_fill_kernel<taps in registers>', 'conv_lastrow_kernel'], False),
    ('convtaps_exact_fill-coef-filled-in', _nf(nf.ELIGIBLE[0]), 128, EXACT, ['convtaps_exact_fill_kernel<taps in registers>'], True),
    # narrow conv-taps
    ('convtaps_narrow-1', _cc('c16-o64'), 1, NARROW, ['convtaps_narrow_kernel<1> (lane'], False),
    ('convtaps_narrow-3', _cc('c16-o64'), 3, NARROW, ['convtaps_narrow_kernel<4,masked to 3> (lane'], True),
    ('convtaps_narrow-8', _cc('c16-o64'), 8, NARROW, ['convtaps_narrow_kernel<8> (lane'], False),
    ('convtaps_narrow-8-summed-coef', _cc('c16-o64-dup-coef'), 8, NARROW, ['convtaps_narrow_kernel<8,stored values summed,coef> (lane'], True),
    ('convtaps_narrow32-NV8', _cc('c16-o64'), 9, NARROW | N32, ['convtaps_narrow32_kernel<NV=8, masked to 9, 2 column blocks>'], True),
    # (rows of 2 305 entries x 9 216 rows: two distinct columns and four regimes keep the oracle at a few seconds)
    ('convtaps_narrow32-NV16', _cc('c256-o256'), 16, NARROW | N32, ['convtaps_narrow32_kernel<NV=16, 1 column block>'], False, 2, ('subnormal', 'by-column', 'overflow', 'signed-zero')),
    ('convtaps_narrow32-NV32', _cc('c256-o256'), 32, NARROW | N32, ['convtaps_narrow32_kernel<NV=32, 1 column block>'], False, 2, ('boundary', 'by-column', 'overflow', 'signed-zero')),
    ('convtaps_narrow_taps-3', _cc('c16-o64'), 3, NARROW | TAPS, ['convtaps_narrow_taps_kernel<9 value rows, P=1, NV=4, masked to 3>'], False),
    ('convtaps_narrow_taps-8', _cc('c16-o64'), 8, NARROW | TAPS, ['convtaps_narrow_taps_kernel<9 value rows, P=1, NV=8>'], True),
    ('convtaps_narrow_taps32-9', _cc('c16-o64'), 9, NARROW | N32 | TAPS | TAPS32, ['convtaps_narrow_taps32_kernel<9 value rows, NV=8, masked to 9, 2 column blocks>'], False),
    ('convtaps_narrow_taps32-32', _cc('c16-o64'), 32, NARROW | N32 | TAPS | TAPS32, ['convtaps_narrow_taps32_kernel<9 value rows, NV=8, 4 column blocks>'], True),
    ('convtaps_narrow_fill-3', _nf(nf.ELIGIBLE[0]), 3, NARROW | FILL, ['convtaps_narrow_fill_kernel<NV=4, masked to 3, 1 column block, coef>'], True),
    ('convtaps_narrow_fill-8', _nf(nf.ELIGIBLE[2]), 8, NARROW | FILL, ['convtaps_narrow_fill_kernel<NV=8, 1 column block, coef>'], False),
    ('convtaps_narrow_fill-32', _nf(nf.ELIGIBLE[1]), 32, NARROW | N32 | FILL, ['convtaps_narrow_fill_kernel<NV=8, 4 column blocks, coef>'], False),
]


# ---- the harness ------------------------------------------------------------------------------------------------------------------------------------------

def _seed(*parts):
    return sum((i + 1) * sum(ord(ch) for ch in str(p)) for (i, p) in enumerate(parts)) % (2 ** 31)


def _columns(n, distinct=None):
    return np.arange(n) % (distinct or (n if n <= 32 else DISTINCT))


def _regime_block(regime, cols, n, has_last, per_row, seed, distinct=None):
    """(X [cols, n] under the regime, the distinct columns it is made of, the column map)."""
    rng = np.random.RandomState(seed)
    src = _columns(n, distinct)
    Xd = rng.randn(cols, int(src.max()) + 1).astype(np.float32)
    if has_last:
        Xd[-1] = 1.0
    Xd = vc.REGIMES[regime].apply(Xd, has_last, rng, per_row)
    return (np.ascontiguousarray(Xd[:, src]), Xd, src)


def _oracle(csr, X):
    with np.errstate(all='ignore'):
        return oracle.csr_matvecs(csr[0], csr[1], csr[2], csr[3], X)


def _window(X, window):
    """(device block [cols, ld], ld, first column): the batch as it is, or as columns 4 .. 4 + n of a block that is NaN everywhere else."""
    n = X.shape[1]
    if not window:
        return (torch.as_tensor(X).to(dev()), None, 0)
    Xw = np.full((X.shape[0], n + 8), np.nan, dtype=np.float32)
    Xw[:, 4:4 + n] = X
    return (torch.as_tensor(Xw).to(dev()), n + 8, 4)


def _outside_intact(whole, n, start):
    out = torch.ones(whole.shape[1], dtype=torch.bool, device=whole.device)
    out[start:start + n] = False
    return bool(torch.all(whole[:, out] == SENTINEL))


def _run_family(row, regimes=None):
    (tag, make, n, flags, texts, window) = row[:6]
    (distinct, row_regimes) = row[6:] if len(row) > 6 else (None, None)
    regimes = regimes or row_regimes or list(vc.REGIMES)
    done = []
    for regime in regimes:
        (op, csr, has_last) = make(vc.variant_of(regime))
        per_row = vc.per_row_of(csr[1])
        (X, Xd, src) = _regime_block(regime, csr[0][1], n, has_last, per_row, _seed(tag, regime), distinct)
        ref = _oracle(csr, Xd)
        print('  %-34s %-11s n=%-3d rows of ~%-6.0f reference: %s' % (tag, regime, n, per_row, vc.share_text(ref)))
        missed = vc.floors_missed(regime, ref)
        assert not missed, (tag, regime, missed, vc.share_text(ref))
        ref = np.ascontiguousarray(ref[:, src])
        (xd, ld, start) = _window(X, window)
        for relu in (0, RELU):
            (win, whole, plan) = _spmm(op, xd, n, flags | relu, ld=ld, start=start)
            for t in texts:
                assert t in plan, (tag, regime, t, plan)
            torch.cuda.synchronize()
            vc.assert_bits_equal(win.cpu().numpy(), vc.relu_ref(ref) if relu else ref, '%s, %s, relu=%d, %s' % (tag, regime, relu, plan[:120]))
            if window:
                assert _outside_intact(whole, n, start), (tag, regime, relu)
        done.append(regime)
    return done


@pytest.mark.parametrize('row', FAMILIES, ids=[r[0] for r in FAMILIES])
def test_bit_exact_family(row):
    done = _run_family(row)
    assert done == list(row[7] if len(row) > 6 else vc.REGIMES) and set(done) & set(vc.FLUSH_REGIMES)


def test_planes():
    """kn_spmm_planes on the loose-rows operator: three planes of three regimes in one launch, each plane against the oracle."""
    regimes = ('subnormal', 'by-column', 'signed-zero')
    (n, ld) = (64, 72)
    made = [_lo(lo.loose_csr)(vc.variant_of(r)) for r in regimes]
    # one launch applies ONE operator: the planes share the `unit` values of the first two regimes; the third plane's integers meet them as they are
    (op, csr, _) = made[0]
    assert vc.variant_of('subnormal')[0] == vc.variant_of('by-column')[0] == 'unit'
    (rows, cols) = csr[0]
    xb = torch.full((3, cols, ld), float('nan'), dtype=torch.float32, device=dev())
    yb = torch.full((3, rows, ld), SENTINEL, dtype=torch.float32, device=dev())
    refs = []
    for (p, r) in enumerate(regimes):
        (X, Xd, src) = _regime_block(r, cols, n, False, vc.per_row_of(csr[1]), _seed('planes', r))
        xb[p, :, 4:4 + n] = torch.as_tensor(X).to(dev())
        refs.append(np.ascontiguousarray(_oracle(csr, Xd)[:, src]))
    with torch.cuda.device(dev()):
        assert 'csr_rows_kernel' in op.plan(n, EXACT, ldx=ld, ldy=ld)
        for relu in (0, RELU):
            yb.fill_(SENTINEL)
            assert op.spmm_planes(xb.data_ptr() + 16, ld, cols * ld, 3, n, yb.data_ptr() + 16, ld, rows * ld, EXACT | relu, torch.cuda.current_stream().cuda_stream) is True
            torch.cuda.synchronize()
            for (p, r) in enumerate(regimes):
                vc.assert_bits_equal(yb[p, :, 4:4 + n].cpu().numpy(), vc.relu_ref(refs[p]) if relu else refs[p], 'plane %d (%s), relu=%d' % (p, r, relu))
                assert _outside_intact(yb[p], n, 4)


# ---- the whole-net kernel ---------------------------------------------------------------------------------------------------------------------------------

def _chains():
    """Three- to five-layer chains, one per layout choice of test_parity_gpu.test_whole_net_kernel_layout_choices_vs_oracle that differs in how a layer's values and
    columns are walked: pattern pools in LDS with keyed Linears on the sequential thin walk behind them, a Linear first (the staged-pool thin walk), two rows per lane
    with pools staged a layer early, and columns from memory."""
    rng = np.random.RandomState(77)
    (g, d, dp) = (lambda *a: _chain_grouped(rng, *a), lambda *a: _chain_dense(rng, *a), lambda *a: _chain_dense_plus(rng, *a))
    return [
        ('lds-pools+sequential-linears', [((645, 200), g(645, 200, 6, 11, 5), 1), ((131, 645), g(131, 645, 16, 50, 2), 0), ((121, 131), dp(121, 131, 1), 1), ((85, 121), dp(85, 121, 3), 1),
                                          ((11, 85), dp(11, 85, 1), 0)], '5 operators (3 on the thin walk -- 3 of them sequentially, 2 with column patterns in LDS)'),
        ('linear-first', [((70, 130), d(70, 130), 1), ((40, 70), dp(40, 70, 1), 1), ((10, 40), dp(10, 40, 1), 0)], '3 operators (2 on the thin walk -- 1 of them sequentially, 1 with column patterns in LDS)'),
        ('two-rows-per-lane', [((2051, 300), g(2051, 300, 6, 11, 5), 1), ((1300, 2051), g(1300, 2051, 1, 7, 0), 0), ((1609, 1300), g(1609, 1300, 16, 50, 9), 1), ((90, 1609), d(90, 1609), 1),
                               ((10, 90), d(10, 90), 0)], '2 with two rows per lane, 2 column pools staged a layer early'),
        ('columns-from-memory', [((4100, 4200), g(4100, 4200, 6, 110, 2), 1), ((64, 4100), g(64, 4100, 8, 9, 0), 1), ((30, 64), d(30, 64), 0)], '(1 on the thin walk'),
    ]


_CHAINS = []
OVERFLOW_TARGETS = (-3, 0)


def _calibrated(layers, base, targets):
    """[(shape, indptr, indices, data, relu)]: `unit` values times the power of two that puts the layer's output, on the unscaled block `base` (the block the regime
    then scales: same seed, same first draw), at a root mean square in [2^t, 2^(t+1)) -- t = targets[0] for the inner layers, targets[1] for the last."""
    (mats, y) = ([], base)
    for (li, (shape, (ip, ix, dt), relu)) in enumerate(layers):
        dv = vc.csr_values(('unit', 0), shape, ip, ix, dt)
        out = _oracle((shape, ip, ix, dv), y)
        if relu:
            out = vc.relu_ref(out)
        e = targets[li == len(layers) - 1] - int(np.floor(np.log2(np.sqrt(np.mean(out.astype(np.float64) ** 2)))))
        mats.append((shape, ip, ix, dv * np.float32(2.0) ** e, relu))
        y = out * np.float32(2.0) ** e
    return mats


@pytest.mark.parametrize('which', range(4), ids=['lds-pools+sequential-linears', 'linear-first', 'two-rows-per-lane', 'columns-from-memory'])
def test_whole_net_kernel(which):
    """The layers carry `unit` values with one more power of two per layer, found on the host from the oracle's own activations of the unscaled block, that keeps
    every layer's output at a root mean square in [1/2, 1): the activations stay in their regime from layer to layer, ReLUs or not.  Under `overflow` the inner
    layers stay at [1/8, 1/4) and the LAST one takes the first further power of two at which the REFERENCE meets the regime's floors, so the block reaches it finite and overflows there.  The floors hold on the last layer's reference."""
    if not _CHAINS:
        _CHAINS.extend(_chains())
    (tag, layers, want) = _CHAINS[which]
    n = 37
    for regime in vc.F32_CHAIN_REGIMES:
        seed = _seed(tag, regime)
        mats = _calibrated(layers, np.random.RandomState(seed).randn(layers[0][0][1], n).astype(np.float32), OVERFLOW_TARGETS if regime == 'overflow' else (-1, -1))
        (X, Xd, src) = _regime_block(regime, layers[0][0][1], n, False, vc.per_row_of(layers[0][1][0]), seed)
        for more in range(6 if regime == 'overflow' else 1):
            ref = Xd
            for (shape, ip, ix, dv, relu) in mats:
                ref = _oracle((shape, ip, ix, dv), ref)
                if relu:
                    ref = vc.relu_ref(ref)
            if not vc.floors_missed(regime, ref):
                break
            mats[-1] = mats[-1][:3] + (mats[-1][3] * np.float32(2.0), mats[-1][4])
        print('  chain %-30s %-10s last layer: %s' % (tag, regime, vc.share_text(ref)))
        missed = vc.floors_missed(regime, ref)
        assert not missed, (tag, regime, missed, vc.share_text(ref))
        ref = np.ascontiguousarray(ref[:, src])
        xd = torch.as_tensor(X).to(dev())
        yd = torch.full((layers[-1][0][0], n), SENTINEL, dtype=torch.float32, device=dev())
        with torch.cuda.device(dev()):
            ops = [C.Operator.csr(shape, ip, ix, dv) for (shape, ip, ix, dv, relu) in mats]
            chain = C.Operator.chain(ops, [m[4] for m in mats])
            plan = chain.plan(n)
            assert 'chain_kernel' in plan and want in plan, plan
            chain.spmm(xd.data_ptr(), n, n, yd.data_ptr(), n, EXACT, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        vc.assert_bits_equal(yd.cpu().numpy(), ref, 'chain %s, %s' % (tag, regime))


# ---- float64 ----------------------------------------------------------------------------------------------------------------------------------------------

_F64 = {}


def _f64_operator(variant, scale_exp=0):
    """4 200 rows of 1 .. 9 stored entries (unsorted, duplicates) in float64: enough rows for csr_rows_f64_kernel<vec=4> at 256 columns and <vec=2> at 128."""
    key = (variant, scale_exp)
    if key not in _F64:
        rng = np.random.RandomState(64)
        (m, nc) = (4200, 300)
        lens = rng.randint(1, 10, m)
        ip = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
        ix = rng.randint(0, nc, int(ip[-1])).astype(np.int32)
        dt = vc.csr_values(variant, (m, nc), ip, ix, rng.randn(len(ix))) * 2.0 ** scale_exp
        with torch.cuda.device(dev()):
            _F64[key] = (C.Operator.csr((m, nc), ip, ix, dt), ((m, nc), ip, ix, dt))
    return _F64[key]


def _f64_both_outputs(op, csr, X, ref64, n, vec, what):
    """kn_spmm (the float64 sum rounded to float32 ONCE) and kn_spmm_f64 (the float64 block itself), ReLU off and on."""
    xd = torch.as_tensor(X).to(dev())
    with np.errstate(all='ignore'):
        ref32 = ref64.astype(np.float32)
        relu32 = vc.relu_ref(ref64).astype(np.float32)                  # the ReLU acts on the float64 block, the rounding follows: a tiny negative sum becomes +0.0, not -0.0
    with torch.cuda.device(dev()):
        plan = op.plan(n, EXACT)
        assert 'csr_rows_f64_kernel<vec=%d,' % vec in plan, plan
        st = torch.cuda.current_stream().cuda_stream
        for relu in (0, RELU):
            y32 = torch.full((csr[0][0], n), SENTINEL, dtype=torch.float32, device=dev())
            y64 = torch.full((csr[0][0], n), SENTINEL, dtype=torch.float64, device=dev())
            op.spmm(xd.data_ptr(), n, n, y32.data_ptr(), n, EXACT | relu, st)
            op.spmm_f64(xd.data_ptr(), n, n, y64.data_ptr(), n, EXACT | relu, st)
            torch.cuda.synchronize()
            vc.assert_bits_equal(y64.cpu().numpy(), vc.relu_ref(ref64) if relu else ref64, '%s, float64 output, relu=%d' % (what, relu))
            vc.assert_bits_equal(y32.cpu().numpy(), relu32 if relu else ref32, '%s, float32 output, relu=%d' % (what, relu))
    return ref32


@pytest.mark.parametrize('n,vec', [(64, 1), (128, 2), (256, 4)])
def test_f64_kernel_in_the_f32_regimes(n, vec):
    """The f32 regimes on a float64 operator.  (a): under `subnormal` / `underflow` the float64 sums are far inside float64's normal range and round ONCE into
    float32's subnormal range; under `overflow` they lie beyond FLT_MAX: finite in the float64 block, Inf in the float32 block."""
    for regime in vc.REGIMES:
        (op, csr) = _f64_operator(vc.variant_of(regime))
        (X, Xd, src) = _regime_block(regime, csr[0][1], n, False, vc.per_row_of(csr[1]), _seed('f64', regime, n))
        ref64 = _oracle(csr, Xd)
        assert ref64.dtype == np.float64
        ref32 = _f64_both_outputs(op, csr, X, np.ascontiguousarray(ref64[:, src]), n, vec, 'f64 operator, %s, n=%d' % (regime, n))
        (s64, s32) = (vc.shares(ref64), vc.shares(ref32))
        print('  f64 %-11s n=%-3d float64 block: %s | rounded once: %s' % (regime, n, vc.share_text(ref64), vc.share_text(ref32)))
        assert not vc.floors_missed(regime, ref32), (regime, vc.share_text(ref32))
        if regime in ('subnormal', 'underflow'):
            assert s64['subnormal'] == 0 and s32['subnormal'] >= 0.7
        if regime == 'overflow':
            assert s32['inf'] >= 0.2 and s64['inf'] < 0.5 * s32['inf']              # sums beyond FLT_MAX that are finite in float64


@pytest.mark.parametrize('n,vec', [(64, 1), (256, 4)])
def test_f64_kernel_exact_ties(n, vec):
    """(b) rows whose float64 sum lies exactly halfway between two float32 neighbours: (1 + m 2^-23) x + 2^-24 x for a power of two x, with the lower neighbour's last
    bit m & 1 odd (the tie goes up) and even (it goes down), at magnitudes from float32's subnormal range to its top binade, both signs."""
    ms = [0, 1, 2, 3, 0x7ffffe, 0x7fffff, 0x2aaaaa, 0x555555]
    m_rows = 4200                                                       # (enough rows for the <vec=4> launch)
    (ip, ix, dt) = ([0], [], [])
    for r in range(m_rows):
        m = ms[r % len(ms)]
        ix.extend([r % 7, r % 7])
        dt.extend([1.0 + m * 2.0 ** -23, 2.0 ** -24])
        ip.append(len(ix))
    csr = ((m_rows, 7), np.array(ip, np.int32), np.array(ix, np.int32), np.array(dt, np.float64))
    exps = np.array([-149 + 24, -140, -126, -1, 0, 1, 60, 127])        # 2^-125 (1 + ...) ... the tie's lower neighbour is normal, from -140 on the sum is a float32 subnormal's tie
    src = _columns(n)
    Xd = np.zeros((7, int(src.max()) + 1), dtype=np.float32)
    for c in range(Xd.shape[1]):
        Xd[:, c] = np.ldexp(np.float32(1.0), exps[(np.arange(7) + c) % len(exps)]) * (-1.0 if c % 3 == 1 else 1.0)
    ref64 = _oracle(csr, Xd)
    with np.errstate(all='ignore'):
        r32 = ref64.astype(np.float32)
    normal = np.abs(r32) >= np.finfo(np.float32).tiny
    tie = (np.ascontiguousarray(ref64).view(np.uint64) & np.uint64((1 << 29) - 1)) == np.uint64(1 << 28)
    assert tie[normal & np.isfinite(r32)].all() and normal.mean() > 0.5          # the float64 sums ARE ties wherever float32 keeps 24 bits
    up = (r32.astype(np.float64) > ref64) == (ref64 > 0)
    assert up[normal].any() and (~up[normal]).any()                              # both directions occur
    with torch.cuda.device(dev()):
        op = C.Operator.csr(*csr)
    X = np.ascontiguousarray(Xd[:, src])
    _f64_both_outputs(op, csr, X, np.ascontiguousarray(ref64[:, src]), n, vec, 'exact ties, n=%d' % n)


@pytest.mark.parametrize('n,vec', [(64, 1), (128, 2)])
def test_f64_kernel_subnormal_products(n, vec):
    """(c) operator values near 2^-920 against subnormal f32 activations (2^-130): products and sums near 2^-1050, float64 subnormals (values near 2^-1000 would
    put every product below float64's last subnormal, 2^-1074).  The float64 block holds them; the float32 block is +0.0 / -0.0 as the one rounding gives it."""
    (op, csr) = _f64_operator(('unit', 0), scale_exp=-920)
    (X, Xd, src) = _regime_block('subnormal', csr[0][1], n, False, vc.per_row_of(csr[1]), _seed('f64-sub', n))
    ref64 = _oracle(csr, Xd)
    print('  f64 subnormal products n=%d: %s' % (n, vc.share_text(ref64)))
    assert vc.shares(ref64)['subnormal'] >= 0.9
    ref32 = _f64_both_outputs(op, csr, X, np.ascontiguousarray(ref64[:, src]), n, vec, 'f64-subnormal products, n=%d' % n)
    assert np.all(ref32 == 0) and np.signbit(ref32).any() and (~np.signbit(ref32)).any()


# ---- the screen slot --------------------------------------------------------------------------------------------------------------------------------------

SCREEN = [r for r in FAMILIES if r[0] in ('csr_rows<4>-loose', 'csr_rows_pair', 'csr_group', 'convtaps_exact_pipe-128-tiles')]


@pytest.mark.parametrize('row', SCREEN, ids=[r[0] for r in SCREEN])
def test_screen_slot_bit_pattern(row):
    """kn_spmm_screen: the slot's bit pattern is that of max |Y| over the reference's non-NaN elements -- a subnormal maximum is reported as one, Inf counts --
    whether it rides in the kernel's epilogue (loose rows) or comes from the pass over Y (groups, the order-preserving conv pipeline)."""
    (tag, make, n, flags, texts, window) = row[:6]
    for regime in ('subnormal', 'by-column', 'overflow'):
        (op, csr, has_last) = make(vc.variant_of(regime))
        (X, Xd, src) = _regime_block(regime, csr[0][1], n, has_last, vc.per_row_of(csr[1]), _seed(tag, regime))
        ref = np.ascontiguousarray(_oracle(csr, Xd)[:, src])
        (xd, ld, start) = _window(X, window)
        for relu in (0, RELU):
            r = vc.relu_ref(ref) if relu else ref
            want = np.abs(r[~np.isnan(r)]).max().astype(np.float32)
            slot = torch.zeros(1, dtype=torch.float32, device=dev())
            (win, whole, plan) = _spmm(op, xd, n, flags | relu, ld=ld, start=start, absmax=slot)
            torch.cuda.synchronize()
            vc.assert_bits_equal(win.cpu().numpy(), r, '%s, %s, relu=%d (screen call)' % (tag, regime, relu))
            vc.assert_bits_equal(slot.cpu().numpy(), np.array([want]), '%s, %s, relu=%d: slot (max |Y| is %s)' % (tag, regime, relu, vc.class_of(want)))
        if regime == 'subnormal' and not has_last:                      # (a homogeneous row hands its 1.0 on: the maximum of such a block)
            assert vc.class_of(want) == 'subnormal'
        if regime == 'overflow':
            assert vc.class_of(want) == 'inf'


# ---- tolerance kernels: exact covariance with a power-of-two scale ------------------------------------------------------------------------------------------

TOLERANCE_ROWS = [r for r in cc.ROWS if not r[6]]


def _covariant(call, X, what):
    """Y(2^k X) == 2^k Y(X) under bits_equal for k = -40, +40, and the same for the screen slot.  call(xd, slot) -> y on the device."""
    xd = torch.as_tensor(np.ascontiguousarray(X)).to(dev())
    s0 = torch.zeros(1, dtype=torch.float32, device=dev())
    y0 = call(xd, s0).clone()
    torch.cuda.synchronize()
    (y0, s0) = (y0.cpu().numpy(), s0.cpu().numpy())
    big = float(np.abs(y0).max())
    tiny = np.abs(y0[y0 != 0]).min()
    assert np.isfinite(y0).all() and big < 2.0 ** 80 and tiny > 2.0 ** -80, (what, big, tiny)     # nothing under- or overflows at |k| = 40
    assert s0[0] == np.float32(big)
    for k in (-40, 40):
        f = np.float32(2.0) ** k
        sk = torch.zeros(1, dtype=torch.float32, device=dev())
        yk = call(xd * float(f), sk).clone()
        torch.cuda.synchronize()
        vc.assert_bits_equal(yk.cpu().numpy(), y0 * f, '%s, k=%d' % (what, k))
        vc.assert_bits_equal(sk.cpu().numpy(), s0 * f, '%s, k=%d: screen slot' % (what, k))


@pytest.mark.parametrize('row', TOLERANCE_ROWS, ids=['%s-n%d%s-f%d%s' % (r[0], r[1], '-ldy+%d' % r[2] if r[2] else '', r[3], '-' + r[4] if r[4] else '') for r in TOLERANCE_ROWS])
def test_tolerance_kernels_commute_with_a_power_of_two(row):
    """Every launch site of test_conv_choice_gpu.ROWS that runs under the float-key tolerance (matrix-core tiles at every loader, the small-K pair, bf16x3, the
    matrix-core narrow kernel): with the WHOLE block scaled by 2^k, homogeneous row included, the result is 2^k times the unscaled one bit for bit -- fma chains,
    the three-way bf16 split, the ordered split-K reduction and lastcol * x_last all commute with a power of two while nothing under- or overflows.  No tolerance:
    an absolute epsilon, a clamp, a flush or a bias added as a constant would all show."""
    (name, n, pad, flags, switch, text, exact_bits) = row
    (op, csr) = cc._operator(name, switch)
    (X, xd, ref) = cc._reference(name, n)
    plans = []

    def call(x, slot):
        (y, whole, plan) = _spmm(op, x, n, flags, ld=n + pad, absmax=slot)
        plans.append(plan)
        return y
    _covariant(call, np.ascontiguousarray(X.T), '%s n=%d flags=%d' % (name, n, flags))
    assert all(text in p for p in plans), plans[0]


def test_dense_handle_commutes_with_a_power_of_two():
    c = lo.dense_case()
    n = 256
    X = np.random.RandomState(12).randn(c.shape[1], n).astype(np.float32)
    X[-1] = 1.0
    plans = []

    def call(x, slot):
        (y, whole, plan) = _spmm(c.op, x, n, 0, absmax=slot)
        plans.append(plan)
        return y
    _covariant(call, X, 'kn_dense_create handle')
    assert all('dense_reduce_kernel' in p for p in plans), plans[0]
    lo.dense_case.cache_clear()


# ---- whole models -----------------------------------------------------------------------------------------------------------------------------------------

def _scaled_cipher(z, k, n=None):
    x = np.array(z['x_cipher'], dtype=np.float32, copy=True)
    if n is not None:
        x = np.ascontiguousarray(x[np.arange(n) % x.shape[0]])
    with np.errstate(all='ignore'):
        x[:, :-1] *= np.float32(2.0) ** k
    assert np.all(x[:, -1] == 1.0)
    return x


@pytest.mark.parametrize('k', [-128, -120, 120])
def test_lenet_permutation_keynet_at_scaled_inputs(golden, k):
    """tests/golden/lenet_perm.npz (forward_linear runs the whole-net kernel) on x_cipher * 2^k with the homogeneous column kept at 1: every layer, walked with the
    layer's own forward, and the logits of forward_linear equal oracle.keynet_forward under bits_equal."""
    from keynet_amd import system as ksys
    z = golden('lenet_perm.npz')
    knet = kio.keynet_from_arrays(z)
    x = _scaled_cipher(z, k)
    with np.errstate(all='ignore'):
        (last, outs) = oracle.keynet_forward(oracle.load_golden_layers(z), x, collect=True)
    y = torch.as_tensor(x).to(dev())
    for (lname, child) in knet._keynet.named_children():
        y = child.forward(y) if isinstance(child, KeyedLayer) else ksys._relu_block(y)
        vc.assert_bits_equal(y.cpu().numpy(), np.ascontiguousarray(outs[lname], dtype=np.float32), 'lenet, 2^%d, layer %s' % (k, lname))
    print('  lenet 2^%d: first keyed layer %s | logits %s' % (k, vc.share_text(outs[[str(v) for v in z['layer_names']][0]]), vc.share_text(last)))
    out = knet.forward_linear(torch.as_tensor(x).to(dev()))
    vc.assert_bits_equal(out.cpu().numpy(), np.ascontiguousarray(last, dtype=np.float32), 'lenet, 2^%d, forward_linear' % k)


@pytest.mark.parametrize('k', [-128, -120, 120])
def test_tiled_permutation_keynet_at_scaled_inputs(golden, k):
    """tests/golden/mini_tiled_permutation.npz (per-layer kernels) on x_cipher * 2^k: every keyed layer on the order-preserving kernels (exact=True) from the oracle's
    own previous-layer output, and the logits of the narrow keyword sets at 1 and 8 images (bit-exact forwards: tests/test_narrow_gpu.py), equal to the oracle under
    bits_equal.  (The default contract of this net puts its conv layers on the matrix cores, inside the float-key tolerance: no bit pattern is promised there.)"""
    z = golden('mini_tiled_permutation.npz')
    knet = kio.keynet_from_arrays(z)
    layers = oracle.load_golden_layers(z)
    x = _scaled_cipher(z, k)
    with np.errstate(all='ignore'):
        (last, outs) = oracle.keynet_forward(layers, x, collect=True)
    prev = x
    for (lname, child) in knet._keynet.named_children():
        if isinstance(child, KeyedLayer):
            xin = torch.as_tensor(prev).to(dev())
            if isinstance(child.W, ksp.Conv2dTiledMatrix):            # (as test_parity_gpu.test_tiled_keynet_layers reaches the order-preserving path of a tiled conv layer)
                y = child.W.torchdot(xin.t(), exact=True).t()
                if 'ReLU' in str(z['L.%s.layertype' % lname]):
                    y = torch.relu(y)
            else:
                y = child.forward(xin)
            vc.assert_bits_equal(np.ascontiguousarray(y.cpu().numpy()), np.ascontiguousarray(outs[lname], dtype=np.float32), 'tiled net, 2^%d, layer %s' % (k, lname))
        prev = np.ascontiguousarray(outs[lname], dtype=np.float32)
    for (n, kw) in ((1, dict(narrow=True)), (8, dict(narrow=True)), (8, dict(narrow=True, narrow_rows=True)), (1, dict(narrow=True, narrow_taps=True)), (8, dict(narrow=True, narrow_taps=True))):
        xn = _scaled_cipher(z, k, n)
        with np.errstate(all='ignore'):
            ref = oracle.keynet_forward(layers, xn)
        out = knet.forward_linear(torch.as_tensor(xn).to(dev()), **kw)
        vc.assert_bits_equal(out.cpu().numpy(), np.ascontiguousarray(ref, dtype=np.float32), 'tiled net, 2^%d, %d images, %r' % (k, n, kw))
