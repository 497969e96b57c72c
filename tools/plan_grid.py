"""Dispatch grid of the conv-taps host side: which kernel kn_spmm would launch for which call, as text.

Loads the library named by KEYNET_HIP_LIB (default: the product library) through keynet_amd/_capi.py WITHOUT torch, creates a fixed list of operators and
prints, per operator, kn_nnz / kn_nnz_expanded / a hash of kn_export_csr and one line per (n_vecs, ldx = ldy, flags) with the text of kn_spmm_plan; the
batches include 1, 2, 3, 4, 8 and 9 columns and the flags the three narrow ones (KN_FLAG_NARROW, _MFMA, _ROWS), and three float32 CSR operators close the list.  Nothing is
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


def report(name, op, out, export=True):
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
            for fl in FLAGS:
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


def main():
    out = sys.stdout
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


if __name__ == '__main__':
    main()
