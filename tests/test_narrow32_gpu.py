"""The low-latency forward for 9 .. 32 images on the GPU (narrow32=True, KN_FLAG_NARROW32): convtaps_narrow32_kernel against the CPU oracle, the 128-column
order-preserving kernels and convtaps_narrow_kernel on column chunks -- bit for bit --; convtaps_narrow_mfma_kernel at NV = 16 | 32 against the oracle under the
criterion of the wide matrix-core kernels and, bit for bit, against itself on chunks of at most 8 columns; the modifier's semantics through the C ABI; and
KeyedModel.forward_linear / capture with the keyword."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from keynet_amd import io as kio
from keynet_amd import sparse as ksp
from keynet_amd import _capi
from keynet_amd.layer import KeyedLayer, gate
from test_parity_gpu import _random_convtaps, close_conditioned, dev
from test_narrow_gpu import SHAPES as NARROW_SHAPES, _build, _oracle, _sorted_csr
from test_narrow_mfma_gpu import SHAPES as MFMA_SHAPES
from narrow_helpers import SENTINEL, _spmm
from fuzz_nets import random_net
from keynet_amd import system as ksys

pytestmark = pytest.mark.gpu

(RELU, EXACT, BF16X3, NARROW, MFMA, ROWS, N32) = (_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_BF16X3, _capi.KN_FLAG_NARROW, _capi.KN_FLAG_NARROW_MFMA,
                                                  _capi.KN_FLAG_NARROW_ROWS, _capi.KN_FLAG_NARROW32)
KERNEL = 'convtaps_narrow32_kernel'
LANE = 'convtaps_narrow_kernel'
MFMA_KERNEL = 'convtaps_narrow_mfma_kernel'
KN_ERR_UNSUPPORTED = 6                # enum kn_status, include/keynet_hip.h
WIDTHS = [9, 15, 16, 17, 31, 32]

# nine output pixels (6 x 6 input, stride 2): an odd pixel count leaves a half-empty 32-column tile at NV = 32 and a quarter tile at NV = 16; 70 channels = one
# full 64-channel block and six lanes of the next
NINE = [('nine-pixels-cin5-cout70-bias', 5, 70, 6, 3, 2, True, True), ('nine-pixels-cin5-cout70-coef-bias', 5, 70, 6, 3, 2, False, True)]
SHAPES = NARROW_SHAPES + NINE
SHAPES_MFMA = MFMA_SHAPES + NINE
_cache = {}


def _case(case):
    """(W, sorted expansion, X [cols, 128], X on the device, the 128-column order-preserving result) of a case, built once."""
    if case[0] not in _cache:
        (W, M, X, _) = _build(case)
        xd = torch.as_tensor(X).to(dev())
        _cache[case[0]] = (W, M, X, xd, W.torchdot(xd, exact=True))
    return _cache[case[0]]


def _chunks(n):
    return [(lo, min(lo + 8, n)) for lo in range(0, n, 8)]


@pytest.mark.parametrize('n_vecs', WIDTHS)
@pytest.mark.parametrize('case', SHAPES, ids=[c[0] for c in SHAPES])
def test_narrow32_kernel_against_the_oracle_the_128_column_kernels_and_the_narrow_kernel(case, n_vecs):
    (W, M, X, xd, y128) = _case(case)
    if case in NINE:
        assert W.shape == (631, 181)
    with torch.cuda.device(dev()):
        plan = W._device_op(dev()).plan(n_vecs, NARROW | N32)
    assert KERNEL in plan and LANE not in plan and 'NV=' in plan and 'column block' in plan, plan
    if case[0].startswith('filled'):
        assert 'stored values summed' in plan, plan
    ref = _oracle(M, X[:, :n_vecs])
    x = xd[:, :n_vecs]
    for relu in (False, True):
        y = W.torchdot(x, relu=relu, exact=True, narrow=True, narrow32=True).cpu().numpy()
        assert np.array_equal(y, np.maximum(ref, 0) if relu else ref), (case[0], n_vecs, relu, float(np.abs(y - ref).max()))
    y = W.torchdot(x, exact=True, narrow=True, narrow32=True)
    assert torch.equal(y, y128[:, :n_vecs])
    for (lo, hi) in _chunks(n_vecs):
        assert torch.equal(y[:, lo:hi], W.torchdot(x[:, lo:hi], exact=True, narrow=True)), (lo, hi)


# (Cin, Cout, H, columns, unit coefficients, bias column, float coefficients on the unit operator's own entries) -> the form the launcher's rule gives it:
# (NV, stored values summed, coefficients, a block the batch does not fill).  Layers with 4 096 (pixel, channel block) items keep the width's form, 2 304 items run
# two blocks of 16 for 32 columns, a small layer blocks of 8 -- unless its taps exceed 2 MB (256 -> 256 channels, 3 x 3: 2.4 MB), which keeps the width's form; operators
# that sum stored values run at most 16 columns per block; without a bias column the masked forms walk their last pixels one column per lane.
FORMS = [
    ((3, 64, 64, 32, True, True, False), (32, False, False, False)),
    ((3, 64, 64, 20, True, False, False), (32, False, False, True)),
    ((3, 64, 64, 16, True, True, False), (16, False, False, False)),
    ((3, 64, 64, 12, True, False, False), (16, False, False, True)),
    ((3, 64, 64, 32, True, True, True), (32, False, True, False)),
    ((4, 64, 48, 32, True, False, True), (16, False, True, False)),
    ((4, 64, 48, 13, True, False, True), (8, False, True, True)),
    ((3, 64, 48, 32, False, True, False), (16, True, True, False)),
    ((3, 64, 48, 25, False, False, False), (16, True, True, True)),
    ((5, 70, 6, 32, True, True, False), (8, False, False, False)),
    ((256, 256, 6, 32, True, True, False), (32, False, False, False)),
    ((256, 256, 6, 11, True, False, False), (16, False, False, True)),
]


@pytest.mark.parametrize('shape,form', FORMS, ids=['cin%d-%dx%d-%d-NV=%d%s%s%s' % (s[0], s[2], s[2], s[3], f[0], '-summed' if f[1] else '', '-coef' if f[2] else '', '-masked' if f[3] else '') for (s, f) in FORMS])
def test_every_form_of_the_kernel_gives_the_oracles_bits(shape, form):
    (Cin, Cout, H, n, unit, has_last, recoef) = shape
    rng = np.random.RandomState(11)
    W = _random_convtaps(rng, Cin, Cout, H, 3, 1, unit, has_last)
    if recoef:
        t = W._taps
        W = ksp.Conv2dTiledMatrix.fromtaps(W._inshape, W._outshape, t['taps'], t['ent_out'], t['ent_in'], t['ent_tap'], (rng.rand(len(t['ent_out'])) + 0.5).astype(np.float32), t['lastcol'])
    X = rng.randn(W.shape[1], n).astype(np.float32)
    if has_last:
        X[-1] = 1.0
    with torch.cuda.device(dev()):
        plan = W._device_op(dev()).plan(n, NARROW | N32 | RELU)
    assert KERNEL in plan, plan
    seen = (int(plan[plan.index('NV=') + 3:].split(',')[0]), 'stored values summed' in plan, ', coef' in plan, 'masked to' in plan)
    assert seen == form, plan
    y = W.torchdot(torch.as_tensor(X).to(dev()), relu=True, exact=False, narrow=True, narrow32=True).cpu().numpy()
    ref = np.maximum(_oracle(_sorted_csr(W), X), 0)
    assert np.array_equal(y, ref), (plan, float(np.abs(y - ref).max()))


@pytest.mark.parametrize('n_vecs', WIDTHS)
@pytest.mark.parametrize('case', SHAPES_MFMA, ids=[c[0] for c in SHAPES_MFMA])
def test_matrix_core_kernel_at_16_and_32_columns(case, n_vecs):
    (W, M, X, xd, _) = _case(case)
    with torch.cuda.device(dev()):
        plan = W._device_op(dev()).plan(n_vecs, MFMA | N32)
    assert MFMA_KERNEL in plan and KERNEL not in plan and ('NV=%d' % (16 if n_vecs <= 16 else 32)) in plan, plan
    ref = _oracle(M, X[:, :n_vecs])
    x = xd[:, :n_vecs]
    for relu in (False, True):
        y = W.torchdot(x, relu=relu, exact=False, narrow='mfma', narrow32=True)
        assert torch.equal(y, W.torchdot(x, relu=relu, exact=False, narrow='mfma', narrow32=True)), (case[0], n_vecs, relu)
        for (lo, hi) in _chunks(n_vecs):
            assert torch.equal(y[:, lo:hi], W.torchdot(x[:, lo:hi], relu=relu, exact=False, narrow='mfma')), (case[0], n_vecs, relu, lo, hi)
        r = np.maximum(ref, 0) if relu else ref
        y = y.cpu().numpy()
        print(case[0], n_vecs, relu, 'max |d| = %.3g' % float(np.abs(y - r).max()))
        assert close_conditioned(y.T, r.T, (M.shape, M.indptr, M.indices, M.data), X[:, :n_vecs].T), (case[0], n_vecs, relu, float(np.abs(y - r).max()))


def test_flag_semantics():
    """The modifier alone, on at most 8 columns and on 33 columns: the plan and bits of the call without it.  With KN_FLAG_EXACT the matrix-core request is the
    channel-lane narrow32 kernel bit for bit; so is the filled-in operator's.  CSR, dense and float64 handles ignore it; a handle that never saw the flag plans
    and computes the same without it."""
    (W, M, X, _) = _build(('semantics', 16, 64, 8, 3, 1, True, True), seed=9)
    xd = torch.as_tensor(X).to(dev())
    with torch.cuda.device(dev()):
        op = W._device_op(dev())
        t = W._taps
        op2 = _capi.Operator.convtaps(W._inshape, W._outshape, t['taps'], t['ent_out'], t['ent_in'], t['ent_tap'], t['ent_coef'], t['lastcol'])
    for n in (1, 5, 8, 9, 16, 32, 33, 64):
        for flags in (0, EXACT, RELU, BF16X3):                               # alone
            (y1, _, p1) = _spmm(op, xd, n, flags | N32)
            (y0, _, p0) = _spmm(op, xd, n, flags)
            assert p1 == p0 and KERNEL not in p1 and torch.equal(y1, y0), (n, flags, p1, p0)
    for n in (1, 5, 8, 33, 64):
        for flags in (NARROW, MFMA, NARROW | EXACT, MFMA | RELU, NARROW | BF16X3):
            (y1, _, p1) = _spmm(op, xd, n, flags | N32)
            (y0, _, p0) = _spmm(op, xd, n, flags)
            assert p1 == p0 and KERNEL not in p1 and 'NV=16' not in p1 and 'NV=32' not in p1 and torch.equal(y1, y0), (n, flags, p1, p0)
    for n in (9, 16, 20, 32):
        (ye, _, pe) = _spmm(op, xd, n, EXACT | NARROW | N32)
        assert KERNEL in pe, pe
        assert np.array_equal(ye.cpu().numpy(), _oracle(M, X[:, :n]))
        (yx, _, _) = _spmm(op, xd, n, EXACT)
        assert torch.equal(ye, yx)
        for flags in (NARROW, NARROW | BF16X3, MFMA | EXACT, MFMA | EXACT | BF16X3, NARROW | MFMA | EXACT):
            (y, _, p) = _spmm(op, xd, n, flags | N32)
            assert KERNEL in p and MFMA_KERNEL not in p and torch.equal(y, ye), (n, flags, p)
        (yr, _, _) = _spmm(op, xd, n, MFMA | EXACT | RELU | N32)
        assert torch.equal(yr, torch.clamp(ye, min=0))
        (ym, _, pm) = _spmm(op, xd, n, MFMA | N32)
        assert MFMA_KERNEL in pm and KERNEL not in pm, pm
    for n in (1, 8, 16, 32, 64):                                             # without the flag: plan and bits as on a handle that never saw it
        for flags in (0, EXACT, RELU, BF16X3, NARROW, MFMA):
            (ya, _, pa) = _spmm(op, xd, n, flags)
            (yb, _, pb) = _spmm(op2, xd, n, flags)
            assert KERNEL not in pa and pa == pb and torch.equal(ya, yb), (n, flags, pa, pb)
    # the filled-in 9 x 9 operator has no matrix-core narrow form
    filled = [c for c in NARROW_SHAPES if c[0].startswith('filled')][0]
    (Wf, Mf, Xf, xf, yf128) = _case(filled)
    with torch.cuda.device(dev()):
        opf = Wf._device_op(dev())
    for n in (9, 32):
        (y1, _, p1) = _spmm(opf, xf, n, MFMA | N32)
        assert KERNEL in p1 and MFMA_KERNEL not in p1 and torch.equal(y1, yf128[:, :n]), (n, p1)
    # CSR, float64 and dense handles
    import scipy.sparse
    A = scipy.sparse.random(40, 30, density=0.3, format='csr', dtype=np.float32, random_state=3)
    xs = torch.as_tensor(np.random.RandomState(2).randn(30, 32).astype(np.float32)).to(dev())
    with torch.cuda.device(dev()):
        opc = ksp.SparseMatrix(A)._device_op(dev())
    for n in (4, 16):
        for flags in (EXACT, EXACT | NARROW, EXACT | MFMA, EXACT | ROWS, EXACT | NARROW | ROWS):
            (y1, _, p1) = _spmm(opc, xs, n, flags | N32)
            (y0, _, p0) = _spmm(opc, xs, n, flags)
            assert p1 == p0 and torch.equal(y1, y0), (n, flags, p1, p0)
    W64 = ksp.SparseMatrix(A.astype(np.float64))
    assert W64.is_float64()
    with torch.cuda.device(dev()):
        op64 = W64._device_op(dev())
        assert op64.plan(16, EXACT | NARROW | N32) == op64.plan(16, EXACT | NARROW) == op64.plan(16, EXACT)
        (ya, yb) = (torch.empty((40, 16), dtype=torch.float64, device=dev()), torch.empty((40, 16), dtype=torch.float64, device=dev()))
        xc = xs[:, :16].contiguous()
        op64.spmm_f64(xc.data_ptr(), 16, 16, ya.data_ptr(), 16, EXACT | NARROW | N32, torch.cuda.current_stream().cuda_stream)
        op64.spmm_f64(xc.data_ptr(), 16, 16, yb.data_ptr(), 16, EXACT, torch.cuda.current_stream().cuda_stream)
    assert torch.equal(ya, yb)
    Dm = np.random.RandomState(4).randn(ksp.SparseMatrix.DENSE_MIN_ELEMENTS // 4097 + 2, 4097).astype(np.float32)      # a keyed Linear: homogeneous last row
    Dm[-1] = 0
    Dm[-1, -1] = 1
    with torch.cuda.device(dev()):
        opd = ksp.SparseMatrix(scipy.sparse.csr_matrix(Dm))._dense_device_op(dev())
    assert opd is not None
    xdn = torch.as_tensor(np.random.RandomState(5).randn(4097, 16).astype(np.float32)).to(dev())
    (y0, _, p0) = _spmm(opd, xdn, 16, 0)
    for flags in (0, NARROW, MFMA, RELU | NARROW):
        (y1, _, p1) = _spmm(opd, xdn, 16, flags | N32)
        (yf, _, pf) = _spmm(opd, xdn, 16, flags)
        assert p1 == pf and torch.equal(y1, yf), (flags, p1, pf)
        assert flags & RELU or (p1 == p0 and torch.equal(y1, y0))


@pytest.mark.parametrize('flags', [NARROW | N32 | RELU, MFMA | N32 | RELU], ids=['channel-lane', 'matrix-core'])
def test_column_window_of_a_wider_block_through_the_c_abi(flags):
    """Twelve columns at offset 8 of a 1 024-wide block (ldx = ldy = 1024): the window equals the stand-alone result, every other element is untouched."""
    (W, M, X, rng) = _build(('window', 5, 24, 8, 3, 1, False, True), seed=13)
    (ld, c0, n) = (1024, 8, 12)
    Xb = rng.randn(W.shape[1], ld).astype(np.float32)
    Xb[-1] = 1.0
    xb = torch.as_tensor(Xb).to(dev())
    with torch.cuda.device(dev()):
        op = W._device_op(dev())
    (win, yb, plan) = _spmm(op, xb, n, flags, ld=ld, start=c0)
    assert (MFMA_KERNEL if flags & MFMA else KERNEL) in plan, plan
    alone = W.torchdot(xb[:, c0:c0 + n], relu=True, exact=False, narrow='mfma' if flags & MFMA else True, narrow32=True)
    assert torch.equal(win, alone)
    r = np.maximum(_oracle(M, Xb[:, c0:c0 + n]), 0)
    if flags & MFMA:
        assert close_conditioned(alone.cpu().numpy().T, r.T, (M.shape, M.indptr, M.indices, M.data), Xb[:, c0:c0 + n].T)
    else:
        assert np.array_equal(alone.cpu().numpy(), r)
    outside = torch.ones(ld, dtype=torch.bool, device=dev())
    outside[c0:c0 + n] = False
    assert bool(torch.all(yb[:, outside] == SENTINEL))


@pytest.mark.parametrize('n', [9, 17, 20])
@pytest.mark.parametrize('case', [SHAPES[0], SHAPES[1], SHAPES[3], SHAPES[7], NINE[1]], ids=lambda c: c[0])
def test_tight_block_carved_from_a_nan_filled_buffer(case, n):
    """ldx = n: the block's minimal extent.  Everything behind it is NaN, so a masked form that let a surplus sum reach Y, or read beyond the extent into a
    stored sum, shows.  With a bias column the homogeneous row ends the block and every step's segment lies inside it; without one the pixels whose window
    touches the last input row at the last channel take the per-column path.  Outputs finite and the oracle's bits."""
    (W, M, X, _, _) = _case(case)
    (rows, cols) = W.shape
    buf = torch.full((cols * n + 4096,), float('nan'), dtype=torch.float32, device=dev())
    buf[:cols * n].view(cols, n).copy_(torch.as_tensor(X[:, :n]))
    y = torch.full((rows, n), SENTINEL, dtype=torch.float32, device=dev())
    with torch.cuda.device(dev()):
        op = W._device_op(dev())
        plan = op.plan(n, NARROW | N32)
        assert KERNEL in plan and 'masked to %d' % n in plan, plan
        op.spmm(buf.data_ptr(), n, n, y.data_ptr(), n, NARROW | N32, torch.cuda.current_stream().cuda_stream)
    y = y.cpu().numpy()
    assert np.isfinite(y).all()
    assert np.array_equal(y, _oracle(M, X[:, :n])), (case[0], n)


@pytest.mark.parametrize('mode', [True, 'mfma'])
@pytest.mark.parametrize('case', [SHAPES[0], SHAPES[2], NINE[1]], ids=lambda c: c[0])
def test_non_finite_activations_at_16_columns(case, mode):
    """One Inf and one NaN input element reach exactly the outputs whose slot lists hold them."""
    (W, M, X0, _, _) = _case(case)
    rng = np.random.RandomState(21)
    n = 16
    X = X0[:, :n].copy()
    rows = rng.choice(W.shape[1] - 1, size=2, replace=False)
    X[rows[0], 11] = np.nan
    X[rows[1], 3] = np.inf
    ref = _oracle(M, X)
    assert np.isnan(ref).any() and np.isfinite(ref[:, 0]).all() and np.isfinite(ref[:, 11]).any()
    y = W.torchdot(torch.as_tensor(X).to(dev()), exact=False, narrow=mode, narrow32=True).cpu().numpy()
    if mode is True:
        assert np.array_equal(y, ref, equal_nan=True), case[0]
    else:
        assert np.array_equal(np.isfinite(y), np.isfinite(ref)) and bool(np.isnan(y[np.isnan(ref)]).all()), case[0]
        fin = np.isfinite(ref)
        (Xf, yf, rf) = (np.where(np.isfinite(X), X, 0).astype(np.float32), np.where(fin, y, 0), np.where(fin, ref, 0))
        assert close_conditioned(yf.T, rf.T, (M.shape, M.indptr, M.indices, M.data), Xf.T), case[0]


def test_the_size_rule_refuses():
    """(Cin HiWi + 1) * ldx + 32 < 2^31 at 9 .. 32 columns with the modifier: beyond it kn_spmm_plan returns KN_ERR_UNSUPPORTED (no fall-back); the same ldx is
    accepted at 8 columns, where the rule is + 8 with or without the modifier.  No allocation."""
    rng = np.random.RandomState(7)
    W = _random_convtaps(rng, 2, 64, 6, 3, 1, True, True)
    assert W.shape[1] == 73
    ldx = 29417584                                                          # 73 * ldx = 2^31 - 16
    assert 73 * ldx + 8 < (1 << 31) <= 73 * ldx + 32
    buf = ctypes.create_string_buffer(1024)
    with torch.cuda.device(dev()):
        op = W._device_op(dev())
        for flags in (NARROW, MFMA, NARROW | EXACT):
            for n in (9, 16, 32):
                assert _capi.lib().kn_spmm_plan(op.handle, n, ldx, n, flags | N32, buf, 1024) == KN_ERR_UNSUPPORTED, (flags, n)
                assert b'32-bit element offsets' in _capi.lib().kn_last_error()
                assert KERNEL in op.plan(n, flags | N32 | EXACT, ldx=ldx - 1, ldy=n)                                  # the last accepted ldx
                assert op.plan(n, flags, ldx=ldx, ldy=n) == op.plan(n, flags & EXACT, ldx=ldx, ldy=n)      # without the modifier: ignored at 9 columns, nothing refused
            for f in (flags, flags | N32):
                assert 'convtaps_narrow' in op.plan(8, f, ldx=ldx, ldy=8)
            assert _capi.lib().kn_spmm_plan(op.handle, 8, ldx + 1, 8, flags | N32, buf, 1024) == KN_ERR_UNSUPPORTED


def _conv_layers(knet):
    return [(n, c) for (n, c) in knet._keyed(named=True) if isinstance(c.W, ksp.Conv2dTiledMatrix)]


def _plans(knet, n, mode):
    out = {}
    for (name, c) in _conv_layers(knet):
        la = c.launch(dev(), narrow=mode, narrow32=True)
        assert la.flags & N32
        with torch.cuda.device(dev()):
            out[name] = la.op.plan(n, la.flags)
    return out


def _tiled(z, n):
    return np.ascontiguousarray(z['x_cipher'][np.arange(n) % z['x_cipher'].shape[0]]).astype(np.float32)


@pytest.mark.parametrize('name', ['mini_tiled_permutation.npz', 'mini_tiled_permutation8.npz', 'mini_tiled_identity.npz'])
def test_whole_keynets_on_permutation_keys(golden, name):
    """forward_linear(narrow=True, narrow32=True) of 9 / 16 / 32 images == the default (padded) forward of the same images under the stored-order contract, logits
    and every layer, bit for bit; nothing is padded; every conv layer plans the new kernel; 33 images and the keyword without `narrow` are refused."""
    z = golden(name)
    knet = kio.keynet_from_arrays(z)
    knet.exact_mode(True)
    for n in (9, 16, 32):
        x = torch.as_tensor(_tiled(z, n)).to(dev())
        knet._padded_forwards = 0
        full = knet.forward_linear(x)
        assert knet._padded_forwards == 1
        knet._padded_forwards = 0
        y = knet.forward_linear(x, narrow=True, narrow32=True)
        assert knet._padded_forwards == 0
        assert y.shape == full.shape and torch.equal(y, full), n
        plans = _plans(knet, n, True)
        assert plans and all(KERNEL in p for p in plans.values()), plans
        (a, b) = (x, x)
        for (k, c, relu) in knet._steps():
            if k is None:
                (a, b) = (ksys._relu_block(a), ksys._relu_block(b))
                continue
            (a, b) = (c.forward(a, fuse_relu=relu, narrow=True, narrow32=True), c.forward(b, fuse_relu=relu))
            assert torch.equal(a, b), (n, k)
        assert torch.equal(knet.forward(x, narrow=True, narrow32=True), knet.forward(x))
    x33 = torch.as_tensor(_tiled(z, 33)).to(dev())
    for call in (knet.forward_linear, knet.forward, knet.capture):
        with pytest.raises(ValueError):
            call(x33, narrow=True, narrow32=True)
        with pytest.raises(ValueError):
            call(x33[:16], narrow32=True)
        with pytest.raises(ValueError):
            call(x33[:9], narrow=True, narrow_rows=True, narrow32=True)
    yr = knet.forward_linear(x33[:8], narrow=True, narrow_rows=True, narrow32=True)      # at most 8 images: the keyword changes nothing
    assert torch.equal(yr, knet.forward_linear(x33[:8], narrow=True, narrow_rows=True))
    with pytest.raises(ValueError):
        _conv_layers(knet)[0][1].W.torchdot(torch.zeros((_conv_layers(knet)[0][1].W.shape[1], 16), device=dev()), narrow32=True)


@pytest.mark.parametrize('name', ['mini_tiled_orthogonal.npz', 'mini_tiled_stochastic.npz', 'mini_tiled_permutation.npz'])
def test_whole_keynets_under_the_calibrated_contract(golden, name):
    """The loaded ('auto') contract after one calibrating wide forward: narrow='mfma', narrow32=True at 9 / 16 / 32 images is inside the gate against the bit-exact
    narrow32 forward, the wide decisions are untouched, nothing is padded; a narrow record is measured on at most 8 columns and its max_abs_x is the maximum of
    the whole batch; a x4 input trips the screen and re-measures."""
    z = golden(name)
    knet = kio.keynet_from_arrays(z)
    knet.exact_mode('auto')
    knet.forward_linear(torch.as_tensor(z['x_cipher']).to(dev()))
    before = copy.deepcopy(knet.contract_report())
    assert not before['undecided']
    knet._padded_forwards = 0
    for n in (16, 9, 32):
        x = torch.as_tensor(_tiled(z, n)).to(dev())
        ym = knet.forward_linear(x, narrow='mfma', narrow32=True)
        ye = knet.forward_linear(x, narrow=True, narrow32=True)
        (ratio, _, _, _) = gate(ym, ye)
        print(name, n, "narrow='mfma' vs narrow=True, narrow32: gate ratio %.3g" % ratio)
        assert ratio <= 1.0, (n, ratio)
    assert knet._padded_forwards == 0
    after = knet.contract_report()
    names = []
    for (rb, ra) in zip(before['layers'], after['layers']):
        assert ra['exact'] == rb['exact'] and ra['screened'] == rb['screened']
        assert {k: v for (k, v) in (ra['calibration'] or {}).items() if k != 'narrow'} == (rb['calibration'] or {}), ra['name']
        if ra['narrow'] is not None:
            assert ra['narrow']['measured_on_columns'] <= 8, ra
            if ra['narrow']['decided'] == 'mfma':
                names.append(ra['name'])
    if name == 'mini_tiled_permutation.npz':
        assert names, after
    # a layer's record, measured from a 16-column batch whose largest |x| sits in column 13: columns 8 .. 15 are measured, max_abs_x is the batch maximum
    layers = dict(knet._keyed(named=True))
    for lname in names:
        c = layers[lname]
        c.unscreen(narrow=True)
        xin = torch.as_tensor(np.random.RandomState(3).randn(16, c.W.shape[1]).astype(np.float32)).to(dev())
        xin[:, -1] = 1.0
        xin[13, 5] = 9.0
        c.forward(xin, narrow='mfma', narrow32=True)
        rec = c.narrow_record()
        assert rec is not None and rec['measured_on_columns'] == 8 and rec['max_abs_x'] == 9.0, rec
        c.unscreen(narrow=True)
    # the screen: only where a measurement put a layer on the matrix-core narrow kernel.  The permutation fixture always has such layers (asserted above); on the two
    # float-key fixtures calibration may leave none, and then there is no narrow screen to trip
    if not names:
        return
    x = torch.as_tensor(_tiled(z, 16)).to(dev())
    knet.forward_linear(x, narrow='mfma', narrow32=True)                    # measures on this batch
    rec0 = {r['name']: dict(r['narrow']) for r in knet.contract_report()['layers'] if r['name'] in names}
    knet.__dict__['_narrow_remeasurements'] = 0
    knet.forward_linear((x * 1.5).contiguous(), narrow='mfma', narrow32=True)
    assert knet.__dict__['_narrow_remeasurements'] == 0
    big = (x * 4.0).contiguous()
    y = knet.forward_linear(big, narrow='mfma', narrow32=True)
    assert knet.__dict__['_narrow_remeasurements'] >= 1
    rep = {r['name']: r for r in knet.contract_report()['layers']}
    assert rep[names[0]]['narrow'] is not None and rep[names[0]]['narrow']['max_abs_x'] > 2 * rec0[names[0]]['max_abs_x']
    assert rep[names[0]]['narrow']['measured_on_columns'] <= 8
    assert gate(y, knet.forward_linear(big, narrow=True, narrow32=True))[0] <= 1.0


@pytest.mark.parametrize('mode', [True, 'mfma'])
def test_capture(golden, mode):
    """capture(x16, narrow=..., narrow32=True): two replays on different inputs each equal the eager forward."""
    z = golden('mini_tiled_permutation.npz')
    knet = kio.keynet_from_arrays(z)
    if mode == 'mfma':
        knet.exact_mode(False)
    x = torch.as_tensor(_tiled(z, 16)).to(dev())
    replay = knet.capture(x, narrow=mode, narrow32=True)
    plans = _plans(knet, 16, mode)
    assert plans and all((MFMA_KERNEL if mode == 'mfma' else KERNEL) in p for p in plans.values()), plans
    other = (x.flip(0) * 0.5).contiguous()
    for xi in (x, other):
        eager = knet.forward_linear(xi, narrow=mode, narrow32=True)
        assert torch.equal(replay(xi).clone(), eager)
    assert not torch.equal(knet.forward_linear(other, narrow=mode, narrow32=True), knet.forward_linear(x, narrow=mode, narrow32=True))
    assert getattr(replay, 'graph', None) is not None


def test_fuzz_on_random_conv_operators():
    """Seeded: the conv layers of random source networks keyed by tiled permutations, and random factored operators with float coefficients, each at a random
    width of 9 .. 32: the channel-lane kernel is the oracle's bits, the matrix-core kernel passes its criterion.  At least 24 operators."""
    rng = np.random.RandomState(20261)
    ops = []
    nets = 0
    while len(ops) < 12:
        nets += 1
        assert nets < 200, 'the generator stopped producing conv layers'
        torch.manual_seed(int(rng.randint(1 << 30)))
        np.random.seed(int(rng.randint(1 << 30)))
        (net, inshape, names) = random_net(rng, sides=(6, 8, 12))
        if not any(n.startswith('conv') for n in names):
            continue
        (_, knet) = ksys.TiledPermutationKeynet(inshape, net, int(rng.choice([2, 3, 4])))
        ops += [(c.W, True) for (_, c) in knet._keyed(named=True) if isinstance(c.W, ksp.Conv2dTiledMatrix)]
    for _ in range(12):
        (Cin, Cout, H, k) = (int(rng.randint(1, 20)), int(rng.randint(20, 200)), int(rng.choice([4, 6, 8])), int(rng.choice([1, 3, 5])))
        (stride, unit, has_last) = (int(rng.choice([1, 2])), bool(rng.rand() < 0.3), bool(rng.rand() < 0.7))
        ops.append((_random_convtaps(rng, Cin, Cout, H, k, stride, unit, has_last), has_last))
    assert len(ops) >= 24
    for (W, has_last) in ops:
        n = int(rng.randint(9, 33))
        relu = bool(rng.rand() < 0.5)
        with torch.cuda.device(dev()):
            plan = W._device_op(dev()).plan(n, NARROW | N32 | (RELU if relu else 0))
            plan_m = W._device_op(dev()).plan(n, MFMA | N32 | (RELU if relu else 0))
        assert KERNEL in plan, (tuple(W.shape), n, plan)
        X = rng.randn(W.shape[1], n).astype(np.float32)
        if has_last:
            X[-1] = 1.0
        M = _sorted_csr(W)
        ref = _oracle(M, X)
        ref = np.maximum(ref, 0) if relu else ref
        xd = torch.as_tensor(X).to(dev())
        y = W.torchdot(xd, relu=relu, exact=False, narrow=True, narrow32=True).cpu().numpy()
        assert np.array_equal(y, ref), (tuple(W.shape), n, relu, plan, float(np.abs(y - ref).max()))
        ym = W.torchdot(xd, relu=relu, exact=False, narrow='mfma', narrow32=True).cpu().numpy()
        if MFMA_KERNEL in plan_m:
            assert close_conditioned(ym.T, ref.T, (M.shape, M.indptr, M.indices, M.data), X.T), (tuple(W.shape), n, relu, plan_m)
        else:
            assert np.array_equal(ym, ref), (tuple(W.shape), n, relu, plan_m)
