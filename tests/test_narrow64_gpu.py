"""The low-latency forward for 33 .. 64 images on the GPU (narrow64=True, KN_FLAG_NARROW64): the order-preserving pipeline with one column per lane
(convtaps_exact_pipe64_kernel, "64-column tiles" in the plan) against the CPU oracle, the 128-column order-preserving kernels and convtaps_narrow32_kernel on
32-column chunks -- bit for bit --; every form the launcher's rule gives; non-finite activations behind the zero guard; the modifier's semantics through the C ABI; the
32-bit offset guard on both sides; and KeyedModel.forward_linear / forward / capture with the keyword."""
import copy

import numpy as np
import pytest
import scipy.sparse
import torch
from torch import nn

from keynet_amd import io as kio
from keynet_amd import sparse as ksp
from keynet_amd import system as ksys
from keynet_amd import _capi
from keynet_amd.layer import KeyedLayer
from test_parity_gpu import _random_convtaps, dev
from test_narrow_gpu import _build, _oracle, _sorted_csr
from test_narrow32_gpu import SHAPES, _case, _conv_layers, _tiled
from test_large_offsets_gpu import bufs, conv, last_ok, run      # noqa: F401  (bufs: the module-scoped fixture of the two shared 8.6 GB buffers)
from test_factored_untiled import conv_layer
from narrow_helpers import SENTINEL, _spmm

pytestmark = pytest.mark.gpu

(RELU, EXACT, BF16X3, NARROW, MFMA, ROWS, N32, N64) = (_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_BF16X3, _capi.KN_FLAG_NARROW, _capi.KN_FLAG_NARROW_MFMA,
                                                       _capi.KN_FLAG_NARROW_ROWS, _capi.KN_FLAG_NARROW32, _capi.KN_FLAG_NARROW64)
PIPE = 'convtaps_exact_pipe_kernel'
FORM = '64-column tiles'
N32_KERNEL = 'convtaps_narrow32_kernel'
WIDTHS = [33, 47, 63, 64]


def _plan(W, n, flags, **kw):
    with torch.cuda.device(dev()):
        return W._device_op(dev()).plan(n, flags, **kw)


def _pipe_shape(W):
    """The pipeline's shape, read off the factored operator: no (output, input) pixel pair hit twice and at most 64 slots per output pixel."""
    t = (W._factored if isinstance(W, ksp.FactoredSparseMatrix) else W)._taps
    pairs = t['ent_out'].astype(np.int64) * (int(t['ent_in'].max()) + 1) + t['ent_in']
    return len(np.unique(pairs)) == len(pairs) and int(np.bincount(t['ent_out']).max()) <= 64


@pytest.mark.parametrize('n_vecs', WIDTHS)
@pytest.mark.parametrize('case', SHAPES, ids=[c[0] for c in SHAPES])
def test_narrow64_form_against_the_oracle_the_128_column_kernels_and_the_narrow32_kernel(case, n_vecs):
    (W, M, X, xd, y128) = _case(case)
    plan = _plan(W, n_vecs, NARROW | N64)
    if _pipe_shape(W):
        assert PIPE in plan and FORM in plan and ',coef' not in plan, plan
    else:                                                                          # filled-in operators: what KN_FLAG_EXACT runs at that width
        assert case[0].startswith('filled') or not case[6]
        assert plan == _plan(W, n_vecs, EXACT) and PIPE not in plan and 'convtaps_exact_' in plan, plan
    if case[0].startswith('factored'):
        assert 'convtaps_zero_guard_kernel' in plan, plan
    ref = _oracle(M, X[:, :n_vecs])
    x = xd[:, :n_vecs]
    for relu in (False, True):
        y = W.torchdot(x, relu=relu, exact=True, narrow=True, narrow64=True).cpu().numpy()
        assert np.array_equal(y, np.maximum(ref, 0) if relu else ref), (case[0], n_vecs, relu, float(np.abs(y - ref).max()))
    y = W.torchdot(x, exact=True, narrow=True, narrow64=True)
    assert torch.equal(y, y128[:, :n_vecs])
    for lo in range(0, n_vecs, 32):
        hi = min(lo + 32, n_vecs)
        assert torch.equal(y[:, lo:hi], W.torchdot(x[:, lo:hi], exact=True, narrow=True, narrow32=True)), (lo, hi)


# (Cin, Cout, H, stride, columns, coefficients, bias column) -> (output channels per wavefront, coefficients): 16 channels need Cout % 16 == 0 and 4 096 (pixel, bundle)
# items -- 64 x 64 pixels x 4 bundles --, the nine-pixel layer runs 8 and its last bundle (channels 64 .. 71) reaches beyond Cout = 70; a width that fills the tile and
# 33, one lane of the second half-wave
FORMS = [((3, 64, 64, 1, n, coef, last), (16, coef)) for n in (64, 33) for coef in (False, True) for last in (True, False)] + \
        [((5, 70, 6, 2, n, coef, last), (8, coef)) for n in (64, 33) for coef in (False, True) for last in (True, False)]


@pytest.mark.parametrize('shape,form', FORMS, ids=['cin%d-cout%d-%dx%d-%d%s%s-rbx%d' % (s[0], s[1], s[2], s[2], s[4], '-coef' if s[5] else '', '-bias' if s[6] else '', f[0]) for (s, f) in FORMS])
def test_every_form_of_the_kernel_gives_the_oracles_bits(shape, form):
    (Cin, Cout, H, stride, n, coef, has_last) = shape
    rng = np.random.RandomState(11)
    W = _random_convtaps(rng, Cin, Cout, H, 3, stride, True, has_last)
    if coef:                                                                  # float coefficients on the unit operator's own entries: no pixel pair hit twice
        t = W._taps
        W = ksp.Conv2dTiledMatrix.fromtaps(W._inshape, W._outshape, t['taps'], t['ent_out'], t['ent_in'], t['ent_tap'], (rng.rand(len(t['ent_out'])) + 0.5).astype(np.float32), t['lastcol'])
    X = rng.randn(W.shape[1], n).astype(np.float32)
    if has_last:
        X[-1] = 1.0
    plan = _plan(W, n, NARROW | N64 | RELU)
    assert PIPE in plan and FORM in plan, plan
    seen = (int(plan[plan.index(PIPE + '<') + len(PIPE) + 1:].split(',')[0]), ',coef' in plan)
    assert seen == form, plan
    y = W.torchdot(torch.as_tensor(X).to(dev()), relu=True, exact=False, narrow=True, narrow64=True).cpu().numpy()
    ref = np.maximum(_oracle(_sorted_csr(W), X), 0)
    assert np.array_equal(y, ref), (plan, float(np.abs(y - ref).max()))


def test_non_finite_activations_behind_the_zero_guard():
    """A kn_convtaps_drop_zero_entries handle (tap entries that are exactly zero, absent from the reference's CSR) at 40 columns with +-Inf and NaN activations: scipy's
    product of the reference operator, NaN for NaN -- 0 * Inf does not appear where the reference has no entry.  A NaN in one column leaves every other column's bits."""
    (W, M, X, rng) = _build(SHAPES[8], seed=21)
    assert SHAPES[8][0].startswith('factored') and isinstance(W, ksp.FactoredSparseMatrix)
    n = 40
    X = X[:, :n].copy()
    rows = rng.choice(W.shape[1] - 1, size=6, replace=False)
    X[rows[:3], 35] = np.nan
    X[rows[3:], 3] = [np.inf, -np.inf, np.inf]
    X[rows[3:], 38] = [-np.inf, np.inf, np.inf]
    ref = _oracle(M, X)
    assert np.isnan(ref).any() and np.isfinite(ref[:, 0]).all()
    plan = _plan(W, n, NARROW | N64 | EXACT)
    assert PIPE in plan and FORM in plan and 'convtaps_zero_guard_kernel' in plan, plan
    for relu in (False, True):
        y = W.torchdot(torch.as_tensor(X).to(dev()), relu=relu, exact=True, narrow=True, narrow64=True).cpu().numpy()
        r = np.where(np.isnan(ref), ref, np.maximum(ref, 0)).astype(np.float32) if relu else ref
        assert np.array_equal(y, r, equal_nan=True), relu
    # a NaN in ONE column of an ordinary operator: the others keep their bits
    (W0, M0, X0, xd0, y128) = _case(SHAPES[0])
    Xn = X0[:, :n].copy()
    Xn[7, 33] = np.nan
    y = W0.torchdot(torch.as_tensor(Xn).to(dev()), exact=True, narrow=True, narrow64=True)
    keep = [c for c in range(n) if c != 33]
    assert torch.equal(y[:, keep], y128[:, keep]) and bool(torch.isnan(y[:, 33]).any())
    assert np.array_equal(y.cpu().numpy(), _oracle(M0, Xn), equal_nan=True)


def test_flag_semantics():
    """The modifier alone; next to KN_FLAG_NARROW at 8, 9, 32 and 65 columns and next to KN_FLAG_NARROW32 at 20: the plan and bits of the call without it.  At 40 columns
    the matrix-core request is the same call bit for bit, and KN_FLAG_EXACT / KN_FLAG_BF16X3 next to the flags change nothing.  Plain KN_FLAG_EXACT at 64 columns keeps the
    generic kernel.  CSR, dense and float64 handles ignore the modifier."""
    (W, M, X, _) = _build(('semantics', 16, 64, 8, 3, 1, True, True), seed=9)
    xd = torch.as_tensor(X).to(dev())
    with torch.cuda.device(dev()):
        op = W._device_op(dev())
    for n in (1, 8, 9, 32, 33, 40, 64, 65, 128):
        for flags in (0, EXACT, RELU, BF16X3, N32, ROWS):                       # alone
            (y1, _, p1) = _spmm(op, xd, n, flags | N64)
            (y0, _, p0) = _spmm(op, xd, n, flags)
            assert p1 == p0 and FORM not in p1 and torch.equal(y1, y0), (n, flags, p1, p0)
    for n in (8, 9, 32, 65):
        for flags in (NARROW, MFMA, NARROW | EXACT, MFMA | RELU, NARROW | BF16X3):
            (y1, _, p1) = _spmm(op, xd, n, flags | N64)
            (y0, _, p0) = _spmm(op, xd, n, flags)
            assert p1 == p0 and FORM not in p1 and torch.equal(y1, y0), (n, flags, p1, p0)
    for flags in (NARROW, MFMA):
        (y1, _, p1) = _spmm(op, xd, 20, flags | N32 | N64)
        (y0, _, p0) = _spmm(op, xd, 20, flags | N32)
        assert p1 == p0 and ('convtaps_narrow' in p1) and FORM not in p1 and torch.equal(y1, y0), (flags, p1, p0)
    (y32, _, p32) = _spmm(op, xd, 20, NARROW | N32 | N64)
    assert N32_KERNEL in p32, p32
    for n in (33, 40, 64):
        (ye, _, pe) = _spmm(op, xd, n, NARROW | N64)
        assert PIPE in pe and FORM in pe, pe
        assert np.array_equal(ye.cpu().numpy(), _oracle(M, X[:, :n]))
        (yx, _, px) = _spmm(op, xd, n, EXACT)
        assert 'convtaps_exact_kernel' in px and PIPE not in px and torch.equal(ye, yx), px      # plain KN_FLAG_EXACT: the generic kernel, the same bits
        for flags in (MFMA, NARROW | EXACT, NARROW | BF16X3, MFMA | EXACT, MFMA | BF16X3, NARROW | MFMA | EXACT | BF16X3, NARROW | N32, MFMA | N32):
            (y, _, p) = _spmm(op, xd, n, flags | N64)
            assert p == pe and torch.equal(y, ye), (n, flags, p)
        (yr, _, _) = _spmm(op, xd, n, MFMA | RELU | N64)
        assert torch.equal(yr, torch.clamp(ye, min=0))
    # CSR, float64 and dense handles
    A = scipy.sparse.random(40, 30, density=0.3, format='csr', dtype=np.float32, random_state=3)
    xs = torch.as_tensor(np.random.RandomState(2).randn(30, 64).astype(np.float32)).to(dev())
    with torch.cuda.device(dev()):
        opc = ksp.SparseMatrix(A)._device_op(dev())
    for n in (4, 40, 64):
        for flags in (EXACT, EXACT | NARROW, EXACT | MFMA, EXACT | NARROW | N32):
            (y1, _, p1) = _spmm(opc, xs, n, flags | N64)
            (y0, _, p0) = _spmm(opc, xs, n, flags)
            assert p1 == p0 and torch.equal(y1, y0), (n, flags, p1, p0)
    W64 = ksp.SparseMatrix(A.astype(np.float64))
    with torch.cuda.device(dev()):
        op64 = W64._device_op(dev())
        assert op64.plan(40, EXACT | NARROW | N64) == op64.plan(40, EXACT)
        (ya, yb) = (torch.empty((40, 40), dtype=torch.float64, device=dev()), torch.empty((40, 40), dtype=torch.float64, device=dev()))
        xc = xs[:, :40].contiguous()
        op64.spmm_f64(xc.data_ptr(), 40, 40, ya.data_ptr(), 40, EXACT | NARROW | N64, torch.cuda.current_stream().cuda_stream)
        op64.spmm_f64(xc.data_ptr(), 40, 40, yb.data_ptr(), 40, EXACT, torch.cuda.current_stream().cuda_stream)
    assert torch.equal(ya, yb)
    Dm = np.random.RandomState(4).randn(ksp.SparseMatrix.DENSE_MIN_ELEMENTS // 4097 + 2, 4097).astype(np.float32)      # a keyed Linear: homogeneous last row
    Dm[-1] = 0
    Dm[-1, -1] = 1
    with torch.cuda.device(dev()):
        opd = ksp.SparseMatrix(scipy.sparse.csr_matrix(Dm))._dense_device_op(dev())
    assert opd is not None
    xdn = torch.as_tensor(np.random.RandomState(5).randn(4097, 40).astype(np.float32)).to(dev())
    for flags in (0, NARROW, MFMA, RELU | NARROW):
        (y1, _, p1) = _spmm(opd, xdn, 40, flags | N64)
        (yf, _, pf) = _spmm(opd, xdn, 40, flags)
        assert p1 == pf and torch.equal(y1, yf), (flags, p1, pf)


@pytest.mark.parametrize('n', [40, 64])
def test_leading_dimensions_and_an_unaligned_block(n):
    """ldx > n_vecs, ldy > n_vecs and an x that starts 4 bytes off a 16-byte boundary (a window at column 5 of a 1 027-wide block): the bits of the compact call, and
    everything outside the window of Y -- the sentinel right behind column n included -- untouched."""
    (W, M, X, rng) = _build(('window64', 5, 24, 8, 3, 1, True, True), seed=13)
    (ld, c0) = (1027, 5)
    Xb = rng.randn(W.shape[1], ld).astype(np.float32)
    Xb[-1] = 1.0
    xb = torch.as_tensor(Xb).to(dev())
    with torch.cuda.device(dev()):
        op = W._device_op(dev())
    (win, yb, plan) = _spmm(op, xb, n, NARROW | N64 | RELU, ld=ld, start=c0)
    assert PIPE in plan and FORM in plan, plan
    alone = W.torchdot(xb[:, c0:c0 + n], relu=True, exact=False, narrow=True, narrow64=True)
    assert torch.equal(win, alone)
    assert np.array_equal(alone.cpu().numpy(), np.maximum(_oracle(M, Xb[:, c0:c0 + n]), 0))
    outside = torch.ones(ld, dtype=torch.bool, device=dev())
    outside[c0:c0 + n] = False
    assert bool(torch.all(yb[:, outside] == SENTINEL)) and bool(torch.all(yb[:, c0 + n] == SENTINEL))


@pytest.mark.parametrize('side', ['last', 'first-beyond'])
def test_conv_pipeline_guard_at_one_column_per_lane(bufs, side):     # noqa: F811
    """(Cin HiWi + 1) * ldx < 2^31, as for the other forms of the pipeline; beyond it the plain order-preserving kernel with the same bits (never a refusal)."""
    c = conv(16, 64, 8, 3, 1, True, True)
    (L, F) = last_ok(1 << 31, 16 * 64 + 1)
    if side == 'last':
        run(bufs, c, 64, NARROW | N64, ldx=L, expect=[PIPE, FORM])
    else:
        plan = run(bufs, c, 64, NARROW | N64, ldx=F, expect=['convtaps_exact_kernel<vec=1>'], forbid=[PIPE])
        with torch.cuda.device(dev()):
            assert plan == c.op.plan(64, EXACT, ldx=F, ldy=64)


def _steps_equal(knet, x, kw):
    (a, b) = (x, x)
    for (k, c, relu) in knet._steps():
        if k is None:
            (a, b) = (ksys._relu_block(a), ksys._relu_block(b))
            continue
        (a, b) = (c.forward(a, fuse_relu=relu, **kw), c.forward(b, fuse_relu=relu))
        assert torch.equal(a, b), k


@pytest.mark.parametrize('name', ['mini_tiled_permutation.npz', 'mini_tiled_identity.npz'])
def test_whole_keynets_under_the_default_contract(golden, name):
    """forward_linear(narrow=True, narrow64=True) of 33 / 50 / 64 images == the default (padded) forward of the same images under the stored-order contract, logits and
    every layer, bit for bit; nothing is padded; every conv layer plans the new form; at 20 images the call is narrow32=True; forward() decrypts to the plain call's logits."""
    z = golden(name)
    knet = kio.keynet_from_arrays(z)
    knet.exact_mode(True)
    kw = dict(narrow=True, narrow64=True)
    for n in (33, 50, 64):
        x = torch.as_tensor(_tiled(z, n)).to(dev())
        knet._padded_forwards = 0
        full = knet.forward_linear(x)
        assert knet._padded_forwards == 1
        y = knet.forward_linear(x, **kw)
        assert knet._padded_forwards == 1
        assert y.shape == full.shape and torch.equal(y, full), n
        seen = 0
        for (lname, c) in _conv_layers(knet):
            la = c.launch(dev(), **kw)
            assert la.flags & NARROW and la.flags & N32 and la.flags & N64
            with torch.cuda.device(dev()):
                (p, pe) = (la.op.plan(n, la.flags), la.op.plan(n, EXACT | (la.flags & RELU)))
            if PIPE in p:                                # (a filled-in layer has no pipeline shape: what KN_FLAG_EXACT runs at that width)
                assert FORM in p, (lname, p)
                seen += 1
            else:
                assert p == pe, (lname, p, pe)
        assert seen, 'no conv layer of the key-net has the pipeline shape'
        _steps_equal(knet, x, kw)
        assert torch.equal(knet.forward(x, **kw), knet.forward(x))
    x20 = torch.as_tensor(_tiled(z, 20)).to(dev())
    assert torch.equal(knet.forward_linear(x20, **kw), knet.forward_linear(x20, narrow=True, narrow32=True))
    for (lname, c) in _conv_layers(knet):
        la = c.launch(dev(), **kw)
        with torch.cuda.device(dev()):
            assert N32_KERNEL in la.op.plan(20, la.flags), lname


def test_capture(golden):
    """capture(x50, narrow=True, narrow64=True): replays on two different batches each equal the eager forward."""
    z = golden('mini_tiled_permutation.npz')
    knet = kio.keynet_from_arrays(z)
    x = torch.as_tensor(_tiled(z, 50)).to(dev())
    replay = knet.capture(x, narrow=True, narrow64=True)
    other = (x.flip(0) * 0.5).contiguous()
    for xi in (x, other):
        eager = knet.forward_linear(xi, narrow=True, narrow64=True)
        assert torch.equal(replay(xi).clone(), eager)
    assert not torch.equal(knet.forward_linear(other, narrow=True, narrow64=True), knet.forward_linear(x, narrow=True, narrow64=True))
    assert getattr(replay, 'graph', None) is not None


def test_an_untiled_factored_keynet_at_48_images(monkeypatch):
    """Two untiled conv layers on their factored device form (never padded; at this width on the generic order-preserving kernel without the keyword): the narrow64
    forward equals the plain one bit for bit and runs both layers on the new form."""
    monkeypatch.setattr(KeyedLayer, 'FACTOR_UNTILED_MIN_NNZ', 0)
    l1 = conv_layer(4, 32, 8, zeros=[(1, 2, 0, 0)], seed=1)
    l2 = conv_layer(32, 16, 8, seed=2)
    assert isinstance(l1.W, ksp.FactoredSparseMatrix) and isinstance(l2.W, ksp.FactoredSparseMatrix)
    knet = ksys.KeyedModel.fromlayers({'conv1': l1, 'relu1': nn.ReLU(), 'conv2': l2}, (16, 8, 8))
    rng = np.random.RandomState(3)
    X = np.hstack((rng.randn(48, 4 * 64).astype(np.float32), np.ones((48, 1), np.float32)))
    x = torch.as_tensor(X).to(dev())
    plain = knet.forward_linear(x)
    y = knet.forward_linear(x, narrow=True, narrow64=True)
    assert torch.equal(y, plain)
    for c in (l1, l2):
        la = c.launch(dev(), narrow=True, narrow64=True)
        with torch.cuda.device(dev()):
            p = la.op.plan(48, la.flags)
            assert PIPE in p and FORM in p, p
            assert 'convtaps_exact_kernel' in la.op.plan(48, c.launch(dev()).flags)


def test_the_contract_report_of_an_auto_keynet_is_unchanged(golden):
    z = golden('mini_tiled_permutation.npz')
    knet = kio.keynet_from_arrays(z)
    knet.exact_mode('auto')
    knet.forward_linear(torch.as_tensor(z['x_cipher']).to(dev()))
    before = copy.deepcopy(knet.contract_report())
    assert not before['undecided']
    x = torch.as_tensor(_tiled(z, 50)).to(dev())
    knet._padded_forwards = 0
    y = knet.forward_linear(x, narrow=True, narrow64=True)
    assert knet._padded_forwards == 0 and knet.contract_report() == before
    knet.exact_mode(True)
    assert torch.equal(y, knet.forward_linear(x))              # the conv layers ran the reference's own arithmetic whatever the contract was


def test_argument_rules(golden):
    z = golden('mini_tiled_permutation.npz')
    knet = kio.keynet_from_arrays(z)
    x65 = torch.as_tensor(_tiled(z, 65)).to(dev())
    for call in (knet.forward_linear, knet.forward, knet.capture):
        with pytest.raises(ValueError):
            call(x65[:40], narrow64=True)                       # without `narrow`
        with pytest.raises(ValueError):
            call(x65, narrow=True, narrow64=True)               # 65 images
        with pytest.raises(ValueError, match='matrix-core'):
            call(x65[:33], narrow='mfma', narrow64=True)        # no matrix-core form at 33 .. 64 images
        with pytest.raises(ValueError):
            call(x65[:9], narrow=True, narrow_rows=True, narrow64=True)
    y = knet.forward_linear(x65[:32], narrow='mfma', narrow64=True)             # accepted at 32: exactly narrow32=True
    assert torch.equal(y, knet.forward_linear(x65[:32], narrow='mfma', narrow32=True))
    with pytest.raises(ValueError):
        W = _conv_layers(knet)[0][1].W
        W.torchdot(torch.zeros((W.shape[1], 40), device=dev()), narrow64=True)
