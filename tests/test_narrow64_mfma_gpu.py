"""The matrix-core forward for 33 .. 64 images on the GPU (narrow64='mfma', KN_FLAG_NARROW64_MFMA): convtaps_mfma_kernel<MT = 64 | 128, NB = 64> through the C ABI.
The contract is the K order: every column has the bits of the same handle's plain matrix-core call on the batch zero-padded to 128 columns (wherever that call's plan
names convtaps_mfma_kernel -- at 128 columns no small-K kernel runs, so that is every case here), and lies inside the project's gate against KN_FLAG_EXACT.  Then the
flag's semantics, and KeyedModel.forward_linear / forward / capture with the keyword on the reference-generated mini-nets."""
import copy

import numpy as np
import pytest
import scipy.sparse
import torch

from keynet_amd import io as kio
from keynet_amd import sparse as ksp
from keynet_amd import _capi
from keynet_amd.layer import KeyedLayer, gate
from test_parity_gpu import _random_convtaps, dev
from test_narrow_gpu import _oracle, _sorted_csr
from test_narrow32_gpu import _conv_layers, _tiled
from test_narrow_host import _tiny_conv
from narrow_helpers import SENTINEL, _spmm

pytestmark = pytest.mark.gpu

(RELU, EXACT, BF16X3, NARROW, MFMA, ROWS, N32, N64, N64M) = (_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_BF16X3, _capi.KN_FLAG_NARROW, _capi.KN_FLAG_NARROW_MFMA,
                                                             _capi.KN_FLAG_NARROW_ROWS, _capi.KN_FLAG_NARROW32, _capi.KN_FLAG_NARROW64, _capi.KN_FLAG_NARROW64_MFMA)
TILE64 = MFMA | N32 | N64 | N64M
KERNEL = 'convtaps_mfma_kernel'
PIPE = 'convtaps_exact_pipe_kernel'
(GENERIC, FAST, SPTR, GROUPS) = ('loader=generic', 'loader=fast(per-thread pointers)', 'loader=sptr(wave-uniform pointers)', 'loader=sptr(wave-uniform pointers, slot groups)')
WIDTHS = [33, 40, 63, 64]

# id -> ((Cin, Cout, H, k, stride, unit coefficients, bias column), tile height, KC, loaders of 64 aligned columns).  The tile height is 128 where that
# divides the padded channel count (64 for Cout <= 64, else whole 128s) and leaves pixels x channel tiles >= 1 024 workgroups: 32 x 32 pixels reach it, 16 x 16 and the small
# layers do not.  cin48: three channel chunks per slot, where chunk-outer and slot-outer walks differ; a 64-channel operator's wide launch (256-column tiles) runs the
# generic loader on a 128-column batch, so its 64-column launch follows that walk on the generic loader too; 9x9 with second entries: more than 64 slots per pixel.
CASES = {
    'cin3-cout40-8x8-bias': ((3, 40, 8, 3, 1, True, True), 64, 4, FAST),
    'cin16-cout64-8x8-nobias': ((16, 64, 8, 3, 1, True, False), 64, 16, SPTR),
    'cin48-cout64-6x6-bias': ((48, 64, 6, 3, 1, True, True), 64, 16, GENERIC),
    'cin48-cout128-7x7-coef-bias': ((48, 128, 7, 3, 1, False, True), 64, 16, SPTR),
    'cin48-cout320-8x8-s2-nobias': ((48, 320, 8, 3, 2, True, False), 64, 16, SPTR),
    'cin32-cout128-12x12-9x9-groups': ((32, 128, 12, 9, 1, False, True), 64, 16, GROUPS),
    'cin16-cout256-32x32-bias': ((16, 256, 32, 3, 1, True, True), 128, 16, SPTR),
    'cin16-cout256-32x32-s2-below-threshold': ((16, 256, 32, 3, 2, True, True), 64, 16, SPTR),
    'cin16-cout320-32x32-coef': ((16, 320, 32, 3, 1, False, False), 128, 16, SPTR),
    'cin3-cout256-32x32-bias': ((3, 256, 32, 3, 1, True, True), 128, 4, FAST),
    'cin5-cout128-32x32-coef': ((5, 128, 32, 3, 1, False, True), 128, 4, GENERIC),
}
_cache = {}


def _case(name):
    """(W, handle, X [cols, 64] on the device, the plain matrix-core result of X zero-padded to 128 columns [rows, 64], the KN_FLAG_EXACT result) -- built once, left unchanged."""
    if name not in _cache:
        shape = CASES[name][0]
        rng = np.random.RandomState(sum(map(ord, name)))
        W = _random_convtaps(rng, *shape)
        X = rng.randn(W.shape[1], 64).astype(np.float32)
        if shape[-1]:
            X[-1] = 1.0
        xd = torch.as_tensor(X).to(dev())
        with torch.cuda.device(dev()):
            op = W._device_op(dev())
        if 'groups' in name:
            assert int(np.bincount(W._taps['ent_out']).max()) > 64
        _cache[name] = (W, op, xd, {}, _spmm(op, xd, 64, EXACT)[0])
    return _cache[name]


def _padded(name, n, relu=0):
    """Columns 0 .. n of the handle's plain matrix-core call on the first n columns zero-padded to 128 aligned columns; that call's plan names the f32 tile kernel."""
    (W, op, xd, memo, _) = _case(name)
    if (n, relu) not in memo:
        xp = torch.zeros((xd.shape[0], 128), dtype=torch.float32, device=dev())
        xp[:, :n] = xd[:, :n]
        (y, _, plan) = _spmm(op, xp, 128, relu)
        assert KERNEL in plan and 'smallk' not in plan, plan
        memo[(n, relu)] = y[:, :n].clone()
    return memo[(n, relu)]


@pytest.mark.parametrize('n', WIDTHS)
@pytest.mark.parametrize('name', sorted(CASES))
def test_every_column_has_the_bits_of_the_padded_matrix_core_call(name, n):
    (W, op, xd, _, ye) = _case(name)
    (shape, mt, kc, loaders) = CASES[name]
    x = xd[:, :n].contiguous()
    slot = torch.zeros(1, dtype=torch.float32, device=dev())
    (y, _, plan) = _spmm(op, x, n, TILE64, absmax=slot)
    assert '%s<MT=%d,NB=64,KC=%d>' % (KERNEL, mt, kc) in plan, plan
    assert (loaders if n == 64 else GENERIC) in plan, plan                         # 64 aligned columns: the loaders of the wide tile; any other width: generic
    assert ('+coef' in plan) == (not shape[5]) and 'tail_split' not in plan and 'occ_cap=0' in plan, plan
    assert torch.equal(y, _padded(name, n)), (name, n, float((y - _padded(name, n)).abs().max()))
    g = gate(y, ye[:, :n])
    print(name, n, plan, 'gate %.3g' % g[0])
    assert g[0] <= 1, (name, n, g)
    assert float(slot) == float(y.abs().max())                                     # max |Y|: in the epilogue at 64 aligned columns, one pass over Y elsewhere
    (y2, _, _) = _spmm(op, x, n, TILE64)
    assert torch.equal(y2, y)                                                      # the same bits twice
    (yr, _, _) = _spmm(op, x, n, TILE64 | RELU)
    assert torch.equal(yr, _padded(name, n, RELU)) and torch.equal(yr, torch.clamp(y, min=0))


def _guarded(op, xb, n, flags, ldy, start):
    """kn_spmm on columns start .. start + n of xb into that window of a sentinel-filled block with two sentinel rows in front of and behind Y: (window, whole block)."""
    (rows, _) = op.shape()
    yb = torch.full((rows + 4, ldy), SENTINEL, dtype=torch.float32, device=dev())
    with torch.cuda.device(dev()):
        op.spmm(xb.data_ptr() + 4 * start, int(xb.shape[1]), n, yb.data_ptr() + 4 * (2 * ldy + start), ldy, flags, torch.cuda.current_stream().cuda_stream)
        plan = op.plan(n, flags, ldx=int(xb.shape[1]), ldy=ldy)
    return (yb[2:-2, start:start + n], yb, plan)


@pytest.mark.parametrize('name', ['cin3-cout40-8x8-bias', 'cin48-cout128-7x7-coef-bias', 'cin48-cout64-6x6-bias', 'cin32-cout128-12x12-9x9-groups'])
def test_leading_dimensions_an_unaligned_block_and_what_stays_untouched(name):
    """ldx, ldy > n_vecs: an aligned window of 64 columns keeps the wide tile's loaders; a window 20 bytes into a 1 027-wide block (and 40 or 63 columns) runs the generic
    loader.  The bits of the compact call; surplus columns and the sentinel rows around Y untouched."""
    (W, op, xd, _, _) = _case(name)
    loaders = CASES[name][3]
    for (ld, c0, n, want) in ((1024, 64, 64, loaders), (1027, 5, 64, GENERIC), (1027, 5, 40, GENERIC), (1024, 0, 63, GENERIC)):
        xb = torch.full((xd.shape[0], ld), 3.0, dtype=torch.float32, device=dev())
        xb[:, c0:c0 + n] = xd[:, :n]
        (win, yb, plan) = _guarded(op, xb, n, TILE64 | RELU, ld, c0)
        assert 'NB=64' in plan and want in plan, plan
        assert torch.equal(win, _padded(name, n, RELU)), (name, ld, c0, n)
        outside = torch.ones(ld, dtype=torch.bool, device=dev())
        outside[c0:c0 + n] = False
        assert bool(torch.all(yb[2:-2][:, outside] == SENTINEL)) and bool(torch.all(yb[:2] == SENTINEL)) and bool(torch.all(yb[-2:] == SENTINEL))


@pytest.mark.parametrize('n', [40, 64])
@pytest.mark.parametrize('name', ['cin3-cout40-8x8-bias', 'cin48-cout128-7x7-coef-bias', 'cin16-cout64-8x8-nobias'])
def test_non_finite_activations(name, n):
    """NaN in one column and +-Inf in another, at a few input rows: the result is finite exactly where the oracle's is and NaN where the oracle's is NaN (as
    test_narrow_mfma_gpu.py compares); every other column keeps its bits."""
    (W, op, xd, _, _) = _case(name)
    M = _sorted_csr(W)
    rng = np.random.RandomState(21)
    X = xd[:, :n].cpu().numpy().copy()
    rows = rng.choice(W.shape[1] - 1, size=6, replace=False)
    X[rows[:3], 35] = np.nan
    X[rows[3:], 3] = [np.inf, -np.inf, np.inf]
    ref = _oracle(M, X)
    assert np.isnan(ref).any() and np.isfinite(ref[:, 0]).all() and np.isfinite(ref[:, 35]).any()
    (y, _, plan) = _spmm(op, torch.as_tensor(X).to(dev()), n, TILE64)
    assert 'NB=64' in plan, plan
    keep = [c for c in range(n) if c not in (3, 35)]
    assert torch.equal(y[:, keep], _padded(name, n)[:, keep])
    y = y.cpu().numpy()
    assert np.array_equal(np.isfinite(y), np.isfinite(ref)) and bool(np.isnan(y[np.isnan(ref)]).all()), name


def test_flag_semantics():
    """The bit alone, next to one of its two companions only, at 32 and fewer or more than 64 columns, on CSR / float64 / dense / chain handles and in kn_spmm_planes: the plan
    and the bits of the call without it.  With both companions at 33 .. 64 columns: the tile kernel; KN_FLAG_BF16X3 next to it changes nothing; with KN_FLAG_EXACT the
    order-preserving pipeline of KN_FLAG_NARROW64; and KN_FLAG_NARROW_MFMA | KN_FLAG_NARROW64 without the bit stays that pipeline."""
    (W, op, xd, _, _) = _case('cin16-cout64-8x8-nobias')
    xw = torch.cat((xd, xd), dim=1).contiguous()
    for n in (1, 8, 9, 32, 33, 40, 64, 65, 128):
        for flags in (0, EXACT, RELU, BF16X3, N32, N64, ROWS, NARROW, MFMA, NARROW | N32, MFMA | N32, NARROW | N64, NARROW | N32 | N64, MFMA | N64 | EXACT, MFMA | N32 | N64 | EXACT | RELU):
            (y1, _, p1) = _spmm(op, xw, n, flags | N64M)
            (y0, _, p0) = _spmm(op, xw, n, flags)
            assert p1 == p0 and 'NB=64' not in p1 and torch.equal(y1, y0), (n, flags, p1, p0)
        if not 32 < n <= 64:
            for flags in (MFMA | N64, MFMA | N32 | N64, MFMA | N32 | N64 | RELU, MFMA | N64 | BF16X3):
                (y1, _, p1) = _spmm(op, xw, n, flags | N64M)
                (y0, _, p0) = _spmm(op, xw, n, flags)
                assert p1 == p0 and 'NB=64' not in p1 and torch.equal(y1, y0), (n, flags, p1, p0)
    for n in (33, 40, 64):
        (yp, _, pp) = _spmm(op, xw, n, MFMA | N64)                                  # without the bit: the order-preserving pipeline (test_narrow64_gpu.py pins it)
        assert PIPE in pp and '64-column tiles' in pp and torch.equal(yp, _spmm(op, xw, n, EXACT)[0]), pp
        (yt, _, pt) = _spmm(op, xw, n, MFMA | N64 | N64M)
        assert KERNEL in pt and 'NB=64' in pt and PIPE not in pt, pt
        for flags in (MFMA | N64 | N64M | N32, MFMA | N64 | N64M | BF16X3, MFMA | N64 | N64M | NARROW, MFMA | N64 | N64M | ROWS):
            (y, _, p) = _spmm(op, xw, n, flags)
            assert p == pt and torch.equal(y, yt), (n, flags, p)
        for flags in (MFMA | N64 | N64M | EXACT, TILE64 | EXACT | BF16X3):
            (y, _, p) = _spmm(op, xw, n, flags)
            assert p == pp and torch.equal(y, yp), (n, flags, p)
    # CSR, float64, dense and chain handles, kn_spmm_planes
    A = scipy.sparse.random(40, 30, density=0.3, format='csr', dtype=np.float32, random_state=3)
    xs = torch.as_tensor(np.random.RandomState(2).randn(30, 64).astype(np.float32)).to(dev())
    with torch.cuda.device(dev()):
        opc = ksp.SparseMatrix(A)._device_op(dev())
        chain = _capi.Operator.chain([_capi.Operator.csr(A.shape, A.indptr, A.indices, A.data)], [0])
    for n in (4, 40, 64):
        for flags in (EXACT, EXACT | MFMA | N64, MFMA | N32 | N64):
            for o in (opc, chain):
                (y1, _, p1) = _spmm(o, xs, n, flags | N64M)
                (y0, _, p0) = _spmm(o, xs, n, flags)
                assert p1 == p0 and torch.equal(y1, y0), (n, flags, p1, p0)
    st = torch.cuda.current_stream().cuda_stream
    xp = torch.stack((xs[:, :40], xs[:, 20:60])).contiguous()
    (ya, yb) = (torch.zeros((2, 40, 40), device=dev()), torch.zeros((2, 40, 40), device=dev()))
    with torch.cuda.device(dev()):
        opc.spmm_planes(xp.data_ptr(), 40, 30 * 40, 2, 40, ya.data_ptr(), 40, 40 * 40, EXACT | TILE64, st)
        opc.spmm_planes(xp.data_ptr(), 40, 30 * 40, 2, 40, yb.data_ptr(), 40, 40 * 40, EXACT, st)
    assert torch.equal(ya, yb) and bool(ya.abs().max() > 0)
    with torch.cuda.device(dev()):
        op64 = ksp.SparseMatrix(A.astype(np.float64))._device_op(dev())
        assert op64.plan(40, EXACT | TILE64) == op64.plan(40, EXACT)
        (ya, yb) = (torch.empty((40, 40), dtype=torch.float64, device=dev()), torch.empty((40, 40), dtype=torch.float64, device=dev()))
        xc = xs[:, :40].contiguous()
        op64.spmm_f64(xc.data_ptr(), 40, 40, ya.data_ptr(), 40, EXACT | TILE64, st)
        op64.spmm_f64(xc.data_ptr(), 40, 40, yb.data_ptr(), 40, EXACT, st)
    assert torch.equal(ya, yb)
    Dm = np.random.RandomState(4).randn(ksp.SparseMatrix.DENSE_MIN_ELEMENTS // 4097 + 2, 4097).astype(np.float32)      # a keyed Linear: homogeneous last row
    Dm[-1] = 0
    Dm[-1, -1] = 1
    with torch.cuda.device(dev()):
        opd = ksp.SparseMatrix(scipy.sparse.csr_matrix(Dm))._dense_device_op(dev())
    assert opd is not None
    xdn = torch.as_tensor(np.random.RandomState(5).randn(4097, 40).astype(np.float32)).to(dev())
    for flags in (0, MFMA | N64, MFMA | N32 | N64 | RELU):
        (y1, _, p1) = _spmm(opd, xdn, 40, flags | N64M)
        (yf, _, pf) = _spmm(opd, xdn, 40, flags)
        assert p1 == pf and torch.equal(y1, yf), (flags, p1, pf)


@pytest.mark.parametrize('contract', [True, False, 'auto', 'bf16x3'])
def test_launch_takes_the_wide_decision_not_the_narrow_record(contract):
    """A layer calibration put on the matrix cores whose narrow='mfma' measurement said 'exact': the 64-column tile is the wide kernel's association, so launch() with
    narrow64='mfma' names the tile under the wide decision, whatever the narrow record says."""
    c = KeyedLayer.fromoperator(_tiny_conv(), 'Conv2d', exact=contract)
    if contract in (False, 'bf16x3'):
        c._contract_record = dict(decided='mfma', max_abs_x=1.0, narrow=dict(decided='exact', max_abs_x=1.0))
        assert c.screened() and c.narrow_mode('mfma') is True
    la = c.launch(dev(), relu=True, narrow='mfma', narrow64='mfma')
    if contract in (False, 'bf16x3'):
        assert la.flags == RELU | TILE64
    else:
        assert la.flags == c.launch(dev(), relu=True, narrow=True, narrow64=True).flags and la.flags & NARROW and not la.flags & (MFMA | N64M)


KW = dict(narrow='mfma', narrow64='mfma')


def _tile_layers(knet):
    return [(n, c) for (n, c) in _conv_layers(knet) if c._exact in (False, 'bf16x3')]


@pytest.mark.parametrize('mode', [False, 'auto'])
@pytest.mark.parametrize('name', ['mini_tiled_permutation.npz', 'mini_tiled_stochastic.npz'])
def test_whole_keynets_equal_the_padded_forward(golden, name, mode):
    """exact_mode(False) / exact_mode('auto'), 33 / 48 / 64 images: the logits of forward_linear(narrow='mfma', narrow64='mfma') are the padded forward's of the same
    images, bit for bit (a key-net with a layer decided 'split' runs that layer on the order-preserving pipeline instead: inside the gate of the float-key contract);
    nothing is padded to 128, decided or recorded; the layers on the f32 tiles plan the 64-column kernel.  At 32 images the call is narrow32=True."""
    z = golden(name)
    knet = kio.keynet_from_arrays(z)
    knet.exact_mode(mode)
    for n in (33, 48, 64):
        x = torch.as_tensor(_tiled(z, n)).to(dev())
        full = knet.forward_linear(x)                                 # (the first one decides an 'auto' key-net)
        before = copy.deepcopy(knet.contract_report())
        assert not before['undecided']
        knet._padded_forwards = 0
        y = knet.forward_linear(x, **KW)
        assert knet._padded_forwards == 0 and knet.contract_report() == before
        assert y.shape == full.shape
        if any(c._exact == 'split' for (_, c) in _conv_layers(knet)):
            assert gate(y, full)[0] <= 2, (n, gate(y, full))           # (two re-ordered results against each other: each inside the gate against the stored order)
        else:
            assert torch.equal(y, full), (n, float((y - full).abs().max()))
        assert torch.equal(knet.forward(x, **KW), knet.forward(x)) or any(c._exact == 'split' for (_, c) in _conv_layers(knet))
        for (lname, c) in _tile_layers(knet):
            la = c.launch(dev(), relu=False, **KW)
            assert la.flags & TILE64 == TILE64 and not la.flags & (EXACT | BF16X3 | NARROW)
            with torch.cuda.device(dev()):
                assert 'NB=64' in la.op.plan(64, la.flags), lname
        if mode is False:
            assert _tile_layers(knet)
    x32 = torch.as_tensor(_tiled(z, 32)).to(dev())
    assert torch.equal(knet.forward_linear(x32, **KW), knet.forward_linear(x32, narrow='mfma', narrow32=True))


@pytest.mark.parametrize('name', ['mini_tiled_permutation.npz', 'mini_tiled_identity.npz'])
def test_under_the_default_contract_the_call_is_the_order_preserving_one(golden, name):
    z = golden(name)
    knet = kio.keynet_from_arrays(z)
    assert not _tile_layers(knet)
    for n in (33, 64):
        x = torch.as_tensor(_tiled(z, n)).to(dev())
        assert torch.equal(knet.forward_linear(x, **KW), knet.forward_linear(x, narrow=True, narrow64=True))


def test_a_batch_beyond_the_calibrated_magnitude_sends_the_layers_back_to_auto(golden):
    """A calibrated key-net, then 40 images scaled past RESCREEN_FACTOR x the calibrated max |x|: the screened layers are 'auto' again (nothing calibrates inside this
    path), the pass ran again with them in the stored order, and the logits are the stored-order forward's.  The next padded forward decides them."""
    z = golden('mini_tiled_permutation.npz')
    knet = kio.keynet_from_arrays(z)
    knet.exact_mode('auto')
    x = torch.as_tensor(_tiled(z, 40)).to(dev())
    knet.forward_linear(x)
    tiles = [lname for (lname, c) in _tile_layers(knet) if c.screened()]
    assert tiles, 'no conv layer of the key-net was put on the matrix cores by calibration'
    ref = kio.keynet_from_arrays(z)
    ref.exact_mode(True)
    xs = (x * (2.5 * KeyedLayer.RESCREEN_FACTOR)).contiguous()
    y = knet.forward_linear(xs, **KW)
    tripped = [lname for (lname, c) in _conv_layers(knet) if lname in tiles and c._exact == 'auto']
    assert tripped, 'no layer tripped its screen'
    assert all(c._exact in (True, 'auto') for (_, c) in _conv_layers(knet)) and torch.equal(y, ref.forward_linear(xs))
    knet.forward_linear(xs)
    assert not knet.contract_report()['undecided']


def test_capture(golden):
    z = golden('mini_tiled_permutation.npz')
    knet = kio.keynet_from_arrays(z)
    knet.exact_mode(False)
    x = torch.as_tensor(_tiled(z, 48)).to(dev())
    replay = knet.capture(x, **KW)
    other = (x.flip(0) * 0.5).contiguous()
    for xi in (x, other):
        eager = knet.forward_linear(xi, **KW)
        assert torch.equal(replay(xi).clone(), eager) and torch.equal(eager, knet.forward_linear(xi))
    assert getattr(replay, 'graph', None) is not None


def test_argument_rules(golden):
    z = golden('mini_tiled_permutation.npz')
    knet = kio.keynet_from_arrays(z)
    x65 = torch.as_tensor(_tiled(z, 65)).to(dev())
    for call in (knet.forward_linear, knet.forward, knet.capture):
        with pytest.raises(ValueError):
            call(x65[:40], narrow=True, narrow64='mfma')            # only together with narrow='mfma'
        with pytest.raises(ValueError):
            call(x65[:40], narrow64='mfma')
        with pytest.raises(ValueError):
            call(x65, **KW)                                          # 65 images
        with pytest.raises(ValueError, match='matrix-core'):
            call(x65[:33], narrow='mfma', narrow64=True)             # True keeps its meaning
    W = _conv_layers(knet)[0][1].W
    with pytest.raises(ValueError):
        W.torchdot(torch.zeros((W.shape[1], 40), device=dev()), exact=False, narrow=True, narrow64='mfma')
    y = W.torchdot(torch.ones((W.shape[1], 40), device=dev()), exact=False, **KW)
    assert gate(y, W.torchdot(torch.ones((W.shape[1], 40), device=dev()), exact=True))[0] <= 1
