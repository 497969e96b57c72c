"""The tap-resident channel-lane kernel for 1 .. 8 batch columns (KN_FLAG_NARROW_TAPS next to KN_FLAG_NARROW; narrow_taps=True next to narrow=True | 'mfma'):
every check is bit for bit -- against scipy's csr_matvecs on the sorted expansion (the oracle), against the same call without the flag / keyword, and against the
first columns of the 128-column order-preserving product.

The operators come from test_parity_gpu._random_convtaps, as in tests/test_narrow_gpu.py.  That generator's operators WITH coefficients (unit=False) put two
slots on one (output, input) pixel pair (the float-weighted second entry of tap (i, j) lands on the input pixel of tap (i, j + 1)) and hold up to 18 slots per
pixel: summed stored values, which the new kernel does not take.  So the coefficient shapes are here twice: `_coef_convtaps` gives the unit operator of the
same shape random coefficients (about half exactly 1), one slot per pixel pair -- ELIGIBLE, the new kernel must run; and the generator's own unit=False
operators of the same shapes sit with the ineligible ones, where the flag must change neither plan nor bits."""
import numpy as np
import pytest
import torch

from keynet_amd import io as kio
from keynet_amd import sparse as ksp
from keynet_amd import system as ksys
from keynet_amd import _capi
from keynet_amd.layer import KeyedLayer
from test_parity_gpu import _random_convtaps, dev
from test_narrow_gpu import _sorted_csr, _oracle, _dropped_zero_operator, _last
from narrow_helpers import _spmm, _spmm_calls, SENTINEL

pytestmark = pytest.mark.gpu


def _keynet(z, name, monkeypatch):
    """The file's key-net; the untiled AllConvNet-shaped one is keyed again from the file's weights with the reference's seed (tests/test_host_keying.py) and without
    the size threshold of the factored form (tests/test_factored_untiled.py), which is what puts its conv layers behind the first on the factored device form --
    loaded from the arrays they are plain CSR containers."""
    if name.startswith('allconv'):
        from nets import TinyAllConv, load_weights
        monkeypatch.setattr(KeyedLayer, 'FACTOR_UNTILED_MIN_NNZ', 0)
        np.random.seed(0)
        return ksys.PermutationKeynet((3, 16, 16), load_weights(TinyAllConv(), z))[1]
    return kio.keynet_from_arrays(z)

(RELU, EXACT, BF16X3, NARROW, MFMA, NARROW32, TAPS) = (_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_BF16X3, _capi.KN_FLAG_NARROW, _capi.KN_FLAG_NARROW_MFMA,
                                                      _capi.KN_FLAG_NARROW32, _capi.KN_FLAG_NARROW_TAPS)
NEW = 'convtaps_narrow_taps_kernel'
OLD = 'convtaps_narrow_kernel'


def _coef_convtaps(rng, Cin, Cout, H, k, stride, has_last, unit=False, ntaps=None):
    """_random_convtaps' unit operator with random coefficients on its entries (about half stay exactly 1): no (output, input) pixel pair is hit twice.
    `ntaps` (10 .. 16): the operator gets that many taps, and the entries of output pixel o take tap (t + o) mod ntaps for t -- still at most nine slots and nine
    distinct taps per pixel, every tap index in use."""
    U = _random_convtaps(rng, Cin, Cout, H, k, stride, True, has_last)
    t = U._taps
    (taps, et) = (t['taps'], t['ent_tap'])
    if ntaps is not None:
        taps = (rng.randn(ntaps, Cout, Cin) / np.sqrt(9 * Cin)).astype(np.float32)
        et = (et + t['ent_out']) % ntaps
        assert len(np.unique(et)) == ntaps
    ec = None if unit else np.where(rng.rand(len(t['ent_out'])) < 0.5, 1.0, rng.randn(len(t['ent_out']))).astype(np.float32)
    return ksp.Conv2dTiledMatrix.fromtaps(U._inshape, U._outshape, taps, t['ent_out'], t['ent_in'], et, ec, t['lastcol'])


# (id, Cin, Cout, H, k, stride, unit coefficients, bias column)
SHAPES = [
    ('3x3-s1-cin3-cout24-h7-bias', 3, 24, 7, 3, 1, True, True),          # 49 pixels: no multiple of a pixel group or of four; masked lanes
    ('3x3-s2-cin5-cout64-nobias', 5, 64, 8, 3, 2, True, False),          # strided: pixels of 4, 6 and 9 slots
    ('3x3-s1-cin16-cout192-coef-bias', 16, 192, 8, 3, 1, False, True),   # three channel blocks
    ('3x3-s1-cin3-cout64-coef-nobias', 3, 64, 8, 3, 1, False, False),
    ('1x1-cin8-cout8-h4', 8, 8, 4, 1, 1, True, True),                    # one slot per pixel, one tap
    ('factored-dropped-zeros', 16, 24, 8, 3, 1, True, True),             # zero guard
    ('3x3-s1-cin5-cout72-13taps-bias', 5, 72, 6, 3, 1, True, True),      # 13 taps, nine per pixel: the 16-row forms, padded value-row loads, tap indices above 8
    ('3x3-s2-cin7-cout24-16taps-coef-nobias', 7, 24, 8, 3, 2, False, False),
]
INELIGIBLE = [
    ('filled-9x9-cin3-cout64', 3, 64, 12, 9, 1, False, True),            # summed stored values, 81 taps
    ('7x7-cin3-cout64', 3, 64, 8, 7, 1, True, True),                     # 49 taps, 49 slots
    ('3x3-s1-cin16-cout192-coef-dups', 16, 192, 8, 3, 1, False, True),   # the generator's coefficient operators: two slots on a pixel pair
    ('3x3-s1-cin3-cout64-coef-dups', 3, 64, 8, 3, 1, False, False),
]
_built = {}


def _build(case, seed=5):
    """(W, sorted CSR, X [cols, 128], oracle product at 8 columns): built once per case and shared, never modified."""
    key = (case, seed)
    if key not in _built:
        (tag, Cin, Cout, H, k, stride, unit, has_last) = case
        rng = np.random.RandomState(seed)
        if tag.startswith('factored'):
            (W, M) = _dropped_zero_operator(rng, Cin, Cout, H)
        else:
            if 'taps' in tag:
                W = _coef_convtaps(rng, Cin, Cout, H, k, stride, has_last, unit=unit, ntaps=int(tag.split('taps')[0].split('-')[-1]))
            elif unit or 'dups' in tag or tag.startswith('filled'):
                W = _random_convtaps(rng, Cin, Cout, H, k, stride, unit, has_last)
            else:
                W = _coef_convtaps(rng, Cin, Cout, H, k, stride, has_last)
            M = _sorted_csr(W)
        X = rng.randn(W.shape[1], 128).astype(np.float32)
        if has_last:
            X[-1] = 1.0
        _built[key] = (W, M, X, _oracle(M, X[:, :8]))
    return _built[key]


@pytest.mark.parametrize('n_vecs', [1, 2, 3, 5, 8])
@pytest.mark.parametrize('case', SHAPES, ids=[c[0] for c in SHAPES])
def test_taps_kernel_against_the_oracle_the_narrow_kernel_and_the_128_column_product(case, n_vecs):
    (W, M, X, ref8) = _build(case)
    xd = torch.as_tensor(X).to(dev())
    with torch.cuda.device(dev()):
        op = W._device_op(dev())
        plan = op.plan(n_vecs, EXACT | NARROW | TAPS)
        plain = op.plan(n_vecs, EXACT | NARROW)
    assert OLD in plain and NEW not in plain, plain
    _names_the_new_kernel(case, n_vecs, plan)
    ref = ref8[:, :n_vecs]
    for relu in (False, True):
        y = W.torchdot(xd[:, :n_vecs], relu=relu, exact=True, narrow=True, narrow_taps=True)
        assert np.array_equal(y.cpu().numpy(), np.maximum(ref, 0) if relu else ref), (case[0], n_vecs, relu, float(np.abs(y.cpu().numpy() - ref).max()))
        assert torch.equal(y, W.torchdot(xd[:, :n_vecs], relu=relu, exact=True, narrow=True))
    y = W.torchdot(xd[:, :n_vecs], exact=True, narrow=True, narrow_taps=True)
    assert torch.equal(y, W.torchdot(xd, exact=True)[:, :n_vecs])


def _names_the_new_kernel(case, n_vecs, plan):
    assert NEW in plan and OLD not in plan, plan
    assert 'P=1' in plan and ('%d value rows' % (16 if 'taps' in case[0] else 9)) in plan, plan      # (these operators are far below the pixel-pair rule: test_pixel_pairs)
    assert (', coef' in plan) == ('coef' in case[0]), plan
    if 'coef' in case[0] and n_vecs > 4:                                # no 8-column form with coefficients: columns 0 .. 3 and the other n - 4, two launches of the new kernel
        rest = n_vecs - 4
        assert plan.count(NEW) == 2 and 'NV=4, coef, columns 0 .. 3' in plan and 'NV=8' not in plan, plan
        assert ('NV=%d%s, coef, columns 4 ..' % (1 if rest == 1 else 4, '' if rest in (1, 4) else ', masked to %d' % rest)) in plan, plan
    else:
        assert plan.count(NEW) == 1 and ('NV=%d' % (1 if n_vecs == 1 else 2 if n_vecs == 2 else 4 if n_vecs <= 4 else 8)) in plan, plan
        assert ('masked to %d' % n_vecs in plan) == (n_vecs in (3, 5)), plan


# The launch rule of the pixel pairs: P = 2 where ceil(pixels / 2) x channel blocks >= 4 096, for NV <= 2 without coefficients.  The sizes are the smallest that cross it with
# an ODD pixel count (the last group holds one pixel): 91 x 91 = 8 281 pixels -> 4 141 pairs; 90 x 90 = 8 100 -> 4 050 is just below.
PAIRS = [
    ('3x3-s1-cin2-cout64-h91', 2, 64, 91, 3, 1, True, True),             # (Cout 64: every lane stores)
    ('3x3-s2-cin3-cout40-h182-nobias', 3, 40, 182, 3, 2, True, False),   # strided: the pixels of a pair hold 4, 6 or 9 slots; masked lanes; 91 x 91 output pixels
]


@pytest.mark.parametrize('case', PAIRS, ids=[c[0] for c in PAIRS])
def test_pixel_pairs(case):
    (W, M, X, ref8) = _build(case)
    assert (W.shape[0] - (1 if case[7] else 0)) // case[2] == 8281
    xd = torch.as_tensor(X[:, :4]).to(dev())
    with torch.cuda.device(dev()):
        op = W._device_op(dev())
    for n in (1, 2, 3):
        for relu in (0, RELU):
            (y, _, plan) = _spmm(op, xd, n, EXACT | NARROW | TAPS | relu)
            assert NEW in plan and (('P=2' if n <= 2 else 'P=1') in plan), plan          # (three columns run NV = 4: one pixel per wavefront)
            ref = ref8[:, :n]
            assert np.array_equal(y.cpu().numpy(), np.maximum(ref, 0) if relu else ref), (case[0], n, relu)
            assert torch.equal(y, _spmm(op, xd, n, EXACT | NARROW | relu)[0])
    Xn = X[:, :2].copy()                                                # a NaN and an Inf: they reach the outputs that hold them, in either pixel of a pair, and no other
    rows = np.random.RandomState(3).choice(W.shape[1] - 1, size=2, replace=False)
    Xn[rows[0], 0] = np.nan
    Xn[rows[1], 1] = np.inf
    xn = torch.as_tensor(Xn).to(dev())
    (y, _, plan) = _spmm(op, xn, 2, NARROW | TAPS)
    assert 'P=2' in plan and torch.equal(y.view(torch.int32), _spmm(op, xn, 2, NARROW)[0].view(torch.int32))
    assert np.array_equal(np.isnan(y.cpu().numpy()), np.isnan(_oracle(M, Xn)))


def test_the_pixel_pair_rule_from_both_sides():
    """Plans only: 4 050 pairs stay at one pixel per wavefront, 4 141 take two; with coefficients, and from NV = 4 on, always one."""
    rng = np.random.RandomState(4)
    below = _random_convtaps(rng, 1, 64, 90, 3, 1, True, False)
    coef = _coef_convtaps(rng, 1, 64, 91, 3, 1, False)
    above = _build(PAIRS[0])[0]
    with torch.cuda.device(dev()):
        for n in (1, 2):
            assert 'P=1' in below._device_op(dev()).plan(n, NARROW | TAPS) and NEW in below._device_op(dev()).plan(n, NARROW | TAPS)
            assert 'P=2' in above._device_op(dev()).plan(n, NARROW | TAPS)
            assert 'P=1' in coef._device_op(dev()).plan(n, NARROW | TAPS) and ', coef' in coef._device_op(dev()).plan(n, NARROW | TAPS)
        for n in (3, 4, 8):
            assert 'P=1' in above._device_op(dev()).plan(n, NARROW | TAPS)


@pytest.mark.parametrize('case', INELIGIBLE, ids=[c[0] for c in INELIGIBLE])
def test_ineligible_operators_keep_plan_and_bits(case):
    (W, M, X, ref8) = _build(case)
    xd = torch.as_tensor(X).to(dev())
    with torch.cuda.device(dev()):
        op = W._device_op(dev())
    for n in (1, 3, 8):
        for flags in (NARROW, EXACT | NARROW | RELU):
            (y1, _, p1) = _spmm(op, xd, n, flags | TAPS)
            (y0, _, p0) = _spmm(op, xd, n, flags)
            assert p1 == p0 and OLD in p1 and NEW not in p1, (n, p1, p0)
            assert torch.equal(y1, y0)
        assert np.array_equal(_spmm(op, xd, n, NARROW | TAPS)[0].cpu().numpy(), ref8[:, :n])


def test_flag_semantics():
    """A modifier of regime NARROW and of nothing else."""
    (W, M, X, _) = _build(('semantics', 16, 64, 8, 3, 1, True, True), seed=9)
    xd = torch.as_tensor(X).to(dev())
    with torch.cuda.device(dev()):
        op = W._device_op(dev())
    for n in (1, 4, 8, 64):
        for flags in (0, EXACT, RELU, BF16X3):                          # alone
            (y1, _, p1) = _spmm(op, xd, n, flags | TAPS)
            (y0, _, p0) = _spmm(op, xd, n, flags)
            assert p1 == p0 and NEW not in p1 and torch.equal(y1, y0), (n, flags, p1, p0)
    for flags in (NARROW, NARROW | EXACT, NARROW | NARROW32, NARROW | NARROW32 | EXACT):      # nine columns
        (y1, _, p1) = _spmm(op, xd, 9, flags | TAPS)
        (y0, _, p0) = _spmm(op, xd, 9, flags)
        assert p1 == p0 and NEW not in p1 and torch.equal(y1, y0), (flags, p1, p0)
    for n in (1, 4, 8):                                                 # with KN_FLAG_NARROW32 at 8 columns and fewer the regime is NARROW: the kernel runs
        (y1, _, p1) = _spmm(op, xd, n, NARROW | NARROW32 | TAPS)
        assert NEW in p1 and torch.equal(y1, _spmm(op, xd, n, NARROW)[0]), p1
    for n in (1, 5, 8):                                                 # the matrix-core regime keeps its kernel; with KN_FLAG_EXACT the flag means KN_FLAG_NARROW
        (y1, _, p1) = _spmm(op, xd, n, MFMA | TAPS)
        (y0, _, p0) = _spmm(op, xd, n, MFMA)
        assert 'convtaps_narrow_mfma_kernel' in p0 and p1 == p0 and torch.equal(y1, y0), (n, p1, p0)
        (ye, _, pe) = _spmm(op, xd, n, MFMA | EXACT | TAPS)
        assert NEW in pe and torch.equal(ye, _spmm(op, xd, n, NARROW | EXACT)[0]), pe
    import scipy.sparse
    A = scipy.sparse.random(40, 30, density=0.3, format='csr', dtype=np.float32, random_state=3)       # a CSR handle
    S = ksp.SparseMatrix(A)
    xs = torch.as_tensor(np.random.RandomState(2).randn(30, 8).astype(np.float32)).to(dev())
    with torch.cuda.device(dev()):
        cs = S._device_op(dev())
    for flags in (EXACT, EXACT | NARROW):
        (y1, _, p1) = _spmm(cs, xs, 4, flags | TAPS)
        (y0, _, p0) = _spmm(cs, xs, 4, flags)
        assert p1 == p0 and torch.equal(y1, y0)


@pytest.mark.parametrize('case', [SHAPES[0], SHAPES[2]], ids=lambda c: c[0])
@pytest.mark.parametrize('n', [1, 3, 4, 8])
def test_column_window_of_a_wider_block_through_the_c_abi(case, n):
    """n columns from column 3 of a 128-wide block (ldx = ldy = 128): the narrow kernel's window, the oracle, and the sentinel everywhere else."""
    (W, M, X, _) = _build(case)
    xd = torch.as_tensor(X).to(dev())
    with torch.cuda.device(dev()):
        op = W._device_op(dev())
    for relu in (0, RELU):
        (win, whole, plan) = _spmm(op, xd, n, EXACT | NARROW | TAPS | relu, ld=128, start=3)
        assert NEW in plan and OLD not in plan and plan.count(NEW) == (2 if ('coef' in case[0] and n > 4) else 1), plan
        assert torch.equal(win, _spmm(op, xd, n, EXACT | NARROW | relu, ld=128, start=3)[0])
        ref = _oracle(M, X[:, 3:3 + n])
        assert np.array_equal(win.cpu().numpy(), np.maximum(ref, 0) if relu else ref)
        outside = torch.ones(128, dtype=torch.bool, device=dev())
        outside[3:3 + n] = False
        assert bool(torch.all(whole[:, outside] == SENTINEL))


@pytest.mark.parametrize('case', [SHAPES[0], SHAPES[1], SHAPES[2], SHAPES[5]], ids=lambda c: c[0])
def test_non_finite_activations(case):
    """One NaN and one Inf activation: the int32 views of the result equal the narrow kernel's, and the oracle's NaN pattern -- a slot the lists do not hold
    contributes nothing, so the non-finite values reach only the outputs that hold them."""
    (W, M, X, _) = _build(case)
    rng = np.random.RandomState(21)
    for n in (1, 5, 8):
        Xn = X[:, :n].copy()
        rows = rng.choice(W.shape[1] - 1, size=2, replace=False)
        Xn[rows[0], 0] = np.nan
        Xn[rows[1], n - 1] = np.inf
        xd = torch.as_tensor(Xn).to(dev())
        ref = _oracle(M, Xn)
        for relu in (False, True):
            y = W.torchdot(xd, relu=relu, exact=True, narrow=True, narrow_taps=True)
            y0 = W.torchdot(xd, relu=relu, exact=True, narrow=True)
            assert torch.equal(y.view(torch.int32), y0.view(torch.int32)), (case[0], n, relu)
            assert np.array_equal(np.isnan(y.cpu().numpy()), np.isnan(ref)), (case[0], n, relu)


@pytest.mark.parametrize('name', ['mini_tiled_permutation.npz', 'mini_tiled_permutation8.npz', 'mini_tiled_identity.npz', 'allconv_tiny_perm.npz', 'mini_tiled_stochastic.npz'])
def test_whole_keynets(golden, name, monkeypatch):
    """forward_linear(narrow=True, narrow_taps=True) == forward_linear(narrow=True) at 1, 3 and 8 images, and the reference's vectors where the file's key-net is under
    the bit-exact contract; the recorded kn_spmm calls carry the flag on the conv layers (eligible: the new kernel; the layers of the stochastic net,
    ineligible: the channel-lane kernel) and on nothing else."""
    z = golden(name)
    knet = _keynet(z, name, monkeypatch)
    x = torch.as_tensor(z['x_cipher'].astype(np.float32)).to(dev())
    if 'stochastic' not in name:
        knet.exact_mode(True)
    else:
        knet.forward_linear(x)                                          # (calibrates)
    for n in (1, 3, 8):
        xi = x[torch.arange(n) % x.shape[0]].contiguous()
        y = knet.forward_linear(xi, narrow=True, narrow_taps=True)
        assert torch.equal(y, knet.forward_linear(xi, narrow=True)), (name, n)
    if 'stochastic' not in name:
        m = min(8, int(x.shape[0]))
        assert np.array_equal(knet.forward_linear(x[:m], narrow=True, narrow_taps=True).cpu().numpy(), _last(z)[:m])
    convs = sum(1 for c in knet._keyed() if c.W.narrow_capable())
    calls = _spmm_calls(monkeypatch)
    knet.forward_linear(x[:1], narrow=True, narrow_rows=True, narrow_taps=True)
    flagged = [(p, f) for (p, f) in calls if f & TAPS]
    assert len(flagged) == convs > 0, (name, len(flagged), convs)
    for (p, f) in calls:
        assert bool(f & TAPS) == bool(f & NARROW), (p, f)
        assert (NEW in p or OLD in p) == bool(f & TAPS), (p, f)
    new = sum(1 for (p, f) in flagged if NEW in p)
    if 'stochastic' in name:      # both conv layers of this file hold more than nine slots per output pixel: flagged, ineligible, the channel-lane kernel
        assert new == 0 and all(OLD in p for (p, f) in flagged), [p for (p, f) in flagged]
        for c in knet._keyed():
            if c.W.narrow_capable():
                assert int(np.diff(c.W.tosparse('csr').indptr).max()) > 9 * c.W._inshape[0] + 1      # a row meets more than nine input pixels per channel (+ the bias entry)
    else:
        assert new == convs, [p for (p, f) in flagged]
    del calls[:]
    knet.forward_linear(x[:1], narrow=True)                             # without the keyword: no call carries the flag
    assert calls and not any(f & TAPS for (p, f) in calls)


def test_narrow_mfma_forward_flags_the_layers_on_the_channel_lane_kernel(golden, monkeypatch):
    """Inside a narrow='mfma' forward the layers under True get the flag too, the layers on the matrix-core kernel do not; with narrow_split=True it combines."""
    z = golden('mini_tiled_permutation.npz')
    knet = kio.keynet_from_arrays(z)
    x = torch.as_tensor(z['x_cipher'].astype(np.float32)).to(dev())
    knet.exact_mode(True)
    want = knet.forward_linear(x[:3], narrow=True)
    calls = _spmm_calls(monkeypatch)
    assert torch.equal(knet.forward_linear(x[:3], narrow='mfma', narrow_taps=True), want)
    assert any(f & TAPS and NEW in p for (p, f) in calls) and not any(f & MFMA for (p, f) in calls)
    assert torch.equal(knet.forward_linear(x[:3], narrow='mfma', narrow_taps=True, narrow_split=True), want)


@pytest.mark.parametrize('name', ['mini_tiled_permutation.npz', 'allconv_tiny_perm.npz'])
def test_capture_replays_the_eager_forward(golden, name, monkeypatch):
    z = golden(name)
    knet = _keynet(z, name, monkeypatch)
    x = torch.as_tensor(z['x_cipher'].astype(np.float32)).to(dev())
    knet.exact_mode(True)
    x4 = x[torch.arange(4) % x.shape[0]].contiguous()
    replay = knet.capture(x4, narrow=True, narrow_taps=True)
    other = (x4.flip(0) * 0.5).contiguous()
    for xi in (x4, other):
        eager = knet.forward_linear(xi, narrow=True, narrow_taps=True)
        assert torch.equal(replay(xi).clone(), eager)
        assert torch.equal(eager, knet.forward_linear(xi, narrow=True))


def test_the_keyword_needs_narrow(golden):
    z = golden('mini_tiled_permutation.npz')
    knet = kio.keynet_from_arrays(z)
    x = torch.as_tensor(z['x_cipher'].astype(np.float32)).to(dev())
    for call in (knet.forward_linear, knet.forward, knet.capture):
        with pytest.raises(ValueError):
            call(x[:1], narrow_taps=True)
        with pytest.raises(ValueError):
            call(x[:1], narrow_rows=True, narrow_taps=True)
    with pytest.raises(ValueError):
        knet.forward_linear(x[torch.arange(9) % x.shape[0]], narrow=True, narrow_taps=True)       # the widths are those of `narrow`
    (W, _, X, _) = _build(SHAPES[0])
    with pytest.raises(ValueError):
        W.torchdot(torch.as_tensor(X[:, :2]).to(dev()), exact=True, narrow_taps=True)
    y = knet.forward_linear(x[torch.arange(9) % x.shape[0]], narrow=True, narrow32=True, narrow_taps=True)      # valid beyond 8 images, where it changes nothing
    assert torch.equal(y, knet.forward_linear(x[torch.arange(9) % x.shape[0]], narrow=True, narrow32=True))


def test_fuzz_random_3x3_operators_against_the_oracle():
    """Seeded: 36 random 3 x 3 operators (Cin 1 .. 20, Cout 1 .. 200, H 3 .. 9, stride 1 | 2, coefficients or not, bias or not) at a random width 1 .. 8."""
    rng = np.random.RandomState(1515)
    for it in range(36):
        (Cin, Cout, H) = (int(rng.randint(1, 21)), int(rng.randint(1, 201)), int(rng.randint(3, 10)))
        (stride, unit, has_last) = (int(rng.choice([1, 2])), bool(rng.rand() < 0.5), bool(rng.rand() < 0.6))
        if H // stride < 1:
            continue
        W = _random_convtaps(rng, Cin, Cout, H, 3, stride, True, has_last) if unit else _coef_convtaps(rng, Cin, Cout, H, 3, stride, has_last)
        n = int(rng.randint(1, 9))
        relu = bool(rng.rand() < 0.5)
        with torch.cuda.device(dev()):
            plan = W._device_op(dev()).plan(n, NARROW | TAPS | (RELU if relu else 0))
        assert NEW in plan and OLD not in plan and (unit or ', coef' in plan), (it, Cin, Cout, H, stride, unit, n, plan)
        X = rng.randn(W.shape[1], n).astype(np.float32)
        if has_last:
            X[-1] = 1.0
        ref = _oracle(_sorted_csr(W), X)
        y = W.torchdot(torch.as_tensor(X).to(dev()), relu=relu, exact=False, narrow=True, narrow_taps=True).cpu().numpy()
        assert np.array_equal(y, np.maximum(ref, 0) if relu else ref), (it, Cin, Cout, H, stride, unit, has_last, n, relu, float(np.abs(y - ref).max()))
