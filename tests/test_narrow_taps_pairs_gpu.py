"""The channel-pair tap-resident kernel for 1 .. 8 batch columns (KN_MODIFIER_NARROW_TAPS_PAIRS next to KN_FLAG_NARROW_TAPS under KN_FLAG_NARROW;
narrow_taps='pairs' next to narrow=True | 'mfma'): every check is bit for bit -- against scipy's csr_matvecs on the sorted expansion (the oracle), against the same
call with narrow_taps=True, and against the first columns of the 128-column order-preserving product.

The shapes are the smallest at which a lane that holds two output channels can go wrong: exactly one 128-channel block; a whole block and a trailing half block
(Cout 192: the second half re-reads the first half's value rows and stores nothing); a block whose second half holds 8 real channels (Cout 72, the 16-row form); two
blocks, the second with 72 channels, on a strided operator without a homogeneous row (pixels of 4, 6 and 9 slots; wavefronts that fetch column by column at the
masked widths); one slot and one tap per pixel; 49 pixels.  Operators of 64 output channels or fewer keep plan and bits."""
import numpy as np
import pytest
import torch

from keynet_amd import io as kio
from keynet_amd import sparse as ksp
from keynet_amd import system as ksys
from keynet_amd import _capi
import value_classes as vc
from test_parity_gpu import dev
from test_narrow_gpu import _oracle
from test_narrow_taps_gpu import SHAPES, INELIGIBLE, _build, _coef_convtaps, _keynet
from narrow_helpers import _spmm, _spmm_calls, SENTINEL

pytestmark = pytest.mark.gpu

(RELU, EXACT, NARROW, MFMA, NARROW32, TAPS, TAPS32, FILL, PAIRS) = (_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_NARROW, _capi.KN_FLAG_NARROW_MFMA, _capi.KN_FLAG_NARROW32,
                                                                   _capi.KN_FLAG_NARROW_TAPS, _capi.KN_MODIFIER_NARROW_TAPS32, _capi.KN_MODIFIER_NARROW_FILL,
                                                                   getattr(_capi, 'KN_MODIFIER_NARROW_TAPS_PAIRS', 0x2000))
NEW = 'convtaps_narrow_taps_pairs_kernel'
TAPS_KERNEL = 'convtaps_narrow_taps_kernel'
OLD = 'convtaps_narrow_kernel'
WIDTHS = [1, 2, 3, 4, 5, 7, 8]

# (id, Cin, Cout, H, k, stride, unit coefficients, bias column): test_narrow_taps_gpu._build's cases
WIDE = [
    [c for c in SHAPES if c[0] == '3x3-s1-cin16-cout192-coef-bias'][0],          # one whole block and a trailing half block, coefficients
    [c for c in SHAPES if c[0] == '3x3-s1-cin5-cout72-13taps-bias'][0],          # one block whose second half holds 8 real channels; the 16-row form
    ('3x3-s1-cin3-cout128-h8-bias', 3, 128, 8, 3, 1, True, True),                # exactly one block
    ('3x3-s2-cin5-cout200-16taps-nobias', 5, 200, 8, 3, 2, True, False),         # two blocks, the second with 72 channels; 4, 6 and 9 slots; no homogeneous row
    ('1x1-cin8-cout136-h4', 8, 136, 4, 1, 1, True, True),                        # one slot, one tap
    ('3x3-s1-cin4-cout130-h7-bias', 4, 130, 7, 3, 1, True, True),                # 49 pixels: not a multiple of four
]
NARROW_SHAPES = [c for c in SHAPES if c[2] <= 64]                                # Cout <= 64: the bit is not read
(COUT128, COUT200) = (WIDE[2], WIDE[3])
assert len(WIDE) == 6 and len(NARROW_SHAPES) >= 5


def _names_the_new_kernel(case, n_vecs, plan):
    assert NEW in plan and TAPS_KERNEL not in plan and OLD not in plan, plan
    assert ('%d value rows' % (16 if 'taps' in case[0] else 9)) in plan and 'lane = two output channels, taps resident, packed f32' in plan, plan
    assert (', coef' in plan) == ('coef' in case[0]), plan
    if 'coef' in case[0] and n_vecs > 4:                                # no 8-column form with coefficients: columns 0 .. 3 and the other n - 4, two launches of the new kernel
        rest = n_vecs - 4
        assert plan.count(NEW) == 2 and 'NV=4, coef, columns 0 .. 3' in plan and 'NV=8' not in plan, plan
        assert ('NV=%d%s, coef, columns 4 ..' % (1 if rest == 1 else 4, '' if rest in (1, 4) else ', masked to %d' % rest)) in plan, plan
    else:
        assert plan.count(NEW) == 1 and ('NV=%d' % (1 if n_vecs == 1 else 2 if n_vecs == 2 else 4 if n_vecs <= 4 else 8)) in plan, plan
        assert ('masked to %d' % n_vecs in plan) == (n_vecs in (3, 5, 7)), plan


@pytest.mark.parametrize('n_vecs', WIDTHS)
@pytest.mark.parametrize('case', WIDE, ids=[c[0] for c in WIDE])
def test_pairs_kernel_against_the_oracle_the_taps_kernel_and_the_128_column_product(case, n_vecs):
    (W, M, X, ref8) = _build(case)
    xd = torch.as_tensor(X).to(dev())
    with torch.cuda.device(dev()):
        op = W._device_op(dev())
        plan = op.plan(n_vecs, EXACT | NARROW | TAPS | PAIRS)
        taps = op.plan(n_vecs, EXACT | NARROW | TAPS)
    assert TAPS_KERNEL in taps and NEW not in taps, taps
    _names_the_new_kernel(case, n_vecs, plan)
    ref = ref8[:, :n_vecs]
    for relu in (False, True):
        y = W.torchdot(xd[:, :n_vecs], relu=relu, exact=True, narrow=True, narrow_taps='pairs')
        assert np.array_equal(y.cpu().numpy(), np.maximum(ref, 0) if relu else ref), (case[0], n_vecs, relu, float(np.abs(y.cpu().numpy() - ref).max()))
        assert torch.equal(y, W.torchdot(xd[:, :n_vecs], relu=relu, exact=True, narrow=True, narrow_taps=True))
    y = W.torchdot(xd[:, :n_vecs], exact=True, narrow=True, narrow_taps='pairs')
    assert torch.equal(y, W.torchdot(xd, exact=True)[:, :n_vecs])


@pytest.mark.parametrize('case', NARROW_SHAPES + INELIGIBLE, ids=[c[0] for c in NARROW_SHAPES + INELIGIBLE])
def test_narrow_and_ineligible_operators_keep_plan_and_bits(case):
    """Cout <= 64, and the operators the tap-resident kernels do not take (among them one of 192 output channels): the plan is the plan without the bit."""
    (W, M, X, ref8) = _build(case)
    xd = torch.as_tensor(X).to(dev())
    with torch.cuda.device(dev()):
        op = W._device_op(dev())
    for n in (1, 3, 8):
        for flags in (NARROW | TAPS, EXACT | NARROW | TAPS | RELU):
            (y1, _, p1) = _spmm(op, xd, n, flags | PAIRS)
            (y0, _, p0) = _spmm(op, xd, n, flags)
            assert p1 == p0 and NEW not in p1, (n, p1, p0)
            assert torch.equal(y1, y0)
        assert np.array_equal(_spmm(op, xd, n, NARROW | TAPS | PAIRS)[0].cpu().numpy(), ref8[:, :n])


_revalued = {}


def _regime_case(case, regime):
    """(W under the regime's operator values, its sorted CSR, X [cols, 8] under the regime): built once, never modified."""
    key = (case[0], regime)
    if key not in _revalued:
        (W, _, X, _) = _build(case)
        (W2, M2) = vc.revalued_convtaps(W, vc.variant_of(regime), seed=3)
        rng = np.random.RandomState(17)
        per_row = M2.nnz / float(M2.shape[0])
        _revalued[key] = (W2, M2, vc.REGIMES[regime].apply(X[:, :8], case[7], rng, per_row))
    return _revalued[key]


@pytest.mark.parametrize('regime', ['subnormal', 'boundary', 'underflow', 'overflow', 'signed-zero', 'by-column'])
@pytest.mark.parametrize('case', [COUT128, COUT200], ids=lambda c: c[0])
def test_value_classes(case, regime):
    """Operands, products and sums at the edges of float32, in both halves of a register pair: the bits of narrow_taps=True, and the oracle's."""
    (W, M, X) = _regime_case(case, regime)
    for n in (1, 8):
        Xn = np.ascontiguousarray(X[:, :n])
        xd = torch.as_tensor(Xn).to(dev())
        with np.errstate(all='ignore'):
            ref = _oracle(M, Xn)
        for relu in (False, True):
            y = W.torchdot(xd, relu=relu, exact=True, narrow=True, narrow_taps='pairs').cpu().numpy()
            y0 = W.torchdot(xd, relu=relu, exact=True, narrow=True, narrow_taps=True).cpu().numpy()
            vc.assert_bits_equal(y, y0, '%s %s n=%d relu=%s against narrow_taps=True' % (case[0], regime, n, relu))
            vc.assert_bits_equal(y, vc.relu_ref(ref) if relu else ref, '%s %s n=%d relu=%s against the oracle' % (case[0], regime, n, relu))
    with torch.cuda.device(dev()):
        assert NEW in W._device_op(dev()).plan(8, EXACT | NARROW | TAPS | TAPS32 | PAIRS)


@pytest.mark.parametrize('case', WIDE, ids=[c[0] for c in WIDE])
def test_non_finite_activations(case):
    """One NaN and one Inf activation: the int32 views of the result equal the tap-resident kernel's, and the oracle's NaN pattern -- a slot the lists do not hold
    contributes nothing, and the absent half of a trailing block is never a product 0 * x."""
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
            y = W.torchdot(xd, relu=relu, exact=True, narrow=True, narrow_taps='pairs')
            y0 = W.torchdot(xd, relu=relu, exact=True, narrow=True, narrow_taps=True)
            assert torch.equal(y.view(torch.int32), y0.view(torch.int32)), (case[0], n, relu)
            assert np.array_equal(np.isnan(y.cpu().numpy()), np.isnan(ref)), (case[0], n, relu)


@pytest.mark.parametrize('case', [WIDE[0], WIDE[1], COUT200], ids=lambda c: c[0])
@pytest.mark.parametrize('n', [1, 3, 4, 7, 8])
def test_column_window_of_a_wider_block_through_the_c_abi(case, n):
    """n columns from column 3 of a 128-wide block (ldx = ldy = 128): the tap-resident kernel's window, the oracle, and the sentinel everywhere else -- in the surplus
    columns and, with the y block two rows longer than the operator, behind the last row."""
    (W, M, X, _) = _build(case)
    xd = torch.as_tensor(X).to(dev())
    with torch.cuda.device(dev()):
        op = W._device_op(dev())
    (rows, _) = op.shape()
    for relu in (0, RELU):
        (win, whole, plan) = _spmm(op, xd, n, EXACT | NARROW | TAPS | PAIRS | relu, ld=128, start=3)
        assert plan.count(NEW) == (2 if ('coef' in case[0] and n > 4) else 1) and TAPS_KERNEL not in plan, plan
        assert torch.equal(win, _spmm(op, xd, n, EXACT | NARROW | TAPS | relu, ld=128, start=3)[0])
        ref = _oracle(M, X[:, 3:3 + n])
        assert np.array_equal(win.cpu().numpy(), np.maximum(ref, 0) if relu else ref)
        outside = torch.ones(128, dtype=torch.bool, device=dev())
        outside[3:3 + n] = False
        assert bool(torch.all(whole[:, outside] == SENTINEL))
        y = torch.full((rows + 2, 128), SENTINEL, dtype=torch.float32, device=dev())          # rows >= Cout * HoWo (+ the homogeneous row): nothing is written there
        with torch.cuda.device(dev()):
            op.spmm(xd.data_ptr() + 12, 128, n, y.data_ptr() + 12, 128, EXACT | NARROW | TAPS | PAIRS | relu, torch.cuda.current_stream().cuda_stream)
        assert torch.equal(y[:rows, 3:3 + n], win) and bool(torch.all(y[rows:] == SENTINEL)) and bool(torch.all(y[:rows][:, outside] == SENTINEL))


def test_flag_semantics():
    """A modifier of KN_FLAG_NARROW_TAPS in regime NARROW and of nothing else: everywhere else the same plan and the same bits as without the bit."""
    (W, M, X, _) = _build(('semantics-cout128', 16, 128, 8, 3, 1, True, True), seed=9)
    xd = torch.as_tensor(X).to(dev())
    with torch.cuda.device(dev()):
        op = W._device_op(dev())

    def same(n, flags, handle=op, x=xd):
        (y1, _, p1) = _spmm(handle, x, n, flags | PAIRS)
        (y0, _, p0) = _spmm(handle, x, n, flags)
        assert p1 == p0 and NEW not in p1 and torch.equal(y1, y0), (n, flags, p1, p0)
    for n in (1, 4, 8, 64):
        for flags in (0, EXACT, RELU):                                  # alone
            same(n, flags)
    for n in (1, 5, 8):
        for flags in (NARROW, NARROW | EXACT, NARROW | TAPS32):         # without KN_FLAG_NARROW_TAPS
            same(n, flags)
        (y1, _, p1) = _spmm(op, xd, n, NARROW | TAPS | PAIRS)           # with it: the kernel runs, with or without the other modifier
        assert NEW in p1 and torch.equal(y1, _spmm(op, xd, n, NARROW)[0]), p1
        assert _spmm(op, xd, n, NARROW | TAPS | TAPS32 | PAIRS)[2] == p1
        (ye, _, pe) = _spmm(op, xd, n, MFMA | EXACT | TAPS | PAIRS)     # with KN_FLAG_EXACT, KN_FLAG_NARROW_MFMA means KN_FLAG_NARROW
        assert NEW in pe and torch.equal(ye, y1), pe
    for n in (9, 32):                                                   # beyond 8 columns
        for flags in (NARROW | NARROW32 | TAPS, NARROW | NARROW32 | TAPS | TAPS32, NARROW | NARROW32 | TAPS | TAPS32 | EXACT):
            same(n, flags)
    for n in (1, 5, 8):                                                 # the matrix-core regime keeps its kernel
        (y0, _, p0) = _spmm(op, xd, n, MFMA | TAPS)
        assert 'convtaps_narrow_mfma_kernel' in p0
        same(n, MFMA | TAPS)
    from fuzz_narrow_cases import _filled, conv_props
    Wf = None                                                           # a filled-in operator of more than 64 output channels: KN_FLAG_NARROW_FILL takes the launch
    for seed in range(64):
        Wf = _filled(np.random.RandomState(seed), True, True)
        if conv_props(Wf)['Cout'] > 64 and conv_props(Wf)['fill_ok']:
            break
    assert conv_props(Wf)['Cout'] > 64 and conv_props(Wf)['fill_ok']
    Xf = np.random.RandomState(8).randn(Wf.shape[1], 8).astype(np.float32)
    Xf[-1] = 1.0
    xf = torch.as_tensor(Xf).to(dev())
    with torch.cuda.device(dev()):
        opf = Wf._device_op(dev())
    for n in (1, 8):
        assert 'convtaps_narrow_fill_kernel' in _spmm(opf, xf, n, NARROW | TAPS | FILL)[2]
        same(n, NARROW | TAPS | FILL, opf, xf)
    import scipy.sparse
    A = scipy.sparse.random(40, 30, density=0.3, format='csr', dtype=np.float32, random_state=3)       # a CSR handle
    S = ksp.SparseMatrix(A)
    xs = torch.as_tensor(np.random.RandomState(2).randn(30, 8).astype(np.float32)).to(dev())
    with torch.cuda.device(dev()):
        cs = S._device_op(dev())
    for flags in (EXACT, EXACT | NARROW | TAPS):
        same(4, flags, cs, xs)


def test_the_measured_losing_shapes_keep_the_tap_resident_kernel():
    """narrow_taps_pairs_loses (kn_internal.h, from the kernel trace of keyed VGG-16): with 128 input channels and more, a shape of fewer than 1 024 (pixel,
    128-channel block) wavefronts keeps convtaps_narrow_taps_kernel at every width, one of fewer than 4 096 up to 4 columns, one of fewer than 8 192 at 3 .. 4
    columns; the same shapes with fewer input channels are not in the rule.  Plans, and the bits of the one width at which the middle shape runs the new kernel."""
    from test_parity_gpu import _random_convtaps
    rng = np.random.RandomState(12)
    shapes = {'conv5': _random_convtaps(rng, 128, 512, 14, 3, 1, True, True),        # 196 pixels x 4 blocks = 784
              'conv4': _random_convtaps(rng, 128, 512, 28, 3, 1, True, False),       # 784 x 4 = 3 136
              'conv3': _random_convtaps(rng, 128, 256, 56, 3, 1, True, False),       # 3 136 x 2 = 6 272
              'conv5-cin64': _random_convtaps(rng, 64, 512, 14, 3, 1, True, True)}
    new_at = {'conv5': (), 'conv4': (5, 7, 8), 'conv3': (1, 2, 5, 7, 8), 'conv5-cin64': tuple(WIDTHS)}
    with torch.cuda.device(dev()):
        for (tag, W) in shapes.items():
            op = W._device_op(dev())
            for n in WIDTHS:
                (p1, p0) = (op.plan(n, NARROW | TAPS | PAIRS), op.plan(n, NARROW | TAPS))
                assert TAPS_KERNEL in p0 and NEW not in p0, (tag, n, p0)
                assert (NEW in p1) == (n in new_at[tag]), (tag, n, p1)
                assert p1 == p0 or n in new_at[tag], (tag, n, p1, p0)
    W = shapes['conv4']
    xd = torch.as_tensor(np.random.RandomState(13).randn(W.shape[1], 8).astype(np.float32)).to(dev())
    assert torch.equal(W.torchdot(xd, exact=True, narrow=True, narrow_taps='pairs'), W.torchdot(xd, exact=True, narrow=True, narrow_taps=True))


def test_the_bit_is_not_read_in_kn_spmm_planes():
    """kn_spmm_planes (CSR handles): two planes of 64 columns with the three tap bits and without -- the same result."""
    import scipy.sparse
    rng = np.random.RandomState(6)
    A = scipy.sparse.random(70, 30, density=0.2, format='csr', dtype=np.float32, random_state=rng)
    S = ksp.SparseMatrix(A)
    with torch.cuda.device(dev()):
        cs = S._device_op(dev())
    (n, planes) = (64, 2)
    xd = torch.as_tensor(rng.randn(planes * 30 * n).astype(np.float32)).to(dev())
    out = []
    for flags in (EXACT, EXACT | NARROW | TAPS | TAPS32 | PAIRS):
        yd = torch.full((planes * 70 * n,), SENTINEL, dtype=torch.float32, device=dev())
        with torch.cuda.device(dev()):
            assert cs.spmm_planes(xd.data_ptr(), n, 30 * n, planes, n, yd.data_ptr(), n, 70 * n, flags, torch.cuda.current_stream().cuda_stream) is True
        out.append(yd)
    assert torch.equal(out[0], out[1])
    ref = _oracle(A, xd.cpu().numpy()[:30 * n].reshape(30, n))
    assert np.array_equal(out[1].cpu().numpy()[:70 * n].reshape(70, n), ref)


def _wide_keynet():
    """A small tiled permutation key-net with conv layers of 72 and 136 output channels (input 2 x 8 x 8, tiles of 4)."""
    from torch import nn
    from keynet_amd.models import _Chain

    class WideNet(_Chain):
        flatten_before = 'fc1'

        def __init__(self):
            super(WideNet, self).__init__()
            self.conv1 = nn.Conv2d(2, 72, 3, stride=1, padding=1)
            self.relu1 = nn.ReLU()
            self.pool1 = nn.AvgPool2d(3, stride=2, padding=1)
            self.conv2 = nn.Conv2d(72, 136, 3, stride=1, padding=1)
            self.relu2 = nn.ReLU()
            self.pool2 = nn.AvgPool2d(3, stride=2, padding=1)
            self.fc1 = nn.Linear(136 * 2 * 2, 10)
    torch.manual_seed(0)
    net = WideNet().eval()
    np.random.seed(0)
    (sensor, knet) = ksys.TiledPermutationKeynet((2, 8, 8), net, 4)
    x = torch.randn(8, 2, 8, 8)
    xc = torch.cat([sensor.fromtensor(x[i:i + 1].to(dev())).encrypt().astensor() for i in range(8)], dim=0)
    return (knet, xc.contiguous())


def _forwards_agree(knet, x, calls=None):
    ran = 0
    for (n, more) in ((1, {}), (3, {}), (8, {}), (16, dict(narrow32=True))):
        xi = x[torch.arange(n) % x.shape[0]].contiguous()
        want = knet.forward_linear(xi, narrow=True, **more)
        if calls is not None:
            del calls[:]
        assert torch.equal(knet.forward_linear(xi, narrow=True, narrow_taps='pairs', **more), want), n
        if calls is not None:
            here = sum(1 for (p, f) in calls if NEW in p)
            assert all(bool(f & PAIRS) == bool(f & TAPS) == bool(f & TAPS32) == bool(f & NARROW) for (p, f) in calls), calls
            assert (here > 0) == (n <= 8), (n, [p for (p, f) in calls])          # at 16 images 'pairs' is 'packed'
            if n > 8:
                assert any('convtaps_narrow_taps32_kernel' in p for (p, f) in calls)
            ran += here
        assert torch.equal(knet.forward(xi, narrow=True, narrow_taps='pairs', **more), knet.forward(xi, narrow=True, **more)), n
        replay = knet.capture(xi, narrow=True, narrow_taps='pairs', **more)
        assert torch.equal(replay(xi).clone(), want), n
    return ran


@pytest.mark.parametrize('name', ['mini_tiled_permutation.npz', 'mini_tiled_identity.npz'])
def test_golden_mini_nets_eager_and_captured(golden, name, monkeypatch):
    """forward, forward_linear and capture().replay() with narrow_taps='pairs' equal the calls without the keyword (these nets' conv layers have at most 8 output
    channels: the keyword reaches them and changes nothing)."""
    z = golden(name)
    knet = _keynet(z, name, monkeypatch)
    knet.exact_mode(True)
    _forwards_agree(knet, torch.as_tensor(z['x_cipher'].astype(np.float32)).to(dev()))


def test_a_keynet_with_wide_conv_layers_runs_the_new_kernel(monkeypatch):
    (knet, x) = _wide_keynet()
    knet.exact_mode(True)
    calls = _spmm_calls(monkeypatch)
    assert _forwards_agree(knet, x, calls) >= 2 * 3                     # both conv layers (72 and 136 output channels), at 1, 3 and 8 images


def test_keyword_errors(golden):
    z = golden('mini_tiled_permutation.npz')
    knet = kio.keynet_from_arrays(z)
    x = torch.as_tensor(z['x_cipher'].astype(np.float32)).to(dev())
    for call in (knet.forward_linear, knet.forward, knet.capture):
        with pytest.raises(ValueError):
            call(x[:1], narrow_taps='pairs')                            # not without `narrow`
        with pytest.raises(ValueError):
            call(x[torch.arange(9) % x.shape[0]], narrow=True, narrow_taps='pairs')           # beyond 8 images it needs narrow32
    (W, _, X, _) = _build(COUT128)
    with pytest.raises(ValueError):
        W.torchdot(torch.as_tensor(X[:, :2]).to(dev()), exact=True, narrow_taps='pairs')
    with pytest.raises(ValueError):
        W.torchdot(torch.as_tensor(X[:, :9]).to(dev()), exact=True, narrow=True, narrow_taps='pairs')
