"""The tap-resident channel-lane kernel of FILLED-IN conv-taps operators for 1 .. 32 batch columns (KN_FLAG_NARROW_FILL next to KN_FLAG_NARROW [| KN_FLAG_NARROW32];
narrow_fill=True next to narrow=True | 'mfma'): every check is bit for bit -- against scipy's csr_matvecs on the sorted expansion (the oracle), against the same call
without the flag / keyword (convtaps_narrow_kernel<stored values summed>, convtaps_narrow32_kernel), and against the first columns of the 128-column order-preserving
product (convtaps_exact_fill_kernel).

Eligible operators: test_parity_gpu._filled_in_convtaps (every entry its own coefficient, several slots on one pixel pair, 18 .. 54 slots per pixel) and
_random_convtaps' own coefficient operators (two slots on a pair, lists shorter than one record batch).  Ineligible: more than 16 taps, no record lists, the
taps-eligible 3 x 3 unit operator, a CSR handle."""
import collections

import numpy as np
import pytest
import torch

import value_classes
from keynet_amd import io as kio
from keynet_amd import sparse as ksp
from keynet_amd import _capi
from keynet_amd.layer import KeyedLayer
from keynet_amd.system import KeyedModel
from test_parity_gpu import _filled_in_convtaps, _random_convtaps, dev
from test_narrow_gpu import _sorted_csr, _oracle
from narrow_helpers import _spmm, _spmm_calls, SENTINEL

pytestmark = pytest.mark.gpu

(RELU, EXACT, BF16X3, NARROW, MFMA, NARROW32, NARROW64, TAPS, FILL) = (_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_BF16X3, _capi.KN_FLAG_NARROW, _capi.KN_FLAG_NARROW_MFMA,
                                                                       _capi.KN_FLAG_NARROW32, _capi.KN_FLAG_NARROW64, _capi.KN_FLAG_NARROW_TAPS, _capi.KN_MODIFIER_NARROW_FILL)
NEW = 'convtaps_narrow_fill_kernel'
OLD = 'convtaps_narrow_kernel'
OLD32 = 'convtaps_narrow32_kernel'

# (id, generator, its arguments)
ELIGIBLE = [
    ('fill3-cin3-cout40-h8-bias', 'filled', (3, 40, 8, 3, True)),              # masked lanes; 27 slots per pixel: no multiple of 8
    ('fill5-cin16-cout64-h6-bias', 'filled', (16, 64, 6, 5, True)),
    ('fill6-cin5-cout136-h4-nobias', 'filled', (5, 136, 4, 6, False)),         # three channel blocks, the last masked; 54 slots on 16 input pixels: values of three and more terms
    ('fill3-cin1-cout64-h4-bias', 'filled', (1, 64, 4, 3, True)),              # Cin = 1: no next channel to prefetch
    ('3x3-s2-cin5-cout64-coef-dups', 'random', (5, 64, 8, 3, 2, False, False)),     # strided, two slots on a pair, lists shorter than one record batch
    ('3x3-s1-cin16-cout192-coef-dups', 'random', (16, 192, 8, 3, 1, False, True)),
    ('4x4-s1-cin3-cout64-coef-dups-16taps', 'random', (3, 64, 8, 4, 1, False, True)),  # 16 taps: the upper bound of the value-row registers
]
INELIGIBLE = [
    ('filled-9x9-cin3-cout64', 'random', (3, 64, 12, 9, 1, False, True)),      # 81 taps
    ('7x7-cin3-cout64', 'random', (3, 64, 8, 7, 1, True, True)),               # no record lists
    ('3x3-cin16-cout64-unit', 'random', (16, 64, 8, 3, 1, True, True)),        # taps-eligible, not fill-eligible
]
_built = {}


def _build(case, seed=7, values=None):
    """(W, sorted CSR, X [cols, 128], oracle product at 32 columns): built once per case and shared, never modified.  `values`: a variant of
    value_classes.conv_values (tests/test_value_classes_gpu.py): the same operator with its values scaled by powers of two."""
    if (case[0], values) not in _built:
        (tag, gen, args) = case
        rng = np.random.RandomState(seed)
        W = _filled_in_convtaps(rng, *args) if gen == 'filled' else _random_convtaps(rng, *args)
        if values is not None:
            W = value_classes.revalued_convtaps(W, values)[0]
        M = _sorted_csr(W)
        X = rng.randn(W.shape[1], 128).astype(np.float32)
        if args[-1]:
            X[-1] = 1.0
        _built[(case[0], values)] = (W, M, X, _oracle(M, X[:, :32]))
    return _built[(case[0], values)]


def _op(W):
    with torch.cuda.device(dev()):
        return W._device_op(dev())


@pytest.mark.parametrize('case', ELIGIBLE, ids=[c[0] for c in ELIGIBLE])
def test_one_to_eight_columns(case):
    (W, M, X, ref32) = _build(case)
    xd = torch.as_tensor(X).to(dev())
    op = _op(W)
    wide = W.torchdot(xd, exact=True)
    for n in (1, 2, 3, 5, 8):
        plan = op.plan(n, EXACT | NARROW | FILL)
        plain = op.plan(n, EXACT | NARROW)
        assert OLD in plain and 'stored values summed' in plain and NEW not in plain, plain
        assert NEW in plan and OLD not in plan and plan.count(NEW) == 1, plan
        assert ('NV=%d' % (1 if n == 1 else 2 if n == 2 else 4 if n <= 4 else 8)) in plan and '1 column block' in plan, plan
        assert ('masked to %d' % n in plan) == (n in (3, 5)) and ', coef' in plan, plan
        ref = ref32[:, :n]
        for relu in (False, True):
            y = W.torchdot(xd[:, :n], relu=relu, exact=True, narrow=True, narrow_fill=True)
            assert np.array_equal(y.cpu().numpy(), np.maximum(ref, 0) if relu else ref), (case[0], n, relu, float(np.abs(y.cpu().numpy() - ref).max()))
            assert torch.equal(y, W.torchdot(xd[:, :n], relu=relu, exact=True, narrow=True))
        assert torch.equal(W.torchdot(xd[:, :n], exact=True, narrow=True, narrow_fill=True), wide[:, :n])


@pytest.mark.parametrize('case', ELIGIBLE, ids=[c[0] for c in ELIGIBLE])
def test_nine_to_thirty_two_columns(case):
    (W, M, X, ref32) = _build(case)
    xd = torch.as_tensor(X).to(dev())
    op = _op(W)
    wide = W.torchdot(xd, exact=True)
    for (n, blocks) in ((9, 2), (16, 2), (17, 3), (32, 4)):
        plan = op.plan(n, EXACT | NARROW | NARROW32 | FILL)
        plain = op.plan(n, EXACT | NARROW | NARROW32)
        assert OLD32 in plain and NEW not in plain, plain
        assert NEW in plan and OLD32 not in plan and 'NV=8' in plan and ('%d column blocks' % blocks) in plan, plan
        assert ('masked to %d' % n in plan) == (n % 8 != 0), plan
        ref = ref32[:, :n]
        for relu in (False, True):
            y = W.torchdot(xd[:, :n], relu=relu, exact=True, narrow=True, narrow32=True, narrow_fill=True)
            assert np.array_equal(y.cpu().numpy(), np.maximum(ref, 0) if relu else ref), (case[0], n, relu)
            assert torch.equal(y, W.torchdot(xd[:, :n], relu=relu, exact=True, narrow=True, narrow32=True))
        assert torch.equal(W.torchdot(xd[:, :n], exact=True, narrow=True, narrow32=True, narrow_fill=True), wide[:, :n])


@pytest.mark.parametrize('case', INELIGIBLE, ids=[c[0] for c in INELIGIBLE])
def test_ineligible_operators_keep_plan_and_bits(case):
    (W, M, X, ref32) = _build(case)
    xd = torch.as_tensor(X).to(dev())
    op = _op(W)
    for n in (1, 3, 8, 12):
        for flags in (NARROW | NARROW32, EXACT | NARROW | NARROW32 | RELU):
            (y1, _, p1) = _spmm(op, xd, n, flags | FILL)
            (y0, _, p0) = _spmm(op, xd, n, flags)
            assert p1 == p0 and NEW not in p1, (n, p1, p0)
            assert torch.equal(y1, y0)
        assert np.array_equal(_spmm(op, xd, n, NARROW | NARROW32 | FILL)[0].cpu().numpy(), ref32[:, :n])


def test_a_csr_handle_keeps_plan_and_bits():
    import scipy.sparse
    A = scipy.sparse.random(40, 30, density=0.3, format='csr', dtype=np.float32, random_state=3)
    cs = _op(ksp.SparseMatrix(A))
    xs = torch.as_tensor(np.random.RandomState(2).randn(30, 8).astype(np.float32)).to(dev())
    for flags in (EXACT, EXACT | NARROW):
        (y1, _, p1) = _spmm(cs, xs, 4, flags | FILL)
        (y0, _, p0) = _spmm(cs, xs, 4, flags)
        assert p1 == p0 and torch.equal(y1, y0)


def test_flag_semantics():
    """A modifier of regimes NARROW and NARROW32 and of nothing else."""
    (W, M, X, ref32) = _build(ELIGIBLE[1])
    xd = torch.as_tensor(X).to(dev())
    op = _op(W)
    for n in (1, 4, 8, 20, 64):
        for flags in (0, EXACT, RELU, BF16X3, EXACT | RELU):            # alone, and with the contract flags only
            (y1, _, p1) = _spmm(op, xd, n, flags | FILL)
            (y0, _, p0) = _spmm(op, xd, n, flags)
            assert p1 == p0 and NEW not in p1 and torch.equal(y1, y0), (n, flags, p1, p0)
    for n in (33, 64):                                                  # the KN_FLAG_NARROW64 range
        (y1, _, p1) = _spmm(op, xd, n, NARROW | NARROW32 | NARROW64 | FILL)
        (y0, _, p0) = _spmm(op, xd, n, NARROW | NARROW32 | NARROW64)
        assert p1 == p0 and NEW not in p1 and torch.equal(y1, y0), (n, p1, p0)
    for n in (1, 5, 8):                                                 # a filled-in operator has no matrix-core narrow form: KN_FLAG_NARROW_MFMA means KN_FLAG_NARROW
        (y1, _, p1) = _spmm(op, xd, n, MFMA | FILL)
        assert NEW in p1 and np.array_equal(y1.cpu().numpy(), ref32[:, :n]), p1
        (y2, _, p2) = _spmm(op, xd, n, NARROW | TAPS | FILL)            # both modifiers: the one the operator is eligible for
        assert NEW in p2 and 'convtaps_narrow_taps_kernel' not in p2 and torch.equal(y2, y1), p2
    (Wt, Mt, Xt, reft) = _build(INELIGIBLE[2])                          # ... and on a taps-eligible operator the other one
    (yt, _, pt) = _spmm(_op(Wt), torch.as_tensor(Xt).to(dev()), 5, NARROW | TAPS | FILL)
    assert 'convtaps_narrow_taps_kernel' in pt and NEW not in pt and np.array_equal(yt.cpu().numpy(), reft[:, :5]), pt


@pytest.mark.parametrize('case', [ELIGIBLE[0], ELIGIBLE[2]], ids=lambda c: c[0])
@pytest.mark.parametrize('n', [1, 3, 8])
def test_column_window_of_a_wider_block_through_the_c_abi(case, n):
    """n columns from column 3 of a 128-wide block (ldx = ldy = 128): the narrow kernel's window, the oracle, and the sentinel everywhere else."""
    (W, M, X, _) = _build(case)
    xd = torch.as_tensor(X).to(dev())
    op = _op(W)
    for relu in (0, RELU):
        (win, whole, plan) = _spmm(op, xd, n, EXACT | NARROW | FILL | relu, ld=128, start=3)
        assert NEW in plan and OLD not in plan, plan
        assert torch.equal(win, _spmm(op, xd, n, EXACT | NARROW | relu, ld=128, start=3)[0])
        ref = _oracle(M, X[:, 3:3 + n])
        assert np.array_equal(win.cpu().numpy(), np.maximum(ref, 0) if relu else ref)
        outside = torch.ones(128, dtype=torch.bool, device=dev())
        outside[3:3 + n] = False
        assert bool(torch.all(whole[:, outside] == SENTINEL))


@pytest.mark.parametrize('case', [ELIGIBLE[0], ELIGIBLE[2], ELIGIBLE[4]], ids=lambda c: c[0])
def test_non_finite_activations(case):
    """One NaN and one Inf activation: the int32 views of the result equal the narrow kernel's, and the oracle's NaN pattern -- the padding records of a list
    request no activation and commit nothing, so the non-finite values reach only the outputs that hold them."""
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
            y = W.torchdot(xd, relu=relu, exact=True, narrow=True, narrow_fill=True)
            y0 = W.torchdot(xd, relu=relu, exact=True, narrow=True)
            assert torch.equal(y.view(torch.int32), y0.view(torch.int32)), (case[0], n, relu)
            assert np.array_equal(np.isnan(y.cpu().numpy()), np.isnan(ref)), (case[0], n, relu)


def test_released_records_are_built_again():
    (W, M, X, ref32) = _build(ELIGIBLE[3])
    xd = torch.as_tensor(X).to(dev())
    op = _op(W)
    (y0, _, p0) = _spmm(op, xd, 5, NARROW | FILL)
    op.release_side_tables()
    (y1, _, p1) = _spmm(op, xd, 5, NARROW | FILL)
    assert NEW in p0 and p1 == p0 and torch.equal(y1, y0) and np.array_equal(y1.cpu().numpy(), ref32[:, :5])
    op.release_side_tables()
    (y2, _, p2) = _spmm(op, xd, 12, NARROW | NARROW32 | FILL | RELU)
    assert NEW in p2 and np.array_equal(y2.cpu().numpy(), np.maximum(ref32[:, :12], 0))


def test_the_stochastic_keynet(golden, monkeypatch):
    """forward_linear(narrow=True, narrow_fill=True) == forward_linear(narrow=True) at 1, 3, 8 images and with narrow32 at 12; the bit rides exactly on the calls that
    carry KN_FLAG_NARROW; a layer whose 128-column KN_FLAG_EXACT plan names convtaps_exact_fill_kernel<taps in registers ...> names the new kernel, every other layer what it named before.
    (Whether this file's conv layers have record lists is decided by that plan at run time: where neither has, the operator cases above carry the kernel.)"""
    z = golden('mini_tiled_stochastic.npz')
    knet = kio.keynet_from_arrays(z)
    x = torch.as_tensor(z['x_cipher'].astype(np.float32)).to(dev())
    knet.forward_linear(x)                                              # (calibrates)
    for (n, kw) in ((1, {}), (3, {}), (8, {}), (12, dict(narrow32=True))):
        xi = x[torch.arange(n) % x.shape[0]].contiguous()
        assert torch.equal(knet.forward_linear(xi, narrow=True, narrow_fill=True, **kw), knet.forward_linear(xi, narrow=True, **kw)), n
    calls = _spmm_calls(monkeypatch)
    knet.forward_linear(x[:1], narrow=True)
    before = list(calls)
    del calls[:]
    knet.forward_linear(x[:1], narrow=True, narrow_fill=True)
    assert len(calls) == len(before) > 0 and not any(f & FILL for (p, f) in before)
    convs = [c for c in knet._keyed() if c.W.narrow_capable()]
    # the record lists hold tap INDICES, and the value rows fit the registers, where the operator has at most 16 taps: the form of the wide kernel whose plan says
    # `taps in registers` (a tiled layer of this file may hold more taps than a 3 x 3 window: then it keeps the channel-lane kernel, like the wide kernel its value-row loads)
    wide = [_op(c.W).plan(128, EXACT) for c in convs]
    filled = sum(1 for p in wide if 'convtaps_exact_fill_kernel<taps in registers' in p)
    for ((p, f), (p0, f0)) in zip(calls, before):
        assert bool(f & FILL) == bool(f & NARROW) and f == f0 | (FILL if f0 & NARROW else 0), (p, f, f0)
        assert p == p0 or (NEW in p and OLD in p0 and 'stored values summed' in p0), (p, p0)
    assert sum(1 for (p, f) in calls if NEW in p) == filled, (wide, [p[:60] for (p, f) in calls])


def _two_layer_net(exact1, exact2):
    rng = np.random.RandomState(11)
    W1 = _filled_in_convtaps(rng, 3, 8, 4, 3, True)
    W2 = _filled_in_convtaps(rng, 8, 40, 4, 4, True)
    L1 = KeyedLayer.fromoperator(W1, 'Conv2d', inshape=W1._inshape, outshape=W1._outshape, exact=exact1)
    L2 = KeyedLayer.fromoperator(W2, 'Conv2d', inshape=W2._inshape, outshape=W2._outshape, exact=exact2)
    knet = KeyedModel.fromlayers(collections.OrderedDict([('conv1', L1), ('conv2', L2)]), W2._outshape)
    x = torch.as_tensor(np.concatenate((rng.randn(12, W1.shape[1] - 1), np.ones((12, 1))), axis=1).astype(np.float32)).to(dev())
    return (knet, x)


def test_a_two_layer_net_of_filled_in_operators(monkeypatch):
    (knet, x) = _two_layer_net(True, True)
    for (n, kw) in ((1, {}), (5, {}), (8, {}), (12, dict(narrow32=True))):
        want = knet.forward_linear(x[:n].contiguous(), narrow=True, **kw)
        assert torch.equal(knet.forward_linear(x[:n].contiguous(), narrow=True, narrow_fill=True, **kw), want), n
        assert torch.equal(want, knet.forward_linear(x[:n].contiguous()))           # (and the padded 128-column forward under the same contract)
    calls = _spmm_calls(monkeypatch)
    knet.forward_linear(x[:3].contiguous(), narrow='mfma', narrow_fill=True)
    assert len(calls) == 2 and all(f & FILL and f & NARROW and NEW in p for (p, f) in calls), calls
    x4 = x[:4].contiguous()
    replay = knet.capture(x4, narrow=True, narrow_fill=True)
    other = (x4.flip(0) * 0.5).contiguous()
    other[:, -1] = 1.0
    for xi in (x4, other):
        eager = knet.forward_linear(xi, narrow=True, narrow_fill=True)
        assert torch.equal(replay(xi).clone(), eager)
        assert torch.equal(eager, knet.forward_linear(xi, narrow=True))
    for call in (knet.forward_linear, knet.forward, knet.capture):
        with pytest.raises(ValueError, match='narrow_fill=True'):
            call(x4, narrow_fill=True)
        with pytest.raises(ValueError, match='narrow_fill=True'):
            call(x4, narrow_rows=True, narrow_fill=True)


def test_the_split_route_keeps_its_layer_and_the_other_runs_the_new_kernel(monkeypatch):
    """narrow='mfma', narrow_split=True, narrow_fill=True: a layer declared 'split' runs the route (no launch of it carries the bit), a layer under True the new kernel."""
    (knet, x) = _two_layer_net('split', True)
    x8 = x[:8].contiguous()
    want = knet.forward_linear(x8, narrow='mfma', narrow_split=True)
    calls = _spmm_calls(monkeypatch)
    assert torch.equal(knet.forward_linear(x8, narrow='mfma', narrow_split=True, narrow_fill=True), want)
    new = [(p, f) for (p, f) in calls if NEW in p]
    assert len(new) == 1 and new[0][1] & FILL and new[0][1] & NARROW, calls
    assert len(calls) >= 2 and all(bool(f & FILL) == bool(f & NARROW) for (p, f) in calls), calls       # the route's launches: neither bit


def test_fuzz_random_filled_in_operators_against_the_oracle():
    """Seeded: 24 random filled-in 3 x 3 operators (Cin 1 .. 12, Cout 1 .. 150, H 3 .. 6, fill 2 .. 6, bias or not, ReLU or not) at a random width 1 .. 32."""
    rng = np.random.RandomState(1616)
    for it in range(24):
        (Cin, Cout, H, fill) = (int(rng.randint(1, 13)), int(rng.randint(1, 151)), int(rng.randint(3, 7)), int(rng.randint(2, 7)))
        (has_last, relu, n) = (bool(rng.rand() < 0.6), bool(rng.rand() < 0.5), int(rng.randint(1, 33)))
        W = _filled_in_convtaps(rng, Cin, Cout, H, fill, has_last)
        flags = NARROW | NARROW32 | FILL | (RELU if relu else 0)
        op = _op(W)
        X = rng.randn(W.shape[1], n).astype(np.float32)
        if has_last:
            X[-1] = 1.0
        ref = _oracle(_sorted_csr(W), X)
        (y, _, plan) = _spmm(op, torch.as_tensor(X).to(dev()), n, flags)
        if 'convtaps_exact_fill_kernel' in op.plan(128, EXACT):       # (an operator whose 18 .. 54 slots happen to fall on distinct input pixels has no record lists)
            assert NEW in plan, (it, Cin, Cout, H, fill, n, plan)
        assert np.array_equal(y.cpu().numpy(), np.maximum(ref, 0) if relu else ref), (it, Cin, Cout, H, fill, has_last, n, relu, plan)
