"""The packed tap-resident channel-lane kernel for 9 .. 32 batch columns (KN_MODIFIER_NARROW_TAPS32 next to KN_FLAG_NARROW_TAPS under KN_FLAG_NARROW | KN_FLAG_NARROW32;
narrow_taps='packed' next to narrow=True | 'mfma' with narrow32=True): every check is bit for bit -- against scipy's csr_matvecs on the sorted expansion (the oracle,
formed here at 32 columns), against the same call without the new bit (convtaps_narrow32_kernel) and against the first columns of the 128-column order-preserving product.

The operators are those of tests/test_narrow_taps_gpu.py (SHAPES, INELIGIBLE, _build, _coef_convtaps).  They are small, so the column-block rule of regime NARROW32
(narrower blocks while fewer than 4 096 work items and at most 2 MB of taps) runs every one of them in blocks of 8 columns; WIDE adds operators of 4 096 output pixels,
where the rule keeps the width's form -- blocks of 16 columns up to 16 columns and one block of 32 beyond."""
import numpy as np
import pytest
import torch

from keynet_amd import io as kio
from keynet_amd import sparse as ksp
from keynet_amd import _capi
from test_parity_gpu import dev
from test_narrow_gpu import _oracle
from test_narrow_taps_gpu import SHAPES, INELIGIBLE, _build, _coef_convtaps, _keynet
from narrow_helpers import _spmm, _spmm_calls, SENTINEL

pytestmark = pytest.mark.gpu

(RELU, EXACT, NARROW, MFMA, NARROW32, NARROW64, TAPS, FILL, BIT) = (_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_NARROW, _capi.KN_FLAG_NARROW_MFMA, _capi.KN_FLAG_NARROW32,
                                                                   _capi.KN_FLAG_NARROW64, _capi.KN_FLAG_NARROW_TAPS, _capi.KN_MODIFIER_NARROW_FILL, _capi.KN_MODIFIER_NARROW_TAPS32)
N32 = NARROW | NARROW32
NEW = 'convtaps_narrow_taps32_kernel'
OLD = 'convtaps_narrow32_kernel'
TAPS8 = 'convtaps_narrow_taps_kernel'
WIDTHS = [9, 12, 16, 17, 24, 31, 32]
# 64 x 64 output pixels x one channel block = 4 096 work items: the column-block rule keeps NV = 16 (9 .. 16 columns) and NV = 32 (17 .. 32)
WIDE = [
    ('3x3-s1-cin2-cout64-h64-bias', 2, 64, 64, 3, 1, True, True),
    ('3x3-s2-cin3-cout40-h128-16taps-nobias', 3, 40, 128, 3, 2, True, False),    # the 16-row forms; idle lanes; without a homogeneous row: wavefronts that fetch column by column
    ('3x3-s1-cin2-cout64-h64-coef-nobias', 2, 64, 64, 3, 1, False, False),       # coefficients at NV = 16 | 32: no such form, the call keeps convtaps_narrow32_kernel
]
_ref32 = {}


def _case(case):
    """(W, sorted CSR, X [cols, 128], oracle product at 32 columns): the operator and block of test_narrow_taps_gpu._build, the oracle formed once per case."""
    (W, M, X, _) = _build(case)
    if case not in _ref32:
        _ref32[case] = _oracle(M, X[:, :32])
    return (W, M, X, _ref32[case])


def _expected_blocks(case, W, n):
    """The column-block rule of regime NARROW32 (kn_conv.hip, narrow_choice), written out: (NV, column blocks)."""
    (tag, Cin, Cout) = case[:3]
    n_pix = (W.shape[0] - (1 if case[7] else 0)) // Cout
    items = n_pix * ((Cout + 63) // 64)
    assert 4 * 16 * (Cin + 16) * (Cout + 64) <= (2 << 20)              # (far less than 2 MB of taps, whatever the padding: the rule's second condition holds)
    nv = 16 if n <= 16 else 32
    while nv > 8 and items * ((n + nv - 1) // nv) < 4096:
        nv //= 2
    return (nv, (n + nv - 1) // nv)


def _names_the_new_kernel(case, W, n, plan):
    (nv, colb) = _expected_blocks(case, W, n)
    coef = 'coef' in case[0]
    if coef and nv != 8:                                                # a form that does not ship: the plan is the narrow32 plan
        assert NEW not in plan and OLD in plan, plan
        return False
    assert NEW in plan and OLD not in plan and plan.count(NEW) == 1, plan
    assert ('%d value rows' % (16 if 'taps' in case[0] else 9)) in plan and ('NV=%d' % nv) in plan, plan
    assert (('masked to %d' % n) in plan) == (n % nv != 0) and ('masked' in plan) == (n % nv != 0), plan
    assert ('%d column block%s' % (colb, '' if colb == 1 else 's')) in plan, plan
    assert (', coef' in plan) == coef, plan
    return True


@pytest.mark.parametrize('n_vecs', WIDTHS)
@pytest.mark.parametrize('case', SHAPES + WIDE, ids=[c[0] for c in SHAPES + WIDE])
def test_taps32_kernel_against_the_oracle_the_narrow32_kernel_and_the_128_column_product(case, n_vecs):
    (W, M, X, ref32) = _case(case)
    xd = torch.as_tensor(X).to(dev())
    with torch.cuda.device(dev()):
        op = W._device_op(dev())
        plan = op.plan(n_vecs, EXACT | N32 | TAPS | BIT)
        plain = op.plan(n_vecs, EXACT | N32)
    assert OLD in plain and NEW not in plain, plain
    new = _names_the_new_kernel(case, W, n_vecs, plan)
    assert new or plan == plain
    ref = ref32[:, :n_vecs]
    for relu in (False, True):
        y = W.torchdot(xd[:, :n_vecs], relu=relu, exact=True, narrow=True, narrow32=True, narrow_taps='packed')
        assert np.array_equal(y.cpu().numpy(), np.maximum(ref, 0) if relu else ref), (case[0], n_vecs, relu, float(np.abs(y.cpu().numpy() - ref).max()))
        assert torch.equal(y, W.torchdot(xd[:, :n_vecs], relu=relu, exact=True, narrow=True, narrow32=True))
    y = W.torchdot(xd[:, :n_vecs], exact=True, narrow=True, narrow32=True, narrow_taps='packed')
    assert torch.equal(y, W.torchdot(xd, exact=True)[:, :n_vecs])


def test_column_blocks_of_eight_and_the_widths_forms():
    """The small operators run 16 and 32 columns as two and four blocks of 8; the 4 096-pixel ones as one block of 16 and one of 32."""
    (W, _, _, _) = _case(SHAPES[0])
    (V, _, _, _) = _case(WIDE[0])
    with torch.cuda.device(dev()):
        (small, wide) = (W._device_op(dev()), V._device_op(dev()))
        for (n, colb) in ((16, 2), (32, 4), (9, 2), (24, 3)):
            plan = small.plan(n, N32 | TAPS | BIT)
            assert NEW in plan and 'NV=8' in plan and ('%d column blocks' % colb) in plan, plan
        assert 'NV=16, 1 column block>' in wide.plan(16, N32 | TAPS | BIT)
        assert 'NV=32, 1 column block>' in wide.plan(32, N32 | TAPS | BIT)
        assert 'NV=16, masked to 9, 1 column block>' in wide.plan(9, N32 | TAPS | BIT)
        assert 'NV=32, masked to 17, 1 column block>' in wide.plan(17, N32 | TAPS | BIT)


@pytest.mark.parametrize('case', [SHAPES[0], SHAPES[1], SHAPES[5], WIDE[1]], ids=lambda c: c[0])
def test_non_finite_activations(case):
    """One NaN and one Inf activation: the int32 views of the result equal the narrow32 kernel's, and the oracle's NaN pattern -- a slot the lists do not hold
    contributes nothing, so the non-finite values reach only the outputs that hold them."""
    (W, M, X, _) = _case(case)
    rng = np.random.RandomState(23)
    for n in (16, 31):
        Xn = X[:, :n].copy()
        rows = rng.choice(W.shape[1] - 1, size=2, replace=False)
        Xn[rows[0], 0] = np.nan
        Xn[rows[1], n - 1] = np.inf
        xd = torch.as_tensor(Xn).to(dev())
        ref = _oracle(M, Xn)
        for relu in (False, True):
            y = W.torchdot(xd, relu=relu, exact=True, narrow=True, narrow32=True, narrow_taps='packed')
            y0 = W.torchdot(xd, relu=relu, exact=True, narrow=True, narrow32=True)
            assert torch.equal(y.view(torch.int32), y0.view(torch.int32)), (case[0], n, relu)
            assert np.array_equal(np.isnan(y.cpu().numpy()), np.isnan(ref)), (case[0], n, relu)


@pytest.mark.parametrize('case', [SHAPES[0], SHAPES[3], WIDE[1]], ids=lambda c: c[0])
@pytest.mark.parametrize('n', [9, 17, 24, 32])
def test_no_stray_writes_on_a_column_window_of_a_wider_block(case, n):
    """n columns from column 3 of a 128-wide block (ldx = ldy = 128): the narrow32 kernel's window, the oracle, and the sentinel everywhere else."""
    (W, M, X, _) = _case(case)
    xd = torch.as_tensor(X).to(dev())
    with torch.cuda.device(dev()):
        op = W._device_op(dev())
    for relu in (0, RELU):
        (win, whole, plan) = _spmm(op, xd, n, EXACT | N32 | TAPS | BIT | relu, ld=128, start=3)
        assert NEW in plan and OLD not in plan, plan
        assert torch.equal(win, _spmm(op, xd, n, EXACT | N32 | relu, ld=128, start=3)[0])
        ref = _oracle(M, X[:, 3:3 + n])
        assert np.array_equal(win.cpu().numpy(), np.maximum(ref, 0) if relu else ref)
        outside = torch.ones(128, dtype=torch.bool, device=dev())
        outside[3:3 + n] = False
        assert whole.shape[0] == W.shape[0] and bool(torch.all(whole[:, outside] == SENTINEL))


def test_flag_semantics():
    """A modifier of KN_FLAG_NARROW_TAPS in regime NARROW32 and of nothing else."""
    (W, M, X, _) = _build(('semantics', 16, 64, 8, 3, 1, True, True), seed=9)
    xd = torch.as_tensor(X).to(dev())
    with torch.cuda.device(dev()):
        op = W._device_op(dev())

    def same(n, flags, other):
        (y1, _, p1) = _spmm(op, xd, n, flags)
        (y0, _, p0) = _spmm(op, xd, n, other)
        assert p1 == p0 and NEW not in p1 and torch.equal(y1, y0), (n, flags, p1, p0)
        return p1
    for n in (9, 16, 32):
        for flags in (N32, N32 | EXACT, N32 | RELU):                    # without KN_FLAG_NARROW_TAPS the bit is not read
            assert OLD in same(n, flags | BIT, flags)
        assert OLD in same(n, N32 | TAPS, N32)                          # ... and KN_FLAG_NARROW_TAPS alone stays a no-op at 9+ columns
        for flags in (0, EXACT, RELU):                                  # the two bits without the regime
            same(n, flags | TAPS | BIT, flags)
        (y, _, p) = _spmm(op, xd, n, N32 | TAPS | BIT)                  # both bits: the kernel
        assert NEW in p and torch.equal(y, _spmm(op, xd, n, N32)[0]), p
    for n in (1, 4, 8):                                                 # 8 columns and fewer: the plan of KN_FLAG_NARROW_TAPS
        for flags in (NARROW, N32, N32 | EXACT):
            assert TAPS8 in same(n, flags | TAPS | BIT, flags | TAPS)
    for n in (33, 64):                                                  # beyond 32 columns
        same(n, N32 | NARROW64 | TAPS | BIT, N32 | NARROW64)
        same(n, N32 | NARROW64 | EXACT | TAPS | BIT, N32 | NARROW64 | EXACT)
    for n in (9, 16, 32):                                               # the matrix-core regime keeps its kernel; with KN_FLAG_EXACT the flag means KN_FLAG_NARROW
        assert 'convtaps_narrow_mfma_kernel' in same(n, MFMA | NARROW32 | TAPS | BIT, MFMA | NARROW32)
        (ye, _, pe) = _spmm(op, xd, n, MFMA | NARROW32 | EXACT | TAPS | BIT)
        assert NEW in pe and torch.equal(ye, _spmm(op, xd, n, N32 | EXACT)[0]), pe
    import scipy.sparse
    A = scipy.sparse.random(40, 30, density=0.3, format='csr', dtype=np.float32, random_state=3)       # a CSR handle
    S = ksp.SparseMatrix(A)
    xs = torch.as_tensor(np.random.RandomState(2).randn(30, 32).astype(np.float32)).to(dev())
    with torch.cuda.device(dev()):
        cs = S._device_op(dev())
    for flags in (EXACT, EXACT | N32):
        (y1, _, p1) = _spmm(cs, xs, 16, flags | TAPS | BIT)
        (y0, _, p0) = _spmm(cs, xs, 16, flags)
        assert p1 == p0 and torch.equal(y1, y0)


@pytest.mark.parametrize('case', INELIGIBLE, ids=[c[0] for c in INELIGIBLE])
def test_ineligible_operators_keep_plan_and_bits(case):
    (W, M, X, _) = _build(case)
    xd = torch.as_tensor(X).to(dev())
    with torch.cuda.device(dev()):
        op = W._device_op(dev())
    for n in (9, 16, 32):
        for flags in (N32, EXACT | N32 | RELU):
            (y1, _, p1) = _spmm(op, xd, n, flags | TAPS | BIT)
            (y0, _, p0) = _spmm(op, xd, n, flags)
            assert p1 == p0 and OLD in p1 and NEW not in p1, (n, p1, p0)
            assert torch.equal(y1, y0)
            (yf, _, pf) = _spmm(op, xd, n, flags | FILL | TAPS | BIT)     # where KN_FLAG_NARROW_FILL takes the launch (or does not), the bit changes nothing
            (yg, _, pg) = _spmm(op, xd, n, flags | FILL)
            assert pf == pg and NEW not in pf and torch.equal(yf, yg)


MODELS = ['mini_tiled_permutation.npz', 'mini_tiled_permutation8.npz', 'mini_tiled_identity.npz', 'allconv_tiny_perm.npz']


@pytest.mark.parametrize('name', MODELS)
def test_whole_keynets(golden, name, monkeypatch):
    """forward_linear(narrow=True, narrow32=True, narrow_taps='packed') at 9, 16 and 32 images == the call without the keyword == the padded forward == a capture's
    replay; the recorded kn_spmm calls carry both bits on the conv layers, which run the new kernel, and on nothing else."""
    z = golden(name)
    knet = _keynet(z, name, monkeypatch)
    x = torch.as_tensor(z['x_cipher'].astype(np.float32)).to(dev())
    knet.exact_mode(True)
    for n in (9, 16, 32):
        xi = x[torch.arange(n) % x.shape[0]].contiguous()
        xi = (xi * (1.0 + 0.01 * torch.arange(n, device=xi.device, dtype=xi.dtype)).reshape([n] + [1] * (xi.dim() - 1))).contiguous()      # (no two images alike)
        y = knet.forward_linear(xi, narrow=True, narrow32=True, narrow_taps='packed')
        assert torch.equal(y, knet.forward_linear(xi, narrow=True, narrow32=True)), (name, n)
        assert torch.equal(y, knet.forward_linear(xi)), (name, n)
        replay = knet.capture(xi, narrow=True, narrow32=True, narrow_taps='packed')
        assert torch.equal(replay(xi).clone(), y), (name, n)
        other = (xi.flip(0) * 0.5).contiguous()
        assert torch.equal(replay(other).clone(), knet.forward_linear(other, narrow=True, narrow32=True)), (name, n)
    convs = sum(1 for c in knet._keyed() if c.W.narrow_capable())
    x16 = x[torch.arange(16) % x.shape[0]].contiguous()
    calls = _spmm_calls(monkeypatch)
    knet.forward_linear(x16, narrow=True, narrow32=True, narrow_taps='packed')
    flagged = [(p, f) for (p, f) in calls if f & BIT]
    assert len(flagged) == convs > 0, (name, len(flagged), convs)
    for (p, f) in calls:
        assert bool(f & BIT) == bool(f & TAPS) == bool(f & NARROW), (p, f)
        assert (NEW in p) == bool(f & BIT) and OLD not in p, (p, f)
    del calls[:]
    knet.forward_linear(x16, narrow=True, narrow32=True, narrow_taps=True)       # narrow_taps=True: the first bit only, a no-op at 16 images
    assert calls and not any(f & BIT for (p, f) in calls) and not any(NEW in p for (p, f) in calls)
    assert sum(1 for (p, f) in calls if f & TAPS and OLD in p) == convs
    del calls[:]
    x4 = x[torch.arange(4) % x.shape[0]].contiguous()
    y4 = knet.forward_linear(x4, narrow=True, narrow32=True, narrow_taps='packed')       # 8 images and fewer: exactly narrow_taps=True
    packed = list(calls)
    del calls[:]
    assert torch.equal(y4, knet.forward_linear(x4, narrow=True, narrow32=True, narrow_taps=True))
    assert [p for (p, f) in packed] == [p for (p, f) in calls] and any(TAPS8 in p for (p, f) in calls)


def test_narrow_mfma_next_to_packed(golden, monkeypatch):
    """Inside a narrow='mfma' forward the layers on the matrix-core kernel keep plan and bits; the layers under exact=True take the new kernel."""
    z = golden('mini_tiled_permutation.npz')
    knet = kio.keynet_from_arrays(z)
    x = torch.as_tensor(z['x_cipher'].astype(np.float32)).to(dev())
    x16 = x[torch.arange(16) % x.shape[0]].contiguous()
    knet.exact_mode(False)
    calls = _spmm_calls(monkeypatch)
    y0 = knet.forward_linear(x16, narrow='mfma', narrow32=True)
    plain = list(calls)
    del calls[:]
    y1 = knet.forward_linear(x16, narrow='mfma', narrow32=True, narrow_taps='packed')
    assert torch.equal(y1, y0)
    assert [p for (p, f) in plain] == [p for (p, f) in calls] and any(f & MFMA for (p, f) in calls)
    assert not any(f & (BIT | TAPS) for (p, f) in calls if f & MFMA) and not any(NEW in p for (p, f) in calls if f & MFMA)
    knet.exact_mode(True)
    want = knet.forward_linear(x16, narrow=True, narrow32=True)
    del calls[:]
    assert torch.equal(knet.forward_linear(x16, narrow='mfma', narrow32=True, narrow_taps='packed'), want)
    assert any(f & BIT and NEW in p for (p, f) in calls) and not any(f & MFMA for (p, f) in calls)


def test_the_keyword_needs_narrow_and_narrow32(golden):
    z = golden('mini_tiled_permutation.npz')
    knet = kio.keynet_from_arrays(z)
    x = torch.as_tensor(z['x_cipher'].astype(np.float32)).to(dev())
    x9 = x[torch.arange(9) % x.shape[0]].contiguous()
    for call in (knet.forward_linear, knet.forward, knet.capture):
        with pytest.raises(ValueError):
            call(x9, narrow32=True, narrow_taps='packed')
        with pytest.raises(ValueError):
            call(x9, narrow=True, narrow_taps='packed')                 # nine images: narrow32
    (W, _, X, _) = _build(SHAPES[0])
    with pytest.raises(ValueError):
        W.torchdot(torch.as_tensor(X[:, :16]).to(dev()), exact=True, narrow_taps='packed')
    x40 = x[torch.arange(40) % x.shape[0]].contiguous()                 # beyond 32 images it changes nothing
    knet.exact_mode(True)
    assert torch.equal(knet.forward_linear(x40, narrow=True, narrow64=True, narrow_taps='packed'), knet.forward_linear(x40, narrow=True, narrow64=True))
