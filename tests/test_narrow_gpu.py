"""The low-latency forward for 1 .. 8 images on the GPU: convtaps_narrow_kernel (KN_FLAG_NARROW: lanes are output channels) against the CPU oracle and against
the kernels a 128-column batch runs, the flag's semantics through the C ABI, and KeyedModel.forward_linear / forward / capture with narrow=True.
Every check here is bit for bit unless a docstring says otherwise: the narrow kernel is the reference's own arithmetic."""
import numpy as np
import pytest
import torch

import oracle
from keynet_amd import io as kio
from keynet_amd import sparse as ksp
from keynet_amd import system as ksys
from keynet_amd import _capi
from keynet_amd.layer import KeyedLayer
from test_parity_gpu import _random_convtaps, close, dev
from fuzz_nets import random_net
from narrow_helpers import _spmm

pytestmark = pytest.mark.gpu

(RELU, EXACT, BF16X3, NARROW) = (_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_BF16X3, _capi.KN_FLAG_NARROW)
KERNEL = 'convtaps_narrow_kernel'


def _sorted_csr(W):
    M = W.tosparse('csr')
    M.sort_indices()
    return M


def _oracle(M, X):
    with np.errstate(all='ignore'):
        return oracle.csr_matvecs(M.shape, M.indptr, M.indices, M.data.astype(np.float32), X)


def _dropped_zero_operator(rng, Cin, Cout, H):
    """An untiled keyed conv as the device holds it: the factored stand-in of a CSR from which the keying product has dropped every exact zero."""
    F = _random_convtaps(rng, Cin, Cout, H, 3, 1, True, True)
    taps = F._taps['taps']
    taps[rng.rand(*taps.shape) < 0.004] = 0.0                          # (FactoredSparseMatrix refuses operators with more than 1 % zeros)
    assert np.count_nonzero(taps == 0) > 0
    M = _sorted_csr(F)
    M.eliminate_zeros()
    return (ksp.FactoredSparseMatrix(M.astype(np.float32), F), M)


# (id, Cin, Cout, H, k, stride, unit coefficients, bias column)
SHAPES = [
    ('3x3-s1-cin3-cout24-bias', 3, 24, 8, 3, 1, True, True),
    ('3x3-s2-cin5-cout64-nobias', 5, 64, 8, 3, 2, True, False),
    ('5x5-cin16-cout192-coef-bias', 16, 192, 6, 5, 1, False, True),
    ('3x3-s1-cin3-cout64-coef-nobias', 3, 64, 8, 3, 1, False, False),
    ('3x3-s1-cin16-cout24-nobias', 16, 24, 8, 3, 1, True, False),
    ('3x3-s2-cin5-cout192-coef-bias', 5, 192, 8, 3, 2, False, True),
    ('5x5-cin5-cout64-bias', 5, 64, 6, 5, 1, True, True),
    ('filled-9x9-cin3-cout64', 3, 64, 12, 9, 1, False, True),
    ('factored-dropped-zeros', 16, 24, 8, 3, 1, True, True),
]


def _build(case, seed=5):
    (tag, Cin, Cout, H, k, stride, unit, has_last) = case
    rng = np.random.RandomState(seed)
    if tag.startswith('factored'):
        (W, M) = _dropped_zero_operator(rng, Cin, Cout, H)
    else:
        W = _random_convtaps(rng, Cin, Cout, H, k, stride, unit, has_last)
        M = _sorted_csr(W)
    if tag.startswith('filled'):
        t = W._taps
        pairs = t['ent_out'].astype(np.int64) * (H * H) + t['ent_in']
        assert len(np.unique(pairs)) < len(pairs)                       # several slots on one (output, input) pixel pair
        assert np.bincount(t['ent_out']).max() > 64                     # more than 64 slots per pixel
    X = rng.randn(W.shape[1], 128).astype(np.float32)
    if has_last:
        X[-1] = 1.0
    return (W, M, X, rng)


@pytest.mark.parametrize('n_vecs', [1, 2, 3, 5, 8])
@pytest.mark.parametrize('case', SHAPES, ids=[c[0] for c in SHAPES])
def test_narrow_kernel_against_the_oracle_and_the_128_column_kernels(case, n_vecs):
    """The narrow kernel on n columns == scipy's csr_matvecs on the sorted expansion (with and without ReLU) == the first n columns of what the existing
    order-preserving kernels give at 128 columns."""
    (W, M, X, _) = _build(case)
    xd = torch.as_tensor(X).to(dev())
    with torch.cuda.device(dev()):
        plan = W._device_op(dev()).plan(n_vecs, EXACT | NARROW)
        wide = W._device_op(dev()).plan(128, EXACT | NARROW)
    assert KERNEL in plan, plan
    assert KERNEL not in wide, wide
    if case[0].startswith('filled'):
        assert 'stored values summed' in plan, plan
    ref = _oracle(M, X[:, :n_vecs])
    for relu in (False, True):
        y = W.torchdot(xd[:, :n_vecs], relu=relu, exact=True, narrow=True).cpu().numpy()
        assert np.array_equal(y, np.maximum(ref, 0) if relu else ref), (case[0], n_vecs, relu, float(np.abs(y - ref).max()))
    y = W.torchdot(xd[:, :n_vecs], exact=True, narrow=True)
    y128 = W.torchdot(xd, exact=True)
    assert torch.equal(y, y128[:, :n_vecs])


def test_flag_semantics():
    """KN_FLAG_NARROW alone, with KN_FLAG_EXACT and with KN_FLAG_BF16X3 are the same bits; at nine columns the flag is ignored; without the flag nothing moved."""
    (W, M, X, _) = _build(('semantics', 16, 64, 8, 3, 1, True, True), seed=9)
    xd = torch.as_tensor(X).to(dev())
    with torch.cuda.device(dev()):
        op = W._device_op(dev())
        t = W._taps
        op2 = _capi.Operator.convtaps(W._inshape, W._outshape, t['taps'], t['ent_out'], t['ent_in'], t['ent_tap'], t['ent_coef'], t['lastcol'])      # a second handle of the same operator
    for n in (1, 4, 8):
        (ye, _, pe) = _spmm(op, xd, n, EXACT | NARROW)
        for flags in (NARROW, NARROW | BF16X3, NARROW | BF16X3 | EXACT):
            (y, _, p) = _spmm(op, xd, n, flags)
            assert KERNEL in p and torch.equal(y, ye), (n, flags, p)
        assert np.array_equal(ye.cpu().numpy(), _oracle(M, X[:, :n]))
        (yr, _, _) = _spmm(op, xd, n, NARROW | RELU)
        assert torch.equal(yr, torch.clamp(ye, min=0))
    for flags in (0, EXACT, BF16X3):
        (y9, _, p9) = _spmm(op, xd, 9, flags | NARROW)
        (y0, _, p0) = _spmm(op, xd, 9, flags)
        assert KERNEL not in p9 and p9 == p0 and torch.equal(y9, y0), (flags, p9, p0)
    for n in (1, 8, 64):                                                # without the flag: plan and bits as on a handle that never saw it
        for flags in (0, EXACT, RELU, BF16X3):
            (ya, _, pa) = _spmm(op, xd, n, flags)
            (yb, _, pb) = _spmm(op2, xd, n, flags)
            assert KERNEL not in pa and pa == pb and torch.equal(ya, yb), (n, flags, pa, pb)
    with torch.cuda.device(dev()):
        assert 'convtaps_exact_kernel' in op.plan(64, EXACT)            # (what the existing tests pin at 64 columns)


def test_a_csr_operator_ignores_the_flag():
    rng = np.random.RandomState(2)
    import scipy.sparse
    A = scipy.sparse.random(40, 30, density=0.3, format='csr', dtype=np.float32, random_state=3)
    W = ksp.SparseMatrix(A)
    xd = torch.as_tensor(rng.randn(30, 8).astype(np.float32)).to(dev())
    with torch.cuda.device(dev()):
        op = W._device_op(dev())
    (y1, _, p1) = _spmm(op, xd, 4, EXACT | NARROW)
    (y0, _, p0) = _spmm(op, xd, 4, EXACT)
    assert p1 == p0 and torch.equal(y1, y0)


def test_column_window_of_a_wider_block_through_the_c_abi():
    """Four columns at offset 8 of a 1 024-wide block (ldx = ldy = 1024): the window equals the stand-alone result, every other element is untouched."""
    (W, M, X, rng) = _build(('window', 5, 24, 8, 3, 1, False, True), seed=13)
    (ld, c0, n) = (1024, 8, 4)
    Xb = rng.randn(W.shape[1], ld).astype(np.float32)
    Xb[-1] = 1.0
    xb = torch.as_tensor(Xb).to(dev())
    yb = torch.full((W.shape[0], ld), -3.25, dtype=torch.float32, device=dev())
    with torch.cuda.device(dev()):
        op = W._device_op(dev())
        assert KERNEL in op.plan(n, NARROW, ldx=ld, ldy=ld)
        op.spmm(xb.data_ptr() + 4 * c0, ld, n, yb.data_ptr() + 4 * c0, ld, EXACT | NARROW | RELU, torch.cuda.current_stream().cuda_stream)
    alone = W.torchdot(xb[:, c0:c0 + n], relu=True, exact=True, narrow=True)
    assert torch.equal(yb[:, c0:c0 + n], alone)
    assert np.array_equal(alone.cpu().numpy(), np.maximum(_oracle(M, Xb[:, c0:c0 + n]), 0))
    outside = torch.ones(ld, dtype=torch.bool, device=dev())
    outside[c0:c0 + n] = False
    assert bool(torch.all(yb[:, outside] == -3.25))


@pytest.mark.parametrize('case', [SHAPES[0], SHAPES[2], SHAPES[7], SHAPES[8]], ids=lambda c: c[0])
def test_non_finite_activations(case):
    """A NaN in one column and an Inf in another: what scipy's product of the reference operator gives, NaN for NaN (the dropped-zero stand-in included:
    0 * Inf must not appear where the reference has no entry)."""
    (W, M, X, rng) = _build(case, seed=21)
    n = 5
    X = X[:, :n].copy()
    rows = rng.choice(W.shape[1] - 1, size=6, replace=False)
    X[rows[:3], 1] = np.nan
    X[rows[3:], 3] = [np.inf, -np.inf, np.inf]
    ref = _oracle(M, X)
    assert np.isnan(ref).any() and np.isfinite(ref[:, 0]).all()
    for relu in (False, True):
        y = W.torchdot(torch.as_tensor(X).to(dev()), relu=relu, exact=True, narrow=True).cpu().numpy()
        r = ref.copy()
        if relu:
            r = np.where(np.isnan(r), r, np.maximum(r, 0)).astype(np.float32)
        assert np.array_equal(y, r, equal_nan=True), (case[0], relu)


def _last(z):
    return z['Y.%s' % [str(n) for n in z['layer_names']][-1]]


@pytest.mark.parametrize('name', ['mini_tiled_permutation.npz', 'mini_tiled_permutation8.npz', 'mini_tiled_identity.npz'])
def test_whole_keynets_on_permutation_keys(golden, name):
    """forward_linear(narrow=True) of 1 / 3 / 8 images == the same images inside a batch of 256, bit for bit, nothing padded; the reference's shape from
    forward(); nine images refused; host in, host out; the golden batch, eight images at a time, equals the file's reference vectors bit for bit.
    The batch of 256 runs under exact_mode(True): a key-net loaded from the reference's arrays does not know its keys are permutations and would put
    the conv layers of the wide batch on the matrix cores (another rounding); the stored order is the contract such a key-net is built with
    (TiledPermutationKeynet) and the one arithmetic a narrow forward has.  Under the loaded contract the two agree inside the gate the existing tests
    hold this file to (element-wise 2e-5 + 2e-5 |ref|), which is asserted too."""
    z = golden(name)
    knet = kio.keynet_from_arrays(z)
    rng = np.random.RandomState(0)
    big = torch.as_tensor(z['x_cipher'][rng.randint(0, z['x_cipher'].shape[0], size=256)].astype(np.float32)).to(dev())
    loose = knet.forward_linear(big)                                    # the loaded ('auto') contract: calibrates
    knet.exact_mode(True)
    full = knet.forward_linear(big)
    knet._padded_forwards = 0
    for n in (1, 3, 8):
        y = knet.forward_linear(big[:n], narrow=True)
        assert y.shape == (n, full.shape[1]) and y.is_cuda
        print(name, n, 'max |narrow - exact@256| =', float((y - full[:n]).abs().max()), ' max |narrow - default@256| =', float((y - loose[:n]).abs().max()))
        assert torch.equal(y, full[:n]), n
        assert bool(torch.all((y - loose[:n]).abs() <= 2e-5 + 2e-5 * loose[:n].abs())), n
    assert knet._padded_forwards == 0
    one = knet.forward(big[:1], narrow=True)
    assert tuple(one.shape) == tuple(knet._outshape)
    assert torch.equal(one.flatten(), ksys.ktorch.linear_to_affine(full[:1], knet._outshape).flatten())
    assert tuple(knet.forward(big[:3], narrow=True).shape) == (3,) + tuple(knet._outshape)
    with pytest.raises(ValueError):
        knet.forward_linear(big[:9], narrow=True)
    with pytest.raises(ValueError):
        knet.capture(big[:9], narrow=True)
    x = torch.as_tensor(z['x_cipher']).to(dev())
    m = min(5, int(x.shape[0]))
    yh = knet.forward_linear(torch.as_tensor(z['x_cipher'][:m]), narrow=True)
    assert not yh.is_cuda and yh.shape[0] == m
    assert torch.equal(yh, knet.forward_linear(x[:m], narrow=True).cpu())
    out = torch.cat([knet.forward_linear(x[lo:lo + 8], narrow=True) for lo in range(0, x.shape[0], 8)]).cpu().numpy()
    assert np.array_equal(out, _last(z)), float(np.abs(out - _last(z)).max())
    knet.exact_mode(None)                                               # back to the loaded contract: a narrow forward decides nothing
    y = knet.forward_linear(big[:3], narrow=True)
    assert torch.equal(y, full[:3])
    assert set(knet.contract_report()['undecided']) == set(n for (n, c) in knet._keyed(named=True) if isinstance(c.W, ksp.Conv2dTiledMatrix))
    assert knet._padded_forwards == 0


@pytest.mark.parametrize('name', ['mini_tiled_orthogonal.npz', 'mini_tiled_stochastic.npz'])
def test_whole_keynets_on_float_keys(golden, name):
    """After one ordinary forward has calibrated the net, a narrow forward changes nothing in contract_report() and its logits are inside the reference's
    element-wise gate |d| <= 1e-5 + 1e-5 |ref| against the file's reference output: the arithmetic is the reference's own, so the gate is the reference's
    criterion (the existing whole-net tests of these files allow 2e-5 for the matrix-core layers; not needed here).  The measured distance is printed."""
    z = golden(name)
    knet = kio.keynet_from_arrays(z)
    x = torch.as_tensor(z['x_cipher']).to(dev())
    knet.forward_linear(x)
    import copy
    before = copy.deepcopy(knet.contract_report())
    assert not before['undecided']
    plans = (dict(knet.__dict__.get('_overlap_plans', {})), dict(knet.__dict__.get('_chain_ops', {})))
    knet._padded_forwards = 0
    out = torch.cat([knet.forward_linear(x[lo:lo + 8], narrow=True) for lo in range(0, x.shape[0], 8)]).cpu().numpy()
    assert knet.contract_report() == before
    assert (dict(knet.__dict__.get('_overlap_plans', {})), dict(knet.__dict__.get('_chain_ops', {}))) == plans
    assert knet._padded_forwards == 0
    ref = _last(z)
    d = np.abs(out.astype(np.float64) - ref)
    print(name, 'narrow vs reference: max |d| = %.3g, worst d / (1e-5 + 1e-5 |ref|) = %.3g' % (float(d.max()), float((d / (1e-5 + 1e-5 * np.abs(ref))).max())))
    assert close(out, ref)
    # every conv layer, on the reference's own previous-layer output: the reference's bits
    prev = z['x_cipher']
    for (lname, c) in knet._keynet.named_children():
        if isinstance(c, KeyedLayer) and isinstance(c.W, ksp.Conv2dTiledMatrix):
            y = c.forward(torch.as_tensor(prev[:8]).to(dev()), narrow=True).cpu().numpy()
            assert np.array_equal(y, z['Y.%s' % lname][:8]), lname
        prev = z['Y.%s' % lname]
    assert knet.contract_report() == before


@pytest.mark.parametrize('name', ['mini_tiled_permutation.npz', 'mini_tiled_stochastic.npz', 'lenet_perm.npz'])
def test_capture_of_the_narrow_forward(golden, name):
    """capture(x[:4], narrow=True): two replays on different inputs each equal the eager narrow forward (a key-net without conv-taps layers takes the
    whole-net kernel either way)."""
    z = golden(name)
    knet = kio.keynet_from_arrays(z)
    x = torch.as_tensor(z['x_cipher']).to(dev())
    knet.forward_linear(x)
    replay = knet.capture(x[:4], narrow=True)
    other = (x[:4].flip(0) * 0.5).contiguous()                        # other data of the same shape (the homogeneous 1 scaled too: a linear map of the column)
    assert not torch.equal(other, x[:4])
    for xi in (x[:4], other):
        eager = knet.forward_linear(xi, narrow=True)
        assert torch.equal(replay(xi).clone(), eager)
    assert not torch.equal(knet.forward_linear(other, narrow=True), knet.forward_linear(x[:4], narrow=True))
    assert getattr(replay, 'graph', None) is not None


def test_fuzz_narrow_kernel_on_random_conv_operators():
    """Seeded: the conv layers of random source networks (tests/fuzz_nets.py) keyed by tiled permutations, each operator at a random width of 1 .. 8 against the oracle on
    its sorted expansion.  Every case must run on the narrow kernel; at least 40 operators."""
    rng = np.random.RandomState(20260)
    (done, nets) = (0, 0)
    while done < 40:
        nets += 1
        assert nets < 400, 'the generator stopped producing conv layers'
        torch.manual_seed(int(rng.randint(1 << 30)))
        np.random.seed(int(rng.randint(1 << 30)))
        (net, inshape, names) = random_net(rng, sides=(6, 8, 12))
        if not any(n.startswith('conv') for n in names):
            continue
        (_, knet) = ksys.TiledPermutationKeynet(inshape, net, int(rng.choice([2, 3, 4])))
        for (lname, c) in knet._keyed(named=True):
            if not isinstance(c.W, ksp.Conv2dTiledMatrix):
                continue
            W = c.W
            n = int(rng.randint(1, 9))
            relu = bool(rng.rand() < 0.5)
            with torch.cuda.device(dev()):
                plan = W._device_op(dev()).plan(n, NARROW | (RELU if relu else 0))
            assert KERNEL in plan, (nets, lname, n, plan)
            X = rng.randn(W.shape[1], n).astype(np.float32)
            X[-1] = 1.0
            M = _sorted_csr(W)
            ref = _oracle(M, X)
            y = W.torchdot(torch.as_tensor(X).to(dev()), relu=relu, exact=False, narrow=True).cpu().numpy()
            assert np.array_equal(y, np.maximum(ref, 0) if relu else ref), (nets, lname, tuple(W.shape), n, relu, float(np.abs(y - ref).max()))
            done += 1
    assert done >= 40
    # ... and random factored operators with float coefficients, two or more 64-channel blocks, strides and bias columns at random: the coefficient forms
    # and the channel-block indexing under random shapes
    extra = 0
    for _ in range(16):
        (Cin, Cout, H, k) = (int(rng.randint(1, 20)), int(rng.randint(65, 200)), int(rng.choice([4, 6, 8])), int(rng.choice([1, 3, 5])))
        (stride, unit, has_last) = (int(rng.choice([1, 2])), bool(rng.rand() < 0.3), bool(rng.rand() < 0.7))
        W = _random_convtaps(rng, Cin, Cout, H, k, stride, unit, has_last)
        n = int(rng.randint(1, 9))
        relu = bool(rng.rand() < 0.5)
        with torch.cuda.device(dev()):
            plan = W._device_op(dev()).plan(n, NARROW | (RELU if relu else 0))
        assert KERNEL in plan and (unit or ',coef' in plan), (Cin, Cout, H, k, stride, unit, plan)
        X = rng.randn(W.shape[1], n).astype(np.float32)
        if has_last:
            X[-1] = 1.0
        ref = _oracle(_sorted_csr(W), X)
        y = W.torchdot(torch.as_tensor(X).to(dev()), relu=relu, exact=False, narrow=True).cpu().numpy()
        assert np.array_equal(y, np.maximum(ref, 0) if relu else ref), (Cin, Cout, H, k, stride, unit, has_last, n, relu, float(np.abs(y - ref).max()))
        extra += 1
    assert extra == 16
