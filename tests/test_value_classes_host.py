"""The host side of the value-class tests (tests/value_classes.py; the device side is tests/test_value_classes_gpu.py): the comparison sees what np.array_equal does
not, the reference is right and keeps its subnormals at every regime's magnitudes (the C oracle against scipy's own product, float32 and float64 operators), every
regime reaches its output class on rows as short and as long as the GPU module's operators have, and the reference never produces -0.0."""
import numpy as np
import pytest
import scipy.sparse
import torch  # noqa: F401  (on purpose before the checks: nothing it loads may switch the process to flush-to-zero)

import oracle
import value_classes as vc

# stored entries per row of the operators tests/test_value_classes_gpu.py runs: loose rows (6 .. 12), nine taps x 1 .. 32 channels, 70 slots x 32 channels, long rows, a keyed Linear
ROW_LENGTHS = (6, 9, 27, 70, 145, 640, 1060, 2305, 2501)


def _random_csr(k, rng, m=300, f64=False, ragged=False):
    n = max(2 * k, 64)
    ip = np.sort(np.concatenate(([0, m * k], rng.randint(0, m * k, m - 1)))).astype(np.int32) if ragged else (np.arange(m + 1) * k).astype(np.int32)
    ix = rng.randint(0, n, m * k).astype(np.int32)                      # unsorted, with duplicates
    dt = rng.randn(m * k)
    return ((m, n), ip, ix, dt if f64 else dt.astype(np.float32))


def test_bits_equal_sees_what_array_equal_does_not():
    a = np.array([[0.0, 1.0, 2.0 ** -140, np.inf, np.nan]], dtype=np.float32)
    assert vc.bits_equal(a, a.copy())
    for (k, v) in ((0, -0.0), (2, 0.0), (3, -np.inf), (1, np.nextafter(np.float32(1), np.float32(2)))):
        b = a.copy()
        b[0, k] = v
        assert not vc.bits_equal(b, a) and not vc.bits_equal(a, b), (k, v)
    assert np.array_equal(np.array([-0.0], np.float32), np.array([0.0], np.float32))          # (what the suite compared with so far)
    # two NaNs of different payload and sign are equal; a NaN against a number is not, either way round
    b = a.copy()
    b.view(np.uint32)[0, 4] = 0xffc00001
    assert np.isnan(b[0, 4]) and b.view(np.uint32)[0, 4] != a.view(np.uint32)[0, 4] and vc.bits_equal(b, a)
    b[0, 4] = 1.0
    assert not vc.bits_equal(b, a) and not vc.bits_equal(a, b)
    # float64 blocks by their 64-bit patterns; a dtype or shape mismatch is a mismatch
    d = np.array([0.0, 2.0 ** -1060, np.nan])
    assert vc.bits_equal(d, d.copy()) and not vc.bits_equal(np.array([-0.0, 2.0 ** -1060, np.nan]), d) and not vc.bits_equal(np.array([0.0, 0.0, np.nan]), d)
    assert not vc.bits_equal(d.astype(np.float32), d) and not vc.bits_equal(d[:2], d)
    # the message: the first differing element, both patterns, the reference's class
    b = a.copy()
    b[0, 2] = 0.0
    msg = vc.bits_diff(b, a)
    assert '(0, 2)' in msg and '0x00000000' in msg and ('0x%08x' % int(a.view(np.uint32)[0, 2])) in msg and 'subnormal' in msg, msg
    with pytest.raises(AssertionError, match='subnormal'):
        vc.assert_bits_equal(b, a, 'flushed')
    assert [vc.class_of(v) for v in (np.float32(np.nan), np.float32(-np.inf), np.float32(-0.0), np.float32(1e-40), np.float32(1.2e-38), 1e-310)] == ['nan', 'inf', 'zero', 'subnormal', 'normal', 'subnormal']


def test_the_process_keeps_subnormals():
    """After `import torch`: numpy's product, and the oracle's on a one-entry operator."""
    p = np.float32(2.0 ** -100) * np.float32(2.0 ** -40)
    assert p != 0 and vc.class_of(p) == 'subnormal'
    one = np.array([1.5 * 2.0 ** -100], dtype=np.float32)
    y = oracle.csr_matvecs((1, 1), np.array([0, 1], np.int32), np.array([0], np.int32), one, np.array([[2.0 ** -40]], dtype=np.float32))
    assert y.dtype == np.float32 and y[0, 0] == np.float32(1.5 * 2.0 ** -140) and vc.class_of(y[0, 0]) == 'subnormal'
    y = oracle.csr_matvecs((1, 1), np.array([0, 1], np.int32), np.array([0], np.int32), one.astype(np.float64) * 2.0 ** -900, np.array([[2.0 ** -40]], dtype=np.float32))
    assert y.dtype == np.float64 and y[0, 0] == 1.5 * 2.0 ** -1040 and vc.class_of(y[0, 0]) == 'subnormal'


def test_regime_transforms_keep_mantissas_and_the_homogeneous_row():
    rng = np.random.RandomState(1)
    X = rng.randn(50, 12).astype(np.float32)
    X[-1] = 1.0
    for (name, r) in vc.REGIMES.items():
        Y = r.apply(X, True, np.random.RandomState(2))
        assert Y.dtype == np.float32 and np.all(Y[-1] == 1.0) and np.array_equal(X[-1], np.ones(12, np.float32)), name
        if name in ('overflow', 'wide', 'by-column'):                   # a power-of-two factor: where the result is normal the mantissa and the sign are X's
            keep = np.isfinite(Y[:-1]) & (np.abs(Y[:-1]) >= np.finfo(np.float32).tiny)
            assert np.array_equal((Y[:-1].view(np.uint32) & 0x807fffff)[keep], (X[:-1].view(np.uint32) & 0x807fffff)[keep]), name
        if name == 'wide':
            col = np.flatnonzero(np.isinf(Y).any(axis=0))
            assert len(col) == 1 and sorted(Y[:, col[0]][np.isinf(Y[:, col[0]])]) == [-np.inf, np.inf]
        if name == 'signed-zero':
            assert set(np.unique(Y[:-1])) <= {-2.0, -1.0, 0.0, 1.0, 2.0} and np.any(np.signbit(Y[:-1]) & (Y[:-1] == 0)) and np.any(~np.signbit(Y[:-1]) & (Y[:-1] == 0))
    for n in (1, 2, 3, 8, 64, 256):
        c = vc.by_column_classes(n, np.random.RandomState(n))
        assert np.all(c[1:] != c[:-1]) and (n < 64 or len(set(c)) == 5)
    # the operator side: powers of two per entry (small-int: non-zero integers), the homogeneous row's own 1.0 kept
    dt = rng.randn(400).astype(np.float32)
    for kind in ('unit', 'unit-256', 'overflow', 'wide'):
        out = vc.values(kind, dt, 40, np.random.RandomState(3))
        assert np.array_equal(np.frexp(out)[0], np.frexp(dt)[0]), kind
    assert set(np.unique(vc.values('small-int', dt, 40))) == {-2.0, -1.0, 1.0, 2.0}
    assert 0.7 < np.sqrt(40) * np.sqrt(np.mean(vc.values('unit', dt, 40).astype(np.float64) ** 2)) < 1.42
    assert 2.8 < np.sqrt(40) * np.sqrt(np.mean(vc.values('overflow', dt, 40).astype(np.float64) ** 2)) < 5.7


@pytest.mark.parametrize('f64', [False, True], ids=['f32-operator', 'f64-operator'])
@pytest.mark.parametrize('regime', list(vc.REGIMES))
def test_oracle_matches_scipy_in_every_regime(regime, f64):
    """test_oracle_golden.test_oracle_matches_scipy_on_random_unsorted pins the C restatement at randn; here at every regime's magnitudes, under bits_equal."""
    rng = np.random.RandomState(len(regime) + 2 * f64)
    r = vc.REGIMES[regime]
    for k in (9, 70, 640):
        (shape, ip, ix, dt) = _random_csr(k, rng, m=120, f64=f64, ragged=True)               # (rows of 0 .. several k entries)
        dt = vc.csr_values(vc.variant_of(regime), shape, ip, ix, dt)
        X = r.apply(rng.randn(shape[1], 17).astype(np.float32), False, rng, k)
        with np.errstate(all='ignore'):
            got = oracle.csr_matvecs(shape, ip, ix, dt, X)
            ref = scipy.sparse.csr_matrix((dt, ix, ip), shape=shape).dot(X)
        assert got.dtype == ref.dtype == (np.float64 if f64 else np.float32)
        vc.assert_bits_equal(got, ref, '%s, %d entries per row' % (regime, k))


@pytest.mark.parametrize('regime', [n for (n, r) in vc.REGIMES.items() if r.floors])
def test_every_regime_meets_its_floors_at_the_gpu_modules_row_lengths(regime):
    r = vc.REGIMES[regime]
    for k in ROW_LENGTHS:
        rng = np.random.RandomState(k)
        (shape, ip, ix, dt) = _random_csr(k, rng, m=64 if k > 1000 else 200)
        dt = vc.csr_values(vc.variant_of(regime), shape, ip, ix, dt)
        X = r.apply(rng.randn(shape[1], 16).astype(np.float32), False, rng, k)
        with np.errstate(all='ignore'):
            ref = oracle.csr_matvecs(shape, ip, ix, dt, X)
        assert not vc.floors_missed(regime, ref), (regime, k, vc.share_text(ref))


def test_floors_on_factored_conv_operators_with_a_bias_column():
    """The bias entries follow the regime (Regime.bias_exp), so a bias column does not lift every output back to O(1)."""
    from test_parity_gpu import _filled_in_convtaps, _random_convtaps
    rng = np.random.RandomState(5)
    for W in (_random_convtaps(rng, 16, 64, 6, 3, 1, True, True), _filled_in_convtaps(rng, 3, 40, 6, 3, True)):
        for (regime, r) in vc.REGIMES.items():
            (W2, M) = vc.revalued_convtaps(W, vc.variant_of(regime))
            assert M.shape == W.shape and W2.shape == W.shape
            X = rng.randn(M.shape[1], 9).astype(np.float32)
            X[-1] = 1.0
            X = r.apply(X, True, rng, M.nnz / float(M.shape[0]))
            with np.errstate(all='ignore'):
                ref = oracle.csr_matvecs(M.shape, M.indptr, M.indices, M.data.astype(np.float32), X)
            assert not vc.floors_missed(regime, ref), (regime, vc.share_text(ref))
            assert np.all(ref[-1] == 1.0)


def test_the_reference_never_produces_minus_zero():
    """The premise of the +0.0 argument in kn_csr_mfma.hip: a running sum that starts at +0.0 and adds never becomes -0.0, whatever -0 products it meets -- so a
    product pipe that returns +0 for a -0 product cannot show in Y."""
    r = vc.REGIMES['signed-zero']
    for k in (1, 2, 6, 27, 145, 1060):
        rng = np.random.RandomState(100 + k)
        (shape, ip, ix, dt) = _random_csr(k, rng)
        dt = vc.csr_values(vc.variant_of('signed-zero'), shape, ip, ix, dt)
        X = r.apply(rng.randn(shape[1], 16).astype(np.float32), False, rng, k)
        prod = dt[:, None] * X[ix]
        assert np.any(np.signbit(prod) & (prod == 0)), k                  # -0 products do occur
        ref = oracle.csr_matvecs(shape, ip, ix, dt, X)
        zero = ref == 0
        assert zero.any() and not np.any(np.signbit(ref) & zero), k
