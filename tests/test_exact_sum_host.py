"""The host side of the exact-sum tests (tests/exact_sum.py; the device side is tests/test_exact_sum_gpu.py), on expanded operators of the shapes the GPU module runs,
built without a device handle: the premise -- under the 2^24 condition the oracle's float32 result IS the float64 product, and float32 evaluations in random term
orders, pairwise trees, a four-way split of K, fused and unfused, all give its bits -- and the teeth: three deliberately wrong evaluations (an operand rounded to
bf16's 8 significant bits, one term of +-1 dropped, one row's bias applied twice) fail bits_equal."""
import numpy as np
import pytest
import scipy.sparse

import exact_sum as xs
import oracle
import value_classes as vc
import test_conv_choice_gpu as cc
from test_parity_gpu import _filled_in_convtaps, _random_convtaps
from keynet_amd import sparse as ksp

# every operator of the launch-site rows that run under the tolerance (test_value_classes_gpu.TOLERANCE_ROWS), and the budget the issue expects for it
CC_NAMES = {'c3-o64': 19, 'c3-o128': 19, 'c3-o64-slots10': 19, 'c3-o128-slots10': 19, 'c16-o64': 16, 'c16-o64-coef': 16, 'c16-o128': 16, 'c16-o128-coef': 16, 'c16-o128-h8': 16,
            'c16-o64-two': 15, 'c32-o64-slots70': 12, 'c32-o128-slots70': 12}
N_COLS = 9                                  # columns 3 and 8 of a block cancel (exact_sum.zero_columns); 8 would hold one


def _cc_case(name, split, cap=None):
    (inshape, outshape, taps, eo, ei, et, ec, lc) = cc._factored(name, xs.variant(split, cap))
    W = ksp.Conv2dTiledMatrix.fromtaps(inshape, outshape, taps, eo, ei, et, ec, lc)
    M = W.tosparse('csr')
    M.sort_indices()
    B = xs.budget(int(np.diff(M.indptr).max()))
    (p, q) = xs.split_bits(B, split, cap)
    X = xs.activations(M.shape[1], N_COLS, True, p, seed=len(name), cin=inshape[0])
    xs.condition_factored(W, X, name)
    return (_csr(M), X, B, outshape[0])


def _csr(M):
    return (M.shape, M.indptr, M.indices, M.data.astype(np.float32))


def _conv_case(W, split):
    (W2, M, X, B) = xs.conv_case(W, split, N_COLS, seed=3)
    return (_csr(M), X, B, W2._outshape[0])


def _dense_case(split):
    D = xs.dense_values(split, 1100, 1024, seed=7)
    M = scipy.sparse.csr_matrix(D)
    (p, q) = xs.split_bits(xs.budget(1025), split)
    return (_csr(M), xs.activations(1025, N_COLS, True, p, seed=8), xs.budget(1025), 1100)


# the other operator shapes of the GPU module: 64-column tile cases, the small-K pipeline, the split application (fused expansion), the dense handle
OTHER = {
    'tile64-cin3-cout40-8x8-bias': lambda s: _conv_case(_random_convtaps(np.random.RandomState(1), 3, 40, 8, 3, 1, True, True), s),
    'tile64-cin48-cout128-7x7-coef-bias': lambda s: _conv_case(_random_convtaps(np.random.RandomState(2), 48, 128, 7, 3, 1, False, True), s),
    'tile64-cin32-cout128-12x12-9x9-groups': lambda s: _conv_case(_random_convtaps(np.random.RandomState(3), 32, 128, 12, 9, 1, False, True), s),
    'smallk-pipe-cin3-32x32': lambda s: _conv_case(_random_convtaps(np.random.RandomState(4), 3, 64, 32, 3, 1, True, True), s),
    'smallk-pipe-cin1-32x32-coef': lambda s: _conv_case(_random_convtaps(np.random.RandomState(5), 1, 64, 32, 3, 1, False, True), s),
    'split-16-64-6x6-fill5': lambda s: _conv_case(_filled_in_convtaps(np.random.RandomState(6), 16, 64, 6, 5, True), s),
    'split-3-40-8x8-fill3': lambda s: _conv_case(_filled_in_convtaps(np.random.RandomState(7), 3, 40, 8, 3, True), s),
    'split-32-128-4x4-fill6-nobias': lambda s: _conv_case(_filled_in_convtaps(np.random.RandomState(8), 32, 128, 4, 6, False), s),
    'dense-1100x1024': _dense_case,
}


def _case(name, split):
    return _cc_case(name, split) if name in CC_NAMES else OTHER[name](split)


def _sample_rows(csr, cout, rng, count=96):
    """`count` rows of the operator as padded term arrays (A [rows, L], column indices [rows, L]); half of them rows of the channels that cancel."""
    (shape, ip, ix, dt) = csr
    body = shape[0] - (1 if shape[0] % cout == 1 else 0)                # (a homogeneous last row)
    hw = max(1, body // cout)
    zrows = (xs.zero_channels(cout)[:, None] * hw + np.arange(hw)[None, :]).ravel()
    rows = np.unique(np.concatenate((rng.choice(zrows, size=min(len(zrows), count // 2), replace=False), rng.choice(shape[0], size=count // 2, replace=False))))
    L = int(np.diff(ip)[rows].max())
    (A, J) = (np.zeros((len(rows), L), np.float32), np.zeros((len(rows), L), np.int64))
    for (k, r) in enumerate(rows):
        (lo, hi) = (ip[r], ip[r + 1])
        A[k, :hi - lo] = dt[lo:hi]
        J[k, :hi - lo] = ix[lo:hi]
    return (rows, A, J)


def _sequential(A, Xg, order, fused):
    """float32 running sums over the terms in `order`: unfused rounds the product, then the sum; fused rounds a * x + s once (formed exactly in float64)."""
    s = np.zeros((A.shape[0], Xg.shape[2]), np.float32)
    for k in order:
        if fused:
            s = (A[:, k, None].astype(np.float64) * Xg[:, k].astype(np.float64) + s.astype(np.float64)).astype(np.float32)
        else:
            s = s + A[:, k, None] * Xg[:, k]
        assert s.dtype == np.float32
    return s


def _pairwise(A, Xg, order):
    p = A[:, order, None] * Xg[:, order]
    while p.shape[1] > 1:
        if p.shape[1] % 2:
            p = np.concatenate((p, np.zeros_like(p[:, :1])), axis=1)
        p = p[:, 0::2] + p[:, 1::2]
        assert p.dtype == np.float32
    return p[:, 0]


@pytest.mark.parametrize('name', sorted(CC_NAMES) + sorted(OTHER))
def test_the_premise_holds_on_every_operator_shape(name):
    rng = np.random.RandomState(sum(map(ord, name)))
    for split in xs.SPLITS:
        (csr, X, B, cout) = _case(name, split)
        if name in CC_NAMES:
            assert B == CC_NAMES[name], (name, B)
        worst = xs.condition(csr, X, name)
        ref = oracle.csr_matvecs(csr[0], csr[1], csr[2], csr[3], X)
        ref64 = scipy.sparse.csr_matrix((csr[3].astype(np.float64), csr[2], csr[1]), shape=csr[0]).dot(X.astype(np.float64))
        assert ref.dtype == np.float32 and np.array_equal(ref.astype(np.float64), ref64), (name, split)       # the oracle's float32 result IS the float64 product
        assert np.array_equal(ref64, np.rint(ref64)) and np.abs(ref64).max() <= xs.LIMIT
        zc = xs.zero_columns(N_COLS)
        (rows, A, J) = _sample_rows(csr, cout, rng)
        Xg = X[J]                                                      # [rows, L, columns]
        terms = A[:, :, None].astype(np.float64) * Xg
        cancel = (ref[rows][:, zc] == 0) & (np.abs(terms[:, :, zc]).sum(axis=1) > 0)
        assert (ref[rows][:, zc] == 0).any() and (cancel.any() or 'cin1' in name), (name, split, 'no sampled row cancels to zero')      # (one input channel: no pair to cancel)
        assert not np.signbit(ref[ref == 0]).any()
        want = np.ascontiguousarray(ref[rows])
        L = A.shape[1]
        for trial in range(3):
            order = rng.permutation(L)
            for fused in (False, True):
                vc.assert_bits_equal(_sequential(A, Xg, order, fused), want, '%s %s: sequential, fused=%d' % (name, split, fused))
            vc.assert_bits_equal(_pairwise(A, Xg, order), want, '%s %s: pairwise' % (name, split))
            parts = [_sequential(A, Xg, part, True) for part in np.array_split(order, 4)]                  # K split over four wavefronts, reduced in order
            vc.assert_bits_equal((parts[0] + parts[1]) + (parts[2] + parts[3]), want, '%s %s: four-way split of K' % (name, split))
        print('%-40s %-17s B=%d bits %s, max sum |a||x| = %.0f (%.2f of 2^24)' % (name, split, B, xs.split_bits(B, split), worst, worst / xs.LIMIT))


def _bf16(a):
    """float32 rounded to bf16's 8 significant bits, to nearest even."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def _oracle(csr, X, data=None):
    return oracle.csr_matvecs(csr[0], csr[1], csr[2], csr[3] if data is None else data, X)


MUTATED = ['c16-o64', 'c16-o64-coef', 'c3-o64', 'c32-o64-slots70', 'split-16-64-6x6-fill5', 'dense-1100x1024']


@pytest.mark.parametrize('name', MUTATED)
def test_three_wrong_evaluations_fail_bits_equal(name):
    """Each mutation has to fail on at least one split (the issue's bar); the rounded operand and the doubled bias are asserted to fail on the splits where the
    operand is wider than 8 bits / on every split, the dropped +-1 term wherever the case holds one."""
    failed = dict(act=[], val=[], drop=[], bias=[])
    for split in xs.SPLITS:
        (csr, X, B, cout) = _case(name, split)
        (shape, ip, ix, dt) = csr
        ref = _oracle(csr, X)
        (p, q) = xs.split_bits(B, split)
        # 1. one operand rounded to 8 significant bits
        if not vc.bits_equal(_oracle(csr, _bf16(X)), ref):
            failed['act'].append(split)
        if not vc.bits_equal(_oracle(csr, X, _bf16(dt)), ref):
            failed['val'].append(split)
        # 2. one term of one row dropped whose product is +-1
        rows_of = np.repeat(np.arange(shape[0]), np.diff(ip))
        ones = np.flatnonzero(np.abs(dt) == 1)
        hit = None
        for c in range(N_COLS):
            k = ones[np.abs(X[ix[ones], c]) == 1]
            if len(k):
                hit = (int(k[0]), c)
                break
        if hit is not None:
            (k, c) = hit
            d2 = dt.copy()
            d2[k] = 0
            y = ref.copy()
            y[rows_of[k], c] = _oracle(csr, X, d2)[rows_of[k], c]
            assert abs(float(y[rows_of[k], c]) - float(ref[rows_of[k], c])) == 1.0
            if not vc.bits_equal(y, ref):
                failed['drop'].append(split)
        # 3. the bias entry applied twice on one row
        bias = np.flatnonzero((ix == shape[1] - 1) & (dt != 0) & (rows_of < shape[0] - 1))
        if len(bias):
            d3 = dt.copy()
            d3[bias[len(bias) // 2]] *= 2
            if not vc.bits_equal(_oracle(csr, X, d3), ref):
                failed['bias'].append(split)
    print(name, failed)
    assert 'wide-activations' in failed['act'] and 'wide-values' in failed['val'], failed
    assert failed['drop'], 'no split of %s holds a term of +-1 whose loss shows: the generator is too weak' % name
    has_bias = name != 'split-32-128-4x4-fill6-nobias'
    assert not has_bias or failed['bias'] == list(xs.SPLITS), failed
