"""Exact-sum inputs for the kernels that may re-order a sum (host code, no GPU): integer-valued operator values and activations under a bit budget, on which every
product and every partial sum of a row is exact in float32 -- in any order and any grouping, with or without fused multiply-add, over any split of K, and through the
three-way bf16 split (an operand of at most 16 significant bits has an exact zero as its third part, so the three dropped cross products are exact zeros).  On such
inputs a tolerance kernel has to return the oracle's bits: tests/test_exact_sum_gpu.py asks for them with value_classes.bits_equal, tests/test_exact_sum_host.py
checks the premise and that the inputs catch a lost mantissa bit, a dropped term of +-1 and a bias applied twice.

budget(n_max)            B = floor(log2(2^24 / n_max)), n_max the longest expanded row with its bias entry: every |a x| < 2^B, so sum |a| |x| <= n_max 2^B <= 2^24.
SPLITS                   how B is shared, as (activation bits, operator-value bits), all at full budget: `wide-activations` (B - 2, 2), `wide-values` (2, B - 2),
                         `balanced` (ceil(B / 2), floor(B / 2)); `cap` bounds either side (16 for the bf16 split).
integers(...)            random signs; six in ten magnitudes odd at the top width (the low bit is really used), the rest anywhere below it (so +-1 occur).
conv_values(...)         (taps, coefficients, lastcol) of a factored conv operator: integer taps, coefficients 1 or 2 (powers of two: coef * x and fl(coef * tap) are
                         exact and keep the operand's width, whichever the kernel forms), integer biases (one in ten zero), lastcol[-1] stays 1.0.
dense_values(...)        the same for a dense affine operator (bias column, homogeneous last row).
activations(...)         the integer block, one activation in ten zero, the homogeneous row 1.0.
Rows that sum to zero    output channels ZERO_CHANNELS (co % 8 == 5) read channel 2j + 1 through the taps of channel 2j and carry no bias; the batch columns ZERO_COLUMNS
                         (c % 7 == 3; the last column of a batch narrower than 4) hold x[2j + 1] = -x[2j] (an odd last channel: 0).  Those elements are sums of non-zero
                         terms that cancel exactly -- +0.0 in every order.
condition(...)           sum |a| |x| per output element in float64 on the expanded operator, asserted <= 2^24: a case that misses it is an error of this generator.
"""
import numpy as np
import scipy.sparse

LIMIT = 2.0 ** 24
KIND = 'exact-sum'
SPLITS = ('wide-activations', 'wide-values', 'balanced')
BF16X3_CAP = 16


def budget(n_max):
    B = int(np.floor(np.log2(LIMIT / float(n_max))))
    assert n_max * 2.0 ** B <= LIMIT < n_max * 2.0 ** (B + 1) and B >= 4, (n_max, B)
    return B


def split_bits(B, split, cap=None):
    """(activation bits, operator-value bits) of `split` at budget B."""
    (p, q) = {'wide-activations': (B - 2, 2), 'wide-values': (2, B - 2), 'balanced': ((B + 1) // 2, B // 2)}[split]
    if cap is not None:
        (p, q) = (min(p, cap), min(q, cap))
    assert p >= 2 and q >= 2 and p + q <= B
    return (p, q)


def variant(split, cap=None):
    """The operator-value variant value_classes.conv_values hands to conv_values() below (hashable: the builders cache on it)."""
    assert split in SPLITS
    return (KIND, (split, cap))


def integers(rng, shape, bits, zero_share=0.0):
    """int64: |v| < 2^bits, random signs, 60 % odd in [2^(bits-1), 2^bits), the rest uniform in [1, 2^bits); `zero_share` of them 0."""
    assert 1 <= bits <= 24
    top = rng.randint(1 << (bits - 1), 1 << bits, size=shape).astype(np.int64) | 1
    low = rng.randint(1, 1 << bits, size=shape).astype(np.int64)
    v = np.where(rng.rand(*shape) < 0.6, top, low) * np.where(rng.rand(*shape) < 0.5, -1, 1)
    if zero_share:
        v[rng.rand(*shape) < zero_share] = 0
    return v


def zero_channels(cout):
    z = np.flatnonzero(np.arange(cout) % 8 == 5)
    return z if len(z) else np.array([cout - 1])


def zero_columns(n):
    z = np.flatnonzero(np.arange(n) % 7 == 3)
    return z if len(z) else np.array([n - 1])


def conv_values(split, taps, coef, lastcol, per_row, seed=0, cap=None):
    """per_row: stored entries of the longest expanded row without its bias entry (slots of the fullest output pixel x input channels)."""
    rng = np.random.RandomState(seed + 17 * SPLITS.index(split))
    has_last = lastcol is not None
    B = budget(int(per_row) + (1 if has_last else 0))
    (p, q) = split_bits(B, split, cap)
    (ntaps, cout, cin) = taps.shape
    t = integers(rng, taps.shape, q - 1 if coef is not None else q)
    t[np.asarray(taps) == 0] = 0                                       # (a stored zero stays one)
    Z = zero_channels(cout)
    for j in range(cin // 2):
        t[:, Z, 2 * j + 1] = t[:, Z, 2 * j]
    c = None
    if coef is not None:
        c = np.where(rng.rand(len(coef)) < 0.5, 1, 2) * (np.asarray(coef) != 0)
        c = c.astype(np.float32)
    lc = None
    if has_last:
        bias = integers(rng, (len(lastcol) - 1,), min(B, cap or B), zero_share=0.1)
        hw = (len(lastcol) - 1) // cout
        bias.reshape(cout, hw)[Z] = 0
        lc = np.concatenate((bias, [1])).astype(np.float32)
    return (t.astype(np.float32), c, lc)


def dense_values(split, outs, ins, seed=0, cap=None):
    """D [outs + 1, ins + 1] float32 of a dense affine operator (a keyed Linear: bias column, homogeneous last row): rows r % 8 == 5 hold d[2j + 1] = d[2j] and no bias."""
    rng = np.random.RandomState(seed + 17 * SPLITS.index(split))
    B = budget(ins + 1)
    (p, q) = split_bits(B, split, cap)
    D = np.zeros((outs + 1, ins + 1), dtype=np.int64)
    D[:-1, :-1] = integers(rng, (outs, ins), q)
    D[:-1, -1] = integers(rng, (outs,), min(B, cap or B), zero_share=0.1)
    Z = zero_channels(outs)
    D[Z, -1] = 0
    D[Z[:, None], np.arange(1, ins, 2)[None, :]] = D[Z[:, None], np.arange(0, ins - 1, 2)[None, :]]
    if ins % 2:
        D[Z, ins - 1] = 0
    D[-1, -1] = 1
    return D.astype(np.float32)


def activations(cols, n, has_last, bits, seed=0, cin=None):
    """X [cols, n] float32 of integers below 2^bits; the body rows are cin planes of equal length (None: one row each) for the columns that cancel."""
    rng = np.random.RandomState(seed)
    body = cols - (1 if has_last else 0)
    cin = body if cin is None else cin
    assert cin > 0 and body % cin == 0, (cols, cin)
    hw = body // cin
    X = integers(rng, (cin, hw, n), bits, zero_share=0.1)
    Cz = zero_columns(n)
    for j in range(cin // 2):
        X[2 * j + 1][:, Cz] = -X[2 * j][:, Cz]
    if cin % 2:
        X[cin - 1][:, Cz] = 0
    X = X.reshape(body, n)
    if has_last:
        X = np.concatenate((X, np.ones((1, n), np.int64)))
    return np.ascontiguousarray(X.astype(np.float32))


def condition(csr, X, what=''):
    """max over the output elements of sum |a| |x| (float64, on the expanded operator csr = (shape, indptr, indices, data)); asserted <= 2^24."""
    (shape, ip, ix, dt) = csr
    A = scipy.sparse.csr_matrix((np.abs(np.asarray(dt, dtype=np.float64)), ix, ip), shape=shape)
    S = A.dot(np.abs(np.asarray(X, dtype=np.float64)))
    worst = float(S.max()) if S.size else 0.0
    assert worst <= LIMIT, '%s: sum |a| |x| = %.0f > 2^24: the generator missed its own condition' % (what, worst)
    dt = np.asarray(dt)
    assert np.array_equal(dt, np.rint(dt)) and np.array_equal(X, np.rint(X)), '%s: non-integer operands' % what
    return worst


def abs_operator(W):
    """The factored operator W with |taps|, |coef|, |lastcol|: its expansion times |X| is sum |tap| |coef| |x| over the TERMS of the triple product."""
    from keynet_amd import sparse as ksp
    t = W._taps
    return ksp.Conv2dTiledMatrix.fromtaps(W._inshape, W._outshape, np.abs(t['taps']), t['ent_out'], t['ent_in'], t['ent_tap'],
                                          None if t['ent_coef'] is None else np.abs(t['ent_coef']), None if t['lastcol'] is None else np.abs(t['lastcol']))


def condition_factored(W, X, what=''):
    """condition() on the fully expanded triple product tap x coefficient x activation of a factored operator (pairs hit by several taps count every term)."""
    A = abs_operator(W).tosparse('csr')
    return condition((A.shape, A.indptr, A.indices, A.data), X, what)


def longest_row(W):
    """Stored entries of the longest expanded row of a factored operator, bias entry not counted: slots of its fullest output pixel x input channels."""
    t = W._taps
    return int(np.bincount(t['ent_out']).max()) * int(W._inshape[0])


def revalued(W, split, seed=0, cap=None):
    """(the factored conv operator W with exact-sum values, its sorted CSR, the budget B it ran at): same structure, same entry lists."""
    from keynet_amd import sparse as ksp
    t = W._taps
    per_row = longest_row(W)
    (taps, coef, lastcol) = conv_values(split, t['taps'], t['ent_coef'], t['lastcol'], per_row, seed, cap)
    W2 = ksp.Conv2dTiledMatrix.fromtaps(W._inshape, W._outshape, taps, t['ent_out'], t['ent_in'], t['ent_tap'], coef, lastcol)
    M = W2.tosparse('csr')
    M.sort_indices()
    return (W2, M, budget(per_row + (1 if lastcol is not None else 0)))


def conv_case(W, split, n, seed=0, cap=None):
    """revalued(W) with its activation block [cols, n]: (W2, M, X, B), the 2^24 condition asserted on the triple product."""
    (W2, M, B) = revalued(W, split, seed, cap)
    (p, q) = split_bits(B, split, cap)
    X = activations(W2.shape[1], n, W2._taps['lastcol'] is not None, p, seed + 1, cin=int(W2._inshape[0]))
    condition_factored(W2, X, 'conv case %s' % split)
    return (W2, M, X, B)
