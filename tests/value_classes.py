"""Value classes of IEEE floats for the bit-exact contract (host code, no GPU): a comparison that sees every bit but a NaN's payload, the activation regimes that
put operands, products and sums at the edges of float32, the matching operator-value variants, and the share of each class a regime must reach in the REFERENCE's output.

bits_equal(got, ref)     where ref is NaN got must be NaN (any payload, any sign); everywhere else the uint32 (float64: uint64) patterns are equal.  -0.0 vs +0.0, the
                         sign of Inf and a flushed subnormal are mismatches.  bits_diff() gives the message: first differing element, both patterns, the reference's class.
REGIMES                  name -> Regime: a transform of a randn block X [cols, n] by powers of two only (the mantissas stay), the homogeneous row (where the operator
                         has one) kept at 1.0, the operator-value variant it goes with, and floors on the class shares of the oracle's output.  The floors are conditions
                         on the generator (a case that misses one is an error of the inputs), set below what the CPU oracle gives on rows of 9 .. 600 stored entries.
values(variant, ...)     the operator side: every variant scales the builder's values by powers of two (or, for `small-int`, replaces them by non-zero integers):
                         `unit`      one factor per operator that brings a row's sum to a standard deviation of about 1 (rms ~ 1 / sqrt(entries per row)): the regimes'
                                     thresholds (|y| < 2^-2 is subnormal under `boundary` ...) then cut the same share of every operator's output
                         `unit-256`  `unit` with the entries per row counted as at most 256 (the `underflow` regime on long rows)
                         `overflow`  4 x `unit`: magnitude ~ 4 / sqrt(entries per row)
                         `wide`      `unit` and a per-entry factor 2^e, e uniform in -40 .. 40
                         `small-int` sign(v) * (1 or 2): integer products and sums, exact zeros in the sums, -0 products under a -0.0 activation
conv_values(variant ...) a variant ('exact-sum', (split, cap)) hands the operator to tests/exact_sum.py: integer taps, coefficients and biases under a bit budget (the
                         inputs on which the kernels that may re-order a sum must give the oracle's bits; tests/test_exact_sum_gpu.py)
"""
import collections

import numpy as np

CLASSES = ('nan', 'inf', 'zero', 'subnormal', 'normal')


def classes(a):
    """The class index (into CLASSES) of every element of a float32 / float64 array."""
    a = np.asarray(a)
    assert a.dtype in (np.float32, np.float64), a.dtype
    tiny = np.finfo(a.dtype).tiny
    with np.errstate(all='ignore'):
        mag = np.abs(a)
        out = np.full(a.shape, 4, dtype=np.int8)
        out[mag < tiny] = 3
        out[mag == 0] = 2
        out[np.isinf(a)] = 1
        out[np.isnan(a)] = 0
    return out


def class_of(v):
    return CLASSES[int(classes(np.asarray([v]))[0])]


def shares(a):
    """{class: share of a's elements}."""
    c = classes(a)
    return {name: float(np.count_nonzero(c == k)) / max(1, c.size) for (k, name) in enumerate(CLASSES)}


def _patterns(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def bits_diff(got, ref):
    """'' where got equals ref bit for bit (a NaN of ref: any NaN), else a message naming the first differing element."""
    (got, ref) = (np.asarray(got), np.asarray(ref))
    if got.dtype != ref.dtype or got.dtype not in (np.float32, np.float64):
        return 'dtypes %s / %s (float32 or float64 on both sides)' % (got.dtype, ref.dtype)
    if got.shape != ref.shape:
        return 'shapes %s / %s' % (got.shape, ref.shape)
    (gb, rb) = (_patterns(got), _patterns(ref))
    rnan = np.isnan(ref)
    bad = np.where(rnan, ~np.isnan(got), gb != rb)
    if not bad.any():
        return ''
    at = tuple(int(v) for v in np.argwhere(bad)[0])
    width = 8 if got.dtype == np.float32 else 16
    return '%d of %d elements differ; first at %s: got 0x%0*x (%r, %s), reference 0x%0*x (%r, %s)' % (
        int(bad.sum()), bad.size, at, width, int(gb[at]), got[at], class_of(got[at]), width, int(rb[at]), ref[at], class_of(ref[at]))


def bits_equal(got, ref):
    return bits_diff(got, ref) == ''


def assert_bits_equal(got, ref, what=''):
    d = bits_diff(got, ref)
    assert not d, '%s: %s' % (what, d) if what else d


def relu_ref(ref):
    """torch's ReLU on the reference: a negative element becomes +0.0, -0.0 and NaN stay what they are."""
    return np.where(ref < 0, ref.dtype.type(0), ref)


def _p2(e):
    return np.ldexp(np.float32(1.0), np.asarray(e, dtype=np.int32)).astype(np.float32)


def _body(X, has_last):
    return X[:-1] if has_last else X


def _scaled(X, has_last, factor):
    Y = np.array(X, dtype=np.float32, copy=True)
    b = _body(Y, has_last)
    with np.errstate(all='ignore'):
        b *= factor
    return Y


BY_COLUMN_EXPONENTS = (-130, -124, 0, 60, 126)


def by_column_classes(n, rng):
    """One index into BY_COLUMN_EXPONENTS per column; neighbours always differ (the two halves of a packed instruction, the lanes of the narrow kernels)."""
    c = np.zeros(n, dtype=np.int64)
    c[0] = rng.randint(0, 5)
    for b in range(1, n):
        c[b] = (c[b - 1] + rng.randint(1, 5)) % 5
    return c


def _subnormal(X, has_last, rng, per_row=None):
    return _scaled(X, has_last, _p2(-130))


def _boundary(X, has_last, rng, per_row=None):
    return _scaled(X, has_last, _p2(-124))


def _underflow(X, has_last, rng, per_row=None):
    return _scaled(X, has_last, _p2(-147))


def _overflow(X, has_last, rng, per_row=None):
    return _scaled(X, has_last, _p2(126))


def _wide(X, has_last, rng, per_row=None):
    Y = _scaled(X, has_last, _p2(rng.randint(-60, 61, size=_body(X, has_last).shape)))
    b = _body(Y, has_last)
    col = int(rng.randint(0, b.shape[1]))
    rows = rng.choice(b.shape[0], size=2, replace=False)
    b[rows[0], col] = np.inf
    b[rows[1], col] = -np.inf
    return Y


def _by_column(X, has_last, rng, per_row=None):
    c = by_column_classes(X.shape[1], rng)
    return _scaled(X, has_last, _p2(np.asarray(BY_COLUMN_EXPONENTS)[c])[None, :])


def _signed_zero(X, has_last, rng, per_row=None):
    """Integers in -2 .. 2 (rint keeps the sign: -0.3 -> -0.0).  A row of more than 12 stored entries would almost never sum to zero: there all but about 12 of the
    activations a row reads become zeros of their own sign, which leaves short integer sums between many +0 and -0 products."""
    Y = np.array(X, dtype=np.float32, copy=True)
    b = _body(Y, has_last)
    b[...] = np.clip(np.rint(b), -2, 2)
    if per_row is not None and per_row > 12:
        b[rng.rand(*b.shape) >= 12.0 / per_row] *= np.float32(0.0)
    return Y


Regime = collections.namedtuple('Regime', 'name apply values bias_exp floors target')

# bias_exp: the operator's bias entries (the column the homogeneous row multiplies; x_last stays 1.0) are scaled by 2^bias_exp, so that bias * 1.0 -- an O(1) operand
# next to tiny ones -- lands in the class the regime is for instead of lifting every output back to O(1) (`by-column`: a subnormal bias next to sums of five magnitudes)
REGIMES = collections.OrderedDict((r.name, r) for r in (
    Regime('subnormal', _subnormal, 'unit', -130, {'subnormal': 0.90}, 'subnormal operands, products that are zero or a few quanta, subnormal sums'),
    Regime('boundary', _boundary, 'unit', -124, {'subnormal': 0.10, 'normal': 0.50}, 'sums that cross the normal / subnormal boundary both ways'),
    Regime('underflow', _underflow, 'unit-256', -147, {'subnormal': 0.70, 'zero': 0.03}, 'operands of 1 .. 8 quanta: products that round to zero or to one quantum'),
    Regime('overflow', _overflow, 'overflow', 0, {'inf': 0.20, '_finite': 0.25}, 'sums that overflow on the way, Inf - Inf behind them'),
    Regime('wide', _wide, 'wide', 0, {}, '120 binades of activations x 80 of operator values; one +Inf and one -Inf in one column'),
    Regime('by-column', _by_column, 'unit', -127, {}, 'neighbouring columns of different classes'),
    Regime('signed-zero', _signed_zero, 'small-int', 0, {'zero': 0.01}, 'integer operands with -0.0 activations: -0 products, sums that are exactly zero'),
))
FLUSH_REGIMES = ('subnormal', 'boundary', 'underflow')   # what a build that flushes denormals must fail
F32_CHAIN_REGIMES = ('subnormal', 'boundary', 'overflow', 'by-column')


def floors_missed(regime, ref):
    """The floors of `regime` the reference block `ref` misses: [] where the generator did its work."""
    s = shares(ref)
    s['_finite'] = s['zero'] + s['subnormal'] + s['normal']
    return ['%s share %.3f < %.2f' % (k, s[k], f) for (k, f) in REGIMES[regime].floors.items() if s[k] < f]


def share_text(ref):
    s = shares(ref)
    return ' '.join('%s %.1f%%' % (k, 100 * s[k]) for k in CLASSES if s[k] > 0)


def values(variant, v, per_row, rng=None, rms=None):
    """The operator values `v` (any shape, float32 or float64) under `variant`; per_row = stored entries of a typical row (or of each value's own row), rms = the root mean square of the values a
    row really sums where that is not v's own (a factored conv operator: taps x coefficients)."""
    v = np.asarray(v)
    if variant is None:
        return v
    if variant == 'small-int':
        return (np.where(v < 0, -1, 1) * np.where(np.abs(v) > 0.67 * _rms(v), 2, 1) * (v != 0)).astype(v.dtype)        # (a stored zero stays one)
    if rms is None:
        rms = _rms(v)
    per_row = np.maximum(1.0, np.asarray(per_row, dtype=np.float64))           # one figure, or one per element of v
    if variant == 'unit-256':                             # (products of operands of a few quanta with values below 1 / 16 would nearly all round to zero)
        (variant, per_row) = ('unit', np.minimum(per_row, 256.0))
    e = np.rint(np.log2(1.0 / (np.sqrt(per_row) * rms))).astype(np.int64) + (2 if variant == 'overflow' else 0)
    out = v * v.dtype.type(2.0) ** e
    if variant == 'wide':
        out = out * (v.dtype.type(2.0) ** rng.randint(-40, 41, size=v.shape)).astype(v.dtype)
    else:
        assert variant in ('unit', 'overflow'), variant
    return out.astype(v.dtype)


def _rms(v):
    v = np.asarray(v, dtype=np.float64)
    v = v[np.isfinite(v) & (v != 0)]
    return float(np.sqrt(np.mean(v * v))) if v.size else 1.0


def variant_of(regime):
    """(kind of values(), bias exponent): the operator variant a regime is used with; hashable, so a builder can cache on it."""
    r = REGIMES[regime]
    return (r.values, r.bias_exp)


def per_row_of(ip):
    lens = np.diff(np.asarray(ip))
    lens = lens[lens > 0]
    return float(lens.mean()) if lens.size else 1.0


def csr_values(variant, shape, ip, ix, dt, has_last=False, seed=0):
    """The data array of a CSR operator under variant = (kind, bias exponent) | None.  Every row gets the factor of its OWN length (one power of two per row: a
    short row beside long ones keeps sums of the same magnitude).  With a homogeneous column the entries in it are the biases (the last row's own entry, the 1.0
    that hands the homogeneous row on, is kept)."""
    if variant is None:
        return dt
    (kind, bias_exp) = variant
    (ip, ix, dt) = (np.asarray(ip), np.asarray(ix), np.asarray(dt))
    out = values(kind, dt, np.repeat(np.diff(ip), np.diff(ip)), np.random.RandomState(seed))
    if has_last:
        bias = ix == shape[1] - 1
        keep = np.zeros(len(dt), bool)
        keep[ip[-2]:ip[-1]] = bias[ip[-2]:ip[-1]]
        out[bias] = out[bias] * out.dtype.type(2.0) ** bias_exp
        out[keep] = dt[keep]
    return out


def conv_values(variant, taps, coef, lastcol, per_row, seed=0):
    """(taps, coef, lastcol) of a factored conv operator under variant: the taps carry the kind (coefficients are left as they are, `small-int` apart), the
    biases lastcol[:-1] the kind and the bias exponent, lastcol[-1] stays 1.0."""
    if variant is None:
        return (taps, coef, lastcol)
    (kind, bias_exp) = variant
    if kind == 'exact-sum':                               # (tests/exact_sum.py: integer operands under a bit budget; the variant's second field is (split, cap))
        import exact_sum
        return exact_sum.conv_values(bias_exp[0], taps, coef, lastcol, per_row, seed, cap=bias_exp[1])
    rng = np.random.RandomState(seed)
    rms = _rms(taps) * (_rms(coef) if coef is not None else 1.0)
    t = values(kind, taps, per_row, rng, rms=rms)
    c = coef
    if coef is not None and kind == 'small-int':
        c = values(kind, coef, per_row)
    lc = lastcol
    if lastcol is not None:
        lc = np.array(lastcol, dtype=np.float32, copy=True)
        b = values(kind, lc[:-1], 1.0, rng)
        lc[:-1] = b * np.float32(2.0) ** bias_exp
    return (t, c, lc)


def revalued_convtaps(W, variant, seed=0):
    """(the factored conv operator W -- a Conv2dTiledMatrix built by fromtaps, or a FactoredSparseMatrix around one -- with its values under `variant`, its sorted
    CSR): same structure, same entry lists.  The CSR of a FactoredSparseMatrix is the expansion without its exact zeros, as its builder forms it."""
    from keynet_amd import sparse as ksp
    factored = isinstance(W, ksp.FactoredSparseMatrix)
    F = W._factored if factored else W
    t = F._taps
    n_out = int(F._outshape[1]) * int(F._outshape[2])
    per_row = len(t['ent_out']) / float(n_out) * int(F._inshape[0])
    (taps, coef, lastcol) = conv_values(variant, t['taps'], t['ent_coef'], t['lastcol'], per_row, seed)
    F2 = ksp.Conv2dTiledMatrix.fromtaps(F._inshape, F._outshape, taps, t['ent_out'], t['ent_in'], t['ent_tap'], coef, lastcol)
    M = F2.tosparse('csr')
    M.sort_indices()
    if not factored:
        return (F2, M)
    M.eliminate_zeros()
    return (ksp.FactoredSparseMatrix(M.astype(np.float32), F2), M)
