"""Seeded case generators of the narrow-kernel fuzzers (tests/test_fuzz_narrow_gpu.py) -- pure host code, no torch device use, so tests/test_fuzz_narrow_host.py
runs them without a GPU: conv-taps operators of seven classes with a width, a flag word, a column window, non-finite activations and a screen slot (conv_cases);
structured float32 / float64 CSR operators with the two CSR narrow flags (csr_cases); source networks with a key family, a batch and a VALID narrow keyword set
(model_cases, narrow_keywords).  Every generator draws EVERYTHING of a case from a seeded RandomState in a fixed order and yields the case whole, so `only=` of the
fuzzers re-runs one case of a longer run exactly as that run draws it.

The kernels behind the flags take their forms by rules on the operator and the width (narrow_choice, kn_conv.hip): a form such as P = 2 or the two-launch column split
needs an operator class, a width range and a set of flag bits at once, and independent draws would meet it a few times in a thousand cases.  So a case first draws
its class (evenly, the wide one in ten: conv_plan), then an AIM among those of the class -- a width range and the flag bits a form needs -- and everything the
aim leaves open at random.  'free' aims leave everything open.  About one conv case in four (never a dropped-zero one, whose CSR is given) is then turned into its
exact-sum twin (exact_sum_twin: same shape, flags and window, integer values and activations whose sums are exact in every order).  conv_props / conv_classes / csr_classes compute the HOST-VISIBLE classes of an operator from W._taps and the CSR alone: the
create-time facts the library decides eligibility by (kn_internal.h: narrow_taps_ok, narrow_fill_ok, convtaps_pt_eligibility), restated, never read from a plan."""
import numpy as np
import scipy.sparse
import torch
from torch import nn

import exact_sum
import oracle
from keynet_amd import _capi
from keynet_amd import sparse as ksp
from test_parity_gpu import _random_convtaps
from test_narrow_taps_gpu import _coef_convtaps
from test_narrow_gpu import _dropped_zero_operator
from fuzz_nets import random_net

(RELU, EXACT, NARROW, MFMA, ROWS, N32, N64, N64M, LINEAR, TAPS) = (_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_NARROW, _capi.KN_FLAG_NARROW_MFMA, _capi.KN_FLAG_NARROW_ROWS,
                                                                  _capi.KN_FLAG_NARROW32, _capi.KN_FLAG_NARROW64, _capi.KN_FLAG_NARROW64_MFMA, _capi.KN_FLAG_NARROW_LINEAR, _capi.KN_FLAG_NARROW_TAPS)
(TAPS32, FILL) = (_capi.KN_MODIFIER_NARROW_TAPS32, _capi.KN_MODIFIER_NARROW_FILL)

WIDTHS = [1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 24, 31, 32, 33, 47, 63, 64]
(W8, W32, W64) = ([n for n in WIDTHS if n <= 8], [n for n in WIDTHS if 8 < n <= 32], [n for n in WIDTHS if n > 32])
NONFINITE = [np.inf, -np.inf, np.nan]
ORACLE_BUDGET = 2e7                   # Cout x Cin x entries of a conv case the oracle and the host expansion get through in about a second
CONV_CLASSES = ['canonical', 'coef', 'summed', 'fill', 'ineligible', 'dropped', 'wide']
# what a class's cases aim at: (width list | None, regime 'lane' | 'mfma' | None, modifier bits that are set, modifier bits that stay clear)
CONV_AIMS = {
    'canonical': [('free', None, None, 0, 0), ('taps', W8, 'lane', TAPS, FILL), ('taps32', W32, 'lane', TAPS | TAPS32, FILL), ('pipe64', W64, 'lane', 0, 0), ('tile64', W64, 'mfma', 0, EXACT)],
    'coef': [('free', None, None, 0, 0), ('taps', W8, 'lane', TAPS, FILL), ('taps-two-blocks', [5, 7, 8], 'lane', TAPS, FILL), ('taps-16-rows', W8, 'lane', TAPS, FILL),
             ('taps32', W32, 'lane', TAPS | TAPS32, FILL)],
    'summed': [('free', None, None, 0, 0)],
    'fill': [('free', None, None, 0, 0), ('fill', W8, 'lane', FILL, 0), ('fill-blocks', W32, 'lane', FILL, 0)],
    'ineligible': [('free', None, None, 0, 0), ('modifiers', W8 + W32, 'lane', TAPS | TAPS32 | FILL, 0)],
    'dropped': [('free', None, None, 0, 0), ('taps', W8, 'lane', TAPS, FILL)],
    'wide': [('pairs', [1, 2], 'lane', TAPS, FILL), ('taps32-16', [9, 12, 15, 16], 'lane', TAPS | TAPS32, FILL), ('taps32-32', [17, 24, 31, 32], 'lane', TAPS | TAPS32, FILL),
             ('mfma-two-tiles', [3, 4], 'mfma', 0, EXACT)],
}


def _taps_of(W):
    """The factored description of a conv operator: its own, or that of the factored stand-in of an untiled CSR (FactoredSparseMatrix)."""
    return getattr(W, '_factored', W)._taps


def _shapes_of(W):
    F = getattr(W, '_factored', W)
    return (F._inshape, F._outshape)


def conv_props(W):
    """The host-visible facts of a conv-taps operator, from W._taps alone -- what kn_convtaps_create records and the eligibility rules of the narrow kernels read:
    slots = entries with a non-zero coefficient on a tap that is not zero altogether."""
    t = _taps_of(W)
    ((Cin, Hi, Wi), (Cout, Ho, Wo)) = _shapes_of(W)
    (Pin, Pout, ntaps) = (Hi * Wi, Ho * Wo, int(t['taps'].shape[0]))
    live = np.array([bool(np.any(t['taps'][k] != 0)) for k in range(ntaps)])[t['ent_tap']]
    if t['ent_coef'] is not None:
        live &= t['ent_coef'] != 0
    (eo, ei, et) = (t['ent_out'][live].astype(np.int64), t['ent_in'][live].astype(np.int64), t['ent_tap'][live].astype(np.int64))
    per_pixel = np.bincount(eo, minlength=Pout)
    max_slots = int(per_pixel.max()) if len(eo) else 0
    summed = len(np.unique(eo * Pin + ei)) < len(eo)                    # some (output, input) pixel pair holds several slots: stored values are sums
    max_pair = int(np.bincount(np.unique(eo * Pin + ei, return_inverse=True)[1]).max()) if len(eo) else 0      # the most slots on one (output, input) pixel pair
    max_pair_tap = int(np.bincount(np.unique(eo * ntaps + et, return_inverse=True)[1]).max()) if len(eo) else 0
    coef = t['ent_coef'] is not None and bool(np.any(t['ent_coef'][live] != 1))
    p = dict(Cin=Cin, Cout=Cout, pixels=Pout, ntaps=ntaps, slots=int(len(eo)), max_slots=max_slots, summed=summed, coef=coef, max_pair=max_pair, max_pair_tap=max_pair_tap,
             items=Pout * ((Cout + 63) // 64), empty_pixels=bool(np.any(per_pixel == 0)), bias=t['lastcol'] is not None)
    p['taps_ok'] = (not summed) and len(eo) > 0 and max_slots <= 9 and 1 <= ntaps <= 16          # KN_FLAG_NARROW_TAPS, KN_MODIFIER_NARROW_TAPS32
    p['fill_ok'] = (summed or max_slots > 64) and 1 <= ntaps <= 16                                # KN_FLAG_NARROW_FILL
    p['mfma_ok'] = ntaps > 0 and max_slots <= 64 and max_pair_tap <= 2                            # KN_FLAG_NARROW_MFMA's kernel
    return p


def conv_classes(p):
    """The host-visible classes of tests/test_fuzz_narrow_host.py an operator with the facts `p` belongs to."""
    c = set()
    if p['max_slots'] <= 9 and p['ntaps'] <= 16 and not p['summed']:
        c.add('slots<=9,taps<=16')
    if p['coef']:
        c.add('coefficients')
    if 10 <= p['ntaps'] <= 16 and not p['summed']:
        c.add('taps 10..16')
    if p['summed']:
        c.add('summed values')
    if p['max_pair'] >= 3:                                              # filled in: more taps on a pixel pair than the second, float-weighted entries of _random_convtaps(unit=False) put there (two)
        c.add('filled, taps <= 16' if p['ntaps'] <= 16 else 'filled, taps > 16')
    if p['max_pair_tap'] > 2:
        c.add('>2 slots on a (pixel, tap) pair')
    if p['items'] >= 4096:
        c.add('>= 4096 work items')
    if p['empty_pixels']:
        c.add('empty pixels')
    if p['Cout'] % 64:
        c.add('Cout % 64 != 0')
    return c


def _without_pixels(rng, W):
    """The operator without the entries of a few output pixels: pixels with no slot at all (their rows hold the bias entry alone, or nothing)."""
    t = W._taps
    Pout = W._outshape[1] * W._outshape[2]
    gone = rng.choice(Pout, size=int(rng.randint(1, max(2, Pout // 8 + 1))), replace=False)
    keep = ~np.isin(t['ent_out'], gone)
    if not keep.any():
        keep[0] = True
    return ksp.Conv2dTiledMatrix.fromtaps(W._inshape, W._outshape, t['taps'], t['ent_out'][keep], t['ent_in'][keep], t['ent_tap'][keep],
                                          None if t['ent_coef'] is None else t['ent_coef'][keep], t['lastcol'])


def _filled(rng, eligible, has_last):
    """A filled-in operator in the manner of fuzz_convtaps: random (output, input) pixel pairs, several taps on a pair, entries in no order.  `eligible`: at most 16
    taps and a pair with two of them (the fill kernel's operators); else 17 .. 25 taps, or at most 16 with an output pixel that holds one tap on three input pixels
    (no matrix-core narrow form)."""
    (Cin, Cout) = (int(rng.choice([1, 2, 3, 4, 5, 8, 16, 17])), int(rng.choice([1, 5, 24, 40, 64, 72, 128, 192])))
    (hi, wi, ho, wo) = [int(v) for v in rng.randint(1, 9, size=4)]
    (Pin, Pout) = (hi * wi, ho * wo)
    many = (not eligible) and rng.rand() < 0.5
    ntaps = int(rng.choice([17, 20, 25])) if many else int(rng.choice([2, 4, 9, 13, 16]))
    taps = (rng.randn(ntaps, Cout, Cin) / np.sqrt(max(Cin, 1))).astype(np.float32)
    max_in = int(rng.choice([1, 3, 9, 40]))
    coef = bool(rng.rand() < 0.5)
    (eo, ei, et, ec) = ([], [], [], [])
    for o in range(Pout):
        for i in rng.choice(Pin, size=rng.randint(0 if rng.rand() < 0.1 else 1, min(Pin, max_in) + 1), replace=False):
            for k in rng.choice(ntaps, size=int(rng.randint(1, min(ntaps, 6) + 1)), replace=False):      # entry order, not tap order
                eo.append(o); ei.append(int(i)); et.append(int(k)); ec.append(np.float32(1.0) if rng.rand() < 0.2 else np.float32(rng.randn()))
    o = int(rng.randint(Pout))
    if eligible or many:                                                # a pair with two taps: stored values summed
        i = int(rng.randint(Pin))
        have = set(k for (a, b, k) in zip(eo, ei, et) if a == o and b == i)
        for k in [k for k in range(ntaps) if k not in have][:max(0, 2 - len(have))]:
            eo.append(o); ei.append(i); et.append(k); ec.append(np.float32(rng.randn()))
    elif Pin >= 3:                                                      # one tap on three input pixels of one output pixel
        k = int(rng.randint(ntaps))
        have = set(b for (a, b, kk) in zip(eo, ei, et) if a == o and kk == k)
        for i in [i for i in range(Pin) if i not in have][:max(0, 3 - len(have))]:
            if not any(a == o and b == i and kk == k for (a, b, kk) in zip(eo, ei, et)):
                eo.append(o); ei.append(i); et.append(k); ec.append(np.float32(rng.randn()))
    lastcol = None
    if has_last:
        lastcol = np.concatenate((rng.randn(Cout * Pout), [1.0])).astype(np.float32)
        lastcol[rng.randint(0, Cout * Pout, size=3)] = 0.0
    return ksp.Conv2dTiledMatrix.fromtaps((Cin, hi, wi), (Cout, ho, wo), taps, np.array(eo, np.int32), np.array(ei, np.int32), np.array(et, np.int32),
                                          np.array(ec, np.float32) if coef else None, lastcol)


def _conv_operator(rng, cls, aim, has_last):
    """(W, M): an operator of class `cls` and -- the dropped-zero class alone -- the CSR it stands for (every other class: its own sorted expansion, conv_reference)."""
    (Cin, Cout) = (int(rng.choice([1, 2, 3, 4, 5, 8, 16, 17])), int(rng.choice([1, 5, 24, 40, 64, 72, 128, 192])))
    (k, stride, H) = (int(rng.choice([1, 3])), int(rng.choice([1, 2])), int(rng.randint(3, 13)))
    if cls == 'canonical':
        return (_random_convtaps(rng, Cin, Cout, H, k, stride, True, has_last), None)
    if cls == 'coef':
        many = aim == 'taps-16-rows' or rng.rand() < 1.0 / 3
        if many:
            (k, H) = (3, max(H, 4 * stride))                            # (nine slots on the inner pixels: every one of the 10 .. 16 taps in use, as _coef_convtaps asserts)
        return (_coef_convtaps(rng, Cin, Cout, H, k, stride, has_last, ntaps=int(rng.randint(10, 17)) if many else None), None)
    if cls == 'summed':
        return (_random_convtaps(rng, Cin, Cout, H, 3, stride, False, has_last), None)
    if cls == 'fill':
        return (_filled(rng, True, has_last), None)
    if cls == 'ineligible':
        return (_filled(rng, False, has_last), None)
    if cls == 'dropped':
        (Cin, Cout, H) = (int(rng.choice([3, 5, 8, 16])), int(rng.choice([24, 40, 64, 72])), int(rng.randint(6, 11)))
        while True:
            try:
                return _dropped_zero_operator(rng, Cin, Cout, H)
            except AssertionError:                                      # (no tap entry drew a zero: draw again)
                pass
    # wide: >= 4 096 (pixel x 64-channel block) work items, tiny channel counts; 91 x 91 pixels where the aim needs 4 096 pixel PAIRS or 1 024 tiles of 32 (pixel, image) columns
    (Cin, Cout) = (int(rng.choice([1, 2, 3])), int(rng.choice([1, 5, 24, 40, 64])))
    Ho = 91 if aim in ('pairs', 'mfma-two-tiles') else int(rng.choice([64, 67]))
    stride = int(rng.choice([1, 1, 2]))
    return (_random_convtaps(rng, Cin, Cout, Ho * stride, 3, stride, True, has_last), None)


def conv_flags(rng, n, regime, on, off):
    """The flag word of a conv case: the regime bits `n` needs, a random subset of EXACT, RELU and the three modifiers (`on` set, `off` clear), in one case in
    four the wider regime bits as well, in one case in five NARROW_ROWS | NARROW_LINEAR (which a conv-taps handle ignores)."""
    f = NARROW if regime == 'lane' else MFMA
    wider = rng.rand() < 0.25
    if n > 8 or wider:
        f |= N32
    if n > 32 or wider:
        f |= N64 | (N64M if regime == 'mfma' else 0)
    for bit in (EXACT, RELU, TAPS, TAPS32, FILL):
        if rng.rand() < 0.5:
            f |= bit
    if f & TAPS32 and rng.rand() < 0.7:
        f |= TAPS                                                       # (the second modifier means something next to the first alone)
    f = (f | on) & ~off
    if rng.rand() < 0.2:
        f |= ROWS | LINEAR
    return int(f)


def _window(rng, n):
    """(ld, start) of a case's blocks: half of the cases compact, half a window of a wider block."""
    if rng.rand() < 0.5:
        return (n, 0)
    (start, pad) = (int(rng.randint(0, 6)), int(rng.choice([0, 1, 3, 37])))
    return (start + n + pad, start)


def _nonfinite(rng, rows, n):
    return [(int(rng.randint(rows)), int(rng.randint(n)), float(NONFINITE[rng.randint(3)])) for _ in range(int(rng.randint(1, 4)))] if rng.rand() < 0.2 else []


def conv_plan(n_cases, seed):
    """[(class, aim)] of the cases of a run, from a stream of their own (a seed's reach can be read off without building an operator).  Evenly, not independently:
    every ten cases hold one wide operator and each other class once, the other three drawn, in a shuffled order; a class walks through its aims in shuffled rounds."""
    top = np.random.RandomState(seed)
    (plan, rounds) = ([], dict((c, []) for c in CONV_CLASSES))
    while len(plan) < n_cases:
        block = ['wide'] + CONV_CLASSES[:6] + [CONV_CLASSES[int(k)] for k in top.randint(6, size=3)]
        for cls in [block[k] for k in top.permutation(len(block))]:
            if not rounds[cls]:
                rounds[cls] = [CONV_AIMS[cls][k] for k in top.permutation(len(CONV_AIMS[cls]))]
            plan.append((cls, rounds[cls].pop()))
    return plan[:n_cases]


def conv_cases(n_cases, seed, only=None):
    """Yields one dict per case: `skipped` (a reason) or the whole case -- cls, aim, W, M (None: the sorted expansion), props, n, flags, ld, start, X [cols, 128] (the
    case's batch is its first n columns; non-finite values already in), nonfinite, screen, twin (an exact-sum twin: exact_sum_twin).  Class and aim come from conv_plan, everything else from a stream of the
    case's own (seed, case): `only` yields that one case of the run, exactly as the whole run draws it."""
    for (case, (cls, (aim, widths, regime, on, off))) in enumerate(conv_plan(n_cases, seed)):
        if only is not None and case != only:
            continue
        rng = np.random.RandomState((seed * 1000003 + case) % (1 << 32))
        has_last = bool(rng.rand() < 0.6)
        (W, M) = _conv_operator(rng, cls, aim, has_last)
        if cls not in ('dropped', 'fill', 'ineligible') and rng.rand() < 0.25:
            W = _without_pixels(rng, W)
        n = int(rng.choice(widths if widths is not None else WIDTHS))
        flags = conv_flags(rng, n, regime if regime is not None else ('lane' if rng.rand() < 0.6 else 'mfma'), on, off)
        (ld, start) = _window(rng, n)
        X = rng.randn(W.shape[1], 128).astype(np.float32)
        nonfinite = _nonfinite(rng, W.shape[1] - 1 if W.shape[1] > 1 else 1, n)
        for (r, c, v) in nonfinite:
            X[r, c] = v
        if _taps_of(W)['lastcol'] is not None:
            X[-1] = 1.0
        screen = bool(rng.rand() < 0.25)
        twin = bool(cls != 'dropped' and rng.rand() < 0.25)              # (the last draw of the case's stream: everything above is what it was before there were twins)
        if twin:
            (W, X, nonfinite) = (exact_sum_twin(W, X.shape[1], case) + ([],))
        p = conv_props(W)
        d = dict(case=case, cls=cls, aim=aim, props=p, n=n, flags=flags, ld=ld, start=start, nonfinite=nonfinite, screen=screen, skipped=None, twin=twin)
        if p['Cout'] * p['Cin'] * len(_taps_of(W)['ent_out']) > ORACLE_BUDGET:
            d['skipped'] = 'oracle budget'
        else:
            d.update(W=W, M=M, X=X)
        yield d


def exact_sum_twin(W, n_cols, case):
    """(W, X [cols, n_cols]): the exact-sum twin of a conv case (tests/exact_sum.py) -- the operator's shape and entry lists as drawn, integer taps, coefficients 1 | 2, integer
    biases and activations, the split of the bit budget walking with the case number; sum |tap| |coef| |x| over the terms of every output element <= 2^24, asserted.  On such a
    case every order of the sum gives the oracle's bits, so the fuzzer holds a matrix-core plan to bits_equal instead of its bound.  No non-finite activations."""
    split = exact_sum.SPLITS[case % 3]
    t = W._taps
    per_row = exact_sum.longest_row(W)
    (taps, coef, lastcol) = exact_sum.conv_values(split, t['taps'], t['ent_coef'], t['lastcol'], per_row, seed=case)
    W2 = ksp.Conv2dTiledMatrix.fromtaps(W._inshape, W._outshape, taps, t['ent_out'], t['ent_in'], t['ent_tap'], coef, lastcol)
    (p_bits, _) = exact_sum.split_bits(exact_sum.budget(per_row + (1 if lastcol is not None else 0)), split)
    X = exact_sum.activations(W2.shape[1], n_cols, W2._taps['lastcol'] is not None, p_bits, seed=case + 1, cin=int(W2._inshape[0]))
    exact_sum.condition_factored(W2, X, 'exact-sum twin of conv case %d' % case)
    return (W2, X)


def conv_reference(d):
    """The CSR the oracle judges a conv case by: the operator's sorted canonical expansion (a pair's terms summed in entry order), or the CSR a factored stand-in stands for."""
    if d['M'] is None:
        M = d['W'].tosparse('csr')
        M.sort_indices()
        d['M'] = M
    return d['M']


def conv_abs_sum(d):
    """sum |w| |x| over the TERMS of every output element of a finite conv case, float64 [rows, n]: the scale of fuzz_convtaps' matrix-core bound."""
    W = getattr(d['W'], '_factored', d['W'])
    t = W._taps
    A = ksp.Conv2dTiledMatrix.fromtaps(W._inshape, W._outshape, np.abs(t['taps']), t['ent_out'], t['ent_in'], t['ent_tap'],
                                       None if t['ent_coef'] is None else np.abs(t['ent_coef']), None if t['lastcol'] is None else np.abs(t['lastcol']))
    return A.tosparse('csr').astype(np.float64).dot(np.abs(d['X'][:, :d['n']].astype(np.float64)))


def oracle_product(M, X, relu=False):
    """oracle.csr_matvecs on a scipy CSR in its stored order; ReLU as torch applies it (np.maximum loses NaN)."""
    with np.errstate(all='ignore'):
        ref = oracle.csr_matvecs(M.shape, M.indptr, M.indices, M.data, X)
        return np.where(ref < 0, ref.dtype.type(0), ref) if relu else ref


def describe(d):
    """One line that pins a case: the determinism check compares these."""
    keys = [k for k in ('case', 'cls', 'aim', 'twin', 'kind', 'n', 'flags', 'ld', 'start', 'nonfinite', 'screen', 'skipped', 'relu', 'f64', 'big', 'family', 'tile', 'inshape', 'names', 'keywords', 'float_keys') if k in d]
    s = ' '.join('%s=%s' % (k, d[k]) for k in keys)
    if d.get('props'):
        s += ' ' + ' '.join('%s=%s' % kv for kv in sorted(d['props'].items()))
    for k in ('X', 'data', 'indices'):
        if d.get(k) is not None:
            a = np.nan_to_num(np.asarray(d[k], dtype=np.float64), nan=3.0, posinf=5.0, neginf=-5.0)
            s += ' %s:%s:%.9g' % (k, a.shape, float(a.sum()))
    return s


# ------------------------------------------------------------------------------------------------------------------ CSR operators
def csr_cases(n_cases, seed):
    """Yields one dict per case: fuzz_csr's row kinds (loose rows, pattern groups of 2 .. 600 members, members that lost entries, one long row with duplicates, empty
    rows, explicit zeros, unsorted columns, scattered groups) at sizes the oracle handles in milliseconds; one case in four a keyed-Linear-like operator -- one big
    group over nearly all of 2 048 .. 4 096 columns with 64 .. 300 rows (from 256 on the library's big pattern group: 64-row slices, a last partial one) plus a few
    odd rows --; one case in eight in float64.  With it: n, flags (NARROW_ROWS, NARROW_LINEAR, both; next to conv regime bits in half of the cases), ld, start,
    X [cols, n], nonfinite, screen, relu."""
    rng = np.random.RandomState(seed)
    for case in range(n_cases):
        linear = bool(rng.rand() < 0.25)
        rows = []
        big = False
        if linear:
            n_cols = int(rng.randint(2048, 4097))
            pattern = rng.permutation(n_cols)[:int(rng.randint(n_cols - 3, n_cols + 1))].astype(np.int32)
            members = int(rng.choice([64, 100, 256, 257, 300, 300]))
            big = members >= 256 and len(pattern) >= 2048
            rows = [pattern] * members + [rng.randint(0, n_cols, rng.randint(0, 9)).astype(np.int32) for _ in range(int(rng.randint(0, 6)))]
            if rng.rand() < 0.3:                                        # a second, small group and loose rows behind it
                small = rng.randint(0, n_cols, rng.randint(1, 60)).astype(np.int32)
                rows += [small] * int(rng.choice([2, 17, 64]))
        else:
            n_cols = int(rng.choice([1, 5, 33, 157, 900, 2100]))
            while len(rows) == 0 or (rng.rand() < 0.8 and len(rows) < 3000):
                kind = int(rng.randint(0, 5))
                if kind == 0:                                           # loose rows
                    rows += [rng.randint(0, n_cols, rng.randint(0, 41)).astype(np.int32) for _ in range(rng.randint(1, 80))]
                elif kind in (1, 2):                                    # a pattern group (kind 2: some members lost a few entries)
                    pattern = rng.randint(0, n_cols, rng.randint(0, 121)).astype(np.int32)
                    for _ in range(int(rng.choice([2, 3, 7, 8, 15, 16, 17, 31, 32, 33, 64, 100, 257, 600]))):
                        if kind == 2 and len(pattern) > 3 and rng.rand() < 0.1:
                            rows.append(np.delete(pattern, rng.choice(len(pattern), size=rng.randint(1, 4), replace=False)))
                        else:
                            rows.append(pattern)
                elif kind == 3:                                         # one long row with duplicates
                    rows.append(rng.randint(0, n_cols, rng.randint(500, 4000)).astype(np.int32))
                else:                                                   # empty rows
                    rows += [np.zeros(0, np.int32)] * int(rng.randint(1, 5))
        if rng.rand() < 0.5:
            rows = [rows[i] for i in rng.permutation(len(rows))]        # groups scattered over the operator
        indptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int32)
        indices = np.concatenate(rows).astype(np.int32) if indptr[-1] else np.zeros(0, np.int32)
        f64 = bool(rng.rand() < 0.125)
        data = rng.randn(len(indices)) * np.exp(rng.uniform(-20, 20, len(indices))) if f64 else rng.randn(len(indices)).astype(np.float32)
        if len(data) and rng.rand() < 0.3:
            data[rng.randint(0, len(data), size=min(len(data), 5))] = 0.0          # explicit zeros are stored entries
        n = int(rng.choice(WIDTHS))
        narrow = [ROWS, LINEAR, ROWS | LINEAR][int(rng.randint(3))]
        if linear and rng.rand() < 0.7:
            narrow |= LINEAR
        conv_bits = 0
        if rng.rand() < 0.5:
            for bit in (NARROW, MFMA, N32, N64, N64M, TAPS, TAPS32, FILL):
                if rng.rand() < 0.5:
                    conv_bits |= bit
        relu = bool(rng.rand() < 0.5)
        (ld, start) = _window(rng, n)
        X = rng.randn(n_cols, n).astype(np.float32)
        nonfinite = _nonfinite(rng, n_cols, n)
        for (r, c, v) in nonfinite:
            X[r, c] = v
        screen = bool(rng.rand() < 0.25)
        lens = np.diff(indptr)
        yield dict(case=case, kind='linear' if linear else 'rows', shape=(len(rows), n_cols), indptr=indptr, indices=indices, data=data, f64=f64, big=big, n=n,
                   flags=int(EXACT | (RELU if relu else 0) | narrow | conv_bits), base=int(EXACT | (RELU if relu else 0)), narrow=int(narrow), relu=relu, ld=ld, start=start, X=X,
                   nonfinite=nonfinite, screen=screen, skipped=None, props=dict(rows=len(rows), cols=n_cols, nnz=int(indptr[-1]), longest=int(lens.max()), empty_rows=int((lens == 0).sum())))


def csr_classes(d):
    c = set()
    if d['big']:
        c.add('big-group CSR')
    if d['f64']:
        c.add('float64')
    return c


def csr_matrix_of(d):
    return scipy.sparse.csr_matrix((d['data'], d['indices'], d['indptr']), shape=d['shape'])


# ------------------------------------------------------------------------------------------------------------------ key-nets
BATCHES = [1, 2, 3, 5, 8, 9, 16, 17, 32, 33, 48, 64]


def narrow_keywords(rng, n, mfma=None):
    """A random VALID narrow keyword set for a batch of n images, built from the README's rule (never filtered through _narrow_args): `narrow` True | 'mfma' always; 9 .. 32 images
    need narrow32=True or narrow64; 33 .. 64 images narrow64=True next to narrow=True, or narrow64='mfma' next to narrow='mfma' (which the keyword needs at every
    width); narrow_rows only at 8 images and fewer; narrow_linear, narrow_taps (True | 'packed') and narrow_fill at every width, next to `narrow`.
    `mfma`: True / False force narrow='mfma' / narrow=True."""
    mode = 'mfma' if (mfma if mfma is not None else rng.rand() < 0.3) else True
    kw = dict(narrow=mode)
    wide64 = [True, 'mfma'] if mode == 'mfma' else [True]
    if n > 32:
        kw['narrow64'] = 'mfma' if mode == 'mfma' else True
    elif n > 8:
        if rng.rand() < 0.6:
            kw['narrow32'] = True
            if rng.rand() < 0.3:
                kw['narrow64'] = wide64[int(rng.randint(len(wide64)))]
        else:
            kw['narrow64'] = wide64[int(rng.randint(len(wide64)))]
    else:
        if rng.rand() < 0.3:
            kw['narrow32'] = True
        if rng.rand() < 0.2:
            kw['narrow64'] = wide64[int(rng.randint(len(wide64)))]
    if n <= 8 and rng.rand() < 0.5:
        kw['narrow_rows'] = True
    if rng.rand() < 0.5:
        kw['narrow_linear'] = True
    t = rng.rand()
    if t < 0.35:
        kw['narrow_taps'] = True
    elif t < 0.7:
        kw['narrow_taps'] = 'packed'
    if rng.rand() < 0.3:
        kw['narrow_fill'] = True
    return kw


INVALID_KEYWORDS = [
    (9, dict(narrow32=True)),                                           # narrow32 without narrow
    (9, dict(narrow=True, narrow32=True, narrow_rows=True)),            # narrow_rows at 9
    (40, dict(narrow='mfma', narrow64=True)),
    (4, dict(narrow=True, narrow_split=True)),
    (9, dict(narrow=True, narrow_taps='packed')),                       # 9 images without narrow32 / narrow64: refused whatever narrow_taps is -- 'packed' lifts no limit
]


def _wide_linear_net(rng):
    """A random_net with at least 2 048 input features in front of two or more Linear layers, its first Linear widened to 256 .. 300 outputs: the keyed Linear
    the stream kernel is for (a big pattern group; random_net itself draws at most 149 outputs).  None where twenty draws give no such network."""
    for _ in range(20):
        (net, inshape, names) = random_net(rng, sides=(16, 20))
        if 'fc2' in names and net.fc1.in_features >= 2048:
            out = int(rng.randint(256, 301))
            (fc1, fc2) = (net.fc1, net.fc2)
            net.fc1 = nn.Linear(fc1.in_features, out)
            net.fc2 = nn.Linear(out, fc2.out_features)
            return (net, inshape, names)
    return None


def model_cases(n_cases, seed):
    """Yields one dict per case: a random source network (random_net; one permutation case in four with a wide first Linear, _wide_linear_net), the key family -- 'tiled'
    permutation keys with tile 2 | 3 | 4 | 8, 'untiled' permutation keys, about one case in four 'orthogonal' float keys --, the batch, a valid keyword set, and the two
    seeds the fuzzer keys and draws images with."""
    rng = np.random.RandomState(seed)
    for case in range(n_cases):
        torch_seed = int(rng.randint(1 << 30))
        numpy_seed = int(rng.randint(1 << 30))
        torch.manual_seed(torch_seed)
        float_keys = bool(rng.rand() < 0.25)
        wide = _wide_linear_net(rng) if (not float_keys and rng.rand() < 0.25) else None
        (net, inshape, names) = wide if wide is not None else (random_net(rng, sides=(8, 16)) if float_keys else random_net(rng))
        widened = wide is not None
        tile = 4 if float_keys else int(rng.choice([0, 2, 3, 4, 8]))
        n = int(rng.choice(BATCHES))
        kw = narrow_keywords(rng, n, mfma=True if float_keys else None)
        if widened:
            kw['narrow_linear'] = True                                  # (the layer the network was widened for)
        yield dict(case=case, net=net, inshape=inshape, names=names, family='orthogonal' if float_keys else ('untiled' if tile == 0 else 'tiled'), float_keys=float_keys, tile=tile, n=n,
                   keywords=kw, torch_seed=torch_seed, numpy_seed=numpy_seed, widened=widened, skipped=None)
