"""The host side of the narrow-kernel fuzzers (CPU, no GPU): the case generators of tests/fuzz_narrow_cases.py are deterministic, reach every host-visible operator
class at the tier's seeds and budgets (the part of the fuzzers' reach condition that needs no device), the judge itself -- the oracle on a case's CSR -- sits inside the
f32 summation bound of the float64 product, and the constructive keyword generator emits only sets NarrowForm.of accepts."""
import numpy as np
import pytest
import scipy.sparse

import keynet_amd.sparse as ksp
import exact_sum
import fuzz_narrow_cases as fc

# the tier of tests/test_fuzz_narrow_gpu.py (that module needs no device to import, but it is the GPU tier's: the numbers are restated and compared there)
(CONV_SEED, CONV_CASES) = (20261, 240)
(CSR_SEED, CSR_CASES) = (5151, 300)
(MODEL_SEED, MODEL_CASES) = (8088, 56)
CONV_CLASSES = ['slots<=9,taps<=16', 'coefficients', 'taps 10..16', 'summed values', 'filled, taps <= 16', 'filled, taps > 16', '>2 slots on a (pixel, tap) pair', '>= 4096 work items',
                'empty pixels', 'Cout % 64 != 0']
CSR_CLASSES = ['big-group CSR', 'float64']
_tier = {}


def _conv_tier():
    """The conv cases of the tier, generated once: (descriptions, class counts, skipped, the worst ratio of the oracle's distance from the float64 product to its bound)."""
    if 'conv' not in _tier:
        (lines, counts, skipped, worst) = ([], dict.fromkeys(CONV_CLASSES, 0), 0, 0.0)
        (aims, twins) = ({}, [])
        for d in fc.conv_cases(CONV_CASES, CONV_SEED):
            lines.append(fc.describe(d))
            if d['skipped']:
                skipped += 1
                continue
            for c in fc.conv_classes(d['props']):
                counts[c] += 1
            aims[(d['cls'], d['aim'])] = aims.get((d['cls'], d['aim']), 0) + 1
            if not d['nonfinite']:
                ratio = _judge_ratio(fc.conv_reference(d), d['X'][:, :d['n']])
                worst = max(worst, ratio)
            if d['twin']:
                t = fc._taps_of(d['W'])
                integer = all(np.array_equal(a, np.rint(a)) for a in (t['taps'], d['X']) + tuple(a for a in (t['ent_coef'], t['lastcol']) if a is not None))
                twins.append(dict(case=d['case'], cls=d['cls'], ratio=ratio, integer=integer, nonfinite=d['nonfinite'], sums=exact_sum.condition_factored(d['W'], d['X'][:, :d['n']]),
                                  matrix_core=bool(d['flags'] & fc.MFMA and not d['flags'] & fc.EXACT and ((d['props']['mfma_ok'] and d['n'] <= 32) or (d['n'] > 32 and d['flags'] & fc.N64M)))))
        _tier['conv'] = (lines, counts, skipped, worst, aims)
        _tier['twins'] = twins
    return _tier['conv']


def _csr_tier():
    if 'csr' not in _tier:
        (lines, counts, worst) = ([], dict.fromkeys(CSR_CLASSES, 0), 0.0)
        for d in fc.csr_cases(CSR_CASES, CSR_SEED):
            lines.append(fc.describe(d))
            for c in fc.csr_classes(d):
                counts[c] += 1
            if not d['nonfinite']:
                worst = max(worst, _judge_ratio(fc.csr_matrix_of(d), d['X']))
        _tier['csr'] = (lines, counts, worst)
    return _tier['csr']


def _judge_ratio(M, X):
    """max over the elements of |oracle - float64 product| / (gamma sum |w| |x|), gamma = (row length + 1) 2^-24: the standard bound of a recursive float32 sum of
    rounded products (a float64 operator's oracle sums in float64 and sits far inside it)."""
    ref = fc.oracle_product(M, X).astype(np.float64)
    exact = M.astype(np.float64).dot(X.astype(np.float64))
    A = scipy.sparse.csr_matrix((np.abs(M.data.astype(np.float64)), M.indices, M.indptr), shape=M.shape)      # (|w| entry by entry: abs() of a matrix sums duplicate entries first)
    S = A.dot(np.abs(X.astype(np.float64)))
    gamma = (np.diff(M.indptr) + 1.0)[:, None] * 2.0 ** -24
    with np.errstate(all='ignore'):
        ratio = np.abs(ref - exact) / (gamma * S)
    ratio[(S == 0) & (ref == exact)] = 0.0
    return float(ratio.max()) if ratio.size else 0.0


def test_the_tier_is_the_gpu_tiers():
    import test_fuzz_narrow_gpu as g
    assert ((g.CONV_SEED, g.CONV_CASES), (g.CSR_SEED, g.CSR_CASES), (g.MODEL_SEED, g.MODEL_CASES)) == ((CONV_SEED, CONV_CASES), (CSR_SEED, CSR_CASES), (MODEL_SEED, MODEL_CASES))


def test_generators_are_deterministic():
    """The same seed gives the same case descriptions (class, shapes, width, flags, window, non-finite positions, a checksum of the values); another seed does not."""
    k = 40
    assert [fc.describe(d) for d in fc.conv_cases(k, CONV_SEED)] == _conv_tier()[0][:k]
    assert [fc.describe(d) for d in fc.csr_cases(k, CSR_SEED)] == _csr_tier()[0][:k]
    assert [fc.describe(d) for d in fc.conv_cases(5, CONV_SEED + 1)] != _conv_tier()[0][:5]
    (a, b) = ([fc.describe(d) for d in fc.model_cases(MODEL_CASES, MODEL_SEED)], [fc.describe(d) for d in fc.model_cases(MODEL_CASES, MODEL_SEED)])
    assert a == b and len(set(a)) == MODEL_CASES


def test_conv_cases_reach_every_host_visible_class():
    (_, counts, skipped, _, aims) = _conv_tier()
    print(counts, 'skipped', skipped, sorted(aims.items()))
    assert all(v >= 5 for v in counts.values()), counts
    assert skipped <= 0.1 * CONV_CASES, skipped
    for (cls, forms) in fc.CONV_AIMS.items():                          # every aim of every class is drawn at least 3 times: what the GPU tier's reach condition stands on
        for f in forms:
            assert aims.get((cls, f[0]), 0) >= 3, (cls, f[0], sorted(aims.items()))


def test_exact_sum_twins_of_the_conv_tier():
    """About one conv case in four is an exact-sum twin: integer operands, no non-finite activation, sum |a| |x| over the terms <= 2^24 (exact_sum.condition_factored
    asserts it), so the oracle's float32 product IS the float64 product; and enough of them carry KN_FLAG_NARROW_MFMA on an operator the matrix-core narrow kernel takes (or, beyond 32 columns, the bit of the 64-column tile)
    that the GPU tier's reach condition (one twin on a matrix-core plan) does not hang on one draw."""
    _conv_tier()
    twins = _tier['twins']
    print(len(twins), 'twins;', sum(t['matrix_core'] for t in twins), 'aimed at the matrix-core narrow kernel; largest sum %.0f' % max(t['sums'] for t in twins))
    assert CONV_CASES // 8 <= len(twins) <= 3 * CONV_CASES // 8, len(twins)
    assert all(t['integer'] and not t['nonfinite'] and t['ratio'] == 0.0 and t['sums'] <= exact_sum.LIMIT and t['cls'] != 'dropped' for t in twins), [t for t in twins if t['ratio'] != 0.0][:3]
    assert sum(t['matrix_core'] for t in twins) >= 3


def test_csr_cases_reach_every_host_visible_class():
    (_, counts, _) = _csr_tier()
    print(counts)
    assert all(v >= 5 for v in counts.values()), counts                # (no CSR case is skipped: the sizes are the oracle's by construction)


def test_the_judge_is_inside_the_summation_bound():
    """On every finite case the oracle's product is within gamma sum |w| |x| of the float64 product of the same CSR: this guards the judge, not the kernels."""
    (conv, csr) = (_conv_tier()[3], _csr_tier()[2])
    print('worst |oracle - float64| / bound: conv %.3g, csr %.3g' % (conv, csr))
    assert conv <= 1.0 and csr <= 1.0, (conv, csr)


def test_the_host_visible_facts_of_known_operators():
    """conv_props on operators whose facts are known by construction."""
    rng = np.random.RandomState(3)
    p = fc.conv_props(fc._random_convtaps(rng, 3, 24, 7, 3, 1, True, True))
    assert (p['ntaps'], p['max_slots'], p['summed'], p['coef'], p['max_pair_tap'], p['taps_ok'], p['fill_ok'], p['mfma_ok'], p['empty_pixels']) == (9, 9, False, False, 1, True, False, True, False)
    p = fc.conv_props(fc._random_convtaps(rng, 3, 64, 8, 3, 1, False, False))
    assert p['summed'] and p['coef'] and p['max_slots'] > 9 and not p['taps_ok'] and p['fill_ok'] and p['max_pair_tap'] == 2 and p['mfma_ok']
    p = fc.conv_props(fc._coef_convtaps(rng, 5, 72, 6, 3, 1, True, ntaps=13))
    assert p['ntaps'] == 13 and p['coef'] and p['taps_ok'] and not p['fill_ok'] and 'taps 10..16' in fc.conv_classes(p)
    for eligible in (True, False):
        for _ in range(20):
            p = fc.conv_props(fc._filled(rng, eligible, True))
            assert p['fill_ok'] == eligible or (not eligible and p['ntaps'] <= 16 and p['max_pair_tap'] > 2), p
            assert eligible or p['ntaps'] > 16 or not p['mfma_ok'], p
    p = fc.conv_props(fc._without_pixels(rng, fc._random_convtaps(rng, 2, 5, 6, 3, 1, True, True)))
    assert p['empty_pixels'] and 'Cout % 64 != 0' in fc.conv_classes(p)


def test_every_generated_keyword_set_is_valid_and_the_invalid_ones_still_raise():
    rng = np.random.RandomState(77)
    seen = set()
    for n in fc.BATCHES * 40:
        for mfma in (None, True, False):
            kw = fc.narrow_keywords(rng, n, mfma=mfma)
            form = ksp.NarrowForm.of(n, **kw)                          # ValueError: the generator emitted a set the argument rule refuses
            assert form.mode == kw['narrow'] and bool(form.taps) == bool(kw.get('narrow_taps')) and form.fill == bool(kw.get('narrow_fill'))
            seen.update(kw.items())
    assert seen >= {('narrow', True), ('narrow', 'mfma'), ('narrow_rows', True), ('narrow32', True), ('narrow64', True), ('narrow64', 'mfma'), ('narrow_linear', True),
                    ('narrow_taps', True), ('narrow_taps', 'packed'), ('narrow_fill', True)}, seen
    for d in fc.model_cases(MODEL_CASES, MODEL_SEED):
        ksp.NarrowForm.of(d['n'], **d['keywords'])
    for (n, kw) in fc.INVALID_KEYWORDS:
        with pytest.raises(ValueError):
            ksp.NarrowForm.of(n, **kw)
