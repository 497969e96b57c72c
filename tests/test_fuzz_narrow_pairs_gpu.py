"""Seeded fuzzer of the channel-pair tap-resident kernel (KN_FLAG_NARROW_TAPS | KN_MODIFIER_NARROW_TAPS_PAIRS under KN_FLAG_NARROW) against the oracle, bit for bit
under value_classes.bits_equal.

The cases are tests/fuzz_narrow_cases.conv_cases' (imported, not edited): operator class, column window, non-finite activations and the EXACT / RELU bits as that
generator draws them.  Two things are this file's own: the width is brought to 1 .. 8 columns (a wider case takes W8[n mod 7]), and two cases in three of the
classes the tap-resident kernels take (canonical, coef) are built again by the same builders with 65 .. 200 output channels -- the generator's own Cout list
(1, 5, 24, 40, 64, 72, 128, 192) meets the kernel's 128-channel blocks at three sizes only.  Everything of a case comes from a stream seeded by (seed, case).
The host part (no GPU) checks that the fixed seed reaches the new kernel's rule -- eligible operator, more than 64 output channels -- in at least a quarter of the
cases; the GPU part asserts the same share from the plans."""
import numpy as np
import pytest
import torch

import fuzz_narrow_cases as fc
import value_classes as vc
from keynet_amd import _capi
from narrow_helpers import _spmm, SENTINEL

(RELU, EXACT, NARROW, TAPS) = (_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_NARROW, _capi.KN_FLAG_NARROW_TAPS)
PAIRS = getattr(_capi, 'KN_MODIFIER_NARROW_TAPS_PAIRS', 0x2000)
NEW = 'convtaps_narrow_taps_pairs_kernel'
(SEED, CASES) = (1818, 48)
SHARE = 0.25


def pairs_cases(n_cases=CASES, seed=SEED):
    """conv_cases' cases at 1 .. 8 columns with the flag word EXACT? | RELU? | NARROW | TAPS | PAIRS; the 'wide' class (8 281 pixels: seconds of oracle per case) is
    left out, two canonical / coef cases in three are rebuilt with 65 .. 200 output channels."""
    for d in fc.conv_cases(n_cases, seed):
        if d['skipped'] or d['cls'] == 'wide':
            continue
        rng = np.random.RandomState((seed * 7919 + d['case']) % (1 << 32))
        if d['n'] > 8:
            d['n'] = fc.W8[d['n'] % len(fc.W8)]
            (d['ld'], d['start']) = fc._window(rng, d['n'])
            d['nonfinite'] = []
            d['X'] = np.where(np.isfinite(d['X']), d['X'], np.float32(0.5)).astype(np.float32)
        if d['cls'] in ('canonical', 'coef') and d['case'] % 3 != 0:
            (Cin, H, stride) = (int(rng.choice([1, 2, 3, 5, 8, 17])), int(rng.randint(3, 10)), int(rng.choice([1, 2])))
            (Cout, has_last) = (int(rng.randint(65, 201)), bool(rng.rand() < 0.6))
            if d['cls'] == 'canonical':
                W = fc._random_convtaps(rng, Cin, Cout, H, 3, stride, True, has_last)
            else:
                many = bool(rng.rand() < 0.5)
                W = fc._coef_convtaps(rng, Cin, Cout, max(H, 4 * stride) if many else H, 3, stride, has_last, ntaps=int(rng.randint(10, 17)) if many else None)
            X = rng.randn(W.shape[1], 128).astype(np.float32)
            if rng.rand() < 0.3:
                X[int(rng.randint(W.shape[1] - 1 if has_last else W.shape[1])), int(rng.randint(d['n']))] = fc.NONFINITE[int(rng.randint(3))]
            if has_last:
                X[-1] = 1.0
            d.update(W=W, M=None, X=X, props=fc.conv_props(W), nonfinite=[])
        d['flags'] = int((d['flags'] & (EXACT | RELU)) | NARROW | TAPS | PAIRS)
        yield d


def reaches(p):
    """The host-visible part of the new kernel's rule (kn_internal.h: narrow_taps_ok, Cout > 64)."""
    return bool(p['taps_ok'] and p['Cout'] > 64)


def test_the_seed_reaches_the_new_kernel_in_a_quarter_of_the_cases():
    cases = list(pairs_cases())
    hit = [d for d in cases if reaches(d['props'])]
    assert len(cases) >= 30 and len(hit) >= SHARE * len(cases), (len(hit), len(cases))
    assert all(1 <= d['n'] <= 8 for d in cases) and len(set(d['n'] for d in hit)) >= 5
    assert any(d['props']['Cout'] % 128 not in (0, 64) and d['props']['Cout'] > 128 for d in hit)           # two blocks, the second partly filled
    assert any(d['props']['coef'] for d in hit) and any(d['props']['ntaps'] > 9 for d in hit) and any(not reaches(d['props']) for d in cases)
    assert [fc.describe(d) for d in pairs_cases(6)] == [fc.describe(d) for d in pairs_cases(6)]          # deterministic


@pytest.mark.gpu
def test_fuzz_pairs_against_the_oracle():
    from test_parity_gpu import dev
    (ran, new) = (0, 0)
    for d in pairs_cases():
        (W, X, n, flags, ld, start) = (d['W'], d['X'], d['n'], d['flags'], d['ld'], d['start'])
        Xw = np.full((X.shape[0], ld), np.nan, dtype=np.float32)       # the batch as a window of a block that is NaN everywhere else
        Xw[:, start:start + n] = X[:, :n]
        xw = torch.as_tensor(Xw).to(dev())
        with torch.cuda.device(dev()):
            op = W._device_op(dev())
        (win, whole, plan) = _spmm(op, xw, n, flags, ld=ld, start=start)
        what = (d['case'], d['cls'], n, hex(flags), ld, start, d['props']['Cout'], plan[:160])
        assert (NEW in plan) == reaches(d['props']), what
        ref = fc.oracle_product(fc.conv_reference(d), np.ascontiguousarray(X[:, :n]), relu=bool(flags & RELU))
        vc.assert_bits_equal(win.cpu().numpy(), ref, str(what))
        outside = torch.ones(ld, dtype=torch.bool, device=whole.device)
        outside[start:start + n] = False
        assert bool(torch.all(whole[:, outside] == SENTINEL)), what
        (w0, _, p0) = _spmm(op, xw, n, flags & ~PAIRS, ld=ld, start=start)
        assert torch.equal(win.view(torch.int32), w0.view(torch.int32)) and NEW not in p0, what
        ran += 1
        new += NEW in plan
    assert ran >= 30 and new >= SHARE * ran, (new, ran)
