"""Seeded fuzzers of the narrow kernels (1 .. 64 batch columns) against the CPU oracle, as collected `-m gpu` tests with a case budget: the conv-taps handle under
every narrow regime and modifier through kn_spmm (fuzz_convtaps_narrow), float32 / float64 CSR handles under KN_FLAG_NARROW_ROWS and KN_FLAG_NARROW_LINEAR
(fuzz_csr_narrow), whole key-nets under random valid narrow keyword sets (fuzz_models_narrow).  The cases come from tests/fuzz_narrow_cases.py (host code; its
docstring says how a case is drawn); the judge is oracle.csr_matvecs / oracle.keynet_forward, bit for bit wherever the contract is bit-exact.  Each fuzzer records the
kernel forms its plans name, and the collected tests assert that the run reached every narrow kernel family (CONV_REACH, CSR_REACH, MODEL_REACH).
Larger runs:  python3 tests/test_fuzz_narrow_gpu.py convnarrow 2400 | csrnarrow 3000 | modelsnarrow 560   [seed]"""
import collections
import os
import re
import sys
import tempfile
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle                                    # noqa: E402  (checker)
from value_classes import bits_equal            # noqa: E402  (the uint32 patterns: the sign of a zero and a flushed subnormal count)
from keynet_amd import _capi                     # noqa: E402
import fuzz_narrow_cases as fc                   # noqa: E402
from fuzz_narrow_cases import RELU, EXACT, NARROW, MFMA, ROWS, N32, N64, N64M, LINEAR, TAPS, TAPS32, FILL      # noqa: E402
from narrow_helpers import _spmm, _spmm_calls, SENTINEL      # noqa: E402

pytestmark = pytest.mark.gpu

# the tier: seeds and budgets at which the reach conditions below hold (tests/test_fuzz_narrow_host.py checks the host-visible part of it at the same numbers)
(CONV_SEED, CONV_CASES) = (20261, 240)
(CSR_SEED, CSR_CASES) = (5151, 300)
(MODEL_SEED, MODEL_CASES) = (8088, 56)

(TAPS_KERNEL, TAPS32_KERNEL, FILL_KERNEL, NMFMA_KERNEL, TILE_KERNEL) = ('convtaps_narrow_taps_kernel', 'convtaps_narrow_taps32_kernel', 'convtaps_narrow_fill_kernel',
                                                                       'convtaps_narrow_mfma_kernel', 'convtaps_mfma_kernel')
CONV_REACH = ['convtaps_narrow_kernel', 'convtaps_narrow32_kernel', 'convtaps_exact_pipe64_kernel', NMFMA_KERNEL, TILE_KERNEL + '<NB=64>',
              TAPS_KERNEL + ' P=1', TAPS_KERNEL + ' P=2', TAPS_KERNEL + ' 16 value rows', TAPS_KERNEL + ' coef', TAPS_KERNEL + ' columns 4 ..',
              TAPS32_KERNEL + ' NV=8', TAPS32_KERNEL + ' NV=16', TAPS32_KERNEL + ' NV=32', TAPS32_KERNEL + ' masked',
              FILL_KERNEL + ' <= 8 columns', FILL_KERNEL + ' column blocks']
TWIN_REACH = 'exact-sum twin on a matrix-core plan'
CSR_REACH = ['csr_narrow_kernel', 'csr_stream_group_kernel']
MODEL_REACH = ['tap-resident kernel', 'csr_narrow_kernel', 'csr_stream_group_kernel', 'convtaps_exact_pipe64_kernel', NMFMA_KERNEL]


def conv_forms(plan):
    """The kernel forms a conv plan names, in the words of CONV_REACH (+ the 64-channel tile of the matrix-core narrow kernel, which no condition is set on)."""
    forms = set()
    for seg in plan.split('; '):
        name = seg.split('<')[0].split(' ')[0]
        if name in ('convtaps_narrow_kernel', 'convtaps_narrow32_kernel'):
            forms.add(name)
        if 'convtaps_exact_pipe64_kernel' in seg:
            forms.add('convtaps_exact_pipe64_kernel')
        if name == NMFMA_KERNEL:
            forms.add(name)
            if '<64 channels' in seg:
                forms.add(name + ' TM=2')
        if name == TILE_KERNEL and 'NB=64' in seg:
            forms.add(TILE_KERNEL + '<NB=64>')
        if name == TAPS_KERNEL:
            forms.update(TAPS_KERNEL + ' ' + w for w in ('P=1', 'P=2', '16 value rows', 'columns 4 ..') if w in seg)
            if ', coef' in seg:
                forms.add(TAPS_KERNEL + ' coef')
        if name == TAPS32_KERNEL:
            forms.update(TAPS32_KERNEL + ' ' + w for w in ('NV=8', 'NV=16', 'NV=32', 'masked') if w in seg)
        if name == FILL_KERNEL:
            forms.add(FILL_KERNEL + (' column blocks' if 'column blocks' in seg else ' <= 8 columns'))
    return forms


def _window_block(X, n, ld, start, dev):
    """The case's n columns as columns start .. start + n of a [cols, ld] block that is NaN everywhere else."""
    Xw = np.full((X.shape[0], ld), np.nan, dtype=np.float32)
    Xw[:, start:start + n] = X[:, :n]
    return torch.as_tensor(Xw).to(dev)


def _outside_intact(whole, n, start):
    out = torch.ones(whole.shape[1], dtype=torch.bool, device=whole.device)
    out[start:start + n] = False
    return bool(torch.all(whole[:, out] == SENTINEL))


def _slot_ok(slot, win):
    """The screen slot equals max |Y| of the returned window, NaN ignored."""
    a = torch.nan_to_num(win.abs(), nan=0.0, posinf=float('inf'))
    return float(slot) == (float(a.max()) if a.numel() else 0.0)


def _same_bits(a, b):
    """NaN at the same positions, and everywhere else the same int32 view (which sees the sign of a zero).  The sign and payload of a NaN are no part of any contract
    here: which operand's NaN an addition hands on depends on the operand order the compiler chose (csr_narrow_kernel and csr_group_kernel give 0xffc00000 and
    0x7fc00000 for the same row of inf - inf and w * nan terms), and scipy on the CPU has a third convention."""
    (na, nb) = (torch.isnan(a), torch.isnan(b))
    return bool(torch.equal(na, nb)) and bool(torch.equal(a.contiguous().view(torch.int32)[~na], b.contiguous().view(torch.int32)[~na]))


def fuzz_convtaps_narrow(n_cases, seed=CONV_SEED, verbose=False, only=None):
    """Conv-taps handles of seven operator classes (fuzz_narrow_cases.conv_cases) through kn_spmm at 1 .. 64 columns under KN_FLAG_NARROW / KN_FLAG_NARROW_MFMA with the
    regime bits the width needs and random EXACT, RELU, NARROW_TAPS, NARROW_TAPS32, NARROW_FILL, on compact blocks and column windows (X NaN outside, Y a sentinel),
    with non-finite activations and with the screen slot.  A call whose plan names no matrix-core kernel: the window equals the oracle on the operator's sorted
    canonical CSR bit for bit, NaN positions included, and its int32 view equals that of the first columns of the KN_FLAG_EXACT product at 128 columns where that is
    no NaN (the sign of zero).  A matrix-core call (finite X): inside fuzz_convtaps' bound element-wise, the same bits twice, per image the bits of the call on
    that image's chunk of at most 8 columns (9 .. 32 columns), the bits of the plain matrix-core call on the batch zero-padded to 128 columns (the 64-column tile);
    on an exact-sum twin (about one case in four, fuzz_narrow_cases.exact_sum_twin) the oracle's bits in place of the bound.
    Every call: the sentinel outside the window, the slot == max |Y|.  A modifier that the operator's host-visible class or the width rules out, NARROW_ROWS |
    NARROW_LINEAR, and KN_FLAG_NARROW32 alone: the plan and the bits of the call without it.  Returns dict(cases, checked, skipped, bad); .reach counts the forms."""
    dev = torch.device('cuda:0')
    counts = dict(cases=n_cases, checked=0, skipped=0, bad=0)
    reach = fuzz_convtaps_narrow.reach = collections.Counter()

    def bad(d, what, plan=''):
        counts['bad'] += 1
        print('case', d['case'], 'MISMATCH:', what, '|', d['cls'], d['aim'], 'n', d['n'], 'flags', hex(d['flags']), 'ld', d['ld'], 'start', d['start'], 'nonfinite', d['nonfinite'],
              {k: d['props'][k] for k in ('Cin', 'Cout', 'pixels', 'ntaps', 'max_slots', 'summed', 'coef', 'max_pair_tap', 'bias')}, '|', plan[:200], flush=True)

    for d in fc.conv_cases(n_cases, seed, only=only):
        if d['skipped']:
            counts['skipped'] += 1
            continue
        (W, X, n, flags, ld, start, p) = (d['W'], d['X'], d['n'], d['flags'], d['ld'], d['start'], d['props'])
        relu = RELU if flags & RELU else 0
        finite = not d['nonfinite']
        with torch.cuda.device(dev):
            op = W._device_op(dev)
        xw = _window_block(X, n, ld, start, dev)
        slot = torch.zeros(1, dtype=torch.float32, device=dev) if d['screen'] else None
        (win, whole, plan) = _spmm(op, xw, n, flags, ld=ld, start=start, absmax=slot)
        forms = conv_forms(plan)
        reach.update(forms)
        if verbose:
            print('case', d['case'], d['cls'], d['aim'], 'Cin', p['Cin'], 'Cout', p['Cout'], 'pixels', p['pixels'], 'taps', p['ntaps'], 'slots', p['slots'], 'n', n, 'flags', hex(flags),
                  'ld', ld, 'start', start, 'nonfinite', len(d['nonfinite']), 'screen', d['screen'], '|', plan[:150], flush=True)
        counts['checked'] += 1
        matrix_core = NMFMA_KERNEL in plan or TILE_KERNEL in plan
        if not _outside_intact(whole, n, start):
            bad(d, 'wrote outside the window', plan)
        if slot is not None and not _slot_ok(slot, win):
            bad(d, 'screen slot %r != max |Y| %r' % (float(slot), float(torch.nan_to_num(win.abs(), nan=0.0).max())), plan)
        if not matrix_core or finite:
            ref = fc.oracle_product(fc.conv_reference(d), X[:, :n], relu=bool(relu))
            got = win.cpu().numpy()
        if not matrix_core:
            if not bits_equal(got, ref):
                bad(d, 'differs from the oracle, max %r' % float(np.nanmax(np.abs(got - ref))), plan)
            y128 = _spmm(op, torch.as_tensor(X).to(dev), 128, EXACT | relu)[0][:, :n]
            keep = ~torch.isnan(y128)
            if not bool(torch.equal(win.contiguous().view(torch.int32)[keep], y128.contiguous().view(torch.int32)[keep])):
                bad(d, 'int32 view differs from the 128-column KN_FLAG_EXACT product', plan)
        elif finite:
            if d['twin']:                                               # an exact-sum twin: every order of the sum gives the oracle's bits
                reach[TWIN_REACH] += 1
                if not bits_equal(got, ref):
                    bad(d, 'matrix-core call on an exact-sum twin differs from the oracle, max %r' % float(np.abs(got - ref).max()), plan)
            elif not np.all(np.abs(got.astype(np.float64) - ref) <= 1e-5 * np.maximum(1.0, np.abs(ref)) + 8 * 2.0 ** -24 * fc.conv_abs_sum(d)):      # (fuzz_convtaps' bound of the matrix-core path)
                bad(d, 'matrix-core call off by %r' % float(np.abs(got - ref).max()), plan)
            if not _same_bits(_spmm(op, xw, n, flags, ld=ld, start=start)[0], win):
                bad(d, 'matrix-core call not deterministic', plan)
            xc = torch.as_tensor(np.ascontiguousarray(X[:, :n])).to(dev)
            if NMFMA_KERNEL in plan and n > 8:                          # per image the bits of the flag on that image's chunk of at most 8 columns (tests/test_narrow32_gpu.py)
                for lo in range(0, n, 8):
                    (yc, _, pc) = _spmm(op, xc[:, lo:min(lo + 8, n)].contiguous(), min(lo + 8, n) - lo, MFMA | relu)
                    if NMFMA_KERNEL in pc and not _same_bits(yc, win[:, lo:min(lo + 8, n)]):
                        bad(d, 'columns %d .. differ from the matrix-core call on them alone' % lo, plan)
            if TILE_KERNEL in plan and 'NB=64' in plan:                 # the K order of the plain matrix-core call on the batch zero-padded to 128 columns (tests/test_narrow64_mfma_gpu.py)
                xp = torch.zeros((xc.shape[0], 128), dtype=torch.float32, device=dev)
                xp[:, :n] = xc
                (yp, _, pp) = _spmm(op, xp, 128, relu)
                if TILE_KERNEL in pp and 'smallk' not in pp and not _same_bits(yp[:, :n], win):
                    bad(d, '64-column tile differs from the padded matrix-core call', plan + ' || ' + pp)
        # modifiers that must change nothing, decided from the operator's host-visible class and the width
        drop = flags & (ROWS | LINEAR)
        if flags & TAPS and (not p['taps_ok'] or n > 32 or (n > 8 and not flags & TAPS32)):
            drop |= TAPS
        if flags & TAPS32 and (not p['taps_ok'] or n <= 8 or n > 32 or not flags & TAPS):
            drop |= TAPS32
        if flags & FILL and (not p['fill_ok'] or n > 32):
            drop |= FILL
        if flags & MFMA and not flags & EXACT and n <= 32 and p['mfma_ok'] and not (p['Cin'] <= 4 and n > 4 and p['items'] >= 4096):
            drop |= flags & (TAPS | TAPS32 | FILL)                      # the matrix-core narrow kernel takes the call (narrow_mfma_call, kn_internal.h): the modifiers of the channel-lane forms are not read
        if drop:
            (w0, whole0, plan0) = _spmm(op, xw, n, flags & ~drop, ld=ld, start=start)
            if plan0 != plan or not _same_bits(whole0, whole):
                bad(d, 'ignored bits %s changed the call' % hex(drop), plan + ' || ' + plan0)
        (wa, wha, pa) = _spmm(op, xw, n, EXACT | relu | N32, ld=ld, start=start)      # KN_FLAG_NARROW32 alone
        (wb, whb, pb) = _spmm(op, xw, n, EXACT | relu, ld=ld, start=start)
        if pa != pb or not _same_bits(wha, whb):
            bad(d, 'KN_FLAG_NARROW32 alone changed the call', pa + ' || ' + pb)
        W._op = None                                                    # (the handle goes with the case)
    return counts


def fuzz_csr_narrow(n_cases, seed=CSR_SEED, verbose=False, only=None):
    """CSR handles (fuzz_narrow_cases.csr_cases: fuzz_csr's row kinds, keyed-Linear-like big groups, one case in eight float64) through kn_spmm at 1 .. 64 columns
    under KN_FLAG_NARROW_ROWS, KN_FLAG_NARROW_LINEAR or both, alone and next to conv regime bits, on compact blocks and column windows, with non-finite activations and
    the screen slot: the window bit-equal to the oracle (NaN positions included; a float64 operator: to the float64 oracle rounded once, and kn_spmm_f64 to the
    float64 oracle itself) and to the call without the narrow flags, the sentinel intact outside, the slot == max |Y| (float64 handles included); where a flag must change nothing (KN_FLAG_NARROW_ROWS beyond 8
    columns, KN_FLAG_NARROW_LINEAR beyond 32 or without a big group, both on float64, the conv bits everywhere) the plan of the call without it.
    Returns dict(cases, checked, skipped, bad); .reach counts the kernels the plans name."""
    dev = torch.device('cuda:0')
    counts = dict(cases=n_cases, checked=0, skipped=0, bad=0)
    reach = fuzz_csr_narrow.reach = collections.Counter()

    def bad(d, what, plan=''):
        counts['bad'] += 1
        print('case', d['case'], 'MISMATCH:', what, '|', d['kind'], d['shape'], 'f64' if d['f64'] else 'f32', 'big' if d['big'] else '', 'n', d['n'], 'flags', hex(d['flags']), 'ld', d['ld'],
              'start', d['start'], 'nonfinite', d['nonfinite'], d['props'], '|', plan[:200], flush=True)

    for d in fc.csr_cases(n_cases, seed):
        if only is not None and d['case'] != only:
            continue
        (X, n, flags, base, ld, start) = (d['X'], d['n'], d['flags'], d['base'], d['ld'], d['start'])
        with torch.cuda.device(dev):
            op = _capi.Operator.csr(d['shape'], d['indptr'], d['indices'], d['data'])
        xw = _window_block(X, n, ld, start, dev)
        slot = torch.zeros(1, dtype=torch.float32, device=dev) if d['screen'] else None      # (float64 handles too: kn_spmm_screen reduces the f32 block it wrote)
        (win, whole, plan) = _spmm(op, xw, n, flags, ld=ld, start=start, absmax=slot)
        reach.update(set(re.findall(r'(csr_\w+_kernel)', plan)))
        if verbose:
            print('case', d['case'], d['kind'], d['shape'], 'nnz', d['props']['nnz'], 'f64' if d['f64'] else '', 'big' if d['big'] else '', 'n', n, 'flags', hex(flags), 'ld', ld, 'start', start,
                  'nonfinite', len(d['nonfinite']), '|', plan[:150], flush=True)
        counts['checked'] += 1
        with np.errstate(all='ignore'):
            ref = oracle.csr_matvecs(d['shape'], d['indptr'], d['indices'], d['data'], X)
            if d['relu']:
                ref = np.where(ref < 0, ref.dtype.type(0), ref)
            ref32 = ref.astype(np.float32)
        got = win.cpu().numpy()
        if not bits_equal(got, ref32):
            bad(d, 'differs from the oracle, max %r' % float(np.nanmax(np.abs(got - ref32))), plan)
        if not _outside_intact(whole, n, start):
            bad(d, 'wrote outside the window', plan)
        if slot is not None and not _slot_ok(slot, win):
            bad(d, 'screen slot %r != max |Y|' % float(slot), plan)
        (win0, whole0, plan0) = _spmm(op, xw, n, base, ld=ld, start=start)
        if not _same_bits(whole0, whole):
            bad(d, 'differs from the call without the narrow flags', plan + ' || ' + plan0)
        drop = flags & (NARROW | MFMA | N32 | N64 | N64M | TAPS | TAPS32 | FILL)
        if d['f64'] or n > 8:
            drop |= flags & ROWS
        if d['f64'] or n > 32 or not d['big']:
            drop |= flags & LINEAR
        with torch.cuda.device(dev):
            plan_r = op.plan(n, flags & ~drop, ldx=ld, ldy=ld)
        if plan_r != plan:
            bad(d, 'ignored bits %s changed the plan' % hex(drop), plan + ' || ' + plan_r)
        if d['f64']:
            xc = torch.as_tensor(np.ascontiguousarray(X)).to(dev)
            y64 = torch.empty((d['shape'][0], n), dtype=torch.float64, device=dev)
            with torch.cuda.device(dev):
                op.spmm_f64(xc.data_ptr(), n, n, y64.data_ptr(), n, flags, torch.cuda.current_stream().cuda_stream)
            if not bits_equal(y64.cpu().numpy(), ref):
                bad(d, 'kn_spmm_f64 differs from the float64 oracle', plan)
    return counts


def _wide_decisions(knet):
    return [(r['name'], r['exact'], {k: v for (k, v) in (r['calibration'] or {}).items() if k not in ('narrow', 'narrow_split')}) for r in knet.contract_report()['layers']]


def fuzz_models_narrow(n_cases, seed=MODEL_SEED, verbose=False, only=None):
    """Whole key-nets (fuzz_narrow_cases.model_cases: random_net under tiled / untiled permutation keys, a batch of 1 .. 64 distinct images, a random VALID narrow
    keyword set): the logits torch.equal to forward_linear without keywords and equal to oracle.keynet_forward over the exported operators; capture() with the same
    keywords replays to the eager bits on a second batch.  About one case in four under float keys (TiledOrthogonalKeynet, the 'auto' contract), calibrated by one plain
    forward, then narrow='mfma': inside fuzz_float_models' bound against the oracle, a second forward bit-equal, every layer's wide decision unchanged.
    Returns dict(cases, checked, skipped, bad); .reach counts the cases whose recorded kn_spmm calls name a kernel of MODEL_REACH."""
    from keynet_amd import system as ksys, io as kio
    dev = torch.device('cuda:0')
    counts = dict(cases=n_cases, checked=0, skipped=0, bad=0)
    reach = fuzz_models_narrow.reach = collections.Counter()
    for d in fc.model_cases(n_cases, seed):
        if only is not None and d['case'] != only:
            continue
        (net, inshape, n, kw) = (d['net'], d['inshape'], d['n'], d['keywords'])
        if verbose:
            print('case', d['case'], d['family'], 'tile', d['tile'], 'inshape', inshape, 'n', n, d['names'], 'widened' if d['widened'] else '', kw, flush=True)
        np.random.seed(d['numpy_seed'])
        torch.manual_seed(d['torch_seed'] ^ 1)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                if d['family'] == 'orthogonal':
                    (sensor, knet) = ksys.TiledOrthogonalKeynet(inshape, net, 4)
                else:
                    (sensor, knet) = ksys.PermutationKeynet(inshape, net) if d['tile'] == 0 else ksys.TiledPermutationKeynet(inshape, net, d['tile'])
        except (AssertionError, ValueError) as e:                      # a shape this key family does not admit (the reference asserts the same way)
            counts['skipped'] += 1
            if verbose:
                print('   skipped:', type(e).__name__, str(e)[:80])
            continue
        (x, x2) = (torch.randn((n,) + inshape), torch.randn((n,) + inshape))
        xc = sensor.fromtensor(x.to(dev)).encrypt().astensor()
        y0 = knet.forward_linear(xc)                                    # (float keys: calibrates)
        before = _wide_decisions(knet)
        mp = pytest.MonkeyPatch()
        try:
            calls = _spmm_calls(mp)
            y = knet.forward_linear(xc, **kw)
        finally:
            mp.undo()
        plans = ' ; '.join(pl for (pl, _) in calls)
        reach.update(k for k in MODEL_REACH[1:] if k in plans)
        if fc_taps(plans):
            reach['tap-resident kernel'] += 1
        with tempfile.TemporaryDirectory() as tmp:
            kio.save_keynet(knet, os.path.join(tmp, 'k.npz'))
            z = np.load(os.path.join(tmp, 'k.npz'), allow_pickle=False)
            with np.errstate(all='ignore'):
                ref = oracle.keynet_forward(oracle.load_golden_layers(z), xc.cpu().numpy())
        counts['checked'] += 1
        yn = y.cpu().numpy()
        if d['float_keys']:
            scale = max(1.0, float(np.abs(ref).max()))
            e_ref = float(np.abs(yn - ref).max())
            again = knet.forward_linear(xc, **kw)
            ok = e_ref <= 1e-4 * scale and torch.equal(again, y) and _wide_decisions(knet) == before      # (fuzz_float_models' bound)
            if not ok:
                counts['bad'] += 1
                print('case', d['case'], 'MISMATCH (float keys) vs oracle', e_ref, 'scale', scale, 'repeatable', bool(torch.equal(again, y)), 'wide decisions kept', _wide_decisions(knet) == before,
                      inshape, n, d['names'], kw, flush=True)
            continue
        ok_plain = bool(torch.equal(y, y0))
        ok_bits = bits_equal(yn, ref)
        xc2 = sensor.fromtensor(x2.to(dev)).encrypt().astensor()
        replay = knet.capture(xc, **kw)
        r1 = replay(xc).clone()
        r2 = replay(xc2).clone()
        ok_replay = bool(torch.equal(r1, y)) and bool(torch.equal(r2, knet.forward_linear(xc2, **kw))) and bool(torch.equal(r2, knet.forward_linear(xc2)))
        if not (ok_plain and ok_bits and ok_replay):
            counts['bad'] += 1
            print('case', d['case'], 'MISMATCH equal to the forward without keywords', ok_plain, 'equal to the oracle', ok_bits, 'capture replays', ok_replay, d['family'], 'tile', d['tile'],
                  inshape, n, d['names'], kw, 'max vs oracle', float(np.abs(yn - ref).max()), flush=True)
    return counts


def fc_taps(plans):
    return TAPS_KERNEL in plans or TAPS32_KERNEL in plans


def _check(counts, reach, wanted, at_least):
    assert counts['checked'] > 0, counts                                # (zero mismatches after zero checked cases is no result)
    assert counts['bad'] == 0, counts
    assert counts['skipped'] <= 0.1 * counts['cases'], counts
    missed = {k: reach[k] for k in wanted if reach[k] < at_least}
    assert not missed, (missed, dict(reach))


def test_fuzz_narrow_conv_operators():
    counts = fuzz_convtaps_narrow(CONV_CASES)
    _check(counts, fuzz_convtaps_narrow.reach, CONV_REACH, 3)
    assert fuzz_convtaps_narrow.reach[TWIN_REACH] >= 1, dict(fuzz_convtaps_narrow.reach)


def test_fuzz_narrow_csr_operators():
    counts = fuzz_csr_narrow(CSR_CASES)
    _check(counts, fuzz_csr_narrow.reach, CSR_REACH, 3)


def test_fuzz_narrow_keyed_models():
    counts = fuzz_models_narrow(MODEL_CASES)
    _check(counts, fuzz_models_narrow.reach, MODEL_REACH, 1)


if __name__ == '__main__':
    which = sys.argv[1] if len(sys.argv) > 1 else 'convnarrow'
    (fn, tier_seed) = {'convnarrow': (fuzz_convtaps_narrow, CONV_SEED), 'csrnarrow': (fuzz_csr_narrow, CSR_SEED), 'modelsnarrow': (fuzz_models_narrow, MODEL_SEED)}[which]
    cases = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    r = fn(cases, seed=int(sys.argv[3]) if len(sys.argv) > 3 else tier_seed, verbose=True)      # (a third argument: another seed than the tier's)
    print('kernels reached:', sorted(fn.reach.items()))
    print('%s fuzz: %s' % (which, r))
    sys.exit(1 if r['bad'] or not r['checked'] else 0)
