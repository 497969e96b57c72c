"""The matrix-core form of the low-latency forward for 1 .. 8 images on the GPU: convtaps_narrow_mfma_kernel (KN_FLAG_NARROW_MFMA: an implicit GEMM whose N
dimension is output pixels x images) against the CPU oracle under the criteria the wide matrix-core kernel is held to (test_parity_gpu.close_conditioned /
close), the flag's semantics through the C ABI, and KeyedModel.forward_linear / capture with narrow='mfma': which layers take the kernel under which
contract, the narrow records of calibrated layers and their per-forward screen."""
import copy

import numpy as np
import pytest
import torch

from keynet_amd import io as kio
from keynet_amd import sparse as ksp
from keynet_amd import _capi
from keynet_amd.layer import KeyedLayer, gate
from test_parity_gpu import _random_convtaps, close, close_conditioned, dev
from test_narrow_gpu import SHAPES as NARROW_SHAPES, _build, _last, _oracle, _sorted_csr, _spmm
from narrow_helpers import _spmm_calls

pytestmark = pytest.mark.gpu

(RELU, EXACT, BF16X3, NARROW, MFMA) = (_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_BF16X3, _capi.KN_FLAG_NARROW, _capi.KN_FLAG_NARROW_MFMA)
KERNEL = 'convtaps_narrow_mfma_kernel'
LANE = 'convtaps_narrow_kernel'

# (id, Cin, Cout, H, k, stride, unit coefficients, bias column): Cout below / at / across a 32- and 64-channel tile, Cin no multiple of the 16-channel unit,
# 16 / 36 / 64 pixels (no multiple of the 32-column tile at 1, 3, 5 images), two slots on one (pixel, tap) pair (coef), k = 1
SHAPES = [
    ('3x3-s1-cin3-cout24-bias', 3, 24, 8, 3, 1, True, True),
    ('3x3-s2-cin5-cout64-nobias', 5, 64, 8, 3, 2, True, False),
    ('5x5-cin16-cout192-coef-bias', 16, 192, 6, 5, 1, False, True),
    ('3x3-s2-cin5-cout192-coef-bias', 5, 192, 8, 3, 2, False, True),
    ('1x1-cin7-cout70-bias', 7, 70, 6, 1, 1, True, True),
]
_cache = {}


def _case(case):
    """(W, sorted expansion, X [cols, 8]) of a case, built once."""
    if case[0] not in _cache:
        (W, M, X, _) = _build(case)
        _cache[case[0]] = (W, M, np.ascontiguousarray(X[:, :8]))
    return _cache[case[0]]


@pytest.mark.parametrize('n_vecs', [1, 2, 3, 5, 8])
@pytest.mark.parametrize('case', SHAPES, ids=[c[0] for c in SHAPES])
def test_kernel_against_the_oracle(case, n_vecs):
    """The plan names the kernel; the result passes close_conditioned against scipy's csr_matvecs on the sorted expansion, with and without ReLU; two runs
    give the same bits."""
    (W, M, X) = _case(case)
    X = X[:, :n_vecs]
    xd = torch.as_tensor(X).to(dev())
    with torch.cuda.device(dev()):
        plan = W._device_op(dev()).plan(n_vecs, MFMA)
    assert KERNEL in plan and LANE not in plan, plan
    assert 'NV=%d' % (1 if n_vecs == 1 else 2 if n_vecs == 2 else 4 if n_vecs <= 4 else 8) in plan, plan
    if not case[6]:
        t = W._taps
        pairs = t['ent_out'].astype(np.int64) * len(t['taps']) + t['ent_tap']
        assert np.bincount(pairs).max() == 2 and 'two slots per tap' in plan, plan
    ref = _oracle(M, X)
    for relu in (False, True):
        y = W.torchdot(xd, relu=relu, exact=False, narrow='mfma')
        y2 = W.torchdot(xd, relu=relu, exact=False, narrow='mfma')
        assert torch.equal(y, y2), (case[0], n_vecs, relu)
        r = np.maximum(ref, 0) if relu else ref
        y = y.cpu().numpy()
        print(case[0], n_vecs, relu, 'max |d| = %.3g' % float(np.abs(y - r).max()))
        assert close_conditioned(y.T, r.T, (M.shape, M.indptr, M.indices, M.data), X.T), (case[0], n_vecs, relu, float(np.abs(y - r).max()))


def test_flag_semantics():
    """With KN_FLAG_EXACT, at nine columns, on a CSR operator and on a filled-in operator the flag is KN_FLAG_NARROW: same plan, same bits.  Without the flag
    nothing moved (a second handle that never saw it)."""
    (W, M, X, _) = _build(('semantics', 16, 64, 8, 3, 1, True, True), seed=9)
    xd = torch.as_tensor(X).to(dev())
    with torch.cuda.device(dev()):
        op = W._device_op(dev())
        t = W._taps
        op2 = _capi.Operator.convtaps(W._inshape, W._outshape, t['taps'], t['ent_out'], t['ent_in'], t['ent_tap'], t['ent_coef'], t['lastcol'])
    for n in (1, 4, 8):
        (ym, _, pm) = _spmm(op, xd, n, MFMA)
        assert KERNEL in pm, pm
        (yn, _, pn) = _spmm(op, xd, n, NARROW)
        assert close_conditioned(ym.cpu().numpy().T, yn.cpu().numpy().T, (M.shape, M.indptr, M.indices, M.data), X[:, :n].T)
        for extra in (EXACT, EXACT | RELU, EXACT | BF16X3):
            (y, _, p) = _spmm(op, xd, n, MFMA | extra)
            (y0, _, p0) = _spmm(op, xd, n, NARROW | extra)
            assert KERNEL not in p and p == p0 and torch.equal(y, y0), (n, extra, p, p0)
        (y, _, p) = _spmm(op, xd, n, MFMA | NARROW)                          # both flags: the matrix-core form
        assert p == pm and torch.equal(y, ym)
    for flags in (0, EXACT, BF16X3):
        (y9, _, p9) = _spmm(op, xd, 9, flags | MFMA)
        (y0, _, p0) = _spmm(op, xd, 9, flags | NARROW)
        (yp, _, pp) = _spmm(op, xd, 9, flags)
        assert KERNEL not in p9 and p9 == p0 == pp and torch.equal(y9, y0) and torch.equal(y9, yp), (flags, p9, p0)
    for n in (1, 8, 64):
        for flags in (0, EXACT, RELU, BF16X3, NARROW):
            (ya, _, pa) = _spmm(op, xd, n, flags)
            (yb, _, pb) = _spmm(op2, xd, n, flags)
            assert KERNEL not in pa and pa == pb and torch.equal(ya, yb), (n, flags, pa, pb)
    # a CSR operator
    import scipy.sparse
    A = scipy.sparse.random(40, 30, density=0.3, format='csr', dtype=np.float32, random_state=3)
    xs = torch.as_tensor(np.random.RandomState(2).randn(30, 8).astype(np.float32)).to(dev())
    with torch.cuda.device(dev()):
        opc = ksp.SparseMatrix(A)._device_op(dev())
    (y1, _, p1) = _spmm(opc, xs, 4, EXACT | MFMA)
    (y0, _, p0) = _spmm(opc, xs, 4, EXACT | NARROW)
    assert p1 == p0 and torch.equal(y1, y0)
    # the filled-in 9 x 9 operator: more than 64 slots per pixel, many on one (pixel, tap) pair
    filled = [c for c in NARROW_SHAPES if c[0].startswith('filled')][0]
    (Wf, Mf, Xf, _) = _build(filled)
    xf = torch.as_tensor(Xf).to(dev())
    with torch.cuda.device(dev()):
        opf = Wf._device_op(dev())
    for n in (1, 5):
        (y1, _, p1) = _spmm(opf, xf, n, MFMA | RELU)
        (y0, _, p0) = _spmm(opf, xf, n, NARROW | RELU)
        assert KERNEL not in p1 and LANE in p1 and p1 == p0 and torch.equal(y1, y0), (n, p1, p0)


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
        assert KERNEL in op.plan(n, MFMA | RELU, ldx=ld, ldy=ld)
        op.spmm(xb.data_ptr() + 4 * c0, ld, n, yb.data_ptr() + 4 * c0, ld, MFMA | RELU, torch.cuda.current_stream().cuda_stream)
    alone = W.torchdot(xb[:, c0:c0 + n], relu=True, exact=False, narrow='mfma')
    assert torch.equal(yb[:, c0:c0 + n], alone)
    r = np.maximum(_oracle(M, Xb[:, c0:c0 + n]), 0)
    assert close_conditioned(alone.cpu().numpy().T, r.T, (M.shape, M.indptr, M.indices, M.data), Xb[:, c0:c0 + n].T)
    outside = torch.ones(ld, dtype=torch.bool, device=dev())
    outside[c0:c0 + n] = False
    assert bool(torch.all(yb[:, outside] == -3.25))


@pytest.mark.parametrize('case', [SHAPES[0], SHAPES[2], SHAPES[3]], ids=lambda c: c[0])
def test_non_finite_activations(case):
    """NaN in one column and +-Inf in another, at a few input rows: the result is finite exactly where the oracle's is (the other columns, and the output rows
    whose slot lists do not touch those inputs) and NaN where the oracle's is NaN; the finite part passes the tolerance criterion."""
    (W, M, X0) = _case(case)
    rng = np.random.RandomState(21)
    n = 5
    X = X0[:, :n].copy()
    rows = rng.choice(W.shape[1] - 1, size=6, replace=False)
    X[rows[:3], 1] = np.nan
    X[rows[3:], 3] = [np.inf, -np.inf, np.inf]
    ref = _oracle(M, X)
    assert np.isnan(ref).any() and np.isfinite(ref[:, 0]).all() and np.isfinite(ref[:, 1]).any()
    with torch.cuda.device(dev()):
        assert KERNEL in W._device_op(dev()).plan(n, MFMA)
    for relu in (False, True):
        y = W.torchdot(torch.as_tensor(X).to(dev()), relu=relu, exact=False, narrow='mfma').cpu().numpy()
        r = ref if not relu else np.where(np.isnan(ref), ref, np.maximum(ref, 0)).astype(np.float32)
        if not relu:
            assert np.array_equal(np.isfinite(y), np.isfinite(r)), (case[0], relu)
        else:                                                           # (ReLU turns the oracle's -Inf into 0: finite wherever the sum before it was, nothing claimed at its infinities)
            assert bool(np.isfinite(y[np.isfinite(ref)]).all()) and not np.isfinite(y[np.isnan(ref)]).any(), (case[0], relu)
        assert bool(np.isnan(y[np.isnan(r)]).all()), (case[0], relu)
        # (where the oracle is +-Inf the result is not finite either -- asserted above -- but may be NaN: several taps on one (output, input) pixel pair are ONE stored
        # value of the reference, whose sign decides the oracle's infinity, and separate products w_t * Inf of opposite signs in a re-ordered sum)
        fin = np.isfinite(ref)
        (Xf, yf, rf) = (np.where(np.isfinite(X), X, 0).astype(np.float32), np.where(fin, y, 0), np.where(fin, r, 0))
        bound_ok = close_conditioned(yf.T, rf.T, (M.shape, M.indptr, M.indices, M.data), Xf.T)
        assert bound_ok, (case[0], relu)


def _conv_layers(knet):
    return [(n, c) for (n, c) in knet._keyed(named=True) if isinstance(c.W, ksp.Conv2dTiledMatrix)]


def _plans(knet, n, mode):
    """The plan string of every conv layer's launch under narrow=mode."""
    out = {}
    for (name, c) in _conv_layers(knet):
        la = c.launch(dev(), narrow=mode)
        with torch.cuda.device(dev()):
            out[name] = la.op.plan(n, la.flags)
    return out


@pytest.mark.parametrize('name', ['mini_tiled_permutation.npz', 'mini_tiled_permutation8.npz'])
def test_whole_keynets_on_permutation_keys(golden, name):
    """exact_mode(False): every conv layer of forward_linear(x[:n], narrow='mfma') runs the new kernel, the logits are inside the gate the existing tests hold
    these files to (2e-5 + 2e-5 |ref| against the file's reference vectors), nothing is padded.  exact_mode(True) and a freshly loaded (undecided) key-net:
    narrow='mfma' is narrow=True bit for bit and decides nothing."""
    z = golden(name)
    knet = kio.keynet_from_arrays(z)
    idx = np.arange(8) % z['x_cipher'].shape[0]                          # eight images out of the file's few: each row has its reference vector
    x = torch.as_tensor(z['x_cipher'][idx]).to(dev())
    ref = _last(z)[idx]
    fresh = copy.deepcopy(knet.contract_report())
    assert fresh['undecided']
    y = knet.forward_linear(x[:3], narrow='mfma')
    assert torch.equal(y, knet.forward_linear(x[:3], narrow=True)) and knet.contract_report() == fresh
    assert all(KERNEL not in p and LANE in p for p in _plans(knet, 3, 'mfma').values())
    knet.exact_mode(False)
    knet._padded_forwards = 0
    for n in (1, 3, 8):
        plans = _plans(knet, n, 'mfma')
        assert plans and all(KERNEL in p for p in plans.values()), plans
        y = knet.forward_linear(x[:n], narrow='mfma').cpu().numpy()
        d = np.abs(y.astype(np.float64) - ref[:n])
        print(name, n, 'worst d / (2e-5 + 2e-5 |ref|) = %.3g' % float((d / (2e-5 + 2e-5 * np.abs(ref[:n]))).max()))
        assert close(y, ref[:n], tol=2e-5), (n, float(d.max()))
    assert knet._padded_forwards == 0
    assert all(r['narrow'] is None for r in knet.contract_report()['layers'])      # declared: nothing measured, nothing screened
    knet.exact_mode(True)
    before = copy.deepcopy(knet.contract_report())
    for n in (1, 8):
        assert torch.equal(knet.forward_linear(x[:n], narrow='mfma'), knet.forward_linear(x[:n], narrow=True))
    assert knet.contract_report() == before
    with pytest.raises(ValueError):
        knet.forward_linear(torch.cat([x, x])[:9], narrow='mfma')


@pytest.mark.parametrize('name', ['mini_tiled_orthogonal.npz', 'mini_tiled_stochastic.npz'])
def test_whole_keynets_on_float_keys(golden, name):
    """After one calibrating wide forward the first narrow='mfma' call adds narrow records only to layers calibration left on a re-ordering contract; layers
    decided exact run the channel-lane kernel (the file's bits on the reference's previous-layer activations); the logits pass `close` against the
    reference output; the wide decisions are as before."""
    z = golden(name)
    knet = kio.keynet_from_arrays(z)
    x = torch.as_tensor(z['x_cipher']).to(dev())
    knet.forward_linear(x)
    before = copy.deepcopy(knet.contract_report())
    assert not before['undecided']
    knet._padded_forwards = 0
    out = torch.cat([knet.forward_linear(x[lo:lo + 8], narrow='mfma') for lo in range(0, x.shape[0], 8)]).cpu().numpy()
    assert knet._padded_forwards == 0
    after = knet.contract_report()
    for (rb, ra) in zip(before['layers'], after['layers']):
        c = dict(knet._keyed(named=True))[ra['name']]
        reorder = ra['exact'] in (False, 'bf16x3', 'split') and ra['screened'] and isinstance(c.W, ksp.Conv2dTiledMatrix)
        assert (ra['narrow'] is not None) == reorder, ra
        assert ra['exact'] == rb['exact'] and ra['screened'] == rb['screened']
        wide = {k: v for (k, v) in (ra['calibration'] or {}).items() if k != 'narrow'}
        assert wide == (rb['calibration'] or {}), ra['name']
        if ra['narrow'] is not None:
            nr = ra['narrow']
            print(name, ra['name'], 'narrow record:', nr['decided'], 'gate ratio', nr['gate_ratio'], 'max |x|', nr['max_abs_x'], 'columns', nr['measured_on_columns'])
            assert nr['decided'] in ('mfma', 'exact') and set(('gate_ratio', 'max_abs_x', 'measured_on_columns')) <= set(nr)
            if nr['decided'] == 'mfma':
                assert nr['gate_ratio'] <= 0.5
    assert after['recalibrations'] == before['recalibrations'] and after['switched'] == before['switched']
    ref = _last(z)
    d = np.abs(out.astype(np.float64) - ref)
    print(name, "narrow='mfma' vs reference: worst d / (1e-5 + 1e-5 |ref|) = %.3g" % float((d / (1e-5 + 1e-5 * np.abs(ref))).max()))
    assert close(out, ref)
    prev = z['x_cipher']
    for (lname, c) in knet._keynet.named_children():
        if isinstance(c, KeyedLayer) and isinstance(c.W, ksp.Conv2dTiledMatrix):
            xin = torch.as_tensor(prev[:8]).to(dev())
            mode = c.narrow_mode('mfma')
            la = c.launch(dev(), narrow='mfma')
            with torch.cuda.device(dev()):
                plan = la.op.plan(8, la.flags)
            if getattr(c, '_exact', True) is True:
                assert mode is True and LANE in plan and KERNEL not in plan
                assert np.array_equal(c.forward(xin, narrow='mfma').cpu().numpy(), z['Y.%s' % lname][:8]), lname
            elif mode == 'mfma':
                assert KERNEL in plan, (lname, plan)
                assert close(c.forward(xin, narrow='mfma').cpu().numpy(), z['Y.%s' % lname][:8]), lname
        prev = z['Y.%s' % lname]


def _screened_net(golden):
    """A key-net with at least one accepted narrow record, its input batch and those layers' names."""
    z = golden('mini_tiled_permutation.npz')
    knet = kio.keynet_from_arrays(z)
    x = torch.as_tensor(z['x_cipher']).to(dev())
    knet.forward_linear(x)                                               # calibrates: permutation keys stay on the matrix cores
    knet.forward_linear(x[:4], narrow='mfma')                            # measures
    names = [r['name'] for r in knet.contract_report()['layers'] if r['narrow'] is not None and r['narrow']['decided'] == 'mfma']
    assert names, knet.contract_report()
    return (knet, x, names)


def test_the_screen(golden):
    """A batch 1 000x larger than the measured one (above RESCREEN_FACTOR) sends the accepted layers back to measurement on that batch; the result is inside
    the gate against narrow=True on the same batch.  A batch inside the factor re-measures nothing."""
    (knet, x, names) = _screened_net(golden)
    rec0 = {r['name']: dict(r['narrow']) for r in knet.contract_report()['layers'] if r['name'] in names}
    wide0 = {r['name']: (r['exact'], {k: v for (k, v) in r['calibration'].items() if k != 'narrow'}) for r in knet.contract_report()['layers'] if r['calibration']}
    y = knet.forward_linear((x[:4] * 1.5).contiguous(), narrow='mfma')    # inside the factor
    assert knet.__dict__.get('_narrow_remeasurements', 0) == 0
    assert {r['name']: r['narrow'] for r in knet.contract_report()['layers'] if r['name'] in names} == rec0
    big = (x[:4] * 1000.0).contiguous()
    y = knet.forward_linear(big, narrow='mfma')
    assert knet.__dict__.get('_narrow_remeasurements', 0) >= 1
    rep = {r['name']: r for r in knet.contract_report()['layers']}
    assert rep[names[0]]['narrow'] is not None and rep[names[0]]['narrow']['max_abs_x'] > 100 * rec0[names[0]]['max_abs_x']
    ye = knet.forward_linear(big, narrow=True)
    (ratio, _, _, _) = gate(y, ye)
    print('screen: gate ratio against narrow=True on the large batch = %.3g' % ratio)
    assert ratio <= 1.0
    assert {n: (r['exact'], {k: v for (k, v) in r['calibration'].items() if k != 'narrow'}) for (n, r) in rep.items() if r['calibration']} == wide0
    n0 = knet.__dict__['_narrow_remeasurements']
    knet.forward_linear(big * 1.2, narrow='mfma')
    assert knet.__dict__['_narrow_remeasurements'] == n0


@pytest.mark.parametrize('mode', ['declared', 'calibrated'])
def test_capture(golden, mode):
    """capture(x[:4], narrow='mfma') replayed on two different inputs equals the eager narrow='mfma' forward each time; nine images raise ValueError."""
    if mode == 'declared':
        z = golden('mini_tiled_permutation.npz')
        knet = kio.keynet_from_arrays(z)
        knet.exact_mode(False)
        x = torch.as_tensor(z['x_cipher']).to(dev())
    else:
        (knet, x, _) = _screened_net(golden)
    replay = knet.capture(x[:4], narrow='mfma')
    assert any(KERNEL in p for p in _plans(knet, 4, 'mfma').values())
    other = (x[:4].flip(0) * 0.5).contiguous()
    for xi in (x[:4], other):
        eager = knet.forward_linear(xi, narrow='mfma')
        assert torch.equal(replay(xi).clone(), eager)
    assert not torch.equal(knet.forward_linear(other, narrow='mfma'), knet.forward_linear(x[:4], narrow='mfma'))
    assert getattr(replay, 'graph', None) is not None
    with pytest.raises(ValueError):
        knet.capture(torch.cat([x, x, x])[:9], narrow='mfma')


@pytest.mark.parametrize('n', [1, 3, 8])
def test_the_forward_itself_launches_the_kernel(golden, monkeypatch, n):
    """Not the planner's word for it: the kn_spmm calls forward_linear(x[:n], narrow='mfma') ISSUES on a declared key-net carry KN_FLAG_NARROW_MFMA once per
    conv layer and resolve to the new kernel, those of narrow=True never do, and the two forwards differ in their bits (another association of the sums)."""
    z = golden('mini_tiled_permutation8.npz')
    knet = kio.keynet_from_arrays(z)
    knet.exact_mode(False)
    x = torch.as_tensor(z['x_cipher'][np.arange(8) % z['x_cipher'].shape[0]]).to(dev())[:n]
    knet.forward_linear(x, narrow='mfma')                                # operators resident
    calls = _spmm_calls(monkeypatch)
    ym = knet.forward_linear(x, narrow='mfma')
    convs = len(_conv_layers(knet))
    assert convs and sum(1 for (p, f) in calls if f & MFMA and KERNEL in p) == convs, calls
    assert not any(LANE in p for (p, f) in calls), calls
    del calls[:]
    ye = knet.forward_linear(x, narrow=True)
    assert sum(1 for (p, f) in calls if LANE in p) == convs and not any(f & MFMA or KERNEL in p for (p, f) in calls), calls
    assert not torch.equal(ym, ye)
    assert gate(ym, ye)[0] <= 1.0


def test_save_and_load_keep_the_narrow_records(golden, tmp_path, monkeypatch):
    """io.py's claim: the narrow records ride inside contract_record, so a loaded key-net runs narrow='mfma' on the accepted layers without measuring again
    (same records, same bits, the new kernel in the calls it issues) and still screens against the loaded record."""
    (knet, x, names) = _screened_net(golden)
    want = {r['name']: r['narrow'] for r in knet.contract_report()['layers']}
    y0 = knet.forward_linear(x[:4], narrow='mfma')
    k2 = kio.load_keynet(kio.save_keynet(knet, str(tmp_path / 'k.npz')))
    assert {r['name']: r['narrow'] for r in k2.contract_report()['layers']} == want
    calls = _spmm_calls(monkeypatch)
    y2 = k2.forward_linear(x[:4], narrow='mfma')
    assert torch.equal(y2, y0)
    assert sum(1 for (p, f) in calls if KERNEL in p) == len(names), calls          # one launch per accepted layer: no measurement ran both kernels
    assert {r['name']: r['narrow'] for r in k2.contract_report()['layers']} == want and k2.__dict__.get('_narrow_remeasurements', 0) == 0
    k2.forward_linear((x[:4] * 1000.0).contiguous(), narrow='mfma')
    assert k2.__dict__.get('_narrow_remeasurements', 0) >= 1


def test_the_shape_that_keeps_the_channel_lane_kernel():
    """The library's one shape rule (measured on VGG-16 conv1_1, profiles/r08_narrow_mfma.txt): Cin <= 4 at 5 .. 8 columns on a layer whose channel-lane grid
    fills the chip (64 x 64 pixels x 64 channels = 1 024 workgroups) is KN_FLAG_NARROW bit for bit; up to 4 columns, with Cin = 5, or on fewer pixels it is the
    matrix-core kernel.  A calibrated layer of that shape measures the matrix-core kernel on the columns that run it."""
    rng = np.random.RandomState(3)
    W = _random_convtaps(rng, 3, 64, 64, 3, 1, True, True)
    xd = torch.as_tensor(rng.randn(W.shape[1], 8).astype(np.float32)).to(dev())
    with torch.cuda.device(dev()):
        op = W._device_op(dev())
    for n in (5, 8):
        (y, _, plan) = _spmm(op, xd, n, MFMA)
        (ye, _, plan_e) = _spmm(op, xd, n, NARROW)
        assert plan == plan_e and LANE in plan and KERNEL not in plan and torch.equal(y, ye), plan
    (y4, _, plan) = _spmm(op, xd, 4, MFMA)
    assert KERNEL in plan, plan
    (ye4, _, _) = _spmm(op, xd, 4, NARROW)
    assert gate(y4, ye4)[0] <= 1.0
    for (cin, h) in ((5, 64), (3, 32)):
        V = _random_convtaps(rng, cin, 64, h, 3, 1, True, True)
        with torch.cuda.device(dev()):
            assert KERNEL in V._device_op(dev()).plan(8, MFMA)
    layer = KeyedLayer.__new__(KeyedLayer)
    (layer.W, layer._repr) = (W, 'conv')
    rec = layer._measure_narrow(xd, False)
    assert rec['decided'] == 'mfma' and rec['measured_on_columns'] == 4 and rec['gate_ratio'] > 0, rec
