"""The narrow split route of a filled-in conv layer on the GPU (narrow='mfma', narrow_split=True; 1 .. 32 images): the plane <-> column permute of the C ABI against
numpy.transpose, Conv2dTiledMatrix._torchdot_split_narrow against the wide split route (the intermediate, bit for bit) and against the order-preserving kernel (the
result, under the criterion the wide matrix-core kernel is held to), the argument and fall-back rules of the keyword, the narrow_split record of a calibrated layer
with its screen, save / load, a whole key-net, and capture."""
import collections
import copy

import numpy as np
import pytest
import torch

from keynet_amd import io as kio
from keynet_amd import sparse as ksp
from keynet_amd import _capi
from keynet_amd.layer import KeyedLayer
from keynet_amd.system import KeyedModel
from test_parity_gpu import _filled_in_convtaps, _random_convtaps, close, close_conditioned, dev
from test_narrow_gpu import _last

pytestmark = pytest.mark.gpu

KERNEL = 'convtaps_narrow_mfma_kernel'
SENTINEL = np.float32(7.5)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _recorded(call):
    """(what call() returns, [(plan, flags)] of the kn_spmm / kn_spmm_screen calls the Python host issued inside it): the path the call really takes."""
    calls = []
    spmm = _capi.Operator.spmm

    def recording(self, x_ptr, ldx, n_vecs, y_ptr, ldy, flags, stream, absmax_ptr=None):
        calls.append((self.plan(n_vecs, flags, ldx=ldx, ldy=ldy), int(flags)))
        return spmm(self, x_ptr, ldx, n_vecs, y_ptr, ldy, flags, stream, absmax_ptr)
    _capi.Operator.spmm = recording
    try:
        return (call(), calls)
    finally:
        _capi.Operator.spmm = spmm


# -- the permute ----------------------------------------------------------------------------------------------------------------------------------
def _payload(rng, shape):
    """float32 values as bit patterns: normals, -0, +0, quiet and signalling NaNs with payloads, infinities."""
    v = rng.randn(*shape).astype(np.float32).view(np.uint32)
    special = np.array([0x80000000, 0x00000000, 0x7fc00001, 0xffc12345, 0x7f800001, 0x7f800000, 0xff800000], dtype=np.uint32)
    pick = rng.rand(*shape) < 0.2
    v[pick] = special[rng.randint(0, len(special), size=int(pick.sum()))]
    return v


def _layouts(planes, rows, n):
    """(name, ld, plane stride, base offset of the planes side, ld of the columns side, base offset of the columns side), floats: compact and aligned (16 bytes per
    lane on both sides), strided and unaligned (float by float), and where a row is whole quads the aligned strided form (16 bytes per lane inside each row)."""
    out = [('compact', n, -(-rows * n // 4) * 4, 0, -(-planes * n // 4) * 4, 0),
           ('ragged', n + 3, rows * (n + 3) + 5, 1, planes * n + 7, 3)]
    if n % 4 == 0:
        out.append(('rows of quads', n + 4, rows * (n + 4) + 8, 4, planes * n + 12, 8))
    return out


@pytest.mark.parametrize('planes,rows,n', [(3, 36, 1), (3, 64, 3), (16, 36, 5), (64, 49, 8), (5, 100, 32)])
def test_permute_is_numpy_transpose_both_ways(planes, rows, n):
    rng = np.random.RandomState(planes * 1000 + rows * 10 + n)
    for (name, ld, ps, poff, ldc, coff) in _layouts(planes, rows, n):
        bits = _payload(rng, (planes, rows, n))
        P = np.full(poff + planes * ps + 9, SENTINEL, dtype=np.float32)
        Pw = np.lib.stride_tricks.as_strided(P[poff:], shape=(planes, rows, n), strides=(4 * ps, 4 * ld, 4))
        Pw.view(np.uint32)[...] = bits
        want_cols = np.ascontiguousarray(np.transpose(bits, (1, 0, 2))).reshape(rows, planes * n)
        pd = torch.as_tensor(P).to(dev())
        cd = torch.full((coff + rows * ldc + 9,), float(SENTINEL), dtype=torch.float32, device=dev())
        with torch.cuda.device(dev()):
            _capi.planes_to_columns(pd.data_ptr() + 4 * poff, ps, ld, planes, rows, n, cd.data_ptr() + 4 * coff, ldc, _stream())
        C = cd.cpu().numpy()
        Cw = np.lib.stride_tricks.as_strided(C[coff:], shape=(rows, planes * n), strides=(4 * ldc, 4))
        assert np.array_equal(Cw.view(np.uint32), want_cols), (name, planes, rows, n)
        expect = np.full_like(C, SENTINEL)
        np.lib.stride_tricks.as_strided(expect[coff:], shape=(rows, planes * n), strides=(4 * ldc, 4)).view(np.uint32)[...] = want_cols
        assert np.array_equal(C.view(np.uint32), expect.view(np.uint32)), (name, 'padding of the column block touched')
        # the inverse direction into a sentinel-filled block: the round trip is the identity, the padding stays
        bd = torch.full((len(P),), float(SENTINEL), dtype=torch.float32, device=dev())
        with torch.cuda.device(dev()):
            _capi.columns_to_planes(cd.data_ptr() + 4 * coff, ldc, planes, rows, n, bd.data_ptr() + 4 * poff, ps, ld, _stream())
        assert np.array_equal(bd.cpu().numpy().view(np.uint32), P.view(np.uint32)), (name, planes, rows, n)


def test_permute_of_a_plane_beyond_2_to_31_elements():
    """Two planes, the second beginning beyond 2^31 elements (an 8.6 GB block of which only the two planes are touched), both directions."""
    (rows, n, ld) = (36, 5, 5)
    ps = (1 << 31) + 8
    rng = np.random.RandomState(31)
    bits = _payload(rng, (2, rows, n))
    big = torch.empty(ps + rows * ld + 16, dtype=torch.float32, device=dev())
    for p in range(2):
        big[p * ps:p * ps + rows * ld] = torch.as_tensor(bits[p].view(np.float32).reshape(-1)).to(dev())
    cd = torch.full((rows * 2 * n + 8,), float(SENTINEL), dtype=torch.float32, device=dev())
    with torch.cuda.device(dev()):
        _capi.planes_to_columns(big.data_ptr(), ps, ld, 2, rows, n, cd.data_ptr(), 2 * n, _stream())
    C = cd.cpu().numpy()
    want = np.ascontiguousarray(np.transpose(bits, (1, 0, 2))).reshape(rows, 2 * n)
    assert np.array_equal(C[:rows * 2 * n].view(np.uint32).reshape(rows, 2 * n), want) and np.all(C[rows * 2 * n:] == SENTINEL)
    for p in range(2):
        big[p * ps:p * ps + rows * ld + 8] = float(SENTINEL)
    with torch.cuda.device(dev()):
        _capi.columns_to_planes(cd.data_ptr(), 2 * n, 2, rows, n, big.data_ptr(), ps, ld, _stream())
    for p in range(2):
        got = big[p * ps:p * ps + rows * ld + 8].cpu().numpy()
        assert np.array_equal(got[:rows * ld].view(np.uint32).reshape(rows, n), bits[p]) and np.all(got[rows * ld:] == SENTINEL), p
    del big


# -- the route against the wide route ------------------------------------------------------------------------------------------------------------------
ROUTE = [(16, 64, 6, 5, True), (3, 40, 8, 3, True), (32, 128, 4, 6, False)]
WIDTHS = [1, 2, 3, 5, 8, 9, 16, 32]
_cache = {}


def _route_case(case):
    """Built once per operator and left unchanged: (W, sorted expansion, X [cols, 32], wide intermediate Z [Cin nt HoWo, 32], order-preserving Y [rows, 32])."""
    if case not in _cache:
        (Cin, Cout, H, fill, has_last) = case
        rng = np.random.RandomState(Cin + Cout + fill)
        W = _filled_in_convtaps(rng, Cin, Cout, H, fill, has_last)
        X = rng.randn(W.shape[1], 32).astype(np.float32)
        if has_last:
            X[-1] = 1.0
        M = W.tosparse('csr')
        M.sort_indices()
        xd = torch.as_tensor(X).to(dev())
        # the intermediate as the wide _torchdot_split forms it: the spatial CSR on every input channel's plane (one launch over the planes, else plane by plane)
        (nt, HW) = (len(W._taps['taps']), H * H)
        with torch.cuda.device(dev()):
            (opK, _) = W._split_ops(dev())
            z = torch.empty((Cin * nt * HW, 32), dtype=torch.float32, device=dev())
            if not opK.spmm_planes(xd.data_ptr(), 32, HW * 32, Cin, 32, z.data_ptr(), 32, nt * HW * 32, _capi.KN_FLAG_EXACT, _stream()):
                for ci in range(Cin):
                    opK.spmm(xd.data_ptr() + 4 * ci * HW * 32, 32, 32, z.data_ptr() + 4 * ci * nt * HW * 32, 32, _capi.KN_FLAG_EXACT, _stream())
        ye = W.torchdot(xd, exact=True).cpu().numpy()
        _cache[case] = (W, M, X, z.cpu().numpy(), ye)
    return _cache[case]


def _intermediate(W, n):
    """Z [zrows, n] as the last narrow split call of n columns left it in the operator's workspace."""
    (_, _, z) = W._narrow_split_workspace(dev(), n)
    zrows = W._inshape[0] * len(W._taps['taps']) * W._outshape[1] * W._outshape[2] + (1 if W._taps['lastcol'] is not None else 0)
    return z[:zrows * n].view(zrows, n).cpu().numpy()


@pytest.mark.parametrize('n', WIDTHS)
@pytest.mark.parametrize('case', ROUTE, ids=['cin16', 'cin3', 'cin32-nobias'])
def test_route_against_the_wide_route_and_the_order_preserving_kernel(case, n):
    (W, M, X, zwide, ye) = _route_case(case)
    has_last = case[4]
    xd = torch.as_tensor(np.ascontiguousarray(X[:, :n])).to(dev())
    with torch.cuda.device(dev()):
        plan = W._split_ops(dev())[1].plan(n, W._narrow_split_flags(n, False))
    assert KERNEL in plan, plan
    for relu in (False, True):
        slot = torch.zeros(1, dtype=torch.float32, device=dev())
        y = W._torchdot_split_narrow(xd, relu=relu, absmax=slot)
        Z = _intermediate(W, n)
        assert np.array_equal(Z[:zwide.shape[0]].view(np.uint32), zwide[:, :n].view(np.uint32)), (case, n, 'the intermediate is not the wide route\'s')
        if has_last:
            assert np.array_equal(Z[-1], X[-1, :n])
        assert torch.equal(W._torchdot_split_narrow(xd, relu=relu), y), (case, n, relu)
        y = y.cpu().numpy()
        r = np.maximum(ye[:, :n], 0) if relu else ye[:, :n]
        print(case, n, relu, 'max |d| = %.3g' % float(np.abs(y - r).max()))
        assert close_conditioned(y.T, r.T, (M.shape, M.indptr, M.indices, M.data), X[:, :n].T), (case, n, relu, float(np.abs(y - r).max()))
        assert float(slot) == np.abs(y).max()


@pytest.mark.parametrize('case', ROUTE, ids=['cin16', 'cin3', 'cin32-nobias'])
def test_an_image_has_the_same_bits_at_every_width_and_in_every_window(case):
    (W, M, X, zwide, ye) = _route_case(case)
    y32 = W._torchdot_split_narrow(torch.as_tensor(X).to(dev()))
    for n in WIDTHS[:-1]:
        y = W._torchdot_split_narrow(torch.as_tensor(np.ascontiguousarray(X[:, :n])).to(dev()))
        assert torch.equal(y, y32[:, :n]), (case, n)
    # windows of whole images in the first three steps: 3 images per window at 8 and at 32 columns
    (Cin, nt, HW) = (case[0], 9, case[2] * case[2])
    W.NARROW_SPLIT_Z_BYTES = 4 * nt * HW * Cin * 3
    try:
        assert W._narrow_split_window(8) == 3
        for n in (8, 32):
            y = W._torchdot_split_narrow(torch.as_tensor(np.ascontiguousarray(X[:, :n])).to(dev()))
            assert torch.equal(y, y32[:, :n]), (case, n, 'windows')
            assert np.array_equal(_intermediate(W, n)[:zwide.shape[0]].view(np.uint32), zwide[:, :n].view(np.uint32))
    finally:
        del W.NARROW_SPLIT_Z_BYTES
        W.release_narrow_split_workspace()


# -- argument and fall-back rules --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def offered(monkeypatch):
    """The cost rule offers the route to every operator with a split form (the test operators are far below the sizes its estimate is about)."""
    monkeypatch.setattr(ksp.Conv2dTiledMatrix, 'NARROW_SPLIT_MIN_GAIN', 0.0)


def test_the_keyword_through_torchdot(monkeypatch):
    """exact='split', narrow='mfma', narrow_split=True IS the route (four steps, the last on the matrix-core narrow kernel); the cost rule alone keeps these small
    operators fused; without narrow='mfma' the keyword is refused."""
    (W, M, X, _, _) = _route_case(ROUTE[0])
    for (n, kw) in ((5, {}), (16, dict(narrow32=True))):
        xd = torch.as_tensor(np.ascontiguousarray(X[:, :n])).to(dev())
        direct = W._torchdot_split_narrow(xd, relu=True)
        # the cost rule (its own constants): this operator is not worth the route, and the call is the call without the keyword
        assert not W.narrow_split_capable(n)
        assert torch.equal(W.torchdot(xd, relu=True, exact='split', narrow='mfma', narrow_split=True, **kw), W.torchdot(xd, relu=True, exact='split', narrow='mfma', **kw))
        monkeypatch.setattr(ksp.Conv2dTiledMatrix, 'NARROW_SPLIT_MIN_GAIN', 0.0)
        (y, calls) = _recorded(lambda: W.torchdot(xd, relu=True, exact='split', narrow='mfma', narrow_split=True, **kw))
        assert torch.equal(y, direct) and len(calls) == 2 and KERNEL in calls[1][0], calls
        for narrow in (False, True):
            with pytest.raises(ValueError, match='narrow_split=True'):
                W.torchdot(xd, exact='split', narrow=narrow, narrow_split=True, **(kw if narrow else {}))
        monkeypatch.undo()
    # under every other contract the keyword is inert
    xd = torch.as_tensor(np.ascontiguousarray(X[:, :5])).to(dev())
    for exact in (True, False):
        assert torch.equal(W.torchdot(xd, exact=exact, narrow='mfma', narrow_split=True), W.torchdot(xd, exact=exact, narrow='mfma'))


def _tiny_net(W, exact):
    L = KeyedLayer.fromoperator(W, 'Conv2d', inshape=W._inshape, outshape=W._outshape, exact=exact)
    return (KeyedModel.fromlayers(collections.OrderedDict([('conv', L)]), W._outshape), L)


def test_the_keyword_is_inert_where_there_is_no_route(offered, golden):
    rng = np.random.RandomState(3)
    # a 9-slot (permutation-keyed) conv operator, declared 'split' and declared False
    Wp = _random_convtaps(rng, 16, 64, 6, 3, 1, True, True)
    assert not Wp.split_capable()
    x = torch.as_tensor(np.concatenate((rng.randn(8, Wp.shape[1] - 1), np.ones((8, 1))), axis=1).astype(np.float32)).to(dev())
    for exact in ('split', False):
        (knet, _) = _tiny_net(Wp, exact)
        assert torch.equal(knet.forward_linear(x, narrow='mfma', narrow_split=True), knet.forward_linear(x, narrow='mfma'))
    # CSR layers (an untiled key-net): nothing to route
    z = golden('lenet_perm.npz')
    knet = kio.keynet_from_arrays(z)
    xl = torch.as_tensor(z['x_cipher'][:4]).to(dev())
    assert torch.equal(knet.forward_linear(xl, narrow='mfma', narrow_split=True), knet.forward_linear(xl, narrow='mfma'))
    # a filled-in layer: beyond 32 images, and under exact_mode(True)
    (W, M, X, _, _) = _route_case(ROUTE[0])
    (knet, L) = _tiny_net(W, 'split')
    x64 = torch.as_tensor(np.ascontiguousarray(np.concatenate((X, X * 0.5), axis=1)[:, :40].T)).to(dev())
    x64[:, -1] = 1.0
    kw = dict(narrow='mfma', narrow64='mfma')
    assert torch.equal(knet.forward_linear(x64, narrow_split=True, **kw), knet.forward_linear(x64, **kw))
    x8 = x64[:8].contiguous()
    routed = knet.forward_linear(x8, narrow='mfma', narrow_split=True)
    assert not torch.equal(routed, knet.forward_linear(x8, narrow='mfma'))          # (here the keyword does something: the comparison above is not vacuous)
    knet.exact_mode(True)
    assert torch.equal(knet.forward_linear(x8, narrow='mfma', narrow_split=True), knet.forward_linear(x8, narrow='mfma'))
    for bad in (dict(narrow=True), dict()):
        with pytest.raises(ValueError, match='narrow_split=True'):
            knet.forward_linear(x8, narrow_split=True, **bad)
        with pytest.raises(ValueError, match='narrow_split=True'):
            knet.capture(x8, narrow_split=True, **bad)


# -- a calibrated layer, a whole key-net, capture ----------------------------------------------------------------------------------------------------------------
def _calibrated_layer():
    """The layer of test_parity_gpu.test_calibration_takes_the_split_application_for_a_filled_in_layer, calibrated on its 128 images: decided 'split'."""
    rng = np.random.RandomState(5)
    W = _filled_in_convtaps(rng, 16, 64, 6, 20, gentle=True)
    (knet, L) = _tiny_net(W, 'auto')
    x = torch.as_tensor(np.concatenate((rng.randn(128, W.shape[1] - 1), np.ones((128, 1))), axis=1).astype(np.float32)).to(dev())
    knet.forward_linear(x)
    assert L._exact == 'split' and L.screened() and L.narrow_split_record() is None
    return (knet, L, x)


def test_a_calibrated_layer_measures_records_screens_and_saves(offered, tmp_path):
    (knet, L, x) = _calibrated_layer()
    y_plain = knet.forward_linear(x[:8], narrow='mfma')                   # the parent's behaviour: the fused operator on the channel-lane kernel, a 'narrow' record
    wide0 = {k: copy.deepcopy(v) for (k, v) in L._contract_record.items() if k != 'narrow_split'}
    assert wide0['narrow']['decided'] == 'exact'
    y = knet.forward_linear(x[:8], narrow='mfma', narrow_split=True)
    rec = L.narrow_split_record()
    print('narrow_split record:', rec)
    assert rec['decided'] == 'split' and rec['gate_ratio'] <= 0.5 and rec['measured_on_columns'] == 8 and rec['max_abs_x'] == float(x[:8].abs().max())
    assert {k: v for (k, v) in L._contract_record.items() if k != 'narrow_split'} == wide0 and L._exact == 'split'
    assert torch.equal(y, L.W._torchdot_split_narrow(x[:8].t().contiguous(), relu=False).t()) and not torch.equal(y, y_plain)
    assert torch.equal(knet.forward_linear(x[:8], narrow='mfma'), y_plain)                       # without the keyword nothing moved
    rep = knet.contract_report()['layers'][0]
    assert rep['narrow_split'] == rec and rep['narrow'] == wide0['narrow'] and rep['calibration']['narrow_split'] == rec
    # 32 images: the same record covers them (measured on 8 columns: an image's bits do not depend on the width)
    y32 = knet.forward_linear(x[:32], narrow='mfma', narrow32=True, narrow_split=True)
    assert torch.equal(y32[:8], y) and L.narrow_split_record() == rec and knet.__dict__.get('_narrow_remeasurements', 0) == 0
    # save and load keep it: one route, no measurement
    k2 = kio.load_keynet(kio.save_keynet(knet, str(tmp_path / 'k.npz')))
    assert k2.contract_report()['layers'][0]['narrow_split'] == rec
    (y2, calls) = _recorded(lambda: k2.forward_linear(x[:8], narrow='mfma', narrow_split=True))
    assert torch.equal(y2, y) and len(calls) == 2 and KERNEL in calls[1][0], calls
    # a 3x larger batch trips only that record: measured again on that batch, everything else as it was
    big = (x[:8] * 3.0).contiguous()
    big[:, -1] = 1.0
    yb = knet.forward_linear(big, narrow='mfma', narrow_split=True)
    rec2 = L.narrow_split_record()
    assert knet.__dict__.get('_narrow_remeasurements', 0) == 1 and rec2['max_abs_x'] == float(big.abs().max()) and rec2['decided'] == 'split'
    assert {k: v for (k, v) in L._contract_record.items() if k != 'narrow_split'} == wide0 and L._exact == 'split' and knet.contract_report()['recalibrations'] == 0
    assert torch.equal(yb, L.W._torchdot_split_narrow(big.t().contiguous(), relu=False).t())
    # release_workspace and pickling drop the workspaces; the next call builds them again
    assert L.W.__dict__.get('_narrow_split_ws')
    knet.release_workspace()
    assert not L.W.__dict__.get('_narrow_split_ws') and '_narrow_split_ws' not in L.W.__getstate__()
    assert torch.equal(knet.forward_linear(big, narrow='mfma', narrow_split=True), yb)


def test_whole_keynet_on_doubly_stochastic_keys(offered, golden):
    """mini_tiled_stochastic.npz after its calibrating wide forward: the logits of narrow='mfma', narrow_split=True pass `close` against the reference output, the wide
    decisions are as before, and only layers calibration decided 'split' carry a narrow_split record."""
    z = golden('mini_tiled_stochastic.npz')
    knet = kio.keynet_from_arrays(z)
    x = torch.as_tensor(z['x_cipher']).to(dev())
    knet.forward_linear(x)
    before = copy.deepcopy(knet.contract_report())
    out = torch.cat([knet.forward_linear(x[lo:lo + 8], narrow='mfma', narrow_split=True) for lo in range(0, x.shape[0], 8)]).cpu().numpy()
    after = knet.contract_report()
    for (rb, ra) in zip(before['layers'], after['layers']):
        assert ra['exact'] == rb['exact'] and ra['screened'] == rb['screened'] and ra['declared'] == rb['declared']
        assert {k: v for (k, v) in (ra['calibration'] or {}).items() if k not in ('narrow', 'narrow_split')} == (rb['calibration'] or {}), ra['name']
        assert ('narrow_split' not in ra) or ra['exact'] == 'split'
        print(ra['name'], ra['exact'], ra.get('narrow_split'))
    assert after['switched'] == before['switched'] and after['recalibrations'] == before['recalibrations'] and after['undecided'] == before['undecided']
    ref = _last(z)
    d = np.abs(out.astype(np.float64) - ref)
    print('narrow_split vs reference: worst d / (1e-5 + 1e-5 |ref|) = %.3g' % float((d / (1e-5 + 1e-5 * np.abs(ref))).max()))
    assert close(out, ref)


@pytest.mark.parametrize('n', [1, 8])
def test_capture_replays_the_eager_forward(offered, n):
    (knet, L, x) = _calibrated_layer()
    kw = dict(narrow='mfma', narrow_split=True)
    replay = knet.capture(x[:n], **kw)                                   # measures and allocates eagerly, then captures
    assert L.narrow_split_record()['decided'] == 'split'
    other = (x[n:2 * n] * 0.5).contiguous()
    other[:, -1] = 1.0
    for xi in (x[:n], other):
        assert torch.equal(replay(xi).clone(), knet.forward_linear(xi, **kw))
    assert not torch.equal(knet.forward_linear(other, **kw), knet.forward_linear(x[:n], **kw))
    assert getattr(replay, 'graph', None) is not None
