"""KN_MODIFIER_WINO on the GPU, through the C ABI: a keyed 3 x 3 / pad-1 conv in its 1-D Winograd F(2,3) form (wino_in_kernel, the derived conv-taps operator on the matrix
cores, wino_out_kernel) against the SAME handle's KN_FLAG_EXACT result.

Operators: the factored form keynet_amd.direct emits (shift matrices, tap = 3 i + j) under the identity key and under a pixel permutation on either side.  Every case runs
with and without a last column and with ReLU on and off:
  - inputs with max |x| <= 1: EVERY element inside 1e-5 + 1e-5 |ref| of KN_FLAG_EXACT (no element excluded);
  - integer activations and integer taps with g0 +- g1 + g2 even (so U is integer and every sum exact in f32): bit-equal to KN_FLAG_EXACT -- a wrong index or sign shows;
  - the screen's slot equals max |Y|, the homogeneous row is exact.
Then: two streams on one handle, a captured graph behind kn_reserve_workspace_flags, and the cases where the flag changes nothing (no flag, 37 columns, an odd width, a
gain key): the parent's plan string and bits."""
import numpy as np
import pytest
import torch

from keynet_amd import _capi
from keynet_amd import direct as kdirect
from keynet_amd.layer import gate
from narrow_helpers import _spmm
from test_parity_gpu import dev
from value_classes import assert_bits_equal

pytestmark = pytest.mark.gpu

(RELU, EXACT, WINO) = (_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_MODIFIER_WINO)

# case -> (H, W, Cin, Cout, columns, permuted key, leading dimension or None, start column)
CASES = {
    '6x4': (6, 4, 16, 16, 128, False, None, 0),
    '2x2': (2, 2, 16, 16, 128, True, None, 0),                  # every pixel on two edges
    '8x6-c20-o72': (8, 6, 20, 72, 128, True, None, 0),          # generic loader, Cout tile remainder
    '14x14-c128': (14, 14, 128, 128, 256, True, None, 0),
    '6x4-window': (6, 4, 16, 16, 128, True, 384, 128),          # a column window of a wider block
}
_ops = {}


def _entries(H, W, permuted, rng):
    HW = H * W
    (po, pi) = (rng.permutation(HW), rng.permutation(HW)) if permuted else (np.arange(HW), np.arange(HW))
    (eo, ei, et) = ([], [], [])
    for (t, (_, S)) in enumerate(kdirect.shift_matrices((H, W), 3, 1)):
        S = S.tocoo()
        eo.append(po[S.row]); ei.append(pi[S.col]); et.append(np.full(S.nnz, t))
    return tuple(np.concatenate(a).astype(np.int32) for a in (eo, ei, et))


def _integer_taps(rng, cout, cin):
    """Integer taps in -2 .. 3 with g0 + g1 + g2 even in every kernel row: U1 and U2 are integers."""
    g = rng.randint(-2, 3, size=(3, 3, cout, cin))
    g[:, 1] += (g.sum(axis=1) % 2)
    return g.reshape(9, cout, cin).astype(np.float32)


def _operator(name, last, integer):
    """(handle, X on the device [cols, ld]) -- built once, left unchanged."""
    key = (name, last, integer)
    if key not in _ops:
        (H, W, cin, cout, n, permuted, ld, start) = CASES[name]
        rng = np.random.RandomState(sum(map(ord, name)) + 2 * last + integer)
        HW = H * W
        (eo, ei, et) = _entries(H, W, permuted, rng)
        if integer:
            taps = _integer_taps(rng, cout, cin)
            lastcol = np.concatenate((rng.randint(-4, 5, size=cout * HW), [1])).astype(np.float32)
            X = rng.randint(-3, 4, size=(cin * HW + last, ld or n)).astype(np.float32)
        else:
            taps = (rng.randn(9, cout, cin) / np.sqrt(9 * cin)).astype(np.float32)
            lastcol = np.concatenate((rng.randn(cout * HW), [1.0])).astype(np.float32)
            X = rng.uniform(-1, 1, size=(cin * HW + last, ld or n)).astype(np.float32)
        if last:
            X[-1] = 1.0
        with torch.cuda.device(dev()):
            op = _capi.Operator.convtaps((cin, H, W), (cout, H, W), taps, eo, ei, et, None, lastcol if last else None)
        _ops[key] = (op, torch.as_tensor(X).to(dev()))
    return _ops[key]


@pytest.mark.parametrize('last', (1, 0), ids=('lastcol', 'nolast'))
@pytest.mark.parametrize('name', list(CASES))
def test_form_against_the_order_preserving_result(name, last):
    (H, W, cin, cout, n, permuted, ld, start) = CASES[name]
    for integer in (0, 1):
        (op, xd) = _operator(name, last, integer)
        assert op.wino_status() == (True, 'eligible')
        for relu in (0, RELU):
            slot = torch.zeros(1, dtype=torch.float32, device=dev())
            (y, whole, plan) = _spmm(op, xd, n, WINO | relu, ld=ld, start=start, absmax=slot)
            (ye, _, _) = _spmm(op, xd, n, EXACT | relu, ld=ld, start=start)
            print(plan)
            launches = plan.split('; ')
            assert launches[0].startswith('wino_in_kernel') and 'convtaps_mfma_kernel' in launches[1] and launches[2].startswith('wino_out_kernel'), plan
            assert (launches[3:] == [] if not last else launches[3].startswith('conv_lastrow_kernel')), plan
            if integer:
                assert_bits_equal(y.cpu().numpy(), ye.cpu().numpy(), '%s last=%d relu=%d' % (name, last, relu))
            else:
                g = gate(y, ye)
                print('%s last=%d relu=%d: gate against KN_FLAG_EXACT %.3g' % (name, last, relu, g[0]))
                assert g[0] <= 1, (name, last, relu, g)
            assert float(slot) == float(y.abs().max())
            if last:
                assert torch.equal(y[-1], torch.ones_like(y[-1]))
            if ld is not None:                                  # nothing outside the window was written
                mask = torch.ones_like(whole, dtype=torch.bool)
                mask[:, start:start + n] = False
                assert torch.equal(whole[mask], torch.full_like(whole[mask], float(whole[0, 0])))


def test_two_streams_on_one_handle_give_the_single_call_bits():
    (op, xd) = _operator('14x14-c128', 1, 0)
    (rows, _) = op.shape()
    (y1, _, _) = _spmm(op, xd, 256, WINO | RELU)
    y2 = torch.zeros(rows, 256, dtype=torch.float32, device=dev())
    streams = (torch.cuda.Stream(), torch.cuda.Stream())
    torch.cuda.synchronize()
    with torch.cuda.device(dev()):
        for (k, s) in enumerate(streams):
            op.spmm(xd.data_ptr() + 4 * 128 * k, 256, 128, y2.data_ptr() + 4 * 128 * k, 256, WINO | RELU, s.cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(y1, y2)


def test_a_captured_graph_behind_the_reservation_replays_the_same_bits():
    (op, xd) = _operator('6x4', 1, 0)
    (rows, _) = op.shape()
    (y1, _, _) = _spmm(op, xd, 128, WINO)
    y2 = torch.zeros(rows, 128, dtype=torch.float32, device=dev())
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.device(dev()):
        op.reserve_workspace(128, side.cuda_stream, flags=WINO)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            op.spmm(xd.data_ptr(), 128, 128, y2.data_ptr(), 128, WINO, torch.cuda.current_stream().cuda_stream)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(y1, y2)


def test_where_the_flag_changes_nothing():
    """No flag, a width that is no multiple of 128, KN_FLAG_EXACT, and operators that are not eligible (odd width, a gain key): the plan string and the bits of the call
    without the flag."""
    (op, xd) = _operator('6x4', 1, 0)
    for (n, flags) in ((37, 0), (128, EXACT), (37, RELU)):
        x = xd[:, :n].contiguous()
        (y0, _, p0) = _spmm(op, x, n, flags)
        (y1, _, p1) = _spmm(op, x, n, flags | WINO)
        assert p0 == p1 and 'wino' not in p1 and torch.equal(y0, y1), (n, flags, p0, p1)
    assert 'wino' not in _spmm(op, xd, 128, 0)[2]
    rng = np.random.RandomState(5)
    for (H, W, gain, why) in ((4, 3, False, 'odd width'), (6, 4, True, 'coefficients other than 1')):
        (eo, ei, et) = _entries(H, W, True, rng)
        taps = (rng.randn(9, 16, 16) / 12).astype(np.float32)
        ec = (rng.rand(len(eo)) + 0.5).astype(np.float32) if gain else None
        lastcol = np.concatenate((rng.randn(16 * H * W), [1.0])).astype(np.float32)
        with torch.cuda.device(dev()):
            bad = _capi.Operator.convtaps((16, H, W), (16, H, W), taps, eo, ei, et, ec, lastcol)
        (ok, reason) = bad.wino_status()
        assert not ok and why in reason, reason
        x = torch.as_tensor(rng.uniform(-1, 1, size=(16 * H * W + 1, 128)).astype(np.float32)).to(dev())
        (y0, _, p0) = _spmm(bad, x, 128, RELU)
        (y1, _, p1) = _spmm(bad, x, 128, RELU | WINO)
        assert p0 == p1 and 'wino' not in p1 and torch.equal(y0, y1), (p0, p1)


# ---- the form inside a key-net: calibration offers it, the launch list carries it ---------------------------------------------------------------------------
# A width-16 VGG-16 slice (the model's five pools need 32 x 32 pixels) under a tiled permutation key, exact='auto', the cost threshold lowered to its 16 channels.

def _slice_net(monkeypatch, min_channels):
    from keynet_amd import sparse as ksp
    from keynet_amd import system as ksys
    from keynet_amd.layer import KeyedLayer
    from keynet_amd.models import VGG16
    monkeypatch.setattr(ksp.Conv2dTiledMatrix, 'WINO_MIN_CHANNELS', min_channels)
    # the form is derived from the factored operator of the direct keying (taps 3 i + j), the route the full-size key-nets take by their size: here every conv from
    # conv1_2 on takes it (>= 590 k Toeplitz entries), conv1_1 (442 k) and the pools (<= 262 k) keep the reference route
    monkeypatch.setattr(KeyedLayer, 'DIRECT_THRESHOLD', 500000)
    torch.manual_seed(0)
    net = VGG16(num_classes=10, width=16, fc_width=64, insize=32).eval()
    np.random.seed(0)
    return ksys.TiledPermutationKeynet((3, 32, 32), net, 8, exact='auto')


def test_calibration_offers_the_form_and_the_forward_carries_it(monkeypatch):
    (sensor, knet) = _slice_net(monkeypatch, 16)
    torch.manual_seed(1)
    xc = sensor.fromtensor(torch.rand(256, 3, 32, 32).to(dev())).encrypt().astensor()
    y = knet.forward_linear(xc, overlap=False).clone()
    recs = {r['name']: r['calibration'] for r in knet.contract_report()['layers'] if r['name'].startswith('conv')}
    formed = [n for (n, r) in recs.items() if r.get('form') == 'wino']
    print({n: (r['decided'], r.get('form'), r['gate_ratio']) for (n, r) in recs.items()})
    assert len(formed) == 12 and len(recs) == 13, recs             # every conv but conv1_1 (3 input channels)
    assert all(recs[n]['decided'] == 'mfma' and recs[n]['gate_ratio'] <= 0.25 for n in formed)
    plans = [la.op.plan(256, la.flags) for la in (c.launch(dev(), True) for (_, c) in knet._keyed(named=True)) if la is not None and la.is_conv]
    assert sum('wino_in_kernel' in p for p in plans) == 12, plans
    assert torch.equal(knet.forward_linear(xc, overlap=False), y)
    yo = knet.forward_linear(xc, overlap=True)
    assert torch.equal(yo, y), float((yo - y).abs().max())         # two 128-column windows on two streams: the same bits
    before = knet.__dict__.get('_recalibrations', 0)
    knet.forward_linear(4 * xc, overlap=False)                     # the screen trips: the layers decide again on this batch
    assert knet.__dict__.get('_recalibrations', 0) > before
    knet.exact_mode(True)
    ye = knet.forward_linear(xc, overlap=False).clone()
    g = gate(y, ye)
    print('gate of the formed forward against exact_mode(True): %.3g' % g[0])
    assert g[0] <= 1, g
    (sensor0, knet0) = _slice_net(monkeypatch, 1 << 30)            # the same net, the form never offered
    knet0.forward_linear(xc, overlap=False)                        # (the same seeds: the same keys)
    assert not any((r['calibration'] or {}).get('form') for r in knet0.contract_report()['layers'])
    knet0.exact_mode(True)
    assert torch.equal(knet0.forward_linear(xc, overlap=False), ye)
