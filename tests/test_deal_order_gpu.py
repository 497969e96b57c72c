"""The dealing order of the matrix-core conv-taps kernels on the GPU (ConvTapsDev::pix_deal, kn_deal.h): a handle created with KN_NO_DEAL=1 walks the locality order
itself, a handle created without it the slot-balanced, heavy-first order.  Every output element keeps its K order, so the two give the same bits -- with and without
KN_FLAG_RELU, the same max |Y| in the slot, and the same plan apart from the opts{...} suffix.  One handle is held against the CPU oracle inside close_conditioned (the gate
of the conv tests of test_parity_gpu.py) and against its own KN_FLAG_EXACT result inside the float-key gate.  KN_FLAG_EXACT itself takes the untouched order either way.

The operators are keyed 3x3 / pad-1 convs (9 / 6 / 4 slots per interior / edge / corner pixel) under a pixel permutation, Cin = Cout.  The oracle runs on the expansion of
16 of the output channels (the first and the last eight of the first channel tile, every pixel, every column): the order decides which PIXEL a workgroup computes, and the
expansion of all 128 channels (26 M stored values) would take the test out of its few seconds."""
import os

import numpy as np
import pytest
import torch

from keynet_amd import _capi
from keynet_amd import direct as kdirect
from keynet_amd import sparse as ksp
from keynet_amd.layer import gate
from narrow_helpers import _spmm
from test_narrow_gpu import _oracle, _sorted_csr
from test_parity_gpu import close_conditioned, dev

pytestmark = pytest.mark.gpu

(RELU, EXACT, MFMA, N32, N64, N64M) = (_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_NARROW_MFMA, _capi.KN_FLAG_NARROW32, _capi.KN_FLAG_NARROW64, _capi.KN_FLAG_NARROW64_MFMA)
TILE64 = MFMA | N32 | N64 | N64M

# operator -> (channels, H, W, gain key)
OPS = {'14x14-c128': (128, 14, 14, False), '5x5-c128': (128, 5, 5, False), '9x7-c64': (64, 9, 7, False), '14x14-c128-gain': (128, 14, 14, True),
       '14x14-c16-o512': (16, 14, 14, False)}
# (operator, columns, flags, what the plan names).  14 x 14 x 128 channels: 196 (392 at 256 columns) work items, 25 (49) per XCD -- less than one round of resident
# workgroups, so every item runs as quarter tiles; 5 x 5: 25 items, 4 per XCD and 3 on the last; 9 x 7 x 64 channels: the 64 x 256 tile; the gain key: the coefficient
# loaders; 64 columns under KN_FLAG_NARROW64_MFMA: the 64-column tile.  The last row (16 -> 512 channels, 4 channel tiles x 2 column tiles: 196 items per XCD) has
# whole tiles AND quarter tiles in one launch; it is compared between the handles and with KN_FLAG_EXACT only.
ROWS = [
    ('14x14-c128', 128, 0, 'convtaps_mfma_kernel<MT=128,NB=128,KC=16> loader=sptr(wave-uniform pointers) tail_split', True),
    ('14x14-c128', 256, 0, 'convtaps_mfma_kernel<MT=128,NB=128,KC=16> loader=sptr(wave-uniform pointers) tail_split', True),
    ('5x5-c128', 128, 0, 'convtaps_mfma_kernel<MT=128,NB=128,KC=16> loader=sptr(wave-uniform pointers) tail_split', True),
    ('9x7-c64', 256, 0, 'convtaps_mfma_kernel<MT=64,NB=256,KC=16> loader=sptr(wave-uniform pointers) occ_cap', True),
    ('14x14-c128-gain', 128, 0, 'convtaps_mfma_kernel<MT=128,NB=128,KC=16> loader=sptr(wave-uniform pointers)+coef tail_split', True),
    ('14x14-c128', 64, TILE64, 'convtaps_mfma_kernel<MT=64,NB=64,KC=16> loader=sptr(wave-uniform pointers) occ_cap', True),
    ('14x14-c16-o512', 256, 0, 'convtaps_mfma_kernel<MT=128,NB=128,KC=16> loader=sptr(wave-uniform pointers) tail_split', False),
]
SUFFIX = ' opts{no_deal=1}'
N_MAX = 256

_ops = {}


def _operator(name):
    """(handle with the dealing order, handle created under KN_NO_DEAL=1, X [cols, 256] on host and device, (oracle rows, CSR of those rows) or None) -- built once, left
    unchanged."""
    if name not in _ops:
        (C, H, W, gain) = OPS[name]
        (cin, cout) = (C, 512) if name.endswith('o512') else (C, C)
        rng = np.random.RandomState(sum(map(ord, name)))
        HW = H * W
        taps = (rng.randn(9, cout, cin) / np.sqrt(9 * cin)).astype(np.float32)
        (pi, po) = (rng.permutation(HW), rng.permutation(HW))
        (eo, ei, et) = ([], [], [])
        for (t, (_, S)) in enumerate(kdirect.shift_matrices((H, W), 3, 1)):
            S = S.tocoo()
            eo.append(po[S.row]); ei.append(pi[S.col]); et.append(np.full(S.nnz, t))
        (eo, ei, et) = (np.concatenate(eo).astype(np.int32), np.concatenate(ei).astype(np.int32), np.concatenate(et).astype(np.int32))
        assert sorted(set(np.bincount(eo).tolist())) == [4, 6, 9]
        ec = None
        if gain:                                              # every entry carries a_out[o] / a_in[i]
            (a_out, a_in) = (rng.rand(HW) + 0.5, rng.rand(HW) + 0.5)
            ec = (a_out[eo] / a_in[ei]).astype(np.float32)
        lastcol = np.concatenate((rng.randn(cout * HW), [1.0])).astype(np.float32)
        handles = []
        for switch in (None, '1'):
            assert 'KN_NO_DEAL' not in os.environ
            if switch:
                os.environ['KN_NO_DEAL'] = switch
            try:
                with torch.cuda.device(dev()):
                    handles.append(_capi.Operator.convtaps((cin, H, W), (cout, H, W), taps, eo, ei, et, ec, lastcol))
            finally:
                os.environ.pop('KN_NO_DEAL', None)
        X = rng.randn(cin * HW + 1, N_MAX).astype(np.float32)
        X[-1] = 1.0
        sub = None
        if cout == C:
            sel = np.concatenate((np.arange(8), np.arange(min(cout, 128) - 8, min(cout, 128))))
            rows = np.concatenate(((sel[:, None] * HW + np.arange(HW)).ravel(), [cout * HW]))
            Wsub = ksp.Conv2dTiledMatrix.fromtaps((cin, H, W), (len(sel), H, W), taps[:, sel, :], eo, ei, et, ec, lastcol[rows])
            sub = (torch.as_tensor(rows).to(dev()), _sorted_csr(Wsub))
        _ops[name] = (handles[0], handles[1], X, torch.as_tensor(X).to(dev()), sub)
    return _ops[name]


@pytest.mark.parametrize('row', ROWS, ids=['%s-n%d%s' % (r[0], r[1], '-tile64' if r[2] else '') for r in ROWS])
def test_dealt_and_undealt_handles_give_the_same_bits(row):
    (name, n, flags, text, with_oracle) = row
    (op, op_nodeal, X, xd_all, sub) = _operator(name)
    xd = xd_all[:, :n].contiguous()
    ye = _spmm(op, xd, n, EXACT)[0]
    for relu in (0, RELU):
        (s1, s0) = (torch.zeros(1, dtype=torch.float32, device=dev()), torch.zeros(1, dtype=torch.float32, device=dev()))
        (y1, _, p1) = _spmm(op, xd, n, flags | relu, absmax=s1)
        (y0, _, p0) = _spmm(op_nodeal, xd, n, flags | relu, absmax=s0)
        print(p1)
        assert text in p1 and 'opts{' not in p1, p1
        assert p0 == p1 + SUFFIX, (p0, p1)
        assert torch.equal(y1, y0), (name, n, relu, float((y1 - y0).abs().max()))
        assert float(s1) == float(s0) == float(y1.abs().max())
        g = gate(y1, torch.relu(ye) if relu else ye)
        print('relu=%d: gate against KN_FLAG_EXACT %.3g' % (relu, g[0]))
        assert g[0] <= 1, (name, n, relu, g)
        if with_oracle:
            (rows, M) = sub
            ref = _oracle(M, X[:, :n])
            if relu:
                ref = np.maximum(ref, 0)
            assert close_conditioned(y1[rows].cpu().numpy().T, ref.astype(np.float64).T, (M.shape, M.indptr, M.indices, M.data), X[:, :n].T), (name, n, relu)


def test_order_preserving_calls_take_the_untouched_order():
    """KN_FLAG_EXACT on the 14 x 14 operator: an order-preserving kernel in both plans, the same bits from both handles, and the oracle's bits on the oracle's rows."""
    (op, op_nodeal, X, xd_all, (rows, M)) = _operator('14x14-c128')
    xd = xd_all[:, :128].contiguous()
    for relu in (0, RELU):
        (y1, _, p1) = _spmm(op, xd, 128, EXACT | relu)
        (y0, _, p0) = _spmm(op_nodeal, xd, 128, EXACT | relu)
        assert 'convtaps_exact' in p1 and 'convtaps_mfma_kernel' not in p1 and p0 == p1 + SUFFIX, (p0, p1)
        assert torch.equal(y1, y0)
        ref = _oracle(M, X[:, :128])
        assert np.array_equal(y1[rows].cpu().numpy(), np.maximum(ref, 0) if relu else ref)
