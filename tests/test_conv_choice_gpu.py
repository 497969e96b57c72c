"""Every launch site of the matrix-core and the narrow regimes of a conv-taps handle (mfma_choice / narrow_choice, kn_conv.hip), one row each: the plan names the
site, kn_spmm_screen gives the KN_FLAG_EXACT result of the same handle -- bit for bit at the order-preserving sites, within close_conditioned at the matrix-core ones --
and the slot holds max |Y| (whether it rode in the kernel's epilogue or came from the pass over Y behind it is not told apart here; the plan is that of
kn_spmm_plan for the same call).  The expected plan texts are those of the library before the dispatch was gathered into one choice per regime.

The operators are the smallest that reach a site: 36 .. 81 pixels, 3 / 16 / 32 input and 64 / 128 output channels, nine taps.  Two sites need more: the 9 .. 32 column
kernel keeps 16 | 32 columns per block on a small layer only when its taps exceed 2 MB (256 -> 256 channels), and a 128 x 128 bf16x3 launch runs without quarter tiles
only when its work items fill whole rounds of resident workgroups (64 pixels x 12 column tiles = 96 items per XCD: one round of three workgroups on each of 32 CUs)."""
import os

import numpy as np
import pytest
import torch

import value_classes
from keynet_amd import _capi
from narrow_helpers import _spmm
from test_parity_gpu import close_conditioned, dev

pytestmark = pytest.mark.gpu

(RELU, EXACT, BF16X3, NARROW, MFMA, N32) = (_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_BF16X3, _capi.KN_FLAG_NARROW, _capi.KN_FLAG_NARROW_MFMA, _capi.KN_FLAG_NARROW32)

# name -> (Cin, Cout, H = W, entries per output pixel, float coefficients, three input pixels only)
OPS = {
    'c3-o64': (3, 64, 6, 9, False, False), 'c3-o128': (3, 128, 6, 9, False, False), 'c3-o64-slots10': (3, 64, 6, 10, False, False),
    'c3-o128-slots10': (3, 128, 6, 10, False, False), 'c16-o64': (16, 64, 6, 9, False, False), 'c16-o64-coef': (16, 64, 6, 9, True, False),
    'c16-o128': (16, 128, 6, 9, False, False), 'c16-o128-coef': (16, 128, 6, 9, True, False), 'c16-o128-h8': (16, 128, 8, 9, False, False),
    'c32-o64-slots70': (32, 64, 9, 70, False, False), 'c32-o128-slots70': (32, 128, 9, 70, False, False), 'c16-o64-dup': (16, 64, 6, 9, False, True),
    'c16-o64-dup-coef': (16, 64, 6, 9, True, True), 'c16-o64-two': (16, 64, 6, 18, False, False), 'c256-o256': (256, 256, 6, 9, False, False),
}

TILE = 'convtaps_mfma_kernel<MT=%d,NB=%d,KC=%d> loader=%s'
(GENERIC, FAST, SPTR, GROUPS) = ('generic', 'fast(per-thread pointers)', 'sptr(wave-uniform pointers)', 'sptr(wave-uniform pointers, slot groups)')
# (operator, n_vecs, ldy - n_vecs, flags, switch set when the operator is created, the launch's text in the plan, order-preserving site)
ROWS = [
    # small-K: the persistent kernel, the one-shot kernel under the switch and at two channel tiles
    ('c3-o64', 256, 0, 0, None, 'convtaps_smallk_pipe_kernel grid=', False),
    ('c3-o64', 256, 0, RELU, 'KN_NO_SMALLK_PIPE', 'convtaps_smallk_kernel grid=', False),
    ('c3-o128', 256, 0, 0, None, 'convtaps_smallk_kernel grid=', False),
    # 128 x 128 tiles at KC = 16: the four loaders; quarter tiles behind the two straight-line ones (none where the stores are not wide: ldy = n + 1)
    ('c16-o128', 128, 0, 0, None, TILE % (128, 128, 16, SPTR) + ' tail_split occ_cap=', False),
    ('c16-o128', 128, 0, RELU, 'KN_NO_SPTR', TILE % (128, 128, 16, FAST) + ' tail_split occ_cap=', False),
    ('c16-o128', 128, 1, 0, None, TILE % (128, 128, 16, SPTR) + ' occ_cap=', False),
    ('c16-o128', 128, 1, 0, 'KN_NO_SPTR', TILE % (128, 128, 16, FAST) + ' occ_cap=', False),
    ('c16-o128', 130, 0, 0, None, TILE % (128, 128, 16, GENERIC) + ' occ_cap=', False),
    ('c16-o128-coef', 128, 0, 0, None, TILE % (128, 128, 16, SPTR) + '+coef tail_split occ_cap=', False),
    ('c16-o128-coef', 128, 0, 0, 'KN_NO_SPTR', TILE % (128, 128, 16, GENERIC) + '+coef occ_cap=', False),
    ('c32-o128-slots70', 128, 0, 0, None, TILE % (128, 128, 16, GROUPS) + ' occ_cap=', False),
    # ... at KC = 4
    ('c3-o128-slots10', 128, 0, 0, None, TILE % (128, 128, 4, FAST) + ' occ_cap=', False),
    ('c3-o128-slots10', 130, 0, RELU, None, TILE % (128, 128, 4, GENERIC) + ' occ_cap=', False),
    # 64 x 256 tiles
    ('c16-o64', 256, 0, 0, None, TILE % (64, 256, 16, SPTR) + ' occ_cap=', False),
    ('c16-o64', 256, 0, RELU, 'KN_NO_SPTR', TILE % (64, 256, 16, FAST) + ' occ_cap=', False),
    ('c16-o64', 130, 0, 0, None, TILE % (64, 256, 16, GENERIC) + ' occ_cap=', False),
    ('c32-o64-slots70', 256, 0, 0, None, TILE % (64, 256, 16, GROUPS) + ' occ_cap=', False),
    ('c3-o64-slots10', 256, 0, 0, None, TILE % (64, 256, 4, FAST) + ' occ_cap=', False),
    ('c3-o64-slots10', 130, 0, 0, None, TILE % (64, 256, 4, GENERIC) + ' occ_cap=', False),
    # bf16x3 tiles
    ('c16-o64', 128, 0, BF16X3, None, 'convtaps_bf16x3_kernel<64x128, 3-way bf16 split, 6 products> grid=', False),
    ('c16-o64-coef', 128, 0, BF16X3, None, 'convtaps_bf16x3_kernel<64x128, 3-way bf16 split, 6 products>+coef grid=', False),
    ('c16-o128', 128, 0, BF16X3 | RELU, None, 'convtaps_bf16x3_kernel<128x128, 3-way bf16 split, 6 products> tail_split grid=', False),
    ('c16-o128-coef', 128, 0, BF16X3, None, 'convtaps_bf16x3_kernel<128x128, 3-way bf16 split, 6 products>+coef tail_split grid=', False),
    ('c16-o128-h8', 1536, 0, BF16X3, None, 'convtaps_bf16x3_kernel<128x128, 3-way bf16 split, 6 products> grid=', False),
    # the channel-lane kernel at every width form; stored values summed; coefficients
    ('c16-o64', 1, 0, NARROW, None, 'convtaps_narrow_kernel<1> (lane', True),
    ('c16-o64', 2, 0, NARROW | RELU, None, 'convtaps_narrow_kernel<2> (lane', True),
    ('c16-o64', 3, 0, NARROW, None, 'convtaps_narrow_kernel<4,masked to 3> (lane', True),
    ('c16-o64', 4, 0, NARROW, None, 'convtaps_narrow_kernel<4> (lane', True),
    ('c16-o64', 5, 0, NARROW | RELU, None, 'convtaps_narrow_kernel<8,masked to 5> (lane', True),
    ('c16-o64', 8, 0, NARROW, None, 'convtaps_narrow_kernel<8> (lane', True),
    ('c16-o64-dup', 3, 0, NARROW, None, 'convtaps_narrow_kernel<4,masked to 3,stored values summed> (lane', True),
    ('c16-o64-dup-coef', 8, 0, NARROW, None, 'convtaps_narrow_kernel<8,stored values summed,coef> (lane', True),
    ('c16-o64-coef', 7, 0, NARROW, None, 'convtaps_narrow_kernel<8,masked to 7,coef> (lane', True),
    # the 9 .. 32 column kernel: 8, 16 and 32 columns per block, filled and masked
    ('c16-o64', 9, 0, NARROW | N32, None, 'convtaps_narrow32_kernel<NV=8, masked to 9, 2 column blocks> (lane', True),
    ('c16-o64', 32, 0, NARROW | N32 | RELU, None, 'convtaps_narrow32_kernel<NV=8, 4 column blocks> (lane', True),
    ('c16-o64-coef', 17, 0, NARROW | N32, None, 'convtaps_narrow32_kernel<NV=8, masked to 17, 3 column blocks, coef> (lane', True),
    ('c16-o64-dup', 16, 0, NARROW | N32, None, 'convtaps_narrow32_kernel<NV=8, 2 column blocks, stored values summed> (lane', True),
    ('c16-o64-dup-coef', 13, 0, NARROW | N32, None, 'convtaps_narrow32_kernel<NV=8, masked to 13, 2 column blocks, stored values summed, coef> (lane', True),
    ('c256-o256', 32, 0, NARROW | N32, None, 'convtaps_narrow32_kernel<NV=32, 1 column block> (lane', True),
    ('c256-o256', 24, 0, NARROW | N32, None, 'convtaps_narrow32_kernel<NV=32, masked to 24, 1 column block> (lane', True),
    ('c256-o256', 16, 0, NARROW | N32, None, 'convtaps_narrow32_kernel<NV=16, 1 column block> (lane', True),
    ('c256-o256', 11, 0, NARROW | N32 | RELU, None, 'convtaps_narrow32_kernel<NV=16, masked to 11, 1 column block> (lane', True),
    # the matrix-core narrow kernel
    ('c16-o64', 1, 0, MFMA, None, 'convtaps_narrow_mfma_kernel<32 channels x 32 pixels x NV=1, K split', False),
    ('c16-o64', 3, 0, MFMA | RELU, None, 'convtaps_narrow_mfma_kernel<32 channels x 8 pixels x NV=4 masked to 3, K split', False),
    ('c16-o64', 8, 0, MFMA, None, 'convtaps_narrow_mfma_kernel<32 channels x 4 pixels x NV=8, K split', False),
    ('c16-o64', 16, 0, MFMA | N32, None, 'convtaps_narrow_mfma_kernel<32 channels x 2 pixels x NV=16, K split', False),
    ('c16-o64', 17, 0, MFMA | N32, None, 'convtaps_narrow_mfma_kernel<32 channels x 1 pixels x NV=32 masked to 17, K split', False),
    ('c16-o64-two', 2, 0, MFMA, None, 'NV=2, K split over 4 wavefronts, two slots per tap>', False),
    ('c16-o64-coef', 5, 0, MFMA, None, 'NV=8 masked to 5, K split over 4 wavefronts,coef>', False),
]

_ops = {}
_refs = {}


def _factored(name, values=None):
    """The arguments of kn_convtaps_create for the operator `name` (host arrays: tests/test_exact_sum_host.py expands them without a device)."""
    (cin, cout, hw, per_pixel, coef, dup) = OPS[name]
    rng = np.random.RandomState(len(name) + 7 * cin)
    HW = hw * hw
    eo = np.repeat(np.arange(HW), per_pixel)
    k = np.tile(np.arange(per_pixel), HW)
    ei = (eo % 3) if dup else (eo + 7 * k) % HW
    taps = rng.randn(9, cout, cin).astype(np.float32)
    ec = (rng.rand(len(eo)).astype(np.float32) + 0.5) if coef else None
    lc = np.concatenate((rng.randn(cout * HW), [1.0])).astype(np.float32)
    (taps, ec, lc) = value_classes.conv_values(values, taps, ec, lc, per_pixel * cin)
    return ((cin, hw, hw), (cout, hw, hw), taps, eo.astype(np.int32), ei.astype(np.int32), (k % 9).astype(np.int32), ec, lc)


def _operator(name, switch, values=None):
    """(handle, (shape, indptr, indices, data) of its expansion), created once per (operator, switch): the environment is read when a handle is created.
    `values`: a variant of value_classes.conv_values -- the same operator with its values scaled by powers of two (tests/test_value_classes_gpu.py)."""
    if (name, switch, values) not in _ops:
        (inshape, outshape, taps, eo, ei, et, ec, lc) = _factored(name, values)
        if switch:
            os.environ[switch] = '1'
        try:
            with torch.cuda.device(dev()):
                op = _capi.Operator.convtaps(inshape, outshape, taps, eo, ei, et, ec, lc)
        finally:
            if switch:
                del os.environ[switch]
        (ip, ix, dt) = op.export_csr()
        _ops[(name, switch, values)] = (op, (op.shape(), ip, ix, dt))
    return _ops[(name, switch, values)]


def _reference(name, n):
    """(X [n, cols] on the host, X [cols, n] on the device, the KN_FLAG_EXACT result of the default handle), computed once per (operator, batch)."""
    if (name, n) not in _refs:
        (op, csr) = _operator(name, None)
        X = np.random.RandomState(n).randn(n, csr[0][1]).astype(np.float32)
        X[:, -1] = 1.0
        xd = torch.as_tensor(np.ascontiguousarray(X.T)).to(dev())
        _refs[(name, n)] = (X, xd, _spmm(op, xd, n, EXACT)[0].clone())
    return _refs[(name, n)]


@pytest.mark.parametrize('row', ROWS, ids=['%s-n%d%s-f%d%s' % (r[0], r[1], '-ldy+%d' % r[2] if r[2] else '', r[3], '-' + r[4] if r[4] else '') for r in ROWS])
def test_launch_site(row):
    (name, n, pad, flags, switch, text, exact_bits) = row
    (op, csr) = _operator(name, switch)
    (X, xd, ref) = _reference(name, n)
    if flags & RELU:
        ref = torch.relu(ref)
    slot = torch.zeros(1, dtype=torch.float32, device=dev())
    (y, whole, plan) = _spmm(op, xd, n, flags, ld=n + pad, absmax=slot)
    print(plan)
    assert text in plan, plan
    torch.cuda.synchronize()
    d = float((y - ref).abs().max())
    print('max |y - exact| = %.3g, max |y| = %.6g, slot = %.6g' % (d, float(y.abs().max()), float(slot)))
    if exact_bits:
        assert torch.equal(y, ref), d
    else:
        assert close_conditioned(y.cpu().numpy().T, ref.cpu().numpy().astype(np.float64).T, csr, X), d
    assert float(slot) == float(y.abs().max())
    if pad:
        assert bool((whole[:, n:] == 7.5).all())          # the columns beyond the batch keep narrow_helpers.SENTINEL
