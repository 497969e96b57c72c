"""Tile-height A/B of the 64-column f32 tiles (KN_FLAG_NARROW64_MFMA, mfma64_choice in kn_conv.hip) on VGG-16-shaped conv-taps operators with permuted pixels:
one kn_spmm at 64 aligned columns per tile height 256 | 128 | 64, the rule's own choice, and the plain 128-column launch of the same columns zero-padded (HIP events, median
of 30 launches).  Needs the DIAGNOSTIC build, which reads KN_MFMA64_MT when a handle is created and alone holds the 256 x 64 tile (profiles/r12_narrow64_mfma.txt, section 3):

    python -c "from keynet_amd import build; build.build(out='tools/scratch/libkeynet_hip_abl.so', defines=('KN_ABLATION',))"
    KEYNET_HIP_LIB=$PWD/tools/scratch/libkeynet_hip_abl.so python tools/mfma64_tile_ab.py
"""
import os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from keynet_amd import _capi, sparse as ksp, direct as kdirect

F = _capi.KN_FLAG_NARROW_MFMA | _capi.KN_FLAG_NARROW32 | _capi.KN_FLAG_NARROW64 | _capi.KN_FLAG_NARROW64_MFMA | _capi.KN_FLAG_RELU
dev = torch.device('cuda:0')


def operator(rng, Cin, Cout, H):
    w = (rng.randn(Cout, Cin, 3, 3) / np.sqrt(9 * Cin)).astype(np.float32)
    (pi, po) = (rng.permutation(H * H), rng.permutation(H * H))
    (eo, ei, et) = ([], [], [])
    for (t, ((i, j), S)) in enumerate(kdirect.shift_matrices((H, H), 3, 1)):
        S = S.tocoo()
        eo.append(po[S.row]); ei.append(pi[S.col]); et.append(np.full(S.nnz, t))
    taps = np.stack([w[:, :, i, j] for i in range(3) for j in range(3)])
    lastcol = np.concatenate((rng.randn(Cout * H * H), [1.0])).astype(np.float32)
    return ksp.Conv2dTiledMatrix.fromtaps((Cin, H, H), (Cout, H, H), taps, np.concatenate(eo), np.concatenate(ei), np.concatenate(et), None, lastcol)


def timed(fn, n=30, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        (a, b) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        a.record(); fn(); b.record(); b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out)


rng = np.random.RandomState(0)
print('layer (Cin, Cout, HxH) | workgroups at MT=256 / 128 / 64 | us at MT=256 | 128 | 64 | the rule takes | padded 128-column launch [us]')
for (name, Cin, Cout, H) in (('conv3_1', 128, 256, 56), ('conv3_2', 256, 256, 56), ('conv4_1', 256, 512, 28), ('conv4_2', 512, 512, 28), ('conv5_1', 512, 512, 14)):
    W = operator(rng, Cin, Cout, H)
    x = torch.randn((W.shape[1], 64), device=dev)
    x[-1] = 1.0
    xp = torch.zeros((W.shape[1], 128), device=dev)
    xp[:, :64] = x
    y = torch.empty((W.shape[0], 128), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    res = {}
    for mt in (0, 256, 128, 64):
        os.environ['KN_MFMA64_MT'] = str(mt)
        W._op = None
        with torch.cuda.device(dev):
            op = W._device_op(dev)
            plan = op.plan(64, F)
            res[mt] = (timed(lambda: op.spmm(x.data_ptr(), 64, 64, y.data_ptr(), 64, F, st)), plan.split(' loader')[0])
            if mt == 0:
                wide = timed(lambda: op.spmm(xp.data_ptr(), 128, 128, y.data_ptr(), 128, _capi.KN_FLAG_RELU, st))
    n_pix = H * H
    print('%s (%d, %d, %dx%d) | %d / %d / %d | %.1f | %.1f | %.1f | %s %.1f | %.1f' % (name, Cin, Cout, H, H, n_pix * Cout // 256, n_pix * Cout // 128, n_pix * Cout // 64,
          res[256][0], res[128][0], res[64][0], res[0][1], res[0][0], wide), flush=True)
