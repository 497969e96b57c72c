"""KN_MODIFIER_WINO per layer: every 3 x 3 conv shape of keyed VGG-16 from conv2_2 on (pixel-permutation key, bias column, ReLU) at 128 and 256 columns, the plain matrix-core
call against the call with the flag -- same process, same operands, interleaved A-B-A-B behind one warm launch of each, every launch between two events.

    python tools/wino_layer_ab.py [--reps 7] [--out profiles/wino_layer_ab.txt]

One line per (shape, width): the times of every repetition, whether the form won in EVERY repetition (what wino_offered of keynet_amd/sparse.py may offer), the gate of the
form's result against KN_FLAG_EXACT on these operands, and the plan of the form.  The three launches of the form are not separated by events (they are one kn_spmm); their
split comes from a kernel trace of this tool (rocprofv3 --kernel-trace --stats -- python tools/wino_layer_ab.py --reps 1)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from keynet_amd import _capi                                  # noqa: E402
from keynet_amd import direct as kdirect                      # noqa: E402
from keynet_amd.layer import gate                             # noqa: E402

SHAPES = [('conv2_2', 128, 128, 112), ('conv3_1', 128, 256, 56), ('conv3_2', 256, 256, 56), ('conv4_1', 256, 512, 28), ('conv4_2', 512, 512, 28), ('conv5_1', 512, 512, 14)]
(RELU, EXACT, WINO) = (_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_MODIFIER_WINO)


def operator(cin, cout, hw, rng):
    HW = hw * hw
    (po, pi) = (rng.permutation(HW), rng.permutation(HW))
    (eo, ei, et) = ([], [], [])
    for (t, (_, S)) in enumerate(kdirect.shift_matrices((hw, hw), 3, 1)):
        S = S.tocoo()
        eo.append(po[S.row]); ei.append(pi[S.col]); et.append(np.full(S.nnz, t))
    (eo, ei, et) = (np.concatenate(a).astype(np.int32) for a in (eo, ei, et))
    taps = (rng.randn(9, cout, cin) / np.sqrt(9 * cin)).astype(np.float32)
    lastcol = np.concatenate((0.1 * rng.randn(cout * HW), [1.0])).astype(np.float32)
    return _capi.Operator.convtaps((cin, hw, hw), (cout, hw, hw), taps, eo, ei, et, None, lastcol)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    ap.add_argument('--widths', default='128,256')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    rng = np.random.RandomState(0)
    stream = torch.cuda.current_stream().cuda_stream
    lines = ['# %s, %d repetitions, times in ms (flag off | flag on), flops = 2 * 9 * Cin * Cout * interior-and-edge slots' % (torch.cuda.get_device_name(0), args.reps)]
    for (name, cin, cout, hw) in SHAPES:
        op = operator(cin, cout, hw, rng)
        (ok, why) = op.wino_status()
        (rows, cols) = op.shape()
        for n in [int(w) for w in args.widths.split(',')]:
            x = torch.rand(cols, n, device=dev) * 2 - 1
            x[-1] = 1.0
            (y0, y1) = (torch.empty(rows, n, device=dev), torch.empty(rows, n, device=dev))

            def call(y, flags):
                op.spmm(x.data_ptr(), n, n, y.data_ptr(), n, flags, stream)

            call(y0, RELU)
            call(y1, RELU | WINO)
            torch.cuda.synchronize()
            (t_off, t_on) = ([], [])
            for _ in range(args.reps):
                for (y, flags, ts) in ((y0, RELU, t_off), (y1, RELU | WINO, t_on)):
                    (a, b) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                    a.record()
                    call(y, flags)
                    b.record()
                    b.synchronize()
                    ts.append(a.elapsed_time(b))
            ye = torch.empty(rows, n, device=dev)
            call(ye, RELU | EXACT)
            torch.cuda.synchronize()
            (g1, g0) = (gate(y1, ye)[0], gate(y0, ye)[0])
            wins = all(b < a for (a, b) in zip(t_off, t_on))
            flops = 2.0 * op.nnz_expanded() * n
            lines.append('%s Cin=%d Cout=%d %dx%d n=%d: off median %.3f (%.1f TF/s) on median %.3f (%.1f TF/s effective) ratio %.3f won_every_rep=%s eligible=%s gate on %.3g off %.3g' % (
                name, cin, cout, hw, hw, n, float(np.median(t_off)), flops / np.median(t_off) / 1e9, float(np.median(t_on)), flops / np.median(t_on) / 1e9,
                float(np.median(t_off) / np.median(t_on)), wins, ok if ok else why, g1, g0))
            lines.append('    off ' + ' '.join('%.3f' % t for t in t_off))
            lines.append('    on  ' + ' '.join('%.3f' % t for t in t_on))
            lines.append('    plan ' + op.plan(n, RELU | WINO))
            print('\n'.join(lines[-4:]), flush=True)
            del x, y0, y1, ye
        del op
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
