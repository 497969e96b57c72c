#!/usr/bin/env python
"""The egress of frames next to the torch composition it replaces: one block of decrypted-like activations [n, C*H*W+1] in HBM, one process, four legs

  kernel         ktorch.linear_to_frames(x, inshape)                                   one launch of kn_linear_to_u8, unit gain
  torch          linear_to_affine, round, clamp, to(uint8), permute(0, 2, 3, 1).contiguous()          what a caller writes today for decrypted frames
  range+kernel   ktorch.column_range, ktorch.gray_affine, ktorch.linear_to_frames(gain, bias)          KeyedSensor.asframes on a loaded block
  range+torch    linear_to_affine, amin / amax per image, gray_affine, mul, add, round, clamp, to(uint8), permute(...).contiguous()

Calls rotate over `--blocks` distinct blocks (default 3: 462 MB at the default shape, more than the 256 MiB Infinity Cache holds, so a call reads its block from HBM).
Legs are alternated `--repeats` times after `--warmup` untimed rounds; a timed run is `--iters` calls between two device events on the current stream (linear_to_affine's host
read of the homogeneous check is inside the torch legs: it is part of what the caller runs).  Per leg the median, minimum and maximum of ms per call, and the rate
over the bytes the conversion needs (4 B read + 1 B written per element; the range legs 4 B more per element).  The frames of the two legs of a pair are compared,
byte for byte.  Verdict per pair: the kernel leg is `not slower` when its median is at most the torch leg's plus the two spreads (max - min) added.  Every GPU step
runs under a time limit of its own.  Prints one JSON record (and writes it to --out).

    python tools/egress_rate.py --shape 3,224,224 --batch 256 --out profiles/r20_sensor_egress.txt
"""
import argparse
import faulthandler
import json
import os
import statistics
import sys
from contextlib import contextmanager

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@contextmanager
def limit(seconds, what):
    """A GPU step under its own time limit: past it the traceback is dumped and the process exits."""
    sys.stderr.write('[egress_rate] %s (limit %d s)\n' % (what, seconds))
    sys.stderr.flush()
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--shape', default='3,224,224', help='C,H,W of a frame (default: the VGG-16 frame)')
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--blocks', type=int, default=3, help='distinct input blocks the calls rotate over')
    ap.add_argument('--iters', type=int, default=12, help='calls per timed run')
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--step-limit', type=int, default=120, help='seconds a single GPU step may take')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    from keynet_amd import torch as ktorch

    assert torch.cuda.is_available(), 'egress_rate.py needs an MI355X'
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    (C, H, W) = (int(v) for v in args.shape.split(','))
    (n, D) = (args.batch, C * H * W)

    with limit(args.step_limit, 'the block: ingested random frames plus a decrypt-like error below one half'):
        g = torch.Generator(device=dev).manual_seed(1234)
        (frames_all, xs) = ([], [])
        for _ in range(args.blocks):
            frames_all.append(torch.randint(0, 256, (n, H, W, C), generator=g, device=dev, dtype=torch.uint8))
            xs.append(ktorch.frames_to_linear(frames_all[-1]))
            xs[-1].t()[:D] += (torch.rand((D, n), generator=g, device=dev) - 0.5) * 0.8
        torch.cuda.synchronize()
    (frames, x) = (frames_all[0], xs[0])

    def kernel(x=x):
        return ktorch.linear_to_frames(x, (C, H, W))

    def torch_leg(x=x):
        a = ktorch.linear_to_affine(x, (n, C, H, W))
        return a.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    def range_kernel(x=x):
        (gain, bias) = ktorch.gray_affine(*ktorch.column_range(x))
        return ktorch.linear_to_frames(x, (C, H, W), gain=gain, bias=bias)

    def range_torch(x=x):
        a = ktorch.linear_to_affine(x, (n, C, H, W))
        flat = a.reshape(n, D)
        (gain, bias) = ktorch.gray_affine(flat.amin(dim=1), flat.amax(dim=1))
        t = a.mul(gain.reshape(n, 1, 1, 1)).add(bias.reshape(n, 1, 1, 1))
        return t.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    legs = [('kernel', kernel), ('torch', torch_leg), ('range+kernel', range_kernel), ('range+torch', range_torch)]
    first = {}
    for w in range(args.warmup):
        for (name, leg) in legs:
            with limit(args.step_limit, 'warm-up %d of %s' % (w, name)):
                y = leg()
                torch.cuda.synchronize()
                first.setdefault(name, y)
    equal = {'kernel == torch': bool(torch.equal(first['kernel'], first['torch'])), 'range+kernel == range+torch': bool(torch.equal(first['range+kernel'], first['range+torch'])),
             'kernel == the ingested frames': bool(torch.equal(first['kernel'], frames))}
    first.clear()

    ms = {name: [] for (name, _) in legs}
    for r in range(args.repeats):
        for (name, leg) in legs:
            with limit(args.step_limit, 'repeat %d of %s' % (r, name)):
                (e0, e1) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                torch.cuda.synchronize()
                e0.record()
                for i in range(args.iters):
                    leg(xs[i % len(xs)])
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1) / args.iters)

    need = {'kernel': 5 * n * D, 'torch': 5 * n * D, 'range+kernel': 9 * n * D, 'range+torch': 9 * n * D}
    rec = {}
    for (name, v) in ms.items():
        med = statistics.median(v)
        rec[name] = {'ms_per_call': {'median': med, 'min': min(v), 'max': max(v), 'spread': max(v) - min(v), 'runs': v}, 'needed_bytes': need[name],
                     'GB_per_s_over_needed_bytes': need[name] / med / 1e6}
    verdict = {}
    for (k, t) in (('kernel', 'torch'), ('range+kernel', 'range+torch')):
        margin = rec[k]['ms_per_call']['spread'] + rec[t]['ms_per_call']['spread']
        (mk, mt) = (rec[k]['ms_per_call']['median'], rec[t]['ms_per_call']['median'])
        verdict['%s vs %s' % (k, t)] = {'margin_ms': margin, 'torch_over_kernel': mt / mk, 'verdict': 'not slower' if mk <= mt + margin else 'SLOWER'}
    out = {'tool': 'tools/egress_rate.py', 'device': torch.cuda.get_device_name(dev), 'shape': [C, H, W], 'batch': n, 'block_MB': 4e-6 * (D + 1) * n, 'blocks': args.blocks, 'iters_per_run': args.iters,
           'repeats': args.repeats, 'warmup': args.warmup, 'legs': rec, 'frames_equal': equal, 'verdict': verdict,
           'what': 'device events around `iters` calls on the current stream, legs alternated; the torch legs include the host read of linear_to_affine\'s homogeneous check'}
    print(json.dumps(out))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
