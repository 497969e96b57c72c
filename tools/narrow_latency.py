#!/usr/bin/env python
"""Latency of the low-latency (narrow) forward against the padded forward, on ONE key-net in ONE process.

    python tools/narrow_latency.py [--workload vgg16|allconv] [--forwards 20] [--warmup 3] [--out profiles/r07_narrow_forward.txt]
    python tools/narrow_latency.py --one-forward [-n 1]        # keys, warms up, then runs ONE narrow forward: the program for a kernel trace
                                                               # (rocprofv3 --kernel-trace --stats -- python tools/narrow_latency.py --one-forward)

Keys the headline workload (benchlegs.workloads: TiledPermutationKeynet VGG-16, tile 64, default contract; `--workload allconv`: the untiled PermutationKeynet
AllConvNet, whose conv layers are factored stand-ins) and, for n in (1, 2, 4, 8) images, times three forwards of the SAME images on that key-net:
forward_linear(x) (padded to 128 images: the code path of every earlier release), forward_linear(x, narrow=True) eager, and the replay of
capture(x, narrow=True).  HIP events around each forward, a warm-up, the median over --forwards forwards (min and max beside it).  The narrow logits must be
torch.equal to the padded ones before any time is printed.  Prints one table and appends it to --out."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                                      # noqa: E402
from benchlegs import workloads                   # noqa: E402


def timed(fn, forwards, warmup):
    """[ms] of `forwards` calls of fn(), each between two HIP events on the current stream, after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(forwards):
        (a, b) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='vgg16', choices=['vgg16', 'allconv'])
    ap.add_argument('--forwards', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r07_narrow_forward.txt'))
    ap.add_argument('--one-forward', action='store_true', help='key, warm up, run one narrow forward and exit (for a kernel trace)')
    ap.add_argument('-n', type=int, default=1, help='images of --one-forward')
    args = ap.parse_args()
    assert args.forwards >= 20 or args.one_forward, 'the median of at least 20 forwards'
    t0 = time.time()
    (sensor, knet, inshape, _, desc, _) = workloads.build_workload(args.workload, 0, fanout=True)
    dev = torch.device('cuda:0')
    torch.manual_seed(1)
    imgs = torch.randn((8,) + tuple(inshape))
    xc = sensor.fromtensor(imgs.to(dev)).encrypt().astensor()
    xc = xc.t().contiguous().t()                  # feature-major, as the layers hand blocks on
    print('keyed %s in %.0f s' % (desc, time.time() - t0), flush=True)
    if args.one_forward:
        x = xc[:args.n].t().contiguous().t()
        knet.forward_linear(x, narrow=True)       # operators resident
        torch.cuda.synchronize()
        print('TRACE-FROM-HERE: one narrow forward of %d image(s) follows' % args.n, flush=True)
        knet.forward_linear(x, narrow=True)
        torch.cuda.synchronize()
        return
    rows = []
    pads0 = getattr(knet, '_padded_forwards', 0)
    for n in (1, 2, 4, 8):
        x = xc[:n].t().contiguous().t()
        padded = knet.forward_linear(x)
        narrow = knet.forward_linear(x, narrow=True)
        replay = knet.capture(x, narrow=True)
        graph = replay(x).clone()
        torch.cuda.synchronize()
        assert torch.equal(narrow, padded), 'narrow logits differ from the padded forward at %d image(s): max %g' % (n, float((narrow - padded).abs().max()))
        assert torch.equal(graph, narrow), 'replayed narrow logits differ from the eager ones at %d image(s)' % n
        t = [timed(lambda: knet.forward_linear(x), args.forwards, args.warmup),
             timed(lambda: knet.forward_linear(x, narrow=True), args.forwards, args.warmup),
             timed(lambda: replay(x), args.forwards, args.warmup)]
        rows.append((n, [(statistics.median(v), min(v), max(v)) for v in t]))
        print('n = %d done' % n, flush=True)
    # an untiled key-net (allconv) is not padded by forward_linear: its first column is the plain forward at n columns
    base = 'padded forward_linear [ms]' if getattr(knet, '_padded_forwards', 0) > pads0 else 'forward_linear, unpadded [ms]'
    lines = ['', '== tools/narrow_latency.py --workload %s: %s' % (args.workload, desc),
             '   %s, torch %s; HIP events, %d warm-up + median of %d forwards (min .. max); narrow and replayed logits torch.equal to forward_linear(x): yes'
             % (torch.cuda.get_device_name(0), torch.__version__, args.warmup, args.forwards),
             '   %6s | %-28s | %-28s | %-28s | %s' % ('images', base, 'narrow=True eager [ms]', 'capture(narrow=True) replay', 'first / narrow, / replay')]
    for (n, t) in rows:
        cell = ['%8.3f (%.3f .. %.3f)' % v for v in t]
        lines.append('   %6d | %-28s | %-28s | %-28s | %.2fx, %.2fx' % (n, cell[0], cell[1], cell[2], t[0][0] / t[1][0], t[0][0] / t[2][0]))
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out, 'a') as f:
        f.write(text)


if __name__ == '__main__':
    main()
