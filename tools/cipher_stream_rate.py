#!/usr/bin/env python
"""What a server that receives ENCRYPTED frames gets, next to the pipeline that simulates the sensor: one key-net, one batch size, one process, four legs

  resident           knet.forward_linear(x_cipher) on an encrypted batch that sits in HBM -- the loop bench.py times, the yardstick
  streamed uint8     keynet_amd.stream.StreamedForward(frames='uint8'): plaintext host frames, upload, ingest, the SENSOR's keyed product, forward, read-back
  streamed cipher8   StreamedForward(None, knet, frames='cipher8'): 8-bit encrypted host frames with their ranges, upload, dequantising ingest, forward, read-back --
                     the same bytes as 'streamed uint8', no sensor product
  streamed cipher16  the same from 16-bit encrypted frames (twice the bytes)

alternated `--repeats` times after one warm-up each; per leg the median, minimum and maximum of ms per batch and images/s.  The encrypted frames are made once by
KeyedSensor.encrypt_to_frames from the plaintext frames of the 'uint8' leg; under a permutation image key with range=(0, 255) the 'cipher8' logits are those of the
'uint8' leg, bit for bit (reported).  Next to the legs: microseconds per call of the two new kernels and of their 8-bit neighbours on the same blocks (device events
around `--kernel-calls` back-to-back launches, repeated) --

  kn_u8_to_linear       kn_frames_to_linear at 8 bits (scale and offset given)       kn_frames_to_linear at 16 bits
  kn_linear_to_u8       kn_linear_to_u16

Every GPU step runs under a time limit of its own: a step that overruns it ends the process.  Prints one JSON record (and writes it to --out).

    python tools/cipher_stream_rate.py --workload vgg16 --batch 256 --batches 8 --repeats 5 --out profiles/rNN_cipher_frames.txt
"""
import argparse
import faulthandler
import json
import os
import statistics
import sys
import time
from contextlib import contextmanager

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@contextmanager
def limit(seconds, what):
    """A GPU step under its own time limit: past it the traceback is dumped and the process exits (a watchdog of faulthandler: it fires inside a blocked HIP call too)."""
    sys.stderr.write('[cipher_stream_rate] %s (limit %d s)\n' % (what, seconds))
    sys.stderr.flush()
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def spread(ms, images):
    med = statistics.median(ms)
    return {'ms_per_batch': {'median': med, 'min': min(ms), 'max': max(ms), 'runs': ms}, 'images_per_s': {'median': 1e3 * images / med, 'min': 1e3 * images / max(ms), 'max': 1e3 * images / min(ms)}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--workload', default='vgg16')
    ap.add_argument('--batch', type=int, default=None, help='images per batch (default: the workload\'s)')
    ap.add_argument('--batches', type=int, default=8, help='batches per timed run')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--kernel-calls', type=int, default=20, help='back-to-back launches per kernel timing')
    ap.add_argument('--exact', default=None, choices=['auto', 'true', 'false'], help='the contract the key-net is built under (default: bench.py\'s -- auto for the vgg16 workloads)')
    ap.add_argument('--step-limit', type=int, default=240, help='seconds a single GPU step may take')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from benchlegs.workloads import build_workload, upload_operators
    from keynet_amd import torch as ktorch
    from keynet_amd.stream import StreamedForward

    dev = torch.device('cuda', 0)
    exact = {'auto': 'auto', 'true': True, 'false': False, None: 'auto' if args.workload.startswith('vgg16') else None}[args.exact]
    (sensor, knet, inshape, batch, desc, _) = build_workload(args.workload, 0, exact=exact, fanout=True, prepare=upload_operators(dev))
    assert torch.cuda.is_available(), 'cipher_stream_rate.py needs an MI355X'    # (after the keying: its forked processes start before this one touches the GPU)
    torch.cuda.set_device(dev)
    batch = args.batch or batch
    (C, H, W) = inshape
    rng = np.random.RandomState(1234)
    frames = [torch.as_tensor(rng.randint(0, 256, size=(batch, H, W, C)).astype(np.uint8)) for _ in range(min(4, args.batches))]
    items_u8 = [frames[k % len(frames)] for k in range(args.batches)]
    sf = {'streamed uint8': StreamedForward(sensor, knet, batch, layout='NHWC', frames='uint8'),
          'streamed cipher8': StreamedForward(None, knet, batch, layout='NHWC', frames='cipher8'),
          'streamed cipher16': StreamedForward(None, knet, batch, layout='NHWC', frames='cipher16')}
    pad_to = sf['streamed uint8']._pad_to
    images = batch * args.batches

    with limit(args.step_limit, 'upload of the frames, first forward (operators resident, contracts decided), the encrypted frames'):
        frames_dev = frames[0].to(dev)
        x_cipher = sensor.encrypt_frames(frames_dev, pad_to=pad_to)
        y0 = knet.forward_linear(x_cipher)[:batch].cpu()
        cipher = {8: [], 16: []}
        for f in frames:                                                 # 8 bits: the encrypted block's own bytes; 16 bits: the same integers over (0, 65535)
            cipher[8].append(tuple(v.cpu() for v in sensor.encrypt_to_frames(f.to(dev), depth=8, range=(0, 255))))
            cipher[16].append(tuple(v.cpu() for v in sensor.encrypt_to_frames(f.to(dev), depth=16, range=(0, 65535))))
        torch.cuda.synchronize()
    items = {'streamed uint8': items_u8, 'streamed cipher8': [cipher[8][k % len(frames)] for k in range(args.batches)],
             'streamed cipher16': [cipher[16][k % len(frames)] for k in range(args.batches)]}

    def resident():
        for _ in range(args.batches):
            y = knet.forward_linear(x_cipher)
        torch.cuda.synchronize()
        return y

    def streamed(name):
        def run():
            first = None
            for y in sf[name].run(items[name]):
                first = y if first is None else first
            return first
        return run

    legs = [('resident', resident)] + [(name, streamed(name)) for name in ('streamed uint8', 'streamed cipher8', 'streamed cipher16')]
    equal = {}
    for (name, leg) in legs:
        with limit(args.step_limit, 'warm-up of %s' % name):
            y = leg()
            equal[name] = bool(torch.equal(y[:batch].cpu(), y0))          # (a streamed leg hands back its first batch: frames[0], what the resident leg runs)
    ms = {name: [] for (name, _) in legs}
    for r in range(args.repeats):
        for (name, leg) in legs:
            with limit(args.step_limit, 'repeat %d of %s' % (r, name)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                leg()
                ms[name].append(1e3 * (time.perf_counter() - t0) / args.batches)
    for s in sf.values():
        s.close()

    # the kernels alone, on the blocks of this workload: batch images of (C, H, W), padded as the pipeline pads them
    def per_call_us(call):
        runs = []
        for _ in range(args.repeats + 1):
            (e0, e1) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            e0.record()
            for _ in range(args.kernel_calls):
                call()
            e1.record()
            e1.synchronize()
            runs.append(1e3 * e0.elapsed_time(e1) / args.kernel_calls)
        runs = runs[1:]                                                  # the first round warms up
        return {'median': statistics.median(runs), 'min': min(runs), 'max': max(runs)}

    with limit(args.step_limit, 'the four kernels alone'):
        (c8, c16) = (cipher[8][0][0].to(dev), cipher[16][0][0].to(dev))
        (lo, hi) = (cipher[8][0][1].to(dev), cipher[8][0][2].to(dev))
        (s8, o8) = ktorch.gray_inverse(lo, hi, 255)
        (s16, o16) = ktorch.gray_inverse(cipher[16][0][1].to(dev), cipher[16][0][2].to(dev), 65535)
        (g8, b8) = ktorch.gray_affine(lo, hi, 255)
        (g16, b16) = ktorch.gray_affine(lo, hi, 65535)
        block = x_cipher[:batch] if x_cipher.shape[0] == batch else ktorch.frames_to_linear(c8, pad_to=1)
        kernels = {
            'kn_u8_to_linear': per_call_us(lambda: ktorch.frames_to_linear(c8, pad_to=pad_to)),
            'kn_frames_to_linear depth 8': per_call_us(lambda: ktorch.frames_to_linear(c8, pad_to=pad_to, scale=s8, offset=o8)),
            'kn_frames_to_linear depth 16': per_call_us(lambda: ktorch.frames_to_linear(c16, pad_to=pad_to, scale=s16, offset=o16)),
            'kn_linear_to_u8': per_call_us(lambda: ktorch.linear_to_frames(block, (C, H, W), gain=g8, bias=b8)),
            'kn_linear_to_u16': per_call_us(lambda: ktorch.linear_to_frames(block, (C, H, W), gain=g16, bias=b16, depth=16)),
        }
        torch.cuda.synchronize()

    rec = {name: spread(v, batch) for (name, v) in ms.items()}
    base = rec['resident']['ms_per_batch']['median']
    for name in sf:
        rec[name]['rate_over_resident'] = base / rec[name]['ms_per_batch']['median']
    (u8, c8r) = (rec['streamed uint8']['ms_per_batch'], rec['streamed cipher8']['ms_per_batch'])
    compare = {'cipher8_over_uint8_ms_per_batch': c8r['median'] / u8['median'],
               'cipher8_slower_beyond_the_spread': bool(c8r['min'] > u8['max'])}
    out = {'tool': 'tools/cipher_stream_rate.py', 'workload': desc, 'contract': str(exact), 'device': torch.cuda.get_device_name(dev), 'batch': batch,
           'batches_per_run': args.batches, 'repeats': args.repeats, 'pad_to': pad_to, 'images_per_run': images, 'legs': rec, 'cipher8_against_uint8': compare,
           'kernels_us_per_call': kernels, 'kernel_calls_per_timing': args.kernel_calls, 'logits_bit_equal_to_the_first_forward': equal,
           'what': 'legs: host wall clock around runs that end in a device synchronise (streamed: in the last read-back), alternated; a streamed run includes pipeline '
                   'fill and drain.  kernels: device events around back-to-back calls of the Python entry (the allocation of the result included), one warm-up round dropped'}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
