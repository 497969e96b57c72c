#!/usr/bin/env python
"""What a caller with frames on the HOST gets, next to the device-resident rate bench.py reports: one key-net, one batch size, one process, four legs

  resident          knet.forward_linear(x_cipher) on an encrypted batch that sits in HBM -- the loop bench.py times, the yardstick
  resident+ingest   the same with the ingest of device-resident uint8 frames and the sensor's keyed product inside the loop (no transfer)
  streamed uint8    keynet_amd.stream.StreamedForward from uint8 NHWC host frames: staging copy, upload, ingest, encrypt, forward, read-back of the logits
  streamed float32  the same from float32 NCHW host batches (four times the bytes)

alternated `--repeats` times after one warm-up each; per leg the median, minimum and maximum of ms per batch and images/s.  Every leg runs the same frames, so a
key-net under the 'auto' contract is calibrated once and every leg runs the same kernels (the logits of the legs are compared, bit for bit).  Next to them: the upload
of one batch alone (device events on the copy stream), the host's staging copy alone, and the share of the upload time that is hidden,
1 - (streamed - resident+ingest) / upload, clipped to [0, 1] -- the difference also holds the staging copy and the read-back, so the share is a lower bound.
A streamed run includes the fill and the drain of the pipeline (the first upload and the last read-back overlap nothing).  Every GPU step runs under a time limit
of its own: a step that overruns it ends the process.  Prints one JSON record (and writes it to --out).

    python tools/stream_rate.py --workload vgg16 --batch 256 --batches 16 --repeats 5 --out profiles/streamed_forward.txt
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
    sys.stderr.write('[stream_rate] %s (limit %d s)\n' % (what, seconds))
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
    ap.add_argument('--batches', type=int, default=16, help='batches per timed run')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--exact', default=None, choices=['auto', 'true', 'false'], help='the contract the key-net is built under (default: bench.py\'s -- auto for the vgg16 workloads)')
    ap.add_argument('--step-limit', type=int, default=240, help='seconds a single GPU step may take')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from benchlegs.workloads import build_workload, upload_operators
    from keynet_amd.stream import StreamedForward

    dev = torch.device('cuda', 0)
    exact = {'auto': 'auto', 'true': True, 'false': False, None: 'auto' if args.workload.startswith('vgg16') else None}[args.exact]
    (sensor, knet, inshape, batch, desc, _) = build_workload(args.workload, 0, exact=exact, fanout=True, prepare=upload_operators(dev))
    assert torch.cuda.is_available(), 'stream_rate.py needs an MI355X'          # (after the keying: its forked processes start before this one touches the GPU)
    torch.cuda.set_device(dev)
    batch = args.batch or batch
    (C, H, W) = inshape
    rng = np.random.RandomState(1234)
    frames = [torch.as_tensor(rng.randint(0, 256, size=(batch, H, W, C)).astype(np.uint8)) for _ in range(min(4, args.batches))]
    items_u8 = [frames[k % len(frames)] for k in range(args.batches)]
    floats = [f.permute(0, 3, 1, 2).contiguous().float() for f in frames]
    items_f32 = [floats[k % len(floats)] for k in range(args.batches)]
    sf_u8 = StreamedForward(sensor, knet, batch, layout='NHWC', frames='uint8')
    sf_f32 = StreamedForward(sensor, knet, batch, frames='float32')
    pad_to = sf_u8._pad_to
    images = batch * args.batches

    with limit(args.step_limit, 'upload of the frames, first forward (operators resident, contracts decided)'):
        frames_dev = frames[0].to(dev)
        x_cipher = sensor.encrypt_frames(frames_dev, pad_to=pad_to)
        y0 = knet.forward_linear(x_cipher)[:batch].cpu()
        torch.cuda.synchronize()

    def resident():
        for _ in range(args.batches):
            y = knet.forward_linear(x_cipher)
        torch.cuda.synchronize()
        return y

    def resident_ingest():
        for _ in range(args.batches):
            y = knet.forward_linear(sensor.encrypt_frames(frames_dev, pad_to=pad_to))
        torch.cuda.synchronize()
        return y

    def streamed(sf, items):
        def run():
            first = None
            for y in sf.run(items):
                first = y if first is None else first
            return first
        return run

    legs = [('resident', resident), ('resident+ingest', resident_ingest), ('streamed uint8', streamed(sf_u8, items_u8)), ('streamed float32', streamed(sf_f32, items_f32))]
    equal = {}
    for (name, leg) in legs:
        with limit(args.step_limit, 'warm-up of %s' % name):
            y = leg()
            equal[name] = bool(torch.equal(y[:batch].cpu(), y0))          # (a streamed leg hands back its first batch: frames[0], what the resident legs run)
    ms = {name: [] for (name, _) in legs}
    for r in range(args.repeats):
        for (name, leg) in legs:
            with limit(args.step_limit, 'repeat %d of %s' % (r, name)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                leg()
                ms[name].append(1e3 * (time.perf_counter() - t0) / args.batches)

    def upload_alone(host):
        pin = torch.empty(host.shape, dtype=host.dtype, pin_memory=True)
        t0 = time.perf_counter()
        for _ in range(5):
            pin.copy_(host)
        stage_ms = 1e3 * (time.perf_counter() - t0) / 5
        dst = torch.empty(host.shape, dtype=host.dtype, device=dev)
        s = torch.cuda.Stream(dev)
        (e0, e1) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        with torch.cuda.stream(s):
            dst.copy_(pin, non_blocking=True)
            e0.record(s)
            for _ in range(5):
                dst.copy_(pin, non_blocking=True)
            e1.record(s)
        s.synchronize()
        return {'bytes': int(host.numel() * host.element_size()), 'upload_ms': e0.elapsed_time(e1) / 5, 'staging_copy_ms': stage_ms}

    with limit(args.step_limit, 'the upload of one batch alone'):
        alone = {'uint8': upload_alone(frames[0]), 'float32': upload_alone(floats[0])}
    sf_u8.close()
    sf_f32.close()

    rec = {name: spread(v, batch) for (name, v) in ms.items()}
    base = rec['resident']['ms_per_batch']['median']
    ingest = rec['resident+ingest']['ms_per_batch']['median']
    for (name, kind) in (('streamed uint8', 'uint8'), ('streamed float32', 'float32')):
        t = rec[name]['ms_per_batch']['median']
        rec[name]['rate_over_resident'] = base / t
        rec[name]['ms_over_resident+ingest'] = t - ingest
        rec[name]['upload_alone'] = alone[kind]
        rec[name]['share_of_upload_hidden_at_least'] = min(1.0, max(0.0, 1.0 - (t - ingest) / alone[kind]['upload_ms']))
    out = {'tool': 'tools/stream_rate.py', 'workload': desc, 'contract': str(exact), 'device': torch.cuda.get_device_name(dev), 'batch': batch, 'batches_per_run': args.batches,
           'repeats': args.repeats, 'pad_to': pad_to, 'images_per_run': images, 'legs': rec, 'logits_bit_equal_to_the_first_forward': equal,
           'what': 'host wall clock around runs that end in a device synchronise (streamed: in the last read-back), legs alternated; a streamed run includes pipeline fill and drain'}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
