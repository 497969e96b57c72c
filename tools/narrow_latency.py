#!/usr/bin/env python
"""Latency of the low-latency (narrow) forward against the padded forward, on ONE key-net in ONE process.

    python tools/narrow_latency.py [--workload vgg16|allconv] [--forwards 20] [--warmup 3] [--out FILE]         # default profiles/r07_narrow_forward.txt
    python tools/narrow_latency.py --one-forward [-n 1]        # keys, warms up, then runs ONE narrow forward: the program for a kernel trace
                                                               # (rocprofv3 --kernel-trace --stats -- python tools/narrow_latency.py --one-forward)

Keys the headline workload (benchlegs.workloads: TiledPermutationKeynet VGG-16, tile 64, default contract; `--workload allconv`: the untiled PermutationKeynet
AllConvNet, whose conv layers are factored stand-ins) and, for n in (1, 2, 4, 8) images, times three forwards of the SAME images on that key-net:
forward_linear(x) (padded to 128 images: the code path of every earlier release), forward_linear(x, narrow=True) eager, and the replay of
capture(x, narrow=True).  HIP events around each forward, a warm-up, the median over --forwards forwards (min and max beside it).  The narrow logits must be
torch.equal to the padded ones before any time is printed.  Prints one table and appends it to --out.

    python tools/narrow_latency.py --mfma [--out profiles/r08_narrow_mfma.txt]
    python tools/narrow_latency.py --mfma --one-forward          # the program for a kernel trace: for n in (1, 2, 4, 8) ONE narrow=True forward, then ONE
                                                                 # narrow='mfma' forward (rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python ...)
    python tools/narrow_latency.py --from-trace DIR/.../*_kernel_trace.csv [--convs 13] [--out ...]   # no GPU: the conv launches of those forwards, layer by layer

--mfma: the same key-net under exact_mode('auto') after ONE calibrating wide forward (every conv layer of the permutation-keyed VGG-16 stays on the matrix
cores), three forwards of the same images in this one process: padded, narrow=True (the channel-lane kernel), narrow='mfma' (the matrix-core narrow kernel,
measured and accepted layer by layer on the first call), and the gate ratios of the narrow records (the measured distance between the two narrow
arithmetics).  The narrow='mfma' logits must be inside the float-key gate against narrow=True before any time is printed.  The times of the conv LAUNCHES
themselves (no Python, no launch overhead, no screen reduction) come from the kernel trace: --from-trace reads the device timestamps of the last eight
forwards of a --mfma --one-forward run and prints every conv launch of both kernels beside each other, and their sums.

    python tools/narrow_latency.py --rows [--out profiles/r09_narrow_rows.txt]
    python tools/narrow_latency.py --rows --one-forward          # for n in (1, 2, 4, 8) ONE narrow=True forward, then ONE with narrow_rows=True (for a kernel trace)
    python tools/narrow_latency.py --rows --from-trace DIR/.../*_kernel_trace.csv [--convs 13]       # no GPU: the NON-conv launches of those forwards side by side

--rows: whole forwards with and without narrow_rows in one process, alternating -- narrow=True under the default contract, then narrow='mfma' under
exact_mode('auto') after one calibrating wide forward -- the logits torch.equal before any time is printed; and every layer that takes the row-lane kernel alone,
its kn_spmm with and without KN_FLAG_NARROW_ROWS on the same block (HIP events, median).

    python tools/narrow_latency.py --narrow32 [--out profiles/r10_narrow32.txt]
    python tools/narrow_latency.py --narrow32 --one-forward      # for n in (16, 32) ONE narrow=True, narrow32=True forward, then ONE narrow='mfma', narrow32=True forward
    python tools/narrow_latency.py --narrow32 --from-trace DIR/.../*_kernel_trace.csv          # no GPU: the 13 conv launches of those four forwards
    KEYNET_HIP_LIB=<diagnostic build> python tools/narrow_latency.py --narrow32 --blocks        # one conv5_x-shaped operator at 32 columns per column-block width

--narrow32: for 8, 9, 12, 16, 24 and 32 images, in one process with the forms alternating: the padded forward (no keyword) and narrow=True, narrow32=True under the
default contract -- logits torch.equal before any time is printed --, then under exact_mode('auto') after one calibrating wide forward the padded forward and
narrow='mfma', narrow32=True (inside the float-key gate against narrow=True, narrow32=True); at 8 images the plain narrow forwards are the yardstick.  The bars of
the file are computed from the table.  --blocks: convtaps_narrow32_kernel on a 14 x 14 pixel, 512 -> 512 channel 3 x 3 operator at 32 columns with the block
width forced by KN_NARROW32_NV (read at create by the diagnostic build only: keynet_amd.build.build(out=..., defines=('KN_ABLATION',))) against the launcher's rule.

    python tools/narrow_latency.py --narrow64 [--workload vgg16|allconv] [--out profiles/r11_narrow64.txt]
    python tools/narrow_latency.py --narrow64 --one-forward      # at 64 images ONE forward without the keyword (padded to 128), then ONE narrow=True, narrow64=True forward
    python tools/narrow_latency.py --narrow64 --from-trace DIR/.../*_kernel_trace.csv          # no GPU: the 13 conv launches of those two forwards

--mfma64 (profiles/r12_narrow64_mfma.txt): under exact_mode('auto') after one calibrating padded forward, in one process with the forms alternating, at 33, 48 and 64
images: (a) the forward without the keyword (padded to 128 images), (b) narrow='mfma', narrow64='mfma' (the f32 tile kernel on 64-column tiles; logits torch.equal to (a)
before any time is printed), (c) the same images as two narrow='mfma', narrow32=True forwards.  `--mfma64 --one-forward` / `--mfma64 --from-trace`: the conv launches of one
(a) and one (b) forward at 64 images, layer by layer.
--narrow64: under the default contract, in one process with the forms alternating: the forward without the keyword (a tiled key-net: padded to 128 images) against
narrow=True, narrow64=True at 33, 48 and 64 images (`--workload allconv`: at 48) -- logits torch.equal before any time is printed --, and the narrow32 forward at 32
images for the ladder.  The bars of the file are computed from the table.

    python tools/narrow_latency.py --linear [--out profiles/r13_narrow_linear.txt]
    python tools/narrow_latency.py --linear --one-forward        # for n in (1, 8, 16, 64) ONE narrow forward, then ONE with narrow_linear=True (for a kernel trace)
    python tools/narrow_latency.py --linear --from-trace DIR/.../*_kernel_trace.csv [--convs 13]     # no GPU: the CSR launches of those forwards side by side

    python tools/narrow_latency.py --split [--layers conv1_2,conv5_x]     # no key-net: filled-in synthetic operators of the VGG-16 conv shapes, narrow='mfma' without and with
                                                                          # narrow_split=True at 1, 8 and 32 images in one process (profiles/r14_narrow_split.txt)
    python tools/narrow_latency.py --split --one-forward                  # ONE narrow split call per layer and width behind a warm-up call (for a kernel trace)
    python tools/narrow_latency.py --split --from-trace DIR/.../*_kernel_trace.csv    # no GPU: the four steps of those calls
    python tools/narrow_latency.py --fill [--layers conv1_2,conv5_x]      # the same operators under exact=True: narrow=True without and with narrow_fill=True and the padded 128-column call
                                                                          # at 1, 8, 16, 32 images in one process (profiles/r16_narrow_fill.txt); --one-forward / --from-trace as for --split

    python tools/narrow_latency.py --taps [--out profiles/r15_narrow_taps.txt]
    python tools/narrow_latency.py --taps32 [--workload allconv] [--one-forward | --from-trace DIR/.../*_kernel_trace.csv]
    python tools/narrow_latency.py --pairs [--one-forward | --from-trace DIR/.../*_kernel_trace.csv]
    python tools/narrow_latency.py --taps --one-forward          # for n in (1, 2, 4, 8) ONE narrow forward, then ONE with narrow_taps=True (for a kernel trace)
    python tools/narrow_latency.py --taps --from-trace DIR/.../*_kernel_trace.csv [--convs 13]       # no GPU: the conv launches of those forwards side by side

--taps32: keyed VGG-16 under the default contract, whole forwards narrow=True, narrow32=True, narrow_linear=True without and with narrow_taps='packed' at 9, 12, 16, 24
and 32 images (HIP events, median of 20 with min .. max, the two forms alternating, logits torch.equal), and in the same process the 8-image forward narrow=True,
narrow_rows=True, narrow_linear=True, narrow_taps=True; the two bars of the table: at 16 and 32 images the gain exceeds the two spreads added, and 16 images cost no more
than twice the 8-image forward.  --workload allconv: 16 images (blocks of 8 columns).  --one-forward / --from-trace: as --taps, at 16 and 32 images, against
convtaps_narrow32_kernel in the same trace.  Appends to profiles/r17_narrow_taps32.txt.
--pairs: keyed VGG-16 under the default contract, whole forwards narrow=True, narrow_rows=True, narrow_linear=True, narrow_taps=True against the same with
narrow_taps='pairs' at 1, 2, 4 and 8 images in one process (HIP events, median of 20 with min .. max, the two forms alternating, logits torch.equal before any time
is printed), and whether the one-image forward meets 4 ms.  --one-forward / --from-trace: as --taps, the 13 conv launches of convtaps_narrow_taps_kernel against
those of the narrow_taps='pairs' forward in one trace, three forwards of each form alternating per width: per launch the medians with min .. max, and WINS where
the gain exceeds the two spreads added, else LOSES (the rule of narrow_taps_pairs_loses).  Appends to profiles/r18_narrow_taps_pairs.txt.
--taps: keyed VGG-16 under the default contract, whole forwards narrow=True, narrow_rows=True, narrow_linear=True without and with narrow_taps=True at 1, 2, 4 and 8
images in one process, the forms alternating, the logits torch.equal before any time is printed.

--linear: keyed VGG-16 under the default contract, everything in one process with the forms alternating.  fc6, fc7 and fc8 alone: kn_spmm without and with
KN_FLAG_NARROW_LINEAR at 1, 2, 3, 4, 8, 16, 32, 33 and 64 columns, up to 8 columns also next to KN_FLAG_NARROW_ROWS -- back to back on one block (values as warm as
the layer's size lets them be) and behind a pass over a 512 MB buffer that leaves nothing of the operator on chip (what a forward sees) -- with the plan strings; then
whole forwards at 1, 8, 16 and 64 images, narrow=True with the width's keywords, without and with narrow_linear=True, the logits torch.equal before any time is printed."""
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


def mfma_table(args, knet, xc, desc):
    """--mfma: see the module docstring."""
    from keynet_amd import sparse as ksp
    from keynet_amd.layer import gate
    knet.exact_mode('auto')
    knet.forward_linear(xc)                       # the calibrating wide forward (8 images, padded to 128)
    rep = knet.contract_report()
    convs = [(name, c) for (name, c) in knet._keyed(named=True) if isinstance(c.W, ksp.Conv2dTiledMatrix)]
    wide = dict((r['name'], r['exact']) for r in rep['layers'])
    if args.one_forward:
        for n in (1, 2, 4, 8):                    # operators resident, narrow records measured
            knet.forward_linear(xc[:n].t().contiguous().t(), narrow='mfma')
        torch.cuda.synchronize()
        print("TRACE-FROM-HERE: for n in (1, 2, 4, 8) one narrow=True forward, then one narrow='mfma' forward; %d conv layers" % len(convs), flush=True)
        for n in (1, 2, 4, 8):
            x = xc[:n].t().contiguous().t()
            knet.forward_linear(x, narrow=True)
            knet.forward_linear(x, narrow='mfma')
            torch.cuda.synchronize()
        return
    out = args.out or os.path.join(ROOT, 'profiles', 'r08_narrow_mfma.txt')
    lines = ['', "== tools/narrow_latency.py --mfma: %s under exact_mode('auto') after one calibrating wide forward" % desc,
             '   %s, torch %s; HIP events, %d warm-up + median of %d forwards (min .. max)' % (torch.cuda.get_device_name(0), torch.__version__, args.warmup, args.forwards),
             '   conv layers left on the matrix cores by calibration: %d of %d' % (sum(1 for (name, _) in convs if wide[name] is False), len(convs)),
             '   %6s | %-28s | %-28s | %-28s | %s' % ('images', 'padded forward_linear [ms]', 'narrow=True [ms]', "narrow='mfma' [ms]", "narrow=True / narrow='mfma'")]
    for n in (1, 2, 4, 8):
        x = xc[:n].t().contiguous().t()
        ye = knet.forward_linear(x, narrow=True)
        ym = knet.forward_linear(x, narrow='mfma')
        torch.cuda.synchronize()
        ratio = gate(ym, ye)[0]
        assert ratio <= 1.0, "narrow='mfma' logits outside the float-key gate against narrow=True at %d image(s): %g" % (n, ratio)
        t = [timed(lambda: knet.forward_linear(x), args.forwards, args.warmup),
             timed(lambda: knet.forward_linear(x, narrow=True), args.forwards, args.warmup),
             timed(lambda: knet.forward_linear(x, narrow='mfma'), args.forwards, args.warmup)]
        v = [(statistics.median(u), min(u), max(u)) for u in t]
        cell = ['%8.3f (%.3f .. %.3f)' % u for u in v]
        lines.append('   %6d | %-28s | %-28s | %-28s | %.2fx   (logits: gate ratio %.3g)' % (n, cell[0], cell[1], cell[2], v[1][0] / v[2][0], ratio))
        print('n = %d done' % n, flush=True)
    lines.append('')
    lines.append("   narrow records (the measured distance between the two narrow arithmetics: worst element's share of its tolerance 1e-5 + 1e-5 |ref|):")
    for r in knet.contract_report()['layers']:
        if r['narrow'] is not None:
            lines.append('     %-12s decided %-5s gate ratio %-10.3g max |x| %-10.3g on %d column(s)' % (r['name'], r['narrow']['decided'], r['narrow']['gate_ratio'] or 0.0, r['narrow']['max_abs_x'] or 0.0, r['narrow']['measured_on_columns']))
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(out, 'a') as f:
        f.write(text)


N32_IMAGES = (8, 9, 12, 16, 24, 32)


def narrow32_table(args, knet, xc, desc):
    """--narrow32: see the module docstring."""
    from keynet_amd.layer import gate
    blk = lambda n: xc[:n].t().contiguous().t()
    if args.one_forward:
        knet.exact_mode('auto')
        knet.forward_linear(blk(8))
        for n in (16, 32):                        # operators resident, narrow records measured
            knet.forward_linear(blk(n), narrow=True, narrow32=True)
            knet.forward_linear(blk(n), narrow='mfma', narrow32=True)
        torch.cuda.synchronize()
        print("TRACE-FROM-HERE: for n in (16, 32) one narrow=True, narrow32=True forward, then one narrow='mfma', narrow32=True forward", flush=True)
        for n in (16, 32):
            knet.forward_linear(blk(n), narrow=True, narrow32=True)
            knet.forward_linear(blk(n), narrow='mfma', narrow32=True)
            torch.cuda.synchronize()
        return
    cell = lambda v: '%8.3f (%.3f .. %.3f)' % (statistics.median(v), min(v), max(v))
    lines = ['', '== tools/narrow_latency.py --narrow32%s: %s' % ('' if args.workload == 'vgg16' else ' --workload %s' % args.workload, desc),
             '   %s, torch %s; HIP events, %d warm-up + median of %d forwards (min .. max), the forms of a row alternating in quarters'
             % (torch.cuda.get_device_name(0), torch.__version__, args.warmup, args.forwards)]
    med = {}

    def table(mode, title, check):
        lines.append('   %s' % title)
        lines.append('   %6s | %-28s | %-28s | %-9s | %s' % ('images', 'no keyword [ms]', 'narrow=%r, narrow32=True [ms]' % (mode,), 'speed-up', 'narrow=%r alone (8 images) [ms]' % (mode,)))
        for n in args.images:
            x = blk(n)
            check(n, knet.forward_linear(x), knet.forward_linear(x, narrow=mode, narrow32=True))
            forms = [lambda: knet.forward_linear(x), lambda: knet.forward_linear(x, narrow=mode, narrow32=True)] + ([lambda: knet.forward_linear(x, narrow=mode)] if n <= 8 else [])
            t = [[] for _ in forms]
            for _ in range(4):                    # alternate in quarters
                for (u, f) in zip(t, forms):
                    u += timed(f, args.forwards // 4, args.warmup)
            med[(mode, n)] = [statistics.median(u) for u in t] + [max(u) - min(u) for u in t]
            lines.append('   %6d | %-28s | %-28s | %8.2fx | %s' % (n, cell(t[0]), cell(t[1]), statistics.median(t[0]) / statistics.median(t[1]), cell(t[2]) if n <= 8 else ''))
            print('narrow=%r n = %d done' % (mode, n), flush=True)
        lines.append('')

    def equal(n, y0, y1):
        torch.cuda.synchronize()
        assert torch.equal(y0, y1), 'narrow32 logits differ from the forward without the keyword at %d images: max %g' % (n, float((y0 - y1).abs().max()))

    def inside(n, y0, y1):
        ye = knet.forward_linear(blk(n), narrow=True, narrow32=True)
        torch.cuda.synchronize()
        ratio = gate(y1, ye)[0]
        assert ratio <= 1.0, "narrow='mfma', narrow32=True logits outside the float-key gate against narrow=True, narrow32=True at %d images: %g" % (n, ratio)

    pads0 = getattr(knet, '_padded_forwards', 0)
    table(True, 'default contract (bit-exact); logits torch.equal: yes', equal)
    padded = getattr(knet, '_padded_forwards', 0) > pads0
    if args.workload == 'vgg16':
        knet.exact_mode('auto')
        knet.forward_linear(blk(8))               # the calibrating wide forward
        table('mfma', "exact_mode('auto') after one calibrating wide forward; logits inside the float-key gate against narrow=True, narrow32=True: yes", inside)
        for r in knet.contract_report()['layers']:
            if r['narrow'] is not None:
                lines.append('     %-12s decided %-5s gate ratio %-10.3g max |x| %-10.3g on %d column(s)' % (r['name'], r['narrow']['decided'], r['narrow']['gate_ratio'] or 0.0, r['narrow']['max_abs_x'] or 0.0, r['narrow']['measured_on_columns']))
        lines.append('')
    lines.append('   the forward without the keyword is %s' % ('padded to 128 images' if padded else 'NOT padded (an untiled key-net runs at the width it is given)'))
    for mode in (True, 'mfma'):
        if (mode, 8) in med and (mode, 16) in med:
            (m8, m16) = (med[(mode, 8)], med[(mode, 16)])
            lines.append('   narrow=%r: (a) 16 images / 8 images on the plain narrow forward = %.2fx (bar: <= 2);  (b) no keyword / narrow32 at 16 images = %.2fx (bar: >= 1.5)%s'
                         % (mode, m16[1] / m8[2], m16[0] / m16[1],
                            ';  at 32 images %.3f ms against %.3f ms, spread of the two forms %.3f / %.3f ms' % (med[(mode, 32)][0], med[(mode, 32)][1], med[(mode, 32)][2], med[(mode, 32)][3])
                            if (mode, 32) in med else ''))
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out or os.path.join(ROOT, 'profiles', 'r10_narrow32.txt'), 'a') as f:
        f.write(text)


N64_IMAGES = (33, 48, 64)


def narrow64_table(args, knet, xc, desc):
    """--narrow64: see the module docstring."""
    blk = lambda n: xc[:n].t().contiguous().t()
    kw = dict(narrow=True, narrow64=True)
    if args.one_forward:
        for _ in range(2):                        # operators resident, workspaces sized
            knet.forward_linear(blk(64))
            knet.forward_linear(blk(64), **kw)
        torch.cuda.synchronize()
        print('TRACE-FROM-HERE: at 64 images one forward without the keyword (padded to 128), then one narrow=True, narrow64=True forward', flush=True)
        knet.forward_linear(blk(64))
        torch.cuda.synchronize()
        knet.forward_linear(blk(64), **kw)
        torch.cuda.synchronize()
        return
    cell = lambda v: '%8.3f (%.3f .. %.3f)' % (statistics.median(v), min(v), max(v))
    images = (48,) if args.workload == 'allconv' else N64_IMAGES
    lines = ['', '== tools/narrow_latency.py --narrow64%s: %s' % ('' if args.workload == 'vgg16' else ' --workload %s' % args.workload, desc),
             '   %s, torch %s; HIP events, %d warm-up + median of %d forwards (min .. max), the forms of a row alternating in quarters; default contract, logits torch.equal: yes'
             % (torch.cuda.get_device_name(0), torch.__version__, args.warmup, args.forwards),
             '   %6s | %-28s | %-28s | %-9s | %s' % ('images', 'no keyword [ms]', 'narrow=True, narrow64=True [ms]', 'speed-up', 'ms per image, narrow64')]
    med = {}
    pads0 = getattr(knet, '_padded_forwards', 0)
    for n in images:
        x = blk(n)
        (y0, y1) = (knet.forward_linear(x), knet.forward_linear(x, **kw))
        torch.cuda.synchronize()
        assert torch.equal(y0, y1), 'narrow64 logits differ from the forward without the keyword at %d images: max %g' % (n, float((y0 - y1).abs().max()))
        forms = [lambda: knet.forward_linear(x), lambda: knet.forward_linear(x, **kw)]
        t = [[] for _ in forms]
        for _ in range(4):                        # alternate in quarters
            for (u, f) in zip(t, forms):
                u += timed(f, args.forwards // 4, args.warmup)
        med[n] = [statistics.median(u) for u in t]
        lines.append('   %6d | %-28s | %-28s | %8.2fx | %.3f' % (n, cell(t[0]), cell(t[1]), med[n][0] / med[n][1], med[n][1] / n))
        print('n = %d done' % n, flush=True)
    padded = getattr(knet, '_padded_forwards', 0) > pads0
    lines.append('   the forward without the keyword is %s' % ('padded to 128 images' if padded else 'NOT padded (an untiled key-net runs at the width it is given)'))
    if args.workload == 'vgg16':
        x = blk(32)
        t32 = timed(lambda: knet.forward_linear(x, narrow=True, narrow32=True), args.forwards, args.warmup)
        m32 = statistics.median(t32)
        lines.append('   %6d | %-28s | %-28s |           | %.3f   (narrow=True, narrow32=True: the ladder)' % (32, '', cell(t32), m32 / 32))
        lines.append('   (a) no keyword / narrow64 at 64 images = %.2fx (the instruction count says up to 2x; below 1.3x the form is not worth merging)' % (med[64][0] / med[64][1]))
        lines.append('   (b) narrow64 at 33 / 48 / 64 images: %.3f / %.3f / %.3f ms (one form, masked: 33 and 48 must not cost more than 64); per image at 64: %.3f ms against %.3f ms of narrow32 at 32'
                     % (med[33][1], med[48][1], med[64][1], med[64][1] / 64, m32 / 32))
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out or os.path.join(ROOT, 'profiles', 'r11_narrow64.txt'), 'a') as f:
        f.write(text)


def mfma64_table(args, knet, xc, desc):
    """--mfma64: see the module docstring."""
    from keynet_amd import sparse as ksp
    blk = lambda lo, hi: xc[lo:hi].t().contiguous().t()
    kw = dict(narrow='mfma', narrow64='mfma')
    kw32 = dict(narrow='mfma', narrow32=True)
    knet.exact_mode('auto')
    knet.forward_linear(blk(0, 64))               # the calibrating padded forward
    convs = [(name, c) for (name, c) in knet._keyed(named=True) if isinstance(c.W, ksp.Conv2dTiledMatrix)]
    if args.one_forward:
        for _ in range(2):                        # operators resident, workspaces sized
            knet.forward_linear(blk(0, 64))
            knet.forward_linear(blk(0, 64), **kw)
        torch.cuda.synchronize()
        print("TRACE-FROM-HERE: at 64 images one forward without the keyword (padded to 128), then one narrow='mfma', narrow64='mfma' forward", flush=True)
        knet.forward_linear(blk(0, 64))
        torch.cuda.synchronize()
        knet.forward_linear(blk(0, 64), **kw)
        torch.cuda.synchronize()
        return
    cell = lambda v: '%8.3f (%.3f .. %.3f)' % (statistics.median(v), min(v), max(v))
    lines = ['', "== tools/narrow_latency.py --mfma64: %s under exact_mode('auto') after one calibrating padded forward" % desc,
             '   %s, torch %s; HIP events, %d warm-up + median of %d forwards (min .. max), the forms of a row alternating in quarters; logits of (b) torch.equal to (a): yes'
             % (torch.cuda.get_device_name(0), torch.__version__, args.warmup, args.forwards),
             '   conv layers on the f32 / bf16x3 matrix-core kernels by calibration: %d of %d' % (sum(1 for (_, c) in convs if c._exact in (False, 'bf16x3')), len(convs)),
             "   %6s | %-28s | %-28s | %-28s | %s" % ('images', '(a) no keyword, padded [ms]', "(b) narrow64='mfma' [ms]", "(c) two narrow32 'mfma' [ms]", '(a) / (b), (c) / (b)')]
    med = {}
    for n in N64_IMAGES:
        (x, xa, xb) = (blk(0, n), blk(0, 32), blk(32, n))
        (y0, y1) = (knet.forward_linear(x), knet.forward_linear(x, **kw))
        knet.forward_linear(xa, **kw32)           # (measures the narrow records of calibrated layers once)
        knet.forward_linear(xb, **kw32)
        torch.cuda.synchronize()
        assert torch.equal(y0, y1), "narrow64='mfma' logits differ from the padded forward at %d images: max %g" % (n, float((y0 - y1).abs().max()))
        forms = [lambda: knet.forward_linear(x), lambda: knet.forward_linear(x, **kw), lambda: (knet.forward_linear(xa, **kw32), knet.forward_linear(xb, **kw32))]
        t = [[] for _ in forms]
        for _ in range(4):                        # alternate in quarters
            for (u, f) in zip(t, forms):
                u += timed(f, args.forwards // 4, args.warmup)
        med[n] = [statistics.median(u) for u in t]
        lines.append('   %6d | %-28s | %-28s | %-28s | %.2fx, %.2fx' % (n, cell(t[0]), cell(t[1]), cell(t[2]), med[n][0] / med[n][1], med[n][2] / med[n][1]))
        print('n = %d done' % n, flush=True)
    lines.append('   bars at 64 images: (a) / (b) = %.2fx (>= 1.3x asked, 2x is the ceiling: half the matrix work); (c) / (b) = %.2fx (must exceed 1)' % (med[64][0] / med[64][1], med[64][2] / med[64][1]))
    lines.append('   the 64-column launch of each conv layer (kn_spmm_plan at 64 aligned columns):')
    for (name, c) in convs:
        la = c.launch(xc.device, relu=False, **kw)
        with torch.cuda.device(xc.device):
            lines.append('     %-10s %s' % (name, la.op.plan(64, la.flags).split(';')[0]))
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out or os.path.join(ROOT, 'profiles', 'r12_narrow64_mfma.txt'), 'a') as f:
        f.write(text)


def narrow64_trace_table(args):
    """--narrow64 --from-trace: the conv launches of the last two forwards of a `--narrow64 --one-forward` run (device timestamps).  With --mfma64: of a `--mfma64 --one-forward` run."""
    import csv
    with open(args.from_trace, newline='') as f:
        rows = [r for r in csv.DictReader(f) if 'convtaps_' in r['Kernel_Name'] and 'zero_guard' not in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    k = args.convs + args.linears                 # (a keyed nn.Linear on the matrix cores is a split-K launch of the same kernel family, behind the convs of its forward)
    assert len(rows) >= 2 * k, 'the trace holds %d conv launches, fewer than 2 forwards of %d' % (len(rows), k)
    (wide, new) = (rows[-2 * k:-k], rows[-k:])
    us = lambda r: (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
    wgs = lambda r: int(r.get('Grid_Size_X') or 0) // max(1, int(r.get('Workgroup_Size_X') or 1))
    short = lambda r: r['Kernel_Name'].replace('void kn::', '').split('(')[0]
    (flag, form, out) = ('--mfma64', "narrow='mfma', narrow64='mfma'", 'r12_narrow64_mfma.txt') if args.mfma64 else ('--narrow64', 'narrow=True, narrow64=True', 'r11_narrow64.txt')
    lines = ['', '== tools/narrow_latency.py %s --from-trace: the conv launches of one forward without the keyword (64 images padded to 128) and one %s forward' % (flag, form),
             '   of the same 64 images (rocprofv3 --kernel-trace, device timestamps)', '',
             '   conv launch | workgroups, padded | padded [us] | workgroups, narrow64 | narrow64 [us] | ratio | kernels']
    slower = []
    for (j, (a, b)) in enumerate(zip(wide, new)):
        lines.append('     %2s | %7d | %9.1f | %7d | %9.1f | %5.2fx | %s / %s' % (j + 1 if j < args.convs else 'fc', wgs(a), us(a), wgs(b), us(b), us(a) / us(b), short(a), short(b)))
        if us(b) > us(a) and j < args.convs:
            slower.append(j + 1)
    (sa, sb) = (sum(us(r) for r in wide[:args.convs]), sum(us(r) for r in new[:args.convs]))
    k = args.convs
    lines.append('     sum of the %d conv launches: %9.1f | %9.1f | %5.2fx' % (k, sa, sb, sa / sb))
    lines.append('     conv launches slower on the new form than on the padded 128-column form: %s' % (', '.join(str(j) for j in slower) or 'none'))
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out or os.path.join(ROOT, 'profiles', out), 'a') as f:
        f.write(text)


def narrow32_blocks(args):
    """--narrow32 --blocks: see the module docstring."""
    import copy
    import numpy as np
    from keynet_amd import _capi, direct as kdirect, sparse as ksp
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(0)
    (H, C, n) = (14, 512, 32)
    w = (rng.randn(C, C, 3, 3) / np.sqrt(9 * C)).astype(np.float32)
    (pi, po) = (rng.permutation(H * H), rng.permutation(H * H))
    (eo, ei, et) = ([], [], [])
    for (t, (_, S)) in enumerate(kdirect.shift_matrices((H, H), 3, 1)):
        S = S.tocoo()
        eo.append(po[S.row]); ei.append(pi[S.col]); et.append(np.full(S.nnz, t))
    taps = np.stack([w[:, :, i, j] for i in range(3) for j in range(3)])
    lastcol = np.concatenate((rng.randn(C * H * H), [1.0])).astype(np.float32)
    W = ksp.Conv2dTiledMatrix.fromtaps((C, H, H), (C, H, H), taps, np.concatenate(eo), np.concatenate(ei), np.concatenate(et), None, lastcol)
    x = torch.randn(W.shape[1], n, device=dev)
    x[-1] = 1.0
    flags = _capi.KN_FLAG_NARROW | _capi.KN_FLAG_NARROW32 | _capi.KN_FLAG_RELU
    lines = ['', '== tools/narrow_latency.py --narrow32 --blocks: a conv5_x-shaped operator (14 x 14 pixels, 512 -> 512 channels, 3 x 3, permuted pixels) at 32 columns,',
             '   convtaps_narrow32_kernel per column-block width (KN_NARROW32_NV, diagnostic build); HIP events, %d warm-up + median of %d launches (min .. max)' % (args.warmup, args.forwards)]
    ref = None
    for nv in (0, 8, 16, 32, 0):
        if nv:
            os.environ['KN_NARROW32_NV'] = str(nv)
        else:
            os.environ.pop('KN_NARROW32_NV', None)
        Wv = copy.copy(W)
        Wv._op = None
        with torch.cuda.device(dev):
            op = Wv._device_op(dev)
            plan = op.plan(n, flags).split(' (')[0]
            y = torch.empty((W.shape[0], n), device=dev)
            st = torch.cuda.current_stream().cuda_stream
            t = timed(lambda: op.spmm(x.data_ptr(), n, n, y.data_ptr(), n, flags, st), args.forwards, args.warmup)
        torch.cuda.synchronize()
        ref = y if ref is None else ref
        lines.append('   %-8s %-80s %9.1f us (%.1f .. %.1f)   bit-equal to the rule\'s: %s' % ('rule' if not nv else 'NV=%d' % nv, plan[:80], statistics.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3,
                                                                                          bool(torch.equal(y, ref))))
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out or os.path.join(ROOT, 'profiles', 'r10_narrow32.txt'), 'a') as f:
        f.write(text)


# (name, Cin, Cout, H, entries per (output pixel, tap)): the conv shapes of VGG-16 with fill factors across what Conv2dTiledMatrix.fill_factor() documents for doubly-stochastic
# keys (55 - 600; a 14 x 14 layer has 196 pixels to fill)
SPLIT_LAYERS = [('conv1_1', 3, 64, 224, 55), ('conv1_2', 64, 64, 224, 55), ('conv2_1', 64, 128, 112, 150), ('conv2_2', 128, 128, 112, 150), ('conv3_1', 128, 256, 56, 300),
                ('conv3_2', 256, 256, 56, 300), ('conv4_1', 256, 512, 28, 600), ('conv4_2', 512, 512, 28, 600), ('conv5_x', 512, 512, 14, 196)]
SPLIT_IMAGES = (1, 8, 32)


def _split_operator(rng, Cin, Cout, H, fill):
    """A filled-in factored conv of a VGG-16 layer shape, built the way tests/test_parity_gpu.py's _filled_in_convtaps builds one (every output pixel reads `fill` input pixels
    through each of the nine taps, each entry with its own coefficient; an averaging key), vectorised: tap t reads the pixels o + off_t[k] (mod H x H), off_t distinct."""
    import numpy as np
    from keynet_amd import sparse as ksp
    HW = H * H
    taps = (rng.randn(9, Cout, Cin) / np.sqrt(9 * Cin)).astype(np.float32)
    o = np.arange(HW, dtype=np.int64)
    (eo, ei, et) = ([], [], [])
    for t in range(9):
        off = np.sort(rng.choice(HW, size=fill, replace=False))
        eo.append(np.repeat(o, fill))
        ei.append(((o[:, None] + off[None, :]) % HW).reshape(-1))
        et.append(np.full(HW * fill, t))
    coef = (rng.rand(9 * HW * fill) / fill).astype(np.float32)
    lastcol = np.concatenate((rng.randn(Cout * HW), [1.0])).astype(np.float32)
    return ksp.Conv2dTiledMatrix.fromtaps((Cin, H, H), (Cout, H, H), taps, np.concatenate(eo), np.concatenate(ei), np.concatenate(et), coef, lastcol)


def split_table(args):
    """--split: per layer shape, in ONE process, narrow='mfma' without the keyword (the fused operator on the channel-lane kernel: what a narrow forward ran before) and with
    narrow_split=True (the narrow split route, offered whatever the cost rule says: NARROW_SPLIT_MIN_GAIN = 0 for the measurement) at 1, 8 and 32 images, ReLU fused; next to
    each pair the gate() ratio of the route against the fused kernel's bits, and what narrow_split_capable() says with the constants in the tree.  --one-forward: after one
    warm-up call per width, ONE route call per layer and width and nothing else (the program for a kernel trace; --split --from-trace sums its four steps)."""
    import numpy as np
    from keynet_amd import sparse as ksp
    from keynet_amd.layer import gate
    dev = torch.device('cuda:0')
    layers = [l for l in SPLIT_LAYERS if not args.layers or l[0] in args.layers]
    lines = ['', '== tools/narrow_latency.py --split: filled-in synthetic operators of the VGG-16 conv shapes, contract \'split\', ReLU fused; %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__),
             "   fused = torchdot(narrow='mfma') (the channel-lane kernel, summed stored values): %d warm-up + median of %d calls;  route = the same call with narrow_split=True: %d + %d calls; HIP events"
             % (1, args.fused_calls, args.warmup, args.forwards),
             '   %-8s %4s %4s %4s %5s %9s | %6s | %12s | %12s | %7s | %10s | %s' % ('layer', 'Cin', 'Cout', 'H', 'fill', 'entries', 'images', 'fused [ms]', 'route [ms]', 'gain', 'gate ratio', 'narrow_split_capable')]
    for (name, Cin, Cout, H, fill) in layers:
        rng = np.random.RandomState(H + Cin)
        t0 = time.time()
        W = _split_operator(rng, Cin, Cout, H, fill)
        x32 = torch.randn(W.shape[1], 32, device=dev)
        x32[-1] = 1.0
        print('%s built in %.0f s (fill factor %.0f)' % (name, time.time() - t0, W.fill_factor()), flush=True)
        for n in SPLIT_IMAGES:
            x = x32[:, :n].contiguous()
            kw = dict(relu=True, exact='split', narrow='mfma', narrow32=n > ksp.NARROW_MAX)
            rule = W.narrow_split_capable(n)
            W.NARROW_SPLIT_MIN_GAIN = 0.0
            try:
                if not W.narrow_split_route(n, True, dev):
                    # (conv1_1 at 5 .. 32 images: Cin <= 4 keeps a large layer on the channel-lane kernel, narrow_mfma_loses in csrc/kn_internal.h -- no route, the call is the fused one)
                    lines.append('   %-8s %4d %4d %4d %5d %9d | %6d | the channel-mixing operator does not plan the matrix-core narrow kernel at this width: no route, the keyword changes nothing'
                                 % (name, Cin, Cout, H, fill, len(W._taps['ent_out']), n))
                    print(lines[-1], flush=True)
                    continue
                if args.one_forward:
                    W.torchdot(x, narrow_split=True, **kw)
                    torch.cuda.synchronize()
                    print('TRACE: %s n=%d' % (name, n), flush=True)
                    W.torchdot(x, narrow_split=True, **kw)
                    torch.cuda.synchronize()
                    continue
                ys = W.torchdot(x, narrow_split=True, **kw)
                tr = timed(lambda: W.torchdot(x, narrow_split=True, **kw), args.forwards, args.warmup)
            finally:
                del W.NARROW_SPLIT_MIN_GAIN
            yf = W.torchdot(x, **kw)
            tf = timed(lambda: W.torchdot(x, **kw), args.fused_calls, 1)
            (ratio, _, _, _) = gate(ys, yf)
            (mf, mr) = (statistics.median(tf), statistics.median(tr))
            lines.append('   %-8s %4d %4d %4d %5d %9d | %6d | %12.3f | %12.3f | %6.1fx | %10.3g | %s' % (name, Cin, Cout, H, fill, len(W._taps['ent_out']), n, mf, mr, mf / mr, ratio, rule))
            print(lines[-1], flush=True)
            del ys, yf
        del W, x32
        torch.cuda.empty_cache()
    if args.one_forward:
        return
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out or os.path.join(ROOT, 'profiles', 'r14_narrow_split.txt'), 'a') as f:
        f.write(text)


def split_trace_table(args):
    """--split --from-trace: the four steps of the route, per layer and width, from the kernel trace of a `--split --one-forward` run (device timestamps).  Every (layer, width)
    ran the route twice (a warm-up call, then the traced one) and a call ends with its matrix-core narrow launch: the second of each pair is reported."""
    import csv
    with open(args.from_trace, newline='') as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r['Start_Timestamp']))
    (calls, cur) = ([], [])
    for r in rows:
        cur.append((r['Kernel_Name'], (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3))
        if 'convtaps_narrow_mfma_kernel' in r['Kernel_Name']:
            calls.append(cur)
            cur = []
    layers = [l for l in SPLIT_LAYERS if not args.layers or l[0] in args.layers]
    routed = lambda Cin, Cout, H, n: not (Cin <= 4 and n > 4 and H * H * ((Cout + 63) // 64) >= 4096)      # (narrow_mfma_loses, csrc/kn_internal.h: those widths have no route and ran nothing)
    want = 2 * sum(1 for (_, Cin, Cout, H, _) in layers for n in SPLIT_IMAGES if routed(Cin, Cout, H, n))
    assert len(calls) == want, 'expected %d route calls in the trace, found %d' % (want, len(calls))
    lines = ['', '== tools/narrow_latency.py --split --from-trace: the steps of ONE narrow split call per layer and width (rocprofv3 --kernel-trace, device timestamps, us)',
             '   %-8s %6s | %12s | %12s | %12s | %12s | %8s | %9s | %s' % ('layer', 'images', '1 X -> Xt', "2 Z' = K Xt", "3 Z' -> Z", '4 Y = op2 Z', 'others', 'sum', 'permute GB/s (steps 1 + 3: bytes read + written)')]
    k = 1
    for (name, Cin, Cout, H, fill) in layers:
        for n in SPLIT_IMAGES:
            if not routed(Cin, Cout, H, n):
                continue
            step = [0.0] * 5
            for (kn, us) in calls[k]:
                if 'planes_columns_kernel<true' in kn or 'planes_columns_kernelILb1' in kn:
                    step[0] += us
                elif 'planes_columns_kernel' in kn:
                    step[2] += us
                elif 'convtaps_narrow_mfma_kernel' in kn:
                    step[3] += us
                elif 'csr' in kn:
                    step[1] += us
                else:
                    step[4] += us
            moved = 2.0 * 4 * Cin * n * (H * H + 9 * H * H)
            lines.append('   %-8s %6d | %12.1f | %12.1f | %12.1f | %12.1f | %8.1f | %9.1f | %.0f' % (name, n, step[0], step[1], step[2], step[3], step[4], sum(step), moved / ((step[0] + step[2]) * 1e-6) / 1e9))
            k += 2
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out or os.path.join(ROOT, 'profiles', 'r14_narrow_split.txt'), 'a') as f:
        f.write(text)


FILL_IMAGES = (1, 8, 16, 32)


def fill_table(args):
    """--fill: per layer shape, in ONE process, on the filled-in synthetic operators of --split, contract exact=True, ReLU fused, at 1, 8, 16 and 32 images:
    (a) torchdot(narrow=True[, narrow32=True]) -- the channel-lane kernels that sum stored values, what such a call ran before; (b) the same call with narrow_fill=True
    (convtaps_narrow_fill_kernel); (c) the padded alternative, torchdot(x128, exact=True) on the batch zero-padded to 128 columns (convtaps_exact_fill_kernel).  Medians of HIP-event
    timings; torch.equal of (b) against (a) and against the first columns of (c).  --one-forward: after one warm-up call, ONE call of (a), (b), (c) per layer and width and
    nothing else (the program for a kernel trace; --fill --from-trace reads it)."""
    import numpy as np
    from keynet_amd import sparse as ksp
    dev = torch.device('cuda:0')
    layers = [l for l in SPLIT_LAYERS if not args.layers or l[0] in args.layers]
    out = args.out or os.path.join(ROOT, 'profiles', 'r16_narrow_fill.txt')
    lines = ['', '== tools/narrow_latency.py --fill: filled-in synthetic operators of the VGG-16 conv shapes, contract exact=True, ReLU fused; %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__),
             '   (a) = torchdot(narrow=True[, narrow32=True]): %d warm-up + median of %d calls;  (b) = the same call with narrow_fill=True: %d + %d calls;  (c) = torchdot(x padded to 128 columns, exact=True): %d + %d calls; HIP events'
             % (1, args.fused_calls, args.warmup, args.forwards, 1, args.fused_calls),
             '   %-8s %4s %4s %4s %5s %9s | %6s | %11s | %11s | %11s | %7s | %7s | %6s | %6s | %s' % ('layer', 'Cin', 'Cout', 'H', 'fill', 'entries', 'images', '(a) [ms]', '(b) [ms]', '(c) [ms]', '(a)/(b)', '(c)/(b)',
                                                                                                 'b == a', 'b == c', 'kernel of (b)')]
    if not args.one_forward:
        with open(out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    for (name, Cin, Cout, H, fill) in layers:
        rng = np.random.RandomState(H + Cin)
        t0 = time.time()
        W = _split_operator(rng, Cin, Cout, H, fill)
        x128 = torch.zeros(W.shape[1], 128, device=dev)
        x128[:, :32] = torch.randn(W.shape[1], 32, device=dev)
        x128[-1, :32] = 1.0
        print('%s built in %.0f s' % (name, time.time() - t0), flush=True)
        with torch.cuda.device(dev):
            op = W._device_op(dev)
        for n in FILL_IMAGES:
            x = x128[:, :n].contiguous()
            xp = x128.clone()
            xp[:, n:] = 0.0
            kw = dict(relu=True, exact=True, narrow=True, narrow32=n > ksp.NARROW_MAX)
            from keynet_amd import _capi
            flags = _capi.KN_FLAG_RELU | _capi.KN_FLAG_EXACT | _capi.KN_FLAG_NARROW | (_capi.KN_FLAG_NARROW32 if n > ksp.NARROW_MAX else 0) | _capi.KN_MODIFIER_NARROW_FILL
            kernel = op.plan(n, flags).split(' (')[0]
            if args.one_forward:
                yb = W.torchdot(x, narrow_fill=True, **kw)       # (warm-up: builds the records)
                torch.cuda.synchronize()
                print('TRACE: %s n=%d' % (name, n), flush=True)
                W.torchdot(x, **kw)
                W.torchdot(x, narrow_fill=True, **kw)
                W.torchdot(xp, relu=True, exact=True)
                torch.cuda.synchronize()
                continue
            yb = W.torchdot(x, narrow_fill=True, **kw)
            tb = timed(lambda: W.torchdot(x, narrow_fill=True, **kw), args.forwards, args.warmup)
            ya = W.torchdot(x, **kw)
            ta = timed(lambda: W.torchdot(x, **kw), args.fused_calls, 0)
            yc = W.torchdot(xp, relu=True, exact=True)
            tc = timed(lambda: W.torchdot(xp, relu=True, exact=True), args.fused_calls, 0)
            (ma, mb, mc) = (statistics.median(ta), statistics.median(tb), statistics.median(tc))
            line = '   %-8s %4d %4d %4d %5d %9d | %6d | %11.3f | %11.3f | %11.3f | %6.2fx | %6.2fx | %6s | %6s | %s' % (
                name, Cin, Cout, H, fill, len(W._taps['ent_out']), n, ma, mb, mc, ma / mb, mc / mb, torch.equal(yb, ya), torch.equal(yb, yc[:, :n]), kernel)
            print(line, flush=True)
            with open(out, 'a') as f:
                f.write(line + '\n')
            del ya, yb, yc
        del W, op, x128
        torch.cuda.empty_cache()


def fill_trace_table(args):
    """--fill --from-trace: the launches of ONE call of (a), (b), (c) per layer and width, from the kernel trace of a `--fill --one-forward` run (device timestamps).  Per
    (layer, width) the run issues a warm-up call of (b) and then (a), (b), (c): the last three launches of a conv-taps main kernel in each group of four are reported."""
    import csv
    with open(args.from_trace, newline='') as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r['Start_Timestamp']))
    main = [(r['Kernel_Name'], (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3) for r in rows
            if any(k in r['Kernel_Name'] for k in ('convtaps_narrow_kernel', 'convtaps_narrow32_kernel', 'convtaps_narrow_fill_kernel', 'convtaps_exact_fill_kernel'))]
    layers = [l for l in SPLIT_LAYERS if not args.layers or l[0] in args.layers]
    assert len(main) == 4 * len(layers) * len(FILL_IMAGES), 'expected %d conv-taps launches in the trace, found %d' % (4 * len(layers) * len(FILL_IMAGES), len(main))
    lines = ['', '== tools/narrow_latency.py --fill --from-trace: ONE launch of (a), (b), (c) per layer and width (rocprofv3 --kernel-trace, device timestamps, us)',
             '   %-8s %6s | %12s | %12s | %12s | %7s | %7s' % ('layer', 'images', '(a)', '(b)', '(c)', '(a)/(b)', '(c)/(b)')]
    k = 0
    for (name, Cin, Cout, H, fill) in layers:
        for n in FILL_IMAGES:
            (a, b, c) = (main[k + 1], main[k + 2], main[k + 3])
            assert 'convtaps_narrow_fill_kernel' in b[0] and 'convtaps_exact_fill_kernel' in c[0] and 'fill' not in a[0], (a[0], b[0], c[0])
            lines.append('   %-8s %6d | %12.1f | %12.1f | %12.1f | %6.2fx | %6.2fx' % (name, n, a[1], b[1], c[1], a[1] / b[1], c[1] / b[1]))
            k += 4
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out or os.path.join(ROOT, 'profiles', 'r16_narrow_fill.txt'), 'a') as f:
        f.write(text)


def narrow32_trace_table(args):
    """--narrow32 --from-trace: the conv launches of the last four forwards of a `--narrow32 --one-forward` run (device timestamps)."""
    import csv
    with open(args.from_trace, newline='') as f:
        rows = [r for r in csv.DictReader(f) if 'convtaps_narrow' in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    k = args.convs
    assert len(rows) >= 4 * k, 'the trace holds %d narrow conv launches, fewer than 4 forwards of %d' % (len(rows), k)
    rows = rows[-4 * k:]
    us = lambda r: (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
    wgs = lambda r: int(r.get('Grid_Size_X') or 0) // max(1, int(r.get('Workgroup_Size_X') or 1))
    short = lambda r: 'matrix-core' if 'mfma' in r['Kernel_Name'] else ('narrow32 ' + r['Kernel_Name'].split('<')[1].split('>')[0] if '<' in r['Kernel_Name'] else 'narrow32')
    lines = ['', "== tools/narrow_latency.py --narrow32 --from-trace: the conv launches of one narrow=True and one narrow='mfma' forward with narrow32=True (rocprofv3 --kernel-trace, device timestamps)"]
    for (i, n) in enumerate((16, 32)):
        (lane, mfma) = (rows[(2 * i) * k:(2 * i + 1) * k], rows[(2 * i + 1) * k:(2 * i + 2) * k])
        assert all('mfma' not in r['Kernel_Name'] for r in lane), 'the narrow=True forward launched a matrix-core kernel'
        lines.append('')
        lines.append("   %d images [us]: conv launch | workgroups, channel-lane | channel-lane | workgroups, narrow='mfma' | narrow='mfma' | ratio | kernels" % n)
        for (j, (a, b)) in enumerate(zip(lane, mfma)):
            lines.append('     %2d | %6d | %9.1f | %6d | %9.1f | %5.2fx | %s / %s' % (j + 1, wgs(a), us(a), wgs(b), us(b), us(a) / us(b), short(a), short(b)))
        (sa, sb) = (sum(us(r) for r in lane), sum(us(r) for r in mfma))
        lines.append('     sum of the %d conv launches: %9.1f | %9.1f | %5.2fx' % (k, sa, sb, sa / sb))
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out or os.path.join(ROOT, 'profiles', 'r10_narrow32.txt'), 'a') as f:
        f.write(text)


def rows_table(args, knet, xc, desc):
    """--rows: see the module docstring."""
    dev = xc.device
    if args.one_forward:
        for n in (1, 2, 4, 8):                    # operators resident
            knet.forward_linear(xc[:n].t().contiguous().t(), narrow=True, narrow_rows=True)
        torch.cuda.synchronize()
        print('TRACE-FROM-HERE: for n in (1, 2, 4, 8) one narrow=True forward, then one with narrow_rows=True', flush=True)
        for n in (1, 2, 4, 8):
            x = xc[:n].t().contiguous().t()
            knet.forward_linear(x, narrow=True)
            knet.forward_linear(x, narrow=True, narrow_rows=True)
            torch.cuda.synchronize()
        return
    med = lambda v: '%8.3f (%.3f .. %.3f)' % (statistics.median(v), min(v), max(v))
    lines = ['', '== tools/narrow_latency.py --rows: %s' % desc,
             '   %s, torch %s; HIP events, %d warm-up + median of %d forwards (min .. max), the two forms alternating; logits torch.equal: yes'
             % (torch.cuda.get_device_name(0), torch.__version__, args.warmup, args.forwards)]

    def forwards(mode, title):
        lines.append('   %s' % title)
        lines.append('   %6s | %-28s | %-28s | %s' % ('images', 'narrow=%r [ms]' % (mode,), '+ narrow_rows=True [ms]', 'without / with'))
        for n in (1, 2, 4, 8):
            x = xc[:n].t().contiguous().t()
            (y0, y1) = (knet.forward_linear(x, narrow=mode), knet.forward_linear(x, narrow=mode, narrow_rows=True))
            torch.cuda.synchronize()
            assert torch.equal(y0, y1), 'narrow_rows changed the logits at %d image(s), narrow=%r' % (n, mode)
            (a, b) = ([], [])
            for _ in range(4):                    # alternate in quarters
                a += timed(lambda: knet.forward_linear(x, narrow=mode), args.forwards // 4, args.warmup)
                b += timed(lambda: knet.forward_linear(x, narrow=mode, narrow_rows=True), args.forwards // 4, args.warmup)
            lines.append('   %6d | %-28s | %-28s | %.2fx' % (n, med(a), med(b), statistics.median(a) / statistics.median(b)))
            print('narrow=%r n = %d done' % (mode, n), flush=True)

    forwards(True, 'whole forwards, default contract')
    lines.append('')
    widths = (1, 2, 3, 4, 5, 6, 7, 8)
    lines.append('   every layer that carries KN_FLAG_NARROW_ROWS, alone: kn_spmm on one block, without / with the flag [us] and their ratio; "=" where the handle rule')
    lines.append('   keeps the kernels of the call without the flag (the same plan string)')
    lines.append('   %-10s %-16s | %s' % ('layer', 'rows x cols', ' | '.join('%d image(s)%s' % (n, ' ' * 11) for n in widths)))
    st = torch.cuda.current_stream().cuda_stream
    sums = dict((n, [0.0, 0.0]) for n in widths)
    for (name, c) in knet._keyed(named=True):
        (la0, la1) = (c.launch(dev, narrow=True), c.launch(dev, narrow=True, narrow_rows=True))
        if la1 is None or la1.flags == la0.flags:
            continue
        cells = []
        for n in widths:
            x = torch.randn((la1.cols, n), device=dev)
            y = torch.empty((la1.rows, n), device=dev)
            same = la1.op.plan(n, la1.flags) == la0.op.plan(n, la0.flags)
            (a, b) = ([], [])
            for _ in range(2):
                a += timed(lambda: la0.op.spmm(x.data_ptr(), n, n, y.data_ptr(), n, la0.flags, st), args.forwards, args.warmup)
                b += timed(lambda: la1.op.spmm(x.data_ptr(), n, n, y.data_ptr(), n, la1.flags, st), args.forwards, args.warmup)
            (ma, mb) = (statistics.median(a) * 1e3, statistics.median(b) * 1e3)
            sums[n][0] += ma
            sums[n][1] += mb
            cells.append('%7.1f %7.1f %s' % (ma, mb, '    =' if same else '%4.2fx' % (ma / mb)))
        lines.append('   %-10s %-16s | %s' % (name, '%d x %d' % (la1.rows, la1.cols), ' | '.join(cells)))
        lines.append('   %-10s %-16s   %s' % ('', '', la1.op.plan(1, la1.flags)))
    lines.append('   %-10s %-16s | %s' % ('sum', '', ' | '.join('%7.1f %7.1f %4.2fx' % (sums[n][0], sums[n][1], sums[n][0] / max(sums[n][1], 1e-9)) for n in widths)))
    lines.append('')
    knet.exact_mode('auto')
    knet.forward_linear(xc)                       # the calibrating wide forward
    forwards('mfma', "whole forwards, exact_mode('auto') after one calibrating wide forward")
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out or os.path.join(ROOT, 'profiles', 'r09_narrow_rows.txt'), 'a') as f:
        f.write(text)


LINEAR_WIDTHS = (1, 2, 3, 4, 8, 16, 32, 33, 64)
LINEAR_IMAGES = (1, 8, 16, 64)


def _width_keywords(n):
    return dict(narrow=True, narrow32=n > 8, narrow64=n > 32)


def linear_table(args, knet, xc, desc):
    """--linear: see the module docstring."""
    from keynet_amd import _capi
    dev = xc.device
    (ROWS, LINEAR) = (_capi.KN_FLAG_NARROW_ROWS, _capi.KN_FLAG_NARROW_LINEAR)
    if args.one_forward:
        for n in LINEAR_IMAGES:                   # operators resident
            knet.forward_linear(xc[:n].t().contiguous().t(), narrow_linear=True, **_width_keywords(n))
        torch.cuda.synchronize()
        print('TRACE-FROM-HERE: for n in (1, 8, 16, 64) one narrow=True forward with the width\'s keywords, then one with narrow_linear=True', flush=True)
        for n in LINEAR_IMAGES:
            x = xc[:n].t().contiguous().t()
            knet.forward_linear(x, **_width_keywords(n))
            knet.forward_linear(x, narrow_linear=True, **_width_keywords(n))
            torch.cuda.synchronize()
        return
    med = lambda v: '%8.3f (%.3f .. %.3f)' % (statistics.median(v), min(v), max(v))
    lines = ['', '== tools/narrow_latency.py --linear: %s' % desc,
             '   %s, torch %s; HIP events, %d warm-up + median of %d calls (min .. max), the forms alternating; logits torch.equal: yes'
             % (torch.cuda.get_device_name(0), torch.__version__, args.warmup, args.forwards)]
    st = torch.cuda.current_stream().cuda_stream
    flush = torch.empty(128 << 20, dtype=torch.float32, device=dev)     # 512 MB: twice the Infinity Cache

    def cold(fn, calls):
        out = []
        for _ in range(calls):
            flush.zero_()
            (a, b) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        return out

    linears = []
    for (name, c) in knet._keyed(named=True):
        (la0, la1) = (c.launch(dev, narrow=True), c.launch(dev, narrow=True, narrow_linear=True))
        if la1 is not None and la1.flags != la0.flags and 'csr_stream_group_kernel' in la1.op.plan(1, la1.flags):
            linears.append((name, la0))
    lines.append('   the layers with big pattern groups, alone: kn_spmm [us] without the flag | with KN_FLAG_NARROW_LINEAR (ratio) and, up to 8 columns, with KN_FLAG_NARROW_ROWS |')
    lines.append('   with both (ratio to KN_FLAG_NARROW_ROWS alone); first line back to back on one block, second line behind a pass over 512 MB (cold values)')
    for (name, la) in linears:
        lines.append('   %s  %d x %d' % (name, la.rows, la.cols))
        for n in LINEAR_WIDTHS:
            x = torch.randn((la.cols, n), device=dev)
            ys = [torch.empty((la.rows, n), device=dev) for _ in range(2)]
            forms = [la.flags, la.flags | LINEAR] + ([la.flags | ROWS, la.flags | ROWS | LINEAR] if n <= 8 else [])
            calls = [(lambda f=f, y=ys[i & 1]: la.op.spmm(x.data_ptr(), n, n, y.data_ptr(), n, f, st)) for (i, f) in enumerate(forms)]
            for k in range(0, len(forms), 2):
                calls[k]()
                calls[k + 1]()
                torch.cuda.synchronize()
                assert torch.equal(ys[0], ys[1]), 'KN_FLAG_NARROW_LINEAR changed the bits of %s at %d column(s)' % (name, n)
            (warm, cool) = ([[] for _ in forms], [[] for _ in forms])
            for _ in range(2):
                for (k, fn) in enumerate(calls):
                    warm[k] += timed(fn, args.forwards // 2, args.warmup)
                    cool[k] += cold(fn, args.forwards // 2)
            for (tag, t) in (('warm', warm), ('cold', cool)):
                m = [statistics.median(v) * 1e3 for v in t]
                cell = '%8.1f | %8.1f (%4.2fx)' % (m[0], m[1], m[0] / m[1])
                if n <= 8:
                    cell += ' | %8.1f | %8.1f (%4.2fx)' % (m[2], m[3], m[2] / m[3])
                lines.append('     %2d column(s) %s: %s' % (n, tag, cell))
            lines.append('        %s' % la.op.plan(n, la.flags | LINEAR))
            if n <= 8:
                lines.append('        %s' % la.op.plan(n, la.flags | ROWS | LINEAR))
        print('%s done' % name, flush=True)
    lines.append('')
    lines.append('   whole forwards, default contract, narrow=True with the width\'s keywords')
    lines.append('   %6s | %-28s | %-28s | %s' % ('images', 'without [ms]', '+ narrow_linear=True [ms]', 'without / with'))
    for n in LINEAR_IMAGES:
        x = xc[:n].t().contiguous().t()
        kw = _width_keywords(n)
        (y0, y1) = (knet.forward_linear(x, **kw), knet.forward_linear(x, narrow_linear=True, **kw))
        torch.cuda.synchronize()
        assert torch.equal(y0, y1), 'narrow_linear changed the logits at %d image(s)' % n
        (a, b) = ([], [])
        for _ in range(4):                        # alternate in quarters
            a += timed(lambda: knet.forward_linear(x, **kw), args.forwards // 4, args.warmup)
            b += timed(lambda: knet.forward_linear(x, narrow_linear=True, **kw), args.forwards // 4, args.warmup)
        lines.append('   %6d | %-28s | %-28s | %.2fx' % (n, med(a), med(b), statistics.median(a) / statistics.median(b)))
        print('n = %d done' % n, flush=True)
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out or os.path.join(ROOT, 'profiles', 'r13_narrow_linear.txt'), 'a') as f:
        f.write(text)


def linear_trace_table(args):
    """--linear --from-trace: the CSR launches (fc6 - fc8 and the pools, with their helpers) of the last eight forwards of a `--linear --one-forward` run."""
    import csv
    with open(args.from_trace, newline='') as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r['Start_Timestamp']))
    first = next(i for (i, r) in enumerate(rows) if 'convtaps' in r['Kernel_Name'])
    (fw, seen) = ([[]], 0)
    for r in rows[first:]:                        # a forward = its k conv launches and the launches between and behind them, up to the next conv launch
        conv = 'convtaps' in r['Kernel_Name']
        if conv and seen == args.convs:
            fw.append([])
            seen = 0
        seen += conv
        fw[-1].append(r)
    fw = fw[-8:]
    assert len(fw) == 8, 'the trace holds %d forwards, fewer than 8' % len(fw)
    us = lambda r: (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
    big = lambda r: any(k in r['Kernel_Name'] for k in ('csr_big_group', 'csr_stream_group', 'mfma16'))
    lines = ['', '== tools/narrow_latency.py --linear --from-trace: the launches of fc6 - fc8 and the pools (with their helpers) in one narrow=True forward and one with narrow_linear=True (rocprofv3 --kernel-trace)']
    for (i, n) in enumerate(LINEAR_IMAGES):
        (a, b) = [[r for r in f if 'kn::' in r['Kernel_Name'] and 'conv' not in r['Kernel_Name']] for f in (fw[2 * i], fw[2 * i + 1])]
        lines.append('')
        lines.append('   %d image(s) [us]: without narrow_linear | with narrow_linear' % n)
        for j in range(max(len(a), len(b))):
            cell = lambda L: ('%9.1f %-60s' % (us(L[j]), L[j]['Kernel_Name'][:60])) if j < len(L) else ' ' * 70
            lines.append('     %s | %s' % (cell(a), cell(b)))
        (sa, sb) = (sum(us(r) for r in a if big(r)), sum(us(r) for r in b if big(r)))
        lines.append('     sum of the big-group launches (fc6 - fc8): %9.1f | %9.1f | %5.2fx' % (sa, sb, sa / max(sb, 1e-9)))
        (wa, wb) = [(int(f[-1]['End_Timestamp']) - int(f[0]['Start_Timestamp'])) / 1e3 for f in (fw[2 * i], fw[2 * i + 1])]
        lines.append('     first launch to last launch of the forward:  %9.1f | %9.1f | %5.2fx' % (wa, wb, wa / max(wb, 1e-9)))
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out or os.path.join(ROOT, 'profiles', 'r13_narrow_linear.txt'), 'a') as f:
        f.write(text)


def rows_trace_table(args):
    """--rows --from-trace: the NON-conv launches of the last eight forwards of a `--rows --one-forward` run (device timestamps), forward by forward."""
    import csv
    with open(args.from_trace, newline='') as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r['Start_Timestamp']))
    first = next(i for (i, r) in enumerate(rows) if 'convtaps' in r['Kernel_Name'])
    (fw, seen) = ([[]], 0)
    for r in rows[first:]:                        # a forward = its k conv launches and the launches between and behind them, up to the next conv launch
        conv = 'convtaps' in r['Kernel_Name']
        if conv and seen == args.convs:
            fw.append([])
            seen = 0
        seen += conv
        fw[-1].append(r)
    fw = fw[-8:]
    assert len(fw) == 8, 'the trace holds %d forwards, fewer than 8' % len(fw)
    us = lambda r: (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
    lines = ['', '== tools/narrow_latency.py --rows --from-trace: the launches of fc6 - fc8 and the pools (with their helpers) in one narrow=True forward and one with narrow_rows=True (rocprofv3 --kernel-trace)']
    for (i, n) in enumerate((1, 2, 4, 8)):
        # (the conv launches' own helper, conv_lastrow_kernel, and torch's copy kernels between two forwards are neither fc nor pool launches)
        (a, b) = [[r for r in f if 'kn::' in r['Kernel_Name'] and 'conv' not in r['Kernel_Name']] for f in (fw[2 * i], fw[2 * i + 1])]
        lines.append('')
        lines.append('   %d image(s) [us]: without narrow_rows | with narrow_rows' % n)
        for j in range(max(len(a), len(b))):
            cell = lambda L: ('%9.1f %-60s' % (us(L[j]), L[j]['Kernel_Name'][:60])) if j < len(L) else ' ' * 70
            lines.append('     %s | %s' % (cell(a), cell(b)))
        (sa, sb) = (sum(us(r) for r in a), sum(us(r) for r in b))
        lines.append('     sum of the non-conv launches: %9.1f | %9.1f | %5.2fx' % (sa, sb, sa / max(sb, 1e-9)))
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out or os.path.join(ROOT, 'profiles', 'r09_narrow_rows.txt'), 'a') as f:
        f.write(text)


TAPS_FORM = dict(narrow=True, narrow_rows=True, narrow_linear=True)


def taps_table(args, knet, xc, desc):
    """--taps: see the module docstring."""
    if args.one_forward:
        for n in (1, 2, 4, 8):
            x = xc[:n].t().contiguous().t()
            for kw in (dict(), dict(narrow_taps=True)):
                knet.forward_linear(x, **TAPS_FORM, **kw)      # (operators resident, kernels loaded)
            torch.cuda.synchronize()
        print('TRACE-FROM-HERE: for n in (1, 2, 4, 8) one narrow forward, then one with narrow_taps=True', flush=True)
        for n in (1, 2, 4, 8):
            x = xc[:n].t().contiguous().t()
            for kw in (dict(), dict(narrow_taps=True)):
                knet.forward_linear(x, **TAPS_FORM, **kw)
                torch.cuda.synchronize()
        return
    rows = []
    for n in (1, 2, 4, 8):
        x = xc[:n].t().contiguous().t()
        (plain, taps) = (knet.forward_linear(x, **TAPS_FORM), knet.forward_linear(x, narrow_taps=True, **TAPS_FORM))
        torch.cuda.synchronize()
        assert torch.equal(plain, taps), 'narrow_taps logits differ at %d image(s): max %g' % (n, float((plain - taps).abs().max()))
        t = ([], [])
        for _ in range(2):                        # the forms alternating, two rounds of --forwards / 2 each
            t[0].extend(timed(lambda: knet.forward_linear(x, **TAPS_FORM), args.forwards // 2, args.warmup))
            t[1].extend(timed(lambda: knet.forward_linear(x, narrow_taps=True, **TAPS_FORM), args.forwards // 2, args.warmup))
        rows.append((n, [(statistics.median(v), min(v), max(v)) for v in t]))
        print('n = %d done' % n, flush=True)
    lines = ['', '== tools/narrow_latency.py --taps --workload %s: %s' % (args.workload, desc),
             '   %s, torch %s; HIP events, %d warm-up + median of %d forwards (min .. max), forms alternating; logits torch.equal: yes'
             % (torch.cuda.get_device_name(0), torch.__version__, args.warmup, args.forwards),
             '   %6s | %-34s | %-34s | %s' % ('images', 'narrow, narrow_rows, narrow_linear [ms]', '... and narrow_taps=True [ms]', 'ratio')]
    for (n, t) in rows:
        cell = ['%8.3f (%.3f .. %.3f)' % v for v in t]
        lines.append('   %6d | %-34s | %-34s | %.2fx' % (n, cell[0], cell[1], t[0][0] / t[1][0]))
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out or os.path.join(ROOT, 'profiles', 'r15_narrow_taps.txt'), 'a') as f:
        f.write(text)


def taps_trace_table(args):
    """--taps --from-trace: the conv launches of the last eight forwards of a `--taps --one-forward` run under rocprofv3 --kernel-trace (device timestamps)."""
    import csv
    with open(args.from_trace, newline='') as f:
        rows = [r for r in csv.DictReader(f) if 'convtaps_narrow' in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    k = args.convs
    assert len(rows) >= 8 * k, 'the trace holds %d narrow conv launches, fewer than 8 forwards of %d' % (len(rows), k)
    rows = rows[-8 * k:]
    us = lambda r: (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
    lines = ['', '== tools/narrow_latency.py --taps --from-trace: the conv launches of one narrow forward and one with narrow_taps=True (rocprofv3 --kernel-trace, device timestamps)']
    for (i, n) in enumerate((1, 2, 4, 8)):
        (old, new) = (rows[(2 * i) * k:(2 * i + 1) * k], rows[(2 * i + 1) * k:(2 * i + 2) * k])
        assert all('narrow_taps' not in r['Kernel_Name'] for r in old), 'the forward without the keyword launched the tap-resident kernel'
        lines.append('')
        lines.append('   %d image(s) [us]: conv launch | workgroups | convtaps_narrow_kernel | with narrow_taps | ratio | kernel of the narrow_taps forward' % n)
        for (j, (a, b)) in enumerate(zip(old, new)):
            name = b['Kernel_Name']
            form = name[name.index('<'):name.index('>') + 1] if ('narrow_taps' in name and '<' in name and '>' in name) else ''
            lines.append('     %2d | %6d | %9.1f | %9.1f | %5.2fx | %s' % (j + 1, int(b.get('Grid_Size_X') or 0) // max(1, int(b.get('Workgroup_Size_X') or 1)), us(a), us(b), us(a) / us(b),
                                                                  ('taps resident <NT, P, NV, FULL, COEF> = ' + form) if 'narrow_taps' in name else 'channel-lane'))
        (sa, sb) = (sum(us(r) for r in old), sum(us(r) for r in new))
        lines.append('     sum of the %d conv launches: %9.1f | %9.1f | %5.2fx' % (k, sa, sb, sa / sb))
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out or os.path.join(ROOT, 'profiles', 'r15_narrow_taps.txt'), 'a') as f:
        f.write(text)


PAIRS_FORM = dict(narrow=True, narrow_rows=True, narrow_linear=True)
PAIRS_IMAGES = (1, 2, 4, 8)
PAIRS_REPEATS = 3                                 # traced forwards per form and width: a launch's min .. max spread


def pairs_table(args, knet, xc, desc):
    """--pairs: see the module docstring."""
    forms = (dict(narrow_taps=True), dict(narrow_taps='pairs'))
    if args.one_forward:
        for n in PAIRS_IMAGES:
            x = xc[:n].t().contiguous().t()
            for kw in forms:
                knet.forward_linear(x, **PAIRS_FORM, **kw)      # (operators resident, kernels loaded)
            torch.cuda.synchronize()
        print('TRACE-FROM-HERE: for n in (1, 2, 4, 8) %d times one forward with narrow_taps=True, then one with narrow_taps=\'pairs\'' % PAIRS_REPEATS, flush=True)
        for n in PAIRS_IMAGES:
            x = xc[:n].t().contiguous().t()
            for _ in range(PAIRS_REPEATS):
                for kw in forms:
                    knet.forward_linear(x, **PAIRS_FORM, **kw)
                    torch.cuda.synchronize()
        return
    rows = []
    for n in PAIRS_IMAGES:
        x = xc[:n].t().contiguous().t()
        (taps, pairs) = (knet.forward_linear(x, **PAIRS_FORM, **forms[0]), knet.forward_linear(x, **PAIRS_FORM, **forms[1]))
        torch.cuda.synchronize()
        assert torch.equal(taps, pairs), 'narrow_taps=\'pairs\' logits differ at %d image(s): max %g' % (n, float((taps - pairs).abs().max()))
        t = ([], [])
        for _ in range(2):                        # the forms alternating, two rounds of --forwards / 2 each
            t[0].extend(timed(lambda: knet.forward_linear(x, **PAIRS_FORM, **forms[0]), args.forwards // 2, args.warmup))
            t[1].extend(timed(lambda: knet.forward_linear(x, **PAIRS_FORM, **forms[1]), args.forwards // 2, args.warmup))
        rows.append((n, [(statistics.median(v), min(v), max(v)) for v in t]))
        print('n = %d done' % n, flush=True)
    lines = ['', '== tools/narrow_latency.py --pairs --workload %s: %s' % (args.workload, desc),
             '   %s, torch %s; HIP events, %d warm-up + median of %d forwards (min .. max), forms alternating; logits torch.equal: yes'
             % (torch.cuda.get_device_name(0), torch.__version__, args.warmup, args.forwards),
             '   %6s | %-34s | %-34s | %s' % ('images', '... narrow_taps=True [ms]', '... narrow_taps=\'pairs\' [ms]', 'ratio | gain [ms] against the two spreads added [ms]')]
    for (n, t) in rows:
        cell = ['%8.3f (%.3f .. %.3f)' % v for v in t]
        (gain, spreads) = (t[0][0] - t[1][0], (t[0][2] - t[0][1]) + (t[1][2] - t[1][1]))
        lines.append('   %6d | %-34s | %-34s | %.2fx | %.3f against %.3f' % (n, cell[0], cell[1], t[0][0] / t[1][0], gain, spreads))
    if args.workload == 'vgg16':
        one = rows[0][1][1][0]
        lines.append('   one image with narrow_taps=\'pairs\': %.3f ms against the 4 ms target: %s' % (one, 'MET' if one <= 4.0 else 'MISSED'))
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out or os.path.join(ROOT, 'profiles', 'r18_narrow_taps_pairs.txt'), 'a') as f:
        f.write(text)


def pairs_trace_table(args):
    """--pairs --from-trace: the conv launches of the last 8 x PAIRS_REPEATS forwards of a `--pairs --one-forward` run under rocprofv3 --kernel-trace (device
    timestamps): per launch the median of the repeats with min .. max on both sides, and the rule of narrow_taps_pairs_loses -- a (layer, width) stays on the new
    kernel only where the gain exceeds the two spreads added."""
    import csv
    with open(args.from_trace, newline='') as f:
        rows = [r for r in csv.DictReader(f) if 'convtaps_narrow' in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    (k, reps) = (args.convs, PAIRS_REPEATS)
    assert len(rows) >= 8 * reps * k, 'the trace holds %d narrow conv launches, fewer than %d forwards of %d' % (len(rows), 8 * reps, k)
    rows = rows[-8 * reps * k:]
    us = lambda r: (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
    stat = lambda v: (statistics.median(v), min(v), max(v))
    lines = ['', '== tools/narrow_latency.py --pairs --from-trace: the conv launches of %d forwards with narrow_taps=True and %d with narrow_taps=\'pairs\', alternating (rocprofv3 --kernel-trace, device timestamps)' % (reps, reps)]
    for (i, n) in enumerate(PAIRS_IMAGES):
        fw = [rows[(2 * reps * i + j) * k:(2 * reps * i + j + 1) * k] for j in range(2 * reps)]
        (old, new) = (fw[0::2], fw[1::2])
        assert all('taps_pairs' not in r['Kernel_Name'] for f_ in old for r in f_), 'the narrow_taps=True forward launched the channel-pair kernel'
        lines.append('')
        lines.append('   %d image(s) [us, median (min .. max) of %d]: conv launch | workgroups | convtaps_narrow_taps_kernel | with narrow_taps=\'pairs\' | ratio | gain against the two spreads added | kernel of the pairs forward' % (n, reps))
        (sa, sb) = (0.0, 0.0)
        for j in range(k):
            (a, b) = (stat([us(f_[j]) for f_ in old]), stat([us(f_[j]) for f_ in new]))
            r = new[0][j]
            name = r['Kernel_Name']
            mine = 'taps_pairs' in name
            form = name[name.index('<'):name.index('>') + 1] if ('<' in name and '>' in name) else ''
            (gain, spreads) = (a[0] - b[0], (a[2] - a[1]) + (b[2] - b[1]))
            lines.append('     %2d | %6d | %8.1f (%.1f .. %.1f) | %8.1f (%.1f .. %.1f) | %5.2fx | %7.1f against %6.1f%s | %s' % (
                (j + 1, int(r.get('Grid_Size_X') or 0) // max(1, int(r.get('Workgroup_Size_X') or 1))) + a + b + (a[0] / b[0], gain, spreads, ('' if not mine else ': WINS' if gain > spreads else ': LOSES'),
                                                                                                                    ('two channels per lane <NT, NV, FULL, COEF> = ' if mine else 'convtaps_narrow_taps_kernel <NT, P, NV, FULL, COEF> = ') + form)))
            sa += a[0]
            sb += b[0]
        lines.append('     sum of the %d conv launches (medians): %9.1f | %9.1f | %5.2fx' % (k, sa, sb, sa / sb))
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out or os.path.join(ROOT, 'profiles', 'r18_narrow_taps_pairs.txt'), 'a') as f:
        f.write(text)


TAPS32_FORM = dict(narrow=True, narrow32=True, narrow_linear=True)
TAPS32_IMAGES = (9, 12, 16, 24, 32)
TAPS32_TRACED = (16, 32)


def taps32_table(args, knet, xc, desc):
    """--taps32: see the module docstring."""
    images = TAPS32_IMAGES if args.workload == 'vgg16' else (16,)
    if args.one_forward:
        for n in TAPS32_TRACED:
            x = xc[:n].t().contiguous().t()
            for kw in (dict(), dict(narrow_taps='packed')):
                knet.forward_linear(x, **TAPS32_FORM, **kw)      # (operators resident, kernels loaded)
            torch.cuda.synchronize()
        print('TRACE-FROM-HERE: for n in (16, 32) one narrow32 forward, then one with narrow_taps=\'packed\'', flush=True)
        for n in TAPS32_TRACED:
            x = xc[:n].t().contiguous().t()
            for kw in (dict(), dict(narrow_taps='packed')):
                knet.forward_linear(x, **TAPS32_FORM, **kw)
                torch.cuda.synchronize()
        return
    rows = []
    for n in images:
        x = xc[:n].t().contiguous().t()
        (plain, packed) = (knet.forward_linear(x, **TAPS32_FORM), knet.forward_linear(x, narrow_taps='packed', **TAPS32_FORM))
        torch.cuda.synchronize()
        assert torch.equal(plain, packed), 'narrow_taps=\'packed\' logits differ at %d images: max %g' % (n, float((plain - packed).abs().max()))
        t = ([], [])
        for _ in range(2):                        # the forms alternating, two rounds of --forwards / 2 each
            t[0].extend(timed(lambda: knet.forward_linear(x, **TAPS32_FORM), args.forwards // 2, args.warmup))
            t[1].extend(timed(lambda: knet.forward_linear(x, narrow_taps='packed', **TAPS32_FORM), args.forwards // 2, args.warmup))
        rows.append((n, [(statistics.median(v), min(v), max(v)) for v in t]))
        print('n = %d done' % n, flush=True)
    x8 = xc[:8].t().contiguous().t()              # the best bit-exact 8-image forward, in this process
    v8 = timed(lambda: knet.forward_linear(x8, narrow_taps=True, **TAPS_FORM), args.forwards, args.warmup)
    t8 = (statistics.median(v8), min(v8), max(v8))
    lines = ['', '== tools/narrow_latency.py --taps32 --workload %s: %s' % (args.workload, desc),
             '   %s, torch %s; HIP events, %d warm-up + median of %d forwards (min .. max), forms alternating; logits torch.equal: yes'
             % (torch.cuda.get_device_name(0), torch.__version__, args.warmup, args.forwards),
             '   %6s | %-34s | %-34s | %s' % ('images', 'narrow, narrow32, narrow_linear [ms]', '... and narrow_taps=\'packed\' [ms]', 'ratio | gain [ms] against the two spreads added [ms]')]
    for (n, t) in rows:
        cell = ['%8.3f (%.3f .. %.3f)' % v for v in t]
        (gain, spreads) = (t[0][0] - t[1][0], (t[0][2] - t[0][1]) + (t[1][2] - t[1][1]))
        lines.append('   %6d | %-34s | %-34s | %.2fx | %.3f against %.3f%s' % (n, cell[0], cell[1], t[0][0] / t[1][0], gain, spreads,
                                                                             '' if (n not in TAPS32_TRACED or args.workload != 'vgg16') else (': bar MET' if gain > spreads else ': bar MISSED')))
    lines.append('   %6d | narrow, narrow_rows, narrow_linear, narrow_taps=True [ms]: %8.3f (%.3f .. %.3f)' % ((8,) + t8))
    for (n, t) in rows:
        if n == 16 and args.workload == 'vgg16':
            lines.append('   16 images packed %.3f ms against twice the 8-image forward %.3f ms: bar %s' % (t[1][0], 2 * t8[0], 'MET' if t[1][0] <= 2 * t8[0] else 'MISSED'))
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out or os.path.join(ROOT, 'profiles', 'r17_narrow_taps32.txt'), 'a') as f:
        f.write(text)


def taps32_trace_table(args):
    """--taps32 --from-trace: the conv launches of the last four forwards of a `--taps32 --one-forward` run under rocprofv3 --kernel-trace (device timestamps)."""
    import csv
    with open(args.from_trace, newline='') as f:
        rows = [r for r in csv.DictReader(f) if 'convtaps_narrow' in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    k = args.convs
    assert len(rows) >= 4 * k, 'the trace holds %d narrow conv launches, fewer than 4 forwards of %d' % (len(rows), k)
    rows = rows[-4 * k:]
    us = lambda r: (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
    lines = ['', '== tools/narrow_latency.py --taps32 --from-trace: the conv launches of one narrow32 forward and one with narrow_taps=\'packed\' (rocprofv3 --kernel-trace, device timestamps)']
    for (i, n) in enumerate(TAPS32_TRACED):
        (old, new) = (rows[(2 * i) * k:(2 * i + 1) * k], rows[(2 * i + 1) * k:(2 * i + 2) * k])
        assert all('narrow_taps32' not in r['Kernel_Name'] for r in old), 'the forward without the keyword launched the packed tap-resident kernel'
        lines.append('')
        lines.append('   %d images [us]: conv launch | workgroups | convtaps_narrow32_kernel | with narrow_taps=\'packed\' | ratio | kernel of the packed forward' % n)
        for (j, (a, b)) in enumerate(zip(old, new)):
            name = b['Kernel_Name']
            form = name[name.index('<'):name.index('>') + 1] if ('narrow_taps32' in name and '<' in name and '>' in name) else ''
            lines.append('     %2d | %6d | %9.1f | %9.1f | %5.2fx | %s%s' % (j + 1, int(b.get('Grid_Size_X') or 0) // max(1, int(b.get('Workgroup_Size_X') or 1)), us(a), us(b), us(a) / us(b),
                                                                    ('taps resident, packed <NT, NV, FULL, COEF> = ' + form) if 'narrow_taps32' in name else 'convtaps_narrow32_kernel',
                                                                    ' -- SLOWER' if 'narrow_taps32' in name and us(b) > us(a) else ''))
        (sa, sb) = (sum(us(r) for r in old), sum(us(r) for r in new))
        lines.append('     sum of the %d conv launches: %9.1f | %9.1f | %5.2fx' % (k, sa, sb, sa / sb))
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out or os.path.join(ROOT, 'profiles', 'r17_narrow_taps32.txt'), 'a') as f:
        f.write(text)


def trace_table(args):
    """--from-trace: the conv launches of the last eight forwards of a `--mfma --one-forward` run under rocprofv3 --kernel-trace (device timestamps)."""
    import csv
    with open(args.from_trace, newline='') as f:
        rows = [r for r in csv.DictReader(f) if 'convtaps_narrow' in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    k = args.convs
    assert len(rows) >= 8 * k, 'the trace holds %d narrow conv launches, fewer than 8 forwards of %d' % (len(rows), k)
    rows = rows[-8 * k:]
    lines = ['', '== tools/narrow_latency.py --from-trace: the conv launches of one narrow=True and one narrow=\'mfma\' forward (rocprofv3 --kernel-trace, device timestamps)']
    for (i, n) in enumerate((1, 2, 4, 8)):
        (lane, mfma) = (rows[(2 * i) * k:(2 * i + 1) * k], rows[(2 * i + 1) * k:(2 * i + 2) * k])
        assert all('mfma' not in r['Kernel_Name'] for r in lane), 'the narrow=True forward launched a matrix-core kernel'
        lines.append('')
        lines.append('   %d image(s) [us]: conv launch | workgroups | channel-lane | narrow=\'mfma\' | ratio | kernel of the narrow=\'mfma\' forward' % n)
        us = lambda r: (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
        for (j, (a, b)) in enumerate(zip(lane, mfma)):
            lines.append('     %2d | %6d | %9.1f | %9.1f | %5.2fx | %s' % (j + 1, int(b.get('Grid_Size_X') or 0) // max(1, int(b.get('Workgroup_Size_X') or 1)), us(a), us(b), us(a) / us(b),
                                                                  'matrix-core' if 'mfma' in b['Kernel_Name'] else 'channel-lane'))
        (sa, sb) = (sum(us(r) for r in lane), sum(us(r) for r in mfma))
        lines.append('     sum of the %d conv launches: %9.1f | %9.1f | %5.2fx' % (k, sa, sb, sa / sb))
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out or os.path.join(ROOT, 'profiles', 'r08_narrow_mfma.txt'), 'a') as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='vgg16', choices=['vgg16', 'allconv'])
    ap.add_argument('--forwards', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None, help='the file the table is appended to (default: profiles/r07_narrow_forward.txt, with --mfma or --from-trace profiles/r08_narrow_mfma.txt)')
    ap.add_argument('--from-trace', default=None, help='a *_kernel_trace.csv of a --mfma --one-forward run: print its conv launches, layer by layer (no GPU)')
    ap.add_argument('--convs', type=int, default=13, help='conv layers per forward in --from-trace')
    ap.add_argument('--linears', type=int, default=0, help='with --from-trace: keyed nn.Linear layers per forward that launch the conv-taps tile kernel as split-K (VGG-16 under the tolerance contract: 3)')
    ap.add_argument('--one-forward', action='store_true', help='key, warm up, run one narrow forward and exit (for a kernel trace)')
    ap.add_argument('-n', type=int, default=1, help='images of --one-forward')
    ap.add_argument('--rows', action='store_true', help='whole forwards and single layers with and without narrow_rows=True (profiles/r09_narrow_rows.txt)')
    ap.add_argument('--linear', action='store_true', help='fc6 - fc8 alone and whole forwards with and without narrow_linear=True (profiles/r13_narrow_linear.txt)')
    ap.add_argument('--mfma', action='store_true', help="exact_mode('auto') after one calibrating wide forward: padded, narrow=True, narrow='mfma'")
    ap.add_argument('--narrow32', action='store_true', help='9 .. 32 images: no keyword against narrow32=True, both contracts (profiles/r10_narrow32.txt)')
    ap.add_argument('--narrow64', action='store_true', help='33 .. 64 images: no keyword against narrow=True, narrow64=True under the default contract (profiles/r11_narrow64.txt)')
    ap.add_argument('--mfma64', action='store_true', help="33 .. 64 images under exact_mode('auto'): padded forward, narrow='mfma' narrow64='mfma', two narrow32 forwards (profiles/r12_narrow64_mfma.txt)")
    ap.add_argument('--images', type=lambda v: tuple(int(k) for k in v.split(',')), default=N32_IMAGES, help='image counts of --narrow32')
    ap.add_argument('--blocks', action='store_true', help='with --narrow32: one conv5_x-shaped operator per column-block width (diagnostic build)')
    ap.add_argument('--split', action='store_true', help="filled-in synthetic operators of the VGG-16 conv shapes: narrow='mfma' without and with narrow_split=True at 1, 8, 32 images (profiles/r14_narrow_split.txt)")
    ap.add_argument('--fill', action='store_true', help='filled-in synthetic operators of the VGG-16 conv shapes under exact=True: narrow=True without and with narrow_fill=True, and the padded 128-column call, at 1, 8, 16, 32 images (profiles/r16_narrow_fill.txt)')
    ap.add_argument('--taps', action='store_true', help='whole forwards with and without narrow_taps=True at 1, 2, 4, 8 images (profiles/r15_narrow_taps.txt)')
    ap.add_argument('--taps32', action='store_true', help="whole forwards narrow32=True without and with narrow_taps='packed' at 9, 12, 16, 24, 32 images, and the 8-image narrow_taps=True forward (profiles/r17_narrow_taps32.txt)")
    ap.add_argument('--pairs', action='store_true', help="whole forwards with narrow_taps=True against narrow_taps='pairs' at 1, 2, 4, 8 images (profiles/r18_narrow_taps_pairs.txt)")
    ap.add_argument('--layers', type=lambda v: tuple(v.split(',')), default=(), help='with --split: only these layer shapes (conv1_1, conv1_2, conv2_1, ..., conv5_x)')
    ap.add_argument('--fused-calls', type=int, default=3, help='with --split: timed calls of the fused channel-lane launch (hundreds of ms each on the larger layers)')
    args = ap.parse_args()
    if args.split:
        return split_trace_table(args) if args.from_trace else split_table(args)
    if args.fill:
        return fill_trace_table(args) if args.from_trace else fill_table(args)
    if args.from_trace and args.taps:
        return taps_trace_table(args)
    if args.from_trace and args.pairs:
        return pairs_trace_table(args)
    if args.from_trace and args.taps32:
        return taps32_trace_table(args)
    if args.from_trace:
        return narrow64_trace_table(args) if (args.narrow64 or args.mfma64) else narrow32_trace_table(args) if args.narrow32 else rows_trace_table(args) if args.rows else linear_trace_table(args) if args.linear else trace_table(args)
    if args.narrow32 and args.blocks:
        return narrow32_blocks(args)
    assert args.forwards >= 20 or args.one_forward, 'the median of at least 20 forwards'
    t0 = time.time()
    (sensor, knet, inshape, _, desc, _) = workloads.build_workload(args.workload, 0, fanout=True)
    dev = torch.device('cuda:0')
    torch.manual_seed(1)
    imgs = torch.randn((64 if (args.narrow64 or args.mfma64 or args.linear) else max(args.images) if args.narrow32 else 32 if args.taps32 else 8,) + tuple(inshape))
    xc = sensor.fromtensor(imgs.to(dev)).encrypt().astensor()
    xc = xc.t().contiguous().t()                  # feature-major, as the layers hand blocks on
    print('keyed %s in %.0f s' % (desc, time.time() - t0), flush=True)
    if args.taps:
        return taps_table(args, knet, xc, desc)
    if args.pairs:
        return pairs_table(args, knet, xc, desc)
    if args.taps32:
        return taps32_table(args, knet, xc, desc)
    if args.mfma64:
        return mfma64_table(args, knet, xc, desc)
    if args.narrow64:
        return narrow64_table(args, knet, xc, desc)
    if args.narrow32:
        return narrow32_table(args, knet, xc, desc)
    if args.mfma:
        return mfma_table(args, knet, xc, desc)
    if args.rows:
        return rows_table(args, knet, xc, desc)
    if args.linear:
        return linear_table(args, knet, xc, desc)
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
    with open(args.out or os.path.join(ROOT, 'profiles', 'r07_narrow_forward.txt'), 'a') as f:
        f.write(text)


if __name__ == '__main__':
    main()
