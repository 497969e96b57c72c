#!/usr/bin/env python
"""Every kn_spmm the Python host issues for the wide and the narrow forwards of small key-nets, as text: what a host-side refactor must not move.

    python tools/narrow_launches.py [--dump DIR] > launches.txt

Wraps _capi.Operator.spmm and prints one line per call: the layer's index in the key-net (-1: not a layer's own handle, e.g. the whole-net kernel), the text of
kn_spmm_plan for that very call, the flags in hex, n_vecs, ldx, ldy and whether an absmax slot was given.  Covered: the key-nets NETS of tests/golden, each
under the contract it loads with and after exact_mode(True), exact_mode(False) and exact_mode('auto') with one calibrating wide forward, and one untiled key-net
with a keyed Linear that holds a big pattern group (keyed here, one launch per layer).  On each, every keyword set of CASES -- the wide forward and narrow=True |
'mfma' with and without narrow_rows at 1, 3 and 8 images; narrow32=True at 16 and 32; narrow=True, narrow64=True at 33 and 48; narrow='mfma', narrow64='mfma' at
20, 40 and 64; narrow_linear=True at 1, 8 and 32, with narrow_rows where the width allows -- as one eager forward_linear, then one capture() and two replays on
other images.  Then the trip paths: a batch scaled far beyond every record, eager and through a replay, under narrow='mfma' (the narrow record is dropped and
measured again) and under narrow='mfma', narrow64='mfma' at 40 images (the layer goes back to 'auto').  Last contract_report() (floats rounded), the counters and
the keys of the cached launch lists.  --dump DIR writes the logits of every forward as .npy files.
Two trees issue the same launches when the outputs are byte-identical (cmp) and the dumped logits equal (np.array_equal).  The file uses the public keyword
surfaces only, so one copy of it runs from inside either tree."""
import argparse
import gc
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                # noqa: E402
import torch                                      # noqa: E402
from torch import nn                              # noqa: E402
from keynet_amd import _capi, io as kio, system as ksys           # noqa: E402

NETS = ('mini_tiled_permutation.npz', 'mini_tiled_permutation8.npz', 'mini_tiled_stochastic.npz', 'lenet_perm.npz', 'allconv_tiny_perm.npz')
MODES = (True, 'mfma')
CASES = ([(n, kw) for n in (1, 3, 8) for kw in [{}] + [dict(narrow=m, narrow_rows=r) for m in MODES for r in (False, True)]] +
         [(n, dict(narrow=m, narrow32=True)) for n in (16, 32) for m in MODES] +
         [(n, dict(narrow=True, narrow64=True)) for n in (33, 48)] +
         [(n, dict(narrow='mfma', narrow64='mfma')) for n in (20, 40, 64)] +
         [(n, dict(narrow=m, narrow_rows=r, narrow32=n > 8, narrow_linear=True)) for n in (1, 8, 32) for m in MODES for r in ((False, True) if n <= 8 else (False,))])
TRIP = 64.0       # the factor of the batches that must trip a screen (KeyedLayer.RESCREEN_FACTOR is 2)


class LinearNet(nn.Module):
    """conv -> relu -> fc (256 rows over 2 049 shared columns: one big pattern group) -> relu -> fc."""

    def __init__(self):
        super(LinearNet, self).__init__()
        self.conv1 = nn.Conv2d(1, 8, 3, stride=1, padding=1)
        self.relu1 = nn.ReLU()
        self.fc1 = nn.Linear(8 * 16 * 16, 256)
        self.relu2 = nn.ReLU()
        self.fc2 = nn.Linear(256, 10)

    def forward(self, x):
        x = self.relu1(self.conv1(x))
        return self.fc2(self.relu2(self.fc1(x.reshape(x.shape[0], -1))))


def rounded(v):
    if isinstance(v, float):
        return float('%.6g' % v)
    if isinstance(v, dict):
        return {k: rounded(x) for (k, x) in sorted(v.items())}
    return [rounded(x) for x in v] if isinstance(v, (list, tuple)) else v


def words(kw):
    return ' '.join('%s=%s' % (k, kw[k]) for k in sorted(kw)) or 'wide'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dump', default=None)
    args = ap.parse_args()
    gc.disable()                                          # collected between captures only: see capture() below
    dev = torch.device('cuda:0')
    state = dict(handles={}, tag='')
    spmm = _capi.Operator.spmm

    def recording(self, x_ptr, ldx, n_vecs, y_ptr, ldy, flags, stream, absmax_ptr=None):
        print('%s layer=%d flags=0x%03x n=%d ldx=%d ldy=%d absmax=%s: %s' % (state['tag'], state['handles'].get(id(self), -1),
                                                                            flags, n_vecs, ldx, ldy, 'yes' if absmax_ptr else 'no', self.plan(n_vecs, flags, ldx=ldx, ldy=ldy)))
        return spmm(self, x_ptr, ldx, n_vecs, y_ptr, ldy, flags, stream, absmax_ptr)
    _capi.Operator.spmm = recording

    def run(tag, fn):
        state['tag'] = tag
        y = fn()
        torch.cuda.synchronize()
        print('%s -> shape %s' % (tag, tuple(y.shape)))
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            np.save(os.path.join(args.dump, tag.replace(' ', '_').replace('/', '_').replace("'", '') + '.npy'), y.detach().cpu().numpy())

    def counters(name, knet):
        print('%s padded=%s recalibrations=%s narrow_remeasurements=%s overlap_plans=%s chain_ops=%s' % (
            name, getattr(knet, '_padded_forwards', 0), knet.__dict__.get('_recalibrations', 0), knet.__dict__.get('_narrow_remeasurements', 0),
            sorted(knet.__dict__.get('_overlap_plans', {}).keys()), sorted(knet.__dict__.get('_chain_ops', {}).keys())))

    def capture(knet, x, **kw):
        """knet.capture(x, **kw) with the garbage of earlier captures collected first, the collector being off otherwise (main): a replay closure refers to
        itself, so only the cycle collector frees its HIP graph, and a graph destroyed while a later capture is recording ends the process."""
        gc.collect()
        return knet.capture(x, **kw)

    def cover(name, knet, x, contract=None):
        """Everything the docstring lists, on one key-net under `contract` (an argument of exact_mode; None: as built); x: 64 images on the device."""
        run('%s calibrate' % name, lambda: knet.forward_linear(x[:8]))
        with torch.cuda.device(dev):                       # the handles now resident, by layer: what a recorded call is attributed to
            for (k, c) in enumerate(knet._keyed()):
                for cache in (getattr(c.W, a, None) for a in ('_op', '_op_dense', '_op_split')):
                    for op in (cache.values() if isinstance(cache, dict) else ()):
                        for o in (op if isinstance(op, (list, tuple)) else (op,)):
                            if isinstance(o, _capi.Operator):
                                state['handles'][id(o)] = k
        for (n, kw) in CASES:
            tag = '%s n=%d %s' % (name, n, words(kw))
            run(tag, lambda: knet.forward_linear(x[:n], **kw))
            state['tag'] = tag + ' capture'
            replay = capture(knet, x[:n], **kw)
            for r in (1, 2):
                run('%s replay %d' % (tag, r), lambda: replay(torch.roll(x, 5 * r, 0)[:n]).clone())
        counters(name + ' before the trips', knet)
        for (n, kw) in ((8, dict(narrow='mfma')), (40, dict(narrow='mfma', narrow64='mfma'))):
            tag = '%s trip n=%d %s' % (name, n, words(kw))
            for how in ('eager', 'replay'):                # each from fresh records: decided and measured on x, then a batch TRIP times as large
                knet.exact_mode(contract)
                run('%s %s: calibrate' % (tag, how), lambda: knet.forward_linear(x[:n]))
                if how == 'eager':
                    run('%s eager: records' % tag, lambda: knet.forward_linear(x[:n], **kw))
                    run('%s eager: trip' % tag, lambda: knet.forward_linear(TRIP * x[:n], **kw))
                else:
                    state['tag'] = tag + ' capture'
                    replay = capture(knet, x[:n], **kw)
                    run('%s replay: trip' % tag, lambda: replay(TRIP * x[:n]).clone())
                counters('%s %s' % (tag, how), knet)
        print('%s report %s' % (name, json.dumps(rounded(knet.contract_report()), sort_keys=True, default=str)))
        state['handles'].clear()

    for fname in NETS:
        z = np.load(os.path.join(ROOT, 'tests', 'golden', fname), allow_pickle=False)
        x = torch.as_tensor(z['x_cipher']).to(dev)
        x = (x.repeat(-(-64 // x.shape[0]), 1)[:64] * torch.linspace(0.5, 1.0, 64, device=dev)[:, None]).contiguous()
        for contract in ('loaded', True, False, 'auto'):
            knet = kio.keynet_from_arrays(z)
            if contract != 'loaded':
                knet.exact_mode(contract)
            cover('%s[%s]' % (fname[:-4], contract), knet, x, None if contract == 'loaded' else contract)
    torch.manual_seed(3)
    np.random.seed(3)
    (sensor, knet) = ksys.PermutationKeynet((1, 16, 16), LinearNet())
    knet.CHAIN = False                                     # one launch per layer: the whole-net kernel would take a key-net this small in one
    cover('linear_net', knet, sensor.fromtensor(torch.rand(64, 1, 16, 16).to(dev)).encrypt().astensor())


if __name__ == '__main__':
    main()
