#!/usr/bin/env python
"""Every kn_spmm the Python host issues for the wide and the narrow forwards of the small golden key-nets, as text: what a host-side refactor must not move.

    python tools/narrow_launches.py [--dump DIR] > launches.txt

Wraps _capi.Operator.spmm and prints one line per call: the layer's index in the key-net (-1: not a layer's own handle, e.g. the whole-net kernel), the text of
kn_spmm_plan for that very call, the flags in hex, n_vecs, ldx, ldy and whether an absmax slot was given.  Covered: the key-nets NETS of tests/golden, each
under the contract it loads with and after exact_mode(True), exact_mode(False) and exact_mode('auto') with one calibrating wide forward; for 1, 3 and 8 images
forward_linear wide, narrow=True and narrow='mfma', each with and without narrow_rows=True; for 4 images one capture() and two replays of each form; then
contract_report() (floats rounded), the counters and the keys of the cached launch lists.  --dump DIR writes the logits of every forward as .npy files.
Two trees issue the same launches when the outputs are byte-identical (cmp) and the dumped logits equal (np.array_equal)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                # noqa: E402
import torch                                      # noqa: E402
from keynet_amd import _capi, io as kio           # noqa: E402

NETS = ('mini_tiled_permutation.npz', 'mini_tiled_permutation8.npz', 'mini_tiled_stochastic.npz', 'lenet_perm.npz', 'allconv_tiny_perm.npz')
FORMS = [(False, False)] + [(narrow, rows) for narrow in (True, 'mfma') for rows in (False, True)]


def rounded(v):
    if isinstance(v, float):
        return float('%.6g' % v)
    if isinstance(v, dict):
        return {k: rounded(x) for (k, x) in sorted(v.items())}
    return [rounded(x) for x in v] if isinstance(v, (list, tuple)) else v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dump', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    state = dict(handles={}, tag='')
    spmm = _capi.Operator.spmm

    def recording(self, x_ptr, ldx, n_vecs, y_ptr, ldy, flags, stream, absmax_ptr=None):
        print('%s layer=%d flags=0x%02x n=%d ldx=%d ldy=%d absmax=%s: %s' % (state['tag'], state['handles'].get(id(self), -1),
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
            np.save(os.path.join(args.dump, tag.replace(' ', '_').replace('/', '_') + '.npy'), y.detach().cpu().numpy())

    for fname in NETS:
        z = np.load(os.path.join(ROOT, 'tests', 'golden', fname), allow_pickle=False)
        x = torch.as_tensor(z['x_cipher']).to(dev)
        x = x.repeat(-(-8 // x.shape[0]), 1)[:8].contiguous() * torch.linspace(0.5, 1.0, 8, device=dev)[:, None] if x.shape[0] < 8 else x
        for contract in ('loaded', True, False, 'auto'):
            knet = kio.keynet_from_arrays(z)
            name = '%s[%s]' % (fname[:-4], contract)
            if contract != 'loaded':
                knet.exact_mode(contract)
            run('%s calibrate' % name, lambda: knet.forward_linear(x))
            with torch.cuda.device(dev):                       # the handles now resident, by layer: what a recorded call is attributed to
                for (k, c) in enumerate(knet._keyed()):
                    for cache in (getattr(c.W, a, None) for a in ('_op', '_op_dense', '_op_split')):
                        for op in (cache.values() if isinstance(cache, dict) else ()):
                            for o in (op if isinstance(op, (list, tuple)) else (op,)):
                                if isinstance(o, _capi.Operator):
                                    state['handles'][id(o)] = k
            for n in (1, 3, 8):
                for (narrow, rows) in FORMS:
                    run('%s n=%d narrow=%s rows=%s' % (name, n, narrow, rows), lambda: knet.forward_linear(x[:n], narrow=narrow, narrow_rows=rows))
            for (narrow, rows) in FORMS:
                tag = '%s capture n=4 narrow=%s rows=%s' % (name, narrow, rows)
                state['tag'] = tag
                replay = knet.capture(x[:4], narrow=narrow, narrow_rows=rows)
                for r in (0, 1):
                    run('%s replay %d' % (tag, r), lambda: replay(x[4 * r:4 * r + 4]).clone())
            print('%s report %s' % (name, json.dumps(rounded(knet.contract_report()), sort_keys=True, default=str)))
            print('%s padded=%s recalibrations=%s narrow_remeasurements=%s overlap_plans=%s chain_ops=%s' % (
                name, getattr(knet, '_padded_forwards', 0), knet.__dict__.get('_recalibrations', 0), knet.__dict__.get('_narrow_remeasurements', 0),
                sorted(knet.__dict__.get('_overlap_plans', {}).keys()), sorted(knet.__dict__.get('_chain_ops', {}).keys())))
            state['handles'].clear()


if __name__ == '__main__':
    main()
