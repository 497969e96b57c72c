"""A plain `bench.py` run does what its headline needs and nothing else; `--full` adds every other leg.  On CPU: the pooling layers keyed in forked
processes (what a single-rank run does) give the same key-net as keying in one process, a failing forked layer fails the construction and leaves
no process behind, the plain line, and the opt-in legs refused without --full.  On the GPU: a plain run and a --full run of the same arguments time the
same steps on the same inputs and dump the same logits."""
import json
import multiprocessing
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench   # noqa: E402
from benchlegs import workloads   # noqa: E402
from keynet_amd import system as ksys   # noqa: E402
from keynet_amd.layer import KeyedLayer   # noqa: E402
from keynet_amd.models import VGG16   # noqa: E402

HEADLINE = ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data', 'config')
FULL_ONLY = ('roofline', 'cpu_baseline', 'parity', 'exact', 'secondary', 'contract', 'end_to_end', 'collective')


def _differences(a, b, path):
    """Where two keyed layers differ: types, dict keys, arrays bit for bit.  (An operator that went through pickle carries `_op_dense = None`, the
    empty device-cache slot SparseMatrix.__getstate__ writes: not a difference.)"""
    if type(a) is not type(b):
        return ['%s: %s vs %s' % (path, type(a).__name__, type(b).__name__)]
    if isinstance(a, np.ndarray):
        return [] if (a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()) else ['%s: arrays differ' % path]
    if scipy.sparse.issparse(a):
        if (a.format, a.shape, a.dtype) != (b.format, b.shape, b.dtype):
            return ['%s: %s vs %s' % (path, (a.format, a.shape, a.dtype), (b.format, b.shape, b.dtype))]
        return sum((_differences(getattr(a, k), getattr(b, k), path + '.' + k) for k in ('row', 'col', 'data', 'indices', 'indptr', 'offsets') if hasattr(a, k)), [])
    if isinstance(a, torch.Tensor):
        return [] if (a.dtype == b.dtype and torch.equal(a, b)) else ['%s: tensors differ' % path]
    if isinstance(a, dict):
        (a, b) = ({k: v for (k, v) in d.items() if not (k == '_op_dense' and v is None)} for d in (a, b))
        if list(a) != list(b):
            return ['%s: keys %s vs %s' % (path, list(a), list(b))]
        return sum((_differences(a[k], b[k], '%s[%r]' % (path, k)) for k in a), [])
    if isinstance(a, (list, tuple)):
        if len(a) != len(b):
            return ['%s: %d vs %d items' % (path, len(a), len(b))]
        return sum((_differences(x, y, '%s[%d]' % (path, i)) for (i, (x, y)) in enumerate(zip(a, b))), [])
    if hasattr(a, '__dict__') and not isinstance(a, type):
        return _differences(a.__dict__, b.__dict__, path)
    return [] if a == b else ['%s: %r vs %r' % (path, a, b)]


def _vgg_slice():
    torch.manual_seed(0)
    net = VGG16(num_classes=10, width=8, fc_width=64, insize=32).eval()
    np.random.seed(0)
    return net


def test_pooling_layers_keyed_in_forked_processes_give_the_same_key_net():
    make = ksys.layergen
    (s1, k1) = ksys.TiledPermutationKeynet((3, 32, 32), _vgg_slice(), 8, exact='auto')
    prepared = []
    with workloads._keying(workloads.FANOUT_TYPES) as finish:
        (s2, k2) = ksys.TiledPermutationKeynet((3, 32, 32), _vgg_slice(), 8, exact='auto')
        assert sum(isinstance(m, workloads._Pending) for m in k2._keynet.children()) == 5
        finish(k2, prepared.append)
    assert ksys.layergen is make
    assert not multiprocessing.active_children()
    assert [n for (n, _) in k1._keynet.named_children()] == [n for (n, _) in k2._keynet.named_children()]
    for ((name, a), b) in zip(k1._keynet.named_children(), k2._keynet.children()):
        assert not _differences(a.__dict__, b.__dict__, name), _differences(a.__dict__, b.__dict__, name)[:5]
    assert sorted(id(m) for m in prepared) == sorted(id(m) for m in k2._keynet.children() if isinstance(m, KeyedLayer))
    assert _differences(s1.__dict__, s2.__dict__, 'sensor') == []


def test_build_workload_with_fanout_equals_without():
    (_, k1, *_) = workloads.build_workload('vgg16-slice', 0, exact='auto')
    (_, k2, *_) = workloads.build_workload('vgg16-slice', 0, exact='auto', fanout=True)
    for ((name, a), b) in zip(k1._keynet.named_children(), k2._keynet.children()):
        assert not _differences(a.__dict__, b.__dict__, name), name


def test_a_failing_forked_layer_fails_the_construction_and_leaves_nothing_running(monkeypatch):
    make = ksys.layergen

    def broken(module, *a, **kw):
        if isinstance(module, torch.nn.AvgPool2d):
            raise ValueError('no pool today')
        return make(module, *a, **kw)
    monkeypatch.setattr(ksys, 'layergen', broken)
    with pytest.raises(RuntimeError, match='pool1_2.*ValueError: no pool today'):
        with workloads._keying(workloads.FANOUT_TYPES) as finish:
            (_, knet) = ksys.TiledPermutationKeynet((3, 32, 32), _vgg_slice(), 8, exact='auto')
            finish(knet)
    assert ksys.layergen is broken
    assert not multiprocessing.active_children()


def test_plain_record_gives_a_line_with_the_headline_alone():
    res = {'metric': 'encrypted images/sec (whole node), keyed VGG-16 224x224', 'value': 4538.391234, 'unit': 'images/s', 'n_gpus': 1, 'steps': 20, 'warmup': 5,
           'ms_per_step': 56.40771234, 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
           'config': {'workload': 'TiledPermutationKeynet VGG16(2622)', 'mode': 'tolerance', 'headline_contract': "opt-in exact='auto'", 'default_contract_value': 'the `exact` leg of --full',
                      'images_per_gpu': 256, 'global_batch': 256, 'parallelism': 'single GPU'}, 'full': False}
    line = bench.compact_record(res)
    assert '\n' not in line and len(line) < bench.LINE_LIMIT
    r = json.loads(line)
    assert all(k in r for k in HEADLINE) and r['full'] is False and r['detail'] == bench.DETAIL_FILE
    assert not [k for k in FULL_ONLY if k in r]
    assert r['value'] == 4538.39 and r['ms_per_step'] == 56.4077 and r['dtype'] == 'f32' and r['higher_is_better'] is True


@pytest.mark.parametrize('flag', ['--experimental', '--graph-leg', '--exact-layers-parity'])
def test_opt_in_legs_need_full(flag):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), flag], capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and 'add --full' in p.stderr, p.stderr[-2000:]
    assert not p.stdout.strip()


@pytest.mark.gpu
def test_plain_and_full_runs_time_the_same_steps_and_dump_the_same_logits(tmp_path):
    """vgg16-slice (the 21 keyed layers of VGG-16 at width 8), keyed with its pools in forked processes and its operators uploaded as the layers come: the
    --full run adds the parity gate, the per-layer table and the side legs to the same timed steps.  Same logits, bit for bit."""
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'KN_BENCH_SHARE_GPU'):
        env.pop(k, None)
    lines = {}
    for (tag, extra) in (('plain', []), ('full', ['--full', '--no-cpu-baseline', '--layer-iters', '1'])):
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--workload', 'vgg16-slice', '--steps', '3', '--warmup', '1',
                            '--dump-outputs', str(tmp_path / tag), '--detail', str(tmp_path / (tag + '.json'))] + extra, env=env, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-3000:]
        out = [l for l in p.stdout.splitlines() if l.startswith('{')]
        assert len(out) == 1 and len(out[0]) < bench.LINE_LIMIT
        lines[tag] = json.loads(out[0])
    (plain, full) = (lines['plain'], lines['full'])
    assert np.array_equal(np.load(str(tmp_path / 'plain' / 'logits.npy')), np.load(str(tmp_path / 'full' / 'logits.npy')))
    assert plain['full'] is False and full['full'] is True
    for r in (plain, full):
        assert all(k in r for k in HEADLINE) and r['value'] > 0 and r['unit'] == 'images/s' and r['dtype'] == 'f32' and r['steps'] == 3 and r['warmup'] == 1
    assert not [k for k in FULL_ONLY if k in plain]
    assert full['parity']['ok'] is True and full['roofline']['peak'] > 0 and 'contract' in full
    assert {k: v for (k, v) in plain['config'].items() if k != 'default_contract_value'} == \
        {k: v for (k, v) in full['config'].items() if k not in ('default_contract_value', 'nnz_per_image')}
