"""Host-side checks of the narrow split route (narrow='mfma', narrow_split=True): the two permute entry points in the C ABI and its binding, the gfx950 ISA of the
permute kernel (no scratch, its LDS tile), the keyword through ksp.NarrowForm, ksp._narrow_args and every surface that takes it, KeyedLayer.kernel's answer, and
the cost rule.  No GPU."""
import ctypes
import inspect
import os
import re
import shutil

import numpy as np
import pytest
import torch

from keynet_amd import _capi
from keynet_amd import sparse as ksp
from keynet_amd import system as ksys
from keynet_amd.layer import KeyedLayer
from test_isa_lint import _isa, _kernel_bodies
from test_narrow_host import _tiny_conv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ('kn_planes_to_columns', 'kn_columns_to_planes')
KERNEL = r'_ZN2kn21planes_columns_kernel'
MFMA = _capi.KN_FLAG_NARROW_MFMA


def test_header_declares_the_entry_points_and_the_library_exports_them():
    h = open(os.path.join(ROOT, 'include', 'keynet_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', h, flags=re.S)
    for name in ENTRY:
        assert re.search(r'\bint\s+%s\s*\(' % name, code), name
        assert name in _capi.SYMBOLS
    doc = h[h.index('Planes <-> columns of a narrow batch'):h.index('int kn_planes_to_columns(')]
    for word in ('No reference counterpart', 'narrow split route', 'narrow_split=True', '64 bits', 'NaN payloads', 'untouched', 'KN_ABI_VERSION', 'in_dev + p * plane_stride + r * ld + b',
                 'out_dev + r * ld_out + p * n_vecs + b'):
        assert word in doc, word
    v = re.search(r'#define\s+KN_ABI_VERSION\s+(\d+)', h)
    assert v and int(v.group(1)) == 5 and _capi.KN_ABI_VERSION == 5           # entry points added: the header's rule leaves the number where it is
    L = ctypes.CDLL(_capi.LIBPATH)
    for name in ENTRY:
        assert hasattr(L, name), 'libkeynet_hip.so does not export %s' % name
    assert callable(_capi.planes_to_columns) and callable(_capi.columns_to_planes)


def test_the_entry_points_refuse_bad_arguments_without_a_device():
    """Argument checks come before anything touches a device: a wider batch than 32 columns, a leading dimension below the width, overlapping planes."""
    L = _capi.lib()
    one = ctypes.c_void_p(16)
    assert L.kn_planes_to_columns(one, 100, 33, 2, 3, 33, one, 66, None) == 6       # KN_ERR_UNSUPPORTED: not a narrow batch
    assert L.kn_planes_to_columns(one, 100, 3, 2, 3, 4, one, 8, None) == 2          # KN_ERR_SHAPE: ld < n_vecs
    assert L.kn_planes_to_columns(one, 100, 4, 2, 3, 4, one, 7, None) == 2          # ... ld_out < n_planes * n_vecs
    assert L.kn_columns_to_planes(one, 8, 2, 3, 4, one, 11, 4, None) == 2           # ... planes overlap
    assert L.kn_columns_to_planes(one, 8, 2, -1, 4, one, 12, 4, None) == 1          # KN_ERR_INVALID
    assert L.kn_planes_to_columns(None, 0, 1, 0, 0, 1, None, 1, None) in (0, 5)     # nothing to move (KN_OK; without a device the first HIP call may say so)


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='needs hipcc')
def test_permute_kernel_isa(tmp_path):
    """Both directions x (16 bytes | one float per lane) on either side: no scratch, one 40 KB LDS tile (within 64 KB: four workgroups per CU), a barrier between
    the two sides, 16-byte global loads and stores in the aligned forms and none in the float-by-float ones."""
    s = _isa('kn_elementwise.hip', tmp_path)
    kernels = _kernel_bodies(s, [KERNEL])
    forms = sorted(re.match(KERNEL + r'ILb([01])ELi(\d)ELi(\d)EE', name).groups() for (name, _) in kernels)
    assert forms == sorted((d, p, c) for d in '01' for p in '14' for c in '14'), forms
    for (name, lines) in kernels:
        (to_columns, gp, gc) = re.match(KERNEL + r'ILb([01])ELi(\d)ELi(\d)EE', name).groups()
        assert not any(l.startswith('scratch_') or (l.startswith('buffer_store') and 'offen' in l) for l in lines), 'spill in %s' % name
        meta = s[s.index('.amdhsa_kernel ' + name):]
        meta = meta[:meta.index('.end_amdhsa_kernel')]
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', meta).group(1)) == 0, name
        lds = int(re.search(r'\.amdhsa_group_segment_fixed_size\s+(\d+)', meta).group(1))
        assert lds == 4 * 10240 <= 64 * 1024, (name, lds)
        assert any(l.startswith('s_barrier') for l in lines), name
        assert not any('atomic' in l for l in lines), name
        (load_g, store_g) = ((gp, gc) if to_columns == '1' else (gc, gp))
        assert any(l.startswith('global_load_dwordx4') for l in lines) == (load_g == '4'), name
        assert any(l.startswith('global_store_dwordx4') for l in lines) == (store_g == '4'), name
        assert any(re.match(r'global_load_dword ', l) for l in lines) and any(re.match(r'global_store_dword ', l) for l in lines), name      # the ragged ends
        assert any(l.startswith('ds_write') or l.startswith('ds_store') for l in lines) and any(l.startswith('ds_read') or l.startswith('ds_load') for l in lines), name


def test_the_keyword_reaches_every_layer_of_the_python_host():
    for f in (ksys.KeyedModel.forward_linear, ksys.KeyedModel.forward, ksys.KeyedModel.capture, KeyedLayer.forward, KeyedLayer.kernel, KeyedLayer.launch,
              ksp._run_torchdot, ksp._narrow_args, ksp.Conv2dTiledMatrix.torchdot, ksp.NarrowForm.of.__wrapped__):
        p = inspect.signature(f).parameters
        assert 'narrow_split' in p and p['narrow_split'].default is False, f
        assert 'narrow_split' in (f.__doc__ or '') or f is ksp.NarrowForm.of.__wrapped__, f


def test_argument_rule_and_the_form():
    A = ksp._narrow_args
    assert A(8, 'mfma', False, narrow_split=True) == ('mfma', False)
    assert A(32, 'mfma', False, narrow32=True, narrow_split=True) == ('mfma', False)
    assert A(40, 'mfma', False, narrow64='mfma', narrow_split=True) == ('mfma', False)       # accepted, and inert there
    for (n, kw) in ((9, {}), (33, dict(narrow32=True))):
        with pytest.raises(ValueError):
            A(n, 'mfma', False, narrow_split=True, **kw)                                    # the width limit is that of the other keywords
    for alone in (False, True):
        for narrow in (False, True):
            with pytest.raises(ValueError, match="narrow_split=True is the split application.*pass narrow='mfma'"):
                A(2, narrow, False, alone=alone, narrow_split=True)
    # the form carries it and hands it back; without it a form is the six-field value it was
    plain = ksp.NarrowForm.of(8, 'mfma')
    form = ksp.NarrowForm.of(8, 'mfma', narrow_split=True)
    assert form.split is True and plain.split is False and tuple(form) == tuple(plain) and form != plain and plain != form and hash(form) != hash(plain)
    assert form.keywords() == dict(plain.keywords(), narrow_split=True) and 'narrow_split' not in plain.keywords()
    assert ksp.NarrowForm.of(8, **form.keywords()) == form and ksp.NarrowForm.of(None, **form.keywords()).split
    assert type(ksp.NarrowForm.of(8, 'mfma', narrow_split=False)) is ksp.NarrowForm and 'NarrowSplitForm' in repr(form)
    with pytest.raises(ValueError):
        ksp.NarrowForm.of(8, True, narrow_split=True)
    assert ksp.NarrowForm.of(None, True, narrow_split=True).split is False                  # (no batch: nothing refused, and without 'mfma' the keyword adds nothing)


def _filled_in(Cin=4, Cout=8, H=3, fill=3):
    rng = np.random.RandomState(1)
    HW = H * H
    (eo, ei, et) = ([], [], [])
    for t in range(9):
        for o in range(HW):
            eo += [o] * fill
            ei += list(rng.choice(HW, size=fill, replace=False))
            et += [t] * fill
    W = ksp.Conv2dTiledMatrix.fromtaps((Cin, H, H), (Cout, H, H), rng.randn(9, Cout, Cin), eo, ei, et, rng.randn(len(eo)), np.ones(Cout * HW + 1))
    W._device_op = lambda device=None: 'handle'
    return W


def test_kernel_answers_not_one_launch_only_for_a_filled_in_operator_under_split():
    filled = _filled_in()
    nine = _tiny_conv()
    assert filled.split_capable() and not nine.split_capable()
    for relu in (False, True):
        for kw in (dict(), dict(narrow32=True), dict(narrow32=True, narrow64='mfma')):
            assert KeyedLayer.kernel(filled, 'split', relu, None, narrow='mfma', narrow_split=True, **kw) is None
            for contract in (True, False, 'bf16x3', 'auto'):
                assert KeyedLayer.kernel(filled, contract, relu, None, narrow='mfma', narrow_split=True, **kw) == KeyedLayer.kernel(filled, contract, relu, None, narrow='mfma', **kw)
            for contract in (True, False, 'bf16x3', 'split', 'auto'):
                assert KeyedLayer.kernel(nine, contract, relu, None, narrow='mfma', narrow_split=True, **kw) == KeyedLayer.kernel(nine, contract, relu, None, narrow='mfma', **kw)
            assert KeyedLayer.kernel(filled, 'split', relu, None, narrow='mfma', **kw)[1] & MFMA       # without the keyword: one narrow launch, as before
            assert KeyedLayer.kernel(filled, 'split', relu, None, narrow=True, narrow_split=True, **kw) == KeyedLayer.kernel(filled, 'split', relu, None, narrow=True, **kw)


def test_layers_decide_the_route_from_their_contract_and_record(monkeypatch):
    W = _filled_in()
    monkeypatch.setattr(W, 'narrow_split_route', lambda n, relu=False, device=None: True)
    x = torch.zeros((W.shape[1], 4))
    declared = KeyedLayer.fromoperator(W, 'Conv2d', exact='split')
    assert declared.narrow_split_mode(x) is True and declared.narrow_split_mode() is True and declared.launch(None, narrow='mfma', narrow_split=True) is None
    assert declared.launch(None, narrow='mfma').flags & MFMA and declared.narrow_split_record() is None
    for contract in (True, False, 'auto'):
        c = KeyedLayer.fromoperator(W, 'Conv2d', exact=contract)
        assert c.narrow_split_mode(x) is False
        if contract != 'auto':
            assert c.launch(None, narrow='mfma', narrow_split=True) == c.launch(None, narrow='mfma')
    # decided by calibration: a planner measures nothing; a forward measures once, into the record's own key; the answer follows the record
    for decided in ('split', 'exact'):
        c = KeyedLayer.fromoperator(W, 'Conv2d', exact='split')
        c._contract_record = dict(decided='split', max_abs_x=1.0, narrow=dict(decided='exact', gate_ratio=None, max_abs_x=None))
        wide = dict(c._contract_record)
        measured = []
        monkeypatch.setattr(c, '_measure_narrow_split', lambda xt, relu, d=decided: measured.append(int(xt.shape[1])) or dict(decided=d, gate_ratio=0.1, max_abs_x=2.0, measured_on_columns=4))
        assert c.screened() and c.narrow_split_mode() is False and not measured
        assert c.narrow_split_mode(x) is (decided == 'split') and c.narrow_split_mode(x) is (decided == 'split') and measured == [4]
        assert {k: v for (k, v) in c._contract_record.items() if k != 'narrow_split'} == wide and c._exact == 'split'
        assert c.narrow_split_screened() is (decided == 'split')
        (exact, kw) = c.narrowed(ksp.NarrowForm.of(4, 'mfma', narrow_split=True), x)
        assert exact == 'split' and kw.get('narrow_split', False) is (decided == 'split') and kw['narrow'] == ('mfma' if decided == 'split' else True)
        # the screen: against the narrow_split record where the layer is on the route, and a trip drops that record alone
        if decided == 'split':
            assert c.screen_record('split') is c._contract_record['narrow_split'] and c.screen_record(True) is c._contract_record['narrow']
            assert not c.rescreen(3.9, narrow='split') and c.rescreen(4.1, narrow='split')
            c.unscreen('split')
            assert c.narrow_split_record() is None and c._contract_record == wide and c._exact == 'split'
    # the screened set of a narrow_split forward
    c = KeyedLayer.fromoperator(W, 'Conv2d', exact='split')
    c._contract_record = dict(decided='split', max_abs_x=1.0, narrow_split=dict(decided='split', gate_ratio=0.1, max_abs_x=2.0))
    assert ksys.KeyedModel._screen(ksp.NarrowForm.of(4, 'mfma', narrow_split=True), [c]) == ({0}, 'split')
    assert ksys.KeyedModel._screen(ksp.NarrowForm.of(4, 'mfma'), [c]) == (set(), True)


def test_cost_rule():
    """narrow_split_capable: never without a split form or beyond 32 columns; a layer of VGG-16 size under doubly-stochastic keys is offered the route, a toy one is not."""
    assert not _tiny_conv().narrow_split_capable(1) and not _filled_in().narrow_split_capable(1) and _filled_in().narrow_split_capable()

    def layer(Cin, Cout, H, fill):
        ent = 9 * H * H * fill
        z = np.zeros(ent, np.int32)
        return ksp.Conv2dTiledMatrix.fromtaps((Cin, H, H), (Cout, H, H), np.zeros((9, Cout, Cin), np.float32), z, z, z, np.zeros(ent, np.float32), None)
    big = layer(64, 64, 56, 100)
    for n in (1, 8, 32):
        assert big.narrow_split_capable(n), n
    assert not big.narrow_split_capable(33) and not big.narrow_split_capable(0)
    # the margin is a class constant the profile sets: with no margin required every split-capable operator is offered the route
    W = _filled_in()
    W.NARROW_SPLIT_MIN_GAIN = 0.0
    assert W.narrow_split_capable(1) and W.narrow_split_capable(32)
    # windows of whole images
    assert big._narrow_split_window(32) == 32
    big.NARROW_SPLIT_Z_BYTES = 4 * 9 * 56 * 56 * 64 * 5
    assert big._narrow_split_window(32) == 5 and big._narrow_split_window(3) == 3
    # pickling drops the route's device state
    W.__dict__['_narrow_split_ws'] = {'k': 'buffers'}
    W.__dict__['_narrow_split_plans'] = {'k': True}
    del W._device_op
    state = W.__getstate__()
    assert '_narrow_split_ws' not in state and '_narrow_split_plans' not in state and W.__dict__['_narrow_split_ws']
