"""Host-side checks of the tap-resident channel-lane kernel: the KN_FLAG_NARROW_TAPS modifier in the C ABI and its binding, the `narrow_taps` keyword down to
KeyedLayer.kernel and its argument rule, the NarrowForm of calls without the keyword, and the gfx950 ISA of every shipped instantiation of
convtaps_narrow_taps_kernel (separate multiplies and adds, nothing spilled -- neither to scratch nor into vector lanes --, no LDS, no barrier, at most 128 vector
registers, the tap picked by the scalar index mode)."""
import inspect
import os
import re
import shutil

import numpy as np
import pytest
import scipy.sparse

from keynet_amd import _capi
from keynet_amd import sparse as ksp
from keynet_amd import system as ksys
from keynet_amd.layer import KeyedLayer
from test_isa_lint import _isa, _kernel_bodies, FUSED, INT_DIVISION_LITERALS
from test_narrow_host import _tiny_conv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAPS = r'_ZN2kn27convtaps_narrow_taps_kernel'


def test_header_declares_the_modifier_and_the_binding_mirrors_it():
    h = open(os.path.join(ROOT, 'include', 'keynet_hip.h')).read()
    m = re.search(r'#define\s+KN_FLAG_NARROW_TAPS\s+\(0x([0-9a-f]+)u\)', h)
    assert m and int(m.group(1), 16) == 0x400
    assert _capi.KN_FLAG_NARROW_TAPS == 0x400
    flags = [getattr(_capi, n) for n in dir(_capi) if n.startswith('KN_FLAG_')]
    assert len(flags) == 11 and sorted(flags) == [1 << i for i in range(11)]      # one bit each
    v = re.search(r'#define\s+KN_ABI_VERSION\s+(\d+)', h)
    assert v and int(v.group(1)) == 5 and _capi.KN_ABI_VERSION == 5   # a modifier of kn_spmm's flags: no entry point added


def test_the_keyword_reaches_every_layer_of_the_python_host():
    for f in (ksys.KeyedModel.forward_linear, ksys.KeyedModel.forward, ksys.KeyedModel.capture, KeyedLayer.forward, KeyedLayer.kernel, KeyedLayer.launch,
              ksp.Conv2dTiledMatrix.torchdot, ksp.FactoredSparseMatrix.torchdot, ksp._run_torchdot, ksp._narrow_args, ksp.NarrowForm.of.__wrapped__):
        p = inspect.signature(f).parameters
        assert 'narrow_taps' in p and p['narrow_taps'].default is False, f


def test_the_argument_rule():
    for narrow in (True, 'mfma'):
        for n in (1, 8):
            assert ksp._narrow_args(n, narrow, False, narrow_taps=True) == (narrow, False)
            assert ksp._narrow_args(n, narrow, True, narrow_taps=True) == (narrow, True)
        with pytest.raises(ValueError):
            ksp._narrow_args(9, narrow, False, narrow_taps=True)              # the widths are those of the other keywords ...
        assert ksp._narrow_args(9, narrow, False, narrow32=True, narrow_taps=True) == (narrow, False)      # ... every one of them
        assert ksp._narrow_args(32, narrow, False, narrow32=True, narrow_taps=True) == (narrow, False)
    assert ksp._narrow_args(64, True, False, narrow64=True, narrow_taps=True) == (True, False)
    assert ksp._narrow_args(8, 'mfma', False, narrow_split=True, narrow_taps=True) == ('mfma', False)    # combines with narrow_split
    for alone in (False, True):
        for other in ({}, dict(narrow_rows=True), dict(narrow_linear=True)):
            with pytest.raises(ValueError, match='narrow_taps=True'):
                ksp._narrow_args(4, False, other.get('narrow_rows', False), alone=alone, narrow_linear=other.get('narrow_linear', False), narrow_taps=True)


def test_calls_without_the_keyword_have_the_form_they_had():
    keywords = [dict(), dict(narrow=True), dict(narrow='mfma'), dict(narrow=True, narrow_rows=True), dict(narrow=True, narrow32=True), dict(narrow=True, narrow64=True),
                dict(narrow='mfma', narrow64='mfma'), dict(narrow=True, narrow_linear=True), dict(narrow='mfma', narrow_split=True)]
    for kw in keywords:
        for n in (None, 1, 8):
            plain = ksp.NarrowForm.of(n, **kw)
            assert plain == ksp.NarrowForm.of(n, narrow_taps=False, **kw) and plain.taps is False and 'narrow_taps' not in plain.keywords()
            assert type(plain) is (ksp.NarrowSplitForm if kw.get('narrow_split') else ksp.NarrowForm)
            if not kw.get('narrow'):
                continue
            taps = ksp.NarrowForm.of(n, narrow_taps=True, **kw)
            assert tuple(taps) == tuple(plain) and taps.taps is True and taps.split == plain.split      # the same six fields
            assert taps != plain and plain != taps and hash(taps) != hash(plain) and taps == ksp.NarrowForm.of(n, narrow_taps=True, **kw)
            assert taps.keywords() == dict(plain.keywords(), narrow_taps=True)
            assert type(taps) is (ksp.NarrowSplitTapsForm if kw.get('narrow_split') else ksp.NarrowTapsForm)
            assert isinstance(taps, ksp.NarrowSplitForm) == bool(kw.get('narrow_split'))      # a form without narrow_split is no split form
    assert ksp.NarrowForm.of(None, narrow_taps=True).taps is False       # (no batch: nothing is refused, and without `narrow` the keyword says nothing)


@pytest.mark.parametrize('narrow', [True, 'mfma'])
@pytest.mark.parametrize('contract', [True, False, 'auto', 'split', 'bf16x3'])
def test_kernel_adds_the_flag_next_to_kn_flag_narrow_under_every_contract(contract, narrow):
    W = _tiny_conv()
    for relu in (False, True):
        for more in ({}, dict(narrow32=True), dict(narrow64=True)):
            (get_op, flags) = KeyedLayer.kernel(W, contract, relu, narrow=narrow, narrow_taps=True, **more)
            (get_op0, flags0) = KeyedLayer.kernel(W, contract, relu, narrow=narrow, **more)
            assert get_op == get_op0 == W._device_op
            assert not (flags0 & _capi.KN_FLAG_NARROW_TAPS)
            assert flags == flags0 | (_capi.KN_FLAG_NARROW_TAPS if flags0 & _capi.KN_FLAG_NARROW else 0)
            assert bool(flags0 & _capi.KN_FLAG_NARROW) != bool(flags0 & _capi.KN_FLAG_NARROW_MFMA)
            assert bool(flags0 & _capi.KN_FLAG_NARROW) == (narrow is True or contract in (True, 'auto'))
    assert KeyedLayer.kernel(W, contract, False, narrow_taps=True) == KeyedLayer.kernel(W, contract, False)      # without `narrow`: nothing


@pytest.mark.parametrize('narrow', [True, 'mfma'])
def test_operators_without_a_narrow_form_keep_their_flags(narrow):
    M = scipy.sparse.random(12, 9, density=0.4, format='csr', dtype=np.float32, random_state=1)
    W = ksp.SparseMatrix(M)
    assert not W.narrow_capable()
    for relu in (False, True):
        assert KeyedLayer.kernel(W, True, relu, narrow=narrow, narrow_taps=True)[1] == KeyedLayer.kernel(W, True, relu)[1] == _capi.KN_FLAG_EXACT | (_capi.KN_FLAG_RELU if relu else 0)
        assert KeyedLayer.kernel(W, True, relu, narrow=narrow, narrow_rows=True, narrow_taps=True)[1] == KeyedLayer.kernel(W, True, relu, narrow=narrow, narrow_rows=True)[1]
    F = _tiny_conv()
    k = KeyedLayer.kernel(ksp.FactoredSparseMatrix(F.tosparse('csr'), F), True, True, narrow=narrow, narrow_taps=True)
    assert k[1] == _capi.KN_FLAG_EXACT | _capi.KN_FLAG_RELU | _capi.KN_FLAG_NARROW | _capi.KN_FLAG_NARROW_TAPS


def _sgprs(text):
    """The scalar registers an operand text names: s7 -> {7}, s[4:11] -> {4 .. 11}."""
    regs = set()
    for m in re.finditer(r'\bs\[(\d+):(\d+)\]|\bs(\d+)\b', text):
        regs.update(range(int(m.group(1)), int(m.group(2)) + 1) if m.group(3) is None else [int(m.group(3))])
    return regs


def _no_use_of_a_segment_before_it_landed(name, lines):
    """The activation loads are inline assembly the compiler does not count (s_load_dword[xN] sdst, sbase, soffset with the offset in a scalar register): between such a
    load and the next s_waitcnt that waits for lgkmcnt(0), no instruction may name the load's destination registers -- not read them, not copy them, not overwrite
    them.  Scanned in program order over the whole body (labels and branches included: the loads and their wait sit in one block)."""
    pending = set()
    loads = 0
    for l in lines:
        m = re.match(r's_load_dword(x\d+)?\s+(s\d+|s\[\d+:\d+\]),\s*s\[\d+:\d+\],\s*s\d+\s*$', l)
        if m:
            dst = _sgprs(m.group(2))
            assert not (dst & _sgprs(l[l.index(',') + 1:])), 'a segment load overwrites its own address in %s: %s' % (name, l)
            assert not (dst & pending), 'two segment loads in flight into the same registers in %s: %s' % (name, l)
            pending |= dst
            loads += 1
            continue
        if l.startswith('s_waitcnt') and 'lgkmcnt(0)' in l:
            pending = set()
            continue
        if pending and not l.startswith(('.', ';')) and not l.endswith(':'):
            assert not (_sgprs(l) & pending), 'a segment that has not landed is used in %s: %s' % (name, l)
    assert loads >= 9 and not pending, name


def test_the_landing_check_finds_an_early_use():
    ok = ['s_load_dwordx2 s[4:5], s[8:9], s3'] * 1 + ['s_load_dword s%d, s[8:9], s3' % k for k in range(20, 28)] + ['v_mov_b32_e32 v1, s6', 's_waitcnt lgkmcnt(0)', 'v_mul_f32_e32 v0, s4, v1']
    _no_use_of_a_segment_before_it_landed('ok', ok)
    for early in ('v_mul_f32_e32 v0, s5, v1', 's_mov_b32 s30, s4', 's_mov_b64 s[4:5], 0', 's_add_u32 s9, s21, s1'):
        with pytest.raises(AssertionError):
            _no_use_of_a_segment_before_it_landed('bad', ok[:9] + [early] + ok[9:])
    with pytest.raises(AssertionError):
        _no_use_of_a_segment_before_it_landed('vm', ok[:9] + ['s_waitcnt vmcnt(0)', 'v_mul_f32_e32 v0, s4, v1'] + ok[9:])


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='needs hipcc')
def test_narrow_taps_kernel_isa(tmp_path):
    s = _isa('kn_conv.hip', tmp_path)
    kernels = _kernel_bodies(s, [TAPS])
    # <NT, P, NV, FULL, COEF>: one pixel per wavefront at every width (4 and 8 also masked), with coefficients for NV <= 4 only (5 .. 8 columns run as two column blocks); two pixels for NV = 1 | 2
    # without coefficients
    want = []
    for nt in ('9', '16'):
        for (nv, full) in (('1', '1'), ('2', '1'), ('4', '1'), ('4', '0'), ('8', '1'), ('8', '0')):
            want += [(nt, '1', nv, full, c) for c in (('0', '1') if nv != '8' else ('0',))]
        want += [(nt, '2', nv, '1', '0') for nv in ('1', '2')]
    assert sorted(re.match(TAPS + r'ILi(\d+)ELi(\d)ELi(\d)ELb(\d)ELb(\d)E', k[0]).groups() for k in kernels) == sorted(want), [k[0] for k in kernels]
    for (name, lines) in kernels:
        (nt, pix, nv, full, coef) = re.match(TAPS + r'ILi(\d+)ELi(\d)ELi(\d)ELb(\d)ELb(\d)E', name).groups()
        for l in lines:
            if FUSED.match(l):
                assert any(c in l for c in INT_DIVISION_LITERALS), 'fused multiply-add in %s: %s' % (name, l)
        assert any(re.match(r'v_(pk_)?mul_f32', l) for l in lines), name
        assert any(re.match(r'v_(pk_)?add_f32', l) for l in lines), name
        assert not any(l.startswith('scratch_') or (l.startswith('buffer_store') and 'offen' in l) for l in lines), 'spill in %s' % name
        assert not any(l.startswith('ds_') or l.startswith('s_barrier') for l in lines), 'LDS / barrier in %s' % name
        assert not any(l.startswith('v_writelane') for l in lines), 'scalar registers spilled into vector lanes in %s' % name
        assert any(l.startswith('s_set_gpr_idx_on') or l.startswith('v_movrel') for l in lines), 'no index mode in %s' % name
        # a step's activations are ONE scalar load of NV dwords with the offset in a scalar register
        seg = r's_load_dword%s\s+s\S+,\s*s\[\d+:\d+\],\s*s\d+' % ('' if nv == '1' else 'x' + nv)
        assert sum(1 for l in lines if re.match(seg, l)) >= 9 * int(pix), 'no activation segment loads in %s' % name
        assert not any(re.match(r'(global|flat|buffer)_atomic', l) for l in lines), name
        _no_use_of_a_segment_before_it_landed(name, lines)
        meta = s[s.index('.amdhsa_kernel ' + name):]
        meta = meta[:meta.index('.end_amdhsa_kernel')]
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', meta).group(1)) == 0, name
        assert int(re.search(r'\.amdhsa_next_free_vgpr\s+(\d+)', meta).group(1)) <= 128, name
        assert int(re.search(r'\.amdhsa_group_segment_fixed_size\s+(\d+)', meta).group(1)) == 0, name
    entries = list(re.finditer(r'\.name:\s+(%s\S*)' % TAPS, s))
    assert len(entries) == len(want)
    for m in entries:
        k = re.compile(r'\.private_segment_fixed_size:\s+(\d+)').search(s, m.end())
        assert k and int(k.group(1)) == 0, m.group(1)
