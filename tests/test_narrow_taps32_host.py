"""Host-side checks of the packed tap-resident channel-lane kernel for 9 .. 32 batch columns: the KN_MODIFIER_NARROW_TAPS32 bit in the C ABI and its binding, the
narrow_taps='packed' value of the `narrow_taps` keyword down to KeyedLayer.kernel and its argument rule, the NarrowForm of such calls, and the gfx950 ISA of every
shipped instantiation of convtaps_narrow_taps32_kernel (packed multiplies and packed adds and no fused multiply-add, nothing spilled -- neither to scratch nor into
vector lanes --, no LDS, no barrier, no atomics, at most 128 vector registers, the tap picked by the scalar index mode, the activation segments loaded with the offset
in a scalar register and used only behind the wait for them)."""
import os
import re
import shutil

import pytest

from keynet_amd import _capi
from keynet_amd import sparse as ksp
from keynet_amd.layer import KeyedLayer
from test_isa_lint import _isa, _kernel_bodies, FUSED, INT_DIVISION_LITERALS
from test_narrow_host import _tiny_conv
from test_narrow_taps_host import _no_use_of_a_segment_before_it_landed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAPS32 = r'_ZN2kn29convtaps_narrow_taps32_kernel'
BIT = 0x1000


def test_header_declares_the_bit_and_the_binding_mirrors_it():
    h = open(os.path.join(ROOT, 'include', 'keynet_hip.h')).read()
    m = re.search(r'#define\s+KN_MODIFIER_NARROW_TAPS32\s+\(0x([0-9a-f]+)u\)', h)
    assert m and int(m.group(1), 16) == BIT
    assert _capi.KN_MODIFIER_NARROW_TAPS32 == BIT
    flags = [getattr(_capi, n) for n in dir(_capi) if n.startswith('KN_FLAG_')]
    assert flags and not any(f & BIT for f in flags) and not (_capi.KN_MODIFIER_NARROW_FILL & BIT)          # a bit of its own
    declared = [int(v, 0) for (name, v) in re.findall(r'#define\s+(KN_FLAG_\w+)\s+\(?(0x[0-9a-f]+|\d+)u\)?', h)]
    assert declared and not any(v & BIT for v in declared)
    v = re.search(r'#define\s+KN_ABI_VERSION\s+(\d+)', h)
    assert v and int(v.group(1)) == 5 and _capi.KN_ABI_VERSION == 5   # a modifier of kn_spmm's flags: no entry point added


def test_the_argument_rule_of_packed_is_that_of_true():
    for alone in (False, True):
        with pytest.raises(ValueError, match='narrow_taps'):
            ksp._narrow_args(16, False, False, alone=alone, narrow_taps='packed')          # not without `narrow`
        with pytest.raises(ValueError, match='narrow_taps'):
            ksp._narrow_args(4, False, False, alone=alone, narrow32=True, narrow_taps='packed')
    for narrow in (True, 'mfma'):
        with pytest.raises(ValueError):
            ksp._narrow_args(9, narrow, False, narrow_taps='packed')                       # nine images need narrow32
        for n in (1, 8):
            assert ksp._narrow_args(n, narrow, False, narrow_taps='packed') == (narrow, False)
            assert ksp._narrow_args(n, narrow, True, narrow_taps='packed') == (narrow, True)
        for n in (9, 32):
            assert ksp._narrow_args(n, narrow, False, narrow32=True, narrow_taps='packed') == (narrow, False)
        with pytest.raises(ValueError):
            ksp._narrow_args(33, narrow, False, narrow32=True, narrow_taps='packed')
        with pytest.raises(ValueError):
            ksp._narrow_args(9, narrow, True, narrow32=True, narrow_taps='packed')         # narrow_rows keeps its eight columns
    assert ksp._narrow_args(64, True, False, narrow64=True, narrow_taps='packed') == (True, False)
    assert ksp._narrow_args(8, 'mfma', False, narrow_split=True, narrow_taps='packed') == ('mfma', False)


@pytest.mark.parametrize('narrow', [True, 'mfma'])
@pytest.mark.parametrize('contract', [True, False, 'auto', 'split', 'bf16x3'])
def test_kernel_adds_both_bits_exactly_where_true_adds_kn_flag_narrow_taps(contract, narrow):
    W = _tiny_conv()
    for relu in (False, True):
        for more in ({}, dict(narrow32=True), dict(narrow64=True)):
            (get_op, flags) = KeyedLayer.kernel(W, contract, relu, narrow=narrow, narrow_taps='packed', **more)
            (get_op1, flags1) = KeyedLayer.kernel(W, contract, relu, narrow=narrow, narrow_taps=True, **more)
            (get_op0, flags0) = KeyedLayer.kernel(W, contract, relu, narrow=narrow, **more)
            assert get_op == get_op1 == get_op0 == W._device_op
            assert not (flags1 & BIT) and not (flags0 & BIT)
            assert flags == flags1 | (BIT if flags1 & _capi.KN_FLAG_NARROW_TAPS else 0)
            assert bool(flags & BIT) == bool(flags0 & _capi.KN_FLAG_NARROW)
    assert KeyedLayer.kernel(W, contract, False, narrow_taps='packed') == KeyedLayer.kernel(W, contract, False)      # without `narrow`: nothing


def test_forms_of_packed_calls_and_of_all_other_calls():
    keywords = [dict(narrow=True), dict(narrow='mfma'), dict(narrow=True, narrow_rows=True), dict(narrow=True, narrow32=True), dict(narrow=True, narrow64=True),
                dict(narrow='mfma', narrow64='mfma'), dict(narrow=True, narrow_linear=True), dict(narrow='mfma', narrow_split=True), dict(narrow=True, narrow_fill=True),
                dict(narrow='mfma', narrow_split=True, narrow_fill=True)]
    for kw in keywords:
        for n in (None, 1, 8):
            plain = ksp.NarrowForm.of(n, **kw)
            taps = ksp.NarrowForm.of(n, narrow_taps=True, **kw)
            packed = ksp.NarrowForm.of(n, narrow_taps='packed', **kw)
            assert tuple(packed) == tuple(taps) == tuple(plain)                              # the six fields
            assert packed != plain and plain != packed and packed != taps and taps != packed
            assert len({hash(packed), hash(taps), hash(plain)}) == 3
            assert packed == ksp.NarrowForm.of(n, narrow_taps='packed', **kw) and hash(packed) == hash(ksp.NarrowForm.of(n, narrow_taps='packed', **kw))
            assert packed.taps == 'packed' and packed.split == plain.split and packed.fill == plain.fill
            assert isinstance(packed, type(taps)) and isinstance(packed, ksp.NarrowSplitForm) == bool(kw.get('narrow_split'))
            assert packed.keywords() == dict(plain.keywords(), narrow_taps='packed')
            assert ksp.NarrowForm.of(n, **packed.keywords()) == packed                       # round trip
            # the forms of the calls without 'packed' are what they were
            assert taps.taps is True and taps.keywords() == dict(plain.keywords(), narrow_taps=True) and plain.taps is False and 'narrow_taps' not in plain.keywords()
            assert type(plain) in (ksp.NarrowForm, ksp.NarrowSplitForm, ksp.NarrowFillForm, ksp.NarrowSplitFillForm)
            assert type(taps) in (ksp.NarrowTapsForm, ksp.NarrowSplitTapsForm, ksp.NarrowTapsFillForm, ksp.NarrowSplitTapsFillForm)
    assert type(ksp.NarrowForm.of(16, True, narrow32=True)) is ksp.NarrowForm
    assert type(ksp.NarrowForm.of(16, True, narrow32=True, narrow_taps=True)) is ksp.NarrowTapsForm
    assert type(ksp.NarrowForm.of(16, True, narrow32=True, narrow_taps='packed')) is ksp.NarrowPackedForm
    assert ksp.NarrowForm.of(None, narrow_taps='packed').taps is False and type(ksp.NarrowForm.of(None, narrow_taps='packed')) is ksp.NarrowForm      # without `narrow` the keyword says nothing


# <NT, NV, FULL, COEF>: 9 | 16 value rows, blocks of 8 | 16 | 32 columns, full and masked; with coefficients the 8-column blocks only (at 16 and 32 columns the nine
# resident coefficients next to 32 scalar registers of activations spilled scalar registers into vector lanes: not instantiated, those calls keep convtaps_narrow32_kernel)
SHIPPED = sorted((nt, nv, full, coef) for nt in ('9', '16') for nv in ('8', '16', '32') for full in ('0', '1') for coef in (('0', '1') if nv == '8' else ('0',)))


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='needs hipcc')
def test_narrow_taps32_kernel_isa(tmp_path):
    s = _isa('kn_conv.hip', tmp_path)
    kernels = _kernel_bodies(s, [TAPS32])
    sig = TAPS32 + r'ILi(\d+)ELi(\d+)ELb(\d)ELb(\d)E'
    assert sorted(re.match(sig, k[0]).groups() for k in kernels) == SHIPPED, [k[0] for k in kernels]
    for (name, lines) in kernels:
        (nt, nv, full, coef) = re.match(sig, name).groups()
        nv = int(nv)
        for l in lines:
            if FUSED.match(l):
                assert any(c in l for c in INT_DIVISION_LITERALS), 'fused multiply-add in %s: %s' % (name, l)
        (n_mul, n_add) = (sum(1 for l in lines if l.startswith('v_pk_mul_f32')), sum(1 for l in lines if l.startswith('v_pk_add_f32')))
        assert n_mul >= 9 * nv // 2 and n_add >= 9 * nv // 2, (name, n_mul, n_add)             # NV / 2 of each per unrolled step
        # the column pair is a sub-register pair of the segment, named in the multiply: an aligned scalar pair, the term broadcast from the low half of a vector pair
        # (the compiler packs the epilogue's bias products by itself, vector pair times vector pair: the walk's multiplies are the ones with a scalar operand)
        packed = [l for l in lines if l.startswith('v_pk_mul_f32') and ' s[' in l]
        assert len(packed) >= 9 * nv // 2 and all(re.match(r'v_pk_mul_f32 v\[\d+:\d+\], s\[(\d*[02468]):\d+\], v\[\d+:\d+\] op_sel_hi:\[1,0\]$', l) for l in packed), name
        assert not any(l.startswith('scratch_') or (l.startswith('buffer_store') and 'offen' in l) for l in lines), 'spill in %s' % name
        assert not any(l.startswith('ds_') or l.startswith('s_barrier') for l in lines), 'LDS / barrier in %s' % name
        assert not any(l.startswith('v_writelane') for l in lines), 'scalar registers spilled into vector lanes in %s' % name
        assert not any(re.match(r'(global|flat|buffer)_atomic', l) for l in lines), name
        assert any(l.startswith('s_set_gpr_idx_on') or l.startswith('v_movrel') for l in lines), 'no index mode in %s' % name
        # a step's activations: scalar loads of 16 dwords (NV = 8: 8) with the offset in a scalar register -- 9 NV / W of them per unrolled channel
        w = min(nv, 16)
        seg = r's_load_dwordx%d\s+s\[\d+:\d+\],\s*s\[\d+:\d+\],\s*s\d+\s*$' % w
        assert sum(1 for l in lines if re.match(seg, l)) >= 9 * nv // w, 'no activation segment loads in %s' % name
        _no_use_of_a_segment_before_it_landed(name, lines)
        # no scalar copy per column pair inside the walk: the few s_mov_b64 of a body are loop bookkeeping (far fewer than one per packed multiply)
        assert sum(1 for l in lines if l.startswith('s_mov_b64')) < 9, name
        meta = s[s.index('.amdhsa_kernel ' + name):]
        meta = meta[:meta.index('.end_amdhsa_kernel')]
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', meta).group(1)) == 0, name
        assert int(re.search(r'\.amdhsa_group_segment_fixed_size\s+(\d+)', meta).group(1)) == 0, name
        assert int(re.search(r'\.amdhsa_next_free_vgpr\s+(\d+)', meta).group(1)) <= 128, name
    entries = list(re.finditer(r'\.name:\s+(%s\S*)' % TAPS32, s))
    assert len(entries) == len(SHIPPED)
    for m in entries:
        k = re.compile(r'\.private_segment_fixed_size:\s+(\d+)').search(s, m.end())
        assert k and int(k.group(1)) == 0, m.group(1)
