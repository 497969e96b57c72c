"""Host-side checks of the channel-pair tap-resident kernel for 1 .. 8 batch columns: the KN_MODIFIER_NARROW_TAPS_PAIRS bit in the C ABI and its binding, the
narrow_taps='pairs' value of the `narrow_taps` keyword down to KeyedLayer.kernel and its argument rule, the NarrowForm of such calls, and the gfx950 ISA of every
shipped instantiation of convtaps_narrow_taps_pairs_kernel (packed multiplies with a scalar activation operand and packed adds and no fused multiply-add, nothing
spilled -- neither to scratch nor into vector lanes --, no LDS, no barrier, no atomics, at most 128 vector registers, the tap pair picked by the scalar index mode, a
step's activations one scalar load with the offset in a scalar register and used only behind the wait for them)."""
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
PAIRS = r'_ZN2kn33convtaps_narrow_taps_pairs_kernel'
BIT = 0x2000


def test_header_declares_the_bit_and_the_binding_mirrors_it():
    h = open(os.path.join(ROOT, 'include', 'keynet_hip.h')).read()
    m = re.search(r'#define\s+KN_MODIFIER_NARROW_TAPS_PAIRS\s+\(0x([0-9a-f]+)u\)', h)
    assert m and int(m.group(1), 16) == BIT
    assert _capi.KN_MODIFIER_NARROW_TAPS_PAIRS == BIT
    flags = [getattr(_capi, n) for n in dir(_capi) if n.startswith('KN_FLAG_')]
    assert flags and not any(f & BIT for f in flags)                    # a bit of its own
    assert not (_capi.KN_MODIFIER_NARROW_FILL & BIT) and not (_capi.KN_MODIFIER_NARROW_TAPS32 & BIT)
    declared = [(name, int(v, 0)) for (name, v) in re.findall(r'#define\s+(KN_(?:FLAG|MODIFIER)_\w+)\s+\(?(0x[0-9a-f]+|\d+)u\)?', h)]
    assert len(declared) > 11 and [name for (name, v) in declared if v & BIT] == ['KN_MODIFIER_NARROW_TAPS_PAIRS']
    v = re.search(r'#define\s+KN_ABI_VERSION\s+(\d+)', h)
    assert v and int(v.group(1)) == 5 and _capi.KN_ABI_VERSION == 5   # a modifier of kn_spmm's flags: no entry point added


def _rule(n, narrow, narrow_rows, value, **kw):
    try:
        return ksp._narrow_args(n, narrow, narrow_rows, narrow_taps=value, **kw)
    except ValueError:
        return ValueError


def test_the_argument_rule_of_pairs_is_that_of_packed():
    seen = set()
    for n in (1, 4, 8, 9, 16, 32, 33, 64, 65):
        for narrow in (False, True, 'mfma'):
            for rows in (False, True):
                for more in ({}, dict(narrow32=True), dict(narrow64=True), dict(narrow64='mfma'), dict(narrow_linear=True), dict(narrow_split=True), dict(narrow_fill=True),
                             dict(alone=True), dict(alone=True, narrow32=True)):
                    got = _rule(n, narrow, rows, 'pairs', **more)
                    assert got == _rule(n, narrow, rows, 'packed', **more), (n, narrow, rows, more)
                    seen.add(got is ValueError)
    assert seen == {False, True}
    for alone in (False, True):
        with pytest.raises(ValueError, match='narrow_taps'):
            ksp._narrow_args(4, False, False, alone=alone, narrow_taps='pairs')            # not without `narrow`
    for narrow in (True, 'mfma'):
        with pytest.raises(ValueError):
            ksp._narrow_args(9, narrow, False, narrow_taps='pairs')                         # nine images need narrow32
        assert ksp._narrow_args(8, narrow, True, narrow_taps='pairs') == (narrow, True)
        assert ksp._narrow_args(32, narrow, False, narrow32=True, narrow_taps='pairs') == (narrow, False)


@pytest.mark.parametrize('narrow', [True, 'mfma'])
@pytest.mark.parametrize('contract', [True, False, 'auto', 'split', 'bf16x3'])
def test_kernel_adds_the_three_bits_exactly_where_true_adds_kn_flag_narrow_taps(contract, narrow):
    W = _tiny_conv()
    three = _capi.KN_FLAG_NARROW_TAPS | _capi.KN_MODIFIER_NARROW_TAPS32 | BIT
    for relu in (False, True):
        for more in ({}, dict(narrow32=True), dict(narrow64=True)):
            (get_op, flags) = KeyedLayer.kernel(W, contract, relu, narrow=narrow, narrow_taps='pairs', **more)
            (get_op2, flags2) = KeyedLayer.kernel(W, contract, relu, narrow=narrow, narrow_taps='packed', **more)
            (get_op1, flags1) = KeyedLayer.kernel(W, contract, relu, narrow=narrow, narrow_taps=True, **more)
            (get_op0, flags0) = KeyedLayer.kernel(W, contract, relu, narrow=narrow, **more)
            assert get_op == get_op2 == get_op1 == get_op0 == W._device_op
            assert not (flags2 & BIT) and not (flags1 & BIT) and not (flags0 & BIT)          # every other keyword value keeps its flag word
            assert flags1 == flags0 | (_capi.KN_FLAG_NARROW_TAPS if flags0 & _capi.KN_FLAG_NARROW else 0)
            assert flags2 == flags1 | (_capi.KN_MODIFIER_NARROW_TAPS32 if flags1 & _capi.KN_FLAG_NARROW_TAPS else 0)
            assert flags == flags0 | (three if flags1 & _capi.KN_FLAG_NARROW_TAPS else 0)
            assert bool(flags & BIT) == bool(flags0 & _capi.KN_FLAG_NARROW)
    assert KeyedLayer.kernel(W, contract, False, narrow_taps='pairs') == KeyedLayer.kernel(W, contract, False)      # without `narrow`: nothing


def test_forms_of_pairs_calls_and_of_all_other_calls():
    keywords = [dict(narrow=True), dict(narrow='mfma'), dict(narrow=True, narrow_rows=True), dict(narrow=True, narrow32=True), dict(narrow=True, narrow64=True),
                dict(narrow='mfma', narrow64='mfma'), dict(narrow=True, narrow_linear=True), dict(narrow='mfma', narrow_split=True), dict(narrow=True, narrow_fill=True),
                dict(narrow='mfma', narrow_split=True, narrow_fill=True)]
    for kw in keywords:
        for n in (None, 1, 8):
            plain = ksp.NarrowForm.of(n, **kw)
            taps = ksp.NarrowForm.of(n, narrow_taps=True, **kw)
            packed = ksp.NarrowForm.of(n, narrow_taps='packed', **kw)
            pairs = ksp.NarrowForm.of(n, narrow_taps='pairs', **kw)
            assert tuple(pairs) == tuple(packed) == tuple(taps) == tuple(plain)             # the six fields
            for other in (plain, taps, packed):
                assert pairs != other and other != pairs
            assert len({hash(pairs), hash(packed), hash(taps), hash(plain)}) == 4
            assert pairs == ksp.NarrowForm.of(n, narrow_taps='pairs', **kw) and hash(pairs) == hash(ksp.NarrowForm.of(n, narrow_taps='pairs', **kw))
            assert pairs.taps == 'pairs' and pairs.split == plain.split and pairs.fill == plain.fill
            assert isinstance(pairs, type(taps)) and not isinstance(pairs, type(packed)) and isinstance(pairs, ksp.NarrowSplitForm) == bool(kw.get('narrow_split'))
            assert pairs.keywords() == dict(plain.keywords(), narrow_taps='pairs')
            assert ksp.NarrowForm.of(n, **pairs.keywords()) == pairs                         # round trip
            # the forms of the calls without 'pairs' are what they were
            assert taps.taps is True and taps.keywords() == dict(plain.keywords(), narrow_taps=True) and plain.taps is False and 'narrow_taps' not in plain.keywords()
            assert packed.taps == 'packed' and packed.keywords() == dict(plain.keywords(), narrow_taps='packed')
            assert type(plain) in (ksp.NarrowForm, ksp.NarrowSplitForm, ksp.NarrowFillForm, ksp.NarrowSplitFillForm)
            assert type(taps) in (ksp.NarrowTapsForm, ksp.NarrowSplitTapsForm, ksp.NarrowTapsFillForm, ksp.NarrowSplitTapsFillForm)
            assert type(packed) in (ksp.NarrowPackedForm, ksp.NarrowSplitPackedForm, ksp.NarrowPackedFillForm, ksp.NarrowSplitPackedFillForm)
            assert type(pairs) in (ksp.NarrowPairsForm, ksp.NarrowSplitPairsForm, ksp.NarrowPairsFillForm, ksp.NarrowSplitPairsFillForm)
    assert type(ksp.NarrowForm.of(16, True, narrow32=True, narrow_taps='pairs')) is ksp.NarrowPairsForm
    assert type(ksp.NarrowForm.of(16, True, narrow32=True, narrow_taps='packed')) is ksp.NarrowPackedForm
    assert ksp.NarrowForm.of(None, narrow_taps='pairs').taps is False and type(ksp.NarrowForm.of(None, narrow_taps='pairs')) is ksp.NarrowForm      # without `narrow` the keyword says nothing


# <NT, NV, FULL, COEF>: 9 | 16 value rows, NV = 1 | 2 | 4 | 8, the masked forms for NV = 4 | 8; with coefficients NV <= 4 (all six of them compile clean).  The forms
# with coefficients at NV = 8 are not instantiated, as convtaps_narrow_taps_kernel's are not: an operator with coefficients runs 5 .. 8 columns as two column blocks
# (NV = 4, and the form of the other 1 .. 4 columns), both on this kernel.
SHIPPED = sorted((nt, nv, full, coef) for nt in ('9', '16') for (nv, full) in (('1', '1'), ('2', '1'), ('4', '1'), ('4', '0'), ('8', '1'), ('8', '0'))
                 for coef in (('0', '1') if nv != '8' else ('0',)))


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='needs hipcc')
def test_narrow_taps_pairs_kernel_isa(tmp_path):
    s = _isa('kn_conv.hip', tmp_path)
    kernels = _kernel_bodies(s, [PAIRS])
    sig = PAIRS + r'ILi(\d+)ELi(\d+)ELb(\d)ELb(\d)E'
    assert sorted(re.match(sig, k[0]).groups() for k in kernels) == SHIPPED, [k[0] for k in kernels]
    for (name, lines) in kernels:
        (nt, nv, full, coef) = re.match(sig, name).groups()
        nv = int(nv)
        for l in lines:
            if FUSED.match(l):
                assert any(c in l for c in INT_DIVISION_LITERALS), 'fused multiply-add in %s: %s' % (name, l)
        (n_mul, n_add) = (sum(1 for l in lines if l.startswith('v_pk_mul_f32')), sum(1 for l in lines if l.startswith('v_pk_add_f32')))
        assert n_mul >= 9 * nv and n_add >= 9 * nv, (name, n_mul, n_add)                    # NV of each per unrolled step
        # the walk's multiplies: (tap of co0, tap of co1) times one activation -- the half of an aligned scalar pair that op_sel / op_sel_hi broadcast to both halves
        # (the compiler may pack the epilogue's bias products by itself, vector pair times vector pair)
        walk = [l for l in lines if l.startswith('v_pk_mul_f32') and ' s[' in l]
        assert len(walk) >= 9 * nv, name
        for l in walk:
            m = re.match(r'v_pk_mul_f32 v\[\d+:\d+\], s\[(\d+):(\d+)\], v\[\d+:\d+\] op_sel:\[([01]),0\] op_sel_hi:\[([01]),1\]$', l)
            assert m and int(m.group(1)) % 2 == 0 and int(m.group(2)) == int(m.group(1)) + 1 and m.group(3) == m.group(4), (name, l)
        assert not any(l.startswith('scratch_') or (l.startswith('buffer_store') and 'offen' in l) for l in lines), 'spill in %s' % name
        assert not any(l.startswith('ds_') or l.startswith('s_barrier') for l in lines), 'LDS / barrier in %s' % name
        assert not any(l.startswith('v_writelane') for l in lines), 'scalar registers spilled into vector lanes in %s' % name
        assert not any(re.match(r'(global|flat|buffer)_atomic', l) for l in lines), name
        assert any(l.startswith('s_set_gpr_idx_on') or l.startswith('v_movrel') for l in lines), 'no index mode in %s' % name
        # a step's activations are ONE scalar load of NV dwords with the offset in a scalar register: 9 per unrolled channel
        seg = r's_load_dword%s\s+s\S+,\s*s\[\d+:\d+\],\s*s\d+\s*$' % ('' if nv == 1 else 'x%d' % nv)
        assert sum(1 for l in lines if re.match(seg, l)) >= 9, 'no activation segment loads in %s' % name
        _no_use_of_a_segment_before_it_landed(name, lines)
        meta = s[s.index('.amdhsa_kernel ' + name):]
        meta = meta[:meta.index('.end_amdhsa_kernel')]
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', meta).group(1)) == 0, name
        assert int(re.search(r'\.amdhsa_group_segment_fixed_size\s+(\d+)', meta).group(1)) == 0, name
        assert int(re.search(r'\.amdhsa_next_free_vgpr\s+(\d+)', meta).group(1)) <= 128, name
    entries = list(re.finditer(r'\.name:\s+(%s\S*)' % PAIRS, s))
    assert len(entries) == len(SHIPPED)
    for m in entries:
        k = re.compile(r'\.private_segment_fixed_size:\s+(\d+)').search(s, m.end())
        assert k and int(k.group(1)) == 0, m.group(1)
