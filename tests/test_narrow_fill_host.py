"""Host-side checks of the tap-resident channel-lane kernel of filled-in operators: the KN_FLAG_NARROW_FILL modifier in the C ABI and its binding
(_capi.KN_MODIFIER_NARROW_FILL), the `narrow_fill` keyword down to KeyedLayer.kernel and its argument rule, the NarrowForm of calls without the keyword, and the gfx950 ISA of
every shipped instantiation of convtaps_narrow_fill_kernel (separate multiplies and adds, nothing spilled -- neither to scratch nor into vector lanes --, no LDS, no
barrier, at most 128 vector registers, the tap picked by the scalar index mode, no use of a scalar register a scalar load still owns)."""
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
from test_narrow_taps_host import _sgprs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = r'_ZN2kn27convtaps_narrow_fill_kernel'


def test_header_declares_the_modifier_and_the_binding_mirrors_it():
    h = open(os.path.join(ROOT, 'include', 'keynet_hip.h')).read()
    m = re.search(r'#define\s+KN_FLAG_NARROW_FILL\s+\(0x([0-9a-f]+)u\)', h)
    assert m and int(m.group(1), 16) == 0x800
    assert _capi.KN_MODIFIER_NARROW_FILL == 0x800
    flags = [getattr(_capi, n) for n in dir(_capi) if n.startswith('KN_FLAG_')]
    assert not any(f & _capi.KN_MODIFIER_NARROW_FILL for f in flags)                    # a bit of its own
    others = [(name, int(value, 0)) for (name, value) in re.findall(r'#define\s+(KN_FLAG_\w+)\s+\(?(0x[0-9a-f]+|\d+)u\)?', h) if name != 'KN_FLAG_NARROW_FILL']
    assert len(others) == len(flags) == 11 and not any(value & 0x800 for (name, value) in others), others
    v = re.search(r'#define\s+KN_ABI_VERSION\s+(\d+)', h)
    assert v and int(v.group(1)) == 5 and _capi.KN_ABI_VERSION == 5   # a modifier of kn_spmm's flags: no entry point added


def test_the_keyword_reaches_every_layer_of_the_python_host():
    for f in (ksys.KeyedModel.forward_linear, ksys.KeyedModel.forward, ksys.KeyedModel.capture, KeyedLayer.forward, KeyedLayer.kernel, KeyedLayer.launch,
              ksp.Conv2dTiledMatrix.torchdot, ksp.FactoredSparseMatrix.torchdot, ksp._run_torchdot, ksp._narrow_args, ksp.NarrowForm.of.__wrapped__):
        p = inspect.signature(f).parameters
        assert 'narrow_fill' in p and p['narrow_fill'].default is False, f


def test_the_argument_rule():
    for narrow in (True, 'mfma'):
        for n in (1, 8):
            assert ksp._narrow_args(n, narrow, False, narrow_fill=True) == (narrow, False)
            assert ksp._narrow_args(n, narrow, True, narrow_fill=True) == (narrow, True)
        with pytest.raises(ValueError):
            ksp._narrow_args(9, narrow, False, narrow_fill=True)              # the widths are those of the other keywords ...
        assert ksp._narrow_args(9, narrow, False, narrow32=True, narrow_fill=True) == (narrow, False)      # ... every one of them
        assert ksp._narrow_args(32, narrow, False, narrow32=True, narrow_fill=True) == (narrow, False)
        assert ksp._narrow_args(4, narrow, False, narrow_taps=True, narrow_fill=True) == (narrow, False)   # combines with narrow_taps
    assert ksp._narrow_args(64, True, False, narrow64=True, narrow_fill=True) == (True, False)
    assert ksp._narrow_args(8, 'mfma', False, narrow_split=True, narrow_fill=True) == ('mfma', False)    # ... and with narrow_split
    for alone in (False, True):
        for other in ({}, dict(narrow_rows=True), dict(narrow_linear=True)):
            with pytest.raises(ValueError, match='narrow_fill=True'):
                ksp._narrow_args(4, False, other.get('narrow_rows', False), alone=alone, narrow_linear=other.get('narrow_linear', False), narrow_fill=True)


def test_calls_without_the_keyword_have_the_form_they_had():
    keywords = [dict(), dict(narrow=True), dict(narrow='mfma'), dict(narrow=True, narrow_rows=True), dict(narrow=True, narrow32=True), dict(narrow=True, narrow64=True),
                dict(narrow='mfma', narrow64='mfma'), dict(narrow=True, narrow_linear=True), dict(narrow='mfma', narrow_split=True), dict(narrow=True, narrow_taps=True),
                dict(narrow='mfma', narrow_split=True, narrow_taps=True)]
    kinds = {(False, False): ksp.NarrowForm, (True, False): ksp.NarrowSplitForm, (False, True): ksp.NarrowTapsForm, (True, True): ksp.NarrowSplitTapsForm}
    twins = {ksp.NarrowForm: ksp.NarrowFillForm, ksp.NarrowSplitForm: ksp.NarrowSplitFillForm, ksp.NarrowTapsForm: ksp.NarrowTapsFillForm, ksp.NarrowSplitTapsForm: ksp.NarrowSplitTapsFillForm}
    assert len(set(twins.values())) == 4
    for kw in keywords:
        for n in (None, 1, 8):
            plain = ksp.NarrowForm.of(n, **kw)
            assert plain == ksp.NarrowForm.of(n, narrow_fill=False, **kw) and plain.fill is False and 'narrow_fill' not in plain.keywords()
            assert type(plain) is kinds[(bool(kw.get('narrow_split')), bool(kw.get('narrow_taps')))]
            if not kw.get('narrow'):
                continue
            fill = ksp.NarrowForm.of(n, narrow_fill=True, **kw)
            assert tuple(fill) == tuple(plain) and fill.fill is True and fill.split == plain.split and fill.taps == plain.taps      # the same six fields
            assert fill != plain and plain != fill and hash(fill) != hash(plain) and fill == ksp.NarrowForm.of(n, narrow_fill=True, **kw)
            assert fill.keywords() == dict(plain.keywords(), narrow_fill=True)
            assert type(fill) is twins[type(plain)]
            assert isinstance(fill, ksp.NarrowSplitForm) == bool(kw.get('narrow_split'))      # a form without narrow_split is no split form
    assert ksp.NarrowForm.of(None, narrow_fill=True).fill is False       # (no batch: nothing is refused, and without `narrow` the keyword says nothing)
    assert type(ksp.NarrowForm.of(None, narrow_fill=True)) is ksp.NarrowForm


@pytest.mark.parametrize('narrow', [True, 'mfma'])
@pytest.mark.parametrize('contract', [True, False, 'auto', 'split', 'bf16x3'])
def test_kernel_adds_the_bit_next_to_kn_flag_narrow_under_every_contract(contract, narrow):
    W = _tiny_conv()
    bit = _capi.KN_MODIFIER_NARROW_FILL
    for relu in (False, True):
        for more in ({}, dict(narrow32=True), dict(narrow64=True), dict(narrow_taps=True)):
            (get_op, flags) = KeyedLayer.kernel(W, contract, relu, narrow=narrow, narrow_fill=True, **more)
            (get_op0, flags0) = KeyedLayer.kernel(W, contract, relu, narrow=narrow, **more)
            assert get_op == get_op0 == W._device_op
            assert not (flags0 & bit)
            assert flags == flags0 | (bit if flags0 & _capi.KN_FLAG_NARROW else 0)
            assert bool(flags0 & _capi.KN_FLAG_NARROW) == (narrow is True or contract in (True, 'auto'))
    assert KeyedLayer.kernel(W, contract, False, narrow_fill=True) == KeyedLayer.kernel(W, contract, False)      # without `narrow`: nothing


@pytest.mark.parametrize('narrow', [True, 'mfma'])
def test_operators_without_a_narrow_form_keep_their_flags(narrow):
    M = scipy.sparse.random(12, 9, density=0.4, format='csr', dtype=np.float32, random_state=1)
    W = ksp.SparseMatrix(M)
    assert not W.narrow_capable()
    for relu in (False, True):
        assert KeyedLayer.kernel(W, True, relu, narrow=narrow, narrow_fill=True)[1] == KeyedLayer.kernel(W, True, relu)[1] == _capi.KN_FLAG_EXACT | (_capi.KN_FLAG_RELU if relu else 0)
    F = _tiny_conv()
    k = KeyedLayer.kernel(ksp.FactoredSparseMatrix(F.tosparse('csr'), F), True, True, narrow=narrow, narrow_fill=True)
    assert k[1] == _capi.KN_FLAG_EXACT | _capi.KN_FLAG_RELU | _capi.KN_FLAG_NARROW | _capi.KN_MODIFIER_NARROW_FILL


# ---- the ISA ---------------------------------------------------------------------------------------------------------------------------------------------------
SCALAR_LOAD = re.compile(r's_load_dword(?:x\d+)?\s+(s\d+|s\[\d+:\d+\]),\s*s\[\d+:\d+\],\s*s\d+\s*$')      # the asm-issued ones: the offset in a scalar register
BRANCH = re.compile(r's_c?branch\w*\s+(\.L\w+)')


def _no_use_of_a_register_before_its_load_landed(name, lines):
    """The record batches and the activations are inline-assembly scalar loads the compiler does not count; the activation loads stand in wave-uniform branches, which the
    compiler lays out of line.  So the rule of test_isa_lint.test_no_use_of_a_scalar_register_owned_by_a_scalar_load_in_flight -- between such a load and the next
    s_waitcnt lgkmcnt(0) nothing names its destination registers -- is checked along the CONTROL FLOW: the set of owned registers at a block's head is the union over its
    predecessors (fixed point), labels and branches from the text.  Returns the number of asm-issued loads."""
    blocks = [['<entry>', []]]
    for l in lines:
        if l.endswith(':'):
            blocks.append([l[:-1], []])
        elif not l.startswith('.'):
            blocks[-1][1].append(l)
            if BRANCH.match(l):                              # (a basic block ends on its branch: what follows is a block of its own, reached by falling through)
                blocks.append(['<behind %s>' % l, []])
    index = {b[0]: k for (k, b) in enumerate(blocks)}
    succ = []
    for (k, (label, body)) in enumerate(blocks):
        out = set()
        fall = True
        for l in body:
            m = BRANCH.match(l)
            if m:
                out.add(index[m.group(1)])
                if l.startswith('s_branch'):
                    fall = False
            if l.startswith('s_endpgm'):
                fall = False
        if fall and k + 1 < len(blocks):
            out.add(k + 1)
        succ.append(out)
    owned_in = [set() for _ in blocks]
    loads = 0

    def run(k, check):
        owned = set(owned_in[k])
        n = 0
        for l in blocks[k][1]:
            if l.startswith('s_waitcnt') and 'lgkmcnt(0)' in l:
                owned = set()
                continue
            m = SCALAR_LOAD.match(l)
            if m:
                dst = _sgprs(m.group(1))
                if check:
                    assert not (dst & _sgprs(l[l.index(',') + 1:])), 'a scalar load overwrites its own address in %s: %s' % (name, l)
                    assert not (dst & owned), 'two scalar loads in flight into the same registers in %s: %s' % (name, l)
                owned |= dst
                n += 1
                continue
            if check and owned:
                assert not (_sgprs(l) & owned), 'a register whose load has not landed is used in %s (%s): %s' % (name, blocks[k][0], l)
        return (owned, n)

    changed = True
    while changed:
        changed = False
        for k in range(len(blocks)):
            (out, _) = run(k, False)
            for j in succ[k]:
                if not out <= owned_in[j]:
                    owned_in[j] |= out
                    changed = True
    for k in range(len(blocks)):
        loads += run(k, True)[1]
    return loads


def test_the_landing_check_follows_branches():
    ok = ['s_load_dwordx8 s[8:15], s[4:5], s3', 's_waitcnt lgkmcnt(0)', 's_bitcmp1_b32 s11, 0', 's_cbranch_scc1 .LBB0_3', '.LBB0_1:', 'v_mul_f32_e32 v0, s20, v1',
          's_load_dwordx8 s[8:15], s[4:5], s3', 's_waitcnt lgkmcnt(0)', 's_cbranch_scc0 .LBB0_1', 's_endpgm', '.LBB0_3:', 's_load_dword s20, s[6:7], s8', 's_branch .LBB0_4',
          '.LBB0_4:', 's_waitcnt lgkmcnt(0)', 's_branch .LBB0_1']
    assert _no_use_of_a_register_before_its_load_landed('ok', ok) == 3
    bad = list(ok)
    bad[bad.index('.LBB0_4:') + 1] = 's_nop 0'           # the out-of-line load now reaches the multiply without a wait
    with pytest.raises(AssertionError, match='has not landed'):
        _no_use_of_a_register_before_its_load_landed('bad', bad)
    with pytest.raises(AssertionError, match='has not landed'):
        _no_use_of_a_register_before_its_load_landed('copy', ok[:1] + ['s_mov_b64 s[30:31], s[8:9]'] + ok[1:])


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='needs hipcc')
def test_narrow_fill_kernel_isa(tmp_path):
    s = _isa('kn_conv.hip', tmp_path)
    kernels = _kernel_bodies(s, [FILL])
    # <NV, FULL>: every width, 4 and 8 also masked; one form for operators with coefficients and without
    want = [('1', '1'), ('2', '1'), ('4', '1'), ('4', '0'), ('8', '1'), ('8', '0')]
    assert sorted(re.match(FILL + r'ILi(\d)ELb(\d)E', k[0]).groups() for k in kernels) == sorted(want), [k[0] for k in kernels]
    for (name, lines) in kernels:
        (nv, full) = re.match(FILL + r'ILi(\d)ELb(\d)E', name).groups()
        for l in lines:
            if FUSED.match(l):
                assert any(c in l for c in INT_DIVISION_LITERALS), 'fused multiply-add in %s: %s' % (name, l)
        assert any(re.match(r'v_(pk_)?mul_f32', l) for l in lines), name
        assert any(re.match(r'v_(pk_)?add_f32', l) for l in lines), name
        assert not any(l.startswith('scratch_') or (l.startswith('buffer_store') and 'offen' in l) for l in lines), 'spill in %s' % name
        assert not any(l.startswith('ds_') or l.startswith('s_barrier') for l in lines), 'LDS / barrier in %s' % name
        assert not any(l.startswith('v_writelane') for l in lines), 'scalar registers spilled into vector lanes in %s' % name
        assert any(l.startswith('s_set_gpr_idx_on') or l.startswith('v_movrel') for l in lines), 'no index mode in %s' % name
        assert not any(re.match(r'(global|flat|buffer)_atomic', l) for l in lines), name
        # the records: one scalar load per batch (4 records at NV = 1 | 2, 2 from NV = 4 on); a stored column's activations: ONE scalar load of NV dwords
        assert any(re.match(r's_load_dwordx%d\s+s\[\d+:\d+\],\s*s\[\d+:\d+\],\s*s\d+' % (16 if nv in '12' else 8), l) for l in lines), 'no record batches in %s' % name
        seg = r's_load_dword%s\s+s\S+,\s*s\[\d+:\d+\],\s*s\d+' % ('' if nv == '1' else 'x' + nv)
        assert sum(1 for l in lines if re.match(seg, l)) >= 4, 'no activation segment loads in %s' % name
        assert _no_use_of_a_register_before_its_load_landed(name, lines) >= 8, name
        meta = s[s.index('.amdhsa_kernel ' + name):]
        meta = meta[:meta.index('.end_amdhsa_kernel')]
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', meta).group(1)) == 0, name
        assert int(re.search(r'\.amdhsa_next_free_vgpr\s+(\d+)', meta).group(1)) <= 128, name
        assert int(re.search(r'\.amdhsa_group_segment_fixed_size\s+(\d+)', meta).group(1)) == 0, name
    entries = list(re.finditer(r'\.name:\s+(%s\S*)' % FILL, s))
    assert len(entries) == len(want)
    for m in entries:
        k = re.compile(r'\.private_segment_fixed_size:\s+(\d+)').search(s, m.end())
        assert k and int(k.group(1)) == 0, m.group(1)
