"""Host-side checks of the low-latency forward for 33 .. 64 images: the KN_FLAG_NARROW64 modifier in the C ABI and its binding, the `narrow64` keyword down to
KeyedLayer.kernel and its argument rules, and the gfx950 ISA of convtaps_exact_pipe64_kernel -- the order-preserving pipeline with one column per lane: separate packed
multiplies and adds over output-channel pairs (RBX / 2 of each per step), nothing spilled, no LDS, at most 128 vector registers, and no use of a row register while its
asm-issued load is in flight."""
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
from test_isa_lint import _isa, _kernel_bodies, _regs, FUSED, INT_DIVISION_LITERALS
from test_narrow_host import _tiny_conv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPE64 = r'_ZN2kn28convtaps_exact_pipe64_kernel'
ROW_LOAD = re.compile(r'global_load_dword (v\d+), v\d+, s\[')       # the asm-issued activation-row load: saddr form, one dword per lane


def test_header_declares_the_modifier_and_the_binding_mirrors_it():
    h = open(os.path.join(ROOT, 'include', 'keynet_hip.h')).read()
    m = re.search(r'#define\s+KN_FLAG_NARROW64\s+(\w+)u\b', h)
    assert m and int(m.group(1), 0) == 128
    assert _capi.KN_FLAG_NARROW64 == 128
    flags = [_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_BF16X3, _capi.KN_FLAG_NARROW, _capi.KN_FLAG_NARROW_MFMA, _capi.KN_FLAG_NARROW_ROWS, _capi.KN_FLAG_NARROW32,
             _capi.KN_FLAG_NARROW64]
    assert sorted(flags) == [1, 2, 4, 8, 16, 32, 64, 128]             # one bit each
    assert sorted(int(v, 0) for v in re.findall(r'#define\s+KN_FLAG_\w+\s+(\w+)u\b', h)) == [1, 2, 4, 8, 16, 32, 64, 128]
    v = re.search(r'#define\s+KN_ABI_VERSION\s+(\d+)', h)
    assert v and int(v.group(1)) == 5 and _capi.KN_ABI_VERSION == 5   # a modifier of kn_spmm's flags: no entry point added
    assert ksys.KeyedModel.NARROW64_MAX == 64 and ksp.NARROW64_MAX == 64
    assert ksys.KeyedModel.NARROW32_MAX == 32 and ksys.KeyedModel.NARROW_MAX == 8
    assert '(D + 1) * ldx < 2^31' in h[h.index('KN_FLAG_NARROW64 (33 <= n_vecs <= 64)'):][:160]      # the line of the leading-dimension table


def test_the_keyword_reaches_every_layer_of_the_python_host():
    for f in (ksys.KeyedModel.forward_linear, ksys.KeyedModel.forward, ksys.KeyedModel.capture, KeyedLayer.forward, KeyedLayer.kernel, KeyedLayer.launch,
              ksp.Conv2dTiledMatrix.torchdot, ksp.FactoredSparseMatrix.torchdot, ksp._run_torchdot, ksp._narrow_args):
        p = inspect.signature(f).parameters
        assert 'narrow64' in p and p['narrow64'].default is False, f


def test_the_argument_rules():
    for n in (1, 8, 9, 32, 33, 64):
        assert ksp._narrow_args(n, True, False, narrow64=True) == (True, False)
        assert ksp._narrow_args(n, True, False, narrow32=True, narrow64=True) == (True, False)
    for n in (1, 8, 9, 32):
        assert ksp._narrow_args(n, 'mfma', False, narrow64=True) == ('mfma', False)       # at most 32 images: exactly narrow32=True
    for n in (33, 64):
        with pytest.raises(ValueError, match='no matrix-core form'):
            ksp._narrow_args(n, 'mfma', False, narrow64=True)
    for narrow in (True, 'mfma'):
        with pytest.raises(ValueError):
            ksp._narrow_args(65, narrow, False, narrow64=True)
        with pytest.raises(ValueError):
            ksp._narrow_args(33, narrow, False, narrow32=True)        # without the keyword the limits are where they were
        with pytest.raises(ValueError):
            ksp._narrow_args(9, narrow, False)
        with pytest.raises(ValueError):
            ksp._narrow_args(9, narrow, True, narrow64=True)          # the row-lane kernel is an 8-column kernel
        assert ksp._narrow_args(8, narrow, True, narrow64=True) == (narrow, True)
    for alone in (False, True):
        for n in (4, 40):
            with pytest.raises(ValueError):
                ksp._narrow_args(n, False, False, alone=alone, narrow64=True)   # only together with `narrow`


@pytest.mark.parametrize('narrow', [True, 'mfma'])
@pytest.mark.parametrize('contract', [True, False, 'auto', 'split', 'bf16x3'])
def test_kernel_adds_both_modifiers_on_a_conv_operator_under_every_contract(contract, narrow):
    W = _tiny_conv()
    for relu in (False, True):
        (get_op, flags) = KeyedLayer.kernel(W, contract, relu, narrow=narrow, narrow64=True)
        (get_op0, flags0) = KeyedLayer.kernel(W, contract, relu, narrow=narrow)
        assert get_op == get_op0 == W._device_op
        assert not (flags0 & (_capi.KN_FLAG_NARROW32 | _capi.KN_FLAG_NARROW64))
        assert flags == flags0 | _capi.KN_FLAG_NARROW32 | _capi.KN_FLAG_NARROW64
        assert KeyedLayer.kernel(W, contract, relu, narrow=narrow, narrow32=True, narrow64=True)[1] == flags
        assert KeyedLayer.kernel(W, contract, relu, narrow=narrow, narrow32=True)[1] == flags0 | _capi.KN_FLAG_NARROW32
    assert KeyedLayer.kernel(W, contract, False, narrow64=True) == KeyedLayer.kernel(W, contract, False)      # without `narrow`: nothing
    if narrow is True:
        assert KeyedLayer.kernel(W, contract, True, narrow=True, narrow64=True)[1] & ~(_capi.KN_FLAG_EXACT | _capi.KN_FLAG_BF16X3) == \
            _capi.KN_FLAG_RELU | _capi.KN_FLAG_NARROW | _capi.KN_FLAG_NARROW32 | _capi.KN_FLAG_NARROW64


@pytest.mark.parametrize('narrow', [True, 'mfma'])
def test_operators_without_a_narrow_form_keep_their_flags(narrow):
    M = scipy.sparse.random(12, 9, density=0.4, format='csr', dtype=np.float32, random_state=1)
    W = ksp.SparseMatrix(M)
    assert not W.narrow_capable()
    for relu in (False, True):
        assert KeyedLayer.kernel(W, True, relu, narrow=narrow, narrow64=True)[1] == KeyedLayer.kernel(W, True, relu)[1] == _capi.KN_FLAG_EXACT | (_capi.KN_FLAG_RELU if relu else 0)
    F = _tiny_conv()
    k = KeyedLayer.kernel(ksp.FactoredSparseMatrix(F.tosparse('csr'), F), True, True, narrow=narrow, narrow64=True)
    assert k[1] == _capi.KN_FLAG_EXACT | _capi.KN_FLAG_RELU | _capi.KN_FLAG_NARROW | _capi.KN_FLAG_NARROW32 | _capi.KN_FLAG_NARROW64


def _steady_loop(lines):
    """The innermost loop that issues row loads: (first, last) line of the body of the backward branch closest around two ROW_LOADs -- two steps per trip."""
    labels = {l[:-1]: i for (i, l) in enumerate(lines) if l.endswith(':')}
    best = None
    for (i, l) in enumerate(lines):
        m = re.match(r's_cbranch\w*\s+(\S+)', l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            body = lines[labels[m.group(1)] + 1:i]
            if sum(1 for b in body if ROW_LOAD.match(b)) == 2 and any(b.startswith('v_pk_mul_f32') for b in body) and (best is None or len(body) < len(best)):
                best = body
    return best


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='needs hipcc')
def test_pipe64_kernel_isa(tmp_path):
    s = _isa('kn_conv.hip', tmp_path)
    kernels = _kernel_bodies(s, [PIPE64])
    assert len(kernels) == 4, [k[0] for k in kernels]
    assert sorted(re.match(PIPE64 + r'ILi(\d+)ELb(\d)ELi2ELi1EE', k[0]).groups() for k in kernels) == sorted((r, c) for r in ('8', '16') for c in '01')
    for (name, lines) in kernels:
        (rbx, coef) = re.match(PIPE64 + r'ILi(\d+)ELb(\d)E', name).groups()
        (rbx, coef) = (int(rbx), coef == '1')
        for l in lines:
            if FUSED.match(l):
                assert any(c in l for c in INT_DIVISION_LITERALS), 'fused multiply-add in %s: %s' % (name, l)
        assert not any(l.startswith('scratch_') or (l.startswith('buffer_store') and 'offen' in l) for l in lines), 'spill in %s' % name
        assert not any(l.startswith('ds_') or l.startswith('s_barrier') for l in lines), 'LDS / barrier in %s' % name
        assert not any(l.startswith('v_writelane') for l in lines), 'scalar registers spilled into vector lanes in %s' % name
        assert any(re.match(r's_load_dwordx%d\b' % rbx, l) for l in lines), 'no tap tuple load in %s' % name
        meta = s[s.index('.amdhsa_kernel ' + name):]
        meta = meta[:meta.index('.end_amdhsa_kernel')]
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', meta).group(1)) == 0, name
        assert int(re.search(r'\.amdhsa_next_free_vgpr\s+(\d+)', meta).group(1)) <= 128, name
        assert int(re.search(r'\.amdhsa_group_segment_fixed_size\s+(\d+)', meta).group(1)) == 0, name
        # the steady state: two steps per trip, each RBX / 2 packed multiplies (coefficients: as many again for the stored values fl(coef * tap)) and RBX / 2 packed adds,
        # the activation's low half broadcast by op_sel_hi, no register copy, no single-lane multiply or add
        body = _steady_loop(lines)
        assert body is not None, name
        muls = [l for l in body if l.startswith('v_pk_mul_f32')]
        adds = [l for l in body if l.startswith('v_pk_add_f32')]
        assert len(muls) == 2 * (rbx if coef else rbx // 2), (name, len(muls))
        assert len(adds) == 2 * (rbx // 2), (name, len(adds))
        assert sum(1 for l in muls if 'op_sel_hi:[0,1]' in l) == 2 * (rbx // 2), name
        assert not any(re.match(r'v_(mul|add)_', l) for l in body), [l for l in body if re.match(r'v_(mul|add)_', l)]
        movs = [l for l in body if l.startswith('v_mov')]              # the activation is never copied; with coefficients the step's coefficient goes from its SGPR into a VGPR pair
        assert len(movs) == (2 if coef else 0) and all(re.match(r'v_mov_b64_e32 v\[\d+:\d+\], s\[', l) for l in movs), (name, movs)
        assert sum(1 for l in body if re.match(r's_load_dwordx%d\b' % rbx, l)) == 2, name
        # load ownership, on the loop body walked twice (the state at its head is the state at its end): a row register is touched by nothing between its load and the
        # counted wait that retires it (loads return in order)
        fly = []
        for l in body + body:
            m = ROW_LOAD.match(l)
            if m:
                fly.append(int(m.group(1)[1:]))
                continue
            m = re.match(r's_waitcnt .*vmcnt\((\d+)\)', l)
            if m:
                fly = fly[len(fly) - int(m.group(1)):] if int(m.group(1)) else []
                continue
            assert not (_regs(l, 'v') & set(fly)), (name, l, fly)
        assert len(fly) <= 1, name
        # ... and around the loop, in program order from the first asm-issued row load (the last dword load ahead of the first packed multiply) to the first store: the
        # tail's waits stand in straight-line code (a wait inside a branch once made the compiler copy the row register ahead of it: stale activations)
        first_mul = next(i for (i, l) in enumerate(lines) if l.startswith('v_pk_mul_f32'))
        start = max(i for (i, l) in enumerate(lines[:first_mul]) if ROW_LOAD.match(l))
        fly = []
        for l in lines[start:]:
            if l.startswith('global_store'):
                break
            m = ROW_LOAD.match(l)
            if m:
                fly.append(int(m.group(1)[1:]))
                continue
            m = re.match(r's_waitcnt .*vmcnt\((\d+)\)', l)
            if m:
                fly = fly[len(fly) - int(m.group(1)):] if int(m.group(1)) else []
                continue
            assert not (l.startswith('v_') and _regs(l, 'v') & set(fly)), (name, l, fly)
    entries = list(re.finditer(r'\.name:\s+(%s\S*)' % PIPE64, s))
    assert len(entries) == 4
    for m in entries:
        k = re.compile(r'\.private_segment_fixed_size:\s+(\d+)').search(s, m.end())
        assert k and int(k.group(1)) == 0, m.group(1)
