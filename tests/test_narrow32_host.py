"""Host-side checks of the low-latency forward for 9 .. 32 images: the KN_FLAG_NARROW32 modifier in the C ABI and its binding, the `narrow32` keyword down to
KeyedLayer.kernel and its argument rules, and the gfx950 ISA of convtaps_narrow32_kernel (separate multiplies and adds, nothing spilled -- neither to scratch
nor into vector lanes --, no LDS, at most 128 vector registers)."""
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
NARROW32 = r'_ZN2kn24convtaps_narrow32_kernel'


def test_header_declares_the_modifier_and_the_binding_mirrors_it():
    h = open(os.path.join(ROOT, 'include', 'keynet_hip.h')).read()
    m = re.search(r'#define\s+KN_FLAG_NARROW32\s+(\d+)u', h)
    assert m and int(m.group(1)) == 64
    assert _capi.KN_FLAG_NARROW32 == 64
    flags = [_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_BF16X3, _capi.KN_FLAG_NARROW, _capi.KN_FLAG_NARROW_MFMA, _capi.KN_FLAG_NARROW_ROWS, _capi.KN_FLAG_NARROW32]
    assert sorted(flags) == [1, 2, 4, 8, 16, 32, 64]                  # one bit each
    assert sorted(int(v) for v in re.findall(r'#define\s+KN_FLAG_\w+\s+(\d+)u', h)) == [1, 2, 4, 8, 16, 32, 64]
    v = re.search(r'#define\s+KN_ABI_VERSION\s+(\d+)', h)
    assert v and int(v.group(1)) == 5 and _capi.KN_ABI_VERSION == 5   # a modifier of kn_spmm's flags: no entry point added
    assert ksys.KeyedModel.NARROW32_MAX == 32 and ksp.NARROW32_MAX == 32
    assert ksys.KeyedModel.NARROW_MAX == 8 and ksp.NARROW_MAX == 8


def test_the_keyword_reaches_every_layer_of_the_python_host():
    for f in (ksys.KeyedModel.forward_linear, ksys.KeyedModel.forward, ksys.KeyedModel.capture, KeyedLayer.forward, KeyedLayer.kernel, KeyedLayer.launch,
              ksp.Conv2dTiledMatrix.torchdot, ksp.FactoredSparseMatrix.torchdot, ksp._run_torchdot, ksp._narrow_args):
        p = inspect.signature(f).parameters
        assert 'narrow32' in p and p['narrow32'].default is False, f


def test_the_argument_rules():
    for narrow in (True, 'mfma'):
        for n in (1, 8, 9, 32):
            assert ksp._narrow_args(n, narrow, False, narrow32=True) == (narrow, False)
        with pytest.raises(ValueError):
            ksp._narrow_args(33, narrow, False, narrow32=True)
        with pytest.raises(ValueError):
            ksp._narrow_args(9, narrow, False)                        # without the keyword the limit is where it was
        with pytest.raises(ValueError):
            ksp._narrow_args(9, narrow, True, narrow32=True)          # the row-lane kernel is an 8-column kernel
        assert ksp._narrow_args(8, narrow, True, narrow32=True) == (narrow, True)
    for alone in (False, True):
        with pytest.raises(ValueError):
            ksp._narrow_args(4, False, False, alone=alone, narrow32=True)       # only together with `narrow`
        with pytest.raises(ValueError):
            ksp._narrow_args(16, False, False, alone=alone, narrow32=True)


@pytest.mark.parametrize('narrow', [True, 'mfma'])
@pytest.mark.parametrize('contract', [True, False, 'auto', 'split', 'bf16x3'])
def test_kernel_adds_the_modifier_on_a_conv_operator_under_every_contract(contract, narrow):
    W = _tiny_conv()
    for relu in (False, True):
        (get_op, flags) = KeyedLayer.kernel(W, contract, relu, narrow=narrow, narrow32=True)
        (get_op0, flags0) = KeyedLayer.kernel(W, contract, relu, narrow=narrow)
        assert get_op == get_op0 == W._device_op
        assert not (flags0 & _capi.KN_FLAG_NARROW32)
        assert flags == flags0 | _capi.KN_FLAG_NARROW32
    assert KeyedLayer.kernel(W, contract, False, narrow32=True) == KeyedLayer.kernel(W, contract, False)      # without `narrow`: nothing


@pytest.mark.parametrize('narrow', [True, 'mfma'])
def test_operators_without_a_narrow_form_keep_their_flags(narrow):
    M = scipy.sparse.random(12, 9, density=0.4, format='csr', dtype=np.float32, random_state=1)
    W = ksp.SparseMatrix(M)
    assert not W.narrow_capable()
    for relu in (False, True):
        assert KeyedLayer.kernel(W, True, relu, narrow=narrow, narrow32=True)[1] == KeyedLayer.kernel(W, True, relu)[1] == _capi.KN_FLAG_EXACT | (_capi.KN_FLAG_RELU if relu else 0)
    F = _tiny_conv()
    k = KeyedLayer.kernel(ksp.FactoredSparseMatrix(F.tosparse('csr'), F), True, True, narrow=narrow, narrow32=True)
    assert k[1] == _capi.KN_FLAG_EXACT | _capi.KN_FLAG_RELU | _capi.KN_FLAG_NARROW | _capi.KN_FLAG_NARROW32


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='needs hipcc')
def test_narrow32_kernel_isa(tmp_path):
    s = _isa('kn_conv.hip', tmp_path)
    kernels = _kernel_bodies(s, [NARROW32])
    # 8 | 16 columns per block with / without summed stored values and coefficients, 32 columns without summed stored values; a block the batch does not fill
    # is the same instantiation
    assert len(kernels) == 10, [k[0] for k in kernels]
    assert sorted(re.match(NARROW32 + r'ILi(\d+)ELb(\d)ELb(\d)E', k[0]).groups() for k in kernels) == sorted(
        [(nv, d, c) for nv in ('8', '16') for d in '01' for c in '01'] + [('32', '0', c) for c in '01'])
    for (name, lines) in kernels:
        for l in lines:
            if FUSED.match(l):
                assert any(c in l for c in INT_DIVISION_LITERALS), 'fused multiply-add in %s: %s' % (name, l)
        assert any(re.match(r'v_(pk_)?mul_f32', l) for l in lines), name
        assert any(re.match(r'v_(pk_)?add_f32', l) for l in lines), name
        assert not any(l.startswith('scratch_') or (l.startswith('buffer_store') and 'offen' in l) for l in lines), 'spill in %s' % name
        assert not any(l.startswith('ds_') or l.startswith('s_barrier') for l in lines), 'LDS / barrier in %s' % name
        assert not any(l.startswith('v_writelane') for l in lines), 'scalar registers spilled into vector lanes in %s' % name
        # a step's activations arrive as whole segments: NV = 8 one s_load_dwordx8, NV = 16 one s_load_dwordx16, NV = 32 two of them -- and never column by column:
        # the lone s_load_dword left are pointers, sizes and slot records: 9 .. 27 per kernel, where one load per column made 70 .. 91 per batch at NV = 16 | 32
        nv = int(re.match(NARROW32 + r'ILi(\d+)E', name).group(1))
        assert any(re.match(r's_load_dwordx%d\b' % min(nv, 16), l) for l in lines), 'no activation segment load in %s' % name
        if nv == 32:
            assert sum(1 for l in lines if re.match(r's_load_dwordx16\b', l)) >= 2, name
        assert sum(1 for l in lines if re.match(r's_load_dword\s', l)) < 32, 'activations loaded column by column in %s' % name
        meta = s[s.index('.amdhsa_kernel ' + name):]
        meta = meta[:meta.index('.end_amdhsa_kernel')]
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', meta).group(1)) == 0, name
        assert int(re.search(r'\.amdhsa_next_free_vgpr\s+(\d+)', meta).group(1)) <= 128, name
        assert int(re.search(r'\.amdhsa_group_segment_fixed_size\s+(\d+)', meta).group(1)) == 0, name
    entries = list(re.finditer(r'\.name:\s+(%s\S*)' % NARROW32, s))
    assert len(entries) == 10
    for m in entries:
        k = re.compile(r'\.private_segment_fixed_size:\s+(\d+)').search(s, m.end())
        assert k and int(k.group(1)) == 0, m.group(1)
