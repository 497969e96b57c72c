"""Host-side checks of the low-latency (narrow) forward: the KN_FLAG_NARROW flag in the C ABI and its binding, the gfx950 ISA of
convtaps_narrow_kernel (separate multiplies and adds, nothing spilled), and the `narrow` keyword down to KeyedLayer.kernel."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARROW = r'_ZN2kn22convtaps_narrow_kernel'


def test_header_declares_the_flag_and_the_binding_mirrors_it():
    h = open(os.path.join(ROOT, 'include', 'keynet_hip.h')).read()
    m = re.search(r'#define\s+KN_FLAG_NARROW\s+(\d+)u', h)
    assert m and int(m.group(1)) == 8
    assert _capi.KN_FLAG_NARROW == 8
    flags = [_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_BF16X3, _capi.KN_FLAG_NARROW]
    assert sorted(flags) == [1, 2, 4, 8]                              # one bit each
    v = re.search(r'#define\s+KN_ABI_VERSION\s+(\d+)', h)
    assert v and int(v.group(1)) == 5 and _capi.KN_ABI_VERSION == 5   # the flag changed what kn_spmm accepts: a stale library is rebuilt
    assert ksys.KeyedModel.NARROW_MAX == 8 and ksp.NARROW_MAX == 8


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='needs hipcc')
def test_narrow_kernel_isa_rounds_products_and_sums_separately_and_spills_nothing(tmp_path):
    s = _isa('kn_conv.hip', tmp_path)
    kernels = _kernel_bodies(s, [NARROW])
    # 1 | 2 columns always fill their form; 4 | 8 exist full and masked; each with / without summed stored values and coefficients
    assert len(kernels) == 24, [k[0] for k in kernels]
    for (name, lines) in kernels:
        for l in lines:
            if FUSED.match(l):
                assert any(c in l for c in INT_DIVISION_LITERALS), 'fused multiply-add in %s: %s' % (name, l)
        assert any(re.match(r'v_(pk_)?mul_f32', l) for l in lines), name
        assert any(re.match(r'v_(pk_)?add_f32', l) for l in lines), name
        assert not any(l.startswith('scratch_') or (l.startswith('buffer_store') and 'offen' in l) for l in lines), 'spill in %s' % name
        assert not any(l.startswith('ds_') or l.startswith('s_barrier') for l in lines), 'LDS / barrier in %s' % name
        meta = s[s.index('.amdhsa_kernel ' + name):]
        meta = meta[:meta.index('.end_amdhsa_kernel')]
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', meta).group(1)) == 0, name
    entries = list(re.finditer(r'\.name:\s+(%s\S*)' % NARROW, s))      # ... and in the code object's metadata (a kernel's keys are sorted: .name precedes it)
    assert len(entries) == 24
    for m in entries:
        k = re.compile(r'\.private_segment_fixed_size:\s+(\d+)').search(s, m.end())
        assert k and int(k.group(1)) == 0, m.group(1)


def _tiny_conv():
    rng = np.random.RandomState(0)
    (Cin, Cout, H) = (2, 3, 4)
    taps = rng.randn(2, Cout, Cin).astype(np.float32)
    eo = np.repeat(np.arange(H * H, dtype=np.int32), 2)
    ei = (eo + np.tile([0, 1], H * H)).astype(np.int32) % (H * H)
    et = np.tile(np.arange(2, dtype=np.int32), H * H)
    ec = (rng.rand(len(eo)) + 0.5).astype(np.float32)
    lastcol = np.concatenate((rng.randn(Cout * H * H), [1.0])).astype(np.float32)
    return ksp.Conv2dTiledMatrix.fromtaps((Cin, H, H), (Cout, H, H), taps, eo, ei, et, ec, lastcol)


def test_the_keyword_reaches_every_layer_of_the_python_host():
    for f in (ksys.KeyedModel.forward_linear, ksys.KeyedModel.forward, ksys.KeyedModel.capture, KeyedLayer.forward, KeyedLayer.kernel, KeyedLayer.launch,
              ksp.Conv2dTiledMatrix.torchdot, ksp.FactoredSparseMatrix.torchdot):
        p = inspect.signature(f).parameters
        assert 'narrow' in p and p['narrow'].default is False, f


@pytest.mark.parametrize('contract', [True, False, 'auto', 'split', 'bf16x3'])
def test_kernel_sets_the_flag_on_a_conv_operator_under_every_contract(contract):
    W = _tiny_conv()
    today = KeyedLayer.kernel(W, contract, False)
    if contract in ('auto', 'split'):
        assert today is None                                          # not one launch without the keyword: calibrates / two steps
    else:
        assert not (today[1] & _capi.KN_FLAG_NARROW)                  # without the keyword the flags are what they were
    for relu in (False, True):
        k = KeyedLayer.kernel(W, contract, relu, narrow=True)
        assert k is not None
        (get_op, flags) = k
        assert get_op == W._device_op
        assert flags & _capi.KN_FLAG_NARROW
        assert bool(flags & _capi.KN_FLAG_RELU) == relu
        assert bool(flags & _capi.KN_FLAG_EXACT) == (contract is True)
        if today is not None:
            assert flags == (KeyedLayer.kernel(W, contract, relu)[1] | _capi.KN_FLAG_NARROW)


def test_operators_without_a_narrow_form_keep_their_flags():
    M = scipy.sparse.random(12, 9, density=0.4, format='csr', dtype=np.float32, random_state=1)
    W = ksp.SparseMatrix(M)
    assert not W.narrow_capable()
    assert KeyedLayer.kernel(W, True, False, narrow=True)[1] == KeyedLayer.kernel(W, True, False)[1] == _capi.KN_FLAG_EXACT
    assert _tiny_conv().narrow_capable()
    F = _tiny_conv()
    C = F.tosparse('csr')
    assert ksp.FactoredSparseMatrix(C, F).narrow_capable()
    k = KeyedLayer.kernel(ksp.FactoredSparseMatrix(C, F), True, True, narrow=True)
    assert k[1] == _capi.KN_FLAG_EXACT | _capi.KN_FLAG_RELU | _capi.KN_FLAG_NARROW
