"""Host-side checks of the matrix-core narrow forward: the KN_FLAG_NARROW_MFMA flag in the C ABI and its binding, the gfx950 ISA of
convtaps_narrow_mfma_kernel (an f32 matrix instruction, nothing spilled), and narrow='mfma' down to KeyedLayer.kernel."""
import inspect
import os
import re
import shutil

import pytest

from keynet_amd import _capi
from keynet_amd import sparse as ksp
from keynet_amd import system as ksys
from keynet_amd.layer import CONTRACTS, KeyedLayer, _contract
from test_isa_lint import _isa, _kernel_bodies
from test_narrow_host import _tiny_conv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = r'_ZN2kn27convtaps_narrow_mfma_kernel'


def test_header_declares_the_flag_and_the_binding_mirrors_it():
    h = open(os.path.join(ROOT, 'include', 'keynet_hip.h')).read()
    m = re.search(r'#define\s+KN_FLAG_NARROW_MFMA\s+(\d+)u', h)
    assert m and int(m.group(1)) == 16
    assert _capi.KN_FLAG_NARROW_MFMA == 16
    flags = [_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_BF16X3, _capi.KN_FLAG_NARROW, _capi.KN_FLAG_NARROW_MFMA]
    assert sorted(flags) == [1, 2, 4, 8, 16]                          # one bit each
    v = re.search(r'#define\s+KN_ABI_VERSION\s+(\d+)', h)
    assert v and int(v.group(1)) == 5 and _capi.KN_ABI_VERSION == 5   # no entry point was added; a stale library is rebuilt on the source change


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='needs hipcc')
def test_kernel_isa_has_an_f32_matrix_instruction_and_spills_nothing(tmp_path):
    s = _isa('kn_conv.hip', tmp_path)
    kernels = _kernel_bodies(s, [KERNEL])
    assert len(kernels) == 8, [k[0] for k in kernels]                 # 32 | 64 channels x one | two slots per (pixel, tap) x unit | float coefficients
    for (name, lines) in kernels:
        assert any(l.startswith('v_mfma_f32_32x32x2_f32') for l in lines), name
        assert not any(l.startswith('scratch_') or (l.startswith('buffer_store') and 'offen' in l) for l in lines), 'spill in %s' % name
        assert not any('atomic' in l for l in lines), 'an atomic in %s' % name
        meta = s[s.index('.amdhsa_kernel ' + name):]
        meta = meta[:meta.index('.end_amdhsa_kernel')]
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', meta).group(1)) == 0, name
    entries = list(re.finditer(r'\.name:\s+(%s\S*)' % KERNEL, s))
    assert len(entries) == 8
    for m in entries:
        k = re.compile(r'\.private_segment_fixed_size:\s+(\d+)').search(s, m.end())
        assert k and int(k.group(1)) == 0, m.group(1)


def test_the_keyword_reaches_every_layer_of_the_python_host():
    """narrow='mfma' is a second value of the existing keyword (default False everywhere), documented where it is accepted."""
    for f in (ksys.KeyedModel.forward_linear, ksys.KeyedModel.forward, ksys.KeyedModel.capture, KeyedLayer.forward, KeyedLayer.kernel, KeyedLayer.launch,
              ksp.Conv2dTiledMatrix.torchdot, ksp.FactoredSparseMatrix.torchdot):
        p = inspect.signature(f).parameters
        assert 'narrow' in p and p['narrow'].default is False, f
        assert "'mfma'" in (f.__doc__ or ''), f
    for f in (KeyedLayer.narrow_mode, KeyedLayer.narrow_record, KeyedLayer.narrow_screened):
        assert callable(f)


@pytest.mark.parametrize('name', CONTRACTS)
def test_kernel_sets_the_flag_only_under_a_reordering_contract(name):
    contract = _contract(name, True)
    W = _tiny_conv()
    reorder = contract in (False, 'bf16x3', 'split')
    for relu in (False, True):
        (get_op, flags) = KeyedLayer.kernel(W, contract, relu, narrow='mfma')
        assert get_op == W._device_op
        assert bool(flags & _capi.KN_FLAG_RELU) == relu
        if reorder:
            assert flags == (_capi.KN_FLAG_NARROW_MFMA | (_capi.KN_FLAG_RELU if relu else 0))
        else:
            assert flags == KeyedLayer.kernel(W, contract, relu, narrow=True)[1]
            assert flags & _capi.KN_FLAG_NARROW and not (flags & _capi.KN_FLAG_NARROW_MFMA)
        assert not (KeyedLayer.kernel(W, contract, relu, narrow=True)[1] & _capi.KN_FLAG_NARROW_MFMA)     # narrow=True keeps its flags


def test_other_operators_and_layers_keep_the_channel_lane_flag():
    F = _tiny_conv()
    Wf = ksp.FactoredSparseMatrix(F.tosparse('csr'), F)                # a conv-taps handle behind an operator under the bit-exact contract
    for contract in (True, False):
        assert KeyedLayer.kernel(Wf, contract, False, narrow='mfma') == KeyedLayer.kernel(Wf, contract, False, narrow=True)
    for (contract, mode) in ((True, True), ('auto', True), (False, 'mfma'), ('bf16x3', 'mfma')):
        c = KeyedLayer.fromoperator(_tiny_conv(), 'Conv2d', exact=contract)
        assert c.narrow_mode('mfma') == mode and c.narrow_mode(True) is True and c.narrow_record() is None and not c.narrow_screened()
    # a layer on the matrix cores by a calibration decision: a planner (no batch) gets the channel-lane kernel until a forward has measured; then the record decides
    c = KeyedLayer.fromoperator(_tiny_conv(), 'Conv2d', exact=False)
    c._contract_record = dict(decided='mfma', max_abs_x=1.0)
    assert c.screened() and c.narrow_mode('mfma') is True
    c._contract_record['narrow'] = dict(decided='mfma', gate_ratio=0.1, max_abs_x=2.0, measured_on_columns=4)
    assert c.narrow_mode('mfma') == 'mfma' and c.narrow_screened()
    assert not c.rescreen(3.9, narrow=True) and c.rescreen(4.1, narrow=True) and c.rescreen(2.1) and not c.rescreen(1.9)
    c._contract_record['narrow'] = dict(decided='exact', gate_ratio=0.9, max_abs_x=2.0, measured_on_columns=4)
    assert c.narrow_mode('mfma') is True and not c.narrow_screened()
