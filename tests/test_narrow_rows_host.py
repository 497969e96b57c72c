"""Host-side checks of the row-lane narrow forward: the KN_FLAG_NARROW_ROWS flag in the C ABI and its binding, the narrow_rows keyword down to
KeyedLayer.kernel, and the gfx950 ISA of csr_narrow_kernel (separate multiplies and adds, nothing spilled)."""
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
from keynet_amd.build import SOURCES
from keynet_amd.layer import CONTRACTS, KeyedLayer, _contract
from test_isa_lint import FUSED, INT_DIVISION_LITERALS, _isa, _kernel_bodies
from test_narrow_host import _tiny_conv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = r'_ZN2kn17csr_narrow_kernel'
(RELU, EXACT, NARROW, ROWS) = (_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_NARROW, _capi.KN_FLAG_NARROW_ROWS)


def test_header_declares_and_documents_the_flag_and_the_binding_mirrors_it():
    h = open(os.path.join(ROOT, 'include', 'keynet_hip.h')).read()
    m = re.search(r'#define\s+KN_FLAG_NARROW_ROWS\s+(\d+)u\s*/\*(.*?)\*/', h, re.S)
    assert m and int(m.group(1)) == 32 and _capi.KN_FLAG_NARROW_ROWS == 32
    doc = m.group(2)
    for word in ('csr_narrow_kernel', 'bit for bit', 'IGNORED', 'kn_spmm_planes', 'kn_spmm_screen', 'kn_spmm_plan', '2^30'):
        assert word in doc, word
    spmm_doc = h[h.index('What a caller may pass'):h.index('int kn_spmm(')]
    assert 'KN_FLAG_NARROW_ROWS' in spmm_doc and 'cols * ldx + 8 < 2^30' in spmm_doc          # the guard, in the table of kn_spmm
    flags = [_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_BF16X3, _capi.KN_FLAG_NARROW, _capi.KN_FLAG_NARROW_MFMA, _capi.KN_FLAG_NARROW_ROWS]
    assert sorted(flags) == [1, 2, 4, 8, 16, 32]                          # one bit each
    v = re.search(r'#define\s+KN_ABI_VERSION\s+(\d+)', h)
    assert v and int(v.group(1)) == 5 and _capi.KN_ABI_VERSION == 5       # no entry point was added
    assert 'kn_csr_narrow.hip' in SOURCES


def test_the_keyword_reaches_every_layer_of_the_python_host():
    for f in (ksys.KeyedModel.forward_linear, ksys.KeyedModel.forward, ksys.KeyedModel.capture, KeyedLayer.forward, KeyedLayer.kernel, KeyedLayer.launch,
              ksp._run_torchdot, ksp.SparseMatrix.torchdot, ksp.TiledMatrix.torchdot, ksp.DiagonalTiledMatrix.torchdot):
        p = inspect.signature(f).parameters
        assert 'narrow_rows' in p and p['narrow_rows'].default is False, f
        assert 'narrow_rows' in (f.__doc__ or ''), f
    for cls in (ksp.SparseMatrix, ksp.TiledMatrix, ksp.DiagonalTiledMatrix, ksp.FactoredSparseMatrix, ksp.Conv2dTiledMatrix):
        assert callable(cls.rows_capable)


def _csr_operator(dtype=np.float32):
    return ksp.SparseMatrix(scipy.sparse.random(12, 9, density=0.4, format='csr', dtype=dtype, random_state=1))


def test_kernel_sets_the_flag_on_stored_order_csr_operators_only(monkeypatch):
    W = _csr_operator()
    assert W.rows_capable() and not W.narrow_capable()                    # (narrow_capable() is about conv-taps handles: untouched)
    for relu in (False, True):
        base = EXACT | (RELU if relu else 0)
        assert KeyedLayer.kernel(W, True, relu, narrow=True) == (W._device_op, base)                       # only with the keyword
        assert KeyedLayer.kernel(W, True, relu) == (W._device_op, base)
        assert KeyedLayer.kernel(W, True, relu, narrow=True, narrow_rows=True) == (W._device_op, base | ROWS)
        assert KeyedLayer.kernel(W, True, relu, narrow='mfma', narrow_rows=True) == (W._device_op, base | ROWS)
    # a small operator off the exact contract has no dense handle: still its CSR handle in the stored order
    monkeypatch.setattr(W, '_dense_device_op', lambda device=None: None, raising=False)
    assert KeyedLayer.kernel(W, False, False, narrow=True, narrow_rows=True) == (W._device_op, EXACT | ROWS)
    # ... and a plain SparseMatrix that the re-ordering contract put on its dense handle keeps what it has
    dense = (lambda device=None: 'a dense handle')
    monkeypatch.setattr(W, '_dense_device_op', dense, raising=False)
    assert KeyedLayer.kernel(W, False, True, narrow=True, narrow_rows=True) == (dense, RELU)
    assert KeyedLayer.kernel(W, True, True, narrow=True, narrow_rows=True) == (W._device_op, EXACT | RELU | ROWS)       # (under True the dense handle is not in play)
    # a float64 operator
    W64 = _csr_operator(np.float64)
    assert W64.is_float64() and not W64.rows_capable()
    assert KeyedLayer.kernel(W64, True, False, narrow=True, narrow_rows=True)[1] == EXACT
    # conv operators: what `narrow` alone makes them
    F = _tiny_conv()
    for contract in (True, False, 'bf16x3'):
        for mode in (True, 'mfma'):
            assert KeyedLayer.kernel(F, contract, True, narrow=mode, narrow_rows=True) == KeyedLayer.kernel(F, contract, True, narrow=mode)
    Wf = ksp.FactoredSparseMatrix(F.tosparse('csr'), F)
    assert not Wf.rows_capable() and not F.rows_capable()
    assert KeyedLayer.kernel(Wf, True, True, narrow=True, narrow_rows=True)[1] == EXACT | RELU | NARROW
    # a tiled container is expanded to CSR once
    T = ksp.TiledMatrix(scipy.sparse.random(12, 12, density=0.3, format='csr', dtype=np.float32, random_state=2), (4, 4))
    assert T.rows_capable() and KeyedLayer.kernel(T, True, False, narrow=True, narrow_rows=True) == (T._device_op, EXACT | ROWS)


def test_layers_plan_the_flag_only_inside_a_narrow_forward():
    c = KeyedLayer.fromoperator(_csr_operator(), 'Linear', exact=True)
    c.W._device_op = lambda device=None: 'handle'
    assert c.launch(None, narrow=True, narrow_rows=True).flags == EXACT | ROWS
    assert c.launch(None, narrow=True).flags == c.launch(None).flags == c.launch(None, narrow_rows=True).flags == EXACT


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='needs hipcc')
def test_kernel_isa_has_no_fused_multiply_add_and_no_scratch(tmp_path):
    s = _isa('kn_csr_narrow.hip', tmp_path)
    kernels = _kernel_bodies(s, [KERNEL])
    assert len(kernels) == 6, [k[0] for k in kernels]                     # NV 1 | 2 | 4 | 8, and 4 and 8 also masked
    for (name, lines) in kernels:
        for l in lines:
            if FUSED.match(l):
                assert any(c in l for c in INT_DIVISION_LITERALS), 'fused multiply-add in %s: %s' % (name, l)
        assert any(re.match(r'v_(pk_)?mul_f32', l) for l in lines) and any(re.match(r'v_(pk_)?add_f32', l) for l in lines), name
        assert not any(l.startswith('scratch_') or (l.startswith('buffer_store') and 'offen' in l) for l in lines), 'spill in %s' % name
        assert not any('atomic' in l or l.startswith('ds_') for l in lines), 'an atomic or LDS access in %s' % name
        meta = s[s.index('.amdhsa_kernel ' + name):]
        meta = meta[:meta.index('.end_amdhsa_kernel')]
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', meta).group(1)) == 0, name
    entries = list(re.finditer(r'\.name:\s+(%s\S*)' % KERNEL, s))
    assert len(entries) == 6
    for m in entries:
        k = re.compile(r'\.private_segment_fixed_size:\s+(\d+)').search(s, m.end())
        assert k and int(k.group(1)) == 0, m.group(1)


(BF16X3, MFMA) = (_capi.KN_FLAG_BF16X3, _capi.KN_FLAG_NARROW_MFMA)
# (contract, narrow, narrow_rows) -> the flag word without / with a fused ReLU; None = not one launch
KERNEL_FLAGS_CONV = {
    ('exact', False, False): (EXACT, RELU + EXACT),
    ('exact', False, True): (EXACT, RELU + EXACT),
    ('exact', True, False): (EXACT + NARROW, RELU + EXACT + NARROW),
    ('exact', True, True): (EXACT + NARROW, RELU + EXACT + NARROW),
    ('exact', 'mfma', False): (EXACT + NARROW, RELU + EXACT + NARROW),
    ('exact', 'mfma', True): (EXACT + NARROW, RELU + EXACT + NARROW),
    ('mfma', False, False): (0, RELU),
    ('mfma', False, True): (0, RELU),
    ('mfma', True, False): (NARROW, RELU + NARROW),
    ('mfma', True, True): (NARROW, RELU + NARROW),
    ('mfma', 'mfma', False): (MFMA, RELU + MFMA),
    ('mfma', 'mfma', True): (MFMA, RELU + MFMA),
    ('auto', False, False): (None, None),
    ('auto', False, True): (None, None),
    ('auto', True, False): (NARROW, RELU + NARROW),
    ('auto', True, True): (NARROW, RELU + NARROW),
    ('auto', 'mfma', False): (NARROW, RELU + NARROW),
    ('auto', 'mfma', True): (NARROW, RELU + NARROW),
    ('bf16x3', False, False): (BF16X3, RELU + BF16X3),
    ('bf16x3', False, True): (BF16X3, RELU + BF16X3),
    ('bf16x3', True, False): (BF16X3 + NARROW, RELU + BF16X3 + NARROW),
    ('bf16x3', True, True): (BF16X3 + NARROW, RELU + BF16X3 + NARROW),
    ('bf16x3', 'mfma', False): (MFMA, RELU + MFMA),
    ('bf16x3', 'mfma', True): (MFMA, RELU + MFMA),
    ('split', False, False): (None, None),
    ('split', False, True): (None, None),
    ('split', True, False): (NARROW, RELU + NARROW),
    ('split', True, True): (NARROW, RELU + NARROW),
    ('split', 'mfma', False): (MFMA, RELU + MFMA),
    ('split', 'mfma', True): (MFMA, RELU + MFMA),
}
KERNEL_FLAGS_CSR = {
    ('exact', False, False): (EXACT, RELU + EXACT),
    ('exact', False, True): (EXACT + ROWS, RELU + EXACT + ROWS),
    ('exact', True, False): (EXACT, RELU + EXACT),
    ('exact', True, True): (EXACT + ROWS, RELU + EXACT + ROWS),
    ('exact', 'mfma', False): (EXACT, RELU + EXACT),
    ('exact', 'mfma', True): (EXACT + ROWS, RELU + EXACT + ROWS),
    ('mfma', False, False): (EXACT, RELU + EXACT),
    ('mfma', False, True): (EXACT + ROWS, RELU + EXACT + ROWS),
    ('mfma', True, False): (EXACT, RELU + EXACT),
    ('mfma', True, True): (EXACT + ROWS, RELU + EXACT + ROWS),
    ('mfma', 'mfma', False): (EXACT, RELU + EXACT),
    ('mfma', 'mfma', True): (EXACT + ROWS, RELU + EXACT + ROWS),
    ('auto', False, False): (None, None),
    ('auto', False, True): (None, None),
    ('auto', True, False): (None, None),
    ('auto', True, True): (None, None),
    ('auto', 'mfma', False): (None, None),
    ('auto', 'mfma', True): (None, None),
    ('bf16x3', False, False): (EXACT, RELU + EXACT),
    ('bf16x3', False, True): (EXACT + ROWS, RELU + EXACT + ROWS),
    ('bf16x3', True, False): (EXACT, RELU + EXACT),
    ('bf16x3', True, True): (EXACT + ROWS, RELU + EXACT + ROWS),
    ('bf16x3', 'mfma', False): (EXACT, RELU + EXACT),
    ('bf16x3', 'mfma', True): (EXACT + ROWS, RELU + EXACT + ROWS),
    ('split', False, False): (EXACT, RELU + EXACT),
    ('split', False, True): (EXACT + ROWS, RELU + EXACT + ROWS),
    ('split', True, False): (EXACT, RELU + EXACT),
    ('split', True, True): (EXACT + ROWS, RELU + EXACT + ROWS),
    ('split', 'mfma', False): (EXACT, RELU + EXACT),
    ('split', 'mfma', True): (EXACT + ROWS, RELU + EXACT + ROWS),
}


def test_kernel_flag_word_for_every_contract_and_narrow_form(monkeypatch):
    """KeyedLayer.kernel() on the tiny conv-taps operator and on a 12 x 9 CSR operator, for every contract x narrow x narrow_rows x relu, against the two
    tables above.  The tables were filled from kernel() as it stood BEFORE its flag word was assembled in one place (two early narrow returns and the
    original rule): they pin that rule, the odd rows included -- a narrow conv launch keeps the contract's EXACT / BF16X3 next to NARROW, an 'mfma' launch
    carries no contract flag, 'auto' and two-step 'split' are one launch when narrow, and kernel() itself sets NARROW_ROWS without `narrow` (launch() and
    forward() are what tie it to a narrow forward).  Every launch is on the operator's own handle."""
    conv = _tiny_conv()
    csr = _csr_operator()
    monkeypatch.setattr(csr, '_dense_device_op', lambda device=None: None, raising=False)      # (12 x 9: no dense handle; asking for one needs a device)
    seen = 0
    for (W, table) in ((conv, KERNEL_FLAGS_CONV), (csr, KERNEL_FLAGS_CSR)):
        assert sorted(table, key=str) == sorted(((c, n, r) for c in CONTRACTS for n in (False, True, 'mfma') for r in (False, True)), key=str)
        for ((name, narrow, rows), words) in table.items():
            for (relu, want) in zip((False, True), words):
                got = KeyedLayer.kernel(W, _contract(name, True), relu, None, narrow=narrow, narrow_rows=rows)
                assert got == (None if want is None else (W._device_op, want)), (name, narrow, rows, relu, got)
                seen += 1
    assert seen == 2 * len(CONTRACTS) * 3 * 2 * 2
    # ... and with a dense handle in play (a large keyed nn.Linear): the re-ordering contracts take it, with (0, RELU) and never NARROW_ROWS, whatever the keywords;
    # 'exact' and 'auto' are the rows of KERNEL_FLAGS_CSR
    dense = (lambda device=None: 'a dense handle')
    monkeypatch.setattr(csr, '_dense_device_op', dense, raising=False)
    for ((name, narrow, rows), words) in KERNEL_FLAGS_CSR.items():
        for (relu, want) in zip((False, True), words):
            got = KeyedLayer.kernel(csr, _contract(name, True), relu, None, narrow=narrow, narrow_rows=rows)
            if name in ('mfma', 'bf16x3', 'split'):
                assert got == (dense, RELU if relu else 0), (name, narrow, rows, relu, got)
            else:
                assert got == (None if want is None else (csr._device_op, want)), (name, narrow, rows, relu, got)
