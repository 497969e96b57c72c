"""Host-side checks of the LDS value-stream form of a keyed Linear: the KN_FLAG_NARROW_LINEAR flag in the C ABI and its binding, the narrow_linear keyword down to
KeyedLayer.kernel, and the gfx950 ISA of csr_stream_group_kernel (separate multiplies and adds, nothing spilled to scratch, the LDS and registers DESIGN states, counted
waits, and no register owned by a load the compiler cannot see)."""
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
from test_narrow_rows_host import KERNEL_FLAGS_CONV, KERNEL_FLAGS_CSR, _csr_operator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = r'_ZN2kn23csr_stream_group_kernel'
(RELU, EXACT, NARROW, ROWS, LINEAR) = (_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_NARROW, _capi.KN_FLAG_NARROW_ROWS, _capi.KN_FLAG_NARROW_LINEAR)
# (W, NV) -> (static LDS bytes, counted wait of the loop).  A slot is one 16-step slab: 4 096 bytes of values + max(256, 64 W NV) of activations + 256 of column indices;
# as many slots as 64 KB hold, at most 11, three of them spare; the wait leaves (slots - 3 - 1) slabs x ceil((4 + max(1, W NV / 4) + 1) / W) loads per wavefront in flight
# (the form for 33 .. 64 columns, W = 8 x NV = 8, measured slower than the kernel it would replace and is not instantiated: narrow_linear_loses, kn_internal.h)
FORMS = {(1, 1): (11 * 4608, 7 * 6), (2, 1): (11 * 4608, 7 * 3), (4, 1): (11 * 4608, 7 * 2), (8, 1): (11 * 4864, 7 * 1), (8, 2): (11 * 5376, 7 * 2), (8, 4): (10 * 6400, 6 * 2)}


def test_header_declares_and_documents_the_flag_and_the_binding_mirrors_it():
    h = open(os.path.join(ROOT, 'include', 'keynet_hip.h')).read()
    m = re.search(r'#define\s+KN_FLAG_NARROW_LINEAR\s+\(?(\w+)u\)?\s*/\*(.*?)\*/', h, re.S)
    assert m and int(m.group(1), 0) == 512 and _capi.KN_FLAG_NARROW_LINEAR == 512
    doc = m.group(2)
    for word in ('csr_stream_group_kernel', 'bit for bit', 'changes NOTHING', 'kn_spmm_planes', 'kn_spmm_screen', 'kn_spmm_plan', '64 bits', 'KN_FLAG_NARROW_ROWS'):
        assert word in doc, word
    spmm_doc = h[h.index('What a caller may pass'):h.index('int kn_spmm(')]
    assert 'KN_FLAG_NARROW_LINEAR' in spmm_doc and 'any ldx' in spmm_doc[spmm_doc.index('KN_FLAG_NARROW_LINEAR'):]      # no guard: said in the table of kn_spmm
    flags = [_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_BF16X3, _capi.KN_FLAG_NARROW, _capi.KN_FLAG_NARROW_MFMA, _capi.KN_FLAG_NARROW_ROWS, _capi.KN_FLAG_NARROW32,
             _capi.KN_FLAG_NARROW64, _capi.KN_FLAG_NARROW64_MFMA, _capi.KN_FLAG_NARROW_LINEAR]
    assert sorted(flags) == [1 << i for i in range(10)]                   # one bit each
    v = re.search(r'#define\s+KN_ABI_VERSION\s+(\d+)', h)
    assert v and int(v.group(1)) == 5 and _capi.KN_ABI_VERSION == 5       # no entry point was added
    assert 'kn_csr_stream.hip' in SOURCES
    internal = open(os.path.join(ROOT, 'keynet_amd', 'csrc', 'kn_internal.h')).read()
    assert internal.count('& KN_FLAG_NARROW_LINEAR') == 1 and 'narrow_linear_call' in internal and 'narrow_linear_loses' in internal      # read in one place, next to its handle rule
    for src in SOURCES:
        assert 'KN_FLAG_NARROW_LINEAR' not in re.sub(r'//[^\n]*', '', open(os.path.join(ROOT, 'keynet_amd', 'csrc', src)).read()), src


def test_the_keyword_reaches_every_layer_of_the_python_host():
    for f in (ksys.KeyedModel.forward_linear, ksys.KeyedModel.forward, ksys.KeyedModel.capture, KeyedLayer.forward, KeyedLayer.kernel, KeyedLayer.launch,
              ksp._run_torchdot, ksp._narrow_args, ksp.SparseMatrix.torchdot, ksp.TiledMatrix.torchdot, ksp.DiagonalTiledMatrix.torchdot):
        p = inspect.signature(f).parameters
        assert 'narrow_linear' in p and p['narrow_linear'].default is False, f
        assert 'narrow_linear' in (f.__doc__ or ''), f


def test_argument_rule():
    A = ksp._narrow_args
    for narrow in (True, 'mfma'):
        assert A(8, narrow, False, narrow_linear=True) == (narrow, False)
        assert A(8, narrow, True, narrow_linear=True) == (narrow, True)
        assert A(32, narrow, False, narrow32=True, narrow_linear=True) == (narrow, False)
        with pytest.raises(ValueError):
            A(9, narrow, False, narrow_linear=True)                       # the width limit is that of the `narrow` keywords passed
        with pytest.raises(ValueError):
            A(33, narrow, False, narrow32=True, narrow_linear=True)
    assert A(64, True, False, narrow64=True, narrow_linear=True) == (True, False)
    with pytest.raises(ValueError):
        A(65, True, False, narrow64=True, narrow_linear=True)
    with pytest.raises(ValueError, match='narrow_linear=True is a form of the narrow forward'):
        A(2, False, False, narrow_linear=True)
    assert A(64, False, False, alone=True, narrow_linear=True) == (False, False)       # a container's own torchdot takes it alone, up to the kernel's range
    with pytest.raises(ValueError, match='narrow_linear=True takes at most 64'):
        A(65, False, False, alone=True, narrow_linear=True)
    assert A(8, True, False) == (True, False)                             # without the keyword nothing changed


def test_kernel_sets_the_flag_where_it_sets_the_row_lane_flag(monkeypatch):
    """KeyedLayer.kernel: KN_FLAG_NARROW_LINEAR under exactly the condition of KN_FLAG_NARROW_ROWS -- for every contract x narrow x relu on the tiny conv-taps operator and on
    a 12 x 9 CSR operator, the word with narrow_linear=True is the word of narrow_rows=True (tests/test_narrow_rows_host.py pins those) with the one bit for the other;
    without the keyword no word carries the flag."""
    conv = _tiny_conv()
    csr = _csr_operator()
    dense = (lambda device=None: 'a dense handle')
    swap = lambda w: (w & ~ROWS) | (LINEAR if w & ROWS else 0)
    for handle in (lambda device=None: None, dense):
        monkeypatch.setattr(csr, '_dense_device_op', handle, raising=False)
        for W in (conv, csr):
            for name in CONTRACTS:
                for narrow in (False, True, 'mfma'):
                    for relu in (False, True):
                        c = _contract(name, True)
                        rows = KeyedLayer.kernel(W, c, relu, None, narrow=narrow, narrow_rows=True)
                        lin = KeyedLayer.kernel(W, c, relu, None, narrow=narrow, narrow_linear=True)
                        both = KeyedLayer.kernel(W, c, relu, None, narrow=narrow, narrow_rows=True, narrow_linear=True)
                        plain = KeyedLayer.kernel(W, c, relu, None, narrow=narrow)
                        if rows is None:
                            assert lin is None and both is None and plain is None
                            continue
                        assert lin == (rows[0], swap(rows[1])) and both == (rows[0], rows[1] | (LINEAR if rows[1] & ROWS else 0)), (name, narrow, relu, rows, lin, both)
                        assert not plain[1] & LINEAR and not rows[1] & LINEAR
    monkeypatch.setattr(csr, '_dense_device_op', lambda device=None: None, raising=False)
    assert KeyedLayer.kernel(csr, True, True, narrow=True, narrow_linear=True) == (csr._device_op, EXACT | RELU | LINEAR)
    monkeypatch.setattr(csr, '_dense_device_op', dense, raising=False)
    assert KeyedLayer.kernel(csr, False, True, narrow=True, narrow_linear=True) == (dense, RELU)          # a re-ordering contract put it on its dense handle: it keeps it
    W64 = _csr_operator(np.float64)
    assert KeyedLayer.kernel(W64, True, False, narrow=True, narrow_linear=True)[1] == EXACT
    T = ksp.TiledMatrix(scipy.sparse.random(12, 12, density=0.3, format='csr', dtype=np.float32, random_state=2), (4, 4))
    assert KeyedLayer.kernel(T, True, False, narrow=True, narrow_linear=True) == (T._device_op, EXACT | LINEAR)
    assert KERNEL_FLAGS_CONV and KERNEL_FLAGS_CSR


def test_layers_plan_the_flag_only_inside_a_narrow_forward():
    c = KeyedLayer.fromoperator(_csr_operator(), 'Linear', exact=True)
    c.W._device_op = lambda device=None: 'handle'
    assert c.launch(None, narrow=True, narrow_linear=True).flags == EXACT | LINEAR
    assert c.launch(None, narrow=True, narrow_rows=True, narrow_linear=True).flags == EXACT | ROWS | LINEAR
    assert c.launch(None, narrow=True).flags == c.launch(None).flags == c.launch(None, narrow_linear=True).flags == EXACT


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='needs hipcc')
def test_kernel_isa(tmp_path):
    s = _isa('kn_csr_stream.hip', tmp_path)
    kernels = _kernel_bodies(s, [KERNEL])
    forms = sorted(tuple(int(v) for v in re.match(KERNEL + r'ILi(\d+)ELi(\d+)EE', k[0]).groups()) for k in kernels)
    assert forms == sorted(FORMS), forms
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    for (lds, _) in FORMS.values():                                      # what this test holds the ISA to is what DESIGN states
        assert '{:,}'.format(lds).replace(',', ' ') in design, lds
    assert 'one workgroup per CU' in design
    for (name, lines) in kernels:
        form = tuple(int(v) for v in re.match(KERNEL + r'ILi(\d+)ELi(\d+)EE', name).groups())
        (lds, wait) = FORMS[form]
        for l in lines:
            if FUSED.match(l):
                assert any(c in l for c in INT_DIVISION_LITERALS), 'fused multiply-add in %s: %s' % (name, l)
        assert any(re.match(r'v_(pk_)?mul_f32', l) for l in lines) and any(re.match(r'v_(pk_)?add_f32', l) for l in lines), name
        assert not any(l.startswith('scratch_') or (l.startswith('buffer_store') and 'offen' in l) for l in lines), 'spill in %s' % name
        assert not any('atomic' in l for l in lines), 'an atomic in %s' % name
        meta = s[s.index('.amdhsa_kernel ' + name):]
        meta = meta[:meta.index('.end_amdhsa_kernel')]
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', meta).group(1)) == 0, name
        assert int(re.search(r'\.amdhsa_group_segment_fixed_size\s+(\d+)', meta).group(1)) == lds <= 64 * 1024, name
        # occupancy: one workgroup per CU (a keyed Linear has fewer chunks than the chip has CUs) = ceil(W / 4) wavefronts per SIMD of 512 registers per lane
        vgprs = (int(re.search(r'\.amdhsa_next_free_vgpr\s+(\d+)', meta).group(1)) + 7) // 8 * 8
        assert 512 // vgprs >= (form[0] + 3) // 4, (name, vgprs)
        # the ring: every fill is an LDS-DMA load -- 16 bytes per lane for the values, 4 for the activations and the column indices --, every read of the walk an LDS read
        fills = [i for (i, l) in enumerate(lines) if l.startswith('global_load_lds')]
        assert any(lines[i].startswith('global_load_lds_dwordx4') for i in fills) and any(lines[i].startswith('global_load_lds_dword ') for i in fills), name
        assert all(re.match(r'global_load_lds_dword(x4)? ', lines[i]) for i in fills), name
        assert any(re.match(r'ds_read2?(st64)?_b32', l) for l in lines), name
        assert (form[0] == 1) == (not any(l.startswith('s_barrier') for l in lines)), name               # one wavefront needs no barrier
        # counted waits: from the first fill on every vmcnt of the kernel is the counted one or a full one, and no full one stands inside a loop that fills (the body of a backward branch
        # around a fill): the walk never drains the ring; the drain and the epilogue's wait stand behind the loops
        waits = [int(m.group(1)) for l in lines[fills[0]:] for m in [re.match(r's_waitcnt .*vmcnt\((\d+)\)', l)] if m]      # (ahead of the first fill: the column indices of the first slabs)
        assert waits.count(wait) >= 2 and set(waits) <= {wait, 0}, (name, wait, waits)
        # the blocks the compiler marks as part of a loop (the slab loop: its header and every block "in Loop")
        raw = s[s.index(name + ':'):]
        raw = raw[:raw.index('.Lfunc_end')].split('\n')[1:]
        (body, inloop) = ([], False)
        for l in raw:
            if re.match(r'\.LBB\d+_\d+:', l):
                inloop = 'Loop' in l
            elif inloop and l.split(';')[0].strip():
                body.append(l.split(';')[0].strip())
        assert any(l.startswith('global_load_lds') for l in body) and any(l.startswith('v_add_f32') or l.startswith('v_pk_add_f32') for l in body), name
        inside = [int(m.group(1)) for l in body for m in [re.match(r's_waitcnt .*vmcnt\((\d+)\)', l)] if m]
        assert inside and all(n == wait for n in inside), (name, wait, inside)
        # load ownership: in the loop the only vector-memory loads are the fills themselves, which own no register -- every register a load writes there is written by an
        # LDS read the compiler issued and waits for itself (lgkmcnt), so nothing is read or copied ahead of its wait; around the loop (from the first fill on) the same holds
        # up to the drain, behind which the epilogue loads its row index
        owned = [l for l in body if re.match(r'(global|buffer|flat|scratch)_load', l) and not l.startswith('global_load_lds')]
        assert not owned, (name, owned)
        assert not any(re.match(r's_(buffer_)?load', l) for l in body), name                              # ... and no scalar load either: nothing waits for memory but the counted wait
        tail = lines[fills[0]:]
        assert not [l for l in tail if re.match(r'(buffer|flat|scratch)_load', l)], name
    entries = list(re.finditer(r'\.name:\s+(%s\S*)' % KERNEL, s))
    assert len(entries) == len(FORMS)
    for m in entries:
        k = re.compile(r'\.private_segment_fixed_size:\s+(\d+)').search(s, m.end())
        assert k and int(k.group(1)) == 0, m.group(1)
