"""Host-side checks of the matrix-core forward for 33 .. 64 images (narrow64='mfma', KN_FLAG_NARROW64_MFMA): the flag in the C ABI and its binding, the argument
rules of the keyword on both sides of each, the flag word KeyedLayer.kernel / launch form per contract, and the gfx950 ISA of the 64-column instantiations of
convtaps_mfma_kernel -- they exist, spill nothing, stay within 128 vector registers, hold the static LDS their tile shape says, run v_mfma_f32_32x32x2, and the
order-preserving kernels of the file still contain no fused multiply-add."""
import inspect
import os
import re
import shutil

import pytest

from keynet_amd import _capi
from keynet_amd import sparse as ksp
from keynet_amd import system as ksys
from keynet_amd.layer import KeyedLayer
from test_isa_lint import _isa, _kernel_bodies, FUSED, INT_DIVISION_LITERALS, ORDER_PRESERVING
from test_narrow_host import _tiny_conv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
(RELU, EXACT, BF16X3, NARROW, MFMA, N32, N64, N64M) = (_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_BF16X3, _capi.KN_FLAG_NARROW, _capi.KN_FLAG_NARROW_MFMA,
                                                       _capi.KN_FLAG_NARROW32, _capi.KN_FLAG_NARROW64, getattr(_capi, 'KN_FLAG_NARROW64_MFMA', None))


def test_header_declares_the_flag_and_the_binding_mirrors_it():
    h = open(os.path.join(ROOT, 'include', 'keynet_hip.h')).read()
    m = re.search(r'#define\s+KN_FLAG_NARROW64_MFMA\s+\(?(\w+)u\)?', h)
    assert m and int(m.group(1), 0) == 0x100
    assert N64M == 0x100
    assert sorted([RELU, EXACT, BF16X3, NARROW, MFMA, _capi.KN_FLAG_NARROW_ROWS, N32, N64, N64M]) == [1 << i for i in range(9)]      # one bit each
    v = re.search(r'#define\s+KN_ABI_VERSION\s+(\d+)', h)
    assert v and int(v.group(1)) == 5 and _capi.KN_ABI_VERSION == 5      # a flag of kn_spmm: no entry point added
    assert 'KN_FLAG_NARROW64_MFMA (33 .. 64)' in h                       # the line of the size-rule table of kn_spmm


def test_the_argument_rules():
    A = ksp._narrow_args
    for n in (1, 8, 9, 32, 33, 40, 64):
        assert A(n, 'mfma', False, narrow64='mfma') == ('mfma', False)
        assert A(n, 'mfma', False, narrow32=True, narrow64='mfma') == ('mfma', False)
    with pytest.raises(ValueError):
        A(65, 'mfma', False, narrow64='mfma')                             # at most 64 images
    for n in (4, 32, 40):
        for alone in (False, True):
            with pytest.raises(ValueError, match='narrow=\'mfma\''):
                A(n, True, False, alone=alone, narrow64='mfma')           # only together with narrow='mfma'
            with pytest.raises(ValueError):
                A(n, False, False, alone=alone, narrow64='mfma')
    for n in (33, 64):                                                    # narrow64=True keeps its meaning: no matrix-core form is ASKED for
        with pytest.raises(ValueError, match='no matrix-core form'):
            A(n, 'mfma', False, narrow64=True)
        assert A(n, True, False, narrow64=True) == (True, False)
    assert A(8, 'mfma', True, narrow64='mfma') == ('mfma', True)
    with pytest.raises(ValueError):
        A(9, 'mfma', True, narrow64='mfma')                               # the row-lane kernel is an 8-column kernel
    # the normalised keyword of a forward: 'mfma' beyond 32 images only
    F = ksys.KeyedModel._narrow64_form
    assert [F(n, 'mfma') for n in (1, 32, 33, 64)] == [True, True, 'mfma', 'mfma']
    assert [F(n, True) for n in (1, 32, 33, 64)] == [True] * 4 and F(40, False) is False


def test_the_keyword_value_is_documented_where_it_is_accepted():
    for f in (ksys.KeyedModel.forward_linear, ksys.KeyedModel.forward, ksys.KeyedModel.capture, KeyedLayer.forward, KeyedLayer.kernel, KeyedLayer.launch,
              ksp.Conv2dTiledMatrix.torchdot, ksp._run_torchdot, ksp._narrow_args):
        assert 'narrow64' in inspect.signature(f).parameters and "narrow64='mfma'" in f.__doc__, f


@pytest.mark.parametrize('contract', [True, False, 'auto', 'split', 'bf16x3'])
def test_the_flag_word_per_contract(contract):
    W = _tiny_conv()
    for relu in (False, True):
        r = RELU if relu else 0
        flags = KeyedLayer.kernel(W, contract, relu, narrow='mfma', narrow64='mfma')[1]
        if contract in (False, 'bf16x3'):
            assert flags == r | MFMA | N32 | N64 | N64M                  # and no other contract flag
        else:                                                             # what narrow64=True gives: the library runs the pipeline at 33 .. 64 columns
            assert flags == KeyedLayer.kernel(W, contract, relu, narrow='mfma', narrow64=True)[1] and not flags & N64M
        for narrow in (True, False):                                      # the value next to anything but narrow='mfma' adds no bit (the public methods refuse it)
            k = KeyedLayer.kernel(W, contract, relu, narrow=narrow, narrow64='mfma')
            assert k is None or not k[1] & N64M
        assert not KeyedLayer.kernel(W, contract, relu, narrow='mfma', narrow64=True)[1] & N64M


TILES = {(64, 16): 18432, (128, 16): 27136, (64, 4): 6144, (128, 4): 8704}      # 4 * (2 KC MT + 2 KC 64 + 256 + 2 (MT + 64)) bytes


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='needs hipcc')
def test_isa_of_the_64_column_tiles(tmp_path):
    s = _isa('kn_conv.hip', tmp_path)
    meta = {}
    for m in re.finditer(r'\.amdhsa_kernel (_ZN2kn20convtaps_mfma_kernelILi(\d+)ELi64ELi(\d+)ELi\dELi\dELi(\d)ELb0EEE\w+)(.*?)\.end_amdhsa_kernel', s, re.S):
        meta[(int(m.group(2)), int(m.group(3)), int(m.group(4)))] = (m.group(1), m.group(5))
    # generic, straight-line, wave-uniform, slot groups at KC = 16; generic and straight-line at KC = 4 (a 256-channel tile was measured slower: diagnostic build only)
    want = set((mt, 16, mode) for mt in (64, 128) for mode in (0, 1, 2, 3)) | set((mt, 4, mode) for mt in (64, 128) for mode in (0, 1))
    assert set(meta) == want, sorted(set(meta) ^ want)
    for ((mt, kc, mode), (name, body)) in sorted(meta.items()):
        get = lambda k: int(re.search(r'\.amdhsa_%s (\d+)' % k, body).group(1))
        assert get('private_segment_fixed_size') == 0, name                                   # no scratch
        assert get('group_segment_fixed_size') == TILES[(mt, kc)], (name, get('group_segment_fixed_size'))
        md = s[s.index('.name:', s.index('amdhsa.kernels')):]
        md = md[md.index('.name:           ' + name):]
        md = md[:md.index('.wavefront_size')]
        (vgpr, spill) = (int(re.search(r'\.vgpr_count:\s+(\d+)', md).group(1)), int(re.search(r'\.vgpr_spill_count:\s+(\d+)', md).group(1)))
        print(name, 'vgpr_count', vgpr)
        assert vgpr <= 128 and spill == 0, (name, vgpr, spill)
    bodies = _kernel_bodies(s, [r'_ZN2kn20convtaps_mfma_kernelILi\d+ELi64E'])
    assert len(bodies) == len(want)
    for (name, lines) in bodies:
        assert any(l.startswith('v_mfma_f32_32x32x2') for l in lines), name
    # the order-preserving kernels of the file: still no fused multiply-add (the notion of test_isa_lint.py)
    kernels = _kernel_bodies(s, ORDER_PRESERVING['kn_conv.hip'])
    assert kernels
    for (name, lines) in kernels:
        for l in lines:
            if FUSED.match(l):
                assert any(c in l for c in INT_DIVISION_LITERALS), 'fused multiply-add in an order-preserving kernel: %s: %s' % (name, l)
