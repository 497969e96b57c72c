"""KN_MODIFIER_WINO on the host (keynet_amd/csrc/kn_wino.h: plain C++17, the derivation kn_api.hip runs on a handle's entry table).  tests/wino_host_main.cpp, a stand-alone
program with its own main, is compiled with g++ under the address and undefined-behaviour sanitizers (-DKN_HOST_PACK_ONLY as for the library's host build) and run
directly, nothing preloaded: 6x4, 2x2, 1x2 and a permuted 4x6 are eligible, hold exactly HiWi / 2 pseudo input pixels per j, and T_out . U . T_in equals the operator to
1e-12 in double at Cin = Cout = 2; an odd width, two entries on one (pixel, tap) pair, a coefficient other than 1, a moved entry and a 5x5 operator are refused with a
reason.  The conditions are the program's.  Header and binding agree on the flag, and the ABI version stays 5."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = ('ERROR: AddressSanitizer', 'runtime error:', 'ERROR: LeakSanitizer', 'AddressSanitizer:DEADLYSIGNAL')


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_wino_derivation_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / 'wino_host_main')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-DKN_HOST_PACK_ONLY', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-fno-omit-frame-pointer', '-I', os.path.join(ROOT, 'keynet_amd', 'csrc'), '-o', exe, os.path.join(ROOT, 'tests', 'wino_host_main.cpp')])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = p.stdout + p.stderr
    print(out)
    assert not any(b in out for b in BAD), out[-4000:]
    assert 'FAIL' not in out and p.returncode == 0 and 'all conditions hold' in p.stdout, out[-4000:]
    for reason in ('odd width', 'more than one entry', 'coefficients other than 1', 'not a 3 x 3 operator'):
        assert reason in out, (reason, out[-4000:])


def test_header_and_binding_agree_on_the_flag():
    from keynet_amd import _capi
    header = open(os.path.join(ROOT, 'include', 'keynet_hip.h')).read()
    m = re.search(r'#define\s+KN_MODIFIER_WINO\s+\(?(0x[0-9a-fA-F]+)u\)?', header)
    assert m and int(m.group(1), 16) == _capi.KN_MODIFIER_WINO == 0x4000
    others = [int(v, 16) if v.startswith('0x') else int(v) for v in re.findall(r'#define\s+KN_(?:FLAG|MODIFIER)_(?!WINO)\w+\s+\(?(0x[0-9a-fA-F]+|\d+)u\)?', header)]
    assert others and all(v & _capi.KN_MODIFIER_WINO == 0 for v in others)          # a bit of its own
    assert re.search(r'#define\s+KN_ABI_VERSION\s+5\b', header) and _capi.KN_ABI_VERSION == 5
    assert 'kn_reserve_workspace_flags' in _capi.SYMBOLS and 'kn_wino_status' in _capi.SYMBOLS
