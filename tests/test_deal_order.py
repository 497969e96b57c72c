"""The dealing order of the matrix-core conv-taps kernels on the host (keynet_amd/csrc/kn_deal.h: plain C++17).  tests/deal_order_main.cpp, a stand-alone program
that includes the header, is compiled with g++ under the address and undefined-behaviour sanitizers and run: a permutation for every grid (1 x 1 .. 56 x 56, 9 x 7,
13 x 1), uniform weights give the input back, slot weight per XCD segment within 1.02 / 1.005 / 1.002 of the mean at 14 x 14 / 28 x 28 / 56 x 56, heavy pixels first
and a weight class in its input order inside every segment, and random weights 1 .. 19 on 784 pixels within 1.01.  The conditions are the program's; it prints a line
per case and exits 1 when one is missed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = ('ERROR: AddressSanitizer', 'runtime error:', 'ERROR: LeakSanitizer', 'AddressSanitizer:DEADLYSIGNAL')


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_deal_order_conditions_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / 'deal_order_main')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer',
                           '-I', os.path.join(ROOT, 'keynet_amd', 'csrc'), '-o', exe, os.path.join(ROOT, 'tests', 'deal_order_main.cpp')])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = p.stdout + p.stderr
    print(out)
    assert not any(b in out for b in BAD), out[-4000:]
    assert 'FAIL' not in out and p.returncode == 0 and 'all conditions hold' in p.stdout, out[-4000:]
