"""The C-ABI library loads on a CPU-only box and exports every symbol include/keynet_hip.h declares (no compute calls)."""
import os
import re
import ctypes
import pytest
from keynet_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    src = open(os.path.join(ROOT, 'include', 'keynet_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(kn_[a-z0-9_]+)\s*\(', src)))


def test_library_exports_every_declared_symbol():
    syms = _header_symbols()
    assert len(syms) >= 16
    assert sorted(_capi.SYMBOLS) == syms, 'binding list and header disagree'
    L = ctypes.CDLL(_capi.LIBPATH)
    for s in syms:
        assert hasattr(L, s), 'libkeynet_hip.so does not export %s' % s


def test_abi_version_and_error_channel():
    L = _capi.lib()
    assert L.kn_abi_version() == _capi.KN_ABI_VERSION
    (n, arch) = _capi.device_info()
    assert n >= 0


def test_no_cpu_fallback_without_gpu():
    """On a box without an MI355X the product must fail loudly, never compute on the CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    import numpy as np
    import scipy.sparse
    from keynet_amd.sparse import SparseMatrix
    W = SparseMatrix(scipy.sparse.eye(4, dtype=np.float32).tocsr())
    with pytest.raises(_capi.KeynetHipError):
        W.torchdot(torch.ones(4, 2))
    with pytest.raises(_capi.KeynetHipError):
        _capi.Operator.csr((2, 2), [0, 1, 2], [0, 1], [1.0, 2.0])


def test_product_never_imports_oracle():
    """oracle/ is test infrastructure: nothing under keynet_amd/ may import or reference it."""
    pkg = os.path.join(ROOT, 'keynet_amd')
    for (d, _, files) in os.walk(pkg):
        for f in files:
            if f.endswith(('.py', '.hip', '.h', '.cpp')):
                src = open(os.path.join(d, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle\b', src, flags=re.M), f
                assert 'kn_oracle' not in src, f


def test_no_cpp_exception_crosses_the_c_abi():
    """include/keynet_hip.h promises integer codes only.  Sizes that cannot be allocated (a host std::vector of 2^60 elements throws
    std::length_error / std::bad_alloc inside the create function) and sizes that contradict the arrays must come back as codes with a
    message -- a C++ exception unwinding into ctypes would abort the interpreter, so surviving this test IS the assertion."""
    import numpy as np
    L = _capi.lib()
    h = ctypes.c_void_p()
    ip = np.array([0, 1, 2], dtype=np.int32)
    ix = np.array([0, 1], dtype=np.int32)
    dt = np.array([1.0, 2.0], dtype=np.float32)
    vp = (lambda a: a.ctypes.data_as(ctypes.c_void_p))
    # absurd nnz with valid small arrays
    for nnz in (1 << 60, (1 << 31) + 5, -3):
        rc = L.kn_csr_create(2, 2, nnz, vp(ip), vp(ix), vp(dt), ctypes.byref(h))
        assert rc in (1, 6) and h.value is None and len(L.kn_last_error()) > 0
    # 2^60 tile entries: the per-entry tables are host vectors sized by `nent` before any entry is read
    shp = np.array([1, 2, 2], dtype=np.int64)
    blocks = np.zeros((1, 3), dtype=np.int64)
    keys = np.zeros((1, 3), dtype=np.int64)
    isb = np.zeros(1, dtype=np.uint8)
    chan = np.ones((1, 1, 1), dtype=np.float32)
    bias = np.zeros(1, dtype=np.float32)
    rc = L.kn_conv2dtiled_create(4, 4, vp(shp), vp(shp), 1, vp(blocks), 1 << 60, vp(keys), vp(isb), vp(chan), vp(bias), ctypes.byref(h))
    assert rc == 4 and h.value is None, (rc, L.kn_last_error())          # KN_ERR_NOMEM
    assert b'alloc' in L.kn_last_error()
    # a well-formed call still works as before on this box (no device: KN_ERR_NODEVICE; with a device: a handle)
    rc = L.kn_csr_create(2, 2, 2, vp(ip), vp(ix), vp(dt), ctypes.byref(h))
    assert rc in (0, 5)
    if rc == 0:
        assert L.kn_destroy(h) == 0
