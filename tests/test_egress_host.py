"""The egress of frames, host side (no GPU): the rule of kn_linear_to_u8 as a numpy statement (the inverse of tests/test_ingest_host.py's u8_to_linear_rule), the
argument checks of linear_to_frames, column_range, KeyedSensor.decrypt_frames / asframes / asimage / save (each raised before any GPU call), gray_affine on CPU
tensors, the C ABI entries and their refusals, and the key algebra of save() with scipy."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse
import torch

from keynet_amd import _capi
from keynet_amd import system as ksys
from keynet_amd import torch as ktorch
from test_ingest_host import u8_to_linear_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5                  # the byte around the frames: nothing may change it
GUARD = 8                        # sentinel bytes in front of and behind the frames

# (t, byte) for t = gain * x + bias: round to nearest, ties to even, saturate, NaN -> 0
EDGES = [(0.5, 0), (1.5, 2), (2.5, 2), (254.5, 254), (255.5, 255), (-0.0, 0), (-0.4, 0), (-3.0, 0), (300.0, 255), (np.inf, 255), (-np.inf, 0), (np.nan, 0),
         (0.0, 0), (0.49999997, 0), (0.50000006, 1), (254.50002, 255), (255.0, 255), (127.5, 128), (128.5, 128)]


def linear_to_u8_rule(x, ldx, n, chw, layout, gain=None, bias=None):
    """include/keynet_hip.h's statement of kn_linear_to_u8 on a sentinel-filled byte buffer: x holds the feature-major block, rows of ldx floats (the ones row need not be
    there: it is not read); the result is GUARD sentinel bytes, the n frames of D bytes ([n, C, H, W] for layout 0, [n, H, W, C] for layout 1), GUARD sentinel bytes."""
    (c, h, w) = chw
    D = c * h * w
    assert layout in (0, 1) and 1 <= n <= ldx
    X = np.asarray(x, dtype=np.float32).reshape(-1)[:D * ldx].reshape(D, ldx)[:, :n]
    g = np.ones(n, np.float32) if gain is None else np.asarray(gain, dtype=np.float32).reshape(n)
    b = np.zeros(n, np.float32) if bias is None else np.asarray(bias, dtype=np.float32).reshape(n)
    with np.errstate(invalid='ignore', over='ignore'):
        t = (g[None, :] * X).astype(np.float32)                          # one IEEE f32 multiply
        t = (t + b[None, :]).astype(np.float32)                          # one IEEE f32 add
        r = np.clip(np.rint(t), np.float32(0), np.float32(255))          # ties to even; -Inf -> 0, +Inf -> 255
        r = np.where(np.isnan(t), np.float32(0), r).astype(np.uint8)
    frames = r.T.reshape(n, c, h, w)
    if layout == 1:
        frames = frames.transpose(0, 2, 3, 1)
    out = np.full(GUARD + n * D + GUARD, SENTINEL, dtype=np.uint8)
    out[GUARD:GUARD + n * D] = np.ascontiguousarray(frames).reshape(-1)
    return out


def frames_of(buf, n, chw, layout):
    (c, h, w) = chw
    assert np.all(buf[:GUARD] == SENTINEL) and np.all(buf[GUARD + n * c * h * w:] == SENTINEL)
    return buf[GUARD:GUARD + n * c * h * w].reshape((n, c, h, w) if layout == 0 else (n, h, w, c))


@pytest.mark.parametrize('layout', [0, 1], ids=['NCHW', 'NHWC'])
@pytest.mark.parametrize('shape', [(1, 5, 7), (3, 9, 11), (3, 32, 32)])
def test_rule_inverts_the_ingest_rule(shape, layout):
    (C, H, W) = shape
    n = 5
    rng = np.random.RandomState(1)
    frames = rng.randint(0, 256, size=(n, C, H, W) if layout == 0 else (n, H, W, C)).astype(np.uint8)
    block = u8_to_linear_rule(frames, layout, n + 3, n + 4)              # [D + 1, n + 4]: pad columns and sentinel NaNs beyond n
    back = linear_to_u8_rule(block, n + 4, n, shape, layout)
    assert np.array_equal(frames_of(back, n, shape, layout), frames)
    other = linear_to_u8_rule(block, n + 4, n, shape, 1 - layout)      # the other layout: the same images, permuted
    want = frames.transpose(0, 2, 3, 1) if layout == 0 else frames.transpose(0, 3, 1, 2)
    assert np.array_equal(frames_of(other, n, shape, 1 - layout), want)


def test_rule_on_the_edge_values():
    t = np.array([e[0] for e in EDGES], dtype=np.float32)
    want = np.array([e[1] for e in EDGES], dtype=np.uint8)
    got = linear_to_u8_rule(t.reshape(-1, 1), 1, 1, (1, 1, len(EDGES)), 0)
    assert np.array_equal(frames_of(got, 1, (1, 1, len(EDGES)), 0).reshape(-1), want)
    # the same values reached through an affine: 2 * (t / 2) + 0 is exact, and a bias moves a tie
    got = linear_to_u8_rule((t / 2).reshape(-1, 1), 1, 1, (1, 1, len(EDGES)), 0, gain=[2.0], bias=[0.0])
    assert np.array_equal(frames_of(got, 1, (1, 1, len(EDGES)), 0).reshape(-1), want)
    got = linear_to_u8_rule(np.array([[0.5], [1.5], [254.0]], np.float32), 1, 1, (1, 1, 3), 0, bias=[1.0])
    assert list(frames_of(got, 1, (1, 1, 3), 0).reshape(-1)) == [2, 2, 255]


@pytest.fixture
def no_gpu_call(monkeypatch):
    """Any _capi compute call, and any move to the device, fails the test."""
    def reached(*a, **k):
        raise AssertionError('a GPU call was reached')
    for name in ('linear_to_u8', 'column_range', 'u8_to_linear', 'affine_to_linear', 'linear_to_affine'):
        monkeypatch.setattr(_capi, name, reached)
    monkeypatch.setattr(ksys.ksp, '_device_block', reached)
    monkeypatch.setattr(ksys.ksp, '_run_torchdot', reached)


def _sensor(shape=(3, 8, 8)):
    np.random.seed(2)
    return ksys.Keynet(shape, None, global_geometric='permutation')[0]


def test_linear_to_frames_refuses_before_the_gpu(no_gpu_call):
    good = torch.zeros((2, 3 * 8 * 8 + 1))
    with pytest.raises(ValueError, match='layout'):
        ktorch.linear_to_frames(good, (3, 8, 8), layout='HWC')
    with pytest.raises(ValueError, match='rank'):
        ktorch.linear_to_frames(good[0], (3, 8, 8))
    with pytest.raises(ValueError, match='float32'):
        ktorch.linear_to_frames(good.double(), (3, 8, 8))
    with pytest.raises(ValueError, match='features'):
        ktorch.linear_to_frames(good, (3, 8, 7))
    with pytest.raises(ValueError, match='inshape'):
        ktorch.linear_to_frames(good, (3, 8))
    with pytest.raises(ValueError, match='torch tensor'):
        ktorch.linear_to_frames(good.numpy(), (3, 8, 8))
    with pytest.raises(ValueError, match='on the device'):
        ktorch.linear_to_frames(good, (3, 8, 8))
    with pytest.raises(ValueError, match='rank'):
        ktorch.column_range(good[0])
    with pytest.raises(ValueError, match='on the device'):
        ktorch.column_range(good)


def test_sensor_egress_refuses_before_the_gpu(no_gpu_call, tmp_path):
    sensor = _sensor()
    good = torch.zeros((2, 3 * 8 * 8 + 1))
    with pytest.raises(ValueError, match='layout'):
        sensor.decrypt_frames(good, layout='nhwc')
    with pytest.raises(ValueError, match='rank'):
        sensor.decrypt_frames(good[0])
    with pytest.raises(ValueError, match='float32'):
        sensor.decrypt_frames(good.to(torch.uint8))
    with pytest.raises(ValueError, match='features'):
        sensor.decrypt_frames(torch.zeros((2, 3 * 8 * 8)))
    with pytest.raises(ValueError, match='on the device'):
        sensor.decrypt_frames(good)
    assert sensor._tensor is None
    x = torch.rand((1, 3, 8, 8))
    sensor.fromtensor(x)
    with pytest.raises(ValueError, match='layout'):
        sensor.asframes(layout='HWC')
    with pytest.raises(AssertionError, match='encrypt'):
        sensor.save(str(tmp_path / 'plain.png'))                       # save() stores the ENCRYPTED image
    assert not os.path.exists(str(tmp_path / 'plain.png'))
    assert torch.equal(sensor._tensor, x)
    two = ksys.Keynet((2, 4, 4), None, global_geometric='permutation')[0].fromtensor(torch.rand((1, 2, 4, 4)))
    with pytest.raises(ValueError, match='channels'):
        two.asimage()
    with pytest.raises(AssertionError, match='Load image first'):
        _sensor().asframes()
    public = ksys.PublicKeyedSensor((3, 8, 8))
    with pytest.raises(ValueError):
        public.encrypt()
    with pytest.raises(ValueError):
        public.decrypt()


def test_header_declares_and_capi_binds_the_egress():
    src = open(os.path.join(ROOT, 'include', 'keynet_hip.h')).read()
    rng_decl = re.search(r'int kn_column_range\(const float\* x_dev, int64_t rows, int64_t ld, int64_t n_vecs,\s*float\* lo_dev, float\* hi_dev, void\* stream\);', src)
    u8_decl = re.search(r'int kn_linear_to_u8\(const float\* x_dev, int64_t ldx, int64_t n, int64_t c, int64_t h, int64_t w, int layout,\s*'
                        r'const float\* gain_dev, const float\* bias_dev, uint8_t\* img_dev, void\* stream\);', src)
    assert rng_decl and u8_decl, 'include/keynet_hip.h does not declare the two entry points as specified'
    comment = src[:u8_decl.start()].rsplit('/*', 1)[1]
    for line in ('keynet/torch.py:71-77', 'keynet/sparse.py:25-33', 'keynet/system.py:173-181', 'one IEEE f32 multiply', 'never fused', 'ties to even'):
        assert line in comment, line
    assert 'keynet/sparse.py:25-33' in src[:rng_decl.start()].rsplit('/*', 1)[1]
    assert re.search(r'#define KN_ABI_VERSION 5\b', src) and _capi.KN_ABI_VERSION == 5          # added entry points leave the version where it is
    flags = sorted(set(re.findall(r'\bKN_FLAG_[A-Z0-9_]+', src)))
    assert not [f for f in flags if 'U8' in f or 'RANGE' in f or 'GRAY' in f]
    for name in ('kn_column_range', 'kn_linear_to_u8'):
        assert name in _capi.SYMBOLS
    assert callable(_capi.column_range) and callable(_capi.linear_to_u8)
    L = _capi.lib()
    assert len(L.kn_column_range.argtypes) == 7 and len(L.kn_linear_to_u8.argtypes) == 11


def test_entry_points_refuse_without_a_device():
    """Shape and NULL refusals come back as codes before anything touches a device (the style of the kn_chain_create checks of tests/test_contract_host.py)."""
    L = _capi.lib()
    (x, img, lo, hi) = (ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(12288), ctypes.c_void_p(16384))      # never dereferenced: every call is refused
    (INVALID, SHAPE) = (1, 2)
    assert L.kn_linear_to_u8(x, 4, 0, 3, 5, 7, 1, None, None, img, None) == SHAPE               # n = 0
    assert L.kn_linear_to_u8(x, 4, 5, 3, 5, 7, 1, None, None, img, None) == SHAPE               # n > ldx
    assert L.kn_linear_to_u8(x, 4, 4, 0, 5, 7, 1, None, None, img, None) == SHAPE               # c = 0
    assert L.kn_linear_to_u8(x, 4, 4, 3, 5, 0, 0, None, None, img, None) == SHAPE               # w = 0
    assert L.kn_linear_to_u8(x, 4, 4, 3, 5, 7, 2, None, None, img, None) == INVALID             # no such layout
    assert L.kn_linear_to_u8(None, 4, 4, 3, 5, 7, 1, None, None, img, None) == INVALID
    assert L.kn_linear_to_u8(x, 4, 4, 3, 5, 7, 1, None, None, None, None) == INVALID
    assert len(L.kn_last_error()) > 0
    assert L.kn_column_range(x, 10, 3, 4, lo, hi, None) == SHAPE                                # ld < n_vecs
    assert L.kn_column_range(x, -1, 4, 4, lo, hi, None) == INVALID
    assert L.kn_column_range(None, 10, 4, 4, lo, hi, None) == INVALID
    assert L.kn_column_range(x, 10, 4, 4, None, hi, None) == INVALID
    assert L.kn_column_range(x, 10, 4, 4, lo, None, None) == INVALID
    assert len(L.kn_last_error()) > 0


def test_gray_affine_on_cpu_tensors():
    inf = float('inf')
    lo = torch.tensor([0.0, -3.0, 7.0, -inf, 0.0, inf, float('nan'), 1.0, 0.0], dtype=torch.float32)
    hi = torch.tensor([255.0, 5.0, 7.0, 4.0, inf, -inf, 2.0, 1.0 + 2.0 ** -23, 1e-42], dtype=torch.float32)
    (gain, bias) = ktorch.gray_affine(lo, hi)
    assert gain.dtype == torch.float32 and bias.dtype == torch.float32
    assert gain[0] == 1.0 and bias[0] == 0.0
    assert gain[1] == np.float32(255.0) / np.float32(8.0) and bias[1] == np.float32(3.0) * gain[1]
    for k in (2, 3, 4, 5, 6, 8):                                         # constant, infinite either way, empty, NaN, a span whose gain overflows: black
        assert gain[k] == 0.0 and bias[k] == 0.0, k
    assert torch.isfinite(gain[7]) and gain[7] > 0                       # the smallest span above a float: still a range
    # the mapped ends: lo lands on 0 exactly, hi on 255 after rounding
    for k in (0, 1):
        (g, b) = (np.float32(gain[k]), np.float32(bias[k]))
        assert np.float32(g * np.float32(lo[k])) + b == 0.0
        assert np.rint(np.float32(np.float32(g * np.float32(hi[k])) + b)) == 255.0


@pytest.mark.parametrize('shape', [(1, 6, 5), (3, 8, 8)])
def test_save_key_algebra(shape):
    """imagekey . (quantised gray image / 255, 1) is the original image to within half a gray step of the ENCRYPTED image's range, (hi - lo) / 510, plus
    2^-12 * max(1, |hi|, |lo|): sixteen ulps of 255 for the float32 affine and its inverse."""
    sensor = _sensor(shape)
    D = int(np.prod(shape))
    rng = np.random.RandomState(4)
    x = (rng.rand(D) * 255).astype(np.float32)
    (E, Dk) = sensor.keypair()
    xc = scipy.sparse.csr_matrix(E).astype(np.float32).dot(np.concatenate((x, [1.0])).astype(np.float32)).astype(np.float32)
    (lo, hi) = (float(xc[:D].min()), float(xc[:D].max()))
    (gain, bias) = ktorch.gray_affine(torch.tensor([lo]), torch.tensor([hi]))
    q = frames_of(linear_to_u8_rule(xc.reshape(D + 1, 1), 1, 1, shape, 0, gain.numpy(), bias.numpy()), 1, shape, 0).reshape(D)
    assert q.min() == 0 and q.max() == 255
    key = sensor.gray_imagekey(gain[0], bias[0])
    assert scipy.sparse.issparse(key) and key.shape == (D + 1, D + 1) and key.dtype == np.float32
    stored = np.concatenate((q.astype(np.float32) * np.float32(1.0 / 255.0), [1.0])).astype(np.float32)
    back = key.dot(stored)
    assert back.dtype == np.float32 and back[D] == 1.0
    bound = (hi - lo) / 510.0 + 2.0 ** -12 * max(1.0, abs(hi), abs(lo))
    err = float(np.abs(back[:D].astype(np.float64) - x.astype(np.float64)).max())
    assert err <= bound, (err, bound)
    assert err > 0.01 * bound                                            # (the quantisation is there: the check is not vacuous)
    with pytest.raises(ValueError, match='no inverse'):
        sensor.gray_imagekey(torch.tensor(0.0), torch.tensor(0.0))
