"""Quantised encrypted frames as the wire between sensor and model, host side (no GPU): the rules of kn_frames_to_linear and kn_linear_to_u16 as numpy statements,
gray_inverse and the levels of gray_affine on CPU tensors, the round-trip bound of egress then ingest, the argument checks of every new Python call (each raised before
any GPU call), the C ABI entries and their refusals, and the constructor rules of the two new StreamedForward kinds."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from keynet_amd import _capi
from keynet_amd import stream as kstream
from keynet_amd import system as ksys
from keynet_amd import torch as ktorch
from keynet_amd.models import LeNet_AvgPool
from keynet_amd.stream import StreamedForward
from test_egress_host import linear_to_u8_rule
from test_ingest_host import NAN_BITS, u8_to_linear_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL16 = 0xA5C3              # the halfword around 16-bit frames: nothing may change it
GUARD = 8                        # sentinel elements in front of and behind the frames
LEVELS = {8: 255, 16: 65535}
DTYPES = {8: np.uint8, 16: np.uint16}


def frames_to_linear_rule(img, layout, n_cols, ldo, scale=None, offset=None):
    """include/keynet_hip.h's statement of kn_frames_to_linear on a sentinel-filled [D + 1, ldo] block: img is [n, C, H, W] (layout 0) or [n, H, W, C] (layout 1), uint8
    or uint16; scale / offset are None or n floats.  The multiply and the add are two float32 operations, each rounded."""
    img = np.asarray(img)
    assert img.dtype in (np.uint8, np.uint16) and img.ndim == 4 and layout in (0, 1)
    (n, c, h, w) = img.shape if layout == 0 else (img.shape[0], img.shape[3], img.shape[1], img.shape[2])
    assert 1 <= n <= n_cols <= ldo
    D = c * h * w
    out = np.full((D + 1, ldo), NAN_BITS, dtype=np.uint32).view(np.float32)
    out[:, n:n_cols] = np.float32(0.0)                                   # a zero image is a zero image: it is not `offset`
    out[D, :n] = np.float32(1.0)
    planes = img if layout == 0 else img.transpose(0, 3, 1, 2)
    t = planes.reshape(n, D).T.astype(np.float32)                        # exact at both depths
    with np.errstate(invalid='ignore', over='ignore'):
        if scale is not None:
            t = (np.asarray(scale, dtype=np.float32).reshape(1, n) * t).astype(np.float32)        # one IEEE f32 multiply
        if offset is not None:
            t = (t + np.asarray(offset, dtype=np.float32).reshape(1, n)).astype(np.float32)       # one IEEE f32 add
    out[:D, :n] = t
    return out


def linear_to_u16_rule(x, ldx, n, chw, layout, gain=None, bias=None):
    """include/keynet_hip.h's statement of kn_linear_to_u16 on a sentinel-filled uint16 buffer: GUARD sentinels, the n frames of D halfwords, GUARD sentinels."""
    (c, h, w) = chw
    D = c * h * w
    assert layout in (0, 1) and 1 <= n <= ldx
    X = np.asarray(x, dtype=np.float32).reshape(-1)[:D * ldx].reshape(D, ldx)[:, :n]
    g = np.ones(n, np.float32) if gain is None else np.asarray(gain, dtype=np.float32).reshape(n)
    b = np.zeros(n, np.float32) if bias is None else np.asarray(bias, dtype=np.float32).reshape(n)
    with np.errstate(invalid='ignore', over='ignore'):
        t = (g[None, :] * X).astype(np.float32)                          # one IEEE f32 multiply
        t = (t + b[None, :]).astype(np.float32)                          # one IEEE f32 add
        r = np.clip(np.rint(t), np.float32(0), np.float32(65535))        # ties to even; -Inf -> 0, +Inf -> 65535
        r = np.where(np.isnan(t), np.float32(0), r).astype(np.uint16)
    frames = r.T.reshape(n, c, h, w)
    if layout == 1:
        frames = frames.transpose(0, 2, 3, 1)
    out = np.full(GUARD + n * D + GUARD, SENTINEL16, dtype=np.uint16)
    out[GUARD:GUARD + n * D] = np.ascontiguousarray(frames).reshape(-1)
    return out


def frames16_of(buf, n, chw, layout):
    (c, h, w) = chw
    assert np.all(buf[:GUARD] == SENTINEL16) and np.all(buf[GUARD + n * c * h * w:] == SENTINEL16)
    return buf[GUARD:GUARD + n * c * h * w].reshape((n, c, h, w) if layout == 0 else (n, h, w, c))


def roundtrip_bound(lo, hi, levels):
    """The largest |restored - x| of egress by gray_affine(lo, hi, levels) then ingest by gray_inverse(lo, hi, levels), for features x in [lo, hi]:
    half a gray step s = (hi - lo) / levels, plus the float32 roundings -- of gain * x + bias before rint, which is up to 2^-23 * levels * max(|lo|, |hi|) / (hi - lo)
    <= 4 * 2^-23 * levels gray steps per operation under the condition, and of scale * q + offset on the way back, relative to max(|lo|, |hi|).  The condition
    max(|lo|, |hi|) <= 4 * (hi - lo) is asserted per case: a narrow range far from zero has no such bound in float32."""
    (lo, hi) = (np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64))
    big = np.maximum(np.abs(lo), np.abs(hi))
    assert np.all(hi > lo) and np.all(big <= 4.0 * (hi - lo)), 'the input condition of the round-trip bound does not hold'
    s = (hi - lo) / levels
    return (0.5 + 16.0 * 2.0 ** -23 * levels) * s + 4.0 * 2.0 ** -23 * big


def random_ranges(rng, k):
    """k ranges (lo, hi), float32, under the condition of roundtrip_bound: spans over several binades, placed so that zero is inside, at an end, or up to 3 spans away."""
    span = (2.0 ** rng.uniform(-6, 10, size=k)).astype(np.float32)
    lo = (span * rng.uniform(-4.0, 3.0, size=k)).astype(np.float32)
    hi = (lo + span).astype(np.float32)
    keep = np.maximum(np.abs(lo), np.abs(hi)).astype(np.float64) <= 4.0 * (hi.astype(np.float64) - lo.astype(np.float64))
    return (lo[keep], hi[keep])


@pytest.mark.parametrize('depth', [8, 16])
@pytest.mark.parametrize('layout', [0, 1], ids=['NCHW', 'NHWC'])
def test_ingest_rule(depth, layout):
    (n, C, H, W) = (3, 3, 4, 5)
    D = C * H * W
    rng = np.random.RandomState(depth + layout)
    img = rng.randint(0, LEVELS[depth] + 1, size=(n, C, H, W) if layout == 0 else (n, H, W, C)).astype(DTYPES[depth])
    plain = frames_to_linear_rule(img, layout, n + 2, n + 3)
    if depth == 8:                                                       # no scale, no offset: kn_u8_to_linear's block
        assert np.array_equal(plain.view(np.uint32), u8_to_linear_rule(img, layout, n + 2, n + 3).view(np.uint32))
    (scale, offset) = (np.array([0.5, -3.0, 0.0], np.float32), np.array([-7.25, 1e-3, 2.0], np.float32))
    got = frames_to_linear_rule(img, layout, n + 2, n + 3, scale, offset)
    planes = (img if layout == 0 else img.transpose(0, 3, 1, 2)).reshape(n, D)
    for b in range(n):
        for r in (0, D // 2, D - 1):
            want = np.float32(np.float32(scale[b] * np.float32(planes[b, r])) + offset[b])
            assert got[r, b] == want
    assert np.all(got[:D, 2] == 2.0)                                     # a zero scale: the offset
    assert np.array_equal(got[:, n:n + 2].view(np.uint32), np.zeros((D + 1, 2), np.uint32))               # pad columns: +0.0, not offset
    assert np.all(got[D, :n] == 1.0) and np.all(got[:, n + 2:].view(np.uint32) == NAN_BITS)
    # the multiply and the add round separately: a fused multiply-add differs on this operand
    (s, q, o) = (np.float32(1.0 + 2.0 ** -23), np.uint16(255), np.float32(-255.0))
    two = frames_to_linear_rule(np.full((1, 1, 1, 1), q, DTYPES[depth]), 0, 1, 1, [s], [o])[0, 0]
    assert two == np.float32(np.float32(s * np.float32(q)) + o) and float(two) != float(s) * float(q) + float(o)


def test_egress16_rule():
    edges = [(0.5, 0), (1.5, 2), (2.5, 2), (65534.5, 65534), (65535.5, 65535), (-0.0, 0), (-0.4, 0), (-3.0, 0), (70000.0, 65535), (np.inf, 65535), (-np.inf, 0),
             (np.nan, 0), (255.5, 256), (256.5, 256), (32767.5, 32768), (65535.0, 65535), (0.49999997, 0), (0.50000006, 1)]
    t = np.array([e[0] for e in edges], dtype=np.float32)
    want = np.array([e[1] for e in edges], dtype=np.uint16)
    shape = (1, 1, len(edges))
    assert np.array_equal(frames16_of(linear_to_u16_rule(t.reshape(-1, 1), 1, 1, shape, 0), 1, shape, 0).reshape(-1), want)
    got = linear_to_u16_rule((t / 2).reshape(-1, 1), 1, 1, shape, 0, gain=[2.0], bias=[0.0])
    assert np.array_equal(frames16_of(got, 1, shape, 0).reshape(-1), want)
    # below 256 the two depths agree, and the 16-bit rule inverts the ingest rule in both layouts
    rng = np.random.RandomState(3)
    x = (rng.rand(12, 2) * 255).astype(np.float32)
    assert np.array_equal(frames16_of(linear_to_u16_rule(x, 2, 2, (3, 2, 2), 1), 2, (3, 2, 2), 1), linear_to_u8_rule(x, 2, 2, (3, 2, 2), 1)[8:-8].reshape(2, 2, 2, 3))
    for layout in (0, 1):
        f = rng.randint(0, 65536, size=(2, 3, 2, 2) if layout == 0 else (2, 2, 2, 3)).astype(np.uint16)
        block = frames_to_linear_rule(f, layout, 3, 4)
        assert np.array_equal(frames16_of(linear_to_u16_rule(block, 4, 2, (3, 2, 2), layout), 2, (3, 2, 2), layout), f)


def test_gray_inverse_on_cpu_tensors():
    (inf, nan) = (float('inf'), float('nan'))
    lo = torch.tensor([0.0, -3.0, 7.0, inf, nan, -inf, -3.0], dtype=torch.float32)
    hi = torch.tensor([255.0, 5.0, 7.0, -inf, 1.0, 3.0, 5.0], dtype=torch.float32)
    (scale, offset) = ktorch.gray_inverse(lo, hi)
    assert scale.dtype == torch.float32 and offset.dtype == torch.float32
    assert scale[0] == 1.0 and offset[0] == 0.0
    assert scale[1] == np.float32(8.0) / np.float32(255.0) and offset[1] == -3.0                   # a normal range
    assert scale[2] == 0.0 and offset[2] == 7.0                                                    # a constant image: restored exactly
    for k in (3, 4, 5):                                                                            # (+Inf, -Inf), (NaN, 1), (-Inf, 3)
        assert scale[k] == 0.0 and offset[k] == 0.0, k
        assert not np.signbit(scale[k].item()) or scale[k] == 0
    (scale16, offset16) = ktorch.gray_inverse(lo, hi, levels=65535)
    assert scale16[1] == np.float32(8.0) / np.float32(65535.0) and offset16[1] == -3.0
    assert scale16[0] == np.float32(255.0) / np.float32(65535.0)
    assert scale16[2] == 0.0 and offset16[2] == 7.0 and scale16[3] == 0.0 and offset16[3] == 0.0
    (s2, o2) = ktorch.gray_inverse(torch.tensor([0.0]), torch.tensor([65535.0]), 65535)
    assert s2[0] == 1.0 and o2[0] == 0.0


def test_gray_affine_levels():
    lo = torch.tensor([0.0, -3.0, 7.0, float('-inf'), 0.25], dtype=torch.float32)
    hi = torch.tensor([255.0, 5.0, 7.0, 4.0, 900.0], dtype=torch.float32)
    (g0, b0) = ktorch.gray_affine(lo, hi)
    (g1, b1) = ktorch.gray_affine(lo, hi, 255)
    assert torch.equal(g0, g1) and torch.equal(b0, b1)                   # the default keeps its values bit for bit
    (g, b) = ktorch.gray_affine(lo, hi, levels=65535)
    assert g[0] == 257.0 and b[0] == 0.0
    assert g[1] == np.float32(65535.0) / np.float32(8.0) and b[1] == np.float32(3.0) * g[1]
    assert g[2] == 0.0 and b[2] == 0.0 and g[3] == 0.0 and b[3] == 0.0
    (g, b) = ktorch.gray_affine(torch.tensor([0.0]), torch.tensor([65535.0]), 65535)
    assert g[0] == 1.0 and b[0] == 0.0


@pytest.mark.parametrize('depth', [8, 16])
def test_roundtrip_bound_in_numpy(depth):
    """egress by gray_affine then ingest by gray_inverse, both as the numpy rules, over 4 000 random ranges: every feature within roundtrip_bound."""
    levels = LEVELS[depth]
    rng = np.random.RandomState(100 + depth)
    (lo, hi) = random_ranges(rng, 4000)
    n = lo.size
    assert n > 3000
    D = 64
    u = rng.rand(D, n)
    u[0, :] = 0.0                                                        # both ends of every range are among the features
    u[1, :] = 1.0
    x = np.clip((lo[None, :].astype(np.float64) + u * (hi.astype(np.float64) - lo.astype(np.float64))[None, :]).astype(np.float32), lo[None, :], hi[None, :])
    bound = roundtrip_bound(lo, hi, levels)                              # asserts the input condition per case
    (gain, bias) = ktorch.gray_affine(torch.as_tensor(lo), torch.as_tensor(hi), levels)
    (scale, offset) = ktorch.gray_inverse(torch.as_tensor(lo), torch.as_tensor(hi), levels)
    assert bool((gain > 0).all())
    if depth == 8:
        q = linear_to_u8_rule(x, n, n, (1, 1, D), 0, gain.numpy(), bias.numpy())[8:-8].reshape(n, 1, 1, D)
    else:
        q = frames16_of(linear_to_u16_rule(x, n, n, (1, 1, D), 0, gain.numpy(), bias.numpy()), n, (1, 1, D), 0)
    back = frames_to_linear_rule(q, 0, n, n, scale.numpy(), offset.numpy())[:D]
    err = np.abs(back.astype(np.float64) - x.astype(np.float64))
    ratio = float((err / bound[None, :]).max())
    print('depth %d: worst |restored - x| / bound = %.3f over %d ranges' % (depth, ratio, n))
    assert ratio <= 1.0, ratio
    assert ratio > 0.5                                                   # (the quantisation is there: the check is not vacuous)
    with pytest.raises(AssertionError, match='input condition'):
        roundtrip_bound(np.float32(100.0), np.float32(101.0), levels)


@pytest.fixture
def no_gpu_call(monkeypatch):
    """Any _capi compute call, and any move to the device, fails the test."""
    def reached(*a, **k):
        raise AssertionError('a GPU call was reached')
    for name in ('frames_to_linear', 'linear_to_u16', 'linear_to_u8', 'column_range', 'u8_to_linear', 'affine_to_linear', 'linear_to_affine'):
        monkeypatch.setattr(_capi, name, reached)
    monkeypatch.setattr(ksys.ksp, '_device_block', reached)
    monkeypatch.setattr(ksys.ksp, '_run_torchdot', reached)


@pytest.fixture(scope='module')
def lenet():
    torch.manual_seed(0)
    np.random.seed(0)
    return ksys.PermutationKeynet((1, 28, 28), LeNet_AvgPool().eval())


def test_torch_calls_refuse_before_the_gpu(no_gpu_call):
    good = torch.zeros((2, 28, 28, 1), dtype=torch.uint16)
    with pytest.raises(ValueError, match='uint8 or torch.uint16'):
        ktorch.frames_to_linear(good.to(torch.int32))
    with pytest.raises(ValueError, match='rank'):
        ktorch.frames_to_linear(good[0])
    with pytest.raises(ValueError, match='layout'):
        ktorch.frames_to_linear(good, layout='HWC')
    with pytest.raises(ValueError, match='pad_to'):
        ktorch.frames_to_linear(good, pad_to=0)
    with pytest.raises(ValueError, match='on the device'):
        ktorch.frames_to_linear(good, scale=torch.ones(2))
    block = torch.zeros((2, 28 * 28 + 1))
    with pytest.raises(ValueError, match='depth'):
        ktorch.linear_to_frames(block, (1, 28, 28), depth=12)
    with pytest.raises(ValueError, match='on the device'):
        ktorch.linear_to_frames(block, (1, 28, 28), depth=16)
    with pytest.raises(ValueError, match='lo must be a float32 tensor'):
        ktorch.cipher_range(good, torch.zeros(3), torch.ones(2), 2)
    with pytest.raises(ValueError, match='hi must be a float32 tensor'):
        ktorch.cipher_range(good, torch.zeros(2), torch.ones(2).double(), 2)


def test_scale_and_offset_follow_the_per_image_rule():
    """frames_to_linear's scale / offset are checked as linear_to_frames's gain / bias are: float32 [n] on the device of the frames (checked here without a device)."""
    dev = torch.device('cpu')
    assert ktorch._per_image(None, 2, dev, 'scale') is None
    for bad in (torch.ones(3), torch.ones(2).double(), torch.ones((2, 1)), [1.0, 1.0]):
        with pytest.raises(ValueError, match=r'scale must be None or a float32 tensor of shape \[2\]'):
            ktorch._per_image(bad, 2, dev, 'scale')
    with pytest.raises(ValueError, match='offset must be on the device'):
        ktorch._per_image(torch.ones(2), 2, dev, 'offset')


def test_sensor_calls_refuse_before_the_gpu(no_gpu_call, lenet):
    (sensor, _) = lenet
    good = torch.zeros((2, 28, 28, 1), dtype=torch.uint8)
    with pytest.raises(ValueError, match='uint8'):
        sensor.encrypt_to_frames(good.float())
    with pytest.raises(ValueError, match='uint8'):
        sensor.encrypt_to_frames(good.to(torch.uint16))                  # plaintext frames are a camera's bytes
    with pytest.raises(ValueError, match='rank'):
        sensor.encrypt_to_frames(good[0])
    with pytest.raises(ValueError, match='layout'):
        sensor.encrypt_to_frames(good, layout='nhwc')
    with pytest.raises(ValueError, match='do not fit the sensor'):
        sensor.encrypt_to_frames(torch.zeros((2, 28, 27, 1), dtype=torch.uint8))
    with pytest.raises(ValueError, match='depth'):
        sensor.encrypt_to_frames(good, depth=12)
    for bad in ((1.0,), (3.0, 3.0), (5.0, 1.0), (0.0, float('inf')), 'ab', 7, (0.0, 1.0, 2.0)):
        with pytest.raises(ValueError, match='range'):
            sensor.encrypt_to_frames(good, range=bad)
    (lo, hi) = (torch.zeros(2), torch.ones(2))
    with pytest.raises(ValueError, match='uint8 or torch.uint16'):
        sensor.decrypt_from_frames(good.float(), lo, hi)
    with pytest.raises(ValueError, match='rank'):
        sensor.decrypt_from_frames(good[0], lo, hi)
    with pytest.raises(ValueError, match='layout'):
        sensor.decrypt_from_frames(good, lo, hi, layout='HWC')
    with pytest.raises(ValueError, match='do not fit the sensor'):
        sensor.decrypt_from_frames(good, lo, hi, layout='NCHW')
    with pytest.raises(ValueError, match='lo must be'):
        sensor.decrypt_from_frames(good, torch.zeros(3), hi)
    with pytest.raises(ValueError, match='hi must be'):
        sensor.decrypt_from_frames(good, lo, np.ones(2, np.float32))
    with pytest.raises(ValueError, match='on the device'):
        sensor.decrypt_from_frames(good, lo, hi)                         # host frames
    assert sensor._tensor is None


def test_forward_frames_refuses_before_the_gpu(no_gpu_call, lenet):
    (_, model) = lenet
    assert model.frame_shape() == (1, 28, 28) and model.frames_pad_to() == 1
    for dtype in (torch.uint8, torch.uint16):
        good = torch.zeros((2, 28, 28, 1), dtype=dtype)
        (lo, hi) = (torch.zeros(2), torch.ones(2))
        with pytest.raises(ValueError, match='uint8 or torch.uint16'):
            model.forward_frames(good.float(), lo, hi)
        with pytest.raises(ValueError, match='rank'):
            model.forward_frames(good[0], lo, hi)
        with pytest.raises(ValueError, match='layout'):
            model.forward_frames(good, lo, hi, layout='HWC')
        with pytest.raises(ValueError, match='do not fit the key-net'):
            model.forward_frames(torch.zeros((2, 28, 27, 1), dtype=dtype), lo, hi)
        with pytest.raises(ValueError, match='do not fit the key-net'):
            model.forward_frames(good, lo, hi, layout='NCHW')
        with pytest.raises(ValueError, match='lo must be'):
            model.forward_frames(good, torch.zeros(3), hi)
        with pytest.raises(ValueError, match='lo must be'):
            model.forward_frames(good, lo.double(), hi)
        with pytest.raises(ValueError, match='hi must be'):
            model.forward_frames(good, lo, [1.0, 1.0])
        with pytest.raises(ValueError, match='on the device'):
            model.forward_frames(good, lo, hi)


def test_entry_points_refuse_without_a_device():
    """Shape, depth, alignment and NULL refusals come back as codes before anything touches a device (the style of tests/test_egress_host.py)."""
    L = _capi.lib()
    (img, out, x, odd) = (ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(12288), ctypes.c_void_p(4097))    # never dereferenced: every call is refused
    (INVALID, SHAPE, UNSUPPORTED) = (1, 2, 6)
    for depth in (8, 16):
        assert L.kn_frames_to_linear(img, depth, 0, 3, 5, 7, 1, None, None, out, 4, 4, None) == SHAPE       # n = 0
        assert L.kn_frames_to_linear(img, depth, 5, 3, 5, 7, 1, None, None, out, 4, 4, None) == SHAPE       # n > n_cols
        assert L.kn_frames_to_linear(img, depth, 2, 3, 5, 7, 1, None, None, out, 3, 4, None) == SHAPE       # n_cols > ldo
        assert L.kn_frames_to_linear(img, depth, 2, 3, 0, 7, 1, None, None, out, 4, 4, None) == SHAPE       # h = 0
        assert L.kn_frames_to_linear(img, depth, 2, 3, 5, 7, 2, None, None, out, 4, 4, None) == INVALID     # no such layout
        assert L.kn_frames_to_linear(None, depth, 2, 3, 5, 7, 1, None, None, out, 4, 4, None) == INVALID
        assert L.kn_frames_to_linear(img, depth, 2, 3, 5, 7, 1, None, None, None, 4, 4, None) == INVALID
    for depth in (12, 0, 32, -8):
        assert L.kn_frames_to_linear(img, depth, 2, 3, 5, 7, 1, None, None, out, 4, 4, None) == UNSUPPORTED
    assert L.kn_frames_to_linear(odd, 16, 2, 3, 5, 7, 1, None, None, out, 4, 4, None) == INVALID            # a 16-bit base that is not 2-byte aligned
    assert len(L.kn_last_error()) > 0
    assert L.kn_linear_to_u16(x, 4, 0, 3, 5, 7, 1, None, None, img, None) == SHAPE                          # n = 0
    assert L.kn_linear_to_u16(x, 4, 5, 3, 5, 7, 1, None, None, img, None) == SHAPE                          # n > ldx
    assert L.kn_linear_to_u16(x, 4, 4, 3, 5, 0, 0, None, None, img, None) == SHAPE                          # w = 0
    assert L.kn_linear_to_u16(x, 4, 4, 3, 5, 7, 2, None, None, img, None) == INVALID
    assert L.kn_linear_to_u16(None, 4, 4, 3, 5, 7, 1, None, None, img, None) == INVALID
    assert L.kn_linear_to_u16(x, 4, 4, 3, 5, 7, 1, None, None, None, None) == INVALID
    assert L.kn_linear_to_u16(x, 4, 4, 3, 5, 7, 1, None, None, odd, None) == INVALID
    assert len(L.kn_last_error()) > 0


def test_header_declares_and_capi_binds_the_cipher_frames():
    src = open(os.path.join(ROOT, 'include', 'keynet_hip.h')).read()
    ingest = re.search(r'int kn_frames_to_linear\(const void\* img_dev, int depth, int64_t n, int64_t c, int64_t h, int64_t w, int layout,\s*'
                       r'const float\* scale_dev, const float\* offset_dev,\s*float\* out_dev, int64_t ldo, int64_t n_cols, void\* stream\);', src)
    egress = re.search(r'int kn_linear_to_u16\(const float\* x_dev, int64_t ldx, int64_t n, int64_t c, int64_t h, int64_t w, int layout,\s*'
                       r'const float\* gain_dev, const float\* bias_dev, uint16_t\* img_dev, void\* stream\);', src)
    assert ingest and egress, 'include/keynet_hip.h does not declare the two entry points as specified'
    comment = src[:ingest.start()].rsplit('/*', 1)[1]
    for line in ('one IEEE f32 multiply', 'never fused', 'KN_ERR_UNSUPPORTED', 'it is NOT', 'bit-equal to kn_u8_to_linear', 'HIP graph', '64 bits'):
        assert line in comment, line
    comment = src[:egress.start()].rsplit('/*', 1)[1]
    for line in ('one IEEE f32 multiply', 'never fused', 'ties to even', '65535'):
        assert line in comment, line
    assert re.search(r'#define KN_ABI_VERSION 5\b', src) and _capi.KN_ABI_VERSION == 5          # added entry points leave the version where it is
    flags = sorted(set(re.findall(r'\bKN_FLAG_[A-Z0-9_]+', src)))
    assert not [f for f in flags if 'U16' in f or 'FRAMES' in f or 'CIPHER' in f or 'DEPTH' in f]
    for name in ('kn_frames_to_linear', 'kn_linear_to_u16'):
        assert name in _capi.SYMBOLS
    assert callable(_capi.frames_to_linear) and callable(_capi.linear_to_u16)
    L = _capi.lib()
    assert len(L.kn_frames_to_linear.argtypes) == 13 and len(L.kn_linear_to_u16.argtypes) == 11


def test_streamed_forward_cipher_kinds(lenet):
    (sensor, model) = lenet
    assert kstream.FRAME_KINDS == ('uint8', 'float32', 'cipher8', 'cipher16')
    for kind in ('uint8', 'float32'):
        with pytest.raises(ValueError, match='sensor'):
            StreamedForward(None, model, 4, frames=kind)
    for kind in ('cipher', 'cipher12', 'uint16', 'float16'):
        with pytest.raises(ValueError, match='frames'):
            StreamedForward(None, model, 4, frames=kind)
    with pytest.raises(ValueError, match='layout'):
        StreamedForward(None, model, 4, frames='cipher8', layout='CHW')
    with pytest.raises(ValueError, match='batch'):
        StreamedForward(None, model, 0, frames='cipher16')
    for (kind, dtype, other) in (('cipher8', np.uint8, np.uint16), ('cipher16', np.uint16, np.uint8)):
        good = np.zeros((4, 28, 28, 1), dtype=dtype)
        (lo, hi) = (np.zeros(4, np.float32), np.ones(4, np.float32))
        for (bad, what) in ((good, 'frames, lo, hi'), ((good, lo), 'frames, lo, hi'), ((good.astype(other), lo, hi), 'frames must be'), ((good[0], lo, hi), 'rank'),
                            ((np.zeros((4, 28, 27, 1), dtype), lo, hi), 'do not fit the key-net'), ((good, lo[:3], hi), 'lo must be'),
                            ((good, lo, hi.astype(np.float64)), 'hi must be'),
                            ((np.zeros((5, 28, 28, 1), dtype), np.zeros(5, np.float32), np.ones(5, np.float32)), 'built for 4')):
            for s in (None, sensor):
                sf = StreamedForward(s, model, 4, frames=kind)
                assert sf._frame == (28, 28, 1) and sf._pad_to == 1
                with pytest.raises(ValueError, match=what):
                    next(sf.run([bad]))
                assert sf._buffers is None                               # nothing was allocated: no stream, no pinned buffer, no device memory
                sf.close()


def test_cipher_pad_to_follows_the_path():
    from benchlegs.workloads import build_workload
    (_, vm, (C, H, W)) = build_workload('vgg16-slice', 0)[:3]
    assert vm.frames_pad_to() == vm.BATCH_TILE and vm.frames_pad_to(narrow=True) == 1
    assert StreamedForward(None, vm, 4, frames='cipher8')._pad_to == vm.BATCH_TILE
    assert StreamedForward(None, vm, 4, frames='cipher16', narrow=True, narrow_rows=True)._pad_to == 1
    assert StreamedForward(None, vm, 4, frames='cipher8')._frame == (H, W, C)
