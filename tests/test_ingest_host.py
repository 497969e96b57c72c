"""The ingest of host frames, host side (no GPU): the layout rule of kn_u8_to_linear as a numpy statement, the argument checks of frames_to_linear,
KeyedSensor.encrypt_frames and StreamedForward (each raised before any GPU call), and the C ABI entry."""
import os
import re

import numpy as np
import pytest
import torch

from keynet_amd import _capi
from keynet_amd import system as ksys
from keynet_amd.models import LeNet_AvgPool
from keynet_amd.stream import StreamedForward
from keynet_amd.torch import frames_to_linear

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_BITS = 0x7FC00BAD            # the sentinel of the GPU tests: a quiet NaN with a payload nothing computes


def u8_to_linear_rule(img, layout, n_cols, ldo):
    """include/keynet_hip.h's statement of kn_u8_to_linear on a sentinel-filled [D + 1, ldo] block: img is [n, C, H, W] (layout 0) or [n, H, W, C] (layout 1) uint8."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 4 and layout in (0, 1)
    (n, c, h, w) = img.shape if layout == 0 else (img.shape[0], img.shape[3], img.shape[1], img.shape[2])
    D = c * h * w
    out = np.full((D + 1, ldo), NAN_BITS, dtype=np.uint32).view(np.float32)
    out[:, n:n_cols] = np.float32(0.0)
    out[D, :n] = np.float32(1.0)
    for b in range(n):
        for ch in range(c):
            plane = img[b, ch] if layout == 0 else img[b, :, :, ch]
            out[ch * h * w:(ch + 1) * h * w, b] = plane.reshape(h * w).astype(np.float32)
    return out


@pytest.mark.parametrize('shape', [(1, 5, 7), (3, 9, 11), (3, 32, 32)])
def test_rule_is_affine_to_linear_of_the_float_frames(shape):
    (C, H, W) = shape
    (n, D) = (5, C * H * W)
    rng = np.random.RandomState(0)
    x = torch.as_tensor(rng.randint(0, 256, size=(n, H, W, C)).astype(np.uint8))
    want = torch.cat((x.permute(0, 3, 1, 2).reshape(n, D).float(), torch.ones(n, 1)), 1).numpy()
    nhwc = u8_to_linear_rule(x.numpy(), 1, n + 3, n + 4)
    nchw = u8_to_linear_rule(np.ascontiguousarray(x.permute(0, 3, 1, 2).numpy()), 0, n + 3, n + 4)
    for got in (nhwc, nchw):
        assert np.array_equal(got[:, :n].T, want)
        assert np.array_equal(got[:, n:n + 3].view(np.uint32), np.zeros((D + 1, 3), np.uint32))            # +0.0, the ones row included
        assert np.all(got[:, n + 3:].view(np.uint32) == NAN_BITS)


def _lenet():
    torch.manual_seed(0)
    np.random.seed(0)
    return ksys.PermutationKeynet((1, 28, 28), LeNet_AvgPool().eval())


@pytest.fixture(scope='module')
def lenet():
    return _lenet()


def test_frames_to_linear_refuses_before_the_gpu():
    good = torch.zeros((2, 28, 28, 1), dtype=torch.uint8)
    with pytest.raises(ValueError, match='uint8'):
        frames_to_linear(good.float())
    with pytest.raises(ValueError, match='rank'):
        frames_to_linear(good[0])
    with pytest.raises(ValueError, match='layout'):
        frames_to_linear(good, layout='HWC')
    with pytest.raises(ValueError, match='pad_to'):
        frames_to_linear(good, pad_to=0)


def test_encrypt_frames_refuses_before_the_gpu(lenet):
    (sensor, _) = lenet
    good = torch.zeros((2, 28, 28, 1), dtype=torch.uint8)
    with pytest.raises(ValueError, match='uint8'):
        sensor.encrypt_frames(good.float())
    with pytest.raises(ValueError, match='rank'):
        sensor.encrypt_frames(good[0])
    with pytest.raises(ValueError, match='layout'):
        sensor.encrypt_frames(good, layout='nhwc')
    with pytest.raises(ValueError, match='do not fit the sensor'):
        sensor.encrypt_frames(torch.zeros((2, 28, 27, 1), dtype=torch.uint8))
    with pytest.raises(ValueError, match='do not fit the sensor'):
        sensor.encrypt_frames(good, layout='NCHW')                       # [2, 28, 28, 1] read as C = 28
    assert sensor._tensor is None


def test_streamed_forward_refuses_before_the_gpu(lenet):
    (sensor, model) = lenet
    with pytest.raises(ValueError, match='layout'):
        StreamedForward(sensor, model, 4, layout='CHW')
    with pytest.raises(ValueError, match='frames'):
        StreamedForward(sensor, model, 4, frames='float16')
    with pytest.raises(ValueError, match='batch'):
        StreamedForward(sensor, model, 0)
    good = np.zeros((4, 28, 28, 1), dtype=np.uint8)
    for (bad, what) in ((good.astype(np.float32), 'uint8'), (good[0], 'rank'), (np.zeros((4, 28, 27, 1), np.uint8), 'do not fit the sensor'),
                        (np.zeros((5, 28, 28, 1), np.uint8), 'built for 4')):
        sf = StreamedForward(sensor, model, 4)
        with pytest.raises(ValueError, match=what):
            next(sf.run([bad]))
        assert sf._buffers is None                                       # nothing was allocated: no stream, no pinned buffer, no device memory
        sf.close()
    sf = StreamedForward(sensor, model, 4, frames='float32')
    with pytest.raises(ValueError, match='float32'):
        next(sf.run([np.zeros((4, 1, 28, 28), np.uint8)]))
    with pytest.raises(ValueError, match='built for 4'):
        next(sf.run([torch.zeros((5, 1, 28, 28))]))
    sf.close()
    with pytest.raises(RuntimeError, match='closed'):
        sf.run([])


def test_pad_to_follows_the_path(lenet):
    """Whole BATCH_TILE tiles only where _prepare would pad: the wide path of a tiled-conv key-net."""
    (sensor, model) = lenet
    assert StreamedForward(sensor, model, 4)._pad_to == 1
    from benchlegs.workloads import build_workload
    (vs, vm) = build_workload('vgg16-slice', 0)[:2]
    assert StreamedForward(vs, vm, 4)._pad_to == vm.BATCH_TILE
    assert StreamedForward(vs, vm, 4, narrow=True, narrow_rows=True)._pad_to == 1


def test_header_declares_and_capi_binds_u8_to_linear():
    src = open(os.path.join(ROOT, 'include', 'keynet_hip.h')).read()
    decl = re.search(r'int kn_u8_to_linear\(const uint8_t\* img_dev, int64_t n, int64_t c, int64_t h, int64_t w, int layout,\s*float\* out_dev, int64_t ldo, int64_t n_cols, void\* stream\);', src)
    assert decl, 'include/keynet_hip.h does not declare kn_u8_to_linear as specified'
    comment = src[:decl.start()].rsplit('/*', 1)[1]
    assert 'keynet/system.py:183-201, 250-255' in comment and 'keynet/torch.py:65-68' in comment
    assert re.search(r'#define KN_ABI_VERSION 5\b', src) and _capi.KN_ABI_VERSION == 5          # an added entry point leaves the version where it is
    assert 'kn_u8_to_linear' in _capi.SYMBOLS and callable(_capi.u8_to_linear)
    fn = _capi.lib().kn_u8_to_linear
    assert len(fn.argtypes) == 10
