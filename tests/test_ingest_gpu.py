"""kn_u8_to_linear on the device against the numpy statement of its layout rule (tests/test_ingest_host.py), bit for bit, and KeyedSensor.encrypt_frames against
the sensor's existing encrypt."""
import ctypes

import numpy as np
import pytest
import torch

from keynet_amd import _capi
from keynet_amd import system as ksys
from keynet_amd.models import LeNet_AvgPool
from test_ingest_host import NAN_BITS, u8_to_linear_rule
from value_classes import assert_bits_equal

pytestmark = pytest.mark.gpu

SHAPES = [(1, 5, 7), (3, 9, 11), (3, 32, 32)]
NS = [1, 3, 64, 65, 130]


def dev():
    return torch.device('cuda:0')


def _frames(n, shape, layout, seed):
    """[n, C, H, W] (layout 0) or [n, H, W, C] (layout 1) bytes: every one of the 256 values first, random ones behind."""
    (C, H, W) = shape
    rng = np.random.RandomState(seed)
    flat = rng.randint(0, 256, size=n * C * H * W).astype(np.uint8)
    if flat.size >= 256:
        flat[:256] = rng.permutation(256).astype(np.uint8)
    return flat.reshape((n, C, H, W) if layout == 0 else (n, H, W, C))


def _sentinel(rows, ldo):
    return torch.as_tensor(np.full((rows, ldo), NAN_BITS, dtype=np.uint32).view(np.float32)).to(dev())


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize('layout', [0, 1], ids=['NCHW', 'NHWC'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_u8_to_linear_is_the_rule_bit_for_bit(shape, layout):
    """Every n, n_cols in (n, n + 1, the next multiple of 128) and ldo in (n_cols, n_cols + 3: scalar stores) of one frame shape and layout."""
    D = int(np.prod(shape))
    with torch.cuda.device(dev()):
        for n in NS:
            img = _frames(n, shape, layout, seed=n)
            if img.size >= 256:
                assert len(np.unique(img)) == 256
            img_d = torch.as_tensor(img).to(dev())
            for n_cols in (n, n + 1, -(-n // 128) * 128):
                for ldo in (n_cols, n_cols + 3):
                    out = _sentinel(D + 1, ldo)
                    _capi.u8_to_linear(img_d.data_ptr(), n, shape[0], shape[1], shape[2], layout, out.data_ptr(), ldo, n_cols, _stream())
                    got = out.cpu().numpy()
                    what = 'n=%d n_cols=%d ldo=%d' % (n, n_cols, ldo)
                    assert np.all(got[:, n_cols:].view(np.uint32) == NAN_BITS), what + ': columns beyond n_cols were written'
                    assert not got[:, n:n_cols].view(np.uint32).any(), what + ': a pad column is not +0.0 in every row'
                    assert np.all(got[D, :n].view(np.uint32) == np.float32(1.0).view(np.uint32)), what + ': the ones row'
                    ref = u8_to_linear_rule(img, layout, n_cols, ldo)
                    assert_bits_equal(got[:, :n_cols], ref[:, :n_cols], what)


def test_u8_to_linear_odd_base_addresses():
    """Frames that start one byte into an allocation (byte loads) and a block that starts one float into one (scalar stores)."""
    (shape, n, layout) = ((3, 32, 32), 5, 1)
    D = int(np.prod(shape))
    img = _frames(n, shape, layout, seed=7)
    with torch.cuda.device(dev()):
        buf = torch.zeros(img.size + 1, dtype=torch.uint8, device=dev())
        buf[1:] = torch.as_tensor(img.reshape(-1)).to(dev())
        out = _sentinel(D + 2, 8)
        _capi.u8_to_linear(buf.data_ptr() + 1, n, shape[0], shape[1], shape[2], layout, out.data_ptr() + 4, 8, 8, _stream())
        got = out.cpu().numpy().reshape(-1)
    assert got[:1].view(np.uint32)[0] == NAN_BITS and np.all(got[1 + (D + 1) * 8:].view(np.uint32) == NAN_BITS)
    assert_bits_equal(got[1:1 + (D + 1) * 8].reshape(D + 1, 8), u8_to_linear_rule(img, layout, 8, 8))


@pytest.mark.parametrize('args', [dict(n=0), dict(n_cols=3), dict(ldo=7), dict(c=0), dict(w=0)], ids=lambda a: '%s=%d' % next(iter(a.items())))
def test_u8_to_linear_refuses_and_launches_nothing(args):
    a = dict(n=4, c=3, h=9, w=11, n_cols=8, ldo=8)
    a.update(args)
    D = 3 * 9 * 11
    with torch.cuda.device(dev()):
        img_d = torch.as_tensor(_frames(4, (3, 9, 11), 1, seed=1)).to(dev())
        out = _sentinel(D + 1, 8)
        rc = _capi.lib().kn_u8_to_linear(img_d.data_ptr(), a['n'], a['c'], a['h'], a['w'], 1, out.data_ptr(), a['ldo'], a['n_cols'], _stream())
        assert rc == 2, (rc, _capi.lib().kn_last_error())                                     # KN_ERR_SHAPE
        with pytest.raises(_capi.KeynetHipError):
            _capi.u8_to_linear(img_d.data_ptr(), a['n'], a['c'], a['h'], a['w'], 1, out.data_ptr(), a['ldo'], a['n_cols'], _stream())
        assert np.all(out.cpu().numpy().view(np.uint32) == NAN_BITS)


def _sensors():
    torch.manual_seed(0)
    np.random.seed(0)
    perm = ksys.PermutationKeynet((1, 28, 28), LeNet_AvgPool().eval())[0]
    np.random.seed(1)
    gain = ksys.Keynet((3, 9, 11), None, global_geometric='permutation', global_photometric='uniform_random_gain', beta=0.5)[0]
    return (('permutation', perm, (1, 28, 28)), ('gain', gain, (3, 9, 11)))


@pytest.mark.parametrize('which', [0, 1], ids=['permutation', 'gain'])
def test_encrypt_frames_is_the_sensors_encrypt(which):
    (name, sensor, shape) = _sensors()[which]
    n = 5
    x = torch.as_tensor(_frames(n, shape, 1, seed=3))
    with torch.cuda.device(dev()):
        want = sensor.fromtensor(x.permute(0, 3, 1, 2).float()).encrypt().astensor().clone()
        held = sensor._tensor
        before = held.clone()
        for (layout, frames) in (('NHWC', x), ('NCHW', x.permute(0, 3, 1, 2).contiguous())):
            for pad_to in (1, 4):
                got = sensor.encrypt_frames(frames.to(dev()), layout=layout, pad_to=pad_to)
                n_cols = -(-n // pad_to) * pad_to
                assert got.is_cuda and tuple(got.shape) == (n_cols, int(np.prod(shape)) + 1) and got.t().is_contiguous()
                assert torch.equal(got[:n].cpu(), want.cpu()), '%s %s pad_to=%d' % (name, layout, pad_to)
                assert not got[n:].cpu().numpy().view(np.uint32).any(), 'the pad rows are not zero images'
        assert sensor._tensor is held and torch.equal(sensor._tensor, before)


def test_public_sensor_only_homogenises():
    shape = (3, 9, 11)
    x = torch.as_tensor(_frames(4, shape, 1, seed=5))
    sensor = ksys.PublicKeyedSensor(shape)
    with torch.cuda.device(dev()):
        got = sensor.encrypt_frames(x.to(dev())).cpu()
        want = sensor.fromtensor(x.permute(0, 3, 1, 2).float()).tensor().cpu()
    assert torch.equal(got, want)
    assert torch.equal(got, torch.cat((x.permute(0, 3, 1, 2).reshape(4, -1).float(), torch.ones(4, 1)), 1))
