"""kn_linear_to_u8 and kn_column_range on the device against their statements (tests/test_egress_host.py's linear_to_u8_rule; np.nanmin / np.nanmax), byte for byte and by
value, and KeyedSensor.decrypt_frames / asframes / save / load(file, imagekey) on top of them."""
import warnings

import numpy as np
import pytest
import scipy.sparse
import torch

from keynet_amd import _capi
from keynet_amd import system as ksys
from keynet_amd import torch as ktorch
from keynet_amd.models import LeNet_AvgPool
from test_egress_host import EDGES, GUARD, SENTINEL, frames_of, linear_to_u8_rule
from test_ingest_host import NAN_BITS

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 5, 7), (3, 17, 19), (4, 16, 16)]              # 1, 105, 969 and 1 024 positions: below, across and exactly four 256-position tiles
NS = [1, 3, 64, 65, 130]                                                 # both sides of the 64-image tile
SHAPE_IDS = ['x'.join(str(v) for v in s) for s in SHAPES]


def dev():
    return torch.device('cuda:0')


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _block(n, ldx, shape, seed):
    """[D + 1, ldx] float32: values around [0, 255] with many exact ties, the edge table first, NaN sentinels in the ones row and in the columns beyond n."""
    D = int(np.prod(shape))
    rng = np.random.RandomState(seed)
    v = (rng.rand(D, n) * 300.0 - 20.0).astype(np.float32)
    ties = rng.rand(D, n) < 0.25
    v[ties] = np.floor(v[ties]) + np.float32(0.5)
    edges = np.array([e[0] for e in EDGES], dtype=np.float32)
    flat = v.reshape(-1)
    k = min(len(edges), flat.size)
    flat[:k] = edges[:k]                                                 # along the first feature rows, across the images
    if D >= len(edges):
        v[:len(edges), n - 1] = edges                                   # and down the last image
    x = np.full((D + 1, ldx), NAN_BITS, dtype=np.uint32).view(np.float32)
    x[:D, :n] = v
    return x


def _affine(n):
    b = np.arange(n)
    gain = (0.5 + 0.37 * (b % 5) * (1 - 2 * (b % 2))).astype(np.float32)          # neighbours differ in size and sign
    bias = (3.25 * ((b + 1) % 4) - 2.0 + 100.0 * (b % 2)).astype(np.float32)
    return (gain, bias)


def _run_u8(x, ldx, n, shape, layout, gain, bias, x_off=0, img_off=0):
    """kn_linear_to_u8 on a sentinel-filled byte buffer; x_off floats / img_off bytes move the bases off their alignment.  Returns the buffer in the rule's form."""
    D = int(np.prod(shape))
    xd = torch.zeros(x.size + x_off, dtype=torch.float32, device=dev())
    xd[x_off:] = torch.as_tensor(x.reshape(-1)).to(dev())
    out = torch.full((GUARD + n * D + GUARD + img_off,), SENTINEL, dtype=torch.uint8, device=dev())
    gd = None if gain is None else torch.as_tensor(gain).to(dev())
    bd = None if bias is None else torch.as_tensor(bias).to(dev())
    _capi.linear_to_u8(xd.data_ptr() + 4 * x_off, ldx, n, shape[0], shape[1], shape[2], layout, None if gd is None else gd.data_ptr(), None if bd is None else bd.data_ptr(),
                       out.data_ptr() + GUARD + img_off, _stream())
    got = out.cpu().numpy()
    assert np.all(got[:img_off] == SENTINEL)
    return got[img_off:]


@pytest.mark.parametrize('layout', [0, 1], ids=['NCHW', 'NHWC'])
@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
def test_linear_to_u8_is_the_rule_byte_for_byte(shape, layout):
    """Every n, ldx in (n, n + 3: scalar loads), with gain / bias NULL and per image, of one frame shape and layout; the sentinel around the frames intact."""
    with torch.cuda.device(dev()):
        for n in NS:
            for ldx in (n, n + 3):
                x = _block(n, ldx, shape, seed=n + ldx)
                for (gain, bias) in ((None, None), _affine(n), (_affine(n)[0], None), (None, _affine(n)[1])):
                    got = _run_u8(x, ldx, n, shape, layout, gain, bias)
                    want = linear_to_u8_rule(x, ldx, n, shape, layout, gain, bias)
                    what = 'n=%d ldx=%d gain=%s bias=%s' % (n, ldx, gain is not None, bias is not None)
                    assert np.all(got[:GUARD] == SENTINEL) and np.all(got[-GUARD:] == SENTINEL), what + ': bytes outside the frames were written'
                    assert np.array_equal(got, want), what + ': %d bytes differ' % int((got != want).sum())


@pytest.mark.parametrize('layout', [0, 1], ids=['NCHW', 'NHWC'])
@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
def test_linear_to_u8_odd_base_addresses(shape, layout):
    """A block that starts one float into an allocation (scalar loads although ldx is a multiple of four) and frames that start one byte into one (byte stores
    although D is a multiple of four), each alone and together."""
    with torch.cuda.device(dev()):
        for n in (4, 68):
            x = _block(n, n, shape, seed=11 + n)
            (gain, bias) = _affine(n)
            want = linear_to_u8_rule(x, n, n, shape, layout, gain, bias)
            for (x_off, img_off) in ((1, 0), (0, 1), (1, 1), (0, 2)):
                got = _run_u8(x, n, n, shape, layout, gain, bias, x_off=x_off, img_off=img_off)
                assert np.array_equal(got, want), 'n=%d x_off=%d img_off=%d: %d bytes differ' % (n, x_off, img_off, int((got != want).sum()))


def test_edge_values_on_the_device():
    t = np.array([e[0] for e in EDGES], dtype=np.float32)
    want = np.array([e[1] for e in EDGES], dtype=np.uint8)
    shape = (1, 1, len(EDGES))
    with torch.cuda.device(dev()):
        got = _run_u8(t.reshape(-1, 1), 1, 1, shape, 0, None, None)
        assert np.array_equal(frames_of(got, 1, shape, 0).reshape(-1), want)
        got = _run_u8((t / 2).reshape(-1, 1), 1, 1, shape, 1, np.float32([2.0]), np.float32([0.0]))
        assert np.array_equal(frames_of(got, 1, shape, 1).reshape(-1), want)
        # multiply and add round separately: take x whose product 3 * x = P + d rounds to the float P with a residue d < -2^-20, and bias = 1.5 - P (exact):
        # the two roundings give P + (1.5 - P) = 1.5 -> 2; one fused rounding would give 1.5 + d, below the tie -> 1
        for k in range(1000):
            x = np.float32(333.0 + 0.37 * k)
            P = np.float32(np.float32(3.0) * x)
            d = 3.0 * float(x) - float(P)
            if d < -2.0 ** -20:
                break
        bias = np.float32(1.5 - float(P))
        assert d < -2.0 ** -20 and float(bias) == 1.5 - float(P) and float(P) + float(bias) == 1.5
        got = _run_u8(np.float32([[x]]), 1, 1, (1, 1, 1), 0, np.float32([3.0]), np.float32([bias]))
        assert frames_of(linear_to_u8_rule(np.float32([[x]]), 1, 1, (1, 1, 1), 0, [3.0], [bias]), 1, (1, 1, 1), 0).reshape(-1)[0] == 2 and got[GUARD] == 2


@pytest.mark.parametrize('args', [dict(n=0), dict(n=9), dict(c=0), dict(h=0), dict(w=0)], ids=lambda a: '%s=%d' % next(iter(a.items())))
def test_linear_to_u8_refuses_and_launches_nothing(args):
    a = dict(n=4, c=3, h=5, w=7, ldx=8)
    a.update(args)
    with torch.cuda.device(dev()):
        x = torch.zeros((3 * 5 * 7 + 1, 8), device=dev())
        out = torch.full((8 * 3 * 5 * 7,), SENTINEL, dtype=torch.uint8, device=dev())
        rc = _capi.lib().kn_linear_to_u8(x.data_ptr(), a['ldx'], a['n'], a['c'], a['h'], a['w'], 1, None, None, out.data_ptr(), _stream())
        assert rc == 2, (rc, _capi.lib().kn_last_error())                                     # KN_ERR_SHAPE
        with pytest.raises(_capi.KeynetHipError):
            _capi.linear_to_u8(x.data_ptr(), a['ldx'], a['n'], a['c'], a['h'], a['w'], 1, None, None, out.data_ptr(), _stream())
        assert np.all(out.cpu().numpy() == SENTINEL)


@pytest.mark.parametrize('layout', [0, 1], ids=['NCHW', 'NHWC'])
@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
def test_round_trip_with_the_ingest(shape, layout):
    (C, H, W) = shape
    with torch.cuda.device(dev()):
        for n in NS:
            rng = np.random.RandomState(n)
            frames = torch.as_tensor(rng.randint(0, 256, size=(n, C, H, W) if layout == 0 else (n, H, W, C)).astype(np.uint8)).to(dev())
            name = ktorch.LAYOUTS[layout]
            for pad_to in (1, 4):
                x = ktorch.frames_to_linear(frames, layout=name, pad_to=pad_to)
                assert torch.equal(ktorch.linear_to_frames(x[:n] if pad_to == 1 else x, shape, layout=name)[:n], frames), 'n=%d pad_to=%d' % (n, pad_to)
            back = ktorch.linear_to_frames(x[:n], shape, layout=name)           # rows of a wider block: not a transposed view of a dense one, goes through a copy
            assert back.shape == frames.shape and torch.equal(back, frames)
            other = ktorch.linear_to_frames(x, shape, layout=ktorch.LAYOUTS[1 - layout])[:n]
            assert torch.equal(other, frames.permute(0, 2, 3, 1) if layout == 0 else frames.permute(0, 3, 1, 2))


# ---- kn_column_range
KINDS = 8


def _columns(rows, n_vecs, ld, seed):
    """[rows, ld] float32; column b is of kind (b + rows) % KINDS, its magnitude 10^((b % 7) - 3): neighbours differ by orders of magnitude."""
    rng = np.random.RandomState(seed)
    x = np.full((rows, ld), NAN_BITS, dtype=np.uint32).view(np.float32)
    v = (rng.randn(rows, n_vecs) * (10.0 ** ((np.arange(n_vecs) % 7) - 3))[None, :]).astype(np.float32)
    for b in range(n_vecs):
        kind = (b + rows) % KINDS
        if kind == 1:
            v[rng.rand(rows) < 0.3, b] = np.nan                          # NaN among the values (perhaps every one of a short column)
        elif kind == 2:
            v[rng.randint(rows), b] = np.inf
        elif kind == 3:
            v[rng.randint(rows), b] = -np.inf
            v[0, b] = np.nan
        elif kind == 4:
            v[:, b] = np.nan                                             # nothing to compare
        elif kind == 5:
            v[:, b] = np.float32(-7.25)                                  # constant
        elif kind == 6:
            v[:, b] = np.where(rng.rand(rows) < 0.5, np.float32(0.0), np.float32(-0.0))          # both zeros
        elif kind == 7:
            v[:, b] = -np.abs(v[:, b]) - np.float32(1e-30)              # all negative: the maximum is the value nearest to zero
    x[:, :n_vecs] = v
    return x


def _nan_range(v):
    """np.nanmin / np.nanmax down the columns; a column with no number gives (+Inf, -Inf), as the header states."""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        (lo, hi) = (np.nanmin(v, axis=0), np.nanmax(v, axis=0))
    empty = np.isnan(v).all(axis=0)
    return (np.where(empty, np.float32(np.inf), lo).astype(np.float32), np.where(empty, np.float32(-np.inf), hi).astype(np.float32))


@pytest.mark.parametrize('rows', [1, 63, 64, 65, 1000, 70001])
def test_column_range_is_nanmin_nanmax(rows):
    with torch.cuda.device(dev()):
        for n_vecs in NS:
            for ld in (n_vecs + 3, (n_vecs + 7) // 4 * 4):                  # scalar loads; a multiple of four beyond n_vecs: 16-byte loads, scalars in the quad across n_vecs
                x = _columns(rows, n_vecs, ld, seed=rows + n_vecs)
                xd = torch.as_tensor(x).to(dev())
                lo = torch.as_tensor(np.full(n_vecs + 4, NAN_BITS, dtype=np.uint32).view(np.float32)).to(dev())
                hi = lo.clone()
                _capi.column_range(xd.data_ptr(), rows, ld, n_vecs, lo.data_ptr() + 8, hi.data_ptr() + 8, _stream())
                (got_lo, got_hi) = (lo.cpu().numpy(), hi.cpu().numpy())
                (want_lo, want_hi) = _nan_range(x[:, :n_vecs])
                what = 'rows=%d n_vecs=%d ld=%d' % (rows, n_vecs, ld)
                for got in (got_lo, got_hi):
                    assert np.all(got[:2].view(np.uint32) == NAN_BITS) and np.all(got[2 + n_vecs:].view(np.uint32) == NAN_BITS), what + ': outputs outside [0, n_vecs) were written'
                assert np.array_equal(got_lo[2:2 + n_vecs], want_lo), what                          # by value: -0.0 == +0.0
                assert np.array_equal(got_hi[2:2 + n_vecs], want_hi), what
                # a second call into the same outputs, its ranges inside the first one's: the call initialises lo / hi itself
                x2 = x.copy()
                x2[:, :n_vecs] *= np.float32(0.25)
                xd.copy_(torch.as_tensor(x2).to(dev()))
                _capi.column_range(xd.data_ptr(), rows, ld, n_vecs, lo.data_ptr() + 8, hi.data_ptr() + 8, _stream())
                (want_lo, want_hi) = _nan_range(x2[:, :n_vecs])
                assert np.array_equal(lo.cpu().numpy()[2:2 + n_vecs], want_lo) and np.array_equal(hi.cpu().numpy()[2:2 + n_vecs], want_hi), what + ': second call'


def test_column_range_of_a_block_leaves_the_ones_row_out():
    with torch.cuda.device(dev()):
        frames = torch.as_tensor(np.random.RandomState(0).randint(2, 200, size=(5, 6, 7, 3)).astype(np.uint8)).to(dev())
        x = ktorch.frames_to_linear(frames)
        (lo, hi) = ktorch.column_range(x)
        flat = frames.reshape(5, -1).float()
        assert torch.equal(lo, flat.min(dim=1).values) and torch.equal(hi, flat.max(dim=1).values) and float(lo.min()) >= 2.0          # the 1.0 of the ones row is not in it


# ---- the sensor
def _sensors():
    torch.manual_seed(0)
    np.random.seed(0)
    lenet = ksys.PermutationKeynet((1, 28, 28), LeNet_AvgPool().eval())[0]
    np.random.seed(1)
    small = ksys.Keynet((3, 8, 8), None, global_geometric='permutation')[0]
    return ((lenet, (1, 28, 28)), (small, (3, 8, 8)))


def _gain_sensor():
    np.random.seed(1)
    return ksys.Keynet((3, 8, 8), None, global_geometric='permutation', global_photometric='uniform_random_gain', beta=0.5)[0]


@pytest.fixture(scope='module')
def sensors():
    return _sensors()


def _camera(n, shape, seed):
    (C, H, W) = shape
    return torch.as_tensor(np.random.RandomState(seed).randint(0, 256, size=(n, H, W, C)).astype(np.uint8))


def _round_trip(sensor, shape):
    with torch.cuda.device(dev()):
        for n in (1, 5, 70):
            f = _camera(n, shape, seed=n)
            for (layout, frames) in (('NHWC', f), ('NCHW', f.permute(0, 3, 1, 2).contiguous())):
                for pad_to in (1, 128):
                    xc = sensor.encrypt_frames(frames.to(dev()), layout=layout, pad_to=pad_to)
                    back = sensor.decrypt_frames(xc, layout=layout)
                    assert back.dtype == torch.uint8 and back.is_cuda and tuple(back.shape) == (xc.shape[0],) + tuple(frames.shape[1:])
                    assert torch.equal(back[:n].cpu(), frames), 'n=%d %s pad_to=%d' % (n, layout, pad_to)
                    assert not back[n:].any(), 'the zero images did not come back as zero frames'
    assert sensor._tensor is None                                        # stateless


@pytest.mark.parametrize('which', [0, 1], ids=['lenet', '3x8x8'])
def test_decrypt_frames_inverts_encrypt_frames_under_a_permutation_key(sensors, which):
    _round_trip(*sensors[which])


def test_decrypt_frames_inverts_encrypt_frames_under_a_gain_key():
    (sensor, shape) = (_gain_sensor(), (3, 8, 8))
    # the premise, on the host with scipy: the decrypt error of this key family on camera frames stays far below one half
    (E, Dk) = (scipy.sparse.csr_matrix(k).astype(np.float32) for k in sensor.keypair())
    for n in (1, 5, 70):
        f = _camera(n, shape, seed=n).permute(0, 3, 1, 2).reshape(n, -1).numpy().astype(np.float32)
        x = np.concatenate((f, np.ones((n, 1), np.float32)), axis=1).T
        err = float(np.abs(Dk.dot(E.dot(x).astype(np.float32)).astype(np.float32)[:-1] - x[:-1]).max())
        assert err < 0.25, 'the premise fails, not the kernel: decrypt error %g' % err
    _round_trip(sensor, shape)


@pytest.mark.parametrize('which', [0, 1], ids=['lenet', '3x8x8'])
def test_asframes_of_an_encrypted_batch(sensors, which):
    (sensor, shape) = sensors[which]
    (n, D) = (7, int(np.prod(shape)))
    x = _camera(n, shape, seed=3).permute(0, 3, 1, 2).float()
    x[2] = 17.0                                                          # a constant image (its permutation-keyed image is constant too)
    try:
        with torch.cuda.device(dev()):
            xc = sensor.fromtensor(x.to(dev())).encrypt().astensor()
            xh = xc.cpu().numpy()
            for layout in (0, 1):
                (frames, gain, bias) = sensor.asframes(ktorch.LAYOUTS[layout])
                assert frames.is_cuda and frames.dtype == torch.uint8 and gain.is_cuda and tuple(gain.shape) == (n,) and tuple(bias.shape) == (n,)
                (g, b) = (gain.cpu().numpy(), bias.cpu().numpy())
                (lo, hi) = (xh[:, :D].min(axis=1), xh[:, :D].max(axis=1))
                (wg, wb) = ktorch.gray_affine(torch.as_tensor(lo), torch.as_tensor(hi))
                assert np.allclose(g, wg.numpy(), rtol=1e-6, atol=0) and np.allclose(b, wb.numpy(), rtol=1e-6, atol=0)      # (a division and a product: an ulp each way)
                want = frames_of(linear_to_u8_rule(np.ascontiguousarray(xh.T), n, n, shape, layout, g, b), n, shape, layout)
                got = frames.cpu().numpy()
                assert np.array_equal(got, want)
                for i in range(n):
                    if lo[i] == hi[i]:
                        assert g[i] == 0 and b[i] == 0 and not got[i].any()                      # constant: black
                    else:
                        assert got[i].min() == 0 and got[i].max() == 255
                assert lo[2] == hi[2]
            # un-encrypted: homogenised first, the same gray mapping of the plain images
            (plain, g2, b2) = sensor.fromtensor(x).asframes('NCHW')
            (wg, wb) = ktorch.gray_affine(x.reshape(n, -1).min(dim=1).values, x.reshape(n, -1).max(dim=1).values)
            (g2, b2) = (g2.cpu().numpy(), b2.cpu().numpy())
            assert np.allclose(g2, wg.numpy(), rtol=1e-6, atol=0) and np.allclose(b2, wb.numpy(), rtol=1e-6, atol=0) and g2[2] == 0 and b2[2] == 0
            xl = np.ascontiguousarray(x.reshape(n, -1).numpy().T)
            assert np.array_equal(plain.cpu().numpy(), frames_of(linear_to_u8_rule(xl, n, n, shape, 0, g2, b2), n, shape, 0))
    finally:
        sensor._tensor = None


@pytest.mark.parametrize('which', [0, 1], ids=['lenet', '3x8x8'])
def test_save_then_load_with_the_image_key(sensors, which, tmp_path):
    from PIL import Image
    (sensor, shape) = sensors[which]
    D = int(np.prod(shape))
    x = (torch.as_tensor(np.random.RandomState(5).rand(1, *shape).astype(np.float32)) * 255.0)
    try:
        with torch.cuda.device(dev()):
            sensor.fromtensor(x).encrypt()
            xc = sensor.astensor().cpu().numpy()
            (lo, hi) = (float(xc[0, :D].min()), float(xc[0, :D].max()))
            im = sensor.asimage()
            assert im.mode == ('L' if shape[0] == 1 else 'RGB') and im.size == (shape[2], shape[1]) and sensor.toimage().tobytes() == im.tobytes()
            (f, key) = sensor.save(str(tmp_path / 'cipher.png'))
            assert sensor.isencrypted()
            stored = Image.open(f)
            assert stored.mode == im.mode and stored.tobytes() == im.tobytes()
            back = sensor.load(f, key).astensor()
            assert tuple(back.shape) == (1,) + tuple(shape) and not sensor.isencrypted()
            bound = (hi - lo) / 510.0 + 2.0 ** -12 * max(1.0, abs(hi), abs(lo))
            err = float((back.cpu().double() - x.double()).abs().max())
            print('save/load: error %g, bound %g' % (err, bound))
            assert err <= bound, (err, bound)
            # without a key: today's path, unchanged (read, convert, bilinear resize to the sensor, [0, 255] floats)
            plain = np.random.RandomState(6).randint(0, 256, size=(shape[1] + 3, shape[2] + 5, 3)).astype(np.uint8)
            Image.fromarray(plain, 'RGB').save(str(tmp_path / 'plain.png'))
            got = sensor.load(str(tmp_path / 'plain.png')).astensor()
            a = np.asarray(Image.open(str(tmp_path / 'plain.png')).convert('L' if shape[0] == 1 else 'RGB').resize((shape[2], shape[1]), Image.BILINEAR), dtype=np.float32)
            a = a.reshape(shape[1], shape[2], 1) if a.ndim == 2 else a
            assert got.dtype == torch.float32 and tuple(got.shape) == (1,) + tuple(shape) and np.array_equal(got.numpy()[0], a.transpose(2, 0, 1))
    finally:
        sensor._tensor = None


def test_range_and_conversion_replay_from_a_graph():
    """kn_column_range and kn_linear_to_u8 allocate nothing and wait for nothing: captured once, replayed on new inputs, the bytes are the eager ones."""
    shape = (3, 17, 19)
    (n, D) = (70, int(np.prod(shape)))
    with torch.cuda.device(dev()):
        g = torch.Generator(device=dev()).manual_seed(0)
        block = torch.empty((D + 1, n), device=dev())
        x = block.t()
        lo = torch.empty(n, device=dev())
        hi = torch.empty(n, device=dev())
        gain = torch.empty(n, device=dev())
        bias = torch.empty(n, device=dev())
        out = torch.empty((n, shape[1], shape[2], shape[0]), dtype=torch.uint8, device=dev())

        def work():
            _capi.column_range(block.data_ptr(), D, n, n, lo.data_ptr(), hi.data_ptr(), _stream())
            (gn, bs) = ktorch.gray_affine(lo, hi)
            gain.copy_(gn)
            bias.copy_(bs)
            _capi.linear_to_u8(block.data_ptr(), n, n, shape[0], shape[1], shape[2], 1, gain.data_ptr(), bias.data_ptr(), out.data_ptr(), _stream())

        block.copy_(torch.randn((D + 1, n), generator=g, device=dev()))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            work()                                                       # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            work()
        for k in range(3):
            block.copy_(torch.randn((D + 1, n), generator=g, device=dev()) * (10.0 ** k) + k)
            graph.replay()
            torch.cuda.synchronize()
            got = out.clone()
            (wlo, whi) = ktorch.column_range(x)
            (wg, wb) = ktorch.gray_affine(wlo, whi)
            assert torch.equal(lo, wlo) and torch.equal(hi, whi)
            want = ktorch.linear_to_frames(x, shape, gain=wg, bias=wb)
            assert torch.equal(got, want) and int(got.max()) == 255 and int(got.min()) == 0, 'replay %d' % k
