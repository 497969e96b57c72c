"""Quantised encrypted frames on the device: kn_frames_to_linear and kn_linear_to_u16 against their numpy rules bit for bit (tests/test_cipher_frames_host.py), the
round trip of egress then ingest inside the host file's bound, the exact path on the permutation nets, the float-key comparison of 8 against 16 bits, and the two
cipher kinds of StreamedForward against KeyedModel.forward_frames.  The shapes are the smallest at which a path of the kernels changes: D odd, D even but no multiple of
four (crossing a position tile at either depth), whole dword frames; one image, a ragged quad, a full column tile, one beyond it, three tiles."""
import numpy as np
import pytest
import torch

from benchlegs.workloads import build_workload
from keynet_amd import _capi
from keynet_amd import system as ksys
from keynet_amd import torch as ktorch
from keynet_amd.models import LeNet_AvgPool
from keynet_amd.stream import StreamedForward
from test_cipher_frames_host import DTYPES, GUARD, LEVELS, SENTINEL16, frames16_of, frames_to_linear_rule, linear_to_u16_rule, random_ranges, roundtrip_bound
from test_ingest_host import NAN_BITS

pytestmark = pytest.mark.gpu

SHAPES = [(3, 5, 7), (2, 9, 15), (1, 28, 28), (3, 32, 32)]
COUNTS = [1, 3, 64, 65, 130]
TDTYPES = {8: torch.uint8, 16: torch.uint16}
SIZES = (6, 3, 6, 1, 6, 5, 2)            # the batch sizes of tests/test_stream_gpu.py
NARROW_SIZES = (4, 2, 4, 1, 4, 4, 3)
NARROW = dict(narrow=True, narrow_rows=True, narrow_taps='pairs')

_nets = {}


def dev():
    return torch.device('cuda:0')


def stream():
    return torch.cuda.current_stream().cuda_stream


def _net(name):
    if name not in _nets:
        (sensor, model, inshape) = build_workload(name, 0)[:3]
        _nets[name] = (sensor, model, tuple(inshape))
    return _nets[name]


def _bits(t):
    """A uint16 device or host tensor as numpy uint16 (through its int16 view: not every torch op takes uint16)."""
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _affines(rng, n, variant):
    """(scale, offset) over several binades, negative offsets, negative scales and a zero scale; variant 1: no scale, 2: no offset, 3: neither."""
    scale = (rng.choice([-1.0, 1.0], size=n) * 2.0 ** rng.uniform(-8, 8, size=n) * rng.uniform(1, 2, size=n)).astype(np.float32)
    offset = (rng.choice([-1.0, 1.0], size=n) * 2.0 ** rng.uniform(-6, 12, size=n) * rng.uniform(1, 2, size=n)).astype(np.float32)
    if n > 1:
        scale[n // 2] = 0.0
    return (None if variant in (1, 3) else scale, None if variant in (2, 3) else offset)


def _ingest(img, depth, layout, n_cols, ldo, scale, offset, out_off, img_off):
    """kn_frames_to_linear through raw pointers: the frames `img_off` elements into their buffer, the block `out_off` floats into a sentinel-filled one.  Returns the
    whole buffer as uint32: out_off sentinels, then [D + 1, ldo]."""
    (n, c, h, w) = img.shape if layout == 0 else (img.shape[0], img.shape[3], img.shape[1], img.shape[2])
    D = c * h * w
    raw = torch.zeros(n * D + img_off, dtype=torch.int16 if depth == 16 else torch.uint8, device=dev())
    flat = np.ascontiguousarray(img).reshape(-1)
    raw[img_off:].copy_(torch.as_tensor(flat.view(np.int16) if depth == 16 else flat))
    buf = torch.full((out_off + (D + 1) * ldo,), NAN_BITS, dtype=torch.int32, device=dev())
    (sc, of) = (None if v is None else torch.as_tensor(v).to(dev()) for v in (scale, offset))
    _capi.frames_to_linear(raw.data_ptr() + img_off * raw.element_size(), depth, n, c, h, w, layout, None if sc is None else sc.data_ptr(),
                           None if of is None else of.data_ptr(), buf.data_ptr() + 4 * out_off, ldo, n_cols, stream())
    return buf.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('layout', [0, 1], ids=['NCHW', 'NHWC'])
@pytest.mark.parametrize('depth', [8, 16])
def test_ingest_against_the_rule(depth, layout):
    rng = np.random.RandomState(10 * depth + layout)
    case = 0
    with torch.cuda.device(dev()):
        for (C, H, W) in SHAPES:
            for n in COUNTS:
                img = rng.randint(0, LEVELS[depth] + 1, size=(n, C, H, W) if layout == 0 else (n, H, W, C)).astype(DTYPES[depth])
                for n_cols in sorted(set((n, -(-n // 128) * 128))):
                    for ldo in (n_cols, n_cols + 3):
                        for (out_off, img_off) in ((0, 0), (1, 0), (0, 1)):                      # an output base one float on; a frame base one element on
                            case += 1
                            (scale, offset) = _affines(rng, n, case % 4)
                            got = _ingest(img, depth, layout, n_cols, ldo, scale, offset, out_off, img_off)
                            want = frames_to_linear_rule(img, layout, n_cols, ldo, scale, offset).view(np.uint32).reshape(-1)
                            what = 'depth %d layout %d (C, H, W) = %s n = %d n_cols = %d ldo = %d offsets (%d, %d) variant %d' % (
                                depth, layout, str((C, H, W)), n, n_cols, ldo, out_off, img_off, case % 4)
                            assert np.all(got[:out_off] == NAN_BITS), what
                            assert np.array_equal(got[out_off:], want), what                       # int32 views: pads +0.0, sentinels beyond n_cols, the ones row
    assert case == len(SHAPES) * len(COUNTS) * 2 * 2 * 3


@pytest.mark.parametrize('layout', ['NCHW', 'NHWC'])
def test_no_affine_at_8_bits_is_u8_to_linear(layout):
    rng = np.random.RandomState(5)
    with torch.cuda.device(dev()):
        for (C, H, W) in SHAPES:
            for n in (3, 65):
                f = torch.as_tensor(rng.randint(0, 256, size=(n, C, H, W) if layout == 'NCHW' else (n, H, W, C)).astype(np.uint8)).to(dev())
                want = ktorch.frames_to_linear(f, layout=layout, pad_to=4)
                got = torch.empty_like(want.t())
                _capi.frames_to_linear(f.data_ptr(), 8, n, C, H, W, ktorch.LAYOUTS.index(layout), None, None, got.data_ptr(), got.shape[1], got.shape[1], stream())
                assert torch.equal(got.view(torch.int32), want.t().contiguous().view(torch.int32))
                ones = torch.ones(n, device=dev())
                viaone = ktorch.frames_to_linear(f, layout=layout, pad_to=4, scale=ones)         # the Python route to the new entry point
                assert torch.equal(viaone.t().contiguous().view(torch.int32), want.t().contiguous().view(torch.int32))


def test_ingest_beyond_2_to_31_elements():
    """D = 3 * 224 * 224 rows of ldo = 16 384 floats: the last rows begin 2.4 G elements in.  Only 64 columns are written."""
    (C, H, W, n, ldo) = (3, 224, 224, 64, 16384)
    D = C * H * W
    with torch.cuda.device(dev()):
        if torch.cuda.mem_get_info()[0] < 12 * 2 ** 30:
            pytest.skip('less than 12 GB of device memory free')
        rng = np.random.RandomState(31)
        img = rng.randint(0, 65536, size=(n, H, W, C)).astype(np.uint16)
        (scale, offset) = _affines(rng, n, 0)
        f = torch.as_tensor(img.view(np.int16)).to(dev())
        (sc, of) = (torch.as_tensor(scale).to(dev()), torch.as_tensor(offset).to(dev()))
        block = torch.empty((D + 1) * ldo, dtype=torch.float32, device=dev())
        assert block.numel() > 2 ** 31
        rows = (0, D // 2, D - 1, D)
        for r in rows:
            block[r * ldo:r * ldo + n + 1].view(torch.int32).fill_(NAN_BITS)
        _capi.frames_to_linear(f.data_ptr(), 16, n, C, H, W, 1, sc.data_ptr(), of.data_ptr(), block.data_ptr(), ldo, n, stream())
        got = {r: block[r * ldo:r * ldo + n + 1].cpu().numpy().view(np.uint32) for r in rows}
        del block
    planes = img.transpose(0, 3, 1, 2).reshape(n, D)
    for r in rows:
        if r == D:
            want = np.ones(n, np.float32)
        else:
            want = ((scale * planes[:, r].astype(np.float32)).astype(np.float32) + offset).astype(np.float32)
        assert np.array_equal(got[r][:n], want.view(np.uint32)), 'row %d' % r
        assert got[r][n] == NAN_BITS                                     # column n_cols is not touched


def _special_block(rng, D, ldx):
    """[D, ldx] floats in and around [0, 65535] with exact ties, values beyond both ends, NaN and both infinities."""
    x = (rng.rand(D, ldx) * 70000.0 - 2000.0).astype(np.float32)
    ties = (rng.randint(0, 65536, size=(D, ldx)) + 0.5).astype(np.float32)
    x = np.where(rng.rand(D, ldx) < 0.3, ties, x)
    flat = x.reshape(-1)
    for (k, v) in enumerate((np.nan, np.inf, -np.inf, 65535.5, 65534.5, 70000.0, -0.0, 0.5, 1.5, 2.5, 1e30, -1e30)):
        flat[(k * 7919) % flat.size] = v
    return x


@pytest.mark.parametrize('layout', [0, 1], ids=['NCHW', 'NHWC'])
def test_egress16_against_the_rule(layout):
    rng = np.random.RandomState(160 + layout)
    case = 0
    with torch.cuda.device(dev()):
        for (C, H, W) in SHAPES:
            D = C * H * W
            for n in COUNTS:
                for ldx in (n, n + 3):
                    for (x_off, img_off) in ((0, 0), (1, 0), (0, 1)):                            # a block base one float on; a frame base one halfword on
                        case += 1
                        x = _special_block(rng, D, ldx)
                        variant = case % 4
                        gain = None if variant in (1, 3) else (2.0 ** rng.uniform(-2, 2, size=n)).astype(np.float32)
                        bias = None if variant in (2, 3) else rng.uniform(-300, 300, size=n).astype(np.float32)
                        xd = torch.zeros(x_off + D * ldx, dtype=torch.float32, device=dev())
                        xd[x_off:].copy_(torch.as_tensor(x.reshape(-1)))
                        out = torch.full((img_off + GUARD + n * D + GUARD,), int(np.uint16(SENTINEL16).view(np.int16)), dtype=torch.int16, device=dev())
                        (g, b) = (None if v is None else torch.as_tensor(v).to(dev()) for v in (gain, bias))
                        _capi.linear_to_u16(xd.data_ptr() + 4 * x_off, ldx, n, C, H, W, layout, None if g is None else g.data_ptr(), None if b is None else b.data_ptr(),
                                            out.data_ptr() + 2 * (img_off + GUARD), stream())
                        got = out.cpu().numpy().view(np.uint16)
                        want = linear_to_u16_rule(x, ldx, n, (C, H, W), layout, gain, bias)
                        what = 'layout %d (C, H, W) = %s n = %d ldx = %d offsets (%d, %d) variant %d' % (layout, str((C, H, W)), n, ldx, x_off, img_off, variant)
                        assert np.all(got[:img_off] == SENTINEL16), what
                        assert np.array_equal(got[img_off:], want), what
                        frames16_of(got[img_off:], n, (C, H, W), layout)                           # the guards on both sides survive


@pytest.mark.parametrize('layout', ['NCHW', 'NHWC'])
def test_inverse_pair_at_16_bits(layout):
    rng = np.random.RandomState(7)
    with torch.cuda.device(dev()):
        for (C, H, W) in SHAPES:
            for n in (3, 65):
                img = rng.randint(0, 65536, size=(n, C, H, W) if layout == 'NCHW' else (n, H, W, C)).astype(np.uint16)
                f16 = torch.as_tensor(img.view(np.int16)).to(dev()).view(torch.uint16)
                block = ktorch.frames_to_linear(f16, layout=layout)
                assert block.shape == (n, C * H * W + 1) and bool((block[:, -1] == 1).all())
                back = ktorch.linear_to_frames(block, (C, H, W), layout=layout, depth=16)
                assert back.dtype == torch.uint16 and back.shape == f16.shape
                assert np.array_equal(_bits(back), img)


@pytest.mark.parametrize('depth', [8, 16])
def test_round_trip_on_the_device(depth):
    """column_range -> gray_affine -> linear_to_frames -> gray_inverse -> frames_to_linear restores every feature to within the host file's bound; a constant image
    comes back exactly."""
    levels = LEVELS[depth]
    rng = np.random.RandomState(200 + depth)
    (C, H, W) = (2, 9, 15)
    D = C * H * W
    (lo, hi) = random_ranges(rng, 90)
    (lo, hi) = (lo[:65], hi[:65])
    n = lo.size
    assert n == 65
    u = rng.rand(n, D)
    u[:, 0] = 0.0
    u[:, 1] = 1.0
    x = np.clip((lo[:, None].astype(np.float64) + u * (hi.astype(np.float64) - lo.astype(np.float64))[:, None]).astype(np.float32), lo[:, None], hi[:, None])
    x[7, :] = np.float32(-3.75)                                          # a constant image
    const = 7
    with torch.cuda.device(dev()):
        block = ktorch.affine_to_linear(torch.as_tensor(x).reshape(n, C, H, W).to(dev()))
        (dlo, dhi) = ktorch.column_range(block)
        (gain, bias) = ktorch.gray_affine(dlo, dhi, levels)
        q = ktorch.linear_to_frames(block, (C, H, W), layout='NHWC', gain=gain, bias=bias, depth=depth)
        assert q.dtype == TDTYPES[depth]
        (scale, offset) = ktorch.gray_inverse(dlo, dhi, levels)
        back = ktorch.frames_to_linear(q, layout='NHWC', scale=scale, offset=offset)
        (back, dlo, dhi) = (back.cpu().numpy(), dlo.cpu().numpy(), dhi.cpu().numpy())
    assert np.all(back[:, D] == 1.0)
    assert np.array_equal(back[const, :D], x[const])                     # (0, lo): restored exactly
    live = np.arange(n) != const
    assert np.array_equal(dlo[live], x[live].min(1)) and np.array_equal(dhi[live], x[live].max(1))
    bound = roundtrip_bound(dlo[live], dhi[live], levels)                # asserts the input condition per image
    err = np.abs(back[live, :D].astype(np.float64) - x[live].astype(np.float64))
    ratio = float((err / bound[:, None]).max())
    print('depth %d on the device: worst |restored - x| / bound = %.3f' % (depth, ratio))
    assert ratio <= 1.0, ratio


def _plain(name, n, seed):
    (C, H, W) = _net(name)[2]
    return torch.as_tensor(np.random.RandomState(seed).randint(0, 256, size=(n, H, W, C)).astype(np.uint8))


def _floats(frames):
    return frames.permute(0, 3, 1, 2).contiguous().float()


@pytest.mark.parametrize('name', ['lenet', 'vgg16-slice'])
def test_exact_path_on_the_permutation_nets(name):
    (sensor, model, (C, H, W)) = _net(name)
    with torch.cuda.device(dev()):
        f = _plain(name, 5, 11).to(dev())
        (cf, lo, hi) = sensor.encrypt_to_frames(f, range=(0, 255))
        assert cf.dtype == torch.uint8 and cf.is_cuda and cf.shape == f.shape and lo.is_cuda and hi.is_cuda
        assert torch.equal(lo, torch.zeros(5, device=dev())) and torch.equal(hi, torch.full((5,), 255.0, device=dev()))
        own = ktorch.linear_to_frames(sensor.encrypt_frames(f), (C, H, W))       # the encrypted block's own bytes (a permutation of the plaintext's)
        assert torch.equal(cf, own) and not torch.equal(cf, f)
        assert torch.equal(sensor.decrypt_from_frames(cf, lo, hi), f)
        want = model.forward_linear(sensor.fromtensor(_floats(f.cpu())).encrypt().astensor()).cpu()        # (a host batch: a host result)
        got = model.forward_frames(cf, lo, hi).cpu()
        assert got.shape == want.shape and torch.equal(got, want)
        # NCHW frames of the same images
        (cn, lo_n, hi_n) = sensor.encrypt_to_frames(f.permute(0, 3, 1, 2).contiguous(), layout='NCHW', range=(0, 255))
        assert torch.equal(model.forward_frames(cn, lo_n, hi_n, layout='NCHW').cpu(), want)
        # three images on the narrow path
        f3 = f[:3].contiguous()
        (c3, lo3, hi3) = sensor.encrypt_to_frames(f3, range=(0, 255))
        want3 = model.forward_linear(sensor.fromtensor(_floats(f3.cpu())).encrypt().astensor(), narrow=True).cpu()
        assert torch.equal(model.forward_frames(c3, lo3, hi3, narrow=True).cpu(), want3)
        # 16 bits over (0, 65535): the same integers
        (c16, lo16, hi16) = sensor.encrypt_to_frames(f, depth=16, range=(0, 65535))
        assert c16.dtype == torch.uint16 and np.array_equal(_bits(c16), cf.cpu().numpy().astype(np.uint16))
        assert torch.equal(model.forward_frames(c16, lo16, hi16).cpu(), want)
        assert torch.equal(sensor.decrypt_from_frames(c16, lo16, hi16), f)
        wide = torch.as_tensor((cf.cpu().numpy().astype(np.uint16) * 257).view(np.int16)).to(dev()).view(torch.uint16)       # frames that are multiples of 257
        want257 = model.forward_linear(sensor.fromtensor(_floats(f.cpu()) * 257.0).encrypt().astensor()).cpu()
        assert torch.equal(model.forward_frames(wide, lo16, hi16).cpu(), want257)
        # the per-image range of a permutation key is the plaintext's own
        (cr, lor, hir) = sensor.encrypt_to_frames(f)
        flat = f.reshape(5, -1).float()
        assert torch.equal(lor, flat.min(1)[0]) and torch.equal(hir, flat.max(1)[0])


def test_float_key_8_against_16_bits():
    """LeNet under an affine photometric image key, 4 images, the default contract: both depths give finite logits, and 16 bits are no further from the unquantised
    forward than 8.  The two figures are printed, not thresholded."""
    torch.manual_seed(0)
    net = LeNet_AvgPool().eval()
    np.random.seed(0)
    (sensor, model) = ksys.Keynet((1, 28, 28), net, global_photometric='uniform_random_affine', beta=1.0, gamma=1.0)
    with torch.cuda.device(dev()):
        f = torch.as_tensor(np.random.RandomState(3).randint(0, 256, size=(4, 28, 28, 1)).astype(np.uint8)).to(dev())
        ref = model.forward_linear(sensor.encrypt_frames(f))
        delta = {}
        for depth in (8, 16):
            (cf, lo, hi) = sensor.encrypt_to_frames(f, depth=depth)
            assert cf.dtype == TDTYPES[depth]
            y = model.forward_frames(cf, lo, hi)
            assert y.shape == ref.shape and bool(torch.isfinite(y).all())
            delta[depth] = float((y - ref).abs().max())
        back = sensor.decrypt_from_frames(*sensor.encrypt_to_frames(f, depth=16))
        wrong16 = int((back != f).sum())
    print('float key, LeNet, 4 images: max |dlogit| cipher8 = %.3e, cipher16 = %.3e (max |logit| %.3e); plaintext bytes changed by a 16-bit round trip: %d of %d'
          % (delta[8], delta[16], float(ref.abs().max()), wrong16, f.numel()))
    assert delta[16] <= delta[8]


def _cipher_batches(name, sizes, depth):
    """[(frames, lo, hi)] on the host: random quantised frames with random ranges, different in every batch."""
    (C, H, W) = _net(name)[2]
    rng = np.random.RandomState(len(name) + sum(sizes) + depth)
    items = []
    for n in sizes:
        frames = rng.randint(0, LEVELS[depth] + 1, size=(n, H, W, C)).astype(DTYPES[depth])
        lo = rng.uniform(-4, 0, size=n).astype(np.float32)
        hi = (lo + rng.uniform(1, 300, size=n)).astype(np.float32)
        items.append((torch.as_tensor(frames.view(np.int16)).view(torch.uint16) if depth == 16 else frames, lo, torch.as_tensor(hi)))
    return items


def _forward_frames_of(name, items, kw):
    model = _net(name)[1]
    out = []
    for (f, lo, hi) in items:
        (f, lo, hi) = (torch.as_tensor(v).to(dev()) for v in (f, lo, hi))
        out.append(model.forward_frames(f, lo, hi, **kw).cpu())
    return out


@pytest.mark.parametrize('kw', [{}, NARROW], ids=['wide', 'narrow'])
@pytest.mark.parametrize('depth', [8, 16])
@pytest.mark.parametrize('name', ['lenet', 'vgg16-slice'])
def test_streamed_cipher_batches_equal_forward_frames(name, depth, kw):
    model = _net(name)[1]
    sizes = NARROW_SIZES if kw else SIZES
    items = _cipher_batches(name, sizes, depth)
    with torch.cuda.device(dev()):
        with StreamedForward(None, model, max(sizes), frames='cipher%d' % depth, **kw) as sf:
            got = list(sf.run(items))
        assert sf._buffers is None
        want = _forward_frames_of(name, items, kw)                       # computed afterwards, batch by batch
    assert len(got) == len(want) and len(set(g.data_ptr() for g in got)) == len(got) and not any(g.is_pinned() for g in got)
    for (k, (g, w)) in enumerate(zip(got, want)):
        assert not g.is_cuda and tuple(g.shape) == tuple(w.shape) == (sizes[k], w.shape[1])
        assert torch.equal(g, w), 'batch %d of %s (%d images)' % (k, name, sizes[k])


@pytest.mark.parametrize('name', ['lenet', 'vgg16-slice'])
def test_streamed_end_to_end_equals_the_plaintext_path(name):
    """plaintext -> encrypt_to_frames(range=(0, 255)) -> host -> 'cipher8' gives what forward_linear gives on the sensor's own encrypt of the plaintext."""
    (sensor, model, _) = _net(name)
    with torch.cuda.device(dev()):
        plains = [_plain(name, n, 40 + k) for (k, n) in enumerate(SIZES)]
        items = [tuple(v.cpu() for v in sensor.encrypt_to_frames(p.to(dev()), range=(0, 255))) for p in plains]
        with StreamedForward(None, model, max(SIZES), frames='cipher8') as sf:
            got = list(sf.run(items))
        for (k, (g, p)) in enumerate(zip(got, plains)):
            want = model.forward_linear(sensor.fromtensor(_floats(p)).encrypt().astensor()).cpu()
            assert torch.equal(g, want), 'batch %d' % k
    assert len(got) == len(SIZES)


class _InputBroke(Exception):
    pass


def test_streamed_cipher_close_in_mid_iteration_and_raising_input():
    name = 'lenet'
    model = _net(name)[1]
    items = _cipher_batches(name, SIZES, 8)
    with torch.cuda.device(dev()):
        want = _forward_frames_of(name, items, {})
        sf = StreamedForward(None, model, max(SIZES), frames='cipher8')
        run = sf.run(items)
        got = [next(run) for _ in range(3)]
        sf.close()
        assert sf._buffers is None and sf._active is None
        with pytest.raises(StopIteration):
            next(run)
        with pytest.raises(RuntimeError):
            sf.run([])
        assert all(torch.equal(g, w) for (g, w) in zip(got, want[:3]))

        def two_then_raise():
            yield items[0]
            yield items[1]
            raise _InputBroke('the sensor went away')

        got = []
        with StreamedForward(None, model, max(SIZES), frames='cipher8') as again:
            with pytest.raises(_InputBroke):
                for g in again.run(two_then_raise()):
                    got.append(g)
            assert len(got) == 2 and all(torch.equal(g, w) for (g, w) in zip(got, want[:2]))
            got = []
            with pytest.raises(ValueError, match='lo must be'):              # a refused batch in mid-run behaves the same way
                for g in again.run(items[:2] + [(items[2][0], items[2][1][:1], items[2][2])]):
                    got.append(g)
            assert len(got) == 2 and all(torch.equal(g, w) for (g, w) in zip(got, want[:2]))
            assert all(torch.equal(g, w) for (g, w) in zip(again.run(items), want))
        torch.cuda.synchronize()
