"""Tensor-side helpers of the keyed forward (mirror of the parts of keynet/torch.py that sit on the path).

On a CUDA(ROCm) tensor the homogeneous augmentation runs in HIP kernels (kn_affine_to_linear / kn_linear_to_affine);
CPU tensors take the trivial torch route (this is plumbing before/after the path, not the path).
"""
from collections import OrderedDict
import numpy as np
import torch
from torch import nn

from . import _capi


def _stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def affine_to_linear(x):
    """NxCxHxW (or CxHxW) -> Nx(C*H*W+1) with a trailing ones column (keynet/torch.py:65-68).

    For a device tensor the result is a transposed VIEW of a feature-major [D+1, N] buffer, i.e. already in the layout
    the keyed layers consume (their x.t() is then free)."""
    if x.dim() == 3:
        x = x.unsqueeze(0)
    (N, D) = (x.shape[0], int(np.prod(x.shape[1:])))
    if x.is_cuda:
        xc = x.reshape(N, D).contiguous().float()
        out = torch.empty((D + 1, N), dtype=torch.float32, device=x.device)
        _capi.affine_to_linear(xc.data_ptr(), N, D, out.data_ptr(), N, _stream_ptr())
        return out.t()
    return torch.cat((x.reshape(N, D), torch.ones(N, 1, dtype=x.dtype)), dim=1)


LAYOUTS = ('NCHW', 'NHWC')      # the `layout` strings of frames_to_linear, in the order of kn_u8_to_linear's codes


FRAME_DTYPES = (torch.uint8, torch.uint16)      # the stored integers of a quantised frame; their depth in bits is 8 * itemsize
GRAY_LEVELS = {8: 255, 16: 65535}               # the top gray level of a depth


def frame_shape(frames, layout='NHWC', dtype=torch.uint8):
    """(n, (C, H, W)) of a batch of frames [n, H, W, C] (layout 'NHWC') or [n, C, H, W] ('NCHW'); ValueError for another layout string, rank or dtype (one, or a tuple of
    admissible ones), or an empty batch.
    Touches no GPU (what frames_to_linear, KeyedSensor.encrypt_frames and StreamedForward check their arguments with)."""
    if layout not in LAYOUTS:
        raise ValueError('invalid layout "%s": one of %s' % (str(layout), ', '.join(LAYOUTS)))
    if not isinstance(frames, torch.Tensor):
        raise ValueError('frames must be a torch tensor, not %s' % type(frames).__name__)
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
    if frames.dtype not in dtypes:
        raise ValueError('frames must be %s, not %s' % (' or '.join(str(d) for d in dtypes), frames.dtype))
    if frames.dim() != 4:
        raise ValueError('frames must be [n, %s], not a tensor of rank %d' % ('H, W, C' if layout == 'NHWC' else 'C, H, W', frames.dim()))
    if min(frames.shape) < 1:
        raise ValueError('empty batch of frames: shape %s' % str(tuple(frames.shape)))
    (n, a, b, c) = (int(v) for v in frames.shape)
    return (n, (c, a, b) if layout == 'NHWC' else (a, b, c))


def frames_to_linear(frames, layout='NHWC', pad_to=1, scale=None, offset=None):
    """uint8 or uint16 frames on the device, [n, H, W, C] (layout 'NHWC': a camera's order) or [n, C, H, W] ('NCHW') -> [n_cols, C*H*W+1] float32 with a trailing ones
    column, n_cols = n rounded up to a multiple of `pad_to`; the rows beyond n are zero images (all zero, the ones column included: what KeyedModel._prepare
    pads a batch with).  Like the device branch of affine_to_linear the result is the transposed VIEW of a fresh feature-major [D+1, n_cols] block; its first n
    rows are bit-equal to affine_to_linear(frames.permute(0, 3, 1, 2).float()).  `scale`, `offset`: None or device float32 tensors [n], one pair per image
    (gray_inverse's): the dequantising ingest, feature = scale[b] * frame + offset[b] -- an f32 multiply, then an f32 add; a None leaves its statement out; the zero
    images stay zero.  One launch on the current stream: kn_u8_to_linear for uint8 frames without `scale` / `offset`, kn_frames_to_linear for everything else.
    ValueError for a wrong dtype, rank or layout string, before any GPU call."""
    (n, (C, H, W)) = frame_shape(frames, layout, FRAME_DTYPES)
    if int(pad_to) < 1:
        raise ValueError('pad_to must be a positive number of images, not %s' % str(pad_to))
    if not frames.is_cuda:
        raise ValueError('frames_to_linear takes frames that are on the device (StreamedForward brings host frames there)')
    (scale, offset) = (_per_image(scale, n, frames.device, 'scale'), _per_image(offset, n, frames.device, 'offset'))
    n_cols = -(-n // int(pad_to)) * int(pad_to)
    fc = frames.contiguous()
    out = torch.empty((C * H * W + 1, n_cols), dtype=torch.float32, device=frames.device)
    with torch.cuda.device(frames.device):
        if frames.dtype == torch.uint8 and scale is None and offset is None:
            _capi.u8_to_linear(fc.data_ptr(), n, C, H, W, LAYOUTS.index(layout), out.data_ptr(), n_cols, n_cols, _stream_ptr())
        else:
            _capi.frames_to_linear(fc.data_ptr(), 8 * fc.element_size(), n, C, H, W, LAYOUTS.index(layout), None if scale is None else scale.data_ptr(),
                                   None if offset is None else offset.data_ptr(), out.data_ptr(), n_cols, n_cols, _stream_ptr())
    return out.t()


def _check_linear(x_linear, what, features=None):
    """(n, D) of an [n, D+1] float32 device tensor; ValueError for another type, rank, dtype or feature count, an empty batch or a host tensor.  Touches no GPU."""
    if not isinstance(x_linear, torch.Tensor):
        raise ValueError('%s takes a torch tensor, not %s' % (what, type(x_linear).__name__))
    if x_linear.dim() != 2:
        raise ValueError('%s takes the homogeneous block [n, D+1], not a tensor of rank %d' % (what, x_linear.dim()))
    if x_linear.dtype != torch.float32:
        raise ValueError('%s takes a float32 block, not %s' % (what, x_linear.dtype))
    (n, D) = (int(x_linear.shape[0]), int(x_linear.shape[1]) - 1)
    if n < 1 or D < 1:
        raise ValueError('%s: empty block of shape %s' % (what, str(tuple(x_linear.shape))))
    if features is not None and D != int(features):
        raise ValueError('%s: %d features per image do not fit the frame shape, which has %d' % (what, D, int(features)))
    if not x_linear.is_cuda:
        raise ValueError('%s takes a block that is on the device' % what)
    return (n, D)


def _feature_major(x_linear):
    """The feature-major [D+1, n] block the kernels read: the transposed view of x_linear in place where that is contiguous (what the keyed layers and frames_to_linear
    return), the block ksp._device_block makes of it otherwise."""
    xt = x_linear.detach().t()
    if xt.is_contiguous():
        return xt
    from . import sparse as ksp
    return ksp._device_block(xt)


def column_range(x_linear):
    """[n, D+1] float32 on the device -> (lo, hi), device float32 [n]: each image's minimum and maximum over its D features, the homogeneous column left out -- the two
    numbers the reference's mat2gray takes of an image on the host (keynet/sparse.py:27).  NaN features are skipped; an image with no other feature gives (+Inf, -Inf).
    kn_column_range on the current stream: no host read, nothing waits.  ValueError as linear_to_frames, before any GPU call."""
    (n, D) = _check_linear(x_linear, 'column_range')
    xt = _feature_major(x_linear)
    lo = torch.empty(n, dtype=torch.float32, device=xt.device)
    hi = torch.empty(n, dtype=torch.float32, device=xt.device)
    with torch.cuda.device(xt.device):
        _capi.column_range(xt.data_ptr(), D, n, n, lo.data_ptr(), hi.data_ptr(), _stream_ptr())
    return (lo, hi)


def gray_affine(lo, hi, levels=255):
    """(gain, bias) of the gray mapping of images whose ranges are [lo, hi] onto [0, levels]: gain = levels / (hi - lo), bias = -lo * gain, element-wise on the tensors' own
    device without a host read (keynet/sparse.py:25-33 with the 255 of the 8-bit image folded in; levels=65535: a 16-bit image).  Where hi == lo or the range is not finite
    (an infinite feature, or the (+Inf, -Inf) of an image with no feature to compare) gain = 0 and bias = 0: such an image becomes black.  The reference divides by zero
    there: its constant image is all NaN."""
    (lo, hi) = (lo.float(), hi.float())
    span = hi - lo
    ok = torch.isfinite(lo) & torch.isfinite(hi) & torch.isfinite(span) & (span > 0)
    (zero, one) = (torch.zeros_like(span), torch.ones_like(span))
    gain = float(levels) / torch.where(ok, span, one)
    bias = -torch.where(ok, lo, zero) * gain
    ok = ok & torch.isfinite(gain) & torch.isfinite(bias)                # (a span so small that levels / span overflows: not a finite range to map either)
    return (torch.where(ok, gain, zero), torch.where(ok, bias, zero))


def gray_inverse(lo, hi, levels=255):
    """(scale, offset) = ((hi - lo) / levels, lo) of the inverse of gray_affine(lo, hi, levels): gray level q of an image whose range is [lo, hi] stands for the feature
    scale * q + offset.  Element-wise on the tensors' own device without a host read.  A constant image (hi == lo: gray_affine stored it as black) gives (0, lo), so it is
    restored exactly; a range that is not finite, or empty (hi < lo), gives (0, 0).  Public numbers: the range of an ENCRYPTED image, or one fixed range of the converter."""
    (lo, hi) = (lo.float(), hi.float())
    span = hi - lo
    ok = torch.isfinite(lo) & torch.isfinite(hi) & torch.isfinite(span) & (span >= 0)
    zero = torch.zeros_like(span)
    return (torch.where(ok, span, zero) / float(levels), torch.where(ok, lo, zero))


def check_range(cipher_frames, lo, hi, n):
    """ValueError for ranges lo / hi that are not float32 tensors [n] on the device of the n quantised frames they came with.  No GPU call."""
    for (v, name) in ((lo, 'lo'), (hi, 'hi')):
        if not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or tuple(v.shape) != (n,) or v.device != cipher_frames.device:
            raise ValueError('%s must be a float32 tensor of shape [%d] on the device of the frames' % (name, n))


def cipher_range(cipher_frames, lo, hi, n):
    """gray_inverse of the ranges that came with n quantised frames, the levels read from the frames' dtype (check_range first)."""
    check_range(cipher_frames, lo, hi, n)
    return gray_inverse(lo, hi, GRAY_LEVELS[8 * cipher_frames.element_size()])


def _per_image(v, n, device, name):
    if v is None:
        return None
    if not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or tuple(v.shape) != (n,):
        raise ValueError('%s must be None or a float32 tensor of shape [%d]' % (name, n))
    if not v.is_cuda or v.device != device:
        raise ValueError('%s must be on the device of the block' % name)
    return v.detach().contiguous()


def linear_to_frames(x_linear, inshape, layout='NHWC', gain=None, bias=None, depth=8):
    """[n, C*H*W+1] float32 on the device (`inshape` = (C, H, W)) -> uint8 frames on the device, [n, H, W, C] (layout 'NHWC': a viewer's or an encoder's order) or
    [n, C, H, W] ('NCHW'): frame = min(255, max(0, rint(gain[b] * x + bias[b]))), NaN -> 0 -- an f32 multiply, an f32 add, round to nearest even.  `gain`, `bias`: None (1 and
    0: the block's own values) or device float32 tensors [n], one pair per image (gray_affine's).  The inverse of frames_to_linear: linear_to_frames(frames_to_linear(f)) == f.
    The homogeneous column is not read (linear_to_affine is the call that checks it).  One launch of kn_linear_to_u8 on the current stream; the transposed view of a
    feature-major block is read in place.  depth=16: torch.uint16 frames through kn_linear_to_u16, the same rule saturating at 65535.  ValueError for a wrong layout
    string, depth, rank, dtype or feature count, or a host tensor, before any GPU call."""
    if depth not in GRAY_LEVELS:
        raise ValueError('invalid depth %s: 8 or 16 bits' % str(depth))
    if layout not in LAYOUTS:
        raise ValueError('invalid layout "%s": one of %s' % (str(layout), ', '.join(LAYOUTS)))
    if len(tuple(inshape)) != 3 or min(int(v) for v in inshape) < 1:
        raise ValueError('inshape must be (C, H, W), not %s' % str(inshape))
    (C, H, W) = (int(v) for v in inshape)
    (n, D) = _check_linear(x_linear, 'linear_to_frames', C * H * W)
    (gain, bias) = (_per_image(gain, n, x_linear.device, 'gain'), _per_image(bias, n, x_linear.device, 'bias'))
    xt = _feature_major(x_linear)
    out = torch.empty((n, H, W, C) if layout == 'NHWC' else (n, C, H, W), dtype=torch.uint8 if depth == 8 else torch.uint16, device=xt.device)
    with torch.cuda.device(xt.device):
        (_capi.linear_to_u8 if depth == 8 else _capi.linear_to_u16)(xt.data_ptr(), n, n, C, H, W, LAYOUTS.index(layout), None if gain is None else gain.data_ptr(), None if bias is None else bias.data_ptr(),
                           out.data_ptr(), _stream_ptr())
    return out


def linear_to_affine(x, outshape=None):
    """Nx(K+1) -> NxK, checking that the homogeneous column is 1 within 1e-3 (ValueError otherwise), then reshaping to
    `outshape` (keynet/torch.py:71-77)."""
    assert x.dim() == 2
    (N, K) = (x.shape[0], x.shape[1] - 1)
    if x.is_cuda and x.t().is_contiguous() and x.dtype == torch.float32:
        xt = x.t()
        out = torch.empty((N, K), dtype=torch.float32, device=x.device)
        dev = torch.zeros(1, dtype=torch.float32, device=x.device)
        _capi.linear_to_affine(xt.data_ptr(), N, N, K, out.data_ptr(), dev.data_ptr(), _stream_ptr())
        d = float(dev.item())
        if not (d <= 1e-3):
            raise ValueError('invalid affine vector: homogeneous coordinate deviates from 1 by %g' % d)
        return out.reshape(outshape) if outshape is not None else out
    last = x[:, -1].detach().cpu().numpy()
    if not np.allclose(last, 1, atol=1e-3):
        raise ValueError('invalid affine vector: homogeneous coordinate deviates from 1 by %g' % float(np.max(np.abs(last - 1))))
    xa = torch.narrow(x, 1, 0, K)
    return xa.reshape(outshape) if outshape is not None else xa


def affine_to_linear_matrix(W_affine, bias=None):
    """(Wx+b)^T as one left-multiplied matrix [[W^T, 0], [b, 1]] of shape (in+1, out+1) (keynet/torch.py:80-89)."""
    Wt = W_affine.t()
    (R, C) = Wt.shape
    M = torch.zeros(R + 1, C + 1, dtype=Wt.dtype)
    M[:R, :C] = Wt
    if bias is not None:
        M[R, :C] = bias.reshape(C)
    M[R, C] = 1
    return M


def fuse_conv2d_and_bn(conv2d_weight, conv2d_bias, bn_running_mean, bn_running_var, bn_eps, bn_weight, bn_bias):
    """Fold an eval-mode BatchNorm2d into the preceding conv (keynet/torch.py:99-113).  The association of the f32
    operations is the reference's -- weights scaled by (bn_weight / std), bias as ((b - mean) / std) * bn_weight + bn_bias --
    because the folded parameters feed the stored keyed operators, which must match bit for bit under the same seed."""
    std = torch.sqrt(bn_running_var + np.float32(bn_eps))
    b = conv2d_bias if conv2d_bias is not None else bn_running_mean.new_zeros(bn_running_mean.shape)
    w = conv2d_weight * (bn_weight / std).reshape(-1, 1, 1, 1)
    return (w, ((b - bn_running_mean) / std) * bn_weight + bn_bias)


def count_parameters(model):
    return sum(p.numel() for p in model.parameters() if p.requires_grad)


def netshape(net, inshape):
    """Trace one dummy forward and return an ordered {name: {inshape, outshape, prevlayer, nextlayer}} chain with the
    pseudo entries 'input' and 'output' (keynet/torch.py:21-62).  Leaf modules are visited in execution order;
    nn.Sequential containers are descended into.  Shapes are canonicalised to (C,H,W) ((C,1,1) for vectors)."""
    chain = OrderedDict()
    hooks = []

    def canon(t):
        return (t.shape[1], t.shape[2], t.shape[3]) if t.dim() == 4 else (t.shape[1], 1, 1)

    def attach(container):
        for (name, layer) in container._modules.items():
            if isinstance(layer, nn.Sequential):
                attach(layer)
            else:
                hooks.append(layer.register_forward_hook(lambda m, i, o, _n=name: record(_n, i, o)))

    def record(name, inp, out):
        (ishape, oshape) = (canon(inp[0]), canon(out))
        if 'input' not in chain:
            chain['input'] = {'prevlayer': None, 'nextlayer': name, 'inshape': ishape, 'outshape': oshape}
        chain.pop('output', None)
        prev = next(reversed(chain))
        chain[name] = {'inshape': ishape, 'outshape': oshape, 'prevlayer': prev, 'nextlayer': None}
        chain[prev]['nextlayer'] = name
        chain['output'] = {'nextlayer': None, 'prevlayer': name, 'inshape': ishape, 'outshape': oshape}

    net.eval()
    attach(net)
    try:
        with torch.no_grad():
            net.forward(torch.rand(1, inshape[0], inshape[1], inshape[2]))
    finally:
        for h in hooks:
            h.remove()
    return chain


class TiledMatrix(object):
    """The explicit tile loop of keynet/torch.py:165-184 (`keynet.torch.TiledMatrix._torchdot`; dead code in the reference, kept for API coverage):

        for (i, j, k) in blocks:  for (ii, jj, v) in tiles[k]:  y[i + ii, :] += v * x[j + jj, :]

    Here the loop is the ORDER of an order-preserving CSR: every output row accumulates its terms in exactly the sequence the loop visits them
    (blocks in the given order, a tile's entries in their stored order), f32 multiply then f32 add, on the device (kn_csr_create + kn_spmm).  The
    reference compiles its loop with numba fastmath + parallel, so its own rounding is unspecified; the serial loop is what tests compare with."""

    @staticmethod
    def _loop_csr(tileshape, shape, tiles, blocks):
        """(indptr, indices, data) whose rows list the loop's terms in visiting order.  `tiles[k]`: array [nnz_k, 3] of (ii, jj, v)."""
        (H, W) = (int(shape[0]), int(shape[1]))
        (rows, cols, vals) = ([], [], [])
        for (i, j, k) in blocks:
            b = np.asarray(tiles[int(k)], dtype=np.float64).reshape(-1, 3)
            rows.append(int(i) + b[:, 0].astype(np.int64))
            cols.append(int(j) + b[:, 1].astype(np.int64))
            vals.append(b[:, 2].astype(np.float32))
        cat = (lambda L, dt: np.concatenate(L).astype(dt) if len(L) else np.zeros(0, dt))
        (r, c, v) = (cat(rows, np.int64), cat(cols, np.int64), cat(vals, np.float32))
        assert r.size == 0 or (r.min() >= 0 and r.max() < H and c.min() >= 0 and c.max() < W), 'tile entry outside the operator'
        order = np.argsort(r, kind='stable')                              # stable: a row keeps the loop's sequence
        indptr = np.zeros(H + 1, np.int64)
        np.cumsum(np.bincount(r, minlength=H), out=indptr[1:])
        return (indptr.astype(np.int32), c[order].astype(np.int32), v[order])

    @staticmethod
    def _torchdot(x, tileshape, shape, tiles, blocks):
        """x: [W, N] float32 torch tensor on a ROCm device (or numpy, moved to the current device) -> y [H, N] on the same device."""
        was_numpy = isinstance(x, np.ndarray)
        if was_numpy:
            x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).to(torch.device('cuda', torch.cuda.current_device()))
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[0] == int(shape[1]), 'non-conformal operand'
        (ip, ix, dt) = TiledMatrix._loop_csr(tileshape, shape, tiles, blocks)
        with torch.cuda.device(x.device):
            op = _capi.Operator.csr((int(shape[0]), int(shape[1])), ip, ix, dt)
            xc = x.contiguous()
            y = torch.empty((int(shape[0]), xc.shape[1]), dtype=torch.float32, device=x.device)
            op.spmm(xc.data_ptr(), xc.shape[1], xc.shape[1], y.data_ptr(), xc.shape[1], _capi.KN_FLAG_EXACT, _stream_ptr())
            torch.cuda.current_stream().synchronize()                     # the operator is destroyed on return
        return y.cpu().numpy() if was_numpy else y
