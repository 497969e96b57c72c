"""The keyed forward fed from the host: camera frames in, logits out, with the transfers behind the compute.

The reference's callers hand CPU tensors to the key-net (keynet/sparse.py:488-492) and its sensor loads and encrypts an image on the host
(keynet/system.py:183-201, 250-255).  StreamedForward is that use at the rate of the device: batches of host frames are uploaded, ingested (kn_u8_to_linear, or
kn_affine_to_linear for float batches), encrypted by the sensor's own keyed product and run through KeyedModel.forward_linear, and the logits come back to the host,
two batches deep -- the upload of the next batch and the read-back of the previous one run on streams of their own while the current batch computes.  Image by image
the logits are those of model.forward_linear(sensor.fromtensor(x.float()).encrypt().astensor(), **keywords), bit for bit: nothing on the path is a different kernel.
One Python thread, no process, no environment variable; forward_linear, _prepare and the existing kernels are used as they are.
The kinds 'cipher8' and 'cipher16' are the deployment in which sensor and server are different parties: the batches are frames that are ALREADY encrypted and quantised
(KeyedSensor.encrypt_to_frames) with their public ranges, the pipeline needs no sensor, and its compute step is KeyedModel.forward_frames."""
import numpy as np
import torch

from . import _capi
from . import sparse as ksp
from . import torch as ktorch

FRAME_KINDS = ('uint8', 'float32', 'cipher8', 'cipher16')
CIPHER_KINDS = {'cipher8': torch.uint8, 'cipher16': torch.uint16}


class StreamedForward(object):
    """StreamedForward(sensor, model, batch, layout='NHWC', frames='uint8', **keywords of model.forward_linear)

    run(batches)   a generator: for every item of `batches` -- a CPU tensor or ndarray of n_k <= batch frames -- the host logits [n_k, classes + 1], in order.
    close()        waits for the streams, drops the pinned and the device buffers (also a context manager).

    frames='uint8':   [n, H, W, C] (layout 'NHWC') or [n, C, H, W] ('NCHW') bytes, raw [0, 255] values as the reference feeds them; one kn_u8_to_linear launch makes the
                      feature-major block, its padding included.
    frames='float32': [n, C, H, W] floats (a caller that normalises on the host; `layout` does not apply), through kn_affine_to_linear: four times the bytes per image.
    frames='cipher8' | 'cipher16': the items are (frames, lo, hi) -- quantised ENCRYPTED frames, uint8 | uint16 in `layout`, and their ranges, host float32 arrays or
                      tensors [n] (what KeyedSensor.encrypt_to_frames returned, brought to the host).  `sensor` may be None: the frame shape comes from the model, the
                      sensor's product is not applied, and the compute step is model.forward_frames (the dequantising ingest kn_frames_to_linear, then forward_linear).
                      lo / hi travel through two small pinned staging buffers and two device buffers of their own, on the copy-in stream behind the same events as
                      their frames.  For the other kinds a sensor is required.
    The keywords (`overlap`, the narrow family) go to model.forward_linear unchanged.  On the wide path of a tiled-conv key-net the ingest pads the batch to whole
    model.BATCH_TILE tiles with zero images, so that KeyedModel._prepare takes the block in place; elsewhere nothing is padded.

    The pipeline, for batch k (slot = k % 2 of two pinned staging buffers, two device frame buffers, two pinned logits buffers):
      1. batch k + 1 is copied into its pinned staging buffer (the host waits for the upload that last used it);
      2. its upload is enqueued on the copy-in stream, behind the event of the ingest that last read that device buffer;
      3. THEN ingest, encrypt and forward_linear of batch k go onto torch's current stream, behind the event of upload k -- a forward that ends in a host read
         (calibrated layers) blocks the host with upload k + 1 already under way;
      4. an event on the current stream; the read-back of the logits on the copy-out stream behind it;
      5. the host waits for the read-back of batch k - 1 and yields a fresh tensor with its logits (never a view of the pinned buffer).
    A buffer is re-used only behind an event; what one stream allocates and another reads is record_stream'ed.  An exception from `batches` (or a batch that is
    refused) is raised after the results of the batches before it have been yielded; closing the generator or the object in mid-iteration waits for the work in flight."""

    def __init__(self, sensor, model, batch, layout='NHWC', frames='uint8', **keywords):
        if frames not in FRAME_KINDS:
            raise ValueError('invalid frames "%s": one of %s' % (str(frames), ', '.join(FRAME_KINDS)))
        if layout not in ktorch.LAYOUTS:
            raise ValueError('invalid layout "%s": one of %s' % (str(layout), ', '.join(ktorch.LAYOUTS)))
        if int(batch) < 1:
            raise ValueError('batch must be a positive number of images, not %s' % str(batch))
        self._cipher = frames in CIPHER_KINDS
        if sensor is None and not self._cipher:
            raise ValueError('frames="%s" needs the sensor whose key the pipeline applies (only %s run without one)' % (frames, ', '.join(sorted(CIPHER_KINDS))))
        (self._sensor, self._model, self._batch, self._keywords) = (sensor, model, int(batch), dict(keywords))
        (self._dtype, self._layout) = (torch.float32, 'NCHW') if frames == 'float32' else (CIPHER_KINDS.get(frames, torch.uint8), layout)
        (C, H, W) = model.frame_shape() if self._cipher else tuple(sensor._inshape[1:])
        self._frame = (H, W, C) if self._layout == 'NHWC' else (C, H, W)
        wide_tiled = not keywords.get('narrow') and any(isinstance(c.W, ksp.Conv2dTiledMatrix) for c in model._keyed())
        self._pad_to = int(model.BATCH_TILE) if wide_tiled else 1
        (self._buffers, self._active, self._closed) = (None, None, False)

    # -- arguments (no GPU call) ---------------------------------------------------------------------------------------------------
    def _checked(self, item):
        """The item of `batches` as a CPU tensor of this pipeline's kind; ValueError otherwise."""
        if self._cipher:
            if not isinstance(item, (tuple, list)) or len(item) != 3:
                raise ValueError('a batch of encrypted frames is (frames, lo, hi), not %s' % type(item).__name__)
            (t, lo, hi) = (torch.as_tensor(v) if isinstance(v, np.ndarray) else v for v in item)
            ktorch.frame_shape(t, self._layout, self._dtype)                  # (the dtype of this pipeline's kind, then the model's own checks)
            n = self._model.check_cipher_frames(t, lo, hi, self._layout)
        else:
            t = torch.as_tensor(item) if isinstance(item, np.ndarray) else item
            n = self._sensor.check_frames(t, self._layout, self._dtype)
        if t.is_cuda:
            raise ValueError('StreamedForward takes host batches (frames on the device go to KeyedSensor.encrypt_frames or KeyedModel.forward_frames)')
        if n > self._batch:
            raise ValueError('a batch of %d images in a pipeline built for %d' % (n, self._batch))
        return (t, lo, hi) if self._cipher else t

    # -- buffers and streams ---------------------------------------------------------------------------------------------------------
    def _allocate(self):
        if not torch.cuda.is_available():
            raise _capi.KeynetHipError('keynet_amd: no MI355X visible -- the keyed forward has no CPU fallback')
        dev = torch.device('cuda', torch.cuda.current_device())
        shape = (self._batch,) + self._frame
        b = dict(device=dev, copy_in=torch.cuda.Stream(dev), copy_out=torch.cuda.Stream(dev), compute=None, pin_out=[None, None],
                 pin_in=[torch.empty(shape, dtype=self._dtype, pin_memory=True) for _ in range(2)],
                 dev_in=[torch.empty(shape, dtype=self._dtype, device=dev) for _ in range(2)],
                 uploaded=[None, None], consumed=[None, None], downloaded=[None, None])
        if self._cipher:                                            # row 0: lo, row 1: hi
            b['pin_range'] = [torch.empty((2, self._batch), dtype=torch.float32, pin_memory=True) for _ in range(2)]
            b['dev_range'] = [torch.empty((2, self._batch), dtype=torch.float32, device=dev) for _ in range(2)]
        for d in b['dev_in'] + b.get('dev_range', []):
            d.record_stream(b['copy_in'])
        self._buffers = b

    def _wait_streams(self):
        b = self._buffers
        if b is not None:
            b['copy_in'].synchronize()
            if b['compute'] is not None:
                b['compute'].synchronize()
            b['copy_out'].synchronize()

    # -- the five steps ------------------------------------------------------------------------------------------------------------------
    def _upload(self, k, t):
        """Steps 1 and 2 for batch k."""
        (t, lo, hi) = t if self._cipher else (t, None, None)
        (b, slot, n) = (self._buffers, k % 2, t.shape[0])
        if b['uploaded'][slot] is not None:
            b['uploaded'][slot].synchronize()                      # the upload of batch k - 2 has read this staging buffer
        b['pin_in'][slot][:n].copy_(t)
        if self._cipher:
            b['pin_range'][slot][0, :n].copy_(lo)
            b['pin_range'][slot][1, :n].copy_(hi)
        with torch.cuda.stream(b['copy_in']):
            if b['consumed'][slot] is not None:
                b['copy_in'].wait_event(b['consumed'][slot])         # the ingest of batch k - 2 has read this device buffer
            b['dev_in'][slot][:n].copy_(b['pin_in'][slot][:n], non_blocking=True)
            if self._cipher:
                b['dev_range'][slot][:, :n].copy_(b['pin_range'][slot][:, :n], non_blocking=True)
            b['uploaded'][slot] = torch.cuda.Event()
            b['uploaded'][slot].record(b['copy_in'])
        return n

    def _linear(self, x):
        """The device frames x as the homogeneous block [n_cols, D + 1] (transposed view of a fresh feature-major block, zero images beyond n)."""
        if self._dtype == torch.uint8:
            return ktorch.frames_to_linear(x, layout=self._layout, pad_to=self._pad_to)
        n = x.shape[0]
        n_cols = -(-n // self._pad_to) * self._pad_to
        if n_cols == n:
            return ktorch.affine_to_linear(x)
        D = int(np.prod(x.shape[1:]))
        out = torch.zeros((D + 1, n_cols), dtype=torch.float32, device=x.device)
        _capi.affine_to_linear(x.data_ptr(), n, D, out.data_ptr(), n_cols, torch.cuda.current_stream().cuda_stream)
        return out.t()

    def _compute(self, k, n):
        """Steps 3 and 4 for batch k of n images."""
        (b, slot) = (self._buffers, k % 2)
        compute = b['compute']
        compute.wait_event(b['uploaded'][slot])
        if self._cipher:                                                  # ingest and forward are one call: the buffers are free behind it
            rng = b['dev_range'][slot]
            y = self._model.forward_frames(b['dev_in'][slot][:n], rng[0, :n], rng[1, :n], layout=self._layout, **self._keywords).contiguous()
            b['consumed'][slot] = torch.cuda.Event()
            b['consumed'][slot].record(compute)
        else:
            lin = self._linear(b['dev_in'][slot][:n])
            b['consumed'][slot] = torch.cuda.Event()
            b['consumed'][slot].record(compute)
            y = self._model.forward_linear(self._sensor.forward(lin), **self._keywords)[:n].contiguous()
        if b['pin_out'][slot] is None or b['pin_out'][slot].shape[1] != y.shape[1]:
            b['pin_out'][slot] = torch.empty((self._batch, y.shape[1]), dtype=y.dtype, pin_memory=True)
        done = torch.cuda.Event()
        done.record(compute)
        with torch.cuda.stream(b['copy_out']):
            b['copy_out'].wait_event(done)
            b['pin_out'][slot][:n].copy_(y, non_blocking=True)
            y.record_stream(b['copy_out'])
            b['downloaded'][slot] = torch.cuda.Event()
            b['downloaded'][slot].record(b['copy_out'])

    def _result(self, k, n):
        """Step 5 for batch k."""
        (b, slot) = (self._buffers, k % 2)
        b['downloaded'][slot].synchronize()
        return b['pin_out'][slot][:n].clone()

    # -- the public surface ----------------------------------------------------------------------------------------------------------------
    def run(self, batches):
        if self._closed:
            raise RuntimeError('this StreamedForward is closed')
        if self._active is not None:
            raise RuntimeError('a run of this StreamedForward is still under way: close its generator first')
        self._active = self._run(iter(batches))
        return self._active

    def _next(self, it):
        """(the next checked batch or None at the end, the exception that ended the input or None)."""
        try:
            return (self._checked(next(it)), None)
        except StopIteration:
            return (None, None)
        except Exception as e:
            return (None, e)

    def _run(self, it):
        try:
            (t, failure) = self._next(it)
            if t is not None:
                if self._buffers is None:
                    self._allocate()
                self._buffers['compute'] = torch.cuda.current_stream(self._buffers['device'])
                (k, n, before) = (0, self._upload(0, t), None)
                while n is not None:
                    (t, failure) = self._next(it)
                    n_next = self._upload(k + 1, t) if t is not None else None
                    self._compute(k, n)
                    if before is not None:
                        yield self._result(k - 1, before)
                    (k, before, n) = (k + 1, n, n_next)
                yield self._result(k - 1, before)
            if failure is not None:
                raise failure
        finally:
            self._active = None
            self._wait_streams()

    def close(self):
        if self._active is not None:
            self._active.close()               # its finally waits for the work in flight
            self._active = None
        self._wait_streams()
        (self._buffers, self._closed) = (None, True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
