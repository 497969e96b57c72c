"""Key-net assembly and the top of the hot path (mirror of keynet/system.py:26-516).

    (sensor, model) = PermutationKeynet(inshape, net)          # factories, keynet/system.py:472-510
    y = model.forward(sensor.fromtensor(x).encrypt().astensor())   # keynet/system.py:130-133, README.md:27-34

Keying (host, offline) follows the reference's algebra call for call so that, under the same numpy seed, the stored
operators are identical (tests/test_host_keying.py compares CSR triplets with the golden vectors).  The forward runs on
the MI355X: layers exchange feature-major [D+1, N] blocks, ReLU is fused into the producing kernel, and batches are
supported (the reference's KeyedModel.forward is N=1 only).
"""
import copy
import warnings
from collections import OrderedDict
import numpy as np
import scipy.sparse
import torch
from torch import nn

from . import torch as ktorch
from . import sparse as ksp
from . import layer as klayer
from . import _capi
from .globals import verbose
from .util import find_closest_positive_divisor
from .sparse import sparse_identity_matrix
from .keys import keygen, diagonal_affine_to_linear   # noqa: F401  (re-exported: the reference exposes keygen from keynet.system)


class KeyedModel(object):
    """The keyed network: an nn.Sequential of KeyedLayer / nn.ReLU plus the two end keys (keynet/system.py:26-157)."""

    def __init__(self, net, inshape, inkey, f_layername_to_keypair, f_module_to_keyedmodule=None, do_output_encryption=False):
        """net: source nn.Module with uniquely named children ('reluN' after a linear layer, '<layer>_bn' batch norms,
        'dropoutN'); inkey: decryption key of the sensor (= Ainv of the first layer); f_layername_to_keypair(name, outshape)
        -> (A, Ainv) draws one key pair per traced layer, in trace order; f_module_to_keyedmodule is the layergen seam."""
        net.eval()
        chain = self._trace(net, inshape)
        (keys, last) = self._draw_keys(chain, inkey, f_layername_to_keypair, do_output_encryption)
        self._keynet = nn.Sequential(self._key_layers(net, chain, keys, f_module_to_keyedmodule))
        self._embeddingkey = keys[last]['outinv'] if do_output_encryption else None
        self._imagekey = inkey
        self._layernames = set(name for (name, _) in net.named_children())
        self._outshape = chain['output']['outshape']

    @staticmethod
    def _trace(net, inshape):
        """Shape trace with the identity layers spliced out of the prev/next links.  The dropout ENTRIES stay in the table
        (the reference's filter at keynet/system.py:35 tests whether the layer name is a substring of 'dropout', which
        real names such as 'dropout0' are not), so each of them still draws a key pair below: part of RNG parity."""
        chain = ktorch.netshape(net, inshape)
        marker = 'dropout'
        chain = OrderedDict((k, v) for (k, v) in chain.items() if k not in marker)
        for v in chain.values():
            if v['nextlayer'] is not None and marker in v['nextlayer']:
                v['nextlayer'] = chain[v['nextlayer']]['nextlayer']
            elif v['prevlayer'] is not None and marker in v['prevlayer']:
                v['prevlayer'] = chain[v['prevlayer']]['prevlayer']
        return chain

    @staticmethod
    def _draw_keys(chain, inkey, draw, do_output_encryption):
        """name -> {'A': output key (None on the last layer unless the output is encrypted), 'Ainv': inverse of the key on
        the layer's input, 'outinv': inverse of its own output key}.  One draw per traced layer, in trace order."""
        last = chain['output']['prevlayer']
        pairs = OrderedDict((k, draw(k, v['outshape'])) for (k, v) in chain.items() if k not in ('input', 'output'))
        keys = {}
        for (k, (A, Ainv)) in pairs.items():
            prev = chain[k]['prevlayer']
            keys[k] = {'A': A if (k != last or do_output_encryption) else None, 'Ainv': inkey if prev == 'input' else pairs[prev][1], 'outinv': Ainv}
        return (keys, last)

    @staticmethod
    def _key_layers(net, chain, keys, make):
        """Walk the children and emit the keyed sequence.  A linear layer followed by a ReLU (or a '<name>_bn' batch norm)
        is keyed together with it, using the follower's output key; Dropout vanishes."""
        out = OrderedDict()

        def rekeyed(follower, target):
            # output key of `target` as seen through `follower`:  (A_f . A_f_in^-1) . A_target
            return keys[follower]['A'].dot(keys[follower]['Ainv']).dot(keys[target]['A'])

        for (name, m) in net.named_children():
            if verbose():
                print('[keynet_amd.KeyedModel]: keying "%s"' % name)
            assert name in keys and name in chain, 'layer "%s" was not reached by the shape trace' % name
            node = chain[name]
            if isinstance(m, nn.Dropout):
                continue
            if isinstance(m, nn.BatchNorm2d):
                host = name.split('_')[0]
                assert '_bn' in name and node['prevlayer'] == host, 'a batch norm must be named "<layer>_bn" and follow "<layer>" directly'
                fused = copy.deepcopy(getattr(net, host))
                (w, b) = ktorch.fuse_conv2d_and_bn(fused.weight, fused.bias, m.running_mean, m.running_var, 1E-5, m.weight, m.bias)
                (fused.weight, fused.bias) = (torch.nn.Parameter(w), torch.nn.Parameter(b))
                out[host] = make(fused, chain[host]['inshape'], node['outshape'], rekeyed(name, host), keys[host]['Ainv'])
            elif isinstance(m, nn.ReLU):
                host = node['prevlayer']
                if '_bn' in host:
                    warnings.warn('ReLU right after the batch norm "%s": it has to be keyed on its own (costly); avoid bn -> relu chains' % host)
                    out[name] = make(m, node['inshape'], node['outshape'], keys[name]['A'], keys[name]['Ainv'])
                else:
                    out[host] = make(getattr(net, host), chain[host]['inshape'], chain[host]['outshape'], rekeyed(name, host), keys[host]['Ainv'])
                    out[name] = copy.deepcopy(m)          # stays a plain ReLU
            else:
                nxt = node['nextlayer']
                if nxt is not None and (nxt == '%s_bn' % name or 'relu' in nxt):
                    continue                               # emitted when its follower is reached
                out[name] = make(m, node['inshape'], node['outshape'], keys[name]['A'], keys[name]['Ainv'])
        return out

    @classmethod
    def fromlayers(cls, layers, outshape, imagekey=None, embeddingkey=None):
        """Assemble from already keyed layers (OrderedDict name -> KeyedLayer | nn.ReLU): public key-nets, fixtures."""
        self = cls.__new__(cls)
        self._keynet = nn.Sequential(OrderedDict(layers))
        (self._embeddingkey, self._imagekey, self._layernames, self._outshape) = (embeddingkey, imagekey, set(layers.keys()), outshape)
        return self

    def __repr__(self):
        return self._keynet.__repr__()

    def __getstate__(self):
        """Whole key-nets are pickled by the reference's users (test/test_keynet.py:106, vipy.util.save): device-side state -- the overlapped
        forward's workspaces and streams, the whole-net kernel's handle -- is dropped and rebuilt on first use (operators: SparseMatrix.__getstate__)."""
        d = dict(self.__dict__)
        self._drop_plans(d)
        return d

    def __setstate__(self, d):
        self.__dict__.update(d)

    def __getattr__(self, attr):
        if attr.startswith('__') or '_keynet' not in self.__dict__:
            raise AttributeError(attr)
        return getattr(self.__dict__['_keynet'], attr)

    # -- the hot path -------------------------------------------------------------------------------------------
    RESCREEN = True              # re-screen the float-key contract on every forward
    RESCREEN_MAX_PASSES = 4
    # A/B switches of the diagnostic tools (tools/ab_rescreen.py) and tests, read here and nowhere else:
    RESCREEN_READ = True         # False: gather the maxima but skip the host read -- what the read itself costs
    OVERLAP_AUTO = True          # False: forward_linear(overlap=None) never chooses the overlapped forward
    CHAIN = True                 # False: the launch-per-layer forward instead of the whole-net kernel

    # -- the launch list: one walk over the key-net's layers, read by everything that launches kernels ------------------------
    def _keyed(self, named=False):
        """The keyed layers in order (named: (name, layer) pairs)."""
        return [(n, c) if named else c for (n, c) in self._keynet.named_children() if isinstance(c, klayer.KeyedLayer)]

    def _steps(self):
        """The key-net in launch order: [(k, layer, relu)] -- keyed layer number k, with `relu` when the unkeyed nn.ReLU behind it is fused into
        its kernel (keynet/system.py:92); a stand-alone nn.ReLU (nothing in front of it to fuse it into) is the step (None, module, False)."""
        (steps, k, fused) = ([], 0, False)
        children = list(self._keynet.children())
        for (i, c) in enumerate(children):
            if isinstance(c, klayer.KeyedLayer):
                fused = (i + 1 < len(children)) and isinstance(children[i + 1], nn.ReLU)
                steps.append((k, c, fused))
                k += 1
            elif isinstance(c, nn.ReLU):
                if not fused:
                    steps.append((None, c, False))
                fused = False
            else:
                raise ValueError('unsupported module in a key-net: %s' % str(type(c)))
        return steps

    def _signature(self):
        """What a cached launch list is valid for: the layers' current (operator, contract) identities."""
        return tuple((id(c.W), getattr(c, '_exact', True)) for c in self._keyed())

    def _drop_plans(self, d=None):
        """Forget the cached launch lists (_overlap_plan, _chain_op): wherever a contract changes, to release their workspaces, and from a pickled state `d`."""
        d = self.__dict__ if d is None else d
        d.pop('_overlap_plans', None)
        d.pop('_chain_ops', None)

    NARROW_MAX = ksp.NARROW_MAX    # forward_linear(narrow=True) takes at most this many images (the channel-lane conv-taps kernel keeps one running sum per image and lane)
    NARROW32_MAX = ksp.NARROW32_MAX    # ... with narrow32=True (convtaps_narrow32_kernel: the columns in blocks of 8 | 16 | 32 running sums per lane)
    NARROW64_MAX = ksp.NARROW64_MAX    # ... with narrow64=True (beyond NARROW32_MAX images convtaps_exact_pipe64_kernel: one column per lane, packed over output-channel pairs)

    def forward_linear(self, img_cipher, overlap=None, narrow=False, narrow_rows=False, narrow32=False, narrow64=False, narrow_linear=False, narrow_split=False, narrow_taps=False, narrow_fill=False):
        """[N, D0+1] -> [N, classes+1]: the nn.Sequential of keynet/system.py:132 with the unkeyed ReLUs fused into the
        producing layer's kernel epilogue.  Stream-ordered on torch's current HIP stream.  Host synchronisation: none for key-nets whose
        layers all run under a DECLARED contract (exact=True: the permutation key-nets; exact=False: forced); a key-net with layers on the
        matrix cores by a CALIBRATION decision (exact='auto': the float-key contract) reads one float per keyed layer back at the end of
        every forward -- max |x| of each such layer, gathered on the device inside the producing kernels (kn_spmm_screen) -- and, when a
        layer's input has outgrown its calibration by more than KeyedLayer.RESCREEN_FACTOR, re-calibrates that layer on this batch and runs
        the batch again.  What that checks (and no more): the batch maximum of each screened layer's input against the maximum the
        decision was calibrated on, with the 2x headroom every accepted decision has (element-wise |d| <= 1e-5 + 1e-5 |ref|, measured on up to 256
        columns of the calibration batch; an unmeasured dense layer is accepted only with its worst-case bound at half the tolerance); NaN activations
        are not screened.  The reference applies one arithmetic on every call (keynet/sparse.py:488-492): only the 'exact' contract IS that arithmetic.
        The first forward of an 'auto' layer calibrates it (host reads).
        Batch sizes (_prepare): an odd device batch of a tiled-conv key-net is padded with zero images to whole 128-image tiles, with the activations
        and workspaces of the padded batch (VGG-16: one image costs what 128 cost, 1.6 GB for its largest layer).  The result: the first N rows of the
        transposed view of a feature-major [classes+1, N'] block (N' = the padded batch); a host batch gets a host tensor.
        `overlap`: run the batch as two half-batch column windows on two side streams, one kernel apart (see _forward_overlapped);
        None = automatically for device-resident feature-major batches that are a multiple of 256 images, False = never.
        Memory: the overlapped forward keeps two ping-pong workspaces of max_rows x N floats per (device, N) plan (VGG-16 at N = 256:
        2 x 3.3 GB) plus two side streams; at most OVERLAP_PLANS_KEPT plans are cached (least recently used dropped),
        release_workspace() drops them all.
        THE NARROW FORMS (low latency, at most 64 images; this is the one place that says what their five keywords mean -- they are resolved once per call into a
        ksp.NarrowForm, ValueError where ksp._narrow_args refuses them: every other keyword only together with `narrow`, no batch beyond the width they allow).  Common to
        all: nothing is padded (but the 64-column tile, below) -- the batch is laid out feature-major once and every layer runs at that width; the overlapped form is never
        taken, the whole-net kernel only where no layer has a narrow form; no layer's wide decision changes, nothing is saved, the cached launch lists are left alone.
        `narrow=True` (1 .. NARROW_MAX images): every conv-taps layer runs the channel-lane order-preserving kernel (KN_FLAG_NARROW), WHATEVER its contract is: the
        reference's own arithmetic on the conv layers -- stored order, separate multiply and add, the bits exact=True gives -- which satisfies every contract, so nothing
        is calibrated, screened, decided or recorded.  The other layers run as they do without the keyword (a layer still undecided: in the reference's order, for this
        call; a non-conv layer a calibration put on the matrix cores stays there and is NOT re-screened by this forward).
        `narrow='mfma'`: the same forward with the conv-taps layers on the matrix-core narrow kernel (KN_FLAG_NARROW_MFMA: an implicit GEMM whose N dimension is
        output pixels x images) WHERE THE LAYER'S CONTRACT IN FORCE ALLOWS RE-ORDERED SUMS (KeyedLayer.narrow_mode): a declared exact=False / 'bf16x3' layer always,
        unscreened; a layer calibration put on a re-ordering kernel after ITS OWN measurement on the first such batch (channel-lane against matrix-core kernel on these
        columns, the rule of _calibrate; recorded under the layer's calibration record as 'narrow'); a layer under True, or still undecided, exactly as narrow=True --
        nothing is decided for it.  Layers accepted by measurement are re-screened on every narrow='mfma' forward like their wide counterparts: max |x| of each comes
        from kn_spmm_screen on its producer (behind the narrow kernels one kn_absmax-style reduction launch per screened layer, one more for the input when the first
        layer is screened), is read back once at the end of the forward, and a layer whose input exceeds RESCREEN_FACTOR x its narrow record's max_abs_x drops that
        record, is measured again on this batch, and the batch runs again (_screen, _rescreen).
        `narrow32=True`: up to NARROW32_MAX images.  Beyond NARROW_MAX the conv-taps layers run convtaps_narrow32_kernel (narrow=True: the bits of exact=True, as at
        1 .. 8) or the matrix-core narrow kernel at 16 | 32 columns per pixel (narrow='mfma': per image the bits of narrow='mfma' on that image; a calibrated layer is
        measured on the 8 images that hold the batch's largest |x| and screened as at 1 .. 8).
        `narrow64=True`: up to NARROW64_MAX images.  It implies `narrow32` -- a service passes one set of keywords for any batch of at most 64 images, and at NARROW32_MAX
        images and fewer the call is exactly narrow32=True.  Beyond, the conv-taps layers run the order-preserving pipeline with one image per lane (KN_FLAG_NARROW64:
        convtaps_exact_pipe64_kernel, half the packed instructions per step of the padded 128-image tile; a filled-in operator runs what exact=True runs at that width) --
        the bits of exact=True under every contract, so the forward of a key-net under the bit-exact contract equals the padded one bit for bit; nothing is calibrated,
        screened, decided or recorded.  narrow='mfma' with narrow64=True is a ValueError at 33 .. 64 images (True asks for the order-preserving form of that width).
        `narrow64='mfma'` (only together with narrow='mfma'): the matrix-core forward of 33 .. 64 images; at NARROW32_MAX images and fewer exactly narrow='mfma',
        narrow32=True, bit for bit.  Beyond, the batch is zero-padded to 64 columns (_prepare64; the argument of _prepare's padding: an image's logits are the same in any
        batch, zero images raise no layer's max |x|), and a conv-taps layer whose contract in force is False or 'bf16x3' runs the f32 tile kernel on 64-column tiles
        (KN_FLAG_NARROW64_MFMA: convtaps_mfma_kernel<MT, NB=64>; there is no bf16 form at this width) -- per image the bits the padded forward's f32 tiles give it, half
        the matrix work of the 128-column tile the padded forward runs half empty.  A conv-taps layer under True, still 'auto', or decided 'split' runs what narrow64=True
        runs, so a key-net with no layer on a re-ordering contract returns the bits of narrow=True, narrow64=True.  The screen: the 64-column tile is the WIDE kernel's
        association, so a declared layer is unscreened and a layer calibration put there is re-screened against its WIDE record (not the narrow one, which belongs to
        the other kernel), through the same slots and RESCREEN_FACTOR.  A tripped layer goes back to 'auto' as on the wide path (launch lists dropped), this pass runs
        again with that layer in the stored order, and the next padded forward calibrates it: nothing calibrates inside this path.
        `narrow_rows=True` (at most NARROW_MAX images, whatever `narrow32` / `narrow64` allow): the layers that are float32 CSR operators in the stored order -- keyed
        Linear layers under the bit-exact contract, pools, every layer of an untiled key-net -- run the row-lane kernel (KN_FLAG_NARROW_ROWS: the lane is the output row,
        the images its running sums) instead of the wide-batch CSR kernels.  The same bits layer by layer; orthogonal to which conv kernel `narrow` selects.
        `narrow_linear=True` (at every width the other keywords allow): the keyed Linear layers under the bit-exact contract -- float32 CSR operators in the stored order
        that hold big pattern groups -- run csr_stream_group_kernel (KN_FLAG_NARROW_LINEAR: a workgroup owns 64 output rows times all images, the values reach it through
        a ring in LDS and leave HBM once per call) instead of the wide-batch kernel, which costs 64 images at every width.  The same bits layer by layer; next to
        `narrow_rows` the other CSR layers and the remaining rows of a Linear keep the row-lane kernel.
        `narrow_split=True` (opt-in; only together with narrow='mfma', ValueError otherwise; 1 .. NARROW_MAX images, to NARROW32_MAX with `narrow32`): the FILLED-IN conv layers
        whose contract in force is 'split' (doubly-stochastic keys: 500 - 5 400 slots per output pixel) run the narrow split route instead of the fused operator on the
        channel-lane kernel, which is all narrow='mfma' has for them (more than two slots on a (pixel, tap) pair: no matrix-core narrow form).  The route
        (Conv2dTiledMatrix._torchdot_split_narrow): X [Cin x HiWi, n] -> Xt [HiWi, Cin x n] (kn_planes_to_columns), ONE stored-order product of the spatial CSR at Cin x n
        columns, back to planes (kn_columns_to_planes), then the 9-slot channel-mixing operator on the matrix-core narrow kernel.  Taken where the operator's cost rule offers it at
        this width (narrow_split_capable) and the second step plans the matrix-core narrow kernel; a layer declared 'split' runs it unscreened, a layer CALIBRATION decided
        'split' after its own measurement on the first such batch (KeyedLayer.narrow_split_mode: channel-lane kernel against the route on these columns, _calibrate's rule),
        recorded under the calibration record's own key 'narrow_split' and re-screened on every narrow_split forward like a narrow record (a trip drops only that record).
        Every other layer -- and a layer calibration sent to 'exact', which stays on the channel-lane kernel -- is what narrow='mfma' makes it, bit for bit; at 33 .. 64
        images (narrow64) the keyword changes nothing.  Workspaces: Xt, Z' and Z per (layer, device, width class 8 | 32), allocated by the first forward of a class
        and kept (release_workspace() drops them); calls that share a layer are ordered by their stream.
        `narrow_taps=True` (opt-in; only together with narrow=True | 'mfma', ValueError otherwise; every width those keywords allow, in effect up to NARROW_MAX images): the
        conv layers that run the channel-lane kernel run convtaps_narrow_taps_kernel instead (KN_FLAG_NARROW_TAPS: slot lists in scalar registers, an input channel's value
        rows of all taps in vector registers) where the operator is eligible -- every conv layer of the tiled permutation / identity key-nets; filled-in layers are not.
        Nothing is calibrated, recorded or screened: the bits are those of the same call without the keyword.
        `narrow_taps='packed'` (opt-in, the same argument rule): up to NARROW_MAX images exactly narrow_taps=True; with narrow32=True (or narrow64=True) at NARROW_MAX + 1 ..
        NARROW32_MAX images the eligible conv layers run convtaps_narrow_taps32_kernel in place of convtaps_narrow32_kernel (KN_MODIFIER_NARROW_TAPS32: the same resident
        slot lists and value rows, a step's activations as 16-float scalar segments, packed f32 multiplies and adds, each element rounded as before) -- the same bits;
        beyond NARROW32_MAX images it changes nothing.  Operators with coefficients have the 8-column-block forms only and keep convtaps_narrow32_kernel elsewhere.
        `narrow_taps='pairs'` (opt-in, the same argument rule): beyond NARROW_MAX images exactly narrow_taps='packed', so one set of keywords serves any batch; up to
        NARROW_MAX images the eligible conv layers of more than 64 output channels run convtaps_narrow_taps_pairs_kernel in place of convtaps_narrow_taps_kernel
        (KN_MODIFIER_NARROW_TAPS_PAIRS: a lane holds two output channels as the halves of a register pair, a step's scalar half is paid once for 128 channels, packed
        f32 multiplies and adds, each element rounded as before) -- the same bits.  Nothing is calibrated, recorded or screened for it.
        `narrow_fill=True` (opt-in; only together with narrow=True | 'mfma', ValueError otherwise; every width those keywords allow, in effect up to NARROW32_MAX images): the
        FILLED-IN conv layers that run the channel-lane kernels in the reference's order -- under doubly-stochastic keys the layers calibration sends to `exact`, and every
        layer of a key-net declared exact=True -- run convtaps_narrow_fill_kernel instead (KN_FLAG_NARROW_FILL: the pixel's slot records streamed by scalar loads, an input
        channel's value rows of all taps in vector registers, one multiply and one add per slot); up to 32 images in blocks of 8.  The first such call of a layer builds
        its record table on the device (16 bytes per slot).  It combines freely with the other keywords (with narrow_split=True it reaches the layers not on the route);
        nothing is calibrated, recorded or screened: the bits are those of the same call without the keyword."""
        (form, x, windows) = self._resolve(img_cipher, (narrow, narrow_rows, narrow32, narrow64, narrow_linear), narrow_split=narrow_split, narrow_taps=narrow_taps, narrow_fill=narrow_fill)
        y = self._forward_passes(x, windows, False if form.mode else overlap, form)[0][:img_cipher.shape[0]]
        return y if img_cipher.is_cuda else y.to(img_cipher.device)

    def _resolve(self, x, keywords, own=False, narrow_split=False, narrow_taps=False, narrow_fill=False):
        """The narrow keywords of forward_linear / capture (in the order of their signatures) on the batch x, once per call: (form, block, windows) -- the ksp.NarrowForm
        everything below reads (ValueError where the argument rule refuses the keywords) and the block the passes run on, _prepare64's where the form takes the 64-column
        tile, else _prepare's.  `own` (capture): a block of the call's own, never x's memory -- the graph's input.
        `narrow_split`, `narrow_taps`, `narrow_fill`: the opt-in sixth, seventh and eighth keywords, carried by the form (NarrowForm.split, .taps, .fill)."""
        form = ksp.NarrowForm.of(x.shape[0], *keywords, narrow_split=narrow_split, narrow_taps=narrow_taps, narrow_fill=narrow_fill)
        if own:
            x = x.detach().float() if form.mode else x.detach()
            x = x if form.tile64 else x.t().clone(memory_format=torch.contiguous_format).t()
        return (form,) + (self._prepare64(x) if form.tile64 else self._prepare(x, form.mode))

    @staticmethod
    def _narrow64_form(n, narrow64):
        """The normalised `narrow64` of a batch of n images, as NarrowForm.keywords() hands it on: 'mfma' beyond NARROW32_MAX images only (at fewer, narrow64='mfma' is exactly narrow64=True, i.e. narrow32), else a bool."""
        return 'mfma' if (narrow64 == 'mfma' and n > ksp.NARROW32_MAX) else bool(narrow64)

    def frame_shape(self):
        """(C, H, W) of the images this key-net takes: the input shape of its first keyed layer."""
        keyed = self._keyed()
        shape = tuple(int(v) for v in keyed[0]._inshape)[-3:] if keyed and keyed[0]._inshape is not None else ()
        if len(shape) != 3:
            raise ValueError('this key-net does not record the shape of its input images')
        return shape

    def frames_pad_to(self, narrow=False):
        """What an ingest pads a batch to so that _prepare takes the block in place: whole BATCH_TILE tiles on the wide path of a tiled-conv key-net, otherwise nothing."""
        wide_tiled = not narrow and any(isinstance(c.W, ksp.Conv2dTiledMatrix) for c in self._keyed())
        return int(self.BATCH_TILE) if wide_tiled else 1

    def check_cipher_frames(self, cipher_frames, lo, hi, layout='NHWC'):
        """n of a batch of quantised encrypted frames (uint8 | uint16, this key-net's image shape) with their ranges lo, hi: float32 [n] on the frames' device.
        ValueError otherwise.  No GPU call."""
        (n, chw) = ktorch.frame_shape(cipher_frames, layout, ktorch.FRAME_DTYPES)
        if chw != self.frame_shape():
            raise ValueError('frames of shape (C, H, W) = %s do not fit the key-net\'s input %s' % (str(chw), str(self.frame_shape())))
        ktorch.check_range(cipher_frames, lo, hi, n)
        return n

    def forward_frames(self, cipher_frames, lo, hi, layout='NHWC', **keywords):
        """Quantised ENCRYPTED frames on the device (what KeyedSensor.encrypt_to_frames returns: uint8 | uint16 [n, H, W, C], or [n, C, H, W] with layout='NCHW', and
        their ranges lo, hi: float32 [n]) -> [n, classes+1]: the server's call.  It needs no sensor and no image key: the ranges are those of the encrypted images.
        ktorch.gray_inverse (levels from the frames' dtype), the dequantising ingest ktorch.frames_to_linear (padded to whole BATCH_TILE tiles on the wide path of a
        tiled-conv key-net, as StreamedForward's), then forward_linear with `keywords`.  ValueError for a wrong dtype, rank, layout or shape, or for lo / hi that are not
        float32 [n] on the frames' device, before any GPU call."""
        n = self.check_cipher_frames(cipher_frames, lo, hi, layout)
        if not cipher_frames.is_cuda:
            raise ValueError('forward_frames takes frames that are on the device (StreamedForward brings host frames there)')
        (scale, offset) = ktorch.cipher_range(cipher_frames, lo, hi, n)
        x = ktorch.frames_to_linear(cipher_frames, layout=layout, pad_to=self.frames_pad_to(bool(keywords.get('narrow'))), scale=scale, offset=offset)
        return self.forward_linear(x, **keywords)[:n]

    def _prepare64(self, x):
        """(x, windows) of a narrow64='mfma' forward of 33 .. 64 images: one feature-major float32 device block of NARROW64_MAX columns, the images beyond the batch zero
        (the straight-line loaders of the 64-column tile take whole aligned tiles, and the stores are wide).  _prepare is not involved."""
        x = x.detach().float()
        if not x.is_cuda:
            x = x.cuda()
        xp = torch.zeros((x.shape[1], self.NARROW64_MAX), dtype=torch.float32, device=x.device).t()
        xp[:x.shape[0]] = x
        return (xp, [(0, self.NARROW64_MAX)])

    def _prepare(self, x, narrow=False):
        """What the kernels get to see: (x, windows), the image ranges of the passes.  A host batch goes to the device ONCE (the layers chain
        there; the screen sees them).  A float32 device batch of a tiled-conv key-net becomes one feature-major block of whole BATCH_TILE tiles
        (ragged conv-taps forms are slow: VGG-16, stored order, 186 ms at 64 images against 72 ms at 128, profiles/r06_vgg16_other_batches.txt;
        zero images raise no layer's max |x|; feature-major memory takes the overlapped form: 58.7 -> 57.0 ms at 256, tools/layout_time.py).
        The fast loaders take 32-bit element offsets: a batch whose largest layer would hold MAX_BLOCK_ELEMENTS activations runs as passes of the
        largest multiple of 256 images that keeps every layer inside (VGG-16 at 1 024 images: conv1_2 113.7 ms against 2 x 31 for two passes of 512);
        each pass copies its window into a block of its own (a padded batch is then held twice while the passes run).  Anything else -- float64,
        an untiled key-net, no image -- passes through as one window.  `narrow` (forward_linear): never padded or split, laid out feature-major once."""
        if not x.is_cuda and x.dim() == 2 and torch.cuda.is_available():
            x = x.detach().float().cuda()
        n = x.shape[0]
        dev32 = x.is_cuda and x.dim() == 2 and x.dtype == torch.float32
        keyed = None if narrow else self._keyed()
        if narrow or not (dev32 and n > 0 and any(isinstance(c.W, ksp.Conv2dTiledMatrix) for c in keyed)):
            if narrow and dev32 and not x.t().is_contiguous():
                x = x.detach().t().contiguous().t()              # every layer hands the next one such a block
            return (x, [(0, n)])
        npad = -(-n // self.BATCH_TILE) * self.BATCH_TILE
        chunk = (self.MAX_BLOCK_ELEMENTS - 1) // max(max(c.W.shape) for c in keyed) // 256 * 256
        windows = [(lo, min(lo + chunk, npad)) for lo in range(0, npad, chunk)] if 0 < chunk < npad else [(0, npad)]
        if len(windows) > 1:
            self._chunked_forwards = getattr(self, '_chunked_forwards', 0) + 1
        if npad > n:
            xp = torch.zeros((x.shape[1], npad), dtype=torch.float32, device=x.device).t()
            xp[:n] = x.detach()
            x = xp
            self._padded_forwards = getattr(self, '_padded_forwards', 0) + 1
        elif len(windows) == 1 and not x.t().is_contiguous():
            x = x.detach().t().contiguous().t()
        return (x, windows)

    def _forward_passes(self, x, windows, overlap, form):
        """The screened forward of a prepared batch under the ksp.NarrowForm `form`: (y, screens).  A pass whose screen re-calibrates a layer runs again (calibrating on its
        own images), then every other pass again: the batch comes out of ONE set of contracts.  At most RESCREEN_MAX_PASSES runs of a pass; then only the last pass is
        re-screened (the next forward decides).  Under a HIP-graph capture nothing is read: `screens` = the arguments of _rescreen per pass, for capture's replay.
        Which layers are screened, and against what: _screen; records made during a pass were measured on this very batch, so only those that existed before it are screened."""
        keyed = self._keyed()
        on_dev = x.is_cuda and x.dim() == 2
        read = on_dev and not torch.cuda.is_current_stream_capturing() and self.RESCREEN_READ
        ys = [None] * len(windows)
        (todo, screens, redos) = (list(range(len(windows))), [], 0)
        while todo:
            k = todo.pop(0)
            (screened, narrow) = self._screen(form, keyed) if on_dev and self.RESCREEN else (set(), False)
            slots = torch.zeros(len(keyed) + 1, dtype=torch.float32, device=x.device) if screened else None
            (lo, hi) = windows[k]
            # (a window of a wider block: its own feature-major block, so that the pass can take the overlapped form)
            ys[k] = self._forward_once(x if len(windows) == 1 else x[lo:hi].t().contiguous().t(), keyed, overlap, slots, screened, form)
            if slots is None:
                continue
            screens.append((slots, screened, narrow))
            if not read or (todo and redos + 1 == self.RESCREEN_MAX_PASSES):
                continue
            if self._rescreen(slots.tolist(), keyed, screened, narrow) and redos + 1 < self.RESCREEN_MAX_PASSES:
                redos += 1
                todo = [k] + [j for j in range(len(windows)) if j != k]
        return (ys[0] if len(ys) == 1 else torch.cat([y.t() for y in ys], dim=1).t(), screens)

    @staticmethod
    def _screen(form, keyed):
        """The per-forward screen under `form`: (screened, narrow) -- the indices of the keyed layers whose input this forward checks, and the record it checks them against
        with what a trip does (_rescreen).  narrow=True: the conv layers run the reference's own arithmetic -- nobody, whatever the other layers are.  narrow='mfma': the
        layers a MEASUREMENT put on the matrix-core narrow kernel, against their narrow records (`narrow`: a trip drops that record, the layer is measured again on this
        batch; an 'auto' layer does not switch the screen off, it runs in the reference's order for this call).  The 64-column tile: the conv-taps layers a CALIBRATION put
        on the f32 / bf16x3 matrix-core kernels -- the wide kernel's association -- against their WIDE records, a trip as on the wide forward.  The wide forward: every layer
        on a re-ordering kernel by calibration, once no layer is 'auto' any more; a trip sends the layer back to 'auto' and drops the launch lists."""
        if form.tile64:
            return (set(j for (j, c) in enumerate(keyed) if c.screened() and isinstance(c.W, ksp.Conv2dTiledMatrix) and c.W.narrow_capable() and c._exact in (False, 'bf16x3')), False)
        if form.mode:
            if form.split:      # narrow_split=True: also the layers a measurement put on the narrow split route, against THAT record ('split': KeyedLayer._screen_key)
                return (set(j for (j, c) in enumerate(keyed) if c.narrow_screened() or c.narrow_split_screened()), 'split')
            return (set(j for (j, c) in enumerate(keyed) if c.narrow_screened()) if form.mode == 'mfma' else set(), True)
        if any(getattr(c, '_exact', True) == 'auto' for c in keyed):
            return (set(), False)
        return (set(j for (j, c) in enumerate(keyed) if c.screened()), False)

    def _rescreen(self, xmax, keyed, screened, narrow=False):
        """Host side of the per-forward screen: layers whose input magnitude has outgrown their calibration go back to 'auto' (decided
        again by the next forward, on that batch).  Returns their indices.  `narrow`: the screen of a narrow='mfma' forward -- against the layers' NARROW
        records; an outgrown one is dropped (measured again by the next narrow='mfma' pass, on that batch), the wide decision and the launch lists stay.  narrow='split' (a
        narrow_split=True forward): a layer on the narrow split route is checked against its narrow_split record, and a trip drops that record alone."""
        redo = [k for k in sorted(screened) if keyed[k].rescreen(xmax[k], narrow=narrow)]
        for k in redo:
            klayer._log.info('keynet_amd: %s: max |x| = %.3g against %.3g at %s: re-calibrating on this batch', keyed[k]._repr, xmax[k], keyed[k].screen_record(narrow)['max_abs_x'],
                             ('its narrow split measurement' if keyed[k]._screen_key(narrow) == 'narrow_split' else 'its narrow measurement') if narrow else 'calibration')
            keyed[k].unscreen(narrow)
        if redo:
            count = '_narrow_remeasurements' if narrow else '_recalibrations'
            self.__dict__[count] = self.__dict__.get(count, 0) + len(redo)
            if not narrow:
                self._drop_plans()
        return redo

    BATCH_TILE = 128           # _prepare pads a device batch of a tiled-conv key-net to whole multiples of this many images
    MAX_BLOCK_ELEMENTS = 1 << 31   # ... and splits a batch whose largest layer would hold this many activations or more into passes

    def _forward_once(self, img_cipher, keyed, overlap, slots, screened, form):
        """One pass over the keyed layers `keyed` (_keyed()).  `slots` (device f32 [L + 1], zeroed) / `screened` (indices of the keyed layers whose contract
        is re-screened): slot k receives max |x| of keyed layer k -- slot 0 by one pass over the input, slot k + 1 by the kernel that
        produces layer k's output.  `form` (ksp.NarrowForm): narrow, every layer in its narrow form (KeyedLayer.forward) and the whole-net kernel only where no layer has one."""
        forced = overlap is True
        if overlap is None and not self.OVERLAP_AUTO:
            overlap = False
        if any(getattr(c, '_exact', True) == 'auto' for c in keyed):
            overlap = False        # first forward of an 'auto' key-net: the layers calibrate their contract one by one (KeyedLayer._calibrate)
        if overlap is None:
            overlap = (img_cipher.is_cuda and img_cipher.dtype == torch.float32 and img_cipher.dim() == 2 and img_cipher.shape[0] >= 256 and
                       img_cipher.shape[0] % 256 == 0 and img_cipher.t().is_contiguous() and not torch.cuda.is_current_stream_capturing())
        if not forced and img_cipher.is_cuda and img_cipher.dim() == 2 and not screened and not (form.mode and any(c.W.narrow_capable() for c in keyed)):
            chain = self._chain_op(img_cipher.device)
            if chain is not None:
                return self._forward_chain(img_cipher, chain)
        if slots is not None and 0 in screened:
            klayer._absmax_into(img_cipher.detach().t().float(), slots[0:1])
        if overlap:
            plan = self._overlap_plan(img_cipher.device, img_cipher.shape[0], force=forced)
            if plan is not None and img_cipher.is_cuda and img_cipher.dtype == torch.float32 and img_cipher.t().is_contiguous():
                return self._forward_overlapped(img_cipher.detach(), plan, slots, screened)
        (y, keywords) = (img_cipher, form.keywords())
        for (k, c, relu) in self._steps():
            if k is None:
                y = _relu_block(y)
            else:
                y = c.forward(y, fuse_relu=relu, absmax=slots[k + 1:k + 2] if (slots is not None and (k + 1) in screened) else None, **keywords)
        return y

    # -- whole-net kernel: every operator of a small untiled key-net in ONE launch, activations in LDS (csrc/kn_chain.hip) --------
    CHAIN_LDS_BYTES = 160 * 1024
    CHAIN_MAX_OPS = 12

    def _chain_op(self, device):
        """kn_chain_create handle for this key-net on `device`, or None when it does not qualify: every layer a keyed layer under the
        bit-exact contract whose operator is a plain / tiled CSR container in float32 (KeyedLayer.launch), every ReLU fusable into its producer, at most 12 operators,
        and the activations of four batch columns of any two consecutive layers within the CU's 160 KiB of LDS (LeNet_AvgPool: 92 KB).
        KeyedModel.CHAIN = False selects the launch-per-layer forward instead."""
        if not self.CHAIN:
            return None
        sig = self._signature()
        cache = self.__dict__.setdefault('_chain_ops', {})
        hit = cache.get(device.index)
        if hit is not None and hit[0] == sig:
            return hit[1]
        if torch.cuda.is_current_stream_capturing():
            return None                  # building the chain allocates: not inside a HIP-graph capture (KeyedModel.capture runs an eager forward first)
        op = None
        launches = [None if k is None else c.launch(device, relu) for (k, c, relu) in self._steps()]
        if 0 < len(launches) <= self.CHAIN_MAX_OPS and all(la is not None and la.exact and not la.is_conv for la in launches):
            feat = [0, 0]
            for (l, la) in enumerate(launches):
                feat[l & 1] = max(feat[l & 1], la.cols)
                feat[(l & 1) ^ 1] = max(feat[(l & 1) ^ 1], la.rows)
            if (feat[0] + feat[1] + 1) * 16 <= self.CHAIN_LDS_BYTES and all(launches[l].cols == launches[l - 1].rows for l in range(1, len(launches))):
                try:
                    with torch.cuda.device(device):
                        op = _capi.Operator.chain([la.op for la in launches], [la.flags & _capi.KN_FLAG_RELU for la in launches])
                except _capi.KeynetHipError as e:
                    # the launch-per-layer forward computes the same thing (bit for bit): a device without 160 KiB of LDS per workgroup, or
                    # no memory left for the packed copy, must not fail the forward.  The failure is cached: no rebuild on every call.
                    klayer._log.warning('keynet_amd: whole-net kernel unavailable for this key-net (%s); using one launch per layer', e)
                    op = None
        cache[device.index] = (sig, op)
        return op

    def _forward_chain(self, x, chain):
        """[N, D0+1] -> [N, classes+1] through the whole-net kernel; stream-ordered on torch's current HIP stream."""
        (rows, cols) = chain.shape()
        assert x.shape[1] == cols, 'Non-conformal shape for the key-net input: %s' % str(tuple(x.shape))
        xt = ksp._device_block(x.t())
        n = xt.shape[1]
        y = torch.empty((rows, n), dtype=torch.float32, device=xt.device)
        with torch.cuda.device(xt.device):
            chain.spmm(xt.data_ptr(), n, n, y.data_ptr(), n, _capi.KN_FLAG_EXACT, torch.cuda.current_stream().cuda_stream)
        return y.t()

    # -- overlapped forward: two half-batch column windows on two HIP streams, one kernel apart ---------------------------------
    OVERLAP_MIN_MACS = 2e11      # below this much work per forward the launches are too short for the overlap to pay (LeNet: launch-bound)
    OVERLAP_PLANS_KEPT = 2       # least-recently-used plans beyond this are dropped (a service that sees many batch sizes must not pile up workspaces)

    def _overlap_plan(self, device, batch, force=False):
        """Launch list (KeyedLayer.launch of every step) + segments for the overlapped forward, or None when this key-net / batch does not
        qualify.  A layer is run per half only if the half batch keeps it on the same kernel instantiation as the whole batch (conv tiles are
        128 or 256 batch columns wide) and it is a matrix-core conv layer; see the segment rule below."""
        key = (device.index, batch, bool(force))
        plans = self.__dict__.setdefault('_overlap_plans', OrderedDict())
        sig = self._signature()
        if key in plans and plans[key][0] == sig:
            plans.move_to_end(key)
            return plans[key][1]
        plans.pop(key, None)
        plan = None
        half = batch // 2
        if (force or self._macs_per_image() * batch >= self.OVERLAP_MIN_MACS) and batch % 8 == 0 and half % 128 == 0:
            (steps, halves) = ([], [])           # halves[k]: the half batch keeps step k on the whole batch's kernel instantiation
            for (k, c, relu) in self._steps():
                la = None if k is None else c.launch(device, relu)
                if la is None:
                    # a ReLU that could not be fused into a producer, a layer still to calibrate, one applied in two steps (Conv2dTiledMatrix._split_ops),
                    # a float64 operator (returns float64 blocks): layer by layer on the simple path
                    steps = []
                    break
                ok = True
                if la.is_conv:
                    # order-preserving conv kernels: 256-column tiles (four batch columns per lane).  They also have a 128-column form (two per lane), but
                    # that one is 5-8 % slower per layer (round 5, same-process A/B on every VGG-16 layer shape: conv5_1 4.08 against 3.88 ms) and the
                    # bit-exact forward of 256 images as two overlapped 128-column windows lost 11 % (1 884 against 2 107 images/s): not split.  MFMA tiles
                    # are 128 (Cout > 64) or 256 columns wide: this mirrors MfmaChoice::nb, the tile rule of mfma_choice in csrc/kn_conv.hip
                    ok = (half % 256 == 0) if la.exact else (half % (128 if c.W._outshape[0] > 64 else 256) == 0)
                    if la.flags & _capi.KN_FLAG_BF16X3:
                        with torch.cuda.device(device):          # kn_spmm_plan checks the current device like kn_spmm does
                            if 'bf16x3' in la.op.plan(batch, _capi.KN_FLAG_BF16X3) and 'bf16x3' not in la.op.plan(half, _capi.KN_FLAG_BF16X3):
                                ok = False     # (cannot happen with 128-column tiles; kept as a guard: a half batch must keep the kernel family)
                steps.append(la)
                halves.append(ok)
            if steps:
                # ONE split region: from the first layer after which every layer keeps its kernel instantiation on a half batch (VGG at 256
                # images: conv1_1 / conv1_2 need 256-wide tiles and run whole) up to the trailing fully connected layers (too small to fill
                # the chip per half: whole again after the join).  Measured alternatives: joining the streams at every pooling layer so
                # that the pools run whole (a half-batch window halves their gathered row segments: pool1_2 0.93 ms as two halves against
                # 0.79 ms whole) exposes two drains per conv run and is SLOWER than the plain forward (58.96 vs 58.34 ms); nets without
                # matrix-core conv layers have short-lived workgroups and gain nothing (AllConvNet at 4096 images: 108.7 k images/s
                # overlapped vs 109.2 k plain), so for them the plain forward is used.
                join_at = len(steps)
                while join_at > 0 and steps[join_at - 1].is_linear:
                    join_at -= 1
                split_at = join_at
                while split_at > 0 and halves[split_at - 1]:
                    split_at -= 1
                mfma = any(la.is_conv and not (la.flags & _capi.KN_FLAG_EXACT) for la in steps[split_at:join_at])
                segs = []
                if join_at - split_at >= 2 and (mfma or force):
                    segs = [sg for sg in (('whole', 0, split_at), ('split', split_at, join_at), ('whole', join_at, len(steps))) if sg[2] > sg[1]]
                if any(sg[0] == 'split' for sg in segs):
                    rows_max = max(la.rows for la in steps)
                    plan = dict(steps=steps, segments=segs,
                                bufs=[torch.empty(rows_max * batch, dtype=torch.float32, device=device) for _ in range(2)],
                                streams=[torch.cuda.Stream(device=device), torch.cuda.Stream(device=device)])
        plans[key] = (sig, plan)
        while len(plans) > self.OVERLAP_PLANS_KEPT:      # each plan holds two workspaces of max_rows x batch floats (VGG-16 at 256 images: 2 x 3.3 GB)
            plans.popitem(last=False)
        return plan

    def _macs_per_image(self):
        """Multiply-adds per image of the keyed forward from the host descriptions (factored conv operators count their expansion)."""
        total = 0.0
        for W in (c.W for c in self._keyed()):
            if isinstance(W, ksp.Conv2dTiledMatrix) and W._taps is not None:
                total += float(len(W._taps['ent_out'])) * W._outshape[0] * W._inshape[0]
            else:
                total += float(W.nnz())
        return total

    def release_workspace(self):
        """Drop the activation workspaces and side streams of the overlapped forward (two ping-pong blocks per batch size), and the Xt / Z' / Z workspaces of the narrow
        split route (per layer, device and width class)."""
        self._drop_plans()
        for c in self._keyed():
            if isinstance(c.W, ksp.Conv2dTiledMatrix):
                c.W.release_narrow_split_workspace()

    def _forward_overlapped(self, x, plan, slots=None, screened=()):
        """x: [N, D0+1] whose transpose is a contiguous feature-major block.  Layers ping-pong between two flat workspaces with the
        SAME leading dimension N, so a stream that owns the column window [c0, c0 + N/2) only ever touches addresses congruent to
        that window modulo N -- the two streams never alias, whatever the layers' row counts.  Stream 1 starts one kernel behind
        stream 0: the two streams' launch boundaries then never coincide, and the workgroups one stream has queued take over the
        CUs that the other stream's draining kernel frees (the drain of a launch costs ~0.3 ms of a 6.5 ms conv layer otherwise).
        Same kernels, same per-column arithmetic: bit-identical to the single-stream forward."""
        (steps, segs, bufs, side) = (plan['steps'], plan['segments'], plan['bufs'], plan['streams'])
        N = x.shape[0]
        half = N // 2
        main = torch.cuda.current_stream(x.device)
        ptr0 = x.t().data_ptr()
        n = len(steps)

        def src_of(k):
            return ptr0 if k == 0 else bufs[(k - 1) % 2].data_ptr()

        def slot_of(k):            # where step k's kernel leaves max |y| (= max |x| of keyed layer k + 1), when that layer is screened
            return (slots.data_ptr() + 4 * (k + 1)) if (slots is not None and (k + 1) in screened) else None

        with torch.cuda.device(x.device):
            if plan.get('done') is not None:
                main.wait_event(plan['done'])                      # the workspaces are shared by successive calls, whatever stream they come from
            for (kind, k0, k1) in segs:
                if kind == 'whole':
                    for k in range(k0, k1):
                        steps[k].op.spmm(src_of(k), N, N, bufs[k % 2].data_ptr(), N, steps[k].flags, main.cuda_stream, absmax_ptr=slot_of(k))
                    continue
                for st in side:
                    st.wait_stream(main)
                for k in range(k0, k1 + 1):
                    for (h, st) in enumerate(side):
                        kk = k - h                                 # stream 1 runs one kernel behind stream 0
                        if kk < k0 or kk >= k1:
                            continue
                        steps[kk].op.spmm(src_of(kk) + 4 * half * h, N, half, bufs[kk % 2].data_ptr() + 4 * half * h, N, steps[kk].flags, st.cuda_stream, absmax_ptr=slot_of(kk))
                    if k == k0:
                        ev = torch.cuda.Event()
                        ev.record(side[0])
                        side[1].wait_event(ev)
                for st in side:
                    main.wait_stream(st)
            rows_out = steps[-1].rows
            out = bufs[(n - 1) % 2][:rows_out * N].view(rows_out, N).clone()      # the workspace is reused by the next call
            plan['done'] = torch.cuda.Event()
            plan['done'].record(main)
        return out.t()

    def exact_mode(self, flag):
        """Switch every keyed layer between the arithmetic contracts WITHOUT re-keying: True = the reference's accumulation
        order and mul-then-add rounding in every layer (bit-exact with scipy: order-preserving kernels, no MFMA); False =
        matrix cores wherever an operator has such a path (conv-taps, large dense operators), whatever the error; 'auto' = per layer,
        decided at the next forward so that the float-key tolerance 1e-5 holds against the reference's arithmetic (KeyedLayer._calibrate;
        see contract_report()); 'auto-bf16x3' = like 'auto', but a conv layer first tries the kernel that emulates f32 products on the bf16
        matrix pipe (three-way split, six of nine cross products: KN_FLAG_BF16X3) and keeps it when its result, measured against the
        order-preserving kernel on the calibration batch, has 4x headroom under the tolerance (EXPERIMENTAL, opt-in); 'bf16x3' forces that
        kernel wherever it applies; None = back to the per-layer setting the key-net was built with (tiled key-nets: 'auto').  Returns self."""
        for c in self._keyed():
            if not hasattr(c, '_exact_built'):
                c._exact_built = getattr(c, '_exact_decl', getattr(c, '_exact', True))
            if flag == 'auto-bf16x3':        # 'auto' with the bf16x3 kernel as the first candidate (opt-in: never chosen by default)
                (c._exact, c._allow_bf16x3) = ('auto', True)
            else:
                c._exact = c._exact_built if flag is None else klayer._contract(flag, True)
                c._allow_bf16x3 = False
            c.__dict__.pop('_contract_record', None)
        self._drop_plans()                  # the launch lists depend on the layers' contracts
        return self

    def contract_report(self):
        """Per keyed layer: the contract in force (True / False / 'auto' = not decided yet) and, for layers decided by calibration, the
        record of that decision (bound, measured difference, tolerance, max |x| it covers).  `switched` lists the layers calibration moved
        off the matrix cores; `rescreen` says whether every forward re-checks the decisions; `recalibrations` counts the layers a later,
        larger batch sent back to calibration.  `narrow` per layer: the record of its narrow='mfma' measurement (KeyedLayer.narrow_mode; also inside
        `calibration`), None for layers that have none.  `narrow_split`: the record of a layer's narrow_split measurement (KeyedLayer.narrow_split_mode; also inside `calibration`)
        -- present only on the layers that have one, so the rows of a key-net that never ran a narrow_split forward are what they were."""
        rows = [dict(name=n, exact=getattr(c, '_exact', True), declared=getattr(c, '_exact_decl', getattr(c, '_exact', True)),
                     calibration=getattr(c, '_contract_record', None), screened=c.screened(), narrow=c.narrow_record()) for (n, c) in self._keyed(named=True)]
        for (r, (_, c)) in zip(rows, self._keyed(named=True)):
            if c.narrow_split_record() is not None:
                r['narrow_split'] = c.narrow_split_record()
        return dict(layers=rows, switched=[r['name'] for r in rows if r['calibration'] is not None and r['calibration'].get('decided') == 'exact' and 'bound' in r['calibration']],
                    undecided=[r['name'] for r in rows if r['exact'] == 'auto'],
                    rescreen=bool(self.RESCREEN and any(r['screened'] for r in rows)),
                    recalibrations=int(self.__dict__.get('_recalibrations', 0)))

    _LEVEL = {'bf16x3': 0, 'split': 1, False: 2, True: 3}       # codes of a decided contract on the wire (sync_contract); only True (the reference's order) outranks the others

    def sync_contract(self, group=None):
        """COLLECTIVE (every rank of `group` must call it, the same number of times): make the calibration decisions of replicated key-nets
        agree.  Each rank decides a layer's contract on the batches IT sees, so one rank may keep a layer on the matrix cores that another
        rank's larger activations moved to the reference's order; replicas would then no longer be bit-identical.  One all-reduce(MAX) of two
        small integers per keyed layer (the largest and the smallest decided code).  Rule: a layer every deciding rank runs under the SAME
        contract keeps it; any disagreement ends in the reference's order on every rank -- an exact decision anywhere wins, and two different
        re-ordering contracts ('split' on one rank, the fused matrix-core kernel on another) are not ordered by conservativeness: a rank's
        calibration measured ITS kernel on ITS batch only, so neither record covers the other kernel (round-5 advisor finding; until then the
        ranks moved to the larger code and kept the old record).  Returns the names of the layers this rank changed (the caller recomputes its
        current batch when the list is not empty: keynet_amd.dist.sharded_forward does).  Layers still 'auto' (no forward yet) are left alone.
        A no-op without an initialised process group."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return []
        named = self._keyed(named=True)
        mine = [self._LEVEL.get(getattr(c, '_exact', True), -1) if getattr(c, '_exact', True) != 'auto' else -1 for (_, c) in named]
        dev = torch.device('cpu') if dist.get_backend(group) == 'gloo' else torch.device('cuda', torch.cuda.current_device())
        t = torch.tensor([mine, [(-m if m >= 0 else -99) for m in mine]], dtype=torch.int32, device=dev)     # row 1: MAX of the negated codes = the smallest decided code
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
        (hi, lo) = (t[0].tolist(), [-v for v in t[1].tolist()])
        changed = []
        for ((n, c), m, a, b) in zip(named, mine, hi, lo):
            if m < 0 or a == b or m == self._LEVEL[True]:
                continue                                # undecided here / every deciding rank agrees / already in the reference's order
            rec = dict(getattr(c, '_contract_record', None) or {})
            rec.update(decided='exact', reason=('another rank\'s batch needed the reference\'s order' if a == self._LEVEL[True] else
                                                'ranks calibrated onto different re-ordering kernels: no rank\'s record covers the other\'s') + ' (KeyedModel.sync_contract)')
            rec.pop('max_abs_x', None)                  # nothing left to screen: the reference's order holds for any input
            (c._exact, c._contract_record) = (True, rec)
            changed.append(n)
        if changed:
            self._drop_plans()
        return changed

    def capture(self, img_cipher, narrow=False, narrow_rows=False, narrow32=False, narrow64=False, narrow_linear=False, narrow_split=False, narrow_taps=False, narrow_fill=False):
        """Capture forward_linear for this input shape into a HIP graph (torch.cuda.CUDAGraph on ROCm) and return a callable
        `replay(x) -> [N, classes+1]`.  Small key-nets are launch-bound (LeNet at N=1024: 7 kernels in 0.25 ms); one graph
        launch replaces them.  The graph runs the passes of the eager forward on the block _prepare made; replay(x) copies x into its first N images.
        The operators must already be resident and every 'auto' layer decided (one eager forward is run first); the returned tensor is the first N
        rows of the graph's static output buffer (clone it to keep a result across replays).  A key-net with calibrated layers keeps its per-forward
        screen: the graph gathers max |x| per layer like the eager forward, replay() reads it back after the launch and, when a layer's input has
        outgrown its calibration, re-runs the batch eagerly (re-calibrating) and captures a new graph.
        `narrow`, `narrow_rows`, `narrow32`, `narrow64`, `narrow_linear` (narrow='mfma', narrow64='mfma' included): the graph of forward_linear under the same keywords, up to
        the same widths -- a straight line of launches on one stream, no parallel branches, decided by the eager forward first.  Where that forward screens layers
        (narrow='mfma': against their narrow records; the 64-column tile: against their wide records; narrow=True: none, replay() reads nothing back) the graph gathers
        their max |x|, replay() reads the slots after the launch and on a trip runs the batch eagerly (measuring or calibrating again) and captures a new graph.
        `narrow_split` (with narrow='mfma'): the graph of that forward -- the eager forward first measures the narrow split route where a calibrated layer has no record of it and
        allocates the route's workspaces, so the capture finds both; replay equals the eager forward bit for bit.  `narrow_taps`, `narrow_fill` (with `narrow`): the graph of that forward (the eager forward run first builds the record tables of narrow_fill, so the capture allocates nothing)."""
        assert img_cipher.is_cuda, 'capture() needs a device tensor'
        n = img_cipher.shape[0]
        (form, static_in, windows) = self._resolve(img_cipher, (narrow, narrow_rows, narrow32, narrow64, narrow_linear), own=True, narrow_split=narrow_split, narrow_taps=narrow_taps, narrow_fill=narrow_fill)
        keyed = self._keyed()
        state = {}

        def build():
            self._forward_passes(static_in, windows, False, form)       # uploads operators, sizes workspaces, calibrates (not capturable)
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self._forward_passes(static_in, windows, False, form)   # warm-up on the capture stream
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            # capture ON THE WARMED STREAM: per-stream state of the operators (the split-K workspace of a dense layer, kn_api.hip) was sized
            # by the warm-up forward above; torch's default capture stream would be a fresh one, and a hipMalloc inside a capture is refused
            with torch.cuda.graph(graph, stream=side):
                (out, screens) = self._forward_passes(static_in, windows, False, form)
            state.update(graph=graph, out=out[:n], screens=screens)

        build()

        def replay(x):
            static_in[:n].copy_(x)
            state['graph'].replay()
            if any(self._rescreen(slots.tolist(), keyed, screened, narrow) for (slots, screened, narrow) in state['screens']):
                build()                                          # eager forward on this batch re-calibrates (narrow: measures again); then a fresh graph
                state['graph'].replay()
            replay.graph = state['graph']
            return state['out']
        replay.graph = state['graph']
        return replay

    def forward(self, img_cipher, outkey=None, narrow=False, narrow_rows=False, narrow32=False, narrow64=False, narrow_linear=False, narrow_split=False, narrow_taps=False, narrow_fill=False):
        """Encrypted image(s) [N, D0+1] -> logits.  N == 1 returns the reference's shape `outshape` = (C,1,1)
        (keynet/system.py:130-133); N > 1 (an extension: the reference cannot) returns (N, C, 1, 1).  `narrow`, `narrow_rows`, `narrow32`, `narrow64`,
        `narrow_linear`, `narrow_split`, `narrow_taps`, `narrow_fill` (narrow='mfma', narrow64='mfma' included): the low-latency forms of this very call, handed to forward_linear, which says what each selects."""
        outkey = outkey if outkey is not None else self.embeddingkey()
        y = self.forward_linear(img_cipher, narrow=narrow, narrow_rows=narrow_rows, narrow32=narrow32, narrow64=narrow64, narrow_linear=narrow_linear, narrow_split=narrow_split, narrow_taps=narrow_taps, narrow_fill=narrow_fill)
        if outkey is not None:
            y = self.decrypt(y, outkey)
        n = y.shape[0]
        return ktorch.linear_to_affine(y, self._outshape if n == 1 else (n,) + tuple(self._outshape))

    def decrypt(self, y_cipher, outkey=None):
        """Apply the embedding key (the reference's version constructs KeyedLayer(W=outkey), an invalid call:
        keynet/system.py:137; the intent -- one more torchdot with the key -- is what is implemented)."""
        outkey = outkey if outkey is not None else self.embeddingkey()
        if outkey is None:
            return y_cipher
        W = outkey if isinstance(outkey, ksp.SparseMatrix) else ksp.SparseMatrix(outkey)
        return W.torchdot(y_cipher.t()).t()

    def imagekey(self):
        return self._imagekey

    def embeddingkey(self):
        return self._embeddingkey

    def public(self):
        """Strip the private keys before releasing the key-net (keynet/system.py:147-151)."""
        (self._imagekey, self._embeddingkey) = (None, None)
        return self

    def num_parameters(self):
        return sum([c.nnz() for (k, c) in self._keynet.named_children() if isinstance(c, klayer.KeyedLayer)])

    def layers(self):
        return self._layernames


def _relu_block(y):
    """Stand-alone nn.ReLU on an [N, D+1] activation (only when it could not be fused into a producer)."""
    src = y.device
    yt = ksp._device_block(y.t()).clone()
    _capi.relu(yt.data_ptr(), yt.shape[0], yt.shape[1], yt.shape[1], torch.cuda.current_stream().cuda_stream)
    out = yt.t()
    return out if src.type == 'cuda' else out.to(src)


class KeyedSensor(klayer.KeyedLayer):
    """The paired sensor: applies the image key A_0 to the homogeneous image (keynet/system.py:160-263)."""

    def __init__(self, inshape, keypair):
        assert isinstance(inshape, tuple) and len(inshape) == 3
        nn.Module.__init__(self)
        (self._encryptkey, self._decryptkey) = keypair
        self._inshape = (1, *inshape)
        self._tensor = None
        self._im = None
        self.W = ksp.SparseMatrix(self._encryptkey)
        self._layertype = 'input'
        self._repr = 'KeyedSensor'
        self._tileshape = None
        self._outshape = None

    def __repr__(self):
        return str('<KeyedSensor: height=%d, width=%d, channels=%d>' % (self._inshape[2], self._inshape[3], self._inshape[1]))

    def load(self, imgfile, imagekey=None):
        """Read + resize an image file to the sensor shape as a float tensor in [0,255] (keynet/system.py:183-201 via
        vipy; here PIL bilinear -- the resize interpolation is parity-unpinned).
        With `imagekey` (what save() returned next to the file; keynet/system.py:185-194): the file is an encrypted 8-bit image, read as stored -- no resize, its shape
        asserted -- scaled by 1/255, homogenised and multiplied by the key (a SparseMatrix.torchdot on the device); the tensor becomes the decrypted [1, C, H, W] image."""
        from PIL import Image
        (C, H, W) = self._inshape[1:]
        if imagekey is not None:
            im = Image.open(imgfile)
            if im.mode != ('L' if C == 1 else 'RGB'):
                im = im.getchannel(0) if C == 1 else im.convert('RGB')          # one channel only, no scaling (keynet/system.py:186-187)
            a = np.asarray(im, dtype=np.float32)
            a = a.reshape(a.shape[0], a.shape[1], 1) if a.ndim == 2 else a
            assert (a.shape[2], a.shape[0], a.shape[1]) == (C, H, W), 'the stored image %s is not the sensor shape %s' % (str(a.shape), str((C, H, W)))
            x = torch.as_tensor(np.ascontiguousarray(a.transpose(2, 0, 1))).unsqueeze(0)
            x_linear = ktorch.affine_to_linear((1.0 / 255.0) * x)               # [0, 255] -> [0, 1], one f32 multiply as the reference's
            key = ksp.SparseMatrix(imagekey) if scipy.sparse.issparse(imagekey) else imagekey
            self._tensor = ktorch.linear_to_affine(key.torchdot(x_linear.t()).t().float(), (1, C, H, W))
            return self
        im = Image.open(imgfile).convert('L' if C == 1 else 'RGB').resize((W, H), Image.BILINEAR)
        a = np.asarray(im, dtype=np.float32)
        a = a.reshape(H, W, 1) if a.ndim == 2 else a
        self._tensor = torch.as_tensor(np.ascontiguousarray(a.transpose(2, 0, 1))).unsqueeze(0)
        return self

    def fromtensor(self, x):
        if x is not None:
            self._tensor = x.clone().float()
        return self

    def tensor(self):
        return self._tensor.unsqueeze(0) if self._tensor.ndim == 3 else self._tensor

    def astensor(self):
        return self.tensor()

    def totensor(self):
        return self.tensor()

    def keypair(self):
        return (self._encryptkey, self._decryptkey)

    def key(self):
        return self._decryptkey

    def isloaded(self):
        return self._tensor is not None

    def isencrypted(self):
        """Encrypted = homogenised [N, C*H*W+1] (the reference only recognises N == 1; batches are an extension)."""
        return self.isloaded() and self._tensor.ndim == 2 and self._tensor.shape[1] == int(np.prod(self._inshape)) + 1

    def encrypt(self):
        """NxCxHxW -> Nx(C*H*W+1) homogenised and keyed (keynet/system.py:250-255)."""
        assert self.isloaded(), 'Load image first'
        if not self.isencrypted():
            self._tensor = self.forward(ktorch.affine_to_linear(self._tensor))
        return self

    def check_frames(self, frames, layout='NHWC', dtype=torch.uint8):
        """n of a batch of frames that has this sensor's shape ([n, H, W, C] under 'NHWC', [n, C, H, W] under 'NCHW'); ValueError otherwise.  No GPU call."""
        (n, chw) = ktorch.frame_shape(frames, layout, dtype)
        if chw != tuple(self._inshape[1:]):
            raise ValueError('frames of shape (C, H, W) = %s do not fit the sensor %s' % (str(chw), str(tuple(self._inshape[1:]))))
        return n

    def encrypt_frames(self, frames, layout='NHWC', pad_to=1):
        """uint8 frames on the device ([n, H, W, C], or [n, C, H, W] with layout='NCHW') -> the encrypted block [n_cols, C*H*W+1] on the device: the load, homogenise,
        encrypt of keynet/system.py:183-201, 250-255 for a batch of raw camera frames, as kn_u8_to_linear (ktorch.frames_to_linear) and this sensor's own keyed product.
        Its first n rows equal fromtensor(frames as float NCHW).encrypt().astensor() bit for bit; rows n .. n_cols - 1 (n_cols = n rounded up to `pad_to`) stay zero
        images.  Stateless: the loaded tensor of this sensor is neither read nor changed.  ValueError for frames that are not the sensor's shape, before any GPU call."""
        self.check_frames(frames, layout)
        return self.forward(ktorch.frames_to_linear(frames, layout=layout, pad_to=pad_to))

    def encrypt_to_frames(self, frames, layout='NHWC', depth=8, range=None):
        """Plaintext uint8 frames on the device -> (cipher_frames, lo, hi), all on the device: the ENCRYPTED images as quantised frames of `depth` = 8 | 16 bits
        (torch.uint8 | torch.uint16, the layout of `frames`) and the float32 [n] ranges they were quantised over -- the wire format between this sensor and a server that
        holds only the keyed model (KeyedModel.forward_frames, StreamedForward(frames='cipher8' | 'cipher16')); the batch form of save()'s picture
        (keynet/system.py:173-181) without a private image key.  encrypt_frames, then the range: range=None takes every encrypted image's own minimum and maximum
        (kn_column_range); range=(lo, hi) is ONE fixed range for every image -- a real converter has one, and it leaks nothing per image; values outside it saturate.
        Then ktorch.gray_affine(levels = 2^depth - 1) and ktorch.linear_to_frames(depth).  Under a permutation image key range=(0, 255) stores the encrypted block's own
        bytes.  Stateless, like encrypt_frames.  ValueError for frames that are not the sensor's shape, another depth or a range that is not two finite numbers lo < hi,
        before any GPU call."""
        n = self.check_frames(frames, layout)
        if depth not in ktorch.GRAY_LEVELS:
            raise ValueError('invalid depth %s: 8 or 16 bits' % str(depth))
        if range is not None:
            try:
                (rlo, rhi) = (float(range[0]), float(range[1]))
                fixed = len(range) == 2 and np.isfinite(rlo) and np.isfinite(rhi) and rlo < rhi
            except (TypeError, ValueError, IndexError):
                fixed = False
            if not fixed:
                raise ValueError('range must be None or two finite numbers (lo, hi) with lo < hi, not %s' % str(range))
        x = self.encrypt_frames(frames, layout=layout)
        if range is None:
            (lo, hi) = ktorch.column_range(x)
        else:
            (lo, hi) = (torch.full((n,), rlo, dtype=torch.float32, device=x.device), torch.full((n,), rhi, dtype=torch.float32, device=x.device))
        (gain, bias) = ktorch.gray_affine(lo, hi, ktorch.GRAY_LEVELS[depth])
        return (ktorch.linear_to_frames(x, tuple(self._inshape[1:]), layout=layout, gain=gain, bias=bias, depth=depth), lo, hi)

    def decrypt_from_frames(self, cipher_frames, lo, hi, layout='NHWC'):
        """What encrypt_to_frames returns -> plaintext uint8 frames on the device: the dequantising ingest (ktorch.gray_inverse, ktorch.frames_to_linear; the depth is
        the frames' dtype), then decrypt_frames.  Under a permutation image key and range=(0, 255) the round trip is exact; otherwise to within the quantisation of the
        encrypted range, seen through the decrypt key.  ValueError for frames that are not the sensor's shape or ranges that are not float32 [n] on the frames' device,
        before any GPU call."""
        n = self.check_frames(cipher_frames, layout, ktorch.FRAME_DTYPES)
        (scale, offset) = ktorch.cipher_range(cipher_frames, lo, hi, n)
        return self.decrypt_frames(ktorch.frames_to_linear(cipher_frames, layout=layout, scale=scale, offset=offset), layout=layout)

    def decrypt(self):
        assert self.isloaded(), 'Load image first'
        if self.isencrypted():
            x_raw = super(KeyedSensor, self).decrypt(self._decryptkey, self._tensor)
            n = x_raw.shape[0]
            self._tensor = ktorch.linear_to_affine(x_raw, (n,) + tuple(self._inshape[1:]))
        return self

    def _check_cipher(self, x_cipher, layout):
        """n of an encrypted block [n, C*H*W+1] (float32, on the device) that has this sensor's shape; ValueError otherwise, also for a wrong layout string.  No GPU call."""
        if layout not in ktorch.LAYOUTS:
            raise ValueError('invalid layout "%s": one of %s' % (str(layout), ', '.join(ktorch.LAYOUTS)))
        return ktorch._check_linear(x_cipher, 'decrypt_frames', int(np.prod(self._inshape)))[0]

    def decrypt_frames(self, x_cipher, layout='NHWC'):
        """The encrypted block [n, C*H*W+1] on the device (what encrypt_frames returns, its zero images included) -> uint8 frames on the device, [n, H, W, C] or
        [n, C, H, W] with layout='NCHW': the decrypt of keynet/system.py:257-263 for a batch, as this sensor's own decrypt product and kn_linear_to_u8
        (ktorch.linear_to_frames with unit gain: round to nearest, saturate).  Under a permutation image key the decrypted block is exact, so
        decrypt_frames(encrypt_frames(f)) == f byte for byte; under a float key as long as the decrypt error stays below one half.  Stateless: the loaded tensor of this
        sensor is neither read nor changed.  The homogeneous column is not checked (decrypt() does: a zero image has none).  ValueError for a block that is not the sensor's
        shape, before any GPU call."""
        self._check_cipher(x_cipher, layout)
        x_raw = super(KeyedSensor, self).decrypt(self._decryptkey, x_cipher)
        return ktorch.linear_to_frames(x_raw.float(), tuple(self._inshape[1:]), layout=layout)

    def asframes(self, layout='NHWC'):
        """The loaded tensor, encrypted or not, one image or a batch, as gray-scaled uint8 frames on the device: (frames, gain, bias), frames [N, H, W, C] (or
        [N, C, H, W]), gain and bias device float32 [N] -- every image mapped by its own range onto [0, 255] (the mat2gray of keynet/system.py:223-228, per image):
        kn_column_range, ktorch.gray_affine, kn_linear_to_u8, nothing read back to the host.  An un-encrypted tensor is homogenised first (affine_to_linear).  A constant
        image is black (gray_affine).  ValueError for a wrong layout string, before any GPU call."""
        if layout not in ktorch.LAYOUTS:
            raise ValueError('invalid layout "%s": one of %s' % (str(layout), ', '.join(ktorch.LAYOUTS)))
        assert self.isloaded(), 'Load image first'
        x = ksp._device_block(self._tensor) if not self._tensor.is_cuda else self._tensor.detach().float()
        if not self.isencrypted():
            x = ktorch.affine_to_linear(x)
        (lo, hi) = ktorch.column_range(x)
        (gain, bias) = ktorch.gray_affine(lo, hi)
        return (ktorch.linear_to_frames(x, tuple(self._inshape[1:]), layout=layout, gain=gain, bias=bias), gain, bias)

    def _image_mode(self):
        C = self._inshape[1]
        if C not in (1, 3):
            raise ValueError('an image has 1 or 3 channels, this sensor has %d (asframes gives the bytes)' % C)
        return 'L' if C == 1 else 'RGB'

    def _asimage(self):
        """(PIL image, gain, bias) of the one loaded image."""
        from PIL import Image
        mode = self._image_mode()
        assert self.isloaded(), 'Load image first'
        assert self._tensor.ndim == 3 or self._tensor.shape[0] == 1, 'asimage is for one image (asframes takes a batch)'
        (frames, gain, bias) = self.asframes('NHWC')
        a = frames[0].cpu().numpy()
        return (Image.fromarray(a[:, :, 0] if mode == 'L' else a, mode), gain, bias)

    def asimage(self):
        """The loaded image (N == 1), encrypted or not, gray-scaled to 8 bits as a PIL.Image, 'RGB' for three channels and 'L' for one (keynet/system.py:223-228, PIL
        in place of vipy); ValueError for another channel count."""
        return self._asimage()[0]

    def toimage(self):
        return self.asimage()

    def gray_imagekey(self, gain, bias):
        """decryptkey . G^-1 for the gray mapping G: y = (gain / 255) x + bias / 255 of one encrypted image onto [0, 1] -- the key that takes the stored 8-bit image,
        scaled by 1/255 and homogenised, back to the decrypted image (keynet/system.py:181).  G^-1 = [[(255 / gain) I, -bias / gain], [0, 1]] in closed form in float64,
        cast at the end (keys.diagonal_affine_to_linear).  Host algebra (scipy); ValueError for gain == 0: a constant image was stored as black and has no inverse."""
        (g, b) = (float(gain) / 255.0, float(bias) / 255.0)
        if not (np.isfinite(g) and np.isfinite(b)) or g == 0.0:
            raise ValueError('the gray mapping of a constant or non-finite image has no inverse (gain %g, bias %g)' % (float(gain), float(bias)))
        D = int(np.prod(self._inshape))
        (_, Ginv) = diagonal_affine_to_linear(scipy.sparse.eye(D, dtype=np.float64).tocsr() * g, np.full((D, 1), b, dtype=np.float64), withinverse=True)
        return scipy.sparse.csr_matrix(self._decryptkey).dot(Ginv.tocsr())

    def save(self, outfile='/tmp/out.png'):
        """Write the encrypted image (N == 1) as an 8-bit PNG and return (outfile, imagekey): load(outfile, imagekey) reads it back and decrypts it, to within half a
        gray step of the encrypted image's range (keynet/system.py:173-181)."""
        assert self.isencrypted(), 'save() stores the encrypted image: encrypt() first'
        (im, gain, bias) = self._asimage()
        im.save(outfile, format='PNG')
        return (outfile, self.gray_imagekey(gain.cpu()[0], bias.cpu()[0]))


class PublicKeyedSensor(KeyedSensor):
    """Sensor with the identity key: only homogenises (keynet/system.py:266-284)."""

    def __init__(self, inshape):
        n = int(np.prod(inshape)) + 1
        super(PublicKeyedSensor, self).__init__(inshape, (sparse_identity_matrix(n), sparse_identity_matrix(n)))

    def __repr__(self):
        return str('<PublicKeyedSensor: height=%d, width=%d, channels=%d>' % (self._inshape[2], self._inshape[3], self._inshape[1]))

    def encrypt(self):
        raise ValueError('PublicKeyedSensor has no encryption keys')

    def decrypt(self):
        raise ValueError('PublicKeyedSensor has no decryption keys')

    def tensor(self):
        assert self.isloaded(), 'Load image first'
        if not self.isencrypted():
            self._tensor = self.forward(ktorch.affine_to_linear(self._tensor))
        return self._tensor


# ------------------------------------------------------------------------------------------------------------------
BACKENDS = ('hip',)


def layergen(module, inshape, outshape, A, Ainv, tileshape=None, backend='hip', direct=None, exact=None):
    """The plug-in seam of the reference (keynet/system.py:303-314): snaps the requested tile to divisors of the
    layer's spatial sizes, then dispatches on `backend`.  The reference accepts only 'scipy'; this build registers
    'hip'.  Anything else raises ValueError('invalid backend ...') exactly like the reference."""
    # exact=None: untiled key-nets bit-exact; tiled key-nets 'auto' (matrix cores wherever the 1e-5 float-key contract holds, decided per
    # layer at the first forward: KeyedLayer._calibrate)
    if tileshape is not None:
        tileshape = (find_closest_positive_divisor(outshape[1], tileshape[0]), find_closest_positive_divisor(inshape[1], tileshape[1]))
    if backend == 'hip':
        return klayer.KeyedLayer(module, inshape, outshape, A, Ainv, tileshape=tileshape, direct=direct, exact=exact)
    raise ValueError('invalid backend "%s"' % backend)


def Keynet(inshape, net=None, backend='hip', global_photometric='identity', local_photometric='identity', global_geometric='identity',
           local_geometric='identity', memoryorder='channel', do_output_encryption=False, alpha=None, beta=None, gamma=None,
           hierarchical_blockshape=None, hierarchical_permute_at_level=None, blocksize=None, tileshape=None, direct=None, exact=None):
    """(sensor, model) for `net` under the chosen key family (keynet/system.py:472-486).  ReLU outputs only admit keys
    that commute with ReLU: a 'relu*' layer keeps identity where identity was asked and otherwise falls back to the
    positive-gain / permutation members of the family (keynet/system.py:476-480)."""
    def f_layergen(module, inshape_, outshape_, A, Ainv):
        return layergen(module, inshape_, outshape_, A, Ainv, tileshape=tileshape, backend=backend, direct=direct, exact=exact)

    def f_keypair(layername, shape):
        isrelu = 'relu' in layername
        return keygen(shape,
                      global_photometric=global_photometric if (not isrelu or global_photometric == 'identity') else 'identity',
                      local_photometric=local_photometric if (not isrelu or local_photometric == 'identity') else 'uniform_random_gain',
                      global_geometric=global_geometric if (not isrelu or global_geometric == 'identity') else 'identity',
                      local_geometric=local_geometric if (not isrelu or local_geometric == 'identity') else 'permutation',
                      memoryorder=memoryorder, blocksize=blocksize, tileshape=tileshape, alpha=alpha, beta=beta, gamma=gamma,
                      hierarchical_blockshape=hierarchical_blockshape, hierarchical_permute_at_level=hierarchical_permute_at_level)

    if backend not in BACKENDS:
        raise ValueError('invalid backend "%s"' % backend)
    sensor = KeyedSensor(inshape, f_keypair('input', inshape))
    model = KeyedModel(net, inshape, sensor.key(), f_keypair, f_layergen, do_output_encryption=do_output_encryption) if net is not None else None
    return (sensor, model)


def IdentityKeynet(inshape, net, backend='hip'):
    return Keynet(inshape, net, backend=backend)


def PermutationKeynet(inshape, net, do_output_encryption=False):
    return Keynet(inshape, net, global_geometric='permutation', do_output_encryption=do_output_encryption)


def TiledOrthogonalKeynet(inshape, net, tilesize, hierarchical_permute_at_level=(0, 1), direct=None, exact=None):
    """Hierarchical block permutation + block-local Givens rotations + block-local affine photometric key, block memory
    order (keynet/system.py:504-510): the float-key family (1e-5 contract)."""
    return Keynet(inshape, net, tileshape=(tilesize, tilesize), global_geometric='hierarchical_permutation', hierarchical_blockshape=(2, 2),
                  hierarchical_permute_at_level=hierarchical_permute_at_level, global_photometric='identity', local_geometric='givens_orthogonal',
                  alpha=tilesize, blocksize=tilesize, local_photometric='uniform_random_affine', beta=0.1, gamma=100.0, memoryorder='block',
                  direct=direct, exact=exact)


def TiledIdentityKeynet(inshape, net, tilesize, direct=None, exact=None):
    return Keynet(inshape, net, tileshape=(tilesize, tilesize), direct=direct, exact=exact)


def TiledPermutationKeynet(inshape, net, tilesize, direct=None, exact=None):
    return Keynet(inshape, net, local_geometric='permutation', tileshape=(tilesize, tilesize), blocksize=tilesize, direct=direct, exact=exact)
