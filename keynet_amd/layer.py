"""KeyedLayer: one keyed linear layer  W_hat = A . W . A_prev^-1  of a key-net (mirror of keynet/layer.py:15-106).

Construction (host, offline) restates the reference's keying; `forward` -- the drop-in boundary -- hands the activation
block to the HIP operator stored in `self.W` (its torchdot), optionally fusing the ReLU that follows.
"""
import collections
import logging
import numpy as np
import scipy.sparse
import torch
from torch import nn
import torch.nn.functional as F

from .globals import verbose
from . import sparse as ksp
from . import direct as kdirect
from .sparse import SparseMatrix, sparse_toeplitz_conv2d, sparse_toeplitz_avgpool2d
from . import _capi
from .torch import affine_to_linear_matrix


def _square(v, what):
    """kernel_size / stride given as int or (a, a) -> a."""
    if isinstance(v, int):
        return v
    assert len(v) in (1, 2) and v[0] == v[-1], '%s must be square / isotropic, got %s' % (what, str(v))
    return v[0]


def _sandwich(A, W, Ainv):
    """A . W . Ainv with the reference's association ((A.W).Ainv, keynet/layer.py:35): scipy's SpGEMM leaves each row in
    an order that depends on it, and that stored order is part of the bit-exact contract.  A is None for the last
    layer of a key-net without output encryption."""
    return W.dot(Ainv) if A is None else A.dot(W).dot(Ainv)


def _conv_operator(m, inshape, outshape, A, Ainv, tileshape, direct):
    k = _square(m.kernel_size, 'kernel')
    stride = _square(m.stride, 'stride')
    assert len(inshape) == 3, 'inshape is the (C,H,W) of the tensor entering this layer'
    assert m.padding[0] == k // 2 and m.padding[-1] == k // 2, "only 'same' padding ((k-1)/2) is keyable"
    (w, b) = (m.weight.detach().numpy(), m.bias.detach().numpy())
    if direct is None:
        direct = tileshape is not None and kdirect.toeplitz_entries('conv', inshape, outshape, k) > KeyedLayer.DIRECT_THRESHOLD
    if direct:
        return ksp.Conv2dTiledMatrix.fromtaps(tileshape=tileshape, **kdirect.keyed_conv_taps(w, b, inshape, outshape, stride, A, Ainv))
    W = _sandwich(A, sparse_toeplitz_conv2d(inshape, w, bias=b, stride=stride), Ainv)
    if tileshape is None:
        # An untiled keyed conv whose stored CSR is, provably, the ascending-column expansion of its factored form (identity / channel-replicated
        # permutation keys on both sides: every conv layer of PermutationKeynet AllConvNet but the first) is handed to the device in factored form:
        # same bits (the proof is entry for entry, order included), 0.3 MB of taps instead of the CSR's hundreds of MB.  See FactoredSparseMatrix.
        if W.nnz >= KeyedLayer.FACTOR_UNTILED_MIN_NNZ:
            try:
                F = ksp.Conv2dTiledMatrix.fromtaps(tileshape=None, **kdirect.keyed_conv_taps(w, b, inshape, outshape, stride, A, Ainv))
                if ksp.FactoredSparseMatrix.proven(W.tocsr() if W.format != 'csr' else W, F):
                    return ksp.FactoredSparseMatrix(W, F)
            except (ValueError, AssertionError):
                pass                                    # keys that are not channel-replicated (a global permutation): the CSR it is
        return W
    return ksp.Conv2dTiledMatrix(W, inshape, outshape, tileshape, bias=True, sanitycheck=False)


def _pool_operator(m, inshape, outshape, A, Ainv, tileshape, direct):
    k = _square(m.kernel_size, 'kernel')
    stride = _square(m.stride, 'stride')
    assert len(inshape) == 3, 'inshape is the (C,H,W) of the tensor entering this layer'
    C = inshape[0]
    if direct is None:
        direct = tileshape is not None and kdirect.toeplitz_entries('pool', inshape, (C,) + tuple(outshape[1:]), k) > KeyedLayer.DIRECT_THRESHOLD
    if direct:
        W = kdirect.keyed_avgpool_csr(C, (inshape[1], inshape[2]), k, stride, A, Ainv)
    else:
        W = _sandwich(A, sparse_toeplitz_avgpool2d(inshape, (C, C, k, k), stride), Ainv)
    return W if tileshape is None else ksp.TiledMatrix(W, tileshape)


def _linear_operator(m, A, Ainv):
    dense = affine_to_linear_matrix(m.weight, m.bias).detach().numpy()      # (in+1, out+1), left-multiplying
    return _sandwich(A, scipy.sparse.coo_matrix(dense).transpose(), Ainv)


def _contract(exact, bit_exact_default):
    """Arithmetic contract of a layer: True (the reference's order and rounding), False (matrix cores, float-key tolerance) or 'auto'
    (decided at the first forward and re-screened on every later one, KeyedLayer._calibrate / rescreen).  None = the default: True for
    untiled layers and for layers keyed by permutations only (north_star: "bit-exact for the permutation-only key"), 'auto' for tiled
    layers whose keys carry float coefficients ("within 1e-5 for float keyed layers").  Strings 'exact' / 'mfma' name True / False."""
    if exact is None:
        return True if bit_exact_default else 'auto'
    if isinstance(exact, str):
        assert exact in CONTRACTS, "exact must be True, False, None or one of %s" % str(CONTRACTS)
        return {'exact': True, 'mfma': False}.get(exact, exact)
    return bool(exact)


CONTRACTS = ('exact', 'mfma', 'auto', 'bf16x3', 'split')


def contract_name(c):
    """True / False / 'auto' / 'bf16x3' / 'split' -> 'exact' / 'mfma' / 'auto' / 'bf16x3' / 'split' (the on-disk and reporting vocabulary)."""
    return c if isinstance(c, str) else ('exact' if c else 'mfma')


def _is_permutation_key(M):
    """Is this key (scipy sparse, or None = no key on that side) a permutation matrix: one entry per row and column, every value
    exactly 1?  Such keys only move entries around: the keyed operator holds the source weights themselves, nothing is scaled or mixed."""
    if M is None:
        return True
    if not scipy.sparse.issparse(M) or M.shape[0] != M.shape[1] or M.nnz != M.shape[0]:
        return False
    C = M.tocoo()
    n = M.shape[0]
    return bool(np.all(C.data == 1) and len(np.unique(C.row)) == n and len(np.unique(C.col)) == n)


FLOAT_KEY_TOL = 1e-5          # BASELINE north_star: "within 1e-5 for float keyed layers"
# ... in the form the reference's own tests assert it (test/test_keynet.py:33,196,218: np.allclose(a, b, atol=1e-5), rtol at numpy's default):
# ELEMENT-WISE |a - b| <= atol + rtol |b|.  A small element next to large ones gets no slack from them.
FLOAT_KEY_ATOL = 1e-5
FLOAT_KEY_RTOL = 1e-5
EPS32 = float(np.finfo(np.float32).eps)


def gate(y, ref):
    """The float-key criterion as a number: max over elements of |y - ref| / (atol + rtol |ref|); <= 1 is np.allclose(y, ref, atol=1e-5)
    (numpy's default rtol).  Returns (ratio, |y - ref| at the worst element, its tolerance, max |y - ref|); NaN when a difference is not
    finite.  Device tensors; one host read."""
    d = (y - ref).abs()
    t = FLOAT_KEY_ATOL + FLOAT_KEY_RTOL * ref.abs()
    r = d / t
    r = torch.where(torch.isnan(r), torch.full_like(r, float('inf')), r)        # NaN (Inf - Inf, NaN on one side): never inside any tolerance
    k = torch.argmax(r)
    (rk, dk, tk, dmax) = torch.stack((r.flatten()[k], d.flatten()[k], t.flatten()[k], d.max())).tolist()      # the four scalars in ONE device-to-host read
    return (rk if np.isfinite(rk) else float('nan'), dk, tk, dmax)


_log = logging.getLogger('keynet_amd')

# One kn_spmm launch of a keyed layer (KeyedLayer.launch): operator handle and flags, and what the planners of a key-net ask about it --
# `exact`: the layer is under the bit-exact contract (_exact is True); `is_conv`: a Conv2dTiledMatrix operator; `is_linear`: keyed from an nn.Linear.
Launch = collections.namedtuple('Launch', 'op flags rows cols is_conv is_linear exact')


def _absmax_into(yt, slot):
    """Raise the one-element device tensor `slot` to max |yt| (kn_absmax: one pass over a feature-major block)."""
    yt = yt if yt.is_contiguous() else yt.contiguous()
    with torch.cuda.device(yt.device):
        _capi.absmax(yt.data_ptr(), yt.shape[0], yt.shape[1], yt.shape[1], slot.data_ptr(), torch.cuda.current_stream().cuda_stream)


class KeyedLayer(nn.Module):
    """One keyed layer of a key-net: holds W_hat = A . W . A_prev^-1 as an HBM-resident operator and applies it."""

    DIRECT_THRESHOLD = 20000000   # Toeplitz entries above which tiled conv/pool layers are keyed in factored form
    FACTOR_UNTILED_MIN_NNZ = 1000000     # untiled conv layers at least this large are checked for a factored device form (FactoredSparseMatrix)

    def __init__(self, module, inshape, outshape, A, Ainv, tileshape=None, direct=None, exact=None):
        """module: the source nn.Conv2d / nn.AvgPool2d / nn.Linear / nn.ReLU; A: this layer's output key (None = leave the
        output unkeyed); Ainv: inverse of the key on its input; tileshape: store conv/pool operators tiled.
        `direct`: None = automatic (factored, Toeplitz-free keying for tiled conv/avgpool layers whose Toeplitz matrix
        would exceed DIRECT_THRESHOLD entries -- the reference route cannot build those at all); True / False force it.
        `exact`: True = every product in the reference's accumulation order and rounding (bit-exact with scipy);
        False = conv-taps and large dense operators run on the matrix cores, whatever the error; 'auto' = the matrix cores where a
        calibration on the first batch shows the result inside the float-key tolerance (element-wise 1e-5 + 1e-5 |ref|), else exact.
        None (default) = exact for untiled layers AND for tiled layers keyed by permutations only (north_star: "bit-exact for the
        permutation-only key"), 'auto' for tiled layers whose keys carry float coefficients.
        Raises ValueError for layer types that cannot be keyed (the reference's behaviour, keynet/layer.py:72-79)."""
        super(KeyedLayer, self).__init__()
        self._layertype = str(type(module))
        (self._inshape, self._outshape, self._tileshape) = (inshape, outshape, tileshape)
        # default contract: bit-exact unless the layer is tiled AND one of its keys carries float coefficients
        self._exact = self._exact_decl = _contract(exact, tileshape is None or exact is not None or (_is_permutation_key(A) and _is_permutation_key(Ainv)))
        if isinstance(module, nn.Conv2d):
            self._repr = 'Conv2d %d->%d, k=%s, s=%s' % (module.in_channels, module.out_channels, str(module.kernel_size), str(module.stride))
            W = _conv_operator(module, inshape, outshape, A, Ainv, tileshape, direct)
        elif isinstance(module, nn.AvgPool2d):
            self._repr = 'AvgPool2d k=%s, s=%s' % (str(module.kernel_size), str(module.stride))
            W = _pool_operator(module, inshape, outshape, A, Ainv, tileshape, direct)
        elif isinstance(module, nn.Linear):
            self._repr = 'Linear %d->%d' % (module.in_features, module.out_features)
            W = _linear_operator(module, A, Ainv)
        elif isinstance(module, nn.ReLU):
            self._repr = 'ReLU'                       # a keyed ReLU: the key change alone, ReLU applied in forward
            W = A.dot(Ainv)
        elif isinstance(module, nn.BatchNorm2d):
            raise ValueError('a BatchNorm2d is folded into the layer before it: name it "<layer>_bn" and place it right after "<layer>"')
        elif isinstance(module, nn.Dropout):
            raise ValueError('Dropout is the identity at inference: it is skipped during keying, never keyed')
        else:
            raise ValueError('unsupported layer type "%s"' % str(type(module)))
        self.W = W if isinstance(W, SparseMatrix) else SparseMatrix(W)

    @classmethod
    def fromoperator(cls, W, layertype, inshape=None, outshape=None, repr_=None, exact=None):
        """Wrap an already keyed operator (a public key-net loaded from a neutral file, a fixture, a direct build)."""
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        # default contract of a loaded operator: bit-exact unless it is a conv operator with float coefficients (a factored operator without
        # coefficient entries was keyed by permutations; a block/tile description does not say, so it gets the float-key contract)
        coef_free = isinstance(W, ksp.Conv2dTiledMatrix) and W._taps is not None and W._taps['ent_coef'] is None
        self._exact = self._exact_decl = _contract(exact, coef_free or not isinstance(W, ksp.Conv2dTiledMatrix))
        (self._layertype, self._tileshape, self._inshape, self._outshape) = (layertype, None, inshape, outshape)
        self._repr = repr_ if repr_ is not None else layertype
        self.W = W if isinstance(W, SparseMatrix) else SparseMatrix(W)
        return self

    def extra_repr(self):
        return str('<%s, backend=hip, shape=%s, nnz=%d>' % (self._repr, str(self.W.shape), self.nnz()))

    def iskeyedrelu(self):
        return 'ReLU' in self._layertype

    def forward(self, x_affine, fuse_relu=False, absmax=None, narrow=False, narrow_rows=False, narrow32=False, narrow64=False, narrow_linear=False, narrow_split=False, narrow_taps=False, narrow_fill=False):
        """[N, Din+1] -> [N, Dout+1] (keynet/layer.py:88-93).  The result is a transposed view of the feature-major
        [Dout+1, N] block the kernel wrote, so the next layer's x.t() is free.  `fuse_relu` folds the unkeyed nn.ReLU
        that follows this layer in the key-net (keynet/system.py:92) into the kernel epilogue.  `absmax`: a one-element device
        f32 tensor raised to max |y| of this call (kn_spmm_screen; KeyedModel.forward_linear re-screens the next layer's contract with it).
        A layer whose contract is still 'auto' decides it here, on this batch (blocking host reads, an extra order-preserving launch:
        not capturable into a HIP graph -- KeyedModel.capture runs an eager forward first).
        `narrow`, `narrow_rows`, `narrow32`, `narrow64`, `narrow_linear` (narrow='mfma', narrow64='mfma' included): this layer of KeyedModel.forward_linear's narrow forms, as
        narrowed() decides it on this batch -- with `narrow` nothing is calibrated, and only narrow='mfma' on a calibrated layer measures and records (narrow_mode()).
        `narrow_split` (only with narrow='mfma'): a filled-in conv layer under 'split' runs the narrow split route where narrow_split_mode() allows it; a calibrated one measures
        and records that under its own key first.  Every other layer, and this one beyond NARROW32_MAX images, is what it is without the keyword.
        `narrow_taps` (only with `narrow`): a conv-taps layer's channel-lane launch carries KN_FLAG_NARROW_TAPS (kernel()); nothing is measured or recorded for it.
        `narrow_fill` (only with `narrow`): the same launches carry KN_FLAG_NARROW_FILL (kernel()); nothing is measured or recorded for it either."""
        if verbose():
            print('[keynet_amd.layer]: forward %s' % str(self))
        (xt, relu) = (x_affine.t(), fuse_relu or self.iskeyedrelu())
        (exact, keywords) = self.narrowed(ksp.NarrowForm.of(None, narrow, narrow_rows, narrow32, narrow64, narrow_linear, narrow_split=narrow_split, narrow_taps=narrow_taps, narrow_fill=narrow_fill), xt, relu)
        if exact == 'auto' and not narrow:
            if x_affine.is_cuda and torch.cuda.is_current_stream_capturing():
                raise _capi.KeynetHipError('keynet_amd: %s has not decided its arithmetic contract yet (exact=\'auto\' calibrates on the first batch, with host reads): '
                                           'run one eager forward before capturing a HIP graph (KeyedModel.capture does), or declare exact=True / False' % self._repr)
            y = self._calibrate(x_affine, relu)
            if absmax is not None:
                _absmax_into(y.t(), absmax)
            return y
        return self.W.torchdot(xt, relu=relu, exact=exact, absmax=absmax, **keywords).t()

    def narrowed(self, form, xt=None, relu=False):
        """What this layer makes of the ksp.NarrowForm `form`: (contract, keywords) -- the contract its operator runs under and the keywords that operator's torchdot /
        kernel() take (none on the wide forward).  `xt` ([cols, N]): the batch of a forward; None: a planner asking (launch()), which decides and measures nothing.
        An operator with a conv-taps handle (W.narrow_capable()): where the 64-column tile is asked for (narrow64='mfma'; with a batch: of more than NARROW32_MAX columns) a
        conv operator under False / 'bf16x3' takes it -- the wide kernel's association, covered by the wide decision: narrow_mode() is not consulted -- and everything else is what
        narrow=True, narrow64=True makes it; otherwise narrow='mfma' is narrow_mode()'s answer for this layer, measured on `xt` where a calibrated layer has no narrow record yet
        (a planner gets the channel-lane kernel).  Any other operator: `narrow_rows` / `narrow_linear` where it is a float32 CSR handle (W.rows_capable()), and a layer still
        'auto' runs in the reference's order for this call (to a planner it stays 'auto': not one launch).  `form.split` (narrow_split=True): ahead of narrow_mode(), a layer
        narrow_split_mode() puts on the narrow split route gets narrow='mfma', narrow_split=True (to a planner: not one launch); any other layer is what it is without it.
        `form.taps` (narrow_taps=True | 'packed'), `form.fill` (narrow_fill=True): handed on to every operator with a conv-taps handle, next to whatever `narrow` it gets."""
        (W, exact) = (self.W, getattr(self, '_exact', True))
        if not form.mode:
            # a layer calibration put on the Winograd form of its matrix-core launch (record: decided='mfma', form='wino'; the contract stays False)
            rec = getattr(self, '_contract_record', None)
            return ('wino' if exact is False and rec is not None and rec.get('form') == 'wino' else exact, {})
        if W.narrow_capable():
            taps = dict(dict(narrow_taps=form.taps) if form.taps else {}, **(dict(narrow_fill=True) if form.fill else {}))
            if form.tile64 and (xt is None or xt.shape[1] > ksp.NARROW32_MAX):
                mode = 'mfma' if isinstance(W, ksp.Conv2dTiledMatrix) and exact in (False, 'bf16x3') else True
                return (exact, dict(narrow=mode, narrow32=True, narrow64=mode, **taps))
            if form.split and self.narrow_split_mode(xt, relu):
                return (exact, dict(narrow='mfma', narrow32=form.narrow32, narrow64=form.narrow64, narrow_split=True, **taps))
            return (exact, dict(narrow=self.narrow_mode('mfma', xt, relu) if form.mode == 'mfma' else True, narrow32=form.narrow32, narrow64=form.narrow64, **taps))
        if exact == 'auto' and xt is not None:
            exact = True
        return (exact, dict(narrow_rows=form.rows, narrow_linear=form.linear) if (form.rows or form.linear) and W.rows_capable() else {})

    @staticmethod
    def kernel(W, contract, relu, device=None, narrow=False, narrow_rows=False, narrow32=False, narrow64=False, narrow_linear=False, narrow_split=False, narrow_taps=False, narrow_fill=False):
        """The one place that turns a decided contract into an operator handle and flags: (get_op, flags) of the kn_spmm launch that applies operator `W`
        under `contract`, get_op(device) -> the handle resident there.  None when that is not one launch: 'auto' (still to calibrate), 'split' on an operator that has a split form (Conv2dTiledMatrix._torchdot_split).
        The rules: 'split' forced on an operator without a split form, and 'bf16x3' on a non-conv operator, are the f32 matrix cores (False); a conv operator
        runs the order-preserving kernel under True, else the matrix cores (bf16x3: the emulation where operator and batch qualify); a plain SparseMatrix
        off the exact contract runs as a dense GEMM when it has such a handle (a large keyed nn.Linear); everything else -- tiled / factored CSR
        containers, float64 operators, small or sparse matrices -- has the reference's order only.
        The flags of the narrow forms (`narrow`, `narrow_rows`, `narrow32`, `narrow64`, `narrow_linear`: KeyedModel.forward_linear says what they select; no batch here, so
        nothing is refused and a keyword that needs `narrow` adds nothing without it):
        `narrow`: an operator that owns a conv-taps handle (W.narrow_capable()) is ONE launch under EVERY contract, the undecided and the two-step ones included --
        KN_FLAG_NARROW next to the flags the contract sets anyway (the library ignores them at these widths); with `narrow32` also KN_FLAG_NARROW32, with `narrow64`
        KN_FLAG_NARROW32 | KN_FLAG_NARROW64.  Every other operator keeps the flags it has without these three.
        narrow='mfma': a CONV operator under a re-ordering contract (False, 'bf16x3', 'split') carries KN_FLAG_NARROW_MFMA instead and no contract flag; under True / 'auto',
        and for every other operator, exactly narrow=True.  (Whether a CALIBRATED layer may pass 'mfma' here is narrow_mode()'s decision.)  With narrow64='mfma' a conv
        operator under False / 'bf16x3' adds KN_FLAG_NARROW64_MFMA (the 64-column tile at 33 .. 64 columns; the library ignores the bit below); every other case is narrow64=True.
        `narrow_rows`, `narrow_linear`: KN_FLAG_NARROW_ROWS, KN_FLAG_NARROW_LINEAR on an operator that runs in the stored order on its own float32 CSR handle
        (W.rows_capable(); not a float64 operator, not a SparseMatrix a re-ordering contract put on its dense handle, not a conv-taps operator), `narrow` or not.
        `narrow_split` (with narrow='mfma'): a conv operator with a split form under 'split' is NOT one launch (None) -- the narrow split route of up to NARROW32_MAX columns,
        Conv2dTiledMatrix._torchdot_split_narrow, which the operator's torchdot takes where narrow_split_route() offers it at the batch's width, asking again without the
        keyword where not; on every other operator and contract the keyword adds nothing.
        `narrow_taps` (with `narrow`): KN_FLAG_NARROW_TAPS exactly where KN_FLAG_NARROW is set -- inside a narrow='mfma' call that is the operators under True / 'auto' and
        the non-conv ones with a conv-taps handle; the library runs the tap-resident kernel on an eligible operator at up to NARROW_MAX columns and ignores the bit elsewhere.
        narrow_taps='packed': KN_MODIFIER_NARROW_TAPS32 next to it, on exactly the same launches -- with KN_FLAG_NARROW32 the library runs convtaps_narrow_taps32_kernel on an
        eligible operator at NARROW_MAX + 1 .. NARROW32_MAX columns; up to NARROW_MAX columns the call is narrow_taps=True.
        narrow_taps='pairs': KN_MODIFIER_NARROW_TAPS_PAIRS next to both bits, on exactly the same launches -- at up to NARROW_MAX columns the library runs
        convtaps_narrow_taps_pairs_kernel on an eligible operator of more than 64 output channels; beyond, the call is narrow_taps='packed'.
        `narrow_fill` (with `narrow`): KN_FLAG_NARROW_FILL (_capi.KN_MODIFIER_NARROW_FILL) on exactly the same launches -- with narrow_split=True those are the layers not on the
        route; the library runs convtaps_narrow_fill_kernel on an eligible (filled-in) operator at up to NARROW32_MAX columns and ignores the bit elsewhere."""
        form = ksp.NarrowForm.of(None, narrow, narrow_rows, narrow32, narrow64, narrow_linear, narrow_split=narrow_split, narrow_taps=narrow_taps, narrow_fill=narrow_fill)
        conv = isinstance(W, ksp.Conv2dTiledMatrix)
        wino = contract == 'wino'          # the matrix cores (False) with KN_MODIFIER_WINO on a conv operator's wide launch: no contract of its own (narrowed() passes it for a layer whose record holds form='wino')
        if wino:
            contract = False
        if form.split and conv and contract == 'split' and W.narrow_capable() and W.split_capable():
            return None
        lane = bool(form.mode) and W.narrow_capable()       # one launch of a narrow conv kernel, whatever the contract
        mfma = lane and form.mode == 'mfma' and conv and contract in (False, 'bf16x3', 'split')      # (the library falls back to the channel-lane kernel on an ineligible operator)
        if not lane:
            if contract == 'auto' or (contract == 'split' and conv and W._taps is not None):
                return None
            if contract == 'split' or (contract == 'bf16x3' and not conv):
                contract = False
        (get_op, exact, bf16x3) = (W._device_op, contract is True or not conv, contract == 'bf16x3')
        if not conv and not contract and type(W) is SparseMatrix and not W.is_float64() and W._dense_device_op(device) is not None:
            (get_op, exact) = (W._dense_device_op, False)
        stored = not lane and not conv and get_op == W._device_op and W.rows_capable()      # the stored order on the operator's own float32 CSR handle
        if mfma:
            (exact, bf16x3) = (False, False)
        return (get_op, (_capi.KN_FLAG_RELU if relu else 0) | (_capi.KN_FLAG_EXACT if exact else 0) | (_capi.KN_FLAG_BF16X3 if bf16x3 else 0) |
                (_capi.KN_FLAG_NARROW_MFMA if mfma else _capi.KN_FLAG_NARROW if lane else 0) | (_capi.KN_FLAG_NARROW_TAPS if form.taps and lane and not mfma else 0) | (_capi.KN_MODIFIER_NARROW_TAPS32 if form.taps in ('packed', 'pairs') and lane and not mfma else 0) | (_capi.KN_MODIFIER_NARROW_TAPS_PAIRS if form.taps == 'pairs' and lane and not mfma else 0) | (_capi.KN_MODIFIER_NARROW_FILL if form.fill and lane and not mfma else 0) | (_capi.KN_FLAG_NARROW32 if lane and form.narrow32 else 0) | (_capi.KN_FLAG_NARROW64 if lane and form.narrow64 else 0) |
                (_capi.KN_FLAG_NARROW64_MFMA if mfma and form.tile64 and contract in (False, 'bf16x3') else 0) |
                (_capi.KN_FLAG_NARROW_ROWS if form.rows and stored else 0) | (_capi.KN_FLAG_NARROW_LINEAR if form.linear and stored else 0) |
                (_capi.KN_MODIFIER_WINO if wino and conv and not lane else 0))

    def launch(self, device, relu=False, narrow=False, narrow_rows=False, narrow32=False, narrow64=False, narrow_linear=False, narrow_split=False, narrow_taps=False, narrow_fill=False):
        """This layer under its contract in force as one launch on `device` (`relu`: the unkeyed nn.ReLU behind it is fused in), or None when it is not one
        kn_spmm launch: see kernel(); a float64 operator (its own kernel and a float64 result: kn_spmm_f64).  What the key-net's planners read
        (KeyedModel._chain_op / _overlap_plan); forward() -> W.torchdot() runs the same rule.  `narrow`, `narrow_rows`, `narrow32`, `narrow64`, `narrow_linear`: the launch
        forward() issues under them (narrowed(); without `narrow` the others say nothing), except that a planner has no batch: a layer still 'auto' is not one launch,
        narrow='mfma' on a calibrated layer without a narrow record answers the channel-lane kernel, and narrow64='mfma' asks for the launch of 33 .. 64 columns.  `narrow_split`: a layer
        on the narrow split route (declared 'split', or an accepted narrow_split record) is not one launch; one still to measure answers what it answers without the keyword.  `narrow_taps`, `narrow_fill`: the launch carries KN_FLAG_NARROW_TAPS, KN_FLAG_NARROW_FILL where kernel() sets them."""
        W = self.W
        (exact, keywords) = self.narrowed(ksp.NarrowForm.of(None, narrow, narrow_rows, narrow32, narrow64, narrow_linear, narrow_split=narrow_split, narrow_taps=narrow_taps, narrow_fill=narrow_fill))
        kernel = None if W.is_float64() else self.kernel(W, exact, relu or self.iskeyedrelu(), device, **keywords)
        if kernel is None:
            return None
        return Launch(kernel[0](device), kernel[1], int(W.shape[0]), int(W.shape[1]), isinstance(W, ksp.Conv2dTiledMatrix), 'Linear' in self._layertype,
                      getattr(self, '_exact', True) is True)

    # -- float-key contract: decided by calibration, re-screened on every forward --------------------------------------
    RESCREEN_FACTOR = 2.0        # a layer is re-calibrated when max |x| exceeds the calibrated value by more than this factor
    ALLOW_SPLIT = True           # calibration offers the split application to filled-in conv operators (set False to put the fused kernels side by side with it)

    def screened(self):
        """Runs this layer on a re-ordering kernel (matrix cores) BY A CALIBRATION DECISION?  Then every forward must check that the
        decision still covers its input (a layer forced there with exact_mode(False) / 'bf16x3' is the caller's responsibility)."""
        rec = getattr(self, '_contract_record', None)
        return getattr(self, '_exact', True) in (False, 'bf16x3', 'split') and rec is not None and rec.get('max_abs_x') is not None

    def _screen_key(self, narrow):
        """Where the record a narrow forward screens sits inside the calibration record: 'narrow', or under narrow='split' (a narrow_split=True forward) 'narrow_split' for a layer
        that forward runs on the narrow split route by a measurement (narrow_split_screened(): narrowed() asks for the route first)."""
        return 'narrow_split' if narrow == 'split' and self.narrow_split_screened() else 'narrow'

    def screen_record(self, narrow=False):
        """The record whose max_abs_x a forward screens: the calibration record, or under `narrow` the narrow record inside it (narrow_record(); narrow='split': _screen_key)."""
        return self._contract_record[self._screen_key(narrow)] if narrow else self._contract_record

    def rescreen(self, xmax, narrow=False):
        """max |x| of a later batch against the calibrated one: True = the decision does not cover this batch (re-calibrate).  The measured
        difference of a re-ordered f32 sum scales with the activations while the tolerance 1e-5 max(1, |y|) has a floor, so a decision
        taken with 2x headroom (accepted at <= 0.5 tol) is kept for inputs up to RESCREEN_FACTOR x the calibrated magnitude.
        `narrow`: against the narrow record (the measurement of the matrix-core narrow kernel) instead of the wide one."""
        cal = float(self.screen_record(narrow)['max_abs_x'])
        if not np.isfinite(cal):
            return False                                          # calibrated on non-finite activations: there is no larger batch to learn from
        return not (xmax <= self.RESCREEN_FACTOR * cal)          # also True for NaN

    def unscreen(self, narrow=False):
        """Drop the record a screen has outgrown: the layer is 'auto' again (decided by the next forward, on that batch); under `narrow` only the narrow
        record goes (measured again by the next narrow='mfma' pass) and the wide decision stays."""
        if narrow:
            self._contract_record.pop(self._screen_key(narrow), None)       # (narrow='split': only the narrow_split record of a layer on that route)
        else:
            self._exact = 'auto'
            self.__dict__.pop('_contract_record', None)

    # -- narrow='mfma': the matrix-core narrow kernel under the layer's contract ------------------------------------------
    def narrow_record(self):
        """The record of this layer's narrow='mfma' measurement (a calibrated layer only), or None."""
        rec = getattr(self, '_contract_record', None)
        return None if rec is None else rec.get('narrow')

    def narrow_screened(self):
        """Does a narrow='mfma' forward run this layer on the matrix-core narrow kernel BY A MEASUREMENT (then it re-screens max |x| like the wide forward)?"""
        rec = self.narrow_record()
        return self.screened() and rec is not None and rec.get('decided') == 'mfma' and rec.get('max_abs_x') is not None

    def narrow_mode(self, narrow, xt=None, relu=False):
        """What `narrow='mfma'` means for this layer now: 'mfma' (KN_FLAG_NARROW_MFMA) or True (the channel-lane kernel, the bits of narrow=True).
        Contract True, or 'auto' still undecided, or not a conv-taps operator: True, nothing decided.  A DECLARED re-ordering contract (exact=False,
        'bf16x3' forced): 'mfma', unscreened -- the caller's responsibility, as on the wide path.  A contract DECIDED BY CALIBRATION (screened()): the kernel is
        one more association of the sum that the wide record does not cover, so the first eager call with a batch `xt` ([cols, N]; of a narrow32 batch the 8-column
        window that holds its largest |x|: a column's bits do not depend on the width of the launch, so the record covers NV = 16 | 32 too) measures it -- the
        channel-lane kernel and the matrix-core kernel on these very columns, gate() -- and accepts by _calibrate's rule: the worst element uses at most half
        its tolerance, a quarter where the bound screen 2 eps32 max_row sum|a| max|x| <= 1e-5 fails.  The outcome is _contract_record['narrow'] = {decided:
        'mfma' | 'exact', gate_ratio, max_abs_x, measured_on_columns, ...}; the wide decision and its fields are never touched.  Without a batch (a planner
        asking) an unmeasured layer answers True."""
        W = self.W
        exact = getattr(self, '_exact', True)
        if narrow != 'mfma' or not isinstance(W, ksp.Conv2dTiledMatrix) or not W.narrow_capable() or exact not in (False, 'bf16x3', 'split'):
            return True if narrow else False
        if not self.screened():
            return 'mfma'
        rec = self.narrow_record()
        if rec is None:
            if xt is None:
                return True
            if xt.is_cuda and torch.cuda.is_current_stream_capturing():
                raise _capi.KeynetHipError('keynet_amd: %s has not measured the matrix-core narrow kernel yet (host reads): run one eager narrow=\'mfma\' forward '
                                           'before capturing a HIP graph (KeyedModel.capture does)' % self._repr)
            rec = self._contract_record['narrow'] = self._measure_narrow(xt, relu)
        return 'mfma' if rec['decided'] == 'mfma' else True

    def _measure_narrow(self, xt, relu):
        """The narrow record of a calibrated layer, measured on the batch xt ([cols, N]): see narrow_mode().  Of more than NARROW_MAX columns the window of
        NARROW_MAX that holds the largest |x| is measured, placed as _calibrate places its window; max_abs_x is the maximum of those columns = of the batch."""
        W = self.W
        xt = ksp._device_block(xt)
        n = int(xt.shape[1])
        if n > ksp.NARROW_MAX:
            c0 = min((int(torch.argmax(xt.detach().abs().amax(dim=0))) // ksp.NARROW_MAX) * ksp.NARROW_MAX, n - ksp.NARROW_MAX)
            (xt, n) = (xt[:, c0:c0 + ksp.NARROW_MAX].contiguous(), ksp.NARROW_MAX)
        dev = xt.device
        with torch.cuda.device(xt.device):
            # the widest of these columns the library runs on the matrix-core kernel (a shape rule of the handle may keep a wide batch of a layer on the
            # channel-lane kernel, where both sides of the measurement would be the same launch): the measurement is of that kernel, on those columns
            for m in (n, 4, 2, 1):
                plan = W._device_op(dev).plan(max(min(m, n), 1), _capi.KN_FLAG_NARROW_MFMA | (_capi.KN_FLAG_RELU if relu else 0))
                if 'convtaps_narrow_mfma_kernel' in plan:
                    break
        if 0 < m < n and 'convtaps_narrow_mfma_kernel' in plan:
            (xt, n) = (xt[:, :m].contiguous(), m)
        if n == 0 or 'convtaps_narrow_mfma_kernel' not in plan:
            return dict(layer=self._repr, decided='exact', reason='an empty batch' if n == 0 else 'the operator has no matrix-core narrow form (more than two slots on a (pixel, tap) pair)',
                        gate_ratio=None, max_abs_x=None, measured_on_columns=n)
        xmax = float(xt.detach().abs().max())
        asum = getattr(self, '_abs_rowsum', None)
        if asum is None:
            asum = self._abs_rowsum = W.max_abs_rowsum()
        bound = 2.0 * EPS32 * asum * xmax
        ye = W.torchdot(xt, relu=relu, exact=True, narrow=True)
        ym = W.torchdot(xt, relu=relu, exact=False, narrow='mfma')
        (ratio, measured, tol, dmax) = gate(ym, ye)
        ok = ratio <= 0.5 and (bound <= FLOAT_KEY_ATOL or ratio <= 0.25)
        if not ok:
            _log.warning('keynet_amd: %s keeps the channel-lane kernel on narrow forwards: matrix-core narrow result off by %.3g where the tolerance is %.3g', self._repr, measured, tol)
        return dict(layer=self._repr, decided='mfma' if ok else 'exact', measured_narrow_mfma_vs_exact=measured, tol=tol, bound=bound, gate_ratio=ratio, max_abs_diff=dmax,
                    max_abs_x=xmax, measured_on_columns=n)

    # -- narrow_split=True: the narrow split route of a filled-in conv layer under 'split' ---------------------------------------------------
    def narrow_split_record(self):
        """The record of this layer's narrow_split measurement (a layer calibration decided 'split' only), or None."""
        rec = getattr(self, '_contract_record', None)
        return None if rec is None else rec.get('narrow_split')

    def narrow_split_screened(self):
        """Does a narrow_split=True forward run this layer on the narrow split route BY A MEASUREMENT (then it re-screens max |x| against that record)?"""
        rec = self.narrow_split_record()
        return self.screened() and rec is not None and rec.get('decided') == 'split' and rec.get('max_abs_x') is not None

    def narrow_split_mode(self, xt=None, relu=False):
        """Does a narrow='mfma', narrow_split=True forward run this layer on the narrow split route (Conv2dTiledMatrix._torchdot_split_narrow) now?  Only a conv-taps operator
        with a split form whose contract in force is 'split', at a width the operator offers the route for (narrow_split_route: the cost rule, and the channel-mixing operator on
        the matrix-core narrow kernel; a planner, without a batch, is not asked about a width).  DECLARED 'split' (exact_mode('split')): yes, unscreened, as every declared
        re-ordering contract.  DECIDED 'split' by calibration (screened()): the route is one more association of the sum that the wide record does not cover, so the first eager
        call with a batch measures it the way narrow_mode() measures the matrix-core narrow kernel -- the channel-lane kernel against the route on these very columns (of a
        wider batch the 8-column window with the largest |x|: per image neither side's bits depend on the width), gate(), accepted by _calibrate's rule -- into a record of its
        OWN, _contract_record['narrow_split'] = {decided: 'split' | 'exact', gate_ratio, max_abs_x, measured_on_columns, ...}.  The 'narrow' record, the wide fields and what
        narrow='mfma' without the keyword does are never touched.  A layer calibration sent to 'exact' is out of reach: it stays on the channel-lane kernel."""
        W = self.W
        if not isinstance(W, ksp.Conv2dTiledMatrix) or not W.narrow_capable() or getattr(self, '_exact', True) != 'split' or not W.split_capable():
            return False
        if xt is not None and not W.narrow_split_route(int(xt.shape[1]), relu, xt.device if xt.is_cuda else None):
            return False
        if not self.screened():
            return True
        rec = self.narrow_split_record()
        if rec is None:
            if xt is None:
                return False
            if xt.is_cuda and torch.cuda.is_current_stream_capturing():
                raise _capi.KeynetHipError('keynet_amd: %s has not measured the narrow split route yet (host reads): run one eager narrow=\'mfma\', narrow_split=True forward '
                                           'before capturing a HIP graph (KeyedModel.capture does)' % self._repr)
            rec = self._contract_record['narrow_split'] = self._measure_narrow_split(xt, relu)
        return rec['decided'] == 'split'

    def _measure_narrow_split(self, xt, relu):
        """The narrow_split record of a layer calibration decided 'split', measured on the batch xt ([cols, N]): see narrow_split_mode().  Of more than NARROW_MAX columns the
        window of NARROW_MAX that holds the largest |x| is measured, placed as _measure_narrow places its window."""
        W = self.W
        xt = ksp._device_block(xt)
        n = int(xt.shape[1])
        if n > ksp.NARROW_MAX:
            c0 = min((int(torch.argmax(xt.detach().abs().amax(dim=0))) // ksp.NARROW_MAX) * ksp.NARROW_MAX, n - ksp.NARROW_MAX)
            (xt, n) = (xt[:, c0:c0 + ksp.NARROW_MAX].contiguous(), ksp.NARROW_MAX)
        if n == 0 or not W.narrow_split_route(n, relu, xt.device):
            return dict(layer=self._repr, decided='exact', reason='an empty batch' if n == 0 else 'the operator does not offer the narrow split route on the measured columns',
                        gate_ratio=None, max_abs_x=None, measured_on_columns=n)
        xmax = float(xt.detach().abs().max())
        asum = getattr(self, '_abs_rowsum', None)
        if asum is None:
            asum = self._abs_rowsum = W.max_abs_rowsum()
        bound = 2.0 * EPS32 * asum * xmax
        ye = W.torchdot(xt, relu=relu, exact=True, narrow=True)
        ys = W._torchdot_split_narrow(xt, relu=relu)
        (ratio, measured, tol, dmax) = gate(ys, ye)
        ok = ratio <= 0.5 and (bound <= FLOAT_KEY_ATOL or ratio <= 0.25)
        if not ok:
            _log.warning('keynet_amd: %s keeps the channel-lane kernel on narrow_split forwards: narrow split result off by %.3g where the tolerance is %.3g', self._repr, measured, tol)
        else:
            with torch.cuda.device(xt.device):                 # the slot records the channel-lane side of the measurement built again (_calibrate released them for a 'split' layer)
                W._device_op(xt.device).release_side_tables()
        return dict(layer=self._repr, decided='split' if ok else 'exact', measured_narrow_split_vs_exact=measured, tol=tol, bound=bound, gate_ratio=ratio, max_abs_diff=dmax,
                    max_abs_x=xmax, measured_on_columns=n)

    def mfma_capable(self, device=None):
        """Does tolerance mode run this layer on the matrix cores at all (conv-taps operator, or a large dense nn.Linear)?"""
        W = self.W
        if isinstance(W, ksp.Conv2dTiledMatrix):
            return True
        return type(W) is SparseMatrix and torch.cuda.is_available() and W._dense_device_op(device) is not None

    def _calibrate(self, x_affine, relu):
        """First forward of a layer whose contract is 'auto': decide ONCE, on this batch, between the matrix cores and the
        order-preserving kernels, so that the float-key tolerance holds in the reference's own form -- element-wise
        |y_mfma - y_reference| <= 1e-5 + 1e-5 |y_reference| (np.allclose(atol=1e-5): test/test_keynet.py:33,196,218), unconditioned.

        An f32 evaluation of sum_j a_j x_j in another order than the reference's differs from it by about 2 eps32 sum|a_j x_j|.  With keys
        that carry large coefficients (TiledOrthogonalKeynet: gamma = 100 bias keys) that is 1e-4 on unit-scale outputs -- the
        reference's own f32 result is that far from the exact sum too -- so such a layer cannot meet 1e-5 against scipy on ANY
        re-ordered arithmetic and must run in the reference's order.  Screen: bound = 2 eps32 (max_row sum|a|) max|x| against the
        tolerance's floor 1e-5 (operator factor from the host description, activation factor reduced on the device).  Check: the
        order-preserving kernel on up to 256 batch columns of this very input -- the window that holds the batch's largest |x| --
        compared with the matrix-core result element by element (always for conv operators -- one launch; for a dense nn.Linear only when
        the screen does not show 2x headroom, because its CSR twin has to be uploaded first).  The layer switches to exact when the worst
        element uses more than half its tolerance, or when the screen fails and the measurement does not show 4x headroom.  (The 2x
        headroom of every accepted decision is what rescreen() relies on: inputs up to RESCREEN_FACTOR x the calibrated magnitude.)"""
        W = self.W
        xt = x_affine.t()
        dev = xt.device if xt.is_cuda else None
        if xt.shape[1] == 0:
            # an empty batch (a rank whose shard of a small batch is empty) decides nothing: the layer stays 'auto' and calibrates on the first batch that holds an image
            return W.torchdot(xt, relu=relu, exact=True).t()
        rec = dict(layer=self._repr, decided='exact', reason='no matrix-core path for this operator')
        if not self.mfma_capable(dev):
            self._exact = True
            self._contract_record = rec
            return W.torchdot(xt, relu=relu, exact=True).t()
        # the measured window: up to 256 batch columns (a multiple of 128 wide when the batch allows), placed over the column with the largest |x|
        n = int(xt.shape[1])
        cols = min(n, 256)
        colmax = xt.detach().abs().amax(dim=0)
        xmax = float(colmax.max()) if n else 0.0
        c0 = 0
        if n > cols:
            c0 = min((int(torch.argmax(colmax)) // cols) * cols, n - cols)
        win = slice(c0, c0 + cols)
        # opt-in first candidate (KeyedModel.exact_mode('auto-bf16x3')): f32 products emulated on the bf16 matrix pipe (KN_FLAG_BF16X3).
        # It is taken only with 4x headroom under the tolerance on this batch; otherwise the decision below is made as usual.
        if getattr(self, '_allow_bf16x3', False) and isinstance(W, ksp.Conv2dTiledMatrix):
            xs = xt[:, win] if cols % 128 == 0 else None
            with torch.cuda.device(xt.device):
                eligible = xs is not None and 'bf16x3' in W._device_op(dev).plan(cols, _capi.KN_FLAG_BF16X3 | (_capi.KN_FLAG_RELU if relu else 0))
            if eligible:
                yb = W.torchdot(xs, relu=relu, exact='bf16x3')
                ye = W.torchdot(xs, relu=relu, exact=True)
                (ratio, meas, tol_b, dmax) = gate(yb, ye)
                ymax_b = float(ye.abs().max())
                del yb, ye
                if ratio <= 0.25:
                    self._exact = 'bf16x3'
                    self._contract_record = dict(layer=self._repr, decided='bf16x3', measured_bf16x3_vs_exact=meas, tol=tol_b, gate_ratio=ratio, max_abs_diff=dmax,
                                                 max_abs_y=ymax_b, measured_on_columns=cols, measured_from_column=c0, max_abs_x=xmax)
                    return W.torchdot(xt, relu=relu, exact='bf16x3').t()
        asum = getattr(self, '_abs_rowsum', None)
        if asum is None:
            asum = self._abs_rowsum = W.max_abs_rowsum()
        bound = 2.0 * EPS32 * asum * xmax
        # first candidate for a FILLED-IN factored conv (a key whose inverse is dense inside its blocks: 500 - 5 400 slots per output pixel): the split
        # application -- spatial mixing per tap, then channel mixing (Conv2dTiledMatrix._split_ops: 1/10 - 1/30 of the fused operator's multiply-adds).
        # Another association of the same sum: measured against the order-preserving kernel and accepted by the rule the matrix-core kernel is held to below.
        ye_win = None
        if isinstance(W, ksp.Conv2dTiledMatrix) and self.ALLOW_SPLIT and W.split_capable(n):
            ye_win = W.torchdot(xt[:, win], relu=relu, exact=True)
            try:
                ys = W.torchdot(xt, relu=relu, exact='split')
                (ratio_s, meas_s, tol_s, dmax_s) = gate(ys[:, win], ye_win)
            except (torch.cuda.OutOfMemoryError, _capi.KeynetHipError) as e:
                # the candidate needs a resident spatial CSR, a second operator and the intermediate (several ranks on one device, a smaller device): not offered then --
                # the fused kernels below need nothing beyond the operator that is already resident (round-5 advisor finding: this used to abort the first forward)
                if isinstance(e, _capi.KeynetHipError) and 'memory' not in str(e).lower():
                    raise
                _log.warning('keynet_amd: %s: the split application does not fit this device now (%s); deciding between the fused kernels', self._repr, str(e)[:120])
                W._op_split = None
                torch.cuda.empty_cache()
                (ys, ratio_s) = (None, float('inf'))
            if ratio_s <= 0.5 and (bound <= FLOAT_KEY_ATOL or ratio_s <= 0.25):
                self._exact = 'split'
                self._contract_record = dict(layer=self._repr, decided='split', max_abs_rowsum=asum, max_abs_x=xmax, max_abs_y=float(ys.abs().max()), tol=tol_s, bound=bound,
                                             measured_split_vs_exact=meas_s, gate_ratio=ratio_s, max_abs_diff=dmax_s, measured_on_columns=cols, measured_from_column=c0,
                                             fill_factor=W.fill_factor())
                # the order-preserving measurement above built the operator's slot records (16 bytes per slot: 0.4 - 4 GB per layer of the doubly-stochastic VGG-16); a layer that
                # runs split does not use them again until it is re-calibrated (round-5 advisor finding)
                with torch.cuda.device(xt.device):
                    W._device_op(dev).release_side_tables()
                return ys.t()
            del ys
        # candidate for a keyed 3 x 3 conv whose plan takes it: the 1-D Winograd F(2,3) form of the matrix-core launch (Conv2dTiledMatrix.wino_offered: the cost rule;
        # the plan: the library's eligibility).  The 2 eps rowsum bound does not describe this association (sums and differences of activations, halved tap sums), so it is
        # held to the rule of the bf16x3 candidate: a quarter of the gate on the measured window.  The contract stays 'mfma'; the record says which form runs.
        if isinstance(W, ksp.Conv2dTiledMatrix) and cols % 128 == 0 and W.wino_offered(cols) and W.wino_offered(n) and W.wino_planned(cols, relu, dev):
            if ye_win is None:
                ye_win = W.torchdot(xt[:, win], relu=relu, exact=True)
            yw = W.torchdot(xt[:, win], relu=relu, exact='wino')
            (ratio_w, meas_w, tol_w, dmax_w) = gate(yw, ye_win)
            ymax_w = float(ye_win.abs().max())
            del yw
            if ratio_w <= 0.25:
                self._exact = False
                self._contract_record = dict(layer=self._repr, decided='mfma', form='wino', max_abs_rowsum=asum, max_abs_x=xmax, max_abs_y=ymax_w, tol=tol_w, bound=bound,
                                             measured_mfma_vs_exact=meas_w, gate_ratio=ratio_w, max_abs_diff=dmax_w, measured_on_columns=cols, measured_from_column=c0)
                return W.torchdot(xt, relu=relu, exact='wino').t()
        y = W.torchdot(xt, relu=relu, exact=False)
        ymax = float(y.abs().max())
        (ratio, measured, tol, dmax) = (None, None, FLOAT_KEY_ATOL, None)
        if isinstance(W, ksp.Conv2dTiledMatrix) or not (bound <= FLOAT_KEY_ATOL / self.RESCREEN_FACTOR):
            ye = ye_win if ye_win is not None else W.torchdot(xt[:, win], relu=relu, exact=True)
            (ratio, measured, tol, dmax) = gate(y[:, win].to(ye.device), ye)
            del ye
        # (a difference that is not finite -- Inf / NaN activations -- cannot be bounded: the reference's order it is)
        switch = ratio is not None and not (ratio <= 0.5 and (bound <= FLOAT_KEY_ATOL or ratio <= 0.25))
        rec = dict(layer=self._repr, decided='exact' if switch else 'mfma', max_abs_rowsum=asum, max_abs_x=xmax, max_abs_y=ymax, tol=tol, bound=bound,
                   measured_mfma_vs_exact=measured, gate_ratio=ratio, max_abs_diff=dmax, measured_on_columns=None if ratio is None else cols,
                   measured_from_column=None if ratio is None else c0)
        self._exact = bool(switch)
        self._contract_record = rec
        if switch:
            _log.warning('keynet_amd: %s runs in the reference\'s accumulation order from now on: matrix-core result off by %.3g where the tolerance is %.3g '
                         '(1e-5 + 1e-5 |y|, element-wise; bound 2 eps sum|a| max|x| = %.3g); KeyedModel.exact_mode(False) forces the matrix cores', self._repr, measured, tol, bound)
            y = W.torchdot(xt, relu=relu, exact=True)
        return y.t()

    def decrypt(self, Ainv, x_affine):
        """Apply a decryption key to this layer's output (keynet/layer.py:95-99)."""
        if scipy.sparse.issparse(Ainv):
            Ainv = SparseMatrix(Ainv)
        return Ainv.torchdot(x_affine.t()).t()

    def nnz(self):
        assert self.W is not None, 'Layer not keyed'
        return self.W.nnz()
