"""Operator containers of the keyed forward, HIP-backed: the objects stored in KeyedLayer.W.

Mirror of the reference's operator interface (keynet/sparse.py:419-835): SparseMatrix, TiledMatrix, DiagonalTiledMatrix,
Conv2dTiledMatrix with torchdot / dot / nnz / shape / tocoo / tocsr / transpose / clone.  The host keeps the defining
arrays (scipy matrix or blocks+tiles) for the structural methods and pickling; `torchdot` -- the hot path -- always runs
in libkeynet_hip.so on an MI355X (there is no CPU route: a missing library or device raises).

Build-time (host, offline) constructors live here too, restated and vectorised: Toeplitz matrices of conv / avgpool
layers (keynet/sparse.py:122-212) and the tilers (keynet/sparse.py:519-571, 692-776).
"""
import collections
import copy
import functools
import numpy as np
import scipy.sparse
import torch

from . import _capi


# ------------------------------------------------------------------------------------------------------------------
# helpers
def is_scipy_sparse(A):
    return scipy.sparse.issparse(A)


def _stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def _compute_dtype(dt):
    """The dtype scipy's product of an operator of dtype `dt` with float32 activations runs and returns in (keynet/sparse.py:488-492:
    `x_torch.type(torch.FloatTensor)` against `self._matrix` as it is; numpy up-casts the pair)."""
    return np.dtype(np.float64) if np.result_type(dt, np.float32) == np.float64 else np.dtype(np.float32)


def _stored_order_csr(M):
    """(indptr, indices, data) whose per-row order equals the accumulation order of scipy's matvec for M's format:
    CSR as stored (csr_matvecs); COO in entry order (coo_matmat_dense); CSC column-major (csc_matvecs).  Nothing is
    sorted or summed -- keyed matrices are non-canonical and the order is part of the result.  The values keep the dtype scipy
    computes in against float32 activations (numpy's up-cast rule: float32 stays float32, float64 -- and integer types -- compute in float64)."""
    vdt = _compute_dtype(M.dtype)
    if M.format == 'csr':
        return (np.asarray(M.indptr, dtype=np.int32), np.asarray(M.indices, dtype=np.int32), np.asarray(M.data, dtype=vdt))
    if M.format == 'csc':
        cols = np.repeat(np.arange(M.shape[1], dtype=np.int64), np.diff(M.indptr))
        (rows, vals) = (np.asarray(M.indices, dtype=np.int64), M.data)
    else:
        C = M if M.format == 'coo' else M.tocoo()
        (rows, cols, vals) = (np.asarray(C.row, dtype=np.int64), np.asarray(C.col, dtype=np.int64), C.data)
    order = np.argsort(rows, kind='stable')
    indptr = np.zeros(M.shape[0] + 1, dtype=np.int64)
    np.add.at(indptr, rows + 1, 1)
    return (np.cumsum(indptr).astype(np.int32), cols[order].astype(np.int32), np.asarray(vals, dtype=vdt)[order])


def _on_device(W, attr, make, device=None):
    """Per-device cache of a container's operator handle: a kn_handle_t lives in ONE GPU's HBM, so it is created under the
    device of the activations it will multiply (not whatever device happens to be current) and looked up by device index.
    `W.<attr> = None` anywhere else drops every cached handle."""
    idx = torch.cuda.current_device() if (device is None or device.index is None) else device.index
    cache = getattr(W, attr, None)
    if not isinstance(cache, dict):
        cache = {}
        setattr(W, attr, cache)
    if idx not in cache:
        with torch.cuda.device(idx):
            cache[idx] = make()
    return cache[idx]


def _device_block(x):
    """x (any device / dtype / strides) -> the detached float32 contiguous block on the GPU that the kernels read (a host tensor goes to the current
    device; the reference coerces to FloatTensor silently, keynet/sparse.py:489-491)."""
    if not torch.cuda.is_available():
        raise _capi.KeynetHipError('keynet_amd: no MI355X visible -- the keyed forward has no CPU fallback')
    xd = x.detach()
    if xd.dtype != torch.float32:
        xd = xd.float()
    if not xd.is_cuda:
        xd = xd.cuda()
    return xd if xd.is_contiguous() else xd.contiguous()


def _run_torchdot(W, x, relu=False, exact=True, absmax=None, narrow=False, narrow_rows=False, narrow32=False, narrow64=False, narrow_linear=False, narrow_split=False, narrow_taps=False, narrow_fill=False):
    """Y = W.X on the GPU under the contract `exact`, on the handle and flags of KeyedLayer.kernel.  x: [cols, N], torch tensor (any device / strides) or ndarray.
    Returns [rows, N] on x's device: float32, or for a float64 operator the float64 block scipy returns for it (kn_spmm_f64; the activations are
    float32 either way).  `narrow`, `narrow_rows`, `narrow32`, `narrow64`, `narrow_linear` (narrow64='mfma' included): the narrow forms of the product
    (KeyedModel.forward_linear), each allowed on its own here (_narrow_args with `alone`: a container's torchdot takes the ones its operator has a form for);
    which flag each one sets on which operator is KeyedLayer.kernel's rule.  `narrow_split` (only with narrow='mfma'): a filled-in conv operator under 'split' runs the
    narrow split route where it has one at this width (Conv2dTiledMatrix.narrow_split_route), else exactly the call without the keyword.  `narrow_taps` (only with
    `narrow`): KN_FLAG_NARROW_TAPS next to KN_FLAG_NARROW -- the tap-resident channel-lane kernel on an eligible conv-taps operator, the same bits.  `narrow_fill` (only
    with `narrow`): KN_FLAG_NARROW_FILL next to KN_FLAG_NARROW -- the tap-resident kernel of FILLED-IN conv-taps operators at up to NARROW32_MAX columns, the same bits."""
    from .layer import KeyedLayer            # (layer.py imports this module)
    x = torch.as_tensor(x)
    assert W.shape[1] == x.shape[0], 'Non-conformal shape for W=%s, x=%s' % (str(W.shape), str(tuple(x.shape)))
    xd = _device_block(x)
    n = xd.shape[1]
    _narrow_args(n, narrow, narrow_rows, 'batch columns', True, narrow32, narrow64, narrow_linear, narrow_split, narrow_taps, narrow_fill)
    kernel = KeyedLayer.kernel(W, exact, relu, xd.device, narrow, narrow_rows, narrow32, narrow64, narrow_linear, narrow_split, narrow_taps, narrow_fill)
    split_narrow = kernel is None and bool(narrow_split) and isinstance(W, Conv2dTiledMatrix) and W.narrow_capable()      # (kernel()'s one "not one launch" among the narrow conv calls)
    if split_narrow and not W.narrow_split_route(n, relu, xd.device):
        (kernel, split_narrow) = (KeyedLayer.kernel(W, exact, relu, xd.device, narrow, narrow_rows, narrow32, narrow64, narrow_linear, narrow_taps=narrow_taps, narrow_fill=narrow_fill), False)
    if split_narrow:
        y = W._torchdot_split_narrow(xd, relu=relu, absmax=absmax)
    elif kernel is None:
        y = W._torchdot_split(xd, relu=relu, absmax=absmax)
    else:
        (get_op, flags) = kernel
        f64 = W.is_float64()
        y = torch.empty((W.shape[0], n), dtype=torch.float64 if f64 else torch.float32, device=xd.device)
        with torch.cuda.device(xd.device):
            if f64:
                get_op(xd.device).spmm_f64(xd.data_ptr(), n, n, y.data_ptr(), n, flags, _stream_ptr())
                if absmax is not None:               # (a float64 layer is never on a re-ordering kernel; the slot still feeds the NEXT layer's screen)
                    _capi.absmax(y.float().data_ptr(), W.shape[0], n, n, absmax.data_ptr(), _stream_ptr())
            else:
                get_op(xd.device).spmm(xd.data_ptr(), n, n, y.data_ptr(), n, flags, _stream_ptr(), absmax_ptr=None if absmax is None else absmax.data_ptr())
    return y if x.is_cuda else y.to(x.device)


NARROW_MAX = 8        # widest batch of the channel-lane conv-taps kernel (KN_FLAG_NARROW; KeyedModel.NARROW_MAX)
NARROW32_MAX = 32     # ... with narrow32=True (KN_FLAG_NARROW32: convtaps_narrow32_kernel, the matrix-core narrow kernel at NV = 16 | 32; KeyedModel.NARROW32_MAX)
NARROW64_MAX = 64     # ... with narrow64=True (KN_FLAG_NARROW64: beyond NARROW32_MAX columns convtaps_exact_pipe64_kernel; narrow64='mfma': the f32 tile kernel on 64-column tiles; KeyedModel.NARROW64_MAX)


def _narrow_args(n, narrow, narrow_rows, what='images', alone=False, narrow32=False, narrow64=False, narrow_linear=False, narrow_split=False, narrow_taps=False, narrow_fill=False):
    """The argument rule of the narrow forms, for a batch of `n`: `narrow_rows` only together with `narrow` (`alone`: a container's torchdot, which takes one
    keyword or the other), at most NARROW_MAX columns; `narrow32` only together with `narrow`, whose limit it lifts to NARROW32_MAX -- not that of `narrow_rows`
    (the row-lane kernel is an 8-column kernel); `narrow64` only together with `narrow` as well: it implies `narrow32` (at most NARROW32_MAX columns the call is exactly
    narrow32=True) and lifts the limit to NARROW64_MAX, where narrow='mfma' with narrow64=True is refused beyond NARROW32_MAX (True asks for the order-preserving form
    of that width); `narrow64='mfma'` only together with narrow='mfma': the matrix-core form of NARROW32_MAX + 1 .. NARROW64_MAX columns (KN_FLAG_NARROW64_MFMA), and at
    NARROW32_MAX columns and fewer exactly narrow='mfma', narrow32=True; `narrow_linear` only together with `narrow` (or `alone`), up to the limit the `narrow`
    keywords passed give -- NARROW_MAX, NARROW32_MAX with `narrow32`, NARROW64_MAX with `narrow64` -- and alone up to NARROW64_MAX, the kernel's own range;
    `narrow_split` only together with narrow='mfma' (`alone` or not: the route ends on the matrix-core narrow kernel), at the widths the other keywords allow -- it takes effect up
    to NARROW32_MAX columns and changes nothing beyond; `narrow_taps` only together with `narrow` (True or 'mfma'; `alone` or not: it modifies that keyword's channel-lane
    kernel), at the widths the other keywords allow -- it takes effect up to NARROW_MAX columns and changes nothing beyond; `narrow_fill` by the same rule -- it takes
    effect up to NARROW32_MAX columns.
    ValueError, or the normalised (mode, rows): mode False | True | 'mfma', rows a bool."""
    if narrow_split and narrow != 'mfma':
        raise ValueError('narrow_split=True is the split application of a filled-in conv layer on the matrix-core narrow kernel: pass narrow=\'mfma\' with it (got narrow=%r)' % (narrow,))
    if narrow_taps and not narrow:
        raise ValueError('narrow_taps=%r is the tap-resident form of the channel-lane conv kernel: pass narrow=True or narrow=\'mfma\' with it (got narrow=%r)' % (narrow_taps, narrow))
    if narrow_fill and not narrow:
        raise ValueError('narrow_fill=True is the tap-resident form of the channel-lane conv kernels for filled-in operators: pass narrow=True or narrow=\'mfma\' with it (got narrow=%r)' % (narrow,))
    if narrow64 == 'mfma' and narrow != 'mfma':
        raise ValueError('narrow64=\'mfma\' is the matrix-core form of %d .. %d %s: pass narrow=\'mfma\' with it (got narrow=%r)' % (NARROW32_MAX + 1, NARROW64_MAX, what, narrow))
    if narrow_rows and not narrow and not alone:
        raise ValueError('narrow_rows=True is a form of the narrow forward: pass narrow=True or narrow=\'mfma\' with it')
    if narrow_linear and not narrow and not alone:
        raise ValueError('narrow_linear=True is a form of the narrow forward: pass narrow=True or narrow=\'mfma\' with it')
    if narrow_linear and not narrow and n > NARROW64_MAX:
        raise ValueError('narrow_linear=True takes at most %d %s, got %d' % (NARROW64_MAX, what, n))
    if narrow32 and not narrow:
        raise ValueError('narrow32=True widens the narrow forward: pass narrow=True or narrow=\'mfma\' with it')
    if narrow64 and not narrow:
        raise ValueError('narrow64=True widens the narrow forward: pass narrow=True with it')
    if narrow_rows and n > NARROW_MAX:
        raise ValueError('narrow_rows=True takes at most %d %s, got %d' % (NARROW_MAX, what, n))
    limit = NARROW64_MAX if narrow64 else (NARROW32_MAX if narrow32 else NARROW_MAX)
    if narrow and n > limit:
        raise ValueError('narrow=%r%s takes at most %d %s, got %d' % (narrow, ', narrow64=True' if narrow64 else (', narrow32=True' if narrow32 else ''), limit, what, n))
    if narrow == 'mfma' and n > NARROW32_MAX and narrow64 != 'mfma':
        raise ValueError('narrow=\'mfma\', narrow64=True: there is no matrix-core form at %d .. %d %s (got %d); the padded forward is the matrix-core path there, '
                         'narrow=True the order-preserving one' % (NARROW32_MAX + 1, NARROW64_MAX, what, n))
    return (narrow if narrow == 'mfma' else bool(narrow), bool(narrow_rows))


class NarrowForm(collections.namedtuple('NarrowForm', 'mode rows narrow32 narrow64 tile64 linear')):
    """The five keywords narrow, narrow_rows, narrow32, narrow64, narrow_linear of one call, resolved once: what KeyedModel.forward_linear documents, as a value.
    `mode`: False (the wide forward) | True (the order-preserving conv kernels) | 'mfma' (the matrix-core narrow kernel where a layer's contract allows it);
    `narrow32`, `narrow64`: the width the keywords allow is lifted to NARROW32_MAX, to NARROW64_MAX (narrow64 implies narrow32); `tile64`: narrow64='mfma' at a
    width that takes the 64-column matrix-core tile; `rows`, `linear`: narrow_rows, narrow_linear.  Built by of() at the surfaces that take the keywords: once per
    call in KeyedModel, which hands the value down to _forward_once; there keywords() hands the keywords back to each KeyedLayer.forward, and that surface and
    KeyedLayer.kernel behind the operator's torchdot each build the value again from them (the keyword surfaces are what a layer and an operator are called by).
    `split`: the opt-in sixth keyword narrow_split=True (only with narrow='mfma': the narrow split route of a filled-in conv layer, KeyedModel.forward_linear).  The six fields
    above ARE the value of every call without it; a call with it gets the same six fields as a NarrowSplitForm, which equals no plain form and hands the keyword back.
    `taps`: the opt-in seventh keyword narrow_taps=True (only with `narrow`: KN_FLAG_NARROW_TAPS on the conv layers' channel-lane launches), carried the same way -- a
    NarrowTapsForm, or with narrow_split=True a NarrowSplitTapsForm; each kind equals its own kind only.
    narrow_taps='packed' (KN_MODIFIER_NARROW_TAPS32 next to KN_FLAG_NARROW_TAPS: the packed tap-resident kernel at NARROW_MAX + 1 .. NARROW32_MAX columns) is a kind of its
    own again, the `packed` twin of the kind narrow_taps=True gives (_packed_kind), with `taps` == 'packed'.
    narrow_taps='pairs' (KN_MODIFIER_NARROW_TAPS_PAIRS next to both: the channel-pair tap-resident kernel at 1 .. NARROW_MAX columns, 'packed' beyond) likewise: the
    `pairs` twin (_pairs_kind), with `taps` == 'pairs'.
    `fill`: the opt-in eighth keyword narrow_fill=True (only with `narrow`: KN_FLAG_NARROW_FILL on the same launches), carried the same way: the kind of the call without
    it has a `fill` twin (_fill_kind: NarrowFillForm, NarrowSplitFillForm, NarrowTapsFillForm, NarrowSplitTapsFillForm), which equals its own kind only."""
    __slots__ = ()
    split = False
    taps = False
    fill = False

    @classmethod
    @functools.lru_cache(maxsize=256)        # (asked per layer and launch, on the shortest forwards, for the same few keyword sets)
    def of(cls, n, narrow=False, narrow_rows=False, narrow32=False, narrow64=False, narrow_linear=False, what='images', alone=False, narrow_split=False, narrow_taps=False, narrow_fill=False):
        """The form of a batch of `n` under the keywords: _narrow_args refuses what the argument rule refuses (`what`, `alone`: its own).  n = None: no batch
        (KeyedLayer.kernel / launch) -- nothing is refused, a keyword without `narrow` means what the rules of kernel() make of it, and the tile is asked for."""
        mode = narrow if narrow == 'mfma' else bool(narrow)
        if n is not None:
            _narrow_args(n, narrow, narrow_rows, what, alone, narrow32=narrow32, narrow64=narrow64, narrow_linear=narrow_linear, narrow_split=narrow_split, narrow_taps=narrow_taps, narrow_fill=narrow_fill)
        (split, taps) = (bool(narrow_split and mode == 'mfma'), bool(narrow_taps and mode))
        kind = (NarrowSplitTapsForm if taps else NarrowSplitForm) if split else (NarrowTapsForm if taps else NarrowForm)
        if narrow_fill and mode:
            kind = _fill_kind[kind]
        if taps and narrow_taps == 'packed':
            kind = _packed_kind[kind]
        elif taps and narrow_taps == 'pairs':
            kind = _pairs_kind[kind]
        return kind(mode, bool(narrow_rows), bool(narrow32 or narrow64), bool(narrow64), mode == 'mfma' and narrow64 == 'mfma' and (n is None or n > NARROW32_MAX), bool(narrow_linear))

    def keywords(self):
        """The keywords of this form, normalised, as KeyedLayer.forward and the surfaces below it take them (narrow64: 'mfma' only where the tile is asked for;
        narrow_split, narrow_taps, narrow_fill: only where they were passed)."""
        kw = dict(narrow=self.mode, narrow_rows=self.rows, narrow32=self.narrow32, narrow64='mfma' if self.tile64 else self.narrow64, narrow_linear=self.linear)
        if self.split:
            kw['narrow_split'] = True
        if self.taps:
            kw['narrow_taps'] = self.taps         # True | 'packed' | 'pairs'
        if self.fill:
            kw['narrow_fill'] = True
        return kw


class _TypedNarrowForm(NarrowForm):
    """The forms of the calls that passed an opt-in keyword beyond the five: the same six fields, equal only to a form of their own kind."""
    __slots__ = ()

    def __eq__(self, other):
        return type(other) is type(self) and tuple.__eq__(self, other)

    def __ne__(self, other):
        return not self.__eq__(other)

    def __hash__(self):
        return hash((type(self), tuple(self)))


class NarrowSplitForm(_TypedNarrowForm):
    """A NarrowForm of a call that passed narrow_split=True (with narrow='mfma'): the same six fields, `split` True."""
    __slots__ = ()
    split = True


class NarrowTapsForm(_TypedNarrowForm):
    """A NarrowForm of a call that passed narrow_taps=True (with `narrow`): the same six fields, `taps` True."""
    __slots__ = ()
    taps = True


class NarrowSplitTapsForm(NarrowSplitForm):
    """... and of a call that passed both narrow_split=True and narrow_taps=True (with narrow='mfma'): a split form with `taps` True."""
    __slots__ = ()
    taps = True


def _fill_twin(kind, name):
    """The kind of the calls that passed narrow_fill=True next to the keywords of `kind`: the same fields, `split` and `taps` (a split kind stays a NarrowSplitForm),
    `fill` True, equal to its own kind only."""
    base = kind if kind is not NarrowForm else _TypedNarrowForm
    return type(name, (base,), dict(__slots__=(), fill=True, __doc__='%s of a call that also passed narrow_fill=True (with `narrow`): the same six fields, `fill` True.' % kind.__name__))


NarrowFillForm = _fill_twin(NarrowForm, 'NarrowFillForm')
NarrowSplitFillForm = _fill_twin(NarrowSplitForm, 'NarrowSplitFillForm')
NarrowTapsFillForm = _fill_twin(NarrowTapsForm, 'NarrowTapsFillForm')
NarrowSplitTapsFillForm = _fill_twin(NarrowSplitTapsForm, 'NarrowSplitTapsFillForm')
_fill_kind = {NarrowForm: NarrowFillForm, NarrowSplitForm: NarrowSplitFillForm, NarrowTapsForm: NarrowTapsFillForm, NarrowSplitTapsForm: NarrowSplitTapsFillForm}


def _packed_twin(kind, name):
    """The kind of the calls that passed narrow_taps='packed' where the calls of `kind` passed narrow_taps=True: the same fields, `split` and `fill`, `taps` the string
    'packed' (true where `taps` is tested, and what keywords() hands back), equal to its own kind only."""
    return type(name, (kind,), dict(__slots__=(), taps='packed', __doc__='%s of a call that passed narrow_taps=\'packed\' in place of narrow_taps=True: the same six fields, `taps` \'packed\'.' % kind.__name__))


NarrowPackedForm = _packed_twin(NarrowTapsForm, 'NarrowPackedForm')
NarrowSplitPackedForm = _packed_twin(NarrowSplitTapsForm, 'NarrowSplitPackedForm')
NarrowPackedFillForm = _packed_twin(NarrowTapsFillForm, 'NarrowPackedFillForm')
NarrowSplitPackedFillForm = _packed_twin(NarrowSplitTapsFillForm, 'NarrowSplitPackedFillForm')
_packed_kind = {NarrowTapsForm: NarrowPackedForm, NarrowSplitTapsForm: NarrowSplitPackedForm, NarrowTapsFillForm: NarrowPackedFillForm, NarrowSplitTapsFillForm: NarrowSplitPackedFillForm}


def _pairs_twin(kind, name):
    """The kind of the calls that passed narrow_taps='pairs' where the calls of `kind` passed narrow_taps=True: the same fields, `split` and `fill`, `taps` the string
    'pairs', equal to its own kind only."""
    return type(name, (kind,), dict(__slots__=(), taps='pairs', __doc__='%s of a call that passed narrow_taps=\'pairs\' in place of narrow_taps=True: the same six fields, `taps` \'pairs\'.' % kind.__name__))


NarrowPairsForm = _pairs_twin(NarrowTapsForm, 'NarrowPairsForm')
NarrowSplitPairsForm = _pairs_twin(NarrowSplitTapsForm, 'NarrowSplitPairsForm')
NarrowPairsFillForm = _pairs_twin(NarrowTapsFillForm, 'NarrowPairsFillForm')
NarrowSplitPairsFillForm = _pairs_twin(NarrowSplitTapsFillForm, 'NarrowSplitPairsFillForm')
_pairs_kind = {NarrowTapsForm: NarrowPairsForm, NarrowSplitTapsForm: NarrowSplitPairsForm, NarrowTapsFillForm: NarrowPairsFillForm, NarrowSplitTapsFillForm: NarrowSplitPairsFillForm}


# ------------------------------------------------------------------------------------------------------------------
class SparseMatrix(object):
    """scipy-sparse (or dense ndarray) operator applied by order-preserving CSR SpMM kernels (keynet/sparse.py:419-514)."""

    def __init__(self, A=None):
        assert A is None or is_scipy_sparse(A) or isinstance(A, np.ndarray), 'Invalid input - %s' % (str(type(A)))
        self.shape = A.shape if A is not None else (0, 0)
        self._matrix = A
        self.dtype = A.dtype if A is not None else None
        self.ndim = 2
        self._op = None
        self._op_dense = None

    def __repr__(self):
        return str('<keynet_amd.SparseMatrix: H=%d, W=%d, backend=hip>' % (self.shape[0], self.shape[1]))

    def __getstate__(self):
        d = dict(self.__dict__)
        d['_op'] = None   # device handles do not pickle; rebuilt lazily
        d['_op_dense'] = None
        if '_op_split' in d:
            d['_op_split'] = None
        return d

    def __add__(self, other):
        assert isinstance(other, SparseMatrix) and self.shape == other.shape, 'Invalid input'
        self._matrix = self._matrix + other._matrix
        self._op = None
        return self

    # -- device side
    def _device_op(self, device=None):
        def make():
            M = self._matrix
            if isinstance(M, np.ndarray):
                M = scipy.sparse.csr_matrix((np.asarray(M, dtype=np.float32).ravel(), np.tile(np.arange(M.shape[1]), M.shape[0]),
                                             np.arange(0, M.size + 1, M.shape[1])), shape=M.shape)
            (ip, ix, dt) = _stored_order_csr(M)
            return _capi.Operator.csr(self.shape, ip, ix, dt)
        return _on_device(self, '_op', make, device)

    def narrow_capable(self):
        """Does this container's device operator have the channel-lane form for 1 .. 8 batch columns (a conv-taps handle: KN_FLAG_NARROW)?"""
        return False

    def rows_capable(self):
        """Does this container's device operator have the row-lane form for 1 .. 8 batch columns (a float32 CSR handle: KN_FLAG_NARROW_ROWS)?"""
        return not self.is_float64()

    def is_float64(self):
        """Does scipy compute this operator's product with float32 activations in float64 (a float64 -- or integer -- scipy matrix)?
        Dense ndarray operators go through BLAS in the reference (no defined order) and stay float32 here."""
        M = getattr(self, '_matrix', None)
        return M is not None and is_scipy_sparse(M) and _compute_dtype(M.dtype) == np.float64

    DENSE_MIN_ELEMENTS = 1 << 20

    def _dense_device_op(self, device=None):
        """kn_dense_create handle for a (nearly) dense operator such as a keyed nn.Linear, or None when not eligible."""
        if getattr(self, '_matrix', None) is None:
            return None          # tiled containers have no single host matrix: never dense-eligible

        def make():
            M = self._matrix
            (r, c) = self.shape
            ok = (M is not None and not self.is_float64() and r * c >= self.DENSE_MIN_ELEMENTS and (c - 1) % 256 == 0 and
                  (M.nnz if is_scipy_sparse(M) else M.size) >= 0.5 * r * c)
            if ok:
                D = np.asarray(M.todense() if is_scipy_sparse(M) else M, dtype=np.float32)
                if bool(np.all(D[-1, :-1] == 0)):
                    return _capi.Operator.dense(D)
            return False
        return _on_device(self, '_op_dense', make, device) or None

    def torchdot(self, x_torch, relu=False, exact=True, absmax=None, narrow_rows=False, narrow_linear=False):
        """W . x for x of shape [W.shape[1], N]: the hot path (keynet/sparse.py:488-492).  exact=True (default): bit-exact
        with scipy (order-preserving CSR kernels).  exact=False: a large dense operator (keyed nn.Linear) may run as a
        split-K f32-MFMA GEMM instead (within 1e-5; used by the tiled key-nets whose conv layers are on MFMA anyway).
        `absmax`: one-element device f32 tensor raised to max |W . x| (kn_spmm_screen).
        `narrow_rows` (N <= NARROW_MAX, ValueError beyond): the stored-order product on the row-lane kernel (KN_FLAG_NARROW_ROWS), the same bits; an operator
        on its dense handle (exact=False) or in float64 is what it is without the keyword.
        `narrow_linear` (N <= NARROW64_MAX, ValueError beyond): the big pattern groups of a keyed Linear on the LDS value-stream kernel (KN_FLAG_NARROW_LINEAR), the
        same bits, under the same conditions; an operator without such a group is what it is without the keyword."""
        return _run_torchdot(self, x_torch, relu=relu, exact=exact, absmax=absmax, narrow_rows=narrow_rows, narrow_linear=narrow_linear)

    def dot(self, x_numpy):
        assert isinstance(x_numpy, np.ndarray)
        return self.torchdot(torch.as_tensor(np.asarray(x_numpy))).cpu().numpy()

    def max_abs_rowsum(self):
        """max_i sum_j |W_ij| (host, float64): the operator-side factor of the float-key error bound (KeyedLayer._calibrate)."""
        M = self._matrix
        if is_scipy_sparse(M):
            return float(abs(M).sum(axis=1).max()) if M.nnz else 0.0
        return float(np.abs(np.asarray(M, dtype=np.float64)).sum(axis=1).max()) if M.size else 0.0

    # -- structure (host)
    def new(self):
        return SparseMatrix()

    def clone(self):
        return copy.deepcopy(self)

    def from_torch_dense(self, A):
        return SparseMatrix(A.detach().numpy())

    def from_scipy_sparse(self, A):
        assert is_scipy_sparse(A)
        return SparseMatrix(A)

    def matmul(self, A):
        """In-place sparse x sparse product on the host (keynet/sparse.py:472-480); not on the forward path."""
        assert isinstance(A, SparseMatrix) or is_scipy_sparse(A)
        self._matrix = self._matrix.dot(A._matrix if isinstance(A, SparseMatrix) else A)
        self.shape = self._matrix.shape
        (self._op, self._op_dense) = (None, None)
        return self

    def nnz(self):
        return self._matrix.nnz if is_scipy_sparse(self._matrix) else self._matrix.size

    def transpose(self):
        self._matrix = self._matrix.transpose()
        self.shape = self._matrix.shape
        (self._op, self._op_dense) = (None, None)
        return self

    def tocoo(self):
        return self._matrix.tocoo() if is_scipy_sparse(self._matrix) else scipy.sparse.coo_matrix(self._matrix)

    def tocsr(self):
        self._matrix = self._matrix.tocsr()
        self._op = None
        return self

    def tocsc(self):
        self._matrix = self._matrix.tocsc()
        self._op = None
        return self

    def from_torch_conv2d(self, inshape, w, b, stride):
        return SparseMatrix(sparse_toeplitz_conv2d(inshape, w.detach().numpy(), bias=b.detach().numpy(), stride=stride))


# ------------------------------------------------------------------------------------------------------------------
class FactoredSparseMatrix(SparseMatrix):
    """An UNTILED keyed conv layer (keynet/layer.py:24-41: a scipy CSR, `SparseMatrix`) whose stored CSR has been PROVEN, on the host, to be the
    ascending-column expansion of a factored conv operator (taps x spatial entries, keynet_amd/direct.py) with the exact zeros dropped.  That is
    what the keying SpGEMMs leave for identity / channel-replicated permutation keys on both sides -- every conv layer of PermutationKeynet
    AllConvNet but the first.  scipy's product in stored order is then, entry for entry, the factored operator's order-preserving product
    (KN_FLAG_EXACT: channel outer, the pixel's slots by ascending input pixel inner, bias last), so the device holds 0.3 MB of taps + the slot lists + a
    stored-column table instead of the CSR's hundreds of MB and runs the matrix-pipe grouped kernel from that table (narrow batches: the conv pipeline);
    kn_convtaps_drop_zero_entries covers the dropped zeros.  Everything on the
    host (`_matrix`, nnz(), tocoo(), pickling, the neutral file format) is the plain CSR container's."""

    def __init__(self, A, factored):
        super(FactoredSparseMatrix, self).__init__(A)
        self._factored = factored

    def __repr__(self):
        return str('<keynet_amd.SparseMatrix: H=%d, W=%d, backend=hip (factored on the device)>' % (self.shape[0], self.shape[1]))

    def _device_op(self, device=None):
        def make():
            t = self._factored._taps
            return _capi.Operator.convtaps(self._factored._inshape, self._factored._outshape, t['taps'], t['ent_out'], t['ent_in'], t['ent_tap'], t['ent_coef'],
                                           t['lastcol']).drop_zero_entries()
        return _on_device(self, '_op', make, device)

    def _dense_device_op(self, device=None):
        return None

    def narrow_capable(self):
        return True

    def rows_capable(self):
        return False                     # (a conv-taps handle on the device)

    def torchdot(self, x_torch, relu=False, exact=True, absmax=None, narrow=False, narrow32=False, narrow64=False, narrow_taps=False, narrow_fill=False):
        """SparseMatrix.torchdot; `narrow` (True or 'mfma': the same here, the operator is under the bit-exact contract): at most NARROW_MAX columns on the channel-lane kernel of the factored device form (KN_FLAG_NARROW) -- the
        same bits as without it (the order-preserving product, which IS scipy's on the stored CSR); `narrow32` (with `narrow`): at most NARROW32_MAX columns (KN_FLAG_NARROW32);
        `narrow64` (with `narrow`): at most NARROW64_MAX (KN_FLAG_NARROW64); `narrow_taps` (with `narrow`): the tap-resident kernel at up to NARROW_MAX columns (KN_FLAG_NARROW_TAPS); `narrow_fill` (with `narrow`): the filled-in operators' tap-resident kernel at up to NARROW32_MAX columns (KN_FLAG_NARROW_FILL)."""
        return _run_torchdot(self, x_torch, relu=relu, exact=exact, absmax=absmax, narrow=narrow, narrow32=narrow32, narrow64=narrow64, narrow_taps=narrow_taps, narrow_fill=narrow_fill)

    @staticmethod
    def proven(M, factored, max_zero_fraction=0.01):
        """Is the stored CSR `M` (scipy) exactly -- indptr, indices AND values, in stored order -- the canonical expansion of `factored` with its
        zero-valued entries removed?  Also refuses operators with many exact zeros (a pruned filter): the device re-checks every such entry."""
        try:
            return FactoredSparseMatrix._proven(M, factored, max_zero_fraction)
        except Exception:                # any surprise in a crafted / damaged description: the plain CSR container it is (the comments promise a fallback)
            return False

    @staticmethod
    def _proven(M, factored, max_zero_fraction):
        t = factored._taps
        if t is None or M.format != 'csr' or tuple(M.shape) != tuple(factored.shape) or M.dtype != np.float32:
            return False
        taps = t['taps']
        live = taps[np.any(taps.reshape(taps.shape[0], -1) != 0, axis=1)]
        if live.size and float(np.count_nonzero(live == 0)) > max_zero_fraction * live.size:
            return False
        E = factored.rows_csr()
        keep = E.data != 0
        if M.nnz != int(np.count_nonzero(keep)):
            return False
        counts = np.diff(np.concatenate(([0], np.cumsum(keep, dtype=np.int64)))[E.indptr.astype(np.int64)])      # kept entries per row (empty rows, trailing ones included: 0)
        (ip, ix, dt) = _stored_order_csr(M)
        return bool(np.array_equal(np.concatenate(([0], np.cumsum(counts))).astype(np.int64), ip.astype(np.int64)) and
                    np.array_equal(E.indices[keep].astype(np.int32), ix) and np.array_equal(E.data[keep].view(np.uint32), dt.view(np.uint32)))


def _structure_preserving(vals64):
    """The reference stores tile values as ((v + off) - off) with off = |min v| + 1 computed in float64, then casts to
    float32 (keynet/sparse.py:562-566, 582): reproduced so tile contents match bit for bit."""
    off = np.abs(np.min(vals64)) + 1.0
    return ((vals64 + off) - off).astype(np.float32)


class TiledMatrix(SparseMatrix):
    """Sparse matrix stored as de-duplicated h x w tiles + a block list (keynet/sparse.py:517-653).

    The tile dictionary is storage compression; on the device the operator is expanded ONCE to canonical CSR (the
    reference re-expands it on every torchdot call, keynet/sparse.py:610) because per non-zero the 8 bytes of (col,val)
    are negligible next to the n_vecs*4-byte activation row it gathers."""

    def __init__(self, T, tileshape):
        assert is_scipy_sparse(T), 'input must be a scipy sparse matrix'
        assert isinstance(tileshape, tuple) and len(tileshape) == 2 and tileshape[0] > 0 and tileshape[1] > 0, 'tileshape must be tuple (tileheight, tilewidth) > 0'
        self._tileshape = tileshape
        self.dtype = T.dtype
        self.shape = (T.shape[0], T.shape[1])
        self.ndim = 2
        self._op = None
        (self._blocks, self._tiles) = _tile_sparse(T, tileshape)

    def __repr__(self):
        return str('<keynet_amd.TiledMatrix: H=%d, W=%d, tileshape=%s, tiles=%d>' % (self.shape[0], self.shape[1], str(self.tileshape()), len(self.tiles())))

    def __iter__(self):
        for (i, j, k) in self._blocks:
            yield (i, j, k)

    def tileshape(self):
        return self._tileshape

    def tiles(self):
        return self._tiles

    def blocks(self):
        return list(self.__iter__())

    def _tile_arrays(self):
        tiles = [t.tocoo() for t in self._tiles]
        ptr = np.cumsum([0] + [t.nnz for t in tiles]).astype(np.int64)
        cat = (lambda L, dt: np.concatenate(L).astype(dt) if len(L) else np.zeros(0, dt))
        return (ptr, cat([t.row for t in tiles], np.int32), cat([t.col for t in tiles], np.int32), cat([t.data for t in tiles], np.float32))

    def _device_op(self, device=None):
        def make():
            (ptr, tr, tc, tv) = self._tile_arrays()
            return _capi.Operator.tiled(self.shape, np.array(list(self), dtype=np.int64).reshape(-1, 3), ptr, tr, tc, tv)
        return _on_device(self, '_op', make, device)

    def torchdot(self, x, relu=False, exact=True, absmax=None, narrow_rows=False, narrow_linear=False):
        """[cols, N] -> [rows, N] (keynet/sparse.py:603-612); always the order-preserving path (bit-exact).  `narrow_rows` (N <= NARROW_MAX, ValueError beyond):
        on the row-lane kernel (KN_FLAG_NARROW_ROWS), the same bits.  `narrow_linear` (N <= NARROW64_MAX, ValueError beyond): big pattern groups of the expanded
        operator on the LDS value-stream kernel (KN_FLAG_NARROW_LINEAR), the same bits; without such a group the call is what it is without the keyword."""
        return _run_torchdot(self, x, relu=relu, exact=True, absmax=absmax, narrow_rows=narrow_rows, narrow_linear=narrow_linear)

    def dot(self, x):
        assert isinstance(x, np.ndarray)
        return self.torchdot(torch.as_tensor(x)).cpu().numpy()

    def max_abs_rowsum(self):
        M = self.tosparse('csr')
        return float(abs(M).sum(axis=1).max()) if M.nnz else 0.0

    def copy(self, blocks, tiles):
        (self._blocks, self._tiles, self._op) = (blocks, tiles, None)
        return self

    def transpose(self):
        self._blocks = [(j, i, k) for (i, j, k) in self._blocks] if self._blocks is not None else self._blocks
        self._tiles = [t.transpose() for t in self._tiles]
        self._tileshape = (self._tileshape[1], self._tileshape[0])
        self.shape = (self.shape[1], self.shape[0])
        self._op = None
        return self

    def tosparse(self, format='coo'):
        """Expanded operator as scipy csr/coo/csc (keynet/sparse.py:621-641); host side, small matrices / tests."""
        tiles = [t.tocoo() for t in self._tiles]
        (R, C, V) = ([], [], [])
        for (i, j, k) in self.__iter__():
            R.append(i + tiles[k].row.astype(np.int64))
            C.append(j + tiles[k].col.astype(np.int64))
            V.append(tiles[k].data)
        cat = (lambda L, dt: np.concatenate(L) if len(L) else np.zeros(0, dt))
        return _from_coo(format, cat(V, np.float32), cat(R, np.int64), cat(C, np.int64), self.shape)

    def tocsr(self):
        return self.tosparse(format='csr')

    def tocoo(self):
        return self.tosparse(format='coo')

    def nnz(self):
        return sum([t.nnz for t in self._tiles])


def _from_coo(format, vals, rows, cols, shape):
    if format == 'csr':
        return scipy.sparse.csr_matrix((vals, (rows, cols)), shape=shape)
    if format == 'coo':
        return scipy.sparse.coo_matrix((vals, (rows, cols)), shape=shape)
    if format == 'csc':
        return scipy.sparse.csc_matrix((vals, (rows, cols)), shape=shape)
    raise ValueError('Invalid format "%s" - must be ["coo", "csr", "csc"]' % format)


def _tile_sparse(T, tileshape):
    """Vectorised restatement of the TiledMatrix tiler (keynet/sparse.py:543-571).

    Returns (blocks, tiles): blocks = [(row0, col0, k)] row-major; tiles[k] = scipy COO (float32) of the k-th distinct
    tile.  Tile ids follow first occurrence in COO order; entries inside a tile are (row, col)-sorted (the reference's
    float64 -> float32 astype canonicalises the COO); two blocks share a tile iff their (i,j,v) sets and block shapes
    are identical (the reference hashes str(sorted(ijv))+str(shape))."""
    T = T.tocoo()
    (h, w) = tileshape
    (H, W) = T.shape
    if T.nnz == 0:
        return ([], [])
    (r, c) = (np.asarray(T.row, dtype=np.int64), np.asarray(T.col, dtype=np.int64))
    v = np.asarray(T.data, dtype=np.float64)
    (bi, bj) = (r // h, c // w)
    nbj = (W + w - 1) // w
    key = bi * nbj + bj
    order = np.argsort(key, kind='stable')
    ks = key[order]
    starts = np.flatnonzero(np.concatenate(([True], ks[1:] != ks[:-1])))
    ends = np.concatenate((starts[1:], [len(ks)]))
    first_seen = order[starts]                     # original COO index of each block's first entry
    tiles = []
    blocks = []
    seen = {}
    for b in np.argsort(first_seen, kind='stable'):
        idx = order[starts[b]:ends[b]]
        (kbi, kbj) = (int(ks[starts[b]] // nbj), int(ks[starts[b]] % nbj))
        (ii, jj, vv) = (r[idx] - kbi * h, c[idx] - kbj * w, v[idx])
        bshape = (h if (kbi * h + h) <= H else (H - kbi * h), w if (kbj * w + w) <= W else (W - kbj * w))
        s = np.lexsort((jj, ii))
        sig = (ii[s].tobytes(), jj[s].tobytes(), vv[s].tobytes(), bshape)
        k = seen.get(sig)
        if k is None:
            k = len(tiles)
            seen[sig] = k
            tiles.append(scipy.sparse.coo_matrix((_structure_preserving(vv)[s], (ii[s], jj[s])), shape=bshape))
        blocks.append((kbi * h, kbj * w, k))
    blocks.sort(key=lambda x: (x[0], x[1]))
    return (blocks, tiles)


class DiagonalTiledMatrix(TiledMatrix):
    """One block repeated down the main diagonal; where the block does not divide the matrix, the last (partial) diagonal
    position holds the matching corner of an identity instead (keynet/sparse.py:657-687)."""

    def __init__(self, B, shape):
        assert B.ndim == 2, 'Invalid block, must be 2D'
        assert isinstance(shape, tuple) and len(shape) == 2, 'invalid shape'
        (H, W) = shape
        if B.shape[0] > H or B.shape[1] > W:
            B = B.tocsr()[0:H, 0:W]                            # an oversized block is clipped to the matrix
        if not scipy.sparse.issparse(B):
            B = _dense_block_as_sparse(B)
        (h, w) = B.shape
        (self._tileshape, self.shape, self.dtype, self.ndim, self._op, self._blocks) = ((h, w), shape, B.dtype, 2, None, None)
        self._tiles = [B.astype(np.float32)]
        if H % h or W % w:
            self._tiles.append(scipy.sparse.eye(max(h, w)).tocsr()[0:H % h, 0:W % w].astype(np.float32))

    def __iter__(self):
        """(row0, col0, tile id) along the diagonal: tile 0 wherever the block fits strictly inside, else the last tile."""
        ((H, W), (h, w)) = (self.shape, self._tileshape)
        n = min(len(range(0, H, h)), len(range(0, W, w)))
        (i, j) = (np.arange(n) * h, np.arange(n) * w)
        k = np.where((i + h < H) & (j + w < W), 0, len(self._tiles) - 1)
        return iter([(int(a), int(b), int(c)) for (a, b, c) in zip(i, j, k)])


def _dense_block_as_sparse(B):
    """Dense block -> CSR keeping EVERY entry stored, zeros included (shift by |min| + 1 before the conversion, shift the stored
    values back afterwards): the tile then has the full h x w structure, as the reference's 'sparsity preserving' round trip."""
    off = np.abs(np.min(B)) + 1.0
    S = scipy.sparse.coo_matrix(B + off)
    S.data -= off
    return S.tocsr()


class Conv2dTiledMatrix(TiledMatrix):
    """Keyed conv operator as spatial blocks x dense channel matrices (keynet/sparse.py:690-835).

    _blocks = [(i, j, k)] over the channel-(0,0) plane (+ bias blocks at column Cin*Hin*Win);
    _tiles  = {(it, jt, k): float32[Cout, Cin]} (+ {(it, 0, k): [[b]]} for bias tiles).
    On the device the channel matrices are de-duplicated into `taps` and the forward is an implicit GEMM per output
    pixel on f32 MFMA (csrc/kn_conv.hip); `exact=True` in torchdot selects the order-preserving CSR path instead."""

    def __init__(self, T, inshape, outshape, tileshape, bias, sanitycheck=True):
        (Cin, Hin, Win) = inshape
        (Cout, Hout, Wout) = outshape
        self._inshape = inshape
        self._outshape = outshape
        self._tileshape = tileshape
        self.shape = T.shape
        self.dtype = T.dtype
        self.ndim = 2
        self._op = None
        self._taps = None
        assert tileshape[0] <= T.shape[0] and tileshape[1] <= T.shape[1]
        if bias:
            assert T.shape[0] == np.prod(outshape) + 1 and T.shape[1] == np.prod(inshape) + 1
            assert (self.shape[0] - 1) % tileshape[0] == 0 and (self.shape[1] - 1) % tileshape[1] == 0
        else:
            assert T.shape[0] == np.prod(outshape) and T.shape[1] == np.prod(inshape)
            assert self.shape[0] % tileshape[0] == 0 and self.shape[1] % tileshape[1] == 0
        T = T.tocsr()
        (HoWo, HiWi) = (Hout * Wout, Hin * Win)
        T_00 = T[0:HoWo, 0:HiWi]
        if sanitycheck and Cout > 1 and Cin > 1:
            T_10 = T[HoWo:2 * HoWo, 0:HiWi]
            T_01 = T[0:HoWo, HiWi:2 * HiWi]
            assert ((T_00 != 0) != (T_10 != 0)).nnz == 0 and ((T_00 != 0) != (T_01 != 0)).nnz == 0, 'channel-inconsistent sparsity'
        (blocks, _) = _tile_sparse(T_00, tileshape)
        T_lastcol = None
        if bias:
            T_lastcol = T[:, -1]
            T = T[0:-1, 0:-1]
        self._tiles = _conv_tiler(T.tocoo(), blocks, inshape, outshape, tileshape)
        self._blocks = list(blocks)
        if bias:
            (bblocks, btiles) = _tile_sparse(T_lastcol, (tileshape[0], 1))
            k_offset = len(self._tiles)
            for (kt, t) in enumerate(btiles):
                for (i, j, v) in zip(t.row, t.col, t.data):
                    self._tiles[(int(i), int(j), int(k_offset + kt))] = np.array(v).reshape(1, 1).astype(np.float32)
            self._blocks += [(i, Cin * HiWi, k_offset + k) for (i, j, k) in bblocks]
        self._blocks = sorted(self._blocks, key=lambda x: (x[0], x[1]))

    @classmethod
    def fromtaps(cls, inshape, outshape, taps, ent_out, ent_in, ent_tap, ent_coef=None, lastcol=None, tileshape=None):
        """Direct construction in factored form (never materialises the Toeplitz matrix): see kn_convtaps_create."""
        self = cls.__new__(cls)
        (self._inshape, self._outshape, self._tileshape) = (tuple(inshape), tuple(outshape), tileshape)
        has_last = lastcol is not None
        self.shape = (int(np.prod(outshape)) + (1 if has_last else 0), int(np.prod(inshape)) + (1 if has_last else 0))
        self.dtype = np.float32
        self.ndim = 2
        self._op = None
        (self._blocks, self._tiles) = (None, None)
        self._taps = dict(taps=np.ascontiguousarray(taps, dtype=np.float32), ent_out=np.asarray(ent_out, dtype=np.int32), ent_in=np.asarray(ent_in, dtype=np.int32),
                          ent_tap=np.asarray(ent_tap, dtype=np.int32), ent_coef=None if ent_coef is None else np.asarray(ent_coef, dtype=np.float32),
                          lastcol=None if lastcol is None else np.asarray(lastcol, dtype=np.float32))
        return self

    def __repr__(self):
        return str('<keynet_amd.Conv2dTiledMatrix: H=%d, W=%d, tileshape=%s, backend=hip>' % (self.shape[0], self.shape[1], str(self._tileshape)))

    def __iter__(self):
        assert self._blocks is not None, 'operator was built in factored form (fromtaps): no block list'
        for (i, j, k) in self._blocks:
            yield (i, j, k)

    def _golden_arrays(self):
        """(blocks, tile_keys, tile_isbias, tile_chan, tile_bias) in the layout of kn_conv2dtiled_create."""
        (Cout, Cin) = (self._outshape[0], self._inshape[0])
        lastcol_at = Cin * self._inshape[1] * self._inshape[2]
        biask = set(int(b[2]) for b in self._blocks if b[1] == lastcol_at and self.shape[1] == lastcol_at + 1)
        keys = list(self._tiles.keys())
        isbias = np.array([k[2] in biask for k in keys], dtype=np.uint8)
        chan = [np.asarray(self._tiles[k], dtype=np.float32) for (k, b) in zip(keys, isbias) if not b]
        bvals = [float(np.asarray(self._tiles[k]).reshape(())) for (k, b) in zip(keys, isbias) if b]
        return (np.array(self._blocks, dtype=np.int64).reshape(-1, 3), np.array(keys, dtype=np.int64).reshape(-1, 3), isbias,
                np.stack(chan) if len(chan) else np.zeros((0, Cout, Cin), np.float32), np.array(bvals, dtype=np.float32))

    def _device_op(self, device=None):
        def make():
            if self._taps is not None:
                t = self._taps
                return _capi.Operator.convtaps(self._inshape, self._outshape, t['taps'], t['ent_out'], t['ent_in'], t['ent_tap'], t['ent_coef'], t['lastcol'])
            (bl, tk, ib, ch, bs) = self._golden_arrays()
            return _capi.Operator.conv2dtiled(self.shape, self._inshape, self._outshape, bl, tk, ib, ch, bs)
        return _on_device(self, '_op', make, device)

    def narrow_capable(self):
        return True

    def rows_capable(self):
        return False                     # (a conv-taps handle on the device)

    def torchdot(self, x, relu=False, exact=False, absmax=None, narrow=False, narrow32=False, narrow64=False, narrow_split=False, narrow_taps=False, narrow_fill=False):
        """[cols, N] -> [rows, N].  `narrow_split` (only with narrow='mfma', ValueError otherwise): under exact='split', at most NARROW32_MAX columns, a filled-in operator runs
        the narrow split route (_torchdot_split_narrow) where narrow_split_route() offers it; everywhere else the call is what it is without the keyword.  `narrow_taps` (only with `narrow`): KN_FLAG_NARROW_TAPS wherever the call carries KN_FLAG_NARROW -- the tap-resident kernel at up to NARROW_MAX columns, the same bits.  `narrow_fill` (only with `narrow`): KN_FLAG_NARROW_FILL wherever the call carries KN_FLAG_NARROW -- a filled-in operator's tap-resident kernel at up to NARROW32_MAX columns, the same bits.  exact=False: f32 MFMA path (f32-input matrix instructions, exact f32 products); exact=True: the
        reference's accumulation order and rounding (order-preserving kernel on the factored operator); exact='split': a filled-in factored
        operator applied as spatial mixing per tap, then channel mixing (see _split_ops: another association of the sum, tolerance contract only); exact='bf16x3': f32 products
        emulated on the bf16 matrix pipe (three-way exact split, six of nine cross products, f32 accumulate: KN_FLAG_BF16X3) where the
        operator and batch qualify, else the f32 MFMA path.  `narrow`, `narrow32`, `narrow64`: the narrow forms of KeyedModel.forward_linear on this one operator, N within
        their limits (ValueError beyond) -- narrow=True the order-preserving narrow kernels whatever `exact` says (the bits of exact=True); narrow='mfma' the matrix-core
        narrow kernel when `exact` is False / 'bf16x3' / 'split' and the operator is eligible (no (pixel, tap) pair with more than two slots), else exactly narrow=True;
        narrow64='mfma' (with narrow='mfma') beyond NARROW32_MAX columns under False / 'bf16x3' the f32 product on 64-column tiles (per column the bits of the plain
        matrix-core call on the batch zero-padded to 128 columns), else narrow64=True.  The flag word is KeyedLayer.kernel's."""
        assert not isinstance(exact, str) or exact in ('bf16x3', 'split', 'wino') or (narrow and exact == 'auto'), "exact must be True, False, 'bf16x3', 'split' or 'wino'"
        return _run_torchdot(self, x, relu=relu, exact=exact, absmax=absmax, narrow=narrow, narrow32=narrow32, narrow64=narrow64, narrow_split=narrow_split, narrow_taps=narrow_taps, narrow_fill=narrow_fill)

    # ---- the 1-D Winograd F(2,3) form of a keyed 3 x 3 conv (tolerance contract only) ----------------------------------------------------
    # exact='wino' is exact=False with KN_MODIFIER_WINO (include/keynet_hip.h): two neighbouring outputs of a 3-tap image row from 4 products instead of 6 -- two thirds
    # of the matrix instructions, paid for with two memory-bound transforms over blocks twice the activations' size.  Whether an operator HAS the form is the
    # library's answer (its entry table must be a 3 x 3 convolution of an image of even width under some pixel permutation; the plan names the launches); whether
    # the form is worth OFFERING is the cost rule here, kept apart from that like split_capable.  Another association of the f32 sum: KeyedLayer._calibrate measures it
    # against the order-preserving kernel and accepts it at a quarter of the gate.  Inf - Inf inside the input transform is NaN where the plain product is Inf:
    # non-finite activations must not reach the form, and they do not -- the screen of the float-key contract sends such a layer to the stored order first.
    WINO_MIN_CHANNELS = 128     # measured (profiles/wino_layer_ab.txt, VGG-16 shapes at 128 and 256 columns, A-B-A-B in one process): every shape from conv2_2 (128 -> 128
                                # channels: 1.04 - 1.08x) to conv5_x (1.35 - 1.41x) won in every repetition; operators with a 64-channel side were not measured and are not offered

    def wino_offered(self, n_vecs):
        """The cost rule of exact='wino': whole 128-column tiles on an operator whose smaller channel count reaches WINO_MIN_CHANNELS."""
        return n_vecs > 0 and n_vecs % 128 == 0 and min(self._inshape[0], self._outshape[0]) >= self.WINO_MIN_CHANNELS

    def wino_planned(self, n_vecs, relu, device):
        """Does a plain call of n_vecs columns with KN_MODIFIER_WINO take the form on this operator (the library's eligibility, read off the plan)?"""
        with torch.cuda.device(device):
            return 'wino_in_kernel' in self._device_op(device).plan(n_vecs, _capi.KN_MODIFIER_WINO | (_capi.KN_FLAG_RELU if relu else 0))

    def __getstate__(self):
        d = super(Conv2dTiledMatrix, self).__getstate__()
        d.pop('_narrow_split_ws', None)           # device workspaces and plan answers of the narrow split route: rebuilt at first use
        d.pop('_narrow_split_plans', None)
        return d

    # ---- the SPLIT application of a filled-in operator (tolerance contract only) -----------------------------------------------------
    # A factored keyed conv is  sum_t F_t (x) K_t  with F_t the Cout x Cin matrix of tap t and K_t = a_out S_t a_in^-1 the HoWo x HiWi spatial
    # matrix of its entries (keynet_amd/direct.py).  The fused operator the reference stores costs  slots x Cin x Cout  multiply-adds per output
    # pixel and batch column; under a key whose inverse is dense inside its blocks (doubly-stochastic keys: 500 - 5 400 slots per pixel instead
    # of 9) that is 60x the un-keyed layer.  The same product in two steps --
    #     Z_t[ci] = K_t X[ci]                  (spatial mixing: one CSR of all taps' entries, applied to every input channel's plane)
    #     Y       = sum_t F_t Z_t              (channel mixing: an ordinary ntaps-slot conv-taps operator on Z, matrix cores, wave-uniform loaders)
    # -- costs  slots x Cin + ntaps x Cin x Cout.  It holds nothing the fused factored form does not hold (the same taps, the same entries), but it
    # is another association of the sum: NOT the reference's arithmetic, so it is a candidate of the float-key contract only (KeyedLayer._calibrate
    # measures it against the order-preserving kernel like the matrix-core kernel; layers that fail run in the reference's order as before).
    SPLIT_MIN_FILL = 2.0        # slots per (output pixel, tap) from which the split application is offered
    SPLIT_Z_BYTES = 32 << 30    # the intermediate Z is produced in column windows of at most this size (VGG-16 conv1_2 at 256 images: 29.6 GB in one window; 74-column windows
                                # under an 8 GB cap ran ragged tiles on the generic loader: 314 ms against 49 ms per 64 images)

    def fill_factor(self):
        """Entries per (output pixel, tap) of a factored operator: 1 for identity / permutation keys, 55 - 600 under doubly-stochastic keys."""
        t = self._taps
        if t is None or len(t['taps']) == 0:
            return 0.0
        return len(t['ent_out']) / float(len(t['taps']) * self._outshape[1] * self._outshape[2])

    def split_capable(self, n_vecs=None):
        """Is the split application worth offering to this operator (at this batch width)?  A filled-in factored operator whose split form is estimated at
        less than half the fused matrix-core launch: fused = entries x Cin x Cout multiply-adds at ~100 TFLOP/s (filled-in pixels run the slot-group / generic
        loaders); split = entries x Cin on the CSR kernels (~10 T MAC/s) + ntaps x HoWo x Cin x Cout on the matrix cores (~120 TFLOP/s) + the intermediate
        written and read once (~3 TB/s).  Givens-rotation keys (2 - 4 entries per pixel and tap) stay fused by this rule: their intermediate costs what the
        saved multiply-adds give back."""
        if self._taps is None or self.fill_factor() < self.SPLIT_MIN_FILL:
            return False
        if n_vecs is None:
            return True
        (Cin, Cout, HoWo) = (self._inshape[0], self._outshape[0], self._outshape[1] * self._outshape[2])
        (ent, nt, n) = (float(len(self._taps['ent_out'])), float(len(self._taps['taps'])), float(n_vecs))
        fused = 2.0 * ent * Cin * Cout * n / 100e12
        split = 2.0 * ent * Cin * n / 10e12 + 2.0 * nt * HoWo * Cin * Cout * n / 120e12 + 2.0 * (4.0 * Cin * nt * HoWo * n) / 3e12
        return split < 0.5 * fused

    def _split_arrays(self):
        """Host side of the split form: (K, second) with K the scipy CSR [ntaps * HoWo, HiWi] of all taps' entries (row t * HoWo + out, column in, value coef)
        and `second` the kwargs of the channel-mixing operator Conv2dTiledMatrix.fromtaps(**second) on Z [Cin, ntaps, HoWo]."""
        t = self._taps
        (Cin, Hin, Win) = self._inshape
        (Cout, Hout, Wout) = self._outshape
        (HoWo, HiWi, nt) = (Hout * Wout, Hin * Win, len(t['taps']))
        coef = t['ent_coef'] if t['ent_coef'] is not None else np.ones(len(t['ent_out']), np.float32)
        K = scipy.sparse.csr_matrix((coef.astype(np.float32), (t['ent_tap'].astype(np.int64) * HoWo + t['ent_out'], t['ent_in'].astype(np.int64))), shape=(nt * HoWo, HiWi))
        K.sort_indices()
        assert K.nnz == len(coef), 'an (output pixel, input pixel, tap) triple appears twice'
        eo = np.tile(np.arange(HoWo, dtype=np.int32), nt)
        et = np.repeat(np.arange(nt, dtype=np.int32), HoWo)
        second = dict(inshape=(Cin, nt, HoWo), outshape=self._outshape, taps=t['taps'], ent_out=eo, ent_in=(et.astype(np.int64) * HoWo + eo).astype(np.int32), ent_tap=et,
                      ent_coef=None, lastcol=t['lastcol'])
        return (K, second)

    def _split_ops(self, device=None):
        """(spatial CSR [ntaps * HoWo, HiWi], channel-mixing conv-taps operator on Z [Cin, ntaps, HoWo] -> [Cout, Hout, Wout]) resident on `device`."""
        def make():
            (K, f) = self._split_arrays()
            opK = _capi.Operator.csr(K.shape, K.indptr, K.indices, K.data)
            op2 = _capi.Operator.convtaps(f['inshape'], f['outshape'], f['taps'], f['ent_out'], f['ent_in'], f['ent_tap'], f['ent_coef'], f['lastcol'])
            return (opK, op2)
        return _on_device(self, '_op_split', make, device)

    def _torchdot_split(self, xd, relu=False, absmax=None):
        """xd: the device block (_device_block) [cols, N] -> [rows, N] on its device."""
        (Cin, Hin, Win) = self._inshape
        (HoWo, HiWi, nt) = (self._outshape[1] * self._outshape[2], Hin * Win, len(self._taps['taps']))
        has_last = self._taps['lastcol'] is not None
        n = int(xd.shape[1])
        zrows = Cin * nt * HoWo + (1 if has_last else 0)
        cap = self.SPLIT_Z_BYTES
        with torch.cuda.device(xd.device):
            (free_b, _) = torch.cuda.mem_get_info()
            free_b += torch.cuda.memory_reserved() - torch.cuda.memory_allocated()       # what the caching allocator holds but does not use is available too
        cap = min(cap, max(free_b - 4 * self.shape[0] * n, 0) // 2)                      # the intermediate takes at most half of what is left beside the output block
        win = max(1, min(n, int(cap // (4 * zrows))))
        if win < n and win >= 64:
            win -= win % (128 if win >= 128 else 64)      # whole tiles of the matrix-core kernel per window
        y = torch.empty((self.shape[0], n), dtype=torch.float32, device=xd.device)
        flags = _capi.KN_FLAG_RELU if relu else 0
        with torch.cuda.device(xd.device):
            (opK, op2) = self._split_ops(xd.device)
            st = _stream_ptr()
            z = torch.empty((zrows, min(win, n)), dtype=torch.float32, device=xd.device)
            for c0 in range(0, n, win):
                w = min(win, n - c0)
                ldz = int(z.shape[1])
                # the spatial CSR on every input channel's plane (rows ci * HiWi ..) -> Z rows ci * ntaps * HoWo ..: ONE launch over all planes (kn_spmm_planes, round 6:
                # conv1_2 .. conv5_3 of the doubly-stochastic VGG-16 used to issue 64 .. 512 launches of 37 us each per layer and window), else plane by plane
                if not opK.spmm_planes(xd.data_ptr() + 4 * c0, n, HiWi * n, Cin, w, z.data_ptr(), ldz, nt * HoWo * ldz, _capi.KN_FLAG_EXACT, st):
                    for ci in range(Cin):
                        opK.spmm(xd.data_ptr() + 4 * (ci * HiWi * n + c0), n, w, z.data_ptr() + 4 * ci * nt * HoWo * ldz, ldz, _capi.KN_FLAG_EXACT, st)
                if has_last:
                    z[-1, :w].copy_(xd[-1, c0:c0 + w])
                op2.spmm(z.data_ptr(), ldz, w, y.data_ptr() + 4 * c0, n, flags, st, absmax_ptr=None if absmax is None else absmax.data_ptr())
        return y

    # ---- the NARROW split route (narrow='mfma', narrow_split=True; 1 .. NARROW32_MAX columns) ---------------------------------------------------
    # kn_spmm_planes puts the input-channel planes on grid dimension y and the batch columns on lanes: at one image one lane in 64 works.  For a narrow batch the
    # planes ARE the batch of the spatial matrix: on Xt[in][(ci, b)] it is an ordinary CSR product with N = Cin x n = 64 .. 16 384 columns, the width the CSR kernels
    # are built for.  Four steps:  X -> Xt (kn_planes_to_columns);  Z' = K Xt (ONE kn_spmm, stored order);  Z' -> Z (kn_columns_to_planes; the homogeneous row copied
    # as on the wide route);  Y = op2 Z on the matrix-core narrow kernel (op2 has one slot per (pixel, tap): eligible, where the fused filled-in operator is not).
    # Z of an image is bit-equal to the wide route's (the same stored-order sums, whatever the width), and an image's Y does not depend on the launch width (the narrow
    # matrix-core kernel's property), so ONE measurement on 8 columns covers every width (KeyedLayer.narrow_split_mode).
    NARROW_SPLIT_Z_BYTES = 4 << 30      # Z' is produced in windows of whole images of at most this size (VGG-16 conv1_2 at 32 images: 3.7 GB, one window); a window is the three
                                        # first steps on a column range of X -- other columns, the same sums: windows change no bit
    NARROW_SPLIT_MIN_GAIN = 1.3         # the route is offered where the estimate of the fused channel-lane launch is at least this many times the route's (the margin every narrow regime was held to)
    # the constants of narrow_split_capable's estimate (seconds; DESIGN section 5 says which are measured):
    # (set from profiles/r14_narrow_split.txt, each on the slow side of what was measured so that the estimate of the route errs high and that of the fused launch low)
    NARROW_SPLIT_STEP_RATE = 1.2e10     # wavefront steps per second of the channel-lane kernel in its summed-stored-values form (measured 1.15 - 1.35e10 at one image; the 9-slot form: 2.1e10)
    NARROW_SPLIT_CSR_RATE = 2.0e12      # multiply-adds per second of the CSR kernels at Cin x n columns (measured 2.0e12 on conv1_2 .. 8.1e12 on conv4_2)
    NARROW_SPLIT_BYTE_RATE = 3.0e12     # bytes per second of the two permutes and of Xt / Z' through the CSR kernel (the permutes measured 4.3 - 5.3e12 on the large layers, 0.6 - 3e12 on the small)
    NARROW_SPLIT_MMA_RATE = 2.0e13      # multiply-adds per second of the matrix-core narrow kernel on the 9-slot operator (measured 0.8 - 3.2e13)
    NARROW_SPLIT_FIXED = 6.0e-5         # three more launches and the narrow kernel's floor (reasoning: its smallest measured launch is 33 us, a launch about 9 us)

    def narrow_split_capable(self, n_vecs=None):
        """Is the narrow split route worth offering to this operator at `n_vecs` columns?  split_capable()'s question for the narrow forward: the fused launch it replaces is the
        channel-lane kernel in its summed-stored-values form -- entries x Cin x ceil(Cout / 64) wavefront steps per block of up to 16 columns -- and the route costs
        entries x Cin x n multiply-adds on the CSR kernels, the activations moved five times (X read, Xt written and read, Z' written and read, Z written: two permutes around
        one product) and the 9-slot narrow launch."""
        if not self.split_capable():
            return False
        if n_vecs is None:
            return True
        if not 0 < n_vecs <= NARROW32_MAX:
            return False
        (Cin, Cout, HoWo, HiWi) = (self._inshape[0], self._outshape[0], self._outshape[1] * self._outshape[2], self._inshape[1] * self._inshape[2])
        (ent, nt, n) = (float(len(self._taps['ent_out'])), float(len(self._taps['taps'])), float(n_vecs))
        fused = ent * Cin * -(-Cout // 64) * -(-n_vecs // 16) / self.NARROW_SPLIT_STEP_RATE
        split = (ent * Cin * n / self.NARROW_SPLIT_CSR_RATE + 4.0 * Cin * n * (3.0 * HiWi + 3.0 * nt * HoWo) / self.NARROW_SPLIT_BYTE_RATE +
                 nt * HoWo * Cin * Cout * n / self.NARROW_SPLIT_MMA_RATE + self.NARROW_SPLIT_FIXED)
        return fused >= self.NARROW_SPLIT_MIN_GAIN * split

    def narrow_split_route(self, n_vecs, relu=False, device=None):
        """Does a narrow_split call of `n_vecs` columns take the route here?  A split form (split_capable()), the cost rule (narrow_split_capable), and the channel-mixing
        operator's narrow launch at this width on the matrix-core narrow kernel (kn_spmm_plan names it; asked once per (device, width, relu))."""
        if not 0 < n_vecs <= NARROW32_MAX or not self.narrow_split_capable(n_vecs):
            return False
        idx = torch.cuda.current_device() if (device is None or device.index is None) else device.index
        plans = self.__dict__.setdefault('_narrow_split_plans', {})
        key = (idx, int(n_vecs), bool(relu))
        if key not in plans:
            with torch.cuda.device(idx):
                plans[key] = 'convtaps_narrow_mfma_kernel' in self._split_ops(device)[1].plan(n_vecs, self._narrow_split_flags(n_vecs, relu))
        return plans[key]

    @staticmethod
    def _narrow_split_flags(n_vecs, relu):
        return _capi.KN_FLAG_NARROW_MFMA | (_capi.KN_FLAG_NARROW32 if n_vecs > NARROW_MAX else 0) | (_capi.KN_FLAG_RELU if relu else 0)

    def _narrow_split_window(self, n_vecs):
        """Images per window of the route's first three steps: whole images, Z' within NARROW_SPLIT_Z_BYTES."""
        (Cin, nt, HoWo) = (self._inshape[0], len(self._taps['taps']), self._outshape[1] * self._outshape[2])
        return max(1, min(int(n_vecs), int(self.NARROW_SPLIT_Z_BYTES // (4 * nt * HoWo * Cin))))

    def _narrow_split_workspace(self, device, n_vecs):
        """(Xt, Z', Z) flat float32 device buffers of the route, per (device, width class 8 | 32, window): allocated at the first call of a class (an eager one: KeyedModel.capture
        runs it before capturing) and reused by every later one on the stream order of the calls; nothing asks the allocator or the device per forward.  Dropped by
        release_narrow_split_workspace() (KeyedModel.release_workspace) and by pickling."""
        (Cin, Hin, Win) = self._inshape
        (HoWo, HiWi, nt) = (self._outshape[1] * self._outshape[2], Hin * Win, len(self._taps['taps']))
        wc = NARROW_MAX if n_vecs <= NARROW_MAX else NARROW32_MAX
        win = self._narrow_split_window(wc)
        ws = self.__dict__.setdefault('_narrow_split_ws', {})
        key = (torch.cuda.current_device() if device.index is None else device.index, wc, win)
        if key not in ws:
            zrows = Cin * nt * HoWo + (1 if self._taps['lastcol'] is not None else 0)
            ws[key] = tuple(torch.empty(k, dtype=torch.float32, device=device) for k in (HiWi * Cin * win, nt * HoWo * Cin * win, zrows * wc))
        return ws[key]

    def release_narrow_split_workspace(self):
        self.__dict__.pop('_narrow_split_ws', None)

    def _torchdot_split_narrow(self, xd, relu=False, absmax=None):
        """xd: the device block (_device_block) [cols, n], n <= NARROW32_MAX -> [rows, n] on its device: the narrow split route (above)."""
        (Cin, Hin, Win) = self._inshape
        (HoWo, HiWi, nt) = (self._outshape[1] * self._outshape[2], Hin * Win, len(self._taps['taps']))
        has_last = self._taps['lastcol'] is not None
        n = int(xd.shape[1])
        assert 0 < n <= NARROW32_MAX, 'the narrow split route takes 1 .. %d columns, got %d' % (NARROW32_MAX, n)
        y = torch.empty((self.shape[0], n), dtype=torch.float32, device=xd.device)
        with torch.cuda.device(xd.device):
            (opK, op2) = self._split_ops(xd.device)
            (xt, zc, z) = self._narrow_split_workspace(xd.device, n)
            win = self._narrow_split_window(NARROW_MAX if n <= NARROW_MAX else NARROW32_MAX)
            st = _stream_ptr()
            for c0 in range(0, n, win):
                w = min(win, n - c0)
                N = Cin * w
                _capi.planes_to_columns(xd.data_ptr() + 4 * c0, HiWi * n, n, Cin, HiWi, w, xt.data_ptr(), N, st)
                opK.spmm(xt.data_ptr(), N, N, zc.data_ptr(), N, _capi.KN_FLAG_EXACT | (_capi.KN_FLAG_NARROW_ROWS if N <= NARROW_MAX else 0), st)
                _capi.columns_to_planes(zc.data_ptr(), N, Cin, nt * HoWo, w, z.data_ptr() + 4 * c0, nt * HoWo * n, n, st)
            zv = z[:(Cin * nt * HoWo + (1 if has_last else 0)) * n].view(-1, n)
            if has_last:
                zv[-1].copy_(xd[-1])
            op2.spmm(z.data_ptr(), n, n, y.data_ptr(), n, self._narrow_split_flags(n, relu), st, absmax_ptr=None if absmax is None else absmax.data_ptr())
        return y

    def _expand_taps_host(self, pixels=None, channels=None):
        """Canonical CSR of a factored operator -- or of its output rows (co, o) for o in `pixels` only, numbered
        co * len(pixels) + position of o -- on the host: the reference's expansion rule (keynet/sparse.py:802-812; kn_export_csr
        does the same on the C side; `channels` further restricts the rows to the first `channels` output channels).  Built
        directly in CSR order, one block copy + one table gather per output channel: row (co, o) holds,
        for ci ascending, the pixel's slots by ascending input pixel, then the bias entry -- exactly the column-sorted row scipy's
        csr_matrix((v,(r,c))) would produce, without ever holding a COO copy (conv5_1 of VGG-16: 420 M entries)."""
        t = self._taps
        (Cout, Hout, Wout) = self._outshape
        (Cin, Hin, Win) = self._inshape
        (HoWo, HiWi) = (Hout * Wout, Hin * Win)
        pixels = np.arange(HoWo, dtype=np.int64) if pixels is None else np.asarray(pixels, dtype=np.int64)
        npx = len(pixels)
        pos = -np.ones(HoWo, dtype=np.int64)
        pos[pixels] = np.arange(npx)
        sel = np.flatnonzero(pos[t['ent_out']] >= 0)
        order = sel[np.lexsort((t['ent_in'][sel], pos[t['ent_out'][sel]]))]          # by (pixel position, input pixel), stable
        (eo, ei, et) = (pos[t['ent_out'][order]], t['ent_in'][order].astype(np.int64), t['ent_tap'][order])
        coef = None if t['ent_coef'] is None else t['ent_coef'][order]
        if len(eo) > 1 and np.any((eo[1:] == eo[:-1]) & (ei[1:] == ei[:-1])):
            # several taps on one (output, input) pixel pair: ONE stored entry per channel pair, the float32 sum of its terms fl(coef * tap) in entry order.  The selected
            # pixels' pairs become the taps of an equivalent duplicate-free operator (one [Cout, Cin] matrix per pair, summed one term position at a time), which the
            # block-copy route below expands -- a per-entry COO route would hold 3 x 8 bytes per stored value and sort them all.
            first = np.ones(len(eo), dtype=bool)
            first[1:] = (eo[1:] != eo[:-1]) | (ei[1:] != ei[:-1])
            seg = np.cumsum(first) - 1
            rank = np.arange(len(eo)) - np.flatnonzero(first)[seg]
            tp = t['taps']
            def term(idx):
                v = tp[et[idx]]
                if coef is None:
                    return v
                cf = coef[idx][:, None, None]
                return np.where(cf == 1.0, v, cf * v).astype(np.float32)
            V = term(np.flatnonzero(first)).astype(np.float32, copy=True)
            for k in range(1, int(rank.max()) + 1):
                idx = np.flatnonzero(rank == k)
                V[seg[idx]] = (V[seg[idx]] + term(idx)).astype(np.float32)
            W2 = Conv2dTiledMatrix.fromtaps(self._inshape, self._outshape, V, pixels[eo[first]], ei[first], np.arange(len(V), dtype=np.int32), None, t['lastcol'])
            return W2._expand_taps_host(pixels, channels)
        Cout = Cout if channels is None else int(channels)                                  # several taps on one (out, in) pair: scipy sums them
        ns = np.bincount(eo, minlength=npx)                                           # slots per selected pixel
        first = np.concatenate(([0], np.cumsum(ns)))[:-1]
        has_last = t['lastcol'] is not None
        rows_n = Cout * npx + (1 if (has_last and npx == HoWo and channels is None) else 0)
        counts = np.tile(ns * Cin, Cout)
        if has_last:
            lastv = t['lastcol'][(np.arange(Cout)[:, None] * HoWo + pixels[None, :]).ravel()]
            counts = counts + (lastv != 0)
        if rows_n > Cout * npx:
            counts = np.concatenate((counts, [1 if t['lastcol'][-1] != 0 else 0]))
        indptr = np.zeros(rows_n + 1, dtype=np.int64)
        np.cumsum(counts, out=indptr[1:])
        total = int(indptr[-1])
        idt = np.int32 if max(total, self.shape[1]) < 2 ** 31 - 1 else np.int64
        indices = np.empty(total, dtype=idt)
        data = np.empty(total, dtype=np.float32)
        taps = t['taps']
        ntaps = taps.shape[0]
        # The Cout rows of a pixel share one column sequence, and the rows of one output channel are contiguous in the result:
        # the channel's block is ONE copy of a precomputed column image and ONE gather from that channel's small [ntaps, Cin]
        # value table.  The image is rebuilt only when the bias column's zero pattern differs between channels.
        cached_mask = None
        for co in range(Cout):
            mask = (lastv[co * npx:(co + 1) * npx] != 0) if has_last else np.zeros(npx, dtype=bool)
            if cached_mask is None or not np.array_equal(mask, cached_mask):
                cached_mask = mask
                cnt = ns * Cin + mask
                loc = np.concatenate(([0], np.cumsum(cnt)))
                col_img = np.empty(int(loc[-1]), dtype=idt)
                src_img = np.zeros(int(loc[-1]), dtype=np.int64)                       # index into taps[:, co, :].ravel()
                ent_img = np.zeros(int(loc[-1]), dtype=np.int64)                       # entry id (for the coefficients)
                for k in np.unique(ns):
                    if k == 0:
                        continue
                    P = np.flatnonzero(ns == k)
                    g = first[P][:, None] + np.arange(k)[None, :]                      # [P, k] entry ids, input pixels ascending
                    dest = loc[P][:, None] + np.arange(Cin * k)[None, :]
                    col_img[dest] = ((np.arange(Cin) * HiWi)[None, :, None] + ei[g][:, None, :]).reshape(len(P), Cin * k)
                    src_img[dest] = (et[g].astype(np.int64)[:, None, :] * Cin + np.arange(Cin)[None, :, None]).reshape(len(P), Cin * k)
                    ent_img[dest] = np.broadcast_to(g[:, None, :], (len(P), Cin, k)).reshape(len(P), Cin * k)
                bias_at = loc[1:][mask] - 1
                col_img[bias_at] = self.shape[1] - 1
            (lo, hi) = (int(indptr[co * npx]), int(indptr[(co + 1) * npx]))
            indices[lo:hi] = col_img
            v = taps[:, co, :].ravel()[src_img]
            if coef is not None:
                cf = coef[ent_img]
                v = np.where(cf == 1.0, v, cf * v)
            if has_last:
                v[bias_at] = lastv[co * npx:(co + 1) * npx][mask]
            data[lo:hi] = v
        if rows_n > Cout * npx and t['lastcol'][-1] != 0:
            indices[-1] = self.shape[1] - 1
            data[-1] = t['lastcol'][-1]
        return scipy.sparse.csr_matrix((data, indices, indptr.astype(idt)), shape=(rows_n, self.shape[1]))

    def rows_csr(self, pixels=None, channels=None):
        """Canonical CSR of the output rows (co, o), o in `pixels` (channel-major: row = co * len(pixels) + index of o), of a
        factored operator: the reference's expansion rule (keynet/sparse.py:802-812) restricted to those rows.  Host side;
        lets a CPU checker or a CPU baseline work on a slice of an operator whose full CSR would be tens of GB.  With every
        pixel selected this is the whole operator incl. its homogeneous row."""
        assert self._taps is not None, 'rows_csr needs the factored form (fromtaps / direct keying)'
        return self._expand_taps_host(pixels, channels)

    def max_abs_rowsum(self):
        """max over output rows (co, o) of sum |W| along the row, from the factored form without expanding it: for row (co, o) it is
        sum over the pixel's entries of |coef| * sum_ci |taps[tap][co][ci]|  (+ |last column|) -- one [HoWo x ntaps] sparse product."""
        if self._taps is None:
            M = self.tosparse('csr')
            return float(abs(M).sum(axis=1).max()) if M.nnz else 0.0
        t = self._taps
        (Cout, Hout, Wout) = self._outshape
        HoWo = Hout * Wout
        tap_abs = np.abs(t['taps'].astype(np.float64)).sum(axis=2)                     # [ntaps, Cout]
        coef = np.ones(len(t['ent_out'])) if t['ent_coef'] is None else np.abs(t['ent_coef'].astype(np.float64))
        S = scipy.sparse.csr_matrix((coef, (t['ent_out'].astype(np.int64), t['ent_tap'].astype(np.int64))), shape=(HoWo, tap_abs.shape[0]))
        rs = S.dot(tap_abs)                                                            # [HoWo, Cout]
        if t['lastcol'] is not None:
            rs = rs + np.abs(t['lastcol'][:Cout * HoWo].astype(np.float64)).reshape(Cout, HoWo).T
        return float(rs.max()) if rs.size else 0.0

    def nnz(self):
        """Stored parameters: sum of tile sizes (keynet/sparse.py:778) -- or, for a factored operator, taps + entries +
        last column (what is actually stored)."""
        if self._tiles is None:
            t = self._taps
            return int(t['taps'].size + len(t['ent_out']) + (np.count_nonzero(t['lastcol']) if t['lastcol'] is not None else 0))
        return sum([v.size for v in self._tiles.values()])

    def transpose(self):
        raise NotImplementedError('transpose of a Conv2dTiledMatrix is not on the forward path')

    def tosparse(self, format='coo'):
        """Expansion rule of keynet/sparse.py:802-812, vectorised."""
        if self._tiles is None:
            return self._expand_taps_host().asformat(format)
        (Cout, Hout, Wout) = self._outshape
        (Cin, Hin, Win) = self._inshape
        bykey = {}
        for ((it, jt, k), m) in self._tiles.items():
            bykey.setdefault(k, []).append((it, jt, m))
        (R, C, V) = ([], [], [])
        for (i, j, k) in self._blocks:
            for (it, jt, m) in bykey.get(k, []):
                (ic, jc) = np.meshgrid(np.arange(m.shape[0]), np.arange(m.shape[1]), indexing='ij')
                R.append((i + it + ic * Hout * Wout).ravel())
                C.append((j + jt + jc * Hin * Win).ravel())
                V.append(np.asarray(m, dtype=np.float32).ravel())
        return _from_coo(format, np.concatenate(V), np.concatenate(R), np.concatenate(C), self.shape)


def _conv_tiler(T, blocks, inshape, outshape, tileshape):
    """Vectorised restatement of Conv2dTiledMatrix.__tiler__ (keynet/sparse.py:692-717): returns the ordered dict
    {(it, jt, k): float32[Cout, Cin]}; where several blocks share a tile id the LAST entry in COO order wins."""
    (Cin, Hin, Win) = inshape
    (Cout, Hout, Wout) = outshape
    (h, w) = tileshape
    (HoWo, HiWi) = (Hout * Wout, Hin * Win)
    tiles = {}
    loc = {}
    for (ib, jb, kt) in blocks:
        loc[(ib, jb)] = kt
        tiles[(0, 0, kt)] = np.zeros((Cout, Cin), dtype=np.float32)
    if T.nnz == 0:
        return tiles
    (i, j, v) = (np.asarray(T.row, dtype=np.int64), np.asarray(T.col, dtype=np.int64), np.asarray(T.data, dtype=np.float32))
    (ip, jp) = (i % HoWo, j % HiWi)
    (ib, jb) = (h * (ip // h), w * (jp // w))
    nbj = HiWi // w + 1
    lut = {}
    bkeys = ib // h * nbj + jb // w
    for ((bi_, bj_), kt) in loc.items():
        lut[bi_ // h * nbj + bj_ // w] = kt
    (ub, inv) = np.unique(bkeys, return_inverse=True)
    kt_of = np.array([lut.get(int(b), -1) for b in ub], dtype=np.int64)[inv]
    keep = kt_of >= 0
    (i, j, v, ip, jp, ib, jb, kt_of) = (i[keep], j[keep], v[keep], ip[keep], jp[keep], ib[keep], jb[keep], kt_of[keep])
    (it, jt, ic, jc) = (ip - ib, jp - jb, i // HoWo, j // HiWi)
    tkey = (kt_of * h + it) * w + jt                      # (it, jt, kt) flattened
    (utk, first_idx, tinv) = np.unique(tkey, return_index=True, return_inverse=True)
    for u in np.argsort(first_idx, kind='stable'):          # dict insertion order = first appearance in COO order
        k3 = (int(utk[u] // w % h), int(utk[u] % w), int(utk[u] // (w * h)))
        if k3 not in tiles:
            tiles[k3] = np.zeros((Cout, Cin), dtype=np.float32)
    # assign; later entries overwrite earlier ones (numpy fancy assignment keeps the last for repeated indices)
    stack = np.zeros((len(utk), Cout, Cin), dtype=np.float32)
    stack[tinv, ic, jc] = v
    for (u, tk) in enumerate(utk):
        k3 = (int(tk // w % h), int(tk % w), int(tk // (w * h)))
        tiles[k3] = stack[u]
    return tiles


# ------------------------------------------------------------------------------------------------------------------
# Build-time constructors (host, offline)
def sparse_toeplitz_conv2d(inshape, f, bias=None, as_correlation=True, stride=1, format='csr'):
    """Explicit sparse matrix of a 'same'-padded, odd, square conv layer acting on the flattened CxUxV image, with the
    bias column and homogeneous row when `bias` is given: conv2d(img, f) == W.dot(img.flatten()).

    Restates keynet/sparse.py:122-203 without the per-entry Python loop.  Rows are (cout, u/stride, v/stride), columns
    (cin, u+p, v+q); taps falling outside the image are omitted.  Values are fl32(fl32(w + off) - off) with
    off = |min w| + 1 exactly as the reference's sparsity-preserving round trip leaves them (SURVEY 8c iv)."""
    assert len(inshape) == 3 and f.ndim == 4
    assert f.shape[1] == inshape[0] and f.shape[2] == f.shape[3] and f.shape[2] % 2 == 1
    assert as_correlation, 'only the correlation form is on the keyed path'
    (C, U, V) = inshape
    (M, _, P, Q) = f.shape
    f = np.asarray(f, dtype=np.float32)
    (Us, Vs) = (U // stride, V // stride)
    (ku, kv) = np.meshgrid(np.arange(Us), np.arange(Vs), indexing='ij')
    (u, v) = (np.arange(0, U, stride)[ku], np.arange(0, V, stride)[kv])
    (R, Cc, D) = ([], [], [])
    (cin, cout) = np.meshgrid(np.arange(C), np.arange(M), indexing='ij')
    for (i, p) in enumerate(range(-((P - 1) // 2), ((P - 1) // 2) + 1)):
        for (j, q) in enumerate(range(-((Q - 1) // 2), ((Q - 1) // 2) + 1)):
            ok = ((u + p) >= 0) & ((u + p) < U) & ((v + q) >= 0) & ((v + q) < V)
            (opix, ipix) = ((ku * Vs + kv)[ok], ((u + p) * V + (v + q))[ok])
            R.append((cout.reshape(1, -1) * (Us * Vs) + opix.reshape(-1, 1)).ravel())
            Cc.append((cin.reshape(1, -1) * (U * V) + ipix.reshape(-1, 1)).ravel())
            D.append(np.broadcast_to(f[cout, cin, i, j].reshape(1, -1), (len(opix), C * M)).ravel())
    (rows, cols, data) = (np.concatenate(R), np.concatenate(Cc), np.concatenate(D).astype(np.float32))
    off = np.float32(np.abs(np.min(data)) + np.float32(1.0))
    data = (data + off) - off
    A = scipy.sparse.coo_matrix((data, (rows, cols)), shape=(M * Us * Vs, C * U * V))
    if bias is not None:
        bias = np.asarray(bias, dtype=np.float32)
        assert bias.ndim == 1 and bias.shape[0] == M
        offb = np.float32(np.abs(np.min(bias)) + np.float32(1.0))
        bcol = ((np.repeat(bias, Us * Vs) + offb) - offb).astype(np.float32)
        lastcol = scipy.sparse.coo_matrix((bcol, (np.arange(M * Us * Vs), np.zeros(M * Us * Vs, dtype=np.int64))), shape=(A.shape[0], 1))
        lastrow = scipy.sparse.coo_matrix(([1], ([0], [A.shape[1]])), shape=(1, A.shape[1] + 1), dtype=np.float32)
        A = scipy.sparse.vstack((scipy.sparse.hstack((A, lastcol)), lastrow))
    return A.tocsr() if format == 'csr' else A


def sparse_toeplitz_avgpool2d(inshape, filtershape, stride):
    """Average pooling as a conv with a (1/k^2)-filled diagonal filter and a zero bias (keynet/sparse.py:206-212):
    k x k window, `stride`, zero padding (k-1)/2 counted in the mean -- independent of the source module's padding."""
    (outchannel, inchannel, k, _) = filtershape
    F = np.zeros(filtershape, dtype=np.float32)
    F[np.arange(outchannel), np.arange(outchannel), :, :] = 1.0 / (k * k)
    return sparse_toeplitz_conv2d(inshape, F, bias=np.zeros(outchannel, dtype=np.float32), stride=stride)


def sparse_affine_to_linear(A, bias=None, dtype=np.float32):
    """The homogeneous form [[A, b], [0, 1]] of x -> A x + b as one sparse matrix (keynet/sparse.py:87-96); b = 0 when no bias."""
    assert is_scipy_sparse(A)
    (m, n) = A.shape
    if bias is not None:
        assert bias.shape[0] == m and bias.shape[1] == 1
    b = scipy.sparse.coo_matrix(bias) if bias is not None else scipy.sparse.coo_matrix((m, 1), dtype=dtype)
    one = scipy.sparse.coo_matrix(([1], ([0], [n])), shape=(1, n + 1), dtype=dtype)
    return scipy.sparse.vstack((scipy.sparse.hstack((A, b)), one))


def sparse_identity_matrix(n, dtype=np.float32):
    return scipy.sparse.eye(n, dtype=dtype)


def sparse_permutation_matrix(n, dtype=np.float32, withinverse=False):
    """Random n x n permutation matrix, row r holding its one in column perm[r]; ONE np.random.permutation(n) draw from numpy's
    global RNG (keynet/sparse.py:280-285).  The inverse of a permutation matrix is its transpose."""
    perm = np.random.permutation(n)
    P = scipy.sparse.csr_matrix((np.ones(n, dtype=dtype), perm, np.arange(n + 1)), shape=(n, n))
    return (P, P.transpose()) if withinverse else P
