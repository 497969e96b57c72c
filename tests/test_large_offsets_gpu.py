"""Every kernel behind the C ABI on activation blocks at and beyond 2^31 elements (include/keynet_hip.h, kn_spmm: "what a caller may pass").

Harness.  Two flat f32 device buffers of 2^31 + 2^27 elements each (9.1 GB), one for X and one for Y, are allocated once for the module and released at teardown;
with the few-MB operands of a case the module holds AT MOST 20 GB live at any time (the fixture skips the module when less than 24 GB are free).  A case views a
buffer as [rows_or_cols, LD] and keeps its data in the LAST columns of every row (window start LD - n_vecs, both multiples of 4: the vector-width dispatch conditions
hold as for a compact block), so every offset a kernel forms is the largest its block allows.  Before a call the X buffer is NaN outside the window (a wrapped read
surfaces as NaN) and the Y buffer is the sentinel -7.  After a call: (1) the Y window equals the CPU oracle (oracle.csr_matvecs on the operator's canonical CSR),
bit for bit, NaN positions included -- kernels that run under the float-key tolerance (matrix-core conv, small-K, bf16x3, dense) are held to the gate their existing
parity test uses instead; (2) the Y window equals the same call on compact blocks (ldx = ldy = n_vecs) bit for bit -- for a tolerance kernel only where the compact call
runs the same kernel (equal plan strings), since two loaders of the matrix-core kernel promise the same value only to rounding; (3) with the window overwritten by the
sentinel the WHOLE Y buffer is the sentinel (min == max == -7 on the device: nothing was stored anywhere else).  Every case asserts through kn_spmm_plan which kernel
the call runs: the fast kernel below a launcher guard, another one (never the fast one) at and above it.

Guards (section A; `L` = last qualifying ldx, `F` = first non-qualifying, both multiples of 4):
  csr_group_pipe_kernel          cols * ldx < 2^31                          test_grouped_csr_pipeline_guard          -> csr_group_kernel
  convtaps_exact_pipe_kernel     (Cin HiWi + 1) * ldx < 2^31, 4 and 2 columns per lane   test_conv_pipeline_guard    -> convtaps_exact_kernel
  convtaps_mfma_kernel           sptr: 4 ((1024 / NB) HiWi ldx + NB) < 2^31; fast: KC HiWi ldx < 2^31 (HiWi ldx < 2^31 is implied by it); generic beyond
                                 test_matrix_core_conv_loader_guards (128 x 128 tiles: three loaders, four cases; 64 x 256 tiles: the two guards coincide, two cases)
  convtaps_exact_fill_kernel     4 ldx < 2^24 (HiWi = 64) and 4 HiWi ldx < 2^32 (HiWi = 400 and 784)   test_filled_in_kernel_guards   -> convtaps_exact_kernel
                                 forms: 32 channels x one tile, 64 x one, 64 x two; 32 x two at the largest block that fits the buffer.  HiWi < 2^24 needs a
                                 16-million-pixel image and is NOT exercised.
  convtaps_narrow_kernel         (Cin HiWi + 1) * ldx + 8 < 2^31 at 1, 3 and 8 columns; beyond it kn_spmm returns KN_ERR_UNSUPPORTED and leaves Y untouched
                                 test_narrow_kernel_guard.  The Python containers (torchdot / forward_linear with narrow=True) always hand the library a COMPACT copy
                                 of their operand (ldx = n_vecs <= 8), so a strided view whose rows lie 2^21 elements apart runs the narrow kernel to the same bits.
  small-K pair                   the table's `cols < INT32_MAX - 1` is a condition on the OPERATOR (checked at create) and no block can straddle it; the kernels form
                                 row * ldx in 64 bits and take any ldx: both sides of cols * ldx = 2^31 must name them (test_small_k_kernels).

Kernels without a guard, at a block of more than 2^31 elements (X side: cols * ldx; Y side: rows * ldy) -- test_unguarded_kernels[<case>-x|y] unless another test is named:
  csr_rows_kernel                loose-x/y; long rows: long-x/y
  csr_rows_pair_kernel           pair-x/y
  csr_group_kernel               group-x/y (and the far side of test_grouped_csr_pipeline_guard)
  csr_group_pipe_kernel          Y side: pipe-y
  csr_big_group_kernel           big-x/y
  csr_group_mfma_kernel          mfma-x/y; TABLE (factored untiled route): table-x/y
  csr_group_mfma16_kernel        mfma16-x/y
  csr_rows_f64_kernel            f64-x/y (f32 output), test_f64_kernel_float64_output (float64 output; its Y side at 2^30 doubles = the same 2^33-byte offset: 2^31 doubles
                                 are 17 GB and break the 20 GB cap)
  csr_patch_guard_kernel         patch-x/y (Inf under a missing entry)
  convtaps_exact_kernel          exact-x/y (far side of the pipeline and fill guards too)
  convtaps_exact_pipe_kernel     Y side: cpipe-y;  convtaps_exact_fill_kernel Y side: fill-y;  convtaps_narrow_kernel Y side: test_narrow_kernel_guard
  convtaps_mfma_kernel generic   generic-x/y (far side of the loader guards too); sptr Y side: sptr-y
  convtaps_smallk_kernel / _pipe test_small_k_kernels (x and y)
  convtaps_bf16x3_kernel         bf16x3-x/y (its own gate: 1e-5 max(1, |ref|max))
  dense split-K + dense_reduce_kernel   dense-x/y
  conv_lastrow_kernel            every conv case with a bias column;  convtaps_zero_guard_kernel: zguard-x/y (Inf under a dropped zero tap)
  absmax (kn_spmm_screen)        test_screen_at_large_offsets;  kn_absmax, kn_relu, kn_affine_to_linear, kn_linear_to_affine: test_helpers_at_large_offsets (these
                                 launch outside the plan mechanism: no plan string exists for them)
  kn_spmm_planes                 test_planes_beyond_2_31 (kn_spmm_plan describes kn_spmm only: the plan of one plane is asserted)
  chain_forward                  test_chain_at_large_offsets

What the block sizes can and cannot show.  The buffers hold 2^31 + 2^27 elements, so a case reaches element offsets just beyond 2^31 and byte offsets just beyond 2^33:
a signed or unsigned 32-bit BYTE offset and a signed 32-bit ELEMENT offset are caught; an unsigned 32-bit element offset would still be right here (it wraps at 2^32
elements = 16 GB per buffer, beyond the 20 GB cap).  Offsets between 2^32 elements and 2^64 are NOT exercised; "right in 64 bits" rests on reading the arithmetic there.

Guard mutations (scratch builds, not committed; the plan assertion fails before anything is launched): `A.cols * ldx < 2^31` -> `< 2^32` at the grouped CSR pipeline
(kn_csr.hip) fails test_grouped_csr_pipeline_guard[first-beyond]; `ldx * 4 < 2^24` -> `<=` at the filled-in kernel (kn_conv.hip, exact_choice) fails
test_filled_in_kernel_guards[...-ldx-first-beyond]; every other case of the two tests still passes.

Measured on an MI355X: the module's 70 cases take 8.2 s from the allocation of the buffers to their release (12.4 s for the pytest process; the slowest case 1.1 s), peak
torch.cuda.max_memory_allocated() = 18.82 GB (the two buffers and a case's operands).  The fixture prints both figures at teardown (run with -s)."""
import ctypes
import functools
import os
import time

import numpy as np
import pytest
import scipy.sparse
import torch

import oracle
import value_classes
from keynet_amd import sparse as ksp
from keynet_amd import _capi
from test_parity_gpu import _random_convtaps, close, close_conditioned, dev
from test_narrow_gpu import _dropped_zero_operator
from test_csr_mfma_gpu import grouped_operator

pytestmark = pytest.mark.gpu

(RELU, EXACT, BF16X3, NARROW) = (_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_BF16X3, _capi.KN_FLAG_NARROW)
NBUF = (1 << 31) + (1 << 27)          # elements of each shared buffer
BIG = (1 << 31) + (1 << 24)           # "beyond 2^31": what an unguarded case's block must reach
SENTINEL = -7.0
KN_ERR_UNSUPPORTED = 6                # enum kn_status, include/keynet_hip.h (keynet_amd/_capi.py has no name for it)


@pytest.fixture(scope='module')
def bufs():
    with torch.cuda.device(dev()):
        free = torch.cuda.mem_get_info()[0]
    if free < 24 * (1 << 30):
        pytest.skip('needs 24 GB of free device memory, %.1f GB free' % (free / 2.0 ** 30))
    torch.cuda.reset_peak_memory_stats(dev())
    t0 = time.time()
    hold = {'x': torch.empty(NBUF, dtype=torch.float32, device=dev()), 'y': torch.empty(NBUF, dtype=torch.float32, device=dev())}
    yield hold
    torch.cuda.synchronize()
    print('\ntest_large_offsets_gpu: wall %.1f s, peak torch.cuda.max_memory_allocated() = %.2f GB' % (time.time() - t0, torch.cuda.max_memory_allocated(dev()) / 1e9))
    x = hold.pop('x')
    y = hold.pop('y')
    del x, y
    for builder in (conv, dropped_zero_conv, grouped_csr, loose_csr, long_rows_csr, linear_csr, f64_csr, patched_csr, dense_case):
        builder.cache_clear()                                        # the operator handles go with the buffers
    torch.cuda.empty_cache()


# ---- operators (built once, shared by the cases that use them) --------------------------------------------------------------------------------------

class Case(object):
    """An operator handle, its canonical CSR for the oracle, and what keeps both alive."""

    def __init__(self, op, shape, ip, ix, dt, has_last=False, keep=None):
        (self.op, self.shape, self.ip, self.ix, self.dt, self.has_last, self.keep) = (op, tuple(int(v) for v in shape), ip, ix, dt, has_last, keep)
        assert tuple(op.shape()) == self.shape

    def ref(self, X):
        with np.errstate(all='ignore'):
            return oracle.csr_matvecs(self.shape, self.ip, self.ix, self.dt, X)


def _env(env, make):
    """make() with the KN_* options of `env` set: they are read when an operator is created and recorded in its handle."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        with torch.cuda.device(dev()):
            return make()
    finally:
        for (k, v) in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _csr_case(shape, ip, ix, dt, env=(), values=None, has_last=False):
    """`values`: a variant of value_classes.csr_values -- the builder's values by powers of two (tests/test_value_classes_gpu.py); None: as they are."""
    (ip, ix) = (np.asarray(ip, np.int32), np.asarray(ix, np.int32))
    dt = value_classes.csr_values(values, shape, ip, ix, dt, has_last)
    return Case(_env(dict(env), lambda: _capi.Operator.csr(shape, ip, ix, dt)), shape, ip, ix, dt)


def _conv_case(W, has_last, M=None, env=(), values=None):
    if values is not None:
        (W, M) = value_classes.revalued_convtaps(W, values)
    op = _env(dict(env), lambda: W._device_op(dev()))
    if M is None:
        M = W.tosparse('csr')
        M.sort_indices()
    return Case(op, M.shape, M.indptr, M.indices, M.data.astype(np.float32), has_last, keep=W)


@functools.lru_cache(maxsize=None)
def conv(Cin, Cout, H, k, stride, unit, has_last, gain=False, env=(), big_bias=False, values=None):
    rng = np.random.RandomState(1000 * Cin + 10 * Cout + H + k)
    assert unit or not gain
    W = _random_convtaps(rng, Cin, Cout, H, k, stride, unit, has_last)
    if gain:                  # one float coefficient per entry, no pixel pair hit twice: a permutation + gain key
        t = W._taps
        W = ksp.Conv2dTiledMatrix.fromtaps(W._inshape, W._outshape, t['taps'], t['ent_out'], t['ent_in'], t['ent_tap'], (0.5 + rng.rand(len(t['ent_out']))).astype(np.float32), t['lastcol'])
    if big_bias:              # the LAST output row proper gets a bias of 1e6: max |Y| then lies in a row whose offset is beyond 2^31 (kn_spmm_screen)
        t = W._taps
        lastcol = t['lastcol'].copy()
        lastcol[-2] = 1e6
        W = ksp.Conv2dTiledMatrix.fromtaps(W._inshape, W._outshape, t['taps'], t['ent_out'], t['ent_in'], t['ent_tap'], t['ent_coef'], lastcol)
    return _conv_case(W, has_last, env=env, values=values)


@functools.lru_cache(maxsize=None)
def dropped_zero_conv(values=None):
    (W, M) = _dropped_zero_operator(np.random.RandomState(5), 16, 32, 8)        # (32 output channels: the operator carries the stored-column table too)
    return _conv_case(W, True, M=M, values=values)


@functools.lru_cache(maxsize=None)
def grouped_csr(members=16, n_groups=1100, n=1024, env=(), values=None):
    rng = np.random.RandomState(members + n_groups)
    (m, ip, ix, dt) = grouped_operator(rng, n, members, n_groups, lambda g: 1 + (g * 7) % 70)
    return _csr_case((m, n), ip, ix, dt, env=env, values=values)


@functools.lru_cache(maxsize=None)
def loose_csr(big_last=False, values=None):
    rng = np.random.RandomState(3)
    (m, n) = (6000, 2048)
    lens = rng.randint(6, 12, m)
    lens[::97] = 0
    lens[5::501] = 40
    ip = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    ix = rng.randint(0, n, int(ip[-1])).astype(np.int32)
    dt = rng.randn(len(ix)).astype(np.float32)
    if big_last:              # the last row's values scaled by 1e6: max |Y| then lies in a row whose offset is beyond 2^31 (kn_spmm_screen)
        assert ip[-1] - ip[-2] >= 6
        dt[ip[-2]:] *= np.float32(1e6)
    return _csr_case((m, n), ip, ix, dt, values=values)


@functools.lru_cache(maxsize=None)
def long_rows_csr(long_rows=1100, values=None):
    """1 100 unrelated rows of 1 024 .. 1 100 stored entries each (duplicates, unsorted) and a few short ones."""
    rng = np.random.RandomState(4)
    (m, n) = (long_rows + 20, 1500)
    lens = np.concatenate((rng.randint(1024, 1101, long_rows), rng.randint(0, 9, 20)))
    ip = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    ix = rng.randint(0, n, int(ip[-1])).astype(np.int32)
    return _csr_case((m, n), ip, ix, (rng.randn(len(ix)) / 32).astype(np.float32), values=values)


@functools.lru_cache(maxsize=None)
def linear_csr(outs=300, ins=2500, env=(), values=None):
    """A keyed nn.Linear in the stored order: every row the same unsorted column sequence (one big pattern group) and the loose homogeneous row."""
    rng = np.random.RandomState(outs + ins)
    perm = rng.permutation(ins + 1).astype(np.int32)
    ix = np.concatenate([perm] * outs + [np.array([ins], np.int32)])
    ip = np.concatenate((np.arange(outs + 1) * (ins + 1), [outs * (ins + 1) + 1])).astype(np.int32)
    dt = np.concatenate(((rng.randn(outs * (ins + 1)) / np.sqrt(ins)).astype(np.float32), [np.float32(1.0)]))
    c = _csr_case((outs + 1, ins + 1), ip, ix, dt, env=env, values=values, has_last=True)
    c.has_last = True
    return c


@functools.lru_cache(maxsize=None)
def f64_csr(values=None):
    rng = np.random.RandomState(100)
    (m, n) = (301, 157)
    rows = [np.zeros(0, np.int32) if r % 17 == 0 else rng.randint(0, n, 3000 if r == 5 else rng.randint(1, 90)).astype(np.int32) for r in range(m)]
    ip = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int32)
    ix = np.concatenate(rows)
    dt = rng.randn(len(ix)) * np.exp(rng.uniform(-30, 30, len(ix)))
    return _csr_case((m, n), ip, ix, dt, values=values)


@functools.lru_cache(maxsize=None)
def patched_csr(values=None):
    """test_patched_group_members_vs_oracle's operator: group members that lost entries; returns (case, (row, missing columns) of the patched rows)."""
    rng = np.random.RandomState(11)
    (n_cols, n_groups, members, seq_len) = (700, 9, 21, 70)
    (ip, ix, dt, missing) = ([0], [], [], [])
    for g in range(n_groups):
        seq = rng.permutation(n_cols)[:seq_len]
        for m in range(members):
            keepm = np.ones(seq_len, bool)
            if m in (3, 7, 20):
                lose = {3: [0], 7: [seq_len - 1, 5], 20: [1, 30, 31]}[m]
                keepm[lose] = False
                missing.append((len(ip) - 1, seq[lose]))
            if m == 11:
                keepm[rng.choice(seq_len, 6, replace=False)] = False
            c = seq[keepm]
            ix.extend(int(v) for v in c)
            dt.extend(rng.randn(len(c)).astype(np.float32))
            ip.append(len(ix))
    for _ in range(13):
        c = rng.randint(0, n_cols, size=rng.randint(0, 9))
        ix.extend(int(v) for v in c)
        dt.extend(rng.randn(len(c)).astype(np.float32))
        ip.append(len(ix))
    return (_csr_case((len(ip) - 1, n_cols), ip, ix, np.array(dt, np.float32), values=values), missing)


@functools.lru_cache(maxsize=None)
def dense_case():
    rng = np.random.RandomState(7)
    (outs, ins) = (1100, 1024)
    D = np.zeros((outs + 1, ins + 1), dtype=np.float32)
    D[:-1, :-1] = (rng.randn(outs, ins) / np.sqrt(ins)).astype(np.float32)
    D[:-1, -1] = rng.randn(outs).astype(np.float32)
    D[-1, -1] = 1.0
    M = scipy.sparse.csr_matrix(D)
    with torch.cuda.device(dev()):
        op = _capi.Operator.dense(D)
    return Case(op, M.shape, M.indptr, M.indices, M.data, True)


# ---- the harness --------------------------------------------------------------------------------------------------------------------------------------

def last_ok(limit, mult, add=0):
    """The largest ldx % 4 == 0 with mult * ldx + add < limit, and the first multiple of 4 beyond it: (L, F)."""
    L = ((limit - add - 1) // mult) // 4 * 4
    assert mult * L + add < limit <= mult * (L + 4) + add
    return (L, L + 4)


def beyond(n_rows):
    """The smallest ld % 4 == 0 that puts a block of n_rows rows beyond BIG elements; it fits the buffer."""
    ld = (-(-BIG // n_rows) + 3) // 4 * 4
    assert n_rows * ld >= BIG > (1 << 31) and n_rows * ld <= NBUF
    return ld


def _data(case, n, seed=0, poison=None):
    rng = np.random.RandomState(seed + n)
    X = rng.randn(case.shape[1], n).astype(np.float32)
    if case.has_last:
        X[-1] = 1.0
    if poison is not None:
        poison(X)
    return X


def _same(a, b):
    """Bit for bit on the device, NaN positions included (-0 == +0, as np.array_equal has it in the existing parity tests)."""
    (na, nb) = (torch.isnan(a), torch.isnan(b))
    return bool(torch.equal(na, nb)) and bool(torch.equal(torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b)))


def _host_equal(y, ref):
    return np.array_equal(y, ref, equal_nan=True)


def _relu_ref(ref):
    return np.where(ref < 0, ref.dtype.type(0), ref)                 # torch relu: NaN stays NaN


def run(bufs, case, n, flags, ldx=None, ldy=None, expect=(), forbid=(), gate=None, X=None, f64out=False, relus=(0, RELU), absmax=False, sentinel=SENTINEL):
    """One call at (ldx, ldy) -- None = compact -- under the three checks; returns the plan.  gate(y, ref, X): the tolerance check of a kernel that is not order-preserving."""
    op = case.op
    (rows, cols) = case.shape
    (xbuf, ybuf) = (bufs['x'], bufs['y'])
    sentinel = float(np.float32(sentinel))                           # as the device holds it
    if f64out:
        ybuf = ybuf.view(torch.float64)
    ydt = torch.float64 if f64out else torch.float32
    esz = 8 if f64out else 4
    npad = (n + 3) // 4 * 4                                          # window start LD - npad: a multiple of 4 whatever n is
    (ldx, ldy) = (n if ldx is None else int(ldx), n if ldy is None else int(ldy))
    assert ldx >= npad or ldx == n
    assert ldy >= npad or ldy == n
    assert cols * ldx <= xbuf.numel() and rows * ldy <= ybuf.numel(), 'the block does not fit the shared buffer'
    (x0, y0) = (0 if ldx == n else ldx - npad, 0 if ldy == n else ldy - npad)
    if X is None:
        X = _data(case, n)
    ref = case.ref(X)
    xc = torch.as_tensor(X).to(dev())
    st = torch.cuda.current_stream(dev()).cuda_stream
    with torch.cuda.device(dev()):
        plan = op.plan(n, flags, ldx=ldx, ldy=ldy)
        plan_c = op.plan(n, flags)
    print('\n  [%s n=%d flags=%d ldx=%d ldy=%d  cols*ldx=2^31%+d rows*ldy=2^31%+d]\n    %s' % (case.shape, n, flags, ldx, ldy, cols * ldx - (1 << 31), rows * ldy - (1 << 31), plan))
    for e in expect:
        assert e in plan, (e, plan)
    for f in forbid:
        assert f not in plan, (f, plan)

    def call(xptr, lx, yptr, ly, fl, am=None):
        with torch.cuda.device(dev()):
            if f64out:
                op.spmm_f64(xptr, lx, n, yptr, ly, fl, st)
            else:
                op.spmm(xptr, lx, n, yptr, ly, fl, st, absmax_ptr=am)

    for relu in relus:
        fl = flags | relu
        r = _relu_ref(ref) if relu else ref
        if f64out:
            r = r.astype(np.float64)
        elif r.dtype != np.float32:
            with np.errstate(all='ignore'):
                r = r.astype(np.float32)                             # a float64 operator through kn_spmm: the block rounded to f32 once
        # the operands: compact ones are tensors of their own, large ones live at the end of every row of the shared buffers
        if ldx == n:
            xptr = xc.data_ptr()
        else:
            xbuf.fill_(float('nan'))
            xbuf[:cols * ldx].view(cols, ldx)[:, x0:x0 + n] = xc
            xptr = xbuf.data_ptr() + 4 * x0
        if ldy == n:
            ybig = torch.full((rows, n), sentinel, dtype=ydt, device=dev())
            yptr = ybig.data_ptr()
            ywin = ybig
        else:
            ybuf.fill_(sentinel)
            ywin = ybuf[:rows * ldy].view(rows, ldy)[:, y0:y0 + n]
            yptr = ybuf.data_ptr() + esz * y0
        am = torch.zeros(1, dtype=torch.float32, device=dev()) if absmax else None
        call(xptr, ldx, yptr, ldy, fl, None if am is None else am.data_ptr())
        torch.cuda.synchronize()
        got = ywin.contiguous()
        # (2) the same call on compact blocks
        yc = torch.full((rows, n), sentinel, dtype=ydt, device=dev())
        call(xc.data_ptr(), n, yc.data_ptr(), n, fl)
        torch.cuda.synchronize()
        # (1) the oracle
        gh = got.cpu().numpy()
        if gate is None:
            assert _host_equal(gh, r), ('oracle', relu, plan, int(np.sum(~((gh == r) | (np.isnan(gh) & np.isnan(r))))))
            assert _same(got, yc), ('compact', relu, plan)
        else:
            d = float(np.nanmax(np.abs(gh.astype(np.float64) - r)))
            print('    relu=%d  max |y - oracle| = %.3g   max |y - compact| = %.3g' % (relu, d, float((got - yc).abs().max())))
            assert gate(gh, r, X), ('gate', relu, plan, d)
            if plan == plan_c:
                assert _same(got, yc), ('compact', relu, plan)
            else:
                assert gate(yc.cpu().numpy(), r, X), ('gate on the compact call', relu, plan_c)
        if am is not None:
            ah = np.where(np.isnan(gh), 0, np.abs(gh))
            assert float(am.item()) == float(ah.max()), (float(am.item()), float(ah.max()))
            if ldy != n:                                             # the maximum must come from a row the kernel reaches only with an offset beyond 2^31
                top = int(np.argmax(ah.max(axis=1)))
                assert top * ldy >= (1 << 31), (top, ldy)
        # (3) nothing was stored outside the window
        if ldy != n:
            ywin.fill_(sentinel)
            assert float(ybuf.min()) == sentinel and float(ybuf.max()) == sentinel, ('a store outside the window', relu, plan)
    return plan


def conditioned(case):
    return lambda y, r, X: close_conditioned(y.T, r.T, (case.shape, case.ip, case.ix, case.dt), X.T)


# ---- A. guarded fast kernels, both sides of every guard ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('side', ['last', 'first-beyond'])
def test_grouped_csr_pipeline_guard(bufs, side):
    """cols * ldx < 2^31 (kn_csr.hip: the pipeline keeps col * ldx in 32 bits): 1 024 columns, ldx = 2^21 - 4 | 2^21."""
    c = grouped_csr()
    (L, F) = last_ok(1 << 31, c.shape[1])
    assert (L, F) == ((1 << 21) - 4, 1 << 21)
    if side == 'last':
        run(bufs, c, 512, EXACT, ldx=L, expect=['csr_group_pipe_kernel'])
    else:
        run(bufs, c, 512, EXACT, ldx=F, expect=['csr_group_kernel'], forbid=['csr_group_pipe_kernel'])


@pytest.mark.parametrize('side', ['last', 'first-beyond'])
@pytest.mark.parametrize('n,form', [(256, ''), (128, '128-column tiles')])
def test_conv_pipeline_guard(bufs, n, form, side):
    """(Cin HiWi + 1) * ldx < 2^31 (signed 32-bit element offsets of convtaps_exact_pipe_kernel), at four and at two batch columns per lane."""
    c = conv(16, 64, 8, 3, 1, True, True)
    (L, F) = last_ok(1 << 31, 16 * 64 + 1)
    if side == 'last':
        plan = run(bufs, c, n, EXACT, ldx=L, expect=['convtaps_exact_pipe_kernel', form])
        assert ('128-column tiles' in plan) == (n == 128)
    else:
        run(bufs, c, n, EXACT, ldx=F, expect=['convtaps_exact_kernel<vec=%d>' % (4 if n == 256 else 1)], forbid=['convtaps_exact_pipe_kernel'])


@pytest.mark.parametrize('Cout,n,which,loader', [
    (128, 128, 'sptr-last', 'loader=sptr('), (128, 128, 'sptr-first-beyond', 'loader=fast('), (128, 128, 'fast-last', 'loader=fast('), (128, 128, 'fast-first-beyond', 'loader=generic'),
    (64, 256, 'sptr-last', 'loader=sptr('), (64, 256, 'fast-first-beyond', 'loader=generic')])
def test_matrix_core_conv_loader_guards(bufs, Cout, n, which, loader):
    """convtaps_mfma_kernel, Cin = 16, 8 x 8 pixels.  128 x 128 tiles: wave-uniform loaders while 4 (8 HiWi ldx + 128) < 2^31, straight-line loaders while
    16 HiWi ldx < 2^31, the generic loader beyond.  64 x 256 tiles: 4 (4 HiWi ldx + 256) < 2^31 and 16 HiWi ldx < 2^31 end at the same ldx."""
    c = conv(16, Cout, 8, 3, 1, True, True)
    NB = 128 if Cout > 64 else 256
    sp = last_ok(1 << 31, 4 * (1024 // NB) * 64, 4 * NB)
    fa = last_ok(1 << 31, 16 * 64)
    if NB == 256:
        assert sp == fa
    ldx = {'sptr-last': sp[0], 'sptr-first-beyond': sp[1], 'fast-last': fa[0], 'fast-first-beyond': fa[1]}[which]
    others = [s for s in ('loader=sptr(', 'loader=fast(', 'loader=generic') if s != loader]
    run(bufs, c, n, 0, ldx=ldx, expect=['convtaps_mfma_kernel<MT=%d,NB=%d,KC=16>' % (128 if Cout > 64 else 64, NB), loader], forbid=others, gate=conditioned(c))


@pytest.mark.parametrize('shape,n,form,guard,side', [
    ((4, 32, 8, 3), 64, '<taps in registers>', 'ldx', 'last'), ((4, 32, 8, 3), 64, '<taps in registers>', 'ldx', 'first-beyond'),
    ((2, 128, 20, 3), 256, '<taps in registers, 64 channels per wavefront>', 'plane', 'last'), ((2, 128, 20, 3), 256, '<taps in registers, 64 channels per wavefront>', 'plane', 'first-beyond'),
    ((2, 128, 28, 3), 256, '<taps in registers, 64 channels per wavefront, two column tiles per wavefront>', 'plane', 'last'),
    ((2, 128, 28, 3), 256, '<taps in registers, 64 channels per wavefront, two column tiles per wavefront>', 'plane', 'first-beyond'),
    ((3, 32, 28, 3), 384, '<taps in registers, two column tiles per wavefront>', 'fits', 'last')])
def test_filled_in_kernel_guards(bufs, shape, n, form, guard, side):
    """convtaps_exact_fill_kernel: 4 ldx < 2^24 (the 24-bit multiply of its row offsets) at 8 x 8 pixels, 4 HiWi ldx < 2^32 (its unsigned 32-bit byte offsets inside one
    input channel) at 20 x 20 and 28 x 28 pixels; beyond either, convtaps_exact_kernel.  'fits': the 32-channel two-tile form at the largest ldx the buffer holds."""
    (Cin, Cout, H, k) = shape
    c = conv(Cin, Cout, H, k, 1, False, True)
    (L, F) = {'ldx': last_ok(1 << 24, 4), 'plane': last_ok(1 << 32, 4 * H * H), 'fits': (NBUF // c.shape[1] // 4 * 4, None)}[guard]
    if guard == 'ldx':
        assert (L, F) == ((1 << 22) - 4, 1 << 22) and H * H <= 144
    if side == 'last':
        assert 4 * L < (1 << 24) and 4 * H * H * L < (1 << 32)
        run(bufs, c, n, EXACT, ldx=L, expect=['convtaps_exact_fill_kernel' + form + ' ('])
    else:
        run(bufs, c, n, EXACT, ldx=F, expect=['convtaps_exact_kernel'], forbid=['convtaps_exact_fill_kernel'])


@pytest.mark.parametrize('n', [1, 3, 8])
def test_narrow_kernel_guard(bufs, n, monkeypatch):
    """KN_FLAG_NARROW: (Cin HiWi + 1) * ldx + 8 < 2^31, else KN_ERR_UNSUPPORTED with Y untouched -- the flag refuses, it does not fall back; its Y side at rows * ldy > 2^31."""
    c = conv(16, 64, 8, 3, 1, True, True)
    (L, F) = last_ok(1 << 31, 16 * 64 + 1, 8)
    run(bufs, c, n, EXACT | NARROW, ldx=L, expect=['convtaps_narrow_kernel'])
    run(bufs, c, n, EXACT | NARROW, ldy=beyond(c.shape[0]), expect=['convtaps_narrow_kernel'], relus=(0,))
    # the first refused ldx
    (rows, cols) = c.shape
    (xbuf, ybuf) = (bufs['x'], bufs['y'])
    assert cols * F <= NBUF
    X = _data(c, n)
    xbuf.fill_(float('nan'))
    xbuf[:cols * F].view(cols, F)[:, F - 8:F - 8 + n] = torch.as_tensor(X).to(dev())
    ybuf.fill_(SENTINEL)
    with torch.cuda.device(dev()):
        buf = ctypes.create_string_buffer(1024)
        assert _capi.lib().kn_spmm_plan(c.op.handle, n, F, n, EXACT | NARROW, buf, 1024) == KN_ERR_UNSUPPORTED
        rc = _capi.lib().kn_spmm(c.op.handle, xbuf.data_ptr() + 4 * (F - 8), F, n, ybuf.data_ptr(), n, EXACT | NARROW, torch.cuda.current_stream(dev()).cuda_stream)
    torch.cuda.synchronize()
    assert rc == KN_ERR_UNSUPPORTED and b'KN_FLAG_NARROW' in _capi.lib().kn_last_error()
    assert float(ybuf.min()) == SENTINEL and float(ybuf.max()) == SENTINEL
    # the Python container hands the library a compact copy of a strided operand: the narrow kernel at ldx = n, the same bits
    view = xbuf[:cols * F].view(cols, F)[:, F - 8:F - 8 + n]
    calls = _spy_spmm(monkeypatch)
    y = c.keep.torchdot(view, exact=True, narrow=True)
    assert _host_equal(y.cpu().numpy(), c.ref(X))
    assert len(calls) == 1 and calls[0][1:] == (n, n, n), calls
    assert 'convtaps_narrow_kernel' in calls[0][0], calls


def _spy_spmm(monkeypatch):
    """Records (plan, ldx, n_vecs, ldy) of every kn_spmm a container issues from here on: which kernel ran, on which block."""
    calls = []
    real = _capi.Operator.spmm

    def spmm(self, x_ptr, ldx, n_vecs, y_ptr, ldy, flags, stream, absmax_ptr=None):
        calls.append((self.plan(n_vecs, flags, ldx=ldx, ldy=ldy), int(ldx), int(n_vecs), int(ldy)))
        return real(self, x_ptr, ldx, n_vecs, y_ptr, ldy, flags, stream, absmax_ptr=absmax_ptr)
    monkeypatch.setattr(_capi.Operator, 'spmm', spmm)
    return calls


def test_narrow_forward_of_a_strided_batch(bufs, golden, monkeypatch):
    """KeyedModel.forward_linear(narrow=True) on a row-major batch whose images lie NBUF / (n - 1) elements apart inside the X buffer (the last one starts beyond 2^31
    elements; NaN everywhere else): the container lays the batch out feature-major ONCE as a compact block, so every layer's kn_spmm sees ldx = ldy = n_vecs, the conv
    layers run convtaps_narrow_kernel, nothing is padded, and the logits are bit-equal to the forward of a compact copy and to the reference vectors of the golden file
    (whose narrow forward is bit-exact: test_narrow_gpu.py)."""
    from keynet_amd import io as kio
    z = golden('mini_tiled_permutation.npz')
    knet = kio.keynet_from_arrays(z)
    xh = np.ascontiguousarray(z['x_cipher'][:8].astype(np.float32))
    (n, d) = xh.shape
    assert 1 <= n <= 8
    assert n >= 2
    LD = (NBUF - d - 3) // (n - 1)
    assert (n - 1) * LD + 3 + d <= NBUF and (n - 1) * LD > (1 << 31)       # the last image starts beyond 2^31 elements
    xbuf = bufs['x']
    xbuf.fill_(float('nan'))
    view = xbuf.as_strided((n, d), (LD, 1), 3)                            # (an odd start: nothing about the view is aligned)
    view.copy_(torch.as_tensor(xh))
    compact = torch.as_tensor(xh).to(dev())
    y_compact = knet.forward_linear(compact, narrow=True)
    knet._padded_forwards = 0
    calls = _spy_spmm(monkeypatch)
    y = knet.forward_linear(view, narrow=True)
    assert torch.equal(y, y_compact)
    names = [str(v) for v in z['layer_names']]
    assert np.array_equal(y.cpu().numpy(), z['Y.%s' % names[-1]][:n])
    assert knet._padded_forwards == 0
    assert calls and all(c[1:] == (n, n, n) for c in calls), [c[1:] for c in calls]
    n_conv = sum(1 for c in knet._keyed() if isinstance(c.W, ksp.Conv2dTiledMatrix))
    assert n_conv > 0 and sum(1 for c in calls if 'convtaps_narrow_kernel' in c[0]) == n_conv, [c[0] for c in calls]
    assert not any('convtaps_mfma_kernel' in c[0] or 'convtaps_exact' in c[0] for c in calls)


@pytest.mark.parametrize('side', ['x', 'y'])
@pytest.mark.parametrize('H,kernel', [(8, 'convtaps_smallk_kernel'), (32, 'convtaps_smallk_pipe_kernel')])
def test_small_k_kernels(bufs, H, kernel, side):
    """The small-K pair forms row * ldx in 64 bits: the same kernel on both sides of cols * ldx = 2^31 and at rows * ldy > 2^31 (the gate of every matrix-core launch)."""
    c = conv(3, 64, H, 3, 1, True, True, env=(('KN_NO_SMALLK_PIPE', '1'),) if H == 8 else ())
    if side == 'y':
        run(bufs, c, 256, 0, ldy=beyond(c.shape[0]), expect=[kernel], gate=conditioned(c), relus=(0,))
        return
    (L, F) = last_ok(1 << 31, c.shape[1])
    run(bufs, c, 256, 0, ldx=L, expect=[kernel], gate=conditioned(c), relus=(0,))
    run(bufs, c, 256, 0, ldx=beyond(c.shape[1]), expect=[kernel], gate=conditioned(c))


# ---- B / C. kernels without a guard: X side (cols * ldx > 2^31) and Y side (rows * ldy > 2^31) --------------------------------------------------------------

def _bf16x3_gate(y, r, X):
    return float(np.abs(y - r).max()) <= 1e-5 * max(1.0, float(np.abs(r).max())) and np.array_equal(y[-1], r[-1])


def _dense_gate(case):
    return lambda y, r, X: conditioned(case)(y, r, X) and close(y, r, tol=2e-5)


def _unguarded(name):
    """(case, n_vecs, flags, kernel names the plan must hold, names it must not hold, gate, X or None, sides)."""
    if name == 'loose':
        return (loose_csr(), 256, EXACT, ['csr_rows_kernel<vec=4>'], ['csr_rows_pair_kernel'], None, None)
    if name == 'pair':
        return (loose_csr(), 128, EXACT, ['csr_rows_pair_kernel'], [], None, None)
    if name == 'long':
        return (long_rows_csr(), 256, EXACT, ['csr_rows_kernel<vec=4> (long rows)'], [], None, None)
    if name == 'group':
        return (grouped_csr(), 100, EXACT, ['csr_group_kernel'], ['csr_group_pipe_kernel'], None, None)
    if name == 'pipe':
        return (grouped_csr(), 512, EXACT, ['csr_group_pipe_kernel'], [], None, None)
    if name == 'big':
        return (linear_csr(env=(('KN_BIG_MFMA16', '0'),)), 100, EXACT, ['csr_big_group_kernel'], ['csr_group_mfma16_kernel'], None, None)
    if name == 'mfma16':
        return (linear_csr(env=(('KN_BIG_MFMA16', '1'),)), 128, EXACT, ['csr_group_mfma16_kernel'], [], None, None)
    if name == 'mfma':
        return (grouped_csr(192, 300, 1100, env=(('KN_GROUP_MFMA', '1'),)), 256, EXACT, ['csr_group_mfma_kernel'], [], None, None)
    if name == 'f64':
        c = f64_csr()
        X = _data(c, 256, poison=_poison_plain)
        return (c, 256, EXACT, ['csr_rows_f64_kernel'], [], None, X)
    if name == 'patch':
        (c, missing) = patched_csr()

        def poison(X):
            X[missing[0][1][0], 1] = np.inf                          # at a missing position of a patched row: must NOT reach that row
            X[missing[4][1][-1], 2] = np.nan
            X[c.ix[c.ip[missing[0][0]]], 3] = -np.inf                # at a present position: must reach it
        return (c, 256, EXACT, ['csr_patch_guard_kernel<%d patched rows>' % len(missing)], [], None, _data(c, 256, poison=poison))
    if name == 'exact':
        return (conv(4, 32, 8, 3, 1, False, True, env=(('KN_NO_FILL_EXACT', '1'),)), 64, EXACT, ['convtaps_exact_kernel', 'conv_lastrow_kernel'], ['convtaps_exact_fill_kernel', 'convtaps_exact_pipe_kernel'], None, None)
    if name == 'cpipe':
        return (conv(16, 64, 8, 3, 1, True, True), 256, EXACT, ['convtaps_exact_pipe_kernel', 'conv_lastrow_kernel'], [], None, None)
    if name == 'fill':
        return (conv(4, 32, 8, 3, 1, False, True), 64, EXACT, ['convtaps_exact_fill_kernel'], [], None, None)
    if name == 'generic':
        c = conv(16, 128, 8, 3, 1, True, True, gain=True, env=(('KN_NO_SPTR', '1'),))
        return (c, 128, 0, ['convtaps_mfma_kernel', 'loader=generic'], [], conditioned(c), None)
    if name == 'sptr':
        c = conv(16, 128, 8, 3, 1, True, True)
        return (c, 128, 0, ['convtaps_mfma_kernel', 'loader=sptr('], [], conditioned(c), None)
    if name == 'bf16x3':
        c = conv(16, 128, 8, 3, 1, True, True)
        return (c, 128, BF16X3, ['convtaps_bf16x3_kernel'], [], _bf16x3_gate, None)
    if name == 'dense':
        c = dense_case()
        return (c, 256, 0, ['convtaps_mfma_kernel', 'dense_reduce_kernel'], [], _dense_gate(c), None)
    if name in ('zguard', 'table'):
        c = dropped_zero_conv()
        n = 64 if name == 'zguard' else 128
        X = _data(c, n, poison=_poison_dropped_zero)
        if name == 'zguard':
            return (c, n, EXACT, ['convtaps_exact_kernel', 'convtaps_zero_guard_kernel'], [], None, X)
        return (c, n, EXACT, ['csr_group_mfma_kernel', 'convtaps_zero_guard_kernel'], ['convtaps_exact_kernel', 'convtaps_exact_pipe_kernel'], None, X)
    raise KeyError(name)


def _poison_plain(X):
    X[3, 0] = np.inf
    X[11, X.shape[1] - 1] = np.nan
    X[20, X.shape[1] // 2] = 1e-42


def _poison_dropped_zero(X):
    """Inf and NaN exactly where the reference has NO entry: under a zero-valued tap entry (t, co, ci) at an input pixel one of the tap's entries reads."""
    F = dropped_zero_conv().keep._factored
    t = F._taps
    zt = np.argwhere(t['taps'] == 0)
    assert len(zt) >= 3
    HW = int(F._inshape[1] * F._inshape[2])
    for (q, (tap, co, ci)) in enumerate(zt[:3]):
        e = np.flatnonzero(t['ent_tap'] == tap)[q]
        X[ci * HW + t['ent_in'][e], 1 + q] = np.inf if q != 1 else np.nan
    X[5, 0] = -np.inf                                                # ... and one the reference does read


UNGUARDED_X = ['loose', 'pair', 'long', 'group', 'big', 'mfma16', 'mfma', 'table', 'f64', 'patch', 'exact', 'generic', 'bf16x3', 'dense', 'zguard']
UNGUARDED_Y = UNGUARDED_X + ['pipe', 'cpipe', 'fill', 'sptr']


@pytest.mark.parametrize('name,side', [(k, 'x') for k in UNGUARDED_X] + [(k, 'y') for k in UNGUARDED_Y], ids=lambda v: v)
def test_unguarded_kernels(bufs, name, side):
    """A kernel that must be right in 64 bits: one block of more than 2^31 elements on the X side (compact Y) or on the Y side (compact X)."""
    (c, n, flags, expect, forbid, gate, X) = _unguarded(name)
    if side == 'x':
        run(bufs, c, n, flags, ldx=beyond(c.shape[1]), expect=expect, forbid=forbid, gate=gate, X=X)
    else:
        run(bufs, c, n, flags, ldy=beyond(c.shape[0]), expect=expect, forbid=forbid, gate=gate, X=X)


@pytest.mark.parametrize('side', ['x', 'y'])
def test_f64_kernel_float64_output(bufs, side):
    """kn_spmm_f64: the float64 block.  Its Y side reaches 2^30 + 2^23 doubles -- the byte offset of 2^31 f32 elements; 2^31 doubles (17 GB) would break the module's cap."""
    c = f64_csr()
    X = _data(c, 256, poison=_poison_plain)
    if side == 'x':
        run(bufs, c, 256, EXACT, ldx=beyond(c.shape[1]), expect=['csr_rows_f64_kernel'], X=X, f64out=True)
    else:
        ldy = (-(-(BIG // 2) // c.shape[0]) + 3) // 4 * 4
        assert c.shape[0] * ldy * 8 > (1 << 33)
        run(bufs, c, 256, EXACT, ldy=ldy, expect=['csr_rows_f64_kernel'], X=X, f64out=True)


@pytest.mark.parametrize('name', ['loose', 'cpipe', 'sptr'])
def test_screen_at_large_offsets(bufs, name):
    """kn_spmm_screen with rows * ldy > 2^31: max |Y| equals the window's, whether it rides in a kernel's epilogue (loose rows, matrix-core tiles) or is a pass over Y
    (absmax_kernel_win4 behind the order-preserving conv kernel).  The operators are variants whose LAST row proper is 1e6 times larger than the others, so the maximum
    lies in a row whose offset is beyond 2^31 (asserted), and the Y buffer outside the window holds -1e30 instead of -7: a read that wrapped into the buffer would raise
    the maximum, a pass that skipped the far rows would lower it.  And with cols * ldx > 2^31, where the two conv operators are beyond their fast kernels' guards and run
    the plain order-preserving kernel / the generic loader."""
    (c, n, flags, expect, gate) = {
        'loose': lambda: (loose_csr(big_last=True), 256, EXACT, ['csr_rows_kernel<vec=4>'], None),
        'cpipe': lambda: (conv(16, 64, 8, 3, 1, True, True, big_bias=True), 256, EXACT, ['convtaps_exact_pipe_kernel', 'conv_lastrow_kernel'], None),
        'sptr': lambda: (conv(16, 128, 8, 3, 1, True, True, big_bias=True), 128, 0, ['convtaps_mfma_kernel', 'loader=sptr('], 'conditioned')}[name]()
    if gate == 'conditioned':
        gate = conditioned(c)
    run(bufs, c, n, flags, ldy=beyond(c.shape[0]), expect=expect, gate=gate, absmax=True, sentinel=-1e30)
    beyond_x = {'loose': ['csr_rows_kernel<vec=4>'], 'cpipe': ['convtaps_exact_kernel<vec=4>'], 'sptr': ['convtaps_mfma_kernel', 'loader=generic']}[name]
    run(bufs, c, n, flags, ldx=beyond(c.shape[1]), expect=beyond_x, forbid=['convtaps_exact_pipe_kernel', 'loader=sptr('], gate=gate, absmax=True, relus=(0,))


# ---- D. helpers, planes, the whole-net kernel ------------------------------------------------------------------------------------------------------------

def test_helpers_at_large_offsets(bufs):
    """kn_relu / kn_absmax with rows * ld > 2^31, kn_affine_to_linear with d * ldo > 2^31, kn_linear_to_affine with d * ldy > 2^31 (its maxdev = the reference's)."""
    (xbuf, ybuf) = (bufs['x'], bufs['y'])
    rng = np.random.RandomState(8)
    st = torch.cuda.current_stream(dev()).cuda_stream
    (rows, n) = (1025, 64)
    ld = beyond(rows)
    A = rng.randn(rows, n).astype(np.float32)
    A[3, 5] = np.nan
    A[rows - 1, 7] = 1e6                                             # kn_absmax: the maximum lies in the last row, whose offset is beyond 2^31
    # kn_relu: only the window changes (the sentinel is negative: a stray ReLU would turn it into 0)
    ybuf.fill_(SENTINEL)
    win = ybuf[:rows * ld].view(rows, ld)[:, ld - n:]
    win.copy_(torch.as_tensor(A))
    with torch.cuda.device(dev()):
        _capi.relu(ybuf.data_ptr() + 4 * (ld - n), rows, ld, n, st)
    torch.cuda.synchronize()
    assert _host_equal(win.cpu().numpy(), _relu_ref(A))
    win.fill_(SENTINEL)
    assert float(ybuf.min()) == SENTINEL and float(ybuf.max()) == SENTINEL
    # kn_absmax: everything outside the window is LARGER than the window's maximum (NaN is ignored by the reduction and would hide a wrapped read)
    xbuf.fill_(1e30)
    xbuf[:rows * ld].view(rows, ld)[:, ld - n:] = torch.as_tensor(A).to(dev())
    for (nn, kernel) in ((n, 'win4'), (n - 1, 'scalar')):
        am = torch.zeros(1, dtype=torch.float32, device=dev())
        with torch.cuda.device(dev()):
            _capi.absmax(xbuf.data_ptr() + 4 * (ld - n), rows, ld, nn, am.data_ptr(), st)
        assert float(am.item()) == float(np.nanmax(np.abs(A[:, :nn]))), kernel
    # kn_affine_to_linear: [n, d] images -> [d + 1, n] feature-major at ldo
    (d, ni) = (1024, 64)
    ldo = beyond(d + 1)
    img = rng.rand(ni, d).astype(np.float32)
    ybuf.fill_(SENTINEL)
    imgd = torch.as_tensor(img).to(dev())
    with torch.cuda.device(dev()):
        _capi.affine_to_linear(imgd.data_ptr(), ni, d, ybuf.data_ptr() + 4 * (ldo - ni), ldo, st)
    torch.cuda.synchronize()
    win = ybuf[:(d + 1) * ldo].view(d + 1, ldo)[:, ldo - ni:]
    assert np.array_equal(win.cpu().numpy(), np.ascontiguousarray(oracle.affine_to_linear(img).T))
    win.fill_(SENTINEL)
    assert float(ybuf.min()) == SENTINEL and float(ybuf.max()) == SENTINEL
    # kn_linear_to_affine: [d + 1, n] feature-major at ldy -> [n, d]
    Yl = np.vstack((rng.randn(d, ni).astype(np.float32), (1.0 + 1e-4 * rng.randn(1, ni)).astype(np.float32)))
    xbuf.fill_(float('nan'))
    xbuf[:(d + 1) * ldo].view(d + 1, ldo)[:, ldo - ni:] = torch.as_tensor(Yl).to(dev())
    out = torch.full((ni, d), SENTINEL, dtype=torch.float32, device=dev())
    md = torch.full((1,), -1.0, dtype=torch.float32, device=dev())
    with torch.cuda.device(dev()):
        _capi.linear_to_affine(xbuf.data_ptr() + 4 * (ldo - ni), ldo, ni, d, out.data_ptr(), md.data_ptr(), st)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), np.ascontiguousarray(Yl[:-1].T))
    assert float(md.item()) == float(np.abs(Yl[-1] - np.float32(1.0)).max())


def test_planes_beyond_2_31(bufs):
    """kn_spmm_planes: plane strides of 2^31 + 2^20 floats on both sides, so the second plane starts beyond 2^31 elements; bit-equal to kn_spmm per plane and to the oracle."""
    (xbuf, ybuf) = (bufs['x'], bufs['y'])
    rng = np.random.RandomState(9)
    (m, nc, n, ld) = (700, 300, 64, 128)
    M = scipy.sparse.random(m, nc, density=0.03, format='csr', random_state=rng, dtype=np.float32)
    c = _csr_case((m, nc), M.indptr, M.indices, M.data.astype(np.float32))
    stride = (1 << 31) + (1 << 20)
    assert stride + max(m, nc) * ld <= NBUF
    st = torch.cuda.current_stream(dev()).cuda_stream
    with torch.cuda.device(dev()):
        assert 'csr_rows_kernel' in c.op.plan(n, EXACT, ldx=ld, ldy=ld)
    Xs = [rng.randn(nc, n).astype(np.float32) for _ in range(2)]
    for relu in (0, RELU):
        xbuf.fill_(float('nan'))
        ybuf.fill_(SENTINEL)
        for (p, X) in enumerate(Xs):
            xbuf[p * stride:p * stride + nc * ld].view(nc, ld)[:, ld - n:] = torch.as_tensor(X).to(dev())
        with torch.cuda.device(dev()):
            assert c.op.spmm_planes(xbuf.data_ptr() + 4 * (ld - n), ld, stride, 2, n, ybuf.data_ptr() + 4 * (ld - n), ld, stride, EXACT | relu, st) is True
        torch.cuda.synchronize()
        for (p, X) in enumerate(Xs):
            win = ybuf[p * stride:p * stride + m * ld].view(m, ld)[:, ld - n:]
            r = c.ref(X)
            assert _host_equal(win.cpu().numpy(), _relu_ref(r) if relu else r), (p, relu)
            yc = torch.full((m, n), SENTINEL, dtype=torch.float32, device=dev())
            xc = torch.as_tensor(X).to(dev())
            with torch.cuda.device(dev()):
                c.op.spmm(xc.data_ptr(), n, n, yc.data_ptr(), n, EXACT | relu, st)
            assert _same(win.contiguous(), yc)
            win.fill_(SENTINEL)
        assert float(ybuf.min()) == SENTINEL and float(ybuf.max()) == SENTINEL


@pytest.mark.parametrize('side', ['x', 'y'])
def test_chain_at_large_offsets(bufs, side):
    """A two-operator kn_chain_create handle (1 025 -> 300 -> 1 025 features) with cols * ldx > 2^31 and with rows * ldy > 2^31: the oracle operator by operator."""
    rng = np.random.RandomState(10)

    def rand_csr(rows, cols):
        lens = rng.randint(1, 14, rows)
        ip = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
        ix = rng.randint(0, cols, int(ip[-1])).astype(np.int32)
        return (ip, ix, rng.randn(len(ix)).astype(np.float32))
    mats = [((300, 1025),) + rand_csr(300, 1025), ((1025, 300),) + rand_csr(1025, 300)]
    with torch.cuda.device(dev()):
        ops = [_capi.Operator.csr(s, ip, ix, dt) for (s, ip, ix, dt) in mats]
        chain = _capi.Operator.chain(ops, [RELU, 0])
    n = 64

    class Chain(Case):
        def ref(self, X):
            y = np.maximum(oracle.csr_matvecs(*mats[0], X), 0)
            return oracle.csr_matvecs(*mats[1], y)
    c = Chain(chain, (1025, 1025), None, None, None)
    kw = {'ldx': beyond(1025)} if side == 'x' else {'ldy': beyond(1025)}
    run(bufs, c, n, EXACT, expect=['chain_kernel'], relus=(0,), **kw)
