"""The row-lane form of the low-latency forward for 1 .. 8 images on the GPU: csr_narrow_kernel (KN_FLAG_NARROW_ROWS: the lane is the output row, the batch
columns are its running sums) against the CPU oracle in stored order, bit for bit, on every role of a CSR handle (big and small pattern groups, loose rows,
long rows, patched rows); the flag's semantics through the C ABI; and KeyedModel.forward_linear / capture with narrow_rows=True."""
import copy
import functools

import numpy as np
import pytest
import torch

import oracle
from keynet_amd import io as kio
from keynet_amd import sparse as ksp
from keynet_amd import _capi
from test_parity_gpu import dev
from test_narrow_gpu import _build, _last
from narrow_helpers import SENTINEL, _spmm, _spmm_calls

pytestmark = pytest.mark.gpu

(RELU, EXACT, NARROW, MFMA, ROWS) = (_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_NARROW, _capi.KN_FLAG_NARROW_MFMA, _capi.KN_FLAG_NARROW_ROWS)
KERNEL = 'csr_narrow_kernel'


# ---- operators: each the smallest that reaches its role -------------------------------------------------------------------------------------------------
def _csr(rows, n_cols, rng):
    """(shape, indptr, indices, data) from a list of column arrays, stored as given (unsorted, repeats allowed); values in [-1, 1) without exact zeros."""
    indptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int32)
    indices = (np.concatenate(rows) if len(rows) else np.zeros(0)).astype(np.int32)
    data = rng.uniform(-1, 1, len(indices)).astype(np.float32)
    data[data == 0] = 0.5
    return ((len(rows), n_cols), indptr, indices, data)


def _linear(rng, members, ncol):
    """A keyed nn.Linear in affine form: `members` rows over ONE shared (permuted) column sequence of ncol entries, and the homogeneous row (a loose row)."""
    pattern = rng.permutation(ncol).astype(np.int32)
    return _csr([pattern] * members + [np.array([ncol - 1], np.int32)], ncol, rng)


def _small_groups(rng):
    """Conv-like: 40 pixel groups of 8 member rows x 28 unsorted columns."""
    n = 300
    rows = []
    for _ in range(40):
        rows += [rng.permutation(n)[:28].astype(np.int32)] * 8
    return _csr(rows, n, rng)


def _pool(rng):
    """Pool-like loose rows of 0 .. 13 entries: empty rows, unsorted indices, a repeated column; 300 rows = two workgroups of the loose role."""
    n = 500
    rows = [rng.randint(0, n, int(k)).astype(np.int32) for k in rng.randint(0, 14, 300)]
    rows[3] = np.zeros(0, np.int32)
    rows[4] = np.array([7, 2, 7, 7, 400, 2], np.int32)                  # a repeated column
    rows[299] = np.zeros(0, np.int32)
    return _csr(rows, n, rng)


def _long(rng):
    """One row of 1 100 entries (the deep-queue role, unchanged) between pool-like rows and a small group."""
    n = 1300
    rows = [rng.randint(0, n, int(k)).astype(np.int32) for k in rng.randint(0, 10, 20)]
    rows.insert(5, rng.randint(0, n, 1100).astype(np.int32))
    rows += [rng.permutation(n)[:40].astype(np.int32)] * 9
    return _csr(rows, n, rng)


PATCH_POS = 5


def _patched(rng):
    """A group of 12 rows over 40 sorted columns and a 13th row that lost entry PATCH_POS to an exact zero: it rides in the group, csr_patch_guard_kernel covers it."""
    n = 200
    pattern = np.sort(rng.permutation(n)[:40]).astype(np.int32)
    return _csr([pattern] * 12 + [np.delete(pattern, PATCH_POS)] + [rng.randint(0, n, 4).astype(np.int32)], n, rng) + (int(pattern[PATCH_POS]),)


CASES = {
    # 262 = 4 x 64 + 6 member rows (no multiple of 64, 32 or 16), 2 057 = 42 x 48 + 41 columns (no multiple of the 48-step ring or a scalar batch): a BIG group
    'linear-big': (lambda rng: _linear(rng, 262, 2057), ['csr_big_group_kernel'], None),
    # the same pattern below either big-group threshold (256 members, 2 048 columns): 16-row bundles of csr_group_kernel without the flag
    'linear-below-members': (lambda rng: _linear(rng, 250, 2057), ['csr_group_kernel'], 'csr_big_group_kernel'),
    'linear-70x1031': (lambda rng: _linear(rng, 70, 1031), ['csr_group_kernel'], 'csr_big_group_kernel'),
    'small-groups': (_small_groups, ['csr_group_kernel'], None),
    'pool-loose': (_pool, ['csr_rows_kernel'], 'csr_group_kernel'),
    'long-row': (_long, ['csr_big_group_kernel'], None),
    'patched': (_patched, ['csr_patch_guard_kernel<1 patched rows>'], None),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(operator handle, (shape, indptr, indices, data), X [cols, 8], oracle result [rows, 8]) -- built once, left unchanged."""
    rng = np.random.RandomState(sum(map(ord, name)))
    made = CASES[name][0](rng)
    (shape, ip, ix, dt) = made[:4]
    with torch.cuda.device(dev()):
        op = _capi.Operator.csr(shape, ip, ix, dt)
    X = rng.uniform(-2, 2, (shape[1], 8)).astype(np.float32)
    return (op, (shape, ip, ix, dt), X, _ref((shape, ip, ix, dt), X), made[4:])


def _ref(csr, X):
    with np.errstate(all='ignore'):
        return oracle.csr_matvecs(csr[0], csr[1], csr[2], csr[3], np.ascontiguousarray(X))


def _relu(r):
    return np.where(r < 0, np.float32(0), r)                            # torch relu: NaN stays NaN


def _nv(n):
    return 1 if n == 1 else 2 if n == 2 else 4 if n <= 4 else 8


@pytest.mark.parametrize('name', sorted(CASES))
def test_kernel_against_the_oracle(name):
    """Every width 1 .. 8, with and without ReLU: np.array_equal with oracle.csr_matvecs in stored order, torch.equal with the same call without the flag; the plan
    names the kernel, NV and the rows-per-wavefront form, and keeps the long-row and patch-guard launches of the call without the flag."""
    (op, csr, X, ref, _) = _case(name)
    (without, gone) = CASES[name][1:]
    for n in range(1, 9):
        xd = torch.as_tensor(np.ascontiguousarray(X[:, :n])).to(dev())
        for relu in (0, RELU):
            (y, _, plan) = _spmm(op, xd, n, EXACT | ROWS | relu)
            (y0, _, plan0) = _spmm(op, xd, n, EXACT | relu)
            assert KERNEL not in plan0 and all(w in plan0 for w in without), plan0
            if name == 'linear-big' and n > 2:                          # the handle rule (test_the_shapes_that_keep_their_kernels): same plan, and below the same bits
                assert plan == plan0, (plan, plan0)
            else:
                assert KERNEL in plan and 'nv=%d' % _nv(n) in plan and 'rows=64' in plan, plan
            if name in ('long-row', 'patched'):
                assert without[0].split('<')[0] in plan, plan           # the long role and the patch guard are launched as today
            if gone:
                assert gone not in plan, plan
            r = _relu(ref[:, :n]) if relu else ref[:, :n]
            assert np.array_equal(y.cpu().numpy(), r), (name, n, relu, int(np.sum(y.cpu().numpy() != r)))
            assert torch.equal(y, y0), (name, n, relu)
    if name == 'linear-big':                                            # 262 rows = four whole 64-row chunks and a partly filled one, plus the homogeneous row
        assert '5 group chunks, 1 loose rows' in _spmm(op, xd[:, :2].contiguous(), 2, EXACT | ROWS)[2]


@pytest.mark.parametrize('name', ['linear-big', 'small-groups', 'pool-loose', 'patched'])
def test_column_window_of_a_wider_block(name):
    """ldx = ldy = 13 > n_vecs, the window starts at column 3: the result is the compact call's, nothing is stored outside the window."""
    (op, csr, X, ref, _) = _case(name)
    rng = np.random.RandomState(5)
    for n in (1, 3, 5, 8):
        wide = rng.uniform(-9, 9, (X.shape[0], 13)).astype(np.float32)
        wide[:, 3:3 + n] = X[:, :n]
        (y, whole, plan) = _spmm(op, torch.as_tensor(wide).to(dev()), n, EXACT | ROWS | RELU, ld=13, start=3)
        assert KERNEL in plan or (name == 'linear-big' and n > 2), plan
        assert np.array_equal(y.cpu().numpy(), _relu(ref[:, :n])), (name, n)
        whole = whole.clone()
        whole[:, 3:3 + n] = SENTINEL
        assert bool(torch.all(whole == SENTINEL)), (name, n, 'a store outside the window')


@pytest.mark.parametrize('name', ['linear-70x1031', 'small-groups', 'pool-loose', 'long-row', 'patched'])
def test_non_finite_activations(name):
    """Inf and NaN at chosen rows of X: the oracle's result, NaN positions equal.  The patched row meets +Inf at its MISSING column: 0 * Inf would leak a NaN the
    reference's row does not have; the guard kernel behind the row-lane kernel rewrites it."""
    (op, csr, X, _, extra) = _case(name)
    X = X.copy()
    hit = np.unique(csr[2])[::7][:6]                                    # columns some row really holds
    X[hit[0], 0] = np.inf
    X[hit[1], 1] = -np.inf
    X[hit[2], 2] = np.nan
    X[hit[3], :] = np.inf
    runs = [X]
    if extra:                                                           # ... and a block that is non-finite ONLY at the patched row's missing column
        Xp = _case(name)[2].copy()
        Xp[extra[0], 0] = np.inf
        Xp[extra[0], 2] = np.nan
        runs.append(Xp)
        prow = csr[0][0] - 2                                             # the patched row: finite in the reference although its group saw +Inf
        assert np.isfinite(_ref(csr, Xp[:, :1])[prow, 0]) and not np.isfinite(_ref(csr, Xp[:, :1])[0, 0])
    for (X, n) in [(Xr, n) for Xr in runs for n in (1, 3, 8)]:
        ref = _ref(csr, X[:, :n])
        for relu in (0, RELU):
            (y, _, plan) = _spmm(op, torch.as_tensor(np.ascontiguousarray(X[:, :n])).to(dev()), n, EXACT | ROWS | relu)
            assert KERNEL in plan
            r = _relu(ref) if relu else ref
            assert np.array_equal(y.cpu().numpy(), r, equal_nan=True), (name, n, relu)


def test_flag_semantics():
    """Where the flag is ignored the plan string and the bits are those of the call without it: nine columns, a conv-taps handle, a float64 handle, kn_spmm_planes.
    KN_FLAG_NARROW next to it changes nothing; kn_spmm_screen raises the slot to max |y|."""
    (op, csr, X, ref, _) = _case('small-groups')
    rng = np.random.RandomState(11)
    x9 = torch.as_tensor(rng.uniform(-2, 2, (X.shape[0], 9)).astype(np.float32)).to(dev())
    (y, _, plan) = _spmm(op, x9, 9, EXACT | ROWS)
    (y0, _, plan0) = _spmm(op, x9, 9, EXACT)
    assert plan == plan0 and KERNEL not in plan and torch.equal(y, y0)
    x8 = torch.as_tensor(X).to(dev())
    for n in (1, 5, 8):
        (ya, _, pa) = _spmm(op, x8[:, :n].contiguous(), n, ROWS | NARROW)
        (yb, _, pb) = _spmm(op, x8[:, :n].contiguous(), n, ROWS)
        (yc, _, pc) = _spmm(op, x8[:, :n].contiguous(), n, ROWS | NARROW | MFMA | EXACT)
        assert pa == pb == pc and KERNEL in pa and torch.equal(ya, yb) and torch.equal(ya, yc)
        (yn, _, pn) = _spmm(op, x8[:, :n].contiguous(), n, NARROW)      # the conv flags alone stay ignored by a CSR handle
        assert KERNEL not in pn and pn == _spmm(op, x8[:, :n].contiguous(), n, 0)[2] and torch.equal(yn, ya)
    # the screen: the library's reduction pass over Y
    for name in ('small-groups', 'pool-loose'):
        (o2, _, X2, r2, _) = _case(name)
        slot = torch.zeros(1, dtype=torch.float32, device=dev())
        (ys, _, ps) = _spmm(o2, torch.as_tensor(np.ascontiguousarray(X2[:, :3])).to(dev()), 3, EXACT | ROWS, absmax=slot)
        assert KERNEL in ps and float(slot.item()) == float(np.abs(r2[:, :3]).max()) and np.array_equal(ys.cpu().numpy(), r2[:, :3])
    # a conv-taps handle
    (W, M, Xc, _) = _build(('rows-on-conv', 5, 24, 6, 3, 1, True, True), seed=3)
    xc = torch.as_tensor(np.ascontiguousarray(Xc[:, :3])).to(dev())
    with torch.cuda.device(dev()):
        cop = W._device_op(dev())
    for fl in (NARROW, EXACT, MFMA):
        (y1, _, p1) = _spmm(cop, xc, 3, fl | ROWS)
        (y2, _, p2) = _spmm(cop, xc, 3, fl)
        assert p1 == p2 and KERNEL not in p1 and torch.equal(y1, y2), (fl, p1, p2)
    # a float64 handle
    (shape, ip, ix, dt) = csr
    with torch.cuda.device(dev()):
        f64 = _capi.Operator.csr(shape, ip, ix, dt.astype(np.float64))
        assert f64.plan(3, EXACT | ROWS) == f64.plan(3, EXACT) and KERNEL not in f64.plan(3, EXACT | ROWS)
        x3 = x8[:, :3].contiguous()
        outs = []
        for fl in (EXACT | ROWS, EXACT):
            y = torch.zeros((shape[0], 3), dtype=torch.float64, device=dev())
            f64.spmm_f64(x3.data_ptr(), 3, 3, y.data_ptr(), 3, fl, torch.cuda.current_stream().cuda_stream)
            outs.append(y)
        assert torch.equal(outs[0], outs[1])
        # kn_spmm_planes: two planes of three columns
        xp = torch.as_tensor(rng.uniform(-2, 2, (2, shape[1], 3)).astype(np.float32)).to(dev())
        outs = []
        for fl in (EXACT | ROWS, EXACT):
            y = torch.full((2, shape[0], 3), SENTINEL, dtype=torch.float32, device=dev())
            assert op.spmm_planes(xp.data_ptr(), 3, shape[1] * 3, 2, 3, y.data_ptr(), 3, shape[0] * 3, fl, torch.cuda.current_stream().cuda_stream)
            outs.append(y)
        assert torch.equal(outs[0], outs[1])
        for k in range(2):                                              # ... which is the per-plane product (no plan string exists for this entry point)
            assert np.array_equal(outs[0][k].cpu().numpy(), _ref(csr, xp[k].cpu().numpy()))


@pytest.mark.parametrize('side', ['last', 'first-beyond'])
def test_offset_guard(side):
    """cols * ldx + 8 < 2^30 (the kernel keeps 32-bit BYTE offsets into X): 1 031 columns; the last leading dimension inside runs the row-lane kernel on a window at
    the end of every row of one shared 4 GiB buffer, the first beyond falls back to the kernels of the call without the flag -- the same plan, the same bits."""
    with torch.cuda.device(dev()):
        if torch.cuda.mem_get_info()[0] < 8 * (1 << 30):
            pytest.skip('needs 8 GB of free device memory')
    (op, csr, X, ref, _) = _case('linear-70x1031')
    cols = csr[0][1]
    last = ((1 << 30) - 9) // cols
    assert cols * last + 8 < (1 << 30) <= cols * (last + 1) + 8
    ldx = last if side == 'last' else last + 1
    n = 3
    buf = torch.full((cols * ldx,), float('nan'), dtype=torch.float32, device=dev())
    win = buf.view(cols, ldx)[:, ldx - n:]
    win.copy_(torch.as_tensor(np.ascontiguousarray(X[:, :n])))
    assert (cols - 1) * ldx * 4 > (1 << 31)                             # the last rows are reached only with byte offsets beyond 2^31
    outs = []
    for fl in (EXACT | ROWS | RELU, EXACT | RELU):
        y = torch.full((csr[0][0], n), SENTINEL, dtype=torch.float32, device=dev())
        with torch.cuda.device(dev()):
            op.spmm(buf.data_ptr() + 4 * (ldx - n), ldx, n, y.data_ptr(), n, fl, torch.cuda.current_stream().cuda_stream)
            outs.append((y, op.plan(n, fl, ldx=ldx, ldy=n)))
    torch.cuda.synchronize()
    print(side, ldx, outs[0][1])
    assert (KERNEL in outs[0][1]) == (side == 'last') and KERNEL not in outs[1][1]
    if side != 'last':
        assert outs[0][1] == outs[1][1]
    assert torch.equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][0].cpu().numpy(), _relu(ref[:, :n]))
    del buf, win
    torch.cuda.empty_cache()


def test_operators_with_long_loose_rows_keep_the_row_kernel_for_them():
    """The handle rule (kn_internal.h, narrow_rows_loose): a lane walks a loose row with nothing else in flight, so an operator whose longest loose row holds more
    than 64 entries keeps csr_rows_kernel for its loose rows; its pattern groups still take the row-lane kernel.  Both sides of the threshold, bit for bit."""
    for (longest, lanes) in ((64, True), (65, False)):
        rng = np.random.RandomState(longest)
        n = 400
        rows = [rng.permutation(n)[:30].astype(np.int32)] * 20 + [rng.randint(0, n, int(k)).astype(np.int32) for k in rng.randint(0, 20, 50)]
        rows.append(rng.randint(0, n, longest).astype(np.int32))
        csr = _csr(rows, n, rng)
        with torch.cuda.device(dev()):
            op = _capi.Operator.csr(*csr)
        X = rng.uniform(-2, 2, (n, 5)).astype(np.float32)
        (y, _, plan) = _spmm(op, torch.as_tensor(X).to(dev()), 5, EXACT | ROWS)
        assert KERNEL in plan and ('csr_rows_kernel' in plan) == (not lanes), plan
        assert (' 0 loose rows' in plan) == (not lanes), plan
        assert np.array_equal(y.cpu().numpy(), _ref(csr, X))


def test_the_shapes_that_keep_their_kernels():
    """The handle rule (kn_internal.h, narrow_rows_loses; measured on VGG-16's fc6 - fc8, profiles/r09_narrow_rows.txt): an operator with a keyed Linear's big pattern
    group (>= 256 rows over >= 2 048 shared columns) takes the row-lane kernel at 1 and 2 columns only; beyond, the flag is ignored -- the plan and the bits of the call
    without it.  The same pattern below either big-group threshold keeps the kernel at every width."""
    rng = np.random.RandomState(7)
    for (members, ncol, widest) in ((262, 2057, 2), (256, 2048, 2), (255, 2057, 8), (262, 2047, 8)):
        csr = _linear(rng, members, ncol)
        with torch.cuda.device(dev()):
            op = _capi.Operator.csr(*csr)
        X = rng.uniform(-2, 2, (ncol, 8)).astype(np.float32)
        ref = _ref(csr, X)
        for n in (1, 2, 3, 4, 5, 8):
            xd = torch.as_tensor(np.ascontiguousarray(X[:, :n])).to(dev())
            (y, _, plan) = _spmm(op, xd, n, EXACT | ROWS)
            (y0, _, plan0) = _spmm(op, xd, n, EXACT)
            assert (KERNEL in plan) == (n <= widest), (members, ncol, n, plan)
            if n > widest:
                assert plan == plan0
            assert torch.equal(y, y0) and np.array_equal(y.cpu().numpy(), ref[:, :n]), (members, ncol, n)


# ---- whole key-nets ---------------------------------------------------------------------------------------------------------------------------------------
def _rows_layers(knet):
    """Layers whose operator is a float32 CSR handle run in the stored order under the contract in force."""
    out = []
    for (name, c) in knet._keyed(named=True):
        la = c.launch(dev(), narrow=True, narrow_rows=True)
        if la is not None and la.flags & ROWS:
            out.append(name)
    return out


@pytest.mark.parametrize('name', ['mini_tiled_permutation.npz', 'mini_tiled_permutation8.npz', 'mini_tiled_stochastic.npz', 'lenet_perm.npz'])
def test_whole_keynets(golden, name):
    z = golden(name)
    knet = kio.keynet_from_arrays(z)
    x = torch.as_tensor(z['x_cipher'][np.arange(8) % z['x_cipher'].shape[0]]).to(dev())
    knet.forward_linear(torch.as_tensor(z['x_cipher']).to(dev()))        # the loaded contract decides itself on the golden batch
    cases = [(mode, n) for mode in (True, 'mfma') for n in (1, 3, 8)]
    plain = [knet.forward_linear(x[:n], narrow=mode) for (mode, n) in cases]      # (a calibrated layer measures its narrow='mfma' record here, without the keyword)
    before = copy.deepcopy(knet.contract_report())
    plans = (dict(knet.__dict__.get('_overlap_plans', {})), dict(knet.__dict__.get('_chain_ops', {})))
    knet._padded_forwards = 0
    assert _rows_layers(knet), 'no layer of %s would take the row-lane kernel' % name
    for ((mode, n), y0) in zip(cases, plain):
        assert torch.equal(knet.forward_linear(x[:n], narrow=mode, narrow_rows=True), y0), (name, mode, n)
    assert tuple(knet.forward(x[:1], narrow=True, narrow_rows=True).shape) == tuple(knet._outshape)
    assert knet.contract_report() == before
    assert (dict(knet.__dict__.get('_overlap_plans', {})), dict(knet.__dict__.get('_chain_ops', {}))) == plans
    assert knet._padded_forwards == 0
    for bad in (lambda: knet.forward_linear(x[:2], narrow_rows=True), lambda: knet.forward_linear(torch.cat([x, x])[:9], narrow=True, narrow_rows=True),
                lambda: knet.capture(x[:2], narrow_rows=True), lambda: knet.capture(torch.cat([x, x])[:9], narrow=True, narrow_rows=True)):
        with pytest.raises(ValueError):
            bad()
    knet.exact_mode(True)
    xg = torch.as_tensor(z['x_cipher']).to(dev())
    out = torch.cat([knet.forward_linear(xg[lo:lo + 8], narrow=True, narrow_rows=True) for lo in range(0, xg.shape[0], 8)]).cpu().numpy()
    print(name, 'max |narrow_rows - reference| =', float(np.abs(out - _last(z)).max()))
    assert np.array_equal(out, _last(z))
    assert knet._padded_forwards == 0


@pytest.mark.parametrize('n', [1, 3, 8])
def test_what_the_forward_issues(golden, monkeypatch, n):
    """The kn_spmm calls forward_linear(x[:n], narrow=True, narrow_rows=True) ISSUES: every stored-order f32 CSR layer's call carries KN_FLAG_NARROW_ROWS and plans
    to the new kernel, the conv calls are those of the forward without the keyword, and without the keyword no call carries the flag."""
    z = golden('mini_tiled_permutation8.npz')
    knet = kio.keynet_from_arrays(z)
    knet.exact_mode(True)
    x = torch.as_tensor(z['x_cipher'][np.arange(8) % z['x_cipher'].shape[0]]).to(dev())[:n]
    knet.forward_linear(x, narrow=True, narrow_rows=True)                # operators resident
    rows_layers = _rows_layers(knet)
    convs = [nm for (nm, c) in knet._keyed(named=True) if isinstance(c.W, ksp.Conv2dTiledMatrix)]
    assert rows_layers and convs and len(rows_layers) + len(convs) == len(knet._keyed())
    calls = _spmm_calls(monkeypatch)
    y = knet.forward_linear(x, narrow=True, narrow_rows=True)
    with_rows = list(calls)
    del calls[:]
    y0 = knet.forward_linear(x, narrow=True)
    without = list(calls)
    assert torch.equal(y, y0)
    assert len(with_rows) == len(without) >= len(rows_layers) + len(convs)
    assert sum(1 for (p, f) in with_rows if f & ROWS and KERNEL in p) == len(rows_layers), with_rows
    assert all(bool(f & ROWS) == (KERNEL in p) for (p, f) in with_rows), with_rows
    assert [c for c in with_rows if not c[1] & ROWS] == [c for c in without if 'convtaps' in c[0]], (with_rows, without)
    assert not any(f & ROWS or KERNEL in p for (p, f) in without), without


def test_capture(golden):
    """capture(x[:4], narrow=True, narrow_rows=True) replayed on two different inputs equals the eager forward each time."""
    z = golden('mini_tiled_permutation.npz')
    knet = kio.keynet_from_arrays(z)
    knet.exact_mode(True)
    x = torch.as_tensor(z['x_cipher']).to(dev())
    replay = knet.capture(x[:4], narrow=True, narrow_rows=True)
    other = (x[:4].flip(0) * 0.5).contiguous()
    for xi in (x[:4], other):
        eager = knet.forward_linear(xi, narrow=True, narrow_rows=True)
        assert torch.equal(replay(xi).clone(), eager)
        assert torch.equal(eager, knet.forward_linear(xi, narrow=True))
    assert not torch.equal(knet.forward_linear(other, narrow=True, narrow_rows=True), knet.forward_linear(x[:4], narrow=True, narrow_rows=True))
    assert getattr(replay, 'graph', None) is not None


def test_fuzz_random_csr_operators():
    """Seeded: 40 random CSR operators mixing the roles (pattern groups of random height and length, ragged loose rows with empties and repeats, now and then a long
    row and a patched row), each at a random width, ReLU and column window, against the oracle."""
    rng = np.random.RandomState(20261)
    for it in range(40):
        n_cols = int(rng.randint(40, 1500))
        rows = []
        for _ in range(int(rng.randint(0, 6))):
            ncol = int(rng.choice([1, 9, 28, 47, 48, 49, 97, 200]))
            pattern = rng.randint(0, n_cols, ncol).astype(np.int32)
            rows += [pattern] * int(rng.choice([2, 8, 15, 16, 17, 63, 64, 65, 130]))
        if rng.rand() < 0.3:
            pattern = np.sort(rng.permutation(n_cols)[:36]).astype(np.int32)
            rows += [pattern] * 9 + [np.delete(pattern, int(rng.randint(0, 36)))]
        rows += [rng.randint(0, n_cols, int(k)).astype(np.int32) for k in rng.randint(0, 14, int(rng.randint(1, 90)))]
        if rng.rand() < 0.2:
            rows.append(rng.randint(0, n_cols, int(rng.randint(1024, 1200))).astype(np.int32))
        order = rng.permutation(len(rows))
        csr = _csr([rows[i] for i in order], n_cols, rng)
        n = int(rng.randint(1, 9))
        relu = RELU if rng.rand() < 0.5 else 0
        (ld, start) = (n, 0) if rng.rand() < 0.5 else (n + int(rng.randint(1, 9)), 1)
        X = rng.uniform(-2, 2, (n_cols, ld)).astype(np.float32)
        with torch.cuda.device(dev()):
            op = _capi.Operator.csr(*csr)
        (y, _, plan) = _spmm(op, torch.as_tensor(X).to(dev()), n, EXACT | ROWS | relu, ld=None if ld == n else ld, start=start if ld != n else 0)
        assert KERNEL in plan, plan
        ref = _ref(csr, X[:, (start if ld != n else 0):(start if ld != n else 0) + n])
        assert np.array_equal(y.cpu().numpy(), _relu(ref) if relu else ref), (it, n, relu, ld, plan)
