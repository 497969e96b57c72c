"""The LDS value-stream form of a keyed Linear for 1 .. 64 images on the GPU: csr_stream_group_kernel (KN_FLAG_NARROW_LINEAR: a workgroup owns 64 member rows of a
big pattern group times all batch columns, the values reach its wavefronts through a ring in LDS) against the CPU oracle in stored order, bit for bit; the flag's
semantics through the C ABI; and KeyedModel.forward_linear / capture with narrow_linear=True."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import oracle
from keynet_amd import io as kio
from keynet_amd import sparse as ksp
from keynet_amd import system as ksys
from keynet_amd import _capi
from nets import _Chain
from test_parity_gpu import dev
from test_narrow_gpu import _build
from test_narrow_rows_gpu import _csr, _linear, _ref, _relu
from narrow_helpers import SENTINEL, _spmm, _spmm_calls

pytestmark = pytest.mark.gpu

(RELU, EXACT, NARROW, MFMA, ROWS, LINEAR) = (_capi.KN_FLAG_RELU, _capi.KN_FLAG_EXACT, _capi.KN_FLAG_NARROW, _capi.KN_FLAG_NARROW_MFMA, _capi.KN_FLAG_NARROW_ROWS,
                                             _capi.KN_FLAG_NARROW_LINEAR)
KERNEL = 'csr_stream_group_kernel'
WIDTHS = list(range(1, 9)) + [9, 15, 16, 17, 31, 32, 33, 48, 63, 64]      # every form, the widths around each change of form, masked and full
PATCH_POS = 1031


WIDEST = 32           # the handle rule (narrow_linear_loses, kn_internal.h): beyond, an operator with big groups keeps the kernels it has


def _form(n):
    """(W, NV) of a width: the fewest running sums per lane that eight wavefronts allow (stream_form, kn_internal.h)."""
    assert n <= WIDEST
    nv = 1 if n <= 8 else 2 if n <= 16 else 4
    per = -(-n // nv)
    return (1 if per <= 1 else 2 if per <= 2 else 4 if per <= 4 else 8, nv)


def _two_groups(rng):
    """Two big groups of different height and length (256 x 2 048 unsorted, 300 x 2 100 sorted), their rows interleaved, between pool-like loose rows (an empty one
    among them) and the homogeneous row."""
    n = 2200
    (pa, pb) = (rng.permutation(n)[:2048].astype(np.int32), np.sort(rng.permutation(n)[:2100]).astype(np.int32))
    rows = [pa] * 256 + [pb] * 300 + [rng.randint(0, n, int(k)).astype(np.int32) for k in rng.randint(0, 12, 40)]
    rows[556] = np.zeros(0, np.int32)
    order = rng.permutation(len(rows))
    return _csr([rows[i] for i in order] + [np.array([n - 1], np.int32)], n, rng)


def _patched(rng):
    """A big group of 262 rows over 2 057 sorted columns and a 263rd row that lost entry PATCH_POS to an exact zero: it rides in the group with 0.0f there,
    csr_patch_guard_kernel covers it.  Then the homogeneous row."""
    n = 2300
    pattern = np.sort(rng.permutation(n)[:2057]).astype(np.int32)
    return _csr([pattern] * 262 + [np.delete(pattern, PATCH_POS)] + [np.array([n - 1], np.int32)], n, rng) + (int(pattern[PATCH_POS]),)


CASES = {
    # 262 = four whole 64-row chunks and one of 6; 2 057 >= the 2 048 threshold and no multiple of a slab (16 | 32 steps), a scalar batch or the ring
    'linear-big': (lambda rng: _linear(rng, 262, 2057), 5),
    'threshold': (lambda rng: _linear(rng, 256, 2048), 4),
    'two-groups': (_two_groups, 4 + 5),
    'patched': (_patched, 5),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(operator handle, (shape, indptr, indices, data), X [cols, 64], oracle result [rows, 64], extras) -- built once, left unchanged."""
    rng = np.random.RandomState(sum(map(ord, name)))
    made = CASES[name][0](rng)
    csr = made[:4]
    with torch.cuda.device(dev()):
        op = _capi.Operator.csr(*csr)
    X = rng.uniform(-2, 2, (csr[0][1], 64)).astype(np.float32)
    return (op, csr, X, _ref(csr, X), made[4:])


def _plan_names_the_form(plan, n, chunks):
    (w, nv) = _form(n)
    assert KERNEL in plan and 'W=%d,NV=%d' % (w, nv) in plan and '%d chunks of 64 rows' % chunks in plan and 'ring of' in plan, plan
    assert ('masked to %d' % n in plan) == (w * nv != n), plan


@pytest.mark.parametrize('name', sorted(CASES))
def test_kernel_against_the_oracle(name):
    """Every form and the widths around it, with and without ReLU: np.array_equal with oracle.csr_matvecs in stored order, torch.equal with the same call without
    the flag; the plan names the kernel, W, NV, the chunks and the ring; csr_big_group_kernel is gone, the patch guard stays.  Beyond 32 columns the measured handle
    rule keeps the kernels of the call without the flag: the same plan string, and below the same bits."""
    (op, csr, X, ref, _) = _case(name)
    for n in WIDTHS:
        xd = torch.as_tensor(np.ascontiguousarray(X[:, :n])).to(dev())
        for relu in (0, RELU):
            (y, _, plan) = _spmm(op, xd, n, EXACT | LINEAR | relu)
            (y0, _, plan0) = _spmm(op, xd, n, EXACT | relu)
            assert KERNEL not in plan0 and 'csr_big_group_kernel' in plan0, plan0
            if n > WIDEST:
                assert plan == plan0, (plan, plan0)
            else:
                _plan_names_the_form(plan, n, CASES[name][1])
                assert 'csr_big_group_kernel' not in plan and 'mfma16' not in plan, plan
            assert ('csr_patch_guard_kernel<1 patched rows>' in plan) == (name == 'patched'), plan
            r = _relu(ref[:, :n]) if relu else ref[:, :n]
            got = y.cpu().numpy()
            assert np.array_equal(got, r), (name, n, relu, int(np.sum(got != r)))
            assert torch.equal(y, y0), (name, n, relu)


@pytest.mark.parametrize('name', ['linear-big', 'two-groups', 'patched'])
def test_column_window_of_a_wider_block(name):
    """ldx = ldy = 70 > n_vecs, the window starts at column 3: the result is the compact call's, nothing is stored outside the window."""
    (op, csr, X, ref, _) = _case(name)
    rng = np.random.RandomState(5)
    for n in (1, 5, 17, 32, 33, 64):
        wide = rng.uniform(-9, 9, (X.shape[0], 70)).astype(np.float32)
        wide[:, 3:3 + n] = X[:, :n]
        (y, whole, plan) = _spmm(op, torch.as_tensor(wide).to(dev()), n, EXACT | LINEAR | RELU, ld=70, start=3)
        assert (KERNEL in plan) == (n <= WIDEST), plan
        assert np.array_equal(y.cpu().numpy(), _relu(ref[:, :n])), (name, n)
        whole = whole.clone()
        whole[:, 3:3 + n] = SENTINEL
        assert bool(torch.all(whole == SENTINEL)), (name, n, 'a store outside the window')


@pytest.mark.parametrize('name', ['linear-big', 'two-groups', 'patched'])
def test_non_finite_activations(name):
    """Inf and NaN at chosen rows of X: the oracle's result, NaN positions equal.  The patched row meets +Inf at its MISSING column: 0 * Inf would leak a NaN the
    reference's row does not have; the guard kernel behind the value-stream kernel rewrites it."""
    (op, csr, X, _, extra) = _case(name)
    X = X.copy()
    hit = np.unique(csr[2])[::7][:6]                                    # columns some row really holds
    X[hit[0], 0] = np.inf
    X[hit[1], 1] = -np.inf
    X[hit[2], 2] = np.nan
    X[hit[3], :] = np.inf
    X[hit[4], 10] = np.nan
    X[hit[5], 30] = -np.inf
    runs = [X]
    if extra:                                                           # ... and a block that is non-finite ONLY at the patched row's missing column
        Xp = _case(name)[2].copy()
        Xp[extra[0], 0] = np.inf
        Xp[extra[0], 2] = np.nan
        Xp[extra[0], 11] = np.inf
        Xp[extra[0], 31] = np.inf
        runs.append(Xp)
        prow = csr[0][0] - 2                                            # the patched row: finite in the reference although its group saw +Inf
        assert np.isfinite(_ref(csr, Xp[:, :1])[prow, 0]) and not np.isfinite(_ref(csr, Xp[:, :1])[0, 0])
    for (Xr, n) in [(Xr, n) for Xr in runs for n in (1, 3, 8, 12, 32, 36, 64)]:
        ref = _ref(csr, Xr[:, :n])
        for relu in (0, RELU):
            (y, _, plan) = _spmm(op, torch.as_tensor(np.ascontiguousarray(Xr[:, :n])).to(dev()), n, EXACT | LINEAR | relu)
            assert (KERNEL in plan) == (n <= WIDEST)
            r = _relu(ref) if relu else ref
            assert np.array_equal(y.cpu().numpy(), r, equal_nan=True), (name, n, relu)


def test_where_the_flag_changes_nothing():
    """The plan string and the bits of the call without the flag: at 65 columns, below either big-group threshold, on a conv-taps handle, on a float64 handle
    (kn_spmm_f64 too), in kn_spmm_planes."""
    (op, csr, X, ref, _) = _case('linear-big')
    rng = np.random.RandomState(11)
    x65 = torch.as_tensor(rng.uniform(-2, 2, (X.shape[0], 65)).astype(np.float32)).to(dev())
    for fl in (EXACT, EXACT | ROWS, EXACT | RELU):
        (y, _, plan) = _spmm(op, x65, 65, fl | LINEAR)
        (y0, _, plan0) = _spmm(op, x65, 65, fl)
        assert plan == plan0 and KERNEL not in plan and torch.equal(y, y0)
    for (members, ncol) in ((255, 2057), (262, 2047)):
        small = _linear(rng, members, ncol)
        with torch.cuda.device(dev()):
            sop = _capi.Operator.csr(*small)
        Xs = rng.uniform(-2, 2, (ncol, 33)).astype(np.float32)
        for n in (1, 2, 5, 8, 33):
            xd = torch.as_tensor(np.ascontiguousarray(Xs[:, :n])).to(dev())
            for fl in (EXACT, EXACT | ROWS):
                (y, _, plan) = _spmm(sop, xd, n, fl | LINEAR)
                (y0, _, plan0) = _spmm(sop, xd, n, fl)
                assert plan == plan0 and KERNEL not in plan and torch.equal(y, y0), (members, ncol, n, fl, plan, plan0)
            assert np.array_equal(y.cpu().numpy(), _ref(small, Xs[:, :n]))
        if members == 255:                                              # kn_spmm_planes (it refuses an operator with big groups): two planes of three columns
            xp = torch.as_tensor(rng.uniform(-2, 2, (2, ncol, 3)).astype(np.float32)).to(dev())
            outs = []
            with torch.cuda.device(dev()):
                for fl in (EXACT | LINEAR, EXACT):
                    y = torch.full((2, members + 1, 3), SENTINEL, dtype=torch.float32, device=dev())
                    assert sop.spmm_planes(xp.data_ptr(), 3, ncol * 3, 2, 3, y.data_ptr(), 3, (members + 1) * 3, fl, torch.cuda.current_stream().cuda_stream)
                    outs.append(y)
            assert torch.equal(outs[0], outs[1])
            for k in range(2):
                assert np.array_equal(outs[0][k].cpu().numpy(), _ref(small, xp[k].cpu().numpy()))
    # a conv-taps handle
    (W, M, Xc, _) = _build(('linear-on-conv', 5, 24, 6, 3, 1, True, True), seed=3)
    xc = torch.as_tensor(np.ascontiguousarray(Xc[:, :3])).to(dev())
    with torch.cuda.device(dev()):
        cop = W._device_op(dev())
    for fl in (NARROW, EXACT, MFMA, 0):
        (y1, _, p1) = _spmm(cop, xc, 3, fl | LINEAR)
        (y2, _, p2) = _spmm(cop, xc, 3, fl)
        assert p1 == p2 and KERNEL not in p1 and torch.equal(y1, y2), (fl, p1, p2)
    # a float64 handle of the big-group operator
    (shape, ip, ix, dt) = csr
    with torch.cuda.device(dev()):
        f64 = _capi.Operator.csr(shape, ip, ix, dt.astype(np.float64))
        assert f64.plan(3, EXACT | LINEAR) == f64.plan(3, EXACT) and KERNEL not in f64.plan(3, EXACT | LINEAR)
        x3 = torch.as_tensor(np.ascontiguousarray(X[:, :3])).to(dev())
        (outs, outs32) = ([], [])
        for fl in (EXACT | LINEAR, EXACT):
            y = torch.zeros((shape[0], 3), dtype=torch.float64, device=dev())
            f64.spmm_f64(x3.data_ptr(), 3, 3, y.data_ptr(), 3, fl, torch.cuda.current_stream().cuda_stream)
            outs.append(y)
            outs32.append(_spmm(f64, x3, 3, fl)[0])
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs32[0], outs32[1])


@pytest.mark.parametrize('name', ['linear-big', 'two-groups'])
def test_next_to_the_row_lane_flag(name):
    """KN_FLAG_NARROW_ROWS next to the flag at 1, 2, 3 and 8 columns: the big groups run the value-stream kernel at every one of them (narrow_linear_loses keeps none),
    the loose rows run what KN_FLAG_NARROW_ROWS alone gives them -- the row-lane kernel at 1 and 2 columns, where the plan of the flag alone names it, and the call's
    other kernels beyond (narrow_rows_loses is untouched) -- and the bits are those of the plain call."""
    (op, csr, X, ref, _) = _case(name)
    loose = csr[0][0] - (262 if name == 'linear-big' else 556)
    for n in (1, 2, 3, 8):
        xd = torch.as_tensor(np.ascontiguousarray(X[:, :n])).to(dev())
        (y, _, plan) = _spmm(op, xd, n, EXACT | ROWS | LINEAR)
        (yl, _, plan_linear) = _spmm(op, xd, n, EXACT | LINEAR)
        (yr, _, plan_rows) = _spmm(op, xd, n, EXACT | ROWS)
        (y0, _, plan0) = _spmm(op, xd, n, EXACT)
        _plan_names_the_form(plan, n, CASES[name][1])
        assert 'csr_big_group_kernel' not in plan, plan
        if n <= 2:
            assert 'csr_narrow_kernel' in plan_rows and 'csr_narrow_kernel' in plan and '0 group chunks, %d loose rows' % loose in plan, (plan, plan_rows)
        else:
            assert plan_rows == plan0 and plan == plan_linear, (plan, plan_linear, plan_rows, plan0)
        for other in (yl, yr, y0):
            assert torch.equal(y, other), (name, n)
        assert np.array_equal(y.cpu().numpy(), ref[:, :n])


def test_screen_and_determinism():
    """kn_spmm_screen with the flag raises the slot to max |y| (the library's reduction pass over Y); two calls on the same block give equal bits."""
    (op, csr, X, ref, _) = _case('two-groups')
    for n in (3, 24):
        xd = torch.as_tensor(np.ascontiguousarray(X[:, :n])).to(dev())
        slot = torch.zeros(1, dtype=torch.float32, device=dev())
        (ys, _, ps) = _spmm(op, xd, n, EXACT | LINEAR, absmax=slot)
        assert KERNEL in ps and float(slot.item()) == float(np.abs(ref[:, :n]).max()) and np.array_equal(ys.cpu().numpy(), ref[:, :n])
        again = _spmm(op, xd, n, EXACT | LINEAR)[0]
        assert torch.equal(ys, again)


def test_block_beyond_2_31_bytes():
    """The kernel forms every address into X in 64 bits, so it has no offset rule (csr_narrow_kernel's is cols * ldx + 8 < 2^30): 2 057 columns at the first leading
    dimension beyond that rule, a window at the end of every row of one shared 4 GiB buffer -- the kernel runs, the bits are those of the call without the flag."""
    with torch.cuda.device(dev()):
        if torch.cuda.mem_get_info()[0] < 8 * (1 << 30):
            pytest.skip('needs 8 GB of free device memory')
    (op, csr, X, ref, _) = _case('linear-big')
    cols = csr[0][1]
    ldx = ((1 << 30) - 9) // cols + 1
    assert cols * ldx + 8 >= (1 << 30) and (cols - 1) * ldx * 4 > (1 << 31)      # the last rows are reached only with byte offsets beyond 2^31
    buf = torch.full((cols * ldx,), float('nan'), dtype=torch.float32, device=dev())
    for n in (2, 31):
        win = buf.view(cols, ldx)[:, ldx - n:]
        win.copy_(torch.as_tensor(np.ascontiguousarray(X[:, :n])))
        outs = []
        for fl in (EXACT | ROWS | LINEAR | RELU, EXACT | RELU):
            y = torch.full((csr[0][0], n), SENTINEL, dtype=torch.float32, device=dev())
            with torch.cuda.device(dev()):
                op.spmm(buf.data_ptr() + 4 * (ldx - n), ldx, n, y.data_ptr(), n, fl, torch.cuda.current_stream().cuda_stream)
                outs.append((y, op.plan(n, fl, ldx=ldx, ldy=n)))
        torch.cuda.synchronize()
        print(ldx, n, outs[0][1])
        assert KERNEL in outs[0][1] and KERNEL not in outs[1][1] and 'csr_narrow_kernel' not in outs[0][1]      # (the row-lane kernel's rule sends the loose row back)
        assert torch.equal(outs[0][0], outs[1][0])
        assert np.array_equal(outs[0][0].cpu().numpy(), _relu(ref[:, :n]))
        win.fill_(float('nan'))
    del buf, win
    torch.cuda.empty_cache()


# ---- whole key-nets ---------------------------------------------------------------------------------------------------------------------------------------
class LinearNet(_Chain):
    """The smallest net whose first Linear is keyed into a big pattern group: 256 + 1 rows over 2 048 + 1 shared columns."""
    flatten_before = 'fc1'

    def __init__(self):
        super(LinearNet, self).__init__()
        self.conv1 = nn.Conv2d(1, 8, 3, stride=1, padding=1)
        self.relu1 = nn.ReLU()
        self.fc1 = nn.Linear(8 * 16 * 16, 256)
        self.relu2 = nn.ReLU()
        self.fc2 = nn.Linear(256, 10)


@functools.lru_cache(maxsize=None)
def _linear_keynet():
    torch.manual_seed(3)
    np.random.seed(3)
    net = LinearNet()
    (sensor, knet) = ksys.PermutationKeynet((1, 16, 16), net)
    knet.exact_mode(True)
    knet.CHAIN = False                   # the launch-per-layer forward: the whole-net kernel takes a key-net this small in ONE launch, with or without the keyword
    x = torch.rand(64, 1, 16, 16)
    xc = sensor.fromtensor(x.to(dev())).encrypt().astensor()
    return (knet, xc)


def _keywords(n):
    return dict(narrow=True, narrow32=n > 8, narrow64=n > 32)


def _linear_layers(knet):
    """Layers whose operator is a float32 CSR handle run in the stored order under the contract in force."""
    out = []
    for (name, c) in knet._keyed(named=True):
        la = c.launch(dev(), narrow=True, narrow_linear=True)
        if la is not None and la.flags & LINEAR:
            out.append(name)
    return out


@pytest.mark.parametrize('n', [1, 3, 8, 16, 33, 64])
def test_whole_keynet_with_a_big_group(monkeypatch, n):
    """Under exact_mode(True): the forward with the keyword is torch.equal to the one without; the recorded kn_spmm calls carry the flag on exactly the stored-order
    CSR layers; the new kernel is in the plan of exactly the layer with the big group; nothing is decided, recorded or planned."""
    (knet, xc) = _linear_keynet()
    x = xc[:n]
    y0 = knet.forward_linear(x, **_keywords(n))
    before = copy.deepcopy(knet.contract_report())
    plans = (dict(knet.__dict__.get('_overlap_plans', {})), dict(knet.__dict__.get('_chain_ops', {})))
    knet._padded_forwards = 0
    layers = _linear_layers(knet)
    assert 'fc1' in layers and 'fc2' in layers, layers
    calls = _spmm_calls(monkeypatch)
    y = knet.forward_linear(x, narrow_linear=True, **_keywords(n))
    with_flag = list(calls)
    del calls[:]
    assert torch.equal(knet.forward_linear(x, **_keywords(n)), y0)
    without = list(calls)
    assert torch.equal(y, y0), n
    assert len(with_flag) == len(without) >= len(knet._keyed())
    assert sum(1 for (p, f) in with_flag if f & LINEAR) == len(layers), with_flag
    big = [(p, f) for (p, f) in with_flag if KERNEL in p]
    if n <= WIDEST:
        assert len(big) == 1 and big[0][1] & LINEAR and '4 chunks of 64 rows' in big[0][0], with_flag  # fc1: 256 rows over 2 049 shared columns (+ the homogeneous row)
    else:                                                               # the handle rule: the flag is carried and ignored, every plan is that of the forward without it
        assert not big and [p for (p, f) in with_flag] == [p for (p, f) in without], with_flag
    if n <= WIDEST:
        (w, nv) = _form(n)
        assert any('W=%d,NV=%d' % (w, nv) in p for (p, f) in with_flag)
    assert not any(f & LINEAR or KERNEL in p for (p, f) in without), without
    assert [(p, f) for (p, f) in with_flag if not f & LINEAR] == [(p, f) for ((p, f), (_, fw)) in zip(without, with_flag) if not fw & LINEAR]
    assert knet.contract_report() == before
    assert (dict(knet.__dict__.get('_overlap_plans', {})), dict(knet.__dict__.get('_chain_ops', {}))) == plans
    assert knet._padded_forwards == 0
    if n == 3:                                                          # next to narrow_rows, and through the whole-net kernel (which the keyword leaves alone): the same bits
        knet.CHAIN = True
        try:
            assert torch.equal(knet.forward_linear(x, narrow=True, narrow_linear=True), y0)
        finally:
            knet.CHAIN = False
        assert torch.equal(knet.forward_linear(x, narrow=True, narrow_rows=True, narrow_linear=True), y0)
        assert tuple(knet.forward(x[:1], narrow=True, narrow_linear=True).shape) == tuple(knet._outshape)


def test_the_keyword_is_a_form_of_the_narrow_forward():
    (knet, xc) = _linear_keynet()
    for bad in (lambda: knet.forward_linear(xc[:2], narrow_linear=True), lambda: knet.forward_linear(xc[:9], narrow=True, narrow_linear=True),
                lambda: knet.forward_linear(torch.cat([xc, xc])[:65], narrow=True, narrow64=True, narrow_linear=True),
                lambda: knet.capture(xc[:2], narrow_linear=True), lambda: knet.capture(xc[:9], narrow=True, narrow_linear=True),
                lambda: knet.forward(xc[:2], narrow_linear=True)):
        with pytest.raises(ValueError):
            bad()
    assert tuple(knet.forward_linear(xc[:9], narrow=True, narrow32=True, narrow_linear=True).shape)[0] == 9


def test_capture():
    """capture(x[:4], narrow=True, narrow_linear=True) replayed on two different inputs equals the eager forward each time."""
    (knet, xc) = _linear_keynet()
    replay = knet.capture(xc[:4], narrow=True, narrow_linear=True)
    other = (xc[4:8] * 0.5).contiguous()
    for xi in (xc[:4], other):
        eager = knet.forward_linear(xi, narrow=True, narrow_linear=True)
        assert torch.equal(replay(xi).clone(), eager)
        assert torch.equal(eager, knet.forward_linear(xi, narrow=True))
    assert not torch.equal(knet.forward_linear(other, narrow=True, narrow_linear=True), knet.forward_linear(xc[:4], narrow=True, narrow_linear=True))
    assert getattr(replay, 'graph', None) is not None


def test_a_keynet_without_a_big_group(golden, monkeypatch):
    """mini_tiled_permutation.npz has no big group: the forward with the keyword equals the forward without it, and every plan string is the same."""
    z = golden('mini_tiled_permutation.npz')
    knet = kio.keynet_from_arrays(z)
    knet.exact_mode(True)
    x = torch.as_tensor(z['x_cipher']).to(dev())[:3]
    y0 = knet.forward_linear(x, narrow=True)
    calls = _spmm_calls(monkeypatch)
    y = knet.forward_linear(x, narrow=True, narrow_linear=True)
    with_flag = list(calls)
    del calls[:]
    knet.forward_linear(x, narrow=True)
    assert torch.equal(y, y0)
    assert [p for (p, f) in with_flag] == [p for (p, f) in calls] and not any(KERNEL in p for (p, f) in with_flag)
    assert any(f & LINEAR for (p, f) in with_flag) and [f & ~LINEAR for (p, f) in with_flag] == [f for (p, f) in calls]
