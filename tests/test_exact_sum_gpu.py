"""The kernels that may re-order a sum, held to the CPU oracle bit for bit on inputs whose sums are exact (tests/exact_sum.py): integer operator values and
activations with sum |a| |x| <= 2^24 per output element, so every product and every partial sum is exact in float32 in any order, any grouping, fused or not, over
any split of K and through the three-way bf16 split.  A dropped or duplicated term, a coefficient applied at the wrong precision, lost low mantissa bits of an operand
or a bias added twice all change an integer below 2^24 and show under value_classes.bits_equal; none of them shows under the conditioned gate or under a
power-of-two scale.  tests/test_exact_sum_host.py checks the premise and these teeth on the host.

Every case asserts the 2^24 condition on the host in float64 (exact_sum.condition: on the expanded operator, on the triple product tap x coefficient x activation
where pairs are hit by several taps), asserts that the plan names the tolerance kernel (a site must not fall back to an order-preserving kernel unnoticed), and
runs the three splits of the bit budget B = floor(log2(2^24 / longest row)): wide activations (B - 2, 2), wide values (2, B - 2), balanced.

Columns.  As in test_value_classes_gpu.py a batch wider than 32 columns holds 29 distinct columns (column c a copy of column c mod 29; 5 for the 32 x 32 pixel
operators of the 64-column tiles): the oracle runs on the distinct ones, every element of the output is compared.

bf16x3.  The three-way split x = hi + mid + lo keeps 8 significant bits per part and the kernel forms six of the nine cross products (kn_conv.hip, head of the
bf16x3 section): it is exact only while lo == 0 on BOTH operands, i.e. while neither has more than 16 significant bits.  Those rows cap either side of a split at 16
bits (exact_sum.BF16X3_CAP; at B = 16 the widest side is 14 bits, so the cap binds on no row today and is there for an operator with shorter rows).

Nothing here is inexact by construction: no site needed the element-wise gate the issue keeps for a reciprocal or a scaled constant in an epilogue."""
import time

import numpy as np
import pytest
import scipy.sparse
import torch
from torch import nn

import exact_sum as xs
import oracle
import value_classes as vc
from keynet_amd import _capi
from keynet_amd import sparse as ksp
from keynet_amd import system as ksys
from keynet_amd.layer import KeyedLayer
from keynet_amd.models import _Chain
from narrow_helpers import _spmm, SENTINEL
from test_parity_gpu import _filled_in_convtaps, _random_convtaps, dev
from test_narrow_split_gpu import _recorded
from test_value_classes_gpu import TOLERANCE_ROWS
import test_conv_choice_gpu as cc
import test_narrow64_mfma_gpu as n64

pytestmark = pytest.mark.gpu

C = _capi
(RELU, EXACT, BF16X3) = (C.KN_FLAG_RELU, C.KN_FLAG_EXACT, C.KN_FLAG_BF16X3)
NMFMA_KERNEL = 'convtaps_narrow_mfma_kernel'
DISTINCT = 29
FULL_FORM_NNZ = 30e6               # up to this many expanded entries sum |a| |x| is formed per element; beyond, its upper bound n_max 2^(p + q) from the operands' maxima
_T0 = [None]


@pytest.fixture(scope='module', autouse=True)
def _wall():
    _T0[0] = time.time()
    yield
    torch.cuda.synchronize()
    print('\ntest_exact_sum_gpu: wall %.1f s' % (time.time() - _T0[0]))
    for k in [k for k in cc._ops if k[2] is not None and k[2][0] == xs.KIND]:
        del cc._ops[k]
    _TILE64.clear()
    torch.cuda.empty_cache()


def _seed(*parts):
    return sum((i + 1) * sum(ord(ch) for ch in str(p)) for (i, p) in enumerate(parts)) % (2 ** 31)


def _columns(n, distinct=DISTINCT):
    return np.arange(n) % (n if n <= 32 else distinct)


def _oracle(csr, X):
    return oracle.csr_matvecs(csr[0], csr[1], csr[2], csr[3], X)


def _longest(csr):
    return int(np.diff(np.asarray(csr[1])).max())


def _check_site(op, csr, Xd, src, n, flags, texts, what, pad=0, exact_too=True, ref_d=None):
    """One launch site on one exact-sum case: the window against the oracle on `csr` under bits_equal with ReLU off and on, the plan texts, the screen slot's bits
    against max |Y|, the sentinel columns beyond the batch, and the same call under KN_FLAG_EXACT."""
    if ref_d is None:
        ref_d = _oracle(csr, Xd)
    assert ref_d.dtype == np.float32 and (ref_d[:, xs.zero_columns(Xd.shape[1])] == 0).any(), what          # the rows that cancel are there
    ref = np.ascontiguousarray(ref_d[:, src])
    xd = torch.as_tensor(np.ascontiguousarray(Xd[:, src])).to(dev())
    flags &= ~RELU
    for relu in (0, RELU):
        r = vc.relu_ref(ref) if relu else ref
        slot = torch.zeros(1, dtype=torch.float32, device=dev())
        (y, whole, plan) = _spmm(op, xd, n, flags | relu, ld=n + pad, absmax=slot)
        for t in texts:
            assert t in plan, (what, t, plan)
        torch.cuda.synchronize()
        vc.assert_bits_equal(y.cpu().numpy(), r, '%s, relu=%d, %s' % (what, relu, plan[:120]))
        vc.assert_bits_equal(slot.cpu().numpy(), np.array([np.abs(r).max()], dtype=np.float32), '%s, relu=%d: screen slot' % (what, relu))
        if pad:
            assert bool((whole[:, n:] == SENTINEL).all()), (what, relu)
        if exact_too:
            (ye, _, pe) = _spmm(op, xd, n, flags | relu | EXACT, ld=n + pad)
            vc.assert_bits_equal(ye.cpu().numpy(), r, '%s, relu=%d, under KN_FLAG_EXACT: %s' % (what, relu, pe[:120]))


# ---- every launch site of the matrix-core and narrow regimes that runs under the tolerance -----------------------------------------------------------------

def _row_id(r):
    return '%s-n%d%s-f%d%s' % (r[0], r[1], '-ldy+%d' % r[2] if r[2] else '', r[3], '-' + r[4] if r[4] else '')


@pytest.mark.parametrize('row', TOLERANCE_ROWS, ids=[_row_id(r) for r in TOLERANCE_ROWS])
def test_launch_site_returns_the_oracles_bits(row):
    """test_conv_choice_gpu.ROWS without its order-preserving rows: matrix-core tiles at each loader and KC, quarter-tile tails, ldy = n + 1, slot groups, the small-K
    pair, bf16x3 at both tile shapes with and without coefficients (either operand capped at 16 significant bits: the module docstring says why), the matrix-core narrow
    kernel at NV = 1 .. 32.  Budgets: 19 bits on the 3-channel operators, 16 on the 16-channel 9-slot ones, 15 on c16-o64-two, 12 on the 70-slot ones."""
    (name, n, pad, flags, switch, text, exact_bits) = row
    assert not exact_bits
    cap = xs.BF16X3_CAP if flags & BF16X3 else None
    for split in xs.SPLITS:
        (op, csr) = cc._operator(name, switch, xs.variant(split, cap))
        B = xs.budget(_longest(csr))
        assert B == xs.budget(cc.OPS[name][3] * cc.OPS[name][0] + 1)
        (p, q) = xs.split_bits(B, split, cap)
        src = _columns(n)
        Xd = xs.activations(csr[0][1], int(src.max()) + 1, True, p, _seed(name, n, split), cin=cc.OPS[name][0])
        what = '%s n=%d flags=%d %s (B=%d: %d-bit activations, %d-bit values)' % (name, n, flags, split, B, p, q)
        worst = xs.condition(csr, Xd, what)
        print('  %s: max sum |a||x| = %.0f' % (what, worst))
        _check_site(op, csr, Xd, src, n, flags, [text], what, pad=pad)


# ---- the 64-column tiles of KN_FLAG_NARROW64_MFMA, against the oracle directly -----------------------------------------------------------------------------

_TILE64 = {}


def _tile64_splits(name):
    """All three splits on the small operators; one (walking through the three by the case's place in the table) on the 32 x 32 pixel ones and on the 81-tap one,
    whose 10^7 .. 10^8 expanded entries cost seconds of host work per split."""
    if '32x32' not in name and '9x9' not in name:
        return xs.SPLITS
    return (xs.SPLITS[sorted(n64.CASES).index(name) % 3],)


def _tile64_case(name, split):
    """(handle, exported CSR, 64 columns of distinct ones, the oracle on the distinct columns, B) -- built once per (case, split) for the three widths."""
    if (name, split) not in _TILE64:
        shape = n64.CASES[name][0]
        W0 = _random_convtaps(np.random.RandomState(sum(map(ord, name))), *shape)
        t = W0._taps
        per_row = xs.longest_row(W0)
        (taps, coef, lastcol) = xs.conv_values(split, t['taps'], t['ent_coef'], t['lastcol'], per_row, _seed(name))
        W = ksp.Conv2dTiledMatrix.fromtaps(W0._inshape, W0._outshape, taps, t['ent_out'], t['ent_in'], t['ent_tap'], coef, lastcol)
        B = xs.budget(per_row + (1 if shape[-1] else 0))
        (p, q) = xs.split_bits(B, split)
        src = _columns(64, 5 if '32x32' in name else DISTINCT)
        Xd = xs.activations(W.shape[1], int(src.max()) + 1, bool(shape[-1]), p, _seed(name, split), cin=shape[0])
        with torch.cuda.device(dev()):
            op = W._device_op(dev())
        (ip, ix, dt) = op.export_csr()
        csr = (op.shape(), ip, ix, dt)
        what = '%s %s' % (name, split)
        if len(dt) <= FULL_FORM_NNZ:
            xs.condition_factored(W, Xd, what)
            xs.condition(csr, Xd, what)
        else:           # the upper bound of the sum from the operands' maxima: every |tap x coef| < 2^q, |x| < 2^p, |bias| < 2^B, at most per_row terms and the bias
            cmax = 1.0 if coef is None else float(np.abs(coef).max())
            assert float(np.abs(taps).max()) * cmax < 2.0 ** q and float(np.abs(Xd).max()) < 2.0 ** p and (lastcol is None or float(np.abs(lastcol).max()) < 2.0 ** B)
            assert per_row * 2.0 ** (p + q) + (2.0 ** B if lastcol is not None else 0) <= xs.LIMIT, what
        _TILE64[(name, split)] = (op, csr, Xd, src, _oracle(csr, Xd), B, W)
    return _TILE64[(name, split)]


@pytest.mark.parametrize('name', sorted(n64.CASES))
def test_64_column_tiles_return_the_oracles_bits(name):
    """The cases of tests/test_narrow64_mfma_gpu.py at 33, 40 and 64 columns under KN_FLAG_NARROW_MFMA | KN_FLAG_NARROW64_MFMA (and the two width bits the tile needs),
    each against the oracle on the handle's exported CSR -- not against the padded matrix-core call, which would share a lost term with it."""
    (shape, mt, kc, loaders) = n64.CASES[name]
    for split in _tile64_splits(name):
        (op, csr, Xd, src, ref_d, B, W) = _tile64_case(name, split)
        for n in (33, 40, 64):
            texts = ['%s<MT=%d,NB=64,KC=%d>' % (n64.KERNEL, mt, kc), loaders if n == 64 else n64.GENERIC]
            _check_site(op, csr, Xd, src[:n], n, n64.TILE64, texts, '%s n=%d %s (B=%d)' % (name, n, split, B), ref_d=ref_d)
        del _TILE64[(name, split)]


# ---- the dense split-K GEMM behind kn_dense_create ---------------------------------------------------------------------------------------------------------

_DENSE = {}


def _dense(split):
    """test_large_offsets_gpu.dense_case()'s operator (1 100 x 1 024 and the affine border) with exact-sum values: that builder takes no value variant."""
    if split not in _DENSE:
        D = xs.dense_values(split, 1100, 1024, seed=7)
        M = scipy.sparse.csr_matrix(D)
        with torch.cuda.device(dev()):
            _DENSE[split] = (C.Operator.dense(D), (M.shape, M.indptr, M.indices, M.data))
    return _DENSE[split]


@pytest.mark.parametrize('n', [4, 200, 256])
def test_dense_split_k_returns_the_oracles_bits(n):
    """Rows of 1 025 entries: B = 13."""
    for split in xs.SPLITS:
        (op, csr) = _dense(split)
        assert _longest(csr) == 1025 and xs.budget(1025) == 13
        (p, q) = xs.split_bits(xs.budget(1025), split)
        src = _columns(n)
        Xd = xs.activations(csr[0][1], int(src.max()) + 1, True, p, _seed('dense', n, split))
        what = 'dense handle n=%d %s' % (n, split)
        xs.condition(csr, Xd, what)
        _check_site(op, csr, Xd, src, n, 0, ['dense_reduce_kernel'], what, exact_too=False)
    if n == 256:
        _DENSE.clear()


# ---- the split application of a filled-in conv -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('Cin,Cout,H,fill,n_vecs,has_last', [(16, 64, 6, 5, 128, True), (3, 40, 8, 3, 100, True), (32, 128, 4, 6, 256, False)])
def test_split_application_returns_the_oracles_bits(monkeypatch, Cin, Cout, H, fill, n_vecs, has_last):
    """test_parity_gpu.test_split_application_of_a_filled_in_conv's three shapes with integer taps, coefficients and biases: the wide route (exact='split') and the
    narrow route (narrow='mfma', narrow_split=True at 1, 8 and 32 images; the cost rule switched off as tests/test_narrow_split_gpu.py does, the recorded calls must
    end on the matrix-core narrow kernel) against the oracle on the FUSED expansion of the same integer terms -- a stored fused value is an exact integer sum, so the
    entry order does not matter.  The condition is formed on the triple product.  Budgets: 14, 17 and 13 bits."""
    monkeypatch.setattr(ksp.Conv2dTiledMatrix, 'NARROW_SPLIT_MIN_GAIN', 0.0)
    W0 = _filled_in_convtaps(np.random.RandomState(Cin + Cout + fill), Cin, Cout, H, fill, has_last)
    for split in xs.SPLITS:
        src = _columns(n_vecs)
        (W, M, Xd, B) = xs.conv_case(W0, split, int(src.max()) + 1, _seed(Cin, Cout, split))
        assert W.split_capable() and B == xs.budget(9 * fill * Cin + (1 if has_last else 0))
        csr = (M.shape, M.indptr, M.indices, M.data.astype(np.float32))
        ref_d = _oracle(csr, Xd)
        assert (ref_d[:, xs.zero_columns(Xd.shape[1])] == 0).any()
        ref = np.ascontiguousarray(ref_d[:, src])
        xd = torch.as_tensor(np.ascontiguousarray(Xd[:, src])).to(dev())
        for relu in (False, True):
            r = vc.relu_ref(ref) if relu else ref
            slot = torch.zeros(1, dtype=torch.float32, device=dev())
            (ys, calls) = _recorded(lambda: W.torchdot(xd, relu=relu, exact='split', absmax=slot))
            assert calls and n64.KERNEL in calls[-1][0], calls               # the channel mixing ran on the matrix cores
            vc.assert_bits_equal(ys.cpu().numpy(), r, 'wide split route %s, relu=%d, B=%d' % (split, relu, B))
            vc.assert_bits_equal(slot.cpu().numpy(), np.array([np.abs(r).max()], dtype=np.float32), 'wide split route %s: slot' % split)
            for n in (1, 8, 32):
                xn = xd[:, :n].contiguous()
                kw = dict(narrow32=True) if n > 8 else {}
                (yn, calls) = _recorded(lambda: W.torchdot(xn, relu=relu, exact='split', narrow='mfma', narrow_split=True, **kw))
                assert len(calls) == 2 and NMFMA_KERNEL in calls[1][0], calls
                vc.assert_bits_equal(yn.cpu().numpy(), np.ascontiguousarray(r[:, :n]), 'narrow split route %s, %d images, relu=%d' % (split, n, relu))
        W.release_narrow_split_workspace()


# ---- the persistent small-K pipeline on enough pixels that every workgroup walks several -------------------------------------------------------------------

@pytest.mark.parametrize('Cin,H,k,stride,n_vecs,unit', [(3, 32, 3, 1, 512, True), (1, 32, 3, 1, 768, False)])
def test_small_k_pipeline_returns_the_oracles_bits(Cin, H, k, stride, n_vecs, unit):
    """Two shapes of test_parity_gpu.test_convtaps_small_k_pipeline (1 024 pixels on 512 persistent workgroups); with coefficients the kernel scales the activation rows
    when it writes them to LDS: coef * x is exact for coef in {1, 2}.  Budgets: 19 bits (28 and 19 entries per row)."""
    W0 = _random_convtaps(np.random.RandomState(100 * Cin + H + n_vecs), Cin, 64, H, k, stride, unit, True)
    for split in xs.SPLITS:
        src = _columns(n_vecs)
        (W, M, Xd, B) = xs.conv_case(W0, split, int(src.max()) + 1, _seed('smallk', Cin, split))
        with torch.cuda.device(dev()):
            op = W._device_op(dev())
        (ip, ix, dt) = op.export_csr()
        csr = (op.shape(), ip, ix, dt)
        xs.condition(csr, Xd, 'small-K pipeline')
        _check_site(op, csr, Xd, src, n_vecs, 0, ['convtaps_smallk_pipe_kernel'], 'small-K pipeline Cin=%d n=%d %s (B=%d)' % (Cin, n_vecs, split, B))


# ---- a whole key-net ---------------------------------------------------------------------------------------------------------------------------------------

class _IntNet(_Chain):
    """conv 3 -> 16, ReLU, conv 16 -> 64, ReLU, a 2 x 2 average pool, Linear.  The keyed pools of this project have odd windows (1 / 9 is no power of two), so the
    pool is written as what it is: a 3 x 3, stride 2 conv whose taps at offsets (0, 0) .. (1, 1) are 2^-2 on the channel diagonal and zero elsewhere."""
    flatten_before = 'fc1'

    def __init__(self):
        super(_IntNet, self).__init__()
        self.conv1 = nn.Conv2d(3, 16, 3, padding=1)
        self.relu1 = nn.ReLU()
        self.conv2 = nn.Conv2d(16, 64, 3, padding=1)
        self.relu2 = nn.ReLU()
        self.conv3 = nn.Conv2d(64, 64, 3, stride=2, padding=1)
        self.fc1 = nn.Linear(64 * 4 * 4, 10)


# (image, conv1, conv2, Linear) significant bits, widest first: the first row whose sums meet the 2^24 condition at every layer on the test's images is taken
NET_WIDTHS = [(5, 3, 3, 2), (5, 3, 2, 2), (4, 3, 2, 2), (4, 2, 2, 2), (4, 2, 2, 1), (3, 2, 2, 1), (3, 2, 1, 1), (2, 1, 1, 1)]
N_IMAGES = 40


def _int_net(widths, seed=5):
    rng = np.random.RandomState(seed)
    net = _IntNet().eval()
    with torch.no_grad():
        for (name, bits) in (('conv1', widths[1]), ('conv2', widths[2]), ('fc1', widths[3])):
            m = getattr(net, name)
            m.weight.copy_(torch.as_tensor(xs.integers(rng, tuple(m.weight.shape), bits).astype(np.float32)))
            m.bias.copy_(torch.as_tensor(xs.integers(rng, tuple(m.bias.shape), bits + 2, zero_share=0.1).astype(np.float32)))
            if name != 'fc1':
                # the tiled conv operator tells its blocks apart by their tiles of channel pair (0, 0) (the reference's rule, Conv2dTiledMatrix.__init__): nine
                # taps of a few bits would hold equal values there and blocks of different taps would share a tile -- a keyed operator that is not the conv
                m.weight[0, 0] = torch.tensor([[1.0, -2.0, 3.0], [-4.0, 5.0, -6.0], [7.0, -8.0, 9.0]])
        w = torch.zeros_like(net.conv3.weight)
        w[torch.arange(64), torch.arange(64), 1:, 1:] = 0.25
        net.conv3.weight.copy_(w)
        net.conv3.bias.zero_()
    x = xs.integers(rng, (N_IMAGES, 3, 8, 8), widths[0], zero_share=0.1).astype(np.float32)
    return (net, torch.as_tensor(x))


def _plain_float64(net, x):
    """[(layer name, its float64 output, max over the elements of sum |a| |x| in units of the output's quantum)] of the plain net, layer by layer on the host."""
    F = torch.nn.functional
    (y, out, quantum) = (x.double(), [], 1.0)
    for (name, m) in net.named_children():
        if isinstance(m, nn.ReLU):
            y = torch.relu(y)
            continue
        (w, b) = (m.weight.detach().double(), m.bias.detach().double())
        if isinstance(m, nn.Conv2d):
            quantum *= float(w.abs()[w != 0].min()) if name == 'conv3' else 1.0
            S = F.conv2d(y.abs(), w.abs(), b.abs(), stride=m.stride, padding=m.padding)
            y = F.conv2d(y, w, b, stride=m.stride, padding=m.padding)
        else:
            y = y.reshape(y.shape[0], -1)
            S = F.linear(y.abs(), w.abs(), b.abs())
            y = F.linear(y, w, b)
        assert bool(torch.all(y / quantum == torch.round(y / quantum)))
        out.append((name, y, float(S.max()) / quantum))
    return out


FORMS = [('padded', N_IMAGES, {}), ('narrow-mfma-1', 1, dict(narrow='mfma')), ('narrow-mfma-8', 8, dict(narrow='mfma')), ('narrow32-16', 16, dict(narrow='mfma', narrow32=True)),
         ('narrow64-mfma-40', 40, dict(narrow='mfma', narrow64='mfma'))]


@pytest.mark.parametrize('mode', [False, 'auto'])
def test_integer_keynet_every_layer_and_the_logits(mode):
    """A hand-built integer net keyed tiled with permutation keys (keynet_amd alone), integer images, sum |a| |x| propagated layer by layer in float64 on the host and
    asserted <= 2^24 (in units of the layer's quantum: 2^-2 behind the pool) at every layer.  Under exact=False and 'auto': the padded forward, narrow='mfma' at 1 and 8
    images, narrow32 at 16, narrow64='mfma' at 40 and one captured replay -- every layer's output (walked layer by layer from the exact=True forward's previous
    output) and the logits bits_equal to the exact=True forward, the logits to the plain net in float64.  Under 'auto' every conv layer decides 'mfma' with a
    measured difference of exactly 0.0."""
    for widths in NET_WIDTHS:
        (net, x) = _int_net(widths)
        plain = _plain_float64(net, x)
        if all(s <= xs.LIMIT for (_, _, s) in plain):
            break
    assert all(s <= xs.LIMIT for (_, _, s) in plain), [(n_, s) for (n_, _, s) in plain]
    print('  integer key-net: widths %r, sum |a||x| per layer (quanta) %s' % (widths, ['%s %.0f' % (n_, s) for (n_, _, s) in plain]))
    assert plain[-1][2] >= 2.0 ** 16                                       # (the sums are not trivially small)
    np.random.seed(3)
    torch.manual_seed(3)
    (sensor, knet) = ksys.TiledPermutationKeynet((3, 8, 8), net, 4)
    xc = sensor.fromtensor(x.to(dev())).encrypt().astensor()
    logits64 = plain[-1][1].numpy()
    assert np.array_equal(logits64.astype(np.float32).astype(np.float64), logits64)
    # the exact=True forward, layer by layer: the reference of every form
    knet.exact_mode(True)
    (outs, y) = ({}, xc)
    children = list(knet._keynet.named_children())
    for (lname, child) in children:
        y = child.forward(y) if isinstance(child, KeyedLayer) else ksys._relu_block(y)
        outs[lname] = y.clone()
    ref_logits = knet.forward_linear(xc).cpu().numpy()
    vc.assert_bits_equal(np.ascontiguousarray(outs[children[-1][0]].cpu().numpy()), ref_logits, 'exact=True: the walk against forward_linear')
    vc.assert_bits_equal(np.ascontiguousarray(ref_logits[:, :-1]), logits64.astype(np.float32), 'exact=True logits against the plain net in float64')
    knet.exact_mode(mode)
    vc.assert_bits_equal(knet.forward_linear(xc).cpu().numpy(), ref_logits, 'contract %r: the padded forward (it calibrates an auto key-net)' % (mode,))
    convs = [(lname, c) for (lname, c) in children if isinstance(c, KeyedLayer) and isinstance(c.W, ksp.Conv2dTiledMatrix)]
    assert len(convs) == 3
    for (name, n, kw) in FORMS:
        xn = xc[:n].contiguous()
        vc.assert_bits_equal(knet.forward_linear(xn, **kw).cpu().numpy(), np.ascontiguousarray(ref_logits[:n]), '%r %s: logits' % (mode, name))
        prev = xn
        for (lname, child) in children:
            got = child.forward(prev, **kw) if isinstance(child, KeyedLayer) else ksys._relu_block(prev)
            want = outs[lname][:n]
            vc.assert_bits_equal(np.ascontiguousarray(got.cpu().numpy()), np.ascontiguousarray(want.cpu().numpy()), '%r %s: layer %s' % (mode, name, lname))
            prev = want.contiguous()
    x8 = xc[:8].contiguous()
    replay = knet.capture(x8, narrow='mfma')
    vc.assert_bits_equal(replay(xc[8:16].contiguous()).clone().cpu().numpy(), np.ascontiguousarray(ref_logits[8:16]), '%r: captured replay' % (mode,))
    assert getattr(replay, 'graph', None) is not None
    for (lname, c) in convs:
        if mode is False:
            assert c._exact is False
            continue
        rec = c._contract_record
        assert c._exact is False and rec['decided'] == 'mfma' and rec['measured_mfma_vs_exact'] == 0.0, (lname, rec)
        if rec.get('narrow') is not None and 'measured_narrow_mfma_vs_exact' in rec['narrow']:      # (where measured: the pool's operator has no matrix-core narrow form, its record says why)
            assert rec['narrow']['decided'] == 'mfma' and rec['narrow']['measured_narrow_mfma_vs_exact'] == 0.0, (lname, rec['narrow'])
    if mode == 'auto':
        assert sum('measured_narrow_mfma_vs_exact' in (c._contract_record.get('narrow') or {}) for (_, c) in convs) >= 1
