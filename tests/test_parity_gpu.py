"""Parity of the HIP path (through the C ABI) against the reference's vectors and the CPU oracle.  Needs an MI355X."""
import copy
import functools

import numpy as np
import pytest
import torch
import scipy.sparse

import oracle
from keynet_amd import io as kio
from keynet_amd import sparse as ksp
from keynet_amd import system as ksys
from keynet_amd import _capi
from keynet_amd.layer import KeyedLayer
from keynet_amd.torch import affine_to_linear, linear_to_affine
from torch import nn
from nets import LeNet_AvgPool, MiniNet, TinyAllConv, load_weights, _Chain

pytestmark = pytest.mark.gpu

EXACT_NETS = ['lenet_perm.npz', 'allconv_tiny_perm.npz', 'bn_tiny_perm.npz', 'bn_tiny_identity.npz']
TILED_NETS = ['mini_tiled_identity.npz', 'mini_tiled_permutation.npz', 'mini_tiled_permutation8.npz', 'mini_tiled_orthogonal.npz', 'mini_tiled_stochastic.npz']
TOL = 1e-5   # north_star: within 1e-5 for float keyed layers (MFMA path); bit-exact elsewhere


def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


def close(a, b, tol=TOL):
    """The reference's own criterion (test/test_keynet.py:33,196,218: np.allclose(a, b, atol=1e-5), numpy's default rtol = 1e-5):
    ELEMENT-WISE |a - b| <= tol + tol |b|.  A small element next to large ones gets no slack from them."""
    return bool(np.all(np.abs(a.astype(np.float64) - b) <= tol + tol * np.abs(b)))


EPS32 = float(np.finfo(np.float32).eps)


def close_conditioned(y, ref, op, x_affine, tol=TOL):
    """|y - ref| <= 1e-5 * max(1, |ref|) + 2 eps32 * sum_k |a_k x_k|, element-wise.

    Two correct f32 evaluations of one sum in different orders (MFMA fma chain vs scipy mul-then-add) differ by
    O(eps * sum|a_k x_k|).  For the identity / permutation keys that term is ~1e-6 and the bound is the north-star's 1e-5;
    for the orthogonal key family (bias key gamma=100: sum|a x| ~ 370 against |y| <= 1) the reference's OWN f32 output is
    3.4e-5 away from the exact (f64) value, so no implementation can be held to an absolute 1e-5 there."""
    (shape, ip, ix, dt) = op
    Wabs = scipy.sparse.csr_matrix((np.abs(dt).astype(np.float64), ix, ip), shape=shape)
    S = Wabs.dot(np.abs(x_affine.T.astype(np.float64))).T
    bound = tol * np.maximum(1.0, np.abs(ref)) + 2 * EPS32 * S
    return bool(np.all(np.abs(y.astype(np.float64) - ref) <= bound))


def test_device_is_gfx950():
    (n, arch) = _capi.device_info()
    assert n >= 1 and 'gfx950' in arch, arch


@pytest.mark.parametrize('name', EXACT_NETS)
def test_permutation_keynet_bit_exact_per_layer(golden, name):
    """Order-preserving CSR kernels == reference outputs (scipy csr_matvecs), bit for bit, every layer, batch > 1."""
    z = golden(name)
    knet = kio.keynet_from_arrays(z)
    y = torch.as_tensor(z['x_cipher']).to(dev())
    for (lname, child) in knet._keynet.named_children():
        if isinstance(child, KeyedLayer):
            y = child.forward(y)
        else:
            y = ksys._relu_block(y)
        assert np.array_equal(y.cpu().numpy(), z['Y.%s' % lname]), 'layer %s of %s' % (lname, name)
    # fused-ReLU forward gives the same final logits
    out = knet.forward_linear(torch.as_tensor(z['x_cipher']).to(dev())).cpu().numpy()
    assert np.array_equal(out, z['Y.%s' % [str(n) for n in z['layer_names']][-1]])
    assert np.array_equal(out, oracle.keynet_forward(oracle.load_golden_layers(z), z['x_cipher']))


@pytest.mark.parametrize('name', TILED_NETS)
def test_tiled_keynet_layers(golden, name):
    """Conv2dTiledMatrix on f32 MFMA: within 1e-5; with exact=True (order-preserving path) and for TiledMatrix /
    SparseMatrix layers: bit for bit.  Inputs to each layer are the reference's own previous-layer outputs."""
    z = golden(name)
    knet = kio.keynet_from_arrays(z)
    names = [str(n) for n in z['layer_names']]
    prev = z['x_cipher']
    for (lname, child) in knet._keynet.named_children():
        ref = z['Y.%s' % lname]
        if isinstance(child, KeyedLayer):
            xin = torch.as_tensor(prev).to(dev())
            if isinstance(child.W, ksp.Conv2dTiledMatrix):
                assert child._exact == 'auto'          # the default contract of a tiled layer; here the matrix-core path itself is under test
                child._exact = False
            y = child.forward(xin).cpu().numpy()
            if isinstance(child.W, ksp.Conv2dTiledMatrix):
                child._exact = 'auto'
                op = oracle.operator_from_golden(z, 'L.%s.' % lname)
                assert close_conditioned(y, ref, op, prev), 'MFMA layer %s of %s: %g' % (lname, name, np.abs(y - ref).max())
                if 'orthogonal' not in name:
                    assert close(y, ref), 'MFMA layer %s of %s: %g' % (lname, name, np.abs(y - ref).max())
                ye = child.W.torchdot(xin.t(), exact=True).t().cpu().numpy()
                assert np.array_equal(ye, ref), 'exact path, layer %s of %s' % (lname, name)
                # export == the reference's tocsr()
                c = child.W.tocsr()
                p = 'L.%s.' % lname
                assert c.nnz == len(z[p + 'data']) and child.W.nnz() == int(z[p + 'nnz'])
            else:
                assert np.array_equal(y, ref), 'layer %s of %s' % (lname, name)
        prev = ref
    # the whole net under its default contract ('auto': every layer meets 1e-5 against the reference's arithmetic, on the matrix cores
    # where that is possible): the float-key net is now as close as the permutation nets
    out = knet.forward_linear(torch.as_tensor(z['x_cipher']).to(dev())).cpu().numpy()
    assert close(out, z['Y.%s' % names[-1]], tol=2e-5)
    assert np.allclose(out[:, :-1], z['logits_plain'], atol=1e-4)      # the reference's criterion is 1e-5..1e-3 (test_keynet.py)
    rep = knet.contract_report()
    assert not rep['undecided']
    if 'orthogonal' in name:
        assert rep['switched'], rep                                    # gamma = 100 bias keys: these conv layers cannot hold 1e-5 on re-ordered f32 arithmetic
    elif 'stochastic' not in name:
        assert not rep['switched'], rep                                # identity / permutation keys stay on the matrix cores


@pytest.mark.parametrize('name', TILED_NETS)
def test_float_key_contract_auto(golden, name):
    """The 1e-5 contract, unconditioned: under the default 'auto' contract EVERY layer of every tiled key-net (inputs = the reference's own
    previous-layer outputs) is within the reference's np.allclose(atol=1e-5) of the reference, element-wise; layers that calibration left on the matrix cores really run
    there (their result differs from the order-preserving kernel's, or the layer is small enough to agree exactly), switched layers are
    bit-equal to the reference; exact_mode(False) brings the old behaviour back, exact_mode('auto') re-decides."""
    z = golden(name)
    knet = kio.keynet_from_arrays(z)
    prev = z['x_cipher']
    for (lname, child) in knet._keynet.named_children():
        ref = z['Y.%s' % lname]
        if isinstance(child, KeyedLayer):
            y = child.forward(torch.as_tensor(prev).to(dev())).cpu().numpy()
            assert close(y, ref), 'layer %s of %s under the auto contract: %g' % (lname, name, np.abs(y - ref).max())
            assert child._exact in (True, False)                       # decided
            if isinstance(child.W, ksp.Conv2dTiledMatrix):
                rec = child._contract_record
                assert rec['measured_mfma_vs_exact'] is not None and rec['decided'] == ('exact' if child._exact else 'mfma')
                if child._exact:
                    assert np.array_equal(y, ref), lname
                    assert rec['measured_mfma_vs_exact'] > 0.25 * rec['tol']
                else:
                    assert rec['measured_mfma_vs_exact'] <= 0.5 * rec['tol']
        prev = ref
    decided = {n: c._exact for (n, c) in knet._keynet.named_children() if isinstance(c, KeyedLayer)}
    knet.exact_mode(False)
    assert all(c._exact is False for c in knet._keynet.children() if isinstance(c, KeyedLayer))
    knet.exact_mode('auto')
    assert set(knet.contract_report()['undecided']) == set(decided)
    knet.forward_linear(torch.as_tensor(z['x_cipher']).to(dev()))
    again = {n: c._exact for (n, c) in knet._keynet.named_children() if isinstance(c, KeyedLayer)}
    if 'orthogonal' not in name:
        assert again == decided                                        # same inputs for the first layers, same decision


@pytest.mark.parametrize('name', ['mini_tiled_orthogonal.npz', 'mini_tiled_permutation.npz'])
def test_float_key_error_is_no_worse_than_the_references_own(golden, name):
    """Evidence for the conditioned bound above.  Per keyed conv layer (inputs = the reference's own previous-layer outputs) the
    float64 product of the stored f32 operator is the truth; the reference's f32 output (scipy: every product AND every sum
    rounded) misses it by e_ref, the MFMA path (one rounding per term) by e_hip.  The orthogonal family's gamma = 100 bias key
    makes e_ref itself exceed 1e-5, so an absolute 1e-5 against the reference cannot be demanded of ANY f32 evaluation; what can
    is that the HIP path is at least as close to the truth as the reference is: max error within 2x, RMS error within 1.25x
    (measured: the MFMA errors are smaller), and the absolute 1e-5 contract wherever the reference itself meets it."""
    z = golden(name)
    knet = kio.keynet_from_arrays(z)
    prev = z['x_cipher']
    report = []
    for (lname, child) in knet._keynet.named_children():
        ref = z['Y.%s' % lname]
        if isinstance(child, KeyedLayer) and isinstance(child.W, ksp.Conv2dTiledMatrix):
            (shape, ip, ix, dt) = oracle.operator_from_golden(z, 'L.%s.' % lname)
            W64 = scipy.sparse.csr_matrix((dt.astype(np.float64), ix, ip), shape=shape)
            truth = W64.dot(prev.T.astype(np.float64)).T                      # [N, Dout+1]; no ReLU inside a KeyedLayer of these nets
            child._exact = False                                              # the matrix-core path is what is characterised here
            y = child.forward(torch.as_tensor(prev).to(dev())).cpu().numpy()
            (e_ref, e_hip) = (np.abs(ref.astype(np.float64) - truth), np.abs(y.astype(np.float64) - truth))
            report.append((lname, float(e_ref.max()), float(e_hip.max()), float(np.sqrt((e_ref ** 2).mean())), float(np.sqrt((e_hip ** 2).mean()))))
            assert e_hip.max() <= 2.0 * e_ref.max() + 1e-7, report[-1]
            assert np.sqrt((e_hip ** 2).mean()) <= 1.25 * np.sqrt((e_ref ** 2).mean()) + 1e-8, report[-1]
            if e_ref.max() <= 0.5e-5 * max(1.0, float(np.abs(truth).max())):
                assert np.abs(y - ref).max() <= 1e-5 * max(1.0, float(np.abs(ref).max())), report[-1]
        prev = ref
    print('float-key error vs f64 truth (layer, max ref, max hip, rms ref, rms hip):', report)
    assert len(report) == 2
    if 'orthogonal' in name:
        assert max(r[1] for r in report) > 1e-5      # the premise: the reference's own f32 result is further than 1e-5 from the truth


@pytest.mark.parametrize('name,n', [('lenet_perm.npz', 1024), ('mini_tiled_permutation.npz', 512), ('allconv_tiny_perm.npz', 256)])
def test_overlapped_forward_is_bit_identical(golden, name, n):
    """KeyedModel.forward_linear's default for large device-resident batches -- two half-batch column windows on two side streams,
    one kernel apart, ping-pong workspaces -- against the plain single-stream forward and the reference vectors: bit for bit
    (every batch column is computed by the same kernel instantiation either way), repeatedly (workspaces are reused)."""
    z = golden(name)
    knet = kio.keynet_from_arrays(z)
    xc = torch.as_tensor(z['x_cipher'])
    m = xc.shape[0]
    x = torch.cat([xc] * ((n + m - 1) // m), dim=0)[:n].to(dev()).t().contiguous().t()
    y0 = knet.forward_linear(x, overlap=False)                   # (decides the tiled net's 'auto' layers: a layer still to calibrate has no launch to plan)
    assert knet._overlap_plan(x.device, n) is None                # these nets are small: the automatic choice is the plain forward
    plan = knet._overlap_plan(x.device, n, force=True)
    assert plan is not None and any(sg[0] == 'split' and sg[2] - sg[1] >= 2 for sg in plan['segments']) and plan['segments'][-1][0] == 'whole'   # trailing fc layers run whole
    # the plan's launch list IS the layers' own rule (KeyedLayer.launch), step for step: the same handle, the same flags
    steps = knet._steps()
    assert len(steps) == len(plan['steps'])
    for ((k, c, relu), st) in zip(steps, plan['steps']):
        la = c.launch(x.device, relu)
        assert st.op is la.op and st.flags == la.flags, (k, st, la)
    for _ in range(3):
        y1 = knet.forward_linear(x, overlap=True)
        assert torch.equal(y0, y1)
    if 'tiled' not in name:
        assert np.array_equal(y0[:m].cpu().numpy(), z['Y.%s' % [str(k) for k in z['layer_names']][-1]])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                                  # also from a non-default caller stream
        s.wait_stream(torch.cuda.default_stream())
        y2 = knet.forward_linear(x, overlap=True)
    s.synchronize()
    assert torch.equal(y0, y2)
    knet.exact_mode(True)
    assert knet._overlap_plan(x.device, n, force=True) is not plan          # contracts changed: the launch lists are rebuilt
    ye = knet.forward_linear(x, overlap=True)
    assert torch.equal(ye, knet.forward_linear(x, overlap=False))


def test_export_csr_matches_reference_tocsr(golden):
    z = golden('mini_tiled_permutation.npz')
    for lname in ('conv1', 'conv2', 'pool1'):
        p = 'L.%s.' % lname
        W = kio.operator_from_arrays(z, p)
        (ip, ix, dt) = W._device_op().export_csr()
        assert np.array_equal(ip, z[p + 'indptr']) and np.array_equal(ix, z[p + 'indices']) and np.array_equal(dt, z[p + 'data']), lname
        assert W._device_op().nnz() == int(z[p + 'nnz'])
        assert W._device_op().shape() == tuple(int(v) for v in z[p + 'shape'])


def test_full_stack_seeded_permutation_keynet(golden):
    """README.md:27-34 flow on the GPU: factory under the seed -> sensor.encrypt -> model.forward == reference."""
    z = golden('lenet_perm.npz')
    net = load_weights(LeNet_AvgPool(), z)
    np.random.seed(0)
    (sensor, knet) = ksys.PermutationKeynet((1, 28, 28), net)
    x = torch.as_tensor(z['x_plain'])
    xc = sensor.fromtensor(x.to(dev())).encrypt().astensor()
    assert np.array_equal(xc.cpu().numpy(), z['x_cipher'])           # permutation sensor = exact gather
    y = knet.forward(xc)
    assert tuple(y.shape) == (8, 10, 1, 1)
    assert np.array_equal(y.reshape(8, 10).cpu().numpy(), z['logits_keyed'])
    assert np.allclose(y.reshape(8, 10).cpu().numpy(), z['logits_plain'], atol=1e-5)   # the reference's own criterion
    # N == 1 API shape and CPU-tensor round trip (drop-in for callers that pass CPU tensors)
    y1 = knet.forward(sensor.fromtensor(x[0:1]).encrypt().astensor())
    assert tuple(y1.shape) == (10, 1, 1) and not y1.is_cuda
    assert np.array_equal(y1.numpy(), z['forward_n1'])
    # decrypt round trip (permutation key: exact)
    back = sensor.fromtensor(x).encrypt().decrypt().astensor()
    assert np.array_equal(back.numpy(), z['x_plain'])
    # config 1: owl.jpg 28x28
    yo = knet.forward(torch.as_tensor(z['owl_cipher']).to(dev()))
    assert np.array_equal(yo.cpu().numpy(), z['owl_forward'])


def test_full_stack_tiled_permutation(golden):
    z = golden('mini_tiled_permutation.npz')
    net = load_weights(MiniNet(), z)
    np.random.seed(0)
    (sensor, knet) = ksys.TiledPermutationKeynet((2, 16, 16), net, 4)
    xc = sensor.fromtensor(torch.as_tensor(z['x_plain']).to(dev())).encrypt().astensor()
    assert np.array_equal(xc.cpu().numpy(), z['x_cipher'])
    y = knet.forward(xc).reshape(4, 10).cpu().numpy()
    assert np.array_equal(y, z['logits_keyed'])          # a permutation-only key-net is bit-exact by default (north_star)
    assert np.allclose(y, z['logits_plain'], atol=1e-4)


@pytest.mark.parametrize('direct', [False, True])
def test_full_stack_tiled_orthogonal(golden, direct):
    """Float-key family through the whole stack (factory under the seed -> encrypt -> forward on MFMA), both keying routes;
    criterion = the reference's own (keyed logits vs plain net, test/test_keynet.py:196-219 use 1e-5 on LeNet; the gamma=100
    bias key costs ~1e-5 of f32 cancellation already in the reference: tests/golden/make_golden.py prints 1.06e-5)."""
    import warnings
    z = golden('mini_tiled_orthogonal.npz')
    net = load_weights(MiniNet(), z)
    np.random.seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        (sensor, knet) = ksys.TiledOrthogonalKeynet((2, 16, 16), net, 4, direct=direct)
    xc = sensor.fromtensor(torch.as_tensor(z['x_plain']).to(dev())).encrypt().astensor()
    assert close(xc.cpu().numpy(), z['x_cipher'], tol=1e-6)
    y = knet.forward(xc).reshape(4, 10).cpu().numpy()
    assert np.allclose(y, z['logits_keyed'], atol=1e-4)
    assert np.allclose(y, z['logits_plain'], atol=1e-4)


def test_filled_in_key_family_direct_route_against_the_reference(golden):
    """The FILLED-IN key family (test/test_keynet.py:116-129; doubly-stochastic local keys keynet/sparse.py:335-353; SpGEMM fill-in keynet/layer.py:35) keyed by
    the DIRECT route (keynet_amd/direct.py: the factored operator holds the terms coef * tap of every stored entry) against the REFERENCE's own per-layer outputs
    (tests/golden/mini_tiled_stochastic.npz; inputs of every layer = the reference's previous-layer outputs).  What is claimed, and no more:
      * KN_FLAG_EXACT on a direct-keyed float operator = the order-preserving product of the factored operator's OWN stored values (each the f32 sum of its terms
        in entry order): bit-equal to the oracle on Conv2dTiledMatrix.rows_csr -- and within the reference's gate (np.allclose(atol=1e-5), element-wise) of the
        reference's outputs, NOT bit-equal to them: scipy's SpGEMM summed the same terms in another order (2e-6 relative on the stored values, tests/test_direct_keying.py);
      * the layer's default contract ('auto'), the matrix-core kernel and the split application: inside the same gate of the reference's outputs;
      * kn_spmm_plan names the kernels this family was built for."""
    import sys, os, warnings
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    from keygen_case_table import STOCHASTIC_KW
    z = golden('mini_tiled_stochastic.npz')
    net = load_weights(MiniNet(), z)
    np.random.seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        (sensor, knet) = ksys.Keynet((2, 16, 16), net, direct=True, **STOCHASTIC_KW)
    xc = sensor.fromtensor(torch.as_tensor(z['x_plain']).to(dev())).encrypt().astensor()
    assert close(xc.cpu().numpy(), z['x_cipher'], tol=1e-6)
    prev = z['x_cipher']
    convs = 0
    for (lname, child) in knet._keynet.named_children():
        ref = z['Y.%s' % lname]
        if isinstance(child, KeyedLayer):
            xin = torch.as_tensor(prev).to(dev())
            W = child.W
            if isinstance(W, ksp.Conv2dTiledMatrix):
                convs += 1
                assert W._taps is not None and W._taps['ent_coef'] is not None and W.fill_factor() >= ksp.Conv2dTiledMatrix.SPLIT_MIN_FILL and W.split_capable()
                with torch.cuda.device(dev()):
                    plan = W._device_op(dev()).plan(int(xin.shape[0]), _capi.KN_FLAG_EXACT)
                assert 'convtaps_exact_fill_kernel' in plan, plan
                ye = W.torchdot(xin.t(), exact=True).t().cpu().numpy()
                assert close(ye, ref), 'order-preserving product of the direct operator, layer %s: %g' % (lname, np.abs(ye - ref).max())
                M = W.rows_csr()                                                   # every pixel: the whole operator incl. its homogeneous row
                assert np.array_equal(ye, oracle.csr_matvecs(M.shape, M.indptr, M.indices, M.data.astype(np.float32), np.ascontiguousarray(prev.T)).T), lname
                R = scipy.sparse.csr_matrix((z['L.%s.data' % lname], z['L.%s.indices' % lname], z['L.%s.indptr' % lname]), shape=M.shape)
                assert abs(M - R).max() <= 2e-6 * abs(R).max()                     # its stored values against the reference's tocsr(): re-associated sums, not bits
                for (mode, what) in ((False, 'matrix cores'), ('split', 'split application')):
                    ym = W.torchdot(xin.t(), exact=mode).t().cpu().numpy()
                    assert close(ym, ref), '%s, layer %s: %g' % (what, lname, np.abs(ym - ref).max())
            y = child.forward(xin).cpu().numpy()                                  # the layer's default contract
            assert close(y, ref), 'layer %s under its default contract: %g' % (lname, np.abs(y - ref).max())
            if isinstance(W, ksp.Conv2dTiledMatrix):
                assert child._contract_record['decided'] in ('split', 'mfma', 'exact'), child._contract_record
        prev = ref
    assert convs == 2
    out = knet.forward(xc).reshape(4, 10).cpu().numpy()
    assert np.allclose(out, z['logits_keyed'], atol=1e-5) and np.allclose(out, z['logits_plain'], atol=1e-5)     # the reference's criterion for this family (test_keynet.py:128)


def test_challenge_known_answer(golden):
    """demo/challenge.ipynb cell 5 through the only key-net the reference ships (demo/keynet_challenge_lenet_10AUG20.pkl): its conv / pool
    operators carry FLOAT64 values, scipy computes them in float64 (keynet/sparse.py:488-492 + numpy's up-cast) and each layer returns a
    float64 block that the next layer's coercion rounds to f32.  Every one of the 11 layer outputs the reference produced -- dtype and
    bits -- and the final floats, bit for bit."""
    z = golden('challenge_kat.npz')
    knet = kio.keynet_from_arrays(z)
    y = torch.as_tensor(z['x_linear']).to(dev())
    for (name, c) in knet._keynet.named_children():
        y = c.forward(y) if isinstance(c, KeyedLayer) else ksys._relu_block(y)
        ref = z['Y.%s' % name]
        if isinstance(c, KeyedLayer):
            assert str(y.dtype).replace('torch.', '') == str(ref.dtype), name                   # float64 operators return float64, as in the reference
            assert np.array_equal(y.cpu().numpy(), ref), name
        else:
            assert np.array_equal(y.cpu().numpy(), ref.astype(np.float32)), name                # (a stand-alone ReLU hands on what the next layer would coerce to)
    # the whole forward (ReLUs fused into the float64 kernels' epilogues): the reference's final floats, and all four printed decimals
    out = knet.forward_linear(torch.as_tensor(z['x_linear']).to(dev()))
    assert out.dtype == torch.float32 and np.array_equal(out.cpu().numpy(), z['Y.fc3'])
    assert np.array_equal(np.round(out.cpu().numpy().flatten()[:-1].astype(np.float64), 4), z['published'])
    # ... and on a batch: rows are independent, every row equals the single-image result
    xb = torch.as_tensor(np.repeat(z['x_linear'], 70, axis=0)).to(dev())
    yb = knet.forward_linear(xb).cpu().numpy()
    assert np.array_equal(yb, np.repeat(z['Y.fc3'], 70, axis=0))


@pytest.mark.parametrize('n_vecs', [1, 3, 64, 130, 256, 1024, 2048])
def test_csr_f64_kernel_vs_oracle_random(n_vecs):
    """A float64 operator (random, non-canonical: unsorted, duplicate columns, empty rows, one long row) against the oracle's float64
    csr_matvecs -- what scipy runs for (float64 matrix, float32 activations) -- at every vector width of the kernel: the float64 block
    (kn_spmm_f64), the same block rounded to f32 once (kn_spmm), ReLU fused, Inf / NaN / denormal values."""
    rng = np.random.RandomState(100 + n_vecs)
    (m, n) = (301, 157)
    rows = []
    for r in range(m):
        if r % 17 == 0:
            rows.append(np.zeros(0, dtype=np.int32))
        elif r == 5:
            rows.append(rng.randint(0, n, 3000).astype(np.int32))
        else:
            rows.append(rng.randint(0, n, rng.randint(1, 90)).astype(np.int32))
    indptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int32)
    indices = np.concatenate(rows)
    data = rng.randn(len(indices)) * np.exp(rng.uniform(-30, 30, len(indices)))          # float64 values well outside f32's precision
    data[7] = 1e-310                                                                      # a float64 denormal
    X = rng.randn(n, n_vecs).astype(np.float32)
    X[3, 0] = np.inf
    X[11, n_vecs - 1] = np.nan
    X[20, n_vecs // 2] = 1e-42                                                            # an f32 denormal
    W = ksp.SparseMatrix(scipy.sparse.csr_matrix((data, indices, indptr), shape=(m, n)))
    assert W.is_float64()
    with np.errstate(all='ignore'):
        ref = oracle.csr_matvecs((m, n), indptr, indices, data, X)
    assert ref.dtype == np.float64
    y = W.torchdot(torch.as_tensor(X).to(dev()))
    assert y.dtype == torch.float64 and np.array_equal(y.cpu().numpy(), ref, equal_nan=True)
    yr = W.torchdot(torch.as_tensor(X).to(dev()), relu=True).cpu().numpy()
    assert np.array_equal(yr, np.where(ref < 0, 0.0, ref), equal_nan=True)
    # kn_spmm on the float64 handle: the block rounded to f32 once
    op = W._device_op(dev())
    assert op.dtype_bits() == 64 and 'csr_rows_f64_kernel' in op.plan(n_vecs)
    xd = torch.as_tensor(X).to(dev())
    y32 = torch.empty((m, n_vecs), dtype=torch.float32, device=dev())
    op.spmm(xd.data_ptr(), n_vecs, n_vecs, y32.data_ptr(), n_vecs, _capi.KN_FLAG_EXACT, torch.cuda.current_stream().cuda_stream)
    with np.errstate(all='ignore'):
        assert np.array_equal(y32.cpu().numpy(), ref.astype(np.float32), equal_nan=True)
    # export: stored order and float64 values come back; the f32 entry points refuse the handle and vice versa
    (ip, ix, dt) = op.export_csr()
    assert dt.dtype == np.float64 and np.array_equal(ip, indptr) and np.array_equal(ix, indices) and np.array_equal(dt, data)
    W32 = ksp.SparseMatrix(scipy.sparse.csr_matrix((data.astype(np.float32), indices, indptr), shape=(m, n)))
    op32 = W32._device_op(dev())
    assert op32.dtype_bits() == 32
    y64 = torch.empty((m, n_vecs), dtype=torch.float64, device=dev())
    with pytest.raises(_capi.KeynetHipError):
        op32.spmm_f64(xd.data_ptr(), n_vecs, n_vecs, y64.data_ptr(), n_vecs, 0, torch.cuda.current_stream().cuda_stream)
    with pytest.raises(_capi.KeynetHipError):
        _capi.Operator.chain([op], [0])


def test_tiled_cases(golden):
    """test/test_sparse.py:122-199 shapes through the device operators."""
    z = golden('tiled_cases.npz')
    names = sorted({k.split('.')[1] for k in z.files if k.startswith('C.')})
    for n in names:
        p = 'C.%s.' % n
        W = kio.operator_from_arrays(z, p)
        x = torch.as_tensor(z[p + 'x']).to(dev())
        if isinstance(W, ksp.Conv2dTiledMatrix):
            y = W.torchdot(x).cpu().numpy()
            assert close(y, z[p + 'y']), n
            assert np.array_equal(W.torchdot(x, exact=True).cpu().numpy(), z[p + 'y']), n
            assert np.array_equal(W.dot(z[p + 'x']).shape, z[p + 'y'].shape)
        else:
            assert np.array_equal(W.torchdot(x).cpu().numpy(), z[p + 'y']), n
    # dense / COO SparseMatrix (test_sparse.py:304-329)
    for M in (z['D.W'], scipy.sparse.coo_matrix(z['D.W'])):
        A = ksp.SparseMatrix(M)
        assert np.allclose(A.dot(z['D.x']), z['D.W'].dot(z['D.x']), atol=1e-5)
        assert np.allclose(A.torchdot(torch.as_tensor(z['D.x'])).numpy(), z['D.W'].dot(z['D.x']), atol=1e-5)


@pytest.mark.parametrize('n_vecs', [4, 256, 200])
def test_dense_linear_mfma_vs_oracle(n_vecs):
    """A keyed nn.Linear as a split-K f32-MFMA GEMM (kn_dense_create; tolerance mode of the tiled key-nets) vs the oracle;
    the same operator with exact=True stays bit-exact."""
    rng = np.random.RandomState(7)
    (outs, ins) = (1100, 1024)
    D = np.zeros((outs + 1, ins + 1), dtype=np.float32)
    D[:-1, :-1] = (rng.randn(outs, ins) / np.sqrt(ins)).astype(np.float32)
    D[:-1, -1] = rng.randn(outs).astype(np.float32)
    D[-1, -1] = 1.0
    perm = rng.permutation(ins)
    M = scipy.sparse.csr_matrix(D)
    M = scipy.sparse.csr_matrix((M.data, np.where(M.indices < ins, perm[np.minimum(M.indices, ins - 1)], M.indices).astype(np.int32), M.indptr), shape=M.shape)  # unsorted columns
    W = ksp.SparseMatrix(M)
    X = np.vstack((rng.randn(ins, n_vecs).astype(np.float32), np.ones((1, n_vecs), np.float32)))
    ref = oracle.csr_matvecs(M.shape, M.indptr, M.indices, M.data, X)
    xd = torch.as_tensor(X).to(dev())
    assert np.array_equal(W.torchdot(xd).cpu().numpy(), ref)                       # default: exact
    assert W._dense_device_op() is not None
    for relu in (False, True):
        y = W.torchdot(xd, relu=relu, exact=False).cpu().numpy()
        r = np.maximum(ref, 0) if relu else ref
        assert close_conditioned(y.T, r.T, (M.shape, M.indptr, M.indices, M.data), X.T), np.abs(y - r).max()
        assert close(y, r, tol=2e-5)
    Ms = scipy.sparse.csr_matrix(D[:65, :])
    small = ksp.SparseMatrix(Ms)
    assert small._dense_device_op() is None                                       # not eligible -> exact CSR path
    assert np.array_equal(small.torchdot(xd, exact=False).cpu().numpy(), oracle.csr_matvecs(Ms.shape, Ms.indptr, Ms.indices, Ms.data, X))


@pytest.mark.parametrize('outs,ins,n_vecs', [(300, 2500, 1), (300, 2500, 100), (1000, 4100, 256), (257, 2048, 64), (513, 3000, 130)])
def test_big_pattern_group_kernel_vs_oracle(outs, ins, n_vecs):
    """A keyed nn.Linear under the bit-exact contract: hundreds of rows sharing one (unsorted) column sequence of thousands of columns
    run in the LDS-staged workgroup kernel (csr_big_group_kernel: 32 rows x 64 batch columns per workgroup, chunks of 32 columns);
    row counts that do not fill the last 32-row block or 8-row bundle, column counts that do not fill the last chunk, ragged
    batches, the loose homogeneous row next to it.  Bit-exact vs the oracle; KN_NO_BIG_GROUPS (read at create) gives the per-wave
    kernel for a bit-for-bit cross-check."""
    import os
    rng = np.random.RandomState(outs + ins + n_vecs)
    D = np.zeros((outs + 1, ins + 1), dtype=np.float32)
    D[:-1, :-1] = (rng.randn(outs, ins) / np.sqrt(ins)).astype(np.float32)
    D[:-1, -1] = rng.randn(outs).astype(np.float32)
    D[-1, -1] = 1.0
    perm = rng.permutation(ins + 1)
    M = scipy.sparse.csr_matrix(D)
    rowlen = np.diff(M.indptr)
    assert np.all(rowlen[:-1] == ins + 1)
    idx = M.indices.copy()
    dat = M.data.copy()
    for r in range(outs):                                       # the same unsorted column order in every row (what a keyed Linear stores)
        idx[M.indptr[r]:M.indptr[r + 1]] = M.indices[M.indptr[r]:M.indptr[r + 1]][perm]
        dat[M.indptr[r]:M.indptr[r + 1]] = M.data[M.indptr[r]:M.indptr[r + 1]][perm]
    M = scipy.sparse.csr_matrix((dat, idx, M.indptr), shape=M.shape)
    X = np.vstack((rng.randn(ins, n_vecs).astype(np.float32), np.ones((1, n_vecs), np.float32)))
    ref = oracle.csr_matvecs(M.shape, M.indptr, M.indices, M.data, X)
    xd = torch.as_tensor(X).to(dev())
    W = ksp.SparseMatrix(M)
    for relu in (False, True):
        y = W.torchdot(xd, relu=relu).cpu().numpy()
        assert np.array_equal(y, np.maximum(ref, 0) if relu else ref), (outs, ins, n_vecs, relu)
    os.environ['KN_NO_BIG_GROUPS'] = '1'
    try:
        W2 = ksp.SparseMatrix(M)
        y2 = W2.torchdot(xd).cpu().numpy()
    finally:
        os.environ.pop('KN_NO_BIG_GROUPS', None)
    assert np.array_equal(y2, ref)


def test_dense_handle_on_two_streams_concurrently():
    """include/keynet_hip.h: one handle may be driven from several streams at once.  A dense (split-K MFMA) operator keeps its
    partial sums in a PER-STREAM workspace: two streams hammering one handle with different inputs (and batch sizes that force
    the workspace to grow mid-flight) must each reproduce what a lone stream computes, bit for bit."""
    rng = np.random.RandomState(11)
    (outs, ins) = (512, 2048)
    D = np.zeros((outs + 1, ins + 1), dtype=np.float32)
    D[:-1, :-1] = (rng.randn(outs, ins) / np.sqrt(ins)).astype(np.float32)
    D[:-1, -1] = rng.randn(outs).astype(np.float32)
    D[-1, -1] = 1.0
    W = ksp.SparseMatrix(D)
    d = dev()
    op = W._dense_device_op(d)
    assert op is not None

    def inputs(n, seed):
        g = torch.Generator(device=d).manual_seed(seed)
        x = torch.randn((ins + 1, n), generator=g, device=d)
        x[-1] = 1.0
        return x
    xs = [inputs(128, 1), inputs(384, 2), inputs(256, 3), inputs(640, 4)]
    lone = []
    for x in xs:                                                # reference: one stream, one call at a time
        y = torch.empty((outs + 1, x.shape[1]), device=d)
        op.spmm(x.data_ptr(), x.shape[1], x.shape[1], y.data_ptr(), x.shape[1], 0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        lone.append(y)
    W2 = ksp.SparseMatrix(D)                                    # a fresh handle: workspaces start empty and must grow under load
    op2 = W2._dense_device_op(d)
    streams = [torch.cuda.Stream(device=d), torch.cuda.Stream(device=d)]
    outs_ = [[None] * len(xs) for _ in streams]
    for rep in range(6):
        for (k, x) in enumerate(xs):
            for (si, st) in enumerate(streams):
                xi = xs[(k + si) % len(xs)]                     # the two streams work on DIFFERENT inputs at the same time
                y = torch.empty((outs + 1, xi.shape[1]), device=d)
                st.wait_stream(torch.cuda.current_stream())
                op2.spmm(xi.data_ptr(), xi.shape[1], xi.shape[1], y.data_ptr(), xi.shape[1], 0, st.cuda_stream)
                outs_[si][(k + si) % len(xs)] = y
    torch.cuda.synchronize()
    for si in range(len(streams)):
        for k in range(len(xs)):
            assert torch.equal(outs_[si][k], lone[k]), (si, k)


def test_operator_is_bound_to_its_device():
    """kn_spmm refuses a handle that lives on another device than the current one (KN_ERR_INVALID) instead of dereferencing
    foreign memory; the Python containers create and cache their handles per device of the activations."""
    W = ksp.SparseMatrix(scipy.sparse.eye(6, dtype=np.float32).tocsr())
    x = torch.ones(6, 3).to(dev())
    assert torch.equal(W.torchdot(x), x)
    assert isinstance(W._op, dict) and list(W._op.keys()) == [dev().index if dev().index is not None else 0]
    if torch.cuda.device_count() > 1:
        op = W._device_op(dev())
        y = torch.empty(6, 3, device='cuda:1')
        with torch.cuda.device(1):
            with pytest.raises(_capi.KeynetHipError):
                op.spmm(x.data_ptr(), 3, 3, y.data_ptr(), 3, 0, torch.cuda.current_stream().cuda_stream)
            x1 = x.to('cuda:1')
            assert torch.equal(W.torchdot(x1), x1) and sorted(W._op.keys()) == [0, 1]


def test_empty_operator_arrays():
    """An all-zero operator (nnz == 0: numpy hands over non-null pointers to empty arrays) must not read host memory."""
    W = ksp.SparseMatrix(scipy.sparse.csr_matrix((5, 7), dtype=np.float32))
    y = W.torchdot(torch.ones(7, 4).to(dev()))
    assert tuple(y.shape) == (5, 4) and float(y.abs().max()) == 0.0


def test_padded_contraction_rows_do_not_leak_nan():
    """Cin = 3 on the chunked MFMA kernel (KC = 4: one zero-padded contraction row per chunk; a 5x5 window keeps the operator off
    the one-shot small-K kernel): the padding rows are stored as zeros, so NaN / Inf in live activations reach exactly the outputs
    whose window contains them -- the same rows as on the order-preserving path -- and every other output stays finite and
    within tolerance."""
    rng = np.random.RandomState(3)
    (Cin, Cout, H) = (3, 64, 8)
    from keynet_amd import direct as kdirect
    (eo, ei, et) = ([], [], [])
    for (t, ((i, j), S)) in enumerate(kdirect.shift_matrices((H, H), 5, 1)):
        S = S.tocoo()
        eo.append(S.row); ei.append(S.col); et.append(np.full(S.nnz, t))
    taps = rng.randn(25, Cout, Cin).astype(np.float32)
    lastcol = np.concatenate((rng.randn(Cout * H * H), [1.0])).astype(np.float32)
    W = ksp.Conv2dTiledMatrix.fromtaps((Cin, H, H), (Cout, H, H), taps, np.concatenate(eo), np.concatenate(ei), np.concatenate(et), None, lastcol)
    x = torch.randn(Cin * H * H + 1, 256, device=dev())
    x[-1] = 1.0
    x[2 * H * H + 3 * H + 3, :] = float('nan')      # pixel (3,3) of the LAST channel: 25 windows contain it
    x[1 * H * H + 0, 7] = float('inf')              # and one Inf in a corner pixel of channel 1, one image only
    y = W.torchdot(x, exact=False)
    ye = W.torchdot(x, exact=True)
    bad = ~torch.isfinite(ye)
    assert bool(torch.equal(~torch.isfinite(y), bad)), 'non-finite pattern of the MFMA path differs from the order-preserving path'
    assert int(torch.isnan(ye).any(dim=1).sum()) == 25 * Cout
    ok = ~bad
    assert float((y[ok] - ye[ok]).abs().max()) <= 1e-5 * max(1.0, float(ye[ok].abs().max()))


@pytest.mark.parametrize('n_vecs', [1, 3, 64, 130, 256, 1024, 2048])
def test_csr_kernel_vs_oracle_random(n_vecs):
    """Random non-canonical CSR (unsorted, duplicate columns, empty rows, one long row, repeated patterns) vs the oracle,
    for every vector width / column-tile path of the kernel."""
    rng = np.random.RandomState(n_vecs)
    (m, n) = (301, 157)
    rows = []
    for r in range(m):
        if r % 17 == 0:
            rows.append(np.zeros(0, dtype=np.int32))                      # empty row
        elif r == 5:
            rows.append(rng.randint(0, n, 3000).astype(np.int32))         # long row with duplicates
        elif r % 3 == 0:
            rows.append(np.array([7, 3, 99, 3, 150, 0, 42, 41, 40], dtype=np.int32))   # shared pattern -> grouped kernel
        else:
            rows.append(rng.randint(0, n, rng.randint(1, 40)).astype(np.int32))
    indptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int32)
    indices = np.concatenate(rows)
    data = rng.randn(len(indices)).astype(np.float32)
    X = rng.randn(n, n_vecs).astype(np.float32)
    W = ksp.SparseMatrix(scipy.sparse.csr_matrix((data, indices, indptr), shape=(m, n)))
    ref = oracle.csr_matvecs((m, n), indptr, indices, data, X)
    y = W.torchdot(torch.as_tensor(X).to(dev())).cpu().numpy()
    assert np.array_equal(y, ref)
    yr = W.torchdot(torch.as_tensor(X).to(dev()), relu=True).cpu().numpy()
    assert np.array_equal(yr, np.maximum(ref, 0))
    # non-contiguous input view (what x_affine.t() is for a row-major batch)
    Xt = torch.as_tensor(np.ascontiguousarray(X.T)).to(dev())
    assert np.array_equal(W.torchdot(Xt.t()).cpu().numpy(), ref)


@pytest.mark.parametrize('cin,cout,hw,n_vecs', [(32, 128, 12, 256), (16, 64, 10, 512), (48, 192, 8, 128), (32, 256, 16, 256)])
def test_convtaps_fast_path_with_gain_coefficients(cin, cout, hw, n_vecs):
    """A permutation + photometric-gain keyed 3x3 conv in factored form: every (output, input) pixel entry carries the coefficient
    gain_out[o] / gain_in[i].  With whole 16-channel chunks the MFMA kernel takes its scalar-pointer fast path and scales each
    activation tile by its slot's coefficient on the way to LDS.  Checked against the order-preserving path within the float-key
    tolerance and against the generic loader (KN_NO_SPTR); the order-preserving path itself (the pipelined kernel's coefficient
    instantiation at 256+ columns: stored value = fl(coef * tap), 8 or 16 channels per wave) is bit-exact vs the oracle on the expanded rows."""
    import os
    from keynet_amd import direct as kdirect
    rng = np.random.RandomState(cin + cout + hw)
    HW = hw * hw
    w = (rng.randn(cout, cin, 3, 3) / np.sqrt(9 * cin)).astype(np.float32)
    b = rng.randn(cout).astype(np.float32)
    (pi, po) = (rng.permutation(HW), rng.permutation(HW))
    (g_out, g_in) = ((rng.rand(HW) + 0.5).astype(np.float32), (rng.rand(HW) + 0.5).astype(np.float32))
    (eo, ei, et, ec) = ([], [], [], [])
    for (t, ((i, j), S)) in enumerate(kdirect.shift_matrices((hw, hw), 3, 1)):
        S = S.tocoo()
        eo.append(po[S.row]); ei.append(pi[S.col]); et.append(np.full(S.nnz, t)); ec.append((g_out[po[S.row]] / g_in[pi[S.col]]).astype(np.float32))
    taps = np.stack([w[:, :, i, j] for i in range(3) for j in range(3)])
    lastcol = np.concatenate((np.repeat(b, HW), [1.0])).astype(np.float32)
    W = ksp.Conv2dTiledMatrix.fromtaps((cin, hw, hw), (cout, hw, hw), taps, np.concatenate(eo).astype(np.int32), np.concatenate(ei).astype(np.int32),
                                       np.concatenate(et).astype(np.int32), np.concatenate(ec), lastcol)
    X = np.vstack((rng.randn(cin * HW, n_vecs).astype(np.float32), np.ones((1, n_vecs), np.float32)))
    xd = torch.as_tensor(X).to(dev())
    M = W.rows_csr()
    ref = oracle.csr_matvecs(M.shape, M.indptr, M.indices, M.data.astype(np.float32), X)
    ye = W.torchdot(xd, relu=False, exact=True).cpu().numpy()
    assert np.array_equal(ye[:-1], ref[:cout * HW])
    scale = float(np.abs(ref).max())
    for relu in (False, True):
        r = np.maximum(ref[:cout * HW], 0) if relu else ref[:cout * HW]
        ym = W.torchdot(xd, relu=relu, exact=False).cpu().numpy()
        assert float(np.abs(ym[:-1] - r).max()) <= 1e-5 * max(1.0, scale), float(np.abs(ym[:-1] - r).max())
        os.environ['KN_NO_SPTR'] = '1'                     # options are recorded when a handle is created: a second handle of the same operator
        try:
            Wg = copy.deepcopy(W)
            Wg._op = None
            yg = Wg.torchdot(xd, relu=relu, exact=False).cpu().numpy()
            with torch.cuda.device(dev()):
                assert 'no_sptr=1' in Wg._device_op(dev()).plan(n_vecs) and 'sptr(' not in Wg._device_op(dev()).plan(n_vecs)
        finally:
            del os.environ['KN_NO_SPTR']
        assert float(np.abs(yg - ym).max()) <= 1e-5 * max(1.0, scale)


@pytest.mark.parametrize('n_vecs,members', [(512, 16), (512, 6), (1024, 37), (768, 96)])
def test_csr_grouped_pipeline_kernel_vs_oracle(n_vecs, members):
    """Permutation-keyed-conv-shaped operators: many groups of `members` rows sharing one unsorted column sequence (1 .. 70 columns:
    fewer than the four activation rows the kernel keeps in flight, not a multiple of four, duplicates), partial 16-row bundles,
    loose rows in between, over a 4-column-per-lane batch -- the software-pipelined grouped kernel (csr_group_pipe_kernel, 16 or 8
    rows per wavefront by bundle fill).  Bit-exact vs the oracle and bit-identical to the plain grouped kernel (KN_NO_GROUP_PIPE)."""
    import os
    rng = np.random.RandomState(n_vecs + members)
    n = 900
    n_groups = 2200 * 16 // max(members, 16)
    rows = []
    for g in range(n_groups):
        ncol = 1 + (g * 7) % 70
        pattern = rng.randint(0, n, ncol).astype(np.int32)
        for _ in range(members):
            rows.append(pattern)
        if g % 5 == 0:
            rows.append(rng.randint(0, n, rng.randint(0, 12)).astype(np.int32))       # loose row (sometimes empty)
    m = len(rows)
    indptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int32)
    indices = np.concatenate(rows)
    data = rng.randn(len(indices)).astype(np.float32)
    X = rng.randn(n, n_vecs).astype(np.float32)
    W = ksp.SparseMatrix(scipy.sparse.csr_matrix((data, indices, indptr), shape=(m, n)))
    ref = oracle.csr_matvecs((m, n), indptr, indices, data, X)
    xd = torch.as_tensor(X).to(dev())
    for relu in (False, True):
        y = W.torchdot(xd, relu=relu).cpu().numpy()
        assert np.array_equal(y, np.maximum(ref, 0) if relu else ref), (n_vecs, members, relu)
    os.environ['KN_NO_GROUP_PIPE'] = '1'                   # recorded at create: a second handle
    try:
        W2 = ksp.SparseMatrix(W._matrix)
        y2 = W2.torchdot(xd).cpu().numpy()
        with torch.cuda.device(dev()):
            assert 'csr_group_pipe_kernel' not in W2._device_op(dev()).plan(n_vecs, _capi.KN_FLAG_EXACT)
            assert 'csr_group_pipe_kernel' in W._device_op(dev()).plan(n_vecs, _capi.KN_FLAG_EXACT)
    finally:
        del os.environ['KN_NO_GROUP_PIPE']
    assert np.array_equal(y2, ref)


@pytest.mark.parametrize('n_vecs,window', [(128, None), (384, None), (128, 256), (128, 512)])
def test_csr_short_rows_half_wave_path(n_vecs, window):
    """Keyed-pooling-shaped operators (thousands of loose rows, ~9 unsorted non-zeros each, a few empty or longer rows) over a batch
    that fills half of a 256-column wave tile -- what each stream of the overlapped forward hands the pooling layers: one row
    per half wavefront (csr_rows_pair_kernel).  Bit-exact vs the oracle; `window` = the operand is a column window of a wider
    activation block (ldx = ldy = window > n_vecs), through the C ABI directly."""
    rng = np.random.RandomState(n_vecs + (window or 0))
    (m, n) = (6000, 2500)
    lens = rng.randint(6, 12, m)
    lens[::97] = 0
    lens[5::501] = 40
    indptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    indices = rng.randint(0, n, int(indptr[-1])).astype(np.int32)
    data = rng.randn(len(indices)).astype(np.float32)
    W = ksp.SparseMatrix(scipy.sparse.csr_matrix((data, indices, indptr), shape=(m, n)))
    if window is None:
        X = rng.randn(n, n_vecs).astype(np.float32)
        ref = oracle.csr_matvecs((m, n), indptr, indices, data, X)
        for relu in (False, True):
            y = W.torchdot(torch.as_tensor(X).to(dev()), relu=relu).cpu().numpy()
            assert np.array_equal(y, np.maximum(ref, 0) if relu else ref)
        return
    Xw = rng.randn(n, window).astype(np.float32)
    xd = torch.as_tensor(Xw).to(dev())
    yd = torch.full((m, window), 7.0, device=dev())
    c0 = window - n_vecs                                           # the LAST window of the block
    W._device_op(dev()).spmm(xd.data_ptr() + 4 * c0, window, n_vecs, yd.data_ptr() + 4 * c0, window, _capi.KN_FLAG_EXACT, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ref = oracle.csr_matvecs((m, n), indptr, indices, data, np.ascontiguousarray(Xw[:, c0:]))
    y = yd.cpu().numpy()
    assert np.array_equal(y[:, c0:], ref) and np.all(y[:, :c0] == 7.0)          # nothing outside the window is touched


def test_batch_columns_are_independent(golden):
    """Size-independent property: column b of a batched forward is bit-identical to the single-image forward."""
    z = golden('lenet_perm.npz')
    knet = kio.keynet_from_arrays(z)
    rng = np.random.RandomState(0)
    X = np.concatenate([z['x_cipher']] * 128 + [z['x_cipher'][:3]], axis=0)      # 1027 images: ragged tail
    X[:, :-1] += rng.randn(*X[:, :-1].shape).astype(np.float32) * 0.1
    yb = knet.forward_linear(torch.as_tensor(X).to(dev())).cpu().numpy()
    for b in (0, 511, 1026):
        y1 = knet.forward_linear(torch.as_tensor(X[b:b + 1]).to(dev())).cpu().numpy()
        assert np.array_equal(yb[b:b + 1], y1)
    ref = oracle.keynet_forward(oracle.load_golden_layers(z), X[:64])
    assert np.array_equal(yb[:64], ref)


def test_homogeneous_helpers_on_device(golden):
    x = torch.rand(5, 2, 3, 7)
    xl = affine_to_linear(x.to(dev()))
    assert xl.shape == (5, 43) and xl.t().is_contiguous()
    assert np.array_equal(xl.cpu().numpy(), oracle.affine_to_linear(x.numpy()))                # the CPU restatement of keynet/torch.py:65-68
    z = golden('challenge_kat.npz')                                                            # and the reference's own vectors: image -> x_linear
    img = (z['png_red_u8'].astype(np.float32) / np.float32(255.0)).reshape(1, 1, 28, 28)
    assert np.array_equal(affine_to_linear(torch.as_tensor(img).to(dev())).cpu().numpy().ravel(), np.asarray(z['x_linear'], dtype=np.float32).ravel())
    zl = golden('lenet_perm.npz')
    xp = torch.as_tensor(zl['x_plain']).to(dev())
    assert np.array_equal(affine_to_linear(xp).cpu().numpy(), zl['x_linear'])                  # keynet.torch.affine_to_linear's own output (make_golden.py)
    assert np.array_equal(affine_to_linear(xp).cpu().numpy(), oracle.affine_to_linear(zl['x_plain']))
    assert np.array_equal(linear_to_affine(affine_to_linear(xp), tuple(zl['x_plain'].shape)).cpu().numpy(), oracle.linear_to_affine(oracle.affine_to_linear(zl['x_plain']), tuple(zl['x_plain'].shape)))
    back = linear_to_affine(xl, (5, 2, 3, 7))
    assert np.array_equal(back.cpu().numpy(), x.numpy())
    bad = xl.t().contiguous()
    bad[-1, 2] = 1.01
    with pytest.raises(ValueError):
        linear_to_affine(bad.t())


def test_error_conventions():
    W = ksp.SparseMatrix(scipy.sparse.eye(4, dtype=np.float32).tocsr())
    with pytest.raises(AssertionError):
        W.torchdot(torch.ones(5, 2).to(dev()))                 # non-conformal (keynet/sparse.py:605)
    with pytest.raises(_capi.KeynetHipError):
        _capi.Operator.csr((2, 2), [0, 1, 2], [0, 5], [1.0, 2.0])   # column out of range
    y = W.torchdot(torch.ones(4, 2, dtype=torch.float64).to(dev()))   # silent f32 coercion (sparse.py:489-491)
    assert y.dtype == torch.float32


def test_allconvnet_permutation_keynet_reduced_width():
    """BASELINE configs[2] (PermutationKeynet AllConvNet 3x32x32) at reduced channel width (24/48 instead of 96/192; the
    full width is `bench.py --workload allconv`): full stack on the GPU, bit-exact vs the CPU oracle, equal to the plain
    net within the reference's own 1e-5 (test/test_keynet.py:222-261), batch columns independent at batch 512."""
    from keynet_amd.models import AllConvNet
    torch.manual_seed(0)
    net = AllConvNet(batchnorm=False, width=24).eval()
    np.random.seed(0)
    (sensor, knet) = ksys.PermutationKeynet((3, 32, 32), net)
    assert knet.num_parameters() > 16000000
    g = torch.Generator().manual_seed(3)
    x = torch.randn(512, 3, 32, 32, generator=g)
    xc = sensor.fromtensor(x.to(dev())).encrypt().astensor()
    y = knet.forward(xc).reshape(512, 10).cpu().numpy()
    with torch.no_grad():
        yp = net(x).numpy()
    assert np.allclose(y, yp, atol=1e-5), np.abs(y - yp).max()
    # oracle on the first 4 images, layer operators taken from the host-side scipy matrices in stored order
    layers = []
    for (name, c) in knet._keynet.named_children():
        if isinstance(c, KeyedLayer):
            M = c.W._matrix
            layers.append((name, (M.shape, M.indptr, M.indices, M.data), False))
        else:
            layers.append((name, 'relu', False))
    ref = oracle.keynet_forward(layers, xc[:4].cpu().numpy())
    out4 = knet.forward_linear(xc[:4]).cpu().numpy()
    assert np.array_equal(out4, ref)
    assert np.array_equal(knet.forward_linear(xc).cpu().numpy()[:4], ref)      # batch 512 vs batch 4: identical columns
    back = sensor.fromtensor(x[:2]).encrypt().decrypt().astensor()
    assert np.array_equal(back.numpy(), x[:2].numpy())


def test_hip_graph_capture_replay(golden):
    """The whole keyed forward captured in a HIP graph: replays are bit-identical to the eager forward, for new inputs too."""
    z = golden('lenet_perm.npz')
    knet = kio.keynet_from_arrays(z)
    rng = np.random.RandomState(0)
    X = np.concatenate([z['x_cipher']] * 16, axis=0)
    X[:, :-1] += rng.randn(*X[:, :-1].shape).astype(np.float32) * 0.05
    xd = torch.as_tensor(X).to(dev())
    eager = knet.forward_linear(xd).cpu().numpy()
    replay = knet.capture(xd)
    assert np.array_equal(replay(xd).cpu().numpy(), eager)
    X2 = X[::-1].copy()
    out2 = replay(torch.as_tensor(X2).to(dev())).cpu().numpy()
    assert np.array_equal(out2, knet.forward_linear(torch.as_tensor(X2).to(dev())).cpu().numpy())
    assert np.array_equal(out2[::-1], eager)


def test_hip_graph_capture_with_dense_linear():
    """A tolerance-mode key-net whose nn.Linear qualifies for the dense split-K path (kn_dense_create: per-STREAM partial-sum workspace):
    capture must happen on the stream that was warmed up, or the first dense layer inside the capture would hipMalloc (refused)."""
    class Net(_Chain):
        flatten_before = 'fc1'

        def __init__(self):
            super(Net, self).__init__()
            self.conv1 = nn.Conv2d(4, 4, 3, padding=1)
            self.relu1 = nn.ReLU()
            self.fc1 = nn.Linear(4 * 16 * 16, 1024)
            self.relu2 = nn.ReLU()
            self.fc2 = nn.Linear(1024, 10)
    torch.manual_seed(3)
    net = Net().eval()
    np.random.seed(3)
    (sensor, knet) = ksys.TiledPermutationKeynet((4, 16, 16), net, 8, exact=False)
    x = torch.randn(256, 4, 16, 16, generator=torch.Generator().manual_seed(5))
    xc = sensor.fromtensor(x.to(dev())).encrypt().astensor()
    assert knet.fc1.W._dense_device_op(xc.device) is not None                # the layer really is on the dense path
    eager = knet.forward_linear(xc).cpu().numpy()
    replay = knet.capture(xc)
    assert np.array_equal(replay(xc).cpu().numpy(), eager)
    x2 = torch.flip(xc, dims=(0,)).t().contiguous().t()
    assert np.array_equal(replay(x2).cpu().numpy()[::-1], eager)
    with torch.no_grad():
        assert np.allclose(eager[:, :-1], net(x).reshape(256, -1).numpy(), atol=1e-4)


@pytest.mark.parametrize('cin,cout,hw,n_vecs,gain', [(32, 128, 12, 256, False), (48, 192, 8, 128, True), (16, 256, 10, 384, False), (64, 128, 9, 256, True)])
def test_convtaps_bf16x3_kernel_vs_oracle(cin, cout, hw, n_vecs, gain):
    """EXPERIMENTAL path (KN_FLAG_BF16X3): f32 products emulated on the bf16 matrix pipe -- both operands split into three bf16 parts,
    six of the nine cross products, f32 accumulate.  A permutation (+ photometric gain) keyed 3x3 conv in factored form, every layout case of
    the kernel (Cout that does not fill the 128-row tile, one to three batch tiles, 1-4 channel chunks, coefficients, bias column, ReLU):
    within the float-key tolerance of the CPU oracle on the expanded operator (measured: a few 1e-7 on unit-scale data), its homogeneous row
    exact; operands that do not qualify (batch not a multiple of 128) take the f32 kernel bit for bit."""
    from keynet_amd import direct as kdirect
    rng = np.random.RandomState(cin + cout + hw + n_vecs)
    HW = hw * hw
    w = (rng.randn(cout, cin, 3, 3) / np.sqrt(9 * cin)).astype(np.float32)
    b = rng.randn(cout).astype(np.float32)
    (pi, po) = (rng.permutation(HW), rng.permutation(HW))
    (g_out, g_in) = ((rng.rand(HW) + 0.5).astype(np.float32), (rng.rand(HW) + 0.5).astype(np.float32))
    (eo, ei, et, ec) = ([], [], [], [])
    for (t, ((i, j), S)) in enumerate(kdirect.shift_matrices((hw, hw), 3, 1)):
        S = S.tocoo()
        eo.append(po[S.row]); ei.append(pi[S.col]); et.append(np.full(S.nnz, t)); ec.append((g_out[po[S.row]] / g_in[pi[S.col]]).astype(np.float32))
    taps = np.stack([w[:, :, i, j] for i in range(3) for j in range(3)])
    lastcol = np.concatenate((np.repeat(b, HW), [1.0])).astype(np.float32)
    W = ksp.Conv2dTiledMatrix.fromtaps((cin, hw, hw), (cout, hw, hw), taps, np.concatenate(eo).astype(np.int32), np.concatenate(ei).astype(np.int32),
                                       np.concatenate(et).astype(np.int32), np.concatenate(ec) if gain else None, lastcol)
    X = np.vstack((rng.randn(cin * HW, n_vecs).astype(np.float32), np.ones((1, n_vecs), np.float32)))
    xd = torch.as_tensor(X).to(dev())
    M = W.rows_csr()
    ref = oracle.csr_matvecs(M.shape, M.indptr, M.indices, M.data.astype(np.float32), X)
    scale = float(np.abs(ref).max())
    assert 'convtaps_bf16x3_kernel' in W._device_op().plan(n_vecs, _capi.KN_FLAG_BF16X3)
    for relu in (False, True):
        r = np.maximum(ref, 0) if relu else ref
        yb = W.torchdot(xd, relu=relu, exact='bf16x3').cpu().numpy()
        err = float(np.abs(yb - r).max())
        assert err <= 1e-5 * max(1.0, scale), (err, scale)
        assert np.array_equal(yb[-1], r[-1])                                     # homogeneous row
    # not a multiple of 128 columns: the flag is ignored, the f32 MFMA kernel runs
    n2 = n_vecs - 28
    assert 'bf16x3' not in W._device_op().plan(n2, _capi.KN_FLAG_BF16X3)
    x2 = xd[:, :n2].contiguous()
    assert torch.equal(W.torchdot(x2, exact='bf16x3'), W.torchdot(x2, exact=False))
    # KN_FLAG_EXACT wins over the flag
    op = W._device_op()
    y1 = torch.empty((W.shape[0], n_vecs), device=dev())
    op.spmm(xd.data_ptr(), n_vecs, n_vecs, y1.data_ptr(), n_vecs, _capi.KN_FLAG_EXACT | _capi.KN_FLAG_BF16X3, torch.cuda.current_stream().cuda_stream)
    assert np.array_equal(y1.cpu().numpy(), ref)


def test_contract_with_bf16x3_candidate():
    """KeyedModel.exact_mode('auto-bf16x3') (opt-in): conv layers that qualify try the bf16x3 kernel first and keep it only with 4x headroom under
    the tolerance on the calibration batch; the default contract never selects it; whatever is selected, every layer stays within 1e-5 of the
    order-preserving path and the logits equal the source network."""
    class Net(_Chain):
        flatten_before = 'fc1'

        def __init__(self):
            super(Net, self).__init__()
            self.conv1 = nn.Conv2d(16, 128, 3, padding=1)
            self.relu1 = nn.ReLU()
            self.conv2 = nn.Conv2d(128, 128, 3, padding=1)
            self.relu2 = nn.ReLU()
            self.pool2 = nn.AvgPool2d(3, stride=2, padding=1)
            self.fc1 = nn.Linear(128 * 4 * 4, 10)
    torch.manual_seed(11)
    net = Net().eval()
    np.random.seed(11)
    (sensor, knet) = ksys.TiledPermutationKeynet((16, 8, 8), net, 4, exact='auto')     # the matrix-core opt-in (the default of a permutation-only key-net is bit-exact)
    x = torch.randn(256, 16, 8, 8, generator=torch.Generator().manual_seed(3))
    xc = sensor.fromtensor(x.to(dev())).encrypt().astensor()
    y_auto = knet.forward_linear(xc)
    assert all(c._exact in (True, False) for c in knet._keynet.children() if isinstance(c, KeyedLayer))      # default: never bf16x3
    knet.exact_mode(True)
    y_exact = knet.forward_linear(xc)
    knet.exact_mode('auto-bf16x3')
    y_b = knet.forward_linear(xc)
    assert knet.conv1._exact == 'bf16x3' and knet.conv2._exact == 'bf16x3', knet.contract_report()
    rec = knet.conv2._contract_record
    assert rec['decided'] == 'bf16x3' and rec['measured_bf16x3_vs_exact'] <= 0.25 * rec['tol']
    scale = max(1.0, float(y_exact.abs().max()))
    assert float((y_b - y_exact).abs().max()) <= 2e-5 * scale and float((y_auto - y_exact).abs().max()) <= 2e-5 * scale
    with torch.no_grad():
        assert np.allclose(y_b[:, :-1].cpu().numpy(), net(x).reshape(256, -1).numpy(), atol=1e-4)
    assert torch.equal(y_b, knet.forward_linear(xc))                               # decided: repeatable
    knet.exact_mode(None)
    assert knet.conv1._exact == 'auto' and not knet.conv1._allow_bf16x3


@pytest.mark.parametrize('n_vecs', [1, 3, 4, 10, 64, 1027])
def test_whole_net_kernel_vs_oracle_random(n_vecs):
    """kn_chain_create / the whole-net kernel on random non-canonical operators that exercise every layout case: rows of unequal length
    inside one wavefront slice, empty rows, duplicate columns, groups of rows sharing one unsorted column sequence (shared column copy),
    unrelated rows (per-lane columns), thin layers (1, 2 and 4 batch columns per lane), ReLU on and off, ragged batches -- bit-equal to
    the CPU oracle applied operator by operator, and to the launch-per-layer kernels."""
    rng = np.random.RandomState(100 + n_vecs)

    def rand_csr(rows, cols, kind):
        (ip, ix, dt) = ([0], [], [])
        shared = None
        for r in range(rows):
            if kind == 'grouped':
                if r % 7 == 0:
                    shared = rng.randint(0, cols, size=rng.randint(1, 40))
                c = shared
            elif kind == 'dense':
                if shared is None:
                    shared = rng.permutation(cols)
                c = shared if r % 11 else shared[:-1]                   # one row in eleven lost an entry: its own pattern
            else:
                c = rng.randint(0, cols, size=(0 if r % 13 == 5 else rng.randint(1, 14)))
            ix.extend(int(v) for v in c)
            dt.extend(rng.randn(len(c)).astype(np.float32))
            ip.append(len(ix))
        return (np.array(ip, np.int32), np.array(ix, np.int32), np.array(dt, np.float32))
    shapes = [(301, 97, 'grouped', 1), (150, 301, 'loose', 0), (70, 150, 'dense', 1), (33, 70, 'dense', 1), (9, 33, 'dense', 0)]
    ops = []
    mats = []
    for (r, c, kind, relu) in shapes:
        (ip, ix, dt) = rand_csr(r, c, kind)
        mats.append(((r, c), ip, ix, dt, relu))
        ops.append(_capi.Operator.csr((r, c), ip, ix, dt))
    chain = _capi.Operator.chain(ops, [m[4] for m in mats])
    assert chain.shape() == (9, 97) and 'chain_kernel' in chain.plan(n_vecs)
    X = rng.randn(97, n_vecs).astype(np.float32)
    ld = n_vecs + 5                                                         # a column window of a wider block, unaligned
    xd = torch.zeros((97, ld), device=dev())
    xd[:, :n_vecs] = torch.as_tensor(X).to(dev())
    yd = torch.full((9, ld), 7.0, device=dev())
    chain.spmm(xd.data_ptr(), ld, n_vecs, yd.data_ptr(), ld, _capi.KN_FLAG_EXACT, torch.cuda.current_stream().cuda_stream)
    ref = X
    per = torch.as_tensor(X).to(dev())
    for ((shape, ip, ix, dt, relu), op) in zip(mats, ops):
        ref = oracle.csr_matvecs(shape, ip, ix, dt, ref)
        if relu:
            ref = np.maximum(ref, 0)
        nxt = torch.empty((shape[0], n_vecs), device=dev())
        op.spmm(per.data_ptr(), n_vecs, n_vecs, nxt.data_ptr(), n_vecs, _capi.KN_FLAG_EXACT | (_capi.KN_FLAG_RELU if relu else 0), torch.cuda.current_stream().cuda_stream)
        per = nxt
    got = yd.cpu().numpy()
    assert np.array_equal(got[:, :n_vecs], ref)
    assert np.array_equal(got[:, n_vecs:], np.full((9, 5), 7.0, np.float32))        # nothing written beyond the batch window
    assert np.array_equal(per.cpu().numpy(), ref)


@pytest.mark.parametrize('n_vecs', [256, 37])
def test_patched_group_members_vs_oracle(n_vecs):
    """Rows that are their pattern group's column sequence minus a few entries (a keyed conv row that lost a weight to an exact zero: AllConvNet
    conv5) ride in the group with 0.0f at the missing positions -- bit-equal to the CPU oracle on the rows' OWN stored sequences; and where the
    activation at a missing position is Inf / NaN the guard kernel restores exactly what the reference computes (no 0 * Inf leak)."""
    rng = np.random.RandomState(11 + n_vecs)
    (n_cols, n_groups, members, seq_len) = (700, 9, 21, 70)
    (ip, ix, dt) = ([0], [], [])
    patched_missing = []
    for g in range(n_groups):
        seq = rng.permutation(n_cols)[:seq_len]                                   # unsorted shared sequence
        for m in range(members):
            keep = np.ones(seq_len, bool)
            if m in (3, 7, 20):                                                  # lose 1..3 entries: first, last and middle positions all occur
                lose = {3: [0], 7: [seq_len - 1, 5], 20: [1, 30, 31]}[m]
                keep[lose] = False
                patched_missing.append((len(ip) - 1, seq[lose]))
            if m == 11:
                keep[rng.choice(seq_len, 6, replace=False)] = False              # too many missing: stays a row of its own
            c = seq[keep]
            ix.extend(int(v) for v in c)
            dt.extend(rng.randn(len(c)).astype(np.float32))
            ip.append(len(ix))
    for _ in range(13):                                                          # unrelated rows
        c = rng.randint(0, n_cols, size=rng.randint(0, 9))
        ix.extend(int(v) for v in c)
        dt.extend(rng.randn(len(c)).astype(np.float32))
        ip.append(len(ix))
    shape = (len(ip) - 1, n_cols)
    (ip, ix, dt) = (np.array(ip, np.int32), np.array(ix, np.int32), np.array(dt, np.float32))
    op = _capi.Operator.csr(shape, ip, ix, dt)
    plan = op.plan(n_vecs, _capi.KN_FLAG_EXACT)
    assert 'csr_patch_guard_kernel<%d patched rows>' % len(patched_missing) in plan, plan
    X = rng.randn(n_cols, n_vecs).astype(np.float32)
    for relu in (0, 1):
        for poison in (False, True):
            Xp = X.copy()
            if poison:
                (r0, miss0) = patched_missing[0]
                (r1, miss1) = patched_missing[4]
                Xp[miss0[0], 1] = np.inf                                        # at a missing position of a patched row: must NOT reach that row
                Xp[miss1[-1], 2] = np.nan
                Xp[ix[ip[r0]], 3] = -np.inf                                     # at a present position: must reach it
            xd = torch.as_tensor(Xp).to(dev())
            yd = torch.empty((shape[0], n_vecs), device=dev())
            op.spmm(xd.data_ptr(), n_vecs, n_vecs, yd.data_ptr(), n_vecs, _capi.KN_FLAG_EXACT | (_capi.KN_FLAG_RELU if relu else 0), torch.cuda.current_stream().cuda_stream)
            with np.errstate(invalid='ignore', over='ignore'):
                ref = oracle.csr_matvecs(shape, ip, ix, dt, Xp)
                if relu:
                    ref = np.where(ref < 0, np.float32(0), ref)
            got = yd.cpu().numpy()
            assert np.array_equal(got, ref, equal_nan=True), (relu, poison, np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))[:5])
            if poison:
                assert np.isfinite(ref[r0, 1]) and np.isfinite(got[r0, 1]) and (relu or not np.isfinite(got[r0, 3]))


def test_explicit_tile_loop_on_device(golden):
    """SURVEY 8(a) row a10 (keynet/torch.py:173-184): keynet_amd.torch.TiledMatrix._torchdot applies the tiles in the loop's own order on the
    device -- bit-equal to the serial loop of the oracle, for a device tensor and for a numpy operand."""
    from keynet_amd.torch import TiledMatrix as TorchTiled
    from test_oracle_golden import _tile_list
    z = golden('tiled_cases.npz')
    names = sorted({k.split('.')[1] for k in z.files if k.startswith('C.') and k.endswith('.tile_ptr')})
    for n in names:
        p = 'C.%s.' % n
        (shape, tileshape, blocks, tiles) = (tuple(int(v) for v in z[p + 'shape']), tuple(int(v) for v in z[p + 'tileshape']), z[p + 'blocks'], _tile_list(z, p))
        ref = oracle.tiled_torchdot_loop(z[p + 'x'], tileshape, shape, tiles, blocks)
        y = TorchTiled._torchdot(torch.as_tensor(z[p + 'x']).to(dev()), tileshape, shape, tiles, blocks)
        assert y.is_cuda and np.array_equal(y.cpu().numpy(), ref), n
        assert np.array_equal(TorchTiled._torchdot(np.asarray(z[p + 'x']), tileshape, shape, tiles, blocks), ref), n
    with pytest.raises(AssertionError):
        TorchTiled._torchdot(torch.zeros(3, 2, device=dev()), (2, 2), (4, 4), [np.zeros((0, 3))], [])


# the layer builders of the whole-net kernel's tests (below, and tests/test_value_classes_gpu.py): (indptr, indices, data) drawn from `rng`
def _chain_grouped(rng, rows, cols, group, nnz, tail_loose):
    (ip, ix, dt) = ([0], [], [])
    shared = None
    for r in range(rows):
        if r >= rows - tail_loose:
            c = rng.randint(0, cols, size=rng.randint(1, 6))         # the odd rows at the end: patterns of their own (e.g. the homogeneous row)
        else:
            if r % group == 0:
                shared = rng.randint(0, cols, size=nnz)
            c = shared
        ix.extend(int(v) for v in c)
        dt.extend(rng.randn(len(c)).astype(np.float32))
        ip.append(len(ix))
    return (np.array(ip, np.int32), np.array(ix, np.int32), np.array(dt, np.float32))


def _chain_dense(rng, rows, cols, seq_len=None):
    perm = rng.permutation(cols)[:seq_len]
    (ip, ix, dt) = ([0], [], [])
    for r in range(rows):
        ix.extend(int(v) for v in perm)
        dt.extend(rng.randn(len(perm)).astype(np.float32))
        ip.append(len(ix))
    return (np.array(ip, np.int32), np.array(ix, np.int32), np.array(dt, np.float32))


def _chain_dense_plus(rng, rows, cols, n_other):
    """A keyed Linear as the reference stores it: `rows - n_other` rows sharing one permuted column sequence + n_other rows of their own (the homogeneous row ...)."""
    (ip, ix, dt) = _chain_dense(rng, rows - n_other, cols)
    (ip, ix, dt) = (list(ip), list(ix), list(dt))
    for _ in range(n_other):
        c = rng.choice(cols, size=rng.randint(1, 4), replace=False)
        ix.extend(int(v) for v in c)
        dt.extend(rng.randn(len(c)).astype(np.float32))
        ip.append(len(ix))
    return (np.array(ip, np.int32), np.array(ix, np.int32), np.array(dt, np.float32))


def test_whole_net_kernel_layout_choices_vs_oracle():
    """The whole-net kernel's per-layer layout choices, each against the CPU oracle bit for bit: conv-like layers (groups of rows sharing an
    unsorted column sequence) with their pattern pool in LDS -- including a last slice of unrelated rows that is stored the same way --, a
    conv-like layer whose pool does NOT fit beside the activations (columns from memory), and a Linear on the thin walk behind them."""
    rng = np.random.RandomState(7)
    (grouped, dense, dense_plus) = (functools.partial(_chain_grouped, rng), functools.partial(_chain_dense, rng), functools.partial(_chain_dense_plus, rng))

    def run(layers, want):
        (ops, mats) = ([], [])
        for (shape, (ip, ix, dt), relu) in layers:
            mats.append((shape, ip, ix, dt, relu))
            ops.append(_capi.Operator.csr(shape, ip, ix, dt))
        chain = _capi.Operator.chain(ops, [m[4] for m in mats])
        n_vecs = 37
        assert want in chain.plan(n_vecs), chain.plan(n_vecs)
        X = rng.randn(layers[0][0][1], n_vecs).astype(np.float32)
        X[3, 5] = np.inf                                                     # non-finite activations travel exactly where the reference's entries carry them
        X[4, 6] = np.nan
        xd = torch.as_tensor(X).to(dev())
        yd = torch.empty((layers[-1][0][0], n_vecs), device=dev())
        chain.spmm(xd.data_ptr(), n_vecs, n_vecs, yd.data_ptr(), n_vecs, _capi.KN_FLAG_EXACT, torch.cuda.current_stream().cuda_stream)
        ref = X
        for (shape, ip, ix, dt, relu) in mats:
            with np.errstate(invalid='ignore', over='ignore'):
                ref = oracle.csr_matvecs(shape, ip, ix, dt, ref)
                if relu:
                    ref = np.where(ref < 0, np.float32(0), ref)              # torch relu: NaN stays NaN
        assert np.array_equal(yd.cpu().numpy(), ref, equal_nan=True)

    # (round 6: a thin layer BEHIND another layer is walked sequentially -- the layer before it writes its output in the thin layer's stored column order)
    run([((645, 200), grouped(645, 200, 6, 11, 5), 1), ((130, 645), grouped(130, 645, 16, 50, 2), 0), ((70, 130), dense(70, 130), 1), ((10, 70), dense(10, 70), 0)],
        '4 operators (2 on the thin walk -- 2 of them sequentially, 2 with column patterns in LDS)')
    # the same with the rows a keyed Linear really has: a homogeneous row (and two more odd ones) beside the shared pattern, pattern lengths 4 k + 1 .. 4 k + 3 (a tail of
    # 1-3 entries), a Linear of more than 64 main rows (two slices = four sequential wavefronts + one for the odd rows), Inf / NaN activations under the odd rows
    run([((645, 200), grouped(645, 200, 6, 11, 5), 1), ((131, 645), grouped(131, 645, 16, 50, 2), 0), ((121, 131), dense_plus(121, 131, 1), 1), ((85, 121), dense_plus(85, 121, 3), 1),
         ((11, 85), dense_plus(11, 85, 1), 0)], '5 operators (3 on the thin walk -- 3 of them sequentially, 2 with column patterns in LDS)')
    # a Linear as the FIRST operator reads the caller's input as it is: the staged-pool thin walk; the one behind it is sequential
    run([((70, 130), dense(70, 130), 1), ((10, 70), dense_plus(10, 70, 1), 0)], '2 operators (2 on the thin walk -- 1 of them sequentially, 0 with column patterns in LDS)')
    # 4200 + 4100 features of four columns = 133 KB of activations; 700 patterns of 28 quads = 314 KB: no room for the pool
    run([((4100, 4200), grouped(4100, 4200, 6, 110, 2), 1), ((64, 4100), grouped(64, 4100, 8, 9, 0), 0)],
        '2 operators (0 on the thin walk -- 0 of them sequentially, 1 with column patterns in LDS), 0 with two rows per lane')
    # conv layers of >= 1024 rows whose patterns hold several rows each: TWO rows per lane (they share every activation read).  Groups of 6 (three
    # lanes per pattern), of 11 (an odd row left over per pattern: a half-empty lane), of 16; 1 .. 9 unrelated rows at the end (lanes of their own, among
    # them the homogeneous row); row lengths that are not a multiple of four; a pooling layer (general walk) and a Linear (thin walk) behind them, so
    # the pools of layers 0, 2 and 3 are staged a layer early and layer 1 runs while layer 2's pool is being written.
    run([((2051, 300), grouped(2051, 300, 6, 11, 5), 1), ((1300, 2051), grouped(1300, 2051, 1, 7, 0), 0), ((1609, 1300), grouped(1609, 1300, 16, 50, 9), 1),
         ((90, 1609), dense(90, 1609), 1), ((10, 90), dense(10, 90), 0)],
        '5 operators (2 on the thin walk -- 2 of them sequentially, 2 with column patterns in LDS), 2 with two rows per lane, 2 column pools staged a layer early')
    run([((1500, 257), grouped(1500, 257, 11, 13, 1), 0), ((33, 1500), dense(33, 1500), 0)],
        '2 operators (1 on the thin walk -- 1 of them sequentially, 1 with column patterns in LDS), 1 with two rows per lane, 1 column pools staged a layer early')
    # a keyed Linear of long rows as the FIRST operator whose column pool is too large for the thin walk (two patterns of 545 quads): pattern walk with shared value blocks, and the
    # short odd rows of its last slice walk the slice's 2 179 entries from their own one-quad blocks on through everything behind them -- the value array has to reach that far
    # (found by the fuzzer's keyed-Linear layers in round 6: a memory access fault 2.8 MB behind the array)
    run([((336, 2184), dense_plus(336, 2184, 9), 0), ((50, 336), dense_plus(50, 336, 1), 1)],
        '2 operators (1 on the thin walk -- 1 of them sequentially, 1 with column patterns in LDS)')
    # a thin first operator whose column pool would be staged twice: 704 quads, 22.5 KB for the two copies, beside 9 000 + 70 + 1 activations that leave 18.7 KB -- columns
    # from memory (general walk)
    run([((70, 9000), dense(70, 9000, 2800), 0)], '1 operators (0 on the thin walk -- 0 of them sequentially, 0 with column patterns in LDS)')
    # two rows per lane tried and dropped: the 64 rows of one 400-column pattern fill a slice at one row per lane; at two they leave half of it to 32 four-column patterns, each
    # then stored at 100 quads -- a pool of 4 772 quads against 3 175 of room, where the pool of one row per lane takes 1 604
    def pairs():
        short = rng.randint(0, 4000, size=(1500, 4))
        row_cols = [rng.randint(0, 4000, size=400)] * 64 + [c for c in short for _ in range(2)]
        ip = np.concatenate(([0], np.cumsum([len(c) for c in row_cols]))).astype(np.int32)
        return (ip, np.concatenate(row_cols).astype(np.int32), rng.randn(ip[-1]).astype(np.float32))
    run([((3064, 4000), pairs(), 1)], '1 operators (0 on the thin walk -- 0 of them sequentially, 1 with column patterns in LDS), 0 with two rows per lane, 1 column pools staged')
    # two pattern pools (2 504 and 3 004 quads) that fit beside the activations (5 239 quads of room) one at a time only: the second is staged at the start of its own layer
    run([((2000, 3000), grouped(2000, 3000, 8, 40, 0), 1), ((400, 2000), grouped(400, 2000, 8, 240, 0), 0)],
        '2 operators (0 on the thin walk -- 0 of them sequentially, 2 with column patterns in LDS), 1 with two rows per lane, 1 column pools staged a layer early')


def test_whole_net_kernel_shares_value_sequences_between_pixels():
    """Round 6: lanes whose rows carry the SAME value sequence read one copy (a keyed conv stores one weight sequence per output channel and border class).  Two conv-like
    layers of identical structure -- 600 "pixels" of 8 "channels" sharing a column sequence each --: in the first every pixel carries the same 8 value sequences, its rows in a
    DIFFERENT order per pixel (what an output permutation key does); in the second all values are distinct.  Both bit-equal to the oracle; the first asks the L2 for a fraction
    of the second's operator words (kn_spmm_plan prints the figure)."""
    import re
    rng = np.random.RandomState(21)
    (pixels, ch, nnz, cols) = (600, 8, 22, 500)
    base_vals = rng.randn(ch, nnz).astype(np.float32)

    def layer(shared_values):
        order = rng.permutation(pixels * ch)                               # row r = (pixel, channel) in a random order: the output key
        (ip, ix, dt) = ([0], [], [])
        pat = [rng.randint(0, cols, size=nnz) for _ in range(pixels)]
        perm_ch = [rng.permutation(ch) for _ in range(pixels)]
        rows = [None] * (pixels * ch)
        for p in range(pixels):
            for c in range(ch):
                rows[order[p * ch + c]] = (pat[p], base_vals[perm_ch[p][c]] if shared_values else rng.randn(nnz).astype(np.float32))
        for (c_, v_) in rows:
            ix.extend(int(v) for v in c_)
            dt.extend(v_)
            ip.append(len(ix))
        return (np.array(ip, np.int32), np.array(ix, np.int32), np.array(dt, np.float32))

    words = []
    for shared_values in (True, False):
        (ip, ix, dt) = layer(shared_values)
        op = _capi.Operator.csr((pixels * ch, cols), ip, ix, dt)
        chain = _capi.Operator.chain([op], [1])
        plan = chain.plan(12)
        words.append(int(re.search(r'(\d+) B of operator words per workgroup', plan).group(1)))
        X = rng.randn(cols, 12).astype(np.float32)
        xd = torch.as_tensor(X).to(dev())
        yd = torch.empty((pixels * ch, 12), device=dev())
        chain.spmm(xd.data_ptr(), 12, 12, yd.data_ptr(), 12, _capi.KN_FLAG_EXACT, torch.cuda.current_stream().cuda_stream)
        ref = np.maximum(oracle.csr_matvecs((pixels * ch, cols), ip, ix, dt, X), 0)
        assert np.array_equal(yd.cpu().numpy(), ref), shared_values
    assert words[0] < 0.6 * words[1], words


def test_whole_net_kernel_is_what_small_keynets_run(golden, monkeypatch):
    """LeNet_AvgPool (BASELINE configs[0]-[1]) takes the whole-net kernel by default; KeyedModel.CHAIN = False selects the launch-per-layer forward;
    both equal the reference's vectors bit for bit, for the golden batch, a ragged one and 1024 images."""
    z = golden('lenet_perm.npz')
    knet = kio.keynet_from_arrays(z)
    xc = torch.as_tensor(z['x_cipher']).to(dev())
    chain = knet._chain_op(xc.device)
    assert chain is not None and chain.shape() == (11, 785)
    assert '7 operators (3 on the thin walk -- 3 of them sequentially, 2 with column patterns in LDS)' in chain.plan(1024)                       # fc1-fc3: two wavefronts per slice, column pool in LDS
    last = 'Y.%s' % [str(n) for n in z['layer_names']][-1]
    assert np.array_equal(knet.forward_linear(xc).cpu().numpy(), z[last])
    assert np.array_equal(knet.forward_linear(xc[:5]).cpu().numpy(), z[last][:5])
    big = torch.cat([xc] * 128, dim=0)
    yb = knet.forward_linear(big)
    monkeypatch.setattr(ksys.KeyedModel, 'CHAIN', False)
    assert knet._chain_op(xc.device) is None
    assert torch.equal(yb, knet.forward_linear(big))
    assert np.array_equal(knet.forward_linear(xc).cpu().numpy(), z[last])
    monkeypatch.setattr(ksys.KeyedModel, 'CHAIN', True)
    # a tiled key-net (matrix-core conv layers) and a key-net too wide for LDS do not qualify
    assert kio.keynet_from_arrays(golden('mini_tiled_permutation.npz'))._chain_op(xc.device) is None


def test_output_encryption_roundtrip(golden):
    """do_output_encryption=True (keynet/system.py:48-50,135-137; the reference's decrypt call is broken, the intent is one more
    torchdot with the embedding key): logits come back decrypted and equal the plain net."""
    z = golden('lenet_perm.npz')
    net = load_weights(LeNet_AvgPool(), z)
    np.random.seed(0)
    (sensor, knet) = ksys.PermutationKeynet((1, 28, 28), net, do_output_encryption=True)
    assert knet.embeddingkey() is not None
    x = torch.as_tensor(z['x_plain'])
    xc = sensor.fromtensor(x.to(dev())).encrypt().astensor()
    y_cipher = knet.forward_linear(xc)
    y = knet.forward(xc).reshape(8, 10).cpu().numpy()
    assert np.allclose(y, z['logits_plain'], atol=1e-5)
    assert not np.allclose(y_cipher[:, :-1].cpu().numpy(), z['logits_plain'], atol=1e-3)    # still encrypted before the key
    pub = knet.public()
    assert pub.embeddingkey() is None and pub.imagekey() is None


def _random_convtaps(rng, Cin, Cout, H, k, stride, unit, has_last):
    """A conv-taps operator with permuted input / output pixels; `unit=False` adds a second, float-weighted entry to about
    half of the (pixel, tap) pairs (the shape of a non-permutation spatial key)."""
    from keynet_amd import direct as kdirect
    (Ho, HW, HoWo) = (H // stride, H * H, (H // stride) ** 2)
    w = (rng.randn(Cout, Cin, k, k) / np.sqrt(k * k * Cin)).astype(np.float32)
    (pi, po) = (rng.permutation(HW), rng.permutation(HoWo))
    (eo, ei, et, ec) = ([], [], [], [])
    for (t, ((i, j), S)) in enumerate(kdirect.shift_matrices((H, H), k, stride)):
        S = S.tocoo()
        eo.append(po[S.row]); ei.append(pi[S.col]); et.append(np.full(S.nnz, t)); ec.append(np.ones(S.nnz, np.float32))
        if not unit:
            sel = rng.rand(S.nnz) < 0.5
            eo.append(po[S.row][sel]); ei.append(pi[(S.col[sel] + 1) % HW]); et.append(np.full(int(sel.sum()), t))
            ec.append(rng.randn(int(sel.sum())).astype(np.float32))
    (eo, ei, et, ec) = (np.concatenate(eo), np.concatenate(ei), np.concatenate(et), np.concatenate(ec))
    if not unit:                                             # merge duplicate (out, in, tap) triples: the operator forbids them
        key = (eo.astype(np.int64) * HW + ei) * (k * k) + et
        (_, first) = np.unique(key, return_index=True)
        (eo, ei, et, ec) = (eo[first], ei[first], et[first], ec[first])
    taps = np.stack([w[:, :, i, j] for i in range(k) for j in range(k)])
    lastcol = np.concatenate((rng.randn(Cout * HoWo), [1.0])).astype(np.float32) if has_last else None
    return ksp.Conv2dTiledMatrix.fromtaps((Cin, H, H), (Cout, Ho, Ho), taps, eo, ei, et, None if unit else ec, lastcol)


def _check_convtaps_vs_oracle(W, rng, n_vecs, has_last, tag):
    X = rng.randn(W.shape[1], n_vecs).astype(np.float32)
    if has_last:
        X[-1] = 1.0
    xd = torch.as_tensor(X).to(dev())
    M = W.tosparse('csr')
    M.sort_indices()
    ref = oracle.csr_matvecs(M.shape, M.indptr, M.indices, M.data.astype(np.float32), X)
    ye = W.torchdot(xd, exact=True).cpu().numpy()
    assert np.array_equal(ye, ref), 'order-preserving path differs from the oracle'
    for relu in (False, True):
        y = W.torchdot(xd, relu=relu).cpu().numpy()
        r = np.maximum(ref, 0) if relu else ref
        assert close_conditioned(y.T, r.T, (M.shape, M.indptr, M.indices, M.data), X.T), (tag, np.abs(y - r).max())


@pytest.mark.parametrize('Cin,Cout,H,k,stride,n_vecs,unit,has_last', [
    (16, 64, 12, 3, 1, 128, True, True),       # 16 channels per wavefront (enough bundles), one 128-column tile
    (16, 64, 12, 3, 1, 384, True, True),       # 384 columns fill three 128-column tiles (two 256-column tiles would waste a quarter)
    (5, 24, 8, 3, 1, 128, True, True),         # 8 channels per wavefront, odd channel counts, Cout not a multiple of 16
    (3, 64, 10, 3, 1, 128, True, False),       # first-layer shape without a bias column
    (8, 32, 8, 3, 2, 128, True, True),         # stride 2
    (12, 48, 8, 3, 1, 128, False, True),       # float coefficients (stored value = fl(coef * tap)): the COEF instantiations
    (4, 16, 6, 5, 1, 640, False, True),        # five 128-column tiles, 5 x 5 window
])
def test_convtaps_exact_pipeline_on_128_column_tiles(Cin, Cout, H, k, stride, n_vecs, unit, has_last):
    """convtaps_exact_pipe_kernel with TWO batch columns per lane (128-column tiles: what each stream of the overlapped forward hands a conv
    layer at 256 images, and batches that fill 128-column tiles better than 256-column ones): bit-equal to the oracle on the whole expansion,
    bit-equal to the four-columns-per-lane instantiation on the same columns (batch columns are independent), ReLU and a column window of a
    wider block through the C ABI."""
    rng = np.random.RandomState(7 * Cin + Cout + n_vecs)
    W = _random_convtaps(rng, Cin, Cout, H, k, stride, True, has_last)
    if not unit:            # one float coefficient per (output pixel, input pixel) entry, no pixel pair hit twice: the shape of a permutation + gain key
        t = W._taps
        W = ksp.Conv2dTiledMatrix.fromtaps(W._inshape, W._outshape, t['taps'], t['ent_out'], t['ent_in'], t['ent_tap'],
                                           (0.5 + rng.rand(len(t['ent_out']))).astype(np.float32), t['lastcol'])
    with torch.cuda.device(dev()):
        plan = W._device_op(dev()).plan(n_vecs, _capi.KN_FLAG_EXACT)
    assert 'convtaps_exact_pipe_kernel' in plan and '128-column tiles' in plan and ('coef' in plan) == (not unit), plan
    X = rng.randn(W.shape[1], 1024).astype(np.float32)
    if has_last:
        X[-1] = 1.0
    M = W.tosparse('csr')
    M.sort_indices()
    ref = oracle.csr_matvecs(M.shape, M.indptr, M.indices, M.data.astype(np.float32), np.ascontiguousarray(X[:, :n_vecs]))
    xd = torch.as_tensor(np.ascontiguousarray(X[:, :n_vecs])).to(dev())
    for relu in (False, True):
        ye = W.torchdot(xd, relu=relu, exact=True).cpu().numpy()
        assert np.array_equal(ye, np.maximum(ref, 0) if relu else ref), (Cin, Cout, n_vecs, relu)
    # the 256-column tiles of the four-columns-per-lane instantiation compute the same columns bit for bit
    xw = torch.as_tensor(X).to(dev())
    with torch.cuda.device(dev()):
        assert '128-column tiles' not in W._device_op(dev()).plan(1024, _capi.KN_FLAG_EXACT)
    yw = W.torchdot(xw, exact=True).cpu().numpy()
    assert np.array_equal(yw[:, :n_vecs], ref)
    # a 128-column window of the 1024-wide block (ldx = ldy = 1024): the overlapped forward's operand
    yd = torch.full((W.shape[0], 1024), 7.0, device=dev())
    c0 = 256
    with torch.cuda.device(dev()):
        W._device_op(dev()).spmm(xw.data_ptr() + 4 * c0, 1024, 128, yd.data_ptr() + 4 * c0, 1024, _capi.KN_FLAG_EXACT, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = yd.cpu().numpy()
    assert np.array_equal(got[:, c0:c0 + 128], yw[:, c0:c0 + 128]) and np.all(got[:, :c0] == 7.0) and np.all(got[:, c0 + 128:] == 7.0)


@pytest.mark.parametrize('Cin,Cout,H,k,n_vecs,unit', [
    (16, 128, 12, 9, 128, True),        # up to 81 slots per pixel = two slot groups (64 + 17), 128 x 128 tiles
    (16, 128, 12, 9, 256, False),       # ... with a float coefficient per slot (the activation tile is scaled on its way to LDS)
    (32, 64, 14, 13, 256, True),        # up to 169 slots = three groups, 64 x 256 tiles, two channel chunks per slot
    (48, 192, 10, 11, 384, False),      # 121 slots, three channel chunks, three batch tiles, Cout over two tiles (the second half empty)
])
def test_convtaps_slot_groups_beyond_64_slots(Cin, Cout, H, k, n_vecs, unit):
    """Fill-in-aware loaders (the reference's doubly-stochastic VGG-16, test/test_keynet.py:116-129, has 500 - 5 400 slots per output
    pixel): a pixel with more than 64 slots is walked slot GROUP by slot group on the wave-uniform-pointer loaders of the matrix-core kernel
    (until round 5 such operators fell to the generic loader: 5-14 TFLOP/s).  Against the order-preserving kernel -- bit-exact with the oracle on
    the whole expansion -- within the conditioned float-key bound, ReLU on and off, and equal to the generic loader (KN_NO_SPTR) to rounding."""
    import os
    rng = np.random.RandomState(Cin + Cout + k)
    W = _random_convtaps(rng, Cin, Cout, H, k, 1, True, True)
    if not unit:
        t = W._taps
        W = ksp.Conv2dTiledMatrix.fromtaps(W._inshape, W._outshape, t['taps'], t['ent_out'], t['ent_in'], t['ent_tap'],
                                           (0.5 + rng.rand(len(t['ent_out']))).astype(np.float32), t['lastcol'])
    slots = np.bincount(W._taps['ent_out'])
    assert slots.max() > 64 and slots.min() < slots.max()                     # border pixels have fewer: groups of every size, pixels with one group too
    with torch.cuda.device(dev()):
        plan = W._device_op(dev()).plan(n_vecs, 0)
    assert 'sptr(wave-uniform pointers, slot groups)' in plan and ('+coef' in plan) == (not unit), plan
    X = rng.randn(W.shape[1], n_vecs).astype(np.float32)
    X[-1] = 1.0
    xd = torch.as_tensor(X).to(dev())
    M = W.tosparse('csr')
    M.sort_indices()
    ref = oracle.csr_matvecs(M.shape, M.indptr, M.indices, M.data.astype(np.float32), X)
    ye = W.torchdot(xd, exact=True).cpu().numpy()
    assert np.array_equal(ye, ref)
    for relu in (False, True):
        y = W.torchdot(xd, relu=relu, exact=False).cpu().numpy()
        r = np.maximum(ref, 0) if relu else ref
        assert close_conditioned(y.T, r.T, (M.shape, M.indptr, M.indices, M.data), X.T), (Cin, Cout, k, relu, np.abs(y - r).max())
    os.environ['KN_NO_SPTR'] = '1'
    try:
        Wg = copy.deepcopy(W)
        Wg._op = None
        yg = Wg.torchdot(xd, exact=False).cpu().numpy()
        with torch.cuda.device(dev()):
            assert 'generic' in Wg._device_op(dev()).plan(n_vecs, 0)
    finally:
        del os.environ['KN_NO_SPTR']
    assert close_conditioned(yg.T, ref.T, (M.shape, M.indptr, M.indices, M.data), X.T)


@pytest.mark.parametrize('Cin,Cout,H,k,n_vecs,unit,has_last,form', [
    (4, 32, 8, 3, 64, False, True, '<taps in registers>'),        # several taps on one (output, input) pixel pair, float coefficients: 9 - 14 slots per pixel, one 64-column tile
    (3, 40, 8, 3, 100, False, True, '<taps in registers>'),       # Cout not a multiple of 32 (second channel block half empty), ragged column tile
    (5, 64, 10, 9, 64, True, True, ''),                           # 81 taps (one value-row load per slot), 81 slots per pixel (two and a bit record batches of 8 per 16), unit coefficients, no pair hit twice
    (2, 33, 10, 9, 256, False, False, ''),                        # > 64 slots AND duplicate pairs, four column tiles, no bias column
    (6, 96, 6, 5, 1, False, True, ''),                            # one batch column (25 taps)
    (16, 128, 6, 3, 192, False, True, '<taps in registers>'),     # VGG-like channel counts, three column tiles
    (2, 128, 28, 3, 128, False, True, '<taps in registers, 64 channels per wavefront>'),     # enough work for the 64-channels-per-wavefront form (784 pixels x 2 channel blocks x 2 column tiles)
    (3, 96, 28, 3, 100, False, False, '<taps in registers, 64 channels per wavefront>'),     # ... with a half-empty second channel block, a ragged column tile and no bias column
    (2, 128, 28, 3, 256, False, True, '<taps in registers, 64 channels per wavefront, two column tiles per wavefront>'),       # round 6: 64 channels x 128 columns per wavefront (784 x 2 x 2 wavefronts)
    (3, 96, 28, 3, 384, False, False, '<taps in registers, 64 channels per wavefront, two column tiles per wavefront>'),       # ... half-empty second channel block, three 128-column tiles, no bias column
    (3, 32, 28, 3, 384, False, True, '<taps in registers, two column tiles per wavefront>'),                                  # 32 channels x 128 columns per wavefront (one channel block: the 64-channel form does not apply)
    (2, 24, 30, 3, 512, False, True, '<taps in registers, two column tiles per wavefront>'),                                  # ... a partial channel block, four 128-column tiles
])
def test_convtaps_exact_fill_kernel_vs_oracle(Cin, Cout, H, k, n_vecs, unit, has_last, form):
    """Filled-in operators in the reference's order (the reference's doubly-stochastic VGG-16, test/test_keynet.py:116-129: 500 - 5 400 slots per
    output pixel, a pixel pair hit by several taps = ONE stored non-zero whose value is the f32 sum of its terms in entry order): convtaps_exact_fill_kernel
    -- stored values formed once per wavefront, products on the matrix pipe, sums on the vector ALU -- is bit-equal to the oracle on the whole expansion
    (scipy's COO -> CSR sums the duplicates in the same order) and to the generic order-preserving kernel (KN_NO_FILL_EXACT=1, a fresh handle), ReLU on and off,
    and through a column window of a wider block.  Round 6: the forms with TWO 64-column tiles per wavefront (batches of whole 128-column tiles) -- bit-equal to the
    oracle and to the one-tile form of the same operator (KN_NO_FILL_TILES2=1, a fresh handle)."""
    import os
    rng = np.random.RandomState(3 * Cin + Cout + k + n_vecs)
    W = _random_convtaps(rng, Cin, Cout, H, k, 1, unit, has_last)
    t = W._taps
    key = t['ent_out'].astype(np.int64) * (H * H) + t['ent_in']
    dups = len(np.unique(key)) < len(key)
    slots = int(np.bincount(t['ent_out']).max())
    assert dups == (not unit) and (dups or slots > 64), (dups, slots)
    with torch.cuda.device(dev()):
        plan = W._device_op(dev()).plan(n_vecs, _capi.KN_FLAG_EXACT)
    assert 'convtaps_exact_fill_kernel' + form + ' (' in plan, plan
    wide = n_vecs + (37 if n_vecs % 128 else 0)                      # (the two-tile forms need an even leading dimension: their window test keeps ldx = n_vecs + 128)
    wide = wide if n_vecs % 128 else n_vecs + 128
    X = rng.randn(W.shape[1], wide).astype(np.float32)
    if has_last:
        X[-1] = 1.0
    xd = torch.as_tensor(X).to(dev())
    M = W.tosparse('csr')
    M.sort_indices()
    ref = oracle.csr_matvecs(M.shape, M.indptr, M.indices, M.data.astype(np.float32), X)
    for relu in (False, True):
        r = np.maximum(ref, 0) if relu else ref
        ye = W.torchdot(xd[:, :n_vecs].contiguous(), relu=relu, exact=True).cpu().numpy()
        assert np.array_equal(ye, r[:, :n_vecs]), (relu, np.abs(ye - r[:, :n_vecs]).max())
    # a column window of the wider block through the C ABI (ldx = ldy = wide; window at column 5 -- or, for the two-tile forms, at column 64: 8-byte aligned rows)
    w0 = 5 if n_vecs % 128 else 64
    yw = torch.full((W.shape[0], wide), -7.0, dtype=torch.float32, device=dev())
    with torch.cuda.device(dev()):
        if 'two column tiles' in form:
            assert 'two column tiles' in W._device_op(dev()).plan(n_vecs, _capi.KN_FLAG_EXACT, ldx=wide, ldy=wide)
        W._device_op(dev()).spmm(xd.data_ptr() + 4 * w0, wide, n_vecs, yw.data_ptr() + 4 * w0, wide, _capi.KN_FLAG_EXACT, torch.cuda.current_stream().cuda_stream)
    yw = yw.cpu().numpy()
    assert np.array_equal(yw[:, w0:w0 + n_vecs], ref[:, w0:w0 + n_vecs]) and np.all(yw[:, :w0] == -7.0) and np.all(yw[:, w0 + n_vecs:] == -7.0)
    if 'two column tiles' in form:
        # an odd window start (4-byte aligned rows only): the dispatch must fall back to one tile per wavefront, same bits
        yo = torch.full((W.shape[0], wide), -7.0, dtype=torch.float32, device=dev())
        with torch.cuda.device(dev()):
            W._device_op(dev()).spmm(xd.data_ptr() + 4 * 5, wide, n_vecs, yo.data_ptr() + 4 * 5, wide, _capi.KN_FLAG_EXACT, torch.cuda.current_stream().cuda_stream)
        assert np.array_equal(yo.cpu().numpy()[:, 5:5 + n_vecs], ref[:, 5:5 + n_vecs])
        os.environ['KN_NO_FILL_TILES2'] = '1'
        try:
            W1 = copy.deepcopy(W)
            W1._op = None
            with torch.cuda.device(dev()):
                p1 = W1._device_op(dev()).plan(n_vecs, _capi.KN_FLAG_EXACT)
            y1 = W1.torchdot(xd[:, :n_vecs].contiguous(), exact=True).cpu().numpy()
        finally:
            del os.environ['KN_NO_FILL_TILES2']
        assert 'convtaps_exact_fill_kernel' in p1 and 'two column tiles' not in p1 and 'no_fill_tiles2=1' in p1, p1
        assert np.array_equal(y1, ref[:, :n_vecs])
    os.environ['KN_NO_FILL_EXACT'] = '1'
    try:
        Wg = copy.deepcopy(W)
        Wg._op = None
        with torch.cuda.device(dev()):
            pg = Wg._device_op(dev()).plan(n_vecs, _capi.KN_FLAG_EXACT)
        yg = Wg.torchdot(xd[:, :n_vecs].contiguous(), exact=True).cpu().numpy()
    finally:
        del os.environ['KN_NO_FILL_EXACT']
    assert 'convtaps_exact_kernel' in pg and 'no_fill_exact=1' in pg, pg
    assert np.array_equal(yg, ref[:, :n_vecs])


def test_convtaps_exact_fill_kernel_sums_a_pairs_terms_in_entry_order():
    """Up to six terms on one (output, input) pixel pair (the doubly-stochastic VGG-16 has nine where a pixel's own key block is concerned): the stored value of
    the pair is fl(...fl(fl(c1 w1) + fl(c2 w2)) + ... ) in ENTRY order (scipy's own COO -> CSR conversion sorts with an unstable sort, so with three or more
    terms it defines no order: the factored operator's entry order is the contract, kn_export_csr and the generic kernel follow it).  The reference here is
    built without the kernel's help: per pair the sequential float32 sum of its terms becomes the single tap of an equivalent duplicate-free operator, whose
    canonical CSR goes through the oracle."""
    rng = np.random.RandomState(11)
    (Cin, Cout, H, n_vecs) = (3, 48, 6, 96)
    HW = H * H
    taps = (rng.randn(9, Cout, Cin) / 3).astype(np.float32)
    (eo, ei, et, ec) = ([], [], [], [])
    for o in range(HW):
        for i in rng.choice(HW, size=rng.randint(1, 9), replace=False):
            k = rng.randint(1, 7)
            for t in rng.choice(9, size=k, replace=False):          # NOT ascending: entry order, not tap order
                eo.append(o); ei.append(i); et.append(t); ec.append(np.float32(rng.randn()))
    (eo, ei, et, ec) = (np.array(eo, np.int32), np.array(ei, np.int32), np.array(et, np.int32), np.array(ec, np.float32))
    lastcol = np.concatenate((rng.randn(Cout * HW), [1.0])).astype(np.float32)
    W = ksp.Conv2dTiledMatrix.fromtaps((Cin, H, H), (Cout, H, H), taps, eo, ei, et, ec, lastcol)
    with torch.cuda.device(dev()):
        plan = W._device_op(dev()).plan(n_vecs, _capi.KN_FLAG_EXACT)
        assert W._device_op(dev()).nnz_expanded() == len(set(zip(eo.tolist(), ei.tolist()))) * Cout * Cin + int(np.count_nonzero(lastcol))
    assert 'convtaps_exact_fill_kernel<taps in registers>' in plan, plan
    # the equivalent duplicate-free operator: one tap per pair, value = the terms' sequential float32 sum in entry order
    order = np.lexsort((np.arange(len(eo)), ei, eo))                # stable: by (out, in), entry order inside a pair
    (pairs, vals) = ([], [])
    for e in order:
        term = (ec[e] * taps[et[e]]).astype(np.float32) if ec[e] != 1.0 else taps[et[e]]
        if pairs and pairs[-1] == (eo[e], ei[e]):
            vals[-1] = (vals[-1] + term).astype(np.float32)
        else:
            pairs.append((eo[e], ei[e]))
            vals.append(term.copy())
    Wd = ksp.Conv2dTiledMatrix.fromtaps((Cin, H, H), (Cout, H, H), np.stack(vals), np.array([q[0] for q in pairs], np.int32), np.array([q[1] for q in pairs], np.int32),
                                        np.arange(len(pairs), dtype=np.int32), None, lastcol)
    M = Wd.tosparse('csr')
    M.sort_indices()
    X = rng.randn(W.shape[1], n_vecs).astype(np.float32)
    X[-1] = 1.0
    ref = oracle.csr_matvecs(M.shape, M.indptr, M.indices, M.data.astype(np.float32), X)
    y = W.torchdot(torch.as_tensor(X).to(dev()), exact=True).cpu().numpy()
    assert np.array_equal(y, ref), np.abs(y - ref).max()
    Mh = W.tosparse('csr')                                         # the host expansion (Conv2dTiledMatrix._expand_taps_host): the same stored values
    Mh.sort_indices()
    assert np.array_equal(Mh.indptr, M.indptr) and np.array_equal(Mh.indices, M.indices) and np.array_equal(Mh.data, M.data.astype(np.float32))
    # kn_export_csr: the same stored values
    E = W._device_op(dev()).export_csr() if hasattr(W._device_op(dev()), 'export_csr') else None
    if E is not None:
        (ip, ix, dt) = E
        assert np.array_equal(ip, M.indptr) and np.array_equal(ix, M.indices) and np.array_equal(dt, M.data.astype(np.float32))


def _filled_in_convtaps(rng, Cin, Cout, H, fill, has_last=True, gentle=False):
    """A factored conv operator shaped like a keyed conv under a key whose inverse is dense inside its blocks: every output pixel reads `fill` input pixels of
    its neighbourhood through each of the nine taps, every entry with its own float coefficient (K_t = a_out S_t a_in^-1)."""
    HW = H * H
    taps = (rng.randn(9, Cout, Cin) / np.sqrt(9 * Cin)).astype(np.float32)
    (eo, ei, et, ec) = ([], [], [], [])
    for t in range(9):
        for o in range(HW):
            ins = rng.choice(HW, size=fill, replace=False)
            eo.append(np.full(fill, o)); ei.append(ins); et.append(np.full(fill, t))
            ec.append(((rng.rand(fill) / fill) if gentle else (rng.randn(fill) / np.sqrt(fill))).astype(np.float32))       # gentle: a well-conditioned averaging key
    lastcol = np.concatenate((rng.randn(Cout * HW), [1.0])).astype(np.float32) if has_last else None
    return ksp.Conv2dTiledMatrix.fromtaps((Cin, H, H), (Cout, H, H), taps, np.concatenate(eo), np.concatenate(ei), np.concatenate(et), np.concatenate(ec), lastcol)


@pytest.mark.parametrize('n_vecs,n_planes,kind', [(64, 5, 'loose'), (256, 3, 'loose'), (128, 4, 'groups'), (100, 7, 'groups'), (64, 2, 'big')])
def test_spmm_planes_is_n_spmm_calls_in_one_launch(n_vecs, n_planes, kind):
    """kn_spmm_planes (round 6): one CSR operator on n activation blocks, grid dimension y = block -- bit-identical to n kn_spmm calls and to the oracle per block, ReLU on and off,
    blocks that are column windows of a wider array (ldx > n_vecs) at plane strides larger than a block; an operator with a big pattern group is refused (the caller loops)."""
    rng = np.random.RandomState(n_vecs + n_planes)
    (m, n) = (700, 300)
    if kind == 'loose':
        M = scipy.sparse.random(m, n, density=0.03, format='csr', random_state=rng, dtype=np.float32)
    elif kind == 'groups':                                        # rows in groups of 9 sharing one column sequence (the taps of one output pixel), plus loose rows
        pats = [np.sort(rng.choice(n, size=rng.randint(5, 40), replace=False)).astype(np.int32) for _ in range(m // 9)]
        lists = [pats[r // 9] if r // 9 < len(pats) and r % 9 < 8 else rng.choice(n, size=rng.randint(0, 12), replace=False).astype(np.int32) for r in range(m)]
        indptr = np.concatenate(([0], np.cumsum([len(v) for v in lists]))).astype(np.int32)
        indices = np.concatenate(lists).astype(np.int32)
        M = scipy.sparse.csr_matrix((rng.randn(len(indices)).astype(np.float32), indices, indptr), shape=(m, n))
    else:                                                         # a dense 300 x 2100 block: ONE big pattern group (>= 256 members, >= 2048 stored columns: a keyed Linear)
        (m, n) = (300, 2100)
        M = scipy.sparse.csr_matrix(rng.randn(m, n).astype(np.float32))
    (ip, ix, dt) = (M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(np.float32))
    op = _capi.Operator.csr((m, n), ip, ix, dt)
    ld = n_vecs + 32
    (xs, ys) = (n * ld + 4 * ld, m * ld + 8 * ld)                  # plane strides (floats): blocks do not overlap, padding between them
    X = rng.randn(n_planes * xs).astype(np.float32)
    xd = torch.as_tensor(X).to(dev())
    st = torch.cuda.current_stream().cuda_stream
    for relu in (0, 1):
        yd = torch.full((n_planes * ys,), -7.0, dtype=torch.float32, device=dev())
        with torch.cuda.device(dev()):
            ok = op.spmm_planes(xd.data_ptr() + 4 * 8, ld, xs, n_planes, n_vecs, yd.data_ptr() + 4 * 8, ld, ys, _capi.KN_FLAG_EXACT | relu, st)
        if kind == 'big':
            assert ok is False                                    # refused, nothing launched
            assert bool((yd == -7.0).all())
            return
        assert ok is True
        y = yd.cpu().numpy()
        yl = torch.full((n_planes * ys,), -7.0, dtype=torch.float32, device=dev())
        with torch.cuda.device(dev()):
            for p in range(n_planes):
                op.spmm(xd.data_ptr() + 4 * (p * xs + 8), ld, n_vecs, yl.data_ptr() + 4 * (p * ys + 8), ld, _capi.KN_FLAG_EXACT | relu, st)
        assert np.array_equal(y, yl.cpu().numpy())                # incl. everything outside the windows: untouched
        for p in range(n_planes):
            Xp = X[p * xs:p * xs + n * ld].reshape(n, ld)[:, 8:8 + n_vecs]
            ref = oracle.csr_matvecs((m, n), ip, ix, dt, np.ascontiguousarray(Xp))
            ref = np.maximum(ref, 0) if relu else ref
            got = y[p * ys:p * ys + m * ld].reshape(m, ld)
            assert np.array_equal(got[:, 8:8 + n_vecs], ref), (p, relu)
            assert np.all(got[:, :8] == -7.0) and np.all(got[:, 8 + n_vecs:] == -7.0)


@pytest.mark.parametrize('Cin,Cout,H,fill,n_vecs,has_last', [(16, 64, 6, 5, 128, True), (3, 40, 8, 3, 100, True), (32, 128, 4, 6, 256, False)])
def test_split_application_of_a_filled_in_conv(Cin, Cout, H, fill, n_vecs, has_last):
    """Conv2dTiledMatrix.torchdot(exact='split') (the reference's doubly-stochastic VGG-16): the factored operator sum_t F_t (x) K_t applied as
    Z_t = K_t X per input channel, then Y = sum_t F_t Z_t -- the same product in another association, so held to the float-key bound against the order-preserving
    kernel (bit-exact with the oracle on the whole expansion): ReLU on and off, max |Y| gathered in the second step's epilogue, and the intermediate produced in
    several column windows."""
    rng = np.random.RandomState(Cin + Cout + fill)
    W = _filled_in_convtaps(rng, Cin, Cout, H, fill, has_last)
    assert W.split_capable() and abs(W.fill_factor() - fill) < 1e-9
    X = rng.randn(W.shape[1], n_vecs).astype(np.float32)
    if has_last:
        X[-1] = 1.0
    xd = torch.as_tensor(X).to(dev())
    ye = W.torchdot(xd, exact=True).cpu().numpy()
    M = W.tosparse('csr')
    M.sort_indices()
    assert np.array_equal(ye, oracle.csr_matvecs(M.shape, M.indptr, M.indices, M.data.astype(np.float32), X))      # (pairs hit by several taps: the host expansion sums in entry order too)
    for relu in (False, True):
        slot = torch.zeros(1, dtype=torch.float32, device=dev())
        ys = W.torchdot(xd, relu=relu, exact='split', absmax=slot).cpu().numpy()
        r = np.maximum(ye, 0) if relu else ye
        assert close_conditioned(ys.T, r.T, (M.shape, M.indptr, M.indices, M.data), X.T), (relu, np.abs(ys - r).max())
        assert float(slot) == np.abs(ys).max()
    whole = W.torchdot(xd, exact='split').cpu().numpy()
    wcols = 128 if n_vecs % 128 == 0 else 48                      # whole 128-column tiles where the batch has them (what the product's window rule keeps), else ragged windows
    W.SPLIT_Z_BYTES = 4 * (Cin * 9 * H * H + (1 if has_last else 0)) * wcols
    try:
        parts = W.torchdot(xd, exact='split').cpu().numpy()
    finally:
        del W.SPLIT_Z_BYTES
    assert np.array_equal(parts, whole)                           # batch columns are independent: windows that keep the kernel instantiation change nothing


def test_calibration_takes_the_split_application_for_a_filled_in_layer():
    """KeyedLayer under the float-key contract ('auto'): a filled-in factored conv is offered the split application first; it is measured against the
    order-preserving kernel on the calibration batch like the matrix-core kernel, accepted with 2x headroom, recorded, re-screened, and travels with a saved
    key-net; with ALLOW_SPLIT off the same layer decides between the fused kernels as before."""
    from keynet_amd.layer import KeyedLayer
    rng = np.random.RandomState(5)
    W = _filled_in_convtaps(rng, 16, 64, 6, 20, gentle=True)
    assert W.split_capable(128) and not _filled_in_convtaps(rng, 16, 64, 6, 3).split_capable(128)       # the cost rule: offered where the estimate is under half the fused launch
    L = KeyedLayer.fromoperator(W, 'Conv2d', inshape=W._inshape, outshape=W._outshape, exact='auto')
    x = torch.as_tensor(np.concatenate((rng.randn(128, W.shape[1] - 1), np.ones((128, 1))), axis=1).astype(np.float32)).to(dev())
    y1 = L.forward(x, fuse_relu=True)
    assert L._exact == 'split' and L._contract_record['decided'] == 'split' and L._contract_record['gate_ratio'] <= 0.5 and L.screened()
    ye = W.torchdot(x.t(), relu=True, exact=True).t()
    assert float((y1 - ye).abs().max()) <= 1e-5 * max(1.0, float(ye.abs().max()))
    assert torch.equal(L.forward(x, fuse_relu=True), y1)
    assert not L.rescreen(float(x.abs().max())) and L.rescreen(3 * float(x.abs().max()))
    KeyedLayer.ALLOW_SPLIT = False
    try:
        L2 = KeyedLayer.fromoperator(W, 'Conv2d', inshape=W._inshape, outshape=W._outshape, exact='auto')
        L2.forward(x, fuse_relu=True)
    finally:
        KeyedLayer.ALLOW_SPLIT = True
    assert L2._exact in (True, False) and L2._contract_record['decided'] in ('exact', 'mfma')


@pytest.mark.parametrize('case', range(10))
def test_convtaps_random_shapes(case):
    """Randomised conv-taps operators (odd channel counts, stride 2, 1x1 / 3x3 / 5x5 windows, several float-coefficient
    entries per (pixel, tap), missing bias column, ragged batches that exercise the generic loader):
    MFMA path vs the order-preserving path (bit-exact vs the oracle) within the conditioned 1e-5 bound."""
    rng = np.random.RandomState(100 + case)
    Cin = int(rng.choice([1, 2, 3, 5, 16, 17, 32, 40]))
    Cout = int(rng.choice([1, 3, 8, 33, 64, 65, 130]))
    H = int(rng.choice([4, 6, 8]))
    k = int(rng.choice([1, 3, 5]))
    stride = int(rng.choice([1, 2]))
    n_vecs = int(rng.choice([1, 3, 4, 64, 100, 128, 256, 260]))
    unit = bool(rng.rand() < 0.5)
    has_last = bool(rng.rand() < 0.7)
    W = _random_convtaps(rng, Cin, Cout, H, k, stride, unit, has_last)
    _check_convtaps_vs_oracle(W, rng, n_vecs, has_last, (case, Cin, Cout, H, k, stride, n_vecs, unit))


@pytest.mark.parametrize('Cin,Cout,k,stride,n_vecs,unit,has_last', [
    (3, 64, 3, 1, 256, True, True),      # VGG conv1_1 shape: K = 27 + bias row = 28, the limit of the one-shot kernel
    (1, 64, 3, 1, 512, False, True),     # float coefficients (<= 18 slots per pixel): folded into the tap rows
    (3, 70, 3, 1, 256, True, False),     # no bias column, odd K (zero row pads the last MFMA step), Cout ragged over 2 tiles
    (1, 6, 5, 1, 256, True, True),       # LeNet conv1 shape: K = 25 + 1
    (2, 33, 3, 2, 256, True, True),      # stride 2
    (3, 64, 3, 1, 256, False, True),     # up to 18 slots * 3 channels: too deep for the one-shot kernel, chunked kernel
    (3, 64, 3, 1, 260, True, True),      # ragged batch: not eligible, generic loader
])
def test_convtaps_small_k_path(Cin, Cout, k, stride, n_vecs, unit, has_last):
    """First-layer operators (slots * Cin + bias <= 28) take the one-shot small-K kernel when the batch is a multiple of 256
    (kn_conv.hip convtaps_smallk_kernel); same bar as every other MFMA launch."""
    rng = np.random.RandomState(7 * Cin + k + n_vecs)
    W = _random_convtaps(rng, Cin, Cout, 8, k, stride, unit, has_last)
    _check_convtaps_vs_oracle(W, rng, n_vecs, has_last, (Cin, Cout, k, stride, n_vecs, unit, has_last))


@pytest.mark.parametrize('Cin,H,k,stride,n_vecs,unit,has_last', [
    (3, 32, 3, 1, 512, True, True),      # VGG conv1_1 shape, 2048 work items on 512 persistent workgroups: 4 pipelined pixels each
    (3, 24, 3, 1, 256, True, True),      # 576 pixels: ragged shares per XCD, most workgroups get one or two pixels
    (1, 32, 3, 1, 768, False, True),     # float coefficients scale the activation rows at LDS-write time; 3 batch tiles
    (3, 32, 3, 2, 256, True, False),     # stride 2, no bias column (no homogeneous row in the contraction)
    (2, 40, 3, 1, 256, False, True),     # Cin = 2 with float coefficients: up to 26 contraction rows + bias... or the chunked kernel
])
def test_convtaps_small_k_pipeline(Cin, H, k, stride, n_vecs, unit, has_last):
    """The persistent, software-pipelined small-K kernel (kn_conv.hip convtaps_smallk_pipe_kernel: Cout == 64, contraction <= 28 rows,
    batch a multiple of 256) on enough pixels that every workgroup walks several of them with stores, gathers and MFMAs of
    neighbouring pixels in flight together: same bar as every MFMA launch against the oracle, and (unit coefficients) bit-identical
    to the one-shot kernel it replaces (same K order, same MFMA shape; KN_NO_SMALLK_PIPE selects the old kernel for the comparison)."""
    import os
    rng = np.random.RandomState(100 * Cin + H + n_vecs)
    W = _random_convtaps(rng, Cin, 64, H, k, stride, unit, has_last)
    _check_convtaps_vs_oracle(W, rng, n_vecs, has_last, (Cin, H, k, stride, n_vecs, unit, has_last))
    X = rng.randn(W.shape[1], n_vecs).astype(np.float32)
    if has_last:
        X[-1] = 1.0
    xd = torch.as_tensor(X).to(dev())
    for relu in (False, True):
        y_pipe = W.torchdot(xd, relu=relu)
        os.environ['KN_NO_SMALLK_PIPE'] = '1'              # recorded at create: a second handle of the same operator
        try:
            W1 = copy.deepcopy(W)
            W1._op = None
            y_one = W1.torchdot(xd, relu=relu)
        finally:
            os.environ.pop('KN_NO_SMALLK_PIPE', None)
        if unit:       # float coefficients: the one-shot kernel scales the tap rows, the pipeline the activation rows (both within the bar above)
            assert torch.equal(y_pipe, y_one), (Cin, H, relu)
        else:
            assert float((y_pipe - y_one).abs().max()) <= 1e-5 * max(1.0, float(y_one.abs().max()))
    y2 = W.torchdot(xd)                                         # repeated launches reuse nothing stale (LDS tables, descriptors)
    assert torch.equal(y2, W.torchdot(xd))


def _keyed_vs_plain(net, inshape, n, factory_kwargs, atol):
    """The reference's own integration criterion (test/test_keynet.py): keyed logits == source-network logits."""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        (sensor, knet) = ksys.Keynet(inshape, net, **factory_kwargs)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, *inshape, generator=g)
    y = knet.forward(sensor.fromtensor(x.to(dev())).encrypt().astensor()).reshape(n, -1).cpu().numpy()
    with torch.no_grad():
        yp = net(x).numpy()
    assert np.allclose(y, yp, atol=atol), (factory_kwargs, np.abs(y - yp).max())
    return knet


@pytest.mark.parametrize('kw,atol', [
    (dict(global_photometric='uniform_random_gain', beta=1.0), 1e-5),                  # test_keynet.py:70-71
    (dict(global_photometric='uniform_random_bias', gamma=1.0), 1e-5),                 # :74-75
    (dict(global_photometric='uniform_random_affine', beta=1.0, gamma=1.0), 1e-4),     # :78-79
    (dict(global_geometric='permutation', memoryorder='block', blocksize=14), 1e-5),   # :59-61
])
def test_photometric_and_block_order_keynets(kw, atol):
    torch.manual_seed(0)
    np.random.seed(1)
    _keyed_vs_plain(LeNet_AvgPool().eval(), (1, 28, 28), 3, kw, atol)


def test_lenet_orthogonal_untiled():
    """test/test_keynet.py:178-197: hierarchical rotation + global bias + local Givens + local affine, block order, untiled."""
    torch.manual_seed(0)
    np.random.seed(2)
    _keyed_vs_plain(LeNet_AvgPool().eval(), (1, 28, 28), 2,
                    dict(tileshape=None, global_geometric='hierarchical_rotation', hierarchical_blockshape=(2, 2), hierarchical_permute_at_level=(0),
                         global_photometric='uniform_random_bias', local_geometric='givens_orthogonal', alpha=2.0, blocksize=8,
                         local_photometric='uniform_random_affine', beta=1.0, gamma=1.0, memoryorder='block'), 2e-5)


def test_lenet_orthogonal_tiled():
    """test/test_keynet.py:200-219: the same family with tileshape (4,4) (conv layers on the MFMA path, effective tiles 4/2/7)."""
    torch.manual_seed(0)
    np.random.seed(3)
    knet = _keyed_vs_plain(LeNet_AvgPool().eval(), (1, 28, 28), 2,
                           dict(tileshape=(4, 4), global_geometric='hierarchical_permutation', hierarchical_blockshape=(2, 2), hierarchical_permute_at_level=(0, 1),
                                global_photometric='identity', local_geometric='givens_orthogonal', alpha=2.0, blocksize=4,
                                local_photometric='uniform_random_affine', beta=1.0, gamma=1.0, memoryorder='block'), 2e-5)
    assert isinstance(knet._keynet.conv1.W, ksp.Conv2dTiledMatrix) and isinstance(knet._keynet.pool1.W, ksp.TiledMatrix)


@pytest.mark.parametrize('tiled', [False, True])
def test_allconvnet_identity_with_batchnorm(tiled):
    """test/test_keynet.py:241-261: AllConvNet(batchnorm=True) -- batch norms folded into conv3/conv6, the ReLUs that follow
    them keyed on their own (KeyedLayer of an nn.ReLU: key change + ReLU in forward) -- identity keys, optionally tiled (8,8).
    Reduced width (16/32 channels); running statistics randomised so the fold is not trivially the identity."""
    from keynet_amd.models import AllConvNet
    torch.manual_seed(0)
    net = AllConvNet(batchnorm=True, width=16).eval()
    with torch.no_grad():
        for m in (net.conv3_bn, net.conv6_bn):
            m.running_mean.copy_(torch.randn_like(m.running_mean) * 0.1)
            m.running_var.copy_(torch.rand_like(m.running_var) + 0.5)
            m.weight.copy_(torch.rand_like(m.weight) + 0.5)
            m.bias.copy_(torch.randn_like(m.bias) * 0.1)
    np.random.seed(4)
    knet = _keyed_vs_plain(net, (3, 32, 32), 2,
                           dict(tileshape=None if not tiled else (8, 8), global_geometric='identity', hierarchical_blockshape=(2, 2), hierarchical_permute_at_level=(0, 1),
                                global_photometric='identity', local_geometric='identity', alpha=2.0, blocksize=8, local_photometric='identity', beta=1.0, gamma=1.0,
                                memoryorder='channel'), 2e-5)
    names = [n for (n, _) in knet._keynet.named_children()]
    assert 'conv3_bn' not in names and 'dropout3' not in names and 'relu3' in names
    assert isinstance(knet._keynet.relu3, KeyedLayer) and knet._keynet.relu3.iskeyedrelu()      # keyed ReLU after the folded batch norm


def test_filled_in_handle_first_used_from_four_threads_at_once():
    """The slot records of the filled-in order-preserving kernel are built on the device at first use (kn_conv.hip: published only once their data is in HBM -- the round-5
    advisor's finding).  Four host threads, a stream each, call a FRESH handle at the same moment (ctypes drops the GIL inside kn_spmm), some with KN_FLAG_EXACT (fill kernel:
    needs the records) and some on the matrix cores; kn_release_side_tables in between rounds (the next call rebuilds).  Every result equals the lone-stream result, bit for bit."""
    import threading
    rng = np.random.RandomState(5)
    W = _random_convtaps(rng, 8, 64, 8, 3, 1, False, True)
    n_vecs = 128
    d = dev()
    X = rng.randn(W.shape[1], n_vecs).astype(np.float32)
    X[-1] = 1.0
    xd = torch.as_tensor(X).to(d)
    with torch.cuda.device(d):
        assert 'convtaps_exact_fill_kernel' in W._device_op(d).plan(n_vecs, _capi.KN_FLAG_EXACT)
        lone = {}
        for fl in (_capi.KN_FLAG_EXACT, 0):
            y = torch.empty((W.shape[0], n_vecs), device=d)
            W._device_op(d).spmm(xd.data_ptr(), n_vecs, n_vecs, y.data_ptr(), n_vecs, fl, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            lone[fl] = y
    for rnd in range(4):
        W2 = copy.deepcopy(W)
        W2._op = None
        with torch.cuda.device(d):
            op = W2._device_op(d)                                  # fresh handle: no side tables yet
        streams = [torch.cuda.Stream(device=d) for _ in range(4)]
        outs = [None] * 4
        errs = []
        go = threading.Barrier(4)

        def work(k):
            try:
                with torch.cuda.device(d):
                    fl = _capi.KN_FLAG_EXACT if k % 2 == 0 else 0
                    go.wait()
                    for rep in range(3):
                        y = torch.empty((W.shape[0], n_vecs), device=d)
                        op.spmm(xd.data_ptr(), n_vecs, n_vecs, y.data_ptr(), n_vecs, fl, streams[k].cuda_stream)
                        outs[k] = (fl, y)
            except Exception as e:                                 # noqa: BLE001
                errs.append(repr(e))
        ts = [threading.Thread(target=work, args=(k,)) for k in range(4)]
        torch.cuda.synchronize()
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        torch.cuda.synchronize()
        assert not errs, errs
        for (fl, y) in outs:
            assert torch.equal(y, lone[fl]), (rnd, fl)
        with torch.cuda.device(d):
            op.release_side_tables()                               # (device-synchronising; the handle stays usable)
            y = torch.empty((W.shape[0], n_vecs), device=d)
            op.spmm(xd.data_ptr(), n_vecs, n_vecs, y.data_ptr(), n_vecs, _capi.KN_FLAG_EXACT, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert torch.equal(y, lone[_capi.KN_FLAG_EXACT])


@pytest.mark.parametrize('name', ['mini_tiled_permutation.npz', 'mini_tiled_stochastic.npz'])
def test_odd_batches_of_a_tiled_keynet_are_padded_to_whole_tiles(golden, name):
    """Round 6: the conv-taps kernels tile the batch in 128 / 256 columns and their ragged forms are slow (profiles/r06_vgg16_other_batches.txt), so KeyedModel.forward_linear pads
    a device batch of a tiled-conv key-net with zero images to whole multiples of 128.  Every image is its own column: its logits are the same in any batch -- bit for bit under
    the stored-order contract (permutation keys), inside the float-key gate otherwise --, a whole-tile batch is not padded, a host batch takes the same route."""
    z = golden(name)
    knet = kio.keynet_from_arrays(z)
    x = torch.as_tensor(z['x_cipher']).to(dev())
    rng = np.random.RandomState(0)
    big = torch.as_tensor(np.vstack([z['x_cipher'][rng.randint(0, z['x_cipher'].shape[0], size=256)]]).astype(np.float32)).to(dev())
    knet._padded_forwards = 0
    full = knet.forward_linear(big)
    assert knet._padded_forwards == 0 and full.shape[0] == 256
    exact = 'permutation' in name
    for n in (1, 37, 130, 200):
        before = knet._padded_forwards
        y = knet.forward_linear(big[:n])
        assert knet._padded_forwards == before + 1 and y.shape[0] == n
        if exact:
            assert torch.equal(y, full[:n]), n
        else:
            assert bool(torch.all((y - full[:n]).abs() <= 2e-5 + 2e-5 * full[:n].abs())), n
    # the reference vectors still come out (batch of the golden file: not a multiple of 128 either)
    y = knet.forward_linear(x).cpu().numpy()
    last = z['Y.%s' % [str(n) for n in z['layer_names']][-1]]
    assert bool(np.all(np.abs(y - last) <= 2e-5 + 2e-5 * np.abs(last)))      # (a key-net loaded from the reference's arrays runs its conv layers on the matrix cores)
    yh = knet.forward_linear(torch.as_tensor(z['x_cipher']))       # host tensor in, host tensor out
    assert not yh.is_cuda and np.array_equal(yh.numpy(), y)


def test_a_batch_too_large_for_32_bit_offsets_runs_in_passes(golden):
    """Round 6: a layer's fast loaders take an activation block of fewer than 2^31 elements; KeyedModel.forward_linear runs a larger batch as passes of whole 256-image tiles
    (VGG-16 in the stored order at 1 024 images: conv1_2 113.7 ms -> 2 x 31 ms).  Here the limit is lowered so that the mini-net's 600 images take three passes: same logits,
    bit for bit, as the one-pass forward; feature-major and row-major batches.
    The real boundary -- blocks at and beyond 2^31 elements through the C ABI, both sides of every launcher guard -- is exercised in tests/test_large_offsets_gpu.py."""
    z = golden('mini_tiled_permutation.npz')
    knet = kio.keynet_from_arrays(z)
    rng = np.random.RandomState(1)
    X = z['x_cipher'][rng.randint(0, z['x_cipher'].shape[0], size=600)].astype(np.float32)
    xr = torch.as_tensor(X).to(dev())                               # row-major
    xf = torch.as_tensor(np.ascontiguousarray(X.T)).to(dev()).t()   # feature-major memory
    one = knet.forward_linear(xf)
    assert getattr(knet, '_chunked_forwards', 0) == 0
    big = max(max(c.W.shape) for c in knet._keynet.children() if hasattr(c, 'W'))
    knet.MAX_BLOCK_ELEMENTS = big * 256 + 1                         # passes of 256 images
    try:
        for x in (xf, xr):
            before = getattr(knet, '_chunked_forwards', 0)
            y = knet.forward_linear(x)
            assert knet._chunked_forwards == before + 1 and y.shape == one.shape
            assert torch.equal(y, one)
    finally:
        del knet.MAX_BLOCK_ELEMENTS


@pytest.mark.parametrize('name', ['mini_tiled_permutation.npz', 'mini_tiled_stochastic.npz', 'lenet_perm.npz'])
def test_graph_capture_at_any_batch_size(golden, name):
    """KeyedModel.capture on batches of 1 / 37 / 128 / 300 images records what the eager forward runs -- a tiled-conv key-net's odd batch padded to whole tiles, once, when
    the graph's input block is prepared: the replayed graph returns the eager logits bit for bit, on the captured input and on other data of the same shape."""
    z = golden(name)
    knet = kio.keynet_from_arrays(z)
    rng = np.random.RandomState(0)
    big = torch.as_tensor(z['x_cipher'][rng.randint(0, z['x_cipher'].shape[0], size=300)].astype(np.float32)).to(dev())
    for n in (1, 37, 128, 300):
        x = big[:n]
        eager = knet.forward_linear(x)
        before = getattr(knet, '_padded_forwards', 0)
        replay = knet.capture(x)
        assert getattr(knet, '_padded_forwards', 0) == before + (1 if (n % 128 and 'tiled' in name) else 0), n
        assert torch.equal(replay(x).clone(), eager), n
        other = big[300 - n:]
        assert torch.equal(replay(other).clone(), knet.forward_linear(other)), n
