"""The bench workloads (host only: no GPU call in this module): BASELINE.json's configs and the reference's float-key VGG-16 tests, keyed under fixed seeds."""
import contextlib
import multiprocessing
import multiprocessing.connection
import time
import traceback

import numpy as np
import torch

from keynet_amd import sparse as ksp
from keynet_amd import system as ksys
from keynet_amd.layer import KeyedLayer
from keynet_amd.models import VGG16, LeNet_AvgPool, AllConvNet
from .common import log

FANOUT_TYPES = (torch.nn.AvgPool2d,)
FANOUT_TIMEOUT_S = 900


class _Pending(torch.nn.Module):
    """Holds a layer's place in the key-net while a forked process keys it (_keying)."""

    def __init__(self, proc, conn):
        super(_Pending, self).__init__()
        (self.proc, self.conn, self.t0) = (proc, conn, time.time())


def _key_in_child(conn, make, args, kw):
    try:
        torch.set_num_threads(1)         # no OpenMP team in a forked child: the parent's threads are not there
        conn.send(('ok', make(*args, **kw)))
    except BaseException as e:
        conn.send(('error', '%s: %s\n%s' % (type(e).__name__, e, traceback.format_exc())))
    finally:
        conn.close()


@contextlib.contextmanager
def _keying(types=()):
    """Inside the block, every layer of a key-net under construction whose source module is one of `types` is keyed in a process forked at that moment
    (its arguments -- the module, the shapes and the two keys, drawn already -- are inherited, not copied); the construction goes on with a _Pending in its
    place.  The keyed VGG-16 spends most of its keying in its five pooling layers, each a pure function of those arguments, so they run side by side and
    behind the rest of the construction.  Yields finish(knet, prepare=None): receives the keyed layers as they complete and puts them in place of the _Pending
    modules; prepare(layer), if given, runs on every keyed layer as soon as it is there -- first on those keyed in this process, then on each forked one as it
    arrives.  With `types` given, the process must not have initialised the GPU when the block starts (a forked child of a HIP process is not safe); prepare
    may, every fork has happened by then."""
    assert not (types and torch.cuda.is_initialized()), 'keying in forked processes: it must run before the GPU is touched'
    ctx = multiprocessing.get_context('fork')
    make = ksys.layergen
    procs = []

    def layergen(module, inshape, outshape, A, Ainv, **kw):
        if not isinstance(module, types):
            return make(module, inshape, outshape, A, Ainv, **kw)
        (mine, theirs) = ctx.Pipe(duplex=False)
        p = ctx.Process(target=_key_in_child, args=(theirs, make, (module, inshape, outshape, A, Ainv), kw), daemon=True)
        p.start()
        theirs.close()
        procs.append(p)
        return _Pending(p, mine)

    def finish(knet, prepare=None):
        pending = {m.conn: (name, m) for (name, m) in knet._keynet.named_children() if isinstance(m, _Pending)}
        if prepare is not None:
            for m in knet._keynet.children():
                if isinstance(m, KeyedLayer):
                    prepare(m)
        deadline = time.time() + FANOUT_TIMEOUT_S
        while pending:
            ready = multiprocessing.connection.wait(list(pending), timeout=max(0.0, deadline - time.time()))
            if not ready:
                raise RuntimeError('keying of %s did not finish in %d s' % (', '.join(n for (n, _) in pending.values()), FANOUT_TIMEOUT_S))
            for conn in ready:
                (name, m) = pending.pop(conn)
                try:
                    (status, layer) = conn.recv()
                except EOFError:
                    (status, layer) = ('error', 'the process keying it exited with %s before sending it' % m.proc.exitcode)
                conn.close()
                m.proc.join()
                if status != 'ok':
                    raise RuntimeError('keying layer "%s" failed: %s' % (name, layer))
                setattr(knet._keynet, name, layer)
                log('[bench] %s keyed in a process of its own in %.1f s' % (name, time.time() - m.t0))
                if prepare is not None:
                    prepare(layer)
        return knet

    if types:
        ksys.layergen = layergen
    try:
        yield finish
    finally:
        ksys.layergen = make
        for p in procs:                                  # nothing keeps running behind a failure
            if p.is_alive():
                p.terminate()
            p.join()


def upload_operators(dev):
    """A prepare() for build_workload: builds on `dev` the device operators the first forward of a key-net under the 'auto' contract builds for the layer
    (KeyedLayer._calibrate: the operator, and for a keyed Linear also its split-K matrix-core form) -- the same handles, only sooner."""
    def prepare(layer):
        W = layer.W
        if type(W) is ksp.SparseMatrix:
            W._dense_device_op(dev)
        W._device_op(dev)
    return prepare


def build_workload(name, rank, exact=None, fanout=False, prepare=None):
    """(sensor, knet, inshape, per_gpu_batch, description, source network).  Deterministic under the seeds, identical on every rank.  `fanout`: key the
    pooling layers in processes of their own (_keying: this process must not have touched the GPU yet).  prepare(layer), if given, runs on every keyed layer
    once it is keyed -- with `fanout`, while the pooling layers are still being keyed."""
    t0 = time.time()
    with _keying(FANOUT_TYPES if fanout else ()) as finish:
        out = _workload(name, exact)
        finish(out[1], prepare)
    log('[bench rank %d] keyed %s on the host in %.1f s%s' % (rank, name, time.time() - t0, '' if prepare is None else ' (operators uploaded as the layers came)'))
    return out


def _workload(name, exact):
    """build_workload's keyed nets under their seeds: (sensor, knet, inshape, per_gpu_batch, description, source network)."""
    if name == 'vgg16':
        torch.manual_seed(0)
        net = VGG16(num_classes=2622).eval()
        np.random.seed(0)
        (sensor, knet) = ksys.TiledPermutationKeynet((3, 224, 224), net, 64, exact=exact)
        (inshape, batch, desc) = ((3, 224, 224), 256, 'TiledPermutationKeynet VGG16(2622) 3x224x224 tile=64 (effective 56/28/14/7)')
    elif name == 'vgg16-gain':
        # the float-key variant of the same config that is constructible at full size: block permutation + block-local photometric gain
        # (every keyed entry carries the coefficient a_out[o] / a_in[i]; 1e-5 contract); orthogonal tile keys fill every tile in
        torch.manual_seed(0)
        net = VGG16(num_classes=2622).eval()
        np.random.seed(0)
        (sensor, knet) = ksys.Keynet((3, 224, 224), net, local_geometric='permutation', local_photometric='uniform_random_gain', beta=0.5,
                                     tileshape=(64, 64), blocksize=64, exact=exact)
        (inshape, batch, desc) = ((3, 224, 224), 256, 'Keynet(permutation + uniform_random_gain, tile=64) VGG16(2622) 3x224x224: float keys')
    elif name == 'vgg16-givens':
        # the reference's OWN float-key VGG-16 configuration (test/test_keynet.py:133-151, test_vgg16_orthogonal): block-local Givens rotations
        # (alpha = 2) + block-local affine photometric keys (beta = gamma = 1), tile = blocksize = 224 // 16 = 14, channel memory order.
        # Keyed directly in factored form (the reference route cannot build it: 15 G non-zeros); fill-in: ~9.0-9.3 slots per output pixel
        # on average, up to 19, every entry carries a coefficient.
        torch.manual_seed(0)
        net = VGG16(num_classes=2622).eval()
        np.random.seed(0)
        (sensor, knet) = ksys.Keynet((3, 224, 224), net, tileshape=(224 // 16, 224 // 16), global_geometric='identity', hierarchical_blockshape=(2, 2),
                                     hierarchical_permute_at_level=(0, 1, 2), local_geometric='givens_orthogonal', alpha=2.0, blocksize=224 // 16,
                                     local_photometric='uniform_random_affine', beta=1.0, gamma=1.0, memoryorder='channel', exact=exact)
        (inshape, batch, desc) = ((3, 224, 224), 256, 'Keynet(givens_orthogonal alpha=2 + uniform_random_affine beta=gamma=1, tile=blocksize=14) VGG16(2622) 3x224x224: '
                                                       'the float-key configuration of test/test_keynet.py:133-151')
    elif name == 'vgg16-givens28':
        # test/test_keynet.py:155-173 (test_vgg16_orthogonal_8): the same float-key family with tile = blocksize = 224 // 8 = 28
        torch.manual_seed(0)
        net = VGG16(num_classes=2622).eval()
        np.random.seed(0)
        (sensor, knet) = ksys.Keynet((3, 224, 224), net, tileshape=(224 // 8, 224 // 8), global_geometric='identity', hierarchical_blockshape=(2, 2),
                                     hierarchical_permute_at_level=(0, 1, 2), local_geometric='givens_orthogonal', alpha=2.0, blocksize=224 // 8,
                                     local_photometric='uniform_random_affine', beta=1.0, gamma=1.0, memoryorder='channel', exact=exact)
        (inshape, batch, desc) = ((3, 224, 224), 256, 'Keynet(givens_orthogonal alpha=2 + uniform_random_affine beta=gamma=1, tile=blocksize=28) VGG16(2622) 3x224x224: '
                                                       'the float-key configuration of test/test_keynet.py:155-173')
    elif name == 'vgg16-stochastic':
        # test/test_keynet.py:116-129 (test_vgg16_stochastic; the reference asserts 1e-5 there): hierarchical block permutation at levels 0, 1, 2 +
        # block-local doubly-stochastic keys (alpha = 2) + affine photometric keys, tile = blocksize = 14.  The INVERSE of a doubly-stochastic block
        # is dense, so every 14 x 14 block of a keyed operator fills in: ~490-560 (first layer of a stage: 1 700-5 400) slots per output pixel instead
        # of 9 -- 60x the multiply-adds of the permutation key-net (0.9 T per image), which is why this workload runs 16 images per step.
        torch.manual_seed(0)
        net = VGG16(num_classes=2622).eval()
        np.random.seed(0)
        (sensor, knet) = ksys.Keynet((3, 224, 224), net, tileshape=(224 // 16, 224 // 16), global_geometric='hierarchical_permutation', hierarchical_blockshape=(2, 2),
                                     hierarchical_permute_at_level=(0, 1, 2), local_geometric='doubly_stochastic', alpha=2.0, blocksize=224 // 16,
                                     local_photometric='uniform_random_affine', beta=1.0, gamma=1.0, memoryorder='channel', exact=exact)
        (inshape, batch, desc) = ((3, 224, 224), 16, 'Keynet(hierarchical_permutation levels 0-2 + doubly_stochastic alpha=2 + uniform_random_affine, tile=blocksize=14) VGG16(2622) '
                                                      '3x224x224: test/test_keynet.py:116-129')
    elif name == 'vgg16-slice':
        # cfg5's topology at a size that keys in seconds (the 21 keyed layers of VGG-16 at width 8 on 32 x 32 inputs, tile 8): what the 8-rank rehearsal test of the
        # tiers runs (tests/test_dist_gpu.py); never a reported number
        torch.manual_seed(0)
        net = VGG16(num_classes=10, width=8, fc_width=64, insize=32).eval()
        np.random.seed(0)
        (sensor, knet) = ksys.TiledPermutationKeynet((3, 32, 32), net, 8, exact=exact)
        (inshape, batch, desc) = ((3, 32, 32), 16, 'TiledPermutationKeynet VGG16 slice (width 8, 3x32x32, tile 8): rehearsal workload, not a BASELINE config')
    elif name == 'lenet':
        torch.manual_seed(0)
        net = LeNet_AvgPool().eval()
        np.random.seed(0)
        (sensor, knet) = ksys.PermutationKeynet((1, 28, 28), net)
        (inshape, batch, desc) = ((1, 28, 28), 1024, 'PermutationKeynet LeNet_AvgPool 1x28x28')
    elif name == 'allconv':
        torch.manual_seed(0)
        net = AllConvNet(batchnorm=False).eval()
        np.random.seed(0)
        (sensor, knet) = ksys.PermutationKeynet((3, 32, 32), net)
        (inshape, batch, desc) = ((3, 32, 32), 4096, 'PermutationKeynet AllConvNet 3x32x32 (BASELINE configs[2])')
    else:
        raise ValueError('unknown workload "%s"' % name)
    return (sensor, knet, inshape, batch, desc, net)
