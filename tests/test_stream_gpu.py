"""StreamedForward against the path it is made of: every batch it yields must equal, bit for bit, forward_linear on the sensor's own encrypt of that batch, computed
afterwards and batch by batch.  The batches of a run hold DIFFERENT random frames, so a staging, frame or logits buffer that is re-used too early shows up as a
wrong result.  Nothing here is calibrated ('auto' depends on which batch came first), timed, or made to fail on the device."""
import numpy as np
import pytest
import torch

from benchlegs.workloads import build_workload
from keynet_amd.stream import StreamedForward

pytestmark = pytest.mark.gpu

SIZES = (6, 3, 6, 1, 6, 5, 2)            # batch = 6: full batches, ragged ones, a single image, a ragged last one
NARROW_SIZES = (4, 2, 4, 1, 4, 4, 3)     # batch = 4
NARROW = dict(narrow=True, narrow_rows=True, narrow_taps='pairs')
NETS = {'lenet': ('lenet', None), 'vgg16-slice': ('vgg16-slice', None), 'vgg16-slice-mfma': ('vgg16-slice', False)}

_nets = {}
_refs = {}


def dev():
    return torch.device('cuda:0')


def _net(name):
    """(sensor, model, (C, H, W)) under the workload's seeds; keyed once per session."""
    if name not in _nets:
        (workload, exact) = NETS[name]
        (sensor, model, inshape) = build_workload(workload, 0, exact=exact)[:3]
        _nets[name] = (sensor, model, tuple(inshape))
    return _nets[name]


def _batches(name, sizes):
    """uint8 NHWC frames, one array per batch, different in every batch."""
    (C, H, W) = _net(name)[2]
    rng = np.random.RandomState(len(name) + sum(sizes))
    return [rng.randint(0, 256, size=(n, H, W, C)).astype(np.uint8) for n in sizes]


def _floats(frames):
    return torch.as_tensor(frames).permute(0, 3, 1, 2).contiguous().float()


def _reference(name, sizes, kw):
    """What the existing path gives for every batch of _batches(name, sizes): computed once, shared, left unchanged."""
    key = (name, sizes, tuple(sorted(kw.items())))
    if key not in _refs:
        (sensor, model, _) = _net(name)
        with torch.cuda.device(dev()):
            _refs[key] = [model.forward_linear(sensor.fromtensor(_floats(x)).encrypt().astensor(), **kw).cpu() for x in _batches(name, sizes)]
    return _refs[key]


def _assert_equal(got, name, sizes, kw, upto=None):
    refs = _reference(name, sizes, kw)[:upto]
    assert len(got) == len(refs)
    for (k, (g, r)) in enumerate(zip(got, refs)):
        assert isinstance(g, torch.Tensor) and not g.is_cuda and tuple(g.shape) == tuple(r.shape) == (sizes[k], r.shape[1])
        assert torch.equal(g, r), 'batch %d of %s (%d images) differs from forward_linear on the sensor\'s encrypt' % (k, name, sizes[k])


@pytest.mark.parametrize('frames', ['uint8', 'float32'])
@pytest.mark.parametrize('name', sorted(NETS))
def test_streamed_batches_equal_the_existing_path(name, frames):
    """Seven batches through one pipeline; the consumer keeps every yielded tensor until the end, so a result that aliased a pinned buffer would have been overwritten."""
    (sensor, model, _) = _net(name)
    items = _batches(name, SIZES)
    if frames == 'float32':
        items = [_floats(x) for x in items]
    with torch.cuda.device(dev()):
        with StreamedForward(sensor, model, max(SIZES), frames=frames) as sf:
            got = list(sf.run(items))
        assert sf._buffers is None
    assert len(set(g.data_ptr() for g in got)) == len(got) and not any(g.is_pinned() for g in got)
    _assert_equal(got, name, SIZES, {})


@pytest.mark.parametrize('name', sorted(NETS))
def test_streamed_narrow_forward(name):
    (sensor, model, _) = _net(name)
    with torch.cuda.device(dev()):
        with StreamedForward(sensor, model, max(NARROW_SIZES), **NARROW) as sf:
            got = list(sf.run(iter(_batches(name, NARROW_SIZES))))
    _assert_equal(got, name, NARROW_SIZES, NARROW)


@pytest.mark.parametrize('name', ['lenet', 'vgg16-slice'])
def test_results_compared_as_they_arrive_and_tensor_batches(name):
    """The consumer that looks at each result at once (the pipeline has batch k + 1 in flight then), fed CPU tensors in NCHW."""
    (sensor, model, _) = _net(name)
    refs = _reference(name, SIZES, {})
    with torch.cuda.device(dev()):
        with StreamedForward(sensor, model, max(SIZES), layout='NCHW') as sf:
            items = (torch.as_tensor(x).permute(0, 3, 1, 2) for x in _batches(name, SIZES))          # non-contiguous views: the staging copy lays them out
            for (k, g) in enumerate(sf.run(items)):
                assert torch.equal(g, refs[k]), 'batch %d' % k
            assert k == len(SIZES) - 1


@pytest.mark.parametrize('name', ['lenet', 'vgg16-slice'])
def test_close_in_mid_iteration_then_a_fresh_pipeline(name):
    (sensor, model, _) = _net(name)
    with torch.cuda.device(dev()):
        sf = StreamedForward(sensor, model, max(SIZES))
        run = sf.run(_batches(name, SIZES))
        got = [next(run) for _ in range(3)]
        sf.close()                                                       # batch 3 is computed and batch 4 uploaded at this point
        assert sf._buffers is None and sf._active is None
        with pytest.raises(StopIteration):
            next(run)
        with pytest.raises(RuntimeError):
            sf.run([])
        _assert_equal(got, name, SIZES, {}, upto=3)
        with StreamedForward(sensor, model, max(SIZES)) as again:
            _assert_equal(list(again.run(_batches(name, SIZES))), name, SIZES, {})
        torch.cuda.synchronize()


class _InputBroke(Exception):
    pass


@pytest.mark.parametrize('name', ['lenet', 'vgg16-slice'])
def test_input_that_raises_delivers_what_came_before(name):
    (sensor, model, _) = _net(name)

    def two_then_raise():
        items = _batches(name, SIZES)
        yield items[0]
        yield items[1]
        raise _InputBroke('the camera went away')

    got = []
    with torch.cuda.device(dev()):
        with StreamedForward(sensor, model, max(SIZES)) as sf:
            with pytest.raises(_InputBroke):
                for g in sf.run(two_then_raise()):
                    got.append(g)
            _assert_equal(got, name, SIZES, {}, upto=2)
            # the pipeline is usable after it: a refused batch in mid-run behaves the same way
            items = _batches(name, SIZES)[:2] + [np.zeros((max(SIZES) + 1,) + items_shape(name), np.uint8)]
            got = []
            with pytest.raises(ValueError, match='built for'):
                for g in sf.run(items):
                    got.append(g)
            _assert_equal(got, name, SIZES, {}, upto=2)
        torch.cuda.synchronize()


def items_shape(name):
    (C, H, W) = _net(name)[2]
    return (H, W, C)
