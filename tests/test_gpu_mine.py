"""Hard-example mining on the GPU (libfplmine.so through ctypes) against the numpy executors
of flypylib_amd/mine.py.

Voxel loss: equal as numbers (-0.0 == 0.0).  The device's double log is within 1 ulp in
double, so rounding it to float32 can - rarely - land on the other neighbour than the
correctly rounded double log numpy takes: up to 1e-6 of the voxels may differ by one float32
ulp, none by more.  Candidate rows and weights: exactly equal, in order."""
import numpy as np
import pytest

from flypylib_amd import fplobjdetect, mine
from tests.mine_cases import mining_case as _mining_case, ulp_distance as _ulp_distance
from tests.trained_fixture import blob_region, trained_network

pytestmark = pytest.mark.gpu

SHAPE, EDGE = (67, 80, 93), (9, 9, 12)
THRESHOLDS = [(None, None), ((0.8, 1.0), None), (None, (0.1, 0.5)), ((0.05, 2.0), (0.1, 0.5))]


def _torch():
    import torch
    return torch


def _dev(a, misalign=False):
    """a resident copy of `a`; misalign: one element past an aligned base, so that the
    kernels' packed loads and stores are not available"""
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')
    if not misalign:
        return t
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    flat[1:] = t.reshape(-1)
    v = flat[1:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % (4 * t.element_size()) != 0
    return v


def _assert_loss(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    dist = _ulp_distance(got, want)
    differ = int((got != want).sum())
    print('%s: %d of %d voxels differ, max %d ulp' % (what, differ, got.size, int(dist.max())))
    assert int(dist[got != want].max(initial=0)) <= 1, what
    assert differ <= 1e-6 * got.size, what


def _case():
    pred, ll, mm = _mining_case(7, SHAPE)
    # exact 0 and 1 (the 1e-8 floor and log(1) = 0), inside the border, for both classes
    pred[20, 30:34, 40:44] = 0.0
    pred[21, 30:34, 40:44] = 1.0
    ll[20:22, 30:32, 40:44] = 0
    ll[20:22, 32:34, 40:44] = 1
    mm[20:22, 30:34, 40:44] = 1
    assert (ll > 1).any() and (mm > 1).any()
    return pred, ll, mm


@pytest.mark.parametrize('misalign', [False, True])
@pytest.mark.parametrize('thresholds', THRESHOLDS)
def test_voxel_loss_kernel_equals_the_numpy_executor(ctx, thresholds, misalign):
    pred, ll, mm = _case()
    want = mine.voxel_loss_numpy(pred, ll, mm, EDGE, *thresholds)
    got = mine.voxel_loss_device(_dev(pred, misalign), _dev(ll, misalign), _dev(mm, misalign),
                                 EDGE, *thresholds, out=_dev(np.full(SHAPE, 7, np.float32), misalign))
    got = got.cpu().numpy()
    _assert_loss(got, want, 'voxel loss %r' % (thresholds,))
    assert (want != 0).sum() > 0.2 * want.size
    # the floor and the exact zero
    floor = np.float32(-np.log(np.float64(np.float32(1e-8))))
    if thresholds == (None, None):
        assert got[20, 30, 40] == 0 and got[21, 30, 40] == floor       # negatives: p = 0, p = 1
        assert got[20, 32, 40] == floor and got[21, 32, 40] == 0       # positives


@pytest.mark.parametrize('shape,edge', [((9, 11, 13), (2, 3, 4)), ((33, 35, 37), (9, 9, 12)),
                                        ((5, 6, 7), (3, 1, 1)), ((1, 1, 3), (0, 0, 0))])
def test_voxel_loss_kernel_on_volumes_that_end_inside_a_group_of_four(ctx, shape, edge):
    pred, ll, mm = _mining_case(9, shape)
    want = mine.voxel_loss_numpy(pred, ll, mm, edge, (0.05, 2.0), (0.1, 0.5))
    got = mine.voxel_loss_device(_dev(pred), _dev(ll), _dev(mm), edge, (0.05, 2.0), (0.1, 0.5))
    _assert_loss(got.cpu().numpy(), want, 'voxel loss %r' % (shape,))


def _assert_rows(got, want, what):
    for g, w, col in zip(got, want, 'zyxw'):
        if w is None:
            assert g is None, (what, col)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, col, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, col)


def _candidates(ll, mm, half, cc, ww, misalign=False):
    want = mine.candidates_numpy(ll, mm, half, cc, ww)
    got = mine.candidates_device(_dev(ll, misalign), _dev(mm, misalign), half, cc,
                                 None if ww is None else _dev(ww, misalign))
    _assert_rows(got, want, (ll.shape, half, cc, ww is not None, misalign))
    return len(want[0])


@pytest.mark.parametrize('misalign', [False, True])
@pytest.mark.parametrize('weighted', [False, True])
def test_compaction_equals_the_numpy_executor(ctx, weighted, misalign):
    """67 x 80 x 93 = 121 chunks and a part of one: the volume ends mid-chunk"""
    _, ll, mm = _mining_case(11, SHAPE)
    ww = None
    if weighted:
        ww = np.random.RandomState(3).uniform(-1, 1, SHAPE).astype(np.float32)
        ww[::3] = 0
        ww[5, 40, 50] = np.nan
    assert np.prod(SHAPE) % 4096 != 0
    for cc in (0, 1, 3):
        n = _candidates(ll, mm, (12, 12, 12), cc, ww, misalign)
        assert n > 100


def test_compaction_edge_cases(ctx):
    rs = np.random.RandomState(5)
    # an empty class, and a class holding every voxel (no border)
    ll = np.zeros(SHAPE, np.uint8)
    mm = np.ones(SHAPE, np.uint8)
    assert _candidates(ll, mm, (12, 12, 12), 1, None) == 0
    assert _candidates(ll, mm, (0, 0, 0), 0, None) == int(np.prod(SHAPE))
    ww = rs.uniform(0.5, 1, SHAPE).astype(np.float32)
    assert _candidates(ll, mm, (0, 0, 0), 0, ww) == int(np.prod(SHAPE))
    assert _candidates(ll, mm, (0, 0, 0), 0, np.zeros(SHAPE, np.float32)) == 0
    # a border that leaves nothing
    assert _candidates(ll, mm, (34, 1, 1), 0, None) == 0
    # volumes smaller than one chunk, one of them not a whole number of groups of four
    for shape in ((9, 11, 13), (8, 8, 8), (1, 1, 1)):
        l2 = (rs.uniform(0, 1, shape) > 0.5).astype(np.uint8)
        m2 = (rs.uniform(0, 1, shape) > 0.2).astype(np.uint8)
        w2 = rs.uniform(-1, 1, shape).astype(np.float32)
        for cc in (0, 1):
            _candidates(l2, m2, (1, 1, 1) if shape[0] > 2 else (0, 0, 0), cc, None)
            _candidates(l2, m2, (0, 0, 0), cc, w2)
    # a volume that ends mid-chunk and mid-group: 33 x 35 x 37 = 10 chunks + 1775 voxels
    shape = (33, 35, 37)
    _, l3, m3 = _mining_case(13, shape)
    w3 = rs.uniform(-1, 1, shape).astype(np.float32)
    for cc in (0, 1):
        assert _candidates(l3, m3, (3, 4, 5), cc, None) > 0
        assert _candidates(l3, m3, (3, 4, 5), cc, w3, misalign=True) > 0
    # exactly one chunk, exactly two
    for shape in ((16, 16, 16), (16, 16, 32)):
        l4 = np.ones(shape, np.uint8)
        assert _candidates(l4, np.ones(shape, np.uint8), (0, 0, 0), 1, None) == int(np.prod(shape))


def _fixture():
    net = trained_network('vgg_like')
    im, ll, _ = blob_region(2, 110)
    mm = np.ones(ll.shape, np.uint8)
    mm[:30, :40, :] = 0
    return net, im, ll, mm


def test_network_voxel_loss_on_the_device_equals_the_numpy_executor_on_its_prediction(ctx):
    torch = _torch()
    net, im, ll, mm = _fixture()
    edge = [int(round(c / 2)) for c in net.rf_size]
    pred = np.array(net.infer(im))
    assert pred.max() > 0.8
    for thresholds in ((None, None), ((0.05, 2.0), (0.1, 0.5))):
        want = mine.voxel_loss_numpy(pred, ll, mm, edge, *thresholds)
        got = net.voxel_loss(im, (ll, mm), *thresholds, device=0)
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float32
        _assert_loss(got.cpu().numpy(), want, 'trained vgg_like %r' % (thresholds,))
        assert (want > 0).sum() > 1000 and (want == 0).sum() > 1000
    # resident labels and mask are taken as they are; labels of another dtype compare alike
    got2 = net.voxel_loss(im, (_dev(ll), _dev(mm)), (0.05, 2.0), (0.1, 0.5), device=0)
    got3 = net.voxel_loss(im, (ll.astype(np.int64), mm.astype(np.float32)), (0.05, 2.0),
                          (0.1, 0.5), device=True)
    assert torch.equal(got, got2) and torch.equal(got, got3)
    # the host path is what it was: numpy in, numpy out
    host = net.voxel_loss(im, (ll, mm), (0.05, 2.0), (0.1, 0.5))
    assert isinstance(host, np.ndarray) and host.dtype == np.float32
    assert np.mean((host == 0) != (want == 0)) < 1e-4


def _same_bytes(a, b, what):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), what


def test_gen_volume2_from_device_mined_weights_equals_gen_volume2_from_host_weights(ctx, tmp_path):
    """write_sampling_weights(device=0) -> gen_volume2(device=0): the tables come from the
    compaction kernels.  The same weights as host arrays -> gen_volume2(device=0): the tables
    come from nonzero().  Same seed, so the same draws and the same gather: identical
    batches.  The thresholds pin every weight to 0, 0.5 or 2: gen_volume2 (host and device
    alike) normalises by a float32 sum that numpy's choice() only accepts when it is exact
    to ~1e-8, the condition tests/batchgen_cases.py meets with whole numbers."""
    torch = _torch()
    net, im, ll, mm = _fixture()
    im2, ll2, _ = blob_region(3, 96)
    train = [(im, ll, mm), (im2, ll2, np.ones(ll2.shape, np.uint8))]
    l0, l1 = (0.5, 0.5), (2.0, 2.0)
    mined = fplobjdetect.write_sampling_weights(train, net, str(tmp_path / 'w'), l0, l1,
                                                device=0, save=True)
    assert all(len(tr) == 4 and tr[3].is_cuda and tr[3].dtype == torch.float32 for tr in mined)
    host = []
    for i, tr in enumerate(mined):
        w = np.load(str(tmp_path / ('w%02d.npy' % i)))
        assert np.array_equal(w, tr[3].cpu().numpy())
        assert set(np.unique(w).tolist()) == {0.0, 0.5, 2.0}
        # after mining the hard examples are a fraction of the volume
        print('volume %d: %d of %d voxels keep a weight' % (i, int((w > 0).sum()), w.size))
        assert 0 < (w > 0).sum() < 0.9 * w.size
        host.append(tuple(tr[:3]) + (w,))
    unsaved = fplobjdetect.write_sampling_weights(train, net, str(tmp_path / 'u'), l0, l1,
                                                  device=0, save=False)
    assert not list(tmp_path.glob('u*')) and torch.equal(unsaved[0][3], mined[0][3])

    args = ((24, 24, 24), 16, 0.6)
    a = fplobjdetect.gen_volume2(mined, *args, noise_aug=[0.05, 0.1],
                                 rng=np.random.RandomState(4), device=0)
    b = fplobjdetect.gen_volume2(host, *args, noise_aug=[0.05, 0.1],
                                 rng=np.random.RandomState(4), device=0)
    c = fplobjdetect.gen_volume2(host, *args, noise_aug=[0.05, 0.1],
                                 rng=np.random.RandomState(4), device=0, tables='device')
    assert a.plan._n == b.plan._n == c.plan._n and min(a.plan._n) > 0
    for x, y in zip(a.plan._cols + a.plan._p, b.plan._cols + b.plan._p):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    # the resident labels the device planner built are the host planner's masked labels
    for x, y in zip(a.plan.labels, b.plan.labels):
        assert x.is_cuda and np.array_equal(x.cpu().numpy(), y)
    assert all(x.data_ptr() == y.data_ptr() for x, y in zip(a._labels, a.plan.labels))
    for i in range(4):
        (da, la), (db, lb), (dc, lc) = next(a), next(b), next(c)
        _same_bytes(da, db, 'data %d' % i)
        _same_bytes(la, lb, 'labels %d' % i)
        _same_bytes(da, dc, 'data %d (tables=device from host arrays)' % i)
        _same_bytes(la, lc, 'labels %d (tables=device from host arrays)' % i)
    # ... and they are the host generator's batches
    h = fplobjdetect.gen_volume2(host, *args, noise_aug=[0.05, 0.1], rng=np.random.RandomState(4))
    for i, (x, y) in enumerate(zip(next(h), next(fplobjdetect.gen_volume2(
            mined, *args, noise_aug=[0.05, 0.1], rng=np.random.RandomState(4), device=0)))):
        assert np.ascontiguousarray(x).tobytes() == y.cpu().numpy().tobytes(), i
