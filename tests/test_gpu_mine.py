"""Hard-example mining on the GPU (libfplmine.so through ctypes) against the numpy executors
of flypylib_amd/mine.py.

Voxel loss: equal as numbers (-0.0 == 0.0).  The device's double log is within 1 ulp in
double, so rounding it to float32 can - rarely - land on the other neighbour than the
correctly rounded double log numpy takes: up to 1e-6 of the voxels may differ by one float32
ulp, none by more.  Candidate rows and weights: exactly equal, in order."""
import functools

import numpy as np
import pytest

from flypylib_amd import _minecapi, fplobjdetect, mine
from tests import mine_cases
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


# ---- more than 1024 chunks, more than one pass of the loss grid, capacity, short rows ------
# (tests/mine_cases.py holds the shapes; tests/test_mine_host.py asserts on the CPU that each
# reaches the path it is named for)

@functools.lru_cache(maxsize=2)
def _scan_case(name, cc=None):
    """(pred, labels, mask, weights), built once for the runs of a case; no test writes to them"""
    return mine_cases.scan_case(name, cc if name == 'scan_one_over' else None)


@functools.lru_cache(maxsize=2)
def _scan_rows(name, half, cc, weighted):
    """candidates_numpy of a scan case"""
    _, ll, mm, ww = _scan_case(name, cc if name == 'scan_one_over' else None)
    want = mine.candidates_numpy(ll, mm, half, cc, ww if weighted else None)
    for a in want[:3]:
        a.setflags(write=False)
    return want


# the non-VEC kernels scan runs too: both classes of the short last run, and the forced ends
MISALIGNED = [('scan_runs_2', (0, 2, 7), 0), ('scan_runs_2', (0, 2, 7), 1),
              ('scan_one_over', (0, 0, 0), 1)]
assert all(c in mine_cases.COMPACTION_CASES for c in MISALIGNED)


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('name,half,cc,misalign',
                         [c + (False,) for c in mine_cases.COMPACTION_CASES] +
                         [c + (True,) for c in MISALIGNED])
def test_compaction_scans_runs_of_chunks(ctx, name, half, cc, misalign, weighted):
    """more than 1024 chunks: a scan thread owns `per` > 1 chunks, the last one fewer, the
    threads behind it none (scan_full: exactly one each)"""
    _, ll, mm, ww = _scan_case(name, cc if name == 'scan_one_over' else None)
    want = _scan_rows(name, half, cc, weighted)
    held, runs = mine_cases.assert_runs_hold_candidates(name, half, weighted, *want[:3])
    print('%s half %r class %d: %d rows, %d of %d runs must hold rows'
          % (name, half, cc, len(want[0]), held, runs))
    got = mine.candidates_device(_dev(ll, misalign), _dev(mm, misalign), half, cc,
                                 _dev(ww, misalign) if weighted else None)
    _assert_rows(got, want, (name, half, cc, weighted, misalign))
    assert len(want[0]) > 10 * runs
    if weighted:
        assert want[3].dtype == np.float32 and (want[3] > 0).all()


LOSS_EDGE = (9, 9, 12)


@functools.lru_cache(maxsize=2)
def _strided_loss(thresholds):
    pred, ll, mm, _ = _scan_case('scan_runs_2')
    want = mine.voxel_loss_numpy(pred, ll, mm, LOSS_EDGE, *thresholds)
    want.setflags(write=False)
    return want


@pytest.mark.parametrize('misalign', [False, True])
@pytest.mark.parametrize('thresholds', [(None, None), ((0.05, 2.0), (0.1, 0.5))])
def test_voxel_loss_kernel_strides_over_a_volume_of_three_passes(ctx, thresholds, misalign):
    """173 x 175 x 177: 1 339 669 groups of four against 524 288 lanes, so a lane takes the
    loop body three times, or twice in the partial last pass, and the volume ends inside a
    group.  `out` is pre-filled, so a voxel no pass reaches fails the comparison."""
    shape = mine_cases.SCAN_SHAPES['scan_runs_2'][0]
    pred, ll, mm, _ = _scan_case('scan_runs_2')
    want = _strided_loss(thresholds)
    got = mine.voxel_loss_device(_dev(pred, misalign), _dev(ll, misalign), _dev(mm, misalign),
                                 LOSS_EDGE, *thresholds,
                                 out=_dev(np.full(shape, 7, np.float32), misalign))
    _assert_loss(got.cpu().numpy(), want,
                 'voxel loss, 3 passes, %r%s' % (thresholds, ', misaligned' if misalign else ''))
    flat, step = want.reshape(-1), mine_cases.PASS_VOXELS
    assert mine_cases.scan_layout(shape)['passes'] == 3 and 2 * step < flat.size < 3 * step
    for p in range(3):
        part = flat[p * step:(p + 1) * step]
        assert (part != 0).sum() > 0.2 * part.size and not (part == 7).any(), p


def test_fill_writes_no_row_beyond_the_capacity(ctx):
    """fplm_candidates_fill told of fewer rows than fplm_candidates_count found: the first
    `capacity` rows as they are in the full table, every later element of every column as it
    was"""
    torch = _torch()
    _, ll, mm = _mining_case(11, SHAPE)
    ww = np.random.RandomState(3).uniform(-1, 1, SHAPE).astype(np.float32)
    ww[::3] = 0
    ww[5, 40, 50] = np.nan
    half, cc = (12, 12, 12), 0
    want = mine.candidates_numpy(ll, mm, half, cc, ww)
    dev = torch.device('cuda', 0)
    dl, dm, dw = _dev(ll), _dev(mm), _dev(ww)
    nscr = _minecapi.scratch_bytes(ll.size)
    scratch = torch.empty(nscr // 4, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev)
    args = (dl.data_ptr(), dm.data_ptr(), dw.data_ptr(), SHAPE, half, cc, scratch.data_ptr(), nscr)
    total = _minecapi.candidates_count(*args, stream.cuda_stream)
    assert total == len(want[0]) > 2000

    for capacity in (total - 1000, 1, total):
        cols = torch.full((3, total), -7, dtype=torch.int32, device=dev)
        w = torch.full((total,), -7.0, dtype=torch.float32, device=dev)
        _minecapi.candidates_fill(*args, capacity, cols[0].data_ptr(), cols[1].data_ptr(),
                                  cols[2].data_ptr(), w.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        got = tuple(cols.cpu().numpy()) + (w.cpu().numpy(),)
        _assert_rows([g[:capacity] for g in got], [c[:capacity] for c in want], ('capacity', capacity))
        for g, col in zip(got, 'zyxw'):
            assert (g[capacity:] == -7).all(), (capacity, col)


def _short_row_inputs(i):
    shape, border = mine_cases.SHORT_ROW_CASES[i]
    pred, ll, mm = _mining_case(40 + i, shape)
    ww = np.random.RandomState(50 + i).uniform(-0.3, 1, shape).astype(np.float32)
    if mine_cases.SHORT_ROW_INSIDE[i] == 1:          # the centre voxel counts, for class 1
        c = tuple(d // 2 for d in shape)
        ll[c], mm[c], ww[c] = 1, 1, 0.5
    return shape, border, pred, ll, mm, ww


@pytest.mark.parametrize('misalign', [False, True])
@pytest.mark.parametrize('i', range(len(mine_cases.SHORT_ROW_CASES)))
def test_rows_shorter_than_a_group_and_borders_at_and_beyond_the_extent(ctx, i, misalign):
    """X < 4: the four voxels of a lane lie in several rows and planes, and whether each is
    inside the border is decided per voxel.  A border beyond the extent is clamped."""
    shape, border, pred, ll, mm, ww = _short_row_inputs(i)
    inside = mine_cases.SHORT_ROW_INSIDE[i]
    for thresholds in ((None, None), ((0.05, 2.0), (0.1, 0.5))):
        want = mine.voxel_loss_numpy(pred, ll, mm, border, *thresholds)
        got = mine.voxel_loss_device(_dev(pred, misalign), _dev(ll, misalign), _dev(mm, misalign),
                                     border, *thresholds,
                                     out=_dev(np.full(shape, 7, np.float32), misalign))
        _assert_loss(got.cpu().numpy(), want, 'voxel loss %r border %r' % (shape, border))
        assert (want != 0).sum() <= inside
    if inside > 1:
        assert 0 < (want != 0).sum()
    totals = [_candidates(ll, mm, border, cc, weights, misalign)
              for cc in (0, 1) for weights in (None, ww)]
    assert totals[0] + totals[2] <= inside and totals[1] <= totals[0] and totals[3] <= totals[2]
    if inside > 1:
        assert totals[0] > 0 and totals[1] > 0
    if inside == 1:
        assert totals == [0, 0, 1, 1] and (want != 0).sum() == 1
    # every voxel inside the border, dense: the rows are the border's box
    ones = np.ones(shape, np.uint8)
    assert _candidates(ones, ones, border, 1, None, misalign) == inside


@pytest.mark.parametrize('misalign', [False, True])
@pytest.mark.parametrize('thresholds', [(None, None), ((0.05, 2.0), (0.1, 0.5))])
def test_voxel_loss_of_predictions_off_the_unit_interval(ctx, thresholds, misalign):
    """NaN, +-inf, -0.25, 1.5 and the exact 1 under both labels: voxel_loss_numpy is the
    specification.  A NaN prediction is a NaN loss on both sides (np.maximum keeps it, and so
    does the kernel's floor); everything else compares as usual."""
    pred, ll, mm = mine_cases.off_unit_case()
    with np.errstate(all='ignore'):
        want = mine.voxel_loss_numpy(pred, ll, mm, (0, 0, 0), *thresholds)
    got = mine.voxel_loss_device(_dev(pred, misalign), _dev(ll, misalign), _dev(mm, misalign),
                                 (0, 0, 0), *thresholds,
                                 out=_dev(np.full(pred.shape, 7, np.float32), misalign))
    got = got.cpu().numpy()
    nan = np.isnan(want)
    assert nan.sum() == 4 and np.array_equal(np.isnan(pred), nan)
    assert np.array_equal(np.isnan(got), nan)
    got[nan], want[nan] = 0, 0
    _assert_loss(got, want, 'voxel loss off the unit interval %r' % (thresholds,))
    assert np.isinf(want).sum() == (2 if thresholds == (None, None) else 0)
    assert np.array_equal(np.isinf(got), np.isinf(want)) and (want < 0).sum() == np.isinf(want).sum() * 2


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
