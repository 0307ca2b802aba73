"""The device planner of write_labels_mask (libfplplan.so through ctypes) against
labels.plan_bricks, its specification: the tables are int32 decided by integer arithmetic,
so every comparison here is array_equal.  The shapes are the smallest at which each mechanism
of the planner can go wrong; a scan block covers 1 024 bricks per step, so the 8 192 bricks of
(64, 512, 1024) take eight blocks, and the 1 048 578 bricks of the thin volume take 1 025 tiles:
more than the 1 024 threads of the block that scans the tile sums, which then scans runs."""
import functools
import os

import numpy as np
import pytest

from flypylib_amd import _plancapi, fplobjdetect, fplsynapses, labels
from tests import labels_cases as cases

pytestmark = pytest.mark.gpu

PARTIAL = (9, 19, 261)                    # partial bricks on all three axes, three along x
SCAN = (64, 512, 1024)                    # 16 x 64 x 8 = 8 192 bricks
THIN = (4 * 1024 * 1024 + 5, 1, 1)        # 1 048 578 bricks of one voxel column each
BIG = (70, 45, 131)


def _torch():
    import torch
    return torch


def _rule(i):
    tbars, roi, ru, ri, _ = cases.rule_case(i)
    return roi.shape, labels.plan_tbars(tbars, roi.shape, ru, ri), cases.half_width(ru, ri)


def _random(seed, shape, half, n):
    return shape, labels.plan_tbars(cases.random_tbars(seed, shape, half, n), shape, half, None), half


def _partial():
    shape, locs, half = _random(32, PARTIAL, 2, 50)
    locs[:2] = [PARTIAL[2] - 3, PARTIAL[1] - 3, PARTIAL[0] - 3]     # in the last, partial brick
    return shape, locs, half


def _faces(outside):
    """two T-bars per face of a (23, 17, 29) volume, half-width 3: the cube ends on the face
    (`outside` 0), or is cut by it, or lies beyond it altogether (negative coordinates among
    them) - plan_bricks clamps those ranges and so must the device"""
    shape, half = (23, 17, 29), 3
    ext = shape[::-1]
    locs = []
    for axis in range(3):
        for step in ([0] if not outside else [2, half + 1, 40]):
            for pos in (half - step, ext[axis] - 1 - half + step):
                p = [14, 8, 11]
                p[axis] = pos
                locs.append(p)
    return shape, np.array(locs, np.int32), half


def _long():
    """1 500 T-bars on one voxel and 1 500 on its neighbour, interleaved: one brick list longer
    than a 1 024-thread block and than the 256 candidates the labels kernel stages"""
    locs = np.empty((3000, 3), np.int32)
    locs[0::2] = [20, 9, 8]
    locs[1::2] = [21, 9, 8]
    return (16, 20, 40), locs, 2


def _scan():
    rs = np.random.RandomState(41)
    g = [np.arange(8, n, 16) for n in SCAN[::-1]]               # 64, 32 and 4 grid points
    locs = np.array([(x, y, z) for z in g[2][[0, 3]] for y in g[1] for x in g[0]], np.int32)
    assert len(locs) == 4096
    locs += rs.randint(-1, 2, locs.shape).astype(np.int32)      # the cubes stay inside
    rs.shuffle(locs)
    return SCAN, locs, 6


def _thin():
    rs = np.random.RandomState(42)
    z = rs.randint(0, THIN[0], 300)
    z[:3] = [0, THIN[0] - 1, THIN[0] - 1]
    locs = np.zeros((300, 3), np.int32)
    locs[:, 2] = z
    return THIN, locs, 0


PLANS = {'rule%02d' % i: functools.partial(_rule, i) for i in range(len(cases.RULE_CASES))}
PLANS.update({
    'half_zero': lambda: _random(31, (36, 38, 40), 0, 40),
    'no_tbars': lambda: (BIG, np.zeros((0, 3), np.int32), 6),
    'one_tbar': lambda: ((36, 38, 40), np.array([[20, 19, 18]], np.int32), 6),
    'partial': _partial,
    'faces': lambda: _faces(False),
    'cut_by_faces': lambda: _faces(True),
    'long_list': _long,
    'scan_blocks': _scan,
    'scan_runs': _thin,
})


@functools.lru_cache(maxsize=None)
def _plan(name):
    """(shape, locs, half, (offsets, index) of labels.plan_bricks)"""
    shape, locs, half = PLANS[name]()
    want = labels.plan_bricks(locs, shape, half)
    for a in (locs,) + want:
        a.setflags(write=False)
    return shape, locs, half, want


def _unclamped(locs, half):
    """the pairs of T-bars whose ranges no face clamps"""
    zyx, b = locs[:, ::-1].astype(np.int64), np.asarray(labels.BRICK)
    return int(np.prod((zyx + half) // b - (zyx - half) // b + 1, axis=1).sum())


def _same_tables(got, want, what):
    torch = _torch()
    for g, w, n in zip(got, want, ('offsets', 'index')):
        assert g.is_cuda and g.dtype == torch.int32 and tuple(g.shape) == w.shape, (what, n)
        g = g.cpu().numpy()
        print('%s %s: %d of %d entries differ' % (what, n, int((g != w).sum()), w.size))
        assert np.array_equal(g, w), (what, n)


@pytest.mark.parametrize('name', sorted(PLANS))
def test_device_tables_are_plan_bricks_byte_for_byte(name):
    shape, locs, half, want = _plan(name)
    got = labels.plan_bricks_device(locs, shape, half, 0)
    _same_tables(got, want, name)
    assert labels.plan_pairs(locs, shape, half) == len(want[1])
    lists = np.diff(want[0])
    if name == 'no_tbars':
        assert not want[0].any() and len(want[1]) == 0 and got[1].numel() == 0
    if name == 'one_tbar':
        assert len(want[1]) == 12 and not want[1].any()
    if name == 'partial':
        assert labels.brick_counts(shape) == (3, 3, 3) and lists[-1] >= 2
    if name == 'faces':
        assert len(want[1]) == _unclamped(locs, half) and len(locs) == 6     # nothing is cut
    if name == 'cut_by_faces':
        assert 0 < len(want[1]) < _unclamped(locs, half) and len(locs) == 18
    if name == 'long_list':
        assert lists.max() == 3000 > 1024
    if name == 'scan_blocks':
        assert len(lists) == 8192 and (lists[-1024:] > 0).any() and (lists[:1024] > 0).any()
    if name == 'scan_runs':
        assert len(lists) > 1024 * 1024 and lists[0] == 1 and lists[-1] == 2


@pytest.mark.parametrize('name', ['long_list', 'scan_blocks', 'rule00'])
def test_two_runs_give_identical_tensors(name):
    torch = _torch()
    shape, locs, half, want = _plan(name)
    a = labels.plan_bricks_device(locs, shape, half, 0)
    b = labels.plan_bricks_device(locs, shape, half, torch.device('cuda', 0))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[1].data_ptr() != b[1].data_ptr()
    _same_tables(b, want, name)


def test_a_wrong_pair_total_sets_the_status_word_and_writes_no_row():
    """fplp_plan_bricks told one pair less than there are: rc 0, a non-zero status word after
    the synchronise, the counted total behind the offsets, and the index - the guard element
    behind its n_index rows included - as it was"""
    torch = _torch()
    shape, locs, half, want = _plan('rule00')
    total = len(want[1])
    dev = torch.device('cuda', 0)
    nb = labels.brick_counts(shape)
    n_bricks = nb[0] * nb[1] * nb[2]

    def run(n_index):
        tb = torch.from_numpy(locs.copy()).to(dev)
        offsets = torch.full((n_bricks + 1,), -7, dtype=torch.int32, device=dev)
        index = torch.full((total,), -7, dtype=torch.int32, device=dev)
        nbytes = _plancapi.scratch_bytes(len(locs), n_bricks, n_index)
        scratch = torch.full(((nbytes + 3) // 4,), 5, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev)
        _plancapi.plan_bricks(tb.data_ptr(), len(locs), shape, half, offsets.data_ptr(),
                              index.data_ptr(), n_index, scratch.data_ptr(), scratch.numel() * 4,
                              stream.cuda_stream)
        stream.synchronize()
        return int(scratch[0].item()), offsets.cpu().numpy(), index.cpu().numpy()

    status, offsets, index = run(total - 1)
    assert status != 0
    assert np.array_equal(offsets, want[0]) and offsets[-1] == total
    assert index[-1] == -7 and (index == -7).all()
    status, offsets, index = run(total)                 # the same buffers' sizes, the true total
    assert status == 0 and np.array_equal(offsets, want[0]) and np.array_equal(index, want[1])


@functools.lru_cache(maxsize=None)
def _case(i):
    """(tbars, roi, radius_use, radius_ign, buffer_size, (labels, mask) of the rule); i = -1:
    the case of tests/golden/synapses.npz"""
    if i < 0:
        tbars, roi, (ru, ri, buf) = cases.GOLDEN_TBARS, np.ones((36, 38, 40), np.uint8), (3, 6, 4)
    else:
        tbars, roi, ru, ri, buf = cases.rule_case(i)
    want = labels.labels_mask_numpy(labels.plan_tbars(tbars, roi.shape, ru, ri), roi, ru, ri, buf)
    for a in (roi,) + want:
        a.setflags(write=False)
    return tbars, roi, ru, ri, buf, want


def _equal(got, want, what):
    torch = _torch()
    for g, w, n in zip(got, want, ('labels', 'mask')):
        assert g.is_cuda and g.dtype == torch.uint8 and tuple(g.shape) == w.shape, (what, n)
        g = g.cpu().numpy()
        print('%s %s: %d of %d voxels differ' % (what, n, int((g != w).sum()), w.size))
        assert np.array_equal(g, w), (what, n)


def _offset_by_one(t):
    """a contiguous view of `t`'s values that starts one byte past an aligned base"""
    torch = _torch()
    flat = torch.empty(t.numel() + 4, dtype=torch.uint8, device=t.device)
    flat[1:1 + t.numel()] = t.reshape(-1)
    v = flat[1:1 + t.numel()].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 4 == 1
    return v


@pytest.mark.parametrize('i', range(-1, len(cases.RULE_CASES)))
def test_write_labels_mask_with_the_device_planner_equals_the_rule(i):
    """... and the host planner's device result, from a host roi_mask, from a resident one and
    from one at a byte offset of 1"""
    torch = _torch()
    tbars, roi, ru, ri, buf, want = _case(i)
    if i < 0:
        gold = np.load(os.path.join(os.path.dirname(cases.__file__), 'golden', 'synapses.npz'))
        assert np.array_equal(want[0], gold['lm_labels']) and np.array_equal(want[1], gold['lm_mask'])
    got = fplsynapses.write_labels_mask(tbars, roi, ru, ri, buf, None, device=0, planner='device')
    _equal(got, want, 'host roi')
    host_planned = fplsynapses.write_labels_mask(tbars, roi, ru, ri, buf, None, device=0,
                                                 planner='host')
    assert torch.equal(got[0], host_planned[0]) and torch.equal(got[1], host_planned[1])
    res = torch.from_numpy(roi.copy()).to('cuda:0')
    _equal(fplsynapses.write_labels_mask(tbars, res, ru, ri, buf, None, device=0,
                                         planner='device'), want, 'resident roi')
    assert np.array_equal(res.cpu().numpy(), roi)                   # the input is left alone
    _equal(fplsynapses.write_labels_mask(tbars, _offset_by_one(res), ru, ri, buf, None, device=True,
                                         planner='device'), want, 'roi off by one byte')


def test_stats_count_the_tbar_table_alone():
    torch = _torch()
    tbars, roi, ru, ri, buf, want = _case(0)
    res = torch.from_numpy(roi.copy()).to('cuda:0')
    locs = labels.plan_tbars(tbars, roi.shape, ru, ri)
    on_device, on_host = {}, {}
    _equal(labels.labels_mask_device(locs, res, ru, ri, buf, stats=on_device, planner='device'),
           want, 'stats')
    labels.labels_mask_device(locs, res, ru, ri, buf, stats=on_host)
    offsets, index = labels.plan_bricks(locs, roi.shape, max(ru, ri))
    assert on_device == {'table_bytes': locs.nbytes, 'pairs': len(index)}
    assert on_host == {'table_bytes': locs.nbytes + offsets.nbytes + index.nbytes,
                       'pairs': len(index)}
    with pytest.raises(ValueError, match="planner 'gpu'"):
        labels.labels_mask_device(locs, res, ru, ri, buf, planner='gpu')
    empty = fplsynapses.write_labels_mask({'locs': np.zeros((0, 3)), 'conf': np.zeros(0)}, res,
                                          ru, ri, buf, None, device=0, planner='device')
    _equal(empty, labels.labels_mask_numpy(np.zeros((0, 3), np.int32), roi, ru, ri, buf), 'empty')


def test_gen_volume2_takes_the_device_planned_pair(ctx):
    """gen_volume2(device=0) on the resident (labels, mask) of planner='device' and on the host
    arrays of the host path, same seed: the same first three batches, byte for byte"""
    tbars = cases.random_tbars(12, BIG, 6, 300)
    roi = (cases.random_roi(3, BIG) != 0).astype(np.uint8)
    im = np.random.RandomState(5).randn(*BIG).astype(np.float32)
    host = fplsynapses.write_labels_mask(tbars, roi, 3, 6, 4, None)
    res = fplsynapses.write_labels_mask(tbars, roi, 3, 6, 4, None, device=0, planner='device')
    args = ((24, 24, 24), 8, 0.5)
    a = fplobjdetect.gen_volume2([(im, res[0], res[1])], *args, noise_aug=[0.05, 0.1],
                                 rng=np.random.RandomState(4), device=0)
    b = fplobjdetect.gen_volume2([(im,) + host], *args, noise_aug=[0.05, 0.1],
                                 rng=np.random.RandomState(4), device=0)
    for i in range(3):
        for x, y in zip(next(a), next(b)):
            x, y = x.cpu().numpy(), y.cpu().numpy()
            assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), i
