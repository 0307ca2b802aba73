"""libfplnear.so on the GPU: the device neighbour table against near.pairs_numpy, byte for
byte, on the point sets where the kernels can go wrong (tests/near_cases.py names each with
its reason); the capacity bound of the fill; rm_tbar_multi_pred(device=) and the pipeline's
merge_device= against their host calls."""
import os
import pickle

import numpy as np
import pytest

from flypylib_amd import _nearcapi, fplpipeline, fplsynapses, near
from tests import near_cases as cases

pytestmark = pytest.mark.gpu

T = cases.T


def _check_table(pts, t=T):
    """the device table equals pairs_numpy's - row pointers, columns, dtypes"""
    want = near.pairs_numpy(pts, t)
    info = {}
    got = near.pairs_device(pts, t, 0, info=info)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32
    assert info['entries'] == len(want[1]) and info['dims'] == near.grid_of(pts, t)[2]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    return want


@pytest.mark.parametrize('name', [n for n in cases.SETS if n != 'no pair'])
def test_device_table_on_the_point_sets(ctx, name):
    cases.check_sets()
    pts = cases.SETS[name]()
    indptr, indices = _check_table(pts)
    rows = np.diff(indptr)
    if name.startswith(('block tail', 'scan runs')):
        assert 5 < rows.mean() < 12                       # about 8 partners each
    if name in ('one point', 'two coincident points'):
        assert len(indices) == 0
    if name == 'two points at exactly T':
        assert indices.tolist() == [1, 0]
    if name == 'boundary':
        assert rows.tolist() == [1, 1, 1, 0, 1, 1, 1, 0]
    if name == 'lattice on the cell faces':
        half = len(pts) // 2
        assert len(indices) >= 2 * half and min(near.grid_of(pts, T)[2]) >= 5
    if name == 'one cell':
        assert np.all(rows == len(pts) - 1)
    if name == 'cluster':
        assert rows.max() == cases.B + 43 and (rows == 0).sum() == 60
    if name == 'thin':
        lo, hi = near.CellGrid(pts, T).runs(near.CellGrid(pts, T).cells)
        assert np.mean(hi - lo == 0) > 0.5 and len(indices) >= 20


def test_other_thresholds(ctx):
    pts = cases.negative_fractional()
    for t in (26.3, 5, 200.0):
        _check_table(pts, t)


def test_no_pair_at_all_is_no_fill_call(ctx, monkeypatch):
    pts = cases.no_pair()
    monkeypatch.setattr(_nearcapi, 'pairs_fill', None)            # calling it would raise
    indptr, indices = _check_table(pts)
    assert len(indices) == 0 and not indptr.any()
    monkeypatch.setattr(_nearcapi, 'pairs_count', None)           # empty input: no call at all
    indptr, indices = near.pairs_device(np.zeros((0, 3)), T, 0)
    assert indptr.tolist() == [0] and len(indices) == 0 and indices.dtype == np.int32


def _counted(pts, t=T):
    """the device state behind pairs_device, up to the count: (args, total, stream, keep-alive)"""
    import torch
    dev = near.torch_device(0)
    pts = np.ascontiguousarray(pts, np.float64)
    n, t2 = len(pts), near.threshold2(t)
    origin, cell, dims = near.grid_of(pts, t)
    nscr = _nearcapi.scratch_bytes(n)
    stream = torch.cuda.current_stream(dev)
    p_dev = torch.from_numpy(pts).to(dev)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    _nearcapi.cell_keys(p_dev.data_ptr(), n, origin, cell, dims, keys.data_ptr(), stream.cuda_stream)
    keys, order = torch.sort(keys)
    scratch = torch.empty((nscr + 7) // 8, dtype=torch.int64, device=dev)
    args = (p_dev.data_ptr(), n, t2, origin, cell, dims, keys.data_ptr(), order.data_ptr(),
            scratch.data_ptr(), nscr)
    total = _nearcapi.pairs_count(*args, stream.cuda_stream)
    return args, total, stream, (p_dev, keys, order, scratch)


def test_fill_honours_capacity_and_a_column_array_off_by_4_bytes(ctx):
    import torch
    pts = cases.random_integer(cases.B + 1)
    want = near.pairs_numpy(pts, T)[1]
    args, total, stream, keep = _counted(pts)
    assert total == len(want) > 1000
    for capacity in (total, total - 1, 1):
        for shift in (0, 1):                     # the header asks for 4-byte alignment only
            buf = torch.full((total + 64 + 1,), -5, dtype=torch.int32, device=keep[0].device)
            _nearcapi.pairs_fill(*args, capacity, buf.data_ptr() + 4 * shift, stream.cuda_stream)
            stream.synchronize()
            host = buf.cpu().numpy()
            assert np.all(host[:shift] == -5)
            assert np.array_equal(host[shift:shift + capacity], want[:capacity])
            assert np.all(host[shift + capacity:] == -5)


def test_the_same_call_twice_gives_the_same_bytes(ctx):
    pts = cases.cluster()
    a, b = near.pairs_device(pts, T, 0), near.pairs_device(pts, T, 0)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_refusals_come_before_any_launch(ctx):
    pts = cases.one_cell()
    args, total, stream, keep = _counted(pts)
    with pytest.raises(_nearcapi.FplNearError, match='the column array is not 4-byte aligned'):
        _nearcapi.pairs_fill(*args, total, keep[3].data_ptr() + 2, stream.cuda_stream)
    small = args[:4] + (args[4] / 2,) + args[5:]
    with pytest.raises(_nearcapi.FplNearError, match=r'cell side .* is below sqrt\(T2\)'):
        _nearcapi.pairs_count(*small, stream.cuda_stream)
    with pytest.raises(_nearcapi.FplNearError, match='scratch of 8 bytes'):
        _nearcapi.pairs_count(*(args[:9] + (8,)), stream.cuda_stream)
    wide = args[:5] + ((2 ** 28, 2 ** 28, 2 ** 7),) + args[6:]
    with pytest.raises(_nearcapi.FplNearError, match=r'exceeds the 2\^62'):
        _nearcapi.pairs_count(*wide, stream.cuda_stream)
    with pytest.raises(ValueError, match='spread too far'):
        near.pairs_device(np.array([[0.0, 0, 0], [1e12, 0, 0]]), T, 0)


def test_device_mode_without_the_library_raises(ctx, monkeypatch):
    """with a GPU at hand as well: the binding's error, no fallback to the numpy table"""
    monkeypatch.setattr(_nearcapi._side, '_lib', None)
    monkeypatch.setattr(_nearcapi._side, 'path', '/nonexistent/libfplnear.so')
    tb = cases.planted(600)
    with pytest.raises(_nearcapi.FplNearError, match='libfplnear.so not found at /nonexistent'):
        fplsynapses.rm_tbar_multi_pred(tb, method='sparse', device=0)


def _same(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)


def test_rm_tbar_multi_pred_on_the_device(ctx):
    tb = cases.planted(600)
    labels = cases.planted_labels(tb)
    for kw in ({}, {'labels': labels}):
        dense = fplsynapses.rm_tbar_multi_pred(tb, method='dense', **kw)
        sparse = fplsynapses.rm_tbar_multi_pred(tb, method='sparse', **kw)
        got = fplsynapses.rm_tbar_multi_pred(tb, method='sparse', device=0, **kw)
        _same(got, sparse)
        _same(got, dense)
        assert got[1].sum() > 20 and got[0].sum() > 20


def test_the_pipeline_keyword(ctx, tmp_path):
    """all.p is the same bytes with and without the keyword; all_merged.p is a direct call's
    result, from the host table and from the device table alike"""
    from flypylib_amd import fplobjdetect
    from tests.test_pipeline import _small_setup
    net, vol, roi = _small_setup()
    kw = dict(obj_min_dist=5, smoothing_sigma=1.5, buffer_sz=10, precision='f32')
    norm = [128., 33., 0.7]
    plain_dir, wd = str(tmp_path / 'plain'), str(tmp_path / 'merged')
    plain = fplobjdetect.full_roi_inference(vol, None, roi, net, 0.2, plain_dir, norm, **kw)
    assert not os.path.exists(plain_dir + '/all_merged.p') and len(plain['conf']) > 20
    host = fplobjdetect.full_roi_inference(vol, None, roi, net, 0.2, wd, norm, neighbor_thresh=12, **kw)
    assert open(wd + '/all.p', 'rb').read() == open(plain_dir + '/all.p', 'rb').read()
    merged_bytes = open(wd + '/all_merged.p', 'rb').read()
    want = fplsynapses.merge_multi_pred(plain, *fplsynapses.rm_tbar_multi_pred(
        plain, neighbor_thresh=12, method='dense'))
    assert 0 < len(want['conf']) < len(plain['conf'])
    for got in (host, pickle.loads(merged_bytes)):
        assert np.array_equal(got['locs'], want['locs']) and np.array_equal(got['conf'], want['conf'])
        assert got['locs'].dtype == plain['locs'].dtype and got['conf'].dtype == plain['conf'].dtype
    # the finished substacks are reused; the merge runs again, on the device table
    dev = fplobjdetect.full_roi_inference(vol, None, roi, net, 0.2, wd, norm, neighbor_thresh=12,
                                          merge_device=0, **kw)
    assert open(wd + '/all_merged.p', 'rb').read() == merged_bytes
    assert np.array_equal(dev['locs'], want['locs'])
    # with a segmentation the labels come from it
    seg = np.zeros(vol.shape, np.int64)
    seg[:, :, vol.shape[2] // 2:] = 1
    labelled = fplpipeline.merge_border_duplicates(plain, 12, fplpipeline._ArraySource(seg), 'sparse', 0)
    at = np.clip(np.round(plain['locs']).astype(int), 0, np.array(vol.shape)[::-1] - 1)   # x, y, z
    want = fplsynapses.merge_multi_pred(plain, *fplsynapses.rm_tbar_multi_pred(
        plain, neighbor_thresh=12, labels=seg[at[:, 2], at[:, 1], at[:, 0]]))
    assert np.array_equal(labelled['locs'], want['locs'])
