"""libfplroi.so on the GPU, through the C ABI and the public API: byte-equal to the numpy
specification of roi.py, with guard bytes on both sides of every output buffer."""
import os

import numpy as np
import pytest

from flypylib_amd import _roicapi, fplsynapses
from flypylib_amd.roi import BlockRoi, cut_normalize_device
from tests.test_roi_host import check_against_golden, export, golden, irregular_roi  # noqa: F401

pytestmark = pytest.mark.gpu
GUARD, FILL = 64, 0xAB


@pytest.fixture(scope='module')
def dev():
    import torch
    return torch.device('cuda', 0)


def guarded(dev, nbytes, shift=0):
    """(buffer, address of the `nbytes` payload): 0xAB everywhere, the payload `shift` bytes past
    a 16-byte aligned address"""
    import torch
    buf = torch.full((nbytes + 2 * GUARD + 16,), FILL, dtype=torch.uint8, device=dev)
    start = GUARD + (-(buf.data_ptr() + GUARD)) % 16 + shift
    return buf, buf.data_ptr() + start, start


def payload(buf, start, nbytes):
    import torch
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:start] == FILL).all() and (host[start + nbytes:] == FILL).all(), 'a guard byte was written'
    return host[start:start + nbytes]


def mask_box(roi, dev, dims, offset, shift=0):
    n = int(np.prod(dims))
    buf, addr, start = guarded(dev, n, shift)
    _roicapi.mask_box(roi.device_tables(dev), len(roi.row_keys), len(roi.runs), roi.block_size, offset,
                      dims, addr)
    return payload(buf, start, n).reshape(dims)


# ---- fplr_mask_box ----------------------------------------------------------------------------------

@pytest.mark.parametrize('width', [1, 15, 16, 17, 33])
def test_mask_box_widths_offsets_and_alignments(dev, width):
    roi, mask, origin = irregular_roi(4)
    for ox in (-11, -16, 3, 0):                     # odd and 16-aligned x offsets
        for shift in (0, 5):                        # the buffer on and off a 16-byte address
            dims, offset = (7, 9, width), (-9, 2, ox)
            got = mask_box(roi, dev, dims, offset, shift)
            assert np.array_equal(got, roi.roi3D(dims, offset)), (ox, shift)


def test_mask_box_run_edges_missing_rows_and_negative_origins(dev):
    b = 4
    roi, mask, origin = irregular_roi(b)
    oz, oy, ox = (o * b for o in origin)
    z, y, x0, x1 = roi.runs[len(roi.runs) // 2].tolist()
    cases = [((3, 5, (x1 + 1) * b - ox), (z * b, y * b - 2, ox)),         # a run ends on the box's face
             ((2, 3, 7 * b + 9), (oz + b, oy + b - 1, ox - 4)),             # two runs one block apart
             ((4, 3 * b, 41), (oz + 2 * b, oy + 2 * b, ox - 7)),            # a missing block row between two
             ((9, 11, 50), (oz - 5, oy - 3, ox - 13)),                      # negative origin
             ((5, 4, 37), (oz + 40 * b, oy, ox)), ((3, 3, 19), (10 ** 9, -10 ** 9, 10 ** 9))]   # outside everything
    for dims, offset in cases:
        want = roi.roi3D(dims, offset)
        assert np.array_equal(mask_box(roi, dev, dims, offset, 1), want), (dims, offset)
    assert not want.any() and cases[0][0][2] > 0
    empty = BlockRoi([], 32)
    assert not mask_box(empty, dev, (3, 4, 35), (-1, 0, 7), 3).any()
    got = roi.roi3D((6, 5, 33), (oz, oy, ox + 1), device=0)                # the public API
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), roi.roi3D((6, 5, 33), (oz, oy, ox + 1)))


def test_mask_box_deep_row_search_and_grid_stride(dev):
    rs = np.random.RandomState(5)
    blocks = rs.rand(20, 20, 9) < 0.5                                      # about 300 block rows
    roi = BlockRoi.from_block_mask(blocks, (-3, 4, -2), block_size=2)
    assert 280 <= len(roi.row_keys) <= 400
    dims, offset = (45, 47, 23), (-8, 5, -5)
    assert np.array_equal(mask_box(roi, dev, dims, offset, 7), roi.roi3D(dims, offset))
    # more voxel rows than one pass of the grid covers
    dims = (131, 130, 17)
    assert dims[0] * dims[1] > _roicapi.MAX_GRID * (_roicapi.BLOCK // 64)
    assert np.array_equal(mask_box(roi, dev, dims, offset, 2), roi.roi3D(dims, offset))


# ---- fplr_ptquery -----------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [0, 1, 63, 64, 65, 257])
def test_ptquery_sizes_run_edges_and_negatives(dev, n):
    import torch
    b = 4
    roi, mask, origin = irregular_roi(b)
    edge = [(z * b, y * b, x) for z, y, x0, x1 in roi.runs.tolist()
            for x in (x0 * b - 1, x0 * b, x1 * b + b - 1, x1 * b + b)]
    rs = np.random.RandomState(n)
    pts = np.concatenate([np.asarray(edge), rs.randint(-20, 30, (300, 3)),
                          [[-2 ** 45, 0, 0], [2 ** 45, 3, 3]]]).astype(np.int64)
    pts = pts[rs.permutation(len(pts))[:n]] if n < 257 else pts[:257]
    buf, addr, start = guarded(dev, n)
    res = torch.from_numpy(pts.copy()).to(dev) if n else None
    _roicapi.ptquery(roi.device_tables(dev), len(roi.row_keys), len(roi.runs), b,
                     res.data_ptr() if n else 0, n, addr if n else 0)
    got = payload(buf, start, n)
    want = roi.ptquery(pts) if n else np.zeros(0, bool)
    assert np.array_equal(got, want.astype(np.uint8))
    if n == 257:
        assert 0 < want.sum() < n
        assert np.array_equal(roi.ptquery(pts, device=0), want)
        assert np.array_equal(roi.ptquery(res, device=0).cpu().numpy(), want)
        assert not BlockRoi([], b).ptquery(pts, device=0).any()


# ---- fplr_box_counts --------------------------------------------------------------------------------

def test_box_counts(dev):
    import torch
    b = 4
    roi, mask, origin = irregular_roi(b)
    oz, oy, ox = (o * b for o in origin)
    whole = (oz - 3, oy - 3, ox - 3) + tuple(n * b + 6 for n in mask.shape)
    boxes = np.asarray([(oz + 1, oy + 2, ox + 3, 9, 10, 11), (10 ** 6, 0, 0, 5, 5, 5), whole], np.int64)
    want = roi.voxel_counts(boxes)
    assert want[1] == 0 and want[2] == roi.n_blocks * b ** 3
    for s in (0, 1, 3):
        buf, addr, start = guarded(dev, 8 * s)
        res = torch.from_numpy(boxes[:s].copy()).to(dev) if s else None
        _roicapi.box_counts(roi.device_tables(dev), len(roi.row_keys), len(roi.runs), b,
                            res.data_ptr() if s else 0, s, addr if s else 0)
        assert payload(buf, start, 8 * s).view(np.int64).tolist() == want[:s].tolist()
    assert roi.voxel_counts(boxes, device=0).tolist() == want.tolist()
    # 2^33 voxels: the count stays int64
    solid = BlockRoi([[z, y, 0, 63] for z in range(64) for y in range(64)], 32)
    got = solid.voxel_counts([[0, 0, 0, 2048, 2048, 2048], [-5, 7, 2000, 100, 100, 100]], device=0)
    assert got.dtype == np.int64 and got.tolist() == [2 ** 33, 95 * 100 * 48]


# ---- fplr_cut_normalize_u8 ----------------------------------------------------------------------------

@pytest.mark.parametrize('norm', [(135.0, 48.0), (128.0, 33.0), (127.3, 0.1)])
def test_cut_normalize_is_numpys_arithmetic(dev, norm):
    import torch
    from flypylib_amd import fplpipeline
    vol = np.random.RandomState(40).randint(0, 256, (40, 40, 40)).astype(np.uint8)
    res = torch.from_numpy(vol).to(dev)
    src = fplpipeline._ArraySource(vol)
    mean, std = np.float32(norm[0]), np.float32(norm[1])
    boxes = [((-3, -4, -5), (46, 47, 49)),          # leaves every face
             ((30, 31, 29), (13, 12, 15)), ((-6, 5, 2), (9, 7, 5)), ((3, 4, 5), (6, 7, 9)),
             ((50, 0, 0), (4, 4, 4)), ((0, 0, 39), (1, 1, 3))]
    for k, (origin, dims) in enumerate(boxes):
        cube = np.zeros(dims, np.uint8)
        lo, hi = np.maximum(origin, 0), np.minimum(np.add(origin, dims), 40)
        if np.all(hi > lo):
            cube[tuple(slice(a - o, c - o) for a, c, o in zip(lo, hi, origin))] = \
                vol[tuple(slice(a, c) for a, c in zip(lo, hi))]
        want = (cube.astype('float32') - mean) / std
        n = int(np.prod(dims))
        buf, addr, start = guarded(dev, 4 * n, shift=4 * (k % 4))          # every float misalignment
        _roicapi.cut_normalize_u8(res, vol.shape, origin, dims, mean, std, addr)
        got = payload(buf, start, 4 * n).view(np.float32).reshape(dims)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (origin, dims)
    got = cut_normalize_device(res, vol.shape, (-3, -4, -5), (46, 47, 49), norm[0], norm[1], dev)
    cube = src.cube_host([-3, -4, -5], 49)[:46, :47]
    assert np.array_equal(got.cpu().numpy().view(np.uint32),
                          ((cube.astype('float32') - mean) / std).view(np.uint32))


# ---- roi_to_substacks(device=0) -----------------------------------------------------------------------

def test_device_roi_to_substacks_on_the_golden_scene(golden, tmp_path, dev):  # noqa: F811
    import torch
    from flypylib_amd import fplobjdetect
    host_dir, dev_dir = str(tmp_path / 'host'), str(tmp_path / 'dev')
    os.makedirs(host_dir), os.makedirs(dev_dir)
    host = export(golden, host_dir)
    seg_res = torch.from_numpy(golden['seg'].view(np.int64)).to(dev)
    got = export(golden, dev_dir, device=0, seg_name=seg_res)
    for o in got:
        assert all(o[k].is_cuda for k in ('image', 'roi_mask', 'labels', 'mask', 'seg'))
    check_against_golden(golden, got, dev_dir, to_host=lambda t: t.cpu().numpy())
    names = sorted(os.listdir(host_dir))
    assert names == sorted(os.listdir(dev_dir))
    for name in names:                              # the written files, byte for byte
        assert open(os.path.join(host_dir, name), 'rb').read() == \
            open(os.path.join(dev_dir, name), 'rb').read(), name
    for h, d in zip(host, got):
        for k in ('image', 'roi_mask', 'labels', 'mask'):
            assert np.array_equal(h[k].view(np.uint8), d[k].cpu().numpy().view(np.uint8)), k
        assert np.array_equal(h['seg'], d['seg'].cpu().numpy().view(np.uint64))
    # a resident grayscale and a host segmentation: the same
    res = export(golden, None, device=0, dvid_server=torch.from_numpy(golden['volume']).to(dev))
    for h, d in zip(host, res):
        assert np.array_equal(h['image'], d['image'].cpu().numpy()) and np.array_equal(h['seg'], d['seg'])
    # labels and mask go straight into gen_volume2(device=0), as write_labels_mask(device=)'s do
    o, h = got[0], host[0]
    args = ((18, 18, 18), 4, 0.5)
    a = fplobjdetect.gen_volume2([(h['image'], o['labels'], o['mask'])], *args, noise_aug=[0.05, 0.1],
                                 rng=np.random.RandomState(4), device=0)
    b = fplobjdetect.gen_volume2([(h['image'], h['labels'], h['mask'])], *args, noise_aug=[0.05, 0.1],
                                 rng=np.random.RandomState(4), device=0)
    for x, y in zip(next(a), next(b)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    rows = fplsynapses.roi_to_substacks(golden['volume'], None, golden['roi'], golden['tbars'], 2,
                                        device=0)
    assert ['%03d\t%.03f\t%3d' % r for r in rows] == golden['stats'].tolist()
