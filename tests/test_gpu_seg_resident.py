"""The segmentation resident on the GPU: the box fill (csrc/seg_box.h, through libfplseg.so's
fpls_pad_box) against numpy's cut + pad element by element, the same kernel inside a context
(fpl_v2o_set_seg with a box descriptor) through voxel2obj(seg=<resident>, seg_origin=) against voxel2obj(seg=<host cut>),
fpls_gather_labels against numpy indexing, and full_roi_inference / evaluate_substacks with
resident labels against their host-label runs.  tests/seg_cases.py holds the shapes and says
why each is there."""
import os

import numpy as np
import pytest

from flypylib_amd import _capi, _segcapi, fplobjdetect, fplpipeline
from tests import seg_cases as sc

pytestmark = pytest.mark.gpu

_VOLUMES = {}


def _volume(dtype):
    dtype = np.dtype(dtype)
    if dtype not in _VOLUMES:
        _VOLUMES[dtype] = sc.label_volume(dtype)
    return _VOLUMES[dtype]


def _resident(ctx, vol, how):
    if how == 'torch':
        import torch
        return torch.from_numpy(vol).cuda()
    return ctx.malloc(vol.shape, vol.dtype).from_host(vol)


def _release(res):
    if isinstance(res, _capi.DeviceBuffer):
        res.free()


RESIDENT_FORMS = [('uint32', 'buffer'), ('uint64', 'buffer'), ('int64', 'torch'), ('int64', 'buffer'),
                  ('int32', 'torch')]


@pytest.mark.parametrize('dtype,how', RESIDENT_FORMS, ids=['%s-%s' % f for f in RESIDENT_FORMS])
def test_fill_equals_the_padded_host_cut(ctx, dtype, how):
    vol = _volume(dtype)
    res = _resident(ctx, vol, how)
    try:
        for name, origin, dims in sc.BOXES:
            pdims = tuple(d + 2 * sc.R for d in dims)
            want = sc.padded_u64(sc.host_cut(vol, origin, dims))
            n = int(np.prod(pdims))
            # guard voxels after the volume, and a destination 8 bytes off the 16-byte grid
            for shift in (0, 1):
                dst = ctx.malloc((n + 9,), np.uint64).from_host(np.full(n + 9, 0x5a5a5a5a5a5a5a5a, np.uint64))
                _segcapi.pad_box(res, origin, dims, sc.R, dst.ptr + 8 * shift)
                flat = dst.to_host()
                dst.free()
                got = flat[shift:shift + n].reshape(pdims)
                assert np.array_equal(got, want), (name, shift, np.argwhere(got != want)[:4])
                assert np.all(flat[:shift] == 0x5a5a5a5a5a5a5a5a) and np.all(flat[shift + n:] == 0x5a5a5a5a5a5a5a5a)
            if name.startswith(('disjoint', 'face')):
                assert not want.any()
    finally:
        _release(res)


def test_fill_rejects_what_it_cannot_read(ctx):
    vol = _volume(np.uint64)
    res = _resident(ctx, vol, 'buffer')
    dims = sc.BOX_A
    pdims = tuple(d + 2 * sc.R for d in dims)
    dst = ctx.malloc(pdims, np.uint64)
    ctx.v2o_smooth(np.zeros(dims, np.float32), dims, sc.R, fplobjdetect.gaussian_kernel1d(1.0), [])
    try:
        with pytest.raises(_capi.FplHipError, match="differ from the prediction's"):
            ctx.v2o_set_seg_box(res, (0, 0, 0), sc.BOX_B)
        with pytest.raises(_capi.FplHipError, match='coordinate range'):
            ctx.v2o_set_seg_box(res, (0, 1 << 21, 0), dims)
        with pytest.raises(ValueError, match='device resident'):
            ctx.v2o_set_seg_box(vol, (0, 0, 0), dims)
        with pytest.raises(ValueError, match='4- or 8-byte'):
            ctx.v2o_set_seg_box(res.view(vol.shape, np.uint16), (0, 0, 0), dims)
        # the C entry point itself: a NULL volume, the label width, a host pointer in the descriptor
        lib, C = ctx.lib, _capi.C
        dd = _capi._arr(dims, C.c_int64)
        for ptr, nbytes, text in ((None, 8, b'NULL'), (res.ptr, 2, b'4 or 8 bytes'),
                                  (vol.ctypes.data, 8, b'device memory')):
            box = _capi.fpl_seg_box(ptr, _capi._arr(vol.shape, C.c_int64), _capi._arr((0, 0, 0), C.c_int64))
            assert lib.fpl_v2o_set_seg(ctx.h, C.cast(C.byref(box), C.c_void_p), nbytes,
                                       _capi.MEM_DEVICE_BOX, dd, -1) != 0
            assert text in lib.fpl_last_error(ctx.h), lib.fpl_last_error(ctx.h)
        ctx.v2o_set_seg_box(res, (0, 0, 0), dims)                    # and the context still works
        # libfplseg.so's own checks
        with pytest.raises(_segcapi.FplSegError, match='coordinate range'):
            _segcapi.pad_box(res, (0, 1 << 21, 0), dims, sc.R, dst)
        with pytest.raises(ValueError, match='device'):
            _segcapi.pad_box(res, (0, 0, 0), dims, sc.R, np.zeros(pdims, np.uint64))
        slib = _segcapi.load_library()
        a3 = _segcapi._arr3
        assert slib.fpls_pad_box(C.c_void_p(vol.ctypes.data), 8, a3(vol.shape), a3((0, 0, 0)), a3(dims),
                                 sc.R, C.c_void_p(dst.ptr), None) != 0
        assert b'device memory' in slib.fpls_last_error()
        assert slib.fpls_pad_box(C.c_void_p(res.ptr), 8, a3(vol.shape), a3((0, 0, 0)), a3(dims),
                                 sc.R, C.c_void_p(np.zeros(pdims, np.uint64).ctypes.data), None) != 0
        assert b'device memory' in slib.fpls_last_error()
    finally:
        dst.free()
        _release(res)


@pytest.mark.parametrize('kind', ['float32', 'float64', 'int32'])
def test_voxel2obj_from_the_resident_volume_equals_the_host_cut(ctx, kind):
    thd = sc.prediction_thd(kind)
    for dtype, how in (('uint64', 'buffer'), ('int32', 'torch')):
        vol = _volume(dtype)
        res = _resident(ctx, vol, how)
        try:
            for name, origin, dims in sc.V2O_BOXES:
                pred = sc.prediction(dims, kind)
                args = (pred, sc.V2O_KW['obj_min_dist'], sc.V2O_KW['smoothing_sigma'], (3, 2, 1), 0, thd)
                want = fplobjdetect.voxel2obj(*args, seg=sc.host_cut(vol, origin, dims), **sc.SEG_KW)
                got = fplobjdetect.voxel2obj(*args, seg=res, seg_origin=origin, **sc.SEG_KW)
                plain = fplobjdetect.voxel2obj(*args)
                assert len(want['conf']) >= 8, (name, len(want['conf']))
                assert got['locs'].dtype == want['locs'].dtype and got['conf'].dtype == want['conf'].dtype
                assert np.array_equal(got['locs'], want['locs']), name
                assert np.array_equal(got['conf'], want['conf']), name
                assert not (plain['locs'].shape == want['locs'].shape
                            and np.array_equal(plain['locs'], want['locs'])), name
        finally:
            _release(res)


def _points(n, extent, seed=0):
    """n points of the volume: its eight corners first, then random ones, some repeated"""
    rs = np.random.RandomState(seed)
    corners = np.array([[z, y, x] for z in (0, extent[0] - 1) for y in (0, extent[1] - 1)
                        for x in (0, extent[2] - 1)], np.int64)
    rand = np.stack([rs.randint(0, e, max(n, 8)) for e in extent], axis=1).astype(np.int64)
    pts = np.concatenate([corners, rand, rand[::3]])[:n] if n >= 8 else rand[:n]
    return np.ascontiguousarray(pts)


@pytest.mark.parametrize('dtype,how', RESIDENT_FORMS[:3], ids=['%s-%s' % f for f in RESIDENT_FORMS[:3]])
def test_gather_labels(ctx, dtype, how):
    import torch
    vol = _volume(dtype)
    res = _resident(ctx, vol, how)
    as_u64 = sc.padded_u64(vol, 0)
    try:
        for n in (0, 1, 257, 5000):
            pts = _points(n, vol.shape, n)
            want = as_u64[pts[:, 0], pts[:, 1], pts[:, 2]]
            got = ctx.gather_labels(res, pts)
            assert got.dtype == np.uint64 and np.array_equal(got, want), n
            # device triples, device output
            out = torch.zeros(max(n, 1), dtype=torch.int64, device='cuda')
            ctx.gather_labels(res, torch.from_numpy(pts).cuda(), out=out)
            assert np.array_equal(out.cpu().numpy()[:n].view(np.uint64), want), n
            # the pipeline's form: labels in the volume's own type
            src = fplpipeline._DeviceLabelSource(res)
            assert src.extent == vol.shape and src.itemsize == vol.dtype.itemsize
            lab = src.labels_at(ctx, pts)
            assert lab.dtype == vol.dtype and np.array_equal(lab, vol[pts[:, 0], pts[:, 1], pts[:, 2]])
        assert len(np.unique(_points(5000, vol.shape, 5000), axis=0)) < 5000         # repeats
        # a point outside the volume: an error, and nothing written - neither inside `out` nor
        # in the guard rows around it
        for bad in ([0, 0, vol.shape[2]], [-1, 0, 0], [0, vol.shape[1], 0], [1 << 40, 0, 0]):
            pts = _points(257, vol.shape, 1)
            pts[130] = bad
            guard = np.full(257 + 64, 0xabababababababab, np.uint64)
            with pytest.raises(_segcapi.FplSegError, match='outside'):
                ctx.gather_labels(res, pts, out=guard[32:-32])
            assert np.all(guard == np.uint64(0xabababababababab))
            d_guard = torch.full((257 + 64,), 0x2b2b2b2b2b2b2b2b, dtype=torch.int64, device='cuda')
            with pytest.raises(_segcapi.FplSegError, match='outside'):
                ctx.gather_labels(res, torch.from_numpy(pts).cuda(), out=d_guard[32:-32])
            assert bool((d_guard == 0x2b2b2b2b2b2b2b2b).all())
    finally:
        _release(res)


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


def test_pipeline_with_resident_labels_writes_the_same_files(ctx, tmp_path, monkeypatch):
    """per-substack pickles, all.p and all_merged.p, byte for byte: host labels on the host path
    (FPL_PIPE_RESIDENT_GB=0), host labels uploaded (default cap), labels already resident"""
    import torch
    from tests.test_pipeline import _small_setup
    net, vol, roi = _small_setup()           # substacks poke out of the 70x90x80 volume; one misses it
    z, y, x = np.meshgrid(*(np.arange(s, dtype=np.uint64) for s in vol.shape), indexing='ij')
    seg = sc._mix((((z // np.uint64(32)) << np.uint64(40)) | ((y // np.uint64(32)) << np.uint64(20))
                   | (x // np.uint64(32))) + np.uint64(1))
    kw = dict(obj_min_dist=11, smoothing_sigma=2.0, buffer_sz=12, precision='f32', neighbor_thresh=12)
    norm = [128., 33.]
    roi = [roi[0], roi[1], roi[3], roi[13], roi[-2], roi[-1]]      # neighbours, a far corner, the one outside
    runs = {}
    monkeypatch.setenv('FPL_PIPE_RESIDENT_GB', '0')
    runs['host'] = fplobjdetect.full_roi_inference(vol, None, roi, net, 0.2, str(tmp_path / 'host'), norm,
                                                   dvid_seg_info=seg, **kw)
    monkeypatch.delenv('FPL_PIPE_RESIDENT_GB')
    runs['uploaded'] = fplobjdetect.full_roi_inference(vol, None, roi, net, 0.2, str(tmp_path / 'uploaded'),
                                                       norm, dvid_seg_info=seg, **kw)
    dseg = torch.from_numpy(seg.view(np.int64)).cuda()
    runs['resident'] = fplobjdetect.full_roi_inference(vol, None, roi, net, 0.2, str(tmp_path / 'resident'),
                                                       norm, dvid_seg_info=dseg, **kw)
    plain = fplobjdetect.full_roi_inference(vol, None, roi, net, 0.2, str(tmp_path / 'plain'), norm,
                                            **dict(kw, neighbor_thresh=None))
    assert len(runs['host']['conf']) > 20
    names = sorted(f for f in os.listdir(str(tmp_path / 'host')) if f.endswith('.p'))
    assert len(names) == len(roi) + 2 and 'all_merged.p' in names
    for other in ('uploaded', 'resident'):
        for f in names:
            assert _read(str(tmp_path / other / f)) == _read(str(tmp_path / 'host' / f)), (other, f)
        assert np.array_equal(runs[other]['locs'], runs['host']['locs'])
    # the segmentation is in the result: in the suppression (all.p) and in the merge's labels
    assert _read(str(tmp_path / 'plain' / 'all.p')) != _read(str(tmp_path / 'host' / 'all.p'))


def test_evaluate_substacks_with_a_resident_segmentation(ctx, tmp_path):
    import torch
    from flypylib_amd import fplsynapses
    from tests.test_pipeline import _small_setup
    net, vol, _ = _small_setup()
    img = (vol.astype(np.float32) - 128) / 33
    det = fplobjdetect.voxel2obj(net.infer(img), 5, 1.5, (0, 0, 0), 5)
    keep = det['conf'] >= float(np.median(det['conf']))
    gt_json = str(tmp_path / 'gt.json')
    rs = np.random.RandomState(1)
    fplsynapses.tbars_to_json_format({'locs': det['locs'][keep] + rs.randint(-2, 3, (int(keep.sum()), 3)),
                                      'conf': det['conf'][keep]}, gt_json)
    seg = np.zeros(vol.shape, np.int64)
    seg[:, :, vol.shape[2] // 2:] = 1
    seg[vol.shape[0] // 2:] += 2
    seg[:, ::2] -= 7                                   # negative labels: the top bit set
    thds = [0.0, float(np.median(det['conf'])), 2.0]
    kw = dict(obj_min_dist=5, smoothing_sigma=1.5, buffer_sz=5)
    want_all, want = fplobjdetect.evaluate_substacks(net, [[img, gt_json, seg]], thds, **kw)
    unlabelled, _ = fplobjdetect.evaluate_substacks(net, [[img, gt_json]], thds, **kw)
    assert want_all.num_tp[0] > 4 and want_all.num_tp[0] < unlabelled.num_tp[0]
    for form in (seg, torch.from_numpy(seg).cuda(), seg.astype(np.int32), seg.astype(np.int16)):
        got_all, got = fplobjdetect.evaluate_substacks(net, [[img, gt_json, form]], thds, device=0, **kw)
        for a, b in zip([got_all] + got, [want_all] + want):
            for f in ('num_tp', 'tot_pred', 'tot_gt', 'pp', 'rr'):
                assert np.array_equal(getattr(a, f), getattr(b, f)), f
