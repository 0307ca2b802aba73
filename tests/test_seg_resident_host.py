"""CPU: the host side of the resident segmentation - argument validation of voxel2obj's
`seg_origin`, the resident-cap arithmetic of full_roi_inference, the coordinate preparation of
merge_border_duplicates, and that the inputs of tests/test_gpu_seg_resident.py show something
(detections, and a result the segmentation changes) on the numpy oracle."""
import numpy as np
import pytest

from flypylib_amd import _capi, fplobjdetect, fplpipeline
from oracle import voxel2obj_oracle
from tests import seg_cases as sc


def test_seg_origin_needs_a_resident_seg():
    pred = np.zeros((8, 8, 8), np.float32)
    seg = np.zeros((20, 20, 20), np.uint64)
    with pytest.raises(ValueError, match=r'\bseg\b.*device resident'):
        fplobjdetect.voxel2obj(pred, 2, 1.0, seg=seg, seg_origin=(1, 2, 3))
    with pytest.raises(ValueError, match='seg_origin needs seg'):
        fplobjdetect.voxel2obj(pred, 2, 1.0, seg_origin=(1, 2, 3))
    for bad in (seg, [1, 2, 3], 'labels.npy'):
        with pytest.raises(ValueError, match='device resident'):
            _capi.resident_labels(bad, 'who')


def test_the_new_entry_points_are_bound():
    """libfplseg.so is built at the header's ABI version (what it exports is
    tests/test_side_libraries.py's), and the box descriptor of fpl_v2o_set_seg has the header's
    layout"""
    import os
    import re
    from flypylib_amd import _segcapi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, 'include', 'fplseg.h')).read()
    lib = _segcapi.load_library()
    assert lib.fpls_abi_version() == _segcapi.ABI_VERSION == int(
        re.search(r'#define FPLS_ABI_VERSION (\d+)', hdr).group(1))
    # every entry point is a function-try-block closed by FPLS_CATCH
    src = open(os.path.join(root, 'flypylib_amd', 'csrc', 'seg', 'seg.hip')).read()
    assert len(re.findall(r'^FPLS_EXPORT int fpls_\w+\([^{]*\) try \{', src, re.M)) == 3
    assert src.count('} FPLS_CATCH()') == 3
    # fplhip.h: fpl_seg_box { const void *vol; int64_t extent[3]; int64_t origin[3]; }, tag 2
    assert _capi.C.sizeof(_capi.fpl_seg_box) == 56 and _capi.fpl_seg_box.extent.offset == 8
    assert _capi.fpl_seg_box.origin.offset == 32
    main = open(os.path.join(root, 'include', 'fplhip.h')).read()
    assert 'FPL_MEM_DEVICE_BOX = %d' % _capi.MEM_DEVICE_BOX in main
    for name in ('v2o_set_seg_box', 'gather_labels'):
        assert callable(getattr(_capi.Context, name))


def test_label_sources_are_opened_apart_from_the_grayscale(tmp_path):
    seg = np.arange(24, dtype=np.uint64).reshape(2, 3, 4)
    src = fplpipeline._open_label_source(seg)
    assert isinstance(src, fplpipeline._ArraySource) and src.extent == (2, 3, 4)
    assert fplpipeline._open_label_source(src) is src
    np.save(str(tmp_path / 'seg.npy'), seg)
    mm = fplpipeline._open_label_source('npy://' + str(tmp_path / 'seg.npy'))
    assert np.array_equal(np.asarray(mm.arr), seg)
    with pytest.raises(NotImplementedError, match='labelmap reader'):
        fplpipeline._open_label_source('http://dvid:8000')


def test_resident_cap_arithmetic(monkeypatch):
    gib = 2 ** 30
    fit = fplpipeline._labels_fit
    # labels alone within the cap, labels + grayscale over it -> the host path
    assert fit((1024, 1024, 1024), 8, 0, 8 * gib)
    assert not fit((1024, 1024, 1024), 8, 1 * gib, 8 * gib)
    assert fit((1024, 1024, 1024), 4, 1 * gib, 8 * gib)
    assert fit((1024, 1024, 1024), 8, 1 * gib, 9 * gib)              # exactly at the cap
    assert not fit((1024, 1024, 1024), 8, 1 * gib + 1, 9 * gib)
    assert not fit((0, 8, 8), 8, 0, gib) and not fit((8, 8, 8), 8, 0, 0)
    # extents whose voxel count overflows 32 bits are counted exactly
    assert not fit((4096, 4096, 4096), 8, 0, 64 * gib) and fit((4096, 4096, 4096), 8, 0, 512 * gib)
    monkeypatch.setenv('FPL_PIPE_RESIDENT_GB', '0')
    assert fplpipeline._resident_cap_bytes() == 0
    assert not fit((8, 8, 8), 8, 0, fplpipeline._resident_cap_bytes())
    monkeypatch.setenv('FPL_PIPE_RESIDENT_GB', '1.5')
    assert fplpipeline._resident_cap_bytes() == 1.5 * gib
    monkeypatch.delenv('FPL_PIPE_RESIDENT_GB')
    assert fplpipeline._resident_cap_bytes() == 64 * gib


def test_label_points_are_the_rounded_clipped_coordinates():
    """the expression merge_border_duplicates has always used: np.round (half to even), clipped
    into the volume, (x, y, z) -> (z, y, x)"""
    extent = (23, 19, 29)
    locs = np.array([[0.5, 1.5, 2.5], [3.5, 4.5, 21.5], [-0.5, -3.0, 0.49], [28.5, 18.5, 22.5],
                     [40.0, 18.49, 22.51], [27.5, 17.5, -0.51], [1e6, -1e6, 7.0]])
    want = np.clip(np.round(locs).astype(np.int64)[:, ::-1], 0, np.asarray(extent) - 1)
    got = fplpipeline._label_points(locs, extent)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert got.tolist()[:2] == [[2, 2, 0], [22, 4, 4]]              # .5 goes to the even side
    assert got.min() >= 0 and np.all(got.max(axis=0) <= np.asarray(extent) - 1)
    # ... and the host lookup through it is the one of before
    seg = sc.label_volume(np.int64)
    merged = fplpipeline.merge_border_duplicates(
        {'locs': locs, 'conf': np.linspace(1, 0.4, len(locs))}, 0.1, fplpipeline._ArraySource(seg))
    assert len(merged['conf']) == len(locs)                         # nothing within 0.1: all kept


def test_case_shapes_hit_the_tail_paths():
    pads = {dims: int(np.prod([d + 2 * sc.R for d in dims])) for _, _, dims in sc.BOXES}
    assert all(n % 256 for n in pads.values())
    assert pads[sc.BOX_C] % 4 == 2 and pads[sc.BOX_BIG] % 2 == 1
    # the volume's x edge inside a pair: pairs are cut from the flat index, so with an odd row
    # length every other row has the edge (padded x = extent - origin + r) in mid-pair
    assert any(o[2] < sc.EXTENT[2] < o[2] + d[2] and
               ((sc.EXTENT[2] - o[2] + sc.R) % 2 or (d[2] + 2 * sc.R) % 2) for _, o, d in sc.BOXES)
    for dt in (np.uint32, np.uint64, np.int64, np.int32):
        vol = sc.label_volume(dt)
        assert vol.dtype == dt and vol.shape == sc.EXTENT and len(np.unique(vol)) > 40


@pytest.mark.parametrize('kind', ['float32', 'float64', 'int32'])
def test_parity_inputs_show_something_on_the_oracle(kind):
    """each voxel2obj parity case has detections, and the segmentation changes them"""
    vol = sc.label_volume(np.uint64)
    thd = sc.prediction_thd(kind)
    for name, origin, dims in sc.V2O_BOXES:
        pred = sc.prediction(dims, kind)
        args = (pred, sc.V2O_KW['obj_min_dist'], sc.V2O_KW['smoothing_sigma'], (0, 0, 0), 0, thd)
        with_seg = voxel2obj_oracle.voxel2obj(*args, seg=sc.host_cut(vol, origin, dims), **sc.SEG_KW)
        plain = voxel2obj_oracle.voxel2obj(*args)
        assert len(with_seg['conf']) >= 8, (name, len(with_seg['conf']))
        assert not (with_seg['locs'].shape == plain['locs'].shape
                    and np.array_equal(with_seg['locs'], plain['locs'])), name
