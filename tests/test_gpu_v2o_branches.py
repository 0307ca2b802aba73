"""GPU: voxel2obj on every dispatch branch of csrc/v2o_plan.h, bit for bit against the scipy
oracle.  The cases and the branch each is there for are tests/v2o_cases.py's table;
tests/test_v2o_plan.py (CPU) holds each row to the header's plan, and the launch names checked
here tie that plan to what ran."""
import numpy as np
import pytest

from flypylib_amd import fplobjdetect
from oracle import voxel2obj_oracle
from tests import v2o_cases
from tests.v2o_cases import CASES, SEG_CASES, padded, wr_of

pytestmark = pytest.mark.gpu

_preds = {}


def _pred(case):
    """the case's prediction, made once and never written to"""
    name, kind, seed, D = case[:4]
    if name not in _preds:
        p = v2o_cases.make_pred(kind, D)
        p.setflags(write=False)
        _preds[name] = p
    return _preds[name]


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_branch_matches_the_oracle_bit_for_bit(ctx, case):
    name, kind, seed, D, r, sigma, thd, n_min, want = case
    pred = _pred(case)
    P = padded(D, r)
    w = fplobjdetect.gaussian_kernel1d(sigma, truncate=2.0)
    assert (w.size - 1) // 2 == wr_of(sigma)
    # the smoothed volume, with the launches that made it
    ctx.timing(True)
    try:
        ctx.timing_reset()
        ctx.v2o_smooth(pred, D, r, w, [])
        launched = ctx.timing_get()
    finally:
        ctx.timing(False)
    got = ctx.v2o_smoothed(P)
    ref = voxel2obj_oracle.smooth_and_clear(pred, r, sigma)
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32
    bad = np.flatnonzero(got.reshape(-1).view(np.uint32) != ref.reshape(-1).view(np.uint32))
    assert bad.size == 0, '%s: %d voxels differ, first at %s' % (
        name, bad.size, np.unravel_index(bad[0], ref.shape))
    # the launch names agree with the plan of the case's row
    windowed = want.get('windowed', True)
    fused = bool(want.get('fused', False)) and windowed
    assert 'fused' in want or not windowed, name
    assert ('v2o_gauss_yx' in launched) == fused, (name, sorted(launched))
    assert ('v2o_gauss_y' in launched) == (not fused) and ('v2o_gauss_x' in launched) == (not fused), \
        (name, sorted(launched))
    assert launched['v2o_gauss_z']['launches'] == 1
    # the point list
    ref_pts = voxel2obj_oracle.voxel2obj(pred, r, sigma, (0, 0, 0), 0, thd)
    pts = fplobjdetect.voxel2obj(pred, r, sigma, (0, 0, 0), 0, thd)
    assert len(ref_pts['conf']) >= n_min
    assert np.array_equal(pts['locs'], ref_pts['locs']), name
    assert np.array_equal(pts['conf'], ref_pts['conf']), name


@pytest.mark.parametrize('name', sorted(SEG_CASES))
def test_segmentation_aware_suppression_on_either_side_of_a_mask_word(ctx, name):
    """r = 31 (one 64-bit mask per cube row, in LDS) against r = 32 (two, in global memory); and
    the 'stage' case, where the first winner's 19^3-cell bounding box is live in every cell: more
    than touch_cell's LDS stage holds"""
    case = v2o_cases.by_name(name)
    _, kind, seed, D, r, sigma, thd, _, _ = case
    pred, seg = _pred(case), v2o_cases.make_seg(D)
    ref = voxel2obj_oracle.voxel2obj(pred, r, sigma, (0, 0, 0), 0, thd, seg=seg, seg_dilate=2)
    got = fplobjdetect.voxel2obj(pred, r, sigma, (0, 0, 0), 0, thd, seg=seg, seg_dilate=2)
    assert len(ref['conf']) >= SEG_CASES[name]
    assert np.array_equal(got['locs'], ref['locs']) and np.array_equal(got['conf'], ref['conf'])


@pytest.mark.parametrize('name', ['x574', 'lds'])
def test_order_statistics_after_either_last_pass(ctx, name):
    """the first radix level comes out of gauss_yx_fused on x574 and out of gauss_x_lds on lds"""
    case = v2o_cases.by_name(name)
    _, kind, seed, D, r, sigma, thd, _, want = case
    pred = _pred(case)
    n = int(np.prod(padded(D, r)))
    ranks = [0, n // 2, int(0.97 * (n - 1)), n - 1]
    vals = ctx.v2o_smooth(pred, D, r, fplobjdetect.gaussian_kernel1d(sigma), ranks)
    s = np.sort(voxel2obj_oracle.smooth_and_clear(pred, r, sigma).reshape(-1))
    assert np.array_equal(vals, s[ranks])
    assert vals[2] > 0 and vals[0] == 0


def test_more_detections_than_cap_is_refused_and_the_context_recovers(ctx):
    case = v2o_cases.by_name('z41')
    _, kind, seed, D, r, sigma, thd, n_min, _ = case
    pred = _pred(case)
    ref_pts = voxel2obj_oracle.voxel2obj(pred, r, sigma, (0, 0, 0), 0, thd)
    assert len(ref_pts['conf']) > 3
    n = int(np.prod(padded(D, r)))
    lo, hi, gamma = fplobjdetect.percentile_plan(n, 97, np.float32)
    lo_v, hi_v = ctx.v2o_smooth(pred, D, r, fplobjdetect.gaussian_kernel1d(sigma), [lo, hi])
    thresh = float(np.maximum(fplobjdetect.percentile_lerp(lo_v, hi_v, gamma), thd))
    with pytest.raises(Exception, match='raise cap'):
        ctx.v2o_nms(thresh, cap=3)
    got = fplobjdetect.voxel2obj(pred, r, sigma, (0, 0, 0), 0, thd)
    assert np.array_equal(got['locs'], ref_pts['locs']) and np.array_equal(got['conf'], ref_pts['conf'])
