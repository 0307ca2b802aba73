"""The device planner of write_labels_mask, host side (no GPU): labels.plan_pairs against
labels.plan_bricks, the planner keyword of the public call and what is libfplplan.so's own of
its C ABI (the rest is tests/test_side_libraries.py's)."""
import os
import re

import numpy as np
import pytest

from flypylib_amd import _labelscapi, _plancapi, fplsynapses, labels
from tests import labels_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('i', range(len(cases.RULE_CASES)))
def test_plan_pairs_is_the_length_of_the_index(i):
    tbars, roi, ru, ri, _ = cases.rule_case(i)
    locs = labels.plan_tbars(tbars, roi.shape, ru, ri)
    for half in (0, 2, cases.half_width(ru, ri)):
        pairs = labels.plan_pairs(locs, roi.shape, half)
        assert isinstance(pairs, int) and pairs == len(labels.plan_bricks(locs, roi.shape, half)[1])
        assert pairs >= len(locs)
    assert labels.plan_pairs(np.zeros((0, 3), np.int32), roi.shape, 3) == 0


def test_plan_pairs_refuses_more_pairs_than_int32_rows():
    """33 x 17 x 2 = 1 122 bricks per T-bar, 2 000 000 T-bars: 2.244e9 pairs, arithmetic only"""
    locs = np.full((2000000, 3), 64, np.int32)
    assert labels.plan_pairs(locs[:1], (129, 129, 129), 64) == 33 * 17 * 2
    with pytest.raises(ValueError, match='2244000000 .* pairs exceed the int32 brick tables'):
        labels.plan_pairs(locs, (129, 129, 129), 64)


def test_the_planner_keyword_is_checked_by_name():
    roi = np.ones((36, 38, 40), np.uint8)
    with pytest.raises(ValueError, match="planner 'numpy': 'host' .* or 'device'"):
        fplsynapses.write_labels_mask(cases.GOLDEN_TBARS, roi, 3, 6, 4, None, planner='numpy')
    with pytest.raises(ValueError, match="planner 'numpy'"):
        fplsynapses.write_labels_mask(cases.GOLDEN_TBARS, roi, 3, 6, 4, None, device=0,
                                      planner='numpy')
    with pytest.raises(ValueError, match="planner='device' needs device=<int>"):
        fplsynapses.write_labels_mask(cases.GOLDEN_TBARS, roi, 3, 6, 4, None, planner='device')
    with pytest.raises(ValueError, match='planner None'):
        labels.check_planner(None)
    # the default is the host planner, and naming it changes nothing on the host path
    want = fplsynapses.write_labels_mask(cases.GOLDEN_TBARS, roi, 3, 6, 4, None)
    got = fplsynapses.write_labels_mask(cases.GOLDEN_TBARS, roi, 3, 6, 4, None, planner='host')
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert labels.PLANNERS == ('host', 'device')


# ---- the C ABI of libfplplan.so -----------------------------------------------------------------

def test_the_other_libraries_keep_their_export_lists():
    """the planner's entry points live in a library of their own"""
    for hdr in ('fplhip.h', 'fplbatch.h', 'fplmine.h', 'fpllabels.h'):
        assert 'fplp_' not in open(os.path.join(ROOT, 'include', hdr)).read()
    csrc = os.path.join(ROOT, 'flypylib_amd', 'csrc')
    for d in (csrc, os.path.join(csrc, 'batchgen'), os.path.join(csrc, 'mine'),
              os.path.join(csrc, 'labels')):
        for f in os.listdir(d):
            if f.endswith(('.hip', '.h')):
                assert 'fplp_' not in open(os.path.join(d, f)).read(), f


def test_the_constants_are_the_headers():
    hdr = open(os.path.join(ROOT, 'include', 'fplplan.h')).read()
    assert int(re.search(r'#define FPLP_ABI_VERSION (\d+)', hdr).group(1)) == _plancapi.ABI_VERSION
    assert tuple(int(re.search(r'#define FPLP_BRICK_%s (\d+)' % a, hdr).group(1))
                 for a in 'ZYX') == _plancapi.BRICK == _labelscapi.BRICK == labels.BRICK
    assert (int(re.search(r'#define FPLP_MAX_RADIUS (\d+)', hdr).group(1)) == _plancapi.MAX_RADIUS
            == _labelscapi.MAX_RADIUS)


def test_scratch_bytes_is_the_documented_layout():
    """16 B of status word, 8 B per tile of 1 024 bricks, 4 B per brick, 4 B per pair"""
    assert _plancapi.scratch_bytes(0, 1, 0) == 16 + 8 + 4
    assert _plancapi.scratch_bytes(7, 1024, 10) == 16 + 8 + 4 * 1024 + 40
    assert _plancapi.scratch_bytes(7, 1025, 10) == 16 + 16 + 4 * 1025 + 40
    assert _plancapi.scratch_bytes(32768, 42250, 335640) == 16 + 8 * 42 + 4 * 42250 + 4 * 335640
    top = 2 ** 31 - 1
    assert _plancapi.scratch_bytes(top // 3, top - 1, top) > 2 ** 34
    with pytest.raises(_plancapi.FplPlanError, match=r'fplp_scratch_bytes: 2147483647 bricks'):
        _plancapi.scratch_bytes(0, top, 0)
    with pytest.raises(_plancapi.FplPlanError, match=r'fplp_scratch_bytes: 0 bricks'):
        _plancapi.scratch_bytes(0, 0, 0)
    with pytest.raises(_plancapi.FplPlanError, match=r'n_index 2147483648 must lie in'):
        _plancapi.scratch_bytes(0, 8, top + 1)
    with pytest.raises(_plancapi.FplPlanError, match=r'n_tbars -1 must lie in'):
        _plancapi.scratch_bytes(-1, 8, 0)
    lib = _plancapi.load_library()
    assert lib.fplp_scratch_bytes(0, 8, 0, None) == 1
    assert lib.fplp_last_error() == b'fplp_scratch_bytes: null pointer argument'


def test_refused_calls_leave_a_message_and_touch_no_gpu():
    """(the addresses below are never dereferenced: every call is refused before a launch)"""
    call = _plancapi.plan_bricks
    err = _plancapi.FplPlanError
    big = 1 << 20
    # tbars, n_tbars, dims, half, offsets, index, n_index, scratch, scratch bytes, stream
    with pytest.raises(err, match='fplp_plan_bricks: null pointer argument$'):
        call(0, 0, (8, 8, 8), 2, 0, 0, 0, 4096, big, 0)
    with pytest.raises(err, match='fplp_plan_bricks: null pointer argument$'):
        call(256, 5, (8, 8, 8), 2, 512, 1024, 5, 0, big, 0)
    with pytest.raises(err, match=r'null pointer argument \(a table of 5 T-bars\)'):
        call(0, 5, (8, 8, 8), 2, 512, 1024, 5, 4096, big, 0)
    with pytest.raises(err, match=r'null pointer argument \(an index of 7 rows\)'):
        call(256, 5, (8, 8, 8), 2, 512, 0, 7, 4096, big, 0)
    with pytest.raises(err, match=r'half -1 must lie in \[0, 1024\]'):
        call(256, 5, (8, 8, 8), -1, 512, 1024, 5, 4096, big, 0)
    with pytest.raises(err, match=r'half 1025 must lie in \[0, 1024\]'):
        call(256, 5, (8, 8, 8), 1025, 512, 1024, 5, 4096, big, 0)
    with pytest.raises(err, match='dims .* must be positive'):
        call(256, 5, (8, 0, 8), 2, 512, 1024, 5, 4096, big, 0)
    # 2048 x 1024 x 1024 = 2^31 voxels: refused by name before any pointer is followed
    with pytest.raises(err, match=r'exceeds the 2\^31 - 1 voxels the brick tables can index'):
        call(256, 5, (2048, 1024, 1024), 2, 512, 1024, 5, 4096, big, 0)
    with pytest.raises(err, match=r'n_index 2147483648 must lie in'):
        call(256, 5, (8, 8, 8), 2, 512, 1024, 2 ** 31, 4096, big, 0)
    with pytest.raises(err, match=r'n_tbars 715827883 must lie in'):
        call(256, (2 ** 31 - 1) // 3 + 1, (8, 8, 8), 2, 512, 1024, 5, 4096, big, 0)
    with pytest.raises(err, match='not aligned to an int32'):
        call(258, 5, (8, 8, 8), 2, 512, 1024, 5, 4096, big, 0)
    # (8, 8, 8): 2 bricks, 5 pairs -> 16 + 8 + 8 + 20 bytes
    assert _plancapi.scratch_bytes(5, 2, 5) == 52
    with pytest.raises(err, match=r'scratch of 51 bytes, fplp_scratch_bytes asks for 52'):
        call(256, 5, (8, 8, 8), 2, 512, 1024, 5, 4096, 51, 0)
    with pytest.raises(err, match=r'scratch of 1048576 bytes, .* \(8-byte aligned\)'):
        call(256, 5, (8, 8, 8), 2, 512, 1024, 5, 4100, big, 0)
    lib = _plancapi.load_library()
    assert lib.fplp_plan_bricks(None, 0, None, 0, None, None, 0, None, 0, None) == 1
    assert lib.fplp_last_error() == b'fplp_plan_bricks: null pointer argument'
