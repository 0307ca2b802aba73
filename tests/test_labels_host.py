"""Labels and mask around T-bars, host side (no GPU): the per-voxel rule of
flypylib_amd/labels.py against the unchanged fplsynapses.write_labels_mask it specifies, the
planners of the device path, and the C ABI of libfpllabels.so."""
import os
import re

import numpy as np
import pytest

from flypylib_amd import _labelscapi, fplsynapses, labels
from tests import labels_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'synapses.npz'))


def _host(tbars, roi, ru, ri, buf):
    return fplsynapses.write_labels_mask(tbars, roi, ru, ri, buf, None)


def _spec(tbars, roi, ru, ri, buf):
    return labels.labels_mask_numpy(labels.plan_tbars(tbars, roi.shape, ru, ri), roi, ru, ri, buf)


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)


@pytest.mark.parametrize('i', range(len(cases.RULE_CASES)))
def test_labels_mask_numpy_equals_the_host_loop(i):
    tbars, roi, ru, ri, buf = cases.rule_case(i)
    want = _host(tbars, roi, ru, ri, buf)
    _same(_spec(tbars, roi, ru, ri, buf), want)
    assert want[0].any()
    if buf == 0:
        assert not want[1].any()
    elif roi.shape == cases.RULE_SHAPES[0]:
        # roi values other than 0 / 1 survive outside every cube (40 cubes leave room in the
        # larger volume; they cover the smaller one)
        assert set(np.unique(want[1]).tolist()) >= {0, 1, 2, 255}


def test_the_order_of_the_list_matters_and_the_rule_follows_it():
    changed = 0
    for i in range(len(cases.RULE_CASES)):
        tbars, roi, ru, ri, buf = cases.rule_case(i)
        back = {'locs': tbars['locs'][::-1].copy(), 'conf': tbars['conf']}
        want, want_back = _host(tbars, roi, ru, ri, buf), _host(back, roi, ru, ri, buf)
        _same(_spec(back, roi, ru, ri, buf), want_back)
        assert np.array_equal(want[0], want_back[0])          # labels never depend on it
        changed += not np.array_equal(want[1], want_back[1])
    assert changed >= 3


def test_labels_mask_numpy_reproduces_the_reference_output():
    roi = np.ones((36, 38, 40), 'uint8')
    got = _spec(cases.GOLDEN_TBARS, roi, 3, 6, 4)
    assert np.array_equal(got[0], GOLD['lm_labels']) and np.array_equal(got[1], GOLD['lm_mask'])
    assert got[0].dtype == np.uint8 and got[1].dtype == np.uint8


def test_empty_single_and_duplicated_lists():
    shape = (23, 17, 29)
    roi = cases.random_roi(7, shape)
    for locs in (np.zeros((0, 3)), np.array([[14., 8, 11]]),
                 np.array([[14., 8, 11], [16, 9, 12], [14, 8, 11]])):
        tbars = {'locs': locs, 'conf': np.ones(len(locs))}
        table = labels.plan_tbars(tbars, shape, 3, 6)
        assert table.dtype == np.int32 and table.shape == (len(locs), 3)
        _same(labels.labels_mask_numpy(table, roi, 3, 6, 2), _host(tbars, roi, 3, 6, 2))
    empty = labels.labels_mask_numpy(np.zeros((0, 3), np.int32), roi, 3, 6, 2)
    assert not empty[0].any() and np.array_equal(empty[1][2:-2, 2:-2, 2:-2], roi[2:-2, 2:-2, 2:-2])
    # the duplicate sets again what its own ignore ball cleared
    assert _host(tbars, roi, 3, 6, 2)[1][11, 8, 14] == 1


def test_plan_tbars_truncates_as_the_host_does():
    t = labels.plan_tbars({'locs': np.array([[10.9, 8.2, 11.99, 0.5]])}, (23, 17, 29), 3, 6)
    assert t.tolist() == [[10, 8, 11]]
    with pytest.raises(ValueError, match='integers >= 0'):
        labels.plan_tbars({'locs': np.zeros((0, 3))}, (23, 17, 29), 2.5, None)
    with pytest.raises(ValueError, match='integers >= 0'):
        labels.plan_tbars({'locs': np.zeros((0, 3))}, (23, 17, 29), 3, -1)
    with pytest.raises(ValueError, match='buffer_size'):
        labels.labels_mask_numpy(np.zeros((0, 3), np.int32), np.ones((8, 8, 8), np.uint8), 1, 2, -1)


@pytest.mark.parametrize('ru, ri', [(3, 6), (4, None), (5, 3)])
def test_a_cube_that_leaves_the_volume_is_refused_on_every_face(ru, ri):
    """... by plan_tbars by name, and by the host loop with numpy's broadcast error"""
    shape = (36, 38, 40)
    h = cases.half_width(ru, ri)
    inside = [20., 19, 18]
    for axis in range(3):
        for pos in (h - 1, shape[2 - axis] - h):
            bad = list(inside)
            bad[axis] = pos + 0.5
            tbars = {'locs': np.array([inside, bad, inside]), 'conf': np.ones(3)}
            with pytest.raises(ValueError, match=r'T-bar 1 at \(x, y, z\) = .* leaves the'):
                labels.plan_tbars(tbars, shape, ru, ri)
            with pytest.raises(ValueError, match='broadcast'):
                _host(tbars, np.ones(shape, np.uint8), ru, ri, 2)
            bad[axis] += 1 if pos == h - 1 else -1              # one step inwards: accepted
            labels.plan_tbars({'locs': np.array([bad])}, shape, ru, ri)


def test_half_width_zero_is_the_documented_difference():
    """the host addresses an empty slice and raises nothing; plan_tbars refuses"""
    shape = (8, 9, 10)
    tbars = {'locs': np.array([[10., 4, 4]]), 'conf': np.ones(1)}
    ll, mm = _host(tbars, np.ones(shape, np.uint8), 0, None, 1)
    assert not ll.any()
    with pytest.raises(ValueError, match='T-bar 0'):
        labels.plan_tbars(tbars, shape, 0, None)
    assert 'half-width 0' in labels.plan_tbars.__doc__


def _pairs_brute(locs, shape, half, brick):
    nb = labels.brick_counts(shape, brick)
    want = set()
    for j, (x, y, z) in enumerate(locs.tolist()):
        for bz in range(nb[0]):
            for by in range(nb[1]):
                for bx in range(nb[2]):
                    lo = (bz * brick[0], by * brick[1], bx * brick[2])
                    hi = tuple(min(l + b, d) - 1 for l, b, d in zip(lo, brick, shape))
                    if all(c + half >= l and c - half <= h
                           for c, l, h in zip((z, y, x), lo, hi)):
                        want.add((j, (bz * nb[1] + by) * nb[2] + bx))
    return want


@pytest.mark.parametrize('shape, half, brick', [((23, 17, 29), 6, labels.BRICK),
                                                ((70, 45, 131), 6, labels.BRICK),
                                                ((36, 38, 40), 0, labels.BRICK),
                                                ((30, 29, 31), 5, (4, 8, 16))])
def test_plan_bricks_lists_every_pair_whose_cube_meets_the_brick(shape, half, brick):
    locs = labels.plan_tbars(cases.random_tbars(3, shape, half, 60), shape, half, None)
    # T-bars in the last, partial bricks of every axis
    locs[:3] = [[shape[2] - half - 1, shape[1] - half - 1, shape[0] - half - 1]] * 3
    offsets, index = labels.plan_bricks(locs, shape, half, brick)
    nb = labels.brick_counts(shape, brick)
    assert offsets.dtype == np.int32 and index.dtype == np.int32
    assert len(offsets) == nb[0] * nb[1] * nb[2] + 1 and offsets[0] == 0
    assert offsets[-1] == len(index) and (np.diff(offsets) >= 0).all()
    got = {(int(j), b) for b in range(len(offsets) - 1) for j in index[offsets[b]:offsets[b + 1]]}
    assert len(got) == len(index)                               # no pair twice
    assert got == _pairs_brute(locs, shape, half, brick)
    last = len(offsets) - 2
    assert {0, 1, 2} <= set(index[offsets[last]:offsets[last + 1]].tolist())
    empty = labels.plan_bricks(np.zeros((0, 3), np.int32), shape, half, brick)
    assert not empty[0].any() and len(empty[1]) == 0


# ---- the C ABI of libfpllabels.so ---------------------------------------------------------------

def test_the_other_libraries_keep_their_export_lists():
    """the labels entry points live in a library of their own"""
    for hdr in ('fplhip.h', 'fplbatch.h', 'fplmine.h'):
        assert 'fpll_' not in open(os.path.join(ROOT, 'include', hdr)).read()
    csrc = os.path.join(ROOT, 'flypylib_amd', 'csrc')
    for d in (csrc, os.path.join(csrc, 'batchgen'), os.path.join(csrc, 'mine')):
        for f in os.listdir(d):
            if f.endswith(('.hip', '.h')):
                assert 'fpll_' not in open(os.path.join(d, f)).read(), f


def test_refused_calls_leave_a_message_and_touch_no_gpu():
    lib = _labelscapi.load_library()
    assert lib.fpll_abi_version() == _labelscapi.ABI_VERSION
    hdr = open(os.path.join(ROOT, 'include', 'fpllabels.h')).read()
    assert int(re.search(r'#define FPLL_ABI_VERSION (\d+)', hdr).group(1)) == _labelscapi.ABI_VERSION
    assert tuple(int(re.search(r'#define FPLL_BRICK_%s (\d+)' % a, hdr).group(1))
                 for a in 'ZYX') == _labelscapi.BRICK == labels.BRICK
    assert int(re.search(r'#define FPLL_MAX_RADIUS (\d+)', hdr).group(1)) == _labelscapi.MAX_RADIUS
    call = _labelscapi.labels_mask
    with pytest.raises(_labelscapi.FplLabelsError, match='fpll_labels_mask: null pointer'):
        call(0, 0, 0, 0, 0, 0, (8, 8, 8), 3, 6, 4, 0, 0, 0)
    with pytest.raises(_labelscapi.FplLabelsError, match='fpll_labels_mask: null pointer'):
        call(256, 0, 0, 0, 0, 0, (8, 8, 8), 3, 6, 4, 512, 0, 0)
    # a table without its rows (the addresses below are never dereferenced)
    with pytest.raises(_labelscapi.FplLabelsError, match=r'null pointer argument \(a table of 5'):
        call(4096, 0, 2, 256, 256, 5, (8, 8, 8), 3, 6, 4, 8192, 12288, 0)
    # 2048 x 1024 x 1024 = 2^31 voxels: refused by name before any pointer is followed
    with pytest.raises(_labelscapi.FplLabelsError, match=r'exceeds the 2\^31 - 1 voxels'):
        call(256, 0, 0, 0, 0, 0, (2048, 1024, 1024), 3, 6, 4, 256, 256, 0)
    with pytest.raises(_labelscapi.FplLabelsError, match=r'must lie in \[0, 1024\]'):
        call(4096, 0, 0, 0, 0, 0, (8, 8, 8), 3, 1025, 4, 8192, 12288, 0)
    with pytest.raises(_labelscapi.FplLabelsError, match=r'must lie in \[0, 1024\]'):
        call(4096, 0, 0, 0, 0, 0, (8, 8, 8), -1, 0, 4, 8192, 12288, 0)
    with pytest.raises(_labelscapi.FplLabelsError, match='buffer_size -2 must not be negative'):
        call(4096, 0, 0, 0, 0, 0, (8, 8, 8), 3, 6, -2, 8192, 12288, 0)
    with pytest.raises(_labelscapi.FplLabelsError, match='dims .* must be positive'):
        call(4096, 0, 0, 0, 0, 0, (8, 0, 8), 3, 6, 4, 8192, 12288, 0)
    with pytest.raises(_labelscapi.FplLabelsError, match='not aligned to an int32'):
        call(4096, 258, 2, 256, 256, 5, (8, 8, 8), 3, 6, 4, 8192, 12288, 0)
    with pytest.raises(_labelscapi.FplLabelsError, match='must be distinct buffers'):
        call(4096, 0, 0, 0, 0, 0, (8, 8, 8), 3, 6, 4, 8192, 8192 + 100, 0)
    with pytest.raises(_labelscapi.FplLabelsError, match='must be distinct buffers'):
        call(4096, 0, 0, 0, 0, 0, (8, 8, 8), 3, 6, 4, 4096, 12288, 0)


def test_the_host_path_is_the_default_and_the_device_path_refuses_misuse(tmp_path):
    roi = np.ones((36, 38, 40), 'uint8')
    ll, mm = fplsynapses.write_labels_mask(cases.GOLDEN_TBARS, roi, 3, 6, 4, str(tmp_path / 'x'))
    assert isinstance(ll, np.ndarray) and np.array_equal(ll, GOLD['lm_labels'])
    assert np.array_equal(mm, GOLD['lm_mask'])
    assert sorted(p.name for p in tmp_path.iterdir()) == ['x_labels.h5', 'x_labels.npy',
                                                          'x_mask.h5', 'x_mask.npy']
    with pytest.raises(ValueError, match='non-empty'):
        labels.check_shape((4, 0, 4))
    with pytest.raises(ValueError, match=r'exceeds the 2\^31 - 1 voxels'):
        labels.check_shape((2048, 1024, 1024))
