"""near.py on the host: pairs_numpy against the self-join of match.pairs_numpy, the cell grid's
ball query, the memory the builder takes, and the C ABI of libfplnear.so as far as it can be
checked without a GPU."""
import os
import re
import tracemalloc

import numpy as np
import pytest

from flypylib_amd import _matchcapi, _nearcapi, near
from flypylib_amd.csrc import build
from tests import near_cases as cases, side_abi_cases as abi

ROOT = abi.ROOT
T = cases.T


# ---- the table ------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(cases.SETS))
def test_pairs_numpy_is_the_self_join_without_coincident_pairs(name):
    cases.check_sets()
    pts = cases.SETS[name]()
    got, want = near.pairs_numpy(pts, T), cases.self_join(pts, T)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize('seed,n,box,t', [(1, 500, 200, 30), (2, 3000, 300, 30), (3, 800, 90, 26.3),
                                          (4, 1200, 400, 5), (5, 300, 50, 200.0)])
def test_pairs_numpy_on_random_sets(seed, n, box, t):
    rs = np.random.RandomState(seed)
    for pts in (rs.randint(0, box, (n, 3)).astype(np.float64), rs.rand(n, 3) * box * 1.37 - 55.5):
        got, want = near.pairs_numpy(pts, t), cases.self_join(pts, t)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        # symmetric: both directions are stored
        i = np.repeat(np.arange(n), np.diff(got[0]))
        assert set(zip(i.tolist(), got[1].tolist())) == set(zip(got[1].tolist(), i.tolist()))


def test_small_blocks_give_the_same_table(monkeypatch):
    pts = cases.cluster()
    want = near.pairs_numpy(pts, T)
    monkeypatch.setattr(near, 'BLOCK_ELEMENTS', 50)          # below one point's candidates
    got = near.pairs_numpy(pts, T)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_empty_and_malformed_input():
    indptr, indices = near.pairs_numpy(np.zeros((0, 3)), T)
    assert indptr.tolist() == [0] and len(indices) == 0 and indices.dtype == np.int32
    with pytest.raises(ValueError, match='N x 3'):
        near.pairs_numpy(np.zeros((4, 2)), T)
    with pytest.raises(ValueError, match='finite'):
        near.pairs_numpy(np.array([[0.0, 0, np.nan]]), T)
    with pytest.raises(ValueError, match='spread too far'):
        near.pairs_numpy(np.array([[0.0, 0, 0], [1e12, 0, 0]]), T)
    with pytest.raises(ValueError, match='2\\^62'):
        near.pairs_numpy(np.array([[0.0, 0, 0], [7e9, 7e9, 7e9]]), T)     # 2^28 > each, 2^62 < all


def test_the_builder_never_holds_an_n_by_n_array():
    """10^5 points: the dense form is 80 GB of distances; the builder stays below 300 MB - a few
    hundred bytes per point and per table entry, and BLOCK_ELEMENTS candidates at a time"""
    rs = np.random.RandomState(9)
    n = 100000
    pts = rs.rand(n, 3) * 1200.0
    tracemalloc.start()
    indptr, indices = near.pairs_numpy(pts, T)
    peak = tracemalloc.get_traced_memory()[1]
    tracemalloc.stop()
    assert peak < 300 << 20 < 8 * n * n
    assert indptr[-1] == len(indices) > 4 * n
    # spot check against the exact expression
    for i in (0, 4711, n - 1):
        d = pts[i] - pts
        s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        want = np.flatnonzero((s > 0) & (s <= near.threshold2(T)))
        assert np.array_equal(indices[indptr[i]:indptr[i + 1]], want)


def test_ball_is_a_superset_of_the_exact_ball_around_any_centre():
    pts = cases.negative_fractional()
    grid = near.CellGrid(pts, T)
    rs = np.random.RandomState(3)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    centres = np.rint(rs.rand(200, 3) * (hi - lo + 120) + lo - 60)      # some outside the grid
    hits = 0
    for c in list(centres) + [pts[5], lo - 29, hi + 29, lo - 1000, hi + 1e15]:
        ball = grid.ball(c)
        assert ball.dtype == np.int64 and np.all(np.diff(ball) > 0)
        d = np.sqrt(np.sum((pts - c) ** 2, axis=1))
        assert set(np.flatnonzero(d < T).tolist()) <= set(ball.tolist())
        hits += int((d < T).sum())
    assert hits > 100
    assert len(near.CellGrid(np.zeros((0, 3)), T).ball([0, 0, 0])) == 0


def test_cell_side_keeps_partners_within_one_cell():
    c = near.cell_side(T)
    assert c >= np.sqrt(near.threshold2(T)) * (1 + 2.0 ** -20) and c < T * (1 + 2.0 ** -19)
    assert near.MAX_AXIS == 2 ** _nearcapi.MAX_AXIS_BITS


# ---- the C ABI of libfplnear.so ----------------------------------------------------------------

def test_the_other_libraries_keep_their_export_lists():
    for hdr in ('fplhip.h', 'fplbatch.h', 'fplmine.h', 'fpllabels.h', 'fplplan.h', 'fplmatch.h'):
        assert 'fpln_' not in open(os.path.join(ROOT, 'include', hdr)).read()
    for sub in ('', 'batchgen', 'mine', 'labels', 'plan', 'match', 'side'):
        d = os.path.join(abi.CSRC, sub)
        for f in os.listdir(d):
            if f.endswith(('.hip', '.h')):
                assert 'fpln_' not in open(os.path.join(d, f)).read(), f
    assert abi.declared('fplmatch.h', 'fple') == set(_matchcapi.SIGNATURES) and len(_matchcapi.SIGNATURES) == 5


def test_the_constants_are_the_headers():
    hdr = open(os.path.join(ROOT, 'include', 'fplnear.h')).read()
    for name, value in (('ABI_VERSION', _nearcapi.ABI_VERSION), ('BLOCK', _nearcapi.BLOCK),
                        ('SCAN_THREADS', _nearcapi.SCAN_THREADS),
                        ('MAX_AXIS_BITS', _nearcapi.MAX_AXIS_BITS)):
        assert int(re.search(r'#define FPLN_%s (\d+)' % name, hdr).group(1)) == value, name


def test_arguments_are_refused_before_the_gpu_is_touched():
    """every refusal here returns before a launch: no GPU is needed to see it"""
    n = 10
    assert _nearcapi.scratch_bytes(n) == 16 + 48 + 40 + 240
    for bad in (0, -1, 2 ** 31):
        with pytest.raises(_nearcapi.FplNearError, match=r'must lie in \[1, 2\^31 - 1\]'):
            _nearcapi.scratch_bytes(bad)
    origin, cell, dims = (0.0, 0.0, 0.0), near.cell_side(T), (4, 4, 4)
    ok = (4096, n, near.threshold2(T), origin, cell, dims, 8192, 16384, 32768, 1 << 20)
    with pytest.raises(_nearcapi.FplNearError, match='fpln_cell_keys: null pointer'):
        _nearcapi.cell_keys(0, n, origin, cell, dims, 8192, None)
    with pytest.raises(_nearcapi.FplNearError, match=r'axis 1, must lie in \[1, 2\^28\]'):
        _nearcapi.cell_keys(4096, n, origin, cell, (4, 2 ** 28 + 1, 4), 8192, None)
    with pytest.raises(_nearcapi.FplNearError, match=r'exceeds the 2\^62'):
        _nearcapi.cell_keys(4096, n, origin, cell, (2 ** 28, 2 ** 28, 2 ** 7), 8192, None)
    with pytest.raises(_nearcapi.FplNearError, match='cell side 0 must be finite and positive'):
        _nearcapi.cell_keys(4096, n, origin, 0.0, dims, 8192, None)
    with pytest.raises(_nearcapi.FplNearError, match='origin is not finite'):
        _nearcapi.cell_keys(4096, n, (0.0, float('nan'), 0.0), cell, dims, 8192, None)
    with pytest.raises(_nearcapi.FplNearError, match='not 8-byte aligned'):
        _nearcapi.cell_keys(4100, n, origin, cell, dims, 8192, None)

    def count(**kw):
        a = dict(zip(('locs', 'n', 't2', 'origin', 'cell', 'dims', 'keys', 'order', 'scratch', 'nscr'), ok))
        a.update(kw)
        return _nearcapi.pairs_count(*a.values(), None)
    with pytest.raises(_nearcapi.FplNearError, match='fpln_pairs_count: null pointer'):
        count(order=0)
    with pytest.raises(_nearcapi.FplNearError, match='T2 -1 must be finite and positive'):
        count(t2=-1.0)
    with pytest.raises(_nearcapi.FplNearError, match=r'is below sqrt\(T2\) \(1 \+ 2\^-20\)'):
        count(cell=float(T))
    with pytest.raises(_nearcapi.FplNearError, match='scratch of 100 bytes, fpln_scratch_bytes asks for 344'):
        count(nscr=100)
    with pytest.raises(_nearcapi.FplNearError, match='fpln_pairs_fill: capacity -1 must lie in'):
        _nearcapi.pairs_fill(*ok, -1, 65536, None)
    with pytest.raises(_nearcapi.FplNearError, match='the column array is not 4-byte aligned'):
        _nearcapi.pairs_fill(*ok, 5, 65538, None)
    with pytest.raises(_nearcapi.FplNearError, match='null pointer argument \\(the column array\\)'):
        _nearcapi.pairs_fill(*ok, 5, 0, None)
    _nearcapi.pairs_fill(*ok, 0, 0, None)                    # capacity 0: nothing to do, no launch


def test_the_kernels_do_not_spill():
    """what the compiler reports for the build's own flags: no spilled register, no scratch"""
    import shutil
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    if not shutil.which(build.HIPCC) and not os.path.exists(build.HIPCC):
        pytest.skip('hipcc not available')
    import kernel_resources
    res = kernel_resources.kernel_resources('near/near.hip')
    names = ('keys_kernel', 'gather_kernel', 'count_kernel', 'scan_kernel', 'fill_kernel')
    assert len(res) == len(names) and all(any(n in k for k in res) for n in names), sorted(res)
    for name, v in res.items():
        assert v['vgpr_spill_count'] == 0 and v['sgpr_spill_count'] == 0, (name, v)
        assert v['private_segment_fixed_size'] == 0 and v['vgpr_count'] <= 128, (name, v)


def test_no_float_atomics_and_no_atomics_at_all():
    src = open(os.path.join(abi.CSRC, 'near', 'near.hip')).read()
    code = re.sub(r'//.*', '', src)
    assert 'atomic' not in code
