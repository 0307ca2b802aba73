"""The device solver, host side (no GPU): components_numpy against scipy, match_sparse after
solve_component was factored out against the recorded results of the commit before, the
solver= keyword of the public calls, the one-optimum property of every case test_gpu_assign.py
and test_gpu_assign_stages.py compare matrix for matrix, the paths the shapes of
test_gpu_assign_stages.py are chosen to reach, and what is libfplassign.so's own of its C ABI
(the rest is tests/test_side_libraries.py's)."""
import os
import re

import numpy as np
import pytest

from flypylib_amd import _assigncapi, fplobjdetect, match
from tests import assign_cases as ac, match_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = ac.T


# ---- the specification of the labelling stage ---------------------------------------------------

@pytest.mark.parametrize('name', list(ac.graph_cases()))
def test_components_numpy_gives_scipys_partition(name):
    n_pred, n_gt, i, j = ac.graph_cases()[name]
    got = match.components_numpy(n_pred, i, j)
    assert got.dtype == np.int64 and got.shape == i.shape
    assert ac.same_partition(got, ac.scipy_labels(n_pred, n_gt, i, j))
    # the label is the smallest prediction index of the component
    for k in np.unique(got):
        assert k == i[got == k].min()
    if name == 'empty':
        assert len(got) == 0
    if name == 'chain':
        assert len(i) == 15 and np.all(got == 0)
    if name == 'crowd 12 x 12':
        assert len(np.unique(got)) == 1 and len(i) > 60
    if name == 'jittered':
        assert 10 < len(np.unique(got)) <= len(i)


def test_same_partition_tells_partitions_apart():
    assert ac.same_partition([0, 0, 5], [9, 9, 2])
    assert not ac.same_partition([0, 0, 5], [9, 2, 2])
    assert not ac.same_partition([0, 0, 0], [9, 9, 2])


# ---- match_sparse is what it was -----------------------------------------------------------------

@pytest.mark.parametrize('seed', ac.GOLDEN_SEEDS)
def test_match_sparse_equals_the_recorded_results(seed):
    golden = np.load(ac.GOLDEN)
    n_pred, n_gt, i, j, cost = ac.golden_case(seed)
    for allow_mult, tag in ((False, 'one'), (True, 'mult')):
        got = match.match_sparse(n_pred, n_gt, i, j, cost, allow_mult)
        key = 'seed%d_%s' % (seed, tag)
        assert np.array_equal(got.indptr, golden[key + '_indptr'])
        assert np.array_equal(got.indices, golden[key + '_indices'])
        assert got.nnz > 200


def test_solve_component_is_the_loop_body():
    pred, gt = ac.component('3x3 greedy')
    i, j, cost = ac.admissible(pred, gt)
    mi, mj = match.solve_component(i, j, cost)
    assert list(zip(mi.tolist(), mj.tolist())) == [(0, 0), (1, 1), (2, 2)]
    optimum = cost[np.isin(i * 3 + j, mi * 3 + mj)].sum()
    assert optimum < ac.greedy_cost(i, j, cost) - 1.0           # nearest first is not optimal


# ---- the solver keyword --------------------------------------------------------------------------

def test_solver_keyword_is_checked_by_name():
    pred, gt, conf = cases.jittered(9, 60, 50)
    p, g = {'locs': pred, 'conf': conf}, {'locs': gt}
    with pytest.raises(ValueError, match="solver='device' needs device="):
        fplobjdetect.obj_pr(pred, gt, T, solver='device')
    with pytest.raises(ValueError, match="solver='device' needs device="):
        fplobjdetect.obj_pr_curve(p, g, T, [0.5], match='sparse', solver='device')
    with pytest.raises(ValueError, match="solver='device' needs device="):
        fplobjdetect.evaluate_substacks(None, [], [0.5], solver='device')
    for call in (lambda: fplobjdetect.obj_pr(pred, gt, T, solver='x'),
                 lambda: fplobjdetect.obj_pr_curve(p, g, T, [0.5], solver='x'),
                 lambda: fplobjdetect.evaluate_substacks(None, [], [0.5], solver='x')):
        with pytest.raises(ValueError, match="solver 'x': 'host' .* or 'device'"):
            call()
    assert fplobjdetect.SOLVERS == ('host', 'device')


def test_solver_host_is_the_default_result():
    pred, gt, conf = cases.jittered(9, 60, 50)
    p, g = {'locs': pred, 'conf': conf}, {'locs': gt}
    for kw in ({}, {'match': 'sparse'}, {'match': 'sparse', 'allow_mult': True}):
        want, got = fplobjdetect.obj_pr(pred, gt, T, **kw), fplobjdetect.obj_pr(pred, gt, T, solver='host', **kw)
        assert got[:5] == want[:5] and type(got.match) is type(want.match)
        assert np.array_equal(np.asarray(got.match.todense() if kw else got.match),
                              np.asarray(want.match.todense() if kw else want.match))
        want = fplobjdetect.obj_pr_curve(p, g, T, [0.2, 0.6], **kw)
        got = fplobjdetect.obj_pr_curve(p, g, T, [0.2, 0.6], solver='host', **kw)
        for a, b in zip(got[:5], want[:5]):
            assert np.array_equal(a, b)


def test_device_solver_without_its_library_raises(monkeypatch):
    """no silent fallback to scipy: the binding's error, before torch is asked for a GPU"""
    monkeypatch.setattr(_assigncapi._side, '_lib', None)
    monkeypatch.setattr(_assigncapi._side, 'path', '/nonexistent/libfplassign.so')
    pred, gt, _ = cases.jittered(1, 20, 20)
    with pytest.raises(_assigncapi.FplAssignError, match='libfplassign.so not found at /nonexistent'):
        match.match_device(pred, gt, T, 0)


def test_labels_the_kernels_cannot_compare_are_refused_by_name():
    pred, gt, _ = cases.jittered(1, 20, 20)
    ok = np.zeros(20, np.int64)
    for bad in (np.zeros(20), np.full(20, 2 ** 63, np.uint64), np.array(['a'] * 20)):
        for kw in ({'predict_lbls': bad, 'groundtruth_lbls': ok}, {'predict_lbls': ok, 'groundtruth_lbls': bad}):
            with pytest.raises(ValueError, match="solver='host'"):
                match.match_device(pred, gt, T, 0, **kw)
    with pytest.raises(ValueError, match='labels of one kind only'):
        match.match_device(pred, gt, T, 0, predict_lbls=ok)
    assert match._device_labels(np.arange(20, dtype=np.uint64), 20, 'x').dtype == np.int64
    assert match._device_labels(np.arange(20, dtype=np.int8), 20, 'x').dtype == np.int64


# ---- one optimum ---------------------------------------------------------------------------------

def test_best_two_enumerates_every_matching():
    # one pair: itself, or nothing
    assert ac.best_two([0], [0], [-3.0]) == [-3.0, 0.0]
    # two predictions on one point: the better, then the other
    assert ac.best_two([0, 1], [0, 0], [-3.0, -5.0]) == [-5.0, -3.0]
    # a tie has no gap
    first, second = ac.best_two([0, 1], [0, 0], [-4.0, -4.0])
    assert first == second == -4.0
    with pytest.raises(AssertionError):
        ac.assert_unique_optimum(2, [0, 1], [0, 0], [-4.0, -4.0])
    # 2 x 2: the diagonal against the anti-diagonal
    assert ac.best_two([0, 0, 1, 1], [0, 1, 0, 1], [-1.0, -4.0, -3.0, -1.0]) == [-7.0, -4.0]


@pytest.mark.parametrize('name', ac.UNIQUE + ('scene',))
def test_the_compared_cases_have_one_optimum(name):
    pred, gt = ac.scene(ac.UNIQUE) if name == 'scene' else ac.component(name)
    i, j, cost = ac.admissible(pred, gt)
    checked, skipped = ac.assert_unique_optimum(len(pred), i, j, cost)
    assert skipped == 0 and checked == (len(ac.UNIQUE) if name == 'scene' else 1)
    rows, cols = len(np.unique(i)), len(np.unique(j))
    if name == 'chain':
        assert (rows, cols, len(i)) == (8, 8, 15)
    elif name == '3x3 greedy':
        assert (rows, cols, len(i)) == (3, 3, 7)
    elif name != 'scene':
        r, c = (int(v) for v in name.split('x'))
        assert (rows, cols, len(i)) == (r, c, r * c)


def test_the_cap_cases_are_single_components_of_the_stated_size():
    for name in ac.AT_THE_CAP + ac.OVER_THE_CAP:
        r, c = (int(v) for v in name.split('x'))
        pred, gt = ac.component(name)
        i, j, cost = ac.admissible(pred, gt)
        assert len(i) == r * c and len(np.unique(match.components_numpy(r, i, j))) == 1
        assert (max(r, c) > _assigncapi.CAP) == (name in ac.OVER_THE_CAP)
    pred, gt = ac.component('tie')
    i, j, cost = ac.admissible(pred, gt)
    assert cost[0] == cost[1] == -22.0


def test_the_labelled_case_has_one_optimum():
    pred, gt, lp, lg = ac.labelled_case()
    i, j, cost = ac.admissible(pred, gt, T, lp, lg)
    checked, skipped = ac.assert_unique_optimum(len(pred), i, j, cost)
    assert checked >= 10 and skipped == 0


def test_the_many_components_case_is_what_it_says():
    pred, gt, n, extra = ac.many_components(300, 40)
    i, j, cost = ac.admissible(pred, gt)
    label = match.components_numpy(len(pred), i, j)
    assert len(np.unique(label)) == n and len(i) == n + extra
    assert np.array_equal(np.unique(label[i >= n]), np.arange(n - extra, n))    # the last components
    checked, skipped = ac.assert_unique_optimum(len(pred), i, j, cost)
    assert checked == n and skipped == 0
    want = match.match_sparse(len(pred), len(gt), i, j, cost)
    assert np.array_equal(want.nonzero()[0], np.arange(n)) and np.array_equal(want.nonzero()[1], np.arange(n))


def test_the_curve_case_has_one_optimum_at_every_threshold():
    pred, gt, conf = cases.jittered(ac.CURVE_SEED, 300, 280)
    for thd in ac.CURVE_THRESHOLDS:
        sel = conf >= thd
        i, j, cost = ac.admissible(pred[sel], gt)
        checked, skipped = ac.assert_unique_optimum(int(sel.sum()), i, j, cost)
        assert checked > 20 and skipped == 0


# ---- a uniqueness check that scales past 8 x 8 -----------------------------------------------------

def _random_component(seed, rows, cols, fill):
    """pairs of one random block, `fill` of its entries present, costs in (-27, 0)"""
    rs = np.random.RandomState(seed)
    present = rs.rand(rows, cols) < fill
    present[np.arange(rows), rs.randint(0, cols, rows)] = True
    i, j = np.nonzero(present)
    return i, j, -27.0 * rs.rand(len(i)) - 1e-3


@pytest.mark.parametrize('name', ac.UNIQUE)
def test_second_best_gap_is_best_twos_on_the_unique_cases(name):
    i, j, cost = ac.admissible(*ac.component(name))
    first, second = ac.best_two(i, j, cost)
    gap = ac.second_best_gap(i, j, cost)
    assert abs(gap - (second - first)) <= 1e-12 * abs(first) and gap > ac.MIN_GAP


def test_second_best_gap_is_best_twos_on_random_components():
    for seed, (rows, cols, fill) in enumerate([(2, 2, 1.0), (3, 5, 0.6), (5, 3, 0.6), (6, 6, 0.4),
                                               (8, 8, 0.3), (8, 8, 1.0), (7, 8, 0.5), (8, 4, 0.7)]):
        i, j, cost = _random_component(seed, rows, cols, fill)
        first, second = ac.best_two(i, j, cost)
        gap = ac.second_best_gap(i, j, cost)
        assert abs(gap - (second - first)) <= 1e-12 * abs(first), (seed, gap, first, second)
        assert gap > 0
    # made to tie: two rows, two columns, both diagonals cost the same
    i, j, cost = np.array([0, 0, 1, 1]), np.array([0, 1, 0, 1]), np.array([-3.0, -5.0, -4.0, -6.0])
    assert ac.best_two(i, j, cost) == [-9.0, -9.0] and ac.second_best_gap(i, j, cost) == 0.0
    # ... and inside a larger component: the tied 2 x 2 hangs on a unique 6 x 6 by one pair
    i6, j6, c6 = _random_component(4, 6, 6, 0.5)
    i, j = np.r_[i6, i + 6, 6], np.r_[j6, j + 6, 0]
    cost = np.r_[c6, cost, -1e-3]
    first, second = ac.best_two(i, j, cost)
    assert second - first < 1e-12 and ac.second_best_gap(i, j, cost) < 1e-12
    assert ac.second_best_gap(i6, j6, c6) > 1e-3
    # a single pair: leaving it out is the second best
    assert ac.second_best_gap([4], [2], [-3.5]) == 3.5
    pred, gt = ac.component('tie')
    assert ac.second_best_gap(*ac.admissible(pred, gt)) == 0.0


# ---- the compaction's shapes -----------------------------------------------------------------------

def test_the_compaction_shapes_reach_their_paths():
    B, S = _assigncapi.BLOCK, _assigncapi.SCAN_THREADS
    assert (B, S, _assigncapi.MAX_BLOCKS) == (256, 1024, 256)
    lay = {k: ac.compaction_layout(n) for k, n in ac.COMPACTION_SHAPES.items()}
    assert [ac.COMPACTION_SHAPES[k] for k in ('one', 'wave-1', 'wave', 'wave+1', 'cell-1', 'cell', 'cell+1')] \
        == [1, 63, 64, 65, 255, 256, 257]
    for k in ('one', 'wave-1', 'wave', 'wave+1', 'cell-1', 'cell'):
        assert (lay[k]['cells'], lay[k]['per']) == (1, 1)
    assert lay['cell']['last_cell'] == B and lay['cell-1']['last_cell'] == B - 1
    assert (lay['cell+1']['cells'], lay['cell+1']['per'], lay['cell+1']['last_cell']) == (2, 1, 1)
    # every scan thread busy, one cell each
    assert lay['scan_full'] == dict(entries=262144, cells=1024, per=1, last_thread=1023, last_run=1,
                                    last_cell=256)
    # runs of 2: thread 512 owns the one-entry last cell alone, threads 513 onwards own none
    assert lay['scan_one_over'] == dict(entries=262145, cells=1025, per=2, last_thread=512, last_run=1,
                                        last_cell=1)
    # runs of 3: thread 683 is the last, its run is full, its last cell holds 3 entries
    assert lay['scan_runs_3'] == dict(entries=524547, cells=2050, per=3, last_thread=683, last_run=1,
                                      last_cell=3)
    assert lay['scan_runs_3']['last_thread'] < S - 1 and 2050 % 3 != 0
    assert max(ac.COMPACTION_SHAPES.values()) < 800000
    # the scratch holds the total and a cell's count each
    for n in ac.COMPACTION_SHAPES.values():
        assert _assigncapi.scratch_bytes(n) >= 8 + 4 * ac.compaction_layout(n)['cells']
    # the existing suite's largest list: one cell a thread
    assert ac.compaction_layout(70100)['cells'] == 274 and ac.compaction_layout(70100)['per'] == 1


@pytest.mark.parametrize('shape', list(ac.COMPACTION_SHAPES))
def test_the_flag_patterns_are_what_they_say(shape):
    n = ac.COMPACTION_SHAPES[shape]
    lay = ac.compaction_layout(n)
    counts = {p: int(np.count_nonzero(ac.flag_pattern(p, n))) for p in ac.FLAG_PATTERNS}
    assert counts['none'] == 0 and counts['all'] == n and counts['first'] == counts['last'] == 1
    assert counts['every 257th'] == -(-n // 257)
    assert ac.flag_pattern('first', n)[0] == 1 and ac.flag_pattern('last', n)[-1] == 1
    odd = ac.flag_pattern('any non-zero', n)
    assert odd.dtype == np.int32 and odd[-1] == ac.INT32_MIN == -2 ** 31
    if n >= 63:
        assert {-1, 2, ac.INT32_MIN, 0} <= set(odd.tolist()) and 0.3 * n < counts['any non-zero'] < 0.8 * n
        assert 0.3 * n < counts['half'] < 0.7 * n
    if lay['per'] > 1:
        # an offset error cannot hide in empty cells: under 'half' every scan run holds flags,
        # the last, short one too; under 'every 257th' most cells hold exactly one
        cells = np.add.reduceat(ac.flag_pattern('half', n) != 0, np.arange(0, n, _assigncapi.BLOCK))
        runs = np.add.reduceat(cells, np.arange(0, lay['cells'], lay['per']))
        assert len(runs) == lay['last_thread'] + 1 and (runs > 0).all()
        assert ac.flag_pattern('half', n)[-lay['last_cell']:].any()
        sparse = np.add.reduceat(ac.flag_pattern('every 257th', n), np.arange(0, n, _assigncapi.BLOCK))
        assert set(sparse.tolist()) == {0, 1}
    a, b, c = ac.compaction_columns(n)
    assert a.dtype == b.dtype == np.int32 and c.dtype == np.float64 and len(a) == len(b) == len(c) == n
    assert np.isnan(c[0]) and (n == 1 or (c[-1] == 0 and np.signbit(c[-1])))
    if n >= 63:
        bits = c.view(np.uint64)
        assert len(set(bits[np.isnan(c)].tolist())) == 2              # NaN of two payloads
        assert np.any((c == 0) & np.signbit(c)) and np.any((c == 0) & ~np.signbit(c))
    idx, rank = ac.compaction_reference(odd)
    assert np.array_equal(rank[idx], np.arange(len(idx))) and (rank >= 0).sum() == len(idx)


def test_the_stride_cases_stride():
    stride = _assigncapi.BLOCK * _assigncapi.MAX_BLOCKS
    assert ac.STRIDE == stride == 65536 and ac.STRIDE_SIZES == (65537, 196611)
    for n in ac.STRIDE_SIZES:
        for thd in ac.THRESHOLDS:
            conf = ac.conf_case(n, thd)
            assert len(conf) == n and np.isnan(conf).any() and np.isposinf(conf).any() and np.isneginf(conf).any()
            with np.errstate(invalid='ignore'):
                want = conf >= thd
            if np.isnan(thd):
                assert not want.any()
                continue
            if np.isneginf(thd):
                assert want.sum() == n - np.isnan(conf).sum()
            assert (conf == thd).sum() > 100 and 0 < want.sum() < n
            if np.isfinite(thd):
                below, above = np.nextafter(thd, -np.inf), np.nextafter(thd, np.inf)
                assert below < thd < above and (conf == below).sum() > 100 and (conf == above).sum() > 100
            # the special values lie on both sides of every multiple of the stride, and at the ends
            for k in list(range(stride, n, stride)) + [8, n - 8]:
                near = conf[k - 8:k + 8]
                with np.errstate(invalid='ignore'):
                    assert (near >= thd).any() and not (near >= thd).all()
        runs = ac.key_case('runs', n)
        assert runs.dtype == np.int32 and np.all(np.diff(runs) >= 0)
        assert runs[0] != runs[1] and runs[-1] != runs[-2] and runs[1] == runs[2] and runs[-2] == runs[-3]
        assert 100 < len(np.unique(runs)) < n // 100 + 3
        for k in range(stride, n - 1, stride):                        # a run across the stride
            assert runs[k - 1] == runs[k] == runs[k + 1]
        assert len(np.unique(ac.key_case('all equal', n))) == 1
        assert len(np.unique(ac.key_case('all distinct', n))) == n
    # at STRIDE + 1 entries the one strided entry is a run of its own; at three times that, runs
    # cross entries 65 535 / 65 536, 131 071 / 131 072 and 196 607 / 196 608
    assert len(range(stride, ac.STRIDE_SIZES[0] - 1, stride)) == 0
    assert len(range(stride, ac.STRIDE_SIZES[1] - 1, stride)) == 3


@pytest.mark.parametrize('name', list(ac.COST_CUBES))
def test_the_cost_tables_are_longer_than_a_stride(name):
    pred, gt, i, j = ac.cost_table(name)
    rows = ac.COST_POINTS ** 2
    assert rows == len(i) == 90000 > ac.STRIDE and len(pred) == len(gt) == 300 > _assigncapi.BLOCK
    assert np.array_equal(i, np.repeat(np.arange(300), 300)) and np.array_equal(j, np.tile(np.arange(300), 300))
    integer = ac.COST_CUBES[name][1]
    assert np.array_equal(pred, np.rint(pred)) == integer
    kept = len(match.pair_costs(pred, gt, i, j, T)[0])
    if name.startswith('full'):
        assert kept == rows
        # the table is the one pairs_numpy finds
        pi, pj = match.pairs_numpy(pred, gt, T)
        assert np.array_equal(pi, i) and np.array_equal(pj, j)
    else:
        assert 0.4 * rows < kept < 0.6 * rows
        # admissible rows lie beyond the first stride as well as within it
        keep = np.linalg.norm(pred[i] - gt[j], axis=1) < T
        assert 0.3 < keep[ac.STRIDE:].mean() < 0.7
    rs = np.random.RandomState(7)
    lp, lg = rs.randint(0, 2, 300), rs.randint(0, 2, 300)
    assert 0.4 * kept < len(match.pair_costs(pred, gt, i, j, T, lp, lg)[0]) < 0.6 * kept


# ---- long graphs -------------------------------------------------------------------------------------

@pytest.mark.parametrize('permuted', [False, True])
def test_the_long_chain_is_one_component_with_its_label_in_the_middle(permuted):
    i, j = ac.long_chain(200, permuted)
    assert len(i) == 399 and i.dtype == j.dtype == np.int32
    assert set(zip(i.tolist(), j.tolist())) == set(zip(*(v.tolist() for v in ac.long_chain(200, not permuted))))
    in_order = np.array_equal(np.lexsort((j, i)), np.arange(399))
    assert in_order != permuted
    # prediction 0 is joined to the points 99 and 100 of the chain's 200
    assert sorted(j[i == 0].tolist()) == [99, 100]
    got = match.components_numpy(200, i, j)
    assert np.all(got == 0) and ac.same_partition(got, ac.scipy_labels(200, 200, i, j))


# ---- mid-size sparse components ----------------------------------------------------------------------

def test_the_rod_list_is_the_one_checked():
    assert len(ac.ROD_CASES) == 23 and (2, 64, 9, 120) not in ac.ROD_CASES
    assert {(n, m) for _, n, m, _ in ac.ROD_CASES} == {(20, 17), (17, 20), (40, 33), (33, 40), (64, 64),
                                                      (64, 40), (9, 64), (64, 9)}
    # the seed left out leaves predictions without a pair
    pred, gt = ac.rod(2, 64, 9, 120)
    assert len(np.unique(ac.admissible(pred, gt)[0])) < 64


@pytest.mark.parametrize('case', ac.ROD_CASES, ids=lambda c: 'seed%d-%dx%d' % c[:3])
def test_every_rod_is_one_sparse_component_with_one_optimum(case):
    seed, n_pred, n_gt, length = case
    pred, gt = ac.rod(seed, n_pred, n_gt, length)
    assert pred.shape == (n_pred, 3) and gt.shape == (n_gt, 3)
    i, j, cost = ac.admissible(pred, gt)
    (label, rows, cols, pairs, gap), = ac.component_gaps(n_pred, i, j, cost)
    assert (label, rows, cols, pairs) == (0, n_pred, n_gt, len(i))
    assert _assigncapi.CAP < pairs < n_pred * n_gt                # more than a chunk, and absent pairs
    assert max(rows, cols) <= _assigncapi.CAP
    assert 1.0e-3 < gap < 0.8 and gap > ac.MIN_GAP
    # in (i, j) order - the order the solver reads - rows and columns come into sight several
    # per 64-pair chunk after the first
    fresh_rows = [len(set(i[:e + 64].tolist())) - len(set(i[:e].tolist())) for e in range(64, len(i), 64)]
    fresh_cols = [len(set(j[:e + 64].tolist())) - len(set(j[:e].tolist())) for e in range(64, len(j), 64)]
    assert max(fresh_rows) >= 2
    if (n_pred, n_gt) in ((64, 64), (33, 40), (64, 40), (9, 64)):     # ... on both sides at once
        assert any(r >= 2 and c >= 2 for r, c in zip(fresh_rows, fresh_cols))


def _solve_order(pred, gt):
    """[(rows, cols, pairs)] of the components in label order, and their gaps"""
    i, j, cost = ac.admissible(pred, gt)
    found = ac.component_gaps(len(pred), i, j, cost)
    return [f[1:4] for f in found], [f[4] for f in found]


@pytest.mark.parametrize('shuffle', [False, True])
def test_the_rod_scene_has_one_optimum_per_component_and_mixes_orientations(shuffle):
    pred, gt = ac.scene_of(ac.ROD_SCENE, shuffle=shuffle)
    order, gaps = _solve_order(pred, gt)
    want = [(64, 64, 681), (2, 1, 2), (9, 64, 239), (3, 3, 7), (64, 9, 210), (17, 20, 170), (1, 1, 1)]
    assert sorted(order) == sorted(want) and min(gaps) > ac.MIN_GAP
    assert len(order) < _assigncapi.CAP                               # one chunk of one wavefront
    if not shuffle:
        assert order == want
    # among the components the wavefront solves (more than one pair), in the order it solves
    # them: a component of more than 64 pairs is followed by a smaller one whose workers are on
    # the other side (rows > columns swaps) - stale costs or numbering in LDS would show
    solved = [o for o in order if o[2] > 1]
    assert any(a[2] > 64 and b[2] < a[2] and (a[0] > a[1]) != (b[0] > b[1]) and b[0] <= a[0] + a[1]
               for a, b in zip(solved, solved[1:]))
    assert {o[0] > o[1] for o in solved} == {False, True}
    if not shuffle:
        # pred and gt in the order given: nothing was shuffled
        assert np.all(np.diff(pred[:, 1]) > -9) and np.all(np.diff(gt[:, 1]) > -9)


def test_the_cap_scenes_overflow_for_the_reason_named():
    cap = _assigncapi.CAP
    sizes = {}
    for name, part in [(ac.OVER_BY_PAIRS, ac.OVER_BY_PAIRS)] + \
            [(k, ('rod',) + v) for k, v in ac.OVER_THE_CAP_RODS.items()]:
        pred, gt = ac.scene_of(('2x2', part, '3x3 greedy'))
        order, _ = _solve_order(pred, gt)
        assert sorted(order)[:2] == [(2, 2, 4), (3, 3, 7)] and len(order) == 3
        sizes[name] = sorted(order)[2]
        # the table in (i, j) order as the solver reads the large component
        i, j, cost = ac.admissible(pred, gt)
        big = match.components_numpy(len(pred), i, j)
        big = big == np.bincount(big).argmax()
        first_rows, first_cols = len(set(i[big][:64].tolist())), len(set(j[big][:64].tolist()))
        assert first_rows <= cap and first_cols <= cap               # not over in the first chunk
    assert sizes['65x64'] == (65, 64, 4160) and 4160 > cap * cap      # over by the pair count
    r, c, pairs = sizes['65x20 rod']
    assert (r, c) == (65, 20) and 64 < pairs < cap * cap              # over on rows, chunks later
    r, c, pairs = sizes['20x65 rod']
    assert (r, c) == (20, 65) and 64 < pairs < cap * cap              # over on columns


@pytest.mark.parametrize('case', ac.TIED_RODS, ids=lambda c: '%dx%d' % c[1:3])
def test_the_integer_rods_hold_equal_costs(case):
    seed, n_pred, n_gt, length = case
    pred, gt = ac.rod(seed, n_pred, n_gt, length, integer=True)
    assert np.array_equal(pred, np.rint(pred)) and np.array_equal(gt, np.rint(gt))
    i, j, cost = ac.admissible(pred, gt)
    assert len(np.unique(cost)) < 0.6 * len(cost)                    # equal costs all over
    # ... within single rows and single columns, where they make the solver choose
    by_row = [len(cost[i == r]) - len(np.unique(cost[i == r])) for r in np.unique(i)]
    by_col = [len(cost[j == c]) - len(np.unique(cost[j == c])) for c in np.unique(j)]
    assert sum(v > 0 for v in by_row) >= 3 and sum(v > 0 for v in by_col) >= 3
    found = ac.component_gaps(n_pred, i, j, cost)
    assert max(f[3] for f in found) > 64 and max(max(f[1], f[2]) for f in found) <= _assigncapi.CAP
    if (n_pred, n_gt) == (40, 33):
        assert min(f[4] for f in found) == 0.0                        # and optima that tie exactly


# ---- the C ABI ------------------------------------------------------------------------------------

def test_the_constants_are_the_headers_and_the_hint_names_the_host_solver():
    with pytest.raises(_assigncapi.FplAssignError) as e:
        _assigncapi.load_library('/nonexistent/x.so')
    assert 'no host fallback' in str(e.value) and "solver='host'" in str(e.value)
    hdr = open(os.path.join(ROOT, 'include', 'fplassign.h')).read()
    for name, value in (('ABI_VERSION', _assigncapi.ABI_VERSION), ('BLOCK', _assigncapi.BLOCK),
                        ('MAX_BLOCKS', _assigncapi.MAX_BLOCKS), ('SCAN_THREADS', _assigncapi.SCAN_THREADS),
                        ('CAP', _assigncapi.CAP), ('SOLVE_BLOCKS', _assigncapi.SOLVE_BLOCKS)):
        assert int(re.search(r'#define FPLA_%s (\d+)' % name, hdr).group(1)) == value, name


def test_arguments_are_refused_before_the_gpu_is_touched():
    """(the addresses below are never dereferenced: every call is refused before a launch)"""
    err = _assigncapi.FplAssignError
    B = _assigncapi.BLOCK
    for n, want in ((1, 16), (B, 16), (B + 1, 16), (2 * B + 1, 24), (70000, 8 + 4 * 274)):
        assert _assigncapi.scratch_bytes(n) == want, n
    for bad in (0, -1, 2 ** 31):
        with pytest.raises(err, match=r'fpla_scratch_bytes: n .* must lie in \[1, 2\^31 - 1\]'):
            _assigncapi.scratch_bytes(bad)
    with pytest.raises(err, match='fpla_flags_count: null pointer argument'):
        _assigncapi.flags_count(0, 5, 4096, 16, None)
    with pytest.raises(err, match='fpla_flags_count: scratch of 8 bytes, fpla_scratch_bytes asks for 16'):
        _assigncapi.flags_count(256, 5, 4096, 8, None)
    with pytest.raises(err, match=r'fpla_flags_fill: capacity -1 must lie in'):
        _assigncapi.flags_fill(256, 5, 4096, 16, -1, None)
    with pytest.raises(err, match='fpla_flags_fill: an output column without its input column'):
        _assigncapi.flags_fill(256, 5, 4096, 16, 5, None, a_out=8192)
    with pytest.raises(err, match='fpla_flags_fill: a column is not aligned'):
        _assigncapi.flags_fill(256, 5, 4096, 16, 5, None, c=8196, c_out=8192)
    _assigncapi.flags_fill(256, 5, 4096, 16, 0, None)               # nothing to write is no launch
    with pytest.raises(err, match='fpla_conf_flags: null pointer argument'):
        _assigncapi.conf_flags(256, 5, 0.5, 0, None)
    with pytest.raises(err, match='fpla_boundaries: null pointer argument'):
        _assigncapi.boundaries(256, 5, 0, None)
    costs = (256, 512, 5, 1024, 3, 2048, 4, 27.0, 0, 0, 0.0, 0, 4096, 8192, 16384, None)
    for at, value, msg in ((0, 0, 'null pointer argument'), (2, 0, r'rows 0 must lie in'),
                           (4, 2 ** 31, r'n_pred 2147483648 must lie in'),
                           (7, float('inf'), 'the threshold inf is not finite'),
                           (8, 64, 'labels of one kind only'), (13, 8196, 'a column is not aligned')):
        args = list(costs)
        args[at] = value
        with pytest.raises(err, match='fpla_pair_costs: ' + msg):
            _assigncapi.pair_costs(*args)
    with pytest.raises(err, match='fpla_labels: max_sweeps 0 must be positive'):
        _assigncapi.labels(256, 512, 5, 3, 4, 1024, 2048, 4096, 8192, 0, None)
    with pytest.raises(err, match='fpla_labels: null pointer argument'):
        _assigncapi.labels(256, 512, 5, 3, 4, 1024, 2048, 0, 8192, 9, None)
    with pytest.raises(err, match='fpla_solve: 6 components of 5 pairs'):
        _assigncapi.solve(256, 512, 1024, 5, 2048, 6, 4096, 8192, None)
    with pytest.raises(err, match='fpla_solve: null pointer argument'):
        _assigncapi.solve(256, 512, 1024, 5, 2048, 2, 0, 8192, None)
