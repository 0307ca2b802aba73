"""The device solver, host side (no GPU): components_numpy against scipy, match_sparse after
solve_component was factored out against the recorded results of the commit before, the
solver= keyword of the public calls, the one-optimum property of every case test_gpu_assign.py
compares matrix for matrix, the fifth table of the build and the C ABI of libfplassign.so."""
import os
import re

import numpy as np
import pytest

from flypylib_amd import _assigncapi, _matchcapi, _sidelib, fplobjdetect, match
from flypylib_amd.csrc import build
from tests import assign_cases as ac, match_cases as cases, side_abi_cases as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_EXPORTS = 10
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


# ---- the build and the C ABI ---------------------------------------------------------------------

def test_libfplassign_exports_exactly_the_declared_names():
    names = abi.check_exports(_assigncapi, 'fplassign.h', 'fpla', N_EXPORTS)
    assert names == {'fpla_last_error', 'fpla_abi_version', 'fpla_scratch_bytes', 'fpla_flags_count',
                     'fpla_flags_fill', 'fpla_conf_flags', 'fpla_boundaries', 'fpla_pair_costs',
                     'fpla_labels', 'fpla_solve'}


def test_every_fpla_entry_point_is_guarded():
    abi.check_guarded('assign', 'fplassign.h', 'fpla', N_EXPORTS)


def test_the_solver_is_a_fifth_table_of_the_build():
    assert build.SOLVE_LIBRARIES == (('assign', 'assign', 'fpla', 'fplassign.h', 'libfplassign.so'),)
    assert build.EVERY_LIBRARY == build.ALL_TABLES + build.SOLVE_LIBRARIES
    assert build.EVAL_LIBRARIES == (('match', 'match', 'fple', 'fplmatch.h', 'libfplmatch.so'),)
    assert _assigncapi not in _sidelib.bindings()
    assert os.path.basename(_assigncapi.LIB_PATH) == 'libfplassign.so'
    assert 'SOLVE_LIBRARIES is a fifth table' in build.__doc__
    # libfplmatch.so keeps its names, and no other library spells this one's
    assert abi.declared('fplmatch.h', 'fple') == set(_matchcapi.SIGNATURES) and len(_matchcapi.SIGNATURES) == 5
    for hdr in os.listdir(os.path.join(ROOT, 'include')):
        if hdr != 'fplassign.h':
            assert 'fpla_' not in open(os.path.join(ROOT, 'include', hdr)).read(), hdr


def test_the_library_loads_and_every_symbol_resolves():
    lib = _assigncapi.load_library()
    assert lib is _assigncapi.load_library()
    assert lib.fpla_abi_version() == _assigncapi.ABI_VERSION
    for name, (res, args) in _assigncapi.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    with pytest.raises(_assigncapi.FplAssignError) as e:
        _assigncapi.load_library('/nonexistent/x.so')
    assert str(e.value).startswith('libfplassign.so not found at /nonexistent/x.so')
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
