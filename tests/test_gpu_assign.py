"""libfplassign.so on the GPU: every stage of match.match_device against its host
specification - the costs against match.pair_costs byte for byte, the labels against
match.components_numpy as partitions, the matching against match.match_sparse (matrix for
matrix where tests/test_assign_host.py proved one optimum, by cost everywhere) - and
solver='device' of the public calls against the host solver."""
import json

import numpy as np
import pytest

from flypylib_amd import _assigncapi, fplobjdetect, fplsynapses, match
from tests import assign_cases as ac, match_cases as cases

pytestmark = pytest.mark.gpu

T = ac.T


# ---- a. costs ------------------------------------------------------------------------------------

def _cost_sets():
    yield 'jittered', cases.jittered(3, 37, 29)[:2]
    yield 'fractional', cases.fractional(5, 37, 29)
    yield 'boundary', cases.boundary(27)


@pytest.mark.parametrize('with_labels', [False, True])
@pytest.mark.parametrize('name,points', list(_cost_sets()), ids=[n for n, _ in _cost_sets()])
def test_costs_equal_pair_costs_byte_for_byte(ctx, name, points, with_labels):
    pred, gt = points
    rs = np.random.RandomState(7)
    lp, lg = (rs.randint(0, 2, len(pred)).astype(np.int64), rs.randint(0, 2, len(gt)).astype(np.int64)) \
        if with_labels else (None, None)
    for t in (T, 40.5) if name != 'boundary' else (27,):
        i, j = match.pairs_numpy(pred, gt, t)
        want = match.pair_costs(pred, gt, i, j, t, lp, lg)
        got = match.costs_device(pred, gt, i, j, t, 0, lp, lg)
        assert got[0].dtype == got[1].dtype == np.int32 and got[2].dtype == np.float64
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert got[2].tobytes() == want[2].tobytes()
        assert len(i) >= 5 and (with_labels or len(want[0]) >= 2)
        if name == 'boundary':                                    # the pairs at exactly t are dropped
            assert len(i) == 5 and len(want[0]) == (0 if with_labels else 2)
        if with_labels and name != 'boundary':
            assert 0 < len(want[0]) < len(i)                      # and so are those across labels


def test_costs_under_a_confidence_filter(ctx):
    """the filter drops the first, the last, all and none of the predictions; i is renumbered
    by the rank of the kept ones"""
    pred, gt = cases.fractional(5, 37, 29)
    t = T
    i, j = match.pairs_numpy(pred, gt, t)
    assert i[0] == 0 and i[-1] == len(pred) - 1                   # both ends have rows to lose
    n = len(pred)
    for conf in (np.r_[0.0, np.ones(n - 1)], np.r_[np.ones(n - 1), 0.0], np.zeros(n), np.ones(n),
                 np.random.RandomState(1).rand(n)):
        sel = conf >= 0.5
        renumber = np.cumsum(sel) - 1
        wi, wj, wc = match.pair_costs(pred, gt, i, j, t)
        keep = sel[wi]
        gi, gj, gc = match.costs_device(pred, gt, i, j, t, 0, conf=conf, thd=0.5)
        assert np.array_equal(gi, renumber[wi[keep]]) and np.array_equal(gj, wj[keep])
        assert gc.tobytes() == wc[keep].tobytes()
        # ... and it is the table of the selected predictions alone
        si, sj = match.pairs_numpy(pred[sel], gt, t)
        alone = match.pair_costs(pred[sel], gt, si, sj, t)
        assert np.array_equal(gi, alone[0]) and gc.tobytes() == alone[2].tobytes()
        assert (len(gi) == 0) == (not sel.any())


# ---- b. labels -----------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(ac.graph_cases()))
def test_labels_give_the_partition_of_components_numpy(ctx, name):
    n_pred, n_gt, i, j = ac.graph_cases()[name]
    info = {}
    got = match.components_device(n_pred, n_gt, i, j, 0, info=info)
    want = match.components_numpy(n_pred, i, j)
    assert ac.same_partition(got, want)
    assert np.array_equal(got, want)                              # and the same labels, at that
    if name == 'chain':
        assert 2 <= info['sweeps'] <= 16                          # 15 pairs across
    if name == 'apart':
        assert len(got) == 0


def test_labels_beyond_one_grid_stride(ctx):
    n = 70000
    assert n > _assigncapi.BLOCK * _assigncapi.MAX_BLOCKS
    i = np.arange(n, dtype=np.int32)
    j = i[::-1].copy()
    info = {}
    got = match.components_device(n, n, i, j, 0, info=info)
    assert np.array_equal(got, i) and info['sweeps'] == 2         # one to label, one to see it
    # two predictions a point: 35 000 components of two pairs
    got = match.components_device(n, n // 2, i, i // 2, 0)
    assert np.array_equal(got, i // 2 * 2)


# ---- d, e. the matching ----------------------------------------------------------------------------

def _check_matching(pred, gt, allow_mult=False, exact=True, **kw):
    """match_device against match_sparse: a valid matching over admissible pairs whose total
    cost agrees within the rounding of n_matched float64 additions; with `exact`, the same
    matrix"""
    i, j, cost = ac.admissible(pred, gt, T, kw.get('predict_lbls'), kw.get('groundtruth_lbls'))
    want = match.match_sparse(len(pred), len(gt), i, j, cost, allow_mult)
    info = {}
    got = match.match_device(pred, gt, T, 0, allow_mult=allow_mult, info=info, **kw)
    assert got.shape == want.shape and got.dtype == bool and got.format == 'csr'
    table = {(a, b): c for a, b, c in zip(i.tolist(), j.tolist(), cost.tolist())}
    gi, gj = got.nonzero()
    assert len(gi) == got.nnz                                     # no pair twice
    assert all((a, b) in table for a, b in zip(gi.tolist(), gj.tolist()))
    assert len(set(gj.tolist())) == len(gj)                       # a ground-truth point once
    if not allow_mult:
        assert len(set(gi.tolist())) == len(gi)                   # a prediction once
    wi, wj = want.nonzero()
    total = sum(table[a, b] for a, b in zip(gi.tolist(), gj.tolist()))
    best = sum(table[a, b] for a, b in zip(wi.tolist(), wj.tolist()))
    bound = max(len(gi), len(wi)) * 2.0 ** -52 * np.abs(cost).max() if len(cost) else 0.0
    print('%d pairs, %d matched: total %.17g, match_sparse %.17g, bound %.3g, %r'
          % (len(i), len(gi), total, best, bound, {k: info[k] for k in ('components', 'largest', 'overflow', 'sweeps')}))
    assert abs(total - best) <= bound
    if exact:
        assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    return info, got


@pytest.mark.parametrize('name', ac.UNIQUE + ('scene',))
def test_solve_equals_match_sparse_where_the_optimum_is_one(ctx, name):
    pred, gt = ac.scene(ac.UNIQUE) if name == 'scene' else ac.component(name)
    info, got = _check_matching(pred, gt)
    assert info['overflow'] == 0
    if name == 'scene':
        assert info['components'] == len(ac.UNIQUE) and info['largest'] == 64 and got.nnz == 24
    else:
        assert info['components'] == 1 and info['largest'] == len(ac.admissible(pred, gt)[0])
    if name == '3x3 greedy':
        assert got.nnz == 3
    if name == 'chain':
        assert got.nnz == 8 and info['sweeps'] >= 2


@pytest.mark.parametrize('name', ac.AT_THE_CAP + ('tie',))
def test_solve_at_the_cap_and_on_a_tie_by_cost(ctx, name):
    pred, gt = ac.component(name)
    info, got = _check_matching(pred, gt, exact=False)
    assert info['overflow'] == 0 and info['components'] == 1
    assert got.nnz == (1 if name == 'tie' else min(int(v) for v in name.split('x')))


@pytest.mark.parametrize('name', ac.OVER_THE_CAP)
def test_components_over_the_cap_are_solved_on_the_host(ctx, name):
    # the large component among two small ones
    pred, gt = ac.scene(('2x2', name, '3x3 greedy'))
    info, got = _check_matching(pred, gt, exact=False)
    assert info['overflow'] == 1 and info['components'] == 3 and info['largest'] == 195
    # the host solves it with match_sparse's own code: the same matrix unless optima tie
    i, j, cost = ac.admissible(pred, gt)
    want = match.match_sparse(len(pred), len(gt), i, j, cost)
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    assert got.nnz == 2 + 3 + 3


def test_solve_across_blocks_and_beyond_one_grid_stride(ctx):
    """a block takes 64 components at a time: 300 components are five blocks, the last with the
    two-pair components; 70 000 are more than SOLVE_BLOCKS blocks take in one pass, so the
    components from 65 536 on - the two-pair ones among them - are reached by the grid stride"""
    info, got = _check_matching(*ac.many_components(300, 40)[:2])
    assert info['components'] == 300 and info['largest'] == 2 and got.nnz == 300
    n, extra = 70000, 100
    assert n - extra > _assigncapi.SOLVE_BLOCKS * _assigncapi.CAP
    pred, gt, _, _ = ac.many_components(n, extra)
    info = {}
    got = match.match_device(pred, gt, T, 0, info=info)
    assert info['components'] == n and info['largest'] == 2 and info['overflow'] == 0
    assert got.shape == (n + extra, n) and got.nnz == n
    gi, gj = got.nonzero()
    assert np.array_equal(gi, np.arange(n)) and np.array_equal(gj, np.arange(n))


def test_a_nan_threshold_selects_nothing(ctx):
    pred, gt, conf = cases.jittered(ac.CURVE_SEED, 300, 280)
    p, g = {'locs': pred, 'conf': conf}, {'locs': gt}
    _same_numbers(fplobjdetect.obj_pr_curve(p, g, T, [0.5, float('nan')], device=0, solver='device'),
                  fplobjdetect.obj_pr_curve(p, g, T, [0.5, float('nan')], match='sparse'))


def test_allow_mult_is_the_lexsort_rule(ctx):
    pred, gt, _ = cases.jittered(3, 37, 29)
    _check_matching(pred, gt, allow_mult=True)
    _check_matching(*ac.scene(ac.UNIQUE), allow_mult=True)
    # a tie on cost: the lowest i wins, wherever it stands in the table
    for order in ([0, 1], [1, 0]):
        pred, gt = ac.component('tie')
        info, got = _check_matching(pred[order], gt, allow_mult=True)
        assert got.nonzero()[0].tolist() == [0]
    # with labels, and with every pair dropped by them
    pred, gt, lp, lg = ac.labelled_case()     # one optimum: tests/test_assign_host.py
    for am in (False, True):
        _check_matching(pred, gt, allow_mult=am, predict_lbls=lp, groundtruth_lbls=lg)
        info, got = _check_matching(pred, gt, allow_mult=am, predict_lbls=np.zeros(37, int),
                                    groundtruth_lbls=np.ones(29, int))
        assert got.nnz == 0


def test_nothing_to_match(ctx):
    pred, gt = cases.apart(4, 30, 40)
    info, got = _check_matching(pred, gt)
    assert got.nnz == 0 and info['components'] == 0
    none = np.zeros((0, 3))
    for a, b in ((none, gt), (pred, none)):
        got = match.match_device(a, b, T, 0)
        assert got.shape == (len(a), len(b)) and got.nnz == 0


# ---- the public path -------------------------------------------------------------------------------

def _same_numbers(a, b):
    for name in ('num_tp', 'tot_pred', 'tot_gt', 'pp', 'rr'):
        x, y = np.asarray(getattr(a, name)), np.asarray(getattr(b, name))
        assert x.shape == y.shape and np.array_equal(x, y), (name, x, y)


def test_obj_pr_curve_with_the_device_solver(ctx):
    pred, gt, conf = cases.jittered(ac.CURVE_SEED, 300, 280)
    p, g = {'locs': pred, 'conf': conf}, {'locs': gt}
    thds = ac.CURVE_THRESHOLDS
    want = fplobjdetect.obj_pr_curve(p, g, T, thds, match='sparse')
    got = fplobjdetect.obj_pr_curve(p, g, T, thds, device=0, solver='device')
    _same_numbers(got, want)
    assert (got.match != want.match).nnz == 0 and want.num_tp[0] > 200 > want.num_tp[-1] > 0
    # per threshold: the matrices of match_device are those of match_sparse
    found = match.match_device(pred, gt, T, 0, conf=conf, thresholds=thds)
    for thd, m in zip(thds, found):
        sel = conf >= thd
        i, j, cost = ac.admissible(pred[sel], gt)
        one = match.match_sparse(int(sel.sum()), len(gt), i, j, cost)
        assert m.shape == one.shape and m.nnz == one.nnz and (m != one).nnz == 0
    rs = np.random.RandomState(5)
    lp, lg = rs.randint(0, 3, len(pred)), rs.randint(0, 3, len(gt))
    for kw in ({'allow_mult': True}, {'predict_lbls': lp, 'groundtruth_lbls': lg}):
        _same_numbers(fplobjdetect.obj_pr_curve(p, g, T, thds, device=0, solver='device', **kw),
                      fplobjdetect.obj_pr_curve(p, g, T, thds, match='sparse', **kw))
    # thresholds that keep nothing, and obj_pr itself
    _same_numbers(fplobjdetect.obj_pr_curve(p, g, T, [0.5, 2.0], device=0, solver='device'),
                  fplobjdetect.obj_pr_curve(p, g, T, [0.5, 2.0], match='sparse'))
    one = fplobjdetect.obj_pr(pred, gt, T, device=True, solver='device')
    _same_numbers(one, fplobjdetect.obj_pr(pred, gt, T, match='sparse'))
    assert one.match.format == 'csr'


def test_evaluate_substacks_with_the_device_solver(ctx, tmp_path):
    from tests.trained_fixture import RECIPES, blob_region, trained_network
    off = RECIPES['vgg_like']['off']
    net = trained_network('vgg_like')
    im, _, locs = blob_region(3, 62)
    rs = np.random.RandomState(3)
    kept = locs[rs.rand(len(locs)) < 0.8]
    tbars = {'locs': kept + rs.randint(-1, 2, kept.shape), 'conf': np.ones(len(kept))}
    fn = str(tmp_path / 'gt.json')
    fplsynapses.tbars_to_json_format(tbars, fn)
    assert len(json.load(open(fn))) > 4
    seg = np.zeros((62, 62, 62), np.int64)
    seg[:, :, 31:] = 1
    seg[31:] += 2
    kw = dict(obj_min_dist=6, smoothing_sigma=1.5, buffer_sz=off + 2)
    for substack in ([im, fn], [im, fn, seg]):
        want_all, want = fplobjdetect.evaluate_substacks(net, [substack], [0.3, 0.6, 0.9], device=0, **kw)
        got_all, got = fplobjdetect.evaluate_substacks(net, [substack], [0.3, 0.6, 0.9], device=0,
                                                       solver='device', **kw)
        _same_numbers(got_all, want_all)
        _same_numbers(got[0], want[0])
        assert want_all.tot_gt[0] > 4
    assert want_all.num_tp[0] >= 1


# ---- labels ----------------------------------------------------------------------------------------

def test_labels_that_do_not_fit_int64_are_refused(ctx):
    pred, gt, _ = cases.jittered(1, 20, 20)
    ok = np.zeros(20, np.int64)
    for bad in (np.zeros(20), np.full(20, 2 ** 63 + 5, np.uint64)):
        with pytest.raises(ValueError, match="solver='host'"):
            fplobjdetect.obj_pr(pred, gt, T, bad, ok, device=0, solver='device')
        with pytest.raises(ValueError, match="solver='host'"):
            match.match_device(pred, gt, T, 0, predict_lbls=ok, groundtruth_lbls=bad)
    # ... which the host solver takes
    assert fplobjdetect.obj_pr(pred, gt, T, np.zeros(20), np.zeros(20), device=0).num_tp > 0
    # unsigned labels that fit are compared as they are
    big = np.full(20, 2 ** 62, np.uint64)
    _same_numbers(fplobjdetect.obj_pr(pred, gt, T, big, big, device=0, solver='device'),
                  fplobjdetect.obj_pr(pred, gt, T, big, big, match='sparse'))
