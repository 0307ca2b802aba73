"""Sparse matching, host side (no GPU): match.pairs_numpy / pair_costs / match_sparse against
the dense obj_pr and obj_match, the match= keyword of the public calls and what is
libfplmatch.so's own of its C ABI (the rest is tests/test_side_libraries.py's)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from flypylib_amd import _matchcapi, fplobjdetect, match
from tests import match_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = cases.T


def _point_sets():
    yield 'jittered', cases.jittered(1, 500, 549)[:2]
    yield 'integer', cases.jittered(2, 320, 300, integer=True)[:2]
    yield 'clustered', cases.clustered(3)
    yield 'apart', cases.apart(4, 40, 50)
    yield 'fractional', cases.fractional(5, 300, 280)
    yield 'boundary', cases.boundary()
    for n, m, _ in cases.SHAPES[:3] + cases.SHAPES[9:10]:
        yield 'crowd %d x %d' % (n, m), cases.crowd(n + m, n, m)


POINT_SETS = dict(_point_sets())


# ---- the C ABI of libfplmatch.so ----------------------------------------------------------------

def test_the_other_libraries_keep_their_export_lists():
    """the matching entry points live in a library of their own"""
    for hdr in ('fplhip.h', 'fplbatch.h', 'fplmine.h', 'fpllabels.h', 'fplplan.h'):
        assert 'fple_' not in open(os.path.join(ROOT, 'include', hdr)).read()
    csrc = os.path.join(ROOT, 'flypylib_amd', 'csrc')
    for d in [csrc] + [os.path.join(csrc, s) for s in ('batchgen', 'mine', 'labels', 'plan', 'side')]:
        for f in os.listdir(d):
            if f.endswith(('.hip', '.h')):
                assert 'fple_' not in open(os.path.join(d, f)).read(), f


def test_the_constants_are_the_headers():
    hdr = open(os.path.join(ROOT, 'include', 'fplmatch.h')).read()
    for name, value in (('ABI_VERSION', _matchcapi.ABI_VERSION), ('BLOCK', _matchcapi.BLOCK),
                        ('TILE', _matchcapi.TILE), ('MAX_SEGMENTS', _matchcapi.MAX_SEGMENTS),
                        ('TARGET_BLOCKS', _matchcapi.TARGET_BLOCKS),
                        ('SCAN_THREADS', _matchcapi.SCAN_THREADS)):
        assert int(re.search(r'#define FPLE_%s (\d+)' % name, hdr).group(1)) == value, name


def test_scratch_bytes_follows_the_segment_rule():
    """8 B of total and 4 B per (prediction, segment) cell; the binding's segments() is the
    library's rule"""
    rs = np.random.RandomState(0)
    shapes = [(n, m) for n, m, _ in cases.SHAPES] + [(3307, 3000), (100000, 100000), (1, 10 ** 6),
                                                      (261889, 10 ** 6), (2 ** 31 - 1, 2 ** 31 - 1)]
    shapes += [(int(n), int(m)) for n, m in rs.randint(1, 400000, (40, 2))]
    for n, m in shapes:
        g = _matchcapi.segments(n, m)
        assert _matchcapi.scratch_bytes(n, m) == 8 + 4 * n * g, (n, m)
        assert 1 <= g <= _matchcapi.MAX_SEGMENTS and g & (g - 1) == 0
        assert _matchcapi.segment_len(n, m) % _matchcapi.TILE == 0
        assert _matchcapi.segment_len(n, m) * g >= m
    assert _matchcapi.segments(3307, 3000) == 16 and _matchcapi.segments(100000, 100000) == 4
    assert _matchcapi.segments(1, 10 ** 6) == 64 and _matchcapi.segments(262145, 10 ** 6) == 1
    cases.check_shapes()
    lib = _matchcapi.load_library()
    assert lib.fple_scratch_bytes(8, 8, None) == 1
    assert lib.fple_last_error() == b'fple_scratch_bytes: null pointer argument'
    for n, m, msg in ((0, 8, r'n_pred 0 must lie in \[1, 2\^31 - 1\]'),
                      (2 ** 31, 8, r'n_pred 2147483648 must lie in'),
                      (8, 0, r'n_gt 0 must lie in'), (8, 2 ** 31, r'n_gt 2147483648 must lie in')):
        with pytest.raises(_matchcapi.FplMatchError, match='fple_scratch_bytes: ' + msg):
            _matchcapi.scratch_bytes(n, m)


def test_refused_calls_leave_a_message_and_touch_no_gpu():
    """(the addresses below are never dereferenced: every call is refused before a launch)"""
    err = _matchcapi.FplMatchError
    big = 1 << 20
    for name, call, tail in (('fple_pairs_count', _matchcapi.pairs_count, (0,)),
                             ('fple_pairs_fill', _matchcapi.pairs_fill, (5, 8192, 8192 + 64, 0))):
        # pred, n_pred, gt, n_gt, T2, scratch, scratch bytes
        with pytest.raises(err, match=name + ': null pointer argument$'):
            call(0, 5, 512, 7, 729.0, 4096, big, *tail)
        with pytest.raises(err, match=name + ': null pointer argument$'):
            call(256, 5, 0, 7, 729.0, 4096, big, *tail)
        with pytest.raises(err, match=name + ': null pointer argument$'):
            call(256, 5, 512, 7, 729.0, 0, big, *tail)
        with pytest.raises(err, match=name + r': n_pred 2147483648 must lie in \[1, 2\^31 - 1\]'):
            call(256, 2 ** 31, 512, 7, 729.0, 4096, 1 << 40, *tail)
        with pytest.raises(err, match=name + r': n_gt 2147483648 must lie in \[1, 2\^31 - 1\]'):
            call(256, 5, 512, 2 ** 31, 729.0, 4096, 1 << 40, *tail)
        with pytest.raises(err, match=name + ': n_pred 0 must lie in'):
            call(256, 0, 512, 7, 729.0, 4096, big, *tail)
        for t2 in (0.0, -1.0, float('inf'), float('nan')):
            with pytest.raises(err, match=name + ': T2 .* must be finite and positive'):
                call(256, 5, 512, 7, t2, 4096, big, *tail)
        with pytest.raises(err, match=name + ': the point tables are not aligned to a double'):
            call(260, 5, 512, 7, 729.0, 4096, big, *tail)
        assert _matchcapi.scratch_bytes(5, 7) == 28
        with pytest.raises(err, match=name + ': scratch of 27 bytes, fple_scratch_bytes asks for 28'):
            call(256, 5, 512, 7, 729.0, 4096, 27, *tail)
        with pytest.raises(err, match=name + r': scratch of 1048576 bytes, .* \(8-byte aligned\)'):
            call(256, 5, 512, 7, 729.0, 4100, big, *tail)
    with pytest.raises(err, match=r'fple_pairs_fill: null pointer argument \(an output column\)'):
        _matchcapi.pairs_fill(256, 5, 512, 7, 729.0, 4096, big, 5, 0, 8192, 0)
    with pytest.raises(err, match=r'fple_pairs_fill: capacity 2147483648 must lie in'):
        _matchcapi.pairs_fill(256, 5, 512, 7, 729.0, 4096, big, 2 ** 31, 8192, 8256, 0)
    with pytest.raises(err, match='fple_pairs_fill: an output column is not 4-byte aligned'):
        _matchcapi.pairs_fill(256, 5, 512, 7, 729.0, 4096, big, 5, 8193, 8256, 0)
    # nothing to write is no launch
    _matchcapi.pairs_fill(256, 5, 512, 7, 729.0, 4096, big, 0, 0, 0, 0)
    lib = _matchcapi.load_library()
    assert lib.fple_pairs_count(None, 0, None, 0, 1.0, None, 0, None, None) == 1
    assert lib.fple_last_error() == b'fple_pairs_count: null pointer argument'
    total = C.c_int64(-1)
    assert lib.fple_pairs_count(None, 5, None, 7, 1.0, None, 0, C.byref(total), None) == 1
    assert lib.fple_last_error() == b'fple_pairs_count: null pointer argument' and total.value == -1
    src = open(os.path.join(ROOT, 'flypylib_amd', 'csrc', 'match', 'match.hip')).read()
    # the one refusal that needs a count first (tests/test_gpu_match.py reaches it)
    assert 'pairs exceed the 2^31 - 1 rows of an int32 table' in src


def test_device_mode_without_the_library_raises(monkeypatch):
    """no silent fallback to the numpy table: the binding's error, before torch is asked for
    a GPU"""
    side = _matchcapi._side
    monkeypatch.setattr(side, '_lib', None)
    monkeypatch.setattr(side, 'path', '/nonexistent/libfplmatch.so')
    pred, gt, conf = cases.jittered(1, 20, 20)
    with pytest.raises(_matchcapi.FplMatchError, match='libfplmatch.so not found at /nonexistent'):
        fplobjdetect.obj_pr(pred, gt, T, device=0)
    with pytest.raises(_matchcapi.FplMatchError, match='libfplmatch.so not found'):
        fplobjdetect.obj_pr_curve({'locs': pred, 'conf': conf}, {'locs': gt}, T, [0.5], device=True)
    with pytest.raises(_matchcapi.FplMatchError, match='libfplmatch.so not found'):
        fplobjdetect.evaluate_substacks(None, [], [0.5], device=0)


# ---- the specification ---------------------------------------------------------------------------

def test_threshold2_is_the_stated_expression():
    assert match.threshold2(27) == 729.0 * (1 + 2.0 ** -40) > 729.0
    assert match.threshold2(np.float32(2.5)) == 6.25 * (1 + 2.0 ** -40)


@pytest.mark.parametrize('name', list(POINT_SETS))
def test_pairs_numpy_is_the_dense_test(name, monkeypatch):
    pred, gt = POINT_SETS[name]
    want = cases.dense_pairs(pred, gt, T)
    for block in (match.BLOCK_ELEMENTS, 1000, 1):        # many rows, a few rows, one row a block
        monkeypatch.setattr(match, 'BLOCK_ELEMENTS', block)
        i, j = match.pairs_numpy(pred, gt, T)
        assert i.dtype == j.dtype == np.int32
        assert np.array_equal(i, want[0]) and np.array_equal(j, want[1])
    if name == 'apart':
        assert len(want[0]) == 0
    if name == 'clustered':
        per_row = np.bincount(want[0], minlength=len(pred))
        assert per_row.max() > 100 and (per_row == 0).sum() > 50
    for a, b in ((pred[:0], gt), (pred, gt[:0])):
        i, j = match.pairs_numpy(a, b, T)
        assert len(i) == len(j) == 0 and i.dtype == np.int32


def _dense_cost(pred, gt, t, lp=None, lg=None):
    """the cost matrix of fplobjdetect.obj_pr, its expressions verbatim"""
    delta = pred.reshape(-1, 1, 3) - gt.reshape(1, -1, 3)
    cost = np.sqrt((delta ** 2).sum(axis=2)) - t
    if lp is not None:
        differ = lp.reshape(-1, 1) != lg.reshape(1, -1)
        cost += (t + 1.) * differ.astype('float32')
    return cost


def _labels(seed, pred, gt):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 3, len(pred)), rs.randint(0, 3, len(gt))


@pytest.mark.parametrize('with_labels', [False, True])
@pytest.mark.parametrize('name', list(POINT_SETS))
def test_pair_costs_keeps_exactly_the_negative_entries(name, with_labels):
    pred, gt = POINT_SETS[name]
    lp, lg = _labels(7, pred, gt) if with_labels else (None, None)
    for t in (T, 27, 26.3):
        cost = _dense_cost(pred, gt, t, lp, lg)
        i, j = match.pairs_numpy(pred, gt, t)
        ki, kj, kc = match.pair_costs(pred, gt, i, j, t, lp, lg)
        want = np.argwhere(cost < 0)
        assert np.array_equal(np.stack([ki, kj], axis=1), want)
        assert np.array_equal(kc, cost[want[:, 0], want[:, 1]])


def test_pairs_at_exactly_the_threshold_are_in_the_superset_and_dropped():
    pred, gt = cases.boundary(27)
    s = cases.dense_s(pred, gt)
    assert s[0, 0] == s[1, 1] == s[2, 2] == 729.0            # (27,0,0), (18,18,9), -(9,18,18)
    i, j = match.pairs_numpy(pred, gt, 27)
    table = set(zip(i.tolist(), j.tolist()))
    assert table == {(0, 0), (1, 1), (2, 2), (3, 3), (5, 4)}  # (4, 3) is 28 away
    ki, kj, kc = match.pair_costs(pred, gt, i, j, 27)
    assert list(zip(ki.tolist(), kj.tolist())) == [(3, 3), (5, 4)] and np.all(kc < 0)
    r = fplobjdetect.obj_pr(pred, gt, 27, match='sparse')
    assert r.num_tp == fplobjdetect.obj_pr(pred, gt, 27).num_tp == 2


# ---- the matching ----------------------------------------------------------------------------

# Seeds 0 - 11 of each generator below were run on the CPU: on every one of them the sparse
# solver reproduces the dense solver's own num_tp (no tie between optima of different
# cardinality occurred), so all twelve are kept.
MATCH_SEEDS = list(range(12))


def _matching_case(seed):
    """clusters, so that components are large; every third seed has integer coordinates (equal
    costs, ties inside a component)"""
    rs = np.random.RandomState(100 + seed)
    if seed % 2:
        pred, gt = cases.clustered(seed, n_far=120)
    else:
        pred, gt, _ = cases.jittered(seed, 260, 240, box=160.0, sd=9.0)
    if seed % 3 == 0:
        pred, gt = np.rint(pred), np.rint(gt)
    lp, lg = (rs.randint(0, 2, len(pred)), rs.randint(0, 2, len(gt))) if seed % 4 == 1 else (None, None)
    return pred, gt, lp, lg


@pytest.mark.parametrize('seed', MATCH_SEEDS)
def test_match_sparse_reaches_the_dense_optimum(seed):
    pred, gt, lp, lg = _matching_case(seed)
    cost = _dense_cost(pred, gt, T, lp, lg)
    i, j = match.pairs_numpy(pred, gt, T)
    ki, kj, kc = match.pair_costs(pred, gt, i, j, T, lp, lg)
    low = np.minimum(cost, 0.0)
    for allow_mult in (False, True):
        want = fplobjdetect.obj_match(cost, allow_mult=allow_mult)
        got = match.match_sparse(len(pred), len(gt), ki, kj, kc, allow_mult)
        assert got.shape == want.shape and got.dtype == bool and got.format == 'csr'
        got = got.toarray()
        assert got.sum(axis=0).max() <= 1                       # a ground-truth point once
        assert np.all(cost[got] < 0)
        if allow_mult:
            assert np.array_equal(got, want)
            continue
        assert got.sum(axis=1).max() <= 1                       # a prediction once
        a, b = low[got].sum(), low[want].sum()
        assert abs(a - b) <= 1e-9 * abs(b) and b < 0
        assert got.sum() == want.sum() > 20
    # the table need not be filtered first: rows with cost >= 0 are ignored
    loose = match.match_sparse(len(pred), len(gt), i, j, cost[i, j], False).toarray()
    assert np.array_equal(loose, match.match_sparse(len(pred), len(gt), ki, kj, kc, False).toarray())


def test_match_sparse_of_an_empty_table():
    none = np.zeros(0, np.int32)
    for allow_mult in (False, True):
        m = match.match_sparse(4, 5, none, none, np.zeros(0), allow_mult)
        assert m.shape == (4, 5) and m.nnz == 0 and m.dtype == bool


# ---- the public calls --------------------------------------------------------------------------

def _same_numbers(a, b):
    for name in ('num_tp', 'tot_pred', 'tot_gt', 'pp', 'rr'):
        x, y = np.asarray(getattr(a, name)), np.asarray(getattr(b, name))
        assert x.shape == y.shape and np.array_equal(x, y), (name, x, y)


@pytest.fixture(scope='module')
def scored():
    """point sets with their labels and the default (dense) results, computed once"""
    out = {}
    for size in ((500, 549), (1500, 1621)):
        pred, gt, conf = cases.jittered(sum(size), *size)
        lp, lg = _labels(size[0], pred, gt)
        thds = np.array([0.3, 0.5, 0.7, 0.9]) if size[0] > 1000 else np.arange(0.0, 1.0, 0.125)
        dense = {}
        for labelled in (False, True):
            for allow_mult in (False, True):
                kw = dict(allow_mult=allow_mult)
                if labelled:
                    kw.update(predict_lbls=lp, groundtruth_lbls=lg)
                dense[labelled, allow_mult] = (
                    kw, fplobjdetect.obj_pr(pred, gt, T, **kw),
                    fplobjdetect.obj_pr_curve({'locs': pred, 'conf': conf}, {'locs': gt}, T, thds, **kw))
        out[size] = (pred, gt, conf, thds, dense)
    return out


@pytest.mark.parametrize('size', [(500, 549), (1500, 1621)])
def test_obj_pr_sparse_equals_the_default(scored, size):
    pred, gt, conf, thds, dense = scored[size]
    for (labelled, allow_mult), (kw, want, _) in dense.items():
        got = fplobjdetect.obj_pr(pred, gt, T, match='sparse', **kw)
        _same_numbers(got, want)
        assert np.array_equal(got.match.toarray(), want.match) or not allow_mult
        assert got.num_tp > 0.8 * min(size) * (0.3 if labelled else 1)
        if allow_mult:
            assert got.tot_pred >= len(pred)


@pytest.mark.parametrize('size', [(500, 549), (1500, 1621)])
def test_obj_pr_curve_sparse_is_one_table_and_equals_obj_pr_per_threshold(scored, size, monkeypatch):
    pred, gt, conf, thds, dense = scored[size]
    calls = []
    real = match.pairs_numpy
    monkeypatch.setattr(match, 'pairs_numpy', lambda *a: calls.append(len(a[0])) or real(*a))
    for (labelled, allow_mult), (kw, _, want) in dense.items():
        del calls[:]
        got = fplobjdetect.obj_pr_curve({'locs': pred, 'conf': conf}, {'locs': gt}, T, thds,
                                        match='sparse', **kw)
        assert calls == [int((conf >= thds.min()).sum())]          # one table, over the lowest
        _same_numbers(got, want)
        assert got.num_tp.shape == thds.shape and got.match.shape[1] == len(gt)
        for k, thd in enumerate(thds):
            sel = conf >= thd
            lkw = dict(kw)
            if labelled:
                lkw['predict_lbls'] = kw['predict_lbls'][sel]
            one = fplobjdetect.obj_pr(pred[sel], gt, T, match='sparse', **lkw)
            for name in ('num_tp', 'tot_pred', 'tot_gt', 'pp', 'rr'):
                assert getattr(got, name)[k] == getattr(one, name), (name, thd)
            if k == 0:
                assert (got.match != one.match).nnz == 0


def test_the_empty_branches_and_a_threshold_above_every_confidence():
    pred, gt, conf = cases.jittered(9, 60, 50)
    none = np.zeros((0, 3))
    for a, b in ((none, gt), (pred, none), (none, none)):
        want = fplobjdetect.obj_pr(a, b, T)
        got = fplobjdetect.obj_pr(a, b, T, match='sparse')
        assert got == want and got.match is None
    for thds in ([0.5, 2.0], [2.0], [3.0, 2.0, 0.1], []):
        for g in (gt, none):
            want = fplobjdetect.obj_pr_curve({'locs': pred, 'conf': conf}, {'locs': g}, T, thds)
            got = fplobjdetect.obj_pr_curve({'locs': pred, 'conf': conf}, {'locs': g}, T, thds,
                                            match='sparse')
            _same_numbers(got, want)
            assert (got.match is None) == (want.match is None)
    above = fplobjdetect.obj_pr_curve({'locs': pred, 'conf': conf}, {'locs': gt}, T, [2.0],
                                      match='sparse')
    assert above.num_tp[0] == 0 and above.tot_pred[0] == 0 and above.pp[0] == 1 and above.rr[0] == 0


def test_the_defaults_are_the_dense_path():
    pred, gt, conf = cases.jittered(9, 60, 50)
    r = fplobjdetect.obj_pr(pred, gt, T)
    assert isinstance(r.match, np.ndarray) and r.match.dtype == bool and r.match.shape == (60, 50)
    same = fplobjdetect.obj_pr(pred, gt, T, match='dense', device=None)
    assert isinstance(same.match, np.ndarray) and np.array_equal(same.match, r.match)
    c = fplobjdetect.obj_pr_curve({'locs': pred, 'conf': conf}, {'locs': gt}, T, [0.2, 0.6])
    assert isinstance(c.match, np.ndarray)
    with pytest.raises(ValueError, match="match 'hungarian': 'dense' .* or 'sparse'"):
        fplobjdetect.obj_pr(pred, gt, T, match='hungarian')
    with pytest.raises(ValueError, match="match None"):
        fplobjdetect.obj_pr_curve({'locs': pred, 'conf': conf}, {'locs': gt}, T, [0.5], match=None)
    assert fplobjdetect.MATCH_MODES == ('dense', 'sparse')
