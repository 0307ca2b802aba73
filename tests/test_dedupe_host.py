"""fplsynapses.rm_tbar_multi_pred on the host: method='dense' against the reference's recorded
results (tests/golden/multi_pred.npz, made by tests/golden/make_multi_pred_golden.py),
method='sparse' against method='dense', merge_multi_pred, the argument checks and the merge
step full_roi_inference runs."""
import numpy as np
import pytest

from flypylib_amd import fplpipeline, fplsynapses, near
from tests import near_cases as cases

OUTPUTS = ('rm_idx', 'mv_idx', 'mv_loc')
CASES = ('two_border_duplicates', 'chain_reaches_a_stranger', 'coincident_points',
         'different_labels', 'exactly_thresh', 'tied_confidences', 'visited_point_already_removed',
         'empty', 'one_point', 'random_200', 'random_200_int_locs_labels',
         'random_150_fractional_thresh_20')


@pytest.fixture(scope='module')
def recorded(golden):
    return golden('multi_pred.npz')


def _case(g, name):
    tbars = {'locs': g[name + '.locs'], 'conf': g[name + '.conf']}
    kw = {'neighbor_thresh': g[name + '.thresh'].item()}
    if name + '.labels' in g.files:
        kw['labels'] = g[name + '.labels']
    return tbars, kw


def _same(got, want):
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def test_the_golden_file_holds_the_listed_cases(recorded):
    assert {k.split('.')[0] for k in recorded.files} == set(CASES)
    assert max(len(recorded[c + '.conf']) for c in CASES) == 200
    assert recorded['random_200.mv_loc'].dtype == np.dtype('int')


@pytest.mark.parametrize('method', ['dense', 'sparse'])
@pytest.mark.parametrize('name', CASES)
def test_both_methods_give_the_reference_results(recorded, name, method):
    tbars, kw = _case(recorded, name)
    got = fplsynapses.rm_tbar_multi_pred(tbars, method=method, **kw)
    assert got[0].dtype == got[1].dtype == np.bool_ and got[2].dtype == np.dtype('int')
    _same(got, [recorded['%s.%s' % (name, k)] for k in OUTPUTS])


def test_what_the_cases_are_there_for(recorded):
    """each recorded result shows the quirk its case was built for"""
    out = {c: [recorded['%s.%s' % (c, k)] for k in OUTPUTS] for c in CASES}
    rm, mv, loc = out['two_border_duplicates']
    assert rm.tolist() == [False, True, False, False, False] and mv.tolist() == [True] + [False] * 4
    assert loc[0].tolist() == [101, 100, 512]
    rm, mv, loc = out['chain_reaches_a_stranger']          # 2 is a neighbour of neither 0 nor 1
    assert rm.tolist() == [False, True, True, False] and loc[0].tolist()[:1] == [214]
    rm, mv, _ = out['coincident_points']
    assert rm[3:].tolist() == [False, False] and mv[3:].tolist() == [False, False]   # no neighbours
    assert rm[:3].sum() == 2                               # ... but removed around a moved centre
    rm, mv, _ = out['different_labels']
    assert rm.tolist() == [False, False, True, False, False] and mv.sum() == 1
    rm, mv, _ = out['exactly_thresh']                      # 30 and 18-24-0 are NOT below 30; 29 is
    assert rm.tolist() == [False] * 5 + [True] and mv.tolist() == [False] * 4 + [True, False]
    rm, mv, _ = out['visited_point_already_removed']
    assert rm.tolist() == [True, False, True, False, True] and mv.tolist() == [False, True, False, True, False]
    assert all(len(out[c][0]) == n and out[c][2].shape == (n, 3) for c, n in (('empty', 0), ('one_point', 1)))


@pytest.mark.parametrize('n', [500, 3000])
@pytest.mark.parametrize('labelled', [False, True])
def test_sparse_equals_dense_on_random_sets(n, labelled):
    """integer coordinates plus a float offset; float32-valued confidences in [0.25, 1): the
    sum of a candidate set's confidences is exact in float64 (24-bit values spanning 2 binades,
    far fewer than 2^27 of them), so the two methods divide by the same number"""
    rs = np.random.RandomState(n + labelled)
    box = int(round((n * cases.BALL / 3.0) ** (1 / 3.0)))           # about 3 partners each
    tbars = {'locs': rs.randint(0, box, (n, 3)) + np.array([0.5, 0.25, 0.125]),
             'conf': (rs.rand(n) * 0.75 + 0.25).astype(np.float32).astype(np.float64)}
    kw = {'labels': rs.randint(0, 3, n)} if labelled else {}
    dense = fplsynapses.rm_tbar_multi_pred(tbars, method='dense', **kw)
    _same(fplsynapses.rm_tbar_multi_pred(tbars, method='sparse', **kw), dense)
    assert dense[1].sum() > n // 10 and dense[0].sum() > n // 5
    planted = cases.planted(n)
    kw = {'labels': cases.planted_labels(planted)} if labelled else {}
    dense = fplsynapses.rm_tbar_multi_pred(planted, method='dense', **kw)
    _same(fplsynapses.rm_tbar_multi_pred(planted, method='sparse', **kw), dense)
    assert n // 20 < dense[1].sum() <= dense[0].sum() + 1


def test_sparse_asks_the_grid_not_the_table_around_a_moved_centre(recorded, monkeypatch):
    asked = []
    real = near.CellGrid.ball
    monkeypatch.setattr(near.CellGrid, 'ball', lambda self, c: asked.append(tuple(c)) or real(self, c))
    tbars, kw = _case(recorded, 'chain_reaches_a_stranger')
    rm, _, _ = fplsynapses.rm_tbar_multi_pred(tbars, method='sparse', **kw)
    assert rm[2] and asked[0] == (214, 200, 200)


def test_labels_and_argument_errors():
    tb = cases.planted(50)
    with pytest.raises(ValueError, match='DVID is out of scope.*labels='):
        fplsynapses.rm_tbar_multi_pred(tb, None, 'segmentation')
    with pytest.raises(ValueError, match='labels holds 3 entries for 50 points'):
        fplsynapses.rm_tbar_multi_pred(tb, labels=[1, 2, 3])
    with pytest.raises(ValueError, match="method 'kdtree'"):
        fplsynapses.rm_tbar_multi_pred(tb, method='kdtree')
    with pytest.raises(ValueError, match="device=0 needs method='sparse'"):
        fplsynapses.rm_tbar_multi_pred(tb, device=0)
    with pytest.raises(ValueError, match="needs method='sparse'"):
        fplsynapses.rm_tbar_multi_pred(tb, method='dense', device=True)
    # labels given: segm_name is not consulted; a falsy segm_name: all labels equal
    ll = cases.planted_labels(tb, slab=60.0)
    _same(fplsynapses.rm_tbar_multi_pred(tb, None, 'segmentation', labels=ll),
          fplsynapses.rm_tbar_multi_pred(tb, labels=ll))
    _same(fplsynapses.rm_tbar_multi_pred(tb, None, '', 30), fplsynapses.rm_tbar_multi_pred(tb, labels=np.ones(50)))


def test_merge_multi_pred():
    tb = {'locs': np.array([[1.5, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]]),
          'conf': np.array([0.5, 0.25, 0.75, 1.0], np.float32)}
    rm = np.array([False, True, False, False])
    mv = np.array([False, False, True, False])
    loc = np.array([[0, 0, 0], [0, 0, 0], [6, 7, 8], [99, 99, 99]])
    out = fplsynapses.merge_multi_pred(tb, rm, mv, loc)
    assert sorted(out) == ['conf', 'locs']
    assert out['locs'].tolist() == [[1.5, 2, 3], [6, 7, 8], [10, 11, 12]] and out['locs'].dtype == np.float64
    assert out['conf'].tolist() == [0.5, 0.75, 1.0] and out['conf'].dtype == np.float32
    assert tb['locs'][2].tolist() == [7, 8, 9]                       # the input is left alone
    ints = fplsynapses.merge_multi_pred({'locs': tb['locs'].astype(np.int32), 'conf': tb['conf']}, rm, mv, loc)
    assert ints['locs'].dtype == np.int32 and ints['locs'][1].tolist() == [6, 7, 8]
    none = fplsynapses.merge_multi_pred({'locs': np.zeros((0, 3)), 'conf': np.zeros(0)},
                                        np.zeros(0, bool), np.zeros(0, bool), np.zeros((0, 3), int))
    assert none['locs'].shape == (0, 3) and none['conf'].shape == (0,)
    # end to end: the planted duplicates are gone, every survivor keeps its confidence
    planted = cases.planted(600)
    merged = fplsynapses.merge_multi_pred(planted, *fplsynapses.rm_tbar_multi_pred(planted, method='sparse'))
    assert 600 - 60 <= len(merged['conf']) <= 600 - 40
    assert len(near.pairs_numpy(merged['locs'], 12)[1]) == 0


def test_the_merge_step_of_the_pipeline():
    """what full_roi_inference(neighbor_thresh=...) runs on the list it wrote to all.p (the
    pipeline itself needs a GPU: tests/test_gpu_near.py)"""
    planted = cases.planted(600)
    want = fplsynapses.merge_multi_pred(planted, *fplsynapses.rm_tbar_multi_pred(planted, method='dense'))
    for method in ('dense', 'sparse'):
        got = fplpipeline.merge_border_duplicates(planted, 30, method=method)
        assert np.array_equal(got['locs'], want['locs']) and np.array_equal(got['conf'], want['conf'])
    # a segmentation (Z, Y, X): labels at the rounded (x, y, z), clipped into the volume
    seg = np.zeros((40, 50, 60), np.uint64)
    seg[:, :, 30:] = 5
    tb = {'locs': np.array([[28.4, 10, 10], [31.6, 12, 10], [31.5, 14, 11], [70.0, 49, 39], [10, 10, 10.4]]),
          'conf': np.array([0.5, 0.75, 0.625, 0.5, 0.25])}
    got = fplpipeline.merge_border_duplicates(tb, 30, fplpipeline._ArraySource(seg), 'sparse')
    labels = np.array([0, 5, 5, 5, 0])                              # 31.5 rounds to 32; 70 is clipped to 59
    want = fplsynapses.merge_multi_pred(tb, *fplsynapses.rm_tbar_multi_pred(tb, labels=labels))
    assert np.array_equal(got['locs'], want['locs']) and len(got['conf']) == 3
    empty = fplpipeline.merge_border_duplicates({'locs': np.zeros((0, 3)), 'conf': np.zeros(0)}, 30,
                                                fplpipeline._ArraySource(seg))
    assert empty['locs'].shape == (0, 3)
    import inspect
    sig = inspect.signature(fplpipeline.full_roi_inference).parameters
    assert [sig[k].default for k in ('neighbor_thresh', 'merge_method', 'merge_device')] == [None, 'sparse', None]
