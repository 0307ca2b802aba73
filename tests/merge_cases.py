"""Inputs of the merge tests (test_merge_host.py, test_gpu_merge.py): every recorded case of
tests/golden/multi_pred.npz, the seeded random sets of test_dedupe_host.py's kind, a hand-made
case for every cause that sends a component to the host, and the realistic list of
tools/bench_configs.py --what dedupe.  A case is (tbars, keywords of rm_tbar_multi_pred)."""
import os

import numpy as np

from flypylib_amd import dedupe
from tests import near_cases

T = near_cases.T
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'multi_pred.npz')
GOLDEN_CASES = ('two_border_duplicates', 'chain_reaches_a_stranger', 'coincident_points',
                'different_labels', 'exactly_thresh', 'tied_confidences', 'visited_point_already_removed',
                'empty', 'one_point', 'random_200', 'random_200_int_locs_labels',
                'random_150_fractional_thresh_20')
# the caps at their defaults, and forced so low that nearly every component goes to the host and
# the closure runs several rounds
CAPS = {'default': {}, 'cand 2': {'cand_cap': 2}, 'comp 2': {'comp_cap': 2}, 'moves 1': {'max_moves': 1},
        'all 1': {'cand_cap': 1, 'comp_cap': 1, 'max_moves': 1}}


def _conf(rs, n):
    """float32-valued confidences in [0.25, 1), held as float64: sums of a few are exact"""
    return (rs.rand(n) * 0.75 + 0.25).astype(np.float32).astype(np.float64)


def golden(name):
    g = np.load(GOLDEN)
    kw = {'neighbor_thresh': g[name + '.thresh'].item()}
    if name + '.labels' in g.files:
        kw['labels'] = g[name + '.labels']
    return {'locs': g[name + '.locs'], 'conf': g[name + '.conf']}, kw


def random_set(n, labelled):
    """test_dedupe_host.py's random set: about 3 partners each"""
    rs = np.random.RandomState(n + labelled)
    box = int(round((n * near_cases.BALL / 3.0) ** (1 / 3.0)))
    tbars = {'locs': rs.randint(0, box, (n, 3)) + np.array([0.5, 0.25, 0.125]), 'conf': _conf(rs, n)}
    return tbars, ({'labels': rs.randint(0, 3, n)} if labelled else {})


def planted_set(n, labelled):
    tbars = near_cases.planted(n)
    return tbars, ({'labels': near_cases.planted_labels(tbars)} if labelled else {})


def realistic(n=3000, seed=5, spacing=34.0, jitter=2, near_plane=10.0, period=512.0, first=250.0):
    """tools/bench_configs.py's dedupe_points: a lattice of spacing 34 jittered by +-2; every
    point within 10 voxels of a z plane 512 apart was detected a second time within 6 voxels;
    shuffled -> (tbars, the number of points detected twice)"""
    rs = np.random.RandomState(seed)
    share = 2 * near_plane / period
    side = int(round((n / (1 + share)) ** (1 / 3.0)))
    g = np.arange(side) * spacing + 40.0
    pts = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)
    pts += rs.randint(-jitter, jitter + 1, pts.shape)
    to_plane = np.abs((pts[:, 2] - first + period / 2) % period - period / 2)
    twice = pts[to_plane <= near_plane]
    pts = np.concatenate([pts, twice + rs.randint(-6, 7, twice.shape)])
    pts = pts[rs.permutation(len(pts))]
    return {'locs': pts, 'conf': _conf(rs, len(pts))}, len(twice)


def _far(k):
    """k lone points far from everything and from each other"""
    return np.array([[1000.0 + 100 * i, 1000.0, 1000.0] for i in range(k)])


def _line(k, step=1.0):
    return np.stack([np.arange(k) * step, np.zeros(k), np.zeros(k)], axis=1)


def hand_made():
    """name -> (tbars, kw, the host_components the executor must report at the default caps, or
    None where the count is not the point)"""
    rs = np.random.RandomState(3)
    out = {}
    pair = np.array([[0.0, 0, 0], [10.0, 0, 0]])
    # the mean (5, 0, 0) is 29.9 from the third point, which is 30.3 from both of the pair
    out['a stranger in a ball'] = (
        {'locs': np.concatenate([pair, [[5.0, 29.9, 0]], _far(2)]), 'conf': np.array([0.5, 0.5, 0.75, 0.5, 0.5])},
        {}, 2)
    # ... two of them in one place: no partners of each other, candidates around the moved centre
    out['coincident strangers'] = (
        {'locs': np.concatenate([pair, [[5.0, 29.9, 0]] * 2, _far(1)]), 'conf': np.array([0.5, 0.5, 0.75, 0.25, 0.5])},
        {}, 3)
    # coincident points inside a component: partners of the others, not of each other
    out['coincident members'] = (
        {'locs': np.array([[0.0, 0, 0], [4.0, 0, 0], [4.0, 0, 0], [8.0, 2, 0]]), 'conf': np.array([0.5, 0.75, 0.25, 0.5])},
        {}, 0)
    cap = dedupe.CAND_CAP
    out['candidates at the cap'] = ({'locs': np.concatenate([_line(cap), _far(3)]), 'conf': _conf(rs, cap + 3)}, {}, 0)
    out['candidates over the cap'] = ({'locs': np.concatenate([_line(cap + 1), _far(3)]), 'conf': _conf(rs, cap + 4)}, {}, 1)
    cc = dedupe.COMP_CAP
    # a chain of spacing 20: neighbours 20 apart, the next 40 - candidate sets of 3, one component
    out['component at the cap'] = ({'locs': _line(cc, 20.0) + 0.5, 'conf': _conf(rs, cc)}, {}, None)
    out['component over the cap'] = ({'locs': _line(cc + 1, 20.0) + 0.5, 'conf': _conf(rs, cc + 1)}, {}, None)
    out['ties inside a component'] = (
        {'locs': np.array([[0.0, 0, 0], [7.0, 0, 0], [3.0, 9, 0], [200.0, 0, 0], [204.0, 3, 0]]),
         'conf': np.array([0.5, 0.5, 0.5, 0.75, 0.75])}, {}, 0)
    pts = near_cases.cluster()                               # 300 points within radius 5, 60 far ones
    out['a cluster of 300'] = ({'locs': pts, 'conf': _conf(rs, len(pts))}, {}, 1)
    out['neighbours of other labels only'] = (
        {'locs': np.array([[0.0, 0, 0], [5.0, 0, 0], [100.0, 0, 0], [104.0, 0, 0], [108.0, 0, 0]]),
         'conf': np.array([0.5, 0.75, 0.5, 0.75, 0.25])}, {'labels': np.array([1, 2, 7, 8, 7])}, 0)
    out['N = 0'] = ({'locs': np.zeros((0, 3)), 'conf': np.zeros(0)}, {}, 0)
    out['N = 1'] = ({'locs': np.array([[5.0, 6, 7]]), 'conf': np.array([0.5])}, {}, 0)
    out['N = 2'] = ({'locs': np.array([[5.0, 6, 7], [9.0, 6, 7]]), 'conf': np.array([0.5, 0.75])}, {}, 0)
    out['N = 2, apart'] = ({'locs': np.array([[5.0, 6, 7], [90.0, 6, 7]]), 'conf': np.array([0.5, 0.75])}, {}, 0)
    return out


def all_cases():
    """name -> (tbars, kw): everything both executors are compared on"""
    out = {'golden: ' + c: golden(c) for c in GOLDEN_CASES}
    for n in (500, 3000):
        for labelled in (False, True):
            tag = '%d%s' % (n, ', labelled' if labelled else '')
            out['random ' + tag] = random_set(n, labelled)
            out['planted ' + tag] = planted_set(n, labelled)
    out.update({'hand-made: ' + k: v[:2] for k, v in hand_made().items()})
    out['realistic'] = (realistic()[0], {})
    return out


def pairs_lattice(k):
    """k components of two points each, on a lattice of spacing 100 -> tbars"""
    rs = np.random.RandomState(k)
    side = int(np.ceil(k ** (1 / 3.0)))
    g = np.arange(side) * 100.0
    a = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)[:k]
    pts = np.concatenate([a, a + rs.randint(1, 7, (k, 3))])
    pts = pts[rs.permutation(2 * k)]
    return {'locs': pts, 'conf': _conf(rs, 2 * k)}


def split(case):
    tbars, kw = case
    ll = kw.get('labels')
    ll = np.zeros(len(tbars['conf'])) if ll is None else np.asarray(ll).reshape(-1)
    return tbars['locs'], tbars['conf'], ll, kw.get('neighbor_thresh', 30)
