"""Inputs of the device-solver tests (test_assign_host.py, test_gpu_assign.py): pair graphs for
the labelling stage, hand-placed components for the solver - each far from every other, at
the pipeline's threshold T = 27 - and the brute-force check that a case has ONE optimum, so
that two correct solvers must return the same matching."""
import os

import numpy as np

from flypylib_amd import match
from tests import match_cases as cases

T = cases.T
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'match_sparse_parent.npz')
GOLDEN_SEEDS = (0, 1, 2)
SOLVE_SEED = 7                  # of the hand-placed components; test_assign_host.py checks it
CURVE_SEED = 31                 # of the public-path case jittered(seed, 300, 280)
CURVE_THRESHOLDS = np.array([0.1, 0.3, 0.5, 0.7, 0.9])
C0 = np.array([1000.0, 1000.0, 1000.0])


def golden_case(seed):
    """the input whose match_sparse result, computed by the commit before solve_component was
    factored out, tests/golden/match_sparse_parent.npz holds: (n_pred, n_gt, i, j, cost)"""
    pred, gt, _ = cases.jittered(seed, 260, 240, box=160.0, sd=9.0)
    i, j = match.pairs_numpy(pred, gt, T)
    return (len(pred), len(gt)) + match.pair_costs(pred, gt, i, j, T)


# ---- pair graphs -------------------------------------------------------------------------------

def chain_pairs(k=8):
    """p0-g0-p1-g1-...-p(k-1)-g(k-1): 2k - 1 pairs in (i, j) order, one component, 2k - 1 across"""
    i = np.repeat(np.arange(k), 2)[1:]
    j = np.repeat(np.arange(k), 2)[:-1]
    return i.astype(np.int32), j.astype(np.int32)


def scipy_labels(n_pred, n_gt, i, j):
    """scipy's component number of every pair"""
    from scipy import sparse
    from scipy.sparse.csgraph import connected_components
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    nodes = n_pred + n_gt
    graph = sparse.csr_matrix((np.ones(len(i), bool), (i, j + n_pred)), shape=(nodes, nodes))
    return connected_components(graph, directed=False)[1][i]


def same_partition(a, b):
    """two labellings of the same pairs put the same pairs together"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    pairs = np.unique(np.stack([a, b], axis=1), axis=0) if len(a) else np.zeros((0, 2))
    return len(pairs) == len(np.unique(a)) == len(np.unique(b))


def graph_cases():
    """name -> (n_pred, n_gt, i, j) for the labelling stage"""
    out = {'empty': (4, 5, np.zeros(0, np.int32), np.zeros(0, np.int32)),
           'single pair': (3, 4, np.array([2], np.int32), np.array([1], np.int32)),
           'chain': (8, 8) + chain_pairs(8)}
    pred, gt = cases.crowd(24, 12, 12)
    out['crowd 12 x 12'] = (12, 12) + match.pairs_numpy(pred, gt, T)
    pred, gt = cases.apart(4, 30, 40)
    out['apart'] = (30, 40) + match.pairs_numpy(pred, gt, T)
    pred, gt, _ = cases.jittered(3, 37, 29)
    out['jittered'] = (37, 29) + match.pairs_numpy(pred, gt, T)
    return out


# ---- hand-placed components ----------------------------------------------------------------------

def _cube(rs, n, side, centre):
    return (rs.rand(n, 3) - 0.5) * side + centre


def component(name, seed=SOLVE_SEED, centre=C0):
    """(pred, gt) of ONE component.  '<rows>x<cols>' names are full blocks: every point lies in
    a cube whose diagonal is below T."""
    rs = np.random.RandomState(seed * 1000 + sum(map(ord, name)))
    jit = lambda n: rs.rand(n, 3) * 0.5                                   # noqa: E731
    x = lambda v: np.stack([np.asarray(v, float), np.zeros(len(v)), np.zeros(len(v))], axis=1)  # noqa: E731
    if name == '1x1':
        pred, gt = x([5]), x([0])
    elif name == '2x1':
        pred, gt = x([5, -8]) + jit(2), x([0])
    elif name == '1x2':
        pred, gt = x([0]), x([5, -8]) + jit(2)
    elif name == '3x3 greedy':
        # nearest first takes (p1, g0) and (p2, g1) and leaves p0 without a partner
        pred, gt = x([0, 12, 30]) + jit(3) * [0, 1, 1], x([10, 24, 40]) + jit(3) * [0, 1, 1]
    elif name == 'chain':
        pred, gt = x(40.0 * np.arange(8)) + jit(8), x(40.0 * np.arange(8) + 18) + jit(8)
    elif name == 'tie':
        pred, gt = x([5, -5]), x([0])                   # two predictions equally far from one point
    else:
        rows, cols = (int(v) for v in name.split('x'))
        side = 11.0 if max(rows, cols) <= 8 else 14.0
        pred, gt = _cube(rs, rows, side, 0.0), _cube(rs, cols, side, 0.0)
    return pred + centre, gt + centre


UNIQUE = ('1x1', '2x1', '1x2', '2x2', '3x3 greedy', 'chain', '8x8')    # compared matrix for matrix
AT_THE_CAP = ('64x64', '64x1', '1x64')                                  # compared by cost
OVER_THE_CAP = ('65x3', '3x65')


def scene(names, seed=SOLVE_SEED):
    """the named components side by side, 500 voxels apart, their points shuffled"""
    rs = np.random.RandomState(seed)
    parts = [component(n, seed, C0 + [500.0 * k, 0, 0]) for k, n in enumerate(names)]
    pred, gt = np.concatenate([p for p, _ in parts]), np.concatenate([g for _, g in parts])
    return pred[rs.permutation(len(pred))], gt[rs.permutation(len(gt))]


def labelled_case():
    """jittered(3, 37, 29) with random labels of two kinds: (pred, gt, pred labels, gt labels)"""
    rs = np.random.RandomState(2)
    pred, gt, _ = cases.jittered(3, 37, 29)
    return pred, gt, rs.randint(0, 2, 37), rs.randint(0, 2, 29)


def many_components(n, extra):
    """n components on a lattice 100 voxels wide - prediction k lies 5 voxels from point k - and
    the LAST `extra` of them have a second prediction 8 voxels away on the other side, numbered
    from n: components of two pairs whose label is still the lattice site's.  The optimum is
    k <-> k for every k < n.  -> (pred, gt, n, extra)"""
    side = int(np.ceil(n ** (1 / 3.0)))
    k = np.arange(n)
    gt = np.stack([k % side, k // side % side, k // (side * side)], axis=1) * 100.0
    pred = np.concatenate([gt + [5.0, 0, 0], gt[n - extra:] - [8.0, 0, 0]])
    return pred, gt, n, extra


def admissible(pred, gt, t=T, lp=None, lg=None):
    i, j = match.pairs_numpy(pred, gt, t)
    return match.pair_costs(pred, gt, i, j, t, lp, lg)


def greedy_cost(i, j, cost):
    """total cost of the nearest-first matching"""
    total, rows, cols = 0.0, set(), set()
    for e in np.argsort(cost, kind='stable'):
        if i[e] not in rows and j[e] not in cols:
            rows.add(i[e]); cols.add(j[e])
            total += cost[e]
    return total


# ---- one optimum ---------------------------------------------------------------------------------

def best_two(i, j, cost):
    """the two lowest total costs over ALL matchings of one component's pairs (every subset of
    the pairs that uses no row and no column twice, the empty one included), by enumeration
    with a bound: a branch is left when even the rows' best pairs cannot bring it below the
    second best so far"""
    rows, ri = np.unique(i, return_inverse=True)
    cols, ci = np.unique(j, return_inverse=True)
    adj = [[] for _ in rows]
    for r, c, w in zip(ri, ci, cost):
        adj[r].append((int(c), float(w)))
    rest = np.r_[np.cumsum([min(w for _, w in a) for a in adj][::-1])[::-1], 0.0]
    best = [np.inf, np.inf]

    def go(r, used, total):
        if total + rest[r] >= best[1]:
            return
        if r == len(adj):
            best[:] = sorted(best + [total])[:2]
            return
        for c, w in adj[r]:
            if not used >> c & 1:
                go(r + 1, used | 1 << c, total + w)
        go(r + 1, used, total)
    go(0, 0, 0.0)
    return best


def assert_unique_optimum(n_pred, i, j, cost, gap=1e-9, limit=8):
    """every component of at most limit x limit points has its best total cost more than `gap`
    below its second best; -> (components checked, components too large to enumerate)"""
    i, j, cost = np.asarray(i), np.asarray(j), np.asarray(cost)
    label = match.components_numpy(n_pred, i, j)
    checked = skipped = 0
    for k in np.unique(label):
        e = label == k
        if len(np.unique(i[e])) > limit or len(np.unique(j[e])) > limit:
            skipped += 1
            continue
        first, second = best_two(i[e], j[e], cost[e])
        assert second - first > gap, (k, first, second)
        checked += 1
    return checked, skipped
