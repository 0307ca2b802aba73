"""Inputs of the device-solver tests (test_assign_host.py, test_gpu_assign.py): pair graphs for
the labelling stage, hand-placed components for the solver - each far from every other, at
the pipeline's threshold T = 27 - and the brute-force check that a case has ONE optimum, so
that two correct solvers must return the same matching."""
import os

import functools

import numpy as np

from flypylib_amd import match
from flypylib_amd._assigncapi import BLOCK, MAX_BLOCKS, SCAN_THREADS
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


def second_best_gap(i, j, cost):
    """second best total minus best total over all matchings of ONE component's pairs (all of
    cost < 0), without enumeration.  Any matching other than the optimum lacks at least one pair
    of the optimum - a strict superset would be cheaper still, every pair costing less than 0 -
    so the second best is the least of the optima of the problems with one matched pair made
    absent (cost 0).  One linear_sum_assignment per matched pair."""
    from scipy.optimize import linear_sum_assignment
    rows, ri = np.unique(i, return_inverse=True)
    cols, ci = np.unique(j, return_inverse=True)
    block = np.zeros((len(rows), len(cols)))
    block[ri, ci] = cost
    assert (block[ri, ci] < 0).all()
    br, bc = linear_sum_assignment(block)
    optimum = block[br, bc].sum()
    gap = np.inf
    for r, c in zip(br, bc):
        if block[r, c] < 0:
            kept, block[r, c] = block[r, c], 0.0
            sr, sc = linear_sum_assignment(block)
            gap = min(gap, block[sr, sc].sum() - optimum)
            block[r, c] = kept
    return gap


MIN_GAP = 1e-6      # of a case compared matrix for matrix; the solver's float64 potentials gather
                    # about 64 roundings of magnitude 27 x 2^-52, about 4e-13


def component_gaps(n_pred, i, j, cost):
    """[(label, distinct rows, distinct columns, pairs, second_best_gap)] of every component, in
    label order - the order the device solver meets them in; the gap of a single pair is its
    own cost's magnitude"""
    i, j, cost = np.asarray(i), np.asarray(j), np.asarray(cost)
    label = match.components_numpy(n_pred, i, j)
    out = []
    for k in np.unique(label):
        e = label == k
        out.append((int(k), len(np.unique(i[e])), len(np.unique(j[e])), int(e.sum()),
                    second_best_gap(i[e], j[e], cost[e])))
    return out


# ---- the ordered compaction ----------------------------------------------------------------------
# List lengths chosen against the constants of csrc/assign/assign.hip: a block of count_kernel
# and fill_kernel is one cell of BLOCK entries, scan_kernel's thread t owns the `per` cells from
# t * per.  tests/test_assign_host.py asserts, without a GPU, that each length is what it says.

def compaction_layout(n):
    """what the three kernels make of a list of n entries"""
    cells = -(-n // BLOCK)
    per = -(-cells // SCAN_THREADS)
    last_thread = (cells - 1) // per
    return dict(entries=n, cells=cells, per=per, last_thread=last_thread,
                last_run=cells - last_thread * per, last_cell=n - (cells - 1) * BLOCK)


COMPACTION_SHAPES = {
    'one': 1, 'wave-1': 63, 'wave': 64, 'wave+1': 65,
    'cell-1': BLOCK - 1, 'cell': BLOCK, 'cell+1': BLOCK + 1,
    'scan_full': BLOCK * SCAN_THREADS,
    'scan_one_over': BLOCK * SCAN_THREADS + 1,
    'scan_runs_3': BLOCK * (2 * SCAN_THREADS) + BLOCK + 3,
}
FLAG_PATTERNS = ('none', 'all', 'first', 'last', 'half', 'every 257th', 'any non-zero')
INT32_MIN = np.iinfo(np.int32).min


def flag_pattern(name, n):
    rs = np.random.RandomState(n % 9973 + 17 * FLAG_PATTERNS.index(name))
    flags = np.zeros(n, np.int32)
    if name == 'all':
        flags[:] = 1
    elif name == 'first':
        flags[0] = 1
    elif name == 'last':
        flags[-1] = 1
    elif name == 'half':
        flags[:] = rs.rand(n) < 0.5
        flags[-1] = 1                             # the last cell, and scan run, is never empty
    elif name == 'every 257th':                   # drifts through the cells, one or none a cell
        flags[::257] = 1
    elif name == 'any non-zero':
        flags[:] = rs.choice(np.array([0, 0, 0, -1, 2, INT32_MIN, 1, 7], np.int32), n)
        flags[0], flags[n // 2], flags[-1] = -1, 2, INT32_MIN      # (n == 1: the last one holds)
    return flags


@functools.lru_cache(maxsize=None)
def compaction_columns(n):
    """(a, b, c): int32, int32 and float64 columns of n entries; c holds NaN of two payloads,
    -0.0 and infinities, at the list's ends and throughout"""
    rs = np.random.RandomState(n % 9973)
    a = rs.randint(INT32_MIN, 2 ** 31 - 1, n).astype(np.int32)
    b = np.arange(n, dtype=np.int32)[::-1] - 5
    c = rs.randn(n)
    special = np.array([np.nan, -0.0, np.inf, -np.inf, 0.0, 5e-324])
    where = rs.rand(n) < 0.25
    c[where] = rs.choice(special, int(where.sum()))
    c[0], c[-1] = np.nan, -0.0
    other_nan = np.array([0xfff8000000000123], np.uint64).view(np.float64)[0]
    c[n // 2:n // 2 + 1][np.isnan(c[n // 2:n // 2 + 1])] = other_nan
    c[n // 3] = other_nan
    for v in (a, b, c):
        v.setflags(write=False)
    return a, b, c


def compaction_reference(flags):
    """(idx, rank): the flagged entries in order, every entry's rank among them or -1"""
    idx = np.flatnonzero(flags)
    rank = np.full(len(flags), -1, np.int32)
    rank[idx] = np.arange(len(idx), dtype=np.int32)
    return idx.astype(np.int32), rank


# ---- beyond one grid stride ------------------------------------------------------------------------

STRIDE = BLOCK * MAX_BLOCKS                     # entries one pass of a grid-stride kernel covers
STRIDE_SIZES = (STRIDE + 1, 3 * (STRIDE + 1))
THRESHOLDS = (0.5, float('nan'), float('inf'), float('-inf'))


def conf_case(n, thd):
    """confidences around `thd`: uniform(0, 1) with NaN, both infinities, thd itself and its two
    float64 neighbours sprinkled throughout and placed at both ends and on both sides of every
    multiple of STRIDE"""
    rs = np.random.RandomState(n % 9973)
    with np.errstate(invalid='ignore'):
        special = np.array([np.nan, np.inf, -np.inf, thd, np.nextafter(thd, -np.inf),
                            np.nextafter(thd, np.inf), -0.0, 1.7976931348623157e308])
    conf = rs.rand(n)
    where = rs.rand(n) < 0.3
    conf[where] = rs.choice(special, int(where.sum()))
    edges = [0, n - len(special)] + [k for k in range(STRIDE - 4, n - len(special), STRIDE)]
    for e in edges:
        conf[e:e + len(special)] = special
    return conf


KEY_PATTERNS = ('runs', 'all equal', 'all distinct')


def key_case(name, n):
    """sorted int32 keys: random runs of 1 to 500 entries with a run of one entry at each end and
    a run across every multiple of STRIDE; one run; n runs"""
    if name == 'all equal':
        return np.full(n, 7, np.int32)
    if name == 'all distinct':
        return np.arange(n, dtype=np.int32) - 3
    rs = np.random.RandomState(n % 9973)
    first = np.zeros(n, bool)
    at = np.cumsum(rs.randint(1, 501, n // 100))
    first[at[at < n]] = True
    for k in range(STRIDE, n, STRIDE):
        first[k - 2:k + 3] = False
    first[[1, n - 1]] = True
    first[n - 2] = False
    return (np.cumsum(first) * 3 - 1).astype(np.int32)


def cube_points(seed, n_pred, n_gt, side, integer):
    """points uniform in a cube of `side` voxels at C0, integer or fractional"""
    rs = np.random.RandomState(seed)
    pred, gt = rs.rand(n_pred, 3) * side + C0, rs.rand(n_gt, 3) * side + C0
    return (np.rint(pred), np.rint(gt)) if integer else (pred, gt)


# name -> (side, integer): 300 x 300 points, the whole cross product as the table.  'full':
# the cube's diagonal is below T, every row is admissible.  'half': about half of them are.
COST_CUBES = {'full': (15.0, False), 'full integer': (15.0, True), 'half': (41.0, False),
              'half integer': (41.0, True)}
COST_POINTS = 300


def cost_table(name):
    """(pred, gt, i, j): the points of a COST_CUBES case and every pair of them in (i, j) order"""
    side, integer = COST_CUBES[name]
    pred, gt = cube_points(11 + len(name), COST_POINTS, COST_POINTS, side, integer)
    i, j = np.divmod(np.arange(COST_POINTS * COST_POINTS, dtype=np.int32), np.int32(COST_POINTS))
    return pred, gt, i.astype(np.int32), j.astype(np.int32)


# ---- long graphs -----------------------------------------------------------------------------------

def long_chain(k=200, permuted=False):
    """chain_pairs(k) with the predictions renumbered so that index 0 sits in the middle of the
    chain and the indices rise towards both ends - every label has half the chain to travel -
    in (i, j) order, or with the rows in random order"""
    i, j = chain_pairs(k)
    i = ((i.astype(np.int64) - k // 2) % k).astype(np.int32)
    order = np.random.RandomState(k).permutation(len(i)) if permuted else np.lexsort((j, i))
    return i[order], j[order]


# ---- mid-size sparse components ----------------------------------------------------------------------

def rod(seed, n_pred, n_gt, length, integer=False):
    """(pred, gt) uniform in a length x 8 x 8 rod at 1000: at T = 27 a point pairs with those up
    to about 27 voxels along the rod, so the component is sparse - many pairs are absent - and
    its rows and columns come into sight a few per 64 pairs of the table"""
    rs = np.random.RandomState(seed)
    pred = rs.rand(n_pred, 3) * [length, 8, 8] + 1000
    gt = rs.rand(n_gt, 3) * [length, 8, 8] + 1000
    return (np.rint(pred), np.rint(gt)) if integer else (pred, gt)


# (n_pred, n_gt, length, seeds): one component each, one optimum each (test_assign_host.py)
RODS = [(20, 17, 90, (0, 1, 2)), (17, 20, 90, (0, 1, 2)), (40, 33, 160, (0, 1, 2)),
        (33, 40, 160, (0, 1, 2)), (64, 64, 300, (0, 1, 2)), (64, 40, 250, (0, 1, 2)),
        (9, 64, 120, (0, 1, 2)), (64, 9, 120, (0, 1))]
ROD_CASES = [(seed, n, m, length) for n, m, length, seeds in RODS for seed in seeds]
TIED_RODS = [(0, 40, 33, 160), (0, 64, 64, 300)]              # integer coordinates: equal costs
# rods beyond the cap on one side, below CAP * CAP pairs: (seed, n_pred, n_gt, length)
OVER_THE_CAP_RODS = {'65x20 rod': (0, 65, 20, 200), '20x65 rod': (0, 20, 65, 200)}
OVER_BY_PAIRS = '65x64'                                        # a full block of 4160 pairs

ROD_SCENE = (('rod', 0, 64, 64, 300), '2x1', ('rod', 0, 9, 64, 120), '3x3 greedy',
             ('rod', 0, 64, 9, 120), ('rod', 0, 17, 20, 90), '1x1')


def scene_of(parts, seed=SOLVE_SEED, shuffle=True):
    """components - names of component() or ('rod', seed, n_pred, n_gt, length) - 500 voxels
    apart along y, in this order; the points shuffled as scene() shuffles them, or left in
    order, so that the components' labels rise in the order given"""
    rs = np.random.RandomState(seed)
    built = []
    for k, part in enumerate(parts):
        off = np.array([0.0, 500.0 * k, 0.0])
        if isinstance(part, str):
            built.append(component(part, seed, C0 + off))
        else:
            pred, gt = rod(*part[1:])
            built.append((pred + off, gt + off))
    pred, gt = np.concatenate([p for p, _ in built]), np.concatenate([g for _, g in built])
    if shuffle:
        pred, gt = pred[rs.permutation(len(pred))], gt[rs.permutation(len(gt))]
    return pred, gt
