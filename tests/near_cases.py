"""Seeded point sets of the neighbour-table tests (test_near_host.py, test_gpu_near.py).  The
sizes are derived from the binding's constants - the block of points and the scan's threads -
and the lattice from near.cell_side, so a later change of a constant moves the shapes with it."""
import numpy as np

from flypylib_amd import _nearcapi as capi, match, near

T = 30.0                       # rm_tbar_multi_pred's default neighbor_thresh
B, S = capi.BLOCK, capi.SCAN_THREADS
BALL = 4.0 / 3.0 * np.pi * T ** 3


def random_integer(n, neighbours=8.0):
    """n integer points in a box sized for about `neighbours` partners each"""
    rs = np.random.RandomState(n)
    box = max(2, int(round((n * BALL / neighbours) ** (1 / 3.0))))
    return rs.randint(0, box, (n, 3)).astype(np.float64)


def lattice(k=5):
    """a k^3 lattice whose spacing IS the cell side - every point on a cell face, none a
    partner of another (the spacing exceeds sqrt(T2)) - and one jittered companion per point
    within 10 voxels, so partners lie across the faces in every direction"""
    rs = np.random.RandomState(7)
    c = near.cell_side(T)
    g = np.arange(k) * c
    pts = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)
    return np.concatenate([pts, pts + rs.uniform(-10, 10, pts.shape)])[rs.permutation(2 * len(pts))]


def negative_fractional(n=700):
    rs = np.random.RandomState(11)
    return rs.rand(n, 3) * 260.0 * 1.37 - 500.3


def one_plane(n=400):
    """the grid is one cell thick in z"""
    rs = np.random.RandomState(12)
    pts = rs.rand(n, 3) * 200.0
    pts[:, 2] = 77.5
    return pts


def one_cell(n=100):
    """every point in one cell: every pair is a pair of the table"""
    rs = np.random.RandomState(13)
    return rs.rand(n, 3) * 10.0 + 3.25


def cluster(n=B + 44, far=60):
    """more points within radius 5 than a block has threads - one cell, rows of n - 1 entries,
    longer than any per-thread buffer could be - among far points with empty rows"""
    rs = np.random.RandomState(14)
    v = rs.randn(n, 3)
    v *= (5.0 * rs.rand(n, 1) ** (1 / 3.0)) / np.linalg.norm(v, axis=1, keepdims=True)
    g = np.arange(4) * 400.0
    lone = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)[:far]
    pts = np.concatenate([v + 777.0, lone])
    return pts[rs.permutation(len(pts))]


def no_pair(k=7):
    """a lattice of spacing 100: no pair at all"""
    g = np.arange(k) * 100.0
    pts = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)
    return pts[np.random.RandomState(15).permutation(len(pts))]


def thin(n=300):
    """spread so thinly that nearly every neighbour key range is empty; a few planted pairs"""
    rs = np.random.RandomState(16)
    pts = np.rint(rs.rand(n, 3) * 1e5)
    pts[n - 10:] = pts[:10] + rs.randint(-9, 10, (10, 3))
    return pts


def boundary():
    """pairs at exactly T: on one axis and as an 18-24-0 offset (s = 900 <= T2: in the table),
    beside pairs just inside and just outside"""
    assert T == 30.0
    a = np.array([[100, 100, 100], [400, 100, 100], [100, 400, 100], [400, 400, 400]], np.float64)
    return np.concatenate([a, a[:1] + [30, 0, 0], a[1:2] + [18, 24, 0], a[2:3] + [0, 0, 29],
                           a[3:4] + [0, 31, 0]])


SETS = {
    'one point': lambda: np.array([[5.0, 6.0, 7.0]]),
    'two coincident points': lambda: np.array([[5.0, 6.0, 7.0], [5.0, 6.0, 7.0]]),
    'two points at exactly T': lambda: np.array([[0.0, 0.0, 0.0], [0.0, T, 0.0]]),
    'boundary': boundary,
    'block tail: B - 1': lambda: random_integer(B - 1),
    'block tail: B': lambda: random_integer(B),
    'block tail: B + 1': lambda: random_integer(B + 1),
    'scan runs of 2, a short last run: S + 1': lambda: random_integer(S + 1),
    'scan runs of 3, a short last run: 2 S + 2': lambda: random_integer(2 * S + 2),
    'lattice on the cell faces': lattice,
    'negative and fractional': negative_fractional,
    'one z plane': one_plane,
    'one cell': one_cell,
    'cluster': cluster,
    'no pair': no_pair,
    'thin': thin,
}


def check_sets():
    """the reasons above, asserted against the binding's rule"""
    assert (S + 1) % S != 0 and -(-(S + 1) // S) == 2 and -(-(2 * S + 2) // S) == 3
    assert (2 * S + 2) % 3 != 0
    assert near.grid_of(one_plane(), T)[2][2] == 1
    assert near.grid_of(one_cell(), T)[2] == (1, 1, 1)
    assert len(cluster()) > B and max(len(f()) for f in SETS.values()) <= 5000


def self_join(locs, t):
    """the table by match.pairs_numpy: its self-join without the s == 0 rows, as CSR"""
    locs = np.ascontiguousarray(locs, np.float64)
    i, j = match.pairs_numpy(locs, locs, t)
    d = locs[i] - locs[j]
    s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    i, j = i[s > 0], j[s > 0]
    indptr = np.zeros(len(locs) + 1, np.int64)
    np.cumsum(np.bincount(i, minlength=len(locs)), out=indptr[1:])
    return indptr, j.astype(np.int32)


def planted(n, seed=31, spacing=70.0, share=0.08, jitter=10.0, period=512.0):
    """a T-bar list as full_roi_inference leaves it: a jittered lattice (integer coordinates plus
    a float offset) in which `share` of the points, those nearest the planes `period` apart,
    were detected a second time within `jitter` voxels; float32-valued confidences in
    [0.25, 1), held as float64 -> {'locs', 'conf'}"""
    rs = np.random.RandomState(seed)
    base = n - int(round(n * share))
    side = int(np.ceil(base ** (1 / 3.0)))
    g = np.arange(side) * spacing
    pts = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)
    pts = pts[rs.permutation(len(pts))[:base]] + rs.randint(-20, 21, (base, 3))
    to_plane = np.abs((pts[:, 2] + period / 2) % period - period / 2)
    twice = np.argsort(to_plane, kind='stable')[:n - base]
    pts = np.concatenate([pts, pts[twice] + rs.randint(-int(jitter), int(jitter) + 1, (n - base, 3))])
    pts = pts[rs.permutation(n)] + np.array([0.5, 0.25, 0.125])
    conf = (rs.rand(n) * 0.75 + 0.25).astype(np.float32).astype(np.float64)
    return {'locs': pts, 'conf': conf}


def planted_labels(tbars, slab=150.0):
    """segment ids: slabs across x, so some duplicates straddle two segments"""
    return (tbars['locs'][:, 0] // slab).astype(np.uint64)
