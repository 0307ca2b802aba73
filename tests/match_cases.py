"""Seeded point sets and the shape list of the sparse-matching tests (test_match_host.py,
test_gpu_match.py).  The shapes are derived from the binding's constants - the block of
predictions, the LDS tile, the segment rule and the scan's threads - so a later change of a
constant cannot let a test miss the path it is there for."""
import numpy as np

from flypylib_amd import _matchcapi as capi, match

T = 27.0                       # the pipeline's obj_min_dist


def jittered(seed, n_pred, n_gt, box=520.0, sd=4.0, integer=False):
    """ground truth uniform in a box; predictions are jittered copies of most of it plus
    uniform false positives, shuffled; -> (pred locs, gt locs, conf)"""
    rs = np.random.RandomState(seed)
    gt = rs.rand(n_gt, 3) * box
    hits = min(n_gt, n_pred) * 9 // 10
    pred = np.concatenate([gt[:hits] + rs.randn(hits, 3) * sd, rs.rand(n_pred - hits, 3) * box])
    pred = pred[rs.permutation(n_pred)]
    if integer:
        pred, gt = np.rint(pred), np.rint(gt)
    return pred, gt, rs.rand(n_pred)


def crowd(seed, n_pred, n_gt, side=40.0):
    """every point in one cube of `side` voxels, non-integer: at T most (prediction, segment)
    cells hold pairs, so a wrong offset cannot hide in empty cells"""
    rs = np.random.RandomState(seed)
    return rs.rand(n_pred, 3) * side + 100.25, rs.rand(n_gt, 3) * side + 100.25


def clustered(seed, n_far=300, box=2000.0):
    """200 predictions and 200 ground-truth points within one ball 40 voxels across - large
    components, rows with more than 100 pairs - among sparse far points whose rows have none"""
    rs = np.random.RandomState(seed)

    def ball(n):
        v = rs.randn(n, 3)
        v *= (20.0 * rs.rand(n, 1) ** (1 / 3.0)) / np.linalg.norm(v, axis=1, keepdims=True)
        return v + box / 2
    far_p, far_g = rs.rand(n_far, 3) * box, rs.rand(n_far, 3) * box
    keep = np.linalg.norm(far_p[:, None] - np.concatenate([far_g, [[box / 2] * 3]])[None], axis=2)
    far_p = far_p[keep.min(axis=1) > 100.0]          # their rows hold no pair at all
    pred = np.concatenate([far_p[:len(far_p) // 2], ball(200), far_p[len(far_p) // 2:]])
    gt = np.concatenate([far_g[:100], ball(200), far_g[100:]])
    return pred, gt


def apart(seed, n_pred, n_gt):
    """no pair at all: the predictions lie 10 000 voxels away from every ground-truth point"""
    rs = np.random.RandomState(seed)
    return rs.rand(n_pred, 3) * 520 + 10000.0, rs.rand(n_gt, 3) * 520


def fractional(seed, n_pred, n_gt):
    """detections as voxel2obj returns them with a fractional volume_offset, against integer
    T-bars"""
    pred, gt, _ = jittered(seed, n_pred, n_gt, integer=True)
    return pred + np.array([0.5, 0.25, 0.125]), gt


def boundary(t=27):
    """integer points, among them pairs at exactly t: offsets (t, 0, 0) and, at t = 27,
    (18, 18, 9).  Cost 0 is not below 0 - inadmissible - but s = t^2 <= T2: in the superset."""
    assert t == 27
    gt = np.array([[100, 100, 100], [300, 100, 100], [100, 300, 100], [300, 300, 300],
                   [500, 500, 500]], np.float64)
    pred = np.concatenate([gt[:1] + [27, 0, 0], gt[1:2] + [18, 18, 9], gt[2:3] - [9, 18, 18],
                           gt[3:4] + [26, 0, 0], gt[3:4] + [0, 28, 0], gt[4:5] + [18, 18, 8]])
    return pred, gt


def dense_s(pred, gt):
    delta = pred.reshape(-1, 1, 3) - gt.reshape(1, -1, 3)
    return (delta ** 2).sum(axis=2)


def dense_pairs(pred, gt, t):
    i, j = np.nonzero(dense_s(pred, gt) <= match.threshold2(t))
    return i.astype(np.int32), j.astype(np.int32)


def assert_clear_of_t2(pred, gt, t):
    """no pair has s within a relative 2^-45 of T2: the superset is then the same set for any
    correctly rounded s, whatever the order of its additions"""
    t2 = match.threshold2(t)
    assert not np.any(np.abs(dense_s(pred, gt) - t2) <= t2 * 2.0 ** -45)


def segment_of(n_pred, n_gt, j):
    return np.asarray(j) // capi.segment_len(n_pred, n_gt)


def live_segments(n_pred, n_gt):
    """the segments that hold ground-truth points"""
    return -(-n_gt // capi.segment_len(n_pred, n_gt))


def scan_run(n_pred, n_gt):
    """(cells, cells per scan thread)"""
    cells = n_pred * capi.segments(n_pred, n_gt)
    return cells, -(-cells // capi.SCAN_THREADS)


B, L, S = capi.BLOCK, capi.TILE, capi.SCAN_THREADS

# (n_pred, n_gt, why); every one is a crowd(): most cells hold pairs
SHAPES = [
    (1, 1, 'one thread, one point'),
    (1, L + 44, 'one prediction, two segments'),
    (300, 1, 'one ground-truth point: G == 1'),
    (B - 1, 300, 'block edge: one short block'),
    (B, 300, 'block edge: one full block'),
    (B + 1, 300, 'block edge: a block of one prediction'),
    (300, L - 1, 'tile edge: one short tile, G == 1'),
    (300, L, 'tile edge: one full tile, G == 1'),
    (300, L + 1, 'tile edge: a tile of one point'),
    (300, 2 * L + 1, 'three tiles in G == 4 segments: the last segment is empty, 513 % 4 != 0'),
    (300, 5 * L + 7, 'six tiles in G == 8 segments: two empty segments, a short last tile'),
    (S + 1, L - 6, 'G == 1, 1 025 cells: scan runs of 2, a short last run'),
    (2 * S + 2, L - 6, 'G == 1, 2 050 cells: scan runs of 3, a short last run'),
    (S + 1, L + 44, 'G == 2, 2 050 cells: scan runs of 3 across segments'),
]


def check_shapes():
    """the reasons above, asserted against the binding's rule"""
    g = {(n, m): capi.segments(n, m) for n, m, _ in SHAPES}
    assert g[(1, L + 44)] == 2 and g[(300, 1)] == 1 and g[(300, L)] == 1 and g[(300, L - 1)] == 1
    assert g[(300, L + 1)] == 2
    assert g[(300, 2 * L + 1)] == 4 and live_segments(300, 2 * L + 1) == 3
    assert (2 * L + 1) % 4 != 0
    assert g[(300, 5 * L + 7)] == 8 and live_segments(300, 5 * L + 7) == 6
    assert g[(S + 1, L - 6)] == 1 and scan_run(S + 1, L - 6) == (S + 1, 2)
    assert g[(2 * S + 2, L - 6)] == 1 and scan_run(2 * S + 2, L - 6) == (2 * S + 2, 3)
    assert (2 * S + 2) % 3 != 0
    assert g[(S + 1, L + 44)] == 2 and scan_run(S + 1, L + 44) == (2 * S + 2, 3)
    assert max(max(n, m) for n, m, _ in SHAPES) <= 5000
