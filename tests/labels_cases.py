"""Seeded inputs shared by tests/test_labels_host.py and tests/test_gpu_labels.py: T-bar
lists whose cubes stay inside the volume, and roi masks drawn from {0, 1, 2, 255}."""
import numpy as np

# (radius_use, radius_ign, buffer_size) x shape: the 14 cases the per-voxel rule was derived on
RULE_PARAMS = [(3, 6, 4), (2, 5, 0), (4, None, 3), (5, 3, 2), (0, 2, 1), (3, 3, 5), (1, 0, 2)]
RULE_SHAPES = [(36, 38, 40), (23, 17, 29)]
RULE_CASES = [(p, s) for p in RULE_PARAMS for s in RULE_SHAPES]

GOLDEN_TBARS = {'locs': np.array([[12, 14, 16], [20, 15, 13], [25, 25, 25]]), 'conf': np.ones(3)}


def half_width(radius_use, radius_ign):
    return max(int(radius_use), int(radius_ign or 0))


def random_tbars(seed, shape, half, n, box=None):
    """n T-bars, float (x, y, z) with fractions (the host truncates them), whose cubes of
    half-width `half` lie inside the (Z, Y, X) volume; `box` = ((x0, x1), (y0, y1), (z0, z1))
    confines the integer positions further (a cluster)"""
    rs = np.random.RandomState(seed)
    ext = shape[::-1]
    cols = []
    for a in range(3):
        lo, hi = half, ext[a] - half
        if box is not None:
            lo, hi = max(lo, box[a][0]), min(hi, box[a][1])
        assert hi > lo, (shape, half, box)
        cols.append(rs.randint(lo, hi, n))
    locs = np.stack(cols, axis=1).astype(np.float64) + rs.rand(n, 3) * 0.99
    return {'locs': locs, 'conf': np.ones(n)}


def random_roi(seed, shape):
    rs = np.random.RandomState(seed)
    return rs.choice(np.array([0, 1, 2, 255], np.uint8), size=shape, p=[0.2, 0.5, 0.15, 0.15])


def rule_case(i):
    (ru, ri, buf), shape = RULE_CASES[i]
    tbars = random_tbars(100 + i, shape, half_width(ru, ri), 40)
    return tbars, random_roi(200 + i, shape), ru, ri, buf
