"""Inputs and measures shared by test_mine_host.py (CPU) and test_gpu_mine.py (GPU)."""
import numpy as np

from flypylib_amd._minecapi import CHUNK           # FPLM_CHUNK: flat voxels per count wave


def ulp_distance(a, b):
    """distance in float32 ulps (units in the last place, counted over the ordered floats)"""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def mining_case(seed, shape):
    rs = np.random.RandomState(seed)
    pred = rs.uniform(0, 1, shape).astype(np.float32)
    ll = (rs.uniform(0, 1, shape) > 0.9).astype(np.uint8)
    ll[rs.uniform(0, 1, shape) > 0.98] = 3           # a label that is neither class
    mm = (rs.uniform(0, 1, shape) > 0.2).astype(np.uint8)
    mm[rs.uniform(0, 1, shape) > 0.97] = 2           # a mask value that is neither 0 nor 1
    return pred, ll, mm


# ---- volumes that reach the scan runs, the grid stride and the short rows ------------------
# The constants of csrc/mine/mine.hip, named once: a shape below is chosen against them, and
# tests/test_mine_host.py asserts (without a GPU) that each shape reaches its path.
BLOCK = 256                  # lanes per block of voxel_loss_kernel
LANE_VOX = 4                 # consecutive flat voxels per lane: a group
LOSS_GRID_CAP = 2048         # blocks of voxel_loss_kernel; the rest by stride
SCAN_THREADS = 1024          # scan_kernel: one block, each thread a run of `per` chunks
PASS_VOXELS = LOSS_GRID_CAP * BLOCK * LANE_VOX     # voxels one pass of the loss grid covers

# name -> (shape, half): the smallest volumes with `per` 1 exactly full, `per` 2 with one
# chunk in the last run, `per` 2 with a short last run and a strided loss, `per` 3 with a run
# of 2 at the end.  The halves leave the z faces alone where a plane is longer than a run of
# chunks, so that no run lies wholly inside the border.
SCAN_SHAPES = {
    'scan_full': ((64, 256, 256), (0, 3, 5)),
    'scan_one_over': ((4194305, 1, 1), (2, 0, 0)),
    'scan_runs_2': ((173, 175, 177), (0, 2, 7)),
    'scan_runs_3': ((215, 217, 219), (0, 4, 6)),
}
SCAN_SEEDS = {'scan_full': 21, 'scan_one_over': 22, 'scan_runs_2': 23, 'scan_runs_3': 24}


def scan_layout(shape):
    """what scan_kernel and voxel_loss_kernel make of a volume: n_chunks, per, the last thread
    with a non-empty run and that run's length, the voxels of the last chunk, the groups of
    four and the passes of the loss grid"""
    n = int(np.prod(shape, dtype=np.int64))
    n_chunks = -(-n // CHUNK)
    per = -(-n_chunks // SCAN_THREADS)
    last_thread = (n_chunks - 1) // per
    groups = -(-n // LANE_VOX)
    return dict(voxels=n, n_chunks=n_chunks, per=per, last_thread=last_thread,
                last_run=n_chunks - last_thread * per, last_chunk_voxels=n - (n_chunks - 1) * CHUNK,
                groups=groups, passes=-(-groups // (LOSS_GRID_CAP * BLOCK)))


def run_sums(per_voxel, shape):
    """`per_voxel` (a bool or count per voxel, any shape of the volume's size) summed over each
    scan thread's run of chunks: one int64 per thread that has a run"""
    lay = scan_layout(shape)
    flat = np.asarray(per_voxel).reshape(-1)
    starts = np.arange(0, lay['voxels'], lay['per'] * CHUNK)
    assert len(starts) == lay['last_thread'] + 1
    return np.add.reduceat(flat.astype(np.int64), starts)


def rows_per_run(z, y, x, shape):
    """candidate rows per scan thread's run, from the rows' own coordinates"""
    lay = scan_layout(shape)
    flat = (z.astype(np.int64) * shape[1] + y) * shape[2] + x
    return np.bincount(flat // (lay['per'] * CHUNK), minlength=lay['last_thread'] + 1)


def scan_weights(shape):
    """the weights of the compaction tests: uniform(-1, 1), every third plane 0, one NaN"""
    ww = np.random.RandomState(3).uniform(-1, 1, shape).astype(np.float32)
    ww[::3] = 0
    z = shape[0] // 2
    ww[z + (z % 3 == 0), shape[1] // 2, shape[2] // 2] = np.nan      # in a plane that has weights
    return ww


def scan_case(name, cc=None):
    """(pred, labels, mask, weights) of a SCAN_SHAPES volume.  `scan_one_over` is built per
    class `cc`: voxel 0 and the single voxel of the last chunk are forced to be candidates of
    that class (they count only under a half that leaves the z faces in)."""
    shape, _ = SCAN_SHAPES[name]
    pred, ll, mm = mining_case(SCAN_SEEDS[name], shape)
    ww = scan_weights(shape)
    if name == 'scan_one_over':
        for i in (0, -1):
            ll[i, 0, 0], mm[i, 0, 0], ww[i, 0, 0] = cc, 1, 0.25
    return pred, ll, mm, ww


# (name, half, class): classes 1 and 3 everywhere, the dense class 0 on two; scan_one_over
# also without a border, where its forced first and last voxel count
COMPACTION_CASES = [(n, SCAN_SHAPES[n][1], cc) for n, ccs in (
    ('scan_full', (1, 3)), ('scan_one_over', (0, 1, 3)), ('scan_runs_2', (0, 1, 3)),
    ('scan_runs_3', (1, 3))) for cc in ccs] + [('scan_one_over', (0, 0, 0), cc) for cc in (1, 3)]
MIN_ELIGIBLE = 512           # a run with this many eligible voxels must hold a candidate


def eligible_per_run(shape, half, weighted):
    """per scan thread's run, the voxels that can be candidates at all: inside the `half`
    border and, with scan_weights, outside the planes whose weight is 0"""
    ok = np.zeros(shape, bool)
    ok[tuple(slice(b, d - b) if d - b > b else slice(0, 0) for d, b in zip(shape, half))] = True
    if weighted:
        ok[::3] = False
    return run_sums(ok, shape)


def assert_runs_hold_candidates(name, half, weighted, z, y, x):
    """an offset error must not hide in empty chunks: every run of `per` chunks with
    MIN_ELIGIBLE eligible voxels holds rows, the last run among them; without weights that is
    every run of the volume (but the one-voxel last run of scan_one_over under its border)"""
    shape = SCAN_SHAPES[name][0]
    eligible, rows = eligible_per_run(shape, half, weighted), rows_per_run(z, y, x, shape)
    must = eligible >= MIN_ELIGIBLE
    bordered_tail = name == 'scan_one_over' and half[0] > 0
    if name == 'scan_one_over' and not bordered_tail:
        must[-1] = True      # one voxel, forced
    assert (rows[must] > 0).all(), (name, half, weighted, np.flatnonzero(must & (rows == 0))[:8])
    # the last run holds rows, save under scan_full's weights, whose last plane has none
    if not (weighted and name == 'scan_full'):
        assert must[-1] != bordered_tail and (rows[-1] > 0) != bordered_tail
    if not weighted:
        assert must[:-1].all()
    assert must.sum() > 0.5 * len(must)
    return int(must.sum()), len(must)


# (shape, border): rows shorter than a group of four, so that Position::next carries into y
# and z inside one group, and borders at and beyond the extent
SHORT_ROW_CASES = [
    ((40, 1, 1), (3, 0, 0)),
    ((17, 3, 1), (2, 1, 0)),
    ((9, 2, 3), (1, 0, 1)),
    ((6, 5, 2), (1, 1, 0)),
    ((9, 11, 13), (100, 0, 0)),      # clamped to the extent: selects nothing
    ((9, 11, 13), (4, 5, 6)),        # leaves the single centre voxel
    ((8, 8, 8), (4, 0, 0)),          # d - b == b: nothing remains
]
# voxels inside the border, by hand
SHORT_ROW_INSIDE = [34, 13, 14, 24, 0, 1, 0]

# predictions off the unit interval, and the exact 1
OFF_UNIT = [np.nan, np.inf, -np.inf, -0.25, 1.5, 1.0]


def off_unit_case():
    """(pred, labels, mask) on 9 x 11 x 13, mask 1: each OFF_UNIT value under a label-0 and a
    label-1 voxel, the rest as mining_case gives it"""
    shape = (9, 11, 13)
    pred, ll, _ = mining_case(31, shape)
    mm = np.ones(shape, np.uint8)
    for k, v in enumerate(OFF_UNIT):
        # x = 2k, 2k + 1: the pairs fall into different groups of four
        pred[4, 5, 2 * k:2 * k + 2] = v
        ll[4, 5, 2 * k], ll[4, 5, 2 * k + 1] = 0, 1
        pred[7, 2 + k, 3:5] = v
        ll[7, 2 + k, 3], ll[7, 2 + k, 4] = 1, 0
    return pred, ll, mm
