"""The voxel2obj branch cases: one table for tests/test_v2o_plan.py (CPU: which branch of
csrc/v2o_plan.h a shape takes) and tests/test_gpu_v2o_branches.py (GPU: bit parity with the
oracle on that branch).

A case is (name, kind, seed, D, r, sigma, thd, n_min, want): `kind` names the generator of the
prediction (`make_pred`), `n_min` is the number of detections the oracle finds (recorded when the
case was added; the GPU test asserts at least as many), `want` the plan fields the case is there
for - v2o_plan.h's names, the smoothing plan's and the NMS plan's in one dict.  Every case holds
fewer than 10 M padded voxels.
"""
import os
import shutil
import subprocess

import numpy as np

from flypylib_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'flypylib_amd', 'csrc')

SEED = 11
N_CU = 256                      # MI355X: what the grid-stride rows of the table are counted for


def wr_of(sigma):
    """radius of the Gaussian at truncate 2.0 (fplobjdetect.gaussian_kernel1d)"""
    return int(2.0 * sigma + 0.5)


# the coordinates, per axis, of the 'stage' case's peaks in a 72-voxel axis: one per NMS cell of
# the padded volume at r = 35 (cells 8 .. 26), the centre's (35) at phase 2 of its cell so that
# its ball's bounding box is 19 cells wide
_STAGE_AXIS = [0] + [4 * k for k in range(1, 9)] + [35] + [4 * k for k in range(10, 18)] + [70]


def make_pred(kind, D):
    if kind == 'blobs':
        return synth.blob_prob_volume(SEED, D, period=32, radius=7.0)
    if kind == 'uniform':
        return synth.hash_uniform_f32(SEED, D)
    if kind == 'corners':
        # 1.0 at the 8 corners and the 6 face centres over noise x 0.1: balls clipped by the r
        # shell of the padded volume on every side
        v = synth.hash_uniform_f32(SEED, D) * np.float32(0.1)
        for z in (0, D[0] - 1):
            for y in (0, D[1] - 1):
                for x in (0, D[2] - 1):
                    v[z, y, x] = 1.0
        c = [d // 2 for d in D]
        for ax in range(3):
            for e in (0, D[ax] - 1):
                p = list(c)
                p[ax] = e
                v[tuple(p)] = 1.0
        return v
    if kind == 'stage':
        # one peak in every NMS cell of the centre peak's bounding box (and nothing else): every
        # cell of that box is live when the centre wins the first round, alone
        assert tuple(D) == (72, 72, 72)
        a = np.asarray(_STAGE_AXIS)
        v = np.zeros(D, np.float32)
        noise = synth.hash_uniform_f32(SEED, (a.size,) * 3)
        v[np.ix_(a, a, a)] = np.float32(0.5) + noise * np.float32(0.1)
        v[35, 35, 35] = 1.0
        return v
    raise ValueError(kind)


def make_seg(D):
    return synth.voronoi_segmentation(SEED, D, 12, 0)


# cases that run a second time with a Voronoi segmentation (seg_dilate 2): name -> n_min
SEG_CASES = {'r31': 20, 'r32': 20, 'stage': 34}

CASES = [
    # ---- workgroup size and x blocks of gauss_z_ring / gauss_yx_fused (one per window radius)
    ('x574', 'uniform', SEED, (20, 24, 564), 5, 5.0, 0, 171,
     dict(wr=10, fused=True, ring=True, block=320, nxb=2, aligned=False, HW=2)),
    ('x500', 'uniform', SEED, (16, 30, 490), 5, 3.0, 0, 198,
     dict(wr=6, fused=True, ring=True, block=256, nxb=2, aligned=True)),
    ('x448', 'uniform', SEED, (16, 30, 440), 4, 2.0, 0, 302,
     dict(wr=4, fused=True, ring=True, block=448, nxb=1, aligned=True, HW=1)),
    ('x380', 'uniform', SEED, (16, 30, 370), 5, 1.5, 0, 336,
     dict(wr=3, fused=True, ring=True, block=384, nxb=1, aligned=True)),
    # (no P2 gives a workgroup of 512: ceil(n / 256) * 256 <= ceil(n / 512) * 512 for every n, and
    # best_block keeps the smaller size on a tie; P2 = 504 is the nearest miss)
    ('x504', 'uniform', SEED, (16, 30, 494), 5, 5.0, 0, 210,
     dict(wr=10, fused=True, ring=True, block=256, nxb=2, aligned=True)),
    # ---- the LDS limit of the fused pass
    ('lds', 'uniform', SEED, (30, 40, 1190), 5, 5.0, 0, 816,
     dict(wr=10, fits=False, fused=False, ring=True, block=256, nxb=5, aligned=True, x_stride=True)),
    ('lds_1112', 'uniform', SEED, (12, 24, 1102), 5, 5.0, 0, 304,
     dict(wr=10, fused=True, ring=True, lds_bytes=61200)),
    ('lds_1113', 'uniform', SEED, (12, 24, 1103), 5, 5.0, 0, 299,
     dict(wr=10, fits=False, fused=False, ring=True, aligned=False)),
    ('lds_1120_w4', 'uniform', SEED, (12, 24, 1114), 3, 2.0, 0, 748,
     dict(wr=4, fused=True, ring=True)),
    ('lds_1121_w4', 'uniform', SEED, (12, 24, 1115), 3, 2.0, 0, 753,
     dict(wr=4, fits=False, fused=False, ring=True)),
    # ---- axes shorter than the window: multi-bounce reflections, gauss_pass_win<0>
    ('thin_z_fused', 'uniform', SEED, (3, 40, 40), 2, 5.0, 0, 36,
     dict(wr=10, fused=True, ring=False, P0_lt_wr=True)),
    ('thin_z_fused_w3', 'uniform', SEED, (3, 40, 40), 1, 1.5, 0, 127,
     dict(wr=3, fused=True, ring=False)),
    ('tiny_all', 'uniform', SEED, (5, 6, 7), 1, 5.0, 0, 5,
     dict(wr=10, fused=False, ring=False, P0_lt_wr=True, P1_lt_wr=True, P2_lt_wr=True)),
    ('tiny_all_w6', 'uniform', SEED, (2, 3, 3), 1, 3.0, 0, 1,
     dict(wr=6, fused=False, ring=False, P0_lt_wr=True, P1_lt_wr=True, P2_lt_wr=True)),
    ('thin_x', 'uniform', SEED, (40, 40, 9), 3, 5.0, 0, 36,
     dict(wr=10, fused=False, ring=True, aligned=False, HW=1)),
    ('thin_x_w3', 'uniform', SEED, (40, 40, 1), 2, 1.5, 0, 54,
     dict(wr=3, fused=False, ring=True, P2_lt_2wr=True)),
    # ---- the ring's own edges: P0 = 2 wr - 1, 2 wr, 2 wr + 1; nseg 1 -> 2 at 4 wr, 4 wr + 1
    ('z19', 'uniform', SEED, (13, 30, 36), 3, 5.0, 0, 23, dict(wr=10, fused=True, ring=False)),
    ('z20', 'uniform', SEED, (14, 30, 36), 3, 5.0, 0, 25, dict(wr=10, fused=True, ring=True, nseg=1, seg_len=40)),
    ('z21', 'uniform', SEED, (15, 30, 36), 3, 5.0, 0, 22, dict(wr=10, fused=True, ring=True, nseg=1)),
    ('z40', 'uniform', SEED, (34, 30, 37), 3, 5.0, 0, 63, dict(wr=10, fused=True, ring=True, nseg=1, seg_len=40)),
    ('z41', 'uniform', SEED, (35, 30, 37), 3, 5.0, 0, 64, dict(wr=10, fused=True, ring=True, nseg=2, seg_len=40)),
    ('z7_w4', 'uniform', SEED, (1, 30, 36), 3, 2.0, 0, 27, dict(wr=4, fused=True, ring=False)),
    ('z11_w6', 'uniform', SEED, (5, 30, 36), 3, 3.0, 0, 27, dict(wr=6, fused=True, ring=False)),
    ('z12_w6', 'uniform', SEED, (6, 30, 36), 3, 3.0, 0, 31, dict(wr=6, fused=True, ring=True, nseg=1)),
    ('z13_w6', 'uniform', SEED, (7, 30, 36), 3, 3.0, 0, 26, dict(wr=6, fused=True, ring=True, nseg=1)),
    ('z24_w6', 'uniform', SEED, (18, 30, 37), 3, 3.0, 0, 41, dict(wr=6, fused=True, ring=True, nseg=1)),
    ('z25_w6', 'uniform', SEED, (19, 30, 37), 3, 3.0, 0, 42, dict(wr=6, fused=True, ring=True, nseg=2)),
    # ---- the plain three-pass kernel
    ('plain_s1', 'uniform', SEED, (5, 6, 50), 1, 1.0, 0, 43, dict(wr=2, windowed=False)),
    ('plain_s4', 'uniform', SEED, (5, 30, 5), 1, 4.0, 0, 26, dict(wr=8, windowed=False, P0_lt_wr=True, P2_lt_wr=True)),
    # ---- NMS: every window_max_seg instance the older tests leave out, the row table's end, the
    # plain window max without a segmentation
    ('hw4', 'blobs', SEED, (60, 50, 70), 14, 3.0, 0.02, 8, dict(HW=4, clear_table=True, wr=6, fused=True)),
    ('hw5', 'blobs', SEED, (60, 50, 70), 18, 3.0, 0.02, 8, dict(HW=5, clear_table=True, wr=6, fused=True)),
    ('hw6', 'blobs', SEED, (60, 50, 70), 23, 3.0, 0.02, 8, dict(HW=6, clear_table=True, wr=6, fused=True)),
    ('hw7', 'blobs', SEED, (60, 50, 70), 27, 3.0, 0.02, 8, dict(HW=7, clear_table=True, wr=6, fused=True)),
    ('r31', 'blobs', SEED, (60, 50, 70), 31, 3.0, 0.02, 8, dict(HW=8, clear_table=True, aligned=True, wr=6, fused=True)),
    ('r32', 'blobs', SEED, (60, 50, 71), 32, 3.0, 0.02, 8, dict(HW=8, clear_table=False, aligned=False, wr=6, fused=True)),
    ('r70', 'blobs', SEED, (150, 40, 44), 70, 2.0, 0.02, 2, dict(HW=0, hw=18, clear_table=False, wr=4, fused=True)),
    ('corners', 'corners', SEED, (40, 41, 42), 9, 2.0, 0, 37, dict(HW=3, wr=4, fused=True)),
    # touch_cell past CLR_STAGE.  Without a segmentation a workgroup of clear_balls stages a quarter
    # of a ball's cut cells, all of them at distance r from the winner, and they must be live:
    # the first such r (v2o_plan.h counts it; the plan test prints it) needs a volume far beyond
    # 10 M voxels.  clear_balls_seg stages the ball's whole bounding box: 19^3 = 6 859 cells at
    # r = 35, the first r with stage_overflows under a segmentation.
    ('stage', 'stage', SEED, (72, 72, 72), 35, 1.0, 0, 18, dict(HW=0, hw=9, windowed=False)),
]


def by_name(name):
    return next(c for c in CASES if c[0] == name)


def padded(D, r):
    return tuple(int(d) + 2 * int(r) for d in D)


# ---- csrc/v2o_plan.h, asked through a small driver built with the host compiler ------------

# One line in, one line out.  in: P0 P1 P2 D1 D2 wr unfused r use_seg wmax_plain n_cu;
# out: `key value` pairs of both plans
DRIVER = r'''
#include <cstdio>
#include <iostream>
#include "v2o_plan.h"
int main() {
  long long P0, P1, P2, D1, D2, wr, unfused, r, use_seg, wplain, n_cu, count;
  while (std::cin >> P0 >> P1 >> P2 >> D1 >> D2 >> wr >> unfused >> r >> use_seg >> wplain >> n_cu >> count) {
    const int64_t P[3] = {P0, P1, P2};
    const V2oSmoothPlan s = v2o_smooth_plan(P, D1, D2, (int)wr, unfused != 0);
    const V2oNmsPlan n = v2o_nms_plan(P, (int)r, use_seg != 0, wplain != 0, count != 0);
    printf("windowed %d fits %d fused %d ring %d block %d nxb %lld seg_len %lld nseg %lld lrow %d "
           "lds_bytes %zu grid_z %lld grid_yx %lld grid_y %lld grid_x %lld x_tiles %lld ",
           s.windowed, s.fits, s.fused, s.ring, s.block, (long long)s.nxb, (long long)s.seg_len,
           (long long)s.nseg, s.lrow, s.lds_bytes, (long long)s.grid_z((int)n_cu),
           (long long)s.grid_yx((int)n_cu), (long long)s.grid_y((int)n_cu),
           (long long)s.grid_x((int)n_cu), (long long)s.x_tiles);
    printf("C0 %lld C1 %lld C2 %lld n_cells %lld hw %d wmax_seg %d HW %d aligned %d clear_table %d "
           "clear_direct %d seg_words %d seg_rows_global %d seg_rows_bytes %zu cut_cells_max %lld "
           "stage_cells_max %lld stage_overflows %d\n",
           (long long)n.C[0], (long long)n.C[1], (long long)n.C[2], (long long)n.n_cells, n.hw,
           n.wmax_seg, n.HW, n.aligned, n.clear_table, n.clear_direct, n.seg_words,
           n.seg_rows_global, n.seg_rows_bytes, (long long)n.cut_cells_max,
           (long long)n.stage_cells_max, n.stage_overflows);
  }
  printf("constants CELL %d GX_ROWS %d GX_SEG %d GZ_OUT %d GYX_TY %d GYX_LDS_MAX %d WM_OUTS %d "
         "CLR_STAGE %d CLR_PARTS %d CLR_ROWS %d\n", CELL, GX_ROWS, GX_SEG, GZ_OUT, GYX_TY,
         GYX_LDS_MAX, WM_OUTS, CLR_STAGE, CLR_PARTS, CLR_ROWS);
  return 0;
}
'''


def host_cxx():
    for name in (os.environ.get('CXX'), 'c++', 'g++', 'clang++'):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def build_driver(tmp_path):
    """the driver's path, or None without a host compiler.  v2o_plan.h is built alone: no HIP, no
    other project header in reach"""
    cxx = host_cxx()
    if not cxx:
        return None
    src = tmp_path / 'v2o_plan_driver.cpp'
    src.write_text(DRIVER)
    exe = tmp_path / 'v2o_plan_driver'
    inc = tmp_path / 'inc'
    inc.mkdir()
    shutil.copy(os.path.join(CSRC, 'v2o_plan.h'), str(inc))
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I' + str(inc), '-o', str(exe), str(src)],
                   check=True)
    return str(exe)


def ask_plans(exe, queries):
    """queries: (P, D, wr, unfused, r, use_seg, wmax_plain, count_cut_cells) -> (list of dicts of
    ints, dict of the header's constants)"""
    text = ''.join('%d %d %d %d %d %d %d %d %d %d %d %d\n'
                   % (P[0], P[1], P[2], D[1], D[2], wr, unfused, r, use_seg, wplain, N_CU, count)
                   for P, D, wr, unfused, r, use_seg, wplain, count in queries)
    out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, check=True, text=True).stdout
    lines = out.strip().split('\n')
    assert len(lines) == len(queries) + 1 and lines[-1].startswith('constants ')

    def parse(tok):
        return {k: int(v) for k, v in zip(tok[0::2], tok[1::2])}
    return [parse(ln.split()) for ln in lines[:-1]], parse(lines[-1].split()[1:])
