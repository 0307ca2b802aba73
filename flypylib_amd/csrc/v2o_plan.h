// Dispatch plan of the float32 voxel2obj stages (v2o.hip): which smoothing kernels run, with
// what workgroup size, segmentation of the z columns, LDS tile and grids, and which window-max
// and ball-clearing forms the NMS takes.  v2o.hip launches from these plans and holds no copy of
// the conditions or of the constants below.  Plain C++ on standard headers only: a host compiler
// builds it alone (tests/test_v2o_plan.py does, and prints the plan of every test case).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

constexpr int CELL = 4;                       // edge of an NMS cell
// x pass through LDS (gauss_x_lds): a workgroup takes GX_ROWS (z,y) rows x GX_SEG outputs
constexpr int GX_ROWS = 8, GX_SEG = 128;
constexpr int GZ_OUT = 12;       // (the size limit of the 32-bit offsets of gauss_z_ring still counts in these rows)
// 12 rows per tile of gauss_yx_fused: the tile is 33 KiB at P2 = 636 and four workgroups fit a
// CU (16 rows, three workgroups: 1.07 ms against 0.94; 8 rows: 0.97).
constexpr int GYX_TY = 12;
constexpr int GYX_LDS_MAX = 60 * 1024;        // dynamic LDS gauss_yx_fused may ask for
constexpr int GW_OUT_ZY = 16;                 // outputs per thread of gauss_pass_win<0/1>
constexpr int WM_OUTS = 8;                    // cells per thread of window_max_seg
constexpr int WM_HW_MAX = 8;                  // largest half window window_max_seg is built for
constexpr int CLR_STAGE = 6144;               // >= the 17^3 cells of a bounding box at r = 31;
                                              // beyond it appends go straight to the list
constexpr int CLR_PARTS = 4;                  // workgroups per winner of clear_balls
constexpr int CLR_ROWS = 1024;                // rows of one part of the cube, r <= 31
constexpr int CLR_SEG_WGS = 1024;             // workgroups of clear_balls_seg

static inline int64_t v2o_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// LDS floats per tile row of gauss_yx_fused: the row, its two halos, rounded up to a
// 16-B multiple plus 4 (the last thread's aligned window may read 3 floats past it)
static inline int gyx_lrow(int64_t P2, int wr) {
  return (int)((v2o_cdiv(P2, 8) * 8 + 2 * wr + 3) / 4 * 4 + 4);
}
// workgroup size (a multiple of 64 in [256, 512]) that wastes the fewest lanes on `n`
// columns / pieces per pass
static inline int best_block(int64_t n) {
  int best = 256;
  double waste = 1e9;
  for (int bd = 256; bd <= 512; bd += 64) {
    const double wst = (double)(v2o_cdiv(n, bd) * bd) / (double)n;
    if (wst < waste - 1e-9) { waste = wst; best = bd; }
  }
  return best;
}
static inline size_t gyx_lds_bytes(int64_t P2, int wr) {
  return (size_t)GYX_TY * gyx_lrow(P2, wr) * sizeof(float) +
         (size_t)(GYX_TY / CELL) * v2o_cdiv(P2, CELL) * sizeof(unsigned long long);
}
static inline bool gyx_fits(const int64_t P[3], int wr) {
  // single-bounce reflections, 32-bit in-plane offsets, tile + cell keys within 60 KiB
  return P[1] * P[2] * 4 < ((int64_t)1 << 31) && P[2] >= 2 * wr && P[1] >= GYX_TY + 2 * wr && P[0] * v2o_cdiv(P[1], GYX_TY) < (1 << 28) &&
         gyx_lds_bytes(P[2], wr) <= (size_t)GYX_LDS_MAX;
}

// The smoothing of a padded volume P (= D + 2 r) with a kernel of radius wr.
//   !windowed:            gauss_pass<0>, <1>, <2>                      (any wr)
//   windowed, z pass:     ring ? gauss_z_ring : gauss_pass_win<0>
//   windowed, y/x passes: fused ? gauss_yx_fused : gauss_pass_win<1> + gauss_x_lds
struct V2oSmoothPlan {
  bool windowed;        // wr is one of the register-window instances (3, 4, 6, 10)
  bool fits;            // gyx_fits: the fused y/x pass can take this shape
  bool fused;           // ... and does (fits, and the FPL_V2O_UNFUSED switch is not set)
  bool ring;            // gauss_z_ring (32-bit offsets hold, P0 >= 2 wr, switch not set)
  int block;            // workgroup size of gauss_z_ring and gauss_yx_fused
  int64_t nxb;          // x blocks of `block` columns per (y, segment) of gauss_z_ring
  int64_t seg_len;      // outputs per z segment of gauss_z_ring: a multiple of 4 wr
  int64_t nseg;         // segments per column
  int lrow;             // LDS floats per tile row of gauss_yx_fused
  size_t lds_bytes;     // its dynamic LDS
  int64_t z_grid, yx_grid, y_grid, x_tiles;   // workgroups (x: tiles, before the grid stride)
  int64_t plain_grid;   // workgroups of each gauss_pass
  // the grids as launched on a device of n_cu compute units; 0: the pass does not run
  int64_t grid_z(int /*n_cu*/) const { return windowed ? z_grid : plain_grid; }
  int64_t grid_yx(int /*n_cu*/) const { return fused ? yx_grid : 0; }
  int64_t grid_y(int /*n_cu*/) const { return windowed ? (fused ? 0 : y_grid) : plain_grid; }
  int64_t grid_x(int n_cu) const {
    return windowed ? (fused ? 0 : std::min<int64_t>(x_tiles, (int64_t)n_cu * 8)) : plain_grid;
  }
};

static inline V2oSmoothPlan v2o_smooth_plan(const int64_t P[3], int64_t D1, int64_t D2, int wr,
                                            bool unfused_env) {
  V2oSmoothPlan p = {};
  // register-window kernels for the kernel radii flypylib's sigmas produce
  // (sigma 1.5, 2, 3, 5 at truncate 2.0); the plain kernel covers the rest
  p.windowed = wr == 3 || wr == 4 || wr == 6 || wr == 10;
  p.block = 256;
  p.plain_grid = v2o_cdiv(P[0] * P[1] * P[2], 256);
  if (!p.windowed) return p;
  p.fits = gyx_fits(P, wr);
  p.fused = p.fits && !unfused_env;
  // 32-bit in-column / in-plane offsets of gauss_z_ring
  const bool small = (GZ_OUT + 2 * wr) * D1 * D2 < ((int64_t)1 << 31) &&
                     P[1] * P[2] * GZ_OUT < ((int64_t)1 << 31) && P[0] >= 2 * wr;
  p.ring = small && !unfused_env;
  // ring form: segments of a multiple of 4 WR outputs (two steps), about a quarter of the column
  p.block = best_block(P[2]);
  p.nxb = v2o_cdiv(P[2], p.block);
  p.seg_len = std::max<int64_t>(4 * wr, v2o_cdiv(v2o_cdiv(P[0], 4), 4 * wr) * 4 * wr);
  p.nseg = v2o_cdiv(P[0], p.seg_len);
  p.z_grid = p.ring ? p.nxb * p.nseg * P[1]
                    : v2o_cdiv(v2o_cdiv(P[0], GW_OUT_ZY) * P[1] * P[2], 256);
  p.lrow = gyx_lrow(P[2], wr);
  p.lds_bytes = gyx_lds_bytes(P[2], wr);
  // fused: whole rounds of the 8 XCDs over the (z group, y tile) work items.  Phase 1 walks P2
  // columns, phase 2 16 * ceil(P2 / 8) pieces: the workgroup is sized for the columns (the
  // pieces are ~2x as many and split evenly enough)
  p.yx_grid = v2o_cdiv(v2o_cdiv(P[0], CELL) * v2o_cdiv(P[1], GYX_TY), 8) * 8;
  p.y_grid = v2o_cdiv(P[0] * v2o_cdiv(P[1], GW_OUT_ZY) * P[2], 256);
  p.x_tiles = v2o_cdiv(P[0] * P[1], GX_ROWS) * v2o_cdiv(P[2], GX_SEG);
  return p;
}

// The NMS on a padded volume P with suppression radius r.
struct V2oNmsPlan {
  int64_t C[3], n_cells;  // cells per axis and in all
  int hw;                 // window half width in cells
  bool wmax_seg;          // window_max_x + window_max_seg<., HW>; else the plain window_max
  int HW;                 // its template instance (0: plain)
  bool aligned;           // P2 % CELL == 0: a cell row is one aligned 16-B piece
  bool clear_table;       // clear_balls: a part's rows fit its LDS row table
  bool clear_direct;      // ... a part computes its rows directly (no r has both: the test)
  int seg_words;          // W of clear_balls_seg (64-bit masks per cube row); 0 without use_seg
  bool seg_rows_global;   // its row sets live in global memory (W > 1)
  size_t seg_rows_bytes;  // ... of this size;  W == 1: the dynamic LDS of clear_balls_seg<1>
  // what a ball can ask of touch_cell's LDS stage (filled when asked for: the launches do not
  // depend on it).  A cell is cut when the ball reaches it but does not hold all of it;
  // clear_balls_seg lists every cell of the ball's bounding box.
  int64_t cut_cells_max;    // most cells one ball can hand to the re-scan list
  int64_t stage_cells_max;  // most of them that ONE workgroup stages before it flushes: a
                            // quarter slab (CLR_PARTS) of clear_balls, all of clear_balls_seg
  bool stage_overflows;     // stage_cells_max > CLR_STAGE: touch_cell can append directly
};

// squared distance range from `centre` to the integer interval [lo, lo + CELL - 1]
// (the arithmetic of clear_balls' span2)
static inline void v2o_span2(int64_t lo, int64_t centre, int &near2, int &far2) {
  const int a = (int)(lo - centre), b = (int)(lo + CELL - 1 - centre);
  const int n = a > 0 ? a : (b < 0 ? -b : 0);
  const int f = -a > b ? -a : b;
  near2 = n * n; far2 = f * f;
}

// cut_cells_max / stage_cells_max: every phase (centre % CELL) per axis, the cell box and the
// part slices exactly as clear_balls / clear_balls_seg walk them
static inline void v2o_cut_cells(int r, bool use_seg, int64_t *cut_max, int64_t *stage_max) {
  *cut_max = *stage_max = 0;
  const int64_t base = (int64_t)(r / CELL + 2) * CELL;       // a centre well inside: no negative cell
  for (int pz = 0; pz < CELL; ++pz)
    for (int py = 0; py < CELL; ++py)
      for (int px = 0; px < CELL; ++px) {
        const int64_t z = base + pz, y = base + py, x = base + px;
        const int64_t cz0 = (z - r) / CELL, cy0 = (y - r) / CELL, cx0 = (x - r) / CELL;
        const int nz = (int)((z + r) / CELL - cz0 + 1), ny = (int)((y + r) / CELL - cy0 + 1),
                  nx = (int)((x + r) / CELL - cx0 + 1);
        const int64_t ncell = (int64_t)nz * ny * nx;
        if (use_seg) {
          *cut_max = std::max(*cut_max, ncell);
          *stage_max = std::max(*stage_max, ncell);
          continue;
        }
        int64_t total = 0;
        for (int part = 0; part < CLR_PARTS; ++part) {
          const int64_t cell_lo = ncell * part / CLR_PARTS, cell_hi = ncell * (part + 1) / CLR_PARTS;
          int64_t cut = 0;
          for (int64_t i = cell_lo; i < cell_hi; ++i) {
            const int64_t cz = cz0 + i / (ny * nx), cy = cy0 + (i / nx) % ny, cx = cx0 + i % nx;
            int nz2, fz2, ny2, fy2, nx2, fx2;
            v2o_span2(cz * CELL, z, nz2, fz2);
            v2o_span2(cy * CELL, y, ny2, fy2);
            v2o_span2(cx * CELL, x, nx2, fx2);
            if (nz2 + ny2 + nx2 > r * r) continue;                  // untouched
            if (fz2 + fy2 + fx2 <= r * r) continue;                 // dead: not listed
            ++cut;
          }
          *stage_max = std::max(*stage_max, cut);
          total += cut;
        }
        *cut_max = std::max(*cut_max, total);
      }
}

static inline V2oNmsPlan v2o_nms_plan(const int64_t P[3], int r, bool use_seg,
                                      bool wmax_plain_env = false, bool count_cut_cells = true) {
  V2oNmsPlan p = {};
  for (int a = 0; a < 3; ++a) p.C[a] = v2o_cdiv(P[a], CELL);
  p.n_cells = p.C[0] * p.C[1] * p.C[2];
  // window half-width in cells: cells [c-hw, c+hw] cover [4c-4hw, 4c+4hw+3]
  // which must contain [p-r, p+r] for every p in [4c, 4c+3]
  p.hw = (r + CELL - 1) / CELL;
  p.wmax_seg = p.hw >= 1 && p.hw <= WM_HW_MAX && p.n_cells < ((int64_t)1 << 31) && !wmax_plain_env;
  p.HW = p.wmax_seg ? p.hw : 0;
  p.aligned = P[2] % CELL == 0;
  const int side = 2 * r + 1;
  const int rows = side * side;
  for (int part = 0; part < CLR_PARTS; ++part) {
    const int row_lo = (int)((int64_t)rows * part / CLR_PARTS),
              row_hi = (int)((int64_t)rows * (part + 1) / CLR_PARTS);
    if (row_hi - row_lo <= CLR_ROWS) p.clear_table = true;
    else p.clear_direct = true;
  }
  if (use_seg) {
    const int W = (side + 63) / 64;
    p.seg_words = W == 1 ? 1 : (W == 2 ? 2 : 4);
    p.seg_rows_global = p.seg_words > 1;
    p.seg_rows_bytes = p.seg_rows_global
        ? (size_t)CLR_SEG_WGS * 2 * side * side * p.seg_words * 8
        : (size_t)2 * side * side * sizeof(unsigned long long);
  }
  if (count_cut_cells) {
    v2o_cut_cells(r, use_seg, &p.cut_cells_max, &p.stage_cells_max);
    p.stage_overflows = p.stage_cells_max > CLR_STAGE;
  }
  return p;
}
