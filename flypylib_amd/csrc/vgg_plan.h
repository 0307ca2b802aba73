// Slab and chunk geometry of the four fused VGG executors (vgg_like and vgg_like2, on plain
// 16-bit operands in vgg_fused.hip and on split halves in vgg_split.hip).  Plain C++ on
// standard headers only: a host compiler builds it alone (tests/test_vgg_plan.py does).
//
// Lattice equivalence with FplNetwork.infer (flypylib/fplnetwork.py:146-187): with an output
// tile edge that is a multiple of the network stride 4 (88 = 4 * 22 for vgg_like, 80 = 4 * 20
// for vgg_like2) every reference tile's input origin is a multiple of 4, so the coarse grid is
// anchored at the volume origin: pred[off + p] = O[p / 4] with O[i] seeing input
// [4i, 4i + 4 + 2 off), zero (normalised) past the volume end - independent of the tiling.
// `off` is the network's border, 7 for vgg_like and 10 for vgg_like2.  The kernels compute O
// directly, over the coarse rows [cz_lo, cz_hi) that a slab of tile rows owns, in chunks of
// rows sized by a scratch budget.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

// What the tile rows [zb, ze) of the reference lattice mean for a network with border `off`.
struct VggSlab {
  int64_t VZ, VY, VX;      // valid (predicted) extent of the volume
  int64_t fz_hi;           // end of the slab's fine output rows, clipped to VZ
  int64_t cz_lo, cz_hi;    // coarse rows the slab owns
  int CY, CX;              // coarse extent in y and x
  bool empty;              // no valid output voxel: nothing to run
};

static inline VggSlab vgg_slab(const int64_t dims[3], const std::vector<int32_t> &origins_z,
                               int32_t out_sz_z, int32_t zb, int32_t ze, int off) {
  VggSlab s = {};
  s.VZ = dims[0] - 2 * off; s.VY = dims[1] - 2 * off; s.VX = dims[2] - 2 * off;
  s.empty = s.VZ <= 0 || s.VY <= 0 || s.VX <= 0 || zb >= ze;
  if (s.empty) return s;
  const int64_t fz_lo = (int64_t)origins_z[zb] - off;
  s.fz_hi = std::min<int64_t>((int64_t)origins_z[ze - 1] - off + out_sz_z, s.VZ);
  s.cz_lo = fz_lo / 4; s.cz_hi = (s.fz_hi + 3) / 4;
  s.CY = (int)((s.VY + 3) / 4); s.CX = (int)((s.VX + 3) / 4);
  return s;
}

// The intermediate tensors of C coarse outputs along one axis.  vgg_like: P2 (quarter
// resolution, one 3-wide convolution above the head) and P1 (half resolution).
struct VggPyramid {
  int P2, P1;
  explicit VggPyramid(int64_t C) : P2((int)C + 2), P1(2 * P2 + 2) {}
};
// vgg_like2: Q (quarter resolution), L3 (T3, half resolution) and H1 (H, half resolution, one
// more 3-wide convolution below L3).
struct Vgg2Pyramid {
  int Q, T3, H;
  explicit Vgg2Pyramid(int64_t C) : Q((int)C + 2), T3(2 * Q + 2), H(T3 + 2) {}
};

// Coarse rows per chunk: the half-resolution tensors of a chunk of c rows have
// 2 c + fixed_rows rows (fixed_rows = the pyramid of 0 rows: 6 for P1, 8 for H1) of
// bytes_per_fine_row each and must fit the budget; at least 4, at most the slab's `span`,
// rounded up to the 4 rows of a head block, then clipped to `cap` (a multiple of 4; 0: none).
static inline int64_t vgg_chunk_rows(int64_t budget_bytes, int64_t bytes_per_fine_row,
                                     int fixed_rows, int64_t span, int64_t cap = 0) {
  int64_t c = std::max<int64_t>(4, (budget_bytes / bytes_per_fine_row - fixed_rows) / 2);
  c = std::min<int64_t>(c, span);
  c = (c + 3) / 4 * 4;
  return cap ? std::min<int64_t>(c, cap) : c;
}

// Split vgg_like only: the tile loads address a pass's hi AND lo plane (16 B per voxel each)
// from one scalar base with 32-bit lane offsets, so two part planes of a chunk's P1 plus the
// tile's reach (tile_z + 2 rows) stay below 4 GiB.  The P1 rows that allows ...
static inline int64_t vgg_split_max_p1_rows(int P1Y, int P1X, int tile_z) {
  return ((int64_t)1 << 32) / 16 / ((int64_t)P1Y * P1X) - (tile_z + 2);
}
// ... and the chunk cap that follows (the caller requires max_rows >= 14 first).
static inline int64_t vgg_split_chunk_cap(int64_t max_rows) {
  return std::max<int64_t>(4, ((max_rows - VggPyramid(0).P1) / 2) / 4 * 4);
}

// ---- Split vgg_like, the mid kernel (conv3 + conv1 + pool: P1 -> P2): block orientations ----
// A block is 8 waves x 4 sub-steps x 16 lanes = 512 pre-pool outputs (64 pooled voxels) on a tile
// of P1 in LDS.  The interior orientation lays that out as 8 z x 4 y x 16 x.  Where P2 cuts the
// last block column (x) or layer (z), most of such a block's lanes or waves hold no P2 voxel, and
// the cut region is walked in an orientation whose SHORT axis is the cut one instead:
//   MID_XCOL    8 z x 16 y x 4 x   lanes along y, sub-steps the (dz, dx) window, lane pair pools y
//   MID_ZLAYER  4 z x 8 y x 16 x   waves along (z 2, y 4), sub-steps and lanes as in the interior
// Only WHICH wave, sub-step and lane computes a voxel changes: the taps keep their numbering
// (tap = (dz * 3 + dy) * 3 + dx) and with it every voxel its sequence of MFMAs.
// (Plain constexpr functions: the kernels and the host compiler's tests share them.)
enum { MID_INTERIOR = 0, MID_XCOL = 1, MID_ZLAYER = 2 };

struct MidGeo {
  int BZ, BY, BX;          // pre-pool outputs of a block; its tile is (BZ + 2) x (BY + 2) x (BX + 2)
  int ZS;                  // LDS slots between z planes of the tile (rows are BX + 2 slots apart)
  constexpr int TZ() const { return BZ + 2; }
  constexpr int TY() const { return BY + 2; }
  constexpr int TX() const { return BX + 2; }
  constexpr int slots() const { return (TZ() - 1) * ZS + TY() * TX(); }
  constexpr int slot(int tz, int ty, int tx) const { return tz * ZS + ty * TX() + tx; }
};
// (z strides: the interior's 118 is padded for conflict-free taps, vgg_split_lds.h; 182 likewise -
// 182 - 2 * 18 - 2 = 144 = 0 mod 16; the x column's lanes are a row of 6 slots apart whatever the
// padding, and 7 does not fit the tile's 1170 slots)
constexpr MidGeo mid_geo(int o) {
  return o == MID_XCOL ? MidGeo{8, 16, 4, 108} : o == MID_ZLAYER ? MidGeo{4, 8, 16, 182} : MidGeo{8, 4, 16, 118};
}

struct MidVox { int z, y, x; };
// the pre-pool output, relative to its block, of wave `wave`, sub-step `sub`, lane column `c`
// (= lane & 15).  Sub-step 0 of an even c is the even corner of a pooled voxel; its 2 x 2 x 2 window
// is the four sub-steps of lanes c and c + 1.
constexpr MidVox mid_voxel(int o, int wave, int sub, int c) {
  return o == MID_XCOL     ? MidVox{2 * (wave >> 1) + (sub >> 1), c, 2 * (wave & 1) + (sub & 1)}
         : o == MID_ZLAYER ? MidVox{2 * (wave >> 2) + (sub >> 1), 2 * (wave & 3) + (sub & 1), c}
                           : MidVox{2 * (wave >> 1) + (sub >> 1), 2 * (wave & 1) + (sub & 1), c};
}
// the tile voxel that LDS slot `s` of a part plane holds; the padding between z planes and the slots
// behind the tile repeat a voxel of the tile (loaded, never read)
constexpr MidVox mid_slot_voxel(const MidGeo &g, int s) {
  const int tz = s / g.ZS < g.TZ() ? s / g.ZS : g.TZ() - 1;
  const int rem = s - tz * g.ZS < g.TY() * g.TX() ? s - tz * g.ZS : g.TY() * g.TX() - 1;
  return MidVox{tz, rem / g.TX(), rem % g.TX()};
}
// slot offset of tap 0 .. 26 from an output voxel's own slot
constexpr int mid_tap_slot(const MidGeo &g, int tap) { return g.slot(tap / 9, (tap / 3) % 3, tap % 3); }

// The launches of the mid kernel over a P2 of (Z, Y, X) pooled voxels: per orientation a grid of
// nbx x nby x nbz blocks whose first block starts at pre-pool (z0, 0, x0).  The interior launch
// gives up its cut column / layer when the other orientation covers it in FEWER blocks (the
// corner goes with the x column); an orientation with no block is not launched.
struct MidWalk {
  int nbx, nby, nbz;
  int z0, x0;
  constexpr int64_t blocks() const { return (int64_t)nbx * nby * nbz; }
};
struct MidPlan { MidWalk w[3]; };

static inline MidPlan vgg_mid_plan(int Z, int Y, int X, bool reorient) {
  auto cdiv = [](int a, int b) { return (a + b - 1) / b; };
  const MidGeo gi = mid_geo(MID_INTERIOR), gx = mid_geo(MID_XCOL), gz = mid_geo(MID_ZLAYER);
  MidPlan p = {};
  MidWalk &in = p.w[MID_INTERIOR], &xc = p.w[MID_XCOL], &zl = p.w[MID_ZLAYER];
  in = MidWalk{cdiv(2 * X, gi.BX), cdiv(2 * Y, gi.BY), cdiv(2 * Z, gi.BZ), 0, 0};
  if (!reorient) return p;
  const int live_x = 2 * X % gi.BX, live_z = 2 * Z % gi.BZ;         // pre-pool extent of the cut column / layer
  if (live_x) {
    const MidWalk c = {cdiv(live_x, gx.BX), cdiv(2 * Y, gx.BY), cdiv(2 * Z, gx.BZ), 0, (in.nbx - 1) * gi.BX};
    if (c.blocks() < (int64_t)in.nby * in.nbz) { xc = c; --in.nbx; }
  }
  if (live_z && in.nbx) {
    const MidWalk c = {in.nbx, cdiv(2 * Y, gz.BY), cdiv(live_z, gz.BZ), (in.nbz - 1) * gi.BZ, 0};
    if (c.blocks() < (int64_t)in.nbx * in.nby) { zl = c; --in.nbz; }
  }
  return p;
}
