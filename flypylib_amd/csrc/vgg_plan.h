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
