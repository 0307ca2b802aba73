// libfplmatch.so (include/fplmatch.h): the table of (prediction, ground-truth) pairs closer
// than the match threshold, for the sparse obj_pr / obj_pr_curve.
//
// Every pair is tested: 10^5 x 10^5 points are 10^10 tests of 8 float64 operations and a
// compare, with nothing to sort or bin first (DESIGN.md section 13 has the measured time).
//
//   count_kernel  a thread owns one prediction, a block FPLE_BLOCK of them; blockIdx.y is
//                 the segment of the ground-truth range the block walks.  The block copies
//                 FPLE_TILE points (768 doubles, 6 KiB) into LDS with three coalesced loads
//                 per thread, then every thread reads the tile point by point - all lanes the
//                 same address, a broadcast read without bank conflicts - and tests it.  One
//                 uint32 per (prediction, segment) cell, prediction-major; an empty segment
//                 writes its zeros.
//   (scan)        side_scan_kernel of csrc/side/side_device.h; the uint64 total sits in front.
//   fill_kernel   the count pass again; a thread writes its rows from its cell's offset in
//                 ascending j.  Cells are prediction-major and segments ascend in j, so the
//                 table is in (i, j) order whatever order the blocks run in.  No atomics.
//
// The squared distance is side_device.h's side_dist2: numpy's (delta ** 2).sum(axis=2) to the bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "fplmatch.h"
#include "../side/side_abi.h"
#include "../side/side_device.h"

// this library's spelling of the shared shell
#define FPLE_EXPORT SIDE_EXPORT
#define FPLE_CATCH() SIDE_CATCH()
#define fple_fail side_fail

namespace {

constexpr int BLOCK = FPLE_BLOCK;
constexpr int TILE = FPLE_TILE;
static_assert(FPLE_SCAN_THREADS == SIDE_SCAN_THREADS, "the scan is side_scan_kernel's block");
static_assert(TILE == BLOCK, "a thread loads three doubles of a tile");

struct Points {
  const double *pred, *gt;      // rows of (x, y, z)
  uint32_t n_pred, n_gt;
  uint32_t segments;            // G
  uint32_t seg_len;             // ground-truth points per segment, whole tiles
  double T2;
};

// the pairs of prediction i within segment blockIdx.y: counted, and with FILL written from `row`
template <bool FILL>
__device__ __forceinline__ uint32_t walk_segment(const Points &p, double *tile, uint32_t row,
                                                 uint32_t capacity, int32_t *__restrict__ i_out,
                                                 int32_t *__restrict__ j_out) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  const bool live = i < p.n_pred;
  double px = 0.0, py = 0.0, pz = 0.0;
  if (live) {
    const double *q = p.pred + (size_t)i * 3;
    px = q[0]; py = q[1]; pz = q[2];
  }
  const uint64_t first = (uint64_t)blockIdx.y * p.seg_len;            // block-uniform
  const uint32_t j1 = (uint32_t)std::min<uint64_t>(first + p.seg_len, p.n_gt);
  uint32_t count = 0;
  for (uint64_t t64 = first; t64 < j1; t64 += TILE) {
    const uint32_t t = (uint32_t)t64;
    const uint32_t n = std::min<uint32_t>(TILE, j1 - t);              // points of this tile
    const double *src = p.gt + (size_t)t * 3;
    __syncthreads();                                                  // the tile before is read
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const uint32_t k = threadIdx.x + e * BLOCK;
      if (k < 3 * n) tile[k] = src[k];
    }
    __syncthreads();
    for (uint32_t k = 0; k < n; ++k) {
      const double s = side_dist2(px, py, pz, tile[3 * k], tile[3 * k + 1], tile[3 * k + 2]);
      if (live && s <= p.T2) {
        if (FILL) {
          if (row < capacity) {
            i_out[row] = (int32_t)i;
            j_out[row] = (int32_t)(t + k);
          }
          ++row;
        }
        ++count;
      }
    }
  }
  return count;
}

__global__ __launch_bounds__(BLOCK) void count_kernel(Points p, uint32_t *__restrict__ cells) {
  __shared__ double tile[3 * TILE];
  const uint32_t count = walk_segment<false>(p, tile, 0u, 0u, nullptr, nullptr);
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i < p.n_pred) cells[(size_t)i * p.segments + blockIdx.y] = count;
}

__global__ __launch_bounds__(BLOCK) void fill_kernel(Points p, const uint32_t *__restrict__ offsets,
                                                     uint32_t capacity, int32_t *__restrict__ i_out,
                                                     int32_t *__restrict__ j_out) {
  __shared__ double tile[3 * TILE];
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  const uint32_t row = i < p.n_pred ? offsets[(size_t)i * p.segments + blockIdx.y] : 0u;
  walk_segment<true>(p, tile, row, capacity, i_out, j_out);
}

// G of the header
uint32_t segments_of(int64_t n_pred, int64_t n_gt) {
  const int64_t blocks = (n_pred + BLOCK - 1) / BLOCK, tiles = (n_gt + TILE - 1) / TILE;
  const int64_t want = std::min(tiles, (FPLE_TARGET_BLOCKS + blocks - 1) / blocks);
  uint32_t g = 1;
  while (g < want && g < FPLE_MAX_SEGMENTS) g <<= 1;
  return g;
}

int counts_ok(const char *fn, int64_t n_pred, int64_t n_gt) {
  if (in_int32_range(fn, "n_pred", n_pred, 1) || in_int32_range(fn, "n_gt", n_gt, 1)) return 1;
  // more than FPLE_TARGET_BLOCKS blocks of predictions are one segment, so this holds for
  // every n_pred: 2^31 - 1 cells at the most
  if (n_pred * (int64_t)segments_of(n_pred, n_gt) > SIDE_INT32_MAX)
    return fple_fail("%s: %lld predictions in %u segments exceed 2^31 - 1 cells", fn,
                     (long long)n_pred, segments_of(n_pred, n_gt));
  return 0;
}

int64_t scratch_for(int64_t n_pred, int64_t n_gt) {
  return 8 + 4 * n_pred * (int64_t)segments_of(n_pred, n_gt);
}

int pair_args(const char *fn, const double *pred, int64_t n_pred, const double *gt, int64_t n_gt,
              double T2, const void *scratch, int64_t scratch_bytes, Points *p) {
  if (!pred || !gt || !scratch) return fple_fail("%s: null pointer argument", fn);
  if (counts_ok(fn, n_pred, n_gt)) return 1;
  if (!(std::isfinite(T2) && T2 > 0.0))
    return fple_fail("%s: T2 %g must be finite and positive", fn, T2);
  if (!aligned(pred, 8) || !aligned(gt, 8))
    return fple_fail("%s: the point tables are not aligned to a double", fn);
  if (!aligned(scratch, 8) || scratch_bytes < scratch_for(n_pred, n_gt))
    return fple_fail("%s: scratch of %lld bytes, fple_scratch_bytes asks for %lld (8-byte aligned)",
                     fn, (long long)scratch_bytes, (long long)scratch_for(n_pred, n_gt));
  p->pred = pred;
  p->gt = gt;
  p->n_pred = (uint32_t)n_pred;
  p->n_gt = (uint32_t)n_gt;
  p->segments = segments_of(n_pred, n_gt);
  const int64_t tiles = (n_gt + TILE - 1) / TILE;
  p->seg_len = (uint32_t)((tiles + p->segments - 1) / p->segments * TILE);   // <= n_gt + 255
  p->T2 = T2;
  return 0;
}

dim3 grid_of(const Points &p) { return dim3((p.n_pred + BLOCK - 1) / BLOCK, p.segments); }

}  // namespace

FPLE_EXPORT const char *fple_last_error(void) try {
  return side_err;
} catch (...) { return "fple_last_error: C++ exception"; }

FPLE_EXPORT int fple_abi_version(void) try {
  return FPLE_ABI_VERSION;
} FPLE_CATCH()

FPLE_EXPORT int fple_scratch_bytes(int64_t n_pred, int64_t n_gt, int64_t *bytes) try {
  if (!bytes) return fple_fail("fple_scratch_bytes: null pointer argument");
  if (counts_ok("fple_scratch_bytes", n_pred, n_gt)) return 1;
  *bytes = scratch_for(n_pred, n_gt);
  return 0;
} FPLE_CATCH()

FPLE_EXPORT int fple_pairs_count(const double *pred, int64_t n_pred, const double *gt,
                                 int64_t n_gt, double T2, void *scratch, int64_t scratch_bytes,
                                 int64_t *total, void *stream) try {
  const char *fn = "fple_pairs_count";
  Points p;
  if (!total) return fple_fail("%s: null pointer argument", fn);
  if (pair_args(fn, pred, n_pred, gt, n_gt, T2, scratch, scratch_bytes, &p)) return 1;
  unsigned long long *sum = (unsigned long long *)scratch;
  uint32_t *cells = (uint32_t *)((char *)scratch + 8);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(count_kernel, grid_of(p), dim3(BLOCK), 0, st, p, cells);
  if (launched("fple_pairs_count")) return 1;
  hipLaunchKernelGGL(side_scan_kernel<uint32_t>, dim3(1), dim3(SIDE_SCAN_THREADS), 0, st, cells,
                     p.n_pred * p.segments, sum, nullptr);
  if (launched("fple_pairs_count (scan)")) return 1;
  unsigned long long got = 0;
  if (side_read_back(fn, st, &got, sum, sizeof(got))) return 1;
  if (got > (unsigned long long)SIDE_INT32_MAX)
    return fple_fail("%s: %llu pairs exceed the 2^31 - 1 rows of an int32 table; match the points "
                     "in parts", fn, got);
  *total = (int64_t)got;
  return 0;
} FPLE_CATCH()

FPLE_EXPORT int fple_pairs_fill(const double *pred, int64_t n_pred, const double *gt, int64_t n_gt,
                                double T2, const void *scratch, int64_t scratch_bytes,
                                int64_t capacity, int32_t *i_out, int32_t *j_out,
                                void *stream) try {
  const char *fn = "fple_pairs_fill";
  Points p;
  if (pair_args(fn, pred, n_pred, gt, n_gt, T2, scratch, scratch_bytes, &p)) return 1;
  if (in_int32_range(fn, "capacity", capacity, 0)) return 1;
  if (capacity == 0) return 0;
  if (!i_out || !j_out) return fple_fail("%s: null pointer argument (an output column)", fn);
  if (!aligned(i_out, 4) || !aligned(j_out, 4))
    return fple_fail("%s: an output column is not 4-byte aligned", fn);
  const uint32_t *offsets = (const uint32_t *)((const char *)scratch + 8);
  hipLaunchKernelGGL(fill_kernel, grid_of(p), dim3(BLOCK), 0, (hipStream_t)stream, p, offsets,
                     (uint32_t)capacity, i_out, j_out);
  return launched(fn);
} FPLE_CATCH()
