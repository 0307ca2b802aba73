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
//   scan_kernel   one block of FPLE_SCAN_THREADS threads: each thread sums a run of
//                 consecutive cells, the sums (uint64) are scanned in LDS, each thread rewrites
//                 its run as exclusive offsets; the total is kept as a uint64 in front of the
//                 cells, so a table beyond int32 rows is seen and refused, not wrapped.
//   fill_kernel   the count pass again; a thread writes its rows from its cell's offset in
//                 ascending j.  Cells are prediction-major and segments ascend in j, so the
//                 table is in (i, j) order whatever order the blocks run in.  No atomics.
//
// s = (dx * dx + dy * dy) + dz * dz with every operation rounded on its own: the library is
// built with -ffp-contract=on, so dist2() switches contraction off and spells the operations
// as __dmul_rn / __dadd_rn.  That is numpy's (delta ** 2).sum(axis=2), bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "fplmatch.h"
#include "../side/side_abi.h"

// this library's spelling of the shared shell
#define FPLE_EXPORT SIDE_EXPORT
#define FPLE_CATCH() SIDE_CATCH()
#define fple_fail side_fail

namespace {

constexpr int BLOCK = FPLE_BLOCK;
constexpr int TILE = FPLE_TILE;
constexpr int SCAN_THREADS = FPLE_SCAN_THREADS;
constexpr int64_t LIMIT = 2147483647;
static_assert(TILE == BLOCK, "a thread loads three doubles of a tile");

struct Points {
  const double *pred, *gt;      // rows of (x, y, z)
  uint32_t n_pred, n_gt;
  uint32_t segments;            // G
  uint32_t seg_len;             // ground-truth points per segment, whole tiles
  double T2;
};

__device__ __forceinline__ double dist2(double px, double py, double pz, double gx, double gy,
                                        double gz) {
#pragma clang fp contract(off)
  const double dx = px - gx, dy = py - gy, dz = pz - gz;
  return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

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
      const double s = dist2(px, py, pz, tile[3 * k], tile[3 * k + 1], tile[3 * k + 2]);
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

// cells[0 .. n) -> exclusive offsets in place (mod 2^32: only a total within int32 rows is
// used), *total = their sum
__global__ __launch_bounds__(SCAN_THREADS) void scan_kernel(uint32_t *__restrict__ cells,
                                                            uint32_t n,
                                                            unsigned long long *__restrict__ total) {
  __shared__ unsigned long long sums[SCAN_THREADS];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (n + SCAN_THREADS - 1) / SCAN_THREADS;
  const uint32_t lo = (uint32_t)std::min<uint64_t>((uint64_t)t * per, n);
  const uint32_t hi = (uint32_t)std::min<uint64_t>((uint64_t)lo + per, n);
  unsigned long long own = 0;
  for (uint32_t j = lo; j < hi; ++j) own += cells[j];
  sums[t] = own;
  __syncthreads();
  for (uint32_t off = 1; off < SCAN_THREADS; off <<= 1) {
    const unsigned long long v = t >= off ? sums[t - off] : 0ull;
    __syncthreads();
    sums[t] += v;
    __syncthreads();
  }
  uint32_t run = (uint32_t)(sums[t] - own);
  for (uint32_t j = lo; j < hi; ++j) {
    const uint32_t v = cells[j];
    cells[j] = run;
    run += v;
  }
  if (t == SCAN_THREADS - 1) *total = sums[t];
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
  if (n_pred < 1 || n_pred > LIMIT)
    return fple_fail("%s: n_pred %lld must lie in [1, 2^31 - 1]", fn, (long long)n_pred);
  if (n_gt < 1 || n_gt > LIMIT)
    return fple_fail("%s: n_gt %lld must lie in [1, 2^31 - 1]", fn, (long long)n_gt);
  // more than FPLE_TARGET_BLOCKS blocks of predictions are one segment, so this holds for
  // every n_pred: 2^31 - 1 cells at the most
  if (n_pred * (int64_t)segments_of(n_pred, n_gt) > LIMIT)
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
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, cells,
                     p.n_pred * p.segments, sum);
  if (launched("fple_pairs_count (scan)")) return 1;
  unsigned long long got = 0;
  hipError_t e = hipMemcpyAsync(&got, sum, sizeof(got), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess)
    return fple_fail("%s: reading the total failed: %s", fn, hipGetErrorString(e));
  if (got > (unsigned long long)LIMIT)
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
  if (capacity < 0 || capacity > LIMIT)
    return fple_fail("%s: capacity %lld must lie in [0, 2^31 - 1]", fn, (long long)capacity);
  if (capacity == 0) return 0;
  if (!i_out || !j_out) return fple_fail("%s: null pointer argument (an output column)", fn);
  if (!aligned(i_out, 4) || !aligned(j_out, 4))
    return fple_fail("%s: an output column is not 4-byte aligned", fn);
  const uint32_t *offsets = (const uint32_t *)((const char *)scratch + 8);
  hipLaunchKernelGGL(fill_kernel, grid_of(p), dim3(BLOCK), 0, (hipStream_t)stream, p, offsets,
                     (uint32_t)capacity, i_out, j_out);
  return launched(fn);
} FPLE_CATCH()
