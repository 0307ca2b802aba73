// libfplnear.so (include/fplnear.h): the close pairs within one point set, as a CSR table, for
// fplsynapses.rm_tbar_multi_pred.
//
// A self-join of N points is N^2 tests if every pair is tried; binned into cells of about the
// threshold it is N times the points of 27 cells.  The caller sorts the cell keys between the
// first kernel and the rest (DESIGN.md section 14 has the measured times).
//
//   keys_kernel    a thread owns one point: its cell along each axis, the key
//                  (cz * ny + cy) * nx + cx.
//   gather_kernel  the points and their indices (as int32) in key order, into the scratch: a
//                  wavefront's points then share their cells and the candidates of a run are read
//                  from consecutive addresses.  An entry of the order outside [0, n) raises the
//                  status word and is read as 0.
//   count_kernel   a thread owns one point of that order.  For each of the 9 (dy, dz) neighbours
//                  the three x-adjacent cells are one key range: two binary searches in the
//                  sorted keys give a run of candidates [lo, hi).  The 18 bounds live in LDS, a
//                  column per thread (the loops over them are not unrolled, so in registers they
//                  would be indexed dynamically and go to scratch).  Every candidate is tested;
//                  the count goes to the point's ORIGINAL index.
//   (scan)         side_scan_kernel of csrc/side/side_device.h; the total as a uint64 in front
//                  and as the last of the n + 1 row offsets.
//   fill_kernel    the count pass again.  The candidates come in cell order, not in ascending j,
//                  and a row may be longer than any per-thread buffer, so a partner is placed by
//                  rank: it goes to the row's offset plus the number of the row's partners with a
//                  smaller index, found by walking the runs a second time.  That is
//                  (partners) x (candidates) tests per point instead of (candidates) - a handful
//                  of partners against some tens of candidates at T-bar densities - and needs no
//                  buffer, no second table and no atomics: every entry has one writer and one
//                  place, whatever order the blocks run in.
//
// The squared distance is side_device.h's side_dist2, every operation rounded on its own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "fplnear.h"
#include "../side/side_abi.h"
#include "../side/side_device.h"

// this library's spelling of the shared shell
#define FPLN_EXPORT SIDE_EXPORT
#define FPLN_CATCH() SIDE_CATCH()
#define fpln_fail side_fail

namespace {

constexpr int BLOCK = FPLN_BLOCK;
static_assert(FPLN_SCAN_THREADS == SIDE_SCAN_THREADS, "the scan is side_scan_kernel's block");
constexpr int64_t MAX_AXIS = (int64_t)1 << FPLN_MAX_AXIS_BITS;
constexpr int RUNS = 9;                     // the (dy, dz) neighbours of a cell row

struct Grid {
  double ox, oy, oz, cell;
  int64_t nx, ny, nz;
};

// the scratch of fpln_pairs_count / _fill
struct Scratch {
  unsigned long long *total;                // [0, 8)
  uint32_t *status;                         // [8, 12): 1 = an entry of `order` outside [0, n)
  uint32_t *offsets;                        // at 16: n + 1, counts before the scan
  uint32_t *perm;                           // n: original index of the k-th point in key order
  double *pts;                              // 3 n: the points in key order
};

int64_t pad8(int64_t b) { return (b + 7) & ~(int64_t)7; }

int64_t scratch_for(int64_t n) { return 16 + pad8(4 * (n + 1)) + pad8(4 * n) + 24 * n; }

Scratch carve(void *scratch, int64_t n) {
  char *b = (char *)scratch;
  Scratch s;
  s.total = (unsigned long long *)b;
  s.status = (uint32_t *)(b + 8);
  s.offsets = (uint32_t *)(b + 16);
  s.perm = (uint32_t *)(b + 16 + pad8(4 * (n + 1)));
  s.pts = (double *)(b + 16 + pad8(4 * (n + 1)) + pad8(4 * n));
  return s;
}

struct Near {
  Grid g;
  const int64_t *keys;                      // sorted
  const uint32_t *perm;
  const double *pts;
  uint32_t n;
  double T2;
};

__device__ __forceinline__ int64_t cell_of(double x, double o, double cell, int64_t n) {
#pragma clang fp contract(off)
  double u = (x - o) / cell;
  u = fmin(fmax(u, 0.0), (double)(n - 1));  // a NaN reads as 0
  return (int64_t)floor(u);
}

__global__ __launch_bounds__(BLOCK) void keys_kernel(const double *__restrict__ locs, uint32_t n,
                                                     Grid g, int64_t *__restrict__ keys) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const double *q = locs + (size_t)i * 3;
  const int64_t cx = cell_of(q[0], g.ox, g.cell, g.nx), cy = cell_of(q[1], g.oy, g.cell, g.ny),
                cz = cell_of(q[2], g.oz, g.cell, g.nz);
  keys[i] = (cz * g.ny + cy) * g.nx + cx;
}

__global__ __launch_bounds__(BLOCK) void gather_kernel(const double *__restrict__ locs, uint32_t n,
                                                       const int64_t *__restrict__ order,
                                                       uint32_t *__restrict__ perm,
                                                       double *__restrict__ pts,
                                                       uint32_t *__restrict__ status) {
  const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
  if (k >= n) return;
  uint64_t j = (uint64_t)order[k];
  if (j >= n) {
    *status = 1u;                           // every writer writes the same word
    j = 0;
  }
  perm[k] = (uint32_t)j;
  const double *q = locs + (size_t)j * 3;
  double *d = pts + (size_t)k * 3;
  d[0] = q[0]; d[1] = q[1]; d[2] = q[2];
}

// the first position in keys[lo, n) whose key is not below k
__device__ __forceinline__ uint32_t lower_bound(const int64_t *__restrict__ keys, uint32_t lo,
                                                uint32_t n, int64_t k) {
  uint32_t hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the candidate runs of the point (px, py, pz): runs[2 r] <= q < runs[2 r + 1], r < RUNS, in
// the calling thread's column of `runs`
__device__ __forceinline__ void find_runs(const Near &a, double px, double py, double pz,
                                          uint32_t (*runs)[BLOCK]) {
  const Grid &g = a.g;
  const int64_t cx = cell_of(px, g.ox, g.cell, g.nx), cy = cell_of(py, g.oy, g.cell, g.ny),
                cz = cell_of(pz, g.oz, g.cell, g.nz);
  const int64_t x0 = cx > 0 ? cx - 1 : 0, x1 = cx + 1 < g.nx ? cx + 1 : g.nx - 1;
#pragma unroll 1
  for (int r = 0; r < RUNS; ++r) {
    const int64_t y = cy + (r % 3 - 1), z = cz + (r / 3 - 1);
    uint32_t lo = 0, hi = 0;
    if (y >= 0 && y < g.ny && z >= 0 && z < g.nz) {
      const int64_t row = (z * g.ny + y) * g.nx;
      lo = lower_bound(a.keys, 0u, a.n, row + x0);
      hi = lower_bound(a.keys, lo, a.n, row + x1 + 1);
    }
    runs[2 * r][threadIdx.x] = lo;
    runs[2 * r + 1][threadIdx.x] = hi;
  }
}

__device__ __forceinline__ bool partner(const Near &a, double px, double py, double pz, uint32_t q) {
  const double *c = a.pts + (size_t)q * 3;
  const double s = side_dist2(px, py, pz, c[0], c[1], c[2]);
  return s > 0.0 && s <= a.T2;
}

__global__ __launch_bounds__(BLOCK) void count_kernel(Near a, uint32_t *__restrict__ counts) {
  __shared__ uint32_t runs[2 * RUNS][BLOCK];
  const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
  if (k >= a.n) return;                     // no barrier below: a thread reads its own column
  const double px = a.pts[(size_t)k * 3], py = a.pts[(size_t)k * 3 + 1],
               pz = a.pts[(size_t)k * 3 + 2];
  find_runs(a, px, py, pz, runs);
  uint32_t count = 0;
#pragma unroll 1
  for (int r = 0; r < RUNS; ++r) {
    const uint32_t hi = runs[2 * r + 1][threadIdx.x];
    for (uint32_t q = runs[2 * r][threadIdx.x]; q < hi; ++q)
      count += partner(a, px, py, pz, q) ? 1u : 0u;
  }
  counts[a.perm[k]] = count;
}

__global__ __launch_bounds__(BLOCK) void fill_kernel(Near a, const uint32_t *__restrict__ offsets,
                                                     uint32_t capacity,
                                                     int32_t *__restrict__ indices) {
  __shared__ uint32_t runs[2 * RUNS][BLOCK];
  const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
  if (k >= a.n) return;
  const double px = a.pts[(size_t)k * 3], py = a.pts[(size_t)k * 3 + 1],
               pz = a.pts[(size_t)k * 3 + 2];
  find_runs(a, px, py, pz, runs);
  const uint32_t first = offsets[std::min(a.perm[k], a.n - 1)];
#pragma unroll 1
  for (int r = 0; r < RUNS; ++r) {
    const uint32_t hi = runs[2 * r + 1][threadIdx.x];
    for (uint32_t q = runs[2 * r][threadIdx.x]; q < hi; ++q) {
      if (!partner(a, px, py, pz, q)) continue;
      const uint32_t j = a.perm[q];
      uint32_t rank = 0;                    // the partners of this row below j
#pragma unroll 1
      for (int r2 = 0; r2 < RUNS; ++r2) {
        const uint32_t hi2 = runs[2 * r2 + 1][threadIdx.x];
        for (uint32_t q2 = runs[2 * r2][threadIdx.x]; q2 < hi2; ++q2)
          rank += (a.perm[q2] < j && partner(a, px, py, pz, q2)) ? 1u : 0u;
      }
      const uint32_t at = first + rank;     // both below 2^31
      if (at < capacity) indices[at] = (int32_t)j;
    }
  }
}

int count_ok(const char *fn, int64_t n) { return in_int32_range(fn, "n", n, 1); }

int grid_args(const char *fn, const double *origin, double cell, const int64_t *dims, Grid *g) {
  if (!origin || !dims) return fpln_fail("%s: null pointer argument (the grid)", fn);
  if (!(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2])))
    return fpln_fail("%s: the grid's origin is not finite", fn);
  if (!(std::isfinite(cell) && cell > 0.0))
    return fpln_fail("%s: cell side %g must be finite and positive", fn, cell);
  for (int a = 0; a < 3; ++a)
    if (dims[a] < 1 || dims[a] > MAX_AXIS)
      return fpln_fail("%s: %lld cells along axis %d, must lie in [1, 2^%d]; the points are "
                       "spread too far for this threshold", fn, (long long)dims[a], a,
                       FPLN_MAX_AXIS_BITS);
  // nx * ny <= 2^56
  if (dims[0] * dims[1] > ((int64_t)1 << 62) / dims[2])
    return fpln_fail("%s: a grid of %lld x %lld x %lld cells exceeds the 2^62 an int64 key can "
                     "number; the points are spread too far for this threshold", fn,
                     (long long)dims[0], (long long)dims[1], (long long)dims[2]);
  g->ox = origin[0]; g->oy = origin[1]; g->oz = origin[2];
  g->cell = cell;
  g->nx = dims[0]; g->ny = dims[1]; g->nz = dims[2];
  return 0;
}

int pair_args(const char *fn, const double *locs, int64_t n, double T2, const double *origin,
              double cell, const int64_t *dims, const int64_t *sorted_keys, const int64_t *order,
              const void *scratch, int64_t scratch_bytes, Near *a) {
  if (!locs || !sorted_keys || !order || !scratch) return fpln_fail("%s: null pointer argument", fn);
  if (count_ok(fn, n)) return 1;
  if (!(std::isfinite(T2) && T2 > 0.0))
    return fpln_fail("%s: T2 %g must be finite and positive", fn, T2);
  if (grid_args(fn, origin, cell, dims, &a->g)) return 1;
  if (!(cell >= std::sqrt(T2) * (1.0 + 0x1p-20)))
    return fpln_fail("%s: cell side %.17g is below sqrt(T2) (1 + 2^-20) = %.17g: partners could "
                     "lie two cells apart", fn, cell, std::sqrt(T2) * (1.0 + 0x1p-20));
  if (!aligned(locs, 8) || !aligned(sorted_keys, 8) || !aligned(order, 8))
    return fpln_fail("%s: the points, keys or order are not 8-byte aligned", fn);
  if (!aligned(scratch, 8) || scratch_bytes < scratch_for(n))
    return fpln_fail("%s: scratch of %lld bytes, fpln_scratch_bytes asks for %lld (8-byte aligned)",
                     fn, (long long)scratch_bytes, (long long)scratch_for(n));
  const Scratch s = carve((void *)scratch, n);
  a->keys = sorted_keys;
  a->perm = s.perm;
  a->pts = s.pts;
  a->n = (uint32_t)n;
  a->T2 = T2;
  return 0;
}

dim3 grid_of(int64_t n) { return dim3((unsigned)((n + BLOCK - 1) / BLOCK)); }

}  // namespace

FPLN_EXPORT const char *fpln_last_error(void) try {
  return side_err;
} catch (...) { return "fpln_last_error: C++ exception"; }

FPLN_EXPORT int fpln_abi_version(void) try {
  return FPLN_ABI_VERSION;
} FPLN_CATCH()

FPLN_EXPORT int fpln_scratch_bytes(int64_t n, int64_t *bytes) try {
  if (!bytes) return fpln_fail("fpln_scratch_bytes: null pointer argument");
  if (count_ok("fpln_scratch_bytes", n)) return 1;
  *bytes = scratch_for(n);
  return 0;
} FPLN_CATCH()

FPLN_EXPORT int fpln_cell_keys(const double *locs, int64_t n, const double *origin, double cell,
                               const int64_t *dims, int64_t *keys, void *stream) try {
  const char *fn = "fpln_cell_keys";
  Grid g;
  if (!locs || !keys) return fpln_fail("%s: null pointer argument", fn);
  if (count_ok(fn, n)) return 1;
  if (grid_args(fn, origin, cell, dims, &g)) return 1;
  if (!aligned(locs, 8) || !aligned(keys, 8))
    return fpln_fail("%s: the points or keys are not 8-byte aligned", fn);
  hipLaunchKernelGGL(keys_kernel, grid_of(n), dim3(BLOCK), 0, (hipStream_t)stream, locs,
                     (uint32_t)n, g, keys);
  return launched(fn);
} FPLN_CATCH()

FPLN_EXPORT int fpln_pairs_count(const double *locs, int64_t n, double T2, const double *origin,
                                 double cell, const int64_t *dims, const int64_t *sorted_keys,
                                 const int64_t *order, void *scratch, int64_t scratch_bytes,
                                 int64_t *total, void *stream) try {
  const char *fn = "fpln_pairs_count";
  Near a;
  if (!total) return fpln_fail("%s: null pointer argument", fn);
  if (pair_args(fn, locs, n, T2, origin, cell, dims, sorted_keys, order, scratch, scratch_bytes, &a))
    return 1;
  const Scratch s = carve(scratch, n);
  hipStream_t st = (hipStream_t)stream;
  // the total, the status word and the counts: a point the order never names has an empty row
  hipError_t e = hipMemsetAsync(scratch, 0, (size_t)(16 + 4 * (n + 1)), st);
  if (e != hipSuccess) return fpln_fail("%s: clearing the scratch failed: %s", fn, hipGetErrorString(e));
  hipLaunchKernelGGL(gather_kernel, grid_of(n), dim3(BLOCK), 0, st, locs, a.n, order, s.perm, s.pts,
                     s.status);
  if (launched("fpln_pairs_count (gather)")) return 1;
  hipLaunchKernelGGL(count_kernel, grid_of(n), dim3(BLOCK), 0, st, a, s.offsets);
  if (launched("fpln_pairs_count")) return 1;
  hipLaunchKernelGGL(side_scan_kernel<uint32_t>, dim3(1), dim3(SIDE_SCAN_THREADS), 0, st, s.offsets,
                     a.n, s.total, s.offsets + a.n);
  if (launched("fpln_pairs_count (scan)")) return 1;
  unsigned long long head[2] = {0, 0};      // the total, the status word
  if (side_read_back(fn, st, head, scratch, sizeof(head))) return 1;
  if ((uint32_t)head[1] != 0)
    return fpln_fail("%s: an entry of the order lies outside [0, %lld)", fn, (long long)n);
  if (head[0] > (unsigned long long)SIDE_INT32_MAX)
    return fpln_fail("%s: %llu table entries exceed the 2^31 - 1 of an int32 table; merge the "
                     "points in parts", fn, head[0]);
  *total = (int64_t)head[0];
  return 0;
} FPLN_CATCH()

FPLN_EXPORT int fpln_pairs_fill(const double *locs, int64_t n, double T2, const double *origin,
                                double cell, const int64_t *dims, const int64_t *sorted_keys,
                                const int64_t *order, const void *scratch, int64_t scratch_bytes,
                                int64_t capacity, int32_t *indices, void *stream) try {
  const char *fn = "fpln_pairs_fill";
  Near a;
  if (pair_args(fn, locs, n, T2, origin, cell, dims, sorted_keys, order, scratch, scratch_bytes, &a))
    return 1;
  if (in_int32_range(fn, "capacity", capacity, 0)) return 1;
  if (capacity == 0) return 0;
  if (!indices) return fpln_fail("%s: null pointer argument (the column array)", fn);
  if (!aligned(indices, 4)) return fpln_fail("%s: the column array is not 4-byte aligned", fn);
  const Scratch s = carve((void *)scratch, n);
  hipLaunchKernelGGL(fill_kernel, grid_of(n), dim3(BLOCK), 0, (hipStream_t)stream, a, s.offsets,
                     (uint32_t)capacity, indices);
  return launched(fn);
} FPLN_CATCH()
