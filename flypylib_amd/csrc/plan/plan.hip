// libfplplan.so (include/fplplan.h): the CSR brick table of the device write_labels_mask,
// built on the GPU from the resident T-bar list (labels.plan_bricks is the specification).
//
// Planning is integer work over (T-bar, brick) pairs: count, scan, scatter, order.  All of it
// runs on the caller's stream and nothing waits for the host.
//   (memset)          the brick counters (in `offsets`) and the brick cursors
//   count_kernel      one wave per T-bar: its lanes walk the T-bar's clamped brick range and
//                     add 1 to each brick's counter
//   tile_sum_kernel   a block of 1024 threads per tile of 1024 counters: the tile's sum
//   tile_scan_kernel  one block: side_scan_runs of csrc/side/side_device.h over the tile sums;
//                     the total goes behind the last brick and is compared with n_index for
//                     the status word
//   offsets_kernel    per tile: exclusive scan of its counters in LDS plus the tile's prefix,
//                     written over the counters
//   fill_kernel       the count pass again; a pair's place in the staging list is its brick's
//                     offset + what the brick's cursor returns
//   order_kernel      one wave per brick: each j of the brick's staged list goes to
//                     offsets[b] + the number of smaller j in the list
// The atomics (plain atomicAdd on int: vector atomics) only add integers, so the counters do
// not depend on the order of arrival; the cursors leave a brick's SET of j in an arbitrary
// order in the staging list, and order_kernel replaces that order by the ascending one: the j
// of a brick are distinct, so the rank of a j is its place.  The table is the same on every
// run.  fill_kernel and order_kernel do nothing when the status word is set, so a wrong
// n_index writes nothing into `index`; every store is bounded by n_index besides.
// Brick ids, counts and offsets are int32 (at most 2^31 - 2 bricks and 2^31 - 1 pairs are
// accepted); the sums of the scan are 64-bit, so a total beyond 2^32 cannot pass for n_index;
// byte offsets from the base pointers are formed in size_t.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fpllabels.h"
#include "fplplan.h"
#include "../side/side_abi.h"
#include "../side/side_device.h"

// this library's spelling of the shared shell
#define FPLP_EXPORT SIDE_EXPORT
#define FPLP_CATCH() SIDE_CATCH()
#define fplp_fail side_fail

static_assert(FPLP_BRICK_Z == FPLL_BRICK_Z && FPLP_BRICK_Y == FPLL_BRICK_Y &&
              FPLP_BRICK_X == FPLL_BRICK_X && FPLP_MAX_RADIUS == FPLL_MAX_RADIUS,
              "the planner's bricks are the labels kernel's");

namespace {

constexpr int BLOCK = 256;                 // 4 waves
constexpr int WAVE = 64;
constexpr int TILE = 1024;                 // counters per scan block, one per thread
static_assert(TILE == SIDE_SCAN_THREADS, "a tile is side_block_scan's block");
constexpr unsigned MAX_BLOCKS = 1u << 16;  // of BLOCK threads; more work goes by stride
constexpr unsigned MAX_TILE_BLOCKS = 1u << 13;
constexpr int BZ = FPLP_BRICK_Z, BY = FPLP_BRICK_Y, BX = FPLP_BRICK_X;

struct Plan {
  int nb0, nb1, nb2;        // bricks along z, y, x
  int half;
  unsigned n_tbars, n_bricks, n_index;
};

// the bricks of one T-bar: a box of c0 x c1 x c2 bricks from (lo0, lo1, lo2), n of them
struct Range {
  int lo0, lo1, lo2, c1, c2;
  unsigned n;
};

// lo = max((p - half) // b, 0) and the count up to min((p + half) // b, nb - 1), as plan_bricks
// forms them (floor division; p is any int32, so the sums are taken in 64 bits)
__device__ __forceinline__ void axis_range(int p, int half, int b, int nb, int &lo, int &cnt) {
  const long long v = (long long)p - half, w = (long long)p + half;
  lo = v < 0 ? 0 : (int)((unsigned)v / (unsigned)b);
  // nb - 1 <= (2^31 - 1) / b, so clamping w to 2^31 - 1 does not change the minimum
  const int hi =
      w < 0 ? -1 : min((int)((unsigned)min(w, 2147483647ll) / (unsigned)b), nb - 1);
  cnt = max(hi - lo + 1, 0);
}

__device__ __forceinline__ Range tbar_range(const int32_t *__restrict__ tbars, unsigned j,
                                            const Plan &p) {
  const int32_t *t = tbars + (size_t)j * 3;
  Range r;
  int c0;
  axis_range(t[2], p.half, BZ, p.nb0, r.lo0, c0);
  axis_range(t[1], p.half, BY, p.nb1, r.lo1, r.c1);
  axis_range(t[0], p.half, BX, p.nb2, r.lo2, r.c2);
  r.n = (unsigned)c0 * (unsigned)r.c1 * (unsigned)r.c2;      // <= n_bricks
  return r;
}

// the i-th brick of a range, i < r.n
__device__ __forceinline__ unsigned brick_of(const Range &r, unsigned i, const Plan &p) {
  const unsigned plane = (unsigned)r.c1 * (unsigned)r.c2;
  const unsigned iz = i / plane, rem = i - iz * plane;
  const unsigned iy = rem / (unsigned)r.c2, ix = rem - iy * (unsigned)r.c2;
  return (((unsigned)r.lo0 + iz) * (unsigned)p.nb1 + (unsigned)r.lo1 + iy) * (unsigned)p.nb2 +
         (unsigned)r.lo2 + ix;
}

__global__ __launch_bounds__(BLOCK) void count_kernel(const int32_t *__restrict__ tbars, Plan p,
                                                      int32_t *__restrict__ counts) {
  const unsigned lane = threadIdx.x & (WAVE - 1);
  const unsigned waves = gridDim.x * (BLOCK / WAVE);
  for (unsigned j = blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE; j < p.n_tbars; j += waves) {
    const Range r = tbar_range(tbars, j, p);
    for (unsigned i = lane; i < r.n; i += WAVE) {
      const unsigned b = brick_of(r, i, p);
      if (b < p.n_bricks) atomicAdd(&counts[b], 1);
    }
  }
}

__global__ __launch_bounds__(TILE) void tile_sum_kernel(const int32_t *__restrict__ counts,
                                                        unsigned n_bricks, unsigned tiles,
                                                        u64 *__restrict__ tile_sums) {
  __shared__ u64 sums[TILE];
  for (unsigned tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const unsigned i = tile * (unsigned)TILE + threadIdx.x;
    const u64 incl = side_block_scan(i < n_bricks ? (u64)(unsigned)counts[i] : 0ull, sums);
    if (threadIdx.x == TILE - 1) tile_sums[tile] = incl;
  }
}

// tile_sums[0 .. tiles) -> exclusive prefixes in place; the total behind the last brick's
// offset and, compared with n_index, into the status word
__global__ __launch_bounds__(TILE) void tile_scan_kernel(u64 *__restrict__ tile_sums,
                                                         unsigned tiles,
                                                         int32_t *__restrict__ offsets,
                                                         unsigned n_bricks, unsigned n_index,
                                                         int32_t *__restrict__ status) {
  __shared__ u64 sums[TILE];
  const u64 total = side_scan_runs<u64>(tile_sums, tiles, sums);
  if (threadIdx.x == TILE - 1) {
    offsets[n_bricks] = (int32_t)total;
    *status = total != (u64)n_index ? 1 : 0;
  }
}

// counters -> exclusive offsets, in place
__global__ __launch_bounds__(TILE) void offsets_kernel(int32_t *__restrict__ counts,
                                                       unsigned n_bricks, unsigned tiles,
                                                       const u64 *__restrict__ tile_sums) {
  __shared__ u64 sums[TILE];
  for (unsigned tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const unsigned i = tile * (unsigned)TILE + threadIdx.x;
    const u64 own = i < n_bricks ? (u64)(unsigned)counts[i] : 0ull;
    const u64 incl = side_block_scan(own, sums);
    if (i < n_bricks) counts[i] = (int32_t)(tile_sums[tile] + incl - own);
  }
}

__global__ __launch_bounds__(BLOCK) void fill_kernel(const int32_t *__restrict__ tbars, Plan p,
                                                     const int32_t *__restrict__ offsets,
                                                     int32_t *__restrict__ cursors,
                                                     const int32_t *__restrict__ status,
                                                     int32_t *__restrict__ staging) {
  if (*status != 0) return;
  const unsigned lane = threadIdx.x & (WAVE - 1);
  const unsigned waves = gridDim.x * (BLOCK / WAVE);
  for (unsigned j = blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE; j < p.n_tbars; j += waves) {
    const Range r = tbar_range(tbars, j, p);
    for (unsigned i = lane; i < r.n; i += WAVE) {
      const unsigned b = brick_of(r, i, p);
      if (b >= p.n_bricks) continue;
      const unsigned at = (unsigned)offsets[b] + (unsigned)atomicAdd(&cursors[b], 1);
      if (at < p.n_index) staging[(size_t)at] = (int32_t)j;
    }
  }
}

__global__ __launch_bounds__(BLOCK) void order_kernel(const int32_t *__restrict__ offsets, Plan p,
                                                      const int32_t *__restrict__ staging,
                                                      const int32_t *__restrict__ status,
                                                      int32_t *__restrict__ index) {
  if (*status != 0) return;
  const int lane = threadIdx.x & (WAVE - 1);
  const unsigned waves = gridDim.x * (BLOCK / WAVE);
  const unsigned first =
      __builtin_amdgcn_readfirstlane(blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE);
  for (unsigned b = first; b < p.n_bricks; b += waves) {       // wave-uniform
    const int beg = max(__builtin_amdgcn_readfirstlane(offsets[b]), 0);
    const int end = min(__builtin_amdgcn_readfirstlane(offsets[b + 1]), (int)p.n_index);
    for (int i0 = beg; i0 < end; i0 += WAVE) {                 // the lane's own j
      const bool own = lane < end - i0;
      const int mine = own ? staging[(size_t)i0 + lane] : 0;
      int rank = 0;
      for (int c0 = beg; c0 < end; c0 += WAVE) {               // against the list, 64 at a time
        const int n = min(WAVE, end - c0);
        const int v = lane < n ? staging[(size_t)c0 + lane] : 0;
        for (int k = 0; k < n; ++k) rank += __builtin_amdgcn_readlane(v, k) < mine ? 1 : 0;
      }
      if (own) index[(size_t)beg + rank] = mine;               // rank < end - beg
    }
  }
}

struct Layout {
  int64_t tiles, sums_at, cursors_at, staging_at, bytes;
};

// scratch: [status word, padded to 16 B][tile sums, 8 B each][cursors][staging list]
Layout layout(int64_t n_bricks, int64_t n_index) {
  Layout l;
  l.tiles = (n_bricks + TILE - 1) / TILE;
  l.sums_at = 16;
  l.cursors_at = l.sums_at + l.tiles * 8;
  l.staging_at = l.cursors_at + n_bricks * 4;
  l.bytes = l.staging_at + n_index * 4;
  return l;
}

int counts_ok(const char *fn, int64_t n_tbars, int64_t n_bricks, int64_t n_index) {
  if (n_tbars < 0 || n_tbars > SIDE_INT32_MAX / 3)
    return fplp_fail("%s: n_tbars %lld must lie in [0, %lld]", fn, (long long)n_tbars,
                     (long long)(SIDE_INT32_MAX / 3));
  if (n_bricks < 1 || n_bricks + 1 > SIDE_INT32_MAX)
    return fplp_fail("%s: %lld bricks: int32 offsets index 1 to 2^31 - 2 bricks", fn,
                     (long long)n_bricks);
  return in_int32_range(fn, "n_index", n_index, 0);
}

unsigned blocks_for(int64_t waves, unsigned cap) {
  const int64_t blocks = (waves + BLOCK / WAVE - 1) / (BLOCK / WAVE);
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, cap));
}

}  // namespace

FPLP_EXPORT const char *fplp_last_error(void) try {
  return side_err;
} catch (...) { return "fplp_last_error: C++ exception"; }

FPLP_EXPORT int fplp_abi_version(void) try {
  return FPLP_ABI_VERSION;
} FPLP_CATCH()

FPLP_EXPORT int fplp_scratch_bytes(int64_t n_tbars, int64_t n_bricks, int64_t n_index,
                                   int64_t *bytes) try {
  const char *fn = "fplp_scratch_bytes";
  if (!bytes) return fplp_fail("%s: null pointer argument", fn);
  if (counts_ok(fn, n_tbars, n_bricks, n_index)) return 1;
  *bytes = layout(n_bricks, n_index).bytes;
  return 0;
} FPLP_CATCH()

FPLP_EXPORT int fplp_plan_bricks(const int32_t *tbars, int64_t n_tbars, const int64_t dims[3],
                                 int32_t half, int32_t *offsets, int32_t *index, int64_t n_index,
                                 void *scratch, int64_t scratch_bytes, void *stream) try {
  const char *fn = "fplp_plan_bricks";
  if (!dims || !offsets || !scratch) return fplp_fail("%s: null pointer argument", fn);
  for (int a = 0; a < 3; ++a)
    if (dims[a] < 1) return fplp_fail("%s: dims (%lld,%lld,%lld) must be positive", fn,
                                      (long long)dims[0], (long long)dims[1], (long long)dims[2]);
  int64_t voxels;
  if (volume_voxels(fn, dims, "the brick tables", "render it in parts", &voxels)) return 1;
  if (half < 0 || half > FPLP_MAX_RADIUS)
    return fplp_fail("%s: half %d must lie in [0, %d]", fn, half, FPLP_MAX_RADIUS);
  Plan p;
  p.nb0 = (int)((dims[0] + BZ - 1) / BZ);
  p.nb1 = (int)((dims[1] + BY - 1) / BY);
  p.nb2 = (int)((dims[2] + BX - 1) / BX);
  const int64_t n_bricks = (int64_t)p.nb0 * p.nb1 * p.nb2;      // <= voxels
  if (counts_ok(fn, n_tbars, n_bricks, n_index)) return 1;
  if (n_tbars > 0 && !tbars)
    return fplp_fail("%s: null pointer argument (a table of %lld T-bars)", fn, (long long)n_tbars);
  if (n_index > 0 && !index)
    return fplp_fail("%s: null pointer argument (an index of %lld rows)", fn, (long long)n_index);
  if (!aligned(tbars, 4) || !aligned(offsets, 4) || !aligned(index, 4))
    return fplp_fail("%s: a table is not aligned to an int32", fn);
  const Layout l = layout(n_bricks, n_index);
  if (!aligned(scratch, 8) || scratch_bytes < l.bytes)
    return fplp_fail("%s: scratch of %lld bytes, fplp_scratch_bytes asks for %lld (8-byte aligned)",
                     fn, (long long)scratch_bytes, (long long)l.bytes);
  p.half = half;
  p.n_tbars = (unsigned)n_tbars;
  p.n_bricks = (unsigned)n_bricks;
  p.n_index = (unsigned)n_index;
  char *base = (char *)scratch;
  int32_t *status = (int32_t *)base;
  u64 *tile_sums = (u64 *)(base + l.sums_at);
  int32_t *cursors = (int32_t *)(base + l.cursors_at);
  int32_t *staging = (int32_t *)(base + l.staging_at);
  const unsigned tiles = (unsigned)l.tiles;
  const unsigned tile_blocks = std::min(tiles, MAX_TILE_BLOCKS);
  hipStream_t st = (hipStream_t)stream;

  hipError_t e = hipMemsetAsync(offsets, 0, (size_t)(n_bricks + 1) * 4, st);
  if (e == hipSuccess) e = hipMemsetAsync(cursors, 0, (size_t)n_bricks * 4, st);
  if (e != hipSuccess)
    return fplp_fail("%s: clearing the counters failed: %s", fn, hipGetErrorString(e));
  if (n_tbars > 0) {
    hipLaunchKernelGGL(count_kernel, dim3(blocks_for(n_tbars, MAX_BLOCKS)), dim3(BLOCK), 0, st,
                       tbars, p, offsets);
    if (launched("fplp_plan_bricks (count)")) return 1;
  }
  hipLaunchKernelGGL(tile_sum_kernel, dim3(tile_blocks), dim3(TILE), 0, st, offsets, p.n_bricks,
                     tiles, tile_sums);
  if (launched("fplp_plan_bricks (tile sums)")) return 1;
  hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(TILE), 0, st, tile_sums, tiles, offsets,
                     p.n_bricks, p.n_index, status);
  if (launched("fplp_plan_bricks (tile scan)")) return 1;
  hipLaunchKernelGGL(offsets_kernel, dim3(tile_blocks), dim3(TILE), 0, st, offsets, p.n_bricks,
                     tiles, tile_sums);
  if (launched("fplp_plan_bricks (offsets)")) return 1;
  if (n_tbars > 0 && n_index > 0) {
    hipLaunchKernelGGL(fill_kernel, dim3(blocks_for(n_tbars, MAX_BLOCKS)), dim3(BLOCK), 0, st,
                       tbars, p, offsets, cursors, status, staging);
    if (launched("fplp_plan_bricks (fill)")) return 1;
    hipLaunchKernelGGL(order_kernel, dim3(blocks_for(n_bricks, MAX_BLOCKS)), dim3(BLOCK), 0, st,
                       offsets, p, staging, status, index);
    return launched("fplp_plan_bricks (order)");
  }
  return 0;
} FPLP_CATCH()
