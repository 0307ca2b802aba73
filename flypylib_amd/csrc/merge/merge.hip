// libfplmerge.so (include/fplmerge.h): the merge loop of fplsynapses.rm_tbar_multi_pred on the
// GPU, from the resident neighbour table of libfplnear.so to the removed / moved flags.
// flypylib_amd/dedupe.py's merge_numpy is the specification; DESIGN.md section 14.1 has the
// argument and the measured times.
//
//   a. rows_count_kernel / rows_fill_kernel   a thread owns a point: its row of the table is
//                       walked, the partners the reference's own sqrt expression keeps are counted
//                       (has_neighbor), the counts scanned (side_scan_kernel) and the kept columns
//                       written in order from the row's offset.  One writer per word.
//   b. sweep_kernel     min-label propagation, PULLED over the CSR rows: a thread owns a point and
//                       writes min(own label, its row's labels) of the sweep before into the other
//                       of two buffers.  The matching's sweep (assign.hip) pushes over a pair list
//                       with atomicMin; here the rows are at hand, so a point can pull and needs no
//                       atomic - and the sweep count no longer depends on how the blocks are
//                       scheduled, so the host executor's count is the device's.  IT GROWS WITH
//                       THE COMPONENT DIAMETER; the host reads the flag once per sweep.
//   c. group_keys_kernel, boundary_kernel and the compaction (count_kernel, side_scan_kernel,
//                       index_fill_kernel - the scheme of assign.hip) around the caller's
//                       torch.sort: the points by (component, rank), the components' starts.
//   d. solve_kernel     A LANE PER COMPONENT.  Components are overwhelmingly 2 - 3 points with
//                       candidate sets of 2 - 3, and the loop is sequential inside a component:
//                       the only parallel work a wavefront per component would find is the scan of
//                       a ball's few dozen candidates, once or twice per merged pair, while 61 of
//                       64 lanes idle through everything else.  With a lane each, 64 components run
//                       side by side and the divergence costs what the slowest of them costs;
//                       the component cap bounds that, and what is larger goes to the host.
//                       The candidate list (FPLG_CAND_CAP indices, kept ascending by insertion)
//                       and the 18 bounds of a ball's key ranges live in LDS, a column per lane:
//                       in registers they would be indexed dynamically and go to scratch.
//                       A lane reads and writes the state of its own component's points only.
//   e. the flagged component ids are compacted like any other flag list.
//
// The candidate count is CAPPED AT 7 (FPLG_CAND_CAP): numpy's np.sum is a plain left-to-right
// loop below 8 elements, which is what the mean here reproduces; its 8-accumulator pairwise form
// from 8 on is not reproduced - such sets raise the flag.
//
// Float64 throughout with every operation rounded on its own (contraction off, __dadd_rn /
// __dmul_rn / __ddiv_rn), the correctly rounded square root, v_rndne for np.round.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "fplmerge.h"
#include "../side/side_abi.h"
#include "../side/side_device.h"

// this library's spelling of the shared shell
#define FPLG_EXPORT SIDE_EXPORT
#define FPLG_CATCH() SIDE_CATCH()
#define fplg_fail side_fail

namespace {

constexpr int BLOCK = FPLG_BLOCK;
constexpr int MAX_BLOCKS = FPLG_MAX_BLOCKS;
constexpr int WAVE = 64;
constexpr int SB = FPLG_SOLVE_BLOCK;
constexpr int CAND = FPLG_CAND_CAP;
constexpr int RUNS = 9;                     // the (dy, dz) neighbours of a cell row
constexpr int32_t IDLE = 2147483647;        // the component field of an idle point's group key
constexpr int64_t MAX_AXIS = (int64_t)1 << 28;
static_assert(FPLG_SCAN_THREADS == SIDE_SCAN_THREADS, "the scan is side_scan_kernel's block");
static_assert(BLOCK % WAVE == 0 && BLOCK / WAVE <= WAVE, "the waves' sums fit one wave");
static_assert(SB == WAVE, "a block of the solve kernel is one wavefront");
static_assert(CAND < 8, "numpy's sum is a plain loop below 8 elements only");

int64_t blocks_of(int64_t n) { return (n + BLOCK - 1) / BLOCK; }
dim3 grid_of(int64_t n) { return dim3((unsigned)blocks_of(n)); }
dim3 stride_grid(int64_t n) { return dim3((unsigned)std::min<int64_t>(blocks_of(n), MAX_BLOCKS)); }
int64_t scratch_for(int64_t n) { return 8 + ((4 * blocks_of(n) + 7) & ~(int64_t)7); }

// d = sqrt((dx*dx + dy*dy) + dz*dz): llvm.sqrt.f64 is IEEE, correctly rounded
__device__ __forceinline__ double dist(const double *a, double bx, double by, double bz) {
  return __builtin_sqrt(side_dist2(a[0], a[1], a[2], bx, by, bz));
}

// ---- a. the rows the reference keeps ------------------------------------------------------------

struct Rows {
  const double *locs;
  uint32_t n;
  double t;
  const uint32_t *offsets;
  const int32_t *indices;
  uint32_t entries;
};

__device__ __forceinline__ bool kept(const Rows &a, const double *p, uint32_t e) {
  const uint32_t j = (uint32_t)a.indices[e];
  if (j >= a.n) return false;
  const double *q = a.locs + (size_t)j * 3;
  const double d = dist(p, q[0], q[1], q[2]);
  return d > 0.0 && d < a.t;
}

__global__ __launch_bounds__(BLOCK) void rows_count_kernel(Rows a, uint32_t *__restrict__ has,
                                                           uint32_t *__restrict__ cells) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= a.n) return;
  const uint32_t lo = std::min(a.offsets[i], a.entries), hi = std::min(a.offsets[i + 1], a.entries);
  const double *p = a.locs + (size_t)i * 3;
  uint32_t count = 0;
  for (uint32_t e = lo; e < hi; ++e) count += kept(a, p, e) ? 1u : 0u;
  has[i] = count;
  cells[i] = count;
}

__global__ __launch_bounds__(BLOCK) void rows_fill_kernel(Rows a, const uint32_t *__restrict__ out_offsets,
                                                          uint32_t capacity,
                                                          int32_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= a.n) return;
  const uint32_t lo = std::min(a.offsets[i], a.entries), hi = std::min(a.offsets[i + 1], a.entries);
  const double *p = a.locs + (size_t)i * 3;
  uint32_t at = out_offsets[i];
  for (uint32_t e = lo; e < hi; ++e) {
    if (!kept(a, p, e)) continue;
    if (at < capacity) out[at] = a.indices[e];
    ++at;
  }
}

// ---- b. labels ----------------------------------------------------------------------------------

__global__ __launch_bounds__(BLOCK) void init_labels_kernel(int32_t *__restrict__ a,
                                                            int32_t *__restrict__ b, uint32_t n) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  a[i] = (int32_t)i;
  b[i] = (int32_t)i;
}

__global__ __launch_bounds__(BLOCK) void sweep_kernel(const uint32_t *__restrict__ offsets,
                                                      const int32_t *__restrict__ indices,
                                                      uint32_t n, uint32_t entries,
                                                      const int32_t *__restrict__ in,
                                                      int32_t *__restrict__ out,
                                                      int32_t *__restrict__ changed) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t lo = std::min(offsets[i], entries), hi = std::min(offsets[i + 1], entries);
  const int32_t own = in[i];
  int32_t m = own;
  for (uint32_t e = lo; e < hi; ++e) {
    const uint32_t j = (uint32_t)indices[e];
    if (j < n) m = std::min(m, in[j]);
  }
  out[i] = m;
  if (m != own) *changed = 1;               // every writer writes the same word
}

// ---- c. grouping and compaction -----------------------------------------------------------------

__global__ __launch_bounds__(BLOCK) void group_keys_kernel(const uint32_t *__restrict__ offsets,
                                                           const int32_t *__restrict__ label,
                                                           const int32_t *__restrict__ rank,
                                                           uint32_t n, int64_t *__restrict__ keys) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const bool idle = offsets[i + 1] <= offsets[i];
  const int64_t c = idle ? IDLE : (label[i] & IDLE);
  keys[i] = (c << 32) | (int64_t)(uint32_t)rank[i];
}

__global__ __launch_bounds__(BLOCK) void boundary_kernel(const int64_t *__restrict__ keys, int64_t n,
                                                         int32_t *__restrict__ flags) {
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e <= n; e += stride) {
    const int64_t before = e > 0 ? keys[e - 1] >> 32 : -1;
    flags[e] = e < n ? ((keys[e] >> 32) != before ? 1 : 0) : (before != IDLE ? 1 : 0);
  }
}

// the flagged entries of this block below the calling thread's, and in *all the block's
__device__ __forceinline__ uint32_t block_rank(bool flag, uint32_t *wave_sums, uint32_t *all) {
  const uint32_t lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
  const unsigned long long m = __ballot(flag);
  if (lane == 0) wave_sums[wave] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t before = 0, total = 0;
#pragma unroll
  for (uint32_t w = 0; w < BLOCK / WAVE; ++w) {
    const uint32_t s = wave_sums[w];
    before += w < wave ? s : 0u;
    total += s;
  }
  *all = total;
  return before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(BLOCK) void count_kernel(const int32_t *__restrict__ flags, int64_t n,
                                                      uint32_t *__restrict__ cells) {
  __shared__ uint32_t wave_sums[BLOCK / WAVE];
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  uint32_t all;
  block_rank(e < n && flags[e] != 0, wave_sums, &all);
  if (threadIdx.x == 0) cells[blockIdx.x] = all;
}

__global__ __launch_bounds__(BLOCK) void index_fill_kernel(const int32_t *__restrict__ flags,
                                                           int64_t n,
                                                           const uint32_t *__restrict__ offsets,
                                                           int64_t capacity,
                                                           int32_t *__restrict__ index_out) {
  __shared__ uint32_t wave_sums[BLOCK / WAVE];
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const bool flag = e < n && flags[e] != 0;
  uint32_t all;
  const int64_t k = (int64_t)offsets[blockIdx.x] + block_rank(flag, wave_sums, &all);
  if (flag && k < capacity) index_out[k] = (int32_t)e;
}

// ---- d. the merge loop --------------------------------------------------------------------------

struct Grid {
  double ox, oy, oz, cell;
  int64_t nx, ny, nz;
};

struct Solve {
  const double *locs, *conf;
  const int64_t *labels;
  const int32_t *comp;
  uint32_t n;
  double t;
  Grid g;
  const int64_t *keys, *order;
  const uint32_t *f_offsets;
  const int32_t *f_indices;
  uint32_t f_entries;
  const int64_t *members;
  const int32_t *starts;
  uint32_t n_comp;
  int cand_cap, comp_cap, max_moves;
  uint8_t *rm, *mv;
  long long *mv_loc;
  int32_t *flagged;
};

// the cell of a centre that may lie outside the grid: beyond it by more than a cell there is
// nothing, and the clamp keeps the int64 exact
__device__ __forceinline__ int64_t centre_cell(double x, double o, double cell, int64_t n) {
#pragma clang fp contract(off)
  double u = floor((x - o) / cell);
  u = fmin(fmax(u, -2.0), (double)(n + 1));
  return (int64_t)u;
}

// the first position in keys[lo, n) whose key is not below k
__device__ __forceinline__ uint32_t lower_bound(const int64_t *__restrict__ keys, uint32_t lo,
                                                uint32_t n, int64_t k) {
  uint32_t hi = n;
  for (int guard = 0; guard < 32 && lo < hi; ++guard) {      // the range halves: 32 steps at most
    const uint32_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// `j` into the calling lane's ascending candidate column; beyond the cap it is counted only
__device__ __forceinline__ void insert(int32_t (*cand)[SB], int *count, int cap, int32_t j) {
  const int t = threadIdx.x;
  if (*count < cap) {
    int p = *count;
    for (int guard = 0; guard < CAND && p > 0 && cand[p - 1][t] > j; ++guard) {
      cand[p][t] = cand[p - 1][t];
      --p;
    }
    cand[p][t] = j;
  }
  ++*count;
}

__global__ __launch_bounds__(SB) void solve_kernel(Solve args) {
#pragma clang fp contract(off)
  __shared__ uint32_t runs[2 * RUNS][SB];
  __shared__ int32_t cand[CAND][SB];
  // The arguments - fourteen arrays, the grid, the caps - are read deep inside divergent loops.
  // As kernel arguments they would all be held in scalar registers across the whole kernel, more
  // than there are, and spill; from LDS each comes into a vector register where it is used.
  __shared__ Solve shared_args;
  const int t = threadIdx.x;
  if (t == 0) shared_args = args;
  __syncthreads();
  const Solve &a = shared_args;
  const Grid &g = a.g;
  // no barrier below: a lane reads its own columns only
  for (int64_t k = (int64_t)blockIdx.x * SB + t; k < a.n_comp; k += (int64_t)gridDim.x * SB) {
    const int64_t m0 = a.starts[k], m1 = a.starts[k + 1];
    if (m0 < 0 || m1 > a.n || m1 <= m0) continue;             // not a component of this list
    const uint64_t first = (uint64_t)a.members[m0];
    if (first >= a.n) continue;
    const int32_t c = a.comp[first];
    if ((uint32_t)c >= a.n) continue;
    if (m1 - m0 > a.comp_cap) {
      a.flagged[c] = 1;
      continue;
    }
    bool dead = false;
    for (int64_t m = m0; m < m1 && !dead; ++m) {
      const uint64_t ii64 = (uint64_t)a.members[m];
      if (ii64 >= a.n) { dead = true; break; }
      const uint32_t ii = (uint32_t)ii64;
      if (a.rm[ii]) continue;
      const uint32_t lo = std::min(a.f_offsets[ii], a.f_entries),
                     hi = std::min(a.f_offsets[ii + 1], a.f_entries);
      if (hi <= lo) continue;                                  // has_neighbor == 0
      const int64_t lab = a.labels[ii];
      int count = 0;
      for (uint32_t e = lo; e < hi; ++e) {
        const uint32_t j = (uint32_t)a.f_indices[e];
        if (j >= a.n || j == ii) continue;
        if (a.comp[j] != c) { dead = true; continue; }         // not this table's component
        if (a.labels[j] == lab && !a.rm[j]) insert(cand, &count, a.cand_cap, (int32_t)j);
      }
      if (dead) break;
      if (count == 0) continue;
      a.mv[ii] = 1;
      insert(cand, &count, a.cand_cap, (int32_t)ii);
      const double *p = a.locs + (size_t)ii * 3;
      double ox = p[0], oy = p[1], oz = p[2];                  // the old location
      for (int move = 0; move <= a.max_moves; ++move) {
        if (count > a.cand_cap || count == 0) { dead = true; break; }
        double sum = 0.0;
        for (int q = 0; q < count; ++q) sum = __dadd_rn(sum, a.conf[cand[q][t]]);
        double mx = 0.0, my = 0.0, mz = 0.0;
        for (int q = 0; q < count; ++q) {
          const uint32_t j = (uint32_t)cand[q][t];
          const double w = __ddiv_rn(a.conf[j], sum);
          const double *r = a.locs + (size_t)j * 3;
          const double rx = __dmul_rn(w, r[0]), ry = __dmul_rn(w, r[1]), rz = __dmul_rn(w, r[2]);
          mx = q ? __dadd_rn(mx, rx) : rx;
          my = q ? __dadd_rn(my, ry) : ry;
          mz = q ? __dadd_rn(mz, rz) : rz;
        }
        if (!(fabs(mx) < 0x1p62 && fabs(my) < 0x1p62 && fabs(mz) < 0x1p62)) { dead = true; break; }
        const double nx = __builtin_rint(mx), ny = __builtin_rint(my), nz = __builtin_rint(mz);
        long long *out = a.mv_loc + (size_t)ii * 3;
        out[0] = (long long)nx; out[1] = (long long)ny; out[2] = (long long)nz;
        if (nx == ox && ny == oy && nz == oz) break;           // it rests
        if (move == a.max_moves) { dead = true; break; }
        ox = nx; oy = ny; oz = nz;
        // the ball around the moved centre, asked of the cell keys over ALL points
        const int64_t cx = centre_cell(nx, g.ox, g.cell, g.nx), cy = centre_cell(ny, g.oy, g.cell, g.ny),
                      cz = centre_cell(nz, g.oz, g.cell, g.nz);
        const int64_t x0 = cx > 0 ? cx - 1 : 0, x1 = cx + 1 < g.nx ? cx + 1 : g.nx - 1;
#pragma unroll 1
        for (int r = 0; r < RUNS; ++r) {
          const int64_t y = cy + (r % 3 - 1), z = cz + (r / 3 - 1);
          uint32_t rl = 0, rh = 0;
          if (y >= 0 && y < g.ny && z >= 0 && z < g.nz && x0 <= x1) {
            const int64_t row = (z * g.ny + y) * g.nx;
            rl = lower_bound(a.keys, 0u, a.n, row + x0);
            rh = lower_bound(a.keys, rl, a.n, row + x1 + 1);
          }
          runs[2 * r][t] = rl;
          runs[2 * r + 1][t] = rh;
        }
        count = 0;
        bool stranger = false;
#pragma unroll 1
        for (int r = 0; r < RUNS; ++r) {
          const uint32_t rh = runs[2 * r + 1][t];
          for (uint32_t q = runs[2 * r][t]; q < rh; ++q) {
            const uint64_t j64 = (uint64_t)a.order[q];
            if (j64 >= a.n) { stranger = true; continue; }     // a broken order: nothing to trust
            const uint32_t j = (uint32_t)j64;
            if (!(dist(a.locs + (size_t)j * 3, nx, ny, nz) < a.t) || a.labels[j] != lab) continue;
            const int32_t cj = a.comp[j];
            if (cj != c) {
              stranger = true;
              if ((uint32_t)cj < a.n) a.flagged[cj] = 1;       // every writer writes the same word
            } else if (!a.rm[j]) {
              insert(cand, &count, a.cand_cap, (int32_t)j);
            }
          }
        }
        if (stranger) { dead = true; break; }
      }
      if (dead) break;
      for (int q = 0; q < count; ++q) a.rm[cand[q][t]] = 1;
    }
    if (dead) a.flagged[c] = 1;
  }
}

// ---- argument checks ----------------------------------------------------------------------------

int count_ok(const char *fn, const char *what, int64_t n) { return in_int32_range(fn, what, n, 1); }

int table_ok(const char *fn, const double *locs, int64_t n, double t, const uint32_t *offsets,
             const int32_t *indices, int64_t entries, Rows *a) {
  if (!locs || !offsets) return fplg_fail("%s: null pointer argument", fn);
  if (count_ok(fn, "n", n) || in_int32_range(fn, "entries", entries, 0)) return 1;
  if (entries && !indices) return fplg_fail("%s: null pointer argument (the columns)", fn);
  if (!(std::isfinite(t) && t > 0.0)) return fplg_fail("%s: t %g must be finite and positive", fn, t);
  if (!aligned(locs, 8) || !aligned(offsets, 4) || !aligned(indices, 4))
    return fplg_fail("%s: a column is not aligned to its element", fn);
  *a = Rows{locs, (uint32_t)n, t, offsets, indices, (uint32_t)entries};
  return 0;
}

int scratch_ok(const char *fn, const void *scratch, int64_t scratch_bytes, int64_t n) {
  if (!aligned(scratch, 8) || scratch_bytes < scratch_for(n))
    return fplg_fail("%s: scratch of %lld bytes, fplg_scratch_bytes asks for %lld (8-byte aligned)",
                     fn, (long long)scratch_bytes, (long long)scratch_for(n));
  return 0;
}

int cap_ok(const char *fn, const char *what, int64_t v, int64_t hi) {
  if (v < 1 || v > hi)
    return fplg_fail("%s: %s %lld must lie in [1, %lld]", fn, what, (long long)v, (long long)hi);
  return 0;
}

}  // namespace

FPLG_EXPORT const char *fplg_last_error(void) try {
  return side_err;
} catch (...) { return "fplg_last_error: C++ exception"; }

FPLG_EXPORT int fplg_abi_version(void) try {
  return FPLG_ABI_VERSION;
} FPLG_CATCH()

FPLG_EXPORT int fplg_rows_count(const double *locs, int64_t n, double t, const uint32_t *offsets,
                                const int32_t *indices, int64_t entries, uint32_t *has_neighbor,
                                uint32_t *out_offsets, void *head, int64_t *total,
                                void *stream) try {
  const char *fn = "fplg_rows_count";
  Rows a;
  if (!has_neighbor || !out_offsets || !head || !total) return fplg_fail("%s: null pointer argument", fn);
  if (table_ok(fn, locs, n, t, offsets, indices, entries, &a)) return 1;
  if (!aligned(has_neighbor, 4) || !aligned(out_offsets, 4) || !aligned(head, 8))
    return fplg_fail("%s: a column is not aligned to its element", fn);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rows_count_kernel, grid_of(n), dim3(BLOCK), 0, st, a, has_neighbor, out_offsets);
  if (launched(fn)) return 1;
  hipLaunchKernelGGL(side_scan_kernel<uint32_t>, dim3(1), dim3(SIDE_SCAN_THREADS), 0, st, out_offsets,
                     a.n, (unsigned long long *)head, out_offsets + a.n);
  if (launched("fplg_rows_count (scan)")) return 1;
  unsigned long long got = 0;
  if (side_read_back(fn, st, &got, head, sizeof(got))) return 1;
  *total = (int64_t)got;                    // at most `entries`
  return 0;
} FPLG_CATCH()

FPLG_EXPORT int fplg_rows_fill(const double *locs, int64_t n, double t, const uint32_t *offsets,
                               const int32_t *indices, int64_t entries, const uint32_t *out_offsets,
                               int64_t capacity, int32_t *out_indices, void *stream) try {
  const char *fn = "fplg_rows_fill";
  Rows a;
  if (!out_offsets) return fplg_fail("%s: null pointer argument", fn);
  if (table_ok(fn, locs, n, t, offsets, indices, entries, &a)) return 1;
  if (in_int32_range(fn, "capacity", capacity, 0)) return 1;
  if (capacity == 0) return 0;
  if (!out_indices) return fplg_fail("%s: null pointer argument (the column array)", fn);
  if (!aligned(out_offsets, 4) || !aligned(out_indices, 4))
    return fplg_fail("%s: a column is not aligned to its element", fn);
  hipLaunchKernelGGL(rows_fill_kernel, grid_of(n), dim3(BLOCK), 0, (hipStream_t)stream, a, out_offsets,
                     (uint32_t)capacity, out_indices);
  return launched(fn);
} FPLG_CATCH()

FPLG_EXPORT int fplg_labels(const uint32_t *offsets, const int32_t *indices, int64_t n,
                            int64_t entries, int32_t *label, int32_t *other, int32_t *changed,
                            int64_t max_sweeps, int64_t *sweeps, void *stream) try {
  const char *fn = "fplg_labels";
  if (!offsets || !label || !other || !changed || !sweeps)
    return fplg_fail("%s: null pointer argument", fn);
  if (count_ok(fn, "n", n) || in_int32_range(fn, "entries", entries, 0)) return 1;
  if (entries && !indices) return fplg_fail("%s: null pointer argument (the columns)", fn);
  if (max_sweeps < 1) return fplg_fail("%s: max_sweeps %lld must be positive", fn, (long long)max_sweeps);
  if (!aligned(offsets, 4) || !aligned(indices, 4) || !aligned(label, 4) || !aligned(other, 4) ||
      !aligned(changed, 4))
    return fplg_fail("%s: a column is not aligned to its element", fn);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(init_labels_kernel, grid_of(n), dim3(BLOCK), 0, st, label, other, (uint32_t)n);
  if (launched("fplg_labels (init)")) return 1;
  int32_t *in = label, *out = other;
  int64_t done = 0;
  for (;;) {
    if (done == max_sweeps)
      return fplg_fail("%s: the labels still change after %lld sweeps", fn, (long long)done);
    hipError_t e = hipMemsetAsync(changed, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return fplg_fail("%s: clearing the flag failed: %s", fn, hipGetErrorString(e));
    hipLaunchKernelGGL(sweep_kernel, grid_of(n), dim3(BLOCK), 0, st, offsets, indices, (uint32_t)n,
                       (uint32_t)entries, in, out, changed);
    if (launched("fplg_labels (sweep)")) return 1;
    ++done;
    int32_t flag = 0;
    if (side_read_back(fn, st, &flag, changed, sizeof(flag))) return 1;
    if (!flag) break;                       // out == in: both buffers hold the result
    std::swap(in, out);
  }
  *sweeps = done;
  return 0;
} FPLG_CATCH()

FPLG_EXPORT int fplg_group_keys(const uint32_t *offsets, const int32_t *label, const int32_t *rank,
                                int64_t n, int64_t *keys, void *stream) try {
  const char *fn = "fplg_group_keys";
  if (!offsets || !label || !rank || !keys) return fplg_fail("%s: null pointer argument", fn);
  if (count_ok(fn, "n", n)) return 1;
  if (!aligned(offsets, 4) || !aligned(label, 4) || !aligned(rank, 4) || !aligned(keys, 8))
    return fplg_fail("%s: a column is not aligned to its element", fn);
  hipLaunchKernelGGL(group_keys_kernel, grid_of(n), dim3(BLOCK), 0, (hipStream_t)stream, offsets, label,
                     rank, (uint32_t)n, keys);
  return launched(fn);
} FPLG_CATCH()

FPLG_EXPORT int fplg_boundaries(const int64_t *sorted_keys, int64_t n, int32_t *flags,
                                void *stream) try {
  const char *fn = "fplg_boundaries";
  if (!sorted_keys || !flags) return fplg_fail("%s: null pointer argument", fn);
  if (count_ok(fn, "n", n)) return 1;
  if (n == SIDE_INT32_MAX) return fplg_fail("%s: n + 1 flags exceed 2^31 - 1", fn);
  if (!aligned(sorted_keys, 8) || !aligned(flags, 4))
    return fplg_fail("%s: a column is not aligned to its element", fn);
  hipLaunchKernelGGL(boundary_kernel, stride_grid(n + 1), dim3(BLOCK), 0, (hipStream_t)stream,
                     sorted_keys, n, flags);
  return launched(fn);
} FPLG_CATCH()

FPLG_EXPORT int fplg_scratch_bytes(int64_t n, int64_t *bytes) try {
  if (!bytes) return fplg_fail("fplg_scratch_bytes: null pointer argument");
  if (count_ok("fplg_scratch_bytes", "n", n)) return 1;
  *bytes = scratch_for(n);
  return 0;
} FPLG_CATCH()

FPLG_EXPORT int fplg_flags_count(const int32_t *flags, int64_t n, void *scratch,
                                 int64_t scratch_bytes, int64_t *total, void *stream) try {
  const char *fn = "fplg_flags_count";
  if (!flags || !scratch || !total) return fplg_fail("%s: null pointer argument", fn);
  if (count_ok(fn, "n", n)) return 1;
  if (!aligned(flags, 4)) return fplg_fail("%s: the flags are not 4-byte aligned", fn);
  if (scratch_ok(fn, scratch, scratch_bytes, n)) return 1;
  unsigned long long *sum = (unsigned long long *)scratch;
  uint32_t *cells = (uint32_t *)((char *)scratch + 8);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(count_kernel, grid_of(n), dim3(BLOCK), 0, st, flags, n, cells);
  if (launched(fn)) return 1;
  hipLaunchKernelGGL(side_scan_kernel<uint32_t>, dim3(1), dim3(SIDE_SCAN_THREADS), 0, st, cells,
                     (uint32_t)blocks_of(n), sum, nullptr);
  if (launched("fplg_flags_count (scan)")) return 1;
  unsigned long long got = 0;
  if (side_read_back(fn, st, &got, sum, sizeof(got))) return 1;
  *total = (int64_t)got;                    // at most n
  return 0;
} FPLG_CATCH()

FPLG_EXPORT int fplg_flags_fill(const int32_t *flags, int64_t n, const void *scratch,
                                int64_t scratch_bytes, int64_t capacity, int32_t *index_out,
                                void *stream) try {
  const char *fn = "fplg_flags_fill";
  if (!flags || !scratch) return fplg_fail("%s: null pointer argument", fn);
  if (count_ok(fn, "n", n)) return 1;
  if (in_int32_range(fn, "capacity", capacity, 0)) return 1;
  if (!aligned(flags, 4)) return fplg_fail("%s: the flags are not 4-byte aligned", fn);
  if (scratch_ok(fn, scratch, scratch_bytes, n)) return 1;
  if (capacity == 0) return 0;
  if (!index_out) return fplg_fail("%s: null pointer argument (the index array)", fn);
  if (!aligned(index_out, 4)) return fplg_fail("%s: the index array is not 4-byte aligned", fn);
  const uint32_t *offsets = (const uint32_t *)((const char *)scratch + 8);
  hipLaunchKernelGGL(index_fill_kernel, grid_of(n), dim3(BLOCK), 0, (hipStream_t)stream, flags, n,
                     offsets, capacity, index_out);
  return launched(fn);
} FPLG_CATCH()

FPLG_EXPORT int fplg_solve(const double *locs, const double *conf, const int64_t *labels,
                           const int32_t *comp, int64_t n, double t, const double *origin,
                           double cell, const int64_t *dims, const int64_t *sorted_keys,
                           const int64_t *order, const uint32_t *f_offsets, const int32_t *f_indices,
                           int64_t f_entries, const int64_t *members, const int32_t *starts,
                           int64_t n_comp, int64_t cand_cap, int64_t comp_cap, int64_t max_moves,
                           uint8_t *rm, uint8_t *mv, int64_t *mv_loc, int32_t *flagged,
                           void *stream) try {
  const char *fn = "fplg_solve";
  if (!locs || !conf || !labels || !comp || !origin || !dims || !sorted_keys || !order ||
      !f_offsets || !members || !starts || !rm || !mv || !mv_loc || !flagged)
    return fplg_fail("%s: null pointer argument", fn);
  if (count_ok(fn, "n", n) || count_ok(fn, "n_comp", n_comp) ||
      in_int32_range(fn, "f_entries", f_entries, 0))
    return 1;
  if (n_comp > n) return fplg_fail("%s: %lld components of %lld points", fn, (long long)n_comp, (long long)n);
  if (f_entries && !f_indices) return fplg_fail("%s: null pointer argument (the columns)", fn);
  if (!(std::isfinite(t) && t > 0.0)) return fplg_fail("%s: t %g must be finite and positive", fn, t);
  if (cap_ok(fn, "cand_cap", cand_cap, FPLG_CAND_CAP) || cap_ok(fn, "comp_cap", comp_cap, FPLG_COMP_CAP) ||
      cap_ok(fn, "max_moves", max_moves, FPLG_MAX_MOVES))
    return 1;
  if (!(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2])))
    return fplg_fail("%s: the grid's origin is not finite", fn);
  if (!(std::isfinite(cell) && cell >= t * (1.0 + 0x1p-20)))
    return fplg_fail("%s: cell side %.17g is below t (1 + 2^-20) = %.17g: a ball could reach two "
                     "cells away", fn, cell, t * (1.0 + 0x1p-20));
  for (int ax = 0; ax < 3; ++ax)
    if (dims[ax] < 1 || dims[ax] > MAX_AXIS)
      return fplg_fail("%s: %lld cells along axis %d, must lie in [1, 2^28]", fn, (long long)dims[ax], ax);
  if (dims[0] * dims[1] > ((int64_t)1 << 62) / dims[2])
    return fplg_fail("%s: a grid of %lld x %lld x %lld cells exceeds the 2^62 an int64 key can "
                     "number", fn, (long long)dims[0], (long long)dims[1], (long long)dims[2]);
  if (!aligned(locs, 8) || !aligned(conf, 8) || !aligned(labels, 8) || !aligned(sorted_keys, 8) ||
      !aligned(order, 8) || !aligned(members, 8) || !aligned(mv_loc, 8) || !aligned(comp, 4) ||
      !aligned(f_offsets, 4) || !aligned(f_indices, 4) || !aligned(starts, 4) || !aligned(flagged, 4))
    return fplg_fail("%s: a column is not aligned to its element", fn);
  Solve a;
  a.locs = locs; a.conf = conf; a.labels = labels; a.comp = comp;
  a.n = (uint32_t)n; a.t = t;
  a.g = Grid{origin[0], origin[1], origin[2], cell, dims[0], dims[1], dims[2]};
  a.keys = sorted_keys; a.order = order;
  a.f_offsets = f_offsets; a.f_indices = f_indices; a.f_entries = (uint32_t)f_entries;
  a.members = members; a.starts = starts; a.n_comp = (uint32_t)n_comp;
  a.cand_cap = (int)cand_cap; a.comp_cap = (int)comp_cap; a.max_moves = (int)max_moves;
  a.rm = rm; a.mv = mv; a.mv_loc = (long long *)mv_loc; a.flagged = flagged;
  const int64_t chunks = (n_comp + SB - 1) / SB;
  const unsigned grid = (unsigned)std::min<int64_t>(chunks, FPLG_SOLVE_BLOCKS);
  hipLaunchKernelGGL(solve_kernel, dim3(grid), dim3(SB), 0, (hipStream_t)stream, a);
  return launched(fn);
} FPLG_CATCH()
