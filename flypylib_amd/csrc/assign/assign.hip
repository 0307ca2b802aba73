// libfplassign.so (include/fplassign.h): the sparse matching of obj_pr / obj_pr_curve solved
// on the GPU, from the resident pair table of libfplmatch.so to the matched pairs.
//
//   a. cost_kernel      a thread owns rows of the table (grid stride): the cost of
//                       match.pair_costs, the label term, the confidence filter by rank.
//      The admissible rows are then compacted in table order by the three kernels every
//      stage below shares:
//        count_kernel   a block counts the flagged entries of its FPLA_BLOCK entries;
//        (scan)         side_scan_kernel of csrc/side/side_device.h over the per-block counts;
//        fill_kernel    the count again; a flagged entry goes to its block's offset plus its
//                       rank within the block (ballot + popcount, the waves' sums in LDS).
//      No atomics: every output has one writer and one place.
//   b. sweep_kernel     min-label propagation over the pair list: both ends of a pair are
//                       lowered to their minimum with an integer atomicMin.  The fixed point -
//                       every node carries the smallest prediction index of its component - is
//                       the same in whatever order the updates land.  A label travels one
//                       pair per sweep at the least, so THE SWEEP COUNT GROWS WITH THE
//                       COMPONENT DIAMETER (a chain of 15 pairs may take 15 sweeps and one
//                       more to see nothing change); the matching's components are a few
//                       points across.  The host reads the flag once per sweep.
//   c. the sort by label is the caller's (torch.sort, stable: the table is in (i, j) order
//      already); boundary_kernel marks the first pair of every component and the compaction
//      turns the marks into start offsets.
//   d. solve_kernel     one wavefront per component, a block is one wavefront.  A chunk of 64
//                       components is read a lane each, the single-pair ones are matched by
//                       their lanes, the others are solved one after the other by the whole
//                       wavefront: the distinct i and j are numbered in LDS, the block of
//                       costs is laid out in LDS with the shorter side as the workers, and
//                       the Jonker-Volgenant / Hungarian iteration with potentials inserts one
//                       worker at a time along a shortest augmenting path - a lane per job
//                       (column) holds the job's potential, slack, predecessor and worker in
//                       registers, the minimum over the free jobs is a butterfly of shuffles.
//                       Every loop has a bound that does not depend on the data's values.
//   e. the matched flags are compacted (component order, then (i, j)) like any other list.
//
// Costs are float64 with every operation rounded on its own: the squared distance is
// side_device.h's side_dist2, the square root is the correctly rounded one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "fplassign.h"
#include "../side/side_abi.h"
#include "../side/side_device.h"

// this library's spelling of the shared shell
#define FPLA_EXPORT SIDE_EXPORT
#define FPLA_CATCH() SIDE_CATCH()
#define fpla_fail side_fail

namespace {

constexpr int BLOCK = FPLA_BLOCK;
constexpr int MAX_BLOCKS = FPLA_MAX_BLOCKS;
constexpr int CAP = FPLA_CAP;
constexpr int WAVE = 64;
static_assert(FPLA_SCAN_THREADS == SIDE_SCAN_THREADS, "the scan is side_scan_kernel's block");
static_assert(CAP == WAVE, "a lane per job");
static_assert(BLOCK % WAVE == 0 && BLOCK / WAVE <= WAVE, "the waves' sums fit one wave");

// ---- the compaction ------------------------------------------------------------------------

int64_t blocks_of(int64_t n) { return (n + BLOCK - 1) / BLOCK; }

int64_t scratch_for(int64_t n) { return 8 + ((4 * blocks_of(n) + 7) & ~(int64_t)7); }

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

struct Fill {
  const int32_t *a, *b;
  const double *c;
  int32_t *a_out, *b_out;
  double *c_out;
  int32_t *index_out, *rank_out;
};

__global__ __launch_bounds__(BLOCK) void fill_kernel(const int32_t *__restrict__ flags, int64_t n,
                                                     const uint32_t *__restrict__ offsets,
                                                     int64_t capacity, Fill f) {
  __shared__ uint32_t wave_sums[BLOCK / WAVE];
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const bool flag = e < n && flags[e] != 0;
  uint32_t all;
  const int64_t k = (int64_t)offsets[blockIdx.x] + block_rank(flag, wave_sums, &all);
  if (e >= n) return;
  if (f.rank_out) f.rank_out[e] = flag ? (int32_t)k : -1;
  if (!flag || k >= capacity) return;
  if (f.a_out) f.a_out[k] = f.a[e];
  if (f.b_out) f.b_out[k] = f.b[e];
  if (f.c_out) f.c_out[k] = f.c[e];
  if (f.index_out) f.index_out[k] = (int32_t)e;
}

__global__ __launch_bounds__(BLOCK) void conf_kernel(const double *__restrict__ conf, int64_t n,
                                                     double thd, int32_t *__restrict__ flags) {
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < n; e += stride)
    flags[e] = conf[e] >= thd ? 1 : 0;
}

__global__ __launch_bounds__(BLOCK) void boundary_kernel(const int32_t *__restrict__ keys, int64_t n,
                                                         int32_t *__restrict__ flags) {
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < n; e += stride)
    flags[e] = (e == 0 || keys[e] != keys[e - 1]) ? 1 : 0;
}

// ---- a. costs ---------------------------------------------------------------------------------

struct Costs {
  const int32_t *ti, *tj;
  int64_t rows;
  const double *pred, *gt;
  uint32_t n_pred, n_gt;
  double t, label_add;
  const int64_t *pred_lbl, *gt_lbl;
  const int32_t *rank;
};

__device__ __forceinline__ double cost_of(const double *p, const double *g, double t) {
  // llvm.sqrt.f64: IEEE, correctly rounded
  return __builtin_sqrt(side_dist2(p[0], p[1], p[2], g[0], g[1], g[2])) - t;
}

__global__ __launch_bounds__(BLOCK) void cost_kernel(Costs a, int32_t *__restrict__ i_out,
                                                     double *__restrict__ cost_out,
                                                     int32_t *__restrict__ keep_out) {
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < a.rows; e += stride) {
    const uint32_t i = (uint32_t)a.ti[e], j = (uint32_t)a.tj[e];
    int32_t i_new = -1;
    double cost = 0.0;
    if (i < a.n_pred && j < a.n_gt) {
      i_new = a.rank ? a.rank[i] : (int32_t)i;
      cost = cost_of(a.pred + (size_t)i * 3, a.gt + (size_t)j * 3, a.t);
      if (a.pred_lbl && a.pred_lbl[i] != a.gt_lbl[j]) cost = __dadd_rn(cost, a.label_add);
    }
    i_out[e] = i_new;
    cost_out[e] = cost;
    keep_out[e] = (i_new >= 0 && cost < 0.0) ? 1 : 0;
  }
}

// ---- b. labels --------------------------------------------------------------------------------

__global__ __launch_bounds__(BLOCK) void init_labels_kernel(int32_t *__restrict__ pred_label,
                                                            int64_t n_pred,
                                                            int32_t *__restrict__ gt_label,
                                                            int64_t n_gt) {
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < n_pred + n_gt; e += stride) {
    if (e < n_pred) pred_label[e] = (int32_t)e;
    else gt_label[e - n_pred] = 2147483647;
  }
}

__global__ __launch_bounds__(BLOCK) void sweep_kernel(const int32_t *__restrict__ pi,
                                                      const int32_t *__restrict__ pj, int64_t rows,
                                                      uint32_t n_pred, uint32_t n_gt,
                                                      int32_t *pred_label, int32_t *gt_label,
                                                      int32_t *changed) {
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  bool any = false;
  for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < rows; e += stride) {
    const uint32_t i = (uint32_t)pi[e], j = (uint32_t)pj[e];
    if (i >= n_pred || j >= n_gt) continue;
    const int32_t a = pred_label[i], b = gt_label[j];
    const int32_t m = a < b ? a : b;
    if (a > m) { atomicMin(&pred_label[i], m); any = true; }
    if (b > m) { atomicMin(&gt_label[j], m); any = true; }
  }
  if (any) *changed = 1;                    // every writer writes the same word
}

__global__ __launch_bounds__(BLOCK) void pair_label_kernel(const int32_t *__restrict__ pi,
                                                           int64_t rows, uint32_t n_pred,
                                                           const int32_t *__restrict__ pred_label,
                                                           int32_t *__restrict__ pair_label) {
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < rows; e += stride) {
    const uint32_t i = (uint32_t)pi[e];
    pair_label[e] = i < n_pred ? pred_label[i] : 2147483647;
  }
}

// ---- d. solve ---------------------------------------------------------------------------------

struct SolveLds {
  double cost[CAP * CAP];                   // [worker][job]
  double u[CAP];                            // the workers' potentials
  int32_t rows[CAP], cols[CAP];             // the distinct i and j, in order of first sight
  uint16_t local[CAP * CAP];                // per pair: local row * CAP + local column
};

// The number of `key` in `list` (n entries so far), appending the keys not seen before in lane
// order.  -1 on the lanes that are not live.  *over is raised, for the whole wavefront, when
// the list would pass CAP entries.  n and *over are wave-uniform.
__device__ __forceinline__ int local_of(int32_t key, bool live, int32_t *list, int *n, bool *over) {
  const int lane = threadIdx.x;
  int at = -1;
  for (int k = 0; k < *n; ++k)
    if (live && list[k] == key) at = k;
  bool fresh = live && at < 0;
  unsigned long long m = __ballot(fresh);
  for (int guard = 0; guard < WAVE && m != 0; ++guard) {
    if (*n == CAP) {
      *over = true;
      break;
    }
    const int lead = __ffsll((unsigned long long)m) - 1;
    const int32_t kv = __shfl(key, lead);
    if (lane == lead) list[*n] = kv;
    if (fresh && key == kv) {
      at = *n;
      fresh = false;
    }
    ++*n;
    m = __ballot(fresh);
  }
  __syncthreads();                          // the list as the next chunk reads it
  return at;
}

// pairs [a, b) of one component, b - a >= 2: the assignment, by the whole wavefront.
// true if the component is within the cap (and matched[] is written), false if not.
__device__ bool solve_component(SolveLds &s, const int32_t *__restrict__ pi,
                                const int32_t *__restrict__ pj, const double *__restrict__ cost,
                                int64_t a, int64_t b, int32_t *__restrict__ matched) {
  const int lane = threadIdx.x;
  const int64_t len = b - a;
  if (len > CAP * CAP) return false;        // distinct pairs: more than CAP rows or columns
  __syncthreads();                          // the component before is read
  int nr = 0, nc = 0;
  bool over = false;
  for (int64_t c0 = 0; c0 < len && !over; c0 += WAVE) {
    const bool live = c0 + lane < len;
    const int64_t e = a + c0 + (live ? lane : 0);
    const int r = local_of(pi[e], live, s.rows, &nr, &over);
    if (over) break;
    const int c = local_of(pj[e], live, s.cols, &nc, &over);
    if (live && !over) s.local[c0 + lane] = (uint16_t)(r * CAP + c);
  }
  if (over) return false;
  // the shorter side works: W workers, J jobs, W <= J
  const bool swap = nr > nc;
  const int W = swap ? nc : nr, J = swap ? nr : nc;
  for (int w = 0; w < W; ++w) s.cost[w * CAP + lane] = 0.0;     // absent pairs cost 0
  s.u[lane] = 0.0;
  __syncthreads();
  for (int64_t c0 = 0; c0 < len; c0 += WAVE) {
    if (c0 + lane < len) {
      const int rc = s.local[c0 + lane], r = rc / CAP, c = rc % CAP;
      s.cost[(swap ? c * CAP + r : r * CAP + c)] = fmin(cost[a + c0 + lane], 0.0);
    }
  }
  __syncthreads();

  const bool in = lane < J;
  const double inf = __builtin_huge_val();
  double v = 0.0;                           // this job's potential
  int worker = -1;                          // this job's worker
  for (int w = 0; w < W; ++w) {
    double slack = inf;
    int way = -1;                           // the job before this one on the path; -1: the start
    bool used = false;
    int j0 = -1, i0 = w;
    for (int step = 0; step <= J; ++step) {
      const double ui0 = s.u[i0];
      if (in && !used) {
        const double cur = s.cost[i0 * CAP + lane] - ui0 - v;
        if (cur < slack) {
          slack = cur;
          way = j0;
        }
      }
      // the free job of least slack, the lowest on ties
      double best = (in && !used) ? slack : inf;
      int bj = (in && !used) ? lane : CAP;
#pragma unroll
      for (int off = WAVE / 2; off > 0; off >>= 1) {
        const double ob = __shfl_xor(best, off);
        const int oj = __shfl_xor(bj, off);
        if (ob < best || (ob == best && oj < bj)) {
          best = ob;
          bj = oj;
        }
      }
      if (bj >= CAP) {                      // no free job: cannot happen while W <= J
        j0 = -1;
        break;
      }
      if (in && used) {
        s.u[worker] += best;                // used jobs have workers, all distinct
        v -= best;
      } else if (in) {
        slack -= best;
      }
      if (lane == 0) s.u[w] += best;        // the start of the path stands for worker w
      __syncthreads();
      j0 = bj;
      if (lane == j0) used = true;
      i0 = __shfl(worker, j0);
      if (i0 < 0) break;                    // a free job: the path ends
    }
    // move every worker on the path one job on
    for (int guard = 0; guard <= J && j0 >= 0; ++guard) {
      const int j1 = __shfl(way, j0);
      const int before = __shfl(worker, j1 < 0 ? 0 : j1);
      if (lane == j0) worker = j1 < 0 ? w : before;
      j0 = j1;
    }
  }
  // the assigned pairs of the list: all of them cost less than 0
  s.rows[lane] = worker;                    // reused: job -> worker
  __syncthreads();
  for (int64_t c0 = 0; c0 < len; c0 += WAVE) {
    if (c0 + lane < len) {
      const int rc = s.local[c0 + lane], r = rc / CAP, c = rc % CAP;
      const int wk = swap ? c : r, job = swap ? r : c;
      matched[a + c0 + lane] = s.rows[job] == wk ? 1 : 0;
    }
  }
  return true;
}

__global__ __launch_bounds__(WAVE) void solve_kernel(const int32_t *__restrict__ pi,
                                                     const int32_t *__restrict__ pj,
                                                     const double *__restrict__ cost, int64_t rows,
                                                     const int32_t *__restrict__ starts,
                                                     int64_t n_comp, int32_t *__restrict__ matched,
                                                     int32_t *__restrict__ overflow) {
  __shared__ SolveLds s;
  const int lane = threadIdx.x;
  for (int64_t k0 = (int64_t)blockIdx.x * WAVE; k0 < n_comp; k0 += (int64_t)gridDim.x * WAVE) {
    const int64_t k = k0 + lane;
    int64_t a = 0, b = 0;
    if (k < n_comp) {
      a = starts[k];
      b = starts[k + 1];
      if (a < 0 || b > rows || b < a) a = b = 0;              // not a component of this list
    }
    if (b - a == 1) matched[a] = 1;         // a component of one pair is its own optimum
    unsigned long long todo = __ballot(b - a > 1);
    for (int guard = 0; guard < WAVE && todo != 0; ++guard) {
      const int src = __ffsll(todo) - 1;
      todo &= todo - 1;
      const int64_t ca = __shfl(a, src), cb = __shfl(b, src);
      if (!solve_component(s, pi, pj, cost, ca, cb, matched) && lane == 0) overflow[k0 + src] = 1;
    }
  }
}

// ---- argument checks --------------------------------------------------------------------------

int count_ok(const char *fn, const char *what, int64_t n) { return in_int32_range(fn, what, n, 1); }

int scratch_ok(const char *fn, const void *scratch, int64_t scratch_bytes, int64_t n) {
  if (!aligned(scratch, 8) || scratch_bytes < scratch_for(n))
    return fpla_fail("%s: scratch of %lld bytes, fpla_scratch_bytes asks for %lld (8-byte aligned)",
                     fn, (long long)scratch_bytes, (long long)scratch_for(n));
  return 0;
}

dim3 stride_grid(int64_t n) { return dim3((unsigned)std::min<int64_t>(blocks_of(n), MAX_BLOCKS)); }

}  // namespace

FPLA_EXPORT const char *fpla_last_error(void) try {
  return side_err;
} catch (...) { return "fpla_last_error: C++ exception"; }

FPLA_EXPORT int fpla_abi_version(void) try {
  return FPLA_ABI_VERSION;
} FPLA_CATCH()

FPLA_EXPORT int fpla_scratch_bytes(int64_t n, int64_t *bytes) try {
  if (!bytes) return fpla_fail("fpla_scratch_bytes: null pointer argument");
  if (count_ok("fpla_scratch_bytes", "n", n)) return 1;
  *bytes = scratch_for(n);
  return 0;
} FPLA_CATCH()

FPLA_EXPORT int fpla_flags_count(const int32_t *flags, int64_t n, void *scratch,
                                 int64_t scratch_bytes, int64_t *total, void *stream) try {
  const char *fn = "fpla_flags_count";
  if (!flags || !scratch || !total) return fpla_fail("%s: null pointer argument", fn);
  if (count_ok(fn, "n", n)) return 1;
  if (!aligned(flags, 4)) return fpla_fail("%s: the flags are not 4-byte aligned", fn);
  if (scratch_ok(fn, scratch, scratch_bytes, n)) return 1;
  unsigned long long *sum = (unsigned long long *)scratch;
  uint32_t *cells = (uint32_t *)((char *)scratch + 8);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(count_kernel, dim3((unsigned)blocks_of(n)), dim3(BLOCK), 0, st, flags, n, cells);
  if (launched("fpla_flags_count")) return 1;
  hipLaunchKernelGGL(side_scan_kernel<uint32_t>, dim3(1), dim3(SIDE_SCAN_THREADS), 0, st, cells,
                     (uint32_t)blocks_of(n), sum, nullptr);
  if (launched("fpla_flags_count (scan)")) return 1;
  unsigned long long got = 0;
  if (side_read_back(fn, st, &got, sum, sizeof(got))) return 1;
  *total = (int64_t)got;                    // at most n
  return 0;
} FPLA_CATCH()

FPLA_EXPORT int fpla_flags_fill(const int32_t *flags, int64_t n, const void *scratch,
                                int64_t scratch_bytes, int64_t capacity, const int32_t *a,
                                const int32_t *b, const double *c, int32_t *a_out, int32_t *b_out,
                                double *c_out, int32_t *index_out, int32_t *rank_out,
                                void *stream) try {
  const char *fn = "fpla_flags_fill";
  if (!flags || !scratch) return fpla_fail("%s: null pointer argument", fn);
  if (count_ok(fn, "n", n)) return 1;
  if (in_int32_range(fn, "capacity", capacity, 0)) return 1;
  if ((a_out && !a) || (b_out && !b) || (c_out && !c))
    return fpla_fail("%s: an output column without its input column", fn);
  if (!aligned(flags, 4) || !aligned(a, 4) || !aligned(b, 4) || !aligned(a_out, 4) ||
      !aligned(b_out, 4) || !aligned(index_out, 4) || !aligned(rank_out, 4) || !aligned(c, 8) ||
      !aligned(c_out, 8))
    return fpla_fail("%s: a column is not aligned to its element", fn);
  if (scratch_ok(fn, scratch, scratch_bytes, n)) return 1;
  if (capacity == 0 && !rank_out) return 0;
  const Fill f = {a, b, c, a_out, b_out, c_out, index_out, rank_out};
  const uint32_t *offsets = (const uint32_t *)((const char *)scratch + 8);
  hipLaunchKernelGGL(fill_kernel, dim3((unsigned)blocks_of(n)), dim3(BLOCK), 0, (hipStream_t)stream,
                     flags, n, offsets, capacity, f);
  return launched(fn);
} FPLA_CATCH()

FPLA_EXPORT int fpla_conf_flags(const double *conf, int64_t n, double thd, int32_t *flags,
                                void *stream) try {
  const char *fn = "fpla_conf_flags";
  if (!conf || !flags) return fpla_fail("%s: null pointer argument", fn);
  if (count_ok(fn, "n", n)) return 1;
  if (!aligned(conf, 8) || !aligned(flags, 4))
    return fpla_fail("%s: a column is not aligned to its element", fn);
  hipLaunchKernelGGL(conf_kernel, stride_grid(n), dim3(BLOCK), 0, (hipStream_t)stream, conf, n, thd,
                     flags);
  return launched(fn);
} FPLA_CATCH()

FPLA_EXPORT int fpla_boundaries(const int32_t *keys, int64_t n, int32_t *flags, void *stream) try {
  const char *fn = "fpla_boundaries";
  if (!keys || !flags) return fpla_fail("%s: null pointer argument", fn);
  if (count_ok(fn, "n", n)) return 1;
  if (!aligned(keys, 4) || !aligned(flags, 4))
    return fpla_fail("%s: a column is not aligned to its element", fn);
  hipLaunchKernelGGL(boundary_kernel, stride_grid(n), dim3(BLOCK), 0, (hipStream_t)stream, keys, n,
                     flags);
  return launched(fn);
} FPLA_CATCH()

FPLA_EXPORT int fpla_pair_costs(const int32_t *ti, const int32_t *tj, int64_t rows,
                                const double *pred, int64_t n_pred, const double *gt, int64_t n_gt,
                                double t, const int64_t *pred_lbl, const int64_t *gt_lbl,
                                double label_add, const int32_t *rank, int32_t *i_out,
                                double *cost_out, int32_t *keep_out, void *stream) try {
  const char *fn = "fpla_pair_costs";
  if (!ti || !tj || !pred || !gt || !i_out || !cost_out || !keep_out)
    return fpla_fail("%s: null pointer argument", fn);
  if (count_ok(fn, "rows", rows) || count_ok(fn, "n_pred", n_pred) || count_ok(fn, "n_gt", n_gt))
    return 1;
  if (!std::isfinite(t)) return fpla_fail("%s: the threshold %g is not finite", fn, t);
  if ((pred_lbl == nullptr) != (gt_lbl == nullptr))
    return fpla_fail("%s: labels of one kind only", fn);
  if (pred_lbl && !std::isfinite(label_add))
    return fpla_fail("%s: the label term %g is not finite", fn, label_add);
  if (!aligned(ti, 4) || !aligned(tj, 4) || !aligned(rank, 4) || !aligned(i_out, 4) ||
      !aligned(keep_out, 4) || !aligned(pred, 8) || !aligned(gt, 8) || !aligned(pred_lbl, 8) ||
      !aligned(gt_lbl, 8) || !aligned(cost_out, 8))
    return fpla_fail("%s: a column is not aligned to its element", fn);
  const Costs a = {ti, tj, rows, pred, gt, (uint32_t)n_pred, (uint32_t)n_gt, t, label_add,
                   pred_lbl, gt_lbl, rank};
  hipLaunchKernelGGL(cost_kernel, stride_grid(rows), dim3(BLOCK), 0, (hipStream_t)stream, a, i_out,
                     cost_out, keep_out);
  return launched(fn);
} FPLA_CATCH()

FPLA_EXPORT int fpla_labels(const int32_t *i, const int32_t *j, int64_t rows, int64_t n_pred,
                            int64_t n_gt, int32_t *pred_label, int32_t *gt_label, int32_t *changed,
                            int32_t *pair_label, int64_t max_sweeps, int64_t *sweeps,
                            void *stream) try {
  const char *fn = "fpla_labels";
  if (!i || !j || !pred_label || !gt_label || !changed || !pair_label || !sweeps)
    return fpla_fail("%s: null pointer argument", fn);
  if (count_ok(fn, "rows", rows) || count_ok(fn, "n_pred", n_pred) || count_ok(fn, "n_gt", n_gt))
    return 1;
  if (max_sweeps < 1) return fpla_fail("%s: max_sweeps %lld must be positive", fn, (long long)max_sweeps);
  if (!aligned(i, 4) || !aligned(j, 4) || !aligned(pred_label, 4) || !aligned(gt_label, 4) ||
      !aligned(changed, 4) || !aligned(pair_label, 4))
    return fpla_fail("%s: a column is not aligned to its element", fn);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(init_labels_kernel, stride_grid(n_pred + n_gt), dim3(BLOCK), 0, st, pred_label,
                     n_pred, gt_label, n_gt);
  if (launched("fpla_labels (init)")) return 1;
  int64_t done = 0;
  for (;;) {
    if (done == max_sweeps)
      return fpla_fail("%s: the labels still change after %lld sweeps", fn, (long long)done);
    hipError_t e = hipMemsetAsync(changed, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return fpla_fail("%s: clearing the flag failed: %s", fn, hipGetErrorString(e));
    hipLaunchKernelGGL(sweep_kernel, stride_grid(rows), dim3(BLOCK), 0, st, i, j, rows,
                       (uint32_t)n_pred, (uint32_t)n_gt, pred_label, gt_label, changed);
    if (launched("fpla_labels (sweep)")) return 1;
    ++done;
    int32_t flag = 0;
    e = hipMemcpyAsync(&flag, changed, sizeof(flag), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fpla_fail("%s: reading the flag failed: %s", fn, hipGetErrorString(e));
    if (!flag) break;
  }
  *sweeps = done;
  hipLaunchKernelGGL(pair_label_kernel, stride_grid(rows), dim3(BLOCK), 0, st, i, rows,
                     (uint32_t)n_pred, pred_label, pair_label);
  return launched(fn);
} FPLA_CATCH()

FPLA_EXPORT int fpla_solve(const int32_t *i, const int32_t *j, const double *cost, int64_t rows,
                           const int32_t *starts, int64_t n_comp, int32_t *matched,
                           int32_t *overflow, void *stream) try {
  const char *fn = "fpla_solve";
  if (!i || !j || !cost || !starts || !matched || !overflow)
    return fpla_fail("%s: null pointer argument", fn);
  if (count_ok(fn, "rows", rows) || count_ok(fn, "n_comp", n_comp)) return 1;
  if (n_comp > rows)
    return fpla_fail("%s: %lld components of %lld pairs", fn, (long long)n_comp, (long long)rows);
  if (!aligned(i, 4) || !aligned(j, 4) || !aligned(starts, 4) || !aligned(matched, 4) ||
      !aligned(overflow, 4) || !aligned(cost, 8))
    return fpla_fail("%s: a column is not aligned to its element", fn);
  const int64_t chunks = (n_comp + WAVE - 1) / WAVE;
  // a wavefront per block and 41 984 B of LDS: 3 blocks a CU, 768 resident on 256 CUs
  const unsigned grid = (unsigned)std::min<int64_t>(chunks, FPLA_SOLVE_BLOCKS);
  hipLaunchKernelGGL(solve_kernel, dim3(grid), dim3(WAVE), 0, (hipStream_t)stream, i, j, cost, rows,
                     starts, n_comp, matched, overflow);
  return launched(fn);
} FPLA_CATCH()
