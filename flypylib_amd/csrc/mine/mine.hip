// libfplmine.so (include/fplmine.h): the per-voxel loss of a resident prediction and the
// ordered candidate tables of gen_volume2, for hard-example mining between training rounds.
//
// voxel_loss_kernel.  Elementwise over the flat volume, 10 B per voxel (pred 4, labels 1,
// mask 1, loss 4).  A lane owns 4 consecutive voxels: one float4 of predictions, one packed
// uint32 each of labels and mask, one float4 store - a wave-instruction moves 1 KiB of
// floats.  The volume is contiguous, so the groups run over the FLAT index: X need not be a
// multiple of 4 and no row start need be aligned; a group that crosses a row end carries its
// (z, y, x) over.  Only the base pointers decide whether the packed forms may be used
// (VEC); the last, partial group of a volume goes voxel by voxel.  The grid is capped and
// strides over the groups.  The log is the double-precision one, rounded once to float
// (LOG32 of the header) and taken only for voxels that have a loss; nothing here is a
// multiply-add, so -ffp-contract cannot change a rounding.
//
// Candidate compaction, three launches and no atomics:
//   count_kernel  one wave per chunk of FPLM_CHUNK flat voxels, 16 steps of 64 lanes x 4
//                 voxels; per step four ballots (one per voxel of the lane) and their
//                 popcounts; lane 0 stores the chunk's count.
//   (scan)        side_scan_kernel of csrc/side/side_device.h; the total lands behind the
//                 last chunk.
//   fill_kernel   the count pass again; a row's place is its chunk's offset + the rows of
//                 the steps before + the set ballot bits of lower lanes + the lane's own
//                 earlier voxels: C order, whatever order the waves run in.
// A volume holds at most 2^31 - 1 voxels (checked at the entry points), so flat indices,
// counts and the uint32 divisions that split an index into (z, y, x) are exact; byte
// offsets from the base pointers are formed in size_t.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fplmine.h"
#include "../side/side_abi.h"
#include "../side/side_device.h"

// this library's spelling of the shared shell
#define FPLM_EXPORT SIDE_EXPORT
#define FPLM_CATCH() SIDE_CATCH()
#define fplm_fail side_fail

namespace {

constexpr int BLOCK = 256;                 // 4 waves
constexpr int LANE_VOX = 4;                // voxels per lane and step
constexpr int STEP = 64 * LANE_VOX;        // voxels per wave and step
constexpr int STEPS = FPLM_CHUNK / STEP;   // steps per chunk
constexpr int SCAN_THREADS = 1024;
static_assert(SCAN_THREADS == SIDE_SCAN_THREADS, "the scan is side_scan_kernel's block");
static_assert(FPLM_CHUNK % STEP == 0, "a chunk is a whole number of wave steps");

struct Geometry {
  uint32_t n, d1, d2;       // voxels, Y, X
  int d0, b0, b1, b2;       // Z and the border (edge / half) per axis
};

struct Position {
  uint32_t z, y, x;
  __device__ __forceinline__ void set(const Geometry &g, uint32_t i) {
    const uint32_t r = i / g.d2;
    x = i - r * g.d2;
    z = r / g.d1;
    y = r - z * g.d1;
  }
  __device__ __forceinline__ void next(const Geometry &g) {
    if (++x == g.d2) {
      x = 0;
      if (++y == g.d1) { y = 0; ++z; }
    }
  }
  __device__ __forceinline__ bool inside(const Geometry &g) const {
    return (int)z >= g.b0 && (int)z < g.d0 - g.b0 && (int)y >= g.b1 &&
           (int)y < (int)g.d1 - g.b1 && (int)x >= g.b2 && (int)x < (int)g.d2 - g.b2;
  }
};

struct Thresholds {
  int has0, has1;
  double lo0, hi0, lo1, hi1;
};

__device__ __forceinline__ float voxel_loss(float p, unsigned label, unsigned mask, bool inside,
                                            const Thresholds &t) {
  const bool m = inside && mask == 1u;
  const bool neg = m && label == 0u, pos = m && label == 1u;
  if (!(neg || pos)) return 0.0f;
  const float a = neg ? 1.0f - p : p;
  const float x = a < 1e-8f ? 1e-8f : a;          // a NaN stays one, as in np.maximum
  double l = -(double)(float)log((double)x);
  if (neg && l < 0.005) return 0.0f;              // confident negative
  if (neg ? t.has0 : t.has1) {
    const double lo = neg ? t.lo0 : t.lo1, hi = neg ? t.hi0 : t.hi1;
    l = l < lo ? lo : l;
    l = l > hi ? hi : l;
  }
  return (float)l;
}

template <bool VEC>
__global__ __launch_bounds__(BLOCK) void voxel_loss_kernel(
    const float *__restrict__ pred, const uint8_t *__restrict__ labels,
    const uint8_t *__restrict__ mask, Geometry g, Thresholds t, float *__restrict__ loss) {
  const uint32_t groups = (g.n + LANE_VOX - 1) / LANE_VOX;
  const uint32_t stride = gridDim.x * BLOCK;
  for (uint32_t grp = blockIdx.x * BLOCK + threadIdx.x; grp < groups; grp += stride) {
    const uint32_t i = grp * LANE_VOX;
    const size_t o = i;
    Position q;
    q.set(g, i);
    if (VEC && i + LANE_VOX <= g.n) {
      const float4 p = *reinterpret_cast<const float4 *>(pred + o);
      const uint32_t l4 = *reinterpret_cast<const uint32_t *>(labels + o);
      const uint32_t m4 = *reinterpret_cast<const uint32_t *>(mask + o);
      float4 r;
      r.x = voxel_loss(p.x, l4 & 255u, m4 & 255u, q.inside(g), t);
      q.next(g);
      r.y = voxel_loss(p.y, (l4 >> 8) & 255u, (m4 >> 8) & 255u, q.inside(g), t);
      q.next(g);
      r.z = voxel_loss(p.z, (l4 >> 16) & 255u, (m4 >> 16) & 255u, q.inside(g), t);
      q.next(g);
      r.w = voxel_loss(p.w, l4 >> 24, m4 >> 24, q.inside(g), t);
      *reinterpret_cast<float4 *>(loss + o) = r;
    } else {
      const uint32_t k_end = min((uint32_t)LANE_VOX, g.n - i);
      for (uint32_t k = 0; k < k_end; ++k) {
        loss[o + k] = voxel_loss(pred[o + k], labels[o + k], mask[o + k], q.inside(g), t);
        q.next(g);
      }
    }
  }
}

struct Candidates {
  const uint8_t *labels, *mask;
  const float *weights;      // null: unweighted
  unsigned cc;
};

// bit k: voxel i + k is a candidate; w[k] its weight where the bit is set and weights are given
template <bool VEC>
__device__ __forceinline__ unsigned candidate_bits(const Candidates &c, const Geometry &g,
                                                   uint32_t i, Position &q, float w[LANE_VOX]) {
  if (i >= g.n) return 0u;
  const size_t o = i;
  q.set(g, i);
  Position r = q;
  unsigned bits = 0u;
  if (VEC && i + LANE_VOX <= g.n) {
    const uint32_t l4 = *reinterpret_cast<const uint32_t *>(c.labels + o);
    const uint32_t m4 = *reinterpret_cast<const uint32_t *>(c.mask + o);
#pragma unroll
    for (int k = 0; k < LANE_VOX; ++k) {
      if (((l4 >> (8 * k)) & 255u) == c.cc && ((m4 >> (8 * k)) & 255u) == 1u && r.inside(g))
        bits |= 1u << k;
      r.next(g);
    }
    if (c.weights && bits) {
      const float4 w4 = *reinterpret_cast<const float4 *>(c.weights + o);
      w[0] = w4.x; w[1] = w4.y; w[2] = w4.z; w[3] = w4.w;
#pragma unroll
      for (int k = 0; k < LANE_VOX; ++k)
        if (!(w[k] > 0.0f)) bits &= ~(1u << k);
    }
    return bits;
  }
  const uint32_t k_end = min((uint32_t)LANE_VOX, g.n - i);
#pragma unroll
  for (uint32_t k = 0; k < LANE_VOX; ++k) {
    if (k < k_end && c.labels[o + k] == c.cc && c.mask[o + k] == 1u && r.inside(g)) {
      bool on = true;
      if (c.weights) {
        w[k] = c.weights[o + k];
        on = w[k] > 0.0f;
      }
      if (on) bits |= 1u << k;
    }
    r.next(g);
  }
  return bits;
}

template <bool VEC>
__global__ __launch_bounds__(BLOCK) void count_kernel(Candidates c, Geometry g, uint32_t n_chunks,
                                                      uint32_t *__restrict__ counts) {
  const uint32_t chunk = blockIdx.x * (BLOCK / 64) + threadIdx.x / 64;   // wave-uniform
  if (chunk >= n_chunks) return;
  const uint32_t lane = threadIdx.x & 63;
  uint32_t count = 0;
  for (int s = 0; s < STEPS; ++s) {
    Position q = {0, 0, 0};
    float w[LANE_VOX];
    const unsigned bits =
        candidate_bits<VEC>(c, g, chunk * FPLM_CHUNK + s * STEP + lane * LANE_VOX, q, w);
#pragma unroll
    for (int k = 0; k < LANE_VOX; ++k) count += __popcll(__ballot((bits >> k) & 1u));
  }
  if (lane == 0) counts[chunk] = count;
}

template <bool VEC>
__global__ __launch_bounds__(BLOCK) void fill_kernel(Candidates c, Geometry g, uint32_t n_chunks,
                                                     const uint32_t *__restrict__ offsets,
                                                     uint32_t capacity, int32_t *__restrict__ z_out,
                                                     int32_t *__restrict__ y_out,
                                                     int32_t *__restrict__ x_out,
                                                     float *__restrict__ w_out) {
  const uint32_t chunk = blockIdx.x * (BLOCK / 64) + threadIdx.x / 64;   // wave-uniform
  if (chunk >= n_chunks) return;
  const uint32_t lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t base = offsets[chunk];
  for (int s = 0; s < STEPS; ++s) {
    Position q = {0, 0, 0};
    float w[LANE_VOX];
    const unsigned bits =
        candidate_bits<VEC>(c, g, chunk * FPLM_CHUNK + s * STEP + lane * LANE_VOX, q, w);
    uint32_t rank = 0, step_total = 0;
#pragma unroll
    for (int k = 0; k < LANE_VOX; ++k) {
      const unsigned long long b = __ballot((bits >> k) & 1u);
      rank += __popcll(b & below);
      step_total += __popcll(b);
    }
    uint32_t row = base + rank;       // of this lane's first candidate
#pragma unroll
    for (int k = 0; k < LANE_VOX; ++k) {
      if ((bits >> k) & 1u) {
        if (row < capacity) {
          z_out[row] = (int32_t)q.z;
          y_out[row] = (int32_t)q.y;
          x_out[row] = (int32_t)q.x;
          if (w_out) w_out[row] = w[k];
        }
        ++row;
      }
      q.next(g);
    }
    base += step_total;
  }
}

// dims and border -> Geometry; a message names what is refused
int geometry(const char *fn, const int64_t dims[3], const int32_t border[3], const char *border_name,
             Geometry *g) {
  for (int a = 0; a < 3; ++a) {
    if (dims[a] < 1) return fplm_fail("%s: dims (%lld,%lld,%lld) must be positive", fn,
                                      (long long)dims[0], (long long)dims[1], (long long)dims[2]);
    if (border[a] < 0) return fplm_fail("%s: %s (%d,%d,%d) must not be negative", fn, border_name,
                                        border[0], border[1], border[2]);
  }
  int64_t n;
  if (volume_voxels(fn, dims, "int32 rows and counts", "mine it in parts", &n)) return 1;
  g->n = (uint32_t)n;
  g->d0 = (int)dims[0];
  g->d1 = (uint32_t)dims[1];
  g->d2 = (uint32_t)dims[2];
  // a border beyond the volume selects nothing; clamp it so that d - b cannot overflow
  g->b0 = border[0] > g->d0 ? g->d0 : border[0];
  g->b1 = border[1] > (int)g->d1 ? (int)g->d1 : border[1];
  g->b2 = border[2] > (int)g->d2 ? (int)g->d2 : border[2];
  return 0;
}

uint32_t chunks_of(const Geometry &g) { return (g.n + FPLM_CHUNK - 1) / FPLM_CHUNK; }

int candidate_args(const char *fn, const uint8_t *labels, const uint8_t *mask, const float *weights,
                   const int64_t dims[3], const int32_t half[3], int32_t cc, const void *scratch,
                   int64_t scratch_bytes, Candidates *c, Geometry *g, bool *vec) {
  if (!labels || !mask || !dims || !half || !scratch)
    return fplm_fail("%s: null pointer argument", fn);
  if (cc < 0 || cc > 255) return fplm_fail("%s: class %d is no uint8 label", fn, cc);
  if (geometry(fn, dims, half, "half", g)) return 1;
  if (!aligned(scratch, 4) || scratch_bytes < FPLM_SCRATCH_BYTES(g->n))
    return fplm_fail("%s: scratch of %lld bytes, FPLM_SCRATCH_BYTES asks for %lld (4-byte aligned)",
                     fn, (long long)scratch_bytes, (long long)FPLM_SCRATCH_BYTES(g->n));
  if (weights && !aligned(weights, 4))
    return fplm_fail("%s: weights are not aligned to a float", fn);
  c->labels = labels;
  c->mask = mask;
  c->weights = weights;
  c->cc = (unsigned)cc;
  *vec = aligned(labels, 4) && aligned(mask, 4) && (!weights || aligned(weights, 16));
  return 0;
}

}  // namespace

FPLM_EXPORT const char *fplm_last_error(void) try {
  return side_err;
} catch (...) { return "fplm_last_error: C++ exception"; }

FPLM_EXPORT int fplm_abi_version(void) try {
  return FPLM_ABI_VERSION;
} FPLM_CATCH()

FPLM_EXPORT int fplm_voxel_loss(const float *pred, const uint8_t *labels, const uint8_t *mask,
                                const int64_t dims[3], const int32_t edge[3], int32_t has_l0,
                                double l0_lo, double l0_hi, int32_t has_l1, double l1_lo,
                                double l1_hi, float *loss, void *stream) try {
  if (!pred || !labels || !mask || !dims || !edge || !loss)
    return fplm_fail("fplm_voxel_loss: null pointer argument");
  Geometry g;
  if (geometry("fplm_voxel_loss", dims, edge, "edge", &g)) return 1;
  if (!aligned(pred, 4) || !aligned(loss, 4))
    return fplm_fail("fplm_voxel_loss: pred / loss are not aligned to a float");
  const Thresholds t = {has_l0 != 0, has_l1 != 0, l0_lo, l0_hi, l1_lo, l1_hi};
  const uint32_t groups = (g.n + LANE_VOX - 1) / LANE_VOX;
  // memory-bound: 8 blocks of 256 per CU's worth of grid, the rest by stride
  const uint32_t grid = std::min((groups + BLOCK - 1) / BLOCK, 2048u);
  hipStream_t st = (hipStream_t)stream;
  if (aligned(pred, 16) && aligned(loss, 16) && aligned(labels, 4) && aligned(mask, 4))
    hipLaunchKernelGGL(voxel_loss_kernel<true>, dim3(grid), dim3(BLOCK), 0, st, pred, labels, mask,
                       g, t, loss);
  else
    hipLaunchKernelGGL(voxel_loss_kernel<false>, dim3(grid), dim3(BLOCK), 0, st, pred, labels,
                       mask, g, t, loss);
  return launched("fplm_voxel_loss");
} FPLM_CATCH()

FPLM_EXPORT int fplm_candidates_count(const uint8_t *labels, const uint8_t *mask,
                                      const float *weights, const int64_t dims[3],
                                      const int32_t half[3], int32_t cc, void *scratch,
                                      int64_t scratch_bytes, int64_t *total, void *stream) try {
  Candidates c;
  Geometry g;
  bool vec;
  if (!total) return fplm_fail("fplm_candidates_count: null pointer argument");
  if (candidate_args("fplm_candidates_count", labels, mask, weights, dims, half, cc, scratch,
                     scratch_bytes, &c, &g, &vec))
    return 1;
  const uint32_t n_chunks = chunks_of(g);
  const dim3 grid((n_chunks + BLOCK / 64 - 1) / (BLOCK / 64));
  uint32_t *counts = (uint32_t *)scratch;
  hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(count_kernel<true>, grid, dim3(BLOCK), 0, st, c, g, n_chunks, counts);
  else
    hipLaunchKernelGGL(count_kernel<false>, grid, dim3(BLOCK), 0, st, c, g, n_chunks, counts);
  if (launched("fplm_candidates_count")) return 1;
  hipLaunchKernelGGL(side_scan_kernel<uint32_t>, dim3(1), dim3(SCAN_THREADS), 0, st, counts,
                     n_chunks, nullptr, counts + n_chunks);
  if (launched("fplm_candidates_count (scan)")) return 1;
  uint32_t got = 0;
  if (side_read_back("fplm_candidates_count", st, &got, counts + n_chunks, sizeof(got))) return 1;
  *total = (int64_t)got;
  return 0;
} FPLM_CATCH()

FPLM_EXPORT int fplm_candidates_fill(const uint8_t *labels, const uint8_t *mask,
                                     const float *weights, const int64_t dims[3],
                                     const int32_t half[3], int32_t cc, const void *scratch,
                                     int64_t scratch_bytes, int64_t capacity, int32_t *z_out,
                                     int32_t *y_out, int32_t *x_out, float *w_out,
                                     void *stream) try {
  Candidates c;
  Geometry g;
  bool vec;
  if (candidate_args("fplm_candidates_fill", labels, mask, weights, dims, half, cc, scratch,
                     scratch_bytes, &c, &g, &vec))
    return 1;
  if (capacity < 0 || capacity > SIDE_INT32_MAX)
    return fplm_fail("fplm_candidates_fill: capacity %lld", (long long)capacity);
  if (capacity == 0) return 0;
  if (!z_out || !y_out || !x_out || (weights && !w_out))
    return fplm_fail("fplm_candidates_fill: null pointer argument (an output column)");
  if (!aligned(z_out, 4) || !aligned(y_out, 4) || !aligned(x_out, 4) || !aligned(w_out, 4))
    return fplm_fail("fplm_candidates_fill: an output column is not 4-byte aligned");
  const uint32_t n_chunks = chunks_of(g);
  const dim3 grid((n_chunks + BLOCK / 64 - 1) / (BLOCK / 64));
  const uint32_t *offsets = (const uint32_t *)scratch;
  float *w = weights ? w_out : nullptr;
  hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(fill_kernel<true>, grid, dim3(BLOCK), 0, st, c, g, n_chunks, offsets,
                       (uint32_t)capacity, z_out, y_out, x_out, w);
  else
    hipLaunchKernelGGL(fill_kernel<false>, grid, dim3(BLOCK), 0, st, c, g, n_chunks, offsets,
                       (uint32_t)capacity, z_out, y_out, x_out, w);
  return launched("fplm_candidates_fill");
} FPLM_CATCH()
