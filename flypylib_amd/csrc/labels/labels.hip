// libfpllabels.so (include/fpllabels.h): the labels and mask of write_labels_mask from a
// resident roi_mask and a T-bar table, one pass, 3 B per voxel (roi 1, labels 1, mask 1).
//
// labels_mask_kernel.  A gather: the host loop's result depends on the order of the T-bar
// list only through two maxima per voxel (the header's J_set and J_clr), so every voxel can
// look at the T-bars near it in any order and no atomics are needed.  One block of 256
// threads owns a brick of 4 x 8 x 128 voxels (z, y, x).  A lane owns 4 consecutive x voxels
// in each of the brick's 4 z planes (16 voxels: 32 registers of maxima and one of `touched`
// bits); the 32 lanes of a half-wave span the brick's 128 x voxels, so with packed 32-bit
// accesses a wave-instruction moves two whole 128-byte rows.  The block walks its brick's
// candidate list (CSR over the bricks, built by labels.plan_bricks) in pieces of STAGE
// T-bars: each thread fetches one candidate into LDS, then every thread reads them all by
// broadcast.  Cube tests come first, so every squared distance that is compared is that of
// a voxel inside a cube of half-width <= FPLL_MAX_RADIUS and fits an int many times over;
// the differences are formed in unsigned arithmetic, which cannot overflow.  The epilogue
// reads roi, applies the rule and the buffer clear and stores both outputs; a brick with an
// empty list goes straight to it (a copy of roi under the buffer clear, labels 0).  A group
// of 4 voxels is loaded and stored as one uint32 each where the three addresses are 4-byte
// aligned and the group lies inside the row, voxel by voxel otherwise (odd X, views that
// start at an odd byte, the end of a row).
#include <hip/hip_runtime.h>

#include "fpllabels.h"
#include "../side/side_abi.h"

// this library's spelling of the shared shell
#define FPLL_EXPORT SIDE_EXPORT
#define FPLL_CATCH() SIDE_CATCH()
#define fpll_fail side_fail

namespace {

constexpr int BLOCK = 256;                 // 4 waves
constexpr int BZ = FPLL_BRICK_Z, BY = FPLL_BRICK_Y, BX = FPLL_BRICK_X;
constexpr int LANE_VOX = 4;                // consecutive x voxels per lane and z plane
constexpr int STAGE = 256;                 // candidates staged through LDS at once
static_assert(BX == 32 * LANE_VOX && BX / LANE_VOX * BY == BLOCK, "one lane per (y, x group)");
static_assert(STAGE == BLOCK, "each thread stages one candidate");

struct Geometry {
  int d0, d1, d2;           // Z, Y, X
  int nb1, nb2;             // bricks along y and x
  int b0, b1, b2;           // the cleared border per axis, clamped to the extent
};

struct Rule {
  int n_tbars, n_index;
  unsigned use2, ign2;      // squared radii
  int has_ign;              // radius_ign > 0
  int rmax;                 // half-width of the larger cube
};

// |a - b| <= r, and a - b as an unsigned difference (its square is exact where this holds)
__device__ __forceinline__ bool near(int a, int b, int r, unsigned &d) {
  d = (unsigned)a - (unsigned)b;
  return d + (unsigned)r <= 2u * (unsigned)r;
}

__global__ __launch_bounds__(BLOCK) void labels_mask_kernel(
    const uint8_t *__restrict__ roi, const int32_t *__restrict__ tbars,
    const int32_t *__restrict__ brick_offsets, const int32_t *__restrict__ brick_index, Geometry g,
    Rule r, uint8_t *__restrict__ labels, uint8_t *__restrict__ mask) {
  __shared__ int4 staged[STAGE];            // (x, y, z, j); j < 0: skip
  const int t = threadIdx.x;
  const unsigned brick = blockIdx.x;
  const int bx = (int)(brick % (unsigned)g.nb2);
  const unsigned rest = brick / (unsigned)g.nb2;
  const int by = (int)(rest % (unsigned)g.nb1), bz = (int)(rest / (unsigned)g.nb1);
  const int x0 = bx * BX + (t & 31) * LANE_VOX, y = by * BY + (t >> 5), z0 = bz * BZ;
  const bool live = y < g.d1 && x0 < g.d2;  // the lane has voxels inside the volume

  int jset[BZ][LANE_VOX], jclr[BZ][LANE_VOX];
#pragma unroll
  for (int zz = 0; zz < BZ; ++zz)
#pragma unroll
    for (int k = 0; k < LANE_VOX; ++k) jset[zz][k] = jclr[zz][k] = -1;
  unsigned touched = 0;                     // bit zz * LANE_VOX + k

  int beg = 0, end = 0;
  if (brick_offsets && r.n_index > 0) {
    beg = max(brick_offsets[brick], 0);
    end = min(brick_offsets[brick + 1], r.n_index);
  }
  for (int c = beg; c < end; c += STAGE) {  // block-uniform
    const int n = min(STAGE, end - c);
    if (t < n) {
      const int j = brick_index[c + t];
      int4 e = make_int4(0, 0, 0, -1);
      if (j >= 0 && j < r.n_tbars) {
        const int32_t *p = tbars + (size_t)j * 3;
        e = make_int4(p[0], p[1], p[2], j);
      }
      staged[t] = e;
    }
    __syncthreads();
    if (live) {
      for (int i = 0; i < n; ++i) {
        const int4 e = staged[i];
        unsigned dy, dx[LANE_VOX];
        if (e.w < 0 || !near(y, e.y, r.rmax, dy)) continue;
        unsigned in_x = 0;
#pragma unroll
        for (int k = 0; k < LANE_VOX; ++k)
          if (near(x0 + k, e.x, r.rmax, dx[k])) in_x |= 1u << k;
        if (!in_x) continue;
        const unsigned dy2 = dy * dy;
#pragma unroll
        for (int k = 0; k < LANE_VOX; ++k) dx[k] *= dx[k];
#pragma unroll
        for (int zz = 0; zz < BZ; ++zz) {
          unsigned dz;
          if (!near(z0 + zz, e.z, r.rmax, dz)) continue;
          const unsigned dzy2 = dz * dz + dy2;
          touched |= in_x << (zz * LANE_VOX);
#pragma unroll
          for (int k = 0; k < LANE_VOX; ++k) {
            const bool in = (in_x >> k) & 1u;
            const unsigned d2 = dzy2 + dx[k];
            if (in && d2 <= r.use2) jset[zz][k] = max(jset[zz][k], e.w);
            if (in && r.has_ign && d2 <= r.ign2) jclr[zz][k] = max(jclr[zz][k], e.w);
          }
        }
      }
    }
    __syncthreads();
  }
  if (!live) return;

  const bool keep_y = y >= g.b1 && y < g.d1 - g.b1;
  unsigned keep_x = 0;
#pragma unroll
  for (int k = 0; k < LANE_VOX; ++k)
    if (x0 + k >= g.b2 && x0 + k < g.d2 - g.b2) keep_x |= 1u << k;
#pragma unroll
  for (int zz = 0; zz < BZ; ++zz) {
    const int z = z0 + zz;
    if (z >= g.d0) break;
    const bool keep_zy = keep_y && z >= g.b0 && z < g.d0 - g.b0;
    const size_t o = ((size_t)z * g.d1 + y) * g.d2 + x0;
    const bool packed =
        x0 + LANE_VOX <= g.d2 &&
        ((((uintptr_t)(roi + o)) | ((uintptr_t)(labels + o)) | ((uintptr_t)(mask + o))) & 3u) == 0;
    uint32_t in4 = 0;
    if (packed) {
      in4 = *reinterpret_cast<const uint32_t *>(roi + o);
    } else {
#pragma unroll
      for (int k = 0; k < LANE_VOX; ++k)
        if (x0 + k < g.d2) in4 |= (uint32_t)roi[o + k] << (8 * k);
    }
    uint32_t l4 = 0, m4 = 0;
#pragma unroll
    for (int k = 0; k < LANE_VOX; ++k) {
      const unsigned v = (in4 >> (8 * k)) & 255u;
      const int js = jset[zz][k], jc = jclr[zz][k];
      unsigned m;
      if (js >= 0 && js >= jc) m = 1u;
      else if (jc >= 0) m = 0u;
      else if ((touched >> (zz * LANE_VOX + k)) & 1u) m = v != 0u;
      else m = v;
      if (!(keep_zy && ((keep_x >> k) & 1u))) m = 0u;
      l4 |= (js >= 0 ? 1u : 0u) << (8 * k);
      m4 |= m << (8 * k);
    }
    if (packed) {
      *reinterpret_cast<uint32_t *>(labels + o) = l4;
      *reinterpret_cast<uint32_t *>(mask + o) = m4;
    } else {
#pragma unroll
      for (int k = 0; k < LANE_VOX; ++k)
        if (x0 + k < g.d2) {
          labels[o + k] = (uint8_t)(l4 >> (8 * k));
          mask[o + k] = (uint8_t)(m4 >> (8 * k));
        }
    }
  }
}

}  // namespace

FPLL_EXPORT const char *fpll_last_error(void) try {
  return side_err;
} catch (...) { return "fpll_last_error: C++ exception"; }

FPLL_EXPORT int fpll_abi_version(void) try {
  return FPLL_ABI_VERSION;
} FPLL_CATCH()

FPLL_EXPORT int fpll_labels_mask(const uint8_t *roi, const int32_t *tbars, int64_t n_tbars,
                                 const int32_t *brick_offsets, const int32_t *brick_index,
                                 int64_t n_index, const int64_t dims[3], int32_t radius_use,
                                 int32_t radius_ign, int32_t buffer_size, uint8_t *labels,
                                 uint8_t *mask, void *stream) try {
  const char *fn = "fpll_labels_mask";
  if (!roi || !dims || !labels || !mask) return fpll_fail("%s: null pointer argument", fn);
  for (int a = 0; a < 3; ++a)
    if (dims[a] < 1) return fpll_fail("%s: dims (%lld,%lld,%lld) must be positive", fn,
                                      (long long)dims[0], (long long)dims[1], (long long)dims[2]);
  int64_t voxels;
  if (volume_voxels(fn, dims, "the brick tables", "render it in parts", &voxels)) return 1;
  if (radius_use < 0 || radius_ign < 0 || radius_use > FPLL_MAX_RADIUS ||
      radius_ign > FPLL_MAX_RADIUS)
    return fpll_fail("%s: radius_use %d / radius_ign %d must lie in [0, %d]", fn, radius_use,
                     radius_ign, FPLL_MAX_RADIUS);
  if (buffer_size < 0) return fpll_fail("%s: buffer_size %d must not be negative", fn, buffer_size);
  if (n_tbars < 0 || n_tbars > SIDE_INT32_MAX / 3 || n_index < 0 || n_index > SIDE_INT32_MAX)
    return fpll_fail("%s: n_tbars %lld / n_index %lld", fn, (long long)n_tbars, (long long)n_index);
  if (n_index > 0 && (!tbars || !brick_offsets || !brick_index || n_tbars == 0))
    return fpll_fail("%s: null pointer argument (a table of %lld candidates)", fn,
                     (long long)n_index);
  if (!aligned(tbars, 4) || !aligned(brick_offsets, 4) || !aligned(brick_index, 4))
    return fpll_fail("%s: a table is not aligned to an int32", fn);
  const size_t n = (size_t)voxels;
  if (roi == labels || roi == mask || labels == mask ||
      (labels < mask ? labels + n > mask : mask + n > labels))
    return fpll_fail("%s: roi, labels and mask must be distinct buffers", fn);

  Geometry g;
  g.d0 = (int)dims[0];
  g.d1 = (int)dims[1];
  g.d2 = (int)dims[2];
  const int64_t nb0 = (dims[0] + BZ - 1) / BZ;
  g.nb1 = (int)((dims[1] + BY - 1) / BY);
  g.nb2 = (int)((dims[2] + BX - 1) / BX);
  const int64_t bricks = nb0 * g.nb1 * g.nb2;
  if (bricks > SIDE_INT32_MAX)
    return fpll_fail("%s: %lld bricks exceed a grid", fn, (long long)bricks);
  // buffer_size 0 clears everything (mask[-0:] = 0 on the host), as does one beyond an extent
  const int64_t b = buffer_size == 0 ? SIDE_INT32_MAX : buffer_size;
  g.b0 = (int)(b > dims[0] ? dims[0] : b);
  g.b1 = (int)(b > dims[1] ? dims[1] : b);
  g.b2 = (int)(b > dims[2] ? dims[2] : b);
  Rule r;
  r.n_tbars = (int)n_tbars;
  r.n_index = (int)n_index;
  r.use2 = (unsigned)(radius_use * radius_use);
  r.ign2 = (unsigned)(radius_ign * radius_ign);
  r.has_ign = radius_ign > 0;
  r.rmax = radius_use > radius_ign ? radius_use : radius_ign;
  hipLaunchKernelGGL(labels_mask_kernel, dim3((unsigned)bricks), dim3(BLOCK), 0,
                     (hipStream_t)stream, roi, tbars, brick_offsets, brick_index, g, r, labels,
                     mask);
  return launched(fn);
} FPLL_CATCH()
