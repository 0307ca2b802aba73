// Kernels that read a label volume RESIDENT in device memory, shared by libfplhip.so (v2o.hip:
// fpl_v2o_set_seg with FPL_MEM_DEVICE_BOX fills the context's padded segmentation) and
// libfplseg.so (seg/seg.hip: the same fill into a caller's buffer, and the gather of point labels).
// Device code and its launchers only; the callers check the arguments.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

// zero-padded u64 copy of the box o .. o + (P - 2r) of a (Z,Y,X) label volume of extents E: padded
// voxel (z, y, x) := vol[o + (z, y, x) - r] inside [0, E), else 0 - the r shell and whatever
// part of the box lies outside the volume.  A pure stream: a thread owns SEG_BOX_VEC
// consecutive padded voxels (x innermost), splits its first flat index once and carries
// from there; full groups leave as 16-byte stores (`vec`: dst is 16-byte aligned - a group
// starts at a multiple of SEG_BOX_VEC voxels), the last partial group voxel by voxel.
constexpr int SEG_BOX_VEC = 4;

template <typename T>
__global__ __launch_bounds__(256) void seg_pad_box(
    const T *__restrict__ vol, int64_t E0, int64_t E1, int64_t E2, int64_t o0, int64_t o1,
    int64_t o2, int r, unsigned long long *__restrict__ dst, int64_t P0, int64_t P1, int64_t P2,
    int64_t n_pad, int64_t n_groups, int vec) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n_groups; g += stride) {
    const int64_t i0 = g * SEG_BOX_VEC;
    const int64_t row = i0 / P2;
    int64_t x = i0 - row * P2;
    int64_t z = row / P1;
    int64_t y = row - z * P1;
    unsigned long long v[SEG_BOX_VEC];
#pragma unroll
    for (int k = 0; k < SEG_BOX_VEC; ++k) {
      const int64_t sz = z - r + o0, sy = y - r + o1, sx = x - r + o2;
      // the shell: padded coordinates within r of a face of the padded box
      const bool in = z >= r && y >= r && x >= r && z < P0 - r && y < P1 - r && x < P2 - r &&
                      sz >= 0 && sy >= 0 && sx >= 0 && sz < E0 && sy < E1 && sx < E2 &&
                      i0 + k < n_pad;
      v[k] = in ? (unsigned long long)vol[(sz * E1 + sy) * E2 + sx] : 0ull;
      if (++x == P2) {
        x = 0;
        if (++y == P1) y = 0, ++z;
      }
    }
    if (vec && i0 + SEG_BOX_VEC <= n_pad) {
      ulonglong2 *d2 = reinterpret_cast<ulonglong2 *>(dst + i0);
#pragma unroll
      for (int k = 0; k < SEG_BOX_VEC; k += 2) d2[k / 2] = make_ulonglong2(v[k], v[k + 1]);
    } else {
      for (int k = 0; k < SEG_BOX_VEC && i0 + k < n_pad; ++k) dst[i0 + k] = v[k];
    }
  }
}

// the launch: `seg_bytes` 4 or 8, `pdims` the padded dims (box dims + 2r), `dst` room for their
// product; at most 8 workgroups per CU, the rest by stride
inline void launch_seg_pad_box(const void *vol, int seg_bytes, const int64_t extent[3],
                               const int64_t origin[3], int r, unsigned long long *dst,
                               const int64_t pdims[3], int n_cu, hipStream_t st) {
  const int64_t n_pad = pdims[0] * pdims[1] * pdims[2];
  const int64_t n_groups = (n_pad + SEG_BOX_VEC - 1) / SEG_BOX_VEC;
  const unsigned grid = (unsigned)std::max<int64_t>(
      1, std::min<int64_t>((n_groups + 255) / 256, (int64_t)std::max(n_cu, 1) * 8));
  const int vec = ((uintptr_t)dst & 15) == 0;
  if (seg_bytes == 8)
    seg_pad_box<unsigned long long><<<grid, 256, 0, st>>>(
        (const unsigned long long *)vol, extent[0], extent[1], extent[2], origin[0], origin[1],
        origin[2], r, dst, pdims[0], pdims[1], pdims[2], n_pad, n_groups, vec);
  else
    seg_pad_box<uint32_t><<<grid, 256, 0, st>>>(
        (const uint32_t *)vol, extent[0], extent[1], extent[2], origin[0], origin[1], origin[2], r,
        dst, pdims[0], pdims[1], pdims[2], n_pad, n_groups, vec);
}

// out[i] = vol[zyx[i]] for n (z, y, x) triples; a triple outside [0, E) reads nothing, writes 0
// and raises `overflow`
template <typename T>
__global__ __launch_bounds__(256) void gather_labels(
    const T *__restrict__ vol, int64_t E0, int64_t E1, int64_t E2,
    const long long *__restrict__ zyx, int64_t n, unsigned long long *__restrict__ out,
    unsigned int *__restrict__ overflow) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t z = zyx[3 * i], y = zyx[3 * i + 1], x = zyx[3 * i + 2];
    const bool in = z >= 0 && y >= 0 && x >= 0 && z < E0 && y < E1 && x < E2;
    out[i] = in ? (unsigned long long)vol[(z * E1 + y) * E2 + x] : 0ull;
    if (!in) atomicExch(overflow, 1u);
  }
}

inline void launch_gather_labels(const void *vol, int seg_bytes, const int64_t extent[3],
                                 const long long *zyx, int64_t n, unsigned long long *out,
                                 unsigned int *overflow, hipStream_t st) {
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 2048));
  if (seg_bytes == 8)
    gather_labels<unsigned long long><<<grid, 256, 0, st>>>(
        (const unsigned long long *)vol, extent[0], extent[1], extent[2], zyx, n, out, overflow);
  else
    gather_labels<uint32_t><<<grid, 256, 0, st>>>((const uint32_t *)vol, extent[0], extent[1],
                                                  extent[2], zyx, n, out, overflow);
}
