// libfplroi.so (include/fplroi.h): the region of interest on the GPU.  The ROI is three small
// resident tables - the sorted keys of its block rows, a CSR row start, the (x0, x1) of every run -
// and four kernels read them: the uint8 mask of a box, point queries, voxel counts of boxes, and
// (without the tables) the cut-and-normalise of a training cube.  All four are bound by their
// stores or are tiny; none uses an atomic, and none waits for its stream.
#include <hip/hip_runtime.h>

#include "fplroi.h"
#include "../side/side_abi.h"

#define FPLR_EXPORT SIDE_EXPORT
#define FPLR_CATCH() SIDE_CATCH()
#define fplr_fail side_fail

namespace {

constexpr long long BLOCK_COORD_LIM = 1LL << 31;       // block coordinates are int32
constexpr int64_t SIDE_LIM = (int64_t)1 << FPLR_SIDE_BITS;
constexpr int64_t COORD_LIM = (int64_t)1 << FPLR_COORD_BITS;
constexpr int WAVES = FPLR_BLOCK / 64;

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Roi {
  const long long *keys;
  const int *row_start;
  const int *runs_x;
  int n_rows;
  int block;
};

// Python's a // b for b > 0
__device__ __forceinline__ long long floor_div(long long a, long long b) {
  const long long q = a / b;
  return q - ((a % b != 0) && (a < 0));
}

// the index of block row (bz, by) in the keys, or -1
__device__ __forceinline__ int find_row(const Roi &roi, long long bz, long long by) {
  if (bz < -BLOCK_COORD_LIM || bz >= BLOCK_COORD_LIM || by < -BLOCK_COORD_LIM || by >= BLOCK_COORD_LIM)
    return -1;
  const long long key = bz * (1LL << 32) + (by + (1LL << 31));
  int lo = 0, hi = roi.n_rows;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (roi.keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return (lo < roi.n_rows && roi.keys[lo] == key) ? lo : -1;
}

// 0x01 in bytes lo .. hi - 1 of eight (0 <= lo, hi <= 8), 0x00 in the others
__device__ __forceinline__ unsigned long long span_bytes(int lo, int hi) {
  if (hi <= lo) return 0;
  const unsigned long long m = (~0ULL >> (64 - 8 * (hi - lo))) << (8 * lo);
  return m & 0x0101010101010101ULL;
}

__device__ __forceinline__ int clamp16(long long v) { return v < 0 ? 0 : (v > 16 ? 16 : (int)v); }

// whether the voxel at box-local x lies in one of the runs r0 .. r1 of a row
__device__ __forceinline__ unsigned char byte_of(const Roi &roi, int r0, int r1, long long ox, int x) {
  unsigned char in = 0;
  for (int k = r0; k < r1; ++k) {
    const long long a = (long long)roi.runs_x[2 * k] * roi.block - ox;
    const long long b = ((long long)roi.runs_x[2 * k + 1] + 1) * roi.block - ox;
    in |= (unsigned char)(x >= a && x < b);
  }
  return in;
}

// A wave per voxel row (z, y) of the box, grid stride over the rows.  The row's block row is
// found once (uniform over the wave); lanes then take the row's 16-byte aligned vectors, each
// walking the row's runs, and the first lanes the bytes before and after the aligned body.
__global__ __launch_bounds__(FPLR_BLOCK) void fplr_mask_box_kernel(
    Roi roi, long long oz, long long oy, long long ox, int Z, int Y, int X, unsigned char *out) {
  const int lane = threadIdx.x & 63;
  const int rows = Z * Y;
  for (long long row = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6); row < rows;
       row += (long long)gridDim.x * WAVES) {
    const int z = (int)(row / Y), y = (int)(row - (long long)z * Y);
    const int r = find_row(roi, floor_div(oz + z, roi.block), floor_div(oy + y, roi.block));
    int r0 = 0, r1 = 0;
    if (r >= 0) { r0 = roi.row_start[r]; r1 = roi.row_start[r + 1]; }
    unsigned char *dst = out + row * X;
    int head = (int)((16 - ((uintptr_t)dst & 15)) & 15);
    if (head > X) head = X;
    const int nvec = (X - head) >> 4;
    const int tail0 = head + (nvec << 4);
    for (int v = lane; v < nvec; v += 64) {
      const int p = head + (v << 4);
      unsigned long long w0 = 0, w1 = 0;
      for (int k = r0; k < r1; ++k) {
        const long long a = (long long)roi.runs_x[2 * k] * roi.block - ox - p;
        const long long b = ((long long)roi.runs_x[2 * k + 1] + 1) * roi.block - ox - p;
        const int l = clamp16(a), h = clamp16(b);
        w0 |= span_bytes(l < 8 ? l : 8, h < 8 ? h : 8);
        w1 |= span_bytes((l > 8 ? l : 8) - 8, (h > 8 ? h : 8) - 8);
      }
      u32x4 w;
      w.x = (unsigned int)w0; w.y = (unsigned int)(w0 >> 32);
      w.z = (unsigned int)w1; w.w = (unsigned int)(w1 >> 32);
      *reinterpret_cast<u32x4 *>(dst + p) = w;
    }
    if (lane < head) dst[lane] = byte_of(roi, r0, r1, ox, lane);
    if (lane < X - tail0) dst[tail0 + lane] = byte_of(roi, r0, r1, ox, tail0 + lane);
  }
}

__global__ __launch_bounds__(FPLR_BLOCK) void fplr_ptquery_kernel(
    Roi roi, const long long *zyx, long long n, unsigned char *flags) {
  const long long i = (long long)blockIdx.x * FPLR_BLOCK + threadIdx.x;
  if (i >= n) return;
  const long long bz = floor_div(zyx[3 * i], roi.block), by = floor_div(zyx[3 * i + 1], roi.block);
  const long long bx = floor_div(zyx[3 * i + 2], roi.block);
  unsigned char in = 0;
  const int r = find_row(roi, bz, by);
  if (r >= 0 && bx >= -BLOCK_COORD_LIM && bx < BLOCK_COORD_LIM) {
    // the last run of the row with x0 <= bx
    int lo = roi.row_start[r], hi = roi.row_start[r + 1];
    const int first = lo;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (roi.runs_x[2 * mid] <= bx) lo = mid + 1; else hi = mid;
    }
    in = (unsigned char)(lo > first && bx <= roi.runs_x[2 * (lo - 1) + 1]);
  }
  flags[i] = in;
}

__device__ __forceinline__ long long overlap(long long lo, long long hi, long long blo, long long bhi) {
  const long long a = lo > blo ? lo : blo, b = hi < bhi ? hi : bhi;
  return b > a ? b - a : 0;
}

// A workgroup per box: thread t sums the block rows t, t + FPLR_BLOCK, ... in int64, the partial
// sums meet in LDS in a fixed tree.
__global__ __launch_bounds__(FPLR_BLOCK) void fplr_box_counts_kernel(
    Roi roi, const long long *boxes, long long *counts) {
  __shared__ long long part[FPLR_BLOCK];
  const long long *box = boxes + 6 * (long long)blockIdx.x;
  const long long z = box[0], y = box[1], x = box[2], dz = box[3], dy = box[4], dx = box[5];
  const bool ok = dz >= 0 && dy >= 0 && dx >= 0 && dz < SIDE_LIM && dy < SIDE_LIM && dx < SIDE_LIM &&
                  z > -COORD_LIM && z < COORD_LIM && y > -COORD_LIM && y < COORD_LIM &&
                  x > -COORD_LIM && x < COORD_LIM;
  const long long b = roi.block;
  long long acc = 0;
  if (ok)
    for (int r = threadIdx.x; r < roi.n_rows; r += FPLR_BLOCK) {
      const long long key = roi.keys[r];
      const long long bz = key >> 32, by = (key & 0xffffffffLL) - (1LL << 31);
      const long long nz = overlap(z, z + dz, bz * b, (bz + 1) * b);
      const long long ny = overlap(y, y + dy, by * b, (by + 1) * b);
      if (nz == 0 || ny == 0) continue;
      long long nx = 0;
      for (int k = roi.row_start[r]; k < roi.row_start[r + 1]; ++k)
        nx += overlap(x, x + dx, (long long)roi.runs_x[2 * k] * b,
                      ((long long)roi.runs_x[2 * k + 1] + 1) * b);
      acc += nz * ny * nx;
    }
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int s = FPLR_BLOCK / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[blockIdx.x] = part[0];
}

// Thread g writes the four floats that share one 16-byte aligned address: the flat elements
// 4 g - mis .. 4 g - mis + 3 (`mis`: the floats by which `out` lies past such an address).  The
// first and the last group may be cut by the ends of the buffer and are written float by float.
__global__ __launch_bounds__(FPLR_BLOCK) void fplr_cut_normalize_kernel(
    const unsigned char *vol, long long EZ, long long EY, long long EX, long long oz, long long oy,
    long long ox, int Y, int X, long long n, int mis, float mean, float sd, float *out) {
  const long long first = 4 * ((long long)blockIdx.x * FPLR_BLOCK + threadIdx.x) - mis;
  if (first >= n) return;
  const long long e0 = first < 0 ? 0 : first;
  const long long e1 = first + 4 < n ? first + 4 : n;
  const long long plane = (long long)Y * X;
  int z = (int)(e0 / plane);
  const int rem = (int)(e0 - z * plane);
  int y = rem / X, x = rem - y * X;
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long e = first + k;
    v[k] = 0.f;
    if (e >= e0 && e < e1) {
      const long long gz = oz + z, gy = oy + y, gx = ox + x;
      unsigned char u = 0;
      if (gz >= 0 && gz < EZ && gy >= 0 && gy < EY && gx >= 0 && gx < EX)
        u = vol[(gz * EY + gy) * EX + gx];
      v[k] = __fdiv_rn(__fsub_rn((float)u, mean), sd);
      if (++x == X) { x = 0; if (++y == Y) { y = 0; ++z; } }
    }
  }
  if (e1 - e0 == 4) {
    f32x4 w;
    w.x = v[0]; w.y = v[1]; w.z = v[2]; w.w = v[3];
    *reinterpret_cast<f32x4 *>(out + first) = w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (first + k >= e0 && first + k < e1) out[first + k] = v[k];
  }
}

// 0 when `p` is device memory
int device_pointer(const char *fn, const char *what, const void *p) {
  hipPointerAttribute_t attr;
  const hipError_t e = hipPointerGetAttributes(&attr, p);
  if (e != hipSuccess) (void)hipGetLastError();          // plain host memory on older runtimes
  if (e != hipSuccess || attr.type != hipMemoryTypeDevice)
    return fplr_fail("%s: %s must be device memory", fn, what);
  return 0;
}

// the three tables of every ROI entry point
int tables_ok(const char *fn, const int64_t *row_keys, const int32_t *row_start, const int32_t *runs_x,
              int64_t n_rows, int64_t n_runs, int32_t block_size) {
  if (!row_keys || !row_start || !runs_x) return fplr_fail("%s: null pointer argument", fn);
  if (in_int32_range(fn, "n_rows", n_rows, 0) || in_int32_range(fn, "n_runs", n_runs, 0)) return 1;
  if (n_runs < n_rows || (n_rows == 0 && n_runs != 0))
    return fplr_fail("%s: %lld runs in %lld rows", fn, (long long)n_runs, (long long)n_rows);
  if (block_size < 1 || block_size > (1 << FPLR_BLOCK_SIZE_BITS))
    return fplr_fail("%s: block_size %d must lie in [1, 2^%d]", fn, block_size, FPLR_BLOCK_SIZE_BITS);
  if (!aligned(row_keys, 8)) return fplr_fail("%s: row_keys is not 8-byte aligned", fn);
  if (!aligned(row_start, 4) || !aligned(runs_x, 4))
    return fplr_fail("%s: row_start / runs_x is not 4-byte aligned", fn);
  return 0;
}

// a box of (z, y, x): sides in [1, 2^21), fewer than 2^31 voxels, origin within +-2^40
int box_ok(const char *fn, const int64_t origin[3], const int64_t dims[3], int64_t *n) {
  if (!origin || !dims) return fplr_fail("%s: null pointer argument", fn);
  for (int a = 0; a < 3; ++a) {
    if (dims[a] < 1 || dims[a] >= SIDE_LIM)
      return fplr_fail("%s: dims[%d] %lld must lie in [1, 2^%d)", fn, a, (long long)dims[a],
                       FPLR_SIDE_BITS);
    if (origin[a] <= -COORD_LIM || origin[a] >= COORD_LIM)
      return fplr_fail("%s: origin[%d] %lld lies outside +-2^%d", fn, a, (long long)origin[a],
                       FPLR_COORD_BITS);
  }
  return volume_voxels(fn, dims, "a box", "render it in parts", n);
}

Roi roi_of(const int64_t *row_keys, const int32_t *row_start, const int32_t *runs_x, int64_t n_rows,
           int32_t block_size) {
  Roi r;
  r.keys = (const long long *)row_keys;
  r.row_start = row_start;
  r.runs_x = runs_x;
  r.n_rows = (int)n_rows;
  r.block = block_size;
  return r;
}

}  // namespace

FPLR_EXPORT const char *fplr_last_error(void) try {
  return side_err;
} catch (...) { return "fplr_last_error: C++ exception"; }

FPLR_EXPORT int fplr_abi_version(void) try {
  return FPLR_ABI_VERSION;
} FPLR_CATCH()

FPLR_EXPORT int fplr_mask_box(const int64_t *row_keys, const int32_t *row_start, const int32_t *runs_x,
                              int64_t n_rows, int64_t n_runs, int32_t block_size,
                              const int64_t origin[3], const int64_t dims[3], uint8_t *out,
                              void *stream) try {
  const char *fn = "fplr_mask_box";
  if (tables_ok(fn, row_keys, row_start, runs_x, n_rows, n_runs, block_size)) return 1;
  int64_t n = 0;
  if (box_ok(fn, origin, dims, &n)) return 1;
  if (!out) return fplr_fail("%s: null pointer argument", fn);
  if (device_pointer(fn, "out", out)) return 1;
  const int64_t rows = dims[0] * dims[1];
  const int64_t want = (rows + WAVES - 1) / WAVES;
  const unsigned grid = (unsigned)(want < FPLR_MAX_GRID ? want : FPLR_MAX_GRID);
  hipLaunchKernelGGL(fplr_mask_box_kernel, dim3(grid), dim3(FPLR_BLOCK), 0, (hipStream_t)stream,
                     roi_of(row_keys, row_start, runs_x, n_rows, block_size), (long long)origin[0],
                     (long long)origin[1], (long long)origin[2], (int)dims[0], (int)dims[1],
                     (int)dims[2], out);
  return launched(fn);
} FPLR_CATCH()

FPLR_EXPORT int fplr_ptquery(const int64_t *row_keys, const int32_t *row_start, const int32_t *runs_x,
                             int64_t n_rows, int64_t n_runs, int32_t block_size, const int64_t *zyx,
                             int64_t n, uint8_t *flags, void *stream) try {
  const char *fn = "fplr_ptquery";
  if (tables_ok(fn, row_keys, row_start, runs_x, n_rows, n_runs, block_size)) return 1;
  if (in_int32_range(fn, "n", n, 0)) return 1;
  if (n == 0) return 0;
  if (!zyx || !flags) return fplr_fail("%s: null pointer argument", fn);
  if (!aligned(zyx, 8)) return fplr_fail("%s: zyx is not 8-byte aligned", fn);
  if (device_pointer(fn, "flags", flags)) return 1;
  const unsigned grid = (unsigned)((n + FPLR_BLOCK - 1) / FPLR_BLOCK);
  hipLaunchKernelGGL(fplr_ptquery_kernel, dim3(grid), dim3(FPLR_BLOCK), 0, (hipStream_t)stream,
                     roi_of(row_keys, row_start, runs_x, n_rows, block_size), (const long long *)zyx,
                     (long long)n, flags);
  return launched(fn);
} FPLR_CATCH()

FPLR_EXPORT int fplr_box_counts(const int64_t *row_keys, const int32_t *row_start,
                                const int32_t *runs_x, int64_t n_rows, int64_t n_runs,
                                int32_t block_size, const int64_t *boxes, int64_t n_boxes,
                                int64_t *counts, void *stream) try {
  const char *fn = "fplr_box_counts";
  if (tables_ok(fn, row_keys, row_start, runs_x, n_rows, n_runs, block_size)) return 1;
  if (in_int32_range(fn, "n_boxes", n_boxes, 0)) return 1;
  if (n_boxes == 0) return 0;
  if (!boxes || !counts) return fplr_fail("%s: null pointer argument", fn);
  if (!aligned(boxes, 8) || !aligned(counts, 8))
    return fplr_fail("%s: boxes / counts is not 8-byte aligned", fn);
  if (device_pointer(fn, "counts", counts)) return 1;
  hipLaunchKernelGGL(fplr_box_counts_kernel, dim3((unsigned)n_boxes), dim3(FPLR_BLOCK), 0,
                     (hipStream_t)stream, roi_of(row_keys, row_start, runs_x, n_rows, block_size),
                     (const long long *)boxes, (long long *)counts);
  return launched(fn);
} FPLR_CATCH()

FPLR_EXPORT int fplr_cut_normalize_u8(const uint8_t *vol, const int64_t extent[3],
                                      const int64_t origin[3], const int64_t dims[3], float mean,
                                      float std, float *out, void *stream) try {
  const char *fn = "fplr_cut_normalize_u8";
  if (!vol || !extent || !out) return fplr_fail("%s: null pointer argument", fn);
  for (int a = 0; a < 3; ++a)
    if (extent[a] < 1 || extent[a] >= SIDE_LIM)
      return fplr_fail("%s: extent[%d] %lld must lie in [1, 2^%d)", fn, a, (long long)extent[a],
                       FPLR_SIDE_BITS);
  int64_t n = 0;
  if (box_ok(fn, origin, dims, &n)) return 1;
  if (!aligned(out, 4)) return fplr_fail("%s: out is not 4-byte aligned", fn);
  if (device_pointer(fn, "vol", vol) || device_pointer(fn, "out", out)) return 1;
  const int mis = (int)(((uintptr_t)out >> 2) & 3);
  const int64_t groups = (n + mis + 3) / 4;
  const unsigned grid = (unsigned)((groups + FPLR_BLOCK - 1) / FPLR_BLOCK);
  hipLaunchKernelGGL(fplr_cut_normalize_kernel, dim3(grid), dim3(FPLR_BLOCK), 0, (hipStream_t)stream,
                     vol, (long long)extent[0], (long long)extent[1], (long long)extent[2],
                     (long long)origin[0], (long long)origin[1], (long long)origin[2], (int)dims[1],
                     (int)dims[2], (long long)n, mis, mean, std, out);
  return launched(fn);
} FPLR_CATCH()
