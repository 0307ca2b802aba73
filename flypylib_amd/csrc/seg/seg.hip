// libfplseg.so (include/fplseg.h): the labels of points of a label volume resident in device
// memory, and the padded u64 copy of a box of it.  The kernels and their launchers are
// csrc/seg_box.h, shared with libfplhip.so's fpl_v2o_set_seg.
#include <hip/hip_runtime.h>

#include "fplseg.h"
#include "../side/side_abi.h"
#include "../seg_box.h"

#define FPLS_EXPORT SIDE_EXPORT
#define FPLS_CATCH() SIDE_CATCH()
#define fpls_fail side_fail

namespace {

constexpr int64_t COORD_LIM = (int64_t)1 << 21;

// device memory freed on every way out
struct DevBlock {
  void *p = nullptr;
  ~DevBlock() { if (p) (void)hipFree(p); }
};

int hip_ok(const char *fn, const char *what, hipError_t e) {
  if (e != hipSuccess) return fpls_fail("%s: %s: %s", fn, what, hipGetErrorString(e));
  return 0;
}

// 0 when `p` is device memory
int device_pointer(const char *fn, const char *what, const void *p) {
  hipPointerAttribute_t attr;
  const hipError_t e = hipPointerGetAttributes(&attr, p);
  if (e != hipSuccess) (void)hipGetLastError();          // plain host memory on older runtimes
  if (e != hipSuccess || attr.type != hipMemoryTypeDevice)
    return fpls_fail("%s: %s must be device memory", fn, what);
  return 0;
}

int volume_ok(const char *fn, const void *vol, int32_t seg_bytes, const int64_t extent[3]) {
  if (!vol || !extent) return fpls_fail("%s: null pointer argument", fn);
  if (seg_bytes != 4 && seg_bytes != 8) return fpls_fail("%s: labels must be 4 or 8 bytes", fn);
  for (int a = 0; a < 3; ++a)
    if (extent[a] <= 0 || extent[a] >= COORD_LIM)
      return fpls_fail("%s: axis %d out of the 2^21 coordinate range", fn, a);
  return device_pointer(fn, "the label volume", vol);
}

}  // namespace

FPLS_EXPORT const char *fpls_last_error(void) try {
  return side_err;
} catch (...) { return "fpls_last_error: C++ exception"; }

FPLS_EXPORT int fpls_abi_version(void) try {
  return FPLS_ABI_VERSION;
} FPLS_CATCH()

FPLS_EXPORT int fpls_pad_box(const void *vol, int32_t seg_bytes, const int64_t extent[3],
                             const int64_t origin[3], const int64_t dims[3], int32_t r,
                             uint64_t *dst, void *stream) try {
  const char *fn = "fpls_pad_box";
  if (!origin || !dims || !dst) return fpls_fail("%s: null pointer argument", fn);
  if (volume_ok(fn, vol, seg_bytes, extent)) return 1;
  if (r < 0 || r >= COORD_LIM) return fpls_fail("%s: r %d", fn, r);
  int64_t pdims[3];
  for (int a = 0; a < 3; ++a) {
    if (dims[a] <= 0 || dims[a] >= COORD_LIM || origin[a] <= -COORD_LIM || origin[a] >= COORD_LIM)
      return fpls_fail("%s: axis %d out of the 2^21 coordinate range", fn, a);
    pdims[a] = dims[a] + 2 * (int64_t)r;
  }
  if (device_pointer(fn, "dst", dst)) return 1;
  if (!aligned(dst, 8)) return fpls_fail("%s: dst is not 8-byte aligned", fn);
  int dev = 0, n_cu = 0;
  if (hip_ok(fn, "hipGetDevice", hipGetDevice(&dev))) return 1;
  if (hip_ok(fn, "hipDeviceGetAttribute",
             hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev))) return 1;
  hipStream_t st = (hipStream_t)stream;
  launch_seg_pad_box(vol, seg_bytes, extent, origin, r, (unsigned long long *)dst, pdims, n_cu, st);
  if (launched(fn)) return 1;
  return hip_ok(fn, "hipStreamSynchronize", hipStreamSynchronize(st));
} FPLS_CATCH()

FPLS_EXPORT int fpls_gather_labels(const void *vol, int32_t seg_bytes, const int64_t extent[3],
                                   const int64_t *zyx, int zyx_mem, int64_t n, uint64_t *out,
                                   int out_mem, void *stream) try {
  const char *fn = "fpls_gather_labels";
  if (n < 0) return fpls_fail("%s: n %lld", fn, (long long)n);
  if (volume_ok(fn, vol, seg_bytes, extent)) return 1;
  if (n == 0) return 0;
  if (!zyx || !out) return fpls_fail("%s: null pointer argument", fn);
  if (zyx_mem == FPLS_MEM_HOST)
    for (int64_t i = 0; i < n; ++i)
      for (int a = 0; a < 3; ++a)
        if (zyx[3 * i + a] < 0 || zyx[3 * i + a] >= extent[a])
          return fpls_fail("%s: point %lld axis %d: %lld outside [0, %lld)", fn, (long long)i, a,
                           (long long)zyx[3 * i + a], (long long)extent[a]);
  hipStream_t st = (hipStream_t)stream;
  DevBlock pts_up, stage_blk;
  const long long *pts = (const long long *)zyx;
  if (zyx_mem == FPLS_MEM_HOST) {
    const size_t nb = (size_t)n * 3 * sizeof(long long);
    if (hip_ok(fn, "hipMalloc", hipMalloc(&pts_up.p, nb))) return 1;
    if (hip_ok(fn, "hipMemcpyAsync", hipMemcpyAsync(pts_up.p, zyx, nb, hipMemcpyHostToDevice, st))) return 1;
    pts = (const long long *)pts_up.p;
  }
  // the kernel writes a staging buffer: a failed call leaves `out` as it was
  const size_t out_bytes = (size_t)n * sizeof(unsigned long long);
  if (hip_ok(fn, "hipMalloc", hipMalloc(&stage_blk.p, out_bytes + 16))) return 1;
  unsigned long long *stage = (unsigned long long *)stage_blk.p;
  unsigned int *overflow = (unsigned int *)(stage + n);
  if (hip_ok(fn, "hipMemsetAsync", hipMemsetAsync(overflow, 0, 4, st))) return 1;
  launch_gather_labels(vol, seg_bytes, extent, pts, n, stage, overflow, st);
  if (launched(fn)) return 1;
  unsigned int ovf = 0;
  if (hip_ok(fn, "hipMemcpyAsync", hipMemcpyAsync(&ovf, overflow, 4, hipMemcpyDeviceToHost, st))) return 1;
  if (hip_ok(fn, "hipStreamSynchronize", hipStreamSynchronize(st))) return 1;
  if (ovf) return fpls_fail("%s: a point lies outside the volume", fn);
  if (hip_ok(fn, "hipMemcpyAsync",
             hipMemcpyAsync(out, stage, out_bytes,
                            out_mem == FPLS_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                            st))) return 1;
  return hip_ok(fn, "hipStreamSynchronize", hipStreamSynchronize(st));
} FPLS_CATCH()
