// The C shell the side libraries share (csrc/build.py's SIDE_LIBRARIES): the thread-local
// error text behind <prefix>_last_error(), the guard of every entry point and the argument
// checks more than one library makes.  Everything has internal linkage, so each library that
// includes this header has an error buffer of its own.  Only launched() needs HIP: the rest
// compiles with a plain host compiler, which is how tests/test_sidelib.py drives it.  What the
// libraries' kernels share is in side_device.h.
//
// A library keeps its own spelling as one-line aliases of SIDE_EXPORT, SIDE_CATCH and
// side_fail, and defines its own <prefix>_last_error (returning side_err) and
// <prefix>_abi_version.
#pragma once

#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <exception>

#define SIDE_EXPORT extern "C" __attribute__((visibility("default")))
#define SIDE_MAX_ERR 512

// the guard of every entry point, written as a function-try-block:
//   int entry(...) try { ... } SIDE_CATCH()
#define SIDE_CATCH()                                                           \
  catch (...) { return side_fail_exception(__func__); }

namespace {

thread_local char side_err[SIDE_MAX_ERR] = {0};

inline int side_fail(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(side_err, sizeof(side_err), fmt, ap);
  va_end(ap);
  return 1;
}

inline int side_fail_exception(const char *fn) {
  try {
    throw;
  } catch (const std::exception &e) {
    return side_fail("%s: C++ exception: %s", fn, e.what());
  } catch (...) {
    return side_fail("%s: unknown C++ exception", fn);
  }
}

inline bool aligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// what an int32 row, count or index can hold
constexpr int64_t SIDE_INT32_MAX = 2147483647;

// 0, or a message when `what` (a count: lo 1, a capacity: lo 0) lies outside [lo, 2^31 - 1]
inline int in_int32_range(const char *fn, const char *what, int64_t v, int lo) {
  if (v < lo || v > SIDE_INT32_MAX)
    return side_fail("%s: %s %lld must lie in [%d, 2^31 - 1]", fn, what, (long long)v, lo);
  return 0;
}

// *n = the voxels of a volume of positive dims, or a message when they exceed the 2^31 - 1 that
// `what` ("the brick tables", ...) can index; `advice` says what to do instead
inline int volume_voxels(const char *fn, const int64_t dims[3], const char *what, const char *advice,
                         int64_t *n) {
  const int64_t lim = SIDE_INT32_MAX;
  if (dims[0] > lim || dims[1] > lim || dims[2] > lim || dims[1] * dims[2] > lim ||
      dims[0] * (dims[1] * dims[2]) > lim)
    return side_fail("%s: a volume of (%lld,%lld,%lld) voxels exceeds the 2^31 - 1 voxels %s can "
                     "index; %s", fn, (long long)dims[0], (long long)dims[1], (long long)dims[2],
                     what, advice);
  *n = dims[0] * dims[1] * dims[2];
  return 0;
}

#ifdef __HIPCC__
// after a kernel launch: 0, or the launch error as a message
inline int launched(const char *fn) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return side_fail("%s: launch failed: %s", fn, hipGetErrorString(e));
  return 0;
}
#endif

}  // namespace
