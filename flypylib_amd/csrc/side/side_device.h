// The device code the side libraries share: the one-block scan that turns counts into the
// offsets of an ordered table, the float64 squared distance, and the read-back of a total.
// HIP only; included after side_abi.h.  Everything has internal linkage, as in side_abi.h, so
// each library has kernels of its own.
//
// An ordered table is built in three launches: count, scan, fill.  The scan is one block of
// SIDE_SCAN_THREADS threads: each thread sums a run of consecutive cells, the sums (uint64)
// are scanned in LDS, each thread rewrites its run as exclusive offsets.  The offsets are
// taken mod 2^32 - only a total within int32 rows is ever used - but the total stays a uint64,
// so a table beyond int32 rows is seen and refused, not wrapped.  The sums take 8 KiB of LDS
// in a single-block launch, also where every total fits a uint32 (the candidate tables of the
// mining library, whose volumes hold at most 2^31 - 1 voxels).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace {

constexpr int SIDE_SCAN_THREADS = 1024;
typedef unsigned long long u64;

// inclusive scan of one value per thread over a block of SIDE_SCAN_THREADS threads
__device__ __forceinline__ u64 side_block_scan(u64 own, u64 *sums) {
  const unsigned t = threadIdx.x;
  sums[t] = own;
  __syncthreads();
  for (unsigned off = 1; off < (unsigned)SIDE_SCAN_THREADS; off <<= 1) {
    const u64 v = t >= off ? sums[t - off] : 0ull;
    __syncthreads();
    sums[t] += v;
    __syncthreads();
  }
  return sums[t];
}

// cells[0 .. n) -> exclusive offsets in place (truncated to Cell), by one block of
// SIDE_SCAN_THREADS threads; every thread returns the sum of the cells
template <typename Cell>
__device__ __forceinline__ u64 side_scan_runs(Cell *__restrict__ cells, uint32_t n, u64 *sums) {
  const uint32_t t = threadIdx.x;
  const uint32_t per = (n + SIDE_SCAN_THREADS - 1) / SIDE_SCAN_THREADS;
  const uint32_t lo = (uint32_t)std::min<uint64_t>((uint64_t)t * per, n);
  const uint32_t hi = (uint32_t)std::min<uint64_t>((uint64_t)lo + per, n);
  u64 own = 0;
  for (uint32_t j = lo; j < hi; ++j) own += cells[j];
  Cell run = (Cell)(side_block_scan(own, sums) - own);
  for (uint32_t j = lo; j < hi; ++j) {
    const Cell v = cells[j];
    cells[j] = run;
    run += v;
  }
  return sums[SIDE_SCAN_THREADS - 1];
}

// the scan as a launch of one block; the sum goes to whichever of *total and *tail (truncated)
// is given.  Launched as side_scan_kernel<uint32_t>: a template, so that a library which only
// calls the functions above carries no kernel it never launches.
template <typename Cell>
__global__ __launch_bounds__(SIDE_SCAN_THREADS) void side_scan_kernel(
    Cell *__restrict__ cells, uint32_t n, unsigned long long *__restrict__ total,
    Cell *__restrict__ tail) {
  __shared__ u64 sums[SIDE_SCAN_THREADS];
  const u64 sum = side_scan_runs(cells, n, sums);
  if (threadIdx.x == SIDE_SCAN_THREADS - 1) {
    if (tail) *tail = (Cell)sum;
    if (total) *total = sum;
  }
}

// s = (dx * dx + dy * dy) + dz * dz with every operation rounded on its own: the libraries are
// built with -ffp-contract=on, so this switches contraction off and spells the operations as
// __dmul_rn / __dadd_rn.  That is numpy's (delta ** 2).sum(axis=2), bit for bit.
__device__ __forceinline__ double side_dist2(double px, double py, double pz, double gx, double gy,
                                             double gz) {
#pragma clang fp contract(off)
  const double dx = px - gx, dy = py - gy, dz = pz - gz;
  return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

// `bytes` from the device into host memory once the stream's work is done: 0, or a message
inline int side_read_back(const char *fn, hipStream_t stream, void *dst, const void *src,
                          size_t bytes) {
  hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess)
    return side_fail("%s: reading the total failed: %s", fn, hipGetErrorString(e));
  return 0;
}

}  // namespace
