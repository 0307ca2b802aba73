// libfplval.so (include/fplval.h): the loss and metric sums of a batch of predictions against its
// labels - the reduction of held-out validation.  The formulas are those of the training
// step's loss_grad (csrc/train.hip), with two differences: the per-element loss is evaluated in
// double from the float32 prediction (so it does not depend on logf's rounding), and no
// gradient is written.
//
// Two launches.  loss_partials: a grid fixed by n alone; every thread walks the 16-byte-aligned
// middle of `pred` in grid strides, one float4 of predictions and one 4-byte word of labels per
// step (the labels byte by byte where their word is not aligned), block 0 also takes the
// elements before the first 16-byte boundary and the n % 4 remainder one by one; the block's
// seven sums are reduced by shuffles, then across its waves in wave order, and written to
// scratch[block][7].  loss_finish: one block adds the partials in block order and writes (or
// adds to) sums[0..7].  Every order is fixed, so equal inputs give equal bits.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fplval.h"
#include "../side/side_abi.h"

#define FPLV_EXPORT SIDE_EXPORT
#define FPLV_CATCH() SIDE_CATCH()
#define fplv_fail side_fail

static_assert(FPLV_SCRATCH_BYTES == FPLV_MAX_BLOCKS * 7 * 8, "scratch = one row of 7 doubles per block");
static_assert(FPLV_ELEMS_PER_THREAD == 4, "the main loop loads one float4 and one label word");
static_assert(FPLV_BLOCK % 64 == 0 && FPLV_BLOCK <= 1024, "whole waves");

namespace {

constexpr int N_PART = 7;                      // sums[7] is n: no partial
constexpr int N_WAVES = FPLV_BLOCK / 64;

// v[0..6] += the element (p, y)
template <int KIND>
__device__ __forceinline__ void add_element(float pf, int yl, double v[N_PART]) {
// every operation rounded on its own, as the numpy specification (valid.loss_sums_numpy) does
#pragma clang fp contract(off)
  const double eps = 1e-7;
  const double p = (double)pf;
  double l;
  if (KIND == FPLV_LOSS_MASKED_FOCAL) {
    const double m = yl < 2 ? 1.0 : 0.0;
    const double pt = yl == 1 ? p : 1.0 - p;
    l = -(m * ((1.0 - pt) * (1.0 - pt)) * log(pt + eps));
  } else {
    const double mask = KIND == FPLV_LOSS_BCE ? 1.0 : (yl != 2 ? 1.0 : 0.0);
    const double t = (double)yl * mask, pm = p * mask;
    const double pc = fmin(fmax(pm, eps), 1.0 - eps);
    const double z = log(pc / (1.0 - pc));
    const double soft = log1p(exp(-fabs(z)));
    if (KIND == FPLV_LOSS_MASKED_WEIGHTED_BCE)
      l = (1.0 - t) * z + (1.0 + 99.0 * t) * (soft + fmax(-z, 0.0));
    else
      l = fmax(z, 0.0) - z * t + soft;
  }
  const float y = (float)yl;
  const float mk = yl != 2 ? 1.f : 0.f;
  v[0] += l;
  v[1] += rintf(pf) == y ? 1.0 : 0.0;
  v[2] += rintf(pf * mk) == y * mk ? 1.0 : 0.0;
  v[3] += yl == 0 ? p : 0.0;
  v[4] += yl == 0 ? 1.0 : 0.0;
  v[5] += yl == 1 ? (double)(1.f - pf) : 0.0;
  v[6] += yl == 1 ? 1.0 : 0.0;
}

// `head` elements precede the first float4, `nvec` float4s follow them, n - head - 4 nvec < 4
// elements remain.  LAB4: labels + head is 4-byte aligned.
template <int KIND, bool LAB4>
__global__ __launch_bounds__(FPLV_BLOCK) void loss_partials(
    const float *__restrict__ pred, const uint8_t *__restrict__ labels, int64_t n, int head,
    int64_t nvec, double *__restrict__ partials) {
  __shared__ double sh[N_PART][N_WAVES];
  const unsigned t = threadIdx.x;
  double v[N_PART] = {0, 0, 0, 0, 0, 0, 0};
  const float4 *__restrict__ p4 = reinterpret_cast<const float4 *>(pred + head);
  const uint8_t *__restrict__ lab = labels + head;
  const int64_t stride = (int64_t)gridDim.x * FPLV_BLOCK;
  for (int64_t j = (int64_t)blockIdx.x * FPLV_BLOCK + t; j < nvec; j += stride) {
    const float4 p = p4[j];
    uint32_t y;
    if (LAB4) {
      y = reinterpret_cast<const uint32_t *>(lab)[j];
    } else {
      const uint8_t *q = lab + 4 * j;
      y = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
    }
    add_element<KIND>(p.x, (int)(y & 255u), v);
    add_element<KIND>(p.y, (int)(y >> 8 & 255u), v);
    add_element<KIND>(p.z, (int)(y >> 16 & 255u), v);
    add_element<KIND>(p.w, (int)(y >> 24), v);
  }
  if (blockIdx.x == 0) {
    const int64_t done = head + 4 * nvec;
    if ((int)t < head) add_element<KIND>(pred[t], labels[t], v);
    if ((int64_t)t < n - done) add_element<KIND>(pred[done + t], labels[done + t], v);
  }
#pragma unroll
  for (int k = 0; k < N_PART; ++k) {
    double s = v[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((t & 63u) == 0) sh[k][t >> 6] = s;
  }
  __syncthreads();
  if (t < (unsigned)N_PART) {
    double s = sh[t][0];
#pragma unroll
    for (int w = 1; w < N_WAVES; ++w) s += sh[t][w];
    partials[(int64_t)blockIdx.x * N_PART + t] = s;
  }
}

__global__ __launch_bounds__(64) void loss_finish(const double *__restrict__ partials, int n_blocks,
                                                  int64_t n, int accumulate,
                                                  double *__restrict__ sums) {
  const unsigned t = threadIdx.x;
  if (t >= (unsigned)FPLV_N_SUMS) return;
  double s;
  if (t < (unsigned)N_PART) {
    s = partials[t];
#pragma unroll 8
    for (int b = 1; b < n_blocks; ++b) s += partials[b * N_PART + t];
  } else {
    s = (double)n;
  }
  sums[t] = accumulate ? sums[t] + s : s;
}

template <int KIND>
void launch(bool lab4, int blocks, hipStream_t st, const float *pred, const uint8_t *labels,
            int64_t n, int head, int64_t nvec, double *partials) {
  if (lab4)
    loss_partials<KIND, true><<<blocks, FPLV_BLOCK, 0, st>>>(pred, labels, n, head, nvec, partials);
  else
    loss_partials<KIND, false><<<blocks, FPLV_BLOCK, 0, st>>>(pred, labels, n, head, nvec, partials);
}

// 0 when `p` is device memory
int device_pointer(const char *fn, const char *what, const void *p) {
  hipPointerAttribute_t attr;
  const hipError_t e = hipPointerGetAttributes(&attr, p);
  if (e != hipSuccess) (void)hipGetLastError();          // plain host memory on older runtimes
  if (e != hipSuccess || attr.type != hipMemoryTypeDevice)
    return fplv_fail("%s: %s must be device memory", fn, what);
  return 0;
}

}  // namespace

FPLV_EXPORT const char *fplv_last_error(void) try {
  return side_err;
} catch (...) { return "fplv_last_error: C++ exception"; }

FPLV_EXPORT int fplv_abi_version(void) try {
  return FPLV_ABI_VERSION;
} FPLV_CATCH()

FPLV_EXPORT int fplv_loss_sums(const float *pred, const uint8_t *labels, int64_t n,
                               int32_t loss_kind, int32_t accumulate, double *sums, void *scratch,
                               int64_t scratch_bytes, void *stream) try {
  const char *fn = "fplv_loss_sums";
  if (in_int32_range(fn, "n", n, 1)) return 1;
  if (loss_kind < FPLV_LOSS_BCE || loss_kind > FPLV_LOSS_MASKED_FOCAL)
    return fplv_fail("%s: unknown loss_kind %d (0 BCE, 1 masked BCE, 2 masked weighted BCE, 3 masked "
                     "focal)", fn, loss_kind);
  if (!pred || !labels || !sums || !scratch) return fplv_fail("%s: null pointer argument", fn);
  if (scratch_bytes < FPLV_SCRATCH_BYTES)
    return fplv_fail("%s: scratch of %lld bytes, FPLV_SCRATCH_BYTES is %d", fn,
                     (long long)scratch_bytes, FPLV_SCRATCH_BYTES);
  if (!aligned(pred, 4)) return fplv_fail("%s: pred is not 4-byte aligned", fn);
  if (!aligned(sums, 8) || !aligned(scratch, 8))
    return fplv_fail("%s: sums and scratch must be 8-byte aligned", fn);
  if (device_pointer(fn, "pred", pred) || device_pointer(fn, "labels", labels) ||
      device_pointer(fn, "sums", sums) || device_pointer(fn, "scratch", scratch))
    return 1;
  // floats up to pred's first 16-byte boundary
  const int head = (int)std::min<int64_t>(n, (int64_t)((16 - ((uintptr_t)pred & 15)) & 15) / 4);
  const int64_t nvec = (n - head) / FPLV_ELEMS_PER_THREAD;
  const int blocks = (int)std::min<int64_t>(
      std::max<int64_t>((nvec + FPLV_BLOCK - 1) / FPLV_BLOCK, 1), FPLV_MAX_BLOCKS);
  const bool lab4 = aligned(labels + head, 4);
  hipStream_t st = (hipStream_t)stream;
  double *partials = (double *)scratch;
  switch (loss_kind) {
    case FPLV_LOSS_BCE:
      launch<FPLV_LOSS_BCE>(lab4, blocks, st, pred, labels, n, head, nvec, partials); break;
    case FPLV_LOSS_MASKED_BCE:
      launch<FPLV_LOSS_MASKED_BCE>(lab4, blocks, st, pred, labels, n, head, nvec, partials); break;
    case FPLV_LOSS_MASKED_WEIGHTED_BCE:
      launch<FPLV_LOSS_MASKED_WEIGHTED_BCE>(lab4, blocks, st, pred, labels, n, head, nvec, partials);
      break;
    default:
      launch<FPLV_LOSS_MASKED_FOCAL>(lab4, blocks, st, pred, labels, n, head, nvec, partials); break;
  }
  if (launched(fn)) return 1;
  loss_finish<<<1, 64, 0, st>>>(partials, blocks, n, accumulate, sums);
  return launched(fn);
} FPLV_CATCH()
