// libfplclahe.so (include/fplclahe.h): per-slice CLAHE of a resident (Z, Y, X) volume, bit for bit
// what flypylib_amd/clahe.py's clahe_numpy computes.  The step letters are the specification's.
//
// range    slice_range: the raw min and max of every slice.  min and max are exact in any order,
//          so each wave reduces by shuffles and folds its pair into the slice's two words with one
//          integer atomicMin / atomicMax on order-preserving keys.  volume_range: one block takes
//          the min and max over the slices: mn, mx.
//          The slice's lo and hi (step b) need no second pass over the data: step (a),
//          s(v) = fl(fl(v - mn) / fl(mx - mn)), is two correctly rounded operations with a
//          positive divisor, each monotone non-decreasing in its left operand, so s is monotone
//          non-decreasing in v and min(s) = s(min v), max(s) = s(max v).
// maps     tile_maps: one workgroup per tile (z, i, j).  The tile's rows in unpadded coordinates
//          are [i ky, (i + 1) ky) (the pad before, ky / 2, cancels against the tile grid's
//          origin), read through reflect_index where they pass the slice's end.  Histogram in LDS
//          by integer atomics (order-free), then wave 0 runs the clip of step (h) collectively,
//          four consecutive bins per lane, in the specification's order: the loop over `index`
//          is sequential, count(under) is ballot + popcount, the strided selection is computed
//          per lane.  An inclusive scan and step (i) follow.
// apply    tile_apply: one thread per pixel of the unpadded slice: g and bin again, four uint16
//          map entries, step (j) in float64 spelled as __dmul_rn / __dadd_rn under contract(off);
//          the uint16 result to scratch; min / max of it per wave, one atomic each.
// finish   rescale: step (k) and zero_mean.
// A uint8 volume has 256 possible values per slice, so tile_maps and tile_apply build the
// value -> bin table of their slice in LDS (one entry per thread) instead of dividing per pixel.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fplclahe.h"
#include "../side/side_abi.h"

#define FPLC_EXPORT SIDE_EXPORT
#define FPLC_CATCH() SIDE_CATCH()
#define fplc_fail side_fail

static_assert(FPLC_BLOCK == 256 && FPLC_MAX_NBINS == 4 * 64, "four bins per lane of one wave");

namespace {

constexpr int WORDS = 4;           // per slice: key of raw min, key of raw max, rmin, rmax
constexpr double TOP = (double)(FPLC_NR_OF_GRAY - 1);

// float <-> uint32 whose unsigned order is the float order
__device__ __forceinline__ uint32_t key_of(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float float_of(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// np.pad(mode='reflect') as a closed form (clahe.reflect_index), for i >= 0
__device__ __forceinline__ uint32_t reflect_index(uint32_t i, uint32_t s) {
  if (i < s) return i;
  if (s == 1) return 0;
  const uint32_t period = 2 * (s - 1);
  const uint32_t m = i % period;
  return m < s ? m : period - m;
}

struct SliceRange {
  float mn, den;       // the volume's mn and fl(mx - mn)
  double lo, hml;      // the slice's lo and hi - lo, float64
  bool live;           // false: the slice comes out 0
};

__device__ __forceinline__ SliceRange slice_range_of(const uint32_t *__restrict__ status,
                                                     const uint32_t *__restrict__ words, int64_t z) {
#pragma clang fp contract(off)
  SliceRange r;
  const float mn = __uint_as_float(status[0]), mx = __uint_as_float(status[1]);
  r.mn = mn;
  r.den = __fsub_rn(mx, mn);
  const float lo = __fdiv_rn(__fsub_rn(float_of(words[z * WORDS + 0]), mn), r.den);
  const float hi = __fdiv_rn(__fsub_rn(float_of(words[z * WORDS + 1]), mn), r.den);
  r.lo = (double)lo;
  r.hml = __dsub_rn((double)hi, (double)lo);
  r.live = status[2] == 0 && mx != mn && hi != lo;
  return r;
}

// steps (a), (c), (f) of one raw value
__device__ __forceinline__ int bin_of(float v, const SliceRange &r, int bin_size) {
#pragma clang fp contract(off)
  const float s = __fdiv_rn(__fsub_rn(v, r.mn), r.den);
  const double g = rint(__dmul_rn(__ddiv_rn(__dsub_rn((double)s, r.lo), r.hml), TOP));
  const int gi = min(max((int)g, 0), FPLC_NR_OF_GRAY - 1);
  return gi / bin_size;
}

template <bool U8>
__device__ __forceinline__ float raw_value(const void *__restrict__ in, int64_t idx) {
  return U8 ? (float)static_cast<const uint8_t *>(in)[idx] : static_cast<const float *>(in)[idx];
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// which: 1 the range words and the flag, 2 the words of the interpolated slice
__global__ __launch_bounds__(FPLC_BLOCK) void init_words(uint32_t *__restrict__ status,
                                                         uint32_t *__restrict__ words, int64_t Z,
                                                         int which) {
  const int64_t z = (int64_t)blockIdx.x * FPLC_BLOCK + threadIdx.x;
  if (z == 0 && which == 1) status[2] = status[3] = 0u;
  if (z >= Z) return;
  const int o = which == 1 ? 0 : 2;
  words[z * WORDS + o] = 0xffffffffu;
  words[z * WORDS + o + 1] = 0u;
}

template <bool U8>
__global__ __launch_bounds__(FPLC_BLOCK) void slice_range(const void *__restrict__ in, int64_t YX,
                                                          int chunks, uint32_t *__restrict__ status,
                                                          uint32_t *__restrict__ words) {
  const int64_t z = blockIdx.x / chunks;
  const int c = blockIdx.x % chunks;
  float lo = INFINITY, hi = -INFINITY;
  int bad = 0;
  for (int64_t p = (int64_t)c * FPLC_BLOCK + threadIdx.x; p < YX; p += (int64_t)chunks * FPLC_BLOCK) {
    const float v = raw_value<U8>(in, z * YX + p) + 0.0f;      // -0 -> +0: one key per value
    if (!U8 && !isfinite(v)) bad = 1;
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, off, 64));
    hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    bad |= __shfl_xor(bad, off, 64);
  }
  if ((threadIdx.x & 63u) == 0) {
    atomicMin(&words[z * WORDS + 0], key_of(lo));
    atomicMax(&words[z * WORDS + 1], key_of(hi));
    if (bad) atomicOr(&status[2], 1u);
  }
}

__global__ __launch_bounds__(FPLC_BLOCK) void volume_range(uint32_t *__restrict__ status,
                                                           const uint32_t *__restrict__ words,
                                                           int64_t Z) {
  __shared__ uint32_t lo_s[FPLC_BLOCK], hi_s[FPLC_BLOCK];
  const unsigned t = threadIdx.x;
  uint32_t lo = 0xffffffffu, hi = 0u;
  for (int64_t z = t; z < Z; z += FPLC_BLOCK) {
    lo = min(lo, words[z * WORDS + 0]);
    hi = max(hi, words[z * WORDS + 1]);
  }
  lo_s[t] = lo;
  hi_s[t] = hi;
  __syncthreads();
  for (unsigned off = FPLC_BLOCK / 2; off > 0; off >>= 1) {
    if (t < off) {
      lo_s[t] = min(lo_s[t], lo_s[t + off]);
      hi_s[t] = max(hi_s[t], hi_s[t + off]);
    }
    __syncthreads();
  }
  if (t == 0) {
    status[0] = __float_as_uint(float_of(lo_s[0]));
    status[1] = __float_as_uint(float_of(hi_s[0]));
  }
}

// step (h) on the histogram of n bins held four consecutive bins per lane by one whole wave:
// lane l holds bins 4 l .. 4 l + 3, `live[q]` where the bin exists
__device__ __forceinline__ void clip_wave(int h[4], const bool live[4], int lane, int n, int clim) {
  int d = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (live[q] && h[q] > clim) {
      d += h[q] - clim;
      h[q] = clim;
    }
  int n_excess = wave_sum(d);
  const int bin_incr = n_excess / n;
  const int upper = clim - bin_incr;
  d = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (live[q] && h[q] < upper) {
      h[q] += bin_incr;
      ++d;
    }
  n_excess -= wave_sum(d) * bin_incr;
  d = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (live[q] && h[q] >= upper && h[q] < clim) {
      d += h[q] - clim;
      h[q] = clim;
    }
  n_excess += wave_sum(d);
  while (n_excess > 0) {
    const int prev = n_excess;
    bool none_under = false;
    for (int index = 0; index < n; ++index) {
      bool under[4];
      int count = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        under[q] = live[q] && h[q] < clim;
        count += __popcll(__ballot(under[q]));
      }
      if (count == 0) {              // nothing can change for any further index
        none_under = true;
        break;
      }
      const int step = max(1, count / n_excess);
      int taken = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int b = 4 * lane + q;
        const bool sel = under[q] && b >= index && (b - index) % step == 0;
        if (sel) ++h[q];
        taken += __popcll(__ballot(sel));
      }
      n_excess -= taken;
      if (n_excess <= 0) break;
    }
    if (none_under || prev == n_excess) break;
  }
}

template <bool U8>
__global__ __launch_bounds__(FPLC_BLOCK) void tile_maps(
    const void *__restrict__ in, const uint32_t *__restrict__ status,
    const uint32_t *__restrict__ words, uint16_t *__restrict__ maps, uint32_t Y, uint32_t X,
    uint32_t ky, uint32_t kx, uint32_t nty, uint32_t ntx, int nbins, int clim) {
#pragma clang fp contract(off)
  __shared__ int hist[FPLC_MAX_NBINS];
  __shared__ uint16_t lut[U8 ? 256 : 1];
  const unsigned t = threadIdx.x;
  const uint32_t j = blockIdx.x % ntx, i = (blockIdx.x / ntx) % nty;
  const int64_t z = blockIdx.x / (ntx * nty);
  const SliceRange r = slice_range_of(status, words, z);
  if (!r.live) return;                                   // the whole block: z is the block's
  const int bin_size = 1 + FPLC_NR_OF_GRAY / nbins;
  hist[t] = 0;
  if (U8) lut[t] = (uint16_t)bin_of((float)t, r, bin_size);
  __syncthreads();
  const int64_t base = z * ((int64_t)Y * X);
  const uint32_t npix = ky * kx;
  for (uint32_t p = t; p < npix; p += FPLC_BLOCK) {
    const uint32_t dy = p / kx, dx = p - dy * kx;
    const uint32_t yy = reflect_index(i * ky + dy, Y), xx = reflect_index(j * kx + dx, X);
    const int64_t idx = base + (int64_t)yy * X + xx;
    const int b = U8 ? (int)lut[static_cast<const uint8_t *>(in)[idx]]
                     : bin_of(static_cast<const float *>(in)[idx], r, bin_size);
    atomicAdd(&hist[b], 1);
  }
  __syncthreads();
  if (t >= 64) return;
  int h[4];
  bool live[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    live[q] = 4 * (int)t + q < nbins;
    h[q] = live[q] ? hist[4 * t + q] : 0;
  }
  clip_wave(h, live, (int)t, nbins, clim);
  // step (i): inclusive scan (a lane's four, then the lanes), scaled and truncated
  long long c[4];
  c[0] = h[0];
#pragma unroll
  for (int q = 1; q < 4; ++q) c[q] = c[q - 1] + h[q];
  long long run = c[3];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const long long v = __shfl_up(run, off, 64);
    if ((int)t >= off) run += v;
  }
  const long long before = run - c[3];
  const double scale = __ddiv_rn(TOP, (double)npix);
  uint16_t *__restrict__ dst = maps + (int64_t)blockIdx.x * nbins;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (live[q]) {
      const double m = fmin(__dmul_rn((double)(before + c[q]), scale), TOP);
      dst[4 * t + q] = (uint16_t)(int)m;
    }
}

template <bool U8>
__global__ __launch_bounds__(FPLC_BLOCK) void tile_apply(
    const void *__restrict__ in, const uint32_t *__restrict__ status, uint32_t *__restrict__ words,
    const uint16_t *__restrict__ maps, uint16_t *__restrict__ rbuf, uint32_t Y, uint32_t X,
    uint32_t ky, uint32_t kx, uint32_t nty, uint32_t ntx, int nbins, uint32_t chunks) {
#pragma clang fp contract(off)
  __shared__ uint16_t lut[U8 ? 256 : 1];
  const unsigned t = threadIdx.x;
  const int64_t z = blockIdx.x / chunks;
  const uint32_t YX = Y * X;
  const uint32_t p = (blockIdx.x % chunks) * FPLC_BLOCK + t;
  const bool valid = p < YX;
  const SliceRange r = slice_range_of(status, words, z);
  const int bin_size = 1 + FPLC_NR_OF_GRAY / nbins;
  if (U8 && r.live) {                                    // uniform over the block
    lut[t] = (uint16_t)bin_of((float)t, r, bin_size);
    __syncthreads();
  }
  uint32_t out = 0;
  if (valid && r.live) {
    const uint32_t yy = p / X, xx = p - yy * X;
    const int64_t idx = z * (int64_t)YX + p;
    const int b = U8 ? (int)lut[static_cast<const uint8_t *>(in)[idx]]
                     : bin_of(static_cast<const float *>(in)[idx], r, bin_size);
    const uint32_t y = yy + ky / 2, x = xx + kx / 2;     // padded coordinates
    const uint32_t by = y / ky, bx = x / kx;
    const double cy = __ddiv_rn((double)(y - by * ky), (double)ky);
    const double cx = __ddiv_rn((double)(x - bx * kx), (double)kx);
    const uint16_t *__restrict__ mz = maps + z * ((int64_t)nty * ntx) * nbins;
    double acc = 0.0;
#pragma unroll
    for (int ey = 0; ey < 2; ++ey) {
      const int ty = min(max((int)by - 1 + ey, 0), (int)nty - 1);
      const double wy = ey ? cy : __dsub_rn(1.0, cy);
#pragma unroll
      for (int ex = 0; ex < 2; ++ex) {
        const int tx = min(max((int)bx - 1 + ex, 0), (int)ntx - 1);
        const double wx = ex ? cx : __dsub_rn(1.0, cx);
        const double m = (double)mz[((int64_t)ty * ntx + tx) * nbins + b];
        acc = __dadd_rn(acc, __dmul_rn(m, __dmul_rn(wy, wx)));
      }
    }
    out = (uint32_t)(int)acc;
  }
  if (valid) rbuf[z * (int64_t)YX + p] = (uint16_t)out;
  uint32_t lo = valid ? out : 0xffffffffu, hi = valid ? out : 0u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = min(lo, (uint32_t)__shfl_xor((int)lo, off, 64));
    hi = max(hi, (uint32_t)__shfl_xor((int)hi, off, 64));
  }
  if ((t & 63u) == 0 && lo != 0xffffffffu) {
    atomicMin(&words[z * WORDS + 2], lo);
    atomicMax(&words[z * WORDS + 3], hi);
  }
}

__global__ __launch_bounds__(FPLC_BLOCK) void rescale(const uint16_t *__restrict__ rbuf,
                                                      const uint32_t *__restrict__ words,
                                                      float *__restrict__ out, int64_t n, uint32_t YX,
                                                      int zero_mean) {
#pragma clang fp contract(off)
  const int64_t idx = (int64_t)blockIdx.x * FPLC_BLOCK + threadIdx.x;
  if (idx >= n) return;
  const int64_t z = idx / YX;
  const uint32_t rmin = words[z * WORDS + 2], rmax = words[z * WORDS + 3];
  float v = 0.0f;
  if (rmax != rmin)
    v = (float)__ddiv_rn(__dsub_rn((double)rbuf[idx], (double)rmin), (double)(rmax - rmin));
  out[idx] = zero_mean ? __fsub_rn(v, 0.5f) : v;
}

struct Layout {
  int64_t n, YX, nty, ntx, tiles, off_words, off_maps, off_r, bytes;
};

inline int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// the sizes a call takes, and where the parts of its scratch lie: 0, or a message
int layout_of(const char *fn, int64_t Z, int64_t Y, int64_t X, int64_t ky, int64_t kx, int32_t nbins,
              Layout *L) {
  if (Z < 1 || Y < 1 || X < 1)
    return fplc_fail("%s: a volume of (%lld,%lld,%lld)", fn, (long long)Z, (long long)Y, (long long)X);
  const int64_t dims[3] = {Z, Y, X};
  if (volume_voxels(fn, dims, "the kernels", "run clahe on the host (device=None)", &L->n)) return 1;
  if (in_int32_range(fn, "ky", ky, 1) || in_int32_range(fn, "kx", kx, 1)) return 1;
  if (ky * kx > SIDE_INT32_MAX)
    return fplc_fail("%s: a tile of %lld x %lld holds 2^31 or more pixels", fn, (long long)ky,
                     (long long)kx);
  if (nbins < 2 || nbins > FPLC_MAX_NBINS)
    return fplc_fail("%s: nbins %d is outside 2..%d", fn, nbins, FPLC_MAX_NBINS);
  L->YX = Y * X;
  L->nty = (Y + ky - 1) / ky;
  L->ntx = (X + kx - 1) / kx;
  L->tiles = Z * L->nty * L->ntx;                 // <= Z Y X
  L->off_words = FPLC_STATUS_BYTES;
  L->off_maps = up16(L->off_words + Z * WORDS * 4);
  L->off_r = up16(L->off_maps + L->tiles * nbins * 2);
  L->bytes = up16(L->off_r + L->n * 2);
  return 0;
}

// 0 when `p` is device memory
int device_pointer(const char *fn, const char *what, const void *p) {
  hipPointerAttribute_t attr;
  const hipError_t e = hipPointerGetAttributes(&attr, p);
  if (e != hipSuccess) (void)hipGetLastError();          // plain host memory on older runtimes
  if (e != hipSuccess || attr.type != hipMemoryTypeDevice)
    return fplc_fail("%s: %s must be device memory", fn, what);
  return 0;
}

template <bool U8>
int run(const char *fn, const Layout &L, const void *in, int64_t Z, int64_t Y, int64_t X, int64_t ky,
        int64_t kx, int clim, int nbins, int zero_mean, float *out, char *scratch, int stages,
        hipStream_t st) {
  uint32_t *status = (uint32_t *)scratch;
  uint32_t *words = (uint32_t *)(scratch + L.off_words);
  uint16_t *maps = (uint16_t *)(scratch + L.off_maps);
  uint16_t *rbuf = (uint16_t *)(scratch + L.off_r);
  const int zblocks = (int)((Z + FPLC_BLOCK - 1) / FPLC_BLOCK);
  if (stages & FPLC_STAGE_RANGE) {
    init_words<<<zblocks, FPLC_BLOCK, 0, st>>>(status, words, Z, 1);
    if (launched(fn)) return 1;
    // 16 values per thread and pass; at most 64 blocks per slice
    const int chunks = (int)std::min<int64_t>(std::max<int64_t>((L.YX + 4095) / 4096, 1), 64);
    slice_range<U8><<<(unsigned)(Z * chunks), FPLC_BLOCK, 0, st>>>(in, L.YX, chunks, status, words);
    if (launched(fn)) return 1;
    volume_range<<<1, FPLC_BLOCK, 0, st>>>(status, words, Z);
    if (launched(fn)) return 1;
  }
  if (stages & FPLC_STAGE_MAPS) {
    tile_maps<U8><<<(unsigned)L.tiles, FPLC_BLOCK, 0, st>>>(
        in, status, words, maps, (uint32_t)Y, (uint32_t)X, (uint32_t)ky, (uint32_t)kx,
        (uint32_t)L.nty, (uint32_t)L.ntx, nbins, clim);
    if (launched(fn)) return 1;
  }
  if (stages & FPLC_STAGE_APPLY) {
    init_words<<<zblocks, FPLC_BLOCK, 0, st>>>(status, words, Z, 2);
    if (launched(fn)) return 1;
    const int64_t chunks = (L.YX + FPLC_BLOCK - 1) / FPLC_BLOCK;
    tile_apply<U8><<<(unsigned)(Z * chunks), FPLC_BLOCK, 0, st>>>(
        in, status, words, maps, rbuf, (uint32_t)Y, (uint32_t)X, (uint32_t)ky, (uint32_t)kx,
        (uint32_t)L.nty, (uint32_t)L.ntx, nbins, (uint32_t)chunks);
    if (launched(fn)) return 1;
  }
  if (stages & FPLC_STAGE_FINISH) {
    rescale<<<(unsigned)((L.n + FPLC_BLOCK - 1) / FPLC_BLOCK), FPLC_BLOCK, 0, st>>>(
        rbuf, words, out, L.n, (uint32_t)L.YX, zero_mean);
    if (launched(fn)) return 1;
  }
  return 0;
}

}  // namespace

FPLC_EXPORT const char *fplc_last_error(void) try {
  return side_err;
} catch (...) { return "fplc_last_error: C++ exception"; }

FPLC_EXPORT int fplc_abi_version(void) try {
  return FPLC_ABI_VERSION;
} FPLC_CATCH()

FPLC_EXPORT int fplc_scratch_bytes(int64_t Z, int64_t Y, int64_t X, int64_t ky, int64_t kx,
                                   int32_t nbins, int64_t *bytes) try {
  const char *fn = "fplc_scratch_bytes";
  Layout L;
  if (!bytes) return fplc_fail("%s: null pointer argument", fn);
  if (layout_of(fn, Z, Y, X, ky, kx, nbins, &L)) return 1;
  *bytes = L.bytes;
  return 0;
} FPLC_CATCH()

FPLC_EXPORT int fplc_clahe(const void *in, int32_t dtype, int64_t Z, int64_t Y, int64_t X, int64_t ky,
                           int64_t kx, int64_t clim, int32_t nbins, int32_t zero_mean, float *out,
                           void *scratch, int64_t scratch_bytes, int32_t stages, void *stream) try {
  const char *fn = "fplc_clahe";
  Layout L;
  if (layout_of(fn, Z, Y, X, ky, kx, nbins, &L)) return 1;
  if (in_int32_range(fn, "clim", clim, 1)) return 1;
  if (dtype != FPLC_U8 && dtype != FPLC_F32)
    return fplc_fail("%s: unknown dtype %d (0 uint8, 1 float32)", fn, dtype);
  if (stages < 1 || stages > FPLC_STAGE_ALL)
    return fplc_fail("%s: stages %d is no combination of 1 range, 2 maps, 4 apply, 8 finish", fn, stages);
  if (!in || !out || !scratch) return fplc_fail("%s: null pointer argument", fn);
  if (scratch_bytes < L.bytes)
    return fplc_fail("%s: scratch of %lld bytes, fplc_scratch_bytes is %lld", fn,
                     (long long)scratch_bytes, (long long)L.bytes);
  if (dtype == FPLC_F32 && !aligned(in, 4)) return fplc_fail("%s: a float32 in is not 4-byte aligned", fn);
  if (!aligned(out, 4)) return fplc_fail("%s: out is not 4-byte aligned", fn);
  if (!aligned(scratch, 16)) return fplc_fail("%s: scratch is not 16-byte aligned", fn);
  if (device_pointer(fn, "in", in) || device_pointer(fn, "out", out) ||
      device_pointer(fn, "scratch", scratch))
    return 1;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == FPLC_U8)
    return run<true>(fn, L, in, Z, Y, X, ky, kx, (int)clim, nbins, zero_mean, out, (char *)scratch,
                     stages, st);
  return run<false>(fn, L, in, Z, Y, X, ky, kx, (int)clim, nbins, zero_mean, out, (char *)scratch,
                    stages, st);
} FPLC_CATCH()
