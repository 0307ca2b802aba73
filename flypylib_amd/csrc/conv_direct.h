// Direct fp32 conv / transposed-conv / strided-conv / dilated-conv kernels shared by the per-op inference executor (generic.hip)
// and the training engine (train.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fplhip.h"

static __device__ __forceinline__ float apply_act(float v, int act) {
  if (act == FPL_ACT_RELU) return fmaxf(v, 0.f);
  if (act == FPL_ACT_SIGMOID) return 1.f / (1.f + expf(-v));
  return v;
}

// Direct valid 3-D cross-correlation.  One thread = one output voxel x CT
// consecutive output channels; weight addresses are wave-uniform (scalar loads).
template <int CT>
static __global__ __launch_bounds__(256) void conv3d_direct_f32(
    const float *__restrict__ x, const float *__restrict__ w,
    const float *__restrict__ scale, const float *__restrict__ shift,
    float *__restrict__ y, int64_t n_vox, int D, int H, int W, int cin, int od,
    int oh, int ow, int cout, int k, int act) {
  int64_t vox = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (vox >= n_vox) return;
  const int co0 = blockIdx.y * CT;
  int64_t t = vox;
  const int ox = (int)(t % ow); t /= ow;
  const int oy = (int)(t % oh); t /= oh;
  const int oz = (int)(t % od); t /= od;
  const int64_t b = t;
  float acc[CT];
#pragma unroll
  for (int j = 0; j < CT; ++j) acc[j] = 0.f;
  for (int dz = 0; dz < k; ++dz)
    for (int dy = 0; dy < k; ++dy)
      for (int dx = 0; dx < k; ++dx) {
        const float *xp =
            x + ((((b * D + oz + dz) * H + oy + dy) * (int64_t)W + ox + dx) * cin);
        const float *wp = w + (int64_t)((dz * k + dy) * k + dx) * cin * cout + co0;
        for (int ci = 0; ci < cin; ++ci) {
          const float xv = xp[ci];
#pragma unroll
          for (int j = 0; j < CT; ++j)
            if (CT == 1 || co0 + j < cout)
              acc[j] = fmaf(xv, wp[(int64_t)ci * cout + j], acc[j]);
        }
      }
  float *yp = y + vox * cout + co0;
#pragma unroll
  for (int j = 0; j < CT; ++j)
    if (co0 + j < cout)
      yp[j] = apply_act(fmaf(acc[j], scale[co0 + j], shift[co0 + j]), act);
}

// Direct Conv3DTranspose(cout, 2, strides=2, 'valid'): the readable restatement of
// FPL_OP_DECONV.  One thread = one output element; its parity (a, b, c) picks the tap, the
// input voxel is the output voxel halved.  x (n, D, H, W, cin), w [8][cout][cin],
// y (n, 2D, 2H, 2W, cout).
static __global__ __launch_bounds__(256) void deconv2_direct_f32(
    const float *__restrict__ x, const float *__restrict__ w,
    const float *__restrict__ scale, const float *__restrict__ shift,
    float *__restrict__ y, int64_t n_out, int D, int H, int W, int cin, int cout, int act) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_out) return;
  int64_t t = i;
  const int co = (int)(t % cout); t /= cout;
  const int ox = (int)(t % (2 * W)); t /= 2 * W;
  const int oy = (int)(t % (2 * H)); t /= 2 * H;
  const int oz = (int)(t % (2 * D)); t /= 2 * D;
  const int tap = ((oz & 1) * 2 + (oy & 1)) * 2 + (ox & 1);
  const float *xp = x + ((((t * D + (oz >> 1)) * H + (oy >> 1)) * (int64_t)W + (ox >> 1)) * cin);
  const float *wp = w + ((int64_t)tap * cout + co) * cin;
  float acc = 0.f;
  for (int ci = 0; ci < cin; ++ci) acc = fmaf(xp[ci], wp[ci], acc);
  y[i] = apply_act(fmaf(acc, scale[co], shift[co]), act);
}

// Direct Conv3D(cout, 2, strides=2, 'valid'): the readable restatement of FPL_OP_DOWN.  One
// thread = one output element, eight taps of cin products each in (a, b, c, ci) order.
// x (n, D, H, W, cin), w [8][cin][cout], y (n, D/2, H/2, W/2, cout); an odd axis drops its last
// input plane.
static __global__ __launch_bounds__(256) void down2_direct_f32(
    const float *__restrict__ x, const float *__restrict__ w,
    const float *__restrict__ scale, const float *__restrict__ shift,
    float *__restrict__ y, int64_t n_out, int D, int H, int W, int cin, int cout, int act) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_out) return;
  const int od = D / 2, oh = H / 2, ow = W / 2;
  int64_t t = i;
  const int co = (int)(t % cout); t /= cout;
  const int ox = (int)(t % ow); t /= ow;
  const int oy = (int)(t % oh); t /= oh;
  const int oz = (int)(t % od); t /= od;
  float acc = 0.f;
  for (int tap = 0; tap < 8; ++tap) {
    const float *xp = x + ((((t * D + 2 * oz + (tap >> 2)) * H + 2 * oy + ((tap >> 1) & 1)) * (int64_t)W +
                            2 * ox + (tap & 1)) * cin);
    const float *wp = w + (int64_t)tap * cin * cout + co;
    for (int ci = 0; ci < cin; ++ci) acc = fmaf(xp[ci], wp[(int64_t)ci * cout], acc);
  }
  y[i] = apply_act(fmaf(acc, scale[co], shift[co]), act);
}

// Direct Conv3D(cout, 3, dilation_rate=2, 'valid'): the readable restatement of FPL_OP_DILATED.
// One thread = one output element, 27 taps two voxels apart of cin products each in
// (a, b, c, ci) order.  x (n, D, H, W, cin), w [27][cin][cout], y (n, D-4, H-4, W-4, cout).
static __global__ __launch_bounds__(256) void atrous3_direct_f32(
    const float *__restrict__ x, const float *__restrict__ w,
    const float *__restrict__ scale, const float *__restrict__ shift,
    float *__restrict__ y, int64_t n_out, int D, int H, int W, int cin, int cout, int act) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_out) return;
  const int od = D - 4, oh = H - 4, ow = W - 4;
  int64_t t = i;
  const int co = (int)(t % cout); t /= cout;
  const int ox = (int)(t % ow); t /= ow;
  const int oy = (int)(t % oh); t /= oh;
  const int oz = (int)(t % od); t /= od;
  float acc = 0.f;
  for (int tap = 0; tap < 27; ++tap) {
    const float *xp = x + ((((t * D + oz + 2 * (tap / 9)) * H + oy + 2 * ((tap / 3) % 3)) * (int64_t)W +
                            ox + 2 * (tap % 3)) * cin);
    const float *wp = w + (int64_t)tap * cin * cout + co;
    for (int ci = 0; ci < cin; ++ci) acc = fmaf(xp[ci], wp[(int64_t)ci * cout], acc);
  }
  y[i] = apply_act(fmaf(acc, scale[co], shift[co]), act);
}
