// Conv3DTranspose(filters, 2, strides=2) on the graph executor (gx_exec.h): the host side of its
// weights.  No HIP in here - tests/test_deconv_gx_host.py compiles this header stand-alone.
//
// The layer's kernel lies in the arena as [8][cout][cin] (tap = 4 a + 2 b + c of output voxel
// (2z + a, 2y + b, 2x + c); out-channels BEFORE in-channels, include/fplhip.h), a convolution's as
// [tap][cin][cout].  Each tap is one voxel GEMM, so each tap becomes the padded [cin_p][cout_p]
// matrix of a 1x1x1 convolution (what gx_padded_op makes of one), which pack_conv1 takes.
#pragma once
#include <cstddef>

// out[r][co] = K[tap][co][r] for r < cin, co < cout; zero in the padding rows and columns
static inline void fpl_deconv_tap_matrix(const float *K, int cin, int cout, int tap, int cin_p, int cout_p,
                                         float *out) {
  for (int r = 0; r < cin_p; ++r)
    for (int co = 0; co < cout_p; ++co)
      out[(size_t)r * cout_p + co] = (r < cin && co < cout) ? K[((size_t)tap * cout + co) * cin + r] : 0.f;
}

// the stand-alone arena of that 1x1x1 convolution: the matrix, then scale[cout_p] (1 in the
// padding) and shift[cout_p] (0 in the padding); ap holds cin_p * cout_p + 2 * cout_p floats
static inline void fpl_deconv_tap_arena(const float *K, const float *scale, const float *shift, int cin, int cout,
                                        int tap, int cin_p, int cout_p, float *ap) {
  fpl_deconv_tap_matrix(K, cin, cout, tap, cin_p, cout_p, ap);
  float *s = ap + (size_t)cin_p * cout_p;
  for (int co = 0; co < cout_p; ++co) {
    s[co] = co < cout ? scale[co] : 1.f;
    s[cout_p + co] = co < cout ? shift[co] : 0.f;
  }
}
