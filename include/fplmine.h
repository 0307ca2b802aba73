/* libfplmine.so: hard-example mining on the GPU (gfx950).
 *
 * The step between two training rounds of the U-Net workflow: the per-voxel loss of the
 * current prediction (FplNetwork.voxel_loss) and the candidate tables gen_volume2 draws its
 * centres from.  A library of its own beside libfplhip.so (include/fplhip.h) and
 * libfplbatch.so (include/fplbatch.h): no context object, raw device pointers and a
 * hipStream_t.  Every function but fplm_last_error returns 0 on success and a non-zero rc
 * with a thread-local message otherwise; no C++ exception crosses this boundary.  Arguments
 * are checked before the GPU is touched.
 *
 * Volumes are C order, dims[3] = (Z, Y, X), and hold at most 2^31 - 1 voxels: the candidate
 * rows are int32 and so are their counts; a larger volume is refused, never wrapped.  The
 * numpy executors of flypylib_amd/mine.py are the specification of every result.
 */
#ifndef FPLMINE_H
#define FPLMINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FPLM_ABI_VERSION 1

/* candidates are counted over fixed flat chunks of FPLM_CHUNK voxels; the scratch buffer
 * of fplm_candidates_count / _fill holds one uint32 per chunk and the total behind them */
#define FPLM_CHUNK 4096
#define FPLM_SCRATCH_BYTES(n_voxels) \
  ((((int64_t)(n_voxels) + FPLM_CHUNK - 1) / FPLM_CHUNK + 1) * 4)

const char *fplm_last_error(void);
int fplm_abi_version(void);

/* loss[v] of every voxel of a resident volume, one pass (10 bytes per voxel):
 *   m   = mask == 1 and the voxel is at least edge[a] from both faces on every axis a
 *   neg = m and labels == 0;   pos = m and labels == 1
 *   l   = -(double)LOG32(max(neg ? fl32(1 - pred) : pred, fl32(1e-8)))     neg or pos
 *   a neg voxel with l < 0.005 is confident: its loss is 0
 *   otherwise, with the class's [lo, hi] pair present, l = min(max(l, lo), hi)
 *   loss = fl32(l), and 0 for a voxel that is neither neg nor pos
 * LOG32(x) = (float)log((double)x).  has_l0 / has_l1 say whether the pair of class 0 / 1
 * is present.  `stream` is a hipStream_t; the launch is asynchronous. */
int fplm_voxel_loss(const float *pred, const uint8_t *labels, const uint8_t *mask,
                    const int64_t dims[3], const int32_t edge[3], int32_t has_l0, double l0_lo,
                    double l0_hi, int32_t has_l1, double l1_lo, double l1_hi, float *loss,
                    void *stream);

/* Candidates of class cc: the voxels with labels == cc, mask == 1, at least half[a] from
 * both faces on every axis and, when `weights` is not null, weights > 0 - in C order, as
 * numpy's nonzero() lists them.
 *
 * fplm_candidates_count counts them per chunk, scans the counts on the device (scratch:
 * at least FPLM_SCRATCH_BYTES(voxels) bytes of device memory, 4-byte aligned), copies the
 * total to *total and waits for `stream`.  fplm_candidates_fill, given the same volume,
 * arguments and the scratch the count left, writes the first `capacity` rows: int32
 * columns z, y, x and, with weights, the float32 weight of each row into w_out (null
 * otherwise).  No atomics: the rows and their order do not depend on scheduling.  A row
 * beyond `capacity` is never written.  fplm_candidates_fill is asynchronous. */
int fplm_candidates_count(const uint8_t *labels, const uint8_t *mask, const float *weights,
                          const int64_t dims[3], const int32_t half[3], int32_t cc,
                          void *scratch, int64_t scratch_bytes, int64_t *total, void *stream);
int fplm_candidates_fill(const uint8_t *labels, const uint8_t *mask, const float *weights,
                         const int64_t dims[3], const int32_t half[3], int32_t cc,
                         const void *scratch, int64_t scratch_bytes, int64_t capacity,
                         int32_t *z_out, int32_t *y_out, int32_t *x_out, float *w_out,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif
