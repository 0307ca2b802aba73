/* libfpllabels.so: training labels and mask around annotated T-bars on the GPU (gfx950).
 *
 * The first step of the U-Net workflow (fplsynapses.write_labels_mask): a library of its
 * own beside libfplhip.so (include/fplhip.h), libfplbatch.so (include/fplbatch.h) and
 * libfplmine.so (include/fplmine.h): no context object, raw device pointers and a
 * hipStream_t.  Every function but fpll_last_error returns 0 on success and a non-zero rc
 * with a thread-local message otherwise; no C++ exception crosses this boundary.  Arguments
 * are checked before the GPU is touched.
 *
 * Volumes are C order, dims[3] = (Z, Y, X), and hold at most 2^31 - 1 voxels; a larger
 * volume is refused, never wrapped.  labels_mask_numpy of flypylib_amd/labels.py is the
 * specification of the result, plan_bricks of the same file the planner of the brick lists.
 */
#ifndef FPLLABELS_H
#define FPLLABELS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FPLL_ABI_VERSION 1

/* the volume is cut into bricks of FPLL_BRICK_Z x FPLL_BRICK_Y x FPLL_BRICK_X voxels, in C
 * order of (brick z, brick y, brick x); a partial brick ends at the volume's end */
#define FPLL_BRICK_Z 4
#define FPLL_BRICK_Y 8
#define FPLL_BRICK_X 128
/* the largest radius: squared distances inside a cube stay far below 2^31 */
#define FPLL_MAX_RADIUS 1024

const char *fpll_last_error(void);
int fpll_abi_version(void);

/* labels and mask of a resident roi_mask in one pass (3 bytes per voxel).  With, per voxel v,
 *   J_set   = the largest j with d2(v, T-bar j) <= radius_use^2
 *   J_clr   = the largest j with d2(v, T-bar j) <= radius_ign^2        (radius_ign > 0 only)
 *   touched = v lies in the cube of half-width max(radius_use, radius_ign) of any T-bar
 *   labels = J_set exists
 *   mask   = 1 if J_set exists and (no J_clr or J_set >= J_clr), else 0 if J_clr exists,
 *            else (roi != 0) if touched, else roi
 *   mask   = 0 within buffer_size voxels of a face; buffer_size 0 clears the whole mask, as
 *            the slice mask[-0:] of the host code does
 * d2 is the integer squared distance.  tbars: n_tbars rows of int32 (x, y, z).  The T-bars a
 * brick has to look at are given as a CSR table over the bricks: brick b's candidates are
 * brick_index[brick_offsets[b] .. brick_offsets[b + 1]), row numbers of tbars in any order;
 * every T-bar whose cube meets the brick must be among them, others may be.  brick_offsets
 * has one int32 per brick and one more; with n_index == 0 it and brick_index may be null.
 * A row number outside [0, n_tbars) and offsets outside [0, n_index] are skipped, never
 * followed.  roi, labels and mask are distinct buffers of Z * Y * X bytes at any alignment.
 * No atomics: the result does not depend on scheduling.  `stream` is a hipStream_t; the
 * launch is asynchronous. */
int fpll_labels_mask(const uint8_t *roi, const int32_t *tbars, int64_t n_tbars,
                     const int32_t *brick_offsets, const int32_t *brick_index, int64_t n_index,
                     const int64_t dims[3], int32_t radius_use, int32_t radius_ign,
                     int32_t buffer_size, uint8_t *labels, uint8_t *mask, void *stream);

#ifdef __cplusplus
}
#endif
#endif
