/* libfplplan.so: the brick tables of the device write_labels_mask, planned on the GPU (gfx950).
 *
 * A stage library beside libfpllabels.so (include/fpllabels.h), whose kernel reads the table
 * built here: no context object, raw device pointers and a hipStream_t.  Every function but
 * fplp_last_error returns 0 on success and a non-zero rc with a thread-local message
 * otherwise; no C++ exception crosses this boundary.  Arguments are checked before the GPU
 * is touched.
 *
 * Volumes are C order, dims[3] = (Z, Y, X), and hold at most 2^31 - 1 voxels; a larger volume
 * is refused, never wrapped.  plan_bricks of flypylib_amd/labels.py is the specification of
 * the table: the arrays written here are equal to its arrays byte for byte.
 */
#ifndef FPLPLAN_H
#define FPLPLAN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FPLP_ABI_VERSION 1

/* the bricks of include/fpllabels.h (FPLL_BRICK_*), in C order of (brick z, brick y, brick x) */
#define FPLP_BRICK_Z 4
#define FPLP_BRICK_Y 8
#define FPLP_BRICK_X 128
/* the largest half-width: FPLL_MAX_RADIUS */
#define FPLP_MAX_RADIUS 1024

const char *fplp_last_error(void);
int fplp_abi_version(void);

/* *bytes = the scratch fplp_plan_bricks asks for (8-byte aligned device memory): a status word,
 * the partial sums of the scan, one cursor per brick and a staging list of n_index rows.
 * n_bricks = the product of ceil(dims[a] / FPLP_BRICK_a); counts beyond 2^31 - 1 are refused. */
int fplp_scratch_bytes(int64_t n_tbars, int64_t n_bricks, int64_t n_index, int64_t *bytes);

/* The CSR table of the T-bars each brick has to look at.  tbars: n_tbars rows of int32
 * (x, y, z).  T-bar j belongs to every brick (bz, by, bx) with
 *   max((c - half) / brick, 0) <= b <= min((c + half) / brick, bricks - 1)     (floor division)
 * on each axis, c its coordinate there.  offsets (one int32 per brick and one more) receives the
 * exclusive prefix sums of the bricks' list lengths and, last, their total; index (n_index
 * int32) receives brick b's T-bars at [offsets[b], offsets[b + 1]) in ascending j, the same
 * on every run.  n_index is the total the caller expects (labels.plan_pairs computes it on the
 * host).  With n_tbars == 0 tbars may be null, with n_index == 0 index may be.
 *
 * Everything runs on `stream` (a hipStream_t) and nothing waits for it.  The first int32 of
 * scratch is a status word: 0 after success, non-zero when the pairs counted on the device
 * differ from n_index; then offsets holds the counted table and index is not written at all.
 * Read it after synchronising the stream.  No row outside [0, n_index) is ever written. */
int fplp_plan_bricks(const int32_t *tbars, int64_t n_tbars, const int64_t dims[3], int32_t half,
                     int32_t *offsets, int32_t *index, int64_t n_index, void *scratch,
                     int64_t scratch_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
