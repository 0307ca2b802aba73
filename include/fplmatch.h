/* libfplmatch.so: the admissible pairs of obj_pr / obj_pr_curve on the GPU (gfx950).
 *
 * Evaluation matches predicted points to ground-truth points that lie closer than a distance
 * threshold.  Almost every (prediction, ground-truth) pair is further apart than that, so the
 * assignment problem is solved on the sparse table of the close pairs; this library finds
 * that table by testing every pair.  A library of its own beside libfplhip.so
 * (include/fplhip.h): no context object, raw device pointers and a hipStream_t.  Every
 * function but fple_last_error returns 0 on success and a non-zero rc with a thread-local
 * message otherwise; no C++ exception crosses this boundary.  Arguments are checked before the
 * GPU is touched.
 *
 * Points are float64 rows (x, y, z), C order, at most 2^31 - 1 of each kind; a table holds at
 * most 2^31 - 1 rows (int32 columns).  What is larger is refused, never wrapped.
 * flypylib_amd/match.py's pairs_numpy is the specification of the table, row for row.
 */
#ifndef FPLMATCH_H
#define FPLMATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FPLE_ABI_VERSION 1

/* A block of FPLE_BLOCK predictions (one per thread) streams ground-truth points through LDS
 * in tiles of FPLE_TILE points.  The ground-truth range is cut into G segments of
 *   ceil(ceil(n_gt / FPLE_TILE) / G)   whole tiles
 * (the last may be short or empty), one grid row each, so that few predictions still fill the
 * machine:
 *   G = the least power of two >= min(tiles, ceil(FPLE_TARGET_BLOCKS / blocks)), at most
 *       FPLE_MAX_SEGMENTS,   blocks = ceil(n_pred / FPLE_BLOCK), tiles = ceil(n_gt / FPLE_TILE)
 * The counts of the n_pred * G (prediction, segment) cells are scanned by one block of
 * FPLE_SCAN_THREADS threads.  The scratch holds the int64 total and one uint32 per cell. */
#define FPLE_BLOCK 256
#define FPLE_TILE 256
#define FPLE_MAX_SEGMENTS 64
#define FPLE_TARGET_BLOCKS 1024
#define FPLE_SCAN_THREADS 1024

const char *fple_last_error(void);
int fple_abi_version(void);

/* *bytes = the device scratch fple_pairs_count / _fill ask for: 8 + 4 * n_pred * G */
int fple_scratch_bytes(int64_t n_pred, int64_t n_gt, int64_t *bytes);

/* The pairs (i, j) with s <= T2, where in float64, every operation rounded on its own,
 *   d = pred[i] - gt[j]  per coordinate,   s = (d.x * d.x + d.y * d.y) + d.z * d.z
 * in ascending (i, j) order.
 *
 * fple_pairs_count counts them per (prediction, segment), scans the counts on the device
 * (scratch: at least fple_scratch_bytes bytes of device memory, 8-byte aligned), copies the
 * total to *total and waits for `stream`; a total above 2^31 - 1 is refused.
 * fple_pairs_fill, given the same points, T2 and the scratch the count left, writes the first
 * `capacity` rows into the int32 columns i_out, j_out.  No atomics: the rows and their order
 * do not depend on scheduling.  A row at or beyond `capacity` is never written.
 * fple_pairs_fill is asynchronous.  n_pred and n_gt are positive, T2 finite and positive. */
int fple_pairs_count(const double *pred, int64_t n_pred, const double *gt, int64_t n_gt,
                     double T2, void *scratch, int64_t scratch_bytes, int64_t *total,
                     void *stream);
int fple_pairs_fill(const double *pred, int64_t n_pred, const double *gt, int64_t n_gt,
                    double T2, const void *scratch, int64_t scratch_bytes, int64_t capacity,
                    int32_t *i_out, int32_t *j_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
