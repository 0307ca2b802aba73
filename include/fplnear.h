/* libfplnear.so: the close pairs WITHIN one point set on the GPU (gfx950), for
 * fplsynapses.rm_tbar_multi_pred.
 *
 * full_roi_inference ends with one large point list in which a T-bar on a substack border can
 * appear twice.  Merging the duplicates needs, per point, the points closer than a threshold:
 * a self-join of 10^5 - 10^7 points, so testing every pair (libfplmatch.so's way) is the wrong
 * algorithm.  Here the points are binned into cells of about the threshold and a point is
 * tested against the 27 cells around its own.  A library of its own beside libfplhip.so
 * (include/fplhip.h): no context object, raw device pointers and a hipStream_t.  Every function
 * but fpln_last_error returns 0 on success and a non-zero rc with a thread-local message
 * otherwise; no C++ exception crosses this boundary.  Arguments are checked before the GPU is
 * touched.
 *
 * Points are float64 rows (x, y, z), C order, at most 2^31 - 1; a table holds at most 2^31 - 1
 * entries (uint32 row offsets, int32 columns).  What is larger is refused, never wrapped.
 * flypylib_amd/near.py's pairs_numpy is the specification of the table, byte for byte.
 */
#ifndef FPLNEAR_H
#define FPLNEAR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FPLN_ABI_VERSION 1

/* A block of FPLN_BLOCK threads owns FPLN_BLOCK points, one each, taken in the order of their
 * cell keys.  The row lengths of the n points are scanned by one block of FPLN_SCAN_THREADS
 * threads.  An axis of the cell grid has at most 2^FPLN_MAX_AXIS_BITS cells: up to there the
 * rounding of a cell coordinate stays inside the margin of the cell side (below). */
#define FPLN_BLOCK 256
#define FPLN_SCAN_THREADS 1024
#define FPLN_MAX_AXIS_BITS 28

const char *fpln_last_error(void);
int fpln_abi_version(void);

/* *bytes = the device scratch fpln_pairs_count / _fill ask for:
 *   16 + 4 * (n + 1) (row offsets, padded to 8) + 4 * n (the order, padded to 8) + 24 * n (the
 *   points in that order) */
int fpln_scratch_bytes(int64_t n, int64_t *bytes);

/* The cell grid.  origin (3 doubles, x y z) and dims (3 int64: nx, ny, nz >= 1) are HOST
 * arrays; `cell` is the side of a cell.  In float64, every operation rounded on its own, a
 * point's cell along an axis is
 *   floor(min(max((x - origin.x) / cell, 0), nx - 1))
 * and its key (cz * ny + cy) * nx + cx, so the three x-adjacent cells of a row are one key
 * range.  nx, ny, nz <= 2^FPLN_MAX_AXIS_BITS and nx * ny * nz <= 2^62, or the call is refused.
 * fpln_pairs_count and _fill find a point's partners in the 27 cells around its own, so they
 * ask for  cell >= sqrt(T2) * (1 + 2^-20):  two points no further apart than sqrt(T2) on an
 * axis then lie at most one cell apart on it, the rounding above included.  origin is meant to
 * be the minimum of the point set and dims its extent in cells; a point outside is clamped
 * into the outermost cells, which keeps that property.
 *
 * fpln_cell_keys writes the n keys (device int64) and is asynchronous.  Sorting them is the
 * caller's: the other two calls take the sorted keys and the order that sorts them. */
int fpln_cell_keys(const double *locs, int64_t n, const double *origin, double cell,
                   const int64_t *dims, int64_t *keys, void *stream);

/* The table, in CSR form: row i holds every j with 0 < s <= T2, in ascending j, where in
 * float64, every operation rounded on its own,
 *   d = locs[i] - locs[j]  per coordinate,   s = (d.x * d.x + d.y * d.y) + d.z * d.z
 * so a point is no partner of itself nor of a coincident point, and both (i, j) and (j, i) are
 * stored.
 *
 * sorted_keys (device int64, ascending) are the keys of fpln_cell_keys for the same locs and
 * grid, order (device int64) the permutation that sorts them: sorted_keys[k] is the key of
 * point order[k].  Points of equal key may come in any order; the table does not depend on it.
 * An entry of `order` outside [0, n) is reported by fpln_pairs_count, never followed.
 *
 * fpln_pairs_count gathers the points into the scratch in that order, counts each point's
 * partners, scans the counts on the device (scratch: at least fpln_scratch_bytes bytes of
 * device memory, 8-byte aligned), copies the total to *total and waits for `stream`; a total
 * above 2^31 - 1 is refused.  The n + 1 row offsets (uint32) then stand at scratch + 16.
 * fpln_pairs_fill, given the same arguments and the scratch the count left, writes the first
 * `capacity` entries of the column array into `indices` (int32, 4-byte aligned): an entry goes
 * to its row's offset plus the number of the row's smaller entries.  No atomics: the bytes do
 * not depend on scheduling.  An entry at or beyond `capacity` is never written.
 * fpln_pairs_fill is asynchronous.  n is positive, T2 finite and positive. */
int fpln_pairs_count(const double *locs, int64_t n, double T2, const double *origin, double cell,
                     const int64_t *dims, const int64_t *sorted_keys, const int64_t *order,
                     void *scratch, int64_t scratch_bytes, int64_t *total, void *stream);
int fpln_pairs_fill(const double *locs, int64_t n, double T2, const double *origin, double cell,
                    const int64_t *dims, const int64_t *sorted_keys, const int64_t *order,
                    const void *scratch, int64_t scratch_bytes, int64_t capacity,
                    int32_t *indices, void *stream);

#ifdef __cplusplus
}
#endif
#endif
