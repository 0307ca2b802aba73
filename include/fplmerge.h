/* libfplmerge.so: the merge loop of fplsynapses.rm_tbar_multi_pred on the GPU (gfx950), from the
 * resident neighbour table of libfplnear.so (include/fplnear.h) to the removed / moved flags and
 * the moved locations (solver='device').
 *
 * The loop is sequential in order of falling confidence.  It is run per connected component of the
 * neighbour table, optimistically: a run raises its component's flag as soon as something happens
 * that it cannot reproduce exactly (fplg_solve lists the causes), and the caller runs the flagged
 * components on the host (flypylib_amd/dedupe.py; DESIGN.md section 14.1 has the argument why the
 * result is the sequential loop's).  flypylib_amd/dedupe.py's merge_numpy is the specification of
 * every output here, byte for byte.
 *
 * A library of its own beside libfplhip.so: no context object, raw device pointers and a
 * hipStream_t.  Every function but fplg_last_error returns 0 on success and a non-zero rc with a
 * thread-local message otherwise; no C++ exception crosses this boundary.  Arguments are checked
 * before the GPU is touched, and every index read from device memory is range-checked before it
 * is followed.  No atomics of any kind: every output word has one writer, or every writer writes
 * the same value.
 *
 * Points are float64 rows (x, y, z), C order, at most 2^31 - 1; tables have uint32 row offsets
 * (n + 1) and int32 columns, at most 2^31 - 1 entries.
 */
#ifndef FPLMERGE_H
#define FPLMERGE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FPLG_ABI_VERSION 1

/* A block of FPLG_BLOCK threads owns FPLG_BLOCK points, or list entries, one each; the
 * grid-stride kernels launch at most FPLG_MAX_BLOCKS of them.  Counts are scanned by one block of
 * FPLG_SCAN_THREADS threads.  fplg_solve gives a component to a lane: blocks of FPLG_SOLVE_BLOCK
 * threads (one wavefront), at most FPLG_SOLVE_BLOCKS of them, which stride over the rest.
 * FPLG_CAND_CAP is the largest candidate set a run accepts: below 8 elements numpy's sum is a
 * plain left-to-right loop, which is the order reproduced here - the pairwise form numpy uses
 * from 8 on is not, so larger sets go to the host.  FPLG_COMP_CAP and FPLG_MAX_MOVES bound what
 * the caller may ask for (points of a component; moves of one point). */
#define FPLG_BLOCK 256
#define FPLG_MAX_BLOCKS 1024
#define FPLG_SCAN_THREADS 1024
#define FPLG_SOLVE_BLOCK 64
#define FPLG_SOLVE_BLOCKS 1024
#define FPLG_CAND_CAP 7
#define FPLG_COMP_CAP 4096
#define FPLG_MAX_MOVES 4096

const char *fplg_last_error(void);
int fplg_abi_version(void);

/* ---- the rows the reference keeps ------------------------------------------------------------
 * The table of libfplnear.so is a superset (0 < s <= T2).  Row i of the filtered table keeps the
 * j of row i with  d > 0  and  d < t,  d = sqrt((dx*dx + dy*dy) + dz*dz)  in float64, every
 * operation rounded on its own and the square root correctly rounded: numpy's
 * np.sqrt(((a - b) ** 2).sum(axis=1)).  The order of a row (ascending j) is kept.
 *
 * fplg_rows_count writes has_neighbor[i] (uint32, n), the length of filtered row i - the
 * reference's has_neighbor, which ignores labels - scans the lengths into out_offsets (uint32,
 * n + 1; head: 16 bytes of device memory, 8-byte aligned, which receive the total), copies the
 * total to *total and waits for `stream`.  fplg_rows_fill, given the same arguments and the
 * offsets the count left, writes the first `capacity` columns into out_indices (int32); it is
 * asynchronous.  A column outside [0, n) is kept out of both.  offsets / indices / entries are
 * the table of fpln_pairs_count / _fill: offsets[i] <= offsets[i + 1] <= entries is not assumed,
 * a row is cut at `entries`. */
int fplg_rows_count(const double *locs, int64_t n, double t, const uint32_t *offsets,
                    const int32_t *indices, int64_t entries, uint32_t *has_neighbor,
                    uint32_t *out_offsets, void *head, int64_t *total, void *stream);
int fplg_rows_fill(const double *locs, int64_t n, double t, const uint32_t *offsets,
                   const int32_t *indices, int64_t entries, const uint32_t *out_offsets,
                   int64_t capacity, int32_t *out_indices, void *stream);

/* ---- the components --------------------------------------------------------------------------
 * label[i] = the smallest index of the connected component of point i in the (symmetric) table.
 * Min-label propagation, pulled: in a sweep a thread owns a point and writes the minimum of its
 * own label and its row's labels, read from the labels of the sweep before (two buffers, label
 * and other, int32, n each).  One writer per word and no atomic, so a sweep is a function of the
 * sweep before and THE SWEEP COUNT IS THE SAME IN EVERY RUN: the longest shortest path from a
 * component's smallest index, plus the sweep that sees nothing change.  `changed` (device int32)
 * is read back after every sweep; *sweeps receives their number.  After more than max_sweeps the
 * call fails.  Both buffers hold the result.  Waits for `stream`. */
int fplg_labels(const uint32_t *offsets, const int32_t *indices, int64_t n, int64_t entries,
                int32_t *label, int32_t *other, int32_t *changed, int64_t max_sweeps,
                int64_t *sweeps, void *stream);

/* ---- the grouping ----------------------------------------------------------------------------
 * fplg_group_keys: keys[i] (int64) = label[i] * 2^32 + rank[i] for a point whose row of the table
 * is not empty, (2^31 - 1) * 2^32 + rank[i] for one whose row is empty (it is a component by
 * itself and has nothing to do).  rank (int32) is the point's place in the host's
 * np.argsort(-conf).  Sorting the keys is the caller's (torch.sort): the points of a component
 * then stand together, in the order the reference visits them, the idle points last.
 * fplg_boundaries: flags (int32, n + 1) from the SORTED keys: flags[e] = 1 where the upper half of
 * keys[e] differs from that of keys[e - 1] (e = 0: always), and flags[n] = 1 if the last key is
 * not an idle point's.  The flagged positions are the starts of the K components and, last, the
 * end of the K-th: K + 1 of them for n >= 1.  Both calls are asynchronous. */
int fplg_group_keys(const uint32_t *offsets, const int32_t *label, const int32_t *rank, int64_t n,
                    int64_t *keys, void *stream);
int fplg_boundaries(const int64_t *sorted_keys, int64_t n, int32_t *flags, void *stream);

/* ---- the ordered compaction of a flag list ------------------------------------------------------
 * The indices of the non-zero entries of flags (int32, n), ascending.  fplg_flags_count counts
 * them per block of FPLG_BLOCK entries, scans the counts (the shared block scan) into the scratch
 * (fplg_scratch_bytes(n) bytes of device memory, 8-byte aligned: the total, then a uint32 per
 * block), copies the total to *total and waits for `stream`.  fplg_flags_fill, given the scratch
 * the count left, writes the first `capacity` indices into index_out (int32); asynchronous.
 * Used for the component starts and for the ids of the flagged components. */
int fplg_scratch_bytes(int64_t n, int64_t *bytes);
int fplg_flags_count(const int32_t *flags, int64_t n, void *scratch, int64_t scratch_bytes,
                     int64_t *total, void *stream);
int fplg_flags_fill(const int32_t *flags, int64_t n, const void *scratch, int64_t scratch_bytes,
                    int64_t capacity, int32_t *index_out, void *stream);

/* ---- the merge loop ----------------------------------------------------------------------------
 * Component k is the points members[starts[k] .. starts[k + 1]) (members: int64, the order that
 * sorts the group keys; starts: int32, n_comp + 1).  A lane owns a component and runs the loop of
 * rm_tbar_multi_pred(method='sparse') over its points in that order:
 *   - a point that is removed, or whose filtered row (f_offsets, f_indices, f_entries; has no
 *     entry) is empty, is passed over;
 *   - the first candidates are the row's points of the point's own label (labels: int64, n) that
 *     are not removed; with none the point is passed over, else it is marked moved, joins the
 *     candidates, and until the rounded mean rests:
 *       ww = conf[c] / sum(conf[c]) over the candidates in ASCENDING INDEX order, the sum from
 *       0.0 left to right; mean = the rows ww[c] * locs[c] added one after the other, per axis;
 *       every operation rounded on its own; the new location is the mean rounded half to even;
 *       if it equals the old location (at first the point's own) the loop ends; else the
 *       candidates are the points closer than t to it (sqrt(...) < t as above), of the point's
 *       label, of this component, not removed - found in the 27 cells around it by the sorted
 *       cell keys of fpln_cell_keys (sorted_keys, order, and the grid's origin, cell, dims as in
 *       fplnear.h; cell >= t (1 + 2^-20));
 *   - the last candidates are removed.
 * The caller clears rm where mv is set at the very end (the reference's last line).
 *
 * A run raises flagged[c] (int32, n; c the component's label, its smallest point index) and
 * leaves the component as it is - the caller discards its outputs - when
 *   - a point of ANOTHER component passes the distance and label tests of a ball query, whatever
 *     its removed state (its component's flag is raised as well; the whole ball is looked at, so
 *     the flags do not depend on the order of the cell keys);
 *   - a candidate set has more than cand_cap points (1 .. FPLG_CAND_CAP) or none;
 *   - a mean is not finite or not below 2^62 in magnitude;
 *   - a point would move more than max_moves times (1 .. FPLG_MAX_MOVES): the reference's
 *     `while True` may cycle between two centres;
 *   - the component has more than comp_cap points (1 .. FPLG_COMP_CAP).
 * Every loop is bounded by one of these numbers, by a row's length or by n, never by a value.
 *
 * rm, mv (uint8, n), mv_loc (int64, 3 n) and flagged are cleared by the caller; a lane writes the
 * rm / mv / mv_loc of its own component's points only and reads rm of those only, so no run sees
 * another's state.  Asynchronous. */
int fplg_solve(const double *locs, const double *conf, const int64_t *labels, const int32_t *comp,
               int64_t n, double t, const double *origin, double cell, const int64_t *dims,
               const int64_t *sorted_keys, const int64_t *order, const uint32_t *f_offsets,
               const int32_t *f_indices, int64_t f_entries, const int64_t *members,
               const int32_t *starts, int64_t n_comp, int64_t cand_cap, int64_t comp_cap,
               int64_t max_moves, uint8_t *rm, uint8_t *mv, int64_t *mv_loc, int32_t *flagged,
               void *stream);

#ifdef __cplusplus
}
#endif
#endif
