/* libfplassign.so: the matching of obj_pr / obj_pr_curve solved on the GPU (gfx950).
 *
 * libfplmatch.so (include/fplmatch.h) leaves the table of close (prediction, ground-truth)
 * pairs in device memory.  This library takes it from there: the exact costs and the
 * admissible rows, the connected components of the pair graph, and the assignment problem of
 * every component of at most FPLA_CAP x FPLA_CAP points - so that only the matched pairs
 * travel to the host.  flypylib_amd/match.py's match_device drives it; the sorts between the
 * stages are torch's.
 *
 * A library of its own: no context object, raw device pointers and a hipStream_t.  Every
 * function but fpla_last_error returns 0 on success and a non-zero rc with a thread-local
 * message otherwise; no C++ exception crosses this boundary.  Arguments are checked before the
 * GPU is touched.  Lists hold at most 2^31 - 1 entries and are indexed in 64 bits.
 *
 * No float atomics anywhere.  The one integer atomic is the atomicMin of fpla_labels, whose
 * fixed point does not depend on the order of the updates.
 */
#ifndef FPLASSIGN_H
#define FPLASSIGN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FPLA_ABI_VERSION 1

/* A block of FPLA_BLOCK threads owns FPLA_BLOCK consecutive list entries.  The kernels that
 * walk a list entry by entry run at most FPLA_MAX_BLOCKS blocks with a grid stride; the
 * compaction has one block, and one uint32 cell, per FPLA_BLOCK entries, scanned by one block
 * of FPLA_SCAN_THREADS threads.  fpla_solve runs one wavefront of FPLA_CAP lanes per block, a block
 * takes FPLA_CAP components at a time, and at most FPLA_SOLVE_BLOCKS blocks run with a grid stride. */
#define FPLA_BLOCK 256
#define FPLA_MAX_BLOCKS 256
#define FPLA_SCAN_THREADS 1024
#define FPLA_CAP 64
#define FPLA_SOLVE_BLOCKS 1024

const char *fpla_last_error(void);
int fpla_abi_version(void);

/* ---- ordered compaction: count, scan, fill (as libfplmatch.so builds its table) ----------- */

/* *bytes = the device scratch fpla_flags_count / _fill ask for a list of n entries:
 * 8 + 4 * ceil(n / FPLA_BLOCK), rounded up to 8 */
int fpla_scratch_bytes(int64_t n, int64_t *bytes);

/* fpla_flags_count counts the non-zero entries of flags[0 .. n) per block, scans the counts on
 * the device (scratch: 8-byte aligned device memory), copies the total to *total and waits
 * for `stream`.  fpla_flags_fill, given the same flags and the scratch the count left, visits
 * the flagged entries e in ascending order; the k-th of them writes, for every pointer that
 * is not null,
 *   a_out[k] = a[e],  b_out[k] = b[e],  c_out[k] = c[e],  index_out[k] = e
 * and rank_out (n entries) receives k at e, and -1 at every entry that is not flagged.  An
 * output at or beyond `capacity` is never written.  No atomics: the order does not depend on
 * scheduling.  fpla_flags_fill is asynchronous. */
int fpla_flags_count(const int32_t *flags, int64_t n, void *scratch, int64_t scratch_bytes,
                     int64_t *total, void *stream);
int fpla_flags_fill(const int32_t *flags, int64_t n, const void *scratch, int64_t scratch_bytes,
                    int64_t capacity, const int32_t *a, const int32_t *b, const double *c,
                    int32_t *a_out, int32_t *b_out, double *c_out, int32_t *index_out,
                    int32_t *rank_out, void *stream);

/* flags[k] = conf[k] >= thd; a NaN on either side compares false, so a NaN threshold selects
 * nothing, as numpy's comparison does; asynchronous */
int fpla_conf_flags(const double *conf, int64_t n, double thd, int32_t *flags, void *stream);

/* flags[0] = 1, flags[e] = keys[e] != keys[e - 1]: the first entry of every run of a sorted
 * list; asynchronous */
int fpla_boundaries(const int32_t *keys, int64_t n, int32_t *flags, void *stream);

/* ---- a. costs and the admissible set -------------------------------------------------------- */

/* For every row (ti[e], tj[e]) of a pair table, in float64 and every operation rounded on its
 * own (the expressions of match.pair_costs),
 *   d = pred[i] - gt[j] per coordinate,  cost = sqrt((d.x * d.x + d.y * d.y) + d.z * d.z) - t
 * and, if pred_lbl and gt_lbl (int64, both or neither) are given and differ at (i, j),
 * cost += label_add.  cost_out[e] = cost, keep_out[e] = cost < 0, i_out[e] = i.
 * With `rank` (n_pred entries, what fpla_flags_fill's rank_out left for fpla_conf_flags): a
 * row whose rank[i] < 0 is dropped, and i_out[e] = rank[i].  A row that names a point outside
 * the tables is dropped.  Asynchronous. */
int fpla_pair_costs(const int32_t *ti, const int32_t *tj, int64_t rows, const double *pred,
                    int64_t n_pred, const double *gt, int64_t n_gt, double t,
                    const int64_t *pred_lbl, const int64_t *gt_lbl, double label_add,
                    const int32_t *rank, int32_t *i_out, double *cost_out, int32_t *keep_out,
                    void *stream);

/* ---- b. component labels ---------------------------------------------------------------------- */

/* pair_label[e] = the smallest prediction index of the connected component of pair e in the
 * bipartite graph of the pairs (i[e], j[e]) - match.components_numpy is the specification.
 * Min-label propagation: pred_label (n_pred) and gt_label (n_gt) are work arrays, `changed`
 * one device int32; a sweep lowers both ends of every pair to their minimum, and sweeps are
 * launched until one leaves `changed` clear.  The flag is read back once per sweep, so the
 * call waits for `stream`.  The number of sweeps grows with the diameter of the largest
 * component; more than max_sweeps is an error.  *sweeps = the sweeps launched. */
int fpla_labels(const int32_t *i, const int32_t *j, int64_t rows, int64_t n_pred, int64_t n_gt,
                int32_t *pred_label, int32_t *gt_label, int32_t *changed, int32_t *pair_label,
                int64_t max_sweeps, int64_t *sweeps, void *stream);

/* ---- d. solve --------------------------------------------------------------------------------- */

/* The pairs (i, j, cost), cost < 0, ordered by (component, i, j); component k is the rows
 * starts[k] .. starts[k + 1] (n_comp + 1 offsets).  One wavefront per component, grid stride:
 * a component of one pair is matched; one of at most FPLA_CAP distinct i and FPLA_CAP
 * distinct j is solved in float64 by shortest augmenting paths on the block min(cost, 0),
 * absent pairs costing 0, and matched[e] = 1 for the assigned pairs of the list; a larger
 * one is left alone and overflow[k] = 1.  matched (rows) and overflow (n_comp) are cleared by
 * the caller.  Asynchronous. */
int fpla_solve(const int32_t *i, const int32_t *j, const double *cost, int64_t rows,
               const int32_t *starts, int64_t n_comp, int32_t *matched, int32_t *overflow,
               void *stream);

#ifdef __cplusplus
}
#endif
#endif
