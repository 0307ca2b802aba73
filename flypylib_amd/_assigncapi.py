"""ctypes binding of libfplassign.so (include/fplassign.h): the sparse matching of obj_pr /
obj_pr_curve solved on the GPU - costs, component labels, the per-component assignment and
the ordered compaction between them.

A missing library is an error (`FplAssignError`), never a silent fallback to the host solver.
The functions here take raw device addresses and a raw hipStream_t; flypylib_amd/match.py's
match_device puts torch tensors around them.
"""
import ctypes as C

from ._sidelib import SideLibrary

ABI_VERSION = 1
BLOCK = 256                  # FPLA_BLOCK: list entries per block, and per compaction cell
MAX_BLOCKS = 256             # FPLA_MAX_BLOCKS: of a grid-stride kernel
SCAN_THREADS = 1024          # FPLA_SCAN_THREADS
SOLVE_BLOCKS = 1024          # FPLA_SOLVE_BLOCKS: of fpla_solve's grid, 64 components a block at a time
CAP = 64                     # FPLA_CAP: distinct predictions, and ground-truth points, of a solved component
MAX_ENTRIES = 2 ** 31 - 1    # of any list


class FplAssignError(RuntimeError):
    pass


_vp, _i64, _f64 = C.c_void_p, C.c_int64, C.c_double

# name -> (restype, argtypes); every symbol include/fplassign.h declares
SIGNATURES = {
    'fpla_last_error': (C.c_char_p, []),
    'fpla_abi_version': (C.c_int, []),
    'fpla_scratch_bytes': (C.c_int, [_i64, C.POINTER(_i64)]),
    'fpla_flags_count': (C.c_int, [_vp, _i64, _vp, _i64, C.POINTER(_i64), _vp]),
    'fpla_flags_fill': (C.c_int, [_vp, _i64, _vp, _i64, _i64] + [_vp] * 9),
    'fpla_conf_flags': (C.c_int, [_vp, _i64, _f64, _vp, _vp]),
    'fpla_boundaries': (C.c_int, [_vp, _i64, _vp, _vp]),
    'fpla_pair_costs': (C.c_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _f64, _vp, _vp, _f64,
                                  _vp, _vp, _vp, _vp, _vp]),
    'fpla_labels': (C.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64,
                              C.POINTER(_i64), _vp]),
    'fpla_solve': (C.c_int, [_vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp]),
}

_side = SideLibrary('assign', FplAssignError, SIGNATURES, ABI_VERSION,
                    "the device solver has no host fallback; use solver='host' for scipy's")
LIB_PATH, load_library, check = _side.path, _side.load, _side.check


def _p(address):
    return _vp(address or None)


def scratch_bytes(n):
    """bytes of device scratch flags_count / flags_fill ask for a list of n entries"""
    lib = load_library()
    out = _i64(0)
    check(lib, lib.fpla_scratch_bytes(int(n), C.byref(out)))
    return out.value


def flags_count(flags_ptr, n, scratch_ptr, n_scratch, stream):
    """the number of non-zero flags; the scanned block offsets stay in the scratch buffer.
    Waits for `stream` (a raw hipStream_t)."""
    lib = load_library()
    total = _i64(-1)
    check(lib, lib.fpla_flags_count(_p(flags_ptr), int(n), _p(scratch_ptr), int(n_scratch),
                                    C.byref(total), _vp(stream)))
    return total.value


def flags_fill(flags_ptr, n, scratch_ptr, n_scratch, capacity, stream, a=0, b=0, c=0, a_out=0,
               b_out=0, c_out=0, index_out=0, rank_out=0):
    """the flagged entries in order: their a, b (int32) and c (float64) columns, their
    indices, and every entry's rank or -1 - whichever outputs are given; asynchronous"""
    lib = load_library()
    check(lib, lib.fpla_flags_fill(_p(flags_ptr), int(n), _p(scratch_ptr), int(n_scratch),
                                   int(capacity), _p(a), _p(b), _p(c), _p(a_out), _p(b_out),
                                   _p(c_out), _p(index_out), _p(rank_out), _vp(stream)))


def conf_flags(conf_ptr, n, thd, flags_ptr, stream):
    """flags = conf >= thd; asynchronous"""
    lib = load_library()
    check(lib, lib.fpla_conf_flags(_p(conf_ptr), int(n), float(thd), _p(flags_ptr), _vp(stream)))


def boundaries(keys_ptr, n, flags_ptr, stream):
    """flags = the first entry of every run of equal keys; asynchronous"""
    lib = load_library()
    check(lib, lib.fpla_boundaries(_p(keys_ptr), int(n), _p(flags_ptr), _vp(stream)))


def pair_costs(ti_ptr, tj_ptr, rows, pred_ptr, n_pred, gt_ptr, n_gt, t, pred_lbl_ptr, gt_lbl_ptr,
               label_add, rank_ptr, i_out_ptr, cost_out_ptr, keep_out_ptr, stream):
    """per row of the table: the (renumbered) prediction, the cost and whether the row is
    admissible; asynchronous"""
    lib = load_library()
    check(lib, lib.fpla_pair_costs(_p(ti_ptr), _p(tj_ptr), int(rows), _p(pred_ptr), int(n_pred),
                                   _p(gt_ptr), int(n_gt), float(t), _p(pred_lbl_ptr),
                                   _p(gt_lbl_ptr), float(label_add), _p(rank_ptr), _p(i_out_ptr),
                                   _p(cost_out_ptr), _p(keep_out_ptr), _vp(stream)))


def labels(i_ptr, j_ptr, rows, n_pred, n_gt, pred_label_ptr, gt_label_ptr, changed_ptr,
           pair_label_ptr, max_sweeps, stream):
    """the component label of every pair; -> the sweeps it took.  Waits for `stream`."""
    lib = load_library()
    sweeps = _i64(0)
    check(lib, lib.fpla_labels(_p(i_ptr), _p(j_ptr), int(rows), int(n_pred), int(n_gt),
                               _p(pred_label_ptr), _p(gt_label_ptr), _p(changed_ptr),
                               _p(pair_label_ptr), int(max_sweeps), C.byref(sweeps), _vp(stream)))
    return sweeps.value


def solve(i_ptr, j_ptr, cost_ptr, rows, starts_ptr, n_comp, matched_ptr, overflow_ptr, stream):
    """matched[e] = 1 on the assigned pairs, overflow[k] = 1 on the components beyond the cap;
    both cleared by the caller; asynchronous"""
    lib = load_library()
    check(lib, lib.fpla_solve(_p(i_ptr), _p(j_ptr), _p(cost_ptr), int(rows), _p(starts_ptr),
                              int(n_comp), _p(matched_ptr), _p(overflow_ptr), _vp(stream)))
