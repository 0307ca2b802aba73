"""ctypes binding of libfplmerge.so (include/fplmerge.h): the merge loop of
fplsynapses.rm_tbar_multi_pred on the GPU - the rows the reference keeps, the components of the
neighbour table, the grouping by (component, rank), the per-component loop and the ordered
compaction between them.

A missing library is an error (`FplMergeError`), never a silent fallback to the host loop.
The functions here take raw device addresses and a raw hipStream_t; flypylib_amd/dedupe.py's
merge_device puts torch tensors around them.
"""
import ctypes as C

from ._sidelib import SideLibrary

ABI_VERSION = 1
BLOCK = 256                  # FPLG_BLOCK: points, or list entries, per block and per compaction cell
MAX_BLOCKS = 1024            # FPLG_MAX_BLOCKS: of a grid-stride kernel
SCAN_THREADS = 1024          # FPLG_SCAN_THREADS
SOLVE_BLOCK = 64             # FPLG_SOLVE_BLOCK: components per block of fplg_solve, a lane each
SOLVE_BLOCKS = 1024          # FPLG_SOLVE_BLOCKS: of fplg_solve's grid; more components are strided over
CAND_CAP = 7                 # FPLG_CAND_CAP: numpy's sum is a plain loop below 8 elements
COMP_CAP = 4096              # FPLG_COMP_CAP: the largest component cap a caller may ask for
MAX_MOVES = 4096             # FPLG_MAX_MOVES: ... and the largest bound on a point's moves
MAX_POINTS = 2 ** 31 - 2     # n + 1 flags are compacted


class FplMergeError(RuntimeError):
    pass


_vp, _i64, _f64 = C.c_void_p, C.c_int64, C.c_double
_out = C.POINTER(_i64)

# name -> (restype, argtypes); every symbol include/fplmerge.h declares
SIGNATURES = {
    'fplg_last_error': (C.c_char_p, []),
    'fplg_abi_version': (C.c_int, []),
    'fplg_rows_count': (C.c_int, [_vp, _i64, _f64, _vp, _vp, _i64, _vp, _vp, _vp, _out, _vp]),
    'fplg_rows_fill': (C.c_int, [_vp, _i64, _f64, _vp, _vp, _i64, _vp, _i64, _vp, _vp]),
    'fplg_labels': (C.c_int, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _out, _vp]),
    'fplg_group_keys': (C.c_int, [_vp, _vp, _vp, _i64, _vp, _vp]),
    'fplg_boundaries': (C.c_int, [_vp, _i64, _vp, _vp]),
    'fplg_scratch_bytes': (C.c_int, [_i64, _out]),
    'fplg_flags_count': (C.c_int, [_vp, _i64, _vp, _i64, _out, _vp]),
    'fplg_flags_fill': (C.c_int, [_vp, _i64, _vp, _i64, _i64, _vp, _vp]),
    'fplg_solve': (C.c_int, [_vp, _vp, _vp, _vp, _i64, _f64, C.POINTER(_f64), _f64, _out,
                             _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64,
                             _vp, _vp, _vp, _vp, _vp]),
}

_side = SideLibrary('merge', FplMergeError, SIGNATURES, ABI_VERSION,
                    "the device merge has no host fallback; use solver='host' for the host loop")
LIB_PATH, load_library, check = _side.path, _side.load, _side.check


def _p(address):
    return _vp(address or None)


def rows_count(locs_ptr, n, t, offsets_ptr, indices_ptr, entries, has_ptr, out_offsets_ptr,
               head_ptr, stream):
    """has_neighbor and the offsets of the filtered table; -> its entry count.  Waits for
    `stream` (a raw hipStream_t)."""
    lib = load_library()
    total = _i64(-1)
    check(lib, lib.fplg_rows_count(_p(locs_ptr), int(n), float(t), _p(offsets_ptr), _p(indices_ptr),
                                   int(entries), _p(has_ptr), _p(out_offsets_ptr), _p(head_ptr),
                                   C.byref(total), _vp(stream)))
    return total.value


def rows_fill(locs_ptr, n, t, offsets_ptr, indices_ptr, entries, out_offsets_ptr, capacity,
              out_indices_ptr, stream):
    """the columns of the filtered table the count sized; asynchronous"""
    lib = load_library()
    check(lib, lib.fplg_rows_fill(_p(locs_ptr), int(n), float(t), _p(offsets_ptr), _p(indices_ptr),
                                  int(entries), _p(out_offsets_ptr), int(capacity),
                                  _p(out_indices_ptr), _vp(stream)))


def labels(offsets_ptr, indices_ptr, n, entries, label_ptr, other_ptr, changed_ptr, max_sweeps,
           stream):
    """the component label of every point (the component's smallest index), in both buffers;
    -> the sweeps it took.  Waits for `stream`."""
    lib = load_library()
    sweeps = _i64(0)
    check(lib, lib.fplg_labels(_p(offsets_ptr), _p(indices_ptr), int(n), int(entries), _p(label_ptr),
                               _p(other_ptr), _p(changed_ptr), int(max_sweeps), C.byref(sweeps),
                               _vp(stream)))
    return sweeps.value


def group_keys(offsets_ptr, label_ptr, rank_ptr, n, keys_ptr, stream):
    """keys = label * 2^32 + rank, idle points last; asynchronous"""
    lib = load_library()
    check(lib, lib.fplg_group_keys(_p(offsets_ptr), _p(label_ptr), _p(rank_ptr), int(n),
                                   _p(keys_ptr), _vp(stream)))


def boundaries(sorted_keys_ptr, n, flags_ptr, stream):
    """the n + 1 flags that mark the components' starts and the last one's end; asynchronous"""
    lib = load_library()
    check(lib, lib.fplg_boundaries(_p(sorted_keys_ptr), int(n), _p(flags_ptr), _vp(stream)))


def scratch_bytes(n):
    """bytes of device scratch flags_count / flags_fill ask for a list of n flags"""
    lib = load_library()
    out = _i64(0)
    check(lib, lib.fplg_scratch_bytes(int(n), C.byref(out)))
    return out.value


def flags_count(flags_ptr, n, scratch_ptr, n_scratch, stream):
    """the number of non-zero flags; the scanned block offsets stay in the scratch buffer.
    Waits for `stream`."""
    lib = load_library()
    total = _i64(-1)
    check(lib, lib.fplg_flags_count(_p(flags_ptr), int(n), _p(scratch_ptr), int(n_scratch),
                                    C.byref(total), _vp(stream)))
    return total.value


def flags_fill(flags_ptr, n, scratch_ptr, n_scratch, capacity, index_out_ptr, stream):
    """the indices of the non-zero flags, ascending; asynchronous"""
    lib = load_library()
    check(lib, lib.fplg_flags_fill(_p(flags_ptr), int(n), _p(scratch_ptr), int(n_scratch),
                                   int(capacity), _p(index_out_ptr), _vp(stream)))


def solve(locs_ptr, conf_ptr, labels_ptr, comp_ptr, n, t, origin, cell, dims, keys_ptr, order_ptr,
          f_offsets_ptr, f_indices_ptr, f_entries, members_ptr, starts_ptr, n_comp, cand_cap,
          comp_cap, max_moves, rm_ptr, mv_ptr, mv_loc_ptr, flagged_ptr, stream):
    """the merge loop, a lane per component; rm, mv, mv_loc and flagged are cleared by the
    caller; asynchronous"""
    lib = load_library()
    check(lib, lib.fplg_solve(_p(locs_ptr), _p(conf_ptr), _p(labels_ptr), _p(comp_ptr), int(n),
                              float(t), (_f64 * 3)(*(float(v) for v in origin)), float(cell),
                              (_i64 * 3)(*(int(v) for v in dims)), _p(keys_ptr), _p(order_ptr),
                              _p(f_offsets_ptr), _p(f_indices_ptr), int(f_entries),
                              _p(members_ptr), _p(starts_ptr), int(n_comp), int(cand_cap),
                              int(comp_cap), int(max_moves), _p(rm_ptr), _p(mv_ptr),
                              _p(mv_loc_ptr), _p(flagged_ptr), _vp(stream)))
