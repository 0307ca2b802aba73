"""ctypes binding of libfplnear.so (include/fplnear.h): the table of the close pairs within
one point set, for the sparse fplsynapses.rm_tbar_multi_pred.

A missing library is an error (`FplNearError`), never a silent fallback to the host table.
The functions here take raw device addresses and a raw hipStream_t; flypylib_amd/near.py puts
torch tensors around them.
"""
import ctypes as C

from ._sidelib import SideLibrary

ABI_VERSION = 1
BLOCK = 256                  # FPLN_BLOCK: points per block
SCAN_THREADS = 1024          # FPLN_SCAN_THREADS
MAX_AXIS_BITS = 28           # FPLN_MAX_AXIS_BITS: an axis has at most 2^28 cells
MAX_POINTS = 2 ** 31 - 1     # and the entries of a table


class FplNearError(RuntimeError):
    pass


_vp, _i64, _f64 = C.c_void_p, C.c_int64, C.c_double
_origin, _dims = C.POINTER(_f64), C.POINTER(_i64)
_grid = [_origin, _f64, _dims]

# name -> (restype, argtypes); every symbol include/fplnear.h declares
SIGNATURES = {
    'fpln_last_error': (C.c_char_p, []),
    'fpln_abi_version': (C.c_int, []),
    'fpln_scratch_bytes': (C.c_int, [_i64, C.POINTER(_i64)]),
    'fpln_cell_keys': (C.c_int, [_vp, _i64] + _grid + [_vp, _vp]),
    'fpln_pairs_count': (C.c_int, [_vp, _i64, _f64] + _grid + [_vp, _vp, _vp, _i64,
                                                                C.POINTER(_i64), _vp]),
    'fpln_pairs_fill': (C.c_int, [_vp, _i64, _f64] + _grid + [_vp, _vp, _vp, _i64, _i64, _vp, _vp]),
}

_side = SideLibrary('near', FplNearError, SIGNATURES, ABI_VERSION,
                    "the device table has no host fallback; use method='sparse' without device= "
                    "for the numpy table")
LIB_PATH, load_library, check = _side.path, _side.load, _side.check


def _grid_args(origin, cell, dims):
    return ((_f64 * 3)(*(float(v) for v in origin)), float(cell),
            (_i64 * 3)(*(int(v) for v in dims)))


def scratch_bytes(n):
    """bytes of device scratch pairs_count / pairs_fill ask for"""
    lib = load_library()
    out = _i64(0)
    check(lib, lib.fpln_scratch_bytes(int(n), C.byref(out)))
    return out.value


def cell_keys(locs_ptr, n, origin, cell, dims, keys_ptr, stream):
    """the int64 cell key of every point, original order; asynchronous"""
    lib = load_library()
    check(lib, lib.fpln_cell_keys(_vp(locs_ptr or None), int(n), *_grid_args(origin, cell, dims),
                                  _vp(keys_ptr or None), _vp(stream)))


def pairs_count(locs_ptr, n, t2, origin, cell, dims, keys_ptr, order_ptr, scratch_ptr, n_scratch,
                stream):
    """the number of table entries; the row offsets stay in the scratch buffer (uint32, n + 1
    of them from byte 16).  Waits for `stream` (a raw hipStream_t)."""
    lib = load_library()
    total = _i64(-1)
    check(lib, lib.fpln_pairs_count(_vp(locs_ptr or None), int(n), float(t2),
                                    *_grid_args(origin, cell, dims), _vp(keys_ptr or None),
                                    _vp(order_ptr or None), _vp(scratch_ptr or None),
                                    int(n_scratch), C.byref(total), _vp(stream)))
    return total.value


def pairs_fill(locs_ptr, n, t2, origin, cell, dims, keys_ptr, order_ptr, scratch_ptr, n_scratch,
               capacity, indices_ptr, stream):
    """write the columns the count found (same arguments, same scratch); asynchronous"""
    lib = load_library()
    check(lib, lib.fpln_pairs_fill(_vp(locs_ptr or None), int(n), float(t2),
                                   *_grid_args(origin, cell, dims), _vp(keys_ptr or None),
                                   _vp(order_ptr or None), _vp(scratch_ptr or None),
                                   int(n_scratch), int(capacity), _vp(indices_ptr or None),
                                   _vp(stream)))
