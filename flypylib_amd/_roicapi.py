"""ctypes binding of libfplroi.so (include/fplroi.h): the ROI's box mask (`mask_box`), point
queries (`ptquery`) and voxel counts (`box_counts`) on the three resident tables of
`roi.BlockRoi.device_tables`, and the cut-and-normalise of a training cube (`cut_normalize_u8`).

A missing library is an error (`FplRoiError`), never a silent fallback to the numpy path.
"""
import ctypes as C

from ._sidelib import SideLibrary

ABI_VERSION = 1
# fplroi.h: threads per block, the most workgroups of mask_box, the limits of the arguments
BLOCK, MAX_GRID = 256, 4096
BLOCK_SIZE_BITS, SIDE_BITS, COORD_BITS = 20, 21, 40


class FplRoiError(RuntimeError):
    pass


_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64
_pi64 = C.POINTER(_i64)
_tables = [_vp, _vp, _vp, _i64, _i64, _i32]

# name -> (restype, argtypes); every symbol include/fplroi.h declares
SIGNATURES = {
    'fplr_last_error': (C.c_char_p, []),
    'fplr_abi_version': (C.c_int, []),
    'fplr_mask_box': (C.c_int, _tables + [_pi64, _pi64, _vp, _vp]),
    'fplr_ptquery': (C.c_int, _tables + [_vp, _i64, _vp, _vp]),
    'fplr_box_counts': (C.c_int, _tables + [_vp, _i64, _vp, _vp]),
    'fplr_cut_normalize_u8': (C.c_int, [_vp, _pi64, _pi64, _pi64, C.c_float, C.c_float, _vp, _vp]),
}

_side = SideLibrary('roi', FplRoiError, SIGNATURES, ABI_VERSION,
                    'BlockRoi(device=) and roi_to_substacks(device=) have no host fallback; use '
                    'device=None for the numpy path')
LIB_PATH, load_library, check = _side.path, _side.load, _side.check


def _arr3(vals):
    return (_i64 * 3)(*[int(v) for v in vals])


def _table_args(tables, n_rows, n_runs, block_size):
    from . import _capi
    keys, row_start, runs_x = tables
    return (_capi._ptr(keys), _capi._ptr(row_start), _capi._ptr(runs_x), int(n_rows), int(n_runs),
            int(block_size))


def mask_box(tables, n_rows, n_runs, block_size, origin, dims, out, stream=None):
    """fplr_mask_box; `tables`: (row_keys, row_start, runs_x) as raw device addresses (ints) or
    anything `_capi._ptr` takes; stream-ordered, returns without waiting"""
    from . import _capi
    lib = load_library()
    check(lib, lib.fplr_mask_box(*_table_args(tables, n_rows, n_runs, block_size), _arr3(origin),
                                 _arr3(dims), _capi._ptr(out), _vp(stream or None)))


def ptquery(tables, n_rows, n_runs, block_size, zyx, n, flags, stream=None):
    """fplr_ptquery on `n` resident int64 (z, y, x) points"""
    from . import _capi
    lib = load_library()
    check(lib, lib.fplr_ptquery(*_table_args(tables, n_rows, n_runs, block_size), _capi._ptr(zyx),
                                int(n), _capi._ptr(flags), _vp(stream or None)))


def box_counts(tables, n_rows, n_runs, block_size, boxes, n_boxes, counts, stream=None):
    """fplr_box_counts on `n_boxes` resident int64 (z, y, x, dz, dy, dx) rows"""
    from . import _capi
    lib = load_library()
    check(lib, lib.fplr_box_counts(*_table_args(tables, n_rows, n_runs, block_size),
                                   _capi._ptr(boxes), int(n_boxes), _capi._ptr(counts),
                                   _vp(stream or None)))


def cut_normalize_u8(vol, extent, origin, dims, mean, std, out, stream=None):
    """fplr_cut_normalize_u8: `mean` and `std` are rounded to float32 here, as numpy rounds them"""
    from . import _capi
    lib = load_library()
    check(lib, lib.fplr_cut_normalize_u8(_capi._ptr(vol), _arr3(extent), _arr3(origin), _arr3(dims),
                                         C.c_float(float(mean)), C.c_float(float(std)),
                                         _capi._ptr(out), _vp(stream or None)))
