"""ctypes binding of libfplplan.so (include/fplplan.h): the brick tables of the device
write_labels_mask planned on the device.

A missing library is an error (`FplPlanError`), never a silent fallback to the host planner.
The functions here take raw device addresses and a raw hipStream_t; flypylib_amd/labels.py
puts torch tensors around them.
"""
import ctypes as C

from ._sidelib import SideLibrary

ABI_VERSION = 1
BRICK = (4, 8, 128)          # FPLP_BRICK_Z, FPLP_BRICK_Y, FPLP_BRICK_X
MAX_RADIUS = 1024            # FPLP_MAX_RADIUS


class FplPlanError(RuntimeError):
    pass


_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64
_dims = C.POINTER(_i64)

# name -> (restype, argtypes); every symbol include/fplplan.h declares
SIGNATURES = {
    'fplp_last_error': (C.c_char_p, []),
    'fplp_abi_version': (C.c_int, []),
    'fplp_scratch_bytes': (C.c_int, [_i64, _i64, _i64, C.POINTER(_i64)]),
    'fplp_plan_bricks': (C.c_int, [_vp, _i64, _dims, _i32, _vp, _vp, _i64, _vp, _i64, _vp]),
}

_side = SideLibrary('plan', FplPlanError, SIGNATURES, ABI_VERSION,
                    "planner='device' has no host fallback; use planner='host' for the numpy "
                    'planner')
LIB_PATH, load_library, check = _side.path, _side.load, _side.check


def scratch_bytes(n_tbars, n_bricks, n_index):
    """bytes of device scratch plan_bricks asks for"""
    lib = load_library()
    out = _i64(0)
    check(lib, lib.fplp_scratch_bytes(int(n_tbars), int(n_bricks), int(n_index), C.byref(out)))
    return out.value


def plan_bricks(tbars_ptr, n_tbars, dims, half, offsets_ptr, index_ptr, n_index, scratch_ptr,
                scratch_size, stream):
    """the launches on `stream` (a raw hipStream_t); asynchronous.  The first int32 of the
    scratch is the status word, to be read after the stream is synchronised."""
    lib = load_library()
    check(lib, lib.fplp_plan_bricks(_vp(tbars_ptr or None), int(n_tbars),
                                    (_i64 * 3)(*[int(d) for d in dims]), int(half),
                                    _vp(offsets_ptr or None), _vp(index_ptr or None),
                                    int(n_index), _vp(scratch_ptr or None), int(scratch_size),
                                    _vp(stream)))
