"""ctypes binding of libfplclahe.so (include/fplclahe.h): per-slice CLAHE of a resident volume
(`clahe`), and the scratch it asks for (`scratch_bytes`).

A missing library is an error (`FplClaheError`), never a silent fallback to the host executor.
"""
import ctypes as C

from ._sidelib import SideLibrary

ABI_VERSION = 1
# fplclahe.h: threads per block, the most bins, the gray levels, the head of the scratch
BLOCK, MAX_NBINS, NR_OF_GRAY, STATUS_BYTES = 256, 256, 16384, 16
STAGE_RANGE, STAGE_MAPS, STAGE_APPLY, STAGE_FINISH, STAGE_ALL = 1, 2, 4, 8, 15
U8, F32 = 0, 1


class FplClaheError(RuntimeError):
    pass


_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64

# name -> (restype, argtypes); every symbol include/fplclahe.h declares
SIGNATURES = {
    'fplc_last_error': (C.c_char_p, []),
    'fplc_abi_version': (C.c_int, []),
    'fplc_scratch_bytes': (C.c_int, [_i64, _i64, _i64, _i64, _i64, _i32, C.POINTER(_i64)]),
    'fplc_clahe': (C.c_int, [_vp, _i32, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _i32, _vp, _vp,
                             _i64, _i32, _vp]),
}

_side = SideLibrary('clahe', FplClaheError, SIGNATURES, ABI_VERSION,
                    'clahe(device=) has no host fallback; use device=None for the numpy executor')
LIB_PATH, load_library, check = _side.path, _side.load, _side.check


def scratch_bytes(Z, Y, X, ky, kx, nbins):
    """bytes of device scratch `clahe` asks for"""
    lib = load_library()
    out = _i64(0)
    check(lib, lib.fplc_scratch_bytes(int(Z), int(Y), int(X), int(ky), int(kx), int(nbins),
                                      C.byref(out)))
    return out.value


def clahe(src, is_u8, dims, k, clim, nbins, zero_mean, out, scratch, scratch_size, stages=STAGE_ALL,
          stream=None):
    """fplc_clahe on raw device addresses (ints) or anything `_capi._ptr` takes; stream-ordered,
    returns without waiting"""
    from . import _capi
    lib = load_library()
    check(lib, lib.fplc_clahe(_capi._ptr(src), U8 if is_u8 else F32, int(dims[0]), int(dims[1]),
                              int(dims[2]), int(k[0]), int(k[1]), int(clim), int(nbins),
                              int(bool(zero_mean)), _capi._ptr(out), _capi._ptr(scratch),
                              int(scratch_size), int(stages), _vp(stream or None)))
