"""ctypes binding of libfplseg.so (include/fplseg.h): reads of a label volume resident in device
memory - the labels of a point list (`gather_labels`) and the padded u64 copy of a box
(`pad_box`, the kernel fpl_v2o_set_seg runs inside a context).

A missing library is an error (`FplSegError`), never a silent fallback to host indexing.
"""
import ctypes as C

import numpy as np

from ._sidelib import SideLibrary

ABI_VERSION = 1
MEM_HOST, MEM_DEVICE = 0, 1


class FplSegError(RuntimeError):
    pass


_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64
_pi64 = C.POINTER(_i64)

# name -> (restype, argtypes); every symbol include/fplseg.h declares
SIGNATURES = {
    'fpls_last_error': (C.c_char_p, []),
    'fpls_abi_version': (C.c_int, []),
    'fpls_pad_box': (C.c_int, [_vp, _i32, _pi64, _pi64, _pi64, _i32, _vp, _vp]),
    'fpls_gather_labels': (C.c_int, [_vp, _i32, _pi64, _vp, C.c_int, _i64, _vp, C.c_int, _vp]),
}

_side = SideLibrary('seg', FplSegError, SIGNATURES, ABI_VERSION,
                    'resident labels have no host fallback; pass a host label array instead')
LIB_PATH, load_library, check = _side.path, _side.load, _side.check


def _arr3(vals):
    return (_i64 * 3)(*[int(v) for v in vals])


def pad_box(vol, origin, dims, r, dst, stream=None):
    """`dst` (device, uint64, dims + 2r) := the box `origin` .. `origin + dims` (z, y, x) of the
    resident label volume `vol` in a zero shell of r, zeros outside the volume"""
    from . import _capi
    nbytes, extent = _capi.resident_labels(vol, 'pad_box')
    if _capi._mem_of(dst) != MEM_DEVICE:
        raise ValueError('pad_box: dst must be device memory')
    lib = load_library()
    check(lib, lib.fpls_pad_box(_capi._ptr(vol), nbytes, _arr3(extent), _arr3(origin), _arr3(dims),
                                int(r), _capi._ptr(dst), _vp(stream or None)))
    return dst


def gather_labels(vol, zyx, out=None, stream=None):
    """uint64 labels of the resident label volume `vol` at the (n, 3) int64 (z, y, x) points
    `zyx` (host array or device tensor); a point outside the volume raises"""
    from . import _capi
    nbytes, extent = _capi.resident_labels(vol, 'gather_labels')
    if isinstance(zyx, np.ndarray) or not hasattr(zyx, 'data_ptr'):
        zyx = np.ascontiguousarray(zyx, np.int64).reshape(-1, 3)
    elif 'int64' not in str(zyx.dtype) or not zyx.is_contiguous() or zyx.shape[-1] != 3:
        raise TypeError('gather_labels: device points must be a contiguous (n, 3) int64 tensor')
    n = int(np.prod(zyx.shape)) // 3
    if out is None:
        out = np.empty(n, np.uint64)
    lib = load_library()
    check(lib, lib.fpls_gather_labels(_capi._ptr(vol), nbytes, _arr3(extent), _capi._ptr(zyx),
                                      _capi._mem_of(zyx), n, _capi._ptr(out), _capi._mem_of(out),
                                      _vp(stream or None)))
    return out
