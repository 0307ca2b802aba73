"""ctypes binding of libfpllabels.so (include/fpllabels.h): the labels and mask of
write_labels_mask rendered on the device.

A missing library is an error (`FplLabelsError`), never a silent host fallback.  The function
here takes raw device addresses and a raw hipStream_t; flypylib_amd/labels.py puts torch
tensors around it.
"""
import ctypes as C

from ._sidelib import SideLibrary

ABI_VERSION = 1
BRICK = (4, 8, 128)          # FPLL_BRICK_Z, FPLL_BRICK_Y, FPLL_BRICK_X
MAX_RADIUS = 1024            # FPLL_MAX_RADIUS
MAX_VOXELS = 2 ** 31 - 1


class FplLabelsError(RuntimeError):
    pass


_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64
_dims = C.POINTER(_i64)

# name -> (restype, argtypes); every symbol include/fpllabels.h declares
SIGNATURES = {
    'fpll_last_error': (C.c_char_p, []),
    'fpll_abi_version': (C.c_int, []),
    'fpll_labels_mask': (C.c_int, [_vp, _vp, _i64, _vp, _vp, _i64, _dims, _i32, _i32, _i32, _vp,
                                   _vp, _vp]),
}

_side = SideLibrary('labels', FplLabelsError, SIGNATURES, ABI_VERSION,
                    'device write_labels_mask has no host fallback; use device=None for the host '
                    'path')
LIB_PATH, load_library, check = _side.path, _side.load, _side.check


def labels_mask(roi_ptr, tbars_ptr, n_tbars, offsets_ptr, index_ptr, n_index, dims, radius_use,
                radius_ign, buffer_size, labels_ptr, mask_ptr, stream):
    """one launch on `stream` (a raw hipStream_t); asynchronous"""
    lib = load_library()
    check(lib, lib.fpll_labels_mask(_vp(roi_ptr or None), _vp(tbars_ptr or None), int(n_tbars),
                                    _vp(offsets_ptr or None), _vp(index_ptr or None),
                                    int(n_index), (_i64 * 3)(*[int(d) for d in dims]),
                                    int(radius_use), int(radius_ign), int(buffer_size),
                                    _vp(labels_ptr or None), _vp(mask_ptr or None), _vp(stream)))
