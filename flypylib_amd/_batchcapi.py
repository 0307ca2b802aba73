"""ctypes binding of libfplbatch.so (include/fplbatch.h): the device batch gather.

A missing library is an error (`FplBatchError`), never a silent host fallback.
"""
import ctypes as C

import numpy as np

from ._sidelib import SideLibrary

ABI_VERSION = 1
U8, F32 = 0, 1
LABELS_CENTRE, LABELS_6 = 0, 1
FLIP_AXIS0, FLIP_AXIS1, FLIP_AXIS2 = 1, 2, 4

# struct fplb_volume / fplb_record (checked against the library by load_library)
VOLUME = np.dtype({'names': ['image', 'labels', 'd0', 'd1', 'd2', 'dtype'],
                   'formats': ['<u8', '<u8', '<i4', '<i4', '<i4', '<i4'],
                   'offsets': [0, 8, 16, 20, 24, 28], 'itemsize': 32})
RECORD = np.dtype({'names': ['vol', 'z', 'y', 'x', 'rot', 'flips', 'mul', 'add'],
                   'formats': ['<i4', '<i4', '<i4', '<i4', 'u1', 'u1', '<f8', '<f8'],
                   'offsets': [0, 4, 8, 12, 16, 17, 24, 32], 'itemsize': 40})


class FplBatchError(RuntimeError):
    pass


_vp, _i32 = C.c_void_p, C.c_int32

# name -> (restype, argtypes); every symbol include/fplbatch.h declares
SIGNATURES = {
    'fplb_last_error': (C.c_char_p, []),
    'fplb_abi_version': (C.c_int, []),
    'fplb_struct_sizes': (C.c_int, [C.POINTER(_i32), C.POINTER(_i32)]),
    'fplb_gather': (C.c_int, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                              _vp, _vp, _vp]),
}


def _check_structs(lib):
    """struct fplb_volume / fplb_record are the library's size"""
    vb, rb = _i32(), _i32()
    _side.check(lib, lib.fplb_struct_sizes(C.byref(vb), C.byref(rb)))
    if (vb.value, rb.value) != (VOLUME.itemsize, RECORD.itemsize):
        raise FplBatchError('libfplbatch.so structs are %d / %d bytes, the binding\'s %d / %d'
                            % (vb.value, rb.value, VOLUME.itemsize, RECORD.itemsize))


_side = SideLibrary('batch', FplBatchError, SIGNATURES, ABI_VERSION,
                    'device batch generators have no host fallback; use device=None for the host '
                    'generators', _check_structs)
LIB_PATH, load_library, check = _side.path, _side.load, _side.check


def gather(vols_ptr, n_vols, recs_ptr, batch, context, src_dtype, noise, label_mode,
           data_ptr, labels_ptr, stream):
    """one launch of the gather kernel on `stream` (a raw hipStream_t); asynchronous"""
    lib = load_library()
    check(lib, lib.fplb_gather(_vp(vols_ptr), n_vols, _vp(recs_ptr), batch, context[0],
                               context[1], context[2], src_dtype, 1 if noise else 0,
                               label_mode, _vp(data_ptr), _vp(labels_ptr), _vp(stream)))
