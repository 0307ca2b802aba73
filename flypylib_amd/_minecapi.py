"""ctypes binding of libfplmine.so (include/fplmine.h): the device voxel loss and the ordered
candidate compaction of hard-example mining.

A missing library is an error (`FplMineError`), never a silent host fallback.  The functions
here take raw device addresses and a raw hipStream_t; flypylib_amd/mine.py puts torch tensors
around them.
"""
import ctypes as C

from ._sidelib import SideLibrary

ABI_VERSION = 1
CHUNK = 4096                 # FPLM_CHUNK
MAX_VOXELS = 2 ** 31 - 1


class FplMineError(RuntimeError):
    pass


_vp, _i32, _i64, _f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
_dims, _triple = C.POINTER(_i64), C.POINTER(_i32)

# name -> (restype, argtypes); every symbol include/fplmine.h declares
SIGNATURES = {
    'fplm_last_error': (C.c_char_p, []),
    'fplm_abi_version': (C.c_int, []),
    'fplm_voxel_loss': (C.c_int, [_vp, _vp, _vp, _dims, _triple, _i32, _f64, _f64, _i32, _f64,
                                  _f64, _vp, _vp]),
    'fplm_candidates_count': (C.c_int, [_vp, _vp, _vp, _dims, _triple, _i32, _vp, _i64,
                                        C.POINTER(_i64), _vp]),
    'fplm_candidates_fill': (C.c_int, [_vp, _vp, _vp, _dims, _triple, _i32, _vp, _i64, _i64,
                                       _vp, _vp, _vp, _vp, _vp]),
}

_side = SideLibrary('mine', FplMineError, SIGNATURES, ABI_VERSION,
                    'device mining has no host fallback; use device=None for the host path')
LIB_PATH, load_library, check = _side.path, _side.load, _side.check


def scratch_bytes(n_voxels):
    """FPLM_SCRATCH_BYTES: one uint32 per chunk and the total"""
    return ((int(n_voxels) + CHUNK - 1) // CHUNK + 1) * 4


def _i64x3(v):
    return (_i64 * 3)(*[int(a) for a in v])


def _i32x3(v):
    return (_i32 * 3)(*[int(a) for a in v])


def _pair(bounds):
    if bounds is None:
        return 0, 0.0, 0.0
    return 1, float(bounds[0]), float(bounds[1])


def voxel_loss(pred_ptr, labels_ptr, mask_ptr, dims, edge, l0_thresh, l1_thresh, loss_ptr,
               stream):
    """one launch on `stream` (a raw hipStream_t); asynchronous"""
    lib = load_library()
    check(lib, lib.fplm_voxel_loss(_vp(pred_ptr), _vp(labels_ptr), _vp(mask_ptr), _i64x3(dims),
                                   _i32x3(edge), *_pair(l0_thresh), *_pair(l1_thresh),
                                   _vp(loss_ptr), _vp(stream)))


def candidates_count(labels_ptr, mask_ptr, weights_ptr, dims, half, cc, scratch_ptr, n_scratch,
                     stream):
    """the number of candidate rows; the scanned counts stay in the scratch buffer.  Waits
    for `stream`."""
    lib = load_library()
    total = _i64(-1)
    check(lib, lib.fplm_candidates_count(_vp(labels_ptr), _vp(mask_ptr), _vp(weights_ptr or None),
                                         _i64x3(dims), _i32x3(half), int(cc), _vp(scratch_ptr),
                                         int(n_scratch), C.byref(total), _vp(stream)))
    return total.value


def candidates_fill(labels_ptr, mask_ptr, weights_ptr, dims, half, cc, scratch_ptr, n_scratch,
                    capacity, z_ptr, y_ptr, x_ptr, w_ptr, stream):
    """write the rows the count found (same arguments, same scratch); asynchronous"""
    lib = load_library()
    check(lib, lib.fplm_candidates_fill(_vp(labels_ptr), _vp(mask_ptr), _vp(weights_ptr or None),
                                        _i64x3(dims), _i32x3(half), int(cc), _vp(scratch_ptr),
                                        int(n_scratch), int(capacity), _vp(z_ptr), _vp(y_ptr),
                                        _vp(x_ptr), _vp(w_ptr or None), _vp(stream)))
