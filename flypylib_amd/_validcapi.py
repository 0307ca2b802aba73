"""ctypes binding of libfplval.so (include/fplval.h): the loss and metric sums of a batch of
predictions against its labels (`loss_sums`), the reduction of held-out validation.

A missing library is an error (`FplValidError`), never a silent fallback to a host reduction.
"""
import ctypes as C

from ._sidelib import SideLibrary

ABI_VERSION = 1
# the launch of fplv_loss_sums (fplval.h): threads per block, elements per thread and grid
# stride, the grid cap, the doubles of `sums`, the least scratch
BLOCK, ELEMS_PER_THREAD, MAX_BLOCKS, N_SUMS = 256, 4, 1024, 8
SCRATCH_BYTES = MAX_BLOCKS * 7 * 8


class FplValidError(RuntimeError):
    pass


_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64

# name -> (restype, argtypes); every symbol include/fplval.h declares
SIGNATURES = {
    'fplv_last_error': (C.c_char_p, []),
    'fplv_abi_version': (C.c_int, []),
    'fplv_loss_sums': (C.c_int, [_vp, _vp, _i64, _i32, _i32, _vp, _vp, _i64, _vp]),
}

_side = SideLibrary('valid', FplValidError, SIGNATURES, ABI_VERSION,
                    'validation has no host fallback; train without validation_data instead')
LIB_PATH, load_library, check = _side.path, _side.load, _side.check


def loss_sums(pred, labels, n, loss_kind, accumulate, sums, scratch, scratch_bytes, stream=None):
    """fplv_loss_sums on raw device addresses (ints) or anything `_capi._ptr` takes; stream-ordered,
    returns without waiting"""
    from . import _capi
    lib = load_library()
    check(lib, lib.fplv_loss_sums(_capi._ptr(pred), _capi._ptr(labels), int(n), int(loss_kind),
                                  int(bool(accumulate)), _capi._ptr(sums), _capi._ptr(scratch),
                                  int(scratch_bytes), _vp(stream or None)))
