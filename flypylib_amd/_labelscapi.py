"""ctypes binding of libfpllabels.so (include/fpllabels.h): the labels and mask of
write_labels_mask rendered on the device.

A missing library is an error (`FplLabelsError`), never a silent host fallback.  The function
here takes raw device addresses and a raw hipStream_t; flypylib_amd/labels.py puts torch
tensors around it.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lib', 'libfpllabels.so')

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

_lib = None


def load_library(path=None):
    """dlopen libfpllabels.so and bind every declared symbol (no GPU needed)"""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise FplLabelsError(
            'libfpllabels.so not found at %s - build it with `python -m flypylib_amd.csrc.build` '
            '(device write_labels_mask has no host fallback; use device=None for the host path)'
            % path)
    # one HIP runtime per process, shared with torch and libfplhip.so: the same preload
    # rule as _capi.load_library
    if not os.environ.get('FPL_NO_TORCH_PRELOAD'):
        try:
            import torch  # noqa: F401
        except Exception:       # noqa: BLE001
            pass
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.fpll_abi_version() != ABI_VERSION:
        raise FplLabelsError('libfpllabels.so ABI %d, binding expects %d'
                             % (lib.fpll_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(lib, rc):
    if rc != 0:
        raise FplLabelsError((lib.fpll_last_error() or b'').decode() or 'rc %d' % rc)


def labels_mask(roi_ptr, tbars_ptr, n_tbars, offsets_ptr, index_ptr, n_index, dims, radius_use,
                radius_ign, buffer_size, labels_ptr, mask_ptr, stream):
    """one launch on `stream` (a raw hipStream_t); asynchronous"""
    lib = load_library()
    check(lib, lib.fpll_labels_mask(_vp(roi_ptr or None), _vp(tbars_ptr or None), int(n_tbars),
                                    _vp(offsets_ptr or None), _vp(index_ptr or None),
                                    int(n_index), (_i64 * 3)(*[int(d) for d in dims]),
                                    int(radius_use), int(radius_ign), int(buffer_size),
                                    _vp(labels_ptr or None), _vp(mask_ptr or None), _vp(stream)))
