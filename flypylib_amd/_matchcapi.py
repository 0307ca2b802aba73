"""ctypes binding of libfplmatch.so (include/fplmatch.h): the table of (prediction,
ground-truth) pairs closer than the match threshold, for the sparse obj_pr / obj_pr_curve.

A missing library is an error (`FplMatchError`), never a silent fallback to the host table.
The functions here take raw device addresses and a raw hipStream_t; flypylib_amd/match.py puts
torch tensors around them.
"""
import ctypes as C

from ._sidelib import SideLibrary

ABI_VERSION = 1
BLOCK = 256                  # FPLE_BLOCK: predictions per block
TILE = 256                   # FPLE_TILE: ground-truth points per LDS tile
MAX_SEGMENTS = 64            # FPLE_MAX_SEGMENTS
TARGET_BLOCKS = 1024         # FPLE_TARGET_BLOCKS
SCAN_THREADS = 1024          # FPLE_SCAN_THREADS
MAX_POINTS = 2 ** 31 - 1     # of either kind, and the rows of a table


class FplMatchError(RuntimeError):
    pass


_vp, _i64, _f64 = C.c_void_p, C.c_int64, C.c_double

# name -> (restype, argtypes); every symbol include/fplmatch.h declares
SIGNATURES = {
    'fple_last_error': (C.c_char_p, []),
    'fple_abi_version': (C.c_int, []),
    'fple_scratch_bytes': (C.c_int, [_i64, _i64, C.POINTER(_i64)]),
    'fple_pairs_count': (C.c_int, [_vp, _i64, _vp, _i64, _f64, _vp, _i64, C.POINTER(_i64), _vp]),
    'fple_pairs_fill': (C.c_int, [_vp, _i64, _vp, _i64, _f64, _vp, _i64, _i64, _vp, _vp, _vp]),
}

_side = SideLibrary('match', FplMatchError, SIGNATURES, ABI_VERSION,
                    "device matching has no host fallback; use match='sparse' for the numpy table")
LIB_PATH, load_library, check = _side.path, _side.load, _side.check


def segments(n_pred, n_gt):
    """G of include/fplmatch.h: the grid rows the ground-truth range is cut into"""
    blocks, tiles = -(-int(n_pred) // BLOCK), -(-int(n_gt) // TILE)
    want = min(tiles, -(-TARGET_BLOCKS // blocks))
    g = 1
    while g < want and g < MAX_SEGMENTS:
        g <<= 1
    return g


def segment_len(n_pred, n_gt):
    """ground-truth points per segment: whole tiles; the last segment may be short or empty"""
    tiles = -(-int(n_gt) // TILE)
    return -(-tiles // segments(n_pred, n_gt)) * TILE


def scratch_bytes(n_pred, n_gt):
    """bytes of device scratch pairs_count / pairs_fill ask for"""
    lib = load_library()
    out = _i64(0)
    check(lib, lib.fple_scratch_bytes(int(n_pred), int(n_gt), C.byref(out)))
    return out.value


def pairs_count(pred_ptr, n_pred, gt_ptr, n_gt, t2, scratch_ptr, n_scratch, stream):
    """the number of rows; the scanned offsets stay in the scratch buffer.  Waits for `stream`
    (a raw hipStream_t)."""
    lib = load_library()
    total = _i64(-1)
    check(lib, lib.fple_pairs_count(_vp(pred_ptr or None), int(n_pred), _vp(gt_ptr or None),
                                    int(n_gt), float(t2), _vp(scratch_ptr or None),
                                    int(n_scratch), C.byref(total), _vp(stream)))
    return total.value


def pairs_fill(pred_ptr, n_pred, gt_ptr, n_gt, t2, scratch_ptr, n_scratch, capacity, i_ptr, j_ptr,
               stream):
    """write the rows the count found (same arguments, same scratch); asynchronous"""
    lib = load_library()
    check(lib, lib.fple_pairs_fill(_vp(pred_ptr or None), int(n_pred), _vp(gt_ptr or None),
                                   int(n_gt), float(t2), _vp(scratch_ptr or None), int(n_scratch),
                                   int(capacity), _vp(i_ptr or None), _vp(j_ptr or None),
                                   _vp(stream)))
