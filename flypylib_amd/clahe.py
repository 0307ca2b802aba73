"""CLAHE preprocessing: per-slice contrast-limited adaptive histogram equalisation of a (Z, Y, X)
volume, what the reference's `fplutils.clahe` (`flypylib/fplutils.py:33-62`) does with
`skimage.exposure.equalize_adapthist` in a Python loop over z.

The specification is THIS PACKAGE'S OWN.  scikit-image is not a dependency, the reference pins no
version of it, its algorithm was rewritten in 0.17 and its intermediate dtypes moved between
releases, so "equal to skimage" is not a testable claim: parity with skimage is UNPINNED (DESIGN.md
section 17).  `clahe_numpy` follows the n-D algorithm of scikit-image >= 0.17
(`exposure/_adapthist.py`) and fixes every type and every order of operations:

  volume   mn, mx: float32 min and max of the whole volume; mx == mn raises ValueError (the
           reference divides by zero there).  Non-finite input raises as well.
  slice    a. s = (slice - mn) / (mx - mn): float32 subtract, float32 mx - mn, one correctly
              rounded float32 divide
           b. lo, hi = min(s), max(s); hi == lo: the output slice is 0.0 (skimage's result there
              depends on its version)
           c. g = rint((float64(s) - lo) / (hi - lo) * 16383.0): every operand float64, left to
              right, round-half-even; a uint16 in [0, 16383]
           d. tile (ky, kx) from kernel_size: a scalar gives (k, k), None gives max(s // 8, 1) per
              axis; ints >= 1
           e. pad before by k // 2, after by (k - s % k) % k + ceil(k / 2), np.pad(mode='reflect')
              (which reflects repeatedly where the pad exceeds s - 1)
           f. bin = g // (1 + 16384 // nbins)
           g. nt = P // k - 1 tiles per axis of the padded shape P; tile (i, j) covers padded rows
              [ky // 2 + i ky, ky // 2 + (i + 1) ky) and the columns likewise; its histogram is the
              bincount of its bins (int64, nbins entries)
           h. clip_histogram with clim = max(int(clip_limit ky kx), 1), or 16384 when
              clip_limit <= 0
           i. map_histogram: int(min(float64(cumsum) * (16383.0 / (ky kx)), 16383.0))
           j. bilinear interpolation between the maps of the four surrounding tiles (edge tiles
              repeated), in float64, the weight product rounded first, then the multiply, then the
              add, in the order (0,0), (0,1), (1,0), (1,1); no fused multiply-add; truncated to
              uint16
           k. the padding removed; rmin, rmax of the uint16 slice; rmax == rmin gives 0.0, else
              float32((float64(r) - rmin) / (rmax - rmin))
  zero_mean  out - float32(0.5)

`clahe_device` runs the same on a GPU through libfplclahe.so (include/fplclahe.h), bit for bit;
without torch, a GPU or the library it raises - there is no silent host fallback.
"""
import math

import numpy as np

NR_OF_GRAY = 16384
MAX_DEVICE_NBINS = 256


def reflect_index(i, s):
    """the index np.pad(mode='reflect') reads for position `i` of an axis of `s` elements, `i`
    counted from the first unpadded element (negative: the pad before, >= s: the pad after): the
    triangular wave of period 2 (s - 1), which is what numpy's repeated reflection amounts to.
    s == 1 reads element 0.  The kernels of libfplclahe.so use this closed form."""
    i, s = int(i), int(s)
    if s == 1:
        return 0
    period = 2 * (s - 1)
    m = i % period                   # Python's modulo: in [0, period)
    return m if m < s else period - m


def clip_histogram(h, clim, _trace=None):
    """step (h): the histogram `h` clipped at `clim`, the excess redistributed; a new int64 array"""
    h = np.array(h, np.int64)
    n, clim = h.size, int(clim)
    over = h > clim
    n_excess = int(h[over].sum()) - int(np.count_nonzero(over)) * clim
    h[over] = clim
    bin_incr = n_excess // n
    upper = clim - bin_incr
    low = h < upper
    n_excess -= int(np.count_nonzero(low)) * bin_incr
    h[low] += bin_incr
    mid = (h >= upper) & (h < clim)
    n_excess += int(h[mid].sum()) - int(np.count_nonzero(mid)) * clim
    h[mid] = clim
    passes = 0
    while n_excess > 0:
        passes += 1
        prev = n_excess
        for index in range(n):
            under = h < clim
            step = max(1, int(np.count_nonzero(under)) // n_excess)
            sel = np.zeros(n, bool)
            sel[index::step] = under[index::step]
            h[sel] += 1
            n_excess -= int(np.count_nonzero(sel))
            if n_excess <= 0:
                break
        if prev == n_excess:
            break
    if _trace is not None:
        _trace.append(passes)
    return h


def map_histogram(h, n_pixels):
    """step (i): the gray-level map of a clipped histogram, uint16 in [0, 16383]"""
    c = np.cumsum(np.asarray(h, np.int64), dtype=np.int64)
    scale = np.float64(NR_OF_GRAY - 1) / np.float64(int(n_pixels))
    m = np.minimum(c.astype(np.float64) * scale, np.float64(NR_OF_GRAY - 1))
    return m.astype(np.int64).astype(np.uint16)


def tile_size(kernel_size, shape):
    """(ky, kx) of step (d)"""
    if kernel_size is None:
        k = tuple(max(int(s) // 8, 1) for s in shape)
    elif np.size(kernel_size) == 1:
        v = int(np.asarray(kernel_size).reshape(-1)[0])
        k = (v, v)
    else:
        k = tuple(int(v) for v in np.asarray(kernel_size).reshape(-1))
    if len(k) != 2 or min(k) < 1:
        raise ValueError('clahe: kernel_size %r is not one or two integers >= 1' % (kernel_size,))
    return k


def clip_count(clip_limit, ky, kx):
    """clim of step (h)"""
    if clip_limit > 0:
        return max(int(clip_limit * ky * kx), 1)
    return NR_OF_GRAY


def pads(s, k):
    """(before, after) of step (e) for an axis of `s` elements and a tile of `k`"""
    return k // 2, (k - s % k) % k + (k + 1) // 2


def _as_volume(im, who):
    im = np.asarray(im)
    if im.ndim != 3 or im.size == 0:
        raise ValueError('%s: the volume must be 3-D (Z, Y, X) and not empty, got shape %s'
                         % (who, im.shape))
    return np.ascontiguousarray(im, np.float32)


def _slice_numpy(s, k, clim, nbins, passes):
    """steps (b) - (k) of one float32 slice `s`; a float32 slice"""
    (sy, sx), (ky, kx) = s.shape, k
    out = np.zeros(s.shape, np.float32)
    lo, hi = s.min(), s.max()
    if hi == lo:
        return out
    lo64, hi64 = np.float64(lo), np.float64(hi)
    g = np.rint((s.astype(np.float64) - lo64) / (hi64 - lo64) * np.float64(NR_OF_GRAY - 1))
    g = g.astype(np.uint16)
    (py0, py1), (px0, px1) = pads(sy, ky), pads(sx, kx)
    g = np.pad(g, ((py0, py1), (px0, px1)), mode='reflect')
    bins = (g // np.uint16(1 + NR_OF_GRAY // nbins)).astype(np.int64)
    P = bins.shape
    nty, ntx = P[0] // ky - 1, P[1] // kx - 1
    maps = np.zeros((nty, ntx, nbins), np.uint16)
    for i in range(nty):
        for j in range(ntx):
            tile = bins[ky // 2 + i * ky: ky // 2 + (i + 1) * ky,
                        kx // 2 + j * kx: kx // 2 + (j + 1) * kx]
            h = np.bincount(tile.reshape(-1), minlength=nbins).astype(np.int64)
            maps[i, j] = map_histogram(clip_histogram(h, clim, passes), ky * kx)
    y, x = np.arange(P[0]), np.arange(P[1])
    by, cy = y // ky, (y % ky).astype(np.float64) / np.float64(ky)
    bx, cx = x // kx, (x % kx).astype(np.float64) / np.float64(kx)
    r = np.zeros(P, np.float64)
    for ey, ex in ((0, 0), (0, 1), (1, 0), (1, 1)):
        ty = np.clip(by - 1 + ey, 0, nty - 1)
        tx = np.clip(bx - 1 + ex, 0, ntx - 1)
        wy = cy if ey else 1.0 - cy
        wx = cx if ex else 1.0 - cx
        w = wy[:, None] * wx[None, :]
        r = r + maps[ty[:, None], tx[None, :], bins].astype(np.float64) * w
    r = r.astype(np.int64).astype(np.uint16)[py0:py0 + sy, px0:px0 + sx]
    rmin, rmax = int(r.min()), int(r.max())
    if rmax == rmin:
        return out
    return ((r.astype(np.float64) - np.float64(rmin)) / np.float64(rmax - rmin)).astype(np.float32)


def clahe_numpy(im, kernel_size, clip_limit=0.01, nbins=256, zero_mean=False, trace=None):
    """the specification (module docstring): float32 (Z, Y, X) of a uint8 or float32 volume.
    A constant slice of a non-constant volume is 0.0 (skimage's result there depends on its
    version); a constant volume raises ValueError.  Single-threaded and written for clarity.

    `trace`: a dict that receives 'max_passes' (the most outer `while` passes a tile's clip took),
    'tiles_in_while' (the tiles that entered the `while` at all), 'max_pad_ratio' (the largest
    pad / (s - 1)) and 'nt' (tiles per axis)."""
    im = _as_volume(im, 'clahe')
    nbins = int(nbins)
    if nbins < 1:
        raise ValueError('clahe: nbins %d' % nbins)
    ky, kx = k = tile_size(kernel_size, im.shape[1:])
    mn, mx = im.min(), im.max()
    if not (np.isfinite(mn) and np.isfinite(mx)):
        raise ValueError('clahe: the volume holds non-finite values')
    if mx == mn:
        raise ValueError('clahe: the volume is constant (%r): its range is empty' % float(mn))
    clim = clip_count(clip_limit, ky, kx)
    out = np.zeros(im.shape, np.float32)
    passes = []
    den = np.float32(mx - mn)
    for z in range(im.shape[0]):
        s = (im[z] - mn) / den
        out[z] = _slice_numpy(s, k, clim, nbins, passes)
    if zero_mean:
        out = out - np.float32(0.5)
    if trace is not None:
        sy, sx = im.shape[1:]
        trace['max_passes'] = max(passes) if passes else 0
        trace['tiles_in_while'] = int(np.count_nonzero(passes))
        trace['max_pad_ratio'] = max(max(pads(s, kk)) / max(s - 1, 1)
                                     for s, kk in ((sy, ky), (sx, kx)))
        trace['nt'] = (-(-sy // ky), -(-sx // kx))
    return out


# ---- the device path -------------------------------------------------------------------------------

def check_device_args(im, k, nbins, who='clahe'):
    """what the device path does not take, as ValueError, before any library is loaded.  Returns
    (shape, is_uint8)."""
    from . import _device
    shape, dtype = tuple(int(v) for v in im.shape), str(im.dtype).replace('torch.', '')
    if dtype not in ('uint8', 'float32'):
        raise ValueError('%s(device=): the volume must be uint8 or float32, got %s' % (who, dtype))
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError('%s(device=): the volume must be 3-D (Z, Y, X) and not empty, got shape %s'
                         % (who, shape))
    if not 2 <= int(nbins) <= MAX_DEVICE_NBINS:
        raise ValueError('%s(device=): nbins %d is outside 2..%d' % (who, int(nbins), MAX_DEVICE_NBINS))
    if k[0] * k[1] >= 2 ** 31:
        raise ValueError('%s(device=): a tile of %d x %d holds 2^31 or more pixels' % (who, k[0], k[1]))
    if shape[0] * shape[1] * shape[2] >= 2 ** 31:
        raise ValueError('%s(device=): a volume of %s holds 2^31 or more voxels, more than the kernels '
                         'index' % (who, shape))
    if _device.is_device_tensor(im) and not im.is_contiguous():
        raise ValueError('%s(device=): a resident volume must be contiguous' % who)
    if not isinstance(im, np.ndarray) and not _device.is_device_tensor(im):
        raise ValueError('%s(device=): the volume must be a numpy array or a torch CUDA tensor, got %s'
                         % (who, type(im).__name__))
    return shape, dtype == 'uint8'


def clahe_device(im, kernel_size, clip_limit=0.01, nbins=256, zero_mean=False, device=True,
                 out=None, scratch=None):
    """`clahe_numpy` on a GPU, bit for bit: `im` is a numpy uint8 / float32 array (uploaded once)
    or a contiguous torch CUDA tensor of those dtypes on that device (a view that starts at an
    element offset is fine).  Returns a contiguous float32 torch CUDA tensor of the input's shape,
    left resident.  `out` (float32, contiguous, the input's shape) and `scratch` (uint8,
    contiguous, 16-byte aligned, at least `_clahecapi.scratch_bytes(...)`) may be given.
    Stream-ordered on torch's current stream; the call ends with one 16-byte download (the
    volume's range), so a constant or non-finite volume raises ValueError as on the host."""
    from . import _clahecapi, _device
    who = 'clahe'
    if not isinstance(im, np.ndarray) and not hasattr(im, 'data_ptr'):
        im = np.asarray(im)
    if len(im.shape) == 3:
        k = tile_size(kernel_size, tuple(im.shape)[1:])
    else:
        k = (1, 1)
    (Z, Y, X), is_u8 = check_device_args(im, k, nbins, who)
    nbins, (ky, kx) = int(nbins), k
    clim = clip_count(clip_limit, ky, kx)
    torch = _device.require_torch('clahe(device=) needs', 'there is no host fallback; use device=None')
    dev = _device.torch_device(device, 'clahe', _clahecapi.load_library)
    if isinstance(im, np.ndarray):
        src = torch.from_numpy(np.ascontiguousarray(im)).to(dev)
    else:
        src = im
        if src.device != dev:
            raise ValueError('%s(device=%s): the volume lives on %s' % (who, dev, src.device))
    if out is None:
        out = torch.empty((Z, Y, X), dtype=torch.float32, device=dev)
    elif not _device.is_device_tensor(out) or out.dtype != torch.float32 or out.device != dev \
            or not out.is_contiguous() or tuple(out.shape) != (Z, Y, X):
        raise ValueError('%s: out must be a contiguous float32 tensor of %s on %s' % (who, (Z, Y, X), dev))
    need = _clahecapi.scratch_bytes(Z, Y, X, ky, kx, nbins)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    elif not _device.is_device_tensor(scratch) or scratch.dtype != torch.uint8 or scratch.device != dev \
            or not scratch.is_contiguous() or scratch.numel() < need or scratch.data_ptr() % 16:
        raise ValueError('%s: scratch must be a contiguous, 16-byte aligned uint8 tensor of at least '
                         '%d bytes on %s' % (who, need, dev))
    with torch.cuda.device(dev):
        _clahecapi.clahe(src, is_u8, (Z, Y, X), (ky, kx), clim, nbins, zero_mean, out, scratch, need,
                         _clahecapi.STAGE_ALL, torch.cuda.current_stream(dev).cuda_stream)
        status = scratch[:_clahecapi.STATUS_BYTES].cpu().numpy()
    mn, mx = status[:8].view(np.float32)
    if status[8:12].view(np.uint32)[0]:
        raise ValueError('clahe: the volume holds non-finite values')
    if mx == mn:
        raise ValueError('clahe: the volume is constant (%r): its range is empty' % float(mn))
    return out
