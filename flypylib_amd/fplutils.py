"""Small helpers shared by the T-bar detection path.

Mirrors the two hot-path helpers of the reference (`flypylib/fplutils.py:9-22`):
`to3d` (scalar -> 3-tuple) and `set_filter` (boolean ball used by the NMS).
`clahe` is the reference's per-slice contrast-limited adaptive histogram equalisation
(`fplutils.py:33-62`), on the host or, with `device=`, on the GPU.  Its specification is this
package's own (`flypylib_amd/clahe.py`), following the n-D algorithm of scikit-image >= 0.17;
scikit-image is no dependency and the reference pins no version of it, so parity with skimage is
UNPINNED.  `roi_from_txt` is not provided.
"""
from collections import namedtuple

import numpy as np

szyx = namedtuple('szyx', 'size z y x')


def to3d(vv):
    """scalar -> (v, v, v); anything of size 3 is returned as given
    (reference `fplutils.py:9-12`)."""
    if np.size(vv) == 1:
        if isinstance(vv, (tuple, list, np.ndarray)):
            vv = np.asarray(vv).reshape(-1)[0]
            if isinstance(vv, np.generic):
                vv = vv.item()
        return (vv, vv, vv)
    return vv


def ball_sq_dist(radius):
    """integer squared distance from the centre on a (2r+1)^3 grid"""
    ax = np.arange(-radius, radius + 1, dtype=np.int64)
    return (ax[:, None, None] ** 2 + ax[None, :, None] ** 2
            + ax[None, None, :] ** 2)


def set_filter(radius, return_dist=False):
    """boolean ball `dist <= radius` on a (2r+1)^3 grid (reference
    `fplutils.py:14-22`).  For integer radius, `sqrt(d2) <= r` and `d2 <= r*r`
    select the same voxels; the float distance is only materialised on request."""
    d2 = ball_sq_dist(int(radius))
    inside = d2 <= int(radius) * int(radius)
    if return_dist:
        return inside, np.sqrt(d2.astype(np.float64))
    return inside


def clahe(im_in, kernel_size, fn_out=None, zero_mean=False, device=None, clip_limit=0.01, nbins=256):
    """per-slice CLAHE of a (Z, Y, X) volume as float32 in [0, 1] (`zero_mean`: - 0.5), the
    reference's `clahe(im_in, kernel_size, fn_out, zero_mean)` (`fplutils.py:33-62`).

    The specification is the package's own, `clahe.clahe_numpy`: the volume is scaled by its own
    min and max, each slice is stretched to 16384 gray levels, tiled into `kernel_size` tiles
    (a scalar, a (ky, kx) pair, or None for an eighth of the slice), every tile's `nbins`-bin
    histogram is clipped at `clip_limit` and turned into a map, and every pixel is interpolated
    between the maps of its four tiles.  Parity with skimage.exposure.equalize_adapthist is
    UNPINNED: skimage is no dependency, the reference pins no version, and its intermediate dtypes
    moved between releases.  A constant slice of a non-constant volume comes out 0.0 (skimage's
    result there depends on its version); a constant volume raises ValueError (the reference
    divides by zero).

    im_in: an array, or a path (`.npy`, or `.h5` with a dataset `/main`).
    device=None: the numpy executor; returns a numpy float32 array.
    device=<int> or True (the runtime's default device): libfplclahe.so.  `im_in` is a numpy uint8
    / float32 array (uploaded once) or a contiguous torch CUDA tensor of those dtypes on that
    device; the result is a contiguous float32 torch CUDA tensor, left resident and bit-identical
    to the numpy executor's.  Other dtypes, nbins outside 2..256, a tile of 2^31 or more pixels
    and a volume that is not 3-D raise ValueError at the call; without torch, a GPU or the
    library the call raises - there is no silent host fallback.
    fn_out: a `.npy` name is written with np.save, anything else as an HDF5 file whose `/main` is
    the float32 volume, CONTIGUOUS (the reference compresses with gzip).  A device result is
    downloaded for this and still returned resident.

    Measured on one MI355X at 520^3 uint8, kernel_size=64 (profiles/clahe.json, medians of 5):
    4 949 ms on the host, 11.3 ms with device= from a host array, 8.8 ms from a resident tensor."""
    from . import clahe as _clahe
    if isinstance(im_in, str):
        from .fplobjdetect import _load_main
        im_in = _load_main(im_in)
    if device is None or device is False:
        if hasattr(im_in, 'data_ptr'):
            im_in = im_in.cpu().numpy()
        im_out = _clahe.clahe_numpy(im_in, kernel_size, clip_limit, nbins, zero_mean)
        host = im_out
    else:
        im_out = _clahe.clahe_device(im_in, kernel_size, clip_limit, nbins, zero_mean, device)
        host = None
    if fn_out is not None:
        if host is None:
            host = im_out.cpu().numpy()
        if str(fn_out).endswith('.npy'):
            np.save(fn_out, host)
        else:
            from . import keras_io
            keras_io.write_main(fn_out, host)
    return im_out
