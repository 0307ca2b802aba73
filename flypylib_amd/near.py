"""The close pairs WITHIN one point set, as a CSR table, for fplsynapses.rm_tbar_multi_pred.

rm_tbar_multi_pred merges detections of one T-bar that two neighbouring substacks both made.
The reference builds an N x N distance matrix for that; at the 10^5 - 10^7 points of a whole ROI
only the few points around each point matter.  Here:

  pairs_numpy / pairs_device  (indptr, indices): row i holds every j != i with 0 < s <= T2 in
                              ascending j - the arithmetic and the generous superset of
                              match.pairs_numpy, so neither executor has to reproduce the
                              other's sqrt.  The numpy function is the specification
                              libfplnear.so's kernels are tested against, byte for byte.
  CellGrid                    the cell binning both are built on, and the ball query around a
                              point that need not be in the set (a moved centre).

Cells.  The side of a cell is c = sqrt(T2) (1 + 2^-20); a point's cell along an axis is
floor((x - min) / c) in float64.  Two points no further apart than sqrt(T2) on an axis differ
by less than 1 - 2^-20 before rounding and by at most 2^-50 times the cell number after it, so
with at most 2^28 cells per axis (MAX_AXIS_BITS; more is refused) they lie at most one cell
apart and every partner of a point is in the 27 cells around its own.  The key of a cell is
(cz * ny + cy) * nx + cx: the three x-adjacent cells of a row are one contiguous key range,
nine ranges per point.
"""
import numpy as np

from . import _device, _nearcapi
from .match import _points, threshold2

BLOCK_ELEMENTS = 1 << 20     # pairs_numpy tests about this many candidate pairs at a time
MARGIN = 1 + 2.0 ** -20
MAX_AXIS = 1 << _nearcapi.MAX_AXIS_BITS
MAX_CELLS = 1 << 62


def cell_side(thresh):
    """c = sqrt(T2) (1 + 2^-20)"""
    return float(np.sqrt(threshold2(thresh))) * MARGIN


def grid_of(locs, thresh):
    """(origin, cell side, (nx, ny, nz)) of the cell grid of N >= 1 finite points; ValueError
    where the points are spread over more cells than a key can number"""
    if not np.all(np.isfinite(locs)):
        raise ValueError('the points must be finite')
    cell = cell_side(thresh)
    origin = locs.min(axis=0)
    dims = tuple(int(v) + 1 for v in np.floor((locs.max(axis=0) - origin) / cell))
    if max(dims) > MAX_AXIS or dims[0] * dims[1] * dims[2] > MAX_CELLS:
        raise ValueError('the points span %d x %d x %d cells of side %g: more than 2^%d along an '
                         'axis or 2^62 in all; they are spread too far for this threshold'
                         % (dims + (cell, _nearcapi.MAX_AXIS_BITS)))
    return origin, cell, dims


def _cells(x, origin, cell, dims):
    """int64 cell coordinates (..., 3) of points inside the grid's box"""
    u = (x - origin) / cell
    return np.floor(np.clip(u, 0.0, np.asarray(dims, np.float64) - 1)).astype(np.int64)


def _expand(lo, hi):
    """(owner, position) of every position in the runs [lo[k], hi[k])"""
    n = hi - lo
    owner = np.repeat(np.arange(len(lo)), n)
    start = np.cumsum(n) - n
    return owner, np.arange(int(n.sum())) - np.repeat(start, n) + np.repeat(lo, n)


class CellGrid:
    """N points binned into cells of side cell_side(thresh): sorted keys and the order that
    sorts them - O(N) memory whatever the extent."""

    def __init__(self, locs, thresh):
        self.locs = _points(locs)
        self.n = len(self.locs)
        if self.n:
            self.origin, self.cell, self.dims = grid_of(self.locs, thresh)
            c = _cells(self.locs, self.origin, self.cell, self.dims)
            keys = (c[:, 2] * self.dims[1] + c[:, 1]) * self.dims[0] + c[:, 0]
            self.order = np.argsort(keys, kind='stable')
            self.keys = keys[self.order]
            self.cells = c

    def runs(self, cells):
        """(lo, hi), each (K, 9): the positions in key order of the candidates of K cell
        coordinates (which may lie outside the grid) - the 27 cells around each"""
        nx, ny, nz = self.dims
        cells = np.asarray(cells, np.int64).reshape(-1, 3)
        d = np.arange(9)
        y = cells[:, 1:2] + (d % 3 - 1)
        z = cells[:, 2:3] + (d // 3 - 1)
        x0 = np.maximum(cells[:, 0:1] - 1, 0)
        x1 = np.minimum(cells[:, 0:1] + 1, nx - 1)
        live = (y >= 0) & (y < ny) & (z >= 0) & (z < nz) & (x0 <= x1)
        row = (np.where(live, z, 0) * ny + np.where(live, y, 0)) * nx
        lo = np.searchsorted(self.keys, row + x0, 'left')
        hi = np.searchsorted(self.keys, row + x1, 'right')
        return np.where(live, lo, 0), np.where(live, hi, 0)

    def ball(self, centre):
        """ascending indices of a superset of the points closer than the threshold to
        `centre`, which need not be a point of the set nor lie inside the grid: the points of
        the 27 cells around its cell.  The caller applies its own exact distance test."""
        if not self.n:
            return np.zeros(0, np.int64)
        u = np.floor((np.asarray(centre, np.float64) - self.origin) / self.cell)
        # beyond the grid by more than a cell there is nothing; the clip keeps int64 exact
        c = np.clip(u, -2.0, np.asarray(self.dims, np.float64) + 1).astype(np.int64)
        lo, hi = self.runs(c)
        _, pos = _expand(lo[0], hi[0])
        return np.sort(self.order[pos])


def pairs_numpy(locs, thresh):
    """(indptr, indices): int64 row pointers (N + 1) and int32 columns of the CSR table whose
    row i holds every j != i with 0 < s <= T2, in ascending j, where
    s = (dx*dx + dy*dy) + dz*dz in float64, every operation rounded on its own, and
    T2 = match.threshold2(thresh).  Coincident points (s == 0) are no partners.  The table is
    symmetric and stores both directions.

    Built by cell binning (CellGrid): the points are walked in key order, about BLOCK_ELEMENTS
    candidate pairs at a time, so the memory is O(N + table) whatever N is - no N x N object."""
    grid = CellGrid(locs, thresh)
    n, pts = grid.n, grid.locs
    t2 = threshold2(thresh)
    ii, jj = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    if n:
        lo, hi = grid.runs(grid.cells[grid.order])           # (N, 9), in key order
        cand = np.cumsum((hi - lo).sum(axis=1))
        k0 = 0
        while k0 < n:
            # as many points as hold about BLOCK_ELEMENTS candidates, at least one
            base = cand[k0 - 1] if k0 else 0
            k1 = max(k0 + 1, int(np.searchsorted(cand, base + BLOCK_ELEMENTS, 'right')))
            owner, pos = _expand(lo[k0:k1].reshape(-1), hi[k0:k1].reshape(-1))
            i, j = grid.order[k0 + owner // 9], grid.order[pos]
            d = pts[i, 0] - pts[j, 0]
            s = d * d
            np.subtract(pts[i, 1], pts[j, 1], out=d)
            s += d * d
            np.subtract(pts[i, 2], pts[j, 2], out=d)
            s += d * d
            keep = (s > 0) & (s <= t2)
            ii.append(i[keep])
            jj.append(j[keep])
            k0 = k1
    i, j = np.concatenate(ii), np.concatenate(jj)
    by_row = np.lexsort((j, i))
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(i, minlength=n), out=indptr[1:])
    return indptr, j[by_row].astype(np.int32)


# ---- device path ---------------------------------------------------------------------------

def _torch():
    return _device.require_torch('the device table needs',
                                 "use method='sparse' without device= for the host table")


def torch_device(device):
    """torch.device of `device` (an int, or True for the runtime's default device);
    FplNearError if the library is not built"""
    _torch()
    return _device.torch_device(device, 'the device table', _nearcapi.load_library)


def pairs_device(locs, thresh, device, info=None):
    """pairs_numpy's table from libfplnear.so: the float64 points are uploaded, their cell
    keys computed and sorted (torch.sort), the partners counted, the columns allocated and
    filled, and only the row offsets and columns are downloaded.  `info`, a dict, receives the
    entry count and the grid."""
    pts = _points(locs)
    n = len(pts)
    torch = _torch()
    dev = torch_device(device)
    if n == 0:
        return np.zeros(1, np.int64), np.zeros(0, np.int32)
    if n > _nearcapi.MAX_POINTS:
        raise ValueError('%d points exceed the 2^31 - 1 the kernels index; merge them in parts' % n)
    t2 = threshold2(thresh)
    origin, cell, dims = grid_of(pts, thresh)
    nscr = _nearcapi.scratch_bytes(n)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        p_dev = torch.from_numpy(pts).to(dev)
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        _nearcapi.cell_keys(p_dev.data_ptr(), n, origin, cell, dims, keys.data_ptr(),
                            stream.cuda_stream)
        keys, order = torch.sort(keys)
        scratch = torch.empty((nscr + 7) // 8, dtype=torch.int64, device=dev)
        args = (p_dev.data_ptr(), n, t2, origin, cell, dims, keys.data_ptr(), order.data_ptr(),
                scratch.data_ptr(), nscr)
        total = _nearcapi.pairs_count(*args, stream.cuda_stream)
        indices = torch.empty(total, dtype=torch.int32, device=dev)
        if total:
            _nearcapi.pairs_fill(*args, total, indices.data_ptr(), stream.cuda_stream)
        # the n + 1 uint32 row offsets stand behind the 16-byte head of the scratch
        offsets = scratch.view(torch.int32)[4:4 + n + 1]
        stream.synchronize()
        indptr = offsets.cpu().numpy().view(np.uint32).astype(np.int64)
        host = indices.cpu().numpy()
    if info is not None:
        info.update(entries=total, dims=dims, cell=cell)
    return indptr, host
