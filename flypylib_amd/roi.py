"""The region of interest as an object: `BlockRoi`, DVID's ROI form - runs of blocks - with the
array work the reference asks three DVID services for (`get_roi_partition`, `get_roi3D`,
`roi_ptquery`; reference fplsynapses.py:154-166, :206-208, :244-248, fplobjdetect.py:974-980).

Everything here is numpy and is the specification.  `roi3D`, `ptquery` and `voxel_counts` take
`device=`: the same answers from libfplroi.so (include/fplroi.h) on three small tables uploaded
once per device - the sorted (z, y) keys of the block rows, a CSR row start and the int32
(x0, x1) of every run.  Nothing falls back to the host when the library or the GPU is missing.

The package's own rules (DVID is not available to compare against, so these are UNPINNED against
it):
  * the block of a voxel coordinate v is v // block_size, Python floor division, for negative
    coordinates too;
  * `partition` lays its cubes on the grid of multiples of `partition_size` blocks from block 0
    (floor division for negatives), keeps a cube that holds at least one ROI block, and orders
    them by ascending (z, y, x).
"""
import json
import os

import numpy as np

from . import fplutils

# block coordinates are int32 on the device, and (x1 + 1) * block_size must stay far from 2^63
MAX_BLOCK_COORD = 2 ** 30
MAX_BLOCK_SIZE = 2 ** 20
# voxel coordinates and box sides the device entry points take
MAX_COORD = 2 ** 40
MAX_SIDE = 2 ** 21


def _row_key(z, y):
    """one int64 per (z, y) of block coordinates, ordered as the pairs are"""
    return np.asarray(z, np.int64) * (1 << 32) + (np.asarray(y, np.int64) + (1 << 31))


def _box(dims, offset, who):
    dims, offset = [int(v) for v in dims], [int(v) for v in offset]
    if len(dims) != 3 or len(offset) != 3 or min(dims) < 0:
        raise ValueError('%s: dims %r and offset %r must be (z, y, x) with no negative side'
                         % (who, dims, offset))
    return dims, offset


class BlockRoi:
    """An ROI as DVID holds it: `runs`, an integer (n, 4) array of [z, y, x0, x1] in BLOCK
    coordinates with x1 inclusive, and `block_size` voxels per block side (DVID's 32).

    The constructor canonicalises: the runs are sorted by (z, y, x0) and the overlapping or
    abutting runs of a row are merged into one, so two ROIs cover the same blocks exactly when
    their `runs` are equal.  x1 < x0, or a shape other than (n, 4), is a ValueError; n = 0 is a
    valid, empty ROI.

    The block of a voxel coordinate v is v // block_size (Python floor division, for negative
    coordinates too).  That is this package's rule: DVID cannot be consulted here."""

    def __init__(self, runs, block_size=32):
        if int(block_size) != block_size or not 1 <= int(block_size) <= MAX_BLOCK_SIZE:
            raise ValueError('block_size %r must be an integer in [1, 2^20]' % (block_size,))
        self.block_size = int(block_size)
        runs = np.asarray(runs)
        if runs.size == 0 and runs.ndim <= 2:
            runs = np.zeros((0, 4), np.int64)
        if runs.ndim != 2 or runs.shape[1] != 4:
            raise ValueError('runs must be (n, 4) rows of [z, y, x0, x1], got shape %r' % (runs.shape,))
        if runs.dtype.kind not in 'iu':
            raise ValueError('runs must be integers, got %s' % runs.dtype)
        runs = runs.astype(np.int64)
        if np.any(runs[:, 3] < runs[:, 2]):
            j = int(np.argmax(runs[:, 3] < runs[:, 2]))
            raise ValueError('run %d: x1 %d < x0 %d' % (j, runs[j, 3], runs[j, 2]))
        if runs.size and np.abs(runs).max() >= MAX_BLOCK_COORD:
            raise ValueError('block coordinates must lie within +-2^30')
        self.runs = self._canonical(runs)
        self.runs.setflags(write=False)
        # the three tables: sorted row keys, CSR row start, int32 (x0, x1)
        key = _row_key(self.runs[:, 0], self.runs[:, 1])
        self.row_keys, first = np.unique(key, return_index=True)
        self.row_start = np.concatenate([first, [len(key)]]).astype(np.int32)
        self.runs_x = np.ascontiguousarray(self.runs[:, 2:4], np.int32)
        # (row index, x0) of every run in one sorted int64: the search of ptquery
        row_of_run = np.repeat(np.arange(len(self.row_keys), dtype=np.int64), np.diff(self.row_start))
        self._run_key = row_of_run * (1 << 32) + (self.runs[:, 2] + (1 << 31))
        self._device_tables = {}

    @staticmethod
    def _canonical(runs):
        if len(runs) == 0:
            return runs.reshape(0, 4)
        runs = runs[np.lexsort((runs[:, 2], runs[:, 1], runs[:, 0]))]
        out = []
        z, y, x0, x1 = (int(v) for v in runs[0])
        for rz, ry, rx0, rx1 in runs[1:].tolist():
            if rz == z and ry == y and rx0 <= x1 + 1:
                x1 = max(x1, rx1)
            else:
                out.append((z, y, x0, x1))
                z, y, x0, x1 = rz, ry, rx0, rx1
        out.append((z, y, x0, x1))
        return np.asarray(out, np.int64)

    def __len__(self):
        return len(self.runs)

    def __eq__(self, other):
        return (isinstance(other, BlockRoi) and self.block_size == other.block_size
                and np.array_equal(self.runs, other.runs))

    __hash__ = None

    def __repr__(self):
        return 'BlockRoi(%d runs, %d blocks, block_size=%d)' % (len(self.runs), self.n_blocks,
                                                               self.block_size)

    @property
    def n_blocks(self):
        return int((self.runs[:, 3] - self.runs[:, 2] + 1).sum())

    # ---- DVID's JSON: a list of [z, y, x0, x1] ------------------------------------------------
    @classmethod
    def from_json(cls, path_or_text, block_size=32):
        text = path_or_text
        if os.path.isfile(path_or_text):
            with open(path_or_text) as f_in:
                text = f_in.read()
        doc = json.loads(text)
        return cls(np.asarray(doc if doc else [], np.int64).reshape(-1, 4), block_size)

    def to_json(self, path=None):
        text = json.dumps(self.runs.tolist())
        if path is not None:
            with open(path, 'w') as f_out:
                f_out.write(text)
        return text

    # ---- dense block masks -----------------------------------------------------------------------
    @classmethod
    def from_block_mask(cls, mask_zyx, origin=(0, 0, 0), block_size=32):
        """the ROI of the blocks set in the (nz, ny, nx) mask, whose [0, 0, 0] is block `origin`"""
        m = np.asarray(mask_zyx) != 0
        if m.ndim != 3:
            raise ValueError('a block mask is (nz, ny, nx), got shape %r' % (m.shape,))
        pad = np.zeros(m.shape[:2] + (1,), bool)
        d = np.diff(np.concatenate([pad, m, pad], axis=2).astype(np.int8), axis=2)
        z, y, x0 = np.nonzero(d == 1)
        _, _, x1 = np.nonzero(d == -1)              # the same row-major order: run for run
        oz, oy, ox = (int(v) for v in origin)
        return cls(np.stack([z + oz, y + oy, x0 + ox, x1 - 1 + ox], axis=1).astype(np.int64),
                   block_size)

    def _sub_block_mask(self, lo, hi):
        """bool mask of the blocks lo <= (z, y, x) < hi"""
        shape = tuple(max(int(h - l), 0) for l, h in zip(lo, hi))
        out = np.zeros(shape, bool)
        r = self.runs
        if out.size == 0 or len(r) == 0:
            return out
        r = r[(r[:, 0] >= lo[0]) & (r[:, 0] < hi[0]) & (r[:, 1] >= lo[1]) & (r[:, 1] < hi[1])
              & (r[:, 3] >= lo[2]) & (r[:, 2] < hi[2])]
        edge = np.zeros(shape[:2] + (shape[2] + 1,), np.int32)
        z, y = r[:, 0] - lo[0], r[:, 1] - lo[1]
        np.add.at(edge, (z, y, np.maximum(r[:, 2], lo[2]) - lo[2]), 1)
        np.add.at(edge, (z, y, np.minimum(r[:, 3] + 1, hi[2]) - lo[2]), -1)
        return np.cumsum(edge, axis=2)[:, :, :-1] > 0

    def block_mask(self):
        """-> (mask, origin): the dense bool mask of the ROI's bounding box of blocks and the
        block coordinates of its [0, 0, 0]; ((0, 0, 0)-shaped, (0, 0, 0)) for the empty ROI"""
        if len(self.runs) == 0:
            return np.zeros((0, 0, 0), bool), (0, 0, 0)
        lo = (int(self.runs[:, 0].min()), int(self.runs[:, 1].min()), int(self.runs[:, 2].min()))
        hi = (int(self.runs[:, 0].max()) + 1, int(self.runs[:, 1].max()) + 1,
              int(self.runs[:, 3].max()) + 1)
        return self._sub_block_mask(lo, hi), lo

    # ---- the three services -------------------------------------------------------------------------
    def roi3D(self, dims, offset, device=None):
        """the uint8 (Z, Y, X) mask, 1 inside the ROI, of the box of `dims` voxels at `offset`,
        both (z, y, x) as libdvid's get_roi3D takes them.  Any part of the box may lie outside
        the ROI's extent or at negative coordinates.  device=<int> (or True): rendered by
        libfplroi.so into a resident uint8 torch tensor, the same bytes."""
        dims, offset = _box(dims, offset, 'roi3D')
        if device is not None:
            return _roi3d_device(self, dims, offset, device)
        b = self.block_size
        ax = [(o + np.arange(d, dtype=np.int64)) // b for d, o in zip(dims, offset)]
        if min(dims) == 0:
            return np.zeros(dims, np.uint8)
        lo = [int(a[0]) for a in ax]
        hi = [int(a[-1]) + 1 for a in ax]
        blocks = self._sub_block_mask(lo, hi)
        return blocks[np.ix_(ax[0] - lo[0], ax[1] - lo[1], ax[2] - lo[2])].astype(np.uint8)

    def ptquery(self, points, device=None):
        """bool (N,): whether each of the integer (N, 3) `points`, (z, y, x) voxels, lies in the
        ROI.  The reference hands over np.fliplr(locs).astype('int') and so do this package's
        callers, truncation included.  device=<int> (or True): libfplroi.so; numpy points are
        uploaded and the flags come back as numpy, a resident int64 tensor gives a resident bool
        tensor."""
        if device is not None:
            return _ptquery_device(self, points, device)
        pts = np.asarray(points)
        if pts.size == 0:
            return np.zeros(0, bool)
        if pts.ndim != 2 or pts.shape[1] != 3 or pts.dtype.kind not in 'iu':
            raise ValueError('points must be integer (N, 3) rows of (z, y, x), got %s %r'
                             % (pts.dtype, pts.shape))
        blk = pts.astype(np.int64) // self.block_size
        if len(self.runs) == 0:
            return np.zeros(len(pts), bool)
        ok = np.all(np.abs(blk) < MAX_BLOCK_COORD, axis=1)
        blk = np.where(ok[:, None], blk, 0)
        key = _row_key(blk[:, 0], blk[:, 1])
        row = np.minimum(np.searchsorted(self.row_keys, key), len(self.row_keys) - 1)
        ok &= self.row_keys[row] == key
        # the last run of that row with x0 <= x
        at = np.searchsorted(self._run_key, row * (1 << 32) + (blk[:, 2] + (1 << 31)), side='right') - 1
        at_c = np.maximum(at, 0)
        ok &= (at >= self.row_start[row]) & (blk[:, 2] <= self.runs[at_c, 3])
        return ok

    def voxel_counts(self, boxes, device=None):
        """int64 (S,): the ROI voxels inside each of the int64 (S, 6) `boxes`, rows of
        (z, y, x, dz, dy, dx) - roi3D((dz, dy, dx), (z, y, x)).sum() - computed from the runs;
        nothing is rendered.  device=<int> (or True): libfplroi.so, one workgroup per box."""
        boxes = np.asarray(boxes)
        if boxes.size == 0:
            boxes = np.zeros((0, 6), np.int64)
        if boxes.ndim != 2 or boxes.shape[1] != 6 or boxes.dtype.kind not in 'iu':
            raise ValueError('boxes must be integer (S, 6) rows of (z, y, x, dz, dy, dx), got %s %r'
                             % (boxes.dtype, boxes.shape))
        boxes = np.ascontiguousarray(boxes, np.int64)
        if np.any(boxes[:, 3:] < 0):
            raise ValueError('a box has a negative side')
        if device is not None:
            return _counts_device(self, boxes, device)
        b, r = self.block_size, self.runs
        out = np.zeros(len(boxes), np.int64)
        if len(r) == 0:
            return out

        def overlap(lo, hi, blo, bhi):      # (S, 1) box against (1, n) run spans
            return np.maximum(np.minimum(hi, bhi) - np.maximum(lo, blo), 0)
        step = max(1, (1 << 22) // len(r))
        for a in range(0, len(boxes), step):
            bx = boxes[a:a + step, :, None]
            nz = overlap(bx[:, 0], bx[:, 0] + bx[:, 3], r[None, :, 0] * b, (r[None, :, 0] + 1) * b)
            ny = overlap(bx[:, 1], bx[:, 1] + bx[:, 4], r[None, :, 1] * b, (r[None, :, 1] + 1) * b)
            nx = overlap(bx[:, 2], bx[:, 2] + bx[:, 5], r[None, :, 2] * b, (r[None, :, 3] + 1) * b)
            out[a:a + step] = (nz * ny * nx).sum(axis=1)
        return out

    def partition(self, partition_size):
        """-> (substacks, packing_factor): the cubes of `partition_size` blocks per side, on the
        grid of multiples of `partition_size` blocks from block 0 (floor division for negatives),
        that hold at least one ROI block, as `fplutils.szyx` in VOXEL coordinates in ascending
        (z, y, x); packing_factor = ROI blocks / (cubes x partition_size^3), 0.0 for the empty
        ROI.  What libdvid's get_roi_partition answers is the reference's; this rule is the
        package's own and unpinned against DVID."""
        p = int(partition_size)
        if p != partition_size or p < 1:
            raise ValueError('partition_size %r must be an integer >= 1' % (partition_size,))
        r = self.runs
        if len(r) == 0:
            return [], 0.0
        c0, c1 = r[:, 2] // p, r[:, 3] // p
        n = c1 - c0 + 1
        which = np.repeat(np.arange(len(r)), n)
        cx = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n) + c0[which]
        cubes = np.unique(np.stack([r[which, 0] // p, r[which, 1] // p, cx], axis=1), axis=0)
        side = p * self.block_size
        subs = [fplutils.szyx(side, int(z) * side, int(y) * side, int(x) * side) for z, y, x in cubes]
        return subs, self.n_blocks / float(len(subs) * p ** 3)

    # ---- the device tables ---------------------------------------------------------------------------
    def device_tables(self, dev):
        """the three tables as resident tensors on the torch device `dev`, uploaded once:
        (row_keys int64 (R,), row_start int32 (R + 1,), runs_x int32 (n, 2)).  An empty ROI
        uploads one spare element each, so every pointer is valid."""
        import torch
        key = str(dev)
        if key not in self._device_tables:
            def up(a, dtype):
                a = np.ascontiguousarray(a, dtype)
                if a.size == 0:
                    a = np.zeros((1,) + a.shape[1:], dtype)
                return torch.from_numpy(a.copy()).to(dev)
            self._device_tables[key] = (up(self.row_keys, np.int64), up(self.row_start, np.int32),
                                        up(self.runs_x, np.int32))
        return self._device_tables[key]


def as_roi(roi, block_size=32):
    """a BlockRoi, or the one its JSON (path or text) describes"""
    if isinstance(roi, BlockRoi):
        return roi
    if isinstance(roi, str):
        return BlockRoi.from_json(roi, block_size)
    raise ValueError('an ROI is a BlockRoi or the path of its JSON, got %s' % type(roi).__name__)


# ---- the device path (libfplroi.so) -----------------------------------------------------------------

def _torch():
    from . import _device
    return _device.require_torch('BlockRoi(device=) needs', 'use device=None for the numpy path')


def torch_device(device):
    """torch.device of a `device=` argument; FplRoiError first if the library is not built"""
    from . import _device, _roicapi
    torch = _torch()
    if isinstance(device, torch.device):
        _roicapi.load_library()
        return device
    return _device.torch_device(device, 'BlockRoi(device=)', _roicapi.load_library)


def _check_box(dims, offset, who):
    if min(dims) < 1 or max(dims) >= MAX_SIDE or dims[0] * dims[1] * dims[2] >= 2 ** 31:
        raise ValueError('%s(device=): a box of %r voxels; every side must lie in [1, 2^21) and the '
                         'box hold fewer than 2^31 voxels' % (who, tuple(dims)))
    if max(abs(o) for o in offset) >= MAX_COORD:
        raise ValueError('%s(device=): offset %r outside +-2^40' % (who, tuple(offset)))


def _roi3d_device(roi, dims, offset, device, out=None):
    from . import _roicapi
    _check_box(dims, offset, 'roi3D')
    torch = _torch()
    dev = torch_device(device)
    if out is None:
        out = torch.empty(tuple(dims), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _roicapi.mask_box(roi.device_tables(dev), len(roi.row_keys), len(roi.runs), roi.block_size,
                          offset, dims, out, torch.cuda.current_stream(dev).cuda_stream)
    return out


def _ptquery_device(roi, points, device):
    from . import _device, _roicapi
    torch = _torch()
    dev = torch_device(device)
    resident = _device.is_device_tensor(points)
    if resident:
        if points.dtype != torch.int64 or points.dim() != 2 or points.shape[1] != 3 \
                or not points.is_contiguous() or points.device != dev:
            raise ValueError('ptquery(device=): resident points must be a contiguous int64 (N, 3) '
                             'tensor on %s' % dev)
        pts = points
    else:
        host = np.asarray(points)
        if host.size == 0:
            return np.zeros(0, bool)
        if host.ndim != 2 or host.shape[1] != 3 or host.dtype.kind not in 'iu':
            raise ValueError('points must be integer (N, 3) rows of (z, y, x), got %s %r'
                             % (host.dtype, host.shape))
        pts = torch.from_numpy(np.array(host, np.int64)).to(dev)
    n = int(pts.shape[0])
    flags = torch.empty(n, dtype=torch.uint8, device=dev)
    if n:
        with torch.cuda.device(dev):
            _roicapi.ptquery(roi.device_tables(dev), len(roi.row_keys), len(roi.runs), roi.block_size,
                             pts, n, flags, torch.cuda.current_stream(dev).cuda_stream)
    return flags != 0 if resident else flags.cpu().numpy().astype(bool)


def _counts_device(roi, boxes, device):
    from . import _roicapi
    torch = _torch()
    dev = torch_device(device)
    if len(boxes) == 0:
        return np.zeros(0, np.int64)
    if boxes[:, 3:].max() >= MAX_SIDE or np.abs(boxes[:, :3]).max() >= MAX_COORD:
        raise ValueError('voxel_counts(device=): a box side of 2^21 or more, or an origin outside '
                         '+-2^40')
    res = torch.from_numpy(boxes.copy()).to(dev)
    counts = torch.empty(len(boxes), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _roicapi.box_counts(roi.device_tables(dev), len(roi.row_keys), len(roi.runs), roi.block_size,
                            res, len(boxes), counts, torch.cuda.current_stream(dev).cuda_stream)
    return counts.cpu().numpy()


def cut_normalize_device(vol, extent, origin, dims, mean, std, dev, out=None):
    """float32 (v - mean) / std of the box `dims` at `origin` of the resident uint8 (Z, Y, X)
    volume `vol` (a torch tensor or a DeviceBuffer) of `extent`, zeros where the box leaves the
    volume: numpy's `(cube.astype('float32') - mean) / std` bit for bit.  A resident tensor."""
    from . import _roicapi
    torch = _torch()
    dims, origin = _box(dims, origin, 'cut_normalize')
    _check_box(dims, origin, 'cut_normalize')
    if out is None:
        out = torch.empty(tuple(dims), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _roicapi.cut_normalize_u8(vol, extent, origin, dims, mean, std, out,
                                  torch.cuda.current_stream(dev).cuda_stream)
    return out
