"""Training labels and mask around annotated T-bars: the per-voxel rule of
fplsynapses.write_labels_mask as a numpy executor (the specification; the CPU tests' and the
GPU tests' oracle), the planners of the device path, and the device path itself over
libfpllabels.so (include/fpllabels.h) and - planner='device' - libfplplan.so (include/fplplan.h).

`fplsynapses.write_labels_mask(device=...)` is the public surface; this module is what it
calls.  Nothing here falls back to the host when the library, torch or the GPU is missing.

The host loop visits the T-bars in list order: T-bar j clears the mask inside its ignore ball,
then sets mask and labels inside its use ball, both through assignments that cover the whole
cube around it.  Per voxel v that is a rule without an order of execution:

    J_set   = the largest j with v in T-bar j's use ball
    J_clr   = the largest j with v in T-bar j's ignore ball       (radius_ign > 0 only)
    touched = v lies in any T-bar's use cube or ignore cube
    labels  = J_set exists
    mask    = 1 if J_set exists and (no J_clr or J_set >= J_clr), else 0 if J_clr exists,
              else (roi != 0) if touched, else roi
    mask    = 0 within buffer_size of a face (buffer_size 0: everywhere, as mask[-0:] = 0)
"""
import numpy as np

from . import _device, _labelscapi, _plancapi

PLANNERS = ('host', 'device')
MAX_VOXELS = _labelscapi.MAX_VOXELS
BRICK = _labelscapi.BRICK


def _radii(radius_use, radius_ign):
    ru, ri = int(radius_use), 0 if radius_ign is None else int(radius_ign)
    if ru != radius_use or (radius_ign is not None and ri != radius_ign) or ru < 0 or ri < 0:
        raise ValueError('radius_use %r / radius_ign %r must be integers >= 0 (radius_ign may be '
                         'None)' % (radius_use, radius_ign))
    return ru, ri


def _table(locs, shape, ru, ri):
    shape = tuple(int(d) for d in shape)
    if len(shape) != 3:
        raise ValueError('shape %r: a (Z, Y, X) volume' % (shape,))
    locs = np.asarray(locs)
    if locs.size == 0:
        return np.zeros((0, 3), np.int32)
    if locs.ndim != 2 or locs.shape[1] < 3:
        raise ValueError("T-bar locations must be (N, >= 3), got %r" % (locs.shape,))
    xyz = np.trunc(locs[:, :3].astype(np.float64)).astype(np.int64)     # int(v) of the host loop
    half = max(ru, ri)
    ext = np.asarray(shape[::-1], np.int64)                              # (X, Y, Z)
    bad = np.any((xyz - half < 0) | (xyz + half >= ext), axis=1)
    if bad.any():
        j = int(np.argmax(bad))
        raise ValueError('T-bar %d at (x, y, z) = %r: its cube of half-width %d leaves the '
                         '(Z, Y, X) = %r volume' % (j, tuple(xyz[j].tolist()), half, shape))
    return np.ascontiguousarray(xyz, np.int32)


def plan_tbars(tbars, shape, radius_use, radius_ign):
    """int32 (N, 3) table of (x, y, z), truncated as the host loop's int(v) does.

    ValueError, naming the first offending T-bar, when the cube of half-width
    max(radius_use, radius_ign or 0) around a T-bar leaves the (Z, Y, X) volume.  The host
    path fails on a cube cut by a face with numpy's broadcast error whenever that half-width
    is > 0.  The documented differences: with half-width 0 the host path raises nothing (a
    T-bar outside the volume addresses an empty slice, or - at a negative coordinate within
    the extent - the voxel Python's negative index wraps to), and a cube that lies wholly at
    negative coordinates is wrapped by the host in the same way; both are refused here."""
    ru, ri = _radii(radius_use, radius_ign)
    locs = tbars['locs'] if isinstance(tbars, dict) else tbars
    return _table(locs, shape, ru, ri)


def _cleared(shape, buffer_size):
    """True where the buffer clear of the host loop zeroes the mask"""
    b = int(buffer_size)
    if b < 0:
        raise ValueError('buffer_size %r must not be negative' % (buffer_size,))
    out = np.ones(shape, bool)
    if b > 0 and all(d - b > b for d in shape):
        out[b:shape[0] - b, b:shape[1] - b, b:shape[2] - b] = False
    return out


def labels_mask_numpy(locs, roi_mask, radius_use, radius_ign, buffer_size, chunk=256):
    """(labels uint8, mask of roi_mask's dtype) by the per-voxel rule of this module's
    docstring, `chunk` T-bars at a time.  `locs`: (N, 3) of (x, y, z) in list order, as
    plan_tbars returns them (any other table is taken through the same check)."""
    ru, ri = _radii(radius_use, radius_ign)
    roi_mask = np.asarray(roi_mask)
    shape = roi_mask.shape
    locs = _table(locs, shape, ru, ri).astype(np.int64)
    half = max(ru, ri)
    Z, Y, X = shape
    n = roi_mask.size
    j_set = np.full(n, -1, np.int64)
    j_clr = np.full(n, -1, np.int64)
    touched = np.zeros(n, bool)
    ax = np.arange(-half, half + 1, dtype=np.int64)
    dz, dy, dx = np.meshgrid(ax, ax, ax, indexing='ij')
    d2 = (dz * dz + dy * dy + dx * dx).ravel()
    off = ((dz * Y + dy) * X + dx).ravel()
    use, ign = d2 <= ru * ru, (d2 <= ri * ri) & (ri > 0)
    for lo in range(0, len(locs), int(chunk)):
        part = locs[lo:lo + int(chunk)]
        j = np.arange(lo, lo + len(part), dtype=np.int64)[:, None]
        at = ((part[:, 2] * Y + part[:, 1]) * X + part[:, 0])[:, None] + off[None, :]
        touched[at.ravel()] = True
        np.maximum.at(j_set, at[:, use].ravel(), np.broadcast_to(j, (len(part), int(use.sum()))).ravel())
        if ri > 0:
            np.maximum.at(j_clr, at[:, ign].ravel(),
                          np.broadcast_to(j, (len(part), int(ign.sum()))).ravel())
    has_set, has_clr = j_set >= 0, j_clr >= 0
    labels = has_set.astype(np.uint8).reshape(shape)
    flat = roi_mask.ravel()
    mask = flat.copy()
    mask[touched] = flat[touched] != 0
    mask[has_clr] = 0
    mask[has_set & (j_set >= j_clr)] = 1
    mask = mask.reshape(shape)
    mask[_cleared(shape, buffer_size)] = 0
    return labels, mask


def brick_counts(shape, brick=BRICK):
    return tuple((int(d) + b - 1) // b for d, b in zip(shape, brick))


def _brick_ranges(locs, shape, half, brick):
    """per T-bar the first brick `lo` and the brick counts `cnt` of its clamped range on
    (z, y, x), their products `per` and the pair total"""
    nb = brick_counts(shape, brick)
    n_bricks = nb[0] * nb[1] * nb[2]
    if n_bricks + 1 > MAX_VOXELS:
        raise ValueError('a volume of %r voxels has more bricks than int32 offsets index'
                         % (tuple(shape),))
    locs = np.asarray(locs, np.int64).reshape(-1, 3)
    zyx = locs[:, ::-1]
    b = np.asarray(brick, np.int64)
    lo = np.maximum((zyx - int(half)) // b, 0)
    hi = np.minimum((zyx + int(half)) // b, np.asarray(nb, np.int64) - 1)
    cnt = np.maximum(hi - lo + 1, 0)
    per = cnt[:, 0] * cnt[:, 1] * cnt[:, 2]
    total = int(per.sum())
    if total > MAX_VOXELS:
        raise ValueError('%d (T-bar, brick) pairs exceed the int32 brick tables; render the '
                         'volume in parts' % total)
    return nb, n_bricks, len(locs), lo, cnt, per, total


def plan_pairs(locs, shape, half, brick=BRICK):
    """the (T-bar, brick) pairs plan_bricks lists, len(plan_bricks(...)[1]), without building
    the table: O(N).  The device planner is told this total; plan_bricks's own ValueError
    beyond 2^31 - 1 pairs."""
    return _brick_ranges(locs, shape, half, brick)[-1]


def plan_bricks(locs, shape, half, brick=BRICK):
    """CSR table of the T-bars each brick has to look at: (offsets int32 (bricks + 1,),
    index int32), bricks in C order of (brick z, brick y, brick x).  Brick b's list is
    index[offsets[b]:offsets[b + 1]]: every T-bar of `locs` ((N, 3) of (x, y, z), inside the
    volume with its cube) whose cube of half-width `half` meets the brick, in ascending j."""
    nb, n_bricks, n, lo, cnt, per, total = _brick_ranges(locs, shape, half, brick)
    j = np.repeat(np.arange(n, dtype=np.int64), per)
    local = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(per) - per, per)
    cy, cx = cnt[j, 1], cnt[j, 2]
    iz, rem = local // (cy * cx), local % (cy * cx)
    bid = ((lo[j, 0] + iz) * nb[1] + lo[j, 1] + rem // cx) * nb[2] + lo[j, 2] + rem % cx
    order = np.argsort(bid, kind='stable')
    offsets = np.zeros(n_bricks + 1, np.int64)
    np.cumsum(np.bincount(bid, minlength=n_bricks), out=offsets[1:])
    return offsets.astype(np.int32), j[order].astype(np.int32)


# ---- device path ---------------------------------------------------------------------------

is_device_tensor = _device.is_device_tensor


def _torch():
    return _device.require_torch('device write_labels_mask needs',
                                 'use device=None for the host path')


def torch_device(device):
    """torch.device of `device` (an int, or True for the runtime's default device);
    FplLabelsError if the library is not built"""
    _torch()
    return _device.torch_device(device, 'device write_labels_mask', _labelscapi.load_library)


def check_shape(shape):
    shape = tuple(int(d) for d in shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError('roi_mask must be a non-empty (Z, Y, X) volume, got shape %r' % (shape,))
    if int(np.prod(shape, dtype=np.int64)) > MAX_VOXELS:
        raise ValueError('a volume of %r voxels exceeds the 2^31 - 1 voxels the brick tables '
                         'can index; render it in parts' % (shape,))
    return shape


def roi_to_device(roi_mask, dev):
    """the resident uint8 roi_mask: a numpy uint8 array is uploaded once, a contiguous uint8
    tensor on `dev` (at any byte offset) is kept; anything else is refused by name"""
    torch = _torch()
    if is_device_tensor(roi_mask):
        if roi_mask.dtype != torch.uint8 or roi_mask.device != dev:
            raise ValueError('a resident roi_mask must be a uint8 tensor on %s, got %s on %s'
                             % (dev, roi_mask.dtype, roi_mask.device))
        if not roi_mask.is_contiguous():
            raise ValueError('a resident roi_mask must be contiguous (strides %r of shape %r)'
                             % (tuple(roi_mask.stride()), tuple(roi_mask.shape)))
        check_shape(roi_mask.shape)
        return roi_mask, 0
    if hasattr(roi_mask, 'is_cuda'):
        raise ValueError('roi_mask is a torch tensor on %s; device write_labels_mask takes a '
                         'numpy uint8 array or a uint8 tensor on %s' % (roi_mask.device, dev))
    roi_mask = np.asarray(roi_mask)
    if roi_mask.dtype != np.uint8:
        raise ValueError('device write_labels_mask takes a uint8 roi_mask, not %s (use the host '
                         'path, device=None)' % roi_mask.dtype)
    check_shape(roi_mask.shape)
    host = np.ascontiguousarray(roi_mask)
    if not host.flags.writeable:                 # torch wraps writable arrays only
        host = host.copy()
    return torch.from_numpy(host).to(dev), roi_mask.nbytes


def check_planner(planner, device=True):
    """ValueError, by name, for a planner that is not one of PLANNERS, and for the device
    planner without a device"""
    if planner not in PLANNERS:
        raise ValueError("planner %r: 'host' (labels.plan_bricks, numpy) or 'device' "
                         '(libfplplan.so)' % (planner,))
    if planner == 'device' and device is None:
        raise ValueError("planner='device' needs device=<int>: the host loop (device=None) "
                         'plans nothing')
    return planner


class _DevicePlan:
    """fplp_plan_bricks enqueued on a stream: the resident tables, the scratch that holds the
    status word and a pinned copy of that word, valid once the stream is synchronised"""

    def __init__(self, locs, shape, half, dev, stream):
        torch = _torch()
        self.n_index = plan_pairs(locs, shape, half)
        nb = brick_counts(shape)
        n_bricks = nb[0] * nb[1] * nb[2]
        nbytes = _plancapi.scratch_bytes(len(locs), n_bricks, self.n_index)
        self.tbars = torch.from_numpy(locs).to(dev) if len(locs) else None
        self.offsets = torch.empty(n_bricks + 1, dtype=torch.int32, device=dev)
        self.index = torch.empty(self.n_index, dtype=torch.int32, device=dev)
        self.scratch = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=dev)
        self.status = torch.empty(1, dtype=torch.int32, pin_memory=True)
        _plancapi.plan_bricks(0 if self.tbars is None else self.tbars.data_ptr(), len(locs),
                              shape, half, self.offsets.data_ptr(),
                              self.index.data_ptr() if self.n_index else 0, self.n_index,
                              self.scratch.data_ptr(), self.scratch.numel() * 4,
                              stream.cuda_stream)
        self.status.copy_(self.scratch[:1], non_blocking=True)

    def check(self):
        """after the stream's synchronise: FplPlanError unless the status word is 0"""
        if int(self.status[0]) != 0:
            raise _plancapi.FplPlanError(
                'fplp_plan_bricks: the device counted %d (T-bar, brick) pairs, plan_pairs %d; '
                'the index was not written' % (int(self.offsets[-1]), self.n_index))


def plan_bricks_device(locs, shape, half, device):
    """plan_bricks on the device (libfplplan.so): resident int32 (offsets, index) tensors, equal
    to plan_bricks's arrays byte for byte and complete when returned.  `locs`: the (N, 3)
    table of plan_tbars; `device`: an int, True (the runtime's default device) or a
    torch.device.  FplPlanError if the library is not built - no fallback to the host planner."""
    torch = _torch()
    if isinstance(device, torch.device):
        _plancapi.load_library()
        dev = device
    else:
        dev = _device.torch_device(device, 'device plan_bricks', _plancapi.load_library)
    shape = check_shape(shape)
    half = int(half)
    if half < 0 or half > _plancapi.MAX_RADIUS:
        raise ValueError('half %d must lie in [0, %d]' % (half, _plancapi.MAX_RADIUS))
    locs = np.array(np.asarray(locs).reshape(-1, 3), np.int32)        # a writable copy
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        plan = _DevicePlan(locs, shape, half, dev, stream)
        stream.synchronize()
    plan.check()
    return plan.offsets, plan.index


def labels_mask_device(locs, roi, radius_use, radius_ign, buffer_size, out=None, stats=None,
                       planner='host'):
    """libfpllabels.so's kernel on a resident contiguous uint8 `roi` and the (N, 3) table of
    plan_tbars: resident uint8 (labels, mask), complete when returned.  `out`: a pair of
    contiguous uint8 tensors to write into.  `stats`: a dict that receives the upload bytes
    of the tables and the planner's pair count.  `planner`: 'host' builds the brick table
    with plan_bricks and uploads it; 'device' uploads the T-bar table alone and builds the
    brick table with libfplplan.so on the stream of the labels kernel (one synchronise;
    FplPlanError if the status word it leaves is not 0)."""
    torch = _torch()
    check_planner(planner)
    ru, ri = _radii(radius_use, radius_ign)
    if max(ru, ri) > _labelscapi.MAX_RADIUS:
        raise ValueError('radius %d exceeds the %d the kernel takes' % (max(ru, ri),
                                                                       _labelscapi.MAX_RADIUS))
    if int(buffer_size) < 0:
        raise ValueError('buffer_size %r must not be negative' % (buffer_size,))
    shape = check_shape(roi.shape)
    dev = roi.device
    locs = _table(locs, shape, ru, ri)
    if planner == 'device':
        _plancapi.load_library()
    else:
        offsets, index = plan_bricks(locs, shape, max(ru, ri))
    if out is None:
        out = (torch.empty(shape, dtype=torch.uint8, device=dev),
               torch.empty(shape, dtype=torch.uint8, device=dev))
    labels, mask = out
    for t in (roi, labels, mask):
        if not (is_device_tensor(t) and t.dtype == torch.uint8 and t.device == dev
                and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError('labels_mask_device: contiguous uint8 roi / labels / mask of one '
                             'shape on one device')
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        if planner == 'device':
            plan = _DevicePlan(locs, shape, max(ru, ri), dev, stream)
            tables, pairs = [plan.tbars, plan.offsets, plan.index], plan.n_index
            table_bytes = int(locs.nbytes)
        else:
            plan = None
            tables = [torch.from_numpy(a).to(dev) if a.size else None
                      for a in (locs, offsets, index)]
            pairs = len(index)
            table_bytes = int(locs.nbytes + offsets.nbytes + index.nbytes)
        ptr = [0 if t is None or not t.numel() else t.data_ptr() for t in tables]
        if not pairs:
            ptr[1] = 0
        _labelscapi.labels_mask(roi.data_ptr(), ptr[0], len(locs), ptr[1], ptr[2], pairs,
                                shape, ru, ri, int(buffer_size), labels.data_ptr(),
                                mask.data_ptr(), stream.cuda_stream)
        stream.synchronize()
    if plan is not None:
        plan.check()
    if stats is not None:
        stats['table_bytes'] = table_bytes
        stats['pairs'] = int(pairs)
    return labels, mask


def write_labels_mask_device(tbars, roi_mask, radius_use, radius_ign, buffer_size, prefix, device,
                             planner='host'):
    """the device route of fplsynapses.write_labels_mask: resident uint8 (labels, mask); with
    `prefix` they are also downloaded and written as the host path writes them.  `planner`:
    as labels_mask_device; a missing libfplplan.so is reported before a missing GPU."""
    if check_planner(planner, device) == 'device':
        _plancapi.load_library()
    dev = torch_device(device)
    roi, _ = roi_to_device(roi_mask, dev)
    locs = plan_tbars(tbars, roi.shape, radius_use, radius_ign)
    labels, mask = labels_mask_device(locs, roi, radius_use, radius_ign, buffer_size,
                                      planner=planner)
    if prefix is not None:
        from . import keras_io
        ll, mm = labels.cpu().numpy(), mask.cpu().numpy()
        np.save('%s_labels.npy' % prefix, ll)
        np.save('%s_mask.npy' % prefix, mm)
        keras_io.write_main('%s_labels.h5' % prefix, ll)
        keras_io.write_main('%s_mask.h5' % prefix, mm)
    return labels, mask
