"""Hard-example mining: the per-voxel loss of a prediction and the candidate tables of
gen_volume2, as numpy executors (the specification; the CPU tests' and the GPU tests'
oracle) and as the device path over libfplmine.so (include/fplmine.h).

`FplNetwork.voxel_loss(device=...)`, `fplobjdetect.write_sampling_weights(device=...)` and
`batchgen.Volume2Planner(tables='device')` are the public surface; this module is what they
call.  Nothing here falls back to the host when the library, torch or the GPU is missing.
"""
import numpy as np

from . import _device, _minecapi

MAX_VOXELS = _minecapi.MAX_VOXELS


def log32(x):
    """LOG32 of include/fplmine.h: the double-precision log of a float32, rounded once"""
    return np.log(np.asarray(x, np.float32).astype(np.float64)).astype(np.float32)


def _inside(shape, border):
    """True where a voxel is at least border[a] from both faces on every axis"""
    m = np.zeros(shape, bool)
    sl = tuple(slice(int(b), int(d) - int(b)) if int(d) - int(b) > int(b) else slice(0, 0)
               for d, b in zip(shape, border))
    m[sl] = True
    return m


def _clamp(loss, bounds, where):
    if bounds is None:
        return loss
    return np.minimum(np.maximum(loss, bounds[0] * where), bounds[1] * where)


def voxel_loss_numpy(pred, labels, mask, edge, l0_thresh=None, l1_thresh=None):
    """the arithmetic of FplNetwork.voxel_loss on a given prediction, with LOG32 in place of
    numpy's float32 log: float32 (Z,Y,X).  `edge`: the border per axis inside which no voxel
    has a loss (round(rf_size / 2) in FplNetwork.voxel_loss)."""
    pred = np.asarray(pred, np.float32)
    labels, mask = np.asarray(labels), np.asarray(mask)
    m = (mask == 1) & _inside(pred.shape, edge)
    neg = m & (labels == 0)
    l0 = np.zeros(pred.shape, np.float64)
    l0[neg] = -log32(np.maximum(np.float32(1) - pred[neg], np.float32(1e-8))).astype(np.float64)
    confident = neg & (l0 < 0.005)
    l0[confident] = 0
    l0 = _clamp(l0, l0_thresh, neg & ~confident)
    pos = m & (labels == 1)
    l1 = np.zeros(pred.shape, np.float64)
    l1[pos] = -log32(np.maximum(pred[pos], np.float32(1e-8))).astype(np.float64)
    l1 = _clamp(l1, l1_thresh, pos)
    return (l0 + l1).astype(np.float32)


def candidates_numpy(labels, mask, half, cc, weights=None):
    """(z, y, x int32 columns, float32 weights or None) of the voxels with labels == cc,
    mask == 1, inside the `half` border and - with weights - weights > 0, in C order: the
    rows `nonzero()` gives in gen_volume2 after `_volumes` has cleared the mask's border"""
    labels, mask = np.asarray(labels), np.asarray(mask)
    sel = (labels == cc) & (mask == 1) & _inside(labels.shape, half)
    if weights is not None:
        weights = np.asarray(weights)
        sel &= weights > 0
    idx = sel.nonzero()
    z, y, x = (a.astype(np.int32) for a in idx)
    return z, y, x, (None if weights is None else weights[idx].astype(np.float32))


# ---- device path ---------------------------------------------------------------------------

is_device_tensor = _device.is_device_tensor


def _torch():
    return _device.require_torch('device mining needs', 'use device=None for the host path')


def torch_device(device):
    """torch.device of `device` (an int, or True for the runtime's default device);
    FplMineError if the library is not built"""
    _torch()
    return _device.torch_device(device, 'device mining', _minecapi.load_library)


def classes_u8(a):
    """labels or a mask as uint8 voxels that compare like the original against 0 and 1: a
    value uint8 cannot hold becomes 2 instead of wrapping"""
    a = np.asarray(a)
    if a.dtype == np.uint8:
        return np.ascontiguousarray(a)
    if a.dtype == np.bool_:
        return np.ascontiguousarray(a).view(np.uint8)
    out = np.full(a.shape, 2, np.uint8)
    out[a == 0] = 0
    out[a == 1] = 1
    return out


def to_device_u8(a, dev):
    """a resident contiguous uint8 tensor of labels / a mask (uploaded once; kept if resident)"""
    torch = _torch()
    if is_device_tensor(a):
        if a.dtype != torch.uint8 or a.device != dev:
            raise ValueError('a resident labels / mask volume must be a uint8 tensor on %s, got '
                             '%s on %s' % (dev, a.dtype, a.device))
        return a.contiguous()
    return torch.from_numpy(classes_u8(a)).to(dev)


def to_device_f32(a, dev, what='weights'):
    torch = _torch()
    if is_device_tensor(a):
        if a.dtype != torch.float32 or a.device != dev:
            raise ValueError('resident %s must be a float32 tensor on %s, got %s on %s'
                             % (what, dev, a.dtype, a.device))
        return a.contiguous()
    a = np.asarray(a)
    if a.dtype != np.float32:
        raise ValueError('device mining takes float32 %s, not %s (use the host path)'
                         % (what, a.dtype))
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _check_volume(shape, *others):
    shape = tuple(int(d) for d in shape)
    if len(shape) != 3 or any(tuple(o.shape) != shape for o in others):
        raise ValueError('volumes must be 3-D and equal in shape: %r'
                         % ([shape] + [tuple(o.shape) for o in others],))
    if int(np.prod(shape, dtype=np.int64)) > MAX_VOXELS:
        raise ValueError('a volume of %r voxels exceeds the 2^31 - 1 voxels the mining kernels '
                         'index; mine it in parts' % (shape,))
    return shape


def voxel_loss_device(pred, labels, mask, edge, l0_thresh=None, l1_thresh=None, out=None):
    """libfplmine.so's voxel-loss kernel on resident tensors (float32 pred, uint8 labels and
    mask, one device): a float32 device tensor, complete when returned"""
    torch = _torch()
    shape = _check_volume(pred.shape, labels, mask)
    dev = pred.device
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    for t, dt in ((pred, torch.float32), (labels, torch.uint8), (mask, torch.uint8),
                  (out, torch.float32)):
        if not is_device_tensor(t) or t.dtype != dt or t.device != dev or not t.is_contiguous():
            raise ValueError('voxel_loss_device: contiguous float32 pred / loss and uint8 labels / '
                             'mask on one device')
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        _minecapi.voxel_loss(pred.data_ptr(), labels.data_ptr(), mask.data_ptr(), shape, edge,
                             l0_thresh, l1_thresh, out.data_ptr(), stream.cuda_stream)
        stream.synchronize()
    return out


def candidates_device(labels, mask, half, cc, weights=None, download=True):
    """libfplmine.so's compaction on resident tensors: (z, y, x, weights or None) as
    candidates_numpy gives them - numpy arrays (only the compacted rows are copied to the
    host), or device tensors with download=False"""
    torch = _torch()
    shape = _check_volume(labels.shape, mask, *(() if weights is None else (weights,)))
    dev = labels.device
    for t, dt in ((labels, torch.uint8), (mask, torch.uint8), (weights, torch.float32)):
        if t is not None and not (is_device_tensor(t) and t.dtype == dt and t.device == dev
                                  and t.is_contiguous()):
            raise ValueError('candidates_device: contiguous uint8 labels / mask and float32 '
                             'weights on one device')
    n = int(np.prod(shape, dtype=np.int64))
    nscr = _minecapi.scratch_bytes(n)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        scratch = torch.empty(nscr // 4, dtype=torch.int32, device=dev)
        wp = 0 if weights is None else weights.data_ptr()
        args = (labels.data_ptr(), mask.data_ptr(), wp, shape, half, cc, scratch.data_ptr(), nscr)
        total = _minecapi.candidates_count(*args, stream.cuda_stream)
        cols = torch.empty((3, total), dtype=torch.int32, device=dev)
        w = None if weights is None else torch.empty(total, dtype=torch.float32, device=dev)
        if total:
            _minecapi.candidates_fill(*args, total, cols[0].data_ptr(), cols[1].data_ptr(),
                                      cols[2].data_ptr(), 0 if w is None else w.data_ptr(),
                                      stream.cuda_stream)
        stream.synchronize()
    if not download:
        return cols[0], cols[1], cols[2], w
    host = cols.cpu().numpy()
    return host[0], host[1], host[2], (None if w is None else w.cpu().numpy())
