"""Inputs shared by the resident-segmentation tests (tests/test_gpu_seg_resident.py on the GPU,
tests/test_seg_resident_host.py on the CPU): a small label volume of odd, unequal extents, the
boxes cut out of it and the predictions post-processed against it.

Why these shapes.  The fill kernel (csrc/v2o.hip: seg_pad_box) gives a thread 4 consecutive
padded voxels and stores them as two 16-byte pairs, the last partial group voxel by voxel:
  * padded dims (16,18,19), (18,18,18), (17,18,19), (33,29,39) -> n_pad 5472, 5832, 5814, 37323:
    none a multiple of 256 (a partial last workgroup), the last two no multiple of 4 (the scalar
    tail) and the last one odd (it ends on half a pair);
  * the rows are 19 / 18 / 39 voxels: a thread's group straddles rows, and planes;
  * origin x = 20 with 13 columns in a 29-column volume: the volume's x edge falls inside a pair.
"""
import numpy as np

EXTENT = (23, 19, 29)
R = 3
BOX_A, BOX_B, BOX_C, BOX_BIG = (10, 12, 13), (12, 12, 12), (11, 12, 13), (27, 23, 33)
# (name, origin (z, y, x), dims)
BOXES = [(name + tag, origin, dims)
         for tag, dims in (('_a', BOX_A), ('_b', BOX_B))
         for name, origin in (('inside', (5, 3, 7)), ('out_low', (-4, -4, -4)),
                              ('out_high', (15, 10, 20)), ('face_z', (23, 3, 7)),
                              ('face_x', (5, 3, 29)), ('disjoint', (40, -30, 35)))]
BOXES.append(('larger_than_the_volume', (-2, -2, -2), BOX_BIG))
BOXES.append(('inside_c', (5, 3, 7), BOX_C))            # n_pad = 2 mod 4
BOXES.append(('out_high_c', (15, 10, 20), BOX_C))
# voxel2obj parity: the boxes that meet the volume in more than a sliver
V2O_BOXES = [b for b in BOXES if b[0].split('_')[0] in ('inside', 'out') or b[0].startswith('larger')]

V2O_KW = dict(obj_min_dist=R, smoothing_sigma=1.0, thd=0.05)
SEG_KW = dict(seg_dilate=2, seg_sz_thd=150, seg_force=1)


def _mix(k):
    with np.errstate(over='ignore'):
        k = (k ^ (k >> np.uint64(33))) * np.uint64(0xff51afd7ed558ccd)
        k = (k ^ (k >> np.uint64(33))) * np.uint64(0xc4ceb9fe1a85ec53)
        return k ^ (k >> np.uint64(33))


def label_volume(dtype, extent=EXTENT, block=(6, 5, 7)):
    """blocks of (z // 6, y // 5, x // 7) hashed to `dtype`; two voxels are planted so that the
    volume holds a value >= 2^32 (8-byte types) and one with the top bit set (every type)"""
    dtype = np.dtype(dtype)
    z, y, x = np.meshgrid(*(np.arange(e, dtype=np.uint64) for e in extent), indexing='ij')
    key = ((z // np.uint64(block[0])) << np.uint64(40)) | ((y // np.uint64(block[1])) << np.uint64(20)) \
        | (x // np.uint64(block[2]))
    lab = _mix(key + np.uint64(1))
    bits = 8 * dtype.itemsize
    if bits == 32:
        lab &= np.uint64(0xffffffff)
    lab[0, 0, 0] = np.uint64(1) << np.uint64(bits - 1) | np.uint64(5)       # top bit set
    lab[-1, -1, -1] = (np.uint64(1) << np.uint64(32)) + np.uint64(1) if bits == 64 else np.uint64(7)
    unsigned = lab.astype(np.dtype('u%d' % dtype.itemsize))
    out = unsigned.view(dtype) if dtype.kind == 'i' else unsigned.astype(dtype)
    assert int(unsigned.max()) >> (bits - 1) == 1
    assert bits == 32 or (unsigned >= np.uint64(1) << np.uint64(32)).any()
    return np.ascontiguousarray(out)


def host_cut(vol, origin, dims):
    """the (dims) box at `origin` of `vol`, zeros outside it - `_ArraySource.cube_host` for a box
    of any dims; all zeros where the box misses the volume"""
    origin, dims = np.asarray(origin), np.asarray(dims)
    lo = np.maximum(origin, 0)
    hi = np.minimum(origin + dims, vol.shape)
    out = np.zeros(tuple(dims), vol.dtype)
    if np.all(hi > lo):
        out[tuple(slice(a - o, b - o) for a, b, o in zip(lo, hi, origin))] = \
            vol[tuple(slice(a, b) for a, b in zip(lo, hi))]
    return out


def padded_u64(cut, r=R):
    """what the padded segmentation must hold: the cut widened to u64 (two's complement for the
    signed types, as the kernels' cast) in a zero shell of r"""
    u = cut.view(np.dtype('u%d' % cut.dtype.itemsize)) if cut.dtype.kind == 'i' else cut
    return np.pad(u.astype(np.uint64), r, 'constant')


def prediction(dims, kind, seed=4):
    """random smoothed blobs of shape `dims`: float32, float64, or int32 (scaled by 1000)"""
    from flypylib_amd import synth
    p = synth.blob_prob_volume(seed, tuple(dims), period=5, radius=1.6, noise=0.02)
    if kind == 'float32':
        return np.ascontiguousarray(p, np.float32)
    if kind == 'float64':
        return np.ascontiguousarray(p, np.float64) * 0.999
    return np.ascontiguousarray(np.asarray(p, np.float64) * 1000).astype(np.int32)


def prediction_thd(kind):
    return V2O_KW['thd'] * (1000 if kind == 'int32' else 1)
