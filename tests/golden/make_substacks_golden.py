"""Dev-time script (beside make_multi_pred_golden.py; never imported by the test-suite): runs the
REFERENCE's own fplsynapses.roi_to_substacks and get_substack_annotations on a small scene and
stores the scene and everything they print and write - data only - in
tests/golden/roi_to_substacks.npz.

    python tests/golden/make_substacks_golden.py

The reference is imported through _ref_import (inert stubs for its absent third-party modules).
Two of those stubs are replaced: DVIDNodeService by a fake node that serves arrays - grayscale,
labels, annotation elements, and the three ROI services answered by flypylib_amd.roi.BlockRoi -
and h5py.File by a recorder of what is written.  The fake's ROI semantics are this package's
own; everything else is pinned by the reference itself: the file names, the normalisation, the
coordinate flips, the labels and the mask.

The scene: a seeded uint8 volume of 48^3; an irregular ROI of 8-voxel blocks that reaches one
block below 0 and two blocks past 48 along x; partition_size 2 (cubes of 16), buffer_size 6,
radii 2 / 4; a uint64 segmentation; 40 annotations.  Three cubes are exported: one inside the
volume and partly outside the ROI, one that starts at x = -16, one past the volume's x face
that holds no annotation.

Keys: 'volume', 'seg', 'runs', 'block_size', 'partition_size', 'buffer_size', 'radius_use',
'radius_ign', 'image_normalize', 'locs', 'conf', 'ids', 'substacks' (size, z, y, x per cube),
'stats' (the printed lines), 'names' (every file written, sorted), 'json.<name>' (the text of a
json document), 'sha.<name>' (SHA-256 of dtype, shape and bytes of a float32 or uint64 volume),
'array.<name>' (a uint8 volume), 'annot.<id>.locs' / '.conf' (get_substack_annotations)."""
import contextlib
import hashlib
import io
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

BLOCK, PARTITION, BUFFER, RU, RI = 8, 2, 6, 2, 4
NORMALIZE = [135.0, 48.0]


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(('%s%r' % (a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def scene():
    from flypylib_amd.roi import BlockRoi
    rs = np.random.RandomState(140)
    volume = rs.randint(0, 256, (48, 48, 48)).astype(np.uint8)
    seg = np.repeat(np.repeat(np.repeat(rs.randint(1, 2 ** 40, (8, 8, 8)), 6, 0), 6, 1), 6, 2
                    ).astype(np.uint64)
    # blocks z, y in 0..5, x in -1..7: a ball with four blocks knocked out
    z, y, x = np.meshgrid(np.arange(6), np.arange(6), np.arange(-1, 8), indexing='ij')
    blocks = (z - 2.5) ** 2 + (y - 2.5) ** 2 + ((x - 3.0) * 0.75) ** 2 < 10.5
    for hole in ((2, 3, 2), (3, 2, 3), (0, 2, 3), (2, 2, 7)):
        blocks[hole[0], hole[1], hole[2] + 1] = False
    roi = BlockRoi.from_block_mask(blocks, origin=(0, 0, -1), block_size=BLOCK)
    subs = roi.partition(PARTITION)[0]
    side = PARTITION * BLOCK
    inside = next(i for i, s in enumerate(subs) if (s.z, s.y, s.x) == (16, 16, 16))
    below = next(i for i, s in enumerate(subs) if s.x < 0 and s.z == 16 and s.y == 16)
    past = next(i for i, s in enumerate(subs) if s.x == 48 and s.z == 16 and s.y == 16)
    ids = [inside, below, past]
    s = subs[inside]
    special = [
        (s.x, s.y + 3, s.z + 5), (s.x + 7, s.y, s.z + 9), (s.x + 9, s.y + 11, s.z),     # lowest faces
        (s.x + side - 1, s.y + side - 1, s.z + side - 1),                               # the last voxel
        (s.x + side, s.y + 4, s.z + 4), (s.x + 4, s.y + side, s.z + 4),                 # one past it
        (s.x + 4, s.y + 4, s.z + side), (s.x - 1, s.y + 2, s.z + 2),
    ]
    pts = list(special)
    for i in (inside, below):
        c = subs[i]
        pts += [(c.x + int(a), c.y + int(b), c.z + int(d)) for a, b, d in rs.randint(0, side, (14, 3))]
    # elsewhere in the volume, none of them in the cube past the x face
    pts += [(int(a), int(b), int(d)) for a, b, d in rs.randint(0, 48, (4, 3))]
    locs = np.asarray(pts, np.int64)
    conf = np.round(rs.rand(len(locs)) * 0.75 + 0.25, 3)
    c = subs[past]
    assert not np.any(np.all((locs >= [c.x, c.y, c.z]) & (locs < np.asarray([c.x, c.y, c.z]) + side), axis=1))
    return volume, seg, roi, locs, conf, ids


class FakeNode:
    """the DVIDNodeService of the scene: arrays in place of a server"""
    scene = None

    def __init__(self, *args):
        self.volume, self.seg, self.roi, self.locs, self.conf = FakeNode.scene

    @staticmethod
    def _cube(vol, dims, offset):
        out = np.zeros(tuple(dims), vol.dtype)
        lo = np.maximum(offset, 0)
        hi = np.minimum(np.asarray(offset) + np.asarray(dims), vol.shape)
        if np.all(hi > lo):
            src = tuple(slice(a, b) for a, b in zip(lo, hi))
            dst = tuple(slice(a - o, b - o) for a, b, o in zip(lo, hi, offset))
            out[dst] = vol[src]
        return out

    def get_roi_partition(self, name, partition_size):
        return self.roi.partition(partition_size)

    def get_roi3D(self, name, dims, offset):
        return self.roi.roi3D(dims, offset)

    def roi_ptquery(self, name, pts):
        return [bool(v) for v in self.roi.ptquery(np.asarray(pts, np.int64).reshape(-1, 3))]

    def get_gray3D(self, name, dims, offset):
        return self._cube(self.volume, dims, offset)

    def get_labels3D(self, name, dims, offset):
        return self._cube(self.seg, dims, offset)

    def custom_request(self, endpoint, payload, method):
        _, what, size, offset = endpoint.split('/')
        assert what == 'elements'
        size = np.asarray([int(v) for v in size.split('_')])
        lo = np.asarray([int(v) for v in offset.split('_')])
        keep = np.all((self.locs >= lo) & (self.locs < lo + size), axis=1)
        if not keep.any():
            return b'null'
        return json.dumps([{'Kind': 'PreSyn', 'Pos': p.tolist(), 'Prop': {'conf': repr(float(c))}}
                           for p, c in zip(self.locs[keep], self.conf[keep])]).encode()


class FakeFile:
    """h5py.File as far as the reference uses it: create_dataset, hh['/main'][:] = array, close"""
    written = {}

    def __init__(self, name, mode):
        assert mode == 'w'
        self.name, self.sets = name, {}

    def create_dataset(self, key, shape, dtype=None, compression=None):
        self.sets[key.lstrip('/')] = np.zeros(shape, dtype)

    def __getitem__(self, key):
        return self.sets[key.lstrip('/')]

    def close(self):
        assert list(self.sets) == ['main']
        FakeFile.written[os.path.basename(self.name)] = self.sets['main']


def main():
    from _ref_import import import_reference
    import_reference()
    from flypylib import fplsynapses as ref
    volume, seg, roi, locs, conf, ids = scene()
    FakeNode.scene = (volume, seg, roi, locs, conf)
    ref.DVIDNodeService = FakeNode
    ref.h5py.File = FakeFile
    store = {'volume': volume, 'seg': seg, 'runs': roi.runs, 'block_size': np.array(BLOCK),
             'partition_size': np.array(PARTITION), 'buffer_size': np.array(BUFFER),
             'radius_use': np.array(RU), 'radius_ign': np.array(RI),
             'image_normalize': np.asarray(NORMALIZE), 'locs': locs, 'conf': conf,
             'ids': np.asarray(ids)}
    subs = roi.partition(PARTITION)[0]
    store['substacks'] = np.asarray([(s.size, s.z, s.y, s.x) for s in subs], np.int64)

    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        ref.roi_to_substacks('server', 'uuid', 'roi', 'synapses', PARTITION)
    store['stats'] = np.asarray(printed.getvalue().splitlines())

    with tempfile.TemporaryDirectory() as data_dir, contextlib.redirect_stdout(io.StringIO()):
        ref.roi_to_substacks('server', 'uuid', 'roi', 'synapses', PARTITION, data_dir=data_dir,
                             substack_ids=ids, image_normalize=NORMALIZE, buffer_size=BUFFER,
                             radius_use=RU, radius_ign=RI, seg_name='segmentation')
        names = sorted(os.listdir(data_dir))
        for name in names:
            store['json.' + name] = np.asarray(open(os.path.join(data_dir, name)).read())
    for name, arr in FakeFile.written.items():
        names.append(name)
        if arr.dtype == np.uint8:
            store['array.' + name] = arr
        else:
            store['sha.' + name] = np.asarray(sha(arr))
    store['names'] = np.asarray(sorted(names))
    node = FakeNode()
    for ii in ids:
        tt = ref.get_substack_annotations(node, 'roi', 'synapses', subs[ii])
        store['annot.%d.locs' % ii] = np.asarray(tt['locs'], np.int64).reshape(-1, 3)
        store['annot.%d.conf' % ii] = np.asarray(tt['conf'], np.float64).reshape(-1)
    np.savez_compressed(os.path.join(HERE, 'roi_to_substacks.npz'), **store)
    print('\n'.join(store['stats'].tolist()))
    print('exported', ids, [tuple(subs[i]) for i in ids])
    print('\n'.join(store['names'].tolist()))
    for ii in ids:
        print(ii, 'annotations', len(store['annot.%d.conf' % ii]))


if __name__ == '__main__':
    main()
