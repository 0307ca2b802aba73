"""Inputs shared by test_batchgen_plan.py (CPU) and test_gpu_batchgen.py (GPU): the five
configurations of tests/golden/training_generators.npz and larger seeded ones.  Below them,
the hand-made record tables of test_gpu_batchgen_records.py, which reach the gather kernel
through the C ABI with no planner and no random centre in between."""
import functools
import os

import numpy as np

from flypylib_amd import _batchcapi, batchgen, fplobjdetect, synth

GOLD_PATH = os.path.join(os.path.dirname(__file__), 'golden', 'training_generators.npz')
GOLD_CASES = [('batches', 3), ('batches_mask', 3), ('volume', 4), ('volume2', 3),
              ('volume2_noise', 3)]

# name -> (host generator, planner, arguments after train_data)
GOLD_MAKE = {
    'batches': ('gen_batches', batchgen.BatchesPlanner, ((12, 10, 10), 6), {}),
    'batches_mask': ('gen_batches', batchgen.BatchesPlanner, ((12, 12, 12), 4, True), {}),
    'volume': ('gen_volume', batchgen.VolumePlanner, ((24, 24, 24), 3, 0.5), {}),
    'volume2': ('gen_volume2', batchgen.Volume2Planner, ((24, 24, 24), 3, 0.5), {}),
    'volume2_noise': ('gen_volume2', batchgen.Volume2Planner, ((24, 24, 24), 2, 0.3),
                      {'noise_aug': [0.05, 0.1]}),
}


def training_volumes(seed, shape):
    """same inputs as test_training_data._training_volumes / make_golden.py"""
    im = synth.em_volume_u8(seed, shape).astype(np.float32)
    ll = (synth.hash_uniform_f32(seed + 100, shape) > np.float32(0.97)).astype(np.uint8)
    mm = np.ones(shape, np.uint8)
    mm[: shape[0] // 3, : shape[1] // 2, :] = 0
    return im, ll, mm


def golden_train_data(gold):
    return [training_volumes(int(seed), tuple(int(d) for d in shape))
            for shape, seed in zip(gold['shapes'], gold['vol_seeds'])]


BIG_SHAPES = [(72, 80, 88), (80, 72, 76), (76, 90, 72)]


def big_train_data(dtype, weighted=False, shapes=BIG_SHAPES):
    """three volumes of different shapes; `dtype` float32 (non-integral values, signed
    zeros included) or uint8; both classes present in every volume"""
    out = []
    for v, shape in enumerate(shapes):
        u8 = synth.em_volume_u8(70 + v, shape)
        if dtype == np.uint8:
            im = u8
        else:
            im = (u8.astype(np.float32) - np.float32(128)) / np.float32(33)
            im[::7, ::5, ::3] = np.float32(-0.0)
            im[1::7, ::5, ::3] = np.float32(0.0)
        ll = (synth.hash_uniform_f32(170 + v, shape) > np.float32(0.9)).astype(np.uint8)
        mm = np.ones(shape, np.uint8)
        mm[: shape[0] // 4, : shape[1] // 3, :] = 0
        tr = (im, ll, mm)
        if weighted:
            # small whole numbers (0..3): the generator normalises by a float32 sum, which
            # must be exact for numpy's choice() to accept the probabilities
            tr += (np.floor(synth.hash_uniform_f32(270 + v, shape) * np.float32(4)),)
        out.append(tr)
    return out


# name -> (host generator, planner, image dtype, weighted, args, kwargs, batches)
BIG_CASES = {
    'batches_f32': ('gen_batches', batchgen.BatchesPlanner, np.float32, False,
                    ((64, 64, 64), 32), {}, 4),
    'batches_u8': ('gen_batches', batchgen.BatchesPlanner, np.uint8, False,
                   ((64, 64, 64), 32), {}, 4),
    'batches_mask_f32': ('gen_batches', batchgen.BatchesPlanner, np.float32, False,
                         ((64, 64, 64), 32, True), {}, 4),
    'batches_mask_u8': ('gen_batches', batchgen.BatchesPlanner, np.uint8, False,
                        ((64, 64, 64), 32, True), {}, 4),
    'volume_f32': ('gen_volume', batchgen.VolumePlanner, np.float32, False,
                   ((24, 24, 24), 64, 0.5), {}, 3),
    'volume_u8': ('gen_volume', batchgen.VolumePlanner, np.uint8, False,
                  ((24, 24, 24), 64, 0.5), {}, 3),
    'volume2_noise_f32': ('gen_volume2', batchgen.Volume2Planner, np.float32, True,
                          ((24, 24, 24), 64, 0.6), {'noise_aug': [0.05, 0.1]}, 3),
    'volume2_noise_u8': ('gen_volume2', batchgen.Volume2Planner, np.uint8, True,
                         ((24, 24, 24), 64, 0.6), {'noise_aug': [0.05, 0.1]}, 3),
    'volume2_quiet_f32': ('gen_volume2', batchgen.Volume2Planner, np.float32, True,
                          ((24, 24, 24), 64, 0.6), {'noise_aug': [0, 0]}, 3),
    'volume2_quiet_u8': ('gen_volume2', batchgen.Volume2Planner, np.uint8, False,
                         ((24, 24, 24), 64, 0.6), {'noise_aug': [0, 0]}, 3),
    'noncubic_f32': ('gen_batches', batchgen.BatchesPlanner, np.float32, False,
                     ((12, 10, 10), 16, True), {}, 4),
    'noncubic_volume_u8': ('gen_volume', batchgen.VolumePlanner, np.uint8, False,
                           ((40, 34, 34), 8, 0.4), {}, 3),
}
BIG_SEED = 11


def host_generator(name, train, args, kw, rng, **extra):
    return getattr(fplobjdetect, name)(train, *args, rng=rng, **kw, **extra)


def combos(records, second_flip):
    """{(rot, second flip, flip of axis 0)} of a list of record arrays"""
    out = set()
    for rec in records:
        out |= set(zip(rec['rot'].tolist(), ((rec['flips'] & second_flip) != 0).tolist(),
                       ((rec['flips'] & 1) != 0).tolist()))
    return out


# ---------------------------------------------------------------------------------------------
# Hand-made record tables.  A record is a row of _batchcapi.RECORD written here by hand; the
# reference of every table is batchgen.execute_numpy (numpy's own rot90 and flip on the cut
# patch) on a RecordPlan.  Nothing below computes a source index.
# ---------------------------------------------------------------------------------------------

# three volumes, no axis a multiple of the kernel's 32-wide tile, each just large enough for
# the largest context (6 x 70 x 70) and for a 6^3 label block with one voxel to spare
RECORD_SHAPES = [(9, 75, 79), (7, 79, 71), (10, 71, 75)]
# the smallest context at which each path of the kernel exists: no tile at all, a patch
# smaller than the label block, one partial tile, exactly one tile, 2 x 2 tiles with a last
# row and column two voxels wide, 3 x 3 tiles (an interior one beside a partial row and
# column), and s1 != s2 (even rot only)
RECORD_CONTEXTS = [(2, 2, 2), (4, 4, 4), (6, 30, 30), (4, 32, 32), (6, 34, 34), (2, 66, 66),
                   (4, 34, 70), (4, 70, 34)]
# (context, label6, noise, image dtype) of every table: (2, 2, 2) labels its centre only
RECORD_CASES = [(c, l6, noise, dt) for c in RECORD_CONTEXTS for l6 in (False, True)
                for noise in (False, True) for dt in (np.float32, np.uint8)
                if not (l6 and c == (2, 2, 2))]


def case_id(case):
    c, l6, noise, dt = case
    return '%dx%dx%d-%s-%s-%s' % (c + ('labels6' if l6 else 'centre', 'noise' if noise else 'plain',
                                       np.dtype(dt).name))


@functools.lru_cache(maxsize=None)
def record_volumes(dtype):
    """[(image, labels)] of RECORD_SHAPES, read-only: uint8 images uniform over 0..255 from
    synth's hash generator, float32 ones (u8 - 128) / 33 with both signed zeros planted as
    big_train_data plants them, labels uniform over {0, 1, 2}"""
    out = []
    for v, shape in enumerate(RECORD_SHAPES):
        u8 = np.floor(synth.hash_uniform_f32(310 + v, shape) * np.float32(256)).astype(np.uint8)
        if np.dtype(dtype) == np.uint8:
            im = u8
        else:
            im = (u8.astype(np.float32) - np.float32(128)) / np.float32(33)
            im[::7, ::5, ::3] = np.float32(-0.0)
            im[1::7, ::5, ::3] = np.float32(0.0)
        ll = np.floor(synth.hash_uniform_f32(410 + v, shape) * np.float32(3)).astype(np.uint8)
        im.setflags(write=False)
        ll.setflags(write=False)
        out.append((im, ll))
    return out


class RecordPlan:
    """what execute_numpy and DeviceBatches read of a planner, around hand-made records"""
    host_name = 'none (hand-made records)'

    def __init__(self, context, label6, noise, dtype, records):
        vols = record_volumes(dtype)
        self.context_sz = tuple(context)
        self.half = tuple(c // 2 for c in context)
        self.images = [im for im, _ in vols]
        self.labels = [ll for _, ll in vols]
        self.noise, self.label6 = bool(noise), bool(label6)
        self.batch_sz = len(records)
        self._records = records

    def records(self):
        return self._records


def centre_range(context, label6, shape):
    """(lowest, highest) legal centre per axis: the patch [c - s/2, c + s/2) and, with
    label6, the label block [c - 3, c + 3) lie inside the volume"""
    reach = [max(c // 2, 3 if label6 else 0) for c in context]
    return reach, [d - r for d, r in zip(shape, reach)]


def transform_codes(context):
    """every (rot, flips) the header allows for the context - 32 for s1 == s2, the 16 of even
    rot otherwise - in Gray-code order, so that the parity of a record's position (which
    picks its corner) is the parity of all five bits and of no single one"""
    square = context[1] == context[2]
    out = []
    for n in range(32 if square else 16):
        g = n ^ (n >> 1)
        out.append((g >> 3 if square else 2 * (g >> 3), g & 7))
    return out


def record_table(context, label6, fixed=False):
    """one record per (rot, flips) of the context.  Record n is cut from volume n % 3 around
    the lowest (n even) or highest (n odd) legal centre on all three axes, so every patch -
    or, where half < 3 under label6, every label block - touches three faces of its volume.
    Multiplier and offset differ per record and are no float32 values.  fixed=True: volume 0,
    its lowest centre, mul 1 and add 0 throughout, so that only the transform differs."""
    codes = transform_codes(context)
    rec = np.zeros(len(codes), batchgen.RECORD)
    for n, (rot, flips) in enumerate(codes):
        vol = 0 if fixed else n % len(RECORD_SHAPES)
        lo, hi = centre_range(context, label6, RECORD_SHAPES[vol])
        z, y, x = lo if fixed or n % 2 == 0 else hi
        mul, add = (1.0, 0.0) if fixed else (0.9 + 0.013 * n, (n % 7 - 3) * 0.3)
        rec[n] = (vol, z, y, x, rot, flips, mul, add)
    return rec


@functools.lru_cache(maxsize=None)
def record_case(case):
    """(volumes, context, label6, noise, dtype, records) of one of RECORD_CASES"""
    context, label6, noise, dtype = case
    rec = record_table(context, label6)
    rec.setflags(write=False)
    return record_volumes(dtype), context, label6, noise, dtype, rec


def reference(context, label6, noise, dtype, records):
    """(data (B, s0*s1*s2) float32, labels (B, 216 or 1) uint8) by execute_numpy"""
    with np.errstate(over='ignore'):
        d, lab = batchgen.execute_numpy(RecordPlan(context, label6, noise, dtype, records), records)
    return d.reshape(len(records), -1), lab.reshape(len(records), -1)


@functools.lru_cache(maxsize=None)
def record_reference(case):
    """reference of one of RECORD_CASES, computed once and read-only"""
    _, context, label6, noise, dtype, rec = record_case(case)
    out = reference(context, label6, noise, dtype, rec)
    for a in out:
        a.setflags(write=False)
    return out


# (mul, add) of the noise table.  In order: identity; an offset of -0.0 (keeps a -0.0 voxel);
# a product of +-0 plus -0.0; negation; float32 denormals; overflow to infinity; a multiplier
# that float32 rounds to 1 (the float32 form loses it, the double form keeps v * 2^-30 until
# its single rounding); a multiplier just above the tie between 1 and 1 + 2^-23 (float32
# rounds it up, so rounding twice differs from rounding once); negation with the largest
# offset; and negation with -0.0, the one pair that gives a uint8 source a -0.0.
NOISE_PAIRS = [(1.0, 0.0), (1.0, -0.0), (0.0, -0.0), (-1.0, 0.0), (2.0 ** -130, 0.0), (1e38, 0.0),
               (1 + 2.0 ** -30, 2.0 ** -30), (1 + 2.0 ** -24 + 2.0 ** -40, 0.0), (-1.0, 255.0),
               (-1.0, -0.0)]
NOISE_CONTEXT = (4, 32, 32)


@functools.lru_cache(maxsize=None)
def noise_records():
    """one record per NOISE_PAIRS: rows 0, 7, 14, ... of the (4, 32, 32) table (corners
    alternate, all three volumes, both parities of rot) with that pair put in"""
    table = record_table(NOISE_CONTEXT, False)
    rec = table[[(7 * i) % len(table) for i in range(len(NOISE_PAIRS))]]
    rec['mul'] = [p[0] for p in NOISE_PAIRS]
    rec['add'] = [p[1] for p in NOISE_PAIRS]
    rec.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def noise_reference(dtype):
    out = reference(NOISE_CONTEXT, False, True, dtype, noise_records())
    for a in out:
        a.setflags(write=False)
    return out


# (context, label6) of the batches whose every other record must write nothing
SKIP_CASES = [((6, 34, 34), True), ((4, 4, 4), True), ((4, 34, 70), False)]
# the kinds of invalid record DeviceBatches._validate is not asked about: it does not look at
# the dtype, and a context with s1 != s2 is refused by the constructor
SKIP_NOT_VALIDATED = ('other dtype', 'odd rot')


@functools.lru_cache(maxsize=None)
def skip_records(context, label6):
    """(records, kinds): invalid records alternating with valid ones of the context's table,
    an invalid one first and last.  kinds[i] is 'valid' or what is wrong with record i.  The
    volume table these are run with has one entry more than RECORD_SHAPES: volume 0 once
    more, declared in the other dtype."""
    base = record_table(context, label6)
    nv = len(RECORD_SHAPES)
    bad = []

    def variant(kind, n, **fields):
        r = base[n % len(base)].copy()
        for k, v in fields.items():
            r[k] = v
        bad.append((kind, r))

    variant('vol -1', 1, vol=-1)
    variant('vol n_vols', 2, vol=nv + 1)
    variant('rot 4', 3, rot=4)
    variant('rot 255', 4, rot=255)
    variant('other dtype', 6, vol=nv, z=base[0]['z'], y=base[0]['y'], x=base[0]['x'])
    # one voxel outside the legal range on one axis, the other two at the lowest (even rows
    # of the table) or highest (odd rows) legal centre
    for corner in (0, 1):
        for a, axis in enumerate('zyx'):
            for side in (0, 1):
                n = (corner + 2 * (2 * a + side + 1)) % len(base)
                lo, hi = centre_range(context, label6, RECORD_SHAPES[n % nv])
                variant('%s %s' % (axis, 'below' if side == 0 else 'above'), n,
                        **{axis: lo[a] - 1 if side == 0 else hi[a] + 1})
    if label6 and min(context) < 6:
        # the patch fits - it touches three faces - and the 6^3 label block does not
        for n in (0, 1):
            lo, hi = centre_range(context, False, RECORD_SHAPES[n % nv])
            z, y, x = (lo, hi)[n]
            variant('label block outside', n, z=z, y=y, x=x)
    if context[1] != context[2]:
        variant('odd rot', 5, rot=1)
        variant('odd rot', 8, rot=3)
    rows, kinds = [], []
    for i, (kind, r) in enumerate(bad):
        rows += [r, base[(5 * i) % len(base)]]
        kinds += [kind, 'valid']
    rows.append(bad[0][1])
    kinds.append(bad[0][0])
    rec = np.zeros(len(rows), batchgen.RECORD)
    for i, r in enumerate(rows):
        rec[i] = r
    rec.setflags(write=False)
    return rec, tuple(kinds)


def inside(context, label6, rec, shapes):
    """per record: it names a volume of `shapes`, its rot is one the context allows, its patch
    lies inside that volume and so does what label6 reads - by slicing bounds, as
    execute_numpy would read them"""
    ok = np.zeros(len(rec), bool)
    for i, r in enumerate(rec):
        if not 0 <= r['vol'] < len(shapes) or r['rot'] > 3:
            continue
        if r['rot'] & 1 and context[1] != context[2]:
            continue
        c = (int(r['z']), int(r['y']), int(r['x']))
        h = [max(s // 2, 3 if label6 else 0) for s in context]
        ok[i] = all(0 <= cc - hh and cc + hh <= d for cc, hh, d in zip(c, h, shapes[r['vol']]))
    return ok
