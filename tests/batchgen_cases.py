"""Inputs shared by test_batchgen_plan.py (CPU) and test_gpu_batchgen.py (GPU): the five
configurations of tests/golden/training_generators.npz and larger seeded ones."""
import os

import numpy as np

from flypylib_amd import batchgen, fplobjdetect, synth

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
