"""Plan / execute split of the training batch generators (flypylib_amd/batchgen.py) and the
C ABI of libfplbatch.so - host logic, no GPU.  The host generators of fplobjdetect.py are
the oracle (pinned to the reference by tests/golden/training_generators.npz)."""
import hashlib
import os
import re

import numpy as np
import pytest

from flypylib_amd import _batchcapi, batchgen, fplobjdetect
from tests import batchgen_cases as cases, side_abi_cases as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('name,n', cases.GOLD_CASES)
def test_plan_and_numpy_executor_match_the_reference_outputs(name, n):
    """same volumes, context sizes, batch sizes and global-numpy seeds as
    test_training_data.test_generators_match_the_reference_outputs"""
    gold = np.load(cases.GOLD_PATH)
    _, planner, args, kw = cases.GOLD_MAKE[name]
    np.random.seed(int(gold['%s_seed' % name]))
    plan = planner(cases.golden_train_data(gold), *args, **kw)      # rng=None: numpy's global one
    for i in range(n):
        d, lab = batchgen.execute_numpy(plan, plan.records())
        assert d.dtype == np.float32 and lab.dtype == np.uint8
        assert np.array_equal(lab, gold['%s_labels_%d' % (name, i)]), (name, i)
        if i == 0:
            assert np.array_equal(d[0, ..., 0], gold['%s_example0' % name]), name
        got = hashlib.sha256(np.ascontiguousarray(d).tobytes()).hexdigest()
        assert got == str(gold['%s_data_sha_%d' % (name, i)]), (name, i)


@pytest.mark.parametrize('name', sorted(cases.BIG_CASES))
def test_plan_and_numpy_executor_equal_the_host_generator_byte_for_byte(name):
    host, planner, dtype, weighted, args, kw, n = cases.BIG_CASES[name]
    train = cases.big_train_data(dtype, weighted)
    r_host, r_plan = (np.random.RandomState(cases.BIG_SEED) for _ in range(2))
    gen = cases.host_generator(host, train, args, kw, r_host)
    plan = planner(train, *args, rng=r_plan, **kw)
    for i in range(n):
        d0, l0 = next(gen)
        d1, l1 = batchgen.execute_numpy(plan, plan.records())
        assert d0.shape == d1.shape and l0.shape == l1.shape
        assert d0.dtype == d1.dtype and l0.dtype == l1.dtype
        assert np.ascontiguousarray(d0).tobytes() == d1.tobytes(), (name, i)
        assert np.ascontiguousarray(l0).tobytes() == l1.tobytes(), (name, i)
    assert r_host.rand() == r_plan.rand()           # the same rng calls were made


def test_float32_inputs_carry_signed_zeros_through_the_noise_arithmetic():
    """what makes tobytes() stricter than array_equal in the test above is present"""
    host, planner, dtype, weighted, args, kw, n = cases.BIG_CASES['volume2_quiet_f32']
    plan = planner(cases.big_train_data(dtype, weighted), *args,
                   rng=np.random.RandomState(cases.BIG_SEED), **kw)
    d, _ = batchgen.execute_numpy(plan, plan.records())
    zeros = d[d == 0]
    assert zeros.size and np.signbit(zeros).any() and not np.signbit(zeros).all()


@pytest.mark.parametrize('name', ['batches_mask_f32', 'volume_f32', 'volume2_noise_f32'])
def test_record_streams_cover_all_sixteen_augmentations(name):
    _, planner, dtype, weighted, args, kw, n = cases.BIG_CASES[name]
    plan = planner(cases.big_train_data(dtype, weighted), *args,
                   rng=np.random.RandomState(cases.BIG_SEED), **kw)
    recs = [plan.records() for _ in range(n)]
    got = cases.combos(recs, plan.second_flip)
    assert got == {(r, a, b) for r in range(4) for a in (False, True) for b in (False, True)}
    assert plan.second_flip == (_batchcapi.FLIP_AXIS1 if name.startswith('volume2')
                                else _batchcapi.FLIP_AXIS2)


def test_records_are_the_c_struct():
    assert _batchcapi.RECORD.itemsize == 40 and _batchcapi.VOLUME.itemsize == 32
    lib = _batchcapi.load_library()              # checks both sizes against the library
    assert lib.fplb_abi_version() == _batchcapi.ABI_VERSION
    hdr = open(os.path.join(ROOT, 'include', 'fplbatch.h')).read()
    assert int(re.search(r'#define FPLB_ABI_VERSION (\d+)', hdr).group(1)) == _batchcapi.ABI_VERSION
    # a refused call leaves the reason behind fplb_last_error (no GPU is touched: the
    # arguments are checked first)
    with pytest.raises(_batchcapi.FplBatchError, match='null pointer'):
        _batchcapi.gather(0, 1, 0, 1, (8, 8, 8), _batchcapi.F32, False, 0, 0, 0, 0)


def test_libfplbatch_exports_exactly_the_declared_names():
    declared = abi.check_exports(_batchcapi, 'fplbatch.h', 'fplb', 4)
    assert not any(n.startswith('fpl_') for n in declared)


def test_every_fplb_entry_point_is_guarded():
    abi.check_guarded('batchgen', 'fplbatch.h', 'fplb', 4)


def test_device_mode_refuses_what_it_does_not_take():
    shape = (40, 40, 40)
    im = np.zeros(shape, np.float64)
    ll = np.zeros(shape, np.uint8)
    ll[18:22, 18:22, 18:22] = 1
    mm = np.ones(shape, np.uint8)
    for make in (lambda: fplobjdetect.gen_batches([(im, ll, mm)], (24, 24, 24), 4, device=0),
                 lambda: fplobjdetect.gen_volume([(im, ll, mm)], (24, 24, 24), 4, 0.5, device=0),
                 lambda: fplobjdetect.gen_volume2([(im, ll, mm)], (24, 24, 24), 4, 0.5, device=0)):
        with pytest.raises(ValueError, match=r'float32 or uint8 images, not float64.*host generator '
                                             r'fplobjdetect\.gen_'):
            make()
    # a class without centres in some volume: the host path re-augments stale rows
    empty = np.zeros(shape, np.uint8)
    with pytest.raises(ValueError, match='volume 1 has no unmasked voxel of class 1'):
        fplobjdetect.gen_batches([(im.astype(np.float32), ll, mm),
                                  (im.astype(np.float32), empty, mm)], (24, 24, 24), 4, device=0)
    # ... while the host generator still takes both (device=None is today's behaviour)
    d, lab = next(fplobjdetect.gen_batches([(im, empty, mm)], (24, 24, 24), 4,
                                           rng=np.random.RandomState(0)))
    assert d.shape == (4, 24, 24, 24, 1) and lab.shape == (4, 1, 1, 1, 1)
    # gen_volume's fallback to class 0 is host logic in the planner, not a refusal
    plan = batchgen.VolumePlanner([(im.astype(np.float32), empty, mm)], (24, 24, 24), 4, 0.0,
                                  rng=np.random.RandomState(0))
    assert len(plan.records()) == 4
