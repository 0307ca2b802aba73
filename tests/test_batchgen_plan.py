"""Plan / execute split of the training batch generators (flypylib_amd/batchgen.py) and the
C ABI of libfplbatch.so - host logic, no GPU.  The host generators of fplobjdetect.py are
the oracle (pinned to the reference by tests/golden/training_generators.npz)."""
import hashlib
import os
import re

import numpy as np
import pytest

from flypylib_amd import _batchcapi, batchgen, fplobjdetect
from tests import batchgen_cases as cases

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


# ---- the hand-made record tables of tests/test_gpu_batchgen_records.py ----------------------

def _tables():
    return [(c, l6) for c in cases.RECORD_CONTEXTS for l6 in (False, True)
            if not (l6 and c == (2, 2, 2))]


def test_record_tables_name_every_transform_once_at_corner_centres():
    """what the GPU tests take for granted of the tables: every (rot, flips) the header allows
    once, all three volumes, every centre legal, and every patch (label block where it is the
    larger) against three faces of its volume - the lowest and the highest in turn"""
    for context, label6 in _tables():
        rec = cases.record_table(context, label6)
        square = context[1] == context[2]
        codes = set(zip(rec['rot'].tolist(), rec['flips'].tolist()))
        assert codes == {(r, f) for r in range(0, 4, 1 if square else 2) for f in range(8)}
        assert len(rec) == len(codes) == (32 if square else 16)
        assert rec['vol'].tolist() == [n % 3 for n in range(len(rec))]
        assert cases.inside(context, label6, rec, cases.RECORD_SHAPES).all()
        for n, r in enumerate(rec):
            shape = cases.RECORD_SHAPES[r['vol']]
            for c, s, d in zip((r['z'], r['y'], r['x']), context, shape):
                h = max(s // 2, 3 if label6 else 0)
                assert (c - h == 0) if n % 2 == 0 else (c + h == d), (context, label6, n)
        # the corner is tied to no single bit of (rot, flips)
        for bit in (1, 2, 4):
            assert len({(n % 2, bool(r['flips'] & bit)) for n, r in enumerate(rec)}) == 4
        assert len({(n % 2, int(r['rot'])) for n, r in enumerate(rec)}) == 2 * len(set(rec['rot']))
    for shape in cases.RECORD_SHAPES:
        assert all(d % 32 for d in shape)
    for dtype in (np.float32, np.uint8):
        vols = cases.record_volumes(dtype)
        assert [im.shape for im, _ in vols] == cases.RECORD_SHAPES
        assert all(im.dtype == dtype and ll.dtype == np.uint8 for im, ll in vols)
        assert all(set(np.unique(ll)) == {0, 1, 2} for _, ll in vols)


@pytest.mark.parametrize('case', cases.RECORD_CASES, ids=cases.case_id)
def test_record_table_references_hold_no_nan(case):
    """the GPU tests fill their buffers with a NaN and take a word that still holds it for
    unwritten: no reference may hold one"""
    data, labels = cases.record_reference(case)
    _, context, label6, _, _, rec = cases.record_case(case)
    assert data.shape == (len(rec), context[0] * context[1] * context[2])
    assert labels.shape == (len(rec), 216 if label6 else 1)
    assert not np.isnan(data).any() and labels.max() <= 2


def _distinct(a):
    return len({row.tobytes() for row in a})


@pytest.mark.parametrize('context', cases.RECORD_CONTEXTS)
def test_the_transforms_of_a_table_are_all_distinct_on_these_images(context):
    """rot90 and the three flips generate a group of 16 elements (8 without the odd
    rotations) which the 32 (16) values of (rot, flips) name twice each.  Around one fixed
    centre the reference outputs are exactly that many distinct examples, so no two different
    transforms coincide on these images and a kernel that applied the wrong one would not
    match by chance."""
    want = 16 if context[1] == context[2] else 8
    for label6 in ((False,) if context == (2, 2, 2) else (False, True)):
        rec = cases.record_table(context, label6, fixed=True)
        assert (rec['mul'] == 1).all() and (rec['add'] == 0).all()
        assert len({(int(r['vol']), int(r['z']), int(r['y']), int(r['x'])) for r in rec}) == 1
        for dtype in (np.float32, np.uint8):
            data, labels = cases.reference(context, label6, False, dtype, rec)
            assert len(data) == 2 * want and _distinct(data) == want, (context, label6, dtype)
            assert _distinct(labels) == (want if label6 else 1)


def test_noise_table_reference_holds_every_class_of_result():
    """denormals, both zeros, infinities - and, from a uint8 source, values at which rounding
    the multiplier and the product to float32 on the way (the float32 source's form) differs
    from rounding once at the end: that is what tells the kernel's double path from its float
    path"""
    rec = cases.noise_records()
    assert list(zip(rec['mul'].tolist(), rec['add'].tolist())) == cases.NOISE_PAIRS
    assert np.float32(2.0 ** -130) != 0 and np.isfinite(np.float32(1e38))
    tiny = np.finfo(np.float32).tiny
    for dtype in (np.float32, np.uint8):
        data, _ = cases.noise_reference(dtype)
        assert not np.isnan(data).any()
        counts = {'denormal': int(((data != 0) & (np.abs(data) < tiny)).sum()),
                  '+0.0': int(((data == 0) & ~np.signbit(data)).sum()),
                  '-0.0': int(((data == 0) & np.signbit(data)).sum()),
                  'inf': int(np.isinf(data).sum())}
        print(np.dtype(dtype).name, counts)
        assert all(n > 0 for n in counts.values()), (dtype, counts)
    # float32 source: both signed zeros go in
    for im, _ in cases.record_volumes(np.float32):
        zeros = im[im == 0]
        assert np.signbit(zeros).any() and not np.signbit(zeros).all()
    # uint8 source: the same records computed the float32 source's way
    data, _ = cases.noise_reference(np.uint8)
    one = cases.reference(cases.NOISE_CONTEXT, False, False, np.uint8,
                          cases.noise_records())[0]        # the transformed voxels themselves
    with np.errstate(over='ignore'):
        two = (rec['mul'].astype(np.float32)[:, None] * one
               + rec['add'].astype(np.float32)[:, None])
    assert two.dtype == np.float32
    differ = (two.view(np.uint32) != data.view(np.uint32)).sum(1)
    print('uint8 source, values per record at which two roundings differ from one:',
          differ.tolist())
    assert differ[cases.NOISE_PAIRS.index((1 + 2.0 ** -24 + 2.0 ** -40, 0.0))] > 0
    assert differ[0] == 0                                   # (1, 0): nothing to round


def test_skip_tables_alternate_valid_records_with_ones_one_voxel_outside():
    """test_gpu_batchgen_records.py expects the kernel to skip exactly the records marked
    invalid here.  For those that are invalid by their centre that marking is checked against
    plain bounds: outside by one voxel on one axis, inside once moved back by it."""
    shapes = cases.RECORD_SHAPES + [cases.RECORD_SHAPES[0]]        # the other-dtype entry
    for context, label6 in cases.SKIP_CASES:
        rec, kinds = cases.skip_records(context, label6)
        assert kinds[0] != 'valid' and kinds[-1] != 'valid'
        assert all((k == 'valid') == (i % 2 == 1) for i, k in enumerate(kinds))
        ok = cases.inside(context, label6, rec, shapes)
        for i, kind in enumerate(kinds):
            assert ok[i] == (kind in ('valid', 'other dtype')), (context, i, kind)
            if kind.split()[0] in 'zyx' and kind.split()[1] in ('below', 'above'):
                axis, side = kind.split()
                back = rec[i:i + 1].copy()
                back[axis] += 1 if side == 'below' else -1
                assert cases.inside(context, label6, back, shapes).all(), (context, i, kind)
            if kind == 'label block outside':
                assert cases.inside(context, False, rec[i:i + 1], shapes).all()
        want = {'vol -1', 'vol n_vols', 'rot 4', 'rot 255', 'other dtype'}
        want |= {'%s %s' % (a, s) for a in 'zyx' for s in ('below', 'above')}
        if context == (4, 4, 4):
            want.add('label block outside')
        if context[1] != context[2]:
            want.add('odd rot')
        assert set(kinds) - {'valid'} == want
        assert sum(k.split()[-1] in ('below', 'above') for k in kinds) == 12


_DUMMY = 4096        # a non-null pointer that is never dereferenced: every call below is refused


@pytest.mark.parametrize('kw,message', [
    (dict(batch=0), r'batch 0 \(1\.\.65535\)'),
    (dict(batch=65536), r'batch 65536 \(1\.\.65535\)'),
    (dict(n_vols=0), r'n_vols 0, batch 1'),
    (dict(context=(8, 7, 8)), r'context \(8,7,8\) must be even'),
    (dict(context=(8, 8, 0)), r'context \(8,8,0\) must be even, 2\.\.4096'),
    (dict(context=(4098, 8, 8)), r'context \(4098,8,8\) must be even, 2\.\.4096'),
    (dict(label_mode=2), r'label_mode 2'),
    (dict(src_dtype=2), r'src_dtype 2 \(FPLB_U8 or FPLB_F32\)'),
])
def test_gather_refuses_before_any_launch(kw, message):
    a = dict(n_vols=1, batch=1, context=(8, 8, 8), src_dtype=_batchcapi.F32, label_mode=0)
    a.update(kw)
    with pytest.raises(_batchcapi.FplBatchError, match=message):
        _batchcapi.gather(_DUMMY, a['n_vols'], _DUMMY, a['batch'], a['context'], a['src_dtype'],
                          False, a['label_mode'], _DUMMY, _DUMMY, 0)
