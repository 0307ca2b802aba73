"""Hard-example mining, host side (no GPU): the C ABI of libfplmine.so, and the numpy
executors of flypylib_amd/mine.py against the code they specify - FplNetwork.voxel_loss and
the nonzero()-built candidate tables of gen_volume2."""
import os
import re

import numpy as np
import pytest

from flypylib_amd import FplNetwork, _minecapi, batchgen, fplobjdetect, mine
from tests import batchgen_cases as cases, side_abi_cases as abi
from tests.mine_cases import mining_case as _mining_case, ulp_distance as _ulp_distance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_EXPORTS = 5


def test_libfplmine_exports_exactly_the_declared_names():
    declared = abi.check_exports(_minecapi, 'fplmine.h', 'fplm', N_EXPORTS)
    assert not any(n.startswith(('fpl_', 'fplb_')) for n in declared)


def test_the_other_libraries_keep_their_export_lists():
    """the mining entry points live in a library of their own"""
    for hdr in ('fplhip.h', 'fplbatch.h'):
        assert 'fplm_' not in open(os.path.join(ROOT, 'include', hdr)).read()
    csrc = os.path.join(ROOT, 'flypylib_amd', 'csrc')
    for f in os.listdir(csrc):
        if f.endswith(('.hip', '.h')):
            assert 'fplm_' not in open(os.path.join(csrc, f)).read(), f


def test_every_fplm_entry_point_is_guarded():
    abi.check_guarded('mine', 'fplmine.h', 'fplm', N_EXPORTS)


def test_refused_calls_leave_a_message_and_touch_no_gpu():
    lib = _minecapi.load_library()
    assert lib.fplm_abi_version() == _minecapi.ABI_VERSION
    hdr = open(os.path.join(ROOT, 'include', 'fplmine.h')).read()
    assert int(re.search(r'#define FPLM_ABI_VERSION (\d+)', hdr).group(1)) == _minecapi.ABI_VERSION
    assert int(re.search(r'#define FPLM_CHUNK (\d+)', hdr).group(1)) == _minecapi.CHUNK
    assert _minecapi.scratch_bytes(1) == 8 and _minecapi.scratch_bytes(4096) == 8
    assert _minecapi.scratch_bytes(4097) == 12
    with pytest.raises(_minecapi.FplMineError, match='fplm_voxel_loss: null pointer'):
        _minecapi.voxel_loss(0, 0, 0, (8, 8, 8), (1, 1, 1), None, None, 0, 0)
    with pytest.raises(_minecapi.FplMineError, match='fplm_candidates_count: null pointer'):
        _minecapi.candidates_count(0, 0, 0, (8, 8, 8), (1, 1, 1), 0, 0, 0, 0)
    with pytest.raises(_minecapi.FplMineError, match='fplm_candidates_fill: null pointer'):
        _minecapi.candidates_fill(0, 0, 0, (8, 8, 8), (1, 1, 1), 0, 0, 0, 4, 0, 0, 0, 0, 0)
    # a volume int32 rows cannot index is refused by name before any pointer is followed
    # (the addresses below are never dereferenced: 2048 x 1024 x 1024 = 2^31 voxels)
    with pytest.raises(_minecapi.FplMineError, match=r'exceeds the 2\^31 - 1 voxels'):
        _minecapi.candidates_count(256, 256, 0, (2048, 1024, 1024), (1, 1, 1), 0, 256, 1 << 40, 0)
    with pytest.raises(_minecapi.FplMineError, match=r'exceeds the 2\^31 - 1 voxels'):
        _minecapi.voxel_loss(256, 256, 256, (2048, 1024, 1024), (1, 1, 1), None, None, 256, 0)
    with pytest.raises(_minecapi.FplMineError, match='scratch of 4 bytes'):
        _minecapi.candidates_count(256, 256, 0, (8, 8, 8), (1, 1, 1), 0, 256, 4, 0)
    with pytest.raises(_minecapi.FplMineError, match='edge .* must not be negative'):
        _minecapi.voxel_loss(256, 256, 256, (8, 8, 8), (1, -1, 1), None, None, 256, 0)


@pytest.mark.parametrize('thresholds', [(None, None), ((0.8, 1.0), None), (None, (0.1, 0.5)),
                                        ((0.05, 2.0), (0.1, 0.5))])
def test_voxel_loss_numpy_is_the_host_formula_up_to_numpys_float32_log(thresholds):
    """FplNetwork.voxel_loss (numpy's float32 log) and mine.voxel_loss_numpy (LOG32: the
    double log rounded once) on one prediction.  They differ only by the error of numpy's
    float32 log; the bound is measured on this test's own log arguments, not fixed:
    d = max ulp distance(np.log(x), LOG32(x)), and d + 1 ulp is allowed on non-zero losses
    (+ 1: a clamp bound or the final rounding may sit between the two).  A voxel whose host
    l0 lies within d + 1 ulp of 0.005 may be zeroed by one and not the other: left out, at
    most 1e-4 of the voxels."""
    shape = (40, 44, 52)
    pred, ll, mm = _mining_case(5, shape)
    net = FplNetwork.__new__(FplNetwork)
    net.rf_size = (6, 6, 8)
    edge = [int(round(c / 2)) for c in net.rf_size]
    net.infer = lambda image, normalize=None: pred
    host = net.voxel_loss(None, (ll, mm), *thresholds)
    got = mine.voxel_loss_numpy(pred, ll, mm, edge, *thresholds)
    assert got.dtype == np.float32 and got.shape == shape and host.dtype == np.float32

    args = np.concatenate([np.maximum(1 - pred, np.float32(1e-8)).ravel(),
                           np.maximum(pred, np.float32(1e-8)).ravel()])
    d = int(_ulp_distance(np.log(args), mine.log32(args)).max())
    tol = d + 1
    print('numpy float32 log vs LOG32 on %d arguments: max %d ulp' % (args.size, d))

    l0_host = -np.log(np.maximum(1 - pred, np.float32(1e-8)))
    near = _ulp_distance(l0_host, np.full(shape, 0.005, np.float32)) <= tol
    near &= (ll == 0) & (mm == 1)
    left_out = int(near.sum())
    print('voxels within %d ulp of the 0.005 cut: %d of %d' % (tol, left_out, pred.size))
    assert left_out <= 1e-4 * pred.size
    keep = ~near
    assert np.array_equal(got[keep] == 0, host[keep] == 0)
    dist = _ulp_distance(got[keep], host[keep])
    print('max distance on kept voxels: %d ulp' % int(dist.max()))
    assert int(dist.max()) <= tol
    assert (got != 0).sum() > 0.3 * pred.size and (got == 0).sum() > 0.1 * pred.size
    # the rf border has no loss
    assert not got[:edge[0]].any() and not got[:, :, -edge[2]:].any()


def test_voxel_loss_numpy_on_the_hand_derived_values():
    """the values of test_training_data.test_voxel_loss_formula_and_sampling_weight_files"""
    shape = (10, 10, 10)
    pred = np.full(shape, 0.5, np.float32)
    ll = np.zeros(shape, np.uint8)
    mm = np.ones(shape, np.uint8)
    pred[5, 5, 5], ll[5, 5, 5] = 0.25, 1
    pred[5, 5, 6] = 0.001
    pred[5, 6, 5] = 0.9
    pred[4, 5, 5], pred[4, 5, 6], ll[4, 5, 6] = 1.0, 0.0, 1     # the 1e-8 floor, both classes
    mm[6, 5, 5] = 0
    got = mine.voxel_loss_numpy(pred, ll, mm, (2, 2, 2))
    assert abs(got[5, 5, 5] - (-np.log(0.25))) < 1e-6
    assert got[5, 5, 6] == 0 and got[6, 5, 5] == 0
    assert abs(got[5, 6, 5] - (-np.log(0.1))) < 1e-6
    assert got[4, 5, 5] == np.float32(-np.log(np.float64(np.float32(1e-8)))) == got[4, 5, 6]
    assert not got[:2].any() and not got[:, :, -2:].any()
    clamped = mine.voxel_loss_numpy(pred, ll, mm, (2, 2, 2), (0.8, 1.0), (0.1, 0.5))
    assert clamped[5, 6, 5] == 1.0 and clamped[4, 4, 4] == np.float32(0.8)
    assert clamped[5, 5, 5] == 0.5 and clamped[5, 5, 6] == 0


def _nonzero_tables(vols, cc, weighted):
    """the tables as _gen_volume2_host builds them, per volume"""
    out = []
    for im, ll, mm, ww in vols:
        sel = (ll == cc) & (mm == 1)
        if weighted:
            sel &= ww > 0
        idx = sel.nonzero()
        out.append(tuple(a.astype(np.int32) for a in idx) + ((ww[idx] if weighted else None),))
    return out


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('context', [(24, 24, 24), (40, 34, 34)])
def test_candidates_numpy_equals_the_nonzero_tables(weighted, context):
    train = cases.big_train_data(np.float32, weighted)
    half = tuple(c // 2 for c in context)
    vols = fplobjdetect._volumes(train, half)
    for cc in range(2):
        want = _nonzero_tables(vols, cc, weighted)
        for tr, w in zip(train, want):
            z, y, x, ww = mine.candidates_numpy(tr[1], tr[2], half, cc,
                                                tr[3] if weighted else None)
            assert all(a.dtype == np.int32 for a in (z, y, x)) and len(z) > 0
            assert np.array_equal(z, w[0]) and np.array_equal(y, w[1]) and np.array_equal(x, w[2])
            if weighted:
                assert ww.dtype == np.float32 and np.array_equal(ww, w[3]) and (ww > 0).all()
            else:
                assert ww is None


def test_candidates_numpy_edge_cases():
    shape = (9, 10, 11)
    ll = np.zeros(shape, np.uint8)
    mm = np.ones(shape, np.uint8)
    z, y, x, w = mine.candidates_numpy(ll, mm, (0, 0, 0), 0)
    assert len(z) == 9 * 10 * 11 and w is None
    assert len(mine.candidates_numpy(ll, mm, (0, 0, 0), 1)[0]) == 0
    assert len(mine.candidates_numpy(ll, mm, (5, 1, 1), 0)[0]) == 0      # border beyond the centre
    z, y, x, _ = mine.candidates_numpy(ll, mm, (4, 4, 5), 0)
    assert (z.tolist(), sorted(set(y.tolist())), x.tolist()) == ([4, 4], [4, 5], [5, 5])


@pytest.mark.parametrize('name', ['volume2_noise_f32', 'volume2_quiet_u8'])
def test_volume2_planner_with_injected_tables_yields_todays_records(name):
    _, planner, dtype, weighted, args, kw, n = cases.BIG_CASES[name]
    train = cases.big_train_data(dtype, weighted)
    r0, r1 = (np.random.RandomState(cases.BIG_SEED) for _ in range(2))
    today = planner(train, *args, rng=r0, **kw)
    injected = planner(train, *args, rng=r1, tables=mine.candidates_numpy, **kw)
    for i in range(n):
        a, b = today.records(), injected.records()
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (name, i)
    assert r0.rand() == r1.rand()
    for a, b in zip(today.labels, injected.labels):
        assert np.array_equal(a, b)


def test_new_arguments_default_to_todays_behaviour_and_refuse_misuse():
    shape = (30, 30, 30)
    im = np.zeros(shape, np.float32)
    ll = np.zeros(shape, np.uint8)
    ll[15, 15, 15] = 1
    mm = np.ones(shape, np.uint8)
    with pytest.raises(ValueError, match='needs device'):
        fplobjdetect.gen_volume2([(im, ll, mm)], (24, 24, 24), 2, 0.5, tables='device')
    with pytest.raises(ValueError, match='needs device'):
        fplobjdetect.write_sampling_weights([(im, ll, mm)], None, 'w', None, None, save=False)
    with pytest.raises(ValueError, match="None, 'device' or a callable"):
        batchgen.Volume2Planner([(im, ll, mm)], (24, 24, 24), 2, 0.5, tables='host')
    assert batchgen.volume2_tables([(im, ll, mm)], None) is None
    assert batchgen.volume2_tables([(im, ll, mm)], 'device') == 'device'
    # uint8 stand-ins of labels / masks of another dtype compare like the original
    a = np.array([0, 1, 2, 256, 257, -1], np.int64)
    assert mine.classes_u8(a).tolist() == [0, 1, 2, 2, 2, 2]
    assert mine.classes_u8(np.array([True, False])).tolist() == [1, 0]
