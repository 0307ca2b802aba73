"""Hard-example mining, host side (no GPU): the C ABI of libfplmine.so, and the numpy
executors of flypylib_amd/mine.py against the code they specify - FplNetwork.voxel_loss and
the nonzero()-built candidate tables of gen_volume2."""
import os
import re

import numpy as np
import pytest

from flypylib_amd import FplNetwork, _minecapi, batchgen, fplobjdetect, mine
from tests import batchgen_cases as cases
from tests import mine_cases
from tests.mine_cases import mining_case as _mining_case, ulp_distance as _ulp_distance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_other_libraries_keep_their_export_lists():
    """the mining entry points live in a library of their own"""
    for hdr in ('fplhip.h', 'fplbatch.h'):
        assert 'fplm_' not in open(os.path.join(ROOT, 'include', hdr)).read()
    csrc = os.path.join(ROOT, 'flypylib_amd', 'csrc')
    for f in os.listdir(csrc):
        if f.endswith(('.hip', '.h')):
            assert 'fplm_' not in open(os.path.join(csrc, f)).read(), f


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


# ---- preflight of tests/test_gpu_mine.py's large and short-row cases -----------------------

def test_the_named_constants_are_the_kernels():
    src = open(os.path.join(ROOT, 'flypylib_amd', 'csrc', 'mine', 'mine.hip')).read()
    for name, value in (('BLOCK', mine_cases.BLOCK), ('LANE_VOX', mine_cases.LANE_VOX),
                        ('SCAN_THREADS', mine_cases.SCAN_THREADS)):
        assert int(re.search(r'constexpr int %s = (\d+);' % name, src).group(1)) == value
    assert re.search(r'std::min\(\(groups \+ BLOCK - 1\) / BLOCK, (\d+)u\)', src).group(1) \
        == str(mine_cases.LOSS_GRID_CAP)
    assert mine_cases.CHUNK == _minecapi.CHUNK == 4096
    assert mine_cases.PASS_VOXELS == 2097152


def test_every_scan_shape_reaches_its_path():
    """n_chunks, per, the last thread with a run and that run's length, and the passes of the
    loss grid, derived from the kernels' constants: a GPU test on one of these shapes cannot
    pass by missing the path it is named for"""
    lay = {n: mine_cases.scan_layout(s) for n, (s, _) in mine_cases.SCAN_SHAPES.items()}
    threads = mine_cases.SCAN_THREADS

    a = lay['scan_full']
    assert (a['voxels'], a['n_chunks'], a['per']) == (4194304, 1024, 1)
    assert (a['last_thread'], a['last_run'], a['last_chunk_voxels']) == (threads - 1, 1, 4096)

    b = lay['scan_one_over']
    assert (b['voxels'], b['n_chunks'], b['per']) == (4194305, 1025, 2)
    assert (b['last_thread'], b['last_run'], b['last_chunk_voxels']) == (512, 1, 1)
    # threads 513 .. 1023: lo = min(t * per, n_chunks) is n_chunks, the run is empty
    assert all(min(t * b['per'], b['n_chunks']) == b['n_chunks'] for t in range(513, threads))
    assert mine_cases.SCAN_SHAPES['scan_one_over'][0][1:] == (1, 1)      # a group spans four planes

    c = lay['scan_runs_2']
    assert (c['voxels'], c['n_chunks'], c['per']) == (5358675, 1309, 2)
    assert (c['last_thread'], c['last_run']) == (654, 1)
    assert c['groups'] == 1339669 and c['passes'] == 3
    assert c['groups'] % (mine_cases.LOSS_GRID_CAP * mine_cases.BLOCK) != 0     # the last pass is partial
    assert c['voxels'] % 4 == 3 and mine_cases.SCAN_SHAPES['scan_runs_2'][0][2] % 2 == 1

    d = lay['scan_runs_3']
    assert (d['voxels'], d['n_chunks'], d['per']) == (10217445, 2495, 3)
    assert (d['last_thread'], d['last_run']) == (831, 2)

    for n, l in lay.items():
        # the layout is the kernel's: every chunk in exactly one run, runs in order
        runs = [(min(t * l['per'], l['n_chunks']), min(min(t * l['per'], l['n_chunks']) + l['per'],
                                                      l['n_chunks'])) for t in range(threads)]
        assert runs[0][0] == 0 and all(p[1] == q[0] for p, q in zip(runs, runs[1:])), n
        assert runs[l['last_thread']] == (l['n_chunks'] - l['last_run'], l['n_chunks']), n
        assert all(lo == hi for lo, hi in runs[l['last_thread'] + 1:]), n
        assert l['voxels'] <= _minecapi.MAX_VOXELS


@pytest.mark.parametrize('name,half,cc', mine_cases.COMPACTION_CASES)
def test_every_run_of_the_scan_cases_holds_candidates(name, half, cc):
    _, ll, mm, ww = mine_cases.scan_case(name, cc)
    shape = mine_cases.SCAN_SHAPES[name][0]
    assert any(half) or name == 'scan_one_over'
    for weights in (None, ww):
        z, y, x, w = mine.candidates_numpy(ll, mm, half, cc, weights)
        held, runs = mine_cases.assert_runs_hold_candidates(name, half, weights is not None, z, y, x)
        print('%s half %r class %d %s: %d rows, %d of %d runs must hold rows'
              % (name, half, cc, 'weighted' if w is not None else 'unweighted', len(z), held, runs))
        assert runs == mine_cases.scan_layout(shape)['last_thread'] + 1
        if name == 'scan_one_over' and not any(half):
            n = shape[0]
            assert (z[0], z[-1]) == (0, n - 1) and (w is None or (w[0], w[-1]) == (0.25, 0.25))
    # every third plane has no weight (but scan_one_over's forced voxel 0), one weight is NaN
    assert np.isnan(ww).sum() == 1 and not ww[3::3].any()
    assert (ll == 3).any() and (mm == 2).any()


def test_the_short_row_cases_select_what_they_are_named_for():
    assert len(mine_cases.SHORT_ROW_CASES) == len(mine_cases.SHORT_ROW_INSIDE) == 7
    for (shape, border), inside in zip(mine_cases.SHORT_ROW_CASES, mine_cases.SHORT_ROW_INSIDE):
        ll, mm = np.zeros(shape, np.uint8), np.ones(shape, np.uint8)
        z, y, x, _ = mine.candidates_numpy(ll, mm, border, 0)
        assert len(z) == inside, (shape, border)
        loss = mine.voxel_loss_numpy(np.full(shape, 0.5, np.float32), ll, mm, border)
        assert int((loss != 0).sum()) == inside, (shape, border)
        if inside == 1:
            assert (z[0], y[0], x[0]) == tuple(d // 2 for d in shape)
    # four of them have rows shorter than a group of four
    assert sum(s[2] < mine_cases.LANE_VOX for s, _ in mine_cases.SHORT_ROW_CASES) == 4


def test_the_off_unit_case_and_what_the_specification_makes_of_it():
    """np.maximum keeps a NaN, so a NaN prediction gives a NaN loss under either label, with
    and without thresholds; every other planted value gives a number"""
    pred, ll, mm = mine_cases.off_unit_case()
    nan = np.isnan(pred)
    assert nan.sum() == 4 and set(ll[nan].tolist()) == {0, 1}
    for v in mine_cases.OFF_UNIT[1:]:
        assert set(ll[pred == np.float32(v)].tolist()) >= {0, 1}, v
    floor = np.float32(-np.log(np.float64(np.float32(1e-8))))
    with np.errstate(all='ignore'):
        free = mine.voxel_loss_numpy(pred, ll, mm, (0, 0, 0))
        clamped = mine.voxel_loss_numpy(pred, ll, mm, (0, 0, 0), (0.05, 2.0), (0.1, 0.5))
    for loss in (free, clamped):
        assert np.array_equal(np.isnan(loss), nan)
    # label 0 at x = 0, 2, ..: +inf -> floor, -inf -> confident, -0.25 -> confident, 1.5 -> floor
    assert free[4, 5, 2] == floor and free[4, 5, 4] == 0 and free[4, 5, 6] == 0
    assert free[4, 5, 8] == floor and free[4, 5, 10] == floor
    # label 1 at x = 1, 3, ..: +inf -> -inf, -inf -> floor, -0.25 -> floor, 1.5 -> -log 1.5, 1 -> 0
    assert free[4, 5, 3] == -np.inf and free[4, 5, 5] == floor and free[4, 5, 7] == floor
    assert free[4, 5, 9] == np.float32(-np.log(1.5)) and free[4, 5, 11] == 0
    assert clamped[4, 5, 2] == 2.0 and clamped[4, 5, 3] == np.float32(0.1)
    assert clamped[4, 5, 9] == np.float32(0.1) and clamped[4, 5, 11] == np.float32(0.1)
