"""dedupe.py on the host: the numpy executor of the per-component merge against
rm_tbar_multi_pred(method='sparse') and 'dense' on every case of tests/merge_cases.py, with the
caps at their defaults and forced low; what sends a component to the host; the share of the
realistic list that goes there; the arguments solver='device' refuses; libfplmerge.so's C ABI and
build as far as they can be checked without a GPU."""
import inspect
import os
import re

import numpy as np
import pytest

from flypylib_amd import _mergecapi, _nearcapi, dedupe, fplpipeline, fplsynapses, near
from flypylib_amd.csrc import build
from tests import merge_cases as mc, near_cases, side_abi_cases as abi

ROOT = abi.ROOT
T = near_cases.T
CASES = mc.all_cases()
_SPARSE = {}


def _sparse(name):
    """method='sparse' of a case, computed once and left unchanged"""
    if name not in _SPARSE:
        tbars, kw = CASES[name]
        _SPARSE[name] = tuple(a.copy() for a in fplsynapses.rm_tbar_multi_pred(tbars, method='sparse', **kw))
    return _SPARSE[name]


def _same(got, want):
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


# ---- the executor ------------------------------------------------------------------------------

@pytest.mark.parametrize('caps', list(mc.CAPS))
@pytest.mark.parametrize('name', list(CASES))
def test_the_executor_gives_the_sparse_methods_arrays(name, caps):
    info = {}
    got = dedupe.merge_numpy(*mc.split(CASES[name]), info=info, **mc.CAPS[caps])
    _same(got, _sparse(name))
    assert sorted(info) == sorted(dedupe.INFO_KEYS) and all(type(v) is int for v in info.values())
    assert info['host_components'] >= (info['closure_rounds'] > 0)
    if caps == 'all 1':
        # no component of two points passes a component cap of 1: all of them run on the host
        assert info['host_components'] >= info['components']


@pytest.mark.parametrize('name', [n for n in CASES if len(CASES[n][0]['conf']) <= 600])
def test_the_executor_gives_the_dense_methods_arrays(name):
    tbars, kw = CASES[name]
    _same(dedupe.merge_numpy(*mc.split(CASES[name])), fplsynapses.rm_tbar_multi_pred(tbars, method='dense', **kw))


def test_the_closure_runs_several_rounds():
    rounds = {}
    for name in ('random 3000', 'random 3000, labelled'):
        for caps in mc.CAPS:
            info = {}
            dedupe.merge_numpy(*mc.split(CASES[name]), info=info, **mc.CAPS[caps])
            rounds[name, caps] = info['closure_rounds']
    assert max(rounds.values()) >= 3 and min(rounds.values()) >= 2, rounds


@pytest.mark.parametrize('name', list(mc.hand_made()))
def test_what_sends_a_component_to_the_host(name):
    tbars, kw, host = mc.hand_made()[name]
    info = {}
    dedupe.merge_numpy(*mc.split((tbars, kw)), info=info)
    if host is not None:
        assert info['host_components'] == host, info
    if name == 'a stranger in a ball':
        assert info['host_points'] == 3 and info['components'] == 1 and info['closure_rounds'] == 1
        rm = fplsynapses.rm_tbar_multi_pred(tbars, method='dense')[0]
        assert rm.tolist() == [False, True, True, False, False]       # the stranger goes with the pair
    if name == 'coincident strangers':
        assert info['host_points'] == 4 and len(near.pairs_numpy(tbars['locs'][2:4], T)[1]) == 0
    if name == 'candidates at the cap':
        assert info['largest'] == dedupe.CAND_CAP == 7
    if name.startswith('component'):
        n = len(tbars['conf'])
        assert info == dict(components=1, largest=n, sweeps=info['sweeps'], host_components=int(n > dedupe.COMP_CAP),
                            host_points=n * (n > dedupe.COMP_CAP), closure_rounds=int(n > dedupe.COMP_CAP))
        assert n - dedupe.COMP_CAP == (name == 'component over the cap')
    if name == 'a cluster of 300':
        assert info['largest'] == 300 and info['host_points'] == 300
    if name == 'neighbours of other labels only':
        mv = fplsynapses.rm_tbar_multi_pred(tbars, **kw)[1]
        assert mv.tolist() == [False, False, True, False, False]     # 0 and 1 have neighbours, none their own
    if name.startswith('N = '):
        assert info['host_points'] == 0 and info['sweeps'] == (0 if name == 'N = 0' else 1 + (name == 'N = 2'))


def test_a_point_that_does_not_come_to_rest_is_flagged_not_followed():
    """max_moves bounds the walk: with a bound of 1 a point that moves twice goes to the host"""
    tbars, kw = CASES['golden: chain_reaches_a_stranger']
    for moves, host in ((1, True), (dedupe.MAX_MOVES, True)):
        info = {}
        dedupe.merge_numpy(*mc.split((tbars, kw)), max_moves=moves, info=info)
        assert (info['host_components'] > 0) == host
    tb = {'locs': np.array([[0.0, 0, 0], [7.0, 0, 0], [3.0, 9, 0]]), 'conf': np.array([0.5, 0.75, 0.25])}
    info = {}
    dedupe.merge_numpy(tb['locs'], tb['conf'], np.zeros(3), T, max_moves=1, info=info)
    assert info['host_components'] == 0                              # it moves once and rests


def test_the_partition_is_the_connected_components():
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    for pts in (near_cases.random_integer(700, 3.0), near_cases.lattice(), near_cases.no_pair(3)):
        ip, ind = near.pairs_numpy(pts, T)
        comp, sweeps = dedupe.partition_numpy(ip, ind)
        n = len(pts)
        k, lab = connected_components(csr_matrix((np.ones(len(ind)), ind, ip), shape=(n, n)), directed=False)
        first = np.full(k, n)
        np.minimum.at(first, lab, np.arange(n))
        assert comp.dtype == np.int32 and np.array_equal(comp, first[lab]) and sweeps >= 1
    assert dedupe.partition_numpy(np.zeros(1, np.int64), np.zeros(0, np.int32))[1] == 0


def test_the_realistic_list_stays_off_the_host():
    """the condition the GPU test asserts of the device path as well: at most 5 % of the points
    that have neighbours run on the host (seed fixed after this was checked)"""
    tb, twice = mc.realistic()
    info = {}
    got = dedupe.merge_numpy(tb['locs'], tb['conf'], np.zeros(len(tb['conf'])), T, info=info)
    _same(got, _sparse('realistic'))
    ip, ind = near.pairs_numpy(tb['locs'], T)
    has = fplsynapses._sparse_rows(tb['locs'], ip, ind, T)[0]
    assert 2800 < len(tb['conf']) < 3200 and twice > 150 and (has > 0).sum() >= 2 * twice
    assert 0 < info['host_points'] <= 0.05 * (has > 0).sum(), (info, (has > 0).sum())
    assert info['components'] > 50 and 2 < info['largest'] <= dedupe.COMP_CAP


def test_the_loop_body_is_shared_with_the_host_method(monkeypatch):
    """_multi_pred_sparse and the closure run one body, fplsynapses._merge_visit"""
    seen = []
    real = fplsynapses._merge_visit
    monkeypatch.setattr(fplsynapses, '_merge_visit', lambda ii, *a, **k: seen.append(ii) or real(ii, *a, **k))
    tbars, kw = CASES['hand-made: a stranger in a ball']
    fplsynapses.rm_tbar_multi_pred(tbars, method='sparse')
    assert len(seen) == 1
    dedupe.merge_numpy(*mc.split((tbars, kw)))
    assert len(seen) == 2


# ---- the public surface ------------------------------------------------------------------------

def test_refusals():
    tb = near_cases.planted(50)
    with pytest.raises(ValueError, match="solver 'gpu'.*solver='host'.*solver='device'"):
        fplsynapses.rm_tbar_multi_pred(tb, solver='gpu')
    with pytest.raises(ValueError, match="solver='device' with method='sparse', device=None.*device=<int>"):
        fplsynapses.rm_tbar_multi_pred(tb, method='sparse', solver='device')
    with pytest.raises(ValueError, match="solver='device' with method='dense', device=None"):
        fplsynapses.rm_tbar_multi_pred(tb, solver='device')
    with pytest.raises(ValueError, match="needs method='sparse'"):
        fplsynapses.rm_tbar_multi_pred(tb, method='dense', device=0, solver='device')
    f32 = {'locs': tb['locs'], 'conf': tb['conf'].astype(np.float32)}
    with pytest.raises(ValueError, match="confidences are float32; use solver='host'"):
        fplsynapses.rm_tbar_multi_pred(f32, method='sparse', device=0, solver='device')
    for bad, what in (({'locs': tb['locs'].astype(np.float32), 'conf': tb['conf']}, 'locations are float32'),
                      ({'locs': tb['locs'].astype(np.int64) * 2 ** 20, 'conf': tb['conf']}, r'beyond 2\^24'),
                      ({'locs': tb['locs'], 'conf': tb['conf'].astype(np.int64)}, 'confidences are int64')):
        with pytest.raises(ValueError, match=what + ".*solver='host'"):
            fplsynapses.rm_tbar_multi_pred(bad, method='sparse', device=0, solver='device')
    with pytest.raises(ValueError, match="NaN label.*solver='host'"):
        fplsynapses.rm_tbar_multi_pred(tb, labels=np.full(50, np.nan), method='sparse', device=0, solver='device')
    for kw in ({'cand_cap': 8}, {'cand_cap': 0}, {'comp_cap': _mergecapi.COMP_CAP + 1}, {'max_moves': 0}):
        with pytest.raises(ValueError, match=r'must lie in \[1, '):
            dedupe.merge_numpy(tb['locs'], tb['conf'], np.zeros(50), T, **kw)
    # the defaults are unchanged and the pipeline passes the keyword on
    sig = inspect.signature(fplsynapses.rm_tbar_multi_pred).parameters
    assert [sig[k].default for k in ('method', 'device', 'solver', 'info')] == ['dense', None, 'host', None]
    sig = inspect.signature(fplpipeline.full_roi_inference).parameters
    assert sig['merge_solver'].default == 'host'
    assert inspect.signature(fplpipeline.merge_border_duplicates).parameters['solver'].default == 'host'
    with pytest.raises(ValueError, match="solver='device' with method='sparse', device=None"):
        fplpipeline.merge_border_duplicates(tb, 30, solver='device')


def test_label_codes_keep_equality():
    pts, conf = np.zeros((4, 3)), np.ones(4)
    for ll in (np.array([0.0, -0.0, 1.5, 1.5]), np.array([2 ** 63, 2 ** 63, 1, 1], np.uint64),
               np.array([-1, -1, 3, 3]), np.array([True, True, False, False]),
               np.array([0.5, 0.5, 2, 2], np.float32)):
        codes = dedupe.check_inputs(pts, conf, ll)[2]
        assert codes.dtype == np.int64
        assert np.array_equal(codes[:, None] == codes[None, :], ll[:, None] == ll[None, :])
    with pytest.raises(ValueError, match='no 64-bit code'):
        dedupe.check_inputs(pts, conf, np.array(['a', 'b', 'c', 'd']))


def test_a_missing_library_is_reported_before_a_missing_gpu(monkeypatch):
    tb = near_cases.planted(50)
    monkeypatch.setattr(_mergecapi._side, '_lib', None)
    monkeypatch.setattr(_mergecapi._side, 'path', '/nonexistent/libfplmerge.so')
    with pytest.raises(_mergecapi.FplMergeError, match='libfplmerge.so not found at /nonexistent') as e:
        fplsynapses.rm_tbar_multi_pred(tb, method='sparse', device=0, solver='device')
    assert 'python -m flypylib_amd.csrc.build' in str(e.value) and "solver='host'" in str(e.value)


# ---- the C ABI and the build -----------------------------------------------------------------------

def test_the_library_loads_and_the_constants_are_the_headers():
    assert _mergecapi.load_library().fplg_abi_version() == _mergecapi.ABI_VERSION
    assert _nearcapi.ABI_VERSION == 1                                # libfplnear.so's ABI is what it was
    hdr = open(os.path.join(ROOT, 'include', 'fplmerge.h')).read()
    for name in ('ABI_VERSION', 'BLOCK', 'MAX_BLOCKS', 'SCAN_THREADS', 'SOLVE_BLOCK', 'SOLVE_BLOCKS',
                 'CAND_CAP', 'COMP_CAP', 'MAX_MOVES'):
        assert int(re.search(r'#define FPLG_%s (\d+)' % name, hdr).group(1)) == getattr(_mergecapi, name), name
    assert dedupe.CAND_CAP == _mergecapi.CAND_CAP == 7 and dedupe.COMP_CAP <= _mergecapi.COMP_CAP
    assert dedupe.MAX_MOVES <= _mergecapi.MAX_MOVES
    src = open(os.path.join(abi.CSRC, 'merge', 'merge.hip')).read()
    assert 'CAPPED AT 7' in src                                      # the header says which way was chosen


def test_arguments_are_refused_before_the_gpu_is_touched():
    """every refusal here returns before a launch: no GPU is needed to see it"""
    c, err = _mergecapi, _mergecapi.FplMergeError
    assert c.scratch_bytes(1) == 16 and c.scratch_bytes(257) == 16 and c.scratch_bytes(3 * 256 + 1) == 24
    for bad in (0, -1, 2 ** 31):
        with pytest.raises(err, match=r'must lie in \[1, 2\^31 - 1\]'):
            c.scratch_bytes(bad)
    with pytest.raises(err, match='fplg_rows_count: null pointer'):
        c.rows_count(4096, 10, T, 8192, 8192, 5, 0, 8192, 8192, None)
    with pytest.raises(err, match='fplg_rows_count: t -1 must be finite and positive'):
        c.rows_count(4096, 10, -1.0, 8192, 8192, 5, 8192, 8192, 8192, None)
    with pytest.raises(err, match=r'fplg_rows_count: null pointer argument \(the columns\)'):
        c.rows_count(4096, 10, T, 8192, 0, 5, 8192, 8192, 8192, None)
    with pytest.raises(err, match='fplg_rows_count: a column is not aligned'):
        c.rows_count(4100, 10, T, 8192, 8192, 5, 8192, 8192, 8192, None)
    with pytest.raises(err, match='fplg_rows_fill: capacity -1 must lie in'):
        c.rows_fill(4096, 10, T, 8192, 8192, 5, 8192, -1, 8192, None)
    c.rows_fill(4096, 10, T, 8192, 8192, 5, 8192, 0, 0, None)          # capacity 0: no launch
    with pytest.raises(err, match='fplg_labels: max_sweeps 0 must be positive'):
        c.labels(8192, 8192, 10, 5, 8192, 8192, 8192, 0, None)
    with pytest.raises(err, match='fplg_labels: null pointer'):
        c.labels(8192, 8192, 10, 5, 8192, 0, 8192, 5, None)
    with pytest.raises(err, match='fplg_group_keys: a column is not aligned'):
        c.group_keys(8192, 8192, 8192, 10, 8196, None)
    with pytest.raises(err, match=r'fplg_boundaries: n 0 must lie in'):
        c.boundaries(8192, 0, 8192, None)
    with pytest.raises(err, match=r'fplg_boundaries: n \+ 1 flags exceed'):
        c.boundaries(8192, 2 ** 31 - 1, 8192, None)
    with pytest.raises(err, match='scratch of 8 bytes, fplg_scratch_bytes asks for 16'):
        c.flags_count(8192, 10, 8192, 8, None)
    with pytest.raises(err, match='the index array is not 4-byte aligned'):
        c.flags_fill(8192, 10, 8192, 16, 5, 8194, None)
    c.flags_fill(8192, 10, 8192, 16, 0, 0, None)                      # capacity 0: no launch

    def solve(**kw):
        a = dict(locs=4096, conf=4096, labels=4096, comp=4096, n=10, t=T, origin=(0.0, 0.0, 0.0),
                 cell=near.cell_side(T), dims=(4, 4, 4), keys=4096, order=4096, f_offsets=4096, f_indices=4096,
                 f_entries=5, members=4096, starts=4096, n_comp=3, cand_cap=7, comp_cap=128, max_moves=16,
                 rm=4096, mv=4096, mv_loc=4096, flagged=4096)
        a.update(kw)
        return c.solve(*a.values(), None)
    for kw, msg in (({'rm': 0}, 'fplg_solve: null pointer'), ({'n_comp': 11}, '11 components of 10 points'),
                    ({'cand_cap': 8}, r'cand_cap 8 must lie in \[1, 7\]'), ({'comp_cap': 0}, 'comp_cap 0 must lie in'),
                    ({'max_moves': 4097}, r'max_moves 4097 must lie in \[1, 4096\]'),
                    ({'cell': float(T)}, r'is below t \(1 \+ 2\^-20\)'), ({'dims': (4, 0, 4)}, 'cells along axis 1'),
                    ({'origin': (0.0, float('inf'), 0.0)}, 'origin is not finite'),
                    ({'dims': (2 ** 28, 2 ** 28, 2 ** 7)}, r'exceeds the 2\^62'),
                    ({'mv_loc': 4100}, 'a column is not aligned'), ({'t': 0.0}, 't 0 must be finite and positive')):
        with pytest.raises(err, match=msg):
            solve(**kw)


def test_the_kernels_do_not_spill():
    """what the compiler reports for the build's own flags: no spilled register, no scratch"""
    import shutil
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    if not shutil.which(build.HIPCC) and not os.path.exists(build.HIPCC):
        pytest.skip('hipcc not available')
    import kernel_resources
    res = kernel_resources.kernel_resources('merge/merge.hip')
    names = ('rows_count_kernel', 'rows_fill_kernel', 'init_labels_kernel', 'sweep_kernel', 'group_keys_kernel',
             'boundary_kernel', 'count_kernel', 'index_fill_kernel', 'solve_kernel', 'scan_kernel')
    assert len(res) == len(names) and all(any(n in k for k in res) for n in names), sorted(res)
    for name, v in res.items():
        assert v['vgpr_spill_count'] == 0 and v['sgpr_spill_count'] == 0, (name, v)
        assert v['private_segment_fixed_size'] == 0 and v['vgpr_count'] <= 128, (name, v)
    solve = next(v for k, v in res.items() if 'solve_kernel' in k)
    # 18 run bounds and 7 candidates per lane, 64 lanes, and the kernel's arguments
    columns = (18 + _mergecapi.CAND_CAP) * 4 * _mergecapi.SOLVE_BLOCK
    assert columns < solve['group_segment_fixed_size'] <= columns + 256


def test_no_atomics_at_all():
    src = open(os.path.join(abi.CSRC, 'merge', 'merge.hip')).read()
    code = re.sub(r'//.*', '', src)
    assert 'atomic' not in code.lower()
