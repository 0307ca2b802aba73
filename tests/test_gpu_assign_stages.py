"""libfplassign.so on the GPU, stage by stage and at the sizes tests/test_gpu_assign.py does not
reach: the ordered compaction called through the binding on lists of up to 2 050 cells (scan
runs of 2 and 3 cells, capacity below the total, flags of any non-zero value, every output
alone and all together), the element-wise kernels beyond one grid stride, the labelling on
long and unordered graphs, and the solver on sparse components of up to 64 x 64 points,
compared matrix for matrix.  Every reference is numpy / scipy on the host;
tests/test_assign_host.py proves, without a GPU, that each input is what its test needs."""
import numpy as np
import pytest

from flypylib_amd import _assigncapi, match
from tests import assign_cases as ac
from tests.test_gpu_assign import _check_matching

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

T = ac.T
SENTINEL = -77777                # of the int32 outputs, no value of any column or index
SENTINEL_C = -777.25             # of the float64 output
PAD = 64                         # entries allocated behind every output: they keep the sentinel
OUTPUTS = ('a_out', 'b_out', 'c_out', 'index_out', 'rank_out')
INPUT_OF = {'a_out': 'a', 'b_out': 'b', 'c_out': 'c'}


# ---- 1. the ordered compaction, through the binding ------------------------------------------------

class _Gpu:
    """torch tensors around the binding's raw addresses, on the stream current at construction"""

    def __init__(self):
        import torch
        self.torch = torch
        self.dev = match.torch_device(0)
        self.stream = torch.cuda.current_stream(self.dev)
        self.st = self.stream.cuda_stream
        self._columns = {}

    def up(self, array):
        return self.torch.from_numpy(np.array(array, order='C')).to(self.dev)

    def full(self, n, value, dtype=None):
        return self.torch.full((n,), value, dtype=dtype or self.torch.int32, device=self.dev)

    def down(self, tensor):
        self.stream.synchronize()
        return tensor.cpu().numpy()

    def columns(self, n):
        """compaction_columns(n), uploaded once"""
        if n not in self._columns:
            self._columns[n] = dict(zip('abc', (self.up(v) for v in ac.compaction_columns(n))))
        return self._columns[n]

    def scratch(self, n):
        nscr = _assigncapi.scratch_bytes(n)
        return self.torch.empty(nscr // 8, dtype=self.torch.int64, device=self.dev), nscr

    def count(self, flags, n, scratch):
        return _assigncapi.flags_count(flags.data_ptr(), n, scratch[0].data_ptr(), scratch[1], self.st)

    def fill(self, flags, n, scratch, capacity, total, outputs):
        """one flags_fill with the named outputs and their input columns, every other pointer
        null -> the outputs downloaded whole, sentinel tails included"""
        cols = self.columns(n)
        out = {k: self.full((n if k == 'rank_out' else total) + PAD,
                            SENTINEL_C if k == 'c_out' else SENTINEL,
                            self.torch.float64 if k == 'c_out' else self.torch.int32) for k in outputs}
        args = {k: v.data_ptr() for k, v in out.items()}
        args.update({INPUT_OF[k]: cols[INPUT_OF[k]].data_ptr() for k in outputs if k in INPUT_OF})
        _assigncapi.flags_fill(flags.data_ptr(), n, scratch[0].data_ptr(), scratch[1], capacity,
                               self.st, **args)
        return {k: self.down(v) for k, v in out.items()}


@pytest.fixture(scope='module')
def gpu(ctx):
    return _Gpu()


def _reference(flags):
    """name -> the whole output of a fill at full capacity, without the sentinel tail"""
    a, b, c = ac.compaction_columns(len(flags))
    idx, rank = ac.compaction_reference(flags)
    return dict(a_out=a[idx], b_out=b[idx], c_out=c[idx], index_out=idx, rank_out=rank)


def _assert_outputs(got, want, capacity, what):
    """every output in `got`, byte for byte: the first min(capacity, total) entries are the
    reference's, every entry behind them keeps the sentinel; the ranks are always complete"""
    for name, host in got.items():
        ref = want[name]
        written = len(ref) if name == 'rank_out' else min(capacity, len(ref))
        expect = np.full(len(host), SENTINEL_C if name == 'c_out' else SENTINEL, host.dtype)
        expect[:written] = ref[:written]
        assert host.dtype == ref.dtype
        if host.tobytes() != expect.tobytes():
            bad = np.flatnonzero(host.view(np.uint8).reshape(len(host), -1) !=
                                 expect.view(np.uint8).reshape(len(host), -1))
            raise AssertionError('%s, %s at capacity %d: %d entries differ, the first at %d: %r for %r'
                                 % (what, name, capacity, len(bad), bad[0] // host.itemsize,
                                    host[bad[0] // host.itemsize], expect[bad[0] // host.itemsize]))


def _check_compaction(gpu, flags, scratch=None, alone=True):
    n = len(flags)
    want = _reference(flags)
    total = len(want['index_out'])
    assert total == np.count_nonzero(flags)
    f_dev = gpu.up(flags)
    scratch = scratch or gpu.scratch(n)
    assert gpu.count(f_dev, n, scratch) == total
    # every output at once: all of the list, then half of it
    for capacity in (total, total // 2):
        _assert_outputs(gpu.fill(f_dev, n, scratch, capacity, total, OUTPUTS), want, capacity, 'together')
    if alone:
        for name in OUTPUTS:
            _assert_outputs(gpu.fill(f_dev, n, scratch, total, total, (name,)), want, total, 'alone')
        # nothing but the ranks, as the confidence filter asks for them
        _assert_outputs(gpu.fill(f_dev, n, scratch, 0, total, ('rank_out',)), want, 0, 'ranks only')
    return total


@pytest.mark.parametrize('pattern', ac.FLAG_PATTERNS)
@pytest.mark.parametrize('shape', list(ac.COMPACTION_SHAPES))
def test_compaction_equals_flatnonzero(gpu, shape, pattern):
    n = ac.COMPACTION_SHAPES[shape]
    total = _check_compaction(gpu, ac.flag_pattern(pattern, n))
    assert (total == 0) == (pattern == 'none') and (pattern != 'all' or total == n)


def test_a_scratch_buffer_serves_one_count_after_another(gpu):
    """the fill follows the LAST count into a scratch buffer, whatever an earlier count of other
    flags, or of a longer list, left in it"""
    n = ac.COMPACTION_SHAPES['scan_one_over']
    scratch = gpu.scratch(n)
    first, second = ac.flag_pattern('half', n), ac.flag_pattern('any non-zero', n)
    assert np.count_nonzero(first) != np.count_nonzero(second)
    first_dev = gpu.up(first)
    assert gpu.count(first_dev, n, scratch) == np.count_nonzero(first)
    _check_compaction(gpu, second, scratch, alone=False)
    # a list of two cells in the scratch of 1 025: the cells behind its own are stale
    short = ac.COMPACTION_SHAPES['cell+1']
    assert scratch[1] > _assigncapi.scratch_bytes(short)
    _check_compaction(gpu, ac.flag_pattern('all', short), scratch, alone=False)
    _check_compaction(gpu, ac.flag_pattern('last', short), scratch, alone=False)


def test_compaction_on_a_stream_of_its_own(ctx):
    import torch
    dev = match.torch_device(0)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        gpu = _Gpu()
        assert gpu.st == side.cuda_stream != torch.cuda.default_stream(dev).cuda_stream
        n = ac.COMPACTION_SHAPES['scan_runs_3']
        _check_compaction(gpu, ac.flag_pattern('half', n), alone=False)
        _check_compaction(gpu, ac.flag_pattern('every 257th', n), alone=False)
    side.synchronize()


# ---- 2. the element-wise kernels beyond one grid stride ----------------------------------------------

@pytest.mark.parametrize('thd', ac.THRESHOLDS, ids=['%g' % v for v in ac.THRESHOLDS])
@pytest.mark.parametrize('n', ac.STRIDE_SIZES)
def test_conf_flags_beyond_one_grid_stride(gpu, n, thd):
    conf = ac.conf_case(n, thd)
    with np.errstate(invalid='ignore'):
        want = (conf >= thd).astype(np.int32)
    conf_dev, flags = gpu.up(conf), gpu.full(n + PAD, SENTINEL)
    _assigncapi.conf_flags(conf_dev.data_ptr(), n, thd, flags.data_ptr(), gpu.st)
    host = gpu.down(flags)
    bad = np.flatnonzero(host[:n] != want)
    assert len(bad) == 0, (len(bad), bad[:5], conf[bad[:5]], host[bad[:5]])
    assert np.all(host[n:] == SENTINEL)
    assert (want.sum() == 0) == bool(np.isnan(thd))


@pytest.mark.parametrize('pattern', ac.KEY_PATTERNS)
@pytest.mark.parametrize('n', ac.STRIDE_SIZES)
def test_boundaries_beyond_one_grid_stride(gpu, n, pattern):
    keys = ac.key_case(pattern, n)
    want = np.r_[True, keys[1:] != keys[:-1]].astype(np.int32)
    keys_dev, flags = gpu.up(keys), gpu.full(n + PAD, SENTINEL)
    _assigncapi.boundaries(keys_dev.data_ptr(), n, flags.data_ptr(), gpu.st)
    host = gpu.down(flags)
    bad = np.flatnonzero(host[:n] != want)
    assert len(bad) == 0, (len(bad), bad[:5], host[bad[:5]])
    assert np.all(host[n:] == SENTINEL)
    assert want.sum() == {'all equal': 1, 'all distinct': n}.get(pattern, len(np.unique(keys)))


def _cube_labels():
    rs = np.random.RandomState(7)
    return rs.randint(0, 2, ac.COST_POINTS).astype(np.int64), rs.randint(0, 2, ac.COST_POINTS).astype(np.int64)


@pytest.mark.parametrize('with_labels', [False, True])
@pytest.mark.parametrize('name', list(ac.COST_CUBES))
def test_costs_beyond_one_grid_stride(ctx, name, with_labels):
    pred, gt, i, j = ac.cost_table(name)
    assert len(i) > ac.STRIDE
    lp, lg = _cube_labels() if with_labels else (None, None)
    want = match.pair_costs(pred, gt, i, j, T, lp, lg)
    got = match.costs_device(pred, gt, i, j, T, 0, lp, lg)
    assert got[0].dtype == got[1].dtype == np.int32 and got[2].dtype == np.float64
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[2].tobytes() == want[2].tobytes()
    assert len(want[0]) > 20000 and (want[0] >= ac.STRIDE // ac.COST_POINTS + 1).any()


def test_costs_beyond_one_grid_stride_under_a_confidence_filter(ctx):
    """300 predictions: the rank of the kept ones spans two cells of the compaction"""
    pred, gt, i, j = ac.cost_table('half')
    n = len(pred)
    conf = np.random.RandomState(3).rand(n)
    sel = conf >= 0.5
    B = _assigncapi.BLOCK
    assert n > B and 0 < sel[:B].sum() < B and 0 < sel[B:].sum() < n - B
    renumber = np.cumsum(sel) - 1
    wi, wj, wc = match.pair_costs(pred, gt, i, j, T)
    keep = sel[wi]
    gi, gj, gc = match.costs_device(pred, gt, i, j, T, 0, conf=conf, thd=0.5)
    assert np.array_equal(gi, renumber[wi[keep]]) and np.array_equal(gj, wj[keep])
    assert gc.tobytes() == wc[keep].tobytes()
    assert len(gi) > 10000 and gi.max() == sel.sum() - 1 > renumber[B]


# ---- 3. labelling on long and unordered graphs --------------------------------------------------------

@pytest.mark.parametrize('permuted', [False, True])
def test_labels_on_a_long_chain(ctx, permuted):
    k = 200
    i, j = ac.long_chain(k, permuted)
    info = {}
    got = match.components_device(k, k, i, j, 0, info=info)
    want = match.components_numpy(k, i, j)
    assert np.array_equal(got, want) and np.all(got == 0) and len(got) == 2 * k - 1
    print('%d sweeps' % info['sweeps'])
    assert 2 <= info['sweeps'] <= k + k + 2                      # the bound match_device passes


def test_labels_on_the_rods(ctx):
    pred, gt = ac.rod(0, 64, 64, 300)
    i, j, _ = ac.admissible(pred, gt)
    got = match.components_device(len(pred), len(gt), i, j, 0)
    assert np.array_equal(got, match.components_numpy(len(pred), i, j)) and np.all(got == 0)
    pred, gt = ac.scene_of(ac.ROD_SCENE)
    i, j, _ = ac.admissible(pred, gt)
    got = match.components_device(len(pred), len(gt), i, j, 0)
    assert np.array_equal(got, match.components_numpy(len(pred), i, j)) and len(np.unique(got)) == 7


def test_labels_that_still_change_are_refused_and_the_next_call_is_right(gpu):
    i, j = ac.chain_pairs(8)
    i_dev, j_dev = gpu.up(i), gpu.up(j)
    work, label = gpu.full(8 + 8 + 1, SENTINEL), gpu.full(len(i) + PAD, SENTINEL)
    args = (i_dev.data_ptr(), j_dev.data_ptr(), len(i), 8, 8, work.data_ptr(), work[8:].data_ptr(),
            work[16:].data_ptr(), label.data_ptr())
    with pytest.raises(_assigncapi.FplAssignError, match='fpla_labels: the labels still change after 1 sweeps'):
        _assigncapi.labels(*args, 1, gpu.st)
    sweeps = _assigncapi.labels(*args, 8 + 8 + 2, gpu.st)
    host = gpu.down(label)
    assert np.all(host[:len(i)] == 0) and np.all(host[len(i):] == SENTINEL) and 2 <= sweeps <= 16
    assert np.array_equal(match.components_device(8, 8, i, j, 0), np.zeros(len(i), np.int32))


# ---- 4. mid-size sparse components, matrix for matrix -------------------------------------------------

@pytest.mark.parametrize('case', ac.ROD_CASES, ids=lambda c: 'seed%d-%dx%d' % c[:3])
def test_solve_equals_match_sparse_on_the_rods(ctx, case):
    seed, n_pred, n_gt, length = case
    pred, gt = ac.rod(seed, n_pred, n_gt, length)
    info, got = _check_matching(pred, gt)                        # one optimum: test_assign_host.py
    assert info['overflow'] == 0 and info['components'] == 1
    assert info['largest'] == len(ac.admissible(pred, gt)[0]) > _assigncapi.CAP
    assert 0 < got.nnz <= min(n_pred, n_gt)


@pytest.mark.parametrize('shuffle', [False, True])
def test_solve_equals_match_sparse_on_the_rod_scene(ctx, shuffle):
    """one wavefront solves a large component, then a small one, then the other orientation"""
    pred, gt = ac.scene_of(ac.ROD_SCENE, shuffle=shuffle)
    info, got = _check_matching(pred, gt)
    assert info['overflow'] == 0 and info['components'] == 7 and info['largest'] == 681
    assert got.nnz > 80


@pytest.mark.parametrize('name', [ac.OVER_BY_PAIRS] + list(ac.OVER_THE_CAP_RODS))
def test_sparse_components_over_the_cap_are_solved_on_the_host(ctx, name):
    part = ('rod',) + ac.OVER_THE_CAP_RODS[name] if name in ac.OVER_THE_CAP_RODS else name
    pred, gt = ac.scene_of(('2x2', part, '3x3 greedy'))
    info, got = _check_matching(pred, gt, exact=False)
    assert info['overflow'] == 1 and info['components'] == 3 and info['largest'] > 300
    i, j, cost = ac.admissible(pred, gt)
    want = match.match_sparse(len(pred), len(gt), i, j, cost)
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    assert got.nnz >= 2 + 3 + 10


@pytest.mark.parametrize('case', ac.TIED_RODS, ids=lambda c: '%dx%d' % c[1:3])
def test_solve_on_integer_coordinates_by_cost(ctx, case):
    seed, n_pred, n_gt, length = case
    pred, gt = ac.rod(seed, n_pred, n_gt, length, integer=True)
    info, got = _check_matching(pred, gt, exact=False)
    assert info['overflow'] == 0 and info['largest'] > _assigncapi.CAP and got.nnz > 0
