"""libfplmerge.so on the GPU: rm_tbar_multi_pred(solver='device') against the numpy executor
dedupe.merge_numpy - the three arrays and `info` - on every case of tests/merge_cases.py, on the
point sets of tests/near_cases.py and at the component counts where a kernel takes another path;
the stages alone through the C ABI; the pipeline's merge_solver=."""
import os

import numpy as np
import pytest

from flypylib_amd import _mergecapi as capi, dedupe, fplpipeline, fplsynapses, near
from tests import merge_cases as mc, near_cases

pytestmark = pytest.mark.gpu

T = near_cases.T
CASES = mc.all_cases()
_WANT = {}


def _want(name, caps):
    """the executor's result, computed once per (case, caps) and left unchanged"""
    key = (name, caps)
    if key not in _WANT:
        info = {}
        out = dedupe.merge_numpy(*mc.split(CASES[name]), info=info, **mc.CAPS[caps])
        _WANT[key] = tuple(a.copy() for a in out), info
    return _WANT[key]


def _same(got, want):
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _device(case, info=None, **caps):
    return dedupe.merge_device(*mc.split(case), 0, info=info, **caps)


@pytest.mark.parametrize('name', list(CASES))
def test_the_device_equals_the_executor(ctx, name):
    want, want_info = _want(name, 'default')
    info = {}
    _same(_device(CASES[name], info), want)
    assert info == want_info
    # ... and what the public function returns is method='sparse''s
    tbars, kw = CASES[name]
    got = fplsynapses.rm_tbar_multi_pred(tbars, method='sparse', device=0, solver='device', **kw)
    _same(got, fplsynapses.rm_tbar_multi_pred(tbars, method='sparse', **kw))


@pytest.mark.parametrize('caps', [c for c in mc.CAPS if c != 'default'])
@pytest.mark.parametrize('name', ['random 500, labelled', 'planted 500', 'random 3000', 'realistic',
                                  'golden: chain_reaches_a_stranger', 'hand-made: coincident strangers',
                                  'hand-made: ties inside a component'])
def test_forced_caps(ctx, name, caps):
    want, want_info = _want(name, caps)
    info = {}
    _same(_device(CASES[name], info, **mc.CAPS[caps]), want)
    assert info == want_info


@pytest.mark.parametrize('name', list(near_cases.SETS))
def test_the_point_sets_of_the_neighbour_table(ctx, name):
    pts = near_cases.SETS[name]()
    rs = np.random.RandomState(len(pts))
    conf = (rs.rand(len(pts)) * 0.75 + 0.25).astype(np.float32).astype(np.float64)
    ll = rs.randint(0, 2, len(pts))
    want_info, info = {}, {}
    want = dedupe.merge_numpy(pts, conf, ll, T, info=want_info)
    _same(dedupe.merge_device(pts, conf, ll, T, 0, info=info), want)
    assert info == want_info


# 255 / 256 / 257: around a block of the compaction; beyond one grid stride of the solve kernel;
# beyond one run per thread of the block scan (over the per-block counts of n + 1 flags)
STRIDE = capi.SOLVE_BLOCK * capi.SOLVE_BLOCKS
SCAN = capi.BLOCK * capi.SCAN_THREADS


@pytest.mark.parametrize('k', [255, 256, 257, STRIDE + 1, SCAN // 2 + 1])
def test_component_counts(ctx, k):
    tb = mc.pairs_lattice(k)
    n = 2 * k
    assert (k > STRIDE) == (k in (STRIDE + 1, SCAN // 2 + 1)) and (n + 1 > SCAN) == (k == SCAN // 2 + 1)
    info = {}
    got = dedupe.merge_device(tb['locs'], tb['conf'], np.zeros(n), T, 0, info=info)
    assert info == dict(components=k, largest=2, sweeps=2, host_components=0, host_points=0, closure_rounds=0)
    # every pair merges: the more confident point moves, the other is removed
    rm, mv, loc = got
    assert rm.sum() == k and mv.sum() == k and not (rm & mv).any()
    if k <= 257:
        _same(got, fplsynapses.rm_tbar_multi_pred(tb, method='sparse'))
    else:
        # the host loop takes a minute here; the pairs are independent, so each is its own problem
        ip, ind = near.pairs_numpy(tb['locs'], T)
        assert np.all(np.diff(ip) == 1)
        partner = ind[ip[:-1]]
        first = np.argsort(-tb['conf'])
        rank = np.empty(n, np.int64)
        rank[first] = np.arange(n)
        assert np.array_equal(mv, rank < rank[partner])
        i = np.nonzero(mv)[0]
        j = partner[i]
        pair = np.stack([np.minimum(i, j), np.maximum(i, j)], axis=1)
        w = tb['conf'][pair]
        w = w / (w[:, :1] + w[:, 1:])
        mean = w[:, :1] * tb['locs'][pair[:, 0]] + w[:, 1:] * tb['locs'][pair[:, 1]]
        assert np.array_equal(loc[i], np.round(mean).astype('int')) and not loc[rm].any()


# ---- the stages through the C ABI ------------------------------------------------------------------

GUARD = 64


def _guarded(torch, n, dtype, fill):
    """a resident array of n elements between two guard bands"""
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device='cuda:0')
    return whole, whole[GUARD:GUARD + n]


def _clean(whole, n, fill):
    g = whole.cpu().numpy()
    return bool(np.all(g[:GUARD] == fill) and np.all(g[GUARD + n:] == fill))


def _table(torch, pts):
    stream = torch.cuda.current_stream()
    return dedupe.device_table(np.ascontiguousarray(pts, np.float64), T, torch.device('cuda', 0), torch, stream), stream


@pytest.mark.parametrize('name', ['boundary', 'block tail: B + 1', 'cluster', 'lattice on the cell faces', 'no pair'])
def test_filtered_rows_are_the_hosts(ctx, name):
    import torch
    pts = near_cases.SETS[name]()
    n = len(pts)
    ip, ind = near.pairs_numpy(pts, T)
    has, f_ip, f_ind = fplsynapses._sparse_rows(pts, ip, ind, T)
    tab, stream = _table(torch, pts)
    has_w, has_d = _guarded(torch, n, torch.int32, -7)
    off_w, off_d = _guarded(torch, n + 1, torch.int32, -7)
    head = torch.zeros(2, dtype=torch.int64, device='cuda:0')
    args = (tab['p'].data_ptr(), n, T, tab['offsets'].data_ptr(), tab['indices'].data_ptr(), tab['entries'])
    total = capi.rows_count(*args, has_d.data_ptr(), off_d.data_ptr(), head.data_ptr(), stream.cuda_stream)
    assert total == len(f_ind)
    out_w, out_d = _guarded(torch, total, torch.int32, -7)
    capi.rows_fill(*args, off_d.data_ptr(), total, out_d.data_ptr(), stream.cuda_stream)
    assert has_d.cpu().numpy().astype(np.int64).tobytes() == has.astype(np.int64).tobytes()
    assert off_d.cpu().numpy().astype(np.int64).tobytes() == f_ip.tobytes()
    assert out_d.cpu().numpy().tobytes() == f_ind.tobytes()
    assert _clean(has_w, n, -7) and _clean(off_w, n + 1, -7) and _clean(out_w, total, -7)
    if total > 3:                                            # a capacity below the table: nothing beyond it
        out_w, out_d = _guarded(torch, total, torch.int32, -7)
        capi.rows_fill(*args, off_d.data_ptr(), total - 3, out_d.data_ptr(), stream.cuda_stream)
        got = out_d.cpu().numpy()
        assert np.array_equal(got[:total - 3], f_ind[:total - 3]) and np.all(got[total - 3:] == -7)


def _chain(pairs=12):
    """a chain a dozen pairs across (25 points 20 apart), shuffled, among far singletons"""
    rs = np.random.RandomState(pairs)
    pts = np.concatenate([mc._line(2 * pairs + 1, 20.0), mc._far(6)])
    return pts[rs.permutation(len(pts))]


@pytest.mark.parametrize('name', ['chain', 'singletons', 'random'])
def test_the_partition_and_the_grouping(ctx, name):
    import torch
    pts = {'chain': _chain, 'singletons': near_cases.no_pair,
           'random': lambda: near_cases.random_integer(700, 3.0)}[name]()
    n = len(pts)
    ip, ind = near.pairs_numpy(pts, T)
    comp, sweeps = dedupe.partition_numpy(ip, ind)
    tab, stream = _table(torch, pts)
    lab_w, lab_d = _guarded(torch, n, torch.int32, -7)
    oth_w, oth_d = _guarded(torch, n, torch.int32, -7)
    changed = torch.zeros(1, dtype=torch.int32, device='cuda:0')
    got = capi.labels(tab['offsets'].data_ptr(), tab['indices'].data_ptr(), n, tab['entries'],
                      lab_d.data_ptr(), oth_d.data_ptr(), changed.data_ptr(), n + 1, stream.cuda_stream)
    assert got == sweeps and (name != 'chain' or sweeps >= 13) and (name != 'singletons' or sweeps == 1)
    assert np.array_equal(lab_d.cpu().numpy(), comp) and np.array_equal(oth_d.cpu().numpy(), comp)
    assert _clean(lab_w, n, -7) and _clean(oth_w, n, -7)
    if name == 'chain':
        with pytest.raises(capi.FplMergeError, match='still change after 3 sweeps'):
            capi.labels(tab['offsets'].data_ptr(), tab['indices'].data_ptr(), n, tab['entries'],
                        lab_d.data_ptr(), oth_d.data_ptr(), changed.data_ptr(), 3, stream.cuda_stream)
    # the grouping: keys, the caller's sort, the starts
    rank = np.random.RandomState(5).permutation(n).astype(np.int32)
    members, starts = dedupe.group_numpy(ip, comp, rank)
    rank_d = torch.from_numpy(rank).cuda()
    comp_d = torch.from_numpy(comp).cuda()
    key_w, key_d = _guarded(torch, n, torch.int64, -7)
    capi.group_keys(tab['offsets'].data_ptr(), comp_d.data_ptr(), rank_d.data_ptr(), n, key_d.data_ptr(),
                    stream.cuda_stream)
    idle = np.diff(ip) == 0
    want_keys = np.where(idle, 2 ** 31 - 1, comp).astype(np.int64) * 2 ** 32 + rank
    assert np.array_equal(key_d.cpu().numpy(), want_keys) and _clean(key_w, n, -7)
    keys, order = torch.sort(key_d)
    flag_w, flag_d = _guarded(torch, n + 1, torch.int32, -7)
    capi.boundaries(keys.data_ptr(), n, flag_d.data_ptr(), stream.cuda_stream)
    got_starts = dedupe.compact(flag_d, n + 1, torch.device('cuda', 0), torch, stream).cpu().numpy()
    assert _clean(flag_w, n + 1, -7)
    assert np.array_equal(got_starts, starts) and got_starts.dtype == np.int32
    assert np.array_equal(order.cpu().numpy()[:len(members)], members)


def test_the_compaction_keeps_within_its_capacity(ctx):
    import torch
    stream = torch.cuda.current_stream()
    n = 3 * capi.BLOCK + 17
    flags = (np.random.RandomState(2).rand(n) < 0.3).astype(np.int32)
    want = np.nonzero(flags)[0]
    flags_d = torch.from_numpy(flags).cuda()
    nscr = capi.scratch_bytes(n)
    scr_w, scr_d = _guarded(torch, (nscr + 7) // 8, torch.int64, -7)
    total = capi.flags_count(flags_d.data_ptr(), n, scr_d.data_ptr(), nscr, stream.cuda_stream)
    assert total == len(want)
    out_w, out_d = _guarded(torch, total, torch.int32, -7)
    capi.flags_fill(flags_d.data_ptr(), n, scr_d.data_ptr(), nscr, total - 5, out_d.data_ptr(), stream.cuda_stream)
    got = out_d.cpu().numpy()
    assert np.array_equal(got[:total - 5], want[:total - 5]) and np.all(got[total - 5:] == -7)
    assert _clean(out_w, total, -7) and _clean(scr_w, (nscr + 7) // 8, -7)


def test_the_solve_stays_inside_its_outputs(ctx, monkeypatch):
    """merge_device with every output of the solve kernel between guard bands"""
    import torch
    made = []
    real = torch.zeros

    def zeros(shape, dtype=None, device=None):
        size = int(np.prod(shape))
        whole = torch.full((size + 2 * GUARD,), 0, dtype=dtype, device=device)
        whole[:GUARD] = 5
        whole[GUARD + size:] = 5
        made.append((whole, size))
        return whole[GUARD:GUARD + size].view(shape)

    case = CASES['realistic']
    want, want_info = _want('realistic', 'default')
    monkeypatch.setattr(torch, 'zeros', zeros)
    info = {}
    got = _device(case, info)
    monkeypatch.setattr(torch, 'zeros', real)
    _same(got, want)
    assert info == want_info and len(made) >= 5
    for whole, size in made:
        g = whole.cpu().numpy()
        assert np.all(g[:GUARD] == 5) and np.all(g[GUARD + size:] == 5)


def test_two_calls_give_equal_bytes(ctx):
    for name in ('realistic', 'random 3000, labelled'):
        a, b = _device(CASES[name]), _device(CASES[name])
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_the_realistic_set_stays_on_the_device(ctx):
    """solver='device' equals solver='host', and it cannot pass by sending everything to the
    host: at most 5 % of the points that have neighbours go there (test_merge_host.py checks the
    same of the executor)"""
    tb, twice = mc.realistic()
    info = {}
    got = fplsynapses.rm_tbar_multi_pred(tb, method='sparse', device=0, solver='device', info=info)
    _same(got, fplsynapses.rm_tbar_multi_pred(tb, method='sparse', device=0, solver='host'))
    ip, ind = near.pairs_numpy(tb['locs'], T)
    has = fplsynapses._sparse_rows(tb['locs'], ip, ind, T)[0]
    print('host_points %d of %d points with neighbours' % (info['host_points'], (has > 0).sum()))
    assert (has > 0).sum() >= 2 * twice and info['host_points'] <= 0.05 * (has > 0).sum()
    assert got[1].sum() >= twice // 2


def test_refusals_with_a_gpu_at_hand(ctx, monkeypatch):
    tb = near_cases.planted(100)
    with pytest.raises(ValueError, match="solver='host'"):
        fplsynapses.rm_tbar_multi_pred({'locs': tb['locs'], 'conf': tb['conf'].astype(np.float32)},
                                       method='sparse', device=0, solver='device')
    with pytest.raises(ValueError, match=r'cand_cap 8 must lie in \[1, 7\]'):
        dedupe.merge_device(tb['locs'], tb['conf'], np.zeros(100), T, 0, cand_cap=8)
    monkeypatch.setattr(capi._side, '_lib', None)
    monkeypatch.setattr(capi._side, 'path', '/nonexistent/libfplmerge.so')
    with pytest.raises(capi.FplMergeError, match='libfplmerge.so not found at /nonexistent'):
        fplsynapses.rm_tbar_multi_pred(tb, method='sparse', device=0, solver='device')


def test_the_pipeline_keyword(ctx, tmp_path):
    """all_merged.p is the same bytes from merge_solver='device' as from the host loop"""
    from flypylib_amd import fplobjdetect
    from tests.test_pipeline import _small_setup
    net, vol, roi = _small_setup()
    kw = dict(obj_min_dist=5, smoothing_sigma=1.5, buffer_sz=10, precision='f32')
    norm = [128., 33., 0.7]
    wd = str(tmp_path / 'merged')
    host = fplobjdetect.full_roi_inference(vol, None, roi, net, 0.2, wd, norm, neighbor_thresh=12, **kw)
    merged = open(wd + '/all_merged.p', 'rb').read()
    os.remove(wd + '/all_merged.p')
    # the finished substacks are reused; the merge runs again, on the device
    dev = fplobjdetect.full_roi_inference(vol, None, roi, net, 0.2, wd, norm, neighbor_thresh=12,
                                          merge_device=0, merge_solver='device', **kw)
    assert open(wd + '/all_merged.p', 'rb').read() == merged
    assert np.array_equal(dev['locs'], host['locs']) and np.array_equal(dev['conf'], host['conf'])
    assert len(host['conf']) > 20
    with pytest.raises(ValueError, match="solver='device' with method='sparse', device=None"):
        fplpipeline.merge_border_duplicates(host, 12, solver='device')
