"""CPU: the dispatch plan of the float32 voxel2obj stages (csrc/v2o_plan.h), built alone with the
host C++ compiler.  Every case of tests/v2o_cases.py takes the branch its row names, the table
reaches every value of every plan field, and the plan equals the conditions v2o.hip carried
inline before the header existed, restated here, on a seeded sweep."""
import os
import re

import numpy as np
import pytest

from oracle import voxel2obj_oracle
from tests import helpers, v2o_cases
from tests.v2o_cases import N_CU, padded, wr_of

CSRC = v2o_cases.CSRC


def _cdiv(a, b):
    return -(-a // b)


# ---- the parent commit's inline conditions (launch_gauss_win, fpl_v2o_smooth, v2o_nms) ----------

def _best_block(n):
    best, waste = 256, 1e9
    for bd in range(256, 513, 64):
        wst = float(_cdiv(n, bd) * bd) / float(n)
        if wst < waste - 1e-9:
            waste, best = wst, bd
    return best


def _gyx_lrow(P2, wr):
    return (_cdiv(P2, 8) * 8 + 2 * wr + 3) // 4 * 4 + 4


def _gyx_lds_bytes(P2, wr):
    return 12 * _gyx_lrow(P2, wr) * 4 + (12 // 4) * _cdiv(P2, 4) * 8


def _parent_smooth(P, D, wr, unfused, n_cu):
    """which kernels the parent launched, with what grid, workgroup, LDS and arguments:
    {pass: (kernel, grid, block, lds, extra arguments)}"""
    n_pad = P[0] * P[1] * P[2]
    if wr not in (3, 4, 6, 10):
        g = _cdiv(n_pad, 256)
        return dict(z=('gauss_pass', g, 256, 0, ()), y=('gauss_pass', g, 256, 0, ()),
                    x=('gauss_pass', g, 256, 0, ()))
    fits = (P[1] * P[2] * 4 < 1 << 31 and P[2] >= 2 * wr and P[1] >= 12 + 2 * wr
            and P[0] * _cdiv(P[1], 12) < 1 << 28 and _gyx_lds_bytes(P[2], wr) <= 60 * 1024)
    fused = fits and not unfused
    small = ((12 + 2 * wr) * D[1] * D[2] < 1 << 31 and P[1] * P[2] * 12 < 1 << 31
             and P[0] >= 2 * wr)
    out = {}
    if small and not unfused:
        bd = _best_block(P[2])
        nxb = _cdiv(P[2], bd)
        seg_len = max(4 * wr, _cdiv(_cdiv(P[0], 4), 4 * wr) * 4 * wr)
        nseg = _cdiv(P[0], seg_len)
        out['z'] = ('gauss_z_ring', nxb * nseg * P[1], bd, 0, (nxb, nseg, seg_len))
    else:
        out['z'] = ('gauss_pass_win0', _cdiv(_cdiv(P[0], 16) * P[1] * P[2], 256), 256, 0, ())
    if fused:
        nwork = _cdiv(P[0], 4) * _cdiv(P[1], 12)
        out['yx'] = ('gauss_yx_fused', _cdiv(nwork, 8) * 8, _best_block(P[2]),
                     _gyx_lds_bytes(P[2], wr), (_gyx_lrow(P[2], wr),))
        return out
    out['y'] = ('gauss_pass_win1', _cdiv(P[0] * _cdiv(P[1], 16) * P[2], 256), 256, 0, ())
    ntiles = _cdiv(P[0] * P[1], 8) * _cdiv(P[2], 128)
    out['x'] = ('gauss_x_lds', min(ntiles, n_cu * 8), 256, 0, ())
    return out


def _plan_smooth(p, wr):
    """the same launches, read off a V2oSmoothPlan as v2o.hip now does"""
    if not p['windowed']:
        return {a: ('gauss_pass', p['grid_' + a], 256, 0, ()) for a in 'zyx'}
    out = {}
    if p['ring']:
        out['z'] = ('gauss_z_ring', p['grid_z'], p['block'], 0, (p['nxb'], p['nseg'], p['seg_len']))
    else:
        out['z'] = ('gauss_pass_win0', p['grid_z'], 256, 0, ())
    if p['fused']:
        out['yx'] = ('gauss_yx_fused', p['grid_yx'], p['block'], p['lds_bytes'], (p['lrow'],))
        return out
    out['y'] = ('gauss_pass_win1', p['grid_y'], 256, 0, ())
    out['x'] = ('gauss_x_lds', p['grid_x'], 256, 0, ())
    return out


def _parent_nms(P, r, use_seg, wplain):
    C = [_cdiv(v, 4) for v in P]
    n_cells = C[0] * C[1] * C[2]
    hw = (r + 3) // 4
    seg_ok = 1 <= hw <= 8 and n_cells < 1 << 31 and not wplain
    side = 2 * r + 1
    out = dict(C0=C[0], C1=C[1], C2=C[2], n_cells=n_cells, hw=hw, HW=hw if seg_ok else 0,
               wmax_seg=int(seg_ok), aligned=int(P[2] % 4 == 0))
    # clear_balls' own test, per part of the (2 r + 1)^2 rows
    fits = [side * side * (k + 1) // 4 - side * side * k // 4 <= 1024 for k in range(4)]
    out['clear_table'], out['clear_direct'] = int(any(fits)), int(not all(fits))
    W = _cdiv(side, 64)
    out['seg_words'] = 0 if not use_seg else (1 if W == 1 else (2 if W == 2 else 4))
    if use_seg and side > 64:
        out['seg_rows_global'] = 1
        out['seg_rows_bytes'] = 1024 * 2 * side * side * (2 if W <= 2 else 4) * 8
    elif use_seg:
        out['seg_rows_global'] = 0
        out['seg_rows_bytes'] = 2 * side * side * 8
    else:
        out['seg_rows_global'] = out['seg_rows_bytes'] = 0
    return out


def _span2(lo, centre):
    a, b = lo - centre, lo + 3 - centre
    n = a if a > 0 else (-b if b < 0 else 0)
    f = -a if -a > b else b
    return n * n, f * f


def _cut_cells(r, use_seg):
    """(most cells a ball hands over, most of them one workgroup stages), brute force over the
    centre's phases with clear_balls' cell walk; numpy over the cell box"""
    best_cut = best_stage = 0
    base = (r // 4 + 2) * 4
    for pz in range(4):
        for py in range(4):
            for px in range(4):
                c = (base + pz, base + py, base + px)
                c0 = [(v - r) // 4 for v in c]
                n = [(v + r) // 4 - lo + 1 for v, lo in zip(c, c0)]
                if use_seg:
                    best_cut = best_stage = max(best_cut, n[0] * n[1] * n[2])
                    continue
                nf = [np.array([_span2((lo + i) * 4, v) for i in range(k)]) for v, lo, k in zip(c, c0, n)]
                near = nf[0][:, None, None, 0] + nf[1][None, :, None, 0] + nf[2][None, None, :, 0]
                far = nf[0][:, None, None, 1] + nf[1][None, :, None, 1] + nf[2][None, None, :, 1]
                cut = ((near <= r * r) & (far > r * r)).reshape(-1)
                ncell = cut.size
                parts = [int(cut[ncell * k // 4:ncell * (k + 1) // 4].sum()) for k in range(4)]
                best_cut, best_stage = max(best_cut, sum(parts)), max(best_stage, max(parts))
    return best_cut, best_stage


# ---- the float32 cases the suite had before the table -------------------------------------------

def _older_cases(golden):
    """(name, D, r, sigma, use_seg) of tests/test_gpu_voxel2obj.py: the golden cases, the oracle
    tests, the FMA witnesses and the segmentation cases"""
    from tests import test_gpu_voxel2obj as t
    out = [(c['name'], c['shape'], c['r'], c['sigma'], 0) for c in helpers.v2o_cases(golden('voxel2obj.npz'))]
    out += [('oracle%d' % i, s, r, sg, 0) for i, (s, r, sg) in enumerate([
        ((120, 110, 130), 27, 5.0), ((160, 160, 160), 27, 5.0), ((90, 140, 75), 9, 2.0),
        ((64, 64, 200), 15, 3.0), ((120, 100, 130), 40, 3.0), ((70, 150, 90), 33, 2.0),
        ((96, 100, 104), 5, 1.5), ((96, 100, 104), 4, 2.0), ((50, 60, 70), 6, 2.0),
        ((80, 70, 90), 10, 3.0), ((30, 30, 30), 5, 2.0)])]
    out += [('fma%d' % seed, s, r, sg, 0) for seed, s, r, sg in t.FMA_WITNESSES]
    out += [(c[0], c[3], c[4], c[5], 1) for c in helpers.V2O_SEG_CASES]
    return out


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    exe = v2o_cases.build_driver(tmp_path_factory.mktemp('v2o_plan'))
    if not exe:
        pytest.skip('no host C++ compiler')
    return exe


def _table_plans(driver):
    """{(name, use_seg): plan} for the table, its segmentation variants included"""
    keys, queries = [], []
    for name, kind, seed, D, r, sigma, thd, n_min, want in v2o_cases.CASES:
        for use_seg in ([0, 1] if name in v2o_cases.SEG_CASES else [0]):
            keys.append((name, use_seg))
            queries.append((padded(D, r), D, wr_of(sigma), 0, r, use_seg, 0, 1))
    plans, consts = v2o_cases.ask_plans(driver, queries)
    return dict(zip(keys, plans)), consts


def test_header_holds_the_constants_and_v2o_hip_none_of_them(driver):
    _, consts = _table_plans(driver)
    assert consts == dict(CELL=4, GX_ROWS=8, GX_SEG=128, GZ_OUT=12, GYX_TY=12, GYX_LDS_MAX=60 * 1024,
                          WM_OUTS=8, CLR_STAGE=6144, CLR_PARTS=4, CLR_ROWS=1024)
    text = open(os.path.join(CSRC, 'v2o.hip')).read()
    assert '#include "v2o_plan.h"' in text
    # no constant and no condition is left behind
    assert not re.search(r'constexpr\s+int\s+(CELL|GX_ROWS|GX_SEG|GZ_OUT|GYX_TY|WM_OUTS|CLR_\w+)\b', text)
    for moved in ('best_block(', 'gyx_fits(', 'gyx_lrow(', 'gyx_lds_bytes(', 'seg_ok', 'P2 % CELL',
                  '>= 2 * WR;', '60 * 1024'):
        assert moved not in text, moved
    assert len(re.findall(r'getenv\("FPL_V2O_UNFUSED"\)', text)) == 1


def test_each_case_takes_the_branch_of_its_row(driver):
    plans, _ = _table_plans(driver)
    names = [c[0] for c in v2o_cases.CASES]
    assert len(set(names)) == len(names)
    for name, kind, seed, D, r, sigma, thd, n_min, want in v2o_cases.CASES:
        P, wr, p = padded(D, r), wr_of(sigma), plans[(name, 0)]
        assert P[0] * P[1] * P[2] < 10e6, name
        derived = dict(wr=wr, x_stride=p['grid_x'] < p['x_tiles'], P2_lt_2wr=P[2] < 2 * wr,
                       **{'P%d_lt_wr' % a: P[a] < wr for a in range(3)})
        print(name, P, 'wr', wr, p)
        for k, v in want.items():
            got = derived[k] if k in derived else p[k]
            assert got == v, (name, k, got, v)
        if name == 'x574':      # the production substack's row: a part-filled last x block
            assert p['nxb'] * p['block'] > P[2] > (p['nxb'] - 1) * p['block']
    # the segmentation variants: one mask word at r = 31, two at r = 32
    assert plans[('r31', 1)]['seg_words'] == 1 and plans[('r32', 1)]['seg_words'] == 2
    assert plans[('r31', 1)]['seg_rows_global'] == 0 and plans[('r32', 1)]['seg_rows_global'] == 1
    # 'stage': every cell of a 19^3 box, staged by one workgroup - more than the stage holds
    st = plans[('stage', 1)]
    assert st['stage_overflows'] == 1 and st['stage_cells_max'] == 19 ** 3 > 6144
    assert plans[('stage', 0)]['stage_overflows'] == 0
    assert plans[('r32', 1)]['stage_overflows'] == 0


def test_first_radii_that_overflow_the_stage(driver):
    """under a segmentation r = 35 is the first radius whose ball can overflow touch_cell's stage
    (the 'stage' case).  Without one a workgroup stages a quarter slab of the cells the sphere
    CUTS: the whole ball first cuts more than the stage holds near r = 85, a quarter of it only
    near r = 170 - a volume of live candidates that wide is out of a fast test's reach, which
    is why the table has no such case."""
    rs = list(range(1, 40)) + list(range(80, 92)) + list(range(160, 181))
    q = [((4, 4, 4), (4, 4, 4), 3, 0, r, s, 0, 1) for s in (0, 1) for r in rs]
    plans, _ = v2o_cases.ask_plans(driver, q)
    seg = dict(zip(rs, plans[len(rs):]))
    plain = dict(zip(rs, plans[:len(rs)]))
    assert min(r for r in rs if seg[r]['stage_overflows']) == 35 == v2o_cases.by_name('stage')[4]
    first_ball = min(r for r in rs if plain[r]['cut_cells_max'] > 6144)
    first_part = min(r for r in rs if plain[r]['stage_overflows'])
    print('no segmentation: a ball cuts > 6144 cells from r =', first_ball,
          '; one workgroup stages > 6144 from r =', first_part)
    assert 80 < first_ball < 92 and 160 < first_part <= 180
    assert not any(plain[r]['stage_overflows'] for r in rs if r < first_part)
    # a live shell at distance r needs D >= 2 r: (4 r)^3 padded voxels
    assert (4 * first_part) ** 3 > 10e6
    # the header's count is clear_balls' own cell walk
    for r in (1, 5, 9, 27, 31, 32, 35, 85, 170):
        for s in (0, 1):
            d = (seg if s else plain)[r]
            assert (d['cut_cells_max'], d['stage_cells_max']) == _cut_cells(r, s), (r, s)


def test_stage_case_fills_every_cell_of_the_first_ball():
    """what the 'stage' case is built on: in the oracle's volume every cell of the centre's box
    holds a candidate above the threshold, and the centre is the largest of them"""
    _, kind, seed, D, r, sigma, thd, _, _ = v2o_cases.by_name('stage')
    sm = voxel2obj_oracle.smooth_and_clear(v2o_cases.make_pred(kind, D), r, sigma)
    thresh = max(float(np.percentile(sm, 97)), 0.0)
    c = 35 + r
    assert c % 4 == 2 and np.unravel_index(np.argmax(sm), sm.shape) == (c, c, c)
    lo, hi = (c - r) // 4, (c + r) // 4
    assert hi - lo + 1 == 19
    box = sm[4 * lo:4 * hi + 4, 4 * lo:4 * hi + 4, 4 * lo:4 * hi + 4]
    assert box.shape == (76, 76, 76)
    live = (box.reshape(19, 4, 19, 4, 19, 4) > thresh).any(axis=(1, 3, 5))
    assert live.all() and live.size > 6144


def test_table_reaches_every_value_of_every_field(driver, golden):
    plans, _ = _table_plans(driver)
    older = _older_cases(golden)
    old_plans, _ = v2o_cases.ask_plans(
        driver, [(padded(D, r), D, wr_of(sg), 0, r, s, 0, 0) for _, D, r, sg, s in older])
    for (name, D, r, sg, s), p in zip(older, old_plans):
        print('older', name, padded(D, r), 'wr', wr_of(sg), p)
    plain = [p for (n, s), p in plans.items() if s == 0]

    def values(field, rows=plain):
        return {p[field] for p in rows}
    win = [p for p in plain if p['windowed']]
    for flag in ('windowed', 'aligned', 'clear_table', 'clear_direct', 'wmax_seg'):
        assert values(flag) == {0, 1}, flag
    for flag in ('fits', 'fused', 'ring'):
        assert values(flag, win) == {0, 1}, flag
    # every combination of the z pass and the y/x passes
    assert {(p['ring'], p['fused']) for p in win} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # every window radius runs every kernel of its family
    by_wr = {}
    for c in v2o_cases.CASES:
        by_wr.setdefault(wr_of(c[5]), []).append(plans[(c[0], 0)])
    assert {3, 4, 6, 10} < set(by_wr)
    for wr in (3, 4, 6, 10):
        assert {p['fused'] for p in by_wr[wr]} == {0, 1} and {p['ring'] for p in by_wr[wr]} == {0, 1}, wr
    for wr in (3, 4, 6, 10):    # ... and the LDS limit or a thin row stops the fused pass
        assert any(not p['fits'] for p in by_wr[wr]), wr
    assert values('HW') == set(range(9))
    # 512 cannot come out of best_block: a multiple of 512 is a multiple of 256, so 256 never
    # wastes more, and the smaller size wins a tie
    assert values('block', [p for p in win if p['ring'] or p['fused']]) == {256, 320, 384, 448}
    assert all(b != 512 for b in map(_best_block, range(1, 20000)))
    assert 1 in values('nxb', win) and max(values('nxb', win)) > 1
    assert 1 in values('nseg', win) and max(values('nseg', win)) > 1
    assert any(p['grid_x'] and p['grid_x'] < p['x_tiles'] for p in win)        # x_lds grid stride
    assert any(p['grid_x'] and p['grid_x'] == p['x_tiles'] for p in win)
    # both values of `aligned` with the fused pass's cell keys and without them
    assert {(p['aligned'], p['fused']) for p in win} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # mask words of clear_balls_seg: 1 and 2 in the table's segmentation variants, 4 in the older
    # suite's seg_r70, whose oracle run is too slow to repeat here
    seg_rows = [p for (n, s), p in plans.items() if s == 1]
    assert values('seg_words', seg_rows) == {1, 2}
    assert values('seg_words', seg_rows + [p for c, p in zip(older, old_plans) if c[4]]) == {1, 2, 4}
    assert values('stage_overflows', seg_rows) == {0, 1}
    # what the table adds to the older cases
    assert values('HW') - values('HW', old_plans) == {5, 6, 8}
    assert values('block', old_plans) == {256}


def test_plan_equals_the_parent_commits_inline_conditions(driver):
    rng = np.random.default_rng(20260)
    queries = []
    edges = [1, 2, 5, 6, 7, 8, 11, 12, 13, 15, 16, 17, 19, 20, 21, 24, 25, 31, 32, 33, 39, 40, 41, 80, 81]
    wide = [255, 256, 257, 320, 321, 380, 384, 385, 448, 449, 500, 504, 512, 513, 574, 636, 1024, 1025,
            1112, 1113, 1120, 1121, 1200, 2047, 2049]
    for i in range(2000):
        wr = int(rng.choice([3, 4, 6, 10, 3, 4, 6, 10, 1, 2, 5, 8, 12]))
        r = int(rng.choice([0, 1, 3, 4, 5, 8, 9, 16, 17, 27, 28, 29, 31, 32, 33, 63, 64, 70, 95, 96, 127]
                           if i % 3 else [int(rng.integers(0, 128))]))
        P = []
        for a in range(3):
            kind = rng.integers(0, 4)
            lo = 2 * r + 1
            if kind == 0:
                v = int(rng.choice(edges))
            elif kind == 1 and a == 2:
                v = int(rng.choice(wide))
            elif kind == 2:
                v = int(rng.integers(1, 700))
            else:
                v = int(rng.choice([wr - 1, wr, 2 * wr - 1, 2 * wr, 2 * wr + 1, 4 * wr, 4 * wr + 1,
                                    12 + 2 * wr - 1, 12 + 2 * wr, 8 * wr, 8 * wr + 1]))
            P.append(max(v, lo))
        if i % 50 == 0:         # the 32-bit limits: a plane beyond 2^31 / 12 and 2^31 / 4 bytes
            P[1], P[2] = int(rng.choice([9000, 13400, 23200])), int(rng.choice([13400, 23200]))
            P[0] = max(2 * r + 1, int(rng.choice([1, 8, 20])))
        D = [v - 2 * r for v in P]
        queries.append((tuple(P), tuple(D), wr, int(i % 7 == 0), r, int(i % 2 and r <= 127),
                        int(i % 11 == 0), 0))
    plans, _ = v2o_cases.ask_plans(driver, queries)
    seen = set()
    for (P, D, wr, unfused, r, use_seg, wplain, _), p in zip(queries, plans):
        want = _parent_smooth(P, D, wr, unfused, N_CU)
        assert _plan_smooth(p, wr) == want, (P, D, wr, unfused, p, want)
        nms = _parent_nms(P, r, use_seg, wplain)
        assert {k: p[k] for k in nms} == nms, (P, r, use_seg, wplain, p, nms)
        assert p['clear_table'] != p['clear_direct']          # no r mixes the two row forms
        seen.add(tuple(sorted((k, v[0]) for k, v in want.items())))
    assert len(seen) == 5, seen                              # every set of kernels was compared
    assert sum(1 for q in queries if q[0][1] * q[0][2] * 12 >= 1 << 31) > 10
