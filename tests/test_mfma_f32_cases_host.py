"""tests/mfma_f32_cases.py on the CPU: every case of test_gpu_mfma_f32.py exercises what it says
(block edges crossed, m-blocks, slices, channel chunks), the kernel launches predicted for it are
the intended ones (the table is printed), its derived bound is neither vacuous nor too tight - the
oracle's own float32 forward stays inside it and it is far below the project's 1e-3 gate - the
integer cases are exact in float32, and every expected side, corrupted, fails its check."""
import re
import os

import numpy as np
import pytest
import torch

from flypylib_amd.program import LayerGraph
from oracle import cnn_oracle
from tests import mfma_f32_cases as mc
from tests.perop_cases import U, _W5, _W7, _conv64, lift_is_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source():
    with open(os.path.join(ROOT, 'flypylib_amd', 'csrc', 'conv_mfma_f32.hip')) as f:
        return f.read()


def _f32(c):
    return cnn_oracle.graph_forward(c['graph'], c['x'], dtype=torch.float32).astype(np.float64)


# ---- the dispatcher's restatement -------------------------------------------------------------
def test_the_launch_names_and_tile_constants_the_cases_rest_on():
    """(that the restated rules are the executor's is shown by behaviour: test_mfma_f32_plan_host.py
    holds the plan header to them on every case here and on a sweep)"""
    src = _source()
    names = set(re.findall(r'"(mfma_[a-z0-9_]+_f32)"', src))
    assert names >= {'mfma_conv3_f32', 'mfma_conv3_conv1_f32', 'mfma_conv3_conv1_pool_f32', 'mfma_stem_f32',
                     'mfma_stem_conv1_pool_f32', 'mfma_conv1_f32', 'mfma_add_f32', 'mfma_pool_f32'}
    # tile constants the shapes were chosen for
    assert 'constexpr int ST_Z = 4, ST_Y = 8, ST_X = 64;' in src and 'constexpr int TZ = 6, TY = 6, TX = 18;' in src


def test_predicted_launch_table(capsys):
    rows = []
    for kind, cin, cout, v in mc.CONV_CASES:
        if v == 'none':
            t = mc.tiles_of(kind, cin, cout)[0]
            rows.append(('%s %d -> %d' % (kind, cin, cout), mc.conv_case(kind, cin, cout, v, t)['launches']))
    for case in mc.FUSED_CASES + mc.UNFUSED_CASES + mc.STEM_FUSED_CASES + mc.STEM_UNFUSED_CASES:
        rows.append(('chain %r' % (case,), mc.fused_case(*case, tile=7)['launches']))
    for name in mc.EXACT_CASES:
        rows.append((name, mc.exact_case(name)['launches']))
    for kind, cin, cout, tile, lifts in mc.DECLINED_CASES + mc.NEIGHBOUR_CASES:
        rows.append(('%s %d -> %d %r' % (kind, cin, cout, lifts), mc.conv_case(kind, cin, cout, 'bias', tile, lifts)['launches']))
    with capsys.disabled():
        print()
        for name, launches in rows:
            print('  %-58s %s' % (name, launches if launches is not None else 'declined: per-op executor'))
    table = dict(rows)
    # the expectations the issue names, stated by hand
    assert table['conv3 32 -> 130'] == {'mfma_conv1_f32': 1, 'mfma_conv3_f32': 3}
    assert table['conv3 48 -> 65'] == {'mfma_conv1_f32': 1, 'mfma_conv3_f32': 2}
    assert table['conv3 192 -> 16'] == {'mfma_conv1_f32': 2, 'mfma_conv3_f32': 1}
    assert table['stem 1 -> 64'] == {'mfma_stem_f32': 1}
    assert table['conv1 48 -> 64'] == {'mfma_conv1_f32': 2} and table['conv1 1 -> 48'] == {'mfma_conv1_f32': 1}
    for case in mc.FUSED_CASES:
        name = 'mfma_conv3_conv1_pool_f32' if case[4] else 'mfma_conv3_conv1_f32'
        assert table['chain %r' % (case,)] == {'mfma_conv1_f32': 1, name: 1}
    for case in mc.UNFUSED_CASES:
        want = {'mfma_conv1_f32': 2, 'mfma_conv3_f32': 1}
        if case[5] == 'second_reader':
            want['mfma_add_f32'] = 1
        elif case[4] == 2:
            want['mfma_pool_f32'] = 1
        assert table['chain %r' % (case,)] == (None if case[4] == 3 else want)
    for case in mc.STEM_FUSED_CASES:
        assert table['chain %r' % (case,)] == {'mfma_stem_conv1_pool_f32': 1}
    for case in mc.STEM_UNFUSED_CASES:
        want = {'mfma_stem_f32': 1, 'mfma_conv1_f32': 1}
        if case[4]:
            want['mfma_pool_f32'] = 1
        assert table['chain %r' % (case,)] == want
    for kind, cin, cout, tile, lifts in mc.DECLINED_CASES:
        assert table['%s %d -> %d %r' % (kind, cin, cout, lifts)] is None
    for kind, cin, cout, tile, lifts in mc.NEIGHBOUR_CASES:
        assert table['%s %d -> %d %r' % (kind, cin, cout, lifts)] is not None
    assert table['cat_skip_up_16_5'] == {'mfma_conv1_f32': 1, 'mfma_stem_f32': 1, 'mfma_pool_f32': 1, 'mfma_conv3_f32': 1}
    assert table['add_relu'] == {'mfma_conv1_f32': 1, 'mfma_conv3_f32': 1, 'mfma_add_f32': 1}
    assert table['pool7_negative'] == {'mfma_conv1_f32': 1, 'mfma_pool_f32': 1}
    assert table['up2'] == {'mfma_conv1_f32': 1, 'mfma_pool_f32': 1, 'mfma_conv3_f32': 1}


def test_the_cases_are_the_issues():
    assert mc.CONV3_PAIRS == [(2, 1), (3, 5), (16, 16), (17, 33), (20, 64), (48, 65), (96, 48), (192, 16), (32, 130)]
    assert mc.STEM_COUTS == [1, 5, 16, 17, 48, 64] and len(mc.STEM_67) == 2
    assert mc.CONV1_PAIRS == [(1, 48), (5, 7), (47, 48), (48, 48), (49, 48), (48, 17), (48, 64), (96, 1), (96, 96), (20, 128)]
    assert mc.FUSED_PAIRS == [(32, 32), (20, 17), (48, 48), (36, 33), (64, 64), (52, 49)] and mc.POOL_TILES == (10, 7, 19)
    assert len(mc.CONV_CASES) == 4 * (9 + 6 + 10) and mc.BATCH == 3
    # every kernel form: conv3 / stem m-blocks 1..4, conv1 m-blocks 1, 2, 3, 4, 6, 8, both conv1 kernels
    f = [mc.conv_facts(k, ci, co, mc.tiles_of(k, ci, co)[-1]) for k, ci, co, v in mc.CONV_CASES if v == 'none']
    kinds = [k for k, _, _, v in mc.CONV_CASES if v == 'none']
    # (conv3_f32<2> alone: the pairs of section 3 that must not fuse, and every FPL_F32_UNFUSED run of a 32-wide pair)
    assert {x['mb'] for x, k in zip(f, kinds) if k == 'conv3'} == {1, 3, 4}
    assert any(mc._mb(c[1]) == 2 for c in mc.UNFUSED_CASES) and any(mc._mb(c[1]) == 2 for c in mc.FUSED_CASES)
    assert {x['mb'] for x, k in zip(f, kinds) if k == 'stem'} == {1, 2, 3, 4}
    assert {x['mb'] for x, k in zip(f, kinds) if k == 'conv1'} == {1, 2, 3, 4, 6, 8}
    assert {x['wreg'] for x, k in zip(f, kinds) if k == 'conv1'} == {True, False}
    assert max(x['chunks'] for x in f) == 12 and {x['slices'] for x in f} == {1, 2, 3}
    assert any(x['ragged_cin'] for x in f) and any(x['ragged_cout'] for x in f)


# ---- 1. convolutions --------------------------------------------------------------------------
def _check_conv_case(kind, cin, cout, variant, tile, lifts=None):
    c = mc.conv_case(kind, cin, cout, variant, tile, lifts)
    k = 1 if kind == 'conv1' else 3
    od = tile - k + 1
    assert c['x'].shape == (3, tile, tile, tile, 1) and c['K'] == k ** 3 * cin + 2
    assert c['ref'].shape == c['bound'].shape == (3, od, od, od, cout) and c['ref'].dtype == np.float64
    assert c['h'].dtype == np.float32 and c['h'].shape[-1] == cin
    ops = c['graph'].lower_inference()[0]
    convs = [o for o in ops if o['kind'] == 0]
    assert (convs[-1]['k'], convs[-1]['cin'], convs[-1]['cout']) == (k, cin, cout)
    assert convs[-1]['act'] == {'none': 0, 'bias': 0, 'relu': 1, 'bn_relu': 1, 'sigmoid': 2}[variant]
    # the composed reference is the float64 oracle of the whole graph up to the lifts' one rounding
    full = cnn_oracle.graph_forward(c['graph'], c['x'], dtype=torch.float64)
    slack = U * c['mag'] * np.abs(c['scale']) * 1.0001 + 1e-15
    assert np.all(np.abs(full - c['ref']) <= (slack if cin > 1 else 1e-12))
    # not too tight: the oracle's own float32 forward is inside.  With BatchNorm the oracle does not
    # fold: it rounds (c - mean) / sqrt(var + eps) * gamma + beta step by step, six roundings on
    # magnitudes the folded form never sees; those are allowed on top, for the oracle alone
    err = np.abs(_f32(c) - c['ref'])
    allow = c['bound']
    if variant == 'bn_relu':
        bn = c['graph'].nodes[c['conv'].idx + 1]
        gm, bt, mu, var = (c['graph'].weights[s].astype(np.float64) for s in bn.weight_slots)
        allow = allow + 8 * U * (np.abs(c['scale']) * (c['mag'] + np.abs(mu)) + np.abs(bt))
    elif variant == 'sigmoid':
        allow = allow + 4 * U                                # torch's own sigmoid: a few ulp of a value < 1
    assert np.all(err <= allow), np.max(err / allow)
    # not vacuous: at the median output far below the 1e-3 gate, and a float32 bound all the same
    assert np.median(c['bound']) < 1e-3 * np.abs(c['ref']).max()
    assert np.median(c['bound']) > 1e3 * 2.0 ** -53 * np.median(np.abs(c['ref']) + 1e-30)
    if od > 1 and variant in ('relu', 'bn_relu'):
        assert 0.05 < np.mean(c['ref'] > 0) < 0.95                  # the clamp acts, and not everywhere
    return c


@pytest.mark.parametrize('kind,cin,cout,variant', mc.CONV_CASES + [mc.SIGMOID_CASE])
def test_conv_case_is_what_it_says(kind, cin, cout, variant):
    tiles = (mc.SIGMOID_TILE,) if variant == 'sigmoid' else mc.tiles_of(kind, cin, cout)
    for tile in tiles:
        c = _check_conv_case(kind, cin, cout, variant, tile)
        f = mc.conv_facts(kind, cin, cout, tile)
        want = {'mfma_conv1_f32': len(mc.lifts_of(cin))}
        name = {'conv3': 'mfma_conv3_f32', 'stem': 'mfma_stem_f32', 'conv1': 'mfma_conv1_f32'}[kind]
        want[name] = want.get(name, 0) + f['slices']
        assert c['launches'] == {k: v for k, v in want.items() if v}
        if kind == 'conv3':
            assert f['blocks'] == {3: (1, 1, 1), 7: (2, 2, 1), 19: (5, 5, 2)}[tile]
            assert f["idle_waves"] and f['chunks'] <= 12
        elif kind == 'stem':
            assert f['blocks'] == {3: (1, 1, 1), 11: (3, 2, 1), 67: (17, 9, 2)}[tile]
        else:
            assert f['groups'][1] == {1: 1, 3: 2, 5: 8}[tile] and f['tail'][1] == {1: 1, 3: 11, 5: 13}[tile]
            assert f['groups'][3] == {1: 1, 3: 6, 5: 24}[tile] and f['tail'][3] == {1: 3, 3: 1, 5: 7}[tile]
    if cin >= 96 and kind == 'conv3':
        assert tiles == (7,)


@pytest.mark.parametrize('kind,cin,cout,tile,lifts', mc.DECLINED_CASES + mc.NEIGHBOUR_CASES)
def test_declined_programs_and_their_neighbours(kind, cin, cout, tile, lifts):
    c = _check_conv_case(kind, cin, cout, 'bias', tile, lifts)
    declined = (kind, cin, cout, tile, lifts) in mc.DECLINED_CASES
    assert (c['launches'] is None) == declined and mc.supported(c['graph']) == (not declined)
    if lifts:
        assert (lifts[0] % 16 != 0) == declined and c['graph'].lower_inference()[0][-2]['kind'] == 4   # a concat


@pytest.mark.parametrize('kind,cin,cout,tile', [('conv3', 17, 33, 7), ('stem', 1, 17, 11), ('conv1', 49, 48, 3),
                                                ('conv3', 48, 65, 7)])
def test_a_corrupted_convolution_reference_is_far_outside_the_bound(kind, cin, cout, tile):
    """the float32 oracle stands in for a correct kernel: against a reference with two taps
    transposed, or with (ci, co) permuted, it misses the bound by orders of magnitude"""
    c = mc.conv_case(kind, cin, cout, 'none', tile)
    good = _f32(c)
    w = c['w'].astype(np.float64)
    bad = []
    if kind != 'conv1':
        t = w.copy()
        t[0, 1, 2], t[2, 1, 0] = w[2, 1, 0], w[0, 1, 2]
        bad.append(t)
    if cin > 1:
        t = w.copy()
        t[..., 0, :], t[..., cin - 1, :] = w[..., cin - 1, :], w[..., 0, :]
        bad.append(t)
    if cout > 1:
        bad.append(np.roll(w, 1, axis=-1))
    assert len(bad) >= 2
    assert np.all(np.abs(good - c['ref']) <= c['bound'])
    for t in bad:
        ratio = np.max(np.abs(good - _conv64(c['h'], t)) / c['bound'])
        print(kind, cin, cout, "corrupted reference: err / bound %.3g" % ratio)
        assert ratio > 10, ratio


# ---- 2. taps ----------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,cin,cout,tile,points', mc.TAP_CASES)
def test_tap_case_is_what_it_says(kind, cin, cout, tile, points):
    g, W = mc.tap_case(kind, cin, cout, tile)
    od = tile - 2
    assert mc.predict_launches(g) == ({'mfma_stem_f32': 1} if kind == 'stem' else
                                      {'mfma_conv1_f32': 1, 'mfma_conv3_f32': -(-cout // 64)})
    edge = (4, 8, 64) if kind == 'stem' else (4, 4, 16)
    lits = []
    for p in points:
        x = np.zeros((1, tile, tile, tile, 1), np.float32)
        x[(0,) + p + (0,)] = 1.0
        want, lit = mc.tap_want(W, tile, p)
        lits.append(lit)
        # the oracle agrees: exactly (one product with 1.0 and zeros)
        assert np.array_equal(cnn_oracle.graph_forward(g, x, dtype=torch.float64), want.astype(np.float64))
        assert np.count_nonzero(want) == lit * cout
        # corrupted expectation: two taps transposed, or the first input channel's weights
        Wt = W.copy()
        Wt[0, 1, 2], Wt[2, 1, 0] = W[2, 1, 0].copy(), W[0, 1, 2].copy()
        if lit == 27:
            assert not np.array_equal(mc.tap_want(Wt, tile, p)[0], want)
        if cin > 1:
            assert not np.array_equal(mc.tap_want(W[:, :, :, ::-1], tile, p)[0], want)
        assert not np.array_equal(mc.tap_want(W[..., ::-1], tile, p)[0], want)
    assert lits == [1, 1, 27, 27]
    # the third voxel's outputs end on the first block's last plane / row / column, the fourth's straddle it
    a, b = points[2], points[3]
    for ax in range(3):
        if edge[ax] < od:
            assert a[ax] == edge[ax] - 1 and b[ax] == edge[ax]
    assert any(edge[ax] < od for ax in range(3))


# ---- 3. conv3 -> conv1 (-> pool) --------------------------------------------------------------
ALL_CHAINS = mc.FUSED_CASES + mc.UNFUSED_CASES + mc.STEM_FUSED_CASES + mc.STEM_UNFUSED_CASES


@pytest.mark.parametrize('case', ALL_CHAINS, ids=lambda c: '-'.join(str(v) for v in c if v != ''))
def test_chain_case_is_what_it_says(case):
    cin, c3, c1, act, pool, flavour = case
    for tile in mc.POOL_TILES:
        c = mc.fused_case(*case, tile=tile)
        od = tile - 2
        assert c['ref'].shape == c['bound'].shape == (3,) + ((od // pool if pool else od),) * 3 + (c1,)
        full = cnn_oracle.graph_forward(c['graph'], c['x'], dtype=torch.float64) if pool != 3 else None
        if full is not None:                                  # (the oracle's pool is MaxPooling3D(2))
            assert np.all(np.abs(full - c['ref']) <= c['bound'] * 1e-3 + 1e-12)
            err = np.abs(_f32(c) - c['ref'])
            allow = c['bound'] + (4 * U if flavour == 'sigmoid' else 0)
            assert np.all(err <= allow), np.max(err / allow)
        assert np.median(c['bound']) < 1e-3 * np.abs(c['ref']).max()
        if act == 'relu' and flavour == '':
            assert 0.05 < np.mean(c['ref'] > 0) < 0.95
        fused = case in mc.FUSED_CASES or case in mc.STEM_FUSED_CASES
        names = set(c['launches'] or ())
        assert fused == bool(names & {'mfma_conv3_conv1_f32', 'mfma_conv3_conv1_pool_f32', 'mfma_stem_conv1_pool_f32'})
        if pool != 3:
            assert not set(c['launches_unfused']) & {'mfma_conv3_conv1_f32', 'mfma_conv3_conv1_pool_f32',
                                                     'mfma_stem_conv1_pool_f32'}
            assert fused == (c['launches'] != c['launches_unfused'])
    if pool == 2:
        assert (7 - 2) % 2 == 1 and (19 - 2) % 2 == 1 and (10 - 2) % 2 == 0     # odd conv extents are met


def test_a_corrupted_chain_reference_is_far_outside_the_bound():
    c = mc.fused_case(mc.FUSE_CIN, 20, 17, 'relu', 2, '', tile=10)
    good = _f32(c)
    assert np.all(np.abs(good - c['ref']) <= c['bound'])
    g2 = LayerGraph(10)
    g2.nodes, g2.output = c['graph'].nodes, c['graph'].output
    w = [a.copy() for a in c['graph'].weights]
    w[3] = np.roll(w[3], 1, axis=-2)                          # the conv1's input channels permuted
    g2.weights = w
    bad = cnn_oracle.graph_forward(g2, c['x'], dtype=torch.float64)
    assert np.max(np.abs(good - bad) / c['bound']) > 1e3


# ---- 4. exact cases ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', mc.EXACT_CASES)
def test_exact_case_is_exact(name):
    c = mc.exact_case(name)
    x, want = c['x'], c['want']
    assert want.dtype == np.float32 and x.shape[0] == 3 and len(set(x.shape[1:4])) == 1
    for w in (_W5, _W7, np.abs(_W5), mc._dyadic(32)):
        assert lift_is_exact(x, w)
    # the float64 oracle of the whole graph round-trips through float32: nothing was rounded
    full = cnn_oracle.graph_forward(c['graph'], x, dtype=torch.float64)
    assert np.array_equal(full, want.astype(np.float64))
    # every convolution's partial sums, in any order, are integers of the granule below 2^24
    assert bool(c['stages']) == (not name.startswith('pool'))
    for h, w in c['stages']:
        for a in (h, w):
            q = a.astype(np.float64) / mc.GRANULE
            assert np.array_equal(q, np.round(q))
        assert np.array_equal(w, np.round(w)) and np.abs(w).max() <= 2 and len(np.unique(w)) >= 3
        assert _conv64(np.abs(h), np.abs(w)).max() / mc.GRANULE < 2 ** 24
    assert len(np.unique(want)) > 20
    # a corrupted expectation fails array_equal: the output channels, or the two halves of a concat
    assert not np.array_equal(want[..., ::-1], want)
    if name.startswith('cat'):
        _, first, _, c0, c1 = name.split('_')
        c0, c1 = int(c0), int(c1)
        h, w = c['stages'][-1]
        assert h.shape[-1] == c0 + c1 and c0 % 16 == 0
        swapped = np.concatenate([h[..., c0:], h[..., :c0]], axis=-1) if c0 != c1 else h[..., ::-1]
        assert not np.array_equal(_conv64(swapped, w).astype(np.float32), want)
        assert (c1 % 16 != 0) == (name in ('cat_skip_up_16_5', 'cat_skip_up_32_24', 'cat_up_skip_16_24', 'cat_up_skip_32_5'))
    if name.startswith('pool'):
        assert x.max() < 0 and want.max() < 0 and want.shape[1:] == (int(name[4]) // 2,) * 3 + (5,)
    if name.startswith('add'):
        assert (want < 0).any() == (name == 'add') and (want > 0).any()
    if name.startswith('crop') or name == 'up2':
        h, w = c['stages'][-1]
        t = w.copy()
        t[0, 1, 2], t[2, 1, 0] = w[2, 1, 0].copy(), w[0, 1, 2].copy()
        assert not np.array_equal(_conv64(h, t).astype(np.float32), want)
