"""tests/perop_cases.py on the CPU: every named case of test_gpu_perop.py, test_gpu_lattice_exact.py
and test_gpu_hist_crop.py exercises what its name says, the references agree with the project's
oracles, and the constants the cases restate are the kernels'."""
import os
import re

import numpy as np
import pytest
import torch

from flypylib_amd.program import OP_CONCAT, OP_CROP, OP_POOL, OP_UP
from oracle import cnn_oracle
from tests import perop_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source(name):
    with open(os.path.join(ROOT, 'flypylib_amd', 'csrc', name)) as f:
        return f.read()


# ---- 1. convolutions --------------------------------------------------------------------------
def test_gamma_is_the_standard_constant():
    assert pc.gamma(1) == pytest.approx(2.0 ** -24, rel=1e-6)
    assert pc.gamma(27 * 96 + 1) == pytest.approx(2593 * 2.0 ** -24, rel=1e-3)
    assert pc.U == np.finfo(np.float32).eps / 2 and pc.TINY == float(np.finfo(np.float32).tiny)


@pytest.mark.parametrize('k,cin,cout,variant', pc.CONV_CASES + [pc.SIGMOID_CASE])
def test_conv_case_is_what_it_says(k, cin, cout, variant):
    c = pc.conv_case(k, cin, cout, variant)
    g, x = c['graph'], c['x']
    ext = pc.CONV_EXTENTS[k]
    assert len(set(ext)) == 3 and x.shape == (pc.BATCH,) + ext + (1,) and pc.BATCH == 2
    assert c['K'] == k ** 3 * cin + 1
    ops = g.lower_inference()[0]
    assert len(ops) == (1 if cin == 1 else 2) and (ops[-1]['k'], ops[-1]['cin'], ops[-1]['cout']) == (k, cin, cout)
    assert ops[-1]['act'] == {'none': 0, 'bias': 0, 'relu': 1, 'bn_relu': 1, 'sigmoid': 2}[variant]
    # both forms of conv_direct.h are met: 16 output channels per thread, and one
    assert (cout % 16 == 0) == ((cin, cout) in [(1, 48), (48, 48), (32, 64)])
    out_ext = tuple(s - k + 1 for s in ext)
    assert c['ref'].shape == c['bound'].shape == (pc.BATCH,) + out_ext + (cout,)
    assert c['ref'].dtype == np.float64 and np.all(c['bound'] >= pc.TINY) and c['ref'].std() > 1e-3
    if variant in ('relu', 'bn_relu'):
        frac = np.mean(c['ref'] > 0)
        assert 0.1 < frac < 0.9                                     # the clamp acts, and not everywhere
    if variant in ('bias', 'sigmoid'):
        assert np.abs(g.weights[c['conv'].weight_slots[1]]).min() > 0
    # the input of the convolution under test: the oracle's float32 lift IS the correctly rounded product
    if cin > 1:
        w1 = g.weights[c['lift'].weight_slots[0]].reshape(-1)
        assert np.array_equal(c['h'], pc.np_lift(x, w1))
    # ... and the composed reference is the float64 oracle of the whole graph, up to that one rounding
    # of the lift: |d ref| <= u * (|h| (*) |w|), times the BN scale, a quarter of it behind the sigmoid
    full = cnn_oracle.graph_forward(g, x, dtype=torch.float64)
    slack = pc.U * c['mag'] * 1.0001 + 1e-15
    if variant == 'bn_relu':
        bn = g.nodes[c['conv'].idx + 1]
        gm, _, _, var = (g.weights[s].astype(np.float64) for s in bn.weight_slots)
        slack = slack * np.abs(gm / np.sqrt(var + 1e-3))
    assert np.all(np.abs(full - c['ref']) <= (slack if cin > 1 else 1e-12))
    # the bound is a float32 bound: far above the float64 reference's own error
    assert np.median(c['bound']) > 1e3 * 2.0 ** -53 * np.median(np.abs(c['ref']) + 1e-30)


# ---- 1b. exact ops ----------------------------------------------------------------------------
@pytest.mark.parametrize('name', pc.EXACT_CASES)
def test_exact_case_is_what_it_says(name):
    g, x, want = pc.exact_case(name)
    ext = x.shape[1:4]
    assert len(set(ext)) == 3 and x.shape[0] == 2 and want.dtype == np.float32
    ops = g.lower_inference()[0]
    kinds = [o['kind'] for o in ops]
    # the project's float64 oracle agrees with the numpy restatement where it has the op
    if name != 'pool3':
        assert np.array_equal(cnn_oracle.graph_forward(g, x, dtype=torch.float64), want.astype(np.float64)) \
            or name.startswith('add')
    if not name.startswith('add'):
        for w in (pc._W5, pc._W7):
            assert pc.lift_is_exact(x, w)
    if name.startswith('pool'):
        f = ops[-1]['p'][0]
        assert kinds[-1] == OP_POOL and f == (3 if name == 'pool3' else 2)
        odd = [s % f for s in ext]
        assert (not any(odd)) if name == 'pool2_even' else any(odd)           # floor pooling drops a remainder
        assert want.shape[1:4] == tuple(s // f for s in ext) and want.shape[4] == 5
        if name == 'pool2_negative':
            assert x.max() < 0 and want.max() < 0 and np.isfinite(want).all()
        else:
            assert (want > 0).any() and len(np.unique(want)) > 20
    elif name.startswith('crop'):
        c = int(name[-1])
        assert kinds[-1] == OP_CROP and want.shape[1:4] == tuple(s - 2 * c for s in ext)
    elif name.startswith('up'):
        assert kinds[-1] == OP_UP and tuple(ops[-1]['p'][:3]) == ((2, 2, 2) if name == 'up2' else (1, 2, 3))
    elif name.startswith('concat'):
        assert kinds[-1] == OP_CONCAT and want.shape[4] == 12
        a, b = ops[-1]['src0'], ops[-1]['src1']
        ch = {o['dst']: o['cout'] for o in ops}
        assert (ch[a], ch[b]) == ((5, 7) if name == 'concat_skip_up' else (7, 5))
        # the halves differ, so a wrong channel offset cannot pass
        assert not np.array_equal(want[..., :5], want[..., 5:10]) and not np.array_equal(want[..., :5], want[..., 7:])
    else:
        # float32 addition that ROUNDS: not equal to the float64 sum of the addends everywhere
        a = pc.np_lift(x, g.weights[0].reshape(-1)).astype(np.float64)
        b = pc.np_lift(x, g.weights[1].reshape(-1)).astype(np.float64)
        s = np.maximum(a + b, 0) if name == 'add_relu' else a + b
        assert np.mean(s != want) > 0.2 and np.max(np.abs(s - want)) <= pc.U * np.max(np.abs(s))
        assert ops[-1]['act'] == (1 if name == 'add_relu' else 0)


def test_factories_are_all_of_fplmodels():
    from flypylib_amd import fplmodels
    import inspect
    public = {n for n, f in inspect.getmembers(fplmodels, inspect.isfunction)
              if not n.startswith('_') and f.__module__ == fplmodels.__name__}
    assert {n for n, _ in pc.FACTORIES} == public
    assert all(s <= 62 for _, s in pc.FACTORIES)


def test_noncubic_lattice_has_partial_tiles_on_every_axis():
    from oracle import infer_oracle
    c = pc.NONCUBIC
    assert len(set(c['tile'])) == 3 and all((t - 14) % 4 == 0 for t in c['tile'])
    _, start, end = infer_oracle.tile_lattice(c['vol'], c['tile'], c['off'])
    ext = end - start
    assert ext.shape[1] == 27 and np.any(np.all(ext < np.asarray(c['tile'])[:, None], axis=0))


# ---- 2. lattice -------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(pc.LATTICE))
def test_lattice_case_is_what_it_says(name):
    c = pc.LATTICE[name]
    assert max(c['vol']) <= 40 and len(set(c['alt'])) == 3
    for tile in ((c['tile'],) * 3, c['alt']):
        f = pc.lattice_facts(name, tile)
        assert f['ragged_on_all_axes'] and f['n_tiles'] >= 4, (tile, f)
        assert all((t - 2 * c['off']) % c['stride'] == 0 for t in tile)
    assert pc.lattice_facts(name)['z_rows'] >= 3                       # three non-empty rank slabs
    ops = pc.lattice_graph(name).lower_inference()[0]
    assert [o['kind'] for o in ops] == {'P1': [OP_CROP, 0], 'P2': [OP_POOL, OP_CROP, 0], 'P3': [OP_POOL, OP_POOL, 0]}[name[:2]]
    for source in pc.SOURCES:
        ref = pc.lattice_reference(name, source)
        _, mean, std, img = pc.lattice_source(name, source)
        assert ref.dtype == np.float32 and ref.shape == c['vol']
        # these programs' results do not depend on the tiling: the four routes can be held to one another
        assert np.array_equal(ref, pc.lattice_reference(name, source, c['alt']))
        off = c['off']
        if off:
            assert not ref[:off].any() and not ref[:, :, -off:].any()
        inner = ref[off:c['vol'][0] - off, off:c['vol'][1] - off, off:c['vol'][2] - off]
        assert np.count_nonzero(inner) > 0.5 * inner.size
        if source != 'f32':
            # the normalisation rounds twice: it is neither the float64 value rounded once nor x * (1 / std)
            u8 = pc.lattice_source(name, source)[0].astype(np.float64)
            once = ((u8 - mean) / std).astype(np.float32)
            recip = (pc.lattice_source(name, source)[0].astype(np.float32) - np.float32(mean)) * (np.float32(1) / np.float32(std))
            assert (img != recip).any()
            if source == 'u8_127.3_0.1':
                assert (img != once).any()
            assert img.min() < -1 and img.max() > 1
    if name == 'P3':
        for source in pc.SOURCES:
            # a pooled window straddles the padding edge, and the padding (0 in the NORMALISED domain) wins it
            _, mean, std, img = pc.lattice_source(name, source)
            ref, nopad = pc.lattice_reference(name, source), pc.p3_ignoring_the_padding(img)
            won = ref != nopad
            assert any(s % 4 for s in c['vol']) and won.any() and not ref[won].any() and (nopad[won] < 0).all()
            if source != 'f32':
                assert np.float32(-mean) / np.float32(std) < nopad.min()       # ... where -mean / std never would


@pytest.mark.parametrize('name', sorted(pc.LATTICE))
def test_thin_volumes(name):
    c = pc.LATTICE[name]
    vols = pc.thin_volumes(name)
    assert len(vols) == (6 if c['off'] else 3)
    for label, vol in vols.items():
        f = pc.lattice_facts(name, vol=vol)
        axis = int(label[-1])
        if label.startswith('none'):
            assert vol[axis] <= 2 * c['off'] and f['n_tiles'] == 0
            assert not pc.lattice_reference(name, 'f32', vol=vol).any()
        else:
            assert vol[axis] == 2 * c['off'] + 1 and f['n_tiles'] >= 1
            assert len(range(c['off'], vol[axis] - c['off'], c['tile'] - 2 * c['off'])) == 1
            assert pc.lattice_reference(name, 'f32', vol=vol).any()


# ---- 3. hist_u8 / crop_u8 ---------------------------------------------------------------------
def test_constants_are_the_kernels():
    src = _source('synth.hip')
    assert re.search(r'constexpr int SYN_PER_WG = 256 \* 4;', src) and pc.SYN_PER_WG == 1024
    assert re.search(r'ceil_div64\(n / 16, 256\), \(int64_t\)ctx->n_cu \* 8\)', src)
    assert 'source must be 16-byte aligned' in src


@pytest.mark.parametrize('n_cu', [1, 64, 256, 304])
def test_hist_sizes_reach_every_part_of_the_kernel(n_cu):
    s = pc.hist_sizes(n_cu)
    f = {k: pc.hist_facts(n, n_cu) for k, n in s.items()}
    assert s['0'] == 0 and f['0']['blocks'] == 1
    for k in ('1', '15'):                                              # n < 16: the remainder loop alone
        assert f[k]['vectors'] == 0 and f[k]['remainder'] == s[k]
    assert (f['16']['vectors'], f['16']['remainder']) == (1, 0)
    assert (f['17']['vectors'], f['17']['remainder']) == (1, 1)
    assert (f['one_block_less_1']['blocks'], f['one_block_less_1']['remainder']) == (1, 15)
    # 16 * 256 * G + 5: the capped grid, every thread one vector, five bytes for block 0 - no stride yet
    assert s['one_pass_5'] == 16 * 256 * n_cu * 8 + 5
    assert f['one_pass_5'] == dict(vectors=256 * 8 * n_cu, remainder=5, blocks=8 * n_cu, passes=1, capped=False)
    # ... 300 vectors more: a second, partial pass over the grid
    g = f['strided_5']
    assert g['remainder'] == 5 and g['capped'] and g['passes'] == 2 and g['vectors'] % (g['blocks'] * 256) == 300
    assert s['strided_5'] < 10 << 20 or n_cu > 256
    for kind in ('random', 'constant', 'even_only'):
        v = pc.hist_data(kind, 4000)
        h = np.bincount(v, minlength=256)
        assert h.sum() == 4000
        assert {'random': (h > 0).all(), 'constant': h[255] == 4000, 'even_only': not h[1::2].any() and (h[::2] > 0).all()}[kind]


def test_crop_boxes_reach_every_part_of_the_kernel():
    boxes = pc.CROP_BOXES
    facts = {k: pc.crop_facts(*b) for k, b in boxes.items()}
    src = pc.crop_source()
    assert src.shape == pc.CROP_EXTENT and src.min() > 0
    assert {b[0][2] for b in boxes.values()} >= {1, 2, 3, 5, 13, 36, 64}
    assert all(len(set(b[0])) == 3 for b in boxes.values())
    f = facts['d2_1_inside']
    assert f['max_rows'] == 4 and f['fast'] == 0 and f['tail'] == 3 and f['crosses_plane'] > 0
    assert facts['d2_2_leaves_z_low']['max_rows'] == 2 and facts['d2_2_leaves_z_low']['leaves'] == {'z_low'}
    f = facts['d2_3_leaves_z_high']
    assert f['max_rows'] == 2 and f['leaves'] == {'z_high'} and f['fast'] == 0
    f = facts['d2_5_leaves_y_low']
    assert f['leaves'] == {'y_low'} and f['tail'] == 1 and f['fast'] > 0 and f['slow'] > 0 and f['crosses_plane'] > 0
    f = facts['d2_13_leaves_y_high_two_chunks']
    assert f['leaves'] == {'y_high'} and f['chunks'] == 2 and f['chunk_base_mid_row'] and f['tail'] == 2
    assert f['fast_odd_address'] > 0 and f['fast'] > f['fast_odd_address']
    f = facts['d2_36_leaves_x_low']
    assert f['leaves'] == {'x_low'} and f['fast'] > 0 and f['slow'] > 0
    f = facts['d2_64_leaves_x_high']
    assert f['leaves'] == {'x_high'} and f['fast'] > 0 and f['slow'] > 0          # a chunk half inside the source row
    f = facts['d2_36_inside_two_chunks']
    assert not f['leaves'] and f['chunks'] == 2 and f['chunk_base_mid_row'] and f['slow'] == 0
    assert f['fast_odd_address'] > 0 and f['inside_voxels'] == f['n']
    for k in ('outside_high', 'outside_low'):
        assert facts[k]['inside_voxels'] == 0 and facts[k]['fast'] == 0
        assert not pc.crop_reference(src, *boxes[k]).any()
    assert facts['all_faces']['leaves'] == {'z_low', 'z_high', 'y_low', 'y_high', 'x_low', 'x_high'}
    union = set().union(*(f['leaves'] for k, f in facts.items() if k != 'all_faces'))
    assert len(union) == 6                                              # each face alone, too
    for k, (dims, origin) in boxes.items():
        want = pc.crop_reference(src, dims, origin)
        assert np.count_nonzero(want) == facts[k]['inside_voxels']     # the source has no zero: zeros are padding
        # the reference against the plainest statement of the operation
        for z, y, x in [(0, 0, 0), tuple(d - 1 for d in dims), tuple(d // 2 for d in dims)]:
            g = (z + origin[0], y + origin[1], x + origin[2])
            inside = all(0 <= gg < e for gg, e in zip(g, pc.CROP_EXTENT))
            assert want[z, y, x] == (src[g] if inside else 0)
