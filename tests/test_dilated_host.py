"""Conv3D(filters, 3, dilation_rate=2) on the host: the three float64 restatements against each
other, the graph API, both lowerings, the Keras interchange file and the compiler's resource
report of the new kernels.  Nothing here needs a GPU."""
import json
import os
import re

import numpy as np
import pytest
import torch

from flypylib_amd import _capi, keras_io
from flypylib_amd.program import (ACT_NONE, ACT_RELU, L_BN, L_CONV, L_DILATED, OP_CONV, OP_DILATED, LayerGraph,
                                  lower_training)
from tests import dilated_cases as di

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPATIAL = [(5, 5, 5), (6, 9, 8), (9, 6, 21)]
CHANNELS = [(1, 4), (3, 5), (16, 16), (17, 33), (48, 32)]


@pytest.mark.parametrize('spatial', SPATIAL)
@pytest.mark.parametrize('cin,cout', CHANNELS)
def test_the_three_restatements_agree(spatial, cin, cout):
    """(a) torch conv3d(dilation=2), (b) 27 einsums over shifted views and (c) the plain 3x3x3 on the
    eight parity classes: float64 round-off.  |x|, |W| ~ 1 and at most 27 * 48 terms: a sum of 1296
    products of order 1 rounds to about sqrt(1296) * 2^-53 * 20 ~ 8e-14; 1e-12 is an order above."""
    rng = np.random.default_rng(cin * 100 + cout)
    for n in (1, 3):
        x = rng.standard_normal((n,) + spatial + (cin,))
        k = rng.standard_normal((3, 3, 3, cin, cout))
        b = rng.standard_normal(cout)
        a = di.conv_dilated64(torch.as_tensor(x).permute(0, 4, 1, 2, 3), torch.as_tensor(k),
                              torch.as_tensor(b)).permute(0, 2, 3, 4, 1).numpy()
        ref = di.dilated_numpy(x, k, b)
        sub = di.sublattice_numpy(x, k, b)
        assert a.shape == ref.shape == sub.shape == (n,) + tuple(s - 4 for s in spatial) + (cout,)
        assert np.max(np.abs(a - ref)) < 1e-12 and np.max(np.abs(sub - ref)) < 1e-12
        assert np.abs(ref).max() > 1.0


def test_graph_api_sizes_weights_and_params():
    g = LayerGraph((9, 10, 12), seed=1)
    x = g.conv(g.input(), 5, 3)                           # (7, 8, 10)
    d = g.dilated(x, 7, use_bias=True, activation='relu')
    assert d.kind == 'dilated' and d.channels == 7 and d.size == (3, 4, 6)
    assert d.attrs == dict(k=3, d=2, use_bias=True, activation='relu')
    assert [g.weights[s].shape for s in d.weight_slots] == [(3, 3, 3, 5, 7), (7,)]
    assert [g.weight_names[s] for s in d.weight_slots] == ['dilated_2/kernel', 'dilated_2/bias']
    assert g.count_params() == 27 * 5 + 27 * 5 * 7 + 7 == g.count_trainable()
    kern = g.weights[d.weight_slots[0]]
    lim = np.sqrt(6.0 / (27 * 5 + 27 * 7))                # glorot_uniform, fans 27 * cin and 27 * cout
    assert np.abs(kern).max() <= lim and np.abs(kern).max() > 0.8 * lim and not g.weights[d.weight_slots[1]].any()
    nb = g.dilated(x, 3)
    assert len(nb.weight_slots) == 1 and nb.attrs['use_bias'] is False and nb.attrs['activation'] is None
    fc = LayerGraph(None)
    assert fc.dilated(fc.input(), 2).size is None
    lines = []
    g.finish(d).summary(lines.append)
    assert any(re.match(r'2\s+dilated\s', l) and l.rstrip().endswith(str(27 * 5 * 7 + 7)) for l in lines)
    w = g.get_weights()
    w[d.weight_slots[0]] = w[d.weight_slots[0]] + 1
    g.set_weights(w)
    assert np.array_equal(g.weights[d.weight_slots[0]], kern + 1)
    assert di.tiny_atrous()[0].output.size == (12, 12, 12) and di.tiny_atrous()[1] == (11, 5, 1)


@pytest.mark.parametrize('kw', [dict(kernel_size=2), dict(kernel_size=5), dict(kernel_size=1), dict(dilation_rate=1),
                                dict(dilation_rate=3), dict(kernel_size=(3, 3, 2)), dict(dilation_rate=(2, 1, 2))])
def test_other_kernels_and_dilations_are_refused(kw):
    g = LayerGraph((8, 8, 8))
    with pytest.raises(ValueError, match='dilated: only kernel_size 3 with dilation_rate 2') as e:
        g.dilated(g.input(), 4, **kw)
    # both values are named
    assert repr(kw.get('kernel_size', 3)) in str(e.value) and repr(kw.get('dilation_rate', 2)) in str(e.value)
    g.dilated(g.input(), 4, kernel_size=3, dilation_rate=(2, 2, 2))


def test_other_activations_and_an_axis_below_five_are_refused():
    g = LayerGraph((8, 8, 8))
    for act in ('sigmoid', 'tanh'):
        with pytest.raises(ValueError, match='dilated: activation'):
            g.dilated(g.input(), 4, activation=act)
    for size in ((4, 8, 8), (8, 4, 8), (8, 8, 4), (1, 5, 5)):
        g = LayerGraph(size)
        with pytest.raises(ValueError, match='dilated'):
            g.dilated(g.input(), 4)
    g = LayerGraph((5, 6, 7))
    assert g.dilated(g.input(), 4).size == (1, 2, 3)


def _run_folded(graph, x):
    """the lowered op list through (b) for the dilated op and numpy for a leading 1x1x1 conv; float64"""
    ops, arena, out_t, n_t = graph.lower_inference()
    arena64 = arena.astype(np.float64)
    t = {0: np.asarray(x, np.float64)}
    for o in ops:
        s, h = arena64[o['scale_off']:o['scale_off'] + o['cout']], arena64[o['shift_off']:o['shift_off'] + o['cout']]
        if o['kind'] == OP_CONV:
            assert o['k'] == 1
            w = arena64[o['w_off']:o['w_off'] + o['cin'] * o['cout']].reshape(o['cin'], o['cout'])
            y = t[o['src0']] @ w * s + h
        else:
            assert o['kind'] == OP_DILATED == 8 and o['k'] == 3 and tuple(o['p']) == (2, 2, 2, 0, 0, 0)
            w = arena64[o['w_off']:o['w_off'] + 27 * o['cin'] * o['cout']].reshape(3, 3, 3, o['cin'], o['cout'])
            y = di.dilated_numpy(t[o['src0']], w) * s + h
        t[o['dst']] = np.maximum(y, 0) if o['act'] == ACT_RELU else y
    return ops, arena, t[out_t]


@pytest.mark.parametrize('bias,relu,bn', [(b, r, n) for b in (0, 1) for r in (0, 1) for n in (0, 1)])
def test_lower_inference_folds_bn_and_relu(bias, relu, bn):
    g, idx = di.dilated_graph(3, 5, bias, relu, bn, (6, 9, 8))
    x = np.random.default_rng(0).standard_normal((2, 6, 9, 8, 1))
    ops, arena, got = _run_folded(g, x)
    assert [o['kind'] for o in ops] == [OP_CONV, OP_DILATED]         # BN and ReLU are gone
    op = ops[1]
    assert op['act'] == (ACT_RELU if relu else ACT_NONE) and (op['cin'], op['cout']) == (3, 5)
    node = g.nodes[idx]
    # the kernel in Keras memory order [27 * cin][cout], untouched
    assert np.array_equal(arena[op['w_off']:op['w_off'] + 27 * 3 * 5], g.weights[node.weight_slots[0]].reshape(-1))
    # the folded scale and shift against float64: y = scale * conv + shift with
    # scale = gamma / sqrt(var + eps), shift = (bias - mean) * scale + beta; stored as fp32, so within
    # 2^-23 relative of the float64 values (one rounding, and the fp32 inputs are exact in float64)
    b64 = g.weights[node.weight_slots[1]].astype(np.float64) if bias else np.zeros(5)
    scale64, shift64 = np.ones(5), b64
    if bn:
        gm, bt, mm, mv = (g.weights[s].astype(np.float64) for s in g.nodes[idx + 1].weight_slots)
        scale64 = gm / np.sqrt(mv + 1e-3)
        shift64 = (b64 - mm) * scale64 + bt
    sc = arena[op['scale_off']:op['scale_off'] + 5].astype(np.float64)
    sh = arena[op['shift_off']:op['shift_off'] + 5].astype(np.float64)
    assert np.all(np.abs(sc - scale64) <= 2.0 ** -23 * np.abs(scale64))
    assert np.all(np.abs(sh - shift64) <= 2.0 ** -23 * np.abs(shift64))
    ref = di.graph_forward64(g, x)
    # fp32 folding of scale and shift: a few 2^-24 relative on values of order 1
    assert got.shape == ref.shape == (2, 2, 5, 4, 5) and np.max(np.abs(got - ref)) < 1e-5 and ref.std() > 1e-2


def test_lower_training_emits_the_layer_with_its_offsets():
    g = di.tiny_atrous()[0]
    layers, arena, offsets, out_t, n_t = lower_training(g)
    assert arena.size == g.count_params() and len(layers) == len(g.nodes) - 1
    first, second = [n for n in g.nodes if n.kind == 'dilated']
    L = layers[first.idx - 1]
    assert L['kind'] == L_DILATED == 11
    assert (L['k'], L['cin'], L['cout'], L['use_bias'], L['act']) == (3, 8, 12, 1, ACT_NONE)
    assert tuple(L['p']) == (2, 2, 2, 0, 0, 0)
    assert L['w_off'][:2] == [offsets[s] for s in first.weight_slots]
    w0 = L['w_off'][0]
    assert np.array_equal(arena[w0:w0 + 27 * 8 * 12], g.weights[first.weight_slots[0]].reshape(-1))
    assert layers[first.idx]['kind'] == L_BN and layers[first.idx]['src0'] == L['dst']
    L2 = layers[second.idx - 1]
    assert L2['kind'] == L_DILATED and (L2['k'], L2['cin'], L2['cout'], L2['use_bias'], L2['act']) == (3, 12, 8, 0, ACT_RELU)
    assert L2['w_off'][0] == offsets[second.weight_slots[0]] and tuple(L2['p']) == (2, 2, 2, 0, 0, 0)
    assert sum(l['kind'] == L_CONV for l in layers) == 3 and sum(l['kind'] == L_DILATED for l in layers) == 2
    # inference: five fused ops, the two layers among them
    ops = g.lower_inference()[0]
    assert [o['kind'] for o in ops] == [OP_CONV, OP_DILATED, OP_DILATED, OP_CONV, OP_CONV]
    assert [o['act'] for o in ops[:3]] == [ACT_RELU] * 3


def _trainable(g):
    return [s for n in g.nodes for s in (n.weight_slots[:2] if n.kind == 'bn' else n.weight_slots)]


def test_keras_file_round_trip(tmp_path):
    g = di.randomize(di.tiny_atrous()[0])
    g.compile(loss='binary_crossentropy', optimizer='adam', metrics=['accuracy'])
    rng = np.random.default_rng(5)
    g.opt_state = ([rng.standard_normal(w.shape).astype(np.float32) for w in g.weights],
                   [rng.random(w.shape).astype(np.float32) for w in g.weights], 17)
    path = str(tmp_path / 'net.keras.h5')
    g.save(path)
    cfg = keras_io.model_config(g)
    f = keras_io.open_h5(path)
    try:
        stored = json.loads(keras_io._text(f.attrs['model_config']))
    finally:
        if hasattr(f, 'close'):
            f.close()
    assert stored == cfg
    assert {l['class_name'] for l in cfg['config']['layers']} == {'InputLayer', 'Conv3D', 'BatchNormalization', 'Activation'}
    convs = [l for l in cfg['config']['layers'] if l['class_name'] == 'Conv3D']
    # Keras numbers by class: the dilated layers are the second and third Conv3D built
    assert [l['name'] for l in convs] == ['conv3d_%d' % i for i in range(1, 6)]
    atrous = [l for l in convs if l['config']['dilation_rate'] == [2, 2, 2]]
    assert [l['name'] for l in atrous] == ['conv3d_2', 'conv3d_3']
    c = atrous[0]['config']
    assert (c['filters'], c['kernel_size'], c['strides'], c['padding'], c['use_bias'], c['activation']) == \
        (12, [3, 3, 3], [1, 1, 1], 'valid', True, 'linear')
    assert c['data_format'] == 'channels_last'
    c = atrous[1]['config']
    assert (c['filters'], c['kernel_size'], c['strides'], c['padding'], c['use_bias'], c['activation']) == \
        (8, [3, 3, 3], [1, 1, 1], 'valid', False, 'relu')
    assert all(l['config']['dilation_rate'] == [1, 1, 1] and l['config']['strides'] == [1, 1, 1]
               for l in convs if l not in atrous)
    tree = keras_io.weight_tree(g)
    assert [w.decode() for w in tree['groups']['conv3d_2']['attrs']['weight_names']] == \
        ['conv3d_2/kernel:0', 'conv3d_2/bias:0']
    assert [w.decode() for w in tree['groups']['conv3d_3']['attrs']['weight_names']] == ['conv3d_3/kernel:0']
    h = di.tiny_atrous(seed=9)[0]
    h.compile(loss='binary_crossentropy', optimizer='adam', metrics=['accuracy'])
    h.load(path)
    for a, b in zip(g.weights, h.weights):
        assert np.array_equal(a, b)
    assert h.opt_state[2] == 17
    for s in _trainable(g):
        assert np.array_equal(h.opt_state[0][s], g.opt_state[0][s]) and np.array_equal(h.opt_state[1][s], g.opt_state[1][s])
    # the .npz pair of save_network likewise
    g.save(str(tmp_path / 'net.weights.npz'))
    h2 = di.tiny_atrous(seed=4)[0]
    h2.load(str(tmp_path / 'net.weights.npz'))
    assert all(np.array_equal(a, b) for a, b in zip(g.weights, h2.weights)) and h2.opt_state[2] == 17
    for s in _trainable(g):
        assert np.array_equal(h2.opt_state[0][s], g.opt_state[0][s])


def test_a_weights_only_file_with_user_named_layers_loads():
    """custom layer names: the (3,3,3,.,.) kernels are dealt, in file order, to the graph's conv and
    dilated nodes together in creation order - one Keras class -, and the shapes are checked"""
    g = di.randomize(di.tiny_atrous()[0])
    roles = {'conv': ['kernel', 'bias'], 'dilated': ['kernel', 'bias'],
             'bn': ['gamma', 'beta', 'moving_mean', 'moving_variance']}
    layers = [('blk%s' % 'abcdefghijklmnopqrstuvwxyz'[n.idx], [(r, g.weights[s]) for r, s in zip(roles[n.kind], n.weight_slots)])
              for n in g.nodes if n.weight_slots]
    assert not any(name.startswith('conv3d') for name, _ in layers)
    got = keras_io.graph_weights_from_layers(di.tiny_atrous(seed=5)[0], layers)
    assert all(np.array_equal(a, b) for a, b in zip(got, g.weights))
    # the two dilated kernels (3,3,3,8,12) and (3,3,3,12,8) swapped in the file: the shape check refuses
    i_a = [i for i, (n, it) in enumerate(layers) if it[0][1].shape == (3, 3, 3, 8, 12)][0]
    i_b = [i for i, (n, it) in enumerate(layers) if it[0][1].shape == (3, 3, 3, 12, 8)][0]
    # (the kernels alone: the first layer keeps its bias, so only the shapes are wrong)
    swapped = list(layers)
    swapped[i_a] = (layers[i_a][0], [layers[i_b][1][0]] + layers[i_a][1][1:])
    swapped[i_b] = (layers[i_b][0], [layers[i_a][1][0]])
    with pytest.raises(ValueError, match='shape'):
        keras_io.graph_weights_from_layers(di.tiny_atrous(seed=5)[0], swapped)


def test_the_header_spells_both_values_and_the_abi_version_is_still_11():
    hdr = open(os.path.join(ROOT, 'include', 'fplhip.h')).read()
    assert int(re.search(r'#define FPL_ABI_VERSION (\d+)', hdr).group(1)) == 11 == _capi.ABI_VERSION
    assert re.search(r'FPL_OP_DILATED = 8\b', hdr) and re.search(r'FPL_L_DILATED = 11\b', hdr)


def test_the_new_kernels_do_not_spill():
    """what the compiler reports for the build's own flags: no spilled register, no scratch"""
    import shutil
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from flypylib_amd.csrc import build
    if not shutil.which(build.HIPCC) and not os.path.exists(build.HIPCC):
        pytest.skip('hipcc not available')
    import kernel_resources
    res = {k: v for k, v in kernel_resources.kernel_resources('conv_mfma_f32.hip').items() if 'atrous3_' in k}
    assert len(res) == 4, sorted(res)                     # atrous3_f32 with 1, 2, 3 and 4 blocks of 16 outputs
    for v in res.values():
        # launch bounds (256, 2): two workgroups a CU, two waves a SIMD, 256 registers each; the
        # tile is dynamic LDS (62208 B, conv3_f32's), nothing static
        assert v['group_segment_fixed_size'] == 0 and v['vgpr_count'] + v['agpr_count'] <= 256, v
    mfma = set(res)
    gen = {k: v for k, v in kernel_resources.kernel_resources('generic.hip').items() if 'atrous3_' in k}
    assert len(gen) == 1, sorted(gen)                     # the per-op kernel of conv_direct.h
    res.update({'generic.hip:' + k: v for k, v in gen.items()})
    res.update({'train.hip:' + k: v for k, v in kernel_resources.kernel_resources('train.hip').items()
                if 'atrous3_' in k})
    # train.hip: the forward (conv_direct.h again), input gradient x 2, the weight-gradient partials
    assert len(res) == 9, sorted(res)
    for name, v in res.items():
        assert v['vgpr_spill_count'] == 0 and v['sgpr_spill_count'] == 0, (name, v)
        assert v['private_segment_fixed_size'] == 0 and (name in mfma or v['vgpr_count'] <= 128), (name, v)
