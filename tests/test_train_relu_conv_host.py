"""Lowering of ReLU-activated convolutions for the training engine (no GPU): unet_like_vol,
the one factory whose convs carry activation='relu', lowers to one L_CONV layer per conv with
act = ACT_RELU; the other nine factories lower as before."""
import numpy as np
import pytest

from flypylib_amd import fplmodels
from flypylib_amd.program import (ACT_NONE, ACT_RELU, ACT_SIGMOID, L_CONCAT, L_CONV, L_CROP,
                                  L_POOL, L_UP, LayerGraph, lower_training)
from tests import relu_conv_cases as rc


def _factories():
    """the model factories of fplmodels: functions returning (graph, rf_info, infer_sz,
    compile_args)"""
    out = {}
    for name in dir(fplmodels):
        f = getattr(fplmodels, name)
        if name.startswith('_') or not callable(f) or getattr(f, '__module__', '') != fplmodels.__name__:
            continue
        try:
            r = f()
        except TypeError:
            continue
        if isinstance(r, tuple) and len(r) == 4 and isinstance(r[0], LayerGraph):
            out[name] = r[0]
    return out


def test_unet_like_vol_lowers_to_relu_convs():
    g = fplmodels.unet_like_vol()[0]
    layers, arena, offsets, out_tensor, n_tensors = lower_training(g)
    assert len(layers) == 17 and n_tensors == 18 and out_tensor == 17
    assert arena.size == g.count_params()
    by_dst = {d['dst']: d for d in layers}
    assert tuple(n.idx for n in rc.relu_convs(g)) == rc.VOL_RELU_NODES
    pairs = {1: (3, 1, 16), 2: (1, 16, 16), 4: (3, 16, 32), 5: (1, 32, 32), 7: (1, 32, 64),
             10: (3, 96, 64), 11: (1, 64, 64), 15: (3, 80, 32), 16: (1, 32, 32)}
    for idx in rc.VOL_RELU_NODES:
        d = by_dst[idx]                                   # tensor id = node index
        assert d['kind'] == L_CONV and d['act'] == ACT_RELU, idx
        assert (d['k'], d['cin'], d['cout']) == pairs[idx], idx
        node = g.nodes[idx]
        assert d['w_off'][0] == offsets[node.weight_slots[0]] and d['use_bias'] == 0
        k, cin, cout = pairs[idx]
        w = arena[d['w_off'][0]:d['w_off'][0] + k ** 3 * cin * cout]
        assert np.array_equal(w, g.weights[node.weight_slots[0]].reshape(-1))
    head = by_dst[out_tensor]
    assert head['kind'] == L_CONV and head['act'] == ACT_SIGMOID
    assert (head['k'], head['cin'], head['cout']) == (1, 32, 1)
    # the rest of the graph: two pools, two upsamplings, the (4, 4) crop, two concatenations
    kinds = [d['kind'] for d in layers]
    assert kinds.count(L_POOL) == 2 and kinds.count(L_UP) == 2 and kinds.count(L_CONCAT) == 2
    crop = [d for d in layers if d['kind'] == L_CROP]
    assert len(crop) == 1 and crop[0]['p'] == (4, 4, 4, 4, 4, 4) and crop[0]['src0'] == 2
    # c1 (tensor 2) feeds the pool and the crop: a ReLU output with two consumers
    assert sorted(d['kind'] for d in layers if d['src0'] == 2) == [L_POOL, L_CROP]


@pytest.mark.parametrize('in_sz', [14, 18, 22, 62])
def test_trainable_patch_sizes_give_the_4_4_crop(in_sz):
    """in_sz = 2 (mod 4), >= 14: both pools are exact, the crop is (4, 4), the output
    (in_sz - 12)^3"""
    g = fplmodels.unet_like_vol(in_sz)[0]
    crop = [n for n in g.nodes if n.kind == 'crop'][0]
    assert crop.attrs['c'] == ((4, 4),) * 3
    assert g.output.size == (in_sz - 12,) * 3
    for n in g.nodes:
        if n.kind == 'pool':
            assert all(s % 2 == 0 for s in g.nodes[n.inputs[0]].size)


def test_other_factories_lower_without_relu_convs():
    """the nine other factories keep their lowering: no conv layer of theirs carries ACT_RELU
    (their ReLUs are layers of their own behind a BatchNorm), sigmoid only on the head"""
    fac = _factories()
    assert 'unet_like_vol' in fac and len(fac) == 10, sorted(fac)
    for name, g in fac.items():
        if name == 'unet_like_vol':
            continue
        layers, _, _, out_tensor, _ = lower_training(g)
        for d in layers:
            if d['kind'] != L_CONV:
                assert d['act'] == ACT_NONE, name
            elif d['dst'] == out_tensor:
                assert d['act'] == ACT_SIGMOID, name
            else:
                assert d['act'] == ACT_NONE, name


def test_branch_graphs_lower_with_relu_on_every_hidden_conv():
    """the hand-built graphs of the GPU test: every conv but the head is a ReLU conv; the tail
    case's second ReLU output has 4 k + 2 elements"""
    for name, (build, shape, _) in rc.BRANCHES.items():
        g = build()
        layers, _, _, out_tensor, _ = lower_training(g)
        convs = [d for d in layers if d['kind'] == L_CONV]
        assert [d['act'] for d in convs] == [ACT_RELU] * (len(convs) - 1) + [ACT_SIGMOID], name
        assert convs[-1]['dst'] == out_tensor
    g = rc.BRANCHES['tail_54'][0]()
    o = rc.out_shape(g, rc.BRANCHES['tail_54'][1])
    assert int(np.prod(o)) % 4 == 2


def test_forward64_agrees_with_the_training_oracle():
    """the float64 forward restated for the input search computes the oracle's network: the
    oracle's loss from forward64's pre-activations of the last ReLU conv"""
    import torch
    from oracle import train_oracle
    shape = rc.VOL_SHAPES[0]
    g = rc.vol_graph(shape[1])
    labels = rc.vol_labels(shape)
    data = next(rc.candidate_inputs(shape, rc.VOL_DATA_SEED))
    pre = rc.forward64(g, g.weights, data)
    assert sorted(pre) == list(rc.VOL_RELU_NODES)
    x = np.maximum(pre[16], 0.0)
    w = g.weights[g.nodes[17].weight_slots[0]].astype(np.float64).reshape(32)
    p = 1.0 / (1.0 + np.exp(-(x @ w)))[..., None]
    want = float(train_oracle.loss_value(torch.tensor(p), torch.tensor(labels, dtype=torch.float64),
                                         'masked_weighted_binary_crossentropy'))
    rl, _, _ = train_oracle.train_step(g, g.weights, data, labels, 5,
                                       loss='masked_weighted_binary_crossentropy')
    assert abs(rl - want) < 1e-12 * max(1.0, abs(rl))
