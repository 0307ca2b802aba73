"""Graphs, inputs and the float64 forward pass shared by the tests of ReLU-activated
convolutions in the training step (test_train_relu_conv_host.py, test_gpu_train_relu_conv.py).

A ReLU routes a gradient element by the sign of a pre-activation, so a pre-activation at
rounding distance from zero can be masked differently by two correct fp32 implementations -
like the max-pool windows `FLIP_GAP` guards in test_gpu_train.py.  `pick_input` therefore
searches the seeds data_seed + 1000 k, k < 8, for an input on which (a) every max-pool window
is separated by more than FLIP_GAP and (b) no ReLU pre-activation of a layer lies closer to
zero than that layer's gap G.  Finding none FAILS: there is no loose fallback.

G is 4 x the largest |GPU - float64| pre-activation difference of the layer, measured once on
an MI355X through FPL_TRAIN_CONVRELU_SEPARATE=1 + FPL_TRAIN_DUMP (the separate path keeps the
pre-activations; the fused default computes bit-identical ones in the same kernels) over all
eight candidate seeds of every case; the factor 4 is the margin FLIP_GAP has over the ~2e-6
spread of the convolutions.  The measured maxima stand next to each constant below."""
import numpy as np
import torch
import torch.nn.functional as F

from flypylib_amd import fplmodels, synth
from flypylib_amd.program import LayerGraph
from oracle import train_oracle

FLIP_GAP = 5e-6      # test_gpu_train.FLIP_GAP


def relu_convs(graph):
    return [n for n in graph.nodes if n.kind == 'conv' and n.attrs['activation'] == 'relu']


def forward64(graph, weights, data):
    """float64 forward of the BatchNorm-free layer kinds -> {node idx: pre-activation of that
    ReLU conv, channels last}"""
    W = [torch.tensor(np.asarray(w), dtype=torch.float64) for w in weights]
    x = torch.tensor(np.asarray(data, np.float32), dtype=torch.float64)
    if x.ndim == 4:
        x = x[..., None]
    vals, pre = {}, {}
    for n in graph.nodes:
        if n.kind == 'input':
            vals[n.idx] = x.permute(0, 4, 1, 2, 3)
            continue
        a = [vals[i] for i in n.inputs]
        if n.kind == 'conv':
            bias = W[n.weight_slots[1]] if n.attrs['use_bias'] else None
            v = F.conv3d(a[0], W[n.weight_slots[0]].permute(4, 3, 0, 1, 2), bias)
            if n.attrs['activation'] == 'relu':
                pre[n.idx] = v.permute(0, 2, 3, 4, 1).contiguous().numpy()
                v = torch.relu(v)
            elif n.attrs['activation'] == 'sigmoid':
                v = torch.sigmoid(v)
        elif n.kind == 'pool':
            v = F.max_pool3d(a[0], 2, 2)
        elif n.kind == 'up':
            v = a[0]
            for ax, f in zip((2, 3, 4), n.attrs['n']):
                v = torch.repeat_interleave(v, int(f), dim=ax)
        elif n.kind == 'crop':
            c = n.attrs['c']
            v = a[0][:, :, c[0][0]:a[0].shape[2] - c[0][1], c[1][0]:a[0].shape[3] - c[1][1],
                     c[2][0]:a[0].shape[4] - c[2][1]]
        elif n.kind == 'concat':
            v = torch.cat(a, dim=1)
        else:
            raise NotImplementedError(n.kind)
        vals[n.idx] = v
    return pre


def candidate_inputs(shape, data_seed, tries=8):
    for k in range(tries):
        rng = np.random.default_rng(data_seed + 1000 * k)
        yield rng.standard_normal(shape).astype(np.float32)


def pick_input(graph, shape, data_seed, labels, gaps, loss='binary_crossentropy', step_seed=5,
               tries=8, flip_gap=FLIP_GAP):
    """-> (data, oracle loss, oracle metrics, oracle grads) on the first candidate input that
    keeps every ReLU pre-activation of node i at least gaps[i] from zero and every max-pool
    window separated by more than flip_gap.  Also requires every ReLU layer to have both
    positive and zero outputs there, so the mask is exercised."""
    nodes = relu_convs(graph)
    assert sorted(gaps) == [n.idx for n in nodes], (sorted(gaps), [n.idx for n in nodes])
    seen = []
    for data in candidate_inputs(shape, data_seed, tries):
        pre = forward64(graph, graph.weights, data)
        margin = min(float(np.min(np.abs(pre[i]))) / gaps[i] for i in gaps)
        if margin < 1.0:
            seen.append('relu margin %.2f' % margin)
            continue
        info = {}
        rl, rm, rg = train_oracle.train_step(graph, graph.weights, data, labels, step_seed,
                                             loss=loss, return_metrics=True, info=info)
        if info.get('min_pool_gap', 1.0) <= flip_gap:
            seen.append('pool gap %.2g' % info['min_pool_gap'])
            continue
        for i in gaps:
            alive = float(np.mean(pre[i] > 0))
            assert 0.0 < alive < 1.0, 'relu conv %d: %.0f %% of its outputs alive' % (i, 100 * alive)
        return data, rl, rm, rg
    raise AssertionError('no input among %d seeds keeps every ReLU pre-activation and max-pool '
                         'window clear of fp32 rounding (%s): pick another data_seed'
                         % (tries, ', '.join(seen)))


# ---- unet_like_vol --------------------------------------------------------------------------
VOL_RELU_NODES = (1, 2, 4, 5, 7, 10, 11, 15, 16)
VOL_SHAPES = ((2, 14, 14, 14, 1), (1, 18, 18, 18, 1))
VOL_DATA_SEED = 3


def vol_graph(in_sz, seed=3):
    g = fplmodels.unet_like_vol(in_sz)[0]
    return synth.synthetic_weights(g, seed)


def vol_labels(shape, seed=8):
    """labels in {0, 1, 2}: the mask class is present"""
    n, o = shape[0], shape[1] - 12
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, 3, (n, o, o, o, 1)).astype(np.uint8)
    lab.reshape(-1)[:3] = (0, 1, 2)
    return lab


# ---- one small graph per convolution kernel branch that gains an activation ------------------
def _head(g, x, use_bias=False):
    return g.finish(g.conv(x, 1, 1, use_bias=use_bias, activation='sigmoid'))


def _chain(specs, use_bias=False, seed=1):
    """conv(relu) -> conv(relu) -> ... -> sigmoid head; specs = ((cout, k), ...)"""
    g = LayerGraph(None, seed=seed)
    x = g.input()
    for f, k in specs:
        x = g.conv(x, f, k, use_bias=use_bias, activation='relu')
    return _head(g, x, use_bias)


def _wide(parts, cout, seed=1):
    """3x3x3 stems of `parts` channels each, concatenated (the only way to a wide tensor from
    a one-channel input), -> 3x3x3 sum(parts) -> cout (relu) -> head"""
    g = LayerGraph(None, seed=seed)
    xs = [g.conv(g.input(), f, 3, activation='relu') for f in parts]
    x = xs[0]
    for y in xs[1:]:
        x = g.concat(x, y)
    return _head(g, g.conv(x, cout, 3, activation='relu'))


def _finish(g, seed, bias_seed=None):
    synth.synthetic_weights(g, seed)
    if bias_seed is not None:           # synthetic_weights zeroes the biases
        rng = np.random.default_rng(bias_seed)
        w = g.get_weights()
        for i, name in enumerate(g.weight_names):
            if name.endswith('/bias'):
                w[i] = (0.2 * rng.standard_normal(w[i].shape)).astype(np.float32)
        g.set_weights(w)
    return g


# name -> (graph builder, input shape, environment of the step)
BRANCHES = {
    'stem_1to16': (lambda: _finish(_chain(((16, 3), (16, 1))), 21), (2, 8, 8, 8, 1), {}),
    'f32_16to32': (lambda: _finish(_chain(((16, 3), (32, 3))), 22), (2, 9, 9, 9, 1), {}),
    'split_96to64': (lambda: _finish(_wide((32, 32, 32), 64), 23), (2, 10, 10, 10, 1), {}),
    'split_80to32': (lambda: _finish(_wide((64, 16), 32), 24), (2, 10, 10, 10, 1), {}),
    'f32_96to64': (lambda: _finish(_wide((32, 32, 32), 64), 23), (2, 10, 10, 10, 1),
                   {'FPL_TRAIN_F32CONV': '1'}),
    'f32_80to32': (lambda: _finish(_wide((64, 16), 32), 24), (2, 10, 10, 10, 1),
                   {'FPL_TRAIN_F32CONV': '1'}),
    'k1_32to64': (lambda: _finish(_chain(((32, 3), (64, 1))), 25), (2, 8, 8, 8, 1), {}),
    'k1_64to64': (lambda: _finish(_chain(((64, 3), (64, 1))), 26), (2, 8, 8, 8, 1), {}),
    'direct_16to32': (lambda: _finish(_chain(((16, 3), (32, 3))), 22), (2, 9, 9, 9, 1),
                      {'FPL_TRAIN_DIRECT': '3'}),
    'bias_1to16': (lambda: _finish(_chain(((16, 3), (16, 1)), use_bias=True), 27, bias_seed=5),
                   (2, 8, 8, 8, 1), {}),
    # the second ReLU conv's output has 2 * 3^3 * 1 = 54 = 4 * 13 + 2 elements: the scalar
    # tail of the mask kernel runs (and its float4 body, on the first conv's 864)
    'tail_54': (lambda: _finish(_chain(((16, 3), (1, 1))), 28), (2, 5, 5, 5, 1), {}),
}


def branch_labels(graph_out_shape, seed=9):
    rng = np.random.default_rng(seed)
    return (rng.random(graph_out_shape) > 0.5).astype(np.uint8)


def out_shape(graph, shape):
    """output shape of a fully convolutional chain for an input shape"""
    shrink = 0
    n = graph.output
    while n.kind != 'input':
        if n.kind == 'conv':
            shrink += n.attrs['k'] - 1
        n = graph.nodes[n.inputs[0]]
    return (shape[0],) + tuple(s - shrink for s in shape[1:4]) + (1,)


def case_graphs():
    """every case of the GPU test: name -> (graph builder, shape, environment)"""
    cases = {'vol_%d' % s[1]: ((lambda s=s: vol_graph(s[1])), s, {}) for s in VOL_SHAPES}
    cases.update(BRANCHES)
    return cases


# name -> {ReLU conv node: largest |GPU - float64| pre-activation difference}, measured on an
# MI355X over the eight candidate inputs of each case (FPL_TRAIN_CONVRELU_SEPARATE=1 +
# FPL_TRAIN_DUMP, the case's own environment set).  The pre-activations are O(1); the split-half
# convolutions (node 10 / 15 of unet_like_vol, node 6 / 4 of the wide graphs) sit within the
# fp32 kernels' error here.
MEASURED = {
    'vol_14': {1: 2.95e-07, 2: 2.16e-07, 4: 7.78e-07, 5: 2.36e-07, 7: 1.72e-07, 10: 3.49e-07,
               11: 2.27e-07, 15: 3.28e-07, 16: 1.79e-07},
    'vol_18': {1: 3.75e-07, 2: 2.18e-07, 4: 7.20e-07, 5: 2.70e-07, 7: 1.79e-07, 10: 3.85e-07,
               11: 2.22e-07, 15: 4.18e-07, 16: 2.55e-07},
    'stem_1to16': {1: 3.82e-07, 2: 1.93e-07},
    'f32_16to32': {1: 3.44e-07, 2: 4.61e-07},
    'split_96to64': {1: 2.26e-07, 2: 2.30e-07, 3: 2.38e-07, 6: 1.23e-06},
    'split_80to32': {1: 1.70e-07, 2: 2.98e-07, 4: 7.01e-07},
    'f32_96to64': {1: 2.26e-07, 2: 2.30e-07, 3: 2.38e-07, 6: 1.57e-06},
    'f32_80to32': {1: 1.70e-07, 2: 2.98e-07, 4: 1.03e-06},
    'k1_32to64': {1: 2.45e-07, 2: 1.72e-07},
    'k1_64to64': {1: 1.61e-07, 2: 1.46e-07},
    'direct_16to32': {1: 2.89e-07, 2: 4.70e-07},
    'bias_1to16': {1: 4.09e-07, 2: 2.31e-07},
    'tail_54': {1: 2.66e-07, 2: 1.27e-07},
}
# G = 4 x the measured difference
GAPS = {name: {i: 4.0 * v for i, v in m.items()} for name, m in MEASURED.items()}
