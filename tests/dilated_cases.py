"""Shared helpers of the Conv3D(filters, 3, dilation_rate=2) tests (test_dilated_host.py,
test_gpu_dilated.py).

The float64 restatements of the new layer live here:

(a) `graph_forward64` / `train_step64`: the walks of tests/down_cases.py with one more branch,
    `torch.nn.functional.conv3d(..., dilation=2)` in float64, for the new kind.  Those walks
    dispatch on the node kind inside their loops and raise on a kind they do not know, so they
    cannot be reused for a graph that holds a 'dilated' node without editing that file: they are
    restated here, every other branch calling the same helpers (`oracle.cnn_oracle`,
    `oracle.train_oracle`, `deconv_cases.conv_transpose64`, `down_cases.conv_down64`).
(b) `dilated_numpy`: an independent numpy restatement - 27 `einsum`s over the shifted views
    `x[:, 2a:2a+O, 2b:2b+O, 2c:2c+O]`.
(c) `sublattice_numpy`: the plain valid 3x3x3 convolution of `oracle.cnn_oracle` on each of the
    eight parity classes `x[a::2, b::2, c::2]`, the results interleaved - the identity the fp32
    MFMA kernel rests on.

PARITY UNPINNED, as for the rest of the CNN oracle: Keras / TensorFlow are absent, the semantics
of `Conv3D(filters, 3, dilation_rate=2, padding='valid')` are restated from the Keras 2
documentation (kernel `(3,3,3,Cin,Cout)`, cross-correlation, stride 1, taps two voxels apart,
output = input - 4).

The example network `tiny_atrous` widens its field with two dilated layers at full resolution;
no factory of `fplmodels` builds one.
"""
import numpy as np
import torch
import torch.nn.functional as F

from flypylib_amd.program import LayerGraph
from oracle import cnn_oracle, train_oracle
from tests import deconv_cases as dc
from tests import down_cases as dn
from tests.deconv_cases import randomize  # noqa: F401  (re-exported)

BN_EPS, BN_MOMENTUM = dc.BN_EPS, dc.BN_MOMENTUM


def tiny_atrous(in_sz=(22,) * 3, seed=3):
    """conv3(1->8) BN ReLU | dilated(8->12, bias) BN ReLU | dilated(12->8, relu) | conv1(8->8, relu)
    | conv1(->1, sigmoid).

    22 -> 20 -> 16 -> 12; the field is 3 + 4 + 4 = 11 voxels, offset 5, stride 1."""
    g = LayerGraph(in_sz, seed=seed)
    c1 = g.conv_bn_relu(g.input(), 8, 3)
    d1 = g.bn_relu(g.dilated(c1, 12, use_bias=True))
    d2 = g.dilated(d1, 8, activation='relu')
    h = g.conv(d2, 8, 1, use_bias=True, activation='relu')
    g.finish(g.conv(h, 1, 1, use_bias=True, activation='sigmoid'))
    return g, (11, 5, 1), in_sz, None


def tiny_atrous_random(in_sz=(22,) * 3):
    """the factory with non-trivial biases and BN statistics (inference tests)"""
    g, rf, sz, ca = tiny_atrous(in_sz)
    return randomize(g), rf, sz, ca


def dilated_graph(cin, cout, use_bias, relu, bn, spatial, seed=0):
    """the op alone: (a 1x1x1 conv 1 -> cin in front when cin > 1: a program's input has one
    channel) -> dilated [-> BN] [-> ReLU]; returns (graph, index of the dilated node)"""
    g = LayerGraph(spatial, seed=seed)
    x = g.input()
    if cin > 1:
        x = g.conv(x, cin, 1, use_bias=True)
    d = g.dilated(x, cout, use_bias=use_bias, activation='relu' if relu and not bn else None)
    out = d
    if bn:
        out = g.bn(out)
        if relu:
            out = g.relu(out)
    g.finish(out)
    randomize(g, seed + 1)
    return g, d.idx


def conv_dilated64(x, kernel, bias=None):
    """x (N,C,D,H,W) torch float64; kernel (3,3,3,Cin,Cout) Keras layout -> torch's (Cout,Cin,3,3,3)"""
    return F.conv3d(x, kernel.permute(4, 3, 0, 1, 2).contiguous(), bias, dilation=2)


def dilated_numpy(x, kernel, bias=None, relu=False):
    """(b): x (N,D,H,W,Cin), kernel (3,3,3,Cin,Cout) -> (N,D-4,H-4,W-4,Cout), float64"""
    x = np.asarray(x, np.float64)
    kernel = np.asarray(kernel, np.float64)
    n, d, h, w, _ = x.shape
    od, oh, ow = d - 4, h - 4, w - 4
    y = np.zeros((n, od, oh, ow, kernel.shape[4]))
    for a in range(3):
        for b in range(3):
            for c in range(3):
                y += np.einsum('ndhwi,io->ndhwo', x[:, 2 * a:2 * a + od, 2 * b:2 * b + oh, 2 * c:2 * c + ow],
                               kernel[a, b, c])
    if bias is not None:
        y = y + np.asarray(bias, np.float64)
    return np.maximum(y, 0.0) if relu else y


def sublattice_numpy(x, kernel, bias=None):
    """(c): the plain valid 3x3x3 convolution (oracle.cnn_oracle.conv3d_valid) of each parity class
    x[:, a::2, b::2, c::2], written to y[:, a::2, b::2, c::2]; a class too short for a 3x3x3 (fewer
    than 3 voxels on an axis) has no output voxel"""
    x = np.asarray(x, np.float64)
    n, d, h, w, _ = x.shape
    k = torch.as_tensor(np.asarray(kernel, np.float64))
    y = np.zeros((n, d - 4, h - 4, w - 4, k.shape[4]))
    b = None if bias is None else torch.as_tensor(np.asarray(bias, np.float64))
    for a in range(2):
        for bb in range(2):
            for c in range(2):
                sub = x[:, a::2, bb::2, c::2]
                if min(sub.shape[1:4]) < 3:
                    assert y[:, a::2, bb::2, c::2].size == 0
                    continue
                v = cnn_oracle.conv3d_valid(torch.as_tensor(np.ascontiguousarray(sub)).permute(0, 4, 1, 2, 3), k, b)
                y[:, a::2, bb::2, c::2] = v.permute(0, 2, 3, 4, 1).numpy()
    return y


def _conv_like(n, a, W):
    bias = W[n.weight_slots[1]] if n.attrs['use_bias'] else None
    f = {'conv': cnn_oracle.conv3d_valid, 'deconv': dc.conv_transpose64, 'down': dn.conv_down64,
         'dilated': conv_dilated64}[n.kind]
    v = f(a[0], W[n.weight_slots[0]], bias)
    if n.attrs['activation'] == 'relu':
        v = torch.relu(v)
    elif n.attrs['activation'] == 'sigmoid':
        v = torch.sigmoid(v)
    return v


_CONV_KINDS = ('conv', 'deconv', 'down', 'dilated')


def graph_forward64(graph, x):
    """(a), inference mode: x (N,D,H,W,1) -> (N,d,h,w,C) float64 numpy"""
    W = [torch.as_tensor(np.asarray(a, np.float64)) for a in graph.weights]
    vals = {}
    for n in graph.nodes:
        a = [vals[i] for i in n.inputs]
        if n.kind == 'input':
            v = torch.as_tensor(np.asarray(x, np.float64)).permute(0, 4, 1, 2, 3)
        elif n.kind in _CONV_KINDS:
            v = _conv_like(n, a, W)
        elif n.kind == 'bn':
            v = cnn_oracle.bn_infer(a[0], *[W[s] for s in n.weight_slots])
        elif n.kind == 'relu':
            v = torch.relu(a[0])
        elif n.kind == 'pool':
            v = cnn_oracle.maxpool2(a[0])
        elif n.kind == 'up':
            v = cnn_oracle.upsample(a[0], n.attrs['n'])
        elif n.kind == 'crop':
            c = n.attrs['c']
            assert len({p for pair in c for p in pair}) == 1
            v = cnn_oracle.crop(a[0], c[0][0])
        elif n.kind == 'concat':
            v = torch.cat(a, dim=1)
        elif n.kind == 'add':
            v = a[0] + a[1]
        elif n.kind == 'drop':
            v = a[0]
        else:
            raise NotImplementedError(n.kind)
        assert v.dtype == torch.float64
        vals[n.idx] = v
    return vals[graph.output.idx].permute(0, 2, 3, 4, 1).contiguous().numpy()


def train_step64(graph, data, labels, loss='binary_crossentropy', want_input_grad_of=None):
    """(a), training mode (BatchNorm on batch statistics), float64 autograd:
    -> (loss, metrics, grads in get_weights() order - the moving statistics' entries are the
    pending deltas, as the engine's gradient arena holds them -, min_pool_gap); with
    `want_input_grad_of` (a node index) a fifth value: the gradient of that node's INPUT,
    (N,D,H,W,C)"""
    dt = torch.float64
    W = [torch.tensor(np.asarray(w, np.float64)) for w in graph.weights]
    for n in graph.nodes:
        for s in (n.weight_slots[:2] if n.kind == 'bn' else n.weight_slots):
            W[s].requires_grad_(True)
    deltas, vals, gap = {}, {}, 1.0
    x = torch.tensor(np.asarray(data, np.float64))
    if x.ndim == 4:
        x = x[..., None]
    for n in graph.nodes:
        a = [vals[i] for i in n.inputs]
        if n.kind == 'input':
            v = x.permute(0, 4, 1, 2, 3)
        elif n.kind in _CONV_KINDS:
            if n.idx == want_input_grad_of:
                a[0].retain_grad()
            v = _conv_like(n, a, W)
        elif n.kind == 'bn':
            g, b, mm, mv = (W[s] for s in n.weight_slots)
            mean = a[0].mean(dim=(0, 2, 3, 4))
            var = a[0].var(dim=(0, 2, 3, 4), unbiased=False)
            shp = (1, -1, 1, 1, 1)
            v = (a[0] - mean.view(shp)) / torch.sqrt(var.view(shp) + BN_EPS) * g.view(shp) + b.view(shp)
            deltas[n.weight_slots[2]] = ((mean - mm) * (1 - BN_MOMENTUM)).detach()
            deltas[n.weight_slots[3]] = ((var - mv) * (1 - BN_MOMENTUM)).detach()
        elif n.kind == 'relu':
            v = torch.relu(a[0])
        elif n.kind == 'pool':
            v = cnn_oracle.maxpool2(a[0])
            win = a[0].detach().unfold(2, 2, 2).unfold(3, 2, 2).unfold(4, 2, 2)
            top = win.reshape(*win.shape[:5], 8).topk(2, dim=-1).values
            pos = top[..., 0] > 0
            if pos.any():
                gap = min(gap, float(((top[..., 0] - top[..., 1]) / top[..., 0])[pos].min()))
        elif n.kind == 'crop':
            v = cnn_oracle.crop(a[0], n.attrs['c'][0][0])
        elif n.kind == 'concat':
            v = torch.cat(a, dim=1)
        else:
            raise NotImplementedError(n.kind)
        vals[n.idx] = v
    p = vals[graph.output.idx].permute(0, 2, 3, 4, 1)
    y = torch.tensor(np.asarray(labels), dtype=dt).reshape(p.shape)
    lv = train_oracle.loss_value(p, y, loss)
    metrics = train_oracle.metric_values(p.detach(), y)
    lv.backward()
    grads = []
    for i, w in enumerate(W):
        grads.append(deltas[i].numpy() if i in deltas else
                     w.grad.numpy() if w.grad is not None else np.zeros(tuple(w.shape)))
    if want_input_grad_of is None:
        return float(lv.detach()), metrics, grads, gap
    src = vals[graph.nodes[want_input_grad_of].inputs[0]]
    return float(lv.detach()), metrics, grads, gap, src.grad.permute(0, 2, 3, 4, 1).contiguous().numpy()
