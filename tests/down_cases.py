"""Shared helpers of the Conv3D(filters, 2, strides=2) tests (test_down_host.py, test_gpu_down.py).

The float64 restatements of the new layer live here:

(a) `graph_forward64` / `train_step64`: the walks of tests/deconv_cases.py with one more branch,
    `torch.nn.functional.conv3d(..., stride=2)` in float64, for the new kind.  Those walks
    dispatch on the node kind inside their loops and raise on a kind they do not know, so they
    cannot be reused for a graph that holds a 'down' node without editing that file: they are
    restated here, every other branch calling the same helpers (`oracle.cnn_oracle`,
    `oracle.train_oracle`, `deconv_cases.conv_transpose64`).
(b) `down_numpy`: an independent numpy restatement - eight `einsum`s over the strided views
    `x[:, a::2, b::2, c::2]`, each cut to `s // 2`.

PARITY UNPINNED, as for the rest of the CNN oracle: Keras / TensorFlow are absent, the semantics
of `Conv3D(filters, 2, strides=2, padding='valid')` are restated from the Keras 2 documentation
(kernel `(2,2,2,Cin,Cout)`, cross-correlation, output = floor(input / 2), the last plane of an
odd axis is not read).

The example network `tiny_vnet` is `deconv_cases.tiny_unet_t` with its pool replaced by the
learned down-convolution; no factory of `fplmodels` builds one.
"""
import numpy as np
import torch
import torch.nn.functional as F

from flypylib_amd.program import LayerGraph
from oracle import cnn_oracle, train_oracle
from tests import deconv_cases as dc
from tests.deconv_cases import randomize  # noqa: F401  (re-exported)

BN_EPS, BN_MOMENTUM = dc.BN_EPS, dc.BN_MOMENTUM


def tiny_vnet(in_sz=None, seed=3):
    """conv3(1->8) BN ReLU | down(8->8, bias) BN ReLU | conv3(8->16) BN ReLU | deconv(16->8, bias)
    BN ReLU | concat with the cropped skip | conv1(16->8, relu) | conv1(->1, sigmoid).

    Geometry and rf_info are tiny_unet_t's: a stride-2 kernel-2 'valid' convolution gives s // 2
    outputs per axis, as MaxPooling3D(2) does, and sees the same 2 x 2 x 2 window."""
    in_sz = (22, 22, 22) if in_sz is None else in_sz
    g = LayerGraph(in_sz, seed=seed)
    x = g.input()
    c1 = g.conv_bn_relu(x, 8, 3)
    d = g.bn_relu(g.down(c1, 8, use_bias=True))
    c2 = g.conv_bn_relu(d, 16, 3)
    u = g.bn_relu(g.deconv(c2, 8, use_bias=True))
    m = g.concat(u, g.crop(c1, 2))
    h = g.conv(m, 8, 1, use_bias=True, activation='relu')
    g.finish(g.conv(h, 1, 1, use_bias=True, activation='sigmoid'))
    return g, (7, 3, 1), in_sz, None


def tiny_vnet_random(in_sz=None):
    """the factory with non-trivial biases and BN statistics (inference tests)"""
    g, rf, sz, ca = tiny_vnet(in_sz)
    return randomize(g), rf, sz, ca


def down_graph(cin, cout, use_bias, relu, bn, spatial, seed=0):
    """the op alone: (a 1x1x1 conv 1 -> cin in front when cin > 1: a program's input has one
    channel) -> down [-> BN] [-> ReLU]; returns (graph, index of the down node)"""
    g = LayerGraph(spatial, seed=seed)
    x = g.input()
    if cin > 1:
        x = g.conv(x, cin, 1, use_bias=True)
    d = g.down(x, cout, use_bias=use_bias, activation='relu' if relu and not bn else None)
    out = d
    if bn:
        out = g.bn(out)
        if relu:
            out = g.relu(out)
    g.finish(out)
    randomize(g, seed + 1)
    return g, d.idx


def conv_down64(x, kernel, bias=None):
    """x (N,C,D,H,W) torch float64; kernel (2,2,2,Cin,Cout) Keras layout -> torch's (Cout,Cin,2,2,2)"""
    return F.conv3d(x, kernel.permute(4, 3, 0, 1, 2).contiguous(), bias, stride=2)


def down_numpy(x, kernel, bias=None, relu=False):
    """(b): x (N,D,H,W,Cin), kernel (2,2,2,Cin,Cout) -> (N,D//2,H//2,W//2,Cout), float64"""
    x = np.asarray(x, np.float64)
    kernel = np.asarray(kernel, np.float64)
    n, d, h, w, _ = x.shape
    od, oh, ow = d // 2, h // 2, w // 2
    y = np.zeros((n, od, oh, ow, kernel.shape[4]))
    for a in range(2):
        for b in range(2):
            for c in range(2):
                y += np.einsum('ndhwi,io->ndhwo', x[:, a::2, b::2, c::2][:, :od, :oh, :ow], kernel[a, b, c])
    if bias is not None:
        y = y + np.asarray(bias, np.float64)
    return np.maximum(y, 0.0) if relu else y


def _conv_like(n, a, W):
    bias = W[n.weight_slots[1]] if n.attrs['use_bias'] else None
    f = {'conv': cnn_oracle.conv3d_valid, 'deconv': dc.conv_transpose64, 'down': conv_down64}[n.kind]
    v = f(a[0], W[n.weight_slots[0]], bias)
    if n.attrs['activation'] == 'relu':
        v = torch.relu(v)
    elif n.attrs['activation'] == 'sigmoid':
        v = torch.sigmoid(v)
    return v


def graph_forward64(graph, x):
    """(a), inference mode: x (N,D,H,W,1) -> (N,d,h,w,C) float64 numpy"""
    W = [torch.as_tensor(np.asarray(a, np.float64)) for a in graph.weights]
    vals = {}
    for n in graph.nodes:
        a = [vals[i] for i in n.inputs]
        if n.kind == 'input':
            v = torch.as_tensor(np.asarray(x, np.float64)).permute(0, 4, 1, 2, 3)
        elif n.kind in ('conv', 'deconv', 'down'):
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
        elif n.kind in ('conv', 'deconv', 'down'):
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
