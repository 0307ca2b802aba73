"""Shared helpers of the Conv3DTranspose tests (test_deconv_host.py, test_gpu_deconv.py).

The float64 restatements of the new layer live here:

(a) `graph_forward64` / `train_step64`: a walk of a `LayerGraph` in torch on the CPU, float64,
    that calls `oracle.cnn_oracle`'s helpers (and `oracle.train_oracle`'s loss) for the layer
    kinds they already state and `torch.nn.functional.conv_transpose3d` for the new one.
(b) `deconv_numpy`: an independent numpy restatement - one `einsum` per output parity, then the
    eight results interleaved.

PARITY UNPINNED, as for the rest of the CNN oracle: Keras / TensorFlow are absent, the semantics
of `Conv3DTranspose(filters, 2, strides=2, padding='valid')` are restated from the Keras 2
documentation (kernel `(2,2,2,Cout,Cin)`, no flip, output = 2 x input).

The example network `tiny_unet_t` is the smallest U-Net with a learned up-convolution; no factory
of `fplmodels` builds one.
"""
import numpy as np
import torch
import torch.nn.functional as F

from flypylib_amd.program import LayerGraph
from oracle import cnn_oracle, train_oracle

BN_EPS, BN_MOMENTUM = 1e-3, 0.99


def tiny_unet_t(in_sz=None, seed=3):
    """conv3(1->8) BN ReLU | pool | conv3(8->16) BN ReLU | deconv(16->8, bias) BN ReLU |
    concat with the cropped skip | conv1(16->8, relu) | conv1(->1, sigmoid).

    rf_info, derived: the two 3x3x3 convolutions see 1 + 2 + 2 * 2 = 7 input voxels per axis
    (the second one works at half resolution), the up-convolution and the 1x1x1 convolutions add
    none: rf_size 7, rf_offset 3.  An input of (even) edge I gives (I - 2) / 2 - 2 pooled voxels,
    doubled: I - 6 outputs, one per input voxel inside the offset - rf_stride 1.  The skip
    (I - 2) is cropped by 2 per side to meet it."""
    in_sz = (22, 22, 22) if in_sz is None else in_sz
    g = LayerGraph(in_sz, seed=seed)
    x = g.input()
    c1 = g.conv_bn_relu(x, 8, 3)
    c2 = g.conv_bn_relu(g.pool(c1), 16, 3)
    u = g.bn_relu(g.deconv(c2, 8, use_bias=True))
    m = g.concat(u, g.crop(c1, 2))
    h = g.conv(m, 8, 1, use_bias=True, activation='relu')
    g.finish(g.conv(h, 1, 1, use_bias=True, activation='sigmoid'))
    return g, (7, 3, 1), in_sz, None


def randomize(graph, seed=11):
    """non-trivial biases and BN statistics (the initialisers leave zeros and ones)"""
    rng = np.random.default_rng(seed)
    graph.randomize_bn(seed)
    for i, name in enumerate(graph.weight_names):
        if name.endswith('/bias'):
            graph.weights[i] = (0.2 * rng.standard_normal(graph.weights[i].shape)).astype(np.float32)
    return graph


def tiny_unet_t_random(in_sz=None):
    """the factory with non-trivial biases and BN statistics (inference tests)"""
    g, rf, sz, ca = tiny_unet_t(in_sz)
    return randomize(g), rf, sz, ca


def deconv_graph(cin, cout, use_bias, relu, bn, spatial, seed=0):
    """the op alone: (a 1x1x1 conv 1 -> cin in front when cin > 1: a program's input has one
    channel) -> deconv [-> BN] [-> ReLU]; returns (graph, index of the deconv node)"""
    g = LayerGraph(spatial, seed=seed)
    x = g.input()
    if cin > 1:
        x = g.conv(x, cin, 1, use_bias=True)
    d = g.deconv(x, cout, use_bias=use_bias, activation='relu' if relu and not bn else None)
    out = d
    if bn:
        out = g.bn(out)
        if relu:
            out = g.relu(out)
    g.finish(out)
    randomize(g, seed + 1)
    return g, d.idx


def conv_transpose64(x, kernel, bias=None):
    """x (N,C,D,H,W) torch float64; kernel (2,2,2,Cout,Cin) Keras layout -> torch's (Cin,Cout,2,2,2)"""
    return F.conv_transpose3d(x, kernel.permute(4, 3, 0, 1, 2).contiguous(), bias, stride=2)


def deconv_numpy(x, kernel, bias=None, relu=False):
    """(b): x (N,D,H,W,Cin), kernel (2,2,2,Cout,Cin) -> (N,2D,2H,2W,Cout), float64"""
    x = np.asarray(x, np.float64)
    kernel = np.asarray(kernel, np.float64)
    n, d, h, w, _ = x.shape
    cout = kernel.shape[3]
    y = np.zeros((n, 2 * d, 2 * h, 2 * w, cout))
    for a in range(2):
        for b in range(2):
            for c in range(2):
                y[:, a::2, b::2, c::2, :] = np.einsum('ndhwi,oi->ndhwo', x, kernel[a, b, c])
    if bias is not None:
        y = y + np.asarray(bias, np.float64)
    return np.maximum(y, 0.0) if relu else y


def graph_forward64(graph, x):
    """(a), inference mode: x (N,D,H,W,1) -> (N,d,h,w,C) float64 numpy"""
    dt = torch.float64
    W = [torch.as_tensor(np.asarray(a, np.float64)) for a in graph.weights]
    vals = {}
    for n in graph.nodes:
        a = [vals[i] for i in n.inputs]
        if n.kind == 'input':
            v = torch.as_tensor(np.asarray(x, np.float64)).permute(0, 4, 1, 2, 3)
        elif n.kind in ('conv', 'deconv'):
            bias = W[n.weight_slots[1]] if n.attrs['use_bias'] else None
            v = (cnn_oracle.conv3d_valid if n.kind == 'conv' else conv_transpose64)(
                a[0], W[n.weight_slots[0]], bias)
            if n.attrs['activation'] == 'relu':
                v = torch.relu(v)
            elif n.attrs['activation'] == 'sigmoid':
                v = torch.sigmoid(v)
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
        assert v.dtype == dt
        vals[n.idx] = v
    return vals[graph.output.idx].permute(0, 2, 3, 4, 1).contiguous().numpy()


def train_step64(graph, data, labels, loss='binary_crossentropy'):
    """(a), training mode (BatchNorm on batch statistics), float64 autograd:
    -> (loss, metrics, grads in get_weights() order - the moving statistics' entries are the
    pending deltas, as the engine's gradient arena holds them -, min_pool_gap)"""
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
        elif n.kind in ('conv', 'deconv'):
            bias = W[n.weight_slots[1]] if n.attrs['use_bias'] else None
            v = (cnn_oracle.conv3d_valid if n.kind == 'conv' else conv_transpose64)(
                a[0], W[n.weight_slots[0]], bias)
            if n.attrs['activation'] == 'relu':
                v = torch.relu(v)
            elif n.attrs['activation'] == 'sigmoid':
                v = torch.sigmoid(v)
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
    return float(lv.detach()), metrics, grads, gap
