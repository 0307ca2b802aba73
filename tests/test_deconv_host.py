"""Conv3DTranspose(filters, 2, strides=2) on the host: the two float64 restatements against each
other, the graph API, both lowerings, the Keras interchange file and the compiler's resource
report of the new kernels.  Nothing here needs a GPU."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from flypylib_amd import fplmodels, keras_io
from flypylib_amd.program import (ACT_NONE, ACT_RELU, L_BN, L_CONV, L_DECONV, OP_CONV, OP_DECONV,
                                  LayerGraph, lower_training)
from tests import deconv_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'lowering_digests_parent.npz')
SPATIAL = [(1, 1, 1), (3, 4, 5), (7, 2, 9)]
CHANNELS = [(1, 1), (3, 5), (16, 16), (48, 32), (33, 17)]


@pytest.mark.parametrize('spatial', SPATIAL)
@pytest.mark.parametrize('cin,cout', CHANNELS)
def test_the_two_restatements_agree(spatial, cin, cout):
    """(a) torch conv_transpose3d and (b) einsum per parity + interleave: float64 round-off.
    |x|, |W| ~ 1 and at most 48 terms: 1e-12 is three orders above the rounding of such a sum."""
    rng = np.random.default_rng(cin * 100 + cout)
    for n in (1, 3):
        x = rng.standard_normal((n,) + spatial + (cin,))
        k = rng.standard_normal((2, 2, 2, cout, cin))
        b = rng.standard_normal(cout)
        a = dc.conv_transpose64(torch.as_tensor(x).permute(0, 4, 1, 2, 3), torch.as_tensor(k),
                                torch.as_tensor(b)).permute(0, 2, 3, 4, 1).numpy()
        ref = dc.deconv_numpy(x, k, b)
        assert a.shape == ref.shape == (n,) + tuple(2 * s for s in spatial) + (cout,)
        assert np.max(np.abs(a - ref)) < 1e-12


def test_graph_api_sizes_weights_and_params():
    g = LayerGraph((6, 8, 10), seed=1)
    x = g.conv(g.input(), 5, 3)
    d = g.deconv(x, 7, use_bias=True, activation='relu')
    assert d.kind == 'deconv' and d.channels == 7 and d.size == (8, 12, 16)
    assert [g.weights[s].shape for s in d.weight_slots] == [(2, 2, 2, 7, 5), (7,)]
    assert [g.weight_names[s] for s in d.weight_slots] == ['deconv_2/kernel', 'deconv_2/bias']
    assert g.count_params() == 27 * 5 + 8 * 7 * 5 + 7 == g.count_trainable()
    kern = g.weights[d.weight_slots[0]]
    lim = np.sqrt(6.0 / (8 * 7 + 8 * 5))                  # Keras' fans for (2,2,2,Cout,Cin)
    assert np.abs(kern).max() <= lim and np.abs(kern).max() > 0.8 * lim and not g.weights[d.weight_slots[1]].any()
    nb = g.deconv(x, 3)
    assert len(nb.weight_slots) == 1
    fc = LayerGraph(None)
    assert fc.deconv(fc.input(), 2).size is None


@pytest.mark.parametrize('kw', [dict(kernel_size=3), dict(kernel_size=4), dict(strides=1), dict(strides=3),
                                dict(kernel_size=(2, 2, 3)), dict(strides=(2, 1, 2))])
def test_other_kernels_and_strides_are_refused(kw):
    g = LayerGraph((4, 4, 4))
    with pytest.raises(ValueError, match='kernel_size 2 with strides 2'):
        g.deconv(g.input(), 4, **kw)
    g.deconv(g.input(), 4, kernel_size=2, strides=(2, 2, 2))


def _run_folded(graph, x):
    """the lowered op list through (b) for the deconv and numpy for a leading 1x1x1 conv"""
    ops, arena, out_t, n_t = graph.lower_inference()
    arena = arena.astype(np.float64)
    t = {0: np.asarray(x, np.float64)}
    for o in ops:
        s, h = arena[o['scale_off']:o['scale_off'] + o['cout']], arena[o['shift_off']:o['shift_off'] + o['cout']]
        if o['kind'] == OP_CONV:
            assert o['k'] == 1
            w = arena[o['w_off']:o['w_off'] + o['cin'] * o['cout']].reshape(o['cin'], o['cout'])
            y = t[o['src0']] @ w * s + h
        else:
            assert o['kind'] == OP_DECONV and o['k'] == 2 and tuple(o['p']) == (2, 2, 2, 0, 0, 0)
            w = arena[o['w_off']:o['w_off'] + 8 * o['cin'] * o['cout']].reshape(2, 2, 2, o['cout'], o['cin'])
            y = dc.deconv_numpy(t[o['src0']], w) * s + h
        t[o['dst']] = np.maximum(y, 0) if o['act'] == ACT_RELU else y
    return ops, t[out_t]


@pytest.mark.parametrize('bias,relu,bn', [(b, r, n) for b in (0, 1) for r in (0, 1) for n in (0, 1)])
def test_lower_inference_folds_bn_and_relu(bias, relu, bn):
    g, _ = dc.deconv_graph(3, 5, bias, relu, bn, (3, 4, 5))
    x = np.random.default_rng(0).standard_normal((2, 3, 4, 5, 1))
    ops, got = _run_folded(g, x)
    assert [o['kind'] for o in ops] == [OP_CONV, OP_DECONV]          # BN and ReLU are gone
    assert ops[1]['act'] == (ACT_RELU if relu else ACT_NONE) and (ops[1]['cin'], ops[1]['cout']) == (3, 5)
    ref = dc.graph_forward64(g, x)
    # fp32 folding of scale and shift: a few 2^-24 relative on values of order 1
    assert got.shape == ref.shape and np.max(np.abs(got - ref)) < 1e-5 and ref.std() > 1e-2


def test_lower_training_emits_the_layer_with_its_offsets():
    g = dc.tiny_unet_t((14, 14, 14))[0]
    layers, arena, offsets, out_t, n_t = lower_training(g)
    assert arena.size == g.count_params() and len(layers) == len(g.nodes) - 1
    node = [n for n in g.nodes if n.kind == 'deconv'][0]
    L = layers[node.idx - 1]
    assert L['kind'] == L_DECONV == 9 and (L['k'], L['cin'], L['cout'], L['use_bias'], L['act']) == (2, 16, 8, 1, ACT_NONE)
    assert tuple(L['p']) == (2, 2, 2, 0, 0, 0)
    assert L['w_off'][:2] == [offsets[s] for s in node.weight_slots]
    w0 = L['w_off'][0]
    assert np.array_equal(arena[w0:w0 + 8 * 16 * 8], g.weights[node.weight_slots[0]].reshape(-1))
    assert layers[node.idx]['kind'] == L_BN and layers[node.idx]['src0'] == L['dst']
    assert sum(l['kind'] == L_CONV for l in layers) == 4
    assert g.output.size == (8, 8, 8) and dc.tiny_unet_t()[0].output.size == (16, 16, 16)


def test_keras_file_round_trip(tmp_path):
    g = dc.randomize(dc.tiny_unet_t((14, 14, 14))[0])
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
    layer = [l for l in cfg['config']['layers'] if l['class_name'] == 'Conv3DTranspose']
    assert len(layer) == 1 and layer[0]['name'] == 'conv3d_transpose_1'
    c = layer[0]['config']
    assert (c['filters'], c['kernel_size'], c['strides'], c['padding'], c['use_bias'], c['activation']) == \
        (8, [2, 2, 2], [2, 2, 2], 'valid', True, 'linear')
    assert c['data_format'] == 'channels_last' and c['kernel_initializer']['class_name'] == 'VarianceScaling'
    tree = keras_io.weight_tree(g)
    assert [w.decode() for w in tree['groups']['conv3d_transpose_1']['attrs']['weight_names']] == \
        ['conv3d_transpose_1/kernel:0', 'conv3d_transpose_1/bias:0']
    h = dc.tiny_unet_t((14, 14, 14), seed=9)[0]
    h.compile(loss='binary_crossentropy', optimizer='adam', metrics=['accuracy'])
    h.load(path)
    for a, b in zip(g.weights, h.weights):
        assert np.array_equal(a, b)
    tr = [s for n in g.nodes for s in (n.weight_slots[:2] if n.kind == 'bn' else n.weight_slots)]
    assert h.opt_state[2] == 17
    for s in tr:
        assert np.array_equal(h.opt_state[0][s], g.opt_state[0][s]) and np.array_equal(h.opt_state[1][s], g.opt_state[1][s])
    # the .npz pair of save_network likewise
    g.save(str(tmp_path / 'net.weights.npz'))
    h2 = dc.tiny_unet_t((14, 14, 14), seed=4)[0]
    h2.load(str(tmp_path / 'net.weights.npz'))
    assert all(np.array_equal(a, b) for a, b in zip(g.weights, h2.weights)) and h2.opt_state[2] == 17


def lowering_digests():
    """SHA-256 of each fplmodels factory's inference and training lowerings: every field of every
    op / layer, the arenas' bytes, the offsets, the tensor counts"""
    out = {}
    for name in sorted(dir(fplmodels)):
        f = getattr(fplmodels, name)
        if name.startswith('_') or not callable(f) or getattr(f, '__module__', '') != fplmodels.__name__:
            continue
        try:
            r = f()
        except TypeError:
            continue
        if not (isinstance(r, tuple) and len(r) == 4 and isinstance(r[0], LayerGraph)):
            continue
        g = r[0]

        def plain(d):
            return {k: ([int(x) for x in v] if isinstance(v, (list, tuple)) else
                        float(v) if isinstance(v, float) else int(v)) for k, v in sorted(d.items())}
        ops, arena, out_t, n_t = g.lower_inference()
        h = hashlib.sha256(json.dumps([[plain(o) for o in ops], int(out_t), int(n_t)]).encode())
        h.update(np.ascontiguousarray(arena, np.float32).tobytes())
        out[name + '/inference'] = np.frombuffer(h.digest(), np.uint8)
        layers, arena, offsets, out_t, n_t = lower_training(g)
        h = hashlib.sha256(json.dumps([[plain(l) for l in layers], [int(o) for o in offsets],
                                       int(out_t), int(n_t)]).encode())
        h.update(np.ascontiguousarray(arena, np.float32).tobytes())
        out[name + '/training'] = np.frombuffer(h.digest(), np.uint8)
    return out


def test_existing_factories_lower_to_the_parents_bytes():
    """tests/golden/lowering_digests_parent.npz: lowering_digests() of the commit before the new
    layer kind (this function run on that tree, once)"""
    got = lowering_digests()
    with np.load(GOLDEN) as z:
        want = {k: z[k] for k in z.files}
    assert len(want) == 20 and sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def test_keras_bytes_of_graphs_without_the_layer_are_unchanged(tmp_path):
    """the file written for a graph that holds no Conv3DTranspose: digest taken on the parent"""
    g = fplmodels.unet_like_vol()[0]
    g.compile(loss='binary_crossentropy', optimizer='adam', metrics=['accuracy'])
    path = str(tmp_path / 'u.h5')
    g.save(path)
    with np.load(GOLDEN.replace('lowering_digests', 'keras_bytes')) as z:
        want = z['unet_like_vol']
    assert np.array_equal(np.frombuffer(hashlib.sha256(open(path, 'rb').read()).digest(), np.uint8), want)


def test_the_new_kernels_do_not_spill():
    """what the compiler reports for the build's own flags: no spilled register, no scratch"""
    import shutil
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from flypylib_amd.csrc import build
    if not shutil.which(build.HIPCC) and not os.path.exists(build.HIPCC):
        pytest.skip('hipcc not available')
    import kernel_resources
    res = {k: v for k, v in kernel_resources.kernel_resources('conv_mfma_f32.hip').items()
           if 'deconv2_f32' in k or 'concat_view_f32' in k}
    assert len(res) == 5, sorted(res)                     # NKB 1, 2, 3 and the any-cin form; the concat
    res.update({k: v for k, v in kernel_resources.kernel_resources('train.hip').items()
                if 'deconv2_' in k or 'conv_wgrad_partial_f32' in k})
    # forward, input gradient x 2, the two weight-gradient stages; the convolutions' fixed-order stage
    assert len(res) == 11, sorted(res)
    for name, v in res.items():
        assert v['vgpr_spill_count'] == 0 and v['sgpr_spill_count'] == 0, (name, v)
        assert v['private_segment_fixed_size'] == 0 and v['vgpr_count'] <= 128, (name, v)


def test_a_user_named_transpose_layer_is_told_by_its_kernel():
    """a Keras file whose layers carry custom names: the (2,2,2,Cout,Cin) kernel goes to the deconv
    node, the file's order is kept"""
    g = dc.randomize(dc.tiny_unet_t((14, 14, 14))[0])
    roles = {'conv': ['kernel', 'bias'], 'deconv': ['kernel', 'bias'],
             'bn': ['gamma', 'beta', 'moving_mean', 'moving_variance']}
    layers = [('blk%s' % 'abcdefghijklmnop'[n.idx], [(r, g.weights[s]) for r, s in zip(roles[n.kind], n.weight_slots)])
              for n in g.nodes if n.weight_slots]
    assert not any('transpose' in name for name, _ in layers)
    got = keras_io.graph_weights_from_layers(dc.tiny_unet_t((14, 14, 14), seed=5)[0], layers)
    assert all(np.array_equal(a, b) for a, b in zip(got, g.weights))
