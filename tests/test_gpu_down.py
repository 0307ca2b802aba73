"""GPU: Conv3D(filters, 2, strides=2) through the C ABI - the op alone on both fp32 executors,
whole-volume inference, the training step, validation - against the float64 restatement (a) of
tests/down_cases.py.  Gates: the fp32 executors' of tests/test_gpu_cnn.py (TOL), the training
step's of tests/test_gpu_train.py, the evaluator's of tests/test_gpu_validate_train.py.
Parity against Keras itself is UNPINNED (down_cases.py)."""
import numpy as np
import pytest

from flypylib_amd import FplNetwork, _capi, fplnetwork, valid
from tests import down_cases as dn
from tests.test_gpu_cnn import TOL
from tests.test_gpu_train import FLIP_GAP, _check_grads
from tests.test_gpu_validate_train import _means_close

pytestmark = pytest.mark.gpu

SPATIAL = [(2, 2, 2), (3, 4, 5), (7, 2, 9)]
# the issue's pairs: below, at and across the MFMA tile edges, and not multiples of anything;
# (1,1), (3,5): one K-block per tap pair in registers; (16,16): two, and 16-B loads;
# (48,32), (33,17), (96,8): the any-cin form, with and without 16-B loads
CHANNELS = [(1, 1), (3, 5), (16, 16), (48, 32), (33, 17), (96, 8)]


def _forward(ctx, graph, x, monkeypatch, perop):
    if perop:
        monkeypatch.setenv('FPL_FORCE_PEROP', '1')
    else:
        monkeypatch.delenv('FPL_FORCE_PEROP', raising=False)
    prog = _capi.Program(ctx, graph)
    try:
        out = prog.forward(x)
        assert ctx.last_path() == ('perop_f32' if perop else 'mfma_f32')
    finally:
        prog.close()
    return out


@pytest.mark.parametrize('spatial', SPATIAL, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('cin,cout', CHANNELS)
def test_the_op_alone_on_both_executors(ctx, monkeypatch, spatial, cin, cout):
    rng = np.random.default_rng(cin + 7 * cout)
    worst = 0.0
    for batch in (1, 3):
        x = rng.standard_normal((batch,) + spatial + (1,)).astype(np.float32)
        for bias in (0, 1):
            for relu in (0, 1):
                for bn in (0, 1):
                    g, _ = dn.down_graph(cin, cout, bias, relu, bn, spatial, seed=bias + 2 * relu + 4 * bn)
                    ref = dn.graph_forward64(g, x)
                    assert ref.shape == (batch,) + tuple(s // 2 for s in spatial) + (cout,)
                    # (a live reference; (2,2,2) gives one voxel, which a ReLU may well clamp)
                    assert np.abs(ref).max() > 1e-3 or (relu and ref.size == batch * cout)
                    for perop in (False, True):
                        got = _forward(ctx, g, x, monkeypatch, perop)
                        assert got.shape == ref.shape
                        err = float(np.max(np.abs(got - ref)))
                        worst = max(worst, err)
                        assert err < TOL, (batch, bias, relu, bn, perop, err)
    print('max |gpu - float64|', worst)


def _one_hot_graph(cin, cout, ci, spatial):
    g, node = dn.down_graph(cin, cout, 0, 0, 0, spatial)
    if cin > 1:                                           # the leading 1x1x1 conv routes the input to channel ci
        first = g.nodes[1]
        k = np.zeros((1, 1, 1, 1, cin), np.float32)
        k[..., ci] = 1.0
        g.weights[first.weight_slots[0]] = k
        g.weights[first.weight_slots[1]] = np.zeros(cin, np.float32)
    return g, g.weights[g.nodes[node].weight_slots[0]]     # (2,2,2,cin,cout), all distinct random values


@pytest.mark.parametrize('perop', [False, True])
@pytest.mark.parametrize('cin,cout', [(1, 3), (5, 6), (20, 6)])
def test_tap_position(ctx, monkeypatch, perop, cin, cout):
    """a one-hot input voxel at (2i+a, 2j+b, 2k+c) in a one-hot channel lights exactly output voxel
    (i, j, k), and it holds W[a, b, c, ci, :]: a swapped (a, b, c) or (ci, co) order cannot pass;
    a one-hot voxel in the dropped last plane of an odd axis lights nothing"""
    spatial, at, ci = (5, 4, 7), (1, 0, 2), cin - 1
    g, W = _one_hot_graph(cin, cout, ci, spatial)
    if perop:
        monkeypatch.setenv('FPL_FORCE_PEROP', '1')
    else:
        monkeypatch.delenv('FPL_FORCE_PEROP', raising=False)
    prog = _capi.Program(ctx, g)
    try:
        for a in range(2):
            for b in range(2):
                for c in range(2):
                    x = np.zeros((1,) + spatial + (1,), np.float32)
                    x[0, 2 * at[0] + a, 2 * at[1] + b, 2 * at[2] + c, 0] = 1.0
                    got = prog.forward(x)
                    assert ctx.last_path() == ('perop_f32' if perop else 'mfma_f32')
                    want = np.zeros((1, 2, 2, 3, cout), np.float32)
                    want[(0,) + at] = W[a, b, c, ci, :]
                    assert got.shape == want.shape and np.count_nonzero(want) == cout
                    assert np.array_equal(got != 0, want != 0), (a, b, c)
                    # one product with 1.0: exact up to an ulp
                    assert np.max(np.abs(got - want)) <= 2.0 ** -23 * np.abs(want).max(), (a, b, c)
        for pos in ((4, 1, 1), (1, 1, 6), (4, 3, 6)):     # the dropped planes z = 4 and x = 6
            x = np.zeros((1,) + spatial + (1,), np.float32)
            x[(0,) + pos + (0,)] = 1.0
            assert not prog.forward(x).any(), pos
    finally:
        prog.close()


# ---- whole-volume inference ------------------------------------------------------------------
_NET = {}


def _net():
    """tiny_vnet with non-trivial statistics, inference tile 22 (16 outputs); made once"""
    if 'net' not in _NET:
        net = FplNetwork(dn.tiny_vnet_random)
        net._set_infer()
        vol = np.random.default_rng(2).standard_normal((40, 44, 50)).astype(np.float32)
        _NET['net'], _NET['vol'] = net, vol
    return _NET['net'], _NET['vol']


def _lattice_reference(net, vol):
    """(a) over the reference's tile lattice: origins off, off + out, ...; edge tiles zero padded"""
    tile, off = net.infer_sz[0], net.rf_offset[0]
    out = tile - 2 * off
    ref = np.zeros(vol.shape, np.float64)
    tiles, where = [], []
    for z in range(off, vol.shape[0] - off, out):
        for y in range(off, vol.shape[1] - off, out):
            for x in range(off, vol.shape[2] - off, out):
                t = np.zeros((tile,) * 3, np.float32)
                src = vol[z - off:z - off + tile, y - off:y - off + tile, x - off:x - off + tile]
                t[:src.shape[0], :src.shape[1], :src.shape[2]] = src
                tiles.append(t)
                where.append((z, y, x, src.shape))
    pred = dn.graph_forward64(net.infer_network.graph, np.stack(tiles)[..., None])[..., 0]
    for p, (z, y, x, shp) in zip(pred, where):
        v = tuple(s - 2 * off for s in shp)
        ref[z:z + v[0], y:y + v[1], x:x + v[2]] = p[:v[0], :v[1], :v[2]]
    return ref


def test_whole_volume_infer(ctx, monkeypatch):
    net, vol = _net()
    assert net.rf_offset == (3, 3, 3) and net.infer_sz == (22, 22, 22)
    assert all((s - 6) % 16 for s in vol.shape)            # a partial tile on every axis
    ref = _lattice_reference(net, vol)
    pred = net.infer(vol)                                  # precision 'auto'
    assert ctx.last_path() == 'mfma_f32'
    err = float(np.max(np.abs(pred - ref)))
    print('max |gpu - float64| over the volume', err)
    assert pred.shape == vol.shape and err < TOL and ref[3:-3, 3:-3, 3:-3].std() > 1e-3
    assert not pred[:3].any() and not pred[-3:].any() and not pred[:, :3].any() and not pred[:, -3:].any()
    assert not pred[:, :, :3].any() and not pred[:, :, -3:].any()
    # the forced per-op executor: held to the same gate
    monkeypatch.setenv('FPL_FORCE_PEROP', '1')
    slow = net.infer(vol, precision='f32')
    assert ctx.last_path() == 'perop_f32' and np.max(np.abs(slow - ref)) < TOL
    monkeypatch.delenv('FPL_FORCE_PEROP')
    monkeypatch.setenv('FPL_NO_TILE_MERGE', '1')
    assert np.array_equal(net.infer(vol), pred)
    assert ctx.last_path() == 'mfma_f32'
    monkeypatch.delenv('FPL_NO_TILE_MERGE')
    for prec in ('f16s', 'f16', 'bf16'):
        with pytest.raises(Exception, match=r'Conv3D\(filters, 2, strides=2\)'):
            net.infer(vol, precision=prec)


def test_super_tiles_of_a_network_without_an_upsampling_are_bit_identical(ctx, monkeypatch):
    """conv3 | down | conv3 | head, output stride 2: no Conv3DTranspose, so the tiles merge
    (infer.hip treats the layer as a pool there) - bit-equal with FPL_NO_TILE_MERGE=1"""
    from flypylib_amd.program import LayerGraph

    def factory(in_sz=None):
        in_sz = (22, 22, 22) if in_sz is None else in_sz
        g = LayerGraph(in_sz, seed=6)
        c1 = g.conv_bn_relu(g.input(), 8, 3)
        d = g.bn_relu(g.down(c1, 12, use_bias=True))
        c2 = g.conv_bn_relu(d, 8, 3)
        g.finish(g.conv(c2, 1, 1, use_bias=True, activation='sigmoid'))
        # 22 -> 20 -> 10 -> 8, upsampled by the stride: 16 outputs; rf 3 + 1 + 2 * 2 = 8
        return dn.randomize(g), (8, 3, 2), in_sz, None
    net = FplNetwork(factory)
    net._set_infer()
    vol = np.random.default_rng(4).standard_normal((38, 54, 70)).astype(np.float32)
    pred = net.infer(vol)
    assert ctx.last_path() == 'mfma_f32' and pred[3:-3, 3:-3, 3:-3].std() > 1e-3
    monkeypatch.setenv('FPL_NO_TILE_MERGE', '1')
    assert np.array_equal(net.infer(vol), pred)


# ---- training --------------------------------------------------------------------------------
def _train_batch(seed, patch=22):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((2,) + (patch,) * 3 + (1,)).astype(np.float32)
    y = (rng.random((2,) + (patch - 6,) * 3 + (1,)) < 0.3).astype(np.uint8)
    return x, y


@pytest.mark.parametrize('patch', [22, 24])
def test_training_step_against_float64_autograd(ctx, patch):
    """patch 22: 20 -> 10 -> 8 -> 16; patch 24: 22 -> 11 -> 9 -> 18, odd sizes behind the layer"""
    g = dn.randomize(dn.tiny_vnet((patch,) * 3)[0])
    x, y = _train_batch(patch, patch)
    rl, rm, rg, gap = dn.train_step64(g, x, y)
    assert gap > FLIP_GAP                                  # (no max-pool in this network: nothing can flip)
    tr = _capi.Trainer(ctx, g)
    loss, acc = tr.step(x, y, seed=5)
    grads = tr.get_grads()
    tr.close()
    print('loss', loss, rl, 'acc', acc, rm['acc'])
    assert abs(loss - rl) < 1e-5 * max(1.0, abs(rl)) and abs(acc - rm['acc']) < 1e-6
    _check_grads(g, grads, rg)
    node = [n for n in g.nodes if n.kind == 'down'][0]
    k, b = node.weight_slots
    assert g.weight_names[k] == 'down_%d/kernel' % node.idx
    print('down kernel max |reference|', np.max(np.abs(rg[k])), 'bias', np.max(np.abs(rg[b])))
    assert np.max(np.abs(rg[k])) > 1e-6                    # held by _check_grads' relative bound
    # the bias sits in front of a BatchNorm on batch statistics, where a per-channel constant cancels:
    # its exact gradient is zero (float64 leaves 1e-17), held as _check_grads holds a zero reference;
    # test_odd_axes_... below holds a live bias gradient
    assert np.max(np.abs(rg[b])) < 1e-12 and np.max(np.abs(grads[b])) < 1e-7


def _down_head_graph():
    """down_graph plus a 1x1x1 sigmoid head at spatial (5, 6, 7): conv1(1 -> 4, bias) | down(4 -> 6,
    bias, relu) | conv1(-> 1, sigmoid); output (2, 3, 3); the planes z = 4 and x = 6 are dropped"""
    g, idx = dn.down_graph(4, 6, 1, 1, 0, (5, 6, 7), seed=8)
    g.finish(g.conv(g.output, 1, 1, use_bias=True, activation='sigmoid'))
    dn.randomize(g, 9)
    return g, g.nodes[idx]


def test_odd_axes_the_dropped_planes_get_a_zero_input_gradient(ctx):
    g, node = _down_head_graph()
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 5, 6, 7, 1)).astype(np.float32)
    y = (rng.random((2, 2, 3, 3, 1)) < 0.4).astype(np.uint8)
    rl, rm, rg, _, dx = dn.train_step64(g, x, y, want_input_grad_of=node.idx)
    assert not dx[:, 4].any() and not dx[:, :, :, 6].any() and np.abs(dx[:, :4, :, :6]).max() > 1e-6
    tr = _capi.Trainer(ctx, g)
    loss, acc = tr.step(x, y, seed=1)
    grads = tr.get_grads()
    assert abs(loss - rl) < 1e-5 * max(1.0, abs(rl)) and abs(acc - rm['acc']) < 1e-6
    # every gradient, the leading convolution's among them: its kernel gradient is
    # sum_v x[v] * dx[v, :] over ALL input voxels, so it is right only if the layer's input
    # gradient is - in the kept planes and in the dropped ones
    _check_grads(g, grads, rg)
    for s in node.weight_slots + g.nodes[1].weight_slots:
        print(g.weight_names[s], 'max |reference|', np.max(np.abs(rg[s])))
        assert np.max(np.abs(rg[s])) > 1e-6               # held by _check_grads' relative bound, not its zero branch
    # ... and EXACTLY zero there: with an input that is zero outside the dropped planes every term of
    # that sum is 0 * dx (kept planes) or x * dx (dropped planes), so the sum is exactly zero if and only
    # if every dx of a dropped plane is (the biases keep the rest of the network alive)
    x0 = np.zeros_like(x)
    x0[:, 4] = x[:, 4]
    x0[:, :, :, 6] = x[:, :, :, 6]
    tr.step(x0, y, seed=1)
    g0 = tr.get_grads()
    tr.close()
    k1 = g.nodes[1].weight_slots[0]
    assert not np.asarray(g0[k1]).any(), g0[k1]
    assert np.abs(g0[node.weight_slots[0]]).max() > 1e-6   # the step itself was a live one


def test_two_steps_from_equal_state_give_bit_equal_gradients(ctx):
    """EVERY gradient of tiny_vnet: it holds a Conv3DTranspose, so all its sums are in a fixed order
    (train.hip, `fixed_order`), and the new layer's own kernels use no float atomics"""
    g = dn.randomize(dn.tiny_vnet((22, 22, 22))[0])
    x, y = _train_batch(0)
    a, b = _capi.Trainer(ctx, g), _capi.Trainer(ctx, g)
    a.step(x, y, seed=5)
    b.step(x, y, seed=5)
    bad = [n for ga, gb, n in zip(a.get_grads(), b.get_grads(), g.weight_names) if not np.array_equal(ga, gb)]
    a.close()
    b.close()
    print('tensors that differ:', bad)
    assert not bad, bad


def _fresh_net():
    return FplNetwork(dn.tiny_vnet)


def test_fit_save_load_and_go_on(ctx, tmp_path):
    """three fit_generator steps lower the loss; save_network / load_network and the per-epoch
    checkpoints carry weights and Adam state bit for bit; one more step after load equals the
    uninterrupted run"""
    batch = _train_batch(77)
    full = _fresh_net()
    log = str(tmp_path / 'log.csv')
    full.train(iter([batch] * 3), 1, 3, log, str(tmp_path / 'ep'))
    rows = open(log).read().strip().splitlines()
    losses = [float(r.split(',')[2]) for r in rows[1:]]
    print('losses', losses)
    assert len(losses) == 3 and losses[2] < losses[0]
    part = _fresh_net()
    part.train(iter([batch] * 2), 1, 2, None, None)
    part.save_network(str(tmp_path / 'net'))
    back = fplnetwork.load_network(str(tmp_path / 'net'))
    assert back.train_single.opt_state is not None and back.train_single.opt_state[2] == 2
    for a, b in zip(part.train_single.get_weights(), back.train_single.get_weights()):
        assert np.array_equal(a, b)
    (m0, v0, _), (m1, v1, _) = part.train_single.opt_state, back.train_single.opt_state
    tr = [s for n in part.train_single.nodes for s in (n.weight_slots[:2] if n.kind == 'bn' else n.weight_slots)]
    assert all(np.array_equal(m0[s], m1[s]) and np.array_equal(v0[s], v1[s]) for s in tr)
    # a per-epoch checkpoint holds the layer too
    h = dn.tiny_vnet()[0]
    h.load(str(tmp_path / 'ep_002.h5'))
    for a, b in zip(full.train_single.get_weights(), h.get_weights()):
        assert np.array_equal(a, b)
    # weights after two steps, save, load and a third step: the bits of three uninterrupted steps
    back.train(iter([batch]), 1, 1, None, None)
    worst = {}
    for a, b, name in zip(full.train_single.get_weights(), back.train_single.get_weights(),
                          full.train_single.weight_names):
        if not np.array_equal(a, b):
            worst[name] = float(np.max(np.abs(a - b)))
    print('weights that differ (max abs)', worst)
    assert not worst, worst
    _NET['trained'] = full


def test_evaluate_in_inference_mode(ctx):
    net = _NET.get('trained')
    if net is None:
        net = _fresh_net()
        net.train(iter([_train_batch(77)] * 2), 1, 2, None, None)
    x, y = _train_batch(78)
    got = net.evaluate((x, y))
    pred = _capi.Program(ctx, net.train_single).forward(x)
    ref = dn.graph_forward64(net.train_single, x)
    assert pred.shape == ref.shape == y.shape and np.max(np.abs(pred - ref)) < TOL
    _means_close(got, valid.loss_sums_numpy(pred, y, 'binary_crossentropy'), ['acc', 'loss'])
    # ... and the loss (a) itself gives.  Per voxel |d bce / d p| <= 1 / min(p, 1 - p), and the two
    # predictions differ by less than TOL (held above), so the MEAN losses differ by at most the
    # mean of TOL / (min(p, 1 - p) - TOL) over the voxels (p clipped at 1e-7 as the loss clips it)
    want = valid.loss_sums_numpy(ref.astype(np.float32), y, 'binary_crossentropy')
    room = np.maximum(np.minimum(ref, 1 - ref) - TOL, 1e-7)
    margin = float(np.mean(TOL / room))
    print('loss', got['loss'], want[0] / want[7], 'margin', margin)
    assert margin < 0.05 * got['loss'] and abs(got['loss'] - want[0] / want[7]) <= margin


def test_launches_of_a_strided_conv_behind_a_lift(ctx, monkeypatch):
    """a batch of 3 at input tile 6 on the fp32 MFMA executor: one launch of the lift's kernel, one of
    the down-convolution's"""
    from tests import mfma_f32_cases as mc
    from tests.test_gpu_mfma_f32 import _run
    g, _ = dn.down_graph(16, 16, True, True, False, (6, 6, 6))
    want = {'mfma_conv1_f32': 1, 'mfma_down2_f32': 1}
    assert mc.predict_launches(g) == want
    x = np.random.default_rng(6).standard_normal((3, 6, 6, 6, 1)).astype(np.float32)
    got, = _run(ctx, monkeypatch, g, (x,), want)
    ref = dn.graph_forward64(g, x)
    assert got.shape == ref.shape == (3, 3, 3, 3, 16) and float(np.max(np.abs(got - ref))) < TOL
