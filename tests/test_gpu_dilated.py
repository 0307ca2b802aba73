"""GPU: Conv3D(filters, 3, dilation_rate=2) through the C ABI - the op alone on both fp32 executors,
tap positions, whole-volume inference, a stride-2 program, the training step, validation and the
public surface - against the float64 restatement (a) of tests/dilated_cases.py.  Gates: the fp32
executors' of tests/test_gpu_cnn.py (TOL), the training step's of tests/test_gpu_train.py, the
evaluator's of tests/test_gpu_validate_train.py.  Parity against Keras itself is UNPINNED
(dilated_cases.py)."""
import numpy as np
import pytest

from flypylib_amd import FplNetwork, _capi, fplnetwork, valid
from flypylib_amd.program import LayerGraph
from tests import dilated_cases as di
from tests.test_gpu_cnn import TOL
from tests.test_gpu_train import FLIP_GAP, _check_grads
from tests.test_gpu_validate_train import _means_close

pytestmark = pytest.mark.gpu

# outputs 1^3, 2 x 5 x 4 and 5 x 2 x 17: one voxel (seven of the eight parity classes are empty),
# ragged classes, and across the 4-row and 16-column edges of a class's blocks (17 columns are 9 + 8
# per class; 5 planes are 3 + 2)
SPATIAL = [(5, 5, 5), (6, 9, 8), (9, 6, 21)]
# below, at and across the 16-channel chunk and the 16-output block: (1,4) the ragged channel tail,
# (3,5) scalar stores, (16,16) one whole chunk, (17,33) two chunks and three blocks with tails,
# (48,32) and (96,8) three and six chunks
CHANNELS = [(1, 4), (3, 5), (16, 16), (17, 33), (48, 32), (96, 8)]


def _set_perop(monkeypatch, perop):
    if perop:
        monkeypatch.setenv('FPL_FORCE_PEROP', '1')
    else:
        monkeypatch.delenv('FPL_FORCE_PEROP', raising=False)


def _forward(ctx, graph, x, monkeypatch, perop):
    _set_perop(monkeypatch, perop)
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
                    g, _ = di.dilated_graph(cin, cout, bias, relu, bn, spatial, seed=bias + 2 * relu + 4 * bn)
                    ref = di.graph_forward64(g, x)
                    assert ref.shape == (batch,) + tuple(s - 4 for s in spatial) + (cout,)
                    assert np.abs(ref).max() > 1e-3                # a live reference
                    for perop in (False, True):
                        got = _forward(ctx, g, x, monkeypatch, perop)
                        assert got.shape == ref.shape
                        err = float(np.max(np.abs(got - ref)))
                        worst = max(worst, err)
                        assert err < TOL, (batch, bias, relu, bn, perop, err)
    print('max |gpu - float64|', worst)


def _one_hot_graph(cin, cout, ci, spatial):
    g, node = di.dilated_graph(cin, cout, 0, 0, 0, spatial)
    if cin > 1:                                           # the leading 1x1x1 conv routes the input to channel ci
        first = g.nodes[1]
        k = np.zeros((1, 1, 1, 1, cin), np.float32)
        k[..., ci] = 1.0
        g.weights[first.weight_slots[0]] = k
        g.weights[first.weight_slots[1]] = np.zeros(cin, np.float32)
    W = g.weights[g.nodes[node].weight_slots[0]]          # (3,3,3,cin,cout), random values
    assert np.unique(W).size == W.size                    # all distinct: a swapped tap cannot hide
    return g, W


@pytest.mark.parametrize('perop', [False, True])
@pytest.mark.parametrize('cin,cout', [(1, 3), (5, 6), (20, 6)])
def test_tap_position(ctx, monkeypatch, perop, cin, cout):
    """a one-hot input voxel p in the last input channel lights exactly the outputs p - 2t that lie
    in range, each holding W[t, ci, :]: a swapped tap or (ci, co) order cannot pass, and neither
    can a dilation-1 kernel, which would light the outputs at odd offsets from p"""
    spatial, ci = (7, 6, 9), cin - 1
    osz = tuple(s - 4 for s in spatial)                    # (3, 2, 5)
    g, W = _one_hot_graph(cin, cout, ci, spatial)
    _set_perop(monkeypatch, perop)
    prog = _capi.Program(ctx, g)
    try:
        for p, lit in (((3, 2, 4), 3), ((0, 0, 0), 1), ((6, 5, 8), 1), ((2, 3, 5), 4)):
            x = np.zeros((1,) + spatial + (1,), np.float32)
            x[(0,) + p + (0,)] = 1.0
            got = prog.forward(x)
            assert ctx.last_path() == ('perop_f32' if perop else 'mfma_f32')
            want = np.zeros((1,) + osz + (cout,), np.float32)
            n = 0
            for t in np.ndindex(3, 3, 3):
                o = tuple(pi - 2 * ti for pi, ti in zip(p, t))
                if all(0 <= oi < si for oi, si in zip(o, osz)):
                    want[(0,) + o] = W[t + (ci,)]
                    n += 1
            assert n == lit and got.shape == want.shape and np.count_nonzero(want) == lit * cout
            # everything else - the odd offsets from p among it - is exactly zero
            assert np.array_equal(got != 0, want != 0), p
            # one product with 1.0: exact up to an ulp
            assert np.max(np.abs(got - want)) <= 2.0 ** -23 * np.abs(want).max(), p
    finally:
        prog.close()


# ---- whole-volume inference ------------------------------------------------------------------
def _lattice_reference(net, vol):
    """(a) over the reference's tile lattice: origins off, off + out, ...; edge tiles zero padded;
    a network of output stride s repeats every prediction s times per axis (UpSampling3D)"""
    tile, off, s = net.infer_sz[0], net.rf_offset[0], net.rf_stride[0]
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
    pred = di.graph_forward64(net.infer_network.graph, np.stack(tiles)[..., None])[..., 0]
    pred = pred.repeat(s, axis=1).repeat(s, axis=2).repeat(s, axis=3)
    assert pred.shape[1:] == (out,) * 3
    for p, (z, y, x, shp) in zip(pred, where):
        v = tuple(n - 2 * off for n in shp)
        ref[z:z + v[0], y:y + v[1], x:x + v[2]] = p[:v[0], :v[1], :v[2]]
    return ref


def _border_is_zero(pred, off):
    return not (pred[:off].any() or pred[-off:].any() or pred[:, :off].any() or pred[:, -off:].any()
                or pred[:, :, :off].any() or pred[:, :, -off:].any())


def test_whole_volume_infer(ctx, monkeypatch):
    net = FplNetwork(di.tiny_atrous_random)
    net._set_infer()
    vol = np.random.default_rng(2).standard_normal((35, 41, 47)).astype(np.float32)
    assert net.rf_offset == (5, 5, 5) and net.infer_sz == (22, 22, 22) and net.rf_stride == (1, 1, 1)
    assert all((s - 10) % 12 for s in vol.shape)           # a partial tile on every axis
    ref = _lattice_reference(net, vol)
    pred = net.infer(vol)                                  # precision 'auto'
    assert ctx.last_path() == 'mfma_f32'
    err = float(np.max(np.abs(pred - ref)))
    print('max |gpu - float64| over the volume', err)
    assert pred.shape == vol.shape and err < TOL and ref[5:-5, 5:-5, 5:-5].std() > 1e-3
    assert _border_is_zero(pred, 5)
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
        with pytest.raises(Exception, match=r'Conv3D\(filters, 3, dilation_rate=2\)'):
            net.infer(vol, precision=prec)


def _pooled_factory(in_sz=None):
    """conv3(1->8) BN ReLU | pool | dilated(8->12, bias) BN ReLU | conv1(->1, sigmoid), output stride 2"""
    in_sz = (22, 22, 22) if in_sz is None else in_sz
    g = LayerGraph(in_sz, seed=6)
    c1 = g.conv_bn_relu(g.input(), 8, 3)
    d = g.bn_relu(g.dilated(g.pool(c1), 12, use_bias=True))
    g.finish(g.conv(d, 1, 1, use_bias=True, activation='sigmoid'))
    # derived here: the field grows by (k - 1) * step of the lattice the layer works on - 3 for the
    # conv3 (step 1), + 1 for the pool, + 2 * 2 * 2 for the dilated layer's taps, 2 coarse voxels = 4
    # fine ones apart (step 2): 3 + 1 + 8 = 12.  Sizes 22 -> 20 -> 10 -> 6, upsampled by the stride: 12
    # outputs, so the offset is (22 - 12) / 2 = 5.
    return di.randomize(g), (12, 5, 2), in_sz, None


def test_a_stride_2_program(ctx, monkeypatch):
    net = FplNetwork(_pooled_factory)
    net._set_infer()
    g = net.infer_network.graph
    assert g.output.size == (6, 6, 6) and net.rf_stride == (2, 2, 2)
    # the field by (a): coarse output o reads the input voxels 2 o .. 2 o + 11 and no other
    rng = np.random.default_rng(1)
    x = rng.standard_normal((1, 22, 22, 22, 1))
    base = di.graph_forward64(g, x)
    for p in (0, 11, 12, 21):
        for axis in range(3):
            x2 = x.copy()
            idx = [0, 7, 7, 7, 0]
            idx[1 + axis] = p
            x2[tuple(idx)] += 1.0
            moved = np.abs(di.graph_forward64(g, x2) - base).max(axis=tuple(a for a in range(5) if a != 1 + axis))
            assert [bool(m > 0) for m in moved] == [2 * o <= p <= 2 * o + 11 for o in range(6)], (p, axis)
    vol = np.random.default_rng(4).standard_normal((37, 49, 61)).astype(np.float32)
    assert all((s - 10) % 12 for s in vol.shape)
    ref = _lattice_reference(net, vol)
    pred = net.infer(vol)
    assert ctx.last_path() == 'mfma_f32'
    err = float(np.max(np.abs(pred - ref)))
    print('max |gpu - float64| over the volume', err)
    assert err < TOL and ref[5:-5, 5:-5, 5:-5].std() > 1e-3 and _border_is_zero(pred, 5)
    monkeypatch.setenv('FPL_NO_TILE_MERGE', '1')
    assert np.array_equal(net.infer(vol), pred)
    assert ctx.last_path() == 'mfma_f32'


# ---- training --------------------------------------------------------------------------------
def _train_batch(seed, patch=22):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((2,) + (patch,) * 3 + (1,)).astype(np.float32)
    y = (rng.random((2,) + (patch - 10,) * 3 + (1,)) < 0.3).astype(np.uint8)
    return x, y


@pytest.mark.parametrize('patch', [22, 23])
def test_training_step_against_float64_autograd(ctx, patch):
    """patch 22: 20 -> 16 -> 12; patch 23: 21 -> 17 -> 13, odd sizes behind the layers"""
    g = di.randomize(di.tiny_atrous((patch,) * 3)[0])
    first, second = [n for n in g.nodes if n.kind == 'dilated']
    x, y = _train_batch(patch, patch)
    rl, rm, rg, gap, dx = di.train_step64(g, x, y, want_input_grad_of=second.idx)
    assert gap > FLIP_GAP                                  # (no max-pool in this network: nothing can flip)
    tr = _capi.Trainer(ctx, g)
    loss, acc = tr.step(x, y, seed=5)
    grads = tr.get_grads()
    tr.close()
    print('loss', loss, rl, 'acc', acc, rm['acc'])
    assert abs(loss - rl) < 1e-5 * max(1.0, abs(rl)) and abs(acc - rm['acc']) < 1e-6
    # every gradient: those of the first layers are right only if both dilated layers' input
    # gradients are, which everything in front of them is a function of
    _check_grads(g, grads, rg)
    assert dx.shape == (2,) + (patch - 6,) * 3 + (12,) and np.abs(dx).max() > 1e-8
    k1, b1 = first.weight_slots
    (k2,) = second.weight_slots
    assert g.weight_names[k1] == 'dilated_%d/kernel' % first.idx
    for s in (k1, k2, g.nodes[1].weight_slots[0]):
        print(g.weight_names[s], 'max |reference|', np.max(np.abs(rg[s])))
        assert np.max(np.abs(rg[s])) > 1e-6                # held by _check_grads' relative bound
    # the first layer's bias sits in front of a BatchNorm on batch statistics, where a per-channel
    # constant cancels: its exact gradient is zero (float64 leaves 1e-17).  Expected, not gated beyond
    # what _check_grads asks of a zero reference; test_the_input_gradient_... holds a live bias gradient
    print('first dilated bias: max |reference|', np.max(np.abs(rg[b1])), 'gpu', np.max(np.abs(grads[b1])))
    assert np.max(np.abs(rg[b1])) < 1e-12


def _head_graph():
    """conv1(1 -> 4, bias) | dilated(4 -> 6, bias, relu) | conv1(-> 1, sigmoid) at spatial (7, 6, 9):
    no BatchNorm behind the layer's bias, so its gradient is live"""
    g, idx = di.dilated_graph(4, 6, 1, 1, 0, (7, 6, 9), seed=8)
    g.finish(g.conv(g.output, 1, 1, use_bias=True, activation='sigmoid'))
    di.randomize(g, 9)
    return g, g.nodes[idx]


def test_the_input_gradient_and_a_live_bias_gradient(ctx):
    g, node = _head_graph()
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 7, 6, 9, 1)).astype(np.float32)
    y = (rng.random((2, 3, 2, 5, 1)) < 0.4).astype(np.uint8)
    rl, rm, rg, _, dx = di.train_step64(g, x, y, want_input_grad_of=node.idx)
    # every input voxel is read by some tap of some output here: the input gradient is live everywhere
    assert dx.shape == (2, 7, 6, 9, 4) and np.abs(dx).min(axis=-1).max() > 1e-6
    tr = _capi.Trainer(ctx, g)
    loss, acc = tr.step(x, y, seed=1)
    grads = tr.get_grads()
    tr.close()
    assert abs(loss - rl) < 1e-5 * max(1.0, abs(rl)) and abs(acc - rm['acc']) < 1e-6
    # the leading convolution's kernel gradient is sum_v x[v] * dx[v, :] over ALL input voxels and its
    # bias gradient sum_v dx[v, :]: they are right only if the layer's input gradient is
    _check_grads(g, grads, rg)
    first = g.nodes[1]
    want_k = np.einsum('ndhw,ndhwc->c', x[..., 0].astype(np.float64), dx)
    assert np.allclose(rg[first.weight_slots[0]].reshape(-1), want_k, rtol=1e-9, atol=1e-12)
    for s in node.weight_slots + first.weight_slots:
        print(g.weight_names[s], 'max |reference|', np.max(np.abs(rg[s])))
        assert np.max(np.abs(rg[s])) > 1e-6               # held by _check_grads' relative bound, not its zero branch


def test_two_trainers_from_equal_state_give_equal_bits_after_two_steps(ctx):
    """the layer's own gradients use no float atomics, and a network that holds it trains with every
    weight gradient summed in a fixed order (train.hip, `fixed_order`): every gradient of the first
    step and every weight after two steps has equal bits in two trainers"""
    g = di.randomize(di.tiny_atrous()[0])
    x, y = _train_batch(0)
    a, b = _capi.Trainer(ctx, g), _capi.Trainer(ctx, g)
    for step in range(2):
        for t in (a, b):
            t.step(x, y, seed=5 + step)
        bad = [n for ga, gb, n in zip(a.get_grads(), b.get_grads(), g.weight_names) if not np.array_equal(ga, gb)]
        assert not bad, (step, bad)
        for t in (a, b):
            t.apply()
    wa, wb = a.get_weights(), b.get_weights()
    a.close()
    b.close()
    bad = [n for u, v, n in zip(wa, wb, g.weight_names) if not np.array_equal(u, v)]
    print('tensors that differ:', bad)
    assert not bad, bad
    assert any(not np.array_equal(u, w) for u, w in zip(wa, g.weights))      # the steps were applied


def test_fit_save_load_infer_and_evaluate(ctx, tmp_path):
    """the public surface: a factory that uses the layer trains for two steps, saves, loads and
    infers; the loaded network's prediction equals the saved one's bit for bit; evaluate agrees with
    the specification on the inference-mode prediction"""
    batch = _train_batch(77)
    net = FplNetwork(di.tiny_atrous)
    log = str(tmp_path / 'log.csv')
    net.train(iter([batch] * 2), 1, 2, log, str(tmp_path / 'ep'))
    losses = [float(r.split(',')[2]) for r in open(log).read().strip().splitlines()[1:]]
    print('losses', losses)
    assert len(losses) == 2 and losses[1] < losses[0]
    vol = np.random.default_rng(9).standard_normal((30, 34, 38)).astype(np.float32)
    pred = net.infer(vol)
    assert ctx.last_path() == 'mfma_f32' and pred[5:-5, 5:-5, 5:-5].std() > 1e-4
    net.save_network(str(tmp_path / 'net'))
    back = fplnetwork.load_network(str(tmp_path / 'net'))
    assert back.train_single.opt_state is not None and back.train_single.opt_state[2] == 2
    for a, b in zip(net.train_single.get_weights(), back.train_single.get_weights()):
        assert np.array_equal(a, b)
    assert np.array_equal(back.infer(vol), pred)
    # the last per-epoch checkpoint (epochs count from 0) holds the layers too
    h = di.tiny_atrous()[0]
    h.load(str(tmp_path / 'ep_001.h5'))
    for a, b in zip(net.train_single.get_weights(), h.get_weights()):
        assert np.array_equal(a, b)
    # evaluate: inference mode, against valid.loss_sums_numpy on the engine's own prediction
    x, y = _train_batch(78)
    got = net.evaluate((x, y))
    fwd = _capi.Program(ctx, net.train_single).forward(x)
    ref = di.graph_forward64(net.train_single, x)
    assert fwd.shape == ref.shape == y.shape and np.max(np.abs(fwd - ref)) < TOL
    _means_close(got, valid.loss_sums_numpy(fwd, y, 'binary_crossentropy'), ['acc', 'loss'])


def test_launches_of_a_dilated_conv_of_two_slices_behind_a_lift(ctx, monkeypatch):
    """a batch of 3 at input tile 6 on the fp32 MFMA executor: 65 outputs are two launches of the
    atrous kernel (64 + 1)"""
    from tests import mfma_f32_cases as mc
    from tests.test_gpu_mfma_f32 import _run
    g, _ = di.dilated_graph(16, 65, True, True, False, (6, 6, 6))
    want = {'mfma_conv1_f32': 1, 'mfma_atrous3_f32': 2}
    assert mc.predict_launches(g) == want
    x = np.random.default_rng(6).standard_normal((3, 6, 6, 6, 1)).astype(np.float32)
    got, = _run(ctx, monkeypatch, g, (x,), want)
    ref = di.graph_forward64(g, x)
    assert got.shape == ref.shape == (3, 2, 2, 2, 65) and float(np.max(np.abs(got - ref))) < TOL
