"""GPU: Conv3DTranspose(filters, 2, strides=2) through the C ABI - the op alone on both fp32
executors, whole-volume inference, the training step, validation - against the float64
restatement (a) of tests/deconv_cases.py.  Gates: the fp32 executors' of tests/test_gpu_cnn.py
(TOL), the training step's of tests/test_gpu_train.py, the evaluator's of tests/test_gpu_valid.py.
Parity against Keras itself is UNPINNED (deconv_cases.py)."""
import numpy as np
import pytest

from flypylib_amd import FplNetwork, _capi, fplnetwork, valid
from tests import deconv_cases as dc
from tests.test_gpu_cnn import TOL
from tests.test_gpu_train import FLIP_GAP, _check_grads
from tests.test_gpu_validate_train import _means_close

pytestmark = pytest.mark.gpu

SPATIAL = [(1, 1, 1), (3, 4, 5), (7, 2, 9)]
# the issue's pairs: below, at and across the MFMA tile edges, and not multiples of anything;
# (96, 8): past the 48 input channels the kernel keeps in registers (its any-cin form)
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
                    g, _ = dc.deconv_graph(cin, cout, bias, relu, bn, spatial, seed=bias + 2 * relu + 4 * bn)
                    ref = dc.graph_forward64(g, x)
                    assert ref.shape == (batch,) + tuple(2 * s for s in spatial) + (cout,) and ref.std() > 1e-3
                    for perop in (False, True):
                        got = _forward(ctx, g, x, monkeypatch, perop)
                        assert got.shape == ref.shape
                        err = float(np.max(np.abs(got - ref)))
                        worst = max(worst, err)
                        assert err < TOL, (batch, bias, relu, bn, perop, err)
    print('max |gpu - float64|', worst)


@pytest.mark.parametrize('perop', [False, True])
@pytest.mark.parametrize('cin,cout', [(1, 3), (5, 6)])
def test_parity_position(ctx, monkeypatch, perop, cin, cout):
    """a one-hot input voxel in a one-hot channel lights exactly the eight output voxels
    2i + {0, 1}, and they hold W[a, b, c, :, ci]: a swapped (a, b, c) or (co, ci) order cannot pass"""
    spatial, at, ci = (3, 4, 5), (1, 2, 3), cin - 1
    g, node = dc.deconv_graph(cin, cout, 0, 0, 0, spatial)
    dnode = g.nodes[node]
    if cin > 1:                                           # the leading 1x1x1 conv routes the input to channel ci
        first = g.nodes[1]
        k = np.zeros((1, 1, 1, 1, cin), np.float32)
        k[..., ci] = 1.0
        g.weights[first.weight_slots[0]] = k
        g.weights[first.weight_slots[1]] = np.zeros(cin, np.float32)
    W = g.weights[dnode.weight_slots[0]]                  # (2,2,2,cout,cin), all distinct random values
    x = np.zeros((1,) + spatial + (1,), np.float32)
    x[(0,) + at + (0,)] = 1.0
    got = _forward(ctx, g, x, monkeypatch, perop)
    want = np.zeros_like(got)
    for a in range(2):
        for b in range(2):
            for c in range(2):
                want[0, 2 * at[0] + a, 2 * at[1] + b, 2 * at[2] + c, :] = W[a, b, c, :, ci]
    assert np.count_nonzero(want) == 8 * cout
    assert np.array_equal(got != 0, want != 0)
    assert np.max(np.abs(got - want)) <= 2.0 ** -23 * np.abs(want).max()     # one product with 1.0: exact up to an ulp


# ---- whole-volume inference ------------------------------------------------------------------
_NET = {}


def _net():
    """tiny_unet_t with non-trivial statistics, inference tile 22 (16 outputs); made once"""
    if 'net' not in _NET:
        net = FplNetwork(dc.tiny_unet_t_random)
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
    pred = dc.graph_forward64(net.infer_network.graph, np.stack(tiles)[..., None])[..., 0]
    for p, (z, y, x, shp) in zip(pred, where):
        v = tuple(s - 2 * off for s in shp)
        ref[z:z + v[0], y:y + v[1], x:x + v[2]] = p[:v[0], :v[1], :v[2]]
    return ref


def test_whole_volume_infer(ctx, monkeypatch):
    import torch
    net, vol = _net()
    assert net.rf_offset == (3, 3, 3) and net.infer_sz == (22, 22, 22)
    assert all((s - 6) % 16 for s in vol.shape)            # a partial tile on every axis
    if 'ref' not in _NET:
        _NET['ref'] = _lattice_reference(net, vol)
    ref = _NET['ref']
    pred = net.infer(vol)                                  # precision 'auto'
    assert ctx.last_path() == 'mfma_f32'
    err = float(np.max(np.abs(pred - ref)))
    print('max |gpu - float64| over the volume', err)
    assert pred.shape == vol.shape and err < TOL and ref[3:-3, 3:-3, 3:-3].std() > 1e-3
    assert not pred[:3].any() and not pred[:, :, -3:].any()
    # resident source and destination
    src = torch.from_numpy(vol).to('cuda:0')
    dst = torch.full(vol.shape, 7.0, dtype=torch.float32, device='cuda:0')
    net.infer_network.program.infer_volume(src, net.infer_sz, net.rf_offset, precision=_capi.PREC_F32,
                                           dst=dst, dims=vol.shape)
    assert ctx.last_path() == 'mfma_f32' and np.array_equal(dst.cpu().numpy(), pred)
    # run-to-run identity
    assert np.array_equal(net.infer(vol), pred)
    # the forced per-op executor: held to the same gate
    monkeypatch.setenv('FPL_FORCE_PEROP', '1')
    slow = net.infer(vol, precision='f32')
    assert ctx.last_path() == 'perop_f32' and np.max(np.abs(slow - ref)) < TOL
    monkeypatch.delenv('FPL_FORCE_PEROP')
    # super-tiles are declined for a graph with the layer: the switch changes nothing
    monkeypatch.setenv('FPL_NO_TILE_MERGE', '1')
    assert np.array_equal(net.infer(vol), pred)
    monkeypatch.delenv('FPL_NO_TILE_MERGE')
    for prec in ('f16s', 'f16', 'bf16'):
        with pytest.raises(Exception, match='Conv3DTranspose'):
            net.infer(vol, precision=prec)


# ---- training --------------------------------------------------------------------------------
def _train_batch(seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((2, 14, 14, 14, 1)).astype(np.float32)
    y = (rng.random((2, 8, 8, 8, 1)) < 0.3).astype(np.uint8)
    return x, y


def test_training_step_against_float64_autograd(ctx):
    g = dc.randomize(dc.tiny_unet_t((14, 14, 14))[0])
    for seed in range(0, 8000, 1000):                       # an input without near-tied pool windows
        x, y = _train_batch(seed)
        rl, rm, rg, gap = dc.train_step64(g, x, y)
        if gap > FLIP_GAP:
            break
    assert gap > FLIP_GAP
    tr = _capi.Trainer(ctx, g)
    loss, acc = tr.step(x, y, seed=5)
    grads = tr.get_grads()
    print('loss', loss, rl, 'acc', acc, rm['acc'])
    assert abs(loss - rl) < 1e-5 * max(1.0, abs(rl)) and abs(acc - rm['acc']) < 1e-6
    _check_grads(g, grads, rg)
    node = [n for n in g.nodes if n.kind == 'deconv'][0]
    for s, name in zip(node.weight_slots, ('kernel', 'bias')):
        assert g.weight_names[s] == 'deconv_%d/%s' % (node.idx, name)
        a, r = np.asarray(grads[s], np.float64), rg[s]
        if name == 'bias':
            # a per-channel constant in front of a BatchNorm on batch statistics cancels: the exact
            # gradient is zero (float64 leaves 1e-17), held as _check_grads holds a zero reference
            print(g.weight_names[s], 'max |g|', np.max(np.abs(a)), 'reference', np.max(np.abs(r)))
            assert np.max(np.abs(r)) < 1e-12 and np.max(np.abs(a)) < 1e-7
            continue
        rel = np.max(np.abs(a - r)) / np.max(np.abs(r))
        print(g.weight_names[s], 'rel err', rel)
        assert np.max(np.abs(r)) > 1e-6 and rel < 2e-4
    # equal state, equal bits for the new layer's own gradients: no float atomics in its kernels
    again = _capi.Trainer(ctx, g)
    again.step(x, y, seed=5)
    g2 = again.get_grads()
    for s in node.weight_slots:
        assert np.array_equal(grads[s], g2[s]), g.weight_names[s]
    tr.close()
    again.close()


def test_two_steps_from_equal_state_give_bit_equal_gradients(ctx):
    """EVERY gradient of tiny_unet_t.  In a network that holds the layer the convolutions' weight
    gradients are summed in a fixed order too (train.hip, `fixed_order`): the fp32 MFMA
    weight-gradient kernels, which add with float atomics, are not used there."""
    g = dc.randomize(dc.tiny_unet_t((14, 14, 14))[0])
    x, y = _train_batch(0)
    a, b = _capi.Trainer(ctx, g), _capi.Trainer(ctx, g)
    a.step(x, y, seed=5)
    b.step(x, y, seed=5)
    bad = [n for ga, gb, n in zip(a.get_grads(), b.get_grads(), g.weight_names) if not np.array_equal(ga, gb)]
    a.close()
    b.close()
    print('tensors that differ:', bad)
    assert not bad, bad


def test_training_step_relu_deconv_with_a_live_bias(ctx):
    """no BatchNorm behind the layer: its bias has a gradient, and its ReLU masks the arriving one"""
    from flypylib_amd.program import LayerGraph
    g = LayerGraph((6, 6, 6), seed=8)
    c = g.conv_bn_relu(g.input(), 4, 3)
    d = g.deconv(c, 6, use_bias=True, activation='relu')
    g.finish(g.conv(d, 1, 1, use_bias=True, activation='sigmoid'))
    dc.randomize(g)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 6, 6, 6, 1)).astype(np.float32)
    y = (rng.random((2, 8, 8, 8, 1)) < 0.4).astype(np.uint8)
    rl, rm, rg, _ = dc.train_step64(g, x, y)
    tr = _capi.Trainer(ctx, g)
    loss, acc = tr.step(x, y, seed=1)
    grads = tr.get_grads()
    assert abs(loss - rl) < 1e-5 * max(1.0, abs(rl)) and abs(acc - rm['acc']) < 1e-6
    _check_grads(g, grads, rg)
    for s in d.weight_slots:
        print(g.weight_names[s], 'max |reference|', np.max(np.abs(rg[s])))
        assert np.max(np.abs(rg[s])) > 1e-6             # held by _check_grads' relative bound, not its zero branch
    again = _capi.Trainer(ctx, g)
    again.step(x, y, seed=1)
    g2 = again.get_grads()
    for s in d.weight_slots:                              # the layer's own sums: fixed order, equal bits
        assert np.array_equal(grads[s], g2[s]), g.weight_names[s]
    tr.close()
    again.close()


def _fresh_net():
    return FplNetwork(dc.tiny_unet_t)


def test_fit_save_load_and_go_on(ctx, tmp_path):
    """three fit_generator steps lower the loss; save_network / load_network and the per-epoch
    checkpoints carry weights and Adam state bit for bit"""
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
    h = dc.tiny_unet_t((14, 14, 14))[0]
    h.load(str(tmp_path / 'ep_002.h5'))
    for a, b in zip(full.train_single.get_weights(), h.get_weights()):
        assert np.array_equal(a, b)
    _NET['trained'] = full


def test_one_more_step_after_load_equals_the_uninterrupted_run(ctx, tmp_path):
    """weights after two steps, save_network, load_network and a third step: the bits of three
    uninterrupted steps (every sum of the step has a fixed order, and the saved state is exact)"""
    batch = _train_batch(77)
    full = _fresh_net()
    full.train(iter([batch] * 3), 1, 3, None, None)
    part = _fresh_net()
    part.train(iter([batch] * 2), 1, 2, None, None)
    part.save_network(str(tmp_path / 'net'))
    back = fplnetwork.load_network(str(tmp_path / 'net'))
    back.train(iter([batch]), 1, 1, None, None)
    worst = {}
    for a, b, name in zip(full.train_single.get_weights(), back.train_single.get_weights(),
                          full.train_single.weight_names):
        if not np.array_equal(a, b):
            worst[name] = float(np.max(np.abs(a - b)))
    print('weights that differ (max abs)', worst)
    assert not worst, worst


def test_evaluate_in_inference_mode(ctx):
    net = _NET.get('trained')
    if net is None:
        net = _fresh_net()
        net.train(iter([_train_batch(77)] * 2), 1, 2, None, None)
    x, y = _train_batch(78)
    got = net.evaluate((x, y))
    pred = _capi.Program(ctx, net.train_single).forward(x)
    ref = dc.graph_forward64(net.train_single, x)
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


def _launches_at_tile_6(ctx, monkeypatch, graph, want):
    """forward of a batch of 3 at input tile 6 on the fp32 MFMA executor: the TimedLaunch names and
    counts are `want`, the result is the float64 restatement's within TOL"""
    from tests import mfma_f32_cases as mc
    from tests.test_gpu_mfma_f32 import _run
    assert mc.predict_launches(graph) == want
    x = np.random.default_rng(6).standard_normal((3, 6, 6, 6, 1)).astype(np.float32)
    got, = _run(ctx, monkeypatch, graph, (x,), want)
    ref = dc.graph_forward64(graph, x)
    assert got.shape == ref.shape and float(np.max(np.abs(got - ref))) < TOL


def test_launches_of_a_conv3dtranspose_behind_a_lift(ctx, monkeypatch):
    g, _ = dc.deconv_graph(16, 16, True, True, False, (6, 6, 6))
    _launches_at_tile_6(ctx, monkeypatch, g, {'mfma_conv1_f32': 1, 'mfma_deconv2_f32': 1})


def test_launches_of_a_concatenation_that_a_1x1x1_conv_reads(ctx, monkeypatch):
    """in a program that holds a Conv3DTranspose such a concatenation is written out"""
    from flypylib_amd.program import LayerGraph
    g = LayerGraph((6, 6, 6), seed=5)
    lift = g.conv(g.input(), 16, 1, use_bias=True)
    u = g.deconv(g.pool(lift), 16, use_bias=True, activation='relu')
    g.finish(g.conv(g.concat(u, lift), 8, 1, use_bias=True))
    dc.randomize(g)
    _launches_at_tile_6(ctx, monkeypatch, g, {'mfma_conv1_f32': 2, 'mfma_pool_f32': 1, 'mfma_deconv2_f32': 1,
                                              'mfma_concat_f32': 1})
