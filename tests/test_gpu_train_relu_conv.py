"""GPU parity of the training step with ReLU-activated convolutions (unet_like_vol; the ReLU
in the conv kernels' epilogue, the in-place gradient mask of the backward pass) against the
float64 torch-autograd oracle, with test_gpu_train.py's bounds: loss within 1e-5 max(1, |loss|),
accuracy within 1e-6, every gradient tensor within 2e-4 of its largest oracle entry.  The
inputs are picked on the CPU (tests/relu_conv_cases.py) clear of max-pool ties and of ReLU
pre-activations at rounding distance from zero."""
import numpy as np
import pytest

from flypylib_amd import _capi, fplmodels
from oracle import train_oracle
from tests import relu_conv_cases as rc

pytestmark = pytest.mark.gpu

VOL_LOSS = 'masked_weighted_binary_crossentropy'


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-12)


def _check_grads(graph, grads, rg):
    """every gradient tensor within 2e-4 (relative to its largest entry) of the oracle's"""
    worst = 0.0
    for i, (g, r) in enumerate(zip(grads, rg)):
        if np.max(np.abs(r)) < 1e-12:
            assert np.max(np.abs(g)) < 1e-7, graph.weight_names[i]
            continue
        worst = max(worst, _rel(g, r))
        assert _rel(g, r) < 2e-4, '%s: rel err %g' % (graph.weight_names[i], _rel(g, r))
    return worst


_VOL = {}


def _vol_case(shape):
    """graph, labels and the oracle's step on the picked input; computed once per shape and
    shared (read-only) by the tests below"""
    if shape not in _VOL:
        g = rc.vol_graph(shape[1])
        labels = rc.vol_labels(shape)
        data, rl, rm, rg = rc.pick_input(g, shape, rc.VOL_DATA_SEED, labels,
                                         rc.GAPS['vol_%d' % shape[1]], loss=VOL_LOSS)
        _VOL[shape] = (g, labels, data, rl, rm, rg)
    return _VOL[shape]


@pytest.mark.parametrize('shape', rc.VOL_SHAPES, ids=lambda s: '%dx%d' % (s[0], s[1]))
def test_unet_like_vol_step_matches_the_oracle(ctx, shape):
    """the two smallest trainable patches: 14^3 (2^3 outputs, a 1^3 bottleneck) and 18^3 (odd 3^3
    at the bottom), loss masked_weighted_binary_crossentropy with the mask class present, and
    the returned masked_accuracy.  The gradients of c1's weights (conv_1, conv_2) cover a ReLU
    output with two consumers: c1 feeds the pool and the crop, both of which have added their
    share to its gradient before the mask runs."""
    g, labels, data, rl, rm, rg = _vol_case(shape)
    assert set(np.unique(labels)) == {0, 1, 2}
    tr = _capi.Trainer(ctx, g, loss=VOL_LOSS)
    loss, acc = tr.step(data, labels, seed=5)
    m = tr.metrics()
    print('loss %.7g (oracle %.7g), acc %.7g (%.7g), masked_accuracy %.7g (%.7g)'
          % (loss, rl, acc, rm['acc'], m['masked_accuracy'], rm['masked_accuracy']))
    assert abs(loss - rl) < 1e-5 * max(1.0, abs(rl)), (loss, rl)
    assert abs(acc - rm['acc']) < 1e-6
    assert abs(m['masked_accuracy'] - rm['masked_accuracy']) < 1e-6
    for k in ('lb0l1err', 'lb1l1err'):
        assert abs(m[k] - rm[k]) < 1e-5, (k, m[k], rm[k])
    print('worst gradient tensor %.2e' % _check_grads(g, tr.get_grads(), rg))
    tr.close()


@pytest.mark.parametrize('name', sorted(rc.BRANCHES))
def test_every_conv_branch_with_a_relu_epilogue(ctx, monkeypatch, name):
    """conv(relu) -> conv(relu) -> sigmoid head, one graph per kernel branch that applies the
    activation: the cin = 1 stem, fp32 MFMA 3x3x3, split halves (96 -> 64, 80 -> 32) and the same
    two on the fp32 kernels (FPL_TRAIN_F32CONV), 1x1x1 32 -> 64 and 64 -> 64, the direct
    kernels (FPL_TRAIN_DIRECT=3), biases (the bias gradient sees the masked dy), and a ReLU
    output of 54 = 4 * 13 + 2 elements (the scalar tail of the mask kernel)."""
    build, shape, env = rc.BRANCHES[name]
    g = build()
    labels = rc.branch_labels(rc.out_shape(g, shape))
    data, rl, rm, rg = rc.pick_input(g, shape, 11, labels, rc.GAPS[name])
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tr = _capi.Trainer(ctx, g)
    loss, acc = tr.step(data, labels, seed=5)
    assert abs(loss - rl) < 1e-5 * max(1.0, abs(rl)), (loss, rl)
    assert abs(acc - rm['acc']) < 1e-6
    print('%s: worst gradient tensor %.2e' % (name, _check_grads(g, tr.get_grads(), rg)))
    tr.close()


def test_fused_relu_agrees_with_the_separate_passes(ctx, monkeypatch):
    """FPL_TRAIN_CONVRELU_SEPARATE=1 runs every ReLU conv as conv (no activation) -> relu_fwd
    and relu_bwd in the backward pass: kernels that existed before the fused path.  Both paths
    see bit-identical pre-activations, hence identical masks: equal loss, gradients within 1e-6
    of each tensor's largest entry."""
    g, labels, data, rl, rm, rg = _vol_case(rc.VOL_SHAPES[0])
    tr = _capi.Trainer(ctx, g, loss=VOL_LOSS)
    loss_f, acc_f = tr.step(data, labels, seed=5)
    grads_f = [x.copy() for x in tr.get_grads()]
    tr.close()
    monkeypatch.setenv('FPL_TRAIN_CONVRELU_SEPARATE', '1')
    tr2 = _capi.Trainer(ctx, g, loss=VOL_LOSS)
    loss_s, acc_s = tr2.step(data, labels, seed=5)
    grads_s = tr2.get_grads()
    tr2.close()
    worst = max(_rel(a, b) for a, b in zip(grads_f, grads_s))
    print('fused vs separate: loss %.9g / %.9g, worst gradient tensor %.2e' % (loss_f, loss_s, worst))
    assert loss_f == loss_s and acc_f == acc_s
    _check_grads(g, grads_s, rg)                   # the cross-check path holds the oracle too
    for i, (a, b) in enumerate(zip(grads_f, grads_s)):
        assert _rel(a, b) < 1e-6, '%s: %g' % (g.weight_names[i], _rel(a, b))


def test_engine_refuses_a_relu_head_and_a_relu_conv_before_bn(ctx):
    from flypylib_amd.program import LayerGraph
    g = LayerGraph(None, seed=1)
    g.finish(g.conv(g.conv(g.input(), 8, 3, activation='relu'), 1, 1, activation='relu'))
    with pytest.raises(RuntimeError, match='head needs a sigmoid'):
        _capi.Trainer(ctx, g)
    g = LayerGraph(None, seed=1)
    x = g.bn_relu(g.conv(g.input(), 8, 3, activation='relu'))
    g.finish(g.conv(x, 1, 1, activation='sigmoid'))
    with pytest.raises(RuntimeError, match='relu activation feeding BatchNorm'):
        _capi.Trainer(ctx, g)


def test_adam_over_steps_matches_the_oracle(ctx):
    """Adam over 3 steps on the 14^3 shape, as test_gpu_train.test_adam_updates_match_oracle_over_steps:
    the update rule is checked by feeding the oracle optimizer the engine's own gradients"""
    shape = rc.VOL_SHAPES[0]
    g = rc.vol_graph(shape[1], seed=6)
    tr = _capi.Trainer(ctx, g, loss=VOL_LOSS)
    adam = train_oracle.Adam(g)
    w_ref = [w.astype(np.float64) for w in g.weights]
    rng = np.random.default_rng(4)
    for step in range(3):
        data = rng.standard_normal(shape).astype(np.float32)
        labels = rng.integers(0, 3, (shape[0], 2, 2, 2, 1)).astype(np.uint8)
        w_before = tr.get_weights()
        loss, _ = tr.step(data, labels, seed=step)
        rl, _, _ = train_oracle.train_step(g, w_before, data, labels, step, loss=VOL_LOSS)
        assert abs(loss - rl) < 1e-4 * max(1.0, abs(rl))
        w_ref = adam.apply(w_ref, tr.get_grads())
        tr.apply(1.0)
    for i, (a, b) in enumerate(zip(tr.get_weights(), w_ref)):
        assert np.max(np.abs(a - b)) < 2e-6 + 1e-5 * np.max(np.abs(b)), g.weight_names[i]
    tr.close()


def test_unet_like_vol_trains_saves_and_resumes(ctx, tmp_path):
    """FplNetwork(unet_like_vol) with the factory's compile args: 2 epochs x 4 steps from
    gen_volume's host generator on a tiny synthetic volume (18^3 patches, its 6^3 labels) lower
    the loss; make_train_parallel(1, ...) trains too; save_network -> load_network (weights and
    Adam's optimizer_weights) -> one more step reproduces the unsaved network's step."""
    from flypylib_amd import FplNetwork, fplnetwork, fplobjdetect
    rng = np.random.RandomState(0)
    img = rng.randn(40, 40, 40).astype(np.float32)
    lab = np.zeros((40, 40, 40), np.uint8)
    lab[16:24, 16:24, 16:24] = 1
    img[lab == 1] += 2.0                       # learnable: bright cube = label 1
    mask = np.ones((40, 40, 40), np.uint8)
    mask[:, :, 30:] = 0                        # masked-out voxels become label 2
    net = FplNetwork(fplmodels.unet_like_vol)
    loss = net.compile_args['loss']
    assert getattr(loss, '__name__', loss) == VOL_LOSS
    gen = fplobjdetect.gen_volume([(img, lab, mask)], 18, 4, 0.5, rng=rng)
    log = str(tmp_path / 'vol.csv')
    net.train(gen, 4, 2, log, None)
    rows = open(log).read().strip().splitlines()
    assert rows[0] == 'epoch,loss,masked_accuracy' and len(rows) == 3
    assert float(rows[2].split(',')[1]) < float(rows[1].split(',')[1])
    # save, load, and the same further step on both
    path = str(tmp_path / 'net')
    net.save_network(path)
    net2 = fplnetwork.load_network(path)
    assert net2.train_single.opt_state is not None and net2.train_single.opt_state[2] == 8
    for a, b in zip(net.train_single.get_weights(), net2.train_single.get_weights()):
        assert np.array_equal(a, b)
    x, y = next(gen)
    x, y = x.copy(), y.copy()
    out = []
    for n in (net, net2):
        log_n = str(tmp_path / ('step_%d.csv' % len(out)))
        n.train(iter([(x, y)]), 1, 1, log_n, None)
        tr = n._trainer[1]
        out.append((open(log_n).read().strip().splitlines()[1], tr.get_grads(), tr.get_opt_state()))
    (row_a, grads_a, opt_a), (row_b, grads_b, opt_b) = out
    la, lb = float(row_a.split(',')[1]), float(row_b.split(',')[1])
    assert abs(la - lb) < 1e-6 * max(1.0, abs(la)), (row_a, row_b)
    assert opt_a[2] == opt_b[2] == 9
    for i, (a, b) in enumerate(zip(grads_a, grads_b)):
        assert _rel(a, b) < 1e-5, i                  # float atomics in the weight gradients
    for a, b in zip(opt_a[0], opt_b[0]):             # Adam's first moments after the step
        assert _rel(a, b) < 1e-5
    # the single-process form of make_train_parallel
    net.make_train_parallel(1, 4, 18)
    hist_log = str(tmp_path / 'par.csv')
    net.train(gen, 2, 1, hist_log, None)
    assert np.isfinite(float(open(hist_log).read().strip().splitlines()[1].split(',')[1]))
