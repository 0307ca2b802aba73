"""GPU: held-out validation through the public interface - FplNetwork.evaluate on one fixed
batch against the numpy specification applied to the GPU's own inference-mode prediction (itself
held to the oracle), that evaluate changes nothing, the val_ columns of FplNetwork.train, and
what validation_data takes and refuses.

The evaluator's means are held to the bound of tests/test_gpu_valid.py on the sums, divided by
the mean's divisor: counts exact, real sums within 1e-12 * max(n, |ref|)."""
import numpy as np
import pytest

from flypylib_amd import FplNetwork, _capi, fplmodels, fplobjdetect, valid
from oracle import cnn_oracle
from tests.test_gpu_cnn import TOL          # the tolerance of fpl_program_forward against the oracle

pytestmark = pytest.mark.gpu

# factory -> (patch edge, batch, label edge)
SHAPES = {'vgg_like': (18, 4, 1), 'unet_like2': (24, 2, 6), 'unet_like_vol': (14, 2, 2)}
_TRAINED = {}


def _batch(name, seed):
    size, batch, out = SHAPES[name]
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((batch, size, size, size, 1)).astype(np.float32)
    hi = 2 if name == 'vgg_like' else 3           # the masked losses see the don't-care class
    y = rng.integers(0, hi, (batch, out, out, out, 1)).astype(np.uint8)
    return x, y


def _trained(name):
    """a network of the factory after two training steps (moving statistics off their initial
    values) and a held-out batch; made once per factory, the tests leave it as it is"""
    if name not in _TRAINED:
        net = FplNetwork(getattr(fplmodels, name))
        net.train(iter([_batch(name, 1), _batch(name, 2)]), 2, 1, None, None)
        _TRAINED[name] = (net, _batch(name, 3))
    return _TRAINED[name]


def _state(net):
    tr = net._trainer[1]
    m, v, steps = tr.get_opt_state()
    arrays = net.train_single.get_weights() + tr.get_weights() + m + v
    return [a.tobytes() for a in arrays], steps, net._train_steps_done


def _means_close(got, sums, cols):
    n = sums[7]
    div = {'loss': n, 'acc': n, 'masked_accuracy': n, 'lb0l1err': max(sums[4], 1), 'lb1l1err': max(sums[6], 1)}
    at = {'loss': 0, 'acc': 1, 'masked_accuracy': 2, 'lb0l1err': 3, 'lb1l1err': 5}
    want = _capi.metrics_from_sums(list(sums))
    assert sorted(got) == sorted(cols)
    for k in cols:
        bound = 0.0 if k in ('acc', 'masked_accuracy') else 1e-12 * max(n, abs(sums[at[k]])) / div[k]
        print(k, got[k], want[k], bound)
        assert abs(got[k] - want[k]) <= bound, (k, got[k], want[k])


@pytest.mark.parametrize('name', list(SHAPES))
def test_evaluate_is_the_specification_on_the_inference_mode_prediction(ctx, name):
    net, (x, y) = _trained(name)
    before = _state(net)
    got = net.evaluate((x, y))
    pred = _capi.Program(ctx, net.train_single).forward(x)
    ref = cnn_oracle.graph_forward(net.train_single, x)
    assert pred.shape == ref.shape == y.shape
    assert np.max(np.abs(pred - ref)) < TOL
    loss, cols = net.compile_args['loss'], None
    loss = getattr(loss, '__name__', loss)
    cols = {'vgg_like': ['acc', 'loss'], 'unet_like2': ['lb0l1err', 'lb1l1err', 'loss', 'masked_accuracy'],
            'unet_like_vol': ['loss', 'masked_accuracy']}[name]
    _means_close(got, valid.loss_sums_numpy(pred, y, loss), cols)
    # device tensors are taken as they are, and a generator of one batch is the same pass
    import torch
    xd, yd = torch.from_numpy(x).to('cuda:0'), torch.from_numpy(y).to('cuda:0')
    assert net.evaluate((xd, yd)) == got and net.evaluate(iter([(x, y)]), steps=1) == got
    # two batches: the sums are accumulated, not the means
    x2, y2 = _batch(name, 4)
    pred2 = _capi.Program(ctx, net.train_single).forward(x2)
    both = valid.loss_sums_numpy(np.concatenate([pred, pred2]), np.concatenate([y, y2]), loss)
    _means_close(net.evaluate(iter([(x, y), (x2, y2)]), steps=2), both, cols)
    # nothing in the network has changed
    after = _state(net)
    assert after[0] == before[0] and after[1:] == before[1:]


def test_evaluate_refuses(ctx):
    net, (x, y) = _trained('vgg_like')
    with pytest.raises(ValueError, match='evaluate: a generator needs steps'):
        net.evaluate(iter([(x, y)]))
    with pytest.raises(ValueError, match="precision 'f16' is not available"):
        net.evaluate((x, y), precision='f16')
    with pytest.raises(ValueError, match=r'labels \(3, 1, 1, 1, 1\) for predictions \(4, 1, 1, 1, 1\)'):
        net.evaluate((x, y[:3]))
    import torch
    with pytest.raises(TypeError, match='contiguous float32 data / uint8 labels'):
        net.evaluate((torch.from_numpy(x).to('cuda:0').double(), torch.from_numpy(y).to('cuda:0')))
    with pytest.raises(TypeError, match="must live on the evaluator's GPU"):
        net.evaluate((torch.from_numpy(x).to('cuda:0'), torch.from_numpy(y)))


def _gen(name, seed):
    rng = np.random.default_rng(seed)
    while True:
        yield _batch(name, int(rng.integers(1 << 30)))


@pytest.mark.parametrize('name', ['vgg_like', 'unet_like2'])
def test_train_logs_val_columns(ctx, tmp_path, name):
    x, y = _batch(name, 3)
    net = FplNetwork(getattr(fplmodels, name))
    log = str(tmp_path / 'val.csv')
    net.train(_gen(name, 7), 2, 2, log, None, validation_data=(x, y))
    rows = [ln.split(',') for ln in open(log).read().strip().splitlines()]
    cols = sorted(set(rows[0][1:]) - {c for c in rows[0] if c.startswith('val_')})
    assert rows[0] == ['epoch'] + sorted(cols + ['val_' + c for c in cols]) and len(rows) == 3
    assert 'val_loss' in rows[0] and rows[0][1:1 + len(cols)] == cols
    # same path, same weights: the last row's val_ values are evaluate's, exactly
    got = net.evaluate((x, y))
    for c in cols:
        assert float(rows[2][rows[0].index('val_' + c)]) == got[c], c
    # the two epochs were evaluated on different weights
    assert rows[1][rows[0].index('val_loss')] != rows[2][rows[0].index('val_loss')]


def test_history_rows_carry_the_val_values(ctx, tmp_path):
    from flypylib_amd import train
    x, y = _batch('vgg_like', 3)
    net = FplNetwork(fplmodels.vgg_like)
    log = str(tmp_path / 'h.csv')
    hist = train.fit_generator(net, _gen('vgg_like', 7), 2, 2, log, None, validation_data=(x, y),
                               validation_steps=1)
    rows = [ln.split(',') for ln in open(log).read().strip().splitlines()]
    assert rows[0] == ['epoch', 'acc', 'loss', 'val_acc', 'val_loss']
    assert [[float(v) for v in r] for r in rows[1:]] == [list(map(float, h)) for h in hist]


def test_without_validation_the_log_is_what_it_was(ctx, tmp_path):
    """validation_data=None and no keyword at all: the same header, and from the same seed the
    same bytes.  One step of vgg_like on 4 patches: its logged loss and accuracy are read from
    one block's sums of the step's forward pass.  Later steps depend on the float atomics of the
    weight gradients, whose order no seed fixes, so two runs of them need not agree bit for bit
    with or without the keyword."""
    logs = []
    for tag, kw in (('plain', {}), ('none', {'validation_data': None, 'validation_steps': None})):
        net = FplNetwork(fplmodels.vgg_like)
        log = str(tmp_path / (tag + '.csv'))
        net.train(_gen('vgg_like', 7), 1, 1, log, None, **kw)
        logs.append(open(log, 'rb').read())
        print(tag, logs[-1])
    assert logs[0] == logs[1] and logs[0].startswith(b'epoch,acc,loss\r\n0,')
    # ... and over two epochs of two steps the same shape of file
    net = FplNetwork(fplmodels.vgg_like)
    log = str(tmp_path / 'none22.csv')
    net.train(_gen('vgg_like', 7), 2, 2, log, None, validation_data=None)
    rows = open(log).read().strip().splitlines()
    assert rows[0] == 'epoch,acc,loss' and [len(r.split(',')) for r in rows] == [3, 3, 3]


def test_the_training_generator_is_refused_as_validation_data(ctx):
    net = FplNetwork(fplmodels.vgg_like)
    gen = _gen('vgg_like', 7)
    with pytest.raises(ValueError, match='validation_data is the training generator itself'):
        net.train(gen, 1, 1, None, None, validation_data=gen, validation_steps=1)
    assert next(gen)[0].shape == (4, 18, 18, 18, 1)             # untouched, not left executing


def test_a_device_generator_validates(ctx, tmp_path):
    """gen_volume2(device=0) with its default ring of 6 as validation_data of unet_like2: every
    validation batch is consumed before the next is drawn"""
    shape = (40, 40, 40)
    rng = np.random.RandomState(0)
    img = rng.randn(*shape).astype(np.float32)
    lab = np.zeros(shape, np.uint8)
    lab[16:24, 16:24, 16:24] = 1
    mask = np.ones(shape, np.uint8)
    mask[:, :, 30:] = 0
    val = fplobjdetect.gen_volume2([(img, lab, mask)], (24, 24, 24), 2, 0.5, rng=np.random.RandomState(2),
                                   device=0, ring=6)
    assert val.ring == 6
    net = FplNetwork(fplmodels.unet_like2)
    log = str(tmp_path / 'dev.csv')
    net.train(_gen('unet_like2', 5), 2, 2, log, None, validation_data=val, validation_steps=3)
    rows = [ln.split(',') for ln in open(log).read().strip().splitlines()]
    assert rows[0][5:] == ['val_lb0l1err', 'val_lb1l1err', 'val_loss', 'val_masked_accuracy'] and len(rows) == 3
    assert all(np.isfinite(float(v)) for r in rows[1:] for v in r)
    # the same generator, evaluated directly: 3 more batches
    got = net.evaluate(val, steps=3)
    assert sorted(got) == ['lb0l1err', 'lb1l1err', 'loss', 'masked_accuracy'] and got['loss'] > 0
