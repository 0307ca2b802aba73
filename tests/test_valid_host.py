"""CPU: held-out validation as far as it can be checked without a GPU - the float64
specification of the eight sums (valid.loss_sums_numpy) against the oracle's losses and metrics,
its edge values, the constants of libfplval.so's C ABI, what fplv_loss_sums and
the Python surface refuse, and the CSV header logic of fit_generator."""
import math
import os
import re

import numpy as np
import pytest
import torch

from flypylib_amd import FplNetwork, _capi, _validcapi, fplmodels, train, valid
from flypylib_amd.csrc import build
from oracle import train_oracle
from tests import side_abi_cases as abi

ROOT = abi.ROOT
KINDS = sorted(_capi.LOSS_KINDS, key=_capi.LOSS_KINDS.get)
EDGES = np.array([0.0, 1e-8, 1e-7, 0.5, 1 - 1e-7, 1.0], np.float32)


def _oracle(p32, y8, kind):
    """the oracle's loss and metrics on the float32 predictions, in float64"""
    p = torch.from_numpy(p32.astype(np.float64))
    y = torch.from_numpy(y8.astype(np.float64))
    out = dict(train_oracle.metric_values(p, y))
    out['loss'] = float(train_oracle.loss_value(p, y, kind))
    return out


def _check_against_oracle(p32, y8, kind):
    s = valid.loss_sums_numpy(p32, y8, kind)
    assert s.dtype == np.float64 and s.shape == (8,) and s[7] == p32.size
    got, want = _capi.metrics_from_sums(list(s)), _oracle(p32, y8, kind)
    for k in ('loss', 'acc', 'masked_accuracy', 'lb0l1err'):
        assert abs(got[k] - want[k]) <= 1e-12 * max(1.0, abs(want[k])), (kind, k, got[k], want[k])
    # 1 - p is a float32 subtraction here (as in the training kernel), float64 in the oracle:
    # half an ulp of 1 per element
    assert abs(got['lb1l1err'] - want['lb1l1err']) <= 2.0 ** -24, (kind, got, want)
    return s


@pytest.mark.parametrize('kind', KINDS)
def test_the_numpy_sums_are_the_oracles_losses_and_metrics(kind):
    rng = np.random.default_rng(3)
    p = rng.random(1501).astype(np.float32)
    y = rng.integers(0, 3, 1501).astype(np.uint8)
    s = _check_against_oracle(p, y, kind)
    assert s[4] == np.count_nonzero(y == 0) and s[6] == np.count_nonzero(y == 1)
    # by name, by value and by function
    assert np.array_equal(s, valid.loss_sums_numpy(p.reshape(19, 79), y.reshape(19, 79),
                                                   _capi.LOSS_KINDS[kind]))
    assert np.array_equal(s, valid.loss_sums_numpy(p, y, getattr(fplmodels, kind, kind)))


@pytest.mark.parametrize('kind', KINDS)
def test_edge_values(kind):
    """0, 1e-8, 1e-7, 0.5, 1 - 1e-7 and 1 under every label: the clip, rint(0.5) == 0, and
    the divisors of max(., 1) when a class is absent"""
    p = np.repeat(EDGES, 3)
    y = np.tile(np.array([0, 1, 2], np.uint8), len(EDGES))
    s = _check_against_oracle(p, y, kind)
    assert np.isfinite(s).all()
    # rintf: 0.5 rounds to 0, 1 - 1e-7 (the float32 below 1) to 1
    assert s[1] == 4 + 2                        # label 0 at 0, 1e-8, 1e-7, 0.5; label 1 at 1-1e-7, 1
    assert s[2] == 6 + len(EDGES)               # ... and every masked voxel (0 == 0)
    # labels all 2: the counts are zero and the means divide by 1
    y2 = np.full(len(EDGES), 2, np.uint8)
    s2 = _check_against_oracle(EDGES, y2, kind)
    assert s2[3] == s2[4] == s2[5] == s2[6] == 0 and s2[2] == len(EDGES)
    m2 = _capi.metrics_from_sums(list(s2))
    assert m2['lb0l1err'] == 0 and m2['lb1l1err'] == 0 and m2['masked_accuracy'] == 1
    if kind == 'masked_focal_loss':
        assert s2[0] == 0
    elif kind != 'binary_crossentropy':
        # every masked voxel costs -log(1 - 1e-7); the weighted form cancels two terms of 16.1
        assert abs(s2[0] - len(EDGES) * -math.log1p(-1e-7)) < 1e-13
    # no label 1
    _check_against_oracle(p, np.where(y == 1, 0, y).astype(np.uint8), kind)


def test_known_values():
    s = valid.loss_sums_numpy([0.5], [1], 'binary_crossentropy')
    assert abs(s[0] - math.log(2)) < 1e-15 and list(s[1:]) == [0, 0, 0, 0, 0.5, 1, 1]
    s = valid.loss_sums_numpy([0.25, 0.75], [0, 1], 'masked_focal_loss')
    assert abs(s[0] - 2 * -(0.25 ** 2) * math.log(0.75 + 1e-7)) < 1e-15
    assert list(s[1:]) == [2, 2, 0.25, 1, 0.25, 1, 2]
    with pytest.raises(ValueError, match='3 predictions, 2 labels'):
        valid.loss_sums_numpy([0.1, 0.2, 0.3], [0, 1], 0)
    with pytest.raises(NotImplementedError, match='hinge'):
        valid.loss_sums_numpy([0.1], [0], 'hinge')
    with pytest.raises(NotImplementedError):
        valid.loss_kind(4)


# ---- the build and the C ABI -----------------------------------------------------------------------

def test_the_library_loads_and_the_constants_are_the_headers():
    assert _validcapi.load_library().fplv_abi_version() == _validcapi.ABI_VERSION
    hdr = open(os.path.join(ROOT, 'include', 'fplval.h')).read()
    for name in ('ABI_VERSION', 'BLOCK', 'ELEMS_PER_THREAD', 'MAX_BLOCKS', 'N_SUMS', 'SCRATCH_BYTES'):
        assert int(re.search(r'#define FPLV_%s (\d+)' % name, hdr).group(1)) == getattr(_validcapi, name), name
    assert _validcapi.SCRATCH_BYTES == _validcapi.MAX_BLOCKS * 7 * 8
    for name, value in _capi.LOSS_KINDS.items():           # the loss table is _capi's
        assert re.search(r'FPLV_LOSS_\w+ = %d' % value, hdr), name
    main = open(os.path.join(ROOT, 'include', 'fplhip.h')).read()
    for short in ('BCE', 'MASKED_BCE', 'MASKED_WEIGHTED_BCE', 'MASKED_FOCAL'):
        a = re.search(r'FPL_LOSS_%s = (\d+)' % short, main).group(1)
        assert a == re.search(r'FPLV_LOSS_%s = (\d+)' % short, hdr).group(1), short


def test_arguments_are_refused_before_the_gpu_is_touched():
    """every refusal here returns before a launch (and before a pointer is looked at): no GPU is
    needed to see it"""
    err = _validcapi.FplValidError
    ok = dict(pred=4096, labels=4096, n=10, loss_kind=0, accumulate=0, sums=8192, scratch=8192,
              scratch_bytes=_validcapi.SCRATCH_BYTES)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return _validcapi.loss_sums(*a.values(), None)
    for bad in (0, -1, 2 ** 31):
        with pytest.raises(err, match=r'fplv_loss_sums: n -?\d+ must lie in \[1, 2\^31 - 1\]'):
            call(n=bad)
    for bad in (-1, 4):
        with pytest.raises(err, match='fplv_loss_sums: unknown loss_kind %d' % bad):
            call(loss_kind=bad)
    for name in ('pred', 'labels', 'sums', 'scratch'):
        with pytest.raises(err, match='fplv_loss_sums: null pointer argument'):
            call(**{name: 0})
    with pytest.raises(err, match='scratch of 57343 bytes, FPLV_SCRATCH_BYTES is 57344'):
        call(scratch_bytes=_validcapi.SCRATCH_BYTES - 1)
    with pytest.raises(err, match='pred is not 4-byte aligned'):
        call(pred=4098)
    for name in ('sums', 'scratch'):
        with pytest.raises(err, match='sums and scratch must be 8-byte aligned'):
            call(**{name: 8196})


def test_the_kernels_do_not_spill_and_use_no_atomics():
    import shutil
    import sys
    src = open(os.path.join(abi.CSRC, 'valid', 'valid.hip')).read()
    assert 'atomic' not in re.sub(r'//.*', '', src).lower()
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    if not shutil.which(build.HIPCC) and not os.path.exists(build.HIPCC):
        pytest.skip('hipcc not available')
    import kernel_resources
    res = kernel_resources.kernel_resources('valid/valid.hip')
    # four loss kinds x (label words, label bytes), and the finishing block
    assert len(res) == 9 and sum('loss_partials' in k for k in res) == 8, sorted(res)
    for name, v in res.items():
        assert v['vgpr_spill_count'] == 0 and v['sgpr_spill_count'] == 0, (name, v)
        assert v['private_segment_fixed_size'] == 0 and v['vgpr_count'] <= 128, (name, v)
        if 'loss_partials' in name:
            assert v['group_segment_fixed_size'] == 7 * (_validcapi.BLOCK // 64) * 8


# ---- the Python surface ----------------------------------------------------------------------------

def test_a_missing_library_is_reported_before_a_missing_gpu(monkeypatch):
    monkeypatch.setattr(_validcapi._side, '_lib', None)
    monkeypatch.setattr(_validcapi._side, 'path', '/nonexistent/libfplval.so')
    p, y = torch.zeros(4), torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(_validcapi.FplValidError, match='libfplval.so not found at /nonexistent') as e:
        valid.loss_sums_device(p, y, 0)
    assert 'python -m flypylib_amd.csrc.build' in str(e.value) and 'no host fallback' in str(e.value)
    net = FplNetwork(fplmodels.vgg_like)
    with pytest.raises(_validcapi.FplValidError, match='libfplval.so not found'):
        net.evaluate((np.zeros((2, 18, 18, 18, 1), np.float32), np.zeros((2, 1, 1, 1, 1), np.uint8)))


def test_loss_sums_device_refuses_by_name():
    p, y = torch.zeros(4), torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(ValueError, match='pred must be a torch tensor, got ndarray'):
        valid.loss_sums_device(np.zeros(4, np.float32), y, 0)
    with pytest.raises(ValueError, match='pred must be torch.float32, got torch.float64'):
        valid.loss_sums_device(p.double(), y, 0)
    with pytest.raises(ValueError, match='labels must be torch.uint8, got torch.int64'):
        valid.loss_sums_device(p, y.long(), 0)
    with pytest.raises(ValueError, match=r'pred must be on a GPU \(there is no host fallback\), got cpu'):
        valid.loss_sums_device(p, y, 0)
    with pytest.raises(NotImplementedError, match='hinge'):
        valid.loss_sums_device(p, y, 'hinge')


def test_batches_of_a_pair_or_a_generator():
    x, y = np.zeros(3), np.ones(3)
    it, steps = valid.as_batches((x, y), None, 'evaluate')
    assert steps == 1 and all(a is x and b is y for a, b in (next(it), next(it), next(it)))
    assert valid.as_batches([x, y], 1, 'evaluate')[1] == 1
    with pytest.raises(ValueError, match=r'evaluate: a \(data, labels\) pair is one batch; steps=3'):
        valid.as_batches((x, y), 3, 'evaluate')
    with pytest.raises(ValueError, match='a fixed batch is a .* pair, got 3 items'):
        valid.as_batches((x, y, x), None, 'evaluate')
    with pytest.raises(ValueError, match='evaluate: a generator needs steps'):
        valid.as_batches(iter([(x, y)]), None, 'evaluate')
    gen = ((x, y) for _ in range(2))
    assert valid.as_batches(gen, 2, 'validation_data') == (gen, 2)


def test_csv_header_logic():
    """CSVLogger's order: 'epoch', then the sorted log keys - 'val_' twins sort after every plain
    column; without validation the header is what it was"""
    loss, cols = train.compile_columns(None)
    assert (loss, cols) == ('binary_crossentropy', ['acc', 'loss'])
    assert train.log_columns(cols, False) == (['epoch', 'acc', 'loss'], ['acc', 'loss'])
    assert train.log_columns(cols, True) == (['epoch', 'acc', 'loss', 'val_acc', 'val_loss'],
                                             ['acc', 'loss', 'val_acc', 'val_loss'])
    loss, cols = train.compile_columns(fplmodels.unet_like2()[3])
    assert loss == 'masked_focal_loss' and cols == ['lb0l1err', 'lb1l1err', 'loss', 'masked_accuracy']
    header, keys = train.log_columns(cols, True)
    assert header == ['epoch'] + keys == ['epoch'] + sorted(cols + ['val_' + c for c in cols])
    assert keys[4:] == ['val_lb0l1err', 'val_lb1l1err', 'val_loss', 'val_masked_accuracy']
    with pytest.raises(NotImplementedError, match="metric 'mae'"):
        train.compile_columns({'metrics': ['mae']})


def test_the_training_generator_is_refused_as_validation_data():
    net = FplNetwork(fplmodels.vgg_like)
    gen = iter([])
    with pytest.raises(ValueError, match='validation_data is the training generator itself'):
        net.train(gen, 1, 1, None, None, validation_data=gen, validation_steps=1)
    with pytest.raises(ValueError, match='validation_data: a generator needs steps'):
        net.train(gen, 1, 1, None, None, validation_data=iter([]))
