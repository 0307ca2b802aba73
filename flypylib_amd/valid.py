"""Held-out validation: the loss and metrics of the network in INFERENCE mode on batches it
does not train on (`FplNetwork.evaluate`, the `val_` columns of `FplNetwork.train`) - what
Keras' `fit_generator(validation_data=..., validation_steps=...)` reports and the reference's
`train` could have had for one keyword.

A validation batch runs through the lowered inference program of the training graph
(`graph.lower_inference()`: BatchNorm on its moving statistics, no Dropout - Keras' learning
phase 0) by `fpl_program_forward`, device to device; `fplv_loss_sums` (libfplval.so) reduces
prediction and labels to the eight sums `_capi.metrics_from_sums` reads, accumulating over the
batches on the device, and one download ends the pass.  `loss_sums_numpy` is the float64
specification of those sums.  No host fallback: without torch, a GPU or libfplval.so the
device functions raise.
"""
import math

import numpy as np

from . import _capi, _device, _validcapi

_F32 = ('f32', 'fp32', 'float32')


def loss_kind(kind):
    """fpl_loss value of a loss given by name, function or value"""
    kind = getattr(kind, '__name__', kind)
    if isinstance(kind, str):
        if kind not in _capi.LOSS_KINDS:
            raise NotImplementedError('loss %r (have %s)' % (kind, sorted(_capi.LOSS_KINDS)))
        return _capi.LOSS_KINDS[kind]
    if int(kind) not in _capi.LOSS_KINDS.values():
        raise NotImplementedError('loss kind %r' % (kind,))
    return int(kind)


def loss_sums_numpy(pred, labels, kind):
    """the eight sums of fplv_loss_sums (include/fplval.h) as float64: the per-element loss of
    csrc/train.hip's loss_grad evaluated in double from the float32 prediction (clip at 1e-7,
    pos_weight 100, mask = y != 2, focal: y < 2), the counts by float32 rint, 1 - p in float32;
    real sums by math.fsum"""
    kind = loss_kind(kind)
    p32 = np.ascontiguousarray(pred, np.float32).reshape(-1)
    y8 = np.ascontiguousarray(labels, np.uint8).reshape(-1)
    if p32.size != y8.size or p32.size < 1:
        raise ValueError('loss_sums_numpy: %d predictions, %d labels' % (p32.size, y8.size))
    p, yl, eps = p32.astype(np.float64), y8.astype(np.int64), 1e-7
    if kind == _capi.LOSS_KINDS['masked_focal_loss']:
        m = (yl < 2).astype(np.float64)
        pt = np.where(yl == 1, p, 1.0 - p)
        loss = -(m * ((1.0 - pt) * (1.0 - pt)) * np.log(pt + eps))
    else:
        mask = np.ones_like(p) if kind == _capi.LOSS_KINDS['binary_crossentropy'] \
            else (yl != 2).astype(np.float64)
        t, pm = yl * mask, p * mask
        pc = np.minimum(np.maximum(pm, eps), 1.0 - eps)
        z = np.log(pc / (1.0 - pc))
        soft = np.log1p(np.exp(-np.abs(z)))
        if kind == _capi.LOSS_KINDS['masked_weighted_binary_crossentropy']:
            loss = (1.0 - t) * z + (1.0 + 99.0 * t) * (soft + np.maximum(-z, 0.0))
        else:
            loss = np.maximum(z, 0.0) - z * t + soft
    yf, mk = y8.astype(np.float32), (y8 != 2).astype(np.float32)
    one_minus = (np.float32(1) - p32).astype(np.float64)
    return np.array([math.fsum(loss),
                     np.count_nonzero(np.rint(p32) == yf),
                     np.count_nonzero(np.rint(p32 * mk) == yf * mk),
                     math.fsum(p[yl == 0]), np.count_nonzero(yl == 0),
                     math.fsum(one_minus[yl == 1]), np.count_nonzero(yl == 1),
                     p32.size], np.float64)


def _check_pair(torch, pred, labels, who):
    pair = (('pred', pred, torch.float32), ('labels', labels, torch.uint8))
    for name, t, dt in pair:
        if not isinstance(t, torch.Tensor):
            raise ValueError('%s: %s must be a torch tensor, got %s' % (who, name, type(t).__name__))
        if t.dtype != dt:
            raise ValueError('%s: %s must be %s, got %s' % (who, name, dt, t.dtype))
    for name, t, dt in pair:
        if not t.is_cuda:
            raise ValueError('%s: %s must be on a GPU (there is no host fallback), got %s'
                             % (who, name, t.device))
        if not t.is_contiguous():
            raise ValueError('%s: %s must be contiguous' % (who, name))
    if labels.device != pred.device:
        raise ValueError('%s: pred is on %s, labels on %s' % (who, pred.device, labels.device))
    if pred.numel() != labels.numel() or pred.numel() < 1:
        raise ValueError('%s: %d predictions, %d labels' % (who, pred.numel(), labels.numel()))


def loss_sums_device(pred, labels, kind, sums=None, accumulate=False, scratch=None):
    """fplv_loss_sums on contiguous float32 predictions / uint8 labels on one GPU.  `sums`: a
    float64 tensor of 8 on that GPU (default: a new one); accumulate=True adds to what it
    holds.  Stream-ordered on torch's current stream; returns `sums`, still on the device."""
    torch = _device.require_torch('loss_sums_device needs', 'there is no host fallback')
    _validcapi.load_library()              # a missing library is reported before a missing GPU
    who = 'loss_sums_device'
    kind = loss_kind(kind)
    _check_pair(torch, pred, labels, who)
    dev = pred.device
    if sums is None:
        sums = torch.zeros(_validcapi.N_SUMS, dtype=torch.float64, device=dev)
    elif not isinstance(sums, torch.Tensor) or sums.dtype != torch.float64 or sums.device != dev \
            or not sums.is_contiguous() or sums.numel() < _validcapi.N_SUMS:
        raise ValueError('%s: sums must be a contiguous float64 tensor of %d on %s'
                         % (who, _validcapi.N_SUMS, dev))
    if scratch is None:
        scratch = torch.empty(_validcapi.SCRATCH_BYTES, dtype=torch.uint8, device=dev)
    elif not isinstance(scratch, torch.Tensor) or scratch.device != dev or not scratch.is_contiguous():
        raise ValueError('%s: scratch must be a contiguous tensor on %s' % (who, dev))
    with torch.cuda.device(dev):
        _validcapi.loss_sums(pred, labels, pred.numel(), kind, accumulate, sums, scratch,
                             scratch.numel() * scratch.element_size(),
                             torch.cuda.current_stream(dev).cuda_stream)
    return sums


class Evaluator:
    """validation passes of one network on one GPU: a stride-(1,1,1) inference program of
    `network.train_single` (the training target is not upsampled, so no rf_stride), a resident
    prediction buffer, the scratch and the 8-double accumulator of fplv_loss_sums.  `device`
    defaults to the network's."""

    def __init__(self, network, device=None):
        from . import runtime, train
        self._torch = torch = _device.require_torch(
            'validation needs', 'train without validation_data instead')
        device = network._device if device is None else device
        self.dev = _device.torch_device(device, 'validation', _validcapi.load_library)
        self.graph = network.train_single
        loss, self.cols = train.compile_columns(network.compile_args)
        self.kind = loss_kind(loss)
        self.ctx = runtime.get_context(self.dev.index)
        self.program = _capi.Program(self.ctx, self.graph, (1, 1, 1))
        self.sums = torch.zeros(_validcapi.N_SUMS, dtype=torch.float64, device=self.dev)
        self.scratch = torch.empty(_validcapi.SCRATCH_BYTES, dtype=torch.uint8, device=self.dev)
        self._pred = None

    def close(self):
        if self.program is not None:
            self.program.close()
        self.program = self._pred = None

    def _batch(self, data, labels):
        """the batch on this GPU: host arrays are uploaded, device tensors taken as they are
        (the checks of Trainer.step)"""
        torch = self._torch
        if isinstance(data, np.ndarray) or not hasattr(data, 'data_ptr'):
            x = torch.from_numpy(np.ascontiguousarray(data, np.float32)).to(self.dev)
            y = torch.from_numpy(np.ascontiguousarray(labels, np.uint8)).to(self.dev)
            return x, y
        x, y = data, labels
        if 'float32' not in str(x.dtype) or 'uint8' not in str(getattr(y, 'dtype', None)) or \
                not x.is_contiguous() or not y.is_contiguous():
            raise TypeError('device batches must be contiguous float32 data / uint8 labels')
        for t in (x, y):            # a raw pointer of another GPU would be a memory fault, not an error
            if not getattr(t, 'is_cuda', False) or t.device != self.dev:
                raise TypeError('device batches must live on the evaluator\'s GPU (%s), got %s'
                                % (self.dev, getattr(t, 'device', type(t))))
        return x, y

    def _pred_buffer(self, shape):
        n = int(np.prod(shape))
        if self._pred is None or self._pred.numel() < n:
            self._pred = self._torch.empty(n, dtype=self._torch.float32, device=self.dev)
        return self._pred[:n].view(shape)

    def run_sums(self, batches, steps, precision='f32'):
        """the eight sums (float64 ndarray) over `steps` batches drawn from the iterator
        `batches`, on the weights `graph` holds now"""
        if precision not in _F32:
            raise ValueError('validation runs the fp32 executor of fpl_program_forward: precision '
                             '%r is not available for patch batches' % (precision,))
        steps = int(steps)
        if steps < 1:
            raise ValueError('validation over %d batches' % steps)
        torch = self._torch
        self.program.set_weights_from(self.graph)
        stream = torch.cuda.current_stream(self.dev)
        for i in range(steps):
            x, y = self._batch(*next(batches))
            shape = tuple(int(v) for v in x.shape)
            if len(shape) == 5:
                shape = shape[:4]                 # trailing channel axis of 1
            out_shape = (shape[0],) + self.program.out_dims(shape[1:])
            if int(np.prod(out_shape)) != y.numel():
                raise ValueError('validation batch %d: labels %s for predictions %s'
                                 % (i, tuple(y.shape), out_shape))
            stream.synchronize()                  # the uploads (and whatever made x, y) are done
            pred = self.program.forward_device(x, self._pred_buffer(out_shape))
            loss_sums_device(pred, y, self.kind, self.sums, i > 0, self.scratch)
            # the batch is consumed before the next one is drawn (a device generator's ring)
            # and before the next forward overwrites the prediction
            stream.synchronize()
        return self.sums.cpu().numpy()

    def run(self, batches, steps, precision='f32'):
        """loss and the reference's metrics over `steps` batches (`_capi.metrics_from_sums`)"""
        return _capi.metrics_from_sums([float(v) for v in self.run_sums(batches, steps, precision)])


def evaluator_of(network, device=None):
    """one evaluator per network, kept like its trainer; rebuilt when the device, the loss or
    the graph's compile generation changes"""
    from . import train
    device = network._device if device is None else device
    graph = network.train_single
    loss, cols = train.compile_columns(network.compile_args)
    key = (int(device), loss, tuple(cols), id(graph), len(graph.weights),
           getattr(graph, 'compile_generation', 0))
    cached = getattr(network, '_evaluator', None)
    if cached is not None and cached[0] == key and cached[1].program is not None \
            and cached[1].program.h is not None and cached[1].ctx.h is not None:
        return cached[1]
    if cached is not None:
        cached[1].close()
    ev = Evaluator(network, device)
    network._evaluator = (key, ev)
    return ev


def as_batches(data, steps, who):
    """(iterator, steps) of `validation_data` / evaluate's argument: a (data, labels) pair is one
    fixed batch, evaluated once per pass; anything else is an iterator and needs `steps`"""
    if isinstance(data, (tuple, list)):
        if len(data) != 2:
            raise ValueError('%s: a fixed batch is a (data, labels) pair, got %d items' % (who, len(data)))
        if steps not in (None, 1):
            raise ValueError('%s: a (data, labels) pair is one batch; steps=%r' % (who, steps))
        pair = (data[0], data[1])
        return iter(lambda: pair, None), 1
    if steps is None:
        raise ValueError('%s: a generator needs steps' % who)
    if not hasattr(data, '__next__'):
        data = iter(data)
    return data, int(steps)
