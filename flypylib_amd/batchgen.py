"""Training batches as plan + execute (the device mode of fplobjdetect.gen_batches,
gen_volume and gen_volume2).

A *planner* makes exactly the `rng` calls of its host generator, in the same order, and
emits per batch a record array (`_batchcapi.RECORD`), one row per example: volume index,
centre, rot 0..3, the flips that apply and the intensity-noise multiplier / offset.  What
is common to a whole stream (context size, label mode, whether noise applies, the image
dtype) is on the planner.  A plan is executed either by `execute_numpy` (the CPU tests'
and the oracle's executor: it reproduces the host generator bit for bit) or by
`DeviceBatches`, which keeps the volumes resident on one GPU and cuts a batch with one
launch of libfplbatch.so's gather kernel (include/fplbatch.h).

The host generators in fplobjdetect.py are the specification and stay as they are.
"""
import time

import numpy as np

from . import _batchcapi, _device, fplobjdetect, fplutils

RECORD = _batchcapi.RECORD
_FLIP0, _FLIP1, _FLIP2 = (_batchcapi.FLIP_AXIS0, _batchcapi.FLIP_AXIS1,
                          _batchcapi.FLIP_AXIS2)


def _context(context_sz, host_name):
    context_sz = tuple(int(c) for c in fplutils.to3d(context_sz))
    half = tuple(int(round(cc / 2)) for cc in context_sz)
    if any(2 * h != c for h, c in zip(half, context_sz)):
        raise ValueError('context_sz %r: a planned batch needs even sizes (use the host '
                         'generator %s)' % (context_sz, host_name))
    return context_sz, half


class _Planner:
    """base of the three planners: `records()` draws the next batch's records"""
    host_name = None
    second_flip = _FLIP2          # the flip between the rotation and the flip of axis 0
    noise = False
    label6 = True

    def __init__(self, context_sz, batch_sz, rng):
        self.rng = np.random if rng is None else rng
        self.context_sz, self.half = _context(context_sz, self.host_name)
        self.batch_sz = int(batch_sz)
        self.images, self.labels = [], []     # per volume; labels as the executor reads them
        self._it = None

    def records(self):
        if self._it is None:
            self._it = self._draw()
        return next(self._it)

    def _augment(self, rec):
        """the three rand(B) draws every generator ends a batch with"""
        B = self.batch_sz
        rot = np.floor(4 * self.rng.rand(B))
        ref = np.floor(2 * self.rng.rand(B))
        fpz = np.floor(2 * self.rng.rand(B))
        rec['rot'] = rot.astype(np.uint8)
        rec['flips'] = (ref.astype(np.uint8) * self.second_flip
                        + fpz.astype(np.uint8) * _FLIP0)

    def _new_records(self):
        rec = np.zeros(self.batch_sz, RECORD)
        rec['mul'] = 1.0
        return rec


class BatchesPlanner(_Planner):
    """plan of fplobjdetect.gen_batches"""
    host_name = 'fplobjdetect.gen_batches(device=None)'

    def __init__(self, train_data, context_sz, batch_sz, is_mask=False, rng=None):
        super().__init__(context_sz, batch_sz, rng)
        self.label6 = bool(is_mask)
        self.n_per_class = int(round(self.batch_sz / 2))
        if 2 * self.n_per_class != self.batch_sz:
            raise ValueError('batch_sz %d: a planned gen_batches batch is two classes of equal '
                             'size (use the host generator %s)' % (self.batch_sz, self.host_name))
        half = self.half
        self.centres = []
        for vi, (im, ll, mm) in enumerate(fplobjdetect._batches_volumes(train_data, half)):
            im = np.asarray(im)
            cen = [tuple(np.asarray(a, np.int32) for a in ((ll == cc) & (mm == 1)).nonzero())
                   for cc in range(2)]
            for cc in range(2):
                if len(cen[cc][0]) == 0:
                    # the host generator keeps the previous batch's already-augmented rows
                    # and augments them again: not a plan of independent examples
                    raise ValueError(
                        'volume %d has no unmasked voxel of class %d: a planned / device '
                        'gen_batches needs both classes in every volume (the host generator '
                        '%s re-augments the previous rows instead)' % (vi, cc, self.host_name))
            if is_mask:
                ll[mm == 0] = 2
            self.images.append(im)
            self.labels.append(ll)
            self.centres.append(cen)

    def _draw(self):
        vi, n = 0, self.n_per_class
        while True:
            rec = self._new_records()
            rec['vol'] = vi
            for cc in range(2):
                cen = self.centres[vi][cc]
                pick = self.rng.choice(len(cen[0]), n, True)
                for name, col in zip('zyx', cen):
                    rec[name][cc::2] = col[pick]
            self._augment(rec)
            yield rec
            vi = (vi + 1) % len(self.images)


def _masked_labels(ll, mm):
    ll = ll.copy()
    ll[mm == 0] = 2
    return ll


class VolumePlanner(_Planner):
    """plan of fplobjdetect.gen_volume.  Its rng calls depend on each other example by
    example (uniform, then a choice whose range depends on the class drawn), so those
    stay a loop; the records are built from their results with numpy."""
    host_name = 'fplobjdetect.gen_volume(device=None)'

    def __init__(self, train_data, context_sz, batch_sz, ratio, rng=None):
        super().__init__(context_sz, batch_sz, rng)
        self.ratio = ratio
        counts, cols = [], [[], [], []]
        for im, ll, mm, _ in fplobjdetect._volumes(train_data, self.half):
            for cc in range(2):
                idx = ((ll == cc) & (mm == 1)).nonzero()
                counts.append(len(idx[0]))
                for a in range(3):
                    cols[a].append(idx[a].astype(np.int32))
            self.images.append(im)
            self.labels.append(_masked_labels(ll, mm))
        self._counts = np.array(counts, np.int64).reshape(-1, 2)
        self._offsets = (np.cumsum(counts) - counts).reshape(-1, 2)
        self._zyx = [np.concatenate(c) for c in cols]

    def _draw(self):
        B, nv, rng = self.batch_sz, len(self.images), self.rng
        train_idx = 0
        counts = self._counts.tolist()
        while True:
            rec = self._new_records()
            vol = (train_idx + np.arange(B)) % nv
            cls = np.empty(B, np.int64)
            ks = np.empty(B, np.int64)
            for ex in range(B):
                vi = (train_idx + ex) % nv
                cc = 0 if rng.uniform(0, 1) < self.ratio else 1
                if counts[vi][cc] == 0:
                    cc = 0
                ks[ex] = rng.choice(counts[vi][cc], B, True)[ex]
                cls[ex] = cc
            train_idx = (train_idx + B) % nv
            flat = self._offsets[vol, cls] + ks
            rec['vol'] = vol
            for name, col in zip('zyx', self._zyx):
                rec[name] = col[flat]
            self._augment(rec)
            yield rec


class Volume2Planner(_Planner):
    """plan of fplobjdetect.gen_volume2"""
    host_name = 'fplobjdetect.gen_volume2(device=None)'
    second_flip = _FLIP1          # np.fliplr
    noise = True                  # the host always computes m * v + a, also for [0, 0]

    def __init__(self, train_data, context_sz, batch_sz, ratio, noise_aug=(0, 0), rng=None,
                 tables=None, device=None):
        """tables=None: the candidate tables come from numpy's nonzero(), as in the host
        generator.  tables='device': from libfplmine.so's compaction on GPU `device` -
        labels, mask and weights are uploaded once (resident tensors are kept), only the
        compacted rows come back, and `images` / `labels` of the plan are left resident for
        DeviceBatches.  A callable `tables(labels, mask, half, cc, weights) -> (z, y, x, w)`
        (mine.candidates_numpy) is used in place of nonzero() on the host volumes."""
        super().__init__(context_sz, batch_sz, rng)
        self.ratio, self.noise_aug = ratio, noise_aug
        if tables == 'device':
            vols, rows = self._device_volumes(train_data, device)
        elif tables is None or callable(tables):
            vols = fplobjdetect._volumes(train_data, self.half)
            rows = tables
        else:
            raise ValueError("tables=%r: None, 'device' or a callable" % (tables,))
        weighted = vols[0][3] is not None
        self._p, cols_all, self._n = [], [[], [], [], []], []
        for cc in range(2):
            cols = [[], [], [], [], []]
            for vi, (im, ll, mm, ww) in enumerate(vols):
                if rows is None:
                    sel = (ll == cc) & (mm == 1)
                    if weighted:
                        sel &= ww > 0
                    idx = sel.nonzero()
                    w = ww[idx] if weighted else None
                else:
                    if weighted and ww is None:
                        raise ValueError('volume %d has no weights, volume 0 has' % vi)
                    *idx, w = rows(ll, mm, self.half, cc, ww if weighted else None)
                cols[0].append(np.full(idx[0].shape, vi, np.int32))
                for a in range(3):
                    cols[1 + a].append(idx[a].astype(np.int32))
                if weighted:
                    cols[4].append(w.astype(np.float64))
            cols = [np.concatenate(c) if c else None for c in cols]
            if weighted:
                cols[4] = cols[4] / np.sum(cols[4].astype('float32'))
            self._p.append(cols[4] if weighted else None)
            self._n.append(len(cols[0]))
            for a in range(4):
                cols_all[a].append(cols[a])
        self._cols = [np.concatenate(c) for c in cols_all]     # class 0 rows, then class 1
        for im, ll, mm, ww in vols:
            self.images.append(im)
            self.labels.append(self._masked(ll, mm) if tables == 'device'
                               else _masked_labels(ll, mm))

    def _device_volumes(self, train_data, device):
        """(image, labels, mask, weights) per volume with labels, mask and weights resident
        (uint8 / uint8 / float32 tensors) and the compaction that reads them.  The mask is
        left as it is: the kernels and `_masked` apply the `half` border themselves."""
        from . import mine
        if device is None:
            raise ValueError("tables='device' needs the GPU to build them on (device=...)")
        dev = mine.torch_device(device)
        vols = []
        for tr in train_data:
            if isinstance(tr[1], str) and not tr[1].endswith('.npy'):
                tr = [tr[0], '%slabels.h5' % tr[1], '%smask.h5' % tr[1]] + list(tr[2:])
            im, ll, mm, ww = (a if a is None or _device.is_device_tensor(a)
                              else fplobjdetect._load_main(a)
                              for a in (list(tr[:4]) + [None])[:4])
            vols.append((im, mine.to_device_u8(ll, dev), mine.to_device_u8(mm, dev),
                         None if ww is None else mine.to_device_f32(ww, dev)))
        self._dev = dev
        return vols, mine.candidates_device

    def _masked(self, ll, mm):
        """_masked_labels on resident tensors: 2 where the mask, cleared inside the `half`
        border as `_volumes` clears it, is 0"""
        import torch
        keep = torch.zeros_like(mm, dtype=torch.bool)
        h, d = self.half, mm.shape
        keep[h[0]:d[0] - h[0], h[1]:d[1] - h[1], h[2]:d[2] - h[2]] = True
        return torch.where(keep & (mm != 0), ll, torch.full_like(ll, 2))

    def _draw(self):
        B, rng = self.batch_sz, self.rng
        outer_batches = 100
        outer_batch_sz = outer_batches * B
        n_neg = int(round(self.ratio * outer_batch_sz))
        n_pos = outer_batch_sz - n_neg
        while True:
            neg_idx = rng.choice(self._n[0], n_neg, True, self._p[0])
            pos_idx = rng.choice(self._n[1], n_pos, True, self._p[1])
            all_idx = rng.permutation(outer_batch_sz)
            # row of the concatenated position table per sample of the round
            table = np.concatenate([np.asarray(neg_idx, np.int64),
                                    self._n[0] + np.asarray(pos_idx, np.int64)])
            for ob in range(outer_batches):
                rec = self._new_records()
                flat = table[all_idx[ob * B:(ob + 1) * B]]
                for name, col in zip(('vol', 'z', 'y', 'x'), self._cols):
                    rec[name] = col[flat]
                # per example: the multiplicative draw, then the additive one
                z = np.asarray(rng.randn(2 * B), np.float64)
                rec['mul'] = (self.noise_aug[1] * z[0::2]) + 1.
                rec['add'] = self.noise_aug[0] * z[1::2]
                self._augment(rec)
                yield rec


def _transform(v, rot, flips):
    if rot:
        v = np.rot90(v, int(rot), (1, 2))
    if flips & _FLIP1:
        v = np.flip(v, 1)
    if flips & _FLIP2:
        v = np.flip(v, 2)
    if flips & _FLIP0:
        v = np.flip(v, 0)
    return v


def execute_numpy(plan, rec):
    """(data (B,s0,s1,s2,1) float32, labels (B,6,6,6,1) or (B,1,1,1,1) uint8) of one
    batch's records: the host generators' own numpy operations, example by example"""
    B = len(rec)
    h = plan.half
    data = np.zeros((B,) + plan.context_sz + (1,), np.float32)
    labels = np.zeros((B, 6, 6, 6, 1) if plan.label6 else (B, 1, 1, 1, 1), np.uint8)
    for ex in range(B):
        r = rec[ex]
        z, y, x = int(r['z']), int(r['y']), int(r['x'])
        im, ll = plan.images[int(r['vol'])], plan.labels[int(r['vol'])]
        patch = im[z - h[0]:z + h[0], y - h[1]:y + h[1], x - h[2]:x + h[2]]
        if plan.noise:
            # Python floats, as on the host: float32 arithmetic for a float32 image,
            # float64 with one rounding on assignment for an integer one
            data[ex, :, :, :, 0] = (float(r['mul']) * patch) + float(r['add'])
        else:
            data[ex, :, :, :, 0] = patch
        data[ex, :, :, :, 0] = _transform(data[ex, :, :, :, 0], r['rot'], int(r['flips']))
        if plan.label6:
            labels[ex, :, :, :, 0] = ll[z - 3:z + 3, y - 3:y + 3, x - 3:x + 3]
            labels[ex, :, :, :, 0] = _transform(labels[ex, :, :, :, 0], r['rot'],
                                                int(r['flips']))
        else:
            labels[ex, 0] = ll[z, y, x]
    return data, labels


def planned_batches(plan):
    """host generator over a plan (plan + numpy executor)"""
    while True:
        yield execute_numpy(plan, plan.records())


def _np_dtype(a):
    """numpy dtype of an array or a torch tensor"""
    if isinstance(a, np.ndarray):
        return a.dtype
    if hasattr(a, 'is_cuda'):
        return np.dtype(str(a.dtype).replace('torch.', ''))
    return np.asarray(a).dtype


def _is_resident(a, dev):
    return hasattr(a, 'is_cuda') and bool(a.is_cuda) and a.device == dev


def volume2_tables(train_data, tables):
    """the `tables` argument gen_volume2's device mode hands its planner: 'device' when asked
    for, or when labels, mask or weights of an entry are torch CUDA tensors"""
    if tables is not None:
        return tables
    for tr in train_data:
        if any(hasattr(a, 'is_cuda') and a.is_cuda for a in tr[1:4]):
            return 'device'
    return None


def check_image_dtypes(plan):
    """device mode keeps float32 and uint8 images in their own dtype; anything else is refused"""
    kinds = {np.dtype(_np_dtype(im)) for im in plan.images}
    for k in kinds:
        if k not in (np.dtype(np.float32), np.dtype(np.uint8)):
            raise ValueError('device batches take float32 or uint8 images, not %s (use the '
                             'host generator %s)' % (k, plan.host_name))
    if len(kinds) != 1:
        raise ValueError('device batches need every image volume in one dtype, got %s (use '
                         'the host generator %s)' % (sorted(str(k) for k in kinds), plan.host_name))
    return _batchcapi.F32 if kinds.pop() == np.dtype(np.float32) else _batchcapi.U8


class DeviceBatches:
    """Iterator of (data, labels) torch CUDA tensors cut on the GPU from resident volumes.

    Lifetime of a yielded batch: the tensors are one of `ring` buffer pairs, handed out
    in turn, so a batch is valid until `ring - 1` further batches have been drawn; the
    draw after that overwrites it.  Copy (`.clone()`, `.cpu()`) what must live longer.

    Each `next()` plans on the host, uploads the records from a pinned staging buffer with
    one asynchronous copy, launches the gather kernel - both on this generator's own side
    stream - and synchronises that stream, so the tensors are complete when returned and
    may be read from any stream.
    """

    def __init__(self, plan, device, ring=6):
        self.plan = plan
        src_dtype = check_image_dtypes(plan)
        cs = plan.context_sz
        if cs[1] != cs[2]:
            raise ValueError('context_sz %r: the rotation in axes (1, 2) needs s1 == s2' % (cs,))
        if plan.label6 and min(plan.half) < 3:
            raise ValueError('context_sz %r: the 6^3 label block needs a context of at least 6' % (cs,))
        ring = int(ring)
        if ring < 2:
            raise ValueError('ring=%d: at least 2 buffer pairs' % ring)
        torch = _device.require_torch('device batches need', 'use device=None for the host '
                                      'generator %s' % plan.host_name)
        # FplBatchError if the library is not built
        self._dev = dev = _device.torch_device(device, 'device batches', _batchcapi.load_library)
        self._torch, self.ring, self.device = torch, ring, dev.index
        self._src_dtype = src_dtype
        want = np.float32 if src_dtype == _batchcapi.F32 else np.uint8
        # what a planner left resident on this device is not uploaded a second time
        self._images = [im.contiguous() if _is_resident(im, dev)
                        else torch.from_numpy(np.ascontiguousarray(im, want)).to(dev)
                        for im in plan.images]
        self._labels = [ll.contiguous() if _is_resident(ll, dev)
                        else torch.from_numpy(np.ascontiguousarray(ll).astype(np.uint8)).to(dev)
                        for ll in plan.labels]
        table = np.zeros(len(self._images), _batchcapi.VOLUME)
        for i, (im, ll) in enumerate(zip(self._images, self._labels)):
            if tuple(im.shape) != tuple(ll.shape) or im.dim() != 3:
                raise ValueError('volume %d: image %s and labels %s must be 3-D and equal in shape'
                                 % (i, tuple(im.shape), tuple(ll.shape)))
            table[i] = (im.data_ptr(), ll.data_ptr()) + tuple(im.shape) + (src_dtype,)
        self._dims = np.array([im.shape for im in self._images], np.int64)
        self._table = torch.from_numpy(table.view(np.uint8)).to(dev)
        B = plan.batch_sz
        self._rec_host = torch.empty(B * RECORD.itemsize, dtype=torch.uint8).pin_memory()
        self._rec_view = self._rec_host.numpy().view(RECORD)
        self._rec_dev = torch.empty(B * RECORD.itemsize, dtype=torch.uint8, device=dev)
        lshape = (B, 6, 6, 6, 1) if plan.label6 else (B, 1, 1, 1, 1)
        self._ring = [(torch.empty((B,) + cs + (1,), dtype=torch.float32, device=dev),
                       torch.empty(lshape, dtype=torch.uint8, device=dev))
                      for _ in range(ring)]
        self._slot = 0
        self._stream = torch.cuda.Stream(dev)
        self._reach = np.maximum(np.array(plan.half), 3 if plan.label6 else 0)
        # measurements (tools/bench_configs.py --what train_gen)
        self.time_kernel = False
        self.batches = 0
        self.plan_seconds = 0.0
        self.kernel_ms = []
        self.last_records = None
        torch.cuda.synchronize(dev)

    def _validate(self, rec):
        """the kernel skips a record whose patch leaves its volume; say so here instead"""
        vol = rec['vol']
        ok = (vol >= 0) & (vol < len(self._dims))
        if ok.all():
            c = np.stack([rec['z'], rec['y'], rec['x']], 1).astype(np.int64)
            d = self._dims[vol]
            ok = ((c - self._reach >= 0) & (c + self._reach <= d)).all(1) & (rec['rot'] < 4)
        if not ok.all():
            raise ValueError('planned records leave their volumes: %r' % (rec[~ok][:4],))

    def __iter__(self):
        return self

    def __next__(self):
        torch = self._torch
        t0 = time.perf_counter()
        rec = self.plan.records()
        self._validate(rec)
        self.plan_seconds += time.perf_counter() - t0
        self.last_records = rec
        data, labels = self._ring[self._slot]
        self._slot = (self._slot + 1) % self.ring
        self._rec_view[:] = rec
        with torch.cuda.device(self._dev), torch.cuda.stream(self._stream):
            self._rec_dev.copy_(self._rec_host, non_blocking=True)
            if self.time_kernel:
                e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                e0.record(self._stream)
            _batchcapi.gather(self._table.data_ptr(), len(self._images), self._rec_dev.data_ptr(),
                              self.plan.batch_sz, self.plan.context_sz, self._src_dtype,
                              self.plan.noise,
                              _batchcapi.LABELS_6 if self.plan.label6 else _batchcapi.LABELS_CENTRE,
                              data.data_ptr(), labels.data_ptr(), self._stream.cuda_stream)
            if self.time_kernel:
                e1.record(self._stream)
        self._stream.synchronize()
        if self.time_kernel:
            self.kernel_ms.append(e0.elapsed_time(e1))
        self.batches += 1
        return data, labels


def device_generator(kind, device, ring, *args, **kw):
    """the device mode of gen_batches / gen_volume / gen_volume2: raises at construction
    (ValueError for input the device mode refuses, RuntimeError / FplBatchError without
    torch, a GPU or the library) - there is no silent host fallback"""
    planner = {'batches': BatchesPlanner, 'volume': VolumePlanner,
               'volume2': Volume2Planner}[kind]
    if kw.get('tables') == 'device':         # gen_volume2: the tables are built on that GPU too
        kw['device'] = device
    return DeviceBatches(planner(*args, **kw), device, ring)
