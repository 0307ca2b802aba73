#!/usr/bin/env python3
"""Secondary measurements for the other BASELINE.json configs (run on the GPU box):

    python tools/bench_configs.py --what unet,train,v2o,pipeline [--out file.json]

  unet      configs[2] unet_like2 inference (reference lattice 100^3, pitch 82) on a
            reduced volume (the fp32 per-op path; size via --unet-size)
  train     configs[3] vgg_like training step, batch 32 of 64^3 patches (1 GPU)
  v2o       voxel2obj on a 582^3 substack-sized probability volume (r=27, sigma=5)
  graphs    baseline_model, resnet_like, unet_like4b, unet_like_vol: 'auto' (graph executor) vs fp32
  roi       configs[4] end to end: fplobjdetect.full_roi_inference over a synthetic
            --roi-size^3 volume (512-substacks + 35 buffer), one substack's points
            diffed against the CPU oracle
  pipeline  configs[4] shape at one substack: vgg_like bf16 inference of a 582^3
            substack + voxel2obj, detections diffed against the CPU oracle on the
            same prediction
  c3share   configs[2] at its stated size: rank 0's slab of the 1024 x 2048 x 2048 volume
            (2 of 13 tile rows + halo), bit-compared with the same rows of a whole-volume run
  c5share   configs[4] at its stated size: rank 0's 64 of the 512 substacks of a 4096^3
            synthetic ROI, one substack diffed against the CPU oracle
  train_gen the training loops fed three ways in one process: (a) the constant batch of
            the `train` / `train_unet` rows, (b) the host generator, (c) the device generator
            (gen_batches(device=...) for vgg_like 32 x 64^3, gen_volume2(device=...) with noise
            for unet_like2 64 x 24^3), through fit_generator's prefetch loop; plus the planner's
            ms per batch and the gather kernel's ms (HIP events), rot 0 and rot 1 separately
  mine      hard-example mining at --mine-size^3 (default 520), all in one process:
            FplNetwork.voxel_loss on the host against device=..., the voxel-loss kernel alone
            (HIP events; GB/s at 10 B/voxel), and gen_volume2's candidate tables built by
            Volume2Planner on the host (nonzero) against tables='device' (libfplmine.so), for
            an unweighted and a mined (weighted) volume; written to profiles/mine.json
  labels    fplsynapses.write_labels_mask on the host against device=..., in one process, at
            520^3 and 256^3, one T-bar per 16^3 voxels (the density of tools/example_flow.py),
            radii 3 / 6 and 6 / 12: the public call from a host roi_mask and from a resident
            one, the planners (plan_tbars + plan_bricks) alone, the kernel alone (HIP events;
            GB/s at 3 B/voxel) and the bytes uploaded; and the same with planner='device':
            fplp_plan_bricks alone (HIP events), the public call from a host and from a
            resident roi_mask, the bytes uploaded; written to profiles/labels.json
  match     obj_pr_curve's matching, all in one process: 3307 x 3000 points in a 520^3 cube at
            the example script's 18 confidence thresholds - the dense default, match='sparse',
            device=... and device=... with solver='device' - with the kernels of libfplmatch.so alone (count + scan and fill by
            HIP events, each kernel by the profiler where it answers) and the rows downloaded;
            and 10^5 x 10^5 points in a 4096^3 box, sparse host against device only (the dense
            matrix would be 80 GB and is not run); written to profiles/match.json
  dedupe    fplsynapses.rm_tbar_multi_pred on a synthetic T-bar list with planted border
            duplicates - a lattice of spacing 34 (3 300 T-bars per 512^3, the 1536^3 run's
            density) jittered by +-2, every point within 10 voxels of a z plane 512 apart
            detected twice, float32-valued confidences - at N = 3 000, 10^5 and 10^6, all in one
            process: the neighbour table on the host (near.pairs_numpy) and on the GPU
            (near.pairs_device; the whole call, and the key kernel, torch.sort, count + scan
            and fill alone by HIP events), and the whole call per method (dense at 3 000 only);
            median, min and max over --dedupe-reps runs; written to profiles/dedupe.json
  train_vol unet_like_vol training step at the factory's 62^3 patches (50^3 outputs), loss
            masked_weighted_binary_crossentropy, at the largest batch of 32 / 16 / 8 that fits:
            the default (ReLU in the conv epilogues, the gradient masked in place) against
            FPL_TRAIN_CONVRELU_SEPARATE=1 (conv, relu_fwd, relu_bwd as passes of their own), the
            two legs alternating in one process on one trainer; median, min and max of the
            rounds' ms per step and the per-kernel table of each leg; written to
            profiles/train_vol.json
  validate  held-out validation (FplNetwork.evaluate, the val_ columns): one pass of 4 batches
            through valid.Evaluator beside 4 training steps on the same resident batches, in one
            process, medians of 5, for unet_like2 at 64 x 24^3 and vgg_like at 32 x 64^3; and the
            two kernels of fplv_loss_sums alone (HIP events); written to profiles/validate.json
  clahe     fplutils.clahe at --clahe-size^3 (default 520; the synthetic uint8 volume of synth.py),
            kernel_size 64, all in one process, one warm-up and then the median, min and max of 5:
            the numpy specification on the host (single-threaded by construction, whatever the
            cores), clahe(device=0) from a host array, clahe(device=0) from a resident tensor, and
            the four stages of fplc_clahe alone (HIP events); written to profiles/clahe.json
  substacks fplsynapses.roi_to_substacks on one 520^3 cube (448 + 2 x 36) with 32 768 T-bars, radii
            3 / 6, nothing written: numpy on the host, device=0 from a host volume and from a
            resident one; the four kernels of libfplroi.so alone (HIP events); BlockRoi.voxel_counts
            over the partition of a 4096^3 ROI on the host and with device=0; written to
            profiles/substacks.json
  deconv    Conv3DTranspose(filters, 2, strides=2) (LayerGraph.deconv), all in one process, one
            warm-up and then the median, min and max of 5: the example U-Net of
            tests/deconv_cases.py (tiny_unet_t) inferring a resident 390^3 volume at tile 102
            (pitch 96) on mfma_f32 and under FPL_FORCE_PEROP=1 with the per-kernel tables; its
            training step at 8 x 62^3 patches (the fixed-order path of a network with the layer)
            with the per-kernel table; and the deconv kernel alone (HIP events) at three shapes,
            its achieved store bandwidth beside a device-to-device copy of the same byte count;
            then the layer on the split-half graph executor: tests/deconv_gx_cases.py's unet_t3
            over the same volume at tile 102 (pitch 94) under 'auto' and under precision 'f32'
            with the per-kernel tables and their ratio, and gx_deconv2 alone at the same three
            shapes ('f16s' and 'f16'); no gate; written to profiles/deconv.json
  errors    fplerroranalysis.ObjPredErrors on the host (it has no device mode) on a 520^3 synthetic
            substack with 3 000 ground-truth points and 3 000 detections (half of them beside a
            ground-truth point), one warm-up and then the median, min and max of 5: construction,
            scores, gallery('fn'), gallery('fp'); written to profiles/errors.json
  down      Conv3D(filters, 2, strides=2) (LayerGraph.down), all in one process, one warm-up and
            then the median, min and max of 5: the example network of tests/down_cases.py
            (tiny_vnet) inferring a resident 390^3 volume at tile 102 (pitch 96) on mfma_f32 with
            the per-kernel table; its training step at 8 x 62^3 patches with the per-kernel table;
            and the down kernel alone (HIP events) at 16 -> 32, 48 -> 64 and 96 -> 128 channels
            beside a device-to-device copy of the bytes it reads and MaxPooling3D(2) of the same
            input; no gate; written to profiles/down.json
These are NOT the driver's bench line (bench.py); they document where the other
rows of SURVEY section 8 stand.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def train_vol(ctx, rounds=7, steps=8):
    """ms per unet_like_vol training step (step + Adam, constant host batch, H2D inside), the
    fused default against FPL_TRAIN_CONVRELU_SEPARATE=1.  The library reads the switch at every
    step, so both legs run on one trainer, alternating round by round (drift hits both alike)."""
    from flypylib_amd import _capi, fplmodels, synth
    g = fplmodels.unet_like_vol()[0]
    synth.synthetic_weights(g, 3)
    loss = 'masked_weighted_binary_crossentropy'
    rng = np.random.default_rng(0)
    out = None
    for batch in (32, 16, 8):
        data = rng.standard_normal((batch, 62, 62, 62, 1)).astype(np.float32)
        labels = rng.integers(0, 3, (batch, 50, 50, 50, 1)).astype(np.uint8)
        tr = _capi.Trainer(ctx, g, loss=loss)
        legs = (('fused', None), ('separate', '1'))

        def run(env, n, seed0):
            if env is None:
                os.environ.pop('FPL_TRAIN_CONVRELU_SEPARATE', None)
            else:
                os.environ['FPL_TRAIN_CONVRELU_SEPARATE'] = env
            ctx.synchronize()
            t0 = time.perf_counter()
            for s in range(n):
                tr.step(data, labels, seed0 + s); tr.apply(1.0)
            ctx.synchronize()
            return (time.perf_counter() - t0) / n * 1e3
        try:
            for _, env in legs:                       # warm-up: both legs' buffers exist
                run(env, 2, 0)
        except _capi.FplHipError as e:
            print('train_vol: batch %d does not fit (%s)' % (batch, e), flush=True)
            tr.close()
            continue
        ms = {name: [] for name, _ in legs}
        for r in range(rounds):
            for name, env in legs:
                ms[name].append(run(env, steps, 10 + r * steps))
        kern = {}
        for name, env in legs:                        # per-kernel events: runs of their own
            ctx.timing(True); ctx.timing_reset()
            run(env, 3, 1000)
            kern[name] = {k: round(v['ms'] / 3, 3) for k, v in ctx.timing_get().items()}
            ctx.timing(False)
        os.environ.pop('FPL_TRAIN_CONVRELU_SEPARATE', None)
        tr.close()
        out = {'batch': batch, 'patch': 62, 'loss': loss, 'rounds': rounds, 'steps_per_round': steps,
               'note': 'ms per step (forward, loss, backward, Adam; host batch, H2D inside), legs '
                       'alternating round by round on one trainer'}
        for name, _ in legs:
            v = ms[name]
            out[name] = {'median_ms': round(float(np.median(v)), 3), 'min_ms': round(min(v), 3),
                         'max_ms': round(max(v), 3), 'rounds_ms': [round(x, 3) for x in v],
                         'kernels_ms': kern[name]}
        f, sp = out['fused'], out['separate']
        out['separate_over_fused'] = round(sp['median_ms'] / f['median_ms'], 4)
        # the expectation: the default is not slower than the separate passes beyond the
        # run-to-run spread of the two legs
        spread = max(f['max_ms'] - f['min_ms'], sp['max_ms'] - sp['min_ms'])
        out['spread_ms'] = round(spread, 3)
        out['fused_not_slower_beyond_spread'] = bool(f['median_ms'] <= sp['median_ms'] + spread)
        break
    if out is None:
        raise RuntimeError('train_vol: no batch of 32 / 16 / 8 fits')
    return out


def validate_bench(ctx, torch, batches=4, reps=5):
    """ms of one validation pass of `batches` batches (valid.Evaluator: inference-mode forward +
    fplv_loss_sums, one download) beside the ms of as many training steps (step + Adam) on the
    same resident batches, in one process, medians of `reps`; and fplv_loss_sums alone by HIP
    events on the case's prediction size"""
    from flypylib_amd import FplNetwork, _capi, fplmodels, valid
    out = {'batches': batches, 'reps': reps,
           'note': 'device-resident batches on both sides; ms per pass / per %d steps' % batches}
    rng = np.random.default_rng(0)
    for name, batch, patch in (('unet_like2', 64, 24), ('vgg_like', 32, 64)):
        net = FplNetwork(getattr(fplmodels, name))
        ev = valid.evaluator_of(net)
        od = ev.program.out_dims((patch,) * 3)
        hi = 2 if name == 'vgg_like' else 3
        pairs = []
        for _ in range(batches):
            x = torch.from_numpy(rng.standard_normal((batch,) + (patch,) * 3 + (1,)).astype(np.float32)).to('cuda:0')
            y = torch.from_numpy(rng.integers(0, hi, (batch,) + od).astype(np.uint8)).to('cuda:0')
            pairs.append((x, y))
        loss = getattr(net.compile_args['loss'], '__name__', net.compile_args['loss']) \
            if net.compile_args else 'binary_crossentropy'
        tr = _capi.Trainer(ctx, net.train_single, loss=loss)

        def val_pass():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev.run_sums(iter(pairs), batches)
            return (time.perf_counter() - t0) * 1e3

        def train_steps():
            ctx.synchronize()
            t0 = time.perf_counter()
            for s, (x, y) in enumerate(pairs):
                tr.step(x, y, seed=s); tr.apply(1.0)
            tr.metrics()
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3
        val_pass(); train_steps()                      # warm-up: both sides' buffers exist
        v = [val_pass() for _ in range(reps)]
        t = [train_steps() for _ in range(reps)]
        n = batch * int(np.prod(od))
        pred, lab = torch.rand(n, device='cuda:0'), pairs[0][1].reshape(-1)
        sums = torch.zeros(8, dtype=torch.float64, device='cuda:0')
        kern = []
        for _ in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            valid.loss_sums_device(pred, lab, loss, sums=sums, scratch=ev.scratch)
            b.record(); b.synchronize()
            kern.append(a.elapsed_time(b))
        tr.close()
        vm, tm = float(np.median(v)), float(np.median(t))
        out['%s_%dx%d' % (name, batch, patch)] = {
            'loss': loss, 'elements_per_batch': n,
            'validation_pass_ms': round(vm, 3), 'validation_ms_per_batch': round(vm / batches, 3),
            'validation_runs_ms': [round(x, 3) for x in v],
            'training_steps_ms': round(tm, 3), 'training_ms_per_step': round(tm / batches, 3),
            'training_runs_ms': [round(x, 3) for x in t],
            'validation_over_training': round(vm / tm, 4),
            'loss_sums_kernels_ms': round(float(np.median(kern[1:])), 4)}
        print(json.dumps(out['%s_%dx%d' % (name, batch, patch)]), flush=True)
    return out


def train_gen(ctx, torch, steps=30, vol=200):
    """ms/step of the training loop fed by a constant batch, the host generator and the
    device generator (same process, same trainer), on synthetic volumes"""
    from flypylib_amd import _capi, fplmodels, fplobjdetect, synth, train as fpl_train
    shape = (vol,) * 3
    im = synth.em_volume_u8(31, shape).astype(np.float32)
    ll = (synth.hash_uniform_f32(131, shape) > np.float32(0.97)).astype(np.uint8)
    train_data = [(im, ll, np.ones(shape, np.uint8))]
    out = {'volume': list(shape), 'image_dtype': 'float32', 'steps': steps}

    def loop(tr, gen):
        # fit_generator's loop without its CSV bookkeeping and metrics() call: the same
        # _Prefetch (depth 2) and _DeviceStager.  The ring of a device generator is safe here
        # for the reason it is there: Trainer.step returns (loss, accuracy), which it reads
        # back from the device, so the step has consumed its batch before the next is taken.
        # The vgg loops train on a constant 12^3 label block (see the DESIGN.md section), so
        # what differs between the three loops is the cutting of the data alone.
        batches = fpl_train._Prefetch(gen, stage=fpl_train._DeviceStager(ctx.device))
        try:
            for s in range(3):
                tr.step(*next(batches), s); tr.apply(1.0)
            ctx.synchronize()
            t0 = time.perf_counter()
            for s in range(steps):
                tr.step(*next(batches), s + 3); tr.apply(1.0)
            ctx.synchronize()
            return (time.perf_counter() - t0) / steps * 1e3
        finally:
            batches.close()

    def constant(batch):
        while True:
            yield batch

    def kernel_ms(make_dev, rot):
        """the gather kernel alone, every example of the batch with one rot"""
        dev = make_dev()
        draw = dev.plan.records

        def forced():
            rec = draw()
            rec['rot'] = rot
            return rec
        dev.plan.records = forced
        dev.time_kernel = True
        for _ in range(13):
            next(dev)
        return float(np.median(dev.kernel_ms[3:]))

    # vgg_like, 32 x 64^3.  gen_batches labels a patch by its centre voxel (or 6^3 around it);
    # on a 64^3 patch vgg_like's output is 12^3, so - as in the constant-batch rows - the
    # labels are a constant 12^3 block and the generators supply the data, which is all but
    # 32 bytes of what they move.
    g = fplmodels.vgg_like()[0]
    synth.synthetic_weights(g, 8)
    tr = _capi.Trainer(ctx, g)
    rng = np.random.default_rng(0)
    lab12 = (rng.random((32, 12, 12, 12)) > 0.9).astype(np.uint8)
    lab12_dev = torch.from_numpy(lab12).to('cuda:%d' % ctx.device)
    data = rng.standard_normal((32, 64, 64, 64)).astype(np.float32)

    def data_of(gen, labels):
        for d, _ in gen:
            yield d, labels
    mk = lambda **kw: fplobjdetect.gen_batches(train_data, 64, 32, rng=np.random.RandomState(0), **kw)  # noqa: E731
    dev = mk(device=ctx.device)
    r = {'constant_ms': loop(tr, constant((data, lab12))),
         'host_gen_ms': loop(tr, data_of(mk(), lab12)),
         'device_gen_ms': loop(tr, data_of(dev, lab12_dev))}
    r['planner_ms_per_batch'] = dev.plan_seconds / dev.batches * 1e3
    moved = 32 * 64 ** 3 * 8
    for rot in (0, 1):
        ms = kernel_ms(lambda: mk(device=ctx.device), rot)
        r['gather_rot%d_ms' % rot] = ms
        r['gather_rot%d_gb_s' % rot] = moved / ms / 1e6
    r['device_over_constant'] = r['device_gen_ms'] / r['constant_ms']
    r['host_over_device'] = r['host_gen_ms'] / r['device_gen_ms']
    out['vgg_like_b32_64cubed'] = {k: round(v, 4) for k, v in r.items()}
    print(json.dumps(out['vgg_like_b32_64cubed']), flush=True)
    tr.close()

    # unet_like2, 64 x 24^3, gen_volume2 with noise on: data and 6^3 labels from the generator
    g = fplmodels.unet_like2()[0]
    synth.synthetic_weights(g, 3)
    tr = _capi.Trainer(ctx, g, loss='masked_focal_loss')
    data = rng.standard_normal((64, 24, 24, 24, 1)).astype(np.float32)
    labels = rng.integers(0, 3, (64, 6, 6, 6, 1)).astype(np.uint8)
    mk = lambda **kw: fplobjdetect.gen_volume2(train_data, 24, 64, 0.5, noise_aug=[0.05, 0.1],  # noqa: E731
                                               rng=np.random.RandomState(0), **kw)
    dev = mk(device=ctx.device)
    r = {'constant_ms': loop(tr, constant((data, labels))),
         'host_gen_ms': loop(tr, mk()),
         'device_gen_ms': loop(tr, dev)}
    r['planner_ms_per_batch'] = dev.plan_seconds / dev.batches * 1e3
    moved = 64 * 24 ** 3 * 8
    for rot in (0, 1):
        ms = kernel_ms(lambda: mk(device=ctx.device), rot)
        r['gather_rot%d_ms' % rot] = ms
        r['gather_rot%d_gb_s' % rot] = moved / ms / 1e6
    r['device_over_constant'] = r['device_gen_ms'] / r['constant_ms']
    r['host_over_device'] = r['host_gen_ms'] / r['device_gen_ms']
    out['unet_like2_b64_24cubed'] = {k: round(v, 4) for k, v in r.items()}
    tr.close()
    return out


def mine_bench(ctx, torch, n=520, reps=5):
    """the mining step between two training rounds, host path against device path"""
    from flypylib_amd import FplNetwork, batchgen, fplmodels, mine, synth
    shape = (n,) * 3
    dev = torch.device('cuda', ctx.device)
    u8 = synth.em_volume_u8(41, shape)
    ll = (synth.hash_uniform_f32(141, shape) > np.float32(0.97)).astype(np.uint8)
    mm = np.ones(shape, np.uint8)
    mm[: n // 4, : n // 3, :] = 0
    net = FplNetwork(fplmodels.vgg_like)
    synth.synthetic_weights(net.train_single, 1)
    net.infer_sz = (102,) * 3
    net._set_infer()
    norm, l0, l1 = (128.0, 33.0), (0.05, 2.0), (0.1, 0.5)
    out = {'volume': list(shape), 'voxels': n ** 3, 'reps': reps}

    def timed(fn, k):
        fn()
        torch.cuda.synchronize(dev)
        ts = []
        for _ in range(k):
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize(dev)
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3, r

    # voxel_loss through the public entry point
    t_inf, _ = timed(lambda: net.infer(u8, normalize=norm), reps)
    t_host, loss_host = timed(lambda: net.voxel_loss(u8, (ll, mm), l0, l1, normalize=norm), 1)
    t_dev, loss_dev = timed(lambda: net.voxel_loss(u8, (ll, mm), l0, l1, normalize=norm,
                                                   device=ctx.device), reps)
    ll_d, mm_d = mine.to_device_u8(ll, dev), mine.to_device_u8(mm, dev)
    t_res, _ = timed(lambda: net.voxel_loss(u8, (ll_d, mm_d), l0, l1, normalize=norm,
                                            device=ctx.device), reps)
    diff = np.abs(loss_dev.cpu().numpy() - loss_host)
    out['voxel_loss'] = dict(infer_host_result_ms=t_inf, host_ms=t_host, device_ms=t_dev,
                             device_resident_labels_ms=t_res, host_over_device=t_host / t_dev,
                             max_abs_diff_host_vs_device=float(diff.max()),
                             voxels_with_loss=int((loss_host > 0).sum()))
    print(json.dumps(out['voxel_loss']), flush=True)
    del loss_host, diff

    # the kernel alone on a synthetic float32 prediction that leaves a mined volume: most
    # negatives confident
    pred = torch.from_numpy(synth.hash_uniform_f32(241, shape) ** 32).to(dev)
    loss = torch.empty(shape, dtype=torch.float32, device=dev)
    edge = [int(round(c / 2)) for c in net.rf_size]
    ms = []
    for i in range(3 + 2 * reps):
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        e0.record()
        mine._minecapi.voxel_loss(pred.data_ptr(), ll_d.data_ptr(), mm_d.data_ptr(), shape, edge,
                                  l0, l1, loss.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        e1.record()
        torch.cuda.synchronize(dev)
        ms.append(e0.elapsed_time(e1))
    k_ms = float(np.median(ms[3:]))
    out['voxel_loss_kernel'] = dict(ms=k_ms, bytes_per_voxel=10, gb_s=10 * n ** 3 / k_ms / 1e6,
                                    timing='HIP events around one launch, median of %d' % (2 * reps))
    print(json.dumps(out['voxel_loss_kernel']), flush=True)

    # candidate tables: Volume2Planner construction, before the first batch can be drawn
    im = u8
    w_dev = loss
    w_host = loss.cpu().numpy()
    out['weights_positive_fraction'] = float((w_host > 0).mean())
    tables = {}
    for name, host_entry, dev_entry in (
            ('unweighted', (im, ll, mm), (im, ll_d, mm_d)),
            ('mined', (im, ll, mm, w_host), (im, ll_d, mm_d, w_dev))):
        t0 = time.perf_counter()
        ph = batchgen.Volume2Planner([host_entry], 24, 64, 0.5)
        t_h = (time.perf_counter() - t0) * 1e3
        t_d, pd = timed(lambda: batchgen.Volume2Planner([dev_entry], 24, 64, 0.5, tables='device',
                                                        device=ctx.device), 3)
        t_up, _ = timed(lambda: batchgen.Volume2Planner([host_entry], 24, 64, 0.5,
                                                        tables='device', device=ctx.device), 3)
        same = all(a.tobytes() == b.tobytes() for a, b in zip(ph._cols, pd._cols))
        # the three launches alone, class by class
        kern = {}
        for cc in range(2):
            ks = []
            for _ in range(4):
                e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                e0.record()
                mine.candidates_device(ll_d, mm_d, (12, 12, 12), cc,
                                       w_dev if name == 'mined' else None, download=False)
                e1.record()
                torch.cuda.synchronize(dev)
                ks.append(e0.elapsed_time(e1))
            kern['class%d_count_scan_fill_ms' % cc] = float(np.median(ks[1:]))
        tables[name] = dict(host_ms=t_h, device_resident_ms=t_d, device_upload_ms=t_up,
                            host_over_device_resident=t_h / t_d, rows=[int(v) for v in ph._n],
                            downloaded_bytes=int(sum(ph._n)) * (16 if name == 'mined' else 12),
                            identical_tables=bool(same), **kern)
        print(json.dumps({name: tables[name]}), flush=True)
        del ph, pd
    out['tables'] = tables
    return out


def match_bench(ctx, torch, reps=5):
    """obj_pr_curve: the dense default against match='sparse' and device=..."""
    from flypylib_amd import _matchcapi, fplobjdetect, match
    dev = torch.device('cuda', ctx.device)
    t_match = 27
    thds = np.arange(0.6, 0.96, 0.02)               # the example script's 18 thresholds

    def points(seed, n_gt, n_hit, n_fp, box):
        rs = np.random.RandomState(seed)
        gt = rs.rand(n_gt, 3) * box
        pred = np.concatenate([gt[:n_hit] + rs.randn(n_hit, 3) * 4, rs.rand(n_fp, 3) * box])
        return {'locs': pred, 'conf': 0.6 + 0.4 * rs.rand(len(pred))}, {'locs': gt}

    def timed(fn, k):
        ts = []
        for _ in range(k):
            t0 = time.perf_counter()
            r = fn()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3, r

    def kernels(pred, gt):
        """count + scan and fill by HIP events around the two entry points; the three kernels
        one by one from the profiler, or None where it does not report them"""
        n, m, t2 = len(pred), len(gt), match.threshold2(t_match)
        nscr = _matchcapi.scratch_bytes(n, m)
        p_dev, g_dev = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
        scratch = torch.empty((nscr + 7) // 8, dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream(dev)
        args = (p_dev.data_ptr(), n, g_dev.data_ptr(), m, t2, scratch.data_ptr(), nscr)
        total = _matchcapi.pairs_count(*args, stream.cuda_stream)
        cols = torch.empty((2, total), dtype=torch.int32, device=dev)

        def fill():
            _matchcapi.pairs_fill(*args, total, cols[0].data_ptr(), cols[1].data_ptr(),
                                  stream.cuda_stream)
        fill()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        count_ms, fill_ms = [], []
        for _ in range(reps):
            ev[0].record(stream)
            _matchcapi.pairs_count(*args, stream.cuda_stream)
            ev[1].record(stream)
            fill()
            ev[2].record(stream)
            stream.synchronize()
            count_ms.append(ev[0].elapsed_time(ev[1]))
            fill_ms.append(ev[1].elapsed_time(ev[2]))
        res = {'rows': int(total), 'segments': _matchcapi.segments(n, m),
               'count_and_scan_ms': float(np.median(count_ms)), 'fill_ms': float(np.median(fill_ms)),
               'pair_tests': n * m}
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                _matchcapi.pairs_count(*args, stream.cuda_stream)
                fill()
                stream.synchronize()
            each = {}
            for e in prof.key_averages():
                for k in ('count_kernel', 'scan_kernel', 'fill_kernel'):
                    if k in e.key:
                        us = getattr(e, 'device_time_total', None)
                        if us is None:
                            us = getattr(e, 'cuda_time_total', 0.0)
                        each[k + '_ms'] = us / 1e3 / max(1, e.count)
            res['profiler'] = each or None
        except Exception as e:      # noqa: BLE001
            res['profiler'] = None
            res['profiler_error'] = '%s: %s' % (type(e).__name__, e)
        return res

    def same(a, b):
        return all(np.array_equal(getattr(a, f), getattr(b, f))
                   for f in ('num_tp', 'tot_pred', 'tot_gt', 'pp', 'rr'))

    def device_solver(p, g, r_ref, t_dev, k):
        """solver='device' beside the device= figure of the same process: the whole call, and
        the stages of one match_device call over all thresholds"""
        curve(p, g, t_match, thds[-2:], device=ctx.device, solver='device')          # warm-up
        t_all, r = timed(lambda: curve(p, g, t_match, thds, device=ctx.device, solver='device'), k)
        base = p['conf'] >= thds.min()
        info = {}
        match.match_device(p['locs'][base], g['locs'], t_match, ctx.device, conf=p['conf'][base],
                           thresholds=thds, info=info)
        return {'obj_pr_curve_ms': t_all, 'device_over_device_solver': t_dev / t_all,
                'table_ms': info['table_ms'], 'costs_labels_sort_solve_ms': info['solve_ms'],
                'download_ms': info['download_ms'], 'overflow': int(sum(info['overflow'])),
                'sweeps': int(max(info['sweeps'])), 'components': int(max(info['components'])),
                'largest_component_pairs': int(max(info['largest'])), 'equal_results': bool(same(r, r_ref))}

    out = {'thresholds': len(thds), 'dist_thresh': t_match, 'reps': reps}
    # one substack of the example: 3307 predictions, 3000 T-bars in a 520^3 cube
    p, g = points(0, 3000, 2800, 507, 520.0)
    curve = fplobjdetect.obj_pr_curve
    fplobjdetect.obj_pr_curve(p, g, t_match, thds[-2:], device=ctx.device)       # warm-up
    t_dense, r_dense = timed(lambda: curve(p, g, t_match, thds), 1)
    print('match: dense %.0f ms' % t_dense, flush=True)
    t_sparse, r_sparse = timed(lambda: curve(p, g, t_match, thds, match='sparse'), reps)
    t_dev, r_dev = timed(lambda: curve(p, g, t_match, thds, device=ctx.device), reps)
    t_np, _ = timed(lambda: match.pairs_numpy(p['locs'], g['locs'], t_match), reps)
    t_pd, _ = timed(lambda: match.pairs_device(p['locs'], g['locs'], t_match, ctx.device), reps)
    out['substack'] = {
        'points': [len(p['locs']), len(g['locs'])], 'box': 520,
        'obj_pr_curve_dense_ms': t_dense, 'obj_pr_curve_sparse_ms': t_sparse,
        'obj_pr_curve_device_ms': t_dev, 'dense_over_sparse': t_dense / t_sparse,
        'dense_over_device': t_dense / t_dev, 'pairs_numpy_ms': t_np, 'pairs_device_ms': t_pd,
        'equal_results': bool(same(r_dense, r_sparse) and same(r_dense, r_dev)),
        'solver_device': device_solver(p, g, r_dev, t_dev, reps),
        'kernels': kernels(p['locs'], g['locs'])}
    print(json.dumps(out['substack']), flush=True)
    # a whole ROI: 10^5 x 10^5 points in a 4096^3 box
    p, g = points(1, 100000, 90000, 10000, 4096.0)
    t_pd, tab = timed(lambda: match.pairs_device(p['locs'], g['locs'], t_match, ctx.device), reps)
    t_dev, r_dev = timed(lambda: curve(p, g, t_match, thds, device=ctx.device), 3)
    print('match: roi device %.0f ms' % t_dev, flush=True)
    roi_solver = device_solver(p, g, r_dev, t_dev, 3)
    print('match: roi solver=device %s' % json.dumps(roi_solver), flush=True)
    # the host table is two minutes of numpy: built once, inside the curve, and timed there
    host_table = {}
    real = match.pairs_numpy

    def pairs_timed(*a):
        t0 = time.perf_counter()
        host_table['table'] = real(*a)
        host_table['ms'] = (time.perf_counter() - t0) * 1e3
        return host_table['table']
    match.pairs_numpy = pairs_timed
    try:
        t_sparse, r_sparse = timed(lambda: curve(p, g, t_match, thds, match='sparse'), 1)
    finally:
        match.pairs_numpy = real
    t_np, tab_np = host_table['ms'], host_table['table']
    out['roi'] = {
        'points': [len(p['locs']), len(g['locs'])], 'box': 4096,
        'obj_pr_curve_dense_ms': None,
        'dense_note': 'not run: the dense cost matrix alone is 80 GB',
        'obj_pr_curve_sparse_ms': t_sparse, 'obj_pr_curve_device_ms': t_dev,
        'sparse_over_device': t_sparse / t_dev, 'pairs_numpy_ms': t_np, 'pairs_device_ms': t_pd,
        'equal_tables': bool(np.array_equal(tab[0], tab_np[0]) and np.array_equal(tab[1], tab_np[1])),
        'equal_results': bool(same(r_sparse, r_dev)),
        'solver_device': roi_solver,
        'kernels': kernels(p['locs'], g['locs'])}
    print(json.dumps(out['roi']), flush=True)
    return out


def dedupe_points(n, seed=0, spacing=34.0, jitter=2, near_plane=10.0, period=512.0, first=250.0):
    """about n T-bars: a jittered lattice; every point within `near_plane` voxels of a z plane
    `period` apart (the first at z = `first`) was detected a second time within 10 voxels; shuffled"""
    rs = np.random.RandomState(seed)
    share = 2 * near_plane / period
    side = int(round((n / (1 + share)) ** (1 / 3.0)))
    g = np.arange(side) * spacing + 40.0
    pts = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)
    pts += rs.randint(-jitter, jitter + 1, pts.shape)
    to_plane = np.abs((pts[:, 2] - first + period / 2) % period - period / 2)
    twice = pts[to_plane <= near_plane]
    pts = np.concatenate([pts, twice + rs.randint(-6, 7, twice.shape)])
    pts = pts[rs.permutation(len(pts))]
    conf = (rs.rand(len(pts)) * 0.75 + 0.25).astype(np.float32).astype(np.float64)
    return {'locs': pts, 'conf': conf}, len(twice)


def dedupe_bench(ctx, torch, sizes=(3000, 100000, 1000000), reps=5):
    """rm_tbar_multi_pred and its neighbour table, host against device"""
    from flypylib_amd import _nearcapi, fplsynapses, near
    dev = torch.device('cuda', ctx.device)
    thresh = 30

    def spread(ms):
        return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)),
                    runs=len(ms))

    def timed(fn, k, warm=0):
        for _ in range(warm):
            fn()
        ts, r = [], None
        for _ in range(k):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize(dev)
            ts.append((time.perf_counter() - t0) * 1e3)
        return spread(ts), r

    rows = []
    for n_want in sizes:
        tb, doubled = dedupe_points(n_want)
        pts = np.ascontiguousarray(tb['locs'])
        n = len(pts)
        row = dict(points=n, doubled=int(doubled), neighbor_thresh=thresh,
                   timing='wall clock around the call, synchronised; ms; median, min, max')
        row['table_host_ms'], tab = timed(lambda: near.pairs_numpy(pts, thresh), reps)
        row['table_device_ms'], tab_d = timed(lambda: near.pairs_device(pts, thresh, ctx.device), reps, warm=2)
        row['entries'] = int(len(tab[1]))
        row['longest_row'] = int(np.diff(tab[0]).max())
        row['equal_tables'] = bool(np.array_equal(tab[0], tab_d[0]) and np.array_equal(tab[1], tab_d[1]))
        # the steps of pairs_device alone, by HIP events on resident inputs
        t2 = near.threshold2(thresh)
        origin, cell, dims = near.grid_of(pts, thresh)
        stream = torch.cuda.current_stream(dev)
        p_dev = torch.from_numpy(pts).to(dev)
        keys0 = torch.empty(n, dtype=torch.int64, device=dev)
        nscr = _nearcapi.scratch_bytes(n)
        scratch = torch.empty((nscr + 7) // 8, dtype=torch.int64, device=dev)
        indices = torch.empty(len(tab[1]), dtype=torch.int32, device=dev)
        steps = {'keys': [], 'sort': [], 'count_scan': [], 'fill': []}
        for i in range(2 + reps):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            ev[0].record()
            _nearcapi.cell_keys(p_dev.data_ptr(), n, origin, cell, dims, keys0.data_ptr(), stream.cuda_stream)
            ev[1].record()
            keys, order = torch.sort(keys0)
            ev[2].record()
            args = (p_dev.data_ptr(), n, t2, origin, cell, dims, keys.data_ptr(), order.data_ptr(),
                    scratch.data_ptr(), nscr)
            total = _nearcapi.pairs_count(*args, stream.cuda_stream)
            ev[3].record()
            _nearcapi.pairs_fill(*args, total, indices.data_ptr(), stream.cuda_stream)
            ev[4].record()
            torch.cuda.synchronize(dev)
            if i >= 2:
                for k, name in enumerate(('keys', 'sort', 'count_scan', 'fill')):
                    steps[name].append(ev[k].elapsed_time(ev[k + 1]))
        row['device_steps_ms'] = {k: spread(v) for k, v in steps.items()}
        row['device_steps_ms']['sum_of_medians'] = float(sum(np.median(v) for v in steps.values()))
        row['device_steps_timing'] = ('HIP events around each step on resident inputs; count_scan '
                                      'includes the gather and the read-back of the total')
        row['device_scratch_bytes'] = int(nscr)
        del p_dev, keys0, scratch, indices, keys, order
        # the whole call
        call_reps = reps
        row['call_sparse_host_ms'], r_host = timed(
            lambda: fplsynapses.rm_tbar_multi_pred(tb, neighbor_thresh=thresh, method='sparse'), call_reps)
        row['call_sparse_device_ms'], r_dev = timed(
            lambda: fplsynapses.rm_tbar_multi_pred(tb, neighbor_thresh=thresh, method='sparse',
                                                   device=ctx.device), call_reps)
        row['equal_results'] = bool(all(np.array_equal(a, b) for a, b in zip(r_host, r_dev)))
        row['moved'], row['removed'] = int(r_host[1].sum()), int(r_host[0].sum())
        # solver='device': the merge loop on the GPU too, same process, same inputs
        from flypylib_amd import dedupe
        minfo = {}
        row['solver_device_ms'], r_solv = timed(
            lambda: fplsynapses.rm_tbar_multi_pred(tb, neighbor_thresh=thresh, method='sparse',
                                                   device=ctx.device, solver='device', info=minfo),
            call_reps, warm=1)
        row['solver_device_equal'] = bool(all(np.array_equal(a, b) and a.dtype == b.dtype
                                              for a, b in zip(r_host, r_solv)))
        row['solver_device_info'] = dict(minfo)
        row['solver_device_to_call_sparse_device'] = (row['solver_device_ms']['median']
                                                      / row['call_sparse_device_ms']['median'])
        stage_runs = []
        for _ in range(call_reps):
            st = {}
            r_st = dedupe.merge_device(tb['locs'], tb['conf'], np.zeros(n), thresh, ctx.device, stages=st)
            row['solver_device_equal'] &= bool(all(np.array_equal(a, b) for a, b in zip(r_host, r_st)))
            stage_runs.append(st)
        row['solver_device_stages_ms'] = {k: spread([s[k] for s in stage_runs]) for k in stage_runs[0]}
        row['solver_device_stages_timing'] = (
            'wall clock per stage, synchronised after each (which the plain call does not do): '
            'argsort_upload = np.argsort(-conf), its rank and the uploads of conf, labels, rank; '
            'table = upload of the points, cell keys, sort, count, fill; filter = the rows the '
            'reference keeps; labels = the sweeps (solver_device_info.sweeps of them, a read-back '
            'each); sort = group keys, torch.sort, boundaries, compaction; solve = the merge loop '
            'and the compaction of the flagged ids; download = rm, mv, mv_loc and, if a component '
            'was flagged, what the closure reads; closure_host = the host loop over the flagged '
            'components')
        points_with_neighbours = int((np.diff(near.pairs_numpy(pts, thresh)[0]) > 0).sum())
        row['solver_device_host_share'] = minfo['host_points'] / max(points_with_neighbours, 1)
        if n <= 5000:
            row['call_dense_ms'], r_dense = timed(
                lambda: fplsynapses.rm_tbar_multi_pred(tb, neighbor_thresh=thresh, method='dense'), reps)
            row['dense_equals_sparse'] = bool(all(np.array_equal(a, b) for a, b in zip(r_dense, r_host)))
        else:
            row['call_dense_ms'] = None
            row['dense_note'] = 'not run: the distance matrix alone is %.0f GB' % (8.0 * n * n / 1e9)
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def labels_bench(ctx, torch, sizes=(520, 256), reps=5):
    """write_labels_mask, host path against device path"""
    from flypylib_amd import fplsynapses, labels
    dev = torch.device('cuda', ctx.device)
    rows = []
    for n in sizes:
        shape = (n,) * 3
        for ru, ri in ((3, 6), (6, 12)):
            half, step, buf = max(ru, ri), 16, 14
            rs = np.random.RandomState(n + ru)
            grid = np.arange(half + 3, n - half - 3, step)
            locs = np.array([(x, y, z) for z in grid for y in grid for x in grid], np.float64)
            locs += rs.randint(-3, 4, locs.shape)
            rs.shuffle(locs)
            tbars = {'locs': locs, 'conf': np.ones(len(locs))}
            roi = np.ones(shape, np.uint8)
            row = dict(volume=list(shape), voxels=n ** 3, radius_use=ru, radius_ign=ri,
                       buffer_size=buf, tbars=len(locs), density='one T-bar per %d^3 voxels' % step)

            t0 = time.perf_counter()
            host = fplsynapses.write_labels_mask(tbars, roi, ru, ri, buf, None)
            row['host_ms'] = (time.perf_counter() - t0) * 1e3

            def timed(fn, k):
                fn()
                torch.cuda.synchronize(dev)
                ts = []
                for _ in range(k):
                    t0 = time.perf_counter()
                    r = fn()
                    torch.cuda.synchronize(dev)
                    ts.append(time.perf_counter() - t0)
                return float(np.median(ts)) * 1e3, r

            row['device_ms'], got = timed(lambda: fplsynapses.write_labels_mask(
                tbars, roi, ru, ri, buf, None, device=ctx.device), reps)
            roi_d = torch.from_numpy(roi).to(dev)
            row['device_resident_roi_ms'], _ = timed(lambda: fplsynapses.write_labels_mask(
                tbars, roi_d, ru, ri, buf, None, device=ctx.device), reps)
            row['identical'] = bool(np.array_equal(got[0].cpu().numpy(), host[0])
                                    and np.array_equal(got[1].cpu().numpy(), host[1]))
            row['host_over_device'] = row['host_ms'] / row['device_ms']
            del host

            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                table = labels.plan_tbars(tbars, shape, ru, ri)
                offsets, index = labels.plan_bricks(table, shape, half)
                ts.append(time.perf_counter() - t0)
            row['planner_ms'] = float(np.median(ts)) * 1e3
            row['pairs'] = int(len(index))
            row['longest_brick_list'] = int(np.diff(offsets).max())
            row['upload_bytes_tables'] = int(table.nbytes + offsets.nbytes + index.nbytes)
            row['upload_bytes_roi_from_host'] = int(roi.nbytes)

            tabs = [torch.from_numpy(a).to(dev) for a in (table, offsets, index)]
            ll, mm = (torch.empty(shape, dtype=torch.uint8, device=dev) for _ in range(2))
            ms = []
            for i in range(3 + 2 * reps):
                e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                e0.record()
                labels._labelscapi.labels_mask(
                    roi_d.data_ptr(), tabs[0].data_ptr(), len(table), tabs[1].data_ptr(),
                    tabs[2].data_ptr(), len(index), shape, ru, ri, buf, ll.data_ptr(),
                    mm.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
                e1.record()
                torch.cuda.synchronize(dev)
                ms.append(e0.elapsed_time(e1))
            k_ms = float(np.median(ms[3:]))
            row['kernel'] = dict(ms=k_ms, bytes_per_voxel=3, gb_s=3 * n ** 3 / k_ms / 1e6,
                                 timing='HIP events around one launch, median of %d' % (2 * reps))
            # the device planner (libfplplan.so), same process, same inputs
            row['device_planner_ms'], got_p = timed(lambda: fplsynapses.write_labels_mask(
                tbars, roi, ru, ri, buf, None, device=ctx.device, planner='device'), reps)
            row['device_planner_resident_roi_ms'], _ = timed(lambda: fplsynapses.write_labels_mask(
                tbars, roi_d, ru, ri, buf, None, device=ctx.device, planner='device'), reps)
            row['device_planner_identical'] = bool(torch.equal(got_p[0], got[0])
                                                   and torch.equal(got_p[1], got[1]))
            t_off, t_idx = labels.plan_bricks_device(table, shape, half, dev)
            row['device_planner_tables_identical'] = bool(
                np.array_equal(t_off.cpu().numpy(), offsets)
                and np.array_equal(t_idx.cpu().numpy(), index))
            row['upload_bytes_tables_device_planner'] = int(table.nbytes)
            nbk = int(np.prod(labels.brick_counts(shape)))
            nbytes = labels._plancapi.scratch_bytes(len(table), nbk, len(index))
            scratch = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=dev)
            ms = []
            for i in range(3 + 2 * reps):
                e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                e0.record()
                labels._plancapi.plan_bricks(
                    tabs[0].data_ptr(), len(table), shape, half, t_off.data_ptr(),
                    t_idx.data_ptr(), len(index), scratch.data_ptr(), scratch.numel() * 4,
                    torch.cuda.current_stream(dev).cuda_stream)
                e1.record()
                torch.cuda.synchronize(dev)
                ms.append(e0.elapsed_time(e1))
            assert int(scratch[0].item()) == 0
            row['planner_device_ms'] = float(np.median(ms[3:]))
            row['planner_device_timing'] = ('HIP events around fplp_plan_bricks, median of %d'
                                            % (2 * reps))
            row['planner_device_scratch_bytes'] = int(nbytes)
            row['plan_pairs_ms'] = timed(lambda: labels.plan_pairs(table, shape, half), reps)[0]
            print(json.dumps(row), flush=True)
            rows.append(row)
            del got, got_p, roi_d, ll, mm, tabs, t_off, t_idx, scratch
    return rows


def clahe_bench(ctx, torch, n=520, k=64, reps=5):
    """fplutils.clahe: the numpy specification against device=, in one process"""
    from flypylib_amd import _clahecapi, clahe, fplutils, synth
    dev = torch.device('cuda', ctx.device)
    im = synth.em_volume_u8(3, (n, n, n))
    row = dict(volume=[n, n, n], voxels=n ** 3, dtype='uint8', kernel_size=k, clip_limit=0.01, nbins=256,
               reps=reps, timing='one warm-up, then median / min / max of %d, ms' % reps,
               host_note='clahe_numpy is single-threaded by construction; the cores of the machine '
                         'do not enter')

    def stats(ts):
        return dict(median=float(np.median(ts)), min=float(min(ts)), max=float(max(ts)))

    def timed(fn, sync):
        ts, r = [], None
        for i in range(reps + 1):
            t0 = time.perf_counter()
            r = fn()
            if sync:
                torch.cuda.synchronize(dev)
            if i:
                ts.append((time.perf_counter() - t0) * 1e3)
        return stats(ts), r

    row['host_ms'], host = timed(lambda: fplutils.clahe(im, k), False)
    row['device_from_host_ms'], got = timed(lambda: fplutils.clahe(im, k, device=ctx.device), True)
    res = torch.from_numpy(im).to(dev)
    row['device_resident_ms'], got_r = timed(lambda: fplutils.clahe(res, k, device=ctx.device), True)
    row['identical'] = bool(np.array_equal(got.cpu().numpy(), host) and torch.equal(got, got_r))
    row['host_over_device_resident'] = row['host_ms']['median'] / row['device_resident_ms']['median']
    del host, got_r
    need = _clahecapi.scratch_bytes(n, n, n, k, k, 256)
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    row['scratch_bytes'] = int(need)
    stream = torch.cuda.current_stream(dev).cuda_stream
    stages = (('range', _clahecapi.STAGE_RANGE), ('maps', _clahecapi.STAGE_MAPS),
              ('apply', _clahecapi.STAGE_APPLY), ('finish', _clahecapi.STAGE_FINISH))
    ms = {name: [] for name, _ in stages}
    for i in range(reps + 1):
        for name, stage in stages:
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record()
            _clahecapi.clahe(res, True, (n, n, n), (k, k), clahe.clip_count(0.01, k, k), 256, False, got,
                             scratch, need, stage, stream)
            e1.record()
            torch.cuda.synchronize(dev)
            if i:
                ms[name].append(e0.elapsed_time(e1))
    row['kernels_ms'] = {name: stats(v) for name, v in ms.items()}
    row['kernels_timing'] = 'HIP events around one stage of fplc_clahe on the resident volume'
    print(json.dumps(row), flush=True)
    return row


def errors_bench(n=520, n_points=3000, reps=5):
    """fplerroranalysis.ObjPredErrors on a synthetic substack, on the host (there is no device mode)"""
    from flypylib_amd import fplerroranalysis as ea, synth
    rs = np.random.RandomState(7)
    im = synth.em_volume_u8(3, (n, n, n))
    pd = rs.rand(n, n, n).astype(np.float32)
    gt = {'locs': rs.randint(0, n, (n_points, 3)).astype(np.float64), 'conf': np.ones(n_points)}
    near = np.clip(gt['locs'][:n_points // 2] + rs.randint(-4, 5, (n_points // 2, 3)), 0, n - 1)
    pred = {'locs': np.concatenate([near, rs.randint(0, n, (n_points - n_points // 2, 3))]).astype(np.float64),
            'conf': rs.rand(n_points)}
    row = dict(volume=[n, n, n], dtype='uint8', gt=n_points, detections=n_points, obj_min_dist=27,
               smoothing_sigma=5, reps=reps, where='host (numpy, scipy)',
               timing='one warm-up, then median / min / max of %d, ms' % reps)

    def timed(fn):
        ts, r = [], None
        for i in range(reps + 1):
            t0 = time.perf_counter()
            r = fn()
            if i:
                ts.append((time.perf_counter() - t0) * 1e3)
        return dict(median=float(np.median(ts)), min=float(min(ts)), max=float(max(ts))), r

    def fresh_scores(e):
        e._scores = e._pd_vs = None
        return e.scores()

    row['construction_ms'], e = timed(lambda: ea.ObjPredErrors(im, pd, gt, obj_pred=pred, buffer_sz=0))
    row['scores_ms'], _ = timed(lambda: fresh_scores(e))
    for which in ('fn', 'fp'):
        row['gallery_%s_ms' % which], g = timed(lambda: e.gallery(which))
        row['gallery_%s_frames' % which] = int(g['rgb'].shape[0])
        del g
    print(json.dumps(row), flush=True)
    return row


def substacks_bench(ctx, torch, n_tbars=32768, reps=5, host_reps=2):
    """fplsynapses.roi_to_substacks on one 520^3 cube (448 + 2 x 36), radii 3 / 6: numpy against
    device=, the four kernels of libfplroi.so alone, and voxel_counts over a 4096^3 ROI's partition"""
    from flypylib_amd import _roicapi, fplsynapses, synth
    from flypylib_amd.roi import BlockRoi
    dev = torch.device('cuda', ctx.device)
    side, buf, n = 448, 36, 520
    vol = synth.em_volume_u8(3, (n, n, n))
    z, y, x = np.meshgrid(*[np.arange(14)] * 3, indexing='ij')
    roi = BlockRoi.from_block_mask((z - 6.5) ** 2 + (y - 6.5) ** 2 + (x - 6.5) ** 2 < 60.0)
    rs = np.random.RandomState(11)
    tbars = {'locs': rs.randint(0, side, (n_tbars, 3)).astype(np.int64), 'conf': rs.rand(n_tbars)}
    kw = dict(substack_ids=[0], image_normalize=[128.0, 33.0], buffer_size=buf, radius_use=3, radius_ign=6)
    row = dict(cube=[n, n, n], substack=side, buffer=buf, tbars=n_tbars, radius_use=3, radius_ign=6,
               roi_blocks=roi.n_blocks, roi_runs=len(roi.runs),
               timing='one warm-up, then median / min / max, ms (host: of %d, device: of %d); no files '
                      'written' % (host_reps, reps))

    def stats(ts):
        return dict(median=float(np.median(ts)), min=float(min(ts)), max=float(max(ts)))

    def timed(fn, sync, k):
        ts, r = [], None
        for i in range(k + 1):
            t0 = time.perf_counter()
            r = fn()
            if sync:
                torch.cuda.synchronize(dev)
            if i:
                ts.append((time.perf_counter() - t0) * 1e3)
        return stats(ts), r

    def export(source, device):
        import contextlib
        import io
        with contextlib.redirect_stdout(io.StringIO()):
            return fplsynapses.roi_to_substacks(source, None, roi, tbars, 14, device=device, **kw)[0]
    row['host_ms'], host = timed(lambda: export(vol, None), False, host_reps)
    row['device_from_host_ms'], got = timed(lambda: export(vol, ctx.device), True, reps)
    res = torch.from_numpy(vol).to(dev)
    row['device_resident_ms'], got_r = timed(lambda: export(res, ctx.device), True, reps)
    row['tbars_in_roi'] = int(len(host['tbars']['conf']))
    row['identical'] = bool(all(np.array_equal(host[k].view(np.uint8), got[k].cpu().numpy().view(np.uint8))
                                and torch.equal(got[k], got_r[k])
                                for k in ('image', 'roi_mask', 'labels', 'mask')))
    row['host_over_device_resident'] = row['host_ms']['median'] / row['device_resident_ms']['median']
    del host, got_r

    # the kernels alone, HIP events
    tables, stream = roi.device_tables(dev), torch.cuda.current_stream(dev).cuda_stream
    nr, nk, b = len(roi.row_keys), len(roi.runs), roi.block_size
    big = BlockRoi.from_block_mask((np.add.outer(np.add.outer((np.arange(128) - 63.5) ** 2,
                                                              (np.arange(128) - 63.5) ** 2),
                                                 (np.arange(128) - 63.5) ** 2)) < 62.0 ** 2)
    cubes = big.partition(16)[0]
    boxes = np.asarray([(s.z, s.y, s.x, s.size, s.size, s.size) for s in cubes], np.int64)
    big_tables, boxes_res = big.device_tables(dev), torch.from_numpy(boxes).to(dev)
    counts = torch.empty(len(boxes), dtype=torch.int64, device=dev)
    pts = torch.from_numpy(np.fliplr(tbars['locs']).copy()).to(dev)
    flags = torch.empty(n_tbars, dtype=torch.uint8, device=dev)
    image, mask = got['image'], got['roi_mask']
    kernels = {
        'mask_box': lambda: _roicapi.mask_box(tables, nr, nk, b, (-buf,) * 3, (n,) * 3, mask, stream),
        'cut_normalize_u8': lambda: _roicapi.cut_normalize_u8(res, (n,) * 3, (-buf,) * 3, (n,) * 3, 128.0,
                                                              33.0, image, stream),
        'ptquery': lambda: _roicapi.ptquery(tables, nr, nk, b, pts, n_tbars, flags, stream),
        'box_counts': lambda: _roicapi.box_counts(big_tables, len(big.row_keys), len(big.runs), 32,
                                                  boxes_res, len(boxes), counts, stream),
    }
    ms = {name: [] for name in kernels}
    for i in range(reps + 1):
        for name, fn in kernels.items():
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize(dev)
            if i:
                ms[name].append(e0.elapsed_time(e1))
    row['kernels_ms'] = {name: stats(v) for name, v in ms.items()}
    row['kernels_timing'] = ('HIP events around one call: mask_box and cut_normalize_u8 on the 520^3 '
                             'cube, ptquery on %d points, box_counts on the %d cubes of the 4096^3 '
                             "ROI's partition(16)" % (n_tbars, len(boxes)))
    row['kernels_bytes'] = {'mask_box': n ** 3, 'cut_normalize_u8': 5 * n ** 3}
    row['voxel_counts'] = dict(roi='a ball of %d blocks in 128^3 (4096^3 voxels), %d runs'
                                   % (big.n_blocks, len(big.runs)), cubes=len(boxes))
    row['voxel_counts']['host_ms'], want = timed(lambda: big.voxel_counts(boxes), False, reps)
    row['voxel_counts']['device_ms'], cnt = timed(lambda: big.voxel_counts(boxes, device=ctx.device), True,
                                                  reps)
    row['voxel_counts']['identical'] = bool(np.array_equal(want, cnt)
                                            and int(want.sum()) == big.n_blocks * 32 ** 3)
    print(json.dumps(row), flush=True)
    return row


def _unet_t_102(in_sz=None):
    """tests/deconv_cases.py's example U-Net at a production tile: 102 in, 96 out"""
    from tests import deconv_cases as dc
    return dc.tiny_unet_t_random((102,) * 3 if in_sz is None else in_sz)


def deconv_bench(ctx, torch, vol=390, reps=5):
    """the example U-Net with a Conv3DTranspose end to end, and the deconv kernel alone"""
    from flypylib_amd import FplNetwork, _capi
    from tests import deconv_cases as dc

    def stats(v):
        return {'median': round(float(np.median(v)), 4), 'min': round(float(min(v)), 4),
                'max': round(float(max(v)), 4)}

    def table():
        return {k: {'ms': round(v['ms'], 4), 'launches': int(v['launches'])}
                for k, v in sorted(ctx.timing_get().items(), key=lambda kv: -kv[1]['ms'])}
    out = {'reps': reps, 'note': 'one warm-up, then median / min / max of %d; resident source and '
                                 'destination; no gate: the path did not exist before' % reps}
    # ---- the U-Net over a volume -------------------------------------------------------------
    net = FplNetwork(_unet_t_102)
    net._set_infer()
    src = torch.from_numpy(np.random.default_rng(0).standard_normal((vol,) * 3).astype(np.float32)).to('cuda:0')
    dst = torch.empty((vol,) * 3, dtype=torch.float32, device='cuda:0')
    prog = net.infer_network.program
    legs = {}
    for leg, env in (('mfma_f32', None), ('perop_f32', '1')):
        if env:
            os.environ['FPL_FORCE_PEROP'] = env
        try:
            ms = []
            for r in range(reps + 1):
                ctx.synchronize()
                t0 = time.perf_counter()
                prog.infer_volume(src, net.infer_sz, net.rf_offset, precision=_capi.PREC_F32, dst=dst,
                                  dims=(vol,) * 3)
                ms.append((time.perf_counter() - t0) * 1e3)
            path = ctx.last_path()
            ctx.timing(True); ctx.timing_reset()
            prog.infer_volume(src, net.infer_sz, net.rf_offset, precision=_capi.PREC_F32, dst=dst, dims=(vol,) * 3)
            kern = table()
            ctx.timing(False)
        finally:
            os.environ.pop('FPL_FORCE_PEROP', None)
        legs[leg] = {'executor': path, 'ms': stats(ms[1:]), 'runs_ms': [round(x, 3) for x in ms[1:]],
                     'mvox_s': round(vol ** 3 / np.median(ms[1:]) / 1e3, 1), 'kernels_one_pass': kern}
        print(leg, json.dumps(legs[leg]['ms']), flush=True)
    out['tiny_unet_t_infer'] = {'volume': [vol] * 3, 'tile_in': 102, 'pitch': 96, 'legs': legs}
    # ---- its training step -------------------------------------------------------------------
    batch, patch = 8, 62
    g = dc.tiny_unet_t((patch,) * 3)[0]
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.standard_normal((batch,) + (patch,) * 3 + (1,)).astype(np.float32)).to('cuda:0')
    y = torch.from_numpy((rng.random((batch,) + (patch - 6,) * 3 + (1,)) < 0.3).astype(np.uint8)).to('cuda:0')
    tr = _capi.Trainer(ctx, g)
    ms = []
    for r in range(reps + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        tr.step(x, y, seed=r); tr.apply(1.0)
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ctx.timing(True); ctx.timing_reset()
    tr.step(x, y, seed=0); tr.apply(1.0)
    ctx.synchronize()
    kern = table()
    ctx.timing(False)
    tr.close()
    out['tiny_unet_t_train_step'] = {
        'batch': batch, 'patch': patch, 'ms': stats(ms[1:]), 'runs_ms': [round(v, 3) for v in ms[1:]],
        'note': 'fixed-order path: plain fp32 weight-gradient kernels for every convolution and the deconv',
        'kernels_one_step': kern}
    print('train', json.dumps(out['tiny_unet_t_train_step']['ms']), flush=True)
    # ---- the kernel alone ----------------------------------------------------------------------
    alone = {}
    for cin, cout, n, edge in ((16, 8, 8, 48), (48, 32, 2, 64), (96, 48, 2, 40)):
        g, _ = dc.deconv_graph(cin, cout, 1, 1, 1, (edge,) * 3)
        p = _capi.Program(ctx, g)
        xin = torch.randn((n,) + (edge,) * 3, device='cuda:0')
        yout = torch.empty((n,) + (2 * edge,) * 3 + (cout,), dtype=torch.float32, device='cuda:0')
        k_ms = []
        for r in range(reps + 1):
            ctx.timing(True); ctx.timing_reset()
            p.forward_device(xin, out=yout)
            t = ctx.timing_get()
            ctx.timing(False)
            k_ms.append(t['mfma_deconv2_f32']['ms'])
        p.close()
        wr = yout.numel() * 4
        rd = n * edge ** 3 * cin * 4
        a_, b_ = torch.empty(wr // 4, device='cuda:0'), torch.empty(wr // 4, device='cuda:0')
        c_ms = []
        for r in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            b_.copy_(a_)
            e1.record(); e1.synchronize()
            c_ms.append(e0.elapsed_time(e1))
        del a_, b_, xin, yout
        km, cm = float(np.median(k_ms[1:])), float(np.median(c_ms[1:]))
        alone['%dto%d_%dx%d' % (cin, cout, n, edge)] = {
            'input_voxels': n * edge ** 3, 'bytes_written': wr, 'bytes_read': rd,
            'kernel_ms': stats(k_ms[1:]), 'store_gb_s': round(wr / km / 1e6, 1),
            'd2d_copy_same_bytes_ms': stats(c_ms[1:]),
            'd2d_copy_gb_s_written': round(wr / cm / 1e6, 1),
            'kernel_over_copy': round(km / cm, 3)}
        print(json.dumps(alone['%dto%d_%dx%d' % (cin, cout, n, edge)]), flush=True)
    out['deconv_kernel_alone'] = alone
    out.update(deconv_gx_bench(ctx, torch, vol, reps, stats, table, alone))
    return out


def _unet_t3_102(in_sz=None):
    """tests/deconv_gx_cases.py's example U-Net (the graph executor takes it) at tile 102: 94 out"""
    from tests import deconv_gx_cases as gc
    return gc.unet_t3_random((102,) * 3 if in_sz is None else in_sz)


def deconv_gx_bench(ctx, torch, vol, reps, stats, table, alone):
    """the layer on the split-half graph executor: unet_t3 under 'auto' against precision 'f32' of the
    same network in the same process, and gx_deconv2 alone at the fp32 kernel's three shapes"""
    from flypylib_amd import FplNetwork, _capi
    from tests import deconv_gx_cases as gc
    net = FplNetwork(_unet_t3_102)
    net._set_infer()
    src = torch.from_numpy(np.random.default_rng(0).standard_normal((vol,) * 3).astype(np.float32)).to('cuda:0')
    dst = torch.empty((vol,) * 3, dtype=torch.float32, device='cuda:0')
    prog = net.infer_network.program
    legs = {}
    for leg, prec in (('auto', _capi.PREC_AUTO), ('f32', _capi.PREC_F32)):
        ms = []
        for r in range(reps + 1):
            ctx.synchronize()
            t0 = time.perf_counter()
            prog.infer_volume(src, net.infer_sz, net.rf_offset, precision=prec, dst=dst, dims=(vol,) * 3)
            ms.append((time.perf_counter() - t0) * 1e3)
        path = ctx.last_path()
        ctx.timing(True); ctx.timing_reset()
        prog.infer_volume(src, net.infer_sz, net.rf_offset, precision=prec, dst=dst, dims=(vol,) * 3)
        kern = table()
        ctx.timing(False)
        legs[leg] = {'executor': path, 'ms': stats(ms[1:]), 'runs_ms': [round(x, 3) for x in ms[1:]],
                     'mvox_s': round(vol ** 3 / np.median(ms[1:]) / 1e3, 1), 'kernels_one_pass': kern}
        print('unet_t3', leg, path, json.dumps(legs[leg]['ms']), flush=True)
    res = {'unet_t3_infer': {
        'volume': [vol] * 3, 'tile_in': 102, 'pitch': 94, 'legs': legs,
        'f32_over_auto': round(legs['f32']['ms']['median'] / legs['auto']['ms']['median'], 3)}}
    del src, dst
    # ---- gx_deconv2 alone: the layer behind a first layer and a pool, n tiles of edge^3 input voxels ------
    rows = {}
    for cin, cout, n, edge in ((16, 8, 8, 48), (48, 32, 2, 64), (96, 48, 2, 40)):
        g, off = gc.layer_alone(cin, cout, 1, 'relu', edge=edge)
        tile = gc.tile_of(cin, edge)
        p = _capi.Program(ctx, g, (1, 1, 1))
        shape = (n * (tile - 2 * off) + 2 * off, tile, tile)
        u8 = np.random.default_rng(1).integers(0, 256, shape, dtype=np.uint8)     # (kernel times only: a host source)
        row = {'input_voxels': n * edge ** 3}
        for kind, prec in (('f16s', _capi.PREC_F16S), ('f16', _capi.PREC_F16)):
            k_ms = []
            for r in range(reps + 1):
                ctx.timing(True); ctx.timing_reset()
                p.infer_volume(u8, (tile,) * 3, (off,) * 3, mean=128.0, std=33.0, precision=prec)
                t = ctx.timing_get()
                ctx.timing(False)
                k_ms.append(t['gx_deconv2']['ms'])
            wr = n * (2 * edge) ** 3 * ((cout + 31) // 32 * 32) * (4 if kind == 'f16s' else 2)
            row[kind] = {'executor': ctx.last_path(), 'kernel_ms': stats(k_ms[1:]), 'bytes_written': wr,
                         'store_gb_s': round(wr / float(np.median(k_ms[1:])) / 1e6, 1)}
        f32 = alone.get('%dto%d_%dx%d' % (cin, cout, n, edge))
        if f32:
            row['f32_kernel_over_f16s'] = round(f32['kernel_ms']['median'] / row['f16s']['kernel_ms']['median'], 3)
        p.close()
        rows['%dto%d_%dx%d' % (cin, cout, n, edge)] = row
        print('gx_deconv2', cin, cout, json.dumps(row), flush=True)
    res['gx_deconv2_alone'] = rows
    return res


def down_bench(ctx, torch, vol=390, reps=5):
    """the example network with a Conv3D(filters, 2, strides=2) end to end, and the kernel alone
    beside a device copy of the bytes it reads and beside MaxPooling3D(2) of the same input"""
    from flypylib_amd import FplNetwork, _capi
    from flypylib_amd.program import LayerGraph
    from tests import down_cases as dn

    def stats(v):
        return {'median': round(float(np.median(v)), 4), 'min': round(float(min(v)), 4),
                'max': round(float(max(v)), 4)}

    def table():
        return {k: {'ms': round(v['ms'], 4), 'launches': int(v['launches'])}
                for k, v in sorted(ctx.timing_get().items(), key=lambda kv: -kv[1]['ms'])}
    out = {'reps': reps, 'note': 'one warm-up, then median / min / max of %d; resident source and '
                                 'destination; no gate: the path did not exist before' % reps}
    # ---- tiny_vnet over a volume -------------------------------------------------------------
    net = FplNetwork(lambda in_sz=None: dn.tiny_vnet_random((102,) * 3 if in_sz is None else in_sz))
    net._set_infer()
    src = torch.from_numpy(np.random.default_rng(0).standard_normal((vol,) * 3).astype(np.float32)).to('cuda:0')
    dst = torch.empty((vol,) * 3, dtype=torch.float32, device='cuda:0')
    prog = net.infer_network.program
    kw = dict(precision=_capi.PREC_F32, dst=dst, dims=(vol,) * 3)
    ms = []
    for r in range(reps + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        prog.infer_volume(src, net.infer_sz, net.rf_offset, **kw)
        ms.append((time.perf_counter() - t0) * 1e3)
    path = ctx.last_path()
    ctx.timing(True); ctx.timing_reset()
    prog.infer_volume(src, net.infer_sz, net.rf_offset, **kw)
    kern = table()
    ctx.timing(False)
    out['tiny_vnet_infer'] = {'volume': [vol] * 3, 'tile_in': 102, 'pitch': 96, 'executor': path,
                              'ms': stats(ms[1:]), 'runs_ms': [round(x, 3) for x in ms[1:]],
                              'mvox_s': round(vol ** 3 / np.median(ms[1:]) / 1e3, 1), 'kernels_one_pass': kern}
    print('infer', json.dumps(out['tiny_vnet_infer']['ms']), flush=True)
    del src, dst
    # ---- its training step -------------------------------------------------------------------
    batch, patch = 8, 62
    g = dn.tiny_vnet((patch,) * 3)[0]
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.standard_normal((batch,) + (patch,) * 3 + (1,)).astype(np.float32)).to('cuda:0')
    y = torch.from_numpy((rng.random((batch,) + (patch - 6,) * 3 + (1,)) < 0.3).astype(np.uint8)).to('cuda:0')
    tr = _capi.Trainer(ctx, g)
    ms = []
    for r in range(reps + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        tr.step(x, y, seed=r); tr.apply(1.0)
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ctx.timing(True); ctx.timing_reset()
    tr.step(x, y, seed=0); tr.apply(1.0)
    ctx.synchronize()
    kern = table()
    ctx.timing(False)
    tr.close()
    out['tiny_vnet_train_step'] = {
        'batch': batch, 'patch': patch, 'ms': stats(ms[1:]), 'runs_ms': [round(v, 3) for v in ms[1:]],
        'note': 'the network holds a Conv3DTranspose too: fixed-order weight gradients for every convolution',
        'kernels_one_step': kern}
    print('train', json.dumps(out['tiny_vnet_train_step']['ms']), flush=True)
    del x, y
    # ---- the kernel alone ----------------------------------------------------------------------
    def kernel_ms(graph, xin, yshape, name):
        p = _capi.Program(ctx, graph)
        yout = torch.empty(yshape, dtype=torch.float32, device='cuda:0')
        v = []
        for r in range(reps + 1):
            ctx.timing(True); ctx.timing_reset()
            p.forward_device(xin, out=yout)
            t = ctx.timing_get()
            ctx.timing(False)
            v.append(t[name]['ms'])
        p.close()
        return v[1:]
    alone = {}
    for cin, cout, n, edge in ((16, 32, 8, 96), (48, 64, 2, 96), (96, 128, 2, 80)):
        xin = torch.randn((n,) + (edge,) * 3, device='cuda:0')
        g, _ = dn.down_graph(cin, cout, 1, 1, 1, (edge,) * 3)
        k_ms = kernel_ms(g, xin, (n,) + (edge // 2,) * 3 + (cout,), 'mfma_down2_f32')
        pg = LayerGraph((edge,) * 3)
        pg.finish(pg.pool(pg.conv(pg.input(), cin, 1, use_bias=True)))
        p_ms = kernel_ms(pg, xin, (n,) + (edge // 2,) * 3 + (cin,), 'mfma_pool_f32')
        rd = n * edge ** 3 * cin * 4
        wr = n * (edge // 2) ** 3 * cout * 4
        a_, b_ = torch.empty(rd // 4, device='cuda:0'), torch.empty(rd // 4, device='cuda:0')
        c_ms = []
        for r in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            b_.copy_(a_)
            e1.record(); e1.synchronize()
            c_ms.append(e0.elapsed_time(e1))
        del a_, b_, xin
        km, pm, cm = float(np.median(k_ms)), float(np.median(p_ms)), float(np.median(c_ms[1:]))
        key = '%dto%d_%dx%d' % (cin, cout, n, edge)
        alone[key] = {
            'output_voxels': n * (edge // 2) ** 3, 'bytes_read': rd, 'bytes_written': wr,
            'kernel_ms': stats(k_ms), 'load_gb_s': round(rd / km / 1e6, 1),
            'd2d_copy_of_the_bytes_read_ms': stats(c_ms[1:]), 'kernel_over_copy': round(km / cm, 3),
            'maxpool_same_input_ms': stats(p_ms), 'kernel_over_maxpool': round(km / pm, 3)}
        print(key, json.dumps(alone[key]), flush=True)
    out['down_kernel_alone'] = alone
    return out


def dilated_bench(ctx, torch, vol=390, reps=5):
    """the example network with two Conv3D(filters, 3, dilation_rate=2) end to end, its training
    step, and the kernel alone beside the plain conv3_f32 at the same widths and output count
    (the same flops, and a kernel this project has measured)"""
    from flypylib_amd import FplNetwork, _capi
    from flypylib_amd.program import LayerGraph
    from tests import dilated_cases as di

    def stats(v):
        return {'median': round(float(np.median(v)), 4), 'min': round(float(min(v)), 4),
                'max': round(float(max(v)), 4)}

    def table():
        return {k: {'ms': round(v['ms'], 4), 'launches': int(v['launches'])}
                for k, v in sorted(ctx.timing_get().items(), key=lambda kv: -kv[1]['ms'])}
    out = {'reps': reps, 'note': 'one warm-up, then median / min / max of %d; resident source and '
                                 'destination; no gate: the path did not exist before' % reps}
    # ---- tiny_atrous over a volume: tile 105, pitch 95, 4 tiles per axis of 390 ----------------
    tile = 105
    net = FplNetwork(lambda in_sz=None: di.tiny_atrous_random((tile,) * 3 if in_sz is None else in_sz))
    net._set_infer()
    src = torch.from_numpy(np.random.default_rng(0).standard_normal((vol,) * 3).astype(np.float32)).to('cuda:0')
    dst = torch.empty((vol,) * 3, dtype=torch.float32, device='cuda:0')
    prog = net.infer_network.program
    kw = dict(precision=_capi.PREC_F32, dst=dst, dims=(vol,) * 3)
    ms = []
    for r in range(reps + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        prog.infer_volume(src, net.infer_sz, net.rf_offset, **kw)
        ms.append((time.perf_counter() - t0) * 1e3)
    path = ctx.last_path()
    ctx.timing(True); ctx.timing_reset()
    prog.infer_volume(src, net.infer_sz, net.rf_offset, **kw)
    kern = table()
    ctx.timing(False)
    out['tiny_atrous_infer'] = {'volume': [vol] * 3, 'tile_in': tile, 'pitch': tile - 10, 'executor': path,
                                'ms': stats(ms[1:]), 'runs_ms': [round(x, 3) for x in ms[1:]],
                                'mvox_s': round(vol ** 3 / np.median(ms[1:]) / 1e3, 1), 'kernels_one_pass': kern}
    print('infer', json.dumps(out['tiny_atrous_infer']['ms']), flush=True)
    del src, dst
    # ---- its training step -------------------------------------------------------------------
    batch, patch = 8, 62
    g = di.tiny_atrous((patch,) * 3)[0]
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.standard_normal((batch,) + (patch,) * 3 + (1,)).astype(np.float32)).to('cuda:0')
    y = torch.from_numpy((rng.random((batch,) + (patch - 10,) * 3 + (1,)) < 0.3).astype(np.uint8)).to('cuda:0')
    tr = _capi.Trainer(ctx, g)
    ms = []
    for r in range(reps + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        tr.step(x, y, seed=r); tr.apply(1.0)
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ctx.timing(True); ctx.timing_reset()
    tr.step(x, y, seed=0); tr.apply(1.0)
    ctx.synchronize()
    kern = table()
    ctx.timing(False)
    tr.close()
    out['tiny_atrous_train_step'] = {
        'batch': batch, 'patch': patch, 'ms': stats(ms[1:]), 'runs_ms': [round(v, 3) for v in ms[1:]],
        'note': 'direct fp32 kernels for the layer; fixed-order weight gradients for every convolution',
        'kernels_one_step': kern}
    print('train', json.dumps(out['tiny_atrous_train_step']['ms']), flush=True)
    del x, y
    # ---- the kernel alone, beside the plain 3x3x3 ---------------------------------------------
    def kernel_ms(graph, xin, yshape, name):
        p = _capi.Program(ctx, graph)
        yout = torch.empty(yshape, dtype=torch.float32, device='cuda:0')
        v = []
        for r in range(reps + 1):
            ctx.timing(True); ctx.timing_reset()
            p.forward_device(xin, out=yout)
            t = ctx.timing_get()
            ctx.timing(False)
            v.append(t[name]['ms'])
        p.close()
        return v[1:]
    alone = {}
    for cin, cout, n, edge in ((16, 16, 8, 100), (48, 48, 2, 100), (96, 32, 2, 84)):
        oe = edge - 4
        xin = torch.randn((n,) + (edge,) * 3, device='cuda:0')
        g, _ = di.dilated_graph(cin, cout, 1, 1, 1, (edge,) * 3)
        k_ms = kernel_ms(g, xin, (n,) + (oe,) * 3 + (cout,), 'mfma_atrous3_f32')
        # the comparator: conv1(1 -> cin) | conv3(cin -> cout) BN ReLU on an input two voxels
        # smaller, so that both kernels write (edge - 4)^3 voxels
        pg = LayerGraph((edge - 2,) * 3)
        pg.finish(pg.conv_bn_relu(pg.conv(pg.input(), cin, 1, use_bias=True), cout, 3))
        di.randomize(pg, 1)
        p_ms = kernel_ms(pg, xin[:, :edge - 2, :edge - 2, :edge - 2].contiguous(), (n,) + (oe,) * 3 + (cout,),
                         'mfma_conv3_f32')
        del xin
        km, pm = float(np.median(k_ms)), float(np.median(p_ms))
        flop = 2.0 * n * oe ** 3 * 27 * cin * cout
        key = '%dto%d_%dx%d' % (cin, cout, n, edge)
        alone[key] = {'output_voxels': n * oe ** 3, 'flop': flop, 'kernel_ms': stats(k_ms),
                      'tflops': round(flop / km / 1e9, 2), 'conv3_f32_same_outputs_ms': stats(p_ms),
                      'conv3_f32_tflops': round(flop / pm / 1e9, 2), 'kernel_over_conv3_f32': round(km / pm, 3)}
        print(key, json.dumps(alone[key]), flush=True)
    out['atrous_kernel_alone'] = alone
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mine-size', type=int, default=520)
    ap.add_argument('--what', default='unet,train,v2o,pipeline')
    ap.add_argument('--clahe-size', type=int, default=520)
    ap.add_argument('--unet-size', type=int, default=264)
    ap.add_argument('--roi-precision', default='auto')
    ap.add_argument('--vgg2-size', type=int, default=1024)
    ap.add_argument('--sub', type=int, default=582)
    ap.add_argument('--roi-size', type=int, default=1536)
    ap.add_argument('--roi-source', default='synth', choices=['synth', 'resident'],
                    help="roi: 'synth' generates every substack + buffer on the device inside the timed "
                         "region (the stand-in for the reference's DVID fetch); 'resident' keeps the whole "
                         "volume in HBM (generated before the clock starts) and cuts the substacks out of it")
    ap.add_argument('--roi-seg', default='none', choices=['none', 'host', 'resident'],
                    help="roi: run the segmentation-aware post-processing on a synthetic label volume (blocks of "
                         "32^3 hashed to 8-byte ids): 'host' hands it over as a host array and keeps it there "
                         "(FPL_PIPE_RESIDENT_GB=0: a label cube is cut and uploaded per substack), 'resident' as "
                         "a device tensor; the CPU oracle check is skipped (it takes minutes per substack)")
    ap.add_argument('--skip-oracle', action='store_true',
                    help='roi: do not re-derive one substack on the CPU oracle (for traces)')
    ap.add_argument('--dedupe-reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from flypylib_amd import _capi, fplmodels, fplobjdetect, runtime, synth
    ctx = runtime.get_context(0)      # the context voxel2obj uses as well
    res = {'device': ctx.device_info()['name']}
    what = a.what.split(',')

    if 'unet' in what:
        g = fplmodels.unet_like2(100)[0]
        synth.synthetic_weights(g, 7)
        prog = _capi.Program(ctx, g, (1, 1, 1))
        n = a.unet_size
        src = torch.empty((n, n, n), dtype=torch.uint8, device='cuda')
        dst = torch.empty((n, n, n), dtype=torch.float32, device='cuda')
        ctx.synth_volume_u8(3, (n, n, n), out=src)
        for pname, prec in (('bf16_mfma', _capi.PREC_BF16), ('f16_mfma', _capi.PREC_F16),
                            ('f16s_split', _capi.PREC_F16S), ('f32_mfma', _capi.PREC_F32)):
            kw = dict(mean=128.0, std=33.0, precision=prec, dst=dst, dims=(n, n, n))
            prog.infer_volume(src, (100,) * 3, (9,) * 3, **kw)
            ctx.synchronize()
            ctx.timing(True); ctx.timing_reset()
            t0 = time.perf_counter()
            prog.infer_volume(src, (100,) * 3, (9,) * 3, **kw)
            ctx.synchronize()
            dt = time.perf_counter() - t0
            vox = (n - 18) ** 3
            res['unet_like2_' + pname] = dict(
                volume=n, mvox_s=vox / dt / 1e6, seconds=dt,
                tflops_algorithmic=vox * 350720 / dt / 1e12,
                kernels={k: round(v['ms'], 2) for k, v in ctx.timing_get().items()})
            ctx.timing(False)
            print(json.dumps(res['unet_like2_' + pname]), flush=True)

    if 'graphs' in what:
        # the four factories of the graph executor (csrc/gx_exec.h) at their own infer_sz, a volume of
        # 5 - 7 tiles per axis: 'auto' (split halves, op by op) against the fp32 MFMA executor
        from flypylib_amd import fplutils
        for name, tiles in (('baseline_model', 6), ('resnet_like', 6), ('unet_like4b', 7), ('unet_like_vol', 5)):
            factory = getattr(fplmodels, name)
            _, rf, infer_sz, _ = factory()
            tile = fplutils.to3d(infer_sz)[0]
            off = fplutils.to3d(rf[1])[0]
            stride = fplutils.to3d(rf[2])
            g = factory(tile)[0]
            synth.synthetic_weights(g, 7)
            prog = _capi.Program(ctx, g, stride)
            n = tiles * (tile - 2 * off) + 2 * off
            src = torch.empty((n, n, n), dtype=torch.uint8, device='cuda')
            dst = torch.empty((n, n, n), dtype=torch.float32, device='cuda')
            ctx.synth_volume_u8(3, (n, n, n), out=src)
            for pname, prec in (('auto', _capi.PREC_AUTO), ('f16', _capi.PREC_F16), ('f32', _capi.PREC_F32)):
                kw = dict(mean=128.0, std=33.0, precision=prec, dst=dst, dims=(n, n, n))
                prog.infer_volume(src, (tile,) * 3, (off,) * 3, **kw)
                ctx.synchronize()
                ctx.timing(True); ctx.timing_reset()
                t0 = time.perf_counter()
                prog.infer_volume(src, (tile,) * 3, (off,) * 3, **kw)
                ctx.synchronize()
                dt = time.perf_counter() - t0
                key = '%s_%s' % (name, pname)
                res[key] = dict(volume=n, tile=tile, executor=ctx.last_path(), seconds=dt,
                                mvox_s=(n - 2 * off) ** 3 / dt / 1e6,
                                kernels={k: round(v['ms'], 2) for k, v in ctx.timing_get().items()})
                ctx.timing(False)
                print(key, json.dumps(res[key]), flush=True)
            del src, dst

    if 'vgg2' in what:
        # vgg_like2 (scripts/fpl_cx1_0_vgg_4ss.py): 5 x conv3, 159 867 FLOP per output voxel
        g = fplmodels.vgg_like2(100)[0]
        synth.synthetic_weights(g, 8)
        prog = _capi.Program(ctx, g, (4, 4, 4))
        n = a.vgg2_size
        src = torch.empty((n, n, n), dtype=torch.uint8, device='cuda')
        dst = torch.empty((n, n, n), dtype=torch.float32, device='cuda')
        ctx.synth_volume_u8(4, (n, n, n), out=src)
        flop = 2 * (27 * 48 + 27 * 48 * 48 + (2 * 27 * 48 * 48) / 8 + (27 * 48 * 48 + 48 * 96 + 96 * 96 + 96) / 64)
        for pname, prec in (('f16s', _capi.PREC_F16S), ('f16', _capi.PREC_F16), ('bf16', _capi.PREC_BF16),
                            ('f32', _capi.PREC_F32)):
            kw = dict(mean=128.0, std=33.0, precision=prec, dst=dst, dims=(n, n, n))
            prog.infer_volume(src, (100,) * 3, (10,) * 3, **kw)
            ctx.synchronize()
            ctx.timing(True); ctx.timing_reset()
            t0 = time.perf_counter()
            prog.infer_volume(src, (100,) * 3, (10,) * 3, **kw)
            ctx.synchronize()
            dt = time.perf_counter() - t0
            vox = (n - 20) ** 3
            res['vgg_like2_' + pname] = dict(
                volume=n, mvox_s=vox / dt / 1e6, seconds=dt, tflops_algorithmic=vox * flop / dt / 1e12,
                kernels={k: round(v['ms'], 2) for k, v in ctx.timing_get().items()})
            ctx.timing(False)
            print(json.dumps(res['vgg_like2_' + pname]), flush=True)

    if 'train' in what:
        g = fplmodels.vgg_like()[0]
        synth.synthetic_weights(g, 8)
        tr = _capi.Trainer(ctx, g)
        rng = np.random.default_rng(0)
        data = rng.standard_normal((32, 64, 64, 64)).astype(np.float32)
        labels = (rng.random((32, 12, 12, 12)) > 0.9).astype(np.uint8)
        # the loop of train.fit_generator (bench.py's leg): the prefetch worker uploads the next
        # batch while the step runs; 20 steps without per-kernel events, then 5 with
        from flypylib_amd import train as fpl_train

        def forever():
            while True:
                yield data, labels
        batches = fpl_train._Prefetch(forever(), stage=fpl_train._DeviceStager(ctx.device))
        tr.step(*next(batches), 0); tr.apply(1.0)
        ctx.synchronize()
        t0 = time.perf_counter()
        steps = 20
        for s in range(steps):
            tr.step(*next(batches), s + 1); tr.apply(1.0)
        ctx.synchronize()
        dt = (time.perf_counter() - t0) / steps
        ctx.timing(True); ctx.timing_reset()
        for s in range(5):
            tr.step(*next(batches), steps + s + 1); tr.apply(1.0)
        ctx.synchronize()
        kern = ctx.timing_get()
        ctx.timing(False)
        batches.close()
        t0 = time.perf_counter()
        for s in range(5):
            tr.step(data, labels, s + 1); tr.apply(1.0)
        ctx.synchronize()
        dt_host = (time.perf_counter() - t0) / 5
        res['vgg_train_b32_64cubed_f32'] = dict(
            seconds_per_step=dt, steps_per_s=1 / dt, steps_per_s_host_arrays=1 / dt_host,
            tflops_algorithmic=492e9 / dt / 1e12,
            note='fit_generator loop (upload of the next batch overlaps the step); '
                 'steps_per_s_host_arrays = the step fed host arrays directly, H2D inside',
            kernels={k: round(v['ms'] / 5, 2) for k, v in kern.items()})
        print(json.dumps(res['vgg_train_b32_64cubed_f32']), flush=True)

    if 'train_unet' in what:
        # unet_like2 as scripts/fpl_cx1_0_unet_4ss_all.py trains it: rf-sized 24^3 patches,
        # batch 64 per GPU, masked focal loss
        g = fplmodels.unet_like2()[0]
        synth.synthetic_weights(g, 3)
        tr = _capi.Trainer(ctx, g, loss='masked_focal_loss')
        rng = np.random.default_rng(0)
        data = rng.standard_normal((64, 24, 24, 24, 1)).astype(np.float32)
        labels = rng.integers(0, 3, (64, 6, 6, 6, 1)).astype(np.uint8)
        tr.step(data, labels, 0); tr.apply(1.0)
        ctx.synchronize()
        # wall clock over 20 steps WITHOUT per-kernel events (this step is ~150 small launches: the events
        # of the table below cost a fifth of it) ...
        t0 = time.perf_counter()
        for s in range(20):
            tr.step(data, labels, s + 1); tr.apply(1.0)
        ctx.synchronize()
        dt = (time.perf_counter() - t0) / 20
        # ... then the per-kernel table of 5 more
        ctx.timing(True); ctx.timing_reset()
        t0 = time.perf_counter()
        steps = 5
        for s in range(steps):
            tr.step(data, labels, s + 21); tr.apply(1.0)
        ctx.synchronize()
        dt_ev = (time.perf_counter() - t0) / steps
        res['unet_train_b64_24cubed_f32'] = dict(
            seconds_per_step=dt, steps_per_s=1 / dt, seconds_per_step_with_kernel_events=dt_ev,
            note='includes H2D of the batch',
            kernels={k: round(v['ms'] / steps, 3) for k, v in ctx.timing_get().items()})
        ctx.timing(False)
        print(json.dumps(res['unet_train_b64_24cubed_f32']), flush=True)

    if 'mine' in what:
        res['mine'] = mine_bench(ctx, torch, a.mine_size)
        if a.out is None:
            a.out = os.path.join(ROOT, 'profiles', 'mine.json')

    if 'match' in what:
        res['match'] = match_bench(ctx, torch)
        if a.out is None:
            a.out = os.path.join(ROOT, 'profiles', 'match.json')

    if 'dedupe' in what:
        res['dedupe'] = dedupe_bench(ctx, torch, reps=a.dedupe_reps)
        if a.out is None:
            a.out = os.path.join(ROOT, 'profiles', 'dedupe.json')

    if 'labels' in what:
        res['labels'] = labels_bench(ctx, torch)
        if a.out is None:
            a.out = os.path.join(ROOT, 'profiles', 'labels.json')

    if 'train_vol' in what:
        res['train_vol'] = train_vol(ctx)
        print(json.dumps(res['train_vol']), flush=True)
        if a.out is None:
            a.out = os.path.join(ROOT, 'profiles', 'train_vol.json')

    if 'validate' in what:
        res['validate'] = validate_bench(ctx, torch)
        if a.out is None:
            a.out = os.path.join(ROOT, 'profiles', 'validate.json')

    if 'clahe' in what:
        res['clahe'] = clahe_bench(ctx, torch, a.clahe_size)
        if a.out is None:
            a.out = os.path.join(ROOT, 'profiles', 'clahe.json')

    if 'errors' in what:
        res['errors'] = errors_bench()
        if a.out is None:
            a.out = os.path.join(ROOT, 'profiles', 'errors.json')

    if 'substacks' in what:
        res['substacks'] = substacks_bench(ctx, torch)
        if a.out is None:
            a.out = os.path.join(ROOT, 'profiles', 'substacks.json')

    if 'deconv' in what:
        res['deconv'] = deconv_bench(ctx, torch)
        if a.out is None:
            a.out = os.path.join(ROOT, 'profiles', 'deconv.json')

    if 'down' in what:
        res['down'] = down_bench(ctx, torch)
        if a.out is None:
            a.out = os.path.join(ROOT, 'profiles', 'down.json')

    if 'dilated' in what:
        res['dilated'] = dilated_bench(ctx, torch)
        if a.out is None:
            a.out = os.path.join(ROOT, 'profiles', 'dilated.json')

    if 'train_gen' in what:
        res['train_gen'] = train_gen(ctx, torch)
        print(json.dumps(res['train_gen']), flush=True)

    if 'v2o' in what or 'pipeline' in what:
        n = a.sub
        g = fplmodels.vgg_like(102)[0]
        synth.synthetic_weights(g, 9)
        prog = _capi.Program(ctx, g, (4, 4, 4))
        src = torch.empty((n, n, n), dtype=torch.uint8, device='cuda')
        pred = torch.empty((n, n, n), dtype=torch.float32, device='cuda')
        ctx.synth_volume_u8(5, (n, n, n), out=src)
        kw = dict(mean=128.0, std=33.0, precision=_capi.PREC_BF16, dst=pred, dims=(n, n, n))
        prog.infer_volume(src, (102,) * 3, (7,) * 3, **kw)
        ctx.synchronize()
        t0 = time.perf_counter()
        prog.infer_volume(src, (102,) * 3, (7,) * 3, **kw)
        ctx.synchronize()
        t_inf = time.perf_counter() - t0
        # blob-like probabilities make the NMS meaningful: add planted blobs
        prob = synth.blob_prob_volume(11, (n, n, n), period=64, radius=9.0)
        prob_dev = torch.from_numpy(prob).cuda()
        fplobjdetect.voxel2obj(prob_dev, 27, 5, (0, 0, 0), 35, 0.1)      # warm-up
        ctx.timing(True); ctx.timing_reset()
        t0 = time.perf_counter()
        out, info = fplobjdetect.voxel2obj(prob_dev, 27, 5, (0, 0, 0), 35, 0.1,
                                           return_info=True)
        t_v2o = time.perf_counter() - t0
        kern = {k: round(v['ms'], 2) for k, v in ctx.timing_get().items()}
        ctx.timing(False)
        padded = (n + 54) ** 3
        res['voxel2obj_sub%d' % n] = dict(
            seconds=t_v2o, mvox_s=n ** 3 / t_v2o / 1e6, detections=len(out['conf']),
            rounds=info['rounds'], gb_s_algorithmic=12 * padded / t_v2o / 1e9,
            kernels=kern)
        res['infer_sub%d_bf16' % n] = dict(seconds=t_inf,
                                           mvox_s=(n - 14) ** 3 / t_inf / 1e6)
        print(json.dumps(res['voxel2obj_sub%d' % n]), flush=True)
        if 'pipeline' in what:
            from oracle import voxel2obj_oracle
            t0 = time.perf_counter()
            ref = voxel2obj_oracle.voxel2obj(prob, 27, 5, (0, 0, 0), 35, 0.1)
            t_cpu = time.perf_counter() - t0
            same = (np.array_equal(ref['locs'], out['locs'])
                    and np.array_equal(ref['conf'], out['conf']))
            res['pipeline_sub%d' % n] = dict(
                infer_s=t_inf, v2o_s=t_v2o, total_mvox_s=n ** 3 / (t_inf + t_v2o) / 1e6,
                detections_identical_to_cpu_oracle=bool(same),
                cpu_oracle_v2o_s=t_cpu, cpu_oracle_mvox_s=n ** 3 / t_cpu / 1e6)
            print(json.dumps(res['pipeline_sub%d' % n]), flush=True)
    if 'roi' in what:
        # configs[4] end to end on one GPU: full_roi_inference over a synthetic
        # volume cut into 512-substacks + 35 buffer (582^3 cubes), bf16, r 27, sigma 5
        import pickle
        import shutil
        import tempfile
        from flypylib_amd import FplNetwork
        from oracle import voxel2obj_oracle
        n = a.roi_size
        # --roi-precision: 'auto' = the package's default (split halves for vgg_like)
        net = FplNetwork(fplmodels.vgg_like, precision=a.roi_precision)
        synth.synthetic_weights(net.train_single, 9)
        net._set_infer()
        wd = tempfile.mkdtemp(prefix='fri_')
        src = 'synth://5,%d,%d,%d' % (n, n, n)
        fplobjdetect.gen_full_tab_roi(wd + '/roi', src, None, step_size=512)
        roi = fplobjdetect.roi_from_txt(wd + '/roi_00.txt')[0]
        norm = [128., 33., 0.5]
        if a.roi_source == 'resident':
            # the same voxels, made once and kept in HBM: inputs resident when the timed region starts
            resident = torch.empty((n, n, n), dtype=torch.uint8, device='cuda')
            ctx.synth_volume_u8(5, (n, n, n), out=resident)
            torch.cuda.synchronize()
            src = resident
        seg_kw = {}
        if a.roi_seg != 'none':
            # blocks of (z // 32, y // 32, x // 32) hashed to 8-byte ids, made on the device plane by plane
            labels = torch.empty((n, n, n), dtype=torch.int64, device='cuda')
            ax = torch.arange(n, dtype=torch.int64, device='cuda') // 32
            plane = (ax[:, None] * 19349663) ^ (ax[None, :] * 83492791)
            for bz in range(0, n, 32):
                labels[bz:bz + 32] = (((plane ^ (bz // 32 * 73856093)) + 1) * -7046029254386353131)[None]
            torch.cuda.synchronize()
            if a.roi_seg == 'host':
                host_labels = labels.cpu().numpy().view(np.uint64)
                del labels
                torch.cuda.empty_cache()
                os.environ['FPL_PIPE_RESIDENT_GB'] = '0'
                seg_kw = dict(dvid_seg_info=host_labels)
            else:
                seg_kw = dict(dvid_seg_info=labels)
        fplobjdetect.full_roi_inference(src, None, roi[:6], net, 0.1, wd + '/warm', norm, **seg_kw)
        ctx.timing(True); ctx.timing_reset()
        t0 = time.perf_counter()
        out = fplobjdetect.full_roi_inference(src, None, wd + '/roi_00.txt', net, 0.1,
                                              wd + '/work', norm, **seg_kw)
        dt = time.perf_counter() - t0
        # (lane 0's inference kernels only: HIP events on the six concurrent streams of the pipeline time the
        # waits for one another, not execution - the kernel table of ALL lanes is the rocprofv3 kernel trace of
        # this run, profiles/r05_roi1536_kernel_stats.csv)
        kern = {k: round(v['ms'], 2) for k, v in ctx.timing_get().items()}
        ctx.timing(False)
        if a.skip_oracle or a.roi_seg != 'none':
            print(json.dumps(dict(substacks=len(roi), seconds=dt, mvox_s=n ** 3 / dt / 1e6, seg=a.roi_seg,
                                  source=a.roi_source, detections=int(len(out['conf'])))), flush=True)
            shutil.rmtree(wd, ignore_errors=True)
            return
        # one substack re-derived and post-processed by the CPU oracle
        ss = roi[len(roi) // 2]
        sz = ss.size + 70
        cube = ctx.malloc((sz,) * 3, np.uint8)
        pred = ctx.malloc((sz,) * 3, np.float32)
        ctx.synth_substack_u8(5, (n, n, n), (sz,) * 3, [ss.z - 35, ss.y - 35, ss.x - 35], cube)
        from flypylib_amd import fplpipeline
        st = fplpipeline.normalisation_from_histogram(ctx.histogram_u8(cube), norm)
        net.infer_network.program.infer_volume(cube, net.infer_sz, net.rf_offset, mean=st['mn_use'],
                                               std=norm[1],
                                               precision=fplpipeline.fplobjdetect_precision(net, None),
                                               dst=pred, dims=(sz,) * 3)
        t0 = time.perf_counter()
        ref = voxel2obj_oracle.voxel2obj(pred.to_host(), 27, 5, (ss.x - 35, ss.y - 35, ss.z - 35), 35, 0.1)
        t_cpu = time.perf_counter() - t0
        got = pickle.load(open(fplobjdetect.fri_filename(wd + '/work', ss), 'rb'))
        same = np.array_equal(ref['locs'], got['locs']) and np.array_equal(ref['conf'], got['conf'])
        res['full_roi_inference_%d' % n] = dict(
            precision=a.roi_precision, source=a.roi_source, executor=ctx.last_path(),
            substacks=len(roi), seconds=dt, mvox_s=n ** 3 / dt / 1e6,
            detections=int(len(out['conf'])), checked_substack=list(ss),
            checked_substack_detections=int(len(got['conf'])),
            detections_identical_to_cpu_oracle=bool(same), cpu_oracle_v2o_s=t_cpu,
            kernel_ms_total=kern)
        print(json.dumps(res['full_roi_inference_%d' % n]), flush=True)
        shutil.rmtree(wd, ignore_errors=True)
    if 'c3share' in what:
        # configs[2] at its stated size, one rank's share: unet_like2 over the
        # 1024 x 2048 x 2048 volume is 13 tile rows of pitch 82 along z; 8 ranks take
        # 2,2,2,2,2,1,1,1 of them.  Rank 0's slab (2 rows + halo = 182 z rows) runs as a
        # standalone volume, as bench.py / torchrun ranks do, and is compared bit for bit
        # with the same rows of a run over the WHOLE volume on this one GPU.
        from flypylib_amd import multi_gpu
        Z, Y, X = 1024, 2048, 2048
        tile, off, world = 100, 9, 8
        g = fplmodels.unet_like2(tile)[0]
        synth.synthetic_weights(g, 7)
        prog = _capi.Program(ctx, g, (1, 1, 1))
        n_rows = multi_gpu.n_tile_rows(Z, tile, off)
        parts = multi_gpu.slab_partition(n_rows, world)
        zb, ze = parts[0]
        pitch = tile - 2 * off
        z_hi = min(ze * pitch + 2 * off, Z)
        whole_src = torch.empty((Z, Y, X), dtype=torch.uint8, device='cuda')
        ctx.synth_volume_u8(3, (Z, Y, X), out=whole_src)
        whole_dst = torch.empty((Z, Y, X), dtype=torch.float32, device='cuda')
        kw = dict(mean=128.0, std=33.0, precision=_capi.PREC_F16)
        t0 = time.perf_counter()
        prog.infer_volume(whole_src, (tile,) * 3, (off,) * 3, dst=whole_dst, dims=(Z, Y, X), **kw)
        ctx.synchronize()
        t_whole = time.perf_counter() - t0
        slab_src = whole_src[:z_hi].contiguous()
        slab_dst = torch.empty((z_hi, Y, X), dtype=torch.float32, device='cuda')
        prog.infer_volume(slab_src, (tile,) * 3, (off,) * 3, dst=slab_dst, dims=(z_hi, Y, X), **kw)
        ctx.synchronize()
        t0 = time.perf_counter()
        prog.infer_volume(slab_src, (tile,) * 3, (off,) * 3, dst=slab_dst, dims=(z_hi, Y, X), **kw)
        ctx.synchronize()
        t_slab = time.perf_counter() - t0
        lo, hi = multi_gpu.slab_rows((zb, ze), Z, tile, off)
        same = bool(torch.equal(slab_dst[lo:hi], whole_dst[lo:hi]))
        own = (hi - lo - off) * (Y - 2 * off) * (X - 2 * off)     # valid voxels rank 0 owns
        res['configs2_rank0_share'] = dict(
            volume=[Z, Y, X], tile_rows=n_rows, partition=parts, rank0_rows=[lo, hi],
            slab_dims=[z_hi, Y, X], seconds=t_slab, mvox_s=own / t_slab / 1e6,
            tflops_algorithmic=own * 350720 / t_slab / 1e12,
            whole_volume_seconds_one_gpu_cold=t_whole,
            whole_volume_mvox_s=(Z - 18) * (Y - 18) * (X - 18) / t_whole / 1e6,
            slab_rows_identical_to_whole=same, executor=ctx.last_path())
        print(json.dumps(res['configs2_rank0_share']), flush=True)
        del whole_src, whole_dst, slab_src, slab_dst
    if 'c5share' in what:
        # configs[4] at its stated size, one rank's share: the 4096^3 ROI is 512 substacks
        # of 512^3 (+ 35 buffer: 582^3 cubes); with 8 ranks a rank takes every 8th = 64.
        # Rank 3's share is run (x block 3: interior substacks; rank 0's all touch the x = 0
        # face, where the zero fill outside the volume leaves next to no detections).
        # RANK / WORLD_SIZE come from the environment as under torchrun; there is no process
        # group here, so the merge step warns and returns the rank's own detections.
        import pickle
        import shutil
        import tempfile
        import warnings
        from flypylib_amd import FplNetwork, fplpipeline
        from oracle import voxel2obj_oracle
        n = 4096
        net = FplNetwork(fplmodels.vgg_like, precision='f16')
        synth.synthetic_weights(net.train_single, 9)
        net._set_infer()
        wd = tempfile.mkdtemp(prefix='fri_')
        src = 'synth://5,%d,%d,%d' % (n, n, n)
        fplobjdetect.gen_full_tab_roi(wd + '/roi', src, None, step_size=512)
        roi = fplobjdetect.roi_from_txt(wd + '/roi_00.txt')[0]
        norm = [128., 33., 0.5]
        share_rank = 3
        os.environ['RANK'], os.environ['WORLD_SIZE'] = str(share_rank), '8'
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            fplobjdetect.full_roi_inference(src, None, roi[:8], net, 0.1, wd + '/warm', norm)
            ctx.timing(True); ctx.timing_reset()
            t0 = time.perf_counter()
            out = fplobjdetect.full_roi_inference(src, None, wd + '/roi_00.txt', net, 0.1,
                                                  wd + '/work', norm)
            dt = time.perf_counter() - t0
        del os.environ['RANK'], os.environ['WORLD_SIZE']
        kern = {k: round(v['ms'], 2) for k, v in ctx.timing_get().items()}
        ctx.timing(False)
        mine = roi[share_rank::8]
        done = [ss for ss in roi if os.path.isfile(fplobjdetect.fri_filename(wd + '/work', ss))]
        # the substack of the share with the most detections goes to the CPU oracle
        counts = [len(pickle.load(open(fplobjdetect.fri_filename(wd + '/work', s_), 'rb'))['conf'])
                  for s_ in mine]
        ss = mine[int(np.argmax(counts))]
        sz = ss.size + 70
        cube = ctx.malloc((sz,) * 3, np.uint8)
        pred = ctx.malloc((sz,) * 3, np.float32)
        ctx.synth_substack_u8(5, (n, n, n), (sz,) * 3, [ss.z - 35, ss.y - 35, ss.x - 35], cube)
        st = fplpipeline.normalisation_from_histogram(ctx.histogram_u8(cube), norm)
        net.infer_network.program.infer_volume(cube, net.infer_sz, net.rf_offset, mean=st['mn_use'],
                                               std=norm[1], precision=_capi.PREC_F16, dst=pred,
                                               dims=(sz,) * 3)
        t0 = time.perf_counter()
        ref = voxel2obj_oracle.voxel2obj(pred.to_host(), 27, 5, (ss.x - 35, ss.y - 35, ss.z - 35), 35, 0.1)
        t_cpu = time.perf_counter() - t0
        got = pickle.load(open(fplobjdetect.fri_filename(wd + '/work', ss), 'rb'))
        same = np.array_equal(ref['locs'], got['locs']) and np.array_equal(ref['conf'], got['conf'])
        res['configs4_rank_share'] = dict(
            roi=[n, n, n], rank=share_rank, world=8, substacks_total=len(roi), substacks_rank=len(mine),
            detections_per_substack_max=int(max(counts)),
            substacks_written=len(done), all_p_written=os.path.isfile(wd + '/work/all.p'),
            seconds=dt, mvox_s_rank=len(mine) * 512 ** 3 / dt / 1e6,
            detections_rank=int(len(out['conf'])), checked_substack=list(ss),
            checked_substack_detections=int(len(got['conf'])),
            detections_identical_to_cpu_oracle=bool(same), cpu_oracle_v2o_s=t_cpu,
            kernel_ms_total=kern)
        print(json.dumps(res['configs4_rank_share']), flush=True)
        shutil.rmtree(wd, ignore_errors=True)
    if a.out:
        json.dump(res, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
