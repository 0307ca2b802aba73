"""GPU: Conv3DTranspose(filters, 2, strides=2) on the 16-bit and split-half graph executor
(csrc/gx_exec.h, FPLK(deconv2) of csrc/conv_mfma.hip) against the float64 restatement of
tests/deconv_cases.py over the reference's tile lattice.  Tolerances: the graph executor's own
(test_gpu_graph_split.TOL) - split halves and 'auto' 1e-5, plain f16 1e-3, bf16 2e-2."""
import numpy as np
import pytest

from flypylib_amd import FplNetwork, _capi, synth
from flypylib_amd.program import LayerGraph
from tests import deconv_cases as dc
from tests import deconv_gx_cases as gc

pytestmark = pytest.mark.gpu
TOL = {'bf16': 2e-2, 'f16': 1e-3, 'f16s': 1e-5, 'auto': 1e-5}
PREC = {'bf16': _capi.PREC_BF16, 'f16': _capi.PREC_F16, 'f16s': _capi.PREC_F16S, 'auto': _capi.PREC_AUTO,
        'f32': _capi.PREC_F32}
OFF = 4
_REF = {}


def _unet(tile, shape):
    """graph, uint8 volume and float64 lattice reference of unet_t3 at one tile: made once, not changed"""
    key = (tile, shape)
    if key not in _REF:
        g = gc.unet_t3_random((tile,) * 3)[0]
        u8 = synth.em_volume_u8(13, shape)
        img = (u8.astype(np.float32) - np.float32(128)) / np.float32(33)
        _REF[key] = (g, u8, gc.lattice_oracle(g, img, tile, OFF))
    return _REF[key]


def _run(prog, u8, tile, off, kind, **kw):
    return prog.infer_volume(u8, (tile,) * 3, (off,) * 3, mean=128.0, std=33.0, precision=PREC[kind], **kw)


@pytest.mark.parametrize('tile,shape', [(24, (46, 24, 37)), (22, (40, 22, 30))])
@pytest.mark.parametrize('kind', ['f16s', 'f16', 'bf16', 'auto'])
def test_unet_with_a_deconv_end_to_end(ctx, tile, shape, kind):
    """tile 24: the deconv reads 9^3 voxels per tile, six tiles - groups of 16 voxels straddle rows,
    planes and tiles and the last one is ragged (6 * 729 = 273 * 16 + 6); tile 22: 8^3, four tiles"""
    g, u8, ref = _unet(tile, shape)
    prog = _capi.Program(ctx, g, (1, 1, 1))
    ctx.timing(True)
    ctx.timing_reset()
    got = _run(prog, u8, tile, OFF, kind)
    names = set(ctx.timing_get())
    ctx.timing(False)
    path = ctx.last_path()
    prog.close()
    err = float(np.max(np.abs(got - ref)))
    print('unet_t3 tile %d %s: max |gpu - float64| %.3g on %s' % (tile, kind, err, path))
    assert path == ('graph_split_f16' if kind in ('f16s', 'auto') else 'graph_mfma_' + kind)
    assert 'gx_deconv2' in names, names
    assert ref[OFF:-OFF, OFF:-OFF, OFF:-OFF].std() > 1e-4
    assert got.shape == shape and err < TOL[kind]
    for ax in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, OFF), slice(shape[ax] - OFF, shape[ax])
        assert not got[tuple(lo)].any() and not got[tuple(hi)].any()


@pytest.mark.parametrize('cin,cout', [(16, 8), (32, 32), (48, 24), (64, 64), (96, 48), (128, 64)])
def test_the_layer_alone_every_width_class_and_epilogue(ctx, cin, cout):
    """deconv input 5^3 voxels per tile (125: a ragged last group), two tiles; with and without bias;
    ReLU on the layer, folded BN + ReLU, no activation into the stand-alone Add"""
    worst = {'f16s': 0.0, 'f16': 0.0, 'f16s-f32': 0.0}
    for epilogue in gc.EPILOGUES:
        for bias in (0, 1):
            g, off = gc.layer_alone(cin, cout, bias, epilogue, edge=5, seed=cin + bias)
            tile = gc.tile_of(cin, 5)
            shape = (2 * tile - 2 * off, tile, tile)
            u8 = synth.em_volume_u8(7 + bias, shape)
            img = (u8.astype(np.float32) - np.float32(128)) / np.float32(33)
            ref = gc.lattice_oracle(g, img, tile, off)
            assert ref[off:-off, off:-off, off:-off].std() > 1e-4
            prog = _capi.Program(ctx, g, (1, 1, 1))
            out = {}
            for kind in ('f16s', 'f16', 'f32'):
                ctx.timing(True)
                ctx.timing_reset()
                out[kind] = _run(prog, u8, tile, off, kind)
                names = set(ctx.timing_get())
                ctx.timing(False)
                if kind != 'f32':
                    assert ctx.last_path() == ('graph_split_f16' if kind == 'f16s' else 'graph_mfma_f16')
                    assert 'gx_deconv2' in names and ('gx_add' in names) == (epilogue == 'add'), names
            prog.close()
            for kind in ('f16s', 'f16'):
                err = float(np.max(np.abs(out[kind] - ref)))
                worst[kind] = max(worst[kind], err)
                assert err < TOL[kind], (epilogue, bias, kind, err)
            err = float(np.max(np.abs(out['f16s'] - out['f32'])))
            worst['f16s-f32'] = max(worst['f16s-f32'], err)
            assert err < 1e-5, (epilogue, bias, err)
    print('%d -> %d: max |gpu - float64|' % (cin, cout), worst)


def test_auto_properties(ctx, monkeypatch):
    """'auto' on the split executor: run to run bit-identical, two Z slabs == whole, and the super-tile
    switch changes no bit (super-tiles are declined for programs with the layer)"""
    from flypylib_amd import multi_gpu
    tile, shape = 24, (46, 24, 37)
    g, u8, ref = _unet(tile, shape)
    prog = _capi.Program(ctx, g, (1, 1, 1))
    whole = _run(prog, u8, tile, OFF, 'auto')
    assert ctx.last_path() == 'graph_split_f16'
    assert np.array_equal(_run(prog, u8, tile, OFF, 'auto'), whole)
    nz = multi_gpu.n_tile_rows(shape[0], tile, OFF)
    assert nz == 3
    out = np.zeros(shape, np.float32)
    for lo, hi in multi_gpu.slab_partition(nz, 2):
        _run(prog, u8, tile, OFF, 'auto', z_range=(lo, hi), dst=out)
    assert np.array_equal(out, whole)
    monkeypatch.setenv('FPL_NO_TILE_MERGE', '1')
    assert np.array_equal(_run(prog, u8, tile, OFF, 'auto'), whole)
    monkeypatch.delenv('FPL_NO_TILE_MERGE')
    prog.close()


def _scaled_unet(tile, target):
    """unet_t3 with its deconv kernel scaled so the largest folded weight (kernel * gamma / sqrt(var + eps))
    is `target`; returns (graph, largest float64 activation behind the layer's BN + ReLU on a test volume)"""
    g = gc.unet_t3_random((tile,) * 3)[0]
    d = [n for n in g.nodes if n.kind == 'deconv'][0]
    bn = g.nodes[d.idx + 1]
    assert bn.kind == 'bn' and g.nodes[d.idx + 2].kind == 'relu'
    gamma, var = g.weights[bn.weight_slots[0]], g.weights[bn.weight_slots[3]]
    fold = np.abs(g.weights[d.weight_slots[0]] * (gamma / np.sqrt(var + dc.BN_EPS))[None, None, None, :, None]).max()
    g.weights[d.weight_slots[0]] = (g.weights[d.weight_slots[0]] * np.float32(target / fold)).astype(np.float32)
    u8 = synth.em_volume_u8(5, (40, tile, tile))
    img = (u8[:tile].astype(np.float64) - 128.0) / 33.0
    out = g.output
    g.output = g.nodes[d.idx + 2]
    try:
        peak = float(dc.graph_forward64(g, img[None, ..., None]).max())
    finally:
        g.output = out
    return g, u8, peak


def test_half_range_guard(ctx):
    """an output of the layer beyond 65504 (its weights inside): 'f16s' fails, 'auto' reruns in fp32;
    a folded weight of the layer beyond 65504: the packer refuses, 'auto' runs fp32"""
    tile = 24
    g, u8, peak = _scaled_unet(tile, 3.0e4)
    assert peak > 65504.0, peak
    prog = _capi.Program(ctx, g, (1, 1, 1))
    with pytest.raises(_capi.FplHipError, match='IEEE-half range'):
        _run(prog, u8, tile, OFF, 'f16s')
    got = _run(prog, u8, tile, OFF, 'auto')
    assert ctx.last_path() == 'mfma_f32(range)' and np.isfinite(got).all()
    prog.close()
    g, u8, peak = _scaled_unet(tile, 1.0e5)
    prog = _capi.Program(ctx, g, (1, 1, 1))
    with pytest.raises(_capi.FplHipError, match='folded weight exceeds the IEEE-half range'):
        _run(prog, u8, tile, OFF, 'f16s')
    got = _run(prog, u8, tile, OFF, 'auto')
    assert ctx.last_path() == 'mfma_f32(range)' and np.isfinite(got).all()
    prog.close()


def _wide():
    """a deconv with 96 outputs: no kernel of that width (conv1's widths: up to 64)"""
    g = LayerGraph((12,) * 3, seed=2)
    x = g.pool(g.conv_bn_relu(g.input(), 16, 3))
    x = g.deconv(x, 96, use_bias=True, activation='relu')
    x = g.conv_bn_relu(x, 16, 1)
    return dc.randomize(g.finish(g.conv(x, 1, 1, use_bias=True, activation='sigmoid'))), 1, (1, 1, 1)


def _pooled():
    """a MaxPooling3D directly on the layer's output"""
    g = LayerGraph((12,) * 3, seed=2)
    x = g.pool(g.conv_bn_relu(g.input(), 16, 3))
    x = g.pool(g.deconv(x, 16, use_bias=True, activation='relu'))
    return dc.randomize(g.finish(g.conv(x, 1, 1, use_bias=True, activation='sigmoid'))), 1, (2, 2, 2)


@pytest.mark.parametrize('make', [_wide, _pooled])
def test_programs_out_of_reach_keep_fp32(ctx, make):
    g, off, stride = make()
    prog = _capi.Program(ctx, g, stride)
    u8 = synth.em_volume_u8(1, (22, 12, 12))
    with pytest.raises(_capi.FplHipError, match='Conv3DTranspose'):
        _run(prog, u8, 12, off, 'f16s')
    got = _run(prog, u8, 12, off, 'auto')
    assert ctx.last_path() == 'mfma_f32' and got[off:-off, off:-off, off:-off].std() > 1e-4
    prog.close()


def test_public_surface(ctx):
    """FplNetwork.infer at the default precision: the split executor, and Program.infer_volume's bits"""
    net = FplNetwork(gc.unet_t3_random)
    net._set_infer()
    assert net.rf_offset == (4, 4, 4) and net.infer_sz == (24, 24, 24)
    vol = np.random.default_rng(2).standard_normal((46, 24, 37)).astype(np.float32)
    pred = net.infer(vol)
    assert ctx.last_path() == 'graph_split_f16'
    same = net.infer_network.program.infer_volume(vol, net.infer_sz, net.rf_offset, precision=_capi.PREC_AUTO)
    assert ctx.last_path() == 'graph_split_f16' and np.array_equal(pred, same)
    assert pred[4:-4, 4:-4, 4:-4].std() > 1e-4 and not pred[:4].any()
