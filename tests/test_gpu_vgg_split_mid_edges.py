"""The split vgg_like mid kernel's cut blocks (csrc/vgg_split.hip: vggs_mid_pool_edge; the rule:
csrc/vgg_plan.h, vgg_mid_plan): where P2 cuts the last block column (x) or layer (z), that region
runs as launches of its own in an orientation whose short axis is the cut one.  Only which wave,
sub-step and lane computes a voxel changes, so the output is bit-identical with
FPL_VGG_EDGE_BLOCKS=0 (every block in the interior orientation, one launch).

P2 = C + 2 per axis (C coarse outputs = ceil((extent - 14) / 4)); the live extent of the cut column
is P2X mod 8 pooled x (re-oriented for 1 .. 6), of the cut layer P2Z mod 4 pooled z (for 1, 2); the
geometry itself is enumerated on the CPU in tests/test_vgg_mid_geometry.py."""
import numpy as np
import pytest

from flypylib_amd import _capi, fplmodels, multi_gpu, synth
from oracle import cnn_oracle, infer_oracle

pytestmark = pytest.mark.gpu
OFF = 7


def _net(seed, tile):
    g = fplmodels.vgg_like(tile)[0]
    synth.synthetic_weights(g, seed)
    return g


def _both(prog, monkeypatch, vol, tile, **kw):
    """(every block in the interior orientation, cut blocks re-oriented) of one volume"""
    kw.setdefault('precision', _capi.PREC_F16S)
    out = []
    for edge in ('0', '1'):
        monkeypatch.setenv('FPL_VGG_EDGE_BLOCKS', edge)
        out.append(prog.infer_volume(vol, (tile,) * 3, (OFF,) * 3, **kw))
    monkeypatch.delenv('FPL_VGG_EDGE_BLOCKS')
    return out


def _extent(c, ragged=0):
    """an extent with c coarse outputs, the last one holding 4 - ragged fine voxels"""
    return 4 * c + 14 - ragged


def test_every_x_and_z_residue_is_bit_identical(ctx, monkeypatch):
    """P2X = 10 .. 17 (every residue modulo 8: 0 and 7 keep the interior orientation), P2Z = 10 .. 13
    (every residue modulo 4: 0 and 3 keep it), P2Y = 15; uint8 and float32 volumes alternate"""
    g = _net(51, 30)
    prog = _capi.Program(ctx, g, (4, 4, 4))
    for rx in range(8):
        for rz in range(4):
            shape = (_extent(8 + rz, rz % 2), _extent(13, 1), _extent(8 + rx, rx % 4))
            u8 = synth.em_volume_u8(300 + 4 * rx + rz, shape)
            if (rx + rz) % 2:
                img = (u8.astype(np.float32) - np.float32(128)) / np.float32(33)
                full, edge = _both(prog, monkeypatch, img, 30)
            else:
                full, edge = _both(prog, monkeypatch, u8, 30, mean=128.0, std=33.0)
            assert ctx.last_path() == 'vgg_split_f16'
            assert np.array_equal(full, edge), (rx, rz, shape, np.abs(full - edge).max())


def test_long_y_and_several_blocks_per_region(ctx, monkeypatch):
    """more than one block along every axis of both re-oriented regions (P2 = 14 x 35 x 30: the x
    column is 3 x 5 x 4 blocks of 2 x 8 x 4 pooled voxels, the z layer 3 x 9 x 1 of 8 x 4 x 2)"""
    g = _net(52, 30)
    prog = _capi.Program(ctx, g, (4, 4, 4))
    shape = (_extent(12), _extent(33, 2), _extent(28, 1))
    u8 = synth.em_volume_u8(9, shape)
    full, edge = _both(prog, monkeypatch, u8, 30, mean=128.0, std=33.0)
    assert np.array_equal(full, edge)


def test_reoriented_blocks_match_fp32(ctx, monkeypatch):
    """uint8 and float volumes against the fp32 oracle (P2 = 10 x 10 x 11: both regions re-oriented)"""
    shape = (46, 46, 50)
    g = _net(53, 30)
    prog = _capi.Program(ctx, g, (4, 4, 4))
    u8 = synth.em_volume_u8(11, shape)
    img = (u8.astype(np.float32) - np.float32(128)) / np.float32(33)
    ref = infer_oracle.infer_lattice(
        img, (30,) * 3, (OFF,) * 3,
        lambda b: cnn_oracle.vgg_like_forward(b.astype(np.float32), g.weights, 4))
    full, edge = _both(prog, monkeypatch, u8, 30, mean=128.0, std=33.0)
    assert np.array_equal(full, edge)
    assert np.abs(edge - ref).max() < 1e-5
    fullf, edgef = _both(prog, monkeypatch, img, 30)
    assert np.array_equal(fullf, edgef)
    assert np.abs(edgef - ref).max() < 1e-5


@pytest.mark.parametrize('dtype', ['u8', 'f32'])
def test_chunks_and_slabs_are_bit_identical(ctx, monkeypatch, dtype):
    """whole (P2Z = 30), Z chunks of the scratch tensors (a cut layer per chunk) and two / three slabs"""
    g = _net(54, 46)
    prog = _capi.Program(ctx, g, (4, 4, 4))
    u8 = synth.em_volume_u8(12, (123, 70, 117))
    if dtype == 'u8':
        vol, kw = u8, dict(mean=128.0, std=33.0, precision=_capi.PREC_F16S)
    else:
        vol, kw = (u8.astype(np.float32) - np.float32(128)) / np.float32(33), dict(precision=_capi.PREC_F16S)
    monkeypatch.setenv('FPL_VGG_EDGE_BLOCKS', '0')
    whole = prog.infer_volume(vol, (46,) * 3, (OFF,) * 3, **kw)
    monkeypatch.setenv('FPL_VGG_EDGE_BLOCKS', '1')
    assert np.array_equal(prog.infer_volume(vol, (46,) * 3, (OFF,) * 3, **kw), whole)
    monkeypatch.setenv('FPL_VGG_SCRATCH_MB', '2')
    assert np.array_equal(prog.infer_volume(vol, (46,) * 3, (OFF,) * 3, **kw), whole)
    monkeypatch.delenv('FPL_VGG_SCRATCH_MB')
    n_rows = multi_gpu.n_tile_rows(123, 46, OFF)
    for n in (2, 3):
        parts = np.zeros_like(whole)
        for zb, ze in multi_gpu.slab_partition(n_rows, n):
            prog.infer_volume(vol, (46,) * 3, (OFF,) * 3, z_range=(zb, ze), dst=parts, **kw)
        assert np.array_equal(parts, whole), n
