"""The split vgg_like stem's partial blocks (csrc/vgg_split.hip, StemTrim): blocks that P1 cuts
run only the tasks that hold P1 voxels, as patches of 4 / 8 / 16 pooled x.  Only which lane and
task computes a voxel changes, so the output is bit-identical with FPL_VGG_EDGE_BLOCKS=0 (every
block walked in full).  The sweep hits every residue of the block's live x extent (P1X mod 32 =
2 CX + 6 mod 32: CX mod 16), of its live y extent (CY mod 4) and of its z extent (CZ mod 2)."""
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
    """(full-block walk, trimmed walk) of one volume"""
    kw.setdefault('precision', _capi.PREC_F16S)
    out = []
    for edge in ('0', '1'):
        monkeypatch.setenv('FPL_VGG_EDGE_BLOCKS', edge)
        out.append(prog.infer_volume(vol, (tile,) * 3, (OFF,) * 3, **kw))
    monkeypatch.delenv('FPL_VGG_EDGE_BLOCKS')
    return out


def _fp32(g, img, tile):
    return infer_oracle.infer_lattice(
        img, (tile,) * 3, (OFF,) * 3,
        lambda b: cnn_oracle.vgg_like_forward(b.astype(np.float32), g.weights, 4))


def test_every_x_residue_is_bit_identical(ctx, monkeypatch):
    g = _net(41, 30)
    prog = _capi.Program(ctx, g, (4, 4, 4))
    for r in range(16):
        shape = (46, 46, 4 * (16 + r) + 14 - (r % 4))     # CX = 16 + r, ragged last coarse x
        u8 = synth.em_volume_u8(100 + r, shape)
        full, trim = _both(prog, monkeypatch, u8, 30, mean=128.0, std=33.0)
        assert ctx.last_path() == 'vgg_split_f16'
        assert np.array_equal(full, trim), (r, shape, np.abs(full - trim).max())


def test_every_y_and_z_residue_is_bit_identical(ctx, monkeypatch):
    g = _net(42, 30)
    prog = _capi.Program(ctx, g, (4, 4, 4))
    for ry in range(4):
        for rz in range(2):
            shape = (4 * (10 + rz) + 14, 4 * (12 + ry) + 14 - ry, 4 * 19 + 14)
            u8 = synth.em_volume_u8(200 + 4 * rz + ry, shape)
            full, trim = _both(prog, monkeypatch, u8, 30, mean=128.0, std=33.0)
            assert np.array_equal(full, trim), (ry, rz, shape)


@pytest.mark.parametrize('shape', [(46, 46, 78), (50, 59, 76), (47, 46, 126)])
def test_trimmed_blocks_match_fp32(ctx, monkeypatch, shape):
    """uint8 (through the padding table) and float volumes, against the fp32 oracle"""
    g = _net(43, 30)
    prog = _capi.Program(ctx, g, (4, 4, 4))
    u8 = synth.em_volume_u8(7, shape)
    img = (u8.astype(np.float32) - np.float32(128)) / np.float32(33)
    ref = _fp32(g, img, 30)
    full, trim = _both(prog, monkeypatch, u8, 30, mean=128.0, std=33.0)
    assert np.array_equal(full, trim)
    assert np.abs(trim - ref).max() < 1e-5
    fullf, trimf = _both(prog, monkeypatch, img, 30)
    assert np.array_equal(fullf, trimf)
    assert np.abs(trimf - ref).max() < 1e-5


def test_chunks_and_slabs_are_bit_identical(ctx, monkeypatch):
    """Z chunks of the scratch tensors (a partial z layer per chunk) and two / three slabs"""
    g = _net(44, 46)
    prog = _capi.Program(ctx, g, (4, 4, 4))
    u8 = synth.em_volume_u8(8, (131, 70, 121))
    kw = dict(mean=128.0, std=33.0, precision=_capi.PREC_F16S)
    monkeypatch.setenv('FPL_VGG_EDGE_BLOCKS', '0')
    whole = prog.infer_volume(u8, (46,) * 3, (OFF,) * 3, **kw)
    monkeypatch.setenv('FPL_VGG_EDGE_BLOCKS', '1')
    assert np.array_equal(prog.infer_volume(u8, (46,) * 3, (OFF,) * 3, **kw), whole)
    monkeypatch.setenv('FPL_VGG_SCRATCH_MB', '2')
    assert np.array_equal(prog.infer_volume(u8, (46,) * 3, (OFF,) * 3, **kw), whole)
    monkeypatch.delenv('FPL_VGG_SCRATCH_MB')
    n_rows = multi_gpu.n_tile_rows(131, 46, OFF)
    for n in (2, 3):
        parts = np.zeros_like(whole)
        for zb, ze in multi_gpu.slab_partition(n_rows, n):
            prog.infer_volume(u8, (46,) * 3, (OFF,) * 3, z_range=(zb, ze), dst=parts, **kw)
        assert np.array_equal(parts, whole), n


def test_520_cube_is_bit_identical(ctx, monkeypatch):
    """the benchmark's volume: 4 of 32 live x and 4 of 8 live y in the last blocks"""
    g = _net(45, 102)
    prog = _capi.Program(ctx, g, (4, 4, 4))
    u8 = synth.em_volume_u8(3, (520, 520, 520))
    full, trim = _both(prog, monkeypatch, u8, 102, mean=128.0, std=33.0)
    assert np.array_equal(full, trim)
