"""GPU: gather_tiles<uint8_t|float>, stitch_tiles and upsample_out of csrc/infer.hip held bit for bit.
The programs of tests/perop_cases.py (P1: crop; P2: pool, crop, output stride 2; P3: two pools, output
stride 4) only move and compare values, so the whole `fpl_infer_volume` result is np.array_equal to
`infer_oracle.infer_lattice` with a numpy `predict` - the on-device u8 normalisation, the zero padding in
the normalised domain, `x / stride` in the stitch, z slabs into one destination included.

Routes.  The fp32 MFMA executor does not take a 1x1x1 convolution on a crop view
(fpl_mfma_f32_supported), so P1 and P2 run on the per-op executor whatever the switches say, and the
tests assert that; P3 runs on both.  With offset 0 there is no halo for a super-tile to save, so P3's
tiles are never merged (infer.hip picks the cheapest m, which is 1): FPL_NO_TILE_MERGE is held to change
nothing, not shown to switch anything off."""
import numpy as np
import pytest

from flypylib_amd import _capi, multi_gpu
from tests import perop_cases as pc

pytestmark = pytest.mark.gpu

NATURAL = {'P1_off0': 'perop_f32', 'P1_off3': 'perop_f32', 'P2': 'perop_f32', 'P3': 'mfma_f32'}


def _program(ctx, name):
    return _capi.Program(ctx, pc.lattice_graph(name), (pc.LATTICE[name]['stride'],) * 3)


def _env(monkeypatch, forced=False, no_merge=False):
    for var, on in (('FPL_FORCE_PEROP', forced), ('FPL_NO_TILE_MERGE', no_merge)):
        if on:
            monkeypatch.setenv(var, '1')
        else:
            monkeypatch.delenv(var, raising=False)


@pytest.mark.parametrize('source', pc.SOURCES)
@pytest.mark.parametrize('name', sorted(pc.LATTICE))
def test_four_routes_equal_the_reference(ctx, monkeypatch, name, source):
    c = pc.LATTICE[name]
    src, mean, std, _ = pc.lattice_source(name, source)
    ref = pc.lattice_reference(name, source)
    off, cubic = (c['off'],) * 3, (c['tile'],) * 3
    prog = _program(ctx, name)
    try:
        for label, tile, forced, no_merge, path in [
                ('default', cubic, False, False, NATURAL[name]),
                ('no tile merge', cubic, False, True, NATURAL[name]),
                ('forced per-op', cubic, True, False, 'perop_f32'),
                ('tile with three different edges', c['alt'], False, False, 'perop_f32')]:
            _env(monkeypatch, forced, no_merge)
            got = prog.infer_volume(src, tile, off, mean=mean, std=std)
            assert ctx.last_path() == path, (label, ctx.last_path())
            assert got.dtype == np.float32 and got.shape == ref.shape
            bad = np.flatnonzero(got != ref)
            assert not bad.size, (label, bad.size, got.flat[bad[:4]], ref.flat[bad[:4]])
    finally:
        prog.close()


@pytest.mark.parametrize('name', sorted(pc.LATTICE))
def test_thin_volumes(ctx, monkeypatch, name):
    """an axis <= 2 * off: no tile, all zero; = 2 * off + 1: one (mostly padded) tile row"""
    c = pc.LATTICE[name]
    off, tile = (c['off'],) * 3, (c['tile'],) * 3
    prog = _program(ctx, name)
    try:
        for label, vol in pc.thin_volumes(name).items():
            src, mean, std, _ = pc.lattice_source(name, 'u8_128_33', vol)
            ref = pc.lattice_reference(name, 'u8_128_33', vol=vol)
            for forced in (False, True):
                _env(monkeypatch, forced)
                dst = np.full(vol, np.nan, np.float32)
                got = prog.infer_volume(src, tile, off, mean=mean, std=std, dst=dst)
                want_path = 'perop_f32' if forced else NATURAL[name]
                assert ctx.last_path() in (want_path, 'none'), (label, ctx.last_path())
                assert np.array_equal(got, ref), (label, forced)
                assert got.any() == label.startswith('one')
    finally:
        prog.close()


@pytest.mark.parametrize('forced', [False, True])
@pytest.mark.parametrize('name', sorted(pc.LATTICE))
def test_slabs_and_resident_buffers(ctx, monkeypatch, name, forced):
    """z_range slabs of 1, 2 and 3 ranks into one destination prefilled with NaN: every voxel is
    written, the shell's zeros included; device-resident source and destination give the same bits"""
    _env(monkeypatch, forced)
    c = pc.LATTICE[name]
    vol, off, tile = c['vol'], (c['off'],) * 3, (c['tile'],) * 3
    src, mean, std, _ = pc.lattice_source(name, 'u8_127.3_0.1')
    ref = pc.lattice_reference(name, 'u8_127.3_0.1')
    path = 'perop_f32' if forced else NATURAL[name]
    n = multi_gpu.n_tile_rows(vol[0], c['tile'], c['off'])
    prog = _program(ctx, name)
    d_src = ctx.malloc(vol, np.uint8).from_host(src)
    d_dst = ctx.malloc(vol, np.float32)
    try:
        for ranks in (1, 2, 3):
            parts = multi_gpu.slab_partition(n, ranks)
            assert all(e > b for b, e in parts)
            host = np.full(vol, np.nan, np.float32)
            d_dst.from_host(host)
            for zr in parts:
                prog.infer_volume(src, tile, off, mean=mean, std=std, z_range=zr, dst=host)
                assert ctx.last_path() == path
                prog.infer_volume(d_src, tile, off, mean=mean, std=std, z_range=zr, dst=d_dst, dims=vol)
                assert ctx.last_path() == path
            assert np.array_equal(host, ref), ranks
            assert np.array_equal(d_dst.to_host(), ref), ranks
    finally:
        prog.close()
        d_src.free()
        d_dst.free()


@pytest.mark.parametrize('forced', [False, True])
@pytest.mark.parametrize('name', ['P2', 'P3'])
def test_forward_upsamples_the_output(ctx, monkeypatch, name, forced):
    """`Program.forward` with an output stride: upsample_out == np.repeat along the three axes, batch 3"""
    _env(monkeypatch, forced)
    c = pc.LATTICE[name]
    prog = _program(ctx, name)
    try:
        for tile, path in (((c['tile'],) * 3, 'perop_f32' if forced else NATURAL[name]), (c['alt'], 'perop_f32')):
            x = np.random.default_rng(sum(tile)).standard_normal((3,) + tuple(tile) + (1,)).astype(np.float32)
            got = prog.forward(x)
            assert ctx.last_path() == path
            want = pc.lattice_predict(name)(x)
            assert want.shape == (3,) + tuple(t - 2 * c['off'] for t in tile) + (1,)
            assert got.dtype == np.float32 and np.array_equal(got, want)
    finally:
        prog.close()
