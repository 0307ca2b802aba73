"""GPU: hist_u8 (`fpl_histogram_u8`) against np.bincount and crop_u8 (`fpl_crop_substack_u8`) against a
numpy crop with zero padding, through the C ABI.  Sizes and boxes: tests/perop_cases.py; that they
reach the vector body, the remainder of block 0, the grid stride, the chunks that cross rows, planes
and work-group chunks is shown on the CPU by test_perop_cases_host.py.

Not reached: crop_u8's own grid stride (more than n_cu * 32 chunks of 1024 voxels - an 8 MiB box and
up); its loop is the one synth_u8 runs at full size in test_gpu_fullsize.py."""
import numpy as np
import pytest

from flypylib_amd import _capi
from tests import perop_cases as pc

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xAB


def _sizes(ctx):
    return pc.hist_sizes(ctx.device_info()['n_cu'])


@pytest.mark.parametrize('label', list(pc.hist_sizes(1)))
def test_histogram_sizes(ctx, label):
    n_cu = ctx.device_info()['n_cu']
    n = _sizes(ctx)[label]
    f = pc.hist_facts(n, n_cu)
    if label == 'strided_5':
        assert f['passes'] == 2 and f['capped'] and f['remainder'] == 5
    v = pc.hist_data('random', n)
    want = np.bincount(v, minlength=256)
    got = ctx.histogram_u8(v)
    assert got.shape == (256,) and got.sum() == n and np.array_equal(got, want)
    # ... and from device memory
    buf = ctx.malloc((n,), np.uint8)
    try:
        if n:
            buf.from_host(v)
        assert buf.ptr % 16 == 0
        got = ctx.histogram_u8(buf)
        assert got.sum() == n and np.array_equal(got, want)
    finally:
        buf.free()


@pytest.mark.parametrize('kind', ['constant', 'even_only'])
def test_histogram_of_degenerate_volumes(ctx, kind):
    """all 255: every atomic of a wave lands in one bin; even values only: half the bins are skipped"""
    sizes = _sizes(ctx)
    for n in (sizes['17'], sizes['one_block_less_1'], 16 * 256 * 40 + 7, sizes['strided_5']):
        v = pc.hist_data(kind, n)
        want = np.bincount(v, minlength=256)
        got = ctx.histogram_u8(v)
        assert got.sum() == n and np.array_equal(got, want)
        assert got[255] == n if kind == 'constant' else not got[1::2].any()


def test_histogram_refuses_an_unaligned_device_source(ctx):
    buf = ctx.malloc((64,), np.uint8).from_host(np.arange(64, dtype=np.uint8))
    try:
        for shift in (1, 4, 8):
            with pytest.raises(_capi.FplHipError, match='fpl_histogram_u8: source must be 16-byte aligned'):
                ctx.histogram_u8(buf.ptr + shift, n=32)
        assert np.array_equal(ctx.histogram_u8(buf.ptr + 16, n=32), np.bincount(np.arange(16, 48), minlength=256))
    finally:
        buf.free()


@pytest.fixture(scope='module')
def crop_src(ctx):
    src = pc.crop_source()
    buf = ctx.malloc(src.shape, np.uint8).from_host(src)
    yield src, buf
    buf.free()


@pytest.mark.parametrize('name', list(pc.CROP_BOXES))
def test_crop_boxes(ctx, crop_src, name):
    src, d_src = crop_src
    dims, origin = pc.CROP_BOXES[name]
    n = int(np.prod(dims))
    want = pc.crop_reference(src, dims, origin)
    # guard bytes before and after the destination; the payload 4-byte aligned, as the entry point asks
    buf = ctx.malloc((GUARD + n + GUARD,), np.uint8).from_host(np.full(GUARD + n + GUARD, FILL, np.uint8))
    try:
        assert (buf.ptr + GUARD) % 4 == 0
        ctx.crop_substack_u8(d_src, src.shape, dims, origin, buf.ptr + GUARD)
        ctx.synchronize()
        host = buf.to_host()
    finally:
        buf.free()
    assert (host[:GUARD] == FILL).all() and (host[GUARD + n:] == FILL).all(), 'a guard byte was written'
    got = host[GUARD:GUARD + n].reshape(dims)
    bad = np.argwhere(got != want)
    assert not len(bad), (name, len(bad), bad[:4].tolist())


def test_crop_requires_an_aligned_destination(ctx, crop_src):
    src, d_src = crop_src
    buf = ctx.malloc((64,), np.uint8)
    try:
        with pytest.raises(_capi.FplHipError, match='dst must be 4-byte aligned'):
            ctx.crop_substack_u8(d_src, src.shape, (2, 3, 5), (0, 0, 0), buf.ptr + 1)
    finally:
        buf.free()
