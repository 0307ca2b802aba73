"""CPU: CLAHE as far as it can be checked without a GPU - the pieces of the numpy specification
(clahe.clip_histogram, map_histogram, reflect_index, clahe_numpy), the public fplutils.clahe and
its files, what the device path refuses before any library is loaded, and what is
libfplclahe.so's own of its C ABI."""
import os
import re
import sys

import numpy as np
import pytest

from flypylib_amd import _clahecapi, clahe, fplutils, keras_io
from flypylib_amd.csrc import build
from tests import side_abi_cases as abi

ROOT = abi.ROOT


def _volume(seed=0, shape=(3, 20, 17)):
    return np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)


# ---- the pieces of the specification ---------------------------------------------------------------

def test_clip_histogram_hand_example():
    got = clahe.clip_histogram([10, 0, 0, 0], 4)
    assert got.dtype == np.int64 and list(got) == [4, 2, 2, 2]


def test_clip_histogram_leaves_a_histogram_below_the_limit_alone():
    h = np.random.default_rng(1).integers(0, 9, 256)
    assert np.array_equal(clahe.clip_histogram(h, 9), h)
    assert np.array_equal(clahe.clip_histogram(h, int(h.max())), h)
    assert np.array_equal(clahe.clip_histogram(h, clahe.NR_OF_GRAY), h)


@pytest.mark.parametrize('seed', range(6))
def test_clip_histogram_keeps_the_sum_where_it_fits(seed):
    """where n * clim >= sum(h) no count is lost.  The sum is preserved in that sense only, since
    the specified clip can hand out more than the excess: bins in [clim - bin_incr, clim) are
    raised to clim whatever is left (256 bins, clim 58, 7917 in excess: 367 counts too many), and
    so can the last strided selection of the loop (64 counts in one bin of 256, clim 1: 63 in
    excess, every fourth bin takes one, 64 bins) - which is why step (i) clamps the map at 16383."""
    rng = np.random.default_rng(seed)
    n = int(rng.choice([4, 16, 64, 256]))
    h = rng.integers(0, 50, n)
    h[rng.integers(0, n)] += int(rng.integers(0, 40 * n))
    clim = -(-int(h.sum()) // n) + int(rng.integers(0, 5))     # n * clim >= sum(h)
    got = clahe.clip_histogram(h, clim)
    assert h.sum() <= got.sum() <= n * clim and got.max() <= clim and got.min() >= 0
    assert (got >= np.minimum(h, clim)).all()                   # a bin only loses what is clipped


def test_clip_histogram_one_occupied_bin_and_a_limit_of_one():
    h = np.zeros(256, np.int64)
    h[17] = 256
    got = clahe.clip_histogram(h, 1)
    assert list(got) == [1] * 256               # 255 in excess, every other bin takes one
    h[17] = 64                                  # 63 in excess, 255 bins under: every fourth from 0
    trace = []
    got = clahe.clip_histogram(h, 1, trace)
    assert list(got) == [int(i % 4 == 0 or i == 17) for i in range(256)] and trace == [1]
    assert clahe.clip_histogram([10, 0, 0, 0], 4).sum() == 10   # the hand example keeps its sum


def test_map_histogram():
    h = np.random.default_rng(2).integers(0, 5, 256)
    m = clahe.map_histogram(h, int(h.sum()))
    assert m.dtype == np.uint16 and m[-1] == clahe.NR_OF_GRAY - 1
    assert (np.diff(m.astype(np.int64)) >= 0).all()
    clipped = clahe.clip_histogram(h, 3)        # counts are lost: the map ends below the top
    m = clahe.map_histogram(clipped, int(h.sum()))
    assert (np.diff(m.astype(np.int64)) >= 0).all() and m[-1] <= clahe.NR_OF_GRAY - 1
    assert list(clahe.map_histogram([1, 0, 3], 4)) == [4095, 4095, 16383]


@pytest.mark.parametrize('s', range(2, 8))
def test_reflect_index_is_numpys_reflect_padding(s):
    for a in range(3 * s + 1):
        for b in range(3 * s + 1):
            want = np.pad(np.arange(s), (a, b), 'reflect')
            assert [clahe.reflect_index(i, s) for i in range(-a, s + b)] == list(want), (s, a, b)
    assert clahe.reflect_index(5, 1) == clahe.reflect_index(-3, 1) == 0


# ---- clahe_numpy -----------------------------------------------------------------------------------

def test_clahe_numpy_shape_dtype_and_range():
    im = _volume()
    out = clahe.clahe_numpy(im, 8)
    assert out.dtype == np.float32 and out.shape == im.shape
    for z in range(im.shape[0]):
        assert out[z].min() == 0.0 and out[z].max() == 1.0
    zm = clahe.clahe_numpy(im, 8, zero_mean=True)
    assert zm.dtype == np.float32 and np.array_equal(zm, out - np.float32(0.5))
    assert np.array_equal(clahe.clahe_numpy(im.astype(np.float32), 8), out)


def test_clahe_numpy_constant_slice_and_constant_volume():
    im = _volume(3)
    im[1] = 77
    out = clahe.clahe_numpy(im, 8)
    assert (out[1] == 0.0).all() and out[0].max() == 1.0 and out[2].max() == 1.0
    assert (clahe.clahe_numpy(im, 8, zero_mean=True)[1] == -0.5).all()
    with pytest.raises(ValueError, match='the volume is constant'):
        clahe.clahe_numpy(np.full((2, 8, 8), 5, np.uint8), 4)
    with pytest.raises(ValueError, match='non-finite'):
        clahe.clahe_numpy(np.array([[[0.0, np.nan], [1.0, 2.0]]], np.float32), 2)
    with pytest.raises(ValueError, match='3-D'):
        clahe.clahe_numpy(np.zeros((8, 8), np.uint8), 4)


def test_clahe_numpy_kernel_size_forms_and_trace():
    im = _volume(4, (2, 24, 40))
    trace = {}
    a = clahe.clahe_numpy(im, 8, trace=trace)
    assert trace['nt'] == (3, 5) and trace['tiles_in_while'] >= 0 and trace['max_passes'] >= 0
    assert np.array_equal(a, clahe.clahe_numpy(im, (8, 8)))
    assert np.array_equal(a, clahe.clahe_numpy(im, [8]))
    b = clahe.clahe_numpy(im, None, trace=trace)                # an eighth of the slice: (3, 5)
    assert trace['nt'] == (8, 8) and np.array_equal(b, clahe.clahe_numpy(im, (3, 5)))
    assert not np.array_equal(a, b)
    assert clahe.tile_size(None, (5, 100)) == (1, 12)
    for bad in (0, (4, 0), (1, 2, 3)):
        with pytest.raises(ValueError, match='kernel_size'):
            clahe.clahe_numpy(im, bad)
    # a pad beyond s - 1 reflects more than once
    clahe.clahe_numpy(_volume(5, (1, 5, 5)), 4, trace=trace)
    assert trace['max_pad_ratio'] == 1.25


def test_equalisation_flattens_the_histogram():
    """what CLAHE is for: one tile over a slice squeezed into a quarter of its range spreads it
    over the whole of [0, 1]; with no clipping it is plain histogram equalisation"""
    im = np.random.default_rng(6).integers(100, 164, (1, 32, 32)).astype(np.uint8)
    out = clahe.clahe_numpy(im, 32, clip_limit=0)
    order = np.argsort(im.reshape(-1), kind='stable')
    assert (np.diff(out.reshape(-1)[order]) >= 0).all()         # monotone in the input
    assert abs(float(out.mean()) - 0.5) < 0.05 and 0.2 < float(np.median(out)) < 0.8


# ---- fplutils.clahe --------------------------------------------------------------------------------

def test_fplutils_clahe_the_references_call_and_its_files(tmp_path):
    im = _volume(7)
    want = clahe.clahe_numpy(im, 8)
    got = fplutils.clahe(im, 8)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(got, want)
    npy_in = str(tmp_path / 'in.npy')
    np.save(npy_in, im)
    npy_out, h5_out = str(tmp_path / 'out.npy'), str(tmp_path / 'out.h5')
    got = fplutils.clahe(npy_in, 8, npy_out, True)              # the reference's four positionals
    assert np.array_equal(got, want - np.float32(0.5)) and np.array_equal(np.load(npy_out), got)
    got = fplutils.clahe(im, 8, h5_out)
    back = keras_io.read_main(h5_out)
    assert back.dtype == np.float32 and np.array_equal(back, want) and np.array_equal(got, want)
    assert np.array_equal(fplutils.clahe(h5_out, 8), clahe.clahe_numpy(want, 8))   # an .h5 path in
    assert np.array_equal(fplutils.clahe(im, (4, 8), clip_limit=0.05, nbins=64),
                          clahe.clahe_numpy(im, (4, 8), 0.05, 64))
    for text in ('UNPINNED', 'constant', 'CONTIGUOUS', 'no silent host fallback'):
        assert text in fplutils.clahe.__doc__, text
    assert 'out of scope' not in fplutils.__doc__ and 'UNPINNED' in fplutils.__doc__


def test_the_device_path_refuses_before_any_library_is_loaded(monkeypatch):
    import torch

    def no_load(*a, **k):
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_clahecapi._side, 'load', no_load)
    monkeypatch.setattr(_clahecapi, 'load_library', no_load)
    im = _volume(8, (2, 8, 8))
    with pytest.raises(ValueError, match=r'nbins 257 is outside 2\.\.256'):
        fplutils.clahe(im, 4, device=0, nbins=257)
    with pytest.raises(ValueError, match=r'nbins 1 is outside 2\.\.256'):
        fplutils.clahe(im, 4, device=0, nbins=1)
    with pytest.raises(ValueError, match='must be uint8 or float32, got float64'):
        fplutils.clahe(torch.zeros((2, 8, 8), dtype=torch.float64), 4, device=0)
    with pytest.raises(ValueError, match='must be uint8 or float32, got int16'):
        fplutils.clahe(im.astype(np.int16), 4, device=True)
    with pytest.raises(ValueError, match='must be 3-D'):
        fplutils.clahe(im[0], 4, device=0)
    with pytest.raises(ValueError, match='holds 2\\^31 or more pixels'):
        fplutils.clahe(im, (2 ** 16, 2 ** 15), device=0)
    with pytest.raises(ValueError, match='numpy array or a torch CUDA tensor'):
        fplutils.clahe(torch.zeros((2, 8, 8), dtype=torch.uint8), 4, device=0)


def test_a_missing_library_is_reported_not_replaced_by_the_host(monkeypatch):
    monkeypatch.setattr(_clahecapi._side, '_lib', None)
    monkeypatch.setattr(_clahecapi._side, 'path', '/nonexistent/libfplclahe.so')
    with pytest.raises(_clahecapi.FplClaheError, match='libfplclahe.so not found at /nonexistent') as e:
        fplutils.clahe(_volume(9, (1, 8, 8)), 4, device=0)
    assert 'python -m flypylib_amd.csrc.build' in str(e.value) and 'no host fallback' in str(e.value)


# ---- the build and the C ABI -----------------------------------------------------------------------

def test_the_library_loads_and_the_constants_are_the_headers():
    assert _clahecapi.load_library().fplc_abi_version() == _clahecapi.ABI_VERSION
    hdr = open(os.path.join(ROOT, 'include', 'fplclahe.h')).read()
    for name in ('ABI_VERSION', 'BLOCK', 'MAX_NBINS', 'NR_OF_GRAY', 'STATUS_BYTES', 'STAGE_RANGE',
                 'STAGE_MAPS', 'STAGE_APPLY', 'STAGE_FINISH', 'STAGE_ALL'):
        assert int(re.search(r'#define FPLC_%s (\d+)' % name, hdr).group(1)) == getattr(_clahecapi, name), name
    assert re.search(r'FPLC_U8 = %d, FPLC_F32 = %d' % (_clahecapi.U8, _clahecapi.F32), hdr)
    assert clahe.NR_OF_GRAY == _clahecapi.NR_OF_GRAY and clahe.MAX_DEVICE_NBINS == _clahecapi.MAX_NBINS


def test_scratch_bytes_and_refusals_before_the_gpu_is_touched():
    """every refusal here returns before a launch (and before a pointer is looked at)"""
    err = _clahecapi.FplClaheError
    # status, 16 bytes per slice, 2 * 4 * 3 tiles of 256 uint16, the uint16 volume; parts on 16
    assert _clahecapi.scratch_bytes(2, 13, 11, 4, 5, 256) == 16 + 32 + 24 * 512 + 576
    assert _clahecapi.scratch_bytes(1, 1, 1, 1, 1, 2) == 16 + 16 + 16 + 16
    with pytest.raises(err, match=r'fplc_scratch_bytes: nbins 257 is outside 2\.\.256'):
        _clahecapi.scratch_bytes(1, 8, 8, 4, 4, 257)
    with pytest.raises(err, match='fplc_scratch_bytes: a volume of'):
        _clahecapi.scratch_bytes(0, 8, 8, 4, 4, 256)
    with pytest.raises(err, match='exceeds the 2\\^31 - 1 voxels'):
        _clahecapi.scratch_bytes(2048, 1024, 1024, 4, 4, 256)
    with pytest.raises(err, match='holds 2\\^31 or more pixels'):
        _clahecapi.scratch_bytes(1, 8, 8, 2 ** 16, 2 ** 15, 256)
    with pytest.raises(err, match=r'ky 0 must lie in \[1, 2\^31 - 1\]'):
        _clahecapi.scratch_bytes(1, 8, 8, 0, 4, 256)
    need = _clahecapi.scratch_bytes(1, 8, 8, 4, 4, 256)
    ok = dict(src=4096, is_u8=False, dims=(1, 8, 8), k=(4, 4), clim=1, nbins=256, zero_mean=0,
              out=8192, scratch=16384, scratch_size=need, stages=15)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return _clahecapi.clahe(*a.values(), None)
    with pytest.raises(err, match=r'fplc_clahe: clim 0 must lie in'):
        call(clim=0)
    for bad in (0, 16):
        with pytest.raises(err, match='fplc_clahe: stages %d is no combination' % bad):
            call(stages=bad)
    for name in ('src', 'out', 'scratch'):
        with pytest.raises(err, match='fplc_clahe: null pointer argument'):
            call(**{name: 0})
    with pytest.raises(err, match='scratch of %d bytes, fplc_scratch_bytes is %d' % (need - 1, need)):
        call(scratch_size=need - 1)
    with pytest.raises(err, match='a float32 in is not 4-byte aligned'):
        call(src=4098)
    with pytest.raises(err, match='out is not 4-byte aligned'):
        call(out=8194)
    with pytest.raises(err, match='scratch is not 16-byte aligned'):
        call(scratch=16392)


def test_the_kernels_do_not_spill_and_use_no_float_atomics():
    import shutil
    src = open(os.path.join(abi.CSRC, 'clahe', 'clahe.hip')).read()
    code = re.sub(r'//.*', '', src)
    assert 'atomicAdd(&hist[' in code and not re.search(r'atomic\w*\([^;]*(float|double)', code)
    for name in ('__fdiv_rn', '__ddiv_rn', 'rint(', '__dmul_rn', '__dadd_rn', 'contract(off)'):
        assert name in code, name
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    if not shutil.which(build.HIPCC) and not os.path.exists(build.HIPCC):
        pytest.skip('hipcc not available')
    import kernel_resources
    res = kernel_resources.kernel_resources('clahe/clahe.hip')
    # init, range (2 dtypes), volume range, maps (2), apply (2), rescale
    assert len(res) == 9, sorted(res)
    for name, v in res.items():
        assert v['vgpr_spill_count'] == 0 and v['sgpr_spill_count'] == 0, (name, v)
        assert v['private_segment_fixed_size'] == 0 and v['vgpr_count'] <= 64, (name, v)


# ---- against scikit-image, where it is installed ---------------------------------------------------

def test_against_skimage_where_installed():
    """UNPINNED: skimage's intermediate dtypes moved between releases, so sub-level differences
    are expected; a mapping error would show as O(1).  The largest difference is printed."""
    pytest.importorskip('skimage')
    from skimage import exposure
    im = np.random.default_rng(11).integers(0, 256, (3, 64, 64)).astype(np.float32)
    want = np.zeros(im.shape, np.float32)
    mn, mx = im.min(), im.max()
    for z in range(im.shape[0]):
        want[z] = exposure.equalize_adapthist((im[z] - mn) / (mx - mn), 8).astype('float32')
    diff = float(np.abs(clahe.clahe_numpy(im, 8) - want).max())
    print('largest |clahe_numpy - skimage| = %g' % diff)
    assert diff < 0.05
