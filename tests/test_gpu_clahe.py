"""GPU: fplutils.clahe(device=...) / clahe.clahe_device against the numpy specification
(clahe.clahe_numpy), bit for bit, on the smallest shapes at which the kernels of libfplclahe.so
can go wrong.  Every case first proves from the specification's trace (or from its own input)
that it exercises what it is named for.  The references are computed once per case and shared."""
import functools
import math

import numpy as np
import pytest

from flypylib_amd import clahe, fplutils

pytestmark = pytest.mark.gpu


def _u8(seed, shape, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(np.uint8)


def _two_levels():
    im = np.full((1, 32, 32), 40, np.uint8)
    im.reshape(-1)[np.random.default_rng(5).permutation(1024)[:51]] = 200      # 5 %
    return im


def _ramp_and_level():
    """a ramp over the upper three quarters of the range, one dominant level on a fifth of the
    pixels (seed 0, found on the CPU), one pixel at 0: with 4 or 8 bins clipped at a quarter of the
    tile, the lowest bin takes the excess one count per outer pass"""
    im = (64 + np.arange(32 * 32) * 192 // 1024).reshape(1, 32, 32).astype(np.uint8)
    im[np.random.default_rng(0).random(im.shape) < 0.2] = 255
    im[0, 0, 0] = 0
    return im


def _slices_differ():
    im = np.empty((3, 16, 16), np.uint8)
    im[0] = _u8(1, (16, 16))
    im[1] = 100
    im[2] = _u8(2, (16, 16), 50, 61)
    return im


def _few_ulps():
    """float32 values within 7 ulp below -1, slice 1 on a sub-range of slice 0's"""
    rng = np.random.default_rng(3)
    steps = np.stack([rng.integers(0, 8, (16, 16)), rng.integers(2, 6, (16, 16))])
    steps[0, 0, :2] = (0, 7)
    steps[1, 0, :2] = (2, 5)
    v = np.float32(-1.0)
    table = [v]
    for _ in range(7):
        table.append(np.nextafter(table[-1], np.float32(-2.0)))
    return np.array(table, np.float32)[steps]


def _thirds():
    """float32 multiples of fl(1/3) from -3 to 4: both signs, inexact divides"""
    rng = np.random.default_rng(4)
    j = rng.integers(-3, 5, (2, 16, 16))
    j[0, 0, :2] = (-3, 4)
    j[1] = np.clip(j[1], -2, 2)
    j[1, 0, :2] = (-2, 2)
    return (j.astype(np.float32) * np.float32(1.0 / 3.0)).astype(np.float32)


def _ties():
    """slice 0 spans [0, 2^15], so s = v / 2^15 is exact; slice 1 spans [0, 32766], so step (c)
    computes fl(fl(v / 32766) * 16383), which is v / 2 in exact arithmetic: odd v can land on x.5"""
    rng = np.random.default_rng(6)
    im = np.empty((2, 16, 16), np.float32)
    im[0] = rng.integers(0, 32769, (16, 16))
    im[0, 0, :2] = (0, 32768)
    im[1] = rng.integers(0, 16383, (16, 16)) * 2 + 1
    im[1, 0, :2] = (0, 32766)
    return im


def _tie_pixels(im):
    """the x of step (c) that are exactly some n + 0.5, as the specification computes them"""
    mn, mx = im.min(), im.max()
    found = []
    for z in range(im.shape[0]):
        s = (im[z] - mn) / np.float32(mx - mn)
        lo, hi = np.float64(s.min()), np.float64(s.max())
        x = (s.astype(np.float64) - lo) / (hi - lo) * 16383.0
        found.extend(x[x - np.floor(x) == 0.5])
    return np.array(found)


# name -> (volume, kernel_size, keywords of clahe, what the trace / input must show)
CASES = {
    'one-tile': (lambda: _u8(10, (1, 8, 8)), 8, {}, lambda t, im: t['nt'] == (1, 1)),
    'ragged': (lambda: _u8(11, (2, 13, 11)), (4, 5), {},
               lambda t, im: t['nt'] == (4, 3) and 13 % 4 and 11 % 5),
    'odd-k': (lambda: _u8(12, (1, 9, 10)), (3, 5), {}, lambda t, im: 3 // 2 != math.ceil(3 / 2)),
    'deep-reflect-5': (lambda: _u8(13, (1, 5, 5)), 4, {}, lambda t, im: t['max_pad_ratio'] > 1),
    'deep-reflect-6': (lambda: _u8(14, (1, 6, 6)), 8, {}, lambda t, im: t['max_pad_ratio'] > 1),
    'k1': (lambda: _u8(15, (1, 6, 7)), 1, {}, lambda t, im: clahe.clip_count(0.01, 1, 1) == 1),
    'big-tile': (lambda: _u8(16, (1, 48, 48)), 40, {}, lambda t, im: 40 * 40 > 256 and t['nt'] == (2, 2)),
    'kernel-size-none': (lambda: _u8(17, (2, 24, 40)), None, {}, lambda t, im: t['nt'] == (8, 8)),
    'peaked-two-levels': (_two_levels, 16, {},
                          lambda t, im: t['tiles_in_while'] > 0 and len(np.unique(im)) == 2
                          and np.count_nonzero(im == 40) == 973),
    'peaked-passes-4': (_ramp_and_level, 16, dict(clip_limit=0.25, nbins=4),
                        lambda t, im: t['max_passes'] >= 2),
    'peaked-passes-8': (_ramp_and_level, 16, dict(clip_limit=0.25, nbins=8),
                        lambda t, im: t['max_passes'] >= 2),
    'no-clip-0': (lambda: _u8(18, (1, 16, 16)), 8, dict(clip_limit=0),
                  lambda t, im: t['tiles_in_while'] == 0),
    'no-clip-1': (lambda: _u8(18, (1, 16, 16)), 8, dict(clip_limit=1.0),
                  lambda t, im: t['tiles_in_while'] == 0),
    'nbins-2': (lambda: _u8(19, (1, 16, 16)), 8, dict(nbins=2), lambda t, im: True),
    'nbins-64': (lambda: _u8(19, (1, 16, 16)), 8, dict(nbins=64), lambda t, im: True),
    'nbins-255': (lambda: _u8(19, (1, 16, 16)), 8, dict(nbins=255), lambda t, im: True),
    'nbins-256': (lambda: _u8(19, (1, 16, 16)), 8, dict(nbins=256), lambda t, im: True),
    'slices-differ': (_slices_differ, 8, {},
                      lambda t, im: im[1].min() == im[1].max() and im[2].max() - im[2].min() == 10),
    'many-slices': (lambda: _u8(20, (70, 8, 8)), 4, {}, lambda t, im: im.shape[0] > 64),
    'monotone-range-ulps': (_few_ulps, 8, {},
                            lambda t, im: im.max() < 0 and len(np.unique(im)) == 8
                            and np.nextafter(im.max(), np.float32(-2)) in im),
    'monotone-range-thirds': (_thirds, 8, {}, lambda t, im: im.min() < 0 < im.max()),
    'ties': (_ties, 8, {},
             lambda t, im: len(_tie_pixels(im)) >= 4 and (np.floor(_tie_pixels(im)) % 2 == 0).any()),
    'float32-input': (lambda: _u8(21, (2, 16, 16)).astype(np.float32), 8, {}, lambda t, im: True),
    'zero-mean': (lambda: _u8(22, (2, 13, 11)), (4, 5), dict(zero_mean=True), lambda t, im: True),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(input, kernel_size, keywords, the specification's result, its trace): computed once, and
    read-only"""
    make, k, kw, _ = CASES[name]
    im, trace = make(), {}
    want = clahe.clahe_numpy(im, k, trace=trace, **kw)
    im.setflags(write=False)
    want.setflags(write=False)
    return im, k, kw, want, trace


def check_case_is_what_it_says(name):
    """the condition of CASES on the specification alone (no GPU): also run on the CPU"""
    im, _, _, want, trace = _case(name)
    assert CASES[name][3](trace, im), (name, trace)
    assert want.dtype == np.float32 and want.shape == im.shape


@pytest.fixture(scope='module')
def dev():
    import torch
    return torch.device('cuda', 0)


@pytest.mark.parametrize('name', sorted(CASES))
def test_device_equals_the_specification(name, dev):
    import torch
    check_case_is_what_it_says(name)
    im, k, kw, want, _ = _case(name)
    got = fplutils.clahe(np.array(im), k, None, kw.get('zero_mean', False), 0,
                         **{a: v for a, v in kw.items() if a != 'zero_mean'})
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and got.device == dev
    assert got.is_contiguous() and tuple(got.shape) == im.shape
    got = got.cpu().numpy()
    assert np.array_equal(got, want), (name, float(np.abs(got - want).max()),
                                       int(np.count_nonzero(got != want)))


def test_uint8_and_float32_of_the_same_values_agree(dev):
    im = _case('ragged')[0]
    a = fplutils.clahe(np.array(im), (4, 5), device=0)
    b = fplutils.clahe(im.astype(np.float32), (4, 5), device=0)
    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert np.array_equal(a.cpu().numpy(), _case('ragged')[3])


def test_host_input_equals_resident_input(dev):
    import torch
    im, k, _, want, _ = _case('slices-differ')
    res = torch.from_numpy(np.array(im)).to(dev)
    a = fplutils.clahe(res, k, device=0)
    b = fplutils.clahe(res, k, device=True)
    for got in (a, b):
        assert got.is_contiguous() and got.dtype == torch.float32 and got.device == dev
        assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(res.cpu(), torch.from_numpy(np.array(im)))      # the input is not written


@pytest.mark.parametrize('dtype,start', [('float32', 1), ('uint8', 1), ('uint8', 3)])
def test_a_view_at_an_element_offset(dev, dtype, start):
    import torch
    name = 'float32-input' if dtype == 'float32' else 'ragged'
    im, k, _, want, _ = _case(name)
    flat = torch.zeros(im.size + start + 5, dtype=getattr(torch, dtype), device=dev)
    assert flat.data_ptr() % 16 == 0
    view = flat[start:start + im.size].view(im.shape)
    view.copy_(torch.from_numpy(np.array(im)))
    assert view.is_contiguous() and view.data_ptr() == flat.data_ptr() + start * flat.element_size()
    assert np.array_equal(fplutils.clahe(view, k, device=0).cpu().numpy(), want)


def test_nothing_outside_the_result_or_the_scratch_is_written(dev):
    import torch
    from flypylib_amd import _clahecapi
    im, k, _, want, _ = _case('ragged')
    n, pad = im.size, 64
    big = torch.full((n + 2 * pad,), -7.25, dtype=torch.float32, device=dev)
    out = big[pad:pad + n].view(im.shape)
    need = _clahecapi.scratch_bytes(*im.shape, *k, 256)
    assert need % 16 == 0 and need >= _clahecapi.STATUS_BYTES + 16 * im.shape[0] + 2 * n
    scratch = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=dev)
    got = clahe.clahe_device(np.array(im), k, device=0, out=out, scratch=scratch)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize(dev)
    assert np.array_equal(got.cpu().numpy(), want)
    host = big.cpu().numpy()
    assert (host[:pad] == -7.25).all() and (host[pad + n:] == -7.25).all()
    assert (scratch[need:].cpu().numpy() == 0xA5).all()


def test_two_calls_give_equal_bytes(dev):
    for name in ('peaked-two-levels', 'peaked-passes-4'):
        im, k, kw, want, _ = _case(name)
        a = clahe.clahe_device(np.array(im), k, device=0, **kw).cpu().numpy()
        b = clahe.clahe_device(np.array(im), k, device=0, **kw).cpu().numpy()
        assert a.tobytes() == b.tobytes() == want.tobytes()


def test_a_constant_volume_raises_as_on_the_host(dev):
    with pytest.raises(ValueError, match='the volume is constant'):
        fplutils.clahe(np.full((2, 8, 8), 9, np.uint8), 4, device=0)
