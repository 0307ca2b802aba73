"""GPU: the per-op fp32 executor (csrc/generic.hip, csrc/conv_direct.h) layer by layer, through
`Program.forward` and `Program.infer_volume`, on inputs with three different extents.  Cases,
references and bounds: tests/perop_cases.py (what each case exercises is shown on the CPU by
test_perop_cases_host.py).  Bounds: exact equality, the derived gamma_K bound of `conv_case`, the
project's fp32 gate TOL - and ONE measured term, next to the sigmoid head's test.

Every run asserts `ctx.last_path()`: the executor is reached both ways it is reached in use -
FPL_FORCE_PEROP set, and unset on extents that are not cubic."""
import numpy as np
import pytest

from flypylib_amd import _capi, multi_gpu
from tests import perop_cases as pc
from tests.test_gpu_cnn import TOL

pytestmark = pytest.mark.gpu


def _forward(ctx, monkeypatch, graph, x, forced, stride=(1, 1, 1), want_path='perop_f32'):
    if forced:
        monkeypatch.setenv('FPL_FORCE_PEROP', '1')
    else:
        monkeypatch.delenv('FPL_FORCE_PEROP', raising=False)
    prog = _capi.Program(ctx, graph, stride)
    try:
        out = prog.forward(x)
        assert ctx.last_path() == want_path, ctx.last_path()
    finally:
        prog.close()
    return out


def _both_routes(ctx, monkeypatch, graph, x):
    """forced, and reached through the extents: one executor, so one result"""
    assert len(set(x.shape[1:4])) == 3
    forced = _forward(ctx, monkeypatch, graph, x, True)
    natural = _forward(ctx, monkeypatch, graph, x, False)
    assert np.array_equal(forced, natural)
    return forced


@pytest.mark.parametrize('k,cin,cout,variant', pc.CONV_CASES)
def test_convolution_within_the_derived_bound(ctx, monkeypatch, k, cin, cout, variant):
    """|got - float64 oracle| <= gamma_K (|h| (*) |w|) + 2^-126 per output element (perop_cases.conv_case)"""
    c = pc.conv_case(k, cin, cout, variant)
    got = _both_routes(ctx, monkeypatch, c['graph'], c['x'])
    assert got.shape == c['ref'].shape
    err = np.abs(got.astype(np.float64) - c['ref'])
    print('max |err| %.3g, max err / bound %.3g' % (err.max(), np.max(err / c['bound'])))
    assert np.all(err <= c['bound'])


# The kernel's expf and divide (conv_direct.h, apply_act) have no bound the project could derive.
# Measured on this case on an MI355X against the float64 oracle (perop_cases.conv_case(1, 96, 1,
# 'sigmoid'), outputs in 0.43 .. 0.64): largest |got - ref| 6.195e-08, one ulp of the outputs.  Largest
# excess of |got - ref| over the derived bound (conv bound / 4): -6.791e-08 - no element exceeded it.
SIGMOID_MEASURED = 6.2e-8
SIGMOID_TERM = 4 * SIGMOID_MEASURED


def test_sigmoid_head(ctx, monkeypatch):
    """(96, 1), bias, sigmoid.  Bound: the conv bound / 4 (the sigmoid's Lipschitz constant) plus
    SIGMOID_TERM = 4 x the largest error measured on this case (6.195e-08 on an MI355X against the
    float64 oracle; the excess over the conv bound / 4 was -6.791e-08, i.e. none), which may not
    exceed 1e-6."""
    c = pc.conv_case(*pc.SIGMOID_CASE)
    got = _both_routes(ctx, monkeypatch, c['graph'], c['x'])
    err = np.abs(got.astype(np.float64) - c['ref'])
    print('sigmoid head: max |err| %.4g, max excess over the conv bound / 4 %.4g'
          % (err.max(), np.max(err - c['bound'])))
    assert SIGMOID_TERM <= 1e-6
    assert 0.05 < c['ref'].min() and c['ref'].max() < 0.95 and c['ref'].std() > 0.02
    assert np.all(err <= c['bound'] + SIGMOID_TERM)


@pytest.mark.parametrize('name', pc.EXACT_CASES)
def test_exact_ops(ctx, monkeypatch, name):
    g, x, want = pc.exact_case(name)
    got = _both_routes(ctx, monkeypatch, g, x)
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.isfinite(got).all() and np.array_equal(got, want)


# the factories the fp32 MFMA executor takes at these tiles (fpl_mfma_f32_supported): all of them
MFMA_FACTORIES = {n for n, _ in pc.FACTORIES}


@pytest.mark.parametrize('name', [n for n, _ in pc.FACTORIES])
def test_every_factory_forced_onto_the_per_op_executor(ctx, monkeypatch, name):
    g, x, ref = pc.factory_case(name)
    slow = _forward(ctx, monkeypatch, g, x, True)
    assert slow.shape == ref.shape and ref.std() > 1e-4
    err = float(np.max(np.abs(slow - ref)))
    print(name, 'perop_f32 max |err| %.3g' % err)
    assert err < TOL
    # ... and the same program where the dispatcher sends it unforced
    monkeypatch.delenv('FPL_FORCE_PEROP', raising=False)
    prog = _capi.Program(ctx, g)
    try:
        fast = prog.forward(x)
        path = ctx.last_path()
    finally:
        prog.close()
    print(name, 'unforced path', path)
    assert path == ('mfma_f32' if name in MFMA_FACTORIES else 'perop_f32')
    assert np.max(np.abs(fast - ref)) < TOL and np.max(np.abs(fast - slow)) < TOL


def test_infer_volume_on_a_tile_with_three_different_edges(ctx, monkeypatch):
    """vgg_like, tile (30, 26, 22): the dispatcher takes the per-op executor without being told"""
    monkeypatch.delenv('FPL_FORCE_PEROP', raising=False)
    c = pc.NONCUBIC
    g, u8, ref = pc.noncubic_case()
    prog = _capi.Program(ctx, g, c['stride'])
    try:
        kw = dict(mean=c['mean'], std=c['std'])
        got = prog.infer_volume(u8, c['tile'], c['off'], **kw)
        assert ctx.last_path() == 'perop_f32'
        assert got.shape == c['vol'] and got.dtype == np.float32
        err = float(np.max(np.abs(got - ref)))
        print('max |err| over the volume %.3g' % err)
        assert err < TOL and ref[7:-7, 7:-7, 7:-7].std() > 1e-3
        shell = np.ones(c['vol'], bool)
        shell[7:-7, 7:-7, 7:-7] = False
        assert not got[shell].any() and got[~shell].all()              # exactly zero, and only there
        # two z slabs into one destination
        n = multi_gpu.n_tile_rows(c['vol'][0], c['tile'][0], c['off'][0])
        assert n == 3
        dst = np.full(c['vol'], np.nan, np.float32)
        for zr in multi_gpu.slab_partition(n, 2):
            prog.infer_volume(u8, c['tile'], c['off'], z_range=zr, dst=dst, **kw)
            assert ctx.last_path() == 'perop_f32'
        assert np.array_equal(dst, got)
    finally:
        prog.close()
