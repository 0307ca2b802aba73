"""GPU: the fp32 MFMA executor (csrc/conv_mfma_f32.hip) op by op, through `Program.forward` on
cubic inputs with FPL_FORCE_PEROP unset.  Cases, float64 references and derived bounds:
tests/mfma_f32_cases.py (what each case exercises is shown on the CPU by
test_mfma_f32_cases_host.py).  Every run asserts the executor (`ctx.last_path()`) AND the kernels:
the TimedLaunch names and counts of the forward are the ones `predict_launches` states for the
case.  Every program runs on a batch of 3 and on its first element alone."""
import numpy as np
import pytest

from flypylib_amd import _capi
from tests import mfma_f32_cases as mc

pytestmark = pytest.mark.gpu

SWITCHES = ('FPL_FORCE_PEROP', 'FPL_F32_UNFUSED', 'FPL_CONV1_GENERIC')


def _run(ctx, monkeypatch, graph, xs, launches, **env):
    """forward of every x in `xs` on one Program; asserts the path and the launches of each"""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    prog = _capi.Program(ctx, graph)
    outs = []
    try:
        ctx.timing(True)
        for x in xs:
            ctx.timing_reset()
            outs.append(prog.forward(x))
            got = {k: v['launches'] for k, v in ctx.timing_get().items() if v['launches']}
            if launches is None:
                assert ctx.last_path() == 'perop_f32', ctx.last_path()
                assert not any(k.startswith('mfma_') for k in got), got
            else:
                assert ctx.last_path() == 'mfma_f32', ctx.last_path()
                assert got == launches, (got, launches)
    finally:
        ctx.timing(False)
        prog.close()
    return outs


def _both_batches(ctx, monkeypatch, graph, x, launches, **env):
    """the batch of 3, and its first element alone: one result"""
    full, first = _run(ctx, monkeypatch, graph, (x, x[:1]), launches, **env)
    assert full.dtype == np.float32 and np.isfinite(full).all()
    assert np.array_equal(full[:1], first)
    return full


def _within(got, c, label, extra=0.0):
    assert got.shape == c['ref'].shape
    err = np.abs(got.astype(np.float64) - c['ref'])
    print('%s: max |err| %.3g, max err / bound %.3g, max excess %.3g'
          % (label, err.max(), np.max(err / c['bound']), np.max(err - c['bound'])))
    assert np.all(err <= c['bound'] + extra), label


# ---- 1. convolutions alone --------------------------------------------------------------------
@pytest.mark.parametrize('kind,cin,cout,variant', mc.CONV_CASES)
def test_convolution_within_the_derived_bound(ctx, monkeypatch, kind, cin, cout, variant):
    """|got - float64 oracle| <= gamma(k^3 cin + 2) (|s| (|h| (*) |w|) + |shift|) + 2^-126 per output
    element (mfma_f32_cases, module docstring), on every tile edge of the kind.  No measured term
    was needed.  Every conv1 case also runs with FPL_CONV1_GENERIC=1: the weights-in-registers
    kernel (cin 48, up to 48 outputs) gives the generic kernel's bits; elsewhere the switch changes
    nothing."""
    for tile in mc.tiles_of(kind, cin, cout):
        c = mc.conv_case(kind, cin, cout, variant, tile)
        got = _both_batches(ctx, monkeypatch, c['graph'], c['x'], c['launches'])
        _within(got, c, 'tile %d' % tile)
        if kind == 'conv1':
            generic = _both_batches(ctx, monkeypatch, c['graph'], c['x'], c['launches'], FPL_CONV1_GENERIC='1')
            assert np.array_equal(got, generic)


# act_f's expf and division (conv_mfma_f32.hip) have no bound the project could derive.  Measured on
# an MI355X on 2026-10-21 against the float64 oracle, batch 3:
#   mfma_f32_cases.conv_case('conv1', 96, 1, 'sigmoid', 5), outputs in 0.49 .. 0.74: largest |got - ref|
#   1.236e-07, two ulp of the outputs; largest excess over the derived bound (conv bound / 4)
#   -6.442e-07 - no element exceeded it.
SIGMOID_MEASURED = 1.24e-7
#   mfma_f32_cases.fused_case(12, 32, 32, 'relu', 0, 'sigmoid', tile), outputs in 0.17 .. 0.77: largest
#   |got - ref| 1.74e-07 / 1.17e-07 / 1.75e-07 on tiles 10 / 7 / 19; the two-layer bound / 4 is far
#   above that (largest excess -3.49e-05, largest err / bound 0.0025) - no element exceeded it.
SIGMOID_CHAIN_MEASURED = 1.75e-7


def test_sigmoid_head(ctx, monkeypatch):
    """(96, 1), bias, sigmoid: the conv bound / 4 (the sigmoid's Lipschitz constant) plus
    4 x SIGMOID_MEASURED, which may not exceed 1e-6"""
    c = mc.conv_case(*mc.SIGMOID_CASE, mc.SIGMOID_TILE)
    got = _both_batches(ctx, monkeypatch, c['graph'], c['x'], c['launches'])
    err = np.abs(got.astype(np.float64) - c['ref'])
    print('sigmoid head: max |err| %.4g, max excess over the conv bound / 4 %.4g' % (err.max(), np.max(err - c['bound'])))
    assert SIGMOID_MEASURED is not None and 4 * SIGMOID_MEASURED <= 1e-6
    assert 0.05 < c['ref'].min() and c['ref'].max() < 0.95 and c['ref'].std() > 0.02
    _within(got, c, 'sigmoid head', 4 * SIGMOID_MEASURED)
    generic = _both_batches(ctx, monkeypatch, c['graph'], c['x'], c['launches'], FPL_CONV1_GENERIC='1')
    assert np.array_equal(got, generic)


# ---- 2. tap and channel order -----------------------------------------------------------------
@pytest.mark.parametrize('kind,cin,cout,tile,points', mc.TAP_CASES)
def test_tap_position(ctx, monkeypatch, kind, cin, cout, tile, points):
    """a one-hot voxel p in the last input channel lights exactly the outputs p - t in range, each
    holding W[t, cin - 1, :] to within an ulp; everything else is exactly zero"""
    g, W = mc.tap_case(kind, cin, cout, tile)
    xs = []
    for p in points:
        x = np.zeros((1, tile, tile, tile, 1), np.float32)
        x[(0,) + p + (0,)] = 1.0
        xs.append(x)
    outs = _run(ctx, monkeypatch, g, xs, mc.predict_launches(g))
    for p, got in zip(points, outs):
        want, lit = mc.tap_want(W, tile, p)
        assert got.shape == want.shape and np.count_nonzero(want) == lit * cout
        assert np.array_equal(got != 0, want != 0), p
        assert np.max(np.abs(got - want)) <= 2.0 ** -23 * np.abs(want).max(), p


# ---- 3. conv3 -> conv1 (-> pool) --------------------------------------------------------------
def _chain(ctx, monkeypatch, case, measured=0.0):
    for tile in mc.POOL_TILES:
        c = mc.fused_case(*case, tile=tile)
        got = _both_batches(ctx, monkeypatch, c['graph'], c['x'], c['launches'])
        _within(got, c, 'tile %d' % tile, measured)
        if c['launches'] is not None:
            apart = _both_batches(ctx, monkeypatch, c['graph'], c['x'], c['launches_unfused'], FPL_F32_UNFUSED='1')
            assert np.array_equal(got, apart)


@pytest.mark.parametrize('case', mc.FUSED_CASES + mc.STEM_FUSED_CASES,
                         ids=lambda c: '-'.join(str(v) for v in c if v != ''))
def test_fused_chain(ctx, monkeypatch, case):
    """one kernel for conv3 -> conv1 (-> pool): within the two-layer bound of the float64 oracle,
    and the bits of the same program run one kernel per op (FPL_F32_UNFUSED=1)"""
    if case[5] == 'sigmoid':
        _chain(ctx, monkeypatch, case, 4 * (SIGMOID_CHAIN_MEASURED or 0.0))
        assert SIGMOID_CHAIN_MEASURED is not None and 4 * SIGMOID_CHAIN_MEASURED <= 1e-6
    else:
        _chain(ctx, monkeypatch, case)


@pytest.mark.parametrize('case', mc.UNFUSED_CASES + mc.STEM_UNFUSED_CASES,
                         ids=lambda c: '-'.join(str(v) for v in c if v != ''))
def test_chain_that_must_not_fuse(ctx, monkeypatch, case):
    """cout % 4 != 0, different or single m-blocks, a second reader, a 3x3x3 pool (the whole program
    is declined: per-op executor), the stem's 64-wide and unpooled pairs: separate kernels"""
    c = mc.fused_case(*case, tile=7)
    fused = {'mfma_conv3_conv1_f32', 'mfma_conv3_conv1_pool_f32', 'mfma_stem_conv1_pool_f32'}
    assert not fused & set(c['launches'] or ())
    _chain(ctx, monkeypatch, case)


# ---- 4. views, add and pool: exact ------------------------------------------------------------
@pytest.mark.parametrize('name', mc.EXACT_CASES)
def test_exact_views_add_and_pool(ctx, monkeypatch, name):
    """integer inputs, dyadic and integer weights: every sum is exact in float32 in any order
    (test_mfma_f32_cases_host.py proves it), so the result IS numpy's"""
    c = mc.exact_case(name)
    got = _both_batches(ctx, monkeypatch, c['graph'], c['x'], c['launches'])
    assert got.shape == c['want'].shape
    assert np.array_equal(got, c['want'])


# ---- 5. programs the executor declines --------------------------------------------------------
@pytest.mark.parametrize('kind,cin,cout,tile,lifts', mc.DECLINED_CASES + mc.NEIGHBOUR_CASES)
def test_declined_programs_run_on_the_per_op_executor(ctx, monkeypatch, kind, cin, cout, tile, lifts):
    """a 1x1x1 conv with 65..80 or 97..112 outputs, a cin = 1 3x3x3 conv with more than 64, a
    concatenation whose first operand is no multiple of 16 channels in front of a 3x3x3 conv: the
    fp32 MFMA executor has no kernel for them, fpl_mfma_f32_supported says so and the dispatcher
    takes the per-op executor (launches None).  Their neighbours stay on the MFMA kernels."""
    c = mc.conv_case(kind, cin, cout, 'bias', tile, lifts)
    assert (c['launches'] is None) == ((kind, cin, cout, tile, lifts) in mc.DECLINED_CASES)
    got = _both_batches(ctx, monkeypatch, c['graph'], c['x'], c['launches'])
    _within(got, c, 'path %s' % ctx.last_path())


# ---- 6. programs the acceptance rule once took and the launch loop then refused ----------------
MOVED_CASES = ('add_of_an_up_view', 'add_of_a_virtual_concat', 'conv3_of_a_concat_of_a_concat')


def _moved_case(name):
    """graph, x, ref (float64 oracle on the lifts' float32 values: one correctly rounded product per
    element, as the GPU's fma(x, w, 0) gives), bound (perop_cases: gamma(K) on the magnitudes, K =
    k^3 cin + 1 for the conv; one rounding of the sum for the add)"""
    from flypylib_amd.program import LayerGraph
    from tests.perop_cases import TINY, U, _conv64, gamma, np_lift, np_pool, np_up
    seed = 900 + MOVED_CASES.index(name)
    tile = 8 if name == 'add_of_an_up_view' else 3
    g = LayerGraph(tile, seed=seed)
    x = np.random.default_rng(seed).standard_normal((mc.BATCH, tile, tile, tile, 1)).astype(np.float32)

    def lift(node, h, c):
        n = g.conv(node, c, 1)
        return n, np_lift(h, g.weights[n.weight_slots[0]].reshape(-1))

    if name == 'add_of_an_up_view':
        a, ha = lift(g.pool(g.input(), 2), np_pool(x, 2), 16)          # at tile 4
        b, hb = lift(g.input(), x, 16)
        g.finish(g.add(g.up(a, 2), b))
        ha = np_up(ha, 2)
    elif name == 'add_of_a_virtual_concat':
        (a0, h0), (a1, h1), (b, hb) = lift(g.input(), x, 16), lift(g.input(), x, 16), lift(g.input(), x, 32)
        g.finish(g.add(g.concat(a0, a1), b))
        ha = np.concatenate([h0, h1], axis=-1)
    else:
        a, h = lift(g.input(), x, 16)
        conv = g.conv(g.concat(g.concat(a, a), a), 16, 3)
        g.finish(conv)
        h = np.concatenate([h, h, h], axis=-1)
        w = g.weights[conv.weight_slots[0]]
        return dict(graph=g, x=x, ref=_conv64(h, w), bound=gamma(27 * 48 + 1) * _conv64(np.abs(h), np.abs(w)) + TINY)
    ref = ha.astype(np.float64) + hb.astype(np.float64)
    return dict(graph=g, x=x, ref=ref, bound=U * np.abs(ref) + TINY)


@pytest.mark.parametrize('name', MOVED_CASES)
def test_programs_the_launch_loop_used_to_refuse_run_on_the_per_op_executor(ctx, monkeypatch, name):
    """an add of an up-sampled view or of a virtual concatenation, a 3x3x3 conv of a concatenation of
    a concatenation: accepted once and then refused with an error at launch; the plan
    (csrc/mfma_f32_plan.h) declines them, so the dispatcher takes the per-op executor"""
    c = _moved_case(name)
    ops, _, out_tensor, _ = c['graph'].lower_inference()
    assert mc.supported_ops(ops, out_tensor) and mc.launch_refusal(ops, out_tensor) is not None
    got = _both_batches(ctx, monkeypatch, c['graph'], c['x'], None)
    _within(got, c, name)
