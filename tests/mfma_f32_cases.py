"""Cases, float64 references and bounds of the op-by-op tests of the fp32 MFMA executor
(csrc/mfma_f32_plan.h: the plan that says what it runs and how; csrc/conv_mfma_f32.hip:
fpl_forward_mfma_f32_dims, which launches from it, and the inference kernels):
test_mfma_f32_cases_host.py (what each case exercises and that its bound is
sound, on the CPU) and test_gpu_mfma_f32.py.  Nothing here touches a GPU.

THE BOUND of one convolution (`conv_case`), from the kernels' own rounding sequence:

  * pack_conv3_f32 / pack_stem_f32 / pack_conv1_f32 store fl(W * scale): one rounding per weight.
    `scale` is 1 (the product is exact) or the folded BatchNorm scale, itself the float32 rounding
    of gamma / sqrt(var + eps): one more.  Two roundings per weight at the most.
  * every kernel starts its accumulator at `shift` (conv3_f32, stem_cin1_f32 and conv1_f32 alike;
    store_quad only applies the activation) and then adds one product per (tap, channel) with a
    chain of v_mfma_f32_16x16x4_f32, each step a fused multiply-add: k^3 * cin roundings for the
    real terms.  `shift` is the bias (exact) or the folded BatchNorm shift (rounded once).
  * the channels and taps that pad a K-block to 16 multiply zeros: fma(0, w, acc) = acc, exact.

So every term of  shift + sum_i h_i * (W_i * s)  passes through at most K = k^3 * cin + 2
roundings, and by Higham's Lemma 3.1, whatever the order of the additions,

    |computed - exact| <= gamma(K) * (|s| * (|h| (*) |W|) + |shift|),   gamma(K) = K u / (1 - K u).

2^-126 is added as an absolute floor.  ReLU is 1-Lipschitz; the sigmoid has Lipschitz constant 1/4
and its own expf and division carry a measured term that lives next to its test.  The per-op
executor's bound (perop_cases.conv_case) has K = k^3 * cin + 1 and a separate affine term; this one
is a little looser where there is no BatchNorm and tighter where there is.

TWO LAYERS (`fused_case`): with a = act(conv3(h)) and B1 the bound above for it,
|conv1(a_gpu) - conv1(a)| <= B1 (*) |W1| for the exact conv1, and the conv1's own rounding is
gamma(K2) * ((|a| + B1) (*) |W1| + |b1|), K2 = c3 + 2, since |a_gpu| <= |a| + B1.  The bound is
their sum; a max pool takes the largest bound of its window (|max a - max b| <= max |a - b|).

`supported_ops`, `fusion` and `predict_launches_ops` restate, in plain Python, the rules that stood
inline in conv_mfma_f32.hip before the plan header existed: which programs the executor takes, and
which TimedLaunch names, and how many of each, a program must produce.  They are the record the
header is held to (test_mfma_f32_plan_host.py), not a reading of it.  A case that lands on another
kernel than intended fails on that."""
import collections
import functools

import numpy as np

from flypylib_amd.program import (ACT_NONE, ACT_RELU, BN_EPS, LayerGraph, OP_ADD, OP_CONCAT, OP_CONV, OP_CROP,
                                  OP_DECONV, OP_DILATED, OP_DOWN, OP_POOL, OP_UP)
from tests.perop_cases import TINY, U, _W5, _W7, _conv64, _ints, gamma, np_crop, np_lift, np_pool, np_up

BATCH = 3                          # every GPU run is made on x and on x[:1]
CACHE = 6                          # cases are used by neighbouring tests only; the large ones are 100 MB


# ---- the dispatcher, restated -----------------------------------------------------------------
def _mb(c):
    return (c + 15) // 16


def _conv3m(o):
    return o['kind'] == OP_CONV and o['k'] == 3 and o['cin'] > 1


def concats_written(ops, out_tensor):
    """per op: a concatenation that is written out.  In a program that holds a Conv3DTranspose, one
    whose readers are not all multi-channel 3x3x3 convs (the program's output counts as a reader)"""
    other = {out_tensor}
    for o in ops:
        if not _conv3m(o):
            other.update(t for t in (o['src0'], o['src1']) if t >= 0)
    deconv = any(o['kind'] == OP_DECONV for o in ops)
    return [deconv and o['kind'] == OP_CONCAT and o['dst'] in other for o in ops]


def supported_ops(ops, out_tensor):
    """the acceptance rule of the fp32 MFMA executor as it stood inline in conv_mfma_f32.hip before
    csrc/mfma_f32_plan.h existed (fpl_mfma_f32_supported with its concats_written), restated"""
    written = concats_written(ops, out_tensor)
    view, ch, cat_first = {0: 0}, {0: 1}, {0: 0}
    for i, o in enumerate(ops):
        kind, s0, s1, d = o['kind'], o['src0'], o['src1'], o['dst']
        v0, v1 = view[s0], view[s1] if s1 >= 0 else 0
        view[d], cat_first[d] = 0, 0
        ch[d] = o['cout'] if kind in (OP_CONV, OP_DECONV, OP_DOWN, OP_DILATED) else ch[s0]
        if kind == OP_CONCAT:
            ch[d], cat_first[d] = ch[s0] + ch[s1], ch[s0]
            if written[i]:
                if v0 == 2 or v1 == 2:
                    return False
            else:
                view[d] = 2
        elif kind in (OP_UP, OP_CROP):
            if v0:
                return False
            view[d] = 1
        elif _conv3m(o):
            if v1 or cat_first[s0] % 16:
                return False
        elif kind == OP_ADD:
            pass
        elif v0 or v1:
            return False
        if d == out_tensor and view[d]:
            return False
        if kind == OP_POOL and tuple(o['p'][:3]) != (2, 2, 2):
            return False
        if kind == OP_UP and tuple(o['p'][:3]) not in ((1, 1, 1), (2, 2, 2)):
            return False
        if kind == OP_CROP and len(set(o['p'])) != 1:
            return False
        if kind == OP_CONV and o['k'] == 3 and (o['cout'] > 256 or o['cin'] > 192 or (o['cin'] == 1 and o['cout'] > 64)):
            return False
        if kind == OP_CONV and o['k'] == 1 and _mb(o['cout']) not in (1, 2, 3, 4, 6, 8):
            return False
        if kind in (OP_DECONV, OP_DOWN) and (o['k'] != 2 or o['cin'] > 256 or o['cout'] > 256):
            return False
        if kind == OP_DILATED and (o['k'] != 3 or o['cout'] > 256 or o['cin'] > 192):
            return False
    return True


def supported(graph):
    """`supported_ops` of a graph's lowered program"""
    ops, _, out_tensor, _ = graph.lower_inference()
    return supported_ops(ops, out_tensor)


def launch_refusal(ops, out_tensor):
    """For a program `supported_ops` accepts: the error with which the launch loop of that time then
    refused it (its structural FPL_REQUIREs, restated with its view bookkeeping), or None where it
    ran.  The dispatchers had picked the executor by then, so such a call failed; the plan declines
    these programs and they run on the per-op executor."""
    written = concats_written(ops, out_tensor)
    buf = dict(p=True, up=1, crop=0)
    view, made_by = {0: buf}, {}
    for i, o in enumerate(ops):
        kind, d = o['kind'], o['dst']
        a, b = view[o['src0']], view.get(o['src1'])
        made_by[d] = o
        if kind in (OP_UP, OP_CROP):
            if a['up'] != 1 or a['crop'] != 0:
                return 'nested views'
            view[d] = dict(a, up=o['p'][0]) if kind == OP_UP else dict(a, crop=o['p'][0])
            continue
        if kind == OP_CONCAT:
            if written[i] and not (a['p'] and b['p']):
                return 'concatenate of a concatenation'
            view[d] = buf if written[i] else dict(a, p=False)
            continue
        if kind == OP_ADD:
            if not (a['p'] and b['p'] and a['up'] == 1 and b['up'] == 1):
                return 'add of incompatible tensors'
        elif _conv3m(o):
            cat = made_by.get(o['src0'])
            if cat is not None and cat['kind'] == OP_CONCAT:
                if not (view[cat['src0']]['p'] and view[cat['src1']]['p']):
                    return 'unsupported concat'
            elif not a['p']:
                return 'conv3 of an unmaterialised tensor'
        elif not (a['p'] and a['up'] == 1 and a['crop'] == 0):
            return 'of a view'
        view[d] = buf
    return None


def fusion(ops, i, out_tensor):
    """the fusion rule for the 3x3x3 conv ops[i], as fpl_forward_mfma_f32_dims stated it inline: (fuses
    the 1x1x1 conv that follows, fuses the pool after that)"""
    op = ops[i]
    if op['kind'] != OP_CONV or op['k'] != 3 or i + 1 >= len(ops):
        return False, False

    def readers(t):
        return int(t == out_tensor) + sum((o['src0'] == t) + (o['src1'] == t) for o in ops)
    n1 = ops[i + 1]
    mb0, mb1 = _mb(op['cout']), _mb(n1['cout'])
    pair_ok = mb0 == mb1 and mb0 in (2, 3, 4) and op['cout'] % 4 == 0
    if not (n1['kind'] == OP_CONV and n1['k'] == 1 and n1['src0'] == op['dst'] and readers(op['dst']) == 1
            and pair_ok and op['act'] in (ACT_NONE, ACT_RELU)):
        return False, False
    pool = False
    if i + 2 < len(ops):
        n2 = ops[i + 2]
        pool = (n2['kind'] == OP_POOL and n2['src0'] == n1['dst'] and readers(n1['dst']) == 1
                and tuple(n2['p'][:3]) == (2, 2, 2) and n1['act'] in (ACT_NONE, ACT_RELU))
    if op['cin'] == 1 and (not pool or mb0 == 4):           # the cin = 1 form exists only pooled, mb 2 / 3
        return False, False
    return True, pool


def predict_launches(graph, unfused=False):
    """`predict_launches_ops` of a graph's lowered program"""
    ops, _, out_tensor, _ = graph.lower_inference()
    return predict_launches_ops(ops, out_tensor, unfused)


def predict_launches_ops(ops, out_tensor, unfused=False):
    """{TimedLaunch name: launches} of one forward on the fp32 MFMA executor, or None where
    `supported_ops` declines the program (the dispatcher then takes the per-op executor)"""
    if not supported_ops(ops, out_tensor):
        return None
    written = concats_written(ops, out_tensor)
    n = collections.Counter()
    i = 0
    while i < len(ops):
        o = ops[i]
        if o['kind'] == OP_POOL:
            n['mfma_pool_f32'] += 1
        elif o['kind'] == OP_ADD:
            n['mfma_add_f32'] += 1
        elif o['kind'] == OP_DECONV:
            n['mfma_deconv2_f32'] += 1
        elif o['kind'] == OP_DOWN:
            n['mfma_down2_f32'] += 1
        elif o['kind'] == OP_DILATED:
            n['mfma_atrous3_f32'] += -(-o['cout'] // 64)             # slices of 64 outputs
        elif o['kind'] == OP_CONCAT and written[i]:
            n['mfma_concat_f32'] += 1
        elif o['kind'] == OP_CONV and o['k'] == 1:
            n['mfma_conv1_f32'] += 1
        elif o['kind'] == OP_CONV:
            f1, fp = (False, False) if unfused else fusion(ops, i, out_tensor)
            if f1:
                n['mfma_stem_conv1_pool_f32' if o['cin'] == 1 else
                  'mfma_conv3_conv1_pool_f32' if fp else 'mfma_conv3_conv1_f32'] += 1
                i += 2 if fp else 1
            elif o['cin'] == 1:
                n['mfma_stem_f32'] += 1
            else:
                n['mfma_conv3_f32'] += -(-o['cout'] // 64)           # slices of 64 outputs
        else:
            assert o['kind'] in (OP_UP, OP_CROP, OP_CONCAT), o['kind']  # views: no launch
        i += 1
    return dict(n)


# ---- 1. convolutions alone --------------------------------------------------------------------
CONV3_PAIRS = [(2, 1), (3, 5), (16, 16), (17, 33), (20, 64), (48, 65), (96, 48), (192, 16), (32, 130)]
STEM_COUTS = [1, 5, 16, 17, 48, 64]
STEM_67 = (5, 17)                  # the two channel counts that also run the 67^3 tile
CONV1_PAIRS = [(1, 48), (5, 7), (47, 48), (48, 48), (49, 48), (48, 17), (48, 64), (96, 1), (96, 96), (20, 128)]
VARIANTS = ('none', 'bias', 'relu', 'bn_relu')
CONV_CASES = ([('conv3', ci, co, v) for ci, co in CONV3_PAIRS for v in VARIANTS]
              + [('stem', 1, co, v) for co in STEM_COUTS for v in VARIANTS]
              + [('conv1', ci, co, v) for ci, co in CONV1_PAIRS for v in VARIANTS])
SIGMOID_CASE = ('conv1', 96, 1, 'sigmoid')
SIGMOID_TILE = 5


def tiles_of(kind, cin, cout):
    """input edges.  conv3 blocks are 4 x 4 x 16 outputs (3: one output; 7: 5^3, ragged rows and
    waves; 19: 17^3, across the 16-column edge); stem blocks 4 x 8 x 64 (11: 9^3, across the 8-row
    edge; 67: 65^3, across the 64-column edge); conv1 groups are 16 voxels, 4 waves a block
    (1: M = batch, under one group)"""
    if kind == 'conv3':
        return (7,) if cin >= 96 else (3, 7, 19)
    if kind == 'stem':
        return (3, 11, 67) if cout in STEM_67 else (3, 11)
    return (1, 3, 5)


def lifts_of(cin):
    """channel counts of the 1x1x1 lifts in front of the convolution under test.  The 1x1x1 kernels
    end at 128 outputs, so 192 channels are a (virtual) concatenation of two lifts to 96"""
    return () if cin == 1 else (96, 96) if cin == 192 else (cin,)


# A worst-case bound grows with K while random signs let the outputs cancel: from K = 27 * 96 on,
# gamma(K) * sum |terms| of zero-mean data is no smaller than 1e-3 of the outputs themselves, and
# the bound would say less than the gate it replaces.  Those cases (conv3 with 96 and 192 inputs)
# get data that does not cancel: inputs of mean 1, positive lift weights, and 3x3x3 weights moved
# by half their range, up for even output channels and down for odd ones.
COHERENT_K = 1500


def _lifted(g, x, lifts, positive=False):
    """(node, the float32 tensor the node holds): lifts of the input, concatenated.  One product per
    element, correctly rounded: what the GPU's lift gives too (fma(x, w, 0))"""
    if not lifts:
        return g.input(), x
    nodes = [g.conv(g.input(), c, 1) for c in lifts]
    if positive:
        for n in nodes:
            g.weights[n.weight_slots[0]] = np.abs(g.weights[n.weight_slots[0]])
    hs = [np_lift(x, g.weights[n.weight_slots[0]].reshape(-1)) for n in nodes]
    node = nodes[0]
    for n in nodes[1:]:
        node = g.concat(node, n)
    return node, np.concatenate(hs, axis=-1)


@functools.lru_cache(maxsize=CACHE)
def conv_case(kind, cin, cout, variant, tile, lifts=None):
    """One convolution - 'conv3' (3x3x3, cin > 1), 'stem' (3x3x3, cin = 1) or 'conv1' - behind its
    lifts, on (BATCH, tile, tile, tile).  The weights depend on (kind, cin, cout, variant) alone.

      graph, x    what the GPU runs
      h           the float32 input of the convolution under test
      ref         float64 oracle of the convolution (+ bias / BatchNorm / activation) on `h`
      bound       per output element (module docstring); for 'sigmoid' the conv bound / 4
      launches    predict_launches(graph)
    """
    k = 1 if kind == 'conv1' else 3
    lifts = lifts_of(cin) if lifts is None else lifts
    assert sum(lifts) == (cin if lifts else 0) and (kind == 'stem') == (k == 3 and cin == 1)
    seed = 7000 * k + 13 * cin + cout + 100003 * len(lifts)
    rng = np.random.default_rng(seed)
    g = LayerGraph(tile, seed=seed)
    x = np.random.default_rng(seed + tile).standard_normal((BATCH, tile, tile, tile, 1)).astype(np.float32)
    coherent = k ** 3 * cin > COHERENT_K
    if coherent:
        x = x + np.float32(1.0)
    node, h = _lifted(g, x, lifts, positive=coherent)
    biased = variant in ('bias', 'sigmoid')
    conv = g.conv(node, cout, k, use_bias=biased, activation='sigmoid' if variant == 'sigmoid' else None)
    if coherent:
        w = g.weights[conv.weight_slots[0]]
        sign = np.where(np.arange(cout) % 2, -1.0, 1.0)
        g.weights[conv.weight_slots[0]] = (w + 0.5 * np.abs(w).max() * sign).astype(np.float32)
    y = conv
    if variant == 'relu':
        y = g.relu(y)
    elif variant == 'bn_relu':
        y = g.bn_relu(y)
    g.finish(y)
    g.randomize_bn(seed)
    if biased:
        g.weights[conv.weight_slots[1]] = rng.uniform(-0.5, 0.5, cout).astype(np.float32)
    w = g.weights[conv.weight_slots[0]]
    c = _conv64(h, w)
    mag = _conv64(np.abs(h), np.abs(w))
    s, t = np.ones(cout), np.zeros(cout)
    if biased:
        t = g.weights[conv.weight_slots[1]].astype(np.float64)
    if variant == 'bn_relu':
        gm, bt, mu, var = (g.weights[i].astype(np.float64) for i in g.nodes[conv.idx + 1].weight_slots)
        s = gm / np.sqrt(var + BN_EPS)
        t = bt - mu * s
    K = k ** 3 * cin + 2
    ref = c * s + t
    bound = gamma(K) * (np.abs(s) * mag + np.abs(t))
    if variant in ('relu', 'bn_relu'):
        ref = np.maximum(ref, 0.0)
    elif variant == 'sigmoid':
        ref = 1.0 / (1.0 + np.exp(-ref))
        bound = bound / 4.0
    return dict(graph=g, x=x, h=h, w=w, ref=ref, bound=bound + TINY, K=K, mag=mag, conv=conv, scale=s, shift=t,
                launches=predict_launches(g))


def conv_facts(kind, cin, cout, tile):
    """what the kernel's tiling meets on this case"""
    k = 1 if kind == 'conv1' else 3
    od = tile - k + 1
    f = dict(out=od, mb=_mb(min(cout, 64)) if kind != 'conv1' else _mb(cout), slices=-(-cout // 64) if kind == 'conv3' else 1,
             chunks=sum(-(-c // 16) for c in lifts_of(cin)), ragged_cout=cout % 4 != 0, ragged_cin=cin % 4 != 0)
    if kind == 'conv3':
        f.update(blocks=(-(-od // 4), -(-od // 4), -(-od // 16)), idle_waves=od % 4 != 0)
    elif kind == 'stem':
        f.update(blocks=(-(-od // 4), -(-od // 8), -(-od // 64)))
    else:
        f.update(groups={b: -(-(b * od ** 3) // 16) for b in (1, BATCH)}, tail={b: (b * od ** 3) % 16 for b in (1, BATCH)},
                 wreg=cin == 48 and _mb(cout) <= 3)
    return f


# ---- 2. tap and channel order -----------------------------------------------------------------
# (kind, cin, cout, tile, one-hot voxels): a corner, the opposite corner, and two interior voxels:
# one whose lit outputs end on the last row / plane / column of the first block, and its neighbour,
# whose outputs lie on both sides of that block edge
TAP_CASES = [('conv3', 5, 6, 19, ((0, 0, 0), (18, 18, 18), (3, 3, 15), (4, 4, 16))),
             ('conv3', 20, 6, 19, ((0, 0, 0), (18, 18, 18), (3, 3, 15), (4, 4, 16))),
             ('conv3', 33, 70, 19, ((0, 0, 0), (18, 18, 18), (3, 3, 15), (4, 4, 16))),
             ('stem', 1, 3, 67, ((0, 0, 0), (66, 66, 66), (3, 7, 63), (4, 8, 64))),
             ('stem', 1, 40, 11, ((0, 0, 0), (10, 10, 10), (3, 7, 5), (4, 8, 6)))]


@functools.lru_cache(maxsize=CACHE)
def tap_case(kind, cin, cout, tile):
    """(graph, W (3, 3, 3, cin, cout)): the lift sends the input to the LAST of `cin` channels with
    weight 1 and to no other; the 3x3x3 weights are all distinct"""
    g = LayerGraph(tile, seed=cin + cout)
    node = g.input()
    if cin > 1:
        node = g.conv(node, cin, 1)
        one = np.zeros((1, 1, 1, 1, cin), np.float32)
        one[..., cin - 1] = 1.0
        g.weights[node.weight_slots[0]] = one
    conv = g.conv(node, cout, 3)
    n = 27 * cin * cout
    W = ((np.random.default_rng(n).permutation(n) + 1.0) / n).astype(np.float32).reshape(3, 3, 3, cin, cout)
    assert len(np.unique(W)) == n
    g.weights[conv.weight_slots[0]] = W
    g.finish(conv)
    return g, W


def tap_want(W, tile, p):
    """a one-hot voxel p in input channel cin - 1: output p - t holds W[t, cin - 1, :]"""
    od = tile - 2
    want = np.zeros((1, od, od, od, W.shape[4]), np.float32)
    lit = 0
    for t in np.ndindex(3, 3, 3):
        o = tuple(pi - ti for pi, ti in zip(p, t))
        if all(0 <= oi < od for oi in o):
            want[(0,) + o] = W[t + (W.shape[3] - 1,)]
            lit += 1
    return want, lit


# ---- 3. conv3 -> conv1 (-> pool) --------------------------------------------------------------
FUSED_PAIRS = [(32, 32), (20, 17), (48, 48), (36, 33), (64, 64), (52, 49)]
FUSE_CIN = 12                      # channels in front of the multi-channel conv3: one ragged chunk
POOL_TILES = (10, 7, 19)           # conv outputs 8, 5 (the odd plane, row and column are dropped), 17
ACTS = ('relu', 'none')
# (cin, c3, c1, act, pool, flavour)
FUSED_CASES = ([(FUSE_CIN, a, b, act, pool, '') for a, b in FUSED_PAIRS for act in ACTS for pool in (0, 2)]
               + [(FUSE_CIN, 32, 32, 'relu', 0, 'sigmoid')])
UNFUSED_CASES = [(FUSE_CIN, 18, 32, 'relu', 2, ''),            # cout % 4 != 0
                 (FUSE_CIN, 32, 48, 'relu', 2, ''),            # mb differs
                 (FUSE_CIN, 16, 16, 'relu', 2, ''),            # mb is 1
                 (FUSE_CIN, 32, 32, 'relu', 0, 'second_reader'),
                 (FUSE_CIN, 32, 32, 'relu', 3, '')]            # a 3x3x3 pool: declined whole (per-op executor)
STEM_FUSED_CASES = [(1, 32, 32, 'relu', 2, ''), (1, 48, 48, 'relu', 2, ''), (1, 48, 48, 'none', 2, ''),
                    (1, 20, 17, 'relu', 2, '')]
STEM_UNFUSED_CASES = [(1, 64, 64, 'relu', 2, ''), (1, 32, 32, 'relu', 0, ''), (1, 48, 48, 'none', 0, '')]


def _act(a, act):
    return np.maximum(a, 0.0) if act == 'relu' else a


@functools.lru_cache(maxsize=CACHE)
def fused_case(cin, c3, c1, act, pool, flavour, tile):
    """lift(cin) -> conv3(c3) + bias, act -> conv1(c1) + bias, act (-> pool).  flavour 'sigmoid': the
    conv1 carries a sigmoid; 'second_reader': add(conv1 output, conv3 output) follows.  Returns
    graph, x, ref (float64), bound (module docstring), launches, launches_unfused"""
    seed = 31 * c3 + c1 + 1000 * cin
    rng = np.random.default_rng(seed)
    g = LayerGraph(tile, seed=seed)
    x = np.random.default_rng(seed + tile).standard_normal((BATCH, tile, tile, tile, 1)).astype(np.float32)
    node, h = _lifted(g, x, () if cin == 1 else (cin,))
    act_name = None if act == 'none' else act
    n3 = g.conv(node, c3, 3, use_bias=True, activation=act_name)
    n1 = g.conv(n3, c1, 1, use_bias=True, activation='sigmoid' if flavour == 'sigmoid' else act_name)
    y = n1
    if flavour == 'second_reader':
        y = g.add(n1, n3)
    if pool:
        y = g.pool(y, pool)
    g.finish(y)
    for n, c in ((n3, c3), (n1, c1)):
        g.weights[n.weight_slots[1]] = rng.uniform(-0.5, 0.5, c).astype(np.float32)
    w0, b0 = (g.weights[s] for s in n3.weight_slots)
    w1, b1 = (g.weights[s] for s in n1.weight_slots)
    a = _act(_conv64(h, w0, b0), act)
    B1 = gamma(27 * cin + 2) * _conv64(np.abs(h), np.abs(w0), np.abs(b0))
    ref = _conv64(a, w1, b1)
    bound = _conv64(B1, np.abs(w1)) + gamma(c3 + 2) * _conv64(np.abs(a) + B1, np.abs(w1), np.abs(b1))
    if flavour == 'sigmoid':
        ref, bound = 1.0 / (1.0 + np.exp(-ref)), bound / 4.0
    else:
        ref = _act(ref, act)
    if flavour == 'second_reader':
        # one float32 addition of the two results: their bounds, and one rounding of the sum
        bound = (bound + B1) * (1 + U) + U * np.abs(ref + a)
        ref = ref + a
    if pool:
        ref, bound = np_pool(ref, pool), np_pool(bound, pool)
    return dict(graph=g, x=x, ref=ref, bound=bound + TINY, launches=predict_launches(g),
                launches_unfused=predict_launches(g, unfused=True))


# ---- 4. views, add and pool: exact integer arithmetic -----------------------------------------
GRANULE = 2.0 ** -3                # every value of these cases is a multiple of it (lifts: _W5 / _W7)
EXACT_CASES = ('crop1', 'crop2', 'up2',
               'cat_skip_up_16_5', 'cat_skip_up_32_24', 'cat_skip_up_16_16',
               'cat_up_skip_16_24', 'cat_up_skip_32_5', 'cat_up_skip_16_16',
               'add', 'add_relu', 'pool6_negative', 'pool7_negative')


def _dyadic(c):
    """c distinct-ish small dyadic lift weights: _W7 repeated, block j times (1 + j)"""
    return (np.resize(_W7, c) * (1 + np.arange(c) // 7)).astype(np.float32)


def _set_lift(g, node, w):
    g.weights[node.weight_slots[0]] = w.reshape(1, 1, 1, 1, -1).copy()
    return node


def _int_conv3(g, node, cout, seed, lim=1):
    n = g.conv(node, cout, 3)
    w = np.random.default_rng(seed).integers(-lim, lim + 1, g.weights[n.weight_slots[0]].shape).astype(np.float32)
    g.weights[n.weight_slots[0]] = w
    return n, w


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """graph, x, want (float32, np.array_equal is asked of the GPU), launches, and `stages`: the
    (input, weights) of every convolution whose sums must be exact - the host test proves it.
    Inputs are small integers, lift weights dyadic, 3x3x3 weights integers."""
    seed = 50 + EXACT_CASES.index(name)
    stages = []

    def conv3(g, node, hin, cout, lim=1):
        n, w = _int_conv3(g, node, cout, seed + len(stages), lim)
        stages.append((hin, w))
        return n, _conv64(hin, w).astype(np.float32)

    if name.startswith('pool'):
        tile = int(name[4])
        g = LayerGraph(tile, seed=seed)
        x = _ints(seed, (BATCH, tile, tile, tile, 1), -90, 0)              # -90 .. -1
        w = np.abs(_W5)
        g.finish(g.pool(_set_lift(g, g.conv(g.input(), 5, 1), w), 2))
        want = np_pool(np_lift(x, w), 2)
    elif name.startswith('crop'):
        c, tile = int(name[-1]), 11
        g = LayerGraph(tile, seed=seed)
        x = _ints(seed, (BATCH, tile, tile, tile, 1))
        lift = _set_lift(g, g.conv(g.input(), 5, 1), _W5)
        n, want = conv3(g, g.crop(lift, c), np_crop(np_lift(x, _W5), c), 6, 2)
        g.finish(n)
    elif name == 'up2':
        tile = 10
        g = LayerGraph(tile, seed=seed)
        x = _ints(seed, (BATCH, tile, tile, tile, 1))
        lift = _set_lift(g, g.conv(g.input(), 7, 1), _W7)
        n, want = conv3(g, g.up(g.pool(lift, 2), 2), np_up(np_pool(np_lift(x, _W7), 2), 2), 6, 2)
        g.finish(n)
    elif name.startswith('cat'):
        # the U-Net joint: crop(skip, 1) beside up(pool(a 3x3x3 conv)); `c0` channels come first
        _, first, _, c0, c1 = name.split('_')
        c0, c1, tile = int(c0), int(c1), 10
        g = LayerGraph(tile, seed=seed)
        x = _ints(seed, (BATCH, tile, tile, tile, 1), -8, 9)
        cs, cl = (c0, c1) if first == 'skip' else (c1, c0)
        ws = _dyadic(cs)
        skip = g.crop(_set_lift(g, g.conv(g.input(), cs, 1), ws), 1)
        low, hl = conv3(g, g.input(), x, cl, 2)
        low = g.up(g.pool(low, 2), 2)
        hs, hl = np_crop(np_lift(x, ws), 1), np_up(np_pool(hl, 2), 2)
        if first == 'skip':
            n, want = conv3(g, g.concat(skip, low), np.concatenate([hs, hl], axis=-1), 6)
        else:
            n, want = conv3(g, g.concat(low, skip), np.concatenate([hl, hs], axis=-1), 6)
        g.finish(n)
    else:
        # resnet_like's shortcut: add(crop(a, 1), conv3(a)) - operands with different buffer edges
        tile = 9
        g = LayerGraph(tile, seed=seed)
        x = _ints(seed, (BATCH, tile, tile, tile, 1))
        w = _dyadic(6)
        a = _set_lift(g, g.conv(g.input(), 6, 1), w)
        ha = np_lift(x, w)
        b, hb = conv3(g, a, ha, 6, 2)
        y = g.add(g.crop(a, 1), b)
        want = np_crop(ha, 1) + hb
        if name == 'add_relu':
            y = g.relu(y)
            want = np.maximum(want, np.float32(0))
        g.finish(y)
    assert want.dtype == np.float32
    return dict(graph=g, x=x, want=np.ascontiguousarray(want), stages=stages, launches=predict_launches(g))


# ---- 5. programs the executor used to accept and could not run --------------------------------
# (kind, cin, cout, tile, lifts): declined now - the dispatcher takes the per-op executor ...
DECLINED_CASES = [('conv1', 16, 70, 5, None), ('conv1', 16, 100, 5, None),
                  ('stem', 1, 65, 11, None), ('stem', 1, 80, 11, None),
                  ('conv3', 21, 8, 7, (5, 16)), ('conv3', 40, 8, 7, (24, 16))]
# ... and their neighbours, which stay
NEIGHBOUR_CASES = [('conv1', 16, 64, 5, None), ('conv1', 16, 96, 5, None), ('conv1', 16, 128, 5, None),
                   ('stem', 1, 64, 11, None), ('conv3', 21, 8, 7, (16, 5))]
