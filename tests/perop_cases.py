"""Cases and numpy / float64 references of the kernel-level tests of the per-op fp32 executor
(csrc/generic.hip, csrc/conv_direct.h), the lattice kernels of csrc/infer.hip and hist_u8 / crop_u8
of csrc/synth.hip: test_perop_cases_host.py (what each case exercises, on the CPU),
test_gpu_perop.py, test_gpu_lattice_exact.py, test_gpu_hist_crop.py.  Nothing here touches a GPU.

Every named case carries a predicate - `*_facts(...)` below - that the host test evaluates, so a
case whose name promises "a chunk that spans rows" or "a pooled window on the padding edge" is
shown to hold one."""
import functools

import numpy as np
import torch

from flypylib_amd import fplmodels, synth
from flypylib_amd.program import BN_EPS, LayerGraph
from oracle import cnn_oracle, infer_oracle

U = 2.0 ** -24                    # unit roundoff of float32
TINY = 2.0 ** -126                # smallest normal float32: the bound's absolute floor
BATCH = 2


def gamma(K):
    """K roundings in a row: |computed - exact| <= gamma(K) * sum |terms| (Higham, Lemma 3.1)"""
    return K * U / (1.0 - K * U)


# ---- 1. convolutions of the per-op executor ---------------------------------------------------
CONV_EXTENTS = {1: (6, 10, 11), 3: (7, 9, 12)}           # three different extents, per kernel size
CONV_PAIRS = [(1, 48), (5, 7), (48, 48), (32, 64), (96, 1), (3, 130)]
CONV_VARIANTS = ('none', 'bias', 'relu', 'bn_relu')
CONV_CASES = [(k, cin, cout, v) for k in (1, 3) for cin, cout in CONV_PAIRS for v in CONV_VARIANTS]
SIGMOID_CASE = (1, 96, 1, 'sigmoid')


def _conv64(h, kernel, bias=None):
    """the oracle's convolution (cnn_oracle.conv3d_valid) in float64 on channels-last arrays"""
    t = torch.as_tensor(np.ascontiguousarray(h), dtype=torch.float64).permute(0, 4, 1, 2, 3)
    b = None if bias is None else torch.as_tensor(np.asarray(bias), dtype=torch.float64)
    y = cnn_oracle.conv3d_valid(t, torch.as_tensor(np.asarray(kernel), dtype=torch.float64), b)
    return y.permute(0, 2, 3, 4, 1).contiguous().numpy()


@functools.lru_cache(maxsize=None)
def conv_case(k, cin, cout, variant):
    """One convolution (lifted to `cin` channels by a 1x1x1 convolution, as test_single_conv_layer
    does) on (BATCH,) + CONV_EXTENTS[k].  Returns a dict:

      graph, x     what the GPU runs
      h            the float32 input of the convolution under test: x itself, or the oracle's
                   float32 output of the lift (one correctly rounded product per element)
      ref          float64 oracle of the convolution (+ bias / BN / activation) on `h`
      bound        per output element, derived, not tuned:
                   gamma(K) * (|h| (*) |w| + |bias|) + 2^-126, K = k^3 * cin + 1 - the k^3 * cin
                   fused multiply-adds of the accumulation and the one of the epilogue
                   (conv_direct.h).  With BatchNorm: times |gamma * invstd|, plus 3u of the
                   affine's magnitude |s| |conv| + |shift| (the folded scale and shift are each
                   rounded once to float32, the epilogue once more).  ReLU is 1-Lipschitz; for the
                   sigmoid (Lipschitz constant 1/4) `bound` is this conv bound divided by 4.
    """
    seed = 1000 * k + 10 * cin + cout
    ext = CONV_EXTENTS[k]
    rng = np.random.default_rng(seed)
    g = LayerGraph(ext, seed=seed)
    node = g.input()
    if cin != 1:
        node = g.conv(node, cin, 1)
    lift = node
    biased = variant in ('bias', 'sigmoid')
    conv = g.conv(node, cout, k, use_bias=biased, activation='sigmoid' if variant == 'sigmoid' else None)
    y = conv
    if variant == 'relu':
        y = g.relu(y)
    elif variant == 'bn_relu':
        y = g.bn_relu(y)
    g.finish(y)
    g.randomize_bn(seed)
    if biased:
        g.weights[conv.weight_slots[1]] = rng.uniform(-0.5, 0.5, cout).astype(np.float32)
    x = rng.standard_normal((BATCH,) + ext + (1,)).astype(np.float32)

    if cin == 1:
        h = x
    else:                              # the oracle's float32 output of the lift alone
        gl = LayerGraph(ext)
        gl.finish(gl.conv(gl.input(), cin, 1))
        gl.set_weights([g.weights[lift.weight_slots[0]]])
        h = cnn_oracle.graph_forward(gl, x, dtype=torch.float32)
    assert h.dtype == np.float32
    w = g.weights[conv.weight_slots[0]]
    bias = g.weights[conv.weight_slots[1]] if biased else None
    c = _conv64(h, w, bias)
    mag = _conv64(np.abs(h), np.abs(w), None if bias is None else np.abs(bias))
    K = k ** 3 * cin + 1
    bound = gamma(K) * mag
    ref = c
    if variant == 'relu':
        ref = np.maximum(c, 0.0)
    elif variant == 'bn_relu':
        bn = g.nodes[conv.idx + 1]
        gm, bt, mu, var = (g.weights[s].astype(np.float64) for s in bn.weight_slots)
        s = gm / np.sqrt(var + BN_EPS)
        t = bt - mu * s
        ref = np.maximum(c * s + t, 0.0)
        bound = np.abs(s) * bound + 3 * U * (np.abs(s) * np.abs(c) + np.abs(t))
    elif variant == 'sigmoid':
        ref = 1.0 / (1.0 + np.exp(-c))
        bound = bound / 4.0
    return dict(graph=g, x=x, h=h, ref=ref, bound=bound + TINY, K=K, mag=mag, lift=lift, conv=conv)


# ---- 1b. the exact ops ------------------------------------------------------------------------
# lifts whose products are exact in float32: integer inputs times small dyadic weights
_W5 = np.array([1.0, -2.0, 0.5, 3.0, -0.25], np.float32)
_W7 = np.array([-1.0, 4.0, 0.75, -3.0, 2.0, 0.125, -6.0], np.float32)


def _ints(seed, shape, lo=-40, hi=41):
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(np.float32)


def _lift(g, x, w):
    n = g.conv(x, w.size, 1)
    g.weights[n.weight_slots[0]] = w.reshape(1, 1, 1, 1, -1).copy()
    return n


def np_lift(x, w):
    return (x * w.reshape(1, 1, 1, 1, -1)).astype(np.float32)


def np_pool(a, f):
    """MaxPooling3D(f): stride f, floor"""
    n, D, H, W, C = a.shape
    d, h, w = D // f, H // f, W // f
    return a[:, :d * f, :h * f, :w * f].reshape(n, d, f, h, f, w, f, C).max(axis=(2, 4, 6))


def np_crop(a, c):
    return a[:, c:a.shape[1] - c, c:a.shape[2] - c, c:a.shape[3] - c]


def np_up(a, f):
    f = (f,) * 3 if np.isscalar(f) else f
    for ax, r in zip((1, 2, 3), f):
        a = np.repeat(a, r, axis=ax)
    return a


EXACT_CASES = ('pool2_even', 'pool2_odd', 'pool2_negative', 'pool3', 'crop1', 'crop2', 'up2', 'up_123',
               'concat_skip_up', 'concat_up_skip', 'add', 'add_relu')


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """(graph, x, want): ops that move or compare values, so the GPU result is np.array_equal to
    numpy's.  Inputs are small integers and the lifts' weights dyadic, so the lift itself is exact;
    'add' instead takes random floats through two random lifts: one rounded product each, then the
    one float32 addition under test."""
    seed = EXACT_CASES.index(name)
    ext = {'pool2_even': (6, 10, 12), 'pool2_odd': (7, 9, 12), 'pool2_negative': (7, 9, 12), 'pool3': (7, 10, 11),
           'crop1': (7, 9, 12), 'crop2': (7, 9, 12), 'up2': (3, 4, 5), 'up_123': (3, 4, 5),
           'concat_skip_up': (8, 10, 14), 'concat_up_skip': (8, 10, 14), 'add': (6, 10, 11),
           'add_relu': (6, 10, 11)}[name]
    g = LayerGraph(ext, seed=seed)
    if name == 'pool2_negative':
        x = _ints(seed, (BATCH,) + ext + (1,), -90, 0)          # -90 .. -1: no zero, no positive
    elif name.startswith('add'):
        x = np.random.default_rng(seed).standard_normal((BATCH,) + ext + (1,)).astype(np.float32)
    else:
        x = _ints(seed, (BATCH,) + ext + (1,))
    if name.startswith('pool'):
        f = 3 if name == 'pool3' else 2
        w = np.abs(_W5) if name == 'pool2_negative' else _W5
        g.finish(g.pool(_lift(g, g.input(), w), f))
        want = np_pool(np_lift(x, w), f)
    elif name.startswith('crop'):
        c = int(name[-1])
        g.finish(g.crop(_lift(g, g.input(), _W5), c))
        want = np_crop(np_lift(x, _W5), c)
    elif name.startswith('up'):
        f = 2 if name == 'up2' else (1, 2, 3)
        g.finish(g.up(_lift(g, g.input(), _W5), f))
        want = np_up(np_lift(x, _W5), f)
    elif name.startswith('concat'):
        skip = g.crop(_lift(g, g.input(), _W5), 1)                               # 5 channels
        low = g.up(g.pool(g.crop(_lift(g, g.input(), _W7), 1), 2), 2)            # 7 channels
        a, b = np_crop(np_lift(x, _W5), 1), np_up(np_pool(np_crop(np_lift(x, _W7), 1), 2), 2)
        if name == 'concat_skip_up':
            g.finish(g.concat(skip, low))
            want = np.concatenate([a, b], axis=-1)
        else:
            g.finish(g.concat(low, skip))
            want = np.concatenate([b, a], axis=-1)
    else:
        na, nb = g.conv(g.input(), 6, 1), g.conv(g.input(), 6, 1)
        y = g.add(na, nb)
        if name == 'add_relu':
            y = g.relu(y)
        g.finish(y)
        a = np_lift(x, g.weights[na.weight_slots[0]].reshape(-1))
        b = np_lift(x, g.weights[nb.weight_slots[0]].reshape(-1))
        want = a + b
        assert want.dtype == np.float32
        if name == 'add_relu':
            want = np.maximum(want, np.float32(0))
    return g, x, np.ascontiguousarray(want)


def lift_is_exact(x, w):
    """every product of the lift is a float32 number: nothing is rounded before the op under test"""
    p = x.astype(np.float64) * w.astype(np.float64).reshape(1, 1, 1, 1, -1)
    return bool(np.array_equal(p.astype(np.float32).astype(np.float64), p))


# ---- 1c. the factories ------------------------------------------------------------------------
# (tile per factory: tests/test_gpu_cnn.py - test_other_architectures_forward and the two tile tests)
FACTORIES = [('baseline_model', 22), ('vgg_like', 30), ('vgg_like2', 28), ('resnet_like', 22),
             ('unet_like', 22), ('unet_like2', 28), ('unet_like3', 36), ('unet_like4', 44),
             ('unet_like4b', 44), ('unet_like_vol', 62)]


@functools.lru_cache(maxsize=None)
def factory_case(name):
    """(graph, x (1, s, s, s, 1), float64 oracle)"""
    size = dict(FACTORIES)[name]
    g = getattr(fplmodels, name)(size)[0]
    synth.synthetic_weights(g, 7)
    x = np.random.default_rng(2).standard_normal((1, size, size, size, 1)).astype(np.float32)
    return g, x, cnn_oracle.graph_forward(g, x, dtype=torch.float64)


# ---- 1d. whole-volume inference on a tile with three different edges --------------------------
NONCUBIC = dict(tile=(30, 26, 22), off=(7, 7, 7), stride=(4, 4, 4), vol=(50, 41, 33), mean=128.0, std=33.0)


@functools.lru_cache(maxsize=None)
def noncubic_case():
    """(graph, u8 volume, float64-oracle lattice) of vgg_like on NONCUBIC"""
    c = NONCUBIC
    g = fplmodels.vgg_like(c['tile'])[0]
    synth.synthetic_weights(g, 8)
    u8 = synth.em_volume_u8(3, c['vol'])
    img = normalise(u8, c['mean'], c['std'])

    def predict(batch):
        return cnn_oracle.vgg_like_forward(batch.astype(np.float32), g.weights, upsample_stride=4,
                                           dtype=torch.float64)
    return g, u8, infer_oracle.infer_lattice(img, c['tile'], c['off'], predict)


# ---- 2. lattice programs whose arithmetic is exact --------------------------------------------
def normalise(u8, mean, std):
    """gather_tiles<uint8_t>: float(u8) - float(mean), then / float(std), each rounded on its own"""
    return (u8.astype(np.float32) - np.float32(mean)) / np.float32(std)


# tile / offset / stride of each program, a second tile with three different edges (the per-op
# route), and a volume (<= 40^3) with three tile rows in z and a ragged last tile on every axis
LATTICE = {
    'P1_off0': dict(off=0, stride=1, tile=6, alt=(6, 5, 10), vol=(13, 8, 15)),
    'P1_off3': dict(off=3, stride=1, tile=10, alt=(10, 12, 14), vol=(17, 15, 12)),
    'P2': dict(off=2, stride=2, tile=12, alt=(12, 16, 20), vol=(21, 23, 18)),
    'P3': dict(off=0, stride=4, tile=16, alt=(16, 8, 12), vol=(33, 21, 25)),
}
SOURCES = ('u8_128_33', 'u8_127.3_0.1', 'f32')


def lattice_graph(name):
    """P1: crop(off) -> conv1x1x1(weight 1);  P2: pool(2) -> crop(1) -> conv1;  P3: pool(2) ->
    pool(2) -> conv1.  fmaf(x, 1, 0) twice (conv_direct.h) returns x: the program moves and
    compares values only."""
    g = LayerGraph(None)
    x = g.input()
    if name.startswith('P1'):
        y = g.crop(x, LATTICE[name]['off'])
    elif name == 'P2':
        y = g.crop(g.pool(x, 2), 1)
    else:
        y = g.pool(g.pool(x, 2), 2)
    g.finish(g.conv(y, 1, 1))
    g.set_weights([np.ones((1, 1, 1, 1, 1), np.float32)])
    return g


def lattice_predict(name):
    """numpy restatement of the program plus the output upsampling, for infer_oracle.infer_lattice"""
    off = LATTICE[name]['off']

    def predict(batch):
        if name.startswith('P1'):
            return np_crop(batch, off)
        if name == 'P2':
            return np_up(np_crop(np_pool(batch, 2), 1), 2)
        return np_up(np_pool(np_pool(batch, 2), 2), 4)
    return predict


def lattice_source(name, source, vol=None):
    """(what infer_volume is given, mean, std, the normalised float32 image)"""
    vol = vol or LATTICE[name]['vol']
    rng = np.random.default_rng(sorted(LATTICE).index(name) * 10 + SOURCES.index(source))
    if source == 'f32':
        img = rng.standard_normal(vol).astype(np.float32)
        return img, 0.0, 1.0, img
    mean, std = (128.0, 33.0) if source == 'u8_128_33' else (127.3, 0.1)
    u8 = rng.integers(0, 256, vol, dtype=np.uint8)
    return u8, mean, std, normalise(u8, mean, std)


@functools.lru_cache(maxsize=None)
def lattice_reference(name, source, tile=None, vol=None):
    c = LATTICE[name]
    tile = tile or (c['tile'],) * 3
    _, _, _, img = lattice_source(name, source, vol)
    return infer_oracle.infer_lattice(img, tile, (c['off'],) * 3, lattice_predict(name))


def thin_volumes(name):
    """{label: volume}: one axis <= 2 * off (no tile at all: all zero) where off > 0, and one axis
    = 2 * off + 1 (a single, mostly padded tile row), each on a different axis"""
    off = LATTICE[name]['off']
    base = [11, 13, 14]
    out = {}
    for axis in range(3):
        if off > 0:
            v = list(base)
            v[axis] = 2 * off - (axis == 1)                   # = 2 * off, and once below it
            out['none_axis%d' % axis] = tuple(v)
        v = list(base)
        v[axis] = 2 * off + 1
        out['one_axis%d' % axis] = tuple(v)
    return out


def lattice_facts(name, tile=None, vol=None):
    c = LATTICE[name]
    tile = tile or (c['tile'],) * 3
    vol = vol or c['vol']
    _, start, end = infer_oracle.tile_lattice(vol, tile, (c['off'],) * 3)
    ext = end - start
    return dict(n_tiles=ext.shape[1],
                ragged_on_all_axes=bool(ext.shape[1] and np.any(np.all(ext < np.asarray(tile)[:, None], axis=0))),
                z_rows=len(range(c['off'], vol[0] - c['off'], tile[0] - 2 * c['off'])))


def p3_ignoring_the_padding(img):
    """P3 over the volume when the zero padding could never win a window: pad with -inf instead"""
    pad = [(0, -s % 4) for s in img.shape]
    a = np.pad(img, pad, constant_values=-np.inf)[None, ..., None]
    r = np_up(np_pool(np_pool(a, 2), 2), 4)[0, ..., 0]
    return r[:img.shape[0], :img.shape[1], :img.shape[2]]


# ---- 3. hist_u8 -------------------------------------------------------------------------------
HIST_BLOCK = 256                   # threads of a block; 16 bytes per thread and pass (synth.hip)


def hist_grid_cap(n_cu):
    return n_cu * 8                # fpl_histogram_u8: min(ceil(n / 16 / 256), n_cu * 8) blocks


def hist_sizes(n_cu):
    """{label: n}.  'one_pass_5' (16 * 256 * G + 5) fills the capped grid exactly once and leaves
    five bytes to block 0; 'strided_5' adds 300 vectors, so the grid stride is taken by some
    threads and not by others."""
    G = hist_grid_cap(n_cu)
    return {'0': 0, '1': 1, '15': 15, '16': 16, '17': 17, 'one_block_less_1': 16 * 256 - 1,
            'one_pass_5': 16 * 256 * G + 5, 'strided_5': 16 * 256 * G + 16 * 300 + 5}


def hist_facts(n, n_cu):
    G = hist_grid_cap(n_cu)
    n16 = n // 16
    blocks = max(1, min(-(-n16 // HIST_BLOCK), G))
    return dict(vectors=n16, remainder=n % 16, blocks=blocks,
                passes=-(-n16 // (blocks * HIST_BLOCK)), capped=-(-n16 // HIST_BLOCK) > G)


def hist_data(kind, n, seed=0):
    rng = np.random.default_rng(seed + n % 9973)
    if kind == 'random':
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == 'constant':
        return np.full(n, 255, np.uint8)
    assert kind == 'even_only'                                # half the bins stay empty
    return rng.integers(0, 256, n, dtype=np.uint8) & np.uint8(0xFE)


# ---- 3b. crop_u8 ------------------------------------------------------------------------------
SYN_PER_WG = 256 * 4               # voxels of the box per work-group chunk (synth.hip)
CROP_EXTENT = (23, 19, 37)
# name: (dims, origin).  Three different dims each; row lengths D2 in {1, 2, 3, 5, 13, 36, 64}
CROP_BOXES = {
    'd2_1_inside': ((7, 5, 1), (3, 4, 9)),
    'd2_2_leaves_z_low': ((5, 9, 2), (-2, 3, 11)),
    'd2_3_leaves_z_high': ((6, 4, 3), (20, 2, 5)),
    'd2_5_leaves_y_low': ((3, 11, 5), (1, -4, 7)),
    'd2_13_leaves_y_high_two_chunks': ((9, 10, 13), (2, 12, 3)),
    'd2_36_leaves_x_low': ((2, 3, 36), (5, 6, -7)),
    'd2_64_leaves_x_high': ((3, 2, 64), (10, 9, 5)),
    'd2_36_inside_two_chunks': ((6, 8, 36), (3, 2, 1)),
    'outside_high': ((2, 3, 5), (30, 0, 0)),
    'outside_low': ((3, 2, 5), (0, 0, -9)),
    'all_faces': ((25, 21, 39), (-1, -1, -1)),
}


def crop_source():
    return np.random.default_rng(77).integers(1, 256, CROP_EXTENT, dtype=np.uint8)      # no zero: padding shows


def crop_reference(src, dims, origin):
    out = np.zeros(dims, np.uint8)
    lo = [max(0, -o) for o in origin]
    hi = [min(d, e - o) for d, e, o in zip(dims, src.shape, origin)]
    if all(h > l for l, h in zip(lo, hi)):
        out[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = src[origin[0] + lo[0]:origin[0] + hi[0],
                                                         origin[1] + lo[1]:origin[1] + hi[1],
                                                         origin[2] + lo[2]:origin[2] + hi[2]]
    return out


def crop_facts(dims, origin, extent=CROP_EXTENT):
    """what crop_u8's threads meet in this box: every thread owns the four voxels from a flat index
    i = 0 (mod 4) on; the fast path (one 4-byte load) needs them in one row of the box and of the
    source"""
    D0, D1, D2 = dims
    E0, E1, E2 = extent
    n = D0 * D1 * D2
    f = dict(n=n, chunks=-(-n // SYN_PER_WG), fast=0, fast_odd_address=0, slow=0, max_rows=0, crosses_plane=0,
             tail=n % 4, leaves=set(), inside_voxels=0, chunk_base_mid_row=bool(n > SYN_PER_WG and SYN_PER_WG % D2))
    for a, (o, d, e) in enumerate(zip(origin, dims, extent)):
        if o < 0 and o + d > 0:
            f['leaves'].add('%s_low' % 'zyx'[a])
        if o + d > e and o < e:
            f['leaves'].add('%s_high' % 'zyx'[a])
    for i in range(0, n, 4):
        idx = np.arange(i, min(i + 4, n))
        z, y, x = idx // (D1 * D2), idx // D2 % D1, idx % D2
        gz, gy, gx = z[0] + origin[0], y[0] + origin[1], x[0] + origin[2]
        fast = (x[0] + 4 <= D2 and gz >= 0 and gy >= 0 and gx >= 0 and gz < E0 and gy < E1 and gx + 4 <= E2
                and i + 4 <= n)
        if fast:
            f['fast'] += 1
            f['fast_odd_address'] += int(((gz * E1 + gy) * E2 + gx) % 2)
        else:
            f['slow'] += 1
            f['max_rows'] = max(f['max_rows'], len(set(zip(z.tolist(), y.tolist()))))
            f['crosses_plane'] += int(z[0] != z[-1])
    inside = [max(0, min(d, e - o) - max(0, -o)) for d, e, o in zip(dims, extent, origin)]
    f['inside_voxels'] = int(np.prod(inside))
    return f
