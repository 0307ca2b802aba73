"""GPU: fplv_loss_sums (libfplval.so) against its float64 specification valid.loss_sums_numpy on
the smallest inputs at which the kernel can go wrong: the scalar head and tail alone, one block's
elements minus one / exact / plus one, a grid stride and a bit, unaligned pred and labels (label
words and label bytes), the edge values of the clip and of rintf, absent classes.

Bounds: the five counts are exact.  The three real sums lie within 1e-12 * max(n, |ref|): a
double evaluation of the per-element formulas is a few ulp of at most 16.2 off (below 1e-13 per
element), a fixed-order double sum of n terms adds at most n * 2^-52 * |S|."""
import numpy as np
import pytest
import torch

from flypylib_amd import _capi, _validcapi, valid

pytestmark = pytest.mark.gpu

KINDS = sorted(_capi.LOSS_KINDS, key=_capi.LOSS_KINDS.get)
PER_BLOCK = _validcapi.BLOCK * _validcapi.ELEMS_PER_THREAD
GRID_STRIDE = PER_BLOCK * _validcapi.MAX_BLOCKS
EDGES = np.array([0.0, 1e-8, 1e-7, 0.5, 1 - 1e-7, 1.0], np.float32)
COUNTS, REALS = (1, 2, 4, 6, 7), (0, 3, 5)
# name -> (n, offset of pred, offset of labels in elements from an aligned base, labels)
CASES = {
    'n1': (1, 0, 0, 'mixed'), 'n3': (3, 0, 0, 'mixed'), 'n4': (4, 0, 0, 'mixed'), 'n5': (5, 0, 0, 'mixed'),
    'block-1': (PER_BLOCK - 1, 0, 0, 'mixed'), 'block': (PER_BLOCK, 0, 0, 'mixed'),
    'block+1': (PER_BLOCK + 1, 0, 0, 'mixed'),
    'stride+5': (GRID_STRIDE + 5, 0, 0, 'mixed'),
    # head of 3 floats; the label word behind it is aligned again
    'both-off-1': (2 * PER_BLOCK + 6, 1, 1, 'mixed'),
    # no head, labels read byte by byte / head of 2 floats, labels byte by byte
    'labels-off-1': (2 * PER_BLOCK + 6, 0, 1, 'mixed'), 'pred-off-2': (2 * PER_BLOCK + 3, 2, 0, 'mixed'),
    'all-2': (PER_BLOCK + 1, 0, 0, 'all2'), 'no-1': (PER_BLOCK + 1, 0, 0, 'no1'),
}
_HOST, _REF = {}, {}


def _host(name):
    """float32 predictions (random, the edge values mixed in) and labels of a case; made once"""
    if name not in _HOST:
        n, _, _, how = CASES[name]
        rng = np.random.default_rng(sorted(CASES).index(name))
        p = rng.random(n).astype(np.float32)
        at = rng.permutation(n)[:max(n // 3, min(n, len(EDGES)))]
        p[at] = EDGES[np.arange(len(at)) % len(EDGES)]
        y = rng.integers(0, 3, n).astype(np.uint8)
        if how == 'all2':
            y[:] = 2
        elif how == 'no1':
            y[y == 1] = 0
        _HOST[name] = (p, y)
    return _HOST[name]


def _ref(name, kind):
    if (name, kind) not in _REF:
        _REF[name, kind] = valid.loss_sums_numpy(*_host(name), kind)
    return _REF[name, kind]


def _device(name):
    """the case on the GPU at its offsets from a 256-byte aligned base"""
    p, y = _host(name)
    _, op, oy, _ = CASES[name]
    pd = torch.zeros(len(p) + op, dtype=torch.float32, device='cuda:0')
    yd = torch.zeros(len(y) + oy, dtype=torch.uint8, device='cuda:0')
    pd[op:] = torch.from_numpy(p)
    yd[oy:] = torch.from_numpy(y)
    pd, yd = pd[op:], yd[oy:]
    assert pd.data_ptr() % 16 == 4 * op % 16 and yd.data_ptr() % 4 == oy % 4
    return pd, yd


def _close(got, ref, n, what):
    print(what, 'got', got.tolist(), 'ref', ref.tolist())
    for k in COUNTS:
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    for k in REALS:
        assert abs(got[k] - ref[k]) <= 1e-12 * max(n, abs(ref[k])), (what, k, got[k], ref[k])


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', list(CASES))
def test_sums_match_the_numpy_specification(ctx, name, kind):
    pd, yd = _device(name)
    got = valid.loss_sums_device(pd, yd, kind).cpu().numpy()
    _close(got, _ref(name, kind), CASES[name][0], (name, kind))
    if name == 'all-2':
        assert got[3] == got[4] == got[5] == got[6] == 0
        assert _capi.metrics_from_sums(list(got))['lb1l1err'] == 0
    if name == 'no-1':
        assert got[5] == got[6] == 0 and got[4] > 0


@pytest.mark.parametrize('name', ['n5', 'stride+5', 'labels-off-1'])
def test_the_same_call_twice_gives_the_same_bytes(ctx, name):
    pd, yd = _device(name)
    for kind in KINDS:
        a = valid.loss_sums_device(pd, yd, kind).cpu().numpy().tobytes()
        b = valid.loss_sums_device(pd, yd, kind).cpu().numpy().tobytes()
        assert a == b, (name, kind)


@pytest.mark.parametrize('kind', KINDS)
def test_three_accumulated_calls_are_one_pass_over_the_concatenation(ctx, kind):
    names = ['block+1', 'n3', 'both-off-1']
    sums = torch.full((8,), 123.0, dtype=torch.float64, device='cuda:0')     # replaced by the first call
    for i, name in enumerate(names):
        out = valid.loss_sums_device(*_device(name), kind, sums=sums, accumulate=i > 0)
        assert out is sums
    p = np.concatenate([_host(n)[0] for n in names])
    y = np.concatenate([_host(n)[1] for n in names])
    _close(sums.cpu().numpy(), valid.loss_sums_numpy(p, y, kind), len(p), ('accumulated', kind))


@pytest.mark.parametrize('name', ['n1', 'block+1', 'stride+5'])
def test_nothing_is_written_around_sums_and_scratch(ctx, name):
    """sentinels before and behind the 8 doubles and the FPLV_SCRATCH_BYTES stay as they were"""
    guard = 64
    pd, yd = _device(name)
    sums = torch.full((8 + 2 * guard,), -7.25, dtype=torch.float64, device='cuda:0')
    scratch = torch.full((_validcapi.SCRATCH_BYTES + 2 * 8 * guard,), 0xA5, dtype=torch.uint8, device='cuda:0')
    got = valid.loss_sums_device(pd, yd, 'masked_focal_loss', sums=sums[guard:guard + 8],
                                 scratch=scratch[8 * guard:8 * guard + _validcapi.SCRATCH_BYTES])
    _close(got.cpu().numpy(), _ref(name, 'masked_focal_loss'), CASES[name][0], name)
    s, c = sums.cpu().numpy(), scratch.cpu().numpy()
    assert (s[:guard] == -7.25).all() and (s[guard + 8:] == -7.25).all()
    assert (c[:8 * guard] == 0xA5).all() and (c[8 * guard + _validcapi.SCRATCH_BYTES:] == 0xA5).all()
    # ... and within the scratch only the rows of the blocks that ran are written
    blocks = min(max(-(-(CASES[name][0] // 4) // _validcapi.BLOCK), 1), _validcapi.MAX_BLOCKS)
    assert (c[8 * guard + blocks * 56:8 * guard + _validcapi.SCRATCH_BYTES] == 0xA5).all()


def test_device_arguments_are_refused_by_name(ctx):
    pd, yd = _device('n5')
    with pytest.raises(ValueError, match='pred must be contiguous'):
        valid.loss_sums_device(torch.zeros(10, dtype=torch.float32, device='cuda:0')[::2], yd, 0)
    with pytest.raises(ValueError, match='5 predictions, 4 labels'):
        valid.loss_sums_device(pd, yd[:4], 0)
    with pytest.raises(ValueError, match='sums must be a contiguous float64 tensor of 8'):
        valid.loss_sums_device(pd, yd, 0, sums=torch.zeros(8, device='cuda:0'))
    with pytest.raises(ValueError, match='labels must be on a GPU'):
        valid.loss_sums_device(pd, yd.cpu(), 0)
    # host memory handed to the C entry point itself is refused, not read
    host = np.zeros(8)
    with pytest.raises(_validcapi.FplValidError, match='fplv_loss_sums: sums must be device memory'):
        _validcapi.loss_sums(pd, yd, 5, 0, 0, host, torch.empty(_validcapi.SCRATCH_BYTES, dtype=torch.uint8,
                                                                device='cuda:0'), _validcapi.SCRATCH_BYTES)
