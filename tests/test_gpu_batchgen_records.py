"""libfplbatch.so's gather kernel through the C ABI on hand-made record tables
(tests/batchgen_cases.py): every (rot, flips) the header allows at every tile geometry, centres
against the faces of their volumes, records that must write nothing, the noise arithmetic at
its edges and the launch's extremes.  The reference is batchgen.execute_numpy; every
comparison is by bytes, so there is no tolerance.

Every output lies between two guards of GUARD elements.  Guards and output are filled with a
sentinel before the call - one NaN bit pattern for data (no reference holds a NaN:
test_batchgen_plan.py), a byte outside {0, 1, 2} for labels - and the whole buffers are compared
afterwards, so a write past an example's own region or past the output shows."""
import numpy as np
import pytest
import torch

from flypylib_amd import _batchcapi, batchgen
from tests import batchgen_cases as cases

pytestmark = pytest.mark.gpu

GUARD = 4096
DATA_SENTINEL = 0x7FA55AA5          # a NaN, as uint32
LABEL_SENTINEL = 0xA5
N_VOLS = len(cases.RECORD_SHAPES)


class _Resident:
    """the three volumes in both image dtypes and, per source dtype, a volume table of four
    entries: the three, and volume 0 once more declared in the other dtype.  That entry
    points at the float32 image whichever dtype it declares, so that a kernel which read it
    all the same would stay inside an allocation."""

    def __init__(self, dev):
        self.dev = dev
        self.images = {dt: [torch.from_numpy(np.array(im)).to(dev)
                            for im, _ in cases.record_volumes(dt)]
                       for dt in (np.float32, np.uint8)}
        self.labels = [torch.from_numpy(np.array(ll)).to(dev)
                       for _, ll in cases.record_volumes(np.uint8)]
        self.tables = {}
        for dt, code, other in ((np.float32, _batchcapi.F32, _batchcapi.U8),
                                (np.uint8, _batchcapi.U8, _batchcapi.F32)):
            t = np.zeros(N_VOLS + 1, _batchcapi.VOLUME)
            for v, (im, ll) in enumerate(zip(self.images[dt], self.labels)):
                t[v] = (im.data_ptr(), ll.data_ptr()) + tuple(im.shape) + (code,)
            im = self.images[np.float32][0]
            t[N_VOLS] = (im.data_ptr(), self.labels[0].data_ptr()) + tuple(im.shape) + (other,)
            self.tables[dt] = (torch.from_numpy(t.view(np.uint8)).to(dev), code)


@pytest.fixture(scope='module')
def resident(ctx):
    return _Resident(torch.device('cuda', 0))


def _gather(resident, context, label6, noise, dtype, rec, n_vols=N_VOLS):
    """one call of fplb_gather into guarded, sentinel-filled buffers; the whole buffers come
    back as (uint32, uint8) numpy arrays"""
    n = len(rec) * context[0] * context[1] * context[2]
    nl = len(rec) * (216 if label6 else 1)
    data = torch.full((GUARD + n + GUARD,), DATA_SENTINEL, dtype=torch.int32, device=resident.dev)
    labels = torch.full((GUARD + nl + GUARD,), LABEL_SENTINEL, dtype=torch.uint8,
                        device=resident.dev)
    rec_dev = torch.from_numpy(np.array(rec).view(np.uint8)).to(resident.dev)
    table, code = resident.tables[dtype]
    _batchcapi.gather(table.data_ptr(), n_vols, rec_dev.data_ptr(), len(rec), context, code, noise,
                      _batchcapi.LABELS_6 if label6 else _batchcapi.LABELS_CENTRE,
                      data.data_ptr() + 4 * GUARD, labels.data_ptr() + GUARD, 0)
    torch.cuda.synchronize(resident.dev)
    return data.cpu().numpy().view(np.uint32), labels.cpu().numpy()


def _check(buf, want, sentinel, what):
    """`buf`: guard, output, guard; `want`: (examples, elements each) of buf's dtype"""
    for name, g in (('front', buf[:GUARD]), ('back', buf[-GUARD:])):
        hit = np.flatnonzero(g != sentinel)
        assert hit.size == 0, ('%s: %d elements of the %s guard overwritten, the first at %d'
                               % (what, hit.size, name, hit[0]))
    got = buf[GUARD:-GUARD].reshape(want.shape)
    if got.tobytes() != want.tobytes():
        diff = (np.ascontiguousarray(got).view(np.uint8).reshape(len(want), -1)
                != np.ascontiguousarray(want).view(np.uint8).reshape(len(want), -1)).sum(1)
        print('%s: differing bytes per example (of %d): %s'
              % (what, want[0].nbytes, diff.tolist()))
        raise AssertionError('%s: %d differing bytes in examples %s'
                             % (what, int(diff.sum()), np.flatnonzero(diff).tolist()))


def _check_both(got, want, what):
    _check(got[0], np.ascontiguousarray(want[0]).view(np.uint32), DATA_SENTINEL, what + ' data')
    _check(got[1], want[1], LABEL_SENTINEL, what + ' labels')


@pytest.mark.parametrize('case', cases.RECORD_CASES, ids=cases.case_id)
def test_every_record_form_equals_the_numpy_executor(resident, case):
    """one record per (rot, flips), each patch against three faces of its volume"""
    _, context, label6, noise, dtype, rec = cases.record_case(case)
    got = _gather(resident, context, label6, noise, dtype, rec)
    _check_both(got, cases.record_reference(case), cases.case_id(case))


def _validator(context, label6, dtype, rec):
    """a DeviceBatches whose _validate sees the volumes of the tables.  Where the constructor
    refuses the context (which is then asserted) the two attributes _validate reads are set
    as the constructor sets them."""
    plan = cases.RecordPlan(context, label6, False, dtype, rec)
    plan.images = [np.array(im) for im in plan.images]        # writable: torch takes them as they are
    refusal = ('s1 == s2' if context[1] != context[2]
               else '6\\^3 label block' if label6 and min(plan.half) < 3 else None)
    if refusal is None:
        return batchgen.DeviceBatches(plan, 0)
    with pytest.raises(ValueError, match=refusal):
        batchgen.DeviceBatches(plan, 0)
    db = object.__new__(batchgen.DeviceBatches)
    db._dims = np.array(cases.RECORD_SHAPES, np.int64)
    db._reach = np.maximum(np.array(plan.half), 3 if label6 else 0)
    return db


@pytest.mark.parametrize('dtype', [np.float32, np.uint8], ids=['float32', 'uint8'])
@pytest.mark.parametrize('context,label6', cases.SKIP_CASES,
                         ids=['6x34x34-labels6', '4x4x4-labels6', '4x34x70-centre'])
def test_invalid_records_write_nothing_and_validate_draws_the_same_line(resident, context, label6,
                                                                        dtype):
    """valid and invalid records alternate: the region of every invalid one is still sentinel
    in data and labels, every valid one equals the reference, and DeviceBatches._validate
    refuses exactly the records the kernel skipped"""
    rec, kinds = cases.skip_records(context, label6)
    valid = np.array([k == 'valid' for k in kinds])
    got = _gather(resident, context, label6, True, dtype, rec, n_vols=N_VOLS + 1)
    ref = cases.reference(context, label6, True, dtype, rec[valid])
    want_d = np.full((len(rec), ref[0].shape[1]), DATA_SENTINEL, np.uint32)
    want_l = np.full((len(rec), ref[1].shape[1]), LABEL_SENTINEL, np.uint8)
    want_d[valid] = ref[0].view(np.uint32)
    want_l[valid] = ref[1]
    what = '%r %s' % (context, np.dtype(dtype).name)
    _check(got[0], want_d, DATA_SENTINEL, what + ' data')
    _check(got[1], want_l, LABEL_SENTINEL, what + ' labels')
    # what the kernel skipped, read off its output alone
    d = got[0][GUARD:-GUARD].reshape(want_d.shape)
    lab = got[1][GUARD:-GUARD].reshape(want_l.shape)
    skipped = (d == DATA_SENTINEL).all(1) & (lab == LABEL_SENTINEL).all(1)
    db = _validator(context, label6, dtype, rec)
    for i, kind in enumerate(kinds):
        if kind in cases.SKIP_NOT_VALIDATED:
            continue
        try:
            db._validate(rec[i:i + 1])
            refused = False
        except ValueError:
            refused = True
        assert refused == bool(skipped[i]), (i, kind, refused)


@pytest.mark.parametrize('dtype', [np.float32, np.uint8], ids=['float32', 'uint8'])
def test_noise_arithmetic_at_its_edges(resident, dtype):
    """signed zeros, float32 denormals, overflow to infinity, and multipliers at which the
    float32 form (two roundings) and the double form (one) part: bit-identical to numpy"""
    got = _gather(resident, cases.NOISE_CONTEXT, False, True, dtype, cases.noise_records())
    _check_both(got, cases.noise_reference(dtype), 'noise %s' % np.dtype(dtype).name)


def test_a_batch_of_one(resident):
    context, label6 = (6, 34, 34), True
    for dtype, row in ((np.float32, 13), (np.uint8, 22)):
        case = (context, label6, True, dtype)
        rec = cases.record_case(case)[5][row:row + 1]
        assert rec['rot'][0] == (1, 3)[dtype == np.uint8]
        got = _gather(resident, context, label6, True, dtype, rec)
        ref = cases.record_reference(case)
        _check_both(got, (ref[0][row:row + 1], ref[1][row:row + 1]), 'batch 1, row %d' % row)
        again = _gather(resident, context, label6, True, dtype, rec)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


@pytest.mark.parametrize('dtype', [np.float32, np.uint8], ids=['float32', 'uint8'])
def test_the_largest_batch_the_entry_point_allows(resident, dtype):
    """65535 examples of (2, 2, 2), the last blockIdx.y: the records cycle through the table
    and so does the reference; the same call twice gives the same bytes"""
    case = ((2, 2, 2), False, True, dtype)
    table = cases.record_case(case)[5]
    pick = np.arange(65535) % len(table)
    rec = table[pick]
    ref = cases.record_reference(case)
    got = _gather(resident, (2, 2, 2), False, True, dtype, rec)
    _check_both(got, (ref[0][pick], ref[1][pick]), 'batch 65535 %s' % np.dtype(dtype).name)
    again = _gather(resident, (2, 2, 2), False, True, dtype, rec)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
