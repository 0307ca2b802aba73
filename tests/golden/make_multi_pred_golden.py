"""Dev-time script (beside make_golden.py; never imported by the test-suite): runs the
REFERENCE's own fplsynapses.rm_tbar_multi_pred on a dozen small point sets and stores inputs
and outputs - data only - in tests/golden/multi_pred.npz.

    python tests/golden/make_multi_pred_golden.py

The reference is imported through _ref_import (inert stubs for its absent third-party
modules).  Its label query, flyem_syn_eval.eval.get_labels - one of those stubs - is patched to
return the case's label array.  Keys: '<case>.locs', '.conf', '.thresh', optionally '.labels',
and the three outputs '.rm_idx', '.mv_idx', '.mv_loc'.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def f32(values):
    """float32-valued confidences, held as float64"""
    return np.asarray(values, np.float32).astype(np.float64)


def cases():
    rs = np.random.RandomState(20)
    far = np.array([[400.0, 400, 400], [10, 300, 50], [250, 20, 310]])
    out = {}
    # a T-bar on the border z = 512, found by both substacks
    out['two_border_duplicates'] = dict(
        locs=np.concatenate([[[100.0, 100, 511], [102, 101, 513]], far]),
        conf=f32([0.9, 0.7, 0.8, 0.6, 0.95]))
    # the centre of (0,0,0) and (29,0,0) is (14,0,0); (14,29,0) lies 29 from it and more than 32
    # from both: a neighbour of no first candidate, removed by the ball around the moved centre
    out['chain_reaches_a_stranger'] = dict(
        locs=np.array([[200.0, 200, 200], [229, 200, 200], [214, 229, 200], [214, 229, 262]]),
        conf=f32([0.9, 0.9, 0.5, 0.4]))
    # coincident points are no neighbours of each other at first, but candidates of a moved centre
    out['coincident_points'] = dict(
        locs=np.array([[50.0, 50, 50], [50, 50, 50], [60, 52, 50], [300, 300, 300],
                       [300, 300, 300]]),
        conf=f32([0.8, 0.6, 0.7, 0.9, 0.5]))
    out['different_labels'] = dict(
        locs=np.array([[50.0, 50, 50], [55, 50, 50], [58, 55, 50], [200, 200, 200], [204, 200, 200]]),
        conf=f32([0.8, 0.6, 0.7, 0.9, 0.5]), labels=np.array([7, 8, 7, 3, 4], np.uint64))
    out['exactly_thresh'] = dict(
        locs=np.array([[100.0, 100, 100], [130, 100, 100], [300, 300, 300], [318, 324, 300],
                       [500, 500, 500], [500, 500, 529]]),
        conf=f32([0.9, 0.8, 0.7, 0.6, 0.5, 0.4]))
    pts = rs.randint(0, 60, (24, 3)).astype(np.float64)
    out['tied_confidences'] = dict(locs=pts, conf=f32(np.repeat([0.5, 0.75], 12)))
    # 1 removes 0 and 2; 0 and 2 are visited later and skipped; 3 merges with 4 alone
    out['visited_point_already_removed'] = dict(
        locs=np.array([[100.0, 100, 100], [110, 100, 100], [120, 100, 100], [150, 100, 100],
                       [160, 104, 100]]),
        conf=f32([0.5, 0.9, 0.6, 0.7, 0.3]))
    out['empty'] = dict(locs=np.zeros((0, 3)), conf=np.zeros(0))
    out['one_point'] = dict(locs=np.array([[5.0, 6, 7]]), conf=f32([0.5]))
    pts = rs.randint(0, 120, (200, 3))
    out['random_200'] = dict(locs=pts.astype(np.float64), conf=f32(rs.rand(200) * 0.75 + 0.25))
    out['random_200_int_locs_labels'] = dict(locs=pts.astype(np.int64),
                                             conf=f32(rs.rand(200) * 0.75 + 0.25),
                                             labels=rs.randint(0, 3, 200).astype(np.uint64))
    pts = rs.randint(0, 100, (150, 3)) + np.array([0.5, 0.25, 0.125])
    out['random_150_fractional_thresh_20'] = dict(locs=pts, conf=f32(rs.rand(150) * 0.75 + 0.25),
                                                  thresh=20)
    return out


def main():
    from _ref_import import import_reference
    import_reference()
    from flypylib import fplsynapses as ref
    store = {}
    for name, c in cases().items():
        tbars = {'locs': c['locs'], 'conf': c['conf']}
        thresh = c.get('thresh', 30)
        if 'labels' in c:
            ref.eval.get_labels = lambda node, segm, tb, ll=c['labels']: ll
            rm, mv, loc = ref.rm_tbar_multi_pred(tbars, None, 'segmentation', thresh)
            store[name + '.labels'] = c['labels']
        else:
            rm, mv, loc = ref.rm_tbar_multi_pred(tbars, None, None, thresh)
        store.update({name + '.locs': c['locs'], name + '.conf': c['conf'],
                      name + '.thresh': np.array(thresh), name + '.rm_idx': rm,
                      name + '.mv_idx': mv, name + '.mv_loc': loc})
        print('%-36s N %3d moved %3d removed %3d' % (name, len(c['conf']), mv.sum(), rm.sum()))
    np.savez_compressed(os.path.join(HERE, 'multi_pred.npz'), **store)


if __name__ == '__main__':
    main()
