"""Sparse matching for obj_pr / obj_pr_curve: the table of close (prediction, ground-truth)
pairs, their exact costs and the matching solved per connected component.

The dense path of fplobjdetect.obj_pr builds an N x M cost matrix and hands all of it to the
assignment solver, although only the pairs closer than the threshold can ever be matched.
Here the work is split in three:

  pairs_numpy / pairs_device  every pair with squared distance s <= T2 - a deliberate,
                              slightly generous superset of the admissible pairs, so that
                              neither executor has to reproduce the other's sqrt rounding.
                              The numpy function is the specification libfplmatch.so's
                              kernels are tested against, row for row.
  pair_costs                  the cost obj_pr computes, on those pairs only, with obj_pr's own
                              expressions; keeps cost < 0.  That set is {cost[i, j] < 0} of the
                              dense matrix exactly.
  match_sparse                the matching, per connected component of the pair graph.
"""
import numpy as np

from . import _device, _matchcapi

BLOCK_ELEMENTS = 1 << 16     # pairs_numpy tests about this many pairs at a time: s and d stay in cache


def threshold2(dist_thresh):
    """T2 = t^2 (1 + 2^-40).  fl(sqrt(s)) - t < 0 implies s < t^2 (1 + 2^-51), far inside."""
    t = float(dist_thresh)
    return (t * t) * (1 + 2.0 ** -40)


def _points(locs):
    locs = np.ascontiguousarray(locs, dtype=np.float64)
    if locs.ndim != 2 or locs.shape[1] != 3:
        raise ValueError('points must be N x 3, got %r' % (locs.shape,))
    return locs


def pairs_numpy(pred_locs, gt_locs, dist_thresh):
    """(i, j): int32 columns of every pair with s <= T2, in ascending (i, j) order, where
    s = (dx*dx + dy*dy) + dz*dz in float64 - the operations, in the order, of numpy's
    (delta ** 2).sum(axis=2) - and T2 = threshold2(dist_thresh).  Row blocks keep the memory
    bounded whatever N and M are."""
    pred, gt = _points(pred_locs), _points(gt_locs)
    t2 = threshold2(dist_thresh)
    n, m = len(pred), len(gt)
    ii, jj = [np.zeros(0, np.int32)], [np.zeros(0, np.int32)]
    if n and m:
        gx, gy, gz = (np.ascontiguousarray(gt[:, a])[None, :] for a in range(3))
        rows = max(1, BLOCK_ELEMENTS // m)
        for r0 in range(0, n, rows):
            p = pred[r0:r0 + rows]
            d = p[:, 0:1] - gx
            s = d * d
            np.subtract(p[:, 1:2], gy, out=d)
            s += d * d
            np.subtract(p[:, 2:3], gz, out=d)
            s += d * d
            bi, bj = np.nonzero(s <= t2)            # C order: ascending (i, j)
            ii.append((bi + r0).astype(np.int32))
            jj.append(bj.astype(np.int32))
    return np.concatenate(ii), np.concatenate(jj)


def pair_costs(pred_locs, gt_locs, i, j, dist_thresh, predict_lbls=None, groundtruth_lbls=None):
    """(i, j, cost) of the rows of a pair table that are admissible: obj_pr's cost - distance
    minus threshold, plus threshold + 1 where the labels differ - below zero.  The labels are
    applied here, on the host."""
    pred, gt = _points(pred_locs), _points(gt_locs)
    i, j = np.asarray(i), np.asarray(j)
    delta = pred[i] - gt[j]
    cost = np.sqrt((delta ** 2).sum(axis=1)) - dist_thresh
    if predict_lbls is not None:
        differ = np.asarray(predict_lbls).reshape(-1)[i] != np.asarray(groundtruth_lbls).reshape(-1)[j]
        cost += (dist_thresh + 1.) * differ.astype('float32')
    keep = cost < 0
    return i[keep], j[keep], cost[keep]


def match_sparse(n_pred, n_gt, i, j, cost, allow_mult=False):
    """The matching of fplobjdetect.obj_match on a sparse pair table (rows (i, j) with
    cost < 0): the summed cost is minimal with every ground-truth point used at most once and,
    unless `allow_mult`, every prediction at most once.  -> scipy.sparse.csr_matrix of bool,
    n_pred x n_gt.

    allow_mult: per ground-truth column the pair of least cost, the lowest i on ties - what
    np.argmin(dists, axis=0) picks.  Otherwise the pair graph falls into connected components
    (scipy.sparse.csgraph.connected_components); each is solved by linear_sum_assignment on its
    own small block of min(cost, 0), absent pairs costing 0, and the assigned pairs with
    cost < 0 are kept.  Every entry of the dense problem is <= 0, so an assignment costs what
    its negative pairs cost, and pairs across components cost 0: the components' optima add up
    to an optimum of the whole.

    Like the dense solver's, the matching is ONE optimum of possibly several.  Where optima of
    different cardinality tie in total cost, the number of matched pairs (num_tp) of the
    sparse and the dense solver may legitimately differ."""
    from scipy import sparse
    n_pred, n_gt = int(n_pred), int(n_gt)
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    cost = np.asarray(cost, np.float64)
    neg = cost < 0
    if not neg.all():
        i, j, cost = i[neg], j[neg], cost[neg]
    if allow_mult:
        order = np.lexsort((i, cost, j))
        first = np.ones(len(order), bool)
        first[1:] = j[order][1:] != j[order][:-1]
        mi, mj = i[order][first], j[order][first]
    elif len(i) == 0:
        mi = mj = np.zeros(0, np.int64)
    else:
        from scipy.optimize import linear_sum_assignment
        from scipy.sparse.csgraph import connected_components
        nodes = n_pred + n_gt
        graph = sparse.csr_matrix((np.ones(len(i), bool), (i, j + n_pred)), shape=(nodes, nodes))
        _, label = connected_components(graph, directed=False)
        comp = label[i]
        order = np.argsort(comp, kind='stable')
        i, j, cost, comp = i[order], j[order], cost[order], comp[order]
        starts = np.flatnonzero(np.r_[True, comp[1:] != comp[:-1]])
        ends = np.r_[starts[1:], len(comp)]
        single = ends - starts == 1                  # a component of one pair is its own optimum
        mi, mj = [i[starts[single]]], [j[starts[single]]]
        for a, b in zip(starts[~single], ends[~single]):
            rows, ri = np.unique(i[a:b], return_inverse=True)
            cols, ci = np.unique(j[a:b], return_inverse=True)
            block = np.zeros((len(rows), len(cols)))
            block[ri, ci] = cost[a:b]
            br, bc = linear_sum_assignment(block)
            ok = block[br, bc] < 0
            mi.append(rows[br[ok]])
            mj.append(cols[bc[ok]])
        mi, mj = np.concatenate(mi), np.concatenate(mj)
    return sparse.csr_matrix((np.ones(len(mi), bool), (mi, mj)), shape=(n_pred, n_gt))


# ---- device path ---------------------------------------------------------------------------

def _torch():
    return _device.require_torch('device matching needs', "use match='sparse' for the host path")


def torch_device(device):
    """torch.device of `device` (an int, or True for the runtime's default device);
    FplMatchError if the library is not built"""
    _torch()
    return _device.torch_device(device, 'device matching', _matchcapi.load_library)


def pairs_device(pred_locs, gt_locs, dist_thresh, device, info=None):
    """pairs_numpy's table from libfplmatch.so: the two float64 tables are uploaded, the
    pairs counted, the columns allocated and filled, and only they are downloaded.  `info`, a
    dict, receives the row count and the segment count of the launch."""
    pred, gt = _points(pred_locs), _points(gt_locs)
    t2 = threshold2(dist_thresh)
    n, m = len(pred), len(gt)
    torch = _torch()
    dev = torch_device(device)
    if n == 0 or m == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    if max(n, m) > _matchcapi.MAX_POINTS:
        raise ValueError('%d x %d points exceed the 2^31 - 1 of a kind the match kernels index; '
                         'match them in parts' % (n, m))
    nscr = _matchcapi.scratch_bytes(n, m)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        p_dev, g_dev = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
        scratch = torch.empty((nscr + 7) // 8, dtype=torch.int64, device=dev)
        args = (p_dev.data_ptr(), n, g_dev.data_ptr(), m, t2, scratch.data_ptr(), nscr)
        total = _matchcapi.pairs_count(*args, stream.cuda_stream)
        cols = torch.empty((2, total), dtype=torch.int32, device=dev)
        if total:
            _matchcapi.pairs_fill(*args, total, cols[0].data_ptr(), cols[1].data_ptr(),
                                  stream.cuda_stream)
        stream.synchronize()
        host = cols.cpu().numpy()
    if info is not None:
        info.update(rows=total, segments=_matchcapi.segments(n, m))
    return host[0], host[1]
