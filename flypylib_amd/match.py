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
  match_device                pair_costs and match_sparse on the GPU (libfplassign.so), from the
                              resident table of pairs_device: only the matched pairs come back.
                              components_numpy is the specification of its labelling stage.
"""
import numpy as np

from . import _assigncapi, _device, _matchcapi

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


def solve_component(i, j, cost):
    """(mi, mj): the matched pairs of ONE connected component, given its pairs (i, j, cost < 0):
    linear_sum_assignment on the block of min(cost, 0) over the component's own rows and
    columns, absent pairs costing 0; the assigned pairs with cost < 0 are kept."""
    from scipy.optimize import linear_sum_assignment
    rows, ri = np.unique(i, return_inverse=True)
    cols, ci = np.unique(j, return_inverse=True)
    block = np.zeros((len(rows), len(cols)))
    block[ri, ci] = cost
    br, bc = linear_sum_assignment(block)
    ok = block[br, bc] < 0
    return rows[br[ok]], cols[bc[ok]]


def components_numpy(n_pred, i, j):
    """The label of every pair (i[e], j[e]) of a bipartite pair graph: the smallest prediction
    index of the pair's connected component (int64, one per pair).  Min-label propagation in
    plain numpy, the specification of libfplassign.so's labelling stage: every prediction
    starts with its own index, every ground-truth point above all of them, and both ends of
    every pair are lowered to their minimum until nothing changes.  Only the partition it
    induces matters to the matching; it is scipy.sparse.csgraph.connected_components'."""
    i, j = np.asarray(i, np.int64).reshape(-1), np.asarray(j, np.int64).reshape(-1)
    if len(i) == 0:
        return np.zeros(0, np.int64)
    pl = np.arange(max(int(n_pred), int(i.max()) + 1), dtype=np.int64)
    gl = np.full(int(j.max()) + 1, np.iinfo(np.int64).max, np.int64)
    while True:                                   # as many rounds as the widest component is across
        low = np.minimum(pl[i], gl[j])
        if np.array_equal(low, pl[i]) and np.array_equal(low, gl[j]):
            return low
        np.minimum.at(pl, i, low)
        np.minimum.at(gl, j, low)


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
            ci, cj = solve_component(i[a:b], j[a:b], cost[a:b])
            mi.append(ci)
            mj.append(cj)
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


def _pairs_resident(torch, dev, pred, gt, t2):
    """the table of pairs_device left on the device: (pred tensor, gt tensor, the 2 x rows
    int32 columns); pred and gt are non-empty.  The fill is queued on the current stream."""
    n, m = len(pred), len(gt)
    if max(n, m) > _matchcapi.MAX_POINTS:
        raise ValueError('%d x %d points exceed the 2^31 - 1 of a kind the match kernels index; '
                         'match them in parts' % (n, m))
    nscr = _matchcapi.scratch_bytes(n, m)
    stream = torch.cuda.current_stream(dev)
    p_dev, g_dev = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    scratch = torch.empty((nscr + 7) // 8, dtype=torch.int64, device=dev)
    args = (p_dev.data_ptr(), n, g_dev.data_ptr(), m, t2, scratch.data_ptr(), nscr)
    total = _matchcapi.pairs_count(*args, stream.cuda_stream)
    cols = torch.empty((2, total), dtype=torch.int32, device=dev)
    if total:
        _matchcapi.pairs_fill(*args, total, cols[0].data_ptr(), cols[1].data_ptr(),
                              stream.cuda_stream)
    return p_dev, g_dev, cols


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
    with torch.cuda.device(dev):
        _, _, cols = _pairs_resident(torch, dev, pred, gt, t2)
        torch.cuda.current_stream(dev).synchronize()
        host = cols.cpu().numpy()
    if info is not None:
        info.update(rows=cols.shape[1], segments=_matchcapi.segments(n, m))
    return host[0], host[1]


# ---- device solver -----------------------------------------------------------------------------

def _device_labels(lbls, n, what):
    """int64 labels for the upload, or ValueError: the kernels compare int64"""
    lbls = np.asarray(lbls).reshape(-1)
    if len(lbls) != n:
        raise ValueError('%d %s labels for %d points' % (len(lbls), what, n))
    if lbls.dtype.kind not in 'iub':
        raise ValueError("%s labels of dtype %s: solver='device' compares int64 labels; use "
                         "solver='host' for labels of any other kind" % (what, lbls.dtype))
    if lbls.dtype.kind == 'u' and lbls.size and int(lbls.max()) > np.iinfo(np.int64).max:
        raise ValueError("%s labels above 2^63 - 1 do not fit int64; use solver='host' for them"
                         % what)
    return np.ascontiguousarray(lbls, dtype=np.int64)


class _Compactor:
    """count, scan and ordered fill of libfplassign.so around torch tensors, one stream"""

    def __init__(self, torch, dev, stream):
        self.torch, self.dev, self.stream = torch, dev, stream.cuda_stream

    def empty(self, n, dtype=None):
        return self.torch.empty(n, dtype=dtype or self.torch.int32, device=self.dev)

    def count(self, flags):
        """(the flagged entries, the scratch the fill needs)"""
        n = flags.numel()
        nscr = _assigncapi.scratch_bytes(n)
        scratch = self.empty(nscr // 8, self.torch.int64)
        return _assigncapi.flags_count(flags.data_ptr(), n, scratch.data_ptr(), nscr, self.stream), \
            (scratch, nscr)

    def fill(self, flags, scratch, capacity, **columns):
        _assigncapi.flags_fill(flags.data_ptr(), flags.numel(), scratch[0].data_ptr(), scratch[1],
                               capacity, self.stream,
                               **{k: v.data_ptr() for k, v in columns.items()})


def _costs_resident(c, cols, p_dev, g_dev, t, lp_dev, lg_dev, label_add, conf_dev, thd):
    """stage a on resident tensors: (the predictions selected, i, j, cost of the admissible
    rows in table order - None where there is none)"""
    n, m, rows = p_dev.shape[0], g_dev.shape[0], cols.shape[1]
    n_sel, rank = n, None
    if thd is not None:
        sel = c.empty(n)
        _assigncapi.conf_flags(conf_dev.data_ptr(), n, thd, sel.data_ptr(), c.stream)
        n_sel, scr = c.count(sel)
        rank = c.empty(n)
        c.fill(sel, scr, 0, rank_out=rank)
    if rows == 0 or n_sel == 0:
        return n_sel, None, None, None
    i_all, cost_all, keep = c.empty(rows), c.empty(rows, c.torch.float64), c.empty(rows)
    _assigncapi.pair_costs(cols[0].data_ptr(), cols[1].data_ptr(), rows, p_dev.data_ptr(), n,
                           g_dev.data_ptr(), m, t, 0 if lp_dev is None else lp_dev.data_ptr(),
                           0 if lg_dev is None else lg_dev.data_ptr(), label_add,
                           0 if rank is None else rank.data_ptr(), i_all.data_ptr(),
                           cost_all.data_ptr(), keep.data_ptr(), c.stream)
    adm, scr = c.count(keep)
    if adm == 0:
        return n_sel, None, None, None
    pi, pj, pc = c.empty(adm), c.empty(adm), c.empty(adm, c.torch.float64)
    c.fill(keep, scr, adm, a=i_all, b=cols[1], c=cost_all, a_out=pi, b_out=pj, c_out=pc)
    return n_sel, pi, pj, pc


def _labels_resident(c, pi, pj, n_pred, n_gt):
    """stage b on resident tensors: (the label of every pair, the sweeps)"""
    adm = pi.numel()
    work = c.empty(n_pred + n_gt + 1)
    label = c.empty(adm)
    sweeps = _assigncapi.labels(pi.data_ptr(), pj.data_ptr(), adm, n_pred, n_gt, work.data_ptr(),
                                work[n_pred:].data_ptr(), work[n_pred + n_gt:].data_ptr(),
                                label.data_ptr(), n_pred + n_gt + 2, c.stream)
    return label, sweeps


def _label_add(dist_thresh):
    """what pair_costs adds where labels differ: its own expression, with numpy's own rule for
    the type of the product"""
    return float(((dist_thresh + 1.) * np.ones(1, 'float32'))[0])


def costs_device(pred_locs, gt_locs, i, j, dist_thresh, device, predict_lbls=None,
                 groundtruth_lbls=None, conf=None, thd=None):
    """pair_costs on the GPU, stage a of match_device on its own: (i, j, cost) of the
    admissible rows of the table (i, j), downloaded.  With conf and thd, the rows of the
    predictions with conf >= thd, i renumbered by their rank."""
    pred, gt = _points(pred_locs), _points(gt_locs)
    torch = _torch()
    dev = torch_device(device)
    _assigncapi.load_library()
    table = np.ascontiguousarray(np.stack([np.asarray(i), np.asarray(j)]), dtype=np.int32)
    none = np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64)
    if len(pred) == 0 or len(gt) == 0:
        return none
    lp_dev = lg_dev = conf_dev = None
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        if predict_lbls is not None:
            lp_dev = torch.from_numpy(_device_labels(predict_lbls, len(pred), 'prediction')).to(dev)
            lg_dev = torch.from_numpy(_device_labels(groundtruth_lbls, len(gt), 'ground-truth')).to(dev)
        if conf is not None:
            conf_dev = torch.from_numpy(np.ascontiguousarray(conf, dtype=np.float64)).to(dev)
        _, pi, pj, pc = _costs_resident(
            _Compactor(torch, dev, stream), torch.from_numpy(table).to(dev),
            torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), float(dist_thresh), lp_dev,
            lg_dev, _label_add(dist_thresh) if lp_dev is not None else 0.0, conf_dev,
            None if conf is None else float(thd))
        if pi is None:
            return none
        stream.synchronize()
        return pi.cpu().numpy(), pj.cpu().numpy(), pc.cpu().numpy()


def components_device(n_pred, n_gt, i, j, device, info=None):
    """components_numpy on the GPU, stage b of match_device on its own: the label of every
    pair, downloaded (int32).  `info` receives the sweeps."""
    torch = _torch()
    dev = torch_device(device)
    _assigncapi.load_library()
    i, j = np.ascontiguousarray(i, dtype=np.int32), np.ascontiguousarray(j, dtype=np.int32)
    if len(i) == 0:
        return np.zeros(0, np.int32)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        label, sweeps = _labels_resident(_Compactor(torch, dev, stream), torch.from_numpy(i).to(dev),
                                         torch.from_numpy(j).to(dev), int(n_pred), int(n_gt))
        stream.synchronize()
        if info is not None:
            info['sweeps'] = sweeps
        return label.cpu().numpy()


def match_device(pred_locs, gt_locs, dist_thresh, device, predict_lbls=None, groundtruth_lbls=None,
                 allow_mult=False, conf=None, thresholds=None, info=None):
    """pair_costs and match_sparse on the GPU: the pair table of pairs_device stays resident,
    libfplassign.so costs it, keeps the admissible rows, labels the connected components of
    the pair graph, and solves every component of at most 64 x 64 points a wavefront each;
    only the matched pairs are downloaded.  -> scipy.sparse.csr_matrix of bool, n_pred x n_gt,
    as match_sparse returns it.

    conf, thresholds: one matrix per threshold, in a list, from ONE table - at each threshold
    the predictions with conf >= threshold are kept and renumbered by their rank, so the k-th
    matrix is that of match_device(pred_locs[conf >= thresholds[k]], ...).

    Components beyond the cap are solved on the host by solve_component, the per-component
    code of match_sparse, and merged in.  Labels must be integers that fit int64 (ValueError
    otherwise: solver='host' takes any).  `info`, a dict, receives `components`, `largest` (the
    pairs of the largest component), `overflow` (the components solved on the host) and
    `sweeps` (of the labelling) - numbers, or with thresholds one list of each - and the
    wall-clock milliseconds `table_ms`, `solve_ms` and `download_ms`."""
    import time
    from scipy import sparse
    pred, gt = _points(pred_locs), _points(gt_locs)
    t = float(dist_thresh)
    if not np.isfinite(t):
        raise ValueError('dist_thresh %r is not finite' % (dist_thresh,))
    n, m = len(pred), len(gt)
    if (predict_lbls is None) != (groundtruth_lbls is None):
        raise ValueError('labels of one kind only: give predict_lbls and groundtruth_lbls, or neither')
    if (conf is None) != (thresholds is None):
        raise ValueError('conf and thresholds go together')
    lp = lg = None
    label_add = 0.0
    if predict_lbls is not None:
        lp, lg = _device_labels(predict_lbls, n, 'prediction'), _device_labels(groundtruth_lbls, m, 'ground-truth')
        label_add = _label_add(dist_thresh)
    if conf is not None:
        conf = np.ascontiguousarray(conf, dtype=np.float64).reshape(-1)
        if len(conf) != n:
            raise ValueError('%d confidences for %d predictions' % (len(conf), n))
        thds = [float(v) for v in np.asarray(thresholds).reshape(-1)]
    torch = _torch()
    _assigncapi.load_library()          # a library that is not built is reported before the GPU
    dev = torch_device(device)
    stats = dict(components=[], largest=[], overflow=[], sweeps=[])
    clock = dict(table_ms=0.0, solve_ms=0.0, download_ms=0.0)

    def finish(out):
        if info is not None:
            info.update({k: (v if conf is not None else v[0]) for k, v in stats.items()})
            info.update(clock)
        return out if conf is not None else out[0]

    def none(n_sel):
        for v in stats.values():
            v.append(0)
        return sparse.csr_matrix((n_sel, m), dtype=bool)

    if n == 0 or m == 0:
        if conf is None:
            return finish([none(n)])
        return finish([none(int((conf >= v).sum())) for v in thds])
    i32 = torch.int32
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        t0 = time.perf_counter()
        p_dev, g_dev, cols = _pairs_resident(torch, dev, pred, gt, threshold2(t))
        rows = cols.shape[1]
        lp_dev = lg_dev = conf_dev = None
        if lp is not None:
            lp_dev, lg_dev = torch.from_numpy(lp).to(dev), torch.from_numpy(lg).to(dev)
        if conf is not None:
            conf_dev = torch.from_numpy(conf).to(dev)
        stream.synchronize()
        clock['table_ms'] = (time.perf_counter() - t0) * 1e3
        c = _Compactor(torch, dev, stream)
        st = stream.cuda_stream
        out = []
        for thd in (thds if conf is not None else [None]):
            t0 = time.perf_counter()
            n_sel, pi, pj, pc = _costs_resident(c, cols, p_dev, g_dev, t, lp_dev, lg_dev, label_add,
                                                conf_dev, thd)
            if pi is None:
                out.append(none(n_sel))
                continue
            adm = pi.numel()
            host = []                                   # pairs of the overflow components
            if allow_mult:
                # per ground-truth column the pair of least cost, the lowest i on ties: the
                # first of every run of j in (j, cost, i) order.  The table is in (i, j)
                # order, so two stable sorts give that order.
                by_cost = torch.sort(pc, stable=True).indices
                by_j = torch.sort(pj[by_cost], stable=True)
                order = by_cost[by_j.indices]
                si, sj = pi[order].contiguous(), by_j.values.contiguous()
                first = c.empty(adm)
                _assigncapi.boundaries(sj.data_ptr(), adm, first.data_ptr(), st)
                got, scr = c.count(first)
                mi, mj = c.empty(got), c.empty(got)
                c.fill(first, scr, got, a=si, b=sj, a_out=mi, b_out=mj)
                for k in ('components', 'largest', 'overflow', 'sweeps'):
                    stats[k].append(0)
            else:
                # b. component labels
                label, sweeps = _labels_resident(c, pi, pj, n_sel, m)
                # c. group: (label, i, j) order is a stable sort by label of the (i, j) order
                by_label = torch.sort(label, stable=True)
                order = by_label.indices
                si, sj, sc = pi[order].contiguous(), pj[order].contiguous(), pc[order].contiguous()
                first = c.empty(adm)
                _assigncapi.boundaries(by_label.values.data_ptr(), adm, first.data_ptr(), st)
                n_comp, scr = c.count(first)
                starts = torch.full((n_comp + 1,), adm, dtype=i32, device=dev)
                c.fill(first, scr, n_comp, index_out=starts)
                # d. solve, e. emit
                matched = torch.zeros(adm, dtype=i32, device=dev)
                over = torch.zeros(n_comp, dtype=i32, device=dev)
                _assigncapi.solve(si.data_ptr(), sj.data_ptr(), sc.data_ptr(), adm, starts.data_ptr(),
                                  n_comp, matched.data_ptr(), over.data_ptr(), st)
                got, scr = c.count(matched)
                mi, mj = c.empty(got), c.empty(got)
                c.fill(matched, scr, got, a=si, b=sj, a_out=mi, b_out=mj)
                n_over, scr = c.count(over)
                if n_over:
                    ids = c.empty(n_over)
                    c.fill(over, scr, n_over, index_out=ids)
                    bounds = torch.stack([starts[ids.long()], starts[ids.long() + 1]]).cpu().numpy()
                    for a, b in bounds.T.tolist():
                        host.append((si[a:b].cpu().numpy(), sj[a:b].cpu().numpy(), sc[a:b].cpu().numpy()))
                stats['components'].append(n_comp)
                stats['largest'].append(int((starts[1:] - starts[:-1]).max()))
                stats['overflow'].append(n_over)
                stats['sweeps'].append(sweeps)
            stream.synchronize()
            clock['solve_ms'] += (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            mi, mj = mi.cpu().numpy().astype(np.int64), mj.cpu().numpy().astype(np.int64)
            clock['download_ms'] += (time.perf_counter() - t0) * 1e3
            for hi, hj, hc in host:
                ci, cj = solve_component(hi.astype(np.int64), hj.astype(np.int64), hc)
                mi, mj = np.concatenate([mi, ci]), np.concatenate([mj, cj])
            out.append(sparse.csr_matrix((np.ones(len(mi), bool), (mi, mj)), shape=(n_sel, m)))
    return finish(out)
