"""The merge loop of fplsynapses.rm_tbar_multi_pred run per component, for solver='device'.

The reference loop is sequential in order of falling confidence, and its interactions are not
confined to the components of the neighbour graph: a moved centre is a rounded weighted mean, no
point of the set, and its ball can hold a "stranger" that is a partner of no candidate.  So the
partition is optimistic and the independence is checked while running:

  1. partition   the connected components of the neighbour table (near.pairs_numpy's superset
                 0 < s <= T2), by min-label propagation: a component's label is its smallest
                 point index.
  2. solve       every component runs the loop of _multi_pred_sparse by itself, over its points in
                 the global order np.argsort(-conf); the balls around moved centres are asked of
                 ALL points.
  3. touch rule  a run flags its component as soon as something happens that it cannot reproduce
                 exactly: a point of another component passes the distance and label tests of a
                 ball query, whatever its removed state (that component is flagged too); a
                 candidate set exceeds `cand_cap` or comes out empty; a mean is not finite; a
                 point moves more than `max_moves` times; the component has more than `comp_cap`
                 points.
  4. closure     the flagged components form a set S.  The host runs the loop over the points of
                 S only, in the global order; a ball that holds a point outside S adds that
                 point's component to S and the run over S is repeated, until nothing outside S
                 is touched.  The results of the components outside S are kept.

At the end every component outside S was processed touching nothing outside itself and S was
processed in the global order touching nothing outside S, so the interleaved sequential run of the
reference gives the same rm_idx, mv_idx, mv_loc.

merge_numpy is the numpy executor of this scheme and the specification of libfplmerge.so's
kernels (include/fplmerge.h); merge_device is the same on the GPU.  Both return the three arrays
of rm_tbar_multi_pred(method='sparse') and fill the same `info`:

  components       connected components of the neighbour table with two points or more
  largest          the points of the largest of them
  sweeps           sweeps of the label propagation, the one that changes nothing included
  host_components  components in S at the end (one-point components counted)
  host_points      their points
  closure_rounds   runs of the host loop over S (0 if no component was flagged)

CAND_CAP is 7 at the most: below 8 elements np.sum is a plain left-to-right loop, which is what
the kernel reproduces; the pairwise form numpy uses from 8 on is left to the host.
"""
import time

import numpy as np

from . import _device, _mergecapi, near
from .match import _points, threshold2

CAND_CAP = _mergecapi.CAND_CAP      # candidates of one mean, the point itself included
# points of a component a run accepts.  Border duplicates chain along the plane they straddle: on
# the realistic lists of DESIGN.md section 14.1 half the components are pairs, the largest of 10^5
# points has 72 points and a cap of 16 would send a sixth of the points to the host.
COMP_CAP = 128
MAX_MOVES = 16                      # moves of one point before its component is flagged
INFO_KEYS = ('components', 'largest', 'sweeps', 'host_components', 'host_points', 'closure_rounds')
_HOST = "use solver='host', which runs the loop in the inputs' own arithmetic"


def check_caps(cand_cap, comp_cap, max_moves):
    for name, v, hi in (('cand_cap', cand_cap, _mergecapi.CAND_CAP), ('comp_cap', comp_cap, _mergecapi.COMP_CAP),
                        ('max_moves', max_moves, _mergecapi.MAX_MOVES)):
        if not 1 <= int(v) <= hi:
            raise ValueError('%s %r must lie in [1, %d]' % (name, v, hi))
    return int(cand_cap), int(comp_cap), int(max_moves)


def check_inputs(pos, conf, ll):
    """(float64 points, float64 confidences, int64 label codes) of inputs whose host loop runs in
    float64, or a ValueError that names solver='host'"""
    pos, conf, ll = np.asarray(pos), np.asarray(conf), np.asarray(ll)
    if pos.ndim != 2 or pos.shape[1] != 3:
        raise ValueError('points must be N x 3, got %r' % (pos.shape,))
    n = pos.shape[0]
    if conf.shape != (n,) or ll.reshape(-1).shape != (n,):
        raise ValueError('%d points with confidences of shape %r and labels of shape %r'
                         % (n, conf.shape, ll.shape))
    if conf.dtype != np.float64:
        raise ValueError("solver='device' runs the loop in float64: the confidences are %s; %s"
                         % (conf.dtype, _HOST))
    if pos.dtype.kind in 'iu':
        # differences, their squares and the sums of three are exact in both arithmetics
        if n and int(np.abs(pos).max()) > 2 ** 24:
            raise ValueError("solver='device' runs the loop in float64: integer locations beyond "
                             '2^24 are not exact there; %s' % _HOST)
    elif pos.dtype != np.float64:
        raise ValueError("solver='device' runs the loop in float64: the locations are %s; %s"
                         % (pos.dtype, _HOST))
    pts = _points(pos)
    if n and not (np.all(np.isfinite(pts)) and np.abs(pts).max() < 2.0 ** 52):
        raise ValueError('the points must be finite and below 2^52 in magnitude; %s' % _HOST)
    ll = ll.reshape(-1)
    if ll.dtype.kind in 'iub':
        codes = ll.astype(np.uint64).view(np.int64) if ll.dtype.kind == 'u' else ll.astype(np.int64)
    elif ll.dtype.kind == 'f':
        if np.isnan(ll).any():
            raise ValueError('a NaN label equals no label, itself included; %s' % _HOST)
        codes = (ll.astype(np.float64) + 0.0).view(np.int64)       # -0.0 + 0.0 is +0.0
    else:
        raise ValueError('labels of dtype %s have no 64-bit code; %s' % (ll.dtype, _HOST))
    return pts, np.ascontiguousarray(conf), np.ascontiguousarray(codes)


def rank_of(conf):
    """(tt_idx, rank): the reference's np.argsort(-conf) - its quicksort decides ties, and ties
    inside a component matter - and every point's place in it, int32"""
    tt_idx = np.argsort(-conf)
    rank = np.empty(len(conf), np.int32)
    rank[tt_idx] = np.arange(len(conf), dtype=np.int32)
    return tt_idx, rank


def partition_numpy(indptr, indices):
    """(comp, sweeps): int32 labels, the smallest index of every point's component in the CSR
    table, by the sweeps of libfplmerge.so's sweep_kernel: a point takes the minimum of its own
    label and its row's labels of the sweep before"""
    n = len(indptr) - 1
    comp = np.arange(n, dtype=np.int32)
    owner = np.repeat(np.arange(n), np.diff(indptr))
    sweeps = 0
    while n:
        new = comp.copy()
        np.minimum.at(new, owner, comp[indices])
        sweeps += 1
        if np.array_equal(new, comp):
            break
        comp = new
    return comp, sweeps


def group_numpy(indptr, comp, rank):
    """(members, starts): the points whose row of the table is not empty, by (component, rank),
    and the K + 1 offsets of the K components among them"""
    active = np.nonzero(np.diff(indptr) > 0)[0]
    members = active[np.lexsort((rank[active], comp[active]))]
    c = comp[members]
    first = np.nonzero(np.concatenate([[True], c[1:] != c[:-1]]))[0] if len(c) else np.zeros(0, np.int64)
    return members, np.concatenate([first, [len(members)]]).astype(np.int64)


class _State:
    """what a run reads and writes"""

    def __init__(self, pos, conf, ll, thresh, comp, f_indptr, f_indices, grid):
        self.pos, self.conf, self.ll, self.thresh, self.comp = pos, conf, ll, thresh, comp
        self.indptr, self.indices, self.grid = f_indptr, f_indices, grid
        n = len(conf)
        self.rm = np.zeros(n, 'bool')
        self.mv = np.zeros(n, 'bool')
        self.mv_loc = np.zeros((n, 3), 'int')


def _run_component(st, c, members, cand_cap, comp_cap, max_moves):
    """the loop over one component's points (in the global order), as libfplmerge.so's
    solve_kernel runs it -> the set of component labels it flags (empty: it ran clean)"""
    pos, conf, ll, comp, rm = st.pos, st.conf, st.ll, st.comp, st.rm
    if len(members) > comp_cap:
        return {c}
    for ii in members:
        if rm[ii] or st.indptr[ii + 1] == st.indptr[ii]:
            continue
        row = st.indices[st.indptr[ii]:st.indptr[ii + 1]]
        jj = row[(ll[row] == ll[ii]) & np.logical_not(rm[row])]
        if jj.size == 0:
            continue
        st.mv[ii] = True
        cand = np.sort(np.append(jj, ii))
        old_loc = pos[ii, :]
        moves = 0
        while True:
            if cand.size > cand_cap or cand.size == 0:
                return {c}
            # the expressions of fplsynapses._merge_visit, so that any dtype runs as it does there
            ww = conf[cand]
            ww = ww / np.sum(ww)                 # fewer than 8 elements: a left-to-right loop
            rows = ww.reshape((-1, 1)) * pos[cand]
            mean = rows[0]
            for r in rows[1:]:
                mean = mean + r
            if not np.all(np.abs(mean) < 2.0 ** 62):              # NaN and infinity included
                return {c}
            st.mv_loc[ii, :] = np.round(mean)
            if np.array_equal(old_loc, st.mv_loc[ii, :]):
                break
            if moves == max_moves:
                return {c}
            moves += 1
            old_loc = st.mv_loc[ii, :].copy()
            ball = st.grid.ball(st.mv_loc[ii, :])
            d = np.sqrt(np.sum((pos[ball] - st.mv_loc[ii, :]) ** 2, axis=1))
            hit = ball[(d < st.thresh) & (ll[ball] == ll[ii])]
            strangers = hit[comp[hit] != c]
            cand = hit[(comp[hit] == c) & np.logical_not(rm[hit])]
            if strangers.size:
                return {c} | set(comp[strangers].tolist())
        rm[cand] = True
    return set()


def _closure(st, tt_rank, flagged):
    """the host loop over the flagged components, grown until it touches nothing outside ->
    (host_components, host_points, closure_rounds).  st.rm / mv / mv_loc hold the runs' results
    on entry and the merged results on return."""
    from .fplsynapses import _merge_visit
    if not len(flagged):
        return 0, 0, 0
    comp = st.comp
    in_s = np.isin(comp, np.asarray(sorted(flagged), comp.dtype))
    rounds = 0
    while True:
        rounds += 1
        pts = np.nonzero(in_s)[0]
        st.rm[pts] = False
        st.mv[pts] = False
        st.mv_loc[pts] = 0
        touched = []

        def watch(hit):
            out = hit[np.logical_not(in_s[hit])]
            if out.size:
                touched.extend(comp[out].tolist())

        has = (st.indptr[pts + 1] - st.indptr[pts]) > 0
        todo = pts[has]
        for ii in todo[np.argsort(tt_rank[todo], kind='stable')]:
            if st.rm[ii]:
                continue
            _merge_visit(ii, st.indices[st.indptr[ii]:st.indptr[ii + 1]], st.pos, st.conf, st.ll,
                         st.thresh, st.grid, st.rm, st.mv, st.mv_loc, watch)
            if touched:
                break
        if not touched:
            break
        in_s |= np.isin(comp, np.asarray(sorted(set(touched)), comp.dtype))
    return int(len(np.unique(comp[in_s]))), int(in_s.sum()), rounds


def _filtered(pos, indptr, indices, thresh):
    from .fplsynapses import _sparse_rows
    return _sparse_rows(pos, indptr, indices, thresh)


def _empty(pos, info):
    if info is not None:
        info.update(dict.fromkeys(INFO_KEYS, 0))
    return np.zeros(0, 'bool'), np.zeros(0, 'bool'), np.zeros(np.asarray(pos).shape, 'int')


def merge_numpy(pos, conf, ll, neighbor_thresh, cand_cap=CAND_CAP, comp_cap=COMP_CAP,
                max_moves=MAX_MOVES, info=None):
    """rm_tbar_multi_pred(method='sparse')'s (rm_idx, mv_idx, mv_loc) by the scheme above, in
    numpy: the specification of merge_device, caps and `info` included.  Unlike merge_device it
    takes any inputs the host loop takes - it is numpy all the way."""
    cand_cap, comp_cap, max_moves = check_caps(cand_cap, comp_cap, max_moves)
    pos, conf, ll = np.asarray(pos), np.asarray(conf), np.asarray(ll).reshape(-1)
    n = pos.shape[0]
    if n == 0:
        return _empty(pos, info)
    indptr, indices = near.pairs_numpy(pos, neighbor_thresh)
    comp, sweeps = partition_numpy(indptr, indices)
    _, f_indptr, f_indices = _filtered(pos, indptr, indices, neighbor_thresh)
    tt_idx, rank = rank_of(conf)
    members, starts = group_numpy(indptr, comp, rank)
    st = _State(pos, conf, ll, neighbor_thresh, comp, f_indptr, f_indices,
                near.CellGrid(pos, neighbor_thresh))
    flagged = set()
    for k in range(len(starts) - 1):
        mem = members[starts[k]:starts[k + 1]]
        flagged |= _run_component(st, int(comp[mem[0]]), mem, cand_cap, comp_cap, max_moves)
    hc, hp, rounds = _closure(st, rank, flagged)
    st.rm[st.mv] = False
    if info is not None:
        info.update(components=len(starts) - 1, largest=int(np.diff(starts).max()) if len(starts) > 1 else 0,
                    sweeps=sweeps, host_components=hc, host_points=hp, closure_rounds=rounds)
    return st.rm, st.mv, st.mv_loc


# ---- device path ---------------------------------------------------------------------------

def _torch():
    return _device.require_torch('the device merge needs', "use solver='host' for the host loop")


def torch_device(device):
    """torch.device of `device`; FplMergeError (then FplNearError) if a library is not built,
    before a GPU that is not there is reported"""
    _mergecapi.load_library()
    _torch()
    return _device.torch_device(device, 'the device merge', near._nearcapi.load_library)


class _Clock:
    """wall-clock milliseconds per stage, synchronised, when a `stages` dict is asked for"""

    def __init__(self, stages, sync):
        self.stages, self.sync = stages, sync
        self.t = time.perf_counter()

    def lap(self, name, device=True):
        if self.stages is None:
            return
        if device:
            self.sync()
        now = time.perf_counter()
        self.stages[name] = self.stages.get(name, 0.0) + (now - self.t) * 1e3
        self.t = now


def device_table(pts, thresh, dev, torch, stream):
    """libfplnear.so's table of the resident float64 points `p_dev`, left on the device ->
    dict(p, keys, order, offsets (uint32 as int32, n + 1), indices, entries, grid)"""
    capi = near._nearcapi
    n = len(pts)
    t2 = threshold2(thresh)
    origin, cell, dims = near.grid_of(pts, thresh)
    nscr = capi.scratch_bytes(n)
    p_dev = torch.from_numpy(pts).to(dev)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    capi.cell_keys(p_dev.data_ptr(), n, origin, cell, dims, keys.data_ptr(), stream.cuda_stream)
    keys, order = torch.sort(keys)
    scratch = torch.empty((nscr + 7) // 8, dtype=torch.int64, device=dev)
    args = (p_dev.data_ptr(), n, t2, origin, cell, dims, keys.data_ptr(), order.data_ptr(),
            scratch.data_ptr(), nscr)
    total = capi.pairs_count(*args, stream.cuda_stream)
    indices = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    if total:
        capi.pairs_fill(*args, total, indices.data_ptr(), stream.cuda_stream)
    # the n + 1 uint32 row offsets stand behind the 16-byte head of the scratch
    offsets = scratch.view(torch.int32)[4:4 + n + 1]
    return dict(p=p_dev, keys=keys, order=order, offsets=offsets, indices=indices, entries=total,
                grid=(origin, cell, dims), scratch=scratch)


def compact(flags, n, dev, torch, stream):
    """the ascending indices (int32, resident) of the non-zero entries of flags[:n]"""
    nscr = _mergecapi.scratch_bytes(n)
    scratch = torch.empty((nscr + 7) // 8, dtype=torch.int64, device=dev)
    total = _mergecapi.flags_count(flags.data_ptr(), n, scratch.data_ptr(), nscr, stream.cuda_stream)
    out = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    _mergecapi.flags_fill(flags.data_ptr(), n, scratch.data_ptr(), nscr, total, out.data_ptr(),
                          stream.cuda_stream)
    return out[:total]


def merge_device(pos, conf, ll, neighbor_thresh, device, cand_cap=CAND_CAP, comp_cap=COMP_CAP,
                 max_moves=MAX_MOVES, info=None, stages=None):
    """merge_numpy on the GPU: libfplnear.so's table stays resident, libfplmerge.so filters its
    rows, labels and groups the components and runs the loop a lane per component; only the flags,
    the three arrays and, if a component was flagged, what the closure on the host reads are
    downloaded.  np.argsort(-conf) stays on the host.  `stages`, a dict, receives the wall-clock
    milliseconds of every stage (which synchronises between them).  No host fallback."""
    cand_cap, comp_cap, max_moves = check_caps(cand_cap, comp_cap, max_moves)
    pts, conf, codes = check_inputs(pos, conf, ll)
    n = len(pts)
    dev = torch_device(device)
    torch = _torch()
    if n == 0:
        return _empty(pos, info)
    if n > _mergecapi.MAX_POINTS:
        raise ValueError('%d points exceed the 2^31 - 2 the kernels index; merge them in parts' % n)
    thresh = float(neighbor_thresh)
    if not (np.isfinite(thresh) and thresh > 0):
        raise ValueError('neighbor_thresh %r must be finite and positive' % (neighbor_thresh,))
    capi = _mergecapi
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        s = stream.cuda_stream
        clock = _Clock(stages, stream.synchronize)
        tt_idx, rank = rank_of(conf)
        conf_d = torch.from_numpy(conf).to(dev)
        lab_d = torch.from_numpy(codes).to(dev)
        rank_d = torch.from_numpy(rank).to(dev)
        clock.lap('argsort_upload')
        tab = device_table(pts, neighbor_thresh, dev, torch, stream)
        origin, cell, dims = tab['grid']
        p, offsets, indices, entries = tab['p'].data_ptr(), tab['offsets'], tab['indices'], tab['entries']
        clock.lap('table')
        # the rows the reference keeps
        has = torch.empty(n, dtype=torch.int32, device=dev)
        f_offsets = torch.empty(n + 1, dtype=torch.int32, device=dev)
        head = torch.zeros(2, dtype=torch.int64, device=dev)
        f_entries = capi.rows_count(p, n, thresh, offsets.data_ptr(), indices.data_ptr(), entries,
                                    has.data_ptr(), f_offsets.data_ptr(), head.data_ptr(), s)
        f_indices = torch.empty(max(f_entries, 1), dtype=torch.int32, device=dev)
        capi.rows_fill(p, n, thresh, offsets.data_ptr(), indices.data_ptr(), entries,
                       f_offsets.data_ptr(), f_entries, f_indices.data_ptr(), s)
        clock.lap('filter')
        # the components
        comp = torch.empty(n, dtype=torch.int32, device=dev)
        other = torch.empty(n, dtype=torch.int32, device=dev)
        changed = torch.zeros(1, dtype=torch.int32, device=dev)
        sweeps = capi.labels(offsets.data_ptr(), indices.data_ptr(), n, entries, comp.data_ptr(),
                             other.data_ptr(), changed.data_ptr(), n + 1, s)
        clock.lap('labels')
        # the points by (component, rank), the components' starts
        gkeys = torch.empty(n, dtype=torch.int64, device=dev)
        capi.group_keys(offsets.data_ptr(), comp.data_ptr(), rank_d.data_ptr(), n, gkeys.data_ptr(), s)
        gkeys, members = torch.sort(gkeys)
        bflags = torch.empty(n + 1, dtype=torch.int32, device=dev)
        capi.boundaries(gkeys.data_ptr(), n, bflags.data_ptr(), s)
        starts = compact(bflags, n + 1, dev, torch, stream)
        n_comp = len(starts) - 1
        largest = int((starts[1:] - starts[:-1]).max().item()) if n_comp > 0 else 0
        clock.lap('sort')
        # the loop
        rm = torch.zeros(n, dtype=torch.uint8, device=dev)
        mv = torch.zeros(n, dtype=torch.uint8, device=dev)
        mv_loc = torch.zeros((n, 3), dtype=torch.int64, device=dev)
        flagged = torch.zeros(n, dtype=torch.int32, device=dev)
        if n_comp > 0:
            capi.solve(p, conf_d.data_ptr(), lab_d.data_ptr(), comp.data_ptr(), n, thresh, origin,
                       cell, dims, tab['keys'].data_ptr(), tab['order'].data_ptr(),
                       f_offsets.data_ptr(), f_indices.data_ptr(), f_entries, members.data_ptr(),
                       starts.data_ptr(), n_comp, cand_cap, comp_cap, max_moves, rm.data_ptr(),
                       mv.data_ptr(), mv_loc.data_ptr(), flagged.data_ptr(), s)
        ids = compact(flagged, n, dev, torch, stream)
        clock.lap('solve')
        rm_h = rm.cpu().numpy().astype('bool')
        mv_h = mv.cpu().numpy().astype('bool')
        loc_h = mv_loc.cpu().numpy().astype('int', copy=False)
        ids_h = ids.cpu().numpy()
        need = len(ids_h) > 0
        if need:
            # what the closure reads: the partition, the filtered table, the cell grid
            comp_h = comp.cpu().numpy()
            f_indptr = f_offsets.cpu().numpy().view(np.uint32).astype(np.int64)
            f_ind_h = f_indices[:f_entries].cpu().numpy()
            grid = _grid_from(pts, neighbor_thresh, tab, n)
        clock.lap('download')
    hc = hp = rounds = 0
    if need:
        st = _State(np.asarray(pos), np.asarray(conf), np.asarray(ll).reshape(-1), neighbor_thresh,
                    comp_h, f_indptr, f_ind_h, grid)
        st.rm, st.mv, st.mv_loc = rm_h, mv_h, loc_h
        hc, hp, rounds = _closure(st, rank, ids_h.tolist())
    rm_h[mv_h] = False
    clock.lap('closure_host', device=False)
    if info is not None:
        info.update(components=n_comp, largest=largest, sweeps=int(sweeps), host_components=hc,
                    host_points=hp, closure_rounds=rounds)
    return rm_h, mv_h, loc_h


def _grid_from(pts, thresh, tab, n):
    """near.CellGrid of the points from the sorted keys the device holds: no second sort"""
    grid = near.CellGrid.__new__(near.CellGrid)
    grid.locs, grid.n = pts, n
    grid.origin, grid.cell, grid.dims = tab['grid']
    grid.keys = tab['keys'].cpu().numpy()
    grid.order = tab['order'].cpu().numpy()
    return grid
