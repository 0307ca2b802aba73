"""Synapse (T-bar) point lists as JSON - the data formats on the output side of the
detection path (reference `flypylib/fplsynapses.py:11-111`) - and the label / mask
volumes training is fed from (`write_labels_mask`, :251-310), and the merging of duplicate
detections along substack borders (`rm_tbar_multi_pred`, :378-449), and the export of training
substacks (`roi_to_substacks`, `get_substack_annotations`, :140-249) on arrays and a
`roi.BlockRoi` in place of a DVID node.  The DVID push and annotation-editing helpers of the
reference need `libdvid` and are not part of this package."""
import json
import os

import numpy as np

from . import fplutils


def _raveler_records(doc):
    """{'data': [{'T-bar': {'location': [x, y, z], 'confidence': c}}, ...]}"""
    tbars = [entry['T-bar'] for entry in doc['data']]
    return ([t['location'] for t in tbars], [t['confidence'] for t in tbars], [])


def _dvid_records(elements):
    """[{'Kind': 'PreSyn', 'Pos': [x, y, z], 'Prop': {'conf': '0.9', 'err': ...}}, ...];
    a list holding one such list is unwrapped; other kinds (PostSyn ...) are skipped;
    a missing confidence reads as 1, a missing error estimate as None"""
    if len(elements) == 1 and isinstance(elements[0], list):
        elements = elements[0]
    pre = [e for e in elements if e['Kind'] == 'PreSyn']
    prop = [e['Prop'] for e in pre]
    return ([e['Pos'] for e in pre],
            [float(p['conf']) if 'conf' in p else 1.0 for p in prop],
            [float(p['err']) if 'err' in p else None for p in prop])


def load_from_json(fn, vol_sz=None, buffer=None):
    """T-bars of a json file (or json text) in either of the formats the reference's
    tools exchange (reference fplsynapses.py:11-76): Raveler ({'data': [{'T-bar': ...}]})
    or DVID annotation elements.  With `buffer` (and `vol_sz`) the points closer than
    the buffer to a face of the volume are dropped.
    -> {'locs': (N, 3), 'conf': (N,), 'err': (N,)}"""
    text = open(fn).read() if os.path.isfile(fn) else fn
    doc = json.loads(text)
    if isinstance(doc, dict) and 'data' in doc:
        locs, conf, err = _raveler_records(doc)
    elif doc is None:
        locs, conf, err = [], [], []
    else:
        locs, conf, err = _dvid_records(doc)
    locs, conf, err = np.asarray(locs), np.asarray(conf), np.asarray(err)
    if locs.size > 0 and buffer is not None and buffer != 0:
        assert vol_sz is not None, 'to apply buffer, must also supply volume size'
        lo = np.asarray(fplutils.to3d(buffer))
        hi = np.asarray(fplutils.to3d(vol_sz)) - lo
        inside = np.all((locs >= lo) & (locs < hi), axis=1)
        locs, conf = locs[inside], conf[inside]
    return {'locs': locs, 'conf': conf, 'err': err}


def _dump(obj, json_file):
    if json_file is not None:
        with open(json_file, 'w') as out:
            json.dump(obj, out)
    return obj


def tbars_to_json_format(tbars_np, json_file=None, user_name='$fpl', labels=None):
    """DVID annotation elements of a {'locs', 'conf'} point list (reference :78-96):
    integer positions, the confidence as a '%.03f' string, optionally the body id"""
    positions = np.asarray(tbars_np['locs']).astype('int').tolist()
    elements = [{'Kind': 'PreSyn', 'Pos': pos,
                 'Prop': {'conf': '%.03f' % c, 'user': user_name}}
                for pos, c in zip(positions, np.asarray(tbars_np['conf']).ravel())]
    if labels is not None:
        for element, body in zip(elements, labels):
            element['body ID'] = str(body)
    return _dump(elements, json_file)


def tbars_to_json_format_raveler(tbars_np, json_file=None):
    """Raveler json of a {'locs', 'conf'} point list (reference :98-111)"""
    positions = np.asarray(tbars_np['locs']).astype('int').tolist()
    doc = {'data': [{'T-bar': {'confidence': '%.03f' % c, 'location': pos}}
                    for pos, c in zip(positions, np.asarray(tbars_np['conf']).ravel())]}
    return _dump(doc, json_file)


def write_labels_mask(tbars, roi_mask, radius_use, radius_ign, buffer_size, prefix, device=None,
                      planner='host'):
    """training labels and mask around annotated T-bars (reference :251-310): label 1
    within `radius_use` of a T-bar; the mask is cleared in the shell between
    `radius_use` and `radius_ign` (neither positive nor negative) and within
    `buffer_size` of the faces.  Written as the reference's '<prefix>_labels.h5' /
    '<prefix>_mask.h5' (dataset 'main') and as '<prefix>_labels.npy' / '<prefix>_mask.npy',
    and returned.

    device=None (default) is the host path: numpy in, numpy out.  device=<int> or True (the
    runtime's default device) renders both volumes with libfpllabels.so's kernel: `roi_mask`
    is a numpy uint8 array (uploaded once) or a contiguous uint8 torch tensor on that device,
    the result a pair of resident uint8 torch tensors that gen_volume2(device=...) and
    FplNetwork.voxel_loss(device=...) take as they are; the files are written only when
    `prefix` is not None.  A T-bar whose cube leaves the volume is a ValueError there
    (labels.plan_tbars).  No host fallback: a missing library raises.

    planner='host' (default) builds the kernel's brick table with numpy (labels.plan_bricks)
    and uploads it; planner='device' uploads the T-bar table alone and builds the brick table
    with libfplplan.so on the kernel's stream: the same bytes.  Any other value, and
    planner='device' with device=None (the host loop plans nothing), is a ValueError."""
    from . import labels as _labels
    _labels.check_planner(planner, device)
    if device is not None:
        return _labels.write_labels_mask_device(tbars, roi_mask, radius_use, radius_ign,
                                                buffer_size, prefix, device, planner=planner)
    radius_use_flt = fplutils.set_filter(radius_use)
    if radius_ign is not None:
        radius_ign_flt = 1 - fplutils.set_filter(radius_ign)
    else:
        radius_ign = 0
    mask = np.copy(roi_mask)
    labels = np.zeros(mask.shape, dtype='uint8')
    for jj in range(tbars['locs'].shape[0]):
        xx, yy, zz = (int(v) for v in tbars['locs'][jj, :3])
        if radius_ign > 0:
            box = (slice(zz - radius_ign, zz + radius_ign + 1),
                   slice(yy - radius_ign, yy + radius_ign + 1),
                   slice(xx - radius_ign, xx + radius_ign + 1))
            mask[box] = np.logical_and(mask[box], radius_ign_flt)
        box = (slice(zz - radius_use, zz + radius_use + 1),
               slice(yy - radius_use, yy + radius_use + 1),
               slice(xx - radius_use, xx + radius_use + 1))
        mask[box] = np.logical_or(mask[box], radius_use_flt)
        labels[box] = np.logical_or(labels[box], radius_use_flt)
    for ax in range(3):
        sl = [slice(None)] * 3
        sl[ax] = slice(0, buffer_size); mask[tuple(sl)] = 0
        sl[ax] = slice(-buffer_size, None); mask[tuple(sl)] = 0
    if prefix is not None:
        from . import keras_io
        np.save('%s_labels.npy' % prefix, labels)
        np.save('%s_mask.npy' % prefix, mask)
        keras_io.write_main('%s_labels.h5' % prefix, labels)
        keras_io.write_main('%s_mask.h5' % prefix, mask)
    return labels, mask


def _multi_pred_labels(tbars_in, segm_name, labels):
    n = np.asarray(tbars_in['conf']).shape[0]
    if labels is not None:
        labels = np.asarray(labels).reshape(-1)
        if labels.shape[0] != n:
            raise ValueError('labels holds %d entries for %d points' % (labels.shape[0], n))
        return labels
    if segm_name:
        raise ValueError('segm_name=%r: reading labels from DVID is out of scope here; pass the '
                         "points' labels as an array, labels=" % (segm_name,))
    return np.zeros(np.asarray(tbars_in['conf']).shape)


def _multi_pred_dense(pos, conf, ll, neighbor_thresh):
    """the reference loop (:386-449), matrix included"""
    dists = np.sqrt((
        (pos.reshape((-1, 1, 3)) - pos.reshape((1, -1, 3))) ** 2).sum(
            axis=2))

    has_neighbor = np.sum((dists > 0) & (dists < neighbor_thresh),
                          axis=1)
    tt_idx = np.argsort(-conf)

    rm_idx = np.zeros(tt_idx.shape, 'bool')
    mv_idx = np.zeros(tt_idx.shape, 'bool')
    mv_loc = np.zeros(pos.shape, 'int')

    for ii in tt_idx:
        if rm_idx[ii]:
            continue
        if not has_neighbor[ii]:
            continue

        candidates = (
            (dists[ii, :] > 0) & (dists[ii, :] < neighbor_thresh) &
            (ll == ll[ii]) &
            (np.logical_not(rm_idx)))

        jj = np.nonzero(candidates)[0]

        if jj.size > 0:
            mv_idx[ii] = True

            old_loc = pos[ii, :]
            candidates[ii] = True
            while True:
                # new location by interpolation
                ww = conf * candidates
                ww = ww / np.sum(ww)

                mv_loc[ii, :] = np.round(
                    np.sum(ww.reshape((-1, 1)) * pos, axis=0))
                if np.array_equal(old_loc, mv_loc[ii, :]):
                    break

                old_loc = mv_loc[ii, :].copy()
                new_dists = np.sqrt(np.sum(
                    (pos - mv_loc[ii, :]) ** 2, axis=1))

                candidates = (
                    (new_dists < neighbor_thresh) &
                    (ll == ll[ii]) &
                    (np.logical_not(rm_idx)))

            jj = np.nonzero(candidates)[0]
            rm_idx[jj] = True

    rm_idx[mv_idx] = False

    return rm_idx, mv_idx, mv_loc


def _sparse_rows(pos, indptr, indices, neighbor_thresh):
    """the neighbour table, a superset (s <= T2), cut down to what the reference's own expression
    keeps -> (has_neighbor, indptr, indices)"""
    n = pos.shape[0]
    keep = np.zeros(len(indices), bool)
    owner = np.repeat(np.arange(n), np.diff(indptr))
    step = 1 << 20
    for a in range(0, len(indices), step):
        d = np.sqrt(((pos[owner[a:a + step]] - pos[indices[a:a + step]]) ** 2).sum(axis=1))
        keep[a:a + step] = (d > 0) & (d < neighbor_thresh)
    has_neighbor = np.bincount(owner[keep], minlength=n)
    indices = indices[keep]
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(has_neighbor, out=indptr[1:])
    return has_neighbor, indptr, indices


def _merge_visit(ii, row, pos, conf, ll, neighbor_thresh, grid, rm_idx, mv_idx, mv_loc, watch=None):
    """one visit of the reference loop: point `ii`, not removed, with the filtered row `row` of
    the neighbour table.  `watch`, if given, is called with the points of every ball that pass
    the distance and label tests, removed or not - the closure of dedupe.py listens there."""
    jj = row[(ll[row] == ll[ii]) & np.logical_not(rm_idx[row])]

    if jj.size > 0:
        mv_idx[ii] = True

        old_loc = pos[ii, :]
        at = np.searchsorted(jj, ii)
        cand = np.concatenate([jj[:at], [ii], jj[at:]])      # ascending, ii among them
        while True:
            # new location by interpolation, over the candidates alone, in index order
            if cand.size:
                ww = conf[cand]
                ww = ww / np.sum(ww)
                rows = ww.reshape((-1, 1)) * pos[cand]
                mean = rows[0]
                for r in rows[1:]:
                    mean = mean + r
            else:
                mean = np.full(3, np.nan)        # the reference's 0 / 0
            mv_loc[ii, :] = np.round(mean)
            if np.array_equal(old_loc, mv_loc[ii, :]):
                break

            old_loc = mv_loc[ii, :].copy()
            # a ball around the moved centre may hold points that are partners of no
            # candidate: asked of the grid, not of the table
            ball = grid.ball(mv_loc[ii, :])
            new_dists = np.sqrt(np.sum(
                (pos[ball] - mv_loc[ii, :]) ** 2, axis=1))
            near_same = (new_dists < neighbor_thresh) & (ll[ball] == ll[ii])
            if watch is not None:
                watch(ball[near_same])
            cand = ball[near_same & (np.logical_not(rm_idx[ball]))]

        rm_idx[cand] = True


def _multi_pred_sparse(pos, conf, ll, neighbor_thresh, device):
    """the same loop on the neighbour table of near.py and a host cell grid: no N x N object"""
    from . import near
    n = pos.shape[0]
    if n == 0:
        return np.zeros(0, 'bool'), np.zeros(0, 'bool'), np.zeros(pos.shape, 'int')
    if device is None:
        indptr, indices = near.pairs_numpy(pos, neighbor_thresh)
    else:
        indptr, indices = near.pairs_device(pos, neighbor_thresh, device)
    has_neighbor, indptr, indices = _sparse_rows(pos, indptr, indices, neighbor_thresh)
    grid = near.CellGrid(pos, neighbor_thresh)

    tt_idx = np.argsort(-conf)

    rm_idx = np.zeros(tt_idx.shape, 'bool')
    mv_idx = np.zeros(tt_idx.shape, 'bool')
    mv_loc = np.zeros(pos.shape, 'int')

    for ii in tt_idx[has_neighbor[tt_idx] > 0]:
        if rm_idx[ii]:
            continue
        _merge_visit(ii, indices[indptr[ii]:indptr[ii + 1]], pos, conf, ll, neighbor_thresh, grid,
                     rm_idx, mv_idx, mv_loc)

    rm_idx[mv_idx] = False

    return rm_idx, mv_idx, mv_loc


SOLVER_FORMS = ("solver='host' (default: the loop on the host, any method and device=) or "
                "solver='device' (with method='sparse' and device=<int> or True: the loop on the GPU)")


def rm_tbar_multi_pred(tbars_in, dvid_node=None, segm_name=None, neighbor_thresh=30, labels=None,
                       method='dense', device=None, solver='host', info=None):
    """Detections of one T-bar made twice, by two neighbouring substacks (reference :378-449).
    In order of falling confidence, a point that has not been removed gathers the points of
    its own segment closer than `neighbor_thresh`, moves to their confidence-weighted mean
    (rounded, and again from the points around the moved centre until it rests) and marks
    them for removal.  -> (rm_idx, mv_idx, mv_loc): bool (N,) removed, bool (N,) moved,
    'int' (N, 3) the new locations of the moved points; merge_multi_pred applies them.

    Labels: `labels`, an array of N segment ids, stands in for the reference's DVID query.
    Without it and with a falsy `segm_name` all labels are equal (the reference's np.zeros
    branch); a truthy `segm_name` without `labels` is a ValueError - DVID is out of scope.

    method='dense' (default) restates the reference loop, its N x N distance matrix included:
    it is the specification, quirks and all - coincident points are no neighbours at first but
    are candidates around a moved centre; has_neighbor ignores labels; a moved point is never
    removed.  The matrix is 8 N^2 bytes: 7 GB at 30 000 points.

    method='sparse' returns the same three arrays without any N x N object.  The first
    candidate set of a point is its row of the neighbour table (near.pairs_numpy, a superset
    filtered by the reference's own sqrt expression); the balls around moved centres are asked
    of a host cell grid (near.CellGrid) and filtered by the reference's expression; the
    weighted mean runs over the candidates alone in ascending index order, which is the order
    of the reference's axis-0 sum with its zero rows left out.
    One difference is known: the reference divides by np.sum(ww), a pairwise sum over all N
    entries whose last bit depends on where the candidates sit in the array.  The two methods
    are bit-equal whenever the sum of the candidates' confidences is exact in float64 - true
    of the float32-valued confidences voxel2obj returns from float32 predictions unless they
    span more than about 2^29 in magnitude.  Otherwise the divisor can differ in its last bit,
    which changes a result only where a mean coordinate lies within an ulp of a half-integer.

    device=<int> (or True, the runtime's default device), with method='sparse' only, takes the
    table from libfplnear.so (near.pairs_device: the same bytes); device=None builds it on the
    host.  No host fallback: a missing library raises.  Anything else is a ValueError.

    solver='host' (default) runs the loop itself on the host, as above.  solver='device', with
    method='sparse' and device= only, runs it on the GPU with libfplmerge.so (dedupe.merge_device):
    the table stays on the device, the loop runs per connected component of it, a lane each, and
    the components whose run met something it cannot reproduce exactly - a point of another
    component in a ball, more than 7 candidates, an empty candidate set, a point that does not
    come to rest, a large component - are run again on the host, in the global order.  The three
    arrays are those of method='sparse', bit for bit.  It asks for float64 confidences and
    float64 locations (integer locations up to 2^24 in magnitude are taken as float64, which is
    exact); anything else is a ValueError that names solver='host'.  A missing library raises
    FplMergeError before a missing GPU is reported; the host loop is never substituted.
    `info`, a dict, then receives `components`, `largest`, `sweeps`, `host_components`,
    `host_points` and `closure_rounds` (dedupe.py says what each counts)."""
    if method not in ('dense', 'sparse'):
        raise ValueError("method %r: 'dense' (the reference's matrix) or 'sparse'" % (method,))
    if device is not None and method != 'sparse':
        raise ValueError("device=%r needs method='sparse': the dense method is the host "
                         'specification' % (device,))
    if solver not in ('host', 'device'):
        raise ValueError('solver %r: %s' % (solver, SOLVER_FORMS))
    if solver == 'device' and (method != 'sparse' or device is None):
        raise ValueError("solver='device' with method=%r, device=%r: %s"
                         % (method, device, SOLVER_FORMS))
    ll = _multi_pred_labels(tbars_in, segm_name, labels)
    pos, conf = tbars_in['locs'], tbars_in['conf']
    if solver == 'device':
        from . import dedupe
        return dedupe.merge_device(pos, conf, ll, neighbor_thresh, device, info=info)
    if method == 'dense':
        return _multi_pred_dense(pos, conf, ll, neighbor_thresh)
    return _multi_pred_sparse(pos, conf, ll, neighbor_thresh, device)


def merge_multi_pred(tbars, rm_idx, mv_idx, mv_loc):
    """the point list after rm_tbar_multi_pred: moved points take their `mv_loc`, removed
    points are dropped, the order is otherwise kept.  -> a new {'locs', 'conf'} of the input's
    dtypes"""
    rm_idx, mv_idx = np.asarray(rm_idx, bool), np.asarray(mv_idx, bool)
    locs = np.array(tbars['locs'], copy=True)
    locs[mv_idx] = np.asarray(mv_loc)[mv_idx]
    keep = np.logical_not(rm_idx)
    return {'locs': locs[keep], 'conf': np.asarray(tbars['conf'])[keep]}


# ---- training-data export (reference :140-249), on arrays ---------------------------------------------

def _annotations(dvid_annotations):
    """{'locs' (N, 3) global (x, y, z), 'conf' (N,)} of a point dict or of anything
    load_from_json reads"""
    tt = dvid_annotations if isinstance(dvid_annotations, dict) else load_from_json(dvid_annotations)
    locs, conf = np.asarray(tt['locs']), np.asarray(tt['conf'])
    return {'locs': locs.reshape(-1, 3) if locs.size == 0 else locs, 'conf': conf.reshape(-1)}


def get_substack_annotations(annotations, roi, ss, device=None):
    """the annotations inside the substack `ss` and inside the ROI (reference :236-249).
    `annotations`: a {'locs', 'conf'} dict in global (x, y, z), or anything load_from_json reads.
    Kept are the points with ss.x <= x < ss.x + ss.size, and likewise for y and z - the box
    DVID's elements/<size>/<offset> answers - and of those the points `roi.ptquery` accepts at
    np.fliplr(locs).astype('int'), as the reference asks roi_ptquery; roi=None filters by the
    box alone.  `device` is roi.ptquery's.  -> a new {'locs', 'conf'}"""
    tt = _annotations(annotations)
    locs, conf = tt['locs'], tt['conf']
    lo = np.asarray([ss.x, ss.y, ss.z])
    keep = np.all((locs >= lo) & (locs < lo + ss.size), axis=1) if len(locs) else np.zeros(0, bool)
    locs, conf = locs[keep], conf[keep]
    if roi is not None and conf.size > 0:
        in_roi = roi.ptquery(np.fliplr(locs).astype('int'), device=device)
        locs, conf = locs[in_roi], conf[in_roi]
    return {'locs': locs, 'conf': conf}


def _substacks_of(dvid_roi, partition_size, roi):
    """(substacks, BlockRoi) of roi_to_substacks' `dvid_roi` and `roi=`"""
    from . import fplpipeline
    from .roi import BlockRoi
    if isinstance(dvid_roi, str) and os.path.isfile(dvid_roi):
        with open(dvid_roi) as f_in:
            is_json = f_in.read(64).lstrip().startswith('[')
        if not is_json:
            if not isinstance(roi, BlockRoi):
                raise ValueError('dvid_roi %r lists substacks and holds no ROI to mask or filter by: '
                                 'pass the BlockRoi as roi=' % (dvid_roi,))
            print('reading roi %s from file' % dvid_roi)
            return fplpipeline.roi_from_txt(dvid_roi)[0], roi
        dvid_roi = BlockRoi.from_json(dvid_roi)
    if not isinstance(dvid_roi, BlockRoi):
        raise ValueError('dvid_roi is a BlockRoi, the path of its JSON or a substack text file, got %r'
                         % (dvid_roi,))
    if roi is not None:
        raise ValueError('roi= goes with a substack text file; dvid_roi is an ROI already')
    return dvid_roi.partition(partition_size)[0], dvid_roi


def _write_volume(base, arr):
    from . import keras_io
    keras_io.write_main(base + '.h5', arr)
    np.save(base + '.npy', arr)


def roi_to_substacks(dvid_server, dvid_uuid, dvid_roi, dvid_annotations, partition_size,
                     data_dir=None, substack_ids=None, image_normalize=None, buffer_size=None,
                     radius_use=None, radius_ign=None, seg_name=None, device=None, roi=None):
    """Training substacks of an ROI (reference :140-233), on arrays instead of a DVID node.  The
    parameter order is the reference's; the parameters mean:

      dvid_server       the grayscale: whatever fplpipeline's sources accept - a uint8 (Z, Y, X)
                        array or memmap, 'npy://file', a resident uint8 tensor / DeviceBuffer
      dvid_uuid         ignored
      dvid_roi          a roi.BlockRoi or the path of its JSON: the substacks are its
                        partition(partition_size); or a substack text file (roi_from_txt): the
                        substacks are the file's, and the ROI to mask and filter by comes as
                        `roi=` (without it: ValueError)
      dvid_annotations  a {'locs', 'conf'} dict in global (x, y, z), or anything load_from_json reads
      seg_name          a label volume with the image's extents (array, 'npy://file', resident), or None

    substack_ids=None prints the reference's statistics, '%03d\\t%.03f\\t%3d' of index, fraction of
    the cube inside the ROI (from BlockRoi.voxel_counts: nothing is rendered) and annotations in
    cube and ROI, and returns the rows [(index, fraction, count)] (the reference returns None).

    Otherwise, for each id: the cube with `buffer_size` voxels around it, zeros outside the
    volume, as float32 (v - image_normalize[0]) / image_normalize[1] with both rounded to
    float32; the annotations in the cube's local coordinates; the ROI mask; write_labels_mask;
    the segmentation cube (uint64) if asked for.  With `data_dir` they are written under the
    reference's names - '%03d_im%g_%g_bf%d', '%03d_bf%d_synapses.json', '%03d_bf%d_roimask',
    '%03d_ru%d_ri%d_bf%d_{labels,mask}', '%03d_seg_bf%d' - each volume as '.h5' (dataset 'main',
    uncompressed: the reference gzips) and as '.npy' beside it.  -> a list of dicts, one per id:
    id, substack, image, tbars, roi_mask, labels, mask, seg (None without seg_name).

    device=None is numpy throughout.  device=<int> (or True) uploads the grayscale once (or
    takes it resident), cuts and normalises with libfplroi.so, renders the mask there, filters
    the annotations there, calls write_labels_mask(device=) on the resident mask and cuts a
    resident segmentation through libfplseg.so (int64 tensor holding the uint64 bits; a host
    segmentation is cut on the host): image, roi_mask, labels and mask are resident torch
    tensors, equal to the host's arrays bit for bit, and each file is written from one download.
    No host fallback: a missing library raises."""
    from . import fplpipeline
    subs, roi = _substacks_of(dvid_roi, partition_size, roi)
    tbars_all = _annotations(dvid_annotations)
    if substack_ids is None:
        boxes = np.asarray([(ss.z, ss.y, ss.x, ss.size, ss.size, ss.size) for ss in subs],
                           np.int64).reshape(-1, 6)
        counts = roi.voxel_counts(boxes, device=device)
        rows = []
        for ii, ss in enumerate(subs):
            frac_in = int(counts[ii]) / float(ss.size ** 3)
            tt = get_substack_annotations(tbars_all, roi, ss, device=device)
            print('%03d\t%.03f\t%3d' % (ii, frac_in, tt['conf'].size))
            rows.append((ii, frac_in, int(tt['conf'].size)))
        return rows

    if not hasattr(substack_ids, '__len__'):
        substack_ids = [substack_ids, ]
    src = fplpipeline._open_source(dvid_server)
    seg_src = None if seg_name is None else fplpipeline._open_label_source(seg_name)
    mean, std = np.float32(image_normalize[0]), np.float32(image_normalize[1])
    dev = gray = None
    if device is not None:
        from . import roi as _roi
        dev = _roi.torch_device(device)
        gray = _resident_gray(src, dev)
    out = []
    for ii in substack_ids:
        print(ii)
        ss = subs[ii]
        image_sz = ss.size + 2 * buffer_size
        image_offset = [ss.z - buffer_size, ss.y - buffer_size, ss.x - buffer_size]
        dims = [image_sz] * 3

        # the image with its buffer
        if dev is None or gray is None:
            cube = src.cube_host(image_offset, image_sz)
            if cube is None:
                cube = np.zeros(dims, np.uint8)
        if dev is None:
            image = (cube.astype('float32') - mean) / std
        elif gray is None:                    # a generated source: the cube goes up, not the volume
            import torch
            image = _roi.cut_normalize_device(torch.from_numpy(cube).to(dev), dims, (0, 0, 0), dims,
                                              mean, std, dev)
        else:
            image = _roi.cut_normalize_device(gray, src.extent, image_offset, dims, mean, std, dev)

        # the annotations, in local coordinates
        tt = get_substack_annotations(tbars_all, roi, ss, device=device)
        if tt['conf'].size > 0:
            tt['locs'] = tt['locs'] - np.fliplr(np.asarray([image_offset]))

        # labels and mask, with the ROI and the buffer
        mask = roi.roi3D(dims, image_offset, device=device)
        prefix = None
        if data_dir is not None:
            _write_volume('%s/%03d_im%g_%g_bf%d' % (data_dir, ii, image_normalize[0],
                                                    image_normalize[1], buffer_size),
                          image if dev is None else image.cpu().numpy())
            tbars_to_json_format_raveler(tt, '%s/%03d_bf%d_synapses.json' % (data_dir, ii, buffer_size))
            _write_volume('%s/%03d_bf%d_roimask' % (data_dir, ii, buffer_size),
                          mask if dev is None else mask.cpu().numpy())
            prefix = '%s/%03d_ru%d_ri%d_bf%d' % (data_dir, ii, radius_use, radius_ign, buffer_size)
        labels, lmask = write_labels_mask(tt, mask, radius_use, radius_ign, buffer_size, prefix,
                                          device=device)

        # the segmentation
        seg = None
        if seg_src is not None:
            seg = _seg_cube(seg_src, image_offset, image_sz, dev)
            if data_dir is not None:
                _write_volume('%s/%03d_seg_bf%d' % (data_dir, ii, buffer_size),
                              seg if isinstance(seg, np.ndarray) else seg.cpu().numpy().view(np.uint64))
        out.append({'id': ii, 'substack': ss, 'image': image, 'tbars': tt, 'roi_mask': mask,
                    'labels': labels, 'mask': lmask, 'seg': seg})
    return out


def _resident_gray(src, dev):
    """the grayscale of `src` on `dev`: a resident source as it is, a host uint8 array uploaded
    once, None for a source that generates its cubes"""
    from . import fplpipeline
    import torch
    if isinstance(src, fplpipeline._DeviceSource):
        if src.device != (dev.index or 0):
            raise ValueError('the grayscale lives on GPU %d, device= names %s' % (src.device, dev))
        return src.vol
    if isinstance(src, fplpipeline._ArraySource):
        if np.dtype(src.arr.dtype) != np.uint8:
            raise ValueError('roi_to_substacks(device=) takes uint8 grayscale, not %s' % src.arr.dtype)
        return torch.from_numpy(np.array(src.arr, np.uint8, order='C')).to(dev)
    return None


def _seg_cube(seg_src, origin, size, dev):
    """the uint64 (size,)*3 cube of the label source at `origin`, zeros outside the volume: a host
    source on the host; a resident one through libfplseg.so, as an int64 tensor of the same bits"""
    from . import fplpipeline
    if isinstance(seg_src, fplpipeline._DeviceLabelSource):
        from . import _segcapi
        import torch
        where = torch.device('cuda', seg_src.device)
        if dev is not None and where != dev:
            raise ValueError('the segmentation lives on %s, device= names %s' % (where, dev))
        dst = torch.empty((size,) * 3, dtype=torch.int64, device=where)
        with torch.cuda.device(where):
            _segcapi.pad_box(seg_src.vol, origin, (size,) * 3, 0, dst,
                             torch.cuda.current_stream(where).cuda_stream)
        return dst
    cube = seg_src.cube_host(origin, size, np.uint64)
    return np.zeros((size,) * 3, np.uint64) if cube is None else cube
