"""The rule the threshold sweep scored with the ARKitScenes detection mAP rests on (box2mask_amd/param_search.py:
detection_tables / detection_records / arkit_param_search), restated in numpy on top of tests/_sweep_rule.py and
tests/_detbox_rule.py, for tests/test_det_sweep_rule.py (CPU) and tests/test_gpu_arkit_sweep.py.

Facts 1 and 2 of _sweep_rule.py carry over unchanged (a prefix per score_th; the mask NMS of a prefix is the restriction of the NMS
of the whole list).  Instead of fact 3:

  3'. Evaluater.arkitscenes_eval (/root/reference/models/evaluation.py:245-316) scores a kept row by the prism of its POINTS -- the
      point count (:280, rows under 50 points are skipped AFTER the mask NMS has run), the z range and the convex hull in x-y
      (:284-292) -- and the IoU of that prism with every ground-truth box of the row's class (eval_det looks at no other pair).
      Point p lies in row r iff bit vox2point[p] of voxel mask r is set, so all of it depends on (cluster_th, mask_bin_th) alone:
      score_th and mask_nms_th only select rows.

``stage_tables`` computes, per scene, what the settings share as ``param_search.DetectionTables``: the voxel masks of
``_sweep_rule.shared_tables`` expanded through vox2point, ``_detbox_rule.hulls_rule`` per row, ``corners_rule`` per ground-truth box
and form (a) of ``iou_forms`` (or ``aabb_rule``) per same-class pair.  ``rows`` composes a setting and applies the gate;
``eval_det`` restates the matching and the VOC AP.  ``mistake=`` states one deliberate MISTAKE as a variant of the rule; the test
shows that the fixture catches each.

The fixture (tests/golden/arkit_sweep.npz, tools/gen_golden_arkit_sweep.py) holds, for the 36 settings of param_sweep.npz and one
case off the grid, what the reference's own code returned; its inputs are those of param_sweep.npz plus ``scene_positions``.
"""
import hashlib
import math

import numpy as np

import _detbox_rule as D
import _nms_rule as R
import _sweep_rule as W
from box2mask_amd import param_search, synth

MISTAKES = ('count_on_voxels', 'gt_min_points', 'iou_of_other_stage', 'rotation_not_transposed', 'no_class_gate', 'gate_before_nms')
MIN_POINTS = 50                                 # evaluation.py:280
POSITION_NOISE = 0.002
SEED = 11
VARIANTS = (('obb', True), ('aabb', False))
THRESHOLDS = (0.5, 0.25)


def scene_positions(seed):
    """(n_pts, 3) float64: the points vox2point indexes -- synth.make_scene(seed, 12000 voxels, points_only) -- with 2 mm of seeded
    noise.  The synthetic furniture has exactly planar faces: a mask that covers one vertical face is a LINE in x-y, on which the
    reference's scipy ConvexHull raises QhullError, so such a setting would have no reference result at all.  The noise enters the
    hulls only: voxels, vox2point and masks are those of param_sweep.npz."""
    raw = synth.make_scene(seed, target_voxels=12000, pts_per_m2=6000.0, points_only=True)
    p = np.asarray(raw['positions'], np.float64)
    return p + np.random.default_rng(9000 + seed).normal(0.0, POSITION_NOISE, p.shape)


def positions_checksum(pos):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(pos, np.float64).tobytes()).digest(), np.uint8).copy()


def fixture_labels(ak, si):
    return {k: ak['ak_s%d_%s' % (si, k)] for k in ('per_instance_bb_centers', 'per_instance_bb_bounds', 'per_instance_bb_rotations',
                                                   'per_instance_semantics')}


def fixture_inputs(sw, ak, gate=False):
    """Per scene (scene of _sweep_rule.fixture_scenes, positions, labels); the positions are checked against the fixture's sum.
    gate=True: the case off the grid -- scene 0 without the points ``ak_gate_dropped_points``."""
    out = []
    for si, scene in enumerate(W.fixture_scenes(sw)):
        pos = scene_positions(SEED + si)
        assert len(pos) == int(ak['ak_s%d_n_pts' % si]) and np.array_equal(positions_checksum(pos), ak['ak_s%d_pos_sha256' % si])
        if gate and si == 0:
            sel = np.setdiff1d(np.arange(len(pos)), ak['ak_gate_dropped_points'])
            scene = dict(scene, vox2point=np.asarray(scene['vox2point'])[sel], gt_ids=np.asarray(scene['gt_ids'])[sel])
            pos = pos[sel]
        out.append((scene, pos, fixture_labels(ak, si)))
    return out


def gt_tables(labels, mistake=None):
    """evaluation.py:257-270: label (g,), boxes (g, OBB_REC) = the corner records of _detbox_rule.corners_rule, centers (g, 3)."""
    centers = np.asarray(labels['per_instance_bb_centers'], np.float64).reshape(-1, 3)
    bounds = np.asarray(labels['per_instance_bb_bounds'], np.float64).reshape(-1, 3)
    rot = np.asarray(labels['per_instance_bb_rotations'], np.float64).reshape(-1, 9)
    if mistake == 'rotation_not_transposed':                                # :261 reshapes AND transposes
        rot = rot.reshape(-1, 3, 3).transpose(0, 2, 1).reshape(-1, 9)
    return dict(label=np.asarray(labels['per_instance_semantics']).astype(np.int32)[:len(centers)], centers=centers,
                boxes=D.corners_rule(centers, bounds, rot))


def row_ious(hulls, gt, pcls, oriented, mistake=None):
    """(K, g): box3d_iou (form (a) of iou_forms: fp64 as the reference evaluates it) or calc_iou where the classes agree."""
    k, g = len(pcls), len(gt['label'])
    gcls = gt['label']
    if mistake == 'no_class_gate':
        same = np.broadcast_to((np.asarray(pcls) >= 0)[:, None], (k, g))
    else:
        same = (np.asarray(pcls)[:, None] == gcls[None, :]) & (np.asarray(pcls) >= 0)[:, None]
    if not oriented:
        out = np.zeros((k, g))
        for r, b in zip(*np.nonzero(same)):                                 # (aabb_rule has its own class gate: one pair at a time)
            out[r, b] = D.aabb_rule(hulls['box6'][r:r + 1], np.zeros(1, np.int32), gt['centers'][b:b + 1], gt['boxes'][b:b + 1],
                                    np.zeros(1, np.int32))[0, 0]
        return out
    out = np.zeros((k, g))
    for r, b in zip(*np.nonzero(same)):
        h, rec = hulls['hulls'][r], gt['boxes'][b]
        if h is None or len(h) < 3:
            continue
        out[r, b] = D.iou_forms(h, hulls['box6'][r, 2], hulls['box6'][r, 5], rec[0:8].reshape(4, 2), rec[8], rec[9], rec[10])['iou_a']
    return out


def stage_tables(scene, pos, labels, grid, oriented=True, min_points=MIN_POINTS, mistake=None):
    """(DetectionTables, aux): aux[ci][bi] = dict(vmask (K', n_vox) bool, pmask (K', n_pts) bool) for the mistakes that need them."""
    t, point_masks = W.shared_tables(scene, grid)
    gt = gt_tables(labels, mistake)
    v2p = np.asarray(scene['vox2point'], np.int64)
    n_vox = len(scene['seg2vox'])
    first = np.full(n_vox, -1, np.int64)
    first[v2p[::-1]] = np.arange(len(v2p))[::-1]                            # a point of every voxel
    assert len(pos) == len(v2p)
    out = param_search.DetectionTables(scene['name'], len(v2p), gt['label'], min_points)
    out.clusters = t.clusters
    aux = []
    for ci in range(len(t.clusters)):
        stages, ax = [], []
        for bi, st in enumerate(t.stages[ci]):
            pm = np.asarray(point_masks[ci][bi]) != 0                       # step 1: the voxel masks through vox2point
            vm = np.zeros((len(pm), n_vox), bool)
            vm[:, first >= 0] = pm[:, first[first >= 0]]
            hulls = D.hulls_rule(pm, pos, 1 << 24)                          # step 2: count, box6 and hull per row
            assert (hulls['flags'] == 0).all()
            count = (vm.sum(1) if mistake == 'count_on_voxels' else hulls['count']).astype(np.int64)
            big = (count > min_points) if mistake == 'gt_min_points' else (count >= min_points)
            pcls = np.where(big, st['label_id'], -1).astype(np.int32)
            stages.append(dict(label_id=st['label_id'], keep=st['keep'], count=count, iou=row_ious(hulls, gt, pcls, oriented, mistake),
                               big=big))
            ax.append(dict(vmask=vm, pmask=pm))
        if mistake == 'iou_of_other_stage':
            ious = [s['iou'] for s in stages]
            for bi, s in enumerate(stages):
                s['iou'] = ious[(bi + 1) % len(stages)]
        out.stages.append(stages)
        aux.append(ax)
    return out, aux


def rows(tables, aux, grid, ci, si, bi, mi, mistake=None):
    """Steps 3 and 4: the rows of setting (ci, si, bi, mi) that are scored, in prediction order."""
    st = tables.stages[ci][bi]
    if mistake == 'gate_before_nms':                                        # the small rows leave first and suppress nothing
        k_s = int(tables.clusters[ci]['ks'][si])
        big = np.nonzero(st['big'][:k_s])[0]
        keep = R.mask_nms(R.pack(aux[ci][bi]['vmask'][big]), grid.mask_nms_th[mi])[1] if len(big) else np.zeros(0)
        return big[np.asarray(keep).reshape(-1) != 0].astype(np.int64)
    kept = W.compose(tables, ci, si, bi, mi)
    return kept[st['big'][kept]]


def records(tables, aux, grid, ci, si, bi, mi, mistake=None):
    st = tables.stages[ci][bi]
    r = rows(tables, aux, grid, ci, si, bi, mi, mistake)
    return {'label': st['label_id'][r], 'conf': tables.clusters[ci]['conf'][r], 'gt_label': tables.gt_label, 'iou': st['iou'][r]}


# ------------------------------------------------------------------ step 5: eval_det restated
def voc_ap(rec, prec):
    """evaluate_detections.py:28-59, the all-points form: the area under the precision envelope."""
    mrec, mpre = [0.0] + list(rec) + [1.0], [0.0] + list(prec) + [0.0]
    for i in range(len(mpre) - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    return float(np.sum([(mrec[i + 1] - mrec[i]) * mpre[i + 1] for i in range(len(mrec) - 1) if mrec[i + 1] != mrec[i]]))


def eval_det(recs, ovthresh):
    """{class id: AP} in the reference's class order.  recs: {scene: record} in scene order.

    evaluate_detections.py:187-207  the classes in order of first appearance: predictions scene by scene, then ground truths;
    :212-219   a class without any prediction raises KeyError (pred[classname]) and gets no entry;
    :97-101    npos = the ground truths of the class over all scenes, each with a `det` flag;
    :121       detections of all scenes by descending confidence (no two equal in the fixture);
    :136-145   per detection the FIRST maximum of the IoU over the ground truths of its scene and class (`iou > ovmax`);
    :147-154   `ovmax > ovthresh`: true positive if that ground truth is free, else (or below the threshold) false positive;
    :157-163   cumulative sums, rec = tp / npos (nan for npos = 0: evaluation.py:314 leaves it out), prec, voc_ap."""
    order = []
    for r in recs.values():
        order += [int(c) for c in r['label'] if int(c) not in order]
    with_pred = list(order)
    for r in recs.values():
        order += [int(c) for c in r['gt_label'] if int(c) not in order]
    ap = {}
    for c in order:
        if c not in with_pred:
            continue
        dets, free, npos = [], {}, 0
        for name, r in recs.items():
            gsel = [j for j, g in enumerate(r['gt_label']) if int(g) == c]
            npos += len(gsel)
            free[name] = [True] * len(gsel)
            dets += [(float(r['conf'][i]), name, [float(r['iou'][i][j]) for j in gsel]) for i, l in enumerate(r['label']) if int(l) == c]
        dets = [dets[i] for i in np.argsort(-np.array([d[0] for d in dets]))]
        tp, fp = [], []
        for _, name, ious in dets:
            best, jmax = -math.inf, -1
            for j, v in enumerate(ious):
                if v > best:
                    best, jmax = v, j
            hit = best > ovthresh and free[name][jmax]
            if hit:
                free[name][jmax] = False
            tp.append(1.0 if hit else 0.0); fp.append(0.0 if hit else 1.0)
        tp, fp = np.cumsum(tp), np.cumsum(fp)
        with np.errstate(divide='ignore', invalid='ignore'):
            rec = tp / float(npos)
        prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
        ap[c] = voc_ap(rec, prec) if npos else math.nan
    return ap


def mean_ap(ap):
    """evaluation.py:314."""
    vals = [v for v in ap.values() if not math.isnan(v)]
    return float(np.mean(np.array(vals))) if vals else math.nan


def same_floats(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a, b, equal_nan=True)


def check_setting(ak, tag, recs, vt, counts=None):
    """One setting's records against the fixture: scored rows and counts exact, IoU within IOU_TOL, per-class AP and mAP bit for
    bit at both thresholds.  Raises AssertionError naming what differs.  counts: per scene the point counts of the KEPT rows."""
    for s, (name, r) in enumerate(recs.items()):
        pre = 'ak_%s_s%d_' % (tag, s)
        want = ak[pre + 'iou_' + vt]
        if counts is not None:
            assert np.array_equal(counts[s], ak[pre + 'count']), (tag, s, 'count')
        assert np.asarray(r['iou']).shape == want.shape, (tag, s, 'scored rows', np.asarray(r['iou']).shape, want.shape)
        assert want.size == 0 or np.abs(np.asarray(r['iou']) - want).max() <= D.IOU_TOL, (tag, s, 'iou')
    for t in THRESHOLDS:
        key = 'ak_%s_%s_%d_' % (tag, vt, round(t * 100))
        ap = eval_det(recs, t)
        assert [int(c) for c in ap] == ak[key + 'classes'].tolist(), (tag, key, 'classes')
        assert same_floats([ap[c] for c in ap], ak[key + 'ap']), (tag, key, 'ap')
        assert same_floats(mean_ap(ap), ak[key + 'map']), (tag, key, 'map')
