"""S3DIS instance-segmentation metric (mPrec / mRec, and the mCov / mWCov / mIoU half the reference computes and drops).

Mirrors ``Evaluater.s3dis_eval`` (/root/reference/models/evaluation.py:124-241) and utils/s3dis_util.py:
``clustering_for_background`` (:146-177), ``assign_semantics_to_proposals`` (:137-144) and ``s3dis_eval`` (:179-338).  The
expensive parts of the reference -- sklearn's DBSCAN over every predicted wall point, a Python loop over every point of every
room and one full-length boolean ``&`` / ``|`` per (prediction, ground truth) pair -- are ``b2m_dbscan``,
``b2m_paint_proposals`` and ``b2m_joint_hist`` (include/b2m.h, csrc/cluster.hip); the metric over the resulting tables walks a few
hundred records per room and stays on the host (``s3dis_eval_from_counts``).

Full resolution (``cfg.full_resolution``, evaluation.py:151-154 and :213-222): the labels predicted on the sampled room are carried
to every point of the unsampled room through ``sparse2dense`` -- the nearest sampled point, box2mask_amd.neighbors -- and scored
against the full room's ground truth.  The caller hands the unsampled rooms to ``evaluate_rooms(..., full_rooms=...)``; the
reference reads them through its dataset module.

Deviations from the reference, both where it raises: ``dbscan`` of zero rows returns zero labels (sklearn raises), and an empty
proposal mask gets semantic class 0 (``np.bincount([]).argmax()`` raises).  Among sampled points at exactly the same distance
``sparse2dense`` takes the lowest row.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import B2MError, ptr
from .eval_detection import pack_masks

NUM_CLASSES = 13                     # s3dis_util.py:17
WALL_EPS, WALL_MIN_SAMPLES = 0.35, 10    # s3dis_util.py:164
WALL_MIN_POINTS = 3000               # s3dis_util.py:170
SEM_MIN, KEEP_RATIO, MIN_POINTS = 3, 0.6, 200   # evaluation.py:181, 187, 190 (and :203)
IOU_TH = 0.5                         # s3dis_util.py:195
JOINT_HIST_MAX = 1 << 24             # B2M_JOINT_HIST_MAX
DBSCAN_MIN_D, DBSCAN_MAX_D = 3, 8


def _dev():
    _lib.require_gpu()
    return torch.device('cuda', torch.cuda.current_device())


def _i32(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a).to(dev).to(torch.int32).contiguous()


def _f64(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a).to(dev).double().contiguous()


def dbscan(x, eps, min_samples, return_count=False):
    """Labels of sklearn's ``DBSCAN(eps=eps, min_samples=min_samples).fit(x).labels_`` for x (n, d), 3 <= d <= 8: int32 (n) on
    the device (b2m_dbscan).  return_count: also the number of clusters (device int32 scalar)."""
    dev = _dev()
    x = _f64(x, dev)
    assert x.dim() == 2, 'x must be (n, d)'
    n, d = x.shape
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    size = _lib.load().b2m_dbscan_workspace(n)
    if size < 0:
        raise B2MError('b2m_dbscan: %d rows are out of range' % n)
    work = torch.empty((size + 7) // 8, dtype=torch.int64, device=dev)
    _lib.call('b2m_dbscan', ptr(x), n, d, float(eps), int(min_samples), ptr(work), ptr(labels), ptr(count))
    return (labels, count) if return_count else labels


def joint_hist(a, b, na, nb=1):
    """(na, nb) int32 table of the pairs (a[p], b[p]); b None = a plain bincount of a.  Out-of-range rows are skipped."""
    dev = a.device
    assert a.is_cuda and a.dtype == torch.int32 and a.dim() == 1 and a.is_contiguous(), 'a: contiguous int32 (n) on the device'
    assert b is None or (b.device == dev and b.dtype == torch.int32 and b.shape == a.shape and b.is_contiguous()), \
        'b: contiguous int32 (n) on the device of a'
    assert na >= 1 and nb >= 1
    hist = torch.empty((na, nb), dtype=torch.int32, device=dev)
    _lib.call('b2m_joint_hist', ptr(a), ptr(b) if b is not None else None, a.shape[0], na, nb, ptr(hist))
    return hist


def clustering_for_background(pred_semantics, coords, normals):
    """s3dis_util.py:146-177: ceiling -> instance 1, floor -> 2, the wall points clustered on [coords, 2 * normals] -> 4 + cluster
    (noise 3), wall instances under 3000 points -> -1, everything else 0.  int32 (n) on the device.  Without a wall point the
    wall part is skipped (sklearn raises on an empty input)."""
    dev = _dev()
    sem = _i32(pred_semantics, dev)
    inst = torch.zeros_like(sem)
    inst[sem == 0] = 1
    inst[sem == 1] = 2
    wall = torch.nonzero(sem == 2).reshape(-1)
    if wall.numel() == 0:
        return inst
    feats = torch.cat([_f64(coords, dev)[wall], _f64(normals, dev)[wall] * 2.0], 1).contiguous()
    labels, count = dbscan(feats, WALL_EPS, WALL_MIN_SAMPLES, return_count=True)
    ncl = int(count.item())
    slot = (labels + 1).contiguous()                                 # 0 = noise, 1 + cluster
    sizes = joint_hist(slot, None, ncl + 1)[:, 0]
    small = sizes[slot.long()] < WALL_MIN_POINTS
    inst[wall] = torch.where(small, torch.full_like(labels, -1), labels + 4)
    return inst


def assign_semantics_to_proposals(pred_semantics, masks, bits=None):
    """s3dis_util.py:137-144: the most frequent class among the points of each mask (lowest class on ties; 0 for an empty mask,
    where the reference raises).  int32 (K) on the device."""
    dev = _dev()
    sem = _i32(pred_semantics, dev)
    bits, words, n = bits if bits is not None else pack_masks(masks, dev)
    k = bits.shape[0]
    out = torch.empty(k, dtype=torch.int32, device=dev)
    _lib.call('b2m_label_hist', ptr(bits), words, None, k, ptr(sem), n, NUM_CLASSES, ptr(out))
    return out


def paint_proposals(bits, words, n, proposal_semantics, semantics):
    """evaluation.py:177-193 over bit rows: (inst int32 (n), rewritten semantics int32 (n), accepted int32 (K)), all on the device."""
    dev = bits.device
    k = bits.shape[0]
    inst = torch.empty(n, dtype=torch.int32, device=dev)
    sem_out = semantics.clone()
    accepted = torch.zeros(max(k, 1), dtype=torch.int32, device=dev)
    unlabeled = torch.empty(max(words, 1), dtype=torch.int64, device=dev)
    _lib.call('b2m_paint_proposals', ptr(bits), words, k, ptr(proposal_semantics), n, SEM_MIN, KEEP_RATIO, MIN_POINTS,
              ptr(unlabeled), ptr(inst), ptr(sem_out), ptr(accepted))
    return inst, sem_out, accepted[:k]


def room_labels(pred_semantics, positions, normals, masks, details=False):
    """evaluation.py:163-212 for one room: {'semantics', 'instances'} (int32 (n), device) as the reference leaves ``pred_label``.
    The proposals repaint the semantics they are accepted over (evaluation.py:193 writes through the array ``pred_label`` holds);
    the background clustering and the vote of the proposals read the semantics as predicted.  masks: (K, n) bool / bytes in
    score order, as ``Model.pred2mask(..., 'eval')`` returns them."""
    dev = _dev()
    sem = _i32(pred_semantics, dev)
    n = sem.shape[0]
    if n == 0:
        raise ValueError('room_labels: a room without points')
    background = clustering_for_background(sem, positions, normals)
    packed = pack_masks(masks, dev) if torch.as_tensor(masks).shape[0] else (torch.empty((0, 1), dtype=torch.int64, device=dev),
                                                                           (n + 63) // 64, n)
    assert packed[2] == n, 'masks over %d points for %d semantics' % (packed[2], n)
    prop_sem = assign_semantics_to_proposals(sem, None, bits=packed)
    inst, sem_out, accepted = paint_proposals(packed[0], packed[1], n, prop_sem, sem)
    # evaluation.py:197-199 (with no accepted proposal the maximum is -1 and the ceiling's id 1 drops to 0, as there)
    max_id = inst.max()
    background = torch.where(background > 0, background + max_id, background)
    inst = torch.where(background > 0, background, inst)
    # evaluation.py:200-210: per class, the instances with fewer than 200 points of that class lose those points
    top = int(inst.max().item()) + 1
    if top > 0:
        if top * NUM_CLASSES > JOINT_HIST_MAX:
            raise B2MError('room_labels: %d instance ids exceed the joint table (%d entries)' % (top, JOINT_HIST_MAX))
        per_class = joint_hist(inst.contiguous(), sem_out, top, NUM_CLASSES)
        seen = (inst >= 0) & (sem_out >= 0) & (sem_out < NUM_CLASSES)
        flat = (inst.long().clamp(min=0) * NUM_CLASSES + sem_out.long().clamp(0, NUM_CLASSES - 1))
        small = seen & (per_class.reshape(-1)[flat] < MIN_POINTS)
        inst = torch.where(small, torch.full_like(inst, -1), inst)
    out = {'semantics': sem_out, 'instances': inst.contiguous()}
    if details:
        out.update(background=background, proposal_semantics=prop_sem, accepted=accepted)
    return out


def _dense(ids, skip=None):
    """Distinct values of an id column in ascending order (np.unique) and the dense index of every row; rows equal to `skip` get -1
    and `skip` is left out of the values."""
    vals, inv = torch.unique(ids, sorted=True, return_inverse=True)
    inv = inv.to(torch.int32)
    if skip is not None and vals.numel() and bool((vals == skip).any()):
        at = int(torch.nonzero(vals == skip)[0, 0].item())
        inv = torch.where(inv == at, torch.full_like(inv, -1), inv - (inv > at).to(torch.int32))
        vals = torch.cat([vals[:at], vals[at + 1:]])
    return vals, inv.contiguous()


def s3dis_counts(pred_label, gt_label):
    """The device half of s3dis_util.s3dis_eval for one room -> host tables: ``pred_class`` (P) / ``gt_class`` (G), the most frequent
    semantic class of every predicted (id -1 left out) / ground-truth instance in ascending id order (lowest class on ties, as
    scipy.stats.mode), ``inter`` (P, G) common points, ``pred_size`` / ``gt_size``, ``cc`` (13, 13) points by (predicted, true)
    class, ``n``."""
    dev = _dev()
    p_ins, p_sem = _i32(pred_label['instances'], dev), _i32(pred_label['semantics'], dev)
    g_ins, g_sem = _i32(gt_label['instances'], dev), _i32(gt_label['semantics'], dev)
    n = p_ins.shape[0]
    assert p_sem.shape[0] == n and g_ins.shape[0] == n and g_sem.shape[0] == n
    pv, pi = _dense(p_ins, skip=-1)
    gv, gi = _dense(g_ins)
    P, G = int(pv.numel()), int(gv.numel())
    if max(P, 1) * max(G, 1) > JOINT_HIST_MAX:
        raise B2MError('s3dis_counts: %d x %d instances exceed the joint table (%d entries)' % (P, G, JOINT_HIST_MAX))
    inter = joint_hist(pi, gi, max(P, 1), max(G, 1))[:P, :G]
    p_cls = joint_hist(pi, p_sem, max(P, 1), NUM_CLASSES)[:P]
    g_cls = joint_hist(gi, g_sem, max(G, 1), NUM_CLASSES)[:G]
    p_size = joint_hist(pi, None, max(P, 1))[:P, 0]
    g_size = joint_hist(gi, None, max(G, 1))[:G, 0]
    cc = joint_hist(p_sem, g_sem, NUM_CLASSES, NUM_CLASSES)
    host = [t.cpu().numpy().astype(np.int64) for t in (inter, p_cls, g_cls, p_size, g_size, cc)]
    return {'inter': host[0].reshape(P, G), 'pred_class': host[1].reshape(P, NUM_CLASSES).argmax(1),
            'gt_class': host[2].reshape(G, NUM_CLASSES).argmax(1), 'pred_size': host[3], 'gt_size': host[4], 'cc': host[5], 'n': n}


def s3dis_eval_from_counts(rooms, details=False):
    """s3dis_util.py:179-338 over the per-room tables of ``s3dis_counts``: (mPrec, mRec, precision[13], recall[13]); with details a
    fifth element {'oAcc', 'iou' (13), 'mIoU', 'MUCov' (13), 'MWCov' (13)} -- what the reference computes and does not return."""
    total_true = 0
    total_seen = 0
    true_positive_classes = np.zeros(NUM_CLASSES)
    positive_classes = np.zeros(NUM_CLASSES)
    gt_classes = np.zeros(NUM_CLASSES)
    total_gt_ins = np.zeros(NUM_CLASSES)
    tpsins = [[] for _ in range(NUM_CLASSES)]
    fpsins = [[] for _ in range(NUM_CLASSES)]
    all_mean_cov = [[] for _ in range(NUM_CLASSES)]
    all_mean_weighted_cov = [[] for _ in range(NUM_CLASSES)]
    for room in rooms:
        cc = np.asarray(room['cc'], np.int64)
        total_true += int(np.trace(cc))
        total_seen += int(room['n'])
        gt_classes += cc.sum(0)
        positive_classes += cc.sum(1)
        true_positive_classes += np.diag(cc)
        inter = np.asarray(room['inter'], np.int64)
        psize, gsize = np.asarray(room['pred_size'], np.int64), np.asarray(room['gt_size'], np.int64)
        pcls, gcls = np.asarray(room['pred_class']), np.asarray(room['gt_class'])
        for i_sem in range(NUM_CLASSES):
            preds = np.nonzero(pcls == i_sem)[0]
            gts = np.nonzero(gcls == i_sem)[0]
            sum_cov = 0
            mean_weighted_cov = 0
            num_gt_point = 0
            for g in gts:
                ovmax = 0.
                num_gt_point += gsize[g]
                for p in preds:
                    iou = float(inter[p, g]) / (psize[p] + gsize[g] - inter[p, g])
                    if iou > ovmax:
                        ovmax = iou
                sum_cov += ovmax
                mean_weighted_cov += ovmax * gsize[g]
            if len(gts) != 0:
                all_mean_cov[i_sem].append(sum_cov / len(gts))
                all_mean_weighted_cov[i_sem].append(mean_weighted_cov / num_gt_point)
            tp = [0.] * len(preds)
            fp = [0.] * len(preds)
            total_gt_ins[i_sem] += len(gts)
            for ip, p in enumerate(preds):
                ovmax = -1.
                for g in gts:
                    iou = float(inter[p, g]) / (psize[p] + gsize[g] - inter[p, g])
                    if iou > ovmax:
                        ovmax = iou
                if ovmax >= IOU_TH:
                    tp[ip] = 1
                else:
                    fp[ip] = 1
            tpsins[i_sem] += tp
            fpsins[i_sem] += fp
    precision = np.zeros(NUM_CLASSES)
    recall = np.zeros(NUM_CLASSES)
    with np.errstate(divide='ignore', invalid='ignore'):
        for i_sem in range(NUM_CLASSES):
            tp = np.sum(np.asarray(tpsins[i_sem]).astype(float))
            fp = np.sum(np.asarray(fpsins[i_sem]).astype(float))
            recall[i_sem] = tp / total_gt_ins[i_sem]
            precision[i_sem] = tp / (tp + fp)
        out = (np.mean(precision), np.mean(recall), precision, recall)
        if not details:
            return out
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)         # (np.mean of an empty list: nan, as in the reference)
            mucov = np.array([np.mean(v) for v in all_mean_cov])
            mwcov = np.array([np.mean(v) for v in all_mean_weighted_cov])
        iou = true_positive_classes / (gt_classes + positive_classes - true_positive_classes)
        extra = {'oAcc': total_true / float(total_seen) if total_seen else float('nan'), 'iou': iou, 'mIoU': np.mean(iou),
                 'MUCov': mucov, 'MWCov': mwcov}
    return out + (extra,)


def instance_counts(rooms):
    """The integers behind precision and recall (s3dis_util.py:273-299) over the per-room tables of ``s3dis_counts``: (tp (13),
    fp (13), total_gt (13)) int64.  A predicted instance is a true positive when a ground-truth instance of its class has
    inter / union >= 0.5, i.e. 3 * inter >= |P| + |G| -- the same decision as the float division for counts below 2^31."""
    tp, fp, total = (np.zeros(NUM_CLASSES, np.int64) for _ in range(3))
    for room in rooms:
        inter = np.asarray(room['inter'], np.int64)
        psize, gsize = np.asarray(room['pred_size'], np.int64), np.asarray(room['gt_size'], np.int64)
        pcls, gcls = np.asarray(room['pred_class']), np.asarray(room['gt_class'])
        total += np.bincount(gcls, minlength=NUM_CLASSES)[:NUM_CLASSES]
        for p, c in enumerate(pcls):
            same = gcls == c
            hit = bool((3 * inter[p][same] >= psize[p] + gsize[same]).any())
            (tp if hit else fp)[c] += 1
    return tp, fp, total


def s3dis_eval(pred_labels, gt_labels, details=False):
    """s3dis_util.s3dis_eval(pred_labels, gt_labels): lists of {'semantics', 'instances'} per room (arrays or tensors)."""
    assert len(pred_labels) == len(gt_labels)
    return s3dis_eval_from_counts([s3dis_counts(p, g) for p, g in zip(pred_labels, gt_labels)], details=details)


def sparse2dense(full_positions, sampled_positions):
    """For every point of the unsampled room the index of the nearest sampled point: int64 (n_full) on the device.

    The reference CALLS ``get_sparse2dense(scene_full, scene, cfg)`` (evaluation.py:154) but defines it nowhere.  This is the
    definition its uses at :219-220 require -- an index into the sampled room per point of the full one -- built on the search the
    reference uses everywhere else (1-nearest neighbour, ball tree).  Lowest row among exactly equidistant sampled points."""
    from .neighbors import NearestIndex
    return NearestIndex(sampled_positions).query(full_positions)


def evaluate_rooms(model, batches, details=False, viz_path=None, full_rooms=None):
    """The loop of Evaluater.s3dis_eval (evaluation.py:137-231) over batches of ONE room each: prediction, masks, per-point
    semantics from the per-voxel head, ``room_labels``, then ``s3dis_eval`` against batch['labels'][0]['semantics' / 'instances'].

    With ``cfg.full_resolution`` the unsampled rooms come through ``full_rooms``: a sequence aligned with ``batches`` of
    ``(scene_full, labels_full)`` dicts ('positions'; 'semantics', 'instances'), or a callable ``name -> (scene_full, labels_full)``
    (what ``s3dis.process_scene`` returns with ``point_sampling_rate = None``, evaluation.py:152-153).  The predicted semantics and
    instances are gathered through ``sparse2dense`` and scored against the full room's ground truth (evaluation.py:213-222)."""
    cfg = model.cfg
    full = bool(getattr(cfg, 'full_resolution', False))
    if full and full_rooms is None:
        raise NotImplementedError('evaluate_rooms: cfg.full_resolution needs the unsampled rooms: pass full_rooms= (a sequence aligned '
                                  'with the batches of (scene_full, labels_full), or a callable name -> (scene_full, labels_full))')
    if viz_path is not None:
        raise NotImplementedError('evaluate_rooms: the visualisation path (visualize_prediction) is not implemented')
    if cfg.mlp_per_vox_semantics not in cfg.network_heads:
        raise ValueError('evaluate_rooms needs the per-voxel semantics head (%s)' % cfg.mlp_per_vox_semantics)
    dev = _dev()
    pred_labels, gt_labels = [], []
    for i, batch in enumerate(batches):
        assert len(batch['scene']) == 1, 'S3DIS is evaluated with batch size 1 (evaluation.py:131)'
        prediction = model.get_prediction(batch, with_grad=False, to_cpu=True, min_size=True)
        scene, labels = batch['scene'][0], batch['labels'][0]
        vox_sem = torch.argmax(torch.as_tensor(prediction[cfg.mlp_per_vox_semantics]), 1)
        results = model.pred2mask(batch, prediction, 'eval')
        v2p = torch.as_tensor(np.asarray(batch['vox2point'][0])).long()
        sem = vox_sem.cpu()[v2p]
        pred = room_labels(sem.to(dev), scene['positions'], scene['normals'], results[scene['name']]['mask'])
        if full:
            scene_full, labels = full_rooms(scene['name']) if callable(full_rooms) else full_rooms[i]
            s2d = sparse2dense(scene_full['positions'], scene['positions'])
            pred = {'semantics': pred['semantics'][s2d], 'instances': pred['instances'][s2d]}
        pred_labels.append(pred)
        gt_labels.append({'semantics': labels['semantics'], 'instances': labels['instances']})
    return s3dis_eval(pred_labels, gt_labels, details=details)
