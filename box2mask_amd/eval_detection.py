"""ARKitScenes oriented-box detection mAP of predicted masks.

Mirrors ``Evaluater.arkitscenes_eval`` (/root/reference/models/evaluation.py:245-316) and what it drives:
``box_util.get_oriented_corners`` / ``get_rotated_bounds`` (utils/box_util.py:339-384), ``box3d_iou`` with ``polygon_clip``
(:19-66, :101-140), ``metric_util.calc_iou`` (utils/metric_util.py:91-113) and ``eval_det`` / ``eval_det_cls`` / ``voc_ap``
(utils/evaluate_detections.py:28-59, 80-165, 174-221).  The expensive part of the reference -- one qhull call per mask over
``positions[mask]`` and a Python polygon clip plus another qhull call per (prediction, ground truth) pair -- is
``b2m_mask_hulls`` over the bit-packed masks and ``b2m_hull_box_iou`` over the pair table (include/b2m.h, csrc/detbox.hip); the
matching walks a few hundred records and stays on the host.

Records are arrays instead of the reference's nested lists: per scene ``label`` / ``conf`` of the kept predictions in
prediction order, ``gt_label`` of the ground-truth boxes in label order and ``iou`` (predictions x ground truths, zero where
the classes differ -- the reference never looks at such a pair).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from ._lib import B2MError, ptr

# arkitscenes_name_from_semantic_class_id (dataprocessing/arkitscenes.py:67-85): for the printed table only
CLASS_NAMES = {3: 'cabinet', 4: 'bed', 5: 'chair', 6: 'sofa', 7: 'table', 15: 'shelf', 18: 'stove', 19: 'washer', 20: 'oven',
               21: 'dishwasher', 22: 'fireplace', 23: 'stool', 24: 'refrigerator', 25: 'tv_monitor', 33: 'toilet', 34: 'sink',
               36: 'bathtub'}
MIN_POINTS = 50                       # evaluation.py:277-278
HULL_MAX = 512                        # B2M_HULL_MAX
HULL_CHUNKS, HULL_PART = 32, 56       # B2M_HULL_CHUNKS, B2M_HULL_PART
OBB_REC = 16                          # B2M_OBB_REC
FLAG_VERTICES, FLAG_CANDIDATES = 1, 2
DEFAULT_CAP = 4096                    # hull candidates per row on the first attempt


def _dev():
    _lib.require_gpu()
    return torch.device('cuda', torch.cuda.current_device())


def _f64(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a).to(dev).double().contiguous()


def pack_masks(masks, dev=None):
    """(K, n) bool / byte masks -> (K, words) bit rows on the device (b2m_mask_pack)."""
    dev = dev or _dev()
    m = torch.as_tensor(masks).to(dev)
    if m.dtype != torch.bool:
        m = m != 0
    m = m.to(torch.uint8).contiguous()
    k, n = m.shape
    words = (n + 63) // 64
    bits = torch.empty((k, max(words, 1)), dtype=torch.int64, device=dev)
    _lib.call('b2m_mask_pack', ptr(m), k, n, ptr(bits), words)
    return bits, words, n


def hulls_from_bits(bits, words, n, positions, cap=DEFAULT_CAP):
    """One b2m_mask_hulls call: per row ``count``, ``box6``, ``hull`` (K, HULL_MAX, 2), ``n_hull``, ``flags``, ``ncand`` (device)."""
    dev = bits.device
    k = bits.shape[0]
    pos = _f64(positions, dev)
    assert pos.shape == (n, 3), 'positions %s for masks over %d points' % (tuple(pos.shape), n)
    out = {'count': torch.empty(k, dtype=torch.int32, device=dev), 'box6': torch.empty((k, 6), dtype=torch.float64, device=dev),
           'hull': torch.zeros((k, HULL_MAX, 2), dtype=torch.float64, device=dev),
           'n_hull': torch.empty(k, dtype=torch.int32, device=dev), 'flags': torch.empty(k, dtype=torch.int32, device=dev),
           'ncand': torch.empty(k, dtype=torch.int32, device=dev), 'cap': cap}
    work = torch.empty(max(k, 1) * HULL_CHUNKS * HULL_PART, dtype=torch.float64, device=dev)
    cand = torch.empty((max(k, 1), cap, 2), dtype=torch.float64, device=dev)
    stk = torch.empty((max(k, 1), cap), dtype=torch.int32, device=dev)
    _lib.call('b2m_mask_hulls', ptr(bits), words, k, ptr(pos), n, ptr(work), ptr(cand), ptr(stk), cap, ptr(out['ncand']),
              ptr(out['count']), ptr(out['box6']), ptr(out['hull']), ptr(out['n_hull']), ptr(out['flags']))
    return out


def check_flags(flags, n_hull, ncand):
    """Host arrays of one b2m_mask_hulls call -> 0 if every hull was reported, else the candidate capacity a second call needs.
    A hull beyond HULL_MAX vertices is an error: it is never reported truncated."""
    over = np.nonzero(flags == FLAG_VERTICES)[0]
    if len(over):
        raise B2MError('convex hull of mask row %d has %d vertices (capacity B2M_HULL_MAX = %d)'
                       % (int(over[0]), int(n_hull[over[0]]), HULL_MAX))
    if (flags == FLAG_CANDIDATES).any():
        return 1 << int(ncand.max() - 1).bit_length()
    return 0


def mask_boxes(pred_info, positions, min_points=MIN_POINTS, check=True, cap=DEFAULT_CAP):
    """Prisms of the predictions of one scene.  pred_info: {'conf' (K,), 'label_id' (K,), 'mask' (K, n)} as
    ``Model.pred2mask(..., 'eval')`` returns; positions (n, 3).  Returns the b2m_mask_hulls arrays on the device plus ``cls``
    (K,) int32 on the device: the label of the predictions with at least ``min_points`` points (evaluation.py:277-278), -1 for
    the others.  check=True reads the flags back (one small copy): B2MError for a hull beyond the capacity, a second pass with
    a larger candidate buffer when the first one filled.  check=False leaves that to ``scene_ious``."""
    dev = _dev()
    bits, words, n = pack_masks(pred_info['mask'], dev)
    label = torch.as_tensor(np.asarray(torch.as_tensor(pred_info['label_id']).cpu()).astype(np.int32)).to(dev)
    out = hulls_from_bits(bits, words, n, positions, cap)
    out.update(bits=bits, words=words, n=n, positions=positions, label=label, min_points=min_points,
               conf=np.asarray(torch.as_tensor(pred_info['conf']).cpu()), label_id=np.asarray(label.cpu()) if check else None)
    out['cls'] = torch.where(out['count'] >= min_points, label, torch.full_like(label, -1))
    if check:
        host = torch.stack([out['flags'], out['n_hull'], out['ncand'], out['count']]).cpu().numpy()
        out = _recheck(out, host)
    return out


def _recheck(out, host):
    need = check_flags(host[0], host[1], host[2])
    if need:
        again = hulls_from_bits(out['bits'], out['words'], out['n'], out['positions'], need)
        out.update(again)
        host = torch.stack([out['flags'], out['n_hull'], out['ncand'], out['count']]).cpu().numpy()
        if check_flags(host[0], host[1], host[2]):
            raise B2MError('hull candidates still exceed the buffer (%d)' % need)
    out['count_host'] = host[3]
    out['keep'] = host[3] >= out['min_points']
    return out


def gt_boxes(labels):
    """Ground-truth boxes of one scene from labels['per_instance_bb_centers' / '_bounds' / '_rotations'] and
    'per_instance_semantics' (evaluation.py:257-270).  Labels without rotations are axis-aligned boxes."""
    dev = _dev()
    centers = _f64(np.asarray(labels['per_instance_bb_centers'], dtype=np.float64).reshape(-1, 3), dev)
    bounds = _f64(np.asarray(labels['per_instance_bb_bounds'], dtype=np.float64).reshape(-1, 3), dev)
    g = centers.shape[0]
    if 'per_instance_bb_rotations' in labels:
        rot = _f64(np.asarray(labels['per_instance_bb_rotations'], dtype=np.float64).reshape(-1, 9), dev)
    else:
        rot = torch.eye(3, dtype=torch.float64, device=dev).reshape(1, 9).repeat(g, 1).contiguous()
    assert bounds.shape[0] == g and rot.shape[0] == g
    label = np.asarray(labels['per_instance_semantics']).astype(np.int32)[:g]
    boxes = torch.empty((g, OBB_REC), dtype=torch.float64, device=dev)
    _lib.call('b2m_obb_corners', ptr(centers), ptr(bounds), ptr(rot), g, ptr(boxes))
    return {'boxes': boxes, 'centers': centers, 'cls': torch.as_tensor(label).to(dev), 'label': label, 'g': g}


def scene_ious(pred, gt, oriented=True):
    """(K, g) float64 IoU table of one scene on the host: box3d_iou (oriented) or calc_iou of every same-class pair, zero
    elsewhere and in the rows of dropped predictions.  One device -> host copy (the table and the hull flags together)."""
    k, g = pred['cls'].shape[0], gt['g']
    dev = pred['cls'].device
    iou = torch.zeros((k, max(g, 1)), dtype=torch.float64, device=dev)
    if oriented:
        _lib.call('b2m_hull_box_iou', ptr(pred['hull']), ptr(pred['n_hull']), ptr(pred['box6']), ptr(pred['cls']), k,
                  ptr(gt['boxes']), ptr(gt['cls']), g, ptr(iou))
    else:
        _lib.call('b2m_aabb_iou', ptr(pred['box6']), ptr(pred['cls']), k, ptr(gt['centers']), ptr(gt['boxes']), ptr(gt['cls']), g,
                  ptr(iou))
    if 'keep' in pred:
        return iou[:, :g].cpu().numpy()
    side = torch.stack([pred['flags'], pred['n_hull'], pred['ncand'], pred['count']], 1).double()
    host = torch.cat([iou, side], 1).cpu().numpy()
    info = host[:, -4:].T.astype(np.int64)
    if oriented and info[0].any():                    # a hull was not reported: raise, or redo the scene with a larger buffer
        _recheck(pred, info)
        return scene_ious(pred, gt, oriented)
    pred['count_host'] = info[3]
    pred['keep'] = info[3] >= pred['min_points']
    return host[:, :g]


def voc_ap(rec, prec, use_07_metric=False):
    """evaluate_detections.py:28-59."""
    if use_07_metric:
        ap = 0.
        for t in np.arange(0., 1.1, 0.1):
            p = 0 if np.sum(rec >= t) == 0 else np.max(prec[rec >= t])
            ap = ap + p / 11.
        return ap
    mrec = np.concatenate(([0.], rec, [1.]))
    mpre = np.concatenate(([0.], prec, [0.]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def eval_det_cls(dets, npos, ovthresh=0.25, use_07_metric=False):
    """evaluate_detections.py:80-165 for one class.  dets: per scene, in scene order, (conf (d,), iou (d, gc)) -- the detections
    of the class in prediction order against the scene's ground truths of the class in label order; npos: ground truths of the
    class over all scenes.  Returns (rec, prec, ap)."""
    confidence = np.array([c for conf, _ in dets for c in conf])
    where = [(s, i) for s, (conf, _) in enumerate(dets) for i in range(len(conf))]
    taken = [np.zeros(iou.shape[1], bool) for _, iou in dets]
    sorted_ind = np.argsort(-confidence)
    nd = len(where)
    tp = np.zeros(nd)
    fp = np.zeros(nd)
    for d in range(nd):
        s, i = where[sorted_ind[d]]
        ovmax = -np.inf
        jmax = -1
        for j, iou in enumerate(dets[s][1][i]):
            if iou > ovmax:                          # the first maximum
                ovmax = iou
                jmax = j
        if ovmax > ovthresh:
            if not taken[s][jmax]:
                tp[d] = 1.
                taken[s][jmax] = True
            else:
                fp[d] = 1.                           # a second detection of a matched ground truth
        else:
            fp[d] = 1.
    fp = np.cumsum(fp)
    tp = np.cumsum(tp)
    with np.errstate(divide='ignore', invalid='ignore'):
        rec = tp / float(npos)                       # (no ground truth of the class anywhere: nan, left out of the mean)
    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    return rec, prec, voc_ap(rec, prec, use_07_metric)


def eval_det(records, ovthresh=0.25, use_07_metric=False):
    """evaluate_detections.py:174-221.  records: {scene: {'label' (K,), 'conf' (K,), 'gt_label' (g,), 'iou' (K, g)}} in scene
    order.  A class is scored if it has a prediction AND appears among the classes of the predictions or the ground truth: as
    in the reference, a class with ground truth and no prediction at all raises KeyError there and is skipped, and a class with
    predictions and no ground truth comes out as nan.  Returns (rec, prec, ap) keyed by class id, in the reference's order."""
    classes = []
    for r in records.values():
        for c in r['label']:
            if int(c) not in classes:
                classes.append(int(c))
    with_pred = set(classes)
    for r in records.values():
        for c in r['gt_label']:
            if int(c) not in classes:
                classes.append(int(c))
    rec, prec, ap = {}, {}, {}
    for c in classes:
        if c not in with_pred:
            continue
        dets = []
        for r in records.values():
            psel = np.nonzero(np.asarray(r['label']) == c)[0]
            if len(psel) == 0:
                continue                              # (scenes without a prediction of the class add no detection)
            gsel = np.nonzero(np.asarray(r['gt_label']) == c)[0]
            dets.append((np.asarray(r['conf'])[psel], np.asarray(r['iou']).reshape(len(r['label']), -1)[np.ix_(psel, gsel)]))
        npos = sum(int((np.asarray(r['gt_label']) == c).sum()) for r in records.values())
        rec[c], prec[c], ap[c] = eval_det_cls(dets, npos, ovthresh, use_07_metric)
    return rec, prec, ap


def mean_ap(ap):
    """evaluation.py:314."""
    vals = [v for v in ap.values() if not math.isnan(v)]
    return np.mean(np.array(vals)) if vals else float('nan')


def scene_record(pred_info, positions, labels, oriented_boxes=True, min_points=MIN_POINTS):
    pred = mask_boxes(pred_info, positions, min_points, check=False)
    gt = gt_boxes(labels)
    iou = scene_ious(pred, gt, oriented_boxes)
    keep = pred['keep']
    label_id = np.asarray(torch.as_tensor(pred_info['label_id']).cpu())
    return {'label': label_id[keep], 'conf': pred['conf'][keep], 'gt_label': gt['label'], 'iou': iou[keep]}


def arkitscenes_eval(results, scenes, labels, oriented_boxes=True, iou_t=0.5, verbose=True):
    """results: {scene name: pred_info} as ``Model.pred2mask(..., 'eval')`` returns, in the order of ``scenes`` (each with
    'name' and 'positions') and ``labels``.  Returns (mAP, {class id: AP})."""
    records = {}
    names = list(results.keys())
    for i, scene in enumerate(scenes):
        records[scene['name']] = scene_record(results[names[i]], scene['positions'], labels[i], oriented_boxes)
    _, _, ap = eval_det(records, ovthresh=iou_t)
    m = mean_ap(ap)
    if verbose:
        for c, v in sorted(ap.items()):
            print(f'{CLASS_NAMES.get(c, str(c)):>15}: \t {v:.3f}')
        print('mAP: ', m)
    return m, ap
