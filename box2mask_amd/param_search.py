"""Threshold search for the votes -> masks stage: every setting of a grid over (cluster_th, score_th, mask_bin_th, mask_nms_th)
scored with the ScanNet AP, from work shared between the settings.

The reference's ``Evaluater.param_search`` (/root/reference/models/evaluation.py:353-366) takes the four thresholds of
``detection2mask`` from the ``*_th_search`` options (config_loader.py:133-139, ``np.linspace`` triples; 6 x 5 x 4 x 5 = 600 settings
by default) and runs every setting as a CPU evaluation job of its own over the whole validation split.  Here:

  * the clusters and heat-maps depend on ``cluster_th`` alone                        -> one ``b2m_nmc_batch`` per cluster_th;
  * ``score_th`` keeps a PREFIX of the cluster list (representatives come in descending score, ``scores > score_th``,
    detection_net.py:427-432), and a cluster's heat-map row, mask and label do not depend on which other clusters were kept
                                                                                     -> rows are projected once, for the smallest score_th;
  * voxel masks, their pairwise intersections, their labels and their overlaps with the ground truth depend on
    (cluster_th, mask_bin_th) alone                                                  -> one mask stage per pair;
  * the fate of row i in the greedy mask NMS (iou_nms.py:130-144) depends on the rows before i only, so the walk over a prefix is
    the restriction of the walk over the whole list: kept(c, s, b, m) = kept(c, b, m) & [0, k_s)
                                                                                     -> one walk per mask_nms_th over the same table;
  * the AP needs, per kept prediction, its score, its label and the number of scene POINTS it shares with every ground-truth id
    (``eval_metric.assign_from_counts``); point p lies in mask r iff bit vox2point[p] of voxel mask r is set
                                                                                     -> ``b2m_mask_hist_index``, no per-point mask.

So 600 settings cost 6 clusterings and 24 mask stages per batch, a few host reads per stage, and the host matching of
``eval_metric`` per setting.  Segment-level flow only (segment-level votes, mask NMS): a network with a per-voxel semantics head
has no mask NMS to sweep.

The reference's search is not ScanNet-specific: with ``dataset_name = arkitscenes`` every job ends in ``arkitscenes_eval``
(evaluation.py:245-316), the oriented-box detection mAP.  The front half above is shared (``_cluster_stages``, built on the scene
inputs, the clustering read-back and the ``MaskTable`` of mask_stages.py, which ``detection2mask`` calls as well); what a stage is
scored with differs:

  * per projected row its point count, z range and x-y convex hull, and the IoU of that prism with every same-class ground-truth
    box, depend on (cluster_th, mask_bin_th) alone -- score_th and mask_nms_th only select rows
                                                                                     -> ``b2m_mask_hulls_index_batch`` + one IoU call per
                                                                                        scene and stage: 24 hull stages, not 600;
  * rows under 50 points are skipped AFTER the mask NMS (evaluation.py:280)          -> ``detection_records`` gates what ``compose`` kept.

The S3DIS flow (per-voxel semantics head, no mask NMS; evaluation.py:124-231) is the third: ``s3dis_param_search`` scores mPrec / mRec.
Its stage 0 and clustering are the same ``mask_stages`` functions, for a batch of one room.  There the wall DBSCAN depends on no
threshold (once per room), the greedy merge of the proposals is prefix-closed (one
``b2m_paint_proposals`` per (cluster_th, mask_bin_th) over the rows of the smallest score_th) and ``b2m_s3dis_prefix_tail`` scores every
score prefix of a stage at once; profiles/s3dis_sweep_rule.md has the rule.

``detection_tables`` / ``detection_records`` / ``arkit_param_search``; matching and VOC AP are the unchanged ``eval_detection.eval_det``.  ``compose`` and the matching are host logic like ``assign_from_counts``; every kernel stage is HIP.
With ``matching='device'`` the matching, the curves and the AP run on the device as well (eval_match.py): the stage results are
matched where they lie and nothing but an entry count per stage comes to the host.
"""
from __future__ import annotations

import contextlib
import itertools
import warnings

import numpy as np
import torch

from . import _lib
from . import eval_detection
from . import eval_metric
from . import iou_nms
from . import mask_stages

_call = _lib.call
AXES = ('cluster_th', 'score_th', 'mask_bin_th', 'mask_nms_th')


class ThresholdGrid:
    """Four ascending float64 arrays.  A threshold enters its stage converted exactly as the single-setting path converts it:
    ``np.float32(score_th)`` on the host, C ``float`` at the ABI for the other three."""

    def __init__(self, cluster_th, score_th, mask_bin_th, mask_nms_th):
        for name, v in zip(AXES, (cluster_th, score_th, mask_bin_th, mask_nms_th)):
            a = np.atleast_1d(np.asarray(v, np.float64)).copy()
            if a.ndim != 1 or a.size == 0 or not np.all(np.isfinite(a)) or not np.all(np.diff(a) > 0):
                raise ValueError('%s: a non-empty, strictly ascending list of thresholds is needed, got %r' % (name, v))
            setattr(self, name, a)
        if not (np.all(self.cluster_th > 0) and np.all(self.cluster_th < 1)):
            raise ValueError('cluster_th must lie in (0, 1) (iou_nms.py:71)')
        if not (np.all(self.mask_bin_th >= 0) and np.all(self.mask_bin_th < 1)):
            raise ValueError('mask_bin_th must lie in [0, 1): below 0 the zero-padded background joins every mask')
        if self.mask_nms_th.size > 64:
            raise ValueError('at most 64 mask_nms_th values per sweep (B2M_SWEEP_MAX_TH)')

    @classmethod
    def from_cfg(cls, cfg):
        """The ``*_th_search`` triples of the configuration, each as ``np.linspace(min, max, num)`` (evaluation.py:359-362)."""
        return cls(*(np.linspace(float(t[0]), float(t[1]), int(t[2])) for t in (getattr(cfg, a + '_search') for a in AXES)))

    @property
    def shape(self):
        return tuple(int(getattr(self, a).size) for a in AXES)

    def settings(self):
        """Every (ci, si, bi, mi) in grid order (the reference's loop nest)."""
        return itertools.product(*(range(n) for n in self.shape))

    def eval_ths(self, ci, si, bi, mi):
        """The setting as a ``cfg.eval_ths`` list."""
        return [float(self.cluster_th[ci]), float(self.score_th[si]), float(self.mask_bin_th[bi]), float(self.mask_nms_th[mi])]


class SweepTables:
    """What every setting of the grid needs of ONE scene, as host arrays.

    clusters[ci]:    K, conf (K,) float32 in visiting order, reps (K,) int64 rows among the foreground votes, ks (n_score,) = the
                     number of clusters with ``conf > score_th`` (a prefix);
    stages[ci][bi]:  label_id (K',) int32, inter (K', G) int64 on POINTS, keep (n_nms, K') bool with K' = ks[0];
    uniq, gt_vert:   the ground-truth ids of the scene (ascending) and their point counts."""
    __slots__ = ('name', 'n_pts', 'uniq', 'gt_vert', 'clusters', 'stages')

    def __init__(self, name, n_pts, uniq, gt_vert):
        self.name, self.n_pts, self.uniq, self.gt_vert = name, n_pts, uniq, gt_vert
        self.clusters, self.stages = [], []


def compose(tables, ci, si, bi, mi):
    """Rows of ``tables.clusters[ci]`` that survive setting (ci, si, bi, mi): the prefix of the score filter, then the restriction
    of the full-list mask NMS to it.  Pure numpy."""
    k_s = int(tables.clusters[ci]['ks'][si])
    return np.nonzero(tables.stages[ci][bi]['keep'][mi, :k_s])[0].astype(np.int64)


def records(tables, ci, si, bi, mi):
    """The scene's per-class records of one setting, through the unchanged ``eval_metric.assign_from_counts``."""
    rows = compose(tables, ci, si, bi, mi)
    st = tables.stages[ci][bi]
    return eval_metric.assign_from_counts(tables.name, st['label_id'][rows].astype(np.int64), tables.clusters[ci]['conf'][rows],
                                          tables.uniq, tables.gt_vert, st['inter'][rows])


# ----------------------------------------------------------------------------------------------------------------- device stages
def _scannet_inputs(net, batch, pred, cfg, dev):
    """``mask_stages.scene_inputs`` with the points, for the sweeps of the ScanNet flow."""
    if net.requires_voxel_outputs:
        raise ValueError('this threshold sweep covers the ScanNet flow only (segment-level votes, mask NMS): a network with a '
                         'per-voxel semantics head (requires_voxel_outputs) has no mask NMS to sweep -- its thresholds are swept '
                         'with the S3DIS metric by param_search.s3dis_param_search')
    return mask_stages.scene_inputs(net, batch, pred, cfg, dev, points=True)


def sweep_tables(net, batch, pred, cfg, grid, gt_ids, acc=None):
    """``SelectionNet.detection2mask_sweep``: one ``SweepTables`` per scene of the batch.  gt_ids: {scene name: (n_pts,) ids
    ``label*1000 + instance``} or a list in scene order.

    With ``acc`` (an ``eval_match.MatchAccumulator`` over all ``grid.settings()`` in grid order) the results of a stage are not
    read to the host: its keep flags, labels and point histograms are matched where they lie, for the n_score x n_nms settings
    of the stage in one launch, and the tables come back with ``clusters`` only (``stages`` stay empty lists)."""
    _lib.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    sc = _scannet_inputs(net, batch, pred, cfg, dev)
    if not sc:
        return []
    S = len(sc)
    n_class = int(max(int(net.semantic_valid_class_ids.max()) + 1, 1))
    tabs = []
    for d in sc:
        ids = np.asarray(gt_ids[d['name']] if isinstance(gt_ids, dict) else gt_ids[d['idx']]).astype(np.int64).reshape(-1)
        if ids.shape[0] != d['n_pts']:
            raise ValueError('%s: %d ground-truth ids for %d points' % (d['name'], ids.shape[0], d['n_pts']))
        if ids.size and ids.min() < 0:
            raise ValueError('negative ground-truth ids')
        uniq, dense, vert = np.unique(ids, return_inverse=True, return_counts=True)
        if len(uniq) > 2048:
            raise ValueError('more than 2048 ground-truth ids in one scene')
        d['G'] = max(len(uniq), 1)
        d['dense32'] = torch.from_numpy(dense.reshape(-1).astype(np.int32)).to(dev)
        tabs.append(SweepTables(d['name'], d['n_pts'], uniq.astype(np.int64), vert.astype(np.int64)))
    for c in _cluster_stages(sc, grid, dev, tabs, n_class, _hist_tail):
        if acc is not None:                                                # the scores of the clusters, where the matching reads them
            conf_dev = [d['boxes'][r.reps[:r.k].long(), 0].contiguous() for d, r in zip(sc, c.rs)]
        for bi, bth in enumerate(grid.mask_bin_th):
            c.shared(bth)
            if c.total:
                _call('b2m_mask_hist_index_batch', c.extra_ptr, S, c.max_words, c.max_pts)
            if acc is not None:
                _match_stage(acc, grid, c.ci, bi, tabs, sc, c.cl, c.ksels, conf_dev, c.res, c.n_nms, c.total, c.o_lab, c.o_tail)
                continue
            host = c.res.cpu().numpy()                                     # the one host read of the stage
            hoff = 0
            for s_, (t, d, k) in enumerate(zip(tabs, sc, c.ksels)):
                keep, label = c.split(host, s_)
                inter = host[c.o_tail + hoff:c.o_tail + hoff + k * d['G']].reshape(k, d['G'])[:, :len(t.uniq)].astype(np.int64)
                t.stages[-1].append(dict(label_id=label, inter=inter, keep=keep))
                hoff += k * d['G']
    return tabs


def _hist_tail(c, sc):
    """The scorer's part of a cluster stage for the ScanNet AP: the point histograms behind the labels, and the B2M_HIST_DESC table."""
    hdesc = np.zeros((len(sc), 10), np.int64)
    tb_all, tb_ptrs = mask_stages.voxel_major_scratch(sc, c.ksels, c.dev)
    n_hist = sum(k * d['G'] for k, d in zip(c.ksels, sc))

    def fill(res):
        hoff = 0
        for s_, (d, k) in enumerate(zip(sc, c.ksels)):
            hdesc[s_] = (c.bits_ptr[s_], k, d['words'], d['n_vox'], d['v2p'].data_ptr(), d['dense32'].data_ptr(), d['n_pts'], d['G'],
                         tb_ptrs[s_], res.data_ptr() + 4 * (c.o_tail + hoff))
            hoff += k * d['G']
        return hdesc.reshape(-1), tb_all
    return n_hist, fill


class _ClusterStage:
    """What the mask stages of ONE cluster_th share, for every scene of the batch: the clusters, the rows of the smallest score_th,
    their bit rows and the result buffer ``res`` = keep flags (n_nms x total) | labels (total) | the scorer's tail, int32."""

    def shared(self, bth):
        """Projection, the mask NMS of every mask_nms_th and the labels of every projected row for one mask_bin_th."""
        if self.total:
            S = len(self.ksels)
            _call('b2m_mask_project_batch', self.desc_ptr, S, self.total, self.max_words, float(bth))
            _call('b2m_mask_nms_sweep_batch', self.desc_ptr, S, max(self.ksels), self.ths_nms.ctypes.data, self.n_nms, self.res.data_ptr(),
                  self.total)
            _call('b2m_label_hist_batch', self.desc_ptr, S, self.total, self.n_class)

    def split(self, host, s_):
        """(keep (n_nms, k) bool, label_id (k,) int32) of scene s_ from the host copy of ``res``."""
        r0, k, total = self.row0[s_], self.ksels[s_], self.total
        keep = np.stack([host[m * total + r0:m * total + r0 + k] for m in range(self.n_nms)], 0) != 0
        return keep, host[self.o_lab + r0:self.o_lab + r0 + k].copy()


def _cluster_stages(sc, grid, dev, tabs, n_class, tail):
    """The front half every scorer shares: per cluster_th the clustering, the prefixes ``ks`` (appended to ``tabs``) and a
    ``_ClusterStage``.  ``tail(c, sc)`` -> (number of int32 the scorer wants behind the labels, fill(res) -> (its int64 descriptor
    table, whatever must stay alive)): the table rides behind the B2M_MASK_DESC table in the one upload, at ``c.extra_ptr``."""
    ths_nms = np.ascontiguousarray(grid.mask_nms_th, np.float32)           # C float, as float(mask_nms_th) becomes at the ABI
    n_nms = len(ths_nms)
    max_words, max_pts = max(d['words'] for d in sc), max(d['n_pts'] for d in sc)
    for ci, cth in enumerate(grid.cluster_th):
        c = _ClusterStage()
        found = mask_stages.clusters(sc, float(cth))
        c.rs = [r for r, _, _ in found]
        c.cl = [dict(K=int(r.k), conf=conf.copy(), reps=reps.copy(), ks=mask_stages.score_prefixes(conf, grid.score_th))
                for r, conf, reps in found]
        for t, cl_ in zip(tabs, c.cl):
            t.clusters.append(cl_)
            t.stages.append([])
        c.ci, c.dev, c.n_class, c.ths_nms, c.n_nms, c.max_words, c.max_pts = ci, dev, n_class, ths_nms, n_nms, max_words, max_pts
        # rows no setting can keep are never projected: the prefix of the SMALLEST score_th (the grid is ascending)
        c.table = tab = mask_stages.MaskTable(sc, [r.heat for r in c.rs], [np.arange(int(cl_['ks'][0])) for cl_ in c.cl], dev)
        c.ksels, c.total, c.row0, c.bits_ptr = tab.ksels, tab.total, tab.row0, tab.bits_ptr
        # every result of a stage in ONE int32 buffer -- keep flags | labels | the scorer's tail -- and one host read of it
        c.o_lab, c.o_tail = n_nms * c.total, n_nms * c.total + c.total
        n_tail, fill = tail(c, sc)
        c.res = torch.zeros(max(c.o_tail + n_tail, 1), dtype=torch.int32, device=dev)
        tab.set_kept(c.ksels, 0, c.res.data_ptr() + 4 * c.o_lab)             # every projected row gets its label
        extra, c.alive = fill(c.res)
        c.desc_ptr, c.extra_ptr = tab.upload(extra)
        yield c


# ----------------------------------------------------------------------------------------------------------------- detection mAP
class DetectionTables:
    """What every setting of the grid needs of ONE scene to be scored with the oriented-box detection mAP, as host arrays.

    clusters[ci]:    as ``SweepTables``;
    gt_label (g,):   the classes of the scene's ground-truth boxes, in label order;
    stages[ci][bi]:  label_id (K',) int32, keep (n_nms, K') bool, count (K',) int64 = scene POINTS in the row's mask, iou (K', g)
                     float64 = box3d_iou (calc_iou without oriented boxes) of the row's prism with every same-class box, zero
                     elsewhere and in the rows under ``min_points`` points; K' = ks[0]."""
    __slots__ = ('name', 'n_pts', 'gt_label', 'min_points', 'clusters', 'stages')

    def __init__(self, name, n_pts, gt_label, min_points):
        self.name, self.n_pts, self.gt_label, self.min_points = name, n_pts, gt_label, min_points
        self.clusters, self.stages = [], []


def _detection_rows(tables, ci, si, bi, mi):
    rows = compose(tables, ci, si, bi, mi)
    return rows[tables.stages[ci][bi]['count'][rows] >= tables.min_points]


def detection_records(tables, ci, si, bi, mi):
    """The scene's ``{'label', 'conf', 'gt_label', 'iou'}`` record of one setting, as ``eval_detection.eval_det`` takes it: the rows
    of ``compose`` with at least ``min_points`` points (evaluation.py:279-281: the gate comes after the mask NMS), in prediction
    order."""
    st = tables.stages[ci][bi]
    rows = _detection_rows(tables, ci, si, bi, mi)
    return {'label': st['label_id'][rows], 'conf': tables.clusters[ci]['conf'][rows], 'gt_label': tables.gt_label, 'iou': st['iou'][rows]}


def _hull_tail(hs, cap):
    """The scorer's part of a cluster stage for the detection mAP.  Behind the labels: flags | n_hull | ncand | count (``total``
    int32 each), then, 8-byte aligned, the IoU tables of the scenes (k x g doubles each).  The B2M_HULLIDX_DESC table."""
    def tail(c, sc):
        c.o_side = c.o_tail
        c.o_iou = c.o_tail + 4 * c.total
        c.o_iou += c.o_iou & 1
        c.scr = [dict(pbits=torch.empty(max(k * ((d['n_pts'] + 63) // 64), 1), dtype=torch.int64, device=c.dev),
                      work=torch.empty(max(k, 1) * eval_detection.HULL_CHUNKS * eval_detection.HULL_PART, dtype=torch.float64, device=c.dev),
                      box6=torch.empty((max(k, 1), 6), dtype=torch.float64, device=c.dev),
                      hull=torch.empty((max(k, 1), eval_detection.HULL_MAX, 2), dtype=torch.float64, device=c.dev))
                 for k, d in zip(c.ksels, sc)]
        return c.o_iou - c.o_tail + 2 * sum(k * h['g'] for k, h in zip(c.ksels, hs)), lambda res: _hull_desc(c, sc, hs, cap)
    return tail


def _hull_desc(c, sc, hs, cap):
    """B2M_HULLIDX_DESC table of a cluster stage with candidate buffers for ``cap`` (flat int64), and the buffers."""
    dev = c.dev
    cand = [torch.empty((max(k, 1), cap, 2), dtype=torch.float64, device=dev) for k in c.ksels]
    stk = [torch.empty((max(k, 1), cap), dtype=torch.int32, device=dev) for k in c.ksels]
    rec = np.zeros((len(sc), 17), np.int64)
    side = lambda j, r0: c.res.data_ptr() + 4 * (c.o_side + j * c.total + r0)
    for s_, (d, h, k, q) in enumerate(zip(sc, hs, c.ksels, c.scr)):
        r0 = c.row0[s_]
        rec[s_] = (c.bits_ptr[s_], k, d['words'], d['n_vox'], d['v2p'].data_ptr(), h['pos'].data_ptr(), d['n_pts'], q['pbits'].data_ptr(),
                   q['work'].data_ptr(), cand[s_].data_ptr(), stk[s_].data_ptr(), side(2, r0), side(3, r0), q['box6'].data_ptr(),
                   q['hull'].data_ptr(), side(1, r0), side(0, r0))
    return rec.reshape(-1), (cand, stk)


def detection_tables(net, batch, pred, cfg, grid, positions=None, labels=None, oriented_boxes=True,
                     min_points=eval_detection.MIN_POINTS, cap=eval_detection.DEFAULT_CAP):
    """``SelectionNet.detection2mask_detection_sweep``: one ``DetectionTables`` per scene of the batch.

    positions: per scene (n_pts, 3), default ``batch['scene'][i]['positions']``; labels: per scene the ``per_instance_bb_*`` dict
    ``eval_detection.gt_boxes`` takes, default ``batch['labels']``.  The prism of a projected row -- its point count, z range and
    x-y hull -- and its IoU with the ground-truth boxes depend on (cluster_th, mask_bin_th) alone: one ``b2m_mask_hulls_index_batch``
    and one IoU call per scene for each such stage, and ONE host read of the stage (keep flags, labels, hull flags, counts and the
    IoU tables together).  A filled candidate buffer redoes the stage's hulls once with the capacity ``check_flags`` asks for; a
    hull beyond B2M_HULL_MAX vertices in a row some setting keeps raises B2MError."""
    _lib.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    sc = _scannet_inputs(net, batch, pred, cfg, dev)
    if not sc:
        return []
    if cap < 64 or cap & (cap - 1):
        raise ValueError('cap: a power of two >= 64, got %r' % (cap,))
    S = len(sc)
    n_class = int(max(int(net.semantic_valid_class_ids.max()) + 1, 1))
    if labels is None:
        labels = batch.get('labels')
    if labels is None or len(labels) != S:
        raise ValueError('the detection mAP needs the ground-truth boxes of every scene (labels / batch[\'labels\'])')
    hs, tabs = [], []
    for d in sc:
        lab = labels[d['idx']]
        if not isinstance(lab, dict) or any(k not in lab for k in ('per_instance_bb_centers', 'per_instance_bb_bounds', 'per_instance_semantics')):
            raise ValueError('%s: labels without boxes (per_instance_bb_centers / _bounds, per_instance_semantics)' % d['name'])
        p = positions[d['idx']] if positions is not None else batch['scene'][d['idx']].get('positions')
        if p is None:
            raise ValueError('%s: no positions' % d['name'])
        p = eval_detection._f64(p, dev)
        if p.dim() != 2 or tuple(p.shape) != (d['n_pts'], 3):
            raise ValueError('%s: positions %s for %d points' % (d['name'], tuple(p.shape), d['n_pts']))
        gt = eval_detection.gt_boxes(lab)                                  # once per scene
        hs.append(dict(pos=p, gt=gt, g=gt['g']))
        tabs.append(DetectionTables(d['name'], d['n_pts'], gt['label'], min_points))
    for c in _cluster_stages(sc, grid, dev, tabs, n_class, _hull_tail(hs, cap)):
        total, res = c.total, c.res
        n_iou = sum(k * h['g'] for k, h in zip(c.ksels, hs))
        iou_all = res[c.o_iou:c.o_iou + 2 * n_iou].view(torch.float64)
        label_dev, count_dev = res[c.o_lab:c.o_lab + total], res[c.o_side + 3 * total:c.o_side + 4 * total]

        def score(desc_ptr, cap_):
            _call('b2m_mask_hulls_index_batch', desc_ptr, S, cap_, max(c.ksels), c.max_pts)
            cls = torch.where(count_dev >= min_points, label_dev, torch.full_like(label_dev, -1))     # evaluation.py:279-281
            ioff = 0
            for s_, (h, k, q) in enumerate(zip(hs, c.ksels, c.scr)):
                g, gt, r0 = h['g'], h['gt'], c.row0[s_]
                if k and g:
                    out = iou_all[ioff:ioff + k * g]
                    side = lambda j: res.data_ptr() + 4 * (c.o_side + j * total + r0)
                    if oriented_boxes:
                        _call('b2m_hull_box_iou', q['hull'].data_ptr(), side(1), q['box6'].data_ptr(), cls[r0:r0 + k].data_ptr(), k,
                              gt['boxes'].data_ptr(), gt['cls'].data_ptr(), g, out.data_ptr())
                    else:
                        _call('b2m_aabb_iou', q['box6'].data_ptr(), cls[r0:r0 + k].data_ptr(), k, gt['centers'].data_ptr(),
                              gt['boxes'].data_ptr(), gt['cls'].data_ptr(), g, out.data_ptr())
                ioff += k * g
            return res.cpu().numpy()                                       # the one host read of the stage

        def need_of(host):
            """0, or the candidate capacity a second pass needs; rows no setting keeps are not looked at."""
            if not oriented_boxes or not total:
                return 0
            used = host[:c.n_nms * total].reshape(c.n_nms, total).any(0)
            side = host[c.o_side:c.o_side + 4 * total].reshape(4, total)
            return eval_detection.check_flags(np.where(used, side[0], 0), side[1], np.where(used, side[2], 0))

        for bi, bth in enumerate(grid.mask_bin_th):
            c.shared(bth)
            host = score(c.extra_ptr, cap) if total else res.cpu().numpy()
            need = need_of(host)
            if need:                                                       # once more, with room for every candidate
                rec, alive = _hull_desc(c, sc, hs, need)
                again = torch.from_numpy(rec).to(dev)
                host = score(again.data_ptr(), need)
                if need_of(host):
                    raise _lib.B2MError('hull candidates still exceed the buffer (%d)' % need)
                del alive
            iou_host = host[c.o_iou:c.o_iou + 2 * n_iou].view(np.float64)
            ioff = 0
            for s_, (t, h, k) in enumerate(zip(tabs, hs, c.ksels)):
                keep, label = c.split(host, s_)
                r0 = c.o_side + 3 * total + c.row0[s_]
                t.stages[-1].append(dict(label_id=label, keep=keep, count=host[r0:r0 + k].astype(np.int64),
                                         iou=iou_host[ioff:ioff + k * h['g']].reshape(k, h['g']).copy()))
                ioff += k * h['g']
    return tabs


def arkit_param_search(model, batches, grid, oriented_boxes=True, iou_t=0.5, per_class=False):
    """Score every setting of ``grid`` with the ARKitScenes detection mAP (``eval_detection.arkitscenes_eval``) over all ``batches``.

    batches: an iterable of batch dicts or ``(batch, pred)`` pairs; the scenes carry ``positions`` and ``batch['labels']`` the
    boxes, as the reference's ARKitScenes loader returns them.  Returns dict(map (nc, ns, nb, nm), with a trailing axis when
    ``iou_t`` is a sequence (the records do not depend on it); best = the setting with the largest mAP (of the first ``iou_t``),
    NaN last, then grid order; best_ths; n_evaluated = the number of DISTINCT record sets matched; with per_class, ap_by_class =
    {setting: {class id: AP}} (a tuple of such per ``iou_t`` for a sequence)).  Matching and the VOC AP are the unchanged
    ``eval_detection.eval_det``, once per distinct record set."""
    shape = grid.shape
    settings = list(grid.settings())
    many = not np.isscalar(iou_t)
    ths = [float(v) for v in (iou_t if many else [iou_t])]
    if not ths:
        raise ValueError('iou_t: a threshold or a non-empty sequence of thresholds')
    recs = {st: {} for st in settings}
    keys = {st: [] for st in settings}
    for batch, pred in _predicted(model, batches):
        for t in model.pred2mask_detection_sweep(batch, pred, grid, oriented_boxes=oriented_boxes):
            for st in settings:
                recs[st][t.name] = detection_records(t, *st)
                # two settings whose scenes score the same rows of the same (cluster_th, mask_bin_th) stage have the same records
                keys[st].append((t.name, st[0], st[2], _detection_rows(t, *st).tobytes()))
    out_map = np.full(shape + (len(ths),), np.nan)
    by_class, done = {}, {}
    for st in settings:
        key = tuple(keys[st])
        if key not in done:
            aps = [eval_detection.eval_det(recs[st], ovthresh=th)[2] for th in ths]
            done[key] = (aps, [float(eval_detection.mean_ap(ap)) for ap in aps])
        aps, means = done[key]
        out_map[st] = means
        by_class[st] = tuple(aps) if many else aps[0]
    best = _best(settings, lambda st: (out_map[st][0],))
    out = dict(map=out_map if many else out_map[..., 0], best=best, best_ths=grid.eval_ths(*best), n_evaluated=len(done))
    if per_class:
        out['ap_by_class'] = by_class
    return out


def _match_stage(acc, grid, ci, bi, tabs, sc, cl, ksels, conf_dev, res, n_nms, total, o_lab, o_hist):
    """The (score_th, mask_nms_th) settings of stage (ci, bi) into ``acc``, straight from the stage's ``res`` buffer: setting
    (si, mi) keeps row r of a scene iff r < ks[si] and flag row mi is set there."""
    _, ns, nb, nm = grid.shape
    pairs = [(si, mi) for si in range(ns) for mi in range(nm)]
    set_id = [((ci * ns + si) * nb + bi) * nm + mi for si, mi in pairs]
    prefix = [[int(c['ks'][si]) for si, _ in pairs] for c in cl]
    scenes, row0, hoff = [], 0, 0
    for t, d, k, cf in zip(tabs, sc, ksels, conf_dev):
        scenes.append(dict(inter=res[o_hist + hoff:o_hist + hoff + k * d['G']].view(k, d['G']), label_id=res[o_lab + row0:o_lab + row0 + k],
                           conf=cf, uniq=t.uniq, gt_vert=t.gt_vert, row0=row0))
        row0 += k; hoff += k * d['G']
    keep = res[:n_nms * total].view(n_nms, total) if total else None
    acc.add(scenes, set_id, prefix, keep, [mi if total else -1 for _, mi in pairs])


def materialize(net, batch, pred, cfg, grid, tables, ci, si, bi, mi):
    """The ordinary ``{scene: {'conf', 'label_id', 'mask'}}`` of ``detection2mask(..., 'eval')`` for ONE setting, masks on points:
    the chosen rows are projected and gathered again (for the tests, and for the masks of the winning setting)."""
    _lib.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    sc = _scannet_inputs(net, batch, pred, cfg, dev)
    rs = iou_nms.nmc_device_batch([d['boxes'] for d in sc], float(grid.cluster_th[ci])) if sc else []
    by_name = {t.name: t for t in tables}
    out = {}
    for d, r in zip(sc, rs):
        t = by_name[d['name']]
        rows = compose(t, ci, si, bi, mi)
        if r.k != t.clusters[ci]['K']:
            raise ValueError('%s: these tables were not made from this batch and these predictions' % d['name'])
        mask = mask_stages.project_gather(d, r.heat, torch.from_numpy(rows.astype(np.int32)).to(dev), len(rows), grid.mask_bin_th[bi])
        out[d['name']] = {'conf': torch.from_numpy(t.clusters[ci]['conf'][rows]).to(d['pdev']),
                          'label_id': t.stages[ci][bi]['label_id'][rows].astype('int32'), 'mask': mask.bool().to(d['pdev'])}
    return out


# ----------------------------------------------------------------------------------------------------------------- the search
def _predicted(model, batches, clock=contextlib.nullcontext):
    """(batch, pred) of every item of ``batches``: a pair as it is, a batch dict predicted here (inside ``clock('forward')``)."""
    for item in batches:
        with clock('forward'):
            pair = item if isinstance(item, (tuple, list)) else \
                (item, model.get_prediction(item, with_grad=False, to_cpu=True, min_size=True))
        yield pair


def _best(settings, key):
    """The setting with the largest ``key(st)`` (a tuple of figures, a NaN counts as -inf); ties go to the first in grid order."""
    rank = lambda st: tuple(-np.inf if np.isnan(v) else v for v in key(st))
    return max(settings, key=lambda st: (rank(st), tuple(-i for i in st)))


def _averages(aps):
    """(AP, AP50, AP25) of an ``evaluate_matches`` table through the unchanged ``eval_metric.compute_averages``."""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)                     # (no class with ground truth: nanmean of nothing)
        avg = eval_metric.compute_averages(aps)
    return avg['all_ap'], avg['all_ap_50%'], avg['all_ap_25%']


def scannet_param_search(model, batches, gt_ids_by_scene, grid, per_class=False, matching='host'):
    """Score every setting of ``grid`` with the ScanNet AP over all ``batches``.

    batches: an iterable of batch dicts (predicted here with ``model.get_prediction``) or of ``(batch, pred)`` pairs.
    Returns dict(ap (nc, ns, nb, nm, 3) = AP, AP50, AP25 of every setting; best = its (ci, si, bi, mi) by AP50, then AP, then grid
    order; best_ths = that setting as ``eval_ths``; n_evaluated = the number of DISTINCT record sets matched; with per_class,
    ap_tables (nc, ns, nb, nm, 1, classes, overlaps) = what ``evaluate_matches`` returned).  The matching and the AP are the
    unchanged host code of eval_metric, once per distinct record set.

    matching='device': the matching, the curves and the AP of EVERY setting on the device (box2mask_amd/eval_match.py) -- the
    stage results are never read to the host, ``compose`` and ``records`` are not called, n_evaluated = the number of settings.
    The AP of a curve of n points is then within 4 n 2^-53 of the host route's (the dot product is summed in ascending order
    of the thresholds); ``best`` follows the same ranking over the device table."""
    shape = grid.shape
    settings = list(grid.settings())
    if matching not in ('host', 'device'):
        raise ValueError("matching must be 'host' or 'device', got %r" % (matching,))
    if matching == 'device':
        return _search_device(model, batches, gt_ids_by_scene, grid, per_class, shape, settings)
    matches = {st: {} for st in settings}
    keys = {st: [] for st in settings}
    for batch, pred in _predicted(model, batches):
        for t in model.pred2mask_sweep(batch, pred, grid, gt_ids_by_scene):
            for st in settings:
                ci, si, bi, mi = st
                matches[st][t.name] = records(t, *st)
                # two settings whose scenes keep the same rows of the same (cluster_th, mask_bin_th) stage have the same records
                keys[st].append((t.name, ci, bi, compose(t, *st).tobytes()))
    ap = np.full(shape + (3,), np.nan)
    ap_tables = np.full(shape + (1, len(eval_metric.CLASS_LABELS), len(eval_metric.OVERLAPS)), np.nan) if per_class else None
    done = {}
    for st in settings:
        key = tuple(keys[st])
        if key not in done:
            aps, _ = eval_metric.evaluate_matches(matches[st])
            done[key] = (aps, _averages(aps))
        aps, three = done[key]
        ap[st] = three
        if per_class:
            ap_tables[st] = aps
    best = _best(settings, lambda st: (ap[st][1], ap[st][0]))
    out = dict(ap=ap, best=best, best_ths=grid.eval_ths(*best), n_evaluated=len(done))
    if per_class:
        out['ap_tables'] = ap_tables
    return out


def _search_device(model, batches, gt_ids_by_scene, grid, per_class, shape, settings):
    from . import eval_match
    acc = eval_match.MatchAccumulator(len(settings))
    for batch, pred in _predicted(model, batches):
        model.pred2mask_sweep(batch, pred, grid, gt_ids_by_scene, acc=acc)
    table = acc.finish()                                                   # (settings, classes, overlaps), grid order
    ap = np.full(shape + (3,), np.nan)
    for q, st in enumerate(settings):
        ap[st] = _averages(table[q:q + 1])
    best = _best(settings, lambda st: (ap[st][1], ap[st][0]))
    out = dict(ap=ap, best=best, best_ths=grid.eval_ths(*best), n_evaluated=len(settings))
    if per_class:
        out['ap_tables'] = table.reshape(shape + (len(eval_metric.CLASS_LABELS), len(eval_metric.OVERLAPS)))[..., None, :, :].copy()
    return out


# ----------------------------------------------------------------------------------------------------------------- S3DIS mPrec / mRec
class S3DISSweepResult(dict):
    """The dict ``s3dis_param_search`` returns, with ``best``."""

    def best(self, criterion='f1'):
        """The setting with the largest harmonic mean of mPrec and mRec, as a ``cfg.eval_ths`` list (mask_nms_th = the grid's
        first value: it has no effect in this flow).  A NaN counts as -inf; ties go to the first setting in grid order.  The
        reference's search only prints the metrics of every job; this choice is this project's own."""
        if criterion != 'f1':
            raise ValueError("criterion: only 'f1' (the harmonic mean of mPrec and mRec) is defined, got %r" % (criterion,))
        p, r = self['mprec'], self['mrec']
        with np.errstate(all='ignore'):
            f1 = 2.0 * p * r / (p + r)
        f1 = np.where(np.isnan(f1), -np.inf, f1)
        ci, si, bi = (int(v) for v in np.unravel_index(int(np.argmax(f1.reshape(-1))), f1.shape))     # argmax: the first of equals
        return self['grid'].eval_ths(ci, si, bi, 0)


def _s3dis_room(net, batch, pred, cfg, dev):
    """``mask_stages.scene_inputs`` with the points for a batch of ONE room of the S3DIS flow: the boxes of the segments whose voxels
    vote a foreground class, their slots, and the predicted class of every point (``sem_pts``)."""
    if not net.requires_voxel_outputs or cfg.mlp_per_vox_semantics not in cfg.network_heads:
        raise ValueError('s3dis_param_search needs the per-voxel semantics head (%s); the ScanNet / ARKitScenes flows are swept by '
                         'scannet_param_search / arkit_param_search' % cfg.mlp_per_vox_semantics)
    if len(batch['scene']) != 1:
        raise ValueError('S3DIS is evaluated with batch size 1 (evaluation.py:131)')
    return mask_stages.scene_inputs(net, batch, pred, cfg, dev, points=True)[0]


def s3dis_stage(d, r, k_rows, mask_bin_th, clock=contextlib.nullcontext):
    """One (cluster_th, mask_bin_th) stage of one room: the first k_rows clusters of ``r`` projected on the voxels, gathered to
    the points, their classes (13-class vote on the points) and ONE greedy merge.  Returns (owner int32 (n_pts): the row that took
    the point or -1, prop_sem int32 (k_rows), accepted int32 (k_rows), masks uint8 (k_rows, n_pts)), all on the device.
    clock(name): a context manager around the 'projection' (project, gather, pack, vote) and the 'paint' part."""
    from . import eval_s3dis as S
    dev = d['boxes'].device
    n = d['n_pts']
    pwords = (n + 63) // 64
    with clock('projection'):
        masks = mask_stages.project_gather(d, r.heat, torch.arange(max(k_rows, 1), dtype=torch.int32, device=dev), k_rows, mask_bin_th)
        pbits = torch.empty((max(k_rows, 1), max(pwords, 1)), dtype=torch.int64, device=dev)
        prop_sem = torch.zeros(max(k_rows, 1), dtype=torch.int32, device=dev)
        if k_rows:
            _call('b2m_mask_pack', masks.data_ptr(), k_rows, n, pbits.data_ptr(), pwords)
            _call('b2m_label_hist', pbits.data_ptr(), pwords, None, k_rows, d['sem_pts'].data_ptr(), n, S.NUM_CLASSES, prop_sem.data_ptr())
    with clock('paint'):
        inst = torch.empty(n, dtype=torch.int32, device=dev)
        accepted = torch.zeros(max(k_rows, 1), dtype=torch.int32, device=dev)
        unlabeled = torch.empty(max(pwords, 1), dtype=torch.int64, device=dev)
        _call('b2m_paint_proposals', pbits.data_ptr(), pwords, k_rows, prop_sem.data_ptr(), n, S.SEM_MIN, S.KEEP_RATIO, S.MIN_POINTS,
              unlabeled.data_ptr(), inst.data_ptr(), None, accepted.data_ptr())
        owner = torch.where(inst > 0, inst - 1, torch.full_like(inst, -1)).contiguous()
    return owner, prop_sem[:k_rows], accepted[:k_rows], masks


def s3dis_prefix_tail(owner, prop_sem, bg, sem, ks, n_inst, gi, gt_class, gt_size, tp, fp, index=None, min_points=None, label_setting=-1):
    """b2m_s3dis_prefix_tail: the true / false positives of every prefix length of ``ks`` are ADDED to tp / fp (int32 (S, 13), device).
    gt_size (G) int32: the evaluation points of every ground-truth instance (``_s3dis_ground_truth`` counts them once per room).
    label_setting >= 0: also returns that setting's (instances, semantics) at the evaluation points."""
    from . import eval_s3dis as S
    dev = owner.device
    ks = np.ascontiguousarray(ks, np.int32)
    n, n_eval = int(owner.shape[0]), int(gi.shape[0])
    k_rows, n_gt = int(prop_sem.shape[0]), int(gt_class.shape[0])
    size = _lib.load().b2m_s3dis_prefix_tail_workspace(k_rows, len(ks), int(n_inst), n_gt) if 1 <= len(ks) <= 64 else 0
    if size < 0:
        raise _lib.B2MError('b2m_s3dis_prefix_tail: %d settings x %d instances x %d ground-truth instances exceed the tables (%d entries)'
                            % (len(ks), n_inst, n_gt, S.JOINT_HIST_MAX))
    work = torch.empty(max(size // 4, 1), dtype=torch.int32, device=dev)
    inst_out = sem_out = None
    if label_setting >= 0:
        inst_out = torch.full((n_eval,), -1, dtype=torch.int32, device=dev)
        sem_out = torch.full((n_eval,), -1, dtype=torch.int32, device=dev)
    _call('b2m_s3dis_prefix_tail', owner.data_ptr(), prop_sem.data_ptr() if k_rows else None, k_rows, bg.data_ptr(), sem.data_ptr(), n,
          ks.ctypes.data, len(ks), int(n_inst), int(S.MIN_POINTS if min_points is None else min_points), gi.data_ptr(),
          gt_class.data_ptr() if n_gt else None, gt_size.data_ptr() if n_gt else None, n_gt,
          None if index is None else index.data_ptr(), n_eval, work.data_ptr(),
          tp.data_ptr(), fp.data_ptr(), int(label_setting), None if inst_out is None else inst_out.data_ptr(),
          None if sem_out is None else sem_out.data_ptr())
    return (inst_out, sem_out) if label_setting >= 0 else None


def _s3dis_ground_truth(labels, dev):
    """Dense index of the ground-truth instance of every evaluation point (ascending ids), the class of every instance (most
    frequent, lowest on ties: scipy.stats.mode, s3dis_util.py:233-238), its points and the instances per class -- once per room, on the
    device."""
    from . import eval_s3dis as S
    g_ins, g_sem = S._i32(labels['instances'], dev).reshape(-1), S._i32(labels['semantics'], dev).reshape(-1)
    vals, gi = S._dense(g_ins)
    G = int(vals.numel())
    if G == 0:
        none = torch.zeros(0, dtype=torch.int32, device=dev)
        return gi, none, none, torch.zeros(S.NUM_CLASSES, dtype=torch.int64, device=dev)
    hist = S.joint_hist(gi, g_sem, G, S.NUM_CLASSES).long()
    key = hist * 16 + (15 - torch.arange(S.NUM_CLASSES, device=dev))       # distinct per row: the largest count, then the lowest class
    gt_class = key.argmax(1).int().contiguous()
    gt_size = S.joint_hist(gi, None, G)[:, 0].contiguous()
    return gi, gt_class, gt_size, torch.bincount(gt_class.long(), minlength=S.NUM_CLASSES)[:S.NUM_CLASSES]


def _stage_clock(timing):
    """clock(name): a context manager that adds the device milliseconds of its body to ``timing[name]`` (HIP events; it waits for
    the second one, so a timed search is a pass of its own)."""
    @contextlib.contextmanager
    def clock(name):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        yield
        b.record()
        b.synchronize()
        timing[name] = timing.get(name, 0.0) + a.elapsed_time(b)
    return clock


def s3dis_param_search(model, batches, grid, full_rooms=None, per_class=False, timing=None):
    """Score every setting of ``grid`` with the S3DIS instance metric (mPrec / mRec, ``eval_s3dis.evaluate_rooms``) over all
    ``batches`` of ONE room each (batch dicts, predicted here, or ``(batch, pred)`` pairs).

    Per room: one forward, one ``clustering_for_background`` (the wall DBSCAN depends on no threshold), the ground-truth tables;
    per cluster_th one clustering; per (cluster_th, mask_bin_th) one projection + point gather + class vote + ``b2m_paint_proposals``
    over the rows of the smallest score_th (``s3dis_stage``), then ``b2m_s3dis_prefix_tail`` for all score settings.  tp / fp /
    total_gt accumulate over the rooms on the device and come to the host in ONE read at the end.  Sizes still cross per room and
    per cluster_th, as on the one-setting route: the number of wall clusters and the largest background id (they size the tables),
    and the clusters' scores, from which the prefix lengths are taken on the host.

    ``grid.mask_nms_th`` is accepted and IGNORED: this flow has no mask NMS (detection_net.py:449-451), every value gives the same
    result.  With ``cfg.full_resolution`` the unsampled rooms come through ``full_rooms`` as for ``evaluate_rooms``.

    Returns an ``S3DISSweepResult``: mprec, mrec (n_cluster, n_score, n_bin) float64 -- the same float64 divisions and np.mean as
    the reference, 0 / 0 is NaN; grid; with per_class also precision, recall (..., 13) and the integer tables tp, fp (..., 13),
    total_gt (13).  ``.best()`` picks a setting.  timing (for tools/bench_param_sweep.py): a dict that receives the device milliseconds
    per stage; such a search waits after every stage."""
    from . import eval_s3dis as S
    cfg = model.cfg
    net = model.detection_model
    full = bool(getattr(cfg, 'full_resolution', False))
    if full and full_rooms is None:
        raise NotImplementedError('s3dis_param_search: cfg.full_resolution needs the unsampled rooms: pass full_rooms= (a sequence '
                                  'aligned with the batches of (scene_full, labels_full), or a callable name -> (scene_full, labels_full))')
    _lib.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    nc, ns, nb, _ = grid.shape
    tp = torch.zeros((nc, nb, ns, S.NUM_CLASSES), dtype=torch.int32, device=dev)
    fp = torch.zeros_like(tp)
    total_gt = torch.zeros(S.NUM_CLASSES, dtype=torch.int64, device=dev)

    clock = _stage_clock(timing) if timing is not None else contextlib.nullcontext
    for i, (batch, pred) in enumerate(_predicted(model, batches, clock)):
        d = _s3dis_room(net, batch, pred, cfg, dev)
        scene, labels = batch['scene'][0], batch['labels'][0]
        with clock('dbscan'):
            bg = S.clustering_for_background(d['sem_pts'], scene['positions'], scene['normals']).contiguous()
        index = None
        if full:
            scene_full, labels = full_rooms(scene['name']) if callable(full_rooms) else full_rooms[i]
            index = S.sparse2dense(scene_full['positions'], scene['positions']).contiguous()
        gi, gt_class, gt_size, per_class_gt = _s3dis_ground_truth(labels, dev)
        if gi.shape[0] != (d['n_pts'] if index is None else index.shape[0]):
            raise ValueError('%s: %d ground-truth labels for %d evaluation points' % (d['name'], gi.shape[0],
                                                                                    d['n_pts'] if index is None else index.shape[0]))
        total_gt += per_class_gt
        bg_top = int(bg.max().item()) if d['n_pts'] else 0
        for ci, cth in enumerate(grid.cluster_th):
            with clock('clustering'):
                (r, conf, _), = mask_stages.clusters([d], float(cth))
            ks = mask_stages.score_prefixes(conf, grid.score_th)
            k_rows = int(ks[0])
            for bi, bth in enumerate(grid.mask_bin_th):
                owner, prop_sem, _, _ = s3dis_stage(d, r, k_rows, bth, clock=clock)
                with clock('tail'):
                    s3dis_prefix_tail(owner, prop_sem, bg, d['sem_pts'], ks, k_rows + max(bg_top, 0) + 1, gi, gt_class, gt_size, tp[ci, bi],
                                      fp[ci, bi], index=index)
    host = torch.cat([tp.reshape(-1).long(), fp.reshape(-1).long(), total_gt]).cpu().numpy()          # the one host read
    m = nc * nb * ns * S.NUM_CLASSES
    tp_h = host[:m].reshape(nc, nb, ns, S.NUM_CLASSES).transpose(0, 2, 1, 3).copy()
    fp_h = host[m:2 * m].reshape(nc, nb, ns, S.NUM_CLASSES).transpose(0, 2, 1, 3).copy()
    gt_h = host[2 * m:]
    precision, recall = np.zeros(tp_h.shape), np.zeros(tp_h.shape)
    mprec, mrec = np.zeros(tp_h.shape[:3]), np.zeros(tp_h.shape[:3])
    with np.errstate(all='ignore'):
        for st in itertools.product(range(nc), range(ns), range(nb)):      # s3dis_util.py:308-320, :338, setting by setting
            t, f = tp_h[st].astype(np.float64), fp_h[st].astype(np.float64)
            recall[st] = t / gt_h.astype(np.float64)
            precision[st] = t / (t + f)
            mprec[st], mrec[st] = np.mean(precision[st]), np.mean(recall[st])
    out = S3DISSweepResult(mprec=mprec, mrec=mrec, grid=grid)
    if per_class:
        out.update(precision=precision, recall=recall, tp=tp_h, fp=fp_h, total_gt=gt_h)
    return out
