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
``eval_metric`` per setting.  ScanNet flow only (segment-level votes, mask NMS, the AP of eval_metric.py): that is what the
reference's search scores.  ``compose`` and the matching are host logic like ``assign_from_counts``; every kernel stage is HIP.
With ``matching='device'`` the matching, the curves and the AP run on the device as well (eval_match.py): the stage results are
matched where they lie and nothing but an entry count per stage comes to the host.
"""
from __future__ import annotations

import itertools
import warnings

import numpy as np
import torch

from . import _lib
from . import eval_metric
from . import iou_nms
from .util import to_bbs_min_max

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
def _scene_inputs(net, batch, pred, cfg, dev):
    """Stage 0 of ``SelectionNet.detection2mask`` in the ScanNet flow: boxes of the foreground votes, their slots, the voxel labels."""
    if net.requires_voxel_outputs:
        raise ValueError('the threshold sweep covers the ScanNet flow only (segment-level votes, mask NMS): a network with a '
                         'per-voxel semantics head (requires_voxel_outputs) has no mask NMS to sweep')
    pdev = pred[cfg.mlp_offsets].device
    pred_bbs = to_bbs_min_max(batch['input_location'].to(pdev), pred[cfg.mlp_offsets], pred[cfg.mlp_bounds],
                              torch.nn.Sigmoid()(pred[cfg.mlp_bb_scores]))
    pred_semantics = torch.argmax(pred[cfg.mlp_semantics], 1)
    pred_semantics = net.semantic_valid_class_ids.to(pdev)[pred_semantics].long()
    batch_ids = batch['batch_ids'].to(pdev)
    sc = []
    for scene_idx, scene in enumerate(batch['scene']):
        scene_mask = batch_ids == scene_idx
        if cfg.do_segment_pooling:
            seg2vox = torch.as_tensor(batch['seg2vox'][scene_idx]).long()
        else:
            seg2vox = torch.arange(int(scene_mask.sum()), dtype=torch.long)
        n_vox = seg2vox.shape[0]
        s2v = seg2vox.to(dev)
        scene_sem = pred_semantics[scene_mask]
        fg = net.is_foreground(scene_sem)
        boxes = pred_bbs[scene_mask][fg].detach().to(dev, torch.float32).contiguous()
        if boxes.shape[0] == 0:
            raise ValueError('NMS_clustering needs at least one box (the reference raises on n == 0 as well)')
        fg_dev = fg.to(dev)
        fg_slot = torch.where(fg_dev, torch.cumsum(fg_dev.int(), 0) - 1, torch.full_like(fg_dev.int(), -1)).int()
        v2p = torch.as_tensor(batch['vox2point'][scene_idx]).long().to(dev).contiguous()
        sc.append(dict(name=scene['name'], idx=scene_idx, s2v=s2v, n_vox=n_vox, sem32=scene_sem.to(dev)[s2v].int().contiguous(),
                       fg_slot=fg_slot, boxes=boxes, n_fg=int(boxes.shape[0]), words=(n_vox + 63) // 64, v2p=v2p,
                       n_pts=int(v2p.shape[0]), pdev=pdev))
    return sc


def _cluster(sc, cluster_th, score_ths):
    """Clusters of every scene for one cluster_th (one launch, two host reads for the batch): per scene the device result and
    dict(K, conf, reps, ks)."""
    rs = iou_nms.nmc_device_batch([d['boxes'] for d in sc], float(cluster_th))
    rep_scores = torch.cat([d['boxes'][r.reps[:r.k].long(), 0] for d, r in zip(sc, rs)]).cpu().numpy()
    reps_host = torch.cat([r.reps[:r.k] for r in rs]).cpu().numpy().astype(np.int64)
    out, o = [], 0
    for r in rs:
        conf, reps = rep_scores[o:o + r.k], reps_host[o:o + r.k]
        o += r.k
        ks = np.zeros(len(score_ths), np.int64)
        for si, th in enumerate(score_ths):
            sel = np.nonzero(conf > np.float32(th))[0]                     # detection_net.py:427-432, as detection2mask filters
            if not np.array_equal(sel, np.arange(len(sel))):
                raise ValueError('the score filter did not keep a prefix of the clusters (NaN scores?)')
            ks[si] = len(sel)
        out.append(dict(K=int(r.k), conf=conf.copy(), reps=reps.copy(), ks=ks))
    return rs, out


def sweep_tables(net, batch, pred, cfg, grid, gt_ids, acc=None):
    """``SelectionNet.detection2mask_sweep``: one ``SweepTables`` per scene of the batch.  gt_ids: {scene name: (n_pts,) ids
    ``label*1000 + instance``} or a list in scene order.

    With ``acc`` (an ``eval_match.MatchAccumulator`` over all ``grid.settings()`` in grid order) the results of a stage are not
    read to the host: its keep flags, labels and point histograms are matched where they lie, for the n_score x n_nms settings
    of the stage in one launch, and the tables come back with ``clusters`` only (``stages`` stay empty lists)."""
    _lib.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    sc = _scene_inputs(net, batch, pred, cfg, dev)
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
    ths_nms = np.ascontiguousarray(grid.mask_nms_th, np.float32)           # C float, as float(mask_nms_th) becomes at the ABI
    n_nms = len(ths_nms)
    max_words, max_pts = max(d['words'] for d in sc), max(d['n_pts'] for d in sc)
    for cth in grid.cluster_th:
        rs, cl = _cluster(sc, cth, grid.score_th)
        for t, c in zip(tabs, cl):
            t.clusters.append(c)
            t.stages.append([])
        ci = len(tabs[0].clusters) - 1
        if acc is not None:                                                # the scores of the clusters, where the matching reads them
            conf_dev = [d['boxes'][r.reps[:r.k].long(), 0].contiguous() for d, r in zip(sc, rs)]
        # rows no setting can keep are never projected: the prefix of the SMALLEST score_th (the grid is ascending)
        ksels = [int(c['ks'][0]) for c in cl]
        total = sum(ksels)
        sel_all = torch.cat([torch.arange(k, dtype=torch.int32) for k in ksels]).to(dev) if total else \
            torch.zeros(1, dtype=torch.int32, device=dev)
        bits_all = torch.empty(max(sum(k * max(d['words'], 1) for k, d in zip(ksels, sc)), 1), dtype=torch.int64, device=dev)
        inter_all = torch.empty(max(sum(k * k for k in ksels), 1), dtype=torch.int32, device=dev)
        tb_all = torch.empty(max(sum(d['n_vox'] * ((k + 63) // 64) for k, d in zip(ksels, sc)), 1), dtype=torch.int64, device=dev)
        # every result of a stage in ONE int32 buffer -- keep flags | labels | point histograms -- and one host read of it
        n_hist = sum(k * d['G'] for k, d in zip(ksels, sc))
        o_lab, o_hist = n_nms * total, n_nms * total + total
        res = torch.zeros(max(o_hist + n_hist, 1), dtype=torch.int32, device=dev)
        desc = np.zeros((S, 20), np.int64)
        hdesc = np.zeros((S, 10), np.int64)
        row0 = boff = ioff = toff = hoff = 0
        for s_, (d, r, k) in enumerate(zip(sc, rs, ksels)):
            bits_ptr = bits_all.data_ptr() + 8 * boff
            desc[s_, 0:10] = (r.heat.data_ptr(), d['n_fg'], sel_all.data_ptr() + 4 * row0, k, d['fg_slot'].data_ptr(),
                              d['s2v'].data_ptr(), d['n_vox'], bits_ptr, d['words'], inter_all.data_ptr() + 4 * ioff)
            desc[s_, 11:15] = (0, k, d['sem32'].data_ptr(), res.data_ptr() + 4 * (o_lab + row0))      # every projected row
            desc[s_, 18:20] = (row0, row0)
            hdesc[s_] = (bits_ptr, k, d['words'], d['n_vox'], d['v2p'].data_ptr(), d['dense32'].data_ptr(), d['n_pts'], d['G'],
                         tb_all.data_ptr() + 8 * toff, res.data_ptr() + 4 * (o_hist + hoff))
            row0 += k; boff += k * max(d['words'], 1); ioff += k * k; toff += d['n_vox'] * ((k + 63) // 64); hoff += k * d['G']
        tables_dev = torch.from_numpy(np.concatenate([desc.reshape(-1), hdesc.reshape(-1)])).to(dev)
        desc_ptr, hdesc_ptr = tables_dev.data_ptr(), tables_dev.data_ptr() + 8 * S * 20
        for bi, bth in enumerate(grid.mask_bin_th):
            if total:
                _call('b2m_mask_project_batch', desc_ptr, S, total, max_words, float(bth))
                _call('b2m_mask_nms_sweep_batch', desc_ptr, S, max(ksels), ths_nms.ctypes.data, n_nms, res.data_ptr(), total)
                _call('b2m_label_hist_batch', desc_ptr, S, total, n_class)
                _call('b2m_mask_hist_index_batch', hdesc_ptr, S, max_words, max_pts)
            if acc is not None:
                _match_stage(acc, grid, ci, bi, tabs, sc, cl, ksels, conf_dev, res, n_nms, total, o_lab, o_hist)
                continue
            host = res.cpu().numpy()                                       # the one host read of the stage
            row0 = hoff = 0
            for t, d, k in zip(tabs, sc, ksels):
                keep = np.stack([host[m * total + row0:m * total + row0 + k] for m in range(n_nms)], 0) != 0
                inter = host[o_hist + hoff:o_hist + hoff + k * d['G']].reshape(k, d['G'])[:, :len(t.uniq)].astype(np.int64)
                t.stages[-1].append(dict(label_id=host[o_lab + row0:o_lab + row0 + k].copy(), inter=inter, keep=keep))
                row0 += k; hoff += k * d['G']
    return tabs


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
    sc = _scene_inputs(net, batch, pred, cfg, dev)
    rs = iou_nms.nmc_device_batch([d['boxes'] for d in sc], float(grid.cluster_th[ci])) if sc else []
    by_name = {t.name: t for t in tables}
    out = {}
    for d, r in zip(sc, rs):
        t = by_name[d['name']]
        rows = compose(t, ci, si, bi, mi)
        kk = len(rows)
        if r.k != t.clusters[ci]['K']:
            raise ValueError('%s: these tables were not made from this batch and these predictions' % d['name'])
        sel = torch.from_numpy(rows.astype(np.int32)).to(dev)
        bits = torch.empty((max(kk, 1), max(d['words'], 1)), dtype=torch.int64, device=dev)
        mask = torch.empty((kk, d['n_pts']), dtype=torch.uint8, device=dev)
        _call('b2m_mask_project', r.heat.data_ptr(), d['n_fg'], sel.data_ptr(), kk, d['fg_slot'].data_ptr(), d['s2v'].data_ptr(),
              d['n_vox'], float(grid.mask_bin_th[bi]), bits.data_ptr(), d['words'])
        _call('b2m_mask_gather', bits.data_ptr(), d['words'], None, kk, d['v2p'].data_ptr(), d['n_pts'], mask.data_ptr())
        out[d['name']] = {'conf': torch.from_numpy(t.clusters[ci]['conf'][rows]).to(d['pdev']),
                          'label_id': t.stages[ci][bi]['label_id'][rows].astype('int32'), 'mask': mask.bool().to(d['pdev'])}
    return out


# ----------------------------------------------------------------------------------------------------------------- the search
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
    for item in batches:
        batch, pred = item if isinstance(item, (tuple, list)) else \
            (item, model.get_prediction(item, with_grad=False, to_cpu=True, min_size=True))
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
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)             # (no class with ground truth: nanmean of nothing)
                avg = eval_metric.compute_averages(aps)
            done[key] = (aps, (avg['all_ap'], avg['all_ap_50%'], avg['all_ap_25%']))
        aps, three = done[key]
        ap[st] = three
        if per_class:
            ap_tables[st] = aps
    rank = lambda st: tuple(-np.inf if np.isnan(v) else v for v in (ap[st][1], ap[st][0]))
    best = max(settings, key=lambda st: (rank(st), tuple(-i for i in st)))
    out = dict(ap=ap, best=best, best_ths=grid.eval_ths(*best), n_evaluated=len(done))
    if per_class:
        out['ap_tables'] = ap_tables
    return out


def _search_device(model, batches, gt_ids_by_scene, grid, per_class, shape, settings):
    from . import eval_match
    acc = eval_match.MatchAccumulator(len(settings))
    for item in batches:
        batch, pred = item if isinstance(item, (tuple, list)) else \
            (item, model.get_prediction(item, with_grad=False, to_cpu=True, min_size=True))
        model.pred2mask_sweep(batch, pred, grid, gt_ids_by_scene, acc=acc)
    table = acc.finish()                                                   # (settings, classes, overlaps), grid order
    ap = np.full(shape + (3,), np.nan)
    for q, st in enumerate(settings):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            avg = eval_metric.compute_averages(table[q:q + 1])
        ap[st] = (avg['all_ap'], avg['all_ap_50%'], avg['all_ap_25%'])
    rank = lambda st: tuple(-np.inf if np.isnan(v) else v for v in (ap[st][1], ap[st][0]))
    best = max(settings, key=lambda st: (rank(st), tuple(-i for i in st)))
    out = dict(ap=ap, best=best, best_ths=grid.eval_ths(*best), n_evaluated=len(settings))
    if per_class:
        out['ap_tables'] = table.reshape(shape + (len(eval_metric.CLASS_LABELS), len(eval_metric.OVERLAPS)))[..., None, :, :].copy()
    return out
