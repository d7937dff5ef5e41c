"""The front half of votes -> masks that ``SelectionNet.detection2mask`` and the threshold sweeps of param_search.py share: the
per-scene inputs (stage 0 of /root/reference/models/detection_net.py:369-488), the clustering read-back with the score filter, the
B2M_MASK_DESC table of the batched mask stages (include/b2m.h) and the projection + point gather of one scene.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import iou_nms
from .util import to_bbs_min_max

_call = _lib.call


def scene_inputs(net, batch, pred, cfg, dev, points=False):
    """Stage 0, one dict per scene of the batch: name, idx, s2v (voxel -> vote row, int64), n_vox, words = ceil(n_vox / 64),
    sem_vox (label per voxel, int32), fg (foreground votes, where the predictions live: pdev), fg_dev, fg_slot (row among the
    foreground votes or -1, int32), bbs (foreground boxes [score, min3, max3] on pdev), boxes (fp32 on the device), n_fg.
    Everything not named pdev is on ``dev``.  points: also v2p (voxel of every point), n_pts and, in the S3DIS flow, sem_pts.

    ScanNet flow: semantics per vote through ``semantic_valid_class_ids``.  S3DIS flow (``net.requires_voxel_outputs``,
    detection_net.py:398-415): per-voxel argmax, then the majority vote of every segment's voxels, the lowest class on ties
    (``b2m_seg_mode``); the class count is the width of the per-voxel head, so every class index is in range."""
    pdev = pred[cfg.mlp_offsets].device
    pred_bbs = to_bbs_min_max(batch['input_location'].to(pdev), pred[cfg.mlp_offsets], pred[cfg.mlp_bounds],
                              torch.nn.Sigmoid()(pred[cfg.mlp_bb_scores]))
    per_vox = net.requires_voxel_outputs
    if per_vox:
        head = torch.as_tensor(pred[cfg.mlp_per_vox_semantics])
        pred_semantics, n_class = torch.argmax(head, 1), int(head.shape[1])
    else:
        pred_semantics = net.semantic_valid_class_ids.to(pdev)[torch.argmax(pred[cfg.mlp_semantics], 1)].long()
    batch_ids = batch['batch_ids'].to(pdev)
    masks = [batch_ids == i for i in range(len(batch['scene']))]
    # without segment pooling the predictions already live on the voxels (detection_net.py:436-445 projects only `if
    # cfg.do_segment_pooling`): the voxel of vote j IS j.  (The reference's branch then indexes per-voxel arrays with masks that have
    # one column per FOREGROUND vote, :463 / :470, and fails on the first background voxel; here background votes are zero-padded
    # exactly as the pooled branch does, which is the same result whenever the reference has one.)
    seg2vox = [torch.as_tensor(batch['seg2vox'][i]).long() if cfg.do_segment_pooling else torch.arange(int(m.sum()), dtype=torch.long)
               for i, m in enumerate(masks)]
    if per_vox and sum(v.shape[0] for v in seg2vox) != pred_semantics.shape[0]:
        raise ValueError('%d per-voxel predictions for %d voxels' % (pred_semantics.shape[0], sum(v.shape[0] for v in seg2vox)))
    sc, vox_start = [], 0
    for idx, (scene, scene_mask, s2v) in enumerate(zip(batch['scene'], masks, seg2vox)):
        n_vox = int(s2v.shape[0])
        scene_bbs = pred_bbs[scene_mask]
        if per_vox:
            n_seg = int(scene_bbs.shape[0])
            if n_vox and int(s2v.max()) >= n_seg:
                raise ValueError('%s: seg2vox names segment %d of %d' % (scene['name'], int(s2v.max()), n_seg))
            s2v = s2v.to(dev).contiguous()
            sem_vox = pred_semantics[vox_start:vox_start + n_vox].to(dev).int().contiguous()
            hist = torch.empty(max(n_seg * n_class, 1), dtype=torch.int32, device=dev)
            mode = torch.zeros(max(n_seg, 1), dtype=torch.int32, device=dev)
            _call('b2m_seg_mode', s2v.int().contiguous().data_ptr(), sem_vox.data_ptr(), n_vox, n_seg, n_class, hist.data_ptr(),
                  mode.data_ptr())
            fg = net.is_foreground(mode[:n_seg].long()).to(pdev)
        else:
            s2v = s2v.to(dev).contiguous()
            scene_sem = pred_semantics[scene_mask]
            fg = net.is_foreground(scene_sem)
            sem_vox = scene_sem.to(dev)[s2v].int().contiguous()
        vox_start += n_vox
        bbs = scene_bbs[fg]
        boxes = bbs.detach().to(dev, torch.float32).contiguous()
        if boxes.shape[0] == 0:
            # the reference crashes on a scene without foreground votes (torch.stack([]), iou_nms.py:103)
            raise ValueError('NMS_clustering needs at least one box (the reference raises on n == 0 as well)')
        fg_dev = fg.to(dev)
        fg_slot = torch.where(fg_dev, torch.cumsum(fg_dev.int(), 0) - 1, torch.full_like(fg_dev.int(), -1)).int()
        d = dict(name=scene['name'], idx=idx, s2v=s2v, n_vox=n_vox, words=(n_vox + 63) // 64, sem_vox=sem_vox, fg=fg, fg_dev=fg_dev,
                 fg_slot=fg_slot, bbs=bbs, boxes=boxes, n_fg=int(boxes.shape[0]), pdev=pdev)
        if points:
            d['v2p'] = torch.as_tensor(batch['vox2point'][idx]).long().to(dev).contiguous()
            d['n_pts'] = int(d['v2p'].shape[0])
            if per_vox:
                d['sem_pts'] = sem_vox[d['v2p']].contiguous()
        sc.append(d)
    return sc


def clusters(sc, cluster_th):
    """Instance clusters (iou_nms.py:68-105) of every scene in one launch, and two host reads for the batch: per scene (the device
    result, conf (K,) float32 = the representatives' scores in visiting order, reps (K,) int64 rows among the foreground votes)."""
    rs = iou_nms.nmc_device_batch([d['boxes'] for d in sc], cluster_th)
    rep_scores = torch.cat([d['boxes'][r.reps[:r.k].long(), 0] for d, r in zip(sc, rs)]).cpu().numpy()
    reps_host = torch.cat([r.reps[:r.k] for r in rs]).cpu().numpy().astype(np.int64)
    offs = np.cumsum([0] + [r.k for r in rs])
    return [(r, rep_scores[o:o + r.k], reps_host[o:o + r.k]) for r, o in zip(rs, offs)]


def score_filter(conf, score_th):
    """Rows with ``conf > score_th`` (detection_net.py:427-432); the threshold enters as float32."""
    return np.nonzero(conf > np.float32(score_th))[0].astype(np.int64)


def score_prefixes(conf, score_ths):
    """ks (len(score_ths),) int64: how many rows ``score_filter`` keeps per threshold.  The sweeps need the kept rows to be a prefix
    (the representatives come in descending score)."""
    ks = np.zeros(len(score_ths), np.int64)
    for si, th in enumerate(score_ths):
        sel = score_filter(conf, th)
        if not np.array_equal(sel, np.arange(len(sel))):
            raise ValueError('the score filter did not keep a prefix of the clusters (NaN scores?)')
        ks[si] = len(sel)
    return ks


def voxel_major_scratch(sc, ks, dev):
    """Scratch for the voxel-major images of ``b2m_mask_gather_batch_t`` / ``b2m_mask_hist_index_batch``, n_vox x ceil(k / 64) words
    per scene: (the buffer, the address of every scene's part)."""
    sizes = [d['n_vox'] * ((k + 63) // 64) for d, k in zip(sc, ks)]
    buf = torch.empty(max(sum(sizes), 1), dtype=torch.int64, device=dev)
    return buf, [buf.data_ptr() + 8 * int(o) for o in np.cumsum([0] + sizes[:-1])]


class MaskTable:
    """The B2M_MASK_DESC table of the batched mask stages: one record of int64 fields per scene, pointers stored as integers
    (include/b2m.h has the meaning of every field).  Each entry reads only the fields of its stage, so the table is made in two
    steps: the selected rows here, the kept rows in ``set_kept``.

    sels: per scene the cluster rows that enter the projection.  Allocates what the stages write -- sel_all (int32, the rows of
    all scenes back to back), bits_all (ksel x max(words, 1) words per scene), inter_all (ksel x ksel) and, with ``keep``, keep_all
    (the flags of ``b2m_mask_nms_batch``; without it field 10 is NULL: no mask NMS).  row0[s] = the first row of scene s among all
    selected rows, bits_ptr[s] = the address of its bit rows, total = the number of selected rows."""
    FIELDS = ('heat', 'n_fg', 'sel', 'ksel', 'fg_slot', 'seg2vox', 'n_vox', 'bits', 'words', 'inter', 'keep', 'rows', 'kk', 'sem',
              'labels', 'index', 'n_pts', 'out', 'row0_sel', 'row0_kept')

    def __init__(self, sc, heats, sels, dev, keep=False):
        self.sc, self.dev = sc, dev
        self.ksels = ksels = [int(len(s)) for s in sels]
        self.total = sum(ksels)
        self.desc = np.zeros((len(sc), len(self.FIELDS)), np.int64)
        self.sel_all = torch.from_numpy(np.concatenate(sels).astype(np.int32)).to(dev) if self.total else \
            torch.zeros(1, dtype=torch.int32, device=dev)
        self.bits_all = torch.empty(max(sum(k * max(d['words'], 1) for k, d in zip(ksels, sc)), 1), dtype=torch.int64, device=dev)
        self.inter_all = torch.empty(max(sum(k * k for k in ksels), 1), dtype=torch.int32, device=dev)
        self.keep_all = torch.empty(max(self.total, 1), dtype=torch.int32, device=dev) if keep else None
        self.row0, self.bits_ptr = [], []
        row0 = boff = ioff = 0
        for s_, (d, heat, k) in enumerate(zip(sc, heats, ksels)):
            self.row0.append(row0)
            self.bits_ptr.append(self.bits_all.data_ptr() + 8 * boff)
            self._set(s_, heat=heat.data_ptr(), n_fg=d['n_fg'], sel=self.sel_all.data_ptr() + 4 * row0, ksel=k,
                      fg_slot=d['fg_slot'].data_ptr(), seg2vox=d['s2v'].data_ptr(), n_vox=d['n_vox'], bits=self.bits_ptr[-1],
                      words=d['words'], inter=self.inter_all.data_ptr() + 4 * ioff,
                      keep=self.keep_all.data_ptr() + 4 * row0 if (keep and k > 0) else 0, row0_sel=row0)
            row0 += k; boff += k * max(d['words'], 1); ioff += k * k

    def _set(self, s_, **fields):
        for name, value in fields.items():
            self.desc[s_, self.FIELDS.index(name)] = value

    def set_kept(self, kks, rows_ptr, labels_ptr, gather=None):
        """Fields 11-17 and 19.  Scene s keeps kks[s] of its bit rows: their int32 row numbers start at rows_ptr (0: rows 0 .. kk - 1)
        and their labels at labels_ptr, both at the scene's first row among all kept rows.  gather: per scene (index, n_pts, out)
        for the point gather -- index = the int64 voxel of every point or None (identity), out = uint8 (kk, n_pts)."""
        row0 = 0
        for s_, (d, kk) in enumerate(zip(self.sc, kks)):
            self._set(s_, rows=rows_ptr + 4 * row0 if rows_ptr else 0, kk=kk, sem=d['sem_vox'].data_ptr(), labels=labels_ptr + 4 * row0,
                      row0_kept=row0)
            if gather is not None:
                index, n_pts, out = gather[s_]
                self._set(s_, index=0 if index is None else index.data_ptr(), n_pts=n_pts, out=out.data_ptr())
            row0 += kk

    def upload(self, tail=()):
        """The table as it stands on the device, an optional int64 tail (the ``tbits`` pointers of ``b2m_mask_gather_batch_t``, a
        scorer's descriptor table) riding behind it in the one upload: (desc_ptr, extra_ptr = the address of the tail)."""
        self.table_dev = torch.from_numpy(np.concatenate([self.desc.reshape(-1), np.asarray(tail, np.int64).reshape(-1)])).to(self.dev)
        return self.table_dev.data_ptr(), self.table_dev.data_ptr() + 8 * self.desc.size


def project_gather(d, heat, sel, k, mask_bin_th):
    """One scene: rows sel[:k] (int32, device) of ``heat`` projected on the voxels and gathered to the points, (k, n_pts) uint8."""
    dev = d['boxes'].device
    bits = torch.empty((max(k, 1), max(d['words'], 1)), dtype=torch.int64, device=dev)
    masks = torch.empty((k, d['n_pts']), dtype=torch.uint8, device=dev)
    if k:
        _call('b2m_mask_project', heat.data_ptr(), d['n_fg'], sel.data_ptr(), k, d['fg_slot'].data_ptr(), d['s2v'].data_ptr(),
              d['n_vox'], float(mask_bin_th), bits.data_ptr(), d['words'])
        _call('b2m_mask_gather', bits.data_ptr(), d['words'], None, k, d['v2p'].data_ptr(), d['n_pts'], masks.data_ptr())
    return masks
