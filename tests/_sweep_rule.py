"""The rule the threshold sweep (box2mask_amd/param_search.py) rests on, restated in numpy on top of tests/_nms_rule.py, for
tests/test_param_sweep_rule.py (CPU) and tests/test_gpu_param_sweep.py.

Three facts, each checked against tests/golden/param_sweep.npz (every setting of a 3 x 3 x 2 x 2 grid run through the real
SelectionNet.detection2mask and scored by the real utils/eval_metric.py):

  1. ``score_th`` selects a PREFIX.  NMS_clustering visits boxes in descending score (iou_nms.py:78; ties go to the lower row
     here), so the representatives' scores are non-increasing and ``scores > score_th`` (detection_net.py:427-432) keeps the
     first k_s clusters.  A cluster's heat-map row, its mask and its label do not depend on which other clusters were kept.
  2. Greedy mask NMS on a prefix is the RESTRICTION of greedy mask NMS on the whole list: the fate of row i in mask_NMS
     (iou_nms.py:130-144) depends on rows before i only, so kept(c, s, b, m) = kept(c, b, m) & [0, k_s).  Nothing carries over
     between two mask_nms_th: each is its own walk over the same intersection table.
  3. The AP needs only COUNTS: per kept prediction its score, its label and the number of scene POINTS it shares with every
     ground-truth id (eval_metric.assign_from_counts).  Point p lies in mask r iff bit vox2point[p] of voxel mask r is set, so
     the count is a histogram of the ground-truth index over the points, looked up through vox2point.

``shared_tables`` computes, per scene, what the settings share -- 3 clusterings and 6 mask stages for the 36 settings -- as
``param_search.SweepTables``; ``compose`` picks the rows of one setting.  ``mistake=`` states one deliberate MISTAKE as a variant
of the rule; the test shows that the fixture catches each.
"""
import numpy as np
import torch

import _nms_rule as R
from box2mask_amd import param_search, synth
from oracle import nms_ref

F = np.float32
MISTAKES = ('ge_score', 'nms_flags_reused', 'inter_on_voxels', 'ks_of_other_cluster_th')
N_CLASS = 41                                    # semantic ids 0 .. 40


def content_sums(masks):
    """64-bit content sum of every boolean row: the sum over its set points p of (p + 1) * 0x9E3779B97F4A7C15, modulo 2^64."""
    masks = np.asarray(masks) != 0
    w = np.arange(1, masks.shape[1] + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    return np.array([w[m].sum(dtype=np.uint64) for m in masks], np.uint64).reshape(len(masks))


def fixture_grid(d, pre='sw_'):
    return param_search.ThresholdGrid(*(d[pre + a] for a in param_search.AXES))


def fixture_scenes(d, pre='sw_'):
    """Per scene of the fixture: the boxes of its foreground votes and everything the mask stages read."""
    valid = synth.scannet_tables()[0].numpy()
    # (torch's sigmoid is part of the consumer of the golden inputs, as in tests/test_oracle_nms.py)
    score = torch.sigmoid(torch.from_numpy(d[pre + 'pred_mlp_bb_scores'])).numpy()
    bbs = nms_ref.to_bbs_min_max(d[pre + 'input_location'], d[pre + 'pred_mlp_offsets'], d[pre + 'pred_mlp_bounds'], score)
    sem = valid[np.argmax(d[pre + 'pred_mlp_semantics'], 1)].astype(np.int64)
    out = []
    for si, name in enumerate(d[pre + 'names']):
        m = d[pre + 'batch_ids'] == si
        fg = (sem[m] > 2) & (sem[m] != 22)
        seg2vox = d[pre + 'seg2vox%d' % si]
        out.append(dict(name=str(name), boxes=bbs[m][fg], fg_slot=np.where(fg, np.cumsum(fg) - 1, -1).astype(np.int32),
                        seg2vox=seg2vox, vox2point=d[pre + 'vox2point%d' % si], sem_vox=sem[m][seg2vox].astype(np.int32),
                        gt_ids=d[pre + 'gt_ids%d' % si]))
    return out


def synthetic_inputs(seed, n_scenes=2, target_voxels=12000):
    """(batch, pred, {scene name: ground-truth ids}): a synthetic batch and head outputs that vote for the scenes' furniture boxes,
    made as the fixture's inputs were (tools/gen_golden.py, _scene_inputs) -- for seeds the fixture does not hold."""
    batch = synth.make_batch(n_scenes, seed0=seed, target_voxels=target_voxels, pts_per_m2=6000.0)
    rng = np.random.default_rng(seed)
    S = batch['input_location'].shape[0]
    fg = batch['fg_instances'].numpy()
    off = batch['gt_bb_offsets'].numpy() + rng.normal(0, 0.03, (S, 3)).astype(F)
    bnd = np.maximum(batch['gt_bb_bounds'].numpy() + rng.normal(0, 0.03, (S, 3)).astype(F), 0.04)
    bnd[~fg] = rng.uniform(0.05, 0.3, ((~fg).sum(), 3))
    logits = rng.normal(0.5, 2.0, (S, 1)).astype(F)
    valid = synth.SCANNET_SEMANTIC_VALID_CLASS_IDS
    sem_logits = rng.normal(0, 1, (S, len(valid))).astype(F)
    gt = batch['gt_semantics'].numpy()
    for s in range(S):
        if rng.random() < 0.9 and gt[s] in valid:
            sem_logits[s, int(np.nonzero(valid == gt[s])[0][0])] += 6.0
    pred = {'mlp_offsets': torch.from_numpy(off.astype(F)), 'mlp_bounds': torch.from_numpy(bnd.astype(F)),
            'mlp_bb_scores': torch.from_numpy(logits), 'mlp_semantics': torch.from_numpy(sem_logits)}
    return batch, pred, {sc['name']: synth.gt_instance_ids(batch, b) for b, sc in enumerate(batch['scene'])}


def fixture_batch(d, pre='sw_'):
    """(batch, pred, ground-truth ids by scene) of the fixture, as Model.pred2mask takes them."""
    names = [str(s) for s in d[pre + 'names']]
    batch = {'input_location': torch.from_numpy(d[pre + 'input_location']), 'batch_ids': torch.from_numpy(d[pre + 'batch_ids']),
             'scene': [{'name': n} for n in names], 'seg2vox': [d[pre + 'seg2vox%d' % i] for i in range(len(names))],
             'vox2point': [d[pre + 'vox2point%d' % i] for i in range(len(names))]}
    pred = {h: torch.from_numpy(d[pre + 'pred_' + h]) for h in ('mlp_offsets', 'mlp_bounds', 'mlp_bb_scores', 'mlp_semantics')}
    return batch, pred, {n: d[pre + 'gt_ids%d' % i] for i, n in enumerate(names)}


def shared_tables(scene, grid, mistake=None):
    """(SweepTables, point masks): point masks[ci][bi] = (K', n_pts) uint8 of every projected row, for the content sums."""
    boxes, v2p = scene['boxes'], np.asarray(scene['vox2point'], np.int64)
    n_vox, n_pts = len(scene['seg2vox']), len(v2p)
    uniq, dense, vert = np.unique(scene['gt_ids'], return_inverse=True, return_counts=True)
    dense = dense.reshape(-1)
    t = param_search.SweepTables(scene['name'], n_pts, uniq.astype(np.int64), vert.astype(np.int64))
    point_masks = []
    for cth in grid.cluster_th:
        r = R.nmc(boxes, cth, len(boxes))
        conf = boxes[r['reps'], 0]
        assert np.all(np.diff(conf) <= 0)                                   # fact 1: non-increasing
        ks = np.array([int(((conf >= F(th)) if mistake == 'ge_score' else (conf > F(th))).sum()) for th in grid.score_th], np.int64)
        assert all(np.array_equal(np.nonzero(conf > F(th))[0], np.arange(k)) for th, k in zip(grid.score_th, ks)) or mistake
        t.clusters.append(dict(K=r['k'], conf=conf, reps=r['reps'].astype(np.int64), ks=ks))
        kp = int(ks[0])                                                     # rows of the smallest score_th: no setting keeps more
        stages, pms = [], []
        for bth in grid.mask_bin_th:
            bits = R.project(r['heat'][:r['k']], np.arange(kp), scene['fg_slot'], scene['seg2vox'], bth)
            keep = np.stack([R.mask_nms(bits, mth)[1] for mth in grid.mask_nms_th], 0).reshape(len(grid.mask_nms_th), kp) != 0
            label = R.label_hist(bits, None, scene['sem_vox'], n_vox, N_CLASS)
            pm = R.gather(bits, None, v2p, n_pts)
            if mistake == 'inter_on_voxels':                                # every voxel once, with the id of its first point
                vox, first = np.unique(v2p, return_index=True)
                vm = R.unpack(bits, n_vox)[:, vox]
                inter = np.stack([np.bincount(dense[first][row], minlength=len(uniq)) for row in vm], 0) if kp else None
            else:
                inter = np.stack([np.bincount(dense[row != 0], minlength=len(uniq)) for row in pm], 0) if kp else None
            if inter is None:
                inter = np.zeros((0, len(uniq)), np.int64)
            stages.append(dict(label_id=label.astype(np.int32), inter=inter.astype(np.int64), keep=keep))
            pms.append(pm)
        t.stages.append(stages)
        point_masks.append(pms)
    return t, point_masks


def compose(tables, ci, si, bi, mi, mistake=None):
    """Rows of clusters[ci] that setting (ci, si, bi, mi) keeps: the prefix, then the restriction of the full-list NMS."""
    k_s = int(tables.clusters[(ci + 1) % len(tables.clusters) if mistake == 'ks_of_other_cluster_th' else ci]['ks'][si])
    keep = tables.stages[ci][bi]['keep']
    return np.nonzero(keep[0 if mistake == 'nms_flags_reused' else mi, :k_s])[0].astype(np.int64)
