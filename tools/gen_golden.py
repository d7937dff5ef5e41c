"""Generate golden vectors from the REAL reference code (run in the build container only).

    python tools/gen_golden.py            # writes tests/golden/*.npz

It imports /root/reference/models/iou_nms.py and utils/util.py unmodified, and drives
SelectionNet.detection2mask / Model.compute_loss_detection through import stand-ins for the
absent MinkowskiEngine / open3d modules (only needed so `import models.detection_net` succeeds;
the two functions themselves use torch / numpy / scipy only — SURVEY.md Appendix B).
Nothing from /root/reference is copied: the fixtures hold inputs and outputs only.
This script is never needed on the GPU box.
"""
from __future__ import annotations

import os
import sys
import types
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, 'tests', 'golden')
REF = '/root/reference'
sys.path.insert(0, ROOT)

from box2mask_amd import synth  # noqa: E402


def _install_stubs():
    class Holder:
        def __init__(self, F=None, C=None, **kw):
            self.F, self.C = F, C

    me = types.ModuleType('MinkowskiEngine')
    me.SparseTensor = Holder
    me.TensorField = Holder
    me.MinkowskiConvolution = me.MinkowskiBatchNorm = me.MinkowskiReLU = object
    mods = types.ModuleType('MinkowskiEngine.modules')
    rb = types.ModuleType('MinkowskiEngine.modules.resnet_block')
    rb.Bottleneck = type('Bottleneck', (), {'expansion': 4})
    rb.BasicBlock = type('BasicBlock', (), {'expansion': 1})
    sys.modules['MinkowskiEngine'] = me
    sys.modules['MinkowskiEngine.modules'] = mods
    sys.modules['MinkowskiEngine.modules.resnet_block'] = rb
    sys.modules['open3d'] = types.ModuleType('open3d')
    if 'tqdm' not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            t = types.ModuleType('tqdm'); t.tqdm = lambda x, **k: x; sys.modules['tqdm'] = t
    return Holder


def gen_iou_nms():
    sys.path.insert(0, REF)
    import models.iou_nms as R
    import utils.util as U
    rng = np.random.default_rng(7)
    out = {}
    cases = {}
    for n, nobj in ((1, 1), (64, 6), (512, 30), (2000, 60)):
        cases['votes%d' % n] = synth.make_votes(n, n_obj=nobj, n_seg=n)
    # degenerate boxes: zero side length (the "Invalid boxes" warning path), identical boxes
    b = synth.make_votes(91, n_obj=8, n_seg=200)
    b[5, 4:] = b[5, 1:4]                     # zero volume
    b[17, 4] = b[17, 1]                      # one zero side
    b[30, 1:] = b[31, 1:]                    # identical geometry, different scores
    b[40, 1:] = b[31, 1:]
    cases['degenerate'] = b
    # a box whose IoU with the top box equals the threshold exactly (kept in `remaining` by `<=`)
    e = np.zeros((3, 7), np.float32)
    e[0] = [0.9, 0, 0, 0, 1, 1, 1]
    e[1] = [0.8, 0, 0, 0, 1, 1, 2]            # IoU = 1/(2+1e-6) < 0.5 ; use th computed from actual value
    e[2] = [0.7, 5, 5, 5, 6, 6, 6]
    cases['edge_th'] = e
    for name, boxes in cases.items():
        bt = torch.from_numpy(boxes)
        th = 0.5
        if name == 'edge_th':
            th = float(R.torch_IOUs(bt[0, 1:], bt[:, 1:])[1])     # threshold == IoU exactly
        reps, clusters, heat = R.NMS_clustering(bt, th)
        out[name + '_boxes'] = boxes
        out[name + '_th'] = np.float64(th)
        out[name + '_reps'] = reps.numpy()
        out[name + '_heat'] = heat.numpy()
        out[name + '_assign'] = _assign(clusters, len(boxes))
        out[name + '_order'] = np.concatenate([c.numpy() for c in clusters]) if False else np.zeros(0)
        # mask NMS on the thresholded heat-maps in descending score order of the representatives
        masks = heat > 0.3
        kept, supp = R.mask_NMS(masks, 0.6)
        out[name + '_masks'] = masks.numpy()
        out[name + '_mask_kept'] = kept.numpy()
    # set_IOUs / semIOU / to_bbs_min_max
    a = np.sort(rng.uniform(0, 3, (300, 2, 3)).astype(np.float32), 1).reshape(300, 6)
    c = np.sort(rng.uniform(0, 3, (300, 2, 3)).astype(np.float32), 1).reshape(300, 6)
    out['set_a'], out['set_b'] = a, c
    out['set_iou'] = R.set_IOUs(torch.from_numpy(a), torch.from_numpy(c)).numpy()
    pl = rng.integers(0, 20, 500); gl = rng.integers(0, 20, 500); gl[rng.random(500) < 0.2] = -100
    out['sem_pred'], out['sem_gt'] = pl, gl
    out['sem_iou'] = R.semIOU(torch.from_numpy(pl), torch.from_numpy(gl))
    loc = rng.normal(0, 1, (50, 3)).astype(np.float32); off = rng.normal(0, .3, (50, 3)).astype(np.float32)
    bnd = rng.uniform(.05, .5, (50, 3)).astype(np.float32); sc = rng.random((50, 1)).astype(np.float32)
    out['bbs_loc'], out['bbs_off'], out['bbs_bnd'], out['bbs_sc'] = loc, off, bnd, sc
    out['bbs_out'] = U.to_bbs_min_max(*(torch.from_numpy(v) for v in (loc, off, bnd, sc))).numpy()
    segs = [rng.integers(0, 9, 40), rng.integers(3, 14, 55), rng.integers(0, 5, 30)]
    out['uniq_in0'], out['uniq_in1'], out['uniq_in2'] = segs
    out['uniq_out'] = U.to_unique([s.copy() for s in segs]).numpy()
    np.savez_compressed(os.path.join(OUT, 'iou_nms.npz'), **out)
    print('iou_nms.npz: %d arrays' % len(out))


def _assign(clusters, n):
    a = np.full(n, -1, np.int32)
    for c, idx in enumerate(clusters):
        a[idx.numpy()] = c
    return a


def _scene_inputs(seed, n_scenes=2, target_voxels=12000):
    """Synthetic batch + head outputs that vote for the scene's furniture boxes (so clusters are meaningful)."""
    batch = synth.make_batch(n_scenes, seed0=seed, target_voxels=target_voxels, pts_per_m2=6000.0)
    rng = np.random.default_rng(seed)
    S = batch['input_location'].shape[0]
    fg = batch['fg_instances'].numpy()
    off = batch['gt_bb_offsets'].numpy() + rng.normal(0, 0.03, (S, 3)).astype(np.float32)
    bnd = np.maximum(batch['gt_bb_bounds'].numpy() + rng.normal(0, 0.03, (S, 3)).astype(np.float32), 0.04)
    bnd[~fg] = rng.uniform(0.05, 0.3, ((~fg).sum(), 3))
    logits = rng.normal(0.5, 2.0, (S, 1)).astype(np.float32)
    valid = synth.SCANNET_SEMANTIC_VALID_CLASS_IDS
    sem_logits = rng.normal(0, 1, (S, len(valid))).astype(np.float32)
    gt = batch['gt_semantics'].numpy()
    for s in range(S):           # mostly-correct semantics so that foreground selection is realistic
        if rng.random() < 0.9 and gt[s] in valid:
            sem_logits[s, int(np.nonzero(valid == gt[s])[0][0])] += 6.0
    pred = {'mlp_offsets': torch.from_numpy(off.astype(np.float32)), 'mlp_bounds': torch.from_numpy(bnd.astype(np.float32)),
            'mlp_bb_scores': torch.from_numpy(logits), 'mlp_semantics': torch.from_numpy(sem_logits)}
    return batch, pred


def gen_detection2mask():
    _install_stubs()
    sys.path.insert(0, REF)
    import models.detection_net as dn
    valid, id2idx, _, is_fg = synth.scannet_tables()
    cfg = SimpleNamespace(mlp_per_vox_semantics='mlp_per_vox_semantics', mlp_semantics='mlp_semantics',
                          network_heads=['mlp_offsets', 'mlp_bounds', 'mlp_bb_scores', 'mlp_semantics'],
                          do_segment_pooling=True)
    ns = SimpleNamespace(requires_voxel_outputs=False, semantic_valid_class_ids=valid, is_foreground=is_fg)
    out = {}
    for case, seed in (('a', 11), ('b', 23)):
        batch, pred = _scene_inputs(seed)
        ths = [0.5, 0.05, 0.3, 0.6]
        for mode in ('eval', 'train'):
            res = dn.SelectionNet.detection2mask(ns, batch, {k: v.clone() for k, v in pred.items()}, cfg, mode, True, *ths)
            for si, sc in enumerate(batch['scene']):
                r = res[sc['name']]
                pre = 'd2m_%s_%s_s%d_' % (case, mode, si)
                out[pre + 'conf'] = r['conf'].numpy()
                out[pre + 'label_id'] = np.asarray(r['label_id'])
                out[pre + 'mask'] = np.packbits(r['mask'].numpy(), axis=1)
                out[pre + 'mask_shape'] = np.asarray(r['mask'].shape)
                if mode != 'eval':
                    out[pre + 'reps'] = r['cluster_representatives'].numpy()
        for k, v in pred.items():
            out['d2m_%s_pred_%s' % (case, k)] = v.numpy()
        out['d2m_%s_input_location' % case] = batch['input_location'].numpy()
        out['d2m_%s_batch_ids' % case] = batch['batch_ids'].numpy()
        for si in range(len(batch['scene'])):
            out['d2m_%s_seg2vox%d' % (case, si)] = np.asarray(batch['seg2vox'][si])
            out['d2m_%s_vox2point%d' % (case, si)] = np.asarray(batch['vox2point'][si])
        out['d2m_%s_names' % case] = np.asarray([s['name'] for s in batch['scene']])
        out['d2m_%s_ths' % case] = np.asarray(ths)
    # ---- S3DIS flow (detection_net.py:398-415,449-451): per-voxel semantics head, majority vote per segment,
    # no mask NMS; batch of ONE scene (the reference indexes the whole batch's voxels there)
    s3_valid = torch.Tensor(np.arange(13))
    cfg3 = SimpleNamespace(mlp_per_vox_semantics='mlp_per_vox_semantics', mlp_semantics='mlp_semantics',
                           network_heads=['mlp_offsets', 'mlp_bounds', 'mlp_bb_scores', 'mlp_per_vox_semantics'],
                           do_segment_pooling=True)
    ns3 = SimpleNamespace(requires_voxel_outputs=True, semantic_valid_class_ids=s3_valid, is_foreground=lambda s: s > 2)
    batch, pred = _scene_inputs(31, n_scenes=1, target_voxels=15000)
    rng = np.random.default_rng(31)
    n_vox = batch['vox_coords'].shape[0]
    seg2vox = np.asarray(batch['seg2vox'][0])
    # per-voxel logits: the segment's class (scannet id mapped into 0..12) + noise, so that votes are not unanimous
    seg_cls = (batch['gt_semantics'].numpy() % 13)
    vox_logits = rng.normal(0, 1, (n_vox, 13)).astype(np.float32)
    vox_logits[np.arange(n_vox), seg_cls[seg2vox]] += 2.0
    pred3 = {k: v for k, v in pred.items() if k != 'mlp_semantics'}
    pred3['mlp_per_vox_semantics'] = torch.from_numpy(vox_logits)
    ths3 = [0.5, 0.03, 0.3, 0.6]
    for mode in ('eval', 'train'):
        res = dn.SelectionNet.detection2mask(ns3, batch, {k: v.clone() for k, v in pred3.items()}, cfg3, mode, True, *ths3)
        r = res[batch['scene'][0]['name']]
        pre = 'd2m_s3_%s_s0_' % mode
        out[pre + 'conf'] = r['conf'].numpy()
        out[pre + 'label_id'] = np.asarray(r['label_id'])
        out[pre + 'mask'] = np.packbits(r['mask'].numpy(), axis=1)
        out[pre + 'mask_shape'] = np.asarray(r['mask'].shape)
    for k, v in pred3.items():
        out['d2m_s3_pred_%s' % k] = v.numpy()
    out['d2m_s3_input_location'] = batch['input_location'].numpy()
    out['d2m_s3_batch_ids'] = batch['batch_ids'].numpy()
    out['d2m_s3_seg2vox0'] = seg2vox
    out['d2m_s3_vox2point0'] = np.asarray(batch['vox2point'][0])
    out['d2m_s3_vox_segments0'] = np.asarray(batch['vox_segments'][0])
    out['d2m_s3_names'] = np.asarray([batch['scene'][0]['name']])
    out['d2m_s3_ths'] = np.asarray(ths3)
    np.savez_compressed(os.path.join(OUT, 'detection2mask.npz'), **out)
    print('detection2mask.npz: %d arrays' % len(out))


SWEEP_GRID = ([0.3, 0.5, 0.7], [0.0, 0.05, 0.2], [0.2, 0.35], [0.4, 0.8])
SWEEP_WITH_MASKS = ((0, 0, 0, 1), (2, 2, 1, 0))


def mask_content_sums(masks):
    """64-bit content sum of every boolean row: the sum over its set points p of (p + 1) * 0x9E3779B97F4A7C15, modulo 2^64."""
    masks = np.asarray(masks, bool)
    w = (np.arange(1, masks.shape[1] + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    return np.array([w[m].sum(dtype=np.uint64) for m in masks], np.uint64).reshape(len(masks))


def gen_sweep():
    """tests/golden/param_sweep.npz: a 3 x 3 x 2 x 2 threshold grid, every setting run through the real SelectionNet.detection2mask
    (the stubs of gen_detection2mask) and scored with the real utils/eval_metric.py (assign_instances_for_scan, evaluate_matches,
    compute_averages; the ground truth of synth.gt_instance_ids in a temporary txt file as in gen_eval).  Per setting and scene the
    scores, labels, point counts and content sums of the masks -- the masks themselves for two settings only, which keeps the
    file small."""
    import itertools
    import tempfile
    _install_stubs()
    for a, t in (('float', float), ('bool', bool), ('int', int)):
        if not hasattr(np, a):
            setattr(np, a, t)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import models.detection_net as dn
    import utils.eval_metric as E
    valid, id2idx, _, is_fg = synth.scannet_tables()
    cfg = SimpleNamespace(mlp_per_vox_semantics='mlp_per_vox_semantics', mlp_semantics='mlp_semantics',
                          network_heads=['mlp_offsets', 'mlp_bounds', 'mlp_bb_scores', 'mlp_semantics'],
                          do_segment_pooling=True)
    ns = SimpleNamespace(requires_voxel_outputs=False, semantic_valid_class_ids=valid, is_foreground=is_fg)
    batch, pred = _scene_inputs(11)
    names = [s['name'] for s in batch['scene']]
    out = {'sw_names': np.asarray(names), 'sw_input_location': batch['input_location'].numpy(), 'sw_batch_ids': batch['batch_ids'].numpy()}
    for k, v in zip(('cluster_th', 'score_th', 'mask_bin_th', 'mask_nms_th'), SWEEP_GRID):
        out['sw_' + k] = np.asarray(v, np.float64)
    for k, v in pred.items():
        out['sw_pred_' + k] = v.numpy()
    gt_files = []
    for si in range(len(names)):
        out['sw_seg2vox%d' % si] = np.asarray(batch['seg2vox'][si])
        out['sw_vox2point%d' % si] = np.asarray(batch['vox2point'][si])
        gt = synth.gt_instance_ids(batch, si)
        out['sw_gt_ids%d' % si] = gt
        with tempfile.NamedTemporaryFile('w', suffix='.txt', delete=False) as f:
            f.write('\n'.join(str(int(v)) for v in gt) + '\n')
        gt_files.append(f.name)
    shape = tuple(len(a) for a in SWEEP_GRID)
    counts = np.zeros(shape + (len(names),), np.int64)
    triples = set()

    def run(ths, tag, with_masks):
        """One setting through the reference; returns the instance count of every scene."""
        res = dn.SelectionNet.detection2mask(ns, batch, {k: v.clone() for k, v in pred.items()}, cfg, 'eval', True, *ths)
        matches, n_inst = {}, []
        for si, name in enumerate(names):
            r = res[name]
            mask = r['mask'].numpy()
            pre = 'sw_%s_s%d_' % (tag, si)
            out[pre + 'conf'] = r['conf'].numpy()
            out[pre + 'label_id'] = np.asarray(r['label_id'])
            out[pre + 'count'] = mask.sum(1).astype(np.int64)
            out[pre + 'sum'] = mask_content_sums(mask)
            if with_masks:
                out[pre + 'mask'] = np.packbits(mask, axis=1)
            n_inst.append(mask.shape[0])
            info = {'conf': r['conf'].numpy(), 'label_id': np.asarray(r['label_id']), 'mask': mask}
            gt2pred, pred2gt = E.assign_instances_for_scan(name, info, gt_files[si])
            matches[name] = {'gt': gt2pred, 'pred': pred2gt}
        ap, _ = E.evaluate_matches(matches)
        avgs = E.compute_averages(ap)
        out['sw_%s_ap' % tag] = ap
        out['sw_%s_avg' % tag] = np.array([avgs['all_ap'], avgs['all_ap_50%'], avgs['all_ap_25%']])
        return n_inst

    for q, st in enumerate(itertools.product(*(range(n) for n in shape))):
        counts[st] = run([SWEEP_GRID[a][i] for a, i in enumerate(st)], 'q%02d' % q, st in SWEEP_WITH_MASKS)
        triples.add(tuple(out['sw_q%02d_avg' % q].tolist()))
    # one setting more, off the grid: score_th EQUAL to the score of an instance the grid keeps -- `scores > score_th` drops that
    # cluster, `>=` would keep it (no score of these inputs equals a grid value, so the grid alone cannot tell the two apart)
    q_tie = int(np.ravel_multi_index((1, 0, 0, 1), shape))
    conf0 = out['sw_q%02d_s0_conf' % q_tie]
    tie = float(conf0[len(conf0) // 2])
    out['sw_tie_ths'] = np.array([SWEEP_GRID[0][1], tie, SWEEP_GRID[2][0], SWEEP_GRID[3][1]], np.float64)
    n_tie = run(out['sw_tie_ths'].tolist(), 'tie', False)
    assert np.float32(tie) == conf0[len(conf0) // 2] and n_tie[0] < len(conf0) and (out['sw_tie_s0_conf'] > np.float32(tie)).all()
    for f in gt_files:
        os.unlink(f)
    # the fixture must never go flat: every axis changes the instance count of some scene, and the AP moves
    for axis in range(4):
        assert (np.diff(counts, axis=axis) != 0).any(), 'axis %d never changes an instance count' % axis
    assert len(triples) >= 8, 'only %d distinct AP / AP50 / AP25 triples' % len(triples)
    path = os.path.join(OUT, 'param_sweep.npz')
    _savez_fixed(path, out)
    assert os.path.getsize(path) <= 1000000
    print('param_sweep.npz: %d bytes, %d settings, %d distinct (K0, K1), %d distinct AP triples, instances %s .. %s'
          % (os.path.getsize(path), counts[..., 0].size, len({tuple(c) for c in counts.reshape(-1, len(names)).tolist()}),
             len(triples), counts.reshape(-1, len(names)).min(0).tolist(), counts.reshape(-1, len(names)).max(0).tolist()))


def gen_detection2mask_nopool():
    """SelectionNet.detection2mask with cfg.do_segment_pooling = False (detection_net.py:436-445: the heat-maps are NOT
    projected through seg2vox, the predictions already live on the voxels).  The reference's branch only executes when every
    voxel of a scene is predicted foreground: it indexes the per-voxel semantics and vox2point with masks that have one
    column per FOREGROUND vote (:463, :470) -- any background voxel is a shape mismatch.  The fixture therefore predicts a
    furniture class everywhere; box2mask_amd pads background votes with zeros as the pooled branch does."""
    _install_stubs()
    sys.path.insert(0, REF)
    import models.detection_net as dn
    valid, id2idx, _, is_fg = synth.scannet_tables()
    cfg = SimpleNamespace(mlp_per_vox_semantics='mlp_per_vox_semantics', mlp_semantics='mlp_semantics',
                          network_heads=['mlp_offsets', 'mlp_bounds', 'mlp_bb_scores', 'mlp_semantics'],
                          do_segment_pooling=False)
    ns = SimpleNamespace(requires_voxel_outputs=False, semantic_valid_class_ids=valid, is_foreground=is_fg)
    out = {}
    for case, seed in (('a', 41), ('b', 47)):
        batch, _ = _scene_inputs(seed, n_scenes=2, target_voxels=2500)
        rng = np.random.default_rng(seed)
        coords = batch['vox_coords'].numpy()
        n_vox = coords.shape[0]
        seg_of_vox = batch['pooling_ids'].numpy()                      # segment row of every voxel (batch-wide)
        loc = (coords[:, 1:].astype(np.float32) * np.float32(0.02))   # vox_world_coords (dataloader.py:98-105)
        seg_loc = batch['input_location'].numpy()[seg_of_vox]
        # every voxel votes for its segment's box (furniture segments) or for a small box of its own
        off = batch['gt_bb_offsets'].numpy()[seg_of_vox] + (seg_loc - loc) + rng.normal(0, 0.03, (n_vox, 3)).astype(np.float32)
        bnd = np.maximum(batch['gt_bb_bounds'].numpy()[seg_of_vox] + rng.normal(0, 0.03, (n_vox, 3)).astype(np.float32), 0.04)
        bg_vox = ~batch['fg_instances'].numpy()[seg_of_vox]           # floor / wall segments: one 1 m box around the segment
        bnd[bg_vox] = (0.5 + rng.normal(0, 0.02, (int(bg_vox.sum()), 3))).astype(np.float32)
        logits = rng.normal(0.5, 2.0, (n_vox, 1)).astype(np.float32)
        fg_classes = np.nonzero(is_fg(torch.from_numpy(valid.numpy() if hasattr(valid, 'numpy') else np.asarray(valid)).long()).numpy())[0]
        sem_logits = rng.normal(0, 1, (n_vox, len(valid))).astype(np.float32)
        pick = fg_classes[(seg_of_vox * 7) % len(fg_classes)]        # one furniture class per segment: every voxel foreground
        sem_logits[np.arange(n_vox), pick] += 12.0
        flip = rng.random(n_vox) < 0.1                                 # some voxels of another (furniture) class
        sem_logits[flip, fg_classes[rng.integers(0, len(fg_classes), int(flip.sum()))]] += 20.0
        pred = {'mlp_offsets': torch.from_numpy(off.astype(np.float32)), 'mlp_bounds': torch.from_numpy(bnd.astype(np.float32)),
                'mlp_bb_scores': torch.from_numpy(logits), 'mlp_semantics': torch.from_numpy(sem_logits)}
        vbatch = {'input_location': torch.from_numpy(loc), 'batch_ids': torch.from_numpy(coords[:, 0].astype(np.int64)),
                  'scene': batch['scene'], 'vox2point': batch['vox2point']}
        ths = [0.5, 0.05, 0.3, 0.6]
        for mode in ('eval', 'train'):
            res = dn.SelectionNet.detection2mask(ns, vbatch, {k: v.clone() for k, v in pred.items()}, cfg, mode, True, *ths)
            for si, sc in enumerate(batch['scene']):
                r = res[sc['name']]
                pre = 'np_%s_%s_s%d_' % (case, mode, si)
                out[pre + 'conf'] = r['conf'].numpy()
                out[pre + 'label_id'] = np.asarray(r['label_id'])
                out[pre + 'mask'] = np.packbits(r['mask'].numpy(), axis=1)
                out[pre + 'mask_shape'] = np.asarray(r['mask'].shape)
                if mode != 'eval':
                    out[pre + 'reps'] = r['cluster_representatives'].numpy()
        for k, v in pred.items():
            out['np_%s_pred_%s' % (case, k)] = v.numpy()
        out['np_%s_input_location' % case] = loc
        out['np_%s_batch_ids' % case] = coords[:, 0].astype(np.int64)
        for si in range(len(batch['scene'])):
            out['np_%s_vox2point%d' % (case, si)] = np.asarray(batch['vox2point'][si])
        out['np_%s_names' % case] = np.asarray([s['name'] for s in batch['scene']])
        out['np_%s_ths' % case] = np.asarray(ths)
    np.savez_compressed(os.path.join(OUT, 'detection2mask_nopool.npz'), **out)
    print('detection2mask_nopool.npz: %d arrays, %s instances' % (len(out), [int(out[k][0]) for k in out if k.endswith('eval_s0_mask_shape')]))


def gen_losses():
    Holder = _install_stubs()
    sys.path.insert(0, REF)
    import models.model as M
    valid, id2idx, _, is_fg = synth.scannet_tables()

    class LUT:                                  # swallows the hard-coded .to('cuda') at model.py:199
        def __init__(self, t): self.t = t
        def __getitem__(self, i):
            r = self.t[i]
            return SimpleNamespace(to=lambda *_: r)

    out = {}
    # a: score loss on; b: IoU loss on, score loss weight 0 (early epoch); c: centre-score head; d: per-voxel
    # semantics head, losses over ALL segments (no foreground selection) -- the S3DIS-style configuration
    for case, seed, epoch in (('a', 5, 150), ('b', 9, 3), ('c', 11, 150), ('d', 13, 150)):
        batch, pred0 = _scene_inputs(seed)
        heads = ['mlp_offsets', 'mlp_bounds', 'mlp_bb_scores', 'mlp_semantics']
        rng = np.random.default_rng(100 + seed)
        if case == 'c':
            heads = heads + ['mlp_center_scores']
            pred0['mlp_center_scores'] = torch.from_numpy(rng.uniform(0, 0.4, (pred0['mlp_offsets'].shape[0], 1)).astype(np.float32))
        if case == 'd':
            heads = ['mlp_offsets', 'mlp_bounds', 'mlp_bb_scores', 'mlp_per_vox_semantics']
            del pred0['mlp_semantics']
            nvox = batch['vox_coords'].shape[0]
            pred0['mlp_per_vox_semantics'] = torch.from_numpy(rng.normal(0, 1, (nvox, 20)).astype(np.float32))
            batch['gt_per_vox_semantics'] = batch['gt_semantics'][batch['pooling_ids']]
        pred = {k: v.clone().requires_grad_(True) for k, v in pred0.items()}
        cfg = SimpleNamespace(mlp_offsets='mlp_offsets', mlp_bounds='mlp_bounds', mlp_bb_scores='mlp_bb_scores',
                              mlp_center_scores='mlp_center_scores', mlp_semantics='mlp_semantics',
                              mlp_per_vox_semantics='mlp_per_vox_semantics',
                              network_heads=heads,
                              loss_on_fg_instances=(case != 'd'), bb_supervision=(case in 'ab'),
                              use_bb_iou_loss=(case == 'b'), loss_weight_center_scores=0.7,
                              loss_weight_per_vox_semantics=0.9,
                              loss_weight_bb_offsets=1.0, loss_weight_bb_bounds=0.5, loss_weight_bb_iou=1.0,
                              loss_weight_bb_scores=1.0, loss_weight_semantics=1.0, min_bb_size=0.04,
                              mlp_bb_scores_start_epoch=100, mlp_center_scores_start_epoch=0)
        ns = SimpleNamespace(cfg=cfg, device='cpu',
                             detection_model=lambda sin, ids: {k: Holder(v) for k, v in pred.items()},
                             BCEWithLogitsLoss=torch.nn.BCEWithLogitsLoss(),
                             semantics_loss=torch.nn.CrossEntropyLoss(ignore_index=-100),
                             semantic_id2idx=LUT(id2idx))
        losses, _ = M.Model.compute_loss_detection(ns, batch, epoch)
        losses['optimization_loss'].backward()
        for k, v in losses.items():
            out['loss_%s_%s' % (case, k)] = np.asarray(v.detach().numpy() if torch.is_tensor(v) else v, dtype=np.float64)
        for k, v in pred.items():
            out['loss_%s_pred_%s' % (case, k)] = pred0[k].numpy()
            out['loss_%s_grad_%s' % (case, k)] = v.grad.numpy() if v.grad is not None else np.zeros_like(pred0[k].numpy())
        for k in ('input_location', 'gt_bb_offsets', 'gt_bb_bounds', 'gt_semantics', 'fg_instances', 'pooling_ids',
                  'gt_per_vox_semantics'):
            if k in batch:
                out['loss_%s_batch_%s' % (case, k)] = batch[k].numpy()
        out['loss_%s_epoch' % case] = np.asarray(epoch)
    np.savez_compressed(os.path.join(OUT, 'losses.npz'), **out)
    print('losses.npz: %d arrays' % len(out))


def gen_prepare():
    """Scene preparation: ScanNet.__getitem__ (dataloader.py:53-123, 'test' mode) and collate_fn (:946-984) of the
    real reference on synthetic raw scenes.  dataprocessing.{scannet,arkitscenes,s3dis} only LOAD scenes (open3d,
    pyviz3d, ... absent here), so they are replaced by empty stand-ins whose process_scene returns the synthetic
    scene; numpy.lib.type_check (an unused import of dataloader.py:4, gone in numpy 2) and
    ME.utils.batched_coordinates likewise.  Everything this fixture records is computed by the reference's own
    lines: np.round / np.unique / sklearn ball tree / the segment loop / to_unique."""
    _install_stubs()
    sys.modules['MinkowskiEngine'].utils = SimpleNamespace(
        batched_coordinates=lambda c, dtype=None: synth.batched_coordinates(c))
    tc = types.ModuleType('numpy.lib.type_check'); tc._is_type_dispatcher = None
    sys.modules['numpy.lib.type_check'] = tc
    dp = types.ModuleType('dataprocessing'); dp.__path__ = []
    sys.modules['dataprocessing'] = dp
    for n in ('scannet', 'arkitscenes', 's3dis'):
        m = types.ModuleType('dataprocessing.' + n); sys.modules['dataprocessing.' + n] = m; setattr(dp, n, m)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import models.dataloader as D

    rng = np.random.default_rng(77)
    scenes = []
    # 0/1: room-shaped surfaces (shifted so that coordinates go negative), 2 cm;  2: a dense blob at 5 cm with many
    # points per voxel;  3: three points
    for seed, tv in ((0, 9000), (1, 6000)):
        sc = synth.make_scene(seed, target_voxels=tv, pts_per_m2=9000.0, points_only=True)
        off = np.array([0.37, 1.21, 0.0]) * (seed + 1)
        sc['positions'] = sc['positions'] - off
        sc['labels']['per_instance_bb_centers'] = (sc['labels']['per_instance_bb_centers'] - off).astype(np.float32)
        sc['voxel_size'] = 0.02
        scenes.append(sc)
    P = 4000
    bp = rng.normal(0, 0.25, (P, 3))
    cell = np.floor((bp + 2.0) / 0.2).astype(np.int64)
    blob_labels = {     # overlapping boxes: segments inside an overlap go to the smallest box (smallest_bb_heuristic)
        'unique_instances': np.arange(5),
        'per_instance_semantics': np.array([5, 7, 9, 2, 0], np.int32),
        'per_instance_bb_centers': np.array([[0, 0, 0], [0.15, 0, 0], [0, 0.1, 0], [0, 0, -1], [3, 3, 3]], np.float32),
        'per_instance_bb_bounds': np.array([[.4, .4, .4], [.4, .4, .4], [.25, .25, .25], [1, 1, .1], [.1, .1, .1]], np.float32),
    }
    blob_seg = (cell[:, 0] * 400 + cell[:, 1] * 20 + cell[:, 2]) * 3 + 1
    blob_labels['seg2inst'] = rng.integers(0, 5, int(blob_seg.max()) + 1).astype(np.int32)
    scenes.append({'name': 'blob', 'positions': bp, 'colors': rng.uniform(0, 1, (P, 3)),
                   'normals': rng.normal(size=(P, 3)), 'segments': blob_seg, 'voxel_size': 0.05,
                   'labels': blob_labels})
    scenes.append({'name': 'tiny', 'positions': np.array([[0.1, 0.2, 0.3], [0.101, 0.2, 0.3], [1.0, -0.5, 0.25]]),
                   'colors': rng.uniform(0, 1, (3, 3)), 'normals': rng.normal(size=(3, 3)),
                   'segments': np.array([5, 5, 9]), 'voxel_size': 0.02})
    out = {'n_scenes': np.array(len(scenes))}
    items = []
    for i, sc in enumerate(scenes):
        D.scannet.process_scene = lambda name, mode, cfg, do_augmentations=False, _sc=sc: (_sc, None)
        ds = D.ScanNet.__new__(D.ScanNet)
        ds.cfg = SimpleNamespace(voxel_size=sc['voxel_size'], use_normals_input=True, do_segment_pooling=True)
        ds.mode = 'test'; ds.do_augmentations = False; ds.data_list = [sc['name']]
        ret = ds[0]
        items.append(ret)
        for k in ('positions', 'colors', 'normals', 'segments'):
            out['s%d_in_%s' % (i, k)] = np.asarray(sc[k])
        out['s%d_in_voxel_size' % i] = np.array(sc['voxel_size'])
        for k in ('vox_coords', 'vox2point', 'point2vox', 'vox_segments', 'vox_features', 'vox_world_coords',
                  'seg2vox', 'seg2point', 'input_location'):
            out['s%d_%s' % (i, k)] = np.asarray(ret[k])
    # ---- 'train' mode with weak box supervision (configs/scannet.txt: bb_supervision, smallest_bb_heuristic):
    # approx_association + bbs_supervision (dataloader.py:165-314) on the two room scenes.  np.int (removed from
    # numpy 1.24 on) is what dataloader.py:187,244,... still spells: aliased for this run only.
    if not hasattr(np, 'int'):
        np.int = int
    train_items = []
    for i in (0, 1, 2):
        sc = scenes[i]
        D.scannet.process_scene = lambda name, mode, cfg, do_augmentations=False, _sc=sc: (_sc, _sc['labels'])
        ds = D.ScanNet.__new__(D.ScanNet)
        ds.cfg = SimpleNamespace(voxel_size=sc['voxel_size'], use_normals_input=True, do_segment_pooling=True,
                                 bb_supervision=True, point_association=False, majority_vote=False,
                                 smallest_bb_heuristic=True, dropout_boxes=None, noisy_boxes=None)
        ds.mode = 'train'; ds.do_augmentations = False; ds.data_list = [sc['name']]
        ret = ds[0]
        train_items.append(ret)
        for k in ('unique_instances', 'per_instance_semantics', 'per_instance_bb_centers', 'per_instance_bb_bounds',
                  'seg2inst'):
            out['s%d_label_%s' % (i, k)] = np.asarray(sc['labels'][k])
        out['s%d_inst_per_point' % i] = np.asarray(ret['pseudo_inst'][0])
        out['s%d_inst_per_seg' % i] = np.asarray(ret['pseudo_inst'][1])
        for k in ('fg_instances', 'gt_bb_bounds', 'gt_bb_offsets', 'gt_semantics'):
            out['s%d_%s' % (i, k)] = np.asarray(ret[k])
    # the two randomised supervision options (seeded by the scene name, dataloader.py:210-232) on scene 1
    sc = scenes[1]
    D.scannet.process_scene = lambda name, mode, cfg, do_augmentations=False, _sc=sc: (_sc, _sc['labels'])
    ds = D.ScanNet.__new__(D.ScanNet)
    ds.cfg = SimpleNamespace(voxel_size=sc['voxel_size'], use_normals_input=True, do_segment_pooling=True,
                             bb_supervision=True, point_association=False, majority_vote=False,
                             smallest_bb_heuristic=True, dropout_boxes=0.15, noisy_boxes=0.004)
    ds.mode = 'train'; ds.do_augmentations = False; ds.data_list = [sc['name']]
    ret = ds[0]
    out['s1_name'] = np.array(sc['name'])
    out['s1_noisy_inst_per_seg'] = np.asarray(ret['pseudo_inst'][1])
    out['s1_noisy_inst_per_point'] = np.asarray(ret['pseudo_inst'][0])
    out['s1_noisy_bbs_min'], out['s1_noisy_bbs_max'] = (np.asarray(v) for v in ret['noisy_bbs'])
    for k in ('fg_instances', 'gt_bb_bounds', 'gt_semantics'):
        out['s1_noisy_%s' % k] = np.asarray(ret[k])
    tb = D.collate_fn(SimpleNamespace(do_segment_pooling=True), 'train')(train_items[:2])
    for k in ('gt_bb_bounds', 'gt_bb_offsets', 'gt_semantics', 'fg_instances'):
        out['collate_%s' % k] = tb[k].numpy()
    # collate of the two 2 cm scenes (one voxel size per config in the reference)
    cf = D.collate_fn(SimpleNamespace(do_segment_pooling=True), 'test')
    b = cf([items[0], items[1]])
    for k in ('vox_features', 'batch_ids', 'input_location', 'pooling_ids'):
        out['collate_%s' % k] = b[k].numpy()
    np.savez_compressed(os.path.join(OUT, 'prepare.npz'), **out)
    print('prepare.npz: %d arrays, %s voxels' % (len(out), [len(it['vox_coords']) for it in items]))


def _dataloader_module():
    """models/dataloader.py of the reference behind stand-ins for the modules that only LOAD data (see gen_prepare)."""
    _install_stubs()
    sys.modules['MinkowskiEngine'].utils = SimpleNamespace(
        batched_coordinates=lambda c, dtype=None: synth.batched_coordinates(c))
    tc = types.ModuleType('numpy.lib.type_check'); tc._is_type_dispatcher = None
    sys.modules['numpy.lib.type_check'] = tc
    dp = types.ModuleType('dataprocessing'); dp.__path__ = []
    sys.modules['dataprocessing'] = dp
    for n in ('scannet', 'arkitscenes', 's3dis'):
        m = types.ModuleType('dataprocessing.' + n); sys.modules['dataprocessing.' + n] = m; setattr(dp, n, m)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import models.dataloader as D
    if not hasattr(np, 'int'):
        np.int = int                      # dataloader.py still spells np.int (removed from numpy 1.24 on)
    # dataloader.py:267,592,868,916 index stats.mode(x, None)[0][0]: the array-valued result of SciPy < 1.11.  The SciPy
    # of this image returns scalars; keepdims=True is that old behaviour (same values, same tie rule).
    import scipy.stats as st
    D.stats = SimpleNamespace(mode=lambda a, axis=0: st.mode(a, axis, keepdims=True))
    # the one function of dataprocessing/s3dis.py the dataset class calls (s3dis.py:79-82, two comparisons)
    D.s3dis.semantics_to_forground_mask = lambda semantics, cfg=None: (semantics > 2) if cfg.ignore_wall_ceiling_floor \
        else (semantics >= 0)
    return D


def gen_prepare2():
    """The remaining branches of the dataset classes from the REAL reference: ScanNet
    majority_vote / point_association / mask_supervision (dataloader.py:138-272), ARKitScenes.__getitem__ at 4 cm with
    oriented-box association (:385-621) and S3DIS box / mask supervision (:737-927), on the two labelled scenes of
    prepare2_scenes()."""
    D = _dataloader_module()
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from golden_scenes import prepare2_scenes
    scenes = prepare2_scenes()
    out = {}

    def run(cls, mod, sc, mode, **cfgkw):
        mod.process_scene = lambda name, m, cfg, do_augmentations=False, subsample_rate=None, _sc=sc: (_sc, _sc['labels'])
        ds = cls.__new__(cls)
        ds.cfg = SimpleNamespace(voxel_size=sc['voxel_size'], use_normals_input=True, dropout_boxes=None, noisy_boxes=None,
                                 **cfgkw)
        ds.mode = mode; ds.do_augmentations = False; ds.data_list = [sc['name']]; ds.data_class = mod
        ds.subsample_rate = None
        return ds[0]

    def put(tag, ret, keys):
        for k in keys:
            if k == 'pseudo_inst':
                for j, v in enumerate(ret.get(k, ())):
                    if v is not None:
                        out['%s_pseudo%d' % (tag, j)] = np.asarray(v)
            elif k in ret:
                out['%s_%s' % (tag, k)] = np.asarray(ret[k])
    TGT = ('pseudo_inst', 'fg_instances', 'gt_bb_bounds', 'gt_bb_offsets', 'gt_semantics', 'gt_per_vox_semantics',
           'instance_ids', 'vox_instances')
    for i, sc in enumerate(scenes):
        out['s%d_rotations' % i] = sc['labels']['per_instance_bb_rotations']
        # ---- ScanNet
        for heur in (True, False):
            r = run(D.ScanNet, D.scannet, sc, 'train', do_segment_pooling=True, bb_supervision=True, point_association=False,
                    majority_vote=True, smallest_bb_heuristic=heur)
            put('s%d_scannet_majority_h%d' % (i, heur), r, TGT)
            r = run(D.ScanNet, D.scannet, sc, 'train', do_segment_pooling=False, bb_supervision=True, point_association=True,
                    majority_vote=False, smallest_bb_heuristic=heur)
            put('s%d_scannet_point_h%d' % (i, heur), r, TGT + ('input_location',))
        for pool in (True, False):
            r = run(D.ScanNet, D.scannet, sc, 'train', do_segment_pooling=pool, bb_supervision=False)
            put('s%d_scannet_mask_p%d' % (i, pool), r, TGT)
        # ---- ARKitScenes (4 cm voxels as configs/arkitscenes.txt)
        sc4 = dict(sc, voxel_size=0.04)
        r = run(D.ARKitScenes, D.arkitscenes, sc4, 'test', do_segment_pooling=True)
        put('s%d_arkit' % i, r, ('vox_coords', 'vox2point', 'point2vox', 'vox_segments', 'vox_features', 'seg2vox',
                                 'seg2point', 'input_location'))
        r = run(D.ARKitScenes, D.arkitscenes, sc4, 'train', do_segment_pooling=True, bb_supervision=True,
                point_association=False)
        out['s%d_arkit_seg_pseudo0' % i], out['s%d_arkit_seg_pseudo1' % i] = (np.asarray(v) for v in
                                                                                 D.ARKitScenes.approx_association(
            SimpleNamespace(cfg=SimpleNamespace()), sc['labels'], sc, False, np.unique(r['vox_segments'])))
        put('s%d_arkit_seg' % i, r, TGT)
        # (the item itself cannot be made with point_association: :550 takes len(unique_segs) of None without segment
        # pooling and :511 raises with it -- only the association is pinned)
        out['s%d_arkit_point_pseudo0' % i] = np.asarray(D.ARKitScenes.approx_association(
            SimpleNamespace(cfg=SimpleNamespace()), sc['labels'], sc, True, np.unique(r['vox_segments']))[0])
        r = run(D.ARKitScenes, D.arkitscenes, sc4, 'train', do_segment_pooling=True, bb_supervision=False)
        put('s%d_arkit_mask' % i, r, TGT)
        # ---- S3DIS
        for ign in (True, False):
            r = run(D.S3DIS, D.s3dis, sc, 'train', do_segment_pooling=True, bb_supervision=True, point_association=False,
                    ignore_wall_ceiling_floor=ign)
            a = D.S3DIS.approx_association(SimpleNamespace(cfg=SimpleNamespace(ignore_wall_ceiling_floor=ign)),
                                           sc['labels'], sc, False, np.unique(r['vox_segments']))
            for j, v in enumerate(a):
                out['s%d_s3dis_i%d_assoc%d' % (i, ign, j)] = np.asarray(v)
            put('s%d_s3dis_i%d' % (i, ign), r, TGT)
            a = D.S3DIS.approx_association(SimpleNamespace(cfg=SimpleNamespace(ignore_wall_ceiling_floor=ign)),
                                           sc['labels'], sc, True, np.unique(r['vox_segments']))
            out['s%d_s3dis_i%d_point0' % (i, ign)], out['s%d_s3dis_i%d_point1' % (i, ign)] = (np.asarray(v) for v in a)
        r = run(D.S3DIS, D.s3dis, sc, 'val', do_segment_pooling=True, bb_supervision=False, ignore_wall_ceiling_floor=True)
        put('s%d_s3dis_mask' % i, r, TGT)
        # the voxelisation block of S3DIS.__getitem__ itself (:671-730)
        put('s%d_s3dis' % i, r, ('vox_coords', 'vox2point', 'point2vox', 'vox_segments', 'vox_features', 'seg2vox',
                                 'seg2point', 'input_location'))
    np.savez_compressed(os.path.join(OUT, 'prepare2.npz'), **out)
    print('prepare2.npz: %d arrays, %.1f kB' % (len(out), os.path.getsize(os.path.join(OUT, 'prepare2.npz')) / 1e3))


def gen_eval():
    """AP evaluation: assign_instances_for_scan / evaluate_matches / compute_averages of the real
    /root/reference/utils/eval_metric.py on synthetic predictions (noisy copies of the ground-truth instances,
    duplicates, wrong labels, tiny masks, void regions).  np.float / np.bool (removed numpy aliases the file still
    spells, eval_metric.py:111,139) are aliased for this run only."""
    import tempfile
    for a, t in (('float', float), ('bool', bool), ('int', int)):
        if not hasattr(np, a):
            setattr(np, a, t)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import utils.eval_metric as E
    rng = np.random.default_rng(5)
    valid = E.VALID_CLASS_IDS
    out = {'n_scenes': np.array(3)}
    matches = {}
    for si in range(3):
        n = 30000 + 5000 * si
        # ground truth: contiguous index ranges as instances; labels incl. void classes 1/2, one unannotated block (0)
        cuts = np.sort(rng.choice(np.arange(200, n - 200), 24 + si, replace=False))
        inst_of = np.searchsorted(cuts, np.arange(n), side='right')
        n_inst = inst_of.max() + 1
        inst_label = rng.choice(np.concatenate([valid[:6], [1, 2]]), n_inst)
        inst_label[0] = 0
        gt_ids = np.where(inst_label[inst_of] == 0, 0, inst_label[inst_of] * 1000 + inst_of + 1).astype(np.int64)
        # tiny ground-truth instance (< 100 vertices) of a valid class inside instance 3
        tiny = np.nonzero(inst_of == 3)[0][:60]
        gt_ids[tiny] = valid[2] * 1000 + 900
        masks, labels, confs = [], [], []
        for g in range(n_inst):
            if rng.random() < 0.15:
                continue                                        # missed instance
            for rep in range(1 + (rng.random() < 0.2)):         # sometimes a duplicate detection
                m = inst_of == g
                flip = rng.random(n) < rng.choice([0.01, 0.05, 0.2, 0.45])
                m = np.where(flip & (np.abs(np.arange(n) - np.nonzero(inst_of == g)[0].mean()) < 3000), ~m, m)
                masks.append(m)
                lab = inst_label[g] if rng.random() < 0.85 else rng.choice(valid[:6])
                labels.append(lab if lab > 2 else valid[0])
                confs.append(rng.random())
        for _ in range(3):                                      # small and spurious detections
            m = np.zeros(n, bool); s0 = rng.integers(0, n - 400); m[s0:s0 + rng.choice([40, 99, 100, 350])] = True
            masks.append(m); labels.append(rng.choice(valid[:6])); confs.append(rng.random())
        masks.append(np.zeros(n, bool)); labels.append(1); confs.append(0.9)     # label outside the benchmark
        pred = {'conf': np.array(confs, np.float32), 'label_id': np.array(labels, np.int32), 'mask': np.stack(masks)}
        name = 'scene%d' % si
        with tempfile.NamedTemporaryFile('w', suffix='.txt', delete=False) as f:
            f.write('\n'.join(str(int(v)) for v in gt_ids) + '\n')
        gt2pred, pred2gt = E.assign_instances_for_scan(name, pred, f.name)
        os.unlink(f.name)
        matches[name] = {'gt': gt2pred, 'pred': pred2gt}
        out['s%d_gt_ids' % si] = gt_ids
        out['s%d_conf' % si] = pred['conf']; out['s%d_label_id' % si] = pred['label_id']
        out['s%d_mask' % si] = np.packbits(pred['mask'], axis=1)
        out['s%d_n' % si] = np.array(n)
    ap, _ = E.evaluate_matches(matches)
    avgs = E.compute_averages(ap)
    out['ap'] = ap
    out['all_ap'] = np.array([avgs['all_ap'], avgs['all_ap_50%'], avgs['all_ap_25%']])
    out['class_ap'] = np.array([[avgs['classes'][c]['ap'], avgs['classes'][c]['ap50%'], avgs['classes'][c]['ap25%']]
                                for c in E.CLASS_LABELS])
    # a one-scene table as well (exercises has_gt / has_pred per class differently)
    ap1, _ = E.evaluate_matches({'scene0': matches['scene0']})
    out['ap_scene0'] = ap1
    np.savez_compressed(os.path.join(OUT, 'eval_metric.npz'), **out)
    print('eval_metric.npz: mAP %.4f  AP50 %.4f  AP25 %.4f' % tuple(out['all_ap']))


def _savez_fixed(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes on every run."""
    import zipfile
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, 'w') as f:
                np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)


ARKIT_IDS = [3, 4, 5, 6, 7, 15, 24, 34]


def detection_scene(rng, si):
    """One synthetic ARKit-shaped room: oriented (yaw-only) ground-truth boxes filled with points, background clutter, and byte
    masks that cover the boxes to varying degrees.  Positions are float32 values (the fixture stores them as such)."""
    g = 9 + si
    centers = np.stack([rng.uniform(0.5, 7.5, g), rng.uniform(0.5, 5.5, g), rng.uniform(0.3, 1.2, g)], 1)
    centers[:, :2] = (np.arange(g)[:, None] * [1.7, 1.1] % [7.0, 5.0]) + 0.5 + rng.uniform(-0.1, 0.1, (g, 2))
    bounds = np.stack([rng.uniform(0.25, 0.6, g), rng.uniform(0.2, 0.5, g), rng.uniform(0.2, 0.5, g)], 1)
    yaw = rng.uniform(-np.pi, np.pi, g)
    yaw[0] = 0.0
    sem = rng.choice(ARKIT_IDS[:5], g)
    sem[g - 1] = 24                                   # a class with ground truth and no prediction
    rot = np.zeros((g, 9))
    pts, owner = [], []
    grid = np.zeros(g, bool)
    grid[[0, 3]] = True                               # objects on a 1 cm grid: many collinear points on the hull
    for i in range(g):
        c, s = np.cos(yaw[i]), np.sin(yaw[i])
        R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        rot[i] = R.T.reshape(-1)                      # the labels store the transpose (evaluation.py:261)
        m = int(rng.integers(250, 600))
        local = rng.uniform(-1.0, 1.0, (m, 3)) * bounds[i]
        if grid[i]:
            R = np.eye(3)
            rot[i] = R.reshape(-1)
            local = np.round(local, 2)
        pts.append(local @ R.T + centers[i])
        owner.append(np.full(m, i))
    nb = 1500
    pts.append(np.stack([rng.uniform(0, 8, nb), rng.uniform(0, 6, nb), rng.uniform(0, 2.4, nb)], 1))
    owner.append(np.full(nb, -1))
    pos = np.concatenate(pts).astype(np.float32)
    owner = np.concatenate(owner)
    perm = rng.permutation(len(pos))
    pos, owner = pos[perm], owner[perm]
    n = len(pos)
    p64 = pos.astype(np.float64)
    masks, labels, confs = [], [], []
    for i in range(g - 1):
        for rep in range(1 + (i % 4 == 1)):           # two predictions on one ground truth
            own = owner == i
            local = (p64 - centers[i])
            cut = rng.choice([-2.0, -0.6, -0.2, 0.15])
            axis = rng.normal(size=2); axis /= np.linalg.norm(axis)
            m = own & (local[:, :2] @ axis > cut * bounds[i, 0])
            near = (np.linalg.norm(local[:, :2], axis=1) < rng.choice([0.3, 0.8])) & (np.abs(local[:, 2]) < 0.4) & (owner == -1)
            m |= near
            masks.append(m); labels.append(sem[i]); confs.append(rng.random())
    small = np.zeros(n, bool); small[np.nonzero(owner == 2)[0][:40]] = True           # under 50 points
    masks.append(small); labels.append(sem[2]); confs.append(rng.random())
    masks.append(owner == 4); labels.append(36)                                       # a class without any ground truth
    confs.append(rng.random())
    other = [c for c in ARKIT_IDS[:5] if c not in sem[[5]]][0]
    masks.append(owner == 5); labels.append(other); confs.append(rng.random())        # right place, wrong class
    masks.append((owner == -1) & (p64[:, 0] < 1.0) & (p64[:, 2] < 1.0)); labels.append(sem[0]); confs.append(rng.random())
    labels_d = {'per_instance_bb_centers': centers.astype(np.float32), 'per_instance_bb_bounds': bounds.astype(np.float32),
                'per_instance_bb_rotations': rot, 'per_instance_semantics': sem.astype(np.int64)}
    pred = {'conf': np.array(confs, np.float32), 'label_id': np.array(labels, np.int32), 'mask': np.stack(masks)}
    return pos, labels_d, pred


def gen_detection():
    """Oriented-box detection metric: ConvexHull hulls as evaluation.py:280-292 takes them, box3d_iou / calc_iou of every
    same-class pair and the reference's own eval_det, from the imported utils.box_util / evaluate_detections / metric_util.
    eval_det's np.array(BB) cannot hold hulls of different vertex counts on this numpy: it is handed (scene, index) handles of
    equal shape and an IoU function that looks the real corner arrays up and calls the reference's get_iou_obb / get_iou."""
    import contextlib
    import io
    _install_stubs()
    pv = types.ModuleType('pyviz3d'); pv.visualizer = types.ModuleType('pyviz3d.visualizer')
    sys.modules['pyviz3d'] = pv; sys.modules['pyviz3d.visualizer'] = pv.visualizer
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from scipy.spatial import ConvexHull
    import utils.box_util as B
    import utils.evaluate_detections as E
    rng = np.random.default_rng(11)
    n_scenes = 4
    out = {'n_scenes': np.array(n_scenes)}
    real = {}                                          # (oriented, scene, 'p' / 'g', index) -> the reference's box
    pred_all = {True: {}, False: {}}
    gt_all = {True: {}, False: {}}
    all_conf = {}
    for si in range(n_scenes):
        pos, labels, pred = detection_scene(rng, si)
        p64 = pos.astype(np.float64)
        name = 'room%d' % si
        g = labels['per_instance_bb_centers'].shape[0]
        for o in (True, False):
            pred_all[o][name] = []; gt_all[o][name] = []
        gcorners, gaabb = [], []
        for i in range(g):                             # evaluation.py:257-270
            bounds = labels['per_instance_bb_bounds'][i].astype(np.float64)
            R = np.reshape(labels['per_instance_bb_rotations'][i], [3, 3]).T
            c = labels['per_instance_bb_centers'][i].astype(np.float64)
            gcorners.append(B.get_oriented_corners(bounds, R, c))
            gaabb.append(np.concatenate([c, B.get_rotated_bounds(bounds, R) * 2.0], 0))
            for o, box in ((True, gcorners[-1]), (False, gaabb[-1])):
                real[(o, si, 'g', i)] = box
                gt_all[o][name].append([labels['per_instance_semantics'][i], np.array([si, i])])
        K = len(pred['conf'])
        count = pred['mask'].sum(1)
        hulls, off, box6 = [], [0], np.zeros((K, 6))
        iou_o = np.zeros((K, g)); iou_a = np.zeros((K, g))
        for r in range(K):                             # evaluation.py:272-299
            positions = p64[pred['mask'][r]]
            if positions.shape[0] < 50:
                off.append(off[-1]); continue
            p2 = positions[:, 0:2]
            hv = p2[ConvexHull(p2).vertices]
            zmin, zmax = np.min(positions[:, 2]), np.max(positions[:, 2])
            prism = np.concatenate([np.concatenate([hv, np.ones([hv.shape[0], 1]) * zmin], 1),
                                    np.concatenate([hv, np.ones([hv.shape[0], 1]) * zmax], 1)], 0)
            pmin, pmax = np.min(positions, 0), np.max(positions, 0)
            aabb = np.concatenate([(pmin + pmax) / 2.0, pmax - pmin], 0)
            hulls.append(hv); off.append(off[-1] + len(hv)); box6[r] = np.concatenate([pmin, pmax])
            for o, box in ((True, prism), (False, aabb)):
                real[(o, si, 'p', r)] = box
                pred_all[o][name].append([pred['label_id'][r], np.array([si, r]), pred['conf'][r]])
            all_conf.setdefault(int(pred['label_id'][r]), []).append(pred['conf'][r])
            for i in range(g):
                if labels['per_instance_semantics'][i] != pred['label_id'][r]:
                    continue
                rect1 = [(prism[j, 0], prism[j, 1]) for j in range(prism.shape[0] // 2, -1, -1)]
                rect2 = [(gcorners[i][j, 0], gcorners[i][j, 1]) for j in range(4)]
                inter = B.polygon_clip(rect1, rect2)
                assert inter is None or len(inter) >= 3, 'degenerate intersection polygon'
                iou_o[r, i] = E.get_iou_obb(prism, gcorners[i])
                iou_a[r, i] = E.get_iou(aabb, gaabb[i])
        for t in (0.5, 0.25):
            assert np.abs(iou_o - t).min() > 1e-6 and np.abs(iou_a - t).min() > 1e-6, 'an IoU within 1e-6 of a threshold'
        out['s%d_pos' % si] = pos
        out['s%d_mask' % si] = np.packbits(pred['mask'], axis=1)
        out['s%d_n' % si] = np.array(len(pos))
        out['s%d_conf' % si] = pred['conf']; out['s%d_label_id' % si] = pred['label_id']
        for k, v in labels.items():
            out['s%d_%s' % (si, k)] = v
        out['s%d_count' % si] = count.astype(np.int64)
        out['s%d_hull' % si] = np.concatenate(hulls, 0); out['s%d_hull_off' % si] = np.array(off, np.int64)
        out['s%d_box6' % si] = box6
        out['s%d_iou_obb' % si] = iou_o; out['s%d_iou_aabb' % si] = iou_a
        out['s%d_hull_max' % si] = np.array(max(len(h) for h in hulls))
    for c, v in all_conf.items():
        assert len(set(float(x) for x in v)) == len(v), 'equal confidences in class %d' % c

    def iou_of(o, fn):
        def f(a, b):
            return fn(real[(o, int(a[0]), 'p', int(a[1]))], real[(o, int(b[0]), 'g', int(b[1]))])
        return f

    for o, tag, fn in ((True, 'obb', E.get_iou_obb), (False, 'aabb', E.get_iou)):
        for t in (0.5, 0.25):
            with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
                rec, prec, ap = E.eval_det(pred_all[o], gt_all[o], ovthresh=t, get_iou_func=iou_of(o, fn))
            key = '%s_%d' % (tag, round(t * 100))
            cls = np.array([int(c) for c in ap.keys()], np.int64)
            out[key + '_classes'] = cls
            out[key + '_ap'] = np.array([ap[c] for c in ap.keys()], np.float64)
            for c in ap.keys():
                out['%s_rec_%d' % (key, int(c))] = np.asarray(rec[c], np.float64)
                out['%s_prec_%d' % (key, int(c))] = np.asarray(prec[c], np.float64)
            vals = [v for v in ap.values() if not np.isnan(v)]
            out[key + '_map'] = np.array(np.mean(np.array(vals)))
            print('eval_detection %s: mAP %.4f over %d classes (%s)' % (key, out[key + '_map'], len(vals),
                                                                       ' '.join('%d:%.3f' % (int(c), ap[c]) for c in ap)))
    _savez_fixed(os.path.join(OUT, 'eval_detection.npz'), out)
    print('eval_detection.npz: %d bytes, largest hull %d vertices'
          % (os.path.getsize(os.path.join(OUT, 'eval_detection.npz')), max(int(out['s%d_hull_max' % s]) for s in range(n_scenes))))


S3DIS_GRID = 1.0 / 128.0
S3DIS_NORMALS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)


def s3dis_room(rng, ri, planes=(5000, 5000, 3600, 3400, 2200), per_object=(700, 1000)):
    """One synthetic S3DIS-shaped room on an integer grid of 1/128 m with axis normals: ceiling, floor, two large walls, a wall of
    fewer than 3000 points, furniture of classes 3 .. 12 (room 2 has no class 12), predicted semantics with a few wrong points
    (some of them stray `wall` points) and proposals that the merge accepts or rejects by each of its three tests."""
    L, W, H = 640, 512, 333
    parts = []                                        # (grid (m, 3), normal index (m), class, instance)

    def plane(m, axis, value, lo, hi, normal, cls, inst):
        g = np.stack([rng.integers(lo[j], hi[j] + 1, m) for j in range(3)], 1)
        g[:, axis] = value
        parts.append((g, np.full(m, normal), cls, inst))

    plane(planes[0], 2, H, (0, 0, 0), (L, W, 0), 5, 0, 0)
    plane(planes[1], 2, 0, (0, 0, 0), (L, W, 0), 4, 1, 1)
    plane(planes[2], 1, 0, (0, 0, 0), (L, 0, H), 2, 2, 2)
    plane(planes[3], 0, 0, (0, 0, 0), (0, W, H), 0, 2, 3)
    plane(planes[4], 1, W, (0, 0, 0), (L, 0, H), 3, 2, 4)
    classes = list(range(3, 13)) + [5] if ri < 2 else list(range(3, 12)) + [5]
    boxes = []
    for i, cls in enumerate(classes):
        cx, cy = 90 + (i % 4) * 150, 90 + (i // 4) * 150
        sx, sy, sz = (int(v) for v in rng.integers(35, 60, 3))
        m = int(rng.integers(per_object[0], per_object[1]))
        g = np.stack([rng.integers(cx - sx, cx + sx + 1, m), rng.integers(cy - sy, cy + sy + 1, m), rng.integers(1, 2 * sz, m)], 1)
        parts.append((g, rng.integers(0, 6, m), cls, 5 + i))
        boxes.append((cx, cy, sx, sy))
    grid = np.concatenate([q[0] for q in parts]).astype(np.int16)
    normal = np.concatenate([q[1] for q in parts]).astype(np.int8)
    gt_sem = np.concatenate([np.full(len(q[0]), q[2]) for q in parts]).astype(np.int64)
    gt_ins = np.concatenate([np.full(len(q[0]), q[3]) for q in parts]).astype(np.int64)
    n = len(grid)
    perm = rng.permutation(n)
    grid, normal, gt_sem, gt_ins = grid[perm], normal[perm], gt_sem[perm], gt_ins[perm]
    pred = gt_sem.copy()
    obj = np.nonzero(gt_sem >= 3)[0]
    wrong = rng.choice(obj, len(obj) // 100, replace=False)
    pred[wrong] = rng.choice(sorted(set(classes)), len(wrong))
    pred[rng.choice(obj, 60, replace=False)] = 2                                   # stray wall points
    wall_a = np.nonzero(gt_ins == 2)[0]
    pred[rng.choice(wall_a, 150, replace=False)] = 0                               # a few wall points taken for ceiling
    masks = []

    def subset(idx, keep):
        m = np.zeros(n, bool)
        m[rng.choice(idx, int(len(idx) * keep), replace=False)] = True
        return m

    def of(i):
        return np.nonzero(gt_ins == 5 + i)[0]

    floor = np.nonzero(gt_ins == 1)[0]
    masks.append(subset(of(0), 0.9))                                               # accepted
    masks.append(subset(of(0), 0.85))                                              # rejected: under 0.6 of it is still unlabeled
    cx, cy, sx, sy = boxes[1]
    near = floor[np.argsort(np.abs(grid[floor, 0] - cx) + np.abs(grid[floor, 1] - cy), kind='stable')[:150]]
    m = subset(of(1), 0.9); m[near] = True
    masks.append(m)                                                                # accepted, repaints 150 floor points
    masks.append(subset(floor, 0.12))                                              # rejected: semantic class below 3
    m = np.zeros(n, bool); m[of(2)[:150]] = True
    masks.append(m)                                                                # rejected: fewer than 200 points
    masks.append(subset(of(2), 0.9))
    keeps = [0.95, 0.55, 0.4, 0.9, 0.8, 0.9, 0.9, 0.9]
    for i in range(3, len(classes) - 1):                                           # the last object gets no proposal
        masks.append(subset(of(i), keeps[(i - 3) % len(keeps)]))
    masks.append(subset(np.nonzero(gt_ins == 3)[0], 0.3))                          # a wall: class 2, rejected
    return grid, normal, gt_sem, gt_ins, pred, np.stack(masks)


def s3dis_dbscan_case(seed, eps=0.2, min_samples=5, sig=0.09, sep=2.5, ncl=80, per=25, n=6000):
    """6000 rows in 6-D (float32 values): Gaussian blobs in touching pairs, in uniform noise."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0, 2.0, (ncl, 6))
    u = rng.normal(size=(ncl // 2, 6))
    c[1::2] = c[0::2] + u / np.linalg.norm(u, axis=1, keepdims=True) * sep * eps
    pts = [c[i] + rng.normal(0, sig, (per, 6)) for i in range(ncl)]
    pts.append(rng.uniform(-0.2, 2.2, (n - ncl * per, 6)))
    x = np.concatenate(pts).astype(np.float32)
    return x[rng.permutation(len(x))], eps, min_samples


def _s3dis_eval_modules():
    """models/evaluation.py and utils/s3dis_util.py of the reference, imported unmodified behind the stand-ins gen_s3dis describes;
    also the stand-in of dataprocessing.s3dis the evaluation module reads its scene names (and the unsampled rooms) through."""
    D = _dataloader_module()
    for name in ('pyviz3d', 'pyviz3d.visualizer', 'quaternion', 'natsort', 'tensorboard', 'torch.utils.tensorboard'):
        try:
            __import__(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)
    sys.modules['pyviz3d'].visualizer = sys.modules['pyviz3d.visualizer']
    if not hasattr(sys.modules['torch.utils.tensorboard'], 'SummaryWriter'):
        sys.modules['torch.utils.tensorboard'].SummaryWriter = object
    if not hasattr(np, 'float'):
        np.float = float
    for n in ('scannet', 'arkitscenes', 's3dis'):
        m = sys.modules['dataprocessing.' + n]
        for attr in ('SCANNET', 'ARKITSCENES', 'S3DIS'):
            for tail in ('_SEMANTIC_VALID_CLASS_IDS', '_SEMANTIC_ID2IDX', '_INSTANCE_ID2IDX'):
                if not hasattr(m, attr + tail):
                    setattr(m, attr + tail, None)
    s3 = sys.modules['dataprocessing.s3dis']
    s3.get_scene_names = lambda mode, cfg: []
    s3.ID2NAME = ['class%d' % c for c in range(13)]
    import models.evaluation as EV
    import utils.s3dis_util as SU
    if EV.s3dis is not s3:                           # imported by an earlier target: it holds that target's stand-in
        s3 = EV.s3dis
        s3.get_scene_names = lambda mode, cfg: []
        s3.ID2NAME = ['class%d' % c for c in range(13)]
    return EV, SU, s3


def gen_s3dis():
    """S3DIS evaluation: tests/golden/eval_s3dis.npz from the reference's own code, imported unmodified -- utils/s3dis_util.py
    (clustering_for_background, assign_semantics_to_proposals, s3dis_eval; sklearn's DBSCAN inside) and Evaluater.s3dis_eval
    (models/evaluation.py:124-241), which is DRIVEN here for the merge stage: a fake model hands it the fixture's per-voxel logits
    and masks, a list is the loader, s3dis.get_scene_names is a stub and s3dis_util's three functions are wrapped to record what
    goes through them.  pyviz3d, quaternion, natsort and tensorboard get empty stand-ins where missing; np.float (gone from numpy)
    is restored in this process only.  The fixture holds data only: positions as int16 steps of 1/128 m, normals as indices into
    the six axis directions, masks bit-packed."""
    import contextlib
    import io
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from _s3dis_rule import dbscan_rule, margin
    EV, SU, s3 = _s3dis_eval_modules()
    from sklearn.cluster import DBSCAN

    out = {}
    # ---- DBSCAN-only cases
    seed = 100
    for ci in range(2):
        while True:
            seed += 1
            x, eps, ms = s3dis_dbscan_case(seed)
            x64 = x.astype(np.float64)
            fit = DBSCAN(eps=eps, min_samples=ms).fit(x64)
            lab = fit.labels_
            core = np.zeros(len(x), bool); core[fit.core_sample_indices_] = True
            rule, rcore, two = dbscan_rule(x64, eps, ms)
            assert np.array_equal(rule, lab) and np.array_equal(rcore, core), 'the labelling rule does not reproduce sklearn'
            ok = lab.max() + 1 >= 50 and ((lab >= 0) & ~core).sum() >= 500 and (lab < 0).sum() >= 1000 and two.sum() >= 20 and \
                margin(x64, eps) >= 1e-12
            if ok:
                break
        perm = np.random.default_rng(seed + 1000).permutation(len(x))
        lab_p = DBSCAN(eps=eps, min_samples=ms).fit(x64[perm]).labels_
        out['db%d_x' % ci] = x
        out['db%d_eps' % ci] = np.float64(eps); out['db%d_min_samples' % ci] = np.int64(ms)
        out['db%d_labels' % ci] = lab.astype(np.int16); out['db%d_core' % ci] = np.packbits(core)
        out['db%d_perm' % ci] = perm.astype(np.int16); out['db%d_labels_perm' % ci] = lab_p.astype(np.int16)
        print('eval_s3dis db%d: seed %d, %d clusters, %d border (%d between two clusters), %d noise, margin %.2e'
              % (ci, seed, lab.max() + 1, ((lab >= 0) & ~core).sum(), two.sum(), (lab < 0).sum(), margin(x64, eps)))

    # ---- rooms through Evaluater.s3dis_eval
    rng = np.random.default_rng(2024)
    rooms = [s3dis_room(rng, ri) for ri in range(3)]
    batches, by_name = [], {}
    for ri, (grid, normal, gt_sem, gt_ins, pred, masks) in enumerate(rooms):
        name = 'room%d' % ri
        scene = {'name': name, 'positions': grid.astype(np.float64) * S3DIS_GRID, 'normals': S3DIS_NORMALS[normal]}
        labels = {'semantics': gt_sem, 'instances': gt_ins}
        n = len(grid)
        batches.append({'scene': [scene], 'labels': [labels], 'vox2point': [np.arange(n)]})
        by_name[name] = (pred, masks)

    class FakeModel:
        def get_prediction(self, batch, with_grad=False, to_cpu=True, min_size=True):
            pred, _ = by_name[batch['scene'][0]['name']]
            return {'mlp_per_vox_semantics': torch.from_numpy(np.eye(13, dtype=np.float32)[pred])}

        def pred2mask(self, batch, prediction, mode='eval'):
            name = batch['scene'][0]['name']
            return {name: {'mask': by_name[name][1].astype(np.uint8)}}

    seen = {'background': [], 'proposal_semantics': [], 'wall_features': []}
    real_bg, real_assign, real_eval = SU.clustering_for_background, SU.assign_semantics_to_proposals, SU.s3dis_eval

    def bg(pred_semantics, coords, normals):
        r = real_bg(pred_semantics, coords, normals)
        seen['background'].append(r.copy())
        w = pred_semantics == 2
        seen['wall_features'].append(np.concatenate([coords[w], normals[w] * 2], 1))
        return r

    def assign(pred_semantics, masks):
        r = real_assign(pred_semantics, masks)
        seen['proposal_semantics'].append(np.array(r))
        return r

    def ev(pred_labels, gt_labels):
        seen['pred_labels'], seen['gt_labels'] = pred_labels, gt_labels
        with np.errstate(all='ignore'):
            return real_eval(pred_labels, gt_labels)

    SU.clustering_for_background, SU.assign_semantics_to_proposals, SU.s3dis_eval = bg, assign, ev
    evaluater = object.__new__(EV.Evaluater)
    evaluater.model = FakeModel()
    evaluater.cfg = SimpleNamespace(eval_ths=[0.5, 0.03, 0.3, 0.6], s3dis_split_fold=5, full_resolution=False)
    loader = SimpleNamespace(get_loader=lambda **kw: batches)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            evaluater.s3dis_eval(loader)
    finally:
        SU.clustering_for_background, SU.assign_semantics_to_proposals, SU.s3dis_eval = real_bg, real_assign, real_eval
    out['n_rooms'] = np.array(3)
    for ri, (grid, normal, gt_sem, gt_ins, pred, masks) in enumerate(rooms):
        fin = seen['pred_labels'][ri]
        bgr = seen['background'][ri]
        f = seen['wall_features'][ri]
        assert margin(f, 0.35) >= 1e-12, 'a wall pair within 1e-12 of eps'
        rule, _, _ = dbscan_rule(f, 0.35, 10)
        assert np.array_equal(rule, DBSCAN(eps=0.35, min_samples=10).fit(f).labels_)
        walls = np.unique(bgr[bgr >= 3])
        sizes = np.bincount(rule[rule >= 0])
        assert len(walls) == 2 and (sizes >= 3000).sum() == 2 and ((sizes < 3000) & (sizes > 1000)).sum() == 1 and (rule < 0).sum() >= 10, \
            (walls, sizes, (rule < 0).sum())
        # the merge: each rejection test decides at least once
        ps = seen['proposal_semantics'][ri]
        acc = np.array([(fin['instances'] == k + 1).any() for k in range(len(masks))])
        assert ps[3] < 3 and ps[-1] < 3 and not acc[1] and ps[1] >= 3 and not acc[4] and ps[4] >= 3 and acc[0] and acc[2] and acc[5]
        # the floor points proposal 2 repainted: background instance, a furniture class, under 200 -> removed
        repainted = (bgr == 2) & (fin['semantics'] != 1)
        assert 100 <= repainted.sum() < 200 and (fin['instances'][repainted] == -1).all()
        for lab in (gt_sem, fin['semantics']):
            assert set(np.unique(lab)) == (set(range(13)) if ri < 2 else set(range(12)))
        out['r%d_n' % ri] = np.array(len(grid))
        out['r%d_grid' % ri] = grid; out['r%d_normal' % ri] = normal
        out['r%d_gt_semantics' % ri] = gt_sem.astype(np.int8); out['r%d_gt_instances' % ri] = gt_ins.astype(np.int16)
        out['r%d_pred_semantics' % ri] = pred.astype(np.int8)
        out['r%d_masks' % ri] = np.packbits(masks, axis=1)
        out['r%d_background' % ri] = bgr.astype(np.int16)
        out['r%d_proposal_semantics' % ri] = ps.astype(np.int8)
        out['r%d_final_semantics' % ri] = np.asarray(fin['semantics']).astype(np.int8)
        out['r%d_final_instances' % ri] = np.asarray(fin['instances']).astype(np.int16)
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        both = real_eval(seen['pred_labels'][:2], seen['gt_labels'][:2])
        alone = real_eval(seen['pred_labels'][2:], seen['gt_labels'][2:])
    assert np.isfinite(both[0]) and np.isfinite(both[1]) and np.isnan(alone[2][12]) and np.isnan(alone[3][12])
    assert 0 < both[0] < 1 and 0 < both[1] < 1
    for tag, r in (('rooms01', both), ('room2', alone)):
        out[tag + '_mprec'] = np.float64(r[0]); out[tag + '_mrec'] = np.float64(r[1])
        out[tag + '_precision'] = np.asarray(r[2], np.float64); out[tag + '_recall'] = np.asarray(r[3], np.float64)
    path = os.path.join(OUT, 'eval_s3dis.npz')
    _savez_fixed(path, out)
    assert os.path.getsize(path) <= 1000000, os.path.getsize(path)
    print('eval_s3dis.npz: %d bytes; rooms 0-1 mPrec %.4f mRec %.4f; room 2 alone mPrec %s' % (os.path.getsize(path), both[0], both[1], alone[0]))


def gen_s3dis_labels():
    """Label transfer of the raw S3DIS dataset: tests/golden/s3dis_labels.npz from the reference's own get_labels
    (dataprocessing/prepare_s3dis.py:71-121), imported unmodified.  The module parses its arguments and runs its main loop on
    import, so it is imported with a patched sys.argv whose --data_dir is an empty directory (the loop finds no room), behind
    stand-ins for skimage, open3d, pyviz3d, natsort and configargparse (argparse's parser) where they are missing.  get_labels then
    runs over a temporary directory of synthetic Annotations/*.txt files with glob.glob wrapped to return a sorted list (the
    reference takes the order of an unsorted glob) and scipy's KDTree wrapped to record the match distances, whose sum the
    reference accumulates and drops; np.loadtxt is called with ndmin=2 meanwhile, because get_labels cannot index the vector a
    file of ONE row loads as, and the fixture has a cloud of one point.  The fixture holds what the reference loaded -- the room's points and every cloud after
    np.loadtxt, the file names -- and what it returned."""
    import argparse
    import glob as glob_module
    import importlib
    import tempfile
    for name in ('skimage', 'skimage.io', 'open3d', 'pyviz3d', 'pyviz3d.visualizer', 'natsort', 'configargparse'):
        try:
            __import__(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)
    sys.modules['skimage'].io = sys.modules['skimage.io']
    sys.modules['pyviz3d'].visualizer = sys.modules['pyviz3d.visualizer']
    if not hasattr(sys.modules['natsort'], 'natsorted'):
        sys.modules['natsort'].natsorted = sorted
    if not hasattr(sys.modules['configargparse'], 'ArgumentParser'):
        sys.modules['configargparse'].ArgumentParser = argparse.ArgumentParser
    for name in [k for k in sys.modules if k == 'dataprocessing' or k.startswith('dataprocessing.')]:
        del sys.modules[name]                                   # the empty stand-ins of the other targets
    if REF not in sys.path:
        sys.path.insert(0, REF)

    rng = np.random.default_rng(4711)
    # name of the annotation file, points; sorted by name this is the order of the clouds
    sizes = [('beam_1', 150), ('board_1', 1), ('ceiling_1', 400), ('chair_1', 3), ('chair_2', 220), ('clutter_1', 180),
             ('floor_1', 400), ('stairs_1', 120), ('table_1', 200), ('wall_1', 350)]
    centres = rng.uniform(0, 1, (len(sizes), 3)) * np.array([8.0, 6.0, 3.0])
    clouds = [np.round(c + rng.normal(0, 0.4, (m, 3)), 6) for (_, m), c in zip(sizes, centres)]
    scene = np.concatenate(clouds)                              # the room file is the concatenation of its annotations ...
    scene = np.concatenate([scene, np.round(rng.uniform(-1, 1, (600, 3)) * 0.5 + scene[rng.integers(0, len(scene), 600)], 6)])
    scene = scene[rng.permutation(len(scene))]                  # ... here with 600 points that are in no cloud, in shuffled order
    assert len(np.unique(scene, axis=0)) == len(scene)
    # chair_1's three points are chair_2's first three: its id disappears in the remap; table_1 claims a point of clutter_1 and wall_1
    # one of floor_1; a fifth of every larger cloud is off its scene point by up to 2 mm (a match distance above zero)
    clouds[4][:3] = clouds[3]
    clouds[8][0] = clouds[5][0]
    clouds[9][0] = clouds[6][0]
    for c in clouds:
        if len(c) >= 100:
            k = len(c) // 5
            c[-k:] = np.round(c[-k:] + rng.uniform(-0.002, 0.002, (k, 3)), 6)

    with tempfile.TemporaryDirectory() as tmp:
        empty = os.path.join(tmp, 'empty'); os.makedirs(empty)
        ann = os.path.join(tmp, 'data', 'Area_9', 'room_1', 'Annotations'); os.makedirs(ann)
        for (name, _), c in zip(sizes, clouds):
            np.savetxt(os.path.join(ann, name + '.txt'), np.concatenate([c, rng.integers(0, 256, (len(c), 3))], 1), fmt='%.6f')
        np.savetxt(os.path.join(tmp, 'room_1.txt'), np.concatenate([scene, rng.integers(0, 256, (len(scene), 3))], 1), fmt='%.6f')
        argv = sys.argv
        sys.argv = ['prepare_s3dis.py', '--data_dir', empty]
        try:
            PS = importlib.import_module('dataprocessing.prepare_s3dis')
        finally:
            sys.argv = argv
        seen = []
        real_tree, real_glob, real_loadtxt = PS.KDTree, glob_module.glob, np.loadtxt

        class Tree(real_tree):
            def query(self, *a, **k):
                r = super().query(*a, **k)
                seen.append((np.array(r[0], copy=True), np.array(r[1], copy=True)))
                return r

        PS.KDTree = Tree
        glob_module.glob = lambda *a, **k: sorted(real_glob(*a, **k))
        np.loadtxt = lambda pth: real_loadtxt(pth, ndmin=2)        # (a file of one row loads as a vector, which get_labels cannot index)
        try:
            scene_data = np.loadtxt(os.path.join(tmp, 'room_1.txt'))
            paths = glob_module.glob(ann + '/*.txt')
            loaded = [np.loadtxt(pth) for pth in paths]
            instances, semantics = PS.get_labels('Area_9.room_1', scene_data, os.path.join(tmp, 'data'))
        finally:
            PS.KDTree, glob_module.glob, np.loadtxt = real_tree, real_glob, real_loadtxt
    names = [os.path.basename(pth)[:-4] for pth in paths]
    assert names == [n for n, _ in sizes] and len(seen) == len(sizes) + 1
    class_ids = np.array([PS.NAME2ID['clutter' if n.split('_')[0] == 'stairs' else n.split('_')[0]] for n in names], np.int64)
    pts = scene_data[:, :3]
    # what the fixture must contain, and that no match is decided by a tie (the k-d tree's choice there is an artefact)
    claims = np.zeros(len(pts), np.int64)
    for (d, i) in seen[:-1]:
        claims[np.unique(i)] += 1
    assert (claims == 0).sum() >= 500 and (claims >= 2).sum() >= 3 and min(len(c) for c in loaded) == 1
    assert len(np.unique(instances)) == len(sizes) - 1 and instances.max() == len(sizes) - 2
    assert instances.dtype == np.float32 and semantics.dtype == np.float32 and instances.shape == semantics.shape == (len(pts), 1)
    decided = claims > 0
    for qs, rs in [(c[:, :3], pts) for c in loaded] + [(pts[~decided], pts[decided])]:
        dx, dy, dz = (qs[:, None, j] - rs[None, :, j] for j in range(3))
        d2 = np.sort((dx * dx + dy * dy) + dz * dz, 1)[:, :2]
        assert (d2[:, 1] - d2[:, 0] > 1e-9 * d2[:, 0]).all(), 'a match within a relative 1e-9 of a tie'
    error = 0
    for (d, i) in seen[:-1]:
        error += d.sum()                                          # prepare_s3dis.py:98
    assert error > 0
    out = {'scene_pts': pts, 'names': np.array(names), 'class_ids': class_ids, 'instances': instances, 'semantics': semantics,
           'error': np.float64(error), 'n_clouds': np.array(len(loaded))}
    for k, c in enumerate(loaded):
        out['cloud%d' % k] = c.reshape(-1, 6)[:, :3]
    path = os.path.join(OUT, 's3dis_labels.npz')
    _savez_fixed(path, out)
    assert os.path.getsize(path) <= 1000000, os.path.getsize(path)
    print('s3dis_labels.npz: %d bytes; %d points, %d in no cloud, %d claimed twice, error %.6f'
          % (os.path.getsize(path), len(pts), (claims == 0).sum(), (claims >= 2).sum(), error))


def s3dis_full_room(rng, ri):
    """A room for the full-resolution evaluation: the SAMPLED room is an s3dis_room of about 11 000 points (one wall large enough
    to survive the 3000-point rule); the full room has four times as many, rows [::4] being the sampled ones as the reference
    samples, the others copies of random sampled points moved by up to two grid steps per axis, with their source's ground truth.
    No two sampled points coincide and no full point has two nearest sampled points at the same distance (checked exactly, on the
    integer grid): the trees' choice there is a traversal artefact."""
    grid, normal, gt_sem, gt_ins, pred, masks = s3dis_room(rng, ri, planes=(300, 500, 3300, 200, 150), per_object=(520, 640))
    grid = grid.astype(np.int64)
    while True:
        _, first = np.unique(grid, axis=0, return_index=True)
        dup = np.setdiff1d(np.arange(len(grid)), first)
        if len(dup) == 0:
            break
        grid[dup] = np.maximum(grid[dup] + rng.integers(-2, 3, (len(dup), 3)), 0)
    n = len(grid)
    full = np.zeros((4 * n, 3), np.int64)
    src = np.zeros(4 * n, np.int64)
    src[0::4] = np.arange(n)
    full[0::4] = grid
    todo = np.nonzero(np.arange(4 * n) % 4 != 0)[0]
    while len(todo):
        src[todo] = rng.integers(0, n, len(todo))
        full[todo] = np.maximum(grid[src[todo]] + rng.integers(-2, 3, (len(todo), 3)), 0)
        tied = []
        for s in range(0, len(todo), 2048):
            rows = todo[s:s + 2048]
            d2 = ((full[rows, None, :] - grid[None, :, :]) ** 2).sum(2)
            two = np.partition(d2, 1, axis=1)[:, :2]
            tied.append(rows[two[:, 0] == two[:, 1]])
        todo = np.concatenate(tied)
    return dict(grid=grid.astype(np.int16), normal=normal, gt_sem=gt_sem, gt_ins=gt_ins, pred=pred, masks=masks,
                full=full.astype(np.int16), full_sem=gt_sem[src], full_ins=gt_ins[src])


def gen_s3dis_full():
    """Full-resolution S3DIS evaluation: tests/golden/eval_s3dis_full.npz from Evaluater.s3dis_eval driven as in gen_s3dis, with
    cfg.full_resolution = True, s3dis.process_scene replaced by a function that returns the full room, and get_sparse2dense --
    which the reference calls (evaluation.py:154) and defines nowhere -- put into the evaluation module's namespace as the sklearn
    ball-tree lookup of the nearest sampled point.  The sampled room is rows [::4] of the full one.  Data only: positions as int16
    steps of 1/128 m, normals as indices into the six axis directions, masks bit-packed."""
    import contextlib
    import io
    from sklearn.neighbors import NearestNeighbors
    EV, SU, s3 = _s3dis_eval_modules()
    rng = np.random.default_rng(2025)
    rooms = [s3dis_full_room(rng, ri) for ri in range(2)]
    batches, by_name, full_by_name = [], {}, {}
    for ri, rm in enumerate(rooms):
        name = 'room%d' % ri
        full_pos = rm['full'].astype(np.float64) * S3DIS_GRID
        scene = {'name': name, 'positions': full_pos[::4], 'normals': S3DIS_NORMALS[rm['normal']]}
        assert np.array_equal(scene['positions'], rm['grid'].astype(np.float64) * S3DIS_GRID)
        labels = {'semantics': rm['gt_sem'], 'instances': rm['gt_ins']}
        batches.append({'scene': [scene], 'labels': [labels], 'vox2point': [np.arange(len(rm['grid']))]})
        by_name[name] = (rm['pred'], rm['masks'])
        full_by_name[name] = ({'name': name, 'positions': full_pos}, {'semantics': rm['full_sem'], 'instances': rm['full_ins']})

    class FakeModel:
        def get_prediction(self, batch, with_grad=False, to_cpu=True, min_size=True):
            pred, _ = by_name[batch['scene'][0]['name']]
            return {'mlp_per_vox_semantics': torch.from_numpy(np.eye(13, dtype=np.float32)[pred])}

        def pred2mask(self, batch, prediction, mode='eval'):
            name = batch['scene'][0]['name']
            return {name: {'mask': by_name[name][1].astype(np.uint8)}}

    seen = {'s2d': []}
    real_eval = SU.s3dis_eval

    def ev(pred_labels, gt_labels):
        seen['pred_labels'], seen['gt_labels'] = pred_labels, gt_labels
        with np.errstate(all='ignore'):
            seen['result'] = real_eval(pred_labels, gt_labels)
        return seen['result']

    def get_sparse2dense(scene_full, scene, cfg):
        tree = NearestNeighbors(n_neighbors=1, algorithm='ball_tree').fit(scene['positions'])
        s2d = tree.kneighbors(scene_full['positions'], return_distance=False)[:, 0]
        seen['s2d'].append(s2d)
        return s2d

    SU.s3dis_eval = ev
    EV.get_sparse2dense = get_sparse2dense
    s3.process_scene = lambda name, mode, cfg: full_by_name[name]
    evaluater = object.__new__(EV.Evaluater)
    evaluater.model = FakeModel()
    evaluater.cfg = SimpleNamespace(eval_ths=[0.5, 0.03, 0.3, 0.6], s3dis_split_fold=5, full_resolution=True, point_sampling_rate=4)
    loader = SimpleNamespace(get_loader=lambda **kw: batches)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            evaluater.s3dis_eval(loader)
    finally:
        SU.s3dis_eval = real_eval
        del EV.get_sparse2dense, s3.process_scene
    assert evaluater.cfg.point_sampling_rate is None                                   # evaluation.py:152
    mprec, mrec, prec, rec = seen['result']
    assert np.isfinite(mprec) and np.isfinite(mrec) and 0 < mprec < 1 and 0 < mrec < 1
    out = {'n_rooms': np.array(2), 'mprec': np.float64(mprec), 'mrec': np.float64(mrec), 'precision': np.asarray(prec, np.float64),
           'recall': np.asarray(rec, np.float64)}
    for ri, rm in enumerate(rooms):
        s2d, fin, gt = seen['s2d'][ri], seen['pred_labels'][ri], seen['gt_labels'][ri]
        n, nf = len(rm['grid']), len(rm['full'])
        assert nf == 4 * n and np.array_equal(s2d[::4], np.arange(n)) and (s2d != np.arange(nf) // 4).sum() > nf // 4
        assert len(fin['instances']) == nf and len(gt['instances']) == nf
        ins = np.asarray(fin['instances'])
        walls = (np.asarray(fin['semantics']) == 2) & (ins > 0)
        assert walls.sum() >= 4 * 3000 * 0.9 and len(np.unique(ins[ins >= 0])) >= 8, 'the large wall or the proposals did not survive'
        out['r%d_full' % ri] = rm['full']; out['r%d_sampled' % ri] = rm['grid']; out['r%d_normal' % ri] = rm['normal']
        out['r%d_pred_semantics' % ri] = rm['pred'].astype(np.int8)
        out['r%d_masks' % ri] = np.packbits(rm['masks'], axis=1)
        out['r%d_gt_semantics' % ri] = rm['gt_sem'].astype(np.int8); out['r%d_gt_instances' % ri] = rm['gt_ins'].astype(np.int8)
        out['r%d_sparse2dense' % ri] = s2d.astype(np.int16)
        out['r%d_full_pred_semantics' % ri] = np.asarray(fin['semantics']).astype(np.int8)
        out['r%d_full_pred_instances' % ri] = ins.astype(np.int8)
        out['r%d_full_gt_semantics' % ri] = np.asarray(gt['semantics']).astype(np.int8)
        out['r%d_full_gt_instances' % ri] = np.asarray(gt['instances']).astype(np.int8)
        for k in ('full_pred_semantics', 'full_pred_instances', 'full_gt_semantics', 'full_gt_instances'):
            src = {'full_pred_semantics': fin['semantics'], 'full_pred_instances': ins, 'full_gt_semantics': gt['semantics'],
                   'full_gt_instances': gt['instances']}[k]
            assert np.array_equal(out['r%d_%s' % (ri, k)], np.asarray(src)), k         # (nothing lost in the narrow types)
    path = os.path.join(OUT, 'eval_s3dis_full.npz')
    _savez_fixed(path, out)
    assert os.path.getsize(path) <= 1000000, os.path.getsize(path)
    print('eval_s3dis_full.npz: %d bytes; %s full points; mPrec %.4f mRec %.4f'
          % (os.path.getsize(path), [len(rm['full']) for rm in rooms], mprec, mrec))


def gen_augment():
    """Augmentation and label recomputation: tests/golden/augment.npz from the reference's own elastic_distortion, HAIS_elastic,
    ChromaticAutoContrast, ChromaticTranslation, color_jittering (dataprocessing/augmentation.py) and compute_bounding_box
    (dataprocessing/scannet.py), imported unmodified through stand-ins for open3d, albumentations, pyviz3d and configargparse.
    While they run, scipy.ndimage.filters.convolve and scipy.interpolate.RegularGridInterpolator are wrapped to record the drawn
    noise, the blurred grid and the axes; the blend / translation / jitter operands are re-drawn from the recorded seeds.  The
    one case the reference's functions cannot reach -- points outside the axes and on the last node -- goes through the same
    RegularGridInterpolator call with the same arguments.  Data only; the same bytes on every run.  Every case records the
    output of every step; the per-step outputs of the 5000-point case go to a second file, tests/golden/augment_steps.npz,
    because no committed file may exceed 1 MiB (together the two stay far below the largest fixture)."""
    import random
    import scipy
    import scipy.interpolate
    import scipy.ndimage
    import scipy.ndimage.filters
    _install_stubs()
    alb = types.ModuleType('albumentations')
    alb.load = lambda *a, **k: None
    for n in ('Normalize', 'Compose', 'HueSaturationValue', 'RandomBrightnessContrast'):
        setattr(alb, n, lambda *a, **k: None)
    sys.modules['albumentations'] = alb
    for name in ('pyviz3d', 'pyviz3d.visualizer', 'configargparse'):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules['pyviz3d'].visualizer = sys.modules['pyviz3d.visualizer']
    for name in [k for k in sys.modules if k == 'dataprocessing' or k.startswith('dataprocessing.')]:
        del sys.modules[name]                                   # the empty stand-ins of the prepare targets
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import dataprocessing.augmentation as AUG
    import dataprocessing.scannet as SC

    calls, axes = [], []
    steps_out = {}
    real_convolve, real_rgi = scipy.ndimage.filters.convolve, scipy.interpolate.RegularGridInterpolator

    def convolve(x, w, **kw):
        y = real_convolve(x, w, **kw)
        calls.append((np.array(x, copy=True), np.array(y, copy=True)))
        return y

    def rgi(ax, values, **kw):
        axes.append([np.array(a, copy=True) for a in ax])
        return real_rgi(ax, values, **kw)

    scipy.ndimage.filters.convolve = convolve
    scipy.interpolate.RegularGridInterpolator = rgi
    out = {}
    rng = np.random.default_rng(606)
    metre = (AUG.SCANNET_ELASTIC_DISTORT_PARAMS, ((6.0, 40.0), (20.0, 160.0)))         # scannet.py:190, :196-197 at 2 cm voxels
    # name, points, lower corner, extent, (elastic params, hais params)
    cases = [('p1', 1, (0.3, 0.2, 0.1), (1, 1, 1), metre), ('p63', 63, (0, 0, 0), (1.1, 0.9, 0.5), metre),
             ('p64', 64, (0, 0, 0), (1.1, 0.9, 0.5), metre), ('p65', 65, (0.5, 0.1, 0), (1.1, 0.9, 0.5), metre),
             ('p1000', 1000, (0, 0, 0), (2.0, 1.5, 1.0), metre), ('p5000', 5000, (0.2, 0.1, 0), (3.0, 2.5, 1.5), metre),
             ('flat', 300, (0, 0, 0.75), (1.5, 1.2, 0.0), metre),
             # voxel units with negative coordinates: larger HAIS grids; elastic granularities to match
             ('neg', 300, (-25, -20, -5), (60, 30, 10), (((4.0, 8.0), (16.0, 32.0)), ((6.0, 40.0), (20.0, 160.0))))]
    out['case_names'] = np.array([c[0] for c in cases])
    for ci, (name, P, lo, ext, (el, ha)) in enumerate(cases):
        pos = np.asarray(lo, np.float64) + rng.random((P, 3)) * np.asarray(ext, np.float64)
        dst = out if P <= 1000 else steps_out                                          # (file size: see the docstring)
        out[name + '_pos'] = pos
        out[name + '_el_params'] = np.asarray(el, np.float64)
        out[name + '_ha_params'] = np.asarray(ha, np.float64)
        cur = pos.copy()
        for k, (gran, mag) in enumerate(el):                                           # scannet.py:189-192
            del calls[:], axes[:]
            np.random.seed(1000 + 10 * ci + k)
            cur = AUG.elastic_distortion(cur, gran, mag)
            assert len(calls) == 6 and len(axes) == 1
            out['%s_el%d_noise' % (name, k)] = calls[0][0]
            out['%s_el%d_blur' % (name, k)] = calls[5][1]
            for a in range(3):
                out['%s_el%d_ax%d' % (name, k, a)] = axes[0][a]
            (out if k == 1 else dst)['%s_el%d_out' % (name, k)] = cur.copy()
        cur = pos.copy()
        for k, (gran, mag) in enumerate(ha):                                           # scannet.py:195-198
            del calls[:], axes[:]
            np.random.seed(2000 + 10 * ci + k)
            cur = AUG.HAIS_elastic(cur, gran, mag)
            assert len(calls) == 18 and len(axes) == 3
            out['%s_ha%d_noise' % (name, k)] = np.stack([calls[c][0] for c in range(3)])
            out['%s_ha%d_blur' % (name, k)] = np.stack([calls[15 + c][1] for c in range(3)])
            for a in range(3):
                out['%s_ha%d_ax%d' % (name, k, a)] = axes[0][a]
            dst['%s_ha%d_out' % (name, k)] = cur.copy()
        cur -= cur.min(0)
        out[name + '_ha_final'] = cur.copy()
    scipy.ndimage.filters.convolve = real_convolve
    scipy.interpolate.RegularGridInterpolator = real_rgi
    # ---- trilinear alone: points outside every axis in turn, on the first and on the last node, on interior nodes
    dims = (4, 3, 5)
    grid = rng.standard_normal(dims + (3,)).astype(np.float32)
    lo, hi = np.array([-0.4, 0.1, 1.0]), np.array([0.8, 0.5, 3.0])
    ax = [np.linspace(a, b, d) for a, b, d in zip(lo, hi, dims)]
    pts = lo + rng.random((40, 3)) * (hi - lo)
    pts[0] = hi; pts[1] = lo; pts[2] = [ax[0][1], ax[1][1], ax[2][3]]
    pts[3] = [hi[0], 0.3, 2.0]; pts[4] = [0.0, hi[1], 2.0]; pts[5] = [0.0, 0.3, hi[2]]
    pts[6] = [hi[0] + 1e-9, 0.3, 2.0]; pts[7] = [0.0, lo[1] - 1e-9, 2.0]; pts[8] = [0.0, 0.3, hi[2] + 0.5]
    pts[9] = [-5.0, -5.0, -5.0]; pts[10] = [np.nextafter(hi[0], 9.0), 0.3, 2.0]; pts[11] = [np.nextafter(lo[0], -9.0), 0.3, 2.0]
    interp = real_rgi(ax, grid, bounds_error=0, fill_value=0)
    out['tri_grid'] = grid; out['tri_lo'] = lo; out['tri_hi'] = hi; out['tri_pts'] = pts; out['tri_mag'] = np.float64(1.6)
    out['tri_out'] = pts + interp(pts) * 1.6
    # ---- colour: the three transforms chained in read_scene's order; `const` has a constant channel (scale = inf, NaN)
    for name, P, seed in (('col', 500, 31), ('colconst', 64, 32)):
        col = rng.random((P, 3))
        col[::7] = np.round(col[::7])                                               # exact 0 / 1 values among them
        if name == 'colconst':
            col[:, 1] = 0.25
        out[name + '_in'] = col.copy()
        random.seed(seed)
        with np.errstate(all='ignore'):
            c1 = AUG.ChromaticAutoContrast()(col.copy())
        random.seed(seed); random.random()
        out[name + '_blend'] = np.float64(random.random())
        out[name + '_contrast'] = c1.copy()
        random.seed(seed); np.random.seed(seed)
        assert random.random() < 0.95
        c2 = AUG.ChromaticTranslation(0.1)(c1.copy())
        np.random.seed(seed)
        out[name + '_tr'] = (np.random.rand(1, 3) - 0.5) * 1.0 * 2 * 0.1
        out[name + '_translation'] = c2.copy()
        np.random.seed(seed + 100)
        c3 = AUG.color_jittering(c2.copy(), -0.1, 0.1)
        np.random.seed(seed + 100)
        out[name + '_jitter'] = np.random.uniform(-0.1, 0.1, c2.shape)
        out[name + '_jittered'] = c3
    # ---- instance boxes: nine instances, one of a single point
    P, I = 1200, 9
    inst = rng.integers(0, I - 1, P).astype(np.int32)
    inst[777] = I - 1
    sem_of = np.array([3, 5, 5, 1, 2, 7, 39, 24, 4], np.int32)
    centre = rng.uniform(-2, 4, (I, 3))
    pos = centre[inst] + rng.normal(0, 0.3, (P, 3)) * rng.uniform(0.3, 1.5, (I, 3))[inst]
    sem = sem_of[inst]
    names = ('bb_centers', 'bb_offsets', 'bb_bounds', 'bb_center_distances', 'bb_radius', 'unique_instances', 'per_instance_semantics',
             'per_instance_bb_centers', 'per_instance_bb_bounds', 'per_instance_bb_radius')
    out['box_pos'] = pos; out['box_instances'] = inst; out['box_semantics'] = sem
    for n, v in zip(names, SC.compute_bounding_box(pos, inst, sem)):
        out['box_' + n] = v
    path = os.path.join(OUT, 'augment.npz')
    _savez_fixed(path, out)
    assert os.path.getsize(path) <= 1000000, os.path.getsize(path)
    print('augment.npz: %d bytes, %d arrays' % (os.path.getsize(path), len(out)))
    path2 = os.path.join(OUT, 'augment_steps.npz')
    _savez_fixed(path2, steps_out)
    assert os.path.getsize(path2) <= 1000000 and os.path.getsize(path) + os.path.getsize(path2) <= 3529354       # <= prepare.npz
    print('augment_steps.npz: %d bytes, %s' % (os.path.getsize(path2), sorted(steps_out)))


if __name__ == '__main__':
    os.makedirs(OUT, exist_ok=True)
    torch.manual_seed(0)
    which = sys.argv[1:] or ['iou_nms', 'detection2mask', 'detection2mask_nopool', 'losses', 'prepare', 'prepare2', 'eval', 'detection', 's3dis', 'augment',
                             's3dis_labels', 's3dis_full', 'sweep']
    if 'sweep' in which:
        gen_sweep()
    if 'iou_nms' in which:
        gen_iou_nms()
    if 'detection2mask' in which:
        gen_detection2mask()
    if 'detection2mask_nopool' in which:
        gen_detection2mask_nopool()
    if 'losses' in which:
        gen_losses()
    if 'prepare' in which:
        gen_prepare()
    if 'prepare2' in which:
        gen_prepare2()
    if 'eval' in which:
        gen_eval()
    if 'detection' in which:
        gen_detection()
    if 's3dis' in which:
        gen_s3dis()
    if 'augment' in which:
        gen_augment()
    if 's3dis_labels' in which:
        gen_s3dis_labels()
    if 's3dis_full' in which:
        gen_s3dis_full()
