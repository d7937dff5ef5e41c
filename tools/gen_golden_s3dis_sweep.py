"""tests/golden/s3dis_sweep.npz: 36 threshold settings of two synthetic S3DIS rooms through the reference's own S3DIS evaluation.

    python tools/gen_golden_s3dis_sweep.py

Every setting (3 cluster_th x 4 score_th x 3 mask_bin_th; mask_nms_th has no effect in this flow, detection_net.py:449-451) runs
through the real SelectionNet.detection2mask in the S3DIS flow (per-voxel semantics head, one room per batch), the body of
Evaluater.s3dis_eval (models/evaluation.py:124-231, driven as tools/gen_golden.py gen_s3dis drives it: a stand-in model hands it
the fixture's head outputs and calls the real detection2mask) and utils/s3dis_util.s3dis_eval.  The true / false positives per class
are the reference's own lists ``tpsins`` / ``fpsins``, read from its frame when it returns.  Room 0 is evaluated once more with
cfg.full_resolution (the unsampled room has three times the points; get_sparse2dense is the ball-tree lookup of gen_s3dis_full).

The rooms are built by hand on a grid of 1/128 m -- groups of voxels (cells of 6 grid steps) with a ground-truth instance, a
predicted class per voxel, a segment and a box vote per segment -- so that the settings reach every edge the sweep's rule has; the
conditions are asserted below with the reference alone, and the file is not written unless all hold.  Nothing from the reference is
copied: the fixture holds arrays only."""
from __future__ import annotations

import contextlib
import io
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402

CELL = 6                                             # grid steps per voxel
THS = ([0.3, 0.5, 0.7], [0.1, 0.5, 0.8, 0.97], [0.3, 0.45, 0.65], [0.6])
FULL_LABEL_SETTINGS = ((1, 0, 0), (1, 2, 0))


class Room:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.pts, self.normal, self.gt_sem, self.gt_ins, self.pred, self.seg = [], [], [], [], [], []
        self.votes = {}                              # segment -> (centre (3) m, half size (3) m, score)
        self.used = set()

    def group(self, lo, hi, nv, ppv, gt_cls, gt_ins, pred, seg, normal=None):
        """nv voxels of the cell box [lo, hi) with ppv points each: one ground-truth instance, one predicted class, one segment."""
        rng = self.rng
        cells = np.stack(np.meshgrid(*[np.arange(lo[j], hi[j]) for j in range(3)], indexing='ij'), -1).reshape(-1, 3)
        assert len(cells) >= nv, (len(cells), nv)
        cells = cells[rng.choice(len(cells), nv, replace=False)]
        for c in cells:
            assert tuple(c) not in self.used, 'two groups share a voxel'
            self.used.add(tuple(c))
            inside = rng.choice(CELL ** 3, ppv, replace=False)
            p = np.stack([inside // (CELL * CELL), inside // CELL % CELL, inside % CELL], 1) + c * CELL
            self.pts.append(p)
        m = nv * ppv
        self.normal.append(np.full(m, normal) if normal is not None else rng.integers(0, 6, m))
        for lst, v in ((self.gt_sem, gt_cls), (self.gt_ins, gt_ins), (self.pred, pred), (self.seg, seg)):
            lst.append(np.full(m, v))

    def vote(self, seg, centre, half, score):
        self.votes[seg] = (np.asarray(centre, np.float64), np.asarray(half, np.float64), float(score))

    def box_object(self, origin, gt_cls, gt_ins, seg0, score, sigma, pred_minor=None, n_minor=0, nv=150, quads=4, vote_shift=None):
        """A piece of furniture of `quads` segments (6 x 6 x 8 cells each); pred_minor: n_minor voxels of every segment are predicted
        that class.  vote_shift: the last two segments vote for the box moved by that much along x."""
        ox, oy, oz = origin
        lo = np.array([ox, oy, oz]) * CELL * G.S3DIS_GRID
        centre = lo + np.array([12, 12, 8]) * CELL * G.S3DIS_GRID / 2.0
        half = np.array([12, 12, 8]) * CELL * G.S3DIS_GRID / 2.0
        for q in range(quads):
            qx, qy = ox + 6 * (q % 2), oy + 6 * (q // 2)
            seg = seg0 + q
            if n_minor:
                self.group((qx, qy, oz), (qx + 3, qy + 6, oz + 8), n_minor, 1, gt_cls, gt_ins, pred_minor, seg)
                self.group((qx + 3, qy, oz), (qx + 6, qy + 6, oz + 8), nv - n_minor, 1, gt_cls, gt_ins, gt_cls, seg)
            else:
                self.group((qx, qy, oz), (qx + 6, qy + 6, oz + 8), nv, 1, gt_cls, gt_ins, gt_cls, seg)
            c = centre + self.rng.normal(0, sigma, 3)
            if vote_shift is not None and q >= 2:
                c = centre + np.array([vote_shift, 0.0, 0.0])
            self.vote(seg, c, np.maximum(half + self.rng.normal(0, sigma, 3), 0.05), score - 0.004 * q)

    def finish(self, name):
        rng = self.rng
        grid = np.concatenate(self.pts)
        assert len(np.unique(grid, axis=0)) == len(grid)
        cat = lambda v: np.concatenate(v)
        normal, gt_sem, gt_ins, pred, seg = (cat(v) for v in (self.normal, self.gt_sem, self.gt_ins, self.pred, self.seg))
        order = np.argsort(gt_ins, kind='stable')                          # long runs of equal labels: the fixture stays small
        grid, normal, gt_sem, gt_ins, pred, seg = (v[order] for v in (grid, normal, gt_sem, gt_ins, pred, seg))
        cells, first, v2p = np.unique(grid // CELL, axis=0, return_index=True, return_inverse=True)
        v2p = v2p.reshape(-1)
        for col in (pred, seg):
            assert np.array_equal(col[first][v2p], col), 'a voxel with two predicted classes or two segments'
        useg, vox_seg = np.unique(seg[first], return_inverse=True)
        vox_seg = vox_seg.reshape(-1)
        n_seg = len(useg)
        world = (cells * CELL + CELL / 2.0) * G.S3DIS_GRID
        cnt = np.bincount(vox_seg, minlength=n_seg).astype(np.float64)
        loc = np.stack([np.bincount(vox_seg, weights=world[:, d], minlength=n_seg) / cnt for d in range(3)], 1).astype(np.float32)
        off, bnd, logit = np.zeros((n_seg, 3), np.float32), np.zeros((n_seg, 3), np.float32), np.zeros((n_seg, 1), np.float32)
        for i, s in enumerate(useg):
            if s in self.votes:
                c, h, p = self.votes[s]
            else:                                                          # background segments: any small box
                c, h, p = loc[i] + rng.normal(0, 0.05, 3), rng.uniform(0.05, 0.3, 3), rng.uniform(0.2, 0.9)
            off[i] = (c - loc[i]).astype(np.float32); bnd[i] = h; logit[i, 0] = np.log(p / (1.0 - p))
        return dict(name=name, grid=grid.astype(np.int16), normal=normal.astype(np.int8), gt_sem=gt_sem.astype(np.int64),
                    gt_ins=gt_ins.astype(np.int64), vox_pred=pred[first].astype(np.int64), vox2point=v2p.astype(np.int64),
                    vox_segments=vox_seg.astype(np.int64), seg_location=loc, seg_offsets=off, seg_bounds=bnd, seg_logits=logit)


def planes(rm, ceiling, floor, split_ceiling):
    """Ceiling (z cell 49), floor (z cell 0), a wall of 3300 points (y cell 0) and one of 200 (x cell 0).  split_ceiling: half of
    the ceiling's points are predicted `wall` -- the predicted ceiling is then exactly half the true one: IoU 0.5 to the point."""
    if split_ceiling:
        rm.group((1, 1, 49), (50, 80, 50), ceiling // 2, 1, 0, 0, 0, 0, normal=5)
        rm.group((50, 1, 49), (100, 80, 50), ceiling - ceiling // 2, 1, 0, 0, 2, 1, normal=5)
    else:
        rm.group((1, 1, 49), (100, 80, 50), ceiling, 1, 0, 0, 0, 0, normal=5)
    rm.group((1, 1, 0), (100, 80, 1), floor, 1, 1, 1, 1, 2, normal=4)
    for q in range(4):                                                     # four segments along x
        rm.group((1 + 25 * q, 0, 1), (min(26 + 25 * q, 100), 1, 49), 825, 1, 2, 2, 2, 3 + q, normal=2)
    rm.group((0, 1, 1), (1, 80, 49), 200, 1, 2, 3, 2, 7, normal=0)


def room0():
    rm = Room(7001)
    planes(rm, 400, 500, True)
    at = lambda i: (6 + 15 * (i % 6), 6 + 15 * (i // 6), 2)
    rm.box_object(at(0), 3, 10, 100, 0.95, 0.02)
    rm.box_object(at(1), 4, 11, 110, 0.90, 0.02)
    rm.box_object(at(2), 5, 12, 120, 0.70, 0.02, pred_minor=1, n_minor=40)                 # 160 points repainted inside the floor
    rm.box_object(at(3), 6, 13, 130, 0.60, 0.12)                                           # noisy votes: fragments
    # one segment whose voxels vote class 7 and whose POINTS vote floor: a proposal of class 1, skipped
    ox, oy, oz = at(4)
    rm.group((ox, oy, oz), (ox + 6, oy + 6, oz + 4), 30, 10, 7, 14, 1, 140)
    rm.group((ox + 6, oy, oz), (ox + 12, oy + 6, oz + 4), 50, 1, 7, 14, 7, 140)
    lo = np.array([ox, oy, oz]) * CELL * G.S3DIS_GRID
    rm.vote(140, lo + np.array([0.28, 0.14, 0.09]), [0.28, 0.14, 0.09], 0.75)
    rm.box_object(at(5), 8, 15, 150, 0.91, 0.01, nv=90, quads=2)                           # 180 points: under the 200-point rule
    rm.box_object(at(6), 9, 16, 160, 0.85, 0.0, vote_shift=0.140625)                       # two vote groups at IoU 0.6: duplicates
    # three segments in a chain (IoU 7/13 between neighbours, 4/16 between the ends): B = S3 + S2 is accepted after A = S1 + S2
    # repainted S2, and its vote differs when read from the repainted classes
    ox, oy, oz = at(7)
    u = 0.05
    base = np.array([ox, oy, oz]) * CELL * G.S3DIS_GRID
    rm.group((ox, oy, oz), (ox + 6, oy + 6, oz + 9), 300, 1, 10, 17, 10, 170)
    rm.group((ox + 6, oy, oz), (ox + 9, oy + 6, oz + 8), 101, 1, 10, 17, 10, 171)
    rm.group((ox + 9, oy, oz), (ox + 12, oy + 6, oz + 8), 99, 1, 10, 17, 12, 171)
    rm.group((ox, oy + 6, oz), (ox + 6, oy + 12, oz + 6), 180, 1, 11, 18, 11, 172)
    rm.group((ox + 6, oy + 6, oz), (ox + 12, oy + 12, oz + 6), 140, 1, 11, 18, 3, 172)
    for seg, x0, p in ((170, 0.0, 0.92), (171, 3.0, 0.55), (172, 6.0, 0.88)):
        rm.vote(seg, base + np.array([(x0 + 5.0) * u, 0.3, 0.2]), [5.0 * u, 0.3, 0.2], p)
    return rm.finish('room0')


def room1():
    rm = Room(7002)
    planes(rm, 300, 250, False)
    at = lambda i: (6 + 15 * (i % 6), 6 + 15 * (i // 6), 2)
    rm.box_object(at(0), 6, 10, 100, 0.93, 0.02)
    rm.box_object(at(1), 8, 11, 110, 0.86, 0.02)
    # 260 of its points are predicted floor and repainted: the floor instance then VOTES class 7 (260 against 250)
    rm.box_object(at(2), 7, 12, 120, 0.65, 0.02, pred_minor=1, n_minor=65)
    rm.box_object(at(3), 12, 13, 130, 0.75, 0.02)
    rm.box_object(at(4), 3, 14, 140, 0.30, 0.02)
    rm.box_object(at(5), 5, 15, 150, 0.62, 0.02)
    return rm.finish('room1')


def full_room(rm, seed, times=3):
    """The unsampled room: four in five of the sampled points, then copies of random sampled points moved by up to two grid steps per
    axis, shuffled together (three times the points in all; some sampled points are nobody's nearest); no full point has two nearest
    sampled points at the same distance (checked exactly on the integer grid)."""
    rng = np.random.default_rng(seed)
    grid = rm['grid'].astype(np.int64)
    n = len(grid)
    kept = np.nonzero(rng.random(n) < 0.8)[0]
    m = times * n - len(kept)
    src = rng.integers(0, n, m)
    extra = np.zeros((m, 3), np.int64)
    todo = np.arange(m)
    while len(todo):
        src[todo] = rng.integers(0, n, len(todo))
        extra[todo] = np.maximum(grid[src[todo]] + rng.integers(-2, 3, (len(todo), 3)), 0)
        tied = []
        for s in range(0, len(todo), 1024):
            rows = todo[s:s + 1024]
            d2 = ((extra[rows, None, :] - grid[None, :, :]) ** 2).sum(2)
            two = np.partition(d2, 1, axis=1)[:, :2]
            tied.append(rows[two[:, 0] == two[:, 1]])
        todo = np.concatenate(tied)
    full = np.concatenate([grid[kept], extra])
    origin = np.concatenate([kept, src])
    perm = rng.permutation(len(full))
    return full[perm].astype(np.int16), rm['gt_sem'][origin][perm], rm['gt_ins'][origin][perm]


def main():
    G._install_stubs()
    for a, t in (('float', float), ('bool', bool), ('int', int)):
        if not hasattr(np, a):
            setattr(np, a, t)
    if G.REF not in sys.path:
        sys.path.insert(0, G.REF)
    EV, SU, s3 = G._s3dis_eval_modules()
    import models.detection_net as dn
    from sklearn.neighbors import NearestNeighbors
    sys.path.insert(0, os.path.join(G.ROOT, 'tests'))
    import _s3dis_sweep_rule as RULE

    cfg3 = SimpleNamespace(mlp_per_vox_semantics='mlp_per_vox_semantics', mlp_semantics='mlp_semantics',
                           network_heads=['mlp_offsets', 'mlp_bounds', 'mlp_bb_scores', 'mlp_per_vox_semantics'], do_segment_pooling=True)
    ns3 = SimpleNamespace(requires_voxel_outputs=True, semantic_valid_class_ids=torch.Tensor(np.arange(13)), is_foreground=lambda s: s > 2)
    rooms = [room0(), room1()]
    full_grid, full_sem, full_ins = full_room(rooms[0], 7100)
    batches, preds = {}, {}
    for rm in rooms:
        rm['positions'] = rm['grid'].astype(np.float64) * G.S3DIS_GRID
        rm['normals'] = G.S3DIS_NORMALS[rm['normal']]
        batches[rm['name']], preds[rm['name']] = RULE.room_batch(rm)
    full_by_name = {'room0': ({'name': 'room0', 'positions': full_grid.astype(np.float64) * G.S3DIS_GRID},
                              {'semantics': full_sem, 'instances': full_ins})}
    seen = {}

    class StandIn:
        ths = None

        def get_prediction(self, batch, with_grad=False, to_cpu=True, min_size=True):
            return {k: v.clone() for k, v in preds[batch['scene'][0]['name']].items()}

        def pred2mask(self, batch, prediction, mode='eval'):
            res = dn.SelectionNet.detection2mask(ns3, batch, prediction, cfg3, mode, True, *self.ths)
            seen.setdefault('masks', []).append(res[batch['scene'][0]['name']])
            return res

    real_bg, real_assign, real_eval = SU.clustering_for_background, SU.assign_semantics_to_proposals, SU.s3dis_eval

    def bg(pred_semantics, coords, normals):
        r = real_bg(pred_semantics, coords, normals)
        seen.setdefault('background', []).append(r.copy())
        return r

    def assign(pred_semantics, masks):
        r = real_assign(pred_semantics, masks)
        seen.setdefault('proposal_semantics', []).append(np.array(r, np.int64).reshape(-1))
        return r

    def ev(pred_labels, gt_labels):
        seen['pred_labels'] = pred_labels
        lists = {}

        def prof(frame, event, arg):
            if event == 'return' and frame.f_code is real_eval.__code__:
                lists['tp'] = [list(v) for v in frame.f_locals['tpsins']]
                lists['fp'] = [list(v) for v in frame.f_locals['fpsins']]
                lists['total_gt'] = np.array(frame.f_locals['total_gt_ins'])

        sys.setprofile(prof)
        try:
            with np.errstate(all='ignore'):
                seen['result'] = real_eval(pred_labels, gt_labels)
        finally:
            sys.setprofile(None)
        seen['tp'] = np.array([int(np.sum(v)) for v in lists['tp']], np.int64)
        seen['fp'] = np.array([int(np.sum(v)) for v in lists['fp']], np.int64)
        seen['total_gt'] = lists['total_gt'].astype(np.int64)
        return seen['result']

    def get_sparse2dense(scene_full, scene, cfg):
        tree = NearestNeighbors(n_neighbors=1, algorithm='ball_tree').fit(scene['positions'])
        seen['s2d'] = tree.kneighbors(scene_full['positions'], return_distance=False)[:, 0]
        return seen['s2d']

    def run(ths, names, full):
        """One setting through Evaluater.s3dis_eval over the rooms `names`."""
        seen.clear()
        model = StandIn()
        model.ths = ths
        evaluater = object.__new__(EV.Evaluater)
        evaluater.model = model
        evaluater.cfg = SimpleNamespace(eval_ths=list(ths), s3dis_split_fold=5, full_resolution=full, point_sampling_rate=3)
        loader = SimpleNamespace(get_loader=lambda **kw: [batches[n] for n in names])
        SU.clustering_for_background, SU.assign_semantics_to_proposals, SU.s3dis_eval = bg, assign, ev
        missing = object()
        before = (getattr(EV, 'get_sparse2dense', missing), getattr(s3, 'process_scene', missing))
        if full:
            EV.get_sparse2dense = get_sparse2dense
            s3.process_scene = lambda name, mode, cfg: full_by_name[name]
        try:
            with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                evaluater.s3dis_eval(loader)
        finally:
            SU.clustering_for_background, SU.assign_semantics_to_proposals, SU.s3dis_eval = real_bg, real_assign, real_eval
            if full:                                                       # what was there before, or nothing
                for mod, name, old in ((EV, 'get_sparse2dense', before[0]), (s3, 'process_scene', before[1])):
                    if old is missing:
                        delattr(mod, name)
                    else:
                        setattr(mod, name, old)
        return dict(seen)

    out = {'n_rooms': np.array(len(rooms))}
    for key, v in zip(('cluster_th', 'score_th', 'mask_bin_th', 'mask_nms_th'), THS):
        out[key] = np.asarray(v, np.float64)
    nc, ns, nb = len(THS[0]), len(THS[1]), len(THS[2])
    ks = np.zeros((len(rooms), nc, ns, nb), np.int64)
    reach = dict(ceiling_drop=False, rej_ratio=False, rej_points=False, rej_class=False, patch=False, tp_moves=False, nan_prec=False,
                 vote_differs=False, iou_half=False)
    stage_masks, stage_conf, tps = {}, {}, {}
    q = 0
    for ci in range(nc):
        for si in range(ns):
            for bi in range(nb):
                ths = [THS[0][ci], THS[1][si], THS[2][bi], THS[3][0]]
                got = run(ths, [rm['name'] for rm in rooms], False)
                tag = 'q%02d_' % q
                mprec, mrec, prec, rec = got['result']
                out[tag + 'tp'], out[tag + 'fp'], out[tag + 'total_gt'] = got['tp'], got['fp'], got['total_gt']
                out[tag + 'precision'], out[tag + 'recall'] = np.asarray(prec, np.float64), np.asarray(rec, np.float64)
                out[tag + 'mprec'], out[tag + 'mrec'] = np.float64(mprec), np.float64(mrec)
                tps[(ci, si, bi)] = got['tp']
                reach['nan_prec'] |= bool(((got['tp'] + got['fp']) == 0).any())
                for r, rm in enumerate(rooms):
                    res, fin = got['masks'][r], got['pred_labels'][r]
                    mask = np.asarray(res['mask']).astype(bool).reshape(-1, len(rm['grid']))
                    conf = np.asarray(res['conf'], np.float32).reshape(-1)
                    ks[r, ci, si, bi] = len(mask)
                    ins, sem = np.asarray(fin['instances']).astype(np.int64), np.asarray(fin['semantics']).astype(np.int64)
                    out[tag + 'r%d_instances' % r] = ins.astype(np.int16); out[tag + 'r%d_semantics' % r] = sem.astype(np.int8)
                    assert np.array_equal(out[tag + 'r%d_instances' % r], ins)
                    rm.setdefault('background', got['background'][r])
                    assert np.array_equal(rm['background'], got['background'][r])       # no threshold reaches the wall clustering
                    if si == 0:
                        stage_masks[(r, ci, bi)], stage_conf[(r, ci, bi)] = mask, conf
                    else:                                                               # the score filter keeps a prefix
                        k = len(mask)
                        assert np.array_equal(mask, stage_masks[(r, ci, bi)][:k]) and np.array_equal(conf, stage_conf[(r, ci, bi)][:k])
                    # ---- what this setting reaches, from the reference's arrays alone
                    owner, prop_sem, fate = RULE.paint(mask, rm['vox_pred'][rm['vox2point']])
                    assert np.array_equal(prop_sem, got['proposal_semantics'][r]) if len(mask) else True
                    reach['ceiling_drop'] |= bool((owner < 0).all() and (rm['background'] == 1).any() and not (ins == 0).any()
                                                  and not (ins[rm['background'] == 1] > 0).any())
                    reach['rej_class'] |= bool((fate == RULE.REJ_CLASS).any())
                    reach['rej_ratio'] |= bool((fate == RULE.REJ_RATIO).any())
                    reach['rej_points'] |= bool((fate == RULE.REJ_POINTS).any())
                    pred_pts = rm['vox_pred'][rm['vox2point']]
                    for u in np.unique(ins[ins >= 0]):
                        m = ins == u
                        if RULE._vote(sem[m]) != RULE._vote(pred_pts[m]):
                            reach['vote_differs'] = True
                    if r == 0:
                        cm = ins == (ins[rm['background'] == 1].max() if (rm['background'] == 1).any() else -5)
                        gm = rm['gt_ins'] == 0
                        if cm.any() and 3 * int((cm & gm).sum()) == int(cm.sum()) + int(gm.sum()):
                            reach['iou_half'] = True
                q += 1
    # a repainted patch of fewer than 200 points inside a background instance, there in one score setting and gone in the next
    for r, rm in enumerate(rooms):
        pred_pts = rm['vox_pred'][rm['vox2point']]
        for ci in range(nc):
            for bi in range(nb):
                for si in range(ns - 1):
                    qa, qb = (ci * ns + si) * nb + bi, (ci * ns + si + 1) * nb + bi
                    sa, sb = out['q%02d_r%d_semantics' % (qa, r)], out['q%02d_r%d_semantics' % (qb, r)]
                    ia, ib = out['q%02d_r%d_instances' % (qa, r)], out['q%02d_r%d_instances' % (qb, r)]
                    patch = (rm['background'] > 0) & (sa != pred_pts) & (sb == pred_pts)
                    if 0 < patch.sum() < 200 and (ia[patch] == -1).all() and (ib[patch] >= 0).all():
                        reach['patch'] = True
                    if (tps[(ci, si, bi)] != tps[(ci, si + 1, bi)]).any():
                        reach['tp_moves'] = True
    missing = [k for k, v in reach.items() if not v]
    assert not missing, 'the settings do not reach: %s' % missing
    finite = [q_ for q_ in range(q) if np.isfinite(out['q%02d_mprec' % q_]) and np.isfinite(out['q%02d_mrec' % q_])]
    pairs = {(float(out['q%02d_mprec' % q_]), float(out['q%02d_mrec' % q_])) for q_ in finite}
    assert len(finite) >= 12 and len(pairs) >= 4 and len({p_[0] for p_ in pairs}) >= 3, 'mPrec / mRec are flat or NaN throughout'
    for axis in (1, 2):                                                    # (mask_bin_th changes the masks, not their number)
        assert (np.diff(ks, axis=axis) != 0).any(), 'axis %d never changes a proposal count' % (axis - 1)
    assert any((tps[(ci, si, 0)] != tps[(ci, si, nb - 1)]).any() for ci in range(nc) for si in range(ns)), 'mask_bin_th never moves a count'
    for r, rm in enumerate(rooms):
        p = 'r%d_' % r
        n_seg = len(rm['seg_location'])
        seg_of_point = rm['vox_segments'][rm['vox2point']]
        _, first = np.unique(seg_of_point, return_index=True)
        assert len(first) == n_seg
        for ci in range(nc):
            for bi in range(nb):
                mask = stage_masks[(r, ci, bi)]
                segmask = mask[:, first]
                assert np.array_equal(segmask[:, seg_of_point], mask)                  # masks are unions of segments
                out[p + 'c%d_b%d_segmask' % (ci, bi)] = np.packbits(segmask, axis=1)
                out[p + 'c%d_b%d_conf' % (ci, bi)] = stage_conf[(r, ci, bi)]
        out[p + 'k'] = ks[r]
        out[p + 'grid'], out[p + 'normal'] = rm['grid'], rm['normal']
        out[p + 'gt_semantics'], out[p + 'gt_instances'] = rm['gt_sem'].astype(np.int8), rm['gt_ins'].astype(np.int16)
        out[p + 'vox2point'], out[p + 'vox_segments'] = rm['vox2point'].astype(np.int32), rm['vox_segments'].astype(np.int32)
        out[p + 'vox_pred'] = rm['vox_pred'].astype(np.int8)
        for key in ('seg_location', 'seg_offsets', 'seg_bounds', 'seg_logits'):
            out[p + key] = rm[key]
        out[p + 'background'] = rm['background'].astype(np.int16)
    # ---- room 0 at full resolution
    out['full_grid'], out['full_gt_semantics'], out['full_gt_instances'] = full_grid, full_sem.astype(np.int8), full_ins.astype(np.int16)
    q = 0
    moved = False
    for ci in range(nc):
        for si in range(ns):
            for bi in range(nb):
                got = run([THS[0][ci], THS[1][si], THS[2][bi], THS[3][0]], ['room0'], True)
                tag = 'full_q%02d_' % q
                mprec, mrec, prec, rec = got['result']
                out[tag + 'tp'], out[tag + 'fp'], out[tag + 'total_gt'] = got['tp'], got['fp'], got['total_gt']
                out[tag + 'precision'], out[tag + 'recall'] = np.asarray(prec, np.float64), np.asarray(rec, np.float64)
                out[tag + 'mprec'], out[tag + 'mrec'] = np.float64(mprec), np.float64(mrec)
                s2d = got['s2d']
                if q == 0:
                    out['full_sparse2dense'] = s2d.astype(np.int32)
                    assert len(np.unique(s2d)) < len(rooms[0]['grid']) and len(s2d) == 3 * len(rooms[0]['grid'])
                assert np.array_equal(out['full_sparse2dense'], s2d)
                fin = got['pred_labels'][0]
                ins, sem = np.asarray(fin['instances']), np.asarray(fin['semantics'])
                assert np.array_equal(ins, out['q%02d_r0_instances' % q][s2d]) and np.array_equal(sem, out['q%02d_r0_semantics' % q][s2d])
                if (ci, si, bi) in FULL_LABEL_SETTINGS:
                    out[tag + 'instances'], out[tag + 'semantics'] = ins.astype(np.int16), sem.astype(np.int8)
                # the pairs under 200 points are dropped on the sampled room: a patch that tripled its points is still gone
                sem0 = rooms[0]['vox_pred'][rooms[0]['vox2point']]
                k = int(ks[0, ci, si, bi])
                late = RULE.labels(*RULE.paint(stage_masks[(0, ci, bi)][:k], sem0)[:2], rooms[0]['background'], sem0, k, s2d,
                                   mistake='small_at_eval')[0]
                moved |= bool((late != ins).any())
                q += 1
    assert moved, 'no pair whose removal depends on the resolution it is counted at'
    path = os.path.join(G.OUT, 's3dis_sweep.npz')
    G._savez_fixed(path, out)
    size = os.path.getsize(path)
    if size > 1000000:
        os.unlink(path)
        raise AssertionError('s3dis_sweep.npz: %d bytes' % size)
    print('s3dis_sweep.npz: %d bytes; points %s, segments %s; proposals per setting %s .. %s; mPrec %.4f .. %.4f over %d finite settings'
          % (size, [len(rm['grid']) for rm in rooms], [len(rm['seg_location']) for rm in rooms], ks.reshape(len(rooms), -1).min(1).tolist(),
             ks.reshape(len(rooms), -1).max(1).tolist(), min(float(out['q%02d_mprec' % q_]) for q_ in finite),
             max(float(out['q%02d_mprec' % q_]) for q_ in finite), len(finite)))


if __name__ == '__main__':
    main()
