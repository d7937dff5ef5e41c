"""tests/golden/arkit_sweep.npz: the 36 settings of the param_sweep fixture scored as Evaluater.arkitscenes_eval scores them.

    python tools/gen_golden_arkit_sweep.py

Inputs: those of param_sweep.npz (tools/gen_golden.py: ``_scene_inputs(11)``, ``SWEEP_GRID``) -- the fixture does not repeat them --
plus, per scene, the positions of ``synth.make_scene(seed, target_voxels=12000, pts_per_m2=6000.0, points_only=True)`` (the points
``vox2point`` indexes, with 2 mm of seeded noise -- tests/_det_sweep_rule.py, scene_positions; only a checksum is stored) and its furniture boxes as ARKitScenes labels, about every second one turned a
few degrees about z.

Every setting runs through the real SelectionNet.detection2mask (/root/reference/models/detection_net.py, the stubs of
gen_golden.py) and is scored with scipy.spatial.ConvexHull (evaluation.py:280-292), the reference's get_oriented_corners /
get_rotated_bounds (utils/box_util.py), get_iou_obb / get_iou and its own eval_det (utils/evaluate_detections.py), for both
``oriented_boxes`` values and ``ovthresh`` 0.5 and 0.25.  eval_det's np.array(BB) cannot hold hulls of different vertex counts: as
in gen_golden.gen_detection it is handed handles of equal shape and an IoU function that looks the real boxes up.

Nothing from /root/reference is copied: the fixture holds arrays only.  The conditions that keep it honest are asserted below; the
file is not written unless all hold.
"""
from __future__ import annotations

import contextlib
import io
import itertools
import os
import sys
import types
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402
sys.path.insert(0, os.path.join(G.ROOT, 'tests'))
import _det_sweep_rule as RULE  # noqa: E402
from box2mask_amd import synth  # noqa: E402

SEED = 11
MIN_POINTS = 50
THRESHOLDS = (0.5, 0.25)
YAW_SEED, YAW_DEGREES = 7000, (3.0, 9.0)
GATE_SETTING = (1, 1, 0, 0)


def scene_points_and_boxes(seed):
    """(positions (n, 3) float64, labels): the furniture boxes of the synthetic room as ARKitScenes labels.  Every second box is
    turned by 3 .. 9 degrees about z (the labels store the TRANSPOSE of the rotation, evaluation.py:261)."""
    raw = synth.make_scene(seed, target_voxels=12000, pts_per_m2=6000.0, points_only=True)
    lab = raw['labels']
    sem = np.asarray(lab['per_instance_semantics'])
    sel = np.arange(len(sem))                                              # furniture, then the floor (2) and the walls (1)
    rng = np.random.default_rng(YAW_SEED + seed)
    rot = np.zeros((len(sel), 9))
    for j in range(len(sel)):
        a = np.deg2rad(rng.uniform(*YAW_DEGREES) * rng.choice([-1.0, 1.0])) if j % 2 else 0.0
        c, s = np.cos(a), np.sin(a)
        R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        rot[j] = R.T.reshape(-1)
    labels = {'per_instance_bb_centers': np.asarray(lab['per_instance_bb_centers'])[sel].astype(np.float32),
              'per_instance_bb_bounds': np.asarray(lab['per_instance_bb_bounds'])[sel].astype(np.float32),
              'per_instance_bb_rotations': rot, 'per_instance_semantics': sem[sel].astype(np.int64)}
    positions = RULE.scene_positions(seed)                                 # (with 2 mm of seeded noise: see there)
    return positions, labels


def main():
    G._install_stubs()
    pv = types.ModuleType('pyviz3d'); pv.visualizer = types.ModuleType('pyviz3d.visualizer')
    sys.modules['pyviz3d'] = pv; sys.modules['pyviz3d.visualizer'] = pv.visualizer
    for a, t in (('float', float), ('bool', bool), ('int', int)):
        if not hasattr(np, a):
            setattr(np, a, t)
    if G.REF not in sys.path:
        sys.path.insert(0, G.REF)
    from scipy.spatial import ConvexHull
    import models.detection_net as dn
    import utils.box_util as B
    import utils.evaluate_detections as E
    valid, _, _, is_fg = synth.scannet_tables()
    cfg = SimpleNamespace(mlp_per_vox_semantics='mlp_per_vox_semantics', mlp_semantics='mlp_semantics',
                          network_heads=['mlp_offsets', 'mlp_bounds', 'mlp_bb_scores', 'mlp_semantics'], do_segment_pooling=True)
    ns = SimpleNamespace(requires_voxel_outputs=False, semantic_valid_class_ids=valid, is_foreground=is_fg)
    batch, pred = G._scene_inputs(SEED)
    names = [s['name'] for s in batch['scene']]
    S = len(names)
    out = {'ak_names': np.asarray(names), 'ak_min_points': np.array(MIN_POINTS), 'ak_thresholds': np.array(THRESHOLDS)}
    pos, labels, gcorners, gaabb = [], [], [], []
    for si in range(S):
        p, lab = scene_points_and_boxes(SEED + si)
        assert len(p) == len(batch['vox2point'][si]), 'the positions are not the points vox2point indexes'
        pos.append(p); labels.append(lab)
        out['ak_s%d_n_pts' % si] = np.array(len(p))
        out['ak_s%d_pos_sha256' % si] = RULE.positions_checksum(p)
        for k, v in lab.items():
            out['ak_s%d_%s' % (si, k)] = v
        gc, ga = [], []
        for i in range(len(lab['per_instance_semantics'])):                # evaluation.py:257-270
            bounds = lab['per_instance_bb_bounds'][i].astype(np.float64)
            R = np.reshape(lab['per_instance_bb_rotations'][i], [3, 3]).T
            c = lab['per_instance_bb_centers'][i].astype(np.float64)
            gc.append(B.get_oriented_corners(bounds, R, c))
            ga.append(np.concatenate([c, B.get_rotated_bounds(bounds, R) * 2.0], 0))
        gcorners.append(gc); gaabb.append(ga)
    assert any((lab['per_instance_bb_rotations'][:, 1] != 0).any() for lab in labels), 'every rotation is the identity'

    cache = {}

    def row_boxes(si, p_si, mask_row, label):
        """(count, prism, aabb, iou_obb (g,), iou_aabb (g,)) of one predicted mask: evaluation.py:279-299 and the pair IoUs."""
        key = (si, len(p_si), int(label), mask_row.tobytes())
        if key in cache:
            return cache[key]
        positions = p_si[mask_row]
        g = len(gcorners[si])
        if positions.shape[0] < MIN_POINTS:
            cache[key] = (positions.shape[0], None, None, None, None)
            return cache[key]
        p2 = positions[:, 0:2]
        hv = p2[ConvexHull(p2).vertices]
        zmin, zmax = np.min(positions[:, 2]), np.max(positions[:, 2])
        prism = np.concatenate([np.concatenate([hv, np.ones([hv.shape[0], 1]) * zmin], 1),
                                np.concatenate([hv, np.ones([hv.shape[0], 1]) * zmax], 1)], 0)
        pmin, pmax = np.min(positions, 0), np.max(positions, 0)
        aabb = np.concatenate([(pmin + pmax) / 2.0, pmax - pmin], 0)
        ro, ra = np.zeros(g), np.zeros(g)
        for i in range(g):
            if labels[si]['per_instance_semantics'][i] != label:
                continue
            ro[i] = E.get_iou_obb(prism, gcorners[si][i])
            ra[i] = E.get_iou(aabb, gaabb[si][i])
        cache[key] = (positions.shape[0], prism, aabb, ro, ra)
        return cache[key]

    maps, per_variant, stats = set(), {}, {'small': 0, 'gt_only': False, 'pred_only': False}

    def run(tag, ths, batch_, pos_):
        """One setting through the reference's detection2mask and arkitscenes_eval; returns per scene (masks, labels, counts)."""
        res = dn.SelectionNet.detection2mask(ns, batch_, {k: v.clone() for k, v in pred.items()}, cfg, 'eval', True, *ths)
        real = {}
        pred_all = {True: {}, False: {}}
        gt_all = {True: {}, False: {}}
        confs, back = {}, []
        for si, name in enumerate(names):
            r = res[name]
            mask, label_id, conf = r['mask'].numpy(), np.asarray(r['label_id']), r['conf'].numpy()
            for o in (True, False):
                pred_all[o][name] = []
                gt_all[o][name] = [[labels[si]['per_instance_semantics'][i], np.array([si, i])] for i in range(len(gcorners[si]))]
            for i in range(len(gcorners[si])):
                real[(True, si, 'g', i)] = gcorners[si][i]; real[(False, si, 'g', i)] = gaabb[si][i]
            counts, io_rows, ia_rows = [], [], []
            for i in range(len(label_id)):
                n, prism, aabb, ro, ra = row_boxes(si, pos_[si], mask[i], label_id[i])
                counts.append(n)
                if n < MIN_POINTS:
                    stats['small'] += 1
                    continue
                io_rows.append(ro); ia_rows.append(ra)
                for o, box in ((True, prism), (False, aabb)):
                    real[(o, si, 'p', i)] = box
                    pred_all[o][name].append([label_id[i], np.array([si, i]), conf[i]])
                confs.setdefault(int(label_id[i]), []).append(float(conf[i]))
            g = len(gcorners[si])
            pre = 'ak_%s_s%d_' % (tag, si)
            out[pre + 'count'] = np.array(counts, np.int64)
            out[pre + 'iou_obb'] = np.array(io_rows, np.float64).reshape(len(io_rows), g)
            out[pre + 'iou_aabb'] = np.array(ia_rows, np.float64).reshape(len(ia_rows), g)
            back.append((mask, label_id, np.array(counts, np.int64), out[pre + 'iou_obb'], conf))
            for t in THRESHOLDS:
                for tab in (out[pre + 'iou_obb'], out[pre + 'iou_aabb']):
                    assert tab.size == 0 or np.abs(tab - t).min() > 1e-6, 'an IoU within 1e-6 of a threshold'
        for c, v in confs.items():                                         # np.argsort(-confidence) is unstable
            assert len(set(v)) == len(v), 'two predictions of class %d with equal confidence in setting %s' % (c, tag)

        def iou_of(o, fn):
            def f(a, b):
                return fn(real[(o, int(a[0]), 'p', int(a[1]))], real[(o, int(b[0]), 'g', int(b[1]))])
            return f

        for o, vt, fn in ((True, 'obb', E.get_iou_obb), (False, 'aabb', E.get_iou)):
            for t in THRESHOLDS:
                with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
                    _, _, ap = E.eval_det(pred_all[o], gt_all[o], ovthresh=t, get_iou_func=iou_of(o, fn))
                key = 'ak_%s_%s_%d_' % (tag, vt, round(t * 100))
                out[key + 'classes'] = np.array([int(c) for c in ap.keys()], np.int64)
                out[key + 'ap'] = np.array([ap[c] for c in ap.keys()], np.float64)
                vals = [v for v in ap.values() if not np.isnan(v)]
                with np.errstate(all='ignore'):
                    out[key + 'map'] = np.array(np.mean(np.array(vals)))                       # evaluation.py:314
                maps.add(float(out[key + 'map']))
                per_variant.setdefault((vt, t), set()).add(float(out[key + 'map']))
                if o and t == 0.5:
                    pcls = {int(p[0]) for v in pred_all[o].values() for p in v}
                    gcls = {int(g_[0]) for v in gt_all[o].values() for g_ in v}
                    stats['gt_only'] |= bool(gcls - pcls)
                    stats['pred_only'] |= bool(pcls - gcls)
        return back

    shape = tuple(len(a) for a in G.SWEEP_GRID)
    scored = np.zeros(shape + (S,), np.int64)
    for q, st in enumerate(itertools.product(*(range(n) for n in shape))):
        back = run('q%02d' % q, [G.SWEEP_GRID[a][i] for a, i in enumerate(st)], batch, pos)
        scored[st] = [int((b[2] >= MIN_POINTS).sum()) for b in back]
        if st == GATE_SETTING:
            strict = back
        if st == GATE_SETTING[:3] + (len(G.SWEEP_GRID[3]) - 1,):
            lax = back
    # One case more, off the grid: scene 0 of GATE_SETTING once more with some of its POINTS left out -- vox2point and positions
    # without them; voxels, votes and therefore the mask NMS are untouched.
    #  (1) No kept row of these inputs has exactly MIN_POINTS points, so the grid cannot tell `< 50` from `<= 50`
    #      (evaluation.py:280): one matched row is thinned to exactly MIN_POINTS points.
    #  (2) No row under MIN_POINTS points suppresses a larger one in the mask NMS, so the grid cannot tell the gate after the NMS
    #      from a gate before it: a kept row A that suppresses a row B (B is kept with the largest mask_nms_th and not here) is
    #      thinned below MIN_POINTS points, B keeps at least MIN_POINTS.
    mask, label_id, counts, iou, conf = strict[0]
    lmask, _, lcounts, _, lconf = lax[0]
    order_case = None
    for b in np.nonzero(~np.isin(lconf, conf) & (lcounts >= MIN_POINTS))[0]:
        above = np.nonzero(conf > lconf[b])[0]
        if not len(above):
            continue
        a = above[np.argmax((mask[above] & lmask[b]).sum(1))]
        both, only_b = mask[a] & lmask[b], lmask[b] & ~mask[a]
        if both.sum() >= 30 and only_b.sum() >= MIN_POINTS - 30 + 5 and (order_case is None or only_b.sum() > order_case[2].sum()):
            order_case = (a, b, only_b, both)
    assert order_case is not None, 'no suppressed row to build case (2) from'
    a, b, only_b, both = order_case
    drop_a = np.concatenate([np.nonzero(mask[a] & ~lmask[b])[0], np.nonzero(both)[0][30:]])
    big = np.nonzero(counts >= MIN_POINTS)[0]
    apart = [r for j, r in enumerate(big) if iou[j].max() > 0.5 and counts[r] > MIN_POINTS and not (mask[r] & (mask[a] | lmask[b])).any()]
    row = min(apart, key=lambda r: counts[r])
    drop = np.union1d(np.nonzero(mask[row])[0][:counts[row] - MIN_POINTS], drop_a)
    sel = np.setdiff1d(np.arange(len(pos[0])), drop)
    batch_g = dict(batch)
    batch_g['vox2point'] = [np.asarray(batch['vox2point'][0])[sel]] + list(batch['vox2point'][1:])
    back = run('gate', [G.SWEEP_GRID[i][j] for i, j in enumerate(GATE_SETTING)], batch_g, [pos[0][sel]] + pos[1:])
    gcounts, gconf = back[0][2], back[0][4]
    assert (gcounts == MIN_POINTS).sum() == 1 and gcounts[gconf == conf[row]].tolist() == [MIN_POINTS], 'case (1) is not there'
    assert (back[0][3][int((gcounts[:np.nonzero(gconf == conf[row])[0][0]] >= MIN_POINTS).sum())] > 0.5).any(), 'case (1) matches nothing'
    assert gcounts[gconf == conf[a]].tolist() == [30] and not (gconf == lconf[b]).any() and lmask[b][sel].sum() >= MIN_POINTS, \
        'case (2) is not there'
    out['ak_gate_setting'] = np.array(GATE_SETTING, np.int64)
    out['ak_gate_dropped_points'] = drop.astype(np.int64)
    n_small, gt_only, pred_only = stats['small'], stats['gt_only'], stats['pred_only']
    for axis in range(4):
        assert (np.diff(scored, axis=axis) != 0).any(), 'axis %d never changes a scored-row count' % axis
    assert len(maps) >= 8, 'only %d distinct mAP values' % len(maps)
    assert n_small > 0, 'no kept row under %d points' % MIN_POINTS
    assert gt_only, 'no class with ground truth and no prediction'
    assert pred_only, 'no class with predictions and no ground truth'
    path = os.path.join(G.OUT, 'arkit_sweep.npz')
    G._savez_fixed(path, out)
    size = os.path.getsize(path)
    if size > 1000000:
        os.unlink(path)
        raise AssertionError('arkit_sweep.npz: %d bytes' % size)
    print('arkit_sweep.npz: %d bytes, %d settings, %d distinct mAP values (%s per variant) %.4f .. %.4f, scored rows %s .. %s, '
          '%d kept rows under %d points'
          % (size, scored[..., 0].size, len(maps), sorted(len(v) for v in per_variant.values()), min(maps), max(maps),
             scored.reshape(-1, S).min(0).tolist(),
             scored.reshape(-1, S).max(0).tolist(), n_small, MIN_POINTS))


if __name__ == '__main__':
    main()
