"""ARKitScenes detection metric on the device (csrc/detbox.hip through box2mask_amd/eval_detection.py) against the fixture taken
from the reference's ConvexHull / box3d_iou / calc_iou / eval_det (tests/golden/eval_detection.npz), and at a size no fixture is
committed for against the numpy restatement of tests/_detbox_rule.py.

Measured on an MI355X (the tests print their figures): hull area relative error 2e-16 and vertex-to-boundary distance 0 against
bounds of 1e-12; IoU max abs error 1.67e-15 (oriented, 59 overlapping pairs) and 2.22e-16 (axis-aligned) against the bound of 1e-9."""
import os

import numpy as np
import pytest
import torch

from _detbox_rule import np_area, np_hull          # the numpy restatement (Andrew's monotone chain, shoelace)

pytestmark = pytest.mark.gpu
IOU_TOL = 1e-9          # set by the issue: an independent fp64 restatement differs from box3d_iou by at most 5.8e-14 over 1 500 pairs


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'eval_detection.npz'))


def _scene(z, s):
    n = int(z['s%d_n' % s])
    mask = np.unpackbits(z['s%d_mask' % s], axis=1)[:, :n].astype(bool)
    pred = {'conf': z['s%d_conf' % s], 'label_id': z['s%d_label_id' % s], 'mask': mask}
    labels = {k: z['s%d_%s' % (s, k)] for k in ('per_instance_bb_centers', 'per_instance_bb_bounds', 'per_instance_bb_rotations',
                                               'per_instance_semantics')}
    return pred, z['s%d_pos' % s].astype(np.float64), labels


def boundary_distance(pts, poly):
    """Largest distance of `pts` to the boundary of the closed polygon `poly`."""
    a, b = poly, np.roll(poly, -1, axis=0)
    d = b - a
    t = np.einsum('pej,ej->pe', pts[:, None, :] - a[None], d) / np.maximum((d * d).sum(1), 1e-300)
    near = a[None] + np.clip(t, 0.0, 1.0)[..., None] * d[None]
    return float(np.sqrt(((pts[:, None, :] - near) ** 2).sum(2)).min(1).max())


def test_hulls_match_qhull(gold):
    from box2mask_amd import eval_detection as D
    worst_area = worst_edge = 0.0
    for s in range(int(gold['n_scenes'])):
        pred, pos, _ = _scene(gold, s)
        out = D.mask_boxes(pred, pos)
        count = out['count'].cpu().numpy()
        assert np.array_equal(count, gold['s%d_count' % s])                        # point counts exact
        assert np.array_equal(out['keep'], count >= 50)
        nh, hull, box6 = out['n_hull'].cpu().numpy(), out['hull'].cpu().numpy(), out['box6'].cpu().numpy()
        off = gold['s%d_hull_off' % s]
        pts = {tuple(q) for q in pos[:, :2]}
        for r in np.nonzero(count >= 50)[0]:
            assert np.array_equal(box6[r], gold['s%d_box6' % s][r])                # min / max corners, zmin / zmax: exact
            ref = gold['s%d_hull' % s][off[r]:off[r + 1]]
            v = hull[r, :nh[r]]
            assert nh[r] >= 3
            assert all(tuple(q) in pts for q in v)                                 # input points, bit for bit
            assert tuple(v[0]) == min(tuple(q) for q in v)                         # starts at the lexicographically smallest
            e1, e2 = np.roll(v, -1, 0) - v, np.roll(v, -2, 0) - np.roll(v, -1, 0)
            assert (e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0] > 0).all()           # counter-clockwise, strictly convex
            a, ra = np_area(v), np_area(ref)
            worst_area = max(worst_area, abs(a - ra) / ra)
            worst_edge = max(worst_edge, boundary_distance(ref, v), boundary_distance(v, ref))
    print('hulls vs qhull: relative area error %.3g, vertex-to-boundary distance %.3g' % (worst_area, worst_edge))
    assert worst_area <= 1e-12 and worst_edge <= 1e-12


def test_iou_tables_match_box3d_iou_and_calc_iou(gold):
    from box2mask_amd import eval_detection as D
    worst = {'obb': 0.0, 'aabb': 0.0}
    pairs = 0
    for s in range(int(gold['n_scenes'])):
        pred, pos, labels = _scene(gold, s)
        boxes, gt = D.mask_boxes(pred, pos), D.gt_boxes(labels)
        keep = boxes['keep']
        for tag, oriented in (('obb', True), ('aabb', False)):
            iou = D.scene_ious(boxes, gt, oriented)
            ref = gold['s%d_iou_%s' % (s, tag)]
            assert iou.shape == ref.shape and (iou[~keep] == 0).all()
            assert np.array_equal(iou[keep] > 0, ref[keep] > 0)                    # the same pairs overlap
            worst[tag] = max(worst[tag], float(np.abs(iou[keep] - ref[keep]).max()))
        pairs += int((gold['s%d_iou_obb' % s][keep] > 0).sum())
    print('IoU tables, %d overlapping pairs: max abs error oriented %.3g, axis-aligned %.3g' % (pairs, worst['obb'], worst['aabb']))
    assert worst['obb'] <= IOU_TOL and worst['aabb'] <= IOU_TOL


@pytest.mark.parametrize('oriented', [True, False])
@pytest.mark.parametrize('th', [0.5, 0.25])
def test_arkitscenes_eval_end_to_end(gold, oriented, th):
    from box2mask_amd import eval_detection as D
    results, scenes, labels = {}, [], []
    for s in range(int(gold['n_scenes'])):
        pred, pos, lab = _scene(gold, s)
        # predictions as Model.pred2mask returns them: torch tensors, masks on the device
        results['room%d' % s] = {'conf': torch.from_numpy(pred['conf']), 'label_id': pred['label_id'],
                                 'mask': torch.from_numpy(pred['mask']).cuda()}
        scenes.append({'name': 'room%d' % s, 'positions': pos})
        labels.append(lab)
    m, ap = D.arkitscenes_eval(results, scenes, labels, oriented_boxes=oriented, iou_t=th, verbose=False)
    key = '%s_%d' % ('obb' if oriented else 'aabb', round(th * 100))
    classes = [int(c) for c in gold[key + '_classes']]
    assert list(ap.keys()) == classes
    got = np.array([ap[c] for c in classes], np.float64)
    assert np.array_equal(got.view(np.uint64), gold[key + '_ap'].view(np.uint64))           # bit for bit, the nan class included
    assert np.float64(m).tobytes() == np.float64(gold[key + '_map']).tobytes()


def _big_case():
    rng = np.random.default_rng(3)
    n, k = 1_000_000, 300
    pos = np.stack([rng.uniform(0, 40, n), rng.uniform(0, 30, n), rng.uniform(0, 3, n)], 1)
    centers = np.stack([rng.uniform(2, 38, k), rng.uniform(2, 28, k)], 1)
    masks = np.zeros((k, n), bool)
    order = np.argsort(pos[:, 0], kind='stable')
    xs = pos[order, 0]
    for r in range(k):
        rad = rng.uniform(0.3, 2.0)
        lo, hi = np.searchsorted(xs, [centers[r, 0] - rad, centers[r, 0] + rad])
        idx = order[lo:hi]
        d = pos[idx, :2] - centers[r]
        sel = (d * d).sum(1) < rad * rad if r % 2 else np.abs(d[:, 1]) < rad * 0.7      # discs and rectangles
        masks[r, idx[sel]] = True
    masks[7] = False                                                                     # an empty row
    masks[8] = False; masks[8, 12345] = True                                             # a single point
    return pos, masks


def test_one_million_points_300_masks():
    from box2mask_amd import eval_detection as D
    pos, masks = _big_case()
    out = D.mask_boxes({'conf': np.zeros(len(masks), np.float32), 'label_id': np.full(len(masks), 5, np.int32),
                        'mask': torch.from_numpy(masks)}, pos)
    count, nh = out['count'].cpu().numpy(), out['n_hull'].cpu().numpy()
    hull, box6 = out['hull'].cpu().numpy(), out['box6'].cpu().numpy()
    assert np.array_equal(count, masks.sum(1))
    assert nh[7] == 0 and nh[8] == 1 and np.array_equal(hull[8, 0], pos[12345, :2])
    worst = 0.0
    for r in range(len(masks)):
        if count[r] == 0:
            continue
        p = pos[masks[r]]
        assert np.array_equal(box6[r], np.concatenate([p.min(0), p.max(0)]))             # z range and corners: exact
        ref = np_hull(p[:, :2])
        if len(ref) >= 3:
            worst = max(worst, abs(np_area(hull[r, :nh[r]]) - np_area(ref)) / np_area(ref))
            assert np.array_equal(hull[r, :nh[r]], ref)                                  # the same chain over the same points
    print('1 M points, 300 masks (%d set points, largest hull %d, most candidates %d): relative area error %.3g'
          % (count.sum(), nh.max(), int(out['ncand'].max()), worst))
    assert worst <= 1e-12


def test_hull_beyond_capacity_raises_and_nothing_is_truncated():
    from box2mask_amd import _lib, eval_detection as D
    m = D.HULL_MAX + 88
    ang = 2 * np.pi * np.arange(m) / m
    pos = np.stack([np.cos(ang), np.sin(ang), np.zeros(m)], 1)
    small = np.zeros(m, bool); small[::10] = True                                        # 60 vertices: fits
    pred = {'conf': np.zeros(2, np.float32), 'label_id': np.array([5, 5], np.int32), 'mask': np.stack([np.ones(m, bool), small])}
    bits, words, n = D.pack_masks(pred['mask'])
    raw = D.hulls_from_bits(bits, words, n, pos)
    assert raw['flags'].cpu().tolist() == [D.FLAG_VERTICES, 0] and raw['n_hull'].cpu().tolist() == [m, 60]
    assert (raw['hull'][0] == 0).all()                                                   # not a vertex written for the flagged row
    with pytest.raises(_lib.B2MError, match='B2M_HULL_MAX'):
        D.mask_boxes(pred, pos)
    with pytest.raises(_lib.B2MError, match='B2M_HULL_MAX'):                             # the deferred check of scene_ious as well
        boxes = D.mask_boxes(pred, pos, check=False)
        D.scene_ious(boxes, D.gt_boxes({'per_instance_bb_centers': np.zeros((1, 3)), 'per_instance_bb_bounds': np.ones((1, 3)),
                                        'per_instance_semantics': np.array([5])}))


def test_full_candidate_buffer_is_reported_and_a_larger_one_gives_the_same_hull():
    from box2mask_amd import eval_detection as D
    g = np.arange(100) * 0.01
    pos = np.stack([np.repeat(g, 100), np.tile(g, 100), np.zeros(10000)], 1)             # a 1 cm grid: ~400 points on the boundary
    pred = {'conf': np.zeros(1, np.float32), 'label_id': np.array([5], np.int32), 'mask': np.ones((1, 10000), bool)}
    bits, words, n = D.pack_masks(pred['mask'])
    raw = D.hulls_from_bits(bits, words, n, pos, cap=64)
    assert raw['flags'].cpu().tolist() == [D.FLAG_CANDIDATES] and raw['n_hull'].cpu().tolist() == [0]
    assert int(raw['ncand'][0]) > 64
    out = D.mask_boxes(pred, pos, cap=64)                                                # second pass with the capacity the first asked for
    v = out['hull'][0, :int(out['n_hull'][0])].cpu().numpy()
    assert np.array_equal(v, [[0.0, 0.0], [g[99], 0.0], [g[99], g[99]], [0.0, g[99]]])   # no collinear vertex kept


def test_two_runs_give_identical_bytes(gold):
    from box2mask_amd import eval_detection as D
    pred, pos, labels = _scene(gold, 1)

    def run():
        boxes, gt = D.mask_boxes(pred, pos), D.gt_boxes(labels)
        return [boxes[k].cpu().numpy().tobytes() for k in ('count', 'box6', 'hull', 'n_hull', 'flags')] + \
               [D.scene_ious(boxes, gt, o).tobytes() for o in (True, False)] + [gt['boxes'].cpu().numpy().tobytes()]
    assert run() == run()


def test_gt_boxes_match_the_restated_corners(gold):
    from box2mask_amd import eval_detection as D
    for s in range(int(gold['n_scenes'])):
        _, _, labels = _scene(gold, s)
        rec = D.gt_boxes(labels)['boxes'].cpu().numpy()
        c = labels['per_instance_bb_centers'].astype(np.float64)
        b = labels['per_instance_bb_bounds'].astype(np.float64)
        for i in range(len(c)):
            R = labels['per_instance_bb_rotations'][i].reshape(3, 3).T
            signs = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]])
            corners = (signs * b[i]) @ R.T + c[i]
            assert np.abs(rec[i, :8].reshape(4, 2) - corners[:4, :2]).max() <= 1e-14
            assert abs(rec[i, 8] - corners[0, 2]) <= 1e-14 and abs(rec[i, 9] - corners[7, 2]) <= 1e-14
            assert abs(rec[i, 10] - 8 * b[i].prod()) <= 1e-13
            assert np.abs(rec[i, 11:14] - 2 * np.maximum((signs * b[i]) @ R.T, 0).max(0)).max() <= 1e-14
