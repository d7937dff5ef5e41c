"""GPU: the threshold sweep scored with the ARKitScenes detection mAP (param_search.detection_tables / detection_records /
arkit_param_search).

  * the 36 settings of tests/golden/arkit_sweep.npz and the case off the grid against what the real reference returned: scored
    rows and counts exact, IoU within _detbox_rule.IOU_TOL, per-class AP and mAP bit for bit, both ``oriented_boxes`` values, both
    thresholds;
  * four settings, ``best`` among them, against the single-setting path -- Model.pred2mask + eval_detection.scene_record /
    arkitscenes_eval -- bit for bit: both paths run the same kernels on the same points;
  * a candidate buffer of 64 forces the second hull pass and changes nothing; a setting that keeps no cluster; the refusals;
  * scannet_param_search on the same batch still reproduces param_sweep.npz."""
import os

import numpy as np
import pytest
import torch

import _det_sweep_rule as A
import _sweep_rule as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def model():
    from box2mask_amd import synth
    from box2mask_amd.config import scannet_config
    from box2mask_amd.model import Model
    return Model(scannet_config(), *synth.scannet_tables())


@pytest.fixture(scope='module')
def fx(golden_dir):
    sw = np.load(os.path.join(golden_dir, 'param_sweep.npz'))
    ak = np.load(os.path.join(golden_dir, 'arkit_sweep.npz'))
    return sw, ak, W.fixture_grid(sw)


def _inputs(fx, gate=False):
    """(batch, pred, ground-truth ids): the batch of param_sweep.npz in the layout of the ARKitScenes loader -- scenes with
    ``positions``, ``batch['labels']`` with the boxes."""
    sw, ak, _ = fx
    batch, pred, gts = W.fixture_batch(sw)
    extra = A.fixture_inputs(sw, ak, gate)
    batch['vox2point'] = [np.asarray(scene['vox2point']) for scene, _, _ in extra]
    for sc, (_, pos, _) in zip(batch['scene'], extra):
        sc['positions'] = pos
    batch['labels'] = [lab for _, _, lab in extra]
    return batch, pred, gts


def _bytes(rec):
    return {k: (np.asarray(v).dtype.str, np.asarray(v).shape, np.asarray(v).tobytes()) for k, v in rec.items()}


@pytest.mark.parametrize('oriented', [True, False])
def test_sweep_reproduces_every_setting_of_the_reference(model, fx, oriented):
    from box2mask_amd import param_search
    sw, ak, grid = fx
    vt = 'obb' if oriented else 'aabb'
    batch, pred, _ = _inputs(fx)
    tabs = model.pred2mask_detection_sweep(batch, pred, grid, oriented_boxes=oriented)
    assert [t.name for t in tabs] == [s['name'] for s in batch['scene']]
    res = param_search.arkit_param_search(model, [(batch, pred)], grid, oriented_boxes=oriented, iou_t=list(A.THRESHOLDS), per_class=True)
    assert res['map'].shape == grid.shape + (2,) and 1 <= res['n_evaluated'] <= 36
    for q, st in enumerate(grid.settings()):
        recs = {t.name: param_search.detection_records(t, *st) for t in tabs}
        counts = [t.stages[st[0]][st[2]]['count'][param_search.compose(t, *st)] for t in tabs]
        A.check_setting(ak, 'q%02d' % q, recs, vt, counts)                  # (the matching restated in the rule)
        for ti, th in enumerate(A.THRESHOLDS):                              # ... and the product's own
            key = 'ak_q%02d_%s_%d_' % (q, vt, round(th * 100))
            ap = res['ap_by_class'][st][ti]
            assert [int(c) for c in ap] == ak[key + 'classes'].tolist(), (st, th)
            assert A.same_floats([ap[c] for c in ap], ak[key + 'ap']) and A.same_floats(res['map'][st][ti], ak[key + 'map']), (st, th)
    flat = res['map'][..., 0].reshape(-1)
    order = sorted(range(36), key=lambda q: (-flat[q] if not np.isnan(flat[q]) else np.inf, q))
    assert res['best'] == tuple(int(v) for v in np.unravel_index(order[0], grid.shape)) and res['best_ths'] == grid.eval_ths(*res['best'])
    one = param_search.arkit_param_search(model, [(batch, pred)], grid, oriented_boxes=oriented)      # a scalar iou_t: no trailing axis
    assert one['map'].shape == grid.shape and A.same_floats(one['map'], res['map'][..., 0]) and one['best'] == res['best']
    # the case off the grid: a row of exactly 50 points is scored, a thinned row that suppresses a larger one still suppresses it
    gbatch, gpred, _ = _inputs(fx, gate=True)
    gate = param_search.ThresholdGrid(*([getattr(grid, a)[i]] for a, i in zip(param_search.AXES, ak['ak_gate_setting'])))
    gtabs = model.pred2mask_detection_sweep(gbatch, gpred, gate, oriented_boxes=oriented)
    recs = {t.name: param_search.detection_records(t, 0, 0, 0, 0) for t in gtabs}
    counts = [t.stages[0][0]['count'][param_search.compose(t, 0, 0, 0, 0)] for t in gtabs]
    A.check_setting(ak, 'gate', recs, vt, counts)
    assert (counts[0] == A.MIN_POINTS).sum() == 1 and (counts[0] < A.MIN_POINTS).any()


def test_sweep_equals_the_single_setting_path(model, fx):
    from box2mask_amd import eval_detection, param_search
    sw, ak, grid = fx
    batch, pred, _ = _inputs(fx)
    saved = model.cfg.eval_ths
    try:
        for oriented in (True, False):
            tabs = model.pred2mask_detection_sweep(batch, pred, grid, oriented_boxes=oriented)
            res = param_search.arkit_param_search(model, [(batch, pred)], grid, oriented_boxes=oriented, iou_t=[0.5, 0.25])
            for st in {res['best'], (0, 0, 0, 0), (2, 2, 1, 0), (1, 0, 1, 1)}:
                model.cfg.eval_ths = grid.eval_ths(*st)
                want = model.pred2mask(batch, pred, 'eval')
                for t, sc, lab in zip(tabs, batch['scene'], batch['labels']):
                    rec = eval_detection.scene_record(want[t.name], sc['positions'], lab, oriented_boxes=oriented)
                    assert _bytes(param_search.detection_records(t, *st)) == _bytes(rec), (oriented, st, t.name)
                for ti, th in enumerate((0.5, 0.25)):
                    m, _ = eval_detection.arkitscenes_eval(want, batch['scene'], batch['labels'], oriented_boxes=oriented, iou_t=th,
                                                           verbose=False)
                    assert A.same_floats(res['map'][st][ti], m), (oriented, st, th)
    finally:
        model.cfg.eval_ths = saved


def test_small_candidate_buffer_forces_a_second_pass_and_changes_nothing(model, fx, monkeypatch):
    from box2mask_amd import param_search
    sw, ak, grid = fx
    batch, pred, _ = _inputs(fx)
    calls = []
    real = param_search._call
    monkeypatch.setattr(param_search, '_call', lambda name, *a: (calls.append((name, a[2]) if name == 'b2m_mask_hulls_index_batch' else None),
                                                                 real(name, *a))[1])
    # every point on a side of the unit square, at dyadic coordinates: no point is strictly inside the polygon of the extremes, so
    # a row of n points has n hull candidates (and 4 to 8 hull vertices)
    rng = np.random.default_rng(5)
    positions = []
    for sc in batch['scene']:
        n = len(sc['positions'])
        t, side = rng.integers(0, 1025, n) / 1024.0, rng.integers(0, 4, n)
        xy = np.where((side < 2)[:, None], np.stack([t, (side == 1) * 1.0], 1), np.stack([(side == 3) * 1.0, t], 1))
        positions.append(np.concatenate([xy, rng.random((n, 1))], 1))
    want = model.pred2mask_detection_sweep(batch, pred, grid, positions=positions, cap=32768)
    n_first = len([c for c in calls if c])
    assert n_first == grid.shape[0] * grid.shape[2] and all(c[1] == 32768 for c in calls if c)         # one hull stage per (ci, bi)
    del calls[:]
    got = model.pred2mask_detection_sweep(batch, pred, grid, positions=positions, cap=64)
    caps = [c[1] for c in calls if c]
    assert len(caps) == 2 * n_first and caps[::2] == [64] * n_first and all(64 < c <= 32768 for c in caps[1::2])
    assert max(int(st['count'].max()) for t in want for row in t.stages for st in row) > 64
    for a, b in zip(want, got):
        for ci in range(grid.shape[0]):
            for bi in range(grid.shape[2]):
                assert _bytes(a.stages[ci][bi]) == _bytes(b.stages[ci][bi]), (a.name, ci, bi)
    with pytest.raises(ValueError, match='cap'):
        model.pred2mask_detection_sweep(batch, pred, grid, cap=100)


def test_setting_that_keeps_no_cluster(model, fx):
    """score_th above every score: no prediction, no class is scored, the mAP is NaN and ranks last."""
    from box2mask_amd import param_search
    batch, pred, _ = _inputs(fx)
    grid = param_search.ThresholdGrid([0.5], [0.05, 1.5], [0.3], [0.6])
    tabs = model.pred2mask_detection_sweep(batch, pred, grid)
    for t in tabs:
        r = param_search.detection_records(t, 0, 1, 0, 0)
        assert t.clusters[0]['ks'][1] == 0 and len(r['label']) == 0 and r['iou'].shape == (0, len(t.gt_label))
    res = param_search.arkit_param_search(model, [(batch, pred)], grid)
    assert res['best'] == (0, 0, 0, 0) and np.isnan(res['map'][0, 1, 0, 0]) and res['map'][0, 0, 0, 0] > 0
    # ... and a grid no setting of which keeps one: no row is projected, no hull is taken
    none = param_search.ThresholdGrid([0.5], [1.5], [0.3], [0.6])
    for t in model.pred2mask_detection_sweep(batch, pred, none):
        st = t.stages[0][0]
        assert st['keep'].shape == (1, 0) and st['iou'].shape == (0, len(t.gt_label)) and len(st['count']) == 0
    assert np.isnan(param_search.arkit_param_search(model, [(batch, pred)], none)['map']).all()


def test_refusals(model, fx):
    sw, ak, grid = fx
    batch, pred, _ = _inputs(fx)
    net = model.detection_model
    net.requires_voxel_outputs = True
    try:
        with pytest.raises(ValueError, match='requires_voxel_outputs'):
            model.pred2mask_detection_sweep(batch, pred, grid)
    finally:
        net.requires_voxel_outputs = False
    with pytest.raises(ValueError, match='positions'):
        model.pred2mask_detection_sweep(batch, pred, grid, positions=[s['positions'][:-1] for s in batch['scene']])
    with pytest.raises(ValueError, match='labels without boxes'):
        model.pred2mask_detection_sweep(batch, pred, grid, labels=[{'per_instance_semantics': np.zeros(3)}] * 2)
    with pytest.raises(ValueError, match='ground-truth boxes'):
        model.pred2mask_detection_sweep({k: v for k, v in batch.items() if k != 'labels'}, pred, grid)
    bg = dict(pred)
    sem = torch.full_like(pred['mlp_semantics'], -10.0)
    sem[:, 0] = 10.0                                                        # class id 1 for every vote: no foreground
    bg['mlp_semantics'] = sem
    with pytest.raises(ValueError, match='at least one box'):
        model.pred2mask_detection_sweep(batch, bg, grid)


def test_scannet_search_on_the_same_batch_is_unchanged(model, fx):
    from box2mask_amd import param_search
    sw, ak, grid = fx
    batch, pred, gts = _inputs(fx)
    res = param_search.scannet_param_search(model, [(batch, pred)], gts, grid, per_class=True)
    for q, st in enumerate(grid.settings()):
        assert A.same_floats(res['ap_tables'][st], sw['sw_q%02d_ap' % q]) and A.same_floats(res['ap'][st], sw['sw_q%02d_avg' % q]), st
