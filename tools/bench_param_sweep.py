"""The threshold sweep (box2mask_amd/param_search.py) on ScanNet-shaped inputs, beside the same settings through the single-setting
path: scenes of ~150 k voxels from synth.make_batch, votes as bench.py's votes leg makes them (every segment votes for its object's
box with 2.5 cm noise, score logits ~ N(0, 2)), the default 6 x 5 x 4 x 5 grid.

    python tools/bench_param_sweep.py [--scenes 8] [--voxels 150000] [--loop-settings 12] [--metric scannet|arkit|s3dis]

Reports the device ms of the sweep's stages (HIP events round every launch, a pass of its own: the events serialise the stream),
the wall time of the sweep up to the tables, the wall time of the host matching of all settings, and the looped path --
Model.pred2mask + eval_metric.compute_eval per setting -- timed on `--loop-settings` settings spread evenly over the grid and
scaled to the grid (0 = every setting).  The looped settings' APs are compared with the sweep's.  Then the same search with
matching='device' (box2mask_amd/eval_match.py): its wall time up to the AP table beside the host route's of this very run, the
device ms of its row-table, matching, sort and curve launches (HIP events round every launch, the median over `--device-runs`
timed searches after a warm-up) and the largest difference between the two routes' averages.  One JSON line at the end.

--metric arkit: the same scenes, votes and grid scored with the oriented-box detection mAP (param_search.arkit_param_search; the
rooms' furniture boxes as ground truth): device ms per stage with the hull passes (b2m_mask_hulls_index_batch) and the IoU calls,
the wall time of the tables and of the whole search, and the looped path -- Model.pred2mask + eval_detection.arkitscenes_eval per
setting -- on `--loop-settings` settings, scaled to the grid, with its mAPs compared with the sweep's.

--metric s3dis: `--scenes` synthetic S3DIS-shaped rooms (batches of one; the rooms of tools/bench_eval_s3dis.py: floor -> class 1, three
walls -> wall, one -> ceiling, furniture -> classes 3 .. 12, per-voxel semantics with 2 % wrong voxels), the 6 x 5 x 4 grid of config.py
(mask_nms_th has no effect in this flow) through param_search.s3dis_param_search, beside the same settings one by one through
eval_s3dis.evaluate_rooms with cfg.eval_ths set (`--loop-settings`, 0 = all 120) in the same process.  Both routes read the same
synthetic head outputs: the network forward is in neither time.  Device ms per stage (DBSCAN, clustering, projection / gather,
paint, tail) from a pass of its own with HIP events round every stage; mPrec / mRec of the looped settings are compared bit for bit.
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import synthetic_votes                                  # noqa: E402
from box2mask_amd import _lib, eval_metric, param_search, synth   # noqa: E402
from box2mask_amd.config import scannet_config                    # noqa: E402
from box2mask_amd.model import Model                              # noqa: E402

AP_STAGES = ('b2m_ap_rows', 'b2m_ap_match', 'b2m_sort_u64', 'b2m_ap_curve')
ARKIT_STAGES = ('b2m_nmc_batch', 'b2m_mask_project_batch', 'b2m_mask_nms_sweep_batch', 'b2m_label_hist_batch',
                'b2m_mask_hulls_index_batch', 'b2m_hull_box_iou')
STAGES = ('b2m_nmc_batch', 'b2m_mask_project_batch', 'b2m_mask_nms_sweep_batch', 'b2m_label_hist_batch', 'b2m_mask_hist_index_batch')


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', type=int, default=8)
    ap.add_argument('--voxels', type=int, default=150000)
    ap.add_argument('--loop-settings', type=int, default=12, help='settings the looped path is timed on, scaled to the grid (0 = all)')
    ap.add_argument('--device-runs', type=int, default=5, help='timed searches with matching=device (median)')
    ap.add_argument('--metric', choices=('scannet', 'arkit', 's3dis'), default='scannet')
    args = ap.parse_args(argv)
    if args.metric == 's3dis':
        return s3dis_leg(args)
    cfg = scannet_config()
    model = Model(cfg, *synth.scannet_tables())
    model.eval()
    if args.metric == 'arkit':
        return arkit_leg(args, cfg, model)
    batch = synth.make_batch(args.scenes, seed0=0, target_voxels=args.voxels)
    pred, _ = synthetic_votes(batch, cfg)
    gts = {sc['name']: synth.gt_instance_ids(batch, b) for b, sc in enumerate(batch['scene'])}
    grid = param_search.ThresholdGrid.from_cfg(cfg)
    n_set = int(np.prod(grid.shape))
    note = lambda msg: print('[bench_param_sweep] ' + msg, file=sys.stderr, flush=True)
    note('%d scenes, %d voxels, %d settings' % (args.scenes, batch['vox_coords'].shape[0], n_set))
    model.pred2mask_sweep(batch, pred, grid, gts)                                       # warm-up
    tabs, sweep_s = wall(lambda: model.pred2mask_sweep(batch, pred, grid, gts))
    # device time per stage
    rec = []

    def hook(name, a, meta=None):
        if name not in STAGES:
            return None
        s_, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s_.record()

        def done():
            e_.record()
            rec.append((name, s_, e_))
        return done
    _lib.set_hook(hook)
    model.pred2mask_sweep(batch, pred, grid, gts)
    torch.cuda.synchronize()
    _lib.set_hook(None)
    stages = {n: {'launches': 0, 'ms': 0.0} for n in STAGES}
    for name, s_, e_ in rec:
        stages[name]['launches'] += 1
        stages[name]['ms'] += s_.elapsed_time(e_)
    note('sweep %.3f s; matching every setting ...' % sweep_s)
    # the whole search: sweep + records + matching of every setting
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        res, search_s = wall(lambda: param_search.scannet_param_search(model, [(batch, pred)], gts, grid))
    note('search %.1f s; the device route ...' % search_s)
    # the same search with the matching on the device: wall time up to the AP table, then the device ms of its launches
    device_search = lambda: param_search.scannet_param_search(model, [(batch, pred)], gts, grid, matching='device')
    device_search()                                                                     # warm-up
    walls, per_run = [], []
    for _ in range(max(args.device_runs, 1)):
        dres, dt = wall(device_search)
        walls.append(dt)
    for _ in range(max(args.device_runs, 1)):
        rec_ap = []

        def ap_hook(name, a, meta=None):
            if name not in AP_STAGES:
                return None
            s_, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s_.record()

            def done():
                e_.record()
                rec_ap.append((name, s_, e_))
            return done
        _lib.set_hook(ap_hook)
        device_search()
        torch.cuda.synchronize()
        _lib.set_hook(None)
        per_run.append({n: (sum(1 for m, _, _ in rec_ap if m == n), sum(s_.elapsed_time(e_) for m, s_, e_ in rec_ap if m == n))
                        for n in AP_STAGES})
    ap_stages = {n: {'launches': per_run[0][n][0], 'ms': round(float(np.median([r[n][1] for r in per_run])), 3)} for n in AP_STAGES}
    both = ~np.isnan(res['ap'])
    ap_diff = float(np.max(np.abs(dres['ap'] - res['ap'])[both], initial=0.0))
    same_nan = bool(np.array_equal(np.isnan(dres['ap']), np.isnan(res['ap'])))
    note('device search %.3f s; the looped path ...' % float(np.median(walls)))
    # the looped path on a subset
    settings = list(grid.settings())
    n_loop = n_set if args.loop_settings <= 0 else min(args.loop_settings, n_set)
    chosen = [settings[i] for i in np.unique(np.linspace(0, n_set - 1, n_loop).round().astype(int))]
    saved, agree = cfg.eval_ths, True
    model.cfg.eval_ths = grid.eval_ths(*chosen[0])
    eval_metric.compute_eval(model.pred2mask(batch, pred, 'eval'), gts)                  # warm-up
    t_mask = t_eval = 0.0
    for st in chosen:
        model.cfg.eval_ths = grid.eval_ths(*st)
        r, dt = wall(lambda: model.pred2mask(batch, pred, 'eval'))
        t_mask += dt
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            (avg, _), dt = wall(lambda: eval_metric.compute_eval(r, gts))
        t_eval += dt
        agree &= bool(np.array_equal(res['ap'][st], [avg['all_ap'], avg['all_ap_50%'], avg['all_ap_25%']], equal_nan=True))
    model.cfg.eval_ths = saved
    scale = n_set / len(chosen)
    out = {'scenes': args.scenes, 'voxels': int(batch['vox_coords'].shape[0]), 'points': int(sum(t.n_pts for t in tabs)),
           'segments': int(batch['input_location'].shape[0]), 'grid': list(grid.shape), 'settings': n_set,
           'clusters_per_cluster_th': [int(sum(t.clusters[ci]['K'] for t in tabs)) for ci in range(grid.shape[0])],
           'projected_rows_per_cluster_th': [int(sum(t.clusters[ci]['ks'][0] for t in tabs)) for ci in range(grid.shape[0])],
           'stages': {n: {'launches': v['launches'], 'ms': round(v['ms'], 3)} for n, v in stages.items()},
           'stages_device_ms': round(sum(v['ms'] for v in stages.values()), 3),
           'sweep_wall_s': round(sweep_s, 4), 'search_wall_s': round(search_s, 3),
           'host_matching_s': round(search_s - sweep_s, 3), 'distinct_record_sets_matched': res['n_evaluated'],
           'device_search_wall_s': round(float(np.median(walls)), 4), 'device_search_wall_runs_s': [round(w, 4) for w in walls],
           'device_stages': ap_stages,
           'device_stages_device_ms': round(sum(v['ms'] for v in ap_stages.values()), 3),
           'device_best_equals_host_best': dres['best'] == res['best'], 'device_vs_host_max_abs_diff': ap_diff,
           'device_nan_pattern_equals_host': same_nan,
           'best': res['best_ths'], 'best_ap_ap50_ap25': [float(v) for v in res['ap'][res['best']]],
           'looped_settings_timed': len(chosen), 'looped_pred2mask_s': round(t_mask, 3), 'looped_compute_eval_s': round(t_eval, 3),
           'looped_scaled_to_grid_s': round((t_mask + t_eval) * scale, 1), 'looped_is_scaled': len(chosen) != n_set,
           'looped_ap_equals_sweep_ap': agree}
    print(json.dumps(out))


def arkit_leg(args, cfg, model):
    from box2mask_amd import eval_detection
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from train_synthetic import box_labels
    batch = synth.make_batch(args.scenes, seed0=0, target_voxels=args.voxels)
    pred, _ = synthetic_votes(batch, cfg)
    # the layout of the ARKitScenes loader: the scenes carry the positions vox2point indexes, the batch the boxes
    raws = [synth.make_scene(s, target_voxels=args.voxels, points_only=True) for s in range(args.scenes)]
    for sc, raw, v2p in zip(batch['scene'], raws, batch['vox2point']):
        assert len(raw['positions']) == len(v2p)
        sc['positions'] = raw['positions']
    batch['labels'] = [box_labels(r) for r in raws]
    grid = param_search.ThresholdGrid.from_cfg(cfg)
    n_set = int(np.prod(grid.shape))
    note = lambda msg: print('[bench_param_sweep] ' + msg, file=sys.stderr, flush=True)
    note('arkit: %d scenes, %d voxels, %d settings' % (args.scenes, batch['vox_coords'].shape[0], n_set))
    model.pred2mask_detection_sweep(batch, pred, grid)                                  # warm-up
    tabs, sweep_s = wall(lambda: model.pred2mask_detection_sweep(batch, pred, grid))
    rec = []

    def hook(name, a, meta=None):
        if name not in ARKIT_STAGES:
            return None
        s_, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s_.record()

        def done():
            e_.record()
            rec.append((name, s_, e_))
        return done
    _lib.set_hook(hook)
    model.pred2mask_detection_sweep(batch, pred, grid)
    torch.cuda.synchronize()
    _lib.set_hook(None)
    stages = {n: {'launches': 0, 'ms': 0.0} for n in ARKIT_STAGES}
    for name, s_, e_ in rec:
        stages[name]['launches'] += 1
        stages[name]['ms'] += s_.elapsed_time(e_)
    note('tables %.3f s; the whole search ...' % sweep_s)
    res, search_s = wall(lambda: param_search.arkit_param_search(model, [(batch, pred)], grid))
    note('search %.1f s; the looped path ...' % search_s)
    settings = list(grid.settings())
    n_loop = n_set if args.loop_settings <= 0 else min(args.loop_settings, n_set)
    chosen = [settings[i] for i in np.unique(np.linspace(0, n_set - 1, n_loop).round().astype(int))]
    saved, agree = cfg.eval_ths, True
    model.cfg.eval_ths = grid.eval_ths(*chosen[0])
    one = lambda r: eval_detection.arkitscenes_eval(r, batch['scene'], batch['labels'], oriented_boxes=True, iou_t=0.5, verbose=False)
    one(model.pred2mask(batch, pred, 'eval'))                                           # warm-up
    t_mask = t_eval = 0.0
    for st in chosen:
        model.cfg.eval_ths = grid.eval_ths(*st)
        r, dt = wall(lambda: model.pred2mask(batch, pred, 'eval'))
        t_mask += dt
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            (m, _), dt = wall(lambda: one(r))
        t_eval += dt
        agree &= bool(np.array_equal(res['map'][st], m, equal_nan=True))
    model.cfg.eval_ths = saved
    scale = n_set / len(chosen)
    hull = stages['b2m_mask_hulls_index_batch']
    out = {'metric': 'arkit', 'scenes': args.scenes, 'voxels': int(batch['vox_coords'].shape[0]), 'points': int(sum(t.n_pts for t in tabs)),
           'ground_truth_boxes': int(sum(len(t.gt_label) for t in tabs)), 'grid': list(grid.shape), 'settings': n_set,
           'projected_rows_per_cluster_th': [int(sum(t.clusters[ci]['ks'][0] for t in tabs)) for ci in range(grid.shape[0])],
           'stages': {n: {'launches': v['launches'], 'ms': round(v['ms'], 3)} for n, v in stages.items()},
           'hull_ms_per_stage': round(hull['ms'] / max(hull['launches'], 1), 3),
           'iou_ms_per_stage': round(stages['b2m_hull_box_iou']['ms'] / max(hull['launches'], 1), 3),
           'stages_device_ms': round(sum(v['ms'] for v in stages.values()), 3),
           'tables_wall_s': round(sweep_s, 4), 'search_wall_s': round(search_s, 3), 'host_matching_s': round(search_s - sweep_s, 3),
           'distinct_record_sets_matched': res['n_evaluated'], 'best': res['best_ths'], 'best_map': float(res['map'][res['best']]),
           'looped_settings_timed': len(chosen), 'looped_pred2mask_s': round(t_mask, 3), 'looped_arkitscenes_eval_s': round(t_eval, 3),
           'looped_scaled_to_grid_s': round((t_mask + t_eval) * scale, 1), 'looped_is_scaled': len(chosen) != n_set,
           'looped_map_equals_sweep_map': agree}
    print(json.dumps(out))


def s3dis_room(seed, voxels, cfg):
    """One S3DIS-shaped room as a batch of one and its head outputs: the votes of bench.py's votes leg, per-voxel semantics."""
    batch = synth.make_batch(1, seed0=seed, target_voxels=voxels)
    pred, _ = synthetic_votes(batch, cfg, seed=7 + seed)
    pred.pop(cfg.mlp_semantics, None)
    raw = synth.make_scene(seed, target_voxels=voxels, points_only=True)
    v2p = np.asarray(batch['vox2point'][0])
    assert len(raw['positions']) == len(v2p)
    inst = raw['labels']['seg2inst'][raw['segments']].astype(np.int64)
    cls = raw['labels']['per_instance_semantics'][inst]
    sem = np.where(cls == 2, 1, 3 + inst % 10)                          # floor -> 1, furniture -> 3 .. 12
    wall = cls == 1
    sem[wall] = np.where(raw['normals'][wall, 0] < 0, 0, 2)              # three walls predicted as wall, one as ceiling
    n_vox = int(batch['vox_coords'].shape[0])
    vox_sem = np.zeros(n_vox, np.int64)
    vox_sem[v2p] = sem
    rng = np.random.default_rng(seed)
    wrong = rng.random(n_vox) < 0.02
    vox_sem[wrong] = rng.integers(0, 13, int(wrong.sum()))
    pred[cfg.mlp_per_vox_semantics] = torch.from_numpy(np.eye(13, dtype=np.float32)[vox_sem])
    batch['scene'][0]['positions'], batch['scene'][0]['normals'] = raw['positions'], raw['normals']
    batch['labels'] = [{'semantics': sem, 'instances': inst}]
    for k in ('input_location', 'batch_ids'):
        batch[k] = batch[k].cpu()
    return batch, pred


class _Votes:
    """evaluate_rooms' model: the synthetic head outputs instead of a forward, the real votes -> masks pass."""

    def __init__(self, model, preds):
        self.model, self.cfg, self.preds = model, model.cfg, preds

    def get_prediction(self, batch, **kw):
        return {k: v.clone() for k, v in self.preds[batch['scene'][0]['name']].items()}

    def pred2mask(self, batch, pred, mode):
        return self.model.pred2mask(batch, pred, mode)


def s3dis_leg(args):
    from box2mask_amd import eval_s3dis
    cfg = scannet_config(network_heads=['mlp_offsets', 'mlp_bounds', 'mlp_bb_scores', 'mlp_per_vox_semantics'])
    ids = torch.arange(13).long()
    model = Model(cfg, torch.Tensor(np.arange(13)), ids, ids.clone(), (lambda s_: s_ > 2))
    model.eval()
    note = lambda msg: print('[bench_param_sweep] ' + msg, file=sys.stderr, flush=True)
    items = [s3dis_room(s_, args.voxels, cfg) for s_ in range(args.scenes)]
    for i, (b, _) in enumerate(items):
        b['scene'][0]['name'] = 'room%d' % i
    grid = param_search.ThresholdGrid.from_cfg(cfg)
    nc, ns, nb, _ = grid.shape
    n_set = nc * ns * nb
    note('s3dis: %d rooms, %s points, %d settings' % (args.scenes, [len(b['vox2point'][0]) for b, _ in items], n_set))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        param_search.s3dis_param_search(model, items, grid)                             # warm-up
        res, sweep_s = wall(lambda: param_search.s3dis_param_search(model, items, grid, per_class=True))
        stages = {}
        param_search.s3dis_param_search(model, items, grid, timing=stages)             # a pass of its own: the events synchronise
    note('sweep %.3f s; the looped path ...' % sweep_s)
    settings = [(ci, si, bi) for ci in range(nc) for si in range(ns) for bi in range(nb)]
    n_loop = n_set if args.loop_settings <= 0 else min(args.loop_settings, n_set)
    chosen = [settings[i] for i in np.unique(np.linspace(0, n_set - 1, n_loop).round().astype(int))]
    votes = _Votes(model, {b['scene'][0]['name']: p for b, p in items})
    batches = [b for b, _ in items]
    saved, agree, t_loop = cfg.eval_ths, True, 0.0
    cfg.eval_ths = grid.eval_ths(*chosen[0], 0)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        eval_s3dis.evaluate_rooms(votes, batches)                                       # warm-up
        for st in chosen:
            cfg.eval_ths = grid.eval_ths(*st, 0)
            (mprec, mrec, _, _), dt = wall(lambda: eval_s3dis.evaluate_rooms(votes, batches))
            t_loop += dt
            if (chosen.index(st) + 1) % 10 == 0:
                note('%d of %d settings one by one: %.1f s' % (chosen.index(st) + 1, len(chosen), t_loop))
            agree &= bool(np.array_equal(res['mprec'][st], mprec, equal_nan=True) and np.array_equal(res['mrec'][st], mrec, equal_nan=True))
    cfg.eval_ths = saved
    scale = n_set / len(chosen)
    looped = t_loop * scale
    order = ('dbscan', 'clustering', 'projection', 'paint', 'tail')
    out = {'metric': 's3dis', 'rooms': args.scenes, 'points': [int(len(b['vox2point'][0])) for b, _ in items],
           'voxels': [int(b['vox_coords'].shape[0]) for b, _ in items], 'grid': [nc, ns, nb], 'settings': n_set,
           'stages_device_ms': {k: round(float(stages.get(k, 0.0)), 3) for k in order},
           'stage_calls': {'dbscan': args.scenes, 'clustering': args.scenes * nc, 'projection': args.scenes * nc * nb,
                           'paint': args.scenes * nc * nb, 'tail': args.scenes * nc * nb},
           'sweep_wall_s': round(sweep_s, 4), 'looped_settings_timed': len(chosen), 'looped_wall_s': round(t_loop, 3),
           'looped_scaled_to_grid_s': round(looped, 2), 'looped_is_scaled': len(chosen) != n_set,
           'speedup': round(looped / sweep_s, 2), 'stage_ratio': round(n_set / (nc * nb), 2),
           'looped_metric_equals_sweep': agree, 'best': res.best(),
           'finite_settings': int(np.isfinite(res['mprec']).sum())}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
