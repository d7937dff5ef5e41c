"""Threshold search on the checkpoint tools/train_synthetic.py writes: every setting of the `*_th_search` grid (config.py; the
reference's `--param_search`, models/evaluation.py:353-366) scored with the ScanNet AP over the validation scenes, in one pass.

    python tools/train_synthetic.py --scenes 4 --voxels 20000 --steps 200 --checkpoint-dir /tmp/b2m_ckpt
    python tools/param_search.py --checkpoint-dir /tmp/b2m_ckpt --scenes 4 --voxels 20000 [--batch-size 2] [--top 10] [--check 5]
                                 [--matching host|device] [--metric scannet|arkit]
    python tools/param_search.py --metric s3dis [--scenes 2] [--voxels 20000] [--top 10] [--check 5]

The scenes are train_synthetic's (seeds 0 .. scenes-1: it validates on the scenes it trains on).  Prints the best settings and the
winner as an `eval_ths` line.  --check N re-evaluates N settings spread over the grid (the winner among them) through
Model.pred2mask and eval_metric.compute_eval and compares the three averages: exactly with --matching host; with --matching
device (matching, curves and AP of every setting on the device, box2mask_amd/eval_match.py) within 4 n 2^-53 + 2^-50, n = one more
than three entries per predicted mask of the setting (the longest curve it can give).  A difference is an error.

--metric arkit scores the same grid with the oriented-box detection mAP of ARKitScenes instead (param_search.arkit_param_search;
the furniture boxes of the synthetic rooms as labels, train_synthetic.box_labels), and --check compares with Model.pred2mask +
eval_detection.arkitscenes_eval: the mAP must be equal bit for bit.

--metric s3dis scores the grid with the S3DIS mPrec / mRec (param_search.s3dis_param_search; mask_nms_th has no effect in that flow).
train_synthetic trains no per-voxel semantics head, so this runs without a checkpoint on the synthetic S3DIS-shaped rooms and head
outputs of tools/bench_param_sweep.py (s3dis_room).  The winner is ``best()``: the largest harmonic mean of mPrec and mRec.  --check
re-evaluates N settings through Model.pred2mask + eval_s3dis.room_labels + s3dis_counts and demands the same true / false positives
and ground-truth counts per class, and the same mPrec / mRec bit for bit.
"""
import argparse
import os
import sys
import time
import warnings
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from box2mask_amd import eval_detection, eval_metric, param_search, synth    # noqa: E402
from box2mask_amd.config import scannet_config                # noqa: E402
from box2mask_amd.model import Model                          # noqa: E402
import train_synthetic as T                                   # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--checkpoint-dir', default=None)
    ap.add_argument('--scenes', type=int, default=4)
    ap.add_argument('--voxels', type=int, default=20000)
    ap.add_argument('--batch-size', type=int, default=2)
    ap.add_argument('--top', type=int, default=10, help='settings to print (0 = the whole table)')
    ap.add_argument('--check', type=int, default=0, help='settings to re-evaluate through Model.pred2mask + compute_eval')
    ap.add_argument('--matching', choices=('host', 'device'), default='host', help='where the matching and the AP of the settings run')
    ap.add_argument('--metric', choices=('scannet', 'arkit', 's3dis'), default='scannet',
                    help='ScanNet AP, the ARKitScenes detection mAP, or the S3DIS mPrec / mRec')
    ap.add_argument('--iou-t', type=float, default=0.5, help='--metric arkit: the IoU threshold of a match')
    for axis in param_search.AXES:
        ap.add_argument('--%s_search' % axis, nargs=3, type=float, default=None, metavar=('MIN', 'MAX', 'NUM'),
                        help='np.linspace triple (default: config.py, the reference\'s)')
    args = ap.parse_args(argv)
    if args.metric == 's3dis':
        return s3dis(args)
    if args.checkpoint_dir is None:
        ap.error('--checkpoint-dir is required for --metric %s' % args.metric)
    cfg = scannet_config(mlp_bb_scores_start_epoch=0)
    cfg.checkpoint_path = args.checkpoint_dir.rstrip('/') + '/'
    for axis in param_search.AXES:
        if getattr(args, axis + '_search') is not None:
            setattr(cfg, axis + '_search', getattr(args, axis + '_search'))
    grid = param_search.ThresholdGrid.from_cfg(cfg)
    model = Model(cfg, *synth.scannet_tables())
    loaded = model.load_checkpoint()
    if len(loaded) < 3:
        raise SystemExit('no checkpoint under %s' % cfg.checkpoint_path)
    model.eval()
    sup = SimpleNamespace(smallest_bb_heuristic=True)
    items, gts = [], {}
    for b0 in range(0, args.scenes, args.batch_size):
        batch, raws = T.build_batch(range(b0, min(b0 + args.batch_size, args.scenes)), args.voxels, 'train', sup)
        pred = model.get_prediction(batch, with_grad=False, to_cpu=True, min_size=True)
        items.append((batch, pred))
        gts.update({r['name']: T.ground_truth_ids(r) for r in raws})
        # the layout of the ARKitScenes loader: the scenes carry their positions, the batch the boxes
        for sc, r in zip(batch['scene'], raws):
            sc['positions'] = r['positions']
        batch['labels'] = [T.box_labels(r) for r in raws]
    if args.metric == 'arkit':
        return arkit(args, model, grid, items, loaded)
    t0 = time.time()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        res = param_search.scannet_param_search(model, items, gts, grid, matching=args.matching)
    dt = time.time() - t0
    ap_ = res['ap']
    settings = list(grid.settings())
    key = lambda st: tuple(-np.inf if np.isnan(v) else v for v in (ap_[st][1], ap_[st][0]))
    ranked = sorted(settings, key=lambda st: (tuple(-v for v in key(st)), st))
    print('checkpoint %s: %d settings (%s) over %d scenes in %.1f s, %d %s'
          % (loaded[2], len(settings), ' x '.join(str(n) for n in grid.shape), args.scenes, dt, res['n_evaluated'],
             'distinct record sets matched' if args.matching == 'host' else 'settings matched on the device'))
    print('cluster_th score_th mask_bin_th mask_nms_th |     AP   AP50   AP25')
    for st in ranked[:args.top or len(ranked)]:
        print('%10.3f %8.3f %11.3f %11.3f | %6.3f %6.3f %6.3f' % (tuple(grid.eval_ths(*st)) + tuple(ap_[st])))
    assert ranked[0] == res['best']
    print('best: eval_ths = %s' % ' '.join('%.3f' % v for v in res['best_ths']))
    if args.check:
        picks = [settings[i] for i in np.unique(np.linspace(0, len(settings) - 1, args.check).round().astype(int))]
        if res['best'] not in picks:
            picks[-1] = res['best']
        bad = 0
        for st in picks:
            model.cfg.eval_ths = grid.eval_ths(*st)
            results = {}
            for batch, pred in items:
                results.update(model.pred2mask(batch, pred, 'eval'))
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)
                avg, _ = eval_metric.compute_eval(results, gts)
            want = [avg['all_ap'], avg['all_ap_50%'], avg['all_ap_25%']]
            if args.matching == 'host':
                same = np.array_equal(ap_[st], want, equal_nan=True)
            else:
                bound = 4 * (3 * sum(int(r['mask'].shape[0]) for r in results.values()) + 1) * 2.0 ** -53 + 2.0 ** -50
                same = np.array_equal(np.isnan(ap_[st]), np.isnan(want)) and \
                    all(abs(a - b) <= bound for a, b in zip(ap_[st], want) if not np.isnan(b))
            bad += not same
            print('check %s: sweep %s  single-setting path %s  %s' % (grid.eval_ths(*st), ap_[st].tolist(), want, ('equal' if args.matching == 'host' else 'within the bound') if same else 'DIFFERENT'))
        if bad:
            raise SystemExit('%d of %d settings differ from the single-setting path' % (bad, len(picks)))
    return res


def arkit(args, model, grid, items, loaded):
    t0 = time.time()
    res = param_search.arkit_param_search(model, items, grid, oriented_boxes=True, iou_t=args.iou_t)
    dt = time.time() - t0
    m = res['map']
    settings = list(grid.settings())
    ranked = sorted(settings, key=lambda st: (np.inf if np.isnan(m[st]) else -m[st], st))
    print('checkpoint %s: %d settings (%s) over %d scenes in %.1f s, %d distinct record sets matched'
          % (loaded[2], len(settings), ' x '.join(str(n) for n in grid.shape), args.scenes, dt, res['n_evaluated']))
    print('cluster_th score_th mask_bin_th mask_nms_th |  mAP@%.2f' % args.iou_t)
    for st in ranked[:args.top or len(ranked)]:
        print('%10.3f %8.3f %11.3f %11.3f | %8.4f' % (tuple(grid.eval_ths(*st)) + (m[st],)))
    assert ranked[0] == res['best']
    print('best: eval_ths = %s' % ' '.join('%.3f' % v for v in res['best_ths']))
    if args.check:
        picks = [settings[i] for i in np.unique(np.linspace(0, len(settings) - 1, args.check).round().astype(int))]
        if res['best'] not in picks:
            picks[-1] = res['best']
        bad = 0
        for st in picks:
            model.cfg.eval_ths = grid.eval_ths(*st)
            results, scenes, labels = {}, [], []
            for batch, pred in items:
                results.update(model.pred2mask(batch, pred, 'eval'))
                scenes += batch['scene']
                labels += batch['labels']
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)
                want, _ = eval_detection.arkitscenes_eval(results, scenes, labels, oriented_boxes=True, iou_t=args.iou_t, verbose=False)
            same = np.array_equal(m[st], want, equal_nan=True)
            bad += not same
            print('check %s: sweep %r  single-setting path %r  %s' % (grid.eval_ths(*st), float(m[st]), float(want), 'equal' if same else 'DIFFERENT'))
        if bad:
            raise SystemExit('%d of %d settings differ from the single-setting path' % (bad, len(picks)))
    return res


def s3dis(args):
    import torch
    from box2mask_amd import eval_s3dis
    from bench_param_sweep import s3dis_room
    cfg = scannet_config(network_heads=['mlp_offsets', 'mlp_bounds', 'mlp_bb_scores', 'mlp_per_vox_semantics'])
    for axis in param_search.AXES:
        if getattr(args, axis + '_search') is not None:
            setattr(cfg, axis + '_search', getattr(args, axis + '_search'))
    grid = param_search.ThresholdGrid.from_cfg(cfg)
    ids = torch.arange(13).long()
    model = Model(cfg, torch.Tensor(np.arange(13)), ids, ids.clone(), (lambda s_: s_ > 2))
    model.eval()
    items = [s3dis_room(s_, args.voxels, cfg) for s_ in range(args.scenes)]
    for i, (b, _) in enumerate(items):
        b['scene'][0]['name'] = 'room%d' % i
    t0 = time.time()
    res = param_search.s3dis_param_search(model, items, grid, per_class=True)
    dt = time.time() - t0
    nc, ns, nb, _ = grid.shape
    settings = [(ci, si, bi) for ci in range(nc) for si in range(ns) for bi in range(nb)]
    with np.errstate(all='ignore'):
        f1 = 2.0 * res['mprec'] * res['mrec'] / (res['mprec'] + res['mrec'])
    f1 = np.where(np.isnan(f1), -np.inf, f1)
    ranked = sorted(settings, key=lambda st: (-f1[st], st))
    print('%d settings (%s; mask_nms_th has no effect) over %d rooms in %.1f s' % (len(settings), ' x '.join(str(n) for n in (nc, ns, nb)),
                                                                                 args.scenes, dt))
    print('cluster_th score_th mask_bin_th |  mPrec   mRec     F1')
    for st in ranked[:args.top or len(ranked)]:
        print('%10.3f %8.3f %11.3f | %6.3f %6.3f %6.3f' % (tuple(grid.eval_ths(*st, 0)[:3]) + (res['mprec'][st], res['mrec'][st], f1[st])))
    best = res.best()
    assert best == grid.eval_ths(*ranked[0], 0)
    print('best: eval_ths = %s' % ' '.join('%.3f' % v for v in best))
    if args.check:
        picks = [settings[i] for i in np.unique(np.linspace(0, len(settings) - 1, args.check).round().astype(int))]
        if ranked[0] not in picks:
            picks[-1] = ranked[0]
        bad = 0
        for st in picks:
            cfg.eval_ths = grid.eval_ths(*st, 0)
            counts = []
            for batch, pred in items:
                scene, labels = batch['scene'][0], batch['labels'][0]
                sem = torch.argmax(pred[cfg.mlp_per_vox_semantics], 1)[torch.as_tensor(np.asarray(batch['vox2point'][0])).long()]
                results = model.pred2mask(batch, {k: v.clone() for k, v in pred.items()}, 'eval')
                lab = eval_s3dis.room_labels(sem.cuda(), scene['positions'], scene['normals'], results[scene['name']]['mask'])
                counts.append(eval_s3dis.s3dis_counts(lab, labels))
            tp, fp, total = eval_s3dis.instance_counts(counts)
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)
                mprec, mrec, _, _ = eval_s3dis.s3dis_eval_from_counts(counts)
            same = np.array_equal(res['tp'][st], tp) and np.array_equal(res['fp'][st], fp) and np.array_equal(res['total_gt'], total) and \
                np.array_equal(res['mprec'][st], mprec, equal_nan=True) and np.array_equal(res['mrec'][st], mrec, equal_nan=True)
            bad += not same
            print('check %s: sweep tp %s fp %s  single-setting path tp %s fp %s  %s'
                  % (grid.eval_ths(*st, 0)[:3], res['tp'][st].tolist(), res['fp'][st].tolist(), tp.tolist(), fp.tolist(),
                     'equal' if same else 'DIFFERENT'))
        if bad:
            raise SystemExit('%d of %d settings differ from the single-setting path' % (bad, len(picks)))
    return res


if __name__ == '__main__':
    main()
