#!/usr/bin/env python
"""The loss region of a training step -- from the heads' outputs to their gradients -- on the fused route and on the torch
route (B2M_FUSED_LOSS=0), on the batch of `bench.py --workload s3dis` (the same four synthetic rooms: 1 528 404 voxel rows,
11 122 segment rows, 13 classes; its locations, boxes, foreground flags and labels), for three head sets: the S3DIS heads (offsets, bounds, scores, per-voxel semantics), the same with use_bb_iou_loss, and
the same with the centre-score head.

The network is replaced by fixed head outputs (leaves), so the region is Model.compute_loss_detection's loss terms plus
optimization_loss.backward() (the gradients' scaling launch included).  HIP events bracket it on the device: the first is
recorded where the network would return, the second after backward.  The host clock runs over the same span with the device
idle at its start: what the host spends enqueueing (and waiting in, where a term reads a value back).  The two routes alternate
inside one process, `--reps` times each after `--warmup`; medians and the range are reported.

`--step-bench` adds the step time of `bench.py --workload s3dis --steps 5 --warmup 2` in this tree and, with `--parent-tree DIR`
(a built checkout of the parent commit), in that one, alternating, each run a fresh child process.

Prints a markdown report (profiles/loss_heads_bench.md is one).  Needs a GPU; there is no CPU path.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENE_VOXELS = [250_000, 400_000, 600_000, 350_000]         # bench.py --workload s3dis
HEAD_SETS = [
    ('s3dis heads', dict()),
    ('s3dis heads + use_bb_iou_loss', dict(use_bb_iou_loss=True)),
    ('s3dis heads + centre head', dict(centre=True)),
]


def loss_region(args):
    import numpy as np
    import torch
    from box2mask_amd.config import scannet_config
    from box2mask_amd.model import Model
    dev = 'cuda'
    from box2mask_amd import synth
    C = 13
    g = torch.Generator().manual_seed(0)
    valid = torch.Tensor(np.arange(C))
    id2idx = torch.arange(41).long() % C
    tables = (valid, id2idx, id2idx.clone(), (lambda s_: s_ > 2))
    # the batch bench.make_workload builds for --workload s3dis, rank 0
    full = synth.collate([synth.make_scene(i, target_voxels=tv) for i, tv in enumerate(SCENE_VOXELS)])
    N, S = full['vox_coords'].shape[0], full['input_location'].shape[0]
    gt_off, gt_bnd = full['gt_bb_offsets'].float(), full['gt_bb_bounds'].float()
    batch = {'input_location': full['input_location'], 'gt_bb_offsets': gt_off, 'gt_bb_bounds': gt_bnd,
             'gt_semantics': full['gt_semantics'] % C, 'fg_instances': full['fg_instances'],
             'gt_per_vox_semantics': torch.from_numpy(np.random.default_rng(0).integers(0, C, N)), 'pooling_ids': torch.arange(4)}
    batch = {k: v.to(dev) for k, v in batch.items()}
    batch['vox_features'] = torch.zeros(4, 6)
    batch['vox_coords'] = torch.tensor([[0, i, 0, 0] for i in range(4)], dtype=torch.int32)
    base = {'mlp_offsets': gt_off + torch.randn(S, 3, generator=g) * 0.15, 'mlp_bounds': gt_bnd + torch.randn(S, 3, generator=g) * 0.1,
            'mlp_bb_scores': torch.randn(S, 1, generator=g), 'mlp_per_vox_semantics': torch.randn(N, C, generator=g) * 3,
            'mlp_center_scores': torch.rand(S, 1, generator=g)}

    class H:
        def __init__(self, F): self.F = F
    rows = []
    for name, opt in HEAD_SETS:
        heads = ['mlp_offsets', 'mlp_bounds', 'mlp_bb_scores', 'mlp_per_vox_semantics'] + (['mlp_center_scores'] if opt.get('centre') else [])
        cfg = scannet_config(batch_size=4, loss_weight_bb_scores=3.0, network_heads=heads,
                             use_bb_iou_loss=bool(opt.get('use_bb_iou_loss')))
        model = Model(cfg, *tables)
        pred = {h: base[h].to(dev).requires_grad_(True) for h in heads}
        mark = [None]

        def net(sin, ids, n=None):
            mark[0] = torch.cuda.Event(enable_timing=True)
            mark[0].record()
            return {h: H(v) for h, v in pred.items()}
        model.detection_model = net
        times = {'fused': [], 'torch': []}
        total = {}
        for it in range(args.warmup + args.reps):
            for route in ('torch', 'fused'):
                os.environ['B2M_FUSED_LOSS'] = '1' if route == 'fused' else '0'
                for p in pred.values():
                    p.grad = None
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                losses, _ = model.compute_loss_detection(batch, 150)
                losses['optimization_loss'].backward()
                t1 = time.perf_counter()
                end = torch.cuda.Event(enable_timing=True)
                end.record()
                torch.cuda.synchronize()
                if it >= args.warmup:
                    times[route].append((mark[0].elapsed_time(end), (t1 - t0) * 1e3))
                total[route] = float(losses['optimization_loss'].detach())
        os.environ['B2M_FUSED_LOSS'] = '1'
        assert abs(total['fused'] - total['torch']) <= 1e-4 * abs(total['torch']), total      # faster and different is not faster
        for route in ('torch', 'fused'):
            dv, hs = [t[0] for t in times[route]], [t[1] for t in times[route]]
            rows.append((name, route, statistics.median(dv), min(dv), max(dv), statistics.median(hs), min(hs), max(hs), total[route]))
    return rows, N, S


def step_bench(tree):
    """ms per step of bench.py --workload s3dis --steps 5 --warmup 2 in `tree` (a fresh child process)."""
    out = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--workload', 's3dis', '--steps', '5', '--warmup', '2'],
                         cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, check=True).stdout.decode()
    line = [l for l in out.splitlines() if l.startswith('{')][-1]
    return float(json.loads(line)['ms_per_step'])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--step-bench', action='store_true')
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--step-runs', type=int, default=2)
    args = ap.parse_args()
    rows, N, S = loss_region(args)
    print('## Loss region, %d voxel rows x 13 classes, %d segment rows (%d alternating repetitions after %d warm-up)\n'
          % (N, S, args.reps, args.warmup))
    print('| head set | route | device ms: median (min .. max) | host ms: median (min .. max) | optimization_loss |')
    print('|---|---|---|---|---|')
    for n, r, d, d0, d1, h, h0, h1, tot in rows:
        print('| %s | %s | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) | %.6f |' % (n, r, d, d0, d1, h, h0, h1, tot))
    bad = [n for i, (n, r, d, *_) in enumerate(rows) if r == 'fused' and d > rows[i - 1][2]]
    print('\nfused device time above the torch route\'s: %s' % (', '.join(bad) if bad else 'in no head set'))
    if args.step_bench:
        print('\n## Step time, bench.py --workload s3dis --steps 5 --warmup 2 (ms per step, one fresh process per run)\n')
        trees = [('this commit', ROOT)] + ([('parent', os.path.abspath(args.parent_tree))] if args.parent_tree else [])
        res = {n: [] for n, _ in trees}
        for _ in range(args.step_runs):
            for n, t in trees:
                res[n].append(step_bench(t))
                print('<!-- %s: %.2f -->' % (n, res[n][-1]), flush=True)
        print('| tree | runs | median |')
        print('|---|---|---|')
        for n, _ in trees:
            print('| %s | %s | %.2f |' % (n, ', '.join('%.2f' % v for v in res[n]), statistics.median(res[n])))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
