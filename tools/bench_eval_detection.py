"""Device time of the detection-metric kernels (b2m_mask_hulls, b2m_hull_box_iou) on ARKit-shaped synthetic scenes, beside the wall
time of a numpy / scipy restatement of the reference's path (one qhull call per mask, a Python Sutherland-Hodgman clip per pair)
on the same inputs on this host.

    python tools/bench_eval_detection.py [--points 1000000] [--masks 300] [--boxes 40] [--repeats 20] [--cpu-masks 60]

HIP events around warm calls, median of the repeats.  The hull scan's effective read rate is taken against the bytes it must touch:
k * words * 8 mask bytes + 16 bytes (x, y) per set bit.  One JSON line at the end.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from box2mask_amd import eval_detection as D          # noqa: E402


def make_case(n, k, g, seed=0):
    rng = np.random.default_rng(seed)
    side = np.sqrt(n / 800.0)                          # ~800 points per square metre of floor plan
    pos = np.stack([rng.uniform(0, side, n), rng.uniform(0, side, n), rng.uniform(0, 2.5, n)], 1)
    order = np.argsort(pos[:, 0], kind='stable')
    xs = pos[order, 0]
    masks = np.zeros((k, n), bool)
    centers = np.stack([rng.uniform(1, side - 1, k), rng.uniform(1, side - 1, k)], 1)
    radius = rng.uniform(0.3, 1.2, k)
    for r in range(k):
        lo, hi = np.searchsorted(xs, [centers[r, 0] - radius[r], centers[r, 0] + radius[r]])
        idx = order[lo:hi]
        masks[r, idx[np.abs(pos[idx, 1] - centers[r, 1]) < radius[r] * 0.8]] = True
    yaw = rng.uniform(-np.pi, np.pi, g)
    rot = np.stack([np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]]).T.reshape(-1) for a in yaw])
    labels = {'per_instance_bb_centers': np.concatenate([centers[:g] + rng.normal(0, 0.2, (g, 2)), np.full((g, 1), 1.25)], 1),
              'per_instance_bb_bounds': np.stack([radius[:g], radius[:g] * 0.8, np.full(g, 1.0)], 1),
              'per_instance_bb_rotations': rot, 'per_instance_semantics': np.full(g, 5)}
    pred = {'conf': rng.random(k).astype(np.float32), 'label_id': np.full(k, 5, np.int32), 'mask': masks}
    return pos, pred, labels


def timed(fn, repeats):
    fn(); fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def cpu_path(pos, pred, labels, rows):
    """evaluation.py:272-292 + box3d_iou restated: qhull per mask, clip + shoelace per same-class pair."""
    from scipy.spatial import ConvexHull
    c, b = labels['per_instance_bb_centers'], labels['per_instance_bb_bounds']
    signs = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]])
    t0 = time.perf_counter()
    hulls = []
    for r in rows:
        p = pos[pred['mask'][r]]
        hulls.append((p[ConvexHull(p[:, :2]).vertices, :2], p[:, 2].min(), p[:, 2].max()) if len(p) >= 50 else None)
    t1 = time.perf_counter()
    pairs = 0
    for h in hulls:
        if h is None:
            continue
        for i in range(len(c)):
            R = labels['per_instance_bb_rotations'][i].reshape(3, 3).T[:2, :2]
            rect = (signs * b[i, :2]) @ R.T + c[i, :2]
            poly = [tuple(q) for q in h[0]]
            for e in range(4):
                c1, c2 = rect[e - 1], rect[e]
                inside = lambda q: (c2[0] - c1[0]) * (q[1] - c1[1]) > (c2[1] - c1[1]) * (q[0] - c1[0])
                out, s = [], poly[-1] if poly else None
                for q in poly:
                    if inside(q) != inside(s):
                        dc, dp = (c1[0] - c2[0], c1[1] - c2[1]), (s[0] - q[0], s[1] - q[1])
                        n1, n2 = c1[0] * c2[1] - c1[1] * c2[0], s[0] * q[1] - s[1] * q[0]
                        n3 = 1.0 / (dc[0] * dp[1] - dc[1] * dp[0])
                        out.append(((n1 * dp[0] - n2 * dc[0]) * n3, (n1 * dp[1] - n2 * dc[1]) * n3))
                    if inside(q):
                        out.append(q)
                    s = q
                poly = out
                if not poly:
                    break
            pairs += 1
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, pairs


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=1_000_000)
    ap.add_argument('--masks', type=int, default=300)
    ap.add_argument('--boxes', type=int, default=40)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--cpu-masks', type=int, default=60, help='masks the host restatement is timed on (scaled to all of them)')
    args = ap.parse_args(argv)
    pos, pred, labels = make_case(args.points, args.masks, args.boxes)
    dev = torch.device('cuda', torch.cuda.current_device())
    bits, words, n = D.pack_masks(pred['mask'], dev)
    dpos = torch.from_numpy(pos).to(dev)
    out = D.hulls_from_bits(bits, words, n, dpos)
    assert not out['flags'].any().item()
    set_bits = int(out['count'].sum().item())
    hull_ms = timed(lambda: D.hulls_from_bits(bits, words, n, dpos), args.repeats)
    boxes = D.mask_boxes(pred, dpos)
    gt = D.gt_boxes(labels)
    k, g = args.masks, args.boxes
    iou = torch.zeros((k, g), dtype=torch.float64, device=dev)
    from box2mask_amd import _lib
    from box2mask_amd._lib import ptr
    iou_ms = timed(lambda: _lib.call('b2m_hull_box_iou', ptr(boxes['hull']), ptr(boxes['n_hull']), ptr(boxes['box6']), ptr(boxes['cls']),
                                     k, ptr(gt['boxes']), ptr(gt['cls']), g, ptr(iou)), args.repeats)
    must = k * words * 8 + 16 * set_bits
    rows = list(range(min(args.cpu_masks, k)))
    cpu_hull, cpu_iou, pairs = cpu_path(pos, pred, labels, rows)
    scale = k / len(rows)
    res = {'points': n, 'masks': k, 'boxes': g, 'set_bits': set_bits, 'largest_hull': int(boxes['n_hull'].max().item()),
           'mask_hulls_ms_median_min_max': hull_ms, 'hull_box_iou_ms_median_min_max': iou_ms,
           'hull_scan_bytes_needed': must, 'hull_scan_GBps_effective': must / (hull_ms[0] * 1e-3) / 1e9,
           'cpu_cores': os.cpu_count(), 'cpu_threads_used': 1,
           'cpu_hulls_s_scaled': cpu_hull * scale, 'cpu_pair_ious_s_scaled': cpu_iou * scale, 'cpu_pairs_timed': pairs,
           'repeats': args.repeats, 'includes': 'hulls_from_bits allocates its scratch inside the timed call'}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
