"""Device time of the S3DIS evaluation (b2m_dbscan per pass; room_labels + s3dis_counts as a whole) on a synthetic room of about a
million points, beside sklearn's DBSCAN and reference-shaped numpy loops on the same input on this host.

    python tools/bench_eval_s3dis.py [--voxels 400000] [--pts-per-m2 6250] [--proposals 100] [--repeats 10] [--no-cpu]

The room is synth.make_scene(points_only=True): floor, furniture boxes and four walls with normals.  Three of the walls are the
predicted wall class (about a quarter of the rows), the floor is predicted as floor, the furniture as classes 3 .. 12.  HIP events
around warm calls, median of the repeats; the passes of b2m_dbscan are taken from a kernel trace (torch.profiler) of one call.
A candidate pair is one (query row, row of the 27 surrounding cells) distance test: 3 d fp64 operations (d subtractions, d
multiply-adds).  The fp64 vector peak is half the FP32 vector peak of 157.3 TFLOPS.  One JSON line at the end.
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

from box2mask_amd import eval_s3dis as S, synth          # noqa: E402

FP64_VECTOR_PEAK = 157.3e12 / 2


def make_case(voxels, pts_per_m2, proposals, seed=0):
    raw = synth.make_scene(seed, target_voxels=voxels, pts_per_m2=pts_per_m2, points_only=True)
    pos, nrm = raw['positions'], raw['normals']
    inst = raw['labels']['seg2inst'][raw['segments']].astype(np.int64)
    cls = raw['labels']['per_instance_semantics'][inst]
    n_box = len(raw['labels']['unique_instances']) - 2
    sem = np.where(cls == 2, 1, 3 + inst % 10)                          # floor -> 1, furniture -> 3 .. 12
    wall = cls == 1
    sem[wall] = np.where(nrm[wall, 0] < 0, 0, 2)                         # three walls predicted as wall, one as ceiling
    rng = np.random.default_rng(seed)
    masks = np.zeros((proposals, len(pos)), bool)
    for r in range(proposals):
        idx = np.nonzero(inst == r % max(n_box, 1))[0]
        masks[r, idx[rng.random(len(idx)) < 0.7]] = True
    gt = {'semantics': sem.copy(), 'instances': inst}
    return pos, nrm, sem.astype(np.int64), masks, gt


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


def pass_group(name):
    """'pass1' .. 'pass3', 'sort', 'other' or None for a kernel name, mangled (db_pass_kernelILi6ELi2EEv...) or demangled
    (db_pass_kernel<6, 2>(...))."""
    import re
    m = re.search(r'db_pass_kernelILi\d+ELi(\d)EE', name) or re.search(r'db_pass_kernel<\s*\d+\s*,\s*(\d)\s*>', name)
    if m:
        return 'pass' + m.group(1)
    if re.search(r'\brs_(hist|scan|scatter)_kernel', name):
        return 'sort'
    if re.search(r'\bdb_\w+_kernel', name):
        return 'other'
    return None


def pass_times(fn):
    """{kernel group: ms} of one call, from a kernel trace of torch.profiler.  Raises if the trace does not hold the three passes."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.events():
        key = pass_group(e.name)
        us = getattr(e, 'device_time', None) or getattr(e, 'cuda_time', 0) or 0
        if key is not None and us > 0:
            out[key] = out.get(key, 0.0) + us / 1e3
    missing = [k for k in ('pass1', 'pass2', 'pass3') if k not in out]
    if missing:
        raise RuntimeError('the kernel trace holds no %s of b2m_dbscan (kernels seen: %s)' % (', '.join(missing), sorted(out)))
    return out


def candidate_pairs(x, eps):
    """Rows each query row is tested against when no pass stops early: the population of its 27 surrounding cells."""
    edge = eps * (1.0 + 1.0 / 1048576.0)
    c = np.floor((x[:, :3] - x[:, :3].min(0)) / edge).astype(np.int64) + 1
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    uk, cnt = np.unique(key, return_counts=True)
    total = np.zeros(len(x), np.int64)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                k2 = key + (dx << 42) + (dy << 21) + dz
                at = np.searchsorted(uk, k2)
                at[at >= len(uk)] = 0
                total += np.where(uk[at] == k2, cnt[at], 0)
    return total


def cpu_loops(pred, gt):
    """s3dis_util.py:216-221 and :244-299 in their own shape: a Python loop over the points, one boolean & and | per pair."""
    t0 = time.perf_counter()
    g_cls, p_cls, tp = np.zeros(13), np.zeros(13), np.zeros(13)
    ps, gs = pred['semantics'], gt['semantics']
    for j in range(gs.shape[0]):
        g, p = int(gs[j]), int(ps[j])
        g_cls[g] += 1; p_cls[p] += 1; tp[g] += int(g == p)
    t1 = time.perf_counter()
    pin, gin = [[] for _ in range(13)], [[] for _ in range(13)]
    for lab, sem, dst, skip in ((pred['instances'], ps, pin, True), (gt['instances'], gs, gin, False)):
        for g in np.unique(lab):
            if skip and g == -1:
                continue
            m = lab == g
            dst[int(np.bincount(sem[m], minlength=13).argmax())].append(m)
    pairs = 0
    for c in range(13):
        for a in gin[c]:
            for b in pin[c]:
                float(np.sum(a & b)) / np.sum(a | b); pairs += 1
        for b in pin[c]:
            for a in gin[c]:
                float(np.sum(a & b)) / np.sum(a | b); pairs += 1
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, pairs


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--voxels', type=int, default=400_000)
    ap.add_argument('--pts-per-m2', type=float, default=6250.0)
    ap.add_argument('--proposals', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--no-cpu', action='store_true')
    args = ap.parse_args(argv)
    pos, nrm, sem, masks, gt = make_case(args.voxels, args.pts_per_m2, args.proposals)
    dev = torch.device('cuda', torch.cuda.current_device())
    n = len(pos)
    wall = sem == 2
    feats = np.concatenate([pos[wall], nrm[wall] * 2], 1)
    dfeats = torch.from_numpy(feats).to(dev)
    dpos, dnrm, dsem, dmasks = (torch.from_numpy(a).to(dev) for a in (pos, nrm, sem, masks))
    dgt = {k: torch.from_numpy(v).to(dev) for k, v in gt.items()}
    labels, count = S.dbscan(dfeats, S.WALL_EPS, S.WALL_MIN_SAMPLES, return_count=True)
    labels = labels.cpu().numpy()
    db_ms = timed(lambda: S.dbscan(dfeats, S.WALL_EPS, S.WALL_MIN_SAMPLES), args.repeats)
    try:
        passes, passes_error = pass_times(lambda: S.dbscan(dfeats, S.WALL_EPS, S.WALL_MIN_SAMPLES)), None
    except Exception as e:                                               # noqa: BLE001  (reported in the line, exit status 2)
        passes, passes_error = None, repr(e)

    def whole():
        out = S.room_labels(dsem, dpos, dnrm, dmasks)
        return S.s3dis_counts(out, dgt)

    whole_ms = timed(whole, args.repeats)
    cand = candidate_pairs(feats, S.WALL_EPS)
    d = feats.shape[1]
    res = {'points': n, 'wall_rows': int(wall.sum()), 'wall_fraction': float(wall.mean()), 'proposals': args.proposals,
           'clusters': int(count.item()), 'noise_rows': int((labels < 0).sum()),
           'dbscan_ms_median_min_max': db_ms, 'dbscan_kernel_ms': passes,
           'room_labels_plus_counts_ms_median_min_max': whole_ms,
           'candidate_pairs_per_full_pass': int(cand.sum()), 'candidates_per_row_mean': float(cand.mean()),
           'repeats': args.repeats, 'includes': 'dbscan() allocates its workspace inside the timed call; room_labels + s3dis_counts '
                                                'include their host reads (cluster count, instance maximum, the count tables)'}
    res['dbscan_kernel_ms_error'] = passes_error
    if passes is not None:
        rate = float(cand.sum()) / (passes['pass2'] * 1e-3)               # every row is core here: pass 2 tests every candidate
        res.update(pass2_pairs_per_s=rate, pass2_fraction_of_fp64_vector_peak=rate * 3 * d / FP64_VECTOR_PEAK)
    if not args.no_cpu:
        res.update(cpu_cores=os.cpu_count())
        try:
            from sklearn.cluster import DBSCAN
            t0 = time.perf_counter()
            ref = DBSCAN(eps=S.WALL_EPS, min_samples=S.WALL_MIN_SAMPLES, n_jobs=16).fit(feats).labels_
            res.update(sklearn_dbscan_s=time.perf_counter() - t0, sklearn_n_jobs=16, labels_equal_sklearn=bool(np.array_equal(ref, labels)))
        except ImportError:
            res.update(sklearn_dbscan_s=None)
        out = S.room_labels(dsem, dpos, dnrm, dmasks)
        pred = {k: v.cpu().numpy().astype(np.int64) for k, v in out.items()}
        point_s, pair_s, pairs = cpu_loops(pred, gt)
        res.update(cpu_point_loop_s=point_s, cpu_pair_loops_s=pair_s, cpu_pairs=pairs)
    print(json.dumps(res))
    return 2 if passes_error else 0


if __name__ == '__main__':
    sys.exit(main())
