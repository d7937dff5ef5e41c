"""numpy restatements shared by tests/test_eval_s3dis.py and tests/test_gpu_eval_s3dis.py: the DBSCAN labelling rule of
include/b2m.h (brute force, O(n^2)), the margin condition of the fixture's DBSCAN inputs, and the count tables of
eval_s3dis.s3dis_counts."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'eval_s3dis.npz')
NORMALS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
GRID = 1.0 / 128.0                                   # positions of the rooms: int16 steps of 1/128 m


def sq_dists(a, b):
    """sum_j (a_j - b_j)^2 in fp64, j ascending: (len(a), len(b))."""
    d2 = np.zeros((len(a), len(b)))
    for j in range(a.shape[1]):
        df = a[:, j, None] - b[None, :, j]
        d2 += df * df
    return d2


def dbscan_rule(x, eps, min_samples, chunk=1024):
    """The labelling rule: neighbours by the fp64 squared distance (self included), core rows, components of the core rows numbered
    by their smallest row, every other row the lowest number among its core neighbours or -1.  Returns (labels, core, two) -- two:
    rows that are not core and have core neighbours in more than one cluster."""
    x = np.asarray(x, np.float64)
    n = len(x)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, bool), np.zeros(0, bool)
    eps2 = eps * eps
    nbrs = []
    for s in range(0, n, chunk):
        m = sq_dists(x[s:s + chunk], x) <= eps2
        nbrs.extend(np.nonzero(r)[0] for r in m)
    core = np.array([len(v) >= min_samples for v in nbrs])
    parent = np.arange(n)

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for i in np.nonzero(core)[0]:
        for j in nbrs[i]:
            if core[j] and j < i:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    roots = np.array([find(i) if core[i] else -1 for i in range(n)])
    order = np.unique(roots[roots >= 0])             # ascending smallest core row
    number = {r: k for k, r in enumerate(order)}
    labels = np.full(n, -1, np.int32)
    two = np.zeros(n, bool)
    for i in range(n):
        if core[i]:
            labels[i] = number[roots[i]]
        else:
            c = {number[roots[j]] for j in nbrs[i] if core[j]}
            if c:
                labels[i] = min(c)
            two[i] = len(c) > 1
    return labels, core, two


def margin(x, eps):
    """min |d^2 - eps^2| over the pairs whose distance over the first three columns is at most 2 eps."""
    from scipy.spatial import cKDTree
    x = np.asarray(x, np.float64)
    pairs = cKDTree(x[:, :3]).query_pairs(2 * eps, output_type='ndarray')
    if len(pairs) == 0:
        return np.inf
    best = np.inf
    for s in range(0, len(pairs), 1 << 20):
        p = pairs[s:s + (1 << 20)]
        d2 = np.zeros(len(p))
        for j in range(x.shape[1]):
            df = x[p[:, 0], j] - x[p[:, 1], j]
            d2 += df * df
        best = min(best, float(np.abs(d2 - eps * eps).min()))
    return best


def room(z, r):
    """Arrays of room r of the fixture: positions / normals (fp64), predicted and true labels, the (K, n) bool masks."""
    n = int(z['r%d_n' % r])
    masks = np.unpackbits(z['r%d_masks' % r], axis=1, count=n).astype(bool)
    return {'n': n, 'positions': z['r%d_grid' % r].astype(np.float64) * GRID, 'normals': NORMALS[z['r%d_normal' % r]],
            'pred_semantics': z['r%d_pred_semantics' % r].astype(np.int64), 'masks': masks,
            'gt': {'semantics': z['r%d_gt_semantics' % r].astype(np.int64), 'instances': z['r%d_gt_instances' % r].astype(np.int64)},
            'final': {'semantics': z['r%d_final_semantics' % r].astype(np.int64),
                      'instances': z['r%d_final_instances' % r].astype(np.int64)},
            'background': z['r%d_background' % r].astype(np.int64), 'proposal_semantics': z['r%d_proposal_semantics' % r].astype(np.int64)}


def wall_features(rm):
    w = rm['pred_semantics'] == 2
    return np.concatenate([rm['positions'][w], rm['normals'][w] * 2], 1)


def counts_numpy(pred, gt, n_class=13):
    """The tables of eval_s3dis.s3dis_counts from per-point labels, with numpy."""
    pi, ps = np.asarray(pred['instances'], np.int64), np.asarray(pred['semantics'], np.int64)
    gi, gs = np.asarray(gt['instances'], np.int64), np.asarray(gt['semantics'], np.int64)
    pv = np.unique(pi); pv = pv[pv != -1]
    gv = np.unique(gi)
    inter = np.array([[np.count_nonzero((pi == p) & (gi == g)) for g in gv] for p in pv], np.int64).reshape(len(pv), len(gv))
    pcls = np.array([np.bincount(ps[pi == p], minlength=n_class).argmax() for p in pv], np.int64)
    gcls = np.array([np.bincount(gs[gi == g], minlength=n_class).argmax() for g in gv], np.int64)
    cc = np.zeros((n_class, n_class), np.int64)
    np.add.at(cc, (ps, gs), 1)
    return {'inter': inter, 'pred_class': pcls, 'gt_class': gcls, 'pred_size': np.array([np.count_nonzero(pi == p) for p in pv], np.int64),
            'gt_size': np.array([np.count_nonzero(gi == g) for g in gv], np.int64), 'cc': cc, 'n': len(pi)}


def details_numpy(preds, gts, n_class=13):
    """oAcc, per-class IoU, MUCov, MWCov restated from the boolean masks (s3dis_util.py:212-270, 302-306, 333-336)."""
    true = seen = 0
    tpc, pc, gc = np.zeros(n_class), np.zeros(n_class), np.zeros(n_class)
    cov = [[] for _ in range(n_class)]
    wcov = [[] for _ in range(n_class)]
    for pred, gt in zip(preds, gts):
        pi, ps = np.asarray(pred['instances']), np.asarray(pred['semantics'])
        gi, gs = np.asarray(gt['instances']), np.asarray(gt['semantics'])
        true += int(np.sum(ps == gs)); seen += len(ps)
        for c in range(n_class):
            gc[c] += np.sum(gs == c); pc[c] += np.sum(ps == c); tpc[c] += np.sum((gs == c) & (ps == c))
        pin = [[] for _ in range(n_class)]
        for g in np.unique(pi):
            if g != -1:
                m = pi == g
                pin[np.bincount(ps[m], minlength=n_class).argmax()].append(m)
        gin = [[] for _ in range(n_class)]
        for g in np.unique(gi):
            m = gi == g
            gin[np.bincount(gs[m], minlength=n_class).argmax()].append(m)
        for c in range(n_class):
            if not gin[c]:
                continue
            s = w = 0.0
            tot = 0
            for g in gin[c]:
                best = max([np.sum(p & g) / np.sum(p | g) for p in pin[c]] + [0.0])
                s += best; w += best * np.sum(g); tot += np.sum(g)
            cov[c].append(s / len(gin[c])); wcov[c].append(w / tot)
    with np.errstate(all='ignore'):
        iou = tpc / (gc + pc - tpc)
    mean = lambda v: np.mean(v) if len(v) else np.nan
    return {'oAcc': true / seen, 'iou': iou, 'mIoU': np.mean(iou), 'MUCov': np.array([mean(v) for v in cov]),
            'MWCov': np.array([mean(v) for v in wcov])}
