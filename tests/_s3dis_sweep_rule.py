"""The S3DIS threshold sweep as a rule over flat arrays (profiles/s3dis_sweep_rule.md): plain numpy, no torch, no device.

"shared stage + prefix restriction + tail": the proposals of the SMALLEST score_th of a (cluster_th, mask_bin_th) stage are merged
once (``paint``: evaluation.py:177-193); score setting s keeps the first k_s proposals, and its labels are that painting restricted
to the owners below k_s (``labels``), scored per predicted instance (``score``: s3dis_util.py:224-299).  ``tail`` is what
b2m_s3dis_prefix_tail computes; ``MISTAKES`` are deliberate errors, each of which tests/test_s3dis_sweep_rule.py shows to fail."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 's3dis_sweep.npz')
NUM_CLASSES = 13
SEM_MIN, KEEP_RATIO, MIN_POINTS = 3, 0.6, 200
GRID = 1.0 / 128.0
NORMALS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)

MISTAKES = ('paint_after_overwrite', 'max_id_full', 'small_before_overwrite', 'small_at_eval', 'vote_predicted', 'iou_gt',
            'ceiling_kept', 'prop_sem_after_paint')
ACCEPTED, REJ_CLASS, REJ_RATIO, REJ_POINTS = 0, 1, 2, 3


def _vote(classes):
    """np.bincount(...).argmax(): the lowest class on ties; 0 for no point (the reference raises there)."""
    return int(np.bincount(classes, minlength=1).argmax()) if len(classes) else 0


def paint(masks, sem, sem_min=SEM_MIN, ratio=KEEP_RATIO, min_points=MIN_POINTS, mistake=None):
    """masks (K, n) bool in score order, sem (n) the predicted classes: (owner (n) int32 = the row that took the point or -1,
    prop_sem (K) int32, fate (K) one of ACCEPTED / REJ_*).  Row i reads the state rows before i left: prefix-closed."""
    masks = np.asarray(masks, bool).reshape(len(masks), len(sem))
    sem = np.asarray(sem, np.int64)
    owner = np.full(len(sem), -1, np.int32)
    cur = sem.copy()
    prop_sem = np.zeros(len(masks), np.int32)
    fate = np.zeros(len(masks), np.int32)
    for i, m in enumerate(masks):
        prop_sem[i] = _vote((cur if mistake == 'prop_sem_after_paint' else sem)[m])
        o = int(m.sum())
        left = m & (owner < 0)
        f = int(left.sum())
        with np.errstate(all='ignore'):
            low = np.float64(1.0 * f) / np.float64(o) < ratio
        if prop_sem[i] < sem_min:
            fate[i] = REJ_CLASS
        elif low:
            fate[i] = REJ_RATIO
        elif f < min_points:
            fate[i] = REJ_POINTS
        else:
            owner[left] = i
            cur[left] = prop_sem[i]
    return owner, prop_sem, fate


def _drop_small(inst, sem, min_points):
    """evaluation.py:200-210: per class, the instances with fewer than min_points points of that class lose those points."""
    inst = inst.copy()
    ok = (inst >= 0) & (sem >= 0) & (sem < NUM_CLASSES)
    if ok.any():
        key = inst[ok].astype(np.int64) * NUM_CLASSES + sem[ok]
        cnt = np.bincount(key)
        sel = np.nonzero(ok)[0]
        inst[sel[cnt[key] < min_points]] = -1
    return inst


def labels(owner, prop_sem, bg, sem, k_s, index=None, min_points=MIN_POINTS, mistake=None):
    """(instances, semantics) int32 of ONE setting at the evaluation points, as the reference leaves ``pred_label``."""
    owner, bg, sem = np.asarray(owner, np.int64), np.asarray(bg, np.int64), np.asarray(sem, np.int64)
    prop_sem = np.asarray(prop_sem, np.int64)
    painted = (owner >= 0) & (owner < k_s)
    inst = np.where(painted, owner + 1, -1)
    cls = np.where(painted, prop_sem[np.clip(owner, 0, max(len(prop_sem) - 1, 0))] if len(prop_sem) else sem, sem)
    if mistake == 'max_id_full':
        max_id = int(owner.max()) + 1 if (owner >= 0).any() else -1
    else:
        max_id = int(inst.max()) if len(inst) else -1
    if mistake == 'ceiling_kept':
        max_id = max(max_id, 0)
    if mistake == 'small_before_overwrite':
        inst = _drop_small(inst, cls, min_points)
    over = (bg > 0) & (bg + max_id > 0)
    if mistake == 'paint_after_overwrite':                                 # the restriction reaches only what the background left
        cls = np.where((owner >= 0) & over, prop_sem[np.clip(owner, 0, max(len(prop_sem) - 1, 0))] if len(prop_sem) else sem, cls)
    inst = np.where(over, bg + max_id, inst)
    if index is not None and mistake == 'small_at_eval':
        index = np.asarray(index, np.int64)
        return _drop_small(inst[index], cls[index], min_points).astype(np.int32), cls[index].astype(np.int32)
    if mistake != 'small_before_overwrite':
        inst = _drop_small(inst, cls, min_points)
    if index is not None:
        index = np.asarray(index, np.int64)
        inst, cls = inst[index], cls[index]
    return inst.astype(np.int32), cls.astype(np.int32)


def gt_tables(gt_ins, gt_sem):
    """Dense ground-truth index per point (ascending ids, np.unique) and the class of every instance (most frequent, lowest on ties)."""
    ids, gi = np.unique(np.asarray(gt_ins), return_inverse=True)
    gi = gi.reshape(-1).astype(np.int32)
    gt_sem = np.asarray(gt_sem, np.int64)
    gt_class = np.array([_vote(gt_sem[gi == g]) for g in range(len(ids))], np.int32)
    return gi, gt_class


def score(inst, sem, gi, gt_class, pred_sem=None, mistake=None):
    """(tp (13), fp (13)) int64 of one room and setting: per predicted instance (ascending id, -1 left out) its class and whether a
    ground-truth instance of that class has inter / union >= 0.5 -- the reference's own float division."""
    inst, sem, gi = np.asarray(inst, np.int64), np.asarray(sem, np.int64), np.asarray(gi, np.int64)
    vote_from = np.asarray(pred_sem, np.int64) if mistake == 'vote_predicted' else sem
    tp, fp = np.zeros(NUM_CLASSES, np.int64), np.zeros(NUM_CLASSES, np.int64)
    gsize = np.bincount(gi[gi >= 0], minlength=len(gt_class))
    for u in np.unique(inst):
        if u == -1:
            continue
        m = inst == u
        c = _vote(vote_from[m])
        inter = np.bincount(gi[m & (gi >= 0)], minlength=len(gt_class))
        ovmax = -1.0
        for g in np.nonzero(np.asarray(gt_class) == c)[0]:
            iou = float(inter[g]) / (int(m.sum()) + int(gsize[g]) - int(inter[g]))
            ovmax = max(ovmax, iou)
        hit = ovmax > 0.5 if mistake == 'iou_gt' else ovmax >= 0.5
        (tp if hit else fp)[c] += 1
    return tp, fp


def tail(owner, prop_sem, bg, sem, ks, gi, gt_class, index=None, min_points=MIN_POINTS, mistake=None):
    """What b2m_s3dis_prefix_tail adds to its tables: (tp (S, 13), fp (S, 13)) int64 for the prefix lengths ks."""
    tp, fp = np.zeros((len(ks), NUM_CLASSES), np.int64), np.zeros((len(ks), NUM_CLASSES), np.int64)
    pred_eval = np.asarray(sem)[index] if index is not None else np.asarray(sem)
    for s, k_s in enumerate(ks):
        inst, cls = labels(owner, prop_sem, bg, sem, int(k_s), index, min_points, mistake)
        tp[s], fp[s] = score(inst, cls, gi, gt_class, pred_eval, mistake)
    return tp, fp


def metric(tp, fp, total_gt):
    """s3dis_util.py:308-320 and :338: (mPrec, mRec, precision (13), recall (13)); 0 / 0 is NaN, as numpy leaves it."""
    precision, recall = np.zeros(NUM_CLASSES), np.zeros(NUM_CLASSES)
    with np.errstate(all='ignore'):
        for c in range(NUM_CLASSES):
            t, f = np.float64(tp[c]), np.float64(fp[c])
            recall[c] = t / np.float64(total_gt[c])
            precision[c] = t / (t + f)
        return np.mean(precision), np.mean(recall), precision, recall


def same_partition(a, b):
    """Two instance columns label the same partition (-1 = unlabelled in both)."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if a.shape != b.shape or not np.array_equal(a < 0, b < 0):
        return False
    pairs = np.unique(np.stack([a, b], 1)[a >= 0], axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) and len(np.unique(pairs[:, 1])) == len(pairs)


# ------------------------------------------------------------------ the fixture
def load(path=GOLD):
    """tests/golden/s3dis_sweep.npz as {'grid': four arrays, 'rooms': [...], 'settings': [(ci, si, bi)], 'full': {...}} (see
    tools/gen_golden_s3dis_sweep.py for what each array is)."""
    z = np.load(path)
    out = {'z': z, 'grid': [z['cluster_th'], z['score_th'], z['mask_bin_th'], z['mask_nms_th']], 'rooms': []}
    nc, ns, nb = (len(out['grid'][a]) for a in range(3))
    out['settings'] = [(ci, si, bi) for ci in range(nc) for si in range(ns) for bi in range(nb)]
    for r in range(int(z['n_rooms'])):
        p = 'r%d_' % r
        v2p = z[p + 'vox2point'].astype(np.int64)
        seg_of_vox = z[p + 'vox_segments'].astype(np.int64)
        rm = dict(name='room%d' % r, n=len(v2p), positions=z[p + 'grid'].astype(np.float64) * GRID, normals=NORMALS[z[p + 'normal']],
                  gt_sem=z[p + 'gt_semantics'].astype(np.int64), gt_ins=z[p + 'gt_instances'].astype(np.int64), vox2point=v2p,
                  vox_segments=seg_of_vox, vox_pred=z[p + 'vox_pred'].astype(np.int64), seg_location=z[p + 'seg_location'],
                  seg_offsets=z[p + 'seg_offsets'], seg_bounds=z[p + 'seg_bounds'], seg_logits=z[p + 'seg_logits'],
                  background=z[p + 'background'].astype(np.int64))
        rm['sem'] = rm['vox_pred'][v2p]
        rm['seg_of_point'] = seg_of_vox[v2p]
        n_seg = len(rm['seg_location'])
        rm['stage_masks'] = {}
        for ci in range(nc):
            for bi in range(nb):
                packed = z[p + 'c%d_b%d_segmask' % (ci, bi)]
                seg = np.unpackbits(packed, axis=1)[:, :n_seg].astype(bool) if len(packed) else np.zeros((0, n_seg), bool)
                rm['stage_masks'][(ci, bi)] = seg[:, rm['seg_of_point']]
        rm['k'] = z[p + 'k'].astype(np.int64)                              # (nc, ns, nb): masks the reference kept
        out['rooms'].append(rm)
    return out


def room_batch(rm):
    """One golden room as the one-room batch of the S3DIS flow and its head outputs (torch tensors on the host)."""
    import torch
    batch = {'scene': [{'name': rm['name'], 'positions': rm['positions'], 'normals': rm['normals']}],
             'labels': [{'semantics': rm['gt_sem'], 'instances': rm['gt_ins']}],
             'input_location': torch.from_numpy(rm['seg_location']), 'batch_ids': torch.zeros(len(rm['seg_location']), dtype=torch.long),
             'vox_segments': [rm['vox_segments']], 'seg2vox': [rm['vox_segments']], 'vox2point': [rm['vox2point']]}
    pred = {'mlp_offsets': torch.from_numpy(rm['seg_offsets']), 'mlp_bounds': torch.from_numpy(rm['seg_bounds']),
            'mlp_bb_scores': torch.from_numpy(rm['seg_logits']),
            'mlp_per_vox_semantics': torch.from_numpy(np.eye(NUM_CLASSES, dtype=np.float32)[rm['vox_pred']])}
    return batch, pred


# ------------------------------------------------------------------ cases for the kernel
def kernel_case(n, k_rows, n_set, n_gt, seed, index=None, owners=True, min_points=3, n_bg=3):
    """Random flat inputs of b2m_s3dis_prefix_tail with a small min_points, so that rooms of a few points exercise every rule:
    owners in runs, background ids 1 .. n_bg (and -1, 0), prefixes from k_rows down to 0."""
    rng = np.random.default_rng(seed)
    runs = lambda lo, hi: np.sort(rng.integers(lo, hi, n)).astype(np.int32)       # a few long runs: pairs above and below min_points
    owner = runs(-1, k_rows) if (owners and k_rows) else np.full(n, -1, np.int32)
    if owners and k_rows and n:
        owner[rng.random(n) < 0.2] = -1
    prop_sem = rng.integers(3, 6, k_rows).astype(np.int32)
    bg = np.where(rng.random(n) < 0.4, runs(-1, n_bg + 1)[::-1], 0).astype(np.int32)
    sem = np.where(bg > 0, (bg - 1) % 3, runs(0, 3))
    sem = np.where(rng.random(n) < 0.15, rng.integers(0, NUM_CLASSES, n), sem).astype(np.int32)
    ks = np.sort(rng.integers(0, k_rows + 1, n_set))[::-1].astype(np.int32)
    ks[0] = k_rows
    if n_set > 1:
        ks[-1] = 0
    # the ground truth follows what the full list predicts, with a tenth of the points elsewhere: true and false positives both occur
    truth = np.where(bg > 0, k_rows + bg, owner + 1).astype(np.int64)
    truth = np.where(rng.random(n) < 0.1, rng.integers(0, k_rows + n_bg + 1, n), truth) % n_gt
    full_class = np.concatenate([[0], prop_sem, (np.arange(n_bg) % 3)]).astype(np.int32)
    gt_class = np.zeros(n_gt, np.int32)
    gt_class[np.arange(len(full_class))[::-1] % n_gt] = full_class[::-1]
    if index == 'gather':
        idx = rng.integers(0, max(n, 1), 2 * n + 3).astype(np.int64)      # repeats; some sampled points are never named
        idx[idx % 5 == 1] = 0
    else:
        idx = None
    gi = (truth if idx is None else truth[idx]).astype(np.int32)
    return dict(owner=owner, prop_sem=prop_sem, bg=bg, sem=sem, ks=ks, gi=gi, gt_class=gt_class, index=idx, min_points=min_points,
                n_inst=k_rows + n_bg + 1)
