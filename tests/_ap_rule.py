"""The rule of the device ScanNet AP (box2mask_amd/csrc/apmatch.hip, box2mask_amd/eval_match.py) in numpy, over the flat per-scene
arrays the kernels take -- not over the record dictionaries of eval_metric.assign_from_counts.

A scene is dict(inter (K, G) ints, label_id (K,), conf (K,) float32, uniq (G,) ascending ids, gt_vert (G,)); a setting selects
rows of it by a boolean mask.  ``Rule`` accumulates entries over scenes, batches and settings exactly as MatchAccumulator does
and ``finish`` gives the tables: per segment (setting, overlap, class) the integer tp / fp / fn per distinct score, precision,
recall, steps and the AP -- the dot product summed sequentially in ascending order of the thresholds, which is the one place the
device defines an order of its own (np.dot's is the BLAS's).

``mistake`` switches on one deliberate error (MISTAKES); tests/test_ap_rule.py shows that each is caught."""
import numpy as np

VALID = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])
OVERLAPS = np.append(np.arange(0.5, 0.95, 0.05), 0.25)
MIN_REGION = 100
NC, NO = len(VALID), len(OVERLAPS)
MISTAKES = ('ge_iou', 'lt_ignore', 'second_taken', 'max_second', 'ignore_without_small_gt', 'vert_gt_100', 'ties_apart')


def class_index(ids):
    """Index into VALID of every id of the array, or -1."""
    ids = np.asarray(ids, np.int64)
    pos = np.searchsorted(VALID, ids)
    ok = (pos < NC) & (VALID[np.minimum(pos, NC - 1)] == ids)
    return np.where(ok, pos, -1).astype(np.int64)


def gt_table(uniq, gt_vert):
    """(3, G) int32: class index of id // 1000 or -1 | id >= 1000 | points of the id -- field 6 of a scene record."""
    uniq = np.asarray(uniq, np.int64)
    return np.stack([class_index(uniq // 1000), (uniq >= 1000).astype(np.int64), np.asarray(gt_vert, np.int64)]).astype(np.int32)


def row_table(sc, mistake=None):
    """(3, K) int64: vert | void | class index of the label when the row counts, else -1 -- what b2m_ap_rows writes."""
    inter = np.asarray(sc['inter'], np.int64).reshape(len(sc['label_id']), len(sc['uniq']))
    gt = gt_table(sc['uniq'], sc['gt_vert'])
    vert = inter.sum(1)
    void = inter[:, gt[0] < 0].sum(1)
    cls = class_index(sc['label_id'])
    counts = vert > MIN_REGION if mistake == 'vert_gt_100' else vert >= MIN_REGION
    return np.stack([vert, void, np.where(counts, cls, -1)])


def match_scene(sc, sel, mistake=None):
    """One scene under one row selection.  Returns (entries {(o, c): [(score float32, true 0/1)]}, hard (NO, NC) ints,
    has_gt (NC,) bool, has_pred (NC,) bool)."""
    K = len(sc['label_id'])
    inter = np.asarray(sc['inter'], np.int64).reshape(K, len(sc['uniq']))
    conf = np.asarray(sc['conf'])
    assert conf.dtype == np.float32
    gcls, gbig, gvert = (a.astype(np.int64) for a in gt_table(sc['uniq'], sc['gt_vert']))
    vert, void, cls = row_table(sc, mistake)
    sel = np.asarray(sel, bool)
    entries = {}
    hard = np.zeros((NO, NC), np.int64)
    has_gt, has_pred = np.zeros(NC, bool), np.zeros(NC, bool)
    for c in range(NC):
        rows = np.nonzero(sel & (cls == c))[0]
        gts = np.nonzero(gcls == c)[0]
        counted = [g for g in gts if gbig[g] and gvert[g] >= MIN_REGION]
        has_pred[c], has_gt[c] = len(rows) > 0, len(counted) > 0
        for o, th in enumerate(OVERLAPS):
            out = entries.setdefault((o, c), [])
            over = (lambda v: v >= th) if mistake == 'ge_iou' else (lambda v: v > th)
            iou = lambda r, g: float(inter[r, g]) / float(max(gvert[g] + vert[r] - inter[r, g], 1))
            taken = set()
            for g in counted:
                best = None
                for r in rows:
                    if inter[r, g] <= 0 or r in taken or not over(iou(r, g)):
                        continue
                    if best is None:
                        best = conf[r]
                        taken.add(r)
                    else:
                        out.append((max(best, conf[r]) if mistake == 'max_second' else min(best, conf[r]), 0))
                        best = max(best, conf[r])
                        if mistake == 'second_taken':
                            taken.add(r)
                if best is None:
                    hard[o, c] += 1
                else:
                    out.append((best, 1))
            for r in rows:
                hit = [g for g in gts if inter[r, g] > 0]
                if any(over(iou(r, g)) for g in hit):
                    continue
                ignore = void[r] + sum(inter[r, g] for g in hit if not gbig[g])
                if mistake != 'ignore_without_small_gt':
                    ignore += sum(inter[r, g] for g in hit if gvert[g] < MIN_REGION)
                share = float(ignore) / float(vert[r])
                if (share < th) if mistake == 'lt_ignore' else (share <= th):
                    out.append((conf[r], 0))
    return entries, hard, has_gt, has_pred


def curve(scores, trues, hard, mistake=None):
    """The curve of one segment from its entries: dict(tp, fp, fn (m,) int64; precision, recall, steps (m + 1,) fp64; ap)."""
    scores, trues = np.asarray(scores, np.float32), np.asarray(trues, np.int64)
    order = np.argsort(scores, kind='stable')
    s, t = scores[order], trues[order]
    n, n_true = len(s), int(t.sum())
    first = [i for i in range(n) if i == 0 or s[i] != s[i - 1] or mistake == 'ties_apart']
    below = np.concatenate([[0], np.cumsum(t)])                 # below[i] = true entries among the first i
    tp = np.array([n_true - below[i] for i in first], np.int64)
    fp = np.array([n - i for i in first], np.int64) - tp
    fn = np.array([below[i] + hard for i in first], np.int64)
    m = len(first)
    precision, recall = np.zeros(m + 1), np.zeros(m + 1)
    for j in range(m):
        precision[j] = float(tp[j]) / float(tp[j] + fp[j])
        recall[j] = float(tp[j]) / float(tp[j] + fn[j])
    precision[m], recall[m] = 1.0, 0.0
    r = np.concatenate([[recall[0]], recall, [0.0]])
    steps = np.array([0.5 * float(r[j]) - 0.5 * float(r[j + 2]) for j in range(m + 1)])
    ap = 0.0
    for j in range(m + 1):                                      # sequential, ascending j, multiply and add separate
        ap = ap + float(precision[j]) * float(steps[j])
    return dict(tp=tp, fp=fp, fn=fn, precision=precision, recall=recall, steps=steps, ap=ap)


class Rule:
    """The accumulator: ``add(scenes, sels, set_ids)`` with sels[j][s] = the row mask of setting set_ids[j] in scene s."""

    def __init__(self, n_settings, mistake=None):
        self.n, self.mistake = n_settings, mistake
        self.entries = {}                                       # (setting, o, c) -> [(score, true)]
        self.hard = np.zeros((n_settings, NO, NC), np.int64)
        self.flags = np.zeros((n_settings, NC), np.int64)       # bit 0 has_gt, bit 1 has_pred

    def add(self, scenes, sels=None, set_ids=None):
        sels = [[np.ones(len(sc['label_id']), bool) for sc in scenes]] if sels is None else sels
        set_ids = list(range(len(sels))) if set_ids is None else set_ids
        for sid, sel in zip(set_ids, sels):
            for sc, m in zip(scenes, sel):
                e, hard, has_gt, has_pred = match_scene(sc, m, self.mistake)
                for (o, c), v in e.items():
                    self.entries.setdefault((sid, o, c), []).extend(v)
                self.hard[sid] += hard
                self.flags[sid] |= has_gt.astype(np.int64) | (has_pred.astype(np.int64) << 1)

    def segment(self, sid, o, c):
        """(scores float32, trues) of one segment, sorted (score, true): the multiset."""
        v = self.entries.get((sid, o, c), [])
        sc = np.array([a for a, _ in v], np.float32)
        tr = np.array([b for _, b in v], np.int64)
        order = np.lexsort((tr, sc))
        return sc[order], tr[order]

    def curve(self, sid, o, c):
        """None where the segment has no curve (AP 0 or NaN from the flags)."""
        if self.flags[sid, c] != 3:
            return None
        sc, tr = self.segment(sid, o, c)
        return curve(sc, tr, int(self.hard[sid, o, c]), self.mistake)

    def finish(self):
        """(n_settings, classes, overlaps) fp64: the layout of evaluate_matches' table per setting."""
        ap = np.full((self.n, NC, NO), np.nan)
        for sid in range(self.n):
            for c in range(NC):
                for o in range(NO):
                    if self.flags[sid, c] == 3:
                        ap[sid, c, o] = self.curve(sid, o, c)['ap']
                    elif self.flags[sid, c] & 1:
                        ap[sid, c, o] = 0.0
        return ap


# ------------------------------------------------------------------------------------------------ seeded records with the edges
def random_scene(rng, K, n_inst, edges=True):
    """A scene of K rows over ground truths with every edge the rule names: ids below 1000, ids of no valid class, ground truths of
    99 and 100 points, rows of 99 and 100 points, labels outside the valid classes, IoU exactly 1 / 2 and 1 / 4, several rows on
    one ground truth, one row over three ground truths, equal scores."""
    cls_pool = VALID[rng.integers(0, 5, n_inst)]                 # few classes: several instances each
    ids = [0, 7, 1000 * 13 + 1] + [int(1000 * c + i + 1) for i, c in enumerate(cls_pool)]
    uniq = np.array(sorted(set(ids)), np.int64)
    G = len(uniq)
    gt_vert = rng.choice([99, 100, 150, 200, 400], G).astype(np.int64)
    inter = np.zeros((K, G), np.int64)
    label = np.zeros(K, np.int64)
    for r in range(K):
        kind = rng.integers(0, 8)
        g = int(rng.integers(0, G))
        label[r] = uniq[g] // 1000 if rng.random() < 0.8 else rng.choice([0, 1, 13, 40, 3])
        if kind == 0:                                            # half of g and as much of id 0: IoU exactly 1 / 3 or 1 / 2 ...
            inter[r, g] = gt_vert[g] // 2
            inter[r, 0] = int(rng.choice([gt_vert[g] // 2, gt_vert[g]]))
        elif kind == 1:                                          # a row over up to three ground truths
            for gg in rng.choice(G, min(3, G), replace=False):
                inter[r, gg] = int(gt_vert[gg] * rng.choice([0.3, 0.6, 1.0]))
        elif kind == 2:                                          # a row of exactly 99 or 100 points
            inter[r, g] = min(int(rng.choice([99, 100])), gt_vert[g])
            if inter[r].sum() < 99:
                inter[r, 0] += 99 - inter[r].sum()
        elif kind == 3:                                          # mostly on ignored ids: the ignore share decides
            inter[r, 0] = int(rng.choice([25, 50, 100]))
            inter[r, g] = int(rng.choice([25, 50, 100, 300]))
        else:
            inter[r, g] = int(gt_vert[g] * rng.choice([0.2, 0.26, 0.5, 0.55, 0.8, 1.0]))
            inter[r, int(rng.integers(0, G))] += int(rng.integers(0, 120))
        inter[r] = np.minimum(inter[r], gt_vert)
    conf = rng.choice(np.linspace(0.05, 0.95, 7), K).astype(np.float32) if edges else rng.random(K).astype(np.float32)
    return dict(inter=inter, label_id=label, conf=conf, uniq=uniq, gt_vert=gt_vert)


def scene(gts, rows):
    """gts: {id: points}; rows: [(label, conf, {id: shared points})]."""
    uniq = np.array(sorted(gts), np.int64)
    inter = np.zeros((len(rows), len(uniq)), np.int64)
    for r, (_, _, hits) in enumerate(rows):
        for i, v in hits.items():
            inter[r, int(np.searchsorted(uniq, i))] = v
    return dict(inter=inter, label_id=np.array([l for l, _, _ in rows], np.int64).reshape(len(rows)),
                conf=np.array([c for _, c, _ in rows], np.float32).reshape(len(rows)), uniq=uniq,
                gt_vert=np.array([gts[int(i)] for i in uniq], np.int64))


def edge_scenes():
    """Hand-built scenes, one edge each (the list of tests/test_gpu_ap_match.py); every scene has id 0 as real scenes do.
    An IoU of exactly 1 / 2 needs inter 100 of union 200 here: a row under 100 points does not count at all."""
    import itertools
    out = []
    # IoU exactly 0.5 and exactly 0.25: `>` does not match; the row then reaches no ground truth and is a false positive
    out.append(scene({0: 1000, 4001: 150}, [(4, .9, {4001: 100, 0: 50})]))
    out.append(scene({0: 1000, 4001: 300}, [(4, .8, {4001: 100, 0: 100})]))
    # ignore share exactly 0.5 and exactly 0.25: `<=` keeps the entry
    out.append(scene({0: 1000, 5001: 1000}, [(5, .7, {0: 100, 5001: 100}), (5, .6, {0: 50, 5001: 150}), (5, .5, {0: 101, 5001: 99})]))
    # two and three rows on one ground truth, every order of their scores
    for perm in itertools.permutations((.3, .6, .9)):
        out.append(scene({0: 500, 6001: 200}, [(6, c, {6001: v}) for c, v in zip(perm, (180, 170, 160))]))
    for perm in itertools.permutations((.4, .7)):
        out.append(scene({0: 500, 6001: 200}, [(6, c, {6001: v}) for c, v in zip(perm, (180, 170))]))
    # the second row on a matched ground truth is NOT taken: it matches the next ground truth at 0.25
    out.append(scene({0: 500, 7001: 200, 7002: 200}, [(7, .9, {7001: 100}), (7, .8, {7001: 100, 7002: 100})]))
    # one row over 0.25 on three ground truths: it matches the first, the others are hard false negatives
    out.append(scene({0: 500, 8001: 100, 8002: 100, 8003: 100}, [(8, .9, {8001: 100, 8002: 100, 8003: 100})]))
    # rows of 99 and 100 points; ground truths of 99 and 100 points; their share of a row is ignored
    out.append(scene({0: 500, 9001: 100}, [(9, .9, {9001: 99}), (9, .8, {9001: 100})]))
    out.append(scene({0: 500, 10001: 99, 10002: 100, 10003: 1000},
                     [(10, .9, {10001: 99, 0: 21}), (10, .8, {10002: 100}), (10, .7, {10001: 60, 10003: 140})]))
    # ids below 1000 and of no valid class are void; labels outside the valid classes do not count
    out.append(scene({0: 500, 7: 300, 13001: 300, 3001: 200}, [(3, .9, {3001: 150, 7: 30, 13001: 30}), (13, .8, {13001: 300}),
                                                             (40, .7, {3001: 200}), (0, .6, {0: 300}), (3, .5, {7: 200, 3001: 20})]))
    # a class with ground truth and no row (11), with rows and no ground truth (12), with neither (all others)
    out.append(scene({0: 500, 11001: 200}, [(12, .9, {0: 100, 11001: 100})]))
    # equal scores, true in one scene and false in the other
    out.append(scene({0: 500, 14001: 200, 14002: 200}, [(14, .5, {14001: 200}), (14, .25, {14002: 190})]))
    out.append(scene({0: 500, 14001: 2000}, [(14, .5, {14001: 100}), (14, .25, {14001: 100}), (14, .75, {14001: 100})]))
    return out


def false_positive_scene(n, cls=16, seed=0):
    """n rows of class `cls` that reach no ground truth: a segment of n entries at every overlap, one hard false negative."""
    rng = np.random.default_rng(seed + n)
    conf = rng.choice(np.linspace(0.01, 0.99, 197), n)          # repeats among them: ties
    return scene({0: 500, cls * 1000 + 1: 100 * n + 1000}, [(cls, float(c), {cls * 1000 + 1: 100}) for c in conf])
