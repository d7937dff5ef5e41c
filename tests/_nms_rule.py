"""Box-vote clustering, heat-map projection, mask NMS, label / instance histograms and the bit-row gathers restated from
include/b2m.h, for tests/test_nms_rule.py (CPU) and tests/test_gpu_nms_edges.py (the kernels of csrc/nms.hip).

Plain numpy.  The fp32 IoU arithmetic is oracle/nms_ref.py's (pinned to the real reference's goldens by
tests/test_oracle_nms.py); everything the C ABI promises beyond the reference is stated here:

  * clustering: boxes are visited by descending score, EQUAL scores by ascending row, and +0.0 == -0.0; the representative of a
    cluster is the first box visited that no earlier cluster took; heat[r] = IoU(box reps[r], every box) with heat[r, reps[r]] = 1;
    a box joins the cluster unless `iou <= th` (so a NaN IoU joins); only heat rows below max_k are written; `order` holds the
    visiting order in the low 32 bits of its first n entries;
  * projection: value(v) = heat[sel[r], fg_slot[seg2vox[v]]] (0 where the slot is negative), bit = value > th, pad bits above n_vox
    are ZERO -- which is what the mask NMS entries receive; the histogram entries must IGNORE bits at or above n_vox / n, and
    their cases set such bits on purpose;
  * mask NMS: the whole symmetric intersection table, float32(inter) / float32(union) against float32(th), suppress unless
    `iou <= th` (0 / 0 = NaN suppresses), a suppressed row suppresses nothing;
  * label histogram: first maximum, 0 for an empty row, labels outside [0, n_class) skipped;
  * gathers: out[r, p] = bit index[p] of row rows[r], both optional.

Every function takes `mistake=`: one deliberate MISTAKE written as a variant of the rule.  tests/test_nms_rule.py shows that each
fails at least one case of the lists below, i.e. that the cases are sharp.  Every case carries a predicate -- computed from the
input alone -- for the branch of the kernel it exists for, so a case cannot silently stop reaching it.
"""
import functools

import numpy as np

from oracle import nms_ref

F = np.float32
U64 = np.uint64
NMC_THREADS = 1024              # search window of nmc_scene
NMC_LDS_SORT = 4096             # padded keys sorted in LDS; above: in global memory
NMC_MAX_N = 262144
HIST_MAX = 2048
HIST_WPB = 2048                 # words per block of mask_hist_kernel
SENT_F = np.array([0xDEADBEEF], np.uint32).view(F)[0]          # sentinel bit pattern of a float that must not be written
SENT_I = -77
SENT_B = 7

MISTAKES = ('lt_cluster', 'lt_mask', 'tie_high', 'zero_sign', 'no_force', 'no_eps', 'prod_order', 'no_clamp', 'fp64_ratio',
            'last_max', 'pad_counted', 'one_window', 'heat_past_max_k', 'chunk_drop_64')


def same_floats(a, b):
    """Equal by bit pattern; a NaN equals a NaN of any payload."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    if a.shape != b.shape:
        return False
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def npow2(n):
    p = 2
    while p < n:
        p <<= 1
    return p


# ----------------------------------------------------------------------------- box IoU
def box_ious(box, boxes, mistake=None):
    """IoU of one [min3, max3] box with n of them, fp32, in the reference's operation order."""
    if mistake not in ('no_eps', 'prod_order', 'no_clamp'):
        return nms_ref.box_ious(box, boxes)
    box, boxes = np.asarray(box, F), np.asarray(boxes, F)
    bs, ss = box[3:] - box[:3], boxes[:, 3:] - boxes[:, :3]
    d = np.minimum(box[3:][None], boxes[:, 3:]) - np.maximum(box[:3][None], boxes[:, :3])
    isl = d if mistake == 'no_clamp' else np.where(d < 0, F(0), d).astype(F)
    if mistake == 'prod_order':
        inter, ba, sa = isl[:, 0] * (isl[:, 1] * isl[:, 2]), bs[0] * (bs[1] * bs[2]), ss[:, 0] * (ss[:, 1] * ss[:, 2])
    else:
        inter, ba, sa = (isl[:, 0] * isl[:, 1]) * isl[:, 2], (bs[0] * bs[1]) * bs[2], (ss[:, 0] * ss[:, 1]) * ss[:, 2]
    union = (ba + sa) - inter
    if mistake != 'no_eps':
        union = union + nms_ref.EPS
    with np.errstate(divide='ignore', invalid='ignore'):
        return (inter / union).astype(F)


def set_ious(a, b):
    return nms_ref.set_ious(a, b)


# ----------------------------------------------------------------------------- clustering
def visiting_order(scores, mistake=None):
    """Rows by descending score; equal scores (the two zeros are equal) by ascending row."""
    s = np.asarray(scores, F)
    assert not np.isnan(s).any(), 'NaN scores are outside the contract'
    rows = np.arange(len(s))
    if mistake == 'zero_sign':                 # order by the bit pattern of -score: +0.0 before -0.0
        u = (-s).view(np.uint32).astype(np.uint64)
        key = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
        return np.lexsort((rows, key))
    neg = -(s + F(0))                          # -0.0 + 0.0 = +0.0
    return np.lexsort((-rows if mistake == 'tie_high' else rows, neg))


def nmc(boxes, th, max_k, heat_rows=None, mistake=None):
    """dict(k, reps (k,), assign (n,), order (n,), heat (heat_rows, n) with SENT_F wherever nothing is written, found = the
    (search start, position found) of every representative in visiting order).  heat_rows defaults to max_k."""
    boxes = np.asarray(boxes, F).reshape(-1, 7)
    n = len(boxes)
    th = F(th)
    heat_rows = max_k if heat_rows is None else heat_rows
    order = visiting_order(boxes[:, 0], mistake)
    b6 = boxes[:, 1:]
    alive = np.ones(n, bool)
    assign = np.full(n, SENT_I, np.int32)
    heat = np.full((heat_rows, n), SENT_F, F)
    reps, found, p0 = [], [], 0
    while p0 < n:
        a = np.flatnonzero(alive[order[p0:]])
        if len(a) == 0 or (mistake == 'one_window' and a[0] >= NMC_THREADS):
            break
        pf = p0 + int(a[0])
        r = int(order[pf])
        h = box_ious(b6[r], b6, mistake)
        if mistake != 'no_force':
            h[r] = F(1)
        if len(reps) < (heat_rows if mistake == 'heat_past_max_k' else min(max_k, heat_rows)):
            heat[len(reps)] = h
        hit = alive & ~((h < th) if mistake == 'lt_cluster' else (h <= th))
        assign[hit] = len(reps)
        alive[hit] = False
        reps.append(r)
        found.append((p0, pf))
        p0 = pf + 1
    return dict(k=len(reps), reps=np.array(reps, np.int32), assign=assign, order=order.astype(np.int64), heat=heat, found=found)


def window_skips(found):
    """Whole windows of NMC_THREADS positions the search for each representative passes over."""
    return [(pf - p0) // NMC_THREADS for p0, pf in found]


def nmc_batch_desc(ns, mks):
    """(desc int64 (S, 6), total boxes, heat elements, order elements): scenes back to back."""
    desc = np.zeros((len(ns), 6), np.int64)
    bo = ho = oo = 0
    for s, (n, mk) in enumerate(zip(ns, mks)):
        desc[s] = (bo, n, npow2(n), mk, ho, oo)
        bo += n; ho += mk * n; oo += npow2(n)
    return desc, bo, ho, oo


# ----------------------------------------------------------------------------- bit rows
def pack(masks):
    """(k, n) bytes, non-zero = set -> (k, ceil(n / 64)) uint64, bit v of word v // 64; pad bits zero."""
    m = np.asarray(masks) != 0
    k, n = m.shape
    words = (n + 63) // 64
    full = np.zeros((k, max(words, 1) * 64), np.uint8)
    full[:, :n] = m
    return np.packbits(full, axis=1, bitorder='little').view('<u8').reshape(k, max(words, 1)).astype(U64)


def unpack(bits, n=None):
    """(k, words) uint64 -> (k, words * 64 or n) bool."""
    b = np.ascontiguousarray(np.asarray(bits, U64)).astype('<u8')
    m = np.unpackbits(b.view(np.uint8).reshape(len(b), b.shape[1] * 8), axis=1, bitorder='little').astype(bool)
    return m if n is None else m[:, :n]


def project(heat, sel, fg_slot, seg2vox, th, mistake=None):
    """Bit rows (ksel, ceil(n_vox / 64)) of heat[sel] through fg_slot[seg2vox]."""
    heat = np.asarray(heat, F)
    slot = np.asarray(fg_slot)[np.asarray(seg2vox)]
    val = np.where(slot[None] >= 0, heat[np.asarray(sel, np.int64)][:, np.maximum(slot, 0)], F(0)).astype(F)
    m = val > F(th)
    if mistake == 'chunk_drop_64':
        m[64::64] = False
    return pack(m)


def inter_table(bits):
    bits = np.asarray(bits, U64)
    k = len(bits)
    out = np.zeros((k, k), np.int64)
    for i in range(k):
        out[i, i:] = np.bitwise_count(bits[i][None] & bits[i:]).sum(1, dtype=np.int64)
        out[i:, i] = out[i, i:]
    return out.astype(np.int32)


def mask_nms(bits, th, mistake=None):
    """(inter (k, k) int32, keep (k,) int32, n_keep).  Rows in the given order; pad bits of `bits` are zero."""
    inter = inter_table(bits).astype(np.int64)
    k = len(inter)
    cnt = np.diagonal(inter).copy()
    keep = np.ones(k, np.int32)
    for i in range(k):
        if not keep[i]:
            continue
        un = cnt[i] + cnt - inter[i]
        with np.errstate(divide='ignore', invalid='ignore'):
            if mistake == 'fp64_ratio':
                iou, t = inter[i].astype(np.float64) / un.astype(np.float64), np.float64(F(th))
            else:
                iou, t = inter[i].astype(F) / un.astype(F), F(th)
        sup = ~((iou < t) if mistake == 'lt_mask' else (iou <= t))
        sup[:i + 1] = False
        keep[sup] = 0
    return inter.astype(np.int32), keep, int(keep.sum())


def _hist(row_bits, label, n, n_class, mistake=None):
    m = unpack(row_bits[None])[0]
    label = np.asarray(label)
    if mistake == 'pad_counted':                            # bits at or above n counted, with the last voxel's label
        lab = np.concatenate([label[:n], np.full(len(m) - n, label[n - 1])])
    else:
        lab, m = label[:n], m[:n]
    lab = lab[m]
    lab = lab[(lab >= 0) & (lab < n_class)]
    return np.bincount(lab, minlength=n_class).astype(np.int32)


def label_hist(bits, rows, sem, n_vox, n_class, mistake=None):
    """labels (k,) int32: the first maximum of each row's class histogram (0 for an empty row)."""
    bits = np.asarray(bits, U64)
    rows = np.arange(len(bits)) if rows is None else np.asarray(rows)
    out = np.zeros(len(rows), np.int32)
    for r, row in enumerate(rows):
        h = _hist(bits[row], sem, n_vox, n_class, mistake)
        out[r] = (n_class - 1 - int(np.argmax(h[::-1]))) if mistake == 'last_max' else int(np.argmax(h))
    return out


def mask_hist(bits, label, n, n_class, mistake=None):
    bits = np.asarray(bits, U64)
    return np.stack([_hist(b, label, n, n_class, mistake) for b in bits], 0).reshape(len(bits), n_class)


def gather(bits, rows, index, n_pts):
    """(k, n_pts) uint8: bit index[p] of row rows[r]."""
    bits = np.asarray(bits, U64)
    rows = np.arange(len(bits)) if rows is None else np.asarray(rows, np.int64)
    v = np.arange(n_pts) if index is None else np.asarray(index, np.int64)
    return ((bits[rows][:, v >> 6] >> (v & 63).astype(U64)) & U64(1)).astype(np.uint8).reshape(len(rows), n_pts)


# ----------------------------------------------------------------------------- the B2M_MASK_DESC table
MASK_FIELDS = ('heat', 'n_fg', 'sel', 'ksel', 'fg_slot', 'seg2vox', 'n_vox', 'bits', 'words', 'inter', 'keep', 'rows', 'kk', 'sem',
               'labels', 'index', 'n_pts', 'out', 'row0_sel', 'row0_kept')
MASK_POINTERS = ('heat', 'sel', 'fg_slot', 'seg2vox', 'bits', 'inter', 'keep', 'rows', 'sem', 'labels', 'index', 'out')
assert len(MASK_FIELDS) == 20


def mask_desc(scenes, address):
    """int64 (S, 20) from a list of scene dicts.  Sizes are read from the dict (missing = 0), address(s, name) gives the device
    address of a pointer field (0 = NULL); fields 18 / 19 are the running counts of ksel / kk."""
    desc = np.zeros((len(scenes), len(MASK_FIELDS)), np.int64)
    r_sel = r_kept = 0
    for s, sc in enumerate(scenes):
        for f, name in enumerate(MASK_FIELDS[:18]):
            desc[s, f] = address(s, name) if name in MASK_POINTERS else int(sc.get(name, 0))
        desc[s, 18:] = (r_sel, r_kept)
        r_sel += int(sc.get('ksel', 0)); r_kept += int(sc.get('kk', 0))
    return desc


# ============================================================================= cases
class Case:
    def __init__(self, name, reach, **kw):
        self.name, self.reach = name, reach             # reach: dict predicate name -> bool, computed from the input
        self.__dict__.update(kw)

    def __repr__(self):
        return self.name


def votes(seed, n, n_obj, jitter=0.02):
    """n boxes [score, min3, max3] around n_obj objects 10 apart (half size 0.4 .. 0.6, bounded jitter: the IoU of two votes of
    one object stays above 0.7), rows shuffled."""
    rng = np.random.default_rng(seed)
    n_obj = max(1, min(n_obj, n))
    c = (10.0 * np.stack(np.unravel_index(np.arange(n_obj), (4, 4, 4)), 1)).astype(F) + rng.uniform(0, 1, (n_obj, 3)).astype(F)
    half = rng.uniform(0.4, 0.6, (n_obj, 3)).astype(F)
    obj = rng.integers(0, n_obj, n)
    obj[:n_obj] = np.arange(n_obj)
    lo = c[obj] - half[obj] + rng.uniform(-jitter, jitter, (n, 3)).astype(F)
    hi = c[obj] + half[obj] + rng.uniform(-jitter, jitter, (n, 3)).astype(F)
    b = np.concatenate([rng.uniform(0.05, 0.95, (n, 1)).astype(F), lo.astype(F), hi.astype(F)], 1).astype(F)
    return np.ascontiguousarray(b[rng.permutation(n)])


def _disjoint(n, scores):
    b = np.zeros((n, 7), F)
    for i in range(n):
        b[i] = [0, 3 * i, 0, 0, 3 * i + 1, 1, 1]
    b[:, 0] = np.asarray(scores, F)
    return b


# ---- clustering: sizes
NMC_SIZES = (1, 2, 31, 32, 33, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097, 8193)


@functools.lru_cache(maxsize=None)
def nmc_size_case(n):
    b = votes(100 + n, n, 5)
    want = nmc(b, 0.5, 8, 9)
    reach = dict(few_clusters=1 <= want['k'] <= 8,
                 sort_path=(npow2(n) <= NMC_LDS_SORT) == (n <= 4096), npad=n not in (4097, 8193) or npow2(n) == {4097: 8192, 8193: 16384}[n],
                 shuffled=n < 31 or not np.array_equal(want['order'], np.arange(n)))
    return Case('n:%d' % n, reach, boxes=b, th=0.5, max_k=8, heat_rows=9, sort='lds' if npow2(n) <= NMC_LDS_SORT else 'global',
                last_word_bits=n % 32)


# ---- clustering: the window search
def _window_boxes(n, survivors, seed):
    """The best box and copies of it everywhere, except disjoint boxes at the visiting positions `survivors`; rows shuffled."""
    rng = np.random.default_rng(seed)
    b = np.zeros((n, 7), F)
    b[:, 1:] = [0, 0, 0, 1, 1, 1]
    for i, p in enumerate(survivors):
        b[p, 1:] = [5 * (i + 1), 0, 0, 5 * (i + 1) + 1, 1, 1]
    b[:, 0] = (F(1) - np.arange(n, dtype=F) / F(n)).astype(F)          # position p has the p-th best score, all distinct
    assert len(np.unique(b[:, 0])) == n
    return np.ascontiguousarray(b[rng.permutation(n)])


WINDOW_CASES = (('win:1023', 3000, (1023,)), ('win:1024', 3000, (1024,)), ('win:1025', 3000, (1025,)), ('win:2048', 2049, (2048,)),
                ('win:2048g', 5000, (2048,)), ('win:last', 3000, (2999,)), ('win:last_g', 5000, (4999,)),
                ('win:all', 5000, (1023, 1024, 1025, 2048, 4999)))


@functools.lru_cache(maxsize=None)
def window_case(name):
    _, n, surv = next(c for c in WINDOW_CASES if c[0] == name)
    b = _window_boxes(n, surv, len(name) + n)
    want = nmc(b, 0.5, len(surv) + 1, len(surv) + 2)
    pos = [pf for _, pf in want['found']]
    skips = window_skips(want['found'])
    slots = [(pf - p0) % NMC_THREADS for p0, pf in want['found']]
    reach = dict(survivors_are_reps=pos == [0] + list(surv), k=want['k'] == len(surv) + 1)
    return Case(name, reach, boxes=b, th=0.5, max_k=len(surv) + 1, heat_rows=len(surv) + 2, skips=skips, slots=slots,
                sort='lds' if npow2(n) <= NMC_LDS_SORT else 'global')


# ---- clustering: ties, IoU edges, degenerate boxes, non-finite values
def _pair_iou():
    a = np.array([0.1, 0.2, 0.3, 1.3, 1.1, 1.7], F)
    b = np.array([0.4, 0.1, 0.5, 1.5, 1.2, 1.9], F)
    return a, b, box_ious(a, b[None])[0]


@functools.lru_cache(maxsize=None)
def nmc_edge_case(name):
    rng = np.random.default_rng(7)
    th, reach = F(0.5), {}
    if name == 'ties_shuffled':
        sc = rng.choice(np.array([0.25, 0.5, 0.75], F), 40)
        b = _disjoint(40, sc)
        b = b[rng.permutation(40)]
        want = visiting_order(b[:, 0])
        reach = dict(ties=len(np.unique(sc)) < 40, rows_decide=not np.array_equal(want, visiting_order(b[:, 0], 'tie_high')))
    elif name in ('zeros:neg_first', 'zeros:pos_first'):
        z = [-0.0, 0.0] if name == 'zeros:neg_first' else [0.0, -0.0]
        b = _disjoint(6, [0.5] + z + [-1.0] + z[::-1])
        reach = dict(both_zeros=set(b[1:3, 0].view(np.uint32).tolist()) == {0, 0x80000000},
                     row_order=np.array_equal(visiting_order(b[:, 0]), [0, 1, 2, 4, 5, 3]),
                     sign_order_differs=not np.array_equal(visiting_order(b[:, 0]), visiting_order(b[:, 0], 'zero_sign')))
    elif name == 'neg_inf_scores':
        b = _disjoint(8, [-1.0, np.inf, -np.inf, 3.0, -2.5, 0.5, np.inf, -np.inf])
        b[5, 1:] = b[3, 1:]                                  # one real merge
        reach = dict(order=np.array_equal(visiting_order(b[:, 0]), [1, 6, 3, 5, 0, 4, 2, 7]))
    elif name in ('iou_eq_th', 'iou_above_th'):
        a, c, t = _pair_iou()
        th = t if name == 'iou_eq_th' else np.nextafter(t, F(0))
        b = np.zeros((2, 7), F)
        b[0], b[1] = np.concatenate([[0.9], a]), np.concatenate([[0.8], c])
        k = nmc(b, th, 2)['k']
        reach = dict(th_in_range=0 < th < 1, merges=k == (2 if name == 'iou_eq_th' else 1))
    elif name == 'zero_volume_rep':
        b = _disjoint(5, [0.9, 0.8, 0.7, 0.6, 0.5])
        b[0, 4] = b[0, 1]                                    # the best box has no extent in x
        b[3, 1:] = [3.2, 0.2, 0.2, 3.2, 0.8, 0.8]            # a flat box inside box 1
        b[4, 1:] = b[0, 1:]                                  # a copy of the flat representative: IoU 0 / 1e-6 = 0
        reach = dict(self_iou_zero=box_ious(b[0, 1:], b[:1, 1:])[0] == 0, own_clusters=nmc(b, th, 5)['k'] == 5)
    elif name == 'inverted':
        b = _disjoint(6, [0.9, 0.8, 0.7, 0.6, 0.5, 0.4])
        b[1, 1:] = [0.9, 0.1, 0.1, 0.2, 0.9, 0.9]            # min > max in x, inside box 0
        b[2, 1:] = [0.8, 0.8, 0.1, 0.1, 0.1, 0.9]            # ... in x and y
        b[4, 1:] = [10, 1, 1, 9, 0, 0]                       # ... on every axis, far away
        b[5, 1:] = [10, 1, 1, 9, 0, 0]
        reach = dict(negative_sides=bool(((b[:, 4:] - b[:, 1:4]) < 0).any()))
    elif name == 'nan_coord':
        b = _disjoint(5, [0.9, 0.8, 0.7, 0.1, 0.6])
        b[3, 2] = np.nan
        want = nmc(b, th, 5)
        reach = dict(not_a_rep=3 not in want['reps'].tolist(), joins_first=want['assign'][3] == 0,
                     heat_nan=bool(np.isnan(want['heat'][:want['k'], 3]).all()))
    elif name == 'duplicates':
        b = votes(3, 60, 4)
        b = np.concatenate([b, b[:30], b[:10]], 0)
        b = np.ascontiguousarray(b[rng.permutation(len(b))])
        reach = dict(dups=len(np.unique(b, axis=0)) < len(b))
    else:
        raise KeyError(name)
    b = np.ascontiguousarray(b, F)
    return Case(name, reach, boxes=b, th=th, max_k=len(b), heat_rows=len(b) + 1)


NMC_EDGE_CASES = ('ties_shuffled', 'zeros:neg_first', 'zeros:pos_first', 'neg_inf_scores', 'iou_eq_th', 'iou_above_th',
                  'zero_volume_rep', 'inverted', 'nan_coord', 'duplicates')


# ---- clustering: max_k
MAXK_CASES = ('k_gt_max_k', 'k_eq_max_k', 'max_k_0')


@functools.lru_cache(maxsize=None)
def maxk_case(name):
    b = votes(11, 300, 6)
    k = nmc(b, 0.5, 300, 0)['k']
    max_k = {'k_gt_max_k': 3, 'k_eq_max_k': k, 'max_k_0': 0}[name]
    reach = dict(k=k == 6, relation={'k_gt_max_k': k > max_k, 'k_eq_max_k': k == max_k, 'max_k_0': max_k == 0}[name])
    return Case(name, reach, boxes=b, th=0.5, max_k=max_k, heat_rows=0 if name == 'max_k_0' else k + 1)


@functools.lru_cache(maxsize=None)
def ceiling_case():
    b = votes(12, NMC_MAX_N, 8)
    return Case('n:262144', dict(at_ceiling=len(b) == NMC_MAX_N, npad=npow2(len(b)) == NMC_MAX_N), boxes=b, th=0.5, max_k=8,
                heat_rows=9)


# ---- clustering: batch
BATCH_NS = (0, 1, 33, 1025, 0, 4097, 300)


@functools.lru_cache(maxsize=None)
def nmc_batch_case():
    scenes = []
    for s, n in enumerate(BATCH_NS):
        if n == 300:
            b = _disjoint(300, np.random.default_rng(5).uniform(0, 1, 300))          # 300 clusters: more than min(n, 256)
        else:
            b = votes(200 + s, n, 4) if n else np.zeros((0, 7), F)
        scenes.append(np.ascontiguousarray(b, F))
    ks = [nmc(b, 0.5, 0, 0)['k'] if len(b) else 0 for b in scenes]
    reach = dict(empty_scenes=BATCH_NS.count(0) == 2, overflow=any(k > min(n, 256) for k, n in zip(ks, BATCH_NS)),
                 both_sorts={npow2(n) <= NMC_LDS_SORT for n in BATCH_NS if n} == {True, False})
    return Case('batch', reach, scenes=scenes, th=0.5, ks=ks)


# ---- projection
PROJ_NVOX = (1, 63, 64, 65, 255, 256, 257, 1000)
PROJ_KSEL = (0, 1, 63, 64, 65, 129)
PROJ_TH = F(0.3)


@functools.lru_cache(maxsize=None)
def project_case(n_vox, ksel):
    rng = np.random.default_rng(1000 * ksel + n_vox)
    n_seg = max(2, n_vox // 3)
    fg = rng.random(n_seg) < 0.7
    fg[0], fg[1] = True, False
    fg_slot = np.where(fg, np.cumsum(fg) - 1, -1).astype(np.int32)
    n_fg = int(fg.sum())
    seg2vox = rng.integers(0, n_seg, n_vox).astype(np.int64)
    if n_vox >= 2:
        seg2vox[-1] = 1                                        # a background voxel at the very end
    K = ksel + 3
    heat = rng.random((K, n_fg)).astype(F)
    heat[rng.random((K, n_fg)) < 0.15] = PROJ_TH               # exactly the threshold: bit off
    sel = rng.permutation(K)[:ksel].astype(np.int32)
    slot = fg_slot[seg2vox]
    reach = dict(chunks=(ksel + 63) // 64 == {0: 0, 1: 1, 63: 1, 64: 1, 65: 2, 129: 3}[ksel], partial_word=(n_vox % 64 != 0) == (n_vox not in (64, 256)),
                 background=n_vox < 2 or bool((slot < 0).any()),
                 at_threshold=ksel == 0 or n_vox < 63 or bool((heat[sel][:, np.maximum(slot, 0)][:, slot >= 0] == PROJ_TH).any()),
                 scrambled=ksel < 63 or not np.array_equal(sel, np.sort(sel)))
    return Case('project:%d:%d' % (n_vox, ksel), reach, heat=heat, n_fg=n_fg, sel=sel, ksel=ksel, fg_slot=fg_slot, seg2vox=seg2vox,
                n_vox=n_vox, words=(n_vox + 63) // 64, th=PROJ_TH)


PROJ_BATCH = ((257, 65), (64, 1), (1000, 0), (63, 129), (1, 64), (255, 63))     # (n_vox, ksel): a ksel = 0 scene in the middle


# ---- mask NMS
MNMS_K = (1, 2, 255, 256, 257, 513)
MNMS_WORDS = (1, 255, 256, 257)


def _proto_rows(rng, k, n_vox, words, n_proto=None):
    """k rows: noisy copies of a few prototypes (IoUs on both sides of the threshold), pad bits zero."""
    n_proto = n_proto or max(1, min(k // 3, 40))
    proto = rng.random((n_proto, n_vox)) < 0.4
    m = proto[rng.integers(0, n_proto, k)] ^ (rng.random((k, n_vox)) < rng.choice([0.02, 0.12, 0.3], (k, 1)))
    m[:, 0] = True                                              # no empty row here
    return pack(m)


@functools.lru_cache(maxsize=None)
def mask_nms_case(k, words):
    rng = np.random.default_rng(31 * k + words)
    n_vox = words * 64 - 5
    bits = _proto_rows(rng, k, n_vox, words)
    _, keep, nk = mask_nms(bits, 0.6)
    reach = dict(pad_zero=not unpack(bits)[:, n_vox:].any(), some_suppressed=k < 255 or 0 < nk < k,
                 j_stride=(k > 256) == (k in (257, 513)), w_stride=(words > 256) == (words == 257))
    return Case('mnms:%d:%d' % (k, words), reach, bits=bits, k=k, words=words, th=F(0.6))


def _rows_of(sets, n):
    m = np.zeros((len(sets), n), bool)
    for i, s in enumerate(sets):
        m[i, list(s)] = True
    return pack(m)


MNMS_EDGE_CASES = ('seven_tenths', 'th_eq_ratio', 'empty_and_identical', 'chain', 'big_union')


@functools.lru_cache(maxsize=None)
def mask_nms_edge_case(name):
    r = range
    if name == 'seven_tenths':
        bits, th = _rows_of([r(0, 8), r(1, 10)], 70), F(0.7)
        want = [1, 1]
    elif name == 'th_eq_ratio':
        bits, th = _rows_of([r(0, 2), r(1, 3), r(100, 101)], 130), F(1) / F(3)
        want = [1, 1, 1]
    elif name == 'empty_and_identical':
        bits, th = _rows_of([r(0, 9), (), r(0, 9), (), r(20, 30)], 64), F(0.5)
        want = [1, 1, 0, 0, 1]
    elif name == 'chain':
        bits, th = _rows_of([r(0, 10), r(3, 13), r(6, 16)], 64), F(0.5)
        want = [1, 0, 1]
    elif name == 'big_union':
        n = (1 << 24) + 4096
        words = n // 64
        bits = np.zeros((2, words), U64)
        bits[0, :] = ~U64(0)
        bits[0, -1] = ~U64(0) >> U64(1)                         # |a| = 2^24 + 4095: float32 rounds it UP to 2^24 + 4096
        m = 9_000_001
        bits[1, :m // 64] = ~U64(0)
        bits[1, m // 64] = (U64(1) << U64(m % 64)) - U64(1)
        th = F(m) / F(n - 1)                                    # in fp32 the ratio IS th: kept; m / (n - 1) exactly is above it
        want = [1, 1]
    else:
        raise KeyError(name)
    inter, keep, nk = mask_nms(bits, th)
    reach = dict(expected=keep.tolist() == want)
    if name == 'big_union':
        un = int(inter[0, 0]) + int(inter[1, 1]) - int(inter[0, 1])
        reach.update(union_rounds=int(F(un)) != un, exact_ratio_above=int(inter[0, 1]) / un > float(th))
    if name == 'seven_tenths':
        reach.update(fp64_above=7 / 10 > float(th), fp32_equal=F(7) / F(10) == th)
    return Case(name, reach, bits=bits, k=len(bits), words=bits.shape[1], th=th)


MNMS_BATCH = ((5, 3, True), (257, 2, True), (40, 257, False), (1, 1, True), (64, 70, True))       # (ksel, words, has keep)


@functools.lru_cache(maxsize=None)
def mask_nms_batch_case():
    rng = np.random.default_rng(77)
    scenes = []
    for ksel, words, has_keep in MNMS_BATCH:
        scenes.append(dict(ksel=ksel, words=words, n_vox=words * 64 - 3, bits=_proto_rows(rng, ksel, words * 64 - 3, words, 4),
                           has_keep=has_keep))
    reach = dict(null_keep=any(not s['has_keep'] for s in scenes), below_max=min(s['ksel'] for s in scenes) < max(s['ksel'] for s in scenes))
    return Case('mnms_batch', reach, scenes=scenes, th=F(0.6), max_k=max(s['ksel'] for s in scenes))


# ---- label histogram
LH_WORDS = (1, 63, 64, 65, 257)
LH_NCLASS = (1, 20, 256)


def _lh_scene(rng, words, n_class, scrambled, k=7):
    """Rows: random, EMPTY, an exact tie between two classes, everything set; the last word's bits above n_vox are set on purpose."""
    n_vox = words * 64 - 7
    sem = rng.integers(-1, n_class + 1, n_vox).astype(np.int32)
    sem[rng.random(n_vox) < 0.05] = -100
    sem[0], sem[n_vox - 1] = min(1, n_class - 1), n_class - 1
    m = rng.random((k, words * 64)) < 0.3
    m[1] = False
    m[3] = True
    if n_class > 1:                                              # row 2: as many voxels of class c2 as of class c1 < c2, nothing else
        assert n_class > 2
        c1, c2 = 1, n_class - 1
        v1, v2 = np.flatnonzero(sem == c1), np.flatnonzero(sem == c2)
        t = min(len(v1), len(v2))
        m[2] = False
        m[2, v1[:t]] = m[2, v2[:t]] = True
    m[:, n_vox:] = True                                          # pad bits SET: the histograms must ignore them
    m[1, n_vox:] = False
    m[4, n_vox:] = False
    bits = pack(m)
    rows = rng.permutation(k)[:k - 2].astype(np.int32) if scrambled else None
    return dict(bits=bits, words=words, n_vox=n_vox, sem=sem, rows=rows, kk=k - 2 if scrambled else k, ksel=k)


@functools.lru_cache(maxsize=None)
def label_hist_case(words, n_class, scrambled):
    sc = _lh_scene(np.random.default_rng(words * 7 + n_class + scrambled), words, n_class, scrambled)
    hist = mask_hist(sc['bits'], sc['sem'], sc['n_vox'], n_class)
    top = hist.max(1)
    reach = dict(pad_bits_set=bool(unpack(sc['bits'])[:, sc['n_vox']:].any()), empty_row=bool((hist.sum(1) == 0).any()),
                 tie=n_class == 1 or bool((((hist == top[:, None]).sum(1) > 1) & (top > 0)).any()),
                 out_of_range=bool((sc['sem'] == -100).any() or words == 1) and bool((sc['sem'] == n_class).any() or words == 1),
                 w_stride=(words > 256) == (words == 257))
    return Case('lh:%d:%d:%d' % (words, n_class, scrambled), reach, n_class=n_class, **sc)


LH_BATCH = ((1, 0), (65, 7), (257, 5), (2, 0), (64, 7), (1, 5), (63, 0))          # (words, kk): kk = 0 at the front, in the middle, at the end


@functools.lru_cache(maxsize=None)
def label_hist_batch_case(n_class):
    rng = np.random.default_rng(900 + n_class)
    scenes = []
    for words, kk in LH_BATCH:
        sc = _lh_scene(rng, words, n_class, kk == 5)
        if kk == 0:
            sc.update(rows=None, kk=0)
        scenes.append(sc)
    kks = [s['kk'] for s in scenes]
    reach = dict(empty_front=kks[0] == 0, empty_middle=kks[3] == 0, empty_end=kks[-1] == 0, mixed_rows={s['rows'] is None for s in scenes if s['kk']} == {True, False})
    return Case('lh_batch:%d' % n_class, reach, scenes=scenes, n_class=n_class)


# ---- instance histogram
MH_WORDS = (1, 2047, 2048, 2049, 4097)
MH_NCLASS = (1, 2048)
MH_K = (1, 3)


@functools.lru_cache(maxsize=None)
def mask_hist_case(words, n_class, k):
    rng = np.random.default_rng(words + n_class + k)
    n = words * 64 - 13
    label = rng.integers(-1, n_class + 1, n).astype(np.int32)
    m = rng.random((k, words * 64)) < 0.5
    m[:, n:] = True
    reach = dict(n_not_multiple=n % 64 != 0, blocks=(words + HIST_WPB - 1) // HIST_WPB == {1: 1, 2047: 1, 2048: 1, 2049: 2, 4097: 3}[words],
                 pad_bits_set=True, out_of_range=n < 100 or bool((label < 0).any() and (label == n_class).any()))
    return Case('mh:%d:%d:%d' % (words, n_class, k), reach, bits=pack(m), words=words, n=n, label=label, n_class=n_class, k=k)


# ---- gathers
GATHER_KK = (1, 63, 64, 65, 128, 129)
GATHER_NPTS = (1, 3, 4, 15, 16, 17, 4095, 4096, 4097)


@functools.lru_cache(maxsize=None)
def gather_batch_case(kk):
    """One table per kk: every n_pts, index / rows alternately NULL, a scene without kept rows in the middle."""
    rng = np.random.default_rng(kk)
    scenes = []
    for i, n_pts in enumerate(GATHER_NPTS):
        ident, norows = i % 3 == 1, i % 2 == 1
        n_vox = n_pts if ident else 333 + 64 * i
        ksel = kk if norows else kk + 3
        words = (n_vox + 63) // 64
        bits = rng.integers(0, 1 << 63, (ksel, words), dtype=np.int64).astype(U64) * U64(2) + rng.integers(0, 2, (ksel, words)).astype(U64)
        scenes.append(dict(n_vox=n_vox, words=words, ksel=ksel, bits=bits, kk=kk, n_pts=n_pts,
                           rows=None if norows else rng.permutation(ksel)[:kk].astype(np.int32),
                           index=None if ident else rng.integers(0, n_vox, n_pts).astype(np.int64)))
        if i == 4:
            scenes.append(dict(n_vox=300, words=5, ksel=4, bits=rng.integers(0, 1 << 62, (4, 5), dtype=np.int64).astype(U64), kk=0,
                               n_pts=640, rows=np.zeros(0, np.int32), index=rng.integers(0, 300, 640).astype(np.int64)))
    reach = dict(nw=(kk + 63) // 64 == {1: 1, 63: 1, 64: 1, 65: 2, 128: 2, 129: 3}[kk],
                 null_index=any(s['index'] is None for s in scenes), null_rows=any(s['rows'] is None and s['kk'] for s in scenes),
                 both=any(s['index'] is not None and s['rows'] is not None for s in scenes),
                 tails={s['n_pts'] % 4 for s in scenes} == {0, 1, 3} and {s['n_pts'] % 16 for s in scenes} >= {0, 1, 15})
    return Case('gather:%d' % kk, reach, scenes=scenes)


PACK_N = (1, 63, 64, 65, 257)


def pack_case(n):
    rng = np.random.default_rng(n)
    m = rng.choice(np.array([0, 0, 1, 2, 128, 255], np.uint8), (5, n))
    m[0, 0] = 2
    return Case('pack:%d' % n, dict(other_bytes=bool((m > 1).any())), masks=m, n=n, words=(n + 63) // 64)


# ---- set_ious
SET_N = (0, 1, 255, 256, 257)


def set_ious_case(n):
    rng = np.random.default_rng(40 + n)
    lo = rng.uniform(-3, 3, (n, 3))
    a = np.concatenate([lo, lo + rng.uniform(0.1, 2, (n, 3))], 1).astype(F)
    lo = lo + rng.uniform(-1, 1, (n, 3))
    b = np.concatenate([lo, lo + rng.uniform(0.1, 2, (n, 3))], 1).astype(F)
    special = [([1, 1, 1, 1, 2, 2], [1, 1, 1, 1, 2, 2]),                  # zero volume both: 0 / 1e-6
               ([0, 0, 0, 1, 1, 1], [1, 0, 0, 2, 1, 1]),                  # touching
               ([0, 0, 0, 4, 4, 4], [1, 1, 1, 2, 2, 2]),                  # containment
               ([0, 0, 0, 1, 1, 1], [0, 0, 0, 1, 1, 1])]                  # identical
    for i, (x, y) in enumerate(special[:max(0, n - 1)]):
        a[i + 1], b[i + 1] = x, y
    reach = dict(full_mantissa=n == 0 or bool((a.view(np.uint32) & 0xFFF).any()), specials=n < 255 or set_ious(a, b)[1] == 0)
    return Case('set:%d' % n, reach, a=a, b=b, n=n)
