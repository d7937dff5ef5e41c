"""Plain torch restatement, on the CPU, of the three loss terms the fused route gained after tests/_loss_rule.py was written:
the IoU loss (the reference's models/model.py:91-129) and the centre-score loss (:179-192) of `b2m_detection_loss_ex`, and the
row-wise cross entropy of the per-voxel head (:212-223, `b2m_rows_ce_loss`).  Same style as _loss_rule: `dtype` = float64 is
the reference value, float32 the yardstick (`_loss_rule.bound`); gradients come from autograd; every discrete decision is taken
from the fp32 inputs so the two evaluations cannot disagree on a branch:

  * the corners of both boxes are formed in fp32 in torch's order; which corner wins a max / min, whether an intersection side
    is clamped, whether a bound is clamped at float32(min_bb_size) and whether the union is floored at float32(1e-6) are read
    off those fp32 numbers (the union's from its fp32 value in torch's order of operations);
  * at ties the conventions are torch autograd's (test_loss_heads_rule.py::test_tie_conventions_are_torch_autograds):
    maximum / minimum of equal corners send half of the gradient to each argument; clamp(x, min=m) passes the gradient at
    x == m -- an intersection side of exactly 0, a bound exactly at min_bb_size, a union exactly at the floor;
  * the sign of an L1 residual and of (centre prediction - target) is that of the fp32 difference, zero gives gradient 0;
  * the arg-max is the first maximum of the fp32 logits, labels outside [0, C) are ignored, the accuracy is hits / ALL rows.

`mistake=` evaluates a deliberately wrong variant (test_loss_heads_rule.py::test_deliberate_mistakes_fail_a_named_case).
"""
import numpy as np
import torch

import _loss_rule as R

VALUE_NAMES = R.VALUE_NAMES + ('iou_loss', 'center_score_loss', 'center_scores_correlation')
HEADS = ('off', 'bnd', 'sc', 'cs', 'sem')
W_IOU, W_CS = 0.9, 0.6
ROW_VALUE_NAMES = ('weighted_loss', 'loss', 'acc')
MISTAKES = ('iou_grad_through_clamp', 'plus_eps', 'centre_not_detached', 'ignored_in_n_valid', 'last_max', 'acc_over_valid')


def _prod(s):
    return (s[:, 0] * s[:, 1]) * s[:, 2]


def corners32(case, rows):
    """fp32 corners in torch's order: (predicted [lo | hi] with clamped bounds, true [lo | hi], bound-is-free mask)."""
    min_bb = torch.tensor(case['min_bb'], dtype=torch.float32)
    loc, off, bnd = case['loc'][rows], case['off'][rows], case['bnd'][rows]
    pc, gc = off + loc, case['gt_off'][rows] + loc
    pb = torch.clamp(bnd, min=float(min_bb))
    gb = case['gt_bnd'][rows]
    return torch.cat((pc - pb, pc + pb), 1), torch.cat((gc - gb, gc + gb), 1), bnd >= min_bb


def iou_term(case, rows, off, bnd, dtype, mistake=None):
    """mean over `rows` of 1 - IoU(predicted box, true box); `off` / `bnd` are the (S, 3) leaves of `dtype`."""
    eps = float(np.float32(1e-6))
    min_bb = float(np.float32(case['min_bb']))
    p32, g32, free = corners32(case, rows)
    cst = {k: case[k][rows].to(dtype) for k in ('gt_off', 'gt_bnd', 'loc')}
    pb = bnd[rows]
    if mistake == 'iou_grad_through_clamp':
        pb = pb + (torch.clamp(pb, min=min_bb) - pb).detach()                # the clamped value, the unclamped gradient
    else:
        pb = torch.where(free, pb, torch.full_like(pb, min_bb))
    pc, gc = off[rows] + cst['loc'], cst['gt_off'] + cst['loc']
    p = torch.cat((pc - pb, pc + pb), 1)
    g = torch.cat((gc - cst['gt_bnd'], gc + cst['gt_bnd']), 1)
    share = lambda a, b: ((a > b).to(dtype) + 0.5 * (a == b).to(dtype))      # of the gradient of max(a, b) that goes to a
    wl, wh = share(p32[:, :3], g32[:, :3]), share(-p32[:, 3:], -g32[:, 3:])
    lo = wl * p[:, :3] + (1 - wl) * g[:, :3]
    hi = wh * p[:, 3:] + (1 - wh) * g[:, 3:]
    side32 = torch.minimum(p32[:, 3:], g32[:, 3:]) - torch.maximum(p32[:, :3], g32[:, :3])
    side = torch.where(side32 >= 0, hi - lo, torch.zeros_like(lo))
    inter = _prod(side)
    union = _prod(p[:, 3:] - p[:, :3]) + _prod(g[:, 3:] - g[:, :3]) - inter
    union32 = _prod(p32[:, 3:] - p32[:, :3]) + _prod(g32[:, 3:] - g32[:, :3]) - _prod(side32.clamp(min=0))
    if mistake == 'plus_eps':
        den = union + eps
    else:
        den = torch.where(union32 >= eps, union, torch.full_like(union, eps))
    return (1.0 - inter / den).mean()


def heads_rule(case, dtype=torch.float64, mistake=None):
    """-> dict(values: 11 floats in the order of VALUE_NAMES, argmax, n_correct, grads: head -> tensor of `dtype` or None).
    `case`: a _loss_rule case plus 'cs' ((S, 1) centre head or None), 'use_iou', 'w_iou', 'w_cs'."""
    base = R.loss_rule(case, dtype)                                           # offsets, bounds, scores, segment semantics
    w_iou, w_cs = float(np.float32(case['w_iou'])), float(np.float32(case['w_cs']))
    S, fg = case['off'].shape[0], case['fg']
    rows = torch.nonzero(fg).reshape(-1) if fg is not None else torch.arange(S)
    off = case['off'].detach().to(dtype).requires_grad_(True)
    bnd = case['bnd'].detach().to(dtype).requires_grad_(True)
    cs = case['cs'].detach().to(dtype).requires_grad_(True) if case['cs'] is not None else None
    vals = list(base['values']) + [0.0, 0.0, 0.0]
    extra = 0.0
    if case['use_iou']:
        l_iou = iou_term(case, rows, off, bnd, dtype, mistake)
        extra = extra + w_iou * l_iou
        vals[8] = float(l_iou.detach())
    if cs is not None:
        sign = torch.sign(case['off'][rows] - case['gt_off'][rows]).to(dtype)
        target = (sign * (off[rows] - case['gt_off'][rows].to(dtype))).sum(1)
        if mistake != 'centre_not_detached':
            target = target.detach()
        t32 = torch.sum(torch.abs(case['off'][rows] - case['gt_off'][rows]), 1)
        p = cs.reshape(-1)[rows]
        l_cs = (torch.sign(case['cs'].reshape(-1)[rows] - t32).to(dtype) * (p - target)).mean()
        extra = extra + w_cs * l_cs
        vals[9], vals[10] = float(l_cs.detach()), float(R.pearson(target.detach(), p.detach()))
    grads = dict(base['grads'], cs=None)
    if torch.is_tensor(extra):
        extra.backward()
        vals[0] = vals[0] + float(extra.detach())
        for h, leaf in (('off', off), ('bnd', bnd)):
            if leaf.grad is not None:
                grads[h] = grads[h] + leaf.grad
        if cs is not None:
            grads['cs'] = cs.grad if cs.grad is not None else torch.zeros_like(cs)
    return {'values': vals, 'argmax': base['argmax'], 'n_correct': base['n_correct'], 'grads': grads}


def rows_rule(case, dtype=torch.float64, mistake=None):
    """Cross entropy over rows.  case: 'z' (N, C) fp32, 't' (N,) int64, 'weight'.  -> dict(values (weight * loss, loss, acc),
    argmax, n_correct, grad (N, C) of weight * loss)."""
    z32, t, w = case['z'], case['t'], float(np.float32(case['weight']))
    N, C = z32.shape
    z = z32.detach().to(dtype).requires_grad_(True)
    valid = (t >= 0) & (t < C)
    t_ign = torch.where(valid, t, torch.full_like(t, -100))
    if mistake == 'ignored_in_n_valid':
        loss = torch.nn.functional.cross_entropy(z, t_ign, ignore_index=-100, reduction='sum') / N
    else:
        loss = torch.nn.functional.cross_entropy(z, t_ign, ignore_index=-100)
    argmax = R.first_argmax(z32)
    if mistake == 'last_max':
        argmax = C - 1 - R.first_argmax(z32.flip(1))
    n_correct = int((argmax == t).sum())
    acc = n_correct / (int(valid.sum()) if mistake == 'acc_over_valid' else N)
    (w * loss).backward()
    return {'values': [w * float(loss.detach()), float(loss.detach()), acc], 'argmax': argmax, 'n_correct': n_correct,
            'grad': z.grad}


# ------------------------------------------------------------------ segment cases
def ex_case(S, seed=0, iou=True, centre=True, scores=True, sem=True, fg_frac=0.6, min_bb=R.MIN_BB):
    c = R.make_case(S, seed=seed, scores=scores, sem=sem, fg_frac=fg_frac, min_bb=min_bb)
    g = torch.Generator().manual_seed(7000 + seed)
    l1 = (c['off'] - c['gt_off']).abs().sum(1, keepdim=True)
    c['cs'] = (l1 + torch.randn(S, 1, generator=g) * 0.1) if centre else None   # near its target, on both sides of it
    c.update(use_iou=iou, w_iou=W_IOU, w_cs=W_CS)
    return c


def _dy(*rows):
    return torch.tensor(rows, dtype=torch.float32)


def dyadic_boxes():
    """Hand-built rows of dyadic numbers (exact in fp32 and fp64 alike; min_bb 0.25, location 0): per row a name, the predicted
    (offset, bound) and the true (offset, bound).  One foreground row each, no mask."""
    q = 0.25
    rows = [
        # name,            pred off,        pred bnd,          gt off,          gt bnd
        ('identical',      (0., 0., 0.),    (1., 1., 1.),      (0., 0., 0.),    (1., 1., 1.)),       # all six corners tie, IoU 1
        ('contained',      (0., 0., 0.),    (.5, .5, .5),      (0., 0., 0.),    (1., 1., 1.)),       # pred inside gt
        ('containing',     (0., 0., 0.),    (2., 2., 2.),      (.25, 0., 0.),   (1., 1., 1.)),       # gt inside pred
        ('touching',       (2., 0., 0.),    (1., 1., 1.),      (0., 0., 0.),    (1., 1., 1.)),       # side 0 exactly zero
        ('disjoint',       (4., 0., 0.),    (1., 1., 1.),      (0., 0., 0.),    (1., 1., 1.)),       # side 0 negative
        ('lo_corner_tie',  (.5, 0., 0.),    (1.5, 1., .5),     (0., 0., 0.),    (1., 2., 1.)),       # pred lo x == gt lo x == -1
        ('hi_corner_tie',  (-.5, 0., 0.),   (1.5, 1., .5),     (0., 0., 0.),    (1., 2., 1.)),       # pred hi x == gt hi x == +1
        ('bound_at_floor', (.5, 0., 0.),    (q, 1., 1.),       (0., 0., 0.),    (1., 1., 1.)),       # bound == min_bb: free
        ('bound_below',    (.5, 0., 0.),    (.125, 1., 1.),    (0., 0., 0.),    (1., 1., 1.)),       # clamped: no gradient
        ('bound_negative', (.5, 0., 0.),    (-1., 1., 1.),     (0., 0., 0.),    (1., 1., 1.)),
    ]
    return rows


def dyadic_case(row, min_bb=0.25):
    name, po, pb, go, gb = row
    return {'off': _dy(po), 'bnd': _dy(pb), 'gt_off': _dy(go), 'gt_bnd': _dy(gb), 'loc': torch.zeros(1, 3), 'fg': None,
            'sc': None, 'sem': None, 'gt_sem': None, 'cs': None, 'weights': R.WEIGHTS, 'min_bb': min_bb,
            'use_iou': True, 'w_iou': W_IOU, 'w_cs': W_CS}


def _stack(cases):
    out = dict(cases[0])
    for k in ('off', 'bnd', 'gt_off', 'gt_bnd', 'loc'):
        out[k] = torch.cat([c[k] for c in cases])
    return out


def _box_kinds():
    """All the dyadic rows in one case of 10 rows, shifted by a dyadic location (the corners stay exact)."""
    c = _stack([dyadic_case(r) for r in dyadic_boxes()])
    c['loc'] = torch.full((len(dyadic_boxes()), 3), 1.5)
    c['cs'] = _dy(*[[0.5 * i] for i in range(len(dyadic_boxes()))])
    return c


def _union_floor():
    """min_bb_size = 0 and zero-volume boxes: the union is below, exactly at and above the floor."""
    e = float(np.float32(1e-6))
    c = _stack([dyadic_case(r, min_bb=0.0) for r in (
        ('flat_both',   (0., 0., 0.), (0., 1., 1.),  (0., 0., 0.), (0., 1., 1.)),     # both volumes 0: union 0 < floor
        ('point_pred',  (0., 0., 0.), (0., 0., 0.),  (0., 0., 0.), (0., 0., 0.)),
        ('neg_bound',   (0., 0., 0.), (-1., 1., 1.), (0., 0., 0.), (0., 1., 1.)),     # clamped at 0: flat, and no gradient
        ('tiny_inside', (0., 0., 0.), (2. ** -8, 2. ** -8, 2. ** -8), (0., 0., 0.), (2. ** -9, 2. ** -9, 2. ** -9)),  # 2^-21 < 1e-6
        ('at_floor',    (0., 0., 0.), (.5, .5, .5),  (8., 8., 8.), (0., 1., 1.)),     # placeholder, replaced below
        ('normal',      (0., 0., 0.), (.5, .5, .5),  (0., 0., 0.), (1., 1., 1.)),
    )])
    # a union of exactly float32(1e-6): pred box 1 x 1 x e (bounds .5, .5, e/2), true box flat and far away
    c['bnd'][4] = torch.tensor([0.5, 0.5, e / 2])
    c['cs'] = None
    return c


def _centre_zero():
    """Centre predictions exactly on their target (gradient 0) and exactly zero L1 residuals.  The rows that tie are made of
    eighths: residuals and their sum are exact in fp32 whatever the order of the three additions."""
    c = ex_case(257, seed=61, iou=False)
    rows = torch.nonzero(c['fg']).reshape(-1)
    tie = rows[::2]
    g = torch.Generator().manual_seed(61)
    c['gt_off'][tie] = torch.round(c['gt_off'][tie] * 8) / 8
    c['off'][tie] = c['gt_off'][tie] + torch.randint(-3, 4, (len(tie), 3), generator=g) / 8.0     # some residuals exactly 0
    c['off'][tie[1]] = c['gt_off'][tie[1]]                                    # a whole row: target 0
    c['cs'][tie] = torch.sum(torch.abs(c['off'][tie] - c['gt_off'][tie]), 1, keepdim=True)        # prediction == target
    return c


def _centre_const():
    c = ex_case(257, seed=62, iou=False)
    c['cs'][:] = 0.75
    return c


def _small_bounds():
    c = ex_case(257, seed=63)
    g = torch.Generator().manual_seed(63)
    c['bnd'] = torch.randn(257, 3, generator=g) * 0.05 + R.MIN_BB
    c['bnd'][5, 1] = float(np.float32(R.MIN_BB))
    c['bnd'][6, 0] = -0.3
    c['fg'][5] = c['fg'][6] = True
    return c


def _empty_block():
    c = ex_case(1031, seed=64)
    c['fg'][256:512] = False
    return c


def _one_fg():
    c = ex_case(1031, seed=65)
    c['fg'][:] = False
    c['fg'][1027] = True
    return c


def _disjoint():
    c = ex_case(257, seed=66, centre=False)       # (a target of 30 m +- rounding has no variance worth a correlation)
    c['off'] = c['gt_off'] + 10.0
    return c


SEG_CASES = {}
for _S in (1, 255, 256, 257, 1031):
    SEG_CASES['S%d' % _S] = (lambda S=_S: ex_case(S, seed=S))
    SEG_CASES['S%d_no_mask' % _S] = (lambda S=_S: ex_case(S, seed=700 + S, fg_frac=None))
SEG_CASES.update({
    'iou_alone': lambda: ex_case(257, seed=51, centre=False, scores=False, sem=False),
    'centre_alone': lambda: ex_case(257, seed=52, iou=False, scores=False, sem=False),
    'centre_inactive': lambda: ex_case(257, seed=53, centre=False),          # early epoch: the caller passes no centre head
    'box_kinds': _box_kinds, 'union_floor': _union_floor, 'small_bounds': _small_bounds, 'disjoint': _disjoint,
    'centre_zero': _centre_zero, 'centre_const': _centre_const, 'empty_block': _empty_block, 'one_fg_last_block': _one_fg,
})
DYADIC = ('box_kinds', 'union_floor')
MARGIN = 2e-6          # between competing corners, of a side from 0: four fp32 ulps of a 4 m coordinate (a corner is two roundings)


def decision_margins(c):
    """Smallest distance of every discrete IoU decision from its tie, over the foreground rows, ties themselves left out:
    (corner vs corner, intersection side vs 0, bound vs min_bb, union vs floor) and the number of exact ties of each."""
    S, fg = c['off'].shape[0], c['fg']
    rows = torch.nonzero(fg).reshape(-1) if fg is not None else torch.arange(S)
    p, g, _ = corners32(c, rows)
    p, g = p.double(), g.double()
    gaps = {'corner': (p - g).abs().reshape(-1),
            'side': (torch.minimum(p[:, 3:], g[:, 3:]) - torch.maximum(p[:, :3], g[:, :3])).abs().reshape(-1),
            'bound': (c['bnd'][rows].double() - float(np.float32(c['min_bb']))).abs().reshape(-1)}
    side = (torch.minimum(p[:, 3:], g[:, 3:]) - torch.maximum(p[:, :3], g[:, :3])).clamp(min=0)
    union = _prod(p[:, 3:] - p[:, :3]) + _prod(g[:, 3:] - g[:, :3]) - _prod(side)
    gaps['union'] = (union - float(np.float32(1e-6))).abs()
    out = {}
    for k, v in gaps.items():
        out[k] = (float(v[v > 0].min()) if bool((v > 0).any()) else float('inf'), int((v == 0).sum()))
    return out


def check_seg_preconditions(name, c):
    S, fg = c['off'].shape[0], c['fg']
    rows = torch.nonzero(fg).reshape(-1) if fg is not None else torch.arange(S)
    m = decision_margins(c)
    if name in DYADIC:
        for k in ('off', 'bnd', 'gt_off', 'gt_bnd', 'loc'):                   # dyadic: every corner is exact in fp32
            if name == 'box_kinds':
                assert torch.equal(c[k] * 8, torch.round(c[k] * 8)), k
    else:
        # no tie, and every decision far enough from one that fp32 and fp64 corners take the same branch
        assert m['corner'][1] == 0 and m['side'][1] == 0 and m['union'][1] == 0, m
        assert m['corner'][0] > MARGIN and m['side'][0] > MARGIN and m['union'][0] > 1e-4, m
        assert m['bound'][0] > 1e-6 or name == 'small_bounds', m
    if name.startswith('S'):
        assert S == int(name[1:].split('_')[0]) and c['use_iou'] and c['cs'] is not None and c['sc'] is not None
        assert (fg is None) == name.endswith('no_mask')
    elif name == 'iou_alone':
        assert c['use_iou'] and c['cs'] is None and c['sc'] is None and c['sem'] is None
    elif name == 'centre_alone':
        assert not c['use_iou'] and c['cs'] is not None and c['sc'] is None and c['sem'] is None
    elif name == 'centre_inactive':
        assert c['use_iou'] and c['cs'] is None and c['sc'] is not None
    elif name == 'box_kinds':
        p, g, free = corners32(c, rows)
        side = torch.minimum(p[:, 3:], g[:, 3:]) - torch.maximum(p[:, :3], g[:, :3])
        names = [r[0] for r in dyadic_boxes()]
        at = lambda n: names.index(n)
        assert torch.equal(p[at('identical')], g[at('identical')])
        assert bool((side[at('touching')] == 0).any()) and bool((side[at('disjoint')] < 0).any())
        assert bool((p[at('contained'), :3] > g[at('contained'), :3]).all()) and bool((p[at('contained'), 3:] < g[at('contained'), 3:]).all())
        assert bool((p[at('containing'), :3] < g[at('containing'), :3]).all()) and bool((p[at('containing'), 3:] > g[at('containing'), 3:]).all())
        assert p[at('lo_corner_tie'), 0] == g[at('lo_corner_tie'), 0] and p[at('hi_corner_tie'), 3] == g[at('hi_corner_tie'), 3]
        assert c['bnd'][at('bound_at_floor'), 0] == c['min_bb'] and bool(free[at('bound_at_floor')].all())
        assert not bool(free[at('bound_below'), 0]) and not bool(free[at('bound_negative'), 0])
    elif name == 'union_floor':
        assert c['min_bb'] == 0.0
        p, g, _ = corners32(c, rows)
        side = (torch.minimum(p[:, 3:], g[:, 3:]) - torch.maximum(p[:, :3], g[:, :3])).clamp(min=0)
        u = _prod(p[:, 3:] - p[:, :3]) + _prod(g[:, 3:] - g[:, :3]) - _prod(side)
        e = float(np.float32(1e-6))
        assert bool((u[:3] == 0).all()) and 0 < float(u[3]) < e and float(u[4]) == e and float(u[5]) > e, u
    elif name == 'small_bounds':
        b, floor = c['bnd'][rows], float(np.float32(c['min_bb']))
        assert bool((b < 0).any()) and bool((b < floor).any()) and bool((b > floor).any()) and bool((b == floor).any())
    elif name == 'disjoint':
        p, g, _ = corners32(c, rows)
        assert bool((p[:, :3] - g[:, 3:] > 1.0).all())
    elif name == 'centre_zero':
        t32 = torch.sum(torch.abs(c['off'] - c['gt_off']), 1)[rows]
        d = c['cs'].reshape(-1)[rows] - t32
        assert int((d == 0).sum()) >= 10 and bool((d > 0).any()) and bool((d < 0).any()) and bool((t32 == 0).any())
        assert int(((c['off'] == c['gt_off'])[rows]).sum()) >= 10
    elif name == 'centre_const':
        assert int(torch.unique(c['cs']).numel()) == 1 and float(c['cs'][0]) != 0
    elif name == 'empty_block':
        assert S == 1031 and not bool(fg[256:512].any()) and all(bool(fg[b:b + 256].any()) for b in (0, 512, 768, 1024))
    elif name == 'one_fg_last_block':
        assert S == 1031 and int(fg.sum()) == 1 and int(rows[0]) >= 1024
    else:
        raise AssertionError('no precondition written for case %s' % name)


# ------------------------------------------------------------------ row cases
def rows_case(N, C, seed=0, labels='valid', spread=3.0, weight=0.9):
    g = torch.Generator().manual_seed(9000 + seed)
    z = torch.randn(N, C, generator=g) * spread
    t = torch.randint(0, C, (N,), generator=g)
    if labels == 'mixed':
        t[::3] = -100
        t[1::7] = C
        t[2::11] = C + 5
        t[3::13] = -1
    elif labels == 'none':
        t[:] = -100
        t[::4] = C
    return {'z': z, 't': t, 'weight': weight}


def _row_ties():
    c = rows_case(257, 13, seed=70)
    z = c['z']
    top = float(z.max()) + 1.0
    for i, r in enumerate(range(0, 257, 4)):
        a = i % 12
        b = a + 1 + (i % (12 - a))
        z[r, a] = z[r, b] = top
    z[3] = 0.25
    c['t'][0] = 0
    c['t'][4] = int(R.first_argmax(z[4:5])[0])
    c['t'][8] = 12 - int(R.first_argmax(z[8:9].flip(1))[0])
    return c


def _row_wide():
    c = rows_case(257, 13, seed=71, labels='mixed')
    g = torch.Generator().manual_seed(71)
    c['z'] = torch.rand(257, 13, generator=g) * 160 - 80
    c['z'][0, 0], c['z'][0, 1] = 80.0, -80.0
    return c


ROW_SIZES = (1, 63, 64, 65, 255, 256, 257, 4099)
ROW_CLASSES = (1, 2, 13, 20, 28)
ROW_CASES = {}
for _N in ROW_SIZES:
    ROW_CASES['N%d' % _N] = (lambda N=_N: rows_case(N, 13, seed=N, labels='mixed' if N > 1 else 'valid'))
for _C in ROW_CLASSES:
    ROW_CASES['C%d' % _C] = (lambda C=_C: rows_case(257, C, seed=200 + C, labels='mixed'))
ROW_CASES.update({
    'labels_valid': lambda: rows_case(257, 13, seed=72), 'labels_mixed': lambda: rows_case(257, 13, seed=73, labels='mixed'),
    'labels_none': lambda: rows_case(257, 13, seed=74, labels='none'), 'ties': _row_ties, 'wide_range': _row_wide,
})
BIG_ROWS = 1048577


def big_rows_case():
    """The per-voxel head at S3DIS size: 1 048 577 x 13, 4097 partial slots, a few percent of the labels ignored."""
    c = rows_case(BIG_ROWS, 13, seed=99)
    c['t'][::29] = -100
    return c


def check_row_preconditions(name, c):
    z, t = c['z'], c['t']
    N, C = z.shape
    valid = (t >= 0) & (t < C)
    if name.startswith('N'):
        assert N == int(name[1:]) and C == 13
    elif name.startswith('C'):
        assert C == int(name[1:]) and N == 257 and 0 < int(valid.sum()) < N
    elif name == 'labels_valid':
        assert bool(valid.all())
    elif name == 'labels_mixed':
        assert 0 < int(valid.sum()) < N and bool((t == -100).any()) and bool((t == C).any()) and bool((t > C).any()) \
            and bool((t == -1).any())
    elif name == 'labels_none':
        assert int(valid.sum()) == 0 and bool((t >= C).any())
    elif name == 'ties':
        k = (z == z.max(1, keepdim=True).values).sum(1)
        first, last = R.first_argmax(z), C - 1 - R.first_argmax(z.flip(1))
        assert int((k == 2).sum()) >= 20 and int((k == C).sum()) == 1
        assert bool((t[k > 1] == first[k > 1]).any()) and bool((t[k > 1] == last[k > 1]).any())
    elif name == 'wide_range':
        assert float(z.max()) == 80 and float(z.min()) == -80 and 0 < int(valid.sum()) < N
    elif name == 'big':
        assert N == BIG_ROWS and C == 13 and (N + 255) // 256 == 4097 and 0 < int((~valid).sum()) < N // 20
    else:
        raise AssertionError('no precondition written for case %s' % name)
