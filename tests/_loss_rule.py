"""Plain torch restatement, on the CPU, of the loss terms `detection_loss_kernel` (box2mask_amd/csrc/nms.hip) fuses: the
reference's Model.compute_loss_detection for the configurations Model._fused_losses accepts (models/model.py:62-88 L1 offset
and bounds, :133-176 IoU-target score loss, :194-210 semantics), plus the seeded case generators shared by
tests/test_loss_rule.py (CPU: the rule against the reference's own numbers, the cases against their preconditions) and
tests/test_gpu_loss.py (the kernel against the rule).

`loss_rule(case, dtype)` widens the fp32 arrays to `dtype` and evaluates the formulas there; gradients come from autograd.
With dtype=float64 it is the reference value; with dtype=float32 the same formulas are the yardstick the kernel's error is
measured with (`bound`).  Every discrete decision is taken from the fp32 inputs, so the two evaluations cannot disagree on a
branch: the sign of an L1 residual comes from the fp32 difference, the bounds are clamped at float32(min_bb_size), the union's
1e-6 is float32(1e-6), the arg-max is the first maximum of the fp32 logits, labels outside [0, C) are ignored.
"""
import numpy as np
import torch

VALUE_NAMES = ('optimization_loss', 'offset_loss', 'bounds_loss', 'bb_score_loss', 'bb_target_scores',
               'bb_scores_correlation', 'semantics_loss', 'semantics_acc')
HEADS = ('off', 'bnd', 'sc', 'sem')
MIN_BB = 0.04                                       # scannet_config().min_bb_size
WEIGHTS = (1.0, 0.5, 0.7, 1.3)                      # offsets, bounds, scores, semantics: all different on purpose


def first_argmax(z):
    """Index of the FIRST maximum of every row, spelled out (no reliance on how torch.argmax breaks ties)."""
    m = z == z.max(1, keepdim=True).values
    idx = torch.arange(z.shape[1]).expand_as(m)
    return torch.where(m, idx, torch.full_like(idx, z.shape[1])).min(1).values


def pearson(a, b):
    """model._pearsonr in the dtype of its inputs: centred sums, zero variance gives 0."""
    a = a - a.mean()
    b = b - b.mean()
    return (a * b).sum() / torch.sqrt((a * a).sum() * (b * b).sum()).clamp_min(1e-300 if a.dtype == torch.float64 else 1e-37)


def loss_rule(case, dtype=torch.float64):
    """-> dict(values: 8 Python floats in the order of VALUE_NAMES (0.0 for an absent head's slots), argmax: (S,) int64 or None,
    grads: dict head -> (S, width) tensor of `dtype` or None, n_correct: int or None)."""
    w = [float(np.float32(v)) for v in case['weights']]             # the C entry receives floats
    min_bb = float(np.float32(case['min_bb']))
    eps = float(np.float32(1e-6))
    S = case['off'].shape[0]
    fg = case['fg']
    rows = torch.nonzero(fg).reshape(-1) if fg is not None else torch.arange(S)
    lead = {h: (case[h].detach().to(dtype).requires_grad_(True) if case[h] is not None else None) for h in HEADS}
    cst = {k: case[k].to(dtype) for k in ('gt_off', 'gt_bnd', 'loc')}
    vals = [0.0] * 8

    def l1(pred, gt, pred32, gt32):                  # model.py:70-71, 84-85: mean over rows of the summed |difference|
        sign = torch.sign(pred32[rows] - gt32[rows]).to(dtype)       # decided in fp32; an exactly zero residual has gradient 0
        return (sign * (pred[rows] - gt[rows])).sum(1).mean()
    off_loss = l1(lead['off'], cst['gt_off'], case['off'], case['gt_off'])
    bnd_loss = l1(lead['bnd'], cst['gt_bnd'], case['bnd'], case['gt_bnd'])
    total = w[0] * off_loss + w[1] * bnd_loss
    vals[1], vals[2] = float(off_loss.detach()), float(bnd_loss.detach())

    if lead['sc'] is not None:                       # model.py:139-176
        x = lead['sc'].reshape(-1)[rows]
        loc, g_off, g_bnd = cst['loc'][rows], cst['gt_off'][rows], cst['gt_bnd'][rows]
        p_off = lead['off'].detach()[rows]
        p_bnd = torch.clamp(lead['bnd'].detach()[rows], min=min_bb)
        gc, pc = g_off + loc, p_off + loc
        a = torch.cat((gc - g_bnd, gc + g_bnd), 1)                   # gt boxes, [min | max]
        b = torch.cat((pc - p_bnd, pc + p_bnd), 1)
        a_side, b_side = a[:, 3:] - a[:, :3], b[:, 3:] - b[:, :3]    # iou_nms.set_IOUs, in its order of operations
        i_side = torch.clamp(torch.minimum(a[:, 3:], b[:, 3:]) - torch.maximum(a[:, :3], b[:, :3]), min=0)
        prod = lambda s: (s[:, 0] * s[:, 1]) * s[:, 2]
        inter = prod(i_side)
        iou = (inter / (prod(a_side) + prod(b_side) - inter + eps)).detach()
        bce = torch.nn.functional.binary_cross_entropy_with_logits(x, iou)
        total = total + w[2] * bce
        vals[3], vals[4], vals[5] = float(bce.detach()), float(iou.mean()), float(pearson(iou, x.detach()))

    argmax = n_correct = None
    if lead['sem'] is not None:                      # model.py:196-209
        C = lead['sem'].shape[1]
        t = case['gt_sem']
        t_ign = torch.where((t >= 0) & (t < C), t, torch.full_like(t, -100))
        ce = torch.nn.functional.cross_entropy(lead['sem'], t_ign, ignore_index=-100)
        argmax = first_argmax(case['sem'])
        n_correct = int((argmax == t).sum())
        total = total + w[3] * ce
        vals[6], vals[7] = float(ce.detach()), n_correct / S
    vals[0] = float(total.detach())
    total.backward()
    grads = {h: (lead[h].grad if lead[h] is not None else None) for h in HEADS}
    for h in HEADS:
        if lead[h] is not None and grads[h] is None:                 # (a head the total does not depend on: none today)
            grads[h] = torch.zeros_like(lead[h])
    return {'values': vals, 'argmax': argmax, 'grads': grads, 'n_correct': n_correct}


def n_fg(case):
    return int(case['fg'].sum()) if case['fg'] is not None else case['off'].shape[0]


def n_valid(case):
    if case['sem'] is None:
        return None
    t = case['gt_sem']
    return int(((t >= 0) & (t < case['sem'].shape[1])).sum())


# ------------------------------------------------------------------ the bound
def ulp32(scale):
    return float(np.spacing(np.float32(abs(scale)))) if np.isfinite(scale) else 0.0


def bound(q32, q64):
    """(kernel error allowed, scale): twice the error of the fp32 evaluation against the fp64 one plus four fp32 ulps of the
    quantity's scale -- |value| for a scalar, the largest magnitude for an array."""
    q32 = torch.as_tensor(q32, dtype=torch.float64).reshape(-1)
    q64 = torch.as_tensor(q64, dtype=torch.float64).reshape(-1)
    fin = torch.isfinite(q64)                        # (a NaN of the reference is matched as such by `error`, not measured)
    if not bool(fin.any()):
        return 0.0, 0.0
    scale = float(q64[fin].abs().max())
    yard = float((q32[fin] - q64[fin]).abs().max())
    return 2.0 * yard + 4.0 * ulp32(scale), scale


def ratio(e, b):
    return e / b if b > 0 else (0.0 if e == 0 else float('inf'))


def error(got, q64):
    """max |got - q64|; a NaN (or inf) must stand where the reference has one, and only there."""
    got = torch.as_tensor(got, dtype=torch.float64).reshape(-1)
    q64 = torch.as_tensor(q64, dtype=torch.float64).reshape(-1)
    odd = ~torch.isfinite(q64)
    if not torch.equal(odd, ~torch.isfinite(got)):
        return float('inf')
    if bool(odd.any()) and not all(str(float(a)) == str(float(b)) for a, b in zip(got[odd], q64[odd])):
        return float('inf')
    return float((got[~odd] - q64[~odd]).abs().max()) if bool((~odd).any()) else 0.0


# ------------------------------------------------------------------ seeded cases
def make_case(S, C=20, seed=0, scores=True, sem=True, fg_frac=0.6, weights=WEIGHTS, min_bb=MIN_BB):
    """Random rows of a plausible scene: locations within +-4 m, boxes of 0.1 .. 1 m half extent, predictions near the truth
    (IoUs spread over (0, 1)), about `fg_frac` of the rows foreground (None: no mask)."""
    g = torch.Generator().manual_seed(1000 + seed)
    r = lambda *s: torch.rand(*s, generator=g)
    n = lambda *s: torch.randn(*s, generator=g)
    loc = r(S, 3) * 8 - 4
    gt_off = n(S, 3) * 0.5
    gt_bnd = r(S, 3) * 0.9 + 0.1
    case = {'loc': loc, 'gt_off': gt_off, 'gt_bnd': gt_bnd,
            'off': gt_off + n(S, 3) * 0.15, 'bnd': gt_bnd + n(S, 3) * 0.1,
            'sc': n(S, 1) * 2 if scores else None, 'sem': n(S, C) * 3 if sem else None,
            'gt_sem': torch.randint(0, C, (S,), generator=g) if sem else None,
            'fg': None, 'weights': tuple(weights), 'min_bb': min_bb}
    if fg_frac is not None:
        fg = r(S) < fg_frac
        fg[int(torch.randint(0, S, (1,), generator=g))] = True       # never empty
        case['fg'] = fg
    return case


def _empty_block():
    c = make_case(1031, seed=30)
    c['fg'][256:512] = False
    return c


def _one_fg():
    c = make_case(1031, seed=31)
    c['fg'][:] = False
    c['fg'][1027] = True
    return c


def _small_bounds():
    c = make_case(257, seed=33)
    g = torch.Generator().manual_seed(33)
    c['bnd'] = torch.randn(257, 3, generator=g) * 0.05 + MIN_BB      # on both sides of min_bb_size, some negative
    c['bnd'][5, 1] = float(np.float32(MIN_BB))                       # exactly the floor
    c['bnd'][6, 0] = -0.3
    c['fg'][5] = c['fg'][6] = True
    return c


def _zero_residual():
    c = make_case(257, seed=34)
    rows = torch.nonzero(c['fg']).reshape(-1)[::3]
    c['off'][rows, 0] = c['gt_off'][rows, 0]
    c['off'][rows[::2], 2] = c['gt_off'][rows[::2], 2]
    c['bnd'][rows, 1] = c['gt_bnd'][rows, 1]
    c['off'][rows[0]] = c['gt_off'][rows[0]]                          # a whole row
    return c


def _labels_mixed():
    c = make_case(257, seed=35)
    t = c['gt_sem']
    t[::3] = -100
    t[1::7] = 20                                                     # == C
    t[2::11] = 25
    return c


def _labels_none():
    c = make_case(257, seed=36)
    c['gt_sem'][:] = -100
    c['gt_sem'][::4] = 20
    return c


def _ties():
    c = make_case(257, seed=37)
    z = c['sem']
    top = float(z.max()) + 1.0
    for i, r in enumerate(range(0, 257, 4)):
        a = i % 19
        b = a + 1 + (i % (19 - a))                                   # a < b <= 19
        z[r, a] = z[r, b] = top
        if i % 5 == 0:
            z[r, 19] = top                                           # three equal maxima
    z[3] = 0.25                                                      # a row of equal logits
    c['gt_sem'][0] = 0                                               # the first maximum of row 0 is the label ...
    c['gt_sem'][4] = int(first_argmax(z[4:5])[0])
    c['gt_sem'][8] = 19 - int(first_argmax(z[8:9].flip(1))[0])       # ... and here the last one is: not a hit
    return c


def _wide_range():
    c = make_case(257, seed=38)
    g = torch.Generator().manual_seed(38)
    c['sem'] = (torch.rand(257, 20, generator=g) * 200 - 100)
    c['sc'] = torch.where(torch.rand(257, 1, generator=g) < 0.5, -80.0, 80.0)
    c['sc'][::5] = torch.randn(52, 1, generator=g)
    return c


def _disjoint():
    c = make_case(257, seed=39)
    c['off'] = c['gt_off'] + 10.0                                    # predicted boxes 10 m off in every axis
    return c


def _equal_scores():
    c = make_case(257, seed=40)
    # (with this constant the uncentred fp64 sums  sum x^2 - (sum x)^2 / F  of the kernel's block tree leave +4.5e-13, not 0)
    c['sc'][:] = float(np.float32(3.9120001792907715))
    return c


def _heads(scores, sem):
    return lambda: make_case(257, seed=20, scores=scores, sem=sem)


CASES = {}
for _S in (1, 63, 64, 65, 255, 256, 257, 1031):
    CASES['S%d' % _S] = (lambda S=_S: make_case(S, seed=S))
for _sc in (False, True):
    for _sem in (False, True):
        CASES['heads_sc%d_sem%d' % (_sc, _sem)] = _heads(_sc, _sem)
for _C in (1, 13, 20):
    CASES['C%d' % _C] = (lambda C=_C: make_case(257, C=C, seed=50 + C))
CASES.update({
    'no_mask': lambda: make_case(257, seed=29, fg_frac=None),
    'empty_block': _empty_block, 'one_fg_last_block': _one_fg,
    'score_weight_off': lambda: make_case(257, seed=32, weights=(WEIGHTS[0], WEIGHTS[1], 0.0, WEIGHTS[3])),
    'small_bounds': _small_bounds, 'zero_residual': _zero_residual,
    'labels_mixed': _labels_mixed, 'labels_none': _labels_none,
    'ties': _ties, 'wide_range': _wide_range, 'disjoint': _disjoint, 'equal_scores': _equal_scores,
})


def check_preconditions(name, c):
    """Every generator proves the edge it is there for (tests/test_loss_rule.py runs this without a GPU)."""
    S = c['off'].shape[0]
    fg = c['fg']
    assert c['off'].dtype == torch.float32 and c['off'].shape == (S, 3) and c['bnd'].shape == (S, 3)
    assert n_fg(c) >= 1
    if name.startswith('S'):
        assert S == int(name[1:]) and c['sc'] is not None and c['sem'].shape[1] == 20
        assert fg is not None and (S < 63 or 0.4 < n_fg(c) / S < 0.8)
        if S > 256:
            assert all(bool(fg[b:b + 256].any()) for b in range(0, S, 256))       # every block contributes
    elif name.startswith('heads_'):
        assert S == 257 and (c['sc'] is not None) == ('sc1' in name) and (c['sem'] is not None) == ('sem1' in name)
    elif name.startswith('C'):
        assert S == 257 and c['sem'].shape[1] == int(name[1:]) and int(c['gt_sem'].max()) < int(name[1:])
    elif name == 'no_mask':
        assert fg is None and n_fg(c) == S == 257
    elif name == 'empty_block':
        assert S == 1031 and not bool(fg[256:512].any())
        assert all(bool(fg[b:b + 256].any()) for b in (0, 512, 768, 1024))
    elif name == 'one_fg_last_block':
        assert S == 1031 and n_fg(c) == 1 and int(torch.nonzero(fg)[0]) >= 1024
    elif name == 'score_weight_off':
        assert c['weights'][2] == 0.0 and c['sc'] is not None and c['weights'][0] != 0 and c['weights'][3] != 0
    elif name == 'small_bounds':
        b, floor = c['bnd'][fg], float(np.float32(c['min_bb']))
        assert bool((b < 0).any()) and bool((b < floor).any()) and bool((b > floor).any()) and bool((b == floor).any())
    elif name == 'zero_residual':
        zo, zb = (c['off'] == c['gt_off'])[fg], (c['bnd'] == c['gt_bnd'])[fg]
        assert int(zo.sum()) >= 10 and int(zb.sum()) >= 10 and bool(zo.all(1).any())
        assert bool((~zo).any()) and bool((~zb).any())
    elif name == 'labels_mixed':
        t = c['gt_sem']
        assert bool((t == -100).any()) and bool((t == 20).any()) and bool((t > 20).any())
        assert 0 < n_valid(c) < S
    elif name == 'labels_none':
        t = c['gt_sem']
        assert n_valid(c) == 0 and bool((t == -100).any()) and bool((t >= 20).any())
    elif name == 'ties':
        z = c['sem']
        k = (z == z.max(1, keepdim=True).values).sum(1)
        assert int((k == 2).sum()) >= 20 and int((k == 3).sum()) >= 5 and int((k == 20).sum()) == 1
        first = first_argmax(z)
        last = 19 - first_argmax(z.flip(1))
        tied = k > 1
        assert bool((first[tied] < last[tied]).all())
        # a hit only if the FIRST maximum is taken, and a miss only then
        assert bool((c['gt_sem'][tied] == first[tied]).any()) and bool((c['gt_sem'][tied] == last[tied]).any())
    elif name == 'wide_range':
        assert float(c['sem'].max()) > 95 and float(c['sem'].min()) < -95
        assert bool((c['sc'][fg] == 80).any()) and bool((c['sc'][fg] == -80).any())
    elif name == 'disjoint':
        lo_p = (c['off'] + c['loc']) - c['bnd'].clamp(min=c['min_bb'])
        hi_g = (c['gt_off'] + c['loc']) + c['gt_bnd']
        assert bool((lo_p - hi_g > 1.0).all())                                    # a metre apart: no rounding closes it
    elif name == 'equal_scores':
        assert int(torch.unique(c['sc']).numel()) == 1 and float(c['sc'][0]) != 0.0
    else:
        raise AssertionError('no precondition written for case %s' % name)
