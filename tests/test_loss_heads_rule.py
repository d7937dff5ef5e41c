"""The restatement of the IoU loss, the centre-score loss and the per-voxel cross entropy (tests/_loss_heads_rule.py) on the
CPU: against the reference's own numbers (tests/golden/losses.npz, cases b, c, d, with the tolerances of
test_gpu_net.py::test_losses_match_reference_golden), every named case of tests/test_gpu_loss_heads.py against the edge it
claims to hold, torch autograd's conventions at ties on inputs of dyadic numbers, and six deliberate mistakes that each fail a
named case by more than the bound the GPU test uses.  No GPU."""
import os

import numpy as np
import pytest
import torch

import _loss_heads_rule as H
import _loss_rule as R

HEAD_KEYS = {'off': 'mlp_offsets', 'bnd': 'mlp_bounds', 'sc': 'mlp_bb_scores', 'cs': 'mlp_center_scores', 'sem': 'mlp_semantics'}


def golden_case(golden_dir, which):
    """Case b, c or d of losses.npz as a _loss_heads_rule case (+ its per-voxel rows case, d only) under the configuration
    test_losses_match_reference_golden gives it."""
    from box2mask_amd import synth
    from box2mask_amd.config import scannet_config
    g = np.load(os.path.join(golden_dir, 'losses.npz'))
    pre = 'loss_%s_' % which
    cfg = scannet_config(use_bb_iou_loss=(which == 'b'), loss_weight_center_scores=0.7, loss_weight_per_vox_semantics=0.9)
    t = lambda k: torch.from_numpy(g[pre + k])
    opt = lambda k: t(k) if pre + k in g.files else None
    epoch = int(g[pre + 'epoch'])
    id2idx = synth.scannet_tables()[1]
    w_sc = cfg.loss_weight_bb_scores if epoch >= cfg.mlp_bb_scores_start_epoch else 0.0
    sem = opt('pred_mlp_semantics')
    case = {'off': t('pred_mlp_offsets'), 'bnd': t('pred_mlp_bounds'), 'sc': t('pred_mlp_bb_scores'), 'sem': sem,
            'cs': opt('pred_mlp_center_scores'), 'gt_off': t('batch_gt_bb_offsets').float(),
            'gt_bnd': t('batch_gt_bb_bounds').float(), 'loc': t('batch_input_location').float(),
            'fg': t('batch_fg_instances').bool() if which != 'd' else None,          # d: the losses run over all segments
            'gt_sem': id2idx[t('batch_gt_semantics')].long() if sem is not None else None,
            'weights': (cfg.loss_weight_bb_offsets, cfg.loss_weight_bb_bounds, w_sc, cfg.loss_weight_semantics),
            'min_bb': cfg.min_bb_size, 'use_iou': which == 'b', 'w_iou': cfg.loss_weight_bb_iou, 'w_cs': cfg.loss_weight_center_scores}
    rows = None
    if which == 'd':
        rows = {'z': t('pred_mlp_per_vox_semantics'), 't': id2idx[t('batch_gt_per_vox_semantics')].long(),
                'weight': cfg.loss_weight_per_vox_semantics}
    return case, rows, g, pre


@pytest.mark.parametrize('which', ['b', 'c', 'd'])
def test_rule_matches_reference_golden(golden_dir, which):
    case, rows, g, pre = golden_case(golden_dir, which)
    out = H.heads_rule(case, torch.float64)
    got = dict(zip(H.VALUE_NAMES, out['values']))
    grads = {HEAD_KEYS[h]: v for h, v in out['grads'].items() if v is not None}
    if rows is not None:
        assert rows['z'].shape == (21829, 20)
        ro = H.rows_rule(rows, torch.float64)
        got['optimization_loss'] += ro['values'][0]
        got['per_vox_semantics_loss'], got['per_vox_semantics_acc'] = ro['values'][1], ro['values'][2]
        grads['mlp_per_vox_semantics'] = ro['grad']
    assert {'b': 'iou_loss', 'c': 'center_score_loss', 'd': 'per_vox_semantics_loss'}[which] + '' in [k[len(pre):] for k in g.files]
    keys = [k[len(pre):] for k in g.files if k.startswith(pre) and not any(s in k for s in ('pred_', 'grad_', 'batch_', 'epoch'))]
    for k in keys:
        if k == 'semantics_mIoU':                                               # (iou_nms.semIOU: not a loss term)
            continue
        ref = float(g[pre + k])
        tol = 2e-4 if 'correlation' in k else 2e-5
        print('%s %-26s rule %.9g reference %.9g error %.2e' % (which, k, got[k], ref, abs(got[k] - ref)))
        assert abs(got[k] - ref) <= tol * max(1.0, abs(ref)), (k, got[k], ref)
    n = 0
    for k in g.files:
        if k.startswith(pre + 'grad_'):
            ref = torch.from_numpy(g[k])
            mine = grads[k[len(pre + 'grad_'):]].reshape(ref.shape).float()
            assert torch.allclose(mine, ref, rtol=1e-4, atol=1e-7), k
            n += 1
    assert n == {'b': 4, 'c': 5, 'd': 4}[which]
    if which == 'b':
        assert int(g[pre + 'epoch']) < 100 and case['weights'][2] == 0.0         # early epoch: the score weight is off
        assert float(grads['mlp_bb_scores'].abs().max()) == 0.0
    if which == 'c':
        assert float(grads['mlp_center_scores'].abs().max()) > 0


# ------------------------------------------------------------------ the cases hold their edges
@pytest.mark.parametrize('name', sorted(H.SEG_CASES))
def test_segment_case_holds_its_edge(name):
    c = H.SEG_CASES[name]()
    H.check_seg_preconditions(name, c)
    again = H.SEG_CASES[name]()
    for k, v in c.items():
        assert torch.equal(v, again[k]) if torch.is_tensor(v) else v == again[k], k
    o64, o32 = H.heads_rule(c, torch.float64), H.heads_rule(c, torch.float32)
    for h in H.HEADS:
        assert (o64['grads'][h] is None) == (c[h] is None), h
        if c[h] is not None and h != 'sem':
            # no branch differs between the two evaluations: the same entries are exactly zero
            assert torch.equal(o32['grads'][h] == 0, o64['grads'][h] == 0), h
    assert all(np.isfinite(x) for x in o64['values']) and all(np.isfinite(x) for x in o32['values'])
    v = dict(zip(H.VALUE_NAMES, o64['values']))
    if name == 'centre_inactive':
        assert o64['grads']['cs'] is None and v['center_score_loss'] == 0.0
    if name == 'centre_const':
        assert v['center_scores_correlation'] == 0.0 and v['center_score_loss'] > 0
        assert dict(zip(H.VALUE_NAMES, o32['values']))['center_scores_correlation'] == 0.0
    if name == 'centre_zero':
        fg = c['fg']
        tie = (c['cs'].reshape(-1) == torch.sum(torch.abs(c['off'] - c['gt_off']), 1)) & fg
        assert int(tie.sum()) >= 10 and float(o64['grads']['cs'][tie].abs().max()) == 0.0
        assert float(o64['grads']['cs'][fg & ~tie].abs().min()) > 0
    if name == 'disjoint':
        assert v['iou_loss'] == 1.0
        assert float((o64['grads']['off'] - R.loss_rule(c)['grads']['off']).abs().max()) == 0.0    # no IoU gradient at all
    if name == 'small_bounds':
        fg, floor = c['fg'], float(np.float32(c['min_bb']))
        l1 = R.loss_rule(c)['grads']['bnd']
        below = (c['bnd'] < floor) & fg[:, None]
        assert float((o64['grads']['bnd'] - l1)[below].abs().max()) == 0.0        # a clamped bound: the L1 gradient alone
        assert float((o64['grads']['bnd'] - l1)[5, 1].abs()) > 0                  # exactly at the floor: free
    if name == 'union_floor':
        assert v['iou_loss'] > 0 and all(bool(torch.isfinite(o64['grads'][h]).all()) for h in ('off', 'bnd'))
    if c['fg'] is not None and bool((~c['fg']).any()):
        for h in ('off', 'bnd', 'cs'):
            if c[h] is not None:
                assert float(o64['grads'][h][~c['fg']].abs().max()) == 0.0, h


@pytest.mark.parametrize('name', sorted(H.ROW_CASES))
def test_row_case_holds_its_edge(name):
    c = H.ROW_CASES[name]()
    H.check_row_preconditions(name, c)
    again = H.ROW_CASES[name]()
    assert torch.equal(c['z'], again['z']) and torch.equal(c['t'], again['t'])
    o64, o32 = H.rows_rule(c, torch.float64), H.rows_rule(c, torch.float32)
    assert torch.equal(o64['argmax'], o32['argmax']) and o64['n_correct'] == o32['n_correct']
    t, C = c['t'], c['z'].shape[1]
    ign = (t < 0) | (t >= C)
    if bool(ign.any()):
        assert float(o64['grad'][ign].abs().max()) == 0.0
    if name == 'labels_none':
        assert np.isnan(o64['values'][0]) and np.isnan(o64['values'][1]) and float(o64['grad'].abs().max()) == 0.0
    else:
        assert all(np.isfinite(x) for x in o64['values']) and bool(torch.isfinite(o64['grad']).all())
    if name == 'ties':
        assert not torch.equal(o64['argmax'], H.rows_rule(c, mistake='last_max')['argmax'])


def test_big_row_case_holds_its_edge():
    H.check_row_preconditions('big', H.big_rows_case())


# ------------------------------------------------------------------ ties: what torch autograd does
def _torch_iou_loss(po, pb, go, gb, loc, min_bb):
    """The reference's formulas as torch writes them (clamp / maximum / minimum), for autograd to differentiate."""
    pb = torch.clamp(pb, min=min_bb)
    pc, gc = po + loc, go + loc
    a_lo, a_hi, b_lo, b_hi = pc - pb, pc + pb, gc - gb, gc + gb
    side = (torch.minimum(a_hi, b_hi) - torch.maximum(a_lo, b_lo)).clamp(min=0)
    vol = lambda s: s[:, 0] * s[:, 1] * s[:, 2]
    inter = vol(side)
    union = vol(a_hi - a_lo) + vol(b_hi - b_lo) - inter
    return (1.0 - inter / torch.clamp(union, min=float(np.float32(1e-6)))).mean()


@pytest.mark.parametrize('name', ['box_kinds', 'union_floor'])
@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['fp64', 'fp32'])
def test_tie_conventions_are_torch_autograds(name, dtype):
    """On dyadic inputs (exact in both precisions, so fp32 and fp64 cannot disagree on a branch) the rule, which spells the
    conventions out, has the values and gradients torch autograd gives the formulas as written -- row by row."""
    c = H.SEG_CASES[name]()
    n = c['off'].shape[0]
    m = H.decision_margins(c)
    assert m['corner'][1] > 0 and m['side'][1] > 0 and (name != 'union_floor' or m['union'][1] == 1)   # the ties are there
    tol = 1e-13 if dtype == torch.float64 else 2e-6
    for r in range(n):
        one = {k: (v[r:r + 1] if torch.is_tensor(v) and v.shape[:1] == (n,) else v) for k, v in c.items()}
        one['cs'] = None
        off = one['off'].to(dtype).requires_grad_(True)
        bnd = one['bnd'].to(dtype).requires_grad_(True)
        ref = _torch_iou_loss(off, bnd, one['gt_off'].to(dtype), one['gt_bnd'].to(dtype), one['loc'].to(dtype),
                              float(np.float32(one['min_bb'])))
        ref.backward()
        o2, b2 = one['off'].to(dtype).requires_grad_(True), one['bnd'].to(dtype).requires_grad_(True)
        mine = H.iou_term(one, torch.arange(1), o2, b2, dtype)
        mine.backward()
        zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
        assert abs(float(mine.detach()) - float(ref.detach())) <= tol, (r, mine, ref)
        assert float((zero(o2) - zero(off)).abs().max()) <= tol * max(1.0, float(zero(off).abs().max())), (r, zero(o2), zero(off))
        assert float((zero(b2) - zero(bnd)).abs().max()) <= tol * max(1.0, float(zero(bnd).abs().max())), (r, zero(b2), zero(bnd))


def test_tie_conventions_spelled_out():
    """The four conventions as numbers, from torch autograd itself."""
    x = torch.tensor([1.0, 2.0], dtype=torch.float64, requires_grad=True)
    y = torch.tensor([1.0, 3.0], dtype=torch.float64, requires_grad=True)
    torch.maximum(x, y).sum().backward()
    assert x.grad.tolist() == [0.5, 0.0] and y.grad.tolist() == [0.5, 1.0]       # equal arguments: half each
    x.grad = y.grad = None
    torch.minimum(x, y).sum().backward()
    assert x.grad.tolist() == [0.5, 1.0] and y.grad.tolist() == [0.5, 0.0]
    z = torch.tensor([-1.0, 0.0, 1.0], dtype=torch.float64, requires_grad=True)
    torch.clamp(z, min=0.0).sum().backward()
    assert z.grad.tolist() == [0.0, 1.0, 1.0]                                    # exactly at the limit: the gradient passes
    # in the rule.  Identical boxes of half extent 1 (all six corners tie, inter = union = 8): half of every side's gradient goes
    # to the prediction, so d iou / d bound_j = (1/8 + 8/64) * 4 * (1/2 + 1/2) - (8/64) * 2 * 4 = 0 and the offsets get
    # +1/2 - 1/2 = 0: a convention that sent a tie's whole gradient to one side would leave both nonzero.
    # Touching boxes (one intersection side exactly 0): the clamp passes the gradient, d inter / d side = 2 * 2, so the offset
    # is pulled towards the true box although the IoU is 0; a clamp that blocked at its limit would leave no gradient at all.
    names = [r[0] for r in H.dyadic_boxes()]
    for kind, flat in (('identical', True), ('touching', False)):
        one = H.dyadic_case(H.dyadic_boxes()[names.index(kind)])
        off, bnd = one['off'].double().requires_grad_(True), one['bnd'].double().requires_grad_(True)
        H.iou_term(one, torch.arange(1), off, bnd, torch.float64).backward()
        assert (float(off.grad.abs().max()) == 0.0) == flat and (float(bnd.grad.abs().max()) == 0.0) == flat, (kind, off.grad, bnd.grad)
        if kind == 'touching':
            assert float(off.grad[0, 0]) > 0 and float(bnd.grad[0, 0]) < 0       # moving left / growing in x lowers the loss


# ------------------------------------------------------------------ deliberate mistakes
MISTAKES = [
    # mistake,                 kind,  case,           quantity
    ('iou_grad_through_clamp', 'seg', 'small_bounds', 'd_bnd'),
    ('plus_eps',               'seg', 'union_floor',  'iou_loss'),
    ('centre_not_detached',    'seg', 'S257',         'd_off'),
    ('ignored_in_n_valid',     'row', 'labels_mixed', 'loss'),
    ('last_max',               'row', 'ties',         'argmax'),
    ('acc_over_valid',         'row', 'labels_mixed', 'acc'),
]


@pytest.mark.parametrize('mistake,kind,name,quantity', MISTAKES, ids=[m[0] for m in MISTAKES])
def test_deliberate_mistakes_fail_a_named_case(mistake, kind, name, quantity):
    """Each wrong variant leaves the bound of tests/test_gpu_loss_heads.py (R.bound) in the named case and quantity."""
    assert mistake in H.MISTAKES
    if kind == 'seg':
        c = H.SEG_CASES[name]()
        o64, o32, bad = H.heads_rule(c), H.heads_rule(c, torch.float32), H.heads_rule(c, mistake=mistake)
        pick = (lambda o: o['grads'][quantity[2:]]) if quantity.startswith('d_') else (lambda o: o['values'][H.VALUE_NAMES.index(quantity)])
    else:
        c = H.ROW_CASES[name]()
        o64, o32, bad = H.rows_rule(c), H.rows_rule(c, torch.float32), H.rows_rule(c, mistake=mistake)
        if quantity == 'argmax':
            assert not torch.equal(bad['argmax'], o64['argmax']) and bad['n_correct'] != o64['n_correct']
            return
        pick = lambda o: o['values'][H.ROW_VALUE_NAMES.index(quantity)]
    b, _ = R.bound(pick(o32), pick(o64))
    e = R.error(pick(bad), pick(o64))
    print('%s: error %.3e, bound %.3e' % (mistake, e, b))
    assert e > 10 * b, (mistake, e, b)
