"""`detection_loss_kernel` (box2mask_amd/csrc/nms.hip: the whole ScanNet training loss, values and gradients, in one launch)
against the fp64 restatement of the reference's formulas in tests/_loss_rule.py, at the edges the one reference fixture
(test_gpu_net.py::test_losses_match_reference_golden, case a: 230 rows, one workgroup, everything present) does not reach:
several workgroups and the fp64 atomics between them, a workgroup without a foreground row, no mask at all, absent heads,
the score weight off, ignored labels (some, all), bounds below min_bb_size, exactly zero residuals, arg-max ties, one
foreground row, leading dimensions wider than the rows, the scaling by the incoming gradient, the no-autograd arg-max.

The bound is not a number picked in advance.  For every case and compared quantity the fp32 evaluation of the rule is held
against its fp64 evaluation on the CPU; the kernel's error against fp64 may be at most TWICE that plus FOUR fp32 ulps of
the quantity's scale (|value| of a scalar, the largest magnitude of a gradient array): the kernel forms the IoU in the fp32
order torch does and sums in fp64, so its error is the fp32 IoU's plus the rounding of w * (float)(1/F) and of its fp32
outputs.  Classes and hit counts are compared exactly.  `ratio` below = kernel error / that bound; every test prints it.

Worst ratios: NOT MEASURED on an MI355X yet -- no device could be had while these tests were written.  What stands in for
them: a numpy emulation of the kernel's arithmetic (fp32 where the kernel is fp32, its fp64 block tree and atomics) passes
every case of test_kernel_matches_rule with ratios of at most 0.54 (S1031: bb_scores_correlation); the same emulation of the
kernel before the zero-variance fix in detection_loss_final_kernel fails case equal_scores (correlation 6.7e-08 instead of 0).
The first run on a device prints the real figures (pytest -s); they belong here.
"""
import functools

import numpy as np
import pytest
import torch

import _loss_rule as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, fp64 evaluation, fp32 evaluation) of a named case: computed once on the CPU, shared, never modified."""
    case = R.CASES[name]()
    return case, R.loss_rule(case, torch.float64), R.loss_rule(case, torch.float32)


def device_args(case, wrap=lambda name, t: t.cuda().requires_grad_(True)):
    """The argument list of functional.detection_loss for a case; `wrap` places the head tensors."""
    heads = {h: (wrap(h, case[h]) if case[h] is not None else None) for h in R.HEADS}
    nv = R.n_valid(case)
    args = (heads['off'], heads['bnd'], heads['sc'], heads['sem'], case['gt_off'].cuda(), case['gt_bnd'].cuda(),
            case['loc'].cuda(), case['fg'].to(torch.uint8).cuda() if case['fg'] is not None else None,
            case['gt_sem'].cuda() if case['sem'] is not None else None, R.n_fg(case),
            torch.tensor([float(nv)], dtype=torch.float64).cuda() if nv is not None else None,
            tuple(float(w) for w in case['weights']), float(case['min_bb']))
    return heads, args


def run_kernel(case, scale=None):
    from box2mask_amd import functional as F
    heads, args = device_args(case)
    res, argmax = F.detection_loss(*args)
    (res[0] if scale is None else res[0] * scale).backward()
    torch.cuda.synchronize()
    return {'values': res.detach().cpu().numpy().copy(), 'argmax': argmax.cpu() if argmax is not None else None,
            'grads': {h: (t.grad.cpu() if t is not None and t.grad is not None else None) for h, t in heads.items()}}


def compare(tag, got, o64, o32, case):
    """Print the ratio of every compared quantity, then assert: values and gradients within the bound, classes exact."""
    rows, bad = [], []
    for i, k in enumerate(R.VALUE_NAMES):
        b, _ = R.bound(o32['values'][i], o64['values'][i])
        e = R.error(float(got['values'][i]), o64['values'][i])
        rows.append((k, e, b))
    for h in R.HEADS:
        if case[h] is None:
            if got['grads'][h] is not None:
                bad.append('a gradient for the absent head %s' % h)
            continue
        if got['grads'][h] is None:
            bad.append('no gradient for head %s' % h)
            continue
        b, _ = R.bound(o32['grads'][h], o64['grads'][h])
        rows.append(('d_' + h, R.error(got['grads'][h], o64['grads'][h]), b))
    for k, e, b in rows:
        print('%-18s %-22s error %.3e  bound %.3e  ratio %.3f' % (tag, k, e, b, R.ratio(e, b)))
        if not e <= b:
            bad.append('%s: error %.3e > bound %.3e' % (k, e, b))
    if case['sem'] is not None:
        S = case['sem'].shape[0]
        if not torch.equal(got['argmax'], o64['argmax']):
            bad.append('predicted classes differ in %d rows' % int((got['argmax'] != o64['argmax']).sum()))
        if np.float32(got['values'][7]) != np.float32(o64['n_correct'] / S):
            bad.append('semantics_acc * S = %r, expected %d' % (float(got['values'][7]) * S, o64['n_correct']))
    else:
        if got['argmax'] is not None:
            bad.append('predicted classes without a semantics head')
    assert not bad, (tag, bad)


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_kernel_matches_rule(name):
    case, o64, o32 = reference(name)
    got = run_kernel(case)
    v = dict(zip(R.VALUE_NAMES, (float(x) for x in got['values'])))
    g = got['grads']
    # what has to be EXACT, before the bounds
    if case['sc'] is None:
        assert v['bb_score_loss'] == 0.0 and v['bb_target_scores'] == 0.0 and v['bb_scores_correlation'] == 0.0
        assert g['sc'] is None
    if case['sem'] is None:
        assert v['semantics_loss'] == 0.0 and v['semantics_acc'] == 0.0 and g['sem'] is None and got['argmax'] is None
    if case['fg'] is not None and bool((~case['fg']).any()):
        bg = ~case['fg']
        for h in ('off', 'bnd', 'sc'):
            if case[h] is not None:
                assert float(g[h][bg].abs().max()) == 0.0, 'background rows have a %s gradient' % h
    if case['sem'] is not None:
        t, C = case['gt_sem'], case['sem'].shape[1]
        ign = (t < 0) | (t >= C)
        if bool(ign.any()):
            assert float(g['sem'][ign].abs().max()) == 0.0, 'ignored labels have a gradient'
    if name == 'score_weight_off':
        assert float(g['sc'].abs().max()) == 0.0
        assert v['bb_score_loss'] > 0 and v['bb_target_scores'] > 0 and v['bb_scores_correlation'] != 0.0
    if name == 'zero_residual':
        fg = case['fg']
        assert float(g['off'][fg][(case['off'] == case['gt_off'])[fg]].abs().max()) == 0.0
        assert float(g['bnd'][fg][(case['bnd'] == case['gt_bnd'])[fg]].abs().max()) == 0.0
    if name == 'labels_none':
        # fp64 torch: the mean over no rows is NaN, the gradient into the logits is 0 (and the other heads' stay finite)
        assert np.isnan(v['semantics_loss']) and np.isnan(v['optimization_loss'])
        assert float(g['sem'].abs().max()) == 0.0 and all(bool(torch.isfinite(g[h]).all()) for h in R.HEADS)
    elif name == 'wide_range':
        assert all(np.isfinite(x) for x in v.values()) and all(bool(torch.isfinite(g[h]).all()) for h in R.HEADS)
    if name in ('disjoint', 'equal_scores'):
        assert v['bb_scores_correlation'] == 0.0, v['bb_scores_correlation']
    if name == 'disjoint':
        assert v['bb_target_scores'] == 0.0
    compare(name, got, o64, o32, case)


# ------------------------------------------------------------------ the autograd wrapper
def test_wrapper_slices_scaling_and_no_grad():
    from box2mask_amd import functional as F
    case, o64, o32 = reference('S257')
    plain = run_kernel(case)
    # heads as column windows of one wider leaf: not contiguous, gradients land in the leaf's columns
    cols = {'off': (1, 4), 'bnd': (6, 9), 'sc': (11, 12), 'sem': (13, 33)}
    wide = torch.full((257, 40), 3.5)
    for h, (a, b) in cols.items():
        wide[:, a:b] = case[h]
    wide = wide.cuda().requires_grad_(True)
    heads, args = device_args(case, wrap=lambda h, t: wide[:, cols[h][0]:cols[h][1]])
    assert not any(heads[h].is_contiguous() for h in ('off', 'bnd', 'sem'))
    res, argmax = F.detection_loss(*args)
    (res[0] * 0.25).backward()
    assert np.array_equal(res.detach().cpu().numpy(), plain['values'])       # two workgroups: the two atomics commute
    assert torch.equal(argmax.cpu(), plain['argmax'])
    gw = wide.grad.cpu()
    used = torch.zeros(40, dtype=torch.bool)
    for h, (a, b) in cols.items():
        assert torch.equal(gw[:, a:b], plain['grads'][h] * 0.25), h           # (a power of two: exact)
        used[a:b] = True
    assert float(gw[:, ~used].abs().max()) == 0.0
    got = dict(plain, values=res.detach().cpu().numpy(), grads={h: gw[:, a:b] * 4 for h, (a, b) in cols.items()})
    compare('S257 sliced x0.25', got, o64, o32, case)
    # without autograd there is no node to carry the kernel's classes: they are re-made, and are the same
    with torch.no_grad():
        _, args = device_args(case, wrap=lambda h, t: t.cuda())
        res2, argmax2 = F.detection_loss(*args)
    assert res2.grad_fn is None and argmax2 is not None
    assert torch.equal(argmax2.cpu(), torch.argmax(case['sem'], 1)) and torch.equal(argmax2.cpu(), plain['argmax'])
    assert np.array_equal(res2.cpu().numpy(), plain['values'])


# ------------------------------------------------------------------ the C entry
def test_c_entry_leading_dimensions_and_output_extents():
    """b2m_detection_loss with heads that are column windows of an (S, 32) buffer (ld_* = 32) and every output placed
    inside a poisoned buffer: the same results as the contiguous call, and nothing written outside the outputs."""
    from box2mask_amd import _lib
    case, _, _ = reference('S257')
    plain = run_kernel(case)
    S, C = 257, 20
    wide = torch.full((S, 32), -9.0)
    cols = {'off': 0, 'bnd': 4, 'sc': 8, 'sem': 12}
    for h, a in cols.items():
        wide[:, a:a + case[h].shape[1]] = case[h]
    wide = wide.cuda()
    at = lambda h: wide.data_ptr() + 4 * cols[h]
    POISON, PAD = -777.25, 37
    sizes = [('d_off', S * 3), ('d_bnd', S * 3), ('d_sc', S), ('d_sem', S * C), ('result', 8)]
    f32 = torch.full((sum(n for _, n in sizes) + PAD * (len(sizes) + 1),), POISON, device='cuda')
    where, pos = {}, PAD
    for k, n in sizes:
        where[k] = (pos, n)
        pos += n + PAD
    i64 = torch.full((S + 2 * PAD,), -12345, dtype=torch.int64, device='cuda')
    f64 = torch.full((16 + 2 * PAD,), POISON, dtype=torch.float64, device='cuda')
    fptr = lambda k: f32.data_ptr() + 4 * where[k][0]
    gt_off, gt_bnd, loc = case['gt_off'].cuda(), case['gt_bnd'].cuda(), case['loc'].cuda()
    fg, gt_sem = case['fg'].to(torch.uint8).cuda(), case['gt_sem'].cuda()
    n_valid = torch.tensor([float(R.n_valid(case))], dtype=torch.float64).cuda()
    w = case['weights']
    _lib.call('b2m_detection_loss', at('off'), 32, at('bnd'), 32, at('sc'), 32, at('sem'), 32, C,
              gt_off.data_ptr(), gt_bnd.data_ptr(), loc.data_ptr(), fg.data_ptr(), gt_sem.data_ptr(), S, float(R.n_fg(case)),
              n_valid.data_ptr(), w[0], w[1], w[2], w[3], float(case['min_bb']), fptr('d_off'), fptr('d_bnd'), fptr('d_sc'),
              fptr('d_sem'), i64.data_ptr() + 8 * PAD, f64.data_ptr() + 8 * PAD, fptr('result'))
    torch.cuda.synchronize()
    f32c, i64c, f64c = f32.cpu(), i64.cpu(), f64.cpu()
    out = lambda k: f32c[where[k][0]:where[k][0] + where[k][1]]
    assert np.array_equal(out('result').numpy(), plain['values'])            # two workgroups: the two atomics commute
    for h in R.HEADS:
        assert torch.equal(out('d_' + h), plain['grads'][h].reshape(-1)), h
    assert torch.equal(i64c[PAD:PAD + S], plain['argmax'])
    keep = torch.ones_like(f32c, dtype=torch.bool)
    for a, n in where.values():
        keep[a:a + n] = False
    assert int(keep.sum()) == PAD * (len(sizes) + 1) and bool((f32c[keep] == POISON).all())
    assert bool((i64c[:PAD] == -12345).all()) and bool((i64c[PAD + S:] == -12345).all())
    assert bool((f64c[:PAD] == POISON).all()) and bool((f64c[PAD + 16:] == POISON).all())
    assert bool((wide.cpu()[:, [3, 7, 9, 10, 11]] == -9.0).all())


def test_two_runs_agree():
    """Gradients and classes are per-row work: the same bits.  The eight values come from fp64 atomics over five workgroups
    whose order is free: the fp64 sums differ in their last bits at most, the fp32 results by one ulp at most."""
    case, _, _ = reference('S1031')
    a, b = run_kernel(case), run_kernel(case)
    for h in R.HEADS:
        assert torch.equal(a['grads'][h], b['grads'][h]), h
    assert torch.equal(a['argmax'], b['argmax'])
    for i, k in enumerate(R.VALUE_NAMES):
        assert abs(float(a['values'][i]) - float(b['values'][i])) <= R.ulp32(float(a['values'][i])), k


# ------------------------------------------------------------------ the model path, fused and term by term
ALL = ['mlp_offsets', 'mlp_bounds', 'mlp_bb_scores', 'mlp_semantics']
MODEL_CASES = [(heads, epoch, True, True) for heads in (ALL[:2], ALL[:3], ALL[:2] + ALL[3:], ALL) for epoch in (99, 100)] + \
              [(ALL, 100, False, True), (ALL, 100, False, False)]
KEY2HEAD = {'mlp_offsets': 'off', 'mlp_bounds': 'bnd', 'mlp_bb_scores': 'sc', 'mlp_semantics': 'sem'}


@pytest.fixture(scope='module')
def model():
    from box2mask_amd import synth
    from box2mask_amd.config import scannet_config
    from box2mask_amd.model import Model
    return Model(scannet_config(), *synth.scannet_tables())


@pytest.mark.parametrize('heads,epoch,bb_supervision,on_fg', MODEL_CASES,
                         ids=['%s-e%d-sup%d-fg%d' % ('+'.join(h[4:7] for h in c[0]), c[1], c[2], c[3]) for c in MODEL_CASES])
def test_model_paths_match_rule(model, monkeypatch, heads, epoch, bb_supervision, on_fg):
    """Model.compute_loss_detection with the network stubbed, through the kernel (default) and term by term
    (B2M_FUSED_LOSS=0): the same keys, both within the bound of the fp64 rule, the same semantics_mIoU."""
    from box2mask_amd import synth
    from box2mask_amd.config import scannet_config
    cfg = scannet_config(network_heads=list(heads), bb_supervision=bb_supervision, loss_on_fg_instances=on_fg)
    assert cfg.mlp_bb_scores_start_epoch == 100
    monkeypatch.setattr(model, 'cfg', cfg)
    S = 300
    base = R.make_case(S, seed=77)
    g = torch.Generator().manual_seed(77)
    raw = torch.randint(0, 41, (S,), generator=g)                            # ScanNet ids: 20 valid, 21 mapped to -100
    lut = synth.scannet_tables()[1]
    masked = bb_supervision or on_fg
    w_sc = cfg.loss_weight_bb_scores if epoch >= cfg.mlp_bb_scores_start_epoch else 0.0
    case = dict(base, sc=base['sc'] if 'mlp_bb_scores' in heads else None, sem=base['sem'] if 'mlp_semantics' in heads else None,
                gt_sem=lut[raw] if 'mlp_semantics' in heads else None, fg=base['fg'] if masked else None,
                weights=(cfg.loss_weight_bb_offsets, cfg.loss_weight_bb_bounds, w_sc, cfg.loss_weight_semantics),
                min_bb=cfg.min_bb_size)
    if case['sem'] is not None:
        assert 0 < R.n_valid(case) < S
    o64, o32 = R.loss_rule(case, torch.float64), R.loss_rule(case, torch.float32)
    batch = {'input_location': base['loc'], 'gt_bb_offsets': base['gt_off'], 'gt_bb_bounds': base['gt_bnd'],
             'gt_semantics': raw, 'fg_instances': base['fg'], 'pooling_ids': torch.arange(S),
             'vox_features': torch.zeros(4, 6), 'vox_coords': torch.tensor([[0, i, 0, 0] for i in range(4)], dtype=torch.int32)}

    class H:
        def __init__(self, F): self.F = F
    results = {}
    for path in ('fused', 'terms'):
        with monkeypatch.context() as mp:
            if path == 'terms':
                mp.setenv('B2M_FUSED_LOSS', '0')
            pred = {k: case[KEY2HEAD[k]].cuda().requires_grad_(True) for k in heads}
            mp.setattr(model, 'detection_model', lambda sin, ids, n=None: {k: H(v) for k, v in pred.items()})
            calls = []
            from box2mask_amd import functional as F
            real = F.detection_loss
            mp.setattr(F, 'detection_loss', lambda *a: (calls.append(1), real(*a))[1])
            losses, _ = model.compute_loss_detection(batch, epoch)
            assert len(calls) == (1 if path == 'fused' else 0), 'the %s path ran the wrong code' % path
            losses['optimization_loss'].backward()
            torch.cuda.synchronize()
        num = lambda x: x.item() if hasattr(x, 'item') else float(x)
        results[path] = {k: num(x) for k, x in losses.items()}
        got = {'values': np.array([results[path].get(k, 0.0) for k in R.VALUE_NAMES]),
               'grads': {KEY2HEAD[k]: (pred[k].grad.cpu() if pred[k].grad is not None else torch.zeros(pred[k].shape))
                         for k in heads},
               'argmax': o64['argmax']}
        got['grads'].update({h: None for h in R.HEADS if case[h] is None})
        rows, bad = [], []
        for i, k in enumerate(R.VALUE_NAMES):
            if k in results[path]:
                rows.append((k, R.error(got['values'][i], o64['values'][i]), R.bound(o32['values'][i], o64['values'][i])[0]))
        for h in R.HEADS:
            if case[h] is not None:
                rows.append(('d_' + h, R.error(got['grads'][h], o64['grads'][h]), R.bound(o32['grads'][h], o64['grads'][h])[0]))
        for k, e, b in rows:
            print('%-6s %-22s error %.3e  bound %.3e  ratio %.3f' % (path, k, e, b, R.ratio(e, b)))
            if not e <= b:
                bad.append('%s: error %.3e > bound %.3e' % (k, e, b))
        assert not bad, (path, bad)
    assert set(results['fused']) == set(results['terms']), (sorted(results['fused']), sorted(results['terms']))
    expect = {'optimization_loss', 'offset_loss', 'bounds_loss'}
    expect |= {'bb_score_loss', 'bb_target_scores', 'bb_scores_correlation'} if case['sc'] is not None else set()
    expect |= {'semantics_loss', 'semantics_acc', 'semantics_mIoU'} if case['sem'] is not None else set()
    assert set(results['fused']) == expect
    if case['sem'] is not None:
        assert results['fused']['semantics_mIoU'] == results['terms']['semantics_mIoU']
        assert np.float32(results['fused']['semantics_acc']) == np.float32(o64['n_correct'] / S)
