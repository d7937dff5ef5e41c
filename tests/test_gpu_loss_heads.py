"""`b2m_detection_loss_ex` (csrc/nms.hip: the segment-level loss with the IoU loss and the centre-score loss) and
`b2m_rows_ce_loss` (csrc/loss.hip: cross entropy over the rows of the per-voxel head) against the fp64 restatement in
tests/_loss_heads_rule.py, and Model.compute_loss_detection through them on cases b, c, d of tests/golden/losses.npz.

The bound is the project's own (`_loss_rule.bound`): for every case and quantity the kernel's error against the fp64 evaluation
may be at most TWICE the error of the fp32 evaluation of the same rule plus FOUR fp32 ulps of the quantity's scale.  Classes and
hit counts are exact.  `ratio` = kernel error / that bound; every test prints it (pytest -s).

Pitches: the autograd functions hand a column window's stride(0) to the entries (the wrapper tests read the entry's arguments
back), and two tests call the entries directly at ld = 40 / ld = n_class + 3 into poisoned buffers.

Worst ratios measured on an MI355X (this file, 657 compared quantities; the table per quantity: profiles/loss_heads_rule.md):
segment kernel 0.546 (S1031: bb_scores_correlation), 0.473 (S1031_no_mask: d offsets), 0.466 (S255_no_mask: d bounds), iou_loss
0.184 (S1_no_mask), centre terms 0.097 at most; row kernel 0.123 (N63 at a pitch of 16: accuracy, an fp32 quotient), loss 0.099
(N4099, 63 classes), gradient 0.073 (direct entry, N65, 2 classes, ld 5); model routes against the rule 0.500 (c:
bb_scores_correlation), against each other 0.441 (c: semantics_loss).  Nothing needed more than the bound.
"""
import functools
import os

import numpy as np
import pytest
import torch

import _loss_heads_rule as H
import _loss_rule as R
from test_loss_heads_rule import HEAD_KEYS, golden_case

pytestmark = pytest.mark.gpu


def rows_table(tag, rows):
    bad = []
    for k, e, b in rows:
        print('%-22s %-26s error %.3e  bound %.3e  ratio %.3f' % (tag, k, e, b, R.ratio(e, b)))
        if not e <= b:
            bad.append('%s: error %.3e > bound %.3e' % (k, e, b))
    return bad


class entry_spy:
    """Records (name, args) of every functional._call inside the block: what the C entry was really handed."""

    def __enter__(self):
        from box2mask_amd import functional as F
        self.F, self.real, self.calls = F, F._call, []
        F._call = lambda name, *a, **k: (self.calls.append((name, a)), self.real(name, *a, **k))[1]
        return self

    def __exit__(self, *exc):
        self.F._call = self.real

    def args(self, name):
        hit = [a for n, a in self.calls if n == name]
        assert len(hit) == 1, (name, [n for n, _ in self.calls])
        return hit[0]


def poisoned(sizes, dtype, poison, pad=37):
    """One buffer holding the named outputs `pad` elements apart: (buffer, name -> (start, count))."""
    where, pos = {}, pad
    for k, n in sizes:
        where[k] = (pos, n)
        pos += n + pad
    return torch.full((pos,), poison, dtype=dtype, device='cuda'), where


def untouched(buf, where, poison):
    keep = torch.ones(buf.shape[0], dtype=torch.bool)
    for a, n in where.values():
        keep[a:a + n] = False
    return bool((buf.cpu()[keep] == poison).all())


# ------------------------------------------------------------------ the segment kernel
@functools.lru_cache(maxsize=None)
def seg_reference(name):
    """(case, fp64 evaluation, fp32 evaluation): computed once on the CPU, shared, never modified."""
    case = H.SEG_CASES[name]()
    return case, H.heads_rule(case, torch.float64), H.heads_rule(case, torch.float32)


def seg_args(case, wrap=lambda name, t: t.cuda().requires_grad_(True)):
    heads = {h: (wrap(h, case[h]) if case[h] is not None else None) for h in H.HEADS}
    nv = R.n_valid(case)
    w = case['weights']
    args = (heads['off'], heads['bnd'], heads['sc'], heads['cs'], heads['sem'], case['gt_off'].cuda(), case['gt_bnd'].cuda(),
            case['loc'].cuda(), case['fg'].to(torch.uint8).cuda() if case['fg'] is not None else None,
            case['gt_sem'].cuda() if case['sem'] is not None else None, R.n_fg(case),
            torch.tensor([float(nv)], dtype=torch.float64).cuda() if nv is not None else None,
            (float(w[0]), float(w[1]), float(case['w_iou']), float(w[2]), float(case['w_cs']), float(w[3])),
            float(case['min_bb']), bool(case['use_iou']))
    return heads, args


def run_seg(case, scale=None):
    from box2mask_amd import functional as F
    heads, args = seg_args(case)
    res, argmax = F.detection_loss_ex(*args)
    (res[0] if scale is None else res[0] * scale).backward()
    torch.cuda.synchronize()
    return {'values': res.detach().cpu().numpy().copy(), 'argmax': argmax.cpu() if argmax is not None else None,
            'grads': {h: (t.grad.cpu() if t is not None and t.grad is not None else None) for h, t in heads.items()}}


def compare_seg(tag, got, o64, o32, case):
    rows, bad = [], []
    for i, k in enumerate(H.VALUE_NAMES):
        rows.append((k, R.error(float(got['values'][i]), o64['values'][i]), R.bound(o32['values'][i], o64['values'][i])[0]))
    for h in H.HEADS:
        if case[h] is None:
            if got['grads'][h] is not None:
                bad.append('a gradient for the absent head %s' % h)
            continue
        if got['grads'][h] is None:
            bad.append('no gradient for head %s' % h)
            continue
        rows.append(('d_' + h, R.error(got['grads'][h], o64['grads'][h]), R.bound(o32['grads'][h], o64['grads'][h])[0]))
    bad += rows_table(tag, rows)
    if case['sem'] is not None:
        if not torch.equal(got['argmax'], o64['argmax']):
            bad.append('predicted classes differ')
        if np.float32(got['values'][7]) != np.float32(o64['n_correct'] / case['sem'].shape[0]):
            bad.append('semantics_acc')
    assert not bad, (tag, bad)


@pytest.mark.parametrize('name', sorted(H.SEG_CASES))
def test_segment_kernel_matches_rule(name):
    case, o64, o32 = seg_reference(name)
    got = run_seg(case)
    v = dict(zip(H.VALUE_NAMES, (float(x) for x in got['values'][:11])))
    g = got['grads']
    assert all(float(x) == 0.0 for x in got['values'][11:])
    # what has to be EXACT, before the bounds
    if not case['use_iou']:
        assert v['iou_loss'] == 0.0
    if case['cs'] is None:
        assert v['center_score_loss'] == 0.0 and v['center_scores_correlation'] == 0.0 and g['cs'] is None
    if case['fg'] is not None and bool((~case['fg']).any()):
        for h in ('off', 'bnd', 'sc', 'cs'):
            if case[h] is not None:
                assert float(g[h][~case['fg']].abs().max()) == 0.0, 'background rows have a %s gradient' % h
    if name == 'centre_zero':
        tie = (case['cs'].reshape(-1) == torch.sum(torch.abs(case['off'] - case['gt_off']), 1)) & case['fg']
        assert float(g['cs'][tie].abs().max()) == 0.0 and float(g['cs'][case['fg'] & ~tie].abs().min()) > 0
    if name == 'centre_const':
        assert v['center_scores_correlation'] == 0.0
    if name == 'disjoint':
        assert v['iou_loss'] == 1.0
    if name == 'box_kinds':
        at = [r[0] for r in H.dyadic_boxes()].index
        l1 = R.loss_rule(case)['grads']
        d_off, d_bnd = g['off'].double() - l1['off'], g['bnd'].double() - l1['bnd']        # the IoU term's share
        assert float(d_off[at('identical')].abs().max()) < 1e-8 and float(d_bnd[at('identical')].abs().max()) < 1e-8
        assert float(d_off[at('touching'), 0]) > 1e-3 and float(d_off[at('disjoint')].abs().max()) < 1e-8
        assert float(d_bnd[at('bound_below'), 0].abs()) < 1e-8 and float(d_bnd[at('bound_at_floor'), 0].abs()) > 1e-3
    compare_seg(name, got, o64, o32, case)


def test_segment_wrapper_pitches_and_scaling():
    """Heads as column windows of one wider leaf (row pitches wider than the rows), the total scaled by 0.25."""
    from box2mask_amd import functional as F
    case, o64, o32 = seg_reference('S257')
    plain = run_seg(case)
    cols = {'off': (1, 4), 'bnd': (6, 9), 'sc': (11, 12), 'cs': (13, 14), 'sem': (16, 36)}
    wide = torch.full((257, 40), 3.5)
    for h, (a, b) in cols.items():
        wide[:, a:b] = case[h]
    wide = wide.cuda().requires_grad_(True)
    heads, args = seg_args(case, wrap=lambda h, t: wide[:, cols[h][0]:cols[h][1]])
    with entry_spy() as spy:
        res, argmax = F.detection_loss_ex(*args)
    a = spy.args('b2m_detection_loss_ex')
    assert [a[i] for i in (1, 3, 5, 7, 9)] == [40] * 5, 'the windows were compacted: the kernel saw no pitch'
    assert a[0] == wide.data_ptr() + 4 * cols['off'][0] and a[8] == wide.data_ptr() + 4 * cols['sem'][0]
    (res[0] * 0.25).backward()
    assert np.array_equal(res.detach().cpu().numpy(), plain['values'])            # two workgroups: the two atomics commute
    assert torch.equal(argmax.cpu(), plain['argmax'])
    gw = wide.grad.cpu()
    used = torch.zeros(40, dtype=torch.bool)
    for h, (a, b) in cols.items():
        assert torch.equal(gw[:, a:b], plain['grads'][h] * 0.25), h                # (a power of two: exact)
        used[a:b] = True
    assert float(gw[:, ~used].abs().max()) == 0.0
    got = dict(plain, grads={h: gw[:, a:b] * 4 for h, (a, b) in cols.items()})
    compare_seg('S257 sliced x0.25', got, o64, o32, case)


@pytest.mark.parametrize('name', ['S257', 'S1031_no_mask'])
def test_segment_entry_leading_dimensions_and_output_extents(name):
    """b2m_detection_loss_ex called directly with every head a column window of one (S, 40) buffer (ld_* = 40) and every output
    inside a poisoned buffer: the bits of the dense call, nothing written outside the outputs, the inputs untouched."""
    from box2mask_amd import _lib
    case, _, _ = seg_reference(name)
    plain = run_seg(case)
    S, C, LD = case['off'].shape[0], case['sem'].shape[1], 40
    cols = {'off': 1, 'bnd': 6, 'sc': 11, 'cs': 13, 'sem': 16}
    wide = torch.full((S, LD), -9.0)
    for h, a in cols.items():
        wide[:, a:a + case[h].shape[1]] = case[h]
    before = wide.clone()
    wide = wide.cuda()
    at = lambda h: wide.data_ptr() + 4 * cols[h]
    POISON = -777.25
    f32, where = poisoned([('d_off', S * 3), ('d_bnd', S * 3), ('d_sc', S), ('d_cs', S), ('d_sem', S * C), ('result', 16)],
                          torch.float32, POISON)
    i64, wi = poisoned([('argmax', S)], torch.int64, -12345)
    f64, wd = poisoned([('sums', 32)], torch.float64, POISON)
    fptr = lambda k: f32.data_ptr() + 4 * where[k][0]
    gt_off, gt_bnd, loc = case['gt_off'].cuda(), case['gt_bnd'].cuda(), case['loc'].cuda()
    fg = case['fg'].to(torch.uint8).cuda() if case['fg'] is not None else None
    gt_sem = case['gt_sem'].cuda()
    n_valid = torch.tensor([float(R.n_valid(case))], dtype=torch.float64).cuda()
    w = case['weights']
    _lib.call('b2m_detection_loss_ex', at('off'), LD, at('bnd'), LD, at('sc'), LD, at('cs'), LD, at('sem'), LD, C,
              gt_off.data_ptr(), gt_bnd.data_ptr(), loc.data_ptr(), _lib.ptr(fg), gt_sem.data_ptr(), S, float(R.n_fg(case)),
              n_valid.data_ptr(), w[0], w[1], case['w_iou'], w[2], case['w_cs'], w[3], float(case['min_bb']), 1,
              fptr('d_off'), fptr('d_bnd'), fptr('d_sc'), fptr('d_cs'), fptr('d_sem'), i64.data_ptr() + 8 * wi['argmax'][0],
              f64.data_ptr() + 8 * wd['sums'][0], fptr('result'))
    torch.cuda.synchronize()
    f32c = f32.cpu()
    out = lambda k: f32c[where[k][0]:where[k][0] + where[k][1]]
    got = out('result').numpy()
    if S <= 512:
        assert np.array_equal(got, plain['values'])                              # two workgroups: the two atomics commute
    else:
        assert all(abs(float(a) - float(b)) <= R.ulp32(float(b)) for a, b in zip(got, plain['values']))
    for h in H.HEADS:
        assert torch.equal(out('d_' + h), plain['grads'][h].reshape(-1)), h
    assert torch.equal(i64.cpu()[wi['argmax'][0]:wi['argmax'][0] + S], plain['argmax'])
    assert untouched(f32, where, POISON) and untouched(i64, wi, -12345) and untouched(f64, wd, POISON)
    assert torch.equal(wide.cpu(), before)


def test_plain_entry_keeps_its_bits(golden_dir):
    """b2m_detection_loss on case a of losses.npz: the bits recorded from the library before b2m_detection_loss_ex shared its row
    code (tests/golden/loss_a_fused_bits.npz, recorded by tools/gen_loss_bits.py from the parent commit's build; 230 rows, one workgroup: no free order anywhere), and the new entry with both new
    terms off returns the same."""
    from box2mask_amd import functional as F
    from test_loss_rule import golden_case as case_a
    import test_gpu_loss as T
    case, _, _ = case_a(golden_dir)
    keep = np.load(os.path.join(golden_dir, 'loss_a_fused_bits.npz'))
    got = T.run_kernel(case)
    assert np.array_equal(got['values'].view(np.uint32), keep['values'].view(np.uint32))
    for h in R.HEADS:
        assert np.array_equal(got['grads'][h].numpy().view(np.uint32), keep['d_' + h].view(np.uint32)), h
    assert np.array_equal(got['argmax'].numpy(), keep['argmax'])
    ex = run_seg(dict(case, cs=None, use_iou=False, w_iou=0.0, w_cs=0.0))
    assert np.array_equal(ex['values'][:8].view(np.uint32), keep['values'].view(np.uint32))
    for h in R.HEADS:
        assert np.array_equal(ex['grads'][h].numpy().view(np.uint32), keep['d_' + h].view(np.uint32)), h


# ------------------------------------------------------------------ the row kernel
@functools.lru_cache(maxsize=None)
def row_reference(name):
    case = H.big_rows_case() if name == 'big' else H.ROW_CASES[name]()
    return case, H.rows_rule(case, torch.float64), H.rows_rule(case, torch.float32)


def run_rows(case, pad=0, scale=None):
    """`pad` > 0: the logits are the first C columns of an (N, C + pad) leaf."""
    from box2mask_amd import functional as F
    z, t = case['z'], case['t']
    N, C = z.shape
    leaf = torch.full((N, C + pad), -7.5)
    leaf[:, :C] = z
    leaf = leaf.cuda().requires_grad_(True)
    t = t.cuda()
    nv = ((t >= 0) & (t < C)).sum(dtype=torch.float64).reshape(1)
    with entry_spy() as spy:
        res, argmax = F.rows_ce_loss(leaf[:, :C] if pad else leaf, t, nv, case['weight'])
    a = spy.args('b2m_rows_ce_loss')
    assert a[0] == leaf.data_ptr() and (a[1] == C + pad or N == 1), 'the window was compacted: the kernel saw no pitch'
    (res[0] if scale is None else res[0] * scale).backward()
    torch.cuda.synchronize()
    g = leaf.grad.cpu()
    if pad:
        assert float(g[:, C:].abs().max()) == 0.0
    return {'values': res.detach().cpu().numpy().copy(), 'argmax': argmax.cpu(), 'grad': g[:, :C].contiguous()}


def compare_rows(tag, got, o64, o32, case):
    rows = [(k, R.error(float(got['values'][i]), o64['values'][i]), R.bound(o32['values'][i], o64['values'][i])[0])
            for i, k in enumerate(H.ROW_VALUE_NAMES)]
    rows.append(('d_logits', R.error(got['grad'], o64['grad']), R.bound(o32['grad'], o64['grad'])[0]))
    bad = rows_table(tag, rows)
    if not torch.equal(got['argmax'], o64['argmax']):
        bad.append('predicted classes differ in %d rows' % int((got['argmax'] != o64['argmax']).sum()))
    if np.float32(got['values'][2]) != np.float32(o64['n_correct'] / case['z'].shape[0]):
        bad.append('accuracy * N = %r, expected %d' % (float(got['values'][2]) * case['z'].shape[0], o64['n_correct']))
    t, C = case['t'], case['z'].shape[1]
    ign = (t < 0) | (t >= C)
    if bool(ign.any()) and float(got['grad'][ign].abs().max()) != 0.0:
        bad.append('ignored labels have a gradient')
    assert not bad, (tag, bad)


@pytest.mark.parametrize('pad', [0, 3], ids=['dense', 'pitch+3'])
@pytest.mark.parametrize('name', sorted(H.ROW_CASES))
def test_rows_kernel_matches_rule(name, pad):
    case, o64, o32 = row_reference(name)
    got = run_rows(case, pad)
    if name == 'labels_none':
        assert np.isnan(got['values'][0]) and np.isnan(got['values'][1]) and float(got['grad'].abs().max()) == 0.0
    else:
        assert bool(np.isfinite(got['values']).all()) and bool(torch.isfinite(got['grad']).all())
    compare_rows('%s pad %d' % (name, pad), got, o64, o32, case)


@pytest.mark.parametrize('N', [65, 4099])
@pytest.mark.parametrize('C', [1, 2, 20, 28, 63])
def test_rows_kernel_sizes_and_classes_cross(N, C):
    """Row counts and class counts varied against each other (the named cases vary one at 13 classes / 257 rows), up to the
    63 classes the entry accepts (the whole 64 KiB of LDS a workgroup may ask for); odd class counts with a pitch of C + 3."""
    case = H.rows_case(N, C, seed=N + C, labels='mixed')
    got = run_rows(case, pad=3 if C % 2 else 0)
    compare_rows('N%d C%d' % (N, C), got, H.rows_rule(case, torch.float64), H.rows_rule(case, torch.float32), case)


@pytest.mark.parametrize('N,C', [(65, 2), (4099, 13), (257, 63)])
def test_rows_entry_pitch_and_output_extents(N, C):
    """b2m_rows_ce_loss called directly on the first C columns of an (N, C + 3) buffer (ld = C + 3), every output inside a
    poisoned buffer -- d_logits dense N x C, partial exactly 2 * ceil(N / 256) doubles: the bits of the call on the compact
    copy (ld = C), nothing written outside the outputs, the padding columns untouched."""
    from box2mask_amd import _lib
    case = H.rows_case(N, C, seed=500 + N + C, labels='mixed')
    t = case['t'].cuda()
    nv = ((t >= 0) & (t < C)).sum(dtype=torch.float64).reshape(1)
    wide = torch.full((N, C + 3), -9.0)
    wide[:, :C] = case['z']
    before = wide.clone()
    wide, dense = wide.cuda(), case['z'].cuda()
    n_part = 2 * ((N + 255) // 256)
    outs = {}
    for tag, z, ld in (('pitch', wide, C + 3), ('dense', dense, C)):
        f32, where = poisoned([('d_logits', N * C), ('result', 3)], torch.float32, -777.25)
        i64, wi = poisoned([('argmax', N)], torch.int64, -12345)
        f64, wd = poisoned([('partial', n_part)], torch.float64, -777.25)
        _lib.call('b2m_rows_ce_loss', z.data_ptr(), ld, N, C, t.data_ptr(), nv.data_ptr(), case['weight'],
                  f32.data_ptr() + 4 * where['d_logits'][0], i64.data_ptr() + 8 * wi['argmax'][0],
                  f64.data_ptr() + 8 * wd['partial'][0], f32.data_ptr() + 4 * where['result'][0])
        torch.cuda.synchronize()
        assert untouched(f32, where, -777.25) and untouched(i64, wi, -12345) and untouched(f64, wd, -777.25), tag
        cut = lambda buf, w: buf.cpu()[w[0]:w[0] + w[1]]
        outs[tag] = (cut(f32, where['d_logits']), cut(f32, where['result']), cut(i64, wi['argmax']), cut(f64, wd['partial']))
        assert not bool((outs[tag][3] == -777.25).any())                         # every partial slot was written
    for a, b in zip(outs['pitch'], outs['dense']):
        assert torch.equal(a, b)
    assert torch.equal(wide.cpu(), before)
    got = {'values': outs['pitch'][1].numpy(), 'argmax': outs['pitch'][2], 'grad': outs['pitch'][0].reshape(N, C)}
    compare_rows('entry N%d C%d ld %d' % (N, C, C + 3), got, H.rows_rule(case, torch.float64), H.rows_rule(case, torch.float32), case)


def test_rows_two_runs_same_bits_and_scaling():
    """17 workgroups, no floating-point atomics: values and gradients have the same bits on every run; the incoming gradient
    scales the stored one."""
    case, _, _ = row_reference('N4099')
    a, b, q = run_rows(case), run_rows(case), run_rows(case, scale=0.25)
    assert np.array_equal(a['values'].view(np.uint32), b['values'].view(np.uint32))
    assert torch.equal(a['grad'], b['grad']) and torch.equal(a['argmax'], b['argmax'])
    assert torch.equal(q['grad'], a['grad'] * 0.25) and np.array_equal(q['values'], a['values'])


def test_rows_kernel_at_s3dis_size():
    """1 048 577 x 13: 4097 partial slots, the size of gt_per_vox_semantics of an S3DIS batch; twice, the same bits."""
    case, o64, o32 = row_reference('big')
    got = run_rows(case)
    compare_rows('big', got, o64, o32, case)
    again = run_rows(case)
    assert np.array_equal(got['values'].view(np.uint32), again['values'].view(np.uint32)) and torch.equal(got['grad'], again['grad'])


def test_rows_entry_checks_its_arguments():
    from box2mask_amd import _lib
    from box2mask_amd import functional as F
    z = torch.zeros(4, 64, device='cuda')
    with pytest.raises(_lib.B2MError):
        F.rows_ce_loss(z, torch.zeros(4, dtype=torch.int64, device='cuda'), torch.ones(1, dtype=torch.float64, device='cuda'), 1.0)


# ------------------------------------------------------------------ the model path, fused and term by term
@pytest.mark.parametrize('which', ['b', 'c', 'd'])
def test_model_takes_the_fused_route(golden_dir, monkeypatch, which):
    """Model.compute_loss_detection on cases b, c, d of losses.npz with a counter around functional._call and around the
    term-by-term code's helpers: by default the new entries run and no torch term does; with B2M_FUSED_LOSS=0 it is the other
    way round; both give the fixture's keys and lie within the bound of the fp64 rule."""
    from box2mask_amd import functional as F, model as M, synth
    from box2mask_amd.config import scannet_config
    case, rows, g, pre = golden_case(golden_dir, which)
    heads = ['mlp_offsets', 'mlp_bounds', 'mlp_bb_scores', 'mlp_semantics']
    if which == 'c':
        heads = heads + ['mlp_center_scores']
    if which == 'd':
        heads = ['mlp_offsets', 'mlp_bounds', 'mlp_bb_scores', 'mlp_per_vox_semantics']
    cfg = scannet_config(use_bb_iou_loss=(which == 'b'), network_heads=heads, loss_on_fg_instances=(which != 'd'),
                         bb_supervision=(which in 'ab'), loss_weight_center_scores=0.7, loss_weight_per_vox_semantics=0.9)
    model = M.Model(cfg, *synth.scannet_tables())
    o64, o32 = H.heads_rule(case, torch.float64), H.heads_rule(case, torch.float32)
    r64, r32 = (H.rows_rule(rows, torch.float64), H.rows_rule(rows, torch.float32)) if rows is not None else (None, None)
    batch = {k: torch.from_numpy(g[pre + 'batch_' + k]) for k in
             ('input_location', 'gt_bb_offsets', 'gt_bb_bounds', 'gt_semantics', 'fg_instances', 'pooling_ids',
              'gt_per_vox_semantics') if pre + 'batch_' + k in g.files}
    batch['vox_features'] = torch.zeros(4, 6)
    batch['vox_coords'] = torch.tensor([[0, i, 0, 0] for i in range(4)], dtype=torch.int32)
    keys = {k[len(pre):] for k in g.files if k.startswith(pre) and not any(s in k for s in ('pred_', 'grad_', 'batch_', 'epoch'))}
    expect = {'b': {'b2m_detection_loss_ex'}, 'c': {'b2m_detection_loss_ex'}, 'd': {'b2m_detection_loss', 'b2m_rows_ce_loss'}}[which]

    class Hd:
        def __init__(self, F): self.F = F
    results, route_grads, route_bounds = {}, {'fused': {}, 'terms': {}}, {}
    for path in ('fused', 'terms'):
        with monkeypatch.context() as mp:
            if path == 'terms':
                mp.setenv('B2M_FUSED_LOSS', '0')
            pred = {h: torch.from_numpy(g[pre + 'pred_' + h]).cuda().requires_grad_(True) for h in heads}
            mp.setattr(model, 'detection_model', lambda sin, ids, n=None: {h: Hd(v) for h, v in pred.items()})
            entries, terms = [], []
            real_call = F._call
            mp.setattr(F, '_call', lambda name, *a, **k: (entries.append(name), real_call(name, *a, **k))[1])
            for obj, attr in ((M, '_pearsonr'), (M, '_paired_box_iou'), (model, 'semantics_loss'), (model, 'BCEWithLogitsLoss')):
                real = getattr(obj, attr)
                mp.setattr(obj, attr, lambda *a, _r=real, _n=attr: (terms.append(_n), _r(*a))[1])
            losses, _ = model.compute_loss_detection(batch, int(g[pre + 'epoch']))
            losses['optimization_loss'].backward()
            torch.cuda.synchronize()
        loss_entries = {n for n in entries if 'loss' in n}
        if path == 'fused':
            assert loss_entries == expect and not terms, (loss_entries, terms)
        else:
            assert not loss_entries and terms, (loss_entries, terms)
        assert set(losses.keys()) == keys, (sorted(losses.keys()), sorted(keys))
        num = lambda x: x.item() if hasattr(x, 'item') else float(x)
        results[path] = {k: num(x) for k, x in losses.items()}
        table = []
        want64, want32 = dict(zip(H.VALUE_NAMES, o64['values'])), dict(zip(H.VALUE_NAMES, o32['values']))
        if rows is not None:
            for w, r in ((want64, r64), (want32, r32)):
                w['optimization_loss'] += r['values'][0]
                w['per_vox_semantics_loss'], w['per_vox_semantics_acc'] = r['values'][1], r['values'][2]
        for k in sorted(keys - {'semantics_mIoU'}):
            table.append((k, R.error(results[path][k], want64[k]), R.bound(want32[k], want64[k])[0]))
        for h in H.HEADS:
            if case[h] is not None:
                got = pred[HEAD_KEYS[h]].grad
                got = got.cpu() if got is not None else torch.zeros(case[h].shape)
                table.append(('d_' + h, R.error(got, o64['grads'][h]), R.bound(o32['grads'][h], o64['grads'][h])[0]))
                route_grads[path][h], route_bounds[h] = got, table[-1][2]
        if rows is not None:
            table.append(('d_per_vox', R.error(pred['mlp_per_vox_semantics'].grad.cpu(), r64['grad']), R.bound(r32['grad'], r64['grad'])[0]))
            route_grads[path]['per_vox'], route_bounds['per_vox'] = pred['mlp_per_vox_semantics'].grad.cpu(), table[-1][2]
        bad = rows_table('%s %s' % (which, path), table)
        assert not bad, (path, bad)
    # the two routes against each other, inside the same bound
    table = [(k, R.error(results['fused'][k], results['terms'][k]), R.bound(want32[k], want64[k])[0])
             for k in sorted(keys - {'semantics_mIoU'})]
    for k in sorted(route_grads['fused']):
        table.append(('d_' + k, R.error(route_grads['fused'][k], route_grads['terms'][k]), route_bounds[k]))
    bad = rows_table('%s fused-terms' % which, table)
    assert not bad, bad
    if 'semantics_mIoU' in keys:
        assert results['fused']['semantics_mIoU'] == results['terms']['semantics_mIoU']


def test_unevaluable_centre_configuration_still_fails_the_same_way(golden_dir):
    """Centre head with bb_supervision and without loss_on_fg_instances: the reference subtracts (S,) from (n_fg,) and raises;
    the fused route must not make it pass."""
    from box2mask_amd import model as M, synth
    from box2mask_amd.config import scannet_config
    case, _, g, pre = golden_case(golden_dir, 'c')
    heads = ['mlp_offsets', 'mlp_bounds', 'mlp_bb_scores', 'mlp_semantics', 'mlp_center_scores']
    cfg = scannet_config(network_heads=heads, loss_on_fg_instances=False, bb_supervision=True)
    model = M.Model(cfg, *synth.scannet_tables())
    pred = {h: torch.from_numpy(g[pre + 'pred_' + h]).cuda() for h in heads}

    class Hd:
        def __init__(self, F): self.F = F
    model.detection_model = lambda sin, ids, n=None: {h: Hd(v) for h, v in pred.items()}
    batch = {k: torch.from_numpy(g[pre + 'batch_' + k]) for k in
             ('input_location', 'gt_bb_offsets', 'gt_bb_bounds', 'gt_semantics', 'fg_instances', 'pooling_ids')}
    batch['vox_features'] = torch.zeros(4, 6)
    batch['vox_coords'] = torch.tensor([[0, i, 0, 0] for i in range(4)], dtype=torch.int32)
    assert 1 < int(batch['fg_instances'].sum()) < batch['fg_instances'].shape[0]
    with pytest.raises(RuntimeError, match='must match the size'):
        model.compute_loss_detection(batch, 150)
