"""The binary16 storage mode of the oracle U-Net (oracle/unet_ref.py forward(storage='half'); profiles/half_oracle_rule.md) -- the rule
tests/test_gpu_half_oracle.py holds the half-precision training pass of the device to.  No GPU here:

  1. storage=None is the oracle of before, bit for bit;
  2. the storage point itself at binary16's edges;
  3. under storage='half' in fp64 the traced tensors of the half region hold binary16 values only, the others do not, and the
     storage points hit are the ones the layer table names;
  4. nothing saturates (the two maxima are printed);
  5. what the fp32 oracle under the same rule (the yardstick) shows against the fp64 one, whole network and segment by segment
     (tests/_half_rule.py), and with it the bounds of the GPU test;
  6. seven deliberate mistakes in how the half kernels are composed, each of which must move a named quantity past its bound."""
import numpy as np
import pytest
import torch

import _half_rule as R

S_ = R.LOSS_SCALE


def _net_cpu():
    from box2mask_amd import synth
    from box2mask_amd.config import scannet_config
    from box2mask_amd.detection_net import SelectionNet
    cfg = scannet_config()
    valid, _, _, is_fg = synth.scannet_tables()
    torch.manual_seed(0)
    net = SelectionNet(cfg, 'cpu', valid, is_fg, out_channels=[96, 96, 6])
    return cfg, {k: v.detach().clone() for k, v in net.state_dict().items()}


@pytest.fixture(scope='module')
def ctx():
    """The passes every test below shares: the fp64 rule on its own ReLU decisions, the fp32 yardstick on the same decisions, and
    the fp64 rule forced segment by segment with the yardstick's values and with its own."""
    from oracle import sparse_ref
    cfg, p_cpu = _net_cpu()
    batch = R.make_batch()
    n_seg = batch['input_location'].shape[0]
    hier = sparse_ref.Hierarchy(batch['vox_coords'].numpy())
    run = lambda dtype, **kw: R.oracle_pass(p_cpu, batch, cfg, hier, n_seg, dtype, **kw)
    rule = run(torch.float64)
    kw = dict(gws=rule.gws, masks=rule.own)
    yard = run(torch.float32, **kw)
    c = dict(cfg=cfg, p_cpu=p_cpu, hier=hier, rule=rule, yard=yard, run=run, kw=kw)
    c['yard_whole'] = R.whole_network(yard, rule)
    c['yard_segments'] = R.segments(yard, run(torch.float64, force=yard, **kw))
    c['self_forced'] = run(torch.float64, force=rule, **kw)
    c['bounds'] = dict(R.bounds(c['yard_whole']), **R.segment_bounds(c['yard_segments']))
    return c


def test_storage_none_is_untouched():
    """Heads and every parameter gradient of forward(..., storage=None) equal those of a call without the argument, bit for bit
    (two scenes: the smallest batch whose deepest levels keep the two rows a training-mode BatchNorm needs)."""
    from box2mask_amd import synth
    from oracle import unet_ref
    cfg, p_cpu = _net_cpu()
    batch = synth.make_batch(2, seed0=R.SEED0, target_voxels=R.VOXELS, pts_per_m2=6000.0)
    n_seg = batch['input_location'].shape[0]
    res = []
    for kw in ({}, {'storage': None, 'loss_scale': 1024.0}):
        p = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and 'running' not in k else v) for k, v in p_cpu.items()}
        trace = {}
        out = unet_ref.forward(p, batch['vox_coords'].numpy(), batch['vox_features'], batch['pooling_ids'], cfg, training=True,
                               n_segments=n_seg, trace=trace, **kw)
        sum((out[h] ** 2).mean() for h in R.HEADS).backward()
        res.append((out, {k: v.grad for k, v in p.items() if v.requires_grad}, trace))
    (o0, g0, t0), (o1, g1, t1) = res
    assert set(g0) == set(g1) and len(g0) == 283 and set(t0) == set(t1)
    for h in R.HEADS:
        assert torch.equal(o0[h], o1[h]), h
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    for k in t0:
        assert torch.equal(t0[k], t1[k]), k


def test_the_storage_point_at_the_edges_of_binary16():
    from oracle.sparse_ref import HalfStorage
    st = HalfStorage(S_)
    u = 2.0 ** -10                                   # binary16's spacing in [1, 2)
    sub = 2.0 ** -24                                 # its smallest subnormal
    cases = [(1 + u / 2, 1.0), (1 + 3 * u / 2, 1 + 2 * u), (1 + 5 * u / 2, 1 + 2 * u),       # ties go to the even neighbour
             (1 + u / 2 + 2.0 ** -30, 1 + u), (-(1 + u / 2), -1.0),
             (65504.0, 65504.0), (65519.0, 65504.0), (65520.0, float('inf')), (-65520.0, -float('inf')),   # the largest finite value; no saturation
             (3 * sub, 3 * sub), (2.5 * sub, 2 * sub), (3.5 * sub, 4 * sub), (0.5 * sub, 0.0), (0.5 * sub + 2.0 ** -60, sub),   # subnormals are kept
             (2.0 ** -14 - sub / 4, 2.0 ** -14), (1.3 * 2.0 ** -30, 0.0)]
    x = torch.tensor([c[0] for c in cases], dtype=torch.float64, requires_grad=True)
    y = st.point(x)
    assert torch.equal(y.detach(), torch.tensor([c[1] for c in cases], dtype=torch.float64)), y
    # backward: the gradient is rounded as if scaled by s -- a value that would vanish un-scaled is a binary16 subnormal once
    # scaled (1.3 * 2^-30 * 2^10 = 20.8 * 2^-24 -> 21 * 2^-24), a tie goes to even, 65504 / s survives, more does not
    g = torch.tensor([1.3 * 2.0 ** -30, (1 + u / 2) / S_, 2.5 * sub / S_, 65504.0 / S_, 65520.0 / S_, 0.5 * sub / S_] + [0.0] * (len(cases) - 6),
                     dtype=torch.float64)
    y.backward(g)
    want = torch.tensor([21 * sub / S_, 1.0 / S_, 2 * sub / S_, 65504.0 / S_, float('inf'), 0.0] + [0.0] * (len(cases) - 6), dtype=torch.float64)
    assert torch.equal(x.grad, want), x.grad
    # ... and a gradient-only point: the identity forward, the same backward; the result times s is a binary16 number, always
    gen = torch.Generator(); gen.manual_seed(0)
    for dtype in (torch.float64, torch.float32):
        z = (torch.randn(4096, generator=gen, dtype=torch.float64) * torch.logspace(-12, 1, 4096, dtype=torch.float64)).to(dtype).requires_grad_(True)
        w = st.grad_only(z)
        assert torch.equal(w.detach(), z.detach())
        gz = torch.randn(4096, generator=gen, dtype=torch.float64).to(dtype) * torch.logspace(-12, 1, 4096, dtype=torch.float64).to(dtype)
        w.backward(gz)
        scaled = z.grad * S_
        assert _is_binary16(scaled)
        assert float((z.grad - gz).abs().max()) > 0 and bool(((z.grad - gz).abs() <= gz.abs() * 2.0 ** -11 + sub / S_ / 2).all())
    assert st.count == {'activation': 1}


def _is_binary16(t):
    from oracle.sparse_ref import to_binary16
    return torch.equal(to_binary16(t), t)


def test_the_half_region_and_only_it_holds_binary16_values(ctx):
    rule = ctx['rule']
    assert set(rule.trace) == set(R.LEVEL_OF)
    for name, t in rule.trace.items():
        if name in R.HALF_TRACED:
            assert _is_binary16(t), name
        else:                                        # stem, tensor strides >= 16: nothing rounds them
            assert float((t.half().to(t.dtype) != t).double().mean()) > 0.1, name
    for h in R.HEADS:
        assert not _is_binary16(rule.heads[h]), h
    for k, g in rule.grads.items():                  # parameter gradients are never rounded
        assert g.numel() < 8 or not _is_binary16(g * S_), k
    # the gradient that arrived at a traced point of the region: sums of binary16 numbers (over the loss scale), the storage point
    # in front of it rounds them once more
    n_conv, n_bn, n_cat = R.layer_table_counts(ctx['p_cpu'])
    assert (n_conv, n_bn, n_cat) == (40, 40, 8)
    assert rule.storage.count == {'to_half': 2, 'conv': n_conv, 'bn': n_bn, 'weight': n_conv}, rule.storage.count
    assert ctx['yard'].storage.count == rule.storage.count


def test_nothing_saturates(ctx):
    st = ctx['rule'].storage
    print('largest activation at a storage point %.4e; largest scaled gradient %.4e (by kind of point: %s); binary16 ends at 65504'
          % (st.max_activation, st.max_scaled_gradient, {k: '%.3e' % v for k, v in st.max_scaled_gradient_at.items()}))
    assert st.max_activation < 65504.0 and st.max_scaled_gradient < 65504.0
    for p in [ctx['rule'], ctx['yard']]:
        assert all(bool(torch.isfinite(g).all()) for g in p.grads.values())


def test_what_the_yardstick_supports(ctx):
    """Both comparisons of the fp32 yardstick with the fp64 rule, printed; the bounds of the GPU test are 4 x these.
    Whole network (measured: heads 2e-2 ... 6e-2, worst parameter gradient 1e-1 ... 2e-1): 4 x that is NOT a fifth of the 1e-1 / 3e-1
    of test_half_training_pass_against_the_fp32_pass -- two correct half-storage passes are as far apart as a half pass is from
    an fp32 one, because a rounding that tips is a half ulp and tips the next (profiles/half_oracle_rule.md).  Segment by segment
    the yardstick is at 1e-6 ... 1e-3, and there the condition holds with room: asserted."""
    yw, ys = ctx['yard_whole'], ctx['yard_segments']
    R.table('whole network, yardstick against itself', yw, yw, head=6)
    R.table('segment by segment, yardstick against itself', ys, ys, R.segment_bounds(ys), head=6)
    st = ctx['yard'].relu_stats
    print('ReLU decisions, yardstick against rule: largest fraction %.3e, largest |pre-activation| / rms %.3e, stored-as-zero %d of %d'
          % (max(d['dev_frac'] for d in st), max(d['dev_worst'] for d in st), sum(d['dev_tiny'] for d in st), sum(d['n'] for d in st)))
    b = ctx['bounds']
    assert max(v for k, v in b.items() if k.startswith('segment head/')) <= 1e-1 / 5
    assert max(v for k, v in b.items() if k.startswith('segment parameter/')) <= 3e-1 / 5
    assert max(v for k, v in b.items() if k.startswith('segment value/')) <= 1e-1 / 5
    assert max(v for k, v in b.items() if k.startswith('segment gradient/')) <= 3e-1 / 5
    # the rule forced with its own values and gradients reproduces itself: the segments fit together
    own = R.segments(ctx['rule'], ctx['self_forced'])
    assert max(own.values()) < 1e-9, max(own.items(), key=lambda kv: kv[1])


def _edit_grads(ctx, edit):
    c = R.Pass(ctx['rule'].heads, dict(ctx['rule'].grads), ctx['rule'].trace, ctx['rule'].trace_grad)
    edit(c.grads)
    return R.segments(c, ctx['self_forced']), R.whole_network(c, ctx['rule'])


def _scaled_bn(g):
    for k in ('block2.1.norm1.bn.weight', 'block2.1.norm1.bn.bias'):
        g[k] = g[k] * S_


def _x2_at_offset_0(g):
    w = g['block7.0.conv1.kernel'].clone()           # ME.cat(up1 (96 channels), block1's output (32)): c1 = 96
    c1 = 96
    c2 = w.shape[1] - c1
    part = w[:, c1:].clone()
    w[:, c1:] = 0
    w[:, :c2] += part
    g['block7.0.conv1.kernel'] = w


def _two_per_cent(g):
    g['block6.1.conv2.kernel'] = g['block6.1.conv2.kernel'] * 1.02


# name -> (how, the quantity that must leave its bound)
MISTAKES = {
    'dgamma and dbeta of one layer left scaled by s': (_scaled_bn, 'segment parameter/block2.1.norm1.bn.weight'),
    'x2 rows of one weight gradient at channel offset 0': (_x2_at_offset_0, 'segment parameter/block7.0.conv1.kernel'),
    'one weight gradient off by 2 per cent': (_two_per_cent, 'segment parameter/block6.1.conv2.kernel'),
    'pass-through gradient dropped at one block': ({'drop_passthrough': 'block2.1'}, 'segment gradient/down2'),
    'dres dropped at one block': ({'drop_dres': 'block6.0'}, 'segment parameter/block6.0.downsample.0.kernel'),
    'loss scale applied twice across the fp32 island': ({'scale_twice': True}, 'segment gradient/added_block6'),
    'ReLU mask of a fused-residual BatchNorm taken before the add': ({'mask_before_add': 'block7.1'}, 'segment parameter/block7.1.conv2.kernel'),
}


@pytest.mark.parametrize('mistake', sorted(MISTAKES))
def test_a_deliberate_mistake_leaves_the_bounds(ctx, mistake):
    """The half-storage oracle with one injected error against itself un-broken, on the same ReLU decisions.  The first three
    change a parameter gradient after the pass; the others change the graph, and run as the forced pass (the un-broken rule's values
    and gradients at the traced points), so the figure is that of the stretch the error sits in."""
    how, named = MISTAKES[mistake]
    if callable(how):
        q, qw = _edit_grads(ctx, how)
    else:
        broken = ctx['run'](torch.float64, force=ctx['rule'], inject=how, **ctx['kw'])
        q, qw = R.segments(ctx['rule'], broken), None
    b = ctx['bounds']
    out = R.outside(q, b)
    print('%s: %s = %.3e, bound %.3e (x %.1f); %d segment quantities outside, worst %s'
          % (mistake, named, q[named], b[named], q[named] / b[named], len(out), ['%s x%.1f' % (k, r) for r, k, _, _ in out[:3]]))
    if qw is not None:
        ow = R.outside(qw, b)
        print('    whole network: %d quantities outside %s' % (len(ow), ['%s %.3e (bound %.3e)' % (k, v, bd) for _, k, v, bd in ow[:2]]))
    assert q[named] > b[named], (named, q[named], b[named])
