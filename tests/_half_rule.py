"""Shared by tests/test_half_oracle_rule.py (CPU) and tests/test_gpu_half_oracle.py: passes of the oracle U-Net under the binary16
storage rule (oracle/unet_ref.py forward(storage='half'), profiles/half_oracle_rule.md), the quantities two passes are compared by,
and the bound on each -- MARGIN x what the fp32 oracle under the same rule shows against the fp64 one.

A *pass* here is anything that ran the network once on the batch and can show heads, parameter gradients, the traced tensors and
the gradients that arrived at them: the fp64 rule, the fp32 yardstick, the device.

Two ways of holding a pass C against the rule:
  whole network -- the rule runs once from the inputs with C's ReLU decisions; everything C produced is compared with it.  What the
      yardstick shows for this is large (heads 1e-2, parameter gradients several 1e-2): a value that lands on the other side of a
      binary16 rounding boundary is off by a half ulp, 2^-11, four orders above the fp32 noise that tipped it, the next layer's
      roundings tip in turn, and the train-mode BatchNorms over the few rows of the deepest levels amplify what reaches them.
  segment by segment -- the rule runs with C's value AND C's gradient put in place at every traced point (`force=`): each stretch
      between two traced points (a strided layer, a stage of two blocks, the heads) then computes from C's own inputs, so what is
      compared is that stretch alone -- its outputs, the gradient it sends back, its parameter gradients.  Nothing cascades past a
      stage, and a composition error of a few per cent in one block stands out."""
import contextlib

import numpy as np
import torch

from _parity import row_rel_err

HEADS = ['mlp_offsets', 'mlp_bounds', 'mlp_bb_scores', 'mlp_semantics']
MARGIN = 4.0
# added to the bound of every segment quantity: sixteen fp32 roundings.  Segment by segment the yardstick of a quantity can be an
# exact 0 (a column sum of a few hundred binary16 numbers is exact in fp32 in whatever order), and no fp32 computation that goes
# through constants rounded to fp32, as the device's BatchNorm does, can be asked for that
FLOOR = 16 * 2.0 ** -24
# the batch: tests/test_gpu_net.py's parity batch (seed0 4, 2 000 voxels a scene) with 16 scenes instead of 8 -- with 8 the largest
# scaled gradient of the pass is 9e4, past binary16's 65504 (profiles/half_oracle_rule.md, "saturation"), with 16 it is 1.4e4
SCENES, SEED0, VOXELS = 16, 4, 2000
LOSS_SCALE = 1024.0

# traced tensor -> level of its rows; the ones the device keeps in binary16 (levels 0 ... 3 behind the stem)
LEVEL_OF = {'out_p1': 0, 'up0': 0, 'block8': 0}
for _l in range(1, 8):
    LEVEL_OF['down%d' % _l] = _l
for _l, _b in enumerate(['block1', 'block2', 'block3', 'block4', 'added_block1', 'added_block2', 'added_block3'], 1):
    LEVEL_OF[_b] = _l
for _l, _b in ((6, 'added_block4'), (5, 'added_block5'), (4, 'added_block6'), (3, 'block5'), (2, 'block6'), (1, 'block7')):
    LEVEL_OF[_b] = _l
    LEVEL_OF['up%d' % _l] = _l
HALF_TRACED = {n for n, l in LEVEL_OF.items() if l <= 3 and n != 'out_p1'}
# the layers of the half region (state-dict prefixes): every '.kernel' below them is one convolution launch forward, and is
# followed by one BatchNorm
HALF_LAYERS = ('conv1p1s2', 'conv2p2s2', 'conv3p4s2', 'block1', 'block2', 'block3', 'block5', 'block6', 'block7', 'block8',
               'convtr5p8s2', 'convtr6p4s2', 'convtr7p2s2')
CAT_BLOCKS = ('block5', 'block6', 'block7', 'block8')


def layer_table_counts(state_dict):
    """(convolutions of the half region, BatchNorms of the half region, convolutions among them that read an ME.cat) from the names
    of the state dict -- what one pass must show as storage points and the device as launches."""
    convs = [k for k in state_dict if k.endswith('.kernel') and k.split('.')[0] in HALF_LAYERS]
    norms = [k for k in state_dict if k.endswith('.bn.weight') and (k.split('.')[0] in HALF_LAYERS or
                                                                    k.split('.')[0] in ('bn1', 'bn2', 'bn3', 'bntr5', 'bntr6', 'bntr7'))]
    cat = [k for k in convs if k.split('.')[0] in CAT_BLOCKS and k.split('.')[1] == '0' and ('conv1' in k or 'downsample' in k)]
    return len(convs), len(norms), len(cat)


def rel(a, b):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def targets(shapes):
    g = torch.Generator()
    g.manual_seed(1)
    return {h: torch.randn(shapes[h], generator=g, dtype=torch.float64) for h in HEADS}


class Pass:
    """heads / grads / trace / trace_grad: name -> CPU tensor (rows in the oracle's order; gradients un-scaled)."""

    def __init__(self, heads, grads, trace, trace_grad):
        self.heads, self.grads, self.trace, self.trace_grad = heads, grads, trace, trace_grad
        self.storage = None          # sparse_ref.HalfStorage of an oracle pass
        self.own = None              # an oracle pass's own ReLU decisions, in call order
        self.relu_stats = None       # per ReLU of a replayed oracle pass: see `relus`
        self.local = None            # of a forced oracle pass: the rule's own value / gradient at every traced point


def round_scaled(g, s=LOSS_SCALE):
    from oracle.sparse_ref import to_binary16
    return to_binary16(g * s) / s


class _Force(torch.autograd.Function):
    """A traced point of a forced pass: the network goes on with `value`; the gradient that arrives is kept (it is the rule's, computed
    from the other pass's gradients further down) and the other pass's gradient goes on up."""

    @staticmethod
    def forward(ctx, x, value, grad, sink, name):
        ctx.grad, ctx.sink, ctx.name = grad, sink, name
        return value.to(x.dtype).clone()

    @staticmethod
    def backward(ctx, g):
        ctx.sink[ctx.name] = g.detach().clone()
        return ctx.grad.to(g.dtype), None, None, None, None


@contextlib.contextmanager
def relus(masks=None, other=None, stats=None, own=None):
    """torch.relu of the oracle for one pass.  masks: decisions to replay in call order (None: the pass's own).  own: list that
    receives the pass's own decisions x > 0.  stats: list that receives, per ReLU, a dict with the fraction of elements on which
    the replayed mask (`dev_*`) and the decisions of `other` (`oth_*`) disagree with the pass's own, the largest |x| / rms among
    those, and the number of disagreeing elements with 0 < x <= 2^-25 (they store as zero in binary16)."""
    relu0 = torch.relu
    idx = [0]

    def one(x, m, o, pre):
        dis = o != m
        nd = int(dis.sum())
        rms = float(x.double().pow(2).mean().sqrt())
        return {pre + 'frac': nd / max(m.numel(), 1), pre + 'worst': (float(x[dis].abs().max()) / max(rms, 1e-30)) if nd else 0.0,
                pre + 'tiny': int((dis & (x > 0) & (x <= 2.0 ** -25)).sum())}

    def relu(x):
        i = idx[0]
        idx[0] += 1
        xd = x.detach()
        o = xd > 0
        if own is not None:
            own.append(o)
        if stats is not None:
            d = {'n': o.numel()}
            if masks is not None:
                d.update(one(xd, masks[i], o, 'dev_'))
            if other is not None:
                d.update(one(xd, other[i], o, 'oth_'))
            stats.append(d)
        if masks is None:
            return relu0(x)
        assert masks[i].shape == x.shape, (i, masks[i].shape, x.shape)
        return x * masks[i].to(x.dtype)
    torch.relu = relu
    try:
        yield
    finally:
        torch.relu = relu0
    assert masks is None or idx[0] == len(masks), (idx[0], len(masks))


def oracle_pass(p_cpu, batch, cfg, hier, n_seg, dtype, gws=None, masks=None, other=None, storage='half', inject=None, force=None):
    """One training pass of the oracle on `batch` in `dtype`, mean-squared head loss against `gws` (made on first use: pass the
    returned pass's `gws` on), gradients of every parameter and at every traced point.  force: a Pass whose traced values and
    gradients are put in place at every traced point."""
    from oracle import unet_ref, sparse_ref
    p = {k: (v.to(dtype).clone().requires_grad_(True) if v.is_floating_point() and 'running' not in k
             else (v.to(dtype) if v.is_floating_point() else v)) for k, v in p_cpu.items()}
    st = sparse_ref.HalfStorage(LOSS_SCALE) if storage == 'half' else None
    trace, tgrad, local_v, local_g = {}, {}, {}, {}

    def tap(name, t):
        if force is None:
            t.register_hook(lambda g, name=name: tgrad.__setitem__(name, g.detach().clone()))
            return t
        local_v[name] = t.detach()
        return _Force.apply(t, force.trace[name], force.trace_grad[name], local_g, name)
    own, stats = [], []
    with relus(masks, other, stats, own):
        out = unet_ref.forward(p, np.asarray(batch['vox_coords']), batch['vox_features'].to(dtype), batch['pooling_ids'], cfg,
                               training=True, n_segments=n_seg, hier=hier, trace=trace, storage=st, loss_scale=LOSS_SCALE,
                               inject=inject, tap=tap)
    if gws is None:
        gws = targets({h: out[h].shape for h in HEADS})
    sum(((out[h] - gws[h].to(dtype)) ** 2).mean() for h in HEADS).backward()
    r = Pass({h: out[h].detach() for h in HEADS}, {k: v.grad for k, v in p.items() if v.requires_grad and v.grad is not None},
             {k: v.detach() for k, v in trace.items()}, tgrad)
    r.storage, r.own, r.relu_stats, r.gws = st, own, stats, gws
    if force is not None:
        r.local = (local_v, local_g)
    return r


def whole_network(c, rule):
    """The quantities of the whole-network comparison of pass c with the rule pass: name -> figure."""
    q = {}
    for h in HEADS:
        q['head/' + h] = rel(c.heads[h], rule.heads[h])
        q['head rows/' + h] = row_rel_err(c.heads[h], rule.heads[h])
    for k in rule.trace:
        q['traced/' + k] = rel(c.trace[k], rule.trace[k])
    assert set(c.grads) == set(rule.grads)
    for k in rule.grads:
        q['gradient/' + k] = rel(c.grads[k], rule.grads[k])
    a = torch.cat([c.grads[k].reshape(-1).double().cpu() for k in rule.grads])
    b = torch.cat([rule.grads[k].reshape(-1).double() for k in rule.grads])
    q['1 - cosine'] = 1.0 - float((a * b).sum() / (a.norm() * b.norm()))
    return q


def segments(c, forced):
    """The quantities of the segment-by-segment comparison: `forced` is the fp64 rule run with c's values and gradients in place
    at the traced points.  At a point the device keeps in binary16 the rule's gradient is rounded as the storage point in front of
    it would round it, and so is c's (a no-op for the device, whose tensor is binary16)."""
    local_v, local_g = forced.local
    q = {}
    for h in HEADS:
        q['segment head/' + h] = rel(c.heads[h], forced.heads[h])
    for k in local_v:
        q['segment value/' + k] = rel(c.trace[k], local_v[k])
        g_rule, g_c = local_g[k], c.trace_grad[k].double()
        if k in HALF_TRACED:
            g_rule, g_c = round_scaled(g_rule), round_scaled(g_c)
        q['segment gradient/' + k] = rel(g_c, g_rule)
    for k in c.grads:                                # (a parameter the forced pass left without a gradient: zeros)
        f = forced.grads.get(k)
        q['segment parameter/' + k] = rel(c.grads[k], f if f is not None else torch.zeros_like(c.grads[k]))
    return q


def bounds(yard, extra=None):
    """name -> MARGIN x the yardstick's figure (+ an allowance derived elsewhere, by prefix)."""
    b = {k: MARGIN * v for k, v in yard.items()}
    for prefix, a in (extra or {}).items():
        for k in b:
            if k.startswith(prefix):
                b[k] += a
    return b


# BatchNorm -> the convolution in front of it, for the layers outside the blocks (the blocks' and the heads' parameters carry
# their stage's name in front)
_CONV_OF = {'bn0': 'conv0p1s1', 'bn1': 'conv1p1s2', 'bn2': 'conv2p2s2', 'bn3': 'conv3p4s2', 'bn4': 'conv4p8s2',
            'added_bn1': 'added_conv1p16s2', 'added_bn2': 'added_conv2p32s2', 'added_bn3': 'added_conv3p64s2',
            'added_bntr4': 'added_convtr4p128s2', 'added_bntr5': 'added_convtr5p64s2', 'added_bntr6': 'added_convtr6p32s2',
            'bntr4': 'convtr4p16s2', 'bntr5': 'convtr5p8s2', 'bntr6': 'convtr6p4s2', 'bntr7': 'convtr7p2s2'}
ULP = 2.0 ** -10          # binary16's spacing just below a power of two, relative


def stretch_of(parameter):
    """The stretch between two traced points a parameter belongs to: a strided / transposed layer with its BatchNorm, a stage of
    blocks, a head."""
    first = parameter.split('.')[0]
    return _CONV_OF.get(first, first)


def segment_bounds(yard):
    """The bounds of the stretch-by-stretch comparison from the yardstick's figures for it.
      * a parameter gradient: MARGIN x the LARGEST yardstick figure among the parameters of its stretch, + FLOOR.  Within a
        stretch every parameter gradient is a sum over the same few tensors with the same handful of tipped roundings in them; how
        hard those hit one parameter (over its own maximum) is luck -- the yardstick of a single BatchNorm weight is one draw, 3e-6
        on one host and 1e-5 on the next --, and the stretch's largest figure is the steadier estimate of what a correct pass
        shows there.  (The weight gradient off by 2 % still stands 6 x outside.)
      * a value or a gradient at a traced point the device keeps in binary16: MARGIN x the yardstick's figure, but not below ULP --
        one tipped rounding moves an element by one binary16 spacing, up to 2^-10 of itself, and whether the element that tips is the
        tensor's largest or a small one is chance; no pass can be held below one spacing at the maximum.
      * everything else (fp32 stretches, heads): MARGIN x the yardstick's figure + FLOOR."""
    top = {}
    for k, v in yard.items():
        if k.startswith('segment parameter/'):
            s = stretch_of(k.split('/', 1)[1])
            top[s] = max(top.get(s, 0.0), v)
    b = {}
    for k, v in yard.items():
        kind, name = k.split('/', 1)
        if kind == 'segment parameter':
            b[k] = MARGIN * top[stretch_of(name)] + FLOOR
        elif kind in ('segment value', 'segment gradient') and name in HALF_TRACED:
            b[k] = max(MARGIN * v, ULP)
        else:
            b[k] = MARGIN * v + FLOOR
    return b


def outside(q, bound):
    """[(ratio, name, figure, bound)] of the quantities past their bound, worst first."""
    return sorted(((v / max(bound[k], 1e-300), k, v, bound[k]) for k, v in q.items() if not v <= bound[k]), reverse=True)


def table(title, yard, got, bound=None, head=12):
    """Both columns, printed: per kind of quantity the medians and maxima, and the `head` quantities closest to (or furthest past)
    their bound."""
    bound = bound if bound is not None else bounds(yard)
    print('---- %s: yardstick | bound | held pass' % title)
    kinds = {}
    for k in yard:
        kinds.setdefault(k.split('/')[0], []).append(k)
    for kind, ks in kinds.items():
        yv, gv, bv = (np.array([d[k] for k in ks]) for d in (yard, got, bound))
        print('%-18s %3d quantities: yardstick median %.3e max %.3e | held pass median %.3e max %.3e | largest held / bound %.2f'
              % (kind, len(ks), np.median(yv), yv.max(), np.median(gv), gv.max(), float((gv / np.maximum(bv, 1e-300)).max())))
        for k in sorted(ks, key=lambda k: -got[k] / max(bound[k], 1e-300))[:head if len(ks) > 8 else len(ks)]:
            print('    %-46s %.3e | %.3e | %.3e' % (k, yard[k], bound[k], got[k]))


def make_batch():
    from box2mask_amd import synth
    return synth.make_batch(SCENES, seed0=SEED0, target_voxels=VOXELS, pts_per_m2=6000.0)
