"""The code between the HIP kernels and autograd -- grad_arena.GradArena, functional.issue_wgrad / grad_slot / _own /
_accumulation_target / _ZeroSlab / _param_grad_slots -- under the backward protocols of tests/_grad_protocol_rule.py, through the
real operators (functional.sparse_conv, batch_norm, relu) on hand-built rulebooks.

The convolution part is compared with torch.equal against the float64 rule (operands for which fp32 is exact in any order, on
either stream, however often a gradient is added to); the BatchNorm branch is held inside the bounds of _norm_rule summed over the
passes.  Results are read on the current stream with NO device-wide synchronize in front: a join that is missing is not hidden.
That a race does not show at these sizes proves nothing (see functional.issue_wgrad); which branch issue_wgrad took is therefore
asserted from its counter, and so is whether the data-gradient kernel added in place.

    protocols    the ten of _grad_protocol_rule.PROTOCOLS (P5 in both forms)
    shapes       193 x 16 (three tiles + 1 row: zero slab, atomic split, accumulate onto a slab piece) and 577 x 32 (over
                 TINY_MAP_ROWS, partial last tile) in the full cross; 193 x 32 and 577 x 16 in the default mode
    modes        default (weight gradients on the side stream: asserted) | B2M_DETERMINISTIC=1
    storage      a GradArena over the parameters, opened as SelectionNet.forward opens it | none
    aliases      B2M_CONV_PASSTHROUGH 1 | 0
    variants     'inplace' in the full cross, 'torch_add' for every protocol, shape and mode
    half         half_train.conv (two layers, loss scale 1) under accumulation and autograd.grad, both row counts, both modes
"""
import numpy as np
import pytest
import torch

import _grad_protocol_rule as P

pytestmark = pytest.mark.gpu

# weight-gradient launches of one pass, in any order: W0 (twice), W1, W2, W3, Wb.  JOINS[protocol]: how many of a protocol's
# launches find something autograd will add them to (functional.issue_wgrad, rule 3) -- a later gradient of W0 in one backward
# pass; every launch of a pass whose .grad exists already; every gradient of a weight already seen in a backward of two passes.
LAUNCHES = 6
JOINS = {'P1_step_loop': 3 * 1, 'P2_accumulation': 1 + 2 * LAUNCHES, 'P3_zero_in_place': 1 + 2 * LAUNCHES,
         'P4_autograd_grad': 1 + 1 + LAUNCHES, 'P5_summed_loss': 2 * LAUNCHES - 5, 'P5_reversed_backwards': 1 + LAUNCHES,
         'P6_retained_graph': 1 + LAUNCHES, 'P7_shared_weight': 2 * 1, 'P8_inference_between': 1,
         'P9_partial_gradients': 1 + 0 + 0}      # (no `a` gradient: W0 still twice | W0 once, nothing kept: NO wait | W0 frozen)


def _rulebook(nbr, n_in):
    from box2mask_amd.sparse import Rulebook
    K, n_out = nbr.shape
    return Rulebook(torch.from_numpy(np.ascontiguousarray(nbr)).cuda(), K, n_out, n_in)


_device = {}


def _device_case(n, c):
    if (n, c) not in _device:
        cs = P.case(n, c)
        d = {'rb': _rulebook(cs['nbr'], n), 'rbr': _rulebook(cs['rev'], n), 'passes': []}
        for p in cs['passes']:
            d['passes'].append({k: (v if torch.is_tensor(v) else torch.from_numpy(v)).cuda() for k, v in p.items()})
        _device[(n, c)] = d
    return _device[(n, c)]


def _engine(n, c, variant, with_arena):
    from box2mask_amd import functional as F_
    from box2mask_amd.grad_arena import GradArena
    cs, d = P.case(n, c), _device_case(n, c)
    rb, rbr = d['rb'], d['rbr']
    params = {k: torch.nn.Parameter(v.cuda()) for k, v in cs['params'].items()}
    q = cs['bn_params']
    for k in ('gamma', 'beta', 'beta2'):
        params[k] = torch.nn.Parameter(torch.from_numpy(q[k]).cuda())
    gamma2 = torch.nn.Parameter(torch.from_numpy(q['gamma2']).cuda(), requires_grad=False)
    running = [torch.from_numpy(q[k]).cuda().clone() for k in ('rm0', 'rv0', 'rm0', 'rv0')]
    arena = GradArena(list(params.values())) if with_arena else None
    conv = lambda x, w, **kw: F_.sparse_conv(x, None, w, None, rb, rbr, False, n, **kw)

    def open_pass(training):                     # the first lines of SelectionNet.forward
        F_.join_side_streams()
        F_.packed_weights.begin_pass(inference=not (training or torch.is_grad_enabled()))
        F_.zero_slab.new_pass()
        if arena is not None and torch.is_grad_enabled():
            arena.begin_pass()
        if training or torch.is_grad_enabled():
            F_.note_training_pass()

    def run_pass(i, training, o):
        p = d['passes'][i]
        a = p['a'].clone().requires_grad_(o['a_grad'] and training)
        h = conv(a, params['W0'])
        t = conv(a, params['W3'])
        y1, hp, _ = conv(h, params['W1'], passthrough=True)
        z = hp if variant == 'inplace' else torch.add(hp, t)
        v = conv(z, params['W2'])
        s = F_.sparse_conv(F_.relu(v), None, params['Wb'], params['bias'], None, None, False, n)
        out = {'y1': y1, 'v': v, 's': s, 't': t, 'u': None}
        loss = (v * p['r2']).sum() + (s * p['r3']).sum() + (t * p['r5']).sum()
        if o['use_y1']:
            out['u'] = conv(y1, params['W0'])
            loss = loss + (y1 * p['r1']).sum() + (out['u'] * p['r4']).sum()
        xb = p['xb'].clone().requires_grad_(training)
        y6 = F_.batch_norm(xb, params['gamma'], params['beta'], running[0], running[1], training)
        y7 = F_.batch_norm(xb, gamma2, params['beta2'], running[2], running[3], training)
        loss = loss + (y6 * p['r6']).sum() + (y7 * p['r7']).sum()
        return loss, out, {'a': a, 'xb': xb}
    return P.TorchEngine(params, run_pass, open_pass), arena


def _cases():
    out = []
    protocols = sorted(P.PROTOCOLS)
    for pr in protocols:
        for n, c in P.SHAPES:
            for mode in ('default', 'deterministic'):
                for arena in (1, 0):
                    for alias in (1, 0):
                        out.append((pr, n, c, mode, arena, alias, 'inplace'))
                out.append((pr, n, c, mode, 1, 1, 'torch_add'))
        for n, c in ((193, 32), (577, 16)):
            out.append((pr, n, c, 'default', 1, 1, 'inplace'))
    return [pytest.param(*t, id='%s-%dx%d-%s-arena%d-alias%d-%s' % t) for t in out]


@pytest.mark.parametrize('protocol,n,c,mode,with_arena,alias,variant', _cases())
def test_protocol_is_the_rule(monkeypatch, protocol, n, c, mode, with_arena, alias, variant):
    from box2mask_amd import functional as F_
    for k in ('B2M_DETERMINISTIC', 'B2M_WGRAD_STREAM', 'B2M_CONV_PASSTHROUGH', 'B2M_CONV_ZERO_SLAB', 'B2M_BN_SMALL_ROWS'):
        monkeypatch.delenv(k, raising=False)
    if mode == 'deterministic':
        monkeypatch.setenv('B2M_DETERMINISTIC', '1')
    else:
        assert F_.wgrad_on_side_stream()
    monkeypatch.setenv('B2M_CONV_PASSTHROUGH', str(alias))
    want = P.expected(n, c, variant, protocol)            # (exactness condition asserted inside; computed once per module)
    in_place = [0]
    target = F_._accumulation_target

    def counting(g, *args):
        r = target(g, *args)
        in_place[0] += r is not None
        return r
    monkeypatch.setattr(F_, '_accumulation_target', counting)
    engine, arena = _engine(n, c, variant, bool(with_arena))
    joins0 = F_._side['early_joins']
    got = P.PROTOCOLS[protocol](engine)
    # no synchronize: `compare` copies to the host on the current stream
    bad = P.compare(got, want)
    assert not bad, bad[:8]
    joins = F_._side['early_joins'] - joins0
    if mode == 'default':
        # the plain step loop (first gradient of a weight, .grad None) placed no wait; everything autograd adds to did
        assert joins == JOINS[protocol], (joins, JOINS[protocol])
    else:
        assert joins == 0
    assert not F_._side['seen'] and not F_._side['armed']
    if variant == 'inplace' and alias:
        assert in_place[0] > 0, 'the gradient of the alias was not added in place'
    else:
        assert in_place[0] == 0, 'a gradient that is not this node\'s own was added in place'
    if with_arena and protocol == 'P1_step_loop':
        base = arena.buffers[0].data_ptr()
        assert arena.buffers[1] is None
        # (W0: two gradients, summed by autograd into a tensor of its own; beta2: its BatchNorm's gamma is frozen, so
        # functional._param_grad_slots allocates both)
        assert all(p.grad.data_ptr() == base + 4 * arena.offset[id(p)] for k, p in engine.params.items() if k not in ('W0', 'beta2'))


# ------------------------------------------------------------------ half training: half_train.conv over the same plumbing
@pytest.mark.parametrize('with_arena', [1, 0], ids=['arena', 'plain'])
@pytest.mark.parametrize('mode', ['default', 'deterministic'])
@pytest.mark.parametrize('n', [193, 577])
@pytest.mark.parametrize('protocol', P.HALF_PROTOCOLS)
def test_half_protocol_is_the_rule(monkeypatch, protocol, n, mode, with_arena):
    """h = conv(a, W0), y = conv(h, W1) through half_train.conv (binary16 activations and data gradients, fp32 weight gradients in
    the arena, loss scale 1) under gradient accumulation and autograd.grad: bit for bit the rule; every binary16 value is
    representable (_grad_protocol_rule.half_values)."""
    from box2mask_amd import functional as F_, half_train as HT
    from box2mask_amd.grad_arena import GradArena
    for k in ('B2M_DETERMINISTIC', 'B2M_WGRAD_STREAM', 'B2M_CONV_PASSTHROUGH'):
        monkeypatch.delenv(k, raising=False)
    if mode == 'deterministic':
        monkeypatch.setenv('B2M_DETERMINISTIC', '1')
    else:
        assert F_.wgrad_on_side_stream()
    monkeypatch.setattr(HT, 'loss_scale', [1.0])
    monkeypatch.setattr(HT, 'guard', [None])
    c = 32
    want = P.half_expected(n, c, protocol)
    cs, d = P.case(n, c), _device_case(n, c)
    rb, rbr = d['rb'], d['rbr']
    params = {k: torch.nn.Parameter(cs['params'][k].cuda()) for k in ('W0', 'W1')}
    arena = GradArena(list(params.values())) if with_arena else None
    HT.images.__init__()

    def open_pass(training):
        F_.join_side_streams()
        F_.packed_weights.begin_pass()
        F_.zero_slab.new_pass()
        if arena is not None:
            arena.begin_pass()
        F_.note_training_pass()
        HT.images.begin_pass()

    def run_pass(i, training, o):
        p = d['passes'][i]
        a = p['a'].half().requires_grad_(True)
        h = HT.conv(a, None, params['W0'], rb, rbr, False, n)
        y = HT.conv(h, None, params['W1'], rb, rbr, False, n)
        assert y.dtype == torch.float16
        return (y.float() * p['r1']).sum(), {'y': y}, {'a': a}
    joins0 = F_._side['early_joins']
    try:
        got = P.PROTOCOLS[protocol](P.TorchEngine(params, run_pass, open_pass))
        bad = P.compare(got, want)            # (no synchronize in front)
    finally:
        HT.images.__init__()
    assert not bad, bad
    joins = F_._side['early_joins'] - joins0
    # two launches per pass, no weight shared: accumulation joins in passes 2 and 3, autograd.grad + backward only in the third pass
    assert joins == ((4 if protocol == 'P2_accumulation' else 2) if mode == 'default' else 0)
