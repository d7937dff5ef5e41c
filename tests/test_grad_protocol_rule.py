"""CPU side of tests/_grad_protocol_rule.py: the rule against float64 torch autograd on a dense restatement of the same network, the
exactness condition for every protocol, box2mask_amd.grad_arena ALONE under the protocols (a stand-in operator in torch, as in
tests/test_parallel.py: the HIP operators need a GPU), and the deliberate mistakes, each of which the comparison of the GPU test
(`compare`) must catch."""
import numpy as np
import pytest
import torch

import _conv_rule as R
import _grad_protocol_rule as P

SHAPES = P.SHAPES
EXTRA_SHAPES = ((193, 32), (577, 16))
P9_OPTS = ({'a_grad': False, 'frozen': ('W2',)}, {'use_y1': False}, {'frozen': ('W0', 'beta')})


def _dense_conv(nbr, x, w):
    t = torch.as_tensor(np.asarray(nbr), dtype=torch.long)
    y = torch.zeros(t.shape[1], w.shape[2], dtype=x.dtype)
    for k in range(t.shape[0]):
        o = torch.nonzero(t[k] >= 0).reshape(-1)
        if o.numel():
            y = y.index_add(0, o, x[t[k, o]] @ w[k])
    return y


def _network(cs, i, variant, o, params, conv, dtype, bn=True, lin=torch.matmul):
    """The network of the rule's docstring on torch operators; `conv(x, w)` is the 27-offset layer, `lin(x, w)` the 1x1 layer."""
    p = cs['passes'][i]
    a = p['a'].to(dtype).clone().requires_grad_(o['a_grad'])
    r = {k: p[k].to(dtype) for k in ('r1', 'r2', 'r3', 'r4', 'r5')}
    h = conv(a, params['W0'])
    t = conv(a, params['W3'])
    y1 = conv(h, params['W1'])
    z = h if variant == 'inplace' else torch.add(h, t)
    v = conv(z, params['W2'])
    s = lin(torch.relu(v), params['Wb']) + params['bias']
    out = {'y1': y1, 'v': v, 's': s, 't': t, 'u': None}
    loss = (v * r['r2']).sum() + (s * r['r3']).sum() + (t * r['r5']).sum()
    if o['use_y1']:
        out['u'] = conv(y1, params['W0'])
        loss = loss + (y1 * r['r1']).sum() + (out['u'] * r['r4']).sum()
    leaf = {'a': a}
    if bn:
        q = cs['bn_params']
        xb = torch.from_numpy(p['xb']).to(dtype).clone().requires_grad_(True)
        eps = float(np.float32(1e-5))
        for gm, bt, rr in ((params['gamma'], params['beta'], p['r6']), (params['gamma2'], params['beta2'], p['r7'])):
            y = torch.nn.functional.batch_norm(xb, None, None, gm, bt, True, 0.1, eps)
            loss = loss + (y * torch.from_numpy(rr).to(dtype)).sum()
        leaf['xb'] = xb
    return loss, out, leaf


@pytest.mark.parametrize('variant', P.VARIANTS)
@pytest.mark.parametrize('n,c', SHAPES)
def test_rule_equals_float64_autograd(n, c, variant):
    cs = P.case(n, c)
    for i, opts in [(0, {}), (1, {}), (2, {})] + list(enumerate(P9_OPTS)):
        o = dict(P.DEFAULT, **opts)
        params = {k: v.double().clone().requires_grad_(k not in o['frozen']) for k, v in cs['params'].items()}
        for k in ('gamma', 'beta', 'gamma2', 'beta2'):
            params[k] = torch.from_numpy(cs['bn_params'][k]).double().clone().requires_grad_(k != 'gamma2' and k not in o['frozen'])
        loss, out, leaf = _network(cs, i, variant, o, params, lambda x, w: _dense_conv(cs['nbr'], x, w), torch.float64)
        loss.backward()
        want = P.pass_values(cs, i, variant, opts)
        for k in P.OUTPUTS:
            assert (out[k] is None) == (want['out.' + k] is None)
            if out[k] is not None:
                assert torch.equal(out[k].detach(), want['out.' + k].v), (i, k)
        for k in P.CONV_PARAMS + ('a',):
            got = leaf['a'].grad if k == 'a' else params[k].grad
            assert (got is None) == (want[k] is None), (i, k)
            if got is not None:
                assert torch.equal(got, want[k].v), (i, k)           # (integers times GRID, far inside 53 bits: any order is exact)
        for k in P.BN_PARAMS + ('xb',):
            got = leaf['xb'].grad if k == 'xb' else params[k].grad
            assert (got is None) == (want[k] is None), (i, k)
            if got is not None:
                scale = float(want[k].v.abs().max())
                assert float((got - want[k].v).abs().max()) <= 1e-9 * scale, (i, k)
        assert params['gamma2'].grad is None


@pytest.mark.parametrize('protocol', sorted(P.PROTOCOLS))
@pytest.mark.parametrize('variant', P.VARIANTS)
@pytest.mark.parametrize('n,c', SHAPES + EXTRA_SHAPES)
def test_exactness_condition_holds_for_every_protocol(n, c, variant, protocol):
    """S of every exact observation, accumulated by the protocol itself, is inside 2^24 GRID (asserted inside `expected`), and the
    rule compared with itself is the same."""
    want = P.expected(n, c, variant, protocol)
    assert any(v is not None and v.s is not None for v in want.values())
    assert any(v is not None and v.b is not None for v in want.values())
    for k, v in want.items():
        if v is not None and v.s is not None:
            assert float(v.s.max()) <= 2.0 ** 24 * P.GRID, k
    assert P.compare({k: (None if v is None else v.v) for k, v in want.items()}, want) == []


# ----------------------------------------------------------------------------- the arena alone
class _ArenaConv(torch.autograd.Function):
    """Stands in for functional._SparseConv: the weight gradient goes into the arena slot where there is one."""

    @staticmethod
    def forward(ctx, x, w, nbr):
        ctx.save_for_backward(x, w)
        ctx.nbr = nbr
        return R.conv_fwd(nbr, x, None, w).float() if w.dim() == 3 else x @ w

    @staticmethod
    def backward(ctx, dy):
        from box2mask_amd.grad_arena import grad_slot
        x, w = ctx.saved_tensors
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = R.conv_dgrad(ctx.nbr, dy, w, x.shape[0]).float() if w.dim() == 3 else dy @ w.t()
        if ctx.needs_input_grad[1]:
            dw = grad_slot(w)
            if dw is None:
                dw = torch.zeros_like(w)
            dw += R.conv_wgrad(ctx.nbr, x, dy, torch.zeros_like(w).double()).float() if w.dim() == 3 else x.t() @ dy
        return dx, dw, None


def _arena_engine(n, c, variant, with_arena=True):
    from box2mask_amd.grad_arena import GradArena
    cs = P.case(n, c)
    params = {k: torch.nn.Parameter(v.clone()) for k, v in cs['params'].items()}
    arena = GradArena(list(params.values())) if with_arena else None
    conv = lambda x, w: _ArenaConv.apply(x, w, cs['nbr'])

    def run_pass(i, training, o):
        return _network(cs, i, variant, o, params, conv, torch.float32, bn=False, lin=conv)

    def open_pass(training):
        if arena is not None and torch.is_grad_enabled():
            arena.begin_pass()
    return P.TorchEngine(params, run_pass, open_pass), arena


@pytest.mark.parametrize('with_arena', [True, False], ids=['arena', 'plain'])
@pytest.mark.parametrize('protocol', sorted(P.PROTOCOLS))
def test_arena_alone_under_every_protocol(protocol, with_arena):
    """GradArena under a stand-in operator: every observation of every protocol is the rule, bit for bit.  (P4_autograd_grad
    failed before the arena kept track of the views it hands out: the tensors autograd.grad had returned were cleared by the
    next pass.)"""
    n, c = SHAPES[0]
    variant = 'torch_add' if protocol in ('P1_step_loop', 'P5_summed_loss') else 'inplace'
    engine, arena = _arena_engine(n, c, variant, with_arena)
    got = P.PROTOCOLS[protocol](engine)
    bad = P.compare(P.conv_only(got), P.conv_only(P.expected(n, c, variant, protocol)))
    assert not bad, bad
    if with_arena and protocol == 'P1_step_loop':        # the plain loop lives in buffer 0 and never needs a second one
        base = arena.buffers[0].data_ptr()
        assert arena.buffers[1] is None
        assert all(p.grad.data_ptr() == base + 4 * arena.offset[id(p)] for k, p in engine.params.items()
                   if k not in ('W0', 'bias'))     # (W0: two gradients summed by autograd; the bias is added by torch here)
    if with_arena and protocol == 'P4_autograd_grad':
        assert arena.current is None                     # third pass: both buffers owned, the arena stood aside


def test_arena_reuses_a_buffer_once_the_handed_views_are_gone():
    from box2mask_amd.grad_arena import GradArena
    w = torch.nn.Parameter(torch.ones(4, 4))
    arena = GradArena([w])
    arena.begin_pass()
    v = arena.slot(w)
    assert arena.current == 0 and v is not None
    arena.begin_pass()
    assert arena.current == 1                            # v is alive: buffer 0 is not cleared
    del v
    arena.begin_pass()
    assert arena.current == 0


# ----------------------------------------------------------------------------- mistakes
@pytest.mark.parametrize('mistake', sorted(P.MISTAKES))
def test_comparison_catches(mistake):
    protocol, variant = P.MISTAKES[mistake]
    n, c = SHAPES[0]
    want = P.expected(n, c, variant, protocol)
    wrong = P.PROTOCOLS[protocol](P.RuleEngine(P.case(n, c), variant, mistake))
    bad = P.compare({k: (None if v is None else v.v) for k, v in wrong.items()}, want)
    print(mistake, bad[:4])
    assert bad, 'the comparison does not see %s under %s' % (mistake, protocol)
    assert all(k.split(':')[0].rsplit('.', 1)[-1] not in P.BN_PARAMS + ('xb',) for k in bad), bad      # (the BatchNorm branch is not touched)


@pytest.mark.parametrize('protocol', P.HALF_PROTOCOLS)
@pytest.mark.parametrize('n', [193, 577])
def test_half_network_is_exact_and_representable(n, protocol):
    """The two-layer network of the half-precision test: binary16 values representable (asserted inside half_values), accumulated
    fp32 weight gradients inside 2^24 HALF_GRID; the values are float64 autograd's."""
    cs = P.case(n, 32)
    want = P.half_expected(n, 32, protocol)
    assert all(float(v.s.max()) <= 2.0 ** 24 * P.HALF_GRID for v in want.values())
    w0, w1 = (cs['params'][k].double().clone().requires_grad_(True) for k in ('W0', 'W1'))
    a = cs['passes'][0]['a'].double().clone().requires_grad_(True)
    y = _dense_conv(cs['nbr'], _dense_conv(cs['nbr'], a, w0), w1)
    (y * cs['passes'][0]['r1'].double()).sum().backward()
    vals = P.half_values(cs, 0)
    assert torch.equal(y.detach(), vals['out.y'].v) and torch.equal(a.grad, vals['a'].v)
    assert torch.equal(w0.grad, vals['W0'].v) and torch.equal(w1.grad, vals['W1'].v)
