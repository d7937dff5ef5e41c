"""Where a gradient lives, when its memory is cleared and what is added to it -- under nine backward protocols -- restated in
float64 on the CPU, for tests/test_grad_protocol_rule.py (CPU: the rule against torch autograd, box2mask_amd.grad_arena alone, and
deliberate mistakes) and tests/test_gpu_grad_protocol.py (the real operators of box2mask_amd.functional over a GradArena, side
stream and zero slab).  The convolution and BatchNorm arithmetic is that of tests/_conv_rule.py and tests/_norm_rule.py, imported.

THE NETWORK (one pass; `a`, `xb` leaves, r1..r7 constants, all of them different from pass to pass)

    h      = conv(a, W0)
    t      = conv(a, W3)
    y1, hp = conv(h, W1, passthrough=True)       hp: the alias of h every other consumer takes
    z      = hp                                  variant 'inplace':   W2's data gradient is made for W1's node, which adds onto it
           = torch.add(hp, t)                    variant 'torch_add': AddBackward hands ONE tensor to hp and t: no in-place add
    v      = conv(z, W2)
    s      = conv1x1(relu(v), Wb, bias)
    u      = conv(y1, W0)                        W0 a second time
    loss   = <y1,r1> + <v,r2> + <s,r3> + <u,r4> + <t,r5> + <BN(xb; gamma, beta), r6> + <BN(xb; gamma2 FROZEN, beta2), r7>

    options of a pass: a_grad (False: `a` does not require a gradient), frozen (names of weights with requires_grad False),
    use_y1 (False: the terms <y1,r1> and <u,r4> are left out -- W1's node then receives dy = None and only the gradient of hp).

THE CONV PART IS EXACT.  a, r in {-1, 0, 1}; W in {-1, 0, 1} g with g a power of two, a fraction DENSITY of them non-zero; bias
integers.  A value behind d weights is a multiple of g^d, d <= 3, so everything -- forward values, data gradients, parameter
gradients and every sum of them over passes -- is a multiple of GRID = g^3.  S is the same network evaluated on the absolute values
(ReLU masks replaced by 1) and accumulated by the same protocol; while S <= 2^24 GRID no partial sum in ANY order needs more than
24 bits, so fp32 with atomics, split maps, either stream and any number of in-place adds gives the float64 value bit for bit
(_conv_rule.assert_exact, asserted for every observation of every protocol).  The comparison is torch.equal.

THE BATCHNORM PART IS BOUNDED.  Per pass _norm_rule.grad_bounds (the one-launch kernels: both shapes are under 2048 rows); dxb is
the sum of two BatchNorms' dx: both bounds plus one rounding of the add; every accumulation into an existing gradient adds one
rounding of the running sum, u |sum|, u = 2^-24.  Nothing is taken from a kernel.

HALF TRAINING (half_train.conv) shares issue_wgrad and grad_slot: a two-layer network with binary16 activations and data gradients
(`half_values`: everything a multiple of g^2 and representable in binary16, asserted) runs the accumulation and autograd.grad protocols.

PROTOCOLS are functions of an engine (below); `RuleEngine` evaluates them on per-pass float64 gradients, holding storage the way
torch promises it (a kept `.grad` is one object that later passes add into; results of autograd.grad are the caller's own).  Each
MISTAKE changes what the RuleEngine does the way the named defect of the package would; `compare` must then fail.
"""
import numpy as np
import torch

import _conv_rule as R
import _norm_rule as N

K = 27
G = 0.5
GRID = G ** 3
DENSITY = 0.25
SHAPES = ((193, 16), (577, 32))            # (rows, channels): under / over functional.TINY_MAP_ROWS = 512, partial last tiles
PASSES = 3
CONV_PARAMS = ('W0', 'W1', 'W2', 'W3', 'Wb', 'bias')
BN_PARAMS = ('gamma', 'beta', 'beta2')     # (gamma2 is frozen)
OUTPUTS = ('y1', 'v', 's', 'u', 't')
VARIANTS = ('inplace', 'torch_add')
DEFAULT = {'a_grad': True, 'frozen': (), 'use_y1': True}
U = N.U


def _f(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


_cases = {}


def case(n, c, seed=0):
    """Tables, parameters and the inputs of PASSES passes (float32 tensors / arrays; the rule widens them exactly)."""
    key = (n, c, seed)
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng([31, n, c, seed])
    nbr = R.table('random', K, n, n, seed=seed + 5)
    tri = lambda shape: rng.integers(-1, 2, shape)
    sparse = lambda shape: tri(shape) * (rng.random(shape) < DENSITY)
    cs = {'n': n, 'c': c, 'nbr': nbr, 'rev': R.reverse_table(nbr, n),
          'params': {'W0': _f(sparse((K, c, c)) * G), 'W1': _f(sparse((K, c, c)) * G), 'W2': _f(sparse((K, c, c)) * G),
                     'W3': _f(sparse((K, c, c)) * G), 'Wb': _f(tri((c, c)) * G), 'bias': _f(rng.integers(-3, 4, (1, c)))},
          'passes': []}
    b0, b1 = N.bn_input(n, c, seed=900), N.bn_input(n, c, seed=901)
    cs['bn_params'] = {'gamma': b0['gamma'], 'beta': b0['beta'], 'gamma2': b1['gamma'], 'beta2': b1['beta'],
                       'rm0': b0['rm0'], 'rv0': b0['rv0']}
    for i in range(PASSES):
        p = {'a': _f(tri((n, c)))}
        for j in range(1, 6):
            p['r%d' % j] = _f(tri((n, c)))
        b = N.bn_input(n, c, seed=910 + i)
        p['xb'], p['r6'], p['r7'] = b['x'], b['dy'], b['res']
        cs['passes'].append(p)
    _cases[key] = cs
    return cs


# ----------------------------------------------------------------------------- one pass of the rule
def conv_pass(cs, i, variant, opts=None, absolute=False, mistake=None, h_saved=None):
    """(outputs, gradients) of the conv part of pass i in float64; gradients of what receives none are None.  absolute: the S of
    every entry instead (operands replaced by their absolute values, ReLU masks by 1).  mistake / h_saved: see MISTAKES."""
    o = dict(DEFAULT, **(opts or {}))
    nbr, n = cs['nbr'], cs['n']
    w = lambda t: t.double().abs() if absolute else t.double()
    P = {k: w(v) for k, v in cs['params'].items()}
    X = {k: w(v) for k, v in cs['passes'][i].items() if k in ('a', 'r1', 'r2', 'r3', 'r4', 'r5')}
    mask = (lambda t: torch.ones_like(t)) if absolute else (lambda t: (t > 0).double())
    fwd = lambda x, wt: R.conv_fwd(nbr, x, None, wt)
    dgrad = lambda dy, wt: R.conv_dgrad(nbr, dy, wt, n)
    wgrad = lambda x, dy: R.conv_wgrad(nbr, x, dy, torch.zeros(K, x.shape[1], dy.shape[1], dtype=torch.float64))
    h = fwd(X['a'], P['W0'])
    t = fwd(X['a'], P['W3'])
    y1 = fwd(h, P['W1'])
    z = h if variant == 'inplace' else h + t
    v = fwd(z, P['W2'])
    rv = v * mask(v)
    s = rv @ P['Wb'] + P['bias']
    out = {'y1': y1, 'v': v, 's': s, 't': t, 'u': fwd(y1, P['W0']) if o['use_y1'] else None}
    g = dict.fromkeys(CONV_PARAMS + ('a', 'W0_first', 'W0_second'))
    ds = X['r3']
    g['Wb'], g['bias'] = rv.t() @ ds, ds.sum(0, keepdim=True)
    dv = X['r2'] + (ds @ P['Wb'].t()) * mask(v)
    g['W2'] = wgrad(z, dv)
    dz = dgrad(dv, P['W2'])
    dt = X['r5'] + (dz if variant == 'torch_add' else 0.0)
    dh = dz
    if o['use_y1']:
        dy1 = X['r1'] + dgrad(X['r4'], P['W0'])
        g['W0_second'] = wgrad(y1, X['r4'])                          # (second in forward order: its backward runs first)
        g['W1'] = wgrad(h if h_saved is None else w(h_saved), dy1)
        d1 = dgrad(dy1, P['W1'])
        dh = dz + d1
        if mistake == 'inplace_on_shared_gradient' and variant == 'torch_add':
            dt = dt + d1                                             # W1's node added onto the tensor t's branch reads as well
    g['W3'] = wgrad(X['a'], dt)
    g['W0_first'] = wgrad(X['a'], dh)
    g['W0'] = g['W0_first'] + (g['W0_second'] if g['W0_second'] is not None else 0.0)
    if mistake == 'second_use_overwrites_slot':
        g['W0'] = g['W0_first']                                      # the later backward operator of W0 wrote the same slot
    if o['a_grad']:
        g['a'] = dgrad(dh, P['W0']) + dgrad(dt, P['W3'])
    for k in o['frozen']:
        g[k] = None
    return out, g


def bn_pass(cs, i):
    """({name: gradient}, {name: bound}) of the BatchNorm branch of pass i (numpy float64): gamma, beta, beta2, xb."""
    p, q = cs['passes'][i], cs['bn_params']
    x = p['xb']
    f1 = N.bn_forward(x, q['gamma'], q['beta'])
    b1 = N.bn_backward(x, q['gamma'], f1, p['r6'])
    e1 = N.grad_bounds(x, q['gamma'], f1, b1, 'one_launch')
    f2 = N.bn_forward(x, q['gamma2'], q['beta2'])
    b2 = N.bn_backward(x, q['gamma2'], f2, p['r7'])
    e2 = N.grad_bounds(x, q['gamma2'], f2, b2, 'one_launch')
    dx = b1['dx'] + b2['dx']
    g = {'gamma': b1['dgamma'], 'beta': b1['dbeta'], 'beta2': b2['dbeta'], 'xb': dx}
    e = {'gamma': e1['dgamma'], 'beta': e1['dbeta'], 'beta2': e2['dbeta'], 'xb': e1['dx'] + e2['dx'] + U * np.abs(dx)}
    return g, e


class Val:
    """A reference value with what it is held to: (value, S) -- exact, S the sum of absolute terms -- or (value, bound)."""
    __slots__ = ('v', 's', 'b')

    def __init__(self, v, s=None, b=None):
        self.v, self.s, self.b = v, s, b

    def copy(self):
        return Val(self.v.clone(), None if self.s is None else self.s.clone(), None if self.b is None else self.b.clone())

    def add_(self, o, rounded=True):
        """In place, the way autograd accumulates: exact values add their S; bounded ones their bounds plus one rounding of the sum."""
        self.v += o.v
        if self.s is not None:
            self.s += o.s
        else:
            self.b += o.b
            if rounded:
                self.b += U * self.v.abs()
        return self

    def scaled(self, k):
        return Val(self.v * k, None if self.s is None else self.s * k, None if self.b is None else self.b * k)


_pass_cache = {}


def pass_values(cs, i, variant, opts=None, mistake=None, h_saved_from=None):
    """{name: Val or None} for the outputs ('out.y1' ...) and the gradients of pass i.  Cached; treat as read-only."""
    o = dict(DEFAULT, **(opts or {}))
    key = (cs['n'], cs['c'], i, variant, o['a_grad'], tuple(o['frozen']), o['use_y1'], mistake, h_saved_from)
    if key in _pass_cache:
        return _pass_cache[key]
    hs = None
    if h_saved_from is not None:
        hs = R.conv_fwd(cs['nbr'], cs['passes'][h_saved_from]['a'], None, cs['params']['W0'])
    out, g = conv_pass(cs, i, variant, o, False, mistake, hs)
    sout, sg = conv_pass(cs, i, variant, o, True, mistake, hs)
    vals = {}
    for k in OUTPUTS:
        vals['out.' + k] = None if out[k] is None else Val(out[k], s=sout[k])
    for k in CONV_PARAMS + ('a', 'W0_first', 'W0_second'):
        vals[k] = None if g[k] is None else Val(g[k], s=sg[k])
    bg, be = bn_pass(cs, i)
    for k in BN_PARAMS + ('xb',):
        vals[k] = None if k in o['frozen'] else Val(torch.from_numpy(bg[k]).clone(), b=torch.from_numpy(np.broadcast_to(be[k], bg[k].shape).copy()))
    _pass_cache[key] = vals
    return vals


LEAVES = ('a', 'xb')
PARAMS = CONV_PARAMS + BN_PARAMS


# ----------------------------------------------------------------------------- engines and protocols
class RuleEngine:
    """The protocols' engine over float64 per-pass gradients, with torch's storage semantics: `.grad` of a parameter is ONE object
    from the pass that creates it until it is dropped, later passes add into it; each pass has leaves of its own."""

    def __init__(self, cs, variant, mistake=None, provider=None, params=PARAMS, leaves=LEAVES):
        """provider(i, opts) -> {name: Val or None}: another network's per-pass values (default: pass_values of this module's)."""
        self.cs, self.variant, self.mistake = cs, variant, mistake
        self.provider, self.params, self.leaves = provider, params, leaves
        self.grad = dict.fromkeys(params)          # name -> Val or None
        self.pending = []                          # passes whose forward has run and whose graph is alive
        self.stale = {}                            # slot_not_cleared: what the slots held when they should have been cleared
        self.handed = []                           # cleared_while_live: results of autograd_grad (Vals the caller holds)

    # -- a pass
    def forward(self, i, training=True, **opts):
        if self.mistake == 'slab_piece_reused':    # this pass's convolutions were given the pieces a pending pass saved for its
            for h in self.pending:                 # backward: that pass now differentiates W1's layer at THIS pass's h
                h['h_saved_from'] = i
        if not training:                           # an inference pass: no graph, nothing to differentiate
            return None
        if self.mistake == 'cleared_while_live':   # begin_pass cleared the buffer the caller's tensors view
            for vals in self.handed:
                for v in vals.values():
                    if v is not None and v.s is not None:
                        v.v.zero_()
        h = {'i': i, 'opts': opts, 'h_saved_from': None, 'leaf': dict.fromkeys(self.leaves), 'runs': 0}
        self.pending.append(h)
        return h

    def _values(self, h):
        if self.provider is not None:
            return self.provider(h['i'], h['opts'])
        m = self.mistake if self.mistake in ('inplace_on_shared_gradient', 'second_use_overwrites_slot') else None
        return pass_values(self.cs, h['i'], self.variant, h['opts'], m, h['h_saved_from'] if self.mistake == 'slab_piece_reused' else None)

    def outputs(self, h):
        return {k: v for k, v in self._values(h).items() if k.startswith('out.') and v is not None}

    def backward(self, *hs, retain_graph=False):
        """One backward() of the sum of the losses of `hs`."""
        for h in hs:
            vals = self._values(h)
            for k in self.params:
                v = vals[k]
                if v is None:
                    continue
                if self.mistake == 'add_before_wgrad' and self.grad[k] is not None and k.startswith('W'):
                    continue                       # the add ran before the weight-gradient kernel had written: the term is missing
                if self.grad[k] is None:
                    self.grad[k] = v.copy()
                    if self.mistake == 'slot_not_cleared' and k in self.stale:
                        self.grad[k].v += self.stale[k]
                else:
                    self.grad[k].add_(v)
            for k in self.leaves:
                if vals[k] is not None:
                    h['leaf'][k] = vals[k].copy() if h['leaf'][k] is None else h['leaf'][k].add_(vals[k])
            h['runs'] += 1
            if not retain_graph:
                self.pending = [q for q in self.pending if q is not h]

    def autograd_grad(self, h):
        """torch.autograd.grad(loss, params + leaves): the caller's own tensors; .grad untouched."""
        vals = self._values(h)
        self.pending = [q for q in self.pending if q is not h]
        res = {k: (None if vals[k] is None else vals[k].copy()) for k in tuple(self.params) + tuple(self.leaves)}
        self.handed.append(res)
        return res

    # -- what the caller does with gradients
    def grads(self):
        """The `.grad` objects themselves (aliases: what `g1 = p.grad` keeps)."""
        return dict(self.grad)

    def snapshot(self):
        return {k: (None if v is None else v.copy()) for k, v in self.grad.items()}

    def leaf_grads(self, h):
        return {k: (None if v is None else v.copy()) for k, v in h['leaf'].items()}

    def drop_grads(self):
        if self.mistake == 'slot_not_cleared':
            self.stale = {k: v.v.clone() for k, v in self.grad.items() if v is not None and v.s is not None}
        self.grad = dict.fromkeys(self.params)

    def zero_grads(self):
        for v in self.grad.values():
            if v is not None:
                v.v.zero_()
                (v.s if v.s is not None else v.b).zero_()

    def same_memory(self, before, after):
        return all(before[k] is after[k] for k in before)

    def expect(self, cond, what):
        assert cond, what


def _obs(obs, tag, d):
    for k, v in d.items():
        obs['%s.%s' % (tag, k)] = v


def p1_step_loop(e):
    obs = {}
    for i in range(PASSES):
        e.drop_grads()
        h = e.forward(i)
        _obs(obs, 'pass%d' % i, e.outputs(h))
        e.backward(h)
        _obs(obs, 'pass%d' % i, e.snapshot())
        _obs(obs, 'pass%d' % i, e.leaf_grads(h))
    return obs


def _kept(e, between):
    obs = {}
    g1 = None
    for i in range(PASSES):
        if i:
            between()
        h = e.forward(i)
        e.backward(h)
        if i == 0:
            g1 = e.grads()
        else:
            e.expect(e.same_memory(g1, e.grads()), '.grad moved to other memory in pass %d' % i)
        _obs(obs, 'after%d' % i, e.snapshot())
        _obs(obs, 'pass%d' % i, e.leaf_grads(h))
    _obs(obs, 'g1', g1)                              # the objects saved after pass 1: the running value, not garbage
    return obs


def p2_accumulation(e):
    return _kept(e, lambda: None)


def p3_zero_in_place(e):
    return _kept(e, e.zero_grads)


def p4_autograd_grad(e):
    obs = {}
    first = e.autograd_grad(e.forward(0))
    e.expect(all(v is None for v in e.grads().values()), 'autograd.grad left a .grad behind')
    h = e.forward(1)
    e.backward(h)
    _obs(obs, 'second', e.snapshot())
    _obs(obs, 'second', e.leaf_grads(h))
    h = e.forward(2)                                 # a third pass while both earlier results are held
    e.backward(h)
    _obs(obs, 'third', e.snapshot())
    _obs(obs, 'first', first)                        # read LAST: still pass 1's
    return obs


def p5_summed_loss(e):
    obs = {}
    ha, hb = e.forward(0), e.forward(1)
    _obs(obs, 'A', e.outputs(ha))
    _obs(obs, 'B', e.outputs(hb))
    e.backward(ha, hb)
    _obs(obs, 'sum', e.snapshot())
    _obs(obs, 'A', e.leaf_grads(ha))
    _obs(obs, 'B', e.leaf_grads(hb))
    return obs


def p5_reversed_backwards(e):
    obs = {}
    ha, hb = e.forward(0), e.forward(1)
    e.backward(hb)
    _obs(obs, 'afterB', e.snapshot())
    e.backward(ha)
    _obs(obs, 'afterA', e.snapshot())
    _obs(obs, 'A', e.leaf_grads(ha))
    _obs(obs, 'B', e.leaf_grads(hb))
    return obs


def p6_retained_graph(e):
    obs = {}
    h = e.forward(0)
    e.backward(h, retain_graph=True)
    e.backward(h)
    _obs(obs, 'twice', e.snapshot())
    _obs(obs, 'twice', e.leaf_grads(h))
    return obs


def p7_shared_weight(e):
    """W0 serves two layers of every pass; here one pass, and the next one after a step, so that the second slot is clean."""
    obs = {}
    for i in (2, 0):
        e.drop_grads()
        h = e.forward(i)
        e.backward(h)
        _obs(obs, 'pass%d' % i, {'W0': e.snapshot()['W0']})
        _obs(obs, 'pass%d' % i, e.leaf_grads(h))
    return obs


def p8_inference_between(e):
    obs = {}
    h = e.forward(0)
    e.forward(1, training=False)
    _obs(obs, 'train', e.outputs(h))
    e.backward(h)
    _obs(obs, 'train', e.snapshot())
    _obs(obs, 'train', e.leaf_grads(h))
    return obs


def p9_partial_gradients(e):
    obs = {}
    for tag, i, opts in (('nograd_a', 0, {'a_grad': False, 'frozen': ('W2',)}), ('alias_only', 1, {'use_y1': False}),
                         ('frozen_shared', 2, {'frozen': ('W0', 'beta')})):
        e.drop_grads()
        h = e.forward(i, **opts)
        e.backward(h)
        _obs(obs, tag, e.snapshot())
        _obs(obs, tag, e.leaf_grads(h))
    return obs


PROTOCOLS = {'P1_step_loop': p1_step_loop, 'P2_accumulation': p2_accumulation, 'P3_zero_in_place': p3_zero_in_place,
             'P4_autograd_grad': p4_autograd_grad, 'P5_summed_loss': p5_summed_loss, 'P5_reversed_backwards': p5_reversed_backwards,
             'P6_retained_graph': p6_retained_graph, 'P7_shared_weight': p7_shared_weight, 'P8_inference_between': p8_inference_between,
             'P9_partial_gradients': p9_partial_gradients}

# mistake -> a protocol and variant under which it must show
MISTAKES = {'slot_not_cleared': ('P1_step_loop', 'inplace'), 'cleared_while_live': ('P4_autograd_grad', 'inplace'),
            'add_before_wgrad': ('P2_accumulation', 'inplace'), 'inplace_on_shared_gradient': ('P1_step_loop', 'torch_add'),
            'second_use_overwrites_slot': ('P7_shared_weight', 'inplace'), 'slab_piece_reused': ('P8_inference_between', 'inplace')}

_expected = {}


def expected(n, c, variant, protocol):
    """{observation: Val or None} of a protocol, with the exactness condition asserted for every exact entry.  Cached."""
    key = (n, c, variant, protocol)
    if key not in _expected:
        obs = PROTOCOLS[protocol](RuleEngine(case(n, c), variant))
        for k, v in obs.items():
            if v is not None and v.s is not None:
                try:
                    R.assert_exact(v.s, v.v, GRID)
                except R.NotExact as err:
                    raise R.NotExact('%s: %s' % (k, err))
        _expected[key] = obs
    return _expected[key]


# ----------------------------------------------------------------------------- the half-precision entry (half_train.conv)
HALF_GRID = G ** 2
HALF_PROTOCOLS = ('P2_accumulation', 'P4_autograd_grad')


def half_values(cs, i):
    """h = conv(a, W0), y = conv(h, W1), loss = <y, r1> with binary16 activations and gradients, fp32 weight gradients, loss
    scale 1: everything a multiple of HALF_GRID = g^2; what is stored in binary16 (h, y, dh, da) must be representable
    (_conv_rule.assert_half_exact on each at its own grid)."""
    key = ('half', cs['n'], cs['c'], i)
    if key in _pass_cache:
        return _pass_cache[key]
    nbr, n = cs['nbr'], cs['n']
    vals = []
    for absolute in (False, True):
        w = lambda t: t.double().abs() if absolute else t.double()
        a, r, w0, w1 = w(cs['passes'][i]['a']), w(cs['passes'][i]['r1']), w(cs['params']['W0']), w(cs['params']['W1'])
        zero = torch.zeros(K, cs['c'], cs['c'], dtype=torch.float64)
        h = R.conv_fwd(nbr, a, None, w0)
        y = R.conv_fwd(nbr, h, None, w1)
        dh = R.conv_dgrad(nbr, r, w1, n)
        da = R.conv_dgrad(nbr, dh, w0, n)
        if not absolute:
            for t, grid in ((h, G), (y, G * G), (dh, G), (da, G * G)):
                R.assert_half_exact(t, grid)
        vals.append({'out.y': y, 'W1': R.conv_wgrad(nbr, h, r, zero), 'W0': R.conv_wgrad(nbr, a, dh, zero), 'a': da})
    _pass_cache[key] = {k: Val(vals[0][k], s=vals[1][k]) for k in vals[0]}
    return _pass_cache[key]


def half_expected(n, c, protocol):
    key = ('half', n, c, protocol)
    if key not in _expected:
        cs = case(n, c)
        obs = PROTOCOLS[protocol](RuleEngine(cs, None, provider=lambda i, opts: half_values(cs, i), params=('W0', 'W1'), leaves=('a',)))
        for k, v in obs.items():
            if v is not None:
                R.assert_exact(v.s, v.v, HALF_GRID)
        _expected[key] = obs
    return _expected[key]


def compare(got, want):
    """The one comparison of the CPU and the GPU tests: got {observation: tensor or None} against want {observation: Val or
    None}.  Exact entries: torch.equal on the float64 widening; bounded ones: every element inside its bound.  Returns the list
    of failures (empty: the same)."""
    bad = []
    if sorted(got) != sorted(want):
        return ['observations differ: %s' % sorted(set(got) ^ set(want))]
    for k in sorted(want):
        g, w = got[k], want[k]
        if (g is None) != (w is None):
            bad.append('%s: %s, expected %s' % (k, 'None' if g is None else 'a tensor', 'None' if w is None else 'a tensor'))
            continue
        if w is None:
            continue
        g = g.detach().cpu().double()
        if tuple(g.shape) != tuple(w.v.shape):
            bad.append('%s: shape %s, expected %s' % (k, tuple(g.shape), tuple(w.v.shape)))
        elif w.s is not None:
            if not torch.equal(g, w.v):
                bad.append('%s: %d elements differ, max %.6g' % (k, int((g != w.v).sum()), float((g - w.v).abs().max())))
        else:
            r = N.ratio((g - w.v).abs().numpy(), w.b.numpy())
            if not r <= 1.0:
                bad.append('%s: error / bound = %.3g' % (k, r))
    return bad


def conv_only(obs):
    """The exact (convolution) observations alone -- for an engine that has no BatchNorm branch."""
    bn = BN_PARAMS + ('xb',)
    return {k: v for k, v in obs.items() if k.rsplit('.', 1)[-1] not in bn}


class TorchEngine:
    """The protocols' engine over real autograd: `run_pass(i, training, opts)` builds the graph of pass i from `params`
    ({name: leaf tensor}) and returns (loss, {output name: tensor}, {leaf name: tensor}); `open_pass(training)` is what the model
    does at the start of a forward pass.  Snapshots are clones made on the current stream; nothing here synchronises a device."""

    def __init__(self, params, run_pass, open_pass=None):
        self.params, self.run_pass, self.open_pass = params, run_pass, open_pass or (lambda training: None)

    def forward(self, i, training=True, **opts):
        o = dict(DEFAULT, **opts)
        if not training:
            with torch.no_grad():
                self.open_pass(False)
                self.run_pass(i, False, o)
            return None
        self.open_pass(True)
        frozen = [self.params[k] for k in o['frozen'] if k in self.params]
        for p in frozen:
            p.requires_grad_(False)
        try:
            loss, out, leaf = self.run_pass(i, True, o)
        finally:
            for p in frozen:
                p.requires_grad_(True)
        return {'loss': loss, 'out': out, 'leaf': leaf}

    def outputs(self, h):
        return {'out.' + k: v.detach() for k, v in h['out'].items() if v is not None}

    def backward(self, *hs, retain_graph=False):
        loss = hs[0]['loss']
        for h in hs[1:]:
            loss = loss + h['loss']
        loss.backward(retain_graph=retain_graph)

    def autograd_grad(self, h):
        named = [(k, p) for k, p in self.params.items()] + [(k, t) for k, t in h['leaf'].items() if t.requires_grad]
        res = torch.autograd.grad(h['loss'], [t for _, t in named], allow_unused=True)
        out = dict.fromkeys(list(self.params) + list(h['leaf']))
        out.update({k: g for (k, _), g in zip(named, res)})
        return out

    def grads(self):
        return {k: p.grad for k, p in self.params.items()}

    def snapshot(self):
        return {k: (None if p.grad is None else p.grad.clone()) for k, p in self.params.items()}

    def leaf_grads(self, h):
        return {k: (None if t.grad is None else t.grad.clone()) for k, t in h['leaf'].items()}

    def drop_grads(self):
        for p in self.params.values():
            p.grad = None

    def zero_grads(self):
        for p in self.params.values():
            if p.grad is not None:
                p.grad.zero_()

    def same_memory(self, before, after):
        return all(before[k] is after[k] and (before[k] is None or before[k].data_ptr() == after[k].data_ptr()) for k in before)

    def expect(self, cond, what):
        assert cond, what
