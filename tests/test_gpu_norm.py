"""The BatchNorm, segment-pooling and elementwise kernels of box2mask_amd/csrc/norm.hip against the float64 rule of
tests/_norm_rule.py, on inputs whose conditioning is set PER COLUMN (|mean| / sigma = 0, 0.5, 30, 100, 1000, a constant column,
sigma = 1e-4 and 1e4 in every tensor) and at the shapes where the kernels change path: the one-launch kernels, the two-stage
kernels from x, the statistics from per-tile sums (one kernel and two launches; once behind a real convolution), the SyncBN
entries of the two-stage, tile-sum and one-launch forms in one process, eval mode, the pair, leading dimensions wider than the rows.  Every bound is a call into _norm_rule
(derivations there; tests/test_norm_rule.py shows on the CPU that they are neither too tight nor too loose); the ReLU mask of the
backward quantities is the device's own y > 0, which must be the rule's outside the borderline elements.

Each BatchNorm case runs twice: through the C entries (constants, running statistics, strides, poisoned surroundings) and through
`functional.batch_norm` with the switches that select the path; the two must agree bit for bit (the kernels are deterministic).
`pytest -s` prints error / bound of every compared quantity.

Worst error / bound measured on an MI355X (all cases of a family): the six constants 0.25 everywhere -- half an ulp32, i.e. the
correctly rounded fp64 value on every path, the |mean| = 1000 sigma columns of the two-stage-from-x kernel included (which summed
in fp32 chains before this file existed; SIMULATED on the CPU, not measured on a device, that misses the invstd bound there by
four orders of magnitude: tests/test_norm_rule.py) --; y 0.32,
dx 0.45, dgamma 0.29, dbeta 0.24 (the SyncBN entry cases: y 0.29, dx 0.36); behind the convolution y 0.14, dx 0.13; the pair y 0.23, dx 0.29, dgamma 0.04; eval y 0.31,
dx 0.48, dgamma 0.08, dbeta 0.08; segment mean 0.26, its gradient 0.50 (of one ulp32); everything exact was exact.
"""
import functools

import numpy as np
import pytest
import torch

import _norm_rule as R

pytestmark = pytest.mark.gpu

ENV = {'small': {}, 'small16k': {'B2M_BN_SMALL_ROWS': '16384'}, 'stats': {'B2M_BN_SMALL_ROWS': '0'},
       'tiles': {'B2M_BN_SMALL_ROWS': '0'}, 'tiles2': {'B2M_BN_SMALL_ROWS': '0', 'B2M_BN_TS_ONE': '0'}, 'sync': {}, 'synctiles': {}, 'syncsmall': {}, 'eval': {}}
POISON = -777.25


@functools.lru_cache(maxsize=2)
def inputs(name):
    return R.bn_case_input(name)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Window:
    """An (n, c) tensor as a column window of a wider, poisoned (n, ld) buffer (ld = c: the tensor itself)."""

    def __init__(self, n, c, ld_kind, data=None):
        ld, off = {None: (c, 0), 'c+4': (c + 4, 4), '2c': (2 * c, c)}[ld_kind]
        self.buf = torch.full((n, ld), POISON, dtype=torch.float32, device='cuda')
        self.t = self.buf[:, off:off + c]
        self.cols = (off, off + c)
        if data is not None:
            self.t.copy_(dev(data))

    def ptr(self):
        return self.t.data_ptr()

    def ld(self):
        return self.t.stride(0)

    def value(self):
        keep = torch.ones(self.buf.shape[1], dtype=torch.bool)
        keep[self.cols[0]:self.cols[1]] = False
        assert bool((self.buf[:, keep.cuda()] == POISON).all()), 'written outside the window'
        return self.t.cpu().numpy().copy()


def run_entries(name, monkeypatch):
    """The case through the C entries, as functional._BatchNorm strings them together."""
    from box2mask_amd import functional as F_
    call = F_._call
    spec, inp = R.BN_CASES[name], inputs(name)
    for k, v in ENV[spec['path']].items():
        monkeypatch.setenv(k, v)
    n, c, ldk, relu, has_res, path = spec['n'], spec['c'], spec['ld'], spec['relu'], spec['res'], spec['path']
    x, dy = Window(n, c, ldk, inp['x']), Window(n, c, ldk, inp['dy'])
    res = Window(n, c, ldk, inp['res']) if has_res else None
    y, dx = Window(n, c, ldk), Window(n, c, ldk)
    dres = Window(n, c, ldk) if has_res else None
    gam, bet, rm, rv = dev(inp['gamma']), dev(inp['beta']), dev(inp['rm0']), dev(inp['rv0'])
    f32 = lambda: torch.full((c + 8,), POISON, device='cuda')[4:4 + c]                 # (16-byte aligned inside its buffer)
    mean, inv, sc, sh, dbeta, dgamma = f32(), f32(), f32(), f32(), f32(), f32()
    P = lambda w: w.ptr() if w is not None else None
    L = lambda w: w.ld() if w is not None else 0
    consts = (gam.data_ptr(), bet.data_ptr(), R.EPS, R.MOMENTUM, rm.data_ptr(), rv.data_ptr(), mean.data_ptr(), inv.data_ptr(),
              sc.data_ptr(), sh.data_ptr())
    use_y = relu and has_res                                                           # (else the mask is recomputed from x)
    mask = (None, None) if (use_y or not relu) else (sc.data_ptr(), sh.data_ptr())
    yarg = (y.ptr(), y.ld()) if use_y else (None, 0)
    partial = torch.empty(2 * c * 4096, dtype=torch.float64, device='cuda')
    sums = torch.empty(2 * c, dtype=torch.float64, device='cuda')
    count_dev = None
    if path in ('small', 'small16k'):
        call('b2m_bn_small_fwd', x.ptr(), x.ld(), n, c, *consts, P(res), L(res), int(relu), y.ptr(), y.ld())
        call('b2m_bn_small_bwd', dy.ptr(), dy.ld(), *yarg, x.ptr(), x.ld(), n, c, mean.data_ptr(), inv.data_ptr(), gam.data_ptr(),
             int(relu), *mask, dbeta.data_ptr(), dgamma.data_ptr(), dx.ptr(), dx.ld(), P(dres), L(dres))
    elif path == 'syncsmall':                   # the one-launch kernels cut in two; an equal second rank "all-reduced" in between
        xchg = torch.empty(2 * c + 1, dtype=torch.float64, device='cuda')
        call('b2m_bn_small_fwd_stats', x.ptr(), x.ld(), n, c, xchg.data_ptr())
        xchg *= 2
        call('b2m_bn_small_fwd_apply', xchg.data_ptr(), x.ptr(), x.ld(), n, c, *consts, P(res), L(res), int(relu), y.ptr(), y.ld())
        head = (dy.ptr(), dy.ld(), *yarg, x.ptr(), x.ld(), n, c, mean.data_ptr(), inv.data_ptr(), gam.data_ptr(), int(relu), *mask)
        xb = torch.empty(2 * c, dtype=torch.float64, device='cuda')
        call('b2m_bn_small_bwd_phase', 1, *head, dbeta.data_ptr(), dgamma.data_ptr(), None, 0, None, 0, xb.data_ptr(), None)
        xb *= 2
        call('b2m_bn_small_bwd_phase', 2, *head, None, None, dx.ptr(), dx.ld(), P(dres), L(dres), xb.data_ptr(),
             xchg.data_ptr() + 8 * 2 * c)
    else:
        if path == 'stats':
            call('b2m_bn_stats_finalize', x.ptr(), x.ld(), n, c, partial.data_ptr(), None, *consts)
        elif path in ('tiles', 'tiles2'):
            ts = dev(R.tile_sums(inp['x']))
            call('b2m_bn_tilestats_finalize', ts.data_ptr(), ts.shape[0], n, c, partial.data_ptr(), None, *consts)
        else:                                   # sync: this rank's sums, "all-reduced" with an equal second rank on the device
            stats = torch.empty(2 * c + 1, dtype=torch.float64, device='cuda')
            if path == 'synctiles':
                ts = dev(R.tile_sums(inp['x']))
                call('b2m_bn_tilestats', ts.data_ptr(), ts.shape[0], c, partial.data_ptr(), stats.data_ptr())
            else:
                call('b2m_bn_stats', x.ptr(), x.ld(), n, c, partial.data_ptr(), stats.data_ptr())
            stats[2 * c:].fill_(float(n))
            stats *= 2
            count_dev = stats[2 * c:]
            call('b2m_bn_finalize', stats.data_ptr(), 0.0, count_dev.data_ptr(), c, *consts)
        call('b2m_bn_apply', x.ptr(), x.ld(), n, c, sc.data_ptr(), sh.data_ptr(), P(res), L(res), int(relu), y.ptr(), y.ld())
        call('b2m_bn_bwd_reduce', dy.ptr(), dy.ld(), *yarg, x.ptr(), x.ld(), n, c, mean.data_ptr(), inv.data_ptr(), int(relu), *mask,
             partial.data_ptr(), sums.data_ptr(), dbeta.data_ptr(), dgamma.data_ptr())
        gsums = sums * 2 if count_dev is not None else sums
        call('b2m_bn_bwd_apply', dy.ptr(), dy.ld(), *yarg, x.ptr(), x.ld(), n, c, mean.data_ptr(), inv.data_ptr(), gam.data_ptr(),
             gsums.data_ptr(), float(n), count_dev.data_ptr() if count_dev is not None else None, int(relu), *mask, dx.ptr(), dx.ld(),
             P(dres), L(dres))
    torch.cuda.synchronize()
    got = {'mean': mean, 'invstd': inv, 'scale': sc, 'shift': sh, 'running_mean': rm, 'running_var': rv, 'dbeta': dbeta,
           'dgamma': dgamma}
    got = {k: v.cpu().numpy().copy() for k, v in got.items()}
    got.update(y=y.value(), dx=dx.value())
    if has_res:
        got['dres'] = dres.value()
    for w, src in ((x, inp['x']), (dy, inp['dy'])):
        assert np.array_equal(w.value(), src), 'an input was modified'
    return got


def run_functional(name, monkeypatch):
    from box2mask_amd import functional as F_
    spec, inp = R.BN_CASES[name], inputs(name)
    for k, v in ENV[spec['path']].items():
        monkeypatch.setenv(k, v)
    n, c = spec['n'], spec['c']
    training = not spec.get('eval')
    x = dev(inp['x']).requires_grad_(True)
    res = dev(inp['res']).requires_grad_(True) if spec['res'] else None
    gam, bet = dev(inp['gamma']).requires_grad_(True), dev(inp['beta']).requires_grad_(True)
    rm, rv = dev(inp['rm0']), dev(inp['rv0'])
    if spec['path'] in ('tiles', 'tiles2'):
        ts = dev(R.tile_sums(inp['x'])).reshape(-1, 2, c)
        x._b2m_tile_stats = (ts, ts.shape[0])
    launched = []
    real = F_._call
    monkeypatch.setattr(F_, '_call', lambda nm, *a, **k: (launched.append(nm), real(nm, *a, **k))[1])
    y = F_.batch_norm(x, gam, bet, rm, rv, training, R.MOMENTUM, R.EPS, residual=res, relu=spec['relu'])
    y.backward(dev(inp['dy']))
    torch.cuda.synchronize()
    monkeypatch.setattr(F_, '_call', real)
    first = {'small': 'b2m_bn_small_fwd', 'small16k': 'b2m_bn_small_fwd', 'stats': 'b2m_bn_stats_finalize',
             'tiles': 'b2m_bn_tilestats_finalize', 'tiles2': 'b2m_bn_tilestats_finalize', 'eval': 'b2m_bn_finalize'}[spec['path']]
    assert launched[0] == first, launched
    got = {'y': y, 'dx': x.grad, 'dgamma': gam.grad, 'dbeta': bet.grad}
    if training:
        got.update(running_mean=rm, running_var=rv)
    if res is not None:
        got['dres'] = res.grad
    return {k: v.detach().cpu().numpy().copy() for k, v in got.items()}


@pytest.mark.parametrize('name', sorted(k for k, s in R.BN_CASES.items() if not s.get('eval')))
def test_batch_norm_training_matches_rule(name, monkeypatch):
    spec, inp = R.BN_CASES[name], inputs(name)
    got = run_entries(name, monkeypatch)
    bad, share = R.bn_check(name, inp, spec, got)
    assert not bad, (name, bad)
    assert share <= 1e-3
    if not spec['path'].startswith('sync'):                                # (functional's SyncBN needs a process group: tests/test_gpu_dp.py)
        fun = run_functional(name, monkeypatch)
        bad2, _ = R.bn_check(name + ' functional', inp, spec, fun)
        assert not bad2, (name, bad2)
        for k, v in fun.items():
            assert np.array_equal(v, got[k]), 'functional and the C entries differ in %s' % k


@pytest.mark.parametrize('name', sorted(k for k, s in R.BN_CASES.items() if s.get('eval')))
def test_batch_norm_eval_matches_rule(name, monkeypatch):
    spec, inp = R.BN_CASES[name], inputs(name)
    from box2mask_amd import functional as F_
    c = spec['c']
    sc, sh = torch.empty(c, device='cuda'), torch.empty(c, device='cuda')
    gam, bet, rm, rv = dev(inp['gamma']), dev(inp['beta']), dev(inp['rm0']), dev(inp['rv0'])
    F_._call('b2m_bn_finalize', None, 1.0, None, c, gam.data_ptr(), bet.data_ptr(), R.EPS, 0.0, rm.data_ptr(), rv.data_ptr(), None, None,
             sc.data_ptr(), sh.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(rm.cpu().numpy(), inp['rm0']) and np.array_equal(rv.cpu().numpy(), inp['rv0'])    # eval mode leaves them alone
    got = run_functional(name, monkeypatch)
    got.update(scale=sc.cpu().numpy(), shift=sh.cpu().numpy())
    bad, share = R.bn_check(name, inp, spec, got)
    assert not bad, (name, bad)
    assert share <= 1e-3


@pytest.mark.parametrize('name', sorted(R.PAIR_CASES))
def test_batch_norm_pair_matches_rule(name):
    from box2mask_amd import functional as F_
    a, b = R.pair_case_input(name)
    relu = R.PAIR_CASES[name][2]
    t = {}
    for s, inp in (('a', a), ('b', b)):
        t[s] = dict(x=dev(inp['x']).requires_grad_(True), g=dev(inp['gamma']).requires_grad_(True),
                    b=dev(inp['beta']).requires_grad_(True), rm=dev(inp['rm0']), rv=dev(inp['rv0']))
    side = lambda s: (t[s]['g'], t[s]['b'], t[s]['rm'], t[s]['rv'], R.MOMENTUM, R.EPS)
    launched = []
    real = F_._call
    F_._call = lambda nm, *args, **k: (launched.append(nm), real(nm, *args, **k))[1]
    try:
        y = F_.batch_norm_pair(t['a']['x'], side('a'), t['b']['x'], side('b'), True, relu=relu)
        y.backward(dev(a['dy']))
        torch.cuda.synchronize()
    finally:
        F_._call = real
    assert 'b2m_bn_apply2' in launched and 'b2m_bn_bwd_reduce2' in launched and 'b2m_bn_bwd_apply2' in launched, launched
    got = {'y': y}
    for s in 'ab':
        got.update({'dx_' + s: t[s]['x'].grad, 'dgamma_' + s: t[s]['g'].grad, 'dbeta_' + s: t[s]['b'].grad,
                    'running_mean_' + s: t[s]['rm'], 'running_var_' + s: t[s]['rv']})
    got = {k: v.detach().cpu().numpy() for k, v in got.items()}
    bad, share = R.pair_check(name, a, b, relu, got)
    assert not bad, (name, bad)
    assert share <= 1e-3


# ------------------------------------------------------------------ statistics a convolution left behind
def test_batch_norm_behind_a_convolution_with_offset_inputs():
    """sparse_conv(collect_stats=True) -> batch_norm on the 12 k-row map of test_gpu_ops: the statistics come from the per-tile
    column sums of the convolution's epilogue.  The inputs sit at 20 +- 1 and the centre tap carries a column offset, so the
    output columns have |mean| / sigma >= 30 (checked on the oracle's output): the constants must still be those of the
    exact statistics OF THE DEVICE'S OWN convolution output."""
    from box2mask_amd import functional as F_
    from box2mask_amd import synth
    from box2mask_amd.sparse import CoordinateManager
    from oracle import sparse_ref as S
    b = synth.make_batch(2, seed0=0, target_voxels=6000, pts_per_m2=6000.0)
    m = CoordinateManager(b['vox_coords'])
    h = S.Hierarchy(b['vox_coords'].numpy(), n_levels=1)
    n, c = h.n(0), 32
    assert n > 8192
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, c, generator=g) + 20.0
    w = torch.randn(27, c, c, generator=g) * 0.01
    w[13] += 1.0
    ref = S.conv_nbr(x.double(), w.double(), h.k3(0), None).numpy()
    assert float((np.abs(ref.mean(0)) / ref.std(0)).min()) >= 30.0
    rb = m.rulebook_same(0, 3)
    conv = F_.sparse_conv(x.cuda(), None, w.cuda(), None, rb, rb, True, n, collect_stats=True)
    assert getattr(conv, '_b2m_tile_stats', None) is not None, 'the convolution left no tile sums'
    rng = np.random.default_rng(11)
    inp = {'x': conv.cpu().numpy(), 'gamma': (rng.random(c) + 0.5).astype(np.float32), 'beta': (rng.random(c) + 0.1).astype(np.float32),
           'rm0': np.zeros(c, dtype=np.float32), 'rv0': np.ones(c, dtype=np.float32),
           'dy': rng.standard_normal((n, c)).astype(np.float32), 'res': None}
    assert float(np.abs(inp['x'] - ref).max()) <= 1e-3 * float(np.abs(ref).max())         # (the convolution itself: test_gpu_ops)
    spec = {'relu': True, 'res': False, 'chain': 'two_stage'}
    xg = conv.detach().requires_grad_(True)
    xg._b2m_tile_stats = conv._b2m_tile_stats
    gam, bet = dev(inp['gamma']).requires_grad_(True), dev(inp['beta']).requires_grad_(True)
    rm, rv = dev(inp['rm0']), dev(inp['rv0'])
    launched = []
    real = F_._call
    F_._call = lambda nm, *a, **k: (launched.append(nm), real(nm, *a, **k))[1]
    try:
        y = F_.batch_norm(xg, gam, bet, rm, rv, True, R.MOMENTUM, R.EPS, relu=True)
        y.backward(dev(inp['dy']))
        torch.cuda.synchronize()
    finally:
        F_._call = real
    assert launched[0] == 'b2m_bn_tilestats_finalize', launched
    got = {'y': y, 'dx': xg.grad, 'dgamma': gam.grad, 'dbeta': bet.grad, 'running_mean': rm, 'running_var': rv}
    got = {k: v.detach().cpu().numpy() for k, v in got.items()}
    bad, share = R.bn_check('conv -> bn', inp, spec, got)
    assert not bad, bad
    assert share <= 1e-3


# ------------------------------------------------------------------ segment pooling
def run_pool_entries(case, mode, window=False):
    from box2mask_amd import functional as F_
    call = F_._call
    n, c, n_seg = case['n'], case['c'], case['n_seg']
    m = 0 if mode == 'avg' else 1
    if window and n:
        wide = torch.full((n, c + 5), POISON, device='cuda')
        x = wide[:, 3:3 + c]
        x.copy_(dev(case['x']))
    else:
        x = dev(case['x'])
    ids = dev(case['ids'])
    out = torch.full((max(n_seg, 1), c), POISON, device='cuda')
    counts = torch.full((max(n_seg, 1),), -5, dtype=torch.int32, device='cuda')
    argmax = torch.full((max(n_seg * c, 1),), -7, dtype=torch.int32, device='cuda')
    scratch = torch.empty(max(n_seg * c, 1), dtype=torch.int64, device='cuda')
    dx = torch.full((max(n, 1), c), POISON, device='cuda')
    dout = dev(case['dout']) if n_seg else torch.zeros(1, c, device='cuda')
    ptr = lambda t: t.data_ptr() if t.numel() else None
    call('b2m_segment_pool_fwd', ptr(x), x.stride(0) if n else c, n, c, ptr(ids), n_seg, m, out.data_ptr(), counts.data_ptr(),
         argmax.data_ptr(), scratch.data_ptr())
    call('b2m_segment_pool_bwd', dout.data_ptr(), n, c, ptr(ids), n_seg, m, counts.data_ptr(), argmax.data_ptr(), dx.data_ptr(), c)
    torch.cuda.synchronize()
    got = {'out': out[:n_seg].cpu().numpy(), 'counts': counts[:n_seg].cpu().numpy(), 'dx': dx[:n].cpu().numpy()}
    if m:
        got['argmax'] = argmax[:n_seg * c].cpu().numpy().reshape(n_seg, c)
    if n_seg == 0:
        assert float(out[0, 0]) == POISON and int(counts[0]) == -5
    if n == 0:
        assert float(dx[0, 0]) == POISON
    return got


def run_pool_functional(case, mode):
    from box2mask_amd import functional as F_
    x = dev(case['x']).requires_grad_(True)
    out = F_.segment_pool(x, dev(case['ids']), case['n_seg'], mode)
    (out * dev(case['dout'])).sum().backward()
    torch.cuda.synchronize()
    dx = x.grad.cpu().numpy() if x.grad is not None else np.zeros(case['x'].shape, dtype=np.float32)     # (no rows: autograd may skip)
    return {'out': out.detach().cpu().numpy(), 'dx': dx}


@pytest.mark.parametrize('name', sorted(R.SEG_CASES))
def test_segment_pool_matches_rule(name, monkeypatch):
    for mode, flavours in (('avg', ('plain',)), ('max', ('plain', 'negative', 'ties'))):
        for i, fl in enumerate(flavours):
            case = R.seg_case(name, fl)
            tag = '%s %s %s' % (name, mode, fl)
            got = run_pool_entries(case, mode, window=(i == 0))
            bad = R.seg_check(tag, case, mode, got)
            assert not bad, (tag, bad)
            fun = run_pool_functional(case, mode)
            fun['counts'] = got['counts']
            if mode == 'max':
                fun['argmax'] = got['argmax']
                assert np.array_equal(fun['out'], got['out']) and np.array_equal(fun['dx'], got['dx'])
            bad = R.seg_check(tag + ' functional', case, mode, fun, quiet=True)
            assert not bad, (tag, bad)
    # the sorted, atomic-free mean (B2M_DETERMINISTIC=1): the same bound, and the same bits on every run
    monkeypatch.setenv('B2M_DETERMINISTIC', '1')
    case = R.seg_case(name)
    a, b = run_pool_functional(case, 'avg'), run_pool_functional(case, 'avg')
    assert np.array_equal(a['out'], b['out']) and np.array_equal(a['dx'], b['dx'])
    a['counts'] = R.seg_rule(case['x'], case['ids'], case['n_seg'], 'avg')['counts']
    bad = R.seg_check(name + ' avg deterministic', case, 'avg', a)
    assert not bad, (name, bad)


# ------------------------------------------------------------------ elementwise
@pytest.mark.parametrize('n_elem', [0, 1, 255, 256, 257, 1000003])
def test_relu_and_add_are_exact(n_elem):
    from box2mask_amd import functional as F_
    rng = np.random.default_rng(n_elem)
    a = rng.standard_normal(n_elem).astype(np.float32)
    b = (rng.standard_normal(n_elem) * 1e3).astype(np.float32)
    a[::5] = 0
    ta, tb = dev(a), dev(b)
    pad = 8
    outs = [torch.full((n_elem + 2 * pad,), POISON, device='cuda') for _ in range(3)]
    o = [t[pad:pad + n_elem] for t in outs]
    ptr = lambda t: t.data_ptr() if t.numel() else None
    F_._call('b2m_relu_fwd', ptr(ta), n_elem, ptr(o[0]))
    F_._call('b2m_relu_bwd', ptr(tb), ptr(o[0]), n_elem, ptr(o[1]))
    F_._call('b2m_add', ptr(ta), ptr(tb), n_elem, ptr(o[2]))
    torch.cuda.synchronize()
    y = R.relu_rule(a)
    assert np.array_equal(o[0].cpu().numpy(), y)
    assert np.array_equal(o[1].cpu().numpy(), R.relu_bwd_rule(b, y))
    assert np.array_equal(o[2].cpu().numpy(), R.add_rule(a, b))
    for t in outs:
        assert bool((t[:pad] == POISON).all()) and bool((t[pad + n_elem:] == POISON).all())
    if n_elem:
        x = ta.clone().requires_grad_(True)
        r = F_.relu(x)
        r.backward(tb)
        assert np.array_equal(r.detach().cpu().numpy(), y) and np.array_equal(x.grad.cpu().numpy(), R.relu_bwd_rule(b, y))
