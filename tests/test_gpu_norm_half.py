"""The binary16 BatchNorm kernels of box2mask_amd/csrc/norm.hip (bn_stats_h, bn_apply_h, bn_bwd_reduce_h, bn_bwd_apply_h and their C
entries; half_train._BatchNormH) and the grouped SyncBN operator (functional._BatchNormGroup) against the float64 rule of
tests/_norm_rule.py.

HALF_CASES: the inputs of test_gpu_norm.py (per-column conditioning: |mean| / sigma = 0, 0.5, 30, 100, 1000, a constant column,
sigma = 1e-4 and 1e4) rounded to binary16 -- the rule works on exactly what the device reads -- at the shapes where the kernels change
path: one block and many, idle threads (c = 96), chains of 114 rows (c = 512), pitches wider than the rows, the statistics from
x, from per-tile sums and through the SyncBN entries with the sums doubled on the device.  Each case runs through the C entries
(poisoned surroundings) and through `half_train.batch_norm` -- the sync_h cases through its SyncBN branch, the group a marker and the
exchange a doubling of the packed sums and row count, one per direction --; the two agree bit for bit.  Every backward runs with param_grad_scale = 1
and 2^-10 (one case also 1 / 1000): the fp64 sums and dx do not move, dbeta and dgamma move by exactly the factor.  The ReLU mask the
backward is held to is the device's own: the stored y > 0 where a residual is fused, else the decisions read off the `dres` that
b2m_bn_bwd_apply_h writes when asked (y = NULL: the kernels recompute the sign of the fp32 pre-activation and never look at y).

Exact tables: roundings that have ONE right answer (ties, subnormals, signed zeros, the largest finite value) bit for bit against
numpy's float16 conversion of an fp32 value that is exact by construction.  Refusals and empty inputs.  GROUP_CASES: every member of
a group against the rule on [x; x], bit-identical to the per-layer SyncBN entry sequence, one exchange per direction.

`pytest -s` prints error / bound of every compared quantity.  Worst error / bound measured on an MI355X (all cases of a family):
the six constants 0.25 on every path (stats_h, tiles_h, sync_h, the group) -- half an ulp32: the correctly rounded fp64 value, the
|mean| = 1000 sigma columns included; y 0.999 and dx 0.999 (tiles_h: 1.000 to three places, below 1) on the binary16 paths -- by construction:
the bound is the fp32 bound plus HALF a binary16 spacing, the store's own rounding error reaches half a spacing, and among 1e5 ... 1e6
elements some sit next to a tie (the same arithmetic in fp32 measures 0.32 / 0.45: test_gpu_norm.py) --; dgamma 0.14 (sync_h 0.10,
tiles_h 0.11), dbeta 0.013; with param_grad_scale = 1 / 1000 dgamma 0.006, dbeta 0.003; the group: y 0.23, dx 0.18, dgamma 0.22,
dbeta 0.015; the peer's running statistics of the n = 0 case 0.25; everything exact was exact.

What the rule caught.  With the library of the commit before this file (bn_stats_h_kernel: fp32 chains per thread), the same cases on the
same device gave invstd error / bound 3.8e5 ... 4.1e5 on all nine n = 5000 cases of stats_h / sync_h (the numpy simulation of that launch
geometry in tests/test_norm_rule.py gives the same figures: 3.81e5 for stats_h-n5000-c96-res0-relu0 in both), 1.3e6 at n = 2049, c = 512,
5.2e5 already at n = 255, c = 96, and 2.7e4 ... 4.2e4 at n = 1025, c = 32; scale and shift 1.2e6, running_var 2.6e5, y 1.1e3, dx 8.9e2,
dgamma 145; n = 2, n = 3 and the tile-sum paths passed.  16 of the 22 cases failed; with fp64 accumulators all pass.
"""
import functools

import numpy as np
import pytest
import torch

import _norm_rule as R
from test_gpu_norm import POISON, dev

pytestmark = pytest.mark.gpu

POISON_H = -777.5                          # (a binary16 value)
PGS = (1.0, 2.0 ** -10)
PGS_ODD = float(np.float32(1.0 / 1000))    # not a power of two: one more rounding of dbeta / dgamma
ODD_CASE = 'stats_h-n5000-c96-res1-relu1'
FIRST = {'stats_h': ['b2m_bn_stats_finalize_h'], 'tiles_h': ['b2m_bn_tilestats_finalize'],
         'sync_h': ['b2m_bn_stats_h', 'b2m_bn_finalize'], 'sync_h-tiles': ['b2m_bn_tilestats', 'b2m_bn_finalize']}


@functools.lru_cache(maxsize=2)
def inputs(name):
    return R.half_case_input(name)


def hdev(a):
    a = np.asarray(a, dtype=np.float32)
    assert np.array_equal(a.astype(np.float16).astype(np.float32), a), 'not a binary16 value'
    return torch.from_numpy(np.ascontiguousarray(a.astype(np.float16))).cuda()


def bits(a):
    """binary16 values (torch or numpy) as their 16-bit patterns: -0.0 and +0.0 differ."""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    assert a.dtype == np.float16
    return np.ascontiguousarray(a).view(np.uint16)


class WindowH:
    """test_gpu_norm.Window with binary16 storage: an (n, c) tensor as a column window of a wider, poisoned (n, ld) buffer.  The
    window starts 4 ('c+4') or c ('2c') elements into a row: 8-byte aligned, as the half entries ask."""

    def __init__(self, n, c, ld_kind, data=None):
        ld, off = {None: (c, 0), 'c+4': (c + 4, 4), '2c': (2 * c, c)}[ld_kind]
        self.buf = torch.full((n, ld), POISON_H, dtype=torch.float16, device='cuda')
        self.t = self.buf[:, off:off + c]
        self.cols = (off, off + c)
        if data is not None:
            self.t.copy_(hdev(data))

    def ptr(self):
        return self.t.data_ptr()

    def ld(self):
        return self.buf.shape[1]

    def raw(self):
        keep = torch.ones(self.buf.shape[1], dtype=torch.bool)
        keep[self.cols[0]:self.cols[1]] = False
        assert bool((self.buf[:, keep.cuda()] == POISON_H).all()), 'written outside the window'
        return self.t.cpu().numpy().copy()

    def value(self):
        return self.raw().astype(np.float32)


def f32_vec(c):
    return torch.full((c + 8,), POISON, device='cuda')[4:4 + c]                            # (16-byte aligned inside its buffer)


def run_entries(name, pgs_list):
    """The case through the C entries, as half_train._BatchNormH strings them together; the backward once per param_grad_scale.
    -> [got per scale], fp64 sums per scale."""
    from box2mask_amd import functional as F_
    call = F_._call
    spec, inp = R.HALF_CASES[name], inputs(name)
    n, c, ldk, relu, has_res, path = spec['n'], spec['c'], spec['ld'], spec['relu'], spec['res'], spec['path']
    x, dy = WindowH(n, c, ldk, inp['x']), WindowH(n, c, ldk, inp['dy'])
    res = WindowH(n, c, ldk, inp['res']) if has_res else None
    y = WindowH(n, c, ldk)
    gam, bet, rm, rv = dev(inp['gamma']), dev(inp['beta']), dev(inp['rm0']), dev(inp['rv0'])
    mean, inv, sc, sh = f32_vec(c), f32_vec(c), f32_vec(c), f32_vec(c)
    P = lambda w: w.ptr() if w is not None else None
    L = lambda w: w.ld() if w is not None else 0
    consts = (gam.data_ptr(), bet.data_ptr(), R.EPS, R.MOMENTUM, rm.data_ptr(), rv.data_ptr(), mean.data_ptr(), inv.data_ptr(),
              sc.data_ptr(), sh.data_ptr())
    use_y = relu and has_res                                                               # (else the mask is recomputed from x)
    mask = (None, None) if (use_y or not relu) else (sc.data_ptr(), sh.data_ptr())
    yarg = (y.ptr(), y.ld()) if use_y else (None, 0)
    partial = torch.empty(2 * c * 4096, dtype=torch.float64, device='cuda')
    count_dev = None
    if path == 'stats_h':
        call('b2m_bn_stats_finalize_h', x.ptr(), x.ld(), n, c, partial.data_ptr(), *consts)
    elif path == 'tiles_h':
        ts = dev(R.tile_sums(inp['x']))
        call('b2m_bn_tilestats_finalize', ts.data_ptr(), ts.shape[0], n, c, partial.data_ptr(), None, *consts)
    else:                                       # sync_h: this rank's sums, "all-reduced" with an equal second rank on the device
        stats = torch.empty(2 * c + 1, dtype=torch.float64, device='cuda')
        if spec.get('tiles'):
            ts = dev(R.tile_sums(inp['x']))
            call('b2m_bn_tilestats', ts.data_ptr(), ts.shape[0], c, partial.data_ptr(), stats.data_ptr())
        else:
            call('b2m_bn_stats_h', x.ptr(), x.ld(), n, c, partial.data_ptr(), stats.data_ptr())
        stats[2 * c:].fill_(float(n))
        stats *= 2
        count_dev = stats[2 * c:]
        call('b2m_bn_finalize', stats.data_ptr(), 0.0, count_dev.data_ptr(), c, *consts)
    call('b2m_bn_apply_h', x.ptr(), x.ld(), n, c, sc.data_ptr(), sh.data_ptr(), P(res), L(res), int(relu), y.ptr(), y.ld())
    fwd = {'mean': mean, 'invstd': inv, 'scale': sc, 'shift': sh, 'running_mean': rm, 'running_var': rv}
    fwd = {k: v.cpu().numpy().copy() for k, v in fwd.items()}
    fwd['y'] = y.value()
    gots, all_sums = [], []
    for pgs in pgs_list:
        dx = WindowH(n, c, ldk)
        # dres is asked for whenever there is a ReLU: with y = NULL it is the only witness of the kernel's own mask
        dres = WindowH(n, c, ldk) if (has_res or relu) else None
        dbeta, dgamma = f32_vec(c), f32_vec(c)
        sums = torch.empty(2 * c, dtype=torch.float64, device='cuda')
        call('b2m_bn_bwd_reduce_h', dy.ptr(), dy.ld(), *yarg, x.ptr(), x.ld(), n, c, mean.data_ptr(), inv.data_ptr(), int(relu), *mask,
             partial.data_ptr(), sums.data_ptr(), dbeta.data_ptr(), dgamma.data_ptr(), pgs)
        gsums = sums * 2 if count_dev is not None else sums
        call('b2m_bn_bwd_apply_h', dy.ptr(), dy.ld(), *yarg, x.ptr(), x.ld(), n, c, mean.data_ptr(), inv.data_ptr(), gam.data_ptr(),
             gsums.data_ptr(), float(n), count_dev.data_ptr() if count_dev is not None else None, int(relu), *mask, dx.ptr(), dx.ld(),
             P(dres), L(dres))
        torch.cuda.synchronize()
        got = dict(fwd, dbeta=dbeta.cpu().numpy().copy(), dgamma=dgamma.cpu().numpy().copy(), dx=dx.value())
        if has_res:
            got['dres'] = dres.value()
        elif relu:
            d = dres.value()
            assert np.array_equal(d[d != 0], inp['dy'][d != 0])                            # a masked COPY of dy, which has no zeros
            got['mask'] = d != 0
        gots.append(got)
        all_sums.append(sums.cpu().numpy().copy())
    for w, src in ((x, inp['x']), (dy, inp['dy'])):
        assert np.array_equal(w.value(), src), 'an input was modified'
    return gots, all_sums


def run_functional(name, loss_scale, monkeypatch):
    """The case through half_train.batch_norm.  sync_h: SyncBN's branch with a group that is a marker and an exchange that doubles
    what it is given -- the sums AND the packed row count, as run_entries does: an equal second rank."""
    from box2mask_amd import functional as F_, half_train as HT
    spec, inp = R.HALF_CASES[name], inputs(name)
    c = spec['c']
    monkeypatch.setattr(HT, 'loss_scale', [loss_scale])
    sync = spec['path'] == 'sync_h'
    marker, exchanged = object(), []

    def all_reduce(t, group):
        assert group is marker and t.dtype == torch.float64
        exchanged.append(t.numel())
        t.mul_(2)
    if sync:
        monkeypatch.setattr(F_, '_sync_group', lambda: marker)
        monkeypatch.setattr(F_, '_sync_all_reduce', all_reduce)
    x = hdev(inp['x']).requires_grad_(True)
    res = hdev(inp['res']).requires_grad_(True) if spec['res'] else None
    gam, bet = dev(inp['gamma']).requires_grad_(True), dev(inp['beta']).requires_grad_(True)
    rm, rv = dev(inp['rm0']), dev(inp['rv0'])
    if spec['path'] == 'tiles_h' or spec.get('tiles'):
        ts = dev(R.tile_sums(inp['x'])).reshape(-1, 2, c)
        x._b2m_tile_stats = (ts, ts.shape[0])
    launched = []
    real = HT._call
    monkeypatch.setattr(HT, '_call', lambda nm, *a, **k: (launched.append(nm), real(nm, *a, **k))[1])
    y = HT.batch_norm(x, gam, bet, rm, rv, R.MOMENTUM, R.EPS, res, spec['relu'], sync=sync)
    y.backward(hdev(inp['dy']))
    torch.cuda.synchronize()
    monkeypatch.setattr(HT, '_call', real)
    first = FIRST[spec['path'] + ('-tiles' if sync and spec.get('tiles') else '')]
    assert launched == first + ['b2m_bn_apply_h', 'b2m_bn_bwd_reduce_h', 'b2m_bn_bwd_apply_h'], launched
    # SyncBN: one packed exchange per direction -- (sum x, sum x^2, n), then (sum g, sum g xhat) -- and none without it
    assert exchanged == ([2 * c + 1, 2 * c] if sync else []), exchanged
    got = {'y': y, 'dx': x.grad, 'dgamma': gam.grad, 'dbeta': bet.grad, 'running_mean': rm, 'running_var': rv}
    if res is not None:
        got['dres'] = res.grad
    assert y.dtype == torch.float16 and x.grad.dtype == torch.float16 and gam.grad.dtype == torch.float32
    return {k: v.detach().float().cpu().numpy().copy() for k, v in got.items()}


@pytest.mark.parametrize('name', list(R.HALF_CASES))
def test_half_batch_norm_matches_rule(name, monkeypatch):
    spec, inp = R.HALF_CASES[name], inputs(name)
    assert not np.any(inp['dy'] == 0)
    scales = PGS + ((PGS_ODD,) if name == ODD_CASE else ())
    gots, sums = run_entries(name, scales)
    for pgs, got in zip(scales, gots):
        bad, share = R.bn_check_half('%s pgs=%.3g' % (name, pgs), inp, spec, got, pgs=pgs)
        assert not bad, (name, pgs, bad)
        assert share <= 1e-3
    # the loss scale un-scales dbeta / dgamma and nothing else: the fp64 sums and dx keep their bits, a power of two is exact
    for k in range(1, len(scales)):
        assert np.array_equal(sums[k], sums[0]) and np.array_equal(gots[k]['dx'], gots[0]['dx'])
    for q in ('dbeta', 'dgamma'):
        assert np.array_equal(gots[1][q], gots[0][q] * np.float32(2.0 ** -10)), q
    for pgs, got in zip(scales, gots):
        fun = run_functional(name, 1.0 / pgs if pgs != PGS_ODD else 1000.0, monkeypatch)
        for k, v in fun.items():
            assert np.array_equal(v, got[k]), 'half_train.batch_norm and the C entries differ in %s (pgs %g)' % (k, pgs)


# ------------------------------------------------------------------ exact tables
# column sets (scale, shift, x values): every fmaf(x, scale, shift) below is exact in fp32, so the stored half has one right value
_TABLE = (
    (2.0, 0.0, (32752.0, -32752.0, 1025.0, 0.5, -0.0, -3.0)),                               # results that are binary16 values: +-65504 ...
    (1.0, 1.0, (2048.0, 2050.0, -2050.0, -2052.0, 0.0, -1.0, -3.0, 65472.0)),               # 2049 -> 2048, 2051 -> 2052, -2049 -> -2048, -2051 -> -2052
    (2.0 ** -25, 0.0, (1.0, -1.0, 3.0, 2.0, 1.5, 1024.0, 1023.0, -1023.0)),                 # 2^-25 -> 0, -2^-25 -> -0.0, subnormals
    (1.0, 15.0, (65504.0, 65472.0, -65504.0, 65440.0)),                                     # 65519 -> 65504, 65487 -> 65472, 65455 -> 65440
)


def _table(n, c):
    x = np.empty((n, c), dtype=np.float32)
    scale, shift = np.empty(c, dtype=np.float32), np.empty(c, dtype=np.float32)
    for j in range(c):
        s, b, xs = _TABLE[j % 4]
        scale[j], shift[j] = s, b
        x[:, j] = [xs[(r + j // 4) % len(xs)] for r in range(n)]
    v = x.astype(np.float64) * scale + shift
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v) and np.abs(v).max() < 65520
    return x, scale, shift, v.astype(np.float32)


def test_half_rounding_table_by_hand():
    """The table holds the cases it is named for (numpy's conversion is the yardstick: tests/test_norm_rule.py pins it by hand)."""
    _, _, _, v = _table(8, 4)
    h = v.astype(np.float16)
    pairs = {(float(a), float(b)) for a, b in zip(v.ravel(), h.ravel())}
    for p in ((2049.0, 2048.0), (2051.0, 2052.0), (-2049.0, -2048.0), (65519.0, 65504.0), (65504.0, 65504.0), (65487.0, 65472.0),
              (-65504.0, -65504.0), (-2051.0, -2052.0), (65455.0, 65440.0),
              (2.0 ** -25, 0.0), (3 * 2.0 ** -25, 2.0 ** -23), (1.5 * 2.0 ** -25, 2.0 ** -24), (2.0 ** -15, 2.0 ** -15),
              (1023 * 2.0 ** -25, 2.0 ** -15)):
        assert p in pairs, p
    neg0 = (h == 0) & np.signbit(h)
    assert neg0.sum() >= 1 and np.all(v[neg0] < 0)                                          # -2^-25 -> -0.0 (fmaf(-0.0, 2, +0.0) is +0.0)


@pytest.mark.parametrize('c', [4, 96])
@pytest.mark.parametrize('n', [1, 63, 64, 65])
def test_half_apply_rounds_to_nearest_even_exactly(n, c):
    from box2mask_amd import functional as F_
    x, scale, shift, v = _table(n, c)
    xw = WindowH(n, c, 'c+4', x)
    sc, sh = dev(scale), dev(shift)
    for relu in (0, 1):
        yw = WindowH(n, c, 'c+4')
        F_._call('b2m_bn_apply_h', xw.ptr(), xw.ld(), n, c, sc.data_ptr(), sh.data_ptr(), None, 0, relu, yw.ptr(), yw.ld())
        torch.cuda.synchronize()
        want = (np.where(v > 0, v, np.float32(0.0)) if relu else v).astype(np.float16)      # ReLU of a negative (and of -0.0): +0.0
        got = yw.raw()
        assert np.array_equal(bits(got), bits(want)), (n, c, relu, np.argwhere(bits(got) != bits(want))[:4])
        if relu:
            assert not np.any(np.signbit(got))
        elif n > 1:
            assert np.any(np.signbit(got) & (got == 0))                                     # -0.0 is kept where there is no ReLU


@pytest.mark.parametrize('c', [4, 96])
@pytest.mark.parametrize('n', [1, 63, 64, 65])
def test_half_backward_apply_with_trivial_statistics_is_gamma_times_g_exactly(n, c):
    """sums = 0, mean = 0, invstd = 1 and a power-of-two gamma: dx = gamma * g has one right value (and dres = g)."""
    from box2mask_amd import functional as F_
    rng = np.random.default_rng(n * 1000 + c)
    g = R.to_half((1.0 + 4.0 * rng.random((n, c))) * np.where(rng.random((n, c)) < 0.5, -1.0, 1.0))     # (|g| in [1, 5]: no product leaves the normal range)
    x = R.to_half(rng.standard_normal((n, c)) * 100)
    gamma = np.array([(1.0, 2.0, 0.5, -4.0, -0.125, 8.0)[j % 6] for j in range(c)], dtype=np.float32)
    want = (g * gamma).astype(np.float16)
    assert np.array_equal(want.astype(np.float32), g * gamma)
    gw, xw, dxw, drw = WindowH(n, c, 'c+4', g), WindowH(n, c, None, x), WindowH(n, c, '2c'), WindowH(n, c, 'c+4')
    zero, one = torch.zeros(c, device='cuda'), torch.ones(c, device='cuda')
    sums = torch.zeros(2 * c, dtype=torch.float64, device='cuda')
    F_._call('b2m_bn_bwd_apply_h', gw.ptr(), gw.ld(), None, 0, xw.ptr(), xw.ld(), n, c, zero.data_ptr(), one.data_ptr(),
             dev(gamma).data_ptr(), sums.data_ptr(), float(n), None, 0, None, None, dxw.ptr(), dxw.ld(), drw.ptr(), drw.ld())
    torch.cuda.synchronize()
    assert np.array_equal(bits(dxw.raw()), bits(want))
    assert np.array_equal(bits(drw.raw()), bits(g.astype(np.float16)))


def test_half_apply_above_the_largest_finite_value_today():
    """RECORDS what the BatchNorm half store does above 65504 as of this test, it does not endorse it: the IEEE conversion -- finite
    up to 65519, +-inf from 65520 -- whereas the convolution's half store saturates at +-65504.  ADVICE.md item 1 (static loss scale,
    no overflow handling) is where the two behaviours and a found-inf flag are to be settled; until then neither changes unseen."""
    from box2mask_amd import functional as F_
    c = 4
    x = np.array([[65504.0, -65504.0, 65504.0, -65504.0]], dtype=np.float32)
    sc = dev(np.ones(c, dtype=np.float32))
    sh = dev(np.array([15.0, -15.0, 16.0, -16.0], dtype=np.float32))
    xw, yw = WindowH(1, c, None, x), WindowH(1, c, None)
    F_._call('b2m_bn_apply_h', xw.ptr(), xw.ld(), 1, c, sc.data_ptr(), sh.data_ptr(), None, 0, 0, yw.ptr(), yw.ld())
    torch.cuda.synchronize()
    assert yw.value()[0].tolist() == [65504.0, -65504.0, float('inf'), float('-inf')]


# ------------------------------------------------------------------ refusals and empties
def test_half_entries_refuse_and_leave_empty_inputs_alone():
    from box2mask_amd import functional as F_, half_train as HT
    from box2mask_amd._lib import B2MError
    call = F_._call
    c = 32
    x, dy, y, dx = (WindowH(4, c, None, np.ones((4, c), dtype=np.float32)) for _ in range(4))
    y.buf.fill_(POISON_H), dx.buf.fill_(POISON_H)
    v = lambda: torch.ones(c, device='cuda')
    mean, inv, sc, sh, gam = v(), v(), v(), v(), v()
    partial = torch.zeros(2 * c * 4096, dtype=torch.float64, device='cuda')
    stats = torch.full((2 * c + 1,), float(POISON), dtype=torch.float64, device='cuda')
    sums = torch.zeros(2 * c, dtype=torch.float64, device='cuda')
    # n = 0: the two apply entries return without writing
    call('b2m_bn_apply_h', x.ptr(), x.ld(), 0, c, sc.data_ptr(), sh.data_ptr(), None, 0, 1, y.ptr(), y.ld())
    call('b2m_bn_bwd_apply_h', dy.ptr(), dy.ld(), None, 0, x.ptr(), x.ld(), 0, c, mean.data_ptr(), inv.data_ptr(), gam.data_ptr(),
         sums.data_ptr(), 1.0, None, 0, None, None, dx.ptr(), dx.ld(), None, 0)
    torch.cuda.synchronize()
    assert bool((y.buf == POISON_H).all()) and bool((dx.buf == POISON_H).all())
    # ... the reductions refuse it (a mean of no rows)
    with pytest.raises(B2MError):
        call('b2m_bn_stats_h', x.ptr(), x.ld(), 0, c, partial.data_ptr(), stats.data_ptr())
    with pytest.raises(B2MError):
        call('b2m_bn_stats_finalize_h', x.ptr(), x.ld(), 0, c, partial.data_ptr(), gam.data_ptr(), gam.data_ptr(), R.EPS, R.MOMENTUM,
             None, None, mean.data_ptr(), inv.data_ptr(), sc.data_ptr(), sh.data_ptr())
    with pytest.raises(B2MError):
        call('b2m_bn_bwd_reduce_h', dy.ptr(), dy.ld(), None, 0, x.ptr(), x.ld(), 0, c, mean.data_ptr(), inv.data_ptr(), 0, None, None,
             partial.data_ptr(), sums.data_ptr(), None, None, 1.0)
    # a row that does not start on 8 bytes, a pitch or a width that is no multiple of 4
    with pytest.raises(B2MError):
        call('b2m_bn_stats_h', x.ptr() + 2, x.ld(), 3, c, partial.data_ptr(), stats.data_ptr())
    with pytest.raises(B2MError):
        call('b2m_bn_apply_h', x.ptr(), x.ld(), 3, c, sc.data_ptr(), sh.data_ptr(), None, 0, 1, y.ptr() + 4, y.ld())
    with pytest.raises(B2MError):
        call('b2m_bn_bwd_apply_h', dy.ptr(), dy.ld(), None, 0, x.ptr() + 6, x.ld(), 3, c, mean.data_ptr(), inv.data_ptr(), gam.data_ptr(),
             sums.data_ptr(), 3.0, None, 0, None, None, dx.ptr(), dx.ld(), None, 0)
    with pytest.raises(B2MError):
        call('b2m_bn_apply_h', x.ptr(), x.ld() + 2, 2, c - 4, sc.data_ptr(), sh.data_ptr(), None, 0, 1, y.ptr(), y.ld())
    with pytest.raises(B2MError):
        call('b2m_bn_stats_h', x.ptr(), x.ld(), 3, c - 2, partial.data_ptr(), stats.data_ptr())
    torch.cuda.synchronize()
    assert bool((y.buf == POISON_H).all()) and bool((dx.buf == POISON_H).all()) and bool((stats == POISON).all())
    # one row and no group: torch's own complaint
    with pytest.raises(ValueError):
        HT.batch_norm(torch.ones(1, c, dtype=torch.float16, device='cuda'), gam, gam, mean, inv, R.MOMENTUM, R.EPS)


def test_half_sync_branch_with_no_local_rows(monkeypatch):
    """A rank without rows under SyncBN: it contributes zero sums and a count of 0, the "peer" (the patched exchange) adds the fp64
    sums of ITS rows; the running statistics are then the rule's on the peer's rows, y is empty and the gradients are zero."""
    from box2mask_amd import functional as F_, half_train as HT
    n2, c = 257, 32
    peer = R.half_input(n2, c, 2900)
    px = R.f64(peer['x'])
    exchanged = []

    def all_reduce(t, group):
        assert group is marker
        exchanged.append(t.numel())
        if t.numel() == 2 * c + 1:
            assert bool((t == 0).all())                                                     # this rank: nothing
            t += dev(np.concatenate([px.sum(0), (px * px).sum(0), [float(n2)]]))
    marker = object()
    monkeypatch.setattr(F_, '_sync_group', lambda: marker)
    monkeypatch.setattr(F_, '_sync_all_reduce', all_reduce)
    monkeypatch.setattr(HT, 'loss_scale', [1024.0])
    launched = []
    real = HT._call
    monkeypatch.setattr(HT, '_call', lambda nm, *a, **k: (launched.append(nm), real(nm, *a, **k))[1])
    x = torch.empty(0, c, dtype=torch.float16, device='cuda', requires_grad=True)
    gam, bet = dev(peer['gamma']).requires_grad_(True), dev(peer['beta']).requires_grad_(True)
    rm, rv = dev(peer['rm0']), dev(peer['rv0'])
    y = HT.batch_norm(x, gam, bet, rm, rv, R.MOMENTUM, R.EPS, None, True, sync=True)
    assert tuple(y.shape) == (0, c) and y.dtype == torch.float16
    y.backward(torch.empty(0, c, dtype=torch.float16, device='cuda'))
    torch.cuda.synchronize()
    assert launched == ['b2m_bn_finalize'] and exchanged == [2 * c + 1, 2 * c], (launched, exchanged)
    fwd = R.bn_forward(peer['x'], peer['gamma'], peer['beta'], None, False, (peer['rm0'], peer['rv0']))
    cb = R.const_bounds(peer['x'], peer['gamma'], fwd)
    bad = R.check('sync_h n=0', [(k, v.cpu().numpy(), fwd[k], cb[k]) for k, v in (('running_mean', rm), ('running_var', rv))])
    assert not bad, bad
    assert tuple(x.grad.shape) == (0, c) and not gam.grad.any() and not bet.grad.any()


# ------------------------------------------------------------------ grouped SyncBN
def sync_entries_f32(inp):
    """One fp32 SyncBN layer without ReLU or residual through the per-layer entry sequence (functional._BatchNorm's large-map SyncBN
    branch), the exchange played by doubling on the device."""
    from box2mask_amd import functional as F_
    call = F_._call
    n, c = inp['x'].shape
    x, dy, gam, bet, rm, rv = (dev(inp[k]) for k in ('x', 'dy', 'gamma', 'beta', 'rm0', 'rv0'))
    y, dx = torch.empty_like(x), torch.empty_like(x)
    mean, inv, sc, sh, dbeta, dgamma = (f32_vec(c) for _ in range(6))
    partial = torch.empty(2 * c * 4096, dtype=torch.float64, device='cuda')
    stats = torch.empty(2 * c + 1, dtype=torch.float64, device='cuda')
    sums = torch.empty(2 * c, dtype=torch.float64, device='cuda')
    call('b2m_bn_stats', x.data_ptr(), c, n, c, partial.data_ptr(), stats.data_ptr())
    stats[2 * c:].fill_(float(n))
    stats *= 2
    count_dev = stats[2 * c:]
    call('b2m_bn_finalize', stats.data_ptr(), 0.0, count_dev.data_ptr(), c, gam.data_ptr(), bet.data_ptr(), R.EPS, R.MOMENTUM,
         rm.data_ptr(), rv.data_ptr(), mean.data_ptr(), inv.data_ptr(), sc.data_ptr(), sh.data_ptr())
    call('b2m_bn_apply', x.data_ptr(), c, n, c, sc.data_ptr(), sh.data_ptr(), None, 0, 0, y.data_ptr(), c)
    call('b2m_bn_bwd_reduce', dy.data_ptr(), c, None, 0, x.data_ptr(), c, n, c, mean.data_ptr(), inv.data_ptr(), 0, None, None,
         partial.data_ptr(), sums.data_ptr(), dbeta.data_ptr(), dgamma.data_ptr())
    gsums = sums * 2
    call('b2m_bn_bwd_apply', dy.data_ptr(), c, None, 0, x.data_ptr(), c, n, c, mean.data_ptr(), inv.data_ptr(), gam.data_ptr(),
         gsums.data_ptr(), float(n), count_dev.data_ptr(), 0, None, None, dx.data_ptr(), c, None, 0)
    torch.cuda.synchronize()
    got = {'y': y, 'dx': dx, 'dgamma': dgamma, 'dbeta': dbeta, 'running_mean': rm, 'running_var': rv}
    return {k: v.cpu().numpy().copy() for k, v in got.items()}


@pytest.mark.parametrize('name', list(R.GROUP_CASES))
def test_batch_norm_group_matches_rule_and_the_per_layer_entries(name, monkeypatch):
    from box2mask_amd import functional as F_
    n, cs = R.GROUP_CASES[name]
    inps = R.group_case_inputs(name)
    exchanged = []
    monkeypatch.setattr(F_, '_sync_all_reduce', lambda t, group: (exchanged.append((t.numel(), t.dtype, group)), t.mul_(2))[1])
    members, keep = [], []
    for j, inp in enumerate(inps):
        c = cs[j]
        if j == 1:                                                                          # a column window of a wider tensor
            wide = torch.full((n, c + 8), POISON, device='cuda')
            wide[:, 4:4 + c] = dev(inp['x'])
            x = wide[:, 4:4 + c].detach().requires_grad_(True)
            assert not x.is_contiguous()
        else:
            x = dev(inp['x']).requires_grad_(True)
        gam, bet = dev(inp['gamma']).requires_grad_(True), dev(inp['beta']).requires_grad_(True)
        rm, rv = dev(inp['rm0']), dev(inp['rv0'])
        members.append((x, gam, bet, rm, rv, R.MOMENTUM, R.EPS))
        keep.append((x, gam, bet, rm, rv))
    launched = []
    real = F_._call
    monkeypatch.setattr(F_, '_call', lambda nm, *a, **k: (launched.append(nm), real(nm, *a, **k))[1])
    ys = F_.batch_norm_group(members, None)
    torch.autograd.backward(ys, [dev(inp['dy']) for inp in inps])
    torch.cuda.synchronize()
    monkeypatch.setattr(F_, '_call', real)
    m = len(cs)
    # one exchange per direction: (sum x, sum x^2) of every member + the row count, then (sum g, sum g xhat) of every member
    assert exchanged == [(2 * sum(cs) + 1, torch.float64, None), (2 * sum(cs), torch.float64, None)], exchanged
    assert launched == ['b2m_bn_stats'] * m + ['b2m_bn_finalize', 'b2m_bn_apply'] * m + ['b2m_bn_bwd_reduce'] * m + \
        ['b2m_bn_bwd_apply'] * m, launched
    for j, inp in enumerate(inps):
        x, gam, bet, rm, rv = keep[j]
        got = {'y': ys[j], 'dx': x.grad, 'dgamma': gam.grad, 'dbeta': bet.grad, 'running_mean': rm, 'running_var': rv}
        got = {k: v.detach().cpu().numpy().copy() for k, v in got.items()}
        bad, _ = R.bn_check('%s[%d] c=%d' % (name, j, cs[j]), inp, R.GROUP_SPEC, got)
        assert not bad, (name, j, bad)
        alone = sync_entries_f32(inp)
        for k, v in alone.items():
            assert np.array_equal(v, got[k]), 'member %d of the group and the per-layer entries differ in %s' % (j, k)
