"""The SyncBN operators with ranks that hold DIFFERENT rows -- functional.batch_norm, functional.batch_norm_pair, nn.batch_norm_group
and half_train.batch_norm through their public entries -- against the float64 rule on the concatenation of the ranks' rows
(tests/_norm_rule.py: bn_ranks_check and its pair, group and binary16 forms), under the replay of tests/_syncbn_ranks.py: one process,
no torch.distributed, `_sync_group` a marker and `_sync_all_reduce` the replay's exchange, three passes from fresh inputs.

Every other SyncBN test of the suite plays the second rank as a copy of the first, which cannot tell the mean of the rank means from
the mean, the pooled variance from the variance, or a local count from the global one (tests/test_norm_rule.py holds the table).
Here the ranks differ in their rows, their row counts (one row, none, three ranks) and -- in the straddling cases -- in the kernels
they run: a rank at or below bn_small_rows() takes the small-map half-kernels, its peer the two-stage kernels, and the two meet in
the same packed exchange.  The replay itself asserts that every rank issues the same exchange sequence (else the ranks would wait for
each other for ever), that the contributions are reproduced bit for bit, and that the constants and running statistics have the same
bits on every rank.  profiles/syncbn_ranks_rule.md has the argument, the bounds and the figures measured on an MI355X.

`pytest -s` prints error / bound of every compared quantity.
"""
import functools

import numpy as np
import pytest
import torch

import _norm_rule as R
import _syncbn_ranks as S
from test_gpu_norm import POISON, dev
from test_gpu_norm_half import hdev

pytestmark = pytest.mark.gpu

MARKER = object()
F64 = torch.float64
SMALL = ['b2m_bn_small_fwd_stats', 'b2m_bn_small_fwd_apply', 'b2m_bn_small_bwd_phase', 'b2m_bn_small_bwd_phase']
TWO_STAGE = ['b2m_bn_stats', 'b2m_bn_finalize', 'b2m_bn_apply', 'b2m_bn_bwd_reduce', 'b2m_bn_bwd_apply']
TILES = ['b2m_bn_tilestats'] + TWO_STAGE[1:]
EMPTY = ['b2m_bn_finalize']                       # a rank without rows: the constants from the peers' sums, nothing on its tensors


class Ranks:
    """The patches of one test: the group a marker, the exchange the replay's, the launches of every rank's LAST run recorded."""

    def __init__(self, monkeypatch, rows, modules):
        from box2mask_amd import functional as F_
        self.mp, self.F, self.rows, self.modules = monkeypatch, F_, rows, modules
        self.launched = [[] for _ in rows]
        self.real = [m._call for m in modules]
        monkeypatch.setattr(F_, '_sync_group', lambda: MARKER)

    def begin(self, r, all_reduce):
        F_ = self.F

        def exchange(t, group):
            assert group is MARKER and t.dtype == F64 and t.is_cuda
            if self.rows[r] == 0:
                assert not bool(t.any()), 'a rank without rows contributes zero sums and a count of 0'
            all_reduce(t)
        self.mp.setattr(F_, '_sync_all_reduce', exchange)
        rec = self.launched[r] = []
        for m, real in zip(self.modules, self.real):
            self.mp.setattr(m, '_call', lambda nm, *a, _real=real, **k: (rec.append(nm), _real(nm, *a, **k))[1])

    def end(self):
        torch.cuda.synchronize()
        for m, real in zip(self.modules, self.real):
            self.mp.setattr(m, '_call', real)


def host(d):
    return {k: (v.detach().float().cpu().numpy().copy() if v is not None else None) for k, v in d.items()}


def leaf(a, window=False):
    """A device tensor that records gradients; window: a column window of a wider, poisoned tensor (not contiguous)."""
    t = dev(a)
    if window:
        wide = torch.full((t.shape[0], t.shape[1] + 8), POISON, device='cuda')
        wide[:, 4:4 + t.shape[1]] = t
        t = wide[:, 4:4 + t.shape[1]].detach()
        assert t.shape[0] <= 1 or not t.is_contiguous()
    return t.requires_grad_(True)


@functools.lru_cache(maxsize=2)
def rank_inputs(name):
    return R.rank_case_inputs(name)


# ------------------------------------------------------------------ functional.batch_norm
@pytest.mark.parametrize('name', list(R.RANK_CASES))
def test_batch_norm_with_unequal_ranks_matches_rule(name, monkeypatch):
    from box2mask_amd import functional as F_
    s, inps = R.RANK_CASES[name], rank_inputs(name)
    rows, c = s['rows'], s['c']
    if s['small_rows'] == 2048:
        monkeypatch.delenv('B2M_BN_SMALL_ROWS', raising=False)                                # the default switches
    else:
        monkeypatch.setenv('B2M_BN_SMALL_ROWS', str(s['small_rows']))
    assert F_.bn_small_rows() == s['small_rows']
    ranks = Ranks(monkeypatch, rows, [F_])

    def run_rank(r, all_reduce):
        inp = inps[r]
        x = leaf(inp['x'], window=s.get('window') == r)
        res = leaf(inp['res']) if s['res'] else None
        gam, bet = leaf(inp['gamma']), leaf(inp['beta'])
        rm, rv = dev(inp['rm0']), dev(inp['rv0'])
        if s.get('tiles') == r:
            ts = dev(R.tile_sums(inp['x'])).reshape(-1, 2, c)
            x._b2m_tile_stats = (ts, ts.shape[0])
        ranks.begin(r, all_reduce)
        y = F_.batch_norm(x, gam, bet, rm, rv, True, R.MOMENTUM, R.EPS, res, s['relu'], sync=True)
        saved = y.grad_fn.saved_tensors
        got = {'y': y, 'mean': saved[3].clone(), 'invstd': saved[4].clone()}
        y.backward(dev(inp['dy']))
        ranks.end()
        assert tuple(y.shape) == tuple(x.grad.shape) == (rows[r], c)
        got.update(dx=x.grad, dgamma=gam.grad, dbeta=bet.grad, running_mean=rm, running_var=rv)
        if res is not None:
            got['dres'] = res.grad
        return host(got)
    gots, seq = S.replay(len(rows), run_rank, 3)
    assert seq == [(2 * c + 1, F64), (2 * c, F64)], seq                                       # one packed exchange per direction
    for r, n in enumerate(rows):
        want = EMPTY if n == 0 else SMALL if n <= s['small_rows'] else TILES if s.get('tiles') == r else TWO_STAGE
        assert ranks.launched[r] == want, (name, r, ranks.launched[r])
        if n == 0:
            assert not gots[r]['dgamma'].any() and not gots[r]['dbeta'].any()
    if rows in ((2048, 2049), (256, 257)):                                                    # the two paths met in one exchange
        assert ranks.launched[0] == SMALL and ranks.launched[1] == TWO_STAGE
    bad, share = R.bn_ranks_check(name, inps, s, gots, R.rank_chains(rows, s['small_rows']))
    assert not bad, (name, bad)
    assert share <= 1e-3, (name, share)


# ------------------------------------------------------------------ functional.batch_norm_pair
@pytest.mark.parametrize('name', list(R.PAIR_RANK_CASES))
def test_batch_norm_pair_with_unequal_ranks_matches_rule(name, monkeypatch):
    from box2mask_amd import functional as F_
    rows, c, relu, _ = R.PAIR_RANK_CASES[name]
    a_inps, b_inps = R.pair_rank_case_inputs(name)
    ranks = Ranks(monkeypatch, rows, [F_])

    def run_rank(r, all_reduce):
        side = {}
        for k, inp in (('a', a_inps[r]), ('b', b_inps[r])):
            side[k] = (leaf(inp['x']), leaf(inp['gamma']), leaf(inp['beta']), dev(inp['rm0']), dev(inp['rv0']))
        ranks.begin(r, all_reduce)
        (xa, ga, ba, rma, rva), (xb, gb, bb, rmb, rvb) = side['a'], side['b']
        y = F_.batch_norm_pair(xa, (ga, ba, rma, rva, R.MOMENTUM, R.EPS), xb, (gb, bb, rmb, rvb, R.MOMENTUM, R.EPS), True, relu, sync=True)
        saved = y.grad_fn.saved_tensors
        got = {'y': y, 'mean_a': saved[5].clone(), 'invstd_a': saved[6].clone(), 'mean_b': saved[7].clone(), 'invstd_b': saved[8].clone()}
        y.backward(dev(a_inps[r]['dy']))
        ranks.end()
        assert tuple(y.shape) == (rows[r], c)
        for k, (x, g, b, rm, rv) in side.items():
            assert tuple(x.grad.shape) == (rows[r], c)
            got.update({'dx_' + k: x.grad, 'dgamma_' + k: g.grad, 'dbeta_' + k: b.grad, 'running_mean_' + k: rm, 'running_var_' + k: rv})
        return host(got)
    gots, seq = S.replay(len(rows), run_rank, 3)
    assert seq == [(4 * c + 1, F64), (3 * c, F64)], seq                                       # both layers in one exchange per direction
    for r, n in enumerate(rows):
        want = EMPTY * 2 if n == 0 else ['b2m_bn_stats'] * 2 + ['b2m_bn_finalize'] * 2 + ['b2m_bn_apply2', 'b2m_bn_bwd_reduce2', 'b2m_bn_bwd_apply2']
        assert ranks.launched[r] == want, (name, r, ranks.launched[r])
        if n == 0:
            assert not any(gots[r][k + s].any() for k in ('dgamma_', 'dbeta_') for s in 'ab')
    bad, share = R.pair_ranks_check(name, a_inps, b_inps, relu, gots)
    assert not bad, (name, bad)
    assert share <= 1e-3, (name, share)


# ------------------------------------------------------------------ nn.batch_norm_group (eligibility included)
@pytest.mark.parametrize('name', list(R.GROUP_RANK_CASES))
def test_batch_norm_group_with_unequal_ranks_matches_rule(name, monkeypatch):
    from box2mask_amd import functional as F_, nn as ME
    rows, _ = R.GROUP_RANK_CASES[name]
    cs = R.GROUP_MEMBERS
    members = R.group_rank_case_inputs(name)                                                  # [member][rank]
    monkeypatch.delenv('B2M_BN_GROUP', raising=False)
    ranks = Ranks(monkeypatch, rows, [F_])
    m = len(cs)

    def run_rank(r, all_reduce):
        norms, xs = [], []
        for j, c in enumerate(cs):
            inp = members[j][r]
            nm = ME.MinkowskiBatchNorm(c, eps=R.EPS, momentum=R.MOMENTUM).cuda().train()
            nm.sync = True
            with torch.no_grad():
                nm.bn.weight.copy_(dev(inp['gamma'])); nm.bn.bias.copy_(dev(inp['beta']))
                nm.bn.running_mean.copy_(dev(inp['rm0'])); nm.bn.running_var.copy_(dev(inp['rv0']))
            norms.append(nm)
            xs.append(leaf(inp['x'], window=(j == 1)))
        pooled = ME.PooledTensor(xs[0])
        ranks.begin(r, all_reduce)
        ys = ME.batch_norm_group(norms, [ME.PooledTensor(x, pooled.serial) for x in xs])
        saved = ys[0].F.grad_fn.saved_tensors
        torch.autograd.backward([y.F for y in ys], [dev(members[j][r]['dy']) for j in range(m)])
        ranks.end()
        got = {}
        for j, (nm, x, y) in enumerate(zip(norms, xs, ys)):
            assert tuple(y.F.shape) == tuple(x.grad.shape) == (rows[r], cs[j])
            got.update({'y_%d' % j: y.F, 'dx_%d' % j: x.grad, 'dgamma_%d' % j: nm.bn.weight.grad, 'dbeta_%d' % j: nm.bn.bias.grad,
                        'running_mean_%d' % j: nm.bn.running_mean, 'running_var_%d' % j: nm.bn.running_var,
                        'mean_%d' % j: saved[5 * j + 3], 'invstd_%d' % j: saved[5 * j + 4]})
        return host(got)
    gots, seq = S.replay(len(rows), run_rank, 3)
    # ONE packed exchange per direction on every rank, the one with a single row (or none) included
    assert seq == [(2 * sum(cs) + 1, F64), (2 * sum(cs), F64)], seq
    for r, n in enumerate(rows):
        want = EMPTY * m if n == 0 else ['b2m_bn_stats'] * m + ['b2m_bn_finalize', 'b2m_bn_apply'] * m + ['b2m_bn_bwd_reduce'] * m + \
            ['b2m_bn_bwd_apply'] * m
        assert ranks.launched[r] == want, (name, r, ranks.launched[r])
    per_member = [[{k.rsplit('_', 1)[0]: v for k, v in g.items() if k.endswith('_%d' % j)} for g in gots] for j in range(m)]
    bad = R.group_ranks_check(name, members, per_member)
    assert not bad, (name, bad)
    for r, n in enumerate(rows):
        if n == 0:
            assert not any(per_member[j][r][k].any() for j in range(m) for k in ('dgamma', 'dbeta'))


# ------------------------------------------------------------------ half_train.batch_norm
@pytest.mark.parametrize('name', list(R.HALF_RANK_CASES))
def test_half_batch_norm_with_unequal_ranks_matches_rule(name, monkeypatch):
    from box2mask_amd import functional as F_, half_train as HT
    rows, c, has_res, relu, _ = R.HALF_RANK_CASES[name]
    inps = R.half_rank_case_inputs(name)
    spec = {'res': has_res, 'relu': relu}
    monkeypatch.setattr(HT, 'loss_scale', [1024.0])
    ranks = Ranks(monkeypatch, rows, [HT])

    def run_rank(r, all_reduce):
        inp = inps[r]
        x = hdev(inp['x']).requires_grad_(True)
        res = hdev(inp['res']).requires_grad_(True) if has_res else None
        gam, bet = leaf(inp['gamma']), leaf(inp['beta'])
        rm, rv = dev(inp['rm0']), dev(inp['rv0'])
        ranks.begin(r, all_reduce)
        y = HT.batch_norm(x, gam, bet, rm, rv, R.MOMENTUM, R.EPS, res, relu, sync=True)
        saved = y.grad_fn.saved_tensors
        got = {'y': y, 'mean': saved[4].clone(), 'invstd': saved[5].clone()}
        y.backward(hdev(inp['dy']))
        ranks.end()
        assert y.dtype == x.grad.dtype == torch.float16 and tuple(y.shape) == tuple(x.grad.shape) == (rows[r], c)
        got.update(dx=x.grad, dgamma=gam.grad, dbeta=bet.grad, running_mean=rm, running_var=rv)
        if res is not None:
            got['dres'] = res.grad
        return host(got)
    gots, seq = S.replay(len(rows), run_rank, 3)
    assert seq == [(2 * c + 1, F64), (2 * c, F64)], seq
    for r, n in enumerate(rows):
        want = EMPTY if n == 0 else ['b2m_bn_stats_h', 'b2m_bn_finalize', 'b2m_bn_apply_h', 'b2m_bn_bwd_reduce_h', 'b2m_bn_bwd_apply_h']
        assert ranks.launched[r] == want, (name, r, ranks.launched[r])
    bad, share = R.bn_ranks_check_half(name, inps, spec, gots, pgs=1.0 / 1024.0)
    assert not bad, (name, bad)
    assert share <= 1e-3, (name, share)
