"""The float64 restatement of BatchNorm, segment pooling, ReLU and add (tests/_norm_rule.py) against float64 torch, its tie and
empty-segment conventions against hand-computed cases, and its bounds against (a) an fp32 evaluation of the same formulas in an
order unlike the kernels' -- they must not be too tight -- and (b) deliberate mistakes -- they must not be too loose -- on the very
cases tests/test_gpu_norm.py runs; the same for the binary16 operator and the members of a SyncBN group (tests/test_gpu_norm_half.py),
with the binary16 rounding conventions by hand.  The last sections: the rule for SyncBN ranks that hold different rows against float64
torch on the concatenation, its bounds against an fp32 emulation of the ranks and against seven ways of combining the ranks'
statistics wrongly (with a record of which of them a copied second rank cannot see), the replay harness of tests/_syncbn_ranks.py on
a toy operator, and nn.batch_norm_group's choice between one packed exchange and many.  No GPU.
"""
import functools

import numpy as np
import pytest
import torch

import _norm_rule as R

T = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64).copy())


def close(got, ref, what, rel=1e-9):
    """float64 against float64: 1e-9 of the column's (or tensor's) largest magnitude -- torch forms the variance in another order,
    and a column with |mean| = 1000 sigma loses six of the sixteen digits there."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    top = np.abs(ref).max(0) if ref.ndim == 2 else np.abs(ref)
    assert got.shape == ref.shape, what
    assert np.all(np.abs(got - ref) <= rel * np.maximum(top, 1e-30)), (what, float(np.abs(got - ref).max()))


# ------------------------------------------------------------------ the rule against float64 torch
@pytest.mark.parametrize('res,relu', [(0, 0), (1, 1), (0, 1)])
def test_rule_matches_torch_batchnorm_float64(res, relu):
    inp = R.bn_input(257, 32, seed=1)
    bn = torch.nn.BatchNorm1d(32, eps=R.EPS, momentum=float(np.float32(R.MOMENTUM))).double()
    with torch.no_grad():
        bn.weight.copy_(T(inp['gamma'])); bn.bias.copy_(T(inp['beta']))
        bn.running_mean.copy_(T(inp['rm0'])); bn.running_var.copy_(T(inp['rv0']))
    bn.eps = float(np.float32(R.EPS))
    x, r = T(inp['x']).requires_grad_(True), T(inp['res']).requires_grad_(True)
    pre = bn(x) + (r if res else 0)
    y = torch.relu(pre) if relu else pre
    (y * T(inp['dy'])).sum().backward()
    fwd = R.bn_forward(inp['x'], inp['gamma'], inp['beta'], inp['res'] if res else None, relu, (inp['rm0'], inp['rv0']))
    mask = (fwd['pre'] > 0).astype(np.float64) if relu else None
    assert not relu or np.array_equal(fwd['pre'] > 0, pre.detach().numpy() > 0)          # (no element on the edge)
    bwd = R.bn_backward(inp['x'], inp['gamma'], fwd, inp['dy'], mask)
    close(fwd['y'], y.detach().numpy(), 'y')
    close(fwd['running_mean'], bn.running_mean.numpy(), 'running_mean')
    close(fwd['running_var'], bn.running_var.numpy(), 'running_var')
    close(bwd['dx'], x.grad.numpy(), 'dx')
    close(bwd['dgamma'], bn.weight.grad.numpy(), 'dgamma', rel=1e-9 * 257)       # (relative to the sum of magnitudes, roughly)
    close(bwd['dbeta'], bn.bias.grad.numpy(), 'dbeta', rel=1e-9 * 257)
    if res:
        close(bwd['dres'], r.grad.numpy(), 'dres')


def test_rule_matches_torch_eval_and_pair_float64():
    inp = R.eval_input(9, 32, seed=2)
    bn = torch.nn.BatchNorm1d(32).double().eval()
    bn.eps = float(np.float32(R.EPS))
    with torch.no_grad():
        bn.weight.copy_(T(inp['gamma'])); bn.bias.copy_(T(inp['beta']))
        bn.running_mean.copy_(T(inp['rm0'])); bn.running_var.copy_(T(inp['rv0']))
    x = T(inp['x']).requires_grad_(True)
    y = torch.relu(bn(x))
    (y * T(inp['dy'])).sum().backward()
    fwd = R.bn_eval_forward(inp['x'], inp['gamma'], inp['beta'], inp['rm0'], inp['rv0'], None, True)
    bwd = R.bn_eval_backward(inp['x'], fwd, inp['dy'], (fwd['pre'] > 0).astype(np.float64))
    close(fwd['y'], y.detach().numpy(), 'y')
    close(bwd['dx'], x.grad.numpy(), 'dx')
    close(bwd['dgamma'], bn.weight.grad.numpy(), 'dgamma', rel=1e-8)
    close(bwd['dbeta'], bn.bias.grad.numpy(), 'dbeta', rel=1e-8)
    assert np.array_equal(T(inp['rm0']).numpy(), bn.running_mean.numpy())                # eval mode leaves them alone
    # the pair: relu(BN_a(xa) + BN_b(xb)) is the rule of one BatchNorm with the other's output as its residual
    a, b = R.pair_case_input('pair-n300-c64')
    fb = R.bn_forward(b['x'], b['gamma'], b['beta'])
    fa = R.bn_forward(a['x'], a['gamma'], a['beta'], fb['y'], True)
    bna, bnb = torch.nn.BatchNorm1d(64).double(), torch.nn.BatchNorm1d(64).double()
    for m, s in ((bna, a), (bnb, b)):
        m.eps = float(np.float32(R.EPS))
        with torch.no_grad():
            m.weight.copy_(T(s['gamma'])); m.bias.copy_(T(s['beta']))
    xa, xb = T(a['x']).requires_grad_(True), T(b['x']).requires_grad_(True)
    y = torch.relu(bna(xa) + bnb(xb))
    (y * T(a['dy'])).sum().backward()
    close(fa['y'], y.detach().numpy(), 'pair y')
    mask = (fa['pre'] > 0).astype(np.float64)
    close(R.bn_backward(a['x'], a['gamma'], fa, a['dy'], mask)['dx'], xa.grad.numpy(), 'pair dx_a')
    close(R.bn_backward(b['x'], b['gamma'], fb, a['dy'], mask)['dx'], xb.grad.numpy(), 'pair dx_b')


@pytest.mark.parametrize('mode', ['avg', 'max'])
def test_rule_matches_scatter_reduce_float64_without_ties(mode):
    case = R.seg_case('seg-n7000-c13-random-s211')
    assert int(np.bincount(case['ids'], minlength=211).min()) > 0
    x = T(case['x']).requires_grad_(True)
    idx = torch.from_numpy(case['ids']).reshape(-1, 1).expand(-1, 13)
    out = torch.zeros(211, 13, dtype=torch.float64).scatter_reduce(0, idx, x, 'mean' if mode == 'avg' else 'amax', include_self=False)
    (out * T(case['dout'])).sum().backward()
    ref = R.seg_rule(case['x'], case['ids'], 211, mode, case['dout'])
    close(ref['out'], out.detach().numpy(), 'out', rel=1e-13)
    close(ref['dx'], x.grad.numpy(), 'dx', rel=1e-13)


# ------------------------------------------------------------------ the conventions, by hand
def test_conventions_by_hand():
    x = np.array([[1.0, -2.0], [3.0, -2.0], [3.0, -5.0], [0.0, 0.0], [0.0, -1.0]], dtype=np.float32)
    ids = np.array([2, 2, 2, 0, 0])
    dout = np.array([[10.0, 20.0], [30.0, 40.0], [50.0, 60.0], [70.0, 80.0]], dtype=np.float32)
    mx = R.seg_rule(x, ids, 4, 'max', dout)
    # segment 2: column 0 has its maximum 3 in rows 1 and 2 -> row 1; column 1 has -2 in rows 0 and 1 -> row 0 (all negative)
    assert mx['out'].tolist() == [[0.0, 0.0], [0.0, 0.0], [3.0, -2.0], [0.0, 0.0]]
    assert mx['argmax'].tolist() == [[3, 3], [-1, -1], [1, 0], [-1, -1]]                  # empty segments 1 and 3: 0 and -1
    assert mx['dx'].tolist() == [[0.0, 60.0], [50.0, 0.0], [0.0, 0.0], [10.0, 20.0], [0.0, 0.0]]
    assert mx['counts'].tolist() == [2, 0, 3, 0]
    av = R.seg_rule(x, ids, 4, 'avg', dout)
    assert av['out'].tolist() == [[0.0, -0.5], [0.0, 0.0], [7.0 / 3.0, -3.0], [0.0, 0.0]]
    assert av['dx'][0].tolist() == [50.0 / 3.0, 20.0] and av['dx'][3].tolist() == [5.0, 10.0]
    # a whole segment of post-ReLU zeros: the value 0 is a real maximum, its gradient goes to the first row
    z = R.seg_rule(np.zeros((3, 1), dtype=np.float32), np.array([1, 1, 1]), 2, 'max', np.array([[5.0], [7.0]], dtype=np.float32))
    assert z['out'].tolist() == [[0.0], [0.0]] and z['argmax'].tolist() == [[-1], [0]] and z['dx'].tolist() == [[7.0], [0.0], [0.0]]
    # no rows at all
    e = R.seg_rule(np.zeros((0, 2), dtype=np.float32), np.zeros(0, dtype=np.int64), 3, 'max', np.ones((3, 2), dtype=np.float32))
    assert e['out'].tolist() == [[0.0, 0.0]] * 3 and e['dx'].shape == (0, 2) and e['counts'].tolist() == [0, 0, 0]
    # BatchNorm of two rows: mean 2, biased variance 1, the running variance takes the unbiased 2
    f = R.bn_forward(np.array([[1.0], [3.0]]), [2.0], [0.5], None, True, ([0.0], [1.0]), eps=0.0, momentum=0.5)
    assert f['mean'][0] == 2.0 and f['var'][0] == 1.0 and f['y'].tolist() == [[0.0], [2.5]]
    assert f['running_mean'][0] == 1.0 and f['running_var'][0] == 1.5
    b = R.bn_backward(np.array([[1.0], [3.0]]), [2.0], f, np.array([[1.0], [1.0]]), (f['pre'] > 0).astype(np.float64))
    assert b['dbeta'][0] == 1.0 and b['dgamma'][0] == 1.0 and b['dres'].tolist() == [[0.0], [1.0]]
    assert np.array_equal(R.relu_rule([-1.0, 0.0, 2.0]), np.float32([0, 0, 2]))
    assert np.array_equal(R.relu_bwd_rule([5.0, 6.0, 7.0], [0.0, 1.0, 0.0]), np.float32([0, 6, 0]))
    assert np.array_equal(R.add_rule([1.0, 2.0 ** -24], [2.0 ** -24, 1.0]), np.float32([1, 1]))


# ------------------------------------------------------------------ the bounds are not too tight
@functools.lru_cache(maxsize=4)
def _inp(name):
    return R.bn_case_input(name)


@pytest.mark.parametrize('name', sorted(R.BN_CASES))
def test_fp32_evaluation_in_another_order_passes_and_few_elements_are_borderline(name):
    spec, inp = R.BN_CASES[name], _inp(name)
    n, c = inp['x'].shape
    assert (n, c) == (spec['n'], spec['c'])
    kinds = {R.kind_of(j) for j in range(c)}
    assert kinds == set(R.KINDS[:min(c, 8)])                                              # every case mixes the conditionings
    if not spec.get('eval') and n >= 255:                                                 # ... and the columns are what they claim
        m, v = R.bn_stats(inp['x'])
        for j in range(min(c, 8)):
            k, sd = R.kind_of(j), np.sqrt(v[j])
            if k in ('ratio30', 'ratio100', 'ratio1000'):
                assert 0.8 * float(k[5:]) < abs(m[j]) / sd < 1.25 * float(k[5:]), (k, m[j], sd)
            elif k in ('ratio0', 'ratio0.5'):                                             # (a sample of n rows: +- 1 / sqrt(n))
                assert abs(abs(m[j]) / sd - float(k[5:])) < 0.25, (k, m[j], sd)
            elif k == 'const':
                assert v[j] == 0.0
            elif k == 'sigma1e-4':
                assert v[j] < R.EPS * 1e-2
            elif k == 'sigma1e4':
                assert v[j] > 0.5e8
    got = R.bn_emulate(inp, spec)
    bad, share = R.bn_check(name, inp, spec, got)
    assert not bad, (name, bad)
    assert share <= 1e-3, (name, share)


@pytest.mark.parametrize('name', sorted(R.PAIR_CASES))
def test_pair_fp32_evaluation_passes(name):
    a, b = R.pair_case_input(name)
    relu = R.PAIR_CASES[name][2]
    bad, share = R.pair_check(name, a, b, relu, R.pair_emulate(a, b, relu))
    assert not bad, (name, bad)
    assert share <= 1e-3, (name, share)


FLAVOURS = {'avg': ('plain',), 'max': ('plain', 'negative', 'ties')}


@pytest.mark.parametrize('name', sorted(R.SEG_CASES))
def test_segment_fp32_evaluation_passes(name):
    for mode, flavours in FLAVOURS.items():
        for fl in flavours:
            case = R.seg_case(name, fl)
            assert case['x'].shape == (case['n'], case['c']) and (case['n'] == 0 or int(case['ids'].max()) < case['n_seg'])
            assert not np.any(np.signbit(case['x']) & (case['x'] == 0)) and np.all(np.isfinite(case['x']))
            bad = R.seg_check('%s %s %s' % (name, mode, fl), case, mode, R.seg_emulate(case, mode), quiet=True)
            assert not bad, (name, mode, fl, bad)


def test_segment_cases_hold_their_edges():
    ties = R.seg_case('seg-n7000-c96-runs-s120', 'ties')
    ref = R.seg_rule(ties['x'], ties['ids'], 120, 'max')
    hit = (ties['x'] == ref['out'][ties['ids']]).astype(np.int64)
    per = np.zeros((120, 96), dtype=np.int64)
    np.add.at(per, ties['ids'], hit)
    assert int((per > 1).sum()) > 1000                                                    # equal maxima, many of them
    zero_seg = [s for s in np.unique(ties['ids']) if not ties['x'][ties['ids'] == s].any()]
    assert len(zero_seg) >= 3 and all(bool((ref['argmax'][s] == np.nonzero(ties['ids'] == s)[0][0]).all()) for s in zero_seg)
    neg = R.seg_case('seg-n7000-c96-runs-s120', 'negative')
    assert float(neg['x'].max()) < 0 and float(R.seg_rule(neg['x'], neg['ids'], 120, 'max')['out'].min()) < 0
    runs = R.seg_case('seg-n7000-c96-runs-s120')
    change = np.nonzero(np.diff(runs['ids']))[0] + 1
    assert len(change) > 20 and np.any(change % 64 != 0) and int(np.diff(change).max()) > 64  # runs cross the 64-row blocks
    assert int((np.bincount(runs['ids'], minlength=120) == 0).sum()) > 0                  # and leave segments empty
    gaps = R.seg_case('seg-n7000-c3-gaps-s50')
    assert int((np.bincount(gaps['ids'], minlength=50) == 0).sum()) >= 30
    many = R.seg_case('seg-n63-c96-random-s200')
    assert many['n_seg'] > many['n']
    assert R.seg_case('seg-n0-c96-random-s5')['x'].shape == (0, 96) and R.seg_case('seg-n0-c13-random-s0')['n_seg'] == 0


# ------------------------------------------------------------------ the bounds are not too loose
LOOSE_ON = ('small-n257-c96-res1-relu1', 'stats-n257-c96-res1-relu1-ldc+4', 'stats-n2-c4-res1-relu1', 'small-n2-c4-res1-relu1',
            'stats-n5000-c256-res1-relu1', 'sync-n257-c32-res0-relu1')


@pytest.mark.parametrize('mistake', [m for m in R.MISTAKES if m != 'fp32_chains'])
def test_a_deliberate_mistake_fails(mistake):
    failed = []
    for name in LOOSE_ON:
        assert name in R.BN_CASES, name
        bad, _ = R.bn_check(name, _inp(name), R.BN_CASES[name], R.bn_emulate(_inp(name), R.BN_CASES[name], mistake), quiet=True)
        if bad:
            failed.append((name, bad))
    print(mistake, failed)
    assert failed, 'the bounds let the mistake %s pass on every case' % mistake


@pytest.mark.parametrize('name', ['stats-n20000-c96-res1-relu1', 'stats-n5000-c256-res1-relu1'])
def test_fp32_accumulation_of_the_statistics_fails_the_constants(name):
    """What bn_stats_kernel did before it accumulated in fp64: fp32 chains (here of 25 rows) of sum x and sum x^2.  invstd must
    miss its bound on the columns with |mean| = 30, 100 and 1000 sigma -- and pass where the mean is small."""
    spec, inp = R.BN_CASES[name], _inp(name)
    got = R.bn_emulate(inp, spec, 'fp32_chains')
    fwd = R.bn_forward(inp['x'], inp['gamma'], inp['beta'], None, False, (inp['rm0'], inp['rv0']))
    cb = R.const_bounds(inp['x'], inp['gamma'], fwd)
    r = np.abs(got['invstd'].astype(np.float64) - fwd['invstd']) / cb['invstd']
    kinds = np.array([R.kind_of(j) for j in range(spec['c'])])
    for k in ('ratio30', 'ratio100', 'ratio1000'):
        print(name, k, 'invstd error / bound: max %.1f, columns over %d of %d' % (r[kinds == k].max(), (r[kinds == k] > 1).sum(),
                                                                                 (kinds == k).sum()))
        assert r[kinds == k].max() > 1.0, (k, r[kinds == k])
    assert r[kinds == 'ratio1000'].min() > 10.0
    assert r[(kinds == 'ratio0') | (kinds == 'ratio0.5')].max() <= 1.0


@pytest.mark.parametrize('mistake', R.SEG_MISTAKES)
def test_a_deliberate_pooling_mistake_fails(mistake):
    failed = []
    for name in ('seg-n65-c96-runs-s4', 'seg-n65-c1-gaps-s12', 'seg-n7000-c96-runs-s120'):
        for mode, fl in (('avg', 'plain'), ('max', 'ties')):
            case = R.seg_case(name, fl)
            if R.seg_check(name, case, mode, R.seg_emulate(case, mode, mistake), quiet=True):
                failed.append((name, mode))
    assert failed, mistake
    if mistake == 'highest_tie':
        assert all(m == 'max' for _, m in failed)


def test_oracle_max_pool_follows_the_rule_on_ties():
    """oracle/sparse_ref.segment_pool('max') gives the gradient to the lowest tied row, like the kernel and the rule."""
    from oracle import sparse_ref as S
    for name, fl in (('seg-n7000-c96-runs-s120', 'ties'), ('seg-n65-c1-gaps-s12', 'ties'), ('seg-n63-c96-random-s200', 'negative'),
                     ('seg-n0-c96-random-s5', 'plain')):
        c = R.seg_case(name, fl)
        x = torch.from_numpy(c['x']).requires_grad_(True)
        o = S.segment_pool(x, torch.from_numpy(c['ids']), c['n_seg'], 'max')
        (o * torch.from_numpy(c['dout'])).sum().backward()
        ref = R.seg_rule(c['x'], c['ids'], c['n_seg'], 'max', c['dout'])
        assert np.array_equal(o.detach().numpy(), ref['out']) and np.array_equal(x.grad.numpy(), ref['dx']), (name, fl)


# ------------------------------------------------------------------ binary16 BatchNorm: conventions, bounds, mistakes
def test_half_rounding_conventions_by_hand():
    h = lambda v: float(R.to_half(np.float32(v)))
    # ties go to the even neighbour: the spacing is 2 in [2048, 4096)
    assert h(2049.0) == 2048.0 and h(2051.0) == 2052.0 and h(2050.0) == 2050.0
    # subnormals are 2^-24 apart; half of the smallest one is a tie and goes to (even) zero, anything above it rounds up
    assert h(2.0 ** -24) == 2.0 ** -24 and h(2.0 ** -25) == 0.0 and h(1.5 * 2.0 ** -25) == 2.0 ** -24
    assert h(3 * 2.0 ** -25) == 2.0 ** -23                                                  # 1.5 subnormal steps: tie to even (2)
    assert h(2.0 ** -14 - 2.0 ** -25) == 2.0 ** -14                                         # the largest subnormal + half a step: tie to even
    # the largest finite value; the rule clips before it converts
    assert h(65504.0) == 65504.0 and h(65519.0) == 65504.0 and h(1e9) == 65504.0 and h(-1e9) == -65504.0
    with np.errstate(over='ignore'):                                                         # IEEE: finite below 65520, infinite from there
        assert np.float32(65519.0).astype(np.float16) == np.float16(65504.0) and np.isinf(np.float32(65520.0).astype(np.float16))
    # the spacing table of the bound
    assert R.half_spacing(0.0) == 2.0 ** -24 and R.half_spacing(2.0 ** -14) == 2.0 ** -24 and R.half_spacing(2.0 ** -13) == 2.0 ** -23
    assert R.half_spacing(1.0) == 2.0 ** -10 and R.half_spacing(1.999) == 2.0 ** -10 and R.half_spacing(2048.0) == 2.0
    assert R.half_spacing(65504.0) == 32.0 and R.half_spacing(1e6) == 32.0
    for v in (1e-7, 3e-5, 0.3, 1000.3, 40000.0):                                            # ... is numpy's
        assert R.half_spacing(v) == float(np.spacing(np.float16(v)))
    # one store: 2049 known to +-0.25 may store as 2048 or 2050 -- a distance of at most 0.25 + 1 from the rule's value
    assert float(R.half_store(2049.0, 0.25)) == 1.25
    # truncation and the emulation's rounding
    assert R._round_half(np.float32([2049.0, 2051.0, -2051.0]), True).tolist() == [2048.0, 2050.0, -2050.0]
    assert R._round_half(np.float32([2049.0, 2051.0, -2051.0])).tolist() == [2048.0, 2052.0, -2052.0]
    # the launch geometry's chain lengths
    assert R.chain_len(5000, 96) == 25 and R.chain_len(5000, 256) == 63 and R.chain_len(2049, 512) == 114
    assert R.chain_len(256, 1024) == 256 and R.chain_len(327680, 256) == 64 and R.chain_len(2, 4) == 1
    assert R.is_pow2(1.0 / 1024) and R.is_pow2(1.0) and not R.is_pow2(np.float32(1.0 / 1000))


@functools.lru_cache(maxsize=4)
def _hinp(name):
    return R.half_case_input(name)


@pytest.mark.parametrize('name', list(R.HALF_CASES))
def test_half_emulation_passes_and_few_elements_are_borderline(name):
    spec, inp = R.HALF_CASES[name], _hinp(name)
    n, c = inp['x'].shape
    assert (n, c) == (spec['n'], spec['c']) and not np.any(inp['dy'] == 0)
    assert np.abs(inp['x']).max() < R.H_MAX
    if n >= 255:                                                                            # the columns are still what they claim
        m, v = R.bn_stats(inp['x'])
        for j in range(min(c, 8)):
            k, sd = R.kind_of(j), np.sqrt(v[j])
            if k in ('ratio30', 'ratio100', 'ratio1000'):
                assert 0.8 * float(k[5:]) < abs(m[j]) / sd < 1.25 * float(k[5:]), (k, m[j], sd)
            elif k == 'const':
                assert v[j] == 0.0
    for pgs in (1.0, 1.0 / 1024, 1.0 / 1000):
        got = R.bn_emulate_h(inp, spec, pgs=pgs)
        bad, share = R.bn_check_half(name, inp, spec, got, pgs=pgs, quiet=pgs != 1.0)
        assert not bad, (name, pgs, bad)
        assert share <= 1e-3, (name, share)


HALF_LOOSE_ON = ('stats_h-n257-c96-res1-relu1-ldc+4', 'stats_h-n2-c4-res1-relu1', 'stats_h-n5000-c256-res1-relu1',
                 'stats_h-n5000-c96-res0-relu1', 'sync_h-n257-c32-res0-relu1')


@pytest.mark.parametrize('mistake', [m for m in R.HALF_MISTAKES if m != 'fp32_chains_h'])
def test_a_deliberate_half_mistake_fails(mistake):
    failed = []
    for name in HALF_LOOSE_ON:
        spec, inp = R.HALF_CASES[name], _hinp(name)
        bad, _ = R.bn_check_half(name, inp, spec, R.bn_emulate_h(inp, spec, mistake, pgs=1.0 / 1024), pgs=1.0 / 1024, quiet=True)
        if bad:
            failed.append((name, [b.split(':')[0] for b in bad]))
    print(mistake, failed)
    assert failed, 'the bounds let the mistake %s pass on every case' % mistake
    named = {q for _, qs in failed for q in qs}
    want = {'truncate_half': {'y', 'dx'}, 'no_unscale': {'dbeta', 'dgamma'}, 'mask_ge': {'dres'}, 'drop_row': {'mean'}}[mistake]
    assert want <= named, (mistake, named)


@pytest.mark.parametrize('name', [k for k, s in R.HALF_CASES.items() if s['path'] in ('stats_h', 'sync_h') and s['n'] >= 5000
                                  and not s.get('tiles')])
def test_fp32_chains_of_the_half_statistics_fail_the_constants(name):
    """bn_stats_h_kernel as it was (fp32 chains per thread in the launch geometry, fp64 from the block combine on), SIMULATED in
    numpy: invstd or scale must miss its bound on every such case with n >= 5000 -- on the |mean| >= 30 sigma columns."""
    spec, inp = R.HALF_CASES[name], _hinp(name)
    got = R.bn_emulate_h(inp, spec, 'fp32_chains_h')
    fwd = R.bn_forward(inp['x'], inp['gamma'], inp['beta'], None, False, (inp['rm0'], inp['rv0']), count_factor=spec.get('count_factor', 1))
    cb = R.const_bounds(inp['x'], inp['gamma'], fwd, count_factor=spec.get('count_factor', 1))
    kinds = np.array([R.kind_of(j) for j in range(spec['c'])])
    over = {}
    for q in ('invstd', 'scale'):
        r = np.abs(got[q].astype(np.float64) - fwd[q]) / cb[q]
        over[q] = float(r.max())
        for k in ('ratio30', 'ratio100', 'ratio1000', 'ratio0.5'):
            print(name, q, k, 'error / bound: max %.3g' % r[kinds == k].max())
        assert r[(kinds == 'ratio0') | (kinds == 'ratio0.5')].max() <= 1.0
    assert over['invstd'] > 1.0 or over['scale'] > 1.0, over
    bad, _ = R.bn_check_half(name, inp, spec, got, quiet=True)
    assert any(b.startswith(('invstd', 'scale')) for b in bad), bad


@pytest.mark.parametrize('name', list(R.GROUP_CASES))
def test_group_members_are_the_syncbn_rule(name):
    n, cs = R.GROUP_CASES[name]
    for j, inp in enumerate(R.group_case_inputs(name)):
        assert inp['x'].shape == (n, cs[j])
        bad, _ = R.bn_check('%s[%d]' % (name, j), inp, R.GROUP_SPEC, R.bn_emulate(inp, R.GROUP_SPEC), quiet=True)
        assert not bad, (name, j, bad)
        bad, _ = R.bn_check('%s[%d]' % (name, j), inp, R.GROUP_SPEC, R.bn_emulate(inp, R.GROUP_SPEC, 'no_bessel'), quiet=True)
        assert bad and all(b.startswith('running_var') for b in bad), (name, j, bad)        # 2n rows in the unbiased factor


# ================================================================== SyncBN over ranks that hold different rows
@pytest.mark.parametrize('res,relu', [(0, 0), (1, 1), (0, 1)])
def test_rank_rule_matches_torch_batchnorm_float64_on_the_concatenation(res, relu):
    """The rule of the unequal ranks against float64 torch with autograd on X = [x_0; x_1; x_2]: y and dx by slices, the ranks'
    parameter gradients by their sum."""
    rows, c = (65, 1, 300), 32
    inps = R.bn_input_ranks(rows, c, seed=11)
    p = inps[0]
    spec = {'res': bool(res), 'relu': bool(relu)}
    assert [i['x'].shape for i in inps] == [(n, c) for n in rows]
    means = np.array([i['x'].astype(np.float64).mean(0) for i in inps])
    _, var = R.bn_stats(np.concatenate([i['x'] for i in inps]))
    within = np.array([R.bn_stats(inps[r]['x'])[1] for r in (0, 2)]).max(0)
    assert int((var > 5 * within + 1e-12).sum()) >= c // 8 and np.ptp(means, axis=0).max() > 0      # the spread between ranks dominates some columns
    bn = torch.nn.BatchNorm1d(c, eps=R.EPS, momentum=float(np.float32(R.MOMENTUM))).double()
    bn.eps = float(np.float32(R.EPS))
    with torch.no_grad():
        bn.weight.copy_(T(p['gamma'])); bn.bias.copy_(T(p['beta']))
        bn.running_mean.copy_(T(p['rm0'])); bn.running_var.copy_(T(p['rv0']))
    cat = lambda k: np.concatenate([i[k] for i in inps])
    x, r = T(cat('x')).requires_grad_(True), T(cat('res')).requires_grad_(True)
    pre = bn(x) + (r if res else 0)
    y = torch.relu(pre) if relu else pre
    (y * T(cat('dy'))).sum().backward()
    rule = R.bn_ranks_rule(inps, spec)
    lo = np.concatenate([[0], np.cumsum(rows)])
    n_all = sum(rows)
    for k, n in enumerate(rows):
        sl = slice(lo[k], lo[k + 1])
        close(rule[k]['y'], y.detach().numpy()[sl], 'y')
        # (dx relative to the tensor's column maxima, not the slice's: a one-row slice may hold a cancelled value)
        assert np.all(np.abs(rule[k]['dx'] - x.grad.numpy()[sl]) <= 1e-9 * np.abs(x.grad.numpy()).max(0)), k
        close(rule[k]['running_mean'], bn.running_mean.numpy(), 'running_mean')
        close(rule[k]['running_var'], bn.running_var.numpy(), 'running_var')
        if res:
            close(rule[k]['dres'], r.grad.numpy()[sl], 'dres')
    close(sum(d['dgamma'] for d in rule), bn.weight.grad.numpy(), 'sum of dgamma_r', rel=1e-9 * n_all)
    close(sum(d['dbeta'] for d in rule), bn.bias.grad.numpy(), 'sum of dbeta_r', rel=1e-9 * n_all)
    # the check holds what the rule says: the rule's own values pass it with error 0
    bad, _ = R.bn_ranks_check('rule', inps, spec, rule, [64, 64, 64], quiet=True)
    assert not bad, bad


def _rank_emulation(name):
    if name in R.RANK_CASES:
        s = R.RANK_CASES[name]
        inps = R.rank_case_inputs(name)
        return R.bn_ranks_check(name, inps, s, R.bn_ranks_emulate(inps, s), R.rank_chains(s['rows'], s['small_rows']))
    if name in R.HALF_RANK_CASES:
        rows, c, res, relu, _ = R.HALF_RANK_CASES[name]
        inps, spec = R.half_rank_case_inputs(name), {'res': res, 'relu': relu}
        pgs = 2.0 ** -10
        return R.bn_ranks_check_half(name, inps, spec, R.bn_ranks_emulate(inps, spec, half=True, pgs=pgs), pgs=pgs)
    if name in R.PAIR_RANK_CASES:
        a, b = R.pair_rank_case_inputs(name)
        relu = R.PAIR_RANK_CASES[name][2]
        return R.pair_ranks_check(name, a, b, relu, R.pair_ranks_emulate(a, b, relu))
    members = R.group_rank_case_inputs(name)
    plain = {'res': False, 'relu': False}
    return R.group_ranks_check(name, members, [R.bn_ranks_emulate(inps, plain) for inps in members]), 0.0


@pytest.mark.parametrize('name', list(R.RANK_CASES) + list(R.HALF_RANK_CASES) + list(R.PAIR_RANK_CASES) + list(R.GROUP_RANK_CASES))
def test_rank_fp32_emulation_passes_and_few_elements_are_borderline(name):
    bad, share = _rank_emulation(name)
    assert not bad, (name, bad)
    assert share <= 1e-3, (name, share)


def test_rank_cases_hold_their_edges():
    rows = {s['rows'] for s in R.RANK_CASES.values()}
    assert {(300, 300), (1, 300), (2048, 2049), (256, 257), (0, 257), (1, 1), (65, 1, 4033)} <= rows
    assert {s['c'] for s in R.RANK_CASES.values()} == {4, 32, 96, 256} and 512 in {v[1] for v in R.HALF_RANK_CASES.values()}
    assert {(s['res'], s['relu']) for s in R.RANK_CASES.values()} == {(False, False), (True, True), (False, True)}
    for name, s in R.RANK_CASES.items():
        chains = R.rank_chains(s['rows'], s['small_rows'])
        if s['rows'] in ((2048, 2049), (256, 257)):
            assert chains == [1, 64], name                                                  # the two paths meet in one exchange
    assert any(s.get('tiles') is not None for s in R.RANK_CASES.values())


# mistake -> the unequal case that has to catch it
RANK_MISTAKE_CASE = {'mean_of_rank_means': 'ranks-1+300-c96-res0-relu1', 'pooled_within_variance': 'ranks-300+300-c32-res1-relu1',
                     'local_count_in_dx': 'ranks-1+300-c96-res0-relu1', 'local_sums_in_dx': 'ranks-300+300-c32-res1-relu1',
                     'unbiased_with_local_n': 'ranks-1+300-c96-res0-relu1', 'count_is_world_times_local': 'ranks-1+300-c96-res0-relu1',
                     'param_grads_from_global_sums': 'ranks-300+300-c32-res1-relu1'}
# ... and whether the form every SyncBN test used before (the second rank a copy of the first: count_factor = 2) sees it
BLIND_WITH_A_COPIED_RANK = {'mean_of_rank_means', 'pooled_within_variance', 'local_sums_in_dx', 'count_is_world_times_local'}


def _copied_rank_form(mistake):
    """The mistake on two ranks that hold the SAME rows, rank 0 held to the rule on [x; x] as the one-process SyncBN tests do."""
    spec = dict(R.BN_CASES['sync-n257-c32-res0-relu1'])
    inp = R.bn_case_input('sync-n257-c32-res0-relu1')
    got = R.bn_ranks_emulate([inp, inp], spec, mistake)[0]
    bad, _ = R.bn_check('copied rank, ' + str(mistake), inp, spec, got, quiet=True)
    return bad


@pytest.mark.parametrize('mistake', R.RANK_MISTAKES)
def test_a_deliberate_rank_mistake_fails_its_unequal_case(mistake):
    name = RANK_MISTAKE_CASE[mistake]
    s, inps = R.RANK_CASES[name], R.rank_case_inputs(name)
    assert len(set(s['rows'])) > 1 or not np.array_equal(inps[0]['x'], inps[1]['x'])
    bad, _ = R.bn_ranks_check(name, inps, s, R.bn_ranks_emulate(inps, s, mistake), R.rank_chains(s['rows'], s['small_rows']), quiet=True)
    copied = _copied_rank_form(mistake)
    print('%-30s %-32s fails: %-60s copied rank: %s' % (mistake, name, sorted({b.split('[')[0].split(':')[0] for b in bad}),
                                                        'seen' if copied else 'BLIND'))
    assert bad, 'the unequal ranks of %s let the mistake %s pass' % (name, mistake)
    assert (not copied) == (mistake in BLIND_WITH_A_COPIED_RANK), (mistake, copied)


def test_the_copied_rank_form_passes_without_a_mistake():
    assert not _copied_rank_form(None)


# ------------------------------------------------------------------ the replay harness on a toy operator
def _toy_rank(data, extra=None):
    """Two exchanges in a chain: (sum v, n) -> mean, then sum (v - mean)^2 -> variance; `extra`: a rank that issues one exchange
    more, or one of another size."""
    def run(r, all_reduce):
        v = data[r]
        first = np.array([v.sum(), float(len(v))])
        all_reduce(first)
        with np.errstate(divide='ignore', invalid='ignore'):
            mean = first[0] / first[1]
            second = np.array([((v - mean) ** 2).sum()] + ([0.0] if extra == ('size', r) else []))
            all_reduce(second)
            if extra == ('more', r):
                all_reduce(np.zeros(1))
            return {'mean': np.array([mean]), 'var': np.array([second[0] / first[1]])}
    return run


def test_replay_converges_in_three_passes_and_reports_a_sequence_mismatch():
    import _syncbn_ranks as S
    rng = np.random.default_rng(5)
    data = [rng.standard_normal(n) + 3.0 * r for r, n in enumerate((7, 1, 0, 40))]
    out, seq = S.replay(4, _toy_rank(data), 3)
    allv = np.concatenate(data)
    assert seq == [(2, np.dtype('float64')), (1, np.dtype('float64'))]
    for o in out:                                                                             # every rank, the one without rows too
        assert abs(o['mean'][0] - allv.mean()) <= 1e-14 * abs(allv).max() and abs(o['var'][0] - allv.var()) <= 1e-13 * allv.var()
        assert o['var'][0] == out[0]['var'][0]
    with pytest.raises(AssertionError, match='too few'):                                      # two passes: the second sum is not yet right
        S.replay(4, _toy_rank(data), 2)
    for kind in ('more', 'size'):
        with pytest.raises(AssertionError, match=r'rank 0 issued \[\(2, float64\), \(1, float64\)\], rank 2 issued \[\(2, float64\), ') as e:
            S.replay(4, _toy_rank(data, (kind, 2)), 3)
        assert 'wait for each other' in str(e.value)


# ------------------------------------------------------------------ grouped or layer by layer: every rank decides alike
@pytest.mark.parametrize('switch', ['1', '0'])
def test_batch_norm_group_decides_alike_for_one_row_and_for_many(switch, monkeypatch):
    """nn.batch_norm_group chooses between one packed exchange per direction and 2m small ones: a choice that looked at this
    rank's row count would set a rank with one pooled row (or none) against its peers.  The operator is a stub: no kernel runs."""
    from box2mask_amd import functional as F_, nn as ME
    monkeypatch.setenv('B2M_BN_GROUP', switch)
    marker = object()
    monkeypatch.setattr(F_, '_sync_group', lambda: marker)
    grouped, single = [], []
    monkeypatch.setattr(F_, 'batch_norm_group', lambda members, group: (grouped.append((len(members), group)), [m[0] for m in members])[1])
    monkeypatch.setattr(F_, 'batch_norm', lambda feats, *a, **k: (single.append(feats.shape[0]), feats)[1])
    decisions = {}
    for n in (0, 1, 300):
        norms = [ME.MinkowskiBatchNorm(c) for c in R.GROUP_MEMBERS]
        for nm in norms:
            nm.sync = True
            nm.train()
        pooled = ME.PooledTensor(torch.zeros(n, 8))
        ts = [ME.PooledTensor(torch.ones(n, c), pooled.serial) for c in R.GROUP_MEMBERS]
        del grouped[:], single[:]
        out = ME.batch_norm_group(norms, ts)
        assert [tuple(o.F.shape) for o in out] == [(n, c) for c in R.GROUP_MEMBERS]
        decisions[n] = (list(grouped), len(single))
        assert all(int(nm.bn.num_batches_tracked) == 1 for nm in norms)
    want = ([(len(R.GROUP_MEMBERS), marker)], 0) if switch == '1' else ([], len(R.GROUP_MEMBERS))
    assert decisions == {0: want, 1: want, 300: want}, decisions
    # one process (no group): one row is torch's own complaint, as before
    monkeypatch.setattr(F_, '_sync_group', lambda: None)
    nm = ME.MinkowskiBatchNorm(4).train()
    with pytest.raises(ValueError):
        ME.batch_norm_group([nm, nm], [ME.PooledTensor(torch.ones(1, 4))] * 2)
