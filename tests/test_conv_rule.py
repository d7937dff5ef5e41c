"""tests/_conv_rule.py held to independent references, without a GPU.

  1. the rule == autograd of oracle.sparse_ref.conv_nbr in float64 (forward, dX, dW, db), and on coordinate-derived tables
     (kernel_map_same, child_table, up_table) == F.conv3d / conv_transpose3d on a small dense grid;
  2. exact operands: an fp32 evaluation of every case in three orders (offset-major, reversed, 16 partial sums added last) IS
     the float64 rule bit for bit, and the exactness check rejects operands that break its condition;
  3. full-mantissa operands: the same three fp32 evaluations stay inside the derived bound (largest ratio printed);
  4. deliberate mistakes in the fp32 evaluator each FAIL the comparison tests/test_gpu_conv_edges.py makes, at the smallest and
     at the largest case of their kind.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_rule as R
from oracle import sparse_ref as S

# (kind, K, n_out, n_in, c1, c2, cout): the smallest and the largest case of every table kind, both directions of n_in != n_out
CASES = [
    ('dense', 27, 65, 65, 16, 0, 16), ('dense', 8, 129, 200, 32, 0, 48), ('dense', 27, 513, 300, 48, 0, 80),
    ('centre', 27, 1, 1, 16, 0, 16), ('centre', 27, 700, 700, 96, 32, 96),
    ('mixed', 27, 129, 129, 20, 0, 13), ('mixed', 27, 4033, 4033, 96, 32, 128),
    ('random', 8, 63, 40, 32, 0, 32), ('random', 27, 700, 900, 256, 128, 256),
    ('broadcast', 27, 129, 64, 32, 0, 32), ('broadcast', 8, 513, 513, 64, 0, 3),
    ('last_row', 125, 64, 64, 8, 0, 32), ('last_row', 27, 4033, 4033, 16, 0, 16),
]
_id = lambda c: '%s-K%d-%d<-%d-%d+%d-%d' % c


def _case(c, family='exact', seed=3):
    kind, K, n_out, n_in, c1, c2, cout = c
    nbr = R.table(kind, K, n_out, n_in, seed)
    ops = (R.exact_operands if family == 'exact' else R.full_operands)(seed, n_in, c1, c2, K, cout, n_out)
    return nbr, ops


# ------------------------------------------------------------------ 1. the rule against independent references
@pytest.mark.parametrize('c', CASES[:4] + CASES[5:6] + CASES[7:8] + CASES[9:12], ids=_id)
def test_rule_equals_autograd_of_the_oracle(c):
    kind, K, n_out, n_in, c1, c2, cout = c
    nbr, ops = _case(c, 'full')
    x = R._cat(ops['x1'], ops['x2']).double().requires_grad_(True)
    w = ops['w'].double().requires_grad_(True)
    b = ops['bias'].double().requires_grad_(True)
    y = S.conv_nbr(x, w, nbr, b)
    y.backward(ops['dy'].double())
    tol = lambda ref: 1e-12 * max(float(ref.abs().max()), 1.0)
    got = R.conv_fwd(nbr, ops['x1'], ops['x2'], ops['w'], ops['bias'])
    assert float((got - y.detach()).abs().max()) <= tol(y.detach())
    # accumulate: onto y0, nothing else changes
    got0 = R.conv_fwd(nbr, ops['x1'], ops['x2'], ops['w'], ops['bias'], ops['y0'])
    assert float((got0 - (y.detach() + ops['y0'].double())).abs().max()) <= tol(got0)
    dx = R.conv_dgrad(nbr, ops['dy'], ops['w'], n_in)
    assert float((dx - x.grad).abs().max()) <= tol(x.grad)
    if c2:                                      # one source's slice of the data gradient
        dx2 = R.conv_dgrad(nbr, ops['dy'], ops['w'], n_in, c1, c2)
        assert float((dx2 - x.grad[:, c1:]).abs().max()) <= tol(x.grad)
    dw = R.conv_wgrad(nbr, R._cat(ops['x1'], ops['x2']), ops['dy'], torch.zeros_like(ops['w']))
    assert float((dw - w.grad).abs().max()) <= tol(w.grad)
    # onto dW0 at a channel offset: the second source's rows of a two-source dW
    dw1 = R.conv_wgrad(nbr, ops['x1'], ops['dy'], ops['dw0'], 0)
    assert float((dw1[:, :c1] - (w.grad[:, :c1] + ops['dw0'].double()[:, :c1])).abs().max()) <= tol(w.grad)
    assert torch.equal(dw1[:, c1:], ops['dw0'].double()[:, c1:])
    assert float((ops['dy'].double().sum(0, keepdim=True) - b.grad).abs().max()) <= tol(b.grad)      # db = column sums of dY
    # the reverse table: the data gradient as a forward pass over it with W^T
    if R.has_reverse(nbr):
        rev = R.reverse_table(nbr, n_in)
        dxr = R.conv_fwd(rev, ops['dy'], None, ops['w'].transpose(1, 2).contiguous())
        assert float((dxr - dx).abs().max()) <= tol(dx)


def test_rule_equals_dense_convolution_on_coordinate_tables():
    from _dense import random_sites as _random_sites, dense_weight as _dense_weight, scatter_dense as _scatter_dense, read_dense as _read_dense
    shape = (2, 10, 8, 6)
    fine = _random_sites(*shape, 0.35, 5)
    coarse, parent, koff = S.stride_coords(fine, 1)
    nf, nc = len(fine), len(coarse)
    cin, cout = 5, 7
    g = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-11 * max(float(b.abs().max()), 1.0)
    # stride 1, 3x3x3: the table is its own reverse with the offsets mirrored
    nbr = S.kernel_map_same(fine, 3, 1)
    assert np.array_equal(R.reverse_table(nbr, nf), nbr[::-1])
    x, w, gy = rnd(nf, cin).requires_grad_(True), rnd(27, cin, cout).requires_grad_(True), rnd(nf, cout)
    yd = _read_dense(F.conv3d(_scatter_dense(x, fine, shape), _dense_weight(w, 3), padding=1), fine)
    yd.backward(gy)
    assert close(R.conv_fwd(nbr, x.detach(), None, w.detach()), yd.detach())
    assert close(R.conv_dgrad(nbr, gy, w.detach(), nf), x.grad)
    assert close(R.conv_wgrad(nbr, x.detach(), gy, torch.zeros(27, cin, cout)), w.grad)
    assert close(R.eval_dgrad(nbr, gy, w.detach(), nf, mirror=True, dtype=torch.float64), x.grad)
    # k2s2 fine -> coarse
    nbr = S.child_table(parent, koff, nc)
    x, w, gy = rnd(nf, cin).requires_grad_(True), rnd(8, cin, cout).requires_grad_(True), rnd(nc, cout)
    yd = _read_dense(F.conv3d(_scatter_dense(x, fine, shape), _dense_weight(w, 2), stride=2), coarse, 2)
    yd.backward(gy)
    assert close(R.conv_fwd(nbr, x.detach(), None, w.detach()), yd.detach())
    assert close(R.conv_dgrad(nbr, gy, w.detach(), nf), x.grad)
    assert close(R.conv_wgrad(nbr, x.detach(), gy, torch.zeros(8, cin, cout)), w.grad)
    assert np.array_equal(R.reverse_table(nbr, nf), S.up_table(parent, koff))
    # transposed k2s2 coarse -> the existing fine sites
    nbr = S.up_table(parent, koff)
    cshape = (shape[0],) + tuple(s // 2 for s in shape[1:])
    x, w, gy = rnd(nc, cin).requires_grad_(True), rnd(8, cin, cout).requires_grad_(True), rnd(nf, cout)
    wt = w.reshape(2, 2, 2, cin, cout).permute(3, 4, 2, 1, 0).contiguous()
    yd = _read_dense(F.conv_transpose3d(_scatter_dense(x, coarse, cshape, 2), wt, stride=2), fine)
    yd.backward(gy)
    assert close(R.conv_fwd(nbr, x.detach(), None, w.detach()), yd.detach())
    assert close(R.conv_dgrad(nbr, gy, w.detach(), nc), x.grad)
    assert close(R.conv_wgrad(nbr, x.detach(), gy, torch.zeros(8, cin, cout)), w.grad)


def test_table_generators_have_the_features_their_names_promise():
    for K, n_out, n_in in ((27, 4033, 4033), (8, 129, 200), (27, 513, 300)):
        nt = (n_out + 63) // 64
        d = R.table('dense', K, n_out, n_in)
        assert (d >= 0).all() and d.max() < n_in
        c = R.table('centre', K, n_out, n_in)
        assert (c[K // 2] >= 0).all() and (np.delete(c, K // 2, 0) == -1).all()
        m = R.table('mixed', K, n_out, n_in)
        cnt = np.stack([(m[:, t * 64:(t + 1) * 64] >= 0).sum(1) for t in range(nt)], 1)      # [K, ntiles]
        assert (cnt[1] == 0).all() and (cnt[:, 1] == 0).all()                                   # an empty offset, an empty tile
        for t in [t for t in (0, 2) if n_out >= 64 * (t + 1)]:               # (whole tiles)
            assert (cnt[:, t] == 64).any() and (cnt[:, t] == 1).any() and ((cnt[:, t] > 1) & (cnt[:, t] < 64)).any()
        r = R.table('random', K, n_out, n_in)
        assert 0.25 < (r >= 0).mean() < 0.35
        b = R.table('broadcast', K, n_out, n_in)
        assert set(np.unique(b[b >= 0])) == {n_in // 2, n_in - 1}
        l = R.table('last_row', K, n_out, n_in)
        assert (l >= 0).sum() == 1 and l[K - 1, n_out - 1] == n_in - 1
        assert R.has_reverse(d) == (n_in >= n_out) and not R.has_reverse(b)
        f = R.few_pairs_table(K, n_out, n_in, 48)
        assert ((f >= 0).sum(1) == 48).all() and R.has_reverse(f) and f.max() < n_in
        assert len(np.unique(np.nonzero(f >= 0)[1] // 64)) > min(nt, 48) // 2                  # ... spread over the tiles
        t2 = R.two_neighbour_table(K, n_out, n_in)
        assert (t2[K // 2] >= 0).all() and (t2 >= 0).sum(0).max() == 2 and (t2 >= 0).sum(0).min() == 1
    ops = R.exact_operands(0, 4033, 8, 16, 27, 24, 4033)
    for k in ('x1', 'x2', 'dy'):
        assert len(np.unique(ops[k].numpy(), axis=0)) == 4033, k
    assert not torch.equal(ops['x1'][:, :8], ops['x2'][:, :8])


# ------------------------------------------------------------------ 2. exact operands
def _all_exact(nbr, ops, n_in, c1, c2):
    """Every quantity of a case from the rule, with its exactness condition asserted: name -> float64 reference."""
    g = ops['g']
    x = R._cat(ops['x1'], ops['x2'])
    ref = {'fwd': R.conv_fwd(nbr, ops['x1'], ops['x2'], ops['w'], ops['bias'], ops['y0'])}
    R.assert_exact(R.S_fwd(nbr, ops['x1'], ops['x2'], ops['w'], ops['bias'], ops['y0']), ref['fwd'], g)
    ref['dgrad'] = R.conv_dgrad(nbr, ops['dy'], ops['w'], n_in, dx0=ops['dx0'])
    R.assert_exact(R.S_dgrad(nbr, ops['dy'], ops['w'], n_in, dx0=ops['dx0']), ref['dgrad'], g)
    ref['wgrad'] = R.conv_wgrad(nbr, ops['x2'] if c2 else x, ops['dy'], ops['dw0'], c1 if c2 else 0)
    R.assert_exact(R.S_wgrad(nbr, ops['x2'] if c2 else x, ops['dy'], ops['dw0'], c1 if c2 else 0), ref['wgrad'], 1.0)
    return ref


@pytest.mark.parametrize('c', CASES, ids=_id)
def test_fp32_in_three_orders_is_the_rule_bit_for_bit(c):
    kind, K, n_out, n_in, c1, c2, cout = c
    nbr, ops = _case(c)
    ref = _all_exact(nbr, ops, n_in, c1, c2)
    x = R._cat(ops['x1'], ops['x2'])
    for order in R.ORDERS:
        y = R.eval_fwd(nbr, ops['x1'], ops['x2'], ops['w'], ops['bias'], ops['y0'], order, width=cout + 4)
        assert R.same(y[:, :cout], ref['fwd']) and bool((y[:, cout:] == -7).all()), order
        if R.has_reverse(nbr):
            assert R.same(R.eval_dgrad(nbr, ops['dy'], ops['w'], n_in, dx0=ops['dx0'], order=order), ref['dgrad']), order
        dw = R.eval_wgrad(nbr, ops['x2'] if c2 else x, ops['dy'], ops['dw0'], c1 if c2 else 0, order)
        assert R.same(dw, ref['wgrad']), order
        for res, relu in ((None, False), (ops['res'], True)):
            e = R.eval_epilogue(y[:, :cout], ops['scale'], ops['shift'], res, relu)
            assert R.same(e, R.epilogue(ref['fwd'], ops['scale'], ops['shift'], res, relu))
    assert torch.equal(R.eval_tile_sums(y[:, :cout], n_out), R.tile_sums(ref['fwd']))


def test_exactness_check_rejects_operands_that_break_the_condition():
    c = ('dense', 27, 65, 65, 256, 0, 16)
    kind, K, n_out, n_in, c1, c2, cout = c
    nbr = R.table(kind, K, n_out, n_in)
    ops = R.exact_operands(0, n_in, c1, c2, K, cout, n_out, xmax=2048, wmax=2048, g=2.0 ** -10)      # S ~ 27 * 256 * 2^20 g
    ref = R.conv_fwd(nbr, ops['x1'], None, ops['w'])
    with pytest.raises(R.NotExact):
        R.assert_exact(R.S_fwd(nbr, ops['x1'], None, ops['w']), ref, ops['g'])
    assert not R.same(R.eval_fwd(nbr, ops['x1'], None, ops['w']), ref)          # ... and fp32 is indeed not exact there
    ops = R.exact_operands(0, n_in, c1, c2, K, cout, n_out)
    w = ops['w'] * 1.0625                                                        # off the grid
    ref = R.conv_fwd(nbr, ops['x1'], None, w)
    with pytest.raises(R.NotExact):
        R.assert_exact(R.S_fwd(nbr, ops['x1'], None, w), ref, ops['g'])
    with pytest.raises(R.NotExact):
        R.assert_half_exact(torch.tensor([2049.0 * 0.125]), 0.125)
    R.assert_half_exact(torch.tensor([2048.0 * 0.125]), 0.125)


# ------------------------------------------------------------------ 3. full-mantissa operands: inside the bound
# short sums only (T <= 64): the centre offset, or the centre and a second offset on half of the rows; cin 16 / 32
BOUND_CASES = [(tab, K, n, n, cin, 0, cout) for tab in ('centre', 'two') for K, n, cin, cout in
               ((27, 65, 16, 32), (27, 4033, 32, 16), (8, 65, 32, 32), (1, 4033, 16, 13), (125, 65, 8, 32))
               if not (tab == 'two' and (K == 1 or cin == 32))]


def _bound_case(c, seed=4):
    tab, K, n_out, n_in, c1, c2, cout = c
    nbr = R.table('centre', K, n_out, n_in, seed) if tab == 'centre' else R.two_neighbour_table(K, n_out, n_in, seed)
    ops = R.full_operands(seed, n_in, c1, c2, K, cout, n_out)
    T = R.terms_fwd(nbr, c1 + c2)
    assert float(T.max()) <= 64
    return nbr, ops, T


@pytest.mark.parametrize('c', BOUND_CASES, ids=_id)
def test_fp32_in_three_orders_stays_inside_the_bound(c):
    tab, K, n_out, n_in, c1, c2, cout = c
    nbr, ops, T = _bound_case(c)
    ref = R.conv_fwd(nbr, ops['x1'], None, ops['w'], ops['bias'], ops['y0'])
    bnd = R.bound(T, R.S_fwd(nbr, ops['x1'], None, ops['w'], ops['bias'], ops['y0']))
    refd = R.conv_dgrad(nbr, ops['dy'], ops['w'], n_in, dx0=ops['dx0'])
    bndd = R.bound(R.terms_dgrad(nbr, cout, n_in), R.S_dgrad(nbr, ops['dy'], ops['w'], n_in, dx0=ops['dx0']))
    worst = 0.0
    for order in R.ORDERS:
        ok, r = R.inside(R.eval_fwd(nbr, ops['x1'], None, ops['w'], ops['bias'], ops['y0'], order), ref, bnd)
        assert ok, (order, r)
        ok, r2 = R.inside(R.eval_dgrad(nbr, ops['dy'], ops['w'], n_in, dx0=ops['dx0'], order=order), refd, bndd)
        assert ok, (order, r2)
        worst = max(worst, r, r2)
    # the weight gradient's sums are as long as an offset has pairs: its short sums come from a table with 48 pairs per offset,
    # spread over all tiles.  n = T + 16 as everywhere: a product in a partial sum of t pairs meets at most t roundings there and
    # one add per partial sum; every add of a further partial sum shortens a chain by at least one pair, so T + 1 (dW0) covers it
    few = R.few_pairs_table(K, n_out, n_in, 48, seed=4)
    Tw = R.terms_wgrad(few)
    assert float(Tw.max()) <= 64
    refw = R.conv_wgrad(few, ops['x1'], ops['dy'], ops['dw0'])
    bndw = R.bound(Tw, R.S_wgrad(few, ops['x1'], ops['dy'], ops['dw0']))
    for order in R.ORDERS:
        ok, r = R.inside(R.eval_wgrad(few, ops['x1'], ops['dy'], ops['dw0'], 0, order), refw, bndw)
        assert ok, (order, r)
        worst = max(worst, r)
    print('largest error / bound: %.3f' % worst)


# ------------------------------------------------------------------ 4. deliberate mistakes must fail
SMALL = ('random', 8, 65, 65, 16, 16, 32)
LARGE = ('mixed', 27, 4033, 4033, 96, 32, 128)
FWD_MISTAKES = ['drop_pair', 'dup_pair', 'mirror_k', 'transpose_w', 'swap_sources', 'skip_channel', 'overhang', 'bias_per_slice',
                'y0_ignored', 'y0_twice']


@pytest.fixture(scope='module')
def mistake_cases():
    out = {}
    for name, c in (('small', SMALL), ('large', LARGE)):
        kind, K, n_out, n_in, c1, c2, cout = c
        nbr, ops = _case(c)
        out[name] = (c, nbr, ops, _all_exact(nbr, ops, n_in, c1, c2))
    return out


@pytest.mark.parametrize('size', ['small', 'large'])
@pytest.mark.parametrize('mut', FWD_MISTAKES)
def test_forward_mistake_fails_the_exact_comparison(mistake_cases, mut, size):
    (kind, K, n_out, n_in, c1, c2, cout), nbr, ops, ref = mistake_cases[size]
    order = 'split16' if mut == 'bias_per_slice' else 'offset_major'
    wide = torch.full((n_out, cout + 4), -7.0, dtype=torch.float64)
    wide[:, :cout] = ref['fwd']
    good = R.eval_fwd(nbr, ops['x1'], ops['x2'], ops['w'], ops['bias'], ops['y0'], order, width=cout + 4)
    assert R.same(good, wide)
    bad = R.eval_fwd(nbr, ops['x1'], ops['x2'], ops['w'], ops['bias'], ops['y0'], order, mut=mut, width=cout + 4)
    assert not R.same(bad, wide)


@pytest.mark.parametrize('size', ['small', 'large'])
@pytest.mark.parametrize('mut', ['drop_pair', 'dup_pair', 'dw_offset_0'])
def test_weight_gradient_mistake_fails_the_exact_comparison(mistake_cases, mut, size):
    (kind, K, n_out, n_in, c1, c2, cout), nbr, ops, ref = mistake_cases[size]
    assert R.same(R.eval_wgrad(nbr, ops['x2'], ops['dy'], ops['dw0'], c1), ref['wgrad'])
    assert not R.same(R.eval_wgrad(nbr, ops['x2'], ops['dy'], ops['dw0'], c1, mut=mut), ref['wgrad'])


@pytest.mark.parametrize('size', ['small', 'large'])
def test_epilogue_and_tile_sum_mistakes_fail(mistake_cases, size):
    (kind, K, n_out, n_in, c1, c2, cout), nbr, ops, ref = mistake_cases[size]
    y = ref['fwd'].float()
    want = R.epilogue(ref['fwd'], ops['scale'], ops['shift'], ops['res'], True)
    assert R.same(R.eval_epilogue(y, ops['scale'], ops['shift'], ops['res'], True), want)
    assert not R.same(R.eval_epilogue(y, ops['scale'], ops['shift'], ops['res'], True, mut='relu_before_res'), want)
    buf = torch.cat([y, ops['bias'] + 1.0])                   # the buffer's next row: what a kernel finds in a row that does not exist
    assert n_out % 64 != 0
    assert torch.equal(R.eval_tile_sums(buf, n_out), R.tile_sums(ref['fwd']))
    assert not torch.equal(R.eval_tile_sums(buf, n_out, mut='row_past_n_out'), R.tile_sums(ref['fwd']))


@pytest.mark.parametrize('shape', [(1, 4, 3, 3), (2, 14, 12, 10)])
def test_unmirrored_data_gradient_fails(shape):
    """A stride-1 map is its own reverse with the offsets mirrored: the data gradient gathers dY through the same table with
    W[K-1-k]^T.  Taking W[k]^T instead must fail (on the smallest and the largest coordinate-derived map used here)."""
    from _dense import random_sites as _random_sites
    coords = _random_sites(*shape, 0.5, 9)
    n = len(coords)
    nbr = S.kernel_map_same(coords, 3, 1)
    ops = R.exact_operands(1, n, 16, 0, 27, 32, n)
    ref = R.conv_dgrad(nbr, ops['dy'], ops['w'], n)
    R.assert_exact(R.S_dgrad(nbr, ops['dy'], ops['w'], n), ref, ops['g'])
    assert R.same(R.eval_dgrad(nbr, ops['dy'], ops['w'], n, mirror=True), ref)
    assert not R.same(R.eval_dgrad(nbr, ops['dy'], ops['w'], n, mirror=True, mut='dx_not_mirrored'), ref)


@pytest.mark.parametrize('c', [BOUND_CASES[0], BOUND_CASES[1], BOUND_CASES[-1]], ids=_id)
@pytest.mark.parametrize('mut', ['x_11_bits', 'acc_half_once'])
def test_arithmetic_mistake_leaves_the_bound(c, mut):
    """What exact operands cannot see: an operand with 11 mantissa bits, an accumulator that passes through binary16 once."""
    tab, K, n_out, n_in, c1, c2, cout = c
    nbr, ops, T = _bound_case(c)
    ref = R.conv_fwd(nbr, ops['x1'], None, ops['w'], ops['bias'], ops['y0'])
    bnd = R.bound(T, R.S_fwd(nbr, ops['x1'], None, ops['w'], ops['bias'], ops['y0']))
    ok, r = R.inside(R.eval_fwd(nbr, ops['x1'], None, ops['w'], ops['bias'], ops['y0'], mut=mut), ref, bnd)
    print('%s: error / bound %.1f' % (mut, r))
    assert not ok and r > 10
    few = R.few_pairs_table(K, n_out, n_in, 48, seed=4)
    refw = R.conv_wgrad(few, ops['x1'], ops['dy'], ops['dw0'])
    bndw = R.bound(R.terms_wgrad(few), R.S_wgrad(few, ops['x1'], ops['dy'], ops['dw0']))
    ok, r = R.inside(R.eval_wgrad(few, ops['x1'], ops['dy'], ops['dw0'], mut=mut), refw, bndw)
    assert not ok and r > 10, r
