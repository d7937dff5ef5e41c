"""GPU: csrc/coords.hip at its edges, bit for bit against the dictionary rule of tests/_coords_rule.py -- the top of the 16-bit
coordinate range (where only the range guard of the kernel maps keeps an aliased key from being a neighbour), the level-0
occupancy bitmap at the origin corner, at word boundaries and on a wide thin grid, row counts around every block and tile
size, one level above 262 144 rows, shuffled rows, duplicates, b2m_rulebook and b2m_rulebook_balance called directly, and the
row-order keys over the whole range of coordinates and batch indices.  The cases and the predicates that say which branch
each one reaches live in _coords_rule.py and are shown to be sharp on the CPU by tests/test_coords_rule.py.  Every comparison
is exact; every input lies inside the documented domain."""
import numpy as np
import pytest
import torch

import _coords_rule as R

pytestmark = pytest.mark.gpu

TILE = R.TILE


def _np(t):
    return t.cpu().numpy()


def _assert_rulebook(rbs, nbr_rule, tag):
    """rb_in / rb_out / rb_cnt, padding included, and (from 64 tiles on) the tail of rb_cnt equal the rule's arrays."""
    rin, rout, cnt, _ = R.encode_rulebook(nbr_rule)
    tail_rule = None
    for rb in rbs:
        K, nt, n_out = rb.K, rb.ntiles, rb.n_out
        assert nbr_rule.shape == (K, n_out) and nt == (n_out + TILE - 1) // TILE, tag
        ldr = nt * TILE
        assert np.array_equal(_np(rb.rb_in[:K * ldr]), rin), (tag, 'rb_in')
        assert np.array_equal(_np(rb.rb_out[:K * ldr]), rout), (tag, 'rb_out')
        raw = _np(rb.rb_cnt)
        assert raw.shape[0] == K * nt + 16 + 2 * nt, tag
        assert np.array_equal(raw[:K * nt], cnt), (tag, 'rb_cnt')
        if nt >= R.BALANCE_MIN_TILES:
            cost, start, order = tail_rule = tail_rule or R.balance_tail(cnt.reshape(K, nt))
            tail = raw[K * nt:]
            assert np.array_equal(tail[:9], start) and (tail[9:16] == 0).all(), (tag, 'starts', tail[:9], start)
            assert np.array_equal(tail[16:16 + nt], cost), (tag, 'cost')
            assert np.array_equal(tail[16 + nt:], order), (tag, 'order')


def _same_bits(a, b, tag):
    for f in ('rb_in', 'rb_out', 'rb_cnt'):
        x, y = getattr(a, f), getattr(b, f)
        if f == 'rb_cnt' and a.ntiles < R.BALANCE_MIN_TILES:      # (the tail behind the counts is written from 64 tiles on)
            x, y = x[:a.K * a.ntiles], y[:a.K * a.ntiles]
        elif f != 'rb_cnt':                                       # (an empty rulebook is allocated with one spare element)
            x, y = x[:a.K * a.ntiles * TILE], y[:a.K * a.ntiles * TILE]
        assert torch.equal(x, y), (tag, f)


def _check_case(case, k0=None, occ=None):
    """One coordinate case through CoordinateManager, with and without neighbour tables.  occ: True / False = the level-0 map
    must (not) have gone through the occupancy bitmap."""
    from box2mask_amd.sparse import CoordinateManager
    rule, L = case.rule(), case.levels
    ct = torch.from_numpy(case.coords)
    m = CoordinateManager(ct, keep_tables=True)
    m2 = CoordinateManager(ct, keep_tables=False)
    m.ensure_level(L - 1); m2.ensure_level(L - 1)
    assert int(m.dup_count.item()) == R.dup_count(case.coords) == int(m2.dup_count.item())
    for l in range(L):
        for mm in (m, m2):
            assert np.array_equal(_np(mm.coords[l]), rule.coords[l]), (case.name, 'coords', l)
            if l + 1 < L:
                assert np.array_equal(_np(mm.parent[l]), rule.parent[l]), (case.name, 'parent', l)
                assert np.array_equal(_np(mm.koff[l]), rule.koff[l]), (case.name, 'koff', l)
    if case.what == 'dups':
        return m
    for l in range(L - 1):
        down, up = rule.down(l), rule.up(l)
        assert np.array_equal(_np(m.rulebook_down(l).nbr)[:, :rule.n(l + 1)], down), (case.name, 'down', l)
        assert np.array_equal(_np(m.rulebook_up(l).nbr)[:, :rule.n(l)], up), (case.name, 'up', l)
        _assert_rulebook([m.rulebook_down(l), m2.rulebook_down(l)], down, (case.name, 'down', l))
        _assert_rulebook([m.rulebook_up(l), m2.rulebook_up(l)], up, (case.name, 'up', l))
    if case.what == 'strided':
        return m
    for l, ks in [(l, 3) for l in range(L)] + [(0, k) for k in (case.k0 if k0 is None else k0) if k != 3]:
        want = rule.same(l, ks)
        a, b = m.rulebook_same(l, ks), m2.rulebook_same(l, ks)
        assert b.nbr is None
        assert np.array_equal(_np(a.nbr)[:, :rule.n(l)], want), (case.name, 'k%d map' % ks, l)
        _assert_rulebook([a, b], want, (case.name, 'k%d' % ks, l))
        _same_bits(a, b, (case.name, ks, l))
    if occ is not None and case.coords.shape[0]:
        for mm in (m, m2):
            assert isinstance(mm._occ, tuple) if occ else mm._occ is None, (case.name, mm._occ)
    return m


# ----------------------------------------------------------------------------- coordinate cases
@pytest.mark.parametrize('k0', [5, 7])
def test_top_of_the_range(k0):
    """Rows within 40 of 65534 on every axis, eight levels, shuffled, with rows whose unguarded 16-bit pack is another row."""
    _check_case(R.coord_case('top_of_range'), k0=(k0,), occ=False)       # (a 65535^3 grid: no bitmap)


@pytest.mark.parametrize('X', R.ORIGIN_WIDTHS)
def test_origin_corner_with_and_without_the_bitmap(X, monkeypatch):
    from box2mask_amd.sparse import CoordinateManager
    case = R.coord_case('origin:%d' % X)
    _check_case(case, occ=True)
    monkeypatch.setattr(CoordinateManager, 'OCC_MAX_BYTES', 0)
    _check_case(case, occ=False)              # (both runs equal the rule bit for bit, hence each other)


def test_wide_thin_grid():
    _check_case(R.coord_case('wide_thin'), occ=True)


@pytest.mark.parametrize('n', R.COUNT_SIZES)
def test_row_counts(n):
    _check_case(R.coord_case('count:%d' % n))


def test_above_262144_rows():
    """Levels 0 -> 1 -> 2 of ~330 k shuffled rows: coordinates, parent, koff, the down and up rulebooks."""
    _check_case(R.coord_case('big'))


def test_strided_maps():
    _check_case(R.coord_case('strided'))


@pytest.mark.parametrize('kind', ['none', 'one', 'many', 'all'])
def test_duplicates(kind):
    _check_case(R.coord_case('dups:' + kind))


# ----------------------------------------------------------------------------- b2m_rulebook, called directly
@pytest.mark.parametrize('K', R.RULEBOOK_K)
def test_rulebook_direct(K):
    """A leading dimension wider than n_out, pair_total given, K no multiple of 4 (125, 343)."""
    from box2mask_amd import _lib
    for n_out in R.RULEBOOK_N_OUT:
        nbr, _ = R.rulebook_case(K, n_out)
        ld = nbr.shape[1]
        assert ld > n_out
        nt = (n_out + TILE - 1) // TILE
        d = torch.from_numpy(nbr).cuda()
        rb_in = torch.full((K * nt * TILE,), 77, dtype=torch.int32, device='cuda')
        rb_out = torch.full((K * nt * TILE,), 77, dtype=torch.uint8, device='cuda')
        size = _lib.load().b2m_rulebook_cnt_size(K, n_out)
        assert size == K * nt + 16 + 2 * nt
        rb_cnt = torch.full((size,), -7, dtype=torch.int32, device='cuda')
        tot = torch.full((K,), -7, dtype=torch.int32, device='cuda')
        _lib.call('b2m_rulebook', d.data_ptr(), ld, K, n_out, rb_in.data_ptr(), rb_out.data_ptr(), rb_cnt.data_ptr(), tot.data_ptr())
        rin, rout, cnt, total = R.encode_rulebook(nbr, n_out)
        assert np.array_equal(_np(rb_in), rin) and np.array_equal(_np(rb_out), rout), (K, n_out)
        raw = _np(rb_cnt)
        assert np.array_equal(raw[:K * nt], cnt) and np.array_equal(_np(tot), total), (K, n_out)
        if nt < R.BALANCE_MIN_TILES:
            assert (raw[K * nt:] == -7).all(), (K, n_out)
        else:
            cost, start, order = R.balance_tail(cnt.reshape(K, nt))
            assert np.array_equal(raw[K * nt:K * nt + 9], start) and np.array_equal(raw[K * nt + 16:K * nt + 16 + nt], cost)
            assert np.array_equal(raw[K * nt + 16 + nt:], order)


# ----------------------------------------------------------------------------- b2m_rulebook_balance, called directly
@pytest.mark.parametrize('nt', R.BALANCE_NTILES)
def test_rulebook_balance_direct(nt):
    from box2mask_amd import _lib
    for K in R.BALANCE_K:
        for pattern in R.BALANCE_PATTERNS:
            cnt, _ = R.balance_case(nt, K, pattern)
            raw = np.full(K * nt + 16 + 2 * nt, -7, np.int32)
            raw[:K * nt] = cnt.reshape(-1)
            d = torch.from_numpy(raw).cuda()
            _lib.call('b2m_rulebook_balance', d.data_ptr(), K, nt * TILE - 5)
            got = _np(d)
            assert np.array_equal(got[:K * nt], raw[:K * nt]), (nt, K, pattern)
            tail = got[K * nt:]
            if nt < R.BALANCE_MIN_TILES:
                assert (tail == -7).all(), (nt, K, pattern)        # below 64 tiles the tail comes back untouched
                continue
            cost, start, order = R.balance_tail(cnt)
            assert np.array_equal(tail[:9], start) and (tail[9:16] == 0).all(), (nt, K, pattern, tail[:9], start)
            assert np.array_equal(tail[16:16 + nt], cost), (nt, K, pattern)
            assert np.array_equal(tail[16 + nt:], order), (nt, K, pattern)


# ----------------------------------------------------------------------------- keys and row order
def test_keys_over_the_whole_range():
    """Morton keys, and Hilbert keys for 1 .. 16 bits, as unsigned values: coordinates up to 65534, batch indices beyond 32767
    (the stored int64 is then negative)."""
    from box2mask_amd import _lib
    c = R.key_case()
    n = len(c)
    keys = torch.empty(n, dtype=torch.int64, device='cuda')
    ct = torch.from_numpy(c).cuda()
    _lib.call('b2m_morton_keys', ct.data_ptr(), n, keys.data_ptr())
    got = _np(keys)
    assert np.array_equal(got.view(np.uint64), R.morton_keys(c)) and (got < 0).any()
    for bits in range(1, 17):
        cb = c.copy()
        cb[:, 1:] &= (1 << bits) - 1
        ct = torch.from_numpy(cb).cuda()
        _lib.call('b2m_hilbert_keys', ct.data_ptr(), n, bits, keys.data_ptr())
        assert np.array_equal(_np(keys).view(np.uint64), R.hilbert_keys(cb, bits)), bits


@pytest.mark.parametrize('order', ['hilbert', 'morton'])
def test_row_order_is_the_argsort_of_the_unsigned_keys(order, monkeypatch):
    from box2mask_amd.sparse import CoordinateManager
    c = R.key_case()
    monkeypatch.setenv('B2M_ROW_ORDER', order)
    want = R.key_order(R.morton_keys(c) if order == 'morton' else R.hilbert_keys(c, 16))
    ct = torch.from_numpy(c)
    m = CoordinateManager(ct, reorder=True)
    perm = _np(m.perm)
    assert np.array_equal(perm, want)
    assert np.array_equal(_np(m.inv_perm)[want], np.arange(len(c)))
    assert np.array_equal(_np(m.coords[0]), c[want])
    u = CoordinateManager(ct, reorder=True, check=False)
    assert torch.equal(u.perm, m.perm) and torch.equal(u.inv_perm, m.inv_perm)
