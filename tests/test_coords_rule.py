"""The dictionary restatement of coordinate maps, kernel maps, rulebooks, XCD runs and row-order keys (tests/_coords_rule.py):
tied to the oracle, tied to definitions that need no implementation, and shown to be SHARP -- every deliberate mistake,
written as a variant of the rule, fails at least one case of the lists tests/test_gpu_coords_edges.py runs on the device."""
import numpy as np
import pytest

import _coords_rule as R
from oracle import sparse_ref as S


def _random_coords(seed, n=1500, side=14, shuffle=True):
    rng = np.random.default_rng(seed)
    c = np.concatenate([rng.integers(0, 3, (n, 1)), rng.integers(0, side, (n, 3))], 1)
    c = np.unique(c, axis=0).astype(np.int32)
    return c[rng.permutation(len(c))] if shuffle else c


# ----------------------------------------------------------------------------- the rule against the oracle
@pytest.mark.parametrize('seed,shuffle', [(0, False), (1, True), (2, True), (3, True)])
def test_rule_matches_the_oracle(seed, shuffle):
    c = _random_coords(seed, shuffle=shuffle)
    h = S.Hierarchy(c, n_levels=4, k0=5)
    r = R.Levels(c, 4)
    for l in range(4):
        assert np.array_equal(r.coords[l], h.coords[l])
        assert np.array_equal(r.same(l, 3), h.k3(l))
        if l < 3:
            assert np.array_equal(r.parent[l], h.parent[l]) and np.array_equal(r.koff[l], h.koff[l])
            assert np.array_equal(r.down(l), h.down(l)) and np.array_equal(r.up(l), h.up(l))
    assert np.array_equal(r.same(0, 5), h.k_first())
    small = c[:300]
    for ks, ts in ((1, 1), (3, 1), (5, 1), (7, 1), (3, 4)):
        assert np.array_equal(R.kernel_map(small, ks, ts), S.kernel_map_bruteforce(small, ks, ts))


def test_rule_matches_the_moved_numpy_restatements():
    rng = np.random.default_rng(4)
    cnt = rng.integers(0, 65, (27, 700)); cnt[rng.random(cnt.shape) < 0.4] = 0
    cost, start, cap = R._expected_runs(cnt)
    c2, s2, _ = R.balance_tail(cnt)
    assert np.array_equal(cost, c2) and np.array_equal(start, s2) and cap == R.xcd_cap(700)
    c = _random_coords(5)
    assert np.array_equal(R.morton_keys(c), R._morton_keys_numpy(c))


# ----------------------------------------------------------------------------- definitions that need no implementation
@pytest.mark.parametrize('ksize', [3, 5, 7])
def test_centre_is_identity_and_offsets_mirror(ksize):
    c = _random_coords(6, n=700, side=9)
    nbr = R.kernel_map(c, ksize, 1)
    K, n = nbr.shape
    assert K == ksize ** 3 and np.array_equal(nbr[K // 2], np.arange(n))
    for k in range(K):
        o = np.flatnonzero(nbr[k] >= 0)
        assert np.array_equal(nbr[K - 1 - k][nbr[k][o]], o)
        dx, dy, dz = R.offsets(ksize)[k]
        assert k == (dx + ksize // 2) + ksize * (dy + ksize // 2) + ksize * ksize * (dz + ksize // 2)
        assert np.array_equal(c[nbr[k][o]][:, 1:], c[o][:, 1:] + [dx, dy, dz]) and np.array_equal(c[nbr[k][o]][:, 0], c[o][:, 0])


def test_every_fine_row_is_exactly_one_parent_koff_pair():
    c = _random_coords(7)
    for ts in (1, 2):
        cc = c.copy(); cc[:, 1:] *= ts
        coarse, parent, koff = R.strided_level(cc, ts)
        down, up = R.child_table(parent, koff, len(coarse)), R.up_table(parent, koff)
        assert (up >= 0).sum() == len(cc) == (down >= 0).sum() and ((up >= 0).sum(0) == 1).all()
        assert np.array_equal(np.sort(down[down >= 0]), np.arange(len(cc)))
        o = np.stack([koff & 1, (koff >> 1) & 1, koff >> 2], 1) * ts
        assert np.array_equal(coarse[parent][:, 1:] + o, cc[:, 1:]) and (coarse[:, 1:] % (2 * ts) == 0).all()
        assert len(np.unique(coarse, axis=0)) == len(coarse)


@pytest.mark.parametrize('bits', [1, 2, 3, 4, 5])
def test_hilbert_keys_walk_a_dense_cube_through_face_adjacent_cells(bits):
    s = 1 << bits
    g = np.stack(np.meshgrid(*[np.arange(s)] * 3, indexing='ij'), -1).reshape(-1, 3)
    c = np.concatenate([np.zeros((len(g), 1), np.int64), g], 1).astype(np.int32)
    k = R.hilbert_keys(c, bits)
    assert np.array_equal(np.sort(k), np.arange(s ** 3, dtype=np.uint64))
    path = g[R.key_order(k)]
    assert (np.abs(np.diff(path, axis=0)).sum(1) == 1).all()


def test_morton_keys_interleave_bit_by_bit():
    c = np.array([[3, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0, 2, 0, 0], [65534, 65534, 65534, 65534]], np.int32)
    k = R.morton_keys(c)
    assert [int(v) for v in k[:4]] == [(3 << 48) | 1, 2, 4, 8]
    assert int(k[4]) == (65534 << 48) | ((1 << 48) - 1 - 7)


def test_rb_cnt_sums_to_the_valid_entries():
    for K, n_out in ((27, 65), (125, 63), (8, 4033)):
        nbr, n_out = R.rulebook_case(K, n_out)
        rb_in, rb_out, cnt, tot = R.encode_rulebook(nbr, n_out)
        assert int(cnt.sum()) == int((nbr[:, :n_out] >= 0).sum()) == int(tot.sum()) == int((rb_in >= 0).sum())
        assert np.array_equal(tot, (nbr[:, :n_out] >= 0).sum(1))


def test_every_case_builds_and_its_predicates_hold():
    n = 0
    for name in R.COORD_CASES:
        case = R.coord_case(name)
        assert all(case.predicates.values()) and case.predicates, name
        n += len(case.predicates)
    for nt in R.BALANCE_NTILES:
        for K in R.BALANCE_K:
            for p in R.BALANCE_PATTERNS:
                R.balance_case(nt, K, p)
    R.key_case()
    assert n > 100


def test_runs_reach_their_branches():
    """per > 1 (more than 1024 tiles), total == 0, both clamps and a run at the cap each occur in the balance list."""
    infos = {(nt, K, p): R.balance_case(nt, K, p)[1] for nt in R.BALANCE_NTILES for K in R.BALANCE_K for p in R.BALANCE_PATTERNS}
    assert max(R.BALANCE_NTILES) > 1024 and {63, 64, 65} <= set(R.BALANCE_NTILES)
    for flag in ('forward_clamp', 'backward_clamp', 'at_cap'):
        assert any(i[flag] for (nt, _, _), i in infos.items() if nt > 1024), flag
    assert any(i['total'] == 0 for i in infos.values())


# ----------------------------------------------------------------------------- the cases are sharp
def _levels_differ(case, mistake):
    good, bad = case.rule(), R.Levels(case.coords, case.levels, mistake)
    for l in range(case.levels):
        if not np.array_equal(good.coords[l], bad.coords[l]):
            return True
        if l + 1 < case.levels and not (np.array_equal(good.parent[l], bad.parent[l]) and np.array_equal(good.koff[l], bad.koff[l])):
            return True
        for ks in (3,) + (case.k0 if l == 0 else ()):
            if not np.array_equal(good.same(l, ks), bad.same(l, ks)):
                return True
    return False


COORD_MISTAKES = {
    'pack16': '16-bit packing without the range guard',
    'z_fastest': 'z-fastest offset order',
    'sorted': 'coarse rows in sorted order instead of first-occurrence order',
    'koff_swap': 'koff with two axes exchanged',
    'round_ts': 'rounding down to ts instead of 2*ts',
    'bitmap_nomask': 'a bitmap-indexed kernel map that does not mask the positions left of x = 0 and right of X-1',
}
# the cases each mistake is tried on (it must fail at least one; which ones it fails is recorded in profiles/coords_rule.md)
_SHARP_CASES = ['top_of_range', 'origin:1', 'origin:2', 'origin:64', 'origin:65', 'count:65', 'count:257', 'strided']


@pytest.mark.parametrize('mistake', sorted(COORD_MISTAKES))
def test_coordinate_mistake_fails_a_case(mistake):
    failed = [name for name in _SHARP_CASES if _levels_differ(R.coord_case(name), mistake)]
    print(mistake, '->', failed)
    assert failed, COORD_MISTAKES[mistake]
    if mistake == 'pack16':            # nothing but the top of the range can see a missing guard
        assert failed == ['top_of_range']
    if mistake == 'bitmap_nomask':
        assert any(f.startswith('origin') for f in failed)


@pytest.mark.parametrize('mistake', ['floor_target', 'forward_only', 'unstable'])
def test_balance_mistake_fails_a_case(mistake):
    failed = []
    for nt in R.BALANCE_NTILES[1:]:
        for K in R.BALANCE_K:
            for p in R.BALANCE_PATTERNS:
                cnt, _ = R.balance_case(nt, K, p)
                cost, start, order = R.balance_tail(cnt)
                if mistake == 'unstable':
                    bad = np.array_equal(order, R.dispatch_order(cost, start, 'unstable'))
                else:
                    bad = np.array_equal(start, R.run_starts(cost, mistake))
                if not bad:
                    failed.append((nt, K, p))
    print(mistake, '->', len(failed), failed[:6])
    assert failed


def test_signed_key_comparison_fails_the_key_case():
    c = R.key_case()
    for keys in (R.morton_keys(c), R.hilbert_keys(c, 16)):
        assert not np.array_equal(R.key_order(keys), R.key_order(keys, 'signed'))
        low = c[:, 0] < 32768                                  # (and only the rows from batch 32768 on make the difference)
        assert np.array_equal(R.key_order(keys[low]), R.key_order(keys[low], 'signed'))


def test_hilbert_order_depends_on_bits_modulo_three():
    """Skilling's transform rotates the axes once per leading zero level: keys computed with b and b + 3 bits order rows alike,
    b + 1 and b + 2 do not.  CoordinateManager(check=False) takes 16 bits; its order equals check=True's when the largest
    coordinate has 16, 13, 10, ... bits.  Either is a Hilbert order; the permutation is undone at the boundary."""
    c = _random_coords(8, n=2000, side=700)
    base = R.key_order(R.hilbert_keys(c, 10))
    assert np.array_equal(base, R.key_order(R.hilbert_keys(c, 13))) and np.array_equal(base, R.key_order(R.hilbert_keys(c, 16)))
    assert not np.array_equal(base, R.key_order(R.hilbert_keys(c, 11)))
    assert not np.array_equal(base, R.key_order(R.hilbert_keys(c, 12)))
