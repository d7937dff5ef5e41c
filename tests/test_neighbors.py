"""The yardstick of the nearest-neighbour tests, checked on the CPU: numpy brute force in the contract's summation order
(tests/_neighbors_cases.py) is unambiguous on every seeded case that is not built to tie, and sklearn's ball tree and scipy's
k-d tree -- the searches the reference runs -- return its rows and its distances bit for bit.  Then the two fixtures taken from
the reference (tools/gen_golden.py s3dis_labels, s3dis_full): numpy restatements of ``prepare.s3dis_point_labels`` and of the
full-resolution gather reproduce what the reference returned, exactly."""
import os

import numpy as np
import pytest
from scipy.spatial import cKDTree
from sklearn.neighbors import NearestNeighbors

import _neighbors_cases as NC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NO_TIES = [n for n in NC.SMALL if not NC.case(n)[2]]


def _d2(ref, q, rows):
    d = q - ref[rows]
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def _gap_ok(best, second):
    """second > best by a relative 1e-9, for EVERY query (none is left out)."""
    return bool(np.all(second - best > NC.GAP * best))


@pytest.mark.parametrize('name', NO_TIES)
def test_brute_force_is_unambiguous_and_the_trees_agree(name):
    ref, q, _ = NC.case(name)
    idx, best, second = NC.brute(ref, q)
    ok_q = np.isfinite(q).all(1)
    ok_r = np.isfinite(ref).all(1)
    assert _gap_ok(best[ok_q], second[ok_q]), 'two candidates within a relative %g' % NC.GAP
    rows = np.nonzero(ok_r)[0]                                              # the trees refuse non-finite rows: leave them out
    r, qq = ref[ok_r], q[ok_q]
    bd, bi = NearestNeighbors(n_neighbors=1, algorithm='ball_tree').fit(r).kneighbors(qq)
    kd, ki = cKDTree(r).query(qq, k=1)
    for d, i in ((bd[:, 0], bi[:, 0]), (kd, ki)):
        assert np.array_equal(rows[i], idx[ok_q])
        assert np.array_equal(d, np.sqrt(best[ok_q]))
    assert (idx[~ok_q] == -1).all() and np.isnan(best[~ok_q]).all() and not np.isin(idx, np.nonzero(~ok_r)[0]).any()


def test_the_large_case_is_unambiguous():
    """70 001 x 70 001 is too much for brute force in a quick test: the two nearest rows come from the k-d tree and their distances
    are recomputed in the contract's order; the ball tree returns the same rows and bit-equal distances."""
    ref, q, _ = NC.case('i')
    kd, ki = cKDTree(ref).query(q, k=2)
    best, second = _d2(ref, q, ki[:, 0]), _d2(ref, q, ki[:, 1])
    assert _gap_ok(best, second)
    assert np.array_equal(kd[:, 0], np.sqrt(best))
    bd, bi = NearestNeighbors(n_neighbors=1, algorithm='ball_tree').fit(ref).kneighbors(q)
    assert np.array_equal(bi[:, 0], ki[:, 0]) and np.array_equal(bd[:, 0], np.sqrt(best))


def test_tie_cases_do_tie():
    ref, q, ties = NC.case('e')
    d2 = NC.d2_rows(ref, q)
    assert ties and ((d2 == d2.min(1, keepdims=True)).sum(1) == 8).all()
    ref, q, ties = NC.case('d')
    d2 = NC.d2_rows(ref, q)
    assert ties and (d2[60] == 0).sum() == 21 and NC.brute(ref, q)[0][60] == 0


# ---------------------------------------------------------------- the edge cases (tests/test_gpu_neighbors_edges.py runs them)
EDGE_NO_TIES = [n for n in NC.EDGE_ORDER if not NC.edge_case(n)[2]] + NC.SHELLS
EDGE_TIES = [n for n in NC.EDGE_ORDER if NC.edge_case(n)[2]]


@pytest.mark.parametrize('name', EDGE_NO_TIES)
def test_edge_cases_are_unambiguous(name):
    ref, q, _ = NC.edge_case(name)
    idx, best, second = NC.edge_brute(name)
    ok_q = np.isfinite(q).all(1)
    assert ok_q.all() and (idx >= 0).all() and np.isfinite(ref[idx]).all()
    assert _gap_ok(best, second), 'two candidates within a relative %g' % NC.GAP


def test_tie_edge_cases_do_tie():
    for name in EDGE_TIES:
        ref, q, _ = NC.edge_case(name)
        idx, best, second = NC.edge_brute(name)
        tied = second == best
        assert tied.any(), name
        with np.errstate(all='ignore'):
            d2 = NC.d2_rows(ref, q)
        d2[:, ~np.isfinite(ref).all(1)] = np.nan
        low = np.array([np.nonzero(r == b)[0][0] for r, b in zip(d2, best)])
        assert np.array_equal(low, idx), (name, 'the lowest of the tied rows')
        if name in ('two_identical', 'all_identical', 'denormal', 'denormal_min'):
            assert tied.all() and (idx == 0).all(), name
        if name == 'denormal':
            assert np.ptp(ref, 0).max() <= 1e-320 and (d2 == d2[:, :1]).all()                    # every row ties for every query
        if name == 'extent_1e300':
            assert np.isinf(best[:100]).all() and (idx[:100] == 0).all() and (best[100:] == 0).all()
            assert np.array_equal(idx[100:], np.arange(100, 150))
        if name == 'overflow':
            assert np.isinf(d2[:, 1:]).all() and (idx == 1).all() and np.isnan(ref[0]).any()      # the lowest FINITE row, at +inf
        if name.startswith('lattice'):
            m = int(name[7:])
            n_tied = (d2 == best[:, None]).sum(1)
            per = (m - 1) ** 3
            assert np.array_equal(n_tied, np.repeat([2, 2, 2, 4, 4, 4, 8], per)), name
            # ties across cells: the tied rows of a query lie in different shells around the query's cell
            grid = NC.grid_of(ref)
            spread = 0
            for j in range(len(q)):
                rows = np.nonzero(d2[j] == best[j])[0]
                sh = NC.shell_of(np.repeat(q[j:j + 1], len(rows), 0), ref[rows], grid)
                spread += int(sh.min() != sh.max())
            assert spread >= len(q) // 10, (name, spread)


def test_equidistant_rows_r_and_r_plus_1_cells_away():
    """Query j of 'equidistant' is exactly half-way between two rows, one j cells from its cell and one j + 1, whatever the last
    places of the edge; brute force takes the lower row."""
    ref, q, _ = NC.edge_case('equidistant')
    idx, best, second = NC.edge_brute('equidistant')
    d2 = NC.d2_rows(ref, q)
    assert (second == best).all()
    for j, r in enumerate(NC.EQUI_R):
        rows = np.nonzero(d2[j] == best[j])[0]
        assert len(rows) == 2 and idx[j] == rows[0] and (ref[rows, 1] == q[j, 1]).all()
        for scale in (1 - 1e-9, 1.0, 1 + 1e-9):
            sh = NC.shell_of(np.repeat(q[j:j + 1], 2, 0), ref[rows], NC.grid_of(ref, scale))
            assert sorted(sh.tolist()) == [r, r + 1], (j, sh)


@pytest.mark.parametrize('kind', list(NC.SHELL_DIRS))
def test_shell_cases_put_the_winner_in_shell_r(kind):
    for r in NC.SHELL_R:
        ref, q, winner, decoy, s = NC.shell_case(kind, r)
        idx, best, second = NC.edge_brute('shell:%s:%d' % (kind, r))
        assert idx[0] == winner, (kind, r)
        d_decoy = NC.d2_rows(ref[decoy:decoy + 1], q)[0, 0]
        assert second[0] == d_decoy > best[0] * 1.05 ** 2, (kind, r, 'the decoy is the runner-up, farther than the winner')
        assert np.ptp(ref, 0).tolist() == [1.0, 1.0, 1.0]
        for scale in (1 - 1e-9, 1.0, 1 + 1e-9):                                 # (whatever the last places of the device's edge)
            grid = NC.grid_of(ref, scale)
            assert grid[3].tolist() == [21, 21, 21]
            assert NC.shell_of(q, ref[[winner]], grid)[0] == r, (kind, r, scale)
            assert NC.shell_of(q, ref[[decoy]], grid)[0] == s, (kind, r, scale)
            # every shell nearer than r holds only farther rows
            near = NC.shell_of(np.repeat(q, len(ref), 0), ref, grid) < r
            assert (NC.d2_rows(ref[near], q)[0] > best[0]).all()
        assert s < r or r == 0, (kind, r, s)
        assert second[0] > ((r - 1) * grid[2]) ** 2 or r < 2, 'the walk cannot stop at the decoy before it reaches shell r'


def test_edge_cases_reach_the_branches_of_the_edge_choice():
    g = {n: NC.grid_of(NC.edge_case(n)[0]) for n in ('one_row', 'two_identical', 'all_identical', 'denormal', 'extent_1e300', 'growth',
                                                       'line', 'long_scan', 'only_last_finite')}
    for n in ('one_row', 'two_identical', 'all_identical', 'only_last_finite'):
        assert g[n][2] == 1.0 and g[n][3].tolist() == [1, 1, 1], n                 # k = 0: one cell
    lo, hi, edge, dim = g['denormal']
    assert (hi - lo).max() / 524288.0 == 0.0 and 0 < edge < (hi - lo).max() <= 1e-320          # `least` underflows, the edge does not
    lo, hi, edge, dim = NC.grid_of(NC.edge_case('denormal_min')[0])
    assert edge == (hi - lo).max() == 3 * 5e-324 and dim.tolist() == [2, 2, 2]                  # the edge underflows: the guard
    lo, hi, edge, dim = g['extent_1e300']
    assert np.isfinite(edge) and dim.prod() <= 4 * 300 + 8
    lo, hi, edge, dim = g['growth']
    ext = hi - lo
    assert ext.max() / 524288.0 > np.exp(np.log(ext).sum() / 3 - np.log(4000.0) / 3), 'the clip is what sets the first edge'
    assert edge > 2 * ext.max() / 524288.0 and dim[0] == dim[1] == 1 and 4000 < dim[2] <= 8008, 'and the growth loop has run'
    lo, hi, edge, dim = g['line']
    assert edge == (hi - lo).max() / 524288.0 and dim.tolist() == [524289, 1, 1], 'the clip at 2^19 cells per axis'
    lo, hi, edge, dim = g['long_scan']
    cells = NC.cell_of(NC.edge_case('long_scan')[0], g['long_scan'])
    assert (cells[:5000] == 0).all() and dim.min() > 10


def test_queries_outside_the_box_and_their_clamped_cells():
    ref, q, _ = NC.edge_case('outside')
    idx = NC.edge_brute('outside')[0]
    grid = NC.grid_of(ref)
    lo, hi = grid[0], grid[1]
    n_out = ((q < lo) | (q > hi)).sum(1)
    assert (n_out >= 1).all() and {1, 2, 3} == set(n_out.tolist())                  # beyond a face, an edge, a corner
    gap = np.where(q < lo, lo - q, np.where(q > hi, q - hi, 0)).max(1) / (hi - lo).max()      # in box sizes
    assert gap.min() < 2e-9 and abs(np.median(gap) - 1) < 1e-9 and gap.max() > 999
    sh = NC.shell_of(q, ref[idx], grid)
    assert (sh > 0).sum() >= 10 and (sh == 0).any(), 'the nearest row is often not in the clamped cell'


# ---------------------------------------------------------------- the fixtures taken from the reference
def test_labels_fixture_holds_its_cases_and_the_restatement_reproduces_the_reference():
    import _s3dis_full_rule as F
    z = F.labels_fixture()
    pts, clouds = z['scene_pts'], z['clouds']
    claims = np.zeros(len(pts), np.int64)
    for c in clouds:
        idx, best, second = NC.brute(pts, c)
        assert _gap_ok(best, second) or len(pts) < 2                       # no match is decided by a tie
        claims[np.unique(idx)] += 1
    assert (claims == 0).sum() >= 500                                       # scene points in no cloud
    assert (claims >= 2).sum() >= 1                                         # a scene point claimed by two clouds
    assert min(len(c) for c in clouds) == 1                                 # a cloud of one point
    assert len(np.unique(z['instances'])) < len(clouds)                     # an id that disappears in the remap
    assert 'stairs_1' in z['names'] and z['class_ids'][z['names'].index('stairs_1')] == 12
    idx, best, second = NC.brute(pts[claims > 0], pts[claims == 0])
    assert _gap_ok(best, second)
    inst, sem, error = F.point_labels_numpy(pts, clouds, z['class_ids'])
    assert inst.dtype == z['instances'].dtype == np.float32 and inst.shape == z['instances'].shape == (len(pts), 1)
    assert np.array_equal(inst, z['instances']) and np.array_equal(sem, z['semantics'])
    assert abs(error - z['error']) <= 1e-12 * z['error'] and z['error'] > 0


def test_full_resolution_fixture_and_the_gather_restated():
    import _s3dis_full_rule as F
    import _s3dis_rule as R
    from box2mask_amd import eval_s3dis as S
    rooms, want = F.full_rooms()
    assert len(rooms) == 2
    counts = []
    for rm in rooms:
        full, n = rm['full_positions'], rm['n']
        assert len(full) == 4 * n and np.array_equal(full[::4], rm['positions'])          # the reference samples every fourth point
        # (two rooms of 44 000 x 11 000 are too much for brute force in a quick test: the two nearest sampled points come from the
        # k-d tree, which the cases above hold to brute force, and their distances are recomputed in the contract's order)
        two = cKDTree(rm['positions']).query(full, k=2)[1]
        s2d = two[:, 0]
        assert _gap_ok(_d2(rm['positions'], full, two[:, 0]), _d2(rm['positions'], full, two[:, 1]))
        assert np.array_equal(s2d, rm['sparse2dense']) and np.array_equal(s2d[::4], np.arange(n))
        assert (s2d != np.arange(4 * n) // 4).sum() > n                                     # not the trivial map
        for k in ('semantics', 'instances'):
            sampled = rm['full_pred'][k][::4]                                               # (sparse2dense[::4] is the identity)
            assert np.array_equal(sampled[s2d], rm['full_pred'][k])
        counts.append(R.counts_numpy(rm['full_pred'], rm['full_gt']))
        assert counts[-1]['n'] == 4 * n
    mprec, mrec, prec, rec = S.s3dis_eval_from_counts(counts)
    assert np.array_equal(prec, want[2], equal_nan=True) and np.array_equal(rec, want[3], equal_nan=True)
    assert mprec == want[0] and mrec == want[1]


# ---------------------------------------------------------------- compile-time properties of csrc/neighbors.hip
def test_the_kernels_compile_without_scratch():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), '..', 'tools'))
    import isa_check
    if not os.path.exists(isa_check.HIPCC):
        pytest.skip('hipcc not available')
    found = isa_check.kernels(isa_check.device_asm('neighbors.hip'))
    names = ('nn_box_kernel', 'nn_grid_kernel', 'nn_key_kernel', 'nn_gather_kernel', 'nn_start_kernel', 'nn_query_kernel')
    for n in names:
        k = [v for name, v in found.items() if n in name]
        assert len(k) == 1, n
        assert k[0].get('scratch', 0) == 0 and not k[0].get('vgpr_spill') and not k[0].get('sgpr_spill'), (n, k[0])
        assert k[0]['vgpr'] <= 64 and k[0]['occupancy'] == 8, (n, k[0])          # (eight waves per SIMD: the queries hide latency)
