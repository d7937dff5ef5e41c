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
