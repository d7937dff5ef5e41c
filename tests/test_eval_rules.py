"""The rules of tests/_cluster_rule.py and tests/_detbox_rule.py against what already pins them (sklearn, scipy, the goldens taken
from the reference), the reach predicates of the cases tests/test_gpu_cluster_edges.py and tests/test_gpu_detbox_edges.py put to
the device -- each computed from the input, with the kernels' constants copied as literals -- and the proof that the cases are
sharp: every deliberate variant of a rule fails at least one named case.  No GPU.  profiles/eval_rule.md holds the tables."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import _cluster_rule as C
import _detbox_rule as D
import _s3dis_rule as R

DET_GOLD = os.path.join(R.ROOT, 'tests', 'golden', 'eval_detection.npz')


# ------------------------------------------------------------------ DBSCAN
@pytest.fixture(scope='module')
def db_cases():
    cases = {**C.size_cases(), **C.edge_cases()}
    return {name: (x, eps, ms, C.rule_labels(x, eps, ms)) for name, (x, eps, ms) in cases.items()}


def test_tree_twin_equals_the_brute_force_rule_on_every_small_case(db_cases):
    for name, (x, eps, ms, (lab, core, _)) in db_cases.items():
        tl, tc, roots = C.dbscan_tree(x, eps, ms)
        assert np.array_equal(tl, lab) and np.array_equal(tc, core), name
        want_roots = [int(np.nonzero(core & (lab == c))[0].min()) for c in range(lab.max() + 1)]
        assert roots.tolist() == want_roots, name


def test_rule_equals_sklearn_where_the_margin_allows(db_cases):
    cluster = pytest.importorskip('sklearn.cluster')
    compared = []
    for name, (x, eps, ms, (lab, _, _)) in db_cases.items():
        if not np.isfinite(x).all() or not R.margin(x, eps) >= 1e-12:
            continue
        got = cluster.DBSCAN(eps=eps, min_samples=ms).fit(x).labels_
        assert np.array_equal(got, lab), name
        compared.append(name)
    assert len(compared) >= 25 and {'cells26', 'clamp', 'tiles', 'ms1', 'shared_border', 'n:2049', 'cols:5'} <= set(compared)
    assert not any(n.startswith('eq_eps') for n in compared)                # at the boundary the rule, not sklearn, decides


@pytest.mark.parametrize('case', [0, 1])
def test_tree_twin_equals_the_sklearn_goldens(case):
    z = np.load(R.GOLD)                                # (the brute-force rule against them: tests/test_eval_s3dis.py)
    x = z['db%d_x' % case].astype(np.float64)
    lab, core, _ = C.dbscan_tree(x, float(z['db%d_eps' % case]), int(z['db%d_min_samples' % case]))
    assert np.array_equal(lab, z['db%d_labels' % case].astype(np.int32))
    assert np.array_equal(core, np.unpackbits(z['db%d_core' % case], count=len(x)).astype(bool))


def _runs(x, eps):
    keys, order, cells = C.cell_order(x, eps)
    starts, ends = C.runs_of(keys[order])
    return starts, ends, order, cells


def test_dbscan_size_cases_reach_the_block_and_scan_edges(db_cases):
    assert C.SIZES == (1, 2, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049)
    seen_d = set()
    for n in C.SIZES:
        x, eps, ms, (lab, core, _) = db_cases['n:%d' % n]
        assert x.shape[0] == n
        seen_d.add(x.shape[1])
        starts, ends, order, _ = _runs(x, eps)
        assert not np.array_equal(order, np.arange(n)) or len(starts) == 1  # shuffled rows (one cell: the stable sort keeps them)
        if n >= 257:                                                       # a cell straddles a 256-row block edge
            assert any(s < 256 * m < e for s, e in zip(starts, ends) for m in range(1, n // 256 + 1)), n
        if n >= 513:                                                       # a cell of more than 512 rows over three blocks
            assert any(e - s > 512 and (e - 1) // 256 - s // 256 >= 2 for s, e in zip(starts, ends)), n
        if n >= 1025:                                                      # roots at rows 1023 and 1024: ranks carry over a scan block
            roots = C.dbscan_tree(x, eps, ms)[2]
            assert {1023, 1024} <= set(roots.tolist()) and (roots < 1023).any(), n
            assert -(-n // C.DB_SCAN_BLOCK) >= 2
    assert seen_d == {3, 4, 5, 6, 7, 8}


def test_dbscan_column_cases(db_cases):
    for d in range(3, 9):
        x, eps, ms, (lab, core, _) = db_cases['cols:%d' % d]
        assert x.shape[1] == d and lab.max() >= 1
        if d > 3:                                                          # pairs that only column d - 1 separates
            near3 = R.sq_dists(x[:, :3], x[:, :3]) <= eps * eps
            near_but_last = R.sq_dists(x[:, :d - 1], x[:, :d - 1]) <= eps * eps
            full = R.sq_dists(x, x) <= eps * eps
            assert (near3 & near_but_last & ~full).sum() >= 100
        x, eps, ms, _ = db_cases['eq_eps:%d' % d]
        d2 = R.sq_dists(x, x)
        eps2 = eps * eps
        assert (d2 == eps2).sum() == 6 and ((d2 > eps2) & (d2 <= eps2 * (1 + 2.0 ** -50))).sum() == 6
        assert (x[:, d - 1] != 0).any()                                    # the 4 of the 3-4-5 sits in the last column


def test_dbscan_cells26_case_has_a_pair_in_every_offset(db_cases):
    x, eps, ms, (lab, core, _) = db_cases['cells26']
    edge = eps * (1 + 2.0 ** -20)
    cells = np.floor((x - x.min(0)) / edge).astype(int)
    assert np.array_equal(cells, C.cell_order(x, eps)[2]) and (x.min(0) == 0).all()
    i, j = np.nonzero(R.sq_dists(x, x) <= eps * eps)
    offs = {tuple(o) for o in (cells[j] - cells[i])}
    assert set(C.OFFSETS26) <= offs
    for axis in range(3):
        at0 = cells[i, axis] == 0
        got = {tuple(o) for o in (cells[j] - cells[i])[at0]}
        assert {o for o in C.OFFSETS26 if o[axis] >= 0} <= got, axis
    assert (lab < 0).sum() == 1 and lab.max() + 1 == 26 + 3 * 17              # every pair its own cluster: a missed run makes noise


def test_dbscan_run_and_tile_cases(db_cases):
    for name, row in (('ninth_run:2', 1), ('ninth_run:5', 1)):
        x, eps, ms, (lab, core, _) = db_cases[name]
        nb = np.nonzero(R.sq_dists(x[row:row + 1], x)[0] <= eps * eps)[0]
        last = C.ninth_run_last(x, eps, row)
        assert len(nb) == ms and last in nb and core[row]                   # min_samples reached exactly by ...
        cells = C.cell_order(x, eps)[2]
        assert (cells == cells[last]).all(1).sum() == 1                     # ... the last row of the ninth run, alone in its cell
        assert (cells[last] == cells[row] + 1).all()
    x, eps, ms, _ = db_cases['tiles']
    starts, ends, order, _ = _runs(x, eps)
    big = int(np.argmax(ends - starts))
    assert ends[big] - starts[big] == 600
    walked, done, total = C.pass1_trace(x, eps, ms)
    rows = order[starts[big]:ends[big]]
    assert (done[rows] == 0).sum() >= 256 and (done[rows] == total[rows] - 1).sum() >= 1    # the first tile / the last of the ninth run
    assert len(set(done[rows].tolist())) >= 3 and walked[rows].max() == total[rows].max() == 5


def test_dbscan_clamp_nonfinite_and_degenerate_cases(db_cases):
    x, eps, ms, (lab, core, two) = db_cases['clamp']
    assert eps == 2.0 ** -10 and (x[:, 0].max() - x[:, 0].min()) / eps > 2 ** 21
    cells = C.cell_order(x, eps)[2]
    clamped = cells[:, 0] == C.DB_CELL_MAX
    free = np.floor(x[:, 0] / (eps * (1 + 2.0 ** -20)))
    assert clamped.sum() == 31 and len(set(free[clamped].tolist())) >= 4      # cells that differ before the clamp
    assert len(set(lab[clamped].tolist())) == 3 and lab.max() == 3 and (~clamped & (lab >= 0)).sum() == 10
    mid = np.nonzero(two)[0]
    assert len(mid) == 1 and clamped[mid[0]] and not core[mid[0]] and lab[mid[0]] == 0
    for ms in (1, 3):
        x, eps, _, (lab, core, _) = db_cases['nonfinite:%d' % ms]
        bad = ~np.isfinite(x).all(1)
        assert len(x) <= 303 and bad.sum() == 3 and np.isnan(x).any() and (x == np.inf).any() and (x == -np.inf).any()
        assert (lab[bad] == -1).all() and not core[bad].any()
        assert ms > 1 or core[~bad].all()                                   # min_samples 1: every finite row is core
    x, eps, ms, (lab, core, _) = db_cases['ms1']
    assert ms == 1 and core.all() and lab.max() + 1 < len(x)
    x, eps, ms, (lab, core, _) = db_cases['zero_core']
    assert not core.any() and (lab == -1).all()
    x, eps, ms, (lab, core, _) = db_cases['identical']
    assert len(np.unique(x, axis=0)) == 1 and len(x) > 2 * C.DB_THREADS and (lab == 0).all()
    x, eps, ms = C.lattice_case()
    assert len(x) == 262145 and -(-len(x) // C.DB_SCAN_BLOCK) == 257 and ms == 1       # 257 block sums: two for thread 0
    assert len(np.unique(x, axis=0)) == len(x) and set(np.unique(np.diff(np.unique(x[:, 0])))) == {2 * eps}


DB_SHARP = {'lt': 'eq_eps', 'noself': 'ms1', 'border_high': 'shared_border', 'number_by_largest': 'cols:3', 'drop_last': 'cols:8'}


def test_every_dbscan_mistake_fails_a_case(db_cases):
    small = [n for n, v in db_cases.items() if len(v[0]) <= 320]
    table = {}
    for v in C.DBSCAN_VARIANTS:
        names = small + [n for n in db_cases if n.startswith(DB_SHARP[v]) and n not in small]
        table[v] = [n for n in names if not np.array_equal(C.dbscan_variant(*db_cases[n][:3], v), db_cases[n][3][0])]
        assert any(n.startswith(DB_SHARP[v]) for n in table[v]), (v, table[v])
    assert set(table['lt']) == {'eq_eps:%d' % d for d in range(3, 9)}       # nothing else sits on the boundary
    assert {'clamp', 'shared_border'} <= set(table['border_high'])
    print('dbscan mistakes:', table)


# ------------------------------------------------------------------ paint, joint histogram
def test_paint_rule_reproduces_the_rooms_of_the_reference():
    z = np.load(R.GOLD)
    for r in range(3):
        rm = R.room(z, r)
        accepted, inst, sem, _ = C.paint_rule(rm['masks'], rm['proposal_semantics'], 3, 0.6, 200, rm['pred_semantics'])
        bg = rm['background'].copy()                                        # evaluation.py:197-210
        bg[bg > 0] += inst.max()
        inst = np.where(bg > 0, bg, inst)
        for c in range(13):
            m = sem == c
            ids, cnt = np.unique(inst[m], return_counts=True)
            inst[m] = np.where(np.isin(inst[m], ids[cnt < 200]), -1, inst[m])
        assert np.array_equal(inst, rm['final']['instances']) and np.array_equal(sem, rm['final']['semantics'])
        assert 0 < accepted.sum() < len(accepted)


def test_paint_cases_reach_their_branches():
    assert C.PAINT_SIZES == (1, 63, 64, 65, 65535, 65536, 65537, 131073)
    strides = [-(-(-(-n // 64)) // C.PAINT_THREADS) for n in C.PAINT_SIZES]
    assert strides == [1, 1, 1, 1, 1, 1, 2, 3] and [-(-n // 64) for n in C.PAINT_SIZES[4:]] == [1024, 1024, 1025, 2049]
    for n in C.PAINT_SIZES:
        acc = C.paint_run_rule(C.paint_size_case(n))[0]
        assert n < 63 or 0 < acc.sum() < len(acc), n
    e = C.paint_edge_cases()
    assert np.float64(3.0) / np.float64(5.0) == e['ratio_eq']['ratio']      # sf / so == ratio exactly, in fp64
    assert C.paint_run_rule(e['ratio_eq'])[0].tolist() == [1, 1] and C.paint_run_rule(e['ratio_below'])[0].tolist() == [1, 0]
    assert C.paint_run_rule(e['min_points_eq'])[0].tolist() == [1, 0, 1]    # 200 accepted, 199 rejected
    assert C.paint_run_rule(e['empty_row:0'])[0].tolist() == [1, 1, 1]      # 0 / 0 passes the ratio test, 0 >= 0 the other
    assert C.paint_run_rule(e['empty_row:200'])[0].tolist() == [0, 0, 0]
    assert C.paint_run_rule(e['sem_edge'])[0].tolist() == [0, 1, 1, 1] and C.paint_run_rule(e['sem_edge:7'])[0].tolist() == [0, 0, 0, 1]
    assert C.paint_run_rule(e['chain'])[0].tolist() == [1, 0, 1, 0]
    assert e['k0']['masks'].shape[0] == 0 and e['no_sem_out']['sem_in'] is None


def test_every_paint_mistake_fails_a_case():
    cases = {**C.paint_edge_cases(), **{'n:%d' % n: C.paint_size_case(n) for n in C.PAINT_SIZES[:5]}}
    table = {}
    for v in C.PAINT_VARIANTS:
        table[v] = []
        for name, c in cases.items():
            a, b = C.paint_run_rule(c), C.paint_run_rule(c, v)
            if not all(np.array_equal(p, q) for p, q in zip(a, b) if p is not None):
                table[v].append(name)
    assert 'ratio_eq' in table['le'] and 'ratio_below' in table['ratio_all'] and 'chain' in table['dense_ids']
    assert {'sem_edge', 'sem_edge:7'} <= set(table['sem_min_off'])
    print('paint mistakes:', table)


def test_joint_hist_cases():
    cases = C.joint_hist_cases()
    cells = sorted({na * nb for _, _, na, nb in cases.values()})
    assert {1, 4095, 4096, 4097} <= set(cells) and C.JH_LDS == 4096
    I = np.iinfo(np.int32)
    for name, (a, b, na, nb) in cases.items():
        h = C.joint_hist_rule(a, b, na, nb)
        ok = (a >= 0) & (a < na) & ((b is None) | ((0 if b is None else b) >= 0) & ((0 if b is None else b) < nb))
        assert h.sum() == ok.sum(), name
        if name.startswith('cells'):
            assert {-1, na, I.min, I.max} <= set(a.tolist()) and {-1, nb, I.min, I.max} <= set(b.tolist())
            assert 0 < h.sum() < len(a)
    assert C.joint_hist_rule(*cases['one_cell']).max() == 70000
    assert C.JH_GRID * 16 + 1 == 2048 * 256 * 16 + 1 == 8388609


# ------------------------------------------------------------------ hulls
@pytest.fixture(scope='module')
def hull_cases():
    cases = D.hull_cases()
    return {name: (c, D.hulls_rule(c['masks'], c['pos'], c['cap'])) for name, c in cases.items()}


def _scene(z, s):
    n = int(z['s%d_n' % s])
    mask = np.unpackbits(z['s%d_mask' % s], axis=1)[:, :n].astype(bool)
    return mask, z['s%d_pos' % s].astype(np.float64)


def test_hull_rule_equals_the_golden_hulls_of_qhull():
    z = np.load(DET_GOLD)
    rows = 0
    for s in range(int(z['n_scenes'])):
        mask, pos = _scene(z, s)
        out = D.hulls_rule(mask, pos, 4096)
        assert np.array_equal(out['count'], z['s%d_count' % s])
        off = z['s%d_hull_off' % s]
        for r in np.nonzero(out['count'] >= 50)[0]:
            assert np.array_equal(out['box6'][r], z['s%d_box6' % s][r])
            ref = z['s%d_hull' % s][off[r]:off[r + 1]]
            assert {tuple(q) for q in out['hulls'][r]} == {tuple(q) for q in ref}     # the same vertices, bit for bit
            assert abs(D.np_area(out['hulls'][r]) - D.np_area(ref)) <= 1e-12 * D.np_area(ref)
            rows += 1
    assert rows >= 16


def test_hull_rule_equals_scipy_on_the_non_degenerate_cases(hull_cases):
    spatial = pytest.importorskip('scipy.spatial')
    compared = 0
    for name in ('sparse', 'words:1024', 'words:1025', 'tie_chunks', 'offset1e6', 'cap64:64', 'cand:2048', 'parabola:512'):
        c, rule = hull_cases[name]
        for r in range(len(c['masks'])):
            h = rule['hulls'][r]
            if h is None or len(h) < 3:
                continue
            p = np.unique(c['pos'][c['masks'][r], :2], axis=0)
            q = spatial.ConvexHull(p)
            if name != 'offset1e6':                   # (qhull's own area loses 1e-11 at coordinates of 1e6: vertices only there)
                assert abs(q.volume - D.np_area(h)) <= 1e-12 * q.volume, name
            assert {tuple(v) for v in p[q.vertices]} == {tuple(v) for v in h}, name
            e1, e2 = np.roll(h, -1, 0) - h, np.roll(h, -2, 0) - np.roll(h, -1, 0)
            assert (e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0] > 0).all() and tuple(h[0]) == min(map(tuple, h))
            compared += 1
    assert compared >= 10


def test_hull_cases_reach_their_branches(hull_cases):
    names = list(D.SMALL_ROWS)
    for tag, mod in (('small:1', 1), ('small:63', 63)):
        c, rule = hull_cases[tag]
        assert c['pos'].shape[0] % 64 == mod and c['pad']
        want = {'empty': 0, 'one': 1, 'two': 2, 'duplicates': 1, 'horizontal': 2, 'vertical': 2, 'ccw3': 3, 'cw3': 3, 'dup_vertices': 4,
                'edge_points': 4}
        for k, v in want.items():
            assert rule['n_hull'][names.index(k)] == v, k
        assert rule['n_hull'][names.index('slope')] >= 2                    # non-dyadic slope: the fp64 turn decides
        assert np.isinf(rule['box6'][0]).all() and rule['box6'][0, 0] > 0 > rule['box6'][0, 3]
        assert np.array_equal(rule['hulls'][names.index('ccw3')], rule['hulls'][names.index('cw3')])
    c, _ = hull_cases['sparse']
    w = C.pack_rows(c['masks'][:1])[0]
    assert (w != 0).sum() == 2 and len(w) == 300
    assert D.chunking(1024) == (1024, 1) and D.chunking(1025) == (1024, 2)
    assert hull_cases['words:1024'][0]['pos'].shape[0] == 1024 * 64 and hull_cases['words:1025'][0]['pos'].shape[0] == 1024 * 64 + 1
    words = -(-D.BIG_N // 64)
    assert words > 32 * 1024 and D.chunking(words) == (1088, 31) and D.BIG_N % 64 == 1
    c, rule = hull_cases['tie_chunks']
    p = c['pos'][c['masks'][0], :2]
    idx = np.nonzero(c['masks'][0])[0]
    for corner in ([0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]):
        at = idx[(p == corner).all(1)]
        assert len(at) == 2 and at[0] // 64 < 1024 <= at[1] // 64            # the same extreme in chunk 0 and in chunk 1
    assert rule['n_hull'][0] == 4
    for name, ncand, in_lds, flag, nh in (('cand:2048', 2048, True, 0, 4), ('cand:2049', 2049, False, 0, 4),
                                          ('cap64:64', 64, True, 0, 4), ('cap64:65', 65, True, D.FLAG_CANDIDATES, 0)):
        c, rule = hull_cases[name]
        m = 1 << int(ncand - 1).bit_length()
        assert rule['ncand'][0] == ncand and (m <= D.LCAP) == in_lds and rule['flags'][0] == flag and rule['n_hull'][0] == nh, name
        assert c['cap'] == (64 if name.startswith('cap64') else 4096)
    assert hull_cases['parabola:512'][1]['n_hull'][0] == 512 == D.HULL_MAX and hull_cases['parabola:512'][1]['flags'][0] == 0
    assert hull_cases['parabola:513'][1]['n_hull'][0] == 513 and hull_cases['parabola:513'][1]['flags'][0] == D.FLAG_VERTICES
    c, rule = hull_cases['circle']
    rad = np.hypot(c['pos'][:, 0], c['pos'][:, 1])
    assert len(rad) == 10400 and ((rad < 1 - 5e-17) & (rad > 1 - 2e-13)).sum() >= 9000
    assert rule['ncand'][0] <= c['cap'] and rule['flags'][0] == D.FLAG_VERTICES and rule['n_hull'][0] > 5000
    c, rule = hull_cases['near_edges']
    assert 100 < rule['n_hull'][0] <= D.HULL_MAX < rule['ncand'][0] <= c['cap']   # candidates the chain itself has to reject
    assert (hull_cases['offset1e6'][0]['pos'][:, :2] > 9e5).all()


def test_every_hull_mistake_fails_a_case():
    table = {}
    for v in D.HULL_VARIANTS:
        table[v] = [k for k, p in D.SMALL_ROWS.items() if not np.array_equal(D.np_hull(p, v), D.np_hull(p))]
    assert {'horizontal', 'vertical', 'edge_points'} <= set(table['lt'])
    assert 'duplicates' in table['nodedup']
    assert {'ccw3', 'cw3', 'edge_points'} <= set(table['cw'])
    print('hull mistakes:', table)


# ------------------------------------------------------------------ corners, axis-aligned IoU
def _same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _gt(z, s):
    c = z['s%d_per_instance_bb_centers' % s].astype(np.float64)
    b = z['s%d_per_instance_bb_bounds' % s].astype(np.float64)
    q = z['s%d_per_instance_bb_rotations' % s].astype(np.float64).reshape(-1, 9)
    return c, D.corners_rule(c, b, q), z['s%d_per_instance_semantics' % s].astype(np.int32)[:len(c)]


def test_aabb_rule_equals_the_golden_table_bit_for_bit():
    z = np.load(DET_GOLD)
    for s in range(int(z['n_scenes'])):
        keep = z['s%d_count' % s] >= 50
        pcls = np.where(keep, z['s%d_label_id' % s].astype(np.int32), -1)
        centers, boxes, gcls = _gt(z, s)
        # The golden sizes are get_rotated_bounds as the reference evaluates it: numpy's `rotation @ corner`, whose 3-term sums do
        # not round as the written q[a]*p0 + q[3+a]*p1 + q[6+a]*p2 does.  calc_iou itself is pinned with the reference's sizes ...
        ref_boxes = boxes.copy()
        for i in range(len(centers)):
            rot = np.reshape(z['s%d_per_instance_bb_rotations' % s][i], [3, 3]).T
            b = z['s%d_per_instance_bb_bounds' % s][i]
            m = np.zeros(3)
            for v in range(8):
                m = np.maximum(m, rot @ np.array([D.SX[v] * b[0], D.SY[v] * b[1], D.SZ[v] * b[2]]))
            ref_boxes[i, 11:14] = m * 2.0
        got = D.aabb_rule(z['s%d_box6' % s], pcls, centers, ref_boxes, gcls)
        assert _same_bits(got[keep], z['s%d_iou_aabb' % s][keep]) and (got[keep] > 0).sum() >= 5
        # ... and the sizes in the kernel's written order stay within 2 ulp of them, the table within 4 ulp of the golden one
        assert (np.abs(ref_boxes[:, 11:14] - boxes[:, 11:14]) <= 2 * 2.0 ** -52 * boxes[:, 11:14]).all()
        assert np.abs(D.aabb_rule(z['s%d_box6' % s], pcls, centers, boxes, gcls)[keep] - z['s%d_iou_aabb' % s][keep]).max() <= 2.0 ** -50


def test_corner_and_aabb_cases():
    rots = D.rotations()
    assert abs(np.linalg.det(rots['reflection']) + 1) < 1e-12 and abs(np.linalg.det(rots['generic']) - 1) < 1e-12
    for g in (1, 63, 64, 65):
        c, b, q = D.corners_case(g)
        rec = D.corners_rule(c, b, q)
        signs = np.stack([D.SX, D.SY, D.SZ], 1)
        for i in range(g):
            corners = (signs * b[i]) @ q[i].reshape(3, 3) + c[i]            # (R = reshape(3, 3).T; x @ R.T)
            assert np.abs(rec[i, :8].reshape(4, 2) - corners[:4, :2]).max() <= 1e-14
            assert abs(rec[i, 10] - 8 * b[i].prod()) <= 1e-12
    box6, pcls, gc, boxes, gcls = D.aabb_edge_case()
    iou = D.aabb_rule(box6, pcls, gc, boxes, gcls)
    assert iou[0, 0] == 0 and iou[0, 5] == 0                                # touching faces
    assert iou[0, 1] == 1.0                                                 # identical
    assert iou[2, 1] == 0.125 and iou[0, 2] == 0.125                        # contained, either way
    assert (iou[:, 4] == 0).all() and (iou[4] == 0).all()                   # class mismatch, pcls -1
    assert 0 < iou[3, 3] < 1
    assert iou[5, 6] == 0                                                   # a point on a zero-size box: touching, not overlapping
    ge = D.aabb_rule(box6, pcls, gc, boxes, gcls, 'ge')                    # `>=` for `>`: touching faces still give 0 (a zero factor)
    assert _same_bits(ge[:5], iou[:5]) and np.isnan(ge[5, 6])              # ... only the 0 / 0 of the degenerate pair tells


# ------------------------------------------------------------------ hull x box IoU
@pytest.fixture(scope='module')
def iou_forms():
    return [(case, D.iou_case_forms(case)) for case in D.iou_cases()]


def test_iou_form_a_equals_the_golden_table_of_box3d_iou():
    z = np.load(DET_GOLD)
    worst = ratio = 0.0
    pairs = 0
    for s in range(int(z['n_scenes'])):
        mask, pos = _scene(z, s)
        hulls = D.hulls_rule(mask, pos, 4096)
        keep = hulls['count'] >= 50
        label = z['s%d_label_id' % s]
        _, boxes, gcls = _gt(z, s)
        ref = z['s%d_iou_obb' % s]
        for r in np.nonzero(keep)[0]:
            for b in range(len(boxes)):
                if label[r] != gcls[b]:
                    assert ref[r, b] == 0
                    continue
                f = D.iou_forms(hulls['hulls'][r], hulls['box6'][r, 2], hulls['box6'][r, 5], boxes[b, :8].reshape(4, 2), boxes[b, 8],
                                boxes[b, 9], boxes[b, 10])
                assert (f['iou_a'] > 0) == (ref[r, b] > 0)
                worst = max(worst, abs(f['iou_a'] - ref[r, b]))
                assert abs(f['iou_a'] - float(f['iou_exact'])) <= f['bound'] <= D.IOU_TOL
                if f['bound']:
                    ratio = max(ratio, abs(f['iou_a'] - float(f['iou_exact'])) / f['bound'])
                pairs += int(ref[r, b] > 0)
    print('form (a) vs box3d_iou over %d overlapping pairs: max abs difference %.3g; error / bound at most %.3g' % (pairs, worst, ratio))
    assert pairs >= 50 and worst <= D.IOU_TOL


def test_every_iou_case_is_valid_and_form_a_lies_inside_the_bound(iou_forms):
    ratio = 0.0
    for case, f in iou_forms:
        assert D.case_is_valid(f), case[0]
        assert f['max_n'] <= D.PCAP
        err = abs(Fraction(f['iou_a']) - f['iou_exact'])
        assert err <= Fraction(f['bound']), case[0]
        if f['exact']:
            assert f['iou_a'] == float(f['iou_exact']), case[0]              # every step exact: the final division rounds once
        if f['bound']:
            ratio = max(ratio, float(err) / f['bound'])
    print('form (a): largest error / bound %.3g over %d cases' % (ratio, len(iou_forms)))


def test_iou_cases_reach_their_branches(iou_forms):
    by = {case[0]: (case, f) for case, f in iou_forms}
    sizes = {len(case[2]) for case, _ in iou_forms}
    assert set(D.IOU_SIZES) | {0, 1, 2} <= sizes and D.IOU_SIZES == (3, 4, 63, 64, 65, 127, 128, 129, 512)
    for fam in ('par', 'cir'):
        for n in D.IOU_SIZES:
            get = lambda kind: by['%s%d:%s' % (fam, n, kind)]
            case, f = get('contain')
            assert f['crossings'] == 0 and f['inter_exact'] == f['area1_exact'] > 0
            case, f = get('contained')
            rect = [tuple(map(Fraction, map(float, c))) for c in case[5]]
            area = abs(sum(rect[i - 1][0] * rect[i][1] - rect[i][0] * rect[i - 1][1] for i in range(4))) / 2
            assert f['inter_exact'] == area and f['crossings'] == 8
            case, f = get('cut')
            assert 0 < f['inter_exact'] < f['area1_exact'] and f['crossings'] >= 2
            assert get('miss_first')[1]['emptied_at'] == 0 and get('miss_last')[1]['emptied_at'] == 3
            assert get('clockwise')[1]['iou_exact'] == 0 and get('clockwise')[1]['emptied_at'] is not None
            if fam == 'par':
                case, f = get('line_outside')
                assert f['iou_exact'] == 0 and f['exact']
                c1, c2 = case[5][0], case[5][1]                              # hull vertices 0 and n - 1 exactly ON a clip line
                on = [(c2[0] - c1[0]) * (p[1] - c1[1]) == (c2[1] - c1[1]) * (p[0] - c1[0]) for p in case[2]]
                assert on[0] and on[-1]
                if n != 512:
                    assert get('line_inside')[1]['iou_exact'] > 0
    exact = {name for name, (_, f) in by.items() if f['exact']}
    assert {'par%d:%s' % (n, k) for n in D.IOU_SIZES for k in ('contain', 'cut', 'line_outside')} <= exact
    assert {'sq:cut', 'sq:identical', 'sq:touch', 'sq:flat', 'sq:z_disjoint', 'sq:z_touch'} <= exact
    assert by['sq:cut'][1]['iou_exact'] == Fraction(1, 9) and by['sq:identical'][1]['iou_exact'] == 1
    assert by['sq:touch'][1]['iou_exact'] == 0 and by['sq:touch'][1]['emptied_at'] == 0      # strict inside: a shared edge line
    assert by['sq:flat'][0][3] == by['sq:flat'][0][4] and by['sq:flat'][1]['inter_exact'] > 0 and by['sq:flat'][1]['iou_exact'] == 0
    assert by['sq:z_disjoint'][1]['iou_exact'] == 0 and by['sq:z_disjoint'][1]['inter_exact'] > 0
    assert any(f['emptied_at'] in (1, 2) for _, f in iou_forms)              # an empty intermediate clip
    assert sum(not f['exact'] and f['iou_exact'] > 0 for _, f in iou_forms) >= 30


def test_the_chain_case_is_valid():
    pos, masks, plabel, centers, bounds, rot, glabel = D.pipeline_case()
    hulls = D.hulls_rule(masks, pos, 4096)
    rec = D.corners_rule(centers, bounds, rot)
    assert hulls['n_hull'].tolist() == [3, 65, 129] and (hulls['flags'] == 0).all()
    forms = [D.iou_forms(hulls['hulls'][r], hulls['box6'][r, 2], hulls['box6'][r, 5], rec[b, :8].reshape(4, 2), rec[b, 8], rec[b, 9], rec[b, 10])
             for r in range(3) for b in range(4)]
    assert all(D.case_is_valid(f) for f in forms) and sum(f['iou_exact'] > 0 for f in forms) == 6
    assert all(f['iou_exact'] == 0 for f in forms[2::4])                     # the box turned about all three axes runs clockwise in x-y


def test_every_clip_mistake_fails_a_case(iou_forms):
    table = {v: [] for v in D.CLIP_VARIANTS}
    for case, f in iou_forms:
        if len(case[2]) > 65:
            continue
        for v in D.CLIP_VARIANTS:
            g = D.iou_case_forms(case, v)
            if abs(g['iou_a'] - f['iou_a']) > 1e-6 or (g['iou_a'] > 0) != (f['iou_a'] > 0) or math.isnan(g['iou_a']):
                table[v].append(case[0])
            elif v == 'ge' and g['emptied_at'] != f['emptied_at']:
                table[v].append(case[0] + ' (polygon only)')
    # `>=` keeps boundary points, which carry no area: no IoU value can tell it from `>`.  It shows in what polygon_clip returns
    # (a degenerate polygon instead of None, which the reference would hand to qhull), so that is what the case is held to here.
    assert table['ge'] and all(n.endswith('(polygon only)') for n in table['ge']) and 'sq:touch (polygon only)' in table['ge']
    assert 'sq:cut' in table['vertex_first'] and 'par3:clockwise' in table['abs_orient']
    print('clip mistakes:', table)
