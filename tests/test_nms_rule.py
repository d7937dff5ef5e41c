"""The restatement of box-vote clustering, projection, mask NMS, the histograms and the gathers (tests/_nms_rule.py): tied to the
oracle and to the real reference's goldens, tied to properties that need no implementation, and shown to be SHARP -- every
deliberate mistake, written as a variant of the rule, fails at least one case of the lists tests/test_gpu_nms_edges.py runs on
the device.  Every reach predicate of every case is asserted here."""
import os

import numpy as np
import pytest

import _nms_rule as R
from oracle import nms_ref

F = np.float32


def _nmc_cases():
    return ([R.nmc_size_case(n) for n in R.NMC_SIZES] + [R.window_case(c[0]) for c in R.WINDOW_CASES] +
            [R.nmc_edge_case(n) for n in R.NMC_EDGE_CASES] + [R.maxk_case(n) for n in R.MAXK_CASES])


def _same_nmc(a, b):
    return (a['k'] == b['k'] and np.array_equal(a['reps'], b['reps']) and np.array_equal(a['assign'], b['assign']) and
            np.array_equal(a['order'], b['order']) and R.same_floats(a['heat'], b['heat']))


# ----------------------------------------------------------------------------- the rule against the oracle and the goldens
@pytest.mark.parametrize('seed,n,nobj', [(0, 400, 12), (1, 1500, 30), (2, 77, 5)])
def test_rule_matches_the_oracle_on_random_votes_and_masks(seed, n, nobj):
    from box2mask_amd import synth
    boxes = synth.make_votes(seed, n_obj=nobj, n_seg=n)
    want = R.nmc(boxes, 0.5, n)
    reps, clusters, heat = nms_ref.nms_clustering(boxes, 0.5)
    assert want['k'] == len(reps) and np.array_equal(want['reps'], reps)
    assert R.same_floats(want['heat'][:want['k']], heat)
    for c, idx in enumerate(clusters):
        assert np.array_equal(np.sort(idx), np.flatnonzero(want['assign'] == c))
        assert np.array_equal(idx, want['order'][want['assign'][want['order']] == c])          # members in visiting order
    assert np.array_equal(want['order'], np.argsort(-boxes[:, 0], kind='stable'))
    masks = heat > F(0.3)
    bits = R.pack(masks)
    inter, keep, nk = R.mask_nms(bits, 0.6)
    assert np.array_equal(np.flatnonzero(keep), nms_ref.mask_nms(masks, 0.6)[0]) and nk == keep.sum()
    assert np.array_equal(inter, (masks[:, None] & masks[None]).sum(2))
    assert np.array_equal(R.unpack(bits, masks.shape[1]), masks)


@pytest.mark.parametrize('case', ['votes1', 'votes64', 'votes512', 'votes2000', 'degenerate', 'edge_th'])
def test_rule_matches_the_goldens_of_the_reference(golden_dir, case):
    g = np.load(os.path.join(golden_dir, 'iou_nms.npz'))
    boxes = g[case + '_boxes']
    want = R.nmc(boxes, float(g[case + '_th']), len(boxes))
    assert np.array_equal(want['reps'], g[case + '_reps'])
    assert R.same_floats(want['heat'][:want['k']], g[case + '_heat'])
    assert np.array_equal(want['assign'], g[case + '_assign'])
    _, keep, _ = R.mask_nms(R.pack(g[case + '_masks']), 0.6)
    assert np.array_equal(np.flatnonzero(keep), g[case + '_mask_kept'])


def test_set_ious_cases_are_inside_the_oracles_domain():
    for n in R.SET_N:
        c = R.set_ious_case(n)
        assert all(c.reach.values()), (c, c.reach)
        out = R.set_ious(c.a, c.b)
        assert out.shape == (n,) and out.dtype == F and not np.isnan(out).any()
        for i in range(min(n, 5)):
            assert out[i].view(np.uint32) == R.box_ious(c.a[i], c.b[i:i + 1])[0].view(np.uint32)


# ----------------------------------------------------------------------------- properties that need no implementation
def test_every_box_is_assigned_once_and_reps_are_first_visited():
    for c in _nmc_cases():
        w = R.nmc(c.boxes, c.th, c.max_k, c.heat_rows)
        n, k = len(c.boxes), w['k']
        assert ((w['assign'] >= 0) & (w['assign'] < k)).all(), c
        assert np.array_equal(np.sort(w['order']), np.arange(n)), c
        sc = c.boxes[w['order'], 0]
        assert (sc[1:] <= sc[:-1]).all(), c
        first = {}
        for row in w['order'].tolist():
            first.setdefault(int(w['assign'][row]), row)
        assert [first[q] for q in range(k)] == w['reps'].tolist(), c
        rows = min(k, c.max_k)
        assert (w['heat'][rows:].view(np.uint32) == R.SENT_F.view(np.uint32)).all(), c
        assert all(w['heat'][r, w['reps'][r]] == 1 for r in range(rows)), c


def test_project_then_identity_gather_is_the_thresholded_heat():
    for n_vox in R.PROJ_NVOX:
        for ksel in R.PROJ_KSEL:
            c = R.project_case(n_vox, ksel)
            bits = R.project(c.heat, c.sel, c.fg_slot, c.seg2vox, c.th)
            assert bits.shape == (ksel, c.words)
            assert not R.unpack(bits)[:, n_vox:].any()                                # pad bits zero
            want = np.zeros((ksel, n_vox), np.uint8)
            for r in range(ksel):
                for v in range(n_vox):
                    s = c.fg_slot[c.seg2vox[v]]
                    want[r, v] = s >= 0 and c.heat[c.sel[r], s] > c.th
            assert np.array_equal(R.gather(bits, None, None, n_vox), want), c


def test_mask_hist_over_classes_is_the_popcount_over_valid_labels():
    for words in R.MH_WORDS[:4]:
        for n_class in R.MH_NCLASS:
            c = R.mask_hist_case(words, n_class, 3)
            h = R.mask_hist(c.bits, c.label, c.n, c.n_class)
            valid = (c.label >= 0) & (c.label < c.n_class)
            assert np.array_equal(h.sum(1), (R.unpack(c.bits, c.n) & valid[None]).sum(1)), c
    for words in R.LH_WORDS:
        for n_class in R.LH_NCLASS:
            c = R.label_hist_case(words, n_class, True)
            h = R.mask_hist(c.bits, c.sem, c.n_vox, n_class)
            lab = R.label_hist(c.bits, c.rows, c.sem, c.n_vox, n_class)
            assert np.array_equal(lab, h[c.rows].argmax(1)) and (h[c.rows].max(1) == h[c.rows, lab]).all()


def test_gather_is_the_bit_of_the_row():
    c = R.gather_batch_case(65)
    for sc in c.scenes:
        out = R.gather(sc['bits'], sc['rows'], sc['index'], sc['n_pts'])
        assert out.shape == (sc['kk'], sc['n_pts'])
        m = R.unpack(sc['bits'])
        for r in range(0, sc['kk'], 17):
            row = r if sc['rows'] is None else sc['rows'][r]
            for p in range(0, sc['n_pts'], 53):
                assert out[r, p] == m[row, p if sc['index'] is None else sc['index'][p]]


def test_mask_desc_follows_the_field_order_of_the_header():
    text = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'b2m.h')).read()
    assert '#define B2M_MASK_DESC %d' % len(R.MASK_FIELDS) in text
    for f, name in ((0, 'heat'), (3, 'ksel'), (7, 'bits'), (8, 'words'), (10, 'keep'), (12, 'kk'), (14, 'labels'), (16, 'n_pts'), (17, 'out')):
        assert R.MASK_FIELDS[f] == name and ' %d %s' % (f, name) in text
    scenes = [dict(ksel=3, kk=2, n_vox=70, words=2), dict(ksel=0, kk=0), dict(ksel=5, kk=5, n_pts=9)]
    d = R.mask_desc(scenes, lambda s, name: 1000 * (s + 1) + R.MASK_FIELDS.index(name))
    assert d.shape == (3, 20) and d[:, 18].tolist() == [0, 3, 3] and d[:, 19].tolist() == [0, 2, 2]
    assert d[0, 6] == 70 and d[0, 8] == 2 and d[2, 16] == 9 and d[1, 7] == 2007 and d[2, 0] == 3000


# ----------------------------------------------------------------------------- every reach predicate, for every case
def test_every_case_reaches_its_branch():
    cases = _nmc_cases() + [R.ceiling_case(), R.nmc_batch_case(), R.mask_nms_batch_case()]
    cases += [R.project_case(v, k) for v in R.PROJ_NVOX for k in R.PROJ_KSEL]
    cases += [R.mask_nms_case(k, w) for k in R.MNMS_K for w in R.MNMS_WORDS] + [R.mask_nms_edge_case(n) for n in R.MNMS_EDGE_CASES]
    cases += [R.label_hist_case(w, c, s) for w in R.LH_WORDS for c in R.LH_NCLASS for s in (False, True)]
    cases += [R.label_hist_batch_case(c) for c in R.LH_NCLASS]
    cases += [R.mask_hist_case(w, c, k) for w in R.MH_WORDS for c in R.MH_NCLASS for k in R.MH_K]
    cases += [R.gather_batch_case(kk) for kk in R.GATHER_KK] + [R.pack_case(n) for n in R.PACK_N] + [R.set_ious_case(n) for n in R.SET_N]
    for c in cases:
        assert c.reach and all(bool(v) for v in c.reach.values()), (c.name, c.reach)
    # the clustering sizes sit on both sides of every constant
    sizes = {n: R.nmc_size_case(n) for n in R.NMC_SIZES}
    assert {c.sort for c in sizes.values()} == {'lds', 'global'} and sizes[4096].sort == 'lds' and sizes[4097].sort == 'global'
    assert {0, 1, 31} <= {c.last_word_bits for c in sizes.values()}
    assert R.npow2(8193) == 16384
    # the window search skips 0, 1 and >= 2 whole windows, lands on a window's first and last slot, on both sort paths
    win = [R.window_case(c[0]) for c in R.WINDOW_CASES]
    later = [(s, slot, c.sort) for c in win for s, slot in zip(c.skips[1:], c.slots[1:])]
    assert {min(s, 2) for s, _, _ in later} == {0, 1, 2}
    assert any(s >= 1 and slot == 0 for s, slot, _ in later) and any(slot == R.NMC_THREADS - 1 for _, slot, _ in later)
    assert {srt for s, _, srt in later if s >= 1} == {'lds', 'global'}


# ----------------------------------------------------------------------------- the cases are sharp
def _failing(mistake):
    """Names of the listed cases on which the rule with `mistake` differs from the rule."""
    bad = []
    if mistake in ('lt_cluster', 'tie_high', 'zero_sign', 'no_force', 'no_eps', 'prod_order', 'no_clamp', 'one_window', 'heat_past_max_k'):
        for c in _nmc_cases():
            if not _same_nmc(R.nmc(c.boxes, c.th, c.max_k, c.heat_rows), R.nmc(c.boxes, c.th, c.max_k, c.heat_rows, mistake)):
                bad.append(c.name)
    if mistake in ('lt_mask', 'fp64_ratio'):
        for c in [R.mask_nms_edge_case(n) for n in R.MNMS_EDGE_CASES] + [R.mask_nms_case(k, w) for k in (2, 257) for w in (1, 257)]:
            if not np.array_equal(R.mask_nms(c.bits, c.th)[1], R.mask_nms(c.bits, c.th, mistake)[1]):
                bad.append(c.name)
    if mistake in ('last_max', 'pad_counted'):
        for c in [R.label_hist_case(w, n, s) for w in R.LH_WORDS for n in R.LH_NCLASS for s in (False, True)]:
            if not np.array_equal(R.label_hist(c.bits, c.rows, c.sem, c.n_vox, c.n_class),
                                  R.label_hist(c.bits, c.rows, c.sem, c.n_vox, c.n_class, mistake)):
                bad.append(c.name)
    if mistake == 'pad_counted':
        for c in [R.mask_hist_case(w, n, 1) for w in R.MH_WORDS[:3] for n in R.MH_NCLASS]:
            if not np.array_equal(R.mask_hist(c.bits, c.label, c.n, c.n_class), R.mask_hist(c.bits, c.label, c.n, c.n_class, mistake)):
                bad.append(c.name)
    if mistake == 'chunk_drop_64':
        for c in [R.project_case(v, k) for v in R.PROJ_NVOX for k in R.PROJ_KSEL]:
            if not np.array_equal(R.project(c.heat, c.sel, c.fg_slot, c.seg2vox, c.th),
                                  R.project(c.heat, c.sel, c.fg_slot, c.seg2vox, c.th, mistake)):
                bad.append(c.name)
    return bad


MUST_FAIL = {'lt_cluster': 'iou_eq_th', 'lt_mask': 'th_eq_ratio', 'tie_high': 'ties_shuffled', 'zero_sign': 'zeros:neg_first',
             'no_force': 'zero_volume_rep', 'no_eps': 'zero_volume_rep', 'prod_order': 'n:1025', 'no_clamp': 'n:33',
             'fp64_ratio': 'seven_tenths', 'last_max': 'lh:1:20:0', 'pad_counted': 'mh:1:1:1', 'one_window': 'win:1025',
             'heat_past_max_k': 'k_gt_max_k', 'chunk_drop_64': 'project:64:65'}


@pytest.mark.parametrize('mistake', R.MISTAKES)
def test_every_mistake_fails_a_listed_case(mistake):
    bad = _failing(mistake)
    print(mistake, len(bad), bad[:12])
    assert MUST_FAIL[mistake] in bad, (mistake, bad)


def test_mistakes_fail_where_they_should_and_nowhere_else():
    assert set(MUST_FAIL) == set(R.MISTAKES)
    assert set(_failing('zero_sign')) == {'zeros:neg_first', 'zeros:pos_first'}
    assert set(_failing('lt_cluster')) >= {'iou_eq_th'} and 'iou_above_th' not in _failing('lt_cluster')
    assert set(_failing('one_window')) == {'win:1025', 'win:2048', 'win:2048g', 'win:last', 'win:last_g', 'win:all'}
    assert set(_failing('heat_past_max_k')) == {'k_gt_max_k'}
    assert set(_failing('fp64_ratio')) >= {'seven_tenths', 'big_union'}
    drop = set(_failing('chunk_drop_64'))                       # (one voxel: row 64's only bit may be off anyway)
    assert {'project:%d:%d' % (v, k) for v in R.PROJ_NVOX[1:] for k in (65, 129)} <= drop
    assert drop <= {'project:%d:%d' % (v, k) for v in R.PROJ_NVOX for k in (65, 129)}
