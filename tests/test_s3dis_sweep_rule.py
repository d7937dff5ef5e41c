"""CPU: the rule of the S3DIS threshold sweep (tests/_s3dis_sweep_rule.py, profiles/s3dis_sweep_rule.md) against the 36 settings of
the real reference in tests/golden/s3dis_sweep.npz (tools/gen_golden_s3dis_sweep.py).

"Shared stage + prefix restriction + tail": per room and (cluster_th, mask_bin_th) the proposals of the smallest score_th are
merged ONCE; every score setting is that painting restricted to a prefix.  The labels (as partitions, as ids, and the semantics),
every true / false positive count, precision / recall with their NaNs and mPrec / mRec to the bit must be the reference's; the
fixture must keep reaching the edges the rule has; and each deliberate mistake of ``MISTAKES`` must fail the case named for it."""
import numpy as np
import pytest

import _s3dis_sweep_rule as R


@pytest.fixture(scope='module')
def fx():
    return R.load()


@pytest.fixture(scope='module')
def stages(fx):
    """{(room, ci, bi): (owner, prop_sem, fate)}: one merge per stage, from the masks of the smallest score_th."""
    out = {}
    for r, rm in enumerate(fx['rooms']):
        for (ci, bi), masks in rm['stage_masks'].items():
            out[(r, ci, bi)] = R.paint(masks, rm['sem'])
    return out


def _q(fx, ci, si, bi):
    return fx['settings'].index((ci, si, bi))


def _labels(fx, stages, r, ci, si, bi, mistake=None, index=None, stage=None):
    rm = fx['rooms'][r]
    owner, prop_sem, _ = stage if stage is not None else stages[(r, ci, bi)]
    return R.labels(owner, prop_sem, rm['background'], rm['sem'], int(rm['k'][ci, si, bi]), index=index, mistake=mistake)


def _counts(fx, stages, ci, si, bi, mistake=None, rooms=None):
    tp, fp, total = np.zeros(13, np.int64), np.zeros(13, np.int64), np.zeros(13, np.int64)
    for r, rm in enumerate(fx['rooms']):
        if rooms is not None and r not in rooms:
            continue
        gi, gt_class = R.gt_tables(rm['gt_ins'], rm['gt_sem'])
        owner, prop_sem, _ = stages[(r, ci, bi)]
        t, f = R.tail(owner, prop_sem, rm['background'], rm['sem'], [int(rm['k'][ci, si, bi])], gi, gt_class, mistake=mistake)
        tp += t[0]; fp += f[0]; total += np.bincount(gt_class, minlength=13)
    return tp, fp, total


def test_the_score_filter_keeps_a_prefix(fx):
    z = fx['z']
    for r, rm in enumerate(fx['rooms']):
        k = rm['k']
        assert (np.diff(k, axis=1) <= 0).all() and (k == k[:, :, :1]).all()    # fewer with a larger score_th; mask_bin_th selects nothing
        for (ci, bi), masks in rm['stage_masks'].items():
            conf = z['r%d_c%d_b%d_conf' % (r, ci, bi)]
            assert len(masks) == k[ci, 0, bi] == len(conf) and (np.diff(conf) < 0).all()
            for si, th in enumerate(fx['grid'][1]):
                assert k[ci, si, bi] == int((conf > np.float32(th)).sum())


def test_every_setting_equals_the_reference(fx, stages):
    z = fx['z']
    assert len(fx['settings']) == 36
    for q, (ci, si, bi) in enumerate(fx['settings']):
        tag = 'q%02d_' % q
        for r in range(len(fx['rooms'])):
            inst, sem = _labels(fx, stages, r, ci, si, bi)
            want = z[tag + 'r%d_instances' % r]
            assert R.same_partition(inst, want), (q, r)
            assert np.array_equal(inst, want), (q, r)
            assert np.array_equal(sem, z[tag + 'r%d_semantics' % r]), (q, r)
        tp, fp, total = _counts(fx, stages, ci, si, bi)
        assert np.array_equal(tp, z[tag + 'tp']) and np.array_equal(fp, z[tag + 'fp']) and np.array_equal(total, z[tag + 'total_gt']), q
        mprec, mrec, prec, rec = R.metric(tp, fp, total)
        for got, key in ((prec, 'precision'), (rec, 'recall'), (np.float64(mprec), 'mprec'), (np.float64(mrec), 'mrec')):
            g, w = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(z[tag + key])
            nan = np.isnan(w)
            assert np.array_equal(np.isnan(g), nan) and g[~nan].tobytes() == w[~nan].tobytes(), (q, key)     # to the bit


def test_the_full_resolution_room_equals_the_reference(fx, stages):
    z = fx['z']
    s2d = z['full_sparse2dense'].astype(np.int64)
    rm = fx['rooms'][0]
    assert len(s2d) == 3 * rm['n'] and len(np.unique(s2d)) < rm['n'] and (np.bincount(s2d) > 1).any()     # repeats, and skips
    gi, gt_class = R.gt_tables(z['full_gt_instances'], z['full_gt_semantics'])
    n_labels = 0
    for q, (ci, si, bi) in enumerate(fx['settings']):
        tag = 'full_q%02d_' % q
        owner, prop_sem, _ = stages[(0, ci, bi)]
        tp, fp = R.tail(owner, prop_sem, rm['background'], rm['sem'], [int(rm['k'][ci, si, bi])], gi, gt_class, index=s2d)
        total = np.bincount(gt_class, minlength=13)
        assert np.array_equal(tp[0], z[tag + 'tp']) and np.array_equal(fp[0], z[tag + 'fp']) and np.array_equal(total, z[tag + 'total_gt']), q
        mprec, mrec, prec, rec = R.metric(tp[0], fp[0], total)
        assert np.array_equal(prec, z[tag + 'precision'], equal_nan=True) and np.array_equal(rec, z[tag + 'recall'], equal_nan=True)
        assert np.array_equal(np.float64(mprec), z[tag + 'mprec'], equal_nan=True) and np.array_equal(np.float64(mrec), z[tag + 'mrec'], equal_nan=True)
        if tag + 'instances' in z.files:
            inst, sem = _labels(fx, stages, 0, ci, si, bi, index=s2d)
            assert np.array_equal(inst, z[tag + 'instances']) and np.array_equal(sem, z[tag + 'semantics'])
            n_labels += 1
    assert n_labels == 2


# ------------------------------------------------------------------ what the fixture reaches
def _reach(fx, stages):
    """The named cases: {name: (room, ci, si, bi)}, found with the rule and the reference's arrays."""
    z = fx['z']
    nc, ns, nb = (len(fx['grid'][a]) for a in range(3))
    found = {}
    for r, rm in enumerate(fx['rooms']):
        for ci in range(nc):
            for bi in range(nb):
                owner, prop_sem, fate = stages[(r, ci, bi)]
                for name, code in (('rej_ratio', R.REJ_RATIO), ('rej_points', R.REJ_POINTS), ('rej_class', R.REJ_CLASS)):
                    rows = np.nonzero(fate == code)[0]
                    for si in range(ns):
                        if len(rows) and rows[0] < rm['k'][ci, si, bi]:
                            found.setdefault(name, (r, ci, si, bi))
                for si in range(ns):
                    k = int(rm['k'][ci, si, bi])
                    q = _q(fx, ci, si, bi)
                    inst = z['q%02d_r%d_instances' % (q, r)].astype(np.int64)
                    sem = z['q%02d_r%d_semantics' % (q, r)].astype(np.int64)
                    ceiling = rm['background'] == 1
                    if not ((owner >= 0) & (owner < k)).any() and (owner >= 0).any() and ceiling.any() and (inst[ceiling] == -1).all():
                        found.setdefault('ceiling_drop', (r, ci, si, bi))
                    for u in np.unique(inst[inst >= 0]):
                        m = inst == u
                        if R._vote(sem[m]) != R._vote(rm['sem'][m]):
                            found.setdefault('vote_differs', (r, ci, si, bi))
                    if r == 0 and ceiling.any() and (inst[ceiling] >= 0).all():
                        cm, gm = inst == inst[ceiling][0], rm['gt_ins'] == rm['gt_ins'][ceiling][0]
                        if 3 * int((cm & gm).sum()) == int(cm.sum()) + int(gm.sum()):
                            found.setdefault('iou_half', (r, ci, si, bi))
                    wrong = R.paint(rm['stage_masks'][(ci, bi)], rm['sem'], mistake='prop_sem_after_paint')
                    moved = np.nonzero((wrong[1] != prop_sem) & (fate == R.ACCEPTED))[0]
                    if len(moved) and moved[0] < k:
                        found.setdefault('vote_after_paint', (r, ci, si, bi))
                    if si + 1 < ns:
                        qn = _q(fx, ci, si + 1, bi)
                        inst_n = z['q%02d_r%d_instances' % (qn, r)].astype(np.int64)
                        sem_n = z['q%02d_r%d_semantics' % (qn, r)].astype(np.int64)
                        patch = (rm['background'] > 0) & (sem != rm['sem']) & (sem_n == rm['sem'])
                        if 0 < patch.sum() < R.MIN_POINTS and (inst[patch] == -1).all() and (inst_n[patch] >= 0).all():
                            found.setdefault('patch', (r, ci, si, bi))
                        if (z['q%02d_tp' % q] != z['q%02d_tp' % qn]).any():
                            found.setdefault('tp_moves', (r, ci, si, bi))
                    if ((z['q%02d_tp' % q] + z['q%02d_fp' % q]) == 0).any():
                        assert np.isnan(z['q%02d_precision' % q][(z['q%02d_tp' % q] + z['q%02d_fp' % q]) == 0]).all()
                        found.setdefault('nan_precision', (r, ci, si, bi))
    return found


REACH = ('ceiling_drop', 'rej_ratio', 'rej_points', 'rej_class', 'patch', 'tp_moves', 'nan_precision', 'vote_differs', 'iou_half',
         'vote_after_paint')


@pytest.fixture(scope='module')
def reach(fx, stages):
    return _reach(fx, stages)


@pytest.mark.parametrize('name', REACH)
def test_the_fixture_reaches(reach, name):
    assert name in reach, 'a regenerated fixture lost the case %r' % name


def test_the_metric_is_not_flat(fx):
    z = fx['z']
    vals = {(float(z['q%02d_mprec' % q]), float(z['q%02d_mrec' % q])) for q in range(36) if np.isfinite(z['q%02d_mprec' % q])}
    assert len(vals) >= 4


# ------------------------------------------------------------------ deliberate mistakes
def _differs(fx, stages, case, mistake, next_score=False):
    """Labels or counts of the named case change under the mistake."""
    r, ci, si, bi = case
    si += int(next_score)
    rm = fx['rooms'][r]
    stage = R.paint(rm['stage_masks'][(ci, bi)], rm['sem'], mistake=mistake) if mistake == 'prop_sem_after_paint' else None
    good = _labels(fx, stages, r, ci, si, bi)
    bad = _labels(fx, stages, r, ci, si, bi, mistake=mistake, stage=stage)
    if not (np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1])):
        return True
    a, b = _counts(fx, stages, ci, si, bi, rooms=[r]), _counts(fx, stages, ci, si, bi, mistake=mistake, rooms=[r])
    return not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))


@pytest.mark.parametrize('mistake,case,next_score', [
    ('paint_after_overwrite', 'patch', True),       # the patch keeps its repainted class in the setting without its proposal
    ('max_id_full', 'ceiling_drop', False),
    ('small_before_overwrite', 'patch', False),     # the patch under 200 points stays inside the background instance
    ('vote_predicted', 'vote_differs', False),
    ('iou_gt', 'iou_half', False),
    ('ceiling_kept', 'ceiling_drop', False),
    ('prop_sem_after_paint', 'vote_after_paint', False),
])
def test_a_mistake_fails_its_case(fx, stages, reach, mistake, case, next_score):
    assert mistake in R.MISTAKES
    assert _differs(fx, stages, reach[case], mistake, next_score), (mistake, case)


def test_small_pairs_at_evaluation_resolution_fail_the_full_room(fx, stages):
    """Mistake 'small_at_eval': counted on the unsampled room, a pair of 180 sampled points has some 540 and stays."""
    z = fx['z']
    s2d = z['full_sparse2dense'].astype(np.int64)
    hit = 0
    for q, (ci, si, bi) in enumerate(fx['settings']):
        if 'full_q%02d_instances' % q not in z.files:
            continue
        good = _labels(fx, stages, 0, ci, si, bi, index=s2d)
        bad = _labels(fx, stages, 0, ci, si, bi, index=s2d, mistake='small_at_eval')
        assert np.array_equal(good[0], z['full_q%02d_instances' % q])
        hit += int(not np.array_equal(good[0], bad[0]))
    assert hit >= 1
    assert len(R.MISTAKES) >= 8


def test_the_kernel_cases_are_well_formed():
    for n in (1, 63, 64, 65, 4097):
        c = R.kernel_case(n, 7, 5, 12, seed=n, index='gather', min_points=1 if n == 1 else 3)
        assert (np.diff(c['ks']) <= 0).all() and c['ks'][0] == 7 and c['ks'][-1] == 0
        assert (np.bincount(c['index'], minlength=n) == 0).any() or n == 1
        tp, fp = R.tail(c['owner'], c['prop_sem'], c['bg'], c['sem'], c['ks'], c['gi'], c['gt_class'], c['index'], c['min_points'])
        assert tp.shape == (5, 13) and (tp + fp).sum() > 0 and tp.sum() > 0 and (n < 63 or fp.sum() > 0)
