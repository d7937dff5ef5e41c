"""GPU: the S3DIS threshold sweep -- b2m_s3dis_prefix_tail against the rule of tests/_s3dis_sweep_rule.py bit for bit, and
param_search.s3dis_param_search on the two rooms of tests/golden/s3dis_sweep.npz against the 36 settings of the real reference and
against the one-setting route (Model.pred2mask + room_labels + s3dis_counts + s3dis_eval_from_counts with cfg.eval_ths set).

The kernel's rooms are a few points large with min_points = 3 (the ABI takes the 200 of the reference as a parameter), so every
rule -- prefix restriction, max_id of the prefix, the ceiling drop, the background overwrite, the small pairs, the class vote, IoU
>= 0.5 in integers -- decides at sizes 1, 63, 64, 65 and 4097.  Every comparison is exact."""
import numpy as np
import pytest
import torch

import _s3dis_sweep_rule as R

pytestmark = pytest.mark.gpu
SENT = -77


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(c, n_inst=None, label_setting=-1, tp=None, fp=None):
    """One call of the C entry on a case of R.kernel_case: (tp, fp (S, 13) device int32, labels or None)."""
    from box2mask_amd import param_search as P
    S = len(c['ks'])
    tp = torch.zeros((S, 13), dtype=torch.int32, device='cuda') if tp is None else tp
    fp = torch.zeros((S, 13), dtype=torch.int32, device='cuda') if fp is None else fp
    n_gt = len(c['gt_class'])
    gt_size = np.bincount(c['gi'][(c['gi'] >= 0) & (c['gi'] < n_gt)], minlength=n_gt).astype(np.int32)
    lab = P.s3dis_prefix_tail(_dev(c['owner']), _dev(c['prop_sem']), _dev(c['bg']), _dev(c['sem']), c['ks'],
                              c['n_inst'] if n_inst is None else n_inst, _dev(c['gi']), _dev(c['gt_class']), _dev(gt_size), tp, fp,
                              index=None if c['index'] is None else _dev(c['index']), min_points=c['min_points'],
                              label_setting=label_setting)
    return tp, fp, lab


def _check(c, n_inst=None):
    want_tp, want_fp = R.tail(c['owner'], c['prop_sem'], c['bg'], c['sem'], c['ks'], c['gi'], c['gt_class'], c['index'], c['min_points'])
    mid = len(c['ks']) // 2
    tp, fp, lab = _run(c, n_inst, label_setting=mid)
    assert np.array_equal(tp.cpu().numpy(), want_tp) and np.array_equal(fp.cpu().numpy(), want_fp)
    inst, sem = R.labels(c['owner'], c['prop_sem'], c['bg'], c['sem'], int(c['ks'][mid]), c['index'], c['min_points'])
    assert np.array_equal(lab[0].cpu().numpy(), inst) and np.array_equal(lab[1].cpu().numpy(), sem)
    # a second run adds the same counts: nothing depends on the order of the atomics
    tp2, fp2, _ = _run(c, n_inst, tp=tp.clone(), fp=fp.clone())
    assert np.array_equal(tp2.cpu().numpy(), 2 * want_tp) and np.array_equal(fp2.cpu().numpy(), 2 * want_fp)
    return want_tp, want_fp


@pytest.mark.parametrize('index', [None, 'gather'])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 4097])
def test_tail_equals_the_rule_at_the_sizes(n, index):
    c = R.kernel_case(n, 7, 5, 12, seed=n, index=index, min_points=1 if n == 1 else 3)
    assert c['ks'][0] == 7 and c['ks'][-1] == 0                           # k_s = K' and k_s = 0
    tp, fp = _check(c)
    assert tp.sum() > 0 and (n < 63 or fp.sum() > 0)
    if index == 'gather':
        named = np.bincount(c['index'], minlength=n)
        assert (named > 1).any() and (n == 1 or (named == 0).any())       # the index repeats, and skips sampled points


@pytest.mark.parametrize('n_inst', [400, 700])
def test_tail_tables_in_global_memory(n_inst):
    """400 instance ids: the pair table fits the LDS image, the evaluation tables do not; 700: neither does."""
    c = R.kernel_case(4097, 7, 5, 12, seed=11, index='gather')
    _check(c, n_inst=n_inst)


def test_tail_edges():
    # no proposal row at all
    c = R.kernel_case(65, 0, 3, 12, seed=1)
    assert len(c['prop_sem']) == 0 and (c['ks'] == 0).all()
    _check(c)
    # one setting, and sixty-four
    _check(R.kernel_case(300, 7, 1, 12, seed=2))
    c = R.kernel_case(300, 70, 64, 80, seed=3, index='gather')
    assert len(set(c['ks'].tolist())) > 20
    _check(c)
    # owners that are all -1: only the background is left, and every prefix gives the same counts
    c = R.kernel_case(300, 7, 4, 12, seed=4, owners=False)
    tp, fp = _check(c)
    assert (tp == tp[0]).all() and (fp == fp[0]).all()
    # one ground-truth instance
    c = R.kernel_case(300, 7, 4, 1, seed=5)
    assert c['gi'].max() == 0
    _check(c)
    # the thresholds of the reference on a room just large enough: pairs of 199 and 200 points
    n = 1000
    owner = np.full(n, -1, np.int32); owner[:200] = 0; owner[200:399] = 1
    sem = np.full(n, 1, np.int32); bg = np.zeros(n, np.int32); bg[399:] = 2
    gi = np.zeros(n, np.int32); gi[200:399] = 1; gi[399:] = 2
    c = dict(owner=owner, prop_sem=np.array([5, 6], np.int32), bg=bg, sem=sem, ks=np.array([2, 1, 0], np.int32), gi=gi,
             gt_class=np.array([5, 6, 1], np.int32), index=None, min_points=200, n_inst=5)
    tp, fp = _check(c)
    assert tp[0].tolist() == [0, 1, 0, 0, 0, 1] + [0] * 7 and fp.sum() == 0          # the row of 199 points is gone, 200 stays


def test_tail_iou_of_exactly_one_half():
    """P inside G with |G| = 2 |P|: 3 * inter == |P| + |G|, a true positive; one point less is not."""
    for cut, want in ((50, 1), (49, 0)):
        n = 100
        owner = np.full(n, -1, np.int32); owner[:cut] = 0
        c = dict(owner=owner, prop_sem=np.array([4], np.int32), bg=np.zeros(n, np.int32), sem=np.full(n, 4, np.int32),
                 ks=np.array([1], np.int32), gi=np.zeros(n, np.int32), gt_class=np.array([4], np.int32), index=None, min_points=3, n_inst=2)
        tp, fp = _check(c)
        assert tp[0, 4] == want and fp[0, 4] == 1 - want


def test_tail_refusals_and_empty_rooms():
    from box2mask_amd import _lib
    c = R.kernel_case(65, 7, 3, 12, seed=9)
    with pytest.raises(_lib.B2MError, match='n_set'):
        _run(dict(c, ks=np.zeros(0, np.int32)))
    with pytest.raises(_lib.B2MError, match='n_set'):
        _run(dict(c, ks=np.zeros(65, np.int32)))
    with pytest.raises(_lib.B2MError, match='not increase'):
        _run(dict(c, ks=np.array([3, 5, 0], np.int32)))
    with pytest.raises(_lib.B2MError, match='exceeds the number of proposal rows'):
        _run(dict(c, ks=np.array([8, 5, 0], np.int32)))
    with pytest.raises(_lib.B2MError, match='exceed the tables'):
        _run(c, n_inst=1 << 20)
    assert _lib.load().b2m_s3dis_prefix_tail_workspace(7, 3, 1 << 20, 12) == -1
    # ... and by the C entry itself, before it touches its workspace
    one = torch.zeros(64, dtype=torch.int32, device='cuda')
    ks = np.array([7, 5, 0], np.int32)
    lib = _lib.load()
    rc = lib.b2m_s3dis_prefix_tail(one.data_ptr(), one.data_ptr(), 7, one.data_ptr(), one.data_ptr(), 64, ks.ctypes.data, 3, 1 << 20, 3,
                                   one.data_ptr(), one.data_ptr(), one.data_ptr(), 12, None, 64, one.data_ptr(), one.data_ptr(),
                                   one.data_ptr(), -1, None, None, _lib.stream())
    assert rc < 0 and 'B2M_JOINT_HIST_MAX' in lib.b2m_last_error().decode()
    with pytest.raises(_lib.B2MError, match='B2M_JOINT_HIST_MAX'):
        _lib.call('b2m_s3dis_prefix_tail', one.data_ptr(), one.data_ptr(), 7, one.data_ptr(), one.data_ptr(), 64, ks.ctypes.data, 3,
                  1 << 20, 3, one.data_ptr(), one.data_ptr(), one.data_ptr(), 12, None, 64, one.data_ptr(), one.data_ptr(),
                  one.data_ptr(), -1, None, None)
    torch.cuda.synchronize()
    assert int(one.abs().sum()) == 0                                       # nothing was launched
    # n = 0 or n_eval = 0: nothing is launched, nothing is written
    for empty in (dict(c, owner=c['owner'][:0], bg=c['bg'][:0], sem=c['sem'][:0]),
                  dict(c, gi=c['gi'][:0], index=np.zeros(0, np.int64))):
        tp = torch.full((3, 13), SENT, dtype=torch.int32, device='cuda')
        fp = torch.full((3, 13), SENT, dtype=torch.int32, device='cuda')
        _run(empty, tp=tp, fp=fp)
        torch.cuda.synchronize()
        assert (tp == SENT).all() and (fp == SENT).all()


# ----------------------------------------------------------------------------- the search on the golden rooms
@pytest.fixture(scope='module')
def fx():
    return R.load()


@pytest.fixture(scope='module')
def model():
    from box2mask_amd.config import scannet_config
    from box2mask_amd.model import Model
    cfg = scannet_config(network_heads=['mlp_offsets', 'mlp_bounds', 'mlp_bb_scores', 'mlp_per_vox_semantics'],
                         eval_ths=[0.5, 0.03, 0.3, 0.6], loss_weight_bb_scores=3.0, batch_size=4)
    ids = torch.arange(13).long()
    torch.manual_seed(0)
    m = Model(cfg, torch.Tensor(np.arange(13)), ids, ids.clone(), (lambda s: s > 2))
    m.eval()
    return m


@pytest.fixture(scope='module')
def grid(fx):
    from box2mask_amd import param_search as P
    return P.ThresholdGrid(*fx['grid'])


@pytest.fixture(scope='module')
def items(fx):
    return [R.room_batch(rm) for rm in fx['rooms']]


@pytest.fixture(scope='module')
def sweep(model, items, grid):
    from box2mask_amd import param_search as P
    return P.s3dis_param_search(model, items, grid, per_class=True)


def _bits_equal(got, want):
    got, want = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(want, np.float64))
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and got[~nan].tobytes() == want[~nan].tobytes()


def test_search_equals_the_reference(fx, sweep):
    z = fx['z']
    assert sweep['mprec'].shape == sweep['mrec'].shape == (3, 4, 3) and sweep['tp'].shape == (3, 4, 3, 13)
    for q, st in enumerate(fx['settings']):
        tag = 'q%02d_' % q
        assert np.array_equal(sweep['tp'][st], z[tag + 'tp']) and np.array_equal(sweep['fp'][st], z[tag + 'fp']), st
        assert np.array_equal(sweep['total_gt'], z[tag + 'total_gt'])
        assert _bits_equal(sweep['precision'][st], z[tag + 'precision']) and _bits_equal(sweep['recall'][st], z[tag + 'recall']), st
        assert _bits_equal(sweep['mprec'][st], z[tag + 'mprec']) and _bits_equal(sweep['mrec'][st], z[tag + 'mrec']), st


def test_stage_labels_equal_the_reference(fx, model, items, grid):
    """The labels of every setting, from the shared stage and the kernel: instances and semantics of the 36 x 2 reference rooms."""
    from box2mask_amd import eval_s3dis as S
    from box2mask_amd import mask_stages as M
    from box2mask_amd import param_search as P
    z = fx['z']
    dev = torch.device('cuda')
    for r, (batch, pred) in enumerate(items):
        rm = fx['rooms'][r]
        d = P._s3dis_room(model.detection_model, batch, pred, model.cfg, dev)
        assert np.array_equal(d['sem_pts'].cpu().numpy(), rm['sem'])
        bg = S.clustering_for_background(d['sem_pts'], rm['positions'], rm['normals']).contiguous()
        assert np.array_equal(bg.cpu().numpy(), rm['background'])
        gi, gt_class, gt_size, _ = P._s3dis_ground_truth(batch['labels'][0], dev)
        assert np.array_equal(gt_size.cpu().numpy(), np.bincount(R.gt_tables(rm['gt_ins'], rm['gt_sem'])[0]))
        want_gi, want_cls = R.gt_tables(rm['gt_ins'], rm['gt_sem'])
        assert np.array_equal(gi.cpu().numpy(), want_gi) and np.array_equal(gt_class.cpu().numpy(), want_cls)
        for ci, cth in enumerate(grid.cluster_th):
            (r0, conf, _), = M.clusters([d], float(cth))
            for bi, bth in enumerate(grid.mask_bin_th):
                ks = M.score_prefixes(conf, grid.score_th)
                assert np.array_equal(ks, rm['k'][ci, :, bi])
                owner, prop_sem, accepted, masks = P.s3dis_stage(d, r0, int(ks[0]), bth)
                assert np.array_equal(masks.cpu().numpy().astype(bool), rm['stage_masks'][(ci, bi)])
                want_owner, want_sem, fate = R.paint(rm['stage_masks'][(ci, bi)], rm['sem'])
                assert np.array_equal(owner.cpu().numpy(), want_owner) and np.array_equal(prop_sem.cpu().numpy(), want_sem)
                assert np.array_equal(accepted.cpu().numpy() != 0, fate == R.ACCEPTED)
                for si in range(len(ks)):
                    tp = torch.zeros((len(ks), 13), dtype=torch.int32, device=dev)
                    inst, sem = P.s3dis_prefix_tail(owner, prop_sem, bg, d['sem_pts'], ks, int(ks[0]) + int(bg.max()) + 1, gi, gt_class,
                                                    gt_size, tp, torch.zeros_like(tp), label_setting=si)
                    q = fx['settings'].index((ci, si, bi))
                    assert np.array_equal(inst.cpu().numpy(), z['q%02d_r%d_instances' % (q, r)]), (r, ci, si, bi)
                    assert np.array_equal(sem.cpu().numpy(), z['q%02d_r%d_semantics' % (q, r)]), (r, ci, si, bi)


def test_search_equals_the_one_setting_route(fx, model, items, grid, sweep):
    """Every setting once more through the route the existing goldens pin: cfg.eval_ths, Model.pred2mask, room_labels, s3dis_counts,
    s3dis_eval_from_counts.  Precision and recall per class (tp / (tp + fp) and tp / total_gt of the same integers), mPrec and mRec."""
    from box2mask_amd import eval_s3dis as S
    cfg = model.cfg
    saved = cfg.eval_ths
    sems = [torch.argmax(pred[cfg.mlp_per_vox_semantics], 1)[torch.as_tensor(batch['vox2point'][0])].cuda() for batch, pred in items]
    try:
        for st in fx['settings']:
            cfg.eval_ths = grid.eval_ths(*st, 0)
            counts = []
            for (batch, pred), sem in zip(items, sems):
                scene, labels = batch['scene'][0], batch['labels'][0]
                res = model.pred2mask(batch, {k: v.clone() for k, v in pred.items()}, 'eval')
                lab = S.room_labels(sem, scene['positions'], scene['normals'], res[scene['name']]['mask'])
                counts.append(S.s3dis_counts(lab, labels))
            mprec, mrec, prec, rec = S.s3dis_eval_from_counts(counts)
            assert _bits_equal(sweep['precision'][st], prec) and _bits_equal(sweep['recall'][st], rec), st
            assert _bits_equal(sweep['mprec'][st], mprec) and _bits_equal(sweep['mrec'][st], mrec), st
            tp, fp, total = S.instance_counts(counts)                          # the integers behind them
            assert np.array_equal(sweep['tp'][st], tp) and np.array_equal(sweep['fp'][st], fp) and np.array_equal(sweep['total_gt'], total), st
    finally:
        cfg.eval_ths = saved


def test_mask_nms_th_has_no_effect_and_best(fx, model, items, grid, sweep):
    from box2mask_amd import param_search as P
    other = P.ThresholdGrid(fx['grid'][0], fx['grid'][1], fx['grid'][2], [0.1, 0.5, 0.9])
    res = P.s3dis_param_search(model, items, other, per_class=True)
    for key in ('tp', 'fp', 'total_gt'):
        assert np.array_equal(res[key], sweep[key]), key
    for key in ('mprec', 'mrec', 'precision', 'recall'):
        assert _bits_equal(res[key], sweep[key]), key
    with np.errstate(all='ignore'):
        f1 = 2 * sweep['mprec'] * sweep['mrec'] / (sweep['mprec'] + sweep['mrec'])
    order = sorted(range(36), key=lambda q: (-(f1.reshape(-1)[q] if np.isfinite(f1.reshape(-1)[q]) else -np.inf), q))
    ci, si, bi = fx['settings'][order[0]]
    assert np.isnan(f1).any() and np.isfinite(f1).any()
    assert sweep.best() == grid.eval_ths(ci, si, bi, 0) and res.best()[:3] == sweep.best()[:3] and res.best()[3] == 0.1
    with pytest.raises(ValueError, match='f1'):
        sweep.best('ap')


def test_search_at_full_resolution(fx, model, items, grid):
    """Room 0 alone with cfg.full_resolution: the labels go to the unsampled room through sparse2dense, the small pairs are
    counted on the sampled room."""
    from box2mask_amd import param_search as P
    z = fx['z']
    cfg = model.cfg
    full = ({'name': 'room0', 'positions': z['full_grid'].astype(np.float64) * R.GRID},
            {'semantics': z['full_gt_semantics'].astype(np.int64), 'instances': z['full_gt_instances'].astype(np.int64)})
    cfg.full_resolution = True
    try:
        with pytest.raises(NotImplementedError):
            P.s3dis_param_search(model, items[:1], grid)
        res = P.s3dis_param_search(model, items[:1], grid, full_rooms=[full], per_class=True)
        by_name = P.s3dis_param_search(model, items[:1], grid, full_rooms=lambda name: full, per_class=True)
    finally:
        cfg.full_resolution = False
    for q, st in enumerate(fx['settings']):
        tag = 'full_q%02d_' % q
        assert np.array_equal(res['tp'][st], z[tag + 'tp']) and np.array_equal(res['fp'][st], z[tag + 'fp']), st
        assert np.array_equal(res['total_gt'], z[tag + 'total_gt'])
        assert _bits_equal(res['precision'][st], z[tag + 'precision']) and _bits_equal(res['recall'][st], z[tag + 'recall']), st
        assert _bits_equal(res['mprec'][st], z[tag + 'mprec']) and _bits_equal(res['mrec'][st], z[tag + 'mrec']), st
    assert np.array_equal(by_name['tp'], res['tp']) and np.array_equal(by_name['fp'], res['fp'])


def test_search_refusals(model, items, grid):
    from box2mask_amd import param_search as P
    batch, pred = items[0]
    net = model.detection_model
    net.requires_voxel_outputs = False
    try:
        with pytest.raises(ValueError, match='per-voxel semantics head'):
            P.s3dis_param_search(model, items[:1], grid)
    finally:
        net.requires_voxel_outputs = True
    with pytest.raises(ValueError, match='s3dis_param_search'):           # the ScanNet sweep points here
        P.sweep_tables(net, batch, pred, model.cfg, grid, {batch['scene'][0]['name']: np.zeros(len(batch['vox2point'][0]), np.int64)})
    two = dict(batch, scene=batch['scene'] * 2)
    with pytest.raises(ValueError, match='batch size 1'):
        P.s3dis_param_search(model, [(two, pred)], grid)
