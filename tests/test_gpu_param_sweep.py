"""GPU: the threshold sweep (box2mask_amd/param_search.py) and its two kernels.

  * b2m_mask_nms_sweep / _batch against b2m_mask_nms, flags bit for bit;
  * b2m_mask_hist_index / _batch against b2m_mask_gather -> b2m_mask_pack -> b2m_mask_hist, counts equal, the same bits twice;
  * the whole sweep against tests/golden/param_sweep.npz (36 settings of the real reference, and the one off the grid) and, with
    a second seed, against the single-setting path -- Model.pred2mask and eval_metric.compute_eval per setting;
  * the refusals.
Every comparison is exact."""
import os
import warnings

import numpy as np
import pytest
import torch

import _nms_rule as R
import _sweep_rule as W

pytestmark = pytest.mark.gpu
F = np.float32
SENT = -77


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _call(name, *args):
    from box2mask_amd import _lib
    _lib.call(name, *args)


def _ptr(t):
    return 0 if t is None or t.numel() == 0 else t.data_ptr()


# ----------------------------------------------------------------------------- mask NMS for several thresholds
def _nms_single(bits_dev, k, words, th):
    """keep (k,) of b2m_mask_nms: the yardstick."""
    inter = torch.empty(max(k * k, 1), dtype=torch.int32, device='cuda')
    keep = torch.full((max(k, 1),), SENT, dtype=torch.int32, device='cuda')
    nk = torch.zeros(1, dtype=torch.int32, device='cuda')
    _call('b2m_mask_nms', bits_dev.data_ptr(), k, words, float(th), inter.data_ptr(), keep.data_ptr(), nk.data_ptr())
    return keep[:k].cpu().numpy()


def _nms_sweep(bits_dev, k, words, ths):
    ths = np.ascontiguousarray(ths, F)
    inter = torch.empty(max(k * k, 1), dtype=torch.int32, device='cuda')
    keep = torch.full((len(ths) * k + 1,), SENT, dtype=torch.int32, device='cuda')
    _call('b2m_mask_nms_sweep', bits_dev.data_ptr(), k, words, ths.ctypes.data, len(ths), inter.data_ptr(), keep.data_ptr())
    keep = keep.cpu().numpy()
    assert keep[-1] == SENT                                      # nothing behind the n_th rows
    return keep[:-1].reshape(len(ths), k)


THS = {1: [0.5], 5: [0.1, 0.3, 0.5, 0.7, 0.9]}


def _random_rows(k, n_vox):
    rng = np.random.default_rng(1000 * k + n_vox)
    words = (n_vox + 63) // 64
    if k == 0:
        return np.zeros((0, words), np.uint64)
    bits = R._proto_rows(rng, k, n_vox, words)
    if k >= 3:
        bits[k // 2] = 0                                         # an empty row: 0 / 0 = NaN suppresses
    return bits


@pytest.mark.parametrize('k', [0, 1, 2, 63, 64, 65, 257])
def test_mask_nms_sweep_equals_mask_nms_per_threshold(k):
    """k = 257 is past one 256-thread pass of the walk; n_vox 1 .. 4097 are the word counts 1, 1, 1, 2 and 65."""
    differ = 0
    for n_vox in (1, 63, 64, 65, 4097):
        bits = _random_rows(k, n_vox)
        words = (n_vox + 63) // 64
        bd = _bits(bits) if k else torch.zeros(1, dtype=torch.int64, device='cuda')
        for n_th in (1, 5):
            got = _nms_sweep(bd, k, words, THS[n_th])
            for t, th in enumerate(THS[n_th]):
                assert np.array_equal(got[t], _nms_single(bd, k, words, th)), (k, n_vox, n_th, th)
            differ += n_th == 5 and len({g.tobytes() for g in got}) > 1
    assert differ or k < 2                                       # the thresholds are told apart


def test_mask_nms_sweep_crafted_rows():
    # a pair at IoU exactly 1 / 2: kept at th = 0.5 (`iou <= th`), suppressed below
    bits = R._rows_of([range(0, 1), range(0, 2)], 70)
    got = _nms_sweep(_bits(bits), 2, 2, [0.4, 0.5])
    assert got.tolist() == [[1, 0], [1, 1]]
    # a chain A - B - C with IoU(A, B) = 6 / 14, IoU(B, C) = 8 / 12, IoU(A, C) = 4 / 16: at 0.3 A suppresses B, which SAVES C; at
    # 0.5 B lives and suppresses C; at 0.7 nothing is suppressed -- C's flag is not monotone in the threshold
    bits = R._rows_of([range(0, 10), range(4, 14), range(6, 16)], 64)
    ths = [0.3, 0.5, 0.7]
    got = _nms_sweep(_bits(bits), 3, 1, ths)
    assert got.tolist() == [[1, 0, 1], [1, 1, 0], [1, 1, 1]]
    for t, th in enumerate(ths):
        assert np.array_equal(got[t], _nms_single(_bits(bits), 3, 1, th)) and np.array_equal(got[t], R.mask_nms(bits, th)[1])


def test_mask_nms_sweep_batch_equals_the_single_form():
    """Three scenes, the middle one without a row; field 10 (keep) of the table is NULL throughout: the sweep does not read it."""
    shapes = [(65, 4097), (0, 640), (9, 63)]
    ths = THS[5]
    scenes, devs, want = [], [], []
    for k, n_vox in shapes:
        bits = _random_rows(k, n_vox)
        words = (n_vox + 63) // 64
        d = dict(bits=_bits(bits) if k else None, inter=torch.empty(max(k * k, 1), dtype=torch.int32, device='cuda'))
        scenes.append(dict(ksel=k, words=words, n_vox=n_vox))
        devs.append(d)
        want.append(_nms_sweep(d['bits'], k, words, ths) if k else np.zeros((len(ths), 0), np.int32))
    desc = R.mask_desc(scenes, lambda s, name: _ptr(devs[s].get(name)))
    assert (desc[:, 10] == 0).all() and desc[:, 18].tolist() == [0, 65, 65]
    total = sum(k for k, _ in shapes)
    keep = torch.full((len(ths) * total + 1,), SENT, dtype=torch.int32, device='cuda')
    tf = np.ascontiguousarray(ths, F)
    _call('b2m_mask_nms_sweep_batch', _dev(desc.reshape(-1)).data_ptr(), len(shapes), max(k for k, _ in shapes), tf.ctypes.data, len(ths),
          keep.data_ptr(), total)
    keep = keep.cpu().numpy()
    assert keep[-1] == SENT
    assert np.array_equal(keep[:-1].reshape(len(ths), total), np.concatenate(want, 1))


# ----------------------------------------------------------------------------- point histogram through an index
def _hist_case(k, n_class, n_pts, seed=0):
    rng = np.random.default_rng(seed + 7 * k + n_class + n_pts)
    n_vox = 5003
    words = (n_vox + 63) // 64
    bits = R.pack(rng.random((k, n_vox)) < rng.choice([0.02, 0.3, 0.6], (k, 1)))
    named = np.flatnonzero(rng.random(n_vox) < 0.7)              # the other voxels are named by no point
    index = rng.choice(named, n_pts).astype(np.int64)            # 70 001 points on ~3 500 voxels: repeats
    label = rng.integers(-1, n_class + 1, n_pts).astype(np.int32)        # -1 and n_class are skipped
    return bits, words, n_vox, index, label


def _hist_chain(bd, words, k, idx, lab, n_pts, n_class):
    """b2m_mask_gather -> b2m_mask_pack -> b2m_mask_hist: the definition."""
    out = torch.empty((k, max(n_pts, 1)), dtype=torch.uint8, device='cuda')
    _call('b2m_mask_gather', bd.data_ptr(), words, None, k, _ptr(idx), n_pts, out.data_ptr())
    pw = (n_pts + 63) // 64
    pbits = torch.empty((k, max(pw, 1)), dtype=torch.int64, device='cuda')
    _call('b2m_mask_pack', out.data_ptr(), k, n_pts, pbits.data_ptr(), pw)
    hist = torch.full((k, n_class), SENT, dtype=torch.int32, device='cuda')
    _call('b2m_mask_hist', pbits.data_ptr(), pw, k, _ptr(lab), n_pts, n_class, hist.data_ptr())
    return hist.cpu().numpy()


def _hist_index(bd, words, k, n_vox, idx, lab, n_pts, n_class):
    tb = torch.empty(max(n_vox * ((k + 63) // 64), 1), dtype=torch.int64, device='cuda')
    hist = torch.full((k * n_class + 1,), SENT, dtype=torch.int32, device='cuda')
    _call('b2m_mask_hist_index', bd.data_ptr(), words, k, n_vox, _ptr(idx), _ptr(lab), n_pts, n_class, tb.data_ptr(), hist.data_ptr())
    hist = hist.cpu().numpy()
    assert hist[-1] == SENT
    return hist[:-1].reshape(k, n_class)


@pytest.mark.parametrize('k', [1, 64, 65, 130])
def test_mask_hist_index_equals_gather_pack_hist(k):
    """k at the word boundaries of the voxel-major image; the table at 1, 40 and the cap of 2048 columns; no, one, many points."""
    for n_class in (1, 40, 2048):
        for n_pts in (0, 1, 70001):
            bits, words, n_vox, index, label = _hist_case(k, n_class, n_pts)
            # (no point: the older entries still want a label pointer)
            bd, idx, lab = _bits(bits), _dev(index if n_pts else np.zeros(1, np.int64)), _dev(label if n_pts else np.zeros(1, np.int32))
            want = _hist_chain(bd, words, k, idx, lab, n_pts, n_class)
            got = _hist_index(bd, words, k, n_vox, idx, lab, n_pts, n_class)
            assert np.array_equal(got, want), (k, n_class, n_pts)
            assert np.array_equal(_hist_index(bd, words, k, n_vox, idx, lab, n_pts, n_class), got)         # the same bits twice
            if n_pts > 1:
                skipped = int(((label < 0) | (label >= n_class)).sum())
                assert skipped > 0 and len(np.unique(index)) < min(n_pts, n_vox)
                # (the definition itself, on the host, once per k)
                if n_class == 40:
                    pm = R.gather(bits, None, index, n_pts)
                    ok = (label >= 0) & (label < n_class)
                    assert np.array_equal(got, np.stack([np.bincount(label[ok & (row != 0)], minlength=n_class) for row in pm], 0))


def test_mask_hist_index_batch_equals_the_single_form():
    cases = [(65, 40, 70001), (0, 7, 100), (3, 2048, 1), (130, 5, 0)]
    recs, keep_alive, want = [], [], []
    for k, n_class, n_pts in cases:
        bits, words, n_vox, index, label = _hist_case(max(k, 1), n_class, n_pts, seed=5)
        bd, idx, lab = _bits(bits), _dev(index) if n_pts else None, _dev(label) if n_pts else None
        tb = torch.empty(max(n_vox * ((k + 63) // 64), 1), dtype=torch.int64, device='cuda')
        hist = torch.full((max(k * n_class, 1),), SENT, dtype=torch.int32, device='cuda')
        keep_alive += [bd, idx, lab, tb]
        recs.append((bd.data_ptr(), k, words, n_vox, _ptr(idx), _ptr(lab), n_pts, n_class, tb.data_ptr(), hist.data_ptr()))
        want.append((hist, _hist_index(bd, words, k, n_vox, idx, lab, n_pts, n_class) if k else None))
    desc = _dev(np.array(recs, np.int64).reshape(-1))
    _call('b2m_mask_hist_index_batch', desc.data_ptr(), len(cases), max(r[2] for r in recs), max(r[6] for r in recs))
    for (k, n_class, _), (hist, w) in zip(cases, want):
        if k:
            assert np.array_equal(hist.cpu().numpy().reshape(k, n_class), w)
        else:
            assert (hist.cpu().numpy() == SENT).all()            # a scene without rows writes nothing


# ----------------------------------------------------------------------------- the whole sweep
@pytest.fixture(scope='module')
def model():
    from box2mask_amd import synth
    from box2mask_amd.config import scannet_config
    from box2mask_amd.model import Model
    return Model(scannet_config(), *synth.scannet_tables())


@pytest.fixture(scope='module')
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, 'param_sweep.npz'))


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _same_ap(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a, b, equal_nan=True)


def _against_fixture(model, fx, grid, tags):
    """tags: {setting: fixture tag}.  Every setting of `grid` against what the reference returned for it."""
    from box2mask_amd import param_search
    batch, pred, gts = W.fixture_batch(fx)
    tabs = model.pred2mask_sweep(batch, pred, grid, gts)
    assert [t.name for t in tabs] == [s['name'] for s in batch['scene']]
    n_masks = 0
    for st, tag in tags.items():
        ci, si, bi, mi = st
        mat = param_search.materialize(model.detection_model, batch, pred, model.cfg, grid, tabs, *st)
        for s, t in enumerate(tabs):
            pre = 'sw_%s_s%d_' % (tag, s)
            rows = param_search.compose(t, *st)
            stage, r = t.stages[ci][bi], mat[t.name]
            assert len(rows) == len(fx[pre + 'conf']), (st, s)
            assert _same_bits(t.clusters[ci]['conf'][rows], fx[pre + 'conf']), (st, s)
            assert stage['label_id'].dtype == np.int32 and np.array_equal(stage['label_id'][rows], fx[pre + 'label_id']), (st, s)
            assert np.array_equal(stage['inter'][rows].sum(1), fx[pre + 'count']), (st, s)      # every point has a ground-truth id
            mask = r['mask'].numpy()
            assert r['mask'].dtype == torch.bool and mask.shape == (len(rows), t.n_pts)
            assert _same_bits(r['conf'].numpy(), fx[pre + 'conf']) and np.array_equal(r['label_id'], fx[pre + 'label_id'])
            assert np.array_equal(mask.sum(1), fx[pre + 'count']) and np.array_equal(W.content_sums(mask), fx[pre + 'sum']), (st, s)
            if pre + 'mask' in fx.files:
                assert np.array_equal(np.packbits(mask, axis=1), fx[pre + 'mask'])
                n_masks += 1
    res = param_search.scannet_param_search(model, [(batch, pred)], gts, grid, per_class=True)
    for st, tag in tags.items():
        assert _same_ap(res['ap_tables'][st], fx['sw_%s_ap' % tag]), st
        assert _same_ap(res['ap'][st], fx['sw_%s_avg' % tag]), st
    return res, n_masks


def test_sweep_reproduces_every_setting_of_the_reference(model, fx):
    grid = W.fixture_grid(fx)
    res, n_masks = _against_fixture(model, fx, grid, {st: 'q%02d' % q for q, st in enumerate(grid.settings())})
    assert n_masks == 4                                          # two settings x two scenes carry their masks
    ap = res['ap'].reshape(-1, 3)
    order = sorted(range(36), key=lambda q: (-ap[q, 1], -ap[q, 0], q))
    assert res['best'] == tuple(int(v) for v in np.unravel_index(order[0], grid.shape)) and res['best_ths'] == grid.eval_ths(*res['best'])
    assert 1 <= res['n_evaluated'] <= 36


def test_sweep_score_threshold_equal_to_a_score(model, fx):
    """score_th equal to the score of an instance: `scores > score_th` drops it."""
    from box2mask_amd import param_search
    grid = param_search.ThresholdGrid(*([v] for v in fx['sw_tie_ths']))
    _against_fixture(model, fx, grid, {(0, 0, 0, 0): 'tie'})


def test_sweep_equals_the_single_setting_path(model):
    """No fixture: a second seed, a 2 x 2 x 2 x 2 grid, every setting against Model.pred2mask(..., 'eval') with cfg.eval_ths set to
    it and eval_metric.compute_eval on those results (the path the existing goldens pin to the reference)."""
    from box2mask_amd import eval_metric, param_search
    batch, pred, gts = W.synthetic_inputs(23)
    grid = param_search.ThresholdGrid([0.4, 0.6], [0.02, 0.15], [0.25, 0.3], [0.5, 0.7])
    tabs = model.pred2mask_sweep(batch, pred, grid, gts)
    res = param_search.scannet_param_search(model, [(batch, pred)], gts, grid)
    saved = model.cfg.eval_ths
    counts = set()
    try:
        for st in grid.settings():
            model.cfg.eval_ths = grid.eval_ths(*st)
            want = model.pred2mask(batch, pred, 'eval')
            got = param_search.materialize(model.detection_model, batch, pred, model.cfg, grid, tabs, *st)
            assert list(got) == list(want)
            for name in want:
                assert torch.equal(got[name]['mask'], want[name]['mask']), (st, name)
                assert np.array_equal(got[name]['label_id'], want[name]['label_id']) and got[name]['label_id'].dtype == want[name]['label_id'].dtype
                assert _same_bits(got[name]['conf'].numpy(), want[name]['conf'].numpy()), (st, name)
            counts.add(tuple(int(want[n]['mask'].shape[0]) for n in want))
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)
                avg, _ = eval_metric.compute_eval(want, gts)
            assert _same_ap(res['ap'][st], [avg['all_ap'], avg['all_ap_50%'], avg['all_ap_25%']]), st
    finally:
        model.cfg.eval_ths = saved
    assert len(counts) >= 4                                      # the settings are told apart


def test_sweep_refusals(model, fx):
    from box2mask_amd import param_search
    batch, pred, gts = W.fixture_batch(fx)
    grid = W.fixture_grid(fx)
    net = model.detection_model
    # the S3DIS flow (per-voxel semantics, no mask NMS) is refused
    net.requires_voxel_outputs = True
    try:
        with pytest.raises(ValueError, match='ScanNet flow'):
            model.pred2mask_sweep(batch, pred, grid, gts)
    finally:
        net.requires_voxel_outputs = False
    # a scene without foreground votes raises as detection2mask does
    bg = dict(pred)
    sem = torch.full_like(pred['mlp_semantics'], -10.0)
    sem[:, 0] = 10.0                                             # class id 1 for every vote: no foreground
    bg['mlp_semantics'] = sem
    with pytest.raises(ValueError, match='at least one box'):
        net.detection2mask(batch, bg, model.cfg, 'eval', True, *model.cfg.eval_ths)
    with pytest.raises(ValueError, match='at least one box'):
        model.pred2mask_sweep(batch, bg, grid, gts)
    # ground-truth ids of another scene
    with pytest.raises(ValueError, match='ground-truth ids'):
        model.pred2mask_sweep(batch, pred, grid, {n: v[:-1] for n, v in gts.items()})


def test_sweep_setting_that_keeps_no_cluster(model, fx):
    """score_th above every score: an empty prediction for the scene, as detection2mask gives today."""
    from box2mask_amd import param_search
    batch, pred, gts = W.fixture_batch(fx)
    grid = param_search.ThresholdGrid([0.5], [0.05, 1.5], [0.3], [0.6])
    tabs = model.pred2mask_sweep(batch, pred, grid, gts)
    for t in tabs:
        assert t.clusters[0]['ks'][1] == 0 and len(param_search.compose(t, 0, 1, 0, 0)) == 0
    got = param_search.materialize(model.detection_model, batch, pred, model.cfg, grid, tabs, 0, 1, 0, 0)
    want = model.detection_model.detection2mask(batch, pred, model.cfg, 'eval', True, 0.5, 1.5, 0.3, 0.6)
    for name in want:
        assert tuple(got[name]['mask'].shape) == tuple(want[name]['mask'].shape) and got[name]['mask'].shape[0] == 0
    res = param_search.scannet_param_search(model, [(batch, pred)], gts, grid)
    assert res['best'] == (0, 0, 0, 0) and res['ap'][0, 1, 0, 0, 1] == 0.0
    # ... and a grid no setting of which keeps one: no row is projected at all
    none = param_search.ThresholdGrid([0.5], [1.5], [0.3], [0.6])
    for t in model.pred2mask_sweep(batch, pred, none, gts):
        st = t.stages[0][0]
        assert st['keep'].shape == (1, 0) and st['inter'].shape == (0, len(t.uniq)) and len(st['label_id']) == 0
