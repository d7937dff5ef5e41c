"""The rule of the threshold sweep (tests/_sweep_rule.py) against the real reference: composing "prefix, then restriction of the
full-list NMS" from the tables the settings share reproduces, for all 36 settings of tests/golden/param_sweep.npz, what
SelectionNet.detection2mask returned setting by setting -- scores (bits), labels, every mask's point count and content sum --
and, through param_search.compose + eval_metric.assign_from_counts + evaluate_matches, the AP tables of utils/eval_metric.py
exactly.  CPU only."""
import os
import warnings

import numpy as np
import pytest

import _sweep_rule as W
from box2mask_amd import eval_metric, param_search
from box2mask_amd.config import scannet_config


@pytest.fixture(scope='module')
def fx(golden_dir):
    d = np.load(os.path.join(golden_dir, 'param_sweep.npz'))
    grid = W.fixture_grid(d)
    scenes = W.fixture_scenes(d)
    # (the setting off the grid: score_th equal to the score of a kept instance, see gen_sweep)
    tie = param_search.ThresholdGrid(*([v] for v in d['sw_tie_ths']))
    return d, (grid, tie), scenes, {}


def _same_ap(a, b):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a, b, equal_nan=True)


def misses(fx, mistake=None):
    """The (setting tag, scene, what) at which the rule -- or a mistaken variant of it -- leaves the fixture."""
    d, (grid, tie), scenes, cache = fx
    table_level = mistake in ('ge_score', 'inter_on_voxels')
    key = mistake if table_level else None
    if key not in cache:
        cache[key] = [[W.shared_tables(s, g, key) for s in scenes] for g in (grid, tie)]
    out = []
    for tag, shared, st in [('q%02d' % q, cache[key][0], st) for q, st in enumerate(grid.settings())] + [('tie', cache[key][1], (0, 0, 0, 0))]:
        if tag == 'tie' and mistake == 'ks_of_other_cluster_th':
            continue                                                # (one cluster_th: there is no other)
        ci, si, bi, mi = st
        matches = {}
        for s, (t, pms) in enumerate(shared):
            rows = W.compose(t, ci, si, bi, mi, None if table_level else mistake)
            if mistake is None:
                assert np.array_equal(rows, param_search.compose(t, ci, si, bi, mi))
            pre = 'sw_%s_s%d_' % (tag, s)
            stage, pm = t.stages[ci][bi], pms[ci][bi][rows]
            if not _same_bits(t.clusters[ci]['conf'][rows], d[pre + 'conf']):
                out.append((tag,s, 'conf'))
            if not np.array_equal(stage['label_id'][rows], d[pre + 'label_id']):
                out.append((tag,s, 'label_id'))
            if not np.array_equal(pm.sum(1).astype(np.int64), d[pre + 'count']):
                out.append((tag,s, 'count'))
            elif not np.array_equal(stage['inter'][rows].sum(1), d[pre + 'count']):
                out.append((tag,s, 'inter'))                       # every point has a ground-truth id: the row sums are the counts
            if not np.array_equal(W.content_sums(pm), d[pre + 'sum']):
                out.append((tag,s, 'sum'))
            if pre + 'mask' in d.files and not np.array_equal(np.packbits(pm != 0, axis=1), d[pre + 'mask']):
                out.append((tag,s, 'mask'))
            matches[t.name] = eval_metric.assign_from_counts(t.name, stage['label_id'][rows].astype(np.int64), t.clusters[ci]['conf'][rows],
                                                             t.uniq, t.gt_vert, stage['inter'][rows])
        ap, _ = eval_metric.evaluate_matches(matches)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            avg = eval_metric.compute_averages(ap)
        if not _same_ap(ap, d['sw_%s_ap' % tag]):
            out.append((tag,None, 'ap'))
        if not _same_ap(np.array([avg['all_ap'], avg['all_ap_50%'], avg['all_ap_25%']]), d['sw_%s_avg' % tag]):
            out.append((tag,None, 'avg'))
    return out


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_fixture_is_not_flat(fx):
    d, (grid, tie), _, _ = fx
    assert grid.shape == (3, 3, 2, 2) and tie.shape == (1, 1, 1, 1)
    assert (d['sw_q%02d_s0_conf' % 13] == np.float32(tie.score_th[0])).sum() == 1      # setting (1, 0, 0, 1) keeps that very score
    k = np.array([[len(d['sw_q%02d_s%d_conf' % (q, s)]) for s in range(2)] for q in range(36)]).reshape(3, 3, 2, 2, 2)
    for axis in range(4):
        assert (np.diff(k, axis=axis) != 0).any()
    assert len({tuple(d['sw_q%02d_avg' % q].tolist()) for q in range(36)}) >= 8
    assert sum(('sw_q%02d_s0_mask' % q) in d.files for q in range(36)) == 2


def test_shared_tables_reproduce_every_setting_of_the_reference(fx):
    assert misses(fx) == []


def test_records_are_the_product_records(fx):
    """param_search.records on the rule's tables is assign_from_counts on the composed rows."""
    misses(fx)
    t = fx[3][None][0][0][0]
    for st in [(0, 0, 0, 1), (2, 2, 1, 0)]:
        rec = param_search.records(t, *st)
        rows = param_search.compose(t, *st)
        assert rec['scene'] == t.name and rec['n_pred'] <= len(rows)
        assert sum(len(c['conf']) for c in rec['classes'].values()) == rec['n_pred']


@pytest.mark.parametrize('mistake', W.MISTAKES)
def test_the_fixture_catches_the_mistake(fx, mistake):
    got = misses(fx, mistake)
    assert got, mistake
    if mistake == 'ge_score':                   # no score of these inputs equals a grid value: only the setting off the grid can tell
        assert {tag for tag, _, _ in got} == {'tie'}


def test_default_grid_is_the_reference_grid():
    g = param_search.ThresholdGrid.from_cfg(scannet_config())
    assert g.shape == (6, 5, 4, 5)
    for a, triple in zip(param_search.AXES, ([0.3, 0.8, 6], [0, 0.2, 5], [0.2, 0.35, 4], [0.4, 0.8, 5])):   # config_loader.py:133-139
        want = np.linspace(*triple)
        got = getattr(g, a)
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert len(list(g.settings())) == 600 and g.eval_ths(0, 0, 0, 0) == [0.3, 0.0, 0.2, 0.4]


def test_sweep_entries_check_their_arguments_on_the_host():
    """Negative return and b2m_last_error before anything touches a device (the convention of include/b2m.h)."""
    from box2mask_amd import _lib
    lib = _lib.load()
    err = lambda: lib.b2m_last_error().decode()
    ths = np.array([0.5] * 65, np.float32)
    p = ths.ctypes.data
    assert lib.b2m_mask_nms_sweep(None, 1, 1, p, 0, None, None, None) < 0 and 'n_th' in err()
    assert lib.b2m_mask_nms_sweep(None, 1, 1, p, 65, None, None, None) < 0 and 'n_th' in err()
    assert lib.b2m_mask_nms_sweep(None, 1, 1, None, 1, None, None, None) < 0 and 'n_th' in err()
    assert lib.b2m_mask_nms_sweep(None, 70000, 1, p, 1, None, None, None) < 0 and 'sizes' in err()
    assert lib.b2m_mask_nms_sweep(None, 1, 1, p, 1, None, None, None) < 0 and 'NULL' in err()
    assert lib.b2m_mask_nms_sweep(None, 0, 1, p, 1, None, None, None) == 0                 # no row: nothing to do, no launch
    assert lib.b2m_mask_nms_sweep_batch(None, 1, 1, p, 0, None, 1, None) < 0 and 'n_th' in err()
    assert lib.b2m_mask_nms_sweep_batch(None, 1, 1, p, 1, None, 1, None) < 0 and 'NULL' in err()
    assert lib.b2m_mask_nms_sweep_batch(None, 0, 0, p, 1, None, 0, None) == 0
    assert lib.b2m_mask_hist_index(None, 1, 1, 64, None, None, 1, 2049, None, None, None) < 0 and 'n_class' in err()
    assert lib.b2m_mask_hist_index(None, 2, 1, 64, None, None, 1, 4, None, None, None) < 0 and 'words' in err()
    assert lib.b2m_mask_hist_index(None, 1, 1, 64, None, None, 1, 4, None, None, None) < 0 and 'NULL' in err()
    assert lib.b2m_mask_hist_index(None, 1, 0, 64, None, None, 1, 4, None, None, None) == 0
    assert lib.b2m_mask_hist_index_batch(None, 1, 1, 1, None) < 0 and 'NULL' in err()
    assert lib.b2m_mask_hist_index_batch(None, 0, 0, 0, None) == 0


@pytest.mark.parametrize('bad', [dict(cluster_th=[0.0, 0.5]), dict(cluster_th=[0.5, 1.0]), dict(mask_bin_th=[-0.1, 0.2]),
                                 dict(mask_bin_th=[0.5, 1.0]), dict(score_th=[0.2, 0.1]), dict(mask_nms_th=[])])
def test_grid_validation(bad):
    kw = dict(cluster_th=[0.3, 0.5], score_th=[0.0, 0.1], mask_bin_th=[0.2, 0.3], mask_nms_th=[0.4, 0.8])
    kw.update(bad)
    with pytest.raises(ValueError):
        param_search.ThresholdGrid(**kw)
