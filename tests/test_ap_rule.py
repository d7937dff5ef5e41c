"""The rule of the device ScanNet AP (tests/_ap_rule.py) against the host route, eval_metric.assign_from_counts +
evaluate_matches, which tests/golden/eval_metric.npz and tests/golden/param_sweep.npz pin to the reference bit for bit.

On the records rebuilt from tests/golden/param_sweep.npz (36 settings, two scenes), on hand-built edge scenes and on seeded random
scenes the rule equals the host route exactly in every integer (the entries of every segment, hard false negatives, flags,
tp / fp / fn), exactly in precision, recall, steps and the NaN pattern, and in the AP within 4 n 2^-53 for a curve of n points:
any order of summing n non-negative products errs by at most gamma_n S with S <= recall[0] <= 1 (the steps telescope), two orders
differ by at most twice that, and the second factor 2 covers the roundings of the steps and gamma's denominator.  CPU only."""
import os
import warnings

import numpy as np
import pytest

import _ap_rule as A
import _sweep_rule as W
from box2mask_amd import eval_metric

U = 2.0 ** -53


# ------------------------------------------------------------------------------------------------ the host route, instrumented
def host_route(scenes, sels):
    """evaluate_matches on the records of the selected rows.  Returns (ap (classes, overlaps), calls {(o, c): (y_true, y_score,
    hard_fn)} of _average_precision, curves): the entries and the hard false negatives are read where the host hands them over."""
    matches = {}
    for s, (sc, m) in enumerate(zip(scenes, sels)):
        rows = np.nonzero(m)[0]
        K = len(sc['label_id'])
        matches['s%d' % s] = eval_metric.assign_from_counts(
            's%d' % s, np.asarray(sc['label_id'], np.int64)[rows], np.asarray(sc['conf'])[rows], np.asarray(sc['uniq'], np.int64),
            np.asarray(sc['gt_vert'], np.int64), np.asarray(sc['inter'], np.int64).reshape(K, len(sc['uniq']))[rows])
    calls, real = [], eval_metric._average_precision

    def spy(y_true, y_score, hard):
        calls.append((y_true.copy(), y_score.copy(), hard))
        return real(y_true, y_score, hard)
    eval_metric._average_precision = spy
    try:
        ap, curves = eval_metric.evaluate_matches(matches)
    finally:
        eval_metric._average_precision = real
    it = iter(calls)
    by_seg = {}
    for o in range(A.NO):                                       # the loop nest of evaluate_matches: overlaps, then classes
        for c in range(A.NC):
            if not np.isnan(ap[0, c, o]) and eval_metric.CLASS_LABELS[c] in curves[eval_metric.OVERLAPS[o]]:
                by_seg[(o, c)] = next(it)
    assert next(it, None) is None
    return ap[0], by_seg, curves


def host_counts(y_true, y_score, hard):
    """tp, fp, fn per distinct score as _average_precision forms them."""
    order = np.argsort(y_score)
    score, true = y_score[order], y_true[order]
    below = np.append(np.cumsum(true), 0)
    _, first = np.unique(score, return_index=True)
    n_true = below[-2] if len(score) else 0
    tp = np.array([n_true - below[i - 1] for i in first])
    fp = np.array([len(score) - i for i in first]) - tp
    fn = np.array([below[i - 1] + hard for i in first])
    return tp.astype(np.int64), fp.astype(np.int64), fn.astype(np.int64)


def differences(scenes, sels, mistake=None):
    """Where the rule (or a mistaken variant) leaves the host route, for ONE setting over `scenes`."""
    rule = A.Rule(1, mistake)
    rule.add(scenes, [sels])
    ap_h, segs, curves = host_route(scenes, sels)
    ap_r = rule.finish()[0]
    out = []
    if not np.array_equal(np.isnan(ap_h), np.isnan(ap_r)):
        out.append('nan pattern')
    for c in range(A.NC):
        has_curve = any((o, c) in segs for o in range(A.NO))
        if (rule.flags[0, c] == 3) != has_curve or (bool(rule.flags[0, c] & 1) != (not np.isnan(ap_h[c, 0]))):
            out.append(('flags', c))
            continue
        for o in range(A.NO):
            if (o, c) not in segs:
                if not has_curve and not np.isnan(ap_h[c, o]) and ap_r[c, o] != 0.0:
                    out.append(('zero', o, c))
                continue
            y_true, y_score, hard = segs[(o, c)]
            sc, tr = rule.segment(0, o, c)
            order = np.lexsort((y_true, y_score))
            if hard != rule.hard[0, o, c]:
                out.append(('hard', o, c))
            if not (np.array_equal(sc.astype(np.float64), y_score[order]) and np.array_equal(tr, y_true[order].astype(np.int64))):
                out.append(('entries', o, c))
                continue
            cv = rule.curve(0, o, c)
            tp, fp, fn = host_counts(y_true, y_score, hard)
            if not (np.array_equal(tp, cv['tp']) and np.array_equal(fp, cv['fp']) and np.array_equal(fn, cv['fn'])):
                out.append(('counts', o, c))
                continue
            h = curves[eval_metric.OVERLAPS[o]][eval_metric.CLASS_LABELS[c]]
            if not (np.array_equal(h['p'], cv['precision']) and np.array_equal(h['r'], cv['recall']) and
                    np.array_equal(h['rstep'], cv['steps'])):
                out.append(('curve', o, c))
            if not abs(ap_h[c, o] - ap_r[c, o]) <= 4 * len(cv['precision']) * U:
                out.append(('ap', o, c, ap_h[c, o], ap_r[c, o]))
    return out


def all_rows(scenes):
    return [np.ones(len(sc['label_id']), bool) for sc in scenes]


# ------------------------------------------------------------------------------------------------ the fixtures
@pytest.fixture(scope='module')
def golden(golden_dir):
    """(fixture, grid, [SweepTables per scene]) rebuilt as tests/test_param_sweep_rule.py rebuilds them."""
    d = np.load(os.path.join(golden_dir, 'param_sweep.npz'))
    grid = W.fixture_grid(d)
    return d, grid, [W.shared_tables(s, grid)[0] for s in W.fixture_scenes(d)]


def stage_scenes(tabs, ci, bi):
    return [dict(inter=t.stages[ci][bi]['inter'], label_id=t.stages[ci][bi]['label_id'],
                 conf=t.clusters[ci]['conf'][:len(t.stages[ci][bi]['label_id'])].astype(np.float32), uniq=t.uniq, gt_vert=t.gt_vert)
            for t in tabs]


def setting_masks(tabs, st):
    ci, si, bi, mi = st
    out = []
    for t in tabs:
        keep = t.stages[ci][bi]['keep'][mi]
        out.append(keep & (np.arange(len(keep)) < int(t.clusters[ci]['ks'][si])))
    return out


def random_scenes(seed):
    rng = np.random.default_rng(seed)
    return [A.random_scene(rng, int(rng.integers(0, 40)), int(rng.integers(1, 12))) for _ in range(4)]


RANDOM_SEEDS = (1, 2, 3, 4, 5)


# ------------------------------------------------------------------------------------------------ the rule is the host route
def test_rule_equals_the_host_route_on_the_golden_settings(golden):
    d, grid, tabs = golden
    n_curves = 0
    for st in grid.settings():
        scenes, sels = stage_scenes(tabs, st[0], st[2]), setting_masks(tabs, st)
        assert differences(scenes, sels) == [], st
        n_curves += 1
    assert n_curves == 36


def test_rule_equals_the_host_route_on_the_edges():
    scenes = A.edge_scenes()
    assert differences(scenes, all_rows(scenes)) == []
    for sc in scenes:                                           # ... and scene by scene: a scene's classes alone
        assert differences([sc], all_rows([sc])) == []


@pytest.mark.parametrize('seed', RANDOM_SEEDS)
def test_rule_equals_the_host_route_on_random_records(seed):
    scenes = random_scenes(seed)
    rng = np.random.default_rng(100 + seed)
    assert differences(scenes, all_rows(scenes)) == []
    sels = [rng.random(len(sc['label_id'])) < 0.6 for sc in scenes]
    assert differences(scenes, sels) == []


def test_random_records_hold_the_edges():
    """The seeded scenes do reach the cases they are there for."""
    seen = dict(second=0, small_gt=0, low_id=0, bad_label=0, ties=0, hard=0)
    for seed in RANDOM_SEEDS:
        scenes = random_scenes(seed)
        rule = A.Rule(1)
        rule.add(scenes)
        for sc in scenes:
            seen['small_gt'] += int(((np.asarray(sc['gt_vert']) < 100) & (sc['uniq'] >= 1000)).sum())
            seen['low_id'] += int((sc['uniq'] < 1000).sum())
            seen['bad_label'] += int((A.class_index(sc['label_id']) < 0).sum())
        for (sid, o, c), v in rule.entries.items():
            s = [a for a, _ in v]
            seen['ties'] += len(s) != len(set(s))
            seen['second'] += sum(1 for _, t in v if t == 0) > 0 and sum(1 for _, t in v if t == 1) > 0
        seen['hard'] += int(rule.hard.sum())
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize('mistake', A.MISTAKES)
def test_the_cases_catch_the_mistake(mistake):
    """Each mistaken variant of the rule leaves the host route on the hand-built scenes."""
    scenes = A.edge_scenes()
    assert differences(scenes, all_rows(scenes), mistake), mistake


# ------------------------------------------------------------------------------------------------ the averages and the winner
def test_averages_and_winner_on_the_golden_settings(golden):
    d, grid, tabs = golden
    settings = list(grid.settings())
    rule = A.Rule(len(settings))
    for q, st in enumerate(settings):
        rule.add(stage_scenes(tabs, st[0], st[2]), [setting_masks(tabs, st)], [q])
    table = rule.finish()
    n_max = max(len(rule.curve(q, o, c)['precision']) for q in range(len(settings)) for o in range(A.NO) for c in range(A.NC)
                if rule.flags[q, c] == 3)
    bound = 4 * n_max * U + 2.0 ** -50
    got = np.zeros((len(settings), 3))
    for q in range(len(settings)):
        want_ap = d['sw_q%02d_ap' % q][0]
        assert np.array_equal(np.isnan(table[q]), np.isnan(want_ap))
        assert np.nanmax(np.abs(table[q] - want_ap), initial=0.0) <= 4 * n_max * U
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            avg = eval_metric.compute_averages(table[q][None])
        got[q] = (avg['all_ap'], avg['all_ap_50%'], avg['all_ap_25%'])
        assert np.all(np.abs(got[q] - d['sw_q%02d_avg' % q]) <= bound), q
    want = np.stack([d['sw_q%02d_avg' % q] for q in range(len(settings))])
    # the winner by (AP50, AP, grid order): told apart by more than the bound, or tied exactly in both tables
    rank = lambda t: sorted(range(len(settings)), key=lambda q: (-t[q, 1], -t[q, 0], q))
    first, second = rank(want)[:2]
    margin = (want[first, 1] - want[second, 1], want[first, 0] - want[second, 0])
    assert margin[0] > 2 * bound or (margin[0] == 0.0 and (margin[1] > 2 * bound or margin[1] == 0.0)), margin
    assert rank(got)[0] == first


# ------------------------------------------------------------------------------------------------ the entries' argument checks
def test_ap_entries_check_their_arguments_on_the_host():
    """Negative return and b2m_last_error before anything touches a device (the convention of include/b2m.h)."""
    from box2mask_amd import _lib
    lib = _lib.load()
    err = lambda: lib.b2m_last_error().decode()
    ths = np.ascontiguousarray(eval_metric.OVERLAPS, np.float64)
    p = ths.ctypes.data
    assert lib.b2m_ap_rows(None, 70000, 1, None) < 0 and 'sizes' in err()
    assert lib.b2m_ap_rows(None, 1, 1, None) < 0 and 'NULL' in err()
    assert lib.b2m_ap_rows(None, 0, 0, None) == 0 and lib.b2m_ap_rows(None, 3, 0, None) == 0      # no scene, no row: no launch
    match = lambda n_scenes, n_set, th, n_settings: lib.b2m_ap_match(None, n_scenes, 0, None, None, None, n_set, None, 0, th, None, None, 0,
                                                                     None, None, None, n_settings, None)
    assert match(1, 1, p, 0) < 0 and 'n_settings' in err()
    assert match(1, 1, p, (1 << 20) + 1) < 0 and 'n_settings' in err()
    assert match(-1, 1, p, 1) < 0 and 'sizes' in err()
    assert match(1, 1, None, 1) < 0 and 'ths_host' in err()
    assert match(1, 1, p, 1) < 0 and 'NULL' in err()
    bad = ths.copy()
    bad[3] = 1.0
    assert match(1, 1, bad.ctypes.data, 1) < 0 and ('NULL' in err() or 'overlap' in err())
    assert match(0, 1, p, 1) == 0 and match(1, 0, p, 1) == 0
    curve = lambda n_keys, n_settings, seg, cap: lib.b2m_ap_curve(None, n_keys, None, None, n_settings, None, seg, cap, None, None, None, None)
    assert curve(0, 0, -1, 0) < 0 and 'n_settings' in err()
    assert curve(-1, 1, -1, 0) < 0 and 'sizes' in err()
    assert curve(0, 1, -1, 0) < 0 and 'NULL' in err()
