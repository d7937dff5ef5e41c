"""GPU: the ScanNet AP on the device (box2mask_amd/eval_match.py, csrc/apmatch.hip).

  * MatchAccumulator against the rule in numpy (tests/_ap_rule.py), bit for bit -- the sorted entries, hard false negatives, flags,
    tp / fp / fn, precision, recall, steps and the AP -- on hand-built and seeded records, the same bits on a second run;
  * the whole sweep with matching='device' against tests/golden/param_sweep.npz and against matching='host' in the same process,
    and compute_eval_device against eval_metric.compute_eval, within 4 n 2^-53 (n = the curve's length; tests/test_ap_rule.py
    derives the bound);
  * the refusals."""
import os
import warnings

import numpy as np
import pytest
import torch

import _ap_rule as A
import _sweep_rule as W

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


def _score_key(conf):
    u = (np.asarray(conf, np.float32) + np.float32(0)).view(np.uint32).astype(np.uint64)
    return np.where(u >> np.uint64(31) != 0, ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))


def _rule_keys(rule):
    out = []
    for (sid, o, c), v in rule.entries.items():
        if v:
            seg = np.uint64(sid * 180 + o * 18 + c)
            out.append((seg << np.uint64(33)) | (_score_key([a for a, _ in v]) << np.uint64(1)) | np.array([t for _, t in v], np.uint64))
    return np.sort(np.concatenate(out)) if out else np.zeros(0, np.uint64)


def _masks(scenes, prefix, keep):
    """sels[j][s] of a call: the prefix and the keep row of setting j."""
    out = []
    for j in range(prefix.shape[1]):
        row, o = [], 0
        for s, sc in enumerate(scenes):
            K = len(sc['label_id'])
            m = np.arange(K) < prefix[s, j]
            row.append(m & keep[j, o:o + K] if keep is not None else m)
            o += K
        out.append(row)
    return out


def _run_device(calls, n_settings, debug=None):
    """calls: [(scenes, set_id, prefix (S, n_set), keep (n_set, total K) bool or None)].  Returns the accumulator's results."""
    from box2mask_amd import eval_match
    acc = eval_match.MatchAccumulator(n_settings)
    for scenes, set_id, prefix, keep in calls:
        dev_scenes = [dict(inter=torch.from_numpy(np.ascontiguousarray(sc['inter'], np.int32).reshape(len(sc['label_id']), len(sc['uniq']))).cuda(),
                           label_id=torch.from_numpy(np.asarray(sc['label_id'], np.int32)).cuda(),
                           conf=torch.from_numpy(np.asarray(sc['conf'])).cuda(), uniq=sc['uniq'], gt_vert=sc['gt_vert']) for sc in scenes]
        if keep is None:
            acc.add(dev_scenes, set_id, prefix)
        else:
            acc.add(dev_scenes, set_id, prefix, torch.from_numpy(np.ascontiguousarray(keep, np.int32)).cuda(), list(range(len(set_id))))
    table = acc.finish()
    keys = acc._sorted[:acc.n_entries].cpu().numpy().view(np.uint64)
    curves = {seg: acc.finish(seg, cap)[1] for seg, cap in (debug or {}).items()}
    return dict(table=table, keys=keys, hard=acc.hard_fn.cpu().numpy().reshape(n_settings, A.NO, A.NC),
                flags=acc.flags.cpu().numpy().reshape(n_settings, A.NC), curves=curves, acc=acc)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                                 b.view(np.uint64) if b.dtype == np.float64 else b)


def _check(calls, n_settings, all_curves=True):
    """Device against rule, bit for bit, and the device against itself."""
    rule = A.Rule(n_settings)
    for scenes, set_id, prefix, keep in calls:
        rule.add(scenes, _masks(scenes, prefix, keep), list(set_id))
    want = rule.finish()
    debug = {}
    for sid in range(n_settings):
        for o in range(A.NO):
            for c in range(A.NC):
                if rule.flags[sid, c] == 3 and (all_curves or (o in (0, 9) and sid < 2)):
                    debug[(sid, o, c)] = len(rule.curve(sid, o, c)['precision'])
    got = _run_device(calls, n_settings, debug)
    assert np.array_equal(got['flags'], rule.flags)
    assert np.array_equal(got['hard'], rule.hard)
    assert np.array_equal(got['keys'], _rule_keys(rule))
    assert np.array_equal(np.isnan(got['table']), np.isnan(want))
    assert _same(np.nan_to_num(got['table'], nan=-1.0), np.nan_to_num(want, nan=-1.0))
    for seg, cv in got['curves'].items():
        ref = rule.curve(*seg)
        for name in ('tp', 'fp', 'fn', 'precision', 'recall', 'steps'):
            assert _same(cv[name], ref[name]), (seg, name)
    again = _run_device(calls, n_settings)
    assert np.array_equal(again['keys'], got['keys']) and _same(np.nan_to_num(again['table'], nan=-1.0), np.nan_to_num(got['table'], nan=-1.0))
    assert np.array_equal(again['hard'], got['hard']) and np.array_equal(again['flags'], got['flags'])
    return rule, got


def _one(scenes):
    """A plain evaluation: one setting that keeps every row."""
    return [(scenes, [0], np.array([[len(sc['label_id'])] for sc in scenes], np.int64).reshape(len(scenes), 1), None)]


# ----------------------------------------------------------------------------- hand-built records
def test_edge_scenes_bit_for_bit():
    scenes = A.edge_scenes()
    rule, got = _check(_one(scenes), 1)
    t = got['table'][0]
    c11, c12 = int(np.nonzero(A.VALID == 11)[0][0]), int(np.nonzero(A.VALID == 12)[0][0])
    assert (t[c11] == 0.0).all() and np.isnan(t[c12]).all()                 # ground truth without a row; rows without ground truth
    assert np.isnan(t[A.NC - 1]).all() and rule.flags[0, A.NC - 1] == 0      # neither
    assert (rule.flags[0] == 3).sum() >= 8


def test_edge_scenes_one_by_one():
    for sc in A.edge_scenes():
        _check(_one([sc]), 1)


def test_no_row_and_only_id_zero():
    empty = A.scene({0: 500, 3001: 200}, [])
    only0 = A.scene({0: 700}, [(3, .9, {0: 300}), (4, .5, {0: 100})])
    rule, got = _check(_one([empty, only0]), 1)
    assert got['acc'].n_entries == 0 and rule.hard[0, :, 0].tolist() == [1] * A.NO
    _check(_one([empty]), 1)
    _check(_one([only0]), 1)


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 1025])
def test_segment_lengths(n):
    """Segments of n false positives, and of up to 65 entries with true ones among them, in neighbouring classes: the ranges of the
    sorted entries, the sort's padding and the ties."""
    fp = A.false_positive_scene(n, cls=16)
    rng = np.random.default_rng(n)
    gts = {0: 500}
    rows = []
    for i in range(min(n, 65)):                                          # class 14: a ground truth per row, matched or missed
        gts[14001 + i] = 200
        rows.append((14, float(rng.choice(np.linspace(0.1, 0.9, 9))), {14001 + i: int(rng.choice([40, 120, 200])), 0: 100}))
    rule, got = _check(_one([fp, A.scene(gts, rows)]), 1, all_curves=False)
    c16 = int(np.nonzero(A.VALID == 16)[0][0])
    assert all(len(rule.segment(0, o, c16)[0]) == n for o in range(A.NO))


# ----------------------------------------------------------------------------- seeded records, settings, batches
def _random_call(rng, n_set, set_id, n_scenes=3, empty_at=None):
    scenes = [A.random_scene(rng, 0 if s == empty_at else int(rng.integers(1, 30)), int(rng.integers(1, 9))) for s in range(n_scenes)]
    ks = np.array([len(sc['label_id']) for sc in scenes])
    prefix = rng.integers(0, ks[:, None] + 1, (n_scenes, n_set))
    prefix[:, 0] = ks                                                    # prefix K ...
    if n_set > 1:
        prefix[:, 1] = 0                                                 # ... and 0
    keep = rng.random((n_set, int(ks.sum()))) < 0.7
    return scenes, list(set_id), prefix.astype(np.int64), keep


@pytest.mark.parametrize('n_set', [1, 2, 65])
def test_settings_prefixes_and_batches(n_set):
    """Three add calls (batches) into the same settings, an empty scene among them; the settings of a call in shuffled order."""
    rng = np.random.default_rng(40 + n_set)
    calls = [_random_call(rng, n_set, rng.permutation(n_set), empty_at=1 if b == 1 else None) for b in range(3)]
    rule, got = _check(calls, n_set, all_curves=n_set < 65)
    assert (rule.flags == 3).any() and len(got['keys']) > 0


def test_settings_of_different_calls():
    """A sweep's stages: every call scores other settings of the table."""
    rng = np.random.default_rng(7)
    calls = [_random_call(rng, 2, [2 * b, 2 * b + 1]) for b in range(3)]
    calls.append((calls[0][0], [5], calls[0][2][:, :1], None))           # no keep table: the prefix alone
    _check(calls, 7)                                                     # (setting 6 is never scored: NaN everywhere)


def test_ids_at_the_cap():
    from box2mask_amd import eval_match
    gts = {0: 500}
    gts.update({3001 + i: 100 + (i % 7) for i in range(2047)})
    sc = A.scene(gts, [(3, .9, {3001: 100, 5047: 50}), (3, .8, {3002: 60, 0: 40})])
    assert len(sc['uniq']) == 2048
    _check(_one([sc]), 1, all_curves=False)
    gts[40000] = 100
    big = A.scene(gts, [(3, .9, {3001: 100})])
    with pytest.raises(ValueError, match='2048'):
        eval_match.MatchAccumulator(1).add([big])


# ----------------------------------------------------------------------------- refusals
def test_refusals():
    from box2mask_amd import eval_match
    sc = A.scene({0: 500, 3001: 200}, [(3, .9, {3001: 150}), (3, .8, {3001: 20, 0: 100})])
    ok = lambda **kw: dict(sc, **kw)
    acc = eval_match.MatchAccumulator(2)
    with pytest.raises(ValueError, match='float32'):
        acc.add([ok(conf=np.array([0.1, 0.8]))])                         # float64 values that no float32 holds
    with pytest.raises(ValueError, match='float32'):
        acc.add([ok(conf=np.array([1, 0]))])
    with pytest.raises(ValueError, match='inter'):
        acc.add([ok(inter=sc['inter'][:1])])
    with pytest.raises(ValueError, match='inter'):
        acc.add([ok(inter=sc['inter'][:, :1])])
    with pytest.raises(ValueError, match='scores'):
        acc.add([ok(conf=sc['conf'][:1])])
    with pytest.raises(ValueError, match='point counts'):
        acc.add([ok(gt_vert=sc['gt_vert'][:1])])
    with pytest.raises(ValueError, match='prefix'):
        acc.add([sc], [0, 1], [[2]])
    with pytest.raises(ValueError, match='prefix'):
        acc.add([sc], [0], [[3]])
    with pytest.raises(ValueError, match='set_id'):
        acc.add([sc], [2])
    with pytest.raises(ValueError, match='keep'):
        acc.add([sc], [0], None, None, [0])
    assert acc.n_entries == 0
    acc.add([ok(conf=np.array([0.5, 0.25]))])                            # float64 that IS float32: taken
    acc.finish()
    with pytest.raises(RuntimeError, match='finished'):
        acc.add([sc])


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


def _bound(model, batch, pred, grid, gts):
    """4 n 2^-53 for the longest curve these inputs can give: a row adds at most 3 entries to a segment (overlap 0.25), and the
    curve has one point more than its entries."""
    tabs = model.pred2mask_sweep(batch, pred, grid, gts)
    rows = max(sum(int(t.clusters[ci]['ks'][0]) for t in tabs) for ci in range(grid.shape[0]))
    return 4 * (3 * rows + 1) * U


def _close(a, b, bound):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and bool(np.all(np.abs(a - b)[~np.isnan(a)] <= bound))


def _sweep_both(model, fx, grid, tags):
    from box2mask_amd import param_search
    batch, pred, gts = W.fixture_batch(fx)
    bound = _bound(model, batch, pred, grid, gts)
    assert bound < 1e-11
    dev = param_search.scannet_param_search(model, [(batch, pred)], gts, grid, per_class=True, matching='device')
    host = param_search.scannet_param_search(model, [(batch, pred)], gts, grid, per_class=True, matching='host')
    assert dev['n_evaluated'] == len(tags) and dev['ap_tables'].shape == host['ap_tables'].shape
    for st, tag in tags.items():
        assert _close(dev['ap_tables'][st], fx['sw_%s_ap' % tag], bound), st
        assert _close(dev['ap'][st], fx['sw_%s_avg' % tag], bound + 2.0 ** -50), st
        assert _close(dev['ap_tables'][st], host['ap_tables'][st], bound), st
        assert _close(dev['ap'][st], host['ap'][st], bound + 2.0 ** -50), st
    return dev, host, bound


def test_device_sweep_reproduces_the_reference_and_the_host_route(model, fx):
    grid = W.fixture_grid(fx)
    dev, host, bound = _sweep_both(model, fx, grid, {st: 'q%02d' % q for q, st in enumerate(grid.settings())})
    assert dev['best'] == host['best'] and dev['best_ths'] == host['best_ths']
    assert len({tuple(v) for v in dev['ap'].reshape(-1, 3).tolist()}) >= 8       # the settings are told apart


def test_device_sweep_score_threshold_equal_to_a_score(model, fx):
    from box2mask_amd import param_search
    grid = param_search.ThresholdGrid(*([v] for v in fx['sw_tie_ths']))
    dev, host, _ = _sweep_both(model, fx, grid, {(0, 0, 0, 0): 'tie'})
    assert dev['best'] == host['best'] == (0, 0, 0, 0)


def test_device_sweep_over_two_batches_and_a_setting_without_rows(model, fx):
    """The same batch twice is two batches of scenes; score_th 1.5 keeps no cluster."""
    from box2mask_amd import param_search
    batch, pred, gts = W.fixture_batch(fx)
    grid = param_search.ThresholdGrid([0.5], [0.05, 1.5], [0.3], [0.6])
    other = {'scene': [{'name': s['name'] + '_b'} for s in batch['scene']]}
    batch2 = dict(batch, **other)
    gts2 = dict(gts, **{s['name'] + '_b': gts[s['name']] for s in batch['scene']})
    bound = _bound(model, batch, pred, grid, gts) * 2
    dev = param_search.scannet_param_search(model, [(batch, pred), (batch2, pred)], gts2, grid, matching='device')
    host = param_search.scannet_param_search(model, [(batch, pred), (batch2, pred)], gts2, grid, matching='host')
    assert _close(dev['ap'], host['ap'], bound + 2.0 ** -50) and dev['best'] == host['best'] == (0, 0, 0, 0)
    assert dev['ap'][0, 1, 0, 0, 1] == 0.0
    with pytest.raises(ValueError, match='matching'):
        param_search.scannet_param_search(model, [(batch, pred)], gts, grid, matching='gpu')


def test_compute_eval_device_equals_compute_eval(model, fx):
    from box2mask_amd import eval_match, eval_metric
    batch, pred, gts = W.fixture_batch(fx)
    results = model.pred2mask(batch, pred, 'eval')
    rows = sum(int(r['mask'].shape[0]) for r in results.values())
    assert rows > 4
    bound = 4 * (3 * rows + 1) * U + 2.0 ** -50
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        want, _ = eval_metric.compute_eval(results, gts)
        got = eval_match.compute_eval_device(results, gts)
    assert set(got) == set(want) and set(got['classes']) == set(want['classes'])
    for k in ('all_ap', 'all_ap_50%', 'all_ap_25%'):
        assert _close(got[k], want[k], bound), k
    for name in want['classes']:
        for k in ('ap', 'ap50%', 'ap25%'):
            assert _close(got['classes'][name][k], want['classes'][name][k], bound), (name, k)
    assert want['all_ap_25%'] > 0
