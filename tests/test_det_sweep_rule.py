"""The rule of the threshold sweep scored with the ARKitScenes detection mAP (tests/_det_sweep_rule.py) against the real reference:
for all 36 settings of tests/golden/arkit_sweep.npz and the case off the grid, composing the rows of a setting from the tables the
settings share, gating them at 50 POINTS after the mask NMS and matching them as eval_det does reproduces what
SelectionNet.detection2mask + Evaluater.arkitscenes_eval returned setting by setting -- the scored rows and the point counts of the
kept rows exactly, the IoU tables within _detbox_rule.IOU_TOL, per-class AP and mAP bit for bit, for both ``oriented_boxes`` values
and both thresholds.  Every stated mistake leaves the fixture at a named setting.  CPU only."""
import os

import numpy as np
import pytest

import _det_sweep_rule as A
import _sweep_rule as W
from box2mask_amd import eval_detection, param_search


@pytest.fixture(scope='module')
def fx(golden_dir):
    sw = np.load(os.path.join(golden_dir, 'param_sweep.npz'))
    ak = np.load(os.path.join(golden_dir, 'arkit_sweep.npz'))
    return sw, ak, W.fixture_grid(sw), {}


def tables(fx, oriented=True, mistake=None, gate=False, sub=None):
    """(grid, per scene (DetectionTables, aux), [(fixture tag, setting)]) of the whole grid, of the sub-grid ``sub`` (per axis the
    indices it keeps) or, gate=True, of the one setting of the case off the grid."""
    sw, ak, grid, cache = fx
    if gate:
        sub = tuple([int(i)] for i in ak['ak_gate_setting'])
    sub = sub or tuple(list(range(n)) for n in grid.shape)
    key = (oriented, None if mistake == 'gate_before_nms' else mistake, gate, repr(sub))
    if key not in cache:
        g = param_search.ThresholdGrid(*(getattr(grid, a)[idx] for a, idx in zip(param_search.AXES, sub)))
        cache[key] = (g, [A.stage_tables(scene, pos, lab, g, oriented, mistake=key[1]) for scene, pos, lab in A.fixture_inputs(sw, ak, gate)])
    g, tabs = cache[key]
    tags = [('gate' if gate else 'q%02d' % np.ravel_multi_index(tuple(idx[i] for idx, i in zip(sub, st)), grid.shape), st)
            for st in g.settings()]
    return g, tabs, tags


def first_miss(fx, oriented=True, mistake=None, gate=False, sub=None, also_product=False):
    """The first setting at which the rule -- or a mistaken variant of it -- leaves the fixture, as the assertion's arguments."""
    ak = fx[1]
    grid, tabs, tags = tables(fx, oriented, mistake, gate, sub)
    vt = 'obb' if oriented else 'aabb'
    for tag, st in tags:
        recs, counts = {}, []
        for t, aux in tabs:
            recs[t.name] = A.records(t, aux, grid, *st, mistake=mistake)
            counts.append(t.stages[st[0]][st[2]]['count'][W.compose(t, *st)])
            if also_product:                                                # the product's composition on the rule's tables
                got = param_search.detection_records(t, *st)
                assert all(np.array_equal(got[k], recs[t.name][k]) and got[k].dtype == recs[t.name][k].dtype for k in got), (tag, t.name)
        try:
            A.check_setting(ak, tag, recs, vt, counts=None if mistake == 'gate_before_nms' else counts)
        except AssertionError as e:
            return e.args[0] if e.args else (tag,)
    return None


@pytest.mark.parametrize('oriented', [True, False])
def test_rule_reproduces_every_setting_of_the_reference(fx, oriented):
    assert first_miss(fx, oriented, also_product=True) is None
    assert first_miss(fx, oriented, gate=True, also_product=True) is None


def test_product_matching_equals_the_restated_matching(fx):
    """eval_detection.eval_det on the product's records: the same classes, APs and mAP as the fixture, bit for bit."""
    ak = fx[1]
    grid, tabs, tags = tables(fx, True)
    for tag, st in tags[::5]:
        recs = {t.name: param_search.detection_records(t, *st) for t, _ in tabs}
        for th in A.THRESHOLDS:
            key = 'ak_%s_obb_%d_' % (tag, round(th * 100))
            ap = eval_detection.eval_det(recs, ovthresh=th)[2]
            assert [int(c) for c in ap] == ak[key + 'classes'].tolist()
            assert A.same_floats([ap[c] for c in ap], ak[key + 'ap']) and A.same_floats(eval_detection.mean_ap(ap), ak[key + 'map'])


def test_fixture_is_not_flat(fx):
    """What tools/gen_golden_arkit_sweep.py asserted before it wrote the file, seen from here."""
    sw, ak, grid, _ = fx
    scored = np.array([[ak['ak_q%02d_s%d_iou_obb' % (q, s)].shape[0] for s in range(2)] for q in range(36)]).reshape(grid.shape + (2,))
    assert all((np.diff(scored, axis=a) != 0).any() for a in range(4))
    counts = np.concatenate([ak['ak_q%02d_s%d_count' % (q, s)] for q in range(36) for s in range(2)])
    assert (counts < A.MIN_POINTS).sum() > 0 and not (counts == A.MIN_POINTS).any()          # (hence the case off the grid)
    assert (ak['ak_gate_s0_count'] == A.MIN_POINTS).sum() == 1
    assert len({float(ak['ak_q%02d_%s_%d_map' % (q, vt, t)]) for q in range(36) for vt in ('obb', 'aabb') for t in (50, 25)}) >= 8
    gcls = set(np.concatenate([ak['ak_s%d_per_instance_semantics' % s] for s in range(2)]).tolist())
    pcls = set(ak['ak_q00_obb_50_classes'].tolist())                        # (eval_det lists the classes of both)
    scored_cls = {int(c) for c, v in zip(ak['ak_q00_obb_50_classes'], ak['ak_q00_obb_50_ap'])}
    assert gcls - scored_cls and np.isnan(ak['ak_q00_obb_50_ap']).any() and pcls
    assert any((ak['ak_s%d_per_instance_bb_rotations' % s][:, 1] != 0).any() for s in range(2))


# the named setting each mistake fails (the sub-grid that holds it), and what differs there
ONE = ([0], [0], [0], [0])
CAUGHT = {
    'count_on_voxels': (dict(sub=ONE), ('q00', 0, 'count')),
    'gt_min_points': (dict(gate=True), ('gate', 0, 'scored rows')),         # the row of exactly 50 points
    'iou_of_other_stage': (dict(sub=([0], [0], [0, 1], [0])), ('q00', 0, 'iou')),
    'rotation_not_transposed': (dict(sub=ONE), ('q00', 0, 'iou')),
    'no_class_gate': (dict(sub=ONE), ('q00', 0, 'iou')),
    'gate_before_nms': (dict(gate=True), ('gate', 0, 'scored rows')),       # the thinned row that suppresses a larger one
}


@pytest.mark.parametrize('mistake', A.MISTAKES)
def test_each_mistake_leaves_the_fixture(fx, mistake):
    kw, where = CAUGHT[mistake]
    assert first_miss(fx, mistake=None, **kw) is None                       # the same tables without the mistake: no miss
    miss = first_miss(fx, mistake=mistake, **kw)
    assert miss is not None and tuple(miss[:3]) == where, (mistake, miss)


def test_argument_checks_on_the_host():
    from box2mask_amd import _lib
    lib = _lib.load()
    err = lambda: lib.b2m_last_error().decode()
    p = 64                                                                   # a non-NULL address that is never dereferenced
    single = lambda bits=p, words=1, k=1, n_vox=64, pos=p, n_pts=64, pbits=p, cap=64, flags=p: lib.b2m_mask_hulls_index(
        bits, words, k, n_vox, None, pos, n_pts, pbits, p, p, p, cap, p, p, p, p, p, flags, None)
    assert single(k=-1) < 0 and 'bad sizes' in err()
    assert single(k=65536) < 0 and 'bad sizes' in err()
    assert single(n_pts=1 << 31) < 0 and 'bad sizes' in err()
    assert single(words=2) < 0 and 'words' in err()
    assert single(n_vox=65) < 0 and 'words' in err()
    assert single(cap=63) < 0 and 'cap' in err()
    assert single(cap=96) < 0 and 'cap' in err()
    assert single(flags=None) < 0 and 'NULL' in err()
    assert single(bits=None) < 0 and 'NULL' in err()
    assert single(pos=None) < 0 and 'NULL' in err()
    assert single(pbits=None) < 0 and 'NULL' in err()
    assert single(k=0, bits=None, pos=None, pbits=None, flags=None) == 0     # nothing to do: nothing is looked at
    batch = lambda desc=p, n=1, cap=64, max_k=1, max_pts=64: lib.b2m_mask_hulls_index_batch(desc, n, cap, max_k, max_pts, None)
    assert batch(n=-1) < 0 and 'bad sizes' in err()
    assert batch(max_k=65536) < 0 and 'bad sizes' in err()
    assert batch(max_pts=1 << 31) < 0 and 'bad sizes' in err()
    assert batch(cap=100) < 0 and 'cap' in err()
    assert batch(desc=None) < 0 and 'NULL' in err()
    assert batch(desc=None, n=0) == 0 and batch(desc=None, max_k=0) == 0
    # the host entries
    grid = param_search.ThresholdGrid([0.5], [0.05], [0.3], [0.6])
    t = param_search.DetectionTables('s', 4, np.array([5], np.int32), 50)
    t.clusters.append(dict(K=3, conf=np.array([0.9, 0.8, 0.7], np.float32), reps=np.arange(3), ks=np.array([2])))
    t.stages.append([dict(label_id=np.array([5, 5, 7], np.int32), keep=np.array([[True, True, True]]), count=np.array([49, 50, 90]),
                          iou=np.array([[0.0], [0.6], [0.0]]))])
    r = param_search.detection_records(t, 0, 0, 0, 0)                        # the prefix of 2, then the gate: row 1 alone
    assert r['label'].tolist() == [5] and r['conf'].tolist() == [np.float32(0.8)] and r['iou'].tolist() == [[0.6]] and r['gt_label'] is t.gt_label
    with pytest.raises(ValueError, match='iou_t'):
        param_search.arkit_param_search(None, [], grid, iou_t=[])
    res = param_search.arkit_param_search(None, [], grid, iou_t=[0.5, 0.25])  # no batch at all: nothing is scored
    assert res['map'].shape == (1, 1, 1, 1, 2) and np.isnan(res['map']).all() and res['best'] == (0, 0, 0, 0)
