"""CPU: the over-segmentation rule (tests/_overseg_rule.py) against the reference's recorded `segIndices`
(tests/golden/overseg.npz, tools/gen_golden_overseg.py), and the cases of tests/_overseg_cases.py against what they claim to reach.

The reference's std::sort leaves tied weights in an unspecified order, so it pins the PARTITION (compared after relabelling by first
occurrence) and not the ids; the goldens are meshes whose partition does not depend on that order, which is checked again here."""
import json

import numpy as np
import pytest

import _overseg_cases as C
import _overseg_rule as R

GOLDEN = sorted(C.golden())


def test_goldens_cover_the_issue_cases():
    g = C.golden()
    assert {v['k'] for v in g.values()} >= {0.01, 0.05, 0.5} and {v['m'] for v in g.values()} >= {1, 20, 50}
    kinds = {n.split('_', 1)[1] for n in g}
    assert kinds >= {'field40', 'field30', 'unused', 'repeated', 'sheets'}
    for name, v in g.items():
        assert len(v['pos']) <= 1600 and v['pos'].dtype == np.float32
        assert v['ties'] == R.n_ties(C.golden_rule(name)['w']) > 1000, name
    v = g[[n for n in g if n.endswith('unused')][0]]
    assert len(np.setdiff1d(np.arange(len(v['pos'])), v['faces'])) == 60
    v = g[[n for n in g if n.endswith('repeated')][0]]
    assert len(np.unique(v['faces'], axis=0)) == len(v['faces']) - 3


@pytest.mark.parametrize('name', GOLDEN)
def test_rule_partition_equals_reference(name):
    g, r = C.golden()[name], C.golden_rule(name)
    assert np.isfinite(r['w']).all()
    assert np.array_equal(R.relabel(r['seg']), R.relabel(g['ref'])), name
    # ids are roots: every label is a member of its own segment
    assert np.array_equal(r['seg'][r['seg']], r['seg']) and np.array_equal(g['ref'][g['ref']], g['ref'])
    # unnamed vertices keep a zero normal and stay alone
    loose = np.setdiff1d(np.arange(len(g['pos'])), g['faces'])
    assert not r['normals'][loose].any() and np.array_equal(r['seg'][loose], loose)


@pytest.mark.parametrize('name', GOLDEN)
def test_partition_does_not_depend_on_tie_order(name):
    g, r = C.golden()[name], C.golden_rule(name)
    want = R.relabel(g['ref'])
    for p in range(3):
        seg = R.segment(g['pos'], g['faces'], g['k'], g['m'], rng=np.random.default_rng(1000 + p))[0]
        assert np.array_equal(R.relabel(seg), want), (name, p)


def test_keys_order_is_the_w_e_order():
    for name in GOLDEN[:2] + ['nan']:
        w = C.golden_rule(name)['w'] if name != 'nan' else C.graph_case(name)[2]
        keys = R.sort_keys(w)
        assert len(np.unique(keys)) == len(keys) and keys.max() < np.uint64(2 ** 64 - 1)
        assert np.array_equal(np.argsort(keys, kind='stable'), R.edge_order(w)), name
    w = C.graph_case('nan')[2]
    assert R.edge_order(w).tolist() == [1, 2, 4, 3, 0]                # -0 == +0 by index, then +inf, the NaN last


@pytest.mark.parametrize('name', C.MESH_ORDER + C.GRAPH_ORDER)
def test_case_reaches_what_it_claims(name):
    assert C.reach(name) is None, (name, C.reach(name))


# each deliberate mistake, and the named case that fails under it
CAUGHT_BY = {'strict_thr': 'thr_equal', 'le_m': 'sizes_m', 'pass2_unsorted': 'pass2_order', 'thr_size_before': 'thr_ulp_above',
             'no_square': 'm00_field40', 'dot2_na': 'm00_field40', 'slot_i2i3': 'm00_field40'}


@pytest.mark.parametrize('mistake', R.MISTAKES)
def test_every_deliberate_mistake_is_caught(mistake):
    case = CAUGHT_BY[mistake]
    if case in C.GRAPH_ORDER:
        a, b, w, n, k, m = C.graph_case(case)
        wrong = R.graph_segment(a, b, w, n, k, m, mistake=mistake)
        assert not np.array_equal(R.relabel(wrong), R.relabel(C.graph_rule(case)['seg'])), (mistake, case)
    else:
        g = C.golden()[case]
        wrong = R.segment(g['pos'], g['faces'], g['k'], g['m'], mistake=mistake)[0]
        assert not np.array_equal(R.relabel(wrong), R.relabel(g['ref'])), (mistake, case)
    assert set(CAUGHT_BY) == set(R.MISTAKES) and len(R.MISTAKES) == 7


def test_segs_json_layout_and_no_cpu_path():
    import torch
    from box2mask_amd import _lib, oversegment
    doc = json.loads(oversegment.segs_json(np.array([2, 2, 2, 5, 5, 5]), 'scene0707_00', 0.01, 20))
    assert doc == {'params': {'kThresh': 0.01, 'segMinVerts': 20}, 'sceneId': 'scene0707_00', 'segIndices': [2, 2, 2, 5, 5, 5]}
    assert oversegment.segs_json([0], 'x', 0.5, 1).startswith('{"params":{"kThresh":0.5,"segMinVerts":1},"sceneId":"x",')
    if not torch.cuda.is_available():
        pos, faces, _, _ = C.mesh_case('strip:1')
        with pytest.raises(_lib.B2MError):
            oversegment.segment_mesh(pos, faces)
        with pytest.raises(_lib.B2MError):
            oversegment.graph_segment([0], [1], [0.0], 2)
