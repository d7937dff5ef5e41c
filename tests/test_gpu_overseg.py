"""GPU: mesh over-segmentation (csrc/overseg.hip, box2mask_amd/oversegment.py) against the rule of tests/_overseg_rule.py -- normals,
weights and sort keys bit for bit, every segment id equal -- and against the reference's recorded partition on the golden meshes
(tests/golden/overseg.npz).  tests/test_overseg_rule.py shows on the CPU that the rule gives the reference's partition on those
meshes and that each case of tests/_overseg_cases.py reaches what it is there for."""
import numpy as np
import pytest
import torch

from box2mask_amd import _lib, oversegment as O

import _overseg_cases as C
import _overseg_rule as R

pytestmark = pytest.mark.gpu

GOLDEN = sorted(C.golden())


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what + ': NaN pattern'
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)) & ~nan)
    assert len(bad[0]) == 0, '%s: %d of %d differ, first at %s: got %r want %r' % (
        what, len(bad[0]), got.size, [int(b[0]) for b in bad], got[tuple(b[0] for b in bad)], want[tuple(b[0] for b in bad)])


def _mesh(name):
    if name in C.MESH_ORDER:
        pos, faces, k, m = C.mesh_case(name)
        return pos, faces, k, m, C.mesh_rule(name)
    g = C.golden()[name]
    return g['pos'], g['faces'], g['k'], g['m'], C.golden_rule(name)


FIRST_HALF = [n for n in C.MESH_ORDER if n != 'strip:0'] + GOLDEN


@pytest.mark.parametrize('name', FIRST_HALF)
def test_edge_weights_equal_the_rule_bit_for_bit(name):
    pos, faces, k, m, want = _mesh(name)
    normals, weights, keys, ea, eb = O.mesh_edge_weights(pos, faces)
    _same_bits(normals.cpu().numpy(), want['normals'], name + ' normals')
    _same_bits(weights.cpu().numpy(), want['w'], name + ' weights')
    assert np.array_equal(keys.cpu().numpy().view(np.uint64), want['keys']), name
    assert np.array_equal(ea.cpu().numpy(), want['a']) and np.array_equal(eb.cpu().numpy(), want['b']), name


@pytest.mark.parametrize('name', C.GRAPH_ORDER)
def test_graph_segment_equals_the_rule_on_hand_built_graphs(name):
    a, b, w, n, k, m = C.graph_case(name)
    seg, info = O.graph_segment(a, b, w, n, k, m, return_info=True)
    want = C.graph_rule(name)['seg']
    assert seg.dtype == torch.int64 and np.array_equal(seg.cpu().numpy(), want), (name, seg.cpu().numpy(), want)
    assert info['n_segments'] == len(np.unique(want)) and info['n_nan'] == int(np.isnan(w).sum())


@pytest.mark.parametrize('name', FIRST_HALF)
def test_graph_segment_equals_the_rule_on_mesh_graphs(name):
    """The second half alone, fed the RULE's edges and weights: its ids do not lean on the first half's kernels."""
    pos, faces, k, m, want = _mesh(name)
    seg = O.graph_segment(want['a'], want['b'], want['w'], len(pos), k, m)
    assert np.array_equal(seg.cpu().numpy(), want['seg']), name


@pytest.mark.parametrize('name', C.MESH_ORDER + GOLDEN)
def test_segment_mesh_equals_the_rule_ids(name):
    pos, faces, k, m, want = _mesh(name)
    seg, info = O.segment_mesh(pos, faces, k, m, return_info=True)
    got = seg.cpu().numpy()
    assert seg.dtype == torch.int64 and seg.is_cuda and np.array_equal(got, want['seg']), name
    assert info['n_segments'] == len(np.unique(want['seg'])) and info['n_nan'] == int(np.isnan(want['w']).sum()), name
    _same_bits(info['normals'].cpu().numpy(), want['normals'], name + ' normals')
    if name in GOLDEN:
        assert np.array_equal(R.relabel(got), R.relabel(C.golden()[name]['ref'])), name + ': the reference partition'
    if name in ('field100', GOLDEN[0], 'degenerate'):                           # twice, the same bits
        again, info2 = O.segment_mesh(pos, faces, k, m, return_info=True)
        assert torch.equal(again, seg) and torch.equal(info2['normals'].view(torch.int32), info['normals'].view(torch.int32))


def test_batched_equals_single_with_an_empty_scene_in_the_middle():
    scenes = [C.mesh_case(n)[:2] for n in C.BATCH]
    segs, infos = O.segment_meshes(scenes, 0.01, 3, return_info=True)
    assert len(segs) == 3
    for name, seg, info in zip(C.BATCH, segs, infos):
        want = C.mesh_rule(name)
        assert np.array_equal(seg.cpu().numpy(), want['seg']), name
        single = O.segment_mesh(*C.mesh_case(name)[:2], 0.01, 3)
        assert torch.equal(single, seg), name
        assert info['n_segments'] == len(np.unique(want['seg'])) and info['n_nan'] == 0
    assert segs[1].tolist() == [0, 1, 2, 3, 4] and infos[1]['n_segments'] == 5
    # scenes of different k and m give what they give alone; dict scenes are accepted
    g = C.golden()
    names = GOLDEN[:3]
    for name in names:
        v = g[name]
        both = O.segment_meshes([{'positions': v['pos'], 'faces': v['faces']}, scenes[0]], v['k'], v['m'])
        assert np.array_equal(both[0].cpu().numpy(), C.golden_rule(name)['seg']), name


def test_float64_positions_are_rounded_to_float32_first():
    pos, faces, k, m, want = _mesh('strip:22')
    seg = O.segment_mesh(pos.astype(np.float64) + 1e-12, torch.from_numpy(faces).cuda(), k, m)
    assert np.array_equal(seg.cpu().numpy(), want['seg'])


def test_voxelize_scene_accepts_the_segments():
    from box2mask_amd import prepare
    pos, faces, k, m, want = _mesh('field100')
    seg = O.segment_mesh(pos, faces, k, m)
    rng = np.random.default_rng(0)
    scene = {'positions': pos.astype(np.float64), 'colors': rng.random((len(pos), 3)), 'normals': rng.random((len(pos), 3)),
             'segments': seg}
    out = prepare.voxelize_scene(scene, 0.02)
    ids = out['vox_segments'] if isinstance(out, dict) else None
    assert ids is not None and set(np.unique(torch.as_tensor(ids).cpu().numpy()).tolist()) <= set(np.unique(want['seg']).tolist())


def test_refusals():
    pos, faces, k, m, _ = _mesh('strip:22')
    for bad in (-1, len(pos)):
        f = faces.copy()
        f[5, 1] = bad
        with pytest.raises(ValueError):
            O.segment_mesh(pos, f)
        with pytest.raises(ValueError):
            O.segment_meshes([(pos, faces), (pos, f)])
    with pytest.raises(ValueError):
        O.segment_mesh(pos[:, :2], faces)
    with pytest.raises(ValueError):
        O.segment_mesh(pos, faces.astype(np.float32))
    with pytest.raises(ValueError):
        O.graph_segment([0, 1], [1, 5], [0.0, 0.0], 5)
    with pytest.raises(ValueError):
        O.graph_segment([0, -1], [1, 2], [0.0, 0.0], 5)
    with pytest.raises(ValueError):
        O.graph_segment([0, 1], [1, 2], [0.0], 5)
    # the entries refuse sizes on the arguments alone, before anything is launched
    table = torch.zeros(O.DESC, dtype=torch.int64, device='cuda')
    for args in ((1, 2 ** 31, 64), (1, 64, 2 ** 31), (65536, 64, 64), (-1, 64, 64)):
        with pytest.raises(_lib.B2MError):
            _lib.call('b2m_mesh_edge_weights', table.data_ptr(), *args)
    for args in ((1, 2 ** 31, 64, 0.01, 20, 7), (1, 64, 2 ** 31, 0.01, 20, 7), (1, 64, 64, 0.01, 20, 0), (1, 64, 64, 0.01, 20, 8)):
        with pytest.raises(_lib.B2MError):
            _lib.call('b2m_graph_segment', table.data_ptr(), *args)
    with pytest.raises(_lib.B2MError):
        _lib.call('b2m_edge_sort_keys', table.data_ptr(), 4, table.data_ptr(), 2)
    # an endpoint outside the vertices that reaches the kernel past the wrapper raises the scene's flag and nothing is touched
    a = torch.tensor([0, 1], dtype=torch.int32, device='cuda')
    b = torch.tensor([1, 7], dtype=torch.int32, device='cuda')
    w = torch.zeros(2, dtype=torch.float32, device='cuda')
    keys = torch.empty(2, dtype=torch.int64, device='cuda')
    forest = O._forest(3, 2, 'cuda')
    out = torch.zeros((1, 4), dtype=torch.int32, device='cuda')
    g = dict(forest, n_vert=3, n_faces=0, n_edges=2, n_pad=2, edge_a=a, edge_b=b, weights=w, keys=keys)
    desc = O._table([g], out, 'cuda')
    _lib.call('b2m_edge_sort_keys', w.data_ptr(), 2, keys.data_ptr(), 2)
    _lib.call('b2m_sort_u64', keys.data_ptr(), 2)
    _lib.call('b2m_graph_segment', desc.data_ptr(), 1, 3, 2, 0.01, 1, 7)
    assert out.cpu().tolist()[0][2] == 1
