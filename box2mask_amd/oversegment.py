"""Mesh over-segmentation on the device: vertices + faces -> the `segments` every scene starts from.

The reference makes them with a C++ tool of its own (dataprocessing/oversegmentation/cpp/segmentator.cpp: Felzenszwalb's graph
segmentation over the mesh's faces, weights from smoothed vertex normals) and reads them back from `*.segs.json`; ScanNet test scenes
and ARKitScenes ship none.  Here the same rule (profiles/overseg_rule.md) runs in csrc/overseg.hip: ``b2m_mesh_edge_weights`` (normals,
weights, sort keys), the existing ``b2m_sort_u64``, and ``b2m_graph_segment`` (the two sequential passes, one wave per scene, and the
labels).  The reference's sort is unstable; ours orders edges by (weight, edge index), which fixes the ids where the reference fixes
only the partition.  No CPU fallback.
"""
from __future__ import annotations

import json

import numpy as np
import torch

from . import _lib
from ._lib import ptr
from .augment import _check_face_range, _face_range, vertex_face_csr

DESC = 20                      # B2M_OVERSEG_DESC
MAX_EDGES = 1 << 30            # the padded edge count must stay below 2^31 (b2m_sort_u64)


def _pow2(n):
    return 1 << max(int(n) - 1, 1).bit_length()


def _scene_arrays(scene):
    if isinstance(scene, dict):
        return scene['positions'], scene['faces']
    return scene


def _to_device(pos, faces, device):
    """float32 positions (float64 is ROUNDED to float32: the reference reads PLY floats) and int64 faces, contiguous on the device."""
    pos = torch.as_tensor(np.asarray(pos) if not torch.is_tensor(pos) else pos)
    faces = torch.as_tensor(np.asarray(faces) if not torch.is_tensor(faces) else faces)
    if pos.numel() == 0:
        pos = pos.reshape(0, 3)
    if faces.numel() == 0:
        faces = faces.reshape(0, 3)
    if pos.dim() != 2 or pos.shape[1] != 3 or not pos.is_floating_point():
        raise ValueError('positions: a floating-point (V, 3) array')
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.is_floating_point() or faces.dtype == torch.bool:
        raise ValueError('faces: an integer (F, 3) array')
    if pos.shape[0] >= 2 ** 31 or 3 * faces.shape[0] >= 2 ** 32:
        raise ValueError('segment_mesh: V < 2^31 and 3F < 2^32')
    if 3 * faces.shape[0] > MAX_EDGES:
        raise ValueError('segment_mesh: at most 2^30 edges (3F): the sort pads them to a power of two below 2^31')
    return (pos.to(device=device, dtype=torch.float32).contiguous(), faces.to(device=device, dtype=torch.int64).contiguous())


def _forest(n_vert, n_edges, device):
    """Workspace and outputs of the second half for one scene."""
    return {'parent': torch.empty(n_vert, dtype=torch.int32, device=device), 'rank': torch.empty(n_vert, dtype=torch.int32, device=device),
            'size': torch.empty(n_vert, dtype=torch.int32, device=device), 'thr': torch.empty(n_vert, dtype=torch.float32, device=device),
            'seg': torch.empty(n_vert, dtype=torch.int64, device=device)}


def _record(b, out_row):
    z = lambda name: ptr(b[name]) if b.get(name) is not None and b[name].numel() else 0
    return [z('pos'), b['n_vert'], z('faces'), b['n_faces'], z('row_ptr'), z('face_of'), z('normals'), z('weights'), z('keys'),
            b['n_pad'], z('edge_a'), z('edge_b'), b['n_edges'], z('parent'), z('rank'), z('size'), z('thr'), z('seg'),
            out_row.data_ptr(), 0]


def _table(bufs, out, device):
    rows = [_record(b, out[i]) for i, b in enumerate(bufs)]
    return torch.tensor(rows, dtype=torch.int64).to(device)


def _params(k_thresh, seg_min_verts):
    k = float(np.float32(k_thresh))
    m = int(seg_min_verts)
    if not -2 ** 31 <= m < 2 ** 31:
        raise ValueError('seg_min_verts must fit 32 bits')
    return k, m


def _raise_on_error(flags):
    bad = [i for i, f in enumerate(flags) if f]
    if bad:
        raise _lib.B2MError('b2m_graph_segment gave up on scene(s) %s: an edge endpoint outside the vertices, or a find longer than 64 hops'
                            % bad)


def segment_meshes(scenes, k_thresh=0.01, seg_min_verts=20, device=None, return_info=False):
    """Segments of a list of meshes in one batch of launches and ONE host read.

    `scenes`: (positions, faces) pairs, or dicts with those keys.  positions (V,3) float32 -- float64 input is rounded to float32
    first, because the reference reads the floats of a PLY file; faces (F,3) integer vertex indices, refused with ValueError outside
    [0, V).  Returns one int64 device tensor (V,) per scene: the ROOT VERTEX id of every vertex's segment (what the reference writes as
    `segIndices`; not dense ranks), usable as ``scene['segments']``.  A scene with V == 0 or F == 0 launches nothing and gets
    arange(V).  With `return_info` also a dict per scene: n_segments, n_nan (NaN weights: degenerate faces, zero-length edges; they
    sort last and only pass two can use them) and the smoothed vertex normals (V,3) the weights were made from."""
    _lib.require_gpu()
    device = torch.device('cuda' if device is None else device)
    k, m = _params(k_thresh, seg_min_verts)
    meshes = [_to_device(*_scene_arrays(s), device) for s in scenes]
    live = [i for i, (p, f) in enumerate(meshes) if p.shape[0] and f.shape[0]]
    bufs = []
    with torch.cuda.device(device):
        out = torch.zeros((max(len(live), 1), 4), dtype=torch.int32, device=device)
        ranges = [_face_range(meshes[i][1]) for i in live]
        for i in live:
            pos, faces = meshes[i]
            n_vert, n_edges = pos.shape[0], 3 * faces.shape[0]
            b = {'pos': pos, 'faces': faces, 'n_vert': n_vert, 'n_faces': faces.shape[0], 'n_edges': n_edges, 'n_pad': _pow2(n_edges),
                 'normals': torch.empty((n_vert, 3), dtype=torch.float32, device=device),
                 'weights': torch.empty(n_edges, dtype=torch.float32, device=device),
                 'edge_a': torch.empty(n_edges, dtype=torch.int32, device=device),
                 'edge_b': torch.empty(n_edges, dtype=torch.int32, device=device)}
            b['keys'] = torch.empty(b['n_pad'], dtype=torch.int64, device=device)
            b.update(_forest(n_vert, n_edges, device))
            bufs.append(b)
        if live:
            # the one read before the launches: faces that name no vertex are refused, never clamped
            for i, (lo, hi) in zip(live, torch.stack(ranges).cpu().tolist()):
                _check_face_range(lo, hi, meshes[i][0].shape[0])
            for b in bufs:
                b['row_ptr'], b['face_of'] = vertex_face_csr(b['faces'], b['n_vert'], checked=True)
            desc = _table(bufs, out, device)
            max_vert, max_pad = max(b['n_vert'] for b in bufs), max(b['n_pad'] for b in bufs)
            max_edges = max(b['n_edges'] for b in bufs)
            _lib.call('b2m_mesh_edge_weights', desc.data_ptr(), len(bufs), max_vert, max_pad)
            for b in bufs:
                _lib.call('b2m_sort_u64', ptr(b['keys']), b['n_pad'])
            _lib.call('b2m_graph_segment', desc.data_ptr(), len(bufs), max_vert, max_edges, k, m, 7)
            counts = out.cpu().tolist()                                        # the one read of the results
            _raise_on_error([c[2] for c in counts])
    segs, infos = [], []
    at = dict(zip(live, range(len(live))))
    for i, (pos, faces) in enumerate(meshes):
        if i in at:
            b, c = bufs[at[i]], counts[at[i]]
            segs.append(b['seg'])
            infos.append({'n_segments': c[0], 'n_nan': c[1], 'normals': b['normals'], 'weights': b['weights'], 'keys': b['keys']})
        else:
            n_vert = pos.shape[0]
            segs.append(torch.arange(n_vert, dtype=torch.int64, device=device))
            infos.append({'n_segments': n_vert, 'n_nan': 0, 'normals': torch.zeros((n_vert, 3), dtype=torch.float32, device=device),
                          'weights': torch.zeros(0, dtype=torch.float32, device=device),
                          'keys': torch.zeros(0, dtype=torch.int64, device=device)})
    return (segs, infos) if return_info else segs


def segment_mesh(positions, faces, k_thresh=0.01, seg_min_verts=20, device=None, return_info=False):
    """One mesh: a batch of one through `segment_meshes` (see there).  Returns seg, or (seg, info)."""
    res = segment_meshes([(positions, faces)], k_thresh, seg_min_verts, device, return_info)
    return (res[0][0], res[1][0]) if return_info else res[0]


def mesh_edge_weights(positions, faces, device=None):
    """The first half on its own: (normals (V,3), weights (3F,), keys (3F,) int64 bit patterns of the unsorted 64-bit keys,
    edge_a, edge_b (3F,) int32).  F >= 1 and V >= 1."""
    _lib.require_gpu()
    device = torch.device('cuda' if device is None else device)
    pos, faces = _to_device(positions, faces, device)
    n_vert, n_edges = pos.shape[0], 3 * faces.shape[0]
    if not n_vert or not n_edges:
        raise ValueError('mesh_edge_weights: an empty mesh has no edges')
    with torch.cuda.device(device):
        _check_face_range(*_face_range(faces).cpu().tolist(), n_vert)
        b = {'pos': pos, 'faces': faces, 'n_vert': n_vert, 'n_faces': faces.shape[0], 'n_edges': n_edges, 'n_pad': _pow2(n_edges),
             'normals': torch.empty((n_vert, 3), dtype=torch.float32, device=device),
             'weights': torch.empty(n_edges, dtype=torch.float32, device=device),
             'edge_a': torch.empty(n_edges, dtype=torch.int32, device=device),
             'edge_b': torch.empty(n_edges, dtype=torch.int32, device=device)}
        b['keys'] = torch.empty(b['n_pad'], dtype=torch.int64, device=device)
        b['row_ptr'], b['face_of'] = vertex_face_csr(faces, n_vert, checked=True)
        out = torch.zeros((1, 4), dtype=torch.int32, device=device)
        desc = _table([b], out, device)
        _lib.call('b2m_mesh_edge_weights', desc.data_ptr(), 1, n_vert, b['n_pad'])
    return b['normals'], b['weights'], b['keys'][:n_edges], b['edge_a'], b['edge_b']


def graph_segment(a, b, w, n_vertices, k_thresh=0.01, seg_min_verts=20, device=None, return_info=False):
    """The second half on its own, for any weighted graph: edges (a[e], b[e]) with float32 weights w[e] over `n_vertices` vertices, in
    the order (w, e) -- -0 == +0, NaN last.  Returns seg (n_vertices,) int64 root ids, or (seg, {'n_segments', 'n_nan'}).  Endpoints
    outside [0, n_vertices) raise ValueError."""
    _lib.require_gpu()
    device = torch.device('cuda' if device is None else device)
    k, m = _params(k_thresh, seg_min_verts)
    n_vert = int(n_vertices)
    ea = torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).reshape(-1)
    eb = torch.as_tensor(np.asarray(b) if not torch.is_tensor(b) else b).reshape(-1)
    ew = torch.as_tensor(np.asarray(w) if not torch.is_tensor(w) else w).reshape(-1)
    n_edges = ea.numel()
    if eb.numel() != n_edges or ew.numel() != n_edges:
        raise ValueError('graph_segment: a, b and w must have one entry per edge')
    if not 0 <= n_vert < 2 ** 31 or n_edges > MAX_EDGES:
        raise ValueError('graph_segment: n_vertices < 2^31 and at most 2^30 edges')
    if n_vert == 0 or n_edges == 0:
        if n_edges:
            raise ValueError('graph_segment: edges without vertices')
        seg = torch.arange(n_vert, dtype=torch.int64, device=device)
        return (seg, {'n_segments': n_vert, 'n_nan': 0}) if return_info else seg
    with torch.cuda.device(device):
        ea = ea.to(device=device, dtype=torch.int64)
        eb = eb.to(device=device, dtype=torch.int64)
        lo, hi = torch.stack([torch.minimum(ea.min(), eb.min()), torch.maximum(ea.max(), eb.max())]).cpu().tolist()
        if lo < 0 or hi >= n_vert:
            raise ValueError('graph_segment: edge endpoints must lie in [0, %d), found [%d, %d]' % (n_vert, lo, hi))
        g = {'n_vert': n_vert, 'n_faces': 0, 'n_edges': n_edges, 'n_pad': _pow2(n_edges),
             'edge_a': ea.to(torch.int32).contiguous(), 'edge_b': eb.to(torch.int32).contiguous(),
             'weights': ew.to(device=device, dtype=torch.float32).contiguous()}
        g['keys'] = torch.empty(g['n_pad'], dtype=torch.int64, device=device)
        g.update(_forest(n_vert, n_edges, device))
        out = torch.zeros((1, 4), dtype=torch.int32, device=device)
        desc = _table([g], out, device)
        _lib.call('b2m_edge_sort_keys', ptr(g['weights']), n_edges, ptr(g['keys']), g['n_pad'])
        _lib.call('b2m_sort_u64', ptr(g['keys']), g['n_pad'])
        _lib.call('b2m_graph_segment', desc.data_ptr(), 1, n_vert, n_edges, k, m, 7)
        counts = out.cpu().tolist()[0]
        _raise_on_error([counts[2]])
    return (g['seg'], {'n_segments': counts[0], 'n_nan': counts[1]}) if return_info else g['seg']


def _short(x):
    """A float as the reference's `ofs << float` prints it: six significant digits, %g."""
    return '%g' % float(np.float32(x))


def segs_json(seg, scene_id, k_thresh=0.01, seg_min_verts=20) -> str:
    """The text of the reference's `<scene>.segs.json` (segmentator.cpp:253-266): params.kThresh, params.segMinVerts, sceneId,
    segIndices -- what dataprocessing/scannet.py:408-410 and arkitscenes.py:320-332 read back with json.load."""
    ids = seg.detach().cpu().numpy() if torch.is_tensor(seg) else np.asarray(seg)
    ids = ids.astype(np.int64).reshape(-1)
    return '{"params":{"kThresh":%s,"segMinVerts":%d},"sceneId":%s,"segIndices":[%s]}' % (
        _short(k_thresh), int(seg_min_verts), json.dumps(str(scene_id)), ','.join(map(str, ids.tolist())))
