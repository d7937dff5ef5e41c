"""Edge cases of the over-segmentation (csrc/overseg.hip), shared by tests/test_overseg_rule.py (CPU: every case reaches what it
claims) and tests/test_gpu_overseg.py (the kernels against tests/_overseg_rule.py).  Meshes: (pos, faces, k, m); graphs: (a, b, w,
n_vertices, k, m).  The rule's result of a case is computed once (functools.lru_cache) and never modified."""
import functools
import os

import numpy as np

import _overseg_rule as R

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'overseg.npz')
WINDOW = 64


def height_field(nx, ny, seed, noise=0.002, step=0.05, shuffle=True, z0=0.0, x0=0.0):
    """A noisy nx x ny height field with a box and a ripple on it, two triangles per cell, faces shuffled."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(nx), np.arange(ny), indexing='ij')
    z = rng.normal(0.0, noise, (nx, ny))
    box = (gx > nx * 0.25) & (gx < nx * 0.55) & (gy > ny * 0.3) & (gy < ny * 0.7)
    z = z + 0.3 * box + 0.02 * np.sin(gx * 0.9) * (gy > ny * 0.75)
    pos = np.stack([x0 + gx * step, gy * step, z0 + z], axis=-1).reshape(-1, 3).astype(np.float32)
    idx = (gx * ny + gy)
    a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[:-1, 1:], idx[1:, 1:]
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([b, d, c], -1).reshape(-1, 3)])
    if shuffle:
        faces = faces[rng.permutation(len(faces))]
    return pos, faces.astype(np.int64)


def strip(n_faces, seed):
    """A noisy triangle strip of n_faces faces (n_faces + 2 vertices; 5 loose vertices when it has none), faces shuffled."""
    rng = np.random.default_rng(seed)
    n_vert = n_faces + 2 if n_faces else 5
    i = np.arange(n_vert)
    pos = np.stack([i * 0.05, (i % 2) * 0.05, rng.normal(0, 0.004, n_vert) + 0.1 * (i > n_vert // 2)], axis=1).astype(F32)
    f = np.arange(n_faces)
    faces = np.where((f % 2 == 0)[:, None], np.stack([f, f + 1, f + 2], 1), np.stack([f + 1, f, f + 2], 1)).reshape(-1, 3)
    return pos, faces[rng.permutation(n_faces)].astype(np.int64)


# ---- meshes
SIZES = (0, 1, 21, 22, 341, 342)            # 3F = 0, 3, 63, 66, 1023, 1026: around the 64-edge window and the sort's padding
MESH_ORDER = ['strip:%d' % f for f in SIZES] + ['degenerate', 'field100']


@functools.lru_cache(maxsize=None)
def mesh_case(name):
    if name.startswith('strip:'):
        n = int(name.split(':')[1])
        return strip(n, 40 + n) + (0.01, 3)
    if name == 'degenerate':               # a face that names one vertex twice (NaN normal, a zero-length edge) among sound ones
        pos, faces = strip(22, 7)
        return pos, np.concatenate([faces[:9], [[3, 3, 5]], faces[9:]]), 0.01, 3
    if name == 'field100':                 # 10 k vertices, ~59 k edges, ~930 windows, components far larger than a window
        return height_field(100, 100, 5) + (0.01, 20)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def mesh_rule(name):
    pos, faces, k, m = mesh_case(name)
    trace = {}
    seg, normals, w, keys, (a, b) = R.segment(pos, faces, k, m, trace=trace)
    return {'seg': seg, 'normals': normals, 'w': w, 'keys': keys, 'a': a, 'b': b, 'trace': trace}


BATCH = ('strip:22', 'strip:0', 'strip:341')     # three scenes, the empty one in the middle


# ---- golden meshes (tools/gen_golden_overseg.py): the reference's segIndices
@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    out = {}
    for name in z['names'].tolist():
        k, m, ties, seed = z[name + '.params'].tolist()
        out[name] = {'pos': z[name + '.pos'], 'faces': z[name + '.faces'].astype(np.int64), 'ref': z[name + '.seg'].astype(np.int64),
                     'k': k, 'm': int(m), 'ties': int(ties)}
    return out


@functools.lru_cache(maxsize=None)
def golden_rule(name):
    g = golden()[name]
    seg, normals, w, keys, (a, b) = R.segment(g['pos'], g['faces'], g['k'], g['m'])
    return {'seg': seg, 'normals': normals, 'w': w, 'keys': keys, 'a': a, 'b': b}


# ---- hand-built graphs
def _chain(first, n, w):
    """Edges that make vertices first .. first+n-1 one component in pass one (n - 1 edges of weight w)."""
    return [(first + i, first + i + 1, w) for i in range(n - 1)]


def _graph(edges, n_vertices, k, m):
    a, b, w = zip(*edges)
    return np.array(a, np.int64), np.array(b, np.int64), np.array(w, F32), n_vertices, k, m


@functools.lru_cache(maxsize=None)
def graph_case(name):
    if name == 'fan64':
        # one window, 64 merges: a tournament over 64 vertices (32 + 16 + 8 + 4 + 2 + 1 edges between vertices whose roots were
        # re-parented earlier in the SAME window), then vertex 64 joins
        edges, step = [], 1
        while step < 64:
            edges += [(i, i + step, 0.0) for i in range(0, 64, 2 * step)]
            step *= 2
        return _graph(edges + [(0, 64, 0.0)], 65, 0.01, 1)
    if name == 'quiet_window':
        # window 0: 64 merging edges; window 1: 64 edges of weight 1 > k between fresh vertices: pass one merges none, pass two all
        edges = _chain(0, 65, 0.001) + [(100 + 2 * i, 101 + 2 * i, 1.0) for i in range(64)]
        return _graph(edges, 228, 0.01, 2)
    if name in ('thr_equal', 'thr_ulp_above'):
        # k = 0.5: {0,1} has thr 0 + 0.5/2 = 0.25, {2,3,4,5} has thr 0.125 + 0.5/4 = 0.25, both exact
        last = F32(0.25) if name == 'thr_equal' else np.nextafter(F32(0.25), F32(1))
        return _graph([(0, 1, 0.0), (2, 3, 0.0), (4, 5, 0.0), (2, 4, 0.125), (0, 2, last)], 6, 0.5, 1)
    if name == 'sizes_m':
        # m = 4; components of 3 (0-2), 4 (3-6), 5 (7-11), 4 (12-15) meet in pass two: (4,5) no, (4,4) no, (3,4) yes
        edges = _chain(0, 3, 0.0) + _chain(3, 4, 0.0) + _chain(7, 5, 0.0) + _chain(12, 4, 0.0)
        return _graph(edges + [(3, 7, 1.0), (3, 12, 1.0), (0, 12, 1.0)], 16, 0.001, 4)
    if name == 'pass2_order':
        # m = 4; edge 6 = (c3, c5) has the larger weight and the lower index than edge 7 = (c3, single): sorted, the single vertex
        # joins first and c3 grows to 4, which then stays apart from c5
        edges = _chain(0, 3, 0.0) + _chain(3, 5, 0.0) + [(0, 3, 2.0), (0, 8, 1.0)]
        return _graph(edges, 9, 0.001, 4)
    if name == 'ranks':
        # equal ranks (0,1), A's rank higher (0,2), B's rank higher (3,0), equal ranks above zero (0,4) after (4,5)
        return _graph([(0, 1, 0.0), (0, 2, 0.0), (3, 0, 0.0), (4, 5, 0.0), (0, 4, 0.0)], 6, 0.5, 1)
    if name == 'nan':
        # a NaN weight: pass one skips it (no comparison holds), pass two joins its ends (sizes 1 < 2); -0 ties with +0 by index
        return _graph([(0, 1, np.nan), (2, 3, -0.0), (3, 4, 0.0), (5, 6, np.inf), (7, 7, 0.0)], 8, 0.01, 2)
    if name == 'tie_root':
        # two edges of one weight: (0,1) then (2,0) leaves root 1, the other order leaves root 0
        return _graph([(0, 1, 0.0), (2, 0, 0.0)], 3, 0.01, 1)
    raise KeyError(name)


GRAPH_ORDER = ['fan64', 'quiet_window', 'thr_equal', 'thr_ulp_above', 'sizes_m', 'pass2_order', 'ranks', 'nan', 'tie_root']


@functools.lru_cache(maxsize=None)
def graph_rule(name):
    a, b, w, n, k, m = graph_case(name)
    trace = {}
    seg = R.graph_segment(a, b, w, n, k, m, trace=trace)
    return {'seg': seg, 'trace': trace}


# ---- reach predicates: each returns None or says what the case failed to reach
def reach(name):
    if name in MESH_ORDER:
        pos, faces, k, m = mesh_case(name)
        r = mesh_rule(name)
        n_edges = 3 * len(faces)
        if name.startswith('strip:'):
            want = {0: 0, 1: 3, 21: 63, 22: 66, 341: 1023, 342: 1026}[len(faces)]
            if n_edges != want:
                return 'edges %d' % n_edges
            if n_edges and not np.isfinite(r['w']).all():
                return 'non-finite weight'
            if len(faces) >= 21 and not (1 < len(np.unique(r['seg'])) < len(pos)):
                return 'trivial partition'
            return None
        if name == 'degenerate':
            n_nan = int(np.isnan(r['w']).sum())
            ok = 0 < n_nan < n_edges and np.isnan(r['normals'][3]).all() and r['trace']['nan_skipped'] > 0
            return None if ok else 'NaN weights %d' % n_nan
        windows = -(-n_edges // WINDOW)
        biggest = np.bincount(R.relabel(r['seg'])).max()
        if not (windows > 900 and biggest > 10 * WINDOW and 2 <= len(np.unique(r['seg'])) < 200):
            return 'windows %d, largest component %d' % (windows, biggest)
        if not (r['trace']['merge1'] and r['trace']['merge2']):
            return 'a pass without merges'
        return None
    a, b, w, n, k, m = graph_case(name)
    r = graph_rule(name)
    t = r['trace']
    seg = r['seg']
    if name == 'fan64':
        rewritten = sum(1 for (pos, lose, win, eq, a_wins) in t['merge1'] if {lose, win} != {int(a[pos]), int(b[pos])})
        ok = len(w) == 64 and [p[0] for p in t['merge1']] == list(range(64)) and len(set(seg.tolist())) == 1 and rewritten >= 30
        return None if ok else 'merges %d, rewritten %d' % (len(t['merge1']), rewritten)
    if name == 'quiet_window':
        ok = (len(w) == 128 and [p[0] for p in t['merge1']] == list(range(64))
              and sorted(p[0] for p in t['merge2']) == list(range(64, 128)))
        return None if ok else 'merges %s / %s' % (t['merge1'], t['merge2'])
    if name == 'thr_equal':
        ok = t['thr_equal'].count(4) == 2 and len(t['merge1']) == 5 and len(set(seg.tolist())) == 1
        return None if ok else 'ties %s' % t['thr_equal']
    if name == 'thr_ulp_above':
        ok = t['thr_ulp_above'].count(4) == 2 and len(t['merge1']) == 4 and len(set(seg.tolist())) == 2
        return None if ok else 'ulp %s' % t['thr_ulp_above']
    if name == 'sizes_m':
        ok = t['sizes2'] == [(4, 5), (4, 4), (3, 4)] and len(t['merge2']) == 1 and len(set(seg.tolist())) == 3
        return None if ok else 'sizes %s' % t['sizes2']
    if name == 'pass2_order':
        ok = t['sizes2'] == [(3, 1), (4, 5)] and len(set(seg.tolist())) == 2
        return None if ok else 'sizes %s' % t['sizes2']
    if name == 'ranks':
        kinds = [(eq, a_wins) for (_, _, _, eq, a_wins) in t['merge1']]
        ok = kinds == [(True, False), (False, True), (False, False), (True, False), (True, False)] and len(set(seg.tolist())) == 1
        return None if ok else 'kinds %s' % kinds
    if name == 'nan':
        ok = t['nan_skipped'] == 1 and t['nan_used'] == 1 and seg[0] == seg[1] and seg[2] == seg[3] == seg[4] and seg[5] == seg[6]
        return None if ok else 'nan %d / %d, seg %s' % (t['nan_skipped'], t['nan_used'], seg)
    if name == 'tie_root':
        other = R.graph_segment(a, b, w, n, k, m, order=np.array([1, 0]))
        ok = seg.tolist() == [1, 1, 1] and other.tolist() == [0, 0, 0]
        return None if ok else 'roots %s / %s' % (seg, other)
    raise KeyError(name)
