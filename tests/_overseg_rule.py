"""The over-segmentation rule (profiles/overseg_rule.md) in numpy float32: every product, sum, quotient and square root is one
float32 operation with the association written out, edges ascend by (w, e) with -0 == +0 and NaN weights last.  `mistake` switches
in one deliberate error at a time (tests/test_overseg_rule.py shows that each is caught).

Not a transcription of the reference's loops: normals are formed per visit rank over all vertices at once, the forest is three
arrays."""
import numpy as np

F32 = np.float32
MISTAKES = ('strict_thr', 'le_m', 'pass2_unsorted', 'thr_size_before', 'no_square', 'dot2_na', 'slot_i2i3')


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _unit(x, y, z):
    with np.errstate(all='ignore'):
        n = np.sqrt(_dot(x, y, z, x, y, z))
        return x / n, y / n, z / n


def face_normals(pos, faces):
    p1, p2, p3 = (pos[faces[:, j]] for j in range(3))
    u, v = p2 - p1, p3 - p1
    with np.errstate(all='ignore'):
        cx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        cy = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        cz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    return np.stack(_unit(cx, cy, cz), axis=1).astype(F32)


def vertex_normals(pos, faces):
    """Running mean in face order: the j-th visit of a vertex (visits ascend in 3f + slot) blends with t = 1 / (j + 1)."""
    pos = np.asarray(pos, F32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    n_vert = len(pos)
    normals = np.zeros((n_vert, 3), F32)
    if not len(faces):
        return normals
    nf = face_normals(pos, faces)
    flat = faces.reshape(-1)
    order = np.argsort(flat, kind='stable')
    vert = flat[order]
    start = np.searchsorted(vert, np.arange(n_vert + 1))
    visit = np.arange(len(flat)) - start[vert]                 # rank of this visit within its vertex
    for j in range(int(visit.max()) + 1):
        sel = visit == j
        v, f = vert[sel], order[sel] // 3
        t = F32(1) / (F32(j) + F32(1))
        u = F32(1) - t
        with np.errstate(all='ignore'):
            normals[v] = t * nf[f] + u * normals[v]
    return normals


def mesh_edges(faces, mistake=None):
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    i1, i2, i3 = faces[:, 0], faces[:, 1], faces[:, 2]
    third = (i2, i3) if mistake == 'slot_i2i3' else (i3, i2)
    a = np.stack([i1, i1, third[0]], axis=1).reshape(-1)
    b = np.stack([i2, i3, third[1]], axis=1).reshape(-1)
    return a, b


def edge_weights(pos, normals, a, b, mistake=None):
    pos = np.asarray(pos, F32)
    with np.errstate(all='ignore'):
        d = pos[b] - pos[a]
        dx, dy, dz = _unit(d[:, 0], d[:, 1], d[:, 2])
        na, nb = normals[a], normals[b]
        dot = _dot(na[:, 0], na[:, 1], na[:, 2], nb[:, 0], nb[:, 1], nb[:, 2])
        n2 = na if mistake == 'dot2_na' else nb
        dot2 = _dot(n2[:, 0], n2[:, 1], n2[:, 2], dx, dy, dz)
        w = F32(1) - dot
        if mistake != 'no_square':
            w = np.where(dot2 > 0, w * w, w)
    return w.astype(F32)


def weight_code(w):
    u = np.asarray(w, F32).view(np.uint32).astype(np.uint64)
    u = np.where(np.asarray(w) == 0, np.uint64(0), u)
    code = np.where(u >> np.uint64(31), (~u) & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))
    return np.where(np.isnan(w), np.uint64(0xFFFFFFFF), code)


def sort_keys(w):
    return (weight_code(w) << np.uint64(32)) | np.arange(len(w), dtype=np.uint64)


def edge_order(w, rng=None):
    """Edge indices ascending by (w, e); with `rng`, tied weights (NaN among themselves included) in a random order instead."""
    w = np.asarray(w, F32)
    nan = np.isnan(w)
    val = np.where(nan | (w == 0), F32(0), w)
    minor = np.arange(len(w)) if rng is None else rng.permutation(len(w))
    return np.lexsort((minor, val, nan))


def n_ties(w):
    """Number of edges whose weight another edge shares."""
    code = weight_code(w)
    _, inv, cnt = np.unique(code, return_inverse=True, return_counts=True)
    return int((cnt[inv] > 1).sum())


class Forest:
    def __init__(self, n):
        self.parent = list(range(n))
        self.rank = [0] * n
        self.size = [1] * n

    def find(self, x):
        p = self.parent
        while p[x] != x:
            x = p[x]
        return x

    def join(self, x, y):
        if self.rank[x] > self.rank[y]:
            x, y = y, x
        elif self.rank[x] == self.rank[y]:
            self.rank[y] += 1
        self.parent[x] = y
        self.size[y] += self.size[x]
        return y


def graph_segment(a, b, w, n_vertices, k_thresh, seg_min_verts, mistake=None, order=None, trace=None):
    """Passes one and two and the labels.  `trace` (a dict) receives what the reach predicates need: the merges of each pass as
    (position in the sorted order, loser, winner, equal ranks?, did a's root win?), and the comparisons of pass one that were exact ties."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    w = np.asarray(w, F32)
    k = F32(k_thresh)
    m = int(seg_min_verts)
    order = edge_order(w) if order is None else np.asarray(order)
    u = Forest(n_vertices)
    thr = [k] * n_vertices
    log = {'merge1': [], 'merge2': [], 'thr_equal': [], 'thr_ulp_above': [], 'sizes2': [], 'nan_skipped': 0, 'nan_used': 0}
    al, bl = a.tolist(), b.tolist()
    for pos, e in enumerate(order.tolist()):
        A, B = u.find(al[e]), u.find(bl[e])
        if A == B:
            continue
        we = w[e]
        if np.isnan(we):
            log['nan_skipped'] += 1
        for t in (thr[A], thr[B]):
            if we == t:
                log['thr_equal'].append(pos)
            elif we == np.nextafter(t, F32(np.inf)):
                log['thr_ulp_above'].append(pos)
        ok = (we < thr[A] and we < thr[B]) if mistake == 'strict_thr' else (we <= thr[A] and we <= thr[B])
        if ok:
            equal = u.rank[A] == u.rank[B]
            before = max(u.size[A], u.size[B])
            R = u.join(A, B)
            log['merge1'].append((pos, A if R == B else B, R, equal, R == A))
            size = before if mistake == 'thr_size_before' else u.size[R]
            thr[R] = we + k / F32(size)
    second = range(len(w)) if mistake == 'pass2_unsorted' else order.tolist()
    for pos, e in enumerate(second):
        A, B = u.find(al[e]), u.find(bl[e])
        if A == B:
            continue
        sa, sb = u.size[A], u.size[B]
        log['sizes2'].append((sa, sb))
        small = (sa <= m or sb <= m) if mistake == 'le_m' else (sa < m or sb < m)
        if small:
            equal = u.rank[A] == u.rank[B]
            R = u.join(A, B)
            log['merge2'].append((pos, A if R == B else B, R, equal, R == A))
            if np.isnan(w[e]):
                log['nan_used'] += 1
    if trace is not None:
        trace.update(log)
    return np.array([u.find(q) for q in range(n_vertices)], np.int64)


def segment(pos, faces, k_thresh=0.01, seg_min_verts=20, mistake=None, rng=None, trace=None):
    """Steps 1-6.  Returns (seg, normals, weights, keys, (a, b)); `rng` permutes tied weights (the tie-invariance check)."""
    pos = np.asarray(pos, F32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    normals = vertex_normals(pos, faces)
    a, b = mesh_edges(faces, mistake)
    w = edge_weights(pos, normals, a, b, mistake) if len(a) else np.zeros(0, F32)
    order = edge_order(w, rng)
    seg = graph_segment(a, b, w, len(pos), k_thresh, seg_min_verts, mistake, order, trace)
    return seg, normals, w, sort_keys(w), (a, b)


def relabel(seg):
    """Labels by first occurrence: two label arrays describe the same partition iff their relabellings are equal."""
    seg = np.asarray(seg)
    _, first, inv = np.unique(seg, return_index=True, return_inverse=True)
    rank = np.argsort(np.argsort(first))
    return rank[inv]
