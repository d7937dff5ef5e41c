"""The rule of csrc/augment.hip: every C entry of the augmentation block of include/b2m_prepare.h restated in numpy, fp64, no
device, in the order of operations the source documents -- so that the device is held to it BIT FOR BIT (tests/test_gpu_augment_edges.py)
after tests/test_augment_rule.py has tied it to the reference's own outputs (tests/golden/augment.npz).

What makes that possible: the kernels are fp64 (or fp64 and one rounding to fp32), compiled without contraction and without fast
math; +, -, *, / and sqrt are correctly rounded on both sides; the only sums longer than three terms (b2m_aug_stats, the face sums of
b2m_aug_vertex_normals) have an order that is a function of the sizes alone, and this module replays it.  numpy evaluates an
expression elementwise in the order it is written and never contracts, so every line below is written as the kernel writes it.

Every function takes ``mistake=``: one deliberate MISTAKE written as a variant of the rule.  tests/test_augment_rule.py shows that
each of them changes a named case of tests/_augment_cases.py: that is how the cases are shown to have teeth."""
import math

import numpy as np

THREADS = 256                        # AUG_THREADS
MAX_BLOCKS = 256                     # AUG_MAX_BLOCKS
ROWS_PER_BLOCK = 4 * THREADS         # b2m_aug_stats: nb = ceil(n / (AUG_THREADS * 4))

MISTAKES = ('blur_tap_order', 'blur_reflect', 'blur_5_passes', 'blur_round_each_tap',
            'displace_no_down', 'displace_no_up', 'displace_last_from_step', 'displace_lt_hi', 'displace_strides_swapped',
            'stats_sequential', 'stats_nb_256', 'stats_no_stride',
            'normals_descending', 'normals_zero_fallback',
            'affine_no_recentre', 'affine_cofactor_transposed',
            'colour_stage_order', 'colour_clip_before_add',
            'boxes_sem_highest', 'boxes_radius_f32', 'boxes_bound_half_extent', 'boxes_count_out_of_range')

# branch record of displace, per point and axis (bits; 0 = none)
DOWN, UP, LAST = 1, 2, 4

F32, F64 = np.float32, np.float64


def bits(a):
    """The raw bits of a float array, for `np.array_equal` on them (NaN payloads and the sign of zero included)."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    """Equal shape, dtype and bits; every NaN counts as equal to every NaN at the same position (the kernels and numpy may
    produce different payloads: the contract promises a NaN, not which)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != 'f':
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


# ----------------------------------------------------------------------------- b2m_aug_stats (augment.hip:29-91)
def stats_blocks(n, mistake=None):
    nb = -(-n // (THREADS if mistake == 'stats_nb_256' else ROWS_PER_BLOCK))
    return min(MAX_BLOCKS, nb)


def chain_length(n):
    """Rows one thread adds, at most: L of the mean's error bound."""
    return -(-n // (THREADS * stats_blocks(n)))


def _merge(a, b):
    """aug_stat_merge (:33-41): sums add; min / max / max|.| keep `a` unless `b` is strictly better, so a NaN never enters them and
    of two zeros of different sign the one already there stays."""
    return np.stack([a[..., 0, :] + b[..., 0, :],
                     np.where(b[..., 1, :] < a[..., 1, :], b[..., 1, :], a[..., 1, :]),
                     np.where(b[..., 2, :] > a[..., 2, :], b[..., 2, :], a[..., 2, :]),
                     np.where(b[..., 3, :] > a[..., 3, :], b[..., 3, :], a[..., 3, :])], -2)


_IDENTITY = np.array([[0.0] * 3, [np.inf] * 3, [-np.inf] * 3, [0.0] * 3])


def _tree(s):
    """aug_stat_block (:42-50): the halving tree over the 256 slots of axis -3; slot 0."""
    o = THREADS // 2
    while o > 0:
        s = _merge(s[..., :o, :, :], s[..., o:2 * o, :, :])
        o >>= 1
    return s[..., 0, :, :]


def stats(x, mistake=None):
    """(stats (12,) as the entry writes them, fsum means (3,)).  NaN rows make the mean NaN and are IGNORED by min, max and
    max|.| (numpy would propagate them; the header says the entry does not)."""
    x = np.asarray(x, F64)
    n = len(x)
    assert n > 0 and x.shape == (n, 3)
    with np.errstate(all='ignore'):
        fmean = np.array([math.fsum(x[:, c]) / n if np.isfinite(x[:, c]).all() else np.nan for c in range(3)])
        rows = np.stack([x, x, x, np.abs(x)], 1)                                   # (n, 4, 3): what one row contributes (:57-62)
        if mistake == 'stats_sequential':
            acc = _IDENTITY.copy()
            for r in rows:
                acc = _merge(acc, r)
            out = acc.copy()
        else:
            nb = stats_blocks(n, mistake)
            per_sweep = nb * THREADS
            L = 1 if mistake == 'stats_no_stride' else -(-n // per_sweep)
            pad = np.broadcast_to(_IDENTITY, (L * per_sweep, 4, 3)).copy()        # the identity changes no accumulator
            m = min(n, L * per_sweep)
            pad[:m] = rows[:m]
            sweeps = pad.reshape(L, nb, THREADS, 4, 3)                             # row = k * nb * 256 + b * 256 + t  (:56)
            acc = np.broadcast_to(_IDENTITY, (nb, THREADS, 4, 3)).copy()
            for k in range(L):                                                     # ascending rows, from the identity
                acc = _merge(acc, sweeps[k])
            partial = _tree(acc)                                                   # (nb, 4, 3): one partial row per block
            fin = np.broadcast_to(_IDENTITY, (THREADS, 4, 3)).copy()               # slots >= nb hold the identity (:72-76)
            fin[:nb] = partial
            out = _tree(fin)
        out[0] = out[0] / F64(n)
    return out.reshape(12), fmean


# ----------------------------------------------------------------------------- b2m_aug_affine (:93-138)
def cofactor(M):
    """The cofactor matrix as the host code forms it (:131-134)."""
    m = np.asarray(M, F64).reshape(9)
    K = np.empty(9)
    K[0] = m[4] * m[8] - m[5] * m[7]; K[1] = m[5] * m[6] - m[3] * m[8]; K[2] = m[3] * m[7] - m[4] * m[6]
    K[3] = m[2] * m[7] - m[1] * m[8]; K[4] = m[0] * m[8] - m[2] * m[6]; K[5] = m[1] * m[6] - m[0] * m[7]
    K[6] = m[1] * m[5] - m[2] * m[4]; K[7] = m[2] * m[3] - m[0] * m[5]; K[8] = m[0] * m[4] - m[1] * m[3]
    return K.reshape(3, 3)


def affine(pos, normals, M, c=None, t=None, recentre=True, mistake=None):
    """(pos', normals' or None).  c: the centre the kernel uses (the device row when given, else the host row, else zero)."""
    pos = np.asarray(pos, F64)
    M = np.asarray(M, F64).reshape(3, 3)
    c = np.zeros(3) if c is None else np.asarray(c, F64).reshape(3)
    t = np.zeros(3) if t is None else np.asarray(t, F64).reshape(3)
    if mistake == 'affine_no_recentre':
        recentre = False
    with np.errstate(all='ignore'):
        dx, dy, dz = pos[:, 0] - c[0], pos[:, 1] - c[1], pos[:, 2] - c[2]
        out = np.empty_like(pos)
        for a in range(3):
            v = dx * M[a, 0] + dy * M[a, 1] + dz * M[a, 2]
            if recentre:
                v = v + c[a]
            out[:, a] = v + t[a]
        if normals is None:
            return out, None
        nrm = np.asarray(normals, F64)
        K = cofactor(M)
        if mistake == 'affine_cofactor_transposed':
            K = K.T
        o = np.stack([nrm[:, 0] * K[a, 0] + nrm[:, 1] * K[a, 1] + nrm[:, 2] * K[a, 2] for a in range(3)], 1)
        length = np.sqrt(o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1] + o[:, 2] * o[:, 2])
        res = o.copy()                                                             # a NaN length: o as it is
        pos_len = length > 0.0
        res[pos_len] = o[pos_len] / length[pos_len, None]
        res[length == 0.0] = [0.0, 0.0, 1.0]
    return out, res


# ----------------------------------------------------------------------------- b2m_aug_axpy (:140-152)
def axpy(x, y, a):
    with np.errstate(all='ignore'):
        return np.asarray(x, F64) + F64(a) * np.asarray(y, F64)


# ----------------------------------------------------------------------------- b2m_aug_blur (:154-188)
def blur_pass(g, axis, mistake=None):
    """One zero-padded 3-tap pass along `axis` of an fp32 grid (nx,ny,nz,3): acc = 0.0, + w*prev (if present), + w*self, + w*next (if
    present), in fp64, one rounding to fp32."""
    w = F64(F32(1) / F32(3))
    g = np.moveaxis(np.asarray(g, F32), axis, 0)
    x = g.astype(F64)
    n = len(x)
    with np.errstate(all='ignore'):
        if mistake == 'blur_round_each_tap':
            acc = np.zeros(x.shape, F32)
            acc[1:] = (acc[1:].astype(F64) + w * x[:-1]).astype(F32)
            acc = (acc.astype(F64) + w * x).astype(F32)
            acc[:-1] = (acc[:-1].astype(F64) + w * x[1:]).astype(F32)
            return np.ascontiguousarray(np.moveaxis(acc, 0, axis))
        prev, nxt = np.zeros_like(x), np.zeros_like(x)
        has_prev, has_next = np.zeros(n, bool), np.zeros(n, bool)
        prev[1:], has_prev[1:] = x[:-1], True
        nxt[:-1], has_next[:-1] = x[1:], True
        if mistake == 'blur_reflect':                                              # scipy's mode='reflect': the edge sample again
            prev[0], nxt[-1] = x[0], x[-1]
            has_prev[:], has_next[:] = True, True
        sel = lambda m: m.reshape((n,) + (1,) * (x.ndim - 1))
        acc = np.zeros_like(x)
        acc = np.where(sel(has_prev), acc + w * prev, acc)
        if mistake == 'blur_tap_order':                                            # prev, next, self
            acc = np.where(sel(has_next), acc + w * nxt, acc)
            acc = acc + w * x
        else:
            acc = acc + w * x
            acc = np.where(sel(has_next), acc + w * nxt, acc)
    return np.ascontiguousarray(np.moveaxis(acc.astype(F32), 0, axis))


def blur(grid, mistake=None):
    """Six passes: x, y, z, x, y, z."""
    g = np.asarray(grid, F32)
    assert g.ndim == 4 and g.shape[3] == 3
    for p in range(5 if mistake == 'blur_5_passes' else 6):
        g = blur_pass(g, p % 3, mistake)
    return g


# ----------------------------------------------------------------------------- b2m_aug_displace (:190-252)
def axis_cell(xa, lo, step, hi, n, mistake=None):
    """One axis of an inside point (:206-220): (cell i, t, branch bits).  floor((x-lo)/step) clamped to [0, n-2]; one step down
    when x lies below the node computed for i; one step up when it lies above the next; the last node is exactly hi."""
    xa = np.asarray(xa, F64)
    lo, step, hi = F64(lo), F64(step), F64(hi)
    last = int(n) - 1
    node = lambda i: lo + i.astype(F64) * step
    if mistake == 'displace_last_from_step':
        upper_node = lambda i: node(i + 1)
    else:
        upper_node = lambda i: np.where(i + 1 == last, hi, node(i + 1))
    with np.errstate(all='ignore'):
        i = np.floor((xa - lo) / step).astype(np.int64)
        i = np.clip(i, 0, last - 1)
        g0 = node(i)
        down = (i > 0) & (xa < g0)
        if mistake == 'displace_no_down':
            down[:] = False
        i = np.where(down, i - 1, i)
        g0 = np.where(down, node(i), g0)
        g1 = upper_node(i)
        up = (i + 1 < last) & (xa > g1)
        if mistake == 'displace_no_up':
            up[:] = False
        i = np.where(up, i + 1, i)
        g0 = np.where(up, g1, g0)
        g1 = np.where(up, upper_node(i), g1)
        t = (xa - g0) / (g1 - g0)
    return i, t, (down * DOWN + up * UP + (i + 1 == last) * LAST).astype(np.uint8)


def displace(pos, grid, lo, step, hi, n, magnitude, mistake=None):
    """(pos', branch (P,3) uint8 of DOWN | UP | LAST bits; 0 for a point outside).  grid: fp32 (nx,ny,nz,3); lo, step, hi: (3,);
    n: (3,) nodes per axis."""
    pos = np.asarray(pos, F64)
    grid = np.asarray(grid, F32)
    lo, step, hi = (np.asarray(v, F64).reshape(3) for v in (lo, step, hi))
    n = [int(v) for v in n]
    assert grid.shape == (n[0], n[1], n[2], 3)
    out = pos.copy()
    branch = np.zeros(pos.shape, np.uint8)
    with np.errstate(all='ignore'):
        upper = (pos < hi) if mistake == 'displace_lt_hi' else (pos <= hi)
        inside = ((pos >= lo) & upper).all(1)                                      # a NaN compares false: outside
        x = pos[inside]
        i0 = np.zeros(x.shape, np.int64)
        t = np.zeros(x.shape)
        br = np.zeros(x.shape, np.uint8)
        for a in range(3):
            i0[:, a], t[:, a], br[:, a] = axis_cell(x[:, a], lo[a], step[a], hi[a], n[a], mistake)
        flat = grid.reshape(-1, 3)
        sy, sx = n[2], n[1] * n[2]                                                 # in cells of 3 floats
        if mistake == 'displace_strides_swapped':
            base = i0[:, 2] * sx + i0[:, 1] * sy + i0[:, 0]
        else:
            base = i0[:, 0] * sx + i0[:, 1] * sy + i0[:, 2]
        d = np.zeros(x.shape)
        for k in range(8):
            bx, by, bz = k >> 2, (k >> 1) & 1, k & 1
            w = ((t[:, 0] if bx else 1.0 - t[:, 0]) * (t[:, 1] if by else 1.0 - t[:, 1])) * (t[:, 2] if bz else 1.0 - t[:, 2])
            if mistake == 'displace_strides_swapped':
                cell = np.clip(base + bz * sx + by * sy + bx, 0, len(flat) - 1)
            else:
                cell = base + bx * sx + by * sy + bz
            q = flat[cell].astype(F64)
            d = d + q * w[:, None]
        out[inside] = x + d * F64(magnitude)
        branch[inside] = br
    return out, branch


# ----------------------------------------------------------------------------- b2m_aug_vertex_normals (:254-293)
def vertex_csr(faces, n_vert):
    """The vertex-to-face CSR augment.vertex_face_csr builds: occurrences sorted by vertex, stable, so faces ascend in a row."""
    flat = np.asarray(faces, np.int64).reshape(-1)
    order = np.argsort(flat, kind='stable')
    row_ptr = np.searchsorted(flat[order], np.arange(n_vert + 1)).astype(np.int64)
    return row_ptr, (order // 3).astype(np.int64)


def vertex_normals(pos, faces, row_ptr=None, face_of=None, mistake=None):
    """Per vertex: its CSR row in order, one term per entry, components as the kernel writes them, summed from 0.0; normalised; any
    length that is not > 0 gives (0,0,1).  Entries of `face_of` and of `faces` whose VALUES are out of range are skipped (:264-270)."""
    pos = np.asarray(pos, F64)
    n_vert = len(pos)
    faces = np.zeros((0, 3), np.int64) if faces is None else np.asarray(faces, np.int64).reshape(-1, 3)
    n_faces = len(faces)
    if row_ptr is None:
        row_ptr, face_of = vertex_csr(faces, n_vert)
    face_of = np.zeros(0, np.int64) if face_of is None else np.asarray(face_of, np.int64)
    s = np.zeros((n_vert, 3))
    with np.errstate(all='ignore'):
        b = np.maximum(np.asarray(row_ptr[:-1], np.int64), 0)
        e = np.minimum(np.asarray(row_ptr[1:], np.int64), 3 * n_faces)
        for r in range(int(max(0, (e - b).max())) if n_vert else 0):
            v = np.nonzero(e - b > r)[0]
            k = (e[v] - 1 - r) if mistake == 'normals_descending' else (b[v] + r)
            f = face_of[k]
            ok = (f >= 0) & (f < n_faces)
            v, f = v[ok], f[ok]
            tri = faces[f]
            ok = ((tri >= 0) & (tri < n_vert)).all(1)
            v, tri = v[ok], tri[ok]
            p0, p1, p2 = pos[tri[:, 0]], pos[tri[:, 1]], pos[tri[:, 2]]
            ax, ay, az = p1[:, 0] - p0[:, 0], p1[:, 1] - p0[:, 1], p1[:, 2] - p0[:, 2]
            bx, by, bz = p2[:, 0] - p0[:, 0], p2[:, 1] - p0[:, 1], p2[:, 2] - p0[:, 2]
            s[v, 0] = s[v, 0] + (ay * bz - az * by)
            s[v, 1] = s[v, 1] + (az * bx - ax * bz)
            s[v, 2] = s[v, 2] + (ax * by - ay * bx)
        length = np.sqrt(s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2])
        out = np.empty_like(s)
        out[:] = [0.0, 0.0, 0.0] if mistake == 'normals_zero_fallback' else [0.0, 0.0, 1.0]
        ok = length > 0.0
        out[ok] = s[ok] / length[ok, None]
    return out


# ----------------------------------------------------------------------------- b2m_aug_colour (:295-334)
def clip01(v):
    """aug_clip01: v < 0 -> 0, v > 1 -> 1, else v -- a NaN stays a NaN."""
    return np.where(v < 0.0, 0.0, np.where(v > 1.0, 1.0, v))


def colour(col, stats12, flags, blend, tr, jitter, mistake=None):
    v = np.asarray(col, F64).copy()
    blend = F64(blend)
    stages = [1, 2, 4]
    if mistake == 'colour_stage_order':
        stages = [2, 1, 4]
    with np.errstate(all='ignore'):
        for stage in stages:
            if not flags & stage:
                continue
            if stage == 1:
                lo, hi = np.asarray(stats12, F64)[3:6], np.asarray(stats12, F64)[6:9]
                scale = 1.0 / (hi - lo)
                contrast = (v - lo) * scale
                v = (1.0 - blend) * v + blend * contrast
            else:
                add = np.asarray(tr, F64).reshape(1, 3) if stage == 2 else np.asarray(jitter, F64)
                v = (add + clip01(v)) if mistake == 'colour_clip_before_add' else clip01(add + v)
    return v


# ----------------------------------------------------------------------------- b2m_inst_boxes (:336-424)
def ordered(v):
    """aug_ordered: the order-preserving map double -> uint64 the min / max atomics run on (-0.0 sorts below +0.0)."""
    u = np.ascontiguousarray(v, F64).view(np.uint64)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))


def unordered(u):
    u = np.asarray(u, np.uint64)
    return np.where(u >> np.uint64(63), u & np.uint64((1 << 63) - 1), ~u).view(F64)


def inst_boxes(pos, inst, sem, n_inst, mistake=None):
    """dict of everything the entry writes: centers64 (I,3) f64, per_sem (I) i32, per_centers / per_bounds (I,3) f32,
    per_radius (I) f32, offsets (P,3) f32, distances (P) f32, missing int."""
    pos = np.asarray(pos, F64)
    inst = np.asarray(inst, np.int64).reshape(-1)
    sem = np.asarray(sem, np.int64).reshape(-1)
    P = len(pos)
    valid = (inst >= 0) & (inst < n_inst)
    ids = inst[valid]
    if mistake == 'boxes_count_out_of_range':                     # ids clamped into the range instead of skipped
        valid = np.ones(P, bool)
        ids = np.clip(inst, 0, n_inst - 1)
    rows = np.nonzero(valid)[0]
    lo_code = np.full((n_inst, 3), np.iinfo(np.uint64).max, np.uint64)
    hi_code = np.zeros((n_inst, 3), np.uint64)
    codes = ordered(pos[valid])
    for c in range(3):
        np.minimum.at(lo_code[:, c], ids, codes[:, c])
        np.maximum.at(hi_code[:, c], ids, codes[:, c])
    first = np.full(n_inst, P, np.int64)
    np.minimum.at(first, ids, rows)
    if mistake == 'boxes_sem_highest':
        first = np.where(first < P, 0, first)
        np.maximum.at(first, ids, rows)
    have = first < P
    with np.errstate(all='ignore'):
        lo, hi = unordered(lo_code), unordered(hi_code)
        centre = (lo + hi) / 2
        bound = (hi - lo) / 2 if mistake == 'boxes_bound_half_extent' else hi - centre
        centers64 = np.where(have[:, None], centre, 0.0)
        per_centers = centers64.astype(F32)
        per_bounds = np.where(have[:, None], bound, 0.0).astype(F32)
        per_sem = np.where(have, sem[np.where(have, first, 0)], 0).astype(np.int32)
        o = np.zeros((P, 3))
        o[valid] = centers64[ids] - pos[valid]
        d = np.sqrt((o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1]) + o[:, 2] * o[:, 2])
        d[~valid] = 0.0
        offsets, distances = o.astype(F32), d.astype(F32)
        if mistake == 'boxes_radius_f32':
            # (rounding is monotone, so the largest float32 distance IS the rounded largest fp64 distance: taken literally this
            # mistake changes nothing.  What a float32 pipeline would do differently is measure the ROUNDED offsets.)
            o32 = offsets.astype(F64)
            d32 = np.sqrt((o32[:, 0] * o32[:, 0] + o32[:, 1] * o32[:, 1]) + o32[:, 2] * o32[:, 2]).astype(F32)
            r32 = np.zeros(n_inst, F32)
            np.maximum.at(r32, ids, d32[valid])
            per_radius = r32
        else:
            r64 = np.zeros(n_inst)
            np.maximum.at(r64, ids, d[valid])
            per_radius = r64.astype(F32)
    return dict(centers64=centers64, per_sem=per_sem, per_centers=per_centers, per_bounds=per_bounds, per_radius=per_radius,
                offsets=offsets, distances=distances, missing=int((~have).sum()))
