"""Scene preparation restated from the contracts of include/b2m_prepare.h, for tests/test_prepare_rule.py (CPU) and
tests/test_gpu_prepare_edges.py (the kernels of csrc/voxelize.hip).  One small function per entry:

  * shift            min(0, min of all coordinates); 0.0 for an empty scene;
  * voxel index      np.round((pos - shift) / voxel_size) in fp64 (subtract, divide, round half to even), one tuple (x, y, z) per
                     point.  A point is in range when every axis is finite and 0 <= v < 2**21;
  * unique           the tuples sorted by Python's own tuple order (x first), the inverse map read from a dict.  Nothing is packed
                     into a 64-bit key and there is no hash table, so there is no field width, shift or probe this module could get
                     wrong.  Plain 64-bit keys are Python integers, i.e. UNSIGNED: sorted(set(keys));
  * nearest point    for every voxel centre, brute force over ALL points: d = ((vx-px)^2 + (vy-py)^2) + (vz-pz)^2 in fp64 in this
                     order, the lowest point index among equal d.  No neighbourhood and no cut-off;
  * gather           float32 (round to nearest even) of the chosen point's colours [and normals]; its segment id;
  * centroid         Python-integer sums of the voxel indices per segment, then ((float(sum) / float(n)) * voxel_size) + shift:
                     the kernel's own evaluation, bit for bit.  centroid_means() is numpy's mean(vox * vs + shift) instead;
  * box membership   closed intervals; count, first box, smallest box by FLOAT32 volume (first on ties); -1, -1 outside every box;
  * oriented boxes   v_j = (R[j,0]*dx + R[j,1]*dy) + R[j,2]*dz with d = p - c, inside when -h_j <= v_j <= h_j for j = 0, 1, 2;
  * segment vote     per voxel-level segment the point with the smallest (count, index) decides: count 0 -> -1, 1 -> ids[first],
                     more -> ids[smallest] under the heuristic, else -2; points of other segments get -2;
  * segment rank     position of the point's segment in the sorted voxel-level list, -1 when it is not there;
  * segment mode     most frequent class of the points of a segment, the LOWEST class index on ties, points of rank -1 ignored.
                     Convention of the entry: a segment without points gives class 0.

Every function takes `mistake`, which turns it into one deliberate error (MISTAKES below); tests/test_prepare_rule.py shows that
each of them fails a named case of tests/_prepare_cases.py, i.e. that the cases are sharp.
"""
import numpy as np

LIM = 1 << 21

MISTAKES = {
    'half_away': 'round half away from zero',
    'shift_min': 'shift = min(pos) without the min(0, .)',
    'z_major': 'z-major key order',
    'tie_highest': 'highest index on distance ties',
    'own_only': "nearest restricted to the voxel's own points",
    'open': 'open box intervals',
    'vol64': 'smallest box by fp64 volume',
    'last_tie': 'last box on volume ties',
    'lowest_index': 'vote by lowest index alone',
    'highest_class': 'highest class on mode ties',
    'transposed': 'rotation transposed',
    'centroid_points': 'centroid from points instead of voxels',
    'signed': 'signed key comparison',
}


# ----------------------------------------------------------------------------- shift, voxel indices
def shift_of(pos, mistake=None):
    pos = np.asarray(pos, np.float64).reshape(-1)
    if pos.size == 0:
        return 0.0
    m = float(pos.min())
    if mistake == 'shift_min':
        return m
    return m if m < 0.0 else 0.0


def scaled(pos, shift, vs):
    """(pos - shift) / voxel_size in fp64: the points in voxel units."""
    return (np.asarray(pos, np.float64).reshape(-1, 3) - np.float64(shift)) / np.float64(vs)


def voxel_index(pos, shift, vs, mistake=None):
    """(n, 3) float64 of rounded indices (NaN / inf stay what they are)."""
    u = scaled(pos, shift, vs)
    if mistake == 'half_away':
        with np.errstate(invalid='ignore'):
            return np.trunc(u + np.copysign(0.5, u))
    return np.round(u)


def in_range(v):
    with np.errstate(invalid='ignore'):
        return np.isfinite(v).all(1) & (v >= 0).all(1) & (v < LIM).all(1)


def bad_count(v):
    return int((~in_range(v)).sum())


def tuples(v):
    """Rows of in-range indices as tuples of Python integers."""
    return [tuple(int(c) for c in r) for r in np.asarray(v).reshape(-1, 3).tolist()]


def unique_tuples(tup, mistake=None):
    """(sorted distinct tuples, inverse int64)."""
    uniq = sorted(set(tup), key=(lambda t: t[::-1]) if mistake == 'z_major' else None)
    index = {t: i for i, t in enumerate(uniq)}
    return uniq, np.array([index[t] for t in tup], np.int64).reshape(-1)


def unique_keys(keys, mistake=None):
    """np.unique(return_inverse=True) of 64-bit keys given as non-negative Python integers (or a uint64 array)."""
    ks = [int(k) for k in (keys.tolist() if isinstance(keys, np.ndarray) else keys)]
    assert all(0 <= k < (1 << 64) for k in ks)
    uniq = sorted(set(ks), key=(lambda k: k - (1 << 64) if k >= (1 << 63) else k) if mistake == 'signed' else None)
    index = {k: i for i, k in enumerate(uniq)}
    return uniq, np.array([index[k] for k in ks], np.int64).reshape(-1)


# ----------------------------------------------------------------------------- nearest point, gather, centroid
def distances(u, vox):
    """(V, P) fp64: d = ((vx-px)^2 + (vy-py)^2) + (vz-pz)^2."""
    q = np.asarray(vox, np.float64).reshape(-1, 3)
    ex, ey, ez = (q[:, None, j] - u[None, :, j] for j in range(3))
    return (ex * ex + ey * ey) + ez * ez


def nearest(u, vox, mistake=None, chunk=256):
    """(point (V,) int64, d (V,), number of points at that d (V,)).  u: points in voxel units, vox: voxel indices."""
    vox = np.asarray(vox, np.float64).reshape(-1, 3)
    P = len(u)
    own = np.round(u) if mistake == 'own_only' else None
    out, dmin, nties = np.empty(len(vox), np.int64), np.empty(len(vox)), np.empty(len(vox), np.int64)
    for a in range(0, len(vox), chunk):
        d = distances(u, vox[a:a + chunk])
        if own is not None:
            d = np.where((own[None] == vox[a:a + chunk, None]).all(-1), d, np.inf)
        lo = d.min(1)
        pick = (P - 1 - np.argmin(d[:, ::-1], 1)) if mistake == 'tie_highest' else np.argmin(d, 1)
        out[a:a + chunk], dmin[a:a + chunk], nties[a:a + chunk] = pick, lo, (d == lo[:, None]).sum(1)
    return out, dmin, nties


def gather(point2vox, colors, normals=None, segments=None):
    cols = np.asarray(colors, np.float64) if normals is None else np.concatenate([colors, normals], 1)
    feats = cols[point2vox].astype(np.float32)
    return feats, (None if segments is None else np.asarray(segments, np.int64)[point2vox])


def centroids(vox, seg2vox, n_seg, vs, shift):
    """(n_seg, 3) fp64: integer sums, one evaluation per segment."""
    sums, cnt = [[0, 0, 0] for _ in range(n_seg)], [0] * n_seg
    for t, s in zip(tuples(vox), np.asarray(seg2vox).tolist()):
        cnt[s] += 1
        for j in range(3):
            sums[s][j] += t[j]
    out = np.empty((n_seg, 3))
    for s in range(n_seg):
        for j in range(3):
            out[s, j] = ((float(sums[s][j]) / float(cnt[s])) * float(vs)) + float(shift)
    return out


def centroid_means(vox, seg2vox, n_seg, vs, shift, mistake=None, pos=None, vox2point=None):
    """numpy's mean of the voxel centres of every segment; mistake 'centroid_points': of the segment's scene points."""
    out = np.empty((n_seg, 3))
    if mistake == 'centroid_points':
        seg2point = np.asarray(seg2vox)[vox2point]
        for s in range(n_seg):
            out[s] = np.mean(np.asarray(pos)[seg2point == s], axis=0)
        return out
    world = np.asarray(vox, np.float64) * vs + shift
    for s in range(n_seg):
        out[s] = np.mean(world[np.asarray(seg2vox) == s], axis=0)
    return out


# ----------------------------------------------------------------------------- boxes
def box_membership(pos, lo, hi, volume, mistake=None):
    """(count, first_bb, smallest_bb) int32.  volume: any float type; compared as float32."""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    lo, hi = np.asarray(lo, np.float64).reshape(-1, 3), np.asarray(hi, np.float64).reshape(-1, 3)
    vol = np.asarray(volume, np.float64 if mistake == 'vol64' else np.float32).reshape(-1)
    n = len(pos)
    count, first, small = np.zeros(n, np.int32), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    sv = np.zeros(n, vol.dtype)
    for b in range(len(lo)):
        if mistake == 'open':
            inside = (pos > lo[b]).all(1) & (pos < hi[b]).all(1)
        else:
            inside = (pos >= lo[b]).all(1) & (pos <= hi[b]).all(1)
        none = count == 0
        first = np.where(inside & none, b, first).astype(np.int32)
        better = inside & (none | ((vol[b] <= sv) if mistake == 'last_tie' else (vol[b] < sv)))
        small = np.where(better, b, small).astype(np.int32)
        sv = np.where(better, vol[b], sv)
        count = count + inside.astype(np.int32)
    return count, first, small


def obb_membership(pos, centers, rot, half, mistake=None):
    """(count, first_bb) int32; rot: (B, 3, 3) row-major."""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    centers, half = np.asarray(centers, np.float64).reshape(-1, 3), np.asarray(half, np.float64).reshape(-1, 3)
    rot = np.asarray(rot, np.float64).reshape(-1, 3, 3)
    n = len(pos)
    count, first = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    for b in range(len(centers)):
        R = rot[b].T if mistake == 'transposed' else rot[b]
        dx, dy, dz = pos[:, 0] - centers[b, 0], pos[:, 1] - centers[b, 1], pos[:, 2] - centers[b, 2]
        inside = np.ones(n, bool)
        for j in range(3):
            v = (R[j, 0] * dx + R[j, 1] * dy) + R[j, 2] * dz
            inside &= (v >= -half[b, j]) & (v <= half[b, j])
        first = np.where(inside & (count == 0), b, first).astype(np.int32)
        count = count + inside.astype(np.int32)
    return count, first


# ----------------------------------------------------------------------------- segments
def segment_rank(segments, useg):
    rank = {int(s): i for i, s in enumerate(useg)}
    return np.array([rank.get(int(s), -1) for s in np.asarray(segments).tolist()], np.int32).reshape(-1)


def segment_vote(segments, useg, count, first_bb, smallest_bb, ids, heuristic, mistake=None):
    """(inst_per_point int64, inst_per_seg int64, seg_of_point int32)."""
    seg_of_point = segment_rank(segments, useg)
    count = np.asarray(count).tolist()
    best = {}
    for p, r in enumerate(seg_of_point.tolist()):
        if r >= 0:
            key = (0, p) if mistake == 'lowest_index' else (count[p], p)
            if r not in best or key < best[r]:
                best[r] = key
    per_seg = np.full(len(useg), -2, np.int64)
    for r, (_, p) in best.items():
        c = count[p]
        if c == 0:
            per_seg[r] = -1
        elif c == 1:
            per_seg[r] = ids[first_bb[p]]
        elif heuristic:
            per_seg[r] = ids[smallest_bb[p]]
    per_point = np.where(seg_of_point >= 0, per_seg[np.maximum(seg_of_point, 0)] if len(useg) else -2, -2).astype(np.int64)
    return per_point.reshape(-1), per_seg, seg_of_point


def segment_mode(seg_of_point, cls, n_seg, n_class, mistake=None):
    """(n_seg,) int32 class index; a segment without points gives 0."""
    hist = [[0] * n_class for _ in range(n_seg)]
    for r, c in zip(np.asarray(seg_of_point).tolist(), np.asarray(cls).tolist()):
        if r >= 0:
            hist[r][c] += 1
    out = np.zeros(n_seg, np.int32)
    for s in range(n_seg):
        top = max(hist[s])
        hits = [c for c in range(n_class) if hist[s][c] == top]
        out[s] = hits[-1] if mistake == 'highest_class' else hits[0]
    return out


def mode_of_values(seg_of_point, values, n_seg, mistake=None):
    """The most frequent VALUE per segment, the smallest on ties: classes are the distinct values in ascending order."""
    uniq = sorted(set(np.asarray(values).tolist()))
    index = {v: i for i, v in enumerate(uniq)}
    cls = [index[v] for v in np.asarray(values).tolist()]
    m = segment_mode(seg_of_point, cls, n_seg, max(len(uniq), 1), mistake)
    return np.array([uniq[c] for c in m.tolist()], np.int64).reshape(-1)


def pooling_ids(per_scene_segments):
    """to_unique over the scenes of a batch: rank of the voxel's segment within its scene plus the number of distinct segments
    of the earlier scenes."""
    out, base = [], 0
    for seg in per_scene_segments:
        uniq, inv = unique_keys([int(s) for s in np.asarray(seg).tolist()])
        out.append(inv + base)
        base += len(uniq)
    return np.concatenate(out).astype(np.int64)


# ----------------------------------------------------------------------------- the voxelisation block as a whole
def voxelize_scene(positions, colors, normals, segments, vs, use_normals=True, mistake=None):
    pos = np.asarray(positions, np.float64).reshape(-1, 3)
    shift = shift_of(pos, mistake)
    u = scaled(pos, shift, vs)
    v = voxel_index(pos, shift, vs, mistake)
    assert bad_count(v) == 0
    uniq, vox2point = unique_tuples(tuples(v), mistake)
    vox = np.array(uniq, np.float64).reshape(-1, 3)
    point2vox, dmin, nties = nearest(u, vox, mistake)
    feats, vox_segments = gather(point2vox, colors, normals if use_normals else None, segments)
    useg, seg2vox = unique_keys(vox_segments)
    middle = centroids(vox, seg2vox, len(useg), vs, shift)
    return {'shift': shift, 'vox_coords': vox, 'vox2point': vox2point, 'point2vox': point2vox, 'vox_segments': vox_segments,
            'vox_features': feats, 'vox_world_coords': vox * vs + shift, 'seg2vox': seg2vox, 'seg2point': seg2vox[vox2point],
            'input_location': middle,
            'input_location_mean': centroid_means(vox, seg2vox, len(useg), vs, shift, mistake, pos, vox2point),
            'unique_vox_segments': np.array(useg, np.int64), 'nearest_d': dmin, 'nearest_ties': nties}


# ----------------------------------------------------------------------------- the three associations
# The weak boxes come as float32 centres and half sizes; the margin is added and the corners and volumes are formed in float32, as
# arrays of that type do; membership is then decided in fp64 on those float32 values.
def _point_votes(count, first, small, ids, heuristic):
    out = np.full(len(count), -1, np.int64)
    for p, c in enumerate(count.tolist()):
        if c == 1:
            out[p] = ids[first[p]]
        elif c > 1:
            out[p] = ids[small[p]] if heuristic else -2
    return out


def scannet_association(pos, segments, labels, useg, heuristic, how='segment', mistake=None):
    """how: 'segment' (the vote), 'point', 'majority'."""
    sem = np.asarray(labels['per_instance_semantics'])
    fg = (sem > 2) & (sem != 22)
    centers = np.asarray(labels['per_instance_bb_centers'], np.float32)[fg]
    bounds = np.asarray(labels['per_instance_bb_bounds'], np.float32)[fg] + np.float32(0.005)
    ids = np.asarray(labels['unique_instances'])[fg]
    volume = np.prod(np.float32(2) * bounds, axis=1, dtype=np.float32)
    count, first, small = box_membership(pos, centers - bounds, centers + bounds, volume, mistake)
    if how == 'segment':
        return segment_vote(segments, useg, count, first, small, ids, heuristic, mistake)[:2]
    per_point = _point_votes(count, first, small, ids, heuristic)
    if how == 'point':
        return per_point, None
    rank = segment_rank(segments, useg)
    per_seg = mode_of_values(rank, per_point, len(useg), mistake)
    return np.where(rank >= 0, per_seg[np.maximum(rank, 0)], -2).astype(np.int64), per_seg


def arkit_association(pos, segments, labels, useg, point_association, mistake=None):
    ids = np.asarray(labels['unique_instances'])
    half = np.asarray(labels['per_instance_bb_bounds'], np.float32) + np.float32(0.05)
    count, first = obb_membership(pos, np.asarray(labels['per_instance_bb_centers']), labels['per_instance_bb_rotations'], half, mistake)
    if point_association:
        return _point_votes(count, first, first, ids, False), None
    return segment_vote(segments, useg, count, first, first, ids, False, mistake)[:2]


def s3dis_association(pos, segments, labels, useg, point_association, ignore_wall_ceiling_floor, mistake=None):
    sem_i = np.asarray(labels['per_instance_semantics'])
    fg = (sem_i > 2) if ignore_wall_ceiling_floor else (sem_i >= 0)
    n = len(pos)
    inst, sem = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    for part, sel in enumerate((fg, ~fg)):                       # foreground boxes first, background boxes for what is left
        ids, sids = np.asarray(labels['unique_instances'])[sel], sem_i[sel]
        centers = np.asarray(labels['per_instance_bb_centers'], np.float32)[sel]
        bounds = np.asarray(labels['per_instance_bb_bounds'], np.float32)[sel] + np.float32(0.0001)
        count, first, _ = box_membership(pos, centers - bounds, centers + bounds, np.zeros(len(ids), np.float32), mistake)
        free = (inst == -1) if part == 1 else np.ones(n, bool)
        for p in np.flatnonzero(free & (count == 1)).tolist():
            inst[p], sem[p] = ids[first[p]], sids[first[p]]
        inst[free & (count > 1)], sem[free & (count > 1)] = -2, -100
    inst[inst == -1], sem[sem == -1] = -2, -100
    if point_association:
        return inst, sem
    rank = segment_rank(segments, useg)
    per_seg, sem_seg = mode_of_values(rank, inst, len(useg), mistake), mode_of_values(rank, sem, len(useg), mistake)
    return np.where(rank >= 0, per_seg[np.maximum(rank, 0)], -1).astype(np.int64), sem, per_seg, sem_seg
