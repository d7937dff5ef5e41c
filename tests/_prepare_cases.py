"""The edge cases of scene preparation, shared by tests/test_prepare_rule.py (CPU: every case is built, its predicates hold, every
deliberate mistake of _prepare_rule.MISTAKES fails a named case) and tests/test_gpu_prepare_edges.py (the same cases through the
entries of include/b2m_prepare.h).  A case is a name, its inputs and PREDICATES: facts computed by the rule that say which edge the
case reaches ("some voxel's winner lies in a face-neighbour cell").  They are asserted when the case is built, so a case that no
longer reaches its edge fails on the CPU.

Inputs are dyadic wherever an entry computes in floating point (voxel size 0.5 or 0.25, coordinates multiples of 2^-6, rotations
that permute the axes), so no order of evaluation can matter; every floating-point entry also has one full-mantissa random case
('*:mantissa'), where the order the contract states decides.  Nothing here leaves an entry's contract: classes lie in
[0, n_class), seg2vox in [0, n_seg), point2vox inside the points, and no key is 2^64-1.

Only this module packs (x, y, z) into x<<42 | y<<21 | z, and only to feed entries that take packed keys; the rule never does.
"""
import functools
from types import SimpleNamespace

import numpy as np

import _prepare_rule as R

SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097)          # "N" of the issue
TOP = R.LIM - 1


def _case(name, predicates, **inputs):
    assert predicates, name
    bad = [k for k, v in predicates.items() if not v]
    assert not bad, (name, bad)
    return SimpleNamespace(name=name, predicates=predicates, **inputs)


def _rng(name):
    return np.random.default_rng(sum(ord(c) * (i + 1) for i, c in enumerate(name)))


def _dyadic(rng, shape, lo, hi, bits=6):
    """Random multiples of 2^-bits in [lo, hi)."""
    return rng.integers(int(lo * (1 << bits)), int(hi * (1 << bits)), shape).astype(np.float64) / (1 << bits)


def pack(t):
    return (t[0] << 42) | (t[1] << 21) | t[2]


def unpack(k):
    k = int(k)
    return (k >> 42, (k >> 21) & TOP, k & TOP)


# ----------------------------------------------------------------------------- b2m_vox_shift
SHIFT_CASES = tuple('n:%d' % n for n in SIZES + (100003,)) + ('all_positive', 'min_first', 'min_last', 'negative_zero', 'empty')


@functools.lru_cache(maxsize=None)
def shift_case(name):
    rng = _rng('shift' + name)
    if name.startswith('n:'):
        n = int(name[2:])
        pos = _dyadic(rng, (n, 3), -40, 40)
        pos[rng.integers(n), rng.integers(3)] = -41.5
        pred = {'n points': len(pos) == n, 'a negative minimum': R.shift_of(pos) == -41.5}
    elif name == 'all_positive':
        pos = _dyadic(rng, (257, 3), 1, 40)
        pred = {'all positive': pos.min() > 0, 'shift is 0': R.shift_of(pos) == 0.0, 'min(pos) is not': pos.min() != 0.0}
    elif name in ('min_first', 'min_last'):
        pos = _dyadic(rng, (4097, 3), -40, 40)
        at = 0 if name == 'min_first' else pos.size - 1
        pos.reshape(-1)[at] = -77.25
        pred = {'the minimum is there and nowhere else': int(np.argmin(pos)) == at and (pos == pos.min()).sum() == 1}
    elif name == 'negative_zero':
        pos = np.full((65, 3), -0.0)
        pred = {'all -0.0': bool(np.signbit(pos).all()), 'shift is +0.0': not np.signbit(R.shift_of(pos))}
    else:
        pos = np.zeros((0, 3))
        pred = {'empty': pos.size == 0 and R.shift_of(pos) == 0.0}
    return _case(name, pred, pos=pos)


# ----------------------------------------------------------------------------- b2m_vox_keys
KEY_CASES = tuple('n:%d' % n for n in SIZES) + ('halves', 'halves_negative_shift', 'top', 'bad:1', 'bad:3', 'bad:all', 'empty',
                                                 'mantissa')


@functools.lru_cache(maxsize=None)
def key_case(name):
    """pos, shift (given to the entry), vs."""
    rng = _rng('keys' + name)
    vs, shift = 0.25, None
    if name.startswith('n:'):
        n = int(name[2:])
        pos = _dyadic(rng, (n, 3), -3, 5)
        pos[rng.integers(n)] = -3.0
        pred = {'n points': len(pos) == n, 'negative shift': R.shift_of(pos) == -3.0}
    elif name.startswith('halves'):
        vs = 0.5
        k = np.arange(6) + 0.5
        pos = np.stack(np.meshgrid(k, k, k, indexing='ij'), -1).reshape(-1, 3) * vs
        if name.endswith('negative_shift'):
            pos = np.concatenate([pos, [[-1.5, 0.25, 0.25]]])
        u = R.scaled(pos, R.shift_of(pos), vs)
        fl = np.floor(u[:216])
        pred = {'every coordinate is k + 0.5': bool((u[:216] - fl == 0.5).all()),
                'k even and odd on each axis': all(set((fl[:, j] % 2).tolist()) == {0.0, 1.0} for j in range(3)),
                'six values per axis': all(len(set(fl[:, j].tolist())) == 6 for j in range(3)),
                'shift as named': (R.shift_of(pos) < 0) == name.endswith('negative_shift'),
                'half away from zero differs': not np.array_equal(R.voxel_index(pos, R.shift_of(pos), vs),
                                                                  R.voxel_index(pos, R.shift_of(pos), vs, 'half_away'))}
    elif name == 'top':
        vs = 1.0
        pos = np.array([[TOP, 0, 0], [0, TOP, 0], [0, 0, TOP], [TOP, TOP, TOP], [TOP + 0.4375, TOP - 0.5, 0.5], [0, 0, 0]], np.float64)
        v = R.voxel_index(pos, 0.0, vs)
        pred = {'all accepted': R.bad_count(v) == 0, '2^21-1 on each axis': all((v[:, j] == TOP).any() for j in range(3)),
                'key bit 62': any(t[0] >> 20 for t in R.tuples(v))}
    elif name.startswith('bad:'):
        vs = 1.0
        pos = _dyadic(rng, (65, 3), 0, 100)
        if name == 'bad:1':
            pos[17, 1] = R.LIM
        elif name == 'bad:3':
            pos[0, 2], pos[33, 0], pos[64, 1] = np.nan, np.inf, TOP + 0.5          # (2^21 - 0.5 rounds to the even 2^21)
        else:
            pos[:, 0], pos[::2, 1], pos[1::3, 2] = R.LIM, np.nan, np.inf
        want = {'bad:1': 1, 'bad:3': 3, 'bad:all': 65}[name]
        pred = {'the rule counts %d' % want: R.bad_count(R.voxel_index(pos, 0.0, vs)) == want}
        shift = 0.0
    elif name == 'empty':
        pos = np.zeros((0, 3))
        pred = {'empty': len(pos) == 0}
    else:
        vs = 0.02
        pos = rng.uniform(-0.83, 7.0, (4097, 3))
        u = R.scaled(pos, R.shift_of(pos), vs)
        pred = {'full mantissa': bool((np.frexp(pos)[0] * (1 << 53) % 2 == 1).mean() > 0.3),
                'no coordinate near a half': bool((np.abs(u - np.floor(u) - 0.5) > 1e-9).all())}
    shift = R.shift_of(pos) if shift is None else shift
    return _case(name, pred, pos=pos, vs=vs, shift=shift)


# ----------------------------------------------------------------------------- unique / sort / rank / decode
CHAIN_CASES = ('distinct:4096', 'distinct:8192') + tuple('single:%d' % n for n in SIZES) + (
    'wave:8x8', 'wave:7of64', 'wave:17', 'wave:33', 'tail:65', 'tail:127', 'fields', 'high_bit')


def _vox_keys(rng, n):
    """n distinct voxel tuples over the whole range, bit 62 set in about half of them."""
    t = set()
    while len(t) < n:
        for r in rng.integers(0, R.LIM, (n, 3)).tolist():
            t.add(tuple(r))
    return sorted(t)[:n]


@functools.lru_cache(maxsize=None)
def chain_case(name):
    """keys: Python integers (the entry's input order); tup: the voxel tuples they pack, or None for plain 64-bit keys;
    n_pad: the padded length the sort is run at (None: the next power of two of the number of distinct keys)."""
    rng = _rng('chain' + name)
    kind, _, arg = name.partition(':')
    tup, n_pad = None, None
    if kind == 'distinct':
        n = int(arg)
        tup = _vox_keys(rng, n)
        tup = [tup[i] for i in rng.permutation(n)]
        keys = [pack(t) for t in tup]
        n_pad = 2 * n
        pred = {'all distinct': len(set(keys)) == n, 'load exactly 0.5 at cap = 2n': (2 * n) & (2 * n - 1) == 0,
                'bit 62': any(k >> 62 for k in keys), 'padding': n_pad > n,
                'global stages': (n_pad // 4096).bit_length() - 1 == {4096: 1, 8192: 2}[n]}
    elif kind == 'single':
        n = int(arg)
        tup = [(TOP, 5, TOP)] * n
        keys = [pack(t) for t in tup]
        pred = {'n copies of one key': len(keys) == n and len(set(keys)) == 1, 'bit 62': keys[0] >> 62 == 1}
    elif kind == 'wave':
        base = _vox_keys(rng, 64)
        if arg == '8x8':
            tup = [base[i % 8] for i in range(64)]
            pred = {'leader group x 8 == 64: the election goes on': tup.count(tup[0]) * 8 == 64, '8 keys': len(set(tup)) == 8}
        elif arg == '7of64':
            tup = [base[0]] * 7 + base[1:58]
            tup = [tup[0]] + [tup[i] for i in (1 + rng.permutation(63))]
            pred = {'leader group x 8 < 64: per-lane path': tup.count(tup[0]) * 8 == 56, '58 keys': len(set(tup)) == 58}
        elif arg == '17':
            tup = [base[0]] * 16 + [base[1 + i % 16] for i in range(48)]
            tup = [tup[0]] + [tup[i] for i in (1 + rng.permutation(63))]
            pred = {'elected': tup.count(tup[0]) * 8 >= 64, '17 keys, each repeated': len(set(tup)) == 17 and min(map(tup.count, tup)) >= 3}
        else:
            tup = [base[0]] * 8 + [base[1 + i % 32] for i in range(56)]
            tup = [tup[0]] + [tup[i] for i in (1 + rng.permutation(63))]
            pred = {'elected': tup.count(tup[0]) * 8 >= 64, '33 keys': len(set(tup)) == 33,
                    '17 keys left after 16 rounds': len(set(tup)) - 16 == 17}
        pred['one wave'] = len(tup) == 64
        keys = [pack(t) for t in tup]
    elif kind == 'tail':
        n = int(arg)
        base = _vox_keys(rng, 5)
        tup = [base[i] for i in rng.integers(0, 5, n)]
        keys = [pack(t) for t in tup]
        pred = {'a partial last wave': n % 64 != 0 and n > 64, 'repeated keys': len(set(keys)) == 5}
    elif kind == 'fields':
        tup = [(a, b, c) for a in (0, 1, TOP) for b in (0, 1, TOP) for c in (0, 1, TOP)]
        tup = [tup[i] for i in rng.permutation(27)] * 3
        keys = [pack(t) for t in tup]
        pred = {'every field at 0 and at 2^21-1': True, 'x-major differs from z-major': R.unique_tuples(tup)[0] != R.unique_tuples(tup, 'z_major')[0]}
    else:
        keys = [int(k) for k in rng.integers(0, 1 << 63, 300, dtype=np.uint64).tolist()]
        keys = keys + [k | (1 << 63) for k in keys[:150]] + [(1 << 64) - 2, 1 << 63, 0, (1 << 63) - 1] * 2
        keys = [keys[i] for i in rng.permutation(len(keys))]
        pred = {'keys on both sides of 2^63': min(keys) < (1 << 63) <= max(keys), 'the reserved key is absent': (1 << 64) - 1 not in keys,
                'signed order differs': R.unique_keys(keys)[0] != R.unique_keys(keys, 'signed')[0]}
    return _case(name, pred, keys=keys, tup=tup, n_pad=n_pad)


# ----------------------------------------------------------------------------- b2m_vox_nearest
NEAREST_CASES = ('n:1', 'n:64', 'n:257', 'n:4097', 'face', 'edge', 'corner_loses', 'tie_075', 'tie_neighbour', 'duplicates',
                 'range_ends', 'negative_shift', 'mantissa')


def _winner_offsets(res, u):
    """Per voxel: number of axes on which the winner's own voxel differs from the voxel."""
    return (np.round(u)[res['point2vox']] != res['vox_coords']).sum(1)


@functools.lru_cache(maxsize=None)
def nearest_case(name):
    """pos, vs.  Coordinates are given in voxel units `u` and scaled by vs = 0.5 (exact)."""
    rng = _rng('nearest' + name)
    vs, off = 0.5, 0.0
    if name.startswith('n:'):
        n = int(name[2:])
        side = {1: 1, 64: 3, 257: 4, 4097: 7}[n]
        u = _dyadic(rng, (n, 3), 0, side, bits=3)
    elif name == 'face':
        u = np.array([[2.4375, 2.4375, 2.4375], [2.53125, 2, 2]])
    elif name == 'edge':
        u = np.array([[2.4375, 2.4375, 2.4375], [2.53125, 2.53125, 2]])
    elif name == 'corner_loses':
        u = np.array([[2.51, 2.51, 2.51], [2.5, 2.5, 2.5]])
    elif name == 'tie_075':
        u = np.array([[0, 0, 0], [2.5, 2.5, 2.5], [1.5, 1.5, 1.5], [2.5, 1.5, 2.5]])
    elif name == 'tie_neighbour':
        u = np.array([[1.5, 1.125, 1.125], [1.375, 1.375, 1.0]])
    elif name == 'duplicates':
        u = np.repeat(_dyadic(rng, (9, 3), 0, 3, bits=3), 8, 0)[rng.permutation(72)]
    elif name == 'range_ends':
        u = np.array([[0, 0, 0], [0.25, 0, 0.4375], [TOP, TOP, TOP], [TOP - 0.25, TOP, 0], [TOP, 0.375, TOP - 0.125], [0, TOP, 0.25]], np.float64)
    elif name == 'negative_shift':
        u, off = _dyadic(rng, (257, 3), 0, 4, bits=3), -2.75
    else:
        vs, off = 0.02, -0.83
        u = rng.uniform(0, 9.0, (4097, 3))
    pos = u * vs + off
    res = R.voxelize_scene(pos, np.zeros_like(pos), None, np.zeros(len(pos), np.int64), vs, use_normals=False)
    uu = R.scaled(pos, res['shift'], vs)
    far = _winner_offsets(res, uu)
    d, ties = res['nearest_d'], res['nearest_ties']
    pred = {'every voxel has a point within 0.75': bool((d <= 0.75).all())}
    if name.startswith('n:'):
        pred['n points'] = len(pos) == int(name[2:])
        if len(pos) > 64:
            pred['winners in neighbour cells'] = bool((far > 0).any())
            pred['exact ties'] = bool((ties > 1).any())
    elif name in ('face', 'edge'):
        pred['a winner in a %s-neighbour cell' % name] = bool((far == {'face': 1, 'edge': 2}[name]).any())
    elif name == 'corner_loses':
        dd = R.distances(uu, res['vox_coords'])
        v = R.tuples(res['vox_coords']).index((2, 2, 2))
        pred.update({'the corner neighbour is at 0.7803 > 0.75': 0.78 < dd[v, 0] < 0.7804 and tuple(np.round(uu[0])) == (3, 3, 3),
                     'the own point at exactly 0.75 wins': dd[v, 1] == 0.75 and res['point2vox'][v] == 1})
    elif name == 'tie_075':
        v = R.tuples(res['vox_coords']).index((2, 2, 2))
        pred.update({'three own points at exactly 0.75': d[v] == 0.75 and ties[v] == 3 and bool((far[v] == 0)),
                     'the lowest index wins': res['point2vox'][v] == 1,
                     'highest-index differs': R.nearest(uu, res['vox_coords'], 'tie_highest')[0][v] == 3})
    elif name == 'tie_neighbour':
        v = R.tuples(res['vox_coords']).index((1, 1, 1))
        pred.update({'own and neighbour tie at 18/64': d[v] == 18 / 64 and ties[v] == 2,
                     'the neighbour has the lower index and wins': res['point2vox'][v] == 0 and far[v] == 1})
    elif name == 'duplicates':
        pred['every voxel ties among duplicates'] = bool((ties >= 8).all())
    elif name == 'range_ends':
        t = R.tuples(res['vox_coords'])
        pred.update({'voxels at 0 and at 2^21-1 on each axis': (0, 0, 0) in t and (TOP, TOP, TOP) in t, 'shift 0': res['shift'] == 0.0})
    elif name == 'negative_shift':
        pred['negative shift'] = res['shift'] == -2.75 + float(u.min()) * vs and res['shift'] < 0
    else:
        pred.update({'no exact tie': bool((ties == 1).all()), 'winners in neighbour cells': bool((far > 0).any())})
    return _case(name, pred, pos=pos, vs=vs, rule=res)


# ----------------------------------------------------------------------------- b2m_vox_gather
GATHER_CASES = ('one', 'halfway', 'many')


@functools.lru_cache(maxsize=None)
def gather_case(name):
    rng = _rng('gather' + name)
    if name == 'one':
        colors, normals, p2v = rng.uniform(0, 1, (3, 3)), rng.normal(size=(3, 3)), np.array([2], np.int32)
        pred = {'one voxel': len(p2v) == 1}
    elif name == 'halfway':
        e = 2.0 ** -24
        colors = np.array([[1 + e, 1 + 3 * e, 1 + 5 * e], [-(1 + e), -(1 + 3 * e), 0.5 + e / 2], [2 + 2 * e, 2 + 6 * e, 1 - e / 2]])
        normals = -colors[::-1]
        p2v = np.array([2, 0, 1, 0], np.int32)
        f = colors.astype(np.float32).astype(np.float64)
        up, dn = np.nextafter(f.astype(np.float32), np.float32(np.inf)).astype(np.float64), np.nextafter(f.astype(np.float32), np.float32(-np.inf)).astype(np.float64)
        half = (np.abs(colors - f) == np.abs(up - f) / 2) | (np.abs(colors - f) == np.abs(f - dn) / 2)
        pred = {'every colour is half-way between two float32': bool(half.all()),
                'rounds to the even mantissa': bool((f.astype(np.float32).view(np.uint32) % 2 == 0).all()),
                'up and down both occur': bool((f > colors).any() and (f < colors).any())}
    else:
        colors, normals = rng.uniform(0, 1, (300, 3)), rng.normal(size=(300, 3))
        p2v = rng.integers(0, 300, 257).astype(np.int32)
        pred = {'more than one block': len(p2v) > 256, 'full mantissa': True}
    return _case(name, pred, colors=colors, normals=normals, point2vox=p2v, segments=_rng(name).integers(0, 1 << 40, len(colors)))


# ----------------------------------------------------------------------------- b2m_seg_centroid
CENTROID_CASES = ('one_each', 'one_segment', 'near_top', 'negative_shift', 'empty', 'mantissa')


@functools.lru_cache(maxsize=None)
def centroid_case(name):
    rng = _rng('centroid' + name)
    vs, shift = 0.25, 0.0
    if name == 'one_each':
        vox, seg = rng.integers(0, 50, (257, 3)), rng.permutation(257)
        pred = {'one voxel per segment': len(set(seg.tolist())) == 257}
    elif name == 'one_segment':
        vox, seg = rng.integers(0, 50, (257, 3)), np.zeros(257, np.int64)
        pred = {'one segment': True}
    elif name == 'near_top':
        vox, seg = rng.integers(R.LIM - 64, R.LIM, (4097, 3)), np.repeat([0, 1], [4096, 1])
        pred = {'a sum above 2^32': int(vox[:4096, 0].sum()) > (1 << 32), 'the index 2^21-1': bool((vox == TOP).any())}
    elif name == 'negative_shift':
        vox, seg, shift = rng.integers(0, 9, (65, 3)), rng.integers(0, 7, 65), -3.125
        seg[:7] = np.arange(7)
        pred = {'negative shift': shift < 0}
    elif name == 'empty':
        vox, seg = np.zeros((0, 3), np.int64), np.zeros(0, np.int64)
        pred = {'no segment': True}
    else:
        vox, seg, vs, shift = rng.integers(0, 700, (4097, 3)), rng.integers(0, 33, 4097), 0.02, -0.8300000001
        seg[:33] = np.arange(33)
        a, b = R.centroids(vox, seg, 33, vs, shift), R.centroid_means(vox, seg, 33, vs, shift)
        pred = {'the integer form is not numpy\'s mean bit for bit': not np.array_equal(a, b),
                'but agrees to 1e-12': bool(np.allclose(a, b, rtol=1e-12, atol=1e-12))}
    n_seg = int(seg.max()) + 1 if len(seg) else 0
    pred['every segment has a voxel'] = len(set(np.asarray(seg).tolist())) == n_seg
    return _case(name, pred, vox=np.asarray(vox, np.int64), seg2vox=np.asarray(seg, np.int64), n_seg=n_seg, vs=vs, shift=shift)


# ----------------------------------------------------------------------------- b2m_box_membership
BOX_NB, BOX_NP = (0, 1, 2, 1023, 1024), (1, 255, 256, 257)
BOX_CASES = tuple('size:%d:%d' % (b, p) for b in BOX_NB for p in BOX_NP) + ('faces', 'inverted', 'equal_volumes', 'f32_volume_tie',
                                                                           'outside', 'mantissa')


def _random_boxes(rng, nb, dyadic=True):
    hmax = 3 if nb < 600 else 0.75                             # (about one box per point at 1024 boxes)
    c = _dyadic(rng, (nb, 3), -4, 4) if dyadic else rng.uniform(-4, 4, (nb, 3))
    h = _dyadic(rng, (nb, 3), 0, hmax) if dyadic else rng.uniform(0, hmax, (nb, 3))
    vol = rng.integers(1, 6, nb).astype(np.float64)            # few distinct volumes: ties everywhere
    return c - h, c + h, vol


@functools.lru_cache(maxsize=None)
def box_case(name):
    rng = _rng('box' + name)
    if name.startswith('size:'):
        nb, n = (int(x) for x in name.split(':')[1:])
        lo, hi, vol = _random_boxes(rng, nb)
        pos = _dyadic(rng, (n, 3), -4, 4)
        if nb >= 1023:
            lo[-1], hi[-1] = pos[-1] - 0.25, pos[-1] + 0.25
        c, f, s = R.box_membership(pos, lo, hi, vol)
        pred = {'sizes': (len(lo), len(pos)) == (nb, n)}
        if nb >= 1023 and n >= 255:
            pred.update({'points in no, one and several boxes': {0, 1}.issubset(c.tolist()) and c.max() > 1,
                         'the smallest box is not always the first': bool((f != s).any()),
                         'volume ties among the boxes of a point': not np.array_equal(s, R.box_membership(pos, lo, hi, vol, 'last_tie')[2])})
        if nb >= 1023:
            pred['the last box holds a point'] = bool(((pos >= lo[-1]).all(1) & (pos <= hi[-1]).all(1)).any())
    elif name == 'faces':
        lo, hi, vol = np.array([[-1.0, -2.0, -3.0]]), np.array([[1.5, 2.5, 3.5]]), np.array([1.0])
        pos = []
        for j in range(3):
            for face, out in ((lo[0, j], -np.inf), (hi[0, j], np.inf)):
                for x in (face, np.nextafter(face, out)):
                    p = [0.25, 0.25, 0.25]
                    p[j] = x
                    pos.append(p)
        pos = np.array(pos)
        c = R.box_membership(pos, lo, hi, vol)[0]
        pred = {'on each face: inside; one ulp outside: outside': c.tolist() == [1, 0] * 6,
                'open intervals differ': R.box_membership(pos, lo, hi, vol, 'open')[0].tolist() == [0] * 12}
    elif name == 'inverted':
        lo, hi, vol = np.array([[1.0, -1, -1], [-1, -1, -1.0]]), np.array([[-1.0, 1, 1], [1, 1, 1.0]]), np.array([1.0, 2.0])
        pos = np.array([[0.0, 0, 0], [1.0, 0, 0], [-1.0, 0, 0]])
        pred = {'the inverted box holds nothing': R.box_membership(pos, lo, hi, vol)[1].tolist() == [1, 1, 1]}
    elif name == 'equal_volumes':
        lo, hi = np.full((4, 3), -1.0), np.full((4, 3), 1.0)
        vol = np.array([2.0, 1.0, 1.0, 1.0])
        pos = np.zeros((3, 3))
        s = R.box_membership(pos, lo, hi, vol)[2]
        pred = {'the first of the smallest': s.tolist() == [1, 1, 1], 'not the last': R.box_membership(pos, lo, hi, vol, 'last_tie')[2][0] == 3}
    elif name == 'f32_volume_tie':
        lo, hi = np.full((2, 3), -1.0), np.full((2, 3), 1.0)
        vol = np.array([1.0 + 2.0 ** -30, 1.0])
        pos = np.zeros((2, 3))
        pred = {'fp64 volumes differ': vol[1] < vol[0], 'float32 volumes are equal': np.float32(vol[0]) == np.float32(vol[1]),
                'the first wins': R.box_membership(pos, lo, hi, vol)[2].tolist() == [0, 0],
                'by fp64 volume the second would': R.box_membership(pos, lo, hi, vol, 'vol64')[2].tolist() == [1, 1]}
    elif name == 'outside':
        lo, hi, vol = _random_boxes(rng, 7)
        pos = np.full((5, 3), 100.0)
        pred = {'0, -1, -1': [x.tolist() for x in R.box_membership(pos, lo, hi, vol)] == [[0] * 5, [-1] * 5, [-1] * 5]}
    else:
        lo, hi, _ = _random_boxes(rng, 257, dyadic=False)
        vol = np.prod(hi - lo, axis=1)
        pos = rng.uniform(-4, 4, (4097, 3))
        c = R.box_membership(pos, lo, hi, vol)[0]
        pred = {'full mantissa': True, 'points in several boxes': int(c.max()) > 1}
    return _case(name, pred, pos=pos, lo=lo, hi=hi, volume=vol)


# ----------------------------------------------------------------------------- b2m_obb_membership
OBB_NB, OBB_NP = (0, 1, 255, 256, 257, 513), (1, 255, 256, 257)
OBB_CASES = tuple('size:%d:%d' % (b, p) for b in OBB_NB for p in OBB_NP) + ('faces:identity', 'faces:z90', 'faces:cyclic',
                                                                           'later_chunk', 'mantissa')
ROT_I = np.eye(3)
ROT_Z90 = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
ROT_CYC = np.array([[0.0, 1, 0], [0, 0, 1], [1, 0, 0]])            # a quarter turn about z, then one about x: (dx,dy,dz) -> (dy,dz,dx)
_ROTS = (ROT_I, ROT_Z90, ROT_Z90 @ ROT_Z90, ROT_CYC, ROT_CYC.T)


@functools.lru_cache(maxsize=None)
def obb_case(name):
    rng = _rng('obb' + name)
    if name.startswith('size:'):
        nb, n = (int(x) for x in name.split(':')[1:])
        centers, half = _dyadic(rng, (nb, 3), -4, 4), _dyadic(rng, (nb, 3), 0, 0.75 if nb > 256 else 1.5)
        rot = np.stack([_ROTS[i] for i in rng.integers(0, len(_ROTS), nb)]) if nb else np.zeros((0, 3, 3))
        pos = _dyadic(rng, (n, 3), -4, 4)
        c, f = R.obb_membership(pos, centers, rot, half)
        pred = {'sizes': (len(centers), len(pos)) == (nb, n)}
        if nb >= 255 and n >= 255:
            pred.update({'points in no, one and several boxes': {0, 1}.issubset(c.tolist()) and c.max() > 1,
                         'a transposed rotation differs': not np.array_equal(c, R.obb_membership(pos, centers, rot, half, 'transposed')[0])})
        if nb > 256:
            centers[-1], half[-1] = pos[-1], 0.25
            c, f = R.obb_membership(pos, centers, rot, half)
            pred['the last box holds a point'] = bool(c[-1] >= 1)
        if nb > 256 and n >= 255:
            pred['a first box in a later chunk'] = int(f.max()) >= 256
        if nb > 256 and n == 1:
            pred['one point: 255 idle threads load the chunks'] = True
    elif name.startswith('faces:'):
        rot = {'identity': ROT_I, 'z90': ROT_Z90, 'cyclic': ROT_CYC}[name[6:]][None]
        # centres farther out than the half sizes: p - c is then exact for p on a face and for p one ulp beyond it
        centers, half = np.array([[8.0, -8.0, 16.0]]), np.array([[1.0, 2.0, 3.0]])
        pos = []
        for j in range(3):                                       # the face v_j = +-h_j, and the world point one ulp beyond it
            a = int(np.argmax(np.abs(rot[0, j])))                # the world axis that v_j reads
            for sgn in (-1.0, 1.0):
                v = np.array([0.25, 0.25, 0.25])
                v[j] = sgn * half[0, j]
                p = rot[0].T @ v + centers[0]
                q = p.copy()
                q[a] = np.nextafter(p[a], sgn * rot[0, j, a] * np.inf)
                pos += [p, q]
        pos = np.array(pos)
        back = (rot[0] @ (pos - centers[0]).T).T
        c = R.obb_membership(pos, centers, rot, half)[0]
        pred = {'the faces are exact in the box frame': bool((np.abs(back[::2]).max(1) == half[0].repeat(2)).all()),
                'on each face: inside; one ulp outside: outside': c.tolist() == [1, 0] * 6}
        if name == 'faces:cyclic':
            pred['a transposed rotation differs'] = R.obb_membership(pos, centers, rot, half, 'transposed')[0].tolist() != c.tolist()
        if name == 'faces:z90':
            pred['transposing a quarter turn about z cannot differ on a symmetric box'] = \
                R.obb_membership(pos, centers, rot, half, 'transposed')[0].tolist() == c.tolist()
    elif name == 'later_chunk':
        centers = np.concatenate([np.full((300, 3), 50.0), np.zeros((213, 3))])
        half, rot = np.full((513, 3), 1.0), np.stack([_ROTS[i % len(_ROTS)] for i in range(513)])
        pos = _dyadic(rng, (65, 3), -1, 1)
        c, f = R.obb_membership(pos, centers, rot, half)
        pred = {'only boxes from 300 on hold the points': f.tolist() == [300] * 65 and c.tolist() == [213] * 65}
    else:
        ang = rng.uniform(0, np.pi, 257)
        rot = np.zeros((257, 3, 3))
        rot[:, 0, 0], rot[:, 0, 1], rot[:, 1, 0], rot[:, 1, 1], rot[:, 2, 2] = np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang), 1
        centers, half, pos = rng.uniform(-4, 4, (257, 3)), rng.uniform(0, 3, (257, 3)), rng.uniform(-4, 4, (4097, 3))
        c = R.obb_membership(pos, centers, rot, half)[0]
        pred = {'full mantissa': True, 'a transposed rotation differs': not np.array_equal(c, R.obb_membership(pos, centers, rot, half, 'transposed')[0])}
    return _case(name, pred, pos=pos, centers=centers, rot=rot, half=half)


# ----------------------------------------------------------------------------- b2m_seg_box_vote
VOTE_CASES = tuple('size:%d:%d' % (s, p) for s in (1, 257) for p in (1, 65, 4097)) + ('deciding_point', 'packing', 'no_boxes')


@functools.lru_cache(maxsize=None)
def vote_case(name):
    """segments (P,), useg (sorted voxel-level segment ids), count / first_bb / smallest_bb (P,), ids (instance ids per box)."""
    rng = _rng('vote' + name)
    n_ids = 1024
    ids = rng.permutation(5000)[:n_ids].astype(np.int64)
    if name.startswith('size:'):
        ns, n = (int(x) for x in name.split(':')[1:])
        useg = sorted(set((rng.permutation(4 * ns)[:ns] * 3 + 1).tolist()))
        absent = [s + 1 for s in useg[:3]]                                       # ids no voxel carries
        segments = np.array([(useg + absent)[i] for i in rng.integers(0, len(useg) + (len(absent) if n > 1 else 0), n)], np.int64)
        count = rng.choice([0, 1, 2, 1024], n, p=[0.1, 0.3, 0.4, 0.2]).astype(np.int32)
        pred = {'sizes': (len(useg), len(segments)) == (ns, n)}
        if n > 64:
            pred['points of absent segments'] = bool((R.segment_rank(segments, useg) < 0).any())
            pred['counts 0, 1, 2 and 1024'] = set(count.tolist()) == {0, 1, 2, 1024}
        if ns == 257 and n == 65:
            pred['segments without a point'] = len(set(segments.tolist()) & set(useg)) < ns
    elif name == 'deciding_point':
        useg = [4, 9]
        segments = np.array([9, 4, 9, 4, 9, 4, 4, 9], np.int64)
        count = np.array([2, 3, 1, 2, 1, 2, 5, 0], np.int32)
        pred = {'segment 4: the deciding point is its second (count 2 at index 3, first of two)': True,
                'segment 9: its last point (count 0) decides': True}
    elif name == 'packing':
        useg = [7]
        segments = np.full(4097, 7, np.int64)
        count = np.full(4097, 1024, np.int32)
        count[4096] = 1
        pred = {'count 1 at index 4096 beats count 1024 at index 0': True}
    else:
        useg = [1, 2, 3]
        segments = np.array([1, 2, 3, 5, 1], np.int64)
        count = np.zeros(5, np.int32)
        ids = np.zeros(0, np.int64)
        pred = {'no point in a box: no instance ids': True}
    n = len(segments)
    first = np.where(count > 0, rng.integers(0, n_ids, n), -1).astype(np.int32)
    small = np.where(count > 1, rng.integers(0, n_ids, n), first).astype(np.int32)
    for h in (0, 1):
        a, b = R.segment_vote(segments, useg, count, first, small, ids, h)[1], R.segment_vote(segments, useg, count, first, small, ids, h, 'lowest_index')[1]
        if name in ('deciding_point', 'packing'):
            pred['the lowest index alone decides otherwise (heuristic %d)' % h] = not np.array_equal(a, b)
    if name != 'no_boxes':
        a, b = (R.segment_vote(segments, useg, count, first, small, ids, h)[1] for h in (0, 1))
        if name == 'deciding_point' or (name.startswith('size:257:') and n > 64):
            pred['the heuristic matters'] = not np.array_equal(a, b)
    return _case(name, pred, segments=segments, useg=useg, count=count, first_bb=first, smallest_bb=small, ids=ids)


# ----------------------------------------------------------------------------- b2m_seg_rank, b2m_seg_mode
MODE_CASES = tuple('classes:%d' % c for c in (1, 2, 33)) + ('ties', 'empty')


@functools.lru_cache(maxsize=None)
def mode_case(name):
    """seg_of_point (P,) with -1, cls (P,), n_seg, n_class."""
    rng = _rng('mode' + name)
    if name.startswith('classes:'):
        nc, n_seg, n = int(name[8:]), 65, 4097
        sop = rng.integers(-1, n_seg - 1, n).astype(np.int32)                    # the last segment has no point
        cls = rng.integers(0, nc, n).astype(np.int32)
        pred = {'points of rank -1': bool((sop < 0).any()), 'a segment without points': n_seg - 1 not in sop.tolist()}
        if nc > 1:
            pred['ties'] = not np.array_equal(R.segment_mode(sop, cls, n_seg, nc), R.segment_mode(sop, cls, n_seg, nc, 'highest_class'))
    elif name == 'ties':
        nc, n_seg = 5, 4
        sop = np.array([0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 2, 2, 2, -1, -1, -1, 0], np.int32)
        cls = np.array([3, 1, 3, 1, 4, 2, 0, 4, 2, 0, 2, 2, 1, 0, 0, 0, 2], np.int32)
        m = R.segment_mode(sop, cls, n_seg, nc)
        pred = {'two-way tie: the lower class': m[0] == 1, 'three-way tie: the lowest': m[1] == 0, 'no tie': m[2] == 2,
                'rank -1 is ignored, no point gives 0': m[3] == 0,
                'the highest class differs': R.segment_mode(sop, cls, n_seg, nc, 'highest_class').tolist() == [3, 4, 2, 4]}
    else:
        nc, n_seg = 3, 0
        sop, cls = np.full(5, -1, np.int32), np.array([0, 1, 2, 1, 0], np.int32)
        pred = {'no segment': True}
    pred['classes within range'] = bool(((cls >= 0) & (cls < nc)).all()) and bool((sop < n_seg).all())
    return _case(name, pred, seg_of_point=sop, cls=cls, n_seg=n_seg, n_class=nc)


RANK_CASES = ('n:1', 'n:65', 'n:4097')


@functools.lru_cache(maxsize=None)
def rank_case(name):
    rng = _rng('rank' + name)
    n = int(name[2:])
    useg = sorted(set((rng.permutation(300)[:70] * 5).tolist()))
    segments = rng.integers(0, 1500, n).astype(np.int64) if n > 1 else np.array([useg[3]], np.int64)
    r = R.segment_rank(segments, useg)
    pred = {'n points': len(segments) == n}
    if n > 1:
        pred['present and absent segments'] = bool((r >= 0).any() and (r < 0).any())
    return _case(name, pred, segments=segments, useg=useg)


# ----------------------------------------------------------------------------- whole scenes for the wrappers
SCENE_CASES = ('one_point', 'one_voxel', 'identical', 'one_segment', 'own_segments', 'ties', 'halves', 'mantissa')


@functools.lru_cache(maxsize=None)
def scene_case(name):
    """A raw scene {'positions','colors','normals','segments'} and its voxel size."""
    rng = _rng('scene' + name)
    vs = 0.5
    n = {'one_point': 1, 'one_voxel': 65, 'identical': 257, 'one_segment': 257, 'own_segments': 257, 'ties': 300, 'halves': 217,
         'mantissa': 2000}[name]
    pos = _dyadic(rng, (n, 3), 0, 2, bits=4) - 0.75
    seg = rng.integers(0, 9, n) * 7 + 2
    if name == 'one_voxel':
        pos = _dyadic(rng, (n, 3), 0.3, 0.7, bits=6)
    elif name == 'identical':
        pos = np.tile([[1.25, -0.5, 0.75]], (n, 1))
    elif name == 'one_segment':
        seg = np.full(n, 11)
    elif name == 'own_segments':
        seg = rng.permutation(n) + 40
    elif name == 'halves':
        pos = key_case('halves_negative_shift').pos
    elif name == 'mantissa':
        vs, pos = 0.02, rng.uniform(-0.3, 0.4, (n, 3))
    colors, normals = rng.uniform(0, 1, (n, 3)), rng.normal(size=(n, 3))
    res = R.voxelize_scene(pos, colors, normals, seg, vs)
    V, S = len(res['vox_coords']), len(res['unique_vox_segments'])
    pred = {'n points': len(pos) == n}
    if name in ('one_voxel', 'identical', 'one_point'):
        pred['one voxel'] = V == 1
    if name == 'identical':
        pred['all points identical: point 0 is associated'] = res['point2vox'].tolist() == [0]
    if name == 'one_segment':
        pred['one segment'] = S == 1 and V > 1
    if name == 'own_segments':
        pred['every point its own segment'] = len(set(seg.tolist())) == n and S > 1
    if name == 'ties':
        far = _winner_offsets(res, R.scaled(pos, res['shift'], vs))
        pred.update({'exact ties': bool((res['nearest_ties'] > 1).any()), 'winners in neighbour cells': bool((far > 0).any())})
    if name in ('ties', 'halves', 'mantissa'):
        pred['x-major differs from z-major'] = R.unique_tuples(R.tuples(res['vox_coords']))[0] != R.unique_tuples(R.tuples(res['vox_coords']), 'z_major')[0]
    if name not in ('one_point',):
        pred['negative shift'] = res['shift'] < 0 or name in ('one_voxel', 'identical')
    scene = {'positions': pos, 'colors': colors, 'normals': normals, 'segments': np.asarray(seg, np.int64), 'name': 'a' + name.replace('_', '')}
    return _case(name, pred, scene=scene, vs=vs, rule=res)


LABELLED = ('boxes', 'no_foreground', 's3dis_fg', 's3dis_bg')


@functools.lru_cache(maxsize=None)
def labelled_scene(kind):
    """A hand-built scene of 245 points with seven weak boxes for the three associations: overlapping boxes, quarter-turn rotations,
    five exact duplicates that carry segment ids of their own (those segments get no voxel).  The semantics decide the kind:
    'boxes' mixes foreground and background, 'no_foreground' has no ScanNet foreground box, 's3dis_fg' / 's3dis_bg' only
    foreground / only background boxes under ignore_wall_ceiling_floor."""
    rng = _rng('labelled' + kind)
    n, vs = 240, 0.25
    pos = _dyadic(rng, (n, 3), 0, 2, bits=4)
    cell = np.floor(pos / 0.5).astype(np.int64)
    seg = cell[:, 0] * 16 + cell[:, 1] * 4 + cell[:, 2]
    pos, seg = np.concatenate([pos, pos[10:15]]), np.concatenate([seg, 1000 + np.arange(5)])
    sem = {'boxes': [5, 7, 9, 2, 0, 22, 4], 'no_foreground': [0, 1, 2, 22, 2, 1, 0], 's3dis_fg': [5, 7, 9, 3, 4, 6, 8],
           's3dis_bg': [0, 1, 2, 0, 1, 2, 0]}[kind]
    centers = np.array([[0.5, 0.5, 0.5], [0.75, 0.5, 0.5], [0.5, 0.75, 0.75], [1, 1, 0.125], [1.5, 1.5, 1.5], [1, 1, 1], [1.5, 0.5, 1.0]], np.float32)
    bounds = np.array([[.5, .5, .5], [.5, .5, .5], [.25, .5, .25], [1, 1, .125], [.25, .25, .25], [.5, .5, .5], [.375, .5, .75]], np.float32)
    rot = np.stack([_ROTS[i % len(_ROTS)] for i in range(7)]).reshape(7, 9)
    labels = {'unique_instances': np.arange(7), 'per_instance_semantics': np.array(sem, np.int32), 'per_instance_bb_centers': centers,
              'per_instance_bb_bounds': bounds, 'per_instance_bb_rotations': rot,
              'seg2inst': rng.integers(0, 7, int(seg.max()) + 1).astype(np.int32)}
    scene = {'positions': pos, 'colors': rng.uniform(0, 1, (n + 5, 3)), 'normals': rng.normal(size=(n + 5, 3)), 'segments': seg,
             'name': 'lab' + kind.replace('_', ''), 'labels': labels}
    res = R.voxelize_scene(pos, scene['colors'], scene['normals'], seg, vs)
    sem = np.array(sem)
    fg = (sem > 2) & (sem != 22)
    b = bounds + np.float32(0.005)
    count = R.box_membership(pos, (centers - b)[fg], (centers + b)[fg], np.prod(2 * b, axis=1)[fg])[0]
    pred = {'segments without a voxel': bool((R.segment_rank(seg, res['unique_vox_segments']) < 0).any())}
    if kind == 'boxes':
        pred['points in no, one, two and three foreground boxes'] = {0, 1, 2, 3}.issubset(count.tolist())
    if kind == 'no_foreground':
        pred['no foreground box'] = not fg.any()
    if kind == 's3dis_fg':
        pred['only foreground boxes'] = bool((sem > 2).all())
    if kind == 's3dis_bg':
        pred['only background boxes'] = not (sem > 2).any()
    return _case(kind, pred, scene=scene, vs=vs, rule=res)
