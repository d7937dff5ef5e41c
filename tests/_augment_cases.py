"""The edge cases of the augmentation entries (csrc/augment.hip), shared by tests/test_augment_rule.py (CPU: every case is built, its
predicates hold, every deliberate mistake of _augment_rule.MISTAKES changes a named case) and tests/test_gpu_augment_edges.py (the same
cases through the C entries, bit for bit against the rule).  A case is a name, its inputs and PREDICATES: facts computed with the rule
that say which edge the case reaches; they are asserted when the case is built, so a case that no longer reaches its edge fails on
the CPU.  Inputs carry full mantissas unless a case says otherwise: only then does the order of operations show.

Sizes are the smallest that cross each boundary: 255 / 256 / 257 around a launch block of 256 threads, 1023 / 1024 / 1025 where
b2m_aug_stats goes from one block to two, 262 144 / 262 145 where its 256 blocks stop growing, 600 001 for uneven strides."""
import functools
from types import SimpleNamespace

import numpy as np

import _augment_rule as R

F32, F64 = np.float32, np.float64


def _case(name, predicates, **inputs):
    bad = [k for k, v in predicates.items() if not v]
    assert not bad, (name, bad)
    return SimpleNamespace(name=name, predicates=predicates, **inputs)


def _rng(name):
    return np.random.default_rng(sum(ord(c) * (i + 1) for i, c in enumerate(name)))


def _ro(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


# ----------------------------------------------------------------------------- b2m_aug_stats
STATS_SIZES = (1, 255, 256, 257, 1023, 1024, 1025, 4097, 262144, 262145, 600001)
STATS_CASES = tuple('n:%d' % n for n in STATS_SIZES) + ('big_mean', 'cancel', 'all_equal', 'mixed_signs', 'both_zeros', 'nan_row')
STATS_LARGEST = 'n:600001'


@functools.lru_cache(maxsize=None)
def stats_case(name):
    rng = _rng('stats' + name)
    pred = {}
    if name.startswith('n:'):
        n = int(name[2:])
        x = rng.standard_normal((n, 3)) * np.array([1.0, 30.0, 1e-3]) + np.array([0.3, -7.0, 0.0])
        nb = R.stats_blocks(n)
        pred = {'n rows': len(x) == n, 'blocks': nb == min(256, -(-n // 1024)),
                'the stride loop runs' if n > 256 else 'one row per thread': (R.chain_length(n) > 1) == (n > 256)}
        if n == 262145:
            pred['the first row past 256 blocks of 1024'] = nb == 256 and R.chain_length(n) == 5 and R.chain_length(n - 1) == 4
    elif name == 'big_mean':
        x = 1e6 + rng.standard_normal((4097, 3))
        x[:, 1] = -x[:, 1]
        pred = {'|mean| = 1e6 x spread': bool(np.all(np.abs(x.mean(0)) > 1e5 * x.std(0)))}
    elif name == 'cancel':
        h = rng.standard_normal((2048, 3)) * 1e3
        x = np.concatenate([h, -h, np.zeros((1, 3))])[rng.permutation(4097)]
        pred = {'the sum cancels': bool(np.all(np.abs(R.stats(x)[1]) == 0.0)) and bool(np.abs(x).sum() > 1e6)}
    elif name == 'all_equal':
        x = np.tile(np.array([[0.1, -0.3, 1e-7]]), (1025, 1))
        pred = {'all rows equal': bool((x == x[0]).all())}
    elif name == 'mixed_signs':
        x = rng.standard_normal((1023, 3)) * np.exp(rng.uniform(-20, 20, (1023, 3)))
        pred = {'both signs, 17 decades': x.min() < -1e6 and x.max() > 1e6 and np.abs(x).min() < 1e-6}
    elif name == 'both_zeros':
        x = np.abs(rng.standard_normal((1025, 3)))
        x[:, 1] = -x[:, 1]
        x[[5, 700], 0] = [0.0, -0.0]
        x[[900, 3], 1] = [0.0, -0.0]
        x[:, 2] = np.where(rng.random(1025) < 0.5, 0.0, -0.0)
        pred = {'+0.0 and -0.0 are the extreme of a column': x[:, 0].min() == 0 and x[:, 1].max() == 0 and np.ptp(x[:, 2]) == 0}
    elif name == 'nan_row':
        x = rng.standard_normal((257, 3))
        x[100] = np.nan
        x[256, 1] = np.nan
        want = R.stats(x)[0]
        ok = ~np.isnan(x)
        pred = {'the mean is NaN': bool(np.isnan(want[0:3]).all()),
                'min, max and max|.| ignore the NaN': all(want[3 + c] == x[ok[:, c], c].min() and want[6 + c] == x[ok[:, c], c].max()
                                                          and want[9 + c] == np.abs(x[ok[:, c], c]).max() for c in range(3)),
                'numpy would propagate it': bool(np.isnan(x.min(0)).all())}
    else:
        raise KeyError(name)
    _ro(x)
    return _case(name, pred, x=x)


# ----------------------------------------------------------------------------- b2m_aug_affine
AFFINE_CASES = ('n:1', 'n:255', 'n:256', 'n:257', 'dev_mean', 'dev_min', 'no_centre', 'recentre0', 't_null', 'normals_null',
                'rank2', 'rank1', 'rank0', 'mirror', 'zero_normals', 'nan_normal')
AFFINE_LARGEST = 'n:257'


@functools.lru_cache(maxsize=None)
def affine_case(name):
    """centre: ('host', xyz) | ('mean',) | ('min',) (the device row of b2m_aug_stats) | None."""
    rng = _rng('affine' + name)
    n = int(name[2:]) if name.startswith('n:') else 257
    pos = rng.standard_normal((n, 3)) * np.array([4.0, 3.0, 1.5]) + np.array([1.0, -2.0, 0.7])
    nrm = rng.standard_normal((n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    M = np.eye(3) + rng.standard_normal((3, 3)) * 0.3
    centre, t, recentre = ('host', rng.standard_normal(3)), rng.standard_normal(3), True
    pred = {'full-mantissa operands': bool((R.bits(pos) & np.uint64(0xFFFF)).any() and (R.bits(M) & np.uint64(0xFFFF)).any())}
    if name == 'dev_mean':
        centre = ('mean',)
    elif name == 'dev_min':
        centre = ('min',)
    elif name == 'no_centre':
        centre = None
    elif name == 'recentre0':
        recentre = False
    elif name == 't_null':
        t = None
    elif name == 'normals_null':
        nrm = None
    elif name in ('rank2', 'rank1', 'rank0'):
        u, v, w = np.array([1.0, -2.0, 0.5]), np.array([3.0, 0.25, -1.0]), np.array([0.5, 4.0, 2.0])
        M = {'rank2': np.outer(u, v) + np.outer(w, u), 'rank1': np.outer(u, v), 'rank0': np.zeros((3, 3))}[name]
        K = R.cofactor(M)
        rank = int(name[4])
        pred = {'rank': np.linalg.matrix_rank(M) == rank, 'cofactor zero below rank 2': bool((K == 0).all()) == (rank < 2)}
        pred['(0,0,1) everywhere' if rank < 2 else 'normals along one direction'] = \
            bool((R.affine(pos, nrm, M)[1] == [0.0, 0.0, 1.0]).all()) == (rank < 2)
    elif name == 'mirror':
        M = np.diag([-1.0, 1.0, 1.0]) @ M
        pred = {'a mirror': np.linalg.det(M) < 0}
    elif name == 'zero_normals':
        nrm[::3] = 0.0
        nrm[1, :] = [0.0, -0.0, 0.0]
        pred = {'zero normals give (0,0,1)': bool((R.affine(pos, nrm, M)[1][::3] == [0.0, 0.0, 1.0]).all())}
    elif name == 'nan_normal':
        nrm[7, 1] = np.nan
        nrm[9] = np.nan
        nrm[11] = [np.inf, 0.0, 0.0]
        out = R.affine(pos, nrm, M)[1]
        pred = {'a NaN normal stays NaN': bool(np.isnan(out[7]).all() and np.isnan(out[9]).all()),
                'the others are finite': bool(np.isfinite(np.delete(out, [7, 9, 11], 0)).all())}
    _ro(pos, nrm, M, t)
    return _case(name, pred, pos=pos, normals=nrm, M=M, centre=centre, t=t, recentre=recentre)


def affine_centre(c, device_stats=None):
    """The centre row the kernel uses: `device_stats` (12,) is what b2m_aug_stats gave (the rule's own when None)."""
    if c.centre is None:
        return None
    if c.centre[0] == 'host':
        return c.centre[1]
    st = R.stats(c.pos)[0] if device_stats is None else device_stats
    return st[0:3] if c.centre[0] == 'mean' else st[3:6]


# ----------------------------------------------------------------------------- b2m_aug_axpy
AXPY_CASES = ('n:1', 'n:255', 'n:256', 'n:257', 'a:0', 'a:negative')


@functools.lru_cache(maxsize=None)
def axpy_case(name):
    rng = _rng('axpy' + name)
    n = int(name[2:]) if name.startswith('n:') else 257
    x, y = rng.standard_normal(n) * 5, rng.standard_normal(n)
    a = {'a:0': 0.0, 'a:negative': -0.37}.get(name, 0.005)
    if name == 'a:0':
        x[3], y[3] = -0.0, 1.0                                    # -0.0 + 0 * 1 = +0.0
    _ro(x, y)
    return _case(name, {'n': len(x) == n}, x=x, y=y, a=a)


# ----------------------------------------------------------------------------- b2m_aug_blur
BLUR_SHAPES = ((2, 2, 2), (2, 3, 129), (3, 3, 3), (5, 2, 7), (2, 2, 21), (2, 2, 22))
BLUR_CASES = tuple('noise:%dx%dx%d' % s for s in BLUR_SHAPES) + ('impulse:corner', 'impulse:edge', 'impulse:face', 'impulse:interior',
                                                                 'halfway', 'absorb')
BLUR_LARGEST = 'noise:2x3x129'
# refused on the arguments alone.  (An axis of one node is refused, so no grid has 85 = 5 * 17 or 86 = 2 * 43 cells: the grids
# nearest to one block of 256 elements are 2 x 2 x 21 = 252 elements and 2 x 2 x 22 = 264.)
BLUR_REFUSED = ((17, 5, 1), (2, 43, 1), (1, 4, 4), (4, 1, 4), (1024, 1024, 1024))
IMPULSE_SHAPE = (5, 4, 6)
IMPULSE_AT = {'corner': (0, 0, 0), 'edge': (4, 3, 2), 'face': (2, 0, 3), 'interior': (2, 2, 3)}


@functools.lru_cache(maxsize=None)
def blur_case(name):
    rng = _rng('blur' + name)
    kind, _, what = name.partition(':')
    if kind == 'noise':
        shape = tuple(int(v) for v in what.split('x'))
        g = rng.standard_normal(shape + (3,)).astype(F32)
        elems = g.size
        pred = {'shape': g.shape[:3] == shape, 'every axis has 2 nodes or more': min(shape) >= 2}
        if shape == (2, 2, 21):
            pred['one launch block, not full'] = elems == 252
        if shape == (2, 2, 22):
            pred['a second launch block'] = 256 < elems == 264
    elif kind == 'absorb':
        # prev = 2^60, self = 1, next = -2^60 on every axis in turn: (w*prev + w*self) + w*next loses `self`, any order that adds
        # prev and next first keeps it
        g = np.ones((3, 3, 3, 3), F32)
        g[0, 1, 1], g[2, 1, 1] = 2.0 ** 60, -2.0 ** 60
        g[1, 0, 1], g[1, 2, 1] = 2.0 ** 60, -2.0 ** 60
        out = R.blur_pass(g, 0)
        pred = {'the middle tap is absorbed': bool((out[1, 1, 1] == 0).all())}
    elif kind == 'impulse':
        g = np.zeros(IMPULSE_SHAPE + (3,), F32)
        at = IMPULSE_AT[what]
        g[at] = [1.0, 3.0, -7.0]
        on_border = sum(int(i == 0 or i == d - 1) for i, d in zip(at, IMPULSE_SHAPE))
        pred = {'position': on_border == {'corner': 3, 'edge': 2, 'face': 1, 'interior': 0}[what]}
        if what != 'interior':                                    # mass leaves through the zero padding; reflection would keep it
            pred['the padding shows'] = not np.array_equal(R.blur(g), R.blur(g, 'blur_reflect'))
    else:
        # pass 1 (x): prev = b, self = a, next = c chosen so that the fp64 sum is exactly half-way between two floats
        # With self = 2^k the product w * self is itself a float (w has 24 bits), so the tie is T = w * self + half an ulp of it;
        # prev = b brings the half ulp up to its own rounding error, next = c cancels that error.
        w = F64(F32(1) / F32(3))
        scale = (2.0 ** rng.integers(-8, 9, (2, 64, 3))) * np.where(rng.random((2, 64, 3)) < 0.5, -1.0, 1.0)
        b0 = F32(2.0 ** -26 / w)
        b1 = (np.full(64, b0, F32).view(np.uint32) + np.arange(64, dtype=np.uint32)).view(F32)      # b0 and the 63 floats above it
        b = np.broadcast_to(b1[None, :, None], (2, 64, 3)).astype(F64)
        T = w + 2.0 ** -26
        c = ((2.0 ** -26 - w * b) / w).astype(F32).astype(F64)
        g = np.stack([b * scale, scale, c * scale], 0).astype(F32)
        acc = ((0.0 + w * g[0].astype(F64)) + w * g[1].astype(F64)) + w * g[2].astype(F64)
        lo32 = (w * g[1].astype(F64)).astype(F32)
        pred = {'w * 2^k is a float': bool(np.array_equal(lo32.astype(F64), w * g[1].astype(F64))),
                'every sum of the first pass is an exact tie': bool(np.array_equal(acc, T * scale)) and
                bool(np.array_equal(np.abs(T * scale) - np.abs(lo32), np.spacing(np.abs(lo32)).astype(F64) / 2)),
                'shape': g.shape == (3, 2, 64, 3)}
    _ro(g)
    return _case(name, pred, grid=g)


# ----------------------------------------------------------------------------- b2m_aug_displace
def _axis_search(kind, count=3):
    """Seeded search over np.linspace axes for `count` axes of different length on which a node-adjacent point takes the branch:
    [(lo, step, hi, n, xs)].  For 'last' the axis must have hi != lo + (n-1)*step, so that "the last node is exactly hi" shows."""
    rng = np.random.default_rng({'down': 101, 'up': 202, 'last': 303}[kind])
    out, seen = [], set()
    for _ in range(20000):
        n = int(rng.integers(3, 14))
        lo = rng.uniform(-5, 5)
        hi = lo + rng.uniform(0.5, 8)
        step = np.linspace(lo, hi, n, retstep=True)[1]
        node = lo + np.arange(n) * step
        xs = np.concatenate([node, np.nextafter(node, -np.inf), np.nextafter(node, np.inf), [hi, np.nextafter(hi, -np.inf)]])
        xs = xs[(xs >= lo) & (xs <= hi)]
        br = R.axis_cell(xs, lo, step, hi, n)[2]
        uneven = hi != lo + (n - 1) * step
        hit = {'down': bool((br & R.DOWN).any()), 'up': bool((br & R.UP).any()), 'last': bool(uneven and (br & R.LAST).any())}[kind]
        if hit and n not in seen:
            seen.add(n)
            out.append((lo, step, hi, n, xs))
            if len(out) == count:
                return out
    return out


def _node_points(lo, step, hi, n, rng, outside=True):
    """Points whose coordinate on one axis runs through every node, one ulp to either side, lo, hi and one ulp outside each, the
    other two coordinates random inside."""
    blocks = []
    for a in range(3):
        node = lo[a] + np.arange(n[a]) * step[a]
        node[-1] = hi[a]
        xs = np.concatenate([node, np.nextafter(node, -np.inf), np.nextafter(node, np.inf), lo[a] + np.arange(n[a]) * step[a]])
        if not outside:
            xs = xs[(xs >= lo[a]) & (xs <= hi[a])]
        p = lo + rng.random((len(xs), 3)) * (hi - lo)
        p[:, a] = xs
        blocks.append(p)
    return np.concatenate(blocks)


DISPLACE_CASES = ('nodes', 'nonfinite', 'two_nodes', 'branch:down', 'branch:up', 'branch:last', 'mag:0', 'mag:-0.4', 'mag:1e3',
                  'n:1', 'n:255', 'n:256', 'n:257')
DISPLACE_LARGEST = 'n:257'


@functools.lru_cache(maxsize=None)
def displace_case(name):
    rng = _rng('displace' + name)
    kind, _, what = name.partition(':')
    mag = 1.0
    n = np.array([4, 3, 5])
    lo, hi = np.array([-1.3, 0.2, -7.7]), np.array([2.9, 0.9, 1.1])
    pred = {}
    if kind == 'branch':
        found = _axis_search(what)
        pred['the search found three axes of different length'] = len(found) == 3
        lo, step, hi, n = (np.array([f[k] for f in found]) for k in range(4))
        blocks = []
        for a, f in enumerate(found):
            p = lo + rng.random((len(f[4]), 3)) * (hi - lo)
            p[:, a] = f[4]
            blocks.append(p)
        pos = np.concatenate(blocks)
    else:
        if kind == 'two_nodes':
            n = np.array([2, 2, 2])
        step = np.array([np.linspace(a, b, d, retstep=True)[1] for a, b, d in zip(lo, hi, n)])
        if kind == 'n':
            m = int(what)
            pos = lo - 0.1 * (hi - lo) + rng.random((m, 3)) * 1.2 * (hi - lo)
            pred['n points'] = len(pos) == m
        elif kind == 'nonfinite':
            pos = lo + rng.random((12, 3)) * (hi - lo)
            pos[0, 0] = pos[1, 1] = pos[2, 2] = np.nan
            pos[3, 0], pos[4, 1], pos[5, 2], pos[6, 0] = np.inf, -np.inf, np.inf, -np.inf
            pos[7] = np.nan
        else:
            pos = _node_points(lo, step, hi, n, rng)
            if kind == 'mag':
                mag = float(what)
    grid = rng.standard_normal(tuple(int(v) for v in n) + (3,)).astype(F32)
    out, br = R.displace(pos, grid, lo, step, hi, n, mag)
    inside = ((pos >= lo) & (pos <= hi)).all(1)
    moved = (R.bits(out) != R.bits(pos)).any(1)
    pred['outside points keep their bits'] = not moved[~inside].any()
    if kind in ('nodes', 'two_nodes'):
        on_lo, on_hi = (pos == lo).any(1) & inside, (pos == hi).any(1) & inside
        pred['points exactly on lo and on hi are inside and move'] = bool(on_lo.any() and on_hi.any() and moved[on_lo | on_hi].all())
        just_out = ((pos == np.nextafter(lo, -np.inf)) | (pos == np.nextafter(hi, np.inf))).any(1)
        pred['one ulp outside on every axis'] = all(((pos[:, a] == np.nextafter(lo[a], -np.inf)).any() and
                                                     (pos[:, a] == np.nextafter(hi[a], np.inf)).any()) for a in range(3))
        pred['... and they are outside'] = not inside[just_out].any()
        pred['three different axis lengths'] = kind == 'two_nodes' or len(set(n.tolist())) == 3
    if kind == 'nonfinite':
        pred['no point is inside but the finite ones'] = bool((inside == np.isfinite(pos).all(1)).all() and inside.sum() == 4)
    if kind == 'branch':
        bit = {'down': R.DOWN, 'up': R.UP, 'last': R.LAST}[what]
        pred['every axis takes the branch'] = all(bool((br[:, a] & bit).any()) for a in range(3))
        pred['three different axis lengths'] = len(set(n.tolist())) == 3
        if what == 'last':
            pred['hi != lo + (n-1)*step on every axis'] = bool(np.all(hi != lo + (n - 1) * step))
    if kind == 'mag' and what == '0':
        pred['x + d * 0 = x'] = bool(np.array_equal(out, pos))
    _ro(pos, grid, lo, step, hi, n)
    return _case(name, pred, pos=pos, grid=grid, lo=lo, step=step, hi=hi, n=n, magnitude=mag, branch=br)


# refused on the arguments alone: (n points, dims, lo, step, hi)
DISPLACE_REFUSED = {
    'descending axis': (5, (3, 3, 3), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2.0, -2.0, 2.0)),
    'step == 0': (5, (3, 3, 3), (0.0, 0.0, 0.0), (1.0, 0.0, 1.0), (2.0, 2.0, 2.0)),
    'step < 0': (5, (3, 3, 3), (0.0, 0.0, 0.0), (1.0, 1.0, -1.0), (2.0, 2.0, 2.0)),
    'one node': (5, (3, 1, 3), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2.0, 2.0, 2.0)),
    'n == 0': (0, (3, 3, 3), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2.0, 2.0, 2.0)),
}


# ----------------------------------------------------------------------------- b2m_aug_vertex_normals
NORMALS_CASES = ('n:1', 'n:255', 'n:256', 'n:257', 'isolated', 'fan300', 'degenerate', 'cancel', 'twice', 'bad_values', 'nan_position')
NORMALS_LARGEST = 'fan300'


@functools.lru_cache(maxsize=None)
def normals_case(name):
    """pos (V,3), faces (F,3) or None, row_ptr (V+1), face_of (3F) or None -- the CSR is always a true one of a clean face list."""
    rng = _rng('normals' + name)
    pred = {}
    if name.startswith('n:'):
        V = int(name[2:])
        pos = rng.standard_normal((V, 3))
        faces = None if V == 1 else np.stack([rng.permutation(V)[:3] for _ in range(2 * V)]).astype(np.int64)
        pred['no faces: NULL arrays'] = (faces is None) == (V == 1)
    elif name == 'isolated':
        pos = rng.standard_normal((40, 3))
        faces = np.stack([rng.permutation(39)[:3] for _ in range(60)]).astype(np.int64)
        pred['vertex 39 is in no face'] = not (faces == 39).any()
    elif name == 'fan300':
        ang = np.sort(rng.uniform(0, 2 * np.pi, 300))
        rim = np.stack([np.cos(ang), np.sin(ang), rng.standard_normal(300) * 0.3], 1) * rng.uniform(0.5, 2, (300, 1))
        pos = np.concatenate([rng.standard_normal((1, 3)) * 0.1, rim])
        k = np.arange(300)
        faces = np.stack([np.zeros(300, np.int64), 1 + k, 1 + (k + 1) % 300], 1)[rng.permutation(300)]
        pred['valence 300'] = int((faces == 0).sum()) == 300
    elif name == 'degenerate':
        pos = np.array([[0.0, 0, 0], [1, 1, 1], [2, 2, 2], [0.3, -0.2, 0.9], [1.5, 0.1, 0.2], [-4, -4, -4]])
        faces = np.array([[0, 1, 2], [3, 3, 4], [1, 5, 2], [3, 4, 4]], np.int64)          # collinear; a repeated vertex; collinear; ...
        pred['every face has zero area: (0,0,1) everywhere'] = bool((R.vertex_normals(pos, faces) == [0.0, 0.0, 1.0]).all())
    elif name == 'cancel':
        pos = rng.standard_normal((5, 3))
        faces = np.array([[0, 1, 2], [0, 2, 1], [2, 3, 4]], np.int64)                    # the same triangle with both windings
        out = R.vertex_normals(pos, faces)
        pred['the two windings cancel exactly'] = bool((out[:2] == [0.0, 0.0, 1.0]).all() and abs(np.linalg.norm(out[2]) - 1) < 1e-12)
    elif name == 'twice':
        pos = rng.standard_normal((6, 3))
        faces = np.array([[0, 1, 2], [3, 1, 3], [3, 4, 5], [2, 2, 2]], np.int64)
        rp = R.vertex_csr(faces, 6)[0]
        pred['vertex 3 has two entries for face 1'] = int(rp[4] - rp[3]) == 3
    elif name == 'bad_values':
        pos = rng.standard_normal((30, 3))
        faces = np.stack([rng.permutation(30)[:3] for _ in range(50)]).astype(np.int64)
    elif name == 'nan_position':
        pos = rng.standard_normal((30, 3))
        pos[4, 1] = np.nan
        faces = np.stack([rng.permutation(30)[:3] for _ in range(50)]).astype(np.int64)
        touched = np.unique(faces[(faces == 4).any(1)])
        out = R.vertex_normals(pos, faces)
        pred['a NaN sum gives (0,0,1), not NaN'] = bool((out[touched] == [0.0, 0.0, 1.0]).all() and len(touched) > 3
                                                        and not np.isnan(out).any())
    else:
        raise KeyError(name)
    row_ptr, face_of = R.vertex_csr(faces, len(pos)) if faces is not None else (np.zeros(len(pos) + 1, np.int64), None)
    if name == 'bad_values':                                      # the arrays stay fully allocated; only VALUES leave the range
        clean = R.vertex_normals(pos, faces)
        faces = faces.copy()
        face_of = face_of.copy()
        faces[7, 1], faces[8, 0], face_of[5], face_of[100] = 30, -1, 50, -3
        out = R.vertex_normals(pos, faces, row_ptr, face_of)
        pred['the skipped entries change some normals'] = 0 < int((out != clean).any(1).sum()) < 30
    want = R.vertex_normals(pos, faces, row_ptr, face_of)
    pred['unit length'] = bool(np.all(np.abs(np.linalg.norm(want, axis=1) - 1) < 1e-12))
    _ro(pos, faces, row_ptr, face_of)
    return _case(name, pred, pos=pos, faces=faces, row_ptr=row_ptr, face_of=face_of)


# ----------------------------------------------------------------------------- b2m_aug_colour
COLOUR_CASES = tuple('flags:%d' % f for f in range(8)) + ('blend:0', 'blend:1', 'const_channel', 'edges01:2', 'edges01:4', 'nan_in',
                                                          'n:85', 'n:86')
COLOUR_LARGEST = 'flags:7'


@functools.lru_cache(maxsize=None)
def colour_case(name):
    rng = _rng('colour' + name)
    kind, _, what = name.partition(':')
    n = {'n': int(what) if kind == 'n' else 0, 'const_channel': 86, 'nan_in': 85}.get(kind, 1000)
    col = rng.random((n, 3))
    flags, blend = 7, 0.37
    tr = (rng.random(3) - 0.5) * 0.2
    jit = rng.uniform(-0.1, 0.1, (n, 3))
    pred = {}
    if kind == 'flags':
        flags = int(what)
    elif kind == 'blend':
        blend = float(what)
    elif kind == 'const_channel':
        col[:, 1] = 0.25
        col[0, 2] = col[:, 2].min()                               # v == lo on a channel that is not constant: 0 * finite
        pred['0 * inf gives NaN where v == lo'] = bool(np.isnan(R.colour(col, R.stats(col)[0], 1, blend, tr, jit)[:, 1]).all())
    elif kind == 'edges01':
        flags = int(what)
        e = np.array([0.75, 0.75 + 2.0 ** -52, np.nextafter(0.75, 0), -0.25, np.nextafter(-0.25, 0), np.nextafter(-0.25, -1)])
        col = np.tile(e[:, None], (167, 3))[:1000]
        tr = np.array([0.25, 0.25, 0.25])
        jit = np.full((1000, 3), 0.25)
        raw = (0.25 + e).tolist()                                 # (these sums are exact)
        out = R.colour(col, None, flags, blend, tr, jit)[:6, 0]
        pred['the sums: exactly 1, one ulp above, one ulp below, exactly 0, just above, just below'] = \
            raw == [1.0, np.nextafter(1.0, 2), np.nextafter(1.0, 0), 0.0, 2.0 ** -55, -2.0 ** -54]
        pred['... clipped only where they left [0, 1]'] = out.tolist() == [1.0, 1.0, np.nextafter(1.0, 0), 0.0, 2.0 ** -55, 0.0]
    elif kind == 'nan_in':
        col[3, 0] = col[4, 1] = np.nan
        flags = 6
        pred['NaN in, NaN out'] = bool(np.isnan(R.colour(col, None, flags, blend, tr, jit)[[3, 4], [0, 1]]).all())
    if kind in ('flags', 'blend', 'n'):
        out = R.colour(col, R.stats(col)[0], flags, blend, tr, jit)
        pred['some values are clipped'] = not (flags & 6) or bool(((out == 0) | (out == 1)).any())
    _ro(col, tr, jit)
    return _case(name, pred, col=col, flags=flags, blend=blend, tr=tr, jitter=jit)


# ----------------------------------------------------------------------------- b2m_inst_boxes
BOX_CASES = ('I:1', 'I:255', 'I:256', 'I:257', 'I==n', 'big', 'shuffled_sem', 'signed_zero', 'out_of_range', 'missing3', 'one_point', 'far')
BOX_LARGEST = 'big'
BOX_DENSE = tuple(c for c in BOX_CASES if c not in ('out_of_range', 'missing3'))          # what instance_labels accepts


@functools.lru_cache(maxsize=None)
def box_case(name):
    rng = _rng('boxes' + name)
    pred = {}
    if name.startswith('I:'):
        I = int(name[2:])
        inst = np.concatenate([np.arange(I), rng.integers(0, I, 2 * I + 5)])
    elif name == 'I==n':
        I = 300
        inst = np.arange(I)
        pred['one point per instance'] = True
    elif name == 'big':
        I = 257
        inst = np.concatenate([np.arange(I), np.where(rng.random(300001 - I) < 0.9, 200, rng.integers(0, I, 300001 - I))])
        pred['300 001 points, 90 % in one instance'] = len(inst) == 300001 and (inst == 200).mean() > 0.89
    elif name == 'one_point':
        I = 9
        inst = np.concatenate([np.arange(I), rng.integers(0, 8, 200)])
        pred['instance 8 has one point'] = int((inst == 8).sum()) == 1
    elif name == 'missing3':
        I = 40
        inst = rng.choice(np.setdiff1d(np.arange(I), [0, 17, 39]), 500)
    else:
        I = 12
        inst = np.concatenate([np.arange(I), rng.integers(0, I, 600)])
    inst = inst[rng.permutation(len(inst))].astype(np.int64)
    P = len(inst)
    pos = rng.standard_normal((P, 3)) * np.array([3.0, 2.0, 1.0]) + rng.standard_normal((I, 3))[inst] * 4
    sem = (inst * 7 + 3) % 19
    if name == 'shuffled_sem':
        sem = rng.integers(0, 19, P)
        first = [np.nonzero(inst == i)[0] for i in range(I)]
        pred['semantics vary inside an instance; the lowest and the highest point disagree'] = \
            any(sem[f[0]] != sem[f[-1]] for f in first)
        pred['points do not arrive in instance order'] = bool((np.diff(inst) < 0).any())
    if name == 'far':                                             # boxes of a few units 1e10 from the origin: lo + hi rounds visibly
        pos = pos + np.array([1e10, -1e10, 3e9])
        pred['hi - centre is not (hi - lo) / 2 in float32'] = not np.array_equal(
            R.inst_boxes(pos, inst, inst, I)['per_bounds'], R.inst_boxes(pos, inst, inst, I, 'boxes_bound_half_extent')['per_bounds'])
    if name == 'signed_zero':
        pos[:, 1] = np.where(rng.random(P) < 0.5, 0.0, -0.0)
        pos[:, 2] = np.abs(pos[:, 2])
        pos[np.nonzero(inst == 3)[0][:2], 2] = [0.0, -0.0]
        pred['a column holds both +0.0 and -0.0'] = bool(np.signbit(pos[:, 1]).any() and not np.signbit(pos[:, 1]).all())
    if name == 'out_of_range':
        inst[[5, 77, 300]] = [-1, I, -(2 ** 40)]
        inst[[6, 78]] = [I + 5, 2 ** 40]
        pred['ids -1 and n_inst among valid ones'] = bool((inst == -1).any() and (inst == I).any())
    sem = sem.astype(np.int64)
    want = R.inst_boxes(pos, inst, sem, I)
    pred['coordinates of both signs'] = pos.min() < 0 < pos.max()
    pred['missing'] = want['missing'] == (3 if name == 'missing3' else 0)
    if name == 'missing3':
        pred['zero rows'] = all(bool((want[k][[0, 17, 39]] == 0).all()) for k in ('centers64', 'per_centers', 'per_bounds', 'per_radius',
                                                                                  'per_sem'))
    _ro(pos, inst, sem)
    return _case(name, pred, pos=pos, inst=inst, sem=sem, n_inst=I)
