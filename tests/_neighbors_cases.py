"""The seeded point sets of the nearest-neighbour tests and the yardstick they are held to: numpy brute force in the contract's
summation order, ``d2 = (dx*dx + dy*dy) + dz*dz`` in fp64 (numpy does not contract), first minimum = lowest row.

A case is ``(ref (n,3), q (m,3), ties)``; ``ties`` marks the cases built to have exactly equal distances, which only the
lowest-row rule decides (tests/test_neighbors.py shows that no other case has two candidates within a relative 1e-9)."""
import numpy as np

SEED = 7000
GAP = 1e-9


def case_a(rng):
    return rng.uniform(-1, 1, (1, 3)), rng.uniform(-2, 2, (33, 3)), False


def case_b(rng):
    return rng.uniform(0, 1, (65, 3)), rng.uniform(-0.1, 1.1, (257, 3)), False


def case_c(rng):
    """The room: 8 x 6 x 3 m, half of the points exactly on z = 0, an outlier clump 40 m away, 40 queries far outside."""
    ref = rng.uniform(0, 1, (4099, 3)) * np.array([8.0, 6.0, 3.0])
    ref[::2, 2] = 0.0
    ref[-7:] += 40.0
    q = rng.uniform(0, 1, (3001, 3)) * np.array([8.0, 6.0, 3.0])
    q[:40] = rng.uniform(-50.0, 58.0, (40, 3))
    return ref, q, False


def case_d(rng):
    """300 points inside a cube of 1e-6, the first of them repeated 20 times; queries inside the cube, next to it and far away."""
    ref = 0.5 + rng.uniform(0, 1e-6, (300, 3))
    ref = np.concatenate([ref, np.repeat(ref[:1], 20, 0)])
    q = np.concatenate([0.5 + rng.uniform(0, 1e-6, (60, 3)), ref[:1], ref[7:8], 0.5 + rng.uniform(-1e-5, 1e-5, (30, 3)),
                        rng.uniform(-30, 30, (20, 3))])
    return ref, q, True


def case_e(rng):
    """6 x 6 x 6 integer lattice in shuffled row order; the queries are the cell centres: eight rows at exactly the same distance."""
    g = np.stack(np.meshgrid(np.arange(6.0), np.arange(6.0), np.arange(6.0), indexing='ij'), -1).reshape(-1, 3)
    ref = g[rng.permutation(len(g))]
    c = np.stack(np.meshgrid(np.arange(5.0), np.arange(5.0), np.arange(5.0), indexing='ij'), -1).reshape(-1, 3) + 0.5
    return ref, c, True


def case_f_line(rng):
    ref = np.stack([rng.uniform(-3, 5, 500), np.full(500, 1.5), np.full(500, -2.0)], 1)
    q = rng.uniform(-4, 6, (300, 3))
    return ref, q, False


def case_f_plane(rng):
    ref = np.stack([rng.uniform(-3, 5, 700), rng.uniform(0, 2, 700), np.full(700, 0.25)], 1)
    q = rng.uniform(-4, 6, (300, 3))
    return ref, q, False


def case_h(rng):
    """One infinite ref row and one NaN query row among finite ones."""
    ref = rng.uniform(0, 4, (200, 3))
    ref[17, 1] = np.inf
    q = rng.uniform(-1, 5, (150, 3))
    q[41, 2] = np.nan
    return ref, q, False


def case_i(rng):
    """Past 65 536 rows on both sides: every scan and sort spans many blocks."""
    box = np.array([10.0, 8.0, 3.0])
    return rng.uniform(0, 1, (70001, 3)) * box, rng.uniform(-0.02, 1.02, (70001, 3)) * box, False


SMALL = {'a': case_a, 'b': case_b, 'c': case_c, 'd': case_d, 'e': case_e, 'f_line': case_f_line, 'f_plane': case_f_plane, 'h': case_h}
ORDER = list(SMALL) + ['i']
_cache = {}


def case(name):
    """(ref, q, ties) of a case; every case has its own stream, SEED + its position, and is made once."""
    if name not in _cache:
        fn = case_i if name == 'i' else SMALL[name]
        ref, q, ties = fn(np.random.default_rng(SEED + ORDER.index(name)))
        ref.setflags(write=False); q.setflags(write=False)
        _cache[name] = (ref, q, ties)
    return _cache[name]


# ----------------------------------------------------------------------------- the edge cases
# Built to stress what carries the correctness argument of csrc/neighbors.hip: the shell-termination bound, the clamped cell of a
# query outside the box, the device-chosen cell edge (its clip, its growth loop, its guards), exact ties across cells, squared
# distances that overflow, and sizes around a launch block.  tests/test_neighbors.py checks every one of them on the CPU (no second
# candidate within a relative 1e-9, or: the case does tie) and says with `grid_of` -- a numpy restatement of nn_grid_kernel --
# which shell each winner of the shell cases lies in.

def grid_of(ref, scale=1.0):
    """nn_box_kernel + nn_grid_kernel restated: (lo, hi, edge, dim) of the index over `ref`, or None when no row is finite.  The
    device's log / exp may differ from numpy's in the last place, so whoever reads a cell off this grid must not depend on the last
    place of the edge: `scale` multiplies the edge for that check."""
    n = len(ref)
    ok = np.isfinite(ref).all(1)
    if not ok.any():
        return None
    with np.errstate(all='ignore'):
        lo, hi = ref[ok].min(0), ref[ok].max(0)
        ext = hi - lo
        ext = np.where(ext < 1.7e308, ext, 1.7e308)
        big = ext.max()
        k = int((ext > 0).sum())
        logv = 0.0
        for e in ext:
            if e > 0:
                logv += np.log(e)
        cap = 4.0 * n + 8.0
        edge, dim = 1.0, np.ones(3, np.int64)
        if k > 0:
            def cells_of(edge):
                u = np.floor(ext / edge)
                d = np.where(u >= 1048576.0, 1048576.0, u + 1.0)
                return d.astype(np.int64), float(d[0] * d[1] * d[2])
            edge = np.exp((logv - np.log(2.0 * n)) / k)
            least = big / (1048576.0 * 0.5)
            if not edge >= least:
                edge = least
            if not edge > 0.0:
                edge = big
            if not edge < 1.7e308:
                edge = 1.7e308
            dim, cells = cells_of(edge)
            for _ in range(64):
                if not cells > cap:
                    break
                edge *= 1.2599210498948732
                if not edge < 1.7e308:
                    edge = 1.7e308
                dim, cells = cells_of(edge)
            if cells > cap:
                edge, dim = 1.7e308, np.ones(3, np.int64)
    return lo, hi, float(edge) * scale, dim


def cell_of(p, grid):
    """nn_cell on every axis: the cell of the points p (m,3), clamped into the grid."""
    lo, _, edge, dim = grid
    with np.errstate(all='ignore'):
        u = np.floor((p - lo) / edge)
    return np.where(u >= dim - 1, dim - 1, np.where(u > 0, u, 0)).astype(np.int64)


def shell_of(q, rows, grid):
    """Chebyshev distance in cells between the (clamped) cell of each query and the cell of its row: the shell the walk finds it in."""
    return np.abs(cell_of(q, grid) - cell_of(rows, grid)).max(1)


SHELL_DIRS = {'axis': (1, 0, 0), 'face': (1, 1, 0), 'space': (1, 1, 1)}
SHELL_R = tuple(range(7))
_SHELL_CELL = np.array([10, 10, 12])
_SHELL_DELTA = 0.1


def shell_case(kind, r):
    """The unit box, pinned by its 8 corners; a dense jittered lattice in the slab z < 0.1 (4096 rows: it sets the edge, ~0.05, and
    lies 11 cells from the query); in the empty rest one query, one WINNER r cells from the query's cell along `kind`, and one DECOY
    in a nearer shell at the far corner of its cell, farther from the query than the winner.  Rows are shuffled.
    -> (ref, q (1,3), winner row, decoy row, decoy shell)."""
    rng = np.random.default_rng(SEED + 500 + 10 * list(SHELL_DIRS).index(kind) + r)
    i, j, k = np.meshgrid(np.arange(32), np.arange(32), np.arange(4), indexing='ij')
    lat = np.stack([i, j, k], -1).reshape(-1, 3) + rng.uniform(0.1, 0.9, (4096, 3))
    lat = lat / np.array([32.0, 32.0, 40.0])
    corners = np.stack(np.meshgrid([0.0, 1.0], [0.0, 1.0], [0.0, 1.0], indexing='ij'), -1).reshape(-1, 3)
    n = 4096 + 8 + 2
    edge = grid_of(np.concatenate([corners, np.zeros((n - 8, 3))]))[2]              # a function of n and the extents alone
    d = _SHELL_DELTA
    dirv = np.array(SHELL_DIRS[kind], np.float64)
    q = (_SHELL_CELL + (1 - d)) * edge
    winner = q - 2 * d * edge * dirv if r == 0 else np.where(dirv > 0, (_SHELL_CELL + r + d) * edge, q)
    dist = np.sqrt(((winner - q) ** 2).sum()) / edge
    s = 0
    while np.sqrt(3.0) * (s + 1 - 2 * d) <= 1.05 * dist:
        s += 1
    decoy = (_SHELL_CELL - s + d) * edge
    ref = np.concatenate([corners, lat, winner[None], decoy[None]])
    perm = rng.permutation(n)
    ref = ref[perm]
    inv = np.argsort(perm)
    return ref, q[None].copy(), int(inv[n - 2]), int(inv[n - 1]), s


EQUI_R = (0, 1, 2, 3)


def _equidistant(rng):
    """The box and the slab of the shell cases; four queries, each exactly half-way between two rows on a line along x, of which one
    lies r cells from the query's cell and the other r + 1 (r = 0 ... 3).  Coordinates are multiples of 2^-20, so q +- t is exact.
    The rows of query j are the two whose y equals the query's."""
    i, j, k = np.meshgrid(np.arange(32), np.arange(32), np.arange(4), indexing='ij')
    lat = (np.stack([i, j, k], -1).reshape(-1, 3) + rng.uniform(0.1, 0.9, (4096, 3))) / np.array([32.0, 32.0, 40.0])
    corners = np.stack(np.meshgrid([0.0, 1.0], [0.0, 1.0], [0.0, 1.0], indexing='ij'), -1).reshape(-1, 3)
    n = 4096 + 8 + 2 * len(EQUI_R)
    edge = grid_of(np.concatenate([corners, np.zeros((n - 8, 3))]))[2]
    dyadic = lambda v: np.round(np.asarray(v) * 2.0 ** 20) / 2.0 ** 20
    q, rows = [], []
    for r, (cy, cz) in zip(EQUI_R, ((4, 6), (14, 6), (4, 15), (14, 15))):
        p = dyadic([(10 + 0.25) * edge, (cy + 0.5) * edge, (cz + 0.5) * edge])
        t = float(dyadic((r + 0.5) * edge))
        q.append(p)
        rows += [p + [t, 0, 0], p - [t, 0, 0]]
    ref = np.concatenate([corners, lat, np.array(rows)])
    return ref[rng.permutation(n)], np.array(q), True


def _outside(rng):
    """300 rows in the unit box; queries beyond a face, an edge and a corner of it, 1e-9, 1 and 1e3 box sizes away."""
    ref = rng.uniform(0, 1, (300, 3))
    lo, hi = ref.min(0), ref.max(0)
    size = (hi - lo).max()
    qs = []
    for dist in (1e-9, 1.0, 1e3):
        for n_out in (1, 2, 3):                                     # face, edge, corner
            for _ in range(12):
                p = rng.uniform(lo, hi)
                axes = rng.permutation(3)[:n_out]
                side = rng.integers(0, 2, n_out)
                p[axes] = np.where(side == 1, hi[axes] + dist * size, lo[axes] - dist * size)
                qs.append(p)
    return ref, np.array(qs), False


def _one_row(rng):
    return rng.uniform(-1, 1, (1, 3)), np.concatenate([rng.uniform(-2, 2, (40, 3)), np.zeros((1, 3))]), False


def _two_identical(rng):
    return np.repeat(rng.uniform(-1, 1, (1, 3)), 2, 0), rng.uniform(-2, 2, (40, 3)), True


def _all_identical(rng):
    return np.repeat(rng.uniform(-1, 1, (1, 3)), 300, 0), rng.uniform(-2, 2, (257, 3)), True


def _denormal(rng):
    """Extent 1e-320: every difference of two rows underflows in the square, so all rows tie for every query."""
    ref = rng.integers(0, 2000, (300, 3)).astype(np.float64) * 5e-324
    ref[:2] = [[0.0, 0.0, 0.0], [2000 * 5e-324] * 3]
    return ref, np.concatenate([ref[:50], rng.uniform(-1, 1, (50, 3)), rng.uniform(0, 1e-320, (50, 3))]), True


def _denormal_min(rng):
    """Extent three denormal steps: the edge the formula gives underflows to zero, and the guard takes the extent instead."""
    ref = rng.integers(0, 4, (300, 3)).astype(np.float64) * 5e-324
    ref[:2] = [[0.0, 0.0, 0.0], [3 * 5e-324] * 3]
    return ref, np.concatenate([ref[:50], rng.uniform(-1, 1, (50, 3))]), True


def _extent_1e300(rng):
    """Extent 1e300: d2 overflows to +inf for every pair but a query that is a row."""
    ref = rng.uniform(0, 1e300, (300, 3))
    return ref, np.concatenate([rng.uniform(0, 1e300, (100, 3)), ref[100:150]]), True


def _extent_1e150(rng):
    ref = rng.uniform(-1e150, 1e150, (300, 3))
    return ref, rng.uniform(-1.2e150, 1.2e150, (257, 3)), False


def _growth(rng):
    """Extents 1e-12 x 1 x 1e6: the edge starts at the clip (largest extent / 2^19) with 2^19 + 1 cells and grows until they fit."""
    box = np.array([1e-12, 1.0, 1e6])
    return rng.uniform(0, 1, (2000, 3)) * box, rng.uniform(-0.05, 1.05, (500, 3)) * box, False


def _line(rng):
    """300 001 rows on a line: the edge is clipped at extent / 2^19.  The queries lie within a few row spacings of the line (further
    away the two nearest rows are equally far to within 1e-9) and past both of its ends."""
    n, L = 300001, 37.0
    ref = np.stack([np.sort(rng.uniform(0, L, n)), np.full(n, 1.5), np.full(n, -2.0)], 1)[rng.permutation(n)]
    q = np.stack([rng.uniform(-0.01 * L, 1.01 * L, 500), 1.5 + rng.uniform(-1, 1, 500) * 1e-5 * L, -2.0 + rng.uniform(-1, 1, 500) * 1e-5 * L], 1)
    return ref, q, False


def _long_scan(rng):
    """5 000 rows in one cell and one outlier that sets the extent."""
    ref = np.concatenate([rng.uniform(0, 1e-3, (5000, 3)), [[100.0, 100.0, 100.0]]])
    q = np.concatenate([rng.uniform(0, 1e-3, (100, 3)), rng.uniform(-1, 101, (100, 3)), 100 + rng.uniform(-1, 1, (20, 3))])
    return ref, q, False


def _overflow(rng):
    """Rows and queries at +-1e160 (x 0.5 ... 1.5): every d2 is +inf; row 0 is not finite, so the answer is row 1."""
    ref = rng.choice([-1.0, 1.0], (200, 3)) * rng.uniform(0.5, 1.5, (200, 3)) * 1e160
    ref[0, 1] = np.nan
    return ref, rng.choice([-1.0, 1.0], (100, 3)) * rng.uniform(0.5, 1.5, (100, 3)) * 1e160, True


def _lattice(m):
    def make(rng):
        """m^3 integer lattice in shuffled row order; queries at face centres (2 tied rows), edge centres (4), cell centres (8), and
        at the midpoints of rows 3 apart along an axis: the tied rows lie in different cells, and in different shells."""
        g = np.stack(np.meshgrid(*[np.arange(float(m))] * 3, indexing='ij'), -1).reshape(-1, 3)
        ref = g[rng.permutation(len(g))]
        c = np.stack(np.meshgrid(*[np.arange(m - 1.0)] * 3, indexing='ij'), -1).reshape(-1, 3)
        q = np.concatenate([c + [0.5, 0, 0], c + [0, 0.5, 0], c + [0, 0, 0.5], c + [0.5, 0.5, 0], c + [0, 0.5, 0.5], c + [0.5, 0, 0.5], c + 0.5])
        return ref, q, True
    return make


def _half_nonfinite(rng):
    ref = rng.uniform(0, 4, (400, 3))
    bad = rng.permutation(400)[:200]
    ref[bad, rng.integers(0, 3, 200)] = rng.choice([np.nan, np.inf, -np.inf], 200)
    return ref, rng.uniform(-1, 5, (257, 3)), False


def _row0_nonfinite(rng):
    ref = rng.uniform(0, 4, (257, 3))
    ref[0] = [np.inf, np.nan, 0.0]
    return ref, np.concatenate([rng.uniform(-1, 5, (100, 3)), [[0.0, 0.0, 0.0]]]), False


def _only_last_finite(rng):
    ref = np.full((257, 3), np.nan)
    ref[::2, 0] = np.inf
    ref[-1] = [0.25, -3.0, 7.0]
    return ref, rng.uniform(-10, 10, (65, 3)), False


def _sizes(n_ref, n_q):
    def make(rng):
        return rng.uniform(0, 1, (n_ref, 3)), rng.uniform(-0.1, 1.1, (n_q, 3)), False
    return make


def _large(rng):
    """100 001 x 1 000: the largest case brute force answers in about a second."""
    box = np.array([10.0, 8.0, 3.0])
    return rng.uniform(0, 1, (100001, 3)) * box, rng.uniform(-0.02, 1.02, (1000, 3)) * box, False


EDGES = {'outside': _outside, 'one_row': _one_row, 'two_identical': _two_identical, 'all_identical': _all_identical,
         'denormal': _denormal, 'extent_1e300': _extent_1e300, 'extent_1e150': _extent_1e150, 'growth': _growth, 'line': _line,
         'long_scan': _long_scan, 'overflow': _overflow, 'lattice5': _lattice(5), 'lattice6': _lattice(6), 'lattice7': _lattice(7),
         'half_nonfinite': _half_nonfinite, 'row0_nonfinite': _row0_nonfinite, 'only_last_finite': _only_last_finite, 'large': _large, 'equidistant': _equidistant, 'denormal_min': _denormal_min}
EDGES.update({'sizes:%dx%d' % (a, b): _sizes(a, b) for a in (255, 256, 257) for b in (255, 256, 257)})
EDGE_ORDER = list(EDGES)
SHELLS = ['shell:%s:%d' % (k, r) for k in SHELL_DIRS for r in SHELL_R]


def edge_case(name):
    """(ref, q, ties) of an edge case or of a shell case, made once."""
    if name not in _cache:
        if name.startswith('shell:'):
            _, kind, r = name.split(':')
            ref, q = shell_case(kind, int(r))[:2]
            ties = False
        else:
            ref, q, ties = EDGES[name](np.random.default_rng(SEED + 100 + EDGE_ORDER.index(name)))
        ref.setflags(write=False); q.setflags(write=False)
        _cache[name] = (ref, q, ties)
    return _cache[name]


_brute_cache = {}


def edge_brute(name):
    """`brute` of an edge case, computed once and shared by the tests that need it."""
    if name not in _brute_cache:
        out = brute(*edge_case(name)[:2])
        for a in out:
            a.setflags(write=False)
        _brute_cache[name] = out
    return _brute_cache[name]


def d2_rows(ref, q):
    """(m, n) squared distances in the contract's order."""
    dx = q[:, None, 0] - ref[None, :, 0]
    dy = q[:, None, 1] - ref[None, :, 1]
    dz = q[:, None, 2] - ref[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def brute(ref, q, chunk=2048):
    """(idx int64 (m), d2 float64 (m), second-smallest d2 (m)) by brute force; non-finite ref rows never win, a non-finite query
    gets -1 / NaN.  ``second`` is inf when fewer than two finite rows exist."""
    m = len(q)
    idx = np.full(m, -1, np.int64)
    best = np.full(m, np.nan)
    second = np.full(m, np.inf)
    ok_ref = np.isfinite(ref).all(1)
    ok_q = np.isfinite(q).all(1)
    if not ok_ref.any():
        return idx, best, second
    finite = np.nonzero(ok_ref)[0]                  # only these are candidates: where every d2 overflows to +inf the first minimum
    fref = ref[finite]                              # must still be a finite row
    chunk = max(1, min(chunk, (1 << 23) // max(1, len(fref))))
    with np.errstate(all='ignore'):
        for s in range(0, m, chunk):
            d2 = d2_rows(fref, q[s:s + chunk])
            i = np.argmin(d2, 1)                                        # the first minimum: the lowest row
            rows = np.arange(len(i))
            b = d2[rows, i]
            if len(finite) > 1:
                d2[rows, i] = np.inf
                second[s:s + chunk] = d2.min(1)
            idx[s:s + chunk] = finite[i]
            best[s:s + chunk] = b
    idx[~ok_q] = -1
    best[~ok_q] = np.nan
    second[~ok_q] = np.inf
    return idx, best, second
