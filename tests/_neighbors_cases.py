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
    with np.errstate(all='ignore'):
        for s in range(0, m, chunk):
            d2 = d2_rows(ref, q[s:s + chunk])
            d2[:, ~ok_ref] = np.inf
            i = np.argmin(d2, 1)                                        # the first minimum: the lowest row
            rows = np.arange(len(i))
            b = d2[rows, i]
            if ok_ref.sum() > 1:
                d2[rows, i] = np.inf
                second[s:s + chunk] = d2.min(1)
            idx[s:s + chunk] = i
            best[s:s + chunk] = b
    idx[~ok_q] = -1
    best[~ok_q] = np.nan
    second[~ok_q] = np.inf
    return idx, best, second
