"""Rules and cases for csrc/cluster.hip (b2m_dbscan, b2m_paint_proposals, b2m_joint_hist): plain numpy / Python, no torch, no device.

DBSCAN: the brute-force labelling of _s3dis_rule.dbscan_rule is THE rule; `dbscan_tree` is its tree-accelerated twin (cKDTree pairs
at a slightly larger radius, then the exact sq_dists filter) and `dbscan_variant` holds the deliberate mistakes that show the cases
are sharp.  `cell_order` / `pass1_trace` restate how the kernel bins, sorts and walks the rows (its constants copied as literals)
so that the reach predicates of tests/test_eval_rules.py are computed from the input.  Paint: evaluation.py:177-193 over boolean
rows.  Joint histogram: np.add.at with out-of-range rows skipped."""
import numpy as np

import _s3dis_rule as R

DB_THREADS, DB_CELL_BITS, DB_SCAN_BLOCK = 256, 21, 1024           # csrc/cluster.hip
DB_CELL_MAX = (1 << DB_CELL_BITS) - 1
PAINT_THREADS, JH_LDS, JH_MAX = 1024, 4096, 1 << 24
JH_GRID = 2048 * 256                                               # threads of the largest joint_hist grid


# ------------------------------------------------------------------ DBSCAN
def _neighbours_brute(x, eps2, strict=False, chunk=1024):
    out = []
    with np.errstate(invalid='ignore'):
        for s in range(0, len(x), chunk):
            d2 = R.sq_dists(x[s:s + chunk], x)
            out.extend(np.nonzero(r)[0] for r in ((d2 < eps2) if strict else (d2 <= eps2)))
    return out


def _neighbours_tree(x, eps, eps2):
    """cKDTree.query_pairs over the finite rows at eps * (1 + 1e-9), then the exact filter; a non-finite row neighbours nothing."""
    from scipy.spatial import cKDTree
    n = len(x)
    fin = np.nonzero(np.isfinite(x).all(1))[0]
    lists = [[] for _ in range(n)]
    if len(fin):
        xf = x[fin]
        pairs = cKDTree(xf).query_pairs(eps * (1 + 1e-9), output_type='ndarray')
        d2 = np.zeros(len(pairs))
        for j in range(x.shape[1]):
            df = xf[pairs[:, 0], j] - xf[pairs[:, 1], j]
            d2 += df * df
        pairs = fin[pairs[d2 <= eps2]]
        for i in fin:
            lists[i].append(i)                                      # d2 == 0 <= eps2: a finite row neighbours itself
        for a, b in pairs.tolist():
            lists[a].append(b); lists[b].append(a)
    return [np.array(sorted(v), np.int64) for v in lists]


def _label(nbrs, n, min_samples, variant=None):
    count = np.array([len(v) for v in nbrs])
    if variant == 'noself':
        count = np.array([int((v != i).sum()) for i, v in enumerate(nbrs)])
    core = count >= min_samples
    parent = np.arange(n)

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for i in np.nonzero(core)[0]:
        for j in nbrs[i]:
            if core[j] and j < i:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    roots = np.array([find(i) if core[i] else -1 for i in range(n)])
    order = np.unique(roots[roots >= 0])
    if variant == 'number_by_largest':
        last = {r: int(np.nonzero(roots == r)[0].max()) for r in order}
        order = np.array(sorted(order, key=lambda r: last[r]), np.int64)
    number = {int(r): k for k, r in enumerate(order)}
    labels = np.full(n, -1, np.int32)
    for i in range(n):
        if core[i]:
            labels[i] = number[int(roots[i])]
        else:
            c = {number[int(roots[j])] for j in nbrs[i] if core[j]}
            if c:
                labels[i] = max(c) if variant == 'border_high' else min(c)
    return labels, core, np.sort(order)


def dbscan_tree(x, eps, min_samples):
    """(labels, core, roots): the twin of _s3dis_rule.dbscan_rule for large n; roots = the smallest core row of every cluster."""
    x = np.asarray(x, np.float64)
    if len(x) == 0:
        return np.zeros(0, np.int32), np.zeros(0, bool), np.zeros(0, np.int64)
    return _label(_neighbours_tree(x, eps, eps * eps), len(x), min_samples)


DBSCAN_VARIANTS = ('lt', 'noself', 'border_high', 'number_by_largest', 'drop_last')


def dbscan_variant(x, eps, min_samples, variant):
    """The rule with one deliberate mistake: labels only."""
    x = np.asarray(x, np.float64)
    if variant == 'drop_last':
        x = x[:, :-1]
    return _label(_neighbours_brute(x, eps * eps, strict=variant == 'lt'), len(x), min_samples, variant)[0]


def rule_labels(x, eps, min_samples):
    """The brute-force rule with its warnings about NaN rows silenced: (labels, core, two)."""
    with np.errstate(invalid='ignore'):
        return R.dbscan_rule(x, eps, min_samples)


def cell_order(x, eps):
    """How the kernel bins and sorts: (keys (n) uint64, order (n): original row of every sorted position, cells (n, 3))."""
    x = np.asarray(x, np.float64)
    edge = eps * (1.0 + 1.0 / 1048576.0)
    with np.errstate(invalid='ignore'):
        lo = np.fmin.reduce(x[:, :3], 0)                            # (db_enc orders a positive NaN above +inf: it never is the minimum)
        u = np.floor((x[:, :3] - lo) / edge)
        c = np.where(u >= DB_CELL_MAX, DB_CELL_MAX, np.where(u > 0, u, 0)).astype(np.int64)
    keys = (c[:, 0] << (2 * DB_CELL_BITS)) | (c[:, 1] << DB_CELL_BITS) | c[:, 2]
    return keys.astype(np.uint64), np.argsort(keys, kind='stable'), c


def runs_of(keys_sorted):
    """[start, end) of every run of equal keys in the sorted order."""
    cut = np.nonzero(np.diff(keys_sorted.astype(np.int64)))[0] + 1
    return np.concatenate([[0], cut]), np.concatenate([cut, [len(keys_sorted)]])


def pass1_trace(x, eps, min_samples):
    """For every row: (tiles, done_tile, total_tiles) of the count pass -- the number of 256-row tiles the row's workgroup streams
    for the row's cell before the early exit, the tile in which THIS row reaches min_samples (-1: never) and the number of tiles
    the nine runs have in all.  Restated from db_pass_kernel<D, 1>: nine runs (x - 1 ... x + 1) x (y - 1 ... y + 1), each the
    z - 1 ... z + 1 stretch of the sorted order, in tiles of 256 from the run's start; a block walks only its own rows of a cell."""
    x = np.asarray(x, np.float64)
    n = len(x)
    keys, order, _ = cell_order(x, eps)
    ks = keys[order].astype(np.int64)
    xs = x[order]
    eps2 = eps * eps
    done = np.full(n, -1)
    total = np.zeros(n, np.int64)
    walked = np.zeros(n, np.int64)
    starts, ends = runs_of(ks)
    for a, b in zip(starts, ends):
        key = int(ks[a])
        cx, cy, cz = key >> (2 * DB_CELL_BITS), (key >> DB_CELL_BITS) & DB_CELL_MAX, key & DB_CELL_MAX
        tiles = []
        for r in range(9):
            ax, ay = cx + r // 3 - 1, cy + r % 3 - 1
            if not (0 <= ax <= DB_CELL_MAX and 0 <= ay <= DB_CELL_MAX):
                continue
            base = (ax << (2 * DB_CELL_BITS)) | (ay << DB_CELL_BITS)
            lo = np.searchsorted(ks, base | max(cz - 1, 0), 'left')
            hi = np.searchsorted(ks, (base | min(cz + 1, DB_CELL_MAX)) + 1, 'left')
            tiles += [(t0, min(t0 + DB_THREADS, hi)) for t0 in range(lo, hi, DB_THREADS)]
        for blk in range(a // DB_THREADS, (b - 1) // DB_THREADS + 1):          # every block owning rows of the cell walks it alone
            rows = np.arange(max(a, blk * DB_THREADS), min(b, (blk + 1) * DB_THREADS))
            cnt = np.zeros(len(rows), np.int64)
            fin = np.full(len(rows), -1)
            used = 0
            for ti, (t0, t1) in enumerate(tiles):
                with np.errstate(invalid='ignore'):
                    hit = (R.sq_dists(xs[rows], xs[t0:t1]) <= eps2).sum(1)
                cnt += hit
                fin[(fin < 0) & (cnt >= min_samples)] = ti
                used = ti + 1
                if (fin >= 0).all():
                    break
            done[order[rows]] = fin
            total[order[rows]] = len(tiles)
            walked[order[rows]] = used
    return walked, done, total


def ninth_run_last(x, eps, row):
    """Original row of the last sorted position of the ninth run (x + 1, y + 1, z - 1 ... z + 1) of `row`'s cell, or -1."""
    keys, order, c = cell_order(x, eps)
    ks = keys[order].astype(np.int64)
    cx, cy, cz = (int(v) for v in c[row])
    base = ((cx + 1) << (2 * DB_CELL_BITS)) | ((cy + 1) << DB_CELL_BITS)
    lo = np.searchsorted(ks, base | max(cz - 1, 0), 'left')
    hi = np.searchsorted(ks, (base | min(cz + 1, DB_CELL_MAX)) + 1, 'left')
    return int(order[hi - 1]) if hi > lo else -1


# ---- cases.  Each is (x, eps, min_samples); the predicates they must meet are asserted in tests/test_eval_rules.py
SIZES = (1, 2, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049)
EPS = 0.25
EDGE = EPS * (1.0 + 1.0 / 1048576.0)


def _extra_columns(rng, n, d, eps):
    """Columns 3 ... d-1: zeros, except the last, which is 0 or 1.5 eps: the only column that separates some close pairs."""
    e = np.zeros((n, d - 3))
    if d > 3:
        e[:, -1] = rng.integers(0, 2, n) * 1.5 * eps
    return e


def size_case(n, d, seed=0):
    """n shuffled rows: a point at the origin (the corner of cell 0), one tight blob inside a single cell (more than 512 rows from
    n = 513 on: it spans three 256-row blocks), a scatter over a few cells of cluster / border / noise density, and -- from
    n = 1025 on -- two far clusters whose roots (smallest core rows) are rows 1023 and 1024."""
    rng = np.random.default_rng(1000 * d + n + seed)
    if n <= 2:
        x = np.concatenate([np.zeros((1, 3)), np.full((n - 1, 3), 0.1)])
        return np.concatenate([x, np.zeros((n, d - 3))], 1), EPS, 1
    blob_n = n if n == 513 else (600 if n >= 1023 else n // 2 + 7)
    far = 2 * 4 if n >= 1025 else 0
    rest = n - 1 - blob_n - far if n != 513 else 0
    parts = [np.zeros((1 if n != 513 else 0, 3))]
    parts.append((10.25 + 0.5 * rng.random((blob_n, 3))) * EDGE)           # inside cell (10, 10, 10), diameter < eps
    parts.append(rng.random((rest, 3)) * np.array([6.0, 5.0, 2.0]) * EDGE)
    xyz = np.concatenate(parts)
    if n == 513:
        xyz[0] = 10.0 * EDGE                                                # (the minimum: the blob's cell becomes cell 0)
    xyz = xyz[rng.permutation(len(xyz))]
    if far:
        # two stars far away: a centre with three satellites 0.9 eps from it and 1.56 eps from each other -- with min_samples 4
        # the centre is the only core row of its cluster, hence its root; the centres go to rows 1023 and 1024
        sat = 0.9 * EPS * np.array([[1.0, 0.0, 0.0], [-0.5, 0.75 ** 0.5, 0.0], [-0.5, -(0.75 ** 0.5), 0.0]])
        c1, c2 = np.array([40.0, 1.0, 1.0]) * EDGE, np.array([1.0, 40.0, 1.0]) * EDGE
        xyz = np.concatenate([xyz, c1 + sat, c2 + sat])
        xyz = np.concatenate([xyz[:1023], [c1, c2], xyz[1023:]])
        star = np.concatenate([np.arange(len(xyz) - 8, len(xyz) - 2), [1023, 1024]]) if len(xyz) == 1025 else \
            np.concatenate([np.arange(len(xyz) - 6, len(xyz)), [1023, 1024]])
    x = np.concatenate([xyz, _extra_columns(rng, len(xyz), d, EPS)], 1)
    if far:
        x[star, 3:] = 0.0                                                   # the stars stay whole
    assert len(x) == n
    return x, EPS, 4


def eq_eps_case(d):
    """Pairs at d2 == eps2 exactly (dyadic 3-4-5 offsets, the 4 in the last column) and pairs one ulp beyond; min_samples 2."""
    eps = 0.625
    rows = []
    for k in range(6):
        base = np.zeros(d); base[0] = 8.0 * k; base[1] = 2.0
        off = np.zeros(d); off[0] = 0.375; off[d - 1] = 0.5
        if k % 2:
            off[d - 1] = np.nextafter(0.5, 1.0)
        rows += [base, base + off]
    return np.array(rows), eps, 2


OFFSETS26 = [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)]


def cells26_case():
    """One isolated neighbour pair per cell offset (interior cells), and for each axis the pairs that start in a cell with
    coordinate 0 on that axis; a row at the origin fixes the corner.  eps 1, min_samples 2: a pair the walk misses is noise."""
    eps = 1.0
    edge = eps * (1.0 + 1.0 / 1048576.0)
    rows = [np.zeros(3)]
    for k, o in enumerate(OFFSETS26):
        o = np.array(o, np.float64)
        a = (np.array([4.0 * k + 2.0, 2.0, 2.0]) + 0.5 + 0.45 * o) * edge
        rows += [a, a + 0.1 * edge * o]
    k = 0
    for axis in range(3):
        for o in OFFSETS26:
            if o[axis] < 0:
                continue
            o = np.array(o, np.float64)
            c = np.zeros(3); c[(axis + 1) % 3] = 4.0 * k + 2.0; c[(axis + 2) % 3] = 6.0 + 4.0 * axis
            a = (c + 0.5 + 0.45 * o) * edge
            rows += [a, a + 0.1 * edge * o]
            k += 1
    return np.array(rows), eps, 2


def ninth_run_case():
    """Rows that reach min_samples exactly with the last row of the ninth run: the only row of cell (+1, +1, +1)."""
    eps = 1.0
    edge = eps * (1.0 + 1.0 / 1048576.0)
    rows = [np.zeros(3)]
    for k, ms_extra in enumerate((0, 3)):
        c = np.array([4.0 * k + 1.0, 1.0, 1.0])
        q = (c + 0.95) * edge
        rows += [q] + [q - 0.01 * (i + 1) * edge for i in range(ms_extra)]      # the cell's own rows
        rows += [(c + 1.05) * edge]                                             # the partner in (+1, +1, +1)
    return np.array(rows), eps, None                                            # min_samples is 2 for group 0 ...


def tiles_case():
    """One cell of 600 rows: 300 identical rows that reach min_samples = 2 in the first tile, and 300 rows, apart from each other in
    column 3, whose second neighbour is one of the 300 rows of cell (+1, +1, 0) -- the ninth run.  d = 4.  The cell is (2, 2, 2): the
    row at the origin is in none of its runs."""
    eps = 1.0
    edge = eps * (1.0 + 1.0 / 1048576.0)
    i = np.arange(300.0)
    a = np.tile([[2.5 * edge, 2.5 * edge, 2.5 * edge, -10.0]], (300, 1))
    b = np.stack([np.full(300, 2.95 * edge), np.full(300, 2.95 * edge), np.full(300, 2.5 * edge), 2.0 * i], 1)
    p = np.stack([np.full(300, 3.05 * edge), np.full(300, 3.05 * edge), np.full(300, 2.5 * edge), 2.0 * i], 1)
    return np.concatenate([np.zeros((1, 4)), a, b, p]), eps, 2


def clamp_case():
    """eps = 2^-10 over coordinates 0 ... 8192: 2^23 cells along x, clamped to DB_CELL_MAX from x ~ 2048 on.  A cluster at each end,
    and at x = 5000 two clusters 0.605 / 0.3 eps ... apart with one border row between them (the shape of `shared_border`)."""
    eps = 2.0 ** -10
    s = eps / 0.3
    a = np.array([[0.001 * i, 0.0, 0.0] for i in range(10)])
    b = np.array([[0.605 + 0.001 * i, 0.0, 0.0] for i in range(10)])
    mid = np.array([[0.3065, 0.0, 0.0]])
    grp = np.concatenate([b, mid, a]) * s
    grp[:, 0] += 5000.0
    low = np.tile([[0.0, 0.0, 0.0]], (10, 1)); low[:, 1] = np.arange(10) * eps * 0.05
    high = np.tile([[8192.0, 0.0, 0.0]], (10, 1)); high[:, 2] = np.arange(10) * eps * 0.05
    return np.concatenate([grp, low, high]), eps, 10


def nonfinite_case(min_samples):
    rng = np.random.default_rng(11)
    x = rng.random((297, 5)) * np.array([2.0, 2.0, 1.0, 0.1, 0.1])
    bad = np.tile(x[:3], (1, 1)).copy()
    bad[0, 1] = np.nan; bad[1, 0] = np.inf; bad[2, 2] = -np.inf
    x = np.concatenate([x[:100], bad[:1], x[100:200], bad[1:2], x[200:], bad[2:]])
    return x, 0.2, min_samples


def edge_cases():
    """name -> (x, eps, min_samples)."""
    rng = np.random.default_rng(7)
    out = {}
    for d in range(3, 9):
        out['cols:%d' % d] = size_case(700, d, seed=5)
        out['eq_eps:%d' % d] = eq_eps_case(d)
    out['cells26'] = cells26_case()
    x, eps, _ = ninth_run_case()
    out['ninth_run:2'] = (x[:3], eps, 2)
    out['ninth_run:5'] = (np.concatenate([x[:1], x[3:]]), eps, 5)
    out['tiles'] = tiles_case()
    out['clamp'] = clamp_case()
    out['ms1'] = (rng.random((300, 3)) * 3.0, 0.25, 1)
    out['nonfinite:1'] = nonfinite_case(1)
    out['nonfinite:3'] = nonfinite_case(3)
    out['identical'] = (np.tile([[1.0, 2.0, 3.0, 0.5]], (700, 1)), 0.35, 10)
    out['identical_short'] = (np.tile([[1.0, 2.0, 3.0, 0.5]], (9, 1)), 0.35, 10)
    out['zero_core'] = (np.arange(40.0)[:, None] * np.ones((1, 3)), 0.5, 2)
    x, eps, ms = shared_border_case()
    out['shared_border'] = (x, eps, ms)
    return out


def shared_border_case():
    a = np.array([[0.001 * i, 0.0, 0.0] for i in range(10)])
    b = np.array([[0.605 + 0.001 * i, 0.0, 0.0] for i in range(10)])
    mid = np.array([[0.3065, 0.0, 0.0]])
    return np.concatenate([b, mid, a]), 0.3, 10


def size_cases():
    return {'n:%d' % n: size_case(n, 3 + i % 6) for i, n in enumerate(SIZES)}


LATTICE_N = 262145                                                   # cdiv(n, 1024) = 257 block sums: two per thread of db_blockscan


def lattice_case():
    """262 145 rows of a lattice spaced 2 eps, min_samples 1: labels == arange(n), n_clusters == n."""
    i = np.arange(LATTICE_N)
    x = np.stack([i % 64, (i // 64) % 64, i // 4096], 1).astype(np.float64) * 0.5
    return x, 0.25, 1


# ------------------------------------------------------------------ paint (evaluation.py:177-193)
PAINT_VARIANTS = ('le', 'ratio_all', 'dense_ids', 'sem_min_off')


def paint_rule(masks, sem, sem_min=3, ratio=0.6, min_points=200, sem_in=None, variant=None):
    """masks (k, n) bool in row order, sem (k): (accepted (k) int32, inst (n) int32, sem_out (n) int32 or None, unlabeled (n) bool).
    The instance id of row r is r + 1; the ratio test is not (f / o < ratio) in fp64, so 0 / 0 passes it."""
    masks = np.asarray(masks, bool)
    k, n = masks.shape
    inst = np.full(n, -1, np.int32)
    sem_out = None if sem_in is None else np.array(sem_in, np.int32)
    accepted = np.zeros(k, np.int32)
    taken = 0
    for r in range(k):
        unlabeled = inst < 0
        o = np.count_nonzero(masks[r])
        if sem[r] < sem_min + (variant == 'sem_min_off'):
            continue
        m = masks[r] & unlabeled
        f = np.count_nonzero(m)
        with np.errstate(invalid='ignore', divide='ignore'):
            q = np.float64(1.0 * (o if variant == 'ratio_all' else f)) / np.float64(o)
            if (q <= ratio) if variant == 'le' else (q < ratio):
                continue
        if f < min_points:
            continue
        taken += 1
        inst[m] = taken if variant == 'dense_ids' else r + 1
        if sem_out is not None:
            sem_out[m] = sem[r]
        accepted[r] = 1
    return accepted, inst, sem_out, inst < 0


def pack_rows(masks, pad=False):
    """(k, n) bool -> (k, ceil(n / 64)) uint64 in the layout of b2m_mask_pack (bit p % 64 of word p / 64; pad bits zero, or all set)."""
    masks = np.asarray(masks, bool)
    k, n = masks.shape
    words = (n + 63) // 64
    full = np.zeros((k, max(words, 1) * 64), bool)
    full[:, :n] = masks
    if pad:
        full[:, n:] = True
    return np.packbits(full, axis=1, bitorder='little').view(np.uint64).reshape(k, -1)[:, :max(words, 1)].copy()


PAINT_SIZES = (1, 63, 64, 65, 65535, 65536, 65537, 131073)


def paint_size_case(n):
    """Six random rows of mixed density and class over n points; thresholds that reject and accept some of them."""
    rng = np.random.default_rng(n)
    dens = np.array([0.5, 0.4, 0.6, 0.02, 0.3, 0.9])
    masks = rng.random((6, n)) < dens[:, None]
    sem = np.array([5, 2, 3, 7, 4, 9], np.int32)
    return {'masks': masks, 'sem': sem, 'sem_min': 3, 'ratio': 0.6, 'min_points': max(1, n // 20), 'sem_in': np.full(n, 1, np.int32)}


def paint_edge_cases():
    out = {}
    n = 70
    m = np.zeros((2, n), bool); m[0, :2] = True; m[1, :5] = True              # row 1: 3 of 5 unlabeled == 0.6
    out['ratio_eq'] = {'masks': m, 'sem': np.array([4, 5], np.int32), 'sem_min': 3, 'ratio': 0.6, 'min_points': 1}
    m = np.zeros((2, n), bool); m[0, :3] = True; m[1, :5] = True              # row 1: 2 of 5
    out['ratio_below'] = {'masks': m, 'sem': np.array([4, 5], np.int32), 'sem_min': 3, 'ratio': 0.6, 'min_points': 1}
    m = np.zeros((3, 500), bool); m[0, :200] = True; m[1, 200:399] = True; m[2, 200:400] = True   # 200, 199, 200 unlabeled points
    out['min_points_eq'] = {'masks': m, 'sem': np.array([4, 5, 6], np.int32), 'sem_min': 3, 'ratio': 0.1, 'min_points': 200}
    m = np.zeros((3, 130), bool); m[1, :20] = True
    out['empty_row:0'] = {'masks': m, 'sem': np.array([4, 5, 6], np.int32), 'sem_min': 3, 'ratio': 0.6, 'min_points': 0}
    out['empty_row:200'] = dict(out['empty_row:0'], min_points=200)
    m = np.zeros((4, 100), bool); m[0, :30] = True; m[1, 30:60] = True; m[2, 60:90] = True; m[3, 90:] = True
    out['sem_edge'] = {'masks': m, 'sem': np.array([2, 3, 6, 7], np.int32), 'sem_min': 3, 'ratio': 0.6, 'min_points': 1}
    out['sem_edge:7'] = dict(out['sem_edge'], sem_min=7)
    # a chain: row 0 accepted; row 1 loses half to it and is rejected; row 2 overlaps row 1 only and is accepted BECAUSE row 1 was
    # rejected; row 3 loses most to row 2
    m = np.zeros((4, 400), bool); m[0, :100] = True; m[1, 50:150] = True; m[2, 100:250] = True; m[3, 200:260] = True
    out['chain'] = {'masks': m, 'sem': np.array([4, 5, 6, 7], np.int32), 'sem_min': 3, 'ratio': 0.6, 'min_points': 10}
    out['k0'] = {'masks': np.zeros((0, 100), bool), 'sem': np.zeros(0, np.int32), 'sem_min': 3, 'ratio': 0.6, 'min_points': 1}
    for v in out.values():
        v['sem_in'] = np.full(v['masks'].shape[1], 1, np.int32)
    out['no_sem_out'] = dict(out['chain'], sem_in=None)
    return out


def paint_run_rule(case, variant=None):
    return paint_rule(case['masks'], case['sem'], case['sem_min'], case['ratio'], case['min_points'], case['sem_in'], variant)


# ------------------------------------------------------------------ joint histogram
def joint_hist_rule(a, b, na, nb):
    a = np.asarray(a, np.int64)
    b = np.zeros_like(a) if b is None else np.asarray(b, np.int64)
    ok = (a >= 0) & (a < na) & (b >= 0) & (b < nb)
    h = np.zeros((na, nb), np.int32)
    np.add.at(h, (a[ok], b[ok]), 1)
    return h


def joint_hist_cases():
    rng = np.random.default_rng(2)
    I = np.iinfo(np.int32)
    out = {}
    for na, nb in ((1, 1), (4095, 1), (64, 64), (4097, 1), (17, 241), (241, 17)):
        n = 5000
        a = rng.integers(-1, na + 1, n).astype(np.int32)
        b = rng.integers(-1, nb + 1, n).astype(np.int32)
        a[:4] = [-1, na, I.min, I.max]
        b[4:8] = [-1, nb, I.min, I.max]
        out['cells:%dx%d' % (na, nb)] = (a, b, na, nb)
    out['b_null'] = (rng.integers(-1, 4098, 3000).astype(np.int32), None, 4097, 1)
    out['one_cell'] = (np.full(70000, 3, np.int32), np.full(70000, 2, np.int32), 5, 7)
    out['one_cell_global'] = (np.full(70000, 699, np.int32), np.full(70000, 8, np.int32), 700, 9)
    out['n0'] = (np.zeros(0, np.int32), np.zeros(0, np.int32), 13, 13)
    return out
