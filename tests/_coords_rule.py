"""Coordinate maps, kernel maps, tile rulebooks, XCD runs and row-order keys restated from their definitions, for
tests/test_coords_rule.py (CPU) and tests/test_gpu_coords_edges.py (the kernels of csrc/coords.hip).

The definitions are those of oracle/sparse_ref.py's header and include/b2m.h:

  * a row is the tuple (b, x, y, z); the coordinate set of a level is a Python dict keyed by that tuple whose value is the FIRST
    row carrying it.  Nothing is packed into 16-bit fields: a probe outside [0, 65535] finds no key, so there is no range guard
    this module could forget (the device packs four 16-bit fields into a uint64 and needs one);
  * strided level at tensor stride ts: every axis floored to a multiple of 2*ts, coarse rows in order of FIRST OCCURRENCE in the
    finer level's row order, parent = coarse row, koff = ox + 2*oy + 4*oz with o = (c - coarse) / ts in {0, 1}^3;
  * stride-1 kernel map of an odd kernel: offsets centred, x fastest, k = (dx+h) + ks*(dy+h) + ks^2*(dz+h), times ts;
  * child[koff[i], parent[i]] = i and up[koff[i], i] = parent[i], -1 elsewhere;
  * tile rulebook: per (offset, tile of 64 output rows) the valid pairs compacted in row order, padding -1 / 0;
  * the tail of rb_cnt: per-tile cost, nine run starts (targets ceil(total*x/8), forward then backward clamp by the cap),
    dispatch order (last 768 positions of a run by cost class, 8 classes below the window's largest cost, stable);
  * Morton / Hilbert keys: batch index from bit 48 up, 3 x bits interleaved below, as UNSIGNED 64-bit values.

Every function takes switches that turn it into one deliberate MISTAKE (an unguarded 16-bit pack, z-fastest offsets, ...):
tests/test_coords_rule.py shows that each mistake fails at least one case of the shared lists below, i.e. that the cases are
sharp.  Every case carries predicates -- computed by the rule, asserted when the case is built -- for the branch it exists
for, so a case cannot silently stop reaching it.
"""
import functools

import numpy as np

TILE = 64
WINDOW = 768                    # B2M_XCD_WINDOW
NCLS = 8                        # B2M_XCD_CLASSES
BALANCE_MIN_TILES = 64
OCC_MAX_BYTES = 256 << 20       # CoordinateManager.OCC_MAX_BYTES
SCAN_ITEMS = 1024               # rows per scan block of b2m_coords_stride; its carry loop takes 256 blocks per trip
COORD_MAX = 65534


def xcd_cap(nt):
    """B2M_XCD_CAP: ceil(1.25 * nt / 8)."""
    return (nt * 5 + 31) // 32


# ----------------------------------------------------------------------------- coordinate sets
def _rows(coords):
    return [tuple(r) for r in np.asarray(coords).reshape(-1, 4).tolist()]


def first_rows(coords):
    """dict (b,x,y,z) -> first row with that coordinate."""
    d = {}
    for i, r in enumerate(_rows(coords)):
        d.setdefault(r, i)
    return d


def dup_count(coords):
    """Rows that are not the first of their coordinate."""
    return len(_rows(coords)) - len(first_rows(coords))


def strided_level(coords, ts, mistake=None):
    """(coarse (M,4) int32, parent (N,) int32, koff (N,) int32).
    mistakes: 'round_ts' floors to ts, 'sorted' orders the coarse rows lexicographically, 'koff_swap' exchanges x and z."""
    step = ts if mistake == 'round_ts' else 2 * ts
    rows = _rows(coords)
    coarse, index, parent, koff = [], {}, [], []
    for (b, x, y, z) in rows:
        c = (b, x // step * step, y // step * step, z // step * step)
        if c not in index:
            index[c] = len(coarse)
            coarse.append(c)
        parent.append(index[c])
        ox, oy, oz = (x - c[1]) // ts, (y - c[2]) // ts, (z - c[3]) // ts
        if mistake == 'koff_swap':
            ox, oz = oz, ox
        koff.append(ox + 2 * oy + 4 * oz)
    parent = np.array(parent, np.int32).reshape(-1)
    if mistake == 'sorted':
        order = sorted(range(len(coarse)), key=lambda i: coarse[i])
        rank = np.empty(len(coarse), np.int32)
        rank[order] = np.arange(len(coarse), dtype=np.int32)
        coarse = [coarse[i] for i in order]
        parent = rank[parent] if len(parent) else parent
    return (np.array(coarse, np.int32).reshape(-1, 4), parent, np.array(koff, np.int32).reshape(-1))


def offsets(ksize, mistake=None):
    """[(dx,dy,dz)] of an odd kernel, centred, x fastest ('z_fastest': the mistake)."""
    assert ksize in (1, 3, 5, 7)
    h = ksize // 2
    r = range(-h, h + 1)
    if mistake == 'z_fastest':
        return [(dx, dy, dz) for dx in r for dy in r for dz in r]
    return [(dx, dy, dz) for dz in r for dy in r for dx in r]


def _pack16_unguarded(b, x, y, z):
    """What a 16-bit-per-field pack without a range guard makes of a probe: the carry is an OR into the next field."""
    m = (1 << 64) - 1
    return (((b & 0xFFFFFFFF) << 48) | ((x & 0xFFFFFFFF) << 32) | ((y & 0xFFFFFFFF) << 16) | (z & 0xFFFFFFFF)) & m


def kernel_map(coords, ksize, ts, mistake=None):
    """nbr[k, o] = first row at coords[o] + offset_k * ts, or -1.
    mistakes: 'pack16' probes with an unguarded 16-bit pack, 'z_fastest', 'bitmap_nomask' answers from a bitmap
    ((b*Z + z)*Y + y)*X + x without masking the positions left of x = 0 and right of X-1 (level 0 only, ts = 1)."""
    rows = _rows(coords)
    n = len(rows)
    offs = offsets(ksize, mistake)
    nbr = np.full((len(offs), n), -1, np.int32)
    if n == 0:
        return nbr
    first = first_rows(coords)
    if mistake == 'pack16':
        packed = {_pack16_unguarded(*r): i for r, i in first.items()}
        for k, (dx, dy, dz) in enumerate(offs):
            nbr[k] = [packed.get(_pack16_unguarded(b, x + dx * ts, y + dy * ts, z + dz * ts), -1) for (b, x, y, z) in rows]
        return nbr
    if mistake == 'bitmap_nomask' and ts == 1:
        _, X, Y, Z = (int(v) + 1 for v in np.asarray(coords).max(0))
        cell = {((b * Z + z) * Y + y) * X + x: i for (b, x, y, z), i in first.items()}
        for k, (dx, dy, dz) in enumerate(offs):
            nbr[k] = [cell.get(((b * Z + z + dz) * Y + y + dy) * X + x + dx, -1)
                      if 0 <= y + dy < Y and 0 <= z + dz < Z else -1 for (b, x, y, z) in rows]
        return nbr
    get = first.get
    for k, (dx, dy, dz) in enumerate(offs):
        nbr[k] = [get((b, x + dx * ts, y + dy * ts, z + dz * ts), -1) for (b, x, y, z) in rows]
    return nbr


def alias_hits(coords, ksize, ts):
    """Per axis (x, y, z): probes that leave [0, 65535] on that axis alone and whose UNGUARDED 16-bit pack equals the key of
    a row that is present -- the false neighbours the range guard of the kernel maps exists to refuse."""
    first = first_rows(coords)
    packed = {_pack16_unguarded(*r) for r in first}
    hits = [0, 0, 0]
    for (b, x, y, z) in first:
        for (dx, dy, dz) in offsets(ksize):
            q = (x + dx * ts, y + dy * ts, z + dz * ts)
            out = [not 0 <= v < 65536 for v in q]
            if sum(out) == 1 and _pack16_unguarded(b, *q) in packed:
                hits[out.index(True)] += 1
    return hits


def child_table(parent, koff, n_coarse):
    """child[koff[i], parent[i]] = i, -1 elsewhere (no two rows of a duplicate-free level share a (parent, koff) pair)."""
    t = np.full((8, n_coarse), -1, np.int32)
    t[koff, parent] = np.arange(len(parent), dtype=np.int32)
    return t


def up_table(parent, koff):
    """up[koff[i], i] = parent[i], -1 elsewhere."""
    t = np.full((8, len(parent)), -1, np.int32)
    t[koff, np.arange(len(parent))] = parent
    return t


# ----------------------------------------------------------------------------- tile rulebook
def encode_rulebook(nbr, n_out=None):
    """(rb_in int32[K*ldr], rb_out uint8[K*ldr], rb_cnt int32[K*ntiles], pair_total int32[K]) of a neighbour table
    (columns beyond n_out, a wider leading dimension, are not part of the map)."""
    nbr = np.asarray(nbr)
    K = nbr.shape[0]
    n_out = nbr.shape[1] if n_out is None else n_out
    nt = (n_out + TILE - 1) // TILE
    rb_in = np.full((K, nt, TILE), -1, np.int32)
    rb_out = np.zeros((K, nt, TILE), np.uint8)
    cnt = np.zeros((K, nt), np.int32)
    for k in range(K):
        row = nbr[k, :n_out]
        for t in range(nt):
            seg = row[t * TILE:(t + 1) * TILE]
            o = np.flatnonzero(seg >= 0)
            cnt[k, t] = len(o)
            rb_in[k, t, :len(o)] = seg[o]
            rb_out[k, t, :len(o)] = o
    return rb_in.reshape(-1), rb_out.reshape(-1), cnt.reshape(-1), cnt.sum(1).astype(np.int32)


def tile_cost(cnt):
    """cnt (K, ntiles): 3 per row group of 16 pairs + 1 per active offset, summed over the offsets of a tile."""
    cnt = np.asarray(cnt).astype(np.int64)
    return np.where(cnt > 0, 3 * ((cnt + 15) // 16) + 1, 0).sum(0)


def run_starts(cost, mistake=None, info=None):
    """The nine run starts.  Run x (1..7) begins behind the tile that carries the work prefix over ceil(total*x/8); no work at
    all: equal tile counts.  Then start[x] is clamped into [start[x-1], start[x-1] + cap] going forward and raised to
    start[x+1] - cap going backward.  mistakes: 'floor_target', 'forward_only'.  info (a dict) receives which clamp moved a start."""
    nt = len(cost)
    total = int(np.sum(cost))
    start = [nt * x // 8 for x in range(8)] + [nt]
    if total > 0:
        for x in range(1, 8):
            target = total * x // 8 if mistake == 'floor_target' else (total * x + 7) // 8
            run = 0
            for t in range(nt):
                before, run = run, run + int(cost[t])
                if before < target <= run:
                    start[x] = t + 1
                    break
    cap = xcd_cap(nt)
    fwd = bwd = False
    for x in range(1, 8):
        v = min(max(start[x], start[x - 1]), start[x - 1] + cap)
        fwd, start[x] = fwd or v != start[x], v
    if mistake != 'forward_only':
        for x in range(7, 0, -1):
            v = max(start[x], start[x + 1] - cap)
            bwd, start[x] = bwd or v != start[x], v
    if info is not None:
        info.update(forward_clamp=fwd, backward_clamp=bwd, total=total, cap=cap,
                    at_cap=any(start[x + 1] - start[x] == cap for x in range(8)))
    return np.array(start, np.int64)


def dispatch_order(cost, start, mistake=None):
    """order[j] = tile worked on at position j: row order up to the last WINDOW positions of every run, those by cost class
    (class = NCLS-1 - cost*NCLS // (largest cost of the window + 1), 0 = heaviest first), row order inside a class.
    mistake 'unstable': descending rows inside a class."""
    order = np.arange(len(cost), dtype=np.int64)
    for x in range(8):
        s0, s1 = int(start[x]), int(start[x + 1])
        w0 = max(s0, s1 - WINDOW)
        if s1 <= w0:
            continue
        c = np.asarray(cost[w0:s1]).astype(np.int64)
        cls = NCLS - 1 - c * NCLS // (int(c.max()) + 1)
        tiles = list(range(w0, s1))
        if mistake == 'unstable':
            tiles.reverse()
        order[w0:s1] = sorted(tiles, key=lambda t: cls[t - w0])          # sorted() is stable
    return order


def balance_tail(cnt, info=None):
    """(cost, nine starts, order) of a (K, ntiles) count array, as b2m_rulebook_balance writes them behind the counts."""
    cost = tile_cost(cnt)
    start = run_starts(cost, info=info)
    return cost, start, dispatch_order(cost, start)


# ----------------------------------------------------------------------------- helpers of tests/test_gpu_coords.py
def _decode_rulebook(rb):
    """tile rulebook -> neighbour table (K, n_out)."""
    from box2mask_amd.sparse import TILE
    K, n_out, nt = rb.K, rb.n_out, rb.ntiles
    ldr = nt * TILE
    rin = rb.rb_in[:K * ldr].cpu().numpy().reshape(K, nt, TILE)
    rout = rb.rb_out[:K * ldr].cpu().numpy().reshape(K, nt, TILE)
    cnt = rb.rb_cnt[:K * nt].cpu().numpy().reshape(K, nt)
    nbr = np.full((K, nt * TILE), -1, np.int32)
    for k in range(K):
        for t in range(nt):
            c = cnt[k, t]
            assert (rin[k, t, c:] == -1).all() and (rout[k, t, c:] == 0).all()
            o = rout[k, t, :c].astype(np.int64)
            assert (np.diff(o) > 0).all()                      # compacted in output-row order
            nbr[k, t * TILE + o] = rin[k, t, :c]
    return nbr[:, :n_out], int(cnt.sum())


def _expected_runs(cnt):
    """XCD work boundaries as include/b2m.h states them (rb_cnt tail), restated with numpy."""
    K, nt = cnt.shape
    cost = np.where(cnt > 0, 3 * ((cnt + 15) // 16) + 1, 0).sum(0).astype(np.int64)
    prefix = np.cumsum(cost)
    total = int(prefix[-1]) if nt else 0
    start = [nt * x // 8 for x in range(8)] + [nt]
    if total > 0:
        for x in range(1, 8):
            target = (total * x + 7) // 8
            start[x] = int(np.searchsorted(prefix, target, side='left')) + 1
    cap = (nt * 5 + 31) // 32
    for x in range(1, 8):
        start[x] = min(max(start[x], start[x - 1]), start[x - 1] + cap)
    for x in range(7, 0, -1):
        start[x] = max(start[x], start[x + 1] - cap)
    return cost, np.array(start), cap


def _hilbert_keys_numpy(c, bits):
    """Skilling's transform, vectorised (the restatement b2m_hilbert_keys is checked against)."""
    X = c[:, 1:4].astype(np.uint64).copy()
    M = np.uint64(1) << np.uint64(bits - 1)
    Q = M
    while Q > 1:
        P = Q - np.uint64(1)
        for a in range(3):
            sel = (X[:, a] & Q) != 0
            X[sel, 0] ^= P
            ns = ~sel
            t = (X[ns, 0] ^ X[ns, a]) & P
            X[ns, 0] ^= t
            X[ns, a] ^= t
        Q >>= np.uint64(1)
    X[:, 1] ^= X[:, 0]; X[:, 2] ^= X[:, 1]
    t = np.zeros(len(X), np.uint64)
    Q = M
    while Q > 1:
        t[(X[:, 2] & Q) != 0] ^= (Q - np.uint64(1))
        Q >>= np.uint64(1)
    X ^= t[:, None]
    k = c[:, 0].astype(np.uint64) << np.uint64(48)
    for bit in range(bits):
        for a in range(3):
            k |= ((X[:, a] >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + (2 - a))
    return k.astype(np.int64)


def _morton_keys_numpy(c):
    """Z-order key: batch index from bit 48 up, bit i of x / y / z at bit 3i / 3i+1 / 3i+2 (uint64)."""
    k = c[:, 0].astype(np.uint64) << np.uint64(48)
    for bit in range(16):
        for a, sh in ((1, 0), (2, 1), (3, 2)):
            k |= ((c[:, a].astype(np.uint64) >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + sh)
    return k


def morton_keys(coords):
    return _morton_keys_numpy(np.asarray(coords).reshape(-1, 4))


def hilbert_keys(coords, bits):
    """Unsigned: the int64 the device stores is this bit pattern (negative from batch index 32768 on)."""
    return _hilbert_keys_numpy(np.asarray(coords).reshape(-1, 4), bits).view(np.uint64)


def key_order(keys, mistake=None):
    """Stable argsort of the UNSIGNED keys ('signed': the mistake of comparing them as int64)."""
    keys = np.asarray(keys, np.uint64)
    return np.argsort(keys.view(np.int64) if mistake == 'signed' else keys, kind='stable')


# ----------------------------------------------------------------------------- the rule of one whole case
class Levels:
    """Everything CoordinateManager derives from one coordinate set, by the rule (cached per level / kernel)."""

    def __init__(self, coords, n_levels, mistake=None):
        self.mistake = mistake
        self.coords = [np.asarray(coords, np.int32).reshape(-1, 4)]
        self.parent, self.koff = [], []
        for l in range(n_levels - 1):
            c, p, k = strided_level(self.coords[l], 1 << l, mistake if mistake in ('round_ts', 'sorted', 'koff_swap') else None)
            self.coords.append(c); self.parent.append(p); self.koff.append(k)
        self._same = {}

    def n(self, l):
        return len(self.coords[l])

    def same(self, l, ksize):
        if (l, ksize) not in self._same:
            mk = self.mistake if self.mistake in ('pack16', 'z_fastest') or (self.mistake == 'bitmap_nomask' and l == 0) else None
            self._same[(l, ksize)] = kernel_map(self.coords[l], ksize, 1 << l, mk)
        return self._same[(l, ksize)]

    def down(self, l):
        return child_table(self.parent[l], self.koff[l], self.n(l + 1))

    def up(self, l):
        return up_table(self.parent[l], self.koff[l])


# ----------------------------------------------------------------------------- shared case lists
class Case:
    """coords (n,4) int32 in the order handed to the device; levels; the kernel sizes asked of level 0 (3 is asked of every
    level); `what` to compare ('all': maps and rulebooks of every level, 'strided': coordinates and k2s2 maps only,
    'dups': duplicate count and the strided level); predicates: {text: bool}, all asserted at construction."""

    def __init__(self, name, coords, levels, k0=(5,), what='all', predicates=None):
        self.name, self.levels, self.k0, self.what = name, levels, tuple(k0), what
        self.coords = np.ascontiguousarray(np.asarray(coords, np.int32).reshape(-1, 4))
        assert self.coords.size == 0 or (self.coords.min() >= 0 and self.coords.max() <= COORD_MAX), name
        self.predicates = dict(predicates or {})
        for text, ok in self.predicates.items():
            assert ok, 'case %s no longer reaches its branch: %s' % (name, text)
        self._rule = None

    def rule(self):
        if self._rule is None:
            self._rule = Levels(self.coords, self.levels)
        return self._rule


def _shuffled(c, rng):
    return c[rng.permutation(len(c))]


def _not_sorted(c):
    r = _rows(c)
    return r != sorted(r)


def _first_occurrence_differs(c, ts=1):
    a = strided_level(c, ts)
    b = strided_level(c, ts, 'sorted')
    return not np.array_equal(a[0], b[0])


def _occ_bytes(c):
    b, x, y, z = (int(v) + 1 for v in np.asarray(c).max(0))
    return ((b * x * y * z + 63) // 64 + 1) * 8


def _straddles(c, ksize):
    """A probed line of ksize bits starts so late in a 64-bit word that it runs into the next one."""
    B, X, Y, Z = (int(v) + 1 for v in np.asarray(c).max(0))
    h = ksize // 2
    for (b, x, y, z) in _rows(c):
        for dz in range(-h, h + 1):
            for dy in range(-h, h + 1):
                if 0 <= y + dy < Y and 0 <= z + dz < Z:
                    b0 = ((b * Z + z + dz) * Y + y + dy) * X + x - h
                    if b0 >= 0 and (b0 & 63) + ksize > 64:
                        return True
    return False


def case_top_of_range():
    rng = np.random.default_rng(11)
    c = np.concatenate([rng.integers(0, 3, (4200, 1)), rng.integers(COORD_MAX - 40, COORD_MAX + 1, (4200, 3))], 1)
    c = np.unique(c, axis=0)[:3000]
    # hand-built aliasing rows: the carry of an unguarded pack is an OR into the next field, whose value is therefore even
    alias = [(0, 65534, 6, 6), (1, 0, 6, 6),            # x = 65536 carries into the batch field: (1, 0, 6, 6)
             (0, 6, 65534, 6), (0, 7, 0, 6),            # y = 65536 carries into x: (0, 7, 0, 6)
             (0, 6, 6, 65534), (0, 6, 7, 0),            # z = 65536 carries into y: (0, 6, 7, 0)
             (2, 65534, 65534, 65534)]
    c = np.unique(np.concatenate([c, np.array(alias)]), axis=0)
    c = _shuffled(c, rng)
    lv = Levels(c, 8)
    pred = {'rows lie within 40 of 65534 on every axis, three batches': len(c) > 2900 and set(c[:, 0]) == {0, 1, 2},
            'rows are not in sorted order': _not_sorted(c),
            'coarse rows in first-occurrence order differ from sorted order': _first_occurrence_differs(c)}
    for ks in (5, 7):
        pred['level 0, k = %d: an unguarded 16-bit pack hits an existing row on each of the three axes' % ks] = \
            all(h > 0 for h in alias_hits(lv.coords[0], ks, 1))
    for l in range(1, 8):
        # (from level 1 on every present coordinate is even, so a carry into bit 0 of the x or y field names no present row:
        # only x = 65536, whose carry lands in the batch field, can alias there)
        pred['level %d, k = 3: an unguarded 16-bit pack hits an existing row (x carries into the batch field)' % l] = \
            alias_hits(lv.coords[l], 3, 1 << l)[0] > 0
    case = Case('top_of_range', c, 8, (5, 7), predicates=pred)
    case._rule = lv
    return case


ORIGIN_WIDTHS = (1, 2, 63, 64, 65, 127, 129)


def case_origin(X):
    """Dense block at the origin of batch 0, random occupancy elsewhere, batches {0, 5}, last voxel of the last batch present."""
    rng = np.random.default_rng(100 + X)
    Y, Z = (7, 5) if X <= 2 else (4, 3)
    g = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing='ij'), -1).reshape(-1, 3)
    rows = []
    for b in (0, 5):
        keep = rng.random(len(g)) < 0.6
        if b == 0:
            keep |= (g[:, 0] < 4) & (g[:, 1] < 3) & (g[:, 2] < 3)
        else:
            keep |= (g == [X - 1, Y - 1, Z - 1]).all(1)
        rows.append(np.concatenate([np.full((int(keep.sum()), 1), b), g[keep]], 1))
    c = _shuffled(np.concatenate(rows), rng)
    first = first_rows(c)
    pred = {'grid width X = %d' % X: int(c[:, 1].max()) + 1 == X,
            'batch ids {0, 5}: ids with gaps': set(c[:, 0]) == {0, 5},
            'the last voxel of the last batch is present (the spare word is read)': (5, X - 1, Y - 1, Z - 1) in first,
            'the bitmap fits OCC_MAX_BYTES': _occ_bytes(c) <= OCC_MAX_BYTES}
    for ks in (3, 5, 7):
        h = ks // 2
        pred['k = %d: a row has x < h at y = z = 0, b = 0 (the line starts left of bit 0)' % ks] = \
            any(b == 0 and y == 0 and z == 0 and x < h for (b, x, y, z) in first)
        pred['k = %d: a probed line straddles a 64-bit word' % ks] = _straddles(c, ks)
    pred['unmasked bitmap positions give a neighbour from the adjacent line'] = \
        not np.array_equal(kernel_map(c, 3, 1), kernel_map(c, 3, 1, 'bitmap_nomask'))
    return Case('origin_X%d' % X, c, 2, (3, 5, 7), predicates=pred)


def case_wide_thin():
    rng = np.random.default_rng(7)
    c = np.concatenate([np.zeros((2500, 1), np.int64), rng.integers(0, COORD_MAX + 1, (2500, 1)), rng.integers(0, 8, (2500, 1)),
                        rng.integers(0, 6, (2500, 1))], 1)
    c[:600, 1] = COORD_MAX - rng.integers(0, 12, 600)             # a populated right edge, a populated left edge
    c[600:1200, 1] = rng.integers(0, 12, 600)
    c = np.concatenate([c, [[0, COORD_MAX, 7, 5], [0, 0, 0, 0]]])
    c = _shuffled(np.unique(c, axis=0), rng)
    X, Y, Z = (int(v) + 1 for v in c[:, 1:].max(0))
    pred = {'X = 65535, Y, Z <= 8': X == 65535 and Y <= 8 and Z <= 8,
            'the bitmap fits OCC_MAX_BYTES': _occ_bytes(c) <= OCC_MAX_BYTES,
            'some row has a k = 5 neighbour': int((kernel_map(c, 5, 1) >= 0).sum()) > len(c)}
    return Case('wide_thin', c, 3, (5,), predicates=pred)


COUNT_SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097)


def case_count(n):
    rng = np.random.default_rng(1000 + n)
    side = max(4, int(round((2.5 * max(n, 1)) ** (1 / 3))) + 1)
    c = np.concatenate([rng.integers(0, 2, (8 * n + 8, 1)), rng.integers(0, side, (8 * n + 8, 3))], 1)
    c = np.unique(c, axis=0)
    c = _shuffled(c, rng)[:n]
    pred = {'n = %d rows, no duplicates' % n: len(c) == n and dup_count(c) == 0}
    if n >= 63:
        pred['rows are not in sorted order'] = _not_sorted(c)
        pred['coarse rows in first-occurrence order differ from sorted order'] = _first_occurrence_differs(c)
    if n >= 8 and n & (n - 1) == 0:
        pred['n is a power of two: the hash table (2n slots) is at load 0.5'] = True
    return Case('count_%d' % n, c, 3, (5,) if n <= 1025 else (), predicates=pred)


def case_big():
    rng = np.random.default_rng(5)
    rows = []
    for b in range(2):
        occ = rng.random((140, 140, 140)) < 0.06
        xyz = np.argwhere(occ)
        rows.append(np.concatenate([np.full((len(xyz), 1), b), xyz], 1))
    c = _shuffled(np.concatenate(rows), rng)
    nb = (len(c) + SCAN_ITEMS - 1) // SCAN_ITEMS
    return Case('big', c, 3, (), what='strided',
                predicates={'more than 262 144 rows: the scan of the block sums takes a second trip': len(c) > 262144 and nb > 256,
                            'rows are not in sorted order': _not_sorted(c[:1000])})


def case_strided():
    """Coarse voxels with 1, 2 and all 8 children; the children of one coarse voxel far apart in the row order."""
    rng = np.random.default_rng(3)
    rows = []
    for i in range(40):                                   # 40 coarse voxels of level 1, with 1 + (i % 8) children
        base = np.array([i % 2, 2 * (i * 7 % 23), 2 * (i * 5 % 19), 2 * (i * 3 % 17)])
        kids = rng.permutation(8)[:1 + i % 8]
        for k in kids:
            rows.append(base + [0, k & 1, (k >> 1) & 1, (k >> 2) & 1])
    full = np.array([[1, 100 + (k & 1), 100 + ((k >> 1) & 1), 100 + ((k >> 2) & 1)] for k in range(8)])
    filler = np.concatenate([np.zeros((300, 1), np.int64), rng.integers(200, 230, (300, 3))], 1)
    c = np.unique(np.concatenate([np.array(rows), filler]), axis=0)
    c = _shuffled(c, rng)
    c = np.concatenate([full[:4], c, full[4:]])           # one family split between the first and the last rows
    _, parent, koff = strided_level(c, 1)
    kids = np.bincount(parent)
    span = max(int(np.ptp(np.flatnonzero(parent == p))) for p in np.flatnonzero(kids == 8))
    return Case('strided', c, 4, (3,), predicates={
        'coarse voxels with 1, 2 and 8 children': {1, 2, 8} <= set(kids.tolist()),
        'the children of one coarse voxel lie more than n/2 rows apart': span > len(c) // 2,
        'no duplicates': dup_count(c) == 0})


def case_dups(kind):
    rng = np.random.default_rng(9)
    base = np.unique(np.concatenate([rng.integers(0, 2, (400, 1)), rng.integers(0, 9, (400, 3))], 1), axis=0)
    if kind == 'none':
        c, want = base, 0
    elif kind == 'one':
        c, want = np.concatenate([base, base[17:18]]), 1
    elif kind == 'many':
        c, want = np.concatenate([base, base[::2], base[::3], base[::2]]), len(base[::2]) * 2 + len(base[::3])
    else:
        c, want = np.repeat(base[5:6], 333, 0), 332
    c = _shuffled(c, rng)
    return Case('dups_' + kind, c, 2, (), what='dups',
                predicates={'the rule counts %d duplicate rows' % want: dup_count(c) == want})


@functools.lru_cache(maxsize=None)
def coord_case(name):
    kind, _, arg = name.partition(':')
    if kind == 'top_of_range':
        return case_top_of_range()
    if kind == 'origin':
        return case_origin(int(arg))
    if kind == 'wide_thin':
        return case_wide_thin()
    if kind == 'count':
        return case_count(int(arg))
    if kind == 'big':
        return case_big()
    if kind == 'strided':
        return case_strided()
    if kind == 'dups':
        return case_dups(arg)
    raise KeyError(name)


COORD_CASES = (['top_of_range'] + ['origin:%d' % X for X in ORIGIN_WIDTHS] + ['wide_thin'] +
               ['count:%d' % n for n in COUNT_SIZES] + ['strided'] + ['dups:%s' % k for k in ('none', 'one', 'many', 'all')] +
               ['big'])
# (the cases a CPU test can afford to run every mistake over)
SMALL_COORD_CASES = [c for c in COORD_CASES if c not in ('big', 'wide_thin') and not c.startswith('dups')]


# -- b2m_rulebook called directly
RULEBOOK_K = (1, 8, 27, 125, 343)
RULEBOOK_N_OUT = (1, 63, 64, 65, 4033)


@functools.lru_cache(maxsize=None)
def rulebook_case(K, n_out):
    """(nbr (K, ld) int32 with ld = n_out + 5 and junk in the spare columns, n_out)."""
    rng = np.random.default_rng(K * 10007 + n_out)
    ld = n_out + 5
    nbr = rng.integers(0, 5 * n_out + 3, (K, ld)).astype(np.int32)
    nbr[rng.random((K, ld)) < 0.55] = -1
    if K > 2:
        nbr[1, :n_out] = -1                                  # an offset without pairs, a full one
        nbr[2, :n_out] = np.arange(n_out)
    nbr[:, n_out:] = 7                                       # spare columns of the wider leading dimension: never part of the map
    return nbr, n_out


# -- b2m_rulebook_balance called directly on synthetic counts
BALANCE_NTILES = (63, 64, 65, 1023, 1024, 1025, 2049, 8191)
BALANCE_K = (1, 8, 27, 125)
BALANCE_PATTERNS = ('zero', 'uniform', 'random', 'heavy_start', 'heavy_middle', 'heavy_end', 'first_eighth', 'last_eighth')


@functools.lru_cache(maxsize=None)
def balance_case(nt, K, pattern):
    """(cnt (K, nt) int32 with counts in 0..64, info of the rule's runs).  Predicates asserted here."""
    rng = np.random.default_rng(nt * 131 + K * 7 + BALANCE_PATTERNS.index(pattern))
    cnt = np.zeros((K, nt), np.int32)
    e = max(nt // 8, 1)
    if pattern == 'uniform':
        cnt[:] = 17
    elif pattern == 'random':
        cnt[:] = rng.integers(0, 65, (K, nt))
        cnt[rng.random((K, nt)) < 0.3] = 0
    elif pattern.startswith('heavy'):
        cnt[:] = rng.integers(0, 2, (K, nt))
        cnt[:, {'heavy_start': 0, 'heavy_middle': nt // 2, 'heavy_end': nt - 1}[pattern]] = 64
    elif pattern == 'first_eighth':
        cnt[:, :e] = rng.integers(1, 65, (K, e))
    elif pattern == 'last_eighth':
        cnt[:, nt - e:] = rng.integers(1, 65, (K, e))
    assert cnt.min() >= 0 and cnt.max() <= 64
    info = {}
    balance_tail(cnt, info)
    if pattern == 'zero':
        assert info['total'] == 0, 'the all-zero pattern must reach the equal-runs branch'
    if pattern in ('first_eighth', 'last_eighth') and nt >= 64:
        assert info['at_cap'], 'all work in one eighth must put a run at the cap (%d tiles, K = %d)' % (nt, K)
    if pattern == 'first_eighth' and nt >= 64:
        assert info['backward_clamp'], 'all work in the first eighth must need the backward clamp'
    if pattern == 'last_eighth' and nt >= 64:
        assert info['forward_clamp'], 'all work in the last eighth must need the forward clamp'
    return cnt, info


# -- keys
@functools.lru_cache(maxsize=None)
def key_case():
    """Rows with coordinates and batch indices over the whole documented range, batch >= 32768 included, shuffled."""
    rng = np.random.default_rng(21)
    c = np.concatenate([rng.integers(0, COORD_MAX + 1, (3000, 4)),
                        np.concatenate([rng.integers(32760, 32776, (600, 1)), rng.integers(0, 40, (600, 3))], 1),
                        [[COORD_MAX] * 4, [0] * 4, [32767, COORD_MAX, 0, 1], [32768, 0, COORD_MAX, 1], [COORD_MAX, 1, 2, 3]]])
    c = _shuffled(np.unique(c, axis=0), rng).astype(np.int32)
    assert (c[:, 0] >= 32768).any() and (c[:, 0] < 32768).any() and c.max() == COORD_MAX and c.min() == 0
    assert (c[:, 1:] >= 1024).any(), 'keys above 10 bits'
    for keys in (morton_keys(c), hilbert_keys(c, 16)):
        assert (keys.view(np.int64) < 0).any(), 'batch >= 32768: the int64 view of a key is negative'
        assert not np.array_equal(key_order(keys), key_order(keys, 'signed'))
    return c
