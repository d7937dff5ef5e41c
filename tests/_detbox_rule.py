"""Rules and cases for csrc/detbox.hip (b2m_mask_hulls, b2m_obb_corners, b2m_hull_box_iou, b2m_aabb_iou): plain numpy / Python,
no torch, no device.

Hulls: Andrew's chain with the fp64 turn, `(p - o) x (q - o) <= 0` pops, on np.unique points; counter-clockwise from the
lexicographic minimum.  `filter_rule` restates the kernel's candidate filter (its constants copied as literals) for the candidate
counts and flags.  Corners and the axis-aligned IoU: the kernel's written operation order in Python floats -- bit-exact.  Hull x box
IoU: polygon_clip + shoelace + box3d_iou (utils/box_util.py:19-66, 101-140) in two forms evaluated side by side by `iou_forms`:
(a) fp64 as the reference evaluates it, with a running bound of its rounding error, and (b) exact in fractions.Fraction, taking the
inside / outside decisions from (a)."""
import math
from fractions import Fraction

import numpy as np

HULL_MAX, HULL_CHUNKS, LCAP, PCAP, NDIR = 512, 32, 2048, 516, 16           # include/b2m.h, csrc/detbox.hip
FLAG_VERTICES, FLAG_CANDIDATES = 1, 2
OBB_REC = 16
FILTER_MARGIN = 8.9e-16
IOU_TOL = 1e-9
MARGIN_MIN = 1e-9
DIRS = np.array([[1.0, 0.0], [0.92387953251128674, 0.38268343236508977], [0.70710678118654752, 0.70710678118654752],
                 [0.38268343236508977, 0.92387953251128674], [0.0, 1.0], [-0.38268343236508977, 0.92387953251128674],
                 [-0.70710678118654752, 0.70710678118654752], [-0.92387953251128674, 0.38268343236508977], [-1.0, 0.0],
                 [-0.92387953251128674, -0.38268343236508977], [-0.70710678118654752, -0.70710678118654752],
                 [-0.38268343236508977, -0.92387953251128674], [0.0, -1.0], [0.38268343236508977, -0.92387953251128674],
                 [0.70710678118654752, -0.70710678118654752], [0.92387953251128674, -0.38268343236508977]])


# ------------------------------------------------------------------ hulls
HULL_VARIANTS = ('lt', 'nodedup', 'cw')


def np_hull(p2, variant=None):
    """Vertices of the convex hull of (m, 2) points: counter-clockwise from the lexicographic minimum, no repeated and no
    collinear-interior vertex; fewer than 3 distinct points, or all collinear: the 1 or 2 extreme points."""
    p2 = np.asarray(p2, np.float64).reshape(-1, 2)
    p = p2[np.lexsort((p2[:, 1], p2[:, 0]))] if variant == 'nodedup' else np.unique(p2, axis=0)
    if len(p) < 3:
        return p

    def chain(pts):
        out = []
        for q in pts.tolist():                       # (python floats: the same IEEE doubles, much faster than numpy scalars)
            while len(out) >= 2:
                t = (out[-1][0] - out[-2][0]) * (q[1] - out[-2][1]) - (out[-1][1] - out[-2][1]) * (q[0] - out[-2][0])
                if not ((t < 0.0) if variant == 'lt' else (t <= 0.0)):
                    break
                out.pop()
            out.append(q)
        return out
    lower, upper = chain(p), chain(p[::-1])
    v = np.array(lower[:-1] + upper[:-1])
    if variant == 'cw' and len(v) > 2:
        v = np.concatenate([v[:1], v[:0:-1]])
    return v


def np_area(v):
    if len(v) < 3:
        return 0.0
    x, y = v[:, 0] - v[0, 0], v[:, 1] - v[0, 1]
    return 0.5 * abs(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1)))


def filter_rule(p2):
    """Number of hull candidates the kernel keeps of the (m, 2) points (in index order): the extreme point along 16 directions (the
    first of equals), consecutive equal extremes merged; fewer than 3: every point is kept; else a point is dropped when it is to
    the left of every edge by more than 8.9e-16 (|l| + |q|)."""
    p2 = np.asarray(p2, np.float64).reshape(-1, 2)
    if len(p2) == 0:
        return 0
    x, y = p2[:, 0], p2[:, 1]
    ext = []
    for d in range(NDIR):
        i = int(np.argmax(x * DIRS[d, 0] + y * DIRS[d, 1]))
        q = (x[i], y[i])
        if not ext or ext[-1] != q:
            ext.append(q)
    if len(ext) > 1 and ext[-1] == ext[0]:
        ext.pop()
    if len(ext) < 3:
        return len(p2)
    inside = np.ones(len(p2), bool)
    for (ax, ay), (bx, by) in zip(ext, ext[1:] + ext[:1]):
        l, q = (bx - ax) * (y - ay), (by - ay) * (x - ax)
        inside &= (l - q) > FILTER_MARGIN * (np.abs(l) + np.abs(q))
    return int((~inside).sum())


def hulls_rule(masks, pos, cap):
    """What b2m_mask_hulls reports for bool rows over pos (n, 3): count, box6, ncand, n_hull, flags, hulls (list; None = not written)."""
    masks = np.asarray(masks, bool)
    k = len(masks)
    out = {'count': np.zeros(k, np.int32), 'box6': np.zeros((k, 6)), 'ncand': np.zeros(k, np.int32), 'n_hull': np.zeros(k, np.int32),
           'flags': np.zeros(k, np.int32), 'hulls': []}
    for r in range(k):
        p = pos[masks[r]]
        out['count'][r] = len(p)
        out['box6'][r] = np.concatenate([p.min(0), p.max(0)]) if len(p) else [np.inf] * 3 + [-np.inf] * 3
        out['ncand'][r] = filter_rule(p[:, :2])
        if out['ncand'][r] > cap:
            out['flags'][r] = FLAG_CANDIDATES
            out['hulls'].append(None)
            continue
        h = np_hull(p[:, :2])
        out['n_hull'][r] = len(h)
        if len(h) > HULL_MAX:
            out['flags'][r] = FLAG_VERTICES
            h = None
        out['hulls'].append(h)
    return out


def chunking(words):
    """(wpb, nchunk) of b2m_mask_hulls."""
    wpb = max(-(-(-(-words // HULL_CHUNKS)) // 64) * 64, 1024)
    return wpb, (1 if words == 0 else -(-words // wpb))


# ------------------------------------------------------------------ ground-truth corners, axis-aligned IoU (bit-exact restatements)
SX = (-1, 1, 1, -1, -1, 1, 1, -1)
SY = (-1, -1, 1, 1, -1, -1, 1, 1)
SZ = (-1, -1, -1, -1, 1, 1, 1, 1)


def corners_rule(centers, bounds, rot):
    centers, bounds, rot = (np.asarray(a, np.float64) for a in (centers, bounds, rot))
    g = len(centers)
    out = np.zeros((g, OBB_REC))
    for i in range(g):
        b = bounds[i].tolist(); q = rot[i].reshape(9).tolist(); ce = centers[i].tolist()
        ext = [0.0, 0.0, 0.0]
        c = []
        for v in range(8):
            p = (SX[v] * b[0], SY[v] * b[1], SZ[v] * b[2])
            cv = []
            for a in range(3):
                rv = q[a] * p[0] + q[3 + a] * p[1] + q[6 + a] * p[2]
                ext[a] = rv if rv > ext[a] else ext[a]
                cv.append(rv + ce[a])
            c.append(cv)

        def dist(u, v):
            dx, dy, dz = c[u][0] - c[v][0], c[u][1] - c[v][1], c[u][2] - c[v][2]
            return math.sqrt(dx * dx + dy * dy + dz * dz)
        for v in range(4):
            out[i, 2 * v], out[i, 2 * v + 1] = c[v][0], c[v][1]
        out[i, 8], out[i, 9] = c[0][2], c[7][2]
        out[i, 10] = dist(0, 1) * dist(1, 2) * dist(0, 4)
        out[i, 11:14] = [ext[0] * 2.0, ext[1] * 2.0, ext[2] * 2.0]
    return out


def aabb_rule(box6, pcls, gcenters, boxes, gcls, variant=None):
    k, g = len(box6), len(gcenters)
    out = np.zeros((k, g))
    for r in range(k):
        for b in range(g):
            if not (pcls[r] >= 0 and pcls[r] == gcls[b]):
                continue
            ok, inter, va, vb = True, 1.0, 1.0, 1.0
            for a in range(3):
                lo, hi = float(box6[r, a]), float(box6[r, 3 + a])
                ca, sa = (lo + hi) / 2.0, hi - lo
                cb, sb = float(gcenters[b, a]), float(boxes[b, 11 + a])
                mn, mx = min(ca + sa / 2, cb + sb / 2), max(ca - sa / 2, cb - sb / 2)
                ok = ok and ((mn >= mx) if variant == 'ge' else (mn > mx))
                inter *= mn - mx
                va *= sa; vb *= sb
            if ok:
                den = va + vb - inter
                out[r, b] = 1.0 * inter / den if den else math.nan * inter       # (0 / 0: what the division gives)
    return out


# ------------------------------------------------------------------ hull x box IoU, forms (a) and (b)
U = 2.0 ** -53


def _up(e):
    return e * (1.0 + 2.0 ** -40)                    # the bound's own arithmetic rounds: keep it an upper bound


class B:
    """An fp64 value as the kernel's written expression gives it, and a bound on its distance from the exact value."""
    __slots__ = ('v', 'e')

    def __init__(self, v, e=0.0):
        self.v, self.e = v, e

    def __add__(self, o):
        v = self.v + o.v
        return B(v, _up(self.e + o.e + U * abs(v)))

    def __sub__(self, o):
        v = self.v - o.v
        return B(v, _up(self.e + o.e + U * abs(v)))

    def __mul__(self, o):
        v = self.v * o.v
        return B(v, _up(abs(self.v) * o.e + abs(o.v) * self.e + self.e * o.e + U * abs(v)))

    def inv(self):
        v = 1.0 / self.v
        if not abs(self.v) > 2 * self.e:
            return B(v, math.inf)
        return B(v, _up(self.e / (abs(self.v) * (abs(self.v) - self.e)) + U * abs(v)))

    def div(self, o):
        v = self.v / o.v
        if not abs(o.v) > 2 * o.e:
            return B(v, math.inf)
        return B(v, _up((self.e + abs(v) * o.e) / (abs(o.v) - o.e) + U * abs(v)))


def _dyadic_sum_is_exact(terms):
    """Every partial sum of the Fractions, in any order, is an fp64 number: all are multiples of 2^-q and sum |t| * 2^q < 2^53."""
    q = 0
    for t in terms:
        d = t.denominator
        if d & (d - 1):
            return False
        q = max(q, d.bit_length() - 1)
    return sum(abs(t) for t in terms) * (1 << q) < (1 << 53)


def _shoelace(fa, fb):
    """Twice the signed area relative to the first vertex: (B value with a bound that holds for ANY summation order, Fraction,
    every-order-exact flag)."""
    n = len(fa)
    ox, oy = fa[0]
    ex, ey = fb[0]
    terms, exact_terms = [], []
    for i in range(n):
        j = i + 1 if i + 1 < n else 0
        terms.append((fa[i][0] - ox) * (fa[j][1] - oy) - (fa[j][0] - ox) * (fa[i][1] - oy))
        exact_terms.append((fb[i][0] - ex) * (fb[j][1] - ey) - (fb[j][0] - ex) * (fb[i][1] - ey))
    s = 0.0
    for t in terms:
        s += t.v
    gamma = n * U / (1.0 - n * U)
    e = _up(sum(t.e for t in terms) + gamma * sum(abs(t.v) + t.e for t in terms))
    exact = all(Fraction(t.v) == x for t, x in zip(terms, exact_terms)) and _dyadic_sum_is_exact(exact_terms)
    return B(s, e), sum(exact_terms, Fraction(0)), exact


CLIP_VARIANTS = ('ge', 'vertex_first', 'abs_orient')


def iou_forms(hull, zlo, zhi, rect, z0, z7, vol2, variant=None):
    """box3d_iou of the prism (hull (n, 2), zlo ... zhi) and the box (rect (4, 2) corners 0..3, z0 ... z7, volume vol2).
    Returns a dict: iou_a (form (a), fp64), iou_exact (form (b), Fraction), bound (|any fp64 evaluation - exact|), margin (the
    smallest relative margin |L - R| / (|L| + |R|) of the inside tests that fp64 does not evaluate exactly), agree (the fp64
    decisions equal the exact ones), exact (form (a) equals form (b) at every step before the final division, in any summation
    order), emptied_at (clip edge after which nothing was left, or None), crossings, max_n (largest intermediate polygon),
    inter_exact / area1_exact (Fractions)."""
    hull = np.asarray(hull, np.float64).reshape(-1, 2)
    rect = np.asarray(rect, np.float64).reshape(4, 2)
    out = {'iou_a': 0.0, 'iou_exact': Fraction(0), 'bound': 0.0, 'margin': math.inf, 'agree': True, 'exact': True,
           'emptied_at': None, 'crossings': 0, 'max_n': len(hull), 'inter_exact': Fraction(0), 'area1_exact': Fraction(0)}
    if len(hull) < 3:
        return out
    rc = [tuple(map(float, c)) for c in rect]
    if variant == 'abs_orient':
        if (rc[1][0] - rc[0][0]) * (rc[2][1] - rc[0][1]) - (rc[2][0] - rc[0][0]) * (rc[1][1] - rc[0][1]) < 0:
            rc = rc[::-1]
    fa = [(B(float(x)), B(float(y))) for x, y in hull]
    fb = [(Fraction(float(x)), Fraction(float(y))) for x, y in hull]
    a1, a1x, ex1 = _shoelace(fa, fb)
    out['area1_exact'] = abs(a1x) / 2
    exact = ex1
    for e in range(4):
        c1, c2 = rc[e - 1], rc[e]
        C1, C2 = (Fraction(c1[0]), Fraction(c1[1])), (Fraction(c2[0]), Fraction(c2[1]))
        dec = []
        for (px, py), (qx, qy) in zip(fa, fb):
            lf, rf = (c2[0] - c1[0]) * (py.v - c1[1]), (c2[1] - c1[1]) * (px.v - c1[0])
            L, R = (C2[0] - C1[0]) * (qy - C1[1]), (C2[1] - C1[1]) * (qx - C1[0])
            dec.append((lf >= rf) if variant == 'ge' else (lf > rf))
            if Fraction(lf) == L and Fraction(rf) == R:
                continue                             # fp64 evaluates this test exactly: the decision is the exact one
            exact = False
            out['margin'] = min(out['margin'], float(abs(L - R) / (abs(L) + abs(R))) if (L or R) else 0.0)
            out['agree'] = out['agree'] and dec[-1] == (L > R)
        na, nb = [], []
        n = len(fa)
        for i in range(n):
            s = i - 1
            if dec[i] != dec[s]:
                out['crossings'] += 1
                (sx, sy), (ex, ey) = fa[s], fa[i]
                c1x, c1y, c2x, c2y = B(c1[0]), B(c1[1]), B(c2[0]), B(c2[1])
                dcx, dcy, dpx, dpy = c1x - c2x, c1y - c2y, sx - ex, sy - ey
                n1, n2 = c1x * c2y - c1y * c2x, sx * ey - sy * ex
                den = dcx * dpy - dcy * dpx
                if den.v == 0.0:
                    out['bound'] = math.inf
                    return out
                n3 = den.inv()
                cross_a = ((n1 * dpx - n2 * dcx) * n3, (n1 * dpy - n2 * dcy) * n3)
                (SX_, SY_), (EX, EY) = fb[s], fb[i]
                DCX, DCY, DPX, DPY = C1[0] - C2[0], C1[1] - C2[1], SX_ - EX, SY_ - EY
                N1, N2 = C1[0] * C2[1] - C1[1] * C2[0], SX_ * EY - SY_ * EX
                DEN = DCX * DPY - DCY * DPX
                if DEN == 0:
                    out['bound'] = math.inf
                    return out
                cross_b = ((N1 * DPX - N2 * DCX) / DEN, (N1 * DPY - N2 * DCY) / DEN)
                exact = exact and Fraction(cross_a[0].v) == cross_b[0] and Fraction(cross_a[1].v) == cross_b[1]
            if dec[i]:
                if not dec[s]:
                    if variant == 'vertex_first':
                        na += [fa[i], cross_a]; nb += [fb[i], cross_b]
                        continue
                    na.append(cross_a); nb.append(cross_b)
                na.append(fa[i]); nb.append(fb[i])
            elif dec[s]:
                na.append(cross_a); nb.append(cross_b)
        fa, fb = na, nb
        out['max_n'] = max(out['max_n'], len(fa))
        if not fa:
            out['emptied_at'] = e
            break
    out['exact'] = exact
    if len(fa) < 3:
        return out
    s2, s2x, ex2 = _shoelace(fa, fb)
    inter = B(0.5 * abs(s2.v), s2.e * 0.5)
    area1 = B(0.5 * abs(a1.v), a1.e * 0.5)
    zmax, zmin = min(zhi, z7), max(zlo, z0)
    h = B(zmax) - B(zmin)
    h = B(max(0.0, h.v), h.e)
    inter_vol = inter * h
    vol1 = area1 * (B(zhi) - B(zlo))
    den = vol1 + B(vol2) - inter_vol
    iou = inter_vol.div(den)
    H = max(Fraction(0), Fraction(zmax) - Fraction(zmin))
    IV = abs(s2x) / 2 * H
    V1 = abs(a1x) / 2 * (Fraction(zhi) - Fraction(zlo))
    DEN = V1 + Fraction(vol2) - IV
    out['inter_exact'] = abs(s2x) / 2
    out['iou_a'], out['bound'] = iou.v, iou.e
    out['iou_exact'] = IV / DEN if DEN else Fraction(0)
    out['exact'] = exact and ex2 and Fraction(inter_vol.v) == IV and Fraction(den.v) == DEN
    return out


def case_is_valid(f):
    """The condition under which a hull x box case may be put to the device."""
    return f['agree'] and math.isfinite(f['bound']) and f['bound'] <= IOU_TOL and (f['exact'] or f['margin'] >= MARGIN_MIN)


# ---- IoU cases
IOU_SIZES = (3, 4, 63, 64, 65, 127, 128, 129, 512)
Z_HULL, Z_BOX = (0.5, 2.0), (1.0, 3.0)


def hull_par(n):
    """n points of a parabola on a dyadic grid: in convex position exactly, counter-clockwise from the lexicographic minimum."""
    i = np.arange(n, dtype=np.float64)
    return np.stack([i / 4.0, i * i / 256.0], 1)


def hull_cir(n):
    a = 2 * np.pi * (np.arange(n) + 0.37) / n
    v = np.stack([7.3 + 3.7 * np.cos(a), -2.1 + 3.7 * np.sin(a)], 1)
    first = np.lexsort((v[:, 1], v[:, 0]))[0]
    return np.roll(v, -first, axis=0)


def _rect(x0, x1, y0, y1, phi=0.0, about=(0.0, 0.0)):
    c = np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float64)
    if phi:
        r = np.array([[math.cos(phi), -math.sin(phi)], [math.sin(phi), math.cos(phi)]])
        c = (c - about) @ r.T + about
    return c


def _vol(rect, z):
    a = math.hypot(*(rect[1] - rect[0])); b = math.hypot(*(rect[2] - rect[1]))
    return a * b * (z[1] - z[0])


def iou_cases():
    """[(name, kind, hull, zlo, zhi, rect, z0, z7, vol2)]: every hull size against rectangles of every kind."""
    out = []
    for fam, make, phi in (('par', hull_par, 0.0), ('cir', hull_cir, 0.4)):
        for n in IOU_SIZES:
            h = make(n)
            cen = h.mean(0)
            local = h if not phi else (h - cen) @ np.array([[math.cos(phi), -math.sin(phi)], [math.sin(phi), math.cos(phi)]]) + cen
            x0, y0 = local.min(0); x1, y1 = local.max(0)
            w, t = x1 - x0, y1 - y0
            # the largest dyadic square round the mean of the vertices that stays inside: a quarter of its distance to the edges
            e1 = np.roll(h, -1, 0) - h
            dist = np.abs(e1[:, 0] * (cen[1] - h[:, 1]) - e1[:, 1] * (cen[0] - h[:, 0])) / np.hypot(e1[:, 0], e1[:, 1])
            r = 2.0 ** math.floor(math.log2(dist.min() / 4))
            cq = np.round(cen / r) * r
            kinds = {'contain': _rect(x0 - 1, x1 + 1, y0 - 1, y1 + 1, phi, cen),
                     'contained': _rect(cq[0] - r, cq[0] + r, cq[1] - r, cq[1] + r, phi, cq),
                     'cut': _rect((x0 + x1) / 2, x1 + 1, y0 - 1, y1 + 1, phi, cen),
                     'miss_first': _rect(x1 + 1, x1 + 3, y0 - 1, y1 + 1, phi, cen),
                     'miss_last': _rect(x0 - 1, x1 + 1, y0 - 3, y0 - 1, phi, cen)}
            kinds['clockwise'] = kinds['cut'][::-1].copy()
            if fam == 'cir':
                kinds['cut_corner'] = _rect(x0 - 1, (x0 + x1) / 2, (y0 + y1) / 2, y1 + 1, phi, cen)
            if fam == 'par':
                # an edge of the rectangle ON the line of the hull's closing edge (dyadic corners: those tests are exact in fp64)
                o, a = h[0], h[-1]
                nrm = np.array([-(a - o)[1], (a - o)[0]])
                nrm = nrm * 2.0 ** -math.floor(math.log2(np.hypot(*nrm)))
                kinds['line_outside'] = np.array([o, a, a + nrm, o + nrm])
                kinds['line_inside'] = np.array([a, o, o - nrm, a - nrm])
            if n == 512:
                kinds.pop('line_inside', None)             # rejected by case_is_valid: a test fp64 does not evaluate exactly has margin 0
            for kind, rect in kinds.items():
                out.append(('%s%d:%s' % (fam, n, kind), kind, h, Z_HULL[0], Z_HULL[1], rect, Z_BOX[0], Z_BOX[1], _vol(rect, Z_BOX)))
    sq = np.array([[0.0, 0.0], [4.0, 0.0], [4.0, 4.0], [0.0, 4.0]])
    r = _rect(2.0, 6.0, 1.0, 3.0)
    out.append(('sq:cut', 'exact_cut', sq, 0.5, 2.0, r, 1.0, 3.0, _vol(r, (1.0, 3.0))))
    out.append(('sq:touch', 'touch', sq, 0.5, 2.0, _rect(4.0, 8.0, 0.0, 4.0), 1.0, 3.0, 32.0))
    out.append(('sq:z_disjoint', 'z_disjoint', sq, 0.5, 2.0, r, 2.5, 3.0, _vol(r, (2.5, 3.0))))
    out.append(('sq:z_touch', 'z_disjoint', sq, 0.5, 2.0, r, 2.0, 3.0, _vol(r, (2.0, 3.0))))
    out.append(('sq:flat', 'flat', sq, 1.5, 1.5, r, 1.0, 3.0, _vol(r, (1.0, 3.0))))
    out.append(('sq:identical', 'identical', sq, 1.0, 3.0, sq.copy(), 1.0, 3.0, 32.0))
    for m in (0, 1, 2):
        out.append(('short:%d' % m, 'short', sq[:m], 0.5, 2.0, r, 1.0, 3.0, _vol(r, (1.0, 3.0))))
    return out


def iou_case_forms(case, variant=None):
    _, _, h, zlo, zhi, rect, z0, z7, vol2 = case
    return iou_forms(h, zlo, zhi, rect, z0, z7, vol2, variant)


# ---- hull cases: name -> {'pos' (n, 3), 'masks' (k, n) bool, 'cap', 'pad' (set the pad bits above n)}
def _rows_to_case(rows, n_mod, cap=64, pad=True):
    """Each row's points laid end to end; unused points appended until n % 64 == n_mod."""
    total = sum(len(r) for r in rows)
    n = total + (n_mod - total) % 64
    pos = np.zeros((n, 3))
    pos[total:] = [100.0, 100.0, 100.0]
    masks = np.zeros((len(rows), n), bool)
    at = 0
    for i, r in enumerate(rows):
        r = np.asarray(r, np.float64).reshape(-1, 2)
        pos[at:at + len(r), :2] = r
        pos[at:at + len(r), 2] = np.arange(len(r)) * 0.25 - 1.0
        masks[i, at:at + len(r)] = True
        at += len(r)
    return {'pos': pos, 'masks': masks, 'cap': cap, 'pad': pad}


SMALL_ROWS = {
    'empty': np.zeros((0, 2)),
    'one': [[0.5, -1.5]],
    'two': [[2.0, 1.0], [-1.0, 3.0]],
    'duplicates': [[0.3, 0.7]] * 5,
    'horizontal': [[0.1 * i, 2.0] for i in (3, 0, 7, 5, 1)],
    'vertical': [[-1.0, 0.3 * i] for i in (3, 0, 7, 5, 1)],
    'slope': [[0.1 * i, 0.3 * i] for i in (3, 0, 7, 5, 1, 2, 6, 4)],
    'ccw3': [[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]],
    'cw3': [[0.0, 0.0], [0.0, 1.0], [1.0, 0.0]],
    'dup_vertices': [[0, 0], [2, 0], [2, 2], [0, 2], [1, 1], [0, 0], [2, 0], [2, 2], [0, 2], [0.5, 1.5]],
    'edge_points': [[0, 0], [1, 0], [2, 0], [2, 1], [2, 2], [1, 2], [0, 2], [0, 1], [1, 1], [0.5, 0], [2, 0.25]],
}


def _square_sides(n_side, n_inner, seed=0):
    """The corners of the unit square first (they win every tie of the extremes), n_side dyadic points on its sides, n_inner inside."""
    rng = np.random.default_rng(seed)
    t = rng.permutation(np.arange(1, 1024))[:(n_side + 3) // 4] / 1024.0
    sides = np.concatenate([np.stack([t, 0 * t], 1), np.stack([0 * t + 1, t], 1), np.stack([t, 0 * t + 1], 1), np.stack([0 * t, t], 1)])
    sides = sides[rng.permutation(len(sides))[:n_side]]
    inner = 0.25 + rng.integers(0, 512, (n_inner, 2)) / 1024.0
    rest = np.concatenate([sides, inner])
    return np.concatenate([[[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]], rest[rng.permutation(len(rest))]])


def _single(p2, cap, z=None):
    p2 = np.asarray(p2, np.float64)
    pos = np.concatenate([p2, (np.zeros(len(p2)) if z is None else z)[:, None]], 1)
    return {'pos': pos, 'masks': np.ones((1, len(p2)), bool), 'cap': cap, 'pad': False}


BIG_N = 32 * 1024 * 64 + 65


def hull_cases():
    rng = np.random.default_rng(4)
    out = {}
    rows = list(SMALL_ROWS.values())
    out['small:1'] = _rows_to_case(rows, 1)
    out['small:63'] = _rows_to_case(rows, 63)
    out['k0'] = {'pos': np.zeros((10, 3)), 'masks': np.zeros((0, 10), bool), 'cap': 64, 'pad': False}
    n = 64 * 300
    pos = rng.normal(0, 1, (n, 3))
    m = np.zeros((2, n), bool); m[0, 7 * 64 + 3:7 * 64 + 40] = True; m[0, 250 * 64:250 * 64 + 64] = True; m[1, 64 * 299 + 63] = True
    out['sparse'] = {'pos': pos, 'masks': m, 'cap': 128, 'pad': False}
    for words in (1024, 1025):
        n = words * 64 - (0 if words == 1024 else 63)
        pos = rng.normal(0, 1, (n, 3))
        m = rng.random((2, n)) < 0.03
        m[1, -1] = True
        out['words:%d' % words] = {'pos': pos, 'masks': m, 'cap': 256, 'pad': words == 1025}
    n = 1025 * 64
    pos = np.concatenate([rng.random((n, 2)) * 0.5 + 0.25, rng.random((n, 1))], 1)
    corners = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    pos[5:9, :2] = corners; pos[1024 * 64 + 3:1024 * 64 + 7, :2] = corners[::-1]
    m = np.zeros((1, n), bool); m[0, ::5] = True; m[0, 5:9] = True; m[0, 1024 * 64 + 3:1024 * 64 + 7] = True
    out['tie_chunks'] = {'pos': pos, 'masks': m, 'cap': 64, 'pad': False}
    out['cand:2048'] = _single(_square_sides(2044, 3000, 1), 4096)
    out['cand:2049'] = _single(_square_sides(2045, 3000, 2), 4096)
    out['cap64:64'] = _single(_square_sides(60, 500, 3), 64)
    out['cap64:65'] = _single(_square_sides(61, 500, 4), 64)
    i = np.arange(513.0)
    par = np.stack([i, i * i], 1)
    out['parabola:512'] = _single(par[:512][rng.permutation(512)], 1024)
    out['parabola:513'] = _single(par[rng.permutation(513)], 1024)
    a = 2 * np.pi * np.arange(400) / 400
    ring = np.stack([np.cos(a), np.sin(a)], 1)
    b = rng.random(10000) * 2 * np.pi
    rad = 1.0 - 10.0 ** rng.uniform(-16, -13, 10000)
    near = np.stack([rad * np.cos(b), rad * np.sin(b)], 1)
    pts = np.concatenate([ring, near])
    out['circle'] = _single(pts[rng.permutation(len(pts))], 16384)
    out['offset1e6'] = _single(1e6 + rng.normal(0, 0.5, (3000, 2)), 256)
    a = 2 * np.pi * np.arange(100) / 100
    ring = np.stack([np.cos(a), np.sin(a)], 1)
    j = rng.integers(0, 100, 600)
    t = rng.random(600)[:, None]
    chord = ring[j] * (1 - t) + ring[(j + 1) % 100] * t                    # on a hull edge, up to the rounding of this line
    under = chord[:300] * (1.0 - 10.0 ** rng.uniform(-16, -13, 300))[:, None]
    pts = np.concatenate([ring, chord, under, rng.normal(0, 0.2, (2000, 2))])
    out['near_edges'] = _single(pts[rng.permutation(len(pts))], 4096)
    return out


def big_hull_case():
    """n = 32 * 1024 * 64 + 65 points (50 MB of positions), one row with ~3 200 set bits in each of the 31 chunks of 1088 words."""
    rng = np.random.default_rng(8)
    pos = rng.normal(0, 1, (BIG_N, 3))
    m = np.zeros((1, BIG_N), bool)
    m[0, rng.integers(0, BIG_N, 100000)] = True
    m[0, BIG_N - rng.integers(1, 8000, 3000)] = True                      # (the last chunk has 129 words only)
    m[0, -1] = True
    return {'pos': pos, 'masks': m, 'cap': 256, 'pad': True}


def pipeline_case():
    """A scene for the whole chain: masks whose hulls have 3, 65 and 129 vertices (plus interior points), boxes turned about z and one
    turned about all three axes.  Returns (pos, masks, labels of the predictions, centers, bounds, rotations, labels of the boxes)."""
    rng = np.random.default_rng(9)
    pts, rows = [], []
    for n in (3, 65, 129):
        h = hull_cir(n)
        inner = h.mean(0) + (h[rng.integers(0, n, 200)] - h.mean(0)) * rng.uniform(0.0, 0.9, (200, 1))
        p = np.concatenate([h, inner])
        rows.append(len(p))
        pts.append(np.concatenate([p, rng.uniform(0.5, 2.0, (len(p), 1))], 1))
    pos = np.concatenate(pts)
    masks = np.zeros((3, len(pos)), bool)
    at = 0
    for r, m in enumerate(rows):
        masks[r, at:at + m] = True
        at += m
    rots = rotations()
    centers = np.array([[7.0, -2.0, 1.5], [9.5, -1.0, 1.0], [7.3, -2.1, 1.2], [20.0, 5.0, 1.0]])
    bounds = np.array([[1.5, 1.0, 0.8], [2.0, 2.5, 1.0], [6.0, 6.0, 2.0], [1.0, 1.0, 1.0]])
    rot = np.array([rots['yaw'].reshape(9), rots['identity'].reshape(9), rots['generic'].reshape(9), rots['yaw'].reshape(9)])
    return pos, masks, np.array([5, 5, 5], np.int32), centers, bounds, rot, np.array([5, 5, 5, 5], np.int32)


# ---- corners / aabb cases
def rotations():
    """name -> row-major 3 x 3: identity, the axis permutations, generic, a reflection."""
    out = {'identity': np.eye(3)}
    for name, p in (('perm_yzx', (1, 2, 0)), ('perm_zxy', (2, 0, 1)), ('swap_xy', (1, 0, 2))):
        out[name] = np.eye(3)[list(p)]
    a, b, c = 0.3, -1.1, 2.0
    rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    rx = np.array([[1, 0, 0], [0, math.cos(c), -math.sin(c)], [0, math.sin(c), math.cos(c)]])
    out['yaw'] = rz
    out['generic'] = rz @ ry @ rx
    out['reflection'] = rz @ np.diag([1.0, -1.0, 1.0])
    return out


def corners_case(g, seed=0):
    rng = np.random.default_rng(100 + g + seed)
    rots = list(rotations().values())
    centers = rng.normal(0, 3, (g, 3))
    bounds = rng.uniform(0.1, 2.0, (g, 3))
    rot = np.array([rots[i % len(rots)].reshape(9) for i in range(g)]).reshape(g, 9)
    return centers, bounds, rot


def aabb_edge_case():
    """box6 (k, 6), pcls, gcenters, boxes (g, 16; only 11..13 are read), gcls: touching faces, contained, identical, class mismatch,
    pcls -1, generic overlaps, and a single-point box on a zero-size ground truth (row 5, box 6: touching on every axis with zero
    volumes -- `>=` for `>` would make it 0 / 0)."""
    box6 = np.array([[0, 0, 0, 2, 2, 2], [0, 0, 0, 2, 2, 2], [0.5, 0.5, 0.5, 1.5, 1.5, 1.5], [0.1, 0.2, 0.3, 1.7, 2.9, 1.3],
                     [0, 0, 0, 2, 2, 2], [1, 1, 1, 1, 1, 1]], np.float64)
    pcls = np.array([5, 5, 5, 5, -1, 7], np.int32)
    gc = np.array([[3, 1, 1], [1, 1, 1], [1, 1, 1], [1.3, 0.9, 1.1], [1, 1, 1], [1, 3, 1], [1, 1, 1]], np.float64)
    gs = np.array([[2, 2, 2], [2, 2, 2], [4, 4, 4], [0.7, 1.9, 2.3], [2, 2, 2], [2, 2, 2], [0, 0, 0]], np.float64)
    gcls = np.array([5, 5, 5, 5, 6, 5, 7], np.int32)
    boxes = np.zeros((len(gc), OBB_REC)); boxes[:, 11:14] = gs
    return box6, pcls, gc, boxes, gcls


def aabb_size_case(k, g, seed=0):
    rng = np.random.default_rng(seed + 31 * k + g)
    lo = rng.uniform(0, 2, (k, 3)); box6 = np.concatenate([lo, lo + rng.uniform(0.2, 2, (k, 3))], 1)
    gc = rng.uniform(0, 3, (g, 3)); boxes = np.zeros((g, OBB_REC)); boxes[:, 11:14] = rng.uniform(0.2, 3, (g, 3))
    return box6, rng.integers(-1, 3, k).astype(np.int32), gc, boxes, rng.integers(0, 3, g).astype(np.int32)
