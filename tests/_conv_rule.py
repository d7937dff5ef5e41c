"""The sparse convolution restated in float64 straight from its definition, for tests/test_conv_rule.py (CPU) and
tests/test_gpu_conv_edges.py (the HIP kernels of csrc/conv.hip, conv_fwd_flow.h, conv_1x1.h).

A layer is a neighbour table nbr[K, n_out] (input row of output row o under offset k, -1 = absent) and

    Y[o]   = Y0[o] + bias + sum_k [X1 | X2][nbr[k, o]] W[k]             forward (two sources, bias, accumulate)
    out    = relu(scale * Y + shift + res)                                the inference epilogue
    dX[i] += dY[o] W[k]^T,   dW[k, ci0 + c] += X[i, c]^T dY[o]            over the pairs (i, o) = (nbr[k, o], o) of offset k
    tile sums: per tile of 64 output rows, the column sums of Y and of Y * Y.

TWO OPERAND FAMILIES, two comparisons -- neither takes a tolerance from what a kernel gives:

  exact      x, dy small integers, w small multiples of a power of two g, bias / y0 integers.  Every product and every
             partial sum, in ANY order, is an integer multiple of g; while S = sum|x||w| + |bias| + |y0| <= 2^24 g none
             of them needs more than the 24 bits of an fp32 significand, so an fmaf chain in any order, a split-K combine
             in LDS or with atomics, and an f16 MFMA with fp32 accumulation all give the fp64 result BIT FOR BIT.  The
             comparison is torch.equal; a dropped, duplicated or misrouted term differs by >= g.  `assert_exact` checks
             the condition on S (a condition on the inputs, computed from the reference) in every case.  Half outputs
             must be representable in binary16 as well: |y| <= 2048 g (`assert_half_exact`).
  bound      full-mantissa operands, |x|, |w| log-uniform in [2^-6, 2^6], random signs.  Each output element is held to
                 |y - y64| <= gamma S,   gamma = n u / (1 - n u),  n = T + 16,  u = 2^-24
             T = the products of that element (counted from the table), 16 = the adds of bias, y0 and up to 16 slice
             partials: the standard bound of a once-rounded fma / add chain in any order (Higham, Accuracy and Stability
             of Numerical Algorithms, 2nd ed., Lemma 3.1 / eq. 3.5; an fp32 MFMA is such a chain).  Sharp only for short
             sums, so these cases keep T <= 64.  Half kernels: + 2^-11 |y64| for the one rounding of the result.
             (The float64 reference's own error, ~T 2^-53 S, is eight orders below the bound.)
"""
import numpy as np
import torch

TILE = 64
U32 = 2.0 ** -24
EXTRA_ADDS = 16


# ----------------------------------------------------------------------------- the rule (float64)
def _long(nbr):
    return torch.as_tensor(np.asarray(nbr), dtype=torch.long)


def _cat(x1, x2):
    return x1 if x2 is None else torch.cat([x1, x2], 1)


def conv_fwd(nbr, x1, x2, w, bias=None, y0=None):
    """Y = Y0 + bias + sum_k [X1|X2][nbr[k]] W[k]; nbr None: the 1x1 layer (row o reads row o)."""
    x = _cat(x1, x2).double()
    w3 = (w if w.dim() == 3 else w.unsqueeze(0)).double()
    n_out = x.shape[0] if nbr is None else np.asarray(nbr).shape[1]
    y = torch.zeros(n_out, w3.shape[2], dtype=torch.float64) if y0 is None else y0.double().clone()
    if bias is not None:
        y += bias.double().reshape(1, -1)
    if nbr is None:
        return y + x[:n_out] @ w3[0]
    t = _long(nbr)
    for k in range(t.shape[0]):
        o = torch.nonzero(t[k] >= 0).reshape(-1)
        if o.numel():
            y.index_add_(0, o, x[t[k, o]] @ w3[k])
    return y


def epilogue(y, scale, shift, res=None, relu=False):
    out = y.double() * scale.double().reshape(1, -1) + shift.double().reshape(1, -1)
    if res is not None:
        out = out + res.double()
    return out.clamp_min(0) if relu else out


def conv_dgrad(nbr, dy, w, n_in, c0=0, c=None, dx0=None):
    """dX[i, c0:c0+c] = dX0 + sum over pairs dY[o] W[k, c0:c0+c]^T."""
    w3 = (w if w.dim() == 3 else w.unsqueeze(0)).double()
    c = w3.shape[1] - c0 if c is None else c
    dy = dy.double()
    dx = torch.zeros(n_in, c, dtype=torch.float64) if dx0 is None else dx0.double().clone()
    if nbr is None:
        dx[:dy.shape[0]] += dy @ w3[0, c0:c0 + c].t()
        return dx
    t = _long(nbr)
    for k in range(t.shape[0]):
        o = torch.nonzero(t[k] >= 0).reshape(-1)
        if o.numel():
            dx.index_add_(0, t[k, o], dy[o] @ w3[k, c0:c0 + c].t())
    return dx


def conv_wgrad(nbr, x, dy, dw0, ci0=0):
    """dW0[:, ci0:ci0+cin] += sum over pairs X[i]^T dY[o]  (dW0: (K, cin_total, cout))."""
    dw = dw0.double().clone()
    x = x.double(); dy = dy.double()
    cin = x.shape[1]
    if nbr is None:
        dw[0, ci0:ci0 + cin] += x[:dy.shape[0]].t() @ dy
        return dw
    t = _long(nbr)
    for k in range(t.shape[0]):
        o = torch.nonzero(t[k] >= 0).reshape(-1)
        if o.numel():
            dw[k, ci0:ci0 + cin] += x[t[k, o]].t() @ dy[o]
    return dw


def tile_sums(y, n_out=None):
    """(ntiles, 2, cout): column sums of Y and Y*Y over tiles of 64 rows; rows >= n_out do not exist."""
    y = y.double()
    n = y.shape[0] if n_out is None else n_out
    nt = (n + TILE - 1) // TILE
    p = torch.zeros(nt * TILE, y.shape[1], dtype=torch.float64)
    p[:n] = y[:n]
    p = p.reshape(nt, TILE, -1)
    return torch.stack([p.sum(1), (p * p).sum(1)], 1)


# ----------------------------------------------------------------------------- term counts, S, exactness, the bound
def terms_fwd(nbr, cin, n_out=None):
    """T[o]: products of an output element (a column vector: the same for every channel)."""
    if nbr is None:
        return torch.full((n_out, 1), float(cin), dtype=torch.float64)
    return torch.from_numpy((np.asarray(nbr) >= 0).sum(0).astype(np.float64) * cin).reshape(-1, 1)


def terms_dgrad(nbr, cout, n_in):
    t = np.asarray(nbr)
    return torch.from_numpy(np.bincount(t[t >= 0].ravel(), minlength=n_in).astype(np.float64) * cout).reshape(-1, 1)


def terms_wgrad(nbr):
    """T[k]: the pairs of offset k (one product per pair and element of dW[k])."""
    return torch.from_numpy((np.asarray(nbr) >= 0).sum(1).astype(np.float64)).reshape(-1, 1, 1)


def _abs(t):
    return None if t is None else t.double().abs()


def S_fwd(nbr, x1, x2, w, bias=None, y0=None):
    return conv_fwd(nbr, _abs(x1), _abs(x2), _abs(w), _abs(bias), _abs(y0))


def S_dgrad(nbr, dy, w, n_in, c0=0, c=None, dx0=None):
    return conv_dgrad(nbr, _abs(dy), _abs(w), n_in, c0, c, _abs(dx0))


def S_wgrad(nbr, x, dy, dw0, ci0=0):
    return conv_wgrad(nbr, _abs(x), _abs(dy), _abs(dw0), ci0)


class NotExact(AssertionError):
    pass


def assert_exact(S, ref, g):
    """The sufficient condition for bit-exact fp32 evaluation in any order: every element's S <= 2^24 g, and the reference
    a multiple of g (which it is when the operands are what `exact_operands` draws)."""
    smax = float(S.max()) if S.numel() else 0.0
    if not smax <= 2.0 ** 24 * g:
        raise NotExact('S = %.6g exceeds 2^24 g = %.6g: fp32 need not be exact for these operands' % (smax, 2.0 ** 24 * g))
    q = ref.double() / g
    if not bool((q == q.round()).all()):
        raise NotExact('the reference is not a multiple of g = %g: the operands are not on the grid' % g)


def assert_half_exact(ref, g):
    m = float(ref.abs().max()) if ref.numel() else 0.0
    if not m <= 2048.0 * g:
        raise NotExact('|y| = %.6g exceeds 2048 g = %.6g: not representable in binary16' % (m, 2048.0 * g))


def bound(T, S, extra=EXTRA_ADDS):
    n = T + extra
    return (n * U32) / (1.0 - n * U32) * S


def bound_half(T, S, ref, extra=EXTRA_ADDS):
    """The fp32 bound e, then one rounding of y32 to binary16: |rd(y32) - y64| <= e + 2^-11 |y32| <= e (1 + 2^-11) + 2^-11 |y64|."""
    return bound(T, S, extra) * (1.0 + 2.0 ** -11) + 2.0 ** -11 * ref.double().abs()


def ratio(got, ref, bnd):
    """Largest |got - ref| / bound over the elements with a non-zero bound; elements with bound 0 must be equal."""
    err = (got.double() - ref.double()).abs()
    bnd = bnd.expand_as(err) if bnd.shape != err.shape else bnd
    zero = bnd == 0
    if bool((err[zero] != 0).any()):
        return float('inf')
    nz = ~zero
    return float((err[nz] / bnd[nz]).max()) if bool(nz.any()) else 0.0


# ----------------------------------------------------------------------------- neighbour tables
KINDS = ('dense', 'centre', 'mixed', 'random', 'broadcast', 'last_row')


def _rows(rng, n_out, n_in):
    """One offset's input rows for all outputs: distinct (a sub-permutation) where n_in >= n_out, so that the table has a reverse."""
    if n_in >= n_out:
        return rng.permutation(n_in)[:n_out].astype(np.int32)
    return rng.integers(0, n_in, n_out).astype(np.int32)


def table(kind, K, n_out, n_in=None, seed=0):
    """nbr[K, n_out] int32 of the named kind:
      dense      every offset present for every row: every visit of every tile is full (64 pairs)
      centre     only offset K // 2 present
      mixed      in each tile some offsets full, some partial, some a single pair (shifted from tile to tile), offset 1 empty
                 everywhere and -- from three tiles on -- tile 1 empty altogether: its rows come out as 0, bias or y0
      random     30 % fill
      broadcast  every second offset: all outputs gather input row n_in // 2, every fifth output row n_in - 1
      last_row   a single pair, (n_in - 1) -> the last row of the last tile, under the last offset
    Input rows of one offset are distinct where n_in >= n_out (so that the table has a reverse), except in `broadcast`."""
    n_in = n_out if n_in is None else n_in
    rng = np.random.default_rng([seed, K, n_out, n_in, KINDS.index(kind)])
    full = np.stack([_rows(rng, n_out, n_in) for _ in range(K)])
    nbr = np.full((K, n_out), -1, np.int32)
    nt = (n_out + TILE - 1) // TILE
    if kind == 'dense':                       # every visit of every tile is full
        nbr[:] = full
    elif kind == 'centre':
        nbr[K // 2] = full[K // 2]
    elif kind == 'random':
        keep = rng.random((K, n_out)) < 0.3
        nbr[keep] = full[keep]
    elif kind == 'mixed':
        # per tile: offsets full / partial / a single pair in turn (shifted from tile to tile), offset 1 (or 0) empty
        # everywhere, one tile empty altogether (where there are at least three)
        empty_k = 1 if K > 1 else -1
        empty_t = 1 if nt >= 3 else -1
        for t in range(nt):
            if t == empty_t:
                continue
            r0, r1 = t * TILE, min((t + 1) * TILE, n_out)
            for k in range(K):
                if k == empty_k:
                    continue
                form = (k + t) % 3
                if form == 0:
                    sel = np.arange(r0, r1)
                elif form == 1:
                    sel = r0 + np.flatnonzero(rng.random(r1 - r0) < 0.5)
                else:
                    sel = np.array([r0 + int(rng.integers(0, r1 - r0))])
                nbr[k, sel] = full[k, sel]
    elif kind == 'broadcast':                 # every output gathers ONE input row; every fifth the last input row
        row = np.full(n_out, n_in // 2, np.int32)
        row[::5] = n_in - 1
        for k in range(0, K, 2):
            nbr[k] = row
    elif kind == 'last_row':                  # a single pair, in the last row of the last tile
        nbr[K - 1, n_out - 1] = n_in - 1
    else:
        raise ValueError(kind)
    return nbr


def two_neighbour_table(K, n_out, n_in=None, seed=0):
    """The centre offset everywhere + a second offset on half of the rows: T <= 2 cin (the arithmetic family)."""
    n_in = n_out if n_in is None else n_in
    nbr = table('centre', K, n_out, n_in, seed)
    if K > 1:
        rng = np.random.default_rng([seed, 77, K, n_out])
        k2 = 0 if K // 2 != 0 else 1
        sel = np.flatnonzero(rng.random(n_out) < 0.5)
        nbr[k2, sel] = _rows(rng, n_out, n_in)[sel]
    return nbr


def few_pairs_table(K, n_out, n_in=None, pairs=48, seed=0):
    """Every offset has `pairs` pairs spread over ALL tiles (distinct output rows, distinct input rows): the weight gradient's
    short sums (T = pairs per element of dW[k]) -- on a 64-tile map they still meet across tile chunks."""
    n_in = n_out if n_in is None else n_in
    rng = np.random.default_rng([seed, 78, K, n_out, n_in])
    nbr = np.full((K, n_out), -1, np.int32)
    p = min(pairs, n_out, n_in)
    for k in range(K):
        nbr[k, rng.permutation(n_out)[:p]] = rng.permutation(n_in)[:p]
    return nbr


def has_reverse(nbr):
    t = np.asarray(nbr)
    return all(len(np.unique(r[r >= 0])) == int((r >= 0).sum()) for r in t)


def reverse_table(nbr, n_in):
    """rev[k, i] = o with nbr[k, o] = i: the table the data gradient gathers dY through (needs distinct rows per offset)."""
    t = np.asarray(nbr)
    assert has_reverse(t), 'an offset gathers one input row twice: no reverse table'
    rev = np.full((t.shape[0], n_in), -1, np.int32)
    for k in range(t.shape[0]):
        o = np.flatnonzero(t[k] >= 0)
        rev[k, t[k, o]] = o
    return rev


# ----------------------------------------------------------------------------- operands
def _distinct_int_rows(rng, n, c, lo, hi):
    """(n, c) integers in [lo, hi], no two rows equal: the leading columns spell a shuffled row number in base hi-lo+1."""
    x = rng.integers(lo, hi + 1, (n, c))
    base = hi - lo + 1
    nd = 1
    while base ** nd < n:
        nd += 1
    assert nd <= c, 'too few channels for %d distinct rows' % n
    ids = rng.permutation(base ** nd)[:n]
    for d in range(nd):
        x[:, d] = ids // base ** d % base + lo
    return x


def exact_operands(seed, n_in, c1, c2, K, cout, n_out, xmax=4, wmax=8, g=0.125, bmax=16):
    """x1 (and x2, drawn from another range), dy: integers; w: multiples of g in [-wmax g, wmax g], neither symmetric under
    offset mirroring nor under transposition; bias, y0: integers.  All float32 tensors; `g` is the grid of every product."""
    rng = np.random.default_rng([seed, n_in, c1, c2, K, cout, n_out])
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    x1 = _distinct_int_rows(rng, n_in, c1, -xmax, xmax)
    x2 = _distinct_int_rows(rng, n_in, c2, -max(xmax - 1, 1), max(xmax - 1, 1)) if c2 else None
    w = rng.integers(-wmax, wmax + 1, (K, c1 + c2, cout)) * g
    if K > 1:
        assert not np.array_equal(w, w[::-1])
    if c1 + c2 == cout and cout > 1:
        assert not np.array_equal(w, w.transpose(0, 2, 1))
    return {'x1': f(x1), 'x2': f(x2) if c2 else None, 'w': f(w), 'g': g,
            'dy': f(_distinct_int_rows(rng, n_out, cout, -xmax, xmax) if 9 ** cout >= n_out else rng.integers(-xmax, xmax + 1, (n_out, cout))),
            'bias': f(rng.integers(-bmax, bmax + 1, (1, cout))), 'y0': f(rng.integers(-bmax, bmax + 1, (n_out, cout))),
            'dx0': f(rng.integers(-bmax, bmax + 1, (n_in, c1 + c2))),
            'dw0': f(rng.integers(-bmax, bmax + 1, (K, c1 + c2, cout))),
            'scale': f(2.0 ** rng.integers(-1, 2, cout)), 'shift': f(rng.integers(-bmax, bmax + 1, cout)),
            'res': f(rng.integers(-bmax, bmax + 1, (n_out, cout)))}


def _logu(rng, shape):
    return (2.0 ** rng.uniform(-6, 6, shape)) * rng.choice([-1.0, 1.0], shape)


def full_operands(seed, n_in, c1, c2, K, cout, n_out):
    """Full-mantissa operands: magnitudes log-uniform in [2^-6, 2^6], random signs, rounded to float32 (the operands ARE the
    float32 values: the reference starts from them)."""
    rng = np.random.default_rng([seed, 1, n_in, c1, c2, K, cout, n_out])
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return {'x1': f(_logu(rng, (n_in, c1))), 'x2': f(_logu(rng, (n_in, c2))) if c2 else None,
            'w': f(_logu(rng, (K, c1 + c2, cout))), 'dy': f(_logu(rng, (n_out, cout))),
            'bias': f(_logu(rng, (1, cout))), 'y0': f(_logu(rng, (n_out, cout))),
            'dx0': f(_logu(rng, (n_in, c1 + c2))), 'dw0': f(_logu(rng, (K, c1 + c2, cout)))}


def half_of(ops):
    """The operands rounded to binary16 (and back to float32 for the reference): what a half kernel is given."""
    out = {}
    for k, v in ops.items():
        out[k] = v.half().float() if torch.is_tensor(v) else v
    return out


# ----------------------------------------------------------------------------- fp32 evaluation in several orders, and mistakes
ORDERS = ('offset_major', 'reversed', 'split16')


def _accumulate(parts, y_init, order):
    """parts: contributions (index rows, values) in offset-major order -> sum in the named order."""
    if order == 'reversed':
        parts = parts[::-1]
    if order == 'split16':
        acc = [torch.zeros_like(y_init) for _ in range(16)]
        for j, (o, v) in enumerate(parts):
            acc[j % 16].index_add_(0, o, v)
        y = y_init.clone()
        for a in acc:
            y += a
        return y
    y = y_init.clone()
    for o, v in parts:
        y.index_add_(0, o, v)
    return y


def eval_fwd(nbr, x1, x2, w, bias=None, y0=None, order='offset_major', mut=None, dtype=torch.float32, width=None):
    """The forward pass in `dtype` arithmetic in the named order, into a buffer of `width` >= cout columns (the columns beyond
    cout hold the marker -7 and must be left alone), with one deliberate mistake `mut`."""
    K, n_out = np.asarray(nbr).shape
    t = _long(nbr).clone()
    w3 = w.to(dtype)
    cout = w3.shape[2]
    c1 = x1.shape[1]
    if mut == 'swap_sources':
        x = torch.cat([x2, x1], 1).to(dtype)
    else:
        x = _cat(x1, x2).to(dtype)
    if mut == 'x_11_bits':
        x = x.half().to(dtype)
    if mut == 'skip_channel':
        x = x.clone(); x[:, -1] = 0
    if mut == 'mirror_k':
        w3 = w3.flip(0)
    if mut == 'transpose_w':
        w3 = w3.transpose(1, 2)
    if mut == 'drop_pair':
        lt = (n_out - 1) // TILE * TILE
        k_, o_ = torch.nonzero(t[:, lt:] >= 0)[-1].tolist()
        t[k_, lt + o_] = -1
    y_init = torch.zeros(n_out, cout, dtype=dtype)
    if y0 is not None and mut != 'y0_ignored':
        y_init = y_init + y0.to(dtype) * (2 if mut == 'y0_twice' else 1)
    if bias is not None:
        y_init = y_init + bias.to(dtype).reshape(1, -1) * (16 if mut == 'bias_per_slice' else 1)
    parts = []
    for k in range(K):
        o = torch.nonzero(t[k] >= 0).reshape(-1)
        if o.numel():
            parts.append((o, x[t[k, o]] @ w3[k]))
    if mut == 'dup_pair':
        o, v = parts[-1]
        parts.append((o[-1:], v[-1:]))
    y = _accumulate(parts, y_init, order)
    if mut == 'acc_half_once':
        y = y.half().to(dtype)
    out = torch.full((n_out, cout if width is None else width), -7.0, dtype=dtype)
    out[:, :cout] = y
    if mut == 'overhang':
        out[:, cout] = y[:, -1]
    return out


def eval_epilogue(y, scale, shift, res, relu, mut=None, dtype=torch.float32):
    out = torch.addcmul(shift.to(dtype).reshape(1, -1), y.to(dtype), scale.to(dtype).reshape(1, -1))
    if mut == 'relu_before_res':
        out = out.clamp_min(0)
        return out + res.to(dtype) if res is not None else out
    if res is not None:
        out = out + res.to(dtype)
    return out.clamp_min(0) if relu else out


def eval_dgrad(nbr, dy, w, n_in, c0=0, c=None, dx0=None, mirror=False, order='offset_major', mut=None, dtype=torch.float32):
    """The data gradient the way the kernels compute it: the forward pass over the reverse table with W[k]^T.  mirror: the
    table IS its own reverse with the offsets mirrored (a stride-1 map: rev[k] = nbr[K-1-k]), so `nbr` is gathered through as it is
    and the weights are taken in mirrored order; the mistake 'dx_not_mirrored' takes them in plain order."""
    w3 = w if w.dim() == 3 else w.unsqueeze(0)
    c = w3.shape[1] - c0 if c is None else c
    wt = w3[:, c0:c0 + c].transpose(1, 2)
    if mirror:
        rev = nbr
        if mut != 'dx_not_mirrored':
            wt = wt.flip(0)
    else:
        rev = reverse_table(nbr, n_in)
    return eval_fwd(rev, dy, None, wt, None, dx0, order, mut if mut not in ('dx_not_mirrored',) else None, dtype)


def eval_wgrad(nbr, x, dy, dw0, ci0=0, order='offset_major', mut=None, dtype=torch.float32):
    """dW in `dtype`: per offset the pairs tile by tile (ascending, descending, or as 16 partial sums added last)."""
    K, n_out = np.asarray(nbr).shape
    t = _long(nbr).clone()
    if mut == 'drop_pair':
        lt = (n_out - 1) // TILE * TILE
        k_, o_ = torch.nonzero(t[:, lt:] >= 0)[-1].tolist()
        t[k_, lt + o_] = -1
    x = x.to(dtype); dy = dy.to(dtype)
    if mut == 'x_11_bits':
        x = x.half().to(dtype)
    cin = x.shape[1]
    dw = dw0.to(dtype).clone()
    at = 0 if mut == 'dw_offset_0' else ci0
    nt = (n_out + TILE - 1) // TILE
    for k in range(K):
        blocks = []
        for ti in range(nt):
            o = torch.nonzero(t[k, ti * TILE:(ti + 1) * TILE] >= 0).reshape(-1) + ti * TILE
            if o.numel():
                blocks.append(x[t[k, o]].t() @ dy[o])
        if mut == 'dup_pair' and blocks and k == K - 1:
            blocks.append(x[t[k, o[-1:]]].t() @ dy[o[-1:]])
        if not blocks:
            continue
        if order == 'reversed':
            blocks = blocks[::-1]
        if order == 'split16':
            acc = [torch.zeros(cin, dy.shape[1], dtype=dtype) for _ in range(16)]
            for j, b in enumerate(blocks):
                acc[j % 16] += b
            blocks = acc
        tot = dw[k, at:at + cin]
        for b in blocks:
            tot += b
        if mut == 'acc_half_once':
            dw[k, at:at + cin] = tot.half().to(dtype)
    return dw


def eval_tile_sums(y, n_out, mut=None):
    """Tile sums of the first n_out rows of a (possibly longer) buffer, the way a kernel gets them: tile by tile, row after row
    into fp64 accumulators (not the reshape of `tile_sums`); the mistake also counts the buffer's row n_out."""
    rows = n_out + 1 if mut == 'row_past_n_out' else n_out
    nt = (n_out + TILE - 1) // TILE
    out = torch.zeros(nt, 2, y.shape[1], dtype=torch.float64)
    for r in range(min(rows, nt * TILE)):
        v = y[r].double()
        out[r // TILE, 0] += v
        out[r // TILE, 1] += v * v
    return out


# ----------------------------------------------------------------------------- the two comparisons (CPU and GPU tests alike)
def same(got, ref):
    """Exact operands: the result IS the float64 rule, bit for bit (a float32 or binary16 value widens exactly)."""
    return tuple(got.shape) == tuple(ref.shape) and torch.equal(got.detach().cpu().double(), ref.double())


def inside(got, ref, bnd):
    """Full-mantissa operands: (every element inside its bound, largest error / bound)."""
    r = ratio(got.detach().cpu(), ref, bnd)
    return r <= 1.0, r

