"""Plain float64 restatement, on the CPU, of what box2mask_amd/csrc/norm.hip computes -- training- and eval-mode BatchNorm with the
fused residual add and ReLU (the reference's models/resnet.py:61-83: MinkowskiBatchNorm = torch BatchNorm1d over all rows, then
`out += residual; relu`), the pair of BatchNorms that meet in one add (resnet.py:73-82), segment mean / max pooling
(models/detection_net.py:345-352: global pooling by pooling id), ReLU and add -- together with the error bounds the kernels are
held to and the seeded cases shared by tests/test_norm_rule.py (CPU: the rule against float64 torch, the bounds against an fp32
evaluation in another order and against deliberate mistakes) and tests/test_gpu_norm.py (the kernels against the rule).  The last
section but one holds the binary16 BatchNorm kernels and the grouped SyncBN operator to the same rule (tests/test_gpu_norm_half.py),
the last one the SyncBN operators over ranks that hold DIFFERENT rows (tests/test_gpu_syncbn_ranks.py, profiles/syncbn_ranks_rule.md).

Everything is numpy float64 on the fp32 inputs widened exactly; column statistics are two-pass (mean, then the mean of the
squared deviations).  Inputs contain no -0.0, no NaN and no infinity: the packed atomic max of the kernel orders -0.0 below
+0.0 and has no slot for a NaN, and the rule says nothing about them.

u = 2^-24 is the relative error of one rounding to fp32; ulp32(v) is the spacing of fp32 at |v| (<= 2 u |v|).
"""
import numpy as np

from _loss_rule import ulp32 as _ulp32_scalar

U = 2.0 ** -24
EPS = 1e-5
MOMENTUM = 0.1
F64_DEPTH = 288           # see const_bounds


def ulp32(v):
    """ulp32 of _loss_rule, element-wise."""
    v = np.asarray(v, dtype=np.float64)
    if v.ndim == 0:
        return _ulp32_scalar(float(v))
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


# ------------------------------------------------------------------ the rule: BatchNorm
def bn_stats(x):
    """(mean, biased variance) of every column of x (n, c), two-pass in float64."""
    x = f64(x)
    mean = x.sum(0) / x.shape[0]
    var = ((x - mean) ** 2).sum(0) / x.shape[0]
    return mean, np.maximum(var, 0.0)


def bn_constants(mean, var, gamma, beta, eps=EPS):
    invstd = 1.0 / np.sqrt(var + float(np.float32(eps)))             # (the C entries take eps as a float)
    scale = f64(gamma) * invstd
    return invstd, scale, f64(beta) - mean * scale


def bn_forward(x, gamma, beta, res=None, relu=False, running=None, eps=EPS, momentum=MOMENTUM, count_factor=1):
    """Training mode.  running = (running_mean, running_var) before the step.  count_factor = 2: the statistics of [x; x] (same
    mean and variance, 2n rows in the unbiased factor), what the single-process SyncBN test feeds the entries."""
    x = f64(x)
    n = x.shape[0] * count_factor
    mean, var = bn_stats(x)
    invstd, scale, shift = bn_constants(mean, var, gamma, beta, eps)
    pre = x * scale + shift + (f64(res) if res is not None else 0.0)
    out = {'mean': mean, 'var': var, 'invstd': invstd, 'scale': scale, 'shift': shift, 'pre': pre,
           'y': np.maximum(pre, 0.0) if relu else pre}
    if running is not None:
        mom = float(np.float32(momentum))
        unb = var * n / (n - 1) if n > 1 else var
        out['running_mean'] = (1.0 - mom) * f64(running[0]) + mom * mean
        out['running_var'] = (1.0 - mom) * f64(running[1]) + mom * unb
    return out


def bn_eval_forward(x, gamma, beta, running_mean, running_var, res=None, relu=False, eps=EPS):
    x = f64(x)
    mean, var = f64(running_mean), f64(running_var)
    invstd, scale, shift = bn_constants(mean, var, gamma, beta, eps)
    pre = x * scale + shift + (f64(res) if res is not None else 0.0)
    return {'mean': mean, 'var': var, 'invstd': invstd, 'scale': scale, 'shift': shift, 'pre': pre,
            'y': np.maximum(pre, 0.0) if relu else pre}


def bn_backward(x, gamma, fwd, dy, mask=None):
    """Training mode, for a given ReLU mask (None: no ReLU): d beta, d gamma, dx, dres."""
    x, dy = f64(x), f64(dy)
    n = x.shape[0]
    g = dy * mask if mask is not None else dy
    xhat = (x - fwd['mean']) * fwd['invstd']
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    dx = f64(gamma) * fwd['invstd'] * (g - dbeta / n - xhat * (dgamma / n))
    return {'dbeta': dbeta, 'dgamma': dgamma, 'dx': dx, 'dres': g, 'g': g, 'xhat': xhat}


def bn_eval_backward(x, fwd, dy, mask=None):
    """Eval mode: an affine map of x; gamma and beta still have gradients (torch.nn.BatchNorm1d gives them)."""
    x, dy = f64(x), f64(dy)
    g = dy * mask if mask is not None else dy
    xhat = (x - fwd['mean']) * fwd['invstd']
    return {'dbeta': g.sum(0), 'dgamma': (g * xhat).sum(0), 'dx': g * fwd['scale'], 'dres': g, 'g': g, 'xhat': xhat}


# ------------------------------------------------------------------ the bounds: BatchNorm
def const_bounds(x, gamma, fwd, momentum=MOMENTUM, count_factor=1):
    """Allowed error of mean, invstd, scale, shift, running_mean, running_var (arrays over the columns).

    Every path forms S1 = sum x and S2 = sum x^2 in FP64 (x * x is exact in a double) and evaluates the finalize formulas in
    fp64, rounding each constant to fp32 ONCE: half an ulp32.  Asked for: 2 ulp32 of the fp64 value (that rounding, with a
    margin of 4), plus what the fp64 sums themselves can be off by.  An element of a column passes through at most
        chain + slots <= 257 (bn_stats_kernel: a thread's chain times the row slots is the block's <= 256 rows; the one-launch
        kernel: <= 64 per thread + 8 tree levels; a tile's 64 rows in the convolution epilogue)  +  <= 20 partials per lane and
        6 shuffle levels of the final kernel  +  the division, the product m * m and the subtraction
    fp64 additions: depth d = min(n + 4, 288), so to first order
        |dS1| <= d 2^-53 sum|x|,   |dS2| <= d 2^-53 sum x^2,
        |d mean| <= d 2^-53 mean|x|,
        |d var|  <= d 2^-53 (mean(x^2) + 2 |m| mean|x|) <= 3 d 2^-53 mean(x^2)        (|m| <= mean|x| <= sqrt(mean(x^2)))
    and through the formulas  d invstd = invstd^3 d var / 2,  d scale = |gamma| d invstd,
    d shift = |scale| d mean + |mean gamma| d invstd.  These fp64 terms matter only where the mean cancels (mean, shift) or
    dwarfs sigma (|mean| = 1000 sigma: 0.8 ulp32 of invstd); an fp32 accumulation of S1, S2 is off by hundreds of ulps there."""
    x = f64(x)
    n = x.shape[0]
    d = min(n + 4, F64_DEPTH) * 2.0 ** -53
    g = np.abs(f64(gamma))
    dmean = d * np.abs(x).sum(0) / n
    dvar = 3.0 * d * (x * x).sum(0) / n
    dinv = 0.5 * fwd['invstd'] ** 3 * dvar
    dshift = np.abs(fwd['scale']) * dmean + np.abs(fwd['mean']) * g * dinv
    b = {'mean': 2 * ulp32(fwd['mean']) + dmean, 'invstd': 2 * ulp32(fwd['invstd']) + dinv,
         'scale': 2 * ulp32(fwd['scale']) + g * dinv, 'shift': 2 * ulp32(fwd['shift']) + dshift,
         '_dscale64': g * dinv, '_dshift64': dshift}
    if 'running_mean' in fwd:
        nn = n * count_factor
        mom = float(np.float32(momentum))
        b['running_mean'] = 2 * ulp32(fwd['running_mean']) + mom * dmean
        b['running_var'] = 2 * ulp32(fwd['running_var']) + mom * dvar * (nn / (nn - 1.0) if nn > 1 else 1.0)
    return b


def y_bound(x, fwd, res=None, cb=None):
    """Per element.  y = max(fl(fl(x s + b) + res), 0) with s, b the fp32 constants: one rounding each of scale and shift
    (u |x scale|, u |shift|), of the fma (u |x scale + shift| <= u (|x scale| + |shift|)) and of the residual add (u |y|, ReLU
    only shrinks an error) -- first order  u (2 |x scale| + 2 |shift| + |y|), asked for with a margin: 4 u (|x scale| + |shift| +
    |res| + |y|), plus the fp64-level terms of const_bounds carried through (|x| d scale + d shift)."""
    x = f64(x)
    b = 4 * U * (np.abs(x * fwd['scale']) + np.abs(fwd['shift']) + (np.abs(f64(res)) if res is not None else 0.0)
                 + np.abs(fwd['y']))
    if cb is not None:
        b = b + np.abs(x) * cb['_dscale64'] + cb['_dshift64']
    return b


CHAIN = {'two_stage': 64, 'one_launch': 1}


def grad_bounds(x, gamma, fwd, bwd, chain, any_order=False):
    """Allowed error of d beta, d gamma (per column) and dx (per element) for the mask the sums were formed with.

    The reduction skeleton of the two-stage kernels forms, per thread, an fp32 chain of L <= 64 terms (c <= 256 and n <= 327 680:
    a block's <= 256 rows over its 256 / (c / 4) row slots) and adds the chains in fp64; the one-launch kernels add every term in
    fp64 (L = 1: no fp32 addition at all).  A chain of L terms has L - 1 roundings, the fp32 copy of the fp64 sum one more:
        |d dbeta|  <= (L + 3) u sum|g|                                   (L u, asked for with the margin of 3 u of the issue)
    A term of d gamma is fl(g fl(fl(x - m32) is32)): the subtraction, invstd's own rounding and the two products are four more
    roundings of |g xhat|, and the fp32 mean (half an ulp, allowed 2: <= 3 u |mean| with the subtraction's share) moves xhat by
    3 u |mean| invstd:
        |d dgamma| <= sum|g| ((L + 4) u |xhat| + 3 u |mean| invstd)
    (THIS DEPARTS FROM THE ISSUE'S FIGURES, 67 u and 4 u: counting the roundings above gives L + 4 = 68 u and 5 u.)
    dx = fl(ga (g - sg - xh sgx)), ga = fl(gamma is32), sg = fl(fl(S_g) inv_n), sgx alike, xh as above: at most 8 roundings on any
    of the four magnitudes |g|, |gbar|, |xhat gxbar| and (through xh's mean) |mean| invstd |gxbar|, all scaled by |gamma invstd|,
    plus the two sums' own errors carried through:
        |d dx| <= |gamma invstd| (8 u (|g| + |gbar| + |xhat gxbar| + |mean| invstd |gxbar|) + B_dbeta / n + |xhat| B_dgamma / n)
    any_order (the eval-mode gradients are torch reductions whose order is not ours to know): L = n.
    The binary16 entries accept c up to 1024, where a thread's chain is longer than 64 (114 rows at c = 512): their bounds call
    _grad_bounds with the L that chain_len derives from the launch geometry; the formulas are these."""
    return _grad_bounds(x, gamma, fwd, bwd, f64(x).shape[0] if any_order else CHAIN[chain])


def _grad_bounds(x, gamma, fwd, bwd, L):
    """grad_bounds for an fp32 chain of L terms (chain_len gives the L of a launch geometry)."""
    n = f64(x).shape[0]
    g, xhat = np.abs(bwd['g']), np.abs(bwd['xhat'])
    mi = np.abs(fwd['mean']) * fwd['invstd']
    b_dbeta = (L + 3) * U * g.sum(0)
    b_dgamma = (g * ((L + 4) * U * xhat + 3 * U * mi)).sum(0)
    gi = np.abs(f64(gamma) * fwd['invstd'])
    gbar, gxbar = np.abs(bwd['dbeta']) / n, np.abs(bwd['dgamma']) / n
    b_dx = gi * (8 * U * (g + gbar + xhat * gxbar + mi * gxbar) + b_dbeta / n + xhat * b_dgamma / n)
    return {'dbeta': b_dbeta, 'dgamma': b_dgamma, 'dx': b_dx}


def eval_grad_bounds(x, fwd, bwd):
    """Eval mode.  dx = fl(g scale32): the constant's rounding and the product, asked for with a margin: 4 u |g scale|.
    d beta is an fp32 sum of n terms in an order that is not ours: (n + 3) u sum|g|.  d gamma is evaluated as
    (sum g x - dbeta mean) invstd in fp32: both sums' any-order errors, scaled by invstd, and three more roundings.
    These are bounds of what functional's eval-mode backward IS (torch reductions; a difference of two sums that cancels where
    |mean| >> sigma), so they are wide -- about n u relative, more on the large-mean columns -- and catch a wrong formula, not a
    lost digit."""
    x = f64(x)
    n = x.shape[0]
    g = np.abs(bwd['g'])
    b_dbeta = (n + 3) * U * g.sum(0)
    b_dgamma = fwd['invstd'] * ((n + 3) * U * (g * np.abs(x)).sum(0) + np.abs(fwd['mean']) * (b_dbeta + 2 * U * g.sum(0))) \
        + 3 * U * np.abs(bwd['dgamma'])
    return {'dbeta': b_dbeta, 'dgamma': b_dgamma, 'dx': 4 * U * np.abs(bwd['dx'])}


def borderline(fwd, yb):
    """Elements whose fp64 pre-activation is within the y bound of zero: their ReLU decision may be the device's."""
    return np.abs(fwd['pre']) <= yb


def ratio(err, bound):
    """max err / bound over an array (0 / 0 = 0, x / 0 = inf)."""
    err, bound = np.broadcast_arrays(f64(err), f64(bound))
    if err.size == 0:
        return 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r))


def check(tag, rows, bad=None, quiet=False):
    """rows: (name, got, reference, bound array or None for exact).  Prints every ratio, returns the failures."""
    bad = [] if bad is None else bad
    for name, got, ref, b in rows:
        got, ref = f64(got), f64(ref)
        if got.shape != ref.shape:
            bad.append('%s: shape %s, expected %s' % (name, got.shape, ref.shape))
            continue
        if not np.all(np.isfinite(got)):
            bad.append('%s: not finite' % name)
            continue
        if b is None:
            k = int((got != ref).sum())
            if not quiet:
                print('%-28s %-14s exact, %d differ' % (tag, name, k))
            if k:
                bad.append('%s: %d elements differ (exact)' % (name, k))
            continue
        r = ratio(np.abs(got - ref), b)
        if not quiet:
            print('%-28s %-14s ratio %.3f' % (tag, name, r))
        if not r <= 1.0:
            bad.append('%s: error / bound = %.3g' % (name, r))
    return bad


CONSTS = ('mean', 'invstd', 'scale', 'shift', 'running_mean', 'running_var')


def bn_check(tag, inp, spec, got, quiet=False):
    """Everything a BatchNorm run produced (`got`: name -> fp32 array; absent names are not checked) against the rule for the case
    `inp` / `spec`.  The backward quantities are held to the rule evaluated with the mask of got['y'] > 0; outside the borderline
    elements that mask must be the rule's own.  Returns (failures, share of borderline elements)."""
    relu, res = spec['relu'], (inp['res'] if spec['res'] else None)
    cf = spec.get('count_factor', 1)
    if spec.get('eval'):
        fwd = bn_eval_forward(inp['x'], inp['gamma'], inp['beta'], inp['rm0'], inp['rv0'], res, relu)
        cb = {k: 2 * ulp32(fwd[k]) for k in ('scale', 'shift')}
        cb.update(_dscale64=0.0, _dshift64=0.0)
    else:
        fwd = bn_forward(inp['x'], inp['gamma'], inp['beta'], res, relu, (inp['rm0'], inp['rv0']), count_factor=cf)
        cb = const_bounds(inp['x'], inp['gamma'], fwd, count_factor=cf)
    yb = y_bound(inp['x'], fwd, res, cb)
    rows = [(k, got[k], fwd[k], cb[k]) for k in CONSTS if k in got and k in cb]
    bad = []
    share = 0.0
    mask = None
    if 'y' in got:
        rows.append(('y', got['y'], fwd['y'], yb))
        if relu:
            mask = f64(got['y']) > 0
            edge = borderline(fwd, yb)
            share = float(edge.mean())
            wrong = (mask != (fwd['pre'] > 0)) & ~edge
            if wrong.any():
                bad.append('ReLU mask differs in %d elements that are not borderline' % int(wrong.sum()))
    elif relu:
        raise ValueError('a ReLU case needs y for its mask')
    if 'dx' in got or 'dbeta' in got:
        m = mask.astype(np.float64) if mask is not None else None
        if spec.get('eval'):
            bwd = bn_eval_backward(inp['x'], fwd, inp['dy'], m)
            gb = eval_grad_bounds(inp['x'], fwd, bwd)
        else:
            bwd = bn_backward(inp['x'], inp['gamma'], fwd, inp['dy'], m)
            gb = grad_bounds(inp['x'], inp['gamma'], fwd, bwd, spec['chain'])
        rows += [(k, got[k], bwd[k], gb[k]) for k in ('dbeta', 'dgamma', 'dx') if k in got]
        if got.get('dres') is not None:
            rows.append(('dres', got['dres'], bwd['dres'], None))
    return check(tag, rows, bad, quiet), share


# ------------------------------------------------------------------ the rule and the bounds: the pair
def pair_check(tag, a, b, relu, got, quiet=False):
    """y = relu?(BN_a(xa) + BN_b(xb)), training mode, both ways (b2m_bn_apply2 / _bwd_reduce2 / _bwd_apply2: the two-stage
    skeleton).  y: the two fmas and the add -- 4 u (|xa sa| + |ba| + |xb sb| + |bb| + |y|) by the argument of y_bound."""
    fa = bn_forward(a['x'], a['gamma'], a['beta'], None, False, (a['rm0'], a['rv0']))
    fb = bn_forward(b['x'], b['gamma'], b['beta'], None, False, (b['rm0'], b['rv0']))
    ca, cb = const_bounds(a['x'], a['gamma'], fa), const_bounds(b['x'], b['gamma'], fb)
    pre = fa['y'] + fb['y']
    y = np.maximum(pre, 0.0) if relu else pre
    yb = 4 * U * (np.abs(f64(a['x']) * fa['scale']) + np.abs(fa['shift']) + np.abs(f64(b['x']) * fb['scale']) + np.abs(fb['shift'])
                  + np.abs(y)) + np.abs(f64(a['x'])) * ca['_dscale64'] + ca['_dshift64'] \
        + np.abs(f64(b['x'])) * cb['_dscale64'] + cb['_dshift64']
    rows = [('y', got['y'], y, yb)]
    for s, f, c in (('a', fa, ca), ('b', fb, cb)):
        rows += [(k + '_' + s, got[k + '_' + s], f[k], c[k]) for k in CONSTS if k + '_' + s in got]
    bad, share, m = [], 0.0, None
    if relu:
        mask = f64(got['y']) > 0
        edge = np.abs(pre) <= yb
        share = float(edge.mean())
        wrong = (mask != (pre > 0)) & ~edge
        if wrong.any():
            bad.append('ReLU mask differs in %d elements that are not borderline' % int(wrong.sum()))
        m = mask.astype(np.float64)
    if 'dx_a' in got:
        for s, inp, f in (('a', a, fa), ('b', b, fb)):
            bwd = bn_backward(inp['x'], inp['gamma'], f, a['dy'], m)
            gb = grad_bounds(inp['x'], inp['gamma'], f, bwd, 'two_stage')
            rows += [(k + '_' + s, got[k + '_' + s], bwd[k], gb[k]) for k in ('dbeta', 'dgamma', 'dx')]
    return check(tag, rows, bad, quiet), share


# ------------------------------------------------------------------ the rule and the bounds: segment pooling, ReLU, add
def seg_rule(x, ids, n_seg, mode, dout=None):
    """mode 'avg': the mean of the rows of every segment, 0 for an empty one; gradient dout[s] / len_s to every row.
    mode 'max': the maximum; the gradient goes to the LOWEST row among equal maxima (MinkowskiEngine's pooling keeps the first
    index it meets; torch's scatter_reduce('amax') would split it); an empty segment gives 0, argmax -1 and no gradient.
    -> dict(out, counts, argmax (max only), dx (if dout), bound (avg: per output element))."""
    x = f64(x)
    n, c = x.shape
    ids = np.asarray(ids, dtype=np.int64)
    counts = np.bincount(ids, minlength=n_seg).astype(np.int64) if n else np.zeros(n_seg, dtype=np.int64)
    out = np.zeros((n_seg, c))
    res = {'counts': counts}
    if mode == 'avg':
        sabs = np.zeros((n_seg, c))
        np.add.at(out, ids, x)
        np.add.at(sabs, ids, np.abs(x))
        ln = np.maximum(counts, 1)[:, None].astype(np.float64)
        out = out / ln
        # fp32 additions of len terms in ANY order (a summation tree over the rows; the atomics commute, the zero the output starts
        # from adds nothing): (len - 1) u sum|x|, the division one more rounding, the fp32 count exact -- over len, with a margin
        # of 3 u:  (len + 3) u sum|x_r| / len
        res['bound'] = (counts[:, None] + 3) * U * sabs / ln
        if dout is not None:
            res['dx'] = f64(dout)[ids] / ln[ids] if n else np.zeros((0, c))
    else:
        arg = np.full((n_seg, c), -1, dtype=np.int64)
        best = np.full((n_seg, c), -np.inf)
        for r in range(n):                                               # in row order: a later equal value does not replace
            s = ids[r]
            win = x[r] > best[s]
            best[s] = np.where(win, x[r], best[s])
            arg[s] = np.where(win, r, arg[s])
        out = np.where(arg >= 0, best, 0.0)
        res['argmax'] = arg
        if dout is not None:
            dx = np.zeros((n, c))
            if n:
                hit = arg[ids] == np.arange(n)[:, None]
                dx = np.where(hit, f64(dout)[ids], 0.0)
            res['dx'] = dx
    res['out'] = out
    return res


def seg_check(tag, case, mode, got, quiet=False):
    """got: out, counts, argmax (max), dx.  Exact: counts, the max values, argmax and the max gradient; the mean within its bound,
    the avg gradient (one correctly rounded division) within 1 ulp32."""
    ref = seg_rule(case['x'], case['ids'], case['n_seg'], mode, case['dout'])
    rows = [('counts', got['counts'], ref['counts'], None)]
    if mode == 'avg':
        rows.append(('out', got['out'], ref['out'], ref['bound']))
        if 'dx' in got:
            rows.append(('dx', got['dx'], ref['dx'], ulp32(ref['dx'])))
    else:
        rows += [('out', got['out'], ref['out'], None), ('argmax', got['argmax'], ref['argmax'], None)]
        if 'dx' in got:
            rows.append(('dx', got['dx'], ref['dx'], None))
    return check(tag, rows, None, quiet)


def relu_rule(x):
    return np.maximum(np.asarray(x, dtype=np.float32), np.float32(0))


def relu_bwd_rule(dy, y):
    return np.where(np.asarray(y) > 0, np.asarray(dy, dtype=np.float32), np.float32(0))


def add_rule(a, b):
    return np.asarray(a, dtype=np.float32) + np.asarray(b, dtype=np.float32)          # one fp32 rounding: the CPU's is the same


# ------------------------------------------------------------------ seeded inputs: BatchNorm
# The conditioning is PER COLUMN; column j is of kind KINDS[j % 8], so c = 4 holds the first four.
KINDS = ('ratio1000', 'const', 'ratio30', 'sigma1e-4', 'ratio100', 'sigma1e4', 'ratio0', 'ratio0.5')
_KIND = {'ratio1000': (1000.0, 1.0), 'ratio30': (30.0, 1.0), 'ratio100': (100.0, 1.0), 'ratio0': (0.0, 1.0),
         'ratio0.5': (0.5, 1.0), 'sigma1e-4': (1e-3, 1e-4), 'sigma1e4': (0.0, 1e4), 'const': (3.7, 0.0)}


def kind_of(j):
    return KINDS[j % 8]


def bn_input(n, c, seed=0):
    """x (n, c) with the per-column conditioning above (the sign of the mean alternates), a residual and an incoming gradient of
    unit scale, gamma in +-[0.5, 1.5], |beta| in [0.1, 1.1], running statistics that are not 0 / 1.  All float32."""
    rng = np.random.default_rng(7000 + 131 * seed + n * 7 + c)
    x = np.empty((n, c), dtype=np.float32)
    for j in range(c):
        mu, sd = _KIND[kind_of(j)]
        sgn = -1.0 if (j // 8) % 2 else 1.0
        x[:, j] = (rng.standard_normal(n) * sd + sgn * mu).astype(np.float32)
    sign = lambda k: np.where(rng.random(k) < 0.5, -1.0, 1.0)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return {'x': x, 'res': f(rng.standard_normal((n, c))), 'dy': f(rng.standard_normal((n, c))),
            'gamma': f(sign(c) * (rng.random(c) + 0.5)), 'beta': f(sign(c) * (rng.random(c) + 0.1)),
            'rm0': f(rng.standard_normal(c) * 0.3), 'rv0': f(rng.random(c) + 0.5)}


def eval_input(n, c, seed=0):
    """Eval mode: running statistics near the batch's own (the mean within sigma / 4, the variance within a factor of 2)."""
    inp = bn_input(n, c, seed)
    rng = np.random.default_rng(99 + seed)
    mean, var = bn_stats(inp['x'])
    sd = np.sqrt(var)
    inp['rm0'] = (mean + (rng.random(c) - 0.5) * 0.5 * sd).astype(np.float32)
    inp['rv0'] = (var * (0.5 + 1.5 * rng.random(c)) + 1e-12).astype(np.float32)
    return inp


_V = ((0, 0), (0, 1), (1, 0), (1, 1))                                   # (residual, relu)


def _bn_cases():
    cases = {}

    def add(path, n, c, res, relu, ld=None, **kw):
        name = '%s-n%d-c%d-res%d-relu%d' % (path, n, c, res, relu) + ('-ld%s' % ld if ld else '')
        chain = 'one_launch' if path in ('small', 'small16k', 'syncsmall') else 'two_stage'
        cases[name] = dict(path=path, n=n, c=c, res=bool(res), relu=bool(relu), ld=ld, chain=chain, **kw)
    # one launch (default B2M_BN_SMALL_ROWS = 2048): c / 4 = 1, 8, 24, 64 workgroups
    for i, (n, c) in enumerate(((2, 4), (2, 96), (255, 32), (256, 96), (256, 4), (257, 256), (2048, 32), (2048, 96))):
        add('small', n, c, *_V[(i + 3) % 4])
    for v in _V:
        add('small', 257, 96, *v)
        add('small', 2048, 256, *v)
    add('small', 255, 96, 1, 1, ld='c+4')
    add('small', 257, 32, 0, 1, ld='2c')
    add('small', 257, 32, 1, 0, ld='2c')
    add('small16k', 16384, 32, 1, 1)                                     # B2M_BN_SMALL_ROWS = 16384: 64 rows per thread
    # two-stage from x (B2M_BN_SMALL_ROWS = 0)
    for i, (n, c) in enumerate(((2, 4), (3, 32), (255, 96), (257, 256), (1025, 32), (1025, 4), (20000, 256))):
        add('stats', n, c, *_V[(i + 3) % 4])
    for v in _V:
        add('stats', 5000, 256, *v)
        add('stats', 20000, 96, *v)
    add('stats', 257, 96, 1, 1, ld='c+4')
    add('stats', 1025, 32, 0, 1, ld='2c')
    add('stats', 1025, 32, 1, 1, ld='2c')
    # statistics from per-tile sums (64 rows per tile, the last one partial); one kernel, and the two-launch form
    for n, c, v, one in ((65, 32, 3, 1), (65, 96, 1, 0), (4097, 96, 3, 1), (4097, 256, 2, 0), (4097, 4, 1, 0)):
        add('tiles' if one else 'tiles2', n, c, *_V[v])
    # the SyncBN entries in one process: the sums doubled and count_dev = 2 n on the device -- the rule on [x; x]
    add('sync', 5000, 96, 1, 1, count_factor=2)
    add('sync', 257, 32, 0, 1, count_factor=2)
    add('sync', 3, 4, 0, 0, count_factor=2)
    add('synctiles', 4097, 96, 1, 1, count_factor=2)                    # ... the sums from b2m_bn_tilestats
    add('syncsmall', 257, 96, 1, 1, count_factor=2)                     # ... the one-launch kernels cut in two around the exchange
    add('syncsmall', 2048, 32, 0, 1, count_factor=2)
    add('eval', 5000, 96, 1, 1, eval=True)
    add('eval', 9, 32, 0, 1, eval=True)
    add('eval', 9, 32, 0, 0, eval=True)
    return cases


BN_CASES = _bn_cases()
PAIR_CASES = {'pair-n300-c64': (300, 64, True), 'pair-n2500-c96': (2500, 96, True), 'pair-n5000-c256': (5000, 256, True),
              'pair-n300-c64-norelu': (300, 64, False)}


def bn_case_input(name):
    s = BN_CASES[name]
    mk = eval_input if s.get('eval') else bn_input
    return mk(s['n'], s['c'], seed=sorted(BN_CASES).index(name))


def pair_case_input(name):
    n, c, _ = PAIR_CASES[name]
    k = sorted(PAIR_CASES).index(name)
    a, b = bn_input(n, c, seed=500 + k), bn_input(n, c, seed=600 + k)
    b['x'] = np.ascontiguousarray(b['x'][:, ::-1])                       # another kind meets each column of a
    return a, b


def tile_sums(x):
    """[ntiles][2c] float64: sum x | sum x^2 over tiles of 64 rows (the last one partial), what b2m_conv_fwd_stats leaves."""
    x = f64(x)
    n, c = x.shape
    nt = (n + 63) // 64
    ts = np.zeros((nt, 2 * c))
    for t in range(nt):
        blk = x[t * 64:(t + 1) * 64]
        ts[t, :c] = blk.sum(0)
        ts[t, c:] = (blk * blk).sum(0)
    return ts


# ------------------------------------------------------------------ seeded inputs: segment pooling
def _ids(layout, n, n_seg, rng):
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    if layout == 'runs':                       # Morton-like: runs of 1 .. 200 rows that cross the 64-row blocks, ids shuffled
        lens = []
        while sum(lens) < n:
            lens.append(int(rng.integers(1, 201)))
        labels = rng.permutation(n_seg)[:len(lens)] if len(lens) <= n_seg else rng.integers(0, n_seg, len(lens))
        return np.repeat(labels, lens)[:n].astype(np.int64)
    if layout == 'random':
        return rng.integers(0, n_seg, n).astype(np.int64)
    if layout == 'one':
        return np.full(n, n_seg - 1, dtype=np.int64)
    if layout == 'gaps':                       # only every third id is used
        return (rng.integers(0, (n_seg + 2) // 3, n) * 3).clip(max=n_seg - 1).astype(np.int64)
    raise ValueError(layout)


SEG_CASES = {}
for _i, (_n, _c, _lay, _ns) in enumerate((
        (1, 1, 'one', 1), (1, 96, 'one', 3), (63, 3, 'runs', 5), (64, 13, 'random', 7), (65, 96, 'runs', 4),
        (67, 256, 'random', 9), (67, 320, 'runs', 3), (65, 1, 'gaps', 12), (64, 320, 'one', 2), (63, 96, 'random', 200),
        (7000, 96, 'runs', 120), (7000, 13, 'random', 211), (7000, 320, 'runs', 90), (7000, 3, 'gaps', 50),
        (7000, 256, 'one', 1), (7000, 1, 'runs', 100), (0, 96, 'random', 5), (0, 13, 'random', 0))):
    SEG_CASES['seg-n%d-c%d-%s-s%d' % (_n, _c, _lay, _ns)] = (_n, _c, _lay, _ns, _i)


def seg_case(name, flavour='plain'):
    """flavour (max inputs): 'negative' -- every value below zero; 'ties' -- every third row a copy of the row before it and
    post-ReLU zeros across whole segments (every value of segment ids[0] and of every fourth segment is 0)."""
    n, c, layout, n_seg, k = SEG_CASES[name]
    rng = np.random.default_rng(4000 + k)
    ids = _ids(layout, n, n_seg, rng)
    x = rng.standard_normal((n, c)).astype(np.float32)
    if flavour == 'negative':
        x = -np.abs(x) - np.float32(0.25)
    elif flavour == 'ties' and n:
        x = np.maximum(x, np.float32(0))       # post-ReLU: many zeros (and no -0.0)
        x[2::3] = x[1:-1:3][:len(x[2::3])]
        x[(ids % 4 == 0) | (ids == ids[0])] = 0
    dout = rng.standard_normal((n_seg, c)).astype(np.float32)
    return {'x': x, 'ids': ids, 'n_seg': n_seg, 'dout': dout, 'n': n, 'c': c}


# ------------------------------------------------------------------ an fp32 evaluation in another order, and mistakes
def _seq32(t):
    """Column sums of an fp32 array, one row after the other in fp32 (np.cumsum is sequential along axis 0)."""
    t = np.asarray(t, dtype=np.float32)
    return np.cumsum(t, axis=0, dtype=np.float32)[-1] if t.shape[0] else np.zeros(t.shape[1], dtype=np.float32)


def _seq64(t):
    t = f64(t)
    return np.cumsum(t, axis=0)[-1] if t.shape[0] else np.zeros(t.shape[1])


MISTAKES = ('drop_row', 'drop_group', 'drop_slot', 'unbiased', 'mask_ge', 'no_bessel', 'fp32_chains')


def bn_emulate(inp, spec, mistake=None):
    """The rule's formulas in fp32 the way a straightforward kernel would evaluate them, in an order unlike norm.hip's: the
    statistics as plain sequential fp64 sums down every column, the backward sums as plain sequential fp32 sums; constants rounded
    once.  `mistake`: one deliberate error (MISTAKES)."""
    f = np.float32
    x, dy = inp['x'], inp['dy']
    n, c = x.shape
    cf = spec.get('count_factor', 1)
    keep = np.ones(n, dtype=bool)
    if mistake == 'drop_row':
        keep[n - 1] = False
    if mistake == 'drop_slot':
        keep[1::max(256 // (c // 4), 2)] = False
    gamma, beta = f64(inp['gamma']), f64(inp['beta'])
    got = {}
    if spec.get('eval'):
        m, var = f64(inp['rm0']), f64(inp['rv0'])
    else:
        if mistake == 'fp32_chains':
            s1, s2 = np.zeros(c), np.zeros(c)
            for r in range(0, n, 25):
                blk = x[r:r + 25]
                s1 += _seq32(blk)
                s2 += _seq32(blk * blk)
        else:
            xs = f64(x[keep])
            s1, s2 = _seq64(xs), _seq64(xs * xs)
        m = s1 / n
        var = np.maximum(s2 / n - m * m, 0.0)
        nn = n * cf
        unb = var if (mistake == 'no_bessel' or nn <= 1) else var * nn / (nn - 1)
        mom = float(f(MOMENTUM))
        got['running_mean'] = ((1 - mom) * f64(inp['rm0']) + mom * m).astype(f)
        got['running_var'] = ((1 - mom) * f64(inp['rv0']) + mom * unb).astype(f)
        if mistake == 'unbiased' and n > 1:
            var = var * n / (n - 1)
    inv = 1.0 / np.sqrt(var + float(f(EPS)))
    mean32, inv32 = m.astype(f), inv.astype(f)
    sc32, sh32 = (gamma * inv).astype(f), (beta - m * gamma * inv).astype(f)
    if not spec.get('eval'):
        got.update(mean=mean32, invstd=inv32)
    got.update(scale=sc32, shift=sh32)
    y = (f64(x) * f64(sc32) + f64(sh32)).astype(f)                         # an fma: one rounding
    if spec['res']:
        y = y + inp['res']
    mask = None
    if spec['relu']:
        y = np.maximum(y, f(0))
        mask = (y >= 0) if mistake == 'mask_ge' else (y > 0)               # (of the OUTPUT: y >= 0 holds everywhere)
    got['y'] = y
    g = dy * mask.astype(f) if mask is not None else dy
    xh = (x - mean32) * inv32
    if spec.get('eval'):
        got.update(dbeta=_seq32(g), dgamma=_seq32(g * xh), dx=g * sc32)
    else:
        sg, sgx = _seq32(g[keep]), _seq32((g * xh)[keep])
        got.update(dbeta=sg, dgamma=sgx)
        inv_n = f(1.0 / n)
        got['dx'] = (inp['gamma'] * inv32) * (g - sg * inv_n - xh * (sgx * inv_n))
    if spec['res']:
        got['dres'] = g.copy()
    if mistake == 'drop_group':
        j = 4 if c > 4 else 0
        for k, v in got.items():
            (v[:, j:j + 4] if v.ndim == 2 else v[j:j + 4]).fill(0)
    return got


SEG_MISTAKES = ('highest_tie', 'empty_count_one', 'drop_row')


def seg_emulate(case, mode, mistake=None):
    """Segment pooling in fp32, every segment's rows added in REVERSE row order."""
    f = np.float32
    x, ids, n_seg, dout = case['x'], case['ids'], case['n_seg'], case['dout']
    n, c = x.shape
    counts = np.bincount(ids, minlength=n_seg).astype(np.int64) if n else np.zeros(n_seg, dtype=np.int64)
    out = np.zeros((n_seg, c), dtype=f)
    arg = np.full((n_seg, c), -1, dtype=np.int64)
    for s in np.unique(ids):
        rows = np.nonzero(ids == s)[0]
        if mistake == 'drop_row' and len(rows) > 1:
            rows = rows[:-1]
        blk = x[rows]
        if mode == 'avg':
            out[s] = _seq32(blk[::-1]) / f(counts[s])
        else:
            out[s] = blk.max(0)
            hit = blk == out[s]
            pick = (len(rows) - 1 - np.argmax(hit[::-1], axis=0)) if mistake == 'highest_tie' else np.argmax(hit, axis=0)
            arg[s] = rows[pick]
    got = {'out': out, 'counts': np.maximum(counts, 1) if mistake == 'empty_count_one' else counts}
    if mode == 'avg':
        got['dx'] = (dout[ids] / counts[ids].astype(f)[:, None]) if n else np.zeros((0, c), dtype=f)
    else:
        got['argmax'] = arg
        got['dx'] = np.where(arg[ids] == np.arange(n)[:, None], dout[ids], f(0)) if n else np.zeros((0, c), dtype=f)
    return got


def pair_emulate(a, b, relu):
    """relu?(BN_a(xa) + BN_b(xb)) and its gradients from two bn_emulate evaluations and one fp32 add."""
    f = np.float32
    plain = {'res': False, 'relu': False}
    ea, eb = bn_emulate(a, plain), bn_emulate(b, plain)
    y = ea['y'] + eb['y']
    mask = (y > 0).astype(f) if relu else np.ones_like(y)
    got = {'y': np.maximum(y, f(0)) if relu else y}
    g = a['dy'] * mask
    n = y.shape[0]
    for s, inp, e in (('a', a, ea), ('b', b, eb)):
        xh = (inp['x'] - e['mean']) * e['invstd']
        sg, sgx = _seq32(g), _seq32(g * xh)
        inv_n = f(1.0 / n)
        got.update({'dbeta_' + s: sg, 'dgamma_' + s: sgx,
                    'dx_' + s: (inp['gamma'] * e['invstd']) * (g - sg * inv_n - xh * (sgx * inv_n))})
        got.update({k + '_' + s: e[k] for k in CONSTS})
    return got


# ================================================================== binary16 BatchNorm (half_train._BatchNormH) and grouped SyncBN
# The half kernels of norm.hip read binary16 x / residual / dy, widen them exactly, do the arithmetic of their fp32 twins and round
# ONCE to binary16 (round to nearest even) on the way out; gamma, beta, the constants and the running statistics are fp32.  The rule
# is the fp64 rule above ON THE HALF-ROUNDED INPUTS (exactly what the device reads), and every bound is the fp32 twin's plus what
# that one rounding can add.  HALF_CASES / GROUP_CASES carry their own seeds: BN_CASES' inputs depend on its sorted key order.
H_MAX = 65504.0
H_TINY = 2.0 ** -24                      # the spacing of the binary16 subnormals (and of the first normal binade)


def to_half(a):
    """fp32 -> binary16 (round to nearest even, numpy's conversion; clipped to the largest finite value first) -> fp32, exactly."""
    return np.clip(np.asarray(a, dtype=np.float32), -H_MAX, H_MAX).astype(np.float16).astype(np.float32)


def half_spacing(v):
    """Distance between neighbouring binary16 values at magnitude |v|: 2^(e - 10) for 2^e <= |v| < 2^(e + 1), e >= -14; the
    subnormals (|v| < 2^-14) are 2^-24 apart; the top binade (e = 15) reaches 65504 and its spacing, 32, serves above it."""
    v = np.abs(f64(v))
    e = np.floor(np.log2(np.maximum(v, 2.0 ** -14)))
    return 2.0 ** (np.minimum(e, 15.0) - 10.0)


def half_store(v32, b):
    """What one round-to-nearest store to binary16 adds to a bound.  The device holds an fp32 value v with |v - r| <= b (r the
    rule's, b the fp32 bound) and stores h = half(v): |h - v| <= spacing16(|v|) / 2, and the spacing never decreases with the
    magnitude, |v| <= |r| + b, so  |h - r| <= b + spacing16(|r| + b) / 2  -- for |r| + b < 65520, where the conversion is finite."""
    return b + 0.5 * half_spacing(np.abs(f64(v32)) + b)


def chain_len(n, c):
    """Longest fp32 chain of the two-stage skeleton (column_reduce_staged in norm.hip) for n rows of c columns: min(ceil(n / 256),
    1280) blocks share the rows evenly, a block's rows go round-robin to its 256 / (c / 4) row slots (integer division), and a
    thread adds its slot's rows in fp32.  <= 64 for c <= 256 and n <= 327 680 (CHAIN['two_stage']); 128 at c = 512, 256 at c = 1024."""
    nblk = min(max(-(-n // 256), 1), 1280)
    rows = -(-n // nblk)
    nslots = 256 // (c // 4)
    return -(-rows // nslots)


def half_input(n, c, seed):
    inp = bn_input(n, c, seed)
    for k in ('x', 'res', 'dy'):
        inp[k] = to_half(inp[k])
    return inp


def _half_cases():
    cases = {}

    def add(path, n, c, res, relu, ld=None, **kw):
        name = '%s-n%d-c%d-res%d-relu%d' % (path, n, c, res, relu) + ('-ld%s' % ld if ld else '')
        cases[name] = dict(path=path, n=n, c=c, res=bool(res), relu=bool(relu), ld=ld, chain=chain_len(n, c), seed=len(cases), **kw)
    for i, (n, c) in enumerate(((2, 4), (3, 32), (255, 96), (257, 256), (1025, 32))):
        add('stats_h', n, c, *_V[(i + 3) % 4])
    for v in _V:
        add('stats_h', 5000, 96, *v)
        add('stats_h', 5000, 256, *v)
    add('stats_h', 2049, 512, 1, 1)
    add('stats_h', 257, 96, 1, 1, ld='c+4')
    add('stats_h', 1025, 32, 0, 1, ld='2c')
    add('stats_h', 1025, 32, 1, 1, ld='2c')
    add('tiles_h', 65, 32, 1, 1)
    add('tiles_h', 4097, 96, 0, 1)
    add('sync_h', 5000, 96, 1, 1, count_factor=2)
    add('sync_h', 257, 32, 0, 1, count_factor=2, tiles=True)          # (this rank's sums from b2m_bn_tilestats)
    add('sync_h', 3, 4, 0, 0, count_factor=2)
    return cases


HALF_CASES = _half_cases()
# members' channel counts; every member is a SyncBN layer without ReLU or residual over the same n rows, the sums doubled
GROUP_CASES = {'group-n2': (2, (96, 32, 4, 256)), 'group-n257': (257, (96, 32, 4, 256)), 'group-n5000': (5000, (96, 32, 4, 256)),
               'group-n3-c96x2': (3, (96, 96))}
GROUP_SPEC = {'relu': False, 'res': False, 'chain': 'two_stage', 'count_factor': 2}


def half_case_input(name):
    s = HALF_CASES[name]
    return half_input(s['n'], s['c'], 2000 + s['seed'])


def group_case_inputs(name):
    n, cs = GROUP_CASES[name]
    k = list(GROUP_CASES).index(name)
    return [bn_input(n, c, 3000 + 10 * k + j) for j, c in enumerate(cs)]


def is_pow2(s):
    m, _ = np.frexp(float(s))
    return m == 0.5


def bn_check_half(tag, inp, spec, got, pgs=1.0, quiet=False):
    """A binary16 BatchNorm run against the rule.  got: the fp32 constants, y / dx / dres (binary16 values, any float dtype), dbeta /
    dgamma (fp32, ALREADY multiplied by pgs = param_grad_scale, a float32 value), and -- for ReLU without a residual -- 'mask', the
    device's own decisions read off the dres the entry writes when asked to.  Returns (failures, borderline share).

    constants  const_bounds as they are: the statistics are fp64 sums of the widened half inputs on every path.
    y          half_store(y, y_bound): the fp32 value y_bound covers, then one store.
    dx         half_store(dx, grad_bounds' dx), with the chain length L = spec['chain'] of the launch geometry (chain_len).
    dres       exact: dy * mask is a binary16 value, widened and stored again.
    dbeta, dgamma   grad_bounds', times pgs: the kernel forms fl(fl32(S) * pgs).  A power of two only moves the exponent (no
               underflow at these magnitudes): no new error.  Any other pgs rounds once more: u (|S pgs| + bound) in addition.
    mask       WITH a fused residual the backward reads the stored y: mask = y16 > 0.  The fp32 value v (|v - pre| <= y_bound) stores
               as 0 when v <= 2^-25 (tie to even), so the decision may be the device's where |pre| <= y_bound + 2^-24.  WITHOUT one the
               kernels take the sign of fl(fma(x, scale, shift)) in fp32 and never look at y: borderline where |pre| <= y_bound.
               Everywhere else the mask must be the rule's pre > 0."""
    relu, res = spec['relu'], (inp['res'] if spec['res'] else None)
    cf = spec.get('count_factor', 1)
    for k in ('x', 'res', 'dy'):
        assert np.array_equal(to_half(inp[k]), inp[k]), '%s is not binary16' % k
    fwd = bn_forward(inp['x'], inp['gamma'], inp['beta'], res, relu, (inp['rm0'], inp['rv0']), count_factor=cf)
    cb = const_bounds(inp['x'], inp['gamma'], fwd, count_factor=cf)
    yb = y_bound(inp['x'], fwd, res, cb)
    rows = [(k, got[k], fwd[k], cb[k]) for k in CONSTS if k in got]
    bad, share, mask = [], 0.0, None
    if 'y' in got:
        rows.append(('y', got['y'], fwd['y'], half_store(fwd['y'], yb)))
    if relu:
        if spec['res']:
            mask = f64(got['y']) > 0
            edge = np.abs(fwd['pre']) <= yb + H_TINY
        else:
            mask = np.asarray(got['mask'], dtype=bool)
            edge = np.abs(fwd['pre']) <= yb
        share = float(edge.mean())
        wrong = (mask != (fwd['pre'] > 0)) & ~edge
        if wrong.any():
            bad.append('ReLU mask differs in %d elements that are not borderline' % int(wrong.sum()))
    if 'dx' in got or 'dbeta' in got:
        m = mask.astype(np.float64) if mask is not None else None
        bwd = bn_backward(inp['x'], inp['gamma'], fwd, inp['dy'], m)
        gb = _grad_bounds(inp['x'], inp['gamma'], fwd, bwd, spec['chain'])
        s = float(np.float32(pgs))
        for k in ('dbeta', 'dgamma'):
            if k in got:
                b = gb[k] * s
                if not is_pow2(s):
                    b = b + U * (np.abs(bwd[k]) * s + b)
                rows.append((k, got[k], bwd[k] * s, b))
        if 'dx' in got:
            rows.append(('dx', got['dx'], bwd['dx'], half_store(bwd['dx'], gb['dx'])))
        if got.get('dres') is not None:
            rows.append(('dres', got['dres'], bwd['dres'], None))
    return check(tag, rows, bad, quiet), share


def _round_half(v32, toward_zero=False):
    v32 = np.asarray(v32, dtype=np.float32)
    h = v32.astype(np.float16)
    if toward_zero:
        over = np.abs(h.astype(np.float32)) > np.abs(v32)
        h = np.where(over, np.nextafter(h, np.float16(0)), h)
    return h.astype(np.float32)


def _chains32(x, c):
    """Sum x and sum x^2 the way bn_stats_h_kernel formed them while it accumulated in fp32: per block and row slot an fp32 chain in
    row order (the product of two binary16 values is exact in fp32), the chains added in fp64 (slots, then blocks)."""
    n = x.shape[0]
    nblk = min(max(-(-n // 256), 1), 1280)
    rows = -(-n // nblk)
    nslots = 256 // (c // 4)
    s1, s2 = np.zeros(c), np.zeros(c)
    for b in range(nblk):
        blk = x[b * rows:min((b + 1) * rows, n)]
        for rs in range(min(nslots, blk.shape[0])):
            t = blk[rs::nslots]
            s1 += _seq32(t)
            s2 += _seq32(t * t)
    return s1, s2


HALF_MISTAKES = ('fp32_chains_h', 'truncate_half', 'no_unscale', 'mask_ge', 'drop_row')


def bn_emulate_h(inp, spec, mistake=None, pgs=1.0):
    """bn_emulate for the binary16 operator: sequential fp64 statistics, sequential fp32 backward sums, fp32 element arithmetic, one
    round-to-nearest-even store of y, dx and dres.  `mistake`: one of HALF_MISTAKES."""
    f = np.float32
    x, dy = inp['x'], inp['dy']
    n, c = x.shape
    cf = spec.get('count_factor', 1)
    keep = np.ones(n, dtype=bool)
    if mistake == 'drop_row':
        keep[n - 1] = False
    gamma, beta = f64(inp['gamma']), f64(inp['beta'])
    if mistake == 'fp32_chains_h':
        s1, s2 = _chains32(x, c)
    else:
        xs = f64(x[keep])
        s1, s2 = _seq64(xs), _seq64(xs * xs)
    m = s1 / n
    var = np.maximum(s2 / n - m * m, 0.0)
    nn = n * cf
    unb = var * nn / (nn - 1) if nn > 1 else var
    mom = float(f(MOMENTUM))
    got = {'running_mean': ((1 - mom) * f64(inp['rm0']) + mom * m).astype(f),
           'running_var': ((1 - mom) * f64(inp['rv0']) + mom * unb).astype(f)}
    inv = 1.0 / np.sqrt(var + float(f(EPS)))
    mean32, inv32 = m.astype(f), inv.astype(f)
    sc32, sh32 = (gamma * inv).astype(f), (beta - m * gamma * inv).astype(f)
    got.update(mean=mean32, invstd=inv32, scale=sc32, shift=sh32)
    v = (f64(x) * f64(sc32) + f64(sh32)).astype(f)                         # an fma: one rounding
    if spec['res']:
        v = v + inp['res']
    rnd = lambda a: _round_half(a, mistake == 'truncate_half')
    mask = None
    if spec['relu']:
        y = rnd(np.maximum(v, f(0)))
        w = y if spec['res'] else v                                        # the stored output's sign / the fp32 value's
        mask = (w >= 0) if mistake == 'mask_ge' else (w > 0)
        if not spec['res']:
            got['mask'] = mask
    else:
        y = rnd(v)
    got['y'] = y
    g = dy * mask.astype(f) if mask is not None else dy
    xh = (x - mean32) * inv32
    sg, sgx = _seq32(g[keep]), _seq32((g * xh)[keep])
    s = f(1.0) if mistake == 'no_unscale' else f(pgs)
    got.update(dbeta=sg * s, dgamma=sgx * s)
    inv_n = f(1.0 / n)
    got['dx'] = rnd((inp['gamma'] * inv32) * (g - sg * inv_n - xh * (sgx * inv_n)))
    if spec['res']:
        got['dres'] = rnd(g)
    return got


# ================================================================== SyncBN over ranks that hold DIFFERENT rows
# W ranks hold x_0 .. x_{W-1} (n_r rows each, any of them possibly none) of one batch X = [x_0; ...; x_{W-1}], N = sum n_r, with the
# incoming gradients DY and residuals stacked alike.  The operators exchange (sum x, sum x^2, n_r) forward and (sum g, sum g xhat)
# backward, each packed into ONE fp64 all-reduce, and document:
#     constants, running statistics   the rule's on X, with N in the unbiased factor -- the same on every rank;
#     y_r, dx_r                       the row slices of the rule's y and dx on X (dx with the sums over ALL rows, over N);
#     dbeta_r, dgamma_r               the sums over rank r's rows only, with the global xhat (the gradient all-reduce averages the
#                                     parameter gradients over the ranks afterwards, like every other gradient).
# The bounds are the one-rank bounds with what the exchange adds:
#     constants   const_bounds(X), its fp64 depth term raised by W: an element of rank r passes through at most min(n_r + 4, 288) <=
#                 min(N + 4, 288) fp64 additions on its rank and at most W more where the packed sums meet (rank order), so
#                 d = (min(N + 4, 288) + W) 2^-53 in const_bounds' formulas;
#     y           y_bound with those constants;
#     dbeta_r, dgamma_r   _grad_bounds on rank r's rows with the chain length L_r of the path that rank took (1: the small-map
#                 half-kernels, every term added in fp64; 64: the two-stage kernels; chain_len(n_r, c) for the binary16 kernels) -- the
#                 global mean's own error enters through the 3 u |mean| invstd term exactly as on one rank;
#     dx_r        _grad_bounds' formula with the carried terms of ALL ranks: the device forms fl(fl32(S) / N) from S = sum_r S_r (fp64,
#                 W - 1 more additions at 2^-53, nothing against the 3 u of margin), and S_r is off by at most B_r:
#                     |gamma invstd| (8 u (|g| + |gbar| + |xhat gxbar| + |mean| invstd |gxbar|) + sum_r B_dbeta_r / N + |xhat| sum_r B_dgamma_r / N)
#                 with gbar = |sum g| / N and gxbar = |sum g xhat| / N over all rows;
#     binary16    one store more (half_store), the mask conventions and param_grad_scale of bn_check_half.
RANK_SPREAD = (0.0, 3.0, 0.3, 10.0)       # distance between neighbouring ranks' column means, in units of the column's sigma


def bn_input_ranks(rows, c, seed=0, half=False):
    """bn_input for ranks of rows[r] rows each -> one dict per rank (x, res, dy of that rank; gamma, beta, rm0, rv0 shared).  The
    column means differ between the ranks: rank r's column j is moved by (r - (W - 1) / 2) * RANK_SPREAD[(j + j // 8) % 4] sigma_j (a
    constant column, sigma = 0, by that many units), so that in a quarter of the columns the spread BETWEEN the ranks is 25 times
    the variance within one, in another quarter about twice, and in one quarter the ranks agree."""
    world, total = len(rows), int(sum(rows))
    base = bn_input(total, c, seed)
    lo = np.concatenate([[0], np.cumsum(rows)]).astype(int)
    step = np.array([RANK_SPREAD[(j + j // 8) % 4] * (_KIND[kind_of(j)][1] or 1.0) for j in range(c)])
    out = []
    for r in range(world):
        sl = slice(lo[r], lo[r + 1])
        d = dict(base)
        d['x'] = np.ascontiguousarray((base['x'][sl].astype(np.float64) + (r - (world - 1) / 2.0) * step).astype(np.float32))
        d['res'], d['dy'] = np.ascontiguousarray(base['res'][sl]), np.ascontiguousarray(base['dy'][sl])
        if half:
            for k in ('x', 'res', 'dy'):
                d[k] = to_half(d[k])
        out.append(d)
    return out


def _stack(inps, k):
    return np.concatenate([f64(i[k]) for i in inps], 0)


def bn_ranks_rule(inps, spec, mask=None):
    """What every rank holds after the layer, in float64: one dict per rank (the constants and running statistics of X; y, dx, dres
    as row slices; dbeta, dgamma over the rank's own rows).  mask: the ReLU decisions of all rows (default: the rule's own)."""
    p = inps[0]
    lo = np.concatenate([[0], np.cumsum([i['x'].shape[0] for i in inps])]).astype(int)
    x_all = _stack(inps, 'x')
    fwd = bn_forward(x_all, p['gamma'], p['beta'], _stack(inps, 'res') if spec['res'] else None, spec['relu'], (p['rm0'], p['rv0']))
    if mask is None and spec['relu']:
        mask = (fwd['pre'] > 0).astype(np.float64)
    bwd = bn_backward(x_all, p['gamma'], fwd, _stack(inps, 'dy'), mask)
    out = []
    for r in range(len(inps)):
        sl = slice(lo[r], lo[r + 1])
        d = {k: fwd[k] for k in CONSTS}
        d.update(y=fwd['y'][sl], dx=bwd['dx'][sl], dbeta=bwd['g'][sl].sum(0), dgamma=(bwd['g'][sl] * bwd['xhat'][sl]).sum(0))
        if spec['res']:
            d['dres'] = bwd['dres'][sl]
        out.append(d)
    return out


def const_bounds_ranks(x_all, gamma, fwd, world):
    """const_bounds on the union batch with its fp64 depth d = min(N + 4, 288) raised to d + W (every fp64 term is linear in d)."""
    cb = const_bounds(x_all, gamma, fwd)
    d0 = float(min(f64(x_all).shape[0] + 4, F64_DEPTH))
    up = (d0 + world) / d0
    out = {k: cb[k] * up for k in ('_dscale64', '_dshift64')}
    for k in CONSTS:
        if k in cb:
            round_once = 2 * ulp32(fwd[k])
            out[k] = round_once + np.maximum(cb[k] - round_once, 0.0) * up
    return out


def _ranks_grad_rows(sfx, inps, gamma, fwd, bwd, gots, chains, half=False, pgs=1.0):
    """The rows of check() for dbeta_r, dgamma_r, dx_r (names + sfx) of every rank; bwd: bn_backward on the union batch."""
    rows_n = [i['x'].shape[0] for i in inps]
    lo = np.concatenate([[0], np.cumsum(rows_n)]).astype(int)
    total = int(lo[-1])
    c = f64(gamma).shape[0]
    s = float(np.float32(pgs))
    per, sum_db, sum_dg = [], np.zeros(c), np.zeros(c)
    for r, inp in enumerate(inps):
        sl = slice(lo[r], lo[r + 1])
        g, xh = bwd['g'][sl], bwd['xhat'][sl]
        mine = {'g': g, 'xhat': xh, 'dbeta': g.sum(0), 'dgamma': (g * xh).sum(0)}
        if rows_n[r]:
            gb = _grad_bounds(inp['x'], gamma, fwd, mine, chains[r])
            b_db, b_dg = gb['dbeta'], gb['dgamma']
        else:
            b_db, b_dg = np.zeros(c), np.zeros(c)
        sum_db, sum_dg = sum_db + b_db, sum_dg + b_dg
        per.append((mine, b_db, b_dg))
    g, xhat = np.abs(bwd['g']), np.abs(bwd['xhat'])
    mi = np.abs(fwd['mean']) * fwd['invstd']
    gi = np.abs(f64(gamma) * fwd['invstd'])
    gbar, gxbar = np.abs(bwd['dbeta']) / total, np.abs(bwd['dgamma']) / total
    b_dx = gi * (8 * U * (g + gbar + xhat * gxbar + mi * gxbar) + sum_db / total + xhat * sum_dg / total)
    if half:
        b_dx = half_store(bwd['dx'], b_dx)
    rows = []
    for r in range(len(inps)):
        sl = slice(lo[r], lo[r + 1])
        mine, b_db, b_dg = per[r]
        for k, b in (('dbeta', b_db), ('dgamma', b_dg)):
            if k + sfx in gots[r]:
                b = b * s
                if not is_pow2(s):
                    b = b + U * (np.abs(mine[k]) * s + b)
                rows.append(('%s%s[%d]' % (k, sfx, r), gots[r][k + sfx], mine[k] * s, b))
        if 'dx' + sfx in gots[r]:
            rows.append(('dx%s[%d]' % (sfx, r), gots[r]['dx' + sfx], bwd['dx'][sl], b_dx[sl]))
    return rows


def bn_ranks_check(tag, inps, spec, gots, chains, half=False, pgs=1.0, quiet=False):
    """One SyncBN layer over ranks with different rows (see the section's head).  inps: bn_input_ranks(...); spec: res, relu;
    gots[r]: what rank r produced (names as in bn_check / bn_check_half; absent names are not checked); chains[r]: the fp32 chain
    length of the path rank r took.  The ReLU mask is the device's own -- the stacked y > 0, or the stacked 'mask' of a binary16 run
    without a residual -- and must be the rule's outside the borderline elements.  -> (failures, share of borderline elements)."""
    relu, has_res = spec['relu'], spec['res']
    world = len(inps)
    rows_n = [i['x'].shape[0] for i in inps]
    lo = np.concatenate([[0], np.cumsum(rows_n)]).astype(int)
    p = inps[0]
    x_all, dy_all = _stack(inps, 'x'), _stack(inps, 'dy')
    res_all = _stack(inps, 'res') if has_res else None
    if half:
        for i in inps:
            for k in ('x', 'res', 'dy'):
                assert np.array_equal(to_half(i[k]), i[k]), '%s is not binary16' % k
    fwd = bn_forward(x_all, p['gamma'], p['beta'], res_all, relu, (p['rm0'], p['rv0']))
    cb = const_bounds_ranks(x_all, p['gamma'], fwd, world)
    yb = y_bound(x_all, fwd, res_all, cb)
    y_store = half_store(fwd['y'], yb) if half else yb
    rows = []
    for r in range(world):
        rows += [('%s[%d]' % (k, r), gots[r][k], fwd[k], cb[k]) for k in CONSTS if k in gots[r]]
        rows.append(('y[%d]' % r, gots[r]['y'], fwd['y'][lo[r]:lo[r + 1]], y_store[lo[r]:lo[r + 1]]))
    bad, share, mask = [], 0.0, None
    if relu:
        if half and not has_res:
            mask = np.concatenate([np.asarray(g['mask'], dtype=bool).reshape(-1, x_all.shape[1]) for g in gots], 0)
            edge = np.abs(fwd['pre']) <= yb
        else:
            mask = np.concatenate([f64(g['y']) for g in gots], 0) > 0
            edge = np.abs(fwd['pre']) <= yb + (H_TINY if half else 0.0)
        share = float(edge.mean())
        wrong = (mask != (fwd['pre'] > 0)) & ~edge
        if wrong.any():
            bad.append('ReLU mask differs in %d elements that are not borderline' % int(wrong.sum()))
    if any('dx' in g or 'dbeta' in g for g in gots):
        bwd = bn_backward(x_all, p['gamma'], fwd, dy_all, mask.astype(np.float64) if mask is not None else None)
        rows += _ranks_grad_rows('', inps, p['gamma'], fwd, bwd, gots, chains, half, pgs)
        for r in range(world):
            if gots[r].get('dres') is not None:
                rows.append(('dres[%d]' % r, gots[r]['dres'], bwd['dres'][lo[r]:lo[r + 1]], None))
    return check(tag, rows, bad, quiet), share


def bn_ranks_check_half(tag, inps, spec, gots, pgs=1.0, quiet=False):
    """bn_ranks_check for half_train.batch_norm: binary16 x / residual / dy / y / dx / dres, the chain of every rank from its launch
    geometry (chain_len; a rank without rows launches nothing), dbeta / dgamma already multiplied by pgs."""
    c = inps[0]['x'].shape[1]
    chains = [chain_len(i['x'].shape[0], c) if i['x'].shape[0] else 1 for i in inps]
    return bn_ranks_check(tag, inps, spec, gots, chains, half=True, pgs=pgs, quiet=quiet)


def pair_ranks_check(tag, a_inps, b_inps, relu, gots, quiet=False):
    """relu?(BN_a(xa) + BN_b(xb)) over ranks with different rows (functional.batch_norm_pair: the two-stage skeleton on every rank,
    4c + 1 doubles forward, 3c backward).  gots[r]: y, dx_a, dx_b, dbeta_a, ... as in pair_check.  The incoming gradient is a's dy."""
    world = len(a_inps)
    rows_n = [i['x'].shape[0] for i in a_inps]
    lo = np.concatenate([[0], np.cumsum(rows_n)]).astype(int)
    side = {}
    for s, inps in (('a', a_inps), ('b', b_inps)):
        p = inps[0]
        x_all = _stack(inps, 'x')
        f = bn_forward(x_all, p['gamma'], p['beta'], None, False, (p['rm0'], p['rv0']))
        side[s] = (inps, x_all, f, const_bounds_ranks(x_all, p['gamma'], f, world))
    (_, xa, fa, ca), (_, xb, fb, cb) = side['a'], side['b']
    pre = fa['y'] + fb['y']
    y = np.maximum(pre, 0.0) if relu else pre
    yb = 4 * U * (np.abs(xa * fa['scale']) + np.abs(fa['shift']) + np.abs(xb * fb['scale']) + np.abs(fb['shift']) + np.abs(y)) \
        + np.abs(xa) * ca['_dscale64'] + ca['_dshift64'] + np.abs(xb) * cb['_dscale64'] + cb['_dshift64']
    rows = []
    for r in range(world):
        rows.append(('y[%d]' % r, gots[r]['y'], y[lo[r]:lo[r + 1]], yb[lo[r]:lo[r + 1]]))
        for s in 'ab':
            _, _, f, cbs = side[s]
            rows += [('%s_%s[%d]' % (k, s, r), gots[r][k + '_' + s], f[k], cbs[k]) for k in CONSTS if k + '_' + s in gots[r]]
    bad, share, m = [], 0.0, None
    if relu:
        mask = np.concatenate([f64(g['y']) for g in gots], 0) > 0
        edge = np.abs(pre) <= yb
        share = float(edge.mean())
        wrong = (mask != (pre > 0)) & ~edge
        if wrong.any():
            bad.append('ReLU mask differs in %d elements that are not borderline' % int(wrong.sum()))
        m = mask.astype(np.float64)
    dy_all = _stack(a_inps, 'dy')
    for s in 'ab':
        inps, x_all, f, _ = side[s]
        bwd = bn_backward(x_all, inps[0]['gamma'], f, dy_all, m)
        rows += _ranks_grad_rows('_' + s, inps, inps[0]['gamma'], f, bwd, gots, [CHAIN['two_stage']] * world)
    return check(tag, rows, bad, quiet), share


def group_ranks_check(tag, member_inps, gots, quiet=False):
    """The members of a SyncBN group over ranks with different rows: each one the single layer's rule (no ReLU, no residual, the
    two-stage kernels).  member_inps[j]: bn_input_ranks of member j; gots[j][r]: what rank r produced for member j."""
    bad = []
    for j, inps in enumerate(member_inps):
        b, _ = bn_ranks_check('%s[%d]' % (tag, j), inps, {'relu': False, 'res': False}, gots[j], [CHAIN['two_stage']] * len(inps),
                              quiet=quiet)
        bad += ['member %d: %s' % (j, t) for t in b]
    return bad


def rank_chains(rows, small_rows):
    """The fp32 chain length of the path functional._BatchNorm takes on every rank: the small-map half-kernels (1) up to small_rows
    rows, the two-stage kernels (64) above."""
    return [CHAIN['one_launch'] if n <= small_rows else CHAIN['two_stage'] for n in rows]


def _rank_cases():
    cases = {}

    def add(rows, c, res, relu, small_rows=2048, **kw):
        name = 'ranks-' + '+'.join(str(n) for n in rows) + '-c%d-res%d-relu%d' % (c, res, relu) + \
            ('-small%d' % small_rows if small_rows != 2048 else '') + ('-' + kw['note'] if kw.get('note') else '')
        cases[name] = dict(rows=tuple(rows), c=c, res=bool(res), relu=bool(relu), small_rows=small_rows, seed=4000 + len(cases), **kw)
    add((300, 300), 32, 1, 1)                                  # equal counts, different rows
    add((300, 300), 96, 0, 0, window=1, note='window')         # ... rank 1's x a column window of a wider tensor
    add((1, 300), 96, 0, 1)                                    # one rank with a single row
    add((2048, 2049), 32, 1, 1)                                # straddles bn_small_rows(): the half-kernels against the two-stage path
    add((256, 257), 96, 0, 1, small_rows=256)                  # the same straddle at B2M_BN_SMALL_ROWS = 256
    add((0, 257), 32, 1, 1)                                    # a rank without rows
    add((1, 1), 4, 0, 0)                                       # N = 2
    add((65, 1, 4033), 256, 0, 1, tiles=2)                     # three ranks; the large one's sums from per-tile sums
    return cases


RANK_CASES = _rank_cases()
# binary16 (half_train.batch_norm): rows, c, res, relu.  (ReLU with a fused residual: the mask is the stored y's, which the operator
# returns; without one it is the kernel's own recomputation, which only the C entries can be asked for -- tests/test_gpu_norm_half.py)
HALF_RANK_CASES = {'ranks_h-1+300-c512-res1-relu1': ((1, 300), 512, True, True, 4100),
                   'ranks_h-0+257-c32-res1-relu1': ((0, 257), 32, True, True, 4101),
                   'ranks_h-65+1+4033-c96-res0-relu0': ((65, 1, 4033), 96, False, False, 4102)}
# the pair: rows, c, relu
PAIR_RANK_CASES = {'pair_ranks-300+300-c32': ((300, 300), 32, True, 4200), 'pair_ranks-1+300-c96': ((1, 300), 96, True, 4201),
                   'pair_ranks-0+257-c4': ((0, 257), 4, False, 4202)}
# the group: rows; the members' channel counts are GROUP_MEMBERS
GROUP_MEMBERS = (96, 32, 4, 256)
GROUP_RANK_CASES = {'group_ranks-1+300': ((1, 300), 4300), 'group_ranks-300+300': ((300, 300), 4310), 'group_ranks-0+257': ((0, 257), 4320)}


def rank_case_inputs(name):
    s = RANK_CASES[name]
    return bn_input_ranks(s['rows'], s['c'], s['seed'])


def half_rank_case_inputs(name):
    rows, c, _, _, seed = HALF_RANK_CASES[name]
    return bn_input_ranks(rows, c, seed, half=True)


def pair_rank_case_inputs(name):
    rows, c, _, seed = PAIR_RANK_CASES[name]
    a, b = bn_input_ranks(rows, c, seed), bn_input_ranks(rows, c, seed + 50)
    for d in b:
        d['x'] = np.ascontiguousarray(d['x'][:, ::-1])         # another kind (and another spread) meets each column of a
    return a, b


def group_rank_case_inputs(name):
    rows, seed = GROUP_RANK_CASES[name]
    return [bn_input_ranks(rows, c, seed + j) for j, c in enumerate(GROUP_MEMBERS)]


RANK_MISTAKES = ('mean_of_rank_means', 'pooled_within_variance', 'local_count_in_dx', 'local_sums_in_dx', 'unbiased_with_local_n',
                 'count_is_world_times_local', 'param_grads_from_global_sums')


def bn_ranks_emulate(inps, spec, mistake=None, half=False, pgs=1.0):
    """bn_emulate / bn_emulate_h rank by rank: every rank's statistics as sequential fp64 sums down its columns, the packed sums
    (sum x, sum x^2, n_r) added in rank order, the constants rounded once; the backward sums sequential in fp32 on every rank, widened
    and added in rank order; fp32 element arithmetic, binary16 stores for `half`.  -> one dict per rank.  `mistake` (RANK_MISTAKES):
        mean_of_rank_means            the mean is the unweighted mean of the ranks' means
        pooled_within_variance        the variance is the row-weighted mean of the ranks' variances (the spread between ranks is lost)
        local_count_in_dx             dx divides the global sums by the LOCAL row count
        local_sums_in_dx              dx from this rank's sums and row count (a one-rank backward with the global constants)
        unbiased_with_local_n         running_var's unbiased factor from the local row count
        count_is_world_times_local    N = W * n_r
        param_grads_from_global_sums  dbeta, dgamma from the all-reduced sums"""
    f = np.float32
    world = len(inps)
    rows_n = [i['x'].shape[0] for i in inps]
    p = inps[0]
    c = p['x'].shape[1]
    gamma, beta = f64(p['gamma']), f64(p['beta'])
    packs = []
    for i in inps:
        xs = f64(i['x'])
        packs.append((_seq64(xs), _seq64(xs * xs), float(xs.shape[0])))
    s1, s2, cnt = np.zeros(c), np.zeros(c), 0.0
    for a, b, k in packs:
        s1, s2, cnt = s1 + a, s2 + b, cnt + k
    rnd = (lambda a: _round_half(a)) if half else (lambda a: a)
    mom = float(f(MOMENTUM))
    fw = []
    for r, i in enumerate(inps):
        n = rows_n[r]
        tot = float(world * n) if mistake == 'count_is_world_times_local' else cnt
        with np.errstate(divide='ignore', invalid='ignore'):
            m = s1 / tot
            if mistake == 'mean_of_rank_means':
                m = sum(a / k for a, _, k in packs if k) / sum(1 for _, _, k in packs if k)
            var = np.maximum(s2 / tot - m * m, 0.0)
            if mistake == 'pooled_within_variance':
                var = sum(k * np.maximum(b / k - (a / k) ** 2, 0.0) for a, b, k in packs if k) / tot
        nn = float(n) if mistake == 'unbiased_with_local_n' else tot
        unb = var * nn / (nn - 1) if nn > 1 else var
        got = {'running_mean': ((1 - mom) * f64(p['rm0']) + mom * m).astype(f),
               'running_var': ((1 - mom) * f64(p['rv0']) + mom * unb).astype(f)}
        inv = 1.0 / np.sqrt(var + float(f(EPS)))
        mean32, inv32 = m.astype(f), inv.astype(f)
        sc32, sh32 = (gamma * inv).astype(f), (beta - m * gamma * inv).astype(f)
        got.update(mean=mean32, invstd=inv32, scale=sc32, shift=sh32)
        x, dy = i['x'], i['dy']
        v = (f64(x) * f64(sc32) + f64(sh32)).astype(f)                     # an fma: one rounding
        if spec['res']:
            v = v + i['res']
        mask = None
        if spec['relu']:
            y = rnd(np.maximum(v, f(0)))
            w = y if (spec['res'] or not half) else v
            mask = w > 0
            if half and not spec['res']:
                got['mask'] = mask
        else:
            y = rnd(v)
        got['y'] = y
        g = dy * mask.astype(f) if mask is not None else dy
        xh = (x - mean32) * inv32
        fw.append((got, g, xh, _seq32(g), _seq32(g * xh), tot))
        if spec['res']:
            got['dres'] = rnd(g)
    g1, g2 = np.zeros(c), np.zeros(c)
    for _, _, _, a, b, _ in fw:
        g1, g2 = g1 + f64(a), g2 + f64(b)
    out = []
    for r, (got, g, xh, sg, sgx, tot) in enumerate(fw):
        n = rows_n[r]
        a, b, over = g1, g2, tot
        if mistake == 'local_sums_in_dx':
            a, b, over = f64(sg), f64(sgx), float(n)
        if mistake == 'local_count_in_dx':
            over = float(n)
        s = f(pgs)
        if mistake == 'param_grads_from_global_sums':
            got.update(dbeta=g1.astype(f) * s, dgamma=g2.astype(f) * s)
        else:
            got.update(dbeta=sg * s, dgamma=sgx * s)
        with np.errstate(divide='ignore', invalid='ignore'):
            inv_n = f(1.0 / over) if over else f(0)
        got['dx'] = rnd((p['gamma'] * got['invstd']) * (g - a.astype(f) * inv_n - xh * (b.astype(f) * inv_n)))
        out.append(got)
    return out


def pair_ranks_emulate(a_inps, b_inps, relu):
    """pair_emulate over ranks: two bn_ranks_emulate forwards, one fp32 add, the backward sums per rank, added in rank order."""
    f = np.float32
    plain = {'res': False, 'relu': False}
    ea, eb = bn_ranks_emulate(a_inps, plain), bn_ranks_emulate(b_inps, plain)
    world = len(a_inps)
    total = float(sum(i['x'].shape[0] for i in a_inps))
    gots, keep = [], []
    for r in range(world):
        y = ea[r]['y'] + eb[r]['y']
        mask = (y > 0).astype(f) if relu else np.ones_like(y)
        got = {'y': np.maximum(y, f(0)) if relu else y}
        g = a_inps[r]['dy'] * mask
        loc = {}
        for s, inps, e in (('a', a_inps, ea), ('b', b_inps, eb)):
            xh = (inps[r]['x'] - e[r]['mean']) * e[r]['invstd']
            loc[s] = (xh, _seq32(g), _seq32(g * xh))
            got.update({'dbeta_' + s: loc[s][1], 'dgamma_' + s: loc[s][2]})
            got.update({k + '_' + s: e[r][k] for k in CONSTS})
        gots.append(got)
        keep.append((g, loc))
    for s, inps, e in (('a', a_inps, ea), ('b', b_inps, eb)):
        g1 = sum(f64(k[1][s][1]) for k in keep)
        g2 = sum(f64(k[1][s][2]) for k in keep)
        inv_n = f(1.0 / total)
        for r in range(world):
            g, loc = keep[r]
            gots[r]['dx_' + s] = (inps[r]['gamma'] * e[r]['invstd']) * (g - g1.astype(f) * inv_n - loc[s][0] * (g2.astype(f) * inv_n))
    return gots
