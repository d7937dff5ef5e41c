"""Named cases for the byte-colour rule (tests/_colour8_rule.py), shared by tests/test_colour8_rule.py (CPU: each deliberate
mistake of the rule must change its named case) and tests/test_gpu_colour8.py (b2m_aug_colour8 / b2m_aug_brightness, bit for
bit).  A case is plain data: the colours, the product mode, an optional brightness beta, optional HSV shifts and the Mix3D numbers
(None: the brightness stage alone).  Each case asserts, when it is built, the predicate that says which edge it reaches."""
from types import SimpleNamespace

import numpy as np

import _colour8_rule as R

IDENTITY = (1.0, 0.0, (0.0, 0.0, 0.0))              # alpha, beta, shifts: the three RGB tables are the identity


def base_colours():
    """The 8 corners, the greys, the colours whose largest channel is shared by two, and 2 600 seeded colours: (3 164, 3) fp64
    in [0, 1].  Every byte value occurs in every channel."""
    rng = np.random.default_rng(20240607)
    corners = np.array([[(k >> 2) & 1, (k >> 1) & 1, k & 1] for k in range(8)], np.float64)
    greys = np.repeat((np.arange(256) + 0.5)[:, None] / 255.0, 3, 1)
    k = (np.arange(100) * 2.5 + 3.5)
    ties = np.concatenate([np.stack([k, k, k * 0.4], 1), np.stack([k * 0.3, k, k], 1), np.stack([k, k * 0.7, k], 1)]) / 255.0
    return np.concatenate([corners, greys, ties, rng.random((2600, 3))])


def _case(colors, hsv=None, mix=IDENTITY, f32=False, beta=None):
    return SimpleNamespace(colors=np.ascontiguousarray(colors, np.float64), hsv=hsv, mix=mix, f32=f32, beta=beta)


# ----------------------------------------------------------------------------- table edges
_BC = {'bc:%g,%g' % (a, b): dict(mix=(a, b, (0.0, 0.0, 0.0))) for a in (1.0, 0.8, 1.2) for b in (0.0, 0.2, -0.2)}
TABLE_PARAMS = {
    # each single shift with the other two exactly 0
    'hue:+50': dict(hsv=(50.0, 0.0, 0.0)), 'hue:-50': dict(hsv=(-50.0, 0.0, 0.0)), 'hue:+1e-9': dict(hsv=(1e-9, 0.0, 0.0)),
    'hue:-1e-9': dict(hsv=(-1e-9, 0.0, 0.0)), 'hue:10.7': dict(hsv=(10.7, 0.0, 0.0)), 'hue:179.5': dict(hsv=(179.5, 0.0, 0.0)),
    'sat:+60': dict(hsv=(0.0, 60.0, 0.0)), 'sat:-60': dict(hsv=(0.0, -60.0, 0.0)), 'sat:12.5': dict(hsv=(0.0, 12.5, 0.0)),
    'val:+50': dict(hsv=(0.0, 0.0, 50.0)), 'val:-50': dict(hsv=(0.0, 0.0, -50.0)), 'val:-7.25': dict(hsv=(0.0, 0.0, -7.25)),
    'hsv:all': dict(hsv=(-50.0, 60.0, -50.0)), 'hsv:zero': dict(hsv=(0.0, 0.0, 0.0)),
    **_BC,
    'shift:+20': dict(mix=(1.0, 0.0, (20.0, 20.0, 20.0))), 'shift:-20': dict(mix=(1.0, 0.0, (-20.0, -20.0, -20.0))),
    'shift:3.3': dict(mix=(1.0, 0.0, (3.3, 3.3, 3.3))), 'shift:unequal': dict(mix=(1.0, 0.0, (20.0, -20.0, -0.75))),
    'mix:all': dict(mix=(0.8, 0.2, (20.0, -20.0, 3.3))),
    'all': dict(hsv=(10.7, -12.5, 7.25), mix=(1.2, -0.2, (-20.0, 3.3, 20.0))),
}
TABLE_CASES = tuple(TABLE_PARAMS)


def table_case(name):
    c = _case(base_colours(), **TABLE_PARAMS[name])
    if name == 'hue:-1e-9':
        assert R.hsv_tables(*c.hsv)[0][0] == 179                        # the mod is taken first, the cast truncates
    if name == 'hue:+1e-9':
        assert np.array_equal(R.hsv_tables(*c.hsv)[0][:180], np.arange(180))
    if name == 'hsv:zero':
        assert all(t is None for t in R.hsv_tables(*c.hsv))
    return c


# ----------------------------------------------------------------------------- quantise edges
def quant_values():
    """Per-channel values at the edges of the quantise: the k / 255, their fp64 neighbours below (where rounding the COLOUR to float32
    first lifts the product over k), half-way values, both zeros, the clamps and NaN."""
    k = np.arange(256) / 255.0
    return np.concatenate([[0.0, -0.0, 1.0, 1.0 + 2.0 ** -52, 1.0 + 2.0 ** -23, -2.0 ** -1074, -2.0 ** -149, -1e-3, -1.0, 2.0, 1e300,
                            np.inf, -np.inf, np.nan], k, np.nextafter(k[1:], 0.0), (np.arange(256) + 0.5) / 255.0])


QUANT_CASES = ('quant:f64', 'quant:f32')


def quant_case(name):
    f32 = name == 'quant:f32'
    v = quant_values()
    i = np.arange(len(v))
    c = _case(np.stack([v, v[(i + 7) % len(v)], v[(i + 13) % len(v)]], 1), f32=f32)
    with np.errstate(invalid='ignore', over='ignore'):
        q64, q32 = R.quantise(v, False), R.quantise(v, True)
        assert (q32 != q64).sum() >= 100                                 # nextafter(k / 255, 0) rounds to a float32 above k / 255
        assert (R.quantise(v, False, 'quant_round') != q64).sum() >= 100
    return c


# ----------------------------------------------------------------------------- brightness at its clip edges
BRIGHT_CASES = ('bright:+0.2', 'bright:-0.2', 'bright:+0.2:hue', 'bright:-0.2:mix3d')


def bright_case(name):
    beta = 0.2 if '+' in name else -0.2
    b32 = np.float32(beta)
    f = np.float32
    edge = []
    for target in (f(0), f(1)):
        x = target - b32                                                 # float32: lands on, just under and just over the clip edge
        edge += [x, np.nextafter(x, f(-9)), np.nextafter(x, f(9))]
    rng = np.random.default_rng(5)
    v = np.concatenate([np.array(edge, np.float64), [0.0, 1.0, -0.0, 0.5, np.nan, 7.0, -7.0, 0.123456789012345],
                        rng.random(286)])                                # fp64 colours: the stage rounds them to float32 first
    i = np.arange(len(v))
    col = np.stack([v, v[(i + 5) % len(v)], v[(i + 11) % len(v)]], 1)
    got = R.brightness(col, beta)
    assert (got == 0).any() and (got == 1).any() and np.isnan(got).any()
    if name.endswith(':hue'):
        return _case(col, hsv=(10.7, -12.5, 7.25), mix=(1.2, -0.2, (-20.0, 3.3, 20.0)), f32=True, beta=beta)
    if name.endswith(':mix3d'):
        return _case(col, mix=(0.8, 0.2, (20.0, -20.0, 3.3)), f32=True, beta=beta)
    return _case(col, mix=None, beta=beta)


# ----------------------------------------------------------------------------- sizes, and every colour once
SIZES = (1, 63, 64, 65, 255, 256, 257, 4097)


def size_case(n):
    rng = np.random.default_rng(n)
    return _case(rng.random((n, 3)), hsv=(10.7, -12.5, 7.25), mix=(1.2, -0.2, (-20.0, 3.3, 20.0)))


def every_colour_case():
    """All 2^24 colours (k + 0.5) / 255 per channel (the truncation is unambiguous), hue shift 1e-9 (the identity on valid hues,
    which forces both conversions), identity RGB tables."""
    k = np.arange(1 << 24, dtype=np.uint32)
    col = (np.stack([k >> 16, (k >> 8) & 255, k & 255], -1).astype(np.float64) + 0.5) / 255.0
    return _case(col, hsv=(1e-9, 0.0, 0.0))


def case(name):
    if name in TABLE_PARAMS:
        return table_case(name)
    if name in QUANT_CASES:
        return quant_case(name)
    if name in BRIGHT_CASES:
        return bright_case(name)
    raise KeyError(name)


def tables(c, mistake=None):
    """The rule's tables of a case: ((hue, sat, val) with None for an absent one, (r, g, b), (mean, den))."""
    hsv = R.hsv_tables(*c.hsv, mistake) if c.hsv is not None else (None, None, None)
    return hsv, R.rgb_tables(*c.mix, mistake), R.norm_rows(mistake)


def want(c, mistake=None):
    """The rule's result of a case, as the fp64 array the entry leaves."""
    if c.mix is None:
        return R.brightness(c.colors, c.beta).astype(np.float64)
    hsv, rgb, rows = tables(c, mistake)
    return R.chain(c.colors, c.f32, hsv, rgb, rows, c.beta, mistake).astype(np.float64)
