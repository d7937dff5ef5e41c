"""GPU: b2m_aug_colour8 / b2m_aug_brightness (csrc/augment.hip) and the byte-colour steps of augment.colour_ / augment_scenes, bit for
bit against the rule of tests/_colour8_rule.py (profiles/colour8_rule.md) on the cases of tests/_colour8_cases.py -- which
tests/test_colour8_rule.py shows to have teeth on the CPU.  No tolerances anywhere.

The entries are called DIRECTLY through _lib.call with the RULE's tables, and through augment.py with its own.  The colours sit
inside poisoned padding, so "writes only its n rows" is checked with every call."""
import ctypes

import numpy as np
import pytest
import torch

import _colour8_cases as C
import _colour8_rule as R
from _augment_rule import bits, same_bits

pytestmark = pytest.mark.gpu

PAD = 64
POISON = -777.25


def _L():
    from box2mask_amd import _lib
    return _lib


class Colours:
    """The (n,3) colours an entry updates in place, inside PAD poisoned doubles on either side."""

    def __init__(self, col):
        col = np.ascontiguousarray(col, np.float64)
        self.shape = col.shape
        self.full = torch.full((col.size + 2 * PAD,), POISON, dtype=torch.float64, device='cuda')
        self.full[PAD:PAD + col.size] = torch.from_numpy(col.reshape(-1)).cuda()
        self.ptr = self.full[PAD:].data_ptr()

    def get(self):
        f = self.full.cpu().numpy()
        assert (f[:PAD] == POISON).all() and (f[-PAD:] == POISON).all(), 'written outside the colours'
        return f[PAD:-PAD].reshape(self.shape)


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _same(got, want, tag):
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, got.shape)
    if not same_bits(got, want):
        bad = np.nonzero((bits(got) != bits(np.ascontiguousarray(want))).reshape(-1))[0]
        raise AssertionError('%s: %d of %d elements differ in their bits; first at %s: got %r want %r'
                             % (tag, len(bad), got.size, bad[:4], got.reshape(-1)[bad[:4]], want.reshape(-1)[bad[:4]]))


def _args(c):
    """(flags, beta, the eight host arrays in the entry's order) of a case, from the RULE's tables."""
    hsv, rgb, (mean, den) = C.tables(c)
    arrays = [None if t is None else np.ascontiguousarray(t, np.uint8) for t in hsv + rgb] + [mean, den]
    return (1 if c.f32 else 0) | (2 if c.beta is not None else 0), float(c.beta or 0.0), arrays


def _entry(c, n=None):
    col = Colours(c.colors)
    n = len(c.colors) if n is None else n
    if c.mix is None:
        _L().call('b2m_aug_brightness', col.ptr, n, float(c.beta))
    else:
        flags, beta, arrays = _args(c)
        _L().call('b2m_aug_colour8', col.ptr, n, flags, beta, *[_p(a) for a in arrays])
    return col.get()


# ----------------------------------------------------------------------------- 1. every colour once
def test_every_colour_once():
    c = C.every_colour_case()
    hue = R.hsv_tables(*c.hsv)[0]
    assert np.array_equal(hue[:180], np.arange(180)) and R.hsv_tables(*c.hsv)[1:] == (None, None)
    u8 = R.quantise(c.colors)
    k = np.arange(1 << 24, dtype=np.uint32)
    assert np.array_equal(u8, np.stack([k >> 16, (k >> 8) & 255, k & 255], -1).astype(np.uint8))
    want = C.want(c)
    assert (R.hsv_to_rgb8(R.rgb_to_hsv8(u8[::257])) != u8[::257]).any()              # both conversions are forced, and seen
    _same(_entry(c), want, 'every colour')


# ----------------------------------------------------------------------------- 2. table edges, 3. quantise edges and the brightness stage
@pytest.fixture(scope='module')
def results():
    return {}


@pytest.mark.parametrize('name', C.TABLE_CASES + C.QUANT_CASES + C.BRIGHT_CASES)
def test_case(name, results):
    c = C.case(name)
    got = _entry(c)
    _same(got, C.want(c), name)
    results[name] = got


def test_quantise_modes_differ_and_clamp():
    a, b = C.quant_case('quant:f64'), C.quant_case('quant:f32')
    assert same_bits(a.colors, b.colors)
    ga, gb = _entry(a), _entry(b)
    assert (bits(ga) != bits(gb)).sum() >= 100
    mean, den = R.norm_rows()
    nan = np.isnan(a.colors)
    for g in (ga, gb):
        u8 = np.rint(g / den.astype(np.float64) + mean.astype(np.float64))
        assert (u8[nan] == 0).all() and (u8[a.colors < 0] == 0).all() and (u8[a.colors > 1] == 255).all()


# ----------------------------------------------------------------------------- 4. sizes
@pytest.mark.parametrize('n', C.SIZES)
def test_sizes_and_rows_beyond_n(n):
    c = C.size_case(n + 37)
    got = _entry(c, n)
    want = C.want(c)
    _same(got[:n], want[:n], 'n = %d' % n)
    _same(got[n:], c.colors[n:], 'rows beyond n = %d' % n)
    b = C._case(c.colors, mix=None, beta=-0.3)
    got = _entry(b, n)
    _same(got[:n], C.want(b)[:n], 'brightness, n = %d' % n)
    _same(got[n:], c.colors[n:], 'brightness, rows beyond n = %d' % n)


# ----------------------------------------------------------------------------- 5. refusals, repeatability, no conversion
def test_refusals():
    L = _L()
    lib = L.load()
    err = lambda: lib.b2m_last_error().decode()
    c = C.table_case('all')
    flags, beta, arrays = _args(c)
    col = Colours(c.colors[:50])
    ptrs = [_p(a) for a in arrays]

    def refused(word, colors=col.ptr, n=50, flags=flags, ptrs=ptrs):
        assert lib.b2m_aug_colour8(colors, n, flags, beta, *ptrs, None) < 0 and word in err(), (word, err())

    refused('NULL', colors=None)
    refused('positive', n=0)
    refused('positive', n=-3)
    refused('flags', flags=4)
    refused('flags', flags=-1)
    for k in (3, 4, 5):
        refused('RGB tables', ptrs=ptrs[:k] + [None] + ptrs[k + 1:])
    for k in (6, 7):
        refused('normalisation', ptrs=ptrs[:k] + [None] + ptrs[k + 1:])
    assert lib.b2m_aug_brightness(None, 50, 0.1, None) < 0 and 'NULL' in err()
    assert lib.b2m_aug_brightness(col.ptr, 0, 0.1, None) < 0 and 'positive' in err()
    with pytest.raises(L.B2MError, match='RGB tables'):
        L.call('b2m_aug_colour8', col.ptr, 50, flags, beta, *ptrs[:3], None, None, None, *ptrs[6:])
    torch.cuda.synchronize()
    _same(col.get(), c.colors[:50], 'a refused call writes nothing')


def test_repeat_gives_the_same_bits(results):
    for name in ('all', 'hsv:all', 'bright:+0.2:hue'):
        first = results[name] if name in results else _entry(C.case(name))
        _same(_entry(C.case(name)), first, name + ' (second run)')


def test_no_hsv_table_means_no_conversion():
    c = C.table_case('mix:all')
    assert c.hsv is None
    got = _entry(c)
    _same(got, R.mix3d_colour(c.colors, *c.mix).astype(np.float64), 'the Mix3D chain')
    # with every table present the same numbers go through both conversions, which are not the identity
    forced = C._case(c.colors, hsv=(1e-9, 0.0, 0.0), mix=c.mix)
    assert (bits(_entry(forced)) != bits(got)).any()
    # hsv:zero -- all three shifts 0 -- is the same call
    z = C._case(c.colors, hsv=(0.0, 0.0, 0.0), mix=c.mix)
    _same(_entry(z), got, 'zero shifts')


# ----------------------------------------------------------------------------- 6. through the public path
def _scene(seed, n):
    rng = np.random.default_rng(seed)
    nrm = rng.standard_normal((n, 3))
    return {'name': 'scene%d' % seed, 'positions': rng.random((n, 3)) * [4.0, 3.0, 2.0], 'colors': rng.random((n, 3)),
            'normals': nrm / np.linalg.norm(nrm, axis=1, keepdims=True), 'segments': rng.integers(0, 40, n)}


PUBLIC = {'hue': dict(apply_hue_aug=True), 'mix3d': dict(mix_3d_color_aug=True),
          'brightness+hue': dict(apply_hue_aug=True, random_brightness=[1.0, 0.2]),
          'brightness': dict(random_brightness=[1.0, 0.2])}


@pytest.mark.parametrize('which', sorted(PUBLIC))
def test_augment_scenes_applies_the_rule(which):
    from box2mask_amd import augment, prepare
    from box2mask_amd.config import scannet_config
    cfg = scannet_config(augmentation=True, rotation_90_aug=True, flipping_aug=0.5, scaling_aug=[1, .8, 1.2],
                         chromatic_auto_contrast=1.0, chromatic_translation=[1.0, 0.1], color_jittering_aug=[1.0, 0.05],
                         **PUBLIC[which])
    rng = np.random.default_rng(11)
    scenes = [_scene(1, 1000), _scene(2, 1037)]
    params = [augment.draw_params(cfg, generator=rng, byte_colour=True) for _ in scenes]
    byte = ('brightness', 'mix3d', 'hue')
    older = []
    for p in params:
        assert [s[0] for s in p.colour if s[0] in byte] == which.split('+')
        older.append(augment.SceneAugment(geometric=list(p.geometric), colour=[s for s in p.colour if s[0] not in byte]))
        assert len(older[-1].colour) >= 2 and p.geometric
    got = augment.augment_scenes(scenes, params)
    base = augment.augment_scenes(scenes, older)                               # today's path: the older steps alone
    for g, b, p, src in zip(got, base, params, scenes):
        for key in ('positions', 'normals'):
            _same(g[key].cpu().numpy(), b[key].cpu().numpy(), key)
        steps = [s for s in p.colour if s[0] in byte]
        want = R.colour_steps(b['colors'].cpu().numpy(), steps)
        col = g['colors'].cpu().numpy()
        _same(col, want, which)
        assert same_bits(col, col.astype(np.float32).astype(np.float64))
        if which != 'brightness':
            assert col.min() < 0                                                # normalised: no longer in [0, 1]
        assert np.array_equal(src['colors'], _scene(int(src['name'][5:]), len(col))['colors']), 'the inputs are not written'
    # the voxelisation takes the normalised colours as they are: its colour features are these float32 values
    items = prepare.voxelize_scenes(got, 0.02)
    for item, g in zip(items, got):
        feats = item['vox_features'].cpu().numpy()
        col = g['colors'].cpu().numpy()[item['point2vox'].cpu().numpy()]
        assert feats.dtype == np.float32 and same_bits(feats[:, :3], col.astype(np.float32))
        assert same_bits(feats[:, :3].astype(np.float64), col)


def test_colour_order_and_exclusion():
    from box2mask_amd import augment
    col = torch.rand(10, 3, dtype=torch.float64, device='cuda')
    mix = (1.0, 0.1, (1.0, 2.0, 3.0))
    with pytest.raises(ValueError, match='reference order'):
        augment.colour_(col, [('mix3d',) + mix, ('brightness', 0.1)])
    with pytest.raises(ValueError, match='reference order'):
        augment.colour_(col, [('hue', 1.0, 2.0, 3.0) + mix, ('translation', np.zeros(3))])
    with pytest.raises(ValueError, match='mix3d and hue'):
        augment.colour_(col, [('mix3d',) + mix, ('hue', 1.0, 2.0, 3.0) + mix])
