"""CPU: the byte-colour rule (tests/_colour8_rule.py, profiles/colour8_rule.md) against an independent colour-space implementation
(matplotlib) within derived bounds, its table builders against literal loops, draw_params(..., byte_colour=True), and the cases of
tests/_colour8_cases.py shown to have teeth: each deliberate mistake of the rule changes its named case.

The bounds of the enumerations are derived, not tuned: half a code value of final rounding, plus the rounding of the divide tables
(0.5 * 1275 / 4096 for hue, whose numerator reaches 5 * 255, and 0.5 * 255 / 4096 for saturation).  Measured maxima: hue 0.640,
saturation 0.522, value 0, HSV->RGB 0.500."""
import math

import numpy as np
import pytest

import _colour8_cases as C
import _colour8_rule as R
from _augment_rule import same_bits
from box2mask_amd import augment
from box2mask_amd.config import scannet_config

HUE_BOUND = 0.66          # 0.5 + 0.5 * 1275 / 4096 = 0.6556...
SAT_BOUND = 0.54          # 0.5 + 0.5 * 255 / 4096 = 0.5311...
RGB_BOUND = 0.501         # 0.5 of final rounding, plus fp32 arithmetic


# ----------------------------------------------------------------------------- the conversions against matplotlib
@pytest.fixture(scope='module')
def every_rgb():
    k = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([k >> 16, (k >> 8) & 255, k & 255], -1).astype(np.uint8)
    return rgb, R.rgb_to_hsv8(rgb)


def test_rgb_to_hsv_on_every_colour_against_matplotlib(every_rgb):
    import matplotlib.colors as mc
    rgb, hsv = every_rgb
    assert hsv.dtype == np.uint8 and int(hsv[:, 0].max()) == 179
    ref = mc.rgb_to_hsv(rgb.astype(np.float64) / 255.0)
    dh = np.abs(hsv[:, 0].astype(np.float64) - ref[:, 0] * 180.0)
    dh = np.minimum(dh, 180.0 - dh)
    ds = np.abs(hsv[:, 1].astype(np.float64) - ref[:, 1] * 255.0)
    print('max |hue| %.4f, max |sat| %.4f' % (dh.max(), ds.max()))
    assert dh.max() <= HUE_BOUND
    assert ds.max() <= SAT_BOUND
    assert np.array_equal(hsv[:, 2], rgb.max(1))
    assert np.array_equal(hsv[:, 2].astype(np.float64), np.rint(ref[:, 2] * 255.0))


def test_hsv_to_rgb_on_every_input_against_matplotlib():
    import matplotlib.colors as mc
    k = np.arange(180 * 256 * 256, dtype=np.uint32)
    hsv = np.stack([k >> 16, (k >> 8) & 255, k & 255], -1).astype(np.uint8)
    out = R.hsv_to_rgb8(hsv)
    ref = mc.hsv_to_rgb(hsv.astype(np.float64) / np.array([180.0, 255.0, 255.0])) * 255.0
    err = np.abs(out.astype(np.float64) - ref).max()
    print('max |rgb| %.6f' % err)
    assert out.dtype == np.uint8 and err <= RGB_BOUND


def test_hues_outside_the_range_wrap():
    """A hue table handed to the entry directly may hold 180..255: fmodf brings them back, and no sector leaves 0..5."""
    hsv = np.stack(np.meshgrid(np.arange(180, 256), [0, 1, 128, 255], [0, 77, 255], indexing='ij'), -1).reshape(-1, 3).astype(np.uint8)
    low = hsv.copy()
    low[:, 0] -= 180
    assert np.abs(R.hsv_to_rgb8(hsv).astype(int) - R.hsv_to_rgb8(low).astype(int)).max() <= 1


# ----------------------------------------------------------------------------- the table builders against literal loops
def _trunc8(x):
    assert 0 <= x < 256
    return int(x)


@pytest.mark.parametrize('shifts', [(50.0, 60.0, 50.0), (-50.0, -60.0, -50.0), (1e-9, 0.0, 12.5), (-1e-9, -7.25, 0.0), (10.7, 0.0, 0.0),
                                    (179.5, 59.999, -49.999), (0.0, 0.0, 0.0)])
def test_hsv_tables_against_loops(shifts):
    for build in (R.hsv_tables, augment.hsv_tables):
        hue, sat, val = build(*shifts)
        for tab, s in zip((hue, sat, val), shifts):
            assert (tab is None) == (s == 0)
        if hue is not None:
            assert hue.dtype == np.uint8 and list(hue) == [_trunc8(math.fmod(i + shifts[0], 180) + (180 if i + shifts[0] < 0 else 0))
                                                           for i in range(256)]
        for tab, s in ((sat, shifts[1]), (val, shifts[2])):
            if tab is not None:
                assert tab.dtype == np.uint8 and list(tab) == [_trunc8(min(max(i + s, 0.0), 255.0)) for i in range(256)]
    assert R.hsv_tables(-1e-9, 0, 0)[0][0] == 179


@pytest.mark.parametrize('alpha', [1.0, 0.8, 1.2, 0.93217])
@pytest.mark.parametrize('beta', [0.0, 0.2, -0.2, 0.04567])
def test_rgb_tables_against_loops(alpha, beta):
    f = np.float32
    shifts = (20.0, -20.0, 3.3)
    bc = []
    for i in range(256):
        x = f(i)
        if alpha != 1:
            x = x * f(alpha)
        if beta != 0:
            x = x + f(beta * 255)
        bc.append(_trunc8(min(max(x, f(0)), f(255))))
    assert list(R.brightness_contrast_table(alpha, beta)) == bc
    for build in (R.rgb_tables, augment.rgb_tables):
        tabs = build(alpha, beta, shifts)
        for tab, s in zip(tabs, shifts):
            assert tab.dtype == np.uint8 and tab.flags.c_contiguous
            assert list(tab) == [_trunc8(min(max(f(bc[i]) + f(s), f(0)), f(255))) for i in range(256)]


def test_normalisation_rows():
    for mean, den in (R.norm_rows(), augment.norm_rows()):
        assert mean.dtype == np.float32 and den.dtype == np.float32
        for k in range(3):
            assert mean[k] == np.float32(R.COLOR_MEAN[k]) * np.float32(255)
            assert den[k] == np.float32(1) / (np.float32(R.COLOR_STD[k]) * np.float32(255))
    assert augment.COLOR_MEAN == R.COLOR_MEAN and augment.COLOR_STD == R.COLOR_STD
    u8 = np.arange(256, dtype=np.uint8)[:, None].repeat(3, 1)
    out = R.normalise(u8)
    ref = (u8 / 255.0 - np.array(R.COLOR_MEAN)) / np.array(R.COLOR_STD)
    assert out.dtype == np.float32 and np.abs(out - ref).max() < 4e-6 and out.min() < -1 and out.max() > 2


def test_the_product_tables_equal_the_rule_on_every_case():
    for name in C.TABLE_CASES:
        c = C.table_case(name)
        hsv, rgb, rows = C.tables(c)
        mine = (augment.hsv_tables(*c.hsv) if c.hsv is not None else (None,) * 3) + augment.rgb_tables(*c.mix)
        for a, b in zip(hsv + rgb, mine):
            assert (a is None and b is None) or np.array_equal(a, b), name


# ----------------------------------------------------------------------------- draw_params(..., byte_colour=True)
def _byte_steps(params):
    return [s for s in params.colour if s[0] in ('brightness', 'mix3d', 'hue')]


def test_draws_lie_in_their_ranges_and_both_mix3d_parts_are_always_there():
    rng = np.random.default_rng(0)
    cfg = scannet_config(augmentation=True, apply_hue_aug=True, random_brightness=[0.5, 0.2], chromatic_auto_contrast=0.2,
                         chromatic_translation=[0.95, 0.1], color_jittering_aug=[0.95, 0.05])
    n, n_bright = 400, 0
    seen = np.zeros((8, 2))
    for _ in range(n):
        p = augment.draw_params(cfg, generator=rng, byte_colour=True)
        kinds = [s[0] for s in p.colour]
        order = [augment._COLOUR_ORDER.index(k) for k in kinds]
        assert order == sorted(set(order)) and kinds[-1] == 'hue'
        steps = _byte_steps(p)
        n_bright += steps[0][0] == 'brightness'
        if steps[0][0] == 'brightness':
            assert type(steps[0][1]) is float and -0.2 <= steps[0][1] <= 0.2
        hue = steps[-1]
        assert len(hue) == 7 and len(hue[6]) == 3
        nums = list(hue[1:6]) + list(hue[6])
        assert all(type(x) is float for x in nums)
        lims = [(-50, 50), (-60, 60), (-50, 50), (0.8, 1.2), (-0.2, 0.2)] + [(-20, 20)] * 3
        for k, (x, (lo, hi)) in enumerate(zip(nums, lims)):
            assert lo <= x <= hi
            seen[k] = [min(seen[k, 0], (x - lo) / (hi - lo) - 0.5), max(seen[k, 1], (x - lo) / (hi - lo) - 0.5)]
    assert abs(n_bright / n - 0.5) < 0.1                               # 4 sigma of a fair coin over 400 draws
    assert (seen[:, 0] < -0.45).all() and (seen[:, 1] > 0.45).all()    # the whole range is used
    mix = augment.draw_params(scannet_config(augmentation=True, mix_3d_color_aug=True), generator=rng, byte_colour=True).colour[-1]
    assert mix[0] == 'mix3d' and len(mix) == 4 and 0.8 <= mix[1] <= 1.2 and -0.2 <= mix[2] <= 0.2 and len(mix[3]) == 3


def test_the_reference_scannet_flags_are_accepted():
    # configs/scannet.txt:32-37 as scannet_config restates them
    cfg = scannet_config(augmentation=True, rotation_90_aug=True, flipping_aug=0.5, scaling_aug=[1, .8, 1.2], apply_hue_aug=True)
    p = augment.draw_params(cfg, generator=np.random.default_rng(1), byte_colour=True)
    assert [s[0] for s in p.colour] == ['hue']
    with pytest.raises(NotImplementedError, match='byte_colour'):
        augment.draw_params(cfg, generator=np.random.default_rng(1))


def test_mix3d_with_hue_is_refused_and_nothing_is_drawn_without_augmentation():
    with pytest.raises(ValueError, match='mix_3d_color_aug.*apply_hue_aug'):
        augment.draw_params(scannet_config(augmentation=True, mix_3d_color_aug=True, apply_hue_aug=True), byte_colour=True)
    rng = np.random.default_rng(3)
    state = rng.bit_generator.state
    p = augment.draw_params(scannet_config(augmentation=False, apply_hue_aug=True, random_brightness=[1.0, 0.2]), generator=rng,
                            byte_colour=True)
    assert p.colour == [] and p.geometric == [] and rng.bit_generator.state == state
    # byte_colour draws nothing new when none of the three fields is set: the same stream as before
    a = augment.draw_params(scannet_config(augmentation=True), generator=np.random.default_rng(4))
    b = augment.draw_params(scannet_config(augmentation=True), generator=np.random.default_rng(4), byte_colour=True)
    assert repr(a) == repr(b)


# ----------------------------------------------------------------------------- the chains are the reference's statements
def test_chains_are_quantise_tables_normalise():
    col = C.base_colours()
    u8 = (col * 255).astype(np.uint8)
    assert np.array_equal(R.quantise(col), u8)
    mix = (0.8, 0.2, (20.0, -20.0, 3.3))
    want = R.normalise(R.apply_rgb_tables(u8, R.rgb_tables(*mix)))
    assert same_bits(R.mix3d_colour(col, *mix), want)
    hued = R.hue_step(u8, 10.7, -12.5, 7.25)
    assert (hued != u8).any()
    assert same_bits(R.hue_colour(col, 10.7, -12.5, 7.25, *mix), R.normalise(R.apply_rgb_tables(hued, R.rgb_tables(*mix))))
    assert R.hue_step(u8, 0.0, 0.0, 0.0) is u8                         # all three shifts zero: skipped entirely
    b = R.brightness(col, 0.1)
    assert b.dtype == np.float32 and same_bits(R.quantise(b, True), (b * 255).astype(np.uint8))
    steps = [('brightness', 0.1), ('hue', 10.7, -12.5, 7.25) + mix]
    assert same_bits(R.colour_steps(col, steps), R.hue_colour(b, 10.7, -12.5, 7.25, *mix, f32_product=True).astype(np.float64))


# ----------------------------------------------------------------------------- the deliberate mistakes
MUST_FAIL = {
    'quant_round': 'quant:f64', 'hue_mod_256': 'hue:-50', 'rgb2hsv_no_2048': 'hue:+1e-9',
    'rgb2hsv_no_wrap': 'hue:-1e-9', 'hsv2rgb_rows_swapped': 'hue:10.7', 'mix3d_shift_first': 'mix:all', 'norm_f64': 'bc:1,0',
    'norm_mean_unscaled': 'bc:1,0', 'hue_zero_shift_table': 'hsv:zero',
}
# Mistakes of the issue's list that change NO output on the whole domain (profiles/colour8_rule.md says why): no case can catch them.
NO_EFFECT = ('rgb2hsv_g_first', 'hsv2rgb_no_grey', 'quant_f64_product')


def test_the_mistake_table_is_complete():
    assert set(MUST_FAIL) | set(NO_EFFECT) == set(R.MISTAKES) and len(R.MISTAKES) == 12
    assert set(MUST_FAIL.values()) <= set(C.TABLE_CASES + C.QUANT_CASES + C.BRIGHT_CASES)


@pytest.mark.parametrize('mistake', sorted(MUST_FAIL))
def test_every_mistake_changes_its_named_case(mistake):
    c = C.case(MUST_FAIL[mistake])
    right = C.want(c)
    assert same_bits(right, C.want(c)), 'the rule is a function of its inputs'
    assert not same_bits(right, C.want(c, mistake)), (mistake, MUST_FAIL[mistake])


def test_three_listed_mistakes_change_nothing_anywhere(every_rgb):
    """`v == g` tested before `v == r` differs only where r == g == v, and there g - b == b - r + 2d == d.  Without the s == 0 branch
    the table is v, v(1 - 0), v(1 - 0 h), v(1 - 0 (1 - h)): v four times, for every finite h.  And the fp64 product of a FLOAT32
    colour truncates like its fp32 product: the float32 numbers below k / 255 lie at least k 2^-24 / 255 below it, so 255 c stays at
    least half a float32 step below k and never rounds up to it (profiles/colour8_rule.md); what the flag of the entry changes is
    the rounding of an fp64 COLOUR to float32, which the case 'quant:f32' reaches."""
    k = np.arange(1, 256)
    near = ((k / 255.0).astype(np.float32).view(np.uint32)[:, None] + np.arange(-512, 513)[None]).astype(np.uint32).view(np.float32)
    some = np.concatenate([near.reshape(-1), np.random.default_rng(0).random(1 << 20).astype(np.float32)])
    assert np.array_equal(R.quantise(some, True, 'quant_f64_product'), R.quantise(some, True))
    assert (R.quantise(some, True) != np.rint(some * np.float32(255))).any()
    rgb, hsv = every_rgb
    tie = rgb[(rgb[:, 0] == rgb[:, 1]) & (rgb[:, 0] >= rgb[:, 2])]
    assert len(tie) == 256 * 257 // 2
    assert np.array_equal(R.rgb_to_hsv8(tie, 'rgb2hsv_g_first'), R.rgb_to_hsv8(tie))
    other = rgb[::4099]
    assert np.array_equal(R.rgb_to_hsv8(other, 'rgb2hsv_g_first'), hsv[::4099])
    grey = np.stack(np.meshgrid(np.arange(256), [0], np.arange(256), indexing='ij'), -1).reshape(-1, 3).astype(np.uint8)
    assert np.array_equal(R.hsv_to_rgb8(grey, 'hsv2rgb_no_grey'), R.hsv_to_rgb8(grey))
    assert np.array_equal(R.hsv_to_rgb8(grey)[:, 0], grey[:, 2])


def test_every_case_builds_and_the_sizes_cover_the_block_edges():
    for name in C.TABLE_CASES + C.QUANT_CASES + C.BRIGHT_CASES:
        c = C.case(name)
        w = C.want(c)
        assert w.shape == c.colors.shape and w.dtype == np.float64
        assert same_bits(w, w.astype(np.float32).astype(np.float64)), 'float32 values, exactly representable'
    col = C.base_colours()
    assert all(len(np.unique((col[:, k] * 255).astype(np.uint8))) == 256 for k in range(3))
    assert {1, 255, 256, 257} <= set(C.SIZES)
