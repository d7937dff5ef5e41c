"""The byte-colour rule (profiles/colour8_rule.md) in numpy, every dtype spelled out: what b2m_aug_colour8 / b2m_aug_brightness
(box2mask_amd/csrc/augment.hip) and augment.colour_ are held to, bit for bit.

It restates apply_mix3d_color_aug, apply_hue_aug and random_brightness of the reference (dataprocessing/augmentation.py:63-66,
148-168) through albumentations 1.0.3's uint8 paths: the table builders and A.Normalize are its numpy statements; the two 8-bit
colour-space conversions are OpenCV's (integer RGB->HSV with hue range 180, fp32 HSV->RGB).  Neither library is available to
pin this against, so the rule is UNPINNED; tests/test_colour8_rule.py holds the conversions to matplotlib's within a derived
bound, and tools/pin_colour8.py pins everything on a machine that has cv2 and albumentations.

Where numpy's float -> uint8 cast is undefined this project's rule is: NaN -> 0, negative -> 0, above 255 -> 255.

Every function takes ``mistake=``: one deliberate MISTAKE written as a variant of the rule.  tests/test_colour8_rule.py shows
that each of them changes a named case of tests/_colour8_cases.py: that is how the cases are shown to have teeth."""
import numpy as np

F32, F64, U8, I32 = np.float32, np.float64, np.uint8, np.int32

COLOR_MEAN = (0.47793125906962, 0.4303257521323044, 0.3749598901421883)
COLOR_STD = (0.2834475483823543, 0.27566157565723015, 0.27018971370874995)

MISTAKES = ('quant_round', 'quant_f64_product', 'hue_mod_256', 'rgb2hsv_no_2048', 'rgb2hsv_no_wrap', 'rgb2hsv_g_first',
            'hsv2rgb_rows_swapped', 'hsv2rgb_no_grey', 'mix3d_shift_first', 'norm_f64', 'norm_mean_unscaled',
            'hue_zero_shift_table')


# ----------------------------------------------------------------------------- quantise
def quantise(color, f32_product=False, mistake=None):
    """u8 = (color * 255).astype(np.uint8): the product in fp64, or in fp32 when the colours are float32 (numpy: float32 array x
    Python int stays float32), truncated.  NaN -> 0, negative -> 0, above 255 -> 255."""
    color = np.asarray(color)
    with np.errstate(over='ignore'):
        c32 = color.astype(F32)
    if not f32_product:
        p = color.astype(F64) * F64(255)
    elif mistake == 'quant_f64_product':
        p = c32.astype(F64) * F64(255)
    else:
        p = c32 * F32(255)
        assert p.dtype == F32
    with np.errstate(invalid='ignore'):
        p = np.where(p > 0, np.minimum(p, p.dtype.type(255)), p.dtype.type(0))            # NaN compares false: 0
    return (np.rint(p) if mistake == 'quant_round' else np.trunc(p)).astype(U8)


# ----------------------------------------------------------------------------- tables (albumentations 1.0.3, numpy statements)
def hsv_tables(hue_shift, sat_shift, val_shift, mistake=None):
    """_shift_hsv_uint8: (hue, sat, val) tables, None where the shift is 0 (that channel is then not touched)."""
    ramp = np.arange(0, 256, dtype=np.int16)
    always = mistake == 'hue_zero_shift_table'
    hue = np.mod(ramp + float(hue_shift), 256 if mistake == 'hue_mod_256' else 180).astype(U8)      # fp64 sum, mod, truncation
    sat = np.clip(ramp + float(sat_shift), 0, 255).astype(U8)
    val = np.clip(ramp + float(val_shift), 0, 255).astype(U8)
    return (hue if hue_shift != 0 or always else None, sat if sat_shift != 0 or always else None,
            val if val_shift != 0 or always else None)


def brightness_contrast_table(alpha, beta):
    """_brightness_contrast_adjust_uint8 with brightness_by_max."""
    lut = np.arange(0, 256).astype('float32')
    if alpha != 1:
        lut *= F32(alpha)
    if beta != 0:
        lut += F32(float(beta) * 255)                      # the product in fp64, the in-place add in fp32
    return np.clip(lut, 0, 255).astype(U8)


def shift_table(shift):
    """_shift_rgb_uint8's table of one channel."""
    lut = np.arange(0, 256).astype('float32')
    lut += F32(shift)
    return np.clip(lut, 0, 255).astype(U8)


def rgb_tables(alpha, beta, shifts, mistake=None):
    """RandomBrightnessContrast then RGBShift, composed into one table per channel."""
    bc = brightness_contrast_table(alpha, beta)
    if mistake == 'mix3d_shift_first':
        return tuple(bc[shift_table(s)] for s in shifts)
    return tuple(shift_table(s)[bc] for s in shifts)


def norm_rows(mistake=None):
    """A.Normalize: mean * 255 and 1 / (std * 255), fp32."""
    mean = np.array(COLOR_MEAN, F32)
    if mistake != 'norm_mean_unscaled':
        mean *= F32(255.0)
    std = np.array(COLOR_STD, F32)
    std *= F32(255.0)
    return mean, np.reciprocal(std, dtype=F32)


# ----------------------------------------------------------------------------- the 8-bit conversions (OpenCV, restated)
_I = np.arange(1, 256, dtype=F64)
SDIV = np.concatenate([[0], np.rint(F64(255 << 12) / (1.0 * _I))]).astype(I32)           # fp64, round half to even
HDIV = np.concatenate([[0], np.rint(F64(180 << 12) / (6.0 * _I))]).astype(I32)
SECTOR_TAB = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])   # (b, g, r) of tab, per sector


def rgb_to_hsv8(rgb, mistake=None):
    """(...,3) uint8 RGB -> (...,3) uint8 HSV, hue in [0, 180): int32 arithmetic."""
    rgb = np.asarray(rgb, U8).astype(I32)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    v = np.maximum(r, np.maximum(g, b))
    d = v - np.minimum(r, np.minimum(g, b))
    half = I32(0 if mistake == 'rgb2hsv_no_2048' else 2048)
    s = (d * SDIV[v] + half) >> 12
    if mistake == 'rgb2hsv_g_first':
        h = np.where(v == g, b - r + 2 * d, np.where(v == r, g - b, r - g + 4 * d))
    else:
        h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))        # the order of the tests is the tie rule
    h = (h * HDIV[d] + half) >> 12                                                          # arithmetic shift of a signed value
    assert h.dtype == I32
    if mistake != 'rgb2hsv_no_wrap':
        h = np.where(h < 0, h + 180, h)
    return np.stack([h, s, v], -1).astype(U8)


def _sat8(x):
    """saturate(rint(x * 255.f)), round half to even; fp32 in."""
    y = np.rint(x * F32(255))
    assert y.dtype == F32
    return np.clip(y, 0, 255).astype(U8)


def hsv_to_rgb8(hsv, mistake=None):
    """(...,3) uint8 HSV -> (...,3) uint8 RGB: fp32 arithmetic, every operation rounded (no contraction)."""
    hsv = np.asarray(hsv, U8)
    h = hsv[..., 0].astype(F32) * (F32(6) / F32(180))
    s = hsv[..., 1].astype(F32) * (F32(1) / F32(255))
    v = hsv[..., 2].astype(F32) * (F32(1) / F32(255))
    h = np.fmod(h, F32(6))
    sector = np.floor(h)
    h = h - sector
    sector = sector.astype(I32)
    out_of_range = (sector < 0) | (sector > 5)
    sector = np.where(out_of_range, 0, sector)
    h = np.where(out_of_range, F32(0), h)
    one = F32(1)
    tab = np.stack([v, v * (one - s), v * (one - s * h), v * (one - s * (one - h))], 0)
    assert tab.dtype == F32
    T = SECTOR_TAB.copy()
    if mistake == 'hsv2rgb_rows_swapped':
        T[[1, 2]] = T[[2, 1]]
    pick = lambda k: np.take_along_axis(tab, T[sector, k][None], 0)[0]
    b, g, r = pick(0), pick(1), pick(2)
    if mistake != 'hsv2rgb_no_grey':
        grey = s == 0
        r, g, b = np.where(grey, v, r), np.where(grey, v, g), np.where(grey, v, b)
    return np.stack([_sat8(r), _sat8(g), _sat8(b)], -1)


# ----------------------------------------------------------------------------- the steps
def hue_step(u8, hue_shift, sat_shift, val_shift, mistake=None):
    """_shift_hsv_uint8: skipped entirely when all three shifts are 0."""
    tabs = hsv_tables(hue_shift, sat_shift, val_shift, mistake)
    return apply_hsv_tables(u8, tabs, mistake)


def apply_hsv_tables(u8, tabs, mistake=None):
    if all(t is None for t in tabs):
        return u8
    hsv = rgb_to_hsv8(u8, mistake)
    hsv = np.stack([hsv[..., k] if tabs[k] is None else tabs[k][hsv[..., k]] for k in range(3)], -1)
    return hsv_to_rgb8(hsv, mistake)


def apply_rgb_tables(u8, tabs):
    return np.stack([tabs[k][u8[..., k]] for k in range(3)], -1)


def normalise(u8, rows=None, mistake=None):
    """(u8.astype(float32) - mean) * den: two fp32 roundings."""
    mean, den = norm_rows(mistake) if rows is None else rows
    if mistake == 'norm_f64':
        return ((u8.astype(F64) - mean.astype(F64)) * den.astype(F64)).astype(F32)
    out = (u8.astype(F32) - mean) * den
    assert out.dtype == F32
    return out


def brightness(colors, beta):
    """random_brightness: float32 colours + float32(beta), clipped to [0,1] (NaN stays); float32 out."""
    c32 = np.asarray(colors).astype(F32)
    c32 += F32(beta)
    return np.clip(c32, 0, 1)


def chain(colors, f32_product, hsv_tabs, rgb_tabs, rows=None, beta=None, mistake=None):
    """What b2m_aug_colour8 computes from explicit tables: [brightness] -> quantise -> [HSV tables] -> RGB tables -> normalise.
    float32 out."""
    if beta is not None:
        colors = brightness(colors, beta)
    u8 = quantise(colors, f32_product, mistake)
    u8 = apply_hsv_tables(u8, hsv_tabs, mistake)
    return normalise(apply_rgb_tables(u8, rgb_tabs), rows, mistake)


def mix3d_colour(colors, alpha, beta, shifts, f32_product=False, mistake=None):
    """apply_mix3d_color_aug: quantise -> Mix3D tables -> normalise."""
    return chain(colors, f32_product, (None, None, None), rgb_tables(alpha, beta, shifts, mistake), mistake=mistake)


def hue_colour(colors, hue_shift, sat_shift, val_shift, alpha, beta, shifts, f32_product=False, mistake=None):
    """apply_hue_aug: quantise -> hue step -> Mix3D tables -> normalise."""
    return chain(colors, f32_product, hsv_tables(hue_shift, sat_shift, val_shift, mistake),
                 rgb_tables(alpha, beta, shifts, mistake), mistake=mistake)


def colour_steps(colors, steps):
    """The byte-colour steps of a SceneAugment.colour list ('brightness', 'mix3d', 'hue'), in order, on fp64 colours; fp64 out
    (the float32 values, exactly)."""
    out, f32 = np.asarray(colors, F64), False
    for s in steps:
        if s[0] == 'brightness':
            out, f32 = brightness(out, s[1]).astype(F64), True
        elif s[0] == 'mix3d':
            out = mix3d_colour(out, s[1], s[2], s[3], f32).astype(F64)
        elif s[0] == 'hue':
            out = hue_colour(out, s[1], s[2], s[3], s[4], s[5], s[6], f32).astype(F64)
        else:
            raise ValueError(s[0])
    return out
