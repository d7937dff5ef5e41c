"""Scene augmentation and label recomputation on the device: the stage the reference runs on CPU workers BEFORE the
voxelisation of prepare.py -- the geometric and colour augmentation of ``read_scene`` (dataprocessing/scannet.py:161-247
with dataprocessing/augmentation.py) and the per-instance box labels ``process_scene`` recomputes from the augmented
positions (``compute_bounding_box``, :321-367).  Host mirror of the b2m_aug_* / b2m_inst_boxes entries of
include/b2m_prepare.h (box2mask_amd/csrc/augment.hip).  Opt-in: nothing else of the package calls it.  No CPU fallback.

Parameters and application are separate.  ``draw_params`` is host code that draws what read_scene draws and returns plain
data (a ``SceneAugment``); ``augment_scenes`` applies such data to a batch of scene dicts on the device; the kernels only
ever see explicit matrices, centres and grids.  ``instance_labels`` recomputes the label dict ``prepare.box_supervision`` /
``mask_supervision`` read.

Pinned to the reference (tests/golden/augment.npz, made by its own functions): the grid blur and the trilinear displacement
of ``elastic_distortion`` / ``HAIS_elastic`` with their grid dimensions and axes, ``ChromaticAutoContrast``,
``ChromaticTranslation``, ``color_jittering`` and ``compute_bounding_box``.  Unpinned (open3d is not available to pin
them): the conventions of open3d that ``draw_params`` restates, and the vertex normals.  The three colour steps that need
albumentations / cv2 -- ``apply_hue_aug``, ``mix_3d_color_aug``, ``random_brightness`` -- are refused by default and drawn with
``draw_params(..., byte_colour=True)``: then they follow the exact rule of profiles/colour8_rule.md (numpy statements for
the tables and the normalisation, OpenCV's 8-bit colour-space conversions restated in integer / fp32 arithmetic), which is
UNPINNED too -- neither library is available to check it against; tools/pin_colour8.py pins it where they are.  The
reference's ``np.random`` call stream is not replayed: the draws have its distributions, not its sequence.

Normals: an affine step maps them by the normalised cofactor matrix, which equals recomputing area-weighted vertex normals
on the transformed mesh (mirroring included).  After a non-affine step (elastic, hais, jitter) they are recomputed from
``faces`` when the scene has them; without faces they keep their affine transform -- an approximation.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib
from ._lib import ptr

SCANNET_ELASTIC_DISTORT_PARAMS = ((0.2, 0.4), (0.8, 1.6))          # augmentation.py:8
_NON_AFFINE = ('elastic', 'hais', 'jitter')
_SEED_MAX = 2 ** 31 - 1


@dataclass
class SceneAugment:
    """What one call of read_scene draws, as plain data.

    geometric: ordered steps
        ('affine', M (3,3), centre 'mean' | 'origin' | xyz, t (3,)[, recentre=True])
                                     pos <- (pos - c) M^T + (c if recentre else 0) + t
        ('elastic', granularity, magnitude, noise (nx,ny,nz,3) float32 array | int seed)       augmentation.py:68-96
        ('hais', gran, mag, noise (3,bx,by,bz) float32 array (or a list of three) | int seed)  augmentation.py:171-188
        ('shift_min',)               pos <- pos - pos.min(0)                                    scannet.py:198
        ('jitter', sigma, seed)      pos <- pos + sigma * randn                                 scannet.py:202-204
    colour: steps in the reference's order
        ('auto_contrast', blend), ('translation', row (3,)), ('jitter', lo, hi, array (P,3) | int seed)
      and, from draw_params(..., byte_colour=True), the byte-colour steps (plain numbers; profiles/colour8_rule.md)
        ('brightness', beta)                                              random_brightness, augmentation.py:63-66
        ('mix3d', alpha, beta, (r, g, b) shifts)                          apply_mix3d_color_aug, :148-156
        ('hue', hue_shift, sat_shift, val_shift, alpha, beta, (r, g, b) shifts)     apply_hue_aug, :158-168
      'mix3d' and 'hue' leave normalised float32 values (negative and above 1); they exclude each other.
    """
    geometric: list = field(default_factory=list)
    colour: list = field(default_factory=list)


def _rot_xyz(ax, ay, az):
    """open3d's get_rotation_matrix_from_xyz((ax, ay, az)) = Rx Ry Rz (unpinned)."""
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], np.float64)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], np.float64)
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], np.float64)
    return rx @ ry @ rz


COLOR_MEAN = (0.47793125906962, 0.4303257521323044, 0.3749598901421883)     # augmentation.py:12-13
COLOR_STD = (0.2834475483823543, 0.27566157565723015, 0.27018971370874995)
HUE_LIMITS = (50.0, 60.0, 50.0)                                             # hue, sat, val shift limits (augmentation.py:19-21)
MIX3D_LIMITS = (0.2, 0.2, 20.0)                                             # contrast, brightness, RGB shift (the Mix3D yaml)
_COLOUR_ORDER = ('auto_contrast', 'translation', 'jitter', 'brightness', 'mix3d', 'hue')


def draw_params(cfg, n_points_hint=None, generator=None, byte_colour=False) -> SceneAugment:
    """Draw what read_scene (scannet.py:161-247) draws, with its probabilities and ranges, from ``generator`` (a
    numpy Generator; a fresh default_rng() if None).  Per-point noise (position jitter, colour jitter) and the noise grids
    are carried as seeds for the device generator, so ``n_points_hint`` is not needed for them and is accepted only for
    callers that size their own buffers.

    The open3d conventions this function restates are UNPINNED (open3d is not available to check them against):
      * get_rotation_matrix_from_xyz((x,y,z)) = Rx Ry Rz;
      * mesh.rotate(R) rotates about the vertex mean -> ('affine', R, 'mean', 0);
      * mesh.scale(s, center=(0,0,0)) -> ('affine', s I, 'origin', 0);
      * mesh.transform(Rt) -> ('affine', Rt[:3,:3], 'origin', Rt[:3,3]).
    They are isolated here: augment_scenes and the kernels see explicit matrices and centres only.

    cfg.apply_hue_aug, cfg.mix_3d_color_aug and cfg.random_brightness[0] > 0 raise NotImplementedError (albumentations)
    unless ``byte_colour=True``: then they are drawn too, after the older colour steps and in the reference's order
    (scannet.py:237-247), to be applied by the restated rule of profiles/colour8_rule.md.  With both mix_3d_color_aug and
    apply_hue_aug the reference quantises already-normalised colours: ValueError."""
    rb = getattr(cfg, 'random_brightness', None)
    if not byte_colour:
        refusal = ('%s needs albumentations / cv2, which this package does not carry; draw_params(..., byte_colour=True) '
                   'applies the restated rule of profiles/colour8_rule.md instead')
        for name in ('apply_hue_aug', 'mix_3d_color_aug'):
            if getattr(cfg, name, False):
                raise NotImplementedError(refusal % name)
        if rb is not None and rb[0] > 0:
            raise NotImplementedError(refusal % 'random_brightness')
    elif getattr(cfg, 'mix_3d_color_aug', False) and getattr(cfg, 'apply_hue_aug', False):
        raise ValueError('mix_3d_color_aug and apply_hue_aug together quantise colours that are already normalised: set one')
    out = SceneAugment()
    if not getattr(cfg, 'augmentation', False):
        return out
    rng = np.random.default_rng() if generator is None else generator
    seed = lambda: int(rng.integers(0, _SEED_MAX))
    zero = np.zeros(3)
    g = out.geometric
    rot = getattr(cfg, 'rotation_aug', [0, math.pi / 100, 1])
    if rng.random() < rot[0]:                                                       # rotate_mesh (augmentation.py:23-35)
        az = rng.uniform(0, 2 * math.pi) if rng.random() < rot[2] else 0.0
        ax = rng.uniform(-rot[1], rot[1]) if rng.random() < rot[2] else 0.0
        ay = rng.uniform(-rot[1], rot[1]) if rng.random() < rot[2] else 0.0
        g.append(('affine', _rot_xyz(ax, ay, az), 'mean', zero))
    if getattr(cfg, 'rotation_90_aug', False):                                      # rotate_mesh_90_degree (:38-44)
        az = [0, 0.5 * math.pi, math.pi, 1.5 * math.pi][int(rng.integers(0, 4))]
        g.append(('affine', _rot_xyz(0.0, 0.0, az), 'mean', zero))
    if rng.random() < getattr(cfg, 'flipping_aug', 0):                              # scannet.py:172-175
        g.append(('affine', np.diag([-1.0, 1.0, 1.0]), 'origin', zero))
    if getattr(cfg, 'HAIS_jitter_aug', False):                                      # :177-185: (pos - mean) m
        m = np.eye(3) + rng.standard_normal((3, 3)) * 0.1
        th = rng.random() * 2 * math.pi
        m = m @ np.array([[math.cos(th), math.sin(th), 0], [-math.sin(th), math.cos(th), 0], [0, 0, 1]])
        g.append(('affine', m.T.copy(), 'mean', zero, False))
    if rng.random() < getattr(cfg, 'elastic_distortion', 0):                        # :189-192
        for gran, mag in SCANNET_ELASTIC_DISTORT_PARAMS:
            g.append(('elastic', gran, mag, seed()))
    if rng.random() < getattr(cfg, 'elastic_distortion_HAIS', 0):                   # :195-199
        inv = 1 / cfg.voxel_size
        g.append(('hais', 6 * inv // 50, 40 * inv / 50, seed()))
        g.append(('hais', 20 * inv // 50, 160 * inv / 50, seed()))
        g.append(('shift_min',))
    pj = getattr(cfg, 'position_jittering', [0, 0.01])
    if rng.random() < pj[0]:                                                        # :202-205
        g.append(('jitter', float(pj[1]), seed()))
    sc = getattr(cfg, 'scaling_aug', [0, .9, 1.1])
    if rng.random() < sc[0]:                                                        # scale_mesh (augmentation.py:46-50)
        g.append(('affine', np.eye(3) * rng.uniform(sc[1], sc[2]), 'origin', zero))
    c = out.colour
    if rng.random() < getattr(cfg, 'chromatic_auto_contrast', 0):                   # scannet.py:223-225
        c.append(('auto_contrast', float(rng.random())))
    ct = getattr(cfg, 'chromatic_translation', [0, .1])
    if rng.random() < ct[0] and rng.random() < 0.95:                                # :228-231, augmentation.py:109
        c.append(('translation', (rng.random(3) - 0.5) * 1.0 * 2 * ct[1]))
    cj = getattr(cfg, 'color_jittering_aug', [0, .1])
    if rng.random() < cj[0]:                                                        # :234-235
        c.append(('jitter', -float(cj[1]), float(cj[1]), seed()))
    if not byte_colour:
        return out
    if rb is not None and rng.random() < rb[0]:                                     # :237-239, augmentation.py:63-66
        c.append(('brightness', float(rng.uniform(-rb[1], rb[1]))))
    hue = getattr(cfg, 'apply_hue_aug', False)
    if hue or getattr(cfg, 'mix_3d_color_aug', False):                              # :241-247
        hsv = tuple(float(rng.uniform(-lim, lim)) for lim in HUE_LIMITS) if hue else ()
        contrast, bright, shift = MIX3D_LIMITS          # always_apply: both Mix3D transforms run whatever their p
        mix = (1.0 + float(rng.uniform(-contrast, contrast)), float(rng.uniform(-bright, bright)),
               tuple(float(rng.uniform(-shift, shift)) for _ in range(3)))
        c.append((('hue',) + hsv + mix) if hue else (('mix3d',) + mix))
    return out


# ---- byte-colour tables (profiles/colour8_rule.md): the numpy statements of albumentations 1.0.3, one implementation for the
# ---- device path; tests/_colour8_rule.py restates them

def hsv_tables(hue_shift, sat_shift, val_shift):
    """_shift_hsv_uint8's 256-entry tables (hue, sat, val), None for a zero shift; all three None skips the conversion."""
    ramp = np.arange(0, 256, dtype=np.int16)
    return (np.mod(ramp + float(hue_shift), 180).astype(np.uint8) if hue_shift != 0 else None,
            np.clip(ramp + float(sat_shift), 0, 255).astype(np.uint8) if sat_shift != 0 else None,
            np.clip(ramp + float(val_shift), 0, 255).astype(np.uint8) if val_shift != 0 else None)


def rgb_tables(alpha, beta, shifts):
    """RandomBrightnessContrast (brightness_by_max) then RGBShift on uint8, composed: three 256-entry tables (r, g, b)."""
    lut = np.arange(0, 256).astype('float32')
    if alpha != 1:
        lut *= np.float32(alpha)
    if beta != 0:
        lut += np.float32(float(beta) * 255)
    bc = np.clip(lut, 0, 255).astype(np.uint8)
    out = []
    for shift in shifts:
        lut = np.arange(0, 256).astype('float32')
        lut += np.float32(shift)
        out.append(np.ascontiguousarray(np.clip(lut, 0, 255).astype(np.uint8)[bc]))
    return tuple(out)


def norm_rows(mean=COLOR_MEAN, std=COLOR_STD):
    """A.Normalize's fp32 rows: (mean * 255, 1 / (std * 255))."""
    m = np.array(mean, np.float32); m *= np.float32(255.0)
    s = np.array(std, np.float32); s *= np.float32(255.0)
    return m, np.reciprocal(s, dtype=np.float32)


# ---- grid geometry on the host (what the reference computes with numpy; tests/test_augment.py holds it to the fixture)

def elastic_grid(coords_min, coords_max, granularity):
    """elastic_distortion's noise grid (augmentation.py:77-93): (dims (3,) int, [axis arrays], lo, step, hi)."""
    coords_min, coords_max = np.asarray(coords_min, np.float64), np.asarray(coords_max, np.float64)
    dims = ((coords_max - coords_min) // granularity).astype(int) + 3
    return _axes(dims, coords_min - granularity, coords_min + granularity * (dims - 2))


def hais_grid(abs_max, gran):
    """HAIS_elastic's noise grid (augmentation.py:176-184)."""
    if int(gran) < 1:
        raise ValueError('hais: int(gran) must be at least 1 (the reference divides by it), got %r' % (gran,))
    dims = np.asarray(abs_max, np.float64).astype(np.int32) // int(gran) + 3
    return _axes(dims, -(dims - 1) * gran, (dims - 1) * gran)


def _axes(dims, start, stop):
    axes, steps = [], []
    for a, b, d in zip(start, stop, dims):
        ax, st = np.linspace(a, b, d, retstep=True)
        axes.append(ax); steps.append(st)
    return (np.asarray(dims, np.int64), axes, np.asarray(start, np.float64).copy(), np.asarray(steps, np.float64),
            np.asarray(stop, np.float64).copy())


# ---- thin wrappers of the entries (also what the tests and tools/bench_augment.py call)

def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


def _f64(v, n):
    a = np.ascontiguousarray(np.asarray(v, np.float64).reshape(-1))
    assert a.shape == (n,)
    return a


def column_stats(x: torch.Tensor) -> torch.Tensor:
    """[mean xyz | min xyz | max xyz | max |.| xyz] of an (n,3) fp64 device tensor: (12,) fp64, no host read."""
    partial = torch.empty(256 * 12, dtype=torch.float64, device=x.device)
    stats = torch.empty(12, dtype=torch.float64, device=x.device)
    _lib.call('b2m_aug_stats', ptr(x), x.shape[0], ptr(partial), ptr(stats))
    return stats


def affine_(pos, normals, M, centre='origin', t=None, recentre=True, stats=None):
    """In place: pos <- (pos - c) M^T + (c if recentre) + t; normals (or None) by the normalised cofactor matrix.
    centre: 'origin', xyz, 'mean' or 'min' (the latter two from ``stats`` = column_stats(pos), computed if missing)."""
    m = _f64(M, 9)
    th = _f64(t, 3) if t is not None else None
    c_host, c_dev = None, None
    if isinstance(centre, str):
        if centre in ('mean', 'min'):
            stats = column_stats(pos) if stats is None else stats
            c_dev = stats[0:3] if centre == 'mean' else stats[3:6]
        elif centre != 'origin':
            raise ValueError('affine: unknown centre %r' % (centre,))
    else:
        c_host = _f64(centre, 3)
    _lib.call('b2m_aug_affine', ptr(pos), ptr(normals), pos.shape[0], _hp(m), _hp(c_host) if c_host is not None else None,
              ptr(c_dev), _hp(th) if th is not None else None, 1 if recentre else 0)


def blur_(grid: torch.Tensor) -> torch.Tensor:
    """In place: the six 3-tap passes over an fp32 device grid (nx,ny,nz,3)."""
    assert grid.dtype == torch.float32 and grid.dim() == 4 and grid.shape[3] == 3 and grid.is_contiguous()
    tmp = torch.empty_like(grid)
    _lib.call('b2m_aug_blur', ptr(grid), ptr(tmp), grid.shape[0], grid.shape[1], grid.shape[2])
    return grid


def displace_(pos, grid, lo, step, hi, magnitude):
    """In place: pos += magnitude * trilinear(grid, pos) on axes linspace(lo, hi, n); points outside stay."""
    assert grid.dtype == torch.float32 and grid.dim() == 4 and grid.shape[3] == 3 and grid.is_contiguous()
    lo, step, hi = _f64(lo, 3), _f64(step, 3), _f64(hi, 3)
    _lib.call('b2m_aug_displace', ptr(pos), pos.shape[0], ptr(grid), grid.shape[0], grid.shape[1], grid.shape[2],
              _hp(lo), _hp(step), _hp(hi), float(magnitude))


def _face_range(faces: torch.Tensor) -> torch.Tensor:
    """[min, max] vertex index of an (F,3) device tensor, on the device ([0, -1] for no faces)."""
    flat = faces.reshape(-1)
    if not flat.numel():
        return torch.tensor([0, -1], dtype=torch.int64, device=faces.device)
    return torch.stack([flat.min(), flat.max()])


def _check_face_range(lo, hi, n_vert):
    if lo < 0 or hi >= n_vert:
        raise ValueError('faces: vertex indices must lie in [0, %d), found [%d, %d]' % (n_vert, lo, hi))


def vertex_face_csr(faces: torch.Tensor, n_vert: int, checked: bool = False):
    """Vertex-to-face CSR of an (F,3) int64 device tensor: (row_ptr (n_vert+1,), face_of (3F,)), faces ascending within a
    row (stable sort).  Unless the caller has already checked the index range (augment_scenes checks all scenes of a batch
    in one read), one host read does; the build itself reads nothing back.  Callers cache the result -- the topology never
    changes."""
    flat = faces.reshape(-1)
    if not checked:
        _check_face_range(*_face_range(faces).cpu().tolist(), n_vert)
    ordered, order = torch.sort(flat, stable=True)                # position k of `flat` belongs to face k // 3
    face_of = torch.div(order, 3, rounding_mode='floor').contiguous()
    row_ptr = torch.searchsorted(ordered, torch.arange(n_vert + 1, dtype=torch.int64, device=faces.device)).contiguous()
    return row_ptr, face_of


def vertex_normals(pos, faces, csr):
    """open3d's compute_vertex_normals() + normalize_normals() as documented (unpinned): normalised sum of the faces'
    unnormalised cross products, (0,0,1) for a zero sum."""
    out = torch.empty_like(pos)
    row_ptr, face_of = csr
    _lib.call('b2m_aug_vertex_normals', ptr(pos), pos.shape[0], ptr(faces) if faces.numel() else None, faces.shape[0],
              ptr(row_ptr), ptr(face_of) if faces.numel() else None, ptr(out))
    return out


def colour_(colors, steps, generator_device=None):
    """In place: the colour steps of a SceneAugment in one min/max reduction and one fused pass, and the byte-colour steps
    ('brightness', 'mix3d' | 'hue'; profiles/colour8_rule.md) in one more pass after it."""
    flags, blend, tr, jit = 0, 0.0, None, None
    bright, chain = None, None
    seen = []
    for s in steps:
        if s[0] not in _COLOUR_ORDER:
            raise ValueError('unknown colour step %r' % (s[0],))
        if seen and _COLOUR_ORDER.index(s[0]) <= seen[-1]:
            raise ValueError('colour steps must follow the reference order: auto_contrast, translation, jitter'
                             + (', brightness, mix3d, hue' if max(seen[-1], _COLOUR_ORDER.index(s[0])) > 2 else ''))
        seen.append(_COLOUR_ORDER.index(s[0]))
        if s[0] == 'auto_contrast':
            flags |= 1; blend = float(s[1])
        elif s[0] == 'translation':
            flags |= 2; tr = _f64(s[1], 3)
        elif s[0] == 'brightness':
            bright = float(s[1])
        elif s[0] in ('mix3d', 'hue'):
            if chain is not None:
                raise ValueError('mix3d and hue together quantise colours that are already normalised: use one')
            chain = s
        else:
            flags |= 4
            lo, hi, src = s[1], s[2], s[3]
            if isinstance(src, (int, np.integer)):
                gen = torch.Generator(device=colors.device); gen.manual_seed(int(src))
                jit = torch.rand(colors.shape, dtype=torch.float64, device=colors.device, generator=gen) * (hi - lo) + lo
            else:
                jit = _dev(src, torch.float64, colors.device)
                if jit.shape != colors.shape:
                    raise ValueError('colour jitter array must have the colours\' shape')
    if flags:
        stats = column_stats(colors) if flags & 1 else None
        _lib.call('b2m_aug_colour', ptr(colors), colors.shape[0], ptr(stats), flags, blend, _hp(tr) if tr is not None else None,
                  ptr(jit))
    if chain is not None:
        # brightness leaves float32 colours, and numpy then forms colour * 255 in float32
        hsv = hsv_tables(*chain[1:4]) if chain[0] == 'hue' else (None, None, None)
        rgb = rgb_tables(*chain[-3:])
        mean, den = norm_rows()
        _lib.call('b2m_aug_colour8', ptr(colors), colors.shape[0], 3 if bright is not None else 0,
                  bright if bright is not None else 0.0, *[_hp(t) if t is not None else None for t in hsv + rgb],
                  _hp(mean), _hp(den))
    elif bright is not None:
        _lib.call('b2m_aug_brightness', ptr(colors), colors.shape[0], bright)
    return colors


def _dev(x, dtype, device):
    t = torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x)
    return t.to(device=device, dtype=dtype).contiguous()


def _noise_grid(step, dims, dev):
    """The step's noise as an fp32 device grid (nx,ny,nz,3): the host array it carries (parity path), else randn of its seed."""
    kind, src = step[0], step[3]
    shape = tuple(int(d) for d in dims) + (3,)
    if isinstance(src, (int, np.integer)):
        gen = torch.Generator(device=dev); gen.manual_seed(int(src))
        return torch.randn(shape, dtype=torch.float32, device=dev, generator=gen)
    a = np.asarray(src, np.float32)
    if kind == 'hais':                                     # three (bx,by,bz) grids, one per output axis
        a = np.moveaxis(a, 0, -1)
    if a.shape != shape:
        raise ValueError('%s: the noise array has shape %s, the grid of this cloud is %s' % (kind, a.shape, shape))
    return _dev(a, torch.float32, dev)


def augment_scenes(scenes, params_list, device=None) -> list:
    """Apply one SceneAugment per scene on the device.  scenes: the dicts ``prepare.voxelize_scenes`` consumes --
    'positions', 'colors', 'normals' (P,3), 'segments' (P,), optionally 'faces' (F,3); numpy or torch.  Returns new dicts
    with fp64 device tensors (segments int64) -- the inputs are not written -- and every other key passed through.

    Staged like voxelize_scenes: every scene advances until its next step needs a number on the host (the extent of the
    cloud that sizes a noise grid), then the pending extents of ALL scenes come back in one copy.  The number of host reads
    per batch is the largest number of elastic / hais steps of any one scene (at most four with draw_params), whatever the
    batch size.  The vertex-to-face CSR of a scene with faces is built once (the index check costs one more read) and cached on
    the scene dict under '_face_csr'; the index checks of all such scenes share one read.  ``device``: the kernels run on
    that device's current stream (the current device if None)."""
    _lib.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != 'cuda':
        raise ValueError('augment_scenes: %s is not a GPU' % (dev,))
    with torch.cuda.device(dev):
        return _augment_scenes(scenes, params_list, torch.device('cuda', torch.cuda.current_device()))


def _augment_scenes(scenes, params_list, dev) -> list:
    if len(scenes) != len(params_list):
        raise ValueError('augment_scenes: %d scenes, %d parameter sets' % (len(scenes), len(params_list)))
    st = []
    for scene, prm in zip(scenes, params_list):
        pos = _dev(scene['positions'], torch.float64, dev)
        if pos.dim() != 2 or pos.shape[1] != 3 or pos.shape[0] == 0:
            raise ValueError('augment_scenes: positions must be (P,3) with P > 0')
        P = pos.shape[0]
        geo, col = list(prm.geometric), list(prm.colour)
        if geo:
            pos = pos.clone() if _aliases(pos, scene['positions']) else pos
        normals = _dev(scene['normals'], torch.float64, dev)
        colors = _dev(scene['colors'], torch.float64, dev)
        assert normals.shape == (P, 3) and colors.shape == (P, 3)
        if geo and _aliases(normals, scene['normals']):
            normals = normals.clone()
        if col and _aliases(colors, scene['colors']):
            colors = colors.clone()
        faces = scene.get('faces')
        from_faces = faces is not None and any(s[0] in _NON_AFFINE for s in geo)
        st.append(dict(scene=scene, pos=pos, normals=normals, colors=colors, geo=geo, col=col, k=0, wait=None,
                       from_faces=from_faces, faces=_dev(faces, torch.int64, dev) if from_faces else None))
    # scenes whose vertex-to-face CSR is not cached yet: the index ranges of all of them in one read, then the builds
    fresh = [s for s in st if s['from_faces'] and '_face_csr' not in s['scene']]
    if fresh:
        ranges = torch.stack([_face_range(s['faces']) for s in fresh]).cpu().tolist()
        for s, (lo, hi) in zip(fresh, ranges):
            _check_face_range(lo, hi, s['pos'].shape[0])
            s['scene']['_face_csr'] = vertex_face_csr(s['faces'], s['pos'].shape[0], checked=True)
    while True:
        # ---- advance every scene to its next grid step (or to the end of its list)
        for s in st:
            pos = s['pos']
            nrm = None if s['from_faces'] else s['normals']            # recomputed from the faces at the end anyway
            while s['k'] < len(s['geo']) and s['wait'] is None:
                step = s['geo'][s['k']]
                kind = step[0]
                if kind == 'affine':
                    affine_(pos, nrm, step[1], step[2], step[3], step[4] if len(step) > 4 else True)
                elif kind == 'shift_min':
                    affine_(pos, None, np.eye(3), 'min', None, False)
                elif kind == 'jitter':
                    gen = torch.Generator(device=dev); gen.manual_seed(int(step[2]))
                    noise = torch.randn(pos.shape, dtype=torch.float64, device=dev, generator=gen)
                    _lib.call('b2m_aug_axpy', ptr(pos), ptr(noise), float(step[1]), pos.numel())
                elif kind in ('elastic', 'hais'):
                    s['wait'] = column_stats(pos)
                    continue
                else:
                    raise ValueError('augment_scenes: unknown geometric step %r' % (kind,))
                s['k'] += 1
        waiting = [s for s in st if s['wait'] is not None]
        if not waiting:
            break
        host = torch.stack([s['wait'] for s in waiting]).cpu().numpy()                # the one read of this round
        for s, h in zip(waiting, host):
            step = s['geo'][s['k']]
            if not np.isfinite(h).all():
                raise ValueError('augment_scenes: non-finite positions')
            if step[0] == 'elastic':
                dims, _, lo, stp, hi = elastic_grid(h[3:6], h[6:9], step[1])
            else:
                dims, _, lo, stp, hi = hais_grid(h[9:12], step[1])
            grid = blur_(_noise_grid(step, dims, dev))
            displace_(s['pos'], grid, lo, stp, hi, step[2])
            s['wait'] = None
            s['k'] += 1
    out = []
    for s in st:
        scene = s['scene']
        if s['from_faces']:
            s['normals'] = vertex_normals(s['pos'], s['faces'], scene['_face_csr'])
        colour_(s['colors'], s['col'])
        new = dict(scene)
        new.update(positions=s['pos'], normals=s['normals'], colors=s['colors'],
                   segments=_dev(scene['segments'], torch.int64, dev).reshape(-1))
        out.append(new)
    return out


def _aliases(t, src):
    return torch.is_tensor(src) and t.data_ptr() == src.data_ptr()


def instance_labels(scene: dict, semantics, instances, seg2inst) -> dict:
    """compute_bounding_box (scannet.py:321-367) on the (augmented) positions of ``scene``: the label dict
    ``prepare.box_supervision`` / ``mask_supervision`` read, as device tensors with the reference's dtypes (float32 boxes,
    int32 per-instance semantics).  semantics, instances: (P,) per point; seg2inst: passed through.  Instance ids must be
    dense 0..I-1 (the reference asserts it, :428): ValueError otherwise.  Two host reads: the id range, then the check.
    'centers' / 'center_distances' (compute_avg_centers) have no consumer in this package and are left out."""
    _lib.require_gpu()
    pos = scene['positions']
    dev = pos.device if torch.is_tensor(pos) and pos.is_cuda else torch.device('cuda', torch.cuda.current_device())
    with torch.cuda.device(dev):                      # the entries launch on the current device's stream
        return _instance_labels(_dev(pos, torch.float64, dev), semantics, instances, seg2inst, dev)


def _instance_labels(pos, semantics, instances, seg2inst, dev) -> dict:
    P = pos.shape[0]
    inst = _dev(instances, torch.int64, dev).reshape(-1)
    sem = _dev(semantics, torch.int64, dev).reshape(-1)
    if P == 0 or inst.shape != (P,) or sem.shape != (P,):
        raise ValueError('instance_labels: need P > 0 points and (P,) semantics / instances')
    lo, hi = torch.stack([inst.min(), inst.max()]).cpu().tolist()
    if lo < 0 or hi >= P:
        raise ValueError('instance_labels: instance ids must be dense 0..I-1, found ids in [%d, %d]' % (lo, hi))
    n_inst = int(hi) + 1
    acc = torch.empty(8 * n_inst, dtype=torch.int64, device=dev)
    centers64 = torch.empty((n_inst, 3), dtype=torch.float64, device=dev)
    per_sem = torch.empty(n_inst, dtype=torch.int32, device=dev)
    per_centers = torch.empty((n_inst, 3), dtype=torch.float32, device=dev)
    per_bounds = torch.empty((n_inst, 3), dtype=torch.float32, device=dev)
    per_radius = torch.empty(n_inst, dtype=torch.float32, device=dev)
    offsets = torch.empty((P, 3), dtype=torch.float32, device=dev)
    dist = torch.empty((P, 1), dtype=torch.float32, device=dev)
    missing = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.call('b2m_inst_boxes', ptr(pos), ptr(inst), ptr(sem), P, n_inst, ptr(acc), ptr(centers64), ptr(per_sem),
              ptr(per_centers), ptr(per_bounds), ptr(per_radius), ptr(offsets), ptr(dist), ptr(missing))
    n_missing = int(missing.item())
    if n_missing:
        raise ValueError('instance_labels: instance ids must be dense 0..I-1, %d of the ids below %d have no point'
                         % (n_missing, n_inst))
    return {
        'semantics': sem, 'instances': inst, 'seg2inst': seg2inst,
        'bb_centers': per_centers[inst], 'bb_offsets': offsets, 'bb_bounds': per_bounds[inst],
        'bb_center_distances': dist, 'bb_radius': per_radius[inst][:, None],
        'unique_instances': torch.arange(n_inst, dtype=torch.int64, device=dev),
        'per_instance_semantics': per_sem, 'per_instance_bb_centers': per_centers, 'per_instance_bb_bounds': per_bounds,
        'per_instance_bb_radius': per_radius,
    }
