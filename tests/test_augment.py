"""Host side of box2mask_amd/augment.py: what draw_params draws, the grid geometry against the reference's own
(tests/golden/augment.npz, tools/gen_golden.py augment), and the argument checks of the new entries.  No device."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from box2mask_amd import _lib, augment
from box2mask_amd.config import scannet_config


@pytest.fixture(scope='module')
def gold(golden_dir):
    """augment.npz and, merged in, augment_steps.npz (the per-step outputs of the 5000-point case: a file of their own for
    the size limit of a committed file)."""
    out = {}
    for f in ('augment.npz', 'augment_steps.npz'):
        with np.load(os.path.join(golden_dir, f)) as z:
            out.update({k: z[k] for k in z.files})
    return out


def _all_on(**kw):
    on = dict(augmentation=True, rotation_aug=[1.0, math.pi / 100, 1], rotation_90_aug=True, flipping_aug=1.0,
              HAIS_jitter_aug=True, elastic_distortion=1.0, elastic_distortion_HAIS=1.0, position_jittering=[1.0, 0.01],
              scaling_aug=[1.0, 0.8, 1.2], chromatic_auto_contrast=1.0, chromatic_translation=[1.0, 0.1],
              color_jittering_aug=[1.0, 0.1])
    on.update(kw)
    return scannet_config(**on)


def test_config_carries_the_reference_defaults():
    cfg = scannet_config()
    assert cfg.augmentation is False and cfg.rotation_aug == [0, math.pi / 100, 1] and cfg.rotation_90_aug is False
    assert cfg.flipping_aug == 0 and cfg.HAIS_jitter_aug is False and cfg.elastic_distortion == 0 and cfg.elastic_distortion_HAIS == 0
    assert cfg.position_jittering == [0, 0.01] and cfg.scaling_aug == [0, .9, 1.1] and cfg.chromatic_auto_contrast == 0
    assert cfg.chromatic_translation == [0, .1] and cfg.color_jittering_aug == [0, .1]


def test_nothing_is_drawn_when_everything_is_off():
    p = augment.draw_params(scannet_config(augmentation=True), generator=np.random.default_rng(0))
    assert p.geometric == [] and p.colour == []
    p = augment.draw_params(_all_on(augmentation=False), generator=np.random.default_rng(0))          # the master switch
    assert p.geometric == [] and p.colour == []


def test_every_drawn_quantity_lies_in_its_reference_range():
    cfg = _all_on()
    seen_translation = 0
    for seed in range(40):
        p = augment.draw_params(cfg, n_points_hint=1000, generator=np.random.default_rng(seed))
        kinds = [s[0] for s in p.geometric]
        assert kinds == ['affine'] * 4 + ['elastic'] * 2 + ['hais'] * 2 + ['shift_min', 'jitter', 'affine'], kinds
        rot, rot90, flip, hj = (p.geometric[i] for i in range(4))
        for r in (rot, rot90):
            assert r[2] == 'mean' and np.all(r[3] == 0)
            assert np.allclose(r[1] @ r[1].T, np.eye(3), atol=1e-14) and abs(np.linalg.det(r[1]) - 1) < 1e-14
        # small tilts about x and y: the z axis moves by at most the two angles together
        assert math.acos(min(1.0, rot[1][2, 2])) <= 2 * math.pi / 100 + 1e-12
        quarter = rot90[1]
        assert np.allclose(quarter[2], [0, 0, 1]) and np.allclose(np.abs(quarter[:2, :2]).sum(), 2, atol=1e-12)
        assert np.allclose(np.round(quarter), quarter, atol=1e-15)
        assert flip[2] == 'origin' and np.array_equal(flip[1], np.diag([-1.0, 1.0, 1.0])) and np.linalg.det(flip[1]) == -1
        assert hj[2] == 'mean' and hj[4] is False and hj[1].shape == (3, 3)
        assert [(s[1], s[2]) for s in p.geometric[4:6]] == [(0.2, 0.4), (0.8, 1.6)]
        assert [(s[1], s[2]) for s in p.geometric[6:8]] == [(6.0, 40.0), (20.0, 160.0)]             # 2 cm voxels
        assert all(isinstance(s[3], int) and 0 <= s[3] < 2 ** 31 for s in p.geometric[4:8])
        assert p.geometric[9][1] == 0.01
        scale = p.geometric[10]
        s = scale[1][0, 0]
        assert scale[2] == 'origin' and 0.8 <= s <= 1.2 and np.array_equal(scale[1], np.eye(3) * s)
        ckinds = [s[0] for s in p.colour]
        assert ckinds in (['auto_contrast', 'translation', 'jitter'], ['auto_contrast', 'jitter']), ckinds   # translation: 95 %
        assert 0 <= p.colour[0][1] < 1
        if 'translation' in ckinds:
            seen_translation += 1
            assert p.colour[1][1].shape == (3,) and np.all(np.abs(p.colour[1][1]) <= 0.1)
        assert p.colour[-1][1:3] == (-0.1, 0.1)
    assert seen_translation >= 30


def test_flip_probability_and_quarter_turns():
    cfg = scannet_config(augmentation=True, rotation_90_aug=True, flipping_aug=0.5, scaling_aug=[1.0, 0.8, 1.2])   # configs/scannet.txt
    rng = np.random.default_rng(5)
    flips, turns = 0, set()
    for _ in range(400):
        g = augment.draw_params(cfg, generator=rng).geometric
        flips += any(np.linalg.det(s[1]) < 0 for s in g)
        turns.add(tuple(np.round(g[0][1][0, :2]).astype(int)))
    assert 150 < flips < 250 and len(turns) == 4


@pytest.mark.parametrize('field,value', [('apply_hue_aug', True), ('mix_3d_color_aug', True), ('random_brightness', [0.5, 0.1])])
def test_unsupported_colour_paths_are_refused(field, value):
    with pytest.raises(NotImplementedError, match=field):
        augment.draw_params(scannet_config(augmentation=True, **{field: value}))


def test_grid_dimensions_and_axes_equal_the_reference(gold):
    for name in gold['case_names']:
        cur = gold[name + '_pos']
        for k in range(2):
            gran = gold[name + '_el_params'][k, 0]
            dims, axes, lo, step, hi = augment.elastic_grid(cur.min(0), cur.max(0), gran)
            assert tuple(dims) == gold['%s_el%d_noise' % (name, k)].shape[:3], (name, k)
            for a in range(3):
                want = gold['%s_el%d_ax%d' % (name, k, a)]
                assert np.array_equal(axes[a], want), (name, k, a)
                # the kernel's node rule: lo + i * step, the last node exactly hi
                node = lo[a] + np.arange(dims[a]) * step[a]
                node[-1] = hi[a]
                assert np.array_equal(node, want)
            cur = gold['%s_el%d_out' % (name, k)]
        cur = gold[name + '_pos']
        for k in range(2):
            gran = gold[name + '_ha_params'][k, 0]
            dims, axes, lo, step, hi = augment.hais_grid(np.abs(cur).max(0), gran)
            assert tuple(dims) == gold['%s_ha%d_noise' % (name, k)].shape[1:], (name, k)
            for a in range(3):
                assert np.array_equal(axes[a], gold['%s_ha%d_ax%d' % (name, k, a)]), (name, k, a)
            cur = gold['%s_ha%d_out' % (name, k)]
    flat = gold['flat_el0_noise'].shape
    assert flat[2] == 3                                     # a flat cloud: the minimum of three nodes on that axis
    with pytest.raises(ValueError):
        augment.hais_grid([1.0, 1.0, 1.0], 0.5)


def test_new_entries_reject_bad_arguments_without_a_device():
    lib = _lib.load()
    err = lambda: lib.b2m_last_error().decode()
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data_as(C.c_void_p)                      # (a host address: the checks return before anything reads it)
    assert lib.b2m_aug_stats(None, 10, p, p, None) < 0 and 'NULL' in err()
    assert lib.b2m_aug_stats(p, 0, p, p, None) < 0 and 'n must' in err()
    assert lib.b2m_aug_affine(p, None, 0, p, None, None, None, 1, None) < 0 and 'positive' in err()
    assert lib.b2m_aug_affine(p, None, 5, None, None, None, None, 1, None) < 0 and 'NULL' in err()
    assert lib.b2m_aug_axpy(p, None, 1.0, 5, None) < 0 and 'NULL' in err()
    assert lib.b2m_aug_axpy(p, p, 1.0, 0, None) < 0
    assert lib.b2m_aug_blur(p, p, 1, 3, 3, None) < 0 and '2 nodes' in err()
    assert lib.b2m_aug_blur(p, None, 3, 3, 3, None) < 0 and 'NULL' in err()
    assert lib.b2m_aug_displace(p, 5, p, 3, 3, 1, p, p, p, 1.0, None) < 0 and '2 nodes' in err()
    assert lib.b2m_aug_displace(p, 0, p, 3, 3, 3, p, p, p, 1.0, None) < 0 and 'positive' in err()
    assert lib.b2m_aug_displace(p, 5, p, 3, 3, 3, p, p, p, 1.0, None) < 0 and 'ascend' in err()     # zero steps
    assert lib.b2m_aug_displace(p, 5, None, 3, 3, 3, p, p, p, 1.0, None) < 0 and 'NULL' in err()
    assert lib.b2m_aug_vertex_normals(p, 0, p, 1, p, p, p, None) < 0
    assert lib.b2m_aug_vertex_normals(p, 4, None, 1, p, p, p, None) < 0 and 'NULL' in err()
    assert lib.b2m_aug_colour(p, 0, p, 1, 0.5, None, None, None) < 0
    assert lib.b2m_aug_colour(p, 5, None, 1, 0.5, None, None, None) < 0 and 'statistics' in err()
    assert lib.b2m_aug_colour(p, 5, p, 2, 0.5, None, None, None) < 0 and 'row' in err()
    assert lib.b2m_aug_colour(p, 5, p, 4, 0.5, None, None, None) < 0 and 'array' in err()
    assert lib.b2m_aug_colour(p, 5, p, 8, 0.5, None, None, None) < 0 and 'flags' in err()
    a = [p, p, p, 0, 1, p, p, p, p, p, p, p, p, p, None]
    assert lib.b2m_inst_boxes(*a) < 0 and 'n must' in err()
    a[3], a[4] = 5, 0
    assert lib.b2m_inst_boxes(*a) < 0 and 'n_inst' in err()
    a[4], a[13] = 2, None
    assert lib.b2m_inst_boxes(*a) < 0 and 'NULL' in err()


def test_the_product_has_no_cpu_path():
    import torch
    if torch.cuda.is_available():
        return
    sc = {'positions': np.zeros((4, 3)), 'colors': np.zeros((4, 3)), 'normals': np.zeros((4, 3)), 'segments': np.zeros(4, np.int64)}
    with pytest.raises(_lib.B2MError):
        augment.augment_scenes([sc], [augment.SceneAugment()])
    with pytest.raises(_lib.B2MError):
        augment.instance_labels(sc, np.zeros(4, np.int64), np.zeros(4, np.int64), np.zeros(1, np.int64))
