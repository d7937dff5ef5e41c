"""GPU parity of box2mask_amd/augment.py (box2mask_amd/csrc/augment.hip) against tests/golden/augment.npz, which the
reference's own elastic_distortion / HAIS_elastic / Chromatic* / color_jittering / compute_bounding_box wrote
(tools/gen_golden.py augment), and against fp64 numpy restatements where open3d would be the reference (affine maps, normals).

Bounds (none of them measured on the code under test):
  blur       every element within 1 fp32 ulp, at most 1e-3 of the elements different at all (numpy restatements of the same
             fp64 sums reproduce scipy's grid with 0 mismatches);
  trilinear  1e-9 * max(1, magnitude), fed the fixture's blurred grid (two fp64 formulations differ by 6.4e-16 at magnitude 1);
  whole step magnitude * 2^-20: one fp32 ulp of a noise value below 8 through a convex combination, times 2;
  colour     4 fp64 ulp, clipped values exactly 0 or 1;
  boxes      per-instance centres / bounds / semantics / ids bit-equal, radius and per-point distances within 1 fp32 ulp;
  affine     1e-12 against numpy fp64."""
import os

import numpy as np
import pytest
import torch

import _augment_rule as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gold(golden_dir):
    """augment.npz and, merged in, augment_steps.npz (the per-step outputs of the 5000-point case: a file of their own for
    the size limit of a committed file)."""
    out = {}
    for f in ('augment.npz', 'augment_steps.npz'):
        with np.load(os.path.join(golden_dir, f)) as z:
            out.update({k: z[k] for k in z.files})
    return out


def _d(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda', dtype).contiguous()


def _n(t):
    return t.cpu().numpy()


def _scene(pos, faces=None, rng=None):
    rng = np.random.default_rng(0) if rng is None else rng
    P = len(pos)
    nrm = rng.standard_normal((P, 3))
    sc = {'positions': pos, 'colors': rng.random((P, 3)), 'normals': nrm / np.linalg.norm(nrm, axis=1, keepdims=True),
          'segments': np.arange(P, dtype=np.int64) // 4}
    if faces is not None:
        sc['faces'] = faces
    return sc


def _steps(gold, name, kind):
    """(input key, noise, blurred grid in (nx,ny,nz,3) layout, granularity, magnitude, output key) of both steps."""
    out = []
    prev = name + '_pos'
    for k in range(2):
        tag = '%s_%s%d' % (name, kind, k)
        noise, blur = gold[tag + '_noise'], gold[tag + '_blur']
        if kind == 'ha':
            noise, blur = np.moveaxis(noise, 0, -1), np.moveaxis(blur, 0, -1)
        gran, mag = gold['%s_%s_params' % (name, kind)][k]
        out.append((prev, np.ascontiguousarray(noise), np.ascontiguousarray(blur), float(gran), float(mag), tag + '_out'))
        prev = tag + '_out'
    return out


def test_case_list_covers_the_sizes(gold):
    sizes = {len(gold[n + '_pos']) for n in gold['case_names']}
    assert {1, 63, 64, 65, 1000, 5000} <= sizes
    assert np.ptp(gold['flat_pos'][:, 2]) == 0 and gold['flat_el0_noise'].shape[2] == 3
    assert gold['neg_pos'].min() < 0


def test_blur_matches_scipy(gold):
    from box2mask_amd import augment
    total = diff = 0
    for name in gold['case_names']:
        for kind in ('el', 'ha'):
            for _, noise, want, _, _, _ in _steps(gold, name, kind):
                got = _n(augment.blur_(_d(noise, torch.float32)))
                assert got.shape == want.shape and got.dtype == np.float32
                assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want))), (name, kind)
                assert R.same_bits(got, R.blur(noise)), (name, kind, 'the rule of tests/_augment_rule.py, bit for bit')
                total += want.size
                diff += int((got != want).sum())
    print('blur: %d of %d elements differ' % (diff, total))
    assert diff <= 1e-3 * total


def test_trilinear_on_the_reference_grid(gold):
    from box2mask_amd import augment
    worst = 0.0
    for name in gold['case_names']:
        for kind in ('el', 'ha'):
            for src, _, blur, gran, mag, dst in _steps(gold, name, kind):
                cur = gold[src]
                if kind == 'el':
                    dims, _, lo, step, hi = augment.elastic_grid(cur.min(0), cur.max(0), gran)
                else:
                    dims, _, lo, step, hi = augment.hais_grid(np.abs(cur).max(0), gran)
                pos = _d(cur)
                augment.displace_(pos, _d(blur, torch.float32), lo, step, hi, mag)
                err = np.abs(_n(pos) - gold[dst]).max()
                assert R.same_bits(_n(pos), R.displace(cur, blur, lo, step, hi, dims, mag)[0]), (name, kind, 'the rule, bit for bit')
                worst = max(worst, err / max(1.0, mag))
                assert err <= 1e-9 * max(1.0, mag), (name, kind, err)
    print('trilinear: worst error / max(1, magnitude) = %.3g' % worst)


def test_trilinear_outside_points_and_last_node(gold):
    from box2mask_amd import augment
    grid, lo, hi, pts, mag = gold['tri_grid'], gold['tri_lo'], gold['tri_hi'], gold['tri_pts'], float(gold['tri_mag'])
    step = np.array([np.linspace(a, b, d, retstep=True)[1] for a, b, d in zip(lo, hi, grid.shape[:3])])
    pos = _d(pts)
    augment.displace_(pos, _d(grid, torch.float32), lo, step, hi, mag)
    got, want = _n(pos), gold['tri_out']
    assert np.abs(got - want).max() <= 1e-9 * max(1.0, mag)
    outside = np.any((pts < lo) | (pts > hi), axis=1)
    assert outside[6:12].all() and not outside[:6].any()
    assert np.array_equal(got[outside], pts[outside])                       # zero displacement, to the bit
    assert np.array_equal(want[outside], pts[outside])
    assert np.any(got[0] != pts[0]) and np.any(got[3] != pts[3])            # on the last node: inside


def test_whole_elastic_and_hais_steps(gold):
    """Device blur + displacement from the recorded noise, chained as read_scene chains them; all cases in one batch."""
    from box2mask_amd import augment
    names = list(gold['case_names'])
    scenes, prm_el, prm_el0, prm_ha = [], [], [], []
    for name in names:
        scenes.append(_scene(gold[name + '_pos']))
        el, ha = _steps(gold, name, 'el'), _steps(gold, name, 'ha')
        prm_el.append(augment.SceneAugment(geometric=[('elastic', s[3], s[4], s[1]) for s in el]))
        prm_el0.append(augment.SceneAugment(geometric=[('elastic', el[0][3], el[0][4], el[0][1])]))
        prm_ha.append(augment.SceneAugment(geometric=[('hais', s[3], s[4], np.moveaxis(s[1], -1, 0)) for s in ha] + [('shift_min',)]))
    out_el = augment.augment_scenes(scenes, prm_el)
    out_el0 = augment.augment_scenes(scenes, prm_el0)
    out_ha = augment.augment_scenes(scenes, prm_ha)
    for i, name in enumerate(names):
        assert np.array_equal(scenes[i]['positions'], gold[name + '_pos'])                         # inputs are not written
        mag = gold[name + '_el_params'][:, 1]
        err = np.abs(_n(out_el[i]['positions']) - gold[name + '_el1_out']).max()
        assert err <= mag[1] * 2.0 ** -20, (name, 'elastic chain', err)
        err = np.abs(_n(out_el0[i]['positions']) - gold[name + '_el0_out']).max()
        assert err <= mag[0] * 2.0 ** -20, (name, 'elastic step', err)
        got = _n(out_ha[i]['positions'])
        err = np.abs(got - gold[name + '_ha_final']).max()
        assert err <= gold[name + '_ha_params'][1, 1] * 2.0 ** -20, (name, 'hais chain', err)
        assert got.min() == 0.0
    with pytest.raises(ValueError, match='noise array'):
        augment.augment_scenes(scenes[:1], [augment.SceneAugment(geometric=[('elastic', 0.2, 0.4, np.zeros((2, 2, 2, 3), np.float32))])])


def _ulp_close(got, want, ulps):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    return np.all(np.abs(got[~nan] - want[~nan]) <= ulps * np.spacing(np.abs(want[~nan])))


@pytest.mark.parametrize('name', ['col', 'colconst'])
def test_colour_steps(gold, name):
    from box2mask_amd import augment
    stages = [(name + '_in', [('auto_contrast', float(gold[name + '_blend']))], name + '_contrast'),
              (name + '_contrast', [('translation', gold[name + '_tr'].reshape(3))], name + '_translation'),
              (name + '_translation', [('jitter', -0.1, 0.1, gold[name + '_jitter'])], name + '_jittered')]
    rule_args = (float(gold[name + '_blend']), gold[name + '_tr'].reshape(3), gold[name + '_jitter'])
    for flag, (src, steps, dst) in zip((1, 2, 4), stages):
        got = _n(augment.colour_(_d(gold[src]), steps))
        want = gold[dst]
        assert _ulp_close(got, want, 4), dst
        assert R.same_bits(got, R.colour(gold[src], R.stats(gold[src])[0], flag, *rule_args)), (dst, 'the rule, bit for bit')
        clipped = (want == 0) | (want == 1)
        assert np.array_equal(got[clipped], want[clipped])
    # the fused pass: all three at once, against the reference's chain
    got = _n(augment.colour_(_d(gold[name + '_in']), [s[1][0] for s in stages]))
    want = gold[name + '_jittered']
    assert _ulp_close(got, want, 4)
    assert R.same_bits(got, R.colour(gold[name + '_in'], R.stats(gold[name + '_in'])[0], 7, *rule_args)), 'the rule, bit for bit'
    clipped = (want == 0) | (want == 1)
    assert clipped.any() and np.array_equal(got[clipped], want[clipped])
    if name == 'colconst':
        assert np.isnan(gold[name + '_contrast'][:, 1]).all()               # 0 * inf, as numpy gives it


def test_instance_boxes_match_compute_bounding_box(gold):
    from box2mask_amd import augment
    pos, inst, sem = gold['box_pos'], gold['box_instances'], gold['box_semantics']
    seg2inst = np.arange(4)
    lab = augment.instance_labels({'positions': pos}, sem, inst, seg2inst)
    assert (inst == 8).sum() == 1                                           # an instance of one point
    for k in ('per_instance_bb_centers', 'per_instance_bb_bounds', 'bb_centers', 'bb_bounds', 'bb_offsets'):
        got = _n(lab[k])
        assert got.dtype == np.float32 and np.array_equal(got, gold['box_' + k]), k
    assert np.array_equal(_n(lab['per_instance_semantics']), gold['box_per_instance_semantics'])
    assert _n(lab['per_instance_semantics']).dtype == np.int32
    assert np.array_equal(_n(lab['unique_instances']), gold['box_unique_instances'])
    for k in ('per_instance_bb_radius', 'bb_radius', 'bb_center_distances'):
        got, want = _n(lab[k]), gold['box_' + k]
        assert got.shape == want.shape and got.dtype == np.float32, k
        assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(want)), k
    rule = R.inst_boxes(pos, inst, sem, 9)                                  # ... and the rule's order, bit for bit
    assert R.same_bits(_n(lab['per_instance_bb_radius']), rule['per_radius'])
    assert R.same_bits(_n(lab['bb_radius']), rule['per_radius'][inst][:, None])
    assert R.same_bits(_n(lab['bb_center_distances']), rule['distances'][:, None])
    assert np.array_equal(_n(lab['semantics']), sem) and np.array_equal(_n(lab['instances']), inst) and lab['seg2inst'] is seg2inst
    gappy = inst.copy()
    gappy[gappy == 4] = 3                                                   # ids 0..8 without 4
    with pytest.raises(ValueError, match='dense'):
        augment.instance_labels({'positions': pos}, sem, gappy, seg2inst)
    with pytest.raises(ValueError, match='dense'):
        augment.instance_labels({'positions': pos}, sem, inst - 1, seg2inst)


def _grid_mesh(n=30):
    """n x n vertices of a bumpy height field, two triangles per cell, plus one vertex no face uses."""
    u, v = np.meshgrid(np.linspace(0, 2, n), np.linspace(-1, 1, n), indexing='ij')
    pos = np.stack([u, v, 0.3 * np.sin(3 * u) * np.cos(2 * v)], -1).reshape(-1, 3)
    pos = np.concatenate([pos, [[5.0, 5.0, 5.0]]])
    i = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None]).reshape(-1)
    faces = np.concatenate([np.stack([i, i + n, i + 1], 1), np.stack([i + 1, i + n, i + n + 1], 1)]).astype(np.int64)
    return pos, faces


def _np_vertex_normals(pos, faces):
    """The documented open3d rule: sum of the faces' unnormalised cross products per vertex, normalised; zero -> (0,0,1)."""
    fn = np.cross(pos[faces[:, 1]] - pos[faces[:, 0]], pos[faces[:, 2]] - pos[faces[:, 0]])
    acc = np.zeros_like(pos)
    for c in range(3):
        np.add.at(acc, faces[:, c], fn)
    length = np.linalg.norm(acc, axis=1, keepdims=True)
    out = np.where(length > 0, acc / np.where(length > 0, length, 1), [[0.0, 0.0, 1.0]])
    return out


def test_affine_positions_and_normals(gold):
    from box2mask_amd import augment
    rng = np.random.default_rng(3)
    pos, faces = _grid_mesh()
    csr = augment.vertex_face_csr(_d(faces, torch.int64), len(pos))
    n0 = _n(augment.vertex_normals(_d(pos), _d(faces, torch.int64), csr))
    want0 = _np_vertex_normals(pos, faces)
    assert np.abs(n0 - want0).max() <= 1e-12
    assert np.array_equal(n0[-1], [0.0, 0.0, 1.0]) and abs(np.linalg.norm(n0[5]) - 1) < 1e-12          # the isolated vertex
    # a purely affine chain with a mirror, a shear and every kind of centre
    m1 = augment._rot_xyz(0.02, -0.01, 1.1)
    m2 = np.diag([-1.0, 1.0, 1.0])
    m3 = np.eye(3) + rng.standard_normal((3, 3)) * 0.1
    m4 = np.eye(3) * 1.17
    t = np.array([0.3, -0.2, 0.05])
    c3 = np.array([0.5, 0.25, -1.0])
    steps = [('affine', m1, 'mean', np.zeros(3)), ('affine', m2, 'origin', t), ('affine', m3, 'mean', np.zeros(3), False),
             ('affine', m4, c3, np.zeros(3))]
    sc = _scene(pos, faces)
    sc['normals'] = n0.copy()
    out = augment.augment_scenes([sc], [augment.SceneAugment(geometric=steps)])[0]
    w = pos.copy()
    c = w.mean(0); w = (w - c) @ m1.T + c
    w = w @ m2.T + t
    w = (w - w.mean(0)) @ m3.T
    w = (w - c3) @ m4.T + c3
    got = _n(out['positions'])
    assert np.abs(got - w).max() <= 1e-12
    # cofactor path == normals recomputed from the faces of the transformed mesh (det < 0: the mirror flips the winding)
    assert np.linalg.det(m4 @ m3 @ m2 @ m1) < 0
    from_faces = _n(augment.vertex_normals(out['positions'], _d(faces, torch.int64), csr))
    cof = _n(out['normals'])
    used = np.ones(len(pos), bool); used[-1] = False
    assert np.abs(cof[used] - from_faces[used]).max() <= 1e-12
    assert np.abs(from_faces - _np_vertex_normals(got, faces)).max() <= 1e-12
    # a non-affine step with faces: normals come from the faces of the final positions; the CSR is cached on the scene
    prm = augment.SceneAugment(geometric=[('affine', m2, 'origin', np.zeros(3)), ('jitter', 0.001, 7)])
    out = augment.augment_scenes([sc], [prm])[0]
    assert '_face_csr' in sc
    assert np.abs(_n(out['normals']) - _np_vertex_normals(_n(out['positions']), faces)).max() <= 1e-12
    assert 0 < np.abs(_n(out['positions']) - pos @ m2.T).max() < 0.01
    # two fresh scenes with faces in one batch: both CSRs are built and cached, each equal to the one built alone
    pair = [_scene(pos, faces), _scene(pos[::-1].copy(), (len(pos) - 1 - faces))]
    outs = augment.augment_scenes(pair, [prm, prm])
    for sc_i, o in zip(pair, outs):
        assert '_face_csr' in sc_i
        alone = augment.vertex_face_csr(_d(sc_i['faces'], torch.int64), len(pos))
        assert all(torch.equal(a, b) for a, b in zip(sc_i['_face_csr'], alone))
        assert np.abs(_n(o['normals']) - _np_vertex_normals(_n(o['positions']), sc_i['faces'])).max() <= 1e-12
    bad = _scene(pos, faces + 2)
    with pytest.raises(ValueError, match='faces'):
        augment.augment_scenes([_scene(pos, faces), bad], [prm, prm])
    assert '_face_csr' not in bad
    # without faces the normals keep their affine transform
    sc2 = _scene(pos)
    out2 = augment.augment_scenes([sc2], [prm])[0]
    cof2 = np.linalg.det(m2) * np.linalg.inv(m2).T                                      # = -m2: the winding is not reordered
    assert np.abs(_n(out2['normals']) - sc2['normals'] @ cof2.T).max() <= 1e-12
    with pytest.raises(ValueError, match='faces'):
        augment.vertex_face_csr(_d(faces + 2, torch.int64), len(pos))          # (+ 1 would still reach the isolated last vertex)


def _scannet_like_cfg():
    from box2mask_amd.config import scannet_config
    return scannet_config(augmentation=True, rotation_90_aug=True, flipping_aug=0.5, scaling_aug=[1.0, 0.8, 1.2],
                          elastic_distortion=1.0, elastic_distortion_HAIS=1.0, position_jittering=[1.0, 0.005],
                          chromatic_auto_contrast=1.0, chromatic_translation=[1.0, 0.1], color_jittering_aug=[1.0, 0.05])


def _synth_scenes():
    from box2mask_amd import synth
    scenes = []
    for seed in (3, 4):
        sc = synth.make_scene(seed, target_voxels=3000, points_only=True, pts_per_m2=8000.0)
        sc['colors'] = np.random.default_rng(seed).random(sc['colors'].shape)
        scenes.append(sc)
    return scenes


def _labels_of(scene_out, raw):
    from box2mask_amd import augment
    lab = raw['labels']
    inst = lab['seg2inst'][raw['segments']]
    return augment.instance_labels(scene_out, lab['per_instance_semantics'][inst], inst, lab['seg2inst'])


def test_two_runs_give_the_same_bits():
    from box2mask_amd import augment
    raws = _synth_scenes()
    prm = [augment.draw_params(_scannet_like_cfg(), generator=np.random.default_rng(20 + i)) for i in range(2)]
    assert all(len(p.geometric) >= 7 and len(p.colour) >= 2 for p in prm)
    runs = []
    for _ in range(2):
        outs = augment.augment_scenes(raws, prm)
        labs = [_labels_of(o, r) for o, r in zip(outs, raws)]
        runs.append((outs, labs))
    for (o1, l1), (o2, l2) in zip(zip(*runs[0]), zip(*runs[1])):
        for k in ('positions', 'normals', 'colors', 'segments'):
            assert torch.equal(o1[k], o2[k]), k
        for k, v in l1.items():
            if torch.is_tensor(v):
                assert torch.equal(v, l2[k]), k
    moved = _n(runs[0][0][0]['positions']) - raws[0]['positions']
    assert np.abs(moved).max() > 0.01                                      # it did something


def test_empty_params_leave_the_batch_bit_identical():
    from types import SimpleNamespace
    from box2mask_amd import augment, prepare
    from box2mask_amd.config import scannet_config
    raws = _synth_scenes()
    sup = SimpleNamespace(smallest_bb_heuristic=True)

    def batch(scenes):
        items = prepare.voxelize_scenes(scenes, 0.02)
        for it, raw in zip(items, raws):
            prepare.box_supervision(it, raw['labels'], sup)
        return prepare.collate(items, 'train')
    plain = batch(raws)
    aug = batch(augment.augment_scenes(raws, [augment.SceneAugment(), augment.draw_params(scannet_config())]))
    for k in ('vox_coords', 'vox_features', 'batch_ids', 'input_location', 'pooling_ids', 'gt_bb_bounds', 'gt_bb_offsets',
              'gt_semantics', 'fg_instances'):
        assert plain[k].dtype == aug[k].dtype and torch.equal(plain[k], aug[k]), k


def test_augmented_batch_trains():
    """ScanNet-config parameters, labels recomputed by instance_labels, one training step with finite losses."""
    from types import SimpleNamespace
    from box2mask_amd import augment, prepare, synth
    from box2mask_amd.config import scannet_config
    from box2mask_amd.model import Model
    raws = _synth_scenes()
    cfg = scannet_config(augmentation=True, rotation_90_aug=True, flipping_aug=0.5, scaling_aug=[1.0, 0.8, 1.2])   # configs/scannet.txt
    prm = [augment.draw_params(cfg, generator=np.random.default_rng(40 + i)) for i in range(2)]
    outs = augment.augment_scenes(raws, prm)
    items = prepare.voxelize_scenes(outs, 0.02)
    for it, o, raw in zip(items, outs, raws):
        lab = _labels_of(o, raw)
        # the recomputed boxes hold their instances' augmented points
        inst = _n(lab['instances'])
        p = _n(o['positions'])
        lo = _n(lab['per_instance_bb_centers']).astype(np.float64) - _n(lab['per_instance_bb_bounds']).astype(np.float64)
        assert np.all(p >= lo[inst] - 1e-5)
        prepare.box_supervision(it, lab, SimpleNamespace(smallest_bb_heuristic=True))
    batch = prepare.collate(items, 'train')
    torch.manual_seed(0)
    model = Model(scannet_config(), *synth.scannet_tables())
    model.train()
    losses = model.compute_loss(batch, 150)
    losses['optimization_loss'].backward()
    assert torch.isfinite(losses['optimization_loss'])
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
