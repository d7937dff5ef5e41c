"""CPU: the rule of tests/_augment_rule.py is tied to the reference before the device is held to it, and the cases of
tests/_augment_cases.py are shown to have teeth.

  * On tests/golden/augment.npz and augment_steps.npz (written by the reference's own elastic_distortion / HAIS_elastic / Chromatic* /
    color_jittering / compute_bounding_box) the rule reproduces the reference within the tolerances tests/test_gpu_augment.py states
    for the device -- and exactly where the reference's order coincides with the rule's (instance-box centres, bounds, offsets,
    semantics, ids; clipped colours).
  * The mean of `stats` against math.fsum / n: 1.01 * (L + 17) * 2^-53 * sum|x| / n, L = ceil(n / (256 nb)) the per-thread chain,
    17 = 8 + 8 tree levels and the division (each a rounding of relative 2^-53 of a partial sum no larger than sum|x|).
  * Every deliberate mistake of the rule changes the case MUST_FAIL names for it.
  * The branch record of `displace` shows every branch taken on every axis."""
import math
import os

import numpy as np
import pytest

import _augment_cases as C
import _augment_rule as R


@pytest.fixture(scope='module')
def gold(golden_dir):
    out = {}
    for f in ('augment.npz', 'augment_steps.npz'):
        with np.load(os.path.join(golden_dir, f)) as z:
            out.update({k: z[k] for k in z.files})
    return out


def _steps(gold, name, kind):
    """As tests/test_gpu_augment.py: (input key, noise, blurred grid in (nx,ny,nz,3) layout, granularity, magnitude, output key)."""
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


# ----------------------------------------------------------------------------- the rule against the reference's outputs
def test_blur_rule_matches_scipy(gold):
    total = diff = 0
    for name in gold['case_names']:
        for kind in ('el', 'ha'):
            for _, noise, want, _, _, _ in _steps(gold, name, kind):
                got = R.blur(noise)
                assert got.shape == want.shape and got.dtype == np.float32
                assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want))), (name, kind)
                total += want.size
                diff += int((got != want).sum())
    print('blur rule: %d of %d elements differ from scipy' % (diff, total))
    assert diff <= 1e-3 * total


def test_displace_rule_matches_the_interpolator(gold):
    from box2mask_amd import augment
    for name in gold['case_names']:
        for kind in ('el', 'ha'):
            for src, _, blur, gran, mag, dst in _steps(gold, name, kind):
                cur = gold[src]
                if kind == 'el':
                    dims, _, lo, step, hi = augment.elastic_grid(cur.min(0), cur.max(0), gran)
                else:
                    dims, _, lo, step, hi = augment.hais_grid(np.abs(cur).max(0), gran)
                got = R.displace(cur, blur, lo, step, hi, dims, mag)[0]
                err = np.abs(got - gold[dst]).max()
                assert err <= 1e-9 * max(1.0, mag), (name, kind, err)
    grid, lo, hi, pts, mag = gold['tri_grid'], gold['tri_lo'], gold['tri_hi'], gold['tri_pts'], float(gold['tri_mag'])
    step = np.array([np.linspace(a, b, d, retstep=True)[1] for a, b, d in zip(lo, hi, grid.shape[:3])])
    got, br = R.displace(pts, grid, lo, step, hi, grid.shape[:3], mag)
    assert np.abs(got - gold['tri_out']).max() <= 1e-9 * max(1.0, mag)
    outside = np.any((pts < lo) | (pts > hi), axis=1)
    assert np.array_equal(got[outside], pts[outside]) and not br[outside].any()
    assert np.any(got[0] != pts[0]) and np.any(got[3] != pts[3])            # on the last node: inside


def _ulp_close(got, want, ulps):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    return np.all(np.abs(got[~nan] - want[~nan]) <= ulps * np.spacing(np.abs(want[~nan])))


@pytest.mark.parametrize('name', ['col', 'colconst'])
def test_colour_rule_matches_the_reference(gold, name):
    blend, tr, jit = float(gold[name + '_blend']), gold[name + '_tr'].reshape(3), gold[name + '_jitter']
    stages = [(name + '_in', 1, name + '_contrast'), (name + '_contrast', 2, name + '_translation'),
              (name + '_translation', 4, name + '_jittered')]
    for src, flag, dst in stages + [(name + '_in', 7, name + '_jittered')]:
        got = R.colour(gold[src], R.stats(gold[src])[0], flag, blend, tr, jit)
        want = gold[dst]
        assert _ulp_close(got, want, 4), dst
        clipped = (want == 0) | (want == 1)
        assert np.array_equal(got[clipped], want[clipped])
        assert flag == 1 or clipped.any()
    if name == 'colconst':
        assert np.isnan(gold[name + '_contrast'][:, 1]).all()


def test_box_rule_matches_compute_bounding_box(gold):
    pos, inst, sem = gold['box_pos'], gold['box_instances'], gold['box_semantics']
    w = R.inst_boxes(pos, inst, sem, 9)
    assert w['missing'] == 0
    exact = {'per_instance_bb_centers': w['per_centers'], 'per_instance_bb_bounds': w['per_bounds'], 'bb_centers': w['per_centers'][inst],
             'bb_bounds': w['per_bounds'][inst], 'bb_offsets': w['offsets'], 'per_instance_semantics': w['per_sem']}
    for k, got in exact.items():
        assert got.dtype == gold['box_' + k].dtype and np.array_equal(got, gold['box_' + k]), k
    assert np.array_equal(np.arange(9), gold['box_unique_instances'])
    close = {'per_instance_bb_radius': w['per_radius'], 'bb_radius': w['per_radius'][inst][:, None], 'bb_center_distances': w['distances'][:, None]}
    for k, got in close.items():
        want = gold['box_' + k]
        assert got.shape == want.shape and got.dtype == np.float32, k
        assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(want)), k


def test_affine_and_normal_rules_match_numpy():
    """No reference output exists for these (open3d): the rule against plain numpy at 1e-12, as tests/test_gpu_augment.py holds
    the device."""
    c = C.affine_case('n:257')
    ctr = C.affine_centre(c)
    got, nrm = R.affine(c.pos, c.normals, c.M, ctr, c.t, c.recentre)
    assert np.abs(got - ((c.pos - ctr) @ c.M.T + ctr + c.t)).max() <= 1e-12
    cof = np.linalg.det(c.M) * np.linalg.inv(c.M).T
    want = c.normals @ cof.T
    assert np.abs(nrm - want / np.linalg.norm(want, axis=1, keepdims=True)).max() <= 1e-12
    assert np.abs(R.cofactor(c.M) - cof).max() <= 1e-12
    v = C.normals_case('n:257')
    fn = np.cross(v.pos[v.faces[:, 1]] - v.pos[v.faces[:, 0]], v.pos[v.faces[:, 2]] - v.pos[v.faces[:, 0]])
    acc = np.zeros_like(v.pos)
    for k in range(3):
        np.add.at(acc, v.faces[:, k], fn)
    length = np.linalg.norm(acc, axis=1, keepdims=True)
    want = np.where(length > 0, acc / np.where(length > 0, length, 1), [[0.0, 0.0, 1.0]])
    assert np.abs(R.vertex_normals(v.pos, v.faces) - want).max() <= 1e-12


# ----------------------------------------------------------------------------- the mean's bound
@pytest.mark.parametrize('name', C.STATS_CASES)
def test_stats_mean_within_its_bound(name):
    x = C.stats_case(name).x
    n = len(x)
    got, fmean = R.stats(x)
    if name == 'nan_row':
        assert np.isnan(got[0:3]).all() and np.isnan(fmean).all()
        return
    L = R.chain_length(n)
    for c in range(3):
        bound = 1.01 * (L + 17) * 2.0 ** -53 * math.fsum(np.abs(x[:, c])) / n
        err = abs(got[c] - math.fsum(x[:, c]) / n)
        assert err <= bound, (name, c, err, bound)
        assert fmean[c] == math.fsum(x[:, c]) / n
    assert np.array_equal(got[3:6], x.min(0)) and np.array_equal(got[6:9], x.max(0)) and np.array_equal(got[9:12], np.abs(x).max(0))


# ----------------------------------------------------------------------------- every case is built; its predicates hold
ALL_CASES = [(C.stats_case, C.STATS_CASES), (C.affine_case, C.AFFINE_CASES), (C.axpy_case, C.AXPY_CASES), (C.blur_case, C.BLUR_CASES),
             (C.displace_case, C.DISPLACE_CASES), (C.normals_case, C.NORMALS_CASES), (C.colour_case, C.COLOUR_CASES),
             (C.box_case, C.BOX_CASES)]


def test_every_case_builds_and_reaches_its_edge():
    for fn, names in ALL_CASES:
        assert len(set(names)) == len(names)
        for n in names:
            c = fn(n)
            assert c.name == n and all(c.predicates.values()), (n, c.predicates)


def test_every_displace_branch_is_taken_on_every_axis():
    """The search of _augment_cases._axis_search found all three: nothing is left out as unreachable."""
    for what, bit in (('down', R.DOWN), ('up', R.UP), ('last', R.LAST)):
        c = C.displace_case('branch:' + what)
        for a in range(3):
            assert (c.branch[:, a] & bit).any(), (what, a)
        if what == 'last':
            assert np.all(c.hi != c.lo + (c.n - 1) * c.step)
    c = C.displace_case('nodes')
    assert (c.branch == 0).any() and (c.branch & R.LAST).any()


# ----------------------------------------------------------------------------- the deliberate mistakes
MUST_FAIL = {
    'blur_tap_order': 'absorb', 'blur_reflect': 'impulse:corner', 'blur_5_passes': 'noise:3x3x3', 'blur_round_each_tap': 'noise:2x3x129',
    'displace_no_down': 'branch:down', 'displace_no_up': 'branch:up', 'displace_last_from_step': 'branch:last',
    'displace_lt_hi': 'nodes', 'displace_strides_swapped': 'nodes',
    'stats_sequential': 'n:4097', 'stats_nb_256': 'n:4097', 'stats_no_stride': 'n:257',
    'normals_descending': 'fan300', 'normals_zero_fallback': 'isolated',
    'affine_no_recentre': 'n:257', 'affine_cofactor_transposed': 'n:257',
    'colour_stage_order': 'flags:3', 'colour_clip_before_add': 'flags:2',
    'boxes_sem_highest': 'shuffled_sem', 'boxes_radius_f32': 'I:257', 'boxes_bound_half_extent': 'far',
    'boxes_count_out_of_range': 'out_of_range',
}


def _run(entry, name, mistake=None):
    """The rule's outputs of one case, as a list of arrays."""
    if entry == 'blur':
        return [R.blur(C.blur_case(name).grid, mistake)]
    if entry == 'displace':
        c = C.displace_case(name)
        return [R.displace(c.pos, c.grid, c.lo, c.step, c.hi, c.n, c.magnitude, mistake)[0]]
    if entry == 'stats':
        return [R.stats(C.stats_case(name).x, mistake)[0]]
    if entry == 'normals':
        c = C.normals_case(name)
        return [R.vertex_normals(c.pos, c.faces, c.row_ptr, c.face_of, mistake)]
    if entry == 'affine':
        c = C.affine_case(name)
        return list(R.affine(c.pos, c.normals, c.M, C.affine_centre(c), c.t, c.recentre, mistake))
    if entry == 'colour':
        c = C.colour_case(name)
        return [R.colour(c.col, R.stats(c.col)[0], c.flags, c.blend, c.tr, c.jitter, mistake)]
    c = C.box_case(name)
    w = R.inst_boxes(c.pos, c.inst, c.sem, c.n_inst, mistake)
    return [np.asarray(w[k]) for k in sorted(w)]


def _same(a, b):
    return all((x is None and y is None) or R.same_bits(x, y) for x, y in zip(a, b))


def test_the_mistake_table_is_complete():
    assert set(MUST_FAIL) == set(R.MISTAKES) and len(R.MISTAKES) == 22


@pytest.mark.parametrize('mistake', R.MISTAKES)
def test_every_mistake_changes_its_named_case(mistake):
    entry = mistake.split('_')[0]
    name = MUST_FAIL[mistake]
    right = _run(entry, name)
    assert _same(right, _run(entry, name)), 'the rule is a function of its inputs'
    assert not _same(right, _run(entry, name, mistake)), (mistake, name)
