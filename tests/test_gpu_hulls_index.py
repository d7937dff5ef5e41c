"""GPU: b2m_mask_hulls_index / _batch (csrc/detbox.hip) -- b2m_mask_hulls for masks that live on voxels and are asked about on
points -- against ``_detbox_rule.hulls_rule`` over the masks expanded through the index on the host.  count, box6, ncand, n_hull,
flags and the hull vertices in their order are compared bit for bit; every output starts as a sentinel, carries 64 sentinel
elements behind it and keeps the sentinel where nothing is reported.  No case provokes a fault: an index outside [0, n_vox) is
part of the contract (such a point is in no mask)."""
import numpy as np
import pytest
import torch

from box2mask_amd import _lib
from box2mask_amd._lib import ptr

import _cluster_rule as C
import _detbox_rule as D

pytestmark = pytest.mark.gpu
PAD = 64
S32, SF = -77, -7.25
KEYS = ('count', 'box6', 'hull', 'n_hull', 'flags', 'ncand')
DESC = 17                                                                    # B2M_HULLIDX_DESC


def expand(case):
    """(k, n_pts) bool: point p is in row r iff voxel index[p] is, a point that names no voxel is in no row."""
    vm, n_pts = np.asarray(case['vmasks'], bool), len(case['pos'])
    idx = np.arange(n_pts, dtype=np.int64) if case['index'] is None else np.asarray(case['index'], np.int64)
    ok = (idx >= 0) & (idx < vm.shape[1])
    out = np.zeros((len(vm), n_pts), bool)
    out[:, ok] = vm[:, idx[ok]]
    return out


def _buf(n, dtype, sentinel):
    return torch.full((n + PAD,), sentinel, dtype=dtype, device='cuda')


def _take(t, n, sentinel):
    host = t.cpu().numpy()
    assert (host[n:] == sentinel).all(), 'written past the end'
    return host[:n]


def _alloc(case):
    """Device buffers of one scene: inputs, scratch and sentinel-filled outputs."""
    vm = np.asarray(case['vmasks'], bool)
    k, n_vox = vm.shape
    n_pts, cap = len(case['pos']), case['cap']
    words, pw = (n_vox + 63) // 64, (n_pts + 63) // 64
    d = dict(k=k, n_vox=n_vox, n_pts=n_pts, words=words, cap=cap)
    d['bits'] = torch.from_numpy(C.pack_rows(vm, pad=case['pad']).view(np.int64)).cuda() if k and words else None
    d['index'] = None if case['index'] is None else torch.from_numpy(np.ascontiguousarray(case['index'], np.int64)).cuda()
    d['pos'] = torch.from_numpy(np.ascontiguousarray(case['pos'], np.float64)).cuda()
    d['pbits'] = torch.full((max(k * pw, 1),), -1, dtype=torch.int64, device='cuda')      # (set bits everywhere: all are rewritten)
    d['work'] = torch.empty(max(k, 1) * D.HULL_CHUNKS * 56, dtype=torch.float64, device='cuda')
    d['cand'] = torch.empty(max(k, 1) * cap * 2, dtype=torch.float64, device='cuda')
    d['stk'] = torch.empty(max(k, 1) * cap, dtype=torch.int32, device='cuda')
    d['out'] = {'count': _buf(k, torch.int32, S32), 'box6': _buf(k * 6, torch.float64, SF),
                'hull': _buf(k * D.HULL_MAX * 2, torch.float64, SF), 'n_hull': _buf(k, torch.int32, S32),
                'flags': _buf(k, torch.int32, S32), 'ncand': _buf(k, torch.int32, S32)}
    return d


def _read(d):
    k, o = d['k'], d['out']
    return {'count': _take(o['count'], k, S32), 'box6': _take(o['box6'], k * 6, SF).reshape(k, 6),
            'hull': _take(o['hull'], k * D.HULL_MAX * 2, SF).reshape(k, D.HULL_MAX, 2), 'n_hull': _take(o['n_hull'], k, S32),
            'flags': _take(o['flags'], k, S32), 'ncand': _take(o['ncand'], k, S32)}


def _single(case):
    d = _alloc(case)
    o = d['out']
    _lib.call('b2m_mask_hulls_index', ptr(d['bits']), d['words'], d['k'], d['n_vox'], ptr(d['index']), ptr(d['pos']), d['n_pts'],
              ptr(d['pbits']), ptr(d['work']), ptr(d['cand']), ptr(d['stk']), d['cap'], ptr(o['ncand']), ptr(o['count']), ptr(o['box6']),
              ptr(o['hull']), ptr(o['n_hull']), ptr(o['flags']))
    return _read(d)


def _batch(cases):
    ds = [_alloc(c) for c in cases]
    assert len({d['cap'] for d in ds}) == 1
    rec = np.zeros((len(ds), DESC), np.int64)
    for s, d in enumerate(ds):
        o = d['out']
        rec[s] = [v or 0 for v in (                                         # (None: a NULL pointer)
            ptr(d['bits']), d['k'], d['words'], d['n_vox'], ptr(d['index']), ptr(d['pos']), d['n_pts'], ptr(d['pbits']),
            ptr(d['work']), ptr(d['cand']), ptr(d['stk']), ptr(o['ncand']), ptr(o['count']), ptr(o['box6']), ptr(o['hull']),
            ptr(o['n_hull']), ptr(o['flags']))]
    desc = torch.from_numpy(rec.reshape(-1)).cuda()
    _lib.call('b2m_mask_hulls_index_batch', ptr(desc), len(ds), ds[0]['cap'], max(d['k'] for d in ds), max(d['n_pts'] for d in ds))
    return [_read(d) for d in ds]


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _against_rule(got, case):
    want = D.hulls_rule(expand(case), np.asarray(case['pos'], np.float64).reshape(-1, 3), case['cap'])
    for key in ('count', 'ncand', 'n_hull', 'flags'):
        assert np.array_equal(got[key], want[key]), (key, got[key], want[key])
    assert _bits_equal(got['box6'], want['box6'])
    for r, h in enumerate(want['hulls']):
        m = 0 if h is None else len(h)
        if m:
            assert _bits_equal(got['hull'][r, :m], h), r
        assert (got['hull'][r, m:] == SF).all(), r                           # nothing behind it; nothing at all for a flagged row
    return want


def _check(case):
    got = _single(case)
    return got, _against_rule(got, case)


# ------------------------------------------------------------------ cases
def _random_case(n_pts, n_vox, k, seed, density=0.5, index='random', grid=False, cap=1024, pad=True):
    rng = np.random.default_rng([seed, n_pts, n_vox, k])
    vm = rng.random((k, n_vox)) < density
    if index == 'random':                                                   # repeats, and voxels that no point names
        idx = rng.integers(0, n_vox, n_pts).astype(np.int64)
    elif index == 'shuffled':                                               # every voxel at most once, in no order
        idx = rng.permutation(max(n_vox, n_pts))[:n_pts].astype(np.int64)
    else:
        idx = None
    if grid:                                                                # many equal extremes: the smallest point index wins
        pos = np.concatenate([rng.integers(0, 8, (n_pts, 2)).astype(np.float64), rng.random((n_pts, 1))], 1)
    else:
        pos = rng.normal(0, 1, (n_pts, 3))
    return {'vmasks': vm, 'index': idx, 'pos': pos, 'cap': cap, 'pad': pad}


def _through_index(case, seed, extra=0):
    """A case of _detbox_rule (masks over n points) as voxel masks: point p sits on voxel perm[p], plus `extra` unnamed voxels."""
    rng = np.random.default_rng(seed)
    masks, pos = np.asarray(case['masks'], bool), np.asarray(case['pos'], np.float64)
    n = masks.shape[1]
    perm = rng.permutation(n + extra)[:n].astype(np.int64)                  # voxel of point p
    vm = np.zeros((len(masks), n + extra), bool)
    vm[:, perm] = masks
    return {'vmasks': vm, 'index': perm, 'pos': pos, 'cap': case['cap'], 'pad': True}


@pytest.mark.parametrize('n_pts', [0, 1, 2, 3, 63, 64, 65, 4097])
def test_point_counts_and_voxel_counts(n_pts):
    """n_vox = 1, 64, 65 (one word, a full word, one bit of a second) with set pad bits above n_vox, and 300 / 5003 voxels: more
    and fewer voxels than points."""
    some = 0
    for n_vox in (1, 64, 65, 300, 5003):
        got, want = _check(_random_case(n_pts, n_vox, 3, seed=1, cap=4096))
        some += int(want['count'].sum())
    assert some > 0 or n_pts == 0


@pytest.mark.parametrize('n_pts', [65535, 65536, 65537, 131073])
def test_chunk_edges(n_pts):
    """One chunk of the passes is 1024 point words: 65 536 points.  Sparse rows over 5 003 voxels; the last point is in row 1."""
    case = _random_case(n_pts, 5003, 2, seed=2, density=0.01, cap=256)
    case['vmasks'][1, case['index'][-1]] = True
    case['vmasks'][0, case['index'][65535 % n_pts]] = True
    got, want = _check(case)
    assert want['count'].min() > 100 and expand(case)[1, -1] and (want['flags'] == 0).all()
    # grid-aligned points: the extremes tie within and across the chunks and the smallest POINT index wins (ncand tells)
    case = _random_case(n_pts, 5003, 2, seed=3, density=0.01, grid=True, cap=2048)
    got, want = _check(case)
    assert (want['ncand'] > 64).all() and (want['n_hull'] >= 4).all()


def test_ties_need_the_smallest_point_index():
    """Two points tie along +x and two along -x; which one becomes the extreme decides whether a probe just inside the hull is
    strictly inside the polygon of the extremes, i.e. the candidate count.  The pairs sit in different lanes, waves and chunks of
    the POINT order (the voxels they name are in no such order), and the rule with the last of equals counts otherwise."""
    case = _random_case(131073, 5003, 2, seed=3, density=0.01, cap=256)
    case['pos'][:, :2] *= 0.2                                               # the cloud: well inside
    special = {3: (10.0, 1.0), 65536 + 70: (10.0, -1.0), 65536 + 200: (-10.0, -1.0), 131072: (-10.0, 1.0), 5: (9.9, 3.0), 6: (9.9, -3.0),
               7: (-9.9, 3.0), 8: (-9.9, -3.0), 9: (9.96, -1.0), 12: (-9.96, 1.0)}
    for j, (p, xy) in enumerate(special.items()):
        case['pos'][p, :2] = xy
        case['index'][p] = 5002 - j                                         # descending voxels for ascending points
        case['vmasks'][:, 5002 - j] = True
    m = expand(case)
    first = [D.filter_rule(case['pos'][row][:, :2]) for row in m]
    last = [D.filter_rule(case['pos'][row][::-1, :2]) for row in m]
    assert all(a != b for a, b in zip(first, last))
    got, want = _check(case)
    assert np.array_equal(got['ncand'], first)


@pytest.mark.parametrize('k', [0, 1, 65])
def test_row_counts(k):
    got, want = _check(_random_case(700, 257, k, seed=4, density=0.2))
    assert len(got['count']) == k


def test_index_forms():
    # shuffled, non-monotone, every voxel at most once
    _check(_random_case(4097, 5003, 3, seed=5, index='shuffled'))
    _check(_random_case(5003, 300, 3, seed=5, index='shuffled'))            # (values up to 5002: most points name no voxel)
    # NULL = identity: more points than voxels (the tail is in no mask) and fewer
    _check(_random_case(700, 257, 3, seed=6, index=None))
    _check(_random_case(257, 700, 3, seed=6, index=None))
    # values outside [0, n_vox) beside set pad bits: -1, n_vox (a set pad bit of the last word), far above, 2^40
    case = _random_case(1000, 65, 4, seed=7)
    case['vmasks'][0] = True
    for p, v in ((0, -1), (1, 65), (2, 127), (3, 128), (4, 1 << 40), (999, -(1 << 40)), (998, 66)):
        case['index'][p] = v
    got, want = _check(case)
    assert want['count'][0] == 1000 - 7


def test_small_rows_through_an_index():
    """Empty, one point, two points, duplicated coordinates, collinear rows, repeated vertices, points on edges."""
    for n_mod in (1, 63):
        base = D._rows_to_case(list(D.SMALL_ROWS.values()), n_mod)
        got, want = _check(_through_index(base, seed=n_mod, extra=40))
        assert want['n_hull'].tolist()[:4] == [0, 1, 2, 1]
    # several points on one voxel: duplicated rows of the mask, each point with coordinates of its own
    case = _random_case(300, 7, 7, seed=8, density=0.4)
    case['vmasks'][3] = False
    _check(case)


def test_vertex_flag_and_candidate_flag():
    i = np.arange(600.0)
    rng = np.random.default_rng(9)
    gon = D._single(np.stack([i, i * i], 1)[rng.permutation(600)], 1024)     # a 600-gon: beyond B2M_HULL_MAX
    got, want = _check(_through_index(gon, seed=10, extra=100))
    assert want['flags'].tolist() == [D.FLAG_VERTICES] and want['n_hull'].tolist() == [600]
    sides = D._single(D._square_sides(61, 500, 4), 64)                       # 65 candidates
    case = _through_index(sides, seed=11, extra=100)
    got, want = _check(case)
    assert want['flags'].tolist() == [D.FLAG_CANDIDATES] and want['ncand'].tolist() == [65] and want['n_hull'].tolist() == [0]
    case['cap'] = 128
    got, want = _check(case)
    assert want['flags'].tolist() == [0] and want['n_hull'][0] >= 4


def test_batch_equals_the_single_form_and_two_runs_agree():
    """Three scenes in one table -- rows and no points, no rows, rows over two chunks -- then five, among them a scene with more
    chunks than the largest one would suggest is not needed: every scene reads its own sizes."""
    cases = [_random_case(0, 300, 5, seed=12, cap=256), _random_case(500, 300, 0, seed=13, cap=256),
             _random_case(70001, 5003, 65, seed=14, density=0.01, cap=256)]
    single = [_single(c) for c in cases]
    runs = [_batch(cases), _batch(cases)]
    for got in runs:
        for s, (g, w) in enumerate(zip(got, single)):
            for key in KEYS:
                assert g[key].tobytes() == w[key].tobytes(), (s, key)
    _against_rule(runs[0][2], cases[2])
    assert single[0]['n_hull'].tolist() == [0] * 5 and np.isinf(single[0]['box6']).all() and single[1]['count'].shape == (0,)
    again = _single(cases[2])
    assert all(again[key].tobytes() == single[2][key].tobytes() for key in KEYS)
    more = [_random_case(n, 257, k, seed=15, density=0.3, cap=256) for n, k in ((64, 17), (65, 1), (4097, 16), (1, 33), (300, 2))]
    for g, c in zip(_batch(more), more):
        _against_rule(g, c)
