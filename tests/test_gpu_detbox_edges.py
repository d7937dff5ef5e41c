"""csrc/detbox.hip at its edges against the rules of tests/_detbox_rule.py (profiles/eval_rule.md): b2m_mask_hulls, b2m_obb_corners,
b2m_aabb_iou and b2m_hull_box_iou through the C entries and the wrappers of box2mask_amd/eval_detection.py.  Integer outputs, hull
vertices, box records and the axis-aligned IoU are compared bit for bit; the hull x box IoU bit for bit with float(Fraction) where
fp64 evaluates every step exactly, and within the derived forward bound of form (b) (itself at most 1e-9) everywhere else.  Every
output buffer starts as a sentinel and carries 64 sentinel elements behind it, which must survive.  The reach predicates of the
cases and the proof that they are sharp are CPU tests (tests/test_eval_rules.py).  No case provokes a fault.

Measured on an MI355X: hull x box IoU, 65 of the 143 direct cases bit for bit, largest |device - exact| / bound 0.0971 on the others,
0.000545 through the whole chain (profiles/eval_rule.md)."""
import numpy as np
import pytest
import torch

from box2mask_amd import _lib, eval_detection as E
from box2mask_amd._lib import ptr

import _cluster_rule as C
import _detbox_rule as D

pytestmark = pytest.mark.gpu
PAD = 64
S32, SF = -77, -7.25


def _buf(n, dtype, sentinel):
    return torch.full((n + PAD,), sentinel, dtype=dtype, device='cuda')


def _take(t, n, sentinel):
    host = t.cpu().numpy()
    assert (host[n:] == sentinel).all(), 'written past the end'
    return host[:n]


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ------------------------------------------------------------------ b2m_mask_hulls
def _hulls(case):
    masks, pos, cap = case['masks'], case['pos'], case['cap']
    k, n = masks.shape
    words = (n + 63) // 64
    bits = torch.from_numpy(C.pack_rows(masks, pad=case['pad']).view(np.int64)).cuda() if k else None
    posd = torch.from_numpy(np.ascontiguousarray(pos, np.float64)).cuda()
    out = {'count': _buf(k, torch.int32, S32), 'box6': _buf(k * 6, torch.float64, SF), 'hull': _buf(k * D.HULL_MAX * 2, torch.float64, SF),
           'n_hull': _buf(k, torch.int32, S32), 'flags': _buf(k, torch.int32, S32), 'ncand': _buf(k, torch.int32, S32)}
    work = torch.empty(max(k, 1) * D.HULL_CHUNKS * 56, dtype=torch.float64, device='cuda')
    cand = torch.empty(max(k, 1) * cap * 2, dtype=torch.float64, device='cuda')
    stk = torch.empty(max(k, 1) * cap, dtype=torch.int32, device='cuda')
    _lib.call('b2m_mask_hulls', ptr(bits), words, k, ptr(posd), n, ptr(work), ptr(cand), ptr(stk), cap, ptr(out['ncand']),
              ptr(out['count']), ptr(out['box6']), ptr(out['hull']), ptr(out['n_hull']), ptr(out['flags']))
    return {'count': _take(out['count'], k, S32), 'box6': _take(out['box6'], k * 6, SF).reshape(k, 6),
            'hull': _take(out['hull'], k * D.HULL_MAX * 2, SF).reshape(k, D.HULL_MAX, 2), 'n_hull': _take(out['n_hull'], k, S32),
            'flags': _take(out['flags'], k, S32), 'ncand': _take(out['ncand'], k, S32)}


def _hulls_check(case):
    want = D.hulls_rule(case['masks'], case['pos'], case['cap'])
    got = _hulls(case)
    for key in ('count', 'ncand', 'n_hull', 'flags'):
        assert np.array_equal(got[key], want[key]), key
    assert _bits(got['box6'], want['box6'])
    for r, h in enumerate(want['hulls']):
        m = 0 if h is None else len(h)
        if m:
            assert np.array_equal(got['hull'][r, :m], h), r                 # the fp64 chain over ALL the row's points
        assert (got['hull'][r, m:] == SF).all(), r                          # nothing behind it; nothing at all for a flagged row
    return got, want


@pytest.mark.parametrize('name', sorted(D.hull_cases()))
def test_mask_hulls_equal_the_rule(name):
    _hulls_check(D.hull_cases()[name])


def test_mask_hulls_two_million_points_in_31_chunks():
    case = D.big_hull_case()                                                # the largest input: wpb = 1088
    got, want = _hulls_check(case)
    assert want['count'][0] > 90000 and want['n_hull'][0] >= 10


def test_mask_hulls_wrapper_and_two_runs():
    case = D.hull_cases()['words:1025']
    want = D.hulls_rule(case['masks'], case['pos'], case['cap'])
    runs = []
    for _ in range(2):
        bits, words, n = E.pack_masks(case['masks'])
        raw = E.hulls_from_bits(bits, words, n, case['pos'], cap=case['cap'])
        runs.append(b''.join(raw[k].cpu().numpy().tobytes() for k in ('count', 'box6', 'hull', 'n_hull', 'flags', 'ncand')))
        for r, h in enumerate(want['hulls']):
            assert np.array_equal(raw['hull'][r, :len(h)].cpu().numpy(), h)
    assert runs[0] == runs[1]


# ------------------------------------------------------------------ b2m_obb_corners, b2m_aabb_iou
@pytest.mark.parametrize('g', [0, 1, 63, 64, 65])
def test_obb_corners_bit_for_bit(g):
    c, b, q = D.corners_case(max(g, 1))
    cd, bd, qd = (torch.from_numpy(np.ascontiguousarray(a[:g])).cuda() for a in (c, b, q))
    out = _buf(g * D.OBB_REC, torch.float64, SF)
    _lib.call('b2m_obb_corners', ptr(cd), ptr(bd), ptr(qd), g, ptr(out))
    assert _bits(_take(out, g * D.OBB_REC, SF).reshape(g, D.OBB_REC), D.corners_rule(c[:g], b[:g], q[:g]))
    if g:
        rec = E.gt_boxes({'per_instance_bb_centers': c[:g], 'per_instance_bb_bounds': b[:g], 'per_instance_bb_rotations': q[:g],
                          'per_instance_semantics': np.zeros(g)})['boxes'].cpu().numpy()
        assert _bits(rec, D.corners_rule(c[:g], b[:g], q[:g]))


def _aabb(box6, pcls, gc, boxes, gcls):
    k, g = len(box6), len(gc)
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (box6, pcls, gc, boxes, gcls)]
    out = _buf(k * g, torch.float64, SF)
    _lib.call('b2m_aabb_iou', ptr(t[0]), ptr(t[1]), k, ptr(t[2]), ptr(t[3]), ptr(t[4]), g, ptr(out))
    return _take(out, k * g, SF).reshape(k, g)


@pytest.mark.parametrize('kg', [(1, 1), (5, 51), (16, 16), (257, 1)])
def test_aabb_iou_sizes_bit_for_bit(kg):
    case = D.aabb_size_case(*kg)
    want = D.aabb_rule(*case)
    assert _bits(_aabb(*case), want) and ((want > 0).any() or kg == (1, 1))


def test_aabb_iou_edges_bit_for_bit():
    case = D.aabb_edge_case()
    want = D.aabb_rule(*case)
    got = _aabb(*case)
    assert _bits(got, want)
    assert got[0, 0] == 0 and got[0, 1] == 1.0 and got[2, 1] == 0.125 and got[5, 6] == 0 and (got[4] == 0).all() and (got[:, 4] == 0).all()


# ------------------------------------------------------------------ b2m_hull_box_iou
def _hull_box(hull, n_hull, box6, pcls, boxes, gcls):
    k, g = len(n_hull), len(gcls)
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (hull, n_hull, box6, pcls, boxes, gcls)]
    out = _buf(k * g, torch.float64, SF)
    _lib.call('b2m_hull_box_iou', ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(t[3]), k, ptr(t[4]), ptr(t[5]), g, ptr(out))
    return _take(out, k * g, SF).reshape(k, g)


def _table(cases):
    """One call for all cases: a hull row per distinct (hull, z range), a box per case; the class ids pair each box with its row."""
    rows, keys = [], {}
    hull = np.full((0, D.HULL_MAX, 2), SF)
    box6, owner, boxes = [], [], []
    for name, _, h, zlo, zhi, rect, z0, z7, vol2 in cases:
        key = (h.tobytes(), zlo, zhi)
        if key not in keys:
            keys[key] = len(rows)
            rows.append(len(h))
            slot = np.full((1, D.HULL_MAX, 2), SF)
            slot[0, :len(h)] = h
            hull = np.concatenate([hull, slot])
            box6.append([0.0, 0.0, zlo, 0.0, 0.0, zhi])
        rec = np.zeros(D.OBB_REC)
        rec[:8] = np.asarray(rect).reshape(8); rec[8], rec[9], rec[10] = z0, z7, vol2
        boxes.append(rec)
        owner.append(keys[key])
    if len(rows) % 2 == 0:                                                   # k * g odd: the last workgroup has one wave without a pair
        rows.append(0); box6.append([0.0] * 6)
        hull = np.concatenate([hull, np.full((1, D.HULL_MAX, 2), SF)])
    if len(boxes) % 2 == 0:
        boxes.append(np.zeros(D.OBB_REC)); owner.append(-5)
    k = len(rows)
    return (hull, np.array(rows, np.int32), np.array(box6), np.arange(k, dtype=np.int32), np.array(boxes), np.array(owner, np.int32))


def test_hull_box_iou_against_the_exact_form():
    cases = D.iou_cases()
    forms = [D.iou_case_forms(c) for c in cases]
    assert all(D.case_is_valid(f) for f in forms)
    args = _table(cases)
    got = _hull_box(*args)
    k, g = got.shape
    assert (k * g) % 2 == 1
    owner = args[5]
    ratio, exact = 0.0, 0
    for b, (case, f) in enumerate(zip(cases, forms)):
        r = owner[b]
        dev = got[r, b]
        assert (dev == 0) == (f['iou_exact'] == 0), case[0]                 # the same zero entries
        if f['exact']:
            assert dev == float(f['iou_exact']), case[0]                    # bit for bit
            exact += 1
        else:
            err = abs(dev - float(f['iou_exact']))
            assert err <= f['bound'] <= D.IOU_TOL, (case[0], err, f['bound'])
            ratio = max(ratio, err / f['bound'] if f['bound'] else 0.0)
    other = np.ones_like(got, bool)
    other[owner[:len(cases)], np.arange(len(cases))] = False
    assert (got[other] == 0).all()                                          # class mismatch everywhere else
    print('hull x box IoU: %d cases, %d bit for bit; largest |device - exact| / bound %.3g' % (len(cases), exact, ratio))


def test_hull_box_iou_single_pair():
    case = [c for c in D.iou_cases() if c[0] == 'sq:cut']
    got = _hull_box(*_table(case))
    assert got.shape == (1, 1) and got[0, 0] == 1.0 / 9.0


def test_whole_chain_through_the_wrappers():
    pos, masks, plabel, centers, bounds, rot, glabel = D.pipeline_case()
    want_h = D.hulls_rule(masks, pos, E.DEFAULT_CAP)
    rec = D.corners_rule(centers, bounds, rot)
    pred = E.mask_boxes({'conf': np.zeros(len(masks), np.float32), 'label_id': plabel, 'mask': masks}, pos, min_points=1)
    gt = E.gt_boxes({'per_instance_bb_centers': centers, 'per_instance_bb_bounds': bounds, 'per_instance_bb_rotations': rot,
                     'per_instance_semantics': glabel})
    assert np.array_equal(pred['n_hull'].cpu().numpy(), [3, 65, 129]) and _bits(gt['boxes'].cpu().numpy(), rec)
    for r, h in enumerate(want_h['hulls']):
        assert np.array_equal(pred['hull'][r, :len(h)].cpu().numpy(), h)
    iou = E.scene_ious(pred, gt, oriented=True)
    ratio = 0.0
    for r in range(len(masks)):
        for b in range(len(centers)):
            f = D.iou_forms(want_h['hulls'][r], want_h['box6'][r, 2], want_h['box6'][r, 5], rec[b, :8].reshape(4, 2), rec[b, 8], rec[b, 9],
                            rec[b, 10])
            assert D.case_is_valid(f)
            err = abs(iou[r, b] - float(f['iou_exact']))
            assert (iou[r, b] == 0) == (f['iou_exact'] == 0) and err <= f['bound'] <= D.IOU_TOL
            ratio = max(ratio, err / f['bound'] if f['bound'] else 0.0)
    assert (iou > 0).sum() >= 6
    aabb = E.scene_ious(pred, gt, oriented=False)
    assert _bits(aabb, D.aabb_rule(want_h['box6'], plabel, centers, rec, glabel))
    print('chain: largest |device - exact| / bound %.3g' % ratio)
