"""Host half of the ARKitScenes detection metric (box2mask_amd/eval_detection.py) against the fixture taken from the reference's
own eval_det (tools/gen_golden.py detection), and the C ABI of the new entries.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from box2mask_amd import _lib, eval_detection as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'eval_detection.npz')
ENTRIES = ['b2m_mask_hulls', 'b2m_obb_corners', 'b2m_hull_box_iou', 'b2m_aabb_iou']


def _records(z, tag):
    """The records eval_det takes, from the fixture's reference IoUs."""
    recs = {}
    for s in range(int(z['n_scenes'])):
        keep = z['s%d_count' % s] >= 50
        recs['room%d' % s] = {'label': z['s%d_label_id' % s][keep], 'conf': z['s%d_conf' % s][keep],
                              'gt_label': z['s%d_per_instance_semantics' % s], 'iou': z['s%d_iou_%s' % (s, tag)][keep]}
    return recs


def _same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize('tag', ['obb', 'aabb'])
@pytest.mark.parametrize('th', [0.5, 0.25])
def test_matching_and_ap_reproduce_the_reference_bit_for_bit(tag, th):
    z = np.load(GOLD)
    rec, prec, ap = D.eval_det(_records(z, tag), ovthresh=th)
    key = '%s_%d' % (tag, round(th * 100))
    classes = [int(c) for c in z[key + '_classes']]
    assert list(ap.keys()) == classes                                 # the same classes in the same order
    assert _same_bits([ap[c] for c in classes], z[key + '_ap'])
    for c in classes:
        assert _same_bits(rec[c], z['%s_rec_%d' % (key, c)]), c
        assert _same_bits(prec[c], z['%s_prec_%d' % (key, c)]), c
    assert _same_bits(D.mean_ap(ap), z[key + '_map'])
    assert any(np.isnan(v) for v in ap.values())                      # the class that has predictions and no ground truth
    assert 24 not in ap                                               # ground truth and no prediction: skipped, as in the reference


def test_fixture_covers_the_cases():
    z = np.load(GOLD)
    for s in range(int(z['n_scenes'])):
        count = z['s%d_count' % s]
        assert (count < 50).any() and (count >= 50).sum() >= 8
        iou = z['s%d_iou_obb' % s][count >= 50]
        assert ((iou > 0.25).sum(0) >= 2).any()                                       # two predictions on one ground truth
        assert (iou > 0).any(1).sum() < len(iou)                                      # a prediction without a same-class overlap
        for t in (0.5, 0.25):
            assert np.abs(iou - t).min() > 1e-6
        assert int(z['s%d_hull_max' % s]) <= 40


def test_voc_ap():
    rec = np.array([0.25, 0.25, 0.5, 0.5, 0.75])
    prec = np.array([1.0, 0.5, 2 / 3, 0.5, 0.6])
    assert D.voc_ap(rec, prec) == 0.25 * 1.0 + 0.25 * (2 / 3) + 0.25 * 0.6
    ap07 = D.voc_ap(rec, prec, use_07_metric=True)
    assert abs(ap07 - (3 * 1.0 + 3 * (2 / 3) + 2 * 0.6) / 11) < 1e-15


def test_matching_rules():
    # one class, one scene, two ground truths: the better detection takes gt 0, the second detection of gt 0 is a false positive,
    # an IoU equal to the threshold is no match, the first maximum wins a tie
    recs = {'a': {'label': np.array([5, 5, 5, 5]), 'conf': np.array([0.9, 0.8, 0.7, 0.6], np.float32), 'gt_label': np.array([5, 5]),
                  'iou': np.array([[0.8, 0.1], [0.7, 0.2], [0.0, 0.5], [0.6, 0.6]])}}
    rec, prec, ap = D.eval_det(recs, ovthresh=0.5)
    assert np.array_equal(rec[5], [0.5, 0.5, 0.5, 0.5])
    assert np.array_equal(prec[5], [1.0, 0.5, 1 / 3, 0.25])


def test_exports_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'b2m.h')).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r'\bint\s+%s\s*\(' % name, hdr), name
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert int(re.search(r'#define\s+B2M_HULL_MAX\s+(\d+)', hdr).group(1)) == D.HULL_MAX
    assert int(re.search(r'#define\s+B2M_HULL_PART\s+(\d+)', hdr).group(1)) == D.HULL_PART
    assert int(re.search(r'#define\s+B2M_HULL_CHUNKS\s+(\d+)', hdr).group(1)) == D.HULL_CHUNKS
    assert int(re.search(r'#define\s+B2M_OBB_REC\s+(\d+)', hdr).group(1)) == D.OBB_REC


def test_entries_check_their_arguments_on_the_host():
    lib = _lib.load()
    err = lambda: lib.b2m_last_error().decode()
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data_as(C.c_void_p)          # never dereferenced: every call below is refused before a launch
    ARG = -1
    hull = lambda bits=p, words=1, k=1, pos=p, n=64, cap=64, flags=p: lib.b2m_mask_hulls(
        bits, words, k, pos, n, p, p, p, cap, p, p, p, p, p, flags, None)
    assert hull(k=-1) == ARG
    assert hull(words=1, n=65) == ARG and 'words' in err()
    assert hull(bits=None) == ARG and 'NULL' in err()
    assert hull(flags=None) == ARG
    assert hull(pos=None) == ARG
    assert hull(cap=100) == ARG and 'power of two' in err()
    assert hull(k=0, bits=None) == 0                                   # nothing to do: no launch, no device needed
    assert lib.b2m_obb_corners(None, p, p, 1, p, None) == ARG
    assert lib.b2m_obb_corners(p, p, p, -1, p, None) == ARG
    assert lib.b2m_obb_corners(None, None, None, 0, None, None) == 0
    assert lib.b2m_hull_box_iou(p, p, p, p, 1, p, p, 1, None, None) == ARG and 'NULL' in err()
    assert lib.b2m_hull_box_iou(p, p, p, p, -1, p, p, 1, p, None) == ARG
    assert lib.b2m_hull_box_iou(None, None, None, None, 0, None, None, 3, None, None) == 0
    assert lib.b2m_aabb_iou(p, None, 1, p, p, p, 1, p, None) == ARG
    assert lib.b2m_aabb_iou(p, p, 1, p, p, p, -2, p, None) == ARG
