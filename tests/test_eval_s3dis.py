"""Host half of the S3DIS metric (box2mask_amd/eval_s3dis.py) against the fixture taken from the reference's own s3dis_util /
Evaluater.s3dis_eval (tools/gen_golden.py s3dis), the fixture's own conditions, and the C ABI of the new entries.  No GPU."""
import ctypes as C
import re
import os

import numpy as np
import pytest

from box2mask_amd import _lib, eval_s3dis as S

import _s3dis_rule as R

ENTRIES = ['b2m_dbscan', 'b2m_paint_proposals', 'b2m_joint_hist']


@pytest.fixture(scope='module')
def gold():
    return np.load(R.GOLD)


def _same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize('case', [0, 1])
def test_dbscan_cases_meet_their_conditions_and_the_rule_reproduces_sklearn(gold, case):
    z = gold
    x = z['db%d_x' % case].astype(np.float64)
    eps, ms = float(z['db%d_eps' % case]), int(z['db%d_min_samples' % case])
    lab = z['db%d_labels' % case].astype(np.int32)
    core = np.unpackbits(z['db%d_core' % case], count=len(x)).astype(bool)
    assert x.shape == (6000, 6)
    assert R.margin(x, eps) >= 1e-12
    rule, rcore, two = R.dbscan_rule(x, eps, ms)
    assert np.array_equal(rule, lab) and np.array_equal(rcore, core)       # the rule of include/b2m.h IS sklearn's labelling
    assert lab.max() + 1 >= 50 and ((lab >= 0) & ~core).sum() >= 500 and (lab < 0).sum() >= 1000 and two.sum() >= 20
    perm = z['db%d_perm' % case].astype(np.int64)
    assert np.array_equal(np.sort(perm), np.arange(len(x)))
    lab_p = z['db%d_labels_perm' % case].astype(np.int32)
    assert not np.array_equal(lab_p, lab[perm])                             # the numbering follows the row order ...
    assert np.array_equal(lab_p >= 0, lab[perm] >= 0)                       # ... noise does not


@pytest.mark.parametrize('room', [0, 1, 2])
def test_rooms_meet_their_conditions(gold, room):
    rm = R.room(gold, room)
    assert 25000 <= rm['n'] <= 35000
    f = R.wall_features(rm)
    assert R.margin(f, S.WALL_EPS) >= 1e-12
    bg = rm['background']
    assert set(np.unique(bg[rm['pred_semantics'] == 0])) == {1} and set(np.unique(bg[rm['pred_semantics'] == 1])) == {2}
    wall = bg[rm['pred_semantics'] == 2]
    ids, cnt = np.unique(wall, return_counts=True)
    assert list(ids[ids >= 3]) == [4, 5] and (cnt[ids >= 3] >= 3000).all()     # two walls kept (noise would be 3) ...
    assert (wall == -1).sum() > 2000                                          # ... a wall under 3000 points and the strays are gone
    ps = rm['proposal_semantics']
    final = rm['final']
    accepted = np.array([(final['instances'] == k + 1).any() for k in range(len(ps))])
    assert accepted.sum() >= 8 and (ps[~accepted] < 3).any() and (ps[~accepted] >= 3).sum() >= 2
    assert (final['semantics'] != rm['pred_semantics']).any()                # the merge rewrote semantics
    repainted = (bg == 2) & (final['semantics'] != 1)
    assert 100 <= repainted.sum() < 200 and (final['instances'][repainted] == -1).all()
    want = set(range(13)) if room < 2 else set(range(12))
    assert set(np.unique(rm['gt']['semantics'])) == want and set(np.unique(final['semantics'])) == want


def test_metric_from_counts_reproduces_the_reference_bit_for_bit(gold):
    z = gold
    rooms = [R.room(z, r) for r in range(3)]
    counts = [R.counts_numpy(rm['final'], rm['gt']) for rm in rooms]
    for tag, sel in (('rooms01', counts[:2]), ('room2', counts[2:])):
        mprec, mrec, prec, rec = S.s3dis_eval_from_counts(sel)
        assert np.array_equal(prec, z[tag + '_precision'], equal_nan=True) and np.array_equal(rec, z[tag + '_recall'], equal_nan=True)
        assert np.array_equal(np.float64(mprec), z[tag + '_mprec'], equal_nan=True)
        assert np.array_equal(np.float64(mrec), z[tag + '_mrec'], equal_nan=True)
    assert np.isfinite(z['rooms01_precision']).all() and np.isfinite(z['rooms01_recall']).all()
    assert np.isnan(z['room2_precision'][12]) and np.isnan(z['room2_recall'][12]) and np.isnan(z['room2_mprec'])
    assert np.isfinite(z['room2_precision'][:12]).all()
    # the details against the restatement from boolean masks
    extra = S.s3dis_eval_from_counts(counts[:2], details=True)[4]
    ref = R.details_numpy([rm['final'] for rm in rooms[:2]], [rm['gt'] for rm in rooms[:2]])
    for k in ('oAcc', 'iou', 'mIoU', 'MUCov', 'MWCov'):
        assert np.allclose(extra[k], ref[k], rtol=0, atol=1e-12), k


def test_exports_are_declared_bound_and_exported():
    hdr = open(os.path.join(R.ROOT, 'include', 'b2m.h')).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r'\bint\s+%s\s*\(' % name, hdr), name
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert 'b2m_dbscan_workspace' in _lib.PLAIN and hasattr(lib, 'b2m_dbscan_workspace')
    m = re.search(r'#define\s+B2M_JOINT_HIST_MAX\s+\(\s*1\s*<<\s*(\d+)\s*\)', hdr)
    assert m and 1 << int(m.group(1)) == S.JOINT_HIST_MAX
    from box2mask_amd import build
    assert 'cluster.hip' in build.SOURCES


def test_entries_check_their_arguments_on_the_host():
    lib = _lib.load()
    err = lambda: lib.b2m_last_error().decode()
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data_as(C.c_void_p)          # never dereferenced: every call below is refused before a launch
    ARG = -1
    db = lambda x=p, n=8, d=6, eps=0.35, ms=10, work=p, labels=p, count=p: lib.b2m_dbscan(x, n, d, eps, ms, work, labels, count, None)
    assert db(d=2) == ARG and '3 ... 8' in err()
    assert db(d=9) == ARG and '3 ... 8' in err()
    assert db(ms=0) == ARG and 'min_samples' in err()
    assert db(eps=0.0) == ARG and 'eps' in err()
    assert db(eps=-1.0) == ARG and db(eps=float('nan')) == ARG
    assert db(labels=None) == ARG and 'NULL' in err()
    assert db(count=None) == ARG and db(x=None) == ARG and db(work=None) == ARG
    assert db(n=-1) == ARG and db(n=1 << 31) == ARG
    assert db(n=0, x=None, work=None, labels=None) == 0                 # nothing to do: no launch, no device needed
    assert lib.b2m_dbscan_workspace(0) >= 0 and lib.b2m_dbscan_workspace(1 << 31) < 0
    assert lib.b2m_dbscan_workspace(1000) < lib.b2m_dbscan_workspace(2000)
    jh = lambda a=p, b=p, n=8, na=13, nb=13, hist=p: lib.b2m_joint_hist(a, b, n, na, nb, hist, None)
    assert jh(na=1 << 13, nb=(1 << 11) + 1) == ARG and 'B2M_JOINT_HIST_MAX' in err()
    assert jh(hist=None) == ARG and 'NULL' in err()
    assert jh(a=None) == ARG and jh(na=0) == ARG and jh(nb=0) == ARG and jh(n=-1) == ARG
    pp = lambda bits=p, words=1, k=1, sem=p, n=64, unl=p, inst=p, acc=p: lib.b2m_paint_proposals(
        bits, words, k, sem, n, 3, 0.6, 200, unl, inst, p, acc, None)
    assert pp(words=2) == ARG and 'words' in err()
    assert pp(inst=None) == ARG and 'NULL' in err()
    assert pp(unl=None) == ARG and pp(bits=None) == ARG and pp(acc=None) == ARG and pp(k=-1) == ARG
    assert pp(n=0, words=0, inst=None, unl=None) == 0


def test_product_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    with pytest.raises(_lib.B2MError):
        S.dbscan(np.zeros((4, 6)), 0.35, 10)
    with pytest.raises(_lib.B2MError):
        S.s3dis_counts({'instances': np.zeros(4), 'semantics': np.zeros(4)}, {'instances': np.zeros(4), 'semantics': np.zeros(4)})
