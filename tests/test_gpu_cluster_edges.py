"""csrc/cluster.hip at its edges against the rules of tests/_cluster_rule.py (profiles/eval_rule.md): b2m_dbscan, b2m_paint_proposals
and b2m_joint_hist through the C entries and, where one exists, the wrappers of box2mask_amd/eval_s3dis.py.  Every comparison is
np.array_equal.  Every output buffer starts as a sentinel and carries 64 sentinel elements behind it, which must survive.  The reach
predicates of the cases and the proof that they are sharp are CPU tests (tests/test_eval_rules.py).  No case provokes a fault: every
refusal below is refused on the host, before a launch."""
import numpy as np
import pytest
import torch

from box2mask_amd import _lib, eval_s3dis as S
from box2mask_amd._lib import ptr

import _cluster_rule as C

pytestmark = pytest.mark.gpu
PAD = 64
S32, S64 = -77, 0x5a5a5a5a5a5a5a5a


def _buf(n, dtype, sentinel):
    return torch.full((n + PAD,), sentinel, dtype=dtype, device='cuda')


def _take(t, n, sentinel):
    """The first n elements on the host, after checking that the 64 elements behind them still hold the sentinel."""
    host = t.cpu().numpy()
    assert (host[n:] == sentinel).all(), 'written past the end'
    return host[:n]


# ------------------------------------------------------------------ b2m_dbscan
def _dbscan(x, eps, ms, d=None, n=None, count0=S32):
    x = np.ascontiguousarray(x, np.float64)
    n = len(x) if n is None else n
    d = x.shape[1] if d is None else d
    xd = torch.from_numpy(x).cuda()
    labels, count = _buf(max(n, 0), torch.int32, S32), _buf(1, torch.int32, count0)
    size = _lib.load().b2m_dbscan_workspace(max(n, 0))
    work = torch.empty(size // 8 + 1, dtype=torch.int64, device='cuda')
    _lib.call('b2m_dbscan', ptr(xd), n, d, float(eps), int(ms), ptr(work), ptr(labels), ptr(count))
    return _take(labels, n, S32), int(_take(count, 1, count0)[0])


@pytest.fixture(scope='module')
def db_rules():
    """name -> (x, eps, min_samples, labels of the tree twin): computed once.  The twin equals the brute-force rule on every one of
    these cases (tests/test_eval_rules.py)."""
    cases = {**C.size_cases(), **C.edge_cases()}
    return {name: (x, eps, ms, C.dbscan_tree(x, eps, ms)[0]) for name, (x, eps, ms) in cases.items()}


DB_NAMES = sorted({**C.size_cases(), **C.edge_cases()})


@pytest.mark.parametrize('name', DB_NAMES)
def test_dbscan_equals_the_rule(db_rules, name):
    x, eps, ms, want = db_rules[name]
    lab, count = _dbscan(x, eps, ms)
    assert np.array_equal(lab, want)
    assert count == want.max() + 1 if len(want) else count == 0             # zero core rows: n_clusters = 0 IS written
    got = S.dbscan(x, eps, ms).cpu().numpy()                                # the wrapper
    assert np.array_equal(got, want)


def test_dbscan_two_runs_give_identical_bytes(db_rules):
    for name in ('n:2049', 'clamp', 'nonfinite:1'):
        x, eps, ms, _ = db_rules[name]
        a, b = _dbscan(x, eps, ms), _dbscan(x, eps, ms)
        assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]


def test_dbscan_lattice_of_262145_singletons():
    """The first n at which db_blockscan's per-thread loop takes two block sums.  Closed form: no rule run."""
    x, eps, ms = C.lattice_case()
    lab, count = _dbscan(x, eps, ms)
    assert count == len(x) and np.array_equal(lab, np.arange(len(x), dtype=np.int32))


def test_dbscan_of_no_rows_leaves_the_count_to_the_caller():
    lab, count = _dbscan(np.zeros((0, 5)), 0.3, 2, count0=1234)
    assert lab.shape == (0,) and count == 1234


@pytest.mark.parametrize('what', ['d=2', 'd=9', 'eps=0', 'eps=nan', 'eps=inf', 'min_samples=0'])
def test_dbscan_refusals_leave_every_output_untouched(what):
    """Each of these is refused by the argument checks of b2m_dbscan on the host: nothing is launched."""
    x = np.random.default_rng(0).random((100, 9))
    kw = {'d=2': dict(d=2), 'd=9': dict(d=9), 'eps=0': dict(eps=0.0), 'eps=nan': dict(eps=float('nan')),
          'eps=inf': dict(eps=float('inf')), 'min_samples=0': dict(ms=0)}[what]
    args = dict(eps=0.3, ms=3, d=5)
    args.update(kw)
    xd = torch.from_numpy(x).cuda()
    labels, count = _buf(100, torch.int32, S32), _buf(1, torch.int32, S32)
    work = torch.empty(_lib.load().b2m_dbscan_workspace(100) // 8 + 1, dtype=torch.int64, device='cuda')
    with pytest.raises(_lib.B2MError):
        _lib.call('b2m_dbscan', ptr(xd), 100, args['d'], args['eps'], args['ms'], ptr(work), ptr(labels), ptr(count))
    torch.cuda.synchronize()
    assert (labels.cpu().numpy() == S32).all() and (count.cpu().numpy() == S32).all()


def test_dbscan_workspace_refuses_sizes_out_of_range():
    lib = _lib.load()                                                       # (host arithmetic only)
    assert lib.b2m_dbscan_workspace(-1) == -1 and lib.b2m_dbscan_workspace(1 << 31) == -1
    assert lib.b2m_dbscan_workspace((1 << 31) - 1) > 0


# ------------------------------------------------------------------ b2m_paint_proposals
def _paint(case):
    masks, sem = case['masks'], case['sem']
    k, n = masks.shape
    words = (n + 63) // 64
    bits = torch.from_numpy(C.pack_rows(masks).view(np.int64)).cuda() if k else None
    semd = torch.from_numpy(sem).cuda() if k else None
    unl, inst, acc = _buf(words, torch.int64, S64), _buf(n, torch.int32, S32), _buf(k, torch.int32, S32)
    sem_out = None
    if case['sem_in'] is not None:
        sem_out = _buf(n, torch.int32, S32)
        sem_out[:n] = torch.from_numpy(case['sem_in']).cuda()
    _lib.call('b2m_paint_proposals', ptr(bits), words, k, ptr(semd), n, case['sem_min'], case['ratio'], case['min_points'], ptr(unl),
              ptr(inst), ptr(sem_out), ptr(acc))
    return (_take(acc, k, S32), _take(inst, n, S32), None if sem_out is None else _take(sem_out, n, S32),
            _take(unl, words, S64).view(np.uint64))


def _paint_check(case):
    accepted, inst, sem_out, unlabeled = C.paint_run_rule(case)
    got = _paint(case)
    assert np.array_equal(got[0], accepted)
    assert np.array_equal(got[1], inst)
    assert (sem_out is None and got[2] is None) or np.array_equal(got[2], sem_out)
    assert np.array_equal(got[3], C.pack_rows(unlabeled[None])[0])          # pad bits zero


@pytest.mark.parametrize('n', C.PAINT_SIZES)
def test_paint_sizes(n):
    _paint_check(C.paint_size_case(n))


@pytest.mark.parametrize('name', sorted(C.paint_edge_cases()))
def test_paint_edges(name):
    _paint_check(C.paint_edge_cases()[name])


def test_paint_wrapper_equals_the_rule():
    case = dict(C.paint_size_case(65537), sem_min=S.SEM_MIN, ratio=S.KEEP_RATIO, min_points=S.MIN_POINTS)
    accepted, inst, sem_out, _ = C.paint_run_rule(case)
    bits, words, n = S.pack_masks(case['masks'])
    got = S.paint_proposals(bits, words, n, torch.from_numpy(case['sem']).cuda(), torch.from_numpy(case['sem_in']).cuda())
    assert np.array_equal(got[0].cpu().numpy(), inst) and np.array_equal(got[1].cpu().numpy(), sem_out)
    assert np.array_equal(got[2].cpu().numpy(), accepted) and 0 < accepted.sum() < len(accepted)


# ------------------------------------------------------------------ b2m_joint_hist
def _hist(a, b, na, nb, poison=S32):
    ad = torch.from_numpy(a).cuda() if len(a) else None
    bd = torch.from_numpy(b).cuda() if b is not None and len(b) else None
    hist = _buf(na * nb, torch.int32, poison)
    _lib.call('b2m_joint_hist', ptr(ad), ptr(bd), len(a), na, nb, ptr(hist))
    return _take(hist, na * nb, poison).reshape(na, nb)


@pytest.mark.parametrize('name', sorted(C.joint_hist_cases()))
def test_joint_hist_equals_the_rule(name):
    a, b, na, nb = C.joint_hist_cases()[name]
    want = C.joint_hist_rule(a, b, na, nb)
    assert np.array_equal(_hist(a, b, na, nb), want)                        # (n0: a poisoned table comes back zeroed)
    if len(a):
        got = S.joint_hist(torch.from_numpy(a).cuda(), None if b is None else torch.from_numpy(b).cuda(), na, nb).cpu().numpy()
        assert np.array_equal(got, want)


def test_joint_hist_table_ceiling():
    a = np.array([0, C.JH_MAX - 1, 5, -1, C.JH_MAX], np.int32)
    got = _hist(a, None, C.JH_MAX, 1)                                       # 2^24 entries: accepted
    assert got[0, 0] == 1 and got[C.JH_MAX - 1, 0] == 1 and got[5, 0] == 1 and got.sum() == 3
    ad = torch.from_numpy(a).cuda()
    hist = _buf(C.JH_MAX + 1, torch.int32, S32)
    with pytest.raises(_lib.B2MError, match='B2M_JOINT_HIST_MAX'):          # 2^24 + 1: refused on the host, nothing launched or zeroed
        _lib.call('b2m_joint_hist', ptr(ad), None, len(a), C.JH_MAX + 1, 1, ptr(hist))
    torch.cuda.synchronize()
    assert (hist.cpu().numpy() == S32).all()


def test_joint_hist_grid_stride_second_pass():
    n = C.JH_GRID * 16 + 1                                                  # 2048 blocks x 256 threads x 16 rows, and one more
    rng = np.random.default_rng(6)
    a = rng.integers(-1, 701, n).astype(np.int32)
    b = rng.integers(-1, 10, n).astype(np.int32)
    ad, bd = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    for na, nb in ((13, 9), (700, 9)):                                      # the LDS table and the global one
        hist = _buf(na * nb, torch.int32, S32)
        _lib.call('b2m_joint_hist', ptr(ad), ptr(bd), n, na, nb, ptr(hist))
        ok = (a >= 0) & (a < na) & (b >= 0) & (b < nb)
        want = np.bincount(a[ok].astype(np.int64) * nb + b[ok], minlength=na * nb)
        assert np.array_equal(_take(hist, na * nb, S32), want)
