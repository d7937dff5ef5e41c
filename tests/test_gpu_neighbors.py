"""The device nearest-neighbour index (box2mask_amd/neighbors.py, csrc/neighbors.hip) against numpy brute force in the contract's
summation order (tests/_neighbors_cases.py; tests/test_neighbors.py shows on the CPU that the yardstick is unambiguous and that
both host trees agree with it).  Indices and distances are compared exactly."""
import numpy as np
import pytest
import torch

from box2mask_amd import _lib
from box2mask_amd.neighbors import NearestIndex, nearest

import _neighbors_cases as NC

pytestmark = pytest.mark.gpu


def _check(ref, q, got_dist, got_idx, want=None):
    idx, d2, _ = want if want is not None else NC.brute(ref, q)
    assert got_idx.dtype == torch.int64 and got_idx.is_cuda and tuple(got_idx.shape) == (len(q),)
    assert got_dist.dtype == torch.float64 and tuple(got_dist.shape) == (len(q),)
    gi, gd = got_idx.cpu().numpy(), got_dist.cpu().numpy()
    bad = np.nonzero(gi != idx)[0]
    assert len(bad) == 0, 'first wrong queries %s: got %s want %s' % (bad[:5], gi[bad[:5]], idx[bad[:5]])
    assert np.array_equal(gd, np.sqrt(d2), equal_nan=True)


@pytest.mark.parametrize('name', sorted(NC.SMALL))
def test_index_equals_brute_force(name):
    ref, q, ties = NC.case(name)
    want = NC.brute(ref, q)
    index = NearestIndex(ref)
    dist, idx = index.query(q, return_distance=True)
    _check(ref, q, dist, idx, want)
    assert torch.equal(index.query(q), idx)                                  # without distances: the same rows
    if name == 'd':                                                          # identical rows: the lowest of them
        assert want[0][60] == 0 and int(idx[60]) == 0 and float(dist[60]) == 0.0
    if name == 'e':                                                          # eight rows at the same distance from every query
        d2 = NC.d2_rows(ref, q)
        assert ((d2 == d2.min(1, keepdims=True)).sum(1) == 8).all()
    if name == 'h':
        assert int(idx[41]) == -1 and np.isnan(float(dist[41])) and not (idx == 17).any()
        assert int((idx < 0).sum()) == 1 and int(torch.isnan(dist).sum()) == 1


def test_empty_sides():
    ref, q, _ = NC.case('b')
    dist, idx = nearest(ref, np.zeros((0, 3)), return_distance=True)         # n_q == 0
    assert tuple(idx.shape) == (0,) and idx.dtype == torch.int64 and tuple(dist.shape) == (0,)
    dist, idx = nearest(np.zeros((0, 3)), q, return_distance=True)           # n_ref == 0
    assert bool((idx == -1).all()) and bool(torch.isnan(dist).all()) and tuple(idx.shape) == (len(q),)
    assert bool((nearest(np.zeros((0, 3)), q) == -1).all())
    dist, idx = nearest(np.full((5, 3), np.nan), q, return_distance=True)    # no finite row at all
    assert bool((idx == -1).all()) and bool(torch.isnan(dist).all())


def test_many_blocks_against_ckdtree():
    """70 001 x 70 001: every scan and sort spans many blocks.  tests/test_neighbors.py shows that no query of this case has a
    second candidate within a relative 1e-9, so the k-d tree's answer is the contract's."""
    from scipy.spatial import cKDTree
    ref, q, _ = NC.case('i')
    want_d, want_i = cKDTree(ref).query(q, k=1)
    dist, idx = nearest(torch.from_numpy(ref), torch.from_numpy(q).cuda(), return_distance=True)
    assert np.array_equal(idx.cpu().numpy(), want_i)
    d = q - ref[want_i]
    assert np.array_equal(dist.cpu().numpy(), np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))
    assert np.array_equal(dist.cpu().numpy(), want_d)


def test_one_build_many_queries_and_two_runs():
    ref, q, _ = NC.case('c')
    q1, q2 = q[:1500], q[1500:]
    index = NearestIndex(ref)
    a1 = index.query(q1, return_distance=True)
    a2 = index.query(q2, return_distance=True)
    b1 = NearestIndex(ref).query(q1, return_distance=True)
    b2 = NearestIndex(ref).query(q2, return_distance=True)
    for a, b in ((a1, b1), (a2, b2)):
        assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int64), b[0].view(torch.int64))
    again = index.query(q1, return_distance=True)
    assert torch.equal(again[1], a1[1]) and torch.equal(again[0].view(torch.int64), a1[0].view(torch.int64))


def test_c_entries_write_only_their_outputs_and_take_no_distances():
    ref, q, _ = NC.case('b')
    want_i, want_d2, _ = NC.brute(ref, q)
    lib = _lib.load()
    n, m, pad = len(ref), len(q), 64
    size = lib.b2m_nn_workspace(n)
    assert size > 0 and lib.b2m_nn_workspace(-1) < 0 and lib.b2m_nn_workspace(1 << 40) < 0
    r = torch.from_numpy(ref).cuda()
    qq = torch.from_numpy(q).cuda()
    work = torch.empty((size + 7) // 8, dtype=torch.int64, device='cuda')
    _lib.call('b2m_nn_build', r.data_ptr(), n, work.data_ptr())
    idx = torch.full((m + 2 * pad,), 0x5a5a5a5a, dtype=torch.int32, device='cuda')
    dist = torch.full((m + 2 * pad,), -777.25, dtype=torch.float64, device='cuda')
    _lib.call('b2m_nn_query', r.data_ptr(), n, work.data_ptr(), qq.data_ptr(), m, idx[pad:].data_ptr(), dist[pad:].data_ptr())
    assert np.array_equal(idx[pad:pad + m].cpu().numpy(), want_i) and np.array_equal(dist[pad:pad + m].cpu().numpy(), np.sqrt(want_d2))
    for t, poison in ((idx, 0x5a5a5a5a), (dist, -777.25)):
        assert bool((t[:pad] == poison).all()) and bool((t[pad + m:] == poison).all())
    idx2 = torch.full((m + 2 * pad,), 0x5a5a5a5a, dtype=torch.int32, device='cuda')
    _lib.call('b2m_nn_query', r.data_ptr(), n, work.data_ptr(), qq.data_ptr(), m, idx2[pad:].data_ptr(), None)      # dist = NULL
    assert torch.equal(idx2, idx)
    with pytest.raises(_lib.B2MError):
        _lib.call('b2m_nn_query', r.data_ptr(), n, work.data_ptr(), qq.data_ptr(), m, None, None)
    with pytest.raises(_lib.B2MError):
        _lib.call('b2m_nn_build', None, n, work.data_ptr())
