"""GPU: the nearest-neighbour index (csrc/neighbors.hip) on the edge cases of tests/_neighbors_cases.py, against the same yardstick as
tests/test_gpu_neighbors.py: numpy brute force in the contract's summation order, rows and distances compared exactly.
tests/test_neighbors.py shows on the CPU what each case reaches (the shell of every winner, the branches of the edge choice, the
clamped cells) and that every case that is not built to tie has no second candidate within a relative 1e-9."""
import numpy as np
import pytest
import torch

from box2mask_amd import _lib
from box2mask_amd.neighbors import NearestIndex

import _neighbors_cases as NC

pytestmark = pytest.mark.gpu


def _check(name, dist, idx):
    want_i, want_d2, _ = NC.edge_brute(name)
    gi, gd = idx.cpu().numpy(), dist.cpu().numpy()
    bad = np.nonzero(gi != want_i)[0]
    assert len(bad) == 0, '%s: first wrong queries %s: got %s want %s' % (name, bad[:5], gi[bad[:5]], want_i[bad[:5]])
    with np.errstate(all='ignore'):
        assert np.array_equal(gd, np.sqrt(want_d2), equal_nan=True), name


@pytest.mark.parametrize('name', NC.EDGE_ORDER)
def test_edge_case_equals_brute_force(name):
    ref, q, ties = NC.edge_case(name)
    index = NearestIndex(ref)
    dist, idx = index.query(q, return_distance=True)
    _check(name, dist, idx)
    assert torch.equal(index.query(q), idx)
    if name == 'overflow':
        assert bool((idx == 1).all()) and bool(torch.isinf(dist).all())
    if name in ('line', 'large'):                                            # the largest builds: twice, the same bits
        d2, i2 = NearestIndex(ref).query(q, return_distance=True)
        assert torch.equal(i2, idx) and torch.equal(d2.view(torch.int64), dist.view(torch.int64))


@pytest.mark.parametrize('kind', list(NC.SHELL_DIRS))
def test_the_winner_of_every_shell(kind):
    """The true nearest row lies r = 0 ... 6 cells from the query's cell and the only row of a nearer shell is farther away: the walk
    must neither stop at the decoy nor run past the winner's distance."""
    for r in NC.SHELL_R:
        name = 'shell:%s:%d' % (kind, r)
        ref, q, winner, decoy, _ = NC.shell_case(kind, r)
        dist, idx = NearestIndex(ref).query(q, return_distance=True)
        assert int(idx[0]) == winner != decoy, (name, int(idx[0]), winner, decoy)
        _check(name, dist, idx)


def test_entry_checks():
    lib = _lib.load()
    assert lib.b2m_nn_workspace(2 ** 29 - 1) > 0 and lib.b2m_nn_workspace(2 ** 29) < 0
    ref, q, _ = NC.edge_case('sizes:257x257')
    r, qq = torch.from_numpy(np.array(ref)).cuda(), torch.from_numpy(np.array(q)).cuda()
    work = torch.empty((lib.b2m_nn_workspace(257) + 7) // 8, dtype=torch.int64, device='cuda')
    _lib.call('b2m_nn_build', r.data_ptr(), 257, work.data_ptr())
    idx = torch.full((257,), 0x5a5a5a5a, dtype=torch.int32, device='cuda')
    for n_ref, n_q in ((257, 2 ** 31), (2 ** 29, 257), (257, -1)):           # refused on the arguments alone
        with pytest.raises(_lib.B2MError):
            _lib.call('b2m_nn_query', r.data_ptr(), n_ref, work.data_ptr(), qq.data_ptr(), n_q, idx.data_ptr(), None)
    with pytest.raises(_lib.B2MError):
        _lib.call('b2m_nn_build', r.data_ptr(), 2 ** 29, work.data_ptr())
    torch.cuda.synchronize()
    assert bool((idx == 0x5a5a5a5a).all())


def test_one_index_queried_from_two_streams():
    """One build, then separate query calls on two streams: the workspace is only read, so both give the bits of the default stream."""
    ref, q, _ = NC.edge_case('long_scan')
    index = NearestIndex(ref)
    base = index.query(q, return_distance=True)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for _ in range(2):
        for s in streams:
            with torch.cuda.stream(s):
                outs.append(index.query(q, return_distance=True))
    torch.cuda.synchronize()
    for d, i in outs:
        assert torch.equal(i, base[1]) and torch.equal(d.view(torch.int64), base[0].view(torch.int64))
    _check('long_scan', *base)
