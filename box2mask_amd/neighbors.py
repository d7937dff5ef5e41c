"""Exact 1-nearest-neighbour search between two point sets on the device.

Host mirror of ``b2m_nn_workspace`` / ``b2m_nn_build`` / ``b2m_nn_query`` (include/b2m_prepare.h, csrc/neighbors.hip): what the
reference asks of ``NearestNeighbors(n_neighbors=1, algorithm='ball_tree')`` and of scipy's ``KDTree(...).query(q, k=1)``.

The contract: ``idx[j]`` is the row of ``ref`` with the smallest ``d2 = (dx*dx + dy*dy) + dz*dz`` in fp64 (no contraction: the ball
tree's reduced distance) and ``dist[j] = sqrt(d2)``.  Rows at exactly the same ``d2`` resolve to the LOWEST row -- this project's rule;
the trees' choice there is an artefact of their traversal.  A non-finite row of ``ref`` is never returned; a
non-finite query, and every query of an index without a finite row, gets ``-1`` and NaN.  The same inputs give the same bits on
every run.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import B2MError, ptr


def _points(a, dev, what):
    if isinstance(a, np.ndarray):
        a = np.ascontiguousarray(a) if a.flags.writeable else np.array(a, order='C')    # (torch refuses read-only arrays)
    t = torch.as_tensor(a)
    t = t.to(device=dev, dtype=torch.float64).contiguous()
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError('%s must be (n, 3), got %s' % (what, tuple(t.shape)))
    return t


class NearestIndex:
    """Index over the rows of ``ref`` (n, 3), array or tensor; built once, kept on the device, queried any number of times."""

    def __init__(self, ref):
        _lib.require_gpu()
        self.device = torch.device('cuda', torch.cuda.current_device())
        self.ref = _points(ref, self.device, 'ref')
        self.n = int(self.ref.shape[0])
        size = _lib.load().b2m_nn_workspace(self.n)
        if size < 0:
            raise B2MError('b2m_nn_workspace: %d rows are out of range' % self.n)
        self.workspace = torch.empty((size + 7) // 8, dtype=torch.int64, device=self.device)
        _lib.call('b2m_nn_build', ptr(self.ref), self.n, ptr(self.workspace))

    def query(self, q, return_distance=False):
        """``idx`` int64 (m) on the device, or ``(dist float64 (m), idx)`` as the trees return them."""
        q = _points(q, self.device, 'q')
        m = int(q.shape[0])
        idx = torch.empty(m, dtype=torch.int32, device=self.device)
        dist = torch.empty(m, dtype=torch.float64, device=self.device) if return_distance else None
        _lib.call('b2m_nn_query', ptr(self.ref), self.n, ptr(self.workspace), ptr(q), m, ptr(idx), ptr(dist))
        idx = idx.long()
        return (dist, idx) if return_distance else idx


def nearest(ref, q, return_distance=False):
    """One-off ``NearestIndex(ref).query(q, return_distance)``."""
    return NearestIndex(ref).query(q, return_distance=return_distance)
