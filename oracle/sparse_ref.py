"""ORACLE (test infrastructure, never shipped, never the thing measured except as `cpu_baseline`).

CPU restatement of the sparse-tensor engine the reference reaches through MinkowskiEngine 0.5.4
(un-vendored third-party dependency, pinned in /root/reference/docs/installation.md:6,42).

PARITY UNPINNED for everything in this file: MinkowskiEngine is neither vendored in
/root/reference nor installed, and the reference ships no tests or golden vectors at this
boundary.  The restatement follows the semantics observable from the reference's
call sites (file:line cited per function) plus ME 0.5.4's published behaviour, and is validated by
independent checks in tests/test_oracle_sparse.py: dense equivalence against
torch.nn.functional.conv3d / conv_transpose3d, brute-force dictionary kernel maps, BatchNorm1d,
scatter_reduce and fp64 gradcheck.

Conventions:
  * coordinates (N,4) int [b,x,y,z] >= 0; a level with tensor stride ts holds multiples of ts
  * kernel offset index enumerates offsets with the first spatial axis (x) fastest
  * odd kernels are centred, even kernels use offsets {0..k-1}*ts, strided output coordinate is
    floor(c / (s*ts)) * (s*ts)
  * transposed convolution re-uses the existing finer coordinate map (no new coordinates)
  * row order of a strided level = order of first occurrence of each coarse voxel in the finer
    level's row order (the build's own canonical, deterministic order; ME's is a hash artefact)
Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module.
"""
from __future__ import annotations

import numpy as np
import torch


# ----------------------------------------------------------------------------- coordinates
def pack_keys(coords: np.ndarray) -> np.ndarray:
    """(N,4) non-negative ints -> int64 keys, 16 bits per field (b,x,y,z)."""
    c = np.asarray(coords).astype(np.int64)
    assert c.ndim == 2 and c.shape[1] == 4
    assert c.min(initial=0) >= 0 and c.max(initial=0) < 65536
    return (c[:, 0] << 48) | (c[:, 1] << 32) | (c[:, 2] << 16) | c[:, 3]


def kernel_offsets(ksize: int, ts: int) -> np.ndarray:
    """(K,3) integer offsets of a cubic kernel at tensor stride ts, x fastest.
    Odd k: {-k//2..k//2}*ts; even k: {0..k-1}*ts  ([ME-mem])."""
    if ksize % 2 == 1:
        r = np.arange(-(ksize // 2), ksize // 2 + 1)
    else:
        r = np.arange(0, ksize)
    dz, dy, dx = np.meshgrid(r, r, r, indexing='ij')   # x fastest in the flattened order
    return np.stack([dx.ravel(), dy.ravel(), dz.ravel()], 1).astype(np.int64) * ts


def stride_coords(coords: np.ndarray, ts: int):
    """k=2,s=2 coordinate generation (/root/reference/models/detection_net.py:42,48,54,61,68,74,81).
    Returns (coords_out (M,4), parent (N,) row of the coarse voxel, koff (N,) kernel index 0..7).
    Output rows are ordered by first occurrence in the input order."""
    c = np.asarray(coords).astype(np.int64)
    ts2 = 2 * ts
    coarse = c.copy()
    coarse[:, 1:] = (c[:, 1:] // ts2) * ts2
    keys = pack_keys(coarse)
    uniq, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    order = np.argsort(first, kind='stable')            # unique-id -> rank by first occurrence
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    parent = rank[inv.reshape(-1)]
    coords_out = coarse[first[order]]
    o = (c[:, 1:] - coarse[:, 1:]) // ts                 # in {0,1}^3
    koff = o[:, 0] + 2 * o[:, 1] + 4 * o[:, 2]
    return coords_out.astype(np.int32), parent.astype(np.int32), koff.astype(np.int32)


def kernel_map_same(coords: np.ndarray, ksize: int, ts: int) -> np.ndarray:
    """Stride-1 kernel map as a neighbour table nbr[k, o] = input row at coords[o]+offset_k or -1.
    (/root/reference/models/resnet.py:61-65, detection_net.py:37)"""
    c = np.asarray(coords).astype(np.int64)
    keys = pack_keys(c)
    order = np.argsort(keys, kind='stable')
    skeys = keys[order]
    offs = kernel_offsets(ksize, ts)
    K, N = len(offs), len(c)
    nbr = np.full((K, N), -1, np.int32)
    for k in range(K):
        q = c.copy()
        q[:, 1:] += offs[k]
        ok = (q[:, 1:] >= 0).all(1) & (q[:, 1:] < 65536).all(1)
        qk = pack_keys(np.where(ok[:, None], q, 0))
        pos = np.searchsorted(skeys, qk)
        pos = np.minimum(pos, N - 1)
        hit = ok & (skeys[pos] == qk)
        nbr[k, hit] = order[pos[hit]]
    return nbr


def kernel_map_bruteforce(coords: np.ndarray, ksize: int, ts: int) -> np.ndarray:
    """Dictionary O(N*K) kernel map, used only to check kernel_map_same on small inputs."""
    c = [tuple(int(v) for v in r) for r in np.asarray(coords)]
    d = {r: i for i, r in enumerate(c)}
    offs = kernel_offsets(ksize, ts)
    nbr = np.full((len(offs), len(c)), -1, np.int32)
    for o, (b, x, y, z) in enumerate(c):
        for k, (dx, dy, dz) in enumerate(offs):
            nbr[k, o] = d.get((b, x + int(dx), y + int(dy), z + int(dz)), -1)
    return nbr


def child_table(parent: np.ndarray, koff: np.ndarray, n_out: int) -> np.ndarray:
    """k2s2 map as a neighbour table over coarse rows: child[k, o] = fine row or -1."""
    t = np.full((8, n_out), -1, np.int32)
    t[koff, parent] = np.arange(len(parent), dtype=np.int32)
    return t


def up_table(parent: np.ndarray, koff: np.ndarray) -> np.ndarray:
    """Transposed k2s2 map as a neighbour table over fine rows: up[k, i] = parent[i] iff koff[i]==k."""
    n = len(parent)
    t = np.full((8, n), -1, np.int32)
    t[koff, np.arange(n)] = parent
    return t


# ----------------------------------------------------------------------------- dense ops (torch CPU, autograd)
def conv_nbr(x: torch.Tensor, w: torch.Tensor, nbr, bias: torch.Tensor | None = None) -> torch.Tensor:
    """Y[o] = sum_k X[nbr[k,o]] @ W[k]   (+bias).  The per-offset index_select -> mm -> index_add_
    formulation of ME's gather-GEMM-scatter.  w: (K,Cin,Cout) or (Cin,Cout) for 1x1."""
    if nbr is None:                                   # 1x1 conv: plain mm
        y = x @ (w if w.dim() == 2 else w[0])
    else:
        nbr_t = torch.as_tensor(np.asarray(nbr), dtype=torch.long)
        K, n_out = nbr_t.shape
        y = torch.zeros(n_out, w.shape[-1], dtype=x.dtype)
        for k in range(K):
            o = torch.nonzero(nbr_t[k] >= 0).reshape(-1)
            if o.numel() == 0:
                continue
            y = y.index_add(0, o, x.index_select(0, nbr_t[k, o]) @ w[k])
    if bias is not None:
        y = y + bias.reshape(1, -1)
    return y


def conv_nbr_explicit(x: torch.Tensor, w: torch.Tensor, nbr, gy: torch.Tensor | None = None):
    """Forward and, given dL/dY, the data and weight gradients of `conv_nbr`, written out per offset from the
    definition (no autograd tape, in-place accumulation) so that whole 150 k .. 1.2 M-row layers fit the host:
        Y[o]    += X[i] W[k]          dX[i] += dY[o] W[k]^T          dW[k] = X[i]^T dY[o]      over pairs (i,o) of k.
    tests/test_oracle_sparse.py checks it against autograd of `conv_nbr`.  Returns (y, dx, dw); dx/dw None without gy."""
    nbr_t = torch.as_tensor(np.asarray(nbr), dtype=torch.long)
    K, n_out = nbr_t.shape
    w3 = w if w.dim() == 3 else w.unsqueeze(0)
    with torch.no_grad():
        y = torch.zeros(n_out, w3.shape[2], dtype=x.dtype)
        dx = torch.zeros_like(x) if gy is not None else None
        dw = torch.zeros_like(w3) if gy is not None else None
        for k in range(K):
            o = torch.nonzero(nbr_t[k] >= 0).reshape(-1)
            if o.numel() == 0:
                continue
            i = nbr_t[k, o]
            xi = x.index_select(0, i)
            y.index_add_(0, o, xi @ w3[k])
            if gy is not None:
                go = gy.index_select(0, o)
                dx.index_add_(0, i, go @ w3[k].t())
                dw[k] = xi.t() @ go
    return y, dx, (dw.reshape(w.shape) if dw is not None else None)


def batch_norm(x, weight, bias, running_mean, running_var, training, momentum=0.1, eps=1e-5):
    """MinkowskiBatchNorm == BatchNorm1d on the feature matrix."""
    return torch.nn.functional.batch_norm(x, running_mean, running_var, weight, bias, training, momentum, eps)


def segment_pool(x: torch.Tensor, ids: torch.Tensor, n_seg: int, mode: str = 'avg') -> torch.Tensor:
    """Global avg/max pool by batch index after the batch column was overwritten with pooling ids
    (/root/reference/models/detection_net.py:345-352); output row r <-> pooling id r."""
    idx = ids.reshape(-1, 1).expand(-1, x.shape[1])
    out = torch.zeros(n_seg, x.shape[1], dtype=x.dtype)
    if mode == 'avg':
        return out.scatter_reduce(0, idx, x, 'mean', include_self=False)
    # max: the value of ONE row per (segment, channel), the lowest row among equal maxima, so the gradient goes to that row alone
    # (scatter_reduce('amax') would split it among the ties); an empty segment gives 0 and no gradient.  That a max pooling
    # routes its gradient to a single index is how such operators are built (an arg-max index per output); WHICH of several
    # equal rows MinkowskiEngine picks is an ASSUMPTION here -- the engine is not available to observe
    n = x.shape[0]
    if n == 0 or n_seg == 0:
        return out + x.sum() * 0                       # (all zeros, still a function of x for autograd)
    top = out.scatter_reduce(0, idx, x.detach(), 'amax', include_self=False)
    rows = torch.arange(n).reshape(-1, 1).expand_as(idx)
    cand = torch.where(x.detach() == top[ids.reshape(-1)], rows, torch.full_like(rows, n))
    arg = torch.full((n_seg, x.shape[1]), n, dtype=torch.int64).scatter_reduce(0, idx, cand, 'amin', include_self=True)
    return torch.where(arg < n, x.gather(0, arg.clamp(max=n - 1)), out)


# ----------------------------------------------------------------------------- binary16 storage (half_train.py's rule)
def to_binary16(x: torch.Tensor) -> torch.Tensor:
    """x rounded to IEEE binary16 and back in x's dtype: ONE round-to-nearest-even, subnormals kept, no saturation (past 65520: inf).
    For fp32 that is `x.half()`.  torch converts an fp64 tensor by way of fp32 -- two roundings, which send 1 + 2^-11 + 2^-30 down to 1
    instead of up to 1 + 2^-10 -- so fp64 goes through numpy, whose conversion rounds the double itself."""
    if x.dtype == torch.float64:
        with np.errstate(over='ignore'):
            return torch.from_numpy(x.detach().contiguous().numpy().astype(np.float16).astype(np.float64)).reshape(x.shape)
    return x.half().to(x.dtype)


class _Stored(torch.autograd.Function):
    """forward: x -> to_binary16(x) where `round_forward`, else the identity; backward: g -> to_binary16(g * s) / s."""

    @staticmethod
    def forward(ctx, x, st, round_forward, kind):
        ctx.st, ctx.kind = st, kind
        if not round_forward:
            return x.view_as(x)
        st.max_activation = max(st.max_activation, float(x.detach().abs().max()) if x.numel() else 0.0)
        return to_binary16(x)

    @staticmethod
    def backward(ctx, g):
        st = ctx.st
        gs = g * st.loss_scale
        m = float(gs.abs().max()) if gs.numel() else 0.0
        st.max_scaled_gradient = max(st.max_scaled_gradient, m)
        st.max_scaled_gradient_at[ctx.kind] = max(st.max_scaled_gradient_at.get(ctx.kind, 0.0), m)
        return to_binary16(gs) / st.loss_scale, None, None, None


class HalfStorage:
    """The storage rule of box2mask_amd/half_train.py for an oracle pass in any arithmetic dtype: a tensor the device keeps in HBM
    as IEEE binary16 is rounded to binary16 (round to nearest even, subnormals kept, no saturation) at the
    place the device writes it (`to_binary16`), and converted back; every sum in between stays in the caller's dtype.

    `point(x)`     -- a storage point: forward x -> half(x); backward g -> half(g * s) / s.  The oracle's graph is NOT scaled: s
                      is a power of two, so rounding "as if scaled by s" is exact -- only the subnormal range and the overflow
                      threshold of the rounding move, which is all the loss scale does on the device.
    `weight(w)`    -- the binary16 image of fp32 master weights; the gradient passes through un-rounded.
    `grad_only(x)` -- forward the identity, backward the same rounding: where the device writes a half gradient that autograd
                      would otherwise add un-rounded to another one.
    `count[kind]` counts the storage points hit; `max_activation` / `max_scaled_gradient` are the largest magnitudes that met a
    rounding (before it), for the saturation head-room."""

    def __init__(self, loss_scale: float = 1024.0):
        self.loss_scale = float(loss_scale)
        m, e = np.frexp(self.loss_scale)
        assert m == 0.5 and self.loss_scale > 0, 'the loss scale is a power of two'
        self.count = {}
        self.max_activation = 0.0
        self.max_scaled_gradient = 0.0
        self.max_scaled_gradient_at = {}          # the same per kind of point ('grad_only': the gradient-only points)

    def point(self, x, kind='activation'):
        self.count[kind] = self.count.get(kind, 0) + 1
        return _Stored.apply(x, self, True, kind)

    def grad_only(self, x):
        return _Stored.apply(x, self, False, 'grad_only')

    def weight(self, w):
        """The binary16 image of a layer's fp32 master weights (half_train._HalfImages): what the forward and the data gradient
        multiply with.  The weight gradient is that of the image, un-rounded, handed to the master weight as it is."""
        self.count['weight'] = self.count.get('weight', 0) + 1
        return _StoredWeight.apply(w)


class _StoredWeight(torch.autograd.Function):
    """forward: w -> to_binary16(w); backward: the identity (the gradient of the image is the gradient of the master weight)."""

    @staticmethod
    def forward(ctx, w):
        return to_binary16(w)

    @staticmethod
    def backward(ctx, g):
        return g


class _ScaleGrad(torch.autograd.Function):
    """identity; the gradient times `factor` (only for the deliberate mistakes of tests/test_half_oracle_rule.py)."""

    @staticmethod
    def forward(ctx, x, factor):
        ctx.factor = factor
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.factor, None


# ----------------------------------------------------------------------------- coordinate hierarchy
class Hierarchy:
    """All coordinate maps / kernel maps SelectionNet needs for one batch (8 levels)."""

    def __init__(self, coords, n_levels: int = 8, k0: int = 5):
        c0 = np.asarray(coords).astype(np.int32)
        self.coords = [c0]
        self.parent, self.koff = [], []
        for l in range(n_levels - 1):
            co, p, ko = stride_coords(self.coords[l], 1 << l)
            self.coords.append(co); self.parent.append(p); self.koff.append(ko)
        self._k3, self._k5 = {}, None
        self.k0 = k0

    def n(self, l):
        return len(self.coords[l])

    def k3(self, l):
        if l not in self._k3:
            self._k3[l] = kernel_map_same(self.coords[l], 3, 1 << l)
        return self._k3[l]

    def k_first(self):
        if self._k5 is None:
            self._k5 = kernel_map_same(self.coords[0], self.k0, 1)
        return self._k5

    def down(self, l):      # level l -> l+1, table over coarse rows
        return child_table(self.parent[l], self.koff[l], self.n(l + 1))

    def up(self, l):        # level l+1 -> l, table over fine rows
        return up_table(self.parent[l], self.koff[l])
