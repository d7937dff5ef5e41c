"""Dense-grid equivalents of the sparse maps, shared by the CPU rule test (tests/test_conv_rule.py) and the device test
(tests/test_gpu_conv_regimes.py): random occupancy, the conv3d weight layout, scatter to / read from a dense [b, c, x, y, z] grid."""
import numpy as np
import torch


def random_sites(B, X, Y, Z, density, seed):
    rng = np.random.default_rng(seed)
    occ = rng.random((B, X, Y, Z)) < density
    occ[:, 0, 0, 0] = True                       # pin the grid origin so that dense and sparse indices agree
    c = np.argwhere(occ).astype(np.int32)
    return c[rng.permutation(len(c))]            # rows in random order


def dense_weight(w, k):
    """(K,Cin,Cout), offset index x-fastest -> conv3d weight (Cout,Cin,kx,ky,kz) for a dense [b,c,x,y,z] grid."""
    K, ci, co = w.shape
    return w.reshape(k, k, k, ci, co).permute(4, 3, 2, 1, 0).contiguous()


def scatter_dense(feat, coords, shape, ts=1):
    B, X, Y, Z = shape
    d = torch.zeros(B, feat.shape[1], X, Y, Z, dtype=feat.dtype)
    c = torch.as_tensor(coords).long()
    d[c[:, 0], :, c[:, 1] // ts, c[:, 2] // ts, c[:, 3] // ts] = feat
    return d


def read_dense(d, coords, ts=1):
    c = torch.as_tensor(coords).long()
    return d[c[:, 0], :, c[:, 1] // ts, c[:, 2] // ts, c[:, 3] // ts]
