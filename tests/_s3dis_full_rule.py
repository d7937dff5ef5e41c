"""Loaders of the two fixtures taken from the reference for the nearest-neighbour index (tools/gen_golden.py s3dis_labels,
s3dis_full) and numpy restatements of what the product computes from them, shared by tests/test_neighbors.py (CPU) and
tests/test_gpu_s3dis_full.py.  The restatements search by brute force in the contract's order (tests/_neighbors_cases.py)."""
import os

import numpy as np

import _neighbors_cases as NC
from _s3dis_rule import GRID, NORMALS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_cache = {}


def labels_fixture():
    """{'scene_pts', 'clouds' (list), 'class_ids', 'names', 'instances', 'semantics', 'error'} of s3dis_labels.npz."""
    if 'labels' not in _cache:
        z = np.load(os.path.join(GOLDEN, 's3dis_labels.npz'))
        _cache['labels'] = {'scene_pts': z['scene_pts'], 'clouds': [z['cloud%d' % k] for k in range(int(z['n_clouds']))],
                            'class_ids': z['class_ids'], 'names': [str(n) for n in z['names']], 'instances': z['instances'],
                            'semantics': z['semantics'], 'error': float(z['error'])}
    return _cache['labels']


def point_labels_numpy(pts, clouds, class_ids):
    """prepare.s3dis_point_labels restated: (instances float32 (n,1), semantics float32 (n,1), error)."""
    inst = np.full(len(pts), -1, np.int64)
    error = 0.0
    for k, c in enumerate(clouds):
        idx, d2, _ = NC.brute(pts, c)
        np.maximum.at(inst, idx, k)
        error += np.sqrt(d2).sum()
    decided = inst >= 0
    rows = np.nonzero(decided)[0]
    idx, _, _ = NC.brute(pts[decided], pts[~decided])
    inst[~decided] = inst[rows[idx]]
    sem = np.asarray(class_ids)[inst]
    rank = np.unique(inst, return_inverse=True)[1].reshape(-1)
    return rank.astype(np.float32).reshape(-1, 1), sem.astype(np.float32).reshape(-1, 1), error


def full_rooms():
    """The rooms of eval_s3dis_full.npz: per room the sampled room as tests/_s3dis_rule.room gives the rooms of eval_s3dis.npz
    ('positions', 'normals', 'pred_semantics', 'masks', 'gt'), 'full_positions', 'sparse2dense', 'full_pred' and 'full_gt'
    ({'semantics', 'instances'}); and the 4-tuple the reference's s3dis_eval returned over both."""
    if 'full' not in _cache:
        z = np.load(os.path.join(GOLDEN, 'eval_s3dis_full.npz'))
        rooms = []
        for r in range(int(z['n_rooms'])):
            g = lambda k: z['r%d_%s' % (r, k)]
            n = len(g('sampled'))
            rooms.append({'n': n, 'positions': g('sampled').astype(np.float64) * GRID, 'normals': NORMALS[g('normal')],
                          'pred_semantics': g('pred_semantics').astype(np.int64),
                          'masks': np.unpackbits(g('masks'), axis=1)[:, :n].astype(bool),
                          'gt': {'semantics': g('gt_semantics').astype(np.int64), 'instances': g('gt_instances').astype(np.int64)},
                          'full_positions': g('full').astype(np.float64) * GRID, 'sparse2dense': g('sparse2dense').astype(np.int64),
                          'full_pred': {'semantics': g('full_pred_semantics').astype(np.int64),
                                        'instances': g('full_pred_instances').astype(np.int64)},
                          'full_gt': {'semantics': g('full_gt_semantics').astype(np.int64),
                                      'instances': g('full_gt_instances').astype(np.int64)}})
        _cache['full'] = (rooms, (float(z['mprec']), float(z['mrec']), z['precision'], z['recall']))
    return _cache['full']
