"""GPU: what ``SelectionNet.detection2mask`` and the threshold sweeps launch now that they share box2mask_amd/mask_stages.py -- the
entry names in order, seen through ``_lib.set_hook`` -- and the segment vote of the S3DIS flow on ties, in the single-setting path
and in the sweep's stage 0.  Two synthetic scenes of a few hundred voxels."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HEADS_S3DIS = ['mlp_offsets', 'mlp_bounds', 'mlp_bb_scores', 'mlp_per_vox_semantics']
FRONT = ['b2m_nmc_batch', 'b2m_mask_project_batch']


def _launches(fn):
    """The names of every library entry ``fn`` calls, in order."""
    from box2mask_amd import _lib
    names = []
    _lib.set_hook(lambda name, args, meta: names.append(name))
    try:
        fn()
    finally:
        _lib.set_hook(None)
    return names


def _bench_stages():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'bench_param_sweep.py')
    spec = importlib.util.spec_from_file_location('bench_param_sweep', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.STAGES, mod.ARKIT_STAGES


@pytest.fixture(scope='module')
def scenes():
    """(batch, votes of the ScanNet flow, votes of the S3DIS flow) of two scenes: every segment votes for its object's box."""
    from box2mask_amd import synth
    from box2mask_amd.config import scannet_config
    cfg = scannet_config()
    batch = synth.make_batch(2, seed0=3, target_voxels=600, pts_per_m2=6000.0)
    valid, id2idx, _, _ = synth.scannet_tables()
    S = batch['input_location'].shape[0]
    g = torch.Generator().manual_seed(5)
    sem_idx = id2idx[batch['gt_semantics']].clamp_min(0)
    pred = {cfg.mlp_offsets: batch['gt_bb_offsets'] + 0.025 * torch.randn(S, 3, generator=g),
            cfg.mlp_bounds: (batch['gt_bb_bounds'] + 0.025 * torch.randn(S, 3, generator=g)).clamp_min(cfg.min_bb_size),
            cfg.mlp_bb_scores: 2.0 * torch.randn(S, 1, generator=g),
            cfg.mlp_semantics: torch.nn.functional.one_hot(sem_idx, len(valid)).float()}
    # S3DIS flow: a class in 0 .. 12 per voxel, that of the voxel's segment; the rows of the scenes back to back
    sem13 = sem_idx % 13
    vox = torch.cat([sem13[batch['batch_ids'] == b][torch.as_tensor(np.asarray(batch['seg2vox'][b])).long()] for b in range(2)])
    assert vox.shape[0] == batch['vox_coords'].shape[0] and all(200 < len(v) < 1000 for v in batch['seg2vox'])
    pred3 = {k: v for k, v in pred.items() if k != cfg.mlp_semantics}
    pred3[cfg.mlp_per_vox_semantics] = torch.nn.functional.one_hot(vox, 13).float()
    return batch, pred, pred3


@pytest.fixture(scope='module')
def model():
    from box2mask_amd import synth
    from box2mask_amd.config import scannet_config
    from box2mask_amd.model import Model
    return Model(scannet_config(), *synth.scannet_tables())


@pytest.fixture(scope='module')
def model3():
    from box2mask_amd.config import scannet_config
    from box2mask_amd.model import Model
    ids = torch.arange(13).long()
    return Model(scannet_config(network_heads=HEADS_S3DIS), torch.Tensor(np.arange(13)), ids, ids.clone(), (lambda s: s > 2))


@pytest.mark.parametrize('mode', ['eval', 'train'])
@pytest.mark.parametrize('gather_t', [None, '0'])
def test_detection2mask_launches_scannet_flow(model, scenes, monkeypatch, mode, gather_t):
    batch, pred, _ = scenes
    if gather_t is None:
        monkeypatch.delenv('B2M_MASK_GATHER_T', raising=False)
    else:
        monkeypatch.setenv('B2M_MASK_GATHER_T', gather_t)
    res = {}
    names = _launches(lambda: res.update(model.pred2mask(batch, pred, mode)))
    assert sum(len(r['conf']) for r in res.values()) > 2
    assert names == FRONT + ['b2m_mask_nms_batch', 'b2m_label_hist_batch',
                             'b2m_mask_gather_batch_t' if gather_t is None else 'b2m_mask_gather_batch']


@pytest.mark.parametrize('mode', ['eval', 'train'])
def test_detection2mask_launches_s3dis_flow(model3, scenes, monkeypatch, mode):
    batch, _, pred3 = scenes
    monkeypatch.delenv('B2M_MASK_GATHER_T', raising=False)
    res = {}
    names = _launches(lambda: res.update(model3.pred2mask(batch, pred3, mode)))
    assert sum(len(r['conf']) for r in res.values()) > 2
    assert names == ['b2m_seg_mode'] * 2 + FRONT + ['b2m_label_hist_batch', 'b2m_mask_gather_batch_t']


def test_sweep_launches(model, scenes):
    """One cluster_th and one mask_bin_th: one clustering and one mask stage, whatever the number of score_th and mask_nms_th."""
    from box2mask_amd import param_search, synth
    STAGES, ARKIT_STAGES = _bench_stages()
    batch, pred, _ = scenes
    grid = param_search.ThresholdGrid([0.5], [0.05, 0.4], [0.3], [0.3, 0.6])
    assert grid.shape == (1, 2, 1, 2)
    gts = {sc['name']: synth.gt_instance_ids(batch, b) for b, sc in enumerate(batch['scene'])}
    tabs = []
    names = _launches(lambda: tabs.extend(model.pred2mask_sweep(batch, pred, grid, gts)))
    assert sum(int(t.clusters[0]['ks'][0]) for t in tabs) > 2
    assert names == list(STAGES)
    # the detection mAP: the same front half, then the hulls of the stage and one IoU call per scene with rows and boxes
    raws = [synth.make_scene(3 + s, target_voxels=600, pts_per_m2=6000.0, points_only=True) for s in range(2)]
    boxed = dict(batch, labels=[], scene=[dict(sc, positions=raw['positions']) for sc, raw in zip(batch['scene'], raws)])
    for raw, v2p in zip(raws, batch['vox2point']):
        assert len(raw['positions']) == len(v2p)
        lab = raw['labels']
        sel = np.nonzero((lab['per_instance_semantics'] > 2) & (lab['per_instance_semantics'] != 22))[0]
        boxed['labels'].append({'per_instance_bb_centers': lab['per_instance_bb_centers'][sel], 'per_instance_bb_bounds': lab['per_instance_bb_bounds'][sel],
                                'per_instance_bb_rotations': np.tile(np.eye(3).reshape(1, 9), (len(sel), 1)),
                                'per_instance_semantics': lab['per_instance_semantics'][sel]})
    names = [n for n in _launches(lambda: model.pred2mask_detection_sweep(boxed, pred, grid)) if n in ARKIT_STAGES]
    assert names[:5] == list(ARKIT_STAGES[:5])                     # (the ground-truth boxes are prepared in front of the stages)
    assert 1 <= len(names[5:]) <= 2 and set(names[5:]) == {ARKIT_STAGES[5]}


def test_s3dis_segment_vote_on_ties(model3):
    """4 segments over 9 voxels: a {2, 7} tie (the lowest class wins: 2, background under s > 2), a {7, 3} tie (3, foreground), a
    clear majority and a single voxel -- np.bincount per segment with argmax taking the first of equals, in detection2mask and in
    the stage 0 of the S3DIS sweep."""
    from box2mask_amd import param_search
    from box2mask_amd.util import to_bbs_min_max
    cfg, net = model3.cfg, model3.detection_model
    assert cfg.do_segment_pooling and net.requires_voxel_outputs
    seg2vox = np.array([2, 0, 1, 2, 3, 0, 2, 1, 2], np.int64)
    sem = np.array([5, 7, 7, 1, 9, 2, 5, 3, 5], np.int64)          # segment 0: 7, 2; 1: 7, 3; 2: 5, 1, 5, 5; 3: 9
    votes = np.stack([np.bincount(sem[seg2vox == s], minlength=13) for s in range(4)])
    assert (votes[0] == votes[0].max()).sum() == 2 and (votes[1] == votes[1].max()).sum() == 2 and votes[3].sum() == 1
    want_class = votes.argmax(1)
    assert want_class.tolist() == [2, 3, 5, 9]
    want_fg = want_class > 2
    batch = {'input_location': torch.tensor([[0., 0, 0], [3, 0, 0], [6, 0, 0], [9, 0, 0]]), 'batch_ids': torch.zeros(4, dtype=torch.long),
             'scene': [{'name': 'room'}], 'seg2vox': [seg2vox], 'vox2point': [np.arange(9)[::-1].copy()]}
    pred = {cfg.mlp_offsets: torch.zeros(4, 3), cfg.mlp_bounds: torch.full((4, 3), 0.5),
            cfg.mlp_bb_scores: torch.tensor([[2.0], [1.0], [0.5], [0.0]]),
            cfg.mlp_per_vox_semantics: torch.nn.functional.one_hot(torch.from_numpy(sem), 13).float()}
    got = model3.pred2mask(batch, pred, 'train')['room']
    assert got['pred_fg'].dtype == torch.bool and np.array_equal(got['pred_fg'].numpy(), want_fg)
    d = param_search._s3dis_room(net, batch, pred, cfg, torch.device('cuda'))
    assert np.array_equal(d['fg'].numpy(), want_fg) and np.array_equal(d['fg_dev'].cpu().numpy(), want_fg)
    bbs = to_bbs_min_max(batch['input_location'], pred[cfg.mlp_offsets], pred[cfg.mlp_bounds], torch.sigmoid(pred[cfg.mlp_bb_scores]))
    assert torch.equal(d['boxes'].cpu(), bbs[torch.from_numpy(want_fg)].float()) and d['n_fg'] == 3
    assert d['fg_slot'].cpu().tolist() == [-1, 0, 1, 2]
    assert np.array_equal(d['sem_pts'].cpu().numpy(), sem[::-1])
