"""Label transfer of the raw S3DIS rooms (prepare.s3dis_point_labels) and the full-resolution evaluation (eval_s3dis.sparse2dense,
evaluate_rooms(..., full_rooms=...)) against the fixtures taken from the reference's own get_labels and Evaluater.s3dis_eval
(tools/gen_golden.py s3dis_labels, s3dis_full).  Everything is compared exactly unless said otherwise."""
import numpy as np
import pytest
import torch

from box2mask_amd import eval_s3dis as S, prepare, synth

import _s3dis_full_rule as F

pytestmark = pytest.mark.gpu


def test_point_labels_equal_the_reference():
    z = F.labels_fixture()
    inst, sem, error = prepare.s3dis_point_labels(z['scene_pts'], z['clouds'], z['class_ids'])
    n = len(z['scene_pts'])
    for t in (inst, sem):
        assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (n, 1)
    assert np.array_equal(inst.cpu().numpy(), z['instances']) and np.array_equal(sem.cpu().numpy(), z['semantics'])
    # a sum of bit-equal terms in another order: n terms of at most `error` each, rounded once per addition
    assert isinstance(error, float) and abs(error - z['error']) <= 1e-12 * z['error']
    # clouds with their colour columns, as np.loadtxt gives them, and tensors on the device: the same labels
    clouds = [torch.from_numpy(np.concatenate([c, np.full((len(c), 3), 7.0)], 1)).cuda() for c in z['clouds']]
    inst2, sem2, error2 = prepare.s3dis_point_labels(torch.from_numpy(z['scene_pts']).cuda(), clouds, list(z['class_ids']))
    assert torch.equal(inst2, inst) and torch.equal(sem2, sem) and error2 == error


def test_point_labels_refuse_what_cannot_be_matched():
    z = F.labels_fixture()
    with pytest.raises(ValueError):
        prepare.s3dis_point_labels(z['scene_pts'], z['clouds'], z['class_ids'][:-1])
    bad = z['clouds'][0].copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        prepare.s3dis_point_labels(z['scene_pts'], [bad] + z['clouds'][1:], z['class_ids'])


@pytest.mark.parametrize('room', [0, 1])
def test_sparse2dense_and_the_gather_equal_the_reference(room):
    rm = F.full_rooms()[0][room]
    s2d = S.sparse2dense(rm['full_positions'], rm['positions'])
    assert s2d.is_cuda and s2d.dtype == torch.int64 and np.array_equal(s2d.cpu().numpy(), rm['sparse2dense'])
    out = S.room_labels(rm['pred_semantics'], rm['positions'], rm['normals'], torch.from_numpy(rm['masks']))
    for k in ('semantics', 'instances'):
        assert np.array_equal(out[k][s2d].cpu().numpy(), rm['full_pred'][k]), k


def test_full_resolution_metric_equals_the_reference():
    rooms, want = F.full_rooms()
    preds = []
    for rm in rooms:
        s2d = S.sparse2dense(rm['full_positions'], rm['positions'])
        out = S.room_labels(rm['pred_semantics'], rm['positions'], rm['normals'], torch.from_numpy(rm['masks']))
        preds.append({'semantics': out['semantics'][s2d], 'instances': out['instances'][s2d]})
    mprec, mrec, prec, rec = S.s3dis_eval(preds, [rm['full_gt'] for rm in rooms])
    assert np.array_equal(prec, want[2], equal_nan=True) and np.array_equal(rec, want[3], equal_nan=True)
    assert np.array_equal(np.float64(mprec), np.float64(want[0]), equal_nan=True)
    assert np.array_equal(np.float64(mrec), np.float64(want[1]), equal_nan=True)


def _room_batch(rm, voxel_size=0.02):
    """The sampled room as a one-room batch in the layout of synth.make_scene / synth.collate (dataloader.py:61-123)."""
    pos = rm['positions']
    vox_f = np.round((pos - min(0, pos.min())) / voxel_size)
    vox_coords, first, vox2point = np.unique(vox_f, axis=0, return_index=True, return_inverse=True)
    vox2point = vox2point.reshape(-1)
    rng = np.random.default_rng(0)
    feats = np.concatenate([rng.normal(0, 1, (len(pos), 3)), rm['normals']], 1)[first].astype(np.float32)
    seg_key = rm['gt']['instances'] * 4096 + (np.floor(pos[:, 0] / 0.3) * 64 + np.floor(pos[:, 1] / 0.3)).astype(np.int64)
    _, segments = np.unique(seg_key, return_inverse=True)
    vox_segments = segments.reshape(-1)[first]
    useg, seg2vox = np.unique(vox_segments, return_inverse=True)
    cnt = np.bincount(seg2vox, minlength=len(useg)).astype(np.float64)
    world = vox_coords * voxel_size + min(0, pos.min())
    loc = np.stack([np.bincount(seg2vox, weights=world[:, d], minlength=len(useg)) / cnt for d in range(3)], 1)
    item = {'scene': {'name': 'room0', 'positions': pos, 'normals': rm['normals']}, 'labels': rm['gt'], 'vox_coords': vox_coords,
            'vox_features': feats, 'vox_segments': vox_segments, 'vox2point': vox2point, 'seg2vox': seg2vox, 'input_location': loc}
    return synth.collate([item], mode='test'), first


class _Taught:
    """The real model behind a teacher (as in tests/test_gpu_eval_s3dis.py): the per-voxel logits get +50 on the fixture's predicted
    class of the voxel's first point and the masks are replaced by the fixture's proposals; the network and pred2mask still run."""

    def __init__(self, model, rm, first):
        self.model, self.cfg, self.rm, self.first = model, model.cfg, rm, first

    def get_prediction(self, batch, **kw):
        pred = self.model.get_prediction(batch, **kw)
        logits = pred['mlp_per_vox_semantics']
        assert logits.shape == (len(self.first), 13) and bool(torch.isfinite(logits).all())
        teach = torch.from_numpy(np.eye(13, dtype=np.float32)[self.rm['pred_semantics'][self.first]]) * 50.0
        pred['mlp_per_vox_semantics'] = logits + teach.to(logits.device)
        return pred

    def pred2mask(self, batch, pred, mode):
        res = self.model.pred2mask(batch, pred, mode)
        assert res['room0']['mask'].shape[1] == self.rm['n']
        res['room0'] = dict(res['room0'], mask=torch.from_numpy(self.rm['masks']))
        return res


def test_evaluate_rooms_at_full_resolution_end_to_end():
    """The loop of evaluate_rooms with cfg.full_resolution on a one-room batch: 13 finite precisions and recalls, counted over the
    FULL room's points; the unsampled room as a sequence and through a callable; without it, NotImplementedError."""
    from box2mask_amd.config import scannet_config
    from box2mask_amd.model import Model
    cfg = scannet_config(network_heads=['mlp_offsets', 'mlp_bounds', 'mlp_bb_scores', 'mlp_per_vox_semantics'],
                         eval_ths=[0.5, 0.03, 0.3, 0.6], loss_weight_bb_scores=3.0, batch_size=4)
    cfg.full_resolution = True
    valid = torch.Tensor(np.arange(13))
    id2idx = torch.arange(13).long()
    torch.manual_seed(0)
    model = Model(cfg, valid, id2idx, id2idx.clone(), (lambda s: s > 2))
    model.eval()
    rm = F.full_rooms()[0][0]
    batch, first = _room_batch(rm)
    taught = _Taught(model, rm, first)
    full = ({'name': 'room0', 'positions': rm['full_positions']}, rm['full_gt'])
    seen = []
    real = S.s3dis_counts
    S.s3dis_counts = lambda p, g: seen.append(real(p, g)) or seen[-1]
    try:
        mprec, mrec, prec, rec = S.evaluate_rooms(taught, [batch], full_rooms=[full])
    finally:
        S.s3dis_counts = real
    assert len(seen) == 1 and seen[0]['n'] == len(rm['full_positions']) == 4 * rm['n']
    assert prec.shape == (13,) and rec.shape == (13,)
    assert np.isfinite(prec).all() and np.isfinite(rec).all() and np.isfinite(mprec) and np.isfinite(mrec)
    assert mprec == np.mean(prec) and mrec == np.mean(rec)
    again = S.evaluate_rooms(taught, [batch], full_rooms=lambda name: {'room0': full}[name])
    assert again[0] == mprec and again[1] == mrec and np.array_equal(again[2], prec) and np.array_equal(again[3], rec)
    with pytest.raises(NotImplementedError, match='full_rooms'):
        S.evaluate_rooms(taught, [batch])
