"""S3DIS evaluation on the device (box2mask_amd/eval_s3dis.py, csrc/cluster.hip) against the fixture taken from the reference's
own code (tools/gen_golden.py s3dis) and against the brute-force restatement of the labelling rule (tests/_s3dis_rule.py).
Everything is compared exactly unless said otherwise."""
import numpy as np
import pytest
import torch

from box2mask_amd import eval_s3dis as S, synth

import _s3dis_rule as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gold():
    return np.load(R.GOLD)


@pytest.fixture(scope='module')
def rooms(gold):
    return [R.room(gold, r) for r in range(3)]


def _labels(x, eps, ms):
    lab, count = S.dbscan(x, eps, ms, return_count=True)
    lab = lab.cpu().numpy()
    assert int(count.item()) == (lab.max() + 1 if len(lab) else 0)
    return lab


@pytest.mark.parametrize('case', [0, 1])
def test_dbscan_equals_sklearn_labels(gold, case):
    x = gold['db%d_x' % case].astype(np.float64)
    eps, ms = float(gold['db%d_eps' % case]), int(gold['db%d_min_samples' % case])
    lab = _labels(x, eps, ms)
    assert np.array_equal(lab, gold['db%d_labels' % case].astype(np.int32))
    perm = gold['db%d_perm' % case].astype(np.int64)
    assert np.array_equal(_labels(x[perm], eps, ms), gold['db%d_labels_perm' % case].astype(np.int32))
    assert np.array_equal(_labels(x, eps, ms), lab)                        # a second run: the same labels


def _chain():
    """Core rows along a line through more than 30 cells, negative coordinates, rows in shuffled order; a few far strays."""
    rng = np.random.default_rng(5)
    t = np.arange(0, 400) * 0.03                                            # 12 units long, eps 0.35: > 30 cells
    line = np.stack([-9.0 + t * 0.8, -3.0 + t * 0.6, -0.5 + 0 * t], 1)      # unit direction (0.8, 0.6, 0)
    strays = rng.uniform(20.0, 30.0, (7, 3))
    x = np.concatenate([line, strays])
    return x[rng.permutation(len(x))]


def _shared_border():
    """Two clusters of 10 rows each and one row between them that is a neighbour of three core rows of the one and two of the
    other (six neighbours with itself: not core).  Distances are 0.2995 or 0.3005 where it matters."""
    a = np.array([[0.001 * i, 0.0, 0.0] for i in range(10)])
    b = np.array([[0.605 + 0.001 * i, 0.0, 0.0] for i in range(10)])
    mid = np.array([[0.3065, 0.0, 0.0]])
    return np.concatenate([b, mid, a])                                       # the later group first: numbering follows the rows


SMALL = {
    'one_row': (np.array([[0.25, -1.0, 3.0]]), 0.35, 1),
    'one_row_noise': (np.array([[0.25, -1.0, 3.0]]), 0.35, 2),
    'nine_identical': (np.tile([[1.0, 2.0, 3.0, 0.0, 0.0, 2.0]], (9, 1)), 0.35, 10),
    'ten_identical': (np.tile([[1.0, 2.0, 3.0, 0.0, 0.0, 2.0]], (10, 1)), 0.35, 10),
    'chain': (_chain(), 0.35, 3),
    'shared_border': (_shared_border(), 0.3, 10),
}


@pytest.mark.parametrize('name', sorted(SMALL))
def test_dbscan_small_shapes_against_the_rule(name):
    x, eps, ms = SMALL[name]
    want, core, two = R.dbscan_rule(x, eps, ms)
    if name == 'chain':
        assert want.max() == 0 and (want == -1).sum() == 7
        cells = np.unique(np.floor(x[want == 0] / eps), axis=0)
        assert len(cells) > 30 and (x[want == 0] < 0).any()
    if name == 'shared_border':
        assert want.max() == 1 and two.sum() == 1 and want[two][0] == 0 and want[0] == 0 and want[-1] == 1
    if name == 'nine_identical':
        assert (want == -1).all()
    if name == 'ten_identical':
        assert (want == 0).all()
    assert np.array_equal(_labels(x, eps, ms), want)


@pytest.mark.parametrize('d', [3, 8])
def test_dbscan_three_and_eight_columns(gold, d):
    x = gold['db0_x'].astype(np.float64)[:1500]
    x = x[:, :3] if d == 3 else np.concatenate([x, x[:, :2] * 0.5], 1)
    eps, ms = (0.12, 4) if d == 3 else (0.3, 4)
    assert R.margin(x, eps) >= 1e-12
    want, core, _ = R.dbscan_rule(x, eps, ms)
    assert want.max() >= 3 and (want < 0).any() and ((want >= 0) & ~core).any()
    assert np.array_equal(_labels(x, eps, ms), want)


def test_dbscan_cell_larger_than_a_tile_and_empty_input():
    x = np.tile([[-2.0, 0.5, 7.0, 0.0, 2.0, 0.0]], (5000, 1))              # one cell, 20 LDS tiles, every pair a neighbour
    x[4990:, 0] += 100.0                                                    # ten rows elsewhere: the second cluster
    lab = _labels(x, 0.35, 10)
    assert (lab[:4990] == 0).all() and (lab[4990:] == 1).all()
    lab, count = S.dbscan(np.zeros((0, 6)), 0.35, 10, return_count=True)
    assert lab.shape == (0,) and lab.dtype == torch.int32 and int(count.item()) == 0


@pytest.mark.parametrize('room', [0, 1, 2])
def test_room_stages_equal_the_reference(rooms, room):
    rm = rooms[room]
    bg = S.clustering_for_background(rm['pred_semantics'], rm['positions'], rm['normals'])
    assert np.array_equal(bg.cpu().numpy(), rm['background'])
    ps = S.assign_semantics_to_proposals(rm['pred_semantics'], rm['masks'])
    assert np.array_equal(ps.cpu().numpy(), rm['proposal_semantics'])
    out = S.room_labels(rm['pred_semantics'], rm['positions'], rm['normals'], torch.from_numpy(rm['masks']))
    assert np.array_equal(out['semantics'].cpu().numpy(), rm['final']['semantics'])
    assert np.array_equal(out['instances'].cpu().numpy(), rm['final']['instances'])


def test_room_labels_without_proposals(rooms):
    """K == 0: only the background instances remain, shifted by the maximum of an all -1 column (evaluation.py:197-199: the
    ceiling's 1 becomes 0 and is not written, the floor is 1, the walls 3 and 4), then pruned per class."""
    rm = rooms[0]
    n = rm['n']
    for masks in (np.zeros((0, n), bool), torch.zeros((0, n), dtype=torch.bool)):
        out = S.room_labels(rm['pred_semantics'], rm['positions'], rm['normals'], masks, details=True)
        assert out['accepted'].shape == (0,) and out['proposal_semantics'].shape == (0,)
        assert np.array_equal(out['semantics'].cpu().numpy(), rm['pred_semantics'])
        bg = rm['background']
        want = np.where(bg - 1 > 0, bg - 1, -1)
        assert np.array_equal(out['instances'].cpu().numpy(), want)


def test_joint_hist_refuses_other_layouts():
    a = torch.zeros(8, dtype=torch.int64, device='cuda')
    with pytest.raises(AssertionError):
        S.joint_hist(a, None, 4)
    a = torch.zeros(16, dtype=torch.int32, device='cuda')
    with pytest.raises(AssertionError):
        S.joint_hist(a[::2], None, 4)
    with pytest.raises(AssertionError):
        S.joint_hist(a, a[:8], 4, 4)


def test_background_without_wall_points():
    sem = np.array([0, 1, 5, 0, 7], np.int64)
    bg = S.clustering_for_background(sem, np.zeros((5, 3)), np.zeros((5, 3)))
    assert bg.cpu().tolist() == [1, 2, 0, 1, 0]


def test_paint_proposals_toy():
    """300 points, four rows in which each of the three tests rejects exactly once: a class below 3 (the row would pass the other
    two); an accepted row; a row of which 0.4 is left unlabeled; a row that is unlabeled throughout and has 80 points."""
    n = 300
    masks = np.zeros((4, n), bool)
    masks[0, :250] = True                       # class 1
    masks[1, :220] = True                       # accepted: 220 of 220
    masks[2, 100:300] = True                    # 200 points, 80 unlabeled: 0.4 < 0.6
    masks[3, 220:300] = True                    # 80 of 80 unlabeled: ratio 1.0, under 200 points
    sem = torch.tensor([1, 5, 6, 8], dtype=torch.int32, device='cuda')
    bits, words, _ = S.pack_masks(masks)
    point_sem = torch.full((n,), 2, dtype=torch.int32, device='cuda')
    inst, sem_out, accepted = S.paint_proposals(bits, words, n, sem, point_sem)
    assert accepted.cpu().tolist() == [0, 1, 0, 0]
    want = np.full(n, -1); want[:220] = 2
    assert np.array_equal(inst.cpu().numpy(), want)
    want_sem = np.full(n, 2); want_sem[:220] = 5
    assert np.array_equal(sem_out.cpu().numpy(), want_sem)
    assert np.array_equal(point_sem.cpu().numpy(), np.full(n, 2))          # the caller's semantics are left alone


def test_joint_hist_against_numpy():
    rng = np.random.default_rng(3)
    n = 70001
    for na, nb in ((13, 13), (700, 9)):         # the LDS table and the global one
        a = rng.integers(-1, na + 1, n).astype(np.int32)
        b = rng.integers(-1, nb + 1, n).astype(np.int32)
        got = S.joint_hist(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), na, nb).cpu().numpy()
        ok = (a >= 0) & (a < na) & (b >= 0) & (b < nb)
        want = np.zeros((na, nb), np.int64)
        np.add.at(want, (a[ok], b[ok]), 1)
        assert np.array_equal(got, want)
    got = S.joint_hist(torch.from_numpy(a).cuda(), None, 700).cpu().numpy()[:, 0]
    assert np.array_equal(got, np.bincount(a[(a >= 0) & (a < 700)], minlength=700))


def test_counts_and_metric_equal_the_reference(gold, rooms):
    z = gold
    finals = [rm['final'] for rm in rooms]
    gts = [rm['gt'] for rm in rooms]
    counts = S.s3dis_counts(finals[0], gts[0])
    want = R.counts_numpy(finals[0], gts[0])
    for k in want:
        assert np.array_equal(counts[k], want[k]), k
    for tag, sel in (('rooms01', slice(0, 2)), ('room2', slice(2, 3))):
        mprec, mrec, prec, rec, extra = S.s3dis_eval(finals[sel], gts[sel], details=True)
        assert np.array_equal(prec, z[tag + '_precision'], equal_nan=True) and np.array_equal(rec, z[tag + '_recall'], equal_nan=True)
        assert np.array_equal(np.float64(mprec), z[tag + '_mprec'], equal_nan=True)
        assert np.array_equal(np.float64(mrec), z[tag + '_mrec'], equal_nan=True)
        ref = R.details_numpy(finals[sel], gts[sel])
        for k in ('oAcc', 'iou', 'mIoU', 'MUCov', 'MWCov'):
            assert np.allclose(extra[k], ref[k], rtol=0, atol=1e-12, equal_nan=True), (tag, k)


def _room_batch(rm, voxel_size=0.02):
    """Room 0 of the fixture as a one-room batch in the layout of synth.make_scene / synth.collate (dataloader.py:61-123)."""
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
    """The real model behind a teacher: the per-voxel logits get +50 on the fixture's predicted class of the voxel's first point
    and the masks of the votes -> masks pass are replaced by the fixture's proposals, so that an UNTRAINED network gives a room in
    which every class has predicted instances (the network and pred2mask still run on the batch)."""

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


def test_evaluate_rooms_end_to_end(rooms):
    """The LOOP of evaluate_rooms on a one-room batch under the head list of the S3DIS configuration (tests/test_gpu_configs.py
    builds it the same way: scannet_config with the per-voxel semantics head).  This proves the plumbing only -- the network and
    pred2mask run on the batch and their shapes are checked, but `_Taught` overrides the logits and replaces the masks, so the
    network's own prediction does not reach room_labels: an untrained network cannot give predicted instances of all 13 classes,
    which finite precisions need.  The prediction path itself is covered by tests/test_gpu_configs.py."""
    from box2mask_amd.config import scannet_config
    from box2mask_amd.model import Model
    cfg = scannet_config(network_heads=['mlp_offsets', 'mlp_bounds', 'mlp_bb_scores', 'mlp_per_vox_semantics'],
                         eval_ths=[0.5, 0.03, 0.3, 0.6], loss_weight_bb_scores=3.0, batch_size=4)
    valid = torch.Tensor(np.arange(13))
    id2idx = torch.arange(13).long()
    torch.manual_seed(0)
    model = Model(cfg, valid, id2idx, id2idx.clone(), (lambda s: s > 2))
    model.eval()
    batch, first = _room_batch(rooms[0])
    taught = _Taught(model, rooms[0], first)
    mprec, mrec, prec, rec = S.evaluate_rooms(taught, [batch])
    assert prec.shape == (13,) and rec.shape == (13,)
    assert np.isfinite(prec).all() and np.isfinite(rec).all() and np.isfinite(mprec) and np.isfinite(mrec)
    assert mprec == np.mean(prec) and mrec == np.mean(rec)
    cfg.full_resolution = True
    with pytest.raises(NotImplementedError):
        S.evaluate_rooms(taught, [batch])
    cfg.full_resolution = False
    with pytest.raises(NotImplementedError):
        S.evaluate_rooms(taught, [batch], viz_path='somewhere')
