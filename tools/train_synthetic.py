"""End-to-end run of everything the repository builds, on synthetic scenes: raw points + weak box labels -> device
batch (prepare.voxelize_scene / box_supervision / collate) -> training steps as models/training.py:63-70 does them
-> a checkpoint in the reference's format -> predictions -> instance masks -> ScanNet AP against the scenes' own
instances (eval_metric.compute_eval).  With --metric arkit the furniture instances are scored as oriented boxes as well
(their labels' boxes, a yaw of zero): the ARKitScenes detection mAP of eval_detection.arkitscenes_eval after the last step.

    python tools/train_synthetic.py --scenes 4 --voxels 20000 --steps 200 [--half 1] [--metric arkit] [--augment [--hue]]

--augment (off by default): every step trains on a batch whose scenes went through augment.augment_scenes with parameters drawn per
scene per step from the values of configs/scannet.txt (rotation_90_aug, flipping_aug 0.5, scaling_aug 0.8 - 1.2) and whose box
labels augment.instance_labels recomputed from the augmented positions; the evaluations stay on the un-augmented scenes.
--hue (with --augment): apply_hue_aug of configs/scannet.txt:37 as well, drawn with draw_params(..., byte_colour=True) and applied by
the byte-colour rule of profiles/colour8_rule.md, which also normalises the colours.  The evaluation colours are then UN-normalised --
as in the reference, whose evaluation skips the whole augmentation block (do_augmentations=False, scannet.py:221-247).
"""
import argparse
import os
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from box2mask_amd import augment, eval_detection, eval_metric, prepare, synth          # noqa: E402
from box2mask_amd.config import scannet_config                # noqa: E402
from box2mask_amd.model import Model                          # noqa: E402


def build_batch(seeds, voxels, mode, cfg_sup):
    items, raws = [], []
    for s in seeds:
        raw = synth.make_scene(s, target_voxels=voxels, points_only=True, pts_per_m2=8000.0)
        raw['name'] = 'synth%04d' % s
        it = prepare.voxelize_scene(raw, 0.02)
        it['scene'] = {'name': raw['name']}
        if mode == 'train':
            prepare.box_supervision(it, raw['labels'], cfg_sup)
        items.append(it); raws.append(raw)
    return prepare.collate(items, mode), raws


def augmented_batch(raws, aug_cfg, rng, cfg_sup, byte_colour=False):
    """One training batch of freshly augmented scenes: parameters per scene, labels from the augmented positions."""
    outs = augment.augment_scenes(raws, [augment.draw_params(aug_cfg, generator=rng, byte_colour=byte_colour) for _ in raws])
    items = prepare.voxelize_scenes(outs, 0.02)
    for it, out, raw in zip(items, outs, raws):
        lab = raw['labels']
        inst = lab['seg2inst'][raw['segments']]
        labels = augment.instance_labels(out, lab['per_instance_semantics'][inst], inst, lab['seg2inst'])
        it['scene'] = {'name': raw['name']}
        prepare.box_supervision(it, labels, cfg_sup)
    return prepare.collate(items, 'train')


def ground_truth_ids(raw):
    """label*1000 + instance + 1 per point for furniture, label*1000 for floor / walls."""
    lab = raw['labels']
    inst = lab['seg2inst'][raw['segments']]
    sem = lab['per_instance_semantics'][inst].astype(np.int64)
    return np.where((sem > 2) & (sem != 22), sem * 1000 + inst + 1, sem * 1000)


def evaluate(model, batch, raws):
    model.eval()
    pred = model.get_prediction(batch, with_grad=False, to_cpu=True, min_size=True)
    res = model.pred2mask(batch, pred, 'eval')
    gts = {r['name']: ground_truth_ids(r) for r in raws}
    avg, _ = eval_metric.compute_eval(res, gts)
    model.train()
    return avg


def box_labels(raw):
    """The furniture instances of a synthetic room as ARKitScenes labels: oriented boxes with the identity rotation."""
    lab = raw['labels']
    sem = lab['per_instance_semantics']
    sel = np.nonzero((sem > 2) & (sem != 22))[0]
    return {'per_instance_bb_centers': lab['per_instance_bb_centers'][sel], 'per_instance_bb_bounds': lab['per_instance_bb_bounds'][sel],
            'per_instance_bb_rotations': np.tile(np.eye(3).reshape(1, 9), (len(sel), 1)), 'per_instance_semantics': sem[sel]}


def evaluate_detection(model, batch, raws):
    model.eval()
    pred = model.get_prediction(batch, with_grad=False, to_cpu=True, min_size=True)
    res = model.pred2mask(batch, pred, 'eval')
    res = {r['name']: res[r['name']] for r in raws}
    m, ap = eval_detection.arkitscenes_eval(res, raws, [box_labels(r) for r in raws], oriented_boxes=True, iou_t=0.5, verbose=False)
    model.train()
    return m, ap


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', type=int, default=4)
    ap.add_argument('--voxels', type=int, default=20000)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--eval-every', type=int, default=50)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--half', type=int, default=0, help='1: cfg.half_training (half activations / gradients in the trunk, half_train.py)')
    ap.add_argument('--loss-scale', default='1024',
                    help="with --half 1: the constant loss scale (a power of two), or 'dynamic' -- the overflow guard of half_guard.py "
                         'skips a step whose gradients overflowed and halves the scale')
    ap.add_argument('--metric', choices=['scannet', 'arkit'], default='scannet',
                    help='arkit: the oriented-box detection mAP (eval_detection.py) beside the ScanNet AP')
    ap.add_argument('--augment', action='store_true',
                    help='train on scenes augmented on the device, parameters drawn per scene per step (augment.py)')
    ap.add_argument('--hue', action='store_true',
                    help='with --augment: apply_hue_aug too, by the byte-colour rule (training colours come out normalised)')
    ap.add_argument('--checkpoint-dir', default=None,
                    help='keep the checkpoint here (tools/param_search.py reads it); default: a temporary directory')
    args = ap.parse_args(argv)
    if args.hue and not args.augment:
        ap.error('--hue needs --augment')
    torch.manual_seed(args.seed)
    cfg = scannet_config(lr=args.lr, mlp_bb_scores_start_epoch=0, half_training=bool(args.half),       # score head trained from the first step
                         half_loss_scale='dynamic' if args.loss_scale == 'dynamic' else float(args.loss_scale))
    if args.checkpoint_dir:
        os.makedirs(args.checkpoint_dir, exist_ok=True)
    cfg.checkpoint_path = (args.checkpoint_dir.rstrip('/') if args.checkpoint_dir else tempfile.mkdtemp(prefix='b2m_ckpt_')) + '/'
    sup = SimpleNamespace(smallest_bb_heuristic=True)
    batch, raws = build_batch(range(args.scenes), args.voxels, 'train', sup)
    if args.augment:
        aug_cfg = scannet_config(augmentation=True, rotation_90_aug=True, flipping_aug=0.5, scaling_aug=[1.0, 0.8, 1.2],   # configs/scannet.txt:32-36
                                 apply_hue_aug=args.hue)                                                                    # :37
        aug_rng = np.random.default_rng(args.seed)
    model = Model(cfg, *synth.scannet_tables())
    opt = torch.optim.Adam(model.parameters(), lr=cfg.lr, fused=True)
    model.attach_optimizer(opt)                  # (--loss-scale dynamic: the optimizer skips an overflowed step; else nothing)
    model.train()
    history = []
    t0 = time.time()
    for step in range(args.steps):
        opt.zero_grad()
        losses = model.compute_loss(augmented_batch(raws, aug_cfg, aug_rng, sup, args.hue) if args.augment else batch, epoch=step)
        losses['optimization_loss'].backward()
        opt.step()
        if step % 10 == 0 or step == args.steps - 1:
            history.append((step, float(losses['optimization_loss'].detach())))
        if args.eval_every and (step % args.eval_every == 0 or step == args.steps - 1):
            avg = evaluate(model, batch, raws)
            print('step %4d  loss %.4f  AP50 %.3f  AP25 %.3f  AP %.3f  (%.1f s)'
                  % (step, float(losses['optimization_loss'].detach()), avg['all_ap_50%'], avg['all_ap_25%'], avg['all_ap'],
                     time.time() - t0), flush=True)
    if model.half_scaler is not None:
        st = model.half_scaler.stats()
        print('loss scale %g after %d steps, %d skipped (largest half gradient of the last step %g)'
              % (st['scale'], st['steps'], st['skipped'], st['max_half_grad']))
    # checkpoint in the reference's format (models/training.py:212-226) and reload through Model.load_checkpoint
    secs = float(int(time.time() - t0))          # the reference names checkpoints by the float training time
    name = 'checkpoint_{}h:{}m:{}s_{}'.format(int(secs // 3600), int((secs // 60) % 60), int(secs % 60), secs)
    torch.save({'epoch': args.steps, 'training_time': secs, 'iteration_num': args.steps,
                'model_state_dict': model.state_dict(), 'optimizer_state_dict': opt.state_dict()},
               cfg.checkpoint_path + name + '.tar')
    fresh = Model(cfg, *synth.scannet_tables())
    epoch, _, loaded, _ = fresh.load_checkpoint()
    a1, a2 = evaluate(model, batch, raws), evaluate(fresh, batch, raws)
    assert a1['all_ap_50%'] == a2['all_ap_50%'], 'a reloaded checkpoint must predict the same masks'
    print('checkpoint %s reloaded: AP50 %.3f' % (loaded, a2['all_ap_50%']))
    if args.metric == 'arkit':
        m, by_class = evaluate_detection(fresh, batch, raws)
        print('detection mAP@0.5 (oriented boxes) %.3f  over %d classes: %s'
              % (m, len(by_class), '  '.join('%d:%.3f' % (c, v) for c, v in sorted(by_class.items()))))
    return history, a2


if __name__ == '__main__':
    main()
