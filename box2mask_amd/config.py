"""The ~25 configuration fields the hot path reads, with the defaults of
/root/reference/config_loader.py and the values of configs/scannet.txt.  The reference's
configargparse front end is out of scope; any object with these attributes works."""
from __future__ import annotations

from types import SimpleNamespace


def scannet_config(**overrides):
    cfg = SimpleNamespace(
        # head-name constants (config_loader.py:284-331)
        mlp_offsets='mlp_offsets', mlp_bounds='mlp_bounds', mlp_bb_scores='mlp_bb_scores',
        mlp_center_scores='mlp_center_scores', mlp_semantics='mlp_semantics',
        mlp_per_vox_semantics='mlp_per_vox_semantics',
        network_heads=['mlp_offsets', 'mlp_bounds', 'mlp_bb_scores', 'mlp_semantics'],   # configs/scannet.txt:12
        in_channels=6, layers=2, load_unused_head=False,
        do_segment_pooling=True, max_pool_segments_detection_net=False, mlp_bounds_relu=False,
        min_bb_size=0.04, multigpu=False,
        bb_supervision=True, loss_on_fg_instances=True, use_bb_iou_loss=False,
        loss_weight_bb_offsets=1.0, loss_weight_bb_bounds=0.5, loss_weight_bb_iou=1.0,
        loss_weight_bb_scores=1.0, loss_weight_center_scores=1.0, loss_weight_semantics=1.0,
        loss_weight_per_vox_semantics=1.0,
        mlp_bb_scores_start_epoch=100, mlp_center_scores_start_epoch=0,
        eval_ths=[0.5, 0.05, 0.3, 0.6],                                                    # configs/scannet.txt:15
        # threshold search (config_loader.py:133-139): np.linspace triples, read by param_search.ThresholdGrid.from_cfg
        cluster_th_search=[0.3, 0.8, 6], score_th_search=[0, 0.2, 5], mask_bin_th_search=[0.2, 0.35, 4],
        mask_nms_th_search=[0.4, 0.8, 5],
        checkpoint_path='experiments/scannet/checkpoints/', voxel_size=0.02, batch_size=8, lr=1e-3,
        half_inference=False,        # build extension (no reference field): inference on half activations, see model.Model
        half_training=False,         # build extension: training passes with the trunk's activations / gradients in half (half_train.py)
        half_loss_scale=1024.0,      # ... and the factor its gradients are scaled by inside the half region (a power of two), or
                                     # 'dynamic' (half_guard.py): a step whose gradients overflowed is skipped and halves the scale,
        half_loss_scale_init=1024.0, # which starts here
        half_growth_interval=2000,   # and doubles after this many clean steps in a row
        # augmentation (config_loader.py:189-227, read by augment.draw_params; everything off by default as in the reference --
        # configs/scannet.txt switches on augmentation, rotation_90_aug, flipping_aug 0.5, scaling_aug [1, .8, 1.2] and apply_hue_aug,
        # the last of which augment.py refuses)
        augmentation=False, rotation_aug=[0.0, 3.141592653589793 / 100, 1], rotation_90_aug=False, flipping_aug=0.0,
        HAIS_jitter_aug=False, elastic_distortion=0.0, elastic_distortion_HAIS=0.0, position_jittering=[0.0, 0.01],
        scaling_aug=[0.0, 0.9, 1.1], chromatic_auto_contrast=0.0, chromatic_translation=[0.0, 0.1],
        color_jittering_aug=[0.0, 0.1], random_brightness=[0.0, 0.1], mix_3d_color_aug=False, apply_hue_aug=False,
    )
    for k, v in overrides.items():
        setattr(cfg, k, v)
    return cfg
