"""bench.py without a GPU: the options a plain run refuses, the synthetic batches made in child processes (the scenes of the
serial loop, bit for bit), and the fixed sample `--dump-outputs` writes."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


@pytest.mark.parametrize('argv', [['--steps', '0'], ['--features', 'f16'], ['--detail', '1']])
def test_plain_run_refuses(argv):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + argv, capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and 'error' in p.stderr, (p.returncode, p.stderr[-500:])


def test_parallel_scenes_are_the_serial_batches():
    from box2mask_amd import synth
    args = types.SimpleNamespace(workload='scannet', batch_size=2, target_voxels=20_000, distinct_batches=4)
    for rank, world in ((0, 1), (1, 2)):
        _, _, _, batches = bench.make_workload(args, rank, world, parallel=True)
        jitter = (1.0, 0.93, 1.07, 1.0)
        ref = [synth.make_batch(2, seed0=(j * world + rank) * 2, target_voxels=int(20_000 * jitter[j % 4])) for j in range(4)]
        assert len(batches) == len(ref)
        for b, r in zip(batches, ref):
            assert b.keys() == r.keys()
            for k in r:
                if torch.is_tensor(r[k]):
                    assert torch.equal(b[k], r[k]), k
                elif k in ('vox2point', 'seg2vox'):
                    assert all(np.array_equal(x, y) for x, y in zip(b[k], r[k])), k


def test_make_workload_is_serial_unless_asked(monkeypatch):
    """A library caller (tools/host_profile.py: no __main__ guard) gets the serial loop: no child process is started."""
    import concurrent.futures

    def refuse(*a, **k):
        raise AssertionError('a process pool was started')
    monkeypatch.setattr(concurrent.futures, 'ProcessPoolExecutor', refuse)
    args = types.SimpleNamespace(workload='scannet', batch_size=2, target_voxels=20_000, distinct_batches=1)
    _, _, _, batches = bench.make_workload(args, 0, 1)
    assert len(batches) == 1 and batches[0]['vox_coords'].shape[0] > 0


def _net():
    from box2mask_amd import synth
    from box2mask_amd.config import scannet_config
    from box2mask_amd.detection_net import SelectionNet
    cfg = scannet_config()
    valid, _, _, is_fg = synth.scannet_tables()
    torch.manual_seed(0)
    return SelectionNet(cfg, 'cpu', valid, is_fg)


def test_dump_outputs_fixed_sample(tmp_path):
    net = _net()
    losses = {'optimization_loss': torch.tensor(1.5, requires_grad=True) * 2, 'offset_loss': torch.tensor(0.25)}
    pred = {'mlp_offsets': torch.randn(300, 3), 'mlp_per_vox_semantics': torch.randn(bench.DUMP_SAMPLE + 5, 1)}
    model = types.SimpleNamespace(detection_model=net)
    bench.dump_outputs(str(tmp_path / 'a'), losses, pred, model)
    bench.dump_outputs(str(tmp_path / 'b'), losses, pred, model)
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == ['bn_stats.npy', 'loss_offset_loss.npy', 'loss_optimization_loss.npy', 'pred_mlp_offsets.npy',
                     'pred_mlp_per_vox_semantics.npy']
    total = 0
    for n in names:
        a, b = np.load(tmp_path / 'a' / n), np.load(tmp_path / 'b' / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
        total += os.path.getsize(tmp_path / 'a' / n)
    assert total <= 64 << 20
    assert float(np.load(tmp_path / 'a' / 'loss_optimization_loss.npy')) == 3.0
    assert np.array_equal(np.load(tmp_path / 'a' / 'pred_mlp_offsets.npy'), pred['mlp_offsets'].numpy())    # (small: whole)
    big = np.load(tmp_path / 'a' / 'pred_mlp_per_vox_semantics.npy')
    assert big.shape == (bench.DUMP_SAMPLE,) and np.all(np.isin(big, pred['mlp_per_vox_semantics'].numpy()))
    stats = [b for _, b in net.named_buffers() if b.is_floating_point()]
    bn = np.load(tmp_path / 'a' / 'bn_stats.npy')
    assert np.array_equal(bn, np.concatenate([b.reshape(-1).numpy() for b in stats]))


def test_restore_state_is_the_fresh_model_and_optimiser():
    """What the last timed step starts from: the seeded weights and BatchNorm statistics, and an Adam whose next step is a
    fresh Adam's first."""
    net = _net()
    model = types.SimpleNamespace(detection_model=net)
    initial = bench.initial_state(model)
    params = list(net.parameters())
    opt = torch.optim.Adam(params, lr=1e-3)
    for _ in range(2):
        for p in params:
            p.grad = torch.randn_like(p)
        opt.step()
        with torch.no_grad():
            for b in net.buffers():
                b.add_(1)
    bench.restore_state(initial, opt)
    assert all(torch.equal(t, c) for t, c in initial)
    torch.manual_seed(1)
    g = [torch.randn_like(p) for p in params]
    for p, g_ in zip(params, g):
        p.grad = g_.clone()
    opt.step()
    after = [p.detach().clone() for p in params]
    bench.restore_state(initial, opt)
    fresh = torch.optim.Adam(params, lr=1e-3)
    for p, g_ in zip(params, g):
        p.grad = g_.clone()
    fresh.step()
    assert all(torch.equal(a, p) for a, p in zip(after, params))
