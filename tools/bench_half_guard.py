"""What dynamic loss scaling (cfg.half_loss_scale = 'dynamic', box2mask_amd/half_guard.py) costs per half training step, against the
constant scale 1024 in the SAME process: the two modes alternate round by round on one model and one batch, every step is timed
with a pair of HIP events, and the guard's own launches are bracketed with events in one extra step per round.

    python tools/bench_half_guard.py            (ROUNDS=5 STEPS=10 WORKLOADS=scannet,arkit)

Prints per workload: ms per step of each mode (median over all timed steps, and per round), the guard kernels' ms and launch
count per step, and the host's wait at the flag event per step.  A figure to report (profiles/half_guard.md), not a gate."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from box2mask_amd import synth, _lib
from box2mask_amd.config import scannet_config
from box2mask_amd.model import Model

ROUNDS = int(os.environ.get('ROUNDS', '5'))
STEPS = int(os.environ.get('STEPS', '10'))
GUARD = ('b2m_half_absmax', 'b2m_f32_absmax', 'b2m_guard_finish')


def make_batch(workload):
    if workload == 'scannet':                    # BASELINE configs[1]: 8 scenes of ~150 k voxels at 2 cm
        batch = synth.make_batch(8, seed0=0, target_voxels=int(os.environ.get('TV', '150000')))
    else:                                        # configs[5]: 4 scenes of 30 - 200 k voxels at 4 cm
        batch = synth.collate([synth.make_scene(10 + i, target_voxels=tv, voxel_size=0.04, pts_per_m2=5000.0)
                               for i, tv in enumerate((30_000, 200_000, 80_000, 120_000))])
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}


def main():
    for workload in os.environ.get('WORKLOADS', 'scannet,arkit').split(','):
        torch.manual_seed(0)
        cfg = scannet_config(half_training=True, half_loss_scale='dynamic')
        model = Model(cfg, *synth.scannet_tables())
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True)
        batch = make_batch(workload)
        model.train()
        scaler = model.half_scaler

        def set_mode(mode):
            scaler.detach(opt)
            cfg.half_loss_scale = 'dynamic' if mode == 'dynamic' else 1024.0
            if mode == 'dynamic':
                scaler.attach(opt)

        def step():
            opt.zero_grad()
            model.compute_loss(batch, 150)['optimization_loss'].backward()
            opt.step()

        times = {'static': [], 'dynamic': []}
        per_round = {'static': [], 'dynamic': []}
        wait, guard_ms, guard_n = [], [], []
        for rnd in range(ROUNDS):
            for mode in ('static', 'dynamic') if rnd % 2 == 0 else ('dynamic', 'static'):
                set_mode(mode)
                for _ in range(3):
                    step()
                torch.cuda.synchronize()
                w0 = scaler.wait_s
                evs = []
                for _ in range(STEPS):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(); step(); b.record()
                    evs.append((a, b))
                torch.cuda.synchronize()
                ms = [a.elapsed_time(b) for a, b in evs]
                times[mode] += ms
                per_round[mode].append(statistics.median(ms))
                if mode == 'dynamic':
                    wait.append((scaler.wait_s - w0) / STEPS * 1e3)
                    # one more step with the guard's launches bracketed (the brackets serialise: not part of the timing above)
                    marks = []

                    def hook(name, args, meta=None):
                        if name not in GUARD:
                            return None
                        a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
                        a.record()
                        marks.append((a, b))
                        return b.record
                    _lib.set_hook(hook)
                    try:
                        step()
                    finally:
                        _lib.set_hook(None)
                    torch.cuda.synchronize()
                    guard_ms.append(sum(a.elapsed_time(b) for a, b in marks))
                    guard_n.append(len(marks))
        med = {m: statistics.median(v) for m, v in times.items()}
        st = scaler.stats()
        print('%s (%d rows): static %.2f ms/step, dynamic %.2f ms/step (+%.2f ms, %+.1f %%); per round static %s dynamic %s'
              % (workload, batch['vox_coords'].shape[0], med['static'], med['dynamic'], med['dynamic'] - med['static'],
                 100.0 * (med['dynamic'] / med['static'] - 1.0), ' '.join('%.2f' % t for t in per_round['static']),
                 ' '.join('%.2f' % t for t in per_round['dynamic'])), flush=True)
        print('  guard kernels: %d launches, %.3f ms per step (bracketed one by one); host wait at the flag event %.3f ms per step; '
              'scale %g, %d steps, %d skipped, largest half gradient %g'
              % (statistics.median(guard_n), statistics.median(guard_ms), statistics.median(wait), st['scale'], st['steps'], st['skipped'],
                 st['max_half_grad']), flush=True)
        del model, opt, batch
        torch.cuda.empty_cache()


if __name__ == '__main__':
    t0 = time.time()
    main()
    print('%.0f s' % (time.time() - t0))
