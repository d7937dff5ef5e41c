"""Two plain `bench.py` runs of the headline command: the headline line and nothing else, `--steps` timed steps, and
`--dump-outputs` writing what the last of them computed -- the same every run, to rounding (the last timed step starts from
the seeded initial state)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                        '--dump-outputs', str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_runs_dump_the_same_last_step(tmp_path):
    runs = [_run(tmp_path / ('out%d' % i)) for i in range(2)]
    for d in runs:
        assert d['unit'] == 'scenes/s' and d['higher_is_better'] is True and d['dtype'] == 'f32'
        assert d['steps'] == 3 and d['config']['steps_executed'] == d['config']['setup_steps'] + 1 + 3
        assert abs(d['value'] - 8 * 3 / (d['ms_per_step'] * 3 / 1e3)) < 0.02 * d['value']
        # the figures of --full are not measured
        for k in ('roofline', 'roofline_timed_region', 'value_incl_h2d', 'votes_to_masks', 'inference', 'prepare', 'cpu_baseline'):
            assert k not in d, k
    names = sorted(os.listdir(tmp_path / 'out0'))
    assert names == sorted(os.listdir(tmp_path / 'out1'))
    assert {'loss_optimization_loss.npy', 'bn_stats.npy', 'pred_mlp_offsets.npy', 'pred_mlp_semantics.npy'} <= set(names)
    assert round(float(np.load(tmp_path / 'out0' / 'loss_optimization_loss.npy')), 4) == runs[0]['config']['final_loss']
    for n in names:
        a, b = np.load(tmp_path / 'out0' / n), np.load(tmp_path / 'out1' / n)
        assert a.dtype in (np.float32, np.float64) and a.shape == b.shape and np.all(np.isfinite(a)), n
        scale = max(float(np.abs(a).max()), 1e-30)
        assert float(np.abs(a.astype(np.float64) - b).max()) <= 1e-4 * scale, n       # rounding, not a different trajectory
