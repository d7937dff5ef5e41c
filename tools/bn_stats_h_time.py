"""Time b2m_bn_stats_finalize_h (the statistics of a binary16 BatchNorm input read from HBM) with HIP events at the shapes of the
half region: about 1.2 M rows x 32 channels (tensor stride 1) and 290 k rows x 96 (stride 2).

    python tools/bn_stats_h_time.py                # one JSON line: median / min / max microseconds per call and shape, over chunks
                                                    # of 100 back-to-back calls that rotate over 640 MB of inputs
    B2M_LIB_PATH=/path/to/another/libb2m_hip.so python tools/bn_stats_h_time.py

For an A/B of two builds run the two alternating, several times each, in one session (profiles/bn_stats_fp64.md)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from box2mask_amd import _lib  # noqa: E402

SHAPES = ((1200000, 32), (290000, 96))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chunks', type=int, default=40)
    ap.add_argument('--per-chunk', type=int, default=100)
    ap.add_argument('--rotate-mb', type=int, default=640, help='the launches walk over copies of x worth this much: past every cache')
    a = ap.parse_args()
    out = {'lib': os.path.abspath(_lib.LIB_PATH)}           # the full path: the two builds of an A/B usually share a file name
    for n, c in SHAPES:
        g = torch.Generator(device='cuda').manual_seed(n + c)
        x0 = (torch.randn(n, c, device='cuda', generator=g) * 1.5 + 0.3).half()
        xs = [x0] + [x0.clone() for _ in range(max(a.rotate_mb * 2 ** 20 // (2 * n * c), 1))]
        f32 = lambda v: torch.full((c,), v, device='cuda')
        gam, bet, rm, rv, mean, inv, sc, sh = f32(1.0), f32(0.0), f32(0.0), f32(1.0), f32(0.0), f32(0.0), f32(0.0), f32(0.0)
        partial = torch.empty(2 * c * 4096, dtype=torch.float64, device='cuda')
        run = lambda x: _lib.call('b2m_bn_stats_finalize_h', x.data_ptr(), c, n, c, partial.data_ptr(), gam.data_ptr(), bet.data_ptr(), 1e-5,
                                  0.1, rm.data_ptr(), rv.data_ptr(), mean.data_ptr(), inv.data_ptr(), sc.data_ptr(), sh.data_ptr())
        for i in range(a.per_chunk):
            run(xs[i % len(xs)])
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.chunks)]
        k = 0
        for s, e in ev:
            s.record()
            for _ in range(a.per_chunk):
                run(xs[k % len(xs)])
                k += 1
            e.record()
        torch.cuda.synchronize()
        t = np.array([s.elapsed_time(e) for s, e in ev]) * 1e3 / a.per_chunk          # microseconds per call (two launches)
        ref = x0.double().mean(0)
        assert float((mean.double() - ref).abs().max()) < 1e-5
        med = float(np.median(t))
        out['%dx%d' % (n, c)] = {'median_us': round(med, 2), 'min_us': round(float(t.min()), 2), 'max_us': round(float(t.max()), 2),
                                 'gb_per_s': round(2.0 * n * c / med * 1e-3, 1), 'calls': a.chunks * a.per_chunk, 'buffers': len(xs)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
