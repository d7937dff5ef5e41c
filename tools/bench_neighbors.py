"""Device time of the nearest-neighbour index (box2mask_amd/neighbors.py, csrc/neighbors.hip) on one synthetic room of about
1 000 000 points, beside scipy's cKDTree and sklearn's ball tree on the same input on this host.

    python tools/bench_neighbors.py [--points 1000000] [--repeats 10] [--no-cpu] [--out profiles/neighbors_bench.md]

HIP events around warm calls, median of the repeats.  Three legs: the build over the room; a query of the full-resolution kind
(as many queries as points: the room's points moved by up to 2 cm, as an unsampled room looks from its every-fourth-point
sample); and the label transfer's kind, the room's points queried in consecutive batches of 250 000 (annotation clouds).  The
host trees are a yardstick for the order of magnitude, not a parity check (tests/test_gpu_neighbors.py is).  There is no pass
mark.  One JSON line at the end; with --out the table is written as markdown.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from box2mask_amd.neighbors import NearestIndex          # noqa: E402

HEADER = """# Nearest-neighbour index on an MI355X (`tools/bench_neighbors.py`)

```
python tools/bench_neighbors.py --out profiles/neighbors_bench.md
```

HIP events around warm calls, median of the repeats; the host columns are scipy's `cKDTree` and sklearn's ball tree on the same
input on the host that ran the tool (one run each).  No pass mark.
"""


def room(n, rng):
    """Points on the six faces of an 8 x 6 x 3 m room and on forty boxes inside it (surfaces, as a scan gives them), float64."""
    ext = np.array([8.0, 6.0, 3.0])
    p = rng.uniform(0, 1, (n, 3)) * ext
    axis = rng.integers(0, 3, n)
    side = rng.integers(0, 2, n)
    half = n // 2
    p[np.arange(half), axis[:half]] = side[:half] * ext[axis[:half]]          # half of the points on the room's faces
    centre = rng.uniform(0.5, 1, (40, 3)) * (ext - 1.0)
    size = rng.uniform(0.2, 0.6, (40, 3))
    b = rng.integers(0, 40, n - half)
    q = centre[b] + rng.uniform(-1, 1, (n - half, 3)) * size[b]
    rows = np.arange(n - half)
    q[rows, axis[half:]] = centre[b, axis[half:]] + (2 * side[half:] - 1) * size[b, axis[half:]]
    p[half:] = q
    return p


def timed(fn, repeats):
    fn(); fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def host(fn, repeats=1):
    best = 1e30
    for _ in range(repeats):
        t = time.perf_counter(); fn()
        best = min(best, time.perf_counter() - t)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=1000000)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    n = args.points
    ref = room(n, rng)
    full = ref + rng.uniform(-0.02, 0.02, (n, 3))
    batch = min(250000, n)
    r, f = torch.from_numpy(ref).cuda(), torch.from_numpy(full).cuda()
    index = NearestIndex(r)
    legs = {}
    legs['build'] = timed(lambda: NearestIndex(r), args.repeats)
    legs['query_full'] = timed(lambda: index.query(f, return_distance=True), args.repeats)
    legs['query_batches'] = timed(lambda: [index.query(r[s:s + batch], return_distance=True) for s in range(0, n, batch)], args.repeats)
    cpu = {}
    if not args.no_cpu:
        from scipy.spatial import cKDTree
        from sklearn.neighbors import NearestNeighbors
        for name, build, query in (
                ('ckdtree', lambda: cKDTree(ref), lambda t, q: t.query(q, k=1)),
                ('ball_tree', lambda: NearestNeighbors(n_neighbors=1, algorithm='ball_tree').fit(ref), lambda t, q: t.kneighbors(q))):
            tree = build()
            cpu[name] = {'build': host(build), 'query_full': host(lambda: query(tree, full)),
                         'query_batches': host(lambda: [query(tree, ref[s:s + batch]) for s in range(0, n, batch)])}
    what = {'build': 'build over %d points' % n, 'query_full': '%d queries within 2 cm of the points' % n,
            'query_batches': 'the points themselves in batches of %d' % batch}
    lines = ['| leg | device ms | cKDTree ms | ball tree ms |', '|---|---|---|---|']
    for k in ('build', 'query_full', 'query_batches'):
        lines.append('| %s | %.3f | %s | %s |' % (what[k], legs[k], *('%.0f' % cpu[t][k] if t in cpu else '-' for t in ('ckdtree', 'ball_tree'))))
    table = '\n'.join(lines)
    print(table)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(HEADER + '\n' + table + '\n')
    print(json.dumps({'points': n, 'device_ms': legs, 'host_ms': cpu}))


if __name__ == '__main__':
    main()
