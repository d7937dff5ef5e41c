"""Device time of every augmentation / label kernel (box2mask_amd/augment.py) on one synthetic scene of about 150 000 points,
beside a scipy / numpy restatement of the reference's lines on the same input on this host.

    python tools/bench_augment.py [--points 150000] [--repeats 20] [--no-cpu] [--out profiles/augment_bench.md]

HIP events around warm calls, median of the repeats.  The CPU side restates dataprocessing/augmentation.py:68-96 / :171-188
(scipy.ndimage.convolve + RegularGridInterpolator), :134-146 / :108-112 / :52-61 and dataprocessing/scannet.py:321-367; it is a
yardstick for the order of magnitude, not a parity check (tests/test_gpu_augment.py is).  One JSON line at the end.  With --out
the report is written as markdown: the header below, the table, and -- kept from the file as it was -- everything from the
KEEP marker on (the host yardsticks and the record of the --augment training run are maintained there by hand).
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

from box2mask_amd import augment, synth          # noqa: E402


KEEP = '<!-- everything below this line is kept by tools/bench_augment.py -->'
HEADER = """# Augmentation and label kernels on an MI355X (`tools/bench_augment.py`)

```
python tools/bench_augment.py --out profiles/augment_bench.md
```

HIP events around warm calls, median of the repeats; the host column is a scipy / numpy restatement of the reference's lines
on the same input on the host that ran the tool.
"""


def write_report(path, table):
    """Header + table + whatever the file held from the KEEP marker on."""
    tail = KEEP + '\n'
    if os.path.exists(path):
        old = open(path).read()
        if KEEP in old:
            tail = old[old.index(KEEP):]
    with open(path, 'w') as f:
        f.write(HEADER + '\n' + table + '\n\n' + tail)


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


def host(fn, repeats=3):
    best = 1e30
    for _ in range(repeats):
        t = time.perf_counter(); fn()
        best = min(best, time.perf_counter() - t)
    return best * 1e3


def np_elastic(coords, noise, gran, mag):
    from scipy.interpolate import RegularGridInterpolator
    from scipy.ndimage import convolve
    blurs = [np.ones(s, np.float32) / 3 for s in ((3, 1, 1, 1), (1, 3, 1, 1), (1, 1, 3, 1))]
    for _ in range(2):
        for b in blurs:
            noise = convolve(noise, b, mode='constant', cval=0)
    dims, axes, _, _, _ = augment.elastic_grid(coords.min(0), coords.max(0), gran)
    return coords + RegularGridInterpolator(axes, noise, bounds_error=0, fill_value=0)(coords) * mag


def np_boxes(pos, inst, sem):
    out = []
    for i in np.unique(inst):
        m = inst == i
        p = pos[m]
        lo, hi = p.min(0), p.max(0)
        c = (lo + hi) / 2
        d = np.linalg.norm(c - p, axis=1)
        out.append((sem[m][0], c.astype(np.float32), (hi - c).astype(np.float32), np.float32(d.max())))
    return out


def np_vertex_normals(pos, faces):
    fn = np.cross(pos[faces[:, 1]] - pos[faces[:, 0]], pos[faces[:, 2]] - pos[faces[:, 0]])
    acc = np.zeros_like(pos)
    for c in range(3):
        np.add.at(acc, faces[:, c], fn)
    return acc / np.maximum(np.linalg.norm(acc, axis=1, keepdims=True), 1e-300)


def np_hue(col, steps):
    """The numpy statement of the byte-colour chain (the rule the device pass is held to, tests/_colour8_rule.py)."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import _colour8_rule
    return _colour8_rule.colour_steps(col, steps)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=150000)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    raw = synth.make_scene(0, target_voxels=int(args.points / 2.2), points_only=True, pts_per_m2=8000.0)
    pos_h = raw['positions']
    P = len(pos_h)
    rng = np.random.default_rng(0)
    col_h = rng.random((P, 3))
    inst_h = raw['labels']['seg2inst'][raw['segments']].astype(np.int64)
    sem_h = raw['labels']['per_instance_semantics'][inst_h].astype(np.int64)
    faces_h = rng.integers(0, P, (2 * P, 3)).astype(np.int64)               # the face count of a closed mesh; random topology
    dev = torch.device('cuda')
    d = lambda a, dt=torch.float64: torch.as_tensor(a).to(dev, dt).contiguous()
    pos, nrm, col = d(pos_h), d(raw['normals']), d(col_h)
    inst, sem, faces = d(inst_h, torch.int64), d(sem_h, torch.int64), d(faces_h, torch.int64)
    rows = []
    rot = augment._rot_xyz(0.01, -0.02, 1.0)
    rows.append(['column stats (mean / min / max)', timed(lambda: augment.column_stats(pos), args.repeats),
                 None if args.no_cpu else host(lambda: (pos_h.mean(0), pos_h.min(0), pos_h.max(0), np.abs(pos_h).max(0)))])
    work = pos.clone(); wn = nrm.clone()
    rows.append(['affine about the mean, with normals', timed(lambda: augment.affine_(work, wn, rot, 'mean'), args.repeats),
                 None if args.no_cpu else host(lambda: ((pos_h - pos_h.mean(0)) @ rot.T + pos_h.mean(0), raw['normals'] @ rot.T))])
    for gran, mag in augment.SCANNET_ELASTIC_DISTORT_PARAMS:
        dims, _, lo, step, hi = augment.elastic_grid(pos_h.min(0), pos_h.max(0), gran)
        noise_h = rng.standard_normal(tuple(dims) + (3,)).astype(np.float32)
        grid = d(noise_h, torch.float32)
        tag = 'granularity %.1f, grid %dx%dx%d' % ((gran,) + tuple(dims))
        t_blur = timed(lambda: augment.blur_(grid), args.repeats)
        work = pos.clone()
        t_disp = timed(lambda: augment.displace_(work, grid, lo, step, hi, 1e-6), args.repeats)
        rows.append(['grid blur, six passes (%s)' % tag, t_blur, None])
        rows.append(['trilinear displace (%s)' % tag, t_disp, None])
        rows.append(['elastic step = blur + displace (%s)' % tag, t_blur + t_disp,
                     None if args.no_cpu else host(lambda: np_elastic(pos_h, noise_h, gran, mag), 1)])
    csr = augment.vertex_face_csr(faces, P)
    rows.append(['vertex normals from %d faces (CSR cached)' % len(faces_h), timed(lambda: augment.vertex_normals(pos, faces, csr), args.repeats),
                 None if args.no_cpu else host(lambda: np_vertex_normals(pos_h, faces_h), 1)])
    steps = [('auto_contrast', 0.4), ('translation', np.array([0.02, -0.03, 0.01])), ('jitter', -0.05, 0.05, d(rng.uniform(-0.05, 0.05, (P, 3))))]
    jit_h = steps[2][3].cpu().numpy()
    work = col.clone()

    def np_colour():
        lo_, hi_ = col_h.min(0, keepdims=True), col_h.max(0, keepdims=True)
        c = 0.6 * col_h + 0.4 * ((col_h - lo_) * (1.0 / (hi_ - lo_)))
        c = np.clip(steps[1][1] + c, 0, 1)
        return np.clip(jit_h + c, 0, 1)
    rows.append(['colour: min/max + fused contrast / translation / jitter', timed(lambda: augment.colour_(work, steps), args.repeats),
                 None if args.no_cpu else host(np_colour)])
    hue = [('brightness', 0.1), ('hue', 10.7, -12.5, 7.25, 1.1, -0.1, (5.5, -20.0, 3.3))]
    work8 = col.clone()

    def fresh_hue():                         # the chain leaves normalised colours: every repeat starts from colours in [0, 1]
        work8.copy_(col)
        augment.colour_(work8, hue)
    t_copy = timed(lambda: work8.copy_(col), args.repeats)
    rows.append(['byte colours through colour_: the host builds the tables, then brightness + hue step + Mix3D tables + normalise in one '
                 'pass (less the %.3f ms refill of its input; the device waits for the host here)' % t_copy,
                 timed(fresh_hue, args.repeats) - t_copy, None if args.no_cpu else host(lambda: np_hue(col_h, hue))])
    # the pass alone: prebuilt tables, 16 launches back to back on 16 fresh copies of the colours
    tabs = list(augment.hsv_tables(*hue[1][1:4])) + list(augment.rgb_tables(*hue[1][4:]))
    rows8 = augment.norm_rows()
    hp = [augment._hp(t) for t in tabs + list(rows8)]
    copies = [col.clone() for _ in range(16)]

    def refill():
        for c in copies:
            c.copy_(col)

    def passes():
        refill()
        for c in copies:
            augment._lib.call('b2m_aug_colour8', c.data_ptr(), P, 3, 0.1, *hp)
    t_refill = timed(refill, args.repeats)
    rows.append(['byte colours, b2m_aug_colour8 alone with prebuilt tables (16 launches back to back, per launch)',
                 (timed(passes, args.repeats) - t_refill) / 16, None])
    scene = {'positions': pos}
    t0 = timed(lambda: augment.instance_labels(scene, sem, inst, None), args.repeats)
    rows.append(['instance boxes, %d instances (whole instance_labels, two host reads)' % (int(inst_h.max()) + 1), t0,
                 None if args.no_cpu else host(lambda: np_boxes(pos_h, inst_h, sem_h), 1)])
    cfgp = augment.SceneAugment(geometric=[('affine', rot, 'mean', np.zeros(3)), ('elastic', 0.2, 0.4, 1), ('elastic', 0.8, 1.6, 2),
                                           ('affine', np.eye(3) * 1.1, 'origin', np.zeros(3))], colour=steps[:2] + [('jitter', -0.05, 0.05, 3)])
    sc = {'positions': pos, 'normals': nrm, 'colors': col, 'segments': d(raw['segments'], torch.int64)}
    t = time.perf_counter()
    for _ in range(args.repeats):
        augment.augment_scenes([sc], [cfgp])
    torch.cuda.synchronize()
    rows.append(['augment_scenes, one scene: rotation, elastic pair, scale, colour (wall clock with host reads)',
                 (time.perf_counter() - t) * 1e3 / args.repeats, None])
    lines = ['| kernel (P = %d points) | device ms | host numpy / scipy ms |' % P, '|---|---|---|']
    for name, dev_ms, cpu_ms in rows:
        lines.append('| %s | %.3f | %s |' % (name, dev_ms, '-' if cpu_ms is None else '%.1f' % cpu_ms))
    print('\n'.join(lines))
    if args.out:
        write_report(args.out, '\n'.join(lines))
    print(json.dumps({'points': P, 'rows': [{'name': n, 'device_ms': a, 'host_ms': b} for n, a, b in rows]}))


if __name__ == '__main__':
    main()
