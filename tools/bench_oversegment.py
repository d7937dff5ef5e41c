"""Device time of the mesh over-segmentation (box2mask_amd/oversegment.py, csrc/overseg.hip), stage by stage, on one seeded
height-field mesh of about 250 000 vertices and 500 000 faces -- the size of a ScanNet mesh; no real scan is used -- and on a batch of
eight such meshes.

    python tools/bench_oversegment.py [--side 500] [--repeats 5] [--batch 8]
    python tools/bench_oversegment.py --reference-only --reference-src <reference>/dataprocessing/oversegmentation/cpp

HIP events around warm calls, median of the repeats: the vertex-to-face CSR (torch sort, plumbing), weights (normals + edge weights +
keys), sort, pass one, pass two, labels.  The passes run one wave per scene, so the batch shows how far they overlap.  With
--reference-only nothing touches a GPU: the reference's segmentator is compiled into a temporary directory (g++ -O2 -std=c++11), run on
the same mesh written as a PLY file, and its wall time -- PLY parse and JSON write included -- is reported.  No pass mark.  One JSON line
at the end.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from _overseg_cases import height_field                                      # noqa: E402

STAGES = ('csr', 'weights', 'sort', 'pass_one', 'pass_two', 'labels')


def reference_wall(src, pos, faces, k, m):
    from gen_golden_overseg import build_segmentator, write_ply
    work = tempfile.mkdtemp(prefix='overseg_bench_')
    try:
        exe = build_segmentator(src, work)
        ply = os.path.join(work, 'mesh.ply')
        write_ply(ply, pos, faces)
        best = 1e30
        for _ in range(3):
            t = time.perf_counter()
            subprocess.check_call([exe, ply, repr(float(k)), str(int(m)), work], stdout=subprocess.DEVNULL)
            best = min(best, time.perf_counter() - t)
        files = [f for f in os.listdir(work) if f.endswith('.segs.json')]
        with open(os.path.join(work, files[0])) as f:
            n_seg = len(set(json.load(f)['segIndices']))
        return best * 1e3, n_seg
    finally:
        shutil.rmtree(work, ignore_errors=True)


def cpu_model():
    try:
        with open('/proc/cpuinfo') as f:
            for line in f:
                if line.startswith('model name'):
                    return line.split(':', 1)[1].strip()
    except OSError:
        pass
    return 'unknown'


def device_stages(meshes, k, m, repeats):
    import torch
    from box2mask_amd import _lib, oversegment as O
    from box2mask_amd.augment import vertex_face_csr
    dev = torch.device('cuda')
    bufs = []
    for pos, faces in meshes:
        p, f = O._to_device(pos, faces, dev)
        n_vert, n_edges = p.shape[0], 3 * f.shape[0]
        b = {'pos': p, 'faces': f, 'n_vert': n_vert, 'n_faces': f.shape[0], 'n_edges': n_edges, 'n_pad': O._pow2(n_edges),
             'normals': torch.empty((n_vert, 3), dtype=torch.float32, device=dev),
             'weights': torch.empty(n_edges, dtype=torch.float32, device=dev),
             'edge_a': torch.empty(n_edges, dtype=torch.int32, device=dev), 'edge_b': torch.empty(n_edges, dtype=torch.int32, device=dev)}
        b['keys'] = torch.empty(b['n_pad'], dtype=torch.int64, device=dev)
        b.update(O._forest(n_vert, n_edges, dev))
        b['row_ptr'], b['face_of'] = vertex_face_csr(f, n_vert)
        bufs.append(b)
    out = torch.zeros((len(bufs), 4), dtype=torch.int32, device=dev)
    desc = O._table(bufs, out, dev)
    S = len(bufs)
    mv, mp, me = max(b['n_vert'] for b in bufs), max(b['n_pad'] for b in bufs), max(b['n_edges'] for b in bufs)

    def csr():
        for b in bufs:
            vertex_face_csr(b['faces'], b['n_vert'], checked=True)
    legs = {
        'csr': csr,
        'weights': lambda: _lib.call('b2m_mesh_edge_weights', desc.data_ptr(), S, mv, mp),
        'sort': lambda: [_lib.call('b2m_sort_u64', b['keys'].data_ptr(), b['n_pad']) for b in bufs],
        'pass_one': lambda: _lib.call('b2m_graph_segment', desc.data_ptr(), S, mv, me, k, m, 1),
        'pass_two': lambda: _lib.call('b2m_graph_segment', desc.data_ptr(), S, mv, me, k, m, 2),
        'labels': lambda: _lib.call('b2m_graph_segment', desc.data_ptr(), S, mv, me, k, m, 4),
    }
    ms = {name: [] for name in STAGES}
    for rep in range(repeats + 1):                       # the stages in pipeline order, so each sees the state it meets in use
        for name in STAGES:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); legs[name](); b.record()
            b.synchronize()
            if rep:
                ms[name].append(a.elapsed_time(b))
    counts = out.cpu().tolist()
    assert not any(c[2] for c in counts), counts
    return {name: float(np.median(v)) for name, v in ms.items()}, [c[0] for c in counts]


def end_to_end(meshes, k, m, repeats):
    import torch
    from box2mask_amd import oversegment as O
    dev_meshes = [O._to_device(p, f, torch.device('cuda')) for p, f in meshes]
    wall = []
    for rep in range(repeats + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        O.segment_meshes(dev_meshes, k, m)
        torch.cuda.synchronize()
        if rep:
            wall.append((time.perf_counter() - t) * 1e3)
    return float(np.median(wall))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', type=int, default=500)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--k', type=float, default=0.01)
    ap.add_argument('--m', type=int, default=20)
    ap.add_argument('--reference-src', default=None)
    ap.add_argument('--reference-only', action='store_true')
    args = ap.parse_args()
    meshes = [height_field(args.side, args.side, 900 + s) for s in range(max(args.batch, 1))]
    pos, faces = meshes[0]
    res = {'vertices': len(pos), 'faces': len(faces), 'edges': 3 * len(faces), 'k': args.k, 'm': args.m}
    if args.reference_src:
        sys.path.insert(0, os.path.join(ROOT, 'tools'))
        wall, n_seg = reference_wall(args.reference_src, pos, faces, args.k, args.m)
        res['reference'] = {'wall_ms_with_ply_parse': wall, 'segments': n_seg, 'cpu': cpu_model()}
        print('reference binary: %.0f ms wall (PLY parse and JSON write included), %d segments, on %s' % (wall, n_seg, cpu_model()))
    if not args.reference_only:
        one, segs = device_stages(meshes[:1], args.k, args.m, args.repeats)
        res['single'] = {'stage_ms': one, 'segments': segs[0], 'end_to_end_ms': end_to_end(meshes[:1], args.k, args.m, args.repeats)}
        many, _ = device_stages(meshes[:args.batch], args.k, args.m, args.repeats)
        res['batch'] = {'scenes': args.batch, 'stage_ms': many, 'end_to_end_ms': end_to_end(meshes[:args.batch], args.k, args.m, args.repeats)}
        print('| stage | 1 mesh, device ms | %d meshes, device ms |' % args.batch)
        print('|---|---|---|')
        for name in STAGES:
            print('| %s | %.3f | %.3f |' % (name, one[name], many[name]))
        print('| segment_meshes, host wall | %.3f | %.3f |' % (res['single']['end_to_end_ms'], res['batch']['end_to_end_ms']))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
