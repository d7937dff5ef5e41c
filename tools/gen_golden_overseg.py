"""Writes tests/golden/overseg.npz: small seeded meshes and the reference segmentator's `segIndices` for them.  Build box only (CPU).

    python tools/gen_golden_overseg.py --segmentator-src <reference>/dataprocessing/oversegmentation/cpp

Compiles segmentator.cpp + tinyply.cpp into a temporary directory OUTSIDE the repository with plain `g++ -O2 -std=c++11` (no -march: no
FMA, so every float operation rounds on its own), writes each mesh as a binary PLY there, runs the binary and keeps positions, faces,
k, m and segIndices.  Nothing of the reference is committed; the fixture holds data only.

A mesh is kept only if (a) all its weights are finite and (b) the rule's partition (tests/_overseg_rule.py) is the same under at least
8 random permutations of its tied weights -- the reference's std::sort is unstable, so only such meshes have ONE reference partition.
A mesh that fails is replaced by the next seed, never tolerated.  The rule's partition must then equal the reference's: a mismatch
stops the generator.  The number of tied weights per mesh is recorded.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _overseg_rule as R                                                      # noqa: E402
from _overseg_cases import height_field                                        # noqa: E402

CXX = ['g++', '-O2', '-std=c++11']
N_PERM = 8


def make_mesh(kind, seed):
    if kind == 'field40':
        return height_field(40, 40, seed)
    if kind == 'field30':
        return height_field(30, 30, seed)
    if kind == 'unused':                                   # vertices that no face names, in front, in the middle and at the end
        pos, faces = height_field(30, 30, seed)
        rng = np.random.default_rng(seed + 1000)
        extra = rng.normal(0, 1, (60, 3)).astype(np.float32)
        pos = np.concatenate([extra[:20], pos[:450], extra[20:40], pos[450:], extra[40:]])
        faces = faces + 20 + 20 * (faces >= 450)
        return pos, faces
    if kind == 'repeated':                                 # one face listed three times, another twice
        pos, faces = height_field(30, 30, seed)
        faces = np.concatenate([faces, faces[[7, 7, 311]]])
        return pos, faces[np.random.default_rng(seed + 2000).permutation(len(faces))]
    if kind == 'sheets':                                   # two disconnected sheets
        p0, f0 = height_field(24, 24, seed)
        p1, f1 = height_field(26, 20, seed + 1, z0=1.0, x0=0.3)
        faces = np.concatenate([f0, f1 + len(p0)])
        return np.concatenate([p0, p1]), faces[np.random.default_rng(seed + 3000).permutation(len(faces))]
    raise ValueError(kind)


CASES = [('field40', 0.01, 20)] + [('field30', k, m) for k in (0.01, 0.05, 0.5) for m in (1, 20, 50)] + [
    ('unused', 0.01, 20), ('repeated', 0.01, 20), ('sheets', 0.01, 20), ('sheets', 0.05, 50)]


def write_ply(path, pos, faces):
    with open(path, 'wb') as f:
        f.write(('ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n'
                 'element face %d\nproperty list uchar int vertex_indices\nend_header\n' % (len(pos), len(faces))).encode())
        f.write(np.asarray(pos, '<f4').tobytes())
        rec = np.zeros(len(faces), dtype=[('n', 'u1'), ('v', '<i4', 3)])
        rec['n'] = 3
        rec['v'] = faces
        f.write(rec.tobytes())


def build_segmentator(src, work):
    exe = os.path.join(work, 'segmentator')
    subprocess.check_call(CXX + [os.path.join(src, 'segmentator.cpp'), os.path.join(src, 'tinyply.cpp'), '-I', src, '-o', exe])
    return exe


def run_segmentator(exe, work, name, pos, faces, k, m):
    ply = os.path.join(work, name + '.ply')
    write_ply(ply, pos, faces)
    out = os.path.join(work, 'out')
    os.makedirs(out, exist_ok=True)
    subprocess.check_call([exe, ply, repr(float(k)), str(int(m)), out], stdout=subprocess.DEVNULL)
    files = [f for f in os.listdir(out) if f.startswith(name + '.') and f.endswith('.segs.json')]
    assert len(files) == 1, files
    with open(os.path.join(out, files[0])) as f:
        doc = json.load(f)
    os.remove(os.path.join(out, files[0]))
    return np.asarray(doc['segIndices'], np.int64)


def admissible(pos, faces, k, m):
    """(ok, ties, seg): finite weights and one partition under N_PERM permutations of the ties."""
    seg, _, w, _, _ = R.segment(pos, faces, k, m)
    if not np.isfinite(w).all():
        return False, 0, seg
    want = R.relabel(seg)
    for p in range(N_PERM):
        other = R.segment(pos, faces, k, m, rng=np.random.default_rng(77 + p))[0]
        if not np.array_equal(R.relabel(other), want):
            return False, 0, seg
    return True, R.n_ties(w), seg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--segmentator-src', required=True, help='directory of segmentator.cpp and tinyply.cpp')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'overseg.npz'))
    args = ap.parse_args()
    work = tempfile.mkdtemp(prefix='overseg_golden_')
    assert not os.path.abspath(work).startswith(ROOT + os.sep)
    try:
        exe = build_segmentator(args.segmentator_src, work)
        store, names = {}, []
        for n, (kind, k, m) in enumerate(CASES):
            seed = 100 * n
            while True:
                pos, faces = make_mesh(kind, seed)
                ok, ties, seg = admissible(pos, faces, k, m)
                if ok:
                    break
                print('%s k=%g m=%d seed %d: not admissible, next seed' % (kind, k, m, seed))
                seed += 1
            assert len(pos) <= 1600
            name = 'm%02d_%s' % (n, kind)
            ref = run_segmentator(exe, work, name, pos, faces, k, m)
            same_part = np.array_equal(R.relabel(ref), R.relabel(seg))
            print('%-14s k=%-5g m=%-3d seed=%-5d V=%d F=%d ties=%d segments=%d partition %s, ids %s'
                  % (name, k, m, seed, len(pos), len(faces), ties, len(np.unique(ref)), 'equal' if same_part else 'DIFFERENT',
                     'equal' if np.array_equal(ref, seg) else 'differ'))
            if not same_part:
                raise SystemExit('the rule and the reference disagree on the partition of an admissible mesh: ' + name)
            names.append(name)
            store[name + '.pos'] = pos
            store[name + '.faces'] = faces.astype(np.int32)
            store[name + '.seg'] = ref.astype(np.int32)
            store[name + '.params'] = np.array([k, m, ties, seed], np.float64)
        store['names'] = np.array(names)
        np.savez_compressed(args.out, **store)
        print(args.out, os.path.getsize(args.out), 'bytes')
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()
