"""Pin the byte-colour rule (tests/_colour8_rule.py, profiles/colour8_rule.md) to the libraries it restates, on a machine that has
them: OpenCV (`cv2`) and albumentations (1.0.3 is what the reference's environment pins).

    python tools/pin_colour8.py [--sets 48] [--seed 0]

  * rgb_to_hsv8 against cv2.cvtColor(COLOR_RGB2HSV) on all 2^24 colours, hsv_to_rgb8 against COLOR_HSV2RGB on all 180 * 256 * 256
    inputs;
  * for --sets drawn parameter sets, on a fixed image of every byte value: the hue step against
    albumentations' shift_hsv, the Mix3D tables against brightness_contrast_adjust and shift_rgb, the normalisation against
    A.Normalize with the reference's mean and std.

Prints the first mismatch of every comparison and exits 1 if there was one; exits 2 with a message when a library is missing.
No test runs this tool, and it reads nothing but this repository."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def first_mismatch(tag, got, want, inputs):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        print('%s: shape / dtype %s %s against %s %s' % (tag, got.shape, got.dtype, want.shape, want.dtype))
        return 1
    bad = np.nonzero((got != want).reshape(len(got), -1).any(1))[0]
    if len(bad):
        k = bad[0]
        print('%s: %d of %d differ; first at %d: input %s, rule %s, library %s' % (tag, len(bad), len(got), k, inputs[k], got[k], want[k]))
        return 1
    print('%s: equal on %d inputs' % (tag, len(got)))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--sets', type=int, default=48)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args(argv)
    try:
        import cv2
        import albumentations as A
        import albumentations.augmentations.functional as F
    except ImportError as e:
        print('pin_colour8 needs cv2 and albumentations, which this machine does not have (%s): the rule stays unpinned' % e)
        return 2
    import _colour8_rule as R
    print('cv2 %s, albumentations %s' % (cv2.__version__, A.__version__))
    fails = 0
    k = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([k >> 16, (k >> 8) & 255, k & 255], -1).astype(np.uint8)
    fails += first_mismatch('RGB->HSV', R.rgb_to_hsv8(rgb), cv2.cvtColor(rgb[None], cv2.COLOR_RGB2HSV)[0], rgb)
    k = np.arange(180 * 256 * 256, dtype=np.uint32)
    hsv = np.stack([k >> 16, (k >> 8) & 255, k & 255], -1).astype(np.uint8)
    fails += first_mismatch('HSV->RGB', R.hsv_to_rgb8(hsv), cv2.cvtColor(hsv[None], cv2.COLOR_HSV2RGB)[0], hsv)
    rng = np.random.default_rng(args.seed)
    img = rng.integers(0, 256, (64, 1024, 3)).astype(np.uint8)
    img[0, :256] = np.arange(256, dtype=np.uint8)[:, None]
    flat = img.reshape(-1, 3)
    norm = A.Normalize(mean=R.COLOR_MEAN, std=R.COLOR_STD)
    fails += first_mismatch('Normalize', R.normalise(flat), norm(image=img)['image'].reshape(-1, 3), flat)
    for i in range(args.sets):
        edge = i % 6 == 0                                      # every sixth set sits on the limits, zeros and near-zeros included
        pick = lambda lim: float(rng.choice([-lim, lim, 0.0, 1e-9, -1e-9])) if edge else float(rng.uniform(-lim, lim))
        h, s, v = pick(50), pick(60), pick(50)
        alpha, beta = 1.0 + pick(0.2), pick(0.2)
        shifts = (pick(20), pick(20), pick(20))
        tag = 'set %d (%r)' % (i, (h, s, v, alpha, beta, shifts))
        fails += first_mismatch(tag + ' shift_hsv', R.hue_step(flat, h, s, v), F.shift_hsv(img, h, s, v).reshape(-1, 3), flat)
        bc = F.brightness_contrast_adjust(img, alpha, beta, beta_by_max=True)
        want = F.shift_rgb(bc, *shifts).reshape(-1, 3)
        fails += first_mismatch(tag + ' Mix3D tables', R.apply_rgb_tables(flat, R.rgb_tables(alpha, beta, shifts)), want, flat)
    print('pinned' if not fails else '%d comparisons differ: the rule is NOT what these libraries compute' % fails)
    return 1 if fails else 0


if __name__ == '__main__':
    sys.exit(main())
