#!/usr/bin/env python
"""Record tests/golden/loss_a_fused_bits.npz: what `b2m_detection_loss` returns, bit for bit, for case a of
tests/golden/losses.npz (230 rows, one workgroup: no free summation order) -- the 8 result floats, the four gradients and the
predicted classes.  tests/test_gpu_loss_heads.py::test_plain_entry_keeps_its_bits holds the entry to them.

The committed file was recorded on an MI355X with the library built from commit bdef3fd ("Single-scene project/NMS/gather and
half packers run the batched bodies"), the last one before `b2m_detection_loss_ex` began to share the entry's row code.  To
record it from another build, point B2M_LIB_PATH at that build's libb2m_hip.so:

    B2M_LIB_PATH=/path/to/libb2m_hip.so python tools/gen_loss_bits.py [--out FILE]

Two runs must agree before anything is written.  Needs a GPU.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'loss_a_fused_bits.npz'))
    args = ap.parse_args()
    import test_gpu_loss as T
    from test_loss_rule import golden_case
    case, _, _ = golden_case(os.path.join(ROOT, 'tests', 'golden'))
    a, b = T.run_kernel(case), T.run_kernel(case)
    out = {'values': a['values'], 'argmax': a['argmax'].numpy()}
    for h in ('off', 'bnd', 'sc', 'sem'):
        out['d_' + h] = a['grads'][h].numpy()
        assert np.array_equal(out['d_' + h], b['grads'][h].numpy()), h
    assert np.array_equal(a['values'], b['values']) and np.array_equal(out['argmax'], b['argmax'].numpy())
    np.savez(args.out, **out)
    print('wrote %s: %s' % (args.out, {k: v.shape for k, v in out.items()}))


if __name__ == '__main__':
    main()
