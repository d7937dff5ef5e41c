"""The overflow guard's rule (include/b2m.h: b2m_half_absmax, b2m_f32_absmax, b2m_guard_finish) in numpy, the deliberate mistakes
a kernel could make, and the named cases that catch each of them.  tests/test_half_guard_rule.py (CPU) holds the rule to the cases;
tests/test_gpu_half_guard.py holds the kernels to the rule.

Magnitude bits order as unsigned integers: finite < 65504 (0x7bff) < inf (0x7c00) < every NaN."""
import numpy as np

H_MAXF, H_INF, H_NAN = 0x7bff, 0x7c00, 0x7e00
F_MAXF, F_INF, F_NAN = 0x7f7fffff, 0x7f800000, 0x7fc00000
PAD = 0x7fff                      # what the tests fill padding columns (and everything around the matrix) with

MISTAKES = ('sign_not_masked', 'padding_read', 'tail_dropped', 'gt_at_threshold', 'nan_below_inf', 'out_overwritten')


def half_absmax(buf, off, ld, n, c, prev, mistake=None):
    """max(prev, max over rows r < n, columns k < c of buf[off + r * ld + k] & 0x7fff); buf: uint16."""
    assert buf.dtype == np.uint16 and ld >= c
    cols = ld if mistake == 'padding_read' else c
    if mistake == 'tail_dropped':
        cols = c - c % 8
    idx = off + np.arange(n, dtype=np.int64)[:, None] * ld + np.arange(cols, dtype=np.int64)[None, :]
    v = buf[idx].astype(np.uint32)
    if mistake != 'sign_not_masked':
        v = v & 0x7fff
    if mistake == 'nan_below_inf':           # (a maximum taken on the VALUES, which drops NaN)
        v = np.where((v & 0x7fff) > H_INF, 0, v)
    m = int(v.max()) if v.size else 0
    return m if mistake == 'out_overwritten' else max(int(prev), m)


def f32_absmax(buf, off, n, prev, mistake=None):
    """max(prev, max over i < n of buf[off + i] & 0x7fffffff); buf: uint32."""
    assert buf.dtype == np.uint32
    cnt = n - n % 4 if mistake == 'tail_dropped' else n
    v = buf[off:off + cnt].astype(np.uint64)
    if mistake != 'sign_not_masked':
        v = v & 0x7fffffff
    if mistake == 'nan_below_inf':
        v = np.where((v & 0x7fffffff) > F_INF, 0, v)
    m = int(v.max()) if v.size else 0
    return m if mistake == 'out_overwritten' else max(int(prev), m)


def finish(flags, counters, mistake=None):
    """(found_inf as a float, counters after): found = flags[0] >= 0x7bff or flags[1] >= 0x7f800000."""
    if mistake == 'gt_at_threshold':
        hit = flags[0] > H_MAXF or flags[1] > F_INF
    else:
        hit = flags[0] >= H_MAXF or flags[1] >= F_INF
    return (1.0 if hit else 0.0), (counters[0] + 1, counters[1] + (1 if hit else 0))


def half_matrix(n, c, ld, off, seed=0, zeros=False):
    """A uint16 buffer holding an n x c matrix of finite values below 1.0 (magnitude bits in [1, 0x3bff], random signs; or +0
    everywhere) at element offset `off` with pitch ld; the padding columns, the elements in front and 16 behind hold PAD
    (0x7fff, a NaN larger than anything a test plants)."""
    rng = np.random.default_rng(seed)
    buf = np.full(off + n * ld + 16, PAD, np.uint16)
    if n and c:
        idx = off + np.arange(n)[:, None] * ld + np.arange(c)[None, :]
        buf[idx] = 0 if zeros else (rng.integers(1, 0x3c00, (n, c)) | (rng.integers(0, 2, (n, c)) << 15)).astype(np.uint16)
    return buf


def positions(n, c):
    """Where the tests plant a value: first element, last element, last of a row, first of the last row."""
    return {'first': (0, 0), 'last': (n - 1, c - 1), 'row_end': (0, c - 1), 'last_row_start': (n - 1, 0)}


def _case(n, c, ld, off, plant, prev, where='last'):
    buf = half_matrix(n, c, ld, off, seed=n * 131 + c)
    r, k = positions(n, c)[where]
    buf[off + r * ld + k] = plant
    return dict(buf=buf, off=off, ld=ld, n=n, c=c, prev=prev)


# name -> (arguments of half_absmax, the answer, the mistake the case exists for)
CASES = {
    # -inf in a matrix of small values: with the sign bit left in, 0xfc00 would come out
    'negative_inf_is_inf': (_case(5, 9, 9, 0, 0xfc00, 0, 'first'), H_INF, 'sign_not_masked'),
    # nothing above 1.0 inside the matrix; the padding columns hold 0x7fff
    'padding_is_not_data': (_case(5, 9, 12, 1, 0x3c00, 0, 'first'), 0x3c00, 'padding_read'),
    # the only large value sits in the last column of a row of 9 = 8 + 1
    'value_in_the_tail': (_case(5, 9, 10, 0, H_MAXF, 0, 'last'), H_MAXF, 'tail_dropped'),
    # a NaN and an inf: the NaN's bits are the larger
    'nan_above_inf': (_case(3, 8, 8, 0, H_NAN, H_INF, 'row_end'), H_NAN, 'nan_below_inf'),
    # *out holds inf from an earlier tensor of the step; this tensor is clean
    'earlier_maximum_survives': (_case(4, 8, 8, 0, 0x3c00, H_INF, 'first'), H_INF, 'out_overwritten'),
}
# (flags, found): exactly 65504 is what the convolution's epilogue clamps to -- it counts
FINISH_CASES = {
    'clipped_value_counts': ((H_MAXF, 0), 1.0, 'gt_at_threshold'),
    'below_both': ((H_MAXF - 1, F_INF - 1), 0.0, None),
    'f32_inf': ((0, F_INF), 1.0, 'gt_at_threshold'),
    'half_inf': ((H_INF, 0), 1.0, None),
    'both': ((H_NAN, F_NAN), 1.0, None),
}
