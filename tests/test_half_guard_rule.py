"""The overflow guard of half training (box2mask_amd/half_guard.py, csrc/guard.hip) without a GPU:

  1. the rule (tests/_guard_rule.py) on its named cases, and every deliberate mistake failing the case that exists for it -- a
     rule that forgave one of them could not hold a kernel to anything;
  2. the scale policy (half_guard.update_scale) against torch's `_amp_update_scale_` on CPU tensors over seeded random flag
     sequences, and against the written rule where the clamps to [1, 65536] bind (torch's operator has none);
  3. the three entries refuse bad arguments on the host, before anything touches a device."""
import numpy as np
import pytest
import torch

import _guard_rule as R
from box2mask_amd import _lib, half_guard as G


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_rule_on_named_cases(name):
    args, want, _ = R.CASES[name]
    assert R.half_absmax(**args) == want


@pytest.mark.parametrize('mistake', [m for m in R.MISTAKES if m != 'gt_at_threshold'])
def test_every_mistake_fails_its_case(mistake):
    hit = [n for n, (args, want, m) in R.CASES.items() if m == mistake]
    assert hit, 'no case for ' + mistake
    for n in hit:
        args, want, _ = R.CASES[n]
        assert R.half_absmax(mistake=mistake, **args) != want, (mistake, n)
    # and the fp32 form of the same mistake, on the fp32 twin of the case
    buf = np.full(16, 0x3f800000, np.uint32)
    cases = {'sign_not_masked': (dict(buf=np.array([0xff800000, 1, 2, 3], np.uint32), off=0, n=4, prev=0), R.F_INF),
             'tail_dropped': (dict(buf=np.array([1, 2, 3, 4, R.F_INF], np.uint32), off=0, n=5, prev=0), R.F_INF),
             'nan_below_inf': (dict(buf=np.array([R.F_NAN, 2, 3, 4], np.uint32), off=0, n=4, prev=R.F_INF), R.F_NAN),
             'out_overwritten': (dict(buf=buf, off=0, n=16, prev=R.F_INF), R.F_INF),
             'padding_read': (dict(buf=np.array([R.F_NAN, 5, 6, R.F_NAN], np.uint32), off=1, n=2, prev=0), 6)}
    args, want = cases[mistake]
    assert R.f32_absmax(**args) == want
    if mistake != 'padding_read':            # (an fp32 array has no padding: the case pins the offset / length instead)
        assert R.f32_absmax(mistake=mistake, **args) != want


@pytest.mark.parametrize('name', sorted(R.FINISH_CASES))
def test_finish_rule_and_the_threshold_mistake(name):
    flags, want, mistake = R.FINISH_CASES[name]
    found, counters = R.finish(flags, (7, 2))
    assert found == want and counters == (8, 2 + int(want))
    assert G.found(*flags) == bool(want)                    # the host's copy of the rule
    if mistake is not None:
        assert R.finish(flags, (7, 2), mistake=mistake)[0] != want


def test_bit_order_is_magnitude_order():
    """finite < 65504 < inf < NaN, as unsigned integers of the masked bits -- for every binary16 value."""
    bits = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    mag = bits & 0x7fff
    val = np.abs(bits.view(np.float16).astype(np.float64))
    finite = np.isfinite(val)
    order = np.argsort(mag[finite], kind='stable')
    assert np.all(np.diff(val[finite][order]) >= 0)
    assert mag[finite].max() == R.H_MAXF and float(np.uint16(R.H_MAXF).view(np.float16)) == 65504.0
    assert np.all(mag[np.isinf(val)] == R.H_INF) and np.all(mag[np.isnan(val)] > R.H_INF)


@pytest.mark.parametrize('p_found', [0.03, 0.3, 0.6, 0.95])
def test_policy_against_torch_amp_update_scale(p_found):
    """50 steps, growth interval 3, from 1024: every step against torch._amp_update_scale_ applied to the state of the step before;
    where a clamp binds (torch has none) against the written rule: the scale stays at the bound, the tracker moves as without it."""
    have_op = hasattr(torch, '_amp_update_scale_')          # (absent: the written rule alone is checked)
    bound_hit = {1.0: 0, 65536.0: 0}
    for seed in range(8):
        rng = np.random.default_rng(1000 * seed + int(100 * p_found))
        flags = rng.random(50) < p_found
        scale, tracker = 1024.0, 0
        for f in flags:
            new_scale, new_tracker = G.update_scale(scale, tracker, bool(f), 2.0, 0.5, 3, 1.0, 65536.0)
            # the written rule
            if f:
                want_s, want_t = scale * 0.5, 0
            elif tracker + 1 == 3:
                want_s, want_t = scale * 2.0, 0
            else:
                want_s, want_t = scale, tracker + 1
            if have_op:
                s, t = torch.tensor([scale], dtype=torch.float32), torch.tensor([tracker], dtype=torch.int32)
                torch._amp_update_scale_(s, t, torch.tensor([1.0 if f else 0.0]), 2.0, 0.5, 3)
                assert (float(s), int(t)) == (want_s, want_t)
            clamped = min(max(want_s, 1.0), 65536.0)
            if clamped != want_s:
                bound_hit[clamped] += 1
            assert (new_scale, new_tracker) == (clamped, want_t), (seed, scale, tracker, f)
            m, _ = np.frexp(new_scale)
            assert m == 0.5                                  # a power of two: scaling and un-scaling stay exact
            scale, tracker = new_scale, new_tracker
    if p_found >= 0.6:
        assert bound_hit[1.0] > 0
    if p_found <= 0.03:
        assert bound_hit[65536.0] > 0


def test_entries_refuse_bad_arguments_on_the_host():
    """NULL pointers, negative sizes, ld < c, a size beyond the kernel's 32-bit indices, misaligned words: a negative return and a
    message, no launch (the convention tests/test_abi.py checks for the entries of round 6).  The addresses are never touched."""
    lib = _lib.load()
    err = lambda: lib.b2m_last_error().decode()
    X, OUT = 1 << 20, 1 << 21
    assert lib.b2m_half_absmax(X, 96, 10, 96, None, None) < 0 and 'out' in err()
    assert lib.b2m_half_absmax(None, 96, 10, 96, OUT, None) < 0 and 'x is NULL' in err()
    assert lib.b2m_half_absmax(X, 96, -1, 96, OUT, None) < 0 and 'negative' in err()
    assert lib.b2m_half_absmax(X, 96, 10, -1, OUT, None) < 0 and 'negative' in err()
    assert lib.b2m_half_absmax(X, 95, 10, 96, OUT, None) < 0 and 'ld < c' in err()
    assert lib.b2m_half_absmax(X, 96, (1 << 31) // 96 + 1, 96, OUT, None) < 0 and '32-bit' in err()
    assert lib.b2m_half_absmax(X, 1 << 31, 1, 96, OUT, None) < 0 and '32-bit' in err()
    assert lib.b2m_half_absmax(X + 1, 96, 10, 96, OUT, None) < 0 and 'aligned' in err()
    assert lib.b2m_half_absmax(X, 96, 10, 96, OUT + 2, None) < 0 and 'aligned' in err()
    assert lib.b2m_half_absmax(None, 96, 0, 96, OUT, None) == 0              # no rows: nothing to launch, no device needed
    assert lib.b2m_f32_absmax(X, 10, None, None) < 0 and 'out' in err()
    assert lib.b2m_f32_absmax(None, 10, OUT, None) < 0 and 'g is NULL' in err()
    assert lib.b2m_f32_absmax(X, -1, OUT, None) < 0 and 'negative' in err()
    assert lib.b2m_f32_absmax(X + 2, 10, OUT, None) < 0 and 'aligned' in err()
    assert lib.b2m_f32_absmax(None, 0, OUT, None) == 0
    assert lib.b2m_guard_finish(None, X, OUT, None) < 0 and 'flags' in err()
    assert lib.b2m_guard_finish(X, None, OUT, None) < 0 and 'found_inf' in err()
    assert lib.b2m_guard_finish(X, OUT, None, None) < 0 and 'counters' in err()
    assert lib.b2m_guard_finish(X, OUT + 1, OUT, None) < 0 and 'aligned' in err()


def test_scaler_refuses_a_scale_that_is_no_power_of_two_and_an_unfused_optimizer():
    """(host only: the constructor's checks run before it allocates anything on a device)"""
    with pytest.raises(ValueError):
        G.HalfScaler(init_scale=1000.0, device='cpu')
    with pytest.raises(ValueError):
        G.HalfScaler(init_scale=2.0 ** 17, device='cpu')
    s = G.HalfScaler(init_scale=512.0, growth_interval=3, device='cpu')
    assert s.state_dict() == {'scale': 512.0, 'growth_tracker': 0, 'steps': 0, 'skipped': 0}
    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(TypeError, match='fused'):
        s.attach(torch.optim.Adam([p], lr=1e-3))
    with pytest.raises(TypeError, match='fused'):
        s.attach(torch.optim.SGD([p], lr=1e-3))
