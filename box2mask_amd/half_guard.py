"""Dynamic loss scaling for half-precision training (half_train.py): a device-side overflow guard and the scale policy of
`torch.amp.GradScaler`.  Opt-in: `cfg.half_loss_scale = 'dynamic'`; with a float nothing here runs.

What can go wrong inside the loss-scaled half region, and in which form it is left behind:

* `_ToFloat.backward` casts `g * scale` to half, `b2m_bn_bwd_apply_h` rounds its result to half: +-inf from 65520 on;
* the data-gradient launches of `b2m_conv_fwd_h` CLAMP on their way out (+-65504, and a NaN becomes finite there too): a gradient
  that blew up reaches the fp32 weight gradients as a finite, wrong number.

The guard only observes.  `b2m_half_absmax` folds the magnitude BITS of every half gradient tensor the region produces into one
word, right behind the launch that produced it and on its stream; bits order as unsigned integers, finite < 65504 (0x7bff) < inf
(0x7c00) < NaN, so `word >= 0x7bff` says "clipped or not finite".  `b2m_f32_absmax` does the same once per step over the flat
gradient buffer (grad_arena.py), `b2m_guard_finish` turns the two words into the `found_inf` tensor torch's fused optimizers
take: with it set they leave parameters, moments and step counts alone, on the device, without a host read.

The scale of pass t is the policy applied to the flags of the steps before it, in order: halve after a step that found
something, double after `growth_interval` clean steps in a row, clamped to [1, 65536] -- powers of two throughout, so scaling and
un-scaling stay exact.  The host learns the flags through an asynchronous copy to pinned memory and waits for it no earlier than
the first backward operator of the next pass's half region: the forward pass of that step is queued by then."""
from __future__ import annotations

import collections
import time

import numpy as np
import torch

from . import _lib

HALF_FOUND = 0x7bff            # 65504: what the convolution's epilogue clamps to -- at or above it the step counts as overflowed
F32_FOUND = 0x7f800000         # inf


def found(half_bits: int, f32_bits: int) -> bool:
    """The rule of b2m_guard_finish, for the host's copy of the flags."""
    return (half_bits & 0xffffffff) >= HALF_FOUND or (f32_bits & 0xffffffff) >= F32_FOUND


def update_scale(scale: float, tracker: int, found_inf: bool, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                 growth_interval: int = 2000, min_scale: float = 1.0, max_scale: float = 65536.0):
    """One step of the policy (torch's `_amp_update_scale_`, plus the clamps): returns (scale, tracker)."""
    if found_inf:
        return max(scale * backoff_factor, min_scale), 0
    tracker += 1
    if tracker == growth_interval:
        return min(scale * growth_factor, max_scale), 0
    return scale, tracker


class HalfScaler:
    def __init__(self, init_scale: float = 1024.0, growth_factor: float = 2.0, backoff_factor: float = 0.5, growth_interval: int = 2000,
                 min_scale: float = 1.0, max_scale: float = 65536.0, device='cuda', arena=None, dp=None):
        m, _ = np.frexp(float(init_scale))
        if not (m == 0.5 and min_scale <= init_scale <= max_scale):
            raise ValueError('HalfScaler: the initial scale is a power of two in [%g, %g], got %r' % (min_scale, max_scale, init_scale))
        if int(growth_interval) < 1:
            raise ValueError('HalfScaler: growth_interval >= 1')
        self.scale, self.growth_tracker = float(init_scale), 0
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self.min_scale, self.max_scale = float(min_scale), float(max_scale)
        self.arena, self.dp = arena, dp
        dev = torch.device(device if device is not None else 'cuda')
        self.flags = torch.zeros(2, dtype=torch.int32, device=dev)          # [largest half magnitude, largest fp32 magnitude], as bits
        self.found_inf = torch.zeros((), dtype=torch.float32, device=dev)   # what the fused optimizer reads
        self.counters = torch.zeros(2, dtype=torch.int32, device=dev)       # [steps seen, steps skipped]
        self.steps = self.skipped = 0          # the host's tally of the steps it has read the flags of
        self.last_flags = (0, 0)
        self.wait_s = 0.0                      # time the host spent waiting at the flag events (tools/bench_half_guard.py)
        self._pending = collections.deque()    # (event, pinned copy of the flags) per optimizer step not yet read
        self._free = []
        self._hooks = []

    # ---- the scans (called by the operators of half_train.py and by the step hook)
    def scan_half(self, t: torch.Tensor):
        """A half gradient tensor, on the current stream -- the one that has just produced it."""
        assert t.dtype == torch.float16
        if t.dim() != 2:
            t = t.reshape(1, -1)
        if t.stride(1) != 1:
            t = t.contiguous()
        n, c = t.shape
        _lib.call('b2m_half_absmax', t.data_ptr(), max(t.stride(0), c), n, c, self.flags.data_ptr())

    def scan_f32(self, t: torch.Tensor):
        t = t if t.is_contiguous() else t.contiguous()
        _lib.call('b2m_f32_absmax', t.data_ptr(), t.numel(), self.flags.data_ptr() + 4)

    def _scan_parameter_gradients(self, params):
        """Every fp32 gradient the optimizer is about to read: the arena buffer(s) live gradients point into in one launch each,
        whatever lives elsewhere (the arena gave up for a pass; a parameter of no arena) tensor by tensor."""
        arena = self.arena
        bufs = arena.buffers if arena is not None else ()
        base = [b.data_ptr() if b is not None else None for b in bufs]
        used = [False] * len(bufs)
        for p in params:
            g = p.grad
            if g is None:
                continue
            off = arena.offset.get(id(p)) if arena is not None else None
            if off is not None:
                a = g.data_ptr() - 4 * off
                hit = [j for j, b in enumerate(base) if b == a]
                if hit:
                    used[hit[0]] = True
                    continue
            if g.dtype == torch.float32:
                self.scan_f32(g)
            else:
                self.scan_f32(g.float())
        for j, u in enumerate(used):
            if u:
                self.scan_f32(bufs[j])

    # ---- the pass
    def begin_backward(self):
        """First thing in every backward operator of the half region: read the flags of the steps taken since the last pass (a
        wait for their copies -- the forward pass of this step is already queued) and set the scale this pass runs at."""
        if self._pending:
            self._resolve()
        from . import half_train as HT
        HT.loss_scale[0] = self.scale

    def _resolve(self):
        while self._pending:
            ev, host = self._pending.popleft()
            t0 = time.perf_counter()
            ev.synchronize()
            self.wait_s += time.perf_counter() - t0
            h, f = int(host[0]) & 0xffffffff, int(host[1]) & 0xffffffff
            self._free.append(host)
            hit = found(h, f)
            self.scale, self.growth_tracker = update_scale(self.scale, self.growth_tracker, hit, self.growth_factor, self.backoff_factor,
                                                           self.growth_interval, self.min_scale, self.max_scale)
            self.steps += 1
            self.skipped += int(hit)
            self.last_flags = (h, f)

    # ---- the optimizer
    def attach(self, optimizer):
        """The optimizer skips a step the guard flags -- parameters, moments and step counts, on the device.  Only torch's FUSED
        implementations read `optimizer.found_inf`; the others assert that it is None."""
        groups = optimizer.param_groups
        if not groups or not all(g.get('fused') for g in groups):
            raise TypeError('HalfScaler.attach needs a fused optimizer (torch.optim.Adam(..., fused=True)): only the fused '
                            'implementations skip a step on `found_inf`, on the device; got %s' % type(optimizer).__name__)
        optimizer.found_inf = self.found_inf
        self._hooks.append(optimizer.register_step_pre_hook(self._before_step))
        return optimizer

    def detach(self, optimizer):
        """Undo attach(): the optimizer steps unconditionally again."""
        for h in self._hooks:
            h.remove()
        self._hooks = []
        optimizer.found_inf = None

    def _before_step(self, optimizer, args, kwargs):
        from . import functional as F_
        F_.join_side_streams()                       # the weight gradients issued on the side stream
        world = 1
        if self.dp is not None:
            self.dp.all_reduce_mean()                # (done when backward ended; a caller without hooks gets it here)
            world = self.dp.world
        self._scan_parameter_gradients([p for g in optimizer.param_groups for p in g['params']])
        if world > 1:
            # every rank, every step: the sequence of collectives does not depend on what a rank found (stream-ordered over RCCL;
            # gloo, the rehearsal backend, stages through the host as it does for the gradient buckets)
            import torch.distributed as dist
            dist.all_reduce(self.flags, op=dist.ReduceOp.MAX, group=self.dp.group)      # (bits <= 0x7fffffff: signed order is theirs)
        _lib.call('b2m_guard_finish', self.flags.data_ptr(), self.found_inf.data_ptr(), self.counters.data_ptr())
        host = self._free.pop() if self._free else torch.empty(2, dtype=torch.int32).pin_memory()
        host.copy_(self.flags, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._pending.append((ev, host))
        self.flags.zero_()                           # the next step's maxima start from nothing

    # ---- surface
    def stats(self):
        """Scale (of the next pass), steps seen, steps skipped and the largest half gradient (as stored: scaled) of the last step.
        Reads the flags of every step taken so far: a host wait when the last one is still in flight."""
        self._resolve()
        h, f = self.last_flags
        return {'scale': self.scale, 'growth_tracker': self.growth_tracker, 'steps': self.steps, 'skipped': self.skipped,
                'max_half_grad': float(np.array([h & 0x7fff], dtype=np.uint16).view(np.float16)[0]),
                'max_grad': float(np.array([f & 0x7fffffff], dtype=np.uint32).view(np.float32)[0])}

    def state_dict(self):
        self._resolve()
        steps, skipped = (int(v) & 0xffffffff for v in self.counters.tolist())
        return {'scale': self.scale, 'growth_tracker': self.growth_tracker, 'steps': steps, 'skipped': skipped}

    def load_state_dict(self, state):
        m, _ = np.frexp(float(state['scale']))
        if not (m == 0.5 and self.min_scale <= state['scale'] <= self.max_scale):
            raise ValueError('HalfScaler: the scale is a power of two in [%g, %g], got %r' % (self.min_scale, self.max_scale, state['scale']))
        self._resolve()
        self.scale, self.growth_tracker = float(state['scale']), int(state['growth_tracker'])
        self.steps, self.skipped = int(state['steps']), int(state['skipped'])
        self.counters.copy_(torch.tensor([self.steps, self.skipped], dtype=torch.int64).to(torch.int32))
