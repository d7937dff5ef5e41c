"""Replay of a SyncBN operator over W ranks that hold DIFFERENT rows, in one process and without torch.distributed: no second device
context, nothing that can wait for a peer.

The ranks run one after the other, in passes.  In pass p, rank r's k-th statistics exchange first stores a copy of what the rank
contributes and then replaces the tensor by the sum, in rank order, of ALL ranks' k-th contributions of pass p - 1 (a contribution
that is missing there counts as zero; in pass 0, which has no pass before it, a rank sees its own contribution alone).  Rank order is
the order in which xchg_allreduce_kernel adds the mailboxes, so every rank is handed the same bits.  Every pass starts from fresh
copies of the inputs, parameters and running statistics (the caller's `run_rank` makes them).

Why this is exact.  The k-th contribution of a rank is a function of its inputs and of the results of exchanges 0 .. k - 1.  The
first contribution depends on the inputs alone, so it is right in pass 0; if contributions 0 .. k - 1 of every rank are right in pass
p - 1, every rank receives the right sums 0 .. k - 1 in pass p and, being deterministic, forms the right k-th contribution there.  An
operator whose exchanges form a chain of length E has therefore all contributions right in pass E - 1, is handed all the right sums in
pass E and computes in that pass what W processes would have computed.  One pass more (E + 1 passes in all; a BatchNorm layer, E = 2:
three) makes the convergence checkable: the last pass must reproduce the contributions of the pass before it BIT FOR BIT, which also
shows that the reductions in front of the exchange are fixed-order.

What replay() asserts by itself:
  * from pass 1 on, every rank issues the same sequence of (numel, dtype) -- ranks that disagree here wait for each other for ever
    over a real transport (or, over the mailboxes, add slots that do not belong together);
  * the last pass reproduces the contributions of the pass before it bit for bit;
  * whatever the ranks return under the names in SHARED (the constants and running statistics of a SyncBN layer, with any suffix
    after an underscore) has the same bits on every rank in the last pass.
"""
import numpy as np

SHARED = ('mean', 'invstd', 'scale', 'shift', 'running_mean', 'running_var')


def _is_torch(t):
    return hasattr(t, 'data_ptr')


def _copy(t):
    return t.detach().clone() if _is_torch(t) else np.array(t, copy=True)


def _numel(t):
    return int(t.numel()) if _is_torch(t) else int(np.asarray(t).size)


def _bits(t):
    a = t.detach().cpu().numpy() if _is_torch(t) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint8)


def _fmt(seq):
    return '[' + ', '.join('(%d, %s)' % (k, str(d).replace('torch.', '')) for k, d in seq) + ']'


class Replay:
    """The exchange of one pass: `exchange(r)` is what rank r calls in place of the all-reduce."""

    def __init__(self, world, prev):
        self.world, self.prev = world, prev
        self.sent = [[] for _ in range(world)]              # [rank][k]: a copy of the contribution
        self.seq = [[] for _ in range(world)]               # [rank][k]: (numel, dtype)

    def exchange(self, r):
        def all_reduce(t, group=None):
            k = len(self.sent[r])
            self.sent[r].append(_copy(t))
            self.seq[r].append((_numel(t), t.dtype))
            if self.prev is None:
                return                                      # pass 0: this rank alone
            total = None
            for q in range(self.world):                     # rank order
                theirs = self.prev.sent[q]
                if k >= len(theirs) or theirs[k].shape != t.shape or theirs[k].dtype != t.dtype:
                    continue                                # missing (a mismatch is reported by check_sequences): zero
                total = _copy(theirs[k]) if total is None else total + theirs[k]
            if total is None:
                total = t * 0
            if _is_torch(t):
                t.copy_(total)
            else:
                t[...] = total
        return all_reduce

    def check_sequences(self, p):
        for q in range(1, self.world):
            assert self.seq[q] == self.seq[0], \
                'pass %d: the ranks would wait for each other: rank 0 issued %s, rank %d issued %s' % (p, _fmt(self.seq[0]), q, _fmt(self.seq[q]))


def replay(world, run_rank, passes):
    """run_rank(r, all_reduce) -> dict of results: runs rank r's operator from fresh inputs, every statistics exchange through
    all_reduce(t[, group]) (in place).  -> (the results of the last pass, one dict per rank; the common exchange sequence)."""
    assert passes >= 2
    prev, out = None, None
    for p in range(passes):
        cur = Replay(world, prev)
        out = [run_rank(r, cur.exchange(r)) for r in range(world)]
        if p >= 1:
            cur.check_sequences(p)
        prev_prev, prev = prev, cur
    for r in range(world):
        for k, (a, b) in enumerate(zip(prev_prev.sent[r], prev.sent[r])):
            assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), \
                'rank %d, exchange %d: the contribution of the last pass is not the one of the pass before it (%d passes are too ' \
                'few for this chain of exchanges, or a reduction is not fixed-order)' % (r, k, passes)
    for name in sorted(set().union(*[set(o) for o in out])):
        if name.split('_')[0] in ('running',):
            base = '_'.join(name.split('_')[:2])
        else:
            base = name.split('_')[0]
        if base not in SHARED:
            continue
        have = [r for r in range(world) if name in out[r] and out[r][name] is not None]
        for r in have[1:]:
            assert np.array_equal(_bits(out[have[0]][name]), _bits(out[r][name])), \
                '%s differs between rank %d and rank %d in the last pass' % (name, have[0], r)
    return out, prev.seq[0]
