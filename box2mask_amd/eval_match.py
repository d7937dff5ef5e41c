"""ScanNet AP on the device: the second half of eval_metric -- the per-row bookkeeping of ``assign_from_counts``, the greedy
matching of ``evaluate_matches`` for the ten overlaps and eighteen classes, the precision / recall curve and the AP -- for one
evaluation or for every setting of a threshold sweep (box2mask_amd/param_search.py).  Kernels: box2mask_amd/csrc/apmatch.hip
(``b2m_ap_rows``, ``b2m_ap_match``, ``b2m_ap_curve``) and the existing ``b2m_sort_u64``.  No CPU fallback.

The rule is eval_metric's own, restated over flat arrays in tests/_ap_rule.py.  Every integer of it -- the entries of every
(setting, overlap, class) segment, hard false negatives, flags, tp / fp / fn -- and precision, recall and the steps are
reproduced exactly.  ONE deviation: the AP is the dot product of precision and steps summed in ascending order of the
thresholds, where ``np.dot`` sums in the order of the BLAS; for a curve of n points the two differ by at most 4 n 2^-53.

Opt-in: ``eval_metric.compute_eval`` and ``scannet_param_search(..., matching='host')`` are unchanged and remain the defaults.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import eval_metric

N_CLASS, N_OVERLAP = len(eval_metric.CLASS_LABELS), len(eval_metric.OVERLAPS)
N_SEG = N_CLASS * N_OVERLAP
MAX_IDS = 2048
ENTRIES_PER_ROW = 12            # 3 at overlap 0.25 (disjoint ground truths exceed 1/4 of a row at most three times), 1 at the nine others
_DESC = 9                       # B2M_AP_DESC


def gt_table(uniq, gt_vert):
    """(3, G) int32 of one scene: class index of ``id // 1000`` among VALID_CLASS_IDS or -1 | ``id >= 1000`` | points of the id."""
    uniq = np.asarray(uniq, np.int64).reshape(-1)
    gt_vert = np.asarray(gt_vert, np.int64).reshape(-1)
    if uniq.shape != gt_vert.shape:
        raise ValueError('%d ground-truth ids, %d point counts' % (uniq.shape[0], gt_vert.shape[0]))
    if uniq.shape[0] > MAX_IDS:
        raise ValueError('more than 2048 ground-truth ids in one scene')
    if uniq.size and (uniq.min() < 0 or np.any(np.diff(uniq) <= 0)):
        raise ValueError('the ground-truth ids must be ascending, distinct and not negative (np.unique)')
    if gt_vert.size and (gt_vert.min() < 0 or gt_vert.max() > 0x7FFFFFFF):
        raise ValueError('point counts out of range')
    cls = uniq // 1000
    pos = np.searchsorted(eval_metric.VALID_CLASS_IDS, cls)
    ok = (pos < N_CLASS) & (eval_metric.VALID_CLASS_IDS[np.minimum(pos, N_CLASS - 1)] == cls)
    return np.stack([np.where(ok, pos, -1), (uniq >= 1000).astype(np.int64), gt_vert]).astype(np.int32)


def _conf32(conf, dev):
    """The scores as a float32 device tensor; anything that is not exactly float32 is refused."""
    t = torch.as_tensor(conf)
    if t.dtype == torch.float32:
        return t.to(dev).contiguous()
    if t.dtype == torch.float64:
        t32 = t.to(torch.float32)
        if bool((t32.to(torch.float64) == t).all()):
            return t32.to(dev).contiguous()
        raise ValueError('conf holds float64 values that are not float32: the scores are float32 confidences')
    raise ValueError('conf must be float32 (got %s)' % (t.dtype,))


class MatchAccumulator:
    """Entries of the matching for ``n_settings`` settings over any number of ``add`` calls (batches), then the AP table.

    ``add(scenes, set_id, prefix, keep, keep_row)``: ``scenes`` is a list of dicts with
        inter     (K, G) or (K, ld >= G) int32 device tensor (anything else is copied there): points shared by row and id,
        label_id  (K,) int32,  conf (>= K,) float32 (the first K are read),
        uniq      (G,) ascending ground-truth ids, gt_vert (G,) their point counts (host arrays; G <= 2048);
    setting j of the call is setting ``set_id[j]`` of all; in scene s it selects row r iff ``r < prefix[s][j]`` and
    (``keep_row[j] < 0`` or ``keep[keep_row[j], row0_s + r] != 0``) where row0_s is the scene's first row in the concatenation of the
    call's scenes (``scene['row0']`` overrides it).  ``keep``: (n_rows, stride) int32 device tensor.  The defaults are one
    evaluation: setting 0 keeps every row.  One host read per call: the entry count."""

    def __init__(self, n_settings):
        _lib.require_gpu()
        n_settings = int(n_settings)
        if not 1 <= n_settings <= (1 << 20):
            raise ValueError('1 <= n_settings <= 2^20')
        self.n_settings = n_settings
        self.dev = torch.device('cuda', torch.cuda.current_device())
        self.hard_fn = torch.zeros(n_settings * N_SEG, dtype=torch.int32, device=self.dev)
        self.flags = torch.zeros(n_settings * N_CLASS, dtype=torch.int32, device=self.dev)
        self.chunks, self.n_entries = [], 0
        self.ths = np.ascontiguousarray(eval_metric.OVERLAPS, np.float64)
        self._sorted = None

    # -------------------------------------------------------------------------------------------------------------- one batch
    def add(self, scenes, set_id=None, prefix=None, keep=None, keep_row=None):
        if self._sorted is not None:
            raise RuntimeError('this MatchAccumulator is finished: make a new one')
        dev, S = self.dev, len(scenes)
        if S == 0:
            return 0
        set_id = np.zeros(1, np.int64) if set_id is None else np.asarray(set_id, np.int64).reshape(-1)
        n_set = len(set_id)
        if n_set == 0:
            return 0
        if set_id.min() < 0 or set_id.max() >= self.n_settings:
            raise ValueError('set_id outside [0, %d)' % self.n_settings)
        keep_row = np.full(n_set, -1, np.int64) if keep_row is None else np.asarray(keep_row, np.int64).reshape(-1)
        if keep_row.shape != (n_set,):
            raise ValueError('%d settings, %d keep rows' % (n_set, keep_row.shape[0]))
        if keep is None:
            if keep_row.max() >= 0:
                raise ValueError('keep_row names rows of a keep table that was not given')
            keep_rows = keep_stride = 0
        else:
            if not (isinstance(keep, torch.Tensor) and keep.is_cuda and keep.dtype == torch.int32 and keep.dim() == 2 and
                    keep.is_contiguous()):
                raise ValueError('keep must be a contiguous (rows, stride) int32 device tensor')
            keep_rows, keep_stride = int(keep.shape[0]), int(keep.shape[1])
            if keep_row.max() >= keep_rows:
                raise ValueError('keep_row outside the %d rows of keep' % keep_rows)
        hold, desc, gts, ks = [], np.zeros((S, _DESC), np.int64), [], []
        row0 = 0
        for s, sc in enumerate(scenes):
            gt = gt_table(sc['uniq'], sc['gt_vert'])
            G = gt.shape[1]
            label = torch.as_tensor(sc['label_id'])
            if label.dim() != 1:
                raise ValueError('label_id must be (K,)')
            K = int(label.shape[0])
            label = label.to(dev, torch.int32).contiguous()
            inter = torch.as_tensor(sc['inter'])
            if inter.dim() != 2 or int(inter.shape[0]) != K or int(inter.shape[1]) < G:
                raise ValueError('inter must be (K, ld >= G) = (%d, >= %d), got %s' % (K, G, tuple(inter.shape)))
            inter = inter.to(dev, torch.int32).contiguous()
            conf = _conf32(sc['conf'], dev)
            if conf.dim() != 1 or int(conf.shape[0]) < K:
                raise ValueError('%d rows, %d scores' % (K, int(conf.shape[0]) if conf.dim() == 1 else -1))
            r0 = int(sc.get('row0', row0))
            if keep is not None and (r0 < 0 or r0 + K > keep_stride):
                raise ValueError('the rows of scene %d lie outside the keep table' % s)
            hold += [label, inter, conf]
            desc[s, :6] = (inter.data_ptr(), K, G, int(inter.shape[1]), label.data_ptr(), conf.data_ptr())
            desc[s, 8] = row0 if keep is None else r0
            gts.append(gt.reshape(-1))
            ks.append(K)
            row0 += K
        total_k = row0
        if keep is not None:
            total_k = max(total_k, max(int(desc[s, 8]) + ks[s] for s in range(S)))      # `taken` is indexed like keep
        prefix = np.asarray([[k] * n_set for k in ks] if prefix is None else prefix, np.int64)
        if prefix.shape != (S, n_set):
            raise ValueError('prefix must be (scenes, settings) = (%d, %d)' % (S, n_set))
        if prefix.min() < 0 or np.any(prefix > np.asarray(ks)[:, None]):
            raise ValueError('a prefix length outside [0, K]')
        # one upload: the ground-truth tables | settings | prefixes (int32), one for the records (int64)
        small = np.concatenate(gts + [set_id.astype(np.int32), keep_row.astype(np.int32), prefix.astype(np.int32).reshape(-1)]).astype(np.int32)
        small_dev = torch.from_numpy(small).to(dev)
        rows_dev = torch.empty(max(3 * sum(ks), 1), dtype=torch.int32, device=dev)
        o_gt = o_rows = 0
        for s in range(S):
            desc[s, 6] = small_dev.data_ptr() + 4 * o_gt
            desc[s, 7] = rows_dev.data_ptr() + 4 * o_rows
            o_gt += 3 * int(desc[s, 2]); o_rows += 3 * ks[s]
        p_set = small_dev.data_ptr() + 4 * o_gt
        desc_dev = torch.from_numpy(desc.reshape(-1)).to(dev)
        selected = int(np.minimum(prefix, np.asarray(ks)[:, None]).sum())
        cap = ENTRIES_PER_ROW * selected
        slab = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        taken = torch.empty(max(n_set * N_OVERLAP * total_k, 1), dtype=torch.uint8, device=dev)
        _lib.call('b2m_ap_rows', desc_dev.data_ptr(), S, max(ks))
        _lib.call('b2m_ap_match', desc_dev.data_ptr(), S, total_k, p_set, p_set + 4 * n_set, p_set + 8 * n_set, n_set,
                  keep.data_ptr() if keep is not None else None, keep_stride, self.ths.ctypes.data, taken.data_ptr(), slab.data_ptr(),
                  cap, count.data_ptr(), self.hard_fn.data_ptr(), self.flags.data_ptr(), self.n_settings)
        n = int(count.item())                                              # the one host read
        if n > cap:
            raise _lib.B2MError('b2m_ap_match: %d entries for a bound of %d (12 per selected row): the intersection counts are '
                                'not those of disjoint ground truths' % (n, cap))
        if n:
            self.chunks.append(slab[:n].clone() if cap > 2 * n + 1024 else slab[:n])
            self.n_entries += n
        del hold
        return n

    # -------------------------------------------------------------------------------------------------------------- the table
    def finish(self, debug_segment=None, debug_cap=0):
        """(n_settings, classes, overlaps) fp64 numpy: ``evaluate_matches``' table of every setting.  With ``debug_segment`` =
        (setting, overlap, class) also a dict(tp, fp, fn, precision, recall, steps) of that segment (None where it has no curve);
        ``debug_cap`` bounds its length."""
        dev = self.dev
        if self._sorted is None:
            n = self.n_entries
            n_pad = 2
            while n_pad < n:
                n_pad *= 2
            if n_pad >= (1 << 31):
                raise ValueError('%d entries: more than one sort holds' % n)
            keys = torch.full((n_pad,), -1, dtype=torch.int64, device=dev)    # 2^64 - 1 behind the entries
            o = 0
            for c in self.chunks:
                keys[o:o + c.shape[0]] = c
                o += c.shape[0]
            self.chunks = []
            _lib.call('b2m_sort_u64', keys.data_ptr(), n_pad)
            self._sorted = keys
        ap = torch.empty((self.n_settings, N_CLASS, N_OVERLAP), dtype=torch.float64, device=dev)
        seg, cap = -1, 0
        if debug_segment is not None:
            q, o, c = (int(v) for v in debug_segment)
            if not (0 <= q < self.n_settings and 0 <= o < N_OVERLAP and 0 <= c < N_CLASS):
                raise ValueError('debug_segment names no segment')
            seg, cap = q * N_SEG + o * N_CLASS + c, max(int(debug_cap), 1)
        counts = torch.zeros((3, max(cap, 1)), dtype=torch.int64, device=dev)
        curve = torch.zeros((3, max(cap, 1)), dtype=torch.float64, device=dev)
        dn = torch.zeros(1, dtype=torch.int64, device=dev)
        _lib.call('b2m_ap_curve', self._sorted.data_ptr(), self.n_entries, self.hard_fn.data_ptr(), self.flags.data_ptr(),
                  self.n_settings, ap.data_ptr(), seg, cap, counts.data_ptr(), curve.data_ptr(), dn.data_ptr())
        table = ap.cpu().numpy()
        if debug_segment is None:
            return table
        m = int(dn.item())
        if m == 0:
            return table, None
        if m > cap:
            raise ValueError('the segment has %d points: debug_cap = %d is too small' % (m, cap))
        cn, cv = counts.cpu().numpy(), curve.cpu().numpy()
        return table, dict(tp=cn[0, :m - 1], fp=cn[1, :m - 1], fn=cn[2, :m - 1], precision=cv[0, :m], recall=cv[1, :m], steps=cv[2, :m])


def _device_counts(pred_masks, gt_ids, dev):
    """``eval_metric.intersections`` with the counts left on the device: (uniq (G,), gt_vert (G,) host arrays, inter (K, G) int32)."""
    from .prepare import _unique_inverse
    from ._lib import ptr
    masks = torch.as_tensor(pred_masks).to(dev)
    if masks.dtype != torch.bool:
        masks = masks != 0
    masks = masks.to(torch.uint8).contiguous()
    k, n = masks.shape
    ids = torch.as_tensor(np.ascontiguousarray(gt_ids) if isinstance(gt_ids, np.ndarray) else gt_ids).to(dev).long()
    if tuple(ids.shape) != (n,):
        raise ValueError('mask length %d vs %d ground-truth ids' % (n, ids.shape[0]))
    if int(ids.min().item()) < 0:
        raise ValueError('negative ground-truth ids')
    ukeys, g, dense, _, _, _ = _unique_inverse(ids)
    if g > MAX_IDS:
        raise ValueError('more than 2048 ground-truth ids in one scene')
    words = (n + 63) // 64
    bits = torch.empty((k + 1, max(words, 1)), dtype=torch.int64, device=dev)
    both = torch.cat([masks, torch.ones((1, n), dtype=torch.uint8, device=dev)], 0)     # row k: every point -> gt_vert
    _lib.call('b2m_mask_pack', ptr(both), k + 1, n, ptr(bits), words)
    hist = torch.empty((k + 1, g), dtype=torch.int32, device=dev)
    dense32 = dense.int().contiguous()
    _lib.call('b2m_mask_hist', ptr(bits), words, k + 1, ptr(dense32), n, g, ptr(hist))
    return ukeys[:g].cpu().numpy(), hist[k].cpu().numpy().astype(np.int64), hist[:k]


def compute_eval_device(results, gt_ids_by_scene):
    """``eval_metric.compute_eval`` with the matching on the device: the same arguments, the same averages dictionary (through the
    unchanged ``compute_averages``; the AP within 4 n 2^-53 of the host route's, see the module text).  Returns the averages
    ONLY: there is no curves dictionary on this route."""
    _lib.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    acc = MatchAccumulator(1)
    for name in results:
        info = results[name]
        uniq, gt_vert, inter = _device_counts(info['mask'], gt_ids_by_scene[name], dev)
        label = torch.as_tensor(np.asarray(torch.as_tensor(info['label_id']).cpu()).astype(np.int32))
        acc.add([dict(inter=inter, label_id=label, conf=torch.as_tensor(info['conf']), uniq=uniq, gt_vert=gt_vert)])
    return eval_metric.compute_averages(acc.finish()[:1])
