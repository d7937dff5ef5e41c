// ScanNet AP on the device: the second half of the reference's utils/eval_metric.py -- the per-row bookkeeping of
// assign_instances_for_scan (:281-345), the greedy matching of evaluate_matches (:102-199) for the ten overlaps and eighteen
// classes, the precision / recall curve and the AP (:205-247) -- for every setting of a threshold sweep at once.  Host mirror:
// box2mask_amd/eval_match.py; the rule in numpy: tests/_ap_rule.py; the host route: box2mask_amd/eval_metric.py.
//
// Three kernels, all plain C++, integer atomics only:
//   ap_rows_kernel    one thread per prediction row: vert, void, class index;
//   ap_match_kernel   one thread per (scene, setting, class, overlap).  An item is a few hundred dependent steps along its ground
//                     truths and nothing else, so the items -- not an item's rows -- are spread over the lanes: neighbouring lanes
//                     are the overlaps and classes of ONE (scene, setting) and read the same rows of `inter`, `keep` and the row
//                     table; a sweep stage of 8 scenes x 25 settings is 36 000 items;
//   ap_curve_kernel   one thread per (setting, overlap, class) segment of the sorted entries: the curve is a sequential sum by
//                     definition.
// Every result is integers, fp64 divisions of integers (IEEE: the comparisons with the overlap are exact) and one sequential
// fp64 sum: the same bits on every run, whatever order the atomics took.
#include "b2m_common.h"
#pragma clang fp contract(off)

#define AP_THREADS 256
#define AP_SEGS (B2M_AP_CLASSES * B2M_AP_OVERLAPS)

struct ApScene {
    const int32_t* inter; int64_t k; int64_t g; int64_t ld; const int32_t* label; const float* conf; const int32_t* gt;
    int32_t* rows; int64_t row0;
};
static_assert(sizeof(ApScene) == B2M_AP_DESC * 8, "ApScene must match B2M_AP_DESC");

// VALID_CLASS_IDS of the ScanNet benchmark (utils/eval_metric.py:15), ascending
__device__ __forceinline__ int ap_class_index(int label) {
    const int ids[B2M_AP_CLASSES] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39};
    int c = -1;
#pragma unroll
    for (int i = 0; i < B2M_AP_CLASSES; ++i) c = ids[i] == label ? i : c;
    return c;
}

__global__ __launch_bounds__(AP_THREADS) void ap_rows_kernel(const ApScene* __restrict__ sc) {
    const ApScene d = sc[blockIdx.y];
    const int64_t r = (int64_t)blockIdx.x * AP_THREADS + threadIdx.x;
    if (r >= d.k) return;
    const int32_t* row = d.inter + r * d.ld;
    int vert = 0, vd = 0;
    for (int64_t g = 0; g < d.g; ++g) {
        const int in = row[g];
        vert += in;
        vd += d.gt[g] < 0 ? in : 0;
    }
    const int c = ap_class_index(d.label[r]);
    d.rows[r] = vert;
    d.rows[d.k + r] = vd;
    d.rows[2 * d.k + r] = vert >= B2M_AP_MIN_REGION ? c : -1;
}

// float -> uint32 whose unsigned order is the order of the floats (-0 counts as +0, as in a comparison)
__device__ __forceinline__ uint32_t ap_score_key(float v) {
    const uint32_t u = __float_as_uint(v + 0.0f);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}

struct ApOverlaps { double th[B2M_AP_OVERLAPS]; };

__device__ __forceinline__ void ap_emit(uint64_t* __restrict__ entries, int64_t cap, unsigned long long* __restrict__ n_entries,
                                        uint64_t seg, float score, bool is_true) {
    const unsigned long long at = atomicAdd(n_entries, 1ull);
    if ((int64_t)at < cap) entries[at] = (seg << 33) | ((uint64_t)ap_score_key(score) << 1) | (is_true ? 1ull : 0ull);
}

__global__ __launch_bounds__(AP_THREADS) void ap_match_kernel(
    const ApScene* __restrict__ sc, int n_scenes, int64_t total_k, const int32_t* __restrict__ set_id,
    const int32_t* __restrict__ set_keep, const int32_t* __restrict__ set_pref, int n_set, const int32_t* __restrict__ keep,
    int64_t keep_stride, ApOverlaps ths, uint8_t* __restrict__ taken_all, uint64_t* __restrict__ entries, int64_t cap,
    unsigned long long* __restrict__ n_entries, int32_t* __restrict__ hard_fn, int32_t* __restrict__ flags) {
    const int64_t item = (int64_t)blockIdx.x * AP_THREADS + threadIdx.x;
    if (item >= (int64_t)n_scenes * n_set * AP_SEGS) return;
    const int o = (int)(item % B2M_AP_OVERLAPS);
    const int c = (int)((item / B2M_AP_OVERLAPS) % B2M_AP_CLASSES);
    const int j = (int)((item / AP_SEGS) % n_set);
    const int s = (int)(item / ((int64_t)AP_SEGS * n_set));
    const ApScene d = sc[s];
    double th = ths.th[0];
#pragma unroll
    for (int i = 1; i < B2M_AP_OVERLAPS; ++i) th = o == i ? ths.th[i] : th;       // (no indexed read of the argument: no scratch)
    const int sid = set_id[j];
    const int krow = set_keep[j];
    int64_t pref = set_pref[(int64_t)s * n_set + j];
    pref = pref < d.k ? pref : d.k;
    const int32_t* kp = krow >= 0 ? keep + (int64_t)krow * keep_stride + d.row0 : nullptr;
    const int32_t* vert = d.rows;
    const int32_t* vd = d.rows + d.k;
    const int32_t* cls = d.rows + 2 * d.k;
    const int32_t* gcls = d.gt;
    const int32_t* gbig = d.gt + d.g;
    const int32_t* gvert = d.gt + 2 * d.g;
    uint8_t* taken = taken_all + ((int64_t)j * B2M_AP_OVERLAPS + o) * total_k + d.row0;
    const uint64_t seg = (uint64_t)sid * AP_SEGS + (uint64_t)(o * B2M_AP_CLASSES + c);

    // the rows of the class this setting keeps: [first, last)
    int64_t first = pref, last = 0;
    for (int64_t r = 0; r < pref; ++r) {
        if (cls[r] != c || (kp && kp[r] == 0)) continue;
        first = r < first ? r : first;
        last = r + 1;
    }
    const bool has_pred = last > 0;
    bool has_gt = false;
    int hard = 0;
    // greedy assignment: ground truths in ascending id, rows in row order (eval_metric.py:143-172)
    for (int64_t g = 0; g < d.g; ++g) {
        if (gcls[g] != c) continue;
        const int gv = gvert[g];
        if (gbig[g] == 0 || gv < B2M_AP_MIN_REGION) continue;
        has_gt = true;
        bool found = false;
        float best = 0.0f;
        for (int64_t r = first; r < last; ++r) {
            if (cls[r] != c || (kp && kp[r] == 0)) continue;
            const int in = d.inter[r * d.ld + g];
            if (in <= 0 || taken[r]) continue;
            const int64_t un = (int64_t)gv + vert[r] - in;              // (both can be close to 2^31 points)
            const double iou = (double)in / (double)(un > 1 ? un : 1);
            if (!(iou > th)) continue;
            const float cf = d.conf[r];
            if (!found) {
                found = true;
                best = cf;
                taken[r] = 1;
            } else {                                    // a second row on a matched ground truth: a false positive, not taken
                ap_emit(entries, cap, n_entries, seg, best < cf ? best : cf, false);
                best = best > cf ? best : cf;
            }
        }
        if (found) ap_emit(entries, cap, n_entries, seg, best, true);
        else ++hard;
    }
    // rows that reach no ground truth of their class at this overlap (:178-199)
    for (int64_t r = first; r < last; ++r) {
        if (cls[r] != c || (kp && kp[r] == 0)) continue;
        const int vr = vert[r];
        bool hit = false;
        int64_t ignore = vd[r];
        for (int64_t g = 0; g < d.g; ++g) {
            if (gcls[g] != c) continue;
            const int in = d.inter[r * d.ld + g];
            if (in <= 0) continue;
            const int gv = gvert[g];
            const int64_t un = (int64_t)gv + vr - in;
            hit = hit || ((double)in / (double)(un > 1 ? un : 1) > th);
            ignore += gbig[g] == 0 ? in : 0;
            ignore += gv < B2M_AP_MIN_REGION ? in : 0;
        }
        if (hit) continue;
        if ((double)ignore / (double)vr <= th) ap_emit(entries, cap, n_entries, seg, d.conf[r], false);
    }
    if (hard) atomicAdd(hard_fn + seg, hard);
    const int f = (has_gt ? 1 : 0) | (has_pred ? 2 : 0);
    if (f && o == 0) atomicOr(flags + (int64_t)sid * B2M_AP_CLASSES + c, f);
}

// first index in [0, n) whose key is >= v
__device__ __forceinline__ int64_t ap_lower_bound(const uint64_t* __restrict__ keys, int64_t n, uint64_t v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(AP_THREADS) void ap_curve_kernel(
    const uint64_t* __restrict__ keys, int64_t n_keys, const int32_t* __restrict__ hard_fn, const int32_t* __restrict__ flags,
    int64_t n_seg, double* __restrict__ ap, int64_t dbg_seg, int64_t dbg_cap, int64_t* __restrict__ dbg_counts,
    double* __restrict__ dbg_curve, int64_t* __restrict__ dbg_n) {
    const int64_t seg = (int64_t)blockIdx.x * AP_THREADS + threadIdx.x;
    if (seg >= n_seg) return;
    const int64_t sid = seg / AP_SEGS;
    const int o = (int)((seg % AP_SEGS) / B2M_AP_CLASSES), c = (int)(seg % B2M_AP_CLASSES);
    double* out = ap + (sid * B2M_AP_CLASSES + c) * B2M_AP_OVERLAPS + o;
    const bool dbg = seg == dbg_seg;
    const int f = flags[sid * B2M_AP_CLASSES + c];
    if (f != 3) {
        *out = (f & 1) ? 0.0 : __longlong_as_double(0x7FF8000000000000ll);
        if (dbg) *dbg_n = 0;
        return;
    }
    const int64_t lo = ap_lower_bound(keys, n_keys, (uint64_t)seg << 33);
    const int64_t hi = ap_lower_bound(keys, n_keys, (uint64_t)(seg + 1) << 33);
    const int64_t n = hi - lo;
    const int64_t hard = hard_fn[seg];
    int64_t n_true = 0;
    for (int64_t i = lo; i < hi; ++i) n_true += (int64_t)(keys[i] & 1ull);
    // point j waits for recall[j + 1]: steps[j] = 0.5 * (j ? recall[j - 1] : recall[0]) - 0.5 * (recall[j + 1] or 0)
    double sum = 0.0, p0 = 0.0, r0 = 0.0, rm1 = 0.0;
    int64_t j = -1, below = 0, i = lo;
    for (;;) {
        double p1, r1;
        const bool closing = i >= hi;
        if (closing) {
            p1 = 1.0; r1 = 0.0;
        } else {
            const int64_t tp = n_true - below, fp = (n - (i - lo)) - tp, fn = below + hard;
            p1 = (double)tp / (double)(tp + fp);
            r1 = (double)tp / (double)(tp + fn);
            if (dbg && j + 1 < dbg_cap) {
                dbg_counts[j + 1] = tp; dbg_counts[dbg_cap + j + 1] = fp; dbg_counts[2 * dbg_cap + j + 1] = fn;
            }
            const uint64_t score = keys[i] >> 1;
            while (i < hi && (keys[i] >> 1) == score) { below += (int64_t)(keys[i] & 1ull); ++i; }
        }
        if (j >= 0) {
            const double step = 0.5 * (j ? rm1 : r0) - 0.5 * r1;
            const double prod = p0 * step;
            sum = sum + prod;
            if (dbg && j < dbg_cap) { dbg_curve[j] = p0; dbg_curve[dbg_cap + j] = r0; dbg_curve[2 * dbg_cap + j] = step; }
        }
        rm1 = r0; p0 = p1; r0 = r1; ++j;
        if (closing) break;
    }
    {   // the closing point itself: nothing follows it
        const double step = 0.5 * (j ? rm1 : r0) - 0.5 * 0.0;
        const double prod = p0 * step;
        sum = sum + prod;
        if (dbg && j < dbg_cap) { dbg_curve[j] = p0; dbg_curve[dbg_cap + j] = r0; dbg_curve[2 * dbg_cap + j] = step; }
    }
    if (dbg) *dbg_n = j + 1;
    *out = sum;
}

extern "C" int b2m_ap_rows(const int64_t* desc, int32_t n_scenes, int32_t max_k, void* stream) {
    B2M_CHECK_ARG(n_scenes >= 0 && n_scenes <= 65535 && max_k >= 0, "bad sizes");
    if (n_scenes == 0 || max_k == 0) return B2M_OK;
    B2M_CHECK_ARG(desc, "NULL argument");
    ap_rows_kernel<<<dim3((unsigned)cdiv64(max_k, AP_THREADS), (unsigned)n_scenes), AP_THREADS, 0, (hipStream_t)stream>>>(
        (const ApScene*)desc);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

extern "C" int b2m_ap_match(const int64_t* desc, int32_t n_scenes, int64_t total_k, const int32_t* set_id, const int32_t* set_keep,
                            const int32_t* set_pref, int32_t n_set, const int32_t* keep, int64_t keep_stride,
                            const double* ths_host, void* taken, uint64_t* entries, int64_t cap, int64_t* n_entries,
                            int32_t* hard_fn, int32_t* flags, int32_t n_settings, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(n_scenes >= 0 && n_scenes <= 65535 && total_k >= 0 && n_set >= 0 && cap >= 0 && keep_stride >= 0, "bad sizes");
    B2M_CHECK_ARG(n_settings >= 1 && n_settings <= (1 << 20), "1 <= n_settings <= 2^20 (the segment number has 31 bits)");
    B2M_CHECK_ARG((int64_t)n_scenes * n_set * AP_SEGS < (1ll << 31) * AP_THREADS, "too many items for one launch");
    B2M_CHECK_ARG(ths_host, "the overlaps are given on the host (ths_host)");
    if (n_scenes == 0 || n_set == 0) return B2M_OK;
    B2M_CHECK_ARG(desc && set_id && set_keep && set_pref && n_entries && hard_fn && flags && (cap == 0 || entries) &&
                  (total_k == 0 || taken), "NULL argument");
    ApOverlaps t;
    for (int i = 0; i < B2M_AP_OVERLAPS; ++i) {
        B2M_CHECK_ARG(ths_host[i] > 0.0 && ths_host[i] < 1.0, "an overlap must lie in (0, 1)");
        t.th[i] = ths_host[i];
    }
    if (total_k > 0) B2M_HIP(hipMemsetAsync(taken, 0, (size_t)n_set * B2M_AP_OVERLAPS * (size_t)total_k, st));
    const int64_t items = (int64_t)n_scenes * n_set * AP_SEGS;
    ap_match_kernel<<<(unsigned)cdiv64(items, AP_THREADS), AP_THREADS, 0, st>>>(
        (const ApScene*)desc, n_scenes, total_k, set_id, set_keep, set_pref, n_set, keep, keep_stride, t, (uint8_t*)taken, entries,
        cap, (unsigned long long*)n_entries, hard_fn, flags);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

extern "C" int b2m_ap_curve(const uint64_t* keys, int64_t n_keys, const int32_t* hard_fn, const int32_t* flags, int32_t n_settings,
                            double* ap, int64_t dbg_seg, int64_t dbg_cap, int64_t* dbg_counts, double* dbg_curve, int64_t* dbg_n,
                            void* stream) {
    B2M_CHECK_ARG(n_keys >= 0 && n_settings >= 1 && n_settings <= (1 << 20), "bad sizes (1 <= n_settings <= 2^20)");
    B2M_CHECK_ARG(hard_fn && flags && ap && (n_keys == 0 || keys), "NULL argument");
    const int64_t n_seg = (int64_t)n_settings * AP_SEGS;
    B2M_CHECK_ARG(dbg_seg < n_seg && dbg_cap >= 0, "dbg_seg names no segment");
    B2M_CHECK_ARG(dbg_seg < 0 || (dbg_counts && dbg_curve && dbg_n && dbg_cap >= 1), "NULL argument (the named segment's tables)");
    ap_curve_kernel<<<(unsigned)cdiv64(n_seg, AP_THREADS), AP_THREADS, 0, (hipStream_t)stream>>>(
        keys, n_keys, hard_fn, flags, n_seg, ap, dbg_seg, dbg_cap, dbg_counts, dbg_curve, dbg_n);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}
