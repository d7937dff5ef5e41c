// Box votes -> instance masks: non-maximum clustering, heat-map projection, mask NMS, label histogram.
// Integer / comparison work; results must be bit-exact against models/iou_nms.py, so floating-point
// contraction is disabled for this file and every IoU is evaluated in torch's operation order.
#include "b2m_common.h"
#pragma clang fp contract(off)

__device__ __forceinline__ float fmax_t(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ float fmin_t(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float clamp0(float x) { return x < 0.f ? 0.f : x; }

// IoU of two axis-aligned boxes given as [min3,max3]; order of operations of torch_IOUs / set_IOUs
// (/root/reference/models/iou_nms.py:4-22,26-45): prod over 3 sides as (s0*s1)*s2,
// union = ((area_a + area_b) - inter) + 1e-6f, result = inter / union (IEEE division).
__device__ __forceinline__ float box_iou(const float* a, const float* b) {
    const float as0 = a[3] - a[0], as1 = a[4] - a[1], as2 = a[5] - a[2];
    const float bs0 = b[3] - b[0], bs1 = b[4] - b[1], bs2 = b[5] - b[2];
    const float i0 = clamp0(fmin_t(a[3], b[3]) - fmax_t(a[0], b[0]));
    const float i1 = clamp0(fmin_t(a[4], b[4]) - fmax_t(a[1], b[1]));
    const float i2 = clamp0(fmin_t(a[5], b[5]) - fmax_t(a[2], b[2]));
    const float inter = (i0 * i1) * i2;
    const float aa = (as0 * as1) * as2, ba = (bs0 * bs1) * bs2;
    const float uni = ((aa + ba) - inter) + 0.000001f;
    return inter / uni;
}

__global__ void set_ious_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n,
                                float* __restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float x[6], y[6];
#pragma unroll
    for (int u = 0; u < 6; ++u) { x[u] = a[i * 6 + u]; y[u] = b[i * 6 + u]; }
    out[i] = box_iou(x, y);
}
extern "C" int b2m_set_ious(const float* a, const float* b, int64_t n, float* out, void* stream) {
    if (n == 0) return B2M_OK;
    B2M_CHECK_ARG(a && b && out && n > 0, "bad arguments");
    set_ious_kernel<<<(unsigned)cdiv64(n, 256), 256, 0, (hipStream_t)stream>>>(a, b, n, out);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// ------------------------------------------------------------------ detection losses, forward + gradients in one launch
// The box and semantics terms of Model.compute_loss_detection in the ScanNet configuration
// (/root/reference/models/model.py:62-88 L1 offset / bounds, :133-176 IoU-target score loss, :194-210 semantics): torch
// evaluates them as ~75 elementwise launches forward and as many backward, all on the critical path between the forward and
// the backward pass of the network.  Here one thread owns one prediction row: the L1 terms, the box IoU against the ground
// truth (set_IOUs' arithmetic), BCE-with-logits against it, the Pearson sums of the logging correlation, cross entropy over
// the class logits and its argmax -- and, in the same pass, the gradient of the weighted total with respect to every head
// output (each is an elementwise function of the row once the normalisers F = foreground rows and n_valid are known).
// Sums in fp64 (block tree, then one atomic per block and value).  out[16] doubles:
//   0 sum |d off|   1 sum |d bounds|   2 sum BCE   3 sum iou   4 sum logit   5 sum iou^2   6 sum logit^2   7 sum iou*logit
//   8 sum CE        9 correct class
// EX (b2m_detection_loss_ex) adds the IoU loss (model.py:91-129) and the centre-score loss (:179-192) to the same row code:
//  10 sum (1 - IoU)   11 sum |centre - target|   12 sum target   13 sum centre   14 sum target^2   15 sum centre^2
//  16 sum target*centre          (target = the row's own L1 offset sum, detached)
struct LossArgs {
    const float* off; int64_t ld_off; const float* bnd; int64_t ld_bnd; const float* sc; int64_t ld_sc;
    const float* sem; int64_t ld_sem; int C;
    const float* gt_off; const float* gt_bnd; const float* loc;            // (S, 3) dense
    const uint8_t* fg; const int64_t* gt_sem; int64_t S;
    float w_off, w_bnd, w_sc, w_sem, min_bb; double F; const double* n_valid;
    float* d_off; float* d_bnd; float* d_sc; float* d_sem; int64_t* argmax; double* out;
    // EX only
    const float* cs; int64_t ld_cs; float* d_cs; float w_iou, w_cs; int use_iou;
};
// d (w_iou / F) * (1 - IoU) / d (offset, bound) of one row, added to g_off / g_bnd; returns 1 - IoU.  The corners are the fp32
// values torch forms (p = predicted box with clamped bounds, g = true box; [min3, max3]); everything after them is fp64.
// Conventions at ties are torch autograd's: maximum / minimum of equal corners send half the gradient to each side, a clamped
// value exactly at its limit (an intersection side of 0, a bound at min_bb_size, a union at the floor) passes the gradient;
// the union's floor is decided on the fp32 union formed in torch's order.
__device__ __forceinline__ double iou_loss_row(const float* p, const float* g, const float* pb, float min_bb, double scale,
                                               double* g_off, double* g_bnd) {
    double s[3], av[3], wl[3], wh[3];
    float sf[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float lo = fmax_t(p[j], g[j]), hi = fmin_t(p[3 + j], g[3 + j]);
        sf[j] = hi - lo;
        const double raw = (double)hi - (double)lo;
        s[j] = sf[j] >= 0.f ? raw : 0.0;
        av[j] = (double)p[3 + j] - (double)p[j];
        wl[j] = p[j] > g[j] ? 1.0 : (p[j] == g[j] ? 0.5 : 0.0);
        wh[j] = p[3 + j] < g[3 + j] ? 1.0 : (p[3 + j] == g[3 + j] ? 0.5 : 0.0);
    }
    const double inter = (s[0] * s[1]) * s[2], va = (av[0] * av[1]) * av[2];
    const double vg = (((double)g[3] - (double)g[0]) * ((double)g[4] - (double)g[1])) * ((double)g[5] - (double)g[2]);
    const double uni = (va + vg) - inter;
    // the same union in fp32, torch's order: decides the floor
    const float interf = (clamp0(sf[0]) * clamp0(sf[1])) * clamp0(sf[2]);
    const float vaf = ((p[3] - p[0]) * (p[4] - p[1])) * (p[5] - p[2]), vgf = ((g[3] - g[0]) * (g[4] - g[1])) * (g[5] - g[2]);
    const bool open = ((vaf + vgf) - interf) >= 0.000001f;
    const double den = open ? uni : (double)0.000001f;
    const double iou = inter / den;
    const double d_i = open ? (1.0 / den + inter / (den * den)) : 1.0 / den;       // d iou / d inter (union = va + vg - inter)
    const double d_v = open ? -inter / (den * den) : 0.0;                           // d iou / d va
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int k = (j + 1) % 3, l = (j + 2) % 3;
        const double di = sf[j] >= 0.f ? s[k] * s[l] : 0.0;                         // d inter / d side j
        g_off[j] -= scale * d_i * di * (wh[j] - wl[j]);
        if (pb[j] >= min_bb) g_bnd[j] -= scale * (d_i * di * (wh[j] + wl[j]) + d_v * 2.0 * (av[k] * av[l]));
    }
    return 1.0 - iou;
}
template <bool EX>
__global__ __launch_bounds__(256) void detection_loss_kernel(LossArgs a) {
    constexpr int NV = EX ? 17 : 10;
    __shared__ double red[4][NV];
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double v[NV] = {};
    if (s < a.S) {
        const bool fg = a.fg == nullptr || a.fg[s] != 0;
        const float inv_f = (float)(1.0 / a.F);
        float po[3], pb[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) { po[j] = a.off[s * a.ld_off + j]; pb[j] = a.bnd[s * a.ld_bnd + j]; }
        if (fg) {
            float l_off = 0.f, l_bnd = 0.f, pbox[6], gbox[6], g_off[3], g_bnd[3];
            double l_off64 = 0.0;                                           // (EX: the centre-score target)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float go = a.gt_off[s * 3 + j], gb = a.gt_bnd[s * 3 + j], lc = a.loc[s * 3 + j];
                const float d0 = po[j] - go, d1 = pb[j] - gb;
                l_off += fabsf(d0); l_bnd += fabsf(d1);
                g_off[j] = d0 > 0.f ? a.w_off * inv_f : (d0 < 0.f ? -a.w_off * inv_f : 0.f);
                g_bnd[j] = d1 > 0.f ? a.w_bnd * inv_f : (d1 < 0.f ? -a.w_bnd * inv_f : 0.f);
                if constexpr (EX) {
                    const double e0 = (double)po[j] - (double)go;
                    l_off64 += d0 > 0.f ? e0 : (d0 < 0.f ? -e0 : 0.0);
                }
                const float pc = po[j] + lc, gc = go + lc;                  // voted / true centre (model.py:147-150)
                const float pbc = pb[j] < a.min_bb ? a.min_bb : pb[j];      // torch.clamp(pred_bounds, min=min_bb_size)
                pbox[j] = pc - pbc; pbox[3 + j] = pc + pbc;
                gbox[j] = gc - gb; gbox[3 + j] = gc + gb;
            }
            v[0] = l_off; v[1] = l_bnd;
            if constexpr (EX) {
                if (a.use_iou) {                                            // model.py:91-129, not detached
                    double e_off[3] = {g_off[0], g_off[1], g_off[2]}, e_bnd[3] = {g_bnd[0], g_bnd[1], g_bnd[2]};
                    v[10] = iou_loss_row(pbox, gbox, pb, a.min_bb, (double)a.w_iou / a.F, e_off, e_bnd);
#pragma unroll
                    for (int j = 0; j < 3; ++j) { g_off[j] = (float)e_off[j]; g_bnd[j] = (float)e_bnd[j]; }
                }
                if (a.cs) {                                                 // model.py:179-192: target = this row's L1 offset sum
                    const float p = a.cs[s * a.ld_cs], d = p - l_off;      // the sign is torch's: fp32 prediction - fp32 target
                    const double e = (double)p - l_off64;
                    v[11] = d > 0.f ? e : (d < 0.f ? -e : 0.0);
                    v[12] = l_off64; v[13] = (double)p; v[14] = l_off64 * l_off64; v[15] = (double)p * (double)p;
                    v[16] = l_off64 * (double)p;
                    a.d_cs[s] = d > 0.f ? (float)((double)a.w_cs / a.F) : (d < 0.f ? (float)(-(double)a.w_cs / a.F) : 0.f);
                }
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) { a.d_off[s * 3 + j] = g_off[j]; a.d_bnd[s * 3 + j] = g_bnd[j]; }
            if (a.sc) {
                const float iou = box_iou(gbox, pbox);                      // set_IOUs(gt_bbs, pred_bbs)
                const double x = (double)a.sc[s * a.ld_sc], y = (double)iou;
                v[2] = (x > 0 ? x : 0) - x * y + log1p(exp(-fabs(x)));      // BCEWithLogitsLoss
                v[3] = y; v[4] = x; v[5] = y * y; v[6] = x * x; v[7] = x * y;
                a.d_sc[s] = (float)((double)a.w_sc * (1.0 / (1.0 + exp(-x)) - y) / a.F);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j) { a.d_off[s * 3 + j] = 0.f; a.d_bnd[s * 3 + j] = 0.f; }
            if (a.sc) a.d_sc[s] = 0.f;
            if constexpr (EX) { if (a.cs) a.d_cs[s] = 0.f; }
        }
        if (a.sem) {
            const float* z = a.sem + s * a.ld_sem;
            const int64_t t = a.gt_sem[s];
            float mx = z[0]; int am = 0;
            for (int c = 1; c < a.C; ++c) if (z[c] > mx) { mx = z[c]; am = c; }        // first maximum, like torch.argmax
            double den = 0;
            for (int c = 0; c < a.C; ++c) den += exp((double)z[c] - (double)mx);
            a.argmax[s] = am;
            v[9] = (t == am) ? 1.0 : 0.0;
            const bool valid = t >= 0 && t < a.C;                                       // ignore_index = -100
            const double inv_n = 1.0 / *a.n_valid;
            if (valid) v[8] = log(den) - ((double)z[t] - (double)mx);
            for (int c = 0; c < a.C; ++c) {
                const double p = exp((double)z[c] - (double)mx) / den;
                a.d_sem[s * a.C + c] = valid ? (float)((double)a.w_sem * (p - (c == t ? 1.0 : 0.0)) * inv_n) : 0.f;
            }
        }
    }
    // block sum in a fixed tree, one atomic per value and block
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        double t = v[u];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) t += __shfl_down(t, d, 64);
        v[u] = t;
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int u = 0; u < NV; ++u) red[threadIdx.x >> 6][u] = v[u];
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const double t = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        if (t != 0.0) atomicAdd(a.out + threadIdx.x, t);
    }
}
// res[0] total, 1 offset_loss, 2 bounds_loss, 3 bb_score_loss, 4 bb_target_scores, 5 bb_scores_correlation, 6 semantics_loss,
// 7 semantics_acc;  EX: 8 iou_loss, 9 center_score_loss, 10 center_scores_correlation, 11..15 zero
// Pearson r of two summed series from their uncentred fp64 sums (n values; sa, sb, saa, sbb, sab).  The centred sums can come
// out a rounding error below zero for (nearly) constant inputs: clamped before the root (a negative product gave NaN -> +-inf
// through the floor below).  Zero variance -- all IoUs 0 at a fresh initialisation -- reads 0 here, as model._pearsonr does;
// scipy.stats.pearsonr returns NaN with a warning for such input.
// The uncentred form  sum x^2 - (sum x)^2 / n  equals the centred sum only up to the rounding of its two terms, each about
// (tree depth + blocks) * 2^-53 of sum x^2: for constant input (every score logit equal) it came out as +-1e-13 instead of the
// exact 0 of  sum (x - mean)^2, and a positive one turned the correlation into ~1e-8 of noise over noise.  A centred sum below
// that rounding is zero variance (tests/test_gpu_loss.py, case equal_scores)
__device__ __forceinline__ float pearson_from_sums(double n, int64_t S, double sa, double sb, double saa, double sbb, double sab) {
    const double ca = saa - sa * sa / n, cb = sbb - sb * sb / n, cab = sab - sa * sb / n;
    const double noise = (double)((S + 255) / 256 + 16) * 0x1p-52;
    const double va = ca > noise * saa ? ca : 0.0, vb = cb > noise * sbb ? cb : 0.0;
    const double den = sqrt(va * vb);
    return den > 1e-300 ? (float)(cab / den) : 0.f;
}
struct LossExFinal { float w_iou, w_cs; int use_iou, has_cs; };
template <bool EX>
__global__ void detection_loss_final_kernel(const double* __restrict__ o, double F, const double* __restrict__ n_valid, int64_t S,
                                            float w_off, float w_bnd, float w_sc, float w_sem, int has_sc, int has_sem,
                                            LossExFinal x, float* __restrict__ res) {
    const double l_off = o[0] / F, l_bnd = o[1] / F;
    double total = (double)w_off * l_off + (double)w_bnd * l_bnd;
    res[1] = (float)l_off; res[2] = (float)l_bnd;
    res[3] = res[4] = res[5] = res[6] = res[7] = 0.f;
    if (has_sc) {
        const double bce = o[2] / F;
        total += (double)w_sc * bce;
        res[3] = (float)bce; res[4] = (float)(o[3] / F);
        res[5] = pearson_from_sums(F, S, o[3], o[4], o[5], o[6], o[7]);        // (IoU, score logit): logging, model.py:88
    }
    if constexpr (EX) {
#pragma unroll
        for (int u = 8; u < 16; ++u) res[u] = 0.f;
        if (x.use_iou) {
            const double l_iou = o[10] / F;
            total += (double)x.w_iou * l_iou;
            res[8] = (float)l_iou;
        }
        if (x.has_cs) {
            const double l_cs = o[11] / F;
            total += (double)x.w_cs * l_cs;
            res[9] = (float)l_cs;
            res[10] = pearson_from_sums(F, S, o[12], o[13], o[14], o[15], o[16]);
        }
    }
    if (has_sem) {
        const double ce = o[8] / *n_valid;
        total += (double)w_sem * ce;
        res[6] = (float)ce; res[7] = (float)(o[9] / (double)S);
    }
    res[0] = (float)total;
}
extern "C" int b2m_detection_loss(const float* off, int64_t ld_off, const float* bnd, int64_t ld_bnd, const float* sc, int64_t ld_sc,
                                  const float* sem, int64_t ld_sem, int32_t n_class, const float* gt_off, const float* gt_bnd,
                                  const float* loc, const uint8_t* fg, const int64_t* gt_sem, int64_t S, double n_fg,
                                  const double* n_valid, float w_off, float w_bnd, float w_sc, float w_sem, float min_bb_size,
                                  float* d_off, float* d_bnd, float* d_sc, float* d_sem, int64_t* argmax, double* sums,
                                  float* result, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(off && bnd && gt_off && gt_bnd && loc && d_off && d_bnd && sums && result && S >= 1 && n_fg >= 1, "bad arguments");
    B2M_CHECK_ARG(ld_off >= 3 && ld_bnd >= 3 && (!sc || (d_sc && ld_sc >= 1)), "leading dimensions / score gradient");
    B2M_CHECK_ARG(!sem || (d_sem && argmax && gt_sem && n_valid && n_class >= 1 && ld_sem >= n_class), "semantics arguments");
    LossArgs a{};
    a.off = off; a.ld_off = ld_off; a.bnd = bnd; a.ld_bnd = ld_bnd; a.sc = sc; a.ld_sc = ld_sc; a.sem = sem; a.ld_sem = ld_sem;
    a.C = n_class; a.gt_off = gt_off; a.gt_bnd = gt_bnd; a.loc = loc; a.fg = fg; a.gt_sem = gt_sem; a.S = S;
    a.w_off = w_off; a.w_bnd = w_bnd; a.w_sc = w_sc; a.w_sem = w_sem; a.min_bb = min_bb_size; a.F = n_fg; a.n_valid = n_valid;
    a.d_off = d_off; a.d_bnd = d_bnd; a.d_sc = d_sc; a.d_sem = d_sem; a.argmax = argmax; a.out = sums;
    B2M_HIP(hipMemsetAsync(sums, 0, 16 * sizeof(double), st));
    detection_loss_kernel<false><<<(unsigned)cdiv64(S, 256), 256, 0, st>>>(a);
    detection_loss_final_kernel<false><<<1, 1, 0, st>>>(sums, n_fg, n_valid, S, w_off, w_bnd, w_sc, w_sem, sc ? 1 : 0, sem ? 1 : 0,
                                                        LossExFinal{}, result);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}
// b2m_detection_loss plus the IoU loss (use_iou) and the centre-score loss (cs != NULL): the same row code, template flag EX.
extern "C" int b2m_detection_loss_ex(const float* off, int64_t ld_off, const float* bnd, int64_t ld_bnd, const float* sc, int64_t ld_sc,
                                     const float* cs, int64_t ld_cs, const float* sem, int64_t ld_sem, int32_t n_class,
                                     const float* gt_off, const float* gt_bnd, const float* loc, const uint8_t* fg,
                                     const int64_t* gt_sem, int64_t S, double n_fg, const double* n_valid, float w_off, float w_bnd,
                                     float w_iou, float w_sc, float w_cs, float w_sem, float min_bb_size, int32_t use_iou,
                                     float* d_off, float* d_bnd, float* d_sc, float* d_cs, float* d_sem, int64_t* argmax,
                                     double* sums, float* result, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(off && bnd && gt_off && gt_bnd && loc && d_off && d_bnd && sums && result && S >= 1 && n_fg >= 1, "bad arguments");
    B2M_CHECK_ARG(ld_off >= 3 && ld_bnd >= 3 && (!sc || (d_sc && ld_sc >= 1)) && (!cs || (d_cs && ld_cs >= 1)),
                  "leading dimensions / score gradients");
    B2M_CHECK_ARG(!sem || (d_sem && argmax && gt_sem && n_valid && n_class >= 1 && ld_sem >= n_class), "semantics arguments");
    LossArgs a{};
    a.off = off; a.ld_off = ld_off; a.bnd = bnd; a.ld_bnd = ld_bnd; a.sc = sc; a.ld_sc = ld_sc; a.sem = sem; a.ld_sem = ld_sem;
    a.C = n_class; a.gt_off = gt_off; a.gt_bnd = gt_bnd; a.loc = loc; a.fg = fg; a.gt_sem = gt_sem; a.S = S;
    a.w_off = w_off; a.w_bnd = w_bnd; a.w_sc = w_sc; a.w_sem = w_sem; a.min_bb = min_bb_size; a.F = n_fg; a.n_valid = n_valid;
    a.d_off = d_off; a.d_bnd = d_bnd; a.d_sc = d_sc; a.d_sem = d_sem; a.argmax = argmax; a.out = sums;
    a.cs = cs; a.ld_cs = ld_cs; a.d_cs = d_cs; a.w_iou = w_iou; a.w_cs = w_cs; a.use_iou = use_iou ? 1 : 0;
    B2M_HIP(hipMemsetAsync(sums, 0, 32 * sizeof(double), st));
    detection_loss_kernel<true><<<(unsigned)cdiv64(S, 256), 256, 0, st>>>(a);
    detection_loss_final_kernel<true><<<1, 1, 0, st>>>(sums, n_fg, n_valid, S, w_off, w_bnd, w_sc, w_sem, sc ? 1 : 0, sem ? 1 : 0,
                                                       LossExFinal{w_iou, w_cs, use_iou ? 1 : 0, cs ? 1 : 0}, result);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// ------------------------------------------------------------------ non-maximum clustering
#define NMC_THREADS 1024
#define NMC_LDS_SORT 4096
#define NMC_MAX_N 262144

__device__ __forceinline__ uint32_t f2ord_u(float f) {
    uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <class P>
__device__ __forceinline__ void bitonic_sort(P keys, int npad) {
    for (int k = 2; k <= npad; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (npad >> 1); t += NMC_THREADS) {
                const int i = ((t / j) * 2 * j) + (t % j), l = i + j;
                const uint64_t a = keys[i], b = keys[l];
                const bool up = (i & k) == 0;
                if ((a > b) == up) { keys[i] = b; keys[l] = a; }
            }
            __syncthreads();
        }
    }
}

// one workgroup clusters the n boxes of one scene
__device__ __forceinline__ void nmc_scene(const float* __restrict__ boxes, int n, float th, int max_k,
                                          int32_t* __restrict__ reps, int32_t* __restrict__ assign,
                                          float* __restrict__ heat, int32_t* __restrict__ k_out,
                                          uint64_t* __restrict__ order, int npad) {
    __shared__ uint64_t skeys[NMC_LDS_SORT];
    __shared__ uint32_t alive[NMC_MAX_N / 32];
    __shared__ int s_first;
    __shared__ float s_box[6];
    const int tid = threadIdx.x;
    const bool in_lds = npad <= NMC_LDS_SORT;

    // ---- visiting order: descending score, ties by ascending row.  (s + 0.0f turns -0.0 into +0.0 -- the two zeros are EQUAL
    // scores, but their bit patterns gave different keys: a +0.0 box was visited before a -0.0 box of a lower row)
    for (int j = tid; j < npad; j += NMC_THREADS) {
        uint64_t key = ~0ull;
        if (j < n) key = ((uint64_t)f2ord_u(-(boxes[(int64_t)j * 7] + 0.0f)) << 32) | (uint32_t)j;
        if (in_lds) skeys[j] = key; else order[j] = key;
    }
    for (int w = tid; w < (n + 31) / 32; w += NMC_THREADS) {
        const int rem = n - w * 32;
        alive[w] = rem >= 32 ? 0xFFFFFFFFu : ((1u << rem) - 1u);
    }
    if (tid == 0) s_first = 0x7FFFFFFF;
    __syncthreads();
    if (in_lds) {
        bitonic_sort(skeys, npad);
        for (int j = tid; j < npad; j += NMC_THREADS) order[j] = skeys[j];
    } else {
        bitonic_sort(order, npad);
    }
    __syncthreads();
    auto ord = [&](int p) -> int { return (int)(uint32_t)(in_lds ? skeys[p] : order[p]); };
    auto is_alive = [&](int j) -> bool { return (alive[j >> 5] >> (j & 31)) & 1u; };

    int kc = 0, p0 = 0;
    for (;;) {
        // ---- next representative: first alive box in visiting order
        int pf;
        for (;;) {
            const int p = p0 + tid;
            if (p < n && is_alive(ord(p))) atomicMin(&s_first, p);
            __syncthreads();
            pf = s_first;
            __syncthreads();                   // every wave has read s_first before any wave publishes the next window
            if (pf != 0x7FFFFFFF || p0 + NMC_THREADS >= n) break;
            p0 += NMC_THREADS;
        }
        if (pf == 0x7FFFFFFF) break;
        const int r = ord(pf);
        if (tid < 6) s_box[tid] = boxes[(int64_t)r * 7 + 1 + tid];
        __syncthreads();                       // s_box visible; everyone has read s_first
        if (tid == 0) { s_first = 0x7FFFFFFF; reps[kc] = r; }
        float rb[6];
#pragma unroll
        for (int u = 0; u < 6; ++u) rb[u] = s_box[u];
        for (int j = tid; j < n; j += NMC_THREADS) {
            float bj[6];
#pragma unroll
            for (int u = 0; u < 6; ++u) bj[u] = boxes[(int64_t)j * 7 + 1 + u];
            float iou = box_iou(rb, bj);
            if (j == r) iou = 1.0f;            // iou_nms.py:90
            if (kc < max_k) heat[(int64_t)kc * n + j] = iou;
            if (is_alive(j) && !(iou <= th)) { // iou_nms.py:97-100 (`<=` keeps the box in `remaining`)
                assign[j] = kc;
                atomicAnd(&alive[j >> 5], ~(1u << (j & 31)));
            }
        }
        ++kc;
        p0 = pf + 1;
        __syncthreads();
    }
    if (tid == 0) *k_out = kc;
}
__global__ __launch_bounds__(NMC_THREADS) void nmc_kernel(const float* __restrict__ boxes, int n, float th, int max_k,
                                                          int32_t* __restrict__ reps, int32_t* __restrict__ assign,
                                                          float* __restrict__ heat, int32_t* __restrict__ k_out,
                                                          uint64_t* __restrict__ order, int npad) {
    nmc_scene(boxes, n, th, max_k, reps, assign, heat, k_out, order, npad);
}
// all scenes of a batch in one launch: workgroup s clusters scene s (descriptor row s = box_off, n, npad, max_k,
// heat_off, order_off; boxes / reps / assign are the per-scene arrays back to back)
#define NMC_DESC 6
__global__ __launch_bounds__(NMC_THREADS) void nmc_batch_kernel(const float* __restrict__ boxes, const int64_t* __restrict__ desc,
                                                                float th, int32_t* __restrict__ reps,
                                                                int32_t* __restrict__ assign, float* __restrict__ heat,
                                                                int32_t* __restrict__ k_out, uint64_t* __restrict__ order) {
    const int64_t* d = desc + (int64_t)blockIdx.x * NMC_DESC;
    const int64_t box_off = d[0];
    const int n = (int)d[1], npad = (int)d[2], max_k = (int)d[3];
    if (n == 0) {
        if (threadIdx.x == 0) k_out[blockIdx.x] = 0;
        return;
    }
    nmc_scene(boxes + box_off * 7, n, th, max_k, reps + box_off, assign + box_off, heat + d[4], k_out + blockIdx.x,
              order + d[5], npad);
}
extern "C" int b2m_nmc_batch(const float* boxes, const int64_t* desc, int32_t n_scenes, int32_t max_n, float cluster_th,
                             int32_t* reps, int32_t* assign, float* heat, int32_t* k_out, uint64_t* order, void* stream) {
    B2M_CHECK_ARG(n_scenes >= 0 && max_n >= 0 && max_n <= NMC_MAX_N, "every scene must have <= 262144 boxes");
    B2M_CHECK_ARG(cluster_th > 0.f && cluster_th < 1.f, "cluster_th must be in (0,1)");   // iou_nms.py:71
    if (n_scenes == 0) return B2M_OK;
    B2M_CHECK_ARG(desc && k_out && (max_n == 0 || (boxes && reps && assign && order)), "NULL argument");
    nmc_batch_kernel<<<(unsigned)n_scenes, NMC_THREADS, 0, (hipStream_t)stream>>>(boxes, desc, cluster_th, reps, assign, heat,
                                                                                  k_out, order);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

extern "C" int b2m_nmc(const float* boxes, int32_t n, float cluster_th, int32_t max_k, int32_t* reps, int32_t* assign,
                       float* heat, int32_t* k_out, uint64_t* order, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(boxes && reps && assign && k_out && order && (heat || max_k == 0), "NULL argument");
    B2M_CHECK_ARG(n >= 0 && n <= NMC_MAX_N, "n must be <= 262144");
    B2M_CHECK_ARG(cluster_th > 0.f && cluster_th < 1.f, "cluster_th must be in (0,1)");   // iou_nms.py:71
    if (n == 0) { B2M_HIP(hipMemsetAsync(k_out, 0, sizeof(int32_t), st)); return B2M_OK; }
    int npad = 1;
    while (npad < n) npad <<= 1;
    if (npad < 2) npad = 2;
    nmc_kernel<<<1, NMC_THREADS, 0, st>>>(boxes, n, cluster_th, max_k, reps, assign, heat, k_out, order, npad);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// ------------------------------------------------------------------ full label histogram of every mask row
// hist[r][c] = |{v in mask r : label[v] == c}|: the prediction x ground-truth-instance intersection counts of
// assign_instances_for_scan (/root/reference/utils/eval_metric.py:316-330), all pairs in one pass over the bits.
#define HIST_MAX 2048
__global__ __launch_bounds__(256) void mask_hist_kernel(const uint64_t* __restrict__ bits, int64_t words,
                                                        const int32_t* __restrict__ label, int64_t n, int n_class,
                                                        int64_t words_per_block, int32_t* __restrict__ hist) {
    __shared__ int h[HIST_MAX];
    const int r = blockIdx.x;
    for (int c = threadIdx.x; c < n_class; c += 256) h[c] = 0;
    __syncthreads();
    const int64_t w0 = (int64_t)blockIdx.y * words_per_block;
    int64_t w1 = w0 + words_per_block;
    if (w1 > words) w1 = words;
    for (int64_t w = w0 + threadIdx.x; w < w1; w += 256) {
        uint64_t m = bits[(int64_t)r * words + w];
        while (m) {
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            const int64_t v = w * 64 + b;
            if (v < n) {
                const int c = label[v];
                if (c >= 0 && c < n_class) atomicAdd(&h[c], 1);
            }
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < n_class; c += 256)
        if (h[c]) atomicAdd(&hist[(int64_t)r * n_class + c], h[c]);
}
extern "C" int b2m_mask_hist(const uint64_t* bits, int64_t words, int32_t k, const int32_t* label, int64_t n,
                             int32_t n_class, int32_t* hist, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(k >= 0 && k <= 65535 && n_class >= 1 && n_class <= HIST_MAX && n >= 0, "bad sizes (n_class <= 2048)");
    if (k == 0) return B2M_OK;
    B2M_CHECK_ARG(bits && label && hist, "NULL argument");
    B2M_HIP(hipMemsetAsync(hist, 0, (size_t)k * n_class * sizeof(int32_t), st));
    if (words == 0) return B2M_OK;
    const int64_t wpb = 2048;
    mask_hist_kernel<<<dim3((unsigned)k, (unsigned)cdiv64(words, wpb)), 256, 0, st>>>(bits, words, label, n, n_class, wpb, hist);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// ------------------------------------------------------------------ bool rows -> bit rows
__global__ __launch_bounds__(256) void mask_pack_kernel(const uint8_t* __restrict__ masks, int64_t n,
                                                        uint64_t* __restrict__ bits, int64_t words) {
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int r = blockIdx.y;
    if (w >= words) return;
    const int64_t v = w * 64 + lane_id();
    const bool bit = v < n && masks[(int64_t)r * n + v] != 0;
    const uint64_t m = __ballot(bit);
    if (lane_id() == 0) bits[(int64_t)r * words + w] = m;
}
extern "C" int b2m_mask_pack(const uint8_t* masks, int32_t k, int64_t n, uint64_t* bits, int64_t words, void* stream) {
    B2M_CHECK_ARG(k >= 0 && k <= 65535 && words == cdiv64(n, 64), "bad sizes");
    if (k == 0 || n == 0) return B2M_OK;
    B2M_CHECK_ARG(masks && bits, "NULL argument");
    mask_pack_kernel<<<dim3((unsigned)cdiv64(words, 4), (unsigned)k), 256, 0, (hipStream_t)stream>>>(masks, n, bits, words);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// ------------------------------------------------------------------ the mask stages: projection, NMS, labels, gather
// detection2mask walks the scenes of a batch (/root/reference/models/detection_net.py:390-477); per scene a stage is a few
// microseconds of work behind a launch (8 scenes: 32 launches).  One launch per stage covers every (scene, instance) row: a
// table of B2M_MASK_DESC int64 fields per scene (include/b2m.h) holds the scene's pointers and sizes, a block finds its scene
// from the running row counts in the table.  Projection, the intersection table and the gather are ONE __device__ body each that
// reads the scene's descriptor at p: *_batch_kernel passes a row of the table, the single-scene kernel of b2m_mask_project /
// b2m_mask_nms / b2m_mask_nms_sweep / b2m_mask_gather its own argument -- the descriptor by value, filled on the host from the
// entry's pointers (fields a stage does not read stay zero).  The greedy walk is one function; the label histogram keeps a
// single-scene kernel of its own.
struct MaskScene {
    const float* heat; int64_t n_fg; const int32_t* sel; int64_t ksel; const int32_t* fg_slot; const int64_t* seg2vox;
    int64_t n_vox; uint64_t* bits; int64_t words; int32_t* inter; int32_t* keep; const int32_t* rows; int64_t kk;
    const int32_t* sem; int32_t* labels; const int64_t* index; int64_t n_pts; uint8_t* out; int64_t row0_sel; int64_t row0_kept;
};
static_assert(sizeof(MaskScene) == B2M_MASK_DESC * 8, "MaskScene must match B2M_MASK_DESC");
// scene of global row r (rows of scene s: [row0, row0 + count)), or -1
__device__ __forceinline__ int scene_of_row(const MaskScene* sc, int n_scenes, int64_t r, bool kept, int64_t& local) {
    for (int s = 0; s < n_scenes; ++s) {
        const int64_t r0 = kept ? sc[s].row0_kept : sc[s].row0_sel, cnt = kept ? sc[s].kk : sc[s].ksel;
        if (r >= r0 && r < r0 + cnt) { local = r - r0; return s; }
    }
    return -1;
}
// ---- heat-maps -> voxel bit masks
// Round 5: a wave owns one 64-voxel word of a scene for ALL of the scene's selected rows -- the voxel's segment and foreground slot
// (seg2vox, fg_slot: 12 bytes per voxel) are read once instead of once per row (PMC: 4.8 x the algorithmic bytes before); lane r
// collects row r's word and the wave writes up to 64 rows' words with one instruction.
__device__ __forceinline__ void mask_project(const MaskScene* __restrict__ p, float th) {
    const MaskScene d = *p;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= d.words || d.ksel == 0) return;
    const int lane = lane_id();
    const int64_t v = w * 64 + lane;
    const int slot = v < d.n_vox ? d.fg_slot[d.seg2vox[v]] : -1;
    for (int64_t r0 = 0; r0 < d.ksel; r0 += 64) {
        const int nr = d.ksel - r0 < 64 ? (int)(d.ksel - r0) : 64;
        uint64_t mine = 0;
        for (int r = 0; r < nr; ++r) {
            const float val = slot >= 0 ? d.heat[(int64_t)d.sel[r0 + r] * d.n_fg + slot] : 0.f;
            const uint64_t m = __ballot(val > th);
            if (lane == r) mine = m;
        }
        if (lane < nr) d.bits[(r0 + lane) * d.words + w] = mine;
    }
}
__global__ __launch_bounds__(256) void mask_project_batch_kernel(const MaskScene* __restrict__ sc, int n_scenes, float th) {
    if ((int)blockIdx.y >= n_scenes) return;
    mask_project(sc + blockIdx.y, th);
}
__global__ __launch_bounds__(256) void mask_project_kernel(MaskScene d, float th) { mask_project(&d, th); }
// ---- mask NMS: intersection table, then the greedy walk
// (sweep: the table is wanted whatever field 10 says -- the sweeps and the single-scene entries write their flags elsewhere)
__device__ __forceinline__ void mask_inter(const MaskScene* __restrict__ p, bool sweep) {
    const MaskScene d = *p;
    const int i = blockIdx.y, j = blockIdx.x, k = (int)d.ksel;
    if (i >= k || j >= k || j < i || (d.keep == nullptr && !sweep)) return;
    __shared__ int wsum[4];
    int s = 0;
    const uint64_t* a = d.bits + (int64_t)i * d.words;
    const uint64_t* b = d.bits + (int64_t)j * d.words;
    for (int64_t w = threadIdx.x; w < d.words; w += 256) s += __popcll(a[w] & b[w]);
#pragma unroll
    for (int e = 32; e > 0; e >>= 1) s += __shfl_down(s, e, 64);
    if (lane_id() == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int t = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        d.inter[(int64_t)i * k + j] = t;
        d.inter[(int64_t)j * k + i] = t;
    }
}
__global__ __launch_bounds__(256) void mask_inter_batch_kernel(const MaskScene* __restrict__ sc, bool sweep) {
    mask_inter(sc + blockIdx.z, sweep);
}
__global__ __launch_bounds__(256) void mask_inter_kernel(MaskScene d) { mask_inter(&d, true); }
// the greedy walk of one workgroup of 256 threads over a k x k intersection table: keep[] doubles as the alive flag (1 = still
// remaining / kept, 0 = suppressed).  Returns the number of kept rows, the same in every thread: all read the same keep[i]
__device__ __forceinline__ int mask_greedy_walk(const int32_t* __restrict__ inter, int k, float th, int32_t* __restrict__ keep) {
    for (int j = threadIdx.x; j < k; j += 256) keep[j] = 1;
    __syncthreads();
    int nk = 0;
    for (int i = 0; i < k; ++i) {
        if (keep[i]) {
            ++nk;
            const int ci = inter[(int64_t)i * k + i];
            for (int j = i + 1 + threadIdx.x; j < k; j += 256) {
                if (!keep[j]) continue;
                const int in = inter[(int64_t)i * k + j];
                const int un = ci + inter[(int64_t)j * k + j] - in;
                const float iou = (float)in / (float)un;         // int64 true-division -> float32 in torch
                if (!(iou <= th)) keep[j] = 0;                   // iou_nms.py:138 keeps `ious <= th`
            }
        }
        __syncthreads();
    }
    return nk;
}
__global__ __launch_bounds__(256) void mask_greedy_batch_kernel(const MaskScene* __restrict__ sc, float th) {
    const MaskScene d = sc[blockIdx.x];
    const int k = (int)d.ksel;
    if (d.keep == nullptr || k == 0) return;
    mask_greedy_walk(d.inter, k, th, d.keep);
}
__global__ __launch_bounds__(256) void mask_greedy_kernel(const int32_t* __restrict__ inter, int k, float th,
                                                          int32_t* __restrict__ keep, int32_t* __restrict__ n_keep) {
    const int nk = mask_greedy_walk(inter, k, th, keep);
    if (threadIdx.x == 0) *n_keep = nk;
}
// ---- per-instance label histogram
// label histogram of a mask row.  A wave reads 64 consecutive words of the bit row at once (512 contiguous bytes) and then
// works only on the non-zero ones, all 64 lanes on the 64 voxels of one word (a coalesced read of their labels): a thread
// per word walked its set bits one by one behind a 4-byte gather each (round 2: 0.42 ms per batch at 16 GB/s).
__global__ __launch_bounds__(256) void label_hist_batch_kernel(const MaskScene* __restrict__ sc, int n_scenes, int n_class) {
    __shared__ int hist[256];
    int64_t r;
    const int s = scene_of_row(sc, n_scenes, blockIdx.x, true, r);
    if (s < 0) return;
    const MaskScene d = sc[s];
    const int64_t row = d.rows ? d.rows[r] : r;
    hist[threadIdx.x] = 0;
    __syncthreads();
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t* brow = d.bits + row * d.words;
    for (int64_t w0 = (int64_t)wave * 64; w0 < d.words; w0 += 256) {
        const uint64_t mine = w0 + lane < d.words ? brow[w0 + lane] : 0ull;
        uint64_t nz = __ballot(mine != 0ull);
        while (nz) {
            const int l = __builtin_ctzll(nz);
            nz &= nz - 1;
            const uint64_t m = (uint64_t)__shfl((long long)mine, l, 64);
            const int64_t v = (w0 + l) * 64 + lane;
            if (((m >> lane) & 1ull) && v < d.n_vox) {
                const int c = d.sem[v];
                if (c >= 0 && c < n_class) atomicAdd(&hist[c], 1);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int best = 0, bc = hist[0];
        for (int c = 1; c < n_class; ++c) if (hist[c] > bc) { bc = hist[c]; best = c; }   // first maximum (np.argmax)
        d.labels[r] = best;
    }
}
// one scene by its pointers: a thread per word walks its set bits.  On ONE scene the wave-per-64-words body above is slower (k rows
// are k workgroups: 55 -> 127 us on a 150 k-voxel scene, 268 -> 467 us for 4 rows over the 1.2 M points of an S3DIS room;
// profiles/single_entry_fold.md section 6), so this stage keeps its single-scene kernel
__global__ __launch_bounds__(256) void label_hist_kernel(const uint64_t* __restrict__ bits, int64_t words,
                                                         const int32_t* __restrict__ rows,
                                                         const int32_t* __restrict__ sem, int64_t n_vox, int n_class,
                                                         int32_t* __restrict__ labels) {
    __shared__ int hist[256];
    const int r = blockIdx.x;
    const int64_t row = rows ? rows[r] : r;
    hist[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t w = threadIdx.x; w < words; w += 256) {
        uint64_t m = bits[row * words + w];
        while (m) {
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            const int64_t v = w * 64 + b;
            if (v < n_vox) {
                const int c = sem[v];
                if (c >= 0 && c < n_class) atomicAdd(&hist[c], 1);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int best = 0, bc = hist[0];
        for (int c = 1; c < n_class; ++c) if (hist[c] > bc) { bc = hist[c]; best = c; }   // first maximum (np.argmax)
        labels[r] = best;
    }
}
// ---- bit rows -> byte masks through an index
// ALL kept rows of a scene: a thread owns four consecutive output points, reads their voxel indices ONCE (a kernel per row
// re-read the 8-byte index for every instance: 99 x 9.6 MB on the benchmark batch) and writes one 4-byte word per row
__device__ __forceinline__ void mask_gather(const MaskScene* __restrict__ p) {
    const MaskScene d = *p;
    const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= d.n_pts || d.kk == 0) return;
    int64_t v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t p = p0 + u < d.n_pts ? p0 + u : d.n_pts - 1;
        v[u] = d.index ? d.index[p] : p;
    }
    const bool whole = p0 + 3 < d.n_pts && ((d.n_pts & 3) == 0);     // the row pitch keeps 4-byte alignment
    for (int64_t r = 0; r < d.kk; ++r) {
        const uint64_t* brow = d.bits + (d.rows ? (int64_t)d.rows[r] : r) * d.words;
        uint32_t w = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) w |= (uint32_t)((brow[v[u] >> 6] >> (v[u] & 63)) & 1ull) << (8 * u);
        uint8_t* o = d.out + r * d.n_pts + p0;
        if (whole) *(uint32_t*)o = w;
        else {
#pragma unroll
            for (int u = 0; u < 4; ++u) if (p0 + u < d.n_pts) o[u] = (uint8_t)(w >> (8 * u));
        }
    }
}
__global__ __launch_bounds__(256) void mask_gather_batch_kernel(const MaskScene* __restrict__ sc) {
    mask_gather(sc + blockIdx.y);
}
__global__ __launch_bounds__(256) void mask_gather_kernel(MaskScene d) { mask_gather(&d); }

// ---- one scene given by its pointers
extern "C" int b2m_mask_project(const float* heat, int32_t n_fg, const int32_t* sel, int32_t ksel,
                                const int32_t* fg_slot, const int64_t* seg2vox, int64_t n_vox, float mask_bin_th,
                                uint64_t* bits, int64_t words, void* stream) {
    B2M_CHECK_ARG(ksel >= 0 && words == cdiv64(n_vox, 64), "bad sizes");
    if (ksel == 0 || n_vox == 0) return B2M_OK;        // no cluster passed the score filter: nothing to project
    B2M_CHECK_ARG(heat && sel && fg_slot && seg2vox && bits && n_fg > 0, "bad arguments");
    MaskScene d{};
    d.heat = heat; d.n_fg = n_fg; d.sel = sel; d.ksel = ksel; d.fg_slot = fg_slot; d.seg2vox = seg2vox; d.n_vox = n_vox;
    d.bits = bits; d.words = words;
    mask_project_kernel<<<(unsigned)cdiv64(words, 4), 256, 0, (hipStream_t)stream>>>(d, mask_bin_th);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}
// the k x k intersection table of one scene's bit rows (b2m_mask_nms, b2m_mask_nms_sweep)
static void mask_inter_launch(const uint64_t* bits, int32_t k, int64_t words, int32_t* inter, hipStream_t st) {
    MaskScene d{};
    d.bits = const_cast<uint64_t*>(bits); d.ksel = k; d.words = words; d.inter = inter;
    mask_inter_kernel<<<dim3((unsigned)k, (unsigned)k), 256, 0, st>>>(d);
}
extern "C" int b2m_mask_nms(const uint64_t* bits, int32_t k, int64_t words, float th, int32_t* inter, int32_t* keep,
                            int32_t* n_keep, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(bits && inter && keep && n_keep && k >= 0 && k <= 65535 && words >= 0, "bad arguments");
    if (k == 0) { B2M_HIP(hipMemsetAsync(n_keep, 0, sizeof(int32_t), st)); return B2M_OK; }
    mask_inter_launch(bits, k, words, inter, st);
    mask_greedy_kernel<<<1, 256, 0, st>>>(inter, k, th, keep, n_keep);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}
extern "C" int b2m_label_hist(const uint64_t* bits, int64_t words, const int32_t* rows, int32_t k, const int32_t* sem,
                              int64_t n_vox, int32_t n_class, int32_t* labels, void* stream) {
    B2M_CHECK_ARG(k >= 0 && n_class >= 1 && n_class <= 256, "bad sizes (n_class <= 256)");
    if (k == 0) return B2M_OK;
    B2M_CHECK_ARG(bits && sem && labels, "NULL argument");
    label_hist_kernel<<<(unsigned)k, 256, 0, (hipStream_t)stream>>>(bits, words, rows, sem, n_vox, n_class, labels);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

extern "C" int b2m_mask_gather(const uint64_t* bits, int64_t words, const int32_t* rows, int32_t k,
                               const int64_t* index, int64_t n_pts, uint8_t* out, void* stream) {
    B2M_CHECK_ARG(k >= 0 && k <= 65535 && n_pts >= 0, "bad sizes");
    if (k == 0 || n_pts == 0) return B2M_OK;            // empty selection: nothing to write (out may be NULL)
    B2M_CHECK_ARG(bits && out, "NULL argument");
    MaskScene d{};
    d.bits = const_cast<uint64_t*>(bits); d.words = words; d.rows = rows; d.kk = k; d.index = index; d.n_pts = n_pts; d.out = out;
    mask_gather_kernel<<<(unsigned)cdiv64(n_pts, 1024), 256, 0, (hipStream_t)stream>>>(d);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}
// ---- all scenes of a batch: the table
extern "C" int b2m_mask_project_batch(const int64_t* desc, int32_t n_scenes, int64_t total_sel, int64_t max_words,
                                      float mask_bin_th, void* stream) {
    B2M_CHECK_ARG(n_scenes >= 0 && total_sel >= 0 && total_sel <= 65535 && max_words >= 0, "bad sizes (at most 65535 rows per batch)");
    if (n_scenes == 0 || total_sel == 0 || max_words == 0) return B2M_OK;
    B2M_CHECK_ARG(desc, "NULL argument");
    mask_project_batch_kernel<<<dim3((unsigned)cdiv64(max_words, 4), (unsigned)n_scenes), 256, 0, (hipStream_t)stream>>>(
        (const MaskScene*)desc, n_scenes, mask_bin_th);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}
extern "C" int b2m_mask_nms_batch(const int64_t* desc, int32_t n_scenes, int32_t max_k, float th, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(n_scenes >= 0 && n_scenes <= 65535 && max_k >= 0 && max_k <= 65535, "bad sizes");
    if (n_scenes == 0 || max_k == 0) return B2M_OK;
    B2M_CHECK_ARG(desc, "NULL argument");
    mask_inter_batch_kernel<<<dim3((unsigned)max_k, (unsigned)max_k, (unsigned)n_scenes), 256, 0, st>>>((const MaskScene*)desc, false);
    mask_greedy_batch_kernel<<<(unsigned)n_scenes, 256, 0, st>>>((const MaskScene*)desc, th);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}
extern "C" int b2m_label_hist_batch(const int64_t* desc, int32_t n_scenes, int64_t total_kept, int32_t n_class, void* stream) {
    B2M_CHECK_ARG(n_scenes >= 0 && total_kept >= 0 && n_class >= 1 && n_class <= 256, "bad sizes (n_class <= 256)");
    if (n_scenes == 0 || total_kept == 0) return B2M_OK;
    B2M_CHECK_ARG(desc, "NULL argument");
    label_hist_batch_kernel<<<(unsigned)total_kept, 256, 0, (hipStream_t)stream>>>((const MaskScene*)desc, n_scenes, n_class);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}
// ---- the same through a voxel-major image of the kept rows (round 5).  mask_gather_batch_kernel looks every (row, point) up in
// the row's bit image: kk x n_pts eight-byte loads for kk x n_pts bytes of output (99 x 2 M on the benchmark batch: 0.19 ms at 13 % of
// the HBM rate the output alone would need).  Transposed once -- word c of voxel v holds the bits of kept rows 64c .. 64c + 63 at v --
// a point needs ONE load per 64 rows, and the kernel is what it looks like: 8 bytes of index and kk bytes of mask per point.
// tbits of a scene: n_vox x nw words, nw = ceil(kk / 64).
__global__ __launch_bounds__(256) void mask_transpose_batch_kernel(const MaskScene* __restrict__ sc, const int64_t* __restrict__ tptr) {
    const MaskScene d = sc[blockIdx.y];
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);       // a wave owns the 64 voxels of bit word w
    if (w >= d.words || d.kk == 0) return;
    const int lane = lane_id();
    uint64_t* tb = (uint64_t*)tptr[blockIdx.y];
    const int nw = (int)((d.kk + 63) >> 6);
    const int64_t v = w * 64 + lane;
    for (int c = 0; c < nw; ++c) {
        const int64_t r = (int64_t)c * 64 + lane;                          // lane r: word w of kept row r
        const uint64_t mine = r < d.kk ? d.bits[(d.rows ? (int64_t)d.rows[r] : r) * d.words + w] : 0ull;
        uint64_t out = 0;                                                  // lane j: bit r = bit j of lane r's word
#pragma unroll 8
        for (int j = 0; j < 64; ++j) {
            const uint64_t m = __ballot((mine >> j) & 1ull);
            if (lane == j) out = m;
        }
        if (v < d.n_vox) tb[v * nw + c] = out;
    }
}
// a thread owns 16 consecutive output points: their voxels' words once per 64 rows, one 16-byte store per row
__global__ __launch_bounds__(256) void mask_gather_t_batch_kernel(const MaskScene* __restrict__ sc, const int64_t* __restrict__ tptr) {
    const MaskScene d = sc[blockIdx.y];
    const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (p0 >= d.n_pts || d.kk == 0) return;
    // (pointers read from the table are generic to hipcc -- flat_load / flat_store; these three are device memory)
    typedef __attribute__((address_space(1))) const uint64_t* gp_u64;
    typedef __attribute__((address_space(1))) const int64_t* gp_i64;
    typedef __attribute__((address_space(1))) uint8_t* gp_u8;
    const gp_u64 tb = (gp_u64)(uintptr_t)tptr[blockIdx.y];
    const gp_i64 index = (gp_i64)(uintptr_t)d.index;
    const gp_u8 outp = (gp_u8)(uintptr_t)d.out;
    const int nw = (int)((d.kk + 63) >> 6);
    int64_t v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int64_t p = p0 + u < d.n_pts ? p0 + u : d.n_pts - 1;
        v[u] = d.index ? index[p] : p;
    }
    // (a row starts wherever r * n_pts falls: the 16-byte store is an UNALIGNED one -- global_store_dwordx4 takes any address in the
    // default access mode, and hipcc emits it for a 16-byte memcpy to a byte pointer)
    const bool whole = p0 + 15 < d.n_pts;
    for (int c = 0; c < nw; ++c) {
        uint64_t t[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) t[u] = tb[v[u] * nw + c];
        const int nr = d.kk - 64 * c < 64 ? (int)(d.kk - 64 * c) : 64;
        for (int r = 0; r < nr; ++r) {
            uint32_t q[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                uint32_t x = 0;
#pragma unroll
                for (int u = 0; u < 4; ++u) x |= (uint32_t)((t[4 * g + u] >> r) & 1ull) << (8 * u);
                q[g] = x;
            }
            gp_u8 o = outp + ((int64_t)c * 64 + r) * d.n_pts + p0;
            if (whole) {
                typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                typedef u32x4 u32x4_unaligned __attribute__((aligned(1)));
                *(__attribute__((address_space(1))) u32x4_unaligned*)o = u32x4{q[0], q[1], q[2], q[3]};
            }
            else {
#pragma unroll
                for (int u = 0; u < 16; ++u) if (p0 + u < d.n_pts) o[u] = (uint8_t)(q[u >> 2] >> (8 * (u & 3)));
            }
        }
    }
}
extern "C" int b2m_mask_gather_batch_t(const int64_t* desc, int32_t n_scenes, int64_t total_kept, int64_t max_pts, int64_t max_words,
                                       const int64_t* tbits, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(n_scenes >= 0 && n_scenes <= 65535 && total_kept >= 0 && max_pts >= 0 && max_words >= 0, "bad sizes");
    if (n_scenes == 0 || total_kept == 0 || max_pts == 0 || max_words == 0) return B2M_OK;
    B2M_CHECK_ARG(desc && tbits, "NULL argument");
    mask_transpose_batch_kernel<<<dim3((unsigned)cdiv64(max_words, 4), (unsigned)n_scenes), 256, 0, st>>>((const MaskScene*)desc, tbits);
    mask_gather_t_batch_kernel<<<dim3((unsigned)cdiv64(max_pts, 4096), (unsigned)n_scenes), 256, 0, st>>>((const MaskScene*)desc, tbits);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}
extern "C" int b2m_mask_gather_batch(const int64_t* desc, int32_t n_scenes, int64_t total_kept, int64_t max_pts, void* stream) {
    B2M_CHECK_ARG(n_scenes >= 0 && n_scenes <= 65535 && total_kept >= 0 && max_pts >= 0, "bad sizes");
    if (n_scenes == 0 || total_kept == 0 || max_pts == 0) return B2M_OK;
    B2M_CHECK_ARG(desc, "NULL argument");
    mask_gather_batch_kernel<<<dim3((unsigned)cdiv64(max_pts, 1024), (unsigned)n_scenes), 256, 0, (hipStream_t)stream>>>(
        (const MaskScene*)desc);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// ------------------------------------------------------------------ threshold sweep (box2mask_amd/param_search.py)
// Evaluater.param_search (/root/reference/models/evaluation.py:353-366) evaluates every mask_nms_th of its grid as a job of its
// own.  The intersection table does not depend on the threshold: it is built once, and workgroup (scene, t) walks it for ths[t].
// Row t is what b2m_mask_nms / b2m_mask_nms_batch write for th = ths[t]: the same division, the same `!(iou <= th)`.
struct SweepThs { float th[B2M_SWEEP_MAX_TH]; };
__global__ __launch_bounds__(256) void mask_greedy_sweep_kernel(const int32_t* __restrict__ inter, int k, SweepThs ths,
                                                                int32_t* __restrict__ keep) {
    mask_greedy_walk(inter, k, ths.th[blockIdx.x], keep + (int64_t)blockIdx.x * k);
}
__global__ __launch_bounds__(256) void mask_greedy_sweep_batch_kernel(const MaskScene* __restrict__ sc, SweepThs ths,
                                                                      int32_t* __restrict__ keep, int64_t total_sel) {
    const MaskScene d = sc[blockIdx.x];
    const int k = (int)d.ksel;
    if (k == 0) return;
    mask_greedy_walk(d.inter, k, ths.th[blockIdx.y], keep + (int64_t)blockIdx.y * total_sel + d.row0_sel);
}
static int sweep_ths(const float* ths_host, int32_t n_th, SweepThs& t) {
    B2M_CHECK_ARG(ths_host && n_th >= 1 && n_th <= B2M_SWEEP_MAX_TH, "1 <= n_th <= 64 thresholds, given on the host");
    for (int i = 0; i < n_th; ++i) t.th[i] = ths_host[i];
    return B2M_OK;
}
extern "C" int b2m_mask_nms_sweep(const uint64_t* bits, int32_t k, int64_t words, const float* ths_host, int32_t n_th,
                                  int32_t* inter, int32_t* keep, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SweepThs t{};
    if (int rc = sweep_ths(ths_host, n_th, t)) return rc;
    B2M_CHECK_ARG(k >= 0 && k <= 65535 && words >= 0, "bad sizes");
    if (k == 0) return B2M_OK;
    B2M_CHECK_ARG(bits && inter && keep, "NULL argument");
    mask_inter_launch(bits, k, words, inter, st);
    mask_greedy_sweep_kernel<<<(unsigned)n_th, 256, 0, st>>>(inter, k, t, keep);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}
extern "C" int b2m_mask_nms_sweep_batch(const int64_t* desc, int32_t n_scenes, int32_t max_k, const float* ths_host, int32_t n_th,
                                        int32_t* keep, int64_t total_sel, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SweepThs t{};
    if (int rc = sweep_ths(ths_host, n_th, t)) return rc;
    B2M_CHECK_ARG(n_scenes >= 0 && n_scenes <= 65535 && max_k >= 0 && max_k <= 65535 && total_sel >= 0, "bad sizes");
    if (n_scenes == 0 || max_k == 0 || total_sel == 0) return B2M_OK;
    B2M_CHECK_ARG(desc && keep, "NULL argument");
    mask_inter_batch_kernel<<<dim3((unsigned)max_k, (unsigned)max_k, (unsigned)n_scenes), 256, 0, st>>>((const MaskScene*)desc, true);
    mask_greedy_sweep_batch_kernel<<<dim3((unsigned)n_scenes, (unsigned)n_th), 256, 0, st>>>((const MaskScene*)desc, t, keep, total_sel);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// ------------------------------------------------------------------ label histogram of every mask row THROUGH an index
// hist[r][c] = |{p < n_pts : bit index[p] of row r set and label[p] == c}|: the prediction x ground-truth counts of
// assign_instances_for_scan on the scene's POINTS, from masks that live on voxels -- b2m_mask_gather, b2m_mask_pack and
// b2m_mask_hist without the k x n_pts bytes in between.  As b2m_mask_gather_batch_t: a voxel-major image first (word c of voxel v =
// rows 64c .. 64c + 63 at v), then one 8-byte look-up per point and 64 rows; every set bit is one integer atomic on the table in
// global memory (k x n_class does not fit LDS at the caps: 65535 x 2048).  Integer sums: the same bits on every run.
struct HistScene {
    const uint64_t* bits; int64_t k; int64_t words; int64_t n_vox; const int64_t* index; const int32_t* label; int64_t n_pts;
    int64_t n_class; uint64_t* tbits; int32_t* hist;
};
static_assert(sizeof(HistScene) == B2M_HIST_DESC * 8, "HistScene must match B2M_HIST_DESC");
// block bx of a scene: zero its share of the table, then transpose the four 64-voxel words it owns
__device__ __forceinline__ void hist_prepare(const HistScene& d, int64_t bx, int64_t nbx) {
    const int64_t cells = d.k * d.n_class;
    for (int64_t e = bx * 256 + threadIdx.x; e < cells; e += nbx * 256) d.hist[e] = 0;
    const int64_t w = bx * 4 + (threadIdx.x >> 6);
    if (w >= d.words) return;
    const int lane = lane_id();
    const int nw = (int)((d.k + 63) >> 6);
    const int64_t v = w * 64 + lane;
    for (int c = 0; c < nw; ++c) {
        const int64_t r = (int64_t)c * 64 + lane;                          // lane r: word w of row r
        const uint64_t mine = r < d.k ? d.bits[r * d.words + w] : 0ull;
        uint64_t out = 0;                                                  // lane j: bit r = bit j of lane r's word
#pragma unroll 8
        for (int j = 0; j < 64; ++j) {
            const uint64_t m = __ballot((mine >> j) & 1ull);
            if (lane == j) out = m;
        }
        if (v < d.n_vox) d.tbits[v * nw + c] = out;
    }
}
// A wave owns 64 consecutive points.  Neighbouring points mostly lie in the same masks and the same ground-truth instance, so their
// adds meet in ONE cell: lane by lane that is 64 atomics on one address (the first form of this kernel: 7.3 ms per launch on 8
// scenes of 1.2 M points, every workgroup queueing on a few hundred cells).  The lanes take their set bits in step; the cells of a
// step are merged inside the wave -- a leader per distinct cell adds the number of lanes that named it.  The whole wave stays in
// the loops (the ballots need every lane); a lane without work carries cell -1.
__device__ __forceinline__ void hist_count(const HistScene& d, int64_t p) {
    const int lane = lane_id();
    bool ok = p < d.n_pts;
    int c = -1;
    int64_t v = 0;
    if (ok) { c = d.label[p]; ok = c >= 0 && c < d.n_class; }
    if (ok) { v = d.index ? d.index[p] : p; ok = v >= 0 && v < d.n_vox; }   // (a point that names no voxel lies in no mask)
    if (!__ballot(ok)) return;
    const int nw = (int)((d.k + 63) >> 6);
    for (int cw = 0; cw < nw; ++cw) {
        uint64_t t = ok ? d.tbits[v * nw + cw] : 0ull;
        while (__ballot(t != 0ull)) {
            int cell = -1;                                                  // k * n_class <= 65535 * 2048 < 2^31
            if (t) {
                cell = (cw * 64 + __builtin_ctzll(t)) * (int)d.n_class + c;
                t &= t - 1;
            }
            uint64_t todo = __ballot(cell >= 0);
            while (todo) {
                const int leader = __builtin_ctzll(todo);
                const int cell0 = __shfl(cell, leader, 64);
                const uint64_t same = __ballot(cell == cell0);
                if (lane == leader) atomicAdd(d.hist + cell0, __popcll(same));
                todo &= ~same;
            }
        }
    }
}
__global__ __launch_bounds__(256) void hist_prepare_kernel(HistScene d) { hist_prepare(d, blockIdx.x, gridDim.x); }
__global__ __launch_bounds__(256) void hist_count_kernel(HistScene d) { hist_count(d, (int64_t)blockIdx.x * 256 + threadIdx.x); }
__global__ __launch_bounds__(256) void hist_prepare_batch_kernel(const HistScene* __restrict__ sc) {
    const HistScene d = sc[blockIdx.y];
    if (d.k == 0) return;
    hist_prepare(d, blockIdx.x, gridDim.x);
}
__global__ __launch_bounds__(256) void hist_count_batch_kernel(const HistScene* __restrict__ sc) {
    const HistScene d = sc[blockIdx.y];
    if (d.k == 0) return;
    hist_count(d, (int64_t)blockIdx.x * 256 + threadIdx.x);
}
extern "C" int b2m_mask_hist_index(const uint64_t* bits, int64_t words, int32_t k, int64_t n_vox, const int64_t* index,
                                   const int32_t* label, int64_t n_pts, int32_t n_class, uint64_t* tbits, int32_t* hist,
                                   void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(k >= 0 && k <= 65535 && n_class >= 1 && n_class <= HIST_MAX, "bad sizes (k <= 65535, n_class <= 2048)");
    B2M_CHECK_ARG(n_vox >= 0 && words == cdiv64(n_vox, 64) && n_pts >= 0 && n_pts <= 0x7FFFFFFF, "bad sizes (words = ceil(n_vox / 64))");
    if (k == 0) return B2M_OK;
    B2M_CHECK_ARG(hist && (n_pts == 0 || label) && (words == 0 || (bits && tbits)), "NULL argument");
    HistScene d{bits, k, words, n_vox, index, label, n_pts, n_class, tbits, hist};
    int64_t nb = cdiv64(words, 4), nz = cdiv64((int64_t)k * n_class, 256);   // blocks of the transposition / of the zero fill
    if (nz > 1024) nz = 1024;                                                // (a block strides over the table)
    if (nb < nz) nb = nz;
    hist_prepare_kernel<<<(unsigned)nb, 256, 0, st>>>(d);
    if (n_pts > 0 && words > 0) hist_count_kernel<<<(unsigned)cdiv64(n_pts, 256), 256, 0, st>>>(d);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}
extern "C" int b2m_mask_hist_index_batch(const int64_t* desc, int32_t n_scenes, int64_t max_words, int64_t max_pts, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(n_scenes >= 0 && n_scenes <= 65535 && max_words >= 0 && max_pts >= 0 && max_pts <= 0x7FFFFFFF, "bad sizes");
    if (n_scenes == 0) return B2M_OK;
    B2M_CHECK_ARG(desc, "NULL argument");
    int64_t nb = cdiv64(max_words, 4);
    if (nb < 256) nb = 256;                                                // (enough blocks for the zero fill of a small scene)
    hist_prepare_batch_kernel<<<dim3((unsigned)nb, (unsigned)n_scenes), 256, 0, st>>>((const HistScene*)desc);
    if (max_pts > 0 && max_words > 0)
        hist_count_batch_kernel<<<dim3((unsigned)cdiv64(max_pts, 256), (unsigned)n_scenes), 256, 0, st>>>((const HistScene*)desc);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}
