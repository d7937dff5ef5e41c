// Oriented-box detection metric of ARKitScenes on the device (include/b2m.h, "detection boxes"): per-mask convex hulls over the
// scene's points, ground-truth box corners, hull x box IoU and the axis-aligned variant.
//
// Replaces, of Evaluater.arkitscenes_eval (/root/reference/models/evaluation.py:245-316): one qhull call per mask over
// positions[mask] (:280-292) and, per (prediction, ground truth) pair, a Python Sutherland-Hodgman clip plus another qhull call
// (utils/box_util.py:19-66, 101-140).  All arithmetic in fp64, evaluated as written (no contraction into fused multiply-adds): the
// clip's intersection formula and the box corners then round as numpy rounds them.
#include "b2m_common.h"
#pragma clang fp contract(off)

#define NDIR 16                      // fan of directions the first pass takes extremes along
#define PART B2M_HULL_PART           // doubles per (row, chunk) record of the first pass:
#define P_BOX 0                      //   0..5 min x,y,z, max x,y,z   6..21 largest dot per direction
#define P_DOT 6                      //   22..53 the (x, y) of the point that has it   54 number of set points
#define P_XY 22
#define P_CNT 54
#define CHUNKS B2M_HULL_CHUNKS
#define HMAX B2M_HULL_MAX
#define LCAP 2048                    // candidates of one row sorted in LDS (above: in the row's global scratch)

// cos / sin of 2 pi d / 16
__constant__ double c_dir[NDIR][2] = {
    {1.0, 0.0}, {0.92387953251128674, 0.38268343236508977}, {0.70710678118654752, 0.70710678118654752},
    {0.38268343236508977, 0.92387953251128674}, {0.0, 1.0}, {-0.38268343236508977, 0.92387953251128674},
    {-0.70710678118654752, 0.70710678118654752}, {-0.92387953251128674, 0.38268343236508977}, {-1.0, 0.0},
    {-0.92387953251128674, -0.38268343236508977}, {-0.70710678118654752, -0.70710678118654752},
    {-0.38268343236508977, -0.92387953251128674}, {0.0, -1.0}, {0.38268343236508977, -0.92387953251128674},
    {0.70710678118654752, -0.70710678118654752}, {0.92387953251128674, -0.38268343236508977}};

// Calls f(p) for every set bit p < n of words [w0, w1) of one bit row.  A wave takes 64 words at a time, skips the zero ones and
// walks a non-zero word with one lane per bit: the 64 points of a word are read as one contiguous 1.5 KB piece of `pos`.
template <class F>
__device__ __forceinline__ void scan_bits(const uint64_t* __restrict__ row, int64_t w0, int64_t w1, int64_t n, F f) {
    const int lane = lane_id();
    for (int64_t base = w0 + (int64_t)(threadIdx.x >> 6) * 64; base < w1; base += 4 * 64) {
        const int64_t w = base + lane;
        const uint64_t mine = w < w1 ? row[w] : 0ull;
        uint64_t nz = __ballot(mine != 0ull);
        while (nz) {
            const int j = __builtin_ctzll(nz);
            nz &= nz - 1;
            const uint64_t word = __shfl(mine, j);
            const int64_t p = (base + j) * 64 + lane;
            if (((word >> lane) & 1ull) && p < n) f(p);
        }
    }
}

// ---- pass 1: count, axis-aligned box and the extreme point along each direction, per (row, chunk of words)
__device__ __forceinline__ void hull_extreme(const uint64_t* __restrict__ bits, int64_t words, const double* __restrict__ pos, int64_t n,
                                             int64_t wpb, int nchunk, double* __restrict__ part, int r, int chunk) {
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int64_t w0 = (int64_t)chunk * wpb;
    int64_t w1 = w0 + wpb;
    if (w1 > words) w1 = words;
    double dot[NDIR];
    int idx[NDIR];
#pragma unroll
    for (int d = 0; d < NDIR; ++d) { dot[d] = -INFINITY; idx[d] = 0x7fffffff; }
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int cnt = 0;
    scan_bits(bits + (int64_t)r * words, w0, w1, n, [&](int64_t p) {
        const double x = pos[3 * p], y = pos[3 * p + 1], z = pos[3 * p + 2];
        ++cnt;
        lo[0] = fmin(lo[0], x); lo[1] = fmin(lo[1], y); lo[2] = fmin(lo[2], z);
        hi[0] = fmax(hi[0], x); hi[1] = fmax(hi[1], y); hi[2] = fmax(hi[2], z);
#pragma unroll
        for (int d = 0; d < NDIR; ++d) {
            const double v = x * c_dir[d][0] + y * c_dir[d][1];
            if (v > dot[d]) { dot[d] = v; idx[d] = (int)p; }          // (a lane meets its points in ascending order)
        }
    });
    // the largest dot, the smallest point index among equals: the same whatever the order of the reduction
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int d = 0; d < NDIR; ++d) {
            const double od = __shfl_xor(dot[d], off);
            const int oi = __shfl_xor(idx[d], off);
            if (od > dot[d] || (od == dot[d] && oi < idx[d])) { dot[d] = od; idx[d] = oi; }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fmin(lo[a], __shfl_xor(lo[a], off));
            hi[a] = fmax(hi[a], __shfl_xor(hi[a], off));
        }
        cnt += __shfl_xor(cnt, off);
    }
    __shared__ double s_dot[4][NDIR], s_box[4][6];
    __shared__ int s_idx[4][NDIR], s_cnt[4];
    if (lane == 0) {
#pragma unroll
        for (int d = 0; d < NDIR; ++d) { s_dot[wave][d] = dot[d]; s_idx[wave][d] = idx[d]; }
#pragma unroll
        for (int a = 0; a < 3; ++a) { s_box[wave][a] = lo[a]; s_box[wave][3 + a] = hi[a]; }
        s_cnt[wave] = cnt;
    }
    __syncthreads();
    double* out = part + ((int64_t)r * nchunk + chunk) * PART;
    const int t = threadIdx.x;
    if (t < NDIR) {
        double bd = s_dot[0][t];
        int bi = s_idx[0][t];
        for (int v = 1; v < 4; ++v)
            if (s_dot[v][t] > bd || (s_dot[v][t] == bd && s_idx[v][t] < bi)) { bd = s_dot[v][t]; bi = s_idx[v][t]; }
        const bool any = bi != 0x7fffffff;
        out[P_DOT + t] = bd;
        out[P_XY + 2 * t] = any ? pos[3 * (int64_t)bi] : 0.0;
        out[P_XY + 2 * t + 1] = any ? pos[3 * (int64_t)bi + 1] : 0.0;
    }
    else if (t >= 64 && t < 70) {
        const int a = t - 64;
        double v = s_box[0][a];
        for (int u = 1; u < 4; ++u) v = a < 3 ? fmin(v, s_box[u][a]) : fmax(v, s_box[u][a]);
        out[P_BOX + a] = v;
    }
    else if (t == 128) out[P_CNT] = (double)(s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]);
}

// ---- pass 2: keep the points that are not strictly inside the polygon of the row's extremes (the only hull candidates)
__device__ __forceinline__ void hull_filter(const uint64_t* __restrict__ bits, int64_t words, const double* __restrict__ pos, int64_t n,
                                            int64_t wpb, int nchunk, const double* __restrict__ part, double* __restrict__ cand,
                                            int32_t cap, int32_t* __restrict__ ncand, int r, int chunk) {
    const int lane = lane_id();
    const int64_t w0 = (int64_t)chunk * wpb;
    int64_t w1 = w0 + wpb;
    if (w1 > words) w1 = words;
    __shared__ double s_x[NDIR], s_y[NDIR], s_px[NDIR + 1], s_py[NDIR + 1];
    __shared__ int s_m;
    const double* pr = part + (int64_t)r * nchunk * PART;
    if (threadIdx.x < NDIR) {
        const int d = threadIdx.x;
        double bd = -INFINITY, bx = 0.0, by = 0.0;
        for (int c = 0; c < nchunk; ++c) {                                // (first chunk among equals: the smallest point index)
            const double v = pr[c * PART + P_DOT + d];
            if (v > bd) { bd = v; bx = pr[c * PART + P_XY + 2 * d]; by = pr[c * PART + P_XY + 2 * d + 1]; }
        }
        s_x[d] = bx; s_y[d] = by;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        // extremes along ascending directions run counter-clockwise round the hull; neighbours often coincide
        int m = 0;
        for (int d = 0; d < NDIR; ++d) {
            if (m > 0 && s_px[m - 1] == s_x[d] && s_py[m - 1] == s_y[d]) continue;
            s_px[m] = s_x[d]; s_py[m] = s_y[d]; ++m;
        }
        if (m > 1 && s_px[m - 1] == s_px[0] && s_py[m - 1] == s_py[0]) --m;
        s_px[m] = s_px[0]; s_py[m] = s_py[0];
        s_m = m;
    }
    __syncthreads();
    const int m = s_m < 3 ? 0 : s_m;                                       // fewer than 3 distinct extremes: every point is kept
    double* crow = cand + (int64_t)r * cap * 2;
    scan_bits(bits + (int64_t)r * words, w0, w1, n, [&](int64_t p) {
        const double x = pos[3 * p], y = pos[3 * p + 1];
        // Strictly to the left of every edge of the closed chain, by more than the rounding error of the test (3 eps of the two
        // products' magnitudes, Shewchuk's bound for this expression): the chain winds round the point, so the point is interior
        // to the hull of the chain's vertices -- input points -- and cannot be on the hull's boundary.
        bool inside = m > 0;
        for (int e = 0; e < m && inside; ++e) {
            const double ax = s_px[e], ay = s_py[e], bx = s_px[e + 1], by = s_py[e + 1];
            const double l = (bx - ax) * (y - ay), q = (by - ay) * (x - ax);
            inside = (l - q) > 8.9e-16 * (fabs(l) + fabs(q));
        }
        const uint64_t keep = __ballot(!inside);                           // (the lanes that reach this point of one word)
        int base = 0;
        const int first = __builtin_ctzll(keep);
        if (!inside) {
            if (lane == first) base = atomicAdd(&ncand[r], __builtin_popcountll(keep));
            base = __shfl(base, first);
            const int slot = base + prefix_popc(keep);
            if (slot < cap) { crow[2 * (int64_t)slot] = x; crow[2 * (int64_t)slot + 1] = y; }
        }
    });
}

__device__ __forceinline__ bool lex_less(double ax, double ay, double bx, double by) { return ax < bx || (ax == bx && ay < by); }

// ---- pass 3: exact hull of the candidates of one row (Andrew's monotone chain over the lexicographically sorted candidates)
__device__ __forceinline__ void hull_exact(const double* __restrict__ part, int nchunk, double* __restrict__ cand, int32_t cap,
                                           const int32_t* __restrict__ ncand, int32_t* __restrict__ stk, int32_t* __restrict__ count,
                                           double* __restrict__ box6, double* __restrict__ hull, int32_t* __restrict__ n_hull,
                                           int32_t* __restrict__ flags, int r) {
    const int t = threadIdx.x;
    __shared__ double s_a[LCAP * 2];
    __shared__ int s_stk[LCAP];
    __shared__ int s_h;
    const double* pr = part + (int64_t)r * nchunk * PART;
    if (t < 6) {
        double v = pr[P_BOX + t];
        for (int c = 1; c < nchunk; ++c) v = t < 3 ? fmin(v, pr[c * PART + P_BOX + t]) : fmax(v, pr[c * PART + P_BOX + t]);
        box6[r * 6 + t] = v;
    }
    if (t == 64) {
        double v = 0.0;
        for (int c = 0; c < nchunk; ++c) v += pr[c * PART + P_CNT];          // (integers below 2^53: exact)
        count[r] = (int32_t)v;
    }
    const int c = ncand[r];
    if (c > cap) {                                                          // the candidate buffer was too small: nothing is reported
        if (t == 0) { n_hull[r] = 0; flags[r] = B2M_HULL_FLAG_CANDIDATES; }
        return;
    }
    if (c == 0) {
        if (t == 0) { n_hull[r] = 0; flags[r] = 0; }
        return;
    }
    int m = 1;
    while (m < c) m <<= 1;                                                  // (cap is a power of two: m <= cap)
    double* grow = cand + (int64_t)r * cap * 2;
    const bool in_lds = m <= LCAP;
    double* a = in_lds ? s_a : grow;
    int* st = in_lds ? s_stk : stk + (int64_t)r * cap;
    for (int i = t; i < m; i += 256) {
        const bool real = i < c;
        if (in_lds) { a[2 * i] = real ? grow[2 * i] : INFINITY; a[2 * i + 1] = real ? grow[2 * i + 1] : INFINITY; }
        else if (!real) { a[2 * i] = INFINITY; a[2 * i + 1] = INFINITY; }
    }
    __syncthreads();
    for (int size = 2; size <= m; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int q = t; q < (m >> 1); q += 256) {
                const int i = ((q / stride) * stride << 1) + (q % stride), j = i + stride;
                const bool up = (i & size) == 0;
                const double ax = a[2 * i], ay = a[2 * i + 1], bx = a[2 * j], by = a[2 * j + 1];
                if (lex_less(bx, by, ax, ay) == up && !(ax == bx && ay == by)) {
                    a[2 * i] = bx; a[2 * i + 1] = by; a[2 * j] = ax; a[2 * j + 1] = ay;
                }
            }
            __syncthreads();
        }
    if (t == 0) {
        auto turn = [&](int o, int p, int q) {
            return (a[2 * p] - a[2 * o]) * (a[2 * q + 1] - a[2 * o + 1]) - (a[2 * p + 1] - a[2 * o + 1]) * (a[2 * q] - a[2 * o]);
        };
        auto same = [&](int p, int q) { return a[2 * p] == a[2 * q] && a[2 * p + 1] == a[2 * q + 1]; };
        int top = 0;
        for (int i = 0; i < c; ++i) {                                       // lower chain, left to right
            if (top > 0 && same(i, st[top - 1])) continue;
            while (top >= 2 && turn(st[top - 2], st[top - 1], i) <= 0.0) --top;
            st[top++] = i;
        }
        int h = 1;
        if (top > 1) {
            const int low = top + 1;
            for (int i = c - 2; i >= 0; --i) {                              // upper chain, right to left, ends on the first point again
                if (same(i, st[top - 1])) continue;
                while (top >= low && turn(st[top - 2], st[top - 1], i) <= 0.0) --top;
                st[top++] = i;
            }
            h = top - 1;
        }
        s_h = h;
        n_hull[r] = h;
        flags[r] = h > HMAX ? B2M_HULL_FLAG_VERTICES : 0;
    }
    __syncthreads();
    const int h = s_h;
    if (h > HMAX) return;                                                   // never a truncated hull
    for (int i = t; i < h; i += 256) {
        hull[((int64_t)r * HMAX + i) * 2] = a[2 * st[i]];
        hull[((int64_t)r * HMAX + i) * 2 + 1] = a[2 * st[i] + 1];
    }
}

__global__ __launch_bounds__(256) void hull_extreme_kernel(const uint64_t* __restrict__ bits, int64_t words, const double* __restrict__ pos,
                                                           int64_t n, int64_t wpb, int nchunk, double* __restrict__ part) {
    hull_extreme(bits, words, pos, n, wpb, nchunk, part, blockIdx.y, blockIdx.x);
}
__global__ __launch_bounds__(256) void hull_filter_kernel(const uint64_t* __restrict__ bits, int64_t words, const double* __restrict__ pos,
                                                          int64_t n, int64_t wpb, int nchunk, const double* __restrict__ part,
                                                          double* __restrict__ cand, int32_t cap, int32_t* __restrict__ ncand) {
    hull_filter(bits, words, pos, n, wpb, nchunk, part, cand, cap, ncand, blockIdx.y, blockIdx.x);
}
__global__ __launch_bounds__(256) void hull_exact_kernel(const double* __restrict__ part, int nchunk, double* __restrict__ cand, int32_t cap,
                                                         const int32_t* __restrict__ ncand, int32_t* __restrict__ stk,
                                                         int32_t* __restrict__ count, double* __restrict__ box6,
                                                         double* __restrict__ hull, int32_t* __restrict__ n_hull,
                                                         int32_t* __restrict__ flags) {
    hull_exact(part, nchunk, cand, cap, ncand, stk, count, box6, hull, n_hull, flags, blockIdx.x);
}

// at most CHUNKS blocks per row, each at least 1024 words (whole groups of 64)
__host__ __device__ __forceinline__ int64_t hull_wpb(int64_t words) {
    const int64_t wpb = (((words + CHUNKS - 1) / CHUNKS + 63) / 64) * 64;
    return wpb < 1024 ? 1024 : wpb;
}
__host__ __device__ __forceinline__ int hull_nchunk(int64_t words) {
    const int64_t wpb = hull_wpb(words);
    return words == 0 ? 1 : (int)((words + wpb - 1) / wpb);
}

extern "C" int b2m_mask_hulls(const uint64_t* bits, int64_t words, int32_t k, const double* pos, int64_t n, double* work, double* cand,
                              int32_t* stk, int32_t cap, int32_t* ncand, int32_t* count, double* box6, double* hull, int32_t* n_hull,
                              int32_t* flags, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(k >= 0 && k <= 65535 && n >= 0 && n < 0x7fffffffll && words >= 0, "bad sizes (k <= 65535, n < 2^31)");
    B2M_CHECK_ARG(words * 64 >= n, "words too small for n points");
    B2M_CHECK_ARG(cap >= 64 && cap <= (1 << 24) && (cap & (cap - 1)) == 0, "cap: a power of two in [64, 2^24]");
    if (k == 0) return B2M_OK;
    B2M_CHECK_ARG(bits && work && cand && stk && ncand && count && box6 && hull && n_hull && flags, "NULL argument");
    B2M_CHECK_ARG(pos || n == 0, "NULL positions");
    const int64_t wpb = hull_wpb(words);
    const int nchunk = hull_nchunk(words);
    B2M_HIP(hipMemsetAsync(ncand, 0, (size_t)k * sizeof(int32_t), st));
    hull_extreme_kernel<<<dim3((unsigned)nchunk, (unsigned)k), 256, 0, st>>>(bits, words, pos, n, wpb, nchunk, work);
    hull_filter_kernel<<<dim3((unsigned)nchunk, (unsigned)k), 256, 0, st>>>(bits, words, pos, n, wpb, nchunk, work, cand, cap, ncand);
    hull_exact_kernel<<<dim3((unsigned)k), 256, 0, st>>>(work, nchunk, cand, cap, ncand, stk, count, box6, hull, n_hull, flags);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// ------------------------------------------------------------------ hulls of masks that live on voxels, asked about on points
// b2m_mask_gather -> b2m_mask_pack -> b2m_mask_hulls without the k x n_pts bytes.  The rows are expanded to POINT bit rows first
// (one bit per point and row: k x n_pts / 8 bytes of scratch) and the three passes above run over those, so point indices, ties,
// chunks and candidates are those of the definition.  Why not a gathering bit source in scan_bits: the passes skip zero words
// 64 at a time and read the 64 points of a set word as one contiguous piece; through the index every one of the three passes would
// walk all n_pts of every row (a row holds a fraction of a percent of the scene) and gather a voxel word per point, three times.
// Here a wave reads the index of its 64 points ONCE for XROWS rows and gathers from voxel rows of a few KB that stay in L2; the
// ballot of the 64 lanes is the point word.
struct HullScene {
    const uint64_t* bits; int64_t k; int64_t words; int64_t n_vox; const int64_t* index; const double* pos; int64_t n_pts;
    uint64_t* pbits; double* work; double* cand; int32_t* stk; int32_t* ncand; int32_t* count; double* box6; double* hull;
    int32_t* n_hull; int32_t* flags;
};
static_assert(sizeof(HullScene) == B2M_HULLIDX_DESC * 8, "HullScene must match B2M_HULLIDX_DESC");
#define XROWS 16                     // rows per block of the expansion
// block (bx, by) of a scene: point words 4 bx .. 4 bx + 3 of rows XROWS by .. ; the blocks of bx = 0 zero ncand of their rows
__device__ __forceinline__ void hull_expand(const HullScene& d, int64_t bx, int by) {
    const int lane = lane_id();
    const int64_t r0 = (int64_t)by * XROWS;
    const int64_t r1 = r0 + XROWS < d.k ? r0 + XROWS : d.k;
    if (bx == 0 && r0 + threadIdx.x < r1) d.ncand[r0 + threadIdx.x] = 0;
    const int64_t pw = (d.n_pts + 63) >> 6;
    const int64_t w = bx * 4 + (threadIdx.x >> 6);
    if (w >= pw) return;                                                    // (whole waves)
    const int64_t p = w * 64 + lane;
    int64_t v = -1;
    if (p < d.n_pts) v = d.index ? d.index[p] : p;
    const bool ok = v >= 0 && v < d.n_vox;                                  // (a point that names no voxel lies in no mask)
    const int64_t vw = ok ? v >> 6 : 0;
    const int sh = (int)(v & 63);
    for (int64_t r = r0; r < r1; ++r) {
        const bool bit = ok && ((d.bits[r * d.words + vw] >> sh) & 1ull);
        const uint64_t m = __ballot(bit);
        if (lane == 0) d.pbits[r * pw + w] = m;
    }
}
__global__ __launch_bounds__(256) void hull_expand_kernel(HullScene d) { hull_expand(d, blockIdx.x, blockIdx.y); }
__global__ __launch_bounds__(256) void hull_expand_batch_kernel(const HullScene* __restrict__ sc) {
    const HullScene d = sc[blockIdx.z];
    if ((int64_t)blockIdx.y * XROWS >= d.k) return;
    hull_expand(d, blockIdx.x, blockIdx.y);
}
__global__ __launch_bounds__(256) void hull_extreme_batch_kernel(const HullScene* __restrict__ sc) {
    const HullScene d = sc[blockIdx.z];
    const int64_t pw = (d.n_pts + 63) >> 6;
    const int nchunk = hull_nchunk(pw);
    if (blockIdx.y >= d.k || (int)blockIdx.x >= nchunk) return;
    hull_extreme(d.pbits, pw, d.pos, d.n_pts, hull_wpb(pw), nchunk, d.work, blockIdx.y, blockIdx.x);
}
__global__ __launch_bounds__(256) void hull_filter_batch_kernel(const HullScene* __restrict__ sc, int32_t cap) {
    const HullScene d = sc[blockIdx.z];
    const int64_t pw = (d.n_pts + 63) >> 6;
    const int nchunk = hull_nchunk(pw);
    if (blockIdx.y >= d.k || (int)blockIdx.x >= nchunk) return;
    hull_filter(d.pbits, pw, d.pos, d.n_pts, hull_wpb(pw), nchunk, d.work, d.cand, cap, d.ncand, blockIdx.y, blockIdx.x);
}
__global__ __launch_bounds__(256) void hull_exact_batch_kernel(const HullScene* __restrict__ sc, int32_t cap) {
    const HullScene d = sc[blockIdx.y];
    if (blockIdx.x >= d.k) return;
    hull_exact(d.work, hull_nchunk((d.n_pts + 63) >> 6), d.cand, cap, d.ncand, d.stk, d.count, d.box6, d.hull, d.n_hull, d.flags,
               blockIdx.x);
}
extern "C" int b2m_mask_hulls_index(const uint64_t* bits, int64_t words, int32_t k, int64_t n_vox, const int64_t* index, const double* pos,
                                    int64_t n_pts, uint64_t* pbits, double* work, double* cand, int32_t* stk, int32_t cap, int32_t* ncand,
                                    int32_t* count, double* box6, double* hull, int32_t* n_hull, int32_t* flags, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(k >= 0 && k <= 65535 && n_pts >= 0 && n_pts < 0x7fffffffll, "bad sizes (k <= 65535, n_pts < 2^31)");
    B2M_CHECK_ARG(n_vox >= 0 && words == cdiv64(n_vox, 64), "bad sizes (words = ceil(n_vox / 64))");
    B2M_CHECK_ARG(cap >= 64 && cap <= (1 << 24) && (cap & (cap - 1)) == 0, "cap: a power of two in [64, 2^24]");
    if (k == 0) return B2M_OK;
    B2M_CHECK_ARG(work && cand && stk && ncand && count && box6 && hull && n_hull && flags, "NULL argument");
    B2M_CHECK_ARG((bits || words == 0) && ((pos && pbits) || n_pts == 0), "NULL argument");
    const HullScene d{bits, k, words, n_vox, index, pos, n_pts, pbits, work, cand, stk, ncand, count, box6, hull, n_hull, flags};
    const int64_t pw = cdiv64(n_pts, 64);
    const int64_t wpb = hull_wpb(pw);
    const int nchunk = hull_nchunk(pw);
    const int64_t xb = pw == 0 ? 1 : cdiv64(pw, 4);
    hull_expand_kernel<<<dim3((unsigned)xb, (unsigned)cdiv64(k, XROWS)), 256, 0, st>>>(d);
    hull_extreme_kernel<<<dim3((unsigned)nchunk, (unsigned)k), 256, 0, st>>>(pbits, pw, pos, n_pts, wpb, nchunk, work);
    hull_filter_kernel<<<dim3((unsigned)nchunk, (unsigned)k), 256, 0, st>>>(pbits, pw, pos, n_pts, wpb, nchunk, work, cand, cap, ncand);
    hull_exact_kernel<<<dim3((unsigned)k), 256, 0, st>>>(work, nchunk, cand, cap, ncand, stk, count, box6, hull, n_hull, flags);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}
extern "C" int b2m_mask_hulls_index_batch(const int64_t* desc, int32_t n_scenes, int32_t cap, int32_t max_k, int64_t max_pts,
                                          void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(n_scenes >= 0 && n_scenes <= 65535 && max_k >= 0 && max_k <= 65535 && max_pts >= 0 && max_pts < 0x7fffffffll,
                  "bad sizes (n_scenes, max_k <= 65535, max_pts < 2^31)");
    B2M_CHECK_ARG(cap >= 64 && cap <= (1 << 24) && (cap & (cap - 1)) == 0, "cap: a power of two in [64, 2^24]");
    if (n_scenes == 0 || max_k == 0) return B2M_OK;
    B2M_CHECK_ARG(desc, "NULL argument");
    const HullScene* sc = (const HullScene*)desc;
    const int64_t pw = cdiv64(max_pts, 64);
    // the chunks of a scene are not monotone in its size (32 of 1024 words, then 31 of 1088): a bound for every size up to pw
    int nchunk = pw == 0 ? 1 : (int)cdiv64(pw, 1024);
    if (nchunk > CHUNKS) nchunk = CHUNKS;
    const int64_t xb = pw == 0 ? 1 : cdiv64(pw, 4);
    hull_expand_batch_kernel<<<dim3((unsigned)xb, (unsigned)cdiv64(max_k, XROWS), (unsigned)n_scenes), 256, 0, st>>>(sc);
    hull_extreme_batch_kernel<<<dim3((unsigned)nchunk, (unsigned)max_k, (unsigned)n_scenes), 256, 0, st>>>(sc);
    hull_filter_batch_kernel<<<dim3((unsigned)nchunk, (unsigned)max_k, (unsigned)n_scenes), 256, 0, st>>>(sc, cap);
    hull_exact_batch_kernel<<<dim3((unsigned)max_k, (unsigned)n_scenes), 256, 0, st>>>(sc, cap);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// ------------------------------------------------------------------ ground-truth boxes
// get_oriented_corners / box3d_vol / get_rotated_bounds of utils/box_util.py for one box per thread; R = reshape(rot, 3, 3).T
__global__ __launch_bounds__(64) void obb_corners_kernel(const double* __restrict__ centers, const double* __restrict__ bounds,
                                                         const double* __restrict__ rot, int g, double* __restrict__ out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= g) return;
    const double b[3] = {bounds[3 * i], bounds[3 * i + 1], bounds[3 * i + 2]};
    const double* q = rot + 9 * (int64_t)i;
    // corner order of get_oriented_corners: 000 100 110 010 001 101 111 011 (x y z signs)
    const int sx[8] = {-1, 1, 1, -1, -1, 1, 1, -1}, sy[8] = {-1, -1, 1, 1, -1, -1, 1, 1}, sz[8] = {-1, -1, -1, -1, 1, 1, 1, 1};
    double c[8][3], ext[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        const double p[3] = {sx[v] * b[0], sy[v] * b[1], sz[v] * b[2]};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double rv = q[a] * p[0] + q[3 + a] * p[1] + q[6 + a] * p[2];   // row a of the transposed matrix
            ext[a] = rv > ext[a] ? rv : ext[a];                                 // get_rotated_bounds: the largest coordinate, from 0
            c[v][a] = rv + centers[3 * i + a];
        }
    }
    auto dist = [&](int u, int v) {
        const double dx = c[u][0] - c[v][0], dy = c[u][1] - c[v][1], dz = c[u][2] - c[v][2];
        return sqrt(dx * dx + dy * dy + dz * dz);
    };
    double* o = out + (int64_t)i * B2M_OBB_REC;
#pragma unroll
    for (int v = 0; v < 4; ++v) { o[2 * v] = c[v][0]; o[2 * v + 1] = c[v][1]; }
    o[8] = c[0][2];
    o[9] = c[7][2];
    o[10] = dist(0, 1) * dist(1, 2) * dist(0, 4);
    o[11] = ext[0] * 2.0; o[12] = ext[1] * 2.0; o[13] = ext[2] * 2.0;
    o[14] = 0.0; o[15] = 0.0;
}
extern "C" int b2m_obb_corners(const double* centers, const double* bounds, const double* rotations, int32_t g, double* boxes,
                               void* stream) {
    B2M_CHECK_ARG(g >= 0, "g < 0");
    if (g == 0) return B2M_OK;
    B2M_CHECK_ARG(centers && bounds && rotations && boxes, "NULL argument");
    obb_corners_kernel<<<dim3((unsigned)cdiv64(g, 64)), 64, 0, (hipStream_t)stream>>>(centers, bounds, rotations, g, boxes);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// ------------------------------------------------------------------ hull x oriented box IoU (box3d_iou, utils/box_util.py:101-140)
#define PCAP (HMAX + 4)
// sum over the polygon's edges of the cross products, relative to its first vertex (twice the signed area), over the wave
__device__ __forceinline__ double wave_shoelace(const double* p, int n) {
    const int lane = lane_id();
    double s = 0.0;
    const double ox = p[0], oy = p[1];
    for (int i = lane; i < n; i += 64) {
        const int j = i + 1 < n ? i + 1 : 0;
        s += (p[2 * i] - ox) * (p[2 * j + 1] - oy) - (p[2 * j] - ox) * (p[2 * i + 1] - oy);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
}
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// One (hull row, box) pair per wave.  Sutherland-Hodgman with the lanes over the subject's vertices: lane i looks at the edge
// (vertex i-1 -> vertex i) and emits what polygon_clip appends for it -- the crossing, then the vertex if it is inside -- at the
// position a wave prefix count gives, so the output is polygon_clip's list in polygon_clip's order.
__global__ __launch_bounds__(128) void hull_box_iou_kernel(const double* __restrict__ hull, const int32_t* __restrict__ n_hull,
                                                           const double* __restrict__ box6, const int32_t* __restrict__ pcls, int k,
                                                           const double* __restrict__ gbox, const int32_t* __restrict__ gcls, int g,
                                                           double* __restrict__ out) {
    __shared__ double s_poly[2][2][PCAP * 2];
    const int wave = threadIdx.x >> 6, lane = lane_id();
    const int64_t pair = (int64_t)blockIdx.x * 2 + wave;
    if (pair >= (int64_t)k * g) return;
    const int r = (int)(pair / g), b = (int)(pair % g);
    double iou = 0.0;
    int n = n_hull[r];
    const double* o = gbox + (int64_t)b * B2M_OBB_REC;
    // rectangle corners 0..3 must run counter-clockwise: with the clip's `inside` a clockwise one keeps nothing, as in the reference
    const double rect2 = (o[2] - o[0]) * (o[5] - o[1]) - (o[4] - o[0]) * (o[3] - o[1]);
    if (pcls[r] >= 0 && pcls[r] == gcls[b] && n >= 3 && n <= HMAX && rect2 > 0.0) {
        double* in = s_poly[wave][0];
        double* nx = s_poly[wave][1];
        for (int i = lane; i < n; i += 64) {
            in[2 * i] = hull[((int64_t)r * HMAX + i) * 2];
            in[2 * i + 1] = hull[((int64_t)r * HMAX + i) * 2 + 1];
        }
        wave_lds_sync();
        const double area1 = 0.5 * fabs(wave_shoelace(in, n));
        for (int e = 0; e < 4 && n > 0; ++e) {
            const int e0 = (e + 3) & 3;
            const double c1x = o[2 * e0], c1y = o[2 * e0 + 1], c2x = o[2 * e], c2y = o[2 * e + 1];
            int outn = 0;
            for (int base = 0; base < n; base += 64) {
                const int i = base + lane;
                const bool valid = i < n;
                const int ii = valid ? i : 0, ss = ii == 0 ? n - 1 : ii - 1;
                const double ex = in[2 * ii], ey = in[2 * ii + 1], sx = in[2 * ss], sy = in[2 * ss + 1];
                const bool in_e = (c2x - c1x) * (ey - c1y) > (c2y - c1y) * (ex - c1x);
                const bool in_s = (c2x - c1x) * (sy - c1y) > (c2y - c1y) * (sx - c1x);
                const bool f_i = valid && in_e != in_s, f_e = valid && in_e;
                const uint64_t b_i = __ballot(f_i), b_e = __ballot(f_e);
                const int at = outn + prefix_popc(b_i) + prefix_popc(b_e);
                if (f_i && at < PCAP) {                                           // computeIntersection, box_util.py:34-40
                    const double dcx = c1x - c2x, dcy = c1y - c2y, dpx = sx - ex, dpy = sy - ey;
                    const double n1 = c1x * c2y - c1y * c2x, n2 = sx * ey - sy * ex, n3 = 1.0 / (dcx * dpy - dcy * dpx);
                    nx[2 * at] = (n1 * dpx - n2 * dcx) * n3;
                    nx[2 * at + 1] = (n1 * dpy - n2 * dcy) * n3;
                }
                if (f_e && at + (int)f_i < PCAP) { nx[2 * (at + f_i)] = ex; nx[2 * (at + f_i) + 1] = ey; }
                outn += __builtin_popcountll(b_i) + __builtin_popcountll(b_e);
            }
            wave_lds_sync();
            n = outn < PCAP ? outn : PCAP;            // (a convex subject gains at most one vertex per clip edge: never reached)
            double* tmp = in; in = nx; nx = tmp;
        }
        if (n >= 3) {
            const double inter = 0.5 * fabs(wave_shoelace(in, n));
            const double zlo = box6[r * 6 + 2], zhi = box6[r * 6 + 5];
            const double zmax = fmin(zhi, o[9]), zmin = fmax(zlo, o[8]);
            const double inter_vol = inter * fmax(0.0, zmax - zmin);
            const double vol1 = area1 * (zhi - zlo), vol2 = o[10];
            iou = inter_vol / (vol1 + vol2 - inter_vol);
        }
    }
    if (lane == 0) out[pair] = iou;
}
extern "C" int b2m_hull_box_iou(const double* hull, const int32_t* n_hull, const double* box6, const int32_t* pcls, int32_t k,
                                const double* boxes, const int32_t* gcls, int32_t g, double* iou, void* stream) {
    B2M_CHECK_ARG(k >= 0 && g >= 0 && (int64_t)k * g < (1ll << 31), "bad sizes");
    if (k == 0 || g == 0) return B2M_OK;
    B2M_CHECK_ARG(hull && n_hull && box6 && pcls && boxes && gcls && iou, "NULL argument");
    hull_box_iou_kernel<<<dim3((unsigned)cdiv64((int64_t)k * g, 2)), 128, 0, (hipStream_t)stream>>>(hull, n_hull, box6, pcls, k, boxes,
                                                                                                   gcls, g, iou);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// ------------------------------------------------------------------ axis-aligned variant (calc_iou, utils/metric_util.py:91-113)
__global__ __launch_bounds__(256) void aabb_iou_kernel(const double* __restrict__ box6, const int32_t* __restrict__ pcls, int k,
                                                       const double* __restrict__ gcenter, const double* __restrict__ gbox,
                                                       const int32_t* __restrict__ gcls, int g, double* __restrict__ out) {
    const int64_t pair = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pair >= (int64_t)k * g) return;
    const int r = (int)(pair / g), b = (int)(pair % g);
    double iou = 0.0;
    if (pcls[r] >= 0 && pcls[r] == gcls[b]) {
        bool all = true;
        double inter = 1.0, va = 1.0, vb = 1.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double lo = box6[r * 6 + a], hi = box6[r * 6 + 3 + a];
            const double ca = (lo + hi) / 2.0, sa = hi - lo;                      // evaluation.py:295-297
            const double cb = gcenter[3 * b + a], sb = gbox[(int64_t)b * B2M_OBB_REC + 11 + a];
            const double min_max = fmin(ca + sa / 2, cb + sb / 2), max_min = fmax(ca - sa / 2, cb - sb / 2);
            all = all && min_max > max_min;
            inter *= min_max - max_min;
            va *= sa; vb *= sb;
        }
        if (all) iou = 1.0 * inter / (va + vb - inter);
    }
    out[pair] = iou;
}
extern "C" int b2m_aabb_iou(const double* box6, const int32_t* pcls, int32_t k, const double* gcenters, const double* boxes,
                            const int32_t* gcls, int32_t g, double* iou, void* stream) {
    B2M_CHECK_ARG(k >= 0 && g >= 0 && (int64_t)k * g < (1ll << 31), "bad sizes");
    if (k == 0 || g == 0) return B2M_OK;
    B2M_CHECK_ARG(box6 && pcls && gcenters && boxes && gcls && iou, "NULL argument");
    aabb_iou_kernel<<<dim3((unsigned)cdiv64((int64_t)k * g, 256)), 256, 0, (hipStream_t)stream>>>(box6, pcls, k, gcenters, boxes, gcls, g,
                                                                                                 iou);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}
