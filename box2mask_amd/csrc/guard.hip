// Overflow guard of half-precision training (box2mask_amd/half_guard.py): the largest magnitude, as BITS, of a binary16 matrix or
// an fp32 array, maximised into one word.  Magnitude bits order as unsigned integers -- finite < 65504 (0x7bff) < inf (0x7c00) <
// every NaN -- so the one word says how large the largest gradient was, whether something was clipped to 65504 by the
// convolution's epilogue, and whether anything is not finite.  The kernels only READ what the training kernels wrote.
//
// Shape of both reductions: 16-byte loads where the address allows them (scalar head and tail), maximum in registers, across the
// wave with shuffles, across the waves through LDS, ONE atomicMax per workgroup (and none for a workgroup that saw only zeros).
#include "b2m_common.h"

#define GUARD_THREADS 256
#define GUARD_MAX_BLOCKS 2048          // 8 workgroups of 4 waves per CU: the grid is clamped, the threads stride

__device__ __forceinline__ uint32_t guard_wave_max(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        uint32_t o = (uint32_t)__shfl_xor((int)v, off);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ void guard_block_max(uint32_t v, uint32_t* __restrict__ out) {
    __shared__ uint32_t part[GUARD_THREADS / 64];
    v = guard_wave_max(v);
    if (lane_id() == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < GUARD_THREADS / 64; ++w) v = part[w] > v ? part[w] : v;
        if (v != 0) atomicMax(out, v);            // (max(*out, 0) == *out)
    }
}

__device__ __forceinline__ uint32_t guard_max2(uint32_t a, uint32_t b) { return a > b ? a : b; }

// the larger of the two binary16 magnitudes packed in one dword
__device__ __forceinline__ uint32_t guard_h2(uint32_t w) { return guard_max2(w & 0x7fffu, (w >> 16) & 0x7fffu); }

__device__ __forceinline__ uint32_t guard_h8(uint4 q) {
    return guard_max2(guard_max2(guard_h2(q.x), guard_h2(q.y)), guard_max2(guard_h2(q.z), guard_h2(q.w)));
}

// One work item = one SLOT of one row; a row has `slots` = ceil(c / 8) + 1 of them.  With h = the number of elements in front of
// the row's first 16-byte boundary (0 ... 7, at most c): slot 0 reads those h elements one by one; slot j >= 1 covers elements
// [h + 8 (j - 1), h + 8 j) -- one 16-byte load when all eight lie inside the row, else the remaining ones one by one.  Nothing at
// column >= c is read.  A matrix without padding (ld == c) arrives here as ONE row of n * c elements (the host entry folds it).
__global__ void __launch_bounds__(GUARD_THREADS)
half_absmax_kernel(const uint16_t* __restrict__ x, int64_t ld, int32_t n_items, int32_t c, int32_t slots, uint32_t* __restrict__ out) {
    uint32_t m = 0;
    const int32_t stride = (int32_t)(gridDim.x * GUARD_THREADS);
    // (n_items < 2^31 - GUARD_MAX_BLOCKS * GUARD_THREADS: the host entry sees to it, so i + stride does not wrap)
    for (int32_t i = (int32_t)(blockIdx.x * GUARD_THREADS + threadIdx.x); i < n_items; i += stride) {
        const int32_t r = i / slots, j = i - r * slots;
        const uint16_t* row = x + (int64_t)r * ld;
        int32_t h = (int32_t)((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u) >> 1;
        h = h < c ? h : c;
        if (j == 0) {
            for (int32_t k = 0; k < h; ++k) m = guard_max2(m, row[k] & 0x7fffu);
        } else {
            const int32_t e0 = h + 8 * (j - 1);
            if (e0 + 8 <= c) {
                m = guard_max2(m, guard_h8(*reinterpret_cast<const uint4*>(row + e0)));
            } else {
                for (int32_t k = e0; k < c; ++k) m = guard_max2(m, row[k] & 0x7fffu);
            }
        }
    }
    guard_block_max(m, out);
}

__device__ __forceinline__ uint32_t guard_f4(uint4 q) {
    return guard_max2(guard_max2(q.x & 0x7fffffffu, q.y & 0x7fffffffu), guard_max2(q.z & 0x7fffffffu, q.w & 0x7fffffffu));
}

// g[0 ... head) and g[head + 4 nvec ... n) one by one (at most 3 each), the nvec 16-byte groups in between with four loads in
// flight per thread
__global__ void __launch_bounds__(GUARD_THREADS)
f32_absmax_kernel(const uint32_t* __restrict__ g, int64_t n, int32_t head, int64_t nvec, uint32_t* __restrict__ out) {
    uint32_t m = 0;
    const int64_t t = (int64_t)blockIdx.x * GUARD_THREADS + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * GUARD_THREADS;
    const uint4* v = reinterpret_cast<const uint4*>(g + head);
    int64_t i = t;
    for (; i + 3 * stride < nvec; i += 4 * stride) {
        const uint4 a = v[i], b = v[i + stride], c = v[i + 2 * stride], d = v[i + 3 * stride];
        m = guard_max2(m, guard_max2(guard_max2(guard_f4(a), guard_f4(b)), guard_max2(guard_f4(c), guard_f4(d))));
    }
    for (; i < nvec; i += stride) m = guard_max2(m, guard_f4(v[i]));
    if (t < head) m = guard_max2(m, g[t] & 0x7fffffffu);
    const int64_t tail = (int64_t)head + 4 * nvec + t;
    if (t < 4 && tail < n) m = guard_max2(m, g[tail] & 0x7fffffffu);
    guard_block_max(m, out);
}

__global__ void guard_finish_kernel(const uint32_t* __restrict__ flags, float* __restrict__ found_inf, uint32_t* __restrict__ counters) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const bool found = flags[0] >= 0x7bffu || flags[1] >= 0x7f800000u;
    *found_inf = found ? 1.0f : 0.0f;
    counters[0] += 1u;
    if (found) counters[1] += 1u;
}

static inline int guard_grid(int64_t items) {
    int64_t b = cdiv64(items, GUARD_THREADS);
    return (int)(b < GUARD_MAX_BLOCKS ? b : GUARD_MAX_BLOCKS);
}

extern "C" int b2m_half_absmax(const void* x, int64_t ld, int64_t n, int32_t c, uint32_t* out, void* stream) {
    B2M_CHECK_ARG(out != nullptr, "out is NULL");
    B2M_CHECK_ARG(((uintptr_t)out & 3u) == 0, "out is not 4-byte aligned");
    B2M_CHECK_ARG(n >= 0 && c >= 0, "negative size");
    B2M_CHECK_ARG(ld >= c, "ld < c");
    if (n == 0 || c == 0) return B2M_OK;
    B2M_CHECK_ARG(x != nullptr, "x is NULL");
    B2M_CHECK_ARG(((uintptr_t)x & 1u) == 0, "x is not 2-byte aligned");
    // the kernel counts its work items (slots of rows) in 32 bits
    const int64_t limit = ((int64_t)1 << 31) - (int64_t)GUARD_MAX_BLOCKS * GUARD_THREADS;
    B2M_CHECK_ARG(ld < ((int64_t)1 << 31) && n <= limit / ld, "n * ld is beyond the 32-bit range of the kernel's indices");
    int64_t rows = n, cols = c, pitch = ld;
    if (ld == c) {                       // no padding: one row of n * c elements, one head and one tail in all
        cols = n * c; rows = 1; pitch = cols;
    }
    const int64_t slots = cdiv64(cols, 8) + 1;
    B2M_CHECK_ARG(rows <= limit / slots, "n * ld is beyond the 32-bit range of the kernel's indices");
    const int64_t items = rows * slots;
    half_absmax_kernel<<<guard_grid(items), GUARD_THREADS, 0, (hipStream_t)stream>>>((const uint16_t*)x, pitch, (int32_t)items,
                                                                                     (int32_t)cols, (int32_t)slots, out);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

extern "C" int b2m_f32_absmax(const float* g, int64_t n, uint32_t* out, void* stream) {
    B2M_CHECK_ARG(out != nullptr, "out is NULL");
    B2M_CHECK_ARG(((uintptr_t)out & 3u) == 0, "out is not 4-byte aligned");
    B2M_CHECK_ARG(n >= 0, "negative size");
    if (n == 0) return B2M_OK;
    B2M_CHECK_ARG(g != nullptr, "g is NULL");
    B2M_CHECK_ARG(((uintptr_t)g & 3u) == 0, "g is not 4-byte aligned");
    int64_t head = (int64_t)(((16u - (uint32_t)((uintptr_t)g & 15u)) & 15u) >> 2);
    head = head < n ? head : n;
    const int64_t nvec = (n - head) / 4;
    // at least the 4 threads that read the head and the tail
    const int64_t items = nvec > 4 ? nvec : 4;
    f32_absmax_kernel<<<guard_grid(items), GUARD_THREADS, 0, (hipStream_t)stream>>>((const uint32_t*)g, n, (int32_t)head, nvec, out);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

extern "C" int b2m_guard_finish(const uint32_t* flags, float* found_inf, uint32_t* counters, void* stream) {
    B2M_CHECK_ARG(flags != nullptr, "flags is NULL");
    B2M_CHECK_ARG(found_inf != nullptr, "found_inf is NULL");
    B2M_CHECK_ARG(counters != nullptr, "counters is NULL");
    B2M_CHECK_ARG((((uintptr_t)flags | (uintptr_t)found_inf | (uintptr_t)counters) & 3u) == 0, "an argument is not 4-byte aligned");
    guard_finish_kernel<<<1, 64, 0, (hipStream_t)stream>>>(flags, found_inf, counters);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}
