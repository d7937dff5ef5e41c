// Row-wise cross entropy for the per-voxel semantics head (the reference's models/model.py:212-223): loss, "pessimistic"
// accuracy (hits / all rows), predicted class per row and the dense gradient, for up to ~10^6 rows of n_class logits.
// The arithmetic is the semantics block of detection_loss_kernel (nms.hip): max-subtracted, fp64 exponentials and sums, labels
// outside [0, n_class) ignored.  What differs is the shape of the work:
//   * a workgroup owns 256 consecutive rows.  Their 256 x n_class logits are one contiguous run of floats (pitch == n_class) or
//     256 runs of n_class floats: consecutive lanes load consecutive floats of it into LDS, each thread then works through its
//     own row in LDS and leaves the row's gradient in place, and the tile goes out the way it came in.  The LDS row pitch is
//     odd, so the 32 rows of a half wave sit on 32 different banks while every thread walks its row.
//   * no floating-point atomics: workgroup b writes its two sums to partial[2b], partial[2b+1]; rows_ce_final_kernel adds them
//     in a fixed order (every lane a contiguous run of slots in slot order, then the lanes in a fixed tree).  The same inputs
//     give the same bits on every run.
//   * every index is int64.
#include "b2m_common.h"
#pragma clang fp contract(off)

#define CE_ROWS 256
#define CE_MAX_CLASS 63                             // 256 rows x 63 floats = 63 KiB of LDS

__global__ __launch_bounds__(CE_ROWS) void rows_ce_kernel(const float* __restrict__ z, int64_t ld, int64_t N, int C,
                                                          const int64_t* __restrict__ labels, const double* __restrict__ n_valid,
                                                          float weight, float* __restrict__ d_z, int64_t* __restrict__ argmax,
                                                          double* __restrict__ partial) {
    extern __shared__ float tile[];                 // [CE_ROWS][Cs]
    __shared__ double red[CE_ROWS / 64][2];
    const int Cs = C | 1;
    const int64_t row0 = (int64_t)blockIdx.x * CE_ROWS;
    const int rows = (int)(N - row0 < CE_ROWS ? N - row0 : CE_ROWS);
    const int n_el = rows * C;
    for (int e = threadIdx.x; e < n_el; e += CE_ROWS) {
        const int r = e / C, c = e - r * C;
        tile[r * Cs + c] = z[(row0 + r) * ld + c];
    }
    __syncthreads();
    double ce = 0.0, hit = 0.0;
    if ((int)threadIdx.x < rows) {
        float* zr = tile + threadIdx.x * Cs;
        const int64_t t = labels[row0 + threadIdx.x];
        float mx = zr[0]; int am = 0;
        for (int c = 1; c < C; ++c) if (zr[c] > mx) { mx = zr[c]; am = c; }            // first maximum, like torch.argmax
        double den = 0;
        for (int c = 0; c < C; ++c) den += exp((double)zr[c] - (double)mx);
        argmax[row0 + threadIdx.x] = am;
        hit = (t == am) ? 1.0 : 0.0;
        const bool valid = t >= 0 && t < C;                                             // ignore_index = -100
        const double inv_n = 1.0 / *n_valid;
        if (valid) ce = log(den) - ((double)zr[t] - (double)mx);
        for (int c = 0; c < C; ++c) {
            const double p = exp((double)zr[c] - (double)mx) / den;
            zr[c] = valid ? (float)((double)weight * (p - (c == t ? 1.0 : 0.0)) * inv_n) : 0.f;
        }
    }
    __syncthreads();
    float* out = d_z + row0 * C;                                                        // the gradient is dense
    for (int e = threadIdx.x; e < n_el; e += CE_ROWS) {
        const int r = e / C, c = e - r * C;
        out[e] = tile[r * Cs + c];
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { ce += __shfl_down(ce, d, 64); hit += __shfl_down(hit, d, 64); }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = ce; red[threadIdx.x >> 6][1] = hit; }
    __syncthreads();
    if (threadIdx.x < 2)
        partial[2 * (int64_t)blockIdx.x + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// result[0] weight * loss, 1 loss, 2 accuracy
__global__ __launch_bounds__(64) void rows_ce_final_kernel(const double* __restrict__ partial, int64_t n_blocks, int64_t N,
                                                           const double* __restrict__ n_valid, float weight,
                                                           float* __restrict__ result) {
    const int64_t per = (n_blocks + 63) / 64, b0 = (int64_t)threadIdx.x * per;
    const int64_t b1 = b0 + per < n_blocks ? b0 + per : n_blocks;
    double ce = 0.0, hit = 0.0;
    for (int64_t b = b0; b < b1; ++b) { ce += partial[2 * b]; hit += partial[2 * b + 1]; }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { ce += __shfl_down(ce, d, 64); hit += __shfl_down(hit, d, 64); }
    if (threadIdx.x == 0) {
        const double loss = ce / *n_valid;
        result[0] = (float)((double)weight * loss); result[1] = (float)loss; result[2] = (float)(hit / (double)N);
    }
}

extern "C" int b2m_rows_ce_loss(const float* logits, int64_t ld, int64_t N, int32_t n_class, const int64_t* labels,
                                const double* n_valid, float weight, float* d_logits, int64_t* argmax, double* partial,
                                float* result, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(logits && labels && n_valid && d_logits && argmax && partial && result && N >= 1, "bad arguments");
    B2M_CHECK_ARG(n_class >= 1 && n_class <= CE_MAX_CLASS && ld >= n_class, "1 <= n_class <= 63 and a pitch of at least n_class");
    const int64_t n_blocks = cdiv64(N, CE_ROWS);
    B2M_CHECK_ARG(n_blocks <= 0x7fffffff, "too many rows");
    const size_t lds = (size_t)CE_ROWS * (size_t)(n_class | 1) * sizeof(float);
    rows_ce_kernel<<<(unsigned)n_blocks, CE_ROWS, lds, st>>>(logits, ld, N, n_class, labels, n_valid, weight, d_logits, argmax,
                                                             partial);
    rows_ce_final_kernel<<<1, 64, 0, st>>>(partial, n_blocks, N, n_valid, weight, result);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}
