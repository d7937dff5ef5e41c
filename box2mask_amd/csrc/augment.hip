// Scene augmentation and label recomputation on the device: the stage the reference runs on CPU workers before the
// voxelisation -- the geometric / colour augmentation of read_scene (dataprocessing/scannet.py:161-247 with
// dataprocessing/augmentation.py) and compute_bounding_box (:321-367).  Host mirror: box2mask_amd/augment.py.
//
// Everything is a streaming pass over P x 24 bytes or over a noise grid that fits in L2: one thread per point / grid
// element / vertex / instance, fp64 arithmetic without contraction (the reference is numpy fp64), no LDS beyond the
// block reductions and the byte-colour tables, no floating-point atomics (min / max go through order-preserving integer codes, sums through a
// fixed tree), so every result is the same bits run to run.
#include "b2m_common.h"
#include "../../include/b2m_prepare.h"
#pragma clang fp contract(off)

#define AUG_THREADS 256
#define AUG_MAX_BLOCKS 256

// order-preserving map double -> uint64 (for atomicMin / atomicMax over signed doubles)
__device__ __forceinline__ unsigned long long aug_ordered(double v) {
    unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double aug_unordered(unsigned long long u) {
    u = (u >> 63) ? (u & 0x7FFFFFFFFFFFFFFFull) : ~u;
    return __longlong_as_double((long long)u);
}

struct Vec3 { double v[3]; };
struct Mat3 { double m[9]; };

// ------------------------------------------------------------------ column statistics: mean, min, max, max |.|
// stats[0:3] = column mean, [3:6] = min, [6:9] = max, [9:12] = max of absolute values, of an (n,3) fp64 array.
// Stage 1: block b reduces the rows b, b + gridDim, ... (thread t of it the rows of that set with index = t mod 256), LDS tree;
// stage 2: one block reduces the gridDim partial rows the same way.  The grid is a function of n alone: a fixed summation order.
__device__ __forceinline__ void aug_stat_merge(double* a, const double* b) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        a[c] += b[c];
        a[3 + c] = b[3 + c] < a[3 + c] ? b[3 + c] : a[3 + c];
        a[6 + c] = b[6 + c] > a[6 + c] ? b[6 + c] : a[6 + c];
        a[9 + c] = b[9 + c] > a[9 + c] ? b[9 + c] : a[9 + c];
    }
}
__device__ __forceinline__ void aug_stat_block(double* acc, double (*sh)[12]) {
#pragma unroll
    for (int k = 0; k < 12; ++k) sh[threadIdx.x][k] = acc[k];
    __syncthreads();
    for (int o = AUG_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) aug_stat_merge(sh[threadIdx.x], sh[threadIdx.x + o]);
        __syncthreads();
    }
}
__global__ __launch_bounds__(AUG_THREADS) void aug_stats_partial_kernel(const double* __restrict__ x, int64_t n,
                                                                        double* __restrict__ partial) {
    __shared__ double sh[AUG_THREADS][12];
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    double acc[12] = {0, 0, 0, inf, inf, inf, -inf, -inf, -inf, 0, 0, 0};
    for (int64_t p = (int64_t)blockIdx.x * AUG_THREADS + threadIdx.x; p < n; p += (int64_t)gridDim.x * AUG_THREADS) {
        double r[12];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v = x[3 * p + c];
            r[c] = v; r[3 + c] = v; r[6 + c] = v; r[9 + c] = fabs(v);
        }
        aug_stat_merge(acc, r);
    }
    aug_stat_block(acc, sh);
    if (threadIdx.x < 12) partial[(int64_t)blockIdx.x * 12 + threadIdx.x] = sh[0][threadIdx.x];
}
__global__ __launch_bounds__(AUG_THREADS) void aug_stats_final_kernel(const double* __restrict__ partial, int nb, int64_t n,
                                                                      double* __restrict__ stats) {
    __shared__ double sh[AUG_THREADS][12];
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    double acc[12] = {0, 0, 0, inf, inf, inf, -inf, -inf, -inf, 0, 0, 0};
    if ((int)threadIdx.x < nb) {
#pragma unroll
        for (int k = 0; k < 12; ++k) acc[k] = partial[(int64_t)threadIdx.x * 12 + k];
    }
    aug_stat_block(acc, sh);
    if (threadIdx.x < 12) stats[threadIdx.x] = threadIdx.x < 3 ? sh[0][threadIdx.x] / (double)n : sh[0][threadIdx.x];
}

extern "C" int b2m_aug_stats(const double* x, int64_t n, double* partial, double* stats, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(x && partial && stats, "NULL pointer");
    B2M_CHECK_ARG(n > 0 && n < (1ll << 31), "n must be in [1, 2^31)");
    int64_t nb = cdiv64(n, AUG_THREADS * 4);
    if (nb > AUG_MAX_BLOCKS) nb = AUG_MAX_BLOCKS;
    aug_stats_partial_kernel<<<(unsigned)nb, AUG_THREADS, 0, st>>>(x, n, partial);
    aug_stats_final_kernel<<<1, AUG_THREADS, 0, st>>>(partial, (int)nb, n, stats);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// ------------------------------------------------------------------ affine map of positions and normals
__global__ void aug_affine_kernel(double* __restrict__ pos, double* __restrict__ normals, int64_t n, Mat3 M, Mat3 K, Vec3 ch,
                                  const double* __restrict__ c_dev, Vec3 t, int recentre) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    double c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = c_dev ? c_dev[a] : ch.v[a];
    const double dx = pos[3 * p] - c[0], dy = pos[3 * p + 1] - c[1], dz = pos[3 * p + 2] - c[2];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double v = dx * M.m[3 * a] + dy * M.m[3 * a + 1] + dz * M.m[3 * a + 2];
        if (recentre) v = v + c[a];
        pos[3 * p + a] = v + t.v[a];
    }
    if (normals) {
        const double nx = normals[3 * p], ny = normals[3 * p + 1], nz = normals[3 * p + 2];
        double o[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) o[a] = nx * K.m[3 * a] + ny * K.m[3 * a + 1] + nz * K.m[3 * a + 2];
        const double len = sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2]);
        if (len > 0.0) { o[0] /= len; o[1] /= len; o[2] /= len; }
        else if (len == 0.0) { o[0] = 0.0; o[1] = 0.0; o[2] = 1.0; }
        normals[3 * p] = o[0]; normals[3 * p + 1] = o[1]; normals[3 * p + 2] = o[2];
    }
}

extern "C" int b2m_aug_affine(double* pos, double* normals, int64_t n, const double* m_host, const double* c_host,
                              const double* c_dev, const double* t_host, int32_t recentre, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(pos && m_host, "NULL pointer");
    B2M_CHECK_ARG(n > 0, "n must be positive");
    Mat3 M, K;
    Vec3 c = {{0, 0, 0}}, t = {{0, 0, 0}};
    for (int k = 0; k < 9; ++k) M.m[k] = m_host[k];
    if (c_host) for (int k = 0; k < 3; ++k) c.v[k] = c_host[k];
    if (t_host) for (int k = 0; k < 3; ++k) t.v[k] = t_host[k];
    // cofactor matrix: K[i][j] = (-1)^(i+j) minor(i,j); area vectors (a x b) of a mesh map to K (a x b) under x -> M x
    const double* m = M.m;
    K.m[0] = m[4] * m[8] - m[5] * m[7]; K.m[1] = m[5] * m[6] - m[3] * m[8]; K.m[2] = m[3] * m[7] - m[4] * m[6];
    K.m[3] = m[2] * m[7] - m[1] * m[8]; K.m[4] = m[0] * m[8] - m[2] * m[6]; K.m[5] = m[1] * m[6] - m[0] * m[7];
    K.m[6] = m[1] * m[5] - m[2] * m[4]; K.m[7] = m[2] * m[3] - m[0] * m[5]; K.m[8] = m[0] * m[4] - m[1] * m[3];
    aug_affine_kernel<<<(unsigned)cdiv64(n, AUG_THREADS), AUG_THREADS, 0, st>>>(pos, normals, n, M, K, c, c_dev, t, recentre ? 1 : 0);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// x += a * y  (position jitter: positions + sigma * randn, scannet.py:202-204)
__global__ void aug_axpy_kernel(double* __restrict__ x, const double* __restrict__ y, double a, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = x[i] + a * y[i];
}
extern "C" int b2m_aug_axpy(double* x, const double* y, double a, int64_t n, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(x && y, "NULL pointer");
    B2M_CHECK_ARG(n > 0, "n must be positive");
    aug_axpy_kernel<<<(unsigned)cdiv64(n, AUG_THREADS), AUG_THREADS, 0, st>>>(x, y, a, n);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// ------------------------------------------------------------------ grid blur
// One zero-padded 3-tap pass along `axis` of an fp32 grid (nx,ny,nz,3): weight float32(1)/float32(3) widened to fp64, fp64 sum,
// one rounding to fp32 -- what scipy.ndimage.convolve(mode='constant', cval=0) does with the float32 arrays of augmentation.py:74-87.
__global__ void aug_blur_kernel(const float* __restrict__ in, float* __restrict__ out, int nx, int ny, int nz, int axis) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)nx * ny * nz * 3;
    if (e >= total) return;
    const int64_t cell = e / 3;
    const int iz = (int)(cell % nz), iy = (int)((cell / nz) % ny), ix = (int)(cell / ((int64_t)nz * ny));
    const int i = axis == 0 ? ix : (axis == 1 ? iy : iz);
    const int len = axis == 0 ? nx : (axis == 1 ? ny : nz);
    const int64_t stride = axis == 0 ? (int64_t)ny * nz * 3 : (axis == 1 ? (int64_t)nz * 3 : 3);
    const double w = (double)(1.0f / 3.0f);
    double acc = 0.0;
    if (i > 0) acc = acc + w * (double)in[e - stride];
    acc = acc + w * (double)in[e];
    if (i + 1 < len) acc = acc + w * (double)in[e + stride];
    out[e] = (float)acc;
}

extern "C" int b2m_aug_blur(float* grid, float* tmp, int32_t nx, int32_t ny, int32_t nz, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(grid && tmp, "NULL pointer");
    B2M_CHECK_ARG(nx >= 2 && ny >= 2 && nz >= 2, "every grid axis needs at least 2 nodes");
    const int64_t total = (int64_t)nx * ny * nz * 3;
    B2M_CHECK_ARG(total < (1ll << 31), "grid too large");
    const unsigned nb = (unsigned)cdiv64(total, AUG_THREADS);
    float *a = grid, *b = tmp;
    for (int pass = 0; pass < 6; ++pass) {              // x, y, z, x, y, z: the result of the sixth pass is back in `grid`
        aug_blur_kernel<<<nb, AUG_THREADS, 0, st>>>(a, b, nx, ny, nz, pass % 3);
        float* s = a; a = b; b = s;
    }
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// ------------------------------------------------------------------ trilinear displacement
struct Axes { double lo[3], step[3], hi[3]; int n[3]; };

__global__ void aug_displace_kernel(double* __restrict__ pos, int64_t n, const float* __restrict__ grid, Axes ax, double magnitude) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    double x[3], t[3];
    int i0[3];
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        x[a] = pos[3 * p + a];
        inside = inside && (x[a] >= ax.lo[a]) && (x[a] <= ax.hi[a]);           // bounds_error=0, fill_value=0; NaN is outside
    }
    if (!inside) return;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int last = ax.n[a] - 1;
        int i = (int)floor((x[a] - ax.lo[a]) / ax.step[a]);
        i = i < 0 ? 0 : (i > last - 1 ? last - 1 : i);
        // nodes as np.linspace lays them out: lo + i * step, the last one exactly hi
        double g0 = ax.lo[a] + (double)i * ax.step[a];
        if (i > 0 && x[a] < g0) { --i; g0 = ax.lo[a] + (double)i * ax.step[a]; }
        double g1 = (i + 1 == last) ? ax.hi[a] : ax.lo[a] + (double)(i + 1) * ax.step[a];
        if (i + 1 < last && x[a] > g1) {
            ++i; g0 = g1;
            g1 = (i + 1 == last) ? ax.hi[a] : ax.lo[a] + (double)(i + 1) * ax.step[a];
        }
        i0[a] = i;
        t[a] = (x[a] - g0) / (g1 - g0);
    }
    const int64_t sy = (int64_t)ax.n[2] * 3, sx = (int64_t)ax.n[1] * sy;
    const float* g = grid + (int64_t)i0[0] * sx + (int64_t)i0[1] * sy + (int64_t)i0[2] * 3;
    double d[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int bx = k >> 2, by = (k >> 1) & 1, bz = k & 1;
        const double w = (bx ? t[0] : 1.0 - t[0]) * (by ? t[1] : 1.0 - t[1]) * (bz ? t[2] : 1.0 - t[2]);
        const float* q = g + bx * sx + by * sy + bz * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = d[c] + (double)q[c] * w;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) pos[3 * p + a] = x[a] + d[a] * magnitude;
}

extern "C" int b2m_aug_displace(double* pos, int64_t n, const float* grid, int32_t nx, int32_t ny, int32_t nz,
                                const double* lo_host, const double* step_host, const double* hi_host, double magnitude,
                                void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(pos && grid && lo_host && step_host && hi_host, "NULL pointer");
    B2M_CHECK_ARG(n > 0, "n must be positive");
    B2M_CHECK_ARG(nx >= 2 && ny >= 2 && nz >= 2, "every grid axis needs at least 2 nodes");
    Axes ax;
    ax.n[0] = nx; ax.n[1] = ny; ax.n[2] = nz;
    for (int a = 0; a < 3; ++a) {
        ax.lo[a] = lo_host[a]; ax.step[a] = step_host[a]; ax.hi[a] = hi_host[a];
        B2M_CHECK_ARG(ax.step[a] > 0.0 && ax.hi[a] > ax.lo[a], "grid axes must ascend");
    }
    aug_displace_kernel<<<(unsigned)cdiv64(n, AUG_THREADS), AUG_THREADS, 0, st>>>(pos, n, grid, ax, magnitude);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// ------------------------------------------------------------------ vertex normals from faces
// One thread per vertex walks its faces (CSR row, ascending face index), sums the unnormalised cross products
// (p1 - p0) x (p2 - p0) and normalises; a zero sum becomes (0,0,1).
__global__ void aug_vertex_normals_kernel(const double* __restrict__ pos, int64_t n_vert, const int64_t* __restrict__ faces,
                                          int64_t n_faces, const int64_t* __restrict__ row_ptr,
                                          const int64_t* __restrict__ face_of, double* __restrict__ normals) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_vert) return;
    double s[3] = {0.0, 0.0, 0.0};
    int64_t b = row_ptr[v], e = row_ptr[v + 1];
    if (b < 0) b = 0;
    if (e > 3 * n_faces) e = 3 * n_faces;
    for (int64_t k = b; k < e; ++k) {
        const int64_t f = face_of[k];
        if (f < 0 || f >= n_faces) continue;
        const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        if (i0 < 0 || i0 >= n_vert || i1 < 0 || i1 >= n_vert || i2 < 0 || i2 >= n_vert) continue;
        const double ax = pos[3 * i1] - pos[3 * i0], ay = pos[3 * i1 + 1] - pos[3 * i0 + 1], az = pos[3 * i1 + 2] - pos[3 * i0 + 2];
        const double bx = pos[3 * i2] - pos[3 * i0], by = pos[3 * i2 + 1] - pos[3 * i0 + 1], bz = pos[3 * i2 + 2] - pos[3 * i0 + 2];
        s[0] = s[0] + (ay * bz - az * by);
        s[1] = s[1] + (az * bx - ax * bz);
        s[2] = s[2] + (ax * by - ay * bx);
    }
    const double len = sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    if (len > 0.0) { s[0] /= len; s[1] /= len; s[2] /= len; }
    else { s[0] = 0.0; s[1] = 0.0; s[2] = 1.0; }
    normals[3 * v] = s[0]; normals[3 * v + 1] = s[1]; normals[3 * v + 2] = s[2];
}

extern "C" int b2m_aug_vertex_normals(const double* pos, int64_t n_vert, const int64_t* faces, int64_t n_faces,
                                      const int64_t* row_ptr, const int64_t* face_of, double* normals, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(pos && row_ptr && normals, "NULL pointer");
    B2M_CHECK_ARG(n_vert > 0 && n_faces >= 0, "n_vert must be positive");
    B2M_CHECK_ARG(n_faces == 0 || (faces && face_of), "NULL pointer");
    aug_vertex_normals_kernel<<<(unsigned)cdiv64(n_vert, AUG_THREADS), AUG_THREADS, 0, st>>>(pos, n_vert, faces, n_faces, row_ptr,
                                                                                             face_of, normals);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// ------------------------------------------------------------------ colour
// In the reference's order (scannet.py:221-235): ChromaticAutoContrast (augmentation.py:134-146; a constant channel gives
// scale = inf and 0 * inf = NaN, as numpy does), ChromaticTranslation (:108-112), color_jittering (:52-61).
#define AUG_COL_CONTRAST 1
#define AUG_COL_TRANSLATE 2
#define AUG_COL_JITTER 4
__device__ __forceinline__ double aug_clip01(double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }      // NaN stays NaN (np.clip)

__global__ void aug_colour_kernel(double* __restrict__ col, int64_t n3, const double* __restrict__ stats, int flags, double blend,
                                  Vec3 tr, const double* __restrict__ jitter) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n3) return;
    const int c = (int)(e % 3);
    double v = col[e];
    if (flags & AUG_COL_CONTRAST) {
        const double lo = stats[3 + c], hi = stats[6 + c];
        const double scale = 1.0 / (hi - lo);
        const double contrast = (v - lo) * scale;
        v = (1.0 - blend) * v + blend * contrast;
    }
    if (flags & AUG_COL_TRANSLATE) v = aug_clip01(tr.v[c] + v);
    if (flags & AUG_COL_JITTER) v = aug_clip01(jitter[e] + v);
    col[e] = v;
}

extern "C" int b2m_aug_colour(double* colors, int64_t n, const double* stats, int32_t flags, double blend,
                              const double* tr_host, const double* jitter, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(colors, "NULL pointer");
    B2M_CHECK_ARG(n > 0, "n must be positive");
    B2M_CHECK_ARG(flags >= 0 && flags < 8, "unknown flags");
    B2M_CHECK_ARG(!(flags & AUG_COL_CONTRAST) || stats, "auto contrast needs the column statistics");
    B2M_CHECK_ARG(!(flags & AUG_COL_TRANSLATE) || tr_host, "translation needs its row");
    B2M_CHECK_ARG(!(flags & AUG_COL_JITTER) || jitter, "jitter needs its array");
    Vec3 tr = {{0, 0, 0}};
    if (tr_host) for (int k = 0; k < 3; ++k) tr.v[k] = tr_host[k];
    aug_colour_kernel<<<(unsigned)cdiv64(n * 3, AUG_THREADS), AUG_THREADS, 0, st>>>(colors, n * 3, stats, flags, blend, tr, jitter);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// ------------------------------------------------------------------ byte colours: brightness, hue step, Mix3D tables, normalisation
// random_brightness (augmentation.py:63-66), apply_mix3d_color_aug (:148-156) and apply_hue_aug (:158-168) as the exact rule of
// profiles/colour8_rule.md (restated in tests/_colour8_rule.py): an optional float32 brightness stage, then quantise -> [RGB->HSV,
// one table per shifted channel, HSV->RGB] -> one composed table per RGB channel -> (u8 - mean) * den in fp32.  The 8-bit
// conversions are OpenCV's integer RGB->HSV (hue range 180) and its fp32 HSV->RGB.  One thread per point, one streaming pass; the
// whole parameter block travels as a kernel argument and is spread to LDS by each block, so the step costs no copy and no host read.
#define AUG_C8_F32_PRODUCT 1
#define AUG_C8_BRIGHTNESS 2
struct Colour8Args {
    uint32_t tab[6 * 64];                   // 256-byte tables: hue, sat, val, then r, g, b
    float mean[3], den[3];
    float beta;
    int32_t flags, hsv;                     // hsv: bit k = the table of HSV channel k is present; 0 = no conversion at all
};

// (color * 255).astype(uint8): truncation; NaN and negative products give 0, products above 255 give 255 (numpy leaves them undefined)
__device__ __forceinline__ int aug_c8_quant(double c, bool f32) {
    if (f32) {
        const float p = (float)c * 255.0f;
        return !(p > 0.0f) ? 0 : (p >= 255.0f ? 255 : (int)p);
    }
    const double p = c * 255.0;
    return !(p > 0.0) ? 0 : (p >= 255.0 ? 255 : (int)p);
}
__device__ __forceinline__ int aug_c8_sat(float x) {              // saturate(rint(x * 255)), round half to even
    const float r = rintf(x * 255.0f);
    return !(r > 0.0f) ? 0 : (r >= 255.0f ? 255 : (int)r);
}

template <bool BYTES>
__global__ __launch_bounds__(AUG_THREADS) void aug_colour8_kernel(double* __restrict__ col, int64_t n, Colour8Args a) {
    __shared__ uint32_t tab_w[6 * 64];
    __shared__ int32_t sdiv[256], hdiv[256];
    const uint8_t* tab = (const uint8_t*)tab_w;
    if (BYTES) {
        for (int k = threadIdx.x; k < 6 * 64; k += AUG_THREADS) tab_w[k] = a.tab[k];
        if (a.hsv) {
            for (int i = threadIdx.x; i < 256; i += AUG_THREADS) {
                sdiv[i] = i ? (int32_t)rint((double)(255 << 12) / (1.0 * (double)i)) : 0;
                hdiv[i] = i ? (int32_t)rint((double)(180 << 12) / (6.0 * (double)i)) : 0;
            }
        }
        __syncthreads();
    }
    for (int64_t p = (int64_t)blockIdx.x * AUG_THREADS + threadIdx.x; p < n; p += (int64_t)gridDim.x * AUG_THREADS) {
        double c[3] = {col[3 * p], col[3 * p + 1], col[3 * p + 2]};
        if (a.flags & AUG_C8_BRIGHTNESS) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float v = (float)c[k];
                v = v + a.beta;
                v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);                  // NaN stays NaN (np.clip)
                c[k] = (double)v;
            }
        }
        if (BYTES) {
            const bool f32 = (a.flags & AUG_C8_F32_PRODUCT) != 0;
            int r = aug_c8_quant(c[0], f32), g = aug_c8_quant(c[1], f32), b = aug_c8_quant(c[2], f32);
            if (a.hsv) {
                // RGB -> HSV, integers; the order of the tests is the tie rule
                const int v = max(r, max(g, b)), d = v - min(r, min(g, b));
                int s = (d * sdiv[v] + 2048) >> 12;
                int h = v == r ? g - b : (v == g ? b - r + 2 * d : r - g + 4 * d);
                h = (h * hdiv[d] + 2048) >> 12;
                if (h < 0) h += 180;
                int H = h, S = s, V = v;
                if (a.hsv & 1) H = tab[H & 255];
                if (a.hsv & 2) S = tab[256 + (S & 255)];
                if (a.hsv & 4) V = tab[512 + V];
                // HSV -> RGB, fp32
                float hf = (float)H * (6.0f / 180.0f);
                const float sf = (float)S * (1.0f / 255.0f), vf = (float)V * (1.0f / 255.0f);
                float fb = vf, fg = vf, fr = vf;
                if (sf != 0.0f) {
                    hf = fmodf(hf, 6.0f);
                    int sector = (int)floorf(hf);
                    hf = hf - (float)sector;
                    if (sector < 0 || sector > 5) { sector = 0; hf = 0.0f; }
                    const float t1 = vf * (1.0f - sf), t2 = vf * (1.0f - sf * hf), t3 = vf * (1.0f - sf * (1.0f - hf));
                    // (b, g, r) = tab[T[sector]], T = {{1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}} over tab = {v, t1, t2, t3}
                    switch (sector) {
                        case 0: fb = t1; fg = t3; fr = vf; break;
                        case 1: fb = t1; fg = vf; fr = t2; break;
                        case 2: fb = t3; fg = vf; fr = t1; break;
                        case 3: fb = vf; fg = t2; fr = t1; break;
                        case 4: fb = vf; fg = t1; fr = t3; break;
                        default: fb = t2; fg = t1; fr = vf; break;
                    }
                }
                r = aug_c8_sat(fr); g = aug_c8_sat(fg); b = aug_c8_sat(fb);
            }
            r = tab[768 + r]; g = tab[1024 + g]; b = tab[1280 + b];
            c[0] = (double)(((float)r - a.mean[0]) * a.den[0]);
            c[1] = (double)(((float)g - a.mean[1]) * a.den[1]);
            c[2] = (double)(((float)b - a.mean[2]) * a.den[2]);
        }
        col[3 * p] = c[0]; col[3 * p + 1] = c[1]; col[3 * p + 2] = c[2];
    }
}

static unsigned aug_colour8_blocks(int64_t n) {
    const int64_t nb = cdiv64(n, AUG_THREADS);
    return (unsigned)(nb > 2048 ? 2048 : nb);                 // 8 blocks on each of the 256 CUs, then a grid-stride loop
}

extern "C" int b2m_aug_colour8(double* colors, int64_t n, int32_t flags, float beta, const uint8_t* hue_tab_host,
                               const uint8_t* sat_tab_host, const uint8_t* val_tab_host, const uint8_t* r_tab_host,
                               const uint8_t* g_tab_host, const uint8_t* b_tab_host, const float* mean_host, const float* den_host,
                               void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(colors, "NULL pointer");
    B2M_CHECK_ARG(n > 0, "n must be positive");
    B2M_CHECK_ARG(flags >= 0 && flags < 4, "unknown flags");
    B2M_CHECK_ARG(r_tab_host && g_tab_host && b_tab_host, "the three RGB tables are needed");
    B2M_CHECK_ARG(mean_host && den_host, "the normalisation needs its mean and reciprocal rows");
    Colour8Args a = {};
    const uint8_t* tabs[6] = {hue_tab_host, sat_tab_host, val_tab_host, r_tab_host, g_tab_host, b_tab_host};
    uint8_t* bytes = (uint8_t*)a.tab;
    for (int k = 0; k < 6; ++k) {
        if (!tabs[k]) continue;
        for (int i = 0; i < 256; ++i) bytes[256 * k + i] = tabs[k][i];
        if (k < 3) a.hsv |= 1 << k;
    }
    for (int k = 0; k < 3; ++k) { a.mean[k] = mean_host[k]; a.den[k] = den_host[k]; }
    a.beta = beta;
    a.flags = flags;
    aug_colour8_kernel<true><<<aug_colour8_blocks(n), AUG_THREADS, 0, st>>>(colors, n, a);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// random_brightness alone: colors <- clip(float32(colors) + beta, 0, 1), the float32 values widened back to fp64
extern "C" int b2m_aug_brightness(double* colors, int64_t n, float beta, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(colors, "NULL pointer");
    B2M_CHECK_ARG(n > 0, "n must be positive");
    Colour8Args a = {};
    a.beta = beta;
    a.flags = AUG_C8_BRIGHTNESS;
    aug_colour8_kernel<false><<<aug_colour8_blocks(n), AUG_THREADS, 0, st>>>(colors, n, a);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// ------------------------------------------------------------------ instance boxes (compute_bounding_box, scannet.py:321-367)
// acc: uint64[8 * n_inst] -- per instance [min xyz (order-preserving codes), lowest point index] x n_inst, then [max xyz] x n_inst,
// then the radius code x n_inst.
__global__ void inst_minmax_kernel(const double* __restrict__ pos, const int64_t* __restrict__ inst, int64_t n, int64_t n_inst,
                                   unsigned long long* __restrict__ acc) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int64_t i = inst[p];
    if (i < 0 || i >= n_inst) return;
    unsigned long long* a = acc + 4 * i;
    unsigned long long* b = acc + 4 * n_inst + 3 * i;
    // a plain read in front of every atomic: once an instance's box has grown, most points no longer touch the atomic unit
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned long long code = aug_ordered(pos[3 * p + c]);
        if (code < __hip_atomic_load(&a[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&a[c], code);
        if (code > __hip_atomic_load(&b[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&b[c], code);
    }
    if ((unsigned long long)p < __hip_atomic_load(&a[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMin(&a[3], (unsigned long long)p);
}
__global__ void inst_box_kernel(const unsigned long long* __restrict__ acc, const int64_t* __restrict__ sem, int64_t n, int64_t n_inst,
                                double* __restrict__ centers64, int32_t* __restrict__ per_sem, float* __restrict__ per_centers,
                                float* __restrict__ per_bounds, int32_t* __restrict__ missing) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_inst) return;
    const unsigned long long* a = acc + 4 * i;
    const unsigned long long* b = acc + 4 * n_inst + 3 * i;
    const unsigned long long first = a[3];
    if (first >= (unsigned long long)n) {                    // an id without a point: the ids are not dense
        atomicAdd(missing, 1);
        per_sem[i] = 0;
        for (int c = 0; c < 3; ++c) { centers64[3 * i + c] = 0.0; per_centers[3 * i + c] = 0.f; per_bounds[3 * i + c] = 0.f; }
        return;
    }
    per_sem[i] = (int32_t)sem[first];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double lo = aug_unordered(a[c]), hi = aug_unordered(b[c]);
        const double centre = (lo + hi) / 2;
        centers64[3 * i + c] = centre;
        per_centers[3 * i + c] = (float)centre;
        per_bounds[3 * i + c] = (float)(hi - centre);
    }
}
__global__ void inst_offsets_kernel(const double* __restrict__ pos, const int64_t* __restrict__ inst, int64_t n, int64_t n_inst,
                                    const double* __restrict__ centers64, float* __restrict__ offsets, float* __restrict__ dist,
                                    unsigned long long* __restrict__ racc) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int64_t i = inst[p];
    if (i < 0 || i >= n_inst) {
        offsets[3 * p] = 0.f; offsets[3 * p + 1] = 0.f; offsets[3 * p + 2] = 0.f; dist[p] = 0.f;
        return;
    }
    const double ox = centers64[3 * i] - pos[3 * p], oy = centers64[3 * i + 1] - pos[3 * p + 1], oz = centers64[3 * i + 2] - pos[3 * p + 2];
    offsets[3 * p] = (float)ox; offsets[3 * p + 1] = (float)oy; offsets[3 * p + 2] = (float)oz;
    const double d = sqrt(ox * ox + oy * oy + oz * oz);
    dist[p] = (float)d;
    const unsigned long long code = (unsigned long long)__double_as_longlong(d);        // d >= 0: bit order == value order
    if (code > __hip_atomic_load(&racc[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&racc[i], code);
}
__global__ void inst_radius_kernel(const unsigned long long* __restrict__ racc, int64_t n_inst, float* __restrict__ per_radius) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_inst) per_radius[i] = (float)__longlong_as_double((long long)racc[i]);
}

extern "C" int b2m_inst_boxes(const double* pos, const int64_t* instances, const int64_t* semantics, int64_t n, int64_t n_inst,
                              uint64_t* acc, double* centers64, int32_t* per_sem, float* per_centers, float* per_bounds,
                              float* per_radius, float* offsets, float* distances, int32_t* missing, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(pos && instances && semantics && acc && centers64 && per_sem && per_centers && per_bounds && per_radius &&
                  offsets && distances && missing, "NULL pointer");
    B2M_CHECK_ARG(n > 0 && n < (1ll << 31), "n must be in [1, 2^31)");
    B2M_CHECK_ARG(n_inst > 0 && n_inst <= n, "n_inst must be in [1, n]");
    unsigned long long* a = (unsigned long long*)acc;
    unsigned long long* racc = a + 7 * n_inst;
    // min codes and the first index start at all ones, max codes and the radius at zero
    B2M_HIP(hipMemsetAsync(a, 0xFF, (size_t)n_inst * 4 * sizeof(uint64_t), st));
    B2M_HIP(hipMemsetAsync(a + 4 * n_inst, 0, (size_t)n_inst * 4 * sizeof(uint64_t), st));
    B2M_HIP(hipMemsetAsync(missing, 0, sizeof(int32_t), st));
    const unsigned nbp = (unsigned)cdiv64(n, AUG_THREADS), nbi = (unsigned)cdiv64(n_inst, AUG_THREADS);
    inst_minmax_kernel<<<nbp, AUG_THREADS, 0, st>>>(pos, instances, n, n_inst, a);
    inst_box_kernel<<<nbi, AUG_THREADS, 0, st>>>(a, semantics, n, n_inst, centers64, per_sem, per_centers, per_bounds, missing);
    inst_offsets_kernel<<<nbp, AUG_THREADS, 0, st>>>(pos, instances, n, n_inst, centers64, offsets, distances, racc);
    inst_radius_kernel<<<nbi, AUG_THREADS, 0, st>>>(racc, n_inst, per_radius);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}
