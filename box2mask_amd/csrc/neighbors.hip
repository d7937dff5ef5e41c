// Exact 1-nearest-neighbour search between two point sets (include/b2m_prepare.h, "nearest-neighbour index"): what the
// reference asks of NearestNeighbors(n_neighbors=1, algorithm='ball_tree') and of scipy's k-d tree, as one general operation.
//
//   build : bounding box of the finite reference rows (64-bit integer atomics over order-preserving keys), a cell edge chosen
//           on the device so that the grid has at most NN_CELLS_PER_ROW * n_ref + NN_CELLS_EXTRA cells whatever the extent, cell keys
//           (x slowest, z fastest: the z-neighbours of a cell are ONE run of the sorted order), the stable radix argsort of
//           coords.hip -- rows of a cell stay in ascending row order -- a sorted copy of the rows and a table of cell starts.
//           Non-finite rows get the key one past the grid: they sort behind every cell and no query ever reads them.
//   query : one thread per query walks the cells around its own (clamped into the grid) in growing Chebyshev shells and stops
//           once the best squared distance is no larger than a conservative lower bound of everything not yet visited.
//
// The distance is the ball tree's reduced distance, (dx*dx + dy*dy) + dz*dz in fp64 without contraction; equal distances
// resolve to the lowest row.  No floating-point atomics, no LDS, no barrier between workgroups: the same bits on every run.
// Every loop is bounded by the grid's dimensions or by the row count.
#include "b2m_common.h"
#include "../../include/b2m_prepare.h"
#pragma clang fp contract(off)

#define NN_THREADS 256
#define NN_CELLS_PER_ROW 4                          // the grid never has more than 4 n_ref + 8 cells ...
#define NN_CELLS_EXTRA 8
#define NN_TARGET_PER_ROW 2                         // ... and aims at 2 n_ref
#define NN_AXIS_MAX 1048576.0                       // the edge is at least the largest extent / 2^19: below 2^20 cells per axis the
                                                    // cell coordinate is exact to ~2^-32 of a cell
#define NN_SLACK (1.0 - 1.0 / 1048576.0)            // shrinks every lower bound by 2^-20, far more than any rounding above
#define NN_NO_ROW 0x7fffffff

struct NnGrid {                                     // written by nn_grid_kernel, read by everything after it
    double lo[3], hi[3];                            // bounding box of the finite rows (lo > hi: there is none)
    double edge;
    int32_t dim[3];
    int32_t any;                                    // 1 when at least one row is finite
    int64_t cells;
};

__device__ __forceinline__ uint64_t nn_enc(double v) {            // order-preserving map double -> uint64
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double nn_dec(uint64_t e) {
    const uint64_t b = (e >> 63) ? (e & 0x7fffffffffffffffull) : ~e;
    return __longlong_as_double((long long)b);
}
__device__ __forceinline__ bool nn_finite3(double x, double y, double z) {
    return isfinite(x) && isfinite(y) && isfinite(z);
}

// box[0:3] = min, box[3:6] = max of the finite rows, as order-preserving keys (initialised to ~0 / 0)
__global__ __launch_bounds__(NN_THREADS) void nn_box_kernel(const double* __restrict__ ref, int64_t n, uint64_t* __restrict__ box) {
    __shared__ uint64_t part[6][NN_THREADS / 64];
    uint64_t m[6] = {~0ull, ~0ull, ~0ull, 0ull, 0ull, 0ull};
    for (int64_t i = (int64_t)blockIdx.x * NN_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * NN_THREADS) {
        const double p[3] = {ref[i * 3], ref[i * 3 + 1], ref[i * 3 + 2]};
        if (!nn_finite3(p[0], p[1], p[2])) continue;
        for (int j = 0; j < 3; ++j) {
            const uint64_t e = nn_enc(p[j]);
            m[j] = e < m[j] ? e : m[j];
            m[3 + j] = e > m[3 + j] ? e : m[3 + j];
        }
    }
    for (int j = 0; j < 6; ++j) {
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t v = (uint64_t)__shfl_xor((unsigned long long)m[j], o);
            m[j] = (j < 3 ? v < m[j] : v > m[j]) ? v : m[j];
        }
        if (lane_id() == 0) part[j][threadIdx.x >> 6] = m[j];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int j = threadIdx.x;
        uint64_t v = part[j][0];
        for (int w = 1; w < NN_THREADS / 64; ++w) v = (j < 3 ? part[j][w] < v : part[j][w] > v) ? part[j][w] : v;
        if (j < 3) atomicMin((unsigned long long*)&box[j], (unsigned long long)v);
        else atomicMax((unsigned long long*)&box[j], (unsigned long long)v);
    }
}

__device__ __forceinline__ double nn_cells_of(const double* ext, double edge, int32_t* dim) {
    double cells = 1.0;
    for (int j = 0; j < 3; ++j) {
        const double u = floor(ext[j] / edge);
        const double d = u >= NN_AXIS_MAX ? NN_AXIS_MAX : u + 1.0;      // (never reached: edge >= largest extent / 2^19)
        dim[j] = (int32_t)d;
        cells *= d;
    }
    return cells;
}

// One thread: the cell edge.  Aims at NN_TARGET_PER_ROW * n cells over the axes of non-zero extent, then grows the edge until
// the count is within the table (at most 64 steps of 2^(1/3), a factor of 2^21 in every axis: 2^19 + 1 cells per axis become one).
__global__ void nn_grid_kernel(const uint64_t* __restrict__ box, int64_t n, NnGrid* __restrict__ g) {
    NnGrid G;
    G.any = box[0] != ~0ull;
    double ext[3];
    double big = 0.0, logv = 0.0;
    int k = 0;
    for (int j = 0; j < 3; ++j) {
        G.lo[j] = G.any ? nn_dec(box[j]) : 1.0;
        G.hi[j] = G.any ? nn_dec(box[3 + j]) : 0.0;
        double e = G.any ? G.hi[j] - G.lo[j] : 0.0;
        if (!(e < 1.7e308)) e = 1.7e308;                            // (hi - lo overflowed)
        ext[j] = e;
        big = e > big ? e : big;
        if (e > 0.0) { logv += log(e); ++k; }
    }
    const double cap = (double)NN_CELLS_PER_ROW * (double)n + (double)NN_CELLS_EXTRA;
    double edge = 1.0;
    G.dim[0] = G.dim[1] = G.dim[2] = 1;
    G.cells = 1;
    if (k > 0) {
        edge = exp((logv - log((double)NN_TARGET_PER_ROW * (double)n)) / (double)k);
        const double least = big / (NN_AXIS_MAX * 0.5);                  // at most 2^19 + 1 cells per axis
        if (!(edge >= least)) edge = least;                         // (also a NaN)
        if (!(edge > 0.0)) edge = big;                              // (underflow of big / 2^19)
        if (!(edge < 1.7e308)) edge = 1.7e308;
        double cells = nn_cells_of(ext, edge, G.dim);
        for (int it = 0; it < 64 && cells > cap; ++it) {
            edge *= 1.2599210498948732;
            if (!(edge < 1.7e308)) edge = 1.7e308;
            cells = nn_cells_of(ext, edge, G.dim);
        }
        if (cells > cap) {                                          // (not reached; one cell is always right)
            G.dim[0] = G.dim[1] = G.dim[2] = 1;
            cells = 1.0;
            edge = 1.7e308;
        }
        G.cells = (int64_t)cells;
    }
    G.edge = edge;
    *g = G;
}

// cell coordinate of v on axis j, clamped into the grid
__device__ __forceinline__ int nn_cell(double v, double lo, double edge, int dim) {
    const double u = floor((v - lo) / edge);
    return u >= (double)(dim - 1) ? dim - 1 : (u > 0.0 ? (int)u : 0);
}

__global__ __launch_bounds__(NN_THREADS) void nn_key_kernel(const double* __restrict__ ref, int64_t n, const NnGrid* __restrict__ g,
                                                            uint64_t* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * NN_THREADS + threadIdx.x;
    if (i >= n) return;
    const double x = ref[i * 3], y = ref[i * 3 + 1], z = ref[i * 3 + 2];
    uint64_t key = (uint64_t)g->cells;                               // non-finite: behind every cell
    if (nn_finite3(x, y, z)) {
        const int cx = nn_cell(x, g->lo[0], g->edge, g->dim[0]);
        const int cy = nn_cell(y, g->lo[1], g->edge, g->dim[1]);
        const int cz = nn_cell(z, g->lo[2], g->edge, g->dim[2]);
        key = ((uint64_t)cx * (uint64_t)g->dim[1] + (uint64_t)cy) * (uint64_t)g->dim[2] + (uint64_t)cz;
    }
    keys[i] = key;
}

__global__ __launch_bounds__(NN_THREADS) void nn_gather_kernel(const double* __restrict__ ref, int64_t n, const uint64_t* __restrict__ keys,
                                                               const int64_t* __restrict__ perm, double* __restrict__ xs,
                                                               uint64_t* __restrict__ skey, int32_t* __restrict__ orig) {
    const int64_t s = (int64_t)blockIdx.x * NN_THREADS + threadIdx.x;
    if (s >= n) return;
    const int64_t i = perm[s];
    xs[s * 3] = ref[i * 3]; xs[s * 3 + 1] = ref[i * 3 + 1]; xs[s * 3 + 2] = ref[i * 3 + 2];
    skey[s] = keys[i];
    orig[s] = (int32_t)i;
}

// start[c] = first sorted position whose key is not below c, for c = 0 ... cells (start[cells] = number of finite rows)
__global__ __launch_bounds__(NN_THREADS) void nn_start_kernel(const uint64_t* __restrict__ skey, int64_t n, const NnGrid* __restrict__ g,
                                                              int32_t* __restrict__ start) {
    const int64_t c = (int64_t)blockIdx.x * NN_THREADS + threadIdx.x;
    if (c > g->cells) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (skey[mid] < (uint64_t)c) lo = mid + 1; else hi = mid;
    }
    start[c] = (int32_t)lo;
}

struct NnLayout {
    int64_t box, grid, keys, perm, inv, radix, xs, skey, orig, start, total;
};
static int64_t nn_cell_cap(int64_t n) { return (int64_t)NN_CELLS_PER_ROW * n + NN_CELLS_EXTRA; }
static NnLayout nn_layout(int64_t n) {
    NnLayout L;
    int64_t at = 0;
    auto take = [&](int64_t bytes) { const int64_t p = at; at += (bytes + 255) / 256 * 256; return p; };
    L.box = take(64);
    L.grid = take(sizeof(NnGrid));
    L.keys = take(n * 8); L.perm = take(n * 8); L.inv = take(n * 8);
    L.radix = take(b2m_radix_argsort_scratch(n));
    L.xs = take(n * 24);
    L.skey = take(n * 8);
    L.orig = take(n * 4);
    L.start = take((nn_cell_cap(n) + 1) * 4);
    L.total = at;
    return L;
}
extern "C" int64_t b2m_nn_workspace(int64_t n_ref) {
    if (n_ref < 0 || n_ref >= (1ll << 29)) return -1;               // (4 n_ref + 8 cells and their starts stay below 2^31)
    return nn_layout(n_ref).total;
}

extern "C" int b2m_nn_build(const double* ref, int64_t n_ref, void* workspace, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(n_ref >= 0 && n_ref < (1ll << 29), "n_ref out of range");
    if (n_ref == 0) return B2M_OK;                                  // nothing to index; no launch
    B2M_CHECK_ARG(ref && workspace, "NULL argument");
    const NnLayout L = nn_layout(n_ref);
    char* w = (char*)workspace;
    uint64_t* box = (uint64_t*)(w + L.box);
    NnGrid* grid = (NnGrid*)(w + L.grid);
    uint64_t* keys = (uint64_t*)(w + L.keys);
    int64_t* perm = (int64_t*)(w + L.perm);
    int64_t* inv = (int64_t*)(w + L.inv);
    const unsigned nb = (unsigned)cdiv64(n_ref, NN_THREADS);
    B2M_HIP(hipMemsetAsync(box, 0xff, 24, st));
    B2M_HIP(hipMemsetAsync(box + 3, 0, 24, st));
    nn_box_kernel<<<nb < 1024 ? nb : 1024, NN_THREADS, 0, st>>>(ref, n_ref, box);
    nn_grid_kernel<<<1, 1, 0, st>>>(box, n_ref, grid);
    nn_key_kernel<<<nb, NN_THREADS, 0, st>>>(ref, n_ref, grid, keys);
    uint64_t mask = 1;
    while (mask <= (uint64_t)nn_cell_cap(n_ref)) mask <<= 1;       // keys are at most `cells` <= the cap
    const int rc = b2m_radix_argsort(keys, n_ref, mask - 1, perm, inv, w + L.radix, stream);
    if (rc != B2M_OK) return rc;
    nn_gather_kernel<<<nb, NN_THREADS, 0, st>>>(ref, n_ref, keys, perm, (double*)(w + L.xs), (uint64_t*)(w + L.skey),
                                                (int32_t*)(w + L.orig));
    nn_start_kernel<<<(unsigned)cdiv64(nn_cell_cap(n_ref) + 1, NN_THREADS), NN_THREADS, 0, st>>>(
        (const uint64_t*)(w + L.skey), n_ref, grid, (int32_t*)(w + L.start));
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// the rows of one run of cells against the query: smallest d2, lowest row among equal ones
__device__ __forceinline__ void nn_scan(const double* __restrict__ xs, const int32_t* __restrict__ orig, int s0, int s1, double qx,
                                        double qy, double qz, double& best, int& row) {
    for (int s = s0; s < s1; ++s) {
        const double dx = qx - xs[(int64_t)s * 3], dy = qy - xs[(int64_t)s * 3 + 1], dz = qz - xs[(int64_t)s * 3 + 2];
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 < best) { best = d2; row = orig[s]; }
        else if (d2 == best) { const int o = orig[s]; row = o < row ? o : row; }
    }
}

__global__ __launch_bounds__(NN_THREADS) void nn_query_kernel(const NnGrid* __restrict__ g, const double* __restrict__ xs,
                                                              const int32_t* __restrict__ orig, const int32_t* __restrict__ start,
                                                              const double* __restrict__ q, int64_t n_q, int32_t* __restrict__ idx,
                                                              double* __restrict__ dist) {
    const int64_t j = (int64_t)blockIdx.x * NN_THREADS + threadIdx.x;
    if (j >= n_q) return;
    const double qx = q[j * 3], qy = q[j * 3 + 1], qz = q[j * 3 + 2];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (!nn_finite3(qx, qy, qz) || !g->any) {
        idx[j] = -1;
        if (dist) dist[j] = nan;
        return;
    }
    const double edge = g->edge;
    const int nx = g->dim[0], ny = g->dim[1], nz = g->dim[2];
    const double qv[3] = {qx, qy, qz};
    int c[3];
    double gap2 = 0.0;                              // squared distance from the query to the box: every row is at least as far
    for (int a = 0; a < 3; ++a) {
        c[a] = nn_cell(qv[a], g->lo[a], edge, g->dim[a]);
        const double below = g->lo[a] - qv[a], above = qv[a] - g->hi[a];
        const double gp = below > 0.0 ? below : (above > 0.0 ? above : 0.0);
        gap2 += gp * gp;
    }
    gap2 *= NN_SLACK;
    int rmax = 0;
    for (int a = 0; a < 3; ++a) {
        const int far = c[a] > g->dim[a] - 1 - c[a] ? c[a] : g->dim[a] - 1 - c[a];
        rmax = far > rmax ? far : rmax;
    }
    double best = __longlong_as_double(0x7ff0000000000000ll);
    int row = NN_NO_ROW;
    for (int r = 0; r <= rmax; ++r) {
        if (r >= 2) {
            // A row not yet visited lies r cells or more from the query's cell on some axis, so at least (r - 1) * edge further
            // along that axis than the box's gap there (the box is convex: the same holds from a clamped cell).
            const double lb = (double)(r - 1) * edge * NN_SLACK;
            const double lb2 = lb * lb;
            if (lb2 > 0.0 && best < 1.7e308 && best <= lb2 + gap2) break;
        }
        const int x0 = c[0] - r, x1 = c[0] + r, y0 = c[1] - r, y1 = c[1] + r;
        const int za = c[2] - r, zb = c[2] + r;
        const int zlo = za > 0 ? za : 0, zhi = zb < nz - 1 ? zb : nz - 1;
        for (int x = x0 > 0 ? x0 : 0; x <= (x1 < nx - 1 ? x1 : nx - 1); ++x) {
            const bool xface = x == x0 || x == x1;
            for (int y = y0 > 0 ? y0 : 0; y <= (y1 < ny - 1 ? y1 : ny - 1); ++y) {
                const int64_t base = ((int64_t)x * ny + y) * nz;
                if (xface || y == y0 || y == y1) {                  // a face of the shell: the whole z-run
                    nn_scan(xs, orig, start[base + zlo], start[base + zhi + 1], qx, qy, qz, best, row);
                } else {                                            // inside: the two end cells (one cell when r == 0 is a face)
                    if (za >= 0) nn_scan(xs, orig, start[base + za], start[base + za + 1], qx, qy, qz, best, row);
                    if (zb <= nz - 1) nn_scan(xs, orig, start[base + zb], start[base + zb + 1], qx, qy, qz, best, row);
                }
            }
        }
    }
    idx[j] = row == NN_NO_ROW ? -1 : row;
    if (dist) dist[j] = row == NN_NO_ROW ? nan : sqrt(best);
}

extern "C" int b2m_nn_query(const double* ref, int64_t n_ref, const void* workspace, const double* q, int64_t n_q, int32_t* idx,
                            double* dist, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(n_ref >= 0 && n_ref < (1ll << 29), "n_ref out of range");
    B2M_CHECK_ARG(n_q >= 0 && n_q < (1ll << 31), "n_q out of range");
    if (n_q == 0) return B2M_OK;                                    // nothing asked; no launch
    B2M_CHECK_ARG(q && idx, "NULL argument");
    if (n_ref == 0) {                                               // -1 and NaN for every query, by two fills
        B2M_HIP(hipMemsetAsync(idx, 0xff, (size_t)n_q * sizeof(int32_t), st));
        if (dist) B2M_HIP(hipMemsetAsync(dist, 0xff, (size_t)n_q * sizeof(double), st));
        return B2M_OK;
    }
    B2M_CHECK_ARG(ref && workspace, "NULL argument");
    const NnLayout L = nn_layout(n_ref);
    const char* w = (const char*)workspace;
    nn_query_kernel<<<(unsigned)cdiv64(n_q, NN_THREADS), NN_THREADS, 0, st>>>(
        (const NnGrid*)(w + L.grid), (const double*)(w + L.xs), (const int32_t*)(w + L.orig), (const int32_t*)(w + L.start), q, n_q,
        idx, dist);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}
