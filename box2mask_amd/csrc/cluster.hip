// S3DIS evaluation on the device (include/b2m.h, "S3DIS evaluation"): DBSCAN with sklearn's labelling, the greedy proposal
// merge over bit-packed masks and a joint histogram of two index columns.  Everything the labelling depends on is an integer
// operation or an fp64 comparison, so two runs give the same labels.
#include "b2m_common.h"

// ------------------------------------------------------------------ DBSCAN
// Rows are binned into cells of edge eps * (1 + 2^-20) over the first three columns (the rounding of the cell coordinate is
// ~2^-30 of a cell below 2^21 cells per axis, so two rows within eps of one another always lie in cells whose indices differ by at
// most one per axis); cell indices beyond 2^21 - 1 are clamped, which only merges cells.  The rows are sorted by cell key
// (x, y, z from the high bits down: the three z-neighbours of a cell are ONE run of the sorted order, so a cell has 9 candidate
// runs, not 27).  One workgroup owns 256 consecutive sorted rows and walks the cells they fall in; per cell it streams the 9
// runs through LDS in tiles of 256 rows, each lane testing its own query row against the tile.
#define DB_THREADS 256
#define DB_CELL_BITS 21
#define DB_CELL_MAX ((1 << DB_CELL_BITS) - 1)
#define DB_SCAN_BLOCK 1024
#define DB_NONE 0x7fffffff

__device__ __forceinline__ uint64_t db_enc(double v) {            // order-preserving map double -> uint64
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double db_dec(uint64_t e) {
    const uint64_t b = (e >> 63) ? (e & 0x7fffffffffffffffull) : ~e;
    return __longlong_as_double((long long)b);
}

__global__ __launch_bounds__(256) void db_min_kernel(const double* __restrict__ x, int64_t n, int d, uint64_t* __restrict__ lo) {
    __shared__ uint64_t part[3][4];
    uint64_t m[3] = {~0ull, ~0ull, ~0ull};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        for (int j = 0; j < 3; ++j) {
            const uint64_t e = db_enc(x[i * d + j]);
            m[j] = e < m[j] ? e : m[j];
        }
    for (int j = 0; j < 3; ++j) {
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t v = (uint64_t)__shfl_xor((unsigned long long)m[j], o);
            m[j] = v < m[j] ? v : m[j];
        }
        if (lane_id() == 0) part[j][threadIdx.x >> 6] = m[j];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        uint64_t v = part[threadIdx.x][0];
        for (int w = 1; w < 4; ++w) v = part[threadIdx.x][w] < v ? part[threadIdx.x][w] : v;
        atomicMin((unsigned long long*)&lo[threadIdx.x], (unsigned long long)v);
    }
}

__global__ __launch_bounds__(256) void db_key_kernel(const double* __restrict__ x, int64_t n, int d, double edge,
                                                     const uint64_t* __restrict__ lo, uint64_t* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint64_t key = 0;
    for (int j = 0; j < 3; ++j) {
        const double u = floor((x[i * d + j] - db_dec(lo[j])) / edge);
        const int c = u >= (double)DB_CELL_MAX ? DB_CELL_MAX : (u > 0.0 ? (int)u : 0);     // (a NaN lands in cell 0)
        key = (key << DB_CELL_BITS) | (uint64_t)c;
    }
    keys[i] = key;
}

__global__ __launch_bounds__(256) void db_gather_kernel(const double* __restrict__ x, int64_t n, int d,
                                                        const uint64_t* __restrict__ keys, const int64_t* __restrict__ perm,
                                                        double* __restrict__ xs, uint64_t* __restrict__ skey,
                                                        int32_t* __restrict__ orig, int32_t* __restrict__ parent) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const int64_t i = perm[s];
    for (int j = 0; j < d; ++j) xs[s * d + j] = x[i * d + j];
    skey[s] = keys[i];
    orig[s] = (int32_t)i;
    parent[s] = (int32_t)s;                         // (indexed by ORIGINAL row; every row is written once over the grid)
}

// first position of the sorted keys that is not below `key`
__device__ __forceinline__ int64_t db_lower_bound(const uint64_t* __restrict__ skey, int64_t n, uint64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (skey[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Union-find over ORIGINAL row numbers.  A link always points from a larger number to a smaller one and only roots are ever
// hooked, so the root of a finished component is its smallest member whatever the order of the joins.
__device__ __forceinline__ int uf_load(const int32_t* p) {
    return __hip_atomic_load(const_cast<int32_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int uf_find(int32_t* __restrict__ parent, int i) {
    int r = i, p = uf_load(&parent[r]);
    while (p != r) { r = p; p = uf_load(&parent[r]); }
    if (r != i) atomicMin(&parent[i], r);           // shortcut for the next walk: r is an ancestor of i for good
    return r;
}
__device__ __forceinline__ int uf_union(int32_t* __restrict__ parent, int i, int j) {
    int a = uf_find(parent, i), b = uf_find(parent, j);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicCAS(&parent[a], a, b);                // the larger root goes under the smaller
        if (old == a) return b;
        a = uf_find(parent, old);                                   // a was hooked meanwhile: go on from its new parent
        b = uf_find(parent, b);
    }
    return a;
}

// PASS 1: neighbour count (stops at min_samples) -> core flags.  PASS 2: joins of core-core pairs.  PASS 3: labels.
template <int D, int PASS>
__global__ __launch_bounds__(DB_THREADS) void db_pass_kernel(const double* __restrict__ xs, const uint64_t* __restrict__ skey,
                                                             const int32_t* __restrict__ orig, int64_t n, double eps2,
                                                             int min_samples, int32_t* __restrict__ core_s,
                                                             int32_t* __restrict__ core_o, int32_t* __restrict__ parent,
                                                             const int32_t* __restrict__ rank, int32_t* __restrict__ labels) {
    __shared__ double tile[DB_THREADS * D];
    __shared__ int aux_row[DB_THREADS], aux_root[DB_THREADS];
    __shared__ uint64_t bkey[DB_THREADS];
    __shared__ int64_t r_lo[9], r_hi[9];
    __shared__ int s_next, s_any;
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * DB_THREADS;
    const int64_t s = row0 + tid;
    const bool live = s < n;
    const int in_block = (int)((n - row0) < DB_THREADS ? (n - row0) : DB_THREADS);
    double q[D];
#pragma unroll
    for (int j = 0; j < D; ++j) q[j] = live ? xs[s * D + j] : 0.0;
    const int me = live ? orig[s] : 0;
    bkey[tid] = live ? skey[s] : ~0ull;             // (real keys are below 2^63)
    bool want = live;
    if (PASS == 2) want = live && core_s[s] != 0;
    if (PASS == 3) want = live && core_s[s] == 0;
    int cnt = 0;                                    // PASS 1
    int myroot = 0;                                 // PASS 2
    int minroot = DB_NONE;                          // PASS 3
    if (PASS == 2 && want) myroot = uf_find(parent, me);
    int seg = 0;
    while (seg < in_block) {
        __syncthreads();
        if (tid == 0) { s_next = DB_THREADS; s_any = 0; }
        __syncthreads();
        const uint64_t key = bkey[seg];
        if (tid > seg && bkey[tid] != key && bkey[tid - 1] == key) s_next = tid;       // (sorted: one writer at most)
        const bool mine = want && tid >= seg && bkey[tid] == key;
        bool pending = mine && (PASS != 1 || cnt < min_samples);
        if (pending) s_any = 1;
        if (tid < 9) {
            const int cx = (int)(key >> (2 * DB_CELL_BITS)) + tid / 3 - 1;
            const int cy = (int)((key >> DB_CELL_BITS) & DB_CELL_MAX) + tid % 3 - 1;
            const int cz = (int)(key & DB_CELL_MAX);
            int64_t lo = 0, hi = 0;
            if (cx >= 0 && cx <= DB_CELL_MAX && cy >= 0 && cy <= DB_CELL_MAX) {
                const uint64_t base = ((uint64_t)cx << (2 * DB_CELL_BITS)) | ((uint64_t)cy << DB_CELL_BITS);
                const int z0 = cz > 0 ? cz - 1 : 0, z1 = cz < DB_CELL_MAX ? cz + 1 : DB_CELL_MAX;
                lo = db_lower_bound(skey, n, base | (uint64_t)z0);
                hi = db_lower_bound(skey, n, (base | (uint64_t)z1) + 1);
            }
            r_lo[tid] = lo; r_hi[tid] = hi;
        }
        __syncthreads();
        const int next = s_next;
        if (s_any) {
            bool more = true;
            for (int r = 0; r < 9 && more; ++r) {
                const int64_t hi = r_hi[r];
                for (int64_t t0 = r_lo[r]; t0 < hi && more; t0 += DB_THREADS) {
                    const int m = (int)((hi - t0) < DB_THREADS ? (hi - t0) : DB_THREADS);
                    __syncthreads();                                                   // the tile before has been read
                    if (tid < m) {
                        const int64_t t = t0 + tid;
#pragma unroll
                        for (int j = 0; j < D; ++j) tile[tid * D + j] = xs[t * D + j];
                        if (PASS >= 2) {
                            const int o = orig[t];
                            const bool c = core_s[t] != 0;
                            aux_row[tid] = o;
                            aux_root[tid] = c ? uf_load(&parent[o]) : (PASS == 2 ? -1 : DB_NONE);
                        }
                    }
                    __syncthreads();
                    if (pending) {
                        for (int c = 0; c < m; ++c) {
                            double d2 = 0.0;
#pragma unroll
                            for (int j = 0; j < D; ++j) { const double df = q[j] - tile[c * D + j]; d2 += df * df; }
                            if (d2 <= eps2) {
                                if (PASS == 1) {
                                    if (++cnt >= min_samples) { pending = false; break; }
                                } else if (PASS == 2) {
                                    const int hint = aux_root[c], j = aux_row[c];
                                    if (hint >= 0 && j < me && hint != myroot) myroot = uf_union(parent, me, j);
                                } else {
                                    const int root = aux_root[c];
                                    minroot = root < minroot ? root : minroot;
                                }
                            }
                        }
                    }
                    if (PASS == 1) more = __syncthreads_or(pending) != 0;             // every row of the cell has its count
                }
            }
        }
        seg = next;
    }
    if (!live) return;
    if (PASS == 1) {
        const int c = cnt >= min_samples;
        core_s[s] = c;
        core_o[me] = c;
    }
    if (PASS == 3) {
        if (core_s[s]) labels[me] = rank[parent[me]];
        else labels[me] = minroot == DB_NONE ? -1 : rank[minroot];
    }
}

// parent[i] = root of i for every core row; flag[i] = 1 for the roots (their number so far is scanned into `rank` below)
__global__ __launch_bounds__(256) void db_flatten_kernel(int32_t* __restrict__ parent, const int32_t* __restrict__ core_o, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !core_o[i]) return;
    uf_find(parent, (int)i);
}
__device__ __forceinline__ int db_is_root(const int32_t* parent, const int32_t* core_o, int64_t i, int64_t n) {
    return i < n && core_o[i] && parent[i] == (int32_t)i;
}
__global__ __launch_bounds__(256) void db_rootcount_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ core_o,
                                                           int64_t n, int32_t* __restrict__ bsum) {
    __shared__ int part[4];
    const int64_t base = (int64_t)blockIdx.x * DB_SCAN_BLOCK;
    int c = 0;
    for (int k = 0; k < DB_SCAN_BLOCK / 256; ++k) c += db_is_root(parent, core_o, base + k * 256 + threadIdx.x, n);
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (lane_id() == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) bsum[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}
// exclusive scan of the block sums in place (one workgroup), the total to *n_clusters
__global__ __launch_bounds__(256) void db_blockscan_kernel(int32_t* __restrict__ bsum, int nblk, int32_t* __restrict__ n_clusters) {
    __shared__ int part[256];
    const int tid = threadIdx.x;
    const int per = (nblk + 255) / 256;
    const int lo = tid * per < nblk ? tid * per : nblk, hi = lo + per < nblk ? lo + per : nblk;
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += bsum[i];
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - sum;
    for (int i = lo; i < hi; ++i) { const int v = bsum[i]; bsum[i] = run; run += v; }
    if (tid == 255) *n_clusters = part[255];
}
// rank[i] = number of roots below row i, for the roots
__global__ __launch_bounds__(256) void db_rank_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ core_o, int64_t n,
                                                      const int32_t* __restrict__ bsum, int32_t* __restrict__ rank) {
    __shared__ int wsum[4];
    __shared__ int carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t base = (int64_t)blockIdx.x * DB_SCAN_BLOCK;
    if (tid == 0) carry = bsum[blockIdx.x];
    for (int k = 0; k < DB_SCAN_BLOCK / 256; ++k) {
        const int64_t i = base + k * 256 + tid;
        const int f = db_is_root(parent, core_o, i, n);
        const uint64_t m = __ballot(f);
        if (lane == 0) wsum[wave] = __builtin_popcountll(m);
        __syncthreads();
        int before = carry + prefix_popc(m);
        for (int w = 0; w < wave; ++w) before += wsum[w];
        if (f) rank[i] = before;
        __syncthreads();
        if (tid == 0) carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
}

struct DbLayout {
    int64_t lo, keys, perm, inv, radix, xs, skey, orig, core_s, core_o, parent, rank, bsum, total;
};
static DbLayout db_layout(int64_t n) {
    DbLayout L;
    int64_t at = 0;
    auto take = [&](int64_t bytes) { const int64_t p = at; at += (bytes + 255) / 256 * 256; return p; };
    L.lo = take(64);
    L.keys = take(n * 8); L.perm = take(n * 8); L.inv = take(n * 8);
    L.radix = take(b2m_radix_argsort_scratch(n));
    L.xs = take(n * 8 * 8);                          // (d <= 8)
    L.skey = take(n * 8);
    L.orig = take(n * 4); L.core_s = take(n * 4); L.core_o = take(n * 4); L.parent = take(n * 4); L.rank = take(n * 4);
    L.bsum = take((cdiv64(n > 0 ? n : 1, DB_SCAN_BLOCK) + 1) * 4);
    L.total = at;
    return L;
}
extern "C" int64_t b2m_dbscan_workspace(int64_t n) {
    if (n < 0 || n >= (1ll << 31)) return -1;
    return db_layout(n).total;
}

template <int D>
static void db_run_passes(hipStream_t st, unsigned nblk, const double* xs, const uint64_t* skey, const int32_t* orig, int64_t n,
                          double eps2, int min_samples, int32_t* core_s, int32_t* core_o, int32_t* parent, int32_t* rank,
                          int32_t* bsum, int32_t* labels, int32_t* n_clusters) {
    db_pass_kernel<D, 1><<<nblk, DB_THREADS, 0, st>>>(xs, skey, orig, n, eps2, min_samples, core_s, core_o, parent, rank, labels);
    db_pass_kernel<D, 2><<<nblk, DB_THREADS, 0, st>>>(xs, skey, orig, n, eps2, min_samples, core_s, core_o, parent, rank, labels);
    db_flatten_kernel<<<(unsigned)cdiv64(n, 256), 256, 0, st>>>(parent, core_o, n);
    const int nscan = (int)cdiv64(n, DB_SCAN_BLOCK);
    db_rootcount_kernel<<<nscan, 256, 0, st>>>(parent, core_o, n, bsum);
    db_blockscan_kernel<<<1, 256, 0, st>>>(bsum, nscan, n_clusters);
    db_rank_kernel<<<nscan, 256, 0, st>>>(parent, core_o, n, bsum, rank);
    db_pass_kernel<D, 3><<<nblk, DB_THREADS, 0, st>>>(xs, skey, orig, n, eps2, min_samples, core_s, core_o, parent, rank, labels);
}

extern "C" int b2m_dbscan(const double* x, int64_t n, int32_t d, double eps, int32_t min_samples, void* workspace,
                          int32_t* labels, int32_t* n_clusters, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(n >= 0 && n < (1ll << 31), "n out of range");
    B2M_CHECK_ARG(d >= 3 && d <= 8, "d must be 3 ... 8");
    B2M_CHECK_ARG(eps > 0.0 && eps < 1e300, "eps must be positive and finite");        // (a NaN fails the first test)
    B2M_CHECK_ARG(min_samples >= 1, "min_samples must be at least 1");
    B2M_CHECK_ARG(n_clusters, "NULL n_clusters");
    if (n == 0) {                                    // nothing to label; no launch (the count is the caller's to zero)
        return B2M_OK;
    }
    B2M_CHECK_ARG(x && workspace && labels, "NULL argument");
    const DbLayout L = db_layout(n);
    char* w = (char*)workspace;
    uint64_t* lo = (uint64_t*)(w + L.lo);
    uint64_t* keys = (uint64_t*)(w + L.keys);
    int64_t* perm = (int64_t*)(w + L.perm);
    int64_t* inv = (int64_t*)(w + L.inv);
    double* xs = (double*)(w + L.xs);
    uint64_t* skey = (uint64_t*)(w + L.skey);
    int32_t* orig = (int32_t*)(w + L.orig);
    int32_t* core_s = (int32_t*)(w + L.core_s);
    int32_t* core_o = (int32_t*)(w + L.core_o);
    int32_t* parent = (int32_t*)(w + L.parent);
    int32_t* rank = (int32_t*)(w + L.rank);
    int32_t* bsum = (int32_t*)(w + L.bsum);
    const unsigned nb256 = (unsigned)cdiv64(n, 256);
    B2M_HIP(hipMemsetAsync(lo, 0xff, 64, st));
    db_min_kernel<<<nb256 < 1024 ? nb256 : 1024, 256, 0, st>>>(x, n, d, lo);
    db_key_kernel<<<nb256, 256, 0, st>>>(x, n, d, eps * (1.0 + 1.0 / 1048576.0), lo, keys);
    const int rc = b2m_radix_argsort(keys, n, 0x7fffffffffffffffull, perm, inv, w + L.radix, stream);
    if (rc != B2M_OK) return rc;
    db_gather_kernel<<<nb256, 256, 0, st>>>(x, n, d, keys, perm, xs, skey, orig, parent);
    const double eps2 = eps * eps;
#define DB_CASE(D_)                                                                                                          \
    case D_: db_run_passes<D_>(st, nb256, xs, skey, orig, n, eps2, min_samples, core_s, core_o, parent, rank, bsum, labels, \
                               n_clusters); break;
    switch (d) { DB_CASE(3) DB_CASE(4) DB_CASE(5) DB_CASE(6) DB_CASE(7) DB_CASE(8) }
#undef DB_CASE
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// ------------------------------------------------------------------ greedy proposal merge (evaluation.py:177-193)
#define PAINT_THREADS 1024
__global__ __launch_bounds__(PAINT_THREADS) void paint_kernel(const uint64_t* __restrict__ bits, int64_t words, int k,
                                                              const int32_t* __restrict__ sem, int64_t n, int sem_min, double ratio,
                                                              int min_points, uint64_t* __restrict__ unlabeled,
                                                              int32_t* __restrict__ inst, int32_t* __restrict__ sem_out,
                                                              int32_t* __restrict__ accepted) {
    __shared__ int part[2][PAINT_THREADS / 64];
    __shared__ int s_take;
    const int tid = threadIdx.x;
    for (int64_t p = tid; p < n; p += PAINT_THREADS) inst[p] = -1;
    for (int64_t w = tid; w < words; w += PAINT_THREADS) {
        const int64_t left = n - w * 64;
        unlabeled[w] = left >= 64 ? ~0ull : ((1ull << left) - 1);
    }
    __syncthreads();
    for (int r = 0; r < k; ++r) {
        const uint64_t* row = bits + (int64_t)r * words;
        const int label = sem[r];
        if (label < sem_min) {                      // (uniform over the workgroup)
            if (tid == 0) accepted[r] = 0;
            continue;
        }
        int o = 0, f = 0;
        for (int64_t w = tid; w < words; w += PAINT_THREADS) {
            const uint64_t m = row[w];
            o += __builtin_popcountll(m);
            f += __builtin_popcountll(m & unlabeled[w]);
        }
        for (int s = 32; s > 0; s >>= 1) { o += __shfl_xor(o, s); f += __shfl_xor(f, s); }
        if ((tid & 63) == 0) { part[0][tid >> 6] = o; part[1][tid >> 6] = f; }
        __syncthreads();
        if (tid == 0) {
            int so = 0, sf = 0;
            for (int w = 0; w < PAINT_THREADS / 64; ++w) { so += part[0][w]; sf += part[1][w]; }
            const bool take = !((double)sf / (double)so < ratio) && !(sf < min_points);
            s_take = take;
            accepted[r] = take;
        }
        __syncthreads();
        if (s_take) {
            for (int64_t w = tid; w < words; w += PAINT_THREADS) {
                const uint64_t u = unlabeled[w];
                uint64_t m = row[w] & u;
                if (!m) continue;
                unlabeled[w] = u & ~m;
                while (m) {
                    const int64_t p = w * 64 + __builtin_ctzll(m);
                    m &= m - 1;
                    inst[p] = r + 1;
                    if (sem_out) sem_out[p] = label;
                }
            }
        }
        __syncthreads();                            // unlabeled / part / s_take are reused by the next row
    }
}
extern "C" int b2m_paint_proposals(const uint64_t* bits, int64_t words, int32_t k, const int32_t* sem, int64_t n, int32_t sem_min,
                                   double ratio, int32_t min_points, uint64_t* unlabeled, int32_t* inst, int32_t* sem_out,
                                   int32_t* accepted, void* stream) {
    B2M_CHECK_ARG(k >= 0 && n >= 0 && n < (1ll << 31) && words == cdiv64(n, 64), "bad sizes (words = ceil(n / 64))");
    if (n == 0) return B2M_OK;
    B2M_CHECK_ARG(unlabeled && inst, "NULL argument");
    B2M_CHECK_ARG(k == 0 || (bits && sem && accepted), "NULL argument");
    paint_kernel<<<1, PAINT_THREADS, 0, (hipStream_t)stream>>>(bits, words, k, sem, n, sem_min, ratio, min_points, unlabeled, inst,
                                                               sem_out, accepted);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// ------------------------------------------------------------------ joint histogram of two index columns
#define JH_LDS 4096
__global__ __launch_bounds__(256) void joint_hist_lds_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ b, int64_t n,
                                                             int na, int nb, int32_t* __restrict__ hist) {
    __shared__ int h[JH_LDS];
    const int cells = na * nb;
    for (int c = threadIdx.x; c < cells; c += 256) h[c] = 0;
    __syncthreads();
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        const int ia = a[p], ib = b ? b[p] : 0;
        if (ia >= 0 && ia < na && ib >= 0 && ib < nb) atomicAdd(&h[ia * nb + ib], 1);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < cells; c += 256)
        if (h[c]) atomicAdd(&hist[c], h[c]);
}
__global__ __launch_bounds__(256) void joint_hist_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ b, int64_t n,
                                                         int na, int nb, int32_t* __restrict__ hist) {
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        const int ia = a[p], ib = b ? b[p] : 0;
        if (ia >= 0 && ia < na && ib >= 0 && ib < nb) atomicAdd(&hist[(int64_t)ia * nb + ib], 1);
    }
}
extern "C" int b2m_joint_hist(const int32_t* a, const int32_t* b, int64_t n, int32_t na, int32_t nb, int32_t* hist, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(n >= 0 && na >= 1 && nb >= 1, "bad sizes");
    B2M_CHECK_ARG((int64_t)na * nb <= B2M_JOINT_HIST_MAX, "table of more than B2M_JOINT_HIST_MAX entries");
    B2M_CHECK_ARG(hist && (n == 0 || a), "NULL argument");
    const int64_t cells = (int64_t)na * nb;
    B2M_HIP(hipMemsetAsync(hist, 0, (size_t)cells * sizeof(int32_t), st));
    if (n == 0) return B2M_OK;
    int64_t blocks = cdiv64(n, 256 * 16);
    if (blocks > 2048) blocks = 2048;
    if (cells <= JH_LDS) joint_hist_lds_kernel<<<(unsigned)blocks, 256, 0, st>>>(a, b, n, na, nb, hist);
    else joint_hist_kernel<<<(unsigned)blocks, 256, 0, st>>>(a, b, n, na, nb, hist);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// ------------------------------------------------------------------ S3DIS threshold sweep: every score prefix of one stage
// (include/b2m.h, b2m_s3dis_prefix_tail).  A (setting x point-chunk) grid; the tables of a setting are privatised in LDS when they
// fit (one global integer add per touched cell and workgroup), else the adds go to global memory.  Integer adds and plain stores
// of one value only: the tables do not depend on the order of the atomics.
#define PT_THREADS 256
#define PT_PER_BLOCK (PT_THREADS * 16)
#define PT_LDS 8192
#define PT_CLASSES 13
struct PtPrefix { int32_t k[B2M_SWEEP_MAX_TH]; };
struct PtLayout { int64_t present, maxid, pair, size, cls, inter, total; };
static PtLayout pt_layout(int64_t k_rows, int64_t n_set, int64_t n_inst, int64_t n_gt) {
    PtLayout L;
    int64_t at = 0;
    auto take = [&](int64_t ints) { const int64_t p = at; at += (ints + 63) / 64 * 64; return p; };
    L.present = take(k_rows > 0 ? k_rows : 1);
    L.maxid = take(n_set);
    L.pair = take(n_set * n_inst * PT_CLASSES);
    L.size = take(n_set * n_inst);
    L.cls = take(n_set * n_inst * PT_CLASSES);
    L.inter = take(n_set * n_inst * (n_gt > 0 ? n_gt : 1));
    L.total = at;
    return L;
}
static bool pt_sizes_ok(int64_t k_rows, int64_t n_set, int64_t n_inst, int64_t n_gt) {
    return k_rows >= 0 && k_rows < (1ll << 31) && n_set >= 1 && n_set <= B2M_SWEEP_MAX_TH && n_inst >= 1 && n_inst < (1ll << 31) &&
           n_gt >= 0 && n_gt < (1ll << 31) && n_set * n_inst <= B2M_JOINT_HIST_MAX &&
           n_set * n_inst * (n_gt > PT_CLASSES ? n_gt : PT_CLASSES) <= B2M_JOINT_HIST_MAX;
}
extern "C" int64_t b2m_s3dis_prefix_tail_workspace(int32_t k_rows, int32_t n_set, int32_t n_inst, int32_t n_gt) {
    if (!pt_sizes_ok(k_rows, n_set, n_inst, n_gt)) return -1;
    return pt_layout(k_rows, n_set, n_inst, n_gt).total * (int64_t)sizeof(int32_t);
}

// the label of sampled point p in a setting before the small pairs go: evaluation.py:192-199 restricted to the owners below k_s
__device__ __forceinline__ void pt_label(const int32_t* __restrict__ owner, const int32_t* __restrict__ prop_sem,
                                         const int32_t* __restrict__ bg, const int32_t* __restrict__ sem, int64_t p, int k_s,
                                         int k_rows, int maxid, int n_inst, int& inst, int& cls) {
    const int o = owner[p];
    const bool painted = o >= 0 && o < k_s && o < k_rows;
    inst = painted ? o + 1 : -1;
    cls = painted ? prop_sem[o] : sem[p];
    const int b = bg[p];
    if (b > 0 && (int64_t)b + maxid > 0) inst = (int64_t)b + maxid < n_inst ? b + maxid : n_inst;
    if (inst >= n_inst) inst = -1;
}

__global__ __launch_bounds__(PT_THREADS) void pt_present_kernel(const int32_t* __restrict__ owner, int64_t n, int k_rows,
                                                                int32_t* __restrict__ present) {
    for (int64_t p = (int64_t)blockIdx.x * PT_THREADS + threadIdx.x; p < n; p += (int64_t)gridDim.x * PT_THREADS) {
        const int o = owner[p];
        if (o >= 0 && o < k_rows) present[o] = 1;   // (every writer stores the same value)
    }
}
// maxid[s] = 1 + the largest owner below k[s] that owns a point, or -1: np.max(pred_instances) of the prefix (evaluation.py:197)
__global__ __launch_bounds__(64) void pt_maxid_kernel(const int32_t* __restrict__ present, PtPrefix pre, int n_set,
                                                      int32_t* __restrict__ maxid) {
    const int s = threadIdx.x;
    if (s >= n_set) return;
    int m = -1;
    for (int o = pre.k[s] - 1; o >= 0; --o)
        if (present[o]) { m = o + 1; break; }
    maxid[s] = m;
}

// table[key] += 1 for every lane with `on`, ONE add per wave and distinct key (the points of a room come in long runs of one
// instance: without this the 64 lanes of a wave queue on one cell).  Every lane of the wave must call it.
__device__ __forceinline__ void pt_wave_add(int32_t* table, int key, bool on) {
    uint64_t todo = __ballot(on);
    while (todo) {                                  // (uniform over the wave)
        const int leader = __builtin_ctzll(todo);
        const int k = __shfl(key, leader);
        const uint64_t same = __ballot(on && key == k);
        if (lane_id() == leader) atomicAdd(&table[k], __builtin_popcountll(same));
        todo &= ~same;
    }
}

// blockIdx.y = setting.  PASS 0: (instance, class) counts over the sampled points.  PASS 1: sizes, class votes and ground-truth
// intersections over the evaluation points, after the pairs under min_points lost their points (evaluation.py:200-222).
template <int PASS, bool LDS>
__global__ __launch_bounds__(PT_THREADS) void pt_count_kernel(const int32_t* __restrict__ owner, const int32_t* __restrict__ prop_sem,
                                                              const int32_t* __restrict__ bg, const int32_t* __restrict__ sem,
                                                              int64_t n, PtPrefix pre, int k_rows, int n_inst, int min_points,
                                                              const int32_t* __restrict__ gi, int n_gt,
                                                              const int64_t* __restrict__ index, int64_t n_eval,
                                                              const int32_t* __restrict__ maxid, int32_t* __restrict__ pair,
                                                              int32_t* __restrict__ size, int32_t* __restrict__ cls_tab,
                                                              int32_t* __restrict__ inter, int label_setting, int32_t* __restrict__ inst_out,
                                                              int32_t* __restrict__ sem_out) {
    __shared__ int h[LDS ? PT_LDS : 1];
    const int s = blockIdx.y;
    const int k_s = pre.k[s], mx = maxid[s];
    const int gw = n_gt > 0 ? n_gt : 1;
    // LDS image of the setting's tables: PASS 0 pair[n_inst][13]; PASS 1 size[n_inst] | cls[n_inst][13] | inter[n_inst][gw]
    const int cells = PASS == 0 ? n_inst * PT_CLASSES : n_inst * (1 + PT_CLASSES + gw);
    const int o_cls = n_inst, o_inter = n_inst * (1 + PT_CLASSES);
    const int32_t* pair_s = pair + (int64_t)s * n_inst * PT_CLASSES;
    if (LDS) {
        for (int c = threadIdx.x; c < cells; c += PT_THREADS) h[c] = 0;
        __syncthreads();
    }
    const int64_t total = PASS == 0 ? n : n_eval;
    // the tables of this setting, in LDS or in global memory; every wave walks the loop as a whole (pt_wave_add ballots)
    int32_t* t_pair = LDS ? h : pair + (int64_t)s * n_inst * PT_CLASSES;
    int32_t* t_size = LDS ? h : size + (int64_t)s * n_inst;
    int32_t* t_cls = LDS ? h + o_cls : cls_tab + (int64_t)s * n_inst * PT_CLASSES;
    int32_t* t_inter = LDS ? h + o_inter : inter + (int64_t)s * n_inst * gw;
    for (int64_t q0 = (int64_t)blockIdx.x * PT_THREADS; q0 < total; q0 += (int64_t)gridDim.x * PT_THREADS) {
        const int64_t q = q0 + threadIdx.x;
        const bool live = q < total;
        int64_t p = q;
        if (PASS == 1 && index && live) p = index[q];
        int inst = -1, c = -1;
        const bool inside = live && p >= 0 && p < n;
        if (inside) pt_label(owner, prop_sem, bg, sem, p, k_s, k_rows, mx, n_inst, inst, c);
        const bool cok = c >= 0 && c < PT_CLASSES;
        if (PASS == 0) {
            pt_wave_add(t_pair, inst * PT_CLASSES + c, inst >= 0 && cok);
            continue;                               // (uniform over the workgroup: PASS is a template argument)
        }
        if (inst >= 0 && cok && pair_s[(int64_t)inst * PT_CLASSES + c] < min_points) inst = -1;
        const int g = live ? gi[q] : -1;
        const bool gok = g >= 0 && g < n_gt;
        if (live && s == label_setting) {
            if (inst_out) inst_out[q] = inst;
            if (sem_out) sem_out[q] = inside ? c : -1;
        }
        pt_wave_add(t_size, inst, inst >= 0);
        pt_wave_add(t_cls, inst * PT_CLASSES + c, inst >= 0 && cok);
        pt_wave_add(t_inter, inst * gw + g, inst >= 0 && gok);
    }
    if (!LDS) return;
    __syncthreads();
    for (int c = threadIdx.x; c < cells; c += PT_THREADS) {
        const int v = h[c];
        if (!v) continue;
        if (PASS == 0) atomicAdd(&pair[(int64_t)s * n_inst * PT_CLASSES + c], v);
        else if (c < o_cls) atomicAdd(&size[(int64_t)s * n_inst + c], v);
        else if (c < o_inter) atomicAdd(&cls_tab[(int64_t)s * n_inst * PT_CLASSES + (c - o_cls)], v);
        else atomicAdd(&inter[(int64_t)s * n_inst * gw + (c - o_inter)], v);
    }
}

// one thread per (setting, instance): class = most frequent rewritten class (lowest on ties, scipy.stats.mode), true positive iff a
// ground-truth instance of that class has inter / union >= 0.5, i.e. 3 * inter >= |P| + |G| (s3dis_util.py:280-296)
__global__ __launch_bounds__(PT_THREADS) void pt_score_kernel(const int32_t* __restrict__ size, const int32_t* __restrict__ cls_tab,
                                                              const int32_t* __restrict__ inter, const int32_t* __restrict__ gsize,
                                                              const int32_t* __restrict__ gt_class, int n_set, int n_inst, int n_gt,
                                                              int32_t* __restrict__ tp, int32_t* __restrict__ fp) {
    const int64_t t = (int64_t)blockIdx.x * PT_THREADS + threadIdx.x;
    if (t >= (int64_t)n_set * n_inst) return;
    const int64_t sz = size[t];
    if (sz <= 0) return;
    const int s = (int)(t / n_inst);
    int best = 0, bc = cls_tab[t * PT_CLASSES];
    for (int c = 1; c < PT_CLASSES; ++c) {
        const int v = cls_tab[t * PT_CLASSES + c];
        if (v > bc) { bc = v; best = c; }
    }
    const int gw = n_gt > 0 ? n_gt : 1;
    bool hit = false;
    for (int g = 0; g < n_gt && !hit; ++g)
        hit = gt_class[g] == best && 3 * (int64_t)inter[t * gw + g] >= sz + (int64_t)gsize[g];
    atomicAdd(hit ? &tp[s * PT_CLASSES + best] : &fp[s * PT_CLASSES + best], 1);
}

extern "C" int b2m_s3dis_prefix_tail(const int32_t* owner, const int32_t* prop_sem, int32_t k_rows, const int32_t* bg,
                                     const int32_t* sem, int64_t n, const int32_t* k_host, int32_t n_set, int32_t n_inst,
                                     int32_t min_points, const int32_t* gi, const int32_t* gt_class, const int32_t* gt_size,
                                     int32_t n_gt, const int64_t* index, int64_t n_eval, void* workspace, int32_t* tp, int32_t* fp,
                                     int32_t label_setting, int32_t* inst_out, int32_t* sem_out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(n_set >= 1 && n_set <= B2M_SWEEP_MAX_TH, "n_set must be 1 ... B2M_SWEEP_MAX_TH");
    B2M_CHECK_ARG(k_host, "NULL k_host");
    B2M_CHECK_ARG(k_rows >= 0 && n >= 0 && n < (1ll << 31) && n_eval >= 0 && n_eval < (1ll << 31) && n_inst >= 1 && n_gt >= 0,
                  "bad sizes");
    PtPrefix pre;
    for (int s = 0; s < n_set; ++s) {
        B2M_CHECK_ARG(k_host[s] >= 0, "negative prefix length");
        B2M_CHECK_ARG(s == 0 || k_host[s] <= k_host[s - 1], "the prefix lengths must not increase");
        pre.k[s] = k_host[s];
    }
    for (int s = n_set; s < B2M_SWEEP_MAX_TH; ++s) pre.k[s] = 0;
    B2M_CHECK_ARG(k_host[0] <= k_rows, "k[0] exceeds the number of proposal rows");
    B2M_CHECK_ARG(pt_sizes_ok(k_rows, n_set, n_inst, n_gt), "tables of more than B2M_JOINT_HIST_MAX entries");
    B2M_CHECK_ARG(label_setting >= -1 && label_setting < n_set, "label_setting must be -1 or a setting");
    if (n == 0 || n_eval == 0) return B2M_OK;       // nothing to score: no launch, nothing written
    B2M_CHECK_ARG(owner && bg && sem && gi && workspace && tp && fp, "NULL argument");
    B2M_CHECK_ARG(k_rows == 0 || prop_sem, "NULL prop_sem");
    B2M_CHECK_ARG(n_gt == 0 || (gt_class && gt_size), "NULL gt_class / gt_size");
    const PtLayout L = pt_layout(k_rows, n_set, n_inst, n_gt);
    int32_t* w = (int32_t*)workspace;
    B2M_HIP(hipMemsetAsync(w, 0, (size_t)L.total * sizeof(int32_t), st));
    auto grid_x = [](int64_t rows) { const int64_t b = cdiv64(rows, PT_PER_BLOCK); return (unsigned)(b > 1024 ? 1024 : b); };
    pt_present_kernel<<<grid_x(n), PT_THREADS, 0, st>>>(owner, n, k_rows, w + L.present);
    pt_maxid_kernel<<<1, 64, 0, st>>>(w + L.present, pre, n_set, w + L.maxid);
    const int gw = n_gt > 0 ? n_gt : 1;
    const bool lds0 = (int64_t)n_inst * PT_CLASSES <= PT_LDS, lds1 = (int64_t)n_inst * (1 + PT_CLASSES + gw) <= PT_LDS;
#define PT_ARGS owner, prop_sem, bg, sem, n, pre, k_rows, n_inst, min_points, gi, n_gt, index, n_eval, w + L.maxid, w + L.pair, \
                w + L.size, w + L.cls, w + L.inter, label_setting, inst_out, sem_out
    const dim3 g0(grid_x(n), (unsigned)n_set), g1(grid_x(n_eval), (unsigned)n_set);
    if (lds0) pt_count_kernel<0, true><<<g0, PT_THREADS, 0, st>>>(PT_ARGS);
    else pt_count_kernel<0, false><<<g0, PT_THREADS, 0, st>>>(PT_ARGS);
    if (lds1) pt_count_kernel<1, true><<<g1, PT_THREADS, 0, st>>>(PT_ARGS);
    else pt_count_kernel<1, false><<<g1, PT_THREADS, 0, st>>>(PT_ARGS);
#undef PT_ARGS
    pt_score_kernel<<<(unsigned)cdiv64((int64_t)n_set * n_inst, PT_THREADS), PT_THREADS, 0, st>>>(
        w + L.size, w + L.cls, w + L.inter, gt_size, gt_class, n_set, n_inst, n_gt, tp, fp);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}
