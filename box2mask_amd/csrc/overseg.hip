// Mesh over-segmentation on the device: the Felzenszwalb graph segmentation the reference runs over a mesh's faces
// (dataprocessing/oversegmentation/cpp/segmentator.cpp), by the rule of profiles/overseg_rule.md.  fp32 throughout, every
// product and sum rounded on its own (the reference is built without FMA), correctly rounded divisions and square roots.
//
//   weights : one thread per vertex runs the reference's running mean of face normals over the vertex's CSR row (the row lists the
//             faces in ascending 3f + slot, the order segmentator.cpp:185-208 visits them in); one thread per edge e = 3f + slot
//             forms the weight and the sort key  code(w) << 32 | e.
//   sort    : b2m_sort_u64 on the keys (voxelize.hip): keys are unique, so this is the (w, e) order.
//   passes  : ONE WAVE per scene.  The recurrence is sequential in the sorted edge order; the wave takes a window of 64 consecutive
//             edges, every lane walks both finds against the forest as it stood at the window's start (independent chains), and the
//             window is then resolved in lane order in registers: a ballot finds the next lane that merges, that lane's roots are
//             broadcast, and every lane that holds the losing root takes the winner and its new size / threshold / rank.  Inside a
//             window only roots are re-parented, so a root found at the window's start stays valid until a broadcast names it.
//   labels  : seg[v] = find(v), one thread per vertex, and the counts.
//
// No spin-waits, no communication between workgroups, every loop bounded: find gives up after OVERSEG_MAX_HOPS hops (union by rank
// allows 31) and raises the scene's error flag.
#include "b2m_common.h"
#include "../../include/b2m_prepare.h"
#pragma clang fp contract(off)

#define OVERSEG_MAX_HOPS 64

struct OversegScene {                  // one record of the table: B2M_OVERSEG_DESC int64 fields (include/b2m_prepare.h)
    const float* pos;       int64_t n_vert;
    const int64_t* faces;   int64_t n_faces;
    const int64_t* row_ptr; const int64_t* face_of;
    float* normals;         float* weights;
    uint64_t* keys;         int64_t n_pad;
    int32_t* edge_a;        int32_t* edge_b;      int64_t n_edges;
    int32_t* parent;        int32_t* rank;        int32_t* size;       float* thr;
    int64_t* seg;           int32_t* out;         int64_t spare;
};
static_assert(sizeof(OversegScene) == B2M_OVERSEG_DESC * sizeof(int64_t), "descriptor layout");

// order-preserving code of a weight: -0 == +0, NaN after everything else (infinities included)
__device__ __forceinline__ uint32_t weight_code(float w) {
    if (w != w) return 0xFFFFFFFFu;
    uint32_t u = __float_as_uint(w);
    if (w == 0.0f) u = 0u;
    return (u >> 31) ? ~u : (u | 0x80000000u);
}

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 load3(const float* __restrict__ p, int64_t i) { return V3{p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__device__ __forceinline__ V3 sub3(V3 a, V3 b) { return V3{(a.x - b.x), (a.y - b.y), (a.z - b.z)}; }
// (a.x*b.x + a.y*b.y) + a.z*b.z, every operation rounded on its own
__device__ __forceinline__ float dot3(V3 a, V3 b) {
    return (((a.x * b.x) + (a.y * b.y)) + (a.z * b.z));
}
__device__ __forceinline__ V3 unit3(V3 c) {
    const float n = sqrtf(dot3(c, c));
    return V3{(c.x / n), (c.y / n), (c.z / n)};
}
// segmentator.cpp:107-112
__device__ __forceinline__ V3 face_normal(V3 p1, V3 p2, V3 p3) {
    const V3 u = sub3(p2, p1), v = sub3(p3, p1);
    V3 c;
    c.x = ((u.y * v.z) - (u.z * v.y));
    c.y = ((u.z * v.x) - (u.x * v.z));
    c.z = ((u.x * v.y) - (u.y * v.x));
    return unit3(c);
}

// ---------------------------------------------------------------- vertex normals: the running mean of segmentator.cpp:203-207
__global__ __launch_bounds__(256) void overseg_normals_kernel(const OversegScene* __restrict__ sc) {
    const OversegScene d = sc[blockIdx.y];
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= d.n_vert) return;
    V3 n{0.0f, 0.0f, 0.0f};
    int64_t r0 = d.row_ptr[v], r1 = d.row_ptr[v + 1];
    const int64_t n_flat = 3 * d.n_faces;
    r0 = r0 < 0 ? 0 : r0;
    r1 = r1 > n_flat ? n_flat : r1;
    int32_t count = 0;
    for (int64_t r = r0; r < r1; ++r) {
        const int64_t f = d.face_of[r];
        if ((uint64_t)f >= (uint64_t)d.n_faces) continue;
        const int64_t i1 = d.faces[3 * f], i2 = d.faces[3 * f + 1], i3 = d.faces[3 * f + 2];
        if ((uint64_t)i1 >= (uint64_t)d.n_vert || (uint64_t)i2 >= (uint64_t)d.n_vert || (uint64_t)i3 >= (uint64_t)d.n_vert) continue;
        const V3 nf = face_normal(load3(d.pos, i1), load3(d.pos, i2), load3(d.pos, i3));
        const float t = (1.0f / ((float)count + 1.0f));
        const float u = (1.0f - t);
        n.x = ((t * nf.x) + (u * n.x));
        n.y = ((t * nf.y) + (u * n.y));
        n.z = ((t * nf.z) + (u * n.z));
        ++count;
    }
    d.normals[3 * v] = n.x; d.normals[3 * v + 1] = n.y; d.normals[3 * v + 2] = n.z;
}

// ---------------------------------------------------------------- edges, weights (segmentator.cpp:197-200, 211-229) and sort keys
__global__ __launch_bounds__(256) void overseg_edges_kernel(const OversegScene* __restrict__ sc) {
    const OversegScene d = sc[blockIdx.y];
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= d.n_pad) return;
    if (e >= d.n_edges) { d.keys[e] = B2M_EMPTY_KEY; return; }
    const int64_t f = e / 3;
    const int slot = (int)(e - 3 * f);
    const int64_t i1 = d.faces[3 * f], i2 = d.faces[3 * f + 1], i3 = d.faces[3 * f + 2];
    int64_t a = slot == 2 ? i3 : i1;
    int64_t b = slot == 1 ? i3 : i2;
    float w;
    if ((uint64_t)a >= (uint64_t)d.n_vert || (uint64_t)b >= (uint64_t)d.n_vert) {      // (the wrapper refuses such faces)
        a = 0; b = 0; w = __uint_as_float(0x7FC00000u);
    } else {
        const V3 na = load3(d.normals, a), nb = load3(d.normals, b);
        const V3 dir = unit3(sub3(load3(d.pos, b), load3(d.pos, a)));
        const float dot = dot3(na, nb);
        const float dot2 = dot3(nb, dir);
        w = (1.0f - dot);
        if (dot2 > 0.0f) w = (w * w);
    }
    d.edge_a[e] = (int32_t)a; d.edge_b[e] = (int32_t)b;
    d.weights[e] = w;
    d.keys[e] = ((uint64_t)weight_code(w) << 32) | (uint64_t)(uint32_t)e;
}

extern "C" int b2m_mesh_edge_weights(const int64_t* desc, int32_t n_scenes, int64_t max_vert, int64_t max_pad, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(n_scenes >= 0 && n_scenes <= 65535, "at most 65535 scenes");
    B2M_CHECK_ARG(max_vert >= 0 && max_vert < (1ll << 31), "a scene has fewer than 2^31 vertices");
    B2M_CHECK_ARG(max_pad >= 0 && max_pad < (1ll << 31), "a scene's padded edge count stays below 2^31 (the sort's limit)");
    if (n_scenes == 0 || (max_vert == 0 && max_pad == 0)) return B2M_OK;
    B2M_CHECK_ARG(desc, "NULL argument");
    if (max_vert)
        overseg_normals_kernel<<<dim3((unsigned)cdiv64(max_vert, 256), (unsigned)n_scenes), 256, 0, st>>>((const OversegScene*)desc);
    if (max_pad)
        overseg_edges_kernel<<<dim3((unsigned)cdiv64(max_pad, 256), (unsigned)n_scenes), 256, 0, st>>>((const OversegScene*)desc);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// keys of caller-made weights (box2mask_amd.oversegment.graph_segment): the same code, padded
__global__ void overseg_keys_kernel(const float* __restrict__ w, int64_t n_edges, uint64_t* __restrict__ keys, int64_t n_pad) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_pad) return;
    keys[e] = e < n_edges ? (((uint64_t)weight_code(w[e]) << 32) | (uint64_t)(uint32_t)e) : B2M_EMPTY_KEY;
}
extern "C" int b2m_edge_sort_keys(const float* weights, int64_t n_edges, uint64_t* keys, int64_t n_pad, void* stream) {
    B2M_CHECK_ARG(n_edges >= 0 && n_pad >= n_edges && n_pad < (1ll << 31), "0 <= n_edges <= n_pad < 2^31");
    if (n_pad == 0) return B2M_OK;
    B2M_CHECK_ARG(keys && (weights || n_edges == 0), "NULL argument");
    overseg_keys_kernel<<<(unsigned)cdiv64(n_pad, 256), 256, 0, (hipStream_t)stream>>>(weights, n_edges, keys, n_pad);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}

// ---------------------------------------------------------------- the forest
// The forest's arrays are read and written through relaxed device-scope atomics: a lane reads what another lane of the wave stored
// one window earlier, and the barrier between two windows orders the two.
__device__ __forceinline__ int32_t ld32(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st32(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float ldf(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void stf(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x, or -1 after OVERSEG_MAX_HOPS hops
__device__ __forceinline__ int32_t overseg_find(const int32_t* parent, int32_t x) {
    for (int hop = 0; hop <= OVERSEG_MAX_HOPS; ++hop) {
        const int32_t p = ld32(parent + x);
        if (p == x) return x;
        x = p;
    }
    return -1;
}

__global__ __launch_bounds__(256) void overseg_init_kernel(const OversegScene* __restrict__ sc, float k) {
    const OversegScene d = sc[blockIdx.y];
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < 4) d.out[v] = 0;
    if (v >= d.n_vert) return;
    d.parent[v] = (int32_t)v; d.rank[v] = 0; d.size[v] = 1; d.thr[v] = k;
}

__device__ __forceinline__ int32_t bcast_i(int32_t v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ float bcast_f(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

// PASS 1: segment_graph (segmentator.cpp:77-89).  PASS 2: the small-segment joins (:237-243) over the same sorted edges.
template <int PASS>
__device__ __forceinline__ bool overseg_pass(const OversegScene& d, float k, int32_t m) {
    const int lane = lane_id();
    const int64_t n_vert = d.n_vert, n_edges = d.n_edges;
    for (int64_t base = 0; base < n_edges; base += 64) {
        const int64_t i = base + lane;
        int32_t A = -1, B = -1;
        float w = 0.0f;
        bool bad = false;
        if (i < n_edges) {
            const uint32_t e = (uint32_t)d.keys[i];
            if ((int64_t)e < n_edges) {
                const int32_t a = d.edge_a[e], b = d.edge_b[e];
                w = d.weights[e];
                if ((uint32_t)a < (uint64_t)n_vert && (uint32_t)b < (uint64_t)n_vert) {
                    A = overseg_find(d.parent, a);
                    B = overseg_find(d.parent, b);
                    bad = A < 0 || B < 0;
                    // (the reference's find stores the root in the vertex it started from: segmentator.cpp:40.  Roots, ranks and
                    // sizes do not depend on it; the shorter chain is what it is for)
                    if (!bad && A != a) st32(d.parent + a, A);
                    if (!bad && B != b) st32(d.parent + b, B);
                } else bad = true;
            } else bad = true;
        }
        if (__ballot(bad)) return false;
        const bool live = A >= 0 && A != B;
        int32_t szA = 0, szB = 0, rkA = 0, rkB = 0;
        float thA = 0.0f, thB = 0.0f;
        if (live) {
            szA = ld32(d.size + A); szB = ld32(d.size + B);
            rkA = ld32(d.rank + A); rkB = ld32(d.rank + B);
            if (PASS == 1) { thA = ldf(d.thr + A); thB = ldf(d.thr + B); }
        }
        // the window in lane order: between two merges no lane's roots change, so the next lane that merges is the first one past
        // the last whose predicate holds now; the lanes in between do not merge, as they would not have at their turn
        uint64_t rest = ~0ull;
        while (rest) {                                                     // (at most 64 rounds: `rest` loses its lowest lane each time)
            const bool pred = PASS == 1 ? (w <= thA && w <= thB) : (szA < m || szB < m);
            const uint64_t go = __ballot(A >= 0 && A != B && pred) & rest;
            if (!go) break;
            const int L = __builtin_amdgcn_readfirstlane(__builtin_ctzll(go));
            rest = L == 63 ? 0ull : (~0ull << (L + 1));
            const int32_t la = bcast_i(A, L), lb = bcast_i(B, L);
            const int32_t lszA = bcast_i(szA, L), lszB = bcast_i(szB, L), lrkA = bcast_i(rkA, L), lrkB = bcast_i(rkB, L);
            // join(la, lb), segmentator.cpp:43-54
            const bool a_wins = lrkA > lrkB;
            const int32_t win = a_wins ? la : lb, lose = a_wins ? lb : la;
            const int32_t nrk = a_wins ? lrkA : lrkB + (lrkA == lrkB ? 1 : 0);
            const int32_t nsz = lszA + lszB;
            float nth = 0.0f;
            if (PASS == 1) nth = (bcast_f(w, L) + (k / (float)nsz));
            if (lane == L) {
                st32(d.parent + lose, win);
                st32(d.size + win, nsz);
                st32(d.rank + win, nrk);
                if (PASS == 1) stf(d.thr + win, nth);
            }
            if (A == lose || A == win) { A = win; szA = nsz; rkA = nrk; thA = nth; }
            if (B == lose || B == win) { B = win; szB = nsz; rkB = nrk; thB = nth; }
        }
        __syncthreads();                       // (one wave: orders this window's stores before the next window's loads)
    }
    return true;
}

__global__ __launch_bounds__(64) void overseg_passes_kernel(const OversegScene* __restrict__ sc, float k, int32_t m, int32_t stages) {
    const OversegScene d = sc[blockIdx.x];
    if (d.n_vert == 0 || d.n_edges == 0) return;
    if (ld32(d.out + 2)) return;                                       // (an earlier stage of this scene gave up)
    bool ok = true;
    if (stages & 1) ok = overseg_pass<1>(d, k, m);
    if (ok && (stages & 2)) ok = overseg_pass<2>(d, k, m);
    if (!ok && lane_id() == 0) st32(d.out + 2, 1);
}

__global__ __launch_bounds__(256) void overseg_labels_kernel(const OversegScene* __restrict__ sc) {
    const OversegScene d = sc[blockIdx.y];
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool root = false, bad = false;
    if (v < d.n_vert) {
        const int32_t r = overseg_find(d.parent, (int32_t)v);
        bad = r < 0;
        root = r == (int32_t)v;
        d.seg[v] = bad ? (int64_t)-1 : (int64_t)r;
    }
    bool nan = false;
    if (v < d.n_edges) { const float w = d.weights[v]; nan = w != w; }
    const uint64_t roots = __ballot(root), nans = __ballot(nan), bads = __ballot(bad);
    if (lane_id() == 0) {
        if (roots) atomicAdd(d.out + 0, (int32_t)__popcll(roots));
        if (nans) atomicAdd(d.out + 1, (int32_t)__popcll(nans));
        if (bads) atomicOr(d.out + 2, 1);
    }
}

extern "C" int b2m_graph_segment(const int64_t* desc, int32_t n_scenes, int64_t max_vert, int64_t max_edges, float k_thresh,
                                 int32_t seg_min_verts, int32_t stages, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    B2M_CHECK_ARG(n_scenes >= 0 && n_scenes <= 65535, "at most 65535 scenes");
    B2M_CHECK_ARG(max_vert >= 0 && max_vert < (1ll << 31), "a scene has fewer than 2^31 vertices");
    B2M_CHECK_ARG(max_edges >= 0 && max_edges < (1ll << 31), "a scene has fewer than 2^31 edges (the sort's limit)");
    B2M_CHECK_ARG(stages >= 1 && stages <= 7, "stages: 1 = initialise + pass one, 2 = pass two, 4 = labels and counts");
    if (n_scenes == 0 || max_vert == 0) return B2M_OK;
    B2M_CHECK_ARG(desc, "NULL argument");
    const int64_t span = max_vert > max_edges ? max_vert : max_edges;
    if (stages & 1)
        overseg_init_kernel<<<dim3((unsigned)cdiv64(max_vert < 4 ? 4 : max_vert, 256), (unsigned)n_scenes), 256, 0, st>>>(
            (const OversegScene*)desc, k_thresh);
    if ((stages & 3) && max_edges)
        overseg_passes_kernel<<<(unsigned)n_scenes, 64, 0, st>>>((const OversegScene*)desc, k_thresh, seg_min_verts, stages);
    if (stages & 4)
        overseg_labels_kernel<<<dim3((unsigned)cdiv64(span, 256), (unsigned)n_scenes), 256, 0, st>>>((const OversegScene*)desc);
    B2M_LAUNCH_CHECK();
    return B2M_OK;
}
