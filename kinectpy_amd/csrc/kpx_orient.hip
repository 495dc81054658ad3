// kpx_orient.hip -- normal orientation ([O3D] PointCloud::NormalizeNormals, OrientNormalsToAlignWithDirection,
// OrientNormalsTowardsCameraLocation, OrientNormalsConsistentTangentPlane) and the exact Euclidean minimum spanning tree the last one
// is built on.  Arithmetic contract AC17, DESIGN.md 5.18.
//   elementwise: one streaming kernel, a thread per normal.
//   Boruvka rounds as a chain of plain launches (no grid barrier): every component takes its minimum outgoing edge under a strict total
//            order in TWO atomicMin passes -- first the 64-bit weight into the slot of the component's root, then, among the edges that
//            carry that weight, the packed pair (a << 32 | b) -- so no edge is ever ranked by a sort.  Then hook (the only cycles of a
//            strict order are mutual pairs: the lower root stays), compress (read-only walk up the hooks of this round), one word back.
//   EMST:    the candidates of a round come from the points' kNN rows (kpx_search_knn of the cloud on itself, ascending in
//            (d2, index)) through cursors that only advance.  A point whose row is used up searches exactly -- a walk of the search
//            index's grid bounded by its component's candidate, or all points when the component has none -- unless the last entry
//            of its row already lies strictly beyond that candidate (5.18: why this cannot change a result).
//   T:       the same rounds over the implicit edge list (kNN rows + EMST) under (1 - |dot|, a, b), the union-find carrying one parity
//            bit per vertex = its flip relative to the root of its component.
#include <vector>

#include "kpx_searchview.h"
#include "kpx_sort.h"

namespace kpx {

constexpr int kOrientThreads = 256;
constexpr unsigned long long kNoEdge = ~0ull;
constexpr int kBoruvkaMaxRounds = 64;                       // a round at least halves the components: 31 suffice below 2^31 points
// device counters of a call (unsigned long long [8]); [0..4] in the order of the header's h_stats, without the two round counts
enum { kCtrEdges = 0, kCtrBounded = 1, kCtrUnbounded = 2, kCtrZero = 4, kCtrRoot = 5, kCtrRootFlip = 6, kCtrWords = 8 };

static inline unsigned orient_blocks(int64_t items)
{
    const int64_t b = cdiv(items > 0 ? items : 1, kOrientThreads);
    return (unsigned)(b > 16384 ? 16384 : b);
}

// AC17: every product and sum rounded separately (the library is built with -ffp-contract=off)
__device__ __host__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) { return (ax * bx + ay * by) + az * bz; }
__device__ __forceinline__ double normal_dot(const float *__restrict__ nrm, int32_t a, int32_t b)
{
    const float *pa = nrm + 3 * (int64_t)a, *pb = nrm + 3 * (int64_t)b;
    return dot3((double)pa[0], (double)pa[1], (double)pa[2], (double)pb[0], (double)pb[1], (double)pb[2]);
}
__device__ __forceinline__ unsigned long long pack_pair(int32_t u, int32_t v)
{
    const uint32_t a = (uint32_t)(u < v ? u : v), b = (uint32_t)(u < v ? v : u);
    return (unsigned long long)a << 32 | b;
}
__device__ __forceinline__ unsigned long long slot_load(const unsigned long long *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// atomicMin that stays off the atomic unit when the slot already holds something smaller (a stale read only costs the atomic)
__device__ __forceinline__ void slot_min(unsigned long long *p, unsigned long long v)
{
    if (v < slot_load(p)) atomicMin(p, v);
}

// ---- elementwise ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kOrientThreads) void orient_elementwise_kernel(const float *__restrict__ pts, float *__restrict__ nrm, int64_t n, int mode,
                                                                            double rx, double ry, double rz)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float *o = nrm + 3 * i;
        const float fx = o[0], fy = o[1], fz = o[2];
        const double x = (double)fx, y = (double)fy, z = (double)fz;
        const double len = sqrt(dot3(x, y, z, x, y, z));
        if (mode == KPX_ORIENT_NORMALIZE) {
            if (len > 0.0) { o[0] = (float)(x / len); o[1] = (float)(y / len); o[2] = (float)(z / len); }
            continue;
        }
        double ax = rx, ay = ry, az = rz;                   // the vector the normal has to agree with
        if (mode == KPX_ORIENT_CAMERA) { ax = rx - (double)pts[3 * i]; ay = ry - (double)pts[3 * i + 1]; az = rz - (double)pts[3 * i + 2]; }
        if (len == 0.0) {
            if (mode == KPX_ORIENT_CAMERA) {
                const double rl = sqrt(dot3(ax, ay, az, ax, ay, az));
                if (rl == 0.0) { ax = 0.0; ay = 0.0; az = 1.0; }
                else { ax /= rl; ay /= rl; az /= rl; }
            }
            o[0] = (float)ax; o[1] = (float)ay; o[2] = (float)az;
        } else if (dot3(x, y, z, ax, ay, az) < 0.0) {
            o[0] = -fx; o[1] = -fy; o[2] = -fz;
        }
    }
}

// ---- the rounds' shared state -------------------------------------------------------------------------------------------------------------
struct Forest {
    int32_t *comp;                     // root of every vertex, compressed at the end of a round
    uint8_t *par;                      // T: flip of the vertex relative to its root
    unsigned long long *best_w;        // slot of a root: the smallest weight leaving its component this round
    unsigned long long *best_ab;       // ... and the smallest pair among the edges of that weight
    int32_t *hookto;                   // roots of this round: the root hooked under (itself: stays a root)
    uint8_t *hookpar;
    unsigned long long *edges;         // the tree's packed pairs in the order they were taken
    unsigned long long *ctr;           // kCtrWords counters
};
static void forest_carve(Arena &a, int64_t n, uint64_t *edges, unsigned long long *ctr, Forest *f)
{
    const size_t nn = (size_t)(n > 0 ? n : 1);
    f->comp = a.get<int32_t>(nn);
    f->par = a.get<uint8_t>(nn);
    f->best_w = a.get<unsigned long long>(nn);
    f->best_ab = a.get<unsigned long long>(nn);
    f->hookto = a.get<int32_t>(nn);
    f->hookpar = a.get<uint8_t>(nn);
    f->edges = reinterpret_cast<unsigned long long *>(edges);
    f->ctr = ctr;
}

__global__ __launch_bounds__(kOrientThreads) void forest_init_kernel(Forest f, int64_t n, int32_t *__restrict__ cursor, int32_t *__restrict__ cand_u)
{
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        f.comp[v] = (int32_t)v;
        f.par[v] = 0;
        f.best_w[v] = kNoEdge;
        f.best_ab[v] = kNoEdge;
        if (cursor) { cursor[v] = 0; cand_u[v] = -1; }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) f.ctr[kCtrEdges] = 0ull;
}

// A root with an outgoing edge hooks under the root at the edge's other end; of two roots that took the same edge the lower one stays.
// Under a strict total order these pairs are the only cycles of the "minimum outgoing edge" graph, so the hooks form a forest and
// every edge is taken once: at most n - 1 in all.
template <bool kParity>
__global__ __launch_bounds__(kOrientThreads) void forest_hook_kernel(Forest f, int64_t n, const float *__restrict__ nrm)
{
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (int64_t)gridDim.x * blockDim.x) {
        if (f.comp[c] != (int32_t)c) continue;
        const unsigned long long ab = f.best_ab[c];
        int32_t to = (int32_t)c;
        uint8_t p = 0;
        if (ab != kNoEdge) {
            const int32_t a = (int32_t)(ab >> 32), b = (int32_t)(uint32_t)ab;
            const int32_t ca = f.comp[a], cb = f.comp[b];
            const int32_t other = ca == (int32_t)c ? cb : ca;
            if (!(f.best_ab[other] == ab && (int32_t)c < other)) {
                to = other;
                if (kParity) {
                    const double d = normal_dot(nrm, a, b);
                    p = (uint8_t)(f.par[a] ^ f.par[b] ^ (d < 0.0 ? 1 : 0));
                    if (d == 0.0) atomicAdd(f.ctr + kCtrZero, 1ull);
                }
                const unsigned long long pos = atomicAdd(f.ctr + kCtrEdges, 1ull);
                if (pos < (unsigned long long)(n - 1)) f.edges[pos] = ab;
            }
        }
        f.hookto[c] = to;
        f.hookpar[c] = p;
    }
}
// every vertex walks from its old root up this round's hooks (only old roots are visited, and their hooks form a forest)
__global__ __launch_bounds__(kOrientThreads) void forest_compress_kernel(Forest f, int64_t n)
{
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        int32_t c = f.comp[v];
        uint8_t p = f.par[v];
        for (int64_t step = 0; step < n; ++step) {
            const int32_t h = f.hookto[c];
            if (h == c) break;
            p ^= f.hookpar[c];
            c = h;
        }
        f.comp[v] = c;
        f.par[v] = p;
        f.best_w[v] = kNoEdge;
        f.best_ab[v] = kNoEdge;
    }
}

// hook, compress, and the number of edges taken so far back on the host
template <bool kParity>
static int forest_close_round(const Forest &f, int64_t n, const float *nrm, hipStream_t st, int64_t *taken)
{
    hipLaunchKernelGGL(forest_hook_kernel<kParity>, dim3(orient_blocks(n)), dim3(kOrientThreads), 0, st, f, n, nrm);
    hipLaunchKernelGGL(forest_compress_kernel, dim3(orient_blocks(n)), dim3(kOrientThreads), 0, st, f, n);
    KPX_LAUNCH_CHECK();
    unsigned long long cnt = 0;
    KPX_HIP(hipMemcpyAsync(&cnt, f.ctr + kCtrEdges, sizeof(cnt), hipMemcpyDeviceToHost, st));
    KPX_HIP(hipStreamSynchronize(st));
    *taken = (int64_t)cnt;
    return KPX_OK;
}

// ---- EMST ---------------------------------------------------------------------------------------------------------------------------------
struct EmstScratch {
    char *index, *search_ws;
    size_t index_bytes, search_ws_bytes;
    int32_t *rows_idx, *rows_cnt;      // [n][kk], [n]: kpx_search_knn of the cloud on itself, kk = min(k, n)
    double *rows_d2;
    int32_t *cursor, *cand_u;          // first row entry in a foreign component; this round's candidate (-1: none)
    unsigned long long *cand_d;
    unsigned long long *ctr;
    DeviceSort<uint64_t, false> sort;  // keys_in = the tree's pairs as taken, keys_out = ascending
    Forest f;
};
static void emst_carve(Arena &a, int64_t n, int kk, EmstScratch *s)
{
    const size_t nn = (size_t)(n > 0 ? n : 1), rows = nn * (size_t)(kk > 0 ? kk : 1);
    s->index_bytes = kpx_search_index_bytes(n);
    s->index = a.get<char>(s->index_bytes);
    const size_t wb = kpx_search_workspace_bytes(n, 0), wq = kpx_search_workspace_bytes(n, kk > 0 ? kk : 1);
    s->search_ws_bytes = wb > wq ? wb : wq;
    s->search_ws = a.get<char>(s->search_ws_bytes);
    s->rows_idx = a.get<int32_t>(rows);
    s->rows_d2 = a.get<double>(rows);
    s->rows_cnt = a.get<int32_t>(nn);
    s->cursor = a.get<int32_t>(nn);
    s->cand_u = a.get<int32_t>(nn);
    s->cand_d = a.get<unsigned long long>(nn);
    s->ctr = a.get<unsigned long long>(kCtrWords);
    dsort_carve(a, n - 1, 64, SortOptions(), &s->sort);
    forest_carve(a, n, s->sort.keys_in, s->ctr, &s->f);
}

__global__ __launch_bounds__(kOrientThreads) void emst_cursor_kernel(Forest f, int64_t n, int kk, const int32_t *__restrict__ rows_idx,
                                                                     const double *__restrict__ rows_d2, int32_t *__restrict__ cursor,
                                                                     int32_t *__restrict__ cand_u, unsigned long long *__restrict__ cand_d)
{
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        const int32_t c = f.comp[v];
        const int32_t *row = rows_idx + v * kk;
        int cur = cursor[v];
        while (cur < kk) {
            const int32_t u = row[cur];
            if (u < 0) { cur = kk; break; }                                     // (a row cut short: a query that is not finite)
            if (f.comp[u] != c) break;
            ++cur;
        }
        cursor[v] = cur;
        if (cur < kk) {
            const unsigned long long d = (unsigned long long)__double_as_longlong(rows_d2[v * kk + cur]);      // d2 >= 0: the patterns order like the values
            cand_u[v] = row[cur];
            cand_d[v] = d;
            slot_min(f.best_w + c, d);
        } else {
            cand_u[v] = -1;
        }
    }
}
// The points whose rows are used up.  Every foreign point of such a point v lies beyond its row: d2 >= L_v, the row's last d2.  With
// B = a d2 some member of v's component has already offered this round, L_v > B means v can neither beat nor tie the component's
// minimum; otherwise v finds its nearest foreign point under (d2, index) among those with d2 <= B -- a grid walk -- or, when nobody
// has offered anything (B = none: the component is closed under its rows), among all points.
__global__ __launch_bounds__(kOrientThreads) void emst_search_kernel(Forest f, int64_t n, int kk, const double *__restrict__ rows_d2,
                                                                     SearchView view, const float *__restrict__ pts, int32_t *__restrict__ cand_u,
                                                                     unsigned long long *__restrict__ cand_d)
{
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        if (cand_u[v] >= 0 || (int64_t)kk >= n) continue;                      // (a row of all n points has no foreign point left to miss)
        const unsigned long long lv = kk > 0 ? (unsigned long long)__double_as_longlong(rows_d2[v * kk + kk - 1]) : 0ull;
        const int32_t c = f.comp[v];
        const unsigned long long bound = slot_load(f.best_w + c);
        if (lv > bound) continue;
        const double q[3] = { (double)pts[3 * v], (double)pts[3 * v + 1], (double)pts[3 * v + 2] };
        unsigned long long bd = kNoEdge;
        int32_t bu = INT_MAX;
        if (bound == kNoEdge) {
            for (int64_t j = 0; j < n; ++j) {
                if (f.comp[j] == c) continue;
                const double dx = q[0] - (double)pts[3 * j], dy = q[1] - (double)pts[3 * j + 1], dz = q[2] - (double)pts[3 * j + 2];
                const unsigned long long d = (unsigned long long)__double_as_longlong(fma(dz, dz, fma(dy, dy, dx * dx)));
                if (d < bd) { bd = d; bu = (int32_t)j; }                        // (j ascends: of equal distances the lowest index stays)
            }
            atomicAdd(f.ctr + kCtrUnbounded, 1ull);
        } else {
            unsigned long long lim = bound;
            grid_radius_scan(view.g, view.cell_start, view.spts, q, sqrt(__longlong_as_double((long long)bound)), INFINITY, [&](uint32_t s, double d2) {
                const unsigned long long d = (unsigned long long)__double_as_longlong(d2);
                if (d > lim) return false;
                const int32_t u = view.sidx[s];
                if (f.comp[u] == c) return false;
                if (d < bd || (d == bd && u < bu)) { bd = d; bu = u; lim = d; }
                return false;
            });
            atomicAdd(f.ctr + kCtrBounded, 1ull);
        }
        if (bu != INT_MAX) {
            cand_u[v] = bu;
            cand_d[v] = bd;
            slot_min(f.best_w + c, bd);
        }
    }
}
__global__ __launch_bounds__(kOrientThreads) void emst_pair_kernel(Forest f, int64_t n, const int32_t *__restrict__ cand_u,
                                                                   const unsigned long long *__restrict__ cand_d)
{
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        const int32_t u = cand_u[v];
        if (u < 0) continue;
        const int32_t c = f.comp[v];
        if (cand_d[v] == f.best_w[c]) slot_min(f.best_ab + c, pack_pair((int32_t)v, u));
    }
}

// leaves the tree's n - 1 packed pairs in s.f.edges (= s.sort.keys_in) in the order they were taken; n >= 2
static int emst_run(const float *pts, int64_t n, int kk, const EmstScratch &s, hipStream_t st, int64_t *rounds)
{
    const unsigned nb = orient_blocks(n);
    KPX_HIP(hipMemsetAsync(s.ctr, 0, kCtrWords * sizeof(unsigned long long), st));
    int rc = kpx_search_index_build(pts, n, s.index, s.index_bytes, s.search_ws, s.search_ws_bytes, st);
    if (rc) return rc;
    SearchView view;                                       // (the exact search walks the index's grid whatever kk is)
    rc = search_open(s.index, s.index_bytes, st, &view);
    if (rc) return rc;
    if (kk > 0) {
        rc = kpx_search_knn(s.index, s.index_bytes, pts, n, kk, 0.0, s.rows_idx, s.rows_d2, s.rows_cnt, s.search_ws, s.search_ws_bytes, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(forest_init_kernel, dim3(nb), dim3(kOrientThreads), 0, st, s.f, n, s.cursor, s.cand_u);
    int64_t taken = 0;
    *rounds = 0;
    while (taken < n - 1) {
        KPX_REQUIRE(*rounds < kBoruvkaMaxRounds, "kpx_emst: %lld of %lld edges after %d rounds", (long long)taken, (long long)(n - 1), kBoruvkaMaxRounds);
        // (kk = 0 too: it withdraws last round's candidates)
        hipLaunchKernelGGL(emst_cursor_kernel, dim3(nb), dim3(kOrientThreads), 0, st, s.f, n, kk, (const int32_t *)s.rows_idx, (const double *)s.rows_d2, s.cursor,
                           s.cand_u, s.cand_d);
        hipLaunchKernelGGL(emst_search_kernel, dim3(nb), dim3(kOrientThreads), 0, st, s.f, n, kk, (const double *)s.rows_d2, view, pts, s.cand_u, s.cand_d);
        hipLaunchKernelGGL(emst_pair_kernel, dim3(nb), dim3(kOrientThreads), 0, st, s.f, n, (const int32_t *)s.cand_u, (const unsigned long long *)s.cand_d);
        const int64_t before = taken;
        rc = forest_close_round<false>(s.f, n, nullptr, st, &taken);
        if (rc) return rc;
        ++*rounds;
        KPX_REQUIRE(taken > before && taken <= n - 1, "kpx_emst: a round took %lld edges", (long long)(taken - before));
    }
    return KPX_OK;
}

__global__ __launch_bounds__(kOrientThreads) void unpack_pairs_kernel(const unsigned long long *__restrict__ keys, int64_t m, int32_t *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        out[2 * i] = (int32_t)(keys[i] >> 32);
        out[2 * i + 1] = (int32_t)(uint32_t)keys[i];
    }
}
// the pairs of s.keys_in ascending -> rows (a, b) of out
static int pairs_out(const DeviceSort<uint64_t, false> &s, int64_t m, int32_t *out, hipStream_t st)
{
    const int rc = dsort_run(s, m, 64, st);
    if (rc) return rc;
    hipLaunchKernelGGL(unpack_pairs_kernel, dim3(orient_blocks(m)), dim3(kOrientThreads), 0, st, (const unsigned long long *)s.keys_out, m, out);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

// ---- the orientation tree T -----------------------------------------------------------------------------------------------------------------
// w = 1 - |dot| may be negative (normals longer than 1): the pattern of a double mapped so that it orders like the value
__device__ __forceinline__ unsigned long long weight_key(const float *__restrict__ nrm, int32_t a, int32_t b)
{
    const double w = 1.0 - fabs(normal_dot(nrm, a, b));
    const unsigned long long bits = (unsigned long long)__double_as_longlong(w);
    return (bits >> 63) ? ~bits : (bits | 1ull << 63);
}
// edge `slot` of the Riemannian graph: the first kk entries of every kNN row (rows of `stride` entries), then the EMST; false: no edge
// there (padding, the point itself)
__device__ __forceinline__ bool graph_edge(int64_t slot, int64_t n, int kk, int stride, const int32_t *__restrict__ rows_idx,
                                           const unsigned long long *__restrict__ emst, int32_t *a, int32_t *b)
{
    const int64_t in_rows = n * kk;
    if (slot < in_rows) {
        const int32_t v = (int32_t)(slot / kk), u = rows_idx[(int64_t)v * stride + (slot % kk)];
        if (u < 0 || u == v) return false;
        *a = u < v ? u : v;
        *b = u < v ? v : u;
        return true;
    }
    const unsigned long long ab = emst[slot - in_rows];
    *a = (int32_t)(ab >> 32);
    *b = (int32_t)(uint32_t)ab;
    return true;
}
// kPairs = false: the weights into the roots' slots; true: the pairs of the edges that carry their component's weight
template <bool kPairs>
__global__ __launch_bounds__(kOrientThreads) void tree_offer_kernel(Forest f, int64_t n, int kk, int stride, const int32_t *__restrict__ rows_idx,
                                                                    const unsigned long long *__restrict__ emst, const float *__restrict__ nrm)
{
    const int64_t m = n * kk + (n - 1);
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < m; s += (int64_t)gridDim.x * blockDim.x) {
        int32_t a, b;
        if (!graph_edge(s, n, kk, stride, rows_idx, emst, &a, &b)) continue;
        const int32_t ca = f.comp[a], cb = f.comp[b];
        if (ca == cb) continue;
        const unsigned long long w = weight_key(nrm, a, b);
        if (!kPairs) {
            slot_min(f.best_w + ca, w);
            slot_min(f.best_w + cb, w);
        } else {
            const unsigned long long ab = (unsigned long long)(uint32_t)a << 32 | (uint32_t)b;
            if (w == f.best_w[ca]) slot_min(f.best_ab + ca, ab);
            if (w == f.best_w[cb]) slot_min(f.best_ab + cb, ab);
        }
    }
}

// the lowest index among the points of maximal z: one atomicMax on (z in an order-preserving pattern, ~index); -0.0 counts as +0.0
__global__ __launch_bounds__(kOrientThreads) void orient_root_kernel(const float *__restrict__ pts, int64_t n, unsigned long long *__restrict__ ctr)
{
    unsigned long long best = 0ull;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t bits = __float_as_uint(pts[3 * v + 2] + 0.0f);
        const uint32_t zk = (bits >> 31) ? ~bits : (bits | 0x80000000u);
        const unsigned long long key = (unsigned long long)zk << 32 | (0xFFFFFFFFu - (uint32_t)v);
        best = key > best ? key : best;
    }
    best = wave_max(best);
    if (lane_id() == 0 && best) atomicMax(ctr + kCtrRoot, best);
}
// what the vertices' parities are relative to, once the forest is one component: the root's own sign
__global__ void orient_root_flip_kernel(Forest f, const float *__restrict__ nrm)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int32_t r = (int32_t)(0xFFFFFFFFu - (uint32_t)f.ctr[kCtrRoot]);
        f.ctr[kCtrRootFlip] = (unsigned long long)((nrm[3 * (int64_t)r + 2] < 0.0f ? 1 : 0) ^ f.par[r]);
    }
}
// host_flips == NULL: flip = parity ^ kCtrRootFlip
__global__ __launch_bounds__(kOrientThreads) void orient_apply_kernel(Forest f, int64_t n, float *__restrict__ nrm, const uint8_t *__restrict__ host_flips,
                                                                      uint8_t *__restrict__ flips)
{
    const uint8_t base = (uint8_t)f.ctr[kCtrRootFlip];
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t x = host_flips ? host_flips[v] : (uint8_t)(base ^ f.par[v]);
        if (flips) flips[v] = x;
        if (x) { nrm[3 * v] = -nrm[3 * v]; nrm[3 * v + 1] = -nrm[3 * v + 1]; nrm[3 * v + 2] = -nrm[3 * v + 2]; }
    }
}

struct TangentScratch {
    EmstScratch e;
    unsigned long long *emst;          // the EMST's pairs (the rounds of T reuse the sort's keys_in for T's own)
    uint8_t *host_flips;
    Forest f;
};
static void tangent_carve(Arena &a, int64_t n, int kk, TangentScratch *s)
{
    emst_carve(a, n, kk, &s->e);
    const size_t nn = (size_t)(n > 0 ? n : 1);
    s->emst = a.get<unsigned long long>(nn);
    s->host_flips = a.get<uint8_t>(nn);
    forest_carve(a, n, s->e.sort.keys_in, s->e.ctr, &s->f);
}

// Open3D's breadth-first walk over T from r, on the host: only when T holds an edge with c == 0, whose rule is directional
static void walk_signs(const std::vector<unsigned long long> &tree, const std::vector<float> &nrm, int64_t n, int32_t r, std::vector<uint8_t> &flips)
{
    std::vector<int64_t> start((size_t)n + 1, 0);
    for (unsigned long long ab : tree) { ++start[(size_t)(ab >> 32) + 1]; ++start[(size_t)(uint32_t)ab + 1]; }
    for (int64_t v = 0; v < n; ++v) start[(size_t)v + 1] += start[(size_t)v];
    std::vector<int32_t> adj(2 * tree.size());
    std::vector<int64_t> fill(start.begin(), start.end() - 1);
    for (unsigned long long ab : tree) {
        const int32_t a = (int32_t)(ab >> 32), b = (int32_t)(uint32_t)ab;
        adj[(size_t)fill[(size_t)a]++] = b;
        adj[(size_t)fill[(size_t)b]++] = a;
    }
    std::vector<uint8_t> seen((size_t)n, 0);
    std::vector<int32_t> queue;
    queue.reserve((size_t)n);
    flips.assign((size_t)n, 0);
    flips[(size_t)r] = nrm[3 * (size_t)r + 2] < 0.0f ? 1 : 0;
    seen[(size_t)r] = 1;
    queue.push_back(r);
    for (size_t head = 0; head < queue.size(); ++head) {
        const int32_t a = queue[head];
        const float *pa = nrm.data() + 3 * (size_t)a;
        for (int64_t e = start[(size_t)a]; e < start[(size_t)a + 1]; ++e) {
            const int32_t b = adj[(size_t)e];
            if (seen[(size_t)b]) continue;
            seen[(size_t)b] = 1;
            const float *pb = nrm.data() + 3 * (size_t)b;
            const double c = dot3((double)pa[0], (double)pa[1], (double)pa[2], (double)pb[0], (double)pb[1], (double)pb[2]);
            flips[(size_t)b] = c == 0.0 ? 0 : (uint8_t)(flips[(size_t)a] ^ (c < 0.0 ? 1 : 0));
            queue.push_back(b);
        }
    }
}

// The EMST does not depend on the width of the rows it works from, its time does (5.18): the tangent-plane call searches rows of at
// least kTangentRow entries and the graph takes the first min(k, n) of each.
constexpr int kTangentRow = 30;
static inline int tangent_row(int64_t n, int32_t k)
{
    const int64_t w = k > kTangentRow ? k : kTangentRow;
    return (int)(w < n ? w : n);
}

static int orient_size_check(const char *who, int64_t n, int32_t k)
{
    KPX_REQUIRE(n >= 0, "%s: bad size", who);
    if (n >= ((int64_t)1 << 31)) return fail(KPX_ERR_RANGE, "%s: %lld points, more than 2^31 - 1", who, (long long)n);
    KPX_REQUIRE(k >= 0 && k <= KPX_ORIENT_MAX_K, "%s: k must lie in [0, %d]", who, KPX_ORIENT_MAX_K);
    return KPX_OK;
}

}  // namespace kpx

using namespace kpx;

KPX_EXPORT int kpx_orient_normals(const float *pts, float *normals, int64_t n, int32_t mode, const double *h_ref, void *stream)
{
    KPX_REQUIRE(mode == KPX_ORIENT_NORMALIZE || mode == KPX_ORIENT_DIRECTION || mode == KPX_ORIENT_CAMERA, "kpx_orient_normals: unknown mode %d", (int)mode);
    const int rc = orient_size_check("kpx_orient_normals", n, 0);
    if (rc) return rc;
    KPX_REQUIRE(mode == KPX_ORIENT_NORMALIZE || h_ref, "kpx_orient_normals: null reference");
    if (n == 0) return KPX_OK;
    KPX_REQUIRE(normals && (pts || mode != KPX_ORIENT_CAMERA), "kpx_orient_normals: null pointer");
    const double r[3] = { h_ref ? h_ref[0] : 0.0, h_ref ? h_ref[1] : 0.0, h_ref ? h_ref[2] : 0.0 };
    hipLaunchKernelGGL(orient_elementwise_kernel, dim3(orient_blocks(n)), dim3(kOrientThreads), 0, (hipStream_t)stream, pts, normals, n, (int)mode, r[0], r[1],
                       r[2]);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT size_t kpx_emst_workspace_bytes(int64_t n, int32_t k)
{
    if (n < 0 || n >= ((int64_t)1 << 31) || k < 0 || k > KPX_ORIENT_MAX_K) return 0;
    Arena a(nullptr, 0);
    EmstScratch s;
    emst_carve(a, n, (int)((int64_t)k < n ? k : n), &s);
    return a.off;
}

KPX_EXPORT int kpx_emst(const float *pts, int64_t n, int32_t k, int32_t *edges, int64_t *h_stats, void *ws, size_t ws_bytes, void *stream)
{
    int rc = orient_size_check("kpx_emst", n, k);
    if (rc) return rc;
    if (h_stats) memset(h_stats, 0, 8 * sizeof(int64_t));
    if (n < 2) return KPX_OK;
    KPX_REQUIRE(pts && edges && ws, "kpx_emst: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int kk = (int)((int64_t)k < n ? k : n);
    Arena a(ws, ws_bytes);
    EmstScratch s;
    emst_carve(a, n, kk, &s);
    KPX_ARENA_CHECK(a);
    int64_t rounds = 0;
    rc = emst_run(pts, n, kk, s, st, &rounds);
    if (rc) return rc;
    rc = pairs_out(s.sort, n - 1, edges, st);
    if (rc) return rc;
    unsigned long long ctr[kCtrWords];
    KPX_HIP(hipMemcpyAsync(ctr, s.ctr, sizeof(ctr), hipMemcpyDeviceToHost, st));
    KPX_HIP(hipStreamSynchronize(st));
    if (h_stats) { h_stats[0] = rounds; h_stats[1] = (int64_t)ctr[kCtrBounded]; h_stats[2] = (int64_t)ctr[kCtrUnbounded]; }
    return KPX_OK;
}

KPX_EXPORT size_t kpx_orient_normals_tangent_workspace_bytes(int64_t n, int32_t k)
{
    if (n < 0 || n >= ((int64_t)1 << 31) || k < 0 || k > KPX_ORIENT_MAX_K) return 0;
    Arena a(nullptr, 0);
    TangentScratch s;
    tangent_carve(a, n, tangent_row(n, k), &s);
    return a.off;
}

KPX_EXPORT int kpx_orient_normals_tangent(const float *pts, float *normals, int64_t n, int32_t k, uint8_t *flips, int32_t *tree, int64_t *h_stats, void *ws,
                                          size_t ws_bytes, void *stream)
{
    int rc = orient_size_check("kpx_orient_normals_tangent", n, k);
    if (rc) return rc;
    if (h_stats) memset(h_stats, 0, 8 * sizeof(int64_t));
    if (n == 0) return KPX_OK;
    KPX_REQUIRE(pts && normals && ws, "kpx_orient_normals_tangent: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int kk = (int)((int64_t)k < n ? k : n), row = tangent_row(n, k);
    Arena a(ws, ws_bytes);
    TangentScratch s;
    tangent_carve(a, n, row, &s);
    KPX_ARENA_CHECK(a);
    const unsigned nb = orient_blocks(n);
    int64_t rounds_e = 0, rounds_t = 0;
    if (n >= 2) {
        rc = emst_run(pts, n, row, s.e, st, &rounds_e);
        if (rc) return rc;
        KPX_HIP(hipMemcpyAsync(s.emst, s.e.f.edges, (size_t)(n - 1) * sizeof(unsigned long long), hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(forest_init_kernel, dim3(nb), dim3(kOrientThreads), 0, st, s.f, n, (int32_t *)nullptr, (int32_t *)nullptr);
        const unsigned mb = orient_blocks(n * kk + n - 1);
        int64_t taken = 0;
        while (taken < n - 1) {
            KPX_REQUIRE(rounds_t < kBoruvkaMaxRounds, "kpx_orient_normals_tangent: %lld of %lld edges after %d rounds", (long long)taken, (long long)(n - 1),
                        kBoruvkaMaxRounds);
            hipLaunchKernelGGL(tree_offer_kernel<false>, dim3(mb), dim3(kOrientThreads), 0, st, s.f, n, kk, row, (const int32_t *)s.e.rows_idx,
                               (const unsigned long long *)s.emst, (const float *)normals);
            hipLaunchKernelGGL(tree_offer_kernel<true>, dim3(mb), dim3(kOrientThreads), 0, st, s.f, n, kk, row, (const int32_t *)s.e.rows_idx,
                               (const unsigned long long *)s.emst, (const float *)normals);
            const int64_t before = taken;
            rc = forest_close_round<true>(s.f, n, normals, st, &taken);
            if (rc) return rc;
            ++rounds_t;
            KPX_REQUIRE(taken > before && taken <= n - 1, "kpx_orient_normals_tangent: a round took %lld edges", (long long)(taken - before));
        }
    } else {
        KPX_HIP(hipMemsetAsync(s.e.ctr, 0, kCtrWords * sizeof(unsigned long long), st));
        hipLaunchKernelGGL(forest_init_kernel, dim3(nb), dim3(kOrientThreads), 0, st, s.f, n, (int32_t *)nullptr, (int32_t *)nullptr);
    }
    hipLaunchKernelGGL(orient_root_kernel, dim3(nb), dim3(kOrientThreads), 0, st, pts, n, s.e.ctr);
    KPX_LAUNCH_CHECK();
    unsigned long long ctr[kCtrWords];
    KPX_HIP(hipMemcpyAsync(ctr, s.e.ctr, sizeof(ctr), hipMemcpyDeviceToHost, st));
    KPX_HIP(hipStreamSynchronize(st));
    if (ctr[kCtrZero] == 0) {
        hipLaunchKernelGGL(orient_root_flip_kernel, dim3(1), dim3(64), 0, st, s.f, (const float *)normals);
        hipLaunchKernelGGL(orient_apply_kernel, dim3(nb), dim3(kOrientThreads), 0, st, s.f, n, normals, (const uint8_t *)nullptr, flips);
    } else {
        std::vector<unsigned long long> t((size_t)(n - 1));
        std::vector<float> hn(3 * (size_t)n);
        std::vector<uint8_t> hf;
        KPX_HIP(hipMemcpyAsync(t.data(), s.f.edges, t.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        KPX_HIP(hipMemcpyAsync(hn.data(), normals, hn.size() * sizeof(float), hipMemcpyDeviceToHost, st));
        KPX_HIP(hipStreamSynchronize(st));
        walk_signs(t, hn, n, (int32_t)(0xFFFFFFFFu - (uint32_t)ctr[kCtrRoot]), hf);
        KPX_HIP(hipMemcpyAsync(s.host_flips, hf.data(), hf.size(), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(orient_apply_kernel, dim3(nb), dim3(kOrientThreads), 0, st, s.f, n, normals, (const uint8_t *)s.host_flips, flips);
        KPX_LAUNCH_CHECK();
        KPX_HIP(hipStreamSynchronize(st));                 // (hf leaves scope)
    }
    KPX_LAUNCH_CHECK();
    if (tree && n >= 2) {
        rc = pairs_out(s.e.sort, n - 1, tree, st);
        if (rc) return rc;
    }
    KPX_HIP(hipStreamSynchronize(st));
    if (h_stats) {
        h_stats[0] = rounds_e; h_stats[1] = (int64_t)ctr[kCtrBounded]; h_stats[2] = (int64_t)ctr[kCtrUnbounded];
        h_stats[3] = rounds_t; h_stats[4] = (int64_t)ctr[kCtrZero];
    }
    return KPX_OK;
}
