// kpx_mesh.hip -- operators on a triangle mesh (float32 vertices, int32 triangles): normals and surface area (arithmetic contract
// AC12) and the clean-up path of AC13: vertex adjacency, non-manifold edges, connected triangles,
// ordered removal, Laplacian / Taubin smoothing and uniform sampling ([O3D] geometry.TriangleMesh).
// The checks of AC15 reuse those pieces: vertex links as a union-find over the adjacency's entries, orientation as a
// union-find over the double cover of the triangles, the volume as the ordered chain with another term, the edge count.
//
// The shape shared by adjacency, edges and clusters: one 64-bit key per (vertex, vertex) pair of every triangle, one stable radix sort,
// then a pass over the sorted keys in which every entry looks only at its predecessor.  Every fp64 sum whose order the contract fixes
// is taken by one owner in that order (a thread over its CSR row, one block's chain over the triangles); the only atomics are the
// union-find's hooks and integer counts, whose results do not depend on the order in which they land.
#include "kpx_compact.h"
#include "kpx_sort.h"
#include "kpx_unionfind.h"

#include <math.h>

namespace kpx {
namespace {

// ---- normals and area of a triangle mesh -----------------------------------------------------------------------------------------
// AC12: n = (v1 - v0) x (v2 - v0) in fp64 from the float32 vertices, each component a b - c d.  A triangle with an index outside
// [0, nv) reads nothing and has n = 0 (callers reject such meshes first).
__device__ __forceinline__ void mesh_cross(const float *__restrict__ v, int64_t nv, const int32_t *__restrict__ tri, int64_t t, double n[3])
{
    const int32_t i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
    n[0] = n[1] = n[2] = 0.0;
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) return;
    double e1[3], e2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double o = (double)v[3 * (int64_t)i0 + k];
        e1[k] = (double)v[3 * (int64_t)i1 + k] - o;
        e2[k] = (double)v[3 * (int64_t)i2 + k] - o;
    }
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
}
__device__ __forceinline__ double mesh_norm(const double n[3]) { return sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]); }
// n / |n|, the zero vector -> (0, 0, 1) ([O3D] NormalizeNormals), rounded to float32 at the store
__device__ __forceinline__ void mesh_store_normal(const double n[3], bool normalized, float *__restrict__ out)
{
    if (!normalized) {
        out[0] = (float)n[0]; out[1] = (float)n[1]; out[2] = (float)n[2];
        return;
    }
    const double len = mesh_norm(n);
    if (len == 0.0) {
        out[0] = 0.0f; out[1] = 0.0f; out[2] = 1.0f;
        return;
    }
    out[0] = (float)(n[0] / len); out[1] = (float)(n[1] / len); out[2] = (float)(n[2] / len);
}

// n64 (fp64 [nt][3], may be null): the unnormalised normals the vertex sums read; pairs (may be null): the identity values of the
// 3 nt (vertex, triangle corner) pairs for the sort
__global__ __launch_bounds__(256) void mesh_triangle_normals_kernel(const float *__restrict__ v, int64_t nv, const int32_t *__restrict__ tri, int64_t nt,
                                                                    int normalized, float *__restrict__ out, double *__restrict__ n64, int32_t *__restrict__ pairs)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    double n[3];
    mesh_cross(v, nv, tri, t, n);
    if (out) mesh_store_normal(n, normalized != 0, out + 3 * t);
    if (n64) { n64[3 * t] = n[0]; n64[3 * t + 1] = n[1]; n64[3 * t + 2] = n[2]; }
    if (pairs) { pairs[3 * t] = (int32_t)(3 * t); pairs[3 * t + 1] = (int32_t)(3 * t + 1); pairs[3 * t + 2] = (int32_t)(3 * t + 2); }
}

// keys: the 3 nt vertex indices sorted (stable: equal vertices keep ascending pair = triangle order), vals: their pair numbers.
// One thread per vertex walks its segment in order: the sum from 0 in ascending triangle index, whatever the segment's length.
__global__ __launch_bounds__(256) void mesh_vertex_normals_kernel(const uint32_t *__restrict__ keys, const int32_t *__restrict__ vals, int64_t npairs,
                                                                  const double *__restrict__ n64, int64_t nv, int normalized, float *__restrict__ out)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    int64_t lo = 0, hi = npairs;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    double acc[3] = { 0.0, 0.0, 0.0 };
    for (int64_t j = lo; j < npairs && (int64_t)keys[j] == v; ++j) {
        const int64_t t = (int64_t)(vals[j] / 3);
        acc[0] = acc[0] + n64[3 * t];
        acc[1] = acc[1] + n64[3 * t + 1];
        acc[2] = acc[2] + n64[3 * t + 2];
    }
    mesh_store_normal(acc, normalized != 0, out + 3 * v);
}

// the sum over the triangles, ascending, of |n| / 2 in fp64.  The order is the contract, so the additions are one chain; everything
// else is kept off it: one block computes the terms of 1024 triangles at a time into LDS (the gathers of the next batch are in flight
// while the current one is summed), and its first wave adds the current batch in order.
constexpr int kAreaThreads = 1024;
__global__ __launch_bounds__(kAreaThreads) void mesh_area_kernel(const float *__restrict__ v, int64_t nv, const int32_t *__restrict__ tri, int64_t nt,
                                                                 double *__restrict__ out)
{
    __shared__ double sh[2][kAreaThreads];
    auto term = [&](int64_t t) {
        double half = 0.0;
        if (t < nt) {
            double n[3];
            mesh_cross(v, nv, tri, t, n);
            half = mesh_norm(n) * 0.5;
        }
        return half;
    };
    sh[0][threadIdx.x] = term(threadIdx.x);
    __syncthreads();
    double s = 0.0;
    int cur = 0;
    for (int64_t b = 0; b < nt; b += kAreaThreads, cur ^= 1) {
        const double next = term(b + kAreaThreads + threadIdx.x);
        if (threadIdx.x < 64) {
            const int cnt = nt - b < kAreaThreads ? (int)(nt - b) : kAreaThreads;
#pragma unroll 16
            for (int i = 0; i < cnt; ++i) s = s + sh[cur][i];
        }
        sh[cur ^ 1][threadIdx.x] = next;
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = s;
}

struct MeshNormalScratch {
    double *n64;
    DeviceSort<uint32_t> sort;          // (vertex, corner) pairs; keys_in: the caller's triangle array
};
void mesh_normals_carve(Arena &a, int64_t nt, MeshNormalScratch *s)
{
    const int64_t t = nt > 0 ? nt : 1;
    s->n64 = a.get<double>(3 * (size_t)t);
    SortOptions o;
    o.keys_in = false;
    dsort_carve(a, 3 * t, 32, o, &s->sort);
}

constexpr int64_t kMeshMax = 2147483647;        // int32 indices
constexpr int kMeshThreads = 256;

inline unsigned mesh_blocks(int64_t n) { return (unsigned)cdiv(n > 0 ? n : 1, kMeshThreads); }
// bits that hold every value in [0, n]
inline int bits_for(int64_t n)
{
    int b = 1;
    while (b < 32 && ((int64_t)1 << b) <= n) ++b;
    return b;
}

// the three corners of triangle t; false when one lies outside [0, nv): such a triangle makes no pair, no edge and no reference
__device__ __forceinline__ bool mesh_corners(const int32_t *__restrict__ tri, int64_t t, int64_t nv, int32_t c[3])
{
    c[0] = tri[3 * t]; c[1] = tri[3 * t + 1]; c[2] = tri[3 * t + 2];
    return c[0] >= 0 && c[1] >= 0 && c[2] >= 0 && c[0] < nv && c[1] < nv && c[2] < nv;
}

// ---- pair keys (AC13) -------------------------------------------------------------------------------------------------------------
// directed: the six ordered corner pairs of a triangle, key = v << 32 | u (adjacency); else its three undirected edges, key =
// min << 32 | max.  A triangle with a corner out of range gets the key nv << 32, above every real one.  vals: the key's number, for
// the caller that needs the triangle behind a sorted key (the clusters); null otherwise.  skip_repeated: a triangle with two equal
// indices gets that key too (AC15's orientation: it takes no part).
__global__ __launch_bounds__(kMeshThreads) void mesh_pair_keys_kernel(const int32_t *__restrict__ tri, int64_t nt, int64_t nv, int directed,
                                                                      uint64_t *__restrict__ keys, int32_t *__restrict__ vals, int32_t *__restrict__ parent,
                                                                      int skip_repeated)
{
    const int64_t t = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (t >= nt) return;
    int32_t c[3];
    bool ok = mesh_corners(tri, t, nv, c);
    if (skip_repeated && (c[0] == c[1] || c[1] == c[2] || c[0] == c[2])) ok = false;
    const uint64_t bad = (uint64_t)nv << 32;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint64_t a = (uint64_t)(uint32_t)c[k], b = (uint64_t)(uint32_t)c[(k + 1) % 3];
        if (directed) {
            const int64_t j = 6 * t + 2 * k;
            keys[j] = ok ? (a << 32 | b) : bad;
            keys[j + 1] = ok ? (b << 32 | a) : bad;
            if (vals) { vals[j] = (int32_t)j; vals[j + 1] = (int32_t)(j + 1); }
        } else {
            const int64_t j = 3 * t + k;
            keys[j] = ok ? (a < b ? (a << 32 | b) : (b << 32 | a)) : bad;
            if (vals) vals[j] = (int32_t)j;
        }
    }
    if (parent) parent[t] = (int32_t)t;
}

// the pairs of every triangle in ascending key order -> keys_out (and vals_out: each key's number, where the sort carries values);
// carved for (directed ? 6 : 3) * nt pairs
template <bool kVals>
int pair_sort(const int32_t *tri, int64_t nt, int64_t nv, bool directed, const DeviceSort<uint64_t, kVals> &s, int32_t *parent, hipStream_t st,
              bool skip_repeated = false)
{
    hipLaunchKernelGGL(mesh_pair_keys_kernel, dim3(mesh_blocks(nt)), dim3(kMeshThreads), 0, st, tri, nt, nv, directed ? 1 : 0, s.keys_in, s.vals_in, parent,
                       skip_repeated ? 1 : 0);
    KPX_LAUNCH_CHECK();
    return dsort_run(s, (directed ? 6 : 3) * nt, 32 + bits_for(nv), st);
}

// ---- adjacency: the distinct sorted pairs are the CSR rows ---------------------------------------------------------------------------
struct UniquePairPred {
    const uint64_t *k; uint64_t bad;
    __device__ bool operator()(int64_t i, int) const { const uint64_t x = k[i]; return x < bad && (i == 0 || k[i - 1] != x); }
};
struct NeighbourEmit {
    const uint64_t *k; int32_t *nb, *owner;
    __device__ void operator()(int64_t i, int, int32_t dst) const { nb[dst] = (int32_t)(uint32_t)k[i]; owner[dst] = (int32_t)(k[i] >> 32); }
};
// offsets[v] = the number of neighbour entries owned by vertices below v, v in [0, nv]
__global__ __launch_bounds__(kMeshThreads) void mesh_offsets_kernel(const int32_t *__restrict__ owner, const int32_t *__restrict__ d_count, int64_t nv,
                                                                    int32_t *__restrict__ offsets)
{
    const int64_t v = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (v > nv) return;
    int32_t lo = 0, hi = *d_count;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)owner[mid] < v) lo = mid + 1; else hi = mid;
    }
    offsets[v] = lo;
}

struct AdjacencyScratch {
    DeviceSort<uint64_t, false> p;
    int32_t *owner, *counts;
};
void adjacency_carve(Arena &a, int64_t nt, AdjacencyScratch *s)
{
    dsort_carve(a, 6 * nt, 64, SortOptions(), &s->p);
    s->owner = a.get<int32_t>((size_t)(nt > 0 ? 6 * nt : 1));
    s->counts = a.get<int32_t>((size_t)compact_ws_ints(6 * nt));
}

// the CSR of n_triangles > 0 triangles -> out_offsets [nv + 1], out_neighbours [6 nt], *d_count entries
int adjacency_run(const int32_t *triangles, int64_t n_vertices, int64_t n_triangles, const AdjacencyScratch &s, int32_t *out_offsets, int32_t *out_neighbours,
                  int32_t *d_count, hipStream_t st)
{
    int rc = pair_sort(triangles, n_triangles, n_vertices, true, s.p, nullptr, st);
    if (rc) return rc;
    const uint64_t bad = (uint64_t)n_vertices << 32;
    rc = compact(UniquePairPred{ s.p.keys_out, bad }, NeighbourEmit{ s.p.keys_out, out_neighbours, s.owner }, 6 * n_triangles, 1, s.counts, d_count, st);
    if (rc) return rc;
    hipLaunchKernelGGL(mesh_offsets_kernel, dim3(mesh_blocks(n_vertices + 1)), dim3(kMeshThreads), 0, st, (const int32_t *)s.owner, (const int32_t *)d_count,
                       n_vertices, out_offsets);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

// ---- edges --------------------------------------------------------------------------------------------------------------------------
// the first entry of a run of equal keys speaks for the edge: the run is longer than 2 (allow_boundary) or not exactly 2 long
struct EdgeRunPred {
    const uint64_t *k; int64_t n; uint64_t bad; int allow_boundary;
    __device__ bool operator()(int64_t i, int) const
    {
        const uint64_t x = k[i];
        if (x >= bad || (i > 0 && k[i - 1] == x)) return false;
        int len = 1;
        while (len < 3 && i + len < n && k[i + len] == x) ++len;
        return allow_boundary ? len > 2 : len != 2;
    }
};
struct EdgeEmit {
    const uint64_t *k; int32_t *out;
    __device__ void operator()(int64_t i, int, int32_t dst) const { out[2 * (int64_t)dst] = (int32_t)(k[i] >> 32); out[2 * (int64_t)dst + 1] = (int32_t)(uint32_t)k[i]; }
};
struct EdgeScratch {
    DeviceSort<uint64_t, false> p;
    int32_t *counts;
};
void edge_carve(Arena &a, int64_t nt, EdgeScratch *s)
{
    dsort_carve(a, 3 * nt, 64, SortOptions(), &s->p);
    s->counts = a.get<int32_t>((size_t)compact_ws_ints(3 * nt));
}

// ---- connected triangles --------------------------------------------------------------------------------------------------------------
// every sorted edge entry is united with its predecessor of equal key: a run of any length becomes one set
__global__ __launch_bounds__(kMeshThreads) void mesh_union_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ vals, int64_t n, uint64_t bad,
                                                                  int32_t *parent, int32_t *__restrict__ err)
{
    const int64_t i = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x + 1;
    if (i >= n) return;
    const uint64_t x = keys[i];
    if (x >= bad || keys[i - 1] != x) return;
    const int32_t ta = vals[i] / 3, tb = vals[i - 1] / 3;
    if (ta == tb) return;
    int32_t ra = ta;
    if (!uf_unite(parent, ra, tb)) atomicExch(err, 1);
}
// parent[t] = root (a concurrent reader sees the old parent or the root: both lead to the root)
__global__ __launch_bounds__(kMeshThreads) void mesh_compress_kernel(int64_t nt, int32_t *parent)
{
    const int64_t t = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (t >= nt) return;
    int32_t r = parent[t];
    while (parent[r] != r) r = parent[r];
    parent[t] = r;
}
struct TriRootPred {
    const int32_t *parent;
    __device__ bool operator()(int64_t i, int) const { return parent[i] == (int32_t)i; }
};
struct TriRankEmit {
    int32_t *rank;
    __device__ void operator()(int64_t i, int, int32_t dst) const { rank[i] = dst; }
};
// cluster id = rank of the root; the counts are integer atomics, one per distinct cluster of a wave (one cluster often holds nearly
// every triangle: an atomic per triangle queues 329 k of them on one address; no order in an integer sum); the (cluster, triangle)
// pairs for the area pass's stable sort; a hook that gave up turns the count into KPX_ERR_RANGE
__global__ __launch_bounds__(kMeshThreads) void mesh_label_kernel(int64_t nt, const int32_t *__restrict__ parent, const int32_t *__restrict__ rank,
                                                                  int32_t *__restrict__ cluster, int32_t *__restrict__ n_tri, uint32_t *__restrict__ ckeys,
                                                                  int32_t *__restrict__ cvals, const int32_t *__restrict__ err, int32_t *__restrict__ d_count)
{
    const int64_t t = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (t == 0 && *err) *d_count = KPX_ERR_RANGE;
    bool todo = t < nt;
    const int32_t c = todo ? rank[parent[t]] : -1;
    if (todo) {
        cluster[t] = c;
        ckeys[t] = (uint32_t)c;
        cvals[t] = (int32_t)t;
    }
    for (;;) {
        const unsigned long long waiting = __ballot(todo);
        if (!waiting) break;
        const int leader = __builtin_ctzll(waiting);
        const int32_t c0 = __shfl(c, leader, 64);
        const unsigned long long same = __ballot(todo && c == c0);
        if (lane_id() == leader) atomicAdd(n_tri + c0, __builtin_popcountll(same));
        if (c == c0) todo = false;
    }
}

// ---- ordered fp64 chains over the triangles' areas ------------------------------------------------------------------------------------
// Item i is triangle order[i] (order null: i); its term is |n| / 2.  The sums are ONE chain in ascending i.  One block: the first lane
// of its first wave only adds -- 16 terms at a time from LDS into registers, 16 dependent additions, 16 partial sums back over the
// terms -- while the other 15 waves gather the terms of the next batch (dependent loads: order, indices, vertices) and store the
// partial sums of the batch before: nothing but the additions and their LDS traffic lies between two additions.  Items past the end
// have the term 0: s + 0.0 = s (s is never -0.0), so the last batch needs no tail.
//   SEG = false: out[i] = the sum of the terms 0 .. i (the sampler's cumulative areas)
//   SEG = true:  seg[i] (ascending) is the item's segment; the accumulator restarts from 0 at each new segment and out[seg] = the sum
//                at the segment's last item (the clusters' areas)
//   TERM = kTermTriple: the term is AC15's v0 . (v1 x v2) instead (the volume); a sum of signed terms that starts from +0.0 is
//                never -0.0 either (x + -x rounds to +0.0)
enum { kTermArea, kTermTriple };
__device__ __forceinline__ double mesh_triple(const float *__restrict__ v, int64_t nv, const int32_t *__restrict__ tri, int64_t t)
{
    int32_t c[3];
    c[0] = tri[3 * t]; c[1] = tri[3 * t + 1]; c[2] = tri[3 * t + 2];
    if (c[0] < 0 || c[1] < 0 || c[2] < 0 || c[0] >= nv || c[1] >= nv || c[2] >= nv) return 0.0;
    double a[3], b[3], d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[k] = (double)v[3 * (int64_t)c[0] + k];
        b[k] = (double)v[3 * (int64_t)c[1] + k];
        d[k] = (double)v[3 * (int64_t)c[2] + k];
    }
    const double cx = b[1] * d[2] - b[2] * d[1], cy = b[2] * d[0] - b[0] * d[2], cz = b[0] * d[1] - b[1] * d[0];
    return (a[0] * cx + a[1] * cy) + a[2] * cz;
}
constexpr int kChainGroup = 16;
constexpr int kChainWorkers = kAreaThreads - 64;
constexpr int kChainBatch = 2 * kChainWorkers;
static_assert(kChainBatch % kChainGroup == 0, "the adder takes whole groups");
template <bool SEG, int TERM = kTermArea>
__global__ __launch_bounds__(kAreaThreads) void mesh_chain_kernel(const float *__restrict__ v, int64_t nv, const int32_t *__restrict__ tri, int64_t nt,
                                                                  const int32_t *__restrict__ order, const uint32_t *__restrict__ seg, double *__restrict__ out)
{
    __shared__ double sh[2][kChainBatch];
    __shared__ uint8_t first[SEG ? 2 : 1][SEG ? kChainBatch : 1];            // 1: the item opens a segment
    const int w = (int)threadIdx.x - 64;                                     // worker number; negative: the adder's wave
    auto term = [&](int64_t i) {
        double half = 0.0;
        if (i < nt) {
            const int64_t t = order ? (int64_t)order[i] : i;
            if (t >= 0 && t < nt) {
                if (TERM == kTermTriple) {
                    half = mesh_triple(v, nv, tri, t);
                } else {
                    double n[3];
                    mesh_cross(v, nv, tri, t, n);
                    half = mesh_norm(n) * 0.5;
                }
            }
        }
        return half;
    };
    // workers: the terms of the batch at `base` into buffer p
    auto fill = [&](int64_t base, int p) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int j = w + k * kChainWorkers;
            const int64_t i = base + j;
            sh[p][j] = term(i);
            if (SEG) first[p][j] = (i > 0 && i < nt && seg[i] != seg[i - 1]) ? 1 : 0;
        }
    };
    // workers: the partial sums of the batch at `base`, left in buffer p by the adder, to where they were asked for
    auto flush = [&](int64_t base, int p) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int j = w + k * kChainWorkers;
            const int64_t i = base + j;
            if (i >= nt) continue;
            if (!SEG) out[i] = sh[p][j];
            else if (i == nt - 1 || seg[i + 1] != seg[i]) out[seg[i]] = sh[p][j];
        }
    };
    if (w >= 0) fill(0, 0);
    __syncthreads();
    double s = 0.0;
    int cur = 0;
    for (int64_t b = 0; b < nt; b += kChainBatch, cur ^= 1) {
        if (threadIdx.x == 0) {                                              // the chain: about 10 ns per addition on MI355X, 20 ns with the restarts
            for (int i = 0; i < kChainBatch; i += kChainGroup) {
                double a[kChainGroup];
                uint8_t f[kChainGroup];
#pragma unroll
                for (int k = 0; k < kChainGroup; ++k) {
                    a[k] = sh[cur][i + k];
                    f[k] = SEG ? first[cur][i + k] : 0;
                }
#pragma unroll
                for (int k = 0; k < kChainGroup; ++k) {
                    if (SEG) s = f[k] ? 0.0 : s;
                    s = s + a[k];
                    a[k] = s;
                }
#pragma unroll
                for (int k = 0; k < kChainGroup; ++k) sh[cur][i + k] = a[k];
            }
        } else if (w >= 0) {
            if (b > 0) flush(b - kChainBatch, cur ^ 1);
            fill(b + kChainBatch, cur ^ 1);
        }
        __syncthreads();
    }
    if (w >= 0 && nt > 0) flush(((nt - 1) / kChainBatch) * kChainBatch, cur ^ 1);
}

struct ClusterScratch {
    DeviceSort<uint64_t> p;          // the edges, each with its number
    int32_t *parent, *rank, *err, *counts;
    DeviceSort<uint32_t> c;          // (cluster, triangle) pairs
};
void cluster_carve(Arena &a, int64_t nt, ClusterScratch *s)
{
    const size_t t = (size_t)(nt > 0 ? nt : 1);
    dsort_carve(a, 3 * nt, 64, SortOptions(), &s->p);
    s->parent = a.get<int32_t>(t);
    s->rank = a.get<int32_t>(t);
    s->err = a.get<int32_t>(1);
    s->counts = a.get<int32_t>((size_t)compact_ws_ints(nt));
    dsort_carve(a, nt, 32, SortOptions(), &s->c);
}

// ---- removal: ordered compactions of the rows ---------------------------------------------------------------------------------------
// kind 0: out[v] = 1 for every vertex some triangle names; 1: out[t] = triangle t has two equal indices; 2: out[idx[j]] = 1 for the
// indices inside [0, n_out).  Kinds 0 and 2 write into a cleared array (the same byte from every writer).
__global__ __launch_bounds__(kMeshThreads) void mesh_flags_kernel(int kind, const int32_t *__restrict__ tri, int64_t nv, int64_t nt,
                                                                  const int64_t *__restrict__ idx, int64_t n_idx, uint8_t *__restrict__ out, int64_t n_out)
{
    const int64_t i = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (kind == 2) {
        if (i >= n_idx) return;
        const int64_t j = idx[i];
        if (j >= 0 && j < n_out) out[j] = 1;
        return;
    }
    if (i >= nt) return;
    int32_t c[3];
    const bool ok = mesh_corners(tri, i, nv, c);
    if (kind == 1) {
        if (i < n_out) out[i] = (c[0] == c[1] || c[1] == c[2] || c[0] == c[2]) ? 1 : 0;
    } else if (ok && nv <= n_out) {
        out[c[0]] = 1; out[c[1]] = 1; out[c[2]] = 1;
    }
}

__device__ __forceinline__ void copy_row3(const float *__restrict__ src, float *__restrict__ dst, int64_t i, int64_t d)
{
    dst[3 * d] = src[3 * i]; dst[3 * d + 1] = src[3 * i + 1]; dst[3 * d + 2] = src[3 * i + 2];
}
struct FlagPred {
    const uint8_t *f; int invert;
    __device__ bool operator()(int64_t i, int) const { return (f[i] != 0) != (invert != 0); }
};
struct TriangleRowEmit {
    const int32_t *tri; const float *tnrm; int32_t *otri; float *otnrm;
    __device__ void operator()(int64_t i, int, int32_t dst) const
    {
        const int64_t d = dst;
        otri[3 * d] = tri[3 * i]; otri[3 * d + 1] = tri[3 * i + 1]; otri[3 * d + 2] = tri[3 * i + 2];
        if (otnrm) copy_row3(tnrm, otnrm, i, d);
    }
};
struct VertexRowEmit {
    const float *vert, *col, *nrm; float *overt, *ocol, *onrm; int32_t *newidx;
    __device__ void operator()(int64_t i, int, int32_t dst) const
    {
        copy_row3(vert, overt, i, dst);
        if (ocol) copy_row3(col, ocol, i, dst);
        if (onrm) copy_row3(nrm, onrm, i, dst);
        newidx[i] = dst;
    }
};
// a triangle stays when its three corners do (a corner out of range counts as removed)
struct KeptCornersPred {
    const int32_t *tri; int64_t nv; FlagPred keep;
    __device__ bool operator()(int64_t t, int) const
    {
        int32_t c[3];
        return mesh_corners(tri, t, nv, c) && keep(c[0], 0) && keep(c[1], 0) && keep(c[2], 0);
    }
};
struct RenumberedRowEmit {
    const int32_t *tri, *newidx; const float *tnrm; int32_t *otri; float *otnrm;
    __device__ void operator()(int64_t i, int, int32_t dst) const
    {
        const int64_t d = dst;
        otri[3 * d] = newidx[tri[3 * i]]; otri[3 * d + 1] = newidx[tri[3 * i + 1]]; otri[3 * d + 2] = newidx[tri[3 * i + 2]];
        if (otnrm) copy_row3(tnrm, otnrm, i, d);
    }
};
struct SelectScratch {
    int32_t *newidx, *counts_v, *counts_t;
};
void select_carve(Arena &a, int64_t nv, int64_t nt, SelectScratch *s)
{
    s->newidx = a.get<int32_t>((size_t)(nv > 0 ? nv : 1));
    s->counts_v = a.get<int32_t>((size_t)compact_ws_ints(nv));
    s->counts_t = a.get<int32_t>((size_t)compact_ws_ints(nt));
}

// ---- smoothing (AC13) -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMeshThreads) void mesh_widen_kernel(const float *__restrict__ in, int64_t n, double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (i < n) out[i] = (double)in[i];
}
__global__ __launch_bounds__(kMeshThreads) void mesh_narrow_kernel(const double *__restrict__ in, int64_t n, float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (i < n) out[i] = (float)in[i];
}
constexpr int kSmoothArrays = 3;            // vertices, normals, colours
struct SmoothArrays {
    const double *in[kSmoothArrays];
    double *out[kSmoothArrays];
    int count;
};
// One step, one thread per vertex over its CSR row in ascending neighbour order.  laplacian = 0: y' = (y + sum y_u) / (1 + |N|).
// Else w_u = 1 / (|x_v - x_u| + 1e-12) from xw, the vertices at the start of the step, whatever array is filtered:
// y' = y + lambda (sum w_u y_u / sum w_u - y); an empty row keeps y.
__global__ __launch_bounds__(kMeshThreads) void mesh_smooth_kernel(const int32_t *__restrict__ offsets, const int32_t *__restrict__ nb, int64_t nv, int64_t n_nb,
                                                                   const double *__restrict__ xw, SmoothArrays A, int laplacian, double lambda)
{
    const int64_t v = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (v >= nv) return;
    int64_t lo = offsets[v], hi = offsets[v + 1];
    if (lo < 0 || hi > n_nb || hi < lo) lo = hi = 0;
    double W = 0.0, s[kSmoothArrays][3] = {};
    double xv[3] = { 0.0, 0.0, 0.0 };
    if (laplacian) { xv[0] = xw[3 * v]; xv[1] = xw[3 * v + 1]; xv[2] = xw[3 * v + 2]; }
    int64_t deg = 0;
    for (int64_t j = lo; j < hi; ++j) {
        const int64_t u = nb[j];
        if (u < 0 || u >= nv) continue;
        ++deg;
        double w = 1.0;
        if (laplacian) {
            const double d0 = xv[0] - xw[3 * u], d1 = xv[1] - xw[3 * u + 1], d2 = xv[2] - xw[3 * u + 2];
            const double dist = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
            w = 1.0 / (dist + 1e-12);
            W = W + w;
        }
#pragma unroll
        for (int a = 0; a < kSmoothArrays; ++a) {
            if (a >= A.count) break;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double y = A.in[a][3 * u + k];
                s[a][k] = s[a][k] + (laplacian ? w * y : y);
            }
        }
    }
#pragma unroll
    for (int a = 0; a < kSmoothArrays; ++a) {
        if (a >= A.count) break;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double y = A.in[a][3 * v + k];
            double r;
            if (!laplacian) r = (y + s[a][k]) / (double)(1 + deg);
            else r = deg == 0 ? y : y + lambda * (s[a][k] / W - y);
            A.out[a][3 * v + k] = r;
        }
    }
}

// ---- uniform sampling (AC13) ------------------------------------------------------------------------------------------------------------
// upto[t] = llround(prefix[t] / total * N), the last one N: the points [upto[t - 1], upto[t]) fall into triangle t
__global__ __launch_bounds__(kMeshThreads) void mesh_sample_split_kernel(const double *__restrict__ prefix, int64_t nt, int64_t n_points, int64_t *__restrict__ upto,
                                                                         double *__restrict__ d_total)
{
    const int64_t t = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (t >= nt) return;
    const double total = prefix[nt - 1];
    if (t == 0) *d_total = total;
    int64_t n = 0;
    if (total > 0.0) {
        const double cum = prefix[t] / total;
        n = (int64_t)llround(cum * (double)n_points);
    }
    upto[t] = t == nt - 1 ? n_points : n;
}
struct SampleArgs {
    const float *vert, *col, *vnrm, *tnrm;
    const int32_t *tri;
    float *opts, *ocol, *onrm;
    int64_t nv, nt, n_points;
    uint32_t seed_lo, seed_hi;
};
__device__ __forceinline__ double unit53(uint32_t lo, uint32_t hi) { return (double)((((uint64_t)hi << 32) | lo) >> 11) * 0x1p-53; }
__device__ __forceinline__ void sample_mix(const float *__restrict__ src, const int32_t c[3], double a, double b, double g, float *__restrict__ dst)
{
#pragma unroll
    for (int k = 0; k < 3; ++k)
        dst[k] = (float)((a * (double)src[3 * (int64_t)c[0] + k] + b * (double)src[3 * (int64_t)c[1] + k]) + g * (double)src[3 * (int64_t)c[2] + k]);
}
__global__ __launch_bounds__(kMeshThreads) void mesh_sample_kernel(const int64_t *__restrict__ upto, const double *__restrict__ d_total, SampleArgs S)
{
    const int64_t p = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (p >= S.n_points || !(*d_total > 0.0)) return;
    int64_t lo = 0, hi = S.nt;                  // t = #{upto <= p}
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (upto[mid] <= p) lo = mid + 1; else hi = mid;
    }
    const int64_t t = lo;
    int32_t c[3];
    if (t >= S.nt || !mesh_corners(S.tri, t, S.nv, c)) return;
    uint32_t o[4];
    philox4x32_10((uint32_t)p, (uint32_t)((uint64_t)p >> 32), 0x4D534D50u /* 'MSMP' */, 0u, S.seed_lo, S.seed_hi, o);
    const double r1 = unit53(o[0], o[1]), r2 = unit53(o[2], o[3]);
    const double q = sqrt(r1), a = 1.0 - q, b = q * (1.0 - r2), g = q * r2;
    sample_mix(S.vert, c, a, b, g, S.opts + 3 * p);
    if (S.ocol) sample_mix(S.col, c, a, b, g, S.ocol + 3 * p);
    if (S.onrm) {
        if (S.vnrm) sample_mix(S.vnrm, c, a, b, g, S.onrm + 3 * p);
        else copy_row3(S.tnrm, S.onrm, t, p);
    }
}
struct SampleScratch {
    double *prefix;
    int64_t *upto;
};
void sample_carve(Arena &a, int64_t nt, SampleScratch *s)
{
    const size_t t = (size_t)(nt > 0 ? nt : 1);
    s->prefix = a.get<double>(t);
    s->upto = a.get<int64_t>(t);
}

// ---- checks (AC15) ----------------------------------------------------------------------------------------------------------------------
// parent[i] = i, mark[i] = 0 (mark may be null)
__global__ __launch_bounds__(kMeshThreads) void mesh_iota_kernel(int64_t n, int32_t *__restrict__ parent, uint8_t *__restrict__ mark)
{
    const int64_t i = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (i >= n) return;
    parent[i] = (int32_t)i;
    if (mark) mark[i] = 0;
}
// where row v of the CSR names u, or -1
__device__ __forceinline__ int32_t link_entry(const int32_t *__restrict__ off, const int32_t *__restrict__ nb, int64_t n_nb, int32_t v, int32_t u)
{
    int64_t lo = off[v], hi = off[v + 1];
    if (lo < 0 || hi > n_nb || hi < lo) return -1;
    const int64_t end = hi;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (nb[mid] < u) lo = mid + 1; else hi = mid;
    }
    return lo < end && nb[lo] == u ? (int32_t)lo : -1;
}
// Vertex links on the CSR: the entries (v, u) are union-find nodes; a triangle in which v occurs once, beside u and w, marks (v, u)
// and (v, w) as link nodes and unites them.  Marks are the same byte from every writer; the hooks are order-free.
__global__ __launch_bounds__(kMeshThreads) void mesh_link_union_kernel(const int32_t *__restrict__ tri, int64_t nt, int64_t nv, const int32_t *__restrict__ off,
                                                                       const int32_t *__restrict__ nb, int64_t n_nb, int32_t *parent, uint8_t *__restrict__ mark,
                                                                       int32_t *__restrict__ err)
{
    const int64_t t = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (t >= nt) return;
    int32_t c[3];
    if (!mesh_corners(tri, t, nv, c)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int32_t v = c[k], u = c[(k + 1) % 3], w = c[(k + 2) % 3];
        if (v == u || v == w) continue;
        const int32_t eu = link_entry(off, nb, n_nb, v, u), ew = link_entry(off, nb, n_nb, v, w);
        if (eu < 0 || ew < 0) continue;                        // (cannot happen: the row was built from these very pairs)
        mark[eu] = 1;
        mark[ew] = 1;
        int32_t r = eu;
        if (eu != ew && !uf_unite(parent, r, ew)) atomicExch(err, 1);
    }
}
// flag[v] = 1 when the link nodes of row v (parent compressed) have more than one root
__global__ __launch_bounds__(kMeshThreads) void mesh_link_flag_kernel(int64_t nv, const int32_t *__restrict__ off, int64_t n_nb, const int32_t *__restrict__ parent,
                                                                      const uint8_t *__restrict__ mark, uint8_t *__restrict__ flag)
{
    const int64_t v = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (v >= nv) return;
    int64_t lo = off[v], hi = off[v + 1];
    if (lo < 0 || hi > n_nb || hi < lo) lo = hi = 0;
    int32_t first = -1;
    uint8_t split = 0;
    for (int64_t e = lo; e < hi; ++e) {
        if (!mark[e]) continue;
        const int32_t r = parent[e];
        if (first < 0) first = r;
        else if (r != first) split = 1;
    }
    flag[v] = split;
}
struct IndexEmit {
    int32_t *out;
    __device__ void operator()(int64_t i, int, int32_t dst) const { out[dst] = (int32_t)i; }
};
struct NoEmit {
    __device__ void operator()(int64_t, int, int32_t) const {}
};
// a hook that gave up turns the count into KPX_ERR_RANGE
__global__ void mesh_status_kernel(const int32_t *__restrict__ err, int32_t *__restrict__ d_count)
{
    if (*err) *d_count = KPX_ERR_RANGE;
}
struct LinkScratch {
    AdjacencyScratch adj;
    int32_t *off, *nb, *n_nb, *parent, *err, *counts;
    uint8_t *mark, *flag;
};
void link_carve(Arena &a, int64_t nv, int64_t nt, LinkScratch *s)
{
    const size_t e = (size_t)(nt > 0 ? 6 * nt : 1), v = (size_t)(nv > 0 ? nv : 1);
    adjacency_carve(a, nt, &s->adj);
    s->off = a.get<int32_t>(v + 1);
    s->nb = a.get<int32_t>(e);
    s->n_nb = a.get<int32_t>(1);
    s->parent = a.get<int32_t>(e);
    s->err = a.get<int32_t>(1);
    s->counts = a.get<int32_t>((size_t)compact_ws_ints(nv));
    s->mark = a.get<uint8_t>(e);
    s->flag = a.get<uint8_t>(v);
}

// Orientation on the double cover: node 2 t is triangle t as it is, 2 t + 1 flipped.  Consecutive entries of a run of equal edge keys
// are neighbours: they agree when they run the edge in opposite directions (the direction is read back from the triangle through the
// key's number 3 t + k).  A run of three or more cannot be satisfied by any assignment (of three directions two are equal, and every
// pair of the run must differ), so it is flagged outright and the remaining pairs of the run need no hook.
__global__ __launch_bounds__(kMeshThreads) void mesh_orient_union_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ vals, int64_t n, uint64_t bad,
                                                                         const int32_t *__restrict__ tri, int32_t *parent, int32_t *__restrict__ err,
                                                                         int32_t *__restrict__ one_sided)
{
    const int64_t i = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x + 1;
    if (i >= n) return;
    const uint64_t x = keys[i];
    if (x >= bad || keys[i - 1] != x) return;
    if (i >= 2 && keys[i - 2] == x) atomicExch(one_sided, 1);
    const int32_t ja = vals[i], jb = vals[i - 1];
    const int32_t ta = ja / 3, ka = ja % 3, tb = jb / 3, kb = jb % 3;
    const bool da = tri[3 * (int64_t)ta + ka] < tri[3 * (int64_t)ta + (ka + 1) % 3], db = tri[3 * (int64_t)tb + kb] < tri[3 * (int64_t)tb + (kb + 1) % 3];
    const int32_t a = 2 * ta, b = 2 * tb + (da == db ? 1 : 0);
    int32_t r = a;
    if (!uf_unite(parent, r, b)) atomicExch(err, 1);
    r = a ^ 1;
    if (!uf_unite(parent, r, b ^ 1)) atomicExch(err, 1);
}
__global__ __launch_bounds__(kMeshThreads) void mesh_orient_check_kernel(int64_t nt, const int32_t *__restrict__ parent, int32_t *__restrict__ one_sided)
{
    const int64_t t = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (t < nt && parent[2 * t] == parent[2 * t + 1]) atomicExch(one_sided, 1);
}
// A root is its set's smallest member, so the set of a component's smallest triangle t0 as it is has the root 2 t0 and the mirror
// set 2 t0 + 1: t is flipped exactly when the root of 2 t is odd.  Nothing is written to the mesh unless it is orientable.
__global__ __launch_bounds__(kMeshThreads) void mesh_orient_apply_kernel(int64_t nt, const int32_t *__restrict__ parent, const int32_t *__restrict__ one_sided,
                                                                         const int32_t *__restrict__ err, uint8_t *__restrict__ out_flip, int32_t *tri, float *tnrm,
                                                                         int32_t *__restrict__ d_orientable)
{
    const int64_t t = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    const bool ok = !*one_sided && !*err;
    if (t == 0) *d_orientable = *err ? KPX_ERR_RANGE : (ok ? 1 : 0);
    if (t >= nt) return;
    const bool flip = ok && (parent[2 * t] & 1);
    if (out_flip) out_flip[t] = flip ? 1 : 0;
    if (!flip) return;
    if (tri) {
        const int32_t c1 = tri[3 * t + 1], c2 = tri[3 * t + 2];
        tri[3 * t + 1] = c2;
        tri[3 * t + 2] = c1;
    }
    if (tnrm) { tnrm[3 * t] = -tnrm[3 * t]; tnrm[3 * t + 1] = -tnrm[3 * t + 1]; tnrm[3 * t + 2] = -tnrm[3 * t + 2]; }
}
struct OrientScratch {
    DeviceSort<uint64_t> p;
    int32_t *parent, *err, *one_sided;
};
void orient_carve(Arena &a, int64_t nt, OrientScratch *s)
{
    dsort_carve(a, 3 * nt, 64, SortOptions(), &s->p);
    s->parent = a.get<int32_t>((size_t)(nt > 0 ? 2 * nt : 1));
    s->err = a.get<int32_t>(1);
    s->one_sided = a.get<int32_t>(1);
}
// *out = |prefix[nt - 1]| / 6.0: one division, after the sum (AC15)
__global__ void mesh_volume_kernel(const double *__restrict__ prefix, int64_t nt, double *__restrict__ out)
{
    *out = nt > 0 ? fabs(prefix[nt - 1]) / 6.0 : 0.0;
}

inline bool mesh_counts_ok(int64_t nv, int64_t nt) { return nv >= 0 && nt >= 0 && nv <= kMeshMax && 6 * nt <= kMeshMax; }
#define KPX_MESH_COUNTS(who, nv, nt)                                                                                                       \
    do {                                                                                                                                   \
        KPX_REQUIRE((nv) >= 0 && (nt) >= 0, who ": negative count");                                                                       \
        if (!mesh_counts_ok(nv, nt))                                                                                                       \
            return fail(KPX_ERR_RANGE, who ": %lld vertices, %lld triangles: at most 2^31 - 1 vertices and 6 x triangles", (long long)(nv), \
                        (long long)(nt));                                                                                                  \
    } while (0)

}  // namespace
}  // namespace kpx

using namespace kpx;

KPX_EXPORT size_t kpx_mesh_normals_workspace_bytes(int64_t n_vertices, int64_t n_triangles)
{
    if (n_vertices < 0 || n_triangles < 0 || n_vertices > kMeshMax || 3 * n_triangles > kMeshMax) return 0;
    Arena a(nullptr, 0);
    MeshNormalScratch s;
    mesh_normals_carve(a, n_triangles, &s);
    return a.off;
}

KPX_EXPORT int kpx_mesh_normals(const float *vertices, int64_t n_vertices, const int32_t *triangles, int64_t n_triangles, int32_t normalized,
                                float *out_triangle_normals, float *out_vertex_normals, void *ws, size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(n_vertices >= 0 && n_triangles >= 0, "kpx_mesh_normals: negative count");
    if (n_vertices > kMeshMax || 3 * n_triangles > kMeshMax)
        return fail(KPX_ERR_RANGE, "kpx_mesh_normals: %lld vertices, %lld triangles: at most 2^31 - 1 vertices and triangle corners", (long long)n_vertices,
                    (long long)n_triangles);
    const bool want_v = out_vertex_normals && n_vertices > 0, want_t = out_triangle_normals && n_triangles > 0;
    if (!want_v && !want_t) return KPX_OK;
    KPX_REQUIRE((n_triangles == 0 || (vertices && triangles)) && (!want_v || ws), "kpx_mesh_normals: null pointer");
    hipStream_t st = (hipStream_t)stream;
    MeshNormalScratch s{};
    if (want_v) {
        Arena a(ws, ws_bytes);
        mesh_normals_carve(a, n_triangles, &s);
        KPX_ARENA_CHECK(a);
        s.sort.keys_in = reinterpret_cast<uint32_t *>(const_cast<int32_t *>(triangles));          // a sort only reads its inputs
    }
    const int64_t npairs = 3 * n_triangles;
    if (n_triangles > 0) {
        hipLaunchKernelGGL(mesh_triangle_normals_kernel, dim3((unsigned)cdiv(n_triangles, 256)), dim3(256), 0, st, vertices, n_vertices, triangles, n_triangles,
                           (int)normalized, want_t ? out_triangle_normals : (float *)nullptr, want_v ? s.n64 : (double *)nullptr,
                           want_v ? s.sort.vals_in : (int32_t *)nullptr);
        KPX_LAUNCH_CHECK();
    }
    if (!want_v) return KPX_OK;
    if (n_triangles > 0) {
        int bits = 1;
        while (bits < 32 && ((int64_t)1 << bits) < n_vertices) ++bits;
        const int rc = dsort_run(s.sort, npairs, bits, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(mesh_vertex_normals_kernel, dim3((unsigned)cdiv(n_vertices, 256)), dim3(256), 0, st, (const uint32_t *)s.sort.keys_out, (const int32_t *)s.sort.vals_out,
                       npairs, (const double *)s.n64, n_vertices, (int)normalized, out_vertex_normals);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT int kpx_mesh_surface_area(const float *vertices, int64_t n_vertices, const int32_t *triangles, int64_t n_triangles, double *d_area, void *stream)
{
    KPX_REQUIRE(n_vertices >= 0 && n_triangles >= 0, "kpx_mesh_surface_area: negative count");
    KPX_REQUIRE(d_area && (n_triangles == 0 || (vertices && triangles)), "kpx_mesh_surface_area: null pointer");
    hipLaunchKernelGGL(mesh_area_kernel, dim3(1), dim3(kAreaThreads), 0, (hipStream_t)stream, vertices, n_vertices, triangles, n_triangles, d_area);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT size_t kpx_mesh_adjacency_workspace_bytes(int64_t n_vertices, int64_t n_triangles)
{
    if (!mesh_counts_ok(n_vertices, n_triangles)) return 0;
    Arena a(nullptr, 0);
    AdjacencyScratch s;
    adjacency_carve(a, n_triangles, &s);
    return a.off;
}

KPX_EXPORT int kpx_mesh_adjacency(const int32_t *triangles, int64_t n_vertices, int64_t n_triangles, int32_t *out_offsets, int32_t *out_neighbours,
                                  int32_t *d_count, void *ws, size_t ws_bytes, void *stream)
{
    KPX_MESH_COUNTS("kpx_mesh_adjacency", n_vertices, n_triangles);
    KPX_REQUIRE(out_offsets && d_count && ws && (n_triangles == 0 || (triangles && out_neighbours)), "kpx_mesh_adjacency: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (n_triangles == 0) {
        KPX_HIP(hipMemsetAsync(out_offsets, 0, (size_t)(n_vertices + 1) * sizeof(int32_t), st));
        KPX_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), st));
        return KPX_OK;
    }
    Arena a(ws, ws_bytes);
    AdjacencyScratch s;
    adjacency_carve(a, n_triangles, &s);
    KPX_ARENA_CHECK(a);
    return adjacency_run(triangles, n_vertices, n_triangles, s, out_offsets, out_neighbours, d_count, st);
}

KPX_EXPORT size_t kpx_mesh_edges_workspace_bytes(int64_t n_vertices, int64_t n_triangles)
{
    if (!mesh_counts_ok(n_vertices, n_triangles)) return 0;
    Arena a(nullptr, 0);
    EdgeScratch s;
    edge_carve(a, n_triangles, &s);
    return a.off;
}

KPX_EXPORT int kpx_mesh_non_manifold_edges(const int32_t *triangles, int64_t n_vertices, int64_t n_triangles, int32_t allow_boundary_edges,
                                           int32_t *out_edges, int32_t *d_count, void *ws, size_t ws_bytes, void *stream)
{
    KPX_MESH_COUNTS("kpx_mesh_non_manifold_edges", n_vertices, n_triangles);
    KPX_REQUIRE(d_count && ws && (n_triangles == 0 || (triangles && out_edges)), "kpx_mesh_non_manifold_edges: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (n_triangles == 0) { KPX_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), st)); return KPX_OK; }
    Arena a(ws, ws_bytes);
    EdgeScratch s;
    edge_carve(a, n_triangles, &s);
    KPX_ARENA_CHECK(a);
    int rc = pair_sort(triangles, n_triangles, n_vertices, false, s.p, nullptr, st);
    if (rc) return rc;
    const int64_t n = 3 * n_triangles;
    return compact(EdgeRunPred{ s.p.keys_out, n, (uint64_t)n_vertices << 32, (int)allow_boundary_edges }, EdgeEmit{ s.p.keys_out, out_edges }, n, 1, s.counts,
                   d_count, st);
}

KPX_EXPORT size_t kpx_mesh_cluster_workspace_bytes(int64_t n_vertices, int64_t n_triangles)
{
    if (!mesh_counts_ok(n_vertices, n_triangles)) return 0;
    Arena a(nullptr, 0);
    ClusterScratch s;
    cluster_carve(a, n_triangles, &s);
    return a.off;
}

KPX_EXPORT int kpx_mesh_cluster_triangles(const float *vertices, int64_t n_vertices, const int32_t *triangles, int64_t n_triangles, int32_t *out_clusters,
                                          int32_t *out_n_triangles, double *out_area, int32_t *d_count, void *ws, size_t ws_bytes, void *stream)
{
    KPX_MESH_COUNTS("kpx_mesh_cluster_triangles", n_vertices, n_triangles);
    KPX_REQUIRE(d_count && ws, "kpx_mesh_cluster_triangles: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (n_triangles == 0) { KPX_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), st)); return KPX_OK; }
    KPX_REQUIRE(vertices && triangles && out_clusters && out_n_triangles && out_area, "kpx_mesh_cluster_triangles: null pointer");
    Arena a(ws, ws_bytes);
    ClusterScratch s;
    cluster_carve(a, n_triangles, &s);
    KPX_ARENA_CHECK(a);
    KPX_HIP(hipMemsetAsync(s.err, 0, sizeof(int32_t), st));
    KPX_HIP(hipMemsetAsync(out_n_triangles, 0, (size_t)n_triangles * sizeof(int32_t), st));
    int rc = pair_sort(triangles, n_triangles, n_vertices, false, s.p, s.parent, st);
    if (rc) return rc;
    const unsigned nb = mesh_blocks(n_triangles);
    hipLaunchKernelGGL(mesh_union_kernel, dim3(mesh_blocks(3 * n_triangles)), dim3(kMeshThreads), 0, st, (const uint64_t *)s.p.keys_out, (const int32_t *)s.p.vals_out,
                       3 * n_triangles, (uint64_t)n_vertices << 32, s.parent, s.err);
    hipLaunchKernelGGL(mesh_compress_kernel, dim3(nb), dim3(kMeshThreads), 0, st, n_triangles, s.parent);
    KPX_LAUNCH_CHECK();
    rc = compact(TriRootPred{ s.parent }, TriRankEmit{ s.rank }, n_triangles, 1, s.counts, d_count, st);
    if (rc) return rc;
    hipLaunchKernelGGL(mesh_label_kernel, dim3(nb), dim3(kMeshThreads), 0, st, n_triangles, (const int32_t *)s.parent, (const int32_t *)s.rank, out_clusters,
                       out_n_triangles, s.c.keys_in, s.c.vals_in, (const int32_t *)s.err, d_count);
    KPX_LAUNCH_CHECK();
    rc = dsort_run(s.c, n_triangles, bits_for(n_triangles), st);
    if (rc) return rc;
    hipLaunchKernelGGL(mesh_chain_kernel<true>, dim3(1), dim3(kAreaThreads), 0, st, vertices, n_vertices, triangles, n_triangles, (const int32_t *)s.c.vals_out,
                       (const uint32_t *)s.c.keys_out, out_area);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT int kpx_mesh_flags(int32_t kind, const int32_t *triangles, int64_t n_vertices, int64_t n_triangles, const int64_t *indices, int64_t n_indices,
                              uint8_t *out_flags, int64_t n_flags, void *stream)
{
    KPX_REQUIRE(kind >= KPX_MESH_FLAG_REFERENCED && kind <= KPX_MESH_FLAG_INDICES, "kpx_mesh_flags: unknown kind %d", (int)kind);
    KPX_REQUIRE(n_vertices >= 0 && n_triangles >= 0 && n_indices >= 0 && n_flags >= 0, "kpx_mesh_flags: negative count");
    const int64_t want = kind == KPX_MESH_FLAG_REFERENCED ? n_vertices : (kind == KPX_MESH_FLAG_DEGENERATE ? n_triangles : n_flags);
    KPX_REQUIRE(n_flags == want, "kpx_mesh_flags: %lld flags where the mesh needs %lld", (long long)n_flags, (long long)want);
    if (n_flags == 0) return KPX_OK;
    const int64_t items = kind == KPX_MESH_FLAG_INDICES ? n_indices : n_triangles;
    KPX_REQUIRE(out_flags && (items == 0 || (kind == KPX_MESH_FLAG_INDICES ? (const void *)indices : (const void *)triangles)), "kpx_mesh_flags: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (kind != KPX_MESH_FLAG_DEGENERATE) KPX_HIP(hipMemsetAsync(out_flags, 0, (size_t)n_flags, st));
    if (items == 0) return KPX_OK;
    hipLaunchKernelGGL(mesh_flags_kernel, dim3(mesh_blocks(items)), dim3(kMeshThreads), 0, st, (int)kind, triangles, n_vertices, n_triangles, indices, n_indices,
                       out_flags, n_flags);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT size_t kpx_mesh_select_workspace_bytes(int64_t n_vertices, int64_t n_triangles)
{
    if (!mesh_counts_ok(n_vertices, n_triangles)) return 0;
    Arena a(nullptr, 0);
    SelectScratch s;
    select_carve(a, n_vertices, n_triangles, &s);
    return a.off;
}

KPX_EXPORT int kpx_mesh_select_triangles(const int32_t *triangles, const float *triangle_normals, int64_t n_triangles, const uint8_t *flags, int32_t invert,
                                         int32_t *out_triangles, float *out_triangle_normals, int32_t *d_count, void *ws, size_t ws_bytes, void *stream)
{
    KPX_MESH_COUNTS("kpx_mesh_select_triangles", (int64_t)0, n_triangles);
    KPX_REQUIRE(d_count && ws, "kpx_mesh_select_triangles: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (n_triangles == 0) { KPX_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), st)); return KPX_OK; }
    KPX_REQUIRE(triangles && flags && out_triangles && (!out_triangle_normals || triangle_normals), "kpx_mesh_select_triangles: null pointer");
    Arena a(ws, ws_bytes);
    SelectScratch s;
    select_carve(a, 0, n_triangles, &s);
    KPX_ARENA_CHECK(a);
    return compact(FlagPred{ flags, (int)invert }, TriangleRowEmit{ triangles, triangle_normals, out_triangles, out_triangle_normals }, n_triangles, 1, s.counts_t,
                   d_count, st);
}

KPX_EXPORT int kpx_mesh_select_vertices(const float *vertices, const float *colors, const float *normals, int64_t n_vertices, const int32_t *triangles,
                                        const float *triangle_normals, int64_t n_triangles, const uint8_t *flags, int32_t invert, float *out_vertices,
                                        float *out_colors, float *out_normals, int32_t *out_triangles, float *out_triangle_normals, int32_t *d_counts, void *ws,
                                        size_t ws_bytes, void *stream)
{
    KPX_MESH_COUNTS("kpx_mesh_select_vertices", n_vertices, n_triangles);
    KPX_REQUIRE(d_counts && ws, "kpx_mesh_select_vertices: null pointer");
    hipStream_t st = (hipStream_t)stream;
    KPX_HIP(hipMemsetAsync(d_counts, 0, 2 * sizeof(int32_t), st));
    if (n_vertices == 0) return KPX_OK;
    KPX_REQUIRE(vertices && flags && out_vertices && (!out_colors || colors) && (!out_normals || normals), "kpx_mesh_select_vertices: null pointer");
    KPX_REQUIRE(n_triangles == 0 || (triangles && out_triangles && (!out_triangle_normals || triangle_normals)), "kpx_mesh_select_vertices: null pointer");
    Arena a(ws, ws_bytes);
    SelectScratch s;
    select_carve(a, n_vertices, n_triangles, &s);
    KPX_ARENA_CHECK(a);
    const FlagPred keep{ flags, (int)invert };
    int rc = compact(keep, VertexRowEmit{ vertices, colors, normals, out_vertices, out_colors, out_normals, s.newidx }, n_vertices, 1, s.counts_v, d_counts, st);
    if (rc || n_triangles == 0) return rc;
    return compact(KeptCornersPred{ triangles, n_vertices, keep }, RenumberedRowEmit{ triangles, s.newidx, triangle_normals, out_triangles, out_triangle_normals },
                   n_triangles, 1, s.counts_t, d_counts + 1, st);
}

// the widened arrays in two generations each, and the vertices a Laplacian step reads when they are not smoothed themselves
struct SmoothScratch { double *buf[kSmoothArrays][2], *fixed_x; };
static void smooth_carve(Arena &a, int64_t n_vertices, SmoothScratch *s)
{
    const size_t n3 = (size_t)(n_vertices > 0 ? 3 * n_vertices : 1);
    for (int k = 0; k < kSmoothArrays; ++k) { s->buf[k][0] = a.get<double>(n3); s->buf[k][1] = a.get<double>(n3); }
    s->fixed_x = a.get<double>(n3);
}
KPX_EXPORT size_t kpx_mesh_smooth_workspace_bytes(int64_t n_vertices)
{
    if (n_vertices < 0 || n_vertices > kMeshMax) return 0;
    Arena a(nullptr, 0);
    SmoothScratch s;
    smooth_carve(a, n_vertices, &s);
    return a.off;
}

KPX_EXPORT int kpx_mesh_smooth(const float *vertices, const float *normals, const float *colors, int64_t n_vertices, const int32_t *offsets,
                               const int32_t *neighbours, int64_t n_neighbours, int32_t method, int32_t iterations, double lambda_filter, double mu,
                               float *out_vertices, float *out_normals, float *out_colors, void *ws, size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(method >= KPX_MESH_SMOOTH_SIMPLE && method <= KPX_MESH_SMOOTH_TAUBIN, "kpx_mesh_smooth: unknown method %d", (int)method);
    KPX_REQUIRE(iterations >= 0, "filter_smooth: number_of_iterations must be non-negative");
    KPX_REQUIRE(n_vertices >= 0 && n_neighbours >= 0, "kpx_mesh_smooth: negative count");
    if (n_vertices > kMeshMax) return fail(KPX_ERR_RANGE, "kpx_mesh_smooth: %lld vertices: at most 2^31 - 1", (long long)n_vertices);
    if (n_vertices == 0 || (!out_vertices && !out_normals && !out_colors)) return KPX_OK;
    KPX_REQUIRE(vertices && offsets && ws && (n_neighbours == 0 || neighbours) && (!out_normals || normals) && (!out_colors || colors),
                "kpx_mesh_smooth: null pointer");
    hipStream_t st = (hipStream_t)stream;
    Arena a(ws, ws_bytes);
    const size_t n3 = (size_t)(3 * n_vertices);
    SmoothScratch sc;
    smooth_carve(a, n_vertices, &sc);
    KPX_ARENA_CHECK(a);
    const float *src[kSmoothArrays] = { vertices, normals, colors };
    float *dst[kSmoothArrays] = { out_vertices, out_normals, out_colors };
    const unsigned nb3 = mesh_blocks((int64_t)n3);
    int which[kSmoothArrays], count = 0;
    for (int k = 0; k < kSmoothArrays; ++k)
        if (dst[k]) {
            which[count++] = k;
            hipLaunchKernelGGL(mesh_widen_kernel, dim3(nb3), dim3(kMeshThreads), 0, st, src[k], (int64_t)n3, sc.buf[k][0]);
        }
    const int laplacian = method != KPX_MESH_SMOOTH_SIMPLE;
    if (laplacian && !out_vertices) hipLaunchKernelGGL(mesh_widen_kernel, dim3(nb3), dim3(kMeshThreads), 0, st, vertices, (int64_t)n3, sc.fixed_x);
    const int64_t steps = (int64_t)iterations * (method == KPX_MESH_SMOOTH_TAUBIN ? 2 : 1);
    int cur = 0;
    for (int64_t s = 0; s < steps; ++s, cur ^= 1) {
        SmoothArrays A{};
        A.count = count;
        for (int i = 0; i < count; ++i) { A.in[i] = sc.buf[which[i]][cur]; A.out[i] = sc.buf[which[i]][cur ^ 1]; }
        const double lam = method == KPX_MESH_SMOOTH_TAUBIN && (s & 1) ? mu : lambda_filter;
        hipLaunchKernelGGL(mesh_smooth_kernel, dim3(mesh_blocks(n_vertices)), dim3(kMeshThreads), 0, st, offsets, neighbours, n_vertices, n_neighbours,
                           (const double *)(out_vertices ? sc.buf[0][cur] : sc.fixed_x), A, laplacian, lam);
    }
    for (int i = 0; i < count; ++i)
        hipLaunchKernelGGL(mesh_narrow_kernel, dim3(nb3), dim3(kMeshThreads), 0, st, (const double *)sc.buf[which[i]][cur], (int64_t)n3, dst[which[i]]);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT size_t kpx_mesh_sample_workspace_bytes(int64_t n_triangles)
{
    if (n_triangles < 0 || n_triangles > kMeshMax) return 0;
    Arena a(nullptr, 0);
    SampleScratch s;
    sample_carve(a, n_triangles, &s);
    return a.off;
}

KPX_EXPORT int kpx_mesh_sample_points(const float *vertices, const float *colors, const float *vertex_normals, const float *triangle_normals,
                                      int64_t n_vertices, const int32_t *triangles, int64_t n_triangles, int64_t n_points, uint64_t seed, float *out_points,
                                      float *out_colors, float *out_normals, double *d_total, void *ws, size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(n_points > 0, "sample_points_uniformly: number_of_points must be positive");
    KPX_REQUIRE(n_triangles > 0 && n_vertices > 0, "sample_points_uniformly: the mesh has no triangles");
    if (n_vertices > kMeshMax || n_triangles > kMeshMax || n_points > kMeshMax)
        return fail(KPX_ERR_RANGE, "kpx_mesh_sample_points: at most 2^31 - 1 vertices, triangles and points");
    KPX_REQUIRE(vertices && triangles && out_points && d_total && ws, "kpx_mesh_sample_points: null pointer");
    KPX_REQUIRE((!out_colors || colors) && (!out_normals || vertex_normals || triangle_normals), "kpx_mesh_sample_points: an output without its input");
    hipStream_t st = (hipStream_t)stream;
    Arena a(ws, ws_bytes);
    SampleScratch s;
    sample_carve(a, n_triangles, &s);
    KPX_ARENA_CHECK(a);
    hipLaunchKernelGGL(mesh_chain_kernel<false>, dim3(1), dim3(kAreaThreads), 0, st, vertices, n_vertices, triangles, n_triangles, (const int32_t *)nullptr,
                       (const uint32_t *)nullptr, s.prefix);
    hipLaunchKernelGGL(mesh_sample_split_kernel, dim3(mesh_blocks(n_triangles)), dim3(kMeshThreads), 0, st, (const double *)s.prefix, n_triangles, n_points, s.upto,
                       d_total);
    SampleArgs S;
    S.vert = vertices; S.col = colors; S.vnrm = vertex_normals; S.tnrm = triangle_normals; S.tri = triangles;
    S.opts = out_points; S.ocol = out_colors; S.onrm = out_normals;
    S.nv = n_vertices; S.nt = n_triangles; S.n_points = n_points;
    S.seed_lo = (uint32_t)seed; S.seed_hi = (uint32_t)(seed >> 32);
    hipLaunchKernelGGL(mesh_sample_kernel, dim3(mesh_blocks(n_points)), dim3(kMeshThreads), 0, st, (const int64_t *)s.upto, (const double *)d_total, S);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT size_t kpx_mesh_links_workspace_bytes(int64_t n_vertices, int64_t n_triangles)
{
    if (!mesh_counts_ok(n_vertices, n_triangles)) return 0;
    Arena a(nullptr, 0);
    LinkScratch s;
    link_carve(a, n_vertices, n_triangles, &s);
    return a.off;
}

KPX_EXPORT int kpx_mesh_non_manifold_vertices(const int32_t *triangles, int64_t n_vertices, int64_t n_triangles, int32_t *out_vertices, int32_t *d_count, void *ws,
                                              size_t ws_bytes, void *stream)
{
    KPX_MESH_COUNTS("kpx_mesh_non_manifold_vertices", n_vertices, n_triangles);
    KPX_REQUIRE(d_count && ws, "kpx_mesh_non_manifold_vertices: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (n_triangles == 0 || n_vertices == 0) { KPX_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), st)); return KPX_OK; }
    KPX_REQUIRE(triangles && out_vertices, "kpx_mesh_non_manifold_vertices: null pointer");
    Arena a(ws, ws_bytes);
    LinkScratch s;
    link_carve(a, n_vertices, n_triangles, &s);
    KPX_ARENA_CHECK(a);
    const int64_t n_nb = 6 * n_triangles;
    KPX_HIP(hipMemsetAsync(s.err, 0, sizeof(int32_t), st));
    int rc = adjacency_run(triangles, n_vertices, n_triangles, s.adj, s.off, s.nb, s.n_nb, st);
    if (rc) return rc;
    hipLaunchKernelGGL(mesh_iota_kernel, dim3(mesh_blocks(n_nb)), dim3(kMeshThreads), 0, st, n_nb, s.parent, s.mark);
    hipLaunchKernelGGL(mesh_link_union_kernel, dim3(mesh_blocks(n_triangles)), dim3(kMeshThreads), 0, st, triangles, n_triangles, n_vertices, (const int32_t *)s.off,
                       (const int32_t *)s.nb, n_nb, s.parent, s.mark, s.err);
    hipLaunchKernelGGL(mesh_compress_kernel, dim3(mesh_blocks(n_nb)), dim3(kMeshThreads), 0, st, n_nb, s.parent);
    hipLaunchKernelGGL(mesh_link_flag_kernel, dim3(mesh_blocks(n_vertices)), dim3(kMeshThreads), 0, st, n_vertices, (const int32_t *)s.off, n_nb,
                       (const int32_t *)s.parent, (const uint8_t *)s.mark, s.flag);
    KPX_LAUNCH_CHECK();
    rc = compact(FlagPred{ s.flag, 0 }, IndexEmit{ out_vertices }, n_vertices, 1, s.counts, d_count, st);
    if (rc) return rc;
    hipLaunchKernelGGL(mesh_status_kernel, dim3(1), dim3(1), 0, st, (const int32_t *)s.err, d_count);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT size_t kpx_mesh_orientation_workspace_bytes(int64_t n_vertices, int64_t n_triangles)
{
    if (!mesh_counts_ok(n_vertices, n_triangles)) return 0;
    Arena a(nullptr, 0);
    OrientScratch s;
    orient_carve(a, n_triangles, &s);
    return a.off;
}

KPX_EXPORT int kpx_mesh_orientation(const int32_t *triangles, int64_t n_vertices, int64_t n_triangles, uint8_t *out_flip, int32_t *apply_triangles,
                                    float *apply_triangle_normals, int32_t *d_orientable, void *ws, size_t ws_bytes, void *stream)
{
    KPX_MESH_COUNTS("kpx_mesh_orientation", n_vertices, n_triangles);          // (6 T < 2^31: the 2 T nodes fit an int32 with room)
    KPX_REQUIRE(d_orientable && ws, "kpx_mesh_orientation: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (n_triangles == 0) {
        const int32_t one = 1;
        KPX_HIP(hipMemcpyAsync(d_orientable, &one, sizeof(one), hipMemcpyHostToDevice, st));
        KPX_HIP(hipStreamSynchronize(st));
        return KPX_OK;
    }
    KPX_REQUIRE(triangles, "kpx_mesh_orientation: null pointer");
    Arena a(ws, ws_bytes);
    OrientScratch s;
    orient_carve(a, n_triangles, &s);
    KPX_ARENA_CHECK(a);
    KPX_HIP(hipMemsetAsync(s.err, 0, sizeof(int32_t), st));
    KPX_HIP(hipMemsetAsync(s.one_sided, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(mesh_iota_kernel, dim3(mesh_blocks(2 * n_triangles)), dim3(kMeshThreads), 0, st, 2 * n_triangles, s.parent, (uint8_t *)nullptr);
    const int rc = pair_sort(triangles, n_triangles, n_vertices, false, s.p, nullptr, st, true);
    if (rc) return rc;
    const unsigned nb = mesh_blocks(n_triangles);
    hipLaunchKernelGGL(mesh_orient_union_kernel, dim3(mesh_blocks(3 * n_triangles)), dim3(kMeshThreads), 0, st, (const uint64_t *)s.p.keys_out,
                       (const int32_t *)s.p.vals_out, 3 * n_triangles, (uint64_t)n_vertices << 32, triangles, s.parent, s.err, s.one_sided);
    hipLaunchKernelGGL(mesh_compress_kernel, dim3(mesh_blocks(2 * n_triangles)), dim3(kMeshThreads), 0, st, 2 * n_triangles, s.parent);
    hipLaunchKernelGGL(mesh_orient_check_kernel, dim3(nb), dim3(kMeshThreads), 0, st, n_triangles, (const int32_t *)s.parent, s.one_sided);
    hipLaunchKernelGGL(mesh_orient_apply_kernel, dim3(nb), dim3(kMeshThreads), 0, st, n_triangles, (const int32_t *)s.parent, (const int32_t *)s.one_sided,
                       (const int32_t *)s.err, out_flip, apply_triangles, apply_triangle_normals, d_orientable);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

static double *volume_carve(Arena &a, int64_t n_triangles) { return a.get<double>((size_t)(n_triangles > 0 ? n_triangles : 1)); }      // the chain's prefix sums
KPX_EXPORT size_t kpx_mesh_volume_workspace_bytes(int64_t n_triangles)
{
    if (n_triangles < 0 || n_triangles > kMeshMax) return 0;
    Arena a(nullptr, 0);
    volume_carve(a, n_triangles);
    return a.off;
}

KPX_EXPORT int kpx_mesh_volume(const float *vertices, int64_t n_vertices, const int32_t *triangles, int64_t n_triangles, double *d_volume, void *ws,
                               size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(n_vertices >= 0 && n_triangles >= 0, "kpx_mesh_volume: negative count");
    if (n_vertices > kMeshMax || n_triangles > kMeshMax) return fail(KPX_ERR_RANGE, "kpx_mesh_volume: at most 2^31 - 1 vertices and triangles");
    KPX_REQUIRE(d_volume && ws && (n_triangles == 0 || (vertices && triangles)), "kpx_mesh_volume: null pointer");
    hipStream_t st = (hipStream_t)stream;
    Arena a(ws, ws_bytes);
    double *prefix = volume_carve(a, n_triangles);
    KPX_ARENA_CHECK(a);
    if (n_triangles > 0)
        hipLaunchKernelGGL((mesh_chain_kernel<false, kTermTriple>), dim3(1), dim3(kAreaThreads), 0, st, vertices, n_vertices, triangles, n_triangles,
                           (const int32_t *)nullptr, (const uint32_t *)nullptr, prefix);
    hipLaunchKernelGGL(mesh_volume_kernel, dim3(1), dim3(1), 0, st, (const double *)prefix, n_triangles, d_volume);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT int kpx_mesh_edge_count(const int32_t *triangles, int64_t n_vertices, int64_t n_triangles, int32_t *d_count, void *ws, size_t ws_bytes, void *stream)
{
    KPX_MESH_COUNTS("kpx_mesh_edge_count", n_vertices, n_triangles);
    KPX_REQUIRE(d_count && ws && (n_triangles == 0 || triangles), "kpx_mesh_edge_count: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (n_triangles == 0) { KPX_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), st)); return KPX_OK; }
    Arena a(ws, ws_bytes);
    EdgeScratch s;
    edge_carve(a, n_triangles, &s);
    KPX_ARENA_CHECK(a);
    const int rc = pair_sort(triangles, n_triangles, n_vertices, false, s.p, nullptr, st);
    if (rc) return rc;
    return compact(UniquePairPred{ s.p.keys_out, (uint64_t)n_vertices << 32 }, NoEmit{}, 3 * n_triangles, 1, s.counts, d_count, st);
}
