// kpx_search.hip -- neighbour search between a cloud and arbitrary query points ([O3D] KDTreeFlann: SearchKNN, SearchRadius,
// SearchHybrid; PointCloud::ComputePointCloudDistance, ComputeNearestNeighborDistance).  DESIGN.md 5.8.
//   index  = the uniform grid of kpx_knn.hip (occupancy 8) copied into ONE caller-owned buffer: header, cell starts, cell-sorted
//            coordinates, original indices.  Nothing in it points back into the cloud it was built from.
//   knn / hybrid: one WAVE per query.  The wave streams the points of the cells that hold the ball of radius rho around the query
//            (a column of cells is one contiguous run of the sorted points) and keeps the candidates that are not beyond the k-th
//            best (d2, index) seen so far in an LDS buffer; a full buffer is sorted (bitonic network, one wave) and cut to k.  The
//            search ends when the k-th distance lies inside rho; otherwise rho becomes that distance and the ball is streamed again.
//   radius: count pass (grid_radius_scan, no cap), the library's own 64-bit scan, fill pass, then every segment sorted by
//            (d2, index): a wave per segment in LDS up to kSegLds entries, one block per longer segment in place in global memory.
// Squared distance (contract AC3): d2 = fma(dz,dz, fma(dy,dy, dx*dx)), d = q - p in fp64.  Rows ascend in (d2, index).
#include "kpx_compact.h"
#include "kpx_searchview.h"

namespace kpx {

// gp == NULL: the index of an empty cloud (one cell, no points)
__global__ __launch_bounds__(256) void search_pack_kernel(char *__restrict__ index, SearchLayout l, int64_t n, int32_t cell_cap,
                                                          const GridParams *__restrict__ gp, const uint32_t *__restrict__ cell_start,
                                                          const float *__restrict__ spts, const int32_t *__restrict__ sidx)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t0 == 0) {
        SearchHeader h;
        h.magic = kSearchMagic; h.n = n; h.bytes = l.bytes; h.cell_cap = cell_cap; h.pad = 0;
        if (gp) h.gp = *gp;
        else { h.gp.org[0] = h.gp.org[1] = h.gp.org[2] = 0.0; h.gp.h = 1.0; h.gp.dim[0] = h.gp.dim[1] = h.gp.dim[2] = 1; h.gp.ncell = 1; }
        *reinterpret_cast<SearchHeader *>(index) = h;
    }
    uint32_t *cs = reinterpret_cast<uint32_t *>(index + l.cell_start);
    float *op = reinterpret_cast<float *>(index + l.pts);
    int32_t *oi = reinterpret_cast<int32_t *>(index + l.idx);
    for (int64_t i = t0; i <= (int64_t)cell_cap; i += stride) cs[i] = gp ? cell_start[i] : 0u;
    for (int64_t i = t0; i < 3 * n; i += stride) op[i] = spts[i];
    for (int64_t i = t0; i < n; i += stride) oi[i] = sidx[i];
}

// ---- (d2 pattern, index) pairs in LDS, sorted ascending by one wave -------------------------------------------------------------------
// Bitonic network in its one-direction form (the first step of every merge mirrors the second half), so that an array of any
// length sorts like its padding to a power of two with +inf: a comparator whose upper end lies past the array never swaps.
__device__ __forceinline__ bool pair_after(unsigned long long ka, int32_t ia, unsigned long long kb, int32_t ib)
{
    return ka > kb || (ka == kb && ia > ib);
}
__device__ __forceinline__ void wave_sort_pairs(unsigned long long *__restrict__ key, int32_t *__restrict__ ix, int n)
{
    const int lane = threadIdx.x & 63;
    if (n < 2) return;
    int half = 1;
    while (half < n) half <<= 1;
    half >>= 1;                                                   // comparators per step of the padded array
    auto cmpswap = [&](int l, int r) {
        if (r >= n) return;
        const unsigned long long kl = key[l], kr = key[r];
        const int32_t il = ix[l], ir = ix[r];
        if (pair_after(kl, il, kr, ir)) { key[l] = kr; key[r] = kl; ix[l] = ir; ix[r] = il; }
    };
    wave_lds_fence();
    for (int size = 2; (size >> 1) < n; size <<= 1) {
        const int hs = size >> 1;
        for (int t = lane; t < half; t += 64) {
            const int l = (t / hs) * size + (t % hs);
            cmpswap(l, l ^ (size - 1));
        }
        wave_lds_fence();
        for (int j = hs >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < half; t += 64) {
                const int l = (t / j) * 2 * j + (t % j);
                cmpswap(l, l + j);
            }
            wave_lds_fence();
        }
    }
}

// ---- knn / hybrid -----------------------------------------------------------------------------------------------------------------------
constexpr int kSearchMaxK = 4096;
// candidate buffer of a wave: room for the k kept entries and at least one more round of 64 (twice k for small k: fewer sorts)
static inline int search_cap(int k)
{
    int cap = 2 * k < k + 1024 ? 2 * k : k + 1024;
    cap = (cap + 63) & ~63;
    return cap < 128 ? 128 : cap;
}

struct WaveTopK {
    unsigned long long *key;       // d2 bit patterns (d2 >= 0: they order like the values)
    int32_t *ix;                   // original indices
    int cap, k, cnt;
    unsigned long long td;         // candidates after (td, ti) cannot be among the k smallest
    int32_t ti;
    __device__ bool admits(unsigned long long kb, int32_t i) const { return kb < td || (kb == td && i <= ti); }
    __device__ void cut()          // sort, keep the k smallest, tighten the bound
    {
        wave_sort_pairs(key, ix, cnt);
        if (cnt >= k) { cnt = k; td = key[k - 1]; ti = ix[k - 1]; }
    }
};

// every point of the cell box [lo, hi] with d2 < r2max that the bound admits goes into the buffer
__device__ __forceinline__ void wave_stream_box(const SearchView &v, const double q[3], const int lo[3], const int hi[3], double r2max,
                                                uint32_t *__restrict__ run_s0, int32_t *__restrict__ run_off, WaveTopK &tk)
{
    const int lane = threadIdx.x & 63;
    const int ny = hi[1] - lo[1] + 1, ncols = (hi[0] - lo[0] + 1) * ny;
    for (int c0 = 0; c0 < ncols; c0 += 64) {
        const int nruns = ncols - c0 < 64 ? ncols - c0 : 64;
        uint32_t s0 = 0;
        int len = 0;
        if (lane < nruns) {
            const int x = lo[0] + (c0 + lane) / ny, y = lo[1] + (c0 + lane) % ny;
            const int64_t col = ((int64_t)x * v.g.dim[1] + y) * v.g.dim[2];
            s0 = v.cell_start[col + lo[2]];
            len = (int)(v.cell_start[col + hi[2] + 1] - s0);
        }
        const int incl = wave_incl_scan(len);
        const int mc = __shfl(incl, 63, 64);
        if (mc == 0) continue;
        wave_lds_fence();
        run_s0[lane] = s0;
        run_off[lane] = incl - len;
        wave_lds_fence();
        for (int t0 = 0; t0 < mc; t0 += 64) {
            const int t = t0 + lane;
            unsigned long long kb = 0ull;
            int32_t oi = 0;
            bool in = false;
            if (t < mc) {
                int a = 0, b = nruns - 1;                                      // last run with off <= t
                while (a < b) {
                    const int mid = (a + b + 1) >> 1;
                    if (run_off[mid] <= t) a = mid; else b = mid - 1;
                }
                const uint32_t sp = run_s0[a] + (uint32_t)(t - run_off[a]);
                const float *pp = v.spts + 3 * (int64_t)sp;
                const double dx = q[0] - (double)pp[0], dy = q[1] - (double)pp[1], dz = q[2] - (double)pp[2];
                const double d = fma(dz, dz, fma(dy, dy, dx * dx));
                oi = v.sidx[sp];
                kb = (unsigned long long)__double_as_longlong(d);
                in = d < r2max;
            }
            bool keep = in && tk.admits(kb, oi);
            unsigned long long km = __builtin_amdgcn_ballot_w64(keep);
            if (km == 0ull) continue;
            if (tk.cnt + __builtin_popcountll(km) > tk.cap) {                   // (cnt > cap - 64 >= k: the cut leaves k entries)
                tk.cut();
                keep = in && tk.admits(kb, oi);
                km = __builtin_amdgcn_ballot_w64(keep);
            }
            if (keep) {
                const int pos = tk.cnt + __builtin_popcountll(km & ((1ull << lane) - 1ull));
                tk.key[pos] = kb;
                tk.ix[pos] = oi;
            }
            tk.cnt += __builtin_popcountll(km);
        }
    }
    wave_lds_fence();
}

// radius <= 0: plain knn.  out rows: count entries ascending in (d2, index), then -1 / +inf.
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void search_knn_kernel(SearchView v, const float *__restrict__ queries, int64_t m, int k, int cap, double radius,
                                                                int32_t *__restrict__ out_idx, double *__restrict__ out_d2, int32_t *__restrict__ out_cnt)
{
    extern __shared__ __align__(16) unsigned long long search_lds[];
    __shared__ uint32_t run_s0[WAVES][64];
    __shared__ int32_t run_off[WAVES][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    WaveTopK tk;
    tk.key = search_lds + (size_t)wave * cap;
    tk.ix = reinterpret_cast<int32_t *>(search_lds + (size_t)WAVES * cap) + (size_t)wave * cap;
    tk.cap = cap;
    const int kk = (int64_t)k < v.n ? k : (int)v.n;                             // entries a row can hold
    tk.k = kk;
    const double r2max = radius > 0.0 ? radius * radius : INFINITY;
    for (int64_t qi = (int64_t)blockIdx.x * WAVES + wave; qi < m; qi += (int64_t)gridDim.x * WAVES) {
        const double q[3] = { (double)queries[3 * qi], (double)queries[3 * qi + 1], (double)queries[3 * qi + 2] };
        tk.cnt = 0; tk.td = ~0ull; tk.ti = INT_MAX;
        const bool finite = isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]);
        if (finite && kk > 0) {
            // first ball: reaches the grid (a query outside starts where its ball first touches the box) and, inside, a few cells
            double out2 = 0.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double below = v.g.org[a] - q[a], above = q[a] - (v.g.org[a] + (double)v.g.dim[a] * v.g.h);
                const double o = below > 0.0 ? below : (above > 0.0 ? above : 0.0);
                out2 = fma(o, o, out2);
            }
            double f0 = sqrt((double)kk / 16.0);
            f0 = f0 < 0.5 ? 0.5 : f0;
            double rho = sqrt(out2) * (1.0 + 1e-9) + f0 * v.g.h;
            bool whole = kk >= v.n;
            for (int round = 0;; ++round) {
                bool last = false;
                if (radius > 0.0 && rho >= radius) { rho = radius; last = true; }
                if (round >= 48) whole = true;                                  // safety net: the whole grid ends every search
                int lo[3], hi[3];
                bool all = true;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double e = rho * (1.0 + 1e-9) + 1e-12 * (fabs(q[a]) + fabs(v.g.org[a]) + v.g.h);     // grid_radius_scan's margin
                    lo[a] = whole ? 0 : cell_coord(q[a] - e, v.g.org[a], v.g.h, v.g.dim[a]);
                    hi[a] = whole ? v.g.dim[a] - 1 : cell_coord(q[a] + e, v.g.org[a], v.g.h, v.g.dim[a]);
                    all = all && lo[a] == 0 && hi[a] == v.g.dim[a] - 1;
                }
                whole = all;
                tk.cnt = 0;
                wave_stream_box(v, q, lo, hi, r2max, run_s0[wave], run_off[wave], tk);
                const bool done = whole || last;
                if (done || tk.cnt >= kk) tk.cut();
                if (done) break;
                if (tk.cnt == kk) {
                    const double top = __longlong_as_double((long long)tk.td);
                    if (top < rho * rho) break;                                  // everything nearer than rho has been seen
                    rho = sqrt(top) * (1.0 + 1e-12);
                } else {
                    double f = cbrt((double)(kk + 1) / (double)(tk.cnt > 0 ? tk.cnt : 1));
                    f = f < 1.5 ? 1.5 : (f > 4.0 ? 4.0 : f);
                    rho *= f;
                }
            }
        }
        wave_lds_fence();
        const int cnt = tk.cnt;
        for (int t = lane; t < k; t += 64) {
            out_idx[qi * k + t] = t < cnt ? tk.ix[t] : -1;
            out_d2[qi * k + t] = t < cnt ? __longlong_as_double((long long)tk.key[t]) : INFINITY;
        }
        if (lane == 0) out_cnt[qi] = cnt;
        wave_lds_fence();
    }
}

// ---- radius ------------------------------------------------------------------------------------------------------------------------------
constexpr int kSegLds = 1024;            // longest segment a wave sorts in LDS
constexpr int kSegWaves = 4;
constexpr int kSegLongBlocks = 64;

__global__ __launch_bounds__(256) void search_radius_count_kernel(SearchView v, const float *__restrict__ queries, int64_t m, double radius, double r2,
                                                                  int64_t *__restrict__ offsets)
{
    for (int64_t qi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; qi < m; qi += (int64_t)gridDim.x * blockDim.x) {
        const double q[3] = { (double)queries[3 * qi], (double)queries[3 * qi + 1], (double)queries[3 * qi + 2] };
        int64_t cnt = 0;
        if (v.n > 0 && isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]))
            grid_radius_scan(v.g, v.cell_start, v.spts, q, radius, r2, [&](uint32_t, double) { ++cnt; return false; });
        offsets[qi] = cnt;
    }
}
__global__ __launch_bounds__(256) void search_radius_fill_kernel(SearchView v, const float *__restrict__ queries, int64_t m, double radius, double r2,
                                                                 const int64_t *__restrict__ offsets, int64_t total, int32_t *__restrict__ out_idx,
                                                                 double *__restrict__ out_d2)
{
    for (int64_t qi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; qi < m; qi += (int64_t)gridDim.x * blockDim.x) {
        const double q[3] = { (double)queries[3 * qi], (double)queries[3 * qi + 1], (double)queries[3 * qi + 2] };
        int64_t pos = offsets[qi], end = offsets[qi + 1];
        end = end < total ? end : total;                                        // (offsets that do not belong to this call write nothing out of bounds)
        if (pos < 0 || pos >= end || v.n == 0 || !(isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]))) continue;
        grid_radius_scan(v.g, v.cell_start, v.spts, q, radius, r2, [&](uint32_t s, double d) {
            out_idx[pos] = v.sidx[s];
            out_d2[pos] = d;
            return ++pos >= end;
        });
    }
}
// a wave per segment; segments longer than kSegLds are listed for search_sort_long_kernel
__global__ __launch_bounds__(kSegWaves * 64) void search_sort_segments_kernel(const int64_t *__restrict__ offsets, int64_t m, int64_t total,
                                                                              int32_t *__restrict__ idx, double *__restrict__ d2,
                                                                              int32_t *__restrict__ long_list, int32_t *__restrict__ long_count)
{
    __shared__ unsigned long long key[kSegWaves][kSegLds];
    __shared__ int32_t ix[kSegWaves][kSegLds];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t qi = (int64_t)blockIdx.x * kSegWaves + wave; qi < m; qi += (int64_t)gridDim.x * kSegWaves) {
        const int64_t b = offsets[qi];
        int64_t e = offsets[qi + 1];
        e = e < total ? e : total;
        if (b < 0 || e - b < 2) continue;
        if (e - b > kSegLds) {
            if (lane == 0) long_list[atomicAdd(long_count, 1)] = (int32_t)qi;
            continue;
        }
        const int len = (int)(e - b);
        wave_lds_fence();
        for (int t = lane; t < len; t += 64) { key[wave][t] = (unsigned long long)__double_as_longlong(d2[b + t]); ix[wave][t] = idx[b + t]; }
        wave_sort_pairs(key[wave], ix[wave], len);
        for (int t = lane; t < len; t += 64) { d2[b + t] = __longlong_as_double((long long)key[wave][t]); idx[b + t] = ix[wave][t]; }
        wave_lds_fence();
    }
}
// the same network over a whole block, in place in global memory (the segment stays in L2)
__global__ __launch_bounds__(1024) void search_sort_long_kernel(const int64_t *__restrict__ offsets, int64_t total, int32_t *__restrict__ idx,
                                                                double *__restrict__ d2, const int32_t *__restrict__ long_list,
                                                                const int32_t *__restrict__ long_count)
{
    const int nlong = *long_count;
    for (int li = blockIdx.x; li < nlong; li += gridDim.x) {
        const int64_t qi = long_list[li];
        const int64_t b = offsets[qi];
        int64_t e = offsets[qi + 1];
        e = e < total ? e : total;
        const int64_t n = e - b;
        int64_t half = 1;
        while (half < n) half <<= 1;
        half >>= 1;
        double *kd = d2 + b;
        int32_t *ki = idx + b;
        auto cmpswap = [&](int64_t l, int64_t r) {
            if (r >= n) return;
            const double dl = kd[l], dr = kd[r];
            const int32_t il = ki[l], ir = ki[r];
            if (dl > dr || (dl == dr && il > ir)) { kd[l] = dr; kd[r] = dl; ki[l] = ir; ki[r] = il; }
        };
        for (int64_t size = 2; (size >> 1) < n; size <<= 1) {
            const int64_t hs = size >> 1;
            for (int64_t t = threadIdx.x; t < half; t += blockDim.x) {
                const int64_t l = (t / hs) * size + (t % hs);
                cmpswap(l, l ^ (size - 1));
            }
            __syncthreads();
            for (int64_t j = hs >> 1; j > 0; j >>= 1) {
                for (int64_t t = threadIdx.x; t < half; t += blockDim.x) {
                    const int64_t l = (t / j) * 2 * j + (t % j);
                    cmpswap(l, l + j);
                }
                __syncthreads();
            }
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
#define KPX_SEARCH_INDEX_ARGS(who)                                                                                                          \
    KPX_REQUIRE(index, who ": null index");                                                                                                 \
    KPX_REQUIRE(index_bytes >= search_layout(0).bytes, who ": index_bytes %zu is smaller than the %zu bytes of an index of 0 points",       \
                index_bytes, search_layout(0).bytes)

struct SearchScratch { int32_t *long_count, *long_list; };
static void search_carve(Arena &a, int64_t m, SearchScratch *s)
{
    s->long_count = a.get<int32_t>(64);
    s->long_list = a.get<int32_t>((size_t)(m > 0 ? m : 1));
}

}  // namespace kpx

using namespace kpx;

KPX_EXPORT size_t kpx_search_index_bytes(int64_t n) { return search_layout(n < 0 ? 0 : n).bytes; }

KPX_EXPORT size_t kpx_search_workspace_bytes(int64_t m, int32_t k)
{
    Arena a(nullptr, 0);
    if (k == 0) {                                   // the build of an index over m points
        Grid g;
        grid_build(nullptr, m, 8.0, a, &g, nullptr);
        return a.off;
    }
    SearchScratch s;
    search_carve(a, m, &s);
    return a.off;
}

KPX_EXPORT int kpx_search_index_build(const float *pts, int64_t n, void *index, size_t index_bytes, void *ws, size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "kpx_search_index_build: bad size");
    KPX_REQUIRE(index, "kpx_search_index_build: null index");
    const SearchLayout l = search_layout(n);
    KPX_REQUIRE(index_bytes >= l.bytes, "kpx_search_index_build: index_bytes %zu is smaller than the %zu bytes of an index of %lld points", index_bytes,
                l.bytes, (long long)n);
    hipStream_t st = (hipStream_t)stream;
    const int32_t cell_cap = search_cell_cap(n);
    if (n == 0) {
        hipLaunchKernelGGL(search_pack_kernel, dim3(64), dim3(256), 0, st, (char *)index, l, n, cell_cap, (const GridParams *)nullptr,
                           (const uint32_t *)nullptr, (const float *)nullptr, (const int32_t *)nullptr);
        KPX_LAUNCH_CHECK();
        return KPX_OK;
    }
    KPX_REQUIRE(pts && ws, "kpx_search_index_build: null pointer");
    Arena a(ws, ws_bytes);
    Grid g;
    const int rc = grid_build(pts, n, 8.0, a, &g, st);
    if (rc) return rc;
    const int nb = (int)(cdiv(3 * n, 256) > 4096 ? 4096 : cdiv(3 * n, 256));
    hipLaunchKernelGGL(search_pack_kernel, dim3(nb < 64 ? 64 : nb), dim3(256), 0, st, (char *)index, l, n, cell_cap, (const GridParams *)g.params,
                       (const uint32_t *)g.cell_start, (const float *)g.sorted_pts, (const int32_t *)g.sorted_idx);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT int kpx_search_knn(const void *index, size_t index_bytes, const float *queries, int64_t m, int32_t k, double radius, int32_t *idx,
                              double *d2, int32_t *count, void *ws, size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(k >= 1, "kpx_search_knn: k (max_nn) must be at least 1");
    KPX_REQUIRE(k <= kSearchMaxK, "kpx_search_knn: k (max_nn) > %d is not supported", kSearchMaxK);
    KPX_REQUIRE(!(radius != radius), "kpx_search_knn: radius is not a number");
    KPX_SEARCH_INDEX_ARGS("kpx_search_knn");
    KPX_REQUIRE(m >= 0 && m < ((int64_t)1 << 31), "kpx_search_knn: bad number of queries");
    if (m == 0) return KPX_OK;
    KPX_REQUIRE(queries && idx && d2 && count, "kpx_search_knn: null pointer");
    hipStream_t st = (hipStream_t)stream;
    SearchView v;
    const int rc = search_open(index, index_bytes, st, &v);
    if (rc) return rc;
    const int kk = (int64_t)k < v.n ? k : (int)(v.n > 0 ? v.n : 1);
    const int cap = search_cap(kk);
    const size_t per_wave = (size_t)cap * (sizeof(unsigned long long) + sizeof(int32_t));
    if (4 * per_wave <= 48 * 1024) {
        hipLaunchKernelGGL(search_knn_kernel<4>, dim3((unsigned)(cdiv(m, 4) > 65536 ? 65536 : cdiv(m, 4))), dim3(256), 4 * per_wave, st, v, queries, m, (int)k,
                           cap, radius, idx, d2, count);
    } else {                                        // up to 5120 entries, 60 KiB: one wave per block
        hipLaunchKernelGGL(search_knn_kernel<1>, dim3((unsigned)(m > 65536 ? 65536 : m)), dim3(64), per_wave, st, v, queries, m, (int)k, cap, radius, idx, d2,
                           count);
    }
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT int kpx_search_radius_count(const void *index, size_t index_bytes, const float *queries, int64_t m, double radius, int64_t *offsets, void *ws,
                                       size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(radius > 0.0, "kpx_search_radius_count: radius must be positive");
    KPX_SEARCH_INDEX_ARGS("kpx_search_radius_count");
    KPX_REQUIRE(m >= 0 && m < ((int64_t)1 << 31), "kpx_search_radius_count: bad number of queries");
    KPX_REQUIRE(offsets && (queries || m == 0), "kpx_search_radius_count: null pointer");
    hipStream_t st = (hipStream_t)stream;
    SearchView v;
    const int rc = search_open(index, index_bytes, st, &v);
    if (rc) return rc;
    if (m > 0)
        hipLaunchKernelGGL(search_radius_count_kernel, dim3((unsigned)(cdiv(m, 256) > 8192 ? 8192 : cdiv(m, 256))), dim3(256), 0, st, v, queries, m, radius,
                           radius * radius, offsets);
    scan_i64(offsets, m, st);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT int kpx_search_radius_fill(const void *index, size_t index_bytes, const float *queries, int64_t m, double radius, const int64_t *offsets,
                                      int64_t total, int32_t *idx, double *d2, void *ws, size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(radius > 0.0, "kpx_search_radius_fill: radius must be positive");
    KPX_SEARCH_INDEX_ARGS("kpx_search_radius_fill");
    KPX_REQUIRE(m >= 0 && m < ((int64_t)1 << 31) && total >= 0, "kpx_search_radius_fill: bad number of queries or entries");
    if (total > (int64_t)INT32_MAX) return fail(KPX_ERR_RANGE, "kpx_search_radius_fill: %lld entries, more than 2^31 - 1", (long long)total);
    if (m == 0 || total == 0) return KPX_OK;
    KPX_REQUIRE(queries && offsets && idx && d2 && ws, "kpx_search_radius_fill: null pointer");
    hipStream_t st = (hipStream_t)stream;
    SearchView v;
    const int rc = search_open(index, index_bytes, st, &v);
    if (rc) return rc;
    Arena a(ws, ws_bytes);
    SearchScratch s;
    search_carve(a, m, &s);
    KPX_ARENA_CHECK(a);
    KPX_HIP(hipMemsetAsync(s.long_count, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(search_radius_fill_kernel, dim3((unsigned)(cdiv(m, 256) > 8192 ? 8192 : cdiv(m, 256))), dim3(256), 0, st, v, queries, m, radius,
                       radius * radius, offsets, total, idx, d2);
    hipLaunchKernelGGL(search_sort_segments_kernel, dim3((unsigned)(cdiv(m, kSegWaves) > 16384 ? 16384 : cdiv(m, kSegWaves))), dim3(kSegWaves * 64), 0, st,
                       offsets, m, total, idx, d2, s.long_list, s.long_count);
    hipLaunchKernelGGL(search_sort_long_kernel, dim3(kSegLongBlocks), dim3(1024), 0, st, offsets, total, idx, d2, (const int32_t *)s.long_list,
                       (const int32_t *)s.long_count);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}
