// kpx_gridknn.h -- the exact grid neighbour search shared by kpx_knn.hip, kpx_fpfh.hip, kpx_cluster.hip and kpx_search.hip: the
// device primitives (heaps, ring walk, radius visitor, wave-per-query selection) and, at the end, the ONE wave-per-query kernel, the
// ONE thread-per-query heap kernel and the host cascade that SOR, normals / covariances and the neighbour lists run them through.
#pragma once
#include <initializer_list>

#include "kpx_internal.h"

namespace kpx {

__device__ __forceinline__ int cell_coord(double v, double org, double h, int dim)
{
    int c = (int)floor((v - org) / h);
    return c < 0 ? 0 : (c >= dim ? dim - 1 : c);
}

// ---- per-thread max-heaps in LDS ---------------------------------------------------------------------
// values only (SOR): slot e of this thread lives at h[e * stride]
struct HeapD {
    double *h; int stride, k, sz;
    static __device__ HeapD make(double *h, int32_t *, int stride, int k) { return HeapD{ h, stride, k, 0 }; }
    __device__ bool full() const { return sz == k; }
    __device__ double worst() const { return h[0]; }
    __device__ void push(double d, int)
    {
        if (sz < k) {
            int c = sz++;
            while (c > 0) {
                int p = (c - 1) >> 1;
                double hp = h[p * stride];
                if (hp < d) { h[c * stride] = hp; c = p; } else break;
            }
            h[c * stride] = d;
        } else if (d < h[0]) {
            int c = 0;
            for (;;) {
                int l = 2 * c + 1, r = l + 1;
                if (l >= k) break;
                double hl = h[l * stride];
                int b = l; double hb = hl;
                if (r < k) { double hr = h[r * stride]; if (hr > hl) { b = r; hb = hr; } }
                if (hb > d) { h[c * stride] = hb; c = b; } else break;
            }
            h[c * stride] = d;
        }
    }
};
// (d2, idx) pairs ordered lexicographically (normals: the neighbour identities matter)
struct HeapDI {
    double *h; int32_t *ix; int stride, k, sz;
    static __device__ HeapDI make(double *h, int32_t *ix, int stride, int k) { return HeapDI{ h, ix, stride, k, 0 }; }
    __device__ bool full() const { return sz == k; }
    __device__ double worst() const { return h[0]; }
    static __device__ bool less(double a, int32_t ai, double b, int32_t bi) { return a < b || (a == b && ai < bi); }
    __device__ void push(double d, int j)
    {
        if (sz < k) {
            int c = sz++;
            while (c > 0) {
                int p = (c - 1) >> 1;
                double hp = h[p * stride]; int32_t ip = ix[p * stride];
                if (less(hp, ip, d, j)) { h[c * stride] = hp; ix[c * stride] = ip; c = p; } else break;
            }
            h[c * stride] = d; ix[c * stride] = j;
        } else if (less(d, j, h[0], ix[0])) {
            int c = 0;
            for (;;) {
                int l = 2 * c + 1, r = l + 1;
                if (l >= k) break;
                int b = l; double hb = h[l * stride]; int32_t ib = ix[l * stride];
                if (r < k) { double hr = h[r * stride]; int32_t ir = ix[r * stride]; if (less(hb, ib, hr, ir)) { b = r; hb = hr; ib = ir; } }
                if (less(d, j, hb, ib)) { h[c * stride] = hb; ix[c * stride] = ib; c = b; } else break;
            }
            h[c * stride] = d; ix[c * stride] = j;
        }
    }
};

// Ring walk.  r2max < 0: plain kNN; otherwise only candidates with d2 < r2max ([O3D] SearchHybrid).
template <class Heap>
__device__ __forceinline__ void grid_knn_scan(const GridParams &g, const uint32_t *__restrict__ cell_start,
                                              const float *__restrict__ spts, const int32_t *__restrict__ sidx, double qx,
                                              double qy, double qz, double r2max, Heap &heap)
{
    const double q[3] = { qx, qy, qz };
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = cell_coord(q[a], g.org[a], g.h, g.dim[a]);
    int maxr = g.dim[0] > g.dim[1] ? g.dim[0] : g.dim[1];
    if (g.dim[2] > maxr) maxr = g.dim[2];
    double gate = heap.full() ? heap.worst() : INFINITY;     // register copy of the heap's worst value
    for (int r = 0; r <= maxr; ++r) {
        if (r > 0) {
            double dcov = INFINITY;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                double lo = g.org[a] + (double)(c[a] - (r - 1)) * g.h;
                double hi = g.org[a] + (double)(c[a] + r) * g.h;
                double dl = (c[a] - (r - 1) <= 0) ? INFINITY : q[a] - lo;
                double dh = (c[a] + r >= g.dim[a]) ? INFINITY : hi - q[a];
                dcov = fmin(dcov, fmin(dl, dh));
            }
            if (dcov == INFINITY) break;
            if (dcov < 0.0) dcov = 0.0;
            double cov2 = dcov * dcov * (1.0 - 1e-12);
            if (heap.full() && heap.worst() < cov2) break;
            if (r2max >= 0.0 && cov2 >= r2max) break;
        }
        const int x0 = c[0] - r, x1 = c[0] + r, y0 = c[1] - r, y1 = c[1] + r, z0 = c[2] - r, z1 = c[2] + r;
        const int xa = x0 < 0 ? 0 : x0, xb = x1 >= g.dim[0] ? g.dim[0] - 1 : x1;
        const int ya = y0 < 0 ? 0 : y0, yb = y1 >= g.dim[1] ? g.dim[1] - 1 : y1;
        const int za = z0 < 0 ? 0 : z0, zb = z1 >= g.dim[2] ? g.dim[2] - 1 : z1;
        for (int x = xa; x <= xb; ++x)
            for (int y = ya; y <= yb; ++y) {
                const bool shell_xy = (x == x0) | (x == x1) | (y == y0) | (y == y1);
                const int64_t col = ((int64_t)x * g.dim[1] + y) * g.dim[2];
                // cells of one (x,y) column are contiguous in the sorted order
                for (int part = 0; part < 2; ++part) {
                    int zs, ze;
                    if (shell_xy) { if (part) break; zs = za; ze = zb; }
                    else {
                        if (part == 0) { if (z0 < 0) continue; zs = ze = z0; }
                        else { if (z1 >= g.dim[2] || r == 0) continue; zs = ze = z1; }
                    }
                    uint32_t s0 = cell_start[col + zs], s1 = cell_start[col + ze + 1];
                    // candidates in batches of 8: all coordinate loads of a batch are issued before the first push
                    // (a push is LDS traffic and branches; interleaved with the loads it exposes one memory latency
                    // per candidate)
                    for (uint32_t sb = s0; sb < s1; sb += 8) {
                        float cx[8], cy[8], cz[8];
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const uint32_t s = sb + e < s1 ? sb + e : s1 - 1;
                            cx[e] = spts[3 * s]; cy[e] = spts[3 * s + 1]; cz[e] = spts[3 * s + 2];
                        }
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            if (sb + e >= s1) break;
                            const double dx = qx - (double)cx[e], dy = qy - (double)cy[e], dz = qz - (double)cz[e];
                            const double d = fma(dz, dz, fma(dy, dy, dx * dx));
                            if (r2max >= 0.0 && !(d < r2max)) continue;
                            if (d > gate) continue;                 // cannot enter a full heap (ties are decided by push)
                            heap.push(d, sidx ? sidx[sb + e] : 0);
                            gate = heap.full() ? heap.worst() : INFINITY;
                        }
                    }
                }
            }
    }
}

// Radius visitor (cluster_dbscan, remove_radius_outlier): every point with d2 < r2 (AC3, strict), in cell-sorted position order
// within each (x, y) column, is handed to visit(sorted position, d2); visit returns true to stop the walk.  The block is the cell
// range that holds [q - eps', q + eps'] on every axis: cell_coord is monotone, and eps' = eps (1 + 1e-9) plus 1e-12 of the
// coordinates' magnitude lies beyond every rounding of q - p and of d2 < eps^2, so no point inside the radius is missed for any h.
template <class Visit>
__device__ __forceinline__ void grid_radius_scan(const GridParams &g, const uint32_t *__restrict__ cell_start,
                                                 const float *__restrict__ spts, const double q[3], double eps, double r2, Visit &&visit)
{
    int lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double e = eps * (1.0 + 1e-9) + 1e-12 * (fabs(q[a]) + fabs(g.org[a]) + g.h);
        lo[a] = cell_coord(q[a] - e, g.org[a], g.h, g.dim[a]);
        hi[a] = cell_coord(q[a] + e, g.org[a], g.h, g.dim[a]);
    }
    for (int x = lo[0]; x <= hi[0]; ++x)
        for (int y = lo[1]; y <= hi[1]; ++y) {
            const int64_t col = ((int64_t)x * g.dim[1] + y) * g.dim[2];
            const uint32_t s0 = cell_start[col + lo[2]], s1 = cell_start[col + hi[2] + 1];     // a column's cells are contiguous
            for (uint32_t s = s0; s < s1; ++s) {
                const float *p = spts + 3 * (int64_t)s;
                const double dx = q[0] - (double)p[0], dy = q[1] - (double)p[1], dz = q[2] - (double)p[2];
                const double d = fma(dz, dz, fma(dy, dy, dx * dx));
                if (d < r2 && visit(s, d)) return;
            }
        }
}

// ---- wave-per-query neighbour selection (knn_wave_kernel below: SOR, normals / covariances, the hybrid neighbour lists) ----------------
// The lanes gather the squared distances (AC3, fp64) of the points of the (2r+1)^3 cell block around the query into
// LDS (every (x, y) column of the block is one contiguous run of the cell-sorted points: 64 columns at a time, lane c
// looks up run c, a wave scan places the runs, all candidates of the chunk are fetched together and the ones that pass
// d^2 <= tau, d^2 < r2max are appended by ballot + popcount).  The k-th smallest is found by counting the IEEE bit
// patterns into buckets (d^2 >= 0: the patterns order like the values; wave_kth_pattern below) and the search ends
// when that value lies inside the distance the block covers -- the termination rule of the ring walk above
// (grid_knn_scan).  Otherwise the k-th candidate found so far bounds the true k-th distance: the candidates are
// gathered again, only those within it, from the block that covers it.  When the buffer fills, gathering stops; the
// cap candidates held are still real points, so their k-th smallest is a valid bound too.  The wave's reductions, scans and
// broadcasts are those of kpx_wave.h (vector ALU only, no ds_bpermute); every call site below is wave-uniform.

// squared distance the block [c-r, c+r] covers around q (infinity once it holds the whole grid)
__device__ __forceinline__ double block_cover2(const GridParams &g, const double q[3], const int c[3], int r)
{
    double dcov = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double lo = g.org[a] + (double)(c[a] - r) * g.h;
        const double hi = g.org[a] + (double)(c[a] + r + 1) * g.h;
        const double dl = (c[a] - r <= 0) ? INFINITY : q[a] - lo;
        const double dh = (c[a] + r + 1 >= g.dim[a]) ? INFINITY : hi - q[a];
        dcov = fmin(dcov, fmin(dl, dh));
    }
    if (dcov == INFINITY) return INFINITY;
    if (dcov < 0.0) dcov = 0.0;
    return dcov * dcov * (1.0 - 1e-12);
}

struct WaveKnnScratch {        // LDS owned by one wave
    double *vals;              // cap candidate distances
    uint32_t *pos;             // cap sorted positions of the candidates (POS only)
    uint32_t *run_s0;          // 64
    int32_t *run_off;          // 64
    int cap;
    uint32_t *hist;            // kKnnBuckets bucket counts of the counting selection (16-byte aligned)
};
constexpr int kKnnBuckets = 256;

// ---- k-th smallest by COUNTING (round 5) ---------------------------------------------------------------------------------------------
// The rank-th smallest (1-based) of the 32-bit keys key(t), t < m, that are in the set and lie in the window [a, a + range]: the window is
// cut into <= 256 buckets of 2^shift, every key inside adds one to its bucket (LDS atomics), lane l sums its four buckets, a wave scan
// finds the bucket of the rank-th and the next level looks inside that bucket only.  It ends with the key itself (a bucket one value wide,
// exact = false) or -- usually after two levels -- with the upper end of a bucket whose LAST key is the rank-th: a pivot with exactly
// `rank` window keys at or below it (exact = true).  The caller has taken the keys below the window out of `rank` and knows that none
// above it matters.  A bisection over the same values took ~24 (high words) to ~60 (64-bit patterns) passes over the candidates.
template <class KeyF>
__device__ __forceinline__ unsigned wave_count_select(KeyF key, int m, unsigned a, unsigned range, int rank, uint32_t *__restrict__ hist, bool &exact)
{
    const int lane = threadIdx.x & 63;
    exact = false;
    while (range > 0u) {
        const int shift = range >= 256u ? 24 - __builtin_clz(range) : 0;      // range >> shift <= 255
        uint4 *hz = reinterpret_cast<uint4 *>(hist + 4 * lane);
        hz[0] = make_uint4(0u, 0u, 0u, 0u);
        wave_lds_fence();
        for (int t = lane; t < m; t += 64) {
            unsigned kv;
            if (key(t, kv) && kv - a <= range) __hip_atomic_fetch_add(hist + ((kv - a) >> shift), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        wave_lds_fence();
        const uint4 t4 = hz[0];
        const int hv[4] = { (int)t4.x, (int)t4.y, (int)t4.z, (int)t4.w };
        const int lsum = hv[0] + hv[1] + hv[2] + hv[3];
        const int incl = wave_incl_scan_i32(lsum), excl = incl - lsum;
        const bool mine = rank > excl && rank <= incl;
        int B = -1, cb = 0, hb = 0;
        if (mine) {
            int cum = excl;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                if (B < 0 && rank <= cum + hv[w]) { B = 4 * lane + w; cb = cum; hb = hv[w]; }
                cum += hv[w];
            }
        }
        const unsigned long long bm = __builtin_amdgcn_ballot_w64(mine);
        if (bm == 0ull) return a;                                   // fewer than `rank` keys in the window: the caller's count is off
        const int owner = __builtin_ctzll(bm);
        B = wave_bcast(B, owner); cb = wave_bcast(cb, owner); hb = wave_bcast(hb, owner);
        const unsigned wend = a + range, bstart = a + ((unsigned)B << shift), bspan = (1u << shift) - 1u;
        const unsigned bend = wend - bstart < bspan ? wend : bstart + bspan;      // the window's end may cut its last bucket
        if (rank - cb == hb) { exact = true; return bend; }        // the rank-th is the last of its bucket
        if (shift == 0) return bstart;                              // one value wide: THE key
        rank -= cb; a = bstart; range = bend - bstart;
    }
    return a;
}
// A threshold thr with { pattern <= thr } = the kk smallest of the m non-negative doubles vals[0 .. m) in LDS plus whatever ties with the
// kk-th (1 <= kk < m): high words first (zero distances -- the query itself, its duplicates -- are counted, not bucketed: with zero in the
// window the first level's buckets are eight binades wide), low words only among the candidates that share the kk-th high word.
// The statistics of the high words -- smallest non-zero, largest, number of zeros -- come from the gather, which tracks them per lane
// for the candidates it stores (WaveHighStats).
struct WaveHighStats {
    unsigned vmin, vmax;
    int zeros;
    __device__ void reset() { vmin = 0xFFFFFFFFu; vmax = 0u; zeros = 0; }
    __device__ void add(double d)
    {
        const unsigned h = (unsigned)((unsigned long long)__double_as_longlong(d) >> 32);
        zeros += h == 0u ? 1 : 0;
        const unsigned nz = h == 0u ? 0xFFFFFFFFu : h;
        vmin = nz < vmin ? nz : vmin; vmax = h > vmax ? h : vmax;
    }
};
__device__ __forceinline__ unsigned long long wave_kth_pattern(const double *__restrict__ vals, int m, int kk, uint32_t *__restrict__ hist, const WaveHighStats &hs)
{
    const int lane = threadIdx.x & 63;
    const uint32_t *w32 = reinterpret_cast<const uint32_t *>(vals);           // little endian: word 2 t + 1 is the high word
    const unsigned vmin = wave_min_u32(hs.vmin), vmax = wave_max_u32(hs.vmax);
    const int zeros = wave_sum_i32(hs.zeros);
    unsigned P = 0u;
    bool exact = false;
    if (kk > zeros) {
        P = vmin;
        if (vmin < vmax)
            P = wave_count_select([&](int t, unsigned &kv) { kv = w32[2 * t + 1]; return kv != 0u; }, m, vmin, vmax - vmin, kk - zeros, hist, exact);
        if (exact) return ((unsigned long long)P << 32) | 0xFFFFFFFFull;
    }
    int c_less = 0, c_eq = 0;
    unsigned lmin = 0xFFFFFFFFu, lmax = 0u;
    for (int t = lane; t < m; t += 64) {
        const unsigned h = w32[2 * t + 1];
        c_less += h < P ? 1 : 0;
        if (h == P) { const unsigned l = w32[2 * t]; ++c_eq; lmin = l < lmin ? l : lmin; lmax = l > lmax ? l : lmax; }
    }
    c_less = wave_sum_i32(c_less); c_eq = wave_sum_i32(c_eq);
    const int r2 = kk - c_less;                                                // rank of the kk-th among the candidates with high word P
    if (r2 >= c_eq) return ((unsigned long long)P << 32) | 0xFFFFFFFFull;      // all of them are selected
    lmin = wave_min_u32(lmin); lmax = wave_max_u32(lmax);
    unsigned Q = lmin;
    if (lmin < lmax)
        Q = wave_count_select([&](int t, unsigned &kv) { kv = w32[2 * t]; return w32[2 * t + 1] == P; }, m, lmin, lmax - lmin, r2, hist, exact);
    return ((unsigned long long)P << 32) | Q;
}
struct WaveKnnResult {
    int m;                     // candidates in vals / pos
    int kk;                    // neighbours selected: min(k, points within r2max)
    int cnt;                   // candidates with pattern <= thr (>= kk: ties at the k-th value)
    unsigned long long thr;    // bit pattern: the selected set is {d^2 pattern <= thr}
    double top;                // largest selected d^2
};
// Returns false when the query does not fit the buffer (the caller hands it to the next pass).
template <bool POS>
__device__ __forceinline__ bool wave_knn_select(const GridParams &g, const uint32_t *__restrict__ cell_start, const float *__restrict__ spts,
                                                const double q[3], int k, double r2max, const WaveKnnScratch &sc, WaveKnnResult &out)
{
    const int lane = threadIdx.x & 63;
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = cell_coord(q[a], g.org[a], g.h, g.dim[a]);
    int maxr = g.dim[0] > g.dim[1] ? g.dim[0] : g.dim[1];
    if (g.dim[2] > maxr) maxr = g.dim[2];
    bool truncated = false;
    WaveHighStats hs;                                             // per lane, of the candidates this lane stored in the last gather
    hs.reset();
    auto gather_block = [&](int r, double tau) -> int {
        const int xa = c[0] - r < 0 ? 0 : c[0] - r, xb = c[0] + r >= g.dim[0] ? g.dim[0] - 1 : c[0] + r;
        const int ya = c[1] - r < 0 ? 0 : c[1] - r, yb = c[1] + r >= g.dim[1] ? g.dim[1] - 1 : c[1] + r;
        const int za = c[2] - r < 0 ? 0 : c[2] - r, zb = c[2] + r >= g.dim[2] ? g.dim[2] - 1 : c[2] + r;
        const int ny = yb - ya + 1, ncols = (xb - xa + 1) * ny;
        int m = 0;
        truncated = false;
        hs.reset();                                               // every gather starts over: a round that gathers again, or a truncated one
        for (int c0 = 0; c0 < ncols && !truncated; c0 += 64) {
            const int nruns = ncols - c0 < 64 ? ncols - c0 : 64;
            uint32_t s0 = 0;
            int len = 0;
            if (lane < nruns) {
                const int x = xa + (c0 + lane) / ny, y = ya + (c0 + lane) % ny;
                const int64_t col = ((int64_t)x * g.dim[1] + y) * g.dim[2];
                s0 = cell_start[col + za];
                len = (int)(cell_start[col + zb + 1] - s0);
            }
            const int incl = wave_incl_scan_i32(len);
            const int mc = wave_bcast(incl, 63);
            if (mc == 0) continue;
            sc.run_s0[lane] = s0;
            sc.run_off[lane] = incl - len;
            wave_lds_fence();
            for (int t0 = 0; t0 < mc; t0 += 64) {
                const int t = t0 + lane;
                double d = INFINITY;
                uint32_t sp = 0;
                if (t < mc) {
                    int lo = 0, hi = nruns - 1;                                    // last run with off <= t
                    while (lo < hi) {
                        const int mid = (lo + hi + 1) >> 1;
                        if (sc.run_off[mid] <= t) lo = mid; else hi = mid - 1;
                    }
                    sp = sc.run_s0[lo] + (uint32_t)(t - sc.run_off[lo]);
                    const float *pp = spts + 3 * (int64_t)sp;
                    const double dx = q[0] - (double)pp[0], dy = q[1] - (double)pp[1], dz = q[2] - (double)pp[2];
                    d = fma(dz, dz, fma(dy, dy, dx * dx));
                }
                const bool keep = t < mc && d <= tau && d < r2max;
                const unsigned long long km = __builtin_amdgcn_ballot_w64(keep);
                const int pos = m + __builtin_popcountll(km & ((1ull << lane) - 1ull));
                if (keep && pos < sc.cap) {
                    hs.add(d);
                    sc.vals[pos] = d;
                    if (POS) sc.pos[pos] = sp;
                }
                m += __builtin_popcountll(km);
                if (m >= sc.cap) { m = sc.cap; truncated = true; break; }
            }
            wave_lds_fence();
        }
        return m;
    };

    double tau = INFINITY;
    int r = 1;
    for (int round = 0; round <= 24; ++round) {                // safety net: past it the query goes to the next pass
        const int m = gather_block(r, tau);
        wave_lds_fence();
        const double cov2 = block_cover2(g, q, c, r);
        const bool whole = cov2 == INFINITY || cov2 >= r2max;   // the block holds everything that may be selected
        if (!truncated && m < k && !whole) {                    // too few candidates: grow by the density seen so far
            const double f = cbrt((double)(k + 1) / (double)(m > 0 ? m : 1));
            int rn = (int)((double)r * (f < 4.0 ? f : 4.0)) + 1;
            r = rn > r ? rn : r + 1;
            if (r > maxr) r = maxr;
            continue;
        }
        const int kk = m < k ? m : k;
        // the threshold of the kk smallest patterns
        unsigned long long lo = 0ull;
        if (m > k) lo = wave_kth_pattern(sc.vals, m, kk, sc.hist, hs);            // by counting (above)
        else if (m > 0) {                                       // everything gathered is selected: the largest pattern
            for (int t = lane; t < m; t += 64) {
                const unsigned long long p = (unsigned long long)__double_as_longlong(sc.vals[t]);
                lo = p > lo ? p : lo;
            }
            lo = wave_max_u64(lo);
        }
        double top = 0.0;
        int cnt = 0;
        for (int t0 = 0; t0 < m; t0 += 64) {
            const int t = t0 + lane;
            const bool le = t < m && (unsigned long long)__double_as_longlong(sc.vals[t]) <= lo;
            if (le) top = fmax(top, sc.vals[t]);
            cnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(le));
        }
        top = wave_max_f64(top);
        if (!truncated && (whole || top < cov2)) {
            out.m = m; out.kk = kk; out.cnt = cnt; out.thr = lo; out.top = top;
            return true;
        }
        // the k-th candidate found so far bounds the true k-th distance: gather again, only what lies within it, from
        // the block that covers it -- that settles the query unless even the ball overflows the buffer
        if (truncated && top >= tau) return false;
        tau = top;
        int rn = (int)(sqrt(top) / g.h) + 1;
        if (rn > maxr) rn = maxr;
        r = rn;
        wave_lds_fence();
    }
    return false;
}


// More candidates at the k-th distance than slots: the `need` lowest ORIGINAL indices among them stay (the (d^2, index)
// order of the heaps above).  Returns the largest original index that is kept among the ties (INT_MAX: all of them).
__device__ __forceinline__ int32_t wave_knn_tie_threshold(const WaveKnnScratch &sc, const WaveKnnResult &res, const int32_t *__restrict__ sidx)
{
    if (res.cnt <= res.kk) return INT_MAX;
    const int lane = threadIdx.x & 63;
    const unsigned long long topp = (unsigned long long)__double_as_longlong(res.top);
    int ntied = 0;
    for (int t0 = 0; t0 < res.m; t0 += 64) {
        const int t = t0 + lane;
        const bool tie = t < res.m && (unsigned long long)__double_as_longlong(sc.vals[t]) == topp;
        ntied += __builtin_popcountll(__builtin_amdgcn_ballot_w64(tie));
    }
    const int need = res.kk - (res.cnt - ntied);
    int32_t last = -1;
    for (int round = 0; round < need; ++round) {
        int32_t cand = INT_MAX;
        for (int t = lane; t < res.m; t += 64)
            if ((unsigned long long)__double_as_longlong(sc.vals[t]) == topp) {
                const int32_t oi = sidx[sc.pos[t]];
                if (oi > last && oi < cand) cand = oi;
            }
        last = (int32_t)wave_min_u32((unsigned)cand);              // original indices: >= 0, the unsigned order is theirs
    }
    return last;
}
// is candidate t one of the kk selected neighbours?
__device__ __forceinline__ bool wave_knn_is_selected(const WaveKnnScratch &sc, const WaveKnnResult &res, const int32_t *__restrict__ sidx,
                                                     int32_t idx_thr, int t)
{
    const unsigned long long p = (unsigned long long)__double_as_longlong(sc.vals[t]);
    const unsigned long long topp = (unsigned long long)__double_as_longlong(res.top);
    if (p > res.thr) return false;
    if (p < topp || res.cnt == res.kk) return true;
    return p == topp && sidx[sc.pos[t]] <= idx_thr;
}

// ---- the two query kernels and their host cascade ------------------------------------------------------------------------------------
// An operator is a small struct Op, passed by value:
//     Op::kPos                    the wave form keeps the candidates' sorted positions (identities matter); false: values only, no `pos`
//                                 half is carved or touched
//     Op::Heap                    HeapD or HeapDI; with kPos the ring walk is handed op.sidx and the heap holds original indices
//     op.r2max(heap_walk)         the hybrid search's squared radius in the convention of wave_knn_select / grid_knn_scan
//     op.defer(s)                 lane 0, when the wave form hands query s to the next pass
//     op.wave(sc, res, s, spts)   the whole wave, with the selected set of query s in LDS.  The operator OWNS the wave's scratch from
//                                 here on: it may overwrite sc.vals, sc.run_s0 and sc.run_off (SorOp stores negated roots over the
//                                 distances and lists positions in run_off), so nothing after op.wave -- the kernel's epilogue, a second
//                                 consumer -- may read them; the next query's gather fills them again
//     op.heap(s, heap)            one thread, with the filled heap of query s (heap_alt: a second consumer, chosen by the host)
// Queries are cell-sorted positions: [q0, q1), or -- in_list != NULL -- in_list[0 .. *in_count), the ones an earlier pass listed.
template <class Op, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void knn_wave_kernel(const GridParams *__restrict__ gp, const uint32_t *__restrict__ cell_start,
                                                              const float *__restrict__ spts, int64_t q0, int64_t q1, int k, int cap, Op op,
                                                              const int32_t *__restrict__ in_list, const int32_t *__restrict__ in_count,
                                                              int32_t *__restrict__ fb_list, int32_t *__restrict__ fb_count)
{
    extern __shared__ __align__(16) double lds[];                // WAVES x cap distances, then (kPos) WAVES x cap positions
    __shared__ uint32_t run_s0[WAVES][64];
    __shared__ int32_t run_off[WAVES][64];
    __shared__ __align__(16) uint32_t knn_hist[WAVES][kKnnBuckets];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t *pos = nullptr;
    if constexpr (Op::kPos) pos = reinterpret_cast<uint32_t *>(lds + (size_t)WAVES * cap) + (size_t)wave * cap;
    const WaveKnnScratch sc{ lds + (size_t)wave * cap, pos, run_s0[wave], run_off[wave], cap, knn_hist[wave] };
    const GridParams g = *gp;
    const int64_t nq = in_list ? (int64_t)*in_count : q1 - q0;
    for (int64_t e = (int64_t)blockIdx.x * WAVES + wave; e < nq; e += (int64_t)gridDim.x * WAVES) {
        const int64_t s = in_list ? (int64_t)in_list[e] : q0 + e;
        const double q[3] = { (double)spts[3 * s], (double)spts[3 * s + 1], (double)spts[3 * s + 2] };
        WaveKnnResult res;
        if (!wave_knn_select<Op::kPos>(g, cell_start, spts, q, k, op.r2max(false), sc, res)) {      // does not fit the buffer
            if (lane == 0) { fb_list[atomicAdd(fb_count, 1)] = (int32_t)s; op.defer(s); }
            continue;
        }
        op.wave(sc, res, s, spts);
        wave_lds_fence();
    }
}
// ---- four queries per wave: a query per row of 16 lanes (SOR, normals / covariances) -------------------------------------------------------
// knn_wave_kernel pays its fixed work -- cell coordinates and cover in fp64, the run look-up, the scans, every level of the counting
// selection, the reductions -- once per wave and so once per query; only the gather and the sums scale with a query's 150-250
// candidates.  Here row g of a wave takes query 4 e + g and every wave-wide step serves four queries; the reductions and scans are the
// row forms of kpx_wave.h.  The kernel knows the COMMON PATH only, round 0 of wave_knn_select at r = 1: the clipped 3 x 3 x 3 block (at
// most nine runs), candidates appended in the same ascending order (the row's 16 bits of the ballot), the kk smallest by counting the
// high words.  It SETTLES a query only when that is the wave kernel's answer too -- not truncated; m >= k with the k-th inside the cover
// (at least kk candidates strictly nearer than cov2, the rule of sor_block_kernel), or m < k with the block whole; and a high-word pivot
// with exactly kk candidates at or below it, so cnt == kk and neither the low words nor the index tie rule are ever asked -- and lists
// everything else for the unchanged cascade behind it (knn_wave_kernel at its present buffer, then the later passes): a listed query
// gets bit for bit what it always got.  `cap` (the buffer per query, below the wave pass's) is free to tune: overflow only defers.
// Control flow is wave-uniform with all 64 lanes active: rows that are finished, deferred or past the end are predicated, a tail row
// replays the last query with its stores suppressed.
// An operator of this kernel has, besides the members listed above,
//     op.row(res, s, spts)        all four rows at once, each with ITS query s and selected set (RowKnnResult).  The sums keep the wave
//                                 form's association: there lane l adds candidates l, l + 64, ... in turn and wave_sum_down_* folds
//                                 halves, then row pairs, then the row; here lane j of the row keeps the four accumulators a_q of
//                                 t = j + 16 q (mod 64) and forms (a0 + a2) + (a1 + a3) before the row's four steps.
constexpr int kKnnRowBuckets = 256;        // per row: 16 per lane
struct RowKnnResult {
    double *vals;              // the row's m candidate distances (the operator may overwrite them)
    const uint32_t *pos;       // their sorted positions (kPos only)
    uint32_t *list;            // kKnnRowBuckets / 4 (= 64) free words of the row
    int m, kk, k;              // selected: the kk <= k candidates t < m whose d^2 high word is <= hi_thr (m = 0: nothing to store)
    unsigned hi_thr;
    int trips16;               // wave-uniform: 16 * trips16 covers every row's m
    bool store;                // false: a tail row, or a query that was handed on -- compute, store nothing
};
template <class Op, int WAVES>
__global__ __launch_bounds__(WAVES * 64, Op::kGroupWavesPerSimd) void knn_group_kernel(const GridParams *__restrict__ gp, const uint32_t *__restrict__ cell_start,
                                                               const float *__restrict__ spts, int64_t q0, int64_t q1, int k, int cap, Op op,
                                                               int32_t *__restrict__ fb_list, int32_t *__restrict__ fb_count)
{
    extern __shared__ __align__(16) double lds[];                // WAVES x 4 x cap distances, then (kPos) WAVES x 4 x cap positions
    __shared__ uint32_t run_s0[WAVES][4][16];
    __shared__ int32_t run_off[WAVES][4][16];
    __shared__ __align__(16) uint32_t row_hist[WAVES][4][kKnnRowBuckets / 4];      // byte counters: cap <= 256
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, row = lane >> 4, j = lane & 15;
    double *vals = lds + ((size_t)wave * 4 + row) * cap;
    uint32_t *pos = nullptr;
    if constexpr (Op::kPos) pos = reinterpret_cast<uint32_t *>(lds + (size_t)WAVES * 4 * cap) + ((size_t)wave * 4 + row) * cap;
    const uint32_t *w32 = reinterpret_cast<const uint32_t *>(vals);            // little endian: word 2 t + 1 is the high word
    uint32_t *rs0 = run_s0[wave][row], *hist = row_hist[wave][row];
    int32_t *roff = run_off[wave][row];
    const GridParams g = *gp;
    const int64_t nq = q1 - q0;
    const double r2max = op.r2max(false);
    for (int64_t e = (int64_t)blockIdx.x * WAVES + wave; 4 * e < nq; e += (int64_t)gridDim.x * WAVES) {
        const bool valid = 4 * e + row < nq;
        const int64_t s = q0 + (valid ? 4 * e + row : nq - 1);
        const double q[3] = { (double)spts[3 * s], (double)spts[3 * s + 1], (double)spts[3 * s + 2] };
        int c[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = cell_coord(q[a], g.org[a], g.h, g.dim[a]);
        const double cov2 = block_cover2(g, q, c, 1);
        const bool whole = cov2 == INFINITY || cov2 >= r2max;   // the block holds everything that may be selected
        // the row's runs, one per (x, y) column of the clipped block, in the wave kernel's order
        const int xa = c[0] - 1 < 0 ? 0 : c[0] - 1, xb = c[0] + 1 >= g.dim[0] ? g.dim[0] - 1 : c[0] + 1;
        const int ya = c[1] - 1 < 0 ? 0 : c[1] - 1, yb = c[1] + 1 >= g.dim[1] ? g.dim[1] - 1 : c[1] + 1;
        const int za = c[2] - 1 < 0 ? 0 : c[2] - 1, zb = c[2] + 1 >= g.dim[2] ? g.dim[2] - 1 : c[2] + 1;
        const int ny = yb - ya + 1, ncols = (xb - xa + 1) * ny;
        uint32_t s0 = 0;
        int len = 0;
        if (j < ncols) {
            const int x = xa + j / ny, y = ya + j % ny;
            const int64_t col = ((int64_t)x * g.dim[1] + y) * g.dim[2];
            s0 = cell_start[col + za];
            len = (int)(cell_start[col + zb + 1] - s0);
        }
        const int incl = row_incl_scan_i32(len);
        const int mc = row_sum_i32(len);
        rs0[j] = s0;
        roff[j] = j < ncols ? incl - len : INT_MAX;
        wave_lds_fence();
        const int mcmax = (int)wave_max_u32((unsigned)mc);
        // The nine runs of the row in registers (offset; start minus offset): the run of candidate t is the last one whose offset is
        // <= t (the offsets ascend; INT_MAX past the last run) -- a chain of compares, no LDS look-up inside the loop.  Op::kGroupTrips trips of 16
        // candidates are fetched together (a lane past its row's end fetches the query itself), then appended in order.
        int roffs[9];
        uint32_t rbase[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) { roffs[i] = roff[i]; rbase[i] = rs0[i] - (uint32_t)roffs[i]; }
        int m = 0, nin = 0;                                       // m: the same in all lanes of the row; nin: this lane's candidates inside the cover
        WaveHighStats hs;
        hs.reset();
        constexpr int U = Op::kGroupTrips;
        for (int t0 = 0; t0 < mcmax; t0 += 16 * U) {
            uint32_t sp[U];
            float px[U], py[U], pz[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + 16 * u + j;
                uint32_t b = rbase[0];
#pragma unroll
                for (int i = 1; i < 9; ++i) b = roffs[i] <= t ? rbase[i] : b;
                sp[u] = t < mc ? b + (uint32_t)t : (uint32_t)s;
                const float *pp = spts + 3 * (int64_t)sp[u];
                px[u] = pp[0]; py[u] = pp[1]; pz[u] = pp[2];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + 16 * u + j;
                const double dx = q[0] - (double)px[u], dy = q[1] - (double)py[u], dz = q[2] - (double)pz[u];
                const double d = fma(dz, dz, fma(dy, dy, dx * dx));
                const bool keep = t < mc && d < r2max;
                const unsigned bits = (unsigned)(__builtin_amdgcn_ballot_w64(keep) >> (16 * row)) & 0xFFFFu;
                const int p = m + __builtin_popcount(bits & ((1u << j) - 1u));
                if (keep && p < cap) {
                    hs.add(d);
                    nin += d < cov2 ? 1 : 0;
                    vals[p] = d;
                    if constexpr (Op::kPos) pos[p] = sp[u];
                }
                m += __builtin_popcount(bits);
            }
        }
        wave_lds_fence();
        const int kk = m < k ? m : k;
        nin = row_sum_i32(nin);
        // handed on: truncated (the wave kernel's `m >= cap`), too few candidates in a block that is not whole, the kk-th not inside the cover
        bool defer = m >= cap || (!whole && (m < k || nin < kk));
        unsigned hi_thr = 0xFFFFFFFFu;                            // m <= k: everything gathered is selected
        bool run = !defer && m > k;
        const int mmax = (int)wave_max_u32((unsigned)(defer ? 0 : m));
        if (__builtin_amdgcn_ballot_w64(run) != 0ull) {
            // the k-th smallest high word by counting (wave_count_select, per row): zero distances are counted, not bucketed, and the
            // window runs from the smallest non-zero high word to the largest
            const unsigned vmin = row_min_u32(hs.vmin), vmax = row_max_u32(hs.vmax);
            int rank = kk - row_sum_i32(hs.zeros);
            unsigned a = vmin, range = vmax - vmin;
            if (run && rank <= 0) {                               // the kk-th is a zero distance: exactly kk of them, or duplicates beyond k
                if (rank == 0) hi_thr = 0u; else defer = true;
                run = false;
            }
            while (__builtin_amdgcn_ballot_w64(run) != 0ull) {
                const int shift = range >= 256u ? 24 - __builtin_clz(range) : 0;      // range >> shift <= 255
                uint4 *hz = reinterpret_cast<uint4 *>(hist + 4 * j);      // this lane's 16 buckets, a byte each (a row holds fewer than 256 keys)
                hz[0] = make_uint4(0u, 0u, 0u, 0u);
                wave_lds_fence();
#pragma unroll 4
                for (int t = j; t < mmax; t += 16) {
                    if (run && t < m) {
                        const unsigned kv = w32[2 * t + 1], b = (kv - a) >> shift;
                        if (kv != 0u && kv - a <= range) __hip_atomic_fetch_add(hist + (b >> 2), 1u << (8 * (b & 3u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
                wave_lds_fence();
                const uint4 t4 = hz[0];
                const unsigned hw[4] = { t4.x, t4.y, t4.z, t4.w };
                int hv[16];
#pragma unroll
                for (int w = 0; w < 16; ++w) hv[w] = (int)((hw[w >> 2] >> (8 * (w & 3))) & 255u);
                int lsum = 0;
#pragma unroll
                for (int w = 0; w < 16; ++w) lsum += hv[w];
                const int incl2 = row_incl_scan_i32(lsum), excl = incl2 - lsum;
                const bool mine = run && rank > excl && rank <= incl2;
                unsigned found = 0u;                              // bit 31, bucket (8 bits), keys below it (11), keys in it (11): m < 2048
                if (mine) {
                    int cum = excl;
#pragma unroll
                    for (int w = 0; w < 16; ++w) {
                        if (found == 0u && rank <= cum + hv[w]) found = 0x80000000u | (unsigned)(16 * j + w) | ((unsigned)cum << 8) | ((unsigned)hv[w] << 19);
                        cum += hv[w];
                    }
                }
                found = row_reduce_u32(found, [](unsigned x, unsigned y) { return x | y; });      // one owner per row at most
                const int B = (int)(found & 255u), cb = (int)((found >> 8) & 2047u), hb = (int)((found >> 19) & 2047u);
                const unsigned wend = a + range, bstart = a + ((unsigned)B << shift), bspan = (1u << shift) - 1u;
                const unsigned bend = wend - bstart < bspan ? wend : bstart + bspan;      // the window's end may cut its last bucket
                if (run) {
                    if ((found >> 31) == 0u) { defer = true; run = false; }               // fewer than `rank` keys in the window: cannot happen
                    else if (rank - cb == hb) { hi_thr = bend; run = false; }             // the rank-th is the last of its bucket: exactly kk at or below
                    else if (shift == 0) { defer = true; run = false; }                   // candidates share the k-th high word: the low words decide
                    else { rank -= cb; a = bstart; range = bend - bstart; }
                }
            }
        }
        const RowKnnResult res{ vals, pos, hist, defer ? 0 : m, kk, k, hi_thr, (mmax + 15) >> 4, valid && !defer };
        op.row(res, s, spts);
        // what was not settled: ONE counter update per wave
        const bool hand = valid && defer && j == 0;
        const unsigned long long fm = __builtin_amdgcn_ballot_w64(hand);
        if (fm != 0ull) {
            int fb_base = 0;
            if (lane == 0) fb_base = atomicAdd(fb_count, __builtin_popcountll(fm));
            fb_base = wave_bcast(fb_base, 0);
            if (hand) fb_list[fb_base + __builtin_popcountll(fm & ((1ull << lane) - 1ull))] = (int32_t)s;
        }
        wave_lds_fence();
    }
}

// Exact ring walk, one thread per query (queries in cell order: neighbouring threads walk neighbouring cells) with a k-heap: in LDS
// (layout [slot][thread]), or -- gheap != NULL, k beyond what LDS holds -- in the workspace, strided by the grid's thread count.
template <class Op, bool ALT>
__global__ void knn_heap_kernel(const GridParams *__restrict__ gp, const uint32_t *__restrict__ cell_start, const float *__restrict__ spts,
                                int64_t q0, int64_t q1, int k, Op op, const int32_t *__restrict__ list, const int32_t *__restrict__ list_count,
                                double *__restrict__ gheap, int32_t *__restrict__ gix)
{
    extern __shared__ __align__(16) double lds[];
    const GridParams g = *gp;
    const int64_t total = list ? (int64_t)*list_count : q1 - q0;
    int32_t *ilds = reinterpret_cast<int32_t *>(lds + (size_t)k * blockDim.x);
    const size_t gt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = list ? (int64_t)list[t] : q0 + t;
        typename Op::Heap heap = Op::Heap::make(gheap ? gheap + gt : lds + threadIdx.x, gheap ? gix + gt : ilds + threadIdx.x,
                                                gheap ? (int)(gridDim.x * blockDim.x) : (int)blockDim.x, k);
        grid_knn_scan(g, cell_start, spts, Op::kPos ? op.sidx : (const int32_t *)nullptr, (double)spts[3 * s], (double)spts[3 * s + 1],
                      (double)spts[3 * s + 2], op.r2max(true), heap);
        if constexpr (ALT) op.heap_alt(s, heap);
        else op.heap(s, heap);
    }
}

// The heap pass's launch shape and, beyond lds_k, its heaps in the workspace (fewer blocks as k grows: <= 256 MB of distances).
struct KnnHeaps {
    bool global;
    int blocks, threads;
    size_t lds;
    double *gheap;
    int32_t *gix;
};
static inline KnnHeaps knn_heaps_carve(Arena &a, int k, int lds_k, bool with_idx, int lds_threads)
{
    KnnHeaps hp{ k > lds_k, 256, lds_threads, 0, nullptr, nullptr };
    if (hp.global) {
        while (hp.blocks > 8 && (size_t)hp.blocks * 64 * (size_t)k * sizeof(double) > ((size_t)256 << 20)) hp.blocks >>= 1;
        hp.threads = 64;
        hp.gheap = a.get<double>((size_t)hp.blocks * 64 * (size_t)k);
        if (with_idx) hp.gix = a.get<int32_t>((size_t)hp.blocks * 64 * (size_t)k);
    } else {
        hp.lds = (size_t)k * hp.threads * (sizeof(double) + (with_idx ? sizeof(int32_t) : 0));
    }
    return hp;
}
// dynamic LDS beyond 64 KB is granted per kernel: once per instantiation
template <auto Kernel, int Bytes> int knn_lds_limit()
{
    static const hipError_t e = hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, Bytes);
    if (e != hipSuccess) return fail(KPX_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed: %s", hipGetErrorString(e));
    return KPX_OK;
}
template <class Op> struct KnnWavePass {
    void (*kernel)(const GridParams *, const uint32_t *, const float *, int64_t, int64_t, int, int, Op, const int32_t *, const int32_t *, int32_t *, int32_t *);
    int rc, waves, cap, max_blocks;
    int32_t *fb_list;                      // what this pass cannot hold, for the next one
    bool on;
};
template <class Op, int WAVES> KnnWavePass<Op> knn_wave_pass(int cap, int max_blocks, int32_t *fb_list, bool on = true)
{
    return { knn_wave_kernel<Op, WAVES>, knn_lds_limit<knn_wave_kernel<Op, WAVES>, 96 * 1024>(), WAVES, cap, max_blocks, fb_list, on };
}
template <class Op> struct KnnHeapPass {
    void (*kernel)(const GridParams *, const uint32_t *, const float *, int64_t, int64_t, int, Op, const int32_t *, const int32_t *, double *, int32_t *);
    int rc;
};
template <class Op, bool ALT = false> KnnHeapPass<Op> knn_heap_pass() { return { knn_heap_kernel<Op, ALT>, knn_lds_limit<knn_heap_kernel<Op, ALT>, 160 * 1024>() }; }
// The cascade: every enabled wave pass searches what came in (all of [q0, q1), or `list`) and lists what it cannot hold for the next
// one; the heap pass takes whatever is left.  counters: one cleared word per wave pass (Grid::spare).
template <class Op>
int knn_cascade(const Grid &g, int k, const Op &op, int64_t q0, int64_t q1, const int32_t *list, const int32_t *count,
                std::initializer_list<KnnWavePass<Op>> passes, int32_t *counters, const KnnHeapPass<Op> &heap, const KnnHeaps &hp, hipStream_t st)
{
    const int64_t nq = q1 - q0;
    if (nq <= 0) return KPX_OK;
    for (const KnnWavePass<Op> &p : passes) {
        int32_t *fb_count = counters++;
        if (p.rc) return p.rc;
        if (!p.on) continue;
        const int64_t blocks = cdiv(nq, p.waves) > p.max_blocks ? p.max_blocks : cdiv(nq, p.waves);
        hipLaunchKernelGGL(p.kernel, dim3((unsigned)blocks), dim3(64 * p.waves), (size_t)p.waves * p.cap * (sizeof(double) + (Op::kPos ? sizeof(uint32_t) : 0)),
                           st, g.params, g.cell_start, g.sorted_pts, q0, q1, k, p.cap, op, list, count, p.fb_list, fb_count);
        list = p.fb_list; count = fb_count;
    }
    if (heap.rc) return heap.rc;
    hipLaunchKernelGGL(heap.kernel, dim3(hp.blocks), dim3(hp.threads), hp.lds, st, g.params, g.cell_start, g.sorted_pts, q0, q1, k, op, list, count,
                       hp.gheap, hp.gix);
    return KPX_OK;
}

// The group pass in front of a cascade: all of [q0, q1) through knn_group_kernel; what it does not settle is listed in fb_list, counted in
// *fb_count (a cleared word), and is the cascade's `list` / `count`.  CAP: the buffer per query, a multiple of 16 and at most 256 (the
// counting selection's buckets are bytes) -- overflow only defers, so it is the caller's to tune (KPX_KNN_GROUP_CAP_SOR / _NORMALS).
// -DKPX_KNN_GROUP=0 builds a library without the pass (A/B runs through KPX_LIBRARY).
#ifndef KPX_KNN_GROUP
#define KPX_KNN_GROUP 1
#endif
#ifndef KPX_KNN_GROUP_WAVES
#define KPX_KNN_GROUP_WAVES 2
#endif
template <class Op, int CAP>
int knn_group_pass(const Grid &g, int k, const Op &op, int64_t q0, int64_t q1, int32_t *fb_list, int32_t *fb_count, hipStream_t st)
{
    static_assert(CAP % 16 == 0 && CAP >= 64 && CAP <= 256, "the group buffer: a multiple of 16; the buckets of a row count its keys in bytes");
    constexpr int W = KPX_KNN_GROUP_WAVES;
    static const int rc = knn_lds_limit<knn_group_kernel<Op, W>, 96 * 1024>();
    if (rc) return rc;
    const int64_t nq = q1 - q0, blocks = cdiv(cdiv(nq, 4), W);
    ThreadResources &tr = thread_resources();                     // kpx_knn_group_last reads the counter word back
    tr.knn_group_word = nq > 0 ? fb_count : nullptr; tr.knn_group_given = nq > 0 ? nq : 0; tr.knn_group_stream = st;
    if (nq <= 0) return KPX_OK;
    hipLaunchKernelGGL((knn_group_kernel<Op, W>), dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(64 * W),
                       (size_t)W * 4 * CAP * (sizeof(double) + (Op::kPos ? sizeof(uint32_t) : 0)), st, g.params, g.cell_start, g.sorted_pts, q0, q1, k, CAP,
                       op, fb_list, fb_count);
    return KPX_OK;
}

}  // namespace kpx
