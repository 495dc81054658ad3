// kpx_cluster.hip -- radius-neighbourhood operators on the exact grid of kpx_knn.hip:
//   PointCloud.cluster_dbscan(eps, min_points)          ([O3D] PointCloud::ClusterDBSCAN)
//   PointCloud.remove_radius_outlier(nb_points, radius) ([O3D] PointCloud::RemoveRadiusOutliers)
//   keypoint.compute_iss_keypoints(...)                 ([O3D] geometry::keypoint::ComputeISSKeypoints; below, "ISS keypoints")
// Neighbours of i: every j (i itself included) with d2(i, j) < eps^2, AC3 arithmetic (d2 = fma(dz,dz, fma(dy,dy, dx*dx)), fp64
// differences of the float32 coordinates), strict <, the convention of the hybrid searches.
//
// DBSCAN computes the closed form of Open3D's sequential loop ("Clustering"):
//   core(i)    <=> |neighbours(i)| >= min_points
//   components  = connected components of the core points under the neighbour relation
//   cluster id  = rank of the component when components are ordered by their smallest core index
//   label(i)    = id of its component (core); smallest id among its core neighbours, or -1 (non-core)
// Passes, one thread per query in cell-sorted order, results by original index:
//   1 count   neighbours up to a cap (early stop): core flags; parent[i] = i
//   2 union   every core pair (j < i) hooks the larger root under the smaller (CAS): the root of a component is its smallest index
//   3 compress parent[i] = root
//   4 rank    ordered compaction of the roots (index order): rank[root] = cluster id, the count -> d_nclusters
//   5 label   core points take rank[parent[i]]; non-core points walk once more and take the smallest id of a core neighbour
// Nothing depends on the order in which the atomics land: the partition, its roots and the ranks are functions of the input.
#include <float.h>

#include "kpx_compact.h"
#include "kpx_fixed.h"
#include "kpx_gridknn.h"
#include "kpx_linalg.h"
#include "kpx_unionfind.h"

namespace kpx {

namespace {

constexpr int kClusterThreads = 256;

// cell occupancy of the grid: from the count cap (the work of the count pass), never from eps -- no result depends on h
double cluster_occupancy(int64_t cap)
{
    double occ = 0.5 * (double)cap;
    return occ < 8.0 ? 8.0 : (occ > 64.0 ? 64.0 : occ);
}

__device__ __forceinline__ void load_query(const float *spts, int64_t s, double q[3])
{
    q[0] = (double)spts[3 * s]; q[1] = (double)spts[3 * s + 1]; q[2] = (double)spts[3 * s + 2];
}

// pass 1: flag = (#neighbours >= cap), by sorted position (flag_s) and by original index (flag_o).  cap <= 1: every point (itself).
// parent (optional): parent[i] = i.
__global__ __launch_bounds__(kClusterThreads) void radius_count_kernel(const GridParams *__restrict__ gp, const uint32_t *__restrict__ cell_start,
                                                                       const float *__restrict__ spts, const int32_t *__restrict__ sidx, int64_t n,
                                                                       double eps, double r2, int64_t cap, uint8_t *__restrict__ flag_s,
                                                                       uint8_t *__restrict__ flag_o, int32_t *__restrict__ parent)
{
    const GridParams g = *gp;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        const int32_t i = sidx[s];
        int64_t cnt = 0;
        if (cap > 1) {
            double q[3];
            load_query(spts, s, q);
            grid_radius_scan(g, cell_start, spts, q, eps, r2, [&](uint32_t, double) { return ++cnt >= cap; });
        }
        const uint8_t f = (cap <= 1 || cnt >= cap) ? 1 : 0;
        flag_s[s] = f;
        flag_o[i] = f;
        if (parent) parent[i] = i;
    }
}

// pass 2: every edge between core points once (from its larger index); *err = 1 if a hook gave up
__global__ __launch_bounds__(kClusterThreads) void dbscan_union_kernel(const GridParams *__restrict__ gp, const uint32_t *__restrict__ cell_start,
                                                                       const float *__restrict__ spts, const int32_t *__restrict__ sidx, int64_t n,
                                                                       double eps, double r2, const uint8_t *__restrict__ core_s,
                                                                       int32_t *parent, int32_t *__restrict__ err)
{
    const GridParams g = *gp;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        if (!core_s[s]) continue;
        const int32_t i = sidx[s];
        int32_t ra = i;
        double q[3];
        load_query(spts, s, q);
        grid_radius_scan(g, cell_start, spts, q, eps, r2, [&](uint32_t t, double) {
            const int32_t j = sidx[t];
            if (j < i && core_s[t] && !uf_unite(parent, ra, j)) { atomicExch(err, 1); return true; }
            return false;
        });
    }
}

// pass 3: parent[i] = root for every core point (a concurrent reader sees the old parent or the root: both lead to the root)
__global__ __launch_bounds__(kClusterThreads) void dbscan_compress_kernel(const uint8_t *__restrict__ core_o, int64_t n, int32_t *parent)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (!core_o[i]) continue;
        int32_t r = parent[i];
        while (parent[r] != r) r = parent[r];
        parent[i] = r;
    }
}

// pass 4: the roots in index order
struct RootPred {
    const uint8_t *core; const int32_t *parent;
    __device__ bool operator()(int64_t i, int) const { return core[i] && parent[i] == (int32_t)i; }
};
struct RankEmit {
    int32_t *rank;
    __device__ void operator()(int64_t i, int, int32_t dst) const { rank[i] = dst; }
};
struct KeepPred {
    const uint8_t *keep;
    __device__ bool operator()(int64_t i, int) const { return keep[i] != 0; }
};
struct KeepEmit {
    int32_t *idx;
    __device__ void operator()(int64_t i, int, int32_t dst) const { idx[dst] = (int32_t)i; }
};

// pass 5a: labels of the core points (cid_s: by sorted position, -1 for non-core); a failed union turns the count into an error
__global__ __launch_bounds__(kClusterThreads) void dbscan_core_label_kernel(const int32_t *__restrict__ sidx, int64_t n, const uint8_t *__restrict__ core_s,
                                                                           const int32_t *__restrict__ parent, const int32_t *__restrict__ rank,
                                                                           int32_t *__restrict__ cid_s, int32_t *__restrict__ labels,
                                                                           const int32_t *__restrict__ err, int32_t *__restrict__ d_nclusters)
{
    if (blockIdx.x == 0 && threadIdx.x == 0 && *err) *d_nclusters = KPX_ERR_RANGE;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        const int32_t i = sidx[s];
        const int32_t c = core_s[s] ? rank[parent[i]] : -1;
        cid_s[s] = c;
        if (c >= 0) labels[i] = c;
    }
}

// pass 5b: non-core points take the smallest id among their core neighbours (the first cluster Open3D's loop grows into them)
__global__ __launch_bounds__(kClusterThreads) void dbscan_border_kernel(const GridParams *__restrict__ gp, const uint32_t *__restrict__ cell_start,
                                                                        const float *__restrict__ spts, const int32_t *__restrict__ sidx, int64_t n,
                                                                        double eps, double r2, const int32_t *__restrict__ cid_s,
                                                                        int32_t *__restrict__ labels)
{
    const GridParams g = *gp;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        if (cid_s[s] >= 0) continue;
        double q[3];
        load_query(spts, s, q);
        int32_t best = INT32_MAX;
        grid_radius_scan(g, cell_start, spts, q, eps, r2, [&](uint32_t t, double) {
            const int32_t c = cid_s[t];
            if (c >= 0 && c < best) best = c;
            return best == 0;                    // nothing is smaller than cluster 0
        });
        labels[sidx[s]] = best == INT32_MAX ? -1 : best;
    }
}

// ---- ISS keypoints ("ISS keypoints") -----------------------------------------------------------------------------------------
//   s_i = smallest eigenvalue e3 of the covariance of the points within salient_radius of i, if there are >= min_neighbors of them,
//         the covariance is not Eigen's isZero (some |C_ab| > 1e-12) and e2/e1 < gamma_21, e3/e2 < gamma_32 (e3 <= e2 <= e1); else 0
//   i is a keypoint <=> s_i > 0, i has >= min_neighbors points within non_max_radius, and none of them has a larger s
// Both passes: one thread per query in cell-sorted order on ONE grid whose cells are half the larger radius (a salient ball holds
// ~10^2 points: cells of 8 points would make the visitor walk hundreds of columns for it).
constexpr double kIssZero = 1e-12;          // Eigen's default precision of isZero() for double

// pass 1.  The moments are those of q - p_j (exact in fp64 for float32 coordinates; the covariance does not move with the origin and
// the sums stay small), Open3D's ComputeCovariance otherwise: nine raw moments / m, C_ab = E[ab] - E[a] E[b].
__global__ __launch_bounds__(kClusterThreads) void iss_saliency_kernel(const GridParams *__restrict__ gp, const uint32_t *__restrict__ cell_start,
                                                                       const float *__restrict__ spts, const int32_t *__restrict__ sidx, int64_t n,
                                                                       double eps, double r2, double gamma_21, double gamma_32, int64_t min_nb,
                                                                       double *__restrict__ sal_s, double *__restrict__ sal_o)
{
    const GridParams g = *gp;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        double q[3];
        load_query(spts, s, q);
        int64_t m = 0;
        double sx = 0.0, sy = 0.0, sz = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
        grid_radius_scan(g, cell_start, spts, q, eps, r2, [&](uint32_t t, double) {
            const float *p = spts + 3 * (int64_t)t;
            const double dx = q[0] - (double)p[0], dy = q[1] - (double)p[1], dz = q[2] - (double)p[2];
            ++m;
            sx += dx; sy += dy; sz += dz;
            sxx += dx * dx; sxy += dx * dy; sxz += dx * dz; syy += dy * dy; syz += dy * dz; szz += dz * dz;
            return false;
        });
        double sal = 0.0;
        if (m >= min_nb && m > 0) {
            const double sums[9] = { sx, sy, sz, sxx, sxy, sxz, syy, syz, szz };
            double c[6];
            cov6_from_moments(sums, (double)m, c);
            bool zero = true;
#pragma unroll
            for (int k = 0; k < 6; ++k) zero = zero && fabs(c[k]) <= kIssZero;
            if (!zero) {
                double w[3], V[9];
                sym3_eigen(c, w, V);
                if (w[1] / w[2] < gamma_21 && w[0] / w[1] < gamma_32) sal = w[0];          // IEEE comparisons: a NaN ratio fails
            }
        }
        if (sal_s) sal_s[s] = sal;
        sal_o[sidx[s]] = sal;
    }
}

// a caller's saliency (by original index) in cell-sorted order for pass 2
__global__ __launch_bounds__(kClusterThreads) void iss_gather_kernel(const int32_t *__restrict__ sidx, int64_t n, const double *__restrict__ sal_o,
                                                                     double *__restrict__ sal_s)
{
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) sal_s[s] = sal_o[sidx[s]];
}

// pass 2: the walk stops at the first neighbour with a larger saliency (a stopped walk is no keypoint whatever its count); equal
// saliencies do not suppress each other
__global__ __launch_bounds__(kClusterThreads) void iss_nonmax_kernel(const GridParams *__restrict__ gp, const uint32_t *__restrict__ cell_start,
                                                                     const float *__restrict__ spts, const int32_t *__restrict__ sidx, int64_t n,
                                                                     double eps, double r2, int64_t min_nb, const double *__restrict__ sal_s,
                                                                     uint8_t *__restrict__ flag_o)
{
    const GridParams g = *gp;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        const double si = sal_s[s];
        uint8_t f = 0;
        if (si > 0.0) {
            double q[3];
            load_query(spts, s, q);
            int64_t cnt = 0;
            bool beaten = false;
            grid_radius_scan(g, cell_start, spts, q, eps, r2, [&](uint32_t t, double) {
                ++cnt;
                beaten = si < sal_s[t];
                return beaten;
            });
            f = (!beaten && cnt >= min_nb) ? 1 : 0;
        }
        flag_o[sidx[s]] = f;
    }
}

// Mean over the m queries of the distance to the nearest OTHER point: row q of a 2-nearest search (d2 [m, stride], count [m]) adds
// sqrt(d2[q, 1]) when it has two results.  The sum is taken in 128-bit fixed point (kpx_fixed.h): exact, whatever the order.
__global__ __launch_bounds__(kClusterThreads) void nn_distance_sum_kernel(const double *__restrict__ d2, const int32_t *__restrict__ cnt, int64_t m,
                                                                          int32_t stride, unsigned long long *__restrict__ acc)
{
    unsigned long long lo = 0ull, hi = 0ull;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x)
        if (cnt[i] >= 2) {
            unsigned long long l, h;
            fixed_split(sqrt(d2[i * stride + 1]), l, h);
            fixed_accumulate(lo, hi, l, h);
        }
    fixed_add_words(acc, lo, hi);
}
__global__ void nn_distance_mean_kernel(const unsigned long long *__restrict__ acc, int64_t m, double *__restrict__ out)
{
    *out = fixed_value(acc[0], acc[1]) / (double)m;
}

unsigned launch_blocks(int64_t n)
{
    const int64_t b = cdiv(n > 0 ? n : 1, kClusterThreads);
    return (unsigned)(b > 65536 ? 65536 : b);
}

struct RadiusScratch {
    uint8_t *flag_s, *flag_o;
    int32_t *counts;               // compaction tiles
};
void radius_carve(Arena &a, int64_t n, RadiusScratch *r)
{
    const size_t nn = (size_t)(n > 0 ? n : 1);
    r->flag_s = a.get<uint8_t>(nn);
    r->flag_o = a.get<uint8_t>(nn);
    r->counts = a.get<int32_t>((size_t)compact_ws_ints(n));
}

int dbscan_impl(const float *pts, int64_t n, double eps, int32_t min_points, int32_t *labels, int32_t *d_nclusters, Arena &a, hipStream_t st)
{
    const int64_t cap = min_points;
    Grid g;
    int rc = grid_build(pts, n, cluster_occupancy(cap), a, &g, st);
    if (rc) return rc;
    RadiusScratch r;
    radius_carve(a, n, &r);
    const size_t nn = (size_t)(n > 0 ? n : 1);
    int32_t *parent = a.get<int32_t>(nn), *rank = a.get<int32_t>(nn), *cid_s = a.get<int32_t>(nn);
    if (a.dry) return KPX_OK;
    KPX_ARENA_CHECK(a);
    int32_t *err = g.spare;                   // cleared by the grid build
    const double r2 = eps * eps;
    const unsigned nb = launch_blocks(n);
    hipLaunchKernelGGL(radius_count_kernel, dim3(nb), dim3(kClusterThreads), 0, st, g.params, g.cell_start, g.sorted_pts, g.sorted_idx, n, eps, r2,
                       cap, r.flag_s, r.flag_o, parent);
    hipLaunchKernelGGL(dbscan_union_kernel, dim3(nb), dim3(kClusterThreads), 0, st, g.params, g.cell_start, g.sorted_pts, g.sorted_idx, n, eps, r2,
                       (const uint8_t *)r.flag_s, parent, err);
    hipLaunchKernelGGL(dbscan_compress_kernel, dim3(nb), dim3(kClusterThreads), 0, st, (const uint8_t *)r.flag_o, n, parent);
    KPX_LAUNCH_CHECK();
    rc = compact(RootPred{ r.flag_o, parent }, RankEmit{ rank }, n, 1, r.counts, d_nclusters, st);
    if (rc) return rc;
    hipLaunchKernelGGL(dbscan_core_label_kernel, dim3(nb), dim3(kClusterThreads), 0, st, (const int32_t *)g.sorted_idx, n, (const uint8_t *)r.flag_s,
                       (const int32_t *)parent, (const int32_t *)rank, cid_s, labels, (const int32_t *)err, d_nclusters);
    hipLaunchKernelGGL(dbscan_border_kernel, dim3(nb), dim3(kClusterThreads), 0, st, g.params, g.cell_start, g.sorted_pts, g.sorted_idx, n, eps, r2,
                       (const int32_t *)cid_s, labels);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

int radius_outlier_impl(const float *pts, int64_t n, int32_t nb_points, double radius, int32_t *keep_idx, int32_t *d_count, Arena &a, hipStream_t st)
{
    const int64_t cap = (int64_t)nb_points + 1;         // kept iff #neighbours > nb_points
    Grid g;
    int rc = grid_build(pts, n, cluster_occupancy(cap), a, &g, st);
    if (rc) return rc;
    RadiusScratch r;
    radius_carve(a, n, &r);
    if (a.dry) return KPX_OK;
    KPX_ARENA_CHECK(a);
    hipLaunchKernelGGL(radius_count_kernel, dim3(launch_blocks(n)), dim3(kClusterThreads), 0, st, g.params, g.cell_start, g.sorted_pts, g.sorted_idx, n,
                       radius, radius * radius, cap, r.flag_s, r.flag_o, (int32_t *)nullptr);
    KPX_LAUNCH_CHECK();
    return compact(KeepPred{ r.flag_o }, KeepEmit{ keep_idx }, n, 1, r.counts, d_count, st);
}

// ISS on one grid: saliency (sal_o written) when salient_radius > 0, else sal_o is the caller's; suppression and the ordered
// compaction when non_max_radius > 0.
int iss_impl(const float *pts, int64_t n, double salient_radius, double non_max_radius, double gamma_21, double gamma_32, int32_t min_neighbors,
             double *sal_o, int32_t *keep_idx, int32_t *d_count, Arena &a, hipStream_t st)
{
    const double rmax = salient_radius > non_max_radius ? salient_radius : non_max_radius;
    Grid g;
    int rc = grid_build(pts, n, 8.0, a, &g, st, 0.5 * rmax);
    if (rc) return rc;
    const size_t nn = (size_t)(n > 0 ? n : 1);
    double *sal_s = a.get<double>(nn);
    uint8_t *flag_o = a.get<uint8_t>(nn);
    int32_t *counts = a.get<int32_t>((size_t)compact_ws_ints(n));
    if (a.dry) return KPX_OK;
    KPX_ARENA_CHECK(a);
    const unsigned nb = launch_blocks(n);
    if (salient_radius > 0.0)
        hipLaunchKernelGGL(iss_saliency_kernel, dim3(nb), dim3(kClusterThreads), 0, st, g.params, g.cell_start, g.sorted_pts, g.sorted_idx, n,
                           salient_radius, salient_radius * salient_radius, gamma_21, gamma_32, (int64_t)min_neighbors,
                           non_max_radius > 0.0 ? sal_s : (double *)nullptr, sal_o);
    else
        hipLaunchKernelGGL(iss_gather_kernel, dim3(nb), dim3(kClusterThreads), 0, st, (const int32_t *)g.sorted_idx, n, (const double *)sal_o, sal_s);
    if (!(non_max_radius > 0.0)) { KPX_LAUNCH_CHECK(); return KPX_OK; }
    hipLaunchKernelGGL(iss_nonmax_kernel, dim3(nb), dim3(kClusterThreads), 0, st, g.params, g.cell_start, g.sorted_pts, g.sorted_idx, n, non_max_radius,
                       non_max_radius * non_max_radius, (int64_t)min_neighbors, (const double *)sal_s, flag_o);
    KPX_LAUNCH_CHECK();
    return compact(KeepPred{ flag_o }, KeepEmit{ keep_idx }, n, 1, counts, d_count, st);
}

}  // namespace

}  // namespace kpx

using namespace kpx;

KPX_EXPORT size_t kpx_dbscan_workspace_bytes(int64_t n)
{
    Arena a(nullptr, 0);
    dbscan_impl(nullptr, n, 1.0, 1, nullptr, nullptr, a, nullptr);
    return a.off;
}
KPX_EXPORT int kpx_cluster_dbscan(const float *pts, int64_t n, double eps, int32_t min_points, int32_t *labels, int32_t *d_nclusters, void *ws,
                                  size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(eps > 0.0, "cluster_dbscan: eps must be positive");
    KPX_REQUIRE(min_points >= 0, "cluster_dbscan: min_points must be non-negative");
    KPX_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "kpx_cluster_dbscan: bad size");
    KPX_REQUIRE(d_nclusters && ws, "kpx_cluster_dbscan: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) { KPX_HIP(hipMemsetAsync(d_nclusters, 0, sizeof(int32_t), st)); return KPX_OK; }
    KPX_REQUIRE(pts && labels, "kpx_cluster_dbscan: null pointer");
    Arena a(ws, ws_bytes);
    return dbscan_impl(pts, n, eps, min_points, labels, d_nclusters, a, st);
}

KPX_EXPORT size_t kpx_radius_outlier_workspace_bytes(int64_t n)
{
    Arena a(nullptr, 0);
    radius_outlier_impl(nullptr, n, 1, 1.0, nullptr, nullptr, a, nullptr);
    return a.off;
}
KPX_EXPORT int kpx_remove_radius_outlier(const float *pts, int64_t n, int32_t nb_points, double radius, int32_t *keep_idx, int32_t *d_count, void *ws,
                                         size_t ws_bytes, void *stream)
{
    // [O3D] RemoveRadiusOutliers
    KPX_REQUIRE(nb_points >= 1 && radius > 0.0, "Illegal input parameters, number of points and radius must be positive");
    KPX_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "kpx_remove_radius_outlier: bad size");
    KPX_REQUIRE(d_count && ws, "kpx_remove_radius_outlier: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) { KPX_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), st)); return KPX_OK; }
    KPX_REQUIRE(pts && keep_idx, "kpx_remove_radius_outlier: null pointer");
    Arena a(ws, ws_bytes);
    return radius_outlier_impl(pts, n, nb_points, radius, keep_idx, d_count, a, st);
}

KPX_EXPORT size_t kpx_iss_workspace_bytes(int64_t n)
{
    Arena a(nullptr, 0);
    iss_impl(nullptr, n, 1.0, 1.0, 0.0, 0.0, 0, nullptr, nullptr, nullptr, a, nullptr);
    return a.off;
}
#define KPX_ISS_RADIUS(r, name) KPX_REQUIRE((r) > 0.0 && (r) <= DBL_MAX, "compute_iss_keypoints: " name " must be positive and finite")
KPX_EXPORT int kpx_iss_saliency(const float *pts, int64_t n, double salient_radius, double gamma_21, double gamma_32, int32_t min_neighbors,
                                double *saliency, void *ws, size_t ws_bytes, void *stream)
{
    KPX_ISS_RADIUS(salient_radius, "salient_radius");
    KPX_REQUIRE(min_neighbors >= 0, "compute_iss_keypoints: min_neighbors must be non-negative");
    KPX_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "kpx_iss_saliency: bad size");
    KPX_REQUIRE(ws, "kpx_iss_saliency: null pointer");
    if (n == 0) return KPX_OK;
    KPX_REQUIRE(pts && saliency, "kpx_iss_saliency: null pointer");
    Arena a(ws, ws_bytes);
    return iss_impl(pts, n, salient_radius, 0.0, gamma_21, gamma_32, min_neighbors, saliency, nullptr, nullptr, a, (hipStream_t)stream);
}
KPX_EXPORT int kpx_iss_nonmax(const float *pts, int64_t n, const double *saliency, double non_max_radius, int32_t min_neighbors, int32_t *keep_idx,
                              int32_t *d_count, void *ws, size_t ws_bytes, void *stream)
{
    KPX_ISS_RADIUS(non_max_radius, "non_max_radius");
    KPX_REQUIRE(min_neighbors >= 0, "compute_iss_keypoints: min_neighbors must be non-negative");
    KPX_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "kpx_iss_nonmax: bad size");
    KPX_REQUIRE(d_count && ws, "kpx_iss_nonmax: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) { KPX_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), st)); return KPX_OK; }
    KPX_REQUIRE(pts && saliency && keep_idx, "kpx_iss_nonmax: null pointer");
    Arena a(ws, ws_bytes);
    return iss_impl(pts, n, 0.0, non_max_radius, 0.0, 0.0, min_neighbors, const_cast<double *>(saliency), keep_idx, d_count, a, st);
}
KPX_EXPORT int kpx_iss_keypoints(const float *pts, int64_t n, double salient_radius, double non_max_radius, double gamma_21, double gamma_32,
                                 int32_t min_neighbors, double *saliency, int32_t *keep_idx, int32_t *d_count, void *ws, size_t ws_bytes, void *stream)
{
    KPX_ISS_RADIUS(salient_radius, "salient_radius");
    KPX_ISS_RADIUS(non_max_radius, "non_max_radius");
    KPX_REQUIRE(min_neighbors >= 0, "compute_iss_keypoints: min_neighbors must be non-negative");
    KPX_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "kpx_iss_keypoints: bad size");
    KPX_REQUIRE(d_count && ws, "kpx_iss_keypoints: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) { KPX_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), st)); return KPX_OK; }
    KPX_REQUIRE(pts && saliency && keep_idx, "kpx_iss_keypoints: null pointer");
    Arena a(ws, ws_bytes);
    return iss_impl(pts, n, salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors, saliency, keep_idx, d_count, a, st);
}
#undef KPX_ISS_RADIUS

KPX_EXPORT int kpx_mean_nn_distance(const double *d2, const int32_t *count, int64_t m, int32_t stride, double *d_mean, void *ws, size_t ws_bytes,
                                    void *stream)
{
    KPX_REQUIRE(m >= 1 && stride >= 2, "kpx_mean_nn_distance: needs at least one row of a 2-nearest search");
    KPX_REQUIRE(d2 && count && d_mean && ws, "kpx_mean_nn_distance: null pointer");
    hipStream_t st = (hipStream_t)stream;
    Arena a(ws, ws_bytes);
    unsigned long long *acc = a.get<unsigned long long>(kFixedWords);
    KPX_ARENA_CHECK(a);
    KPX_HIP(hipMemsetAsync(acc, 0, kFixedWords * sizeof(unsigned long long), st));
    const int64_t b = cdiv(m, kClusterThreads);
    hipLaunchKernelGGL(nn_distance_sum_kernel, dim3((unsigned)(b > 1024 ? 1024 : b)), dim3(kClusterThreads), 0, st, d2, count, m, stride, acc);
    hipLaunchKernelGGL(nn_distance_mean_kernel, dim3(1), dim3(1), 0, st, (const unsigned long long *)acc, m, d_mean);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}
