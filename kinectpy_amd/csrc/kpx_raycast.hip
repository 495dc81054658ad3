// kpx_raycast.hip -- ray casts and closest points on triangle meshes ([O3D] t.geometry.RaycastingScene; arithmetic contract AC14,
// DESIGN.md 3 / 5.15).
//   scene  = ONE caller-owned buffer: header, the boxes of an implicit complete tree, the triangles' corners in curve order, their ids.
//            Nothing in it points back into the meshes it was built from.
//   build  = curve code of every triangle's centroid over the centroids' bounds (kpx_morton.h), one stable sort (kpx_sort.h), then the
//            boxes level by level: a leaf holds KPX_RAYSCENE_LEAF consecutive sorted triangles, a node KPX_RAYSCENE_FANOUT children.
//   tree   = heap layout, root 0, children of j at j F + 1 .. j F + F, leaves at the last level, padded to a power of F with EMPTY boxes
//            (lo > hi).  The walk keeps ONE index and no stack: descend to j F + 1; else, while j is a last child (j % F == 0) go up to
//            (j - 1) / F, then j + 1.  That is a preorder walk which names every node at most once, so the trip count of the loop is
//            bounded by the node count the HOST computed from the validated header -- whatever the boxes hold.
//   query  = one lane per ray / per point.  ray_triangle and closest_triangle are the whole of AC14's arithmetic; the leaf test and the
//            `brute` form (every triangle in ascending global index) call the same two functions, so the hierarchy can only decide
//            WHICH triangles are tested.  A node is skipped only when the contract's pruning clauses allow it.  The closest-point
//            kernel first descends once by the nearest child to have a bound before the walk starts (it decides no result).
//   pairs  = AC15: one lane per query triangle walks the same tree with the visit "boxes overlap" and runs tri_tri in
//            the leaves; count, scan, emit, one sort.
#include "kpx_compact.h"
#include "kpx_morton.h"

#include <math.h>

namespace kpx {
namespace {

constexpr int kLeaf = KPX_RAYSCENE_LEAF, kFan = KPX_RAYSCENE_FANOUT;
constexpr unsigned long long kRaySceneMagic = 0x31454e4353595252ull;      // "RRYSCNE1"
constexpr int64_t kRaySceneMaxTriangles = (int64_t)1 << 28;               // node indices stay below 2^31
constexpr int kRayThreads = 64;

struct RaySceneHeader {
    unsigned long long magic;
    int64_t nt;
    unsigned long long bytes;          // kpx_rayscene_bytes(nt)
    int64_t nodes, first_leaf;
};
struct RaySceneLayout { size_t boxes, corners, ids, bytes; int64_t nodes, first_leaf, leaves; };
static inline RaySceneLayout rayscene_layout(int64_t nt)
{
    const int64_t t = nt > 0 ? nt : 0, used = t > 0 ? cdiv(t, kLeaf) : 1;
    RaySceneLayout l;
    l.leaves = 1;
    l.first_leaf = 0;
    while (l.leaves < used) { l.first_leaf += l.leaves; l.leaves *= kFan; }
    l.nodes = l.first_leaf + l.leaves;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t tt = (size_t)(t > 0 ? t : 1);
    l.boxes = up(sizeof(RaySceneHeader));
    l.corners = l.boxes + up((size_t)l.nodes * 6 * sizeof(double));
    l.ids = l.corners + up(tt * 9 * sizeof(float));
    l.bytes = l.ids + up(tt * 4 * sizeof(int32_t));
    return l;
}
// ids: [position][4] = global index g of the triangle stored there, its geometry, its index inside the geometry, and -- indexed by g
// instead of the position -- where triangle g is stored (the brute form's order)
struct RaySceneView {
    const double *boxes;
    const float *corners;
    const int32_t *ids;
    int64_t nt, nodes, first_leaf;
};

// ---- AC14 -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const double a[3], const double b[3], double c[3])
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
// the box of a triangle: min / max of its corners, widened by 2^-20 of the largest coordinate magnitude
__device__ __forceinline__ void triangle_box(const float *__restrict__ c, double lo[3], double hi[3])
{
    double m = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = (double)fminf(c[k], fminf(c[3 + k], c[6 + k]));
        hi[k] = (double)fmaxf(c[k], fmaxf(c[3 + k], c[6 + k]));
        m = fmax(m, fmax(fabs(lo[k]), fabs(hi[k])));
    }
    const double r = m * 0x1p-20;
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = lo[k] - r; hi[k] = hi[k] + r; }
}
struct Ray {
    double o[3], d[3], inv[3];         // inv[k] = 1 / d[k] where d[k] != 0
};
// the slab test: the ray meets the box on [tn, tf]
__device__ __forceinline__ bool ray_box(const Ray &r, const double lo[3], const double hi[3], double *tn_out, double *tf_out)
{
    double tn = 0.0, tf = INFINITY;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (r.d[k] == 0.0) {
            ok = ok && lo[k] <= r.o[k] && r.o[k] <= hi[k];
        } else {
            const double a = (lo[k] - r.o[k]) * r.inv[k], b = (hi[k] - r.o[k]) * r.inv[k];
            const double mn = a < b ? a : b, mx = a < b ? b : a;
            tn = tn > mn ? tn : mn;
            tf = tf < mx ? tf : mx;
        }
    }
    *tn_out = tn;
    *tf_out = tf;
    return ok && tn <= tf;
}
// Moeller-Trumbore with the contract's box clause; c: the nine corner coordinates
__device__ __forceinline__ bool ray_triangle(const Ray &r, const float *__restrict__ c, double *t_out, double *u_out, double *v_out)
{
    double e1[3], e2[3], s[3], p[3], q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double v0 = (double)c[k];
        e1[k] = (double)c[3 + k] - v0;
        e2[k] = (double)c[6 + k] - v0;
        s[k] = r.o[k] - v0;
    }
    cross3(r.d, e2, p);
    const double det = dot3(e1, p);
    if (det == 0.0) return false;
    const double inv = 1.0 / det;
    const double u = dot3(s, p) * inv;
    cross3(s, e1, q);
    const double v = dot3(r.d, q) * inv;
    const double t = dot3(e2, q) * inv;
    if (!(u >= 0.0 && v >= 0.0 && u + v <= 1.0)) return false;
    double lo[3], hi[3], tn, tf;
    triangle_box(c, lo, hi);
    if (!ray_box(r, lo, hi, &tn, &tf)) return false;
    if (!(tn <= t && t <= tf)) return false;
    *t_out = t; *u_out = u; *v_out = v;
    return true;
}
// Ericson's closest point of a triangle to q, and D = max(AC3 d2(q, closest), gap2 of the triangle's box); D may be NaN
__device__ __forceinline__ double closest_triangle(const double q[3], const float *__restrict__ cn, double cp[3])
{
    double a[3], b[3], c[3], ab[3], ac[3], qa[3], qb[3], qc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[k] = (double)cn[k]; b[k] = (double)cn[3 + k]; c[k] = (double)cn[6 + k];
        ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k];
        qa[k] = q[k] - a[k]; qb[k] = q[k] - b[k]; qc[k] = q[k] - c[k];
    }
    const double d1 = dot3(ab, qa), d2 = dot3(ac, qa), d3 = dot3(ab, qb), d4 = dot3(ac, qb), d5 = dot3(ab, qc), d6 = dot3(ac, qc);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0.0 && d2 <= 0.0) {
        cp[0] = a[0]; cp[1] = a[1]; cp[2] = a[2];
    } else if (d3 >= 0.0 && d4 <= d3) {
        cp[0] = b[0]; cp[1] = b[1]; cp[2] = b[2];
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double w = d1 / (d1 - d3);
#pragma unroll
        for (int k = 0; k < 3; ++k) cp[k] = a[k] + w * ab[k];
    } else if (d6 >= 0.0 && d5 <= d6) {
        cp[0] = c[0]; cp[1] = c[1]; cp[2] = c[2];
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double w = d2 / (d2 - d6);
#pragma unroll
        for (int k = 0; k < 3; ++k) cp[k] = a[k] + w * ac[k];
    } else if (va <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) {
        const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
#pragma unroll
        for (int k = 0; k < 3; ++k) cp[k] = b[k] + w * (c[k] - b[k]);
    } else {
        const double w = 1.0 / ((va + vb) + vc), wb = vb * w, wc = vc * w;
#pragma unroll
        for (int k = 0; k < 3; ++k) cp[k] = (a[k] + ab[k] * wb) + ac[k] * wc;
    }
    const double dx = q[0] - cp[0], dy = q[1] - cp[1], dz = q[2] - cp[2];
    const double dd = fma(dz, dz, fma(dy, dy, dx * dx));
    double lo[3], hi[3];
    triangle_box(cn, lo, hi);
    const double gap = pt_gap2(q[0], q[1], q[2], lo, hi);
    return dd != dd ? dd : (dd > gap ? dd : gap);
}

// ---- the walk ---------------------------------------------------------------------------------------------------------------------------
// visit(j) -> whether to look inside node j; leaf(l) tests the triangles of leaf l.  Preorder over the heap: at most v.nodes trips.
template <class Visit, class Leaf>
__device__ __forceinline__ void walk(const RaySceneView &v, Visit visit, Leaf leaf)
{
    uint32_t j = 0;
    const uint32_t nodes = (uint32_t)v.nodes, first_leaf = (uint32_t)v.first_leaf;
    for (uint32_t trip = 0; trip < nodes && j < nodes; ++trip) {
        const double *bx = v.boxes + 6 * (size_t)j;
        double lo[3] = { bx[0], bx[1], bx[2] }, hi[3] = { bx[3], bx[4], bx[5] };
        if (lo[0] <= hi[0] && visit(lo, hi)) {                      // (lo > hi: a padding node, it holds no triangle)
            if (j < first_leaf) { j = j * kFan + 1; continue; }
            if (leaf(j - first_leaf)) return;
        }
        while (j != 0 && j % kFan == 0) j = (j - 1) / kFan;         // j strictly decreases
        if (j == 0) return;
        ++j;
    }
}

template <int MODE, bool BRUTE>
__global__ __launch_bounds__(kRayThreads) void ray_kernel(RaySceneView v, const float *__restrict__ rays, int64_t m, double tnear, double tfar,
                                                          double *__restrict__ out_t64, float *__restrict__ out_t, float *__restrict__ out_uv,
                                                          float *__restrict__ out_nrm, int32_t *__restrict__ out_geom, int32_t *__restrict__ out_prim,
                                                          int32_t *__restrict__ out_count)
{
    const int64_t i = (int64_t)blockIdx.x * kRayThreads + threadIdx.x;
    if (i >= m) return;
    Ray r;
    bool finite = true, zero = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.o[k] = (double)rays[6 * i + k];
        r.d[k] = (double)rays[6 * i + 3 + k];
        r.inv[k] = 1.0 / r.d[k];
        finite = finite && isfinite(r.o[k]) && isfinite(r.d[k]);
        zero = zero && r.d[k] == 0.0;
    }
    double bt = INFINITY, bu = 0.0, bv = 0.0;
    int64_t bpos = -1;
    int32_t bg = INT32_MAX, count = 0;
    // -> true: nothing more can change the result
    auto test = [&](int64_t pos) {
        double t, u, w;
        if (!ray_triangle(r, v.corners + 9 * pos, &t, &u, &w)) return false;
        if (MODE == KPX_RAY_COUNT) { ++count; return false; }
        if (MODE == KPX_RAY_OCCLUDED) {
            if (tnear <= t && t <= tfar) { count = 1; return true; }
            return false;
        }
        const int32_t g = v.ids[4 * pos];
        if (t < bt || (t == bt && g < bg)) { bt = t; bu = u; bv = w; bg = g; bpos = pos; }
        return false;
    };
    if (finite && !zero) {
        if (BRUTE) {
            for (int64_t g = 0; g < v.nt; ++g) {
                const int64_t pos = v.ids[4 * g + 3];
                if ((uint64_t)pos < (uint64_t)v.nt && test(pos)) break;
            }
        } else {
            walk(v,
                 [&](const double lo[3], const double hi[3]) {
                     double tn, tf;
                     if (!ray_box(r, lo, hi, &tn, &tf)) return false;
                     return MODE != KPX_RAY_CAST || !(tn > bt);
                 },
                 [&](uint32_t leaf) {
                     const int64_t p0 = (int64_t)leaf * kLeaf, p1 = p0 + kLeaf < v.nt ? p0 + kLeaf : v.nt;
                     for (int64_t pos = p0; pos < p1; ++pos)
                         if (test(pos)) return true;
                     return false;
                 });
        }
    }
    if (MODE != KPX_RAY_CAST) {
        out_count[i] = count;
        return;
    }
    float n[3] = { 0.0f, 0.0f, 0.0f };
    if (bpos >= 0) {                                                // AC12's normalised normal of the winner
        const float *c = v.corners + 9 * bpos;
        double e1[3], e2[3], nn[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { e1[k] = (double)c[3 + k] - (double)c[k]; e2[k] = (double)c[6 + k] - (double)c[k]; }
        cross3(e1, e2, nn);
        const double len = sqrt(dot3(nn, nn));
        if (len == 0.0) { n[2] = 1.0f; }
        else { n[0] = (float)(nn[0] / len); n[1] = (float)(nn[1] / len); n[2] = (float)(nn[2] / len); }
    }
    out_t64[i] = bt;
    out_t[i] = (float)bt;
    out_uv[2 * i] = (float)bu; out_uv[2 * i + 1] = (float)bv;
    out_nrm[3 * i] = n[0]; out_nrm[3 * i + 1] = n[1]; out_nrm[3 * i + 2] = n[2];
    out_geom[i] = bpos >= 0 ? v.ids[4 * bpos + 1] : -1;
    out_prim[i] = bpos >= 0 ? v.ids[4 * bpos + 2] : -1;
}

template <bool BRUTE>
__global__ __launch_bounds__(kRayThreads) void closest_kernel(RaySceneView v, const float *__restrict__ queries, int64_t m, double *__restrict__ out_d2,
                                                              float *__restrict__ out_pts, float *__restrict__ out_dist, int32_t *__restrict__ out_geom,
                                                              int32_t *__restrict__ out_prim)
{
    const int64_t i = (int64_t)blockIdx.x * kRayThreads + threadIdx.x;
    if (i >= m) return;
    const double q[3] = { (double)queries[3 * i], (double)queries[3 * i + 1], (double)queries[3 * i + 2] };
    double bd = NAN, bp[3] = { NAN, NAN, NAN };
    int64_t bpos = -1;
    int32_t bg = INT32_MAX;
    auto test = [&](int64_t pos) {
        double cp[3];
        const double d = closest_triangle(q, v.corners + 9 * pos, cp);
        const int32_t g = v.ids[4 * pos];
        if (d == d && (bpos < 0 || d < bd || (d == bd && g < bg))) { bd = d; bg = g; bpos = pos; bp[0] = cp[0]; bp[1] = cp[1]; bp[2] = cp[2]; }
    };
    if (isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2])) {       // (a query with a non-finite coordinate has no closest point)
        if (BRUTE) {
            for (int64_t g = 0; g < v.nt; ++g) {
                const int64_t pos = v.ids[4 * g + 3];
                if ((uint64_t)pos < (uint64_t)v.nt) test(pos);
            }
        } else {
            auto leaf_test = [&](uint32_t leaf) {
                const int64_t p0 = (int64_t)leaf * kLeaf, p1 = p0 + kLeaf < v.nt ? p0 + kLeaf : v.nt;
                for (int64_t pos = p0; pos < p1; ++pos) test(pos);
                return false;
            };
            // A first bound, so that the walk prunes from its first node on: down the tree by the nearest non-empty child, and the
            // triangles of the leaf that ends in.  The walk meets them again (an equal (D, g) changes nothing), so this decides no
            // result.  j grows on every trip (j F + 1 > j) and the loop ends at the first leaf index: at most 32 trips.
            uint32_t j = 0;
            const uint32_t first_leaf = (uint32_t)v.first_leaf;
            for (int trip = 0; trip < 32 && j < first_leaf; ++trip) {
                uint32_t next = j * kFan + 1;
                double near = INFINITY, near_mid = INFINITY;         // smallest gap2; among equal ones (0 where boxes overlap) the nearest centre
#pragma unroll
                for (int c = 0; c < kFan; ++c) {
                    const double *bx = v.boxes + 6 * (size_t)(j * kFan + 1 + c);
                    const double lo[3] = { bx[0], bx[1], bx[2] }, hi[3] = { bx[3], bx[4], bx[5] };
                    const double g2 = pt_gap2(q[0], q[1], q[2], lo, hi);
                    const double mx = 0.5 * (lo[0] + hi[0]) - q[0], my = 0.5 * (lo[1] + hi[1]) - q[1], mz = 0.5 * (lo[2] + hi[2]) - q[2];
                    const double mid = mx * mx + my * my + mz * mz;
                    if (lo[0] <= hi[0] && (g2 < near || (g2 == near && mid < near_mid))) { near = g2; near_mid = mid; next = j * kFan + 1 + c; }
                }
                j = next;
            }
            if (j >= first_leaf && j < (uint32_t)v.nodes) leaf_test(j - first_leaf);
            walk(v, [&](const double lo[3], const double hi[3]) { return bpos < 0 || !(pt_gap2(q[0], q[1], q[2], lo, hi) > bd); }, leaf_test);
        }
    }
    out_d2[i] = bd;
    out_dist[i] = (float)sqrt(bd);
    out_pts[3 * i] = (float)bp[0]; out_pts[3 * i + 1] = (float)bp[1]; out_pts[3 * i + 2] = (float)bp[2];
    out_geom[i] = bpos >= 0 ? v.ids[4 * bpos + 1] : -1;
    out_prim[i] = bpos >= 0 ? v.ids[4 * bpos + 2] : -1;
}

// ---- build ----------------------------------------------------------------------------------------------------------------------------
// the nine corner coordinates of triangle g; a triangle with an index outside [0, nv) reads nothing and lies at the origin (callers
// reject such meshes first)
__device__ __forceinline__ void load_corners(const float *__restrict__ vert, int64_t nv, const int32_t *__restrict__ tri, int64_t g, float c[9])
{
    const int32_t i0 = tri[3 * g], i1 = tri[3 * g + 1], i2 = tri[3 * g + 2];
    const bool ok = i0 >= 0 && i1 >= 0 && i2 >= 0 && i0 < nv && i1 < nv && i2 < nv;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c[k] = ok ? vert[3 * (int64_t)i0 + k] : 0.0f;
        c[3 + k] = ok ? vert[3 * (int64_t)i1 + k] : 0.0f;
        c[6 + k] = ok ? vert[3 * (int64_t)i2 + k] : 0.0f;
    }
}
__global__ __launch_bounds__(256) void ray_centroid_kernel(const float *__restrict__ vert, int64_t nv, const int32_t *__restrict__ tri, int64_t nt,
                                                           float *__restrict__ cen)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    float c[9];
    load_corners(vert, nv, tri, t, c);
#pragma unroll
    for (int k = 0; k < 3; ++k) cen[3 * t + k] = (float)((((double)c[k] + (double)c[3 + k]) + (double)c[6 + k]) / 3.0);
}
// one thread per leaf of the padded last level: gathers its triangles into the scene and fits its box
__global__ __launch_bounds__(256) void ray_leaf_kernel(char *__restrict__ scene, RaySceneLayout l, int64_t nt, const float *__restrict__ vert,
                                                       int64_t nv, const int32_t *__restrict__ tri, const int32_t *__restrict__ tri_ids, const int32_t *__restrict__ perm)
{
    const int64_t leaf = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (leaf == 0) {
        RaySceneHeader h;
        h.magic = kRaySceneMagic; h.nt = nt; h.bytes = l.bytes; h.nodes = l.nodes; h.first_leaf = l.first_leaf;
        *reinterpret_cast<RaySceneHeader *>(scene) = h;
    }
    if (leaf >= l.leaves) return;
    double *box = reinterpret_cast<double *>(scene + l.boxes) + 6 * (l.first_leaf + leaf);
    float *corners = reinterpret_cast<float *>(scene + l.corners);
    int32_t *ids = reinterpret_cast<int32_t *>(scene + l.ids);
    double lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    const int64_t p0 = leaf * kLeaf, p1 = p0 + kLeaf < nt ? p0 + kLeaf : nt;
    for (int64_t pos = p0; pos < p1; ++pos) {
        const int64_t g = perm[pos];
        float c[9];
        load_corners(vert, nv, tri, g, c);
#pragma unroll
        for (int k = 0; k < 9; ++k) corners[9 * pos + k] = c[k];
        ids[4 * pos] = (int32_t)g;
        ids[4 * pos + 1] = tri_ids ? tri_ids[2 * g] : 0;
        ids[4 * pos + 2] = tri_ids ? tri_ids[2 * g + 1] : (int32_t)g;
        ids[4 * g + 3] = (int32_t)pos;
        double tlo[3], thi[3];
        triangle_box(c, tlo, thi);
#pragma unroll
        for (int k = 0; k < 3; ++k) { lo[k] = fmin(lo[k], tlo[k]); hi[k] = fmax(hi[k], thi[k]); }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { box[k] = lo[k]; box[3 + k] = hi[k]; }
}
// the `count` nodes from `first` on: each the union of its kFan children (an empty child changes nothing)
__global__ __launch_bounds__(256) void ray_level_kernel(double *__restrict__ boxes, int64_t first, int64_t count)
{
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= count) return;
    const int64_t j = first + n;
    double lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
#pragma unroll
    for (int c = 0; c < kFan; ++c) {
        const double *cb = boxes + 6 * (j * kFan + 1 + c);
#pragma unroll
        for (int k = 0; k < 3; ++k) { lo[k] = fmin(lo[k], cb[k]); hi[k] = fmax(hi[k], cb[3 + k]); }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { boxes[6 * j + k] = lo[k]; boxes[6 * j + 3 + k] = hi[k]; }
}

struct RayBuildScratch {
    float *centroids;
    int32_t *perm;
    SortScratch sort;
};
void ray_build_carve(Arena &a, int64_t nt, RayBuildScratch *s)
{
    const size_t t = (size_t)(nt > 0 ? nt : 1);
    s->centroids = a.get<float>(3 * t);
    s->perm = a.get<int32_t>(t);
    sort_carve(a, (int64_t)t, &s->sort);
}

// The header comes back to the host (one small copy and a stream synchronisation per call): every bound the kernels loop to is
// computed here from a triangle count that fits the buffer, never read from the buffer by a kernel.
int ray_open(const void *scene, size_t scene_bytes, hipStream_t st, RaySceneView *v)
{
    RaySceneHeader h;
    KPX_HIP(hipMemcpyAsync(&h, scene, sizeof(h), hipMemcpyDeviceToHost, st));
    KPX_HIP(hipStreamSynchronize(st));
    KPX_REQUIRE(h.magic == kRaySceneMagic && h.nt >= 0 && h.nt <= kRaySceneMaxTriangles, "kpx_rayscene: the buffer holds no scene (kpx_rayscene_build)");
    const RaySceneLayout l = rayscene_layout(h.nt);
    KPX_REQUIRE(h.bytes == l.bytes && h.nodes == l.nodes && h.first_leaf == l.first_leaf, "kpx_rayscene: the buffer holds no scene (kpx_rayscene_build)");
    KPX_REQUIRE(scene_bytes >= l.bytes, "kpx_rayscene: scene_bytes %zu is smaller than the %zu bytes of a scene of %lld triangles", scene_bytes, l.bytes,
                (long long)h.nt);
    const char *base = (const char *)scene;
    v->boxes = reinterpret_cast<const double *>(base + l.boxes);
    v->corners = reinterpret_cast<const float *>(base + l.corners);
    v->ids = reinterpret_cast<const int32_t *>(base + l.ids);
    v->nt = h.nt; v->nodes = l.nodes; v->first_leaf = l.first_leaf;
    return KPX_OK;
}
#define KPX_RAYSCENE_ARGS(who)                                                                                                               \
    KPX_REQUIRE(scene, who ": null scene");                                                                                                  \
    KPX_REQUIRE(scene_bytes >= rayscene_layout(0).bytes, who ": scene_bytes %zu is smaller than the %zu bytes of a scene of 0 triangles",    \
                scene_bytes, rayscene_layout(0).bytes);                                                                                      \
    KPX_REQUIRE(m >= 0 && m < ((int64_t)1 << 31), who ": bad number of queries")

template <int MODE>
void ray_launch(bool brute, unsigned nb, hipStream_t st, const RaySceneView &v, const float *rays, int64_t m, double tnear, double tfar, double *t64,
                float *t, float *uv, float *nrm, int32_t *geom, int32_t *prim, int32_t *count)
{
    if (brute) hipLaunchKernelGGL((ray_kernel<MODE, true>), dim3(nb), dim3(kRayThreads), 0, st, v, rays, m, tnear, tfar, t64, t, uv, nrm, geom, prim, count);
    else hipLaunchKernelGGL((ray_kernel<MODE, false>), dim3(nb), dim3(kRayThreads), 0, st, v, rays, m, tnear, tfar, t64, t, uv, nrm, geom, prim, count);
}

// ---- AC15: triangle against triangle ------------------------------------------------------------------------------------------------------
// Moeller's interval-overlap test, division-free, with the coplanar fallback; tests/mesh_checks_ref.py is the pinned statement and
// this follows it operation for operation.  Everything per lane is a scalar or a statically indexed array (the projection axes are
// selects), so nothing lives in scratch memory.
constexpr double kTriTriEpsilon = 1e-6;          // absolute: plane distances below it count as 0, whatever the mesh's scale

__device__ __forceinline__ double pick3(int k, double x, double y, double z) { return k == 0 ? x : (k == 1 ? y : z); }
// -> false: the triangle lies in the other's plane
__device__ __forceinline__ bool tri_intervals(double vv0, double vv1, double vv2, double d0, double d1, double d2, double d0d1, double d0d2, double *A, double *B,
                                              double *C, double *X0, double *X1)
{
    if (d0d1 > 0.0) { *A = vv2; *B = (vv0 - vv2) * d2; *C = (vv1 - vv2) * d2; *X0 = d2 - d0; *X1 = d2 - d1; }
    else if (d0d2 > 0.0) { *A = vv1; *B = (vv0 - vv1) * d1; *C = (vv2 - vv1) * d1; *X0 = d1 - d0; *X1 = d1 - d2; }
    else if (d1 * d2 > 0.0 || d0 != 0.0) { *A = vv0; *B = (vv1 - vv0) * d0; *C = (vv2 - vv0) * d0; *X0 = d0 - d1; *X1 = d0 - d2; }
    else if (d1 != 0.0) { *A = vv1; *B = (vv0 - vv1) * d1; *C = (vv2 - vv1) * d1; *X0 = d1 - d0; *X1 = d1 - d2; }
    else if (d2 != 0.0) { *A = vv2; *B = (vv0 - vv2) * d2; *C = (vv1 - vv2) * d2; *X0 = d2 - d0; *X1 = d2 - d1; }
    else return false;
    return true;
}
// closed test of the 2D edge from (vx, vy) along (ax, ay) against the edge u0 u1; parallel edges report nothing
__device__ __forceinline__ bool edge_edge(double ax, double ay, double vx, double vy, double u0x, double u0y, double u1x, double u1y)
{
    const double bx = u0x - u1x, by = u0y - u1y, cx = vx - u0x, cy = vy - u0y;
    const double f = ay * bx - ax * by, d = by * cx - bx * cy;
    if ((f > 0.0 && d >= 0.0 && d <= f) || (f < 0.0 && d <= 0.0 && d >= f)) {
        const double e = ax * cy - ay * cx;
        return f > 0.0 ? (e >= 0.0 && e <= f) : (e <= 0.0 && e >= f);
    }
    return false;
}
// (px, py) strictly inside the 2D triangle u
__device__ __forceinline__ bool point_in_tri(double px, double py, const double ux[3], const double uy[3])
{
    double a = uy[1] - uy[0], b = -(ux[1] - ux[0]), c = -a * ux[0] - b * uy[0];
    const double d0 = (a * px + b * py) + c;
    a = uy[2] - uy[1]; b = -(ux[2] - ux[1]); c = -a * ux[1] - b * uy[1];
    const double d1 = (a * px + b * py) + c;
    a = uy[0] - uy[2]; b = -(ux[0] - ux[2]); c = -a * ux[2] - b * uy[2];
    const double d2 = (a * px + b * py) + c;
    return d0 * d1 > 0.0 && d0 * d2 > 0.0;
}
__device__ __forceinline__ bool tri_coplanar(const double n[3], const double v[3][3], const double u[3][3])
{
    const double a0 = fabs(n[0]), a1 = fabs(n[1]), a2 = fabs(n[2]);
    // the axes kept: (1, 2) when x is dropped, (0, 1) when z is, else (0, 2)
    const bool drop_x = a0 > a1 && a0 > a2, drop_z = a0 > a1 ? !(a0 > a2) : a2 > a1;
    double px[3], py[3], qx[3], qy[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        px[k] = drop_x ? v[k][1] : v[k][0]; py[k] = drop_z ? v[k][1] : v[k][2];
        qx[k] = drop_x ? u[k][1] : u[k][0]; qy[k] = drop_z ? u[k][1] : u[k][2];
    }
    bool hit = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int e = (k + 1) % 3;
        const double ax = px[e] - px[k], ay = py[e] - py[k];
        hit = hit || edge_edge(ax, ay, px[k], py[k], qx[0], qy[0], qx[1], qy[1]) || edge_edge(ax, ay, px[k], py[k], qx[1], qy[1], qx[2], qy[2]) ||
              edge_edge(ax, ay, px[k], py[k], qx[2], qy[2], qx[0], qy[0]);
    }
    return hit || point_in_tri(px[0], py[0], qx, qy) || point_in_tri(qx[0], qy[0], px, py);
}
// whether triangle v (the query; in a self search the lower index) meets triangle u; nine corner coordinates each
__device__ __forceinline__ bool tri_tri(const float *__restrict__ cv, const float *__restrict__ cu)
{
    double v[3][3], u[3][3], e1[3], e2[3], n1[3], n2[3], dd[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        v[0][k] = (double)cv[k]; v[1][k] = (double)cv[3 + k]; v[2][k] = (double)cv[6 + k];
        u[0][k] = (double)cu[k]; u[1][k] = (double)cu[3 + k]; u[2][k] = (double)cu[6 + k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { e1[k] = v[1][k] - v[0][k]; e2[k] = v[2][k] - v[0][k]; }
    cross3(e1, e2, n1);
    const double d1 = -dot3(n1, v[0]);
    double du0 = dot3(n1, u[0]) + d1, du1 = dot3(n1, u[1]) + d1, du2 = dot3(n1, u[2]) + d1;
    du0 = fabs(du0) < kTriTriEpsilon ? 0.0 : du0;
    du1 = fabs(du1) < kTriTriEpsilon ? 0.0 : du1;
    du2 = fabs(du2) < kTriTriEpsilon ? 0.0 : du2;
    const double du0du1 = du0 * du1, du0du2 = du0 * du2;
    if (du0du1 > 0.0 && du0du2 > 0.0) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) { e1[k] = u[1][k] - u[0][k]; e2[k] = u[2][k] - u[0][k]; }
    cross3(e1, e2, n2);
    const double d2 = -dot3(n2, u[0]);
    double dv0 = dot3(n2, v[0]) + d2, dv1 = dot3(n2, v[1]) + d2, dv2 = dot3(n2, v[2]) + d2;
    dv0 = fabs(dv0) < kTriTriEpsilon ? 0.0 : dv0;
    dv1 = fabs(dv1) < kTriTriEpsilon ? 0.0 : dv1;
    dv2 = fabs(dv2) < kTriTriEpsilon ? 0.0 : dv2;
    const double dv0dv1 = dv0 * dv1, dv0dv2 = dv0 * dv2;
    if (dv0dv1 > 0.0 && dv0dv2 > 0.0) return false;
    cross3(n1, n2, dd);
    int index = 0;
    double big = fabs(dd[0]);
    if (fabs(dd[1]) > big) { index = 1; big = fabs(dd[1]); }
    if (fabs(dd[2]) > big) index = 2;
    double a, b, c, x0, x1, d, e, f, y0, y1;
    if (!tri_intervals(pick3(index, v[0][0], v[0][1], v[0][2]), pick3(index, v[1][0], v[1][1], v[1][2]), pick3(index, v[2][0], v[2][1], v[2][2]), dv0, dv1, dv2, dv0dv1, dv0dv2, &a, &b, &c, &x0, &x1))
        return tri_coplanar(n1, v, u);
    if (!tri_intervals(pick3(index, u[0][0], u[0][1], u[0][2]), pick3(index, u[1][0], u[1][1], u[1][2]), pick3(index, u[2][0], u[2][1], u[2][2]), du0, du1, du2, du0du1, du0du2, &d, &e, &f, &y0, &y1))
        return tri_coplanar(n1, v, u);
    const double xx = x0 * x1, yy = y0 * y1, xxyy = xx * yy;
    double tmp = a * xxyy;
    const double p0 = tmp + (b * x1) * yy, p1 = tmp + (c * x0) * yy;
    tmp = d * xxyy;
    const double q0 = tmp + (e * xx) * y1, q1 = tmp + (f * xx) * y0;
    const double lo1 = p0 > p1 ? p1 : p0, hi1 = p0 > p1 ? p0 : p1, lo2 = q0 > q1 ? q1 : q0, hi2 = q0 > q1 ? q0 : q1;
    return !(hi1 < lo2 || hi2 < lo1);
}
// the exact box of a triangle (no padding) and the closed overlap of two boxes
__device__ __forceinline__ void exact_box(const float *__restrict__ c, double lo[3], double hi[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = (double)fminf(c[k], fminf(c[3 + k], c[6 + k]));
        hi[k] = (double)fmaxf(c[k], fmaxf(c[3 + k], c[6 + k]));
    }
}
__device__ __forceinline__ bool boxes_meet(const double alo[3], const double ahi[3], const double blo[3], const double bhi[3])
{
    return alo[0] <= bhi[0] && blo[0] <= ahi[0] && alo[1] <= bhi[1] && blo[1] <= ahi[1] && alo[2] <= bhi[2] && blo[2] <= ahi[2];
}

// One lane per query triangle i of (q_vert, q_tri).  A scene triangle g is its partner when the exact boxes overlap and tri_tri(i, g)
// says so; SELF: the queries are the triangles the scene was built from, only g > i is looked at and a pair that shares a vertex
// index is skipped (the index triples are q_tri's, found through the scene's stored global index).  A node is entered only when its
// box -- which contains the padded, hence the exact, boxes of its triangles -- overlaps the query's exact box: nothing else prunes.
//   kPairCount: counts[i] = the number of partners      kPairEmit: keys[offsets[i] + n] = i << 32 | g, in the walk's order
//   kPairAny:   *flag = 1 when some lane has a partner; such a lane leaves its walk at once
enum { kPairCount, kPairEmit, kPairAny };
template <int PASS, bool SELF, bool BRUTE>
__global__ __launch_bounds__(kRayThreads) void tri_pairs_kernel(RaySceneView v, const float *__restrict__ q_vert, int64_t q_nv, const int32_t *__restrict__ q_tri,
                                                                int64_t m, int64_t *__restrict__ counts, uint64_t *__restrict__ keys, int64_t total,
                                                                int32_t *__restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * kRayThreads + threadIdx.x;
    if (i >= m) return;
    float qc[9];
    load_corners(q_vert, q_nv, q_tri, i, qc);
    const int32_t q0 = q_tri[3 * i], q1 = q_tri[3 * i + 1], q2 = q_tri[3 * i + 2];
    double qlo[3], qhi[3];
    exact_box(qc, qlo, qhi);
    int64_t count = 0;
    const int64_t base = PASS == kPairEmit ? counts[i] : 0, room = PASS == kPairEmit ? counts[i + 1] - counts[i] : 0;
    // -> true: this lane is done
    auto test = [&](int64_t pos) {
        const int32_t g = v.ids[4 * pos];
        if (SELF) {
            if ((int64_t)g <= i || (int64_t)g >= m) return false;
            const int32_t g0 = q_tri[3 * (int64_t)g], g1 = q_tri[3 * (int64_t)g + 1], g2 = q_tri[3 * (int64_t)g + 2];
            if (g0 == q0 || g0 == q1 || g0 == q2 || g1 == q0 || g1 == q1 || g1 == q2 || g2 == q0 || g2 == q1 || g2 == q2) return false;
        }
        const float *c = v.corners + 9 * pos;
        double lo[3], hi[3];
        exact_box(c, lo, hi);
        if (!boxes_meet(qlo, qhi, lo, hi) || !tri_tri(qc, c)) return false;
        if (PASS == kPairAny) { *flag = 1; return true; }
        if (PASS == kPairEmit && count < room && base + count < total) keys[base + count] = (uint64_t)i << 32 | (uint64_t)(uint32_t)g;
        ++count;
        return false;
    };
    if (BRUTE) {
        for (int64_t g = 0; g < v.nt; ++g) {
            const int64_t pos = v.ids[4 * g + 3];
            if ((uint64_t)pos < (uint64_t)v.nt && test(pos)) break;
        }
    } else {
        walk(v, [&](const double lo[3], const double hi[3]) { return boxes_meet(qlo, qhi, lo, hi); },
             [&](uint32_t leaf) {
                 const int64_t p0 = (int64_t)leaf * kLeaf, p1 = p0 + kLeaf < v.nt ? p0 + kLeaf : v.nt;
                 for (int64_t pos = p0; pos < p1; ++pos)
                     if (test(pos)) return true;
                 return false;
             });
    }
    if (PASS == kPairCount) counts[i] = count;
}
template <int PASS>
void pairs_launch(bool self, bool brute, hipStream_t st, const RaySceneView &v, const float *q_vert, int64_t q_nv, const int32_t *q_tri, int64_t m, int64_t *counts,
                  uint64_t *keys, int64_t total, int32_t *flag)
{
    const dim3 grid((unsigned)cdiv(m, kRayThreads)), block(kRayThreads);
    if (self && brute) hipLaunchKernelGGL((tri_pairs_kernel<PASS, true, true>), grid, block, 0, st, v, q_vert, q_nv, q_tri, m, counts, keys, total, flag);
    else if (self) hipLaunchKernelGGL((tri_pairs_kernel<PASS, true, false>), grid, block, 0, st, v, q_vert, q_nv, q_tri, m, counts, keys, total, flag);
    else if (brute) hipLaunchKernelGGL((tri_pairs_kernel<PASS, false, true>), grid, block, 0, st, v, q_vert, q_nv, q_tri, m, counts, keys, total, flag);
    else hipLaunchKernelGGL((tri_pairs_kernel<PASS, false, false>), grid, block, 0, st, v, q_vert, q_nv, q_tri, m, counts, keys, total, flag);
}
__global__ __launch_bounds__(256) void pair_unpack_kernel(const uint64_t *__restrict__ keys, int64_t n, int32_t *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[2 * i] = (int32_t)(keys[i] >> 32);
    out[2 * i + 1] = (int32_t)(uint32_t)keys[i];
}
constexpr int64_t kPairMax = 2147483647;
int pairs_args(const char *who, const void *scene, size_t scene_bytes, const float *q_vert, int64_t q_nv, const int32_t *q_tri, int64_t m)
{
    KPX_RAYSCENE_ARGS("kpx_rayscene_triangle_pairs");
    KPX_REQUIRE(q_nv >= 0 && q_nv < ((int64_t)1 << 31), "%s: bad number of vertices", who);
    KPX_REQUIRE(m == 0 || (q_vert && q_tri), "%s: null pointer", who);
    return KPX_OK;
}

}  // namespace
}  // namespace kpx

using namespace kpx;

KPX_EXPORT size_t kpx_rayscene_bytes(int64_t n_triangles)
{
    return n_triangles > kRaySceneMaxTriangles ? 0 : rayscene_layout(n_triangles).bytes;
}

KPX_EXPORT size_t kpx_rayscene_workspace_bytes(int64_t n_triangles)
{
    if (n_triangles > kRaySceneMaxTriangles) return 0;
    Arena a(nullptr, 0);
    RayBuildScratch s;
    ray_build_carve(a, n_triangles, &s);
    return a.off;
}

KPX_EXPORT int kpx_rayscene_build(const float *vertices, int64_t n_vertices, const int32_t *triangles, int64_t n_triangles, const int32_t *triangle_ids,
                                  void *scene, size_t scene_bytes, void *ws, size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(n_vertices >= 0 && n_vertices < ((int64_t)1 << 31), "kpx_rayscene_build: bad number of vertices");
    KPX_REQUIRE(n_triangles >= 0 && n_triangles <= kRaySceneMaxTriangles, "kpx_rayscene_build: a scene holds at most 2^28 triangles");
    KPX_REQUIRE(scene, "kpx_rayscene_build: null scene");
    const RaySceneLayout l = rayscene_layout(n_triangles);
    KPX_REQUIRE(scene_bytes >= l.bytes, "kpx_rayscene_build: scene_bytes %zu is smaller than the %zu bytes of a scene of %lld triangles", scene_bytes,
                l.bytes, (long long)n_triangles);
    hipStream_t st = (hipStream_t)stream;
    RayBuildScratch s = {};
    if (n_triangles > 0) {
        KPX_REQUIRE(vertices && triangles && ws, "kpx_rayscene_build: null pointer");
        Arena a(ws, ws_bytes);
        ray_build_carve(a, n_triangles, &s);
        KPX_ARENA_CHECK(a);
        hipLaunchKernelGGL(ray_centroid_kernel, dim3((unsigned)cdiv(n_triangles, 256)), dim3(256), 0, st, vertices, n_vertices, triangles, n_triangles, s.centroids);
        const int rc = morton_order(s.centroids, n_triangles, s.sort, s.perm, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(ray_leaf_kernel, dim3((unsigned)cdiv(l.leaves, 256)), dim3(256), 0, st, (char *)scene, l, n_triangles, vertices, n_vertices, triangles, triangle_ids,
                       (const int32_t *)s.perm);
    double *boxes = reinterpret_cast<double *>((char *)scene + l.boxes);
    for (int64_t count = l.leaves / kFan, first = l.first_leaf; count >= 1; count /= kFan) {
        first -= count;
        hipLaunchKernelGGL(ray_level_kernel, dim3((unsigned)cdiv(count, 256)), dim3(256), 0, st, boxes, first, count);
    }
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT int kpx_rayscene_rays(const void *scene, size_t scene_bytes, const float *rays, int64_t m, int32_t mode, double tnear, double tfar, int32_t brute,
                                 double *out_t, float *out_t_hit, float *out_uvs, float *out_normals, int32_t *out_geometry_ids,
                                 int32_t *out_primitive_ids, int32_t *out_count, void *stream)
{
    KPX_REQUIRE(mode == KPX_RAY_CAST || mode == KPX_RAY_OCCLUDED || mode == KPX_RAY_COUNT, "kpx_rayscene_rays: unknown mode %d", (int)mode);
    KPX_REQUIRE(!(tnear != tnear) && !(tfar != tfar), "kpx_rayscene_rays: tnear / tfar is not a number");
    KPX_RAYSCENE_ARGS("kpx_rayscene_rays");
    if (m == 0) return KPX_OK;
    if (mode == KPX_RAY_CAST) KPX_REQUIRE(rays && out_t && out_t_hit && out_uvs && out_normals && out_geometry_ids && out_primitive_ids, "kpx_rayscene_rays: null pointer");
    else KPX_REQUIRE(rays && out_count, "kpx_rayscene_rays: null pointer");
    hipStream_t st = (hipStream_t)stream;
    RaySceneView v;
    const int rc = ray_open(scene, scene_bytes, st, &v);
    if (rc) return rc;
    const unsigned nb = (unsigned)cdiv(m, kRayThreads);
    if (mode == KPX_RAY_CAST)
        ray_launch<KPX_RAY_CAST>(brute != 0, nb, st, v, rays, m, tnear, tfar, out_t, out_t_hit, out_uvs, out_normals, out_geometry_ids, out_primitive_ids, out_count);
    else if (mode == KPX_RAY_OCCLUDED)
        ray_launch<KPX_RAY_OCCLUDED>(brute != 0, nb, st, v, rays, m, tnear, tfar, out_t, out_t_hit, out_uvs, out_normals, out_geometry_ids, out_primitive_ids, out_count);
    else
        ray_launch<KPX_RAY_COUNT>(brute != 0, nb, st, v, rays, m, tnear, tfar, out_t, out_t_hit, out_uvs, out_normals, out_geometry_ids, out_primitive_ids, out_count);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT int kpx_rayscene_closest(const void *scene, size_t scene_bytes, const float *queries, int64_t m, int32_t brute, double *out_d2, float *out_points,
                                    float *out_distance, int32_t *out_geometry_ids, int32_t *out_primitive_ids, void *stream)
{
    KPX_RAYSCENE_ARGS("kpx_rayscene_closest");
    if (m == 0) return KPX_OK;
    KPX_REQUIRE(queries && out_d2 && out_points && out_distance && out_geometry_ids && out_primitive_ids, "kpx_rayscene_closest: null pointer");
    hipStream_t st = (hipStream_t)stream;
    RaySceneView v;
    const int rc = ray_open(scene, scene_bytes, st, &v);
    if (rc) return rc;
    KPX_REQUIRE(v.nt > 0, "kpx_rayscene_closest: the scene holds no triangle");
    const unsigned nb = (unsigned)cdiv(m, kRayThreads);
    if (brute) hipLaunchKernelGGL(closest_kernel<true>, dim3(nb), dim3(kRayThreads), 0, st, v, queries, m, out_d2, out_points, out_distance, out_geometry_ids, out_primitive_ids);
    else hipLaunchKernelGGL(closest_kernel<false>, dim3(nb), dim3(kRayThreads), 0, st, v, queries, m, out_d2, out_points, out_distance, out_geometry_ids, out_primitive_ids);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT int kpx_rayscene_triangle_pairs_count(const void *scene, size_t scene_bytes, const float *vertices, int64_t n_vertices, const int32_t *triangles,
                                                 int64_t m, int32_t self, int32_t any, int32_t brute, int64_t *out_offsets, int32_t *d_flag, void *stream)
{
    const int rc0 = pairs_args("kpx_rayscene_triangle_pairs_count", scene, scene_bytes, vertices, n_vertices, triangles, m);
    if (rc0) return rc0;
    KPX_REQUIRE(any ? d_flag != nullptr : out_offsets != nullptr, "kpx_rayscene_triangle_pairs_count: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (any) KPX_HIP(hipMemsetAsync(d_flag, 0, sizeof(int32_t), st));
    else KPX_HIP(hipMemsetAsync(out_offsets, 0, (size_t)(m + 1) * sizeof(int64_t), st));
    RaySceneView v;
    const int rc = ray_open(scene, scene_bytes, st, &v);
    if (rc) return rc;
    KPX_REQUIRE(!self || v.nt == m, "kpx_rayscene_triangle_pairs_count: a self search needs the %lld triangles the scene was built from, got %lld",
                (long long)v.nt, (long long)m);
    if (m == 0 || v.nt == 0) return KPX_OK;
    if (any) {
        pairs_launch<kPairAny>(self != 0, brute != 0, st, v, vertices, n_vertices, triangles, m, nullptr, nullptr, 0, d_flag);
    } else {
        pairs_launch<kPairCount>(self != 0, brute != 0, st, v, vertices, n_vertices, triangles, m, out_offsets, nullptr, 0, nullptr);
        scan_i64(out_offsets, m, st);
    }
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT size_t kpx_rayscene_triangle_pairs_workspace_bytes(int64_t n_pairs)
{
    if (n_pairs < 0 || n_pairs > kPairMax) return 0;
    Arena a(nullptr, 0);
    DeviceSort<uint64_t, false> s;
    dsort_carve(a, n_pairs, 64, SortOptions(), &s);
    return a.off;
}

KPX_EXPORT int kpx_rayscene_triangle_pairs_fill(const void *scene, size_t scene_bytes, const float *vertices, int64_t n_vertices, const int32_t *triangles,
                                                int64_t m, int32_t self, int32_t brute, const int64_t *offsets, int64_t n_pairs, int32_t *out_pairs, void *ws,
                                                size_t ws_bytes, void *stream)
{
    const int rc0 = pairs_args("kpx_rayscene_triangle_pairs_fill", scene, scene_bytes, vertices, n_vertices, triangles, m);
    if (rc0) return rc0;
    KPX_REQUIRE(n_pairs >= 0, "kpx_rayscene_triangle_pairs_fill: negative count");
    if (n_pairs > kPairMax) return fail(KPX_ERR_RANGE, "kpx_rayscene_triangle_pairs_fill: %lld pairs: at most 2^31 - 1", (long long)n_pairs);
    if (n_pairs == 0) return KPX_OK;
    KPX_REQUIRE(offsets && out_pairs && ws && m > 0, "kpx_rayscene_triangle_pairs_fill: null pointer");
    hipStream_t st = (hipStream_t)stream;
    RaySceneView v;
    int rc = ray_open(scene, scene_bytes, st, &v);
    if (rc) return rc;
    KPX_REQUIRE(!self || v.nt == m, "kpx_rayscene_triangle_pairs_fill: a self search needs the %lld triangles the scene was built from, got %lld",
                (long long)v.nt, (long long)m);
    Arena a(ws, ws_bytes);
    DeviceSort<uint64_t, false> s;
    dsort_carve(a, n_pairs, 64, SortOptions(), &s);
    KPX_ARENA_CHECK(a);
    // a slot the emit pass does not reach (offsets that are not this search's) sorts last and reads as (-1, -1)
    KPX_HIP(hipMemsetAsync(s.keys_in, 0xff, (size_t)n_pairs * sizeof(uint64_t), st));
    pairs_launch<kPairEmit>(self != 0, brute != 0, st, v, vertices, n_vertices, triangles, m, const_cast<int64_t *>(offsets), s.keys_in, n_pairs, nullptr);
    KPX_LAUNCH_CHECK();
    rc = dsort_run(s, n_pairs, 64, st);
    if (rc) return rc;
    hipLaunchKernelGGL(pair_unpack_kernel, dim3((unsigned)cdiv(n_pairs, 256)), dim3(256), 0, st, (const uint64_t *)s.keys_out, n_pairs, out_pairs);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}
