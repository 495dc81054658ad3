// kpx_voxelgrid.hip -- occupancy grids ([O3D] geometry.VoxelGrid; arithmetic contract AC10): the grid of a
// cloud (the steps of kpx_voxelsteps.h with the grid's own origin), a dense grid, space carving by depth maps and silhouettes (every
// voxel projects its 8 corners into up to KPX_VOXELGRID_MAX_IMAGES images per launch) and point inclusion (binary search).
//
// Layout: a grid is its M keys gx << 42 | gy << 21 | gz (u64, strictly ascending) and one float32 colour triple per key; origin and
// voxel size travel by value.
#include "kpx_voxelsteps.h"

#include <math.h>

namespace kpx {
namespace {

constexpr uint64_t kAxisMask = (1ull << 21) - 1ull;

// ---- grid of a cloud ------------------------------------------------------------------------------------------------------------
// origin = min_bound - v 0.5 of the cloud's box, or the caller's; clears the error word
__global__ void grid_origin_kernel(const double *__restrict__ bbox, double voxel, double g0, double g1, double g2, int given, double *__restrict__ org,
                                   int32_t *__restrict__ err)
{
    const double g[3] = { g0, g1, g2 };
    for (int a = 0; a < 3; ++a) org[a] = given ? g[a] : bbox[a] - voxel * 0.5;
    *err = 0;
}
// 63-bit fixed fields over the grid's origin (voxel_key_kernel hands it over where the other packers take a box); a bad index sets *err
struct OriginKeys {
    struct Grid {};
    uint64_t *keys;
    int32_t *err;
    template <class Set> __device__ __forceinline__ Grid grid(const Set &, const double *, double) const { return Grid(); }
    __device__ __forceinline__ void put(const Grid &, const double *__restrict__ org, double voxel, int64_t i, int, const double q[3]) const
    {
        double f[3];
        const double o[3] = { org[0], org[1], org[2] };
        if (voxel_cell_at(q, o, voxel, f)) { *err = 1; f[0] = f[1] = f[2] = 0.0; }
        keys[i] = ((uint64_t)f[0] << 42) | ((uint64_t)f[1] << 21) | (uint64_t)f[2];
    }
};
// the colours of a cloud alone (the segment sum's point row stays zero and is never written)
struct ColourLoad {
    using Coord = float;
    const float *col;
    __device__ __forceinline__ bool has_col() const { return true; }
    __device__ __forceinline__ void operator()(int64_t p, float v[3], float c[3], float *) const
    {
#pragma unroll
        for (int a = 0; a < 3; ++a) { v[a] = 0.0f; c[a] = col[3 * p + a]; }
    }
};
// one thread per voxel: its key and its mean colour (sequential fp64 sum in ascending point index; zeros without colours)
__global__ __launch_bounds__(256) void grid_colour_kernel(const float *__restrict__ col, int64_t n, const uint64_t *__restrict__ sorted_keys,
                                                          const int32_t *__restrict__ vals, const int32_t *__restrict__ seg_start, int32_t *__restrict__ d_count,
                                                          const int32_t *__restrict__ err, uint64_t *__restrict__ okeys, float *__restrict__ ocol)
{
    const int32_t m_total = *d_count;
    if (blockIdx.x == 0 && threadIdx.x == 0 && *err) *d_count = KPX_ERR_RANGE;      // as voxel_mean_kernel
    for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < m_total; m += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s0 = seg_start[m], s1 = (m + 1 < m_total) ? seg_start[m + 1] : n;
        okeys[m] = sorted_keys[s0];
        double sp[3] = { 0, 0, 0 }, sc[3] = { 0, 0, 0 }, sn[3];
        if (col) voxel_segment_sum<false>(vals, s0, s1, ColourLoad{ col }, sp, sc, sn);
        voxel_write_row(sc, sc, (double)(s1 - s0), ocol + 3 * m, nullptr);           // the colour sums as the row: (float)(sum / count)
    }
}

// ---- dense grid -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void grid_dense_kernel(int64_t total, uint32_t nh, uint32_t nd, float c0, float c1, float c2, uint64_t *__restrict__ keys,
                                                         float *__restrict__ col)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const uint64_t t = (uint64_t)i / nd, z = (uint64_t)i - t * nd, x = t / nh, y = t - x * nh;
    keys[i] = (x << 42) | (y << 21) | z;
    col[3 * i] = c0; col[3 * i + 1] = c1; col[3 * i + 2] = c2;
}

// ---- carving --------------------------------------------------------------------------------------------------------------------
struct CarveImage {
    double E[12];              // world -> camera, rows 0..2 of the row-major 4x4
    const void *px;            // [H W] of the launch's pixel format
};
struct CarveArgs {
    CarveImage im[KPX_VOXELGRID_MAX_IMAGES];
    double org[3], v, fx, fy, cx, cy;
    float scale, dtrunc;
    int32_t W, H, count, mode, keep_outside, keep_unmeasured, first;
};

// pixel (x, y) as the contract's float32 value: FMT 0 float32 as it is, 1 raw uint16 converted as AC9 does, 2 a uint8 mask read as 0 / 1
template <int FMT> __device__ __forceinline__ double carve_pixel(const CarveArgs &a, const void *__restrict__ px, int x, int y)
{
    const int64_t i = (int64_t)y * a.W + x;
    float d;
    if (FMT == 1) {
        d = (float)((const uint16_t *)px)[i] / a.scale;
        if (d > a.dtrunc) d = 0.0f;
    } else if (FMT == 2) {
        d = ((const uint8_t *)px)[i] ? 1.0f : 0.0f;
    } else {
        d = ((const float *)px)[i];
    }
    return (double)d;
}
// AC10 for one corner and one image: does the corner keep the voxel?  No test of the sign of z ([O3D]): IEEE division decides, and a
// NaN or infinite projection is simply not within the image.  The taps are (ui, vi) .. (ui + 1, vi + 1) with 0 <= ui <= W - 2 and
// 0 <= vi <= H - 2 (W, H >= 2 is an argument check): never outside the image.
template <int FMT> __device__ __forceinline__ bool carve_corner_keeps(const CarveArgs &a, const CarveImage &im, const double x[3])
{
    const double *E = im.E;
    const double X = fma(E[0], x[0], fma(E[1], x[1], fma(E[2], x[2], E[3])));
    const double Y = fma(E[4], x[0], fma(E[5], x[1], fma(E[6], x[2], E[7])));
    const double z = fma(E[8], x[0], fma(E[9], x[1], fma(E[10], x[2], E[11])));
    const double u = (a.fx * X + a.cx * z) / z, v = (a.fy * Y + a.cy * z) / z;
    const bool within = u >= 0.0 && u <= (double)(a.W - 1) && v >= 0.0 && v <= (double)(a.H - 1);
    if (!within) return a.keep_outside != 0;
    int ui = (int)u, vi = (int)v;
    ui = ui < a.W - 2 ? ui : a.W - 2; ui = ui > 0 ? ui : 0;
    vi = vi < a.H - 2 ? vi : a.H - 2; vi = vi > 0 ? vi : 0;
    const double pu = u - (double)ui, pv = v - (double)vi;
    const double a00 = carve_pixel<FMT>(a, im.px, ui, vi), a01 = carve_pixel<FMT>(a, im.px, ui, vi + 1);
    const double a10 = carve_pixel<FMT>(a, im.px, ui + 1, vi), a11 = carve_pixel<FMT>(a, im.px, ui + 1, vi + 1);
    const double d = (a00 * (1.0 - pv) + a01 * pv) * (1.0 - pu) + (a10 * (1.0 - pv) + a11 * pv) * pu;
    if (!(d > 0.0)) return a.keep_unmeasured != 0;
    return a.mode == KPX_VOXELGRID_SILHOUETTE || z >= d;
}
// One thread per voxel.  It leaves at the first image that carves the voxel and, within an image, at the first corner that keeps it.
// No conservative screen is applied: without a test of the sign of z a corner behind the camera can land anywhere in the image, so
// no bound on the centre's projection bounds the corners' (a voxel that straddles z = 0 projects to both infinities).
// flags[i] = 1 survivor / 0 carved; first == 0: a later launch of a chunked call -- voxels already carved are skipped.
template <int FMT>
__global__ __launch_bounds__(256) void carve_flag_kernel(const uint64_t *__restrict__ keys, int64_t m, CarveArgs a, uint8_t *__restrict__ flags)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    if (!a.first && !flags[i]) return;
    const uint64_t key = keys[i];
    const double g[3] = { (double)(key >> 42), (double)((key >> 21) & kAxisMask), (double)(key & kAxisMask) };
    const double r = a.v * 0.5;
    double lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double c = a.org[k] + (g[k] + 0.5) * a.v;
        lo[k] = c - r;
        hi[k] = c + r;
    }
    for (int s = 0; s < a.count; ++s) {
        bool kept = false;
        for (int t = 0; t < 8 && !kept; ++t) {
            const double x[3] = { (t & 1) ? hi[0] : lo[0], (t & 2) ? hi[1] : lo[1], (t & 4) ? hi[2] : lo[2] };
            kept = carve_corner_keeps<FMT>(a, a.im[s], x);
        }
        if (!kept) { flags[i] = 0; return; }
    }
    flags[i] = 1;
}
struct FlagPred {
    const uint8_t *flags;
    __device__ bool operator()(int64_t i, int) const { return flags[i] != 0; }
};
struct GridEmit {
    const uint64_t *keys;
    const float *col;
    uint64_t *okeys;
    float *ocol;
    __device__ void operator()(int64_t i, int, int32_t dst) const
    {
        okeys[dst] = keys[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) ocol[3 * (int64_t)dst + k] = col[3 * i + k];
    }
};
struct CarveScratch {
    uint8_t *flags;
    int32_t *counts;
};
void carve_scratch(Arena &a, int64_t m, CarveScratch *s)
{
    s->flags = a.get<uint8_t>((size_t)(m > 0 ? m : 1));
    s->counts = a.get<int32_t>((size_t)compact_ws_ints(m));
}

// ---- inclusion ------------------------------------------------------------------------------------------------------------------
struct IncludedArgs {
    double org[3], v;
};
template <class Q>
__global__ __launch_bounds__(256) void grid_included_kernel(const Q *__restrict__ queries, int64_t n, const uint64_t *__restrict__ keys, int64_t m, IncludedArgs a,
                                                            uint8_t *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double q[3] = { (double)queries[3 * i], (double)queries[3 * i + 1], (double)queries[3 * i + 2] };
    double f[3];
    uint8_t in = 0;
    if (!voxel_cell_at(q, a.org, a.v, f)) {                          // out of [0, 2^21) or NaN: not included
        const uint64_t key = ((uint64_t)f[0] << 42) | ((uint64_t)f[1] << 21) | (uint64_t)f[2];
        int64_t lo = 0, hi = m;                                      // first position with keys[pos] >= key
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (keys[mid] < key) lo = mid + 1; else hi = mid;
        }
        in = (lo < m && keys[lo] == key) ? 1 : 0;
    }
    out[i] = in;
}

inline bool finite3(const double *p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

}  // namespace
}  // namespace kpx

using namespace kpx;

KPX_EXPORT size_t kpx_voxelgrid_from_cloud_workspace_bytes(int64_t n)
{
    if (n < 0 || n >= ((int64_t)1 << 31)) return 0;
    Arena a(nullptr, 0);
    VoxelScratch s;
    voxel_carve(a, n, kPlainCarve, &s);
    return a.off;
}
KPX_EXPORT int kpx_voxelgrid_from_cloud(const float *pts, const float *col, int64_t n, double voxel, const double *h_origin, uint64_t *keys, float *colors,
                                        double *d_origin, int32_t *d_count, void *ws, size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(voxel > 0.0, "voxel_size <= 0");                       // [O3D] raises here
    KPX_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "kpx_voxelgrid_from_cloud: bad size");
    KPX_REQUIRE(!h_origin || finite3(h_origin), "kpx_voxelgrid_from_cloud: the origin must be finite");
    KPX_REQUIRE(d_origin && d_count && ws, "kpx_voxelgrid_from_cloud: null pointer");
    KPX_REQUIRE(n == 0 || (pts && keys && colors), "kpx_voxelgrid_from_cloud: null pointer");
    hipStream_t st = (hipStream_t)stream;
    Arena a(ws, ws_bytes);
    VoxelScratch s;
    voxel_carve(a, n, kPlainCarve, &s);
    KPX_ARENA_CHECK(a);
    if (n == 0) {                       // [O3D] an empty cloud: an empty grid; its origin is the caller's, or zero
        double o[3] = { h_origin ? h_origin[0] : 0.0, h_origin ? h_origin[1] : 0.0, h_origin ? h_origin[2] : 0.0 };
        KPX_HIP(hipMemcpyAsync(d_origin, o, sizeof o, hipMemcpyHostToDevice, st));
        KPX_HIP(hipStreamSynchronize(st));                             // o lives on this stack frame
        KPX_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), st));
        return KPX_OK;
    }
    if (!h_origin) {
        const int rc = bbox_f32(pts, n, s.bbox, s.part, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(grid_origin_kernel, dim3(1), dim3(1), 0, st, (const double *)s.bbox, voxel, h_origin ? h_origin[0] : 0.0, h_origin ? h_origin[1] : 0.0,
                       h_origin ? h_origin[2] : 0.0, h_origin ? 1 : 0, d_origin, s.err);
    const int nb = (int)(cdiv(n, 256) > 4096 ? 4096 : cdiv(n, 256));
    CloudSet<1> one;
    one.pts[0] = pts; one.off[0] = 0; one.off[1] = n; one.count = 1;
    hipLaunchKernelGGL((voxel_key_kernel<CloudSet<1>, StoredPoint, OriginKeys>), dim3(nb), dim3(256), 0, st, one, (const double *)d_origin, voxel,
                       OriginKeys{ s.sort.keys_in, s.err }, s.sort.vals_in);
    const int rc = voxel_sort_and_heads<uint64_t>(s, n, 63, d_count, st);
    if (rc) return rc;
    hipLaunchKernelGGL(grid_colour_kernel, dim3(nb), dim3(256), 0, st, col, n, (const uint64_t *)s.sort.keys_out, (const int32_t *)s.sort.vals_out,
                       (const int32_t *)s.seg_start, d_count, (const int32_t *)s.err, keys, colors);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT int kpx_voxelgrid_dense(int32_t nw, int32_t nh, int32_t nd, const float *h_color, uint64_t *keys, float *colors, void *stream)
{
    KPX_REQUIRE(nw >= 0 && nh >= 0 && nd >= 0 && nw <= KPX_VOXELGRID_AXIS_CELLS && nh <= KPX_VOXELGRID_AXIS_CELLS && nd <= KPX_VOXELGRID_AXIS_CELLS,
                "kpx_voxelgrid_dense: every dimension must be in [0, %d]", KPX_VOXELGRID_AXIS_CELLS);
    const double total_d = (double)nw * (double)nh * (double)nd;
    KPX_REQUIRE(total_d <= 2147483647.0, "kpx_voxelgrid_dense: more than 2^31 - 1 voxels");
    const int64_t total = (int64_t)nw * nh * nd;
    if (total == 0) return KPX_OK;
    KPX_REQUIRE(h_color && keys && colors, "kpx_voxelgrid_dense: null pointer");
    hipLaunchKernelGGL(grid_dense_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, total, (uint32_t)nh, (uint32_t)nd, h_color[0],
                       h_color[1], h_color[2], keys, colors);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT size_t kpx_voxelgrid_carve_workspace_bytes(int64_t m)
{
    if (m < 0 || m >= ((int64_t)1 << 31)) return 0;
    Arena a(nullptr, 0);
    CarveScratch s;
    carve_scratch(a, m, &s);
    return a.off;
}
KPX_EXPORT int kpx_voxelgrid_carve(const uint64_t *keys, const float *colors, int64_t m, const double *h_origin, double voxel, int32_t mode, int32_t count,
                                   const void *const *h_images, int32_t format, double depth_scale, double depth_trunc, int32_t width, int32_t height,
                                   const double *h_intrinsic, const double *h_extrinsics, int32_t keep_voxels_outside_image, int32_t keep_unmeasured,
                                   uint64_t *out_keys, float *out_colors, int32_t *d_count, void *ws, size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(voxel > 0.0, "voxel_size <= 0");
    KPX_REQUIRE(m >= 0 && m < ((int64_t)1 << 31), "kpx_voxelgrid_carve: bad size");
    KPX_REQUIRE(mode == KPX_VOXELGRID_DEPTH || mode == KPX_VOXELGRID_SILHOUETTE, "kpx_voxelgrid_carve: unknown mode %d", mode);
    KPX_REQUIRE(format == KPX_VOXELGRID_F32 || format == KPX_VOXELGRID_U16 || format == KPX_VOXELGRID_U8, "kpx_voxelgrid_carve: unknown pixel format %d", format);
    KPX_REQUIRE(count >= 0, "kpx_voxelgrid_carve: negative image count");
    KPX_REQUIRE(width >= 2 && height >= 2 && (int64_t)width * height < ((int64_t)1 << 31), "kpx_voxelgrid_carve: images need width, height >= 2");
    KPX_REQUIRE(format != KPX_VOXELGRID_U16 || depth_scale > 0.0, "kpx_voxelgrid_carve: depth_scale must be positive");
    KPX_REQUIRE(h_origin && finite3(h_origin) && h_intrinsic && d_count && ws && (count == 0 || (h_images && h_extrinsics)), "kpx_voxelgrid_carve: null pointer");
    KPX_REQUIRE(m == 0 || (keys && colors && out_keys && out_colors && out_keys != keys && out_colors != colors),
                "kpx_voxelgrid_carve: null pointer, or the output aliases the input");
    for (int32_t i = 0; i < count; ++i) KPX_REQUIRE(h_images[i], "kpx_voxelgrid_carve: image %d is null", i);
    hipStream_t st = (hipStream_t)stream;
    Arena a(ws, ws_bytes);
    CarveScratch s;
    carve_scratch(a, m, &s);
    KPX_ARENA_CHECK(a);
    if (m == 0) { KPX_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), st)); return KPX_OK; }
    const unsigned blocks = (unsigned)cdiv(m, 256);
    if (count == 0) KPX_HIP(hipMemsetAsync(s.flags, 1, (size_t)m, st));          // no image carves anything
    for (int32_t first = 0; first < count; first += KPX_VOXELGRID_MAX_IMAGES) {          // more images than a launch holds: chunks
        CarveArgs c;
        memset(&c, 0, sizeof c);
        c.count = count - first < KPX_VOXELGRID_MAX_IMAGES ? count - first : KPX_VOXELGRID_MAX_IMAGES;
        for (int32_t i = 0; i < c.count; ++i) {
            memcpy(c.im[i].E, h_extrinsics + 16 * (size_t)(first + i), sizeof c.im[i].E);
            c.im[i].px = h_images[first + i];
        }
        for (int k = 0; k < 3; ++k) c.org[k] = h_origin[k];
        c.v = voxel;
        c.fx = h_intrinsic[0]; c.fy = h_intrinsic[1]; c.cx = h_intrinsic[2]; c.cy = h_intrinsic[3];
        c.scale = (float)depth_scale; c.dtrunc = (float)depth_trunc;
        c.W = width; c.H = height; c.mode = mode;
        c.keep_outside = keep_voxels_outside_image ? 1 : 0; c.keep_unmeasured = keep_unmeasured ? 1 : 0; c.first = first == 0 ? 1 : 0;
        if (format == KPX_VOXELGRID_U16) hipLaunchKernelGGL(carve_flag_kernel<1>, dim3(blocks), dim3(256), 0, st, keys, m, c, s.flags);
        else if (format == KPX_VOXELGRID_U8) hipLaunchKernelGGL(carve_flag_kernel<2>, dim3(blocks), dim3(256), 0, st, keys, m, c, s.flags);
        else hipLaunchKernelGGL(carve_flag_kernel<0>, dim3(blocks), dim3(256), 0, st, keys, m, c, s.flags);
        KPX_LAUNCH_CHECK();
    }
    return compact(FlagPred{ s.flags }, GridEmit{ keys, colors, out_keys, out_colors }, m, 1, s.counts, d_count, st);
}

KPX_EXPORT int kpx_voxelgrid_included(const void *queries, int32_t queries_f64, int64_t n, const uint64_t *keys, int64_t m, const double *h_origin, double voxel,
                                      uint8_t *out, void *stream)
{
    KPX_REQUIRE(voxel > 0.0, "voxel_size <= 0");
    KPX_REQUIRE(n >= 0 && m >= 0 && m < ((int64_t)1 << 31), "kpx_voxelgrid_included: bad size");
    KPX_REQUIRE(h_origin && finite3(h_origin), "kpx_voxelgrid_included: the origin must be finite");
    if (n == 0) return KPX_OK;
    KPX_REQUIRE(queries && out && (m == 0 || keys), "kpx_voxelgrid_included: null pointer");
    IncludedArgs a;
    for (int k = 0; k < 3; ++k) a.org[k] = h_origin[k];
    a.v = voxel;
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)cdiv(n, 256);
    if (queries_f64) hipLaunchKernelGGL(grid_included_kernel<double>, dim3(blocks), dim3(256), 0, st, (const double *)queries, n, keys, m, a, out);
    else hipLaunchKernelGGL(grid_included_kernel<float>, dim3(blocks), dim3(256), 0, st, (const float *)queries, n, keys, m, a, out);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}
