// kpx_tsdf.hip -- uniform truncated-signed-distance volume ([O3D] pipelines.integration.UniformTSDFVolume; arithmetic contract AC9,
// DESIGN.md 3 and 5.11): integration of depth images (one read-modify-write of the volume for up to KPX_TSDF_MAX_SENSORS images)
// and the two point-cloud extractions (count per block of consecutive voxels -> 64-bit scan -> fill).  The extraction kernels are
// kpx_tsdfcore.h's, over its UniformView; here are the integration kernel and the host side.
//
// Layout: voxel (x, y, z) lives at linear index (x res + y) res + z (z fastest); volume = float2 {tsdf, weight} per voxel, colours
// = float[3] per voxel in a separate array.
#include "kpx_tsdfcore.h"

namespace kpx {
namespace {

// One thread owns two consecutive voxels (one 16-byte access); the last thread of an odd volume owns one.  The volume is read at the
// first image that updates either voxel and written once after the last: a pair no image reaches costs no volume traffic at all.
template <bool U16, bool COLOR>
__global__ __launch_bounds__(256) void tsdf_integrate_kernel(float2 *__restrict__ vol, float *__restrict__ col, int64_t nvox, TsdfIntegrateArgs a)
{
    const int64_t lin0 = 2 * ((int64_t)blockIdx.x * 256 + threadIdx.x);
    if (lin0 >= nvox) return;
    const bool two = lin0 + 1 < nvox;
    double c[2][3];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        int x, y, z;
        tsdf_split((uint32_t)(two || k == 0 ? lin0 + k : lin0), (uint32_t)a.res, x, y, z);
        c[k][0] = a.org[0] + ((double)x + 0.5) * a.vl;
        c[k][1] = a.org[1] + ((double)y + 0.5) * a.vl;
        c[k][2] = a.org[2] + ((double)z + 0.5) * a.vl;
    }
    float f[2] = { 0.0f, 0.0f }, w[2] = { 0.0f, 0.0f }, cc[2][3] = { { 0.0f, 0.0f, 0.0f }, { 0.0f, 0.0f, 0.0f } };
    bool loaded = false;
    for (int s = 0; s < a.count; ++s) {
        float t[2], rgb[2][3];
        bool upd[2];
        upd[0] = tsdf_observe<U16, COLOR>(a, a.s[s], c[0], &t[0], rgb[0]);
        upd[1] = two && tsdf_observe<U16, COLOR>(a, a.s[s], c[1], &t[1], rgb[1]);
        if (!(upd[0] || upd[1])) continue;
        if (!loaded) {
            loaded = true;
            if (two) {
                const float4 q = *reinterpret_cast<const float4 *>(vol + lin0);
                f[0] = q.x; w[0] = q.y; f[1] = q.z; w[1] = q.w;
            } else {
                const float2 q = vol[lin0];
                f[0] = q.x; w[0] = q.y;
            }
            if (COLOR) {
                const float2 *cp = reinterpret_cast<const float2 *>(col + 3 * lin0);        // 24-byte stride: 8-byte aligned
                const float2 q0 = cp[0];
                cc[0][0] = q0.x; cc[0][1] = q0.y;
                if (two) {
                    const float2 q1 = cp[1], q2 = cp[2];
                    cc[0][2] = q1.x; cc[1][0] = q1.y; cc[1][1] = q2.x; cc[1][2] = q2.y;
                } else {
                    cc[0][2] = col[3 * lin0 + 2];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (!upd[k]) continue;
            const float w1 = w[k] + 1.0f;
            f[k] = (f[k] * w[k] + t[k]) / w1;
            if (COLOR) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) cc[k][ch] = (cc[k][ch] * w[k] + rgb[k][ch]) / w1;
            }
            w[k] = w1;
        }
    }
    if (!loaded) return;
    if (two) {
        *reinterpret_cast<float4 *>(vol + lin0) = make_float4(f[0], w[0], f[1], w[1]);
    } else {
        vol[lin0] = make_float2(f[0], w[0]);
    }
    if (COLOR) {
        float2 *cp = reinterpret_cast<float2 *>(col + 3 * lin0);
        cp[0] = make_float2(cc[0][0], cc[0][1]);
        if (two) {
            cp[1] = make_float2(cc[0][2], cc[1][0]);
            cp[2] = make_float2(cc[1][1], cc[1][2]);
        } else {
            col[3 * lin0 + 2] = cc[0][2];
        }
    }
}

inline int64_t tsdf_voxels(int32_t res) { return (int64_t)res * res * res; }
inline int64_t tsdf_chunks(int32_t res) { return cdiv(tsdf_voxels(res), kChunk); }
inline bool tsdf_res_ok(int32_t res) { return res >= 1 && res <= KPX_TSDF_MAX_RESOLUTION; }

}  // namespace
}  // namespace kpx

using namespace kpx;

static int64_t *tsdf_carve(Arena &a, int64_t nchunks) { return a.get<int64_t>((size_t)nchunks + 1); }      // the chunks' offsets and the total
KPX_EXPORT size_t kpx_tsdf_workspace_bytes(int32_t resolution)
{
    if (!tsdf_res_ok(resolution)) return 0;
    Arena a(nullptr, 0);
    tsdf_carve(a, tsdf_chunks(resolution));
    return a.off;
}

KPX_EXPORT int kpx_tsdf_integrate(float *volume, float *color, int32_t resolution, double voxel_length, const double *h_origin, double sdf_trunc,
                                  int32_t count, const void *const *h_depth, int32_t depth_u16, double depth_scale, double depth_trunc,
                                  const uint8_t *const *h_rgb, int32_t width, int32_t height, const double *h_intrinsic, const double *h_extrinsics,
                                  void *stream)
{
    KPX_REQUIRE(tsdf_res_ok(resolution), "kpx_tsdf_integrate: resolution must be in [1, %d]", KPX_TSDF_MAX_RESOLUTION);
    KPX_REQUIRE(voxel_length > 0.0 && sdf_trunc > 0.0, "kpx_tsdf_integrate: voxel_length and sdf_trunc must be positive");
    KPX_REQUIRE(count >= 0, "kpx_tsdf_integrate: negative image count");
    KPX_REQUIRE(width > 0 && height > 0 && (int64_t)width * height < ((int64_t)1 << 31), "kpx_tsdf_integrate: bad image size");
    KPX_REQUIRE(volume && h_origin && h_intrinsic && (count == 0 || (h_depth && h_extrinsics)), "kpx_tsdf_integrate: null pointer");
    KPX_REQUIRE(!color || h_rgb || count == 0, "kpx_tsdf_integrate: a colour volume needs colour images");
    KPX_REQUIRE(((uintptr_t)volume % 16) == 0 && ((uintptr_t)color % 8) == 0, "kpx_tsdf_integrate: the volume must be 16-byte aligned");
    KPX_REQUIRE(!depth_u16 || depth_scale > 0.0, "kpx_tsdf_integrate: depth_scale must be positive");
    for (int32_t i = 0; i < count; ++i)
        KPX_REQUIRE(h_depth[i] && (!color || h_rgb[i]), "kpx_tsdf_integrate: image %d is null", i);
    hipStream_t st = (hipStream_t)stream;
    const int64_t nvox = tsdf_voxels(resolution);
    const unsigned blocks = (unsigned)cdiv(cdiv(nvox, 2), 256);
    for (int32_t first = 0; first < count; first += KPX_TSDF_MAX_SENSORS) {          // more images than a launch holds: chunks, in order
        TsdfIntegrateArgs a;
        memset(&a, 0, sizeof a);
        a.count = count - first < KPX_TSDF_MAX_SENSORS ? count - first : KPX_TSDF_MAX_SENSORS;
        for (int32_t i = 0; i < a.count; ++i) {
            memcpy(a.s[i].E, h_extrinsics + 16 * (size_t)(first + i), sizeof a.s[i].E);
            a.s[i].depth = h_depth[first + i];
            a.s[i].rgb = color ? h_rgb[first + i] : nullptr;
        }
        for (int k = 0; k < 3; ++k) a.org[k] = h_origin[k];
        a.vl = voxel_length; a.trunc = sdf_trunc;
        a.fx = h_intrinsic[0]; a.fy = h_intrinsic[1]; a.cx = h_intrinsic[2]; a.cy = h_intrinsic[3];
        a.scale = (float)depth_scale; a.dtrunc = (float)depth_trunc;
        a.W = width; a.H = height; a.res = resolution;
        float2 *vol = reinterpret_cast<float2 *>(volume);
        if (depth_u16) {
            if (color) hipLaunchKernelGGL((tsdf_integrate_kernel<true, true>), dim3(blocks), dim3(256), 0, st, vol, color, nvox, a);
            else hipLaunchKernelGGL((tsdf_integrate_kernel<true, false>), dim3(blocks), dim3(256), 0, st, vol, color, nvox, a);
        } else {
            if (color) hipLaunchKernelGGL((tsdf_integrate_kernel<false, true>), dim3(blocks), dim3(256), 0, st, vol, color, nvox, a);
            else hipLaunchKernelGGL((tsdf_integrate_kernel<false, false>), dim3(blocks), dim3(256), 0, st, vol, color, nvox, a);
        }
        KPX_LAUNCH_CHECK();
    }
    return KPX_OK;
}

KPX_EXPORT int kpx_tsdf_extract_count(const float *volume, int32_t resolution, int32_t mode, int64_t *d_count, void *ws, size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(tsdf_res_ok(resolution), "kpx_tsdf_extract_count: resolution must be in [1, %d]", KPX_TSDF_MAX_RESOLUTION);
    KPX_REQUIRE(mode == KPX_TSDF_SURFACE || mode == KPX_TSDF_VOXELS, "kpx_tsdf_extract_count: unknown mode %d", mode);
    KPX_REQUIRE(volume && d_count && ws, "kpx_tsdf_extract_count: null pointer");
    const int64_t nchunks = tsdf_chunks(resolution);
    Arena a(ws, ws_bytes);
    int64_t *offsets = tsdf_carve(a, nchunks);
    KPX_ARENA_CHECK(a);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tsdf_count_kernel<UniformView>, dim3((unsigned)cdiv(nchunks, kExtractWaves)), dim3(kExtractWaves * 64), 0, st,
                       uniform_view(volume, nullptr, resolution, 0.0, nullptr), mode, nchunks, offsets);
    scan_i64(offsets, nchunks, st);
    KPX_LAUNCH_CHECK();
    KPX_HIP(hipMemcpyAsync(d_count, offsets + nchunks, sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    return KPX_OK;
}

KPX_EXPORT int kpx_tsdf_extract_fill(const float *volume, const float *color, int32_t resolution, double voxel_length, const double *h_origin,
                                     int32_t mode, int64_t total, float *pts, float *nrm, float *col, void *ws, size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(tsdf_res_ok(resolution), "kpx_tsdf_extract_fill: resolution must be in [1, %d]", KPX_TSDF_MAX_RESOLUTION);
    KPX_REQUIRE(mode == KPX_TSDF_SURFACE || mode == KPX_TSDF_VOXELS, "kpx_tsdf_extract_fill: unknown mode %d", mode);
    KPX_REQUIRE(voxel_length > 0.0 && total >= 0, "kpx_tsdf_extract_fill: bad voxel_length or total");
    if (total == 0) return KPX_OK;
    KPX_REQUIRE(volume && h_origin && pts && ws, "kpx_tsdf_extract_fill: null pointer");
    const int64_t nchunks = tsdf_chunks(resolution);
    Arena a(ws, ws_bytes);
    const int64_t *offsets = tsdf_carve(a, nchunks);
    KPX_ARENA_CHECK(a);
    const TsdfFillArgs f = { pts, mode == KPX_TSDF_SURFACE ? nrm : nullptr, col, total };
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tsdf_fill_kernel<UniformView>, dim3((unsigned)cdiv(nchunks, kExtractWaves)), dim3(kExtractWaves * 64), 0, st,
                       uniform_view(volume, color, resolution, voxel_length, h_origin), mode, nchunks, offsets, f);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}
