// kpx_sensor.hip -- sensor calibration (arithmetic contract AC20): the per-pixel ray table of a distorted lens
// (kpx_xy_table) and the colour image resampled into the depth camera's pixel grid (kpx_color_to_depth).  Both are pure maps: no
// scratch, no atomics, one launch each.  fp64 throughout, every operation rounded separately in the order include/kinectpx.h
// states -- the build's -ffp-contract=off keeps the compiler from fusing any of it, and nothing here calls fma().
#include "kpx_common.h"

namespace kpx {

struct Camera {
    double fx, fy, cx, cy, k1, k2, k3, k4, k5, k6, p1, p2, mr;
};
struct ColorCalibration {
    Camera cam;
    double T[12];          // rows 0..2 of the depth -> colour transform, millimetres
};
struct CalibrationPack {
    ColorCalibration c[KPX_SENSOR_MAX_CALIBRATIONS];       // 16 x 200 bytes: travels in the kernel arguments
};

static Camera camera_from(const double *h)
{
    return Camera{ h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], h[9], h[10], h[11], h[12] };
}

struct Distorted {
    double xd, yd, r2, r4, xx, yy, num, den, radial;
};

__device__ __forceinline__ Distorted distort(const Camera &k, double x, double y)
{
    Distorted o;
    o.xx = x * x;
    o.yy = y * y;
    o.r2 = o.xx + o.yy;
    o.r4 = o.r2 * o.r2;
    const double r6 = o.r4 * o.r2;
    o.num = ((1.0 + k.k1 * o.r2) + k.k2 * o.r4) + k.k3 * r6;
    o.den = ((1.0 + k.k4 * o.r2) + k.k5 * o.r4) + k.k6 * r6;
    o.radial = o.num / o.den;
    const double xy2 = 2.0 * (x * y);
    o.xd = (x * o.radial + k.p1 * xy2) + k.p2 * (o.r2 + 2.0 * o.xx);
    o.yd = (y * o.radial + k.p1 * (o.r2 + 2.0 * o.yy)) + k.p2 * xy2;
    return o;
}

// forward(X, Y, Z) for Z > 0: false = beyond the metric radius
__device__ __forceinline__ bool project(const Camera &k, double X, double Y, double Z, double &u, double &v)
{
    const double x = X / Z, y = Y / Z;
    const Distorted o = distort(k, x, y);
    u = k.fx * o.xd + k.cx;
    v = k.fy * o.yd + k.cy;
    return o.r2 <= k.mr * k.mr;
}

// inverse(u, v): false = the NaN pair
__device__ __forceinline__ bool unproject(const Camera &k, double u, double v, double &x, double &y)
{
    const double xn = (u - k.cx) / k.fx, yn = (v - k.cy) / k.fy;
    x = xn;
    y = yn;
    bool converged = false;
    for (int round = 0; round < 21; ++round) {
        const Distorted o = distort(k, x, y);
        const double ex = o.xd - xn, ey = o.yd - yn;
        if (ex * ex + ey * ey <= 1e-22) { converged = true; break; }
        if (round == 20) break;
        const double nd = (k.k1 + (2.0 * k.k2) * o.r2) + (3.0 * k.k3) * o.r4;
        const double dd = (k.k4 + (2.0 * k.k5) * o.r2) + (3.0 * k.k6) * o.r4;
        const double dr = (nd * o.den - o.num * dd) / (o.den * o.den);
        const double gx = (2.0 * x) * dr, gy = (2.0 * y) * dr;
        const double a = ((o.radial + x * gx) + (2.0 * k.p1) * y) + (6.0 * k.p2) * x;
        const double b = (x * gy + (2.0 * k.p1) * x) + (2.0 * k.p2) * y;
        const double c = (y * gx + (2.0 * k.p1) * x) + (2.0 * k.p2) * y;
        const double d = ((o.radial + y * gy) + (6.0 * k.p1) * y) + (2.0 * k.p2) * x;
        const double det = a * d - b * c;
        if (!__builtin_isfinite(det) || det == 0.0) break;
        x = x - (d * ex - b * ey) / det;
        y = y - (a * ey - c * ex) / det;
    }
    return converged && __builtin_isfinite(x) && __builtin_isfinite(y) && x * x + y * y <= k.mr * k.mr;
}

constexpr int kTableThreads = 256;
// One thread per pixel; a thread's (x, y) is one 8-byte store, a wave's 512 contiguous bytes.
static __global__ __launch_bounds__(kTableThreads) void xy_table_kernel(Camera k, int32_t width, int64_t n_px, float2 *__restrict__ xy)
{
    const int64_t i = (int64_t)blockIdx.x * kTableThreads + threadIdx.x;
    if (i >= n_px) return;
    const int64_t row = i / width;
    const double u = (double)(i - row * width), v = (double)row;
    double x, y;
    const float nan = __builtin_nanf("");
    float2 o = make_float2(nan, nan);
    if (unproject(k, u, v, x, y)) o = make_float2((float)x, (float)y);
    xy[i] = o;
}

// ---- colour -> depth ---------------------------------------------------------------------------------------------------------------
// A block owns kPixPerBlock consecutive depth pixels of one frame (blockIdx.y), four per thread.  The pixels' bytes are packed into
// dwords in registers, laid down in LDS in pixel order, and leave as 16-byte stores from the first 16-byte boundary of the block's
// output range on; the at most 15 bytes in front of that boundary and behind the last whole vector leave as byte stores (a frame's
// output starts wherever frames * n_px * channels puts it, and neighbouring blocks may share a 16-byte line but never a byte).
constexpr int kC2dThreads = 256, kC2dPerThread = 4, kPixPerBlock = kC2dThreads * kC2dPerThread;

template <int C, int INTERP>
__device__ __forceinline__ void sample_pixel(const ColorCalibration &cal, const uint8_t *__restrict__ img, int32_t wc, int32_t hc, uint16_t d, float xt, float yt,
                                             uint32_t out[C])
{
#pragma unroll
    for (int ch = 0; ch < C; ++ch) out[ch] = 0;
    if (d == 0 || __builtin_isnan(xt) || __builtin_isnan(yt)) return;
    const double pz = (double)d, px = (double)xt * pz, py = (double)yt * pz;
    const double *T = cal.T;
    const double qx = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3];
    const double qy = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7];
    const double qz = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];
    if (!(qz > 0.0)) return;
    double uc, vc;
    if (!project(cal.cam, qx, qy, qz, uc, vc)) return;
    if (INTERP == KPX_SAMPLE_NEAREST) {
        const double fx = floor(uc + 0.5), fy = floor(vc + 0.5);
        if (!(fx >= 0.0 && fx <= (double)(wc - 1) && fy >= 0.0 && fy <= (double)(hc - 1))) return;       // (a NaN fails too)
        const uint8_t *p = img + ((int64_t)(int32_t)fy * wc + (int32_t)fx) * C;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) out[ch] = p[ch];
    } else {
        const double x0 = floor(uc), y0 = floor(vc);
        if (!(x0 >= 0.0 && x0 <= (double)(wc - 2) && y0 >= 0.0 && y0 <= (double)(hc - 2))) return;
        const double ax = uc - x0, ay = vc - y0;
        const double bx = 1.0 - ax, by = 1.0 - ay;
        const double w00 = bx * by, w10 = ax * by, w01 = bx * ay, w11 = ax * ay;
        const uint8_t *p0 = img + ((int64_t)(int32_t)y0 * wc + (int32_t)x0) * C;
        const uint8_t *p1 = p0 + (int64_t)wc * C;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const double c00 = (double)p0[ch], c10 = (double)p0[C + ch], c01 = (double)p1[ch], c11 = (double)p1[C + ch];
            const double val = ((w00 * c00 + w10 * c10) + w01 * c01) + w11 * c11;
            out[ch] = (uint32_t)(int32_t)floor(val + 0.5);
        }
    }
}

template <int C, int INTERP>
static __global__ __launch_bounds__(kC2dThreads) void color_to_depth_kernel(const uint16_t *__restrict__ depth, const float *__restrict__ xy,
                                                                            const uint8_t *__restrict__ color, int64_t n_px, int32_t wc, int32_t hc,
                                                                            CalibrationPack pack, int32_t n_cal, int32_t vec_ok,
                                                                            uint8_t *__restrict__ out)
{
    constexpr int kStageWords = kPixPerBlock * C / 4;
    __shared__ uint32_t stage[kStageWords + 8];            // (+8: the funnel below reads up to four words past the last one it needs)
    const int frame = blockIdx.y, cal_id = frame % n_cal;
    const ColorCalibration &cal = pack.c[cal_id];
    const int64_t p0 = (int64_t)blockIdx.x * kPixPerBlock;                     // the block's first pixel
    const int64_t i0 = p0 + (int64_t)threadIdx.x * kC2dPerThread;              // the thread's first pixel
    const uint16_t *dp = depth + (int64_t)frame * n_px;
    const float *tp = xy + (int64_t)cal_id * n_px * 2;
    const uint8_t *img = color + (int64_t)frame * hc * wc * C;

    uint16_t d[kC2dPerThread];
    float xt[kC2dPerThread], yt[kC2dPerThread];
    if (vec_ok && i0 + kC2dPerThread <= n_px) {
        // vec_ok: n_px is a multiple of 4 and both bases are 16-byte aligned, so every frame's and table's group of 4 pixels is too
        const uint2 dv = *reinterpret_cast<const uint2 *>(dp + i0);
        const float4 t0 = *reinterpret_cast<const float4 *>(tp + 2 * i0), t1 = *reinterpret_cast<const float4 *>(tp + 2 * i0 + 4);
        d[0] = (uint16_t)(dv.x & 0xffff); d[1] = (uint16_t)(dv.x >> 16); d[2] = (uint16_t)(dv.y & 0xffff); d[3] = (uint16_t)(dv.y >> 16);
        xt[0] = t0.x; yt[0] = t0.y; xt[1] = t0.z; yt[1] = t0.w; xt[2] = t1.x; yt[2] = t1.y; xt[3] = t1.z; yt[3] = t1.w;
    } else {
#pragma unroll
        for (int k = 0; k < kC2dPerThread; ++k) {
            const bool in = i0 + k < n_px;
            d[k] = in ? dp[i0 + k] : (uint16_t)0;
            xt[k] = in ? tp[2 * (i0 + k)] : 0.0f;
            yt[k] = in ? tp[2 * (i0 + k) + 1] : 0.0f;
        }
    }
    uint32_t px[kC2dPerThread][C];
#pragma unroll
    for (int k = 0; k < kC2dPerThread; ++k) sample_pixel<C, INTERP>(cal, img, wc, hc, d[k], xt[k], yt[k], px[k]);
    if (C == 3) {
        // 12 bytes r g b r g b ... as three little-endian words
        stage[3 * threadIdx.x + 0] = px[0][0] | px[0][1 % C] << 8 | px[0][2 % C] << 16 | px[1][0] << 24;
        stage[3 * threadIdx.x + 1] = px[1][1 % C] | px[1][2 % C] << 8 | px[2][0] << 16 | px[2][1 % C] << 24;
        stage[3 * threadIdx.x + 2] = px[2][2 % C] | px[3][0] << 8 | px[3][1 % C] << 16 | px[3][2 % C] << 24;
    } else {
        stage[threadIdx.x] = px[0][0] | px[1][0] << 8 | px[2][0] << 16 | px[3][0] << 24;
    }
    __syncthreads();

    const int64_t left = n_px - p0;
    const int nbytes = (int)(left < kPixPerBlock ? left : kPixPerBlock) * C;   // what this block owns: out_blk[0 .. nbytes)
    uint8_t *out_blk = out + ((int64_t)frame * n_px + p0) * C;
    const uint8_t *stage_bytes = reinterpret_cast<const uint8_t *>(stage);
    int head = (int)((16 - ((uintptr_t)out_blk & 15)) & 15);                   // bytes in front of the first 16-byte boundary
    if (head > nbytes) head = nbytes;
    const int vecs = (nbytes - head) >> 4;
    const int tail0 = head + 16 * vecs;                                        // first byte behind the last whole vector
    if ((int)threadIdx.x < head) out_blk[threadIdx.x] = stage_bytes[threadIdx.x];
    if ((int)threadIdx.x < nbytes - tail0) out_blk[tail0 + threadIdx.x] = stage_bytes[tail0 + threadIdx.x];
    const int w0 = head >> 2, sh = 8 * (head & 3);
    uint4 *dst = reinterpret_cast<uint4 *>(out_blk + head);
    for (int j = threadIdx.x; j < vecs; j += kC2dThreads) {
        uint32_t w[5];
#pragma unroll
        for (int e = 0; e < 5; ++e) w[e] = stage[w0 + 4 * j + e];
        uint4 v;
        if (sh) {
            v.x = w[0] >> sh | w[1] << (32 - sh);
            v.y = w[1] >> sh | w[2] << (32 - sh);
            v.z = w[2] >> sh | w[3] << (32 - sh);
            v.w = w[3] >> sh | w[4] << (32 - sh);
        } else {
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        dst[j] = v;
    }
}

}  // namespace kpx

using namespace kpx;

static bool camera_ok(const double *h)
{
    for (int i = 0; i < KPX_CAMERA_DOUBLES; ++i)
        if (!__builtin_isfinite(h[i])) return false;
    return h[0] != 0.0 && h[1] != 0.0 && h[12] > 0.0;
}

KPX_EXPORT int kpx_xy_table(const double *h_camera, int32_t width, int32_t height, float *xy, void *stream)
{
    KPX_REQUIRE(width >= 0 && height >= 0, "kpx_xy_table: negative image size %d x %d", (int)width, (int)height);
    KPX_REQUIRE(h_camera, "kpx_xy_table: null camera");
    KPX_REQUIRE(camera_ok(h_camera), "kpx_xy_table: the camera needs finite numbers, non-zero focal lengths and a positive metric radius");
    const int64_t n_px = (int64_t)width * height;
    if (n_px == 0) return KPX_OK;
    KPX_REQUIRE(xy, "kpx_xy_table: null pointer");
    hipLaunchKernelGGL(xy_table_kernel, dim3((unsigned)cdiv(n_px, kTableThreads)), dim3(kTableThreads), 0, (hipStream_t)stream, camera_from(h_camera), width,
                       n_px, reinterpret_cast<float2 *>(xy));
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT int kpx_color_to_depth(const uint16_t *depth, const float *xy, const uint8_t *color, int64_t n_px, int32_t frames, int32_t color_width,
                                  int32_t color_height, int32_t channels, const double *h_calibrations, int32_t calibrations, int32_t interpolation,
                                  uint8_t *out, void *stream)
{
    KPX_REQUIRE(n_px >= 0 && frames >= 0, "kpx_color_to_depth: negative size (n_px %lld, frames %d)", (long long)n_px, (int)frames);
    KPX_REQUIRE(frames <= 65535, "kpx_color_to_depth: at most 65535 frames per call, got %d", (int)frames);
    KPX_REQUIRE(n_px <= (int64_t)kPixPerBlock * 0x7fffffff, "kpx_color_to_depth: n_px %lld is out of range", (long long)n_px);
    KPX_REQUIRE(channels == 1 || channels == 3, "kpx_color_to_depth: channels must be 1 or 3, got %d", (int)channels);
    KPX_REQUIRE(interpolation == KPX_SAMPLE_NEAREST || interpolation == KPX_SAMPLE_BILINEAR, "kpx_color_to_depth: unknown interpolation %d",
                (int)interpolation);
    KPX_REQUIRE(color_width >= 1 && color_height >= 1, "kpx_color_to_depth: colour image size %d x %d", (int)color_width, (int)color_height);
    KPX_REQUIRE(calibrations >= 1 && calibrations <= KPX_SENSOR_MAX_CALIBRATIONS, "kpx_color_to_depth: 1 to %d calibrations, got %d",
                KPX_SENSOR_MAX_CALIBRATIONS, (int)calibrations);
    KPX_REQUIRE(frames % calibrations == 0, "kpx_color_to_depth: %d calibrations do not divide %d frames", (int)calibrations, (int)frames);
    KPX_REQUIRE(h_calibrations, "kpx_color_to_depth: null calibrations");
    for (int s = 0; s < calibrations; ++s) {
        const double *h = h_calibrations + (size_t)s * KPX_CALIBRATION_DOUBLES;
        bool ok = camera_ok(h);
        for (int i = 0; i < 12; ++i) ok = ok && __builtin_isfinite(h[KPX_CAMERA_DOUBLES + i]);
        KPX_REQUIRE(ok, "kpx_color_to_depth: calibration %d needs finite numbers, non-zero focal lengths and a positive metric radius", s);
    }
    if (frames == 0 || n_px == 0) return KPX_OK;
    KPX_REQUIRE(depth && xy && color && out, "kpx_color_to_depth: null pointer");
    CalibrationPack pack;
    memset(&pack, 0, sizeof pack);
    for (int s = 0; s < calibrations; ++s) {
        const double *h = h_calibrations + (size_t)s * KPX_CALIBRATION_DOUBLES;
        pack.c[s].cam = camera_from(h);
        memcpy(pack.c[s].T, h + KPX_CAMERA_DOUBLES, sizeof pack.c[s].T);
    }
    const int32_t vec_ok = n_px % 4 == 0 && (uintptr_t)depth % 16 == 0 && (uintptr_t)xy % 16 == 0;
    const dim3 grid((unsigned)cdiv(n_px, kPixPerBlock), (unsigned)frames), block(kC2dThreads);
    hipStream_t st = (hipStream_t)stream;
#define KPX_C2D(C, I) \
    hipLaunchKernelGGL((color_to_depth_kernel<C, I>), grid, block, 0, st, depth, xy, color, n_px, color_width, color_height, pack, calibrations, vec_ok, out)
    if (channels == 3 && interpolation == KPX_SAMPLE_BILINEAR) KPX_C2D(3, KPX_SAMPLE_BILINEAR);
    else if (channels == 3) KPX_C2D(3, KPX_SAMPLE_NEAREST);
    else if (interpolation == KPX_SAMPLE_BILINEAR) KPX_C2D(1, KPX_SAMPLE_BILINEAR);
    else KPX_C2D(1, KPX_SAMPLE_NEAREST);
#undef KPX_C2D
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}
