// kpx_sensor.hip -- sensor calibration (arithmetic contract AC20): the per-pixel ray table of a distorted lens
// (kpx_xy_table) and the colour image resampled into the depth camera's pixel grid (kpx_color_to_depth).  Both are pure maps: no
// scratch, no atomics, one launch each.  AC21 adds the depth image warped into the colour camera through a 32-bit
// z-buffer of integer minima (kpx_depth_to_color) and the registration with an occlusion test against it (kpx_color_to_depth_visible).
// AC22 adds lens undistortion: the map from the pixels of a distortion-free target camera to source pixel coordinates
// (kpx_undistort_map) and the images resampled through stored maps (kpx_remap_u8, kpx_remap_depth) -- pure maps again.
// fp64 throughout, every operation rounded separately in the order include/kinectpx.h states -- the build's -ffp-contract=off keeps
// the compiler from fusing any of it, and nothing here calls fma().
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
// AC20's "colour -> depth" chain of one depth pixel, which is also AC21's vertex: false = no point in the colour camera (no depth, no
// ray, behind the camera, beyond the metric radius)
__device__ __forceinline__ bool depth_pixel_to_color(const ColorCalibration &cal, uint16_t d, float xt, float yt, double &uc, double &vc, double &qz)
{
    if (d == 0 || __builtin_isnan(xt) || __builtin_isnan(yt)) return false;
    const double pz = (double)d, px = (double)xt * pz, py = (double)yt * pz;
    const double *T = cal.T;
    const double qx = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3];
    const double qy = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7];
    qz = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];
    if (!(qz > 0.0)) return false;
    return project(cal.cam, qx, qy, qz, uc, vc);
}

__device__ __forceinline__ bool occluded(const uint16_t *__restrict__ warped, int32_t wc, double fx, double fy, double qz, double occlusion_mm)
{
    const uint16_t w = warped[(int64_t)(int32_t)fy * wc + (int32_t)fx];
    return w != 0 && qz - (double)w > occlusion_mm;
}

// AC20's samplers at (uc, vc) of a wc x hc image of C channels: out stays as it is where the rules give no sample (a NaN coordinate
// fails the range tests).  VISIBLE: AC21's occlusion test against the warped depth image of the frame (`warped`, colour-camera grid)
template <int C, int INTERP, bool VISIBLE>
__device__ __forceinline__ void sample_at(const uint8_t *__restrict__ img, const uint16_t *__restrict__ warped, double occlusion_mm, int32_t wc, int32_t hc,
                                          double uc, double vc, double qz, uint32_t out[C])
{
    if (INTERP == KPX_SAMPLE_NEAREST) {
        const double fx = floor(uc + 0.5), fy = floor(vc + 0.5);
        if (!(fx >= 0.0 && fx <= (double)(wc - 1) && fy >= 0.0 && fy <= (double)(hc - 1))) return;       // (a NaN fails too)
        if (VISIBLE && occluded(warped, wc, fx, fy, qz, occlusion_mm)) return;
        const uint8_t *p = img + ((int64_t)(int32_t)fy * wc + (int32_t)fx) * C;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) out[ch] = p[ch];
    } else {
        const double x0 = floor(uc), y0 = floor(vc);
        if (!(x0 >= 0.0 && x0 <= (double)(wc - 2) && y0 >= 0.0 && y0 <= (double)(hc - 2))) return;
        if (VISIBLE && occluded(warped, wc, floor(uc + 0.5), floor(vc + 0.5), qz, occlusion_mm)) return;      // (inside: the 2 x 2 block is)
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

template <int C, int INTERP, bool VISIBLE>
__device__ __forceinline__ void sample_pixel(const ColorCalibration &cal, const uint8_t *__restrict__ img, const uint16_t *__restrict__ warped,
                                             double occlusion_mm, int32_t wc, int32_t hc, uint16_t d, float xt, float yt, uint32_t out[C])
{
#pragma unroll
    for (int ch = 0; ch < C; ++ch) out[ch] = 0;
    double uc, vc, qz;
    if (!depth_pixel_to_color(cal, d, xt, yt, uc, vc, qz)) return;
    sample_at<C, INTERP, VISIBLE>(img, warped, occlusion_mm, wc, hc, uc, vc, qz, out);
}

constexpr int kC2dThreads = 256, kC2dPerThread = 4, kPixPerBlock = kC2dThreads * kC2dPerThread;

// The packed store of a block of byte pixels, four per thread: the pixels' bytes are packed into dwords in registers, laid down in LDS
// in pixel order, and leave as 16-byte stores from the first 16-byte boundary of the block's output range out_blk[0 .. nbytes) on; the
// at most 15 bytes in front of that boundary and behind the last whole vector leave as byte stores (neighbouring blocks may share a
// 16-byte line but never a byte).  stage: kPixPerBlock * C / 4 + 8 words of LDS.
template <int C>
__device__ __forceinline__ void store_packed(const uint32_t px[kC2dPerThread][C], uint32_t *stage, uint8_t *__restrict__ out_blk, int nbytes)
{
    if (C == 3) {
        // 12 bytes r g b r g b ... as three little-endian words
        stage[3 * threadIdx.x + 0] = px[0][0] | px[0][1 % C] << 8 | px[0][2 % C] << 16 | px[1][0] << 24;
        stage[3 * threadIdx.x + 1] = px[1][1 % C] | px[1][2 % C] << 8 | px[2][0] << 16 | px[2][1 % C] << 24;
        stage[3 * threadIdx.x + 2] = px[2][2 % C] | px[3][0] << 8 | px[3][1 % C] << 16 | px[3][2 % C] << 24;
    } else {
        stage[threadIdx.x] = px[0][0] | px[1][0] << 8 | px[2][0] << 16 | px[3][0] << 24;
    }
    __syncthreads();

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

// A block owns kPixPerBlock consecutive depth pixels of one frame (blockIdx.y), four per thread, and stores them with store_packed (a
// frame's output starts wherever frames * n_px * channels puts it).
template <int C, int INTERP, bool VISIBLE>
static __global__ __launch_bounds__(kC2dThreads) void color_to_depth_kernel(const uint16_t *__restrict__ depth, const float *__restrict__ xy,
                                                                            const uint8_t *__restrict__ color, const uint16_t *__restrict__ warped,
                                                                            double occlusion_mm, int64_t n_px, int32_t wc, int32_t hc,
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
    const uint16_t *wimg = VISIBLE ? warped + (int64_t)frame * hc * wc : nullptr;

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
    for (int k = 0; k < kC2dPerThread; ++k) sample_pixel<C, INTERP, VISIBLE>(cal, img, wimg, occlusion_mm, wc, hc, d[k], xt[k], yt[k], px[k]);
    const int64_t left = n_px - p0;
    const int nbytes = (int)(left < kPixPerBlock ? left : kPixPerBlock) * C;   // what this block owns
    store_packed<C>(px, stage, out + ((int64_t)frame * n_px + p0) * C, nbytes);
}

// ---- depth -> colour (AC21) -----------------------------------------------------------------------------------------------------------
// Three dispatches: the z-buffer's clear to 0xFFFFFFFF (a memset node), the raster kernel, the resolve kernel.
// Raster: a block owns a tile of kWarpTileW x kWarpTileH quads of one frame (blockIdx.y) and projects the tile's (kWarpTileW + 1) x
// (kWarpTileH + 1) vertices once into LDS -- the fp64 chain with its two divisions runs 1.16 times per depth pixel instead of four.
// An invalid vertex is stored with z = 0 (a valid one has q_z > 0).  Each thread then walks its quad's two triangles over their
// bounding boxes (less than KPX_WARP_MAX_SPAN pixels a side) with one atomicMin per covered pixel on the 32-bit buffer.
constexpr int kWarpTileW = 32, kWarpTileH = 8, kWarpThreads = kWarpTileW * kWarpTileH;
constexpr int kWarpVertW = kWarpTileW + 1, kWarpVerts = kWarpVertW * (kWarpTileH + 1);
constexpr uint32_t kWarpEmpty = 0xFFFFFFFFu;

struct WarpVertex {
    double u, v, z;
};

__device__ __forceinline__ double edge(double au, double av, double bu, double bv, double pu, double pv)
{
    return (bu - au) * (pv - av) - (bv - av) * (pu - au);
}

__device__ __forceinline__ void raster_triangle(const WarpVertex &p0, const WarpVertex &p1, const WarpVertex &p2, double max_gap_mm, int32_t wc,
                                                int32_t hc, uint32_t *__restrict__ zbuf)
{
    if (!(p0.z > 0.0 && p1.z > 0.0 && p2.z > 0.0)) return;
    const double zmax = fmax(fmax(p0.z, p1.z), p2.z), zmin = fmin(fmin(p0.z, p1.z), p2.z);
    if (zmax - zmin > max_gap_mm) return;
    const double bx0 = ceil(fmin(fmin(p0.u, p1.u), p2.u)), bx1 = floor(fmax(fmax(p0.u, p1.u), p2.u));
    const double by0 = ceil(fmin(fmin(p0.v, p1.v), p2.v)), by1 = floor(fmax(fmax(p0.v, p1.v), p2.v));
    if (bx1 - bx0 >= (double)KPX_WARP_MAX_SPAN || by1 - by0 >= (double)KPX_WARP_MAX_SPAN) return;
    const double area = edge(p0.u, p0.v, p1.u, p1.v, p2.u, p2.v);
    if (area == 0.0 || !__builtin_isfinite(area)) return;                      // (finite: every coordinate is, so the box below is too)
    const double cx0 = fmax(bx0, 0.0), cx1 = fmin(bx1, (double)(wc - 1)), cy0 = fmax(by0, 0.0), cy1 = fmin(by1, (double)(hc - 1));
    if (!(cx0 <= cx1 && cy0 <= cy1)) return;
    const int32_t x0 = (int32_t)cx0, x1 = (int32_t)cx1, y0 = (int32_t)cy0, y1 = (int32_t)cy1;
    for (int32_t y = y0; y <= y1; ++y) {
        const double pv = (double)y;
        for (int32_t x = x0; x <= x1; ++x) {
            const double pu = (double)x;
            const double w0 = edge(p1.u, p1.v, p2.u, p2.v, pu, pv);
            const double w1 = edge(p2.u, p2.v, p0.u, p0.v, pu, pv);
            const double w2 = edge(p0.u, p0.v, p1.u, p1.v, pu, pv);
            const bool inside = area > 0.0 ? (w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0) : (w0 <= 0.0 && w1 <= 0.0 && w2 <= 0.0);
            if (!inside) continue;
            const double s = (w0 + w1) + w2;
            if (s == 0.0) continue;
            const double zz = ((w0 * p0.z + w1 * p1.z) + w2 * p2.z) / s;
            const double zi = floor(zz + 0.5);
            if (!(zi >= 1.0 && zi <= 65535.0)) continue;
            atomicMin(zbuf + ((int64_t)y * wc + x), (uint32_t)zi);
        }
    }
}

static __global__ __launch_bounds__(kWarpThreads) void warp_raster_kernel(const uint16_t *__restrict__ depth, const float *__restrict__ xy, int32_t w,
                                                                          int32_t h, int32_t tiles_x, int32_t wc, int32_t hc, CalibrationPack pack,
                                                                          int32_t n_cal, double max_gap_mm, uint32_t *__restrict__ zbuf)
{
    __shared__ WarpVertex vert[kWarpVerts];
    const int frame = blockIdx.y, cal_id = frame % n_cal;
    const ColorCalibration &cal = pack.c[cal_id];
    const int64_t n_px = (int64_t)w * h;
    const uint16_t *dp = depth + (int64_t)frame * n_px;
    const float *tp = xy + (int64_t)cal_id * n_px * 2;
    const int32_t c0 = (int32_t)(blockIdx.x % (uint32_t)tiles_x) * kWarpTileW, r0 = (int32_t)(blockIdx.x / (uint32_t)tiles_x) * kWarpTileH;
    for (int i = threadIdx.x; i < kWarpVerts; i += kWarpThreads) {
        const int32_t c = c0 + i % kWarpVertW, r = r0 + i / kWarpVertW;
        WarpVertex o{ 0.0, 0.0, 0.0 };
        if (c < w && r < h) {
            const int64_t p = (int64_t)r * w + c;
            double u, v, z;
            if (depth_pixel_to_color(cal, dp[p], tp[2 * p], tp[2 * p + 1], u, v, z)) o = WarpVertex{ u, v, z };       // (element loads: no alignment)
        }
        vert[i] = o;
    }
    __syncthreads();
    const int32_t lc = threadIdx.x % kWarpTileW, lr = threadIdx.x / kWarpTileW;
    if (c0 + lc >= w - 1 || r0 + lr >= h - 1) return;
    const WarpVertex p00 = vert[lr * kWarpVertW + lc], p10 = vert[lr * kWarpVertW + lc + 1];
    const WarpVertex p01 = vert[(lr + 1) * kWarpVertW + lc], p11 = vert[(lr + 1) * kWarpVertW + lc + 1];
    uint32_t *zb = zbuf + (int64_t)frame * hc * wc;
    raster_triangle(p00, p10, p01, max_gap_mm, wc, hc, zb);
    raster_triangle(p11, p01, p10, max_gap_mm, wc, hc, zb);
}

// Resolve: a block owns kResolvePerBlock consecutive colour pixels of one frame.  Their u16 values (0 for an untouched pixel) are laid
// down in LDS at the offset the block's output has inside its 16-byte line, so that whole 16-byte vectors of LDS are whole aligned
// vectors of the output; the elements in front of the first and behind the last whole vector leave as element stores (a frame's
// output starts wherever frames * color_height * color_width * 2 puts it; neighbouring blocks may share a line, never an element).
constexpr int kResolveThreads = 256, kResolvePerBlock = 2048;

static __global__ __launch_bounds__(kResolveThreads) void warp_resolve_kernel(const uint32_t *__restrict__ zbuf, int64_t n, int32_t vec_ok,
                                                                              uint16_t *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint16_t stage[kResolvePerBlock + 8];
    const int64_t p0 = (int64_t)blockIdx.x * kResolvePerBlock;
    const int64_t left = n - p0;
    const int cnt = (int)(left < kResolvePerBlock ? left : kResolvePerBlock);
    const uint32_t *zb = zbuf + (int64_t)blockIdx.y * n + p0;
    uint16_t *out_blk = out + (int64_t)blockIdx.y * n + p0;
    if (!vec_ok) {                                                             // an output off its 2-byte boundary
        for (int i = threadIdx.x; i < cnt; i += kResolveThreads) {
            const uint32_t z = zb[i];
            out_blk[i] = z == kWarpEmpty ? (uint16_t)0 : (uint16_t)z;
        }
        return;
    }
    const int a = (int)(((uintptr_t)out_blk & 15) >> 1);                       // the block's first element inside its 16-byte line
    for (int i = threadIdx.x; i < cnt; i += kResolveThreads) {
        const uint32_t z = zb[i];
        stage[a + i] = z == kWarpEmpty ? (uint16_t)0 : (uint16_t)z;
    }
    __syncthreads();
    const int v0 = (a + 7) >> 3, v1 = (a + cnt) >> 3;                          // whole vectors: stage[8 v0 .. 8 v1)
    if (v1 <= v0) {
        for (int i = threadIdx.x; i < cnt; i += kResolveThreads) out_blk[i] = stage[a + i];
        return;
    }
    const int head = 8 * v0 - a, tail0 = 8 * v1 - a;                           // elements [0, head) and [tail0, cnt) leave one by one
    if ((int)threadIdx.x < head) out_blk[threadIdx.x] = stage[a + threadIdx.x];
    if ((int)threadIdx.x < cnt - tail0) out_blk[tail0 + threadIdx.x] = stage[a + tail0 + threadIdx.x];
    const uint4 *src = reinterpret_cast<const uint4 *>(stage);
    uint4 *dst = reinterpret_cast<uint4 *>(out_blk - a);
    for (int j = v0 + threadIdx.x; j < v1; j += kResolveThreads) dst[j] = src[j];
}

// ---- lens undistortion (AC22) ---------------------------------------------------------------------------------------------------------
struct Pinhole {
    double fx, fy, cx, cy;
};

// One thread per pixel of the target camera, closed form (the lens model runs in its forward direction): a thread's (u, v) is one
// 8-byte store, a wave's 512 contiguous bytes.
static __global__ __launch_bounds__(kTableThreads) void undistort_map_kernel(Camera k, Pinhole t, int32_t width, int64_t n_px, float2 *__restrict__ map)
{
    const int64_t i = (int64_t)blockIdx.x * kTableThreads + threadIdx.x;
    if (i >= n_px) return;
    const int64_t row = i / width;
    const double x = ((double)(i - row * width) - t.cx) / t.fx, y = ((double)row - t.cy) / t.fy;
    const Distorted o = distort(k, x, y);
    const double u = k.fx * o.xd + k.cx, v = k.fy * o.yd + k.cy;
    const float nan = __builtin_nanf("");
    float2 e = make_float2(nan, nan);
    if (!(o.r2 > k.mr * k.mr) && __builtin_isfinite(u) && __builtin_isfinite(v)) e = make_float2((float)u, (float)v);
    map[i] = e;
}

// the map entries of a thread's four consecutive output pixels from i0 on (0, 0 behind the last pixel: never stored).  vec_ok: n_px is
// a multiple of 4 and the map's base is 16-byte aligned, so every map's group of 4 entries is two aligned 16-byte loads
__device__ __forceinline__ void load_map4(const float *__restrict__ mp, int64_t i0, int64_t n_px, int32_t vec_ok, float u[kC2dPerThread], float v[kC2dPerThread])
{
    if (vec_ok && i0 + kC2dPerThread <= n_px) {
        const float4 t0 = *reinterpret_cast<const float4 *>(mp + 2 * i0), t1 = *reinterpret_cast<const float4 *>(mp + 2 * i0 + 4);
        u[0] = t0.x; v[0] = t0.y; u[1] = t0.z; v[1] = t0.w; u[2] = t1.x; v[2] = t1.y; u[3] = t1.z; v[3] = t1.w;
    } else {
#pragma unroll
        for (int k = 0; k < kC2dPerThread; ++k) {
            const bool in = i0 + k < n_px;
            u[k] = in ? mp[2 * (i0 + k)] : 0.0f;
            v[k] = in ? mp[2 * (i0 + k) + 1] : 0.0f;
        }
    }
}

// color_to_depth_kernel's shape: a block owns kPixPerBlock consecutive output pixels of one frame (blockIdx.y), four per thread, and
// stores them with store_packed.  A NaN map entry fails the samplers' range tests and leaves the pixel zero.
template <int C, int INTERP>
static __global__ __launch_bounds__(kC2dThreads) void remap_u8_kernel(const uint8_t *__restrict__ src, const float *__restrict__ map, int32_t ws, int32_t hs,
                                                                      int64_t n_px, int32_t n_maps, int32_t vec_ok, uint8_t *__restrict__ out)
{
    constexpr int kStageWords = kPixPerBlock * C / 4;
    __shared__ uint32_t stage[kStageWords + 8];
    const int frame = blockIdx.y;
    const int64_t p0 = (int64_t)blockIdx.x * kPixPerBlock;
    const int64_t i0 = p0 + (int64_t)threadIdx.x * kC2dPerThread;
    const uint8_t *img = src + (int64_t)frame * hs * ws * C;
    float u[kC2dPerThread], v[kC2dPerThread];
    load_map4(map + (int64_t)(frame % n_maps) * n_px * 2, i0, n_px, vec_ok, u, v);
    uint32_t px[kC2dPerThread][C];
#pragma unroll
    for (int k = 0; k < kC2dPerThread; ++k) {
#pragma unroll
        for (int ch = 0; ch < C; ++ch) px[k][ch] = 0;
        if (i0 + k < n_px) sample_at<C, INTERP, false>(img, nullptr, 0.0, ws, hs, (double)u[k], (double)v[k], 0.0, px[k]);
    }
    const int64_t left = n_px - p0;
    const int nbytes = (int)(left < kPixPerBlock ? left : kPixPerBlock) * C;
    store_packed<C>(px, stage, out + ((int64_t)frame * n_px + p0) * C, nbytes);
}

template <int INTERP>
__device__ __forceinline__ uint32_t sample_depth_at(const uint16_t *__restrict__ img, int32_t ws, int32_t hs, double uc, double vc, double max_gap_mm)
{
    if (INTERP == KPX_SAMPLE_NEAREST) {
        const double fx = floor(uc + 0.5), fy = floor(vc + 0.5);
        if (!(fx >= 0.0 && fx <= (double)(ws - 1) && fy >= 0.0 && fy <= (double)(hs - 1))) return 0;
        return img[(int64_t)(int32_t)fy * ws + (int32_t)fx];
    }
    const double x0 = floor(uc), y0 = floor(vc);
    if (!(x0 >= 0.0 && x0 <= (double)(ws - 2) && y0 >= 0.0 && y0 <= (double)(hs - 2))) return 0;
    const uint16_t *p0 = img + ((int64_t)(int32_t)y0 * ws + (int32_t)x0);
    const uint16_t *p1 = p0 + ws;
    const uint32_t d00 = p0[0], d10 = p0[1], d01 = p1[0], d11 = p1[1];
    if (d00 == 0 || d10 == 0 || d01 == 0 || d11 == 0) return 0;
    const uint32_t lo = min(min(d00, d10), min(d01, d11)), hi = max(max(d00, d10), max(d01, d11));
    if ((double)(hi - lo) > max_gap_mm) return 0;
    const double ax = uc - x0, ay = vc - y0;
    const double bx = 1.0 - ax, by = 1.0 - ay;
    const double w00 = bx * by, w10 = ax * by, w01 = bx * ay, w11 = ax * ay;
    const double val = ((w00 * (double)d00 + w10 * (double)d10) + w01 * (double)d01) + w11 * (double)d11;
    return (uint32_t)(int32_t)floor(val + 0.5);
}

// Four consecutive output pixels per thread, one frame per blockIdx.y.  vec_out: n_px is a multiple of 4 and out's base is 8-byte
// aligned, so a thread's four u16 values are one aligned 8-byte store (a wave's 512 contiguous bytes); element stores otherwise.
template <int INTERP>
static __global__ __launch_bounds__(kC2dThreads) void remap_depth_kernel(const uint16_t *__restrict__ src, const float *__restrict__ map, int32_t ws,
                                                                         int32_t hs, int64_t n_px, int32_t n_maps, int32_t vec_ok, int32_t vec_out,
                                                                         double max_gap_mm, uint16_t *__restrict__ out)
{
    const int frame = blockIdx.y;
    const int64_t i0 = ((int64_t)blockIdx.x * kC2dThreads + threadIdx.x) * kC2dPerThread;
    if (i0 >= n_px) return;
    const uint16_t *img = src + (int64_t)frame * hs * ws;
    float u[kC2dPerThread], v[kC2dPerThread];
    load_map4(map + (int64_t)(frame % n_maps) * n_px * 2, i0, n_px, vec_ok, u, v);
    uint32_t d[kC2dPerThread];
#pragma unroll
    for (int k = 0; k < kC2dPerThread; ++k)
        d[k] = i0 + k < n_px ? sample_depth_at<INTERP>(img, ws, hs, (double)u[k], (double)v[k], max_gap_mm) : 0u;
    uint16_t *o = out + (int64_t)frame * n_px + i0;
    if (vec_out) {                                                             // (then i0 + 4 <= n_px)
        *reinterpret_cast<uint2 *>(o) = make_uint2(d[0] | d[1] << 16, d[2] | d[3] << 16);
    } else {
#pragma unroll
        for (int k = 0; k < kC2dPerThread; ++k)
            if (i0 + k < n_px) o[k] = (uint16_t)d[k];
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


// the checks the three batched entries share: false = kpx::fail() has been called
static bool calibrations_ok(const char *who, int32_t frames, const double *h_calibrations, int32_t calibrations)
{
    if (frames > 65535) return fail(KPX_ERR_INVALID, "%s: at most 65535 frames per call, got %d", who, (int)frames), false;
    if (!(calibrations >= 1 && calibrations <= KPX_SENSOR_MAX_CALIBRATIONS))
        return fail(KPX_ERR_INVALID, "%s: 1 to %d calibrations, got %d", who, KPX_SENSOR_MAX_CALIBRATIONS, (int)calibrations), false;
    if (frames % calibrations != 0) return fail(KPX_ERR_INVALID, "%s: %d calibrations do not divide %d frames", who, (int)calibrations, (int)frames), false;
    if (!h_calibrations) return fail(KPX_ERR_INVALID, "%s: null calibrations", who), false;
    for (int s = 0; s < calibrations; ++s) {
        const double *h = h_calibrations + (size_t)s * KPX_CALIBRATION_DOUBLES;
        bool ok = camera_ok(h);
        for (int i = 0; i < 12; ++i) ok = ok && __builtin_isfinite(h[KPX_CAMERA_DOUBLES + i]);
        if (!ok) return fail(KPX_ERR_INVALID, "%s: calibration %d needs finite numbers, non-zero focal lengths and a positive metric radius", who, s), false;
    }
    return true;
}

static CalibrationPack pack_of(const double *h_calibrations, int32_t calibrations)
{
    CalibrationPack pack;
    memset(&pack, 0, sizeof pack);
    for (int s = 0; s < calibrations; ++s) {
        const double *h = h_calibrations + (size_t)s * KPX_CALIBRATION_DOUBLES;
        pack.c[s].cam = camera_from(h);
        memcpy(pack.c[s].T, h + KPX_CAMERA_DOUBLES, sizeof pack.c[s].T);
    }
    return pack;
}

template <bool VISIBLE>
static int color_to_depth(const char *who, const uint16_t *depth, const float *xy, const uint8_t *color, int64_t n_px, int32_t frames, int32_t color_width,
                          int32_t color_height, int32_t channels, const double *h_calibrations, int32_t calibrations, int32_t interpolation,
                          const uint16_t *warped, double occlusion_mm, uint8_t *out, void *stream)
{
    KPX_REQUIRE(n_px >= 0 && frames >= 0, "%s: negative size (n_px %lld, frames %d)", who, (long long)n_px, (int)frames);
    KPX_REQUIRE(frames <= 65535, "%s: at most 65535 frames per call, got %d", who, (int)frames);
    KPX_REQUIRE(n_px <= (int64_t)kPixPerBlock * 0x7fffffff, "%s: n_px %lld is out of range", who, (long long)n_px);
    KPX_REQUIRE(channels == 1 || channels == 3, "%s: channels must be 1 or 3, got %d", who, (int)channels);
    KPX_REQUIRE(interpolation == KPX_SAMPLE_NEAREST || interpolation == KPX_SAMPLE_BILINEAR, "%s: unknown interpolation %d", who, (int)interpolation);
    KPX_REQUIRE(color_width >= 1 && color_height >= 1, "%s: colour image size %d x %d", who, (int)color_width, (int)color_height);
    if (!calibrations_ok(who, frames, h_calibrations, calibrations)) return KPX_ERR_INVALID;
    KPX_REQUIRE(!VISIBLE || occlusion_mm >= 0.0, "%s: occlusion_mm must be >= 0 (+inf: never occluded), got %g", who, occlusion_mm);      // (a NaN fails)
    if (frames == 0 || n_px == 0) return KPX_OK;
    KPX_REQUIRE(depth && xy && color && out && (!VISIBLE || warped), "%s: null pointer", who);
    const CalibrationPack pack = pack_of(h_calibrations, calibrations);
    const int32_t vec_ok = n_px % 4 == 0 && (uintptr_t)depth % 16 == 0 && (uintptr_t)xy % 16 == 0;
    const dim3 grid((unsigned)cdiv(n_px, kPixPerBlock), (unsigned)frames), block(kC2dThreads);
    hipStream_t st = (hipStream_t)stream;
#define KPX_C2D(C, I)                                                                                                                               \
    hipLaunchKernelGGL((color_to_depth_kernel<C, I, VISIBLE>), grid, block, 0, st, depth, xy, color, warped, occlusion_mm, n_px, color_width, color_height, \
                       pack, calibrations, vec_ok, out)
    if (channels == 3 && interpolation == KPX_SAMPLE_BILINEAR) KPX_C2D(3, KPX_SAMPLE_BILINEAR);
    else if (channels == 3) KPX_C2D(3, KPX_SAMPLE_NEAREST);
    else if (interpolation == KPX_SAMPLE_BILINEAR) KPX_C2D(1, KPX_SAMPLE_BILINEAR);
    else KPX_C2D(1, KPX_SAMPLE_NEAREST);
#undef KPX_C2D
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT int kpx_color_to_depth(const uint16_t *depth, const float *xy, const uint8_t *color, int64_t n_px, int32_t frames, int32_t color_width,
                                  int32_t color_height, int32_t channels, const double *h_calibrations, int32_t calibrations, int32_t interpolation,
                                  uint8_t *out, void *stream)
{
    return color_to_depth<false>("kpx_color_to_depth", depth, xy, color, n_px, frames, color_width, color_height, channels, h_calibrations, calibrations,
                                 interpolation, nullptr, 0.0, out, stream);
}

KPX_EXPORT int kpx_color_to_depth_visible(const uint16_t *depth, const float *xy, const uint8_t *color, int64_t n_px, int32_t frames, int32_t color_width,
                                          int32_t color_height, int32_t channels, const double *h_calibrations, int32_t calibrations,
                                          int32_t interpolation, const uint16_t *warped, double occlusion_mm, uint8_t *out, void *stream)
{
    return color_to_depth<true>("kpx_color_to_depth_visible", depth, xy, color, n_px, frames, color_width, color_height, channels, h_calibrations,
                                calibrations, interpolation, warped, occlusion_mm, out, stream);
}

KPX_EXPORT size_t kpx_depth_to_color_workspace_bytes(int32_t frames, int32_t color_width, int32_t color_height)
{
    if (frames <= 0 || color_width <= 0 || color_height <= 0) return 0;
    return (size_t)frames * (size_t)color_height * (size_t)color_width * sizeof(uint32_t);
}

KPX_EXPORT int kpx_depth_to_color(const uint16_t *depth, const float *xy, int32_t depth_width, int32_t depth_height, int32_t frames, int32_t color_width,
                                  int32_t color_height, const double *h_calibrations, int32_t calibrations, double max_gap_mm, uint16_t *out, void *ws,
                                  size_t ws_bytes, void *stream)
{
    const char *who = "kpx_depth_to_color";
    KPX_REQUIRE(depth_width >= 0 && depth_height >= 0 && frames >= 0 && color_width >= 0 && color_height >= 0,
                "%s: negative size (depth %d x %d, colour %d x %d, frames %d)", who, (int)depth_width, (int)depth_height, (int)color_width, (int)color_height,
                (int)frames);
    if (!calibrations_ok(who, frames, h_calibrations, calibrations)) return KPX_ERR_INVALID;
    KPX_REQUIRE(max_gap_mm >= 0.0, "%s: max_gap_mm must be >= 0 (+inf: never too far apart), got %g", who, max_gap_mm);                    // (a NaN fails)
    const int64_t n = (int64_t)color_width * color_height;                     // colour pixels of a frame
    const int64_t tiles_x = cdiv((int64_t)depth_width - 1, kWarpTileW), tiles_y = cdiv((int64_t)depth_height - 1, kWarpTileH);
    KPX_REQUIRE(n <= (int64_t)kResolvePerBlock * 0x7fffffff && tiles_x * tiles_y <= 0x7fffffff, "%s: image size out of range", who);
    const size_t need = kpx_depth_to_color_workspace_bytes(frames, color_width, color_height);
    if (ws_bytes < need) return fail(KPX_ERR_WORKSPACE, "%s: workspace too small: need %zu bytes, have %zu", who, need, ws_bytes);
    if (frames == 0 || n == 0) return KPX_OK;
    KPX_REQUIRE(out && ws, "%s: null pointer", who);
    hipStream_t st = (hipStream_t)stream;
    if (depth_width < 2 || depth_height < 2) {                                 // no triangle: every pixel is untouched
        KPX_HIP(hipMemsetAsync(out, 0, (size_t)frames * n * sizeof(uint16_t), st));
        return KPX_OK;
    }
    KPX_REQUIRE(depth && xy, "%s: null pointer", who);
    uint32_t *zbuf = static_cast<uint32_t *>(ws);
    KPX_HIP(hipMemsetAsync(zbuf, 0xFF, need, st));                             // kWarpEmpty everywhere
    hipLaunchKernelGGL(warp_raster_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)frames), dim3(kWarpThreads), 0, st, depth, xy, depth_width,
                       depth_height, (int32_t)tiles_x, color_width, color_height, pack_of(h_calibrations, calibrations), calibrations, max_gap_mm, zbuf);
    KPX_LAUNCH_CHECK();
    const int32_t vec_ok = (uintptr_t)out % 2 == 0;
    hipLaunchKernelGGL(warp_resolve_kernel, dim3((unsigned)cdiv(n, kResolvePerBlock), (unsigned)frames), dim3(kResolveThreads), 0, st, zbuf, n, vec_ok, out);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

// ---- lens undistortion (AC22) ---------------------------------------------------------------------------------------------------------
KPX_EXPORT int kpx_undistort_map(const double *h_camera, const double *h_pinhole, int32_t out_width, int32_t out_height, float *map, void *stream)
{
    const char *who = "kpx_undistort_map";
    KPX_REQUIRE(out_width >= 0 && out_height >= 0, "%s: negative image size %d x %d", who, (int)out_width, (int)out_height);
    KPX_REQUIRE(h_camera, "%s: null camera", who);
    KPX_REQUIRE(h_pinhole, "%s: null pinhole", who);
    KPX_REQUIRE(camera_ok(h_camera), "%s: the camera needs finite numbers, non-zero focal lengths and a positive metric radius", who);
    bool ok = h_pinhole[0] != 0.0 && h_pinhole[1] != 0.0;
    for (int i = 0; i < 4; ++i) ok = ok && __builtin_isfinite(h_pinhole[i]);
    KPX_REQUIRE(ok, "%s: the pinhole target needs finite numbers and non-zero focal lengths", who);
    const int64_t n_px = (int64_t)out_width * out_height;
    if (n_px == 0) return KPX_OK;
    KPX_REQUIRE(map, "%s: null pointer", who);
    hipLaunchKernelGGL(undistort_map_kernel, dim3((unsigned)cdiv(n_px, kTableThreads)), dim3(kTableThreads), 0, (hipStream_t)stream, camera_from(h_camera),
                       Pinhole{ h_pinhole[0], h_pinhole[1], h_pinhole[2], h_pinhole[3] }, out_width, n_px, reinterpret_cast<float2 *>(map));
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

// the checks the two remap entries share: false = kpx::fail() has been called
static bool remap_ok(const char *who, int32_t src_width, int32_t src_height, int32_t out_width, int32_t out_height, int32_t frames, int32_t maps,
                     int32_t interpolation)
{
    if (src_width < 0 || src_height < 0 || out_width < 0 || out_height < 0 || frames < 0)
        return fail(KPX_ERR_INVALID, "%s: negative size (source %d x %d, output %d x %d, frames %d)", who, (int)src_width, (int)src_height, (int)out_width,
                    (int)out_height, (int)frames), false;
    if (frames > 65535) return fail(KPX_ERR_INVALID, "%s: at most 65535 frames per call, got %d", who, (int)frames), false;
    if ((int64_t)out_width * out_height > (int64_t)kPixPerBlock * 0x7fffffff) return fail(KPX_ERR_INVALID, "%s: output size out of range", who), false;
    if (interpolation != KPX_SAMPLE_NEAREST && interpolation != KPX_SAMPLE_BILINEAR)
        return fail(KPX_ERR_INVALID, "%s: unknown interpolation %d", who, (int)interpolation), false;
    if (!(maps >= 1 && maps <= KPX_SENSOR_MAX_CALIBRATIONS)) return fail(KPX_ERR_INVALID, "%s: 1 to %d maps, got %d", who, KPX_SENSOR_MAX_CALIBRATIONS, (int)maps), false;
    if (frames % maps != 0) return fail(KPX_ERR_INVALID, "%s: %d maps do not divide %d frames", who, (int)maps, (int)frames), false;
    return true;
}

KPX_EXPORT int kpx_remap_u8(const uint8_t *src, const float *map, int32_t src_width, int32_t src_height, int32_t channels, int32_t out_width,
                            int32_t out_height, int32_t frames, int32_t maps, int32_t interpolation, uint8_t *out, void *stream)
{
    const char *who = "kpx_remap_u8";
    if (!remap_ok(who, src_width, src_height, out_width, out_height, frames, maps, interpolation)) return KPX_ERR_INVALID;
    KPX_REQUIRE(channels == 1 || channels == 3, "%s: channels must be 1 or 3, got %d", who, (int)channels);
    const int64_t n_px = (int64_t)out_width * out_height;
    if (frames == 0 || n_px == 0) return KPX_OK;
    KPX_REQUIRE(out, "%s: null pointer", who);
    hipStream_t st = (hipStream_t)stream;
    if (src_width == 0 || src_height == 0) {                                   // no source pixel: every sample lies outside
        KPX_HIP(hipMemsetAsync(out, 0, (size_t)frames * n_px * channels, st));
        return KPX_OK;
    }
    KPX_REQUIRE(src && map, "%s: null pointer", who);
    const int32_t vec_ok = n_px % 4 == 0 && (uintptr_t)map % 16 == 0;
    const dim3 grid((unsigned)cdiv(n_px, kPixPerBlock), (unsigned)frames), block(kC2dThreads);
#define KPX_REMAP(C, I) hipLaunchKernelGGL((remap_u8_kernel<C, I>), grid, block, 0, st, src, map, src_width, src_height, n_px, maps, vec_ok, out)
    if (channels == 3 && interpolation == KPX_SAMPLE_BILINEAR) KPX_REMAP(3, KPX_SAMPLE_BILINEAR);
    else if (channels == 3) KPX_REMAP(3, KPX_SAMPLE_NEAREST);
    else if (interpolation == KPX_SAMPLE_BILINEAR) KPX_REMAP(1, KPX_SAMPLE_BILINEAR);
    else KPX_REMAP(1, KPX_SAMPLE_NEAREST);
#undef KPX_REMAP
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT int kpx_remap_depth(const uint16_t *src, const float *map, int32_t src_width, int32_t src_height, int32_t out_width, int32_t out_height,
                               int32_t frames, int32_t maps, int32_t interpolation, double max_gap_mm, uint16_t *out, void *stream)
{
    const char *who = "kpx_remap_depth";
    if (!remap_ok(who, src_width, src_height, out_width, out_height, frames, maps, interpolation)) return KPX_ERR_INVALID;
    KPX_REQUIRE(max_gap_mm >= 0.0, "%s: max_gap_mm must be >= 0 (+inf: never too far apart), got %g", who, max_gap_mm);                   // (a NaN fails)
    const int64_t n_px = (int64_t)out_width * out_height;
    if (frames == 0 || n_px == 0) return KPX_OK;
    KPX_REQUIRE(out, "%s: null pointer", who);
    hipStream_t st = (hipStream_t)stream;
    if (src_width == 0 || src_height == 0) {
        KPX_HIP(hipMemsetAsync(out, 0, (size_t)frames * n_px * sizeof(uint16_t), st));
        return KPX_OK;
    }
    KPX_REQUIRE(src && map, "%s: null pointer", who);
    const int32_t vec_ok = n_px % 4 == 0 && (uintptr_t)map % 16 == 0, vec_out = n_px % 4 == 0 && (uintptr_t)out % 8 == 0;
    const dim3 grid((unsigned)cdiv(n_px, kPixPerBlock), (unsigned)frames), block(kC2dThreads);
    if (interpolation == KPX_SAMPLE_BILINEAR)
        hipLaunchKernelGGL(remap_depth_kernel<KPX_SAMPLE_BILINEAR>, grid, block, 0, st, src, map, src_width, src_height, n_px, maps, vec_ok, vec_out, max_gap_mm, out);
    else
        hipLaunchKernelGGL(remap_depth_kernel<KPX_SAMPLE_NEAREST>, grid, block, 0, st, src, map, src_width, src_height, n_px, maps, vec_ok, vec_out, max_gap_mm, out);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}
