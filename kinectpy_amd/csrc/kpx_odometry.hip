// kpx_odometry.hip -- image filters / pyramids and RGB-D odometry ([O3D] geometry.Image::Filter / CreatePyramid, pipelines.odometry;
// arithmetic contract AC11).
//
// The odometry of P pairs is ONE chain of launches on the caller's stream (pair = grid.y) without a host read-back: the pose, the
// failure flag and the sums live in device memory.  An iteration is two launches:
//   odo_corr_kernel    a thread per SOURCE pixel projects it into the target and bids for the target pixel with one 64-bit atomicMin
//                      on the key map: key = float32 bits of z' << 32 | source index -- the order of the keys IS AC11's tie rule
//   odo_gather_kernel  a thread per TARGET pixel decodes the winner, resets the key (no memset between iterations), forms its one or
//                      two rows and adds them up: a fixed shuffle tree per wave, the waves in order, the block's totals into its column
//                      of a slab.  The block that takes the last ticket adds the columns up in a fixed order -- so the sums are bitwise
//                      repeatable, at full fp64 precision whatever their magnitude (the photometric entries of a millimetre scene are
//                      ~1e-7: 128-bit fixed point with 64 fractional bits would keep 13 digits of them) -- solves the 6x6 and writes the
//                      new pose.
// Everything a decision depends on is fp64 from plain multiplies and adds in the order written here (-ffp-contract=off), so that
// tests/odometry_ref.py can restate it bit for bit.
#include "kpx_compact.h"
#include "kpx_linalg.h"

#include <math.h>

namespace kpx {
namespace {

constexpr int kOdoThreads = 256;
constexpr int kOdoWaves = kOdoThreads / 64;
constexpr int kSums = 28;                       // 21 (upper triangle of J^T J by rows) + 6 (J^T r) + 1 (r.r)
constexpr int kPlanes = 16;                     // per pair and level: 0 I_s 1 D_s 2 I_t 3 D_t 4 dI/dx 5 dI/dy 6 dD/dx 7 dD/dy, 8..15 scratch
constexpr unsigned long long kEmpty = ~0ull;
constexpr double kRankTol = 1e-12;              // the registration's singular rule (solve6_ldlt_ranked)
constexpr double kLambda = 0.968;               // [O3D] LAMBDA_HYBRID_DEPTH
constexpr double kSobelScale = 0.125;           // [O3D] SOBEL_SCALE
enum { kModeNormalise = 0, kModeColor = 1, kModeHybrid = 2, kModeInfo = 3 };

// ---- filters --------------------------------------------------------------------------------------------------------------------
enum { kTapGauss3 = 0, kTapGauss5 = 1, kTapGauss7 = 2, kTapDiff = 3, kTapSmooth = 4 };
__device__ const double kTaps[5][7] = {
    { 0.25, 0.5, 0.25, 0, 0, 0, 0 },
    { 0.0625, 0.25, 0.375, 0.25, 0.0625, 0, 0 },
    { 0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125 },
    { -1.0, 0.0, 1.0, 0, 0, 0, 0 },
    { 1.0, 2.0, 1.0, 0, 0, 0, 0 },
};
__device__ const int kTapCount[5] = { 3, 5, 7, 3, 3 };

constexpr int kMaxJobs = 4;
struct ImageJobs {
    const float *src[kMaxJobs];
    float *dst[kMaxJobs];
    int kind[kMaxJobs];
};

// one pass of a separable filter for up to kMaxJobs (source, destination, taps) jobs (grid.z) over `count` images (grid.y) that lie
// `stride` floats apart: taps beyond the border read the border pixel; fp64 accumulation in ascending tap order, one rounding
__global__ __launch_bounds__(kOdoThreads) void filter_pass_kernel(ImageJobs j, size_t stride, int W, int H, int horizontal)
{
    const int px = blockIdx.x * kOdoThreads + threadIdx.x;
    if (px >= W * H) return;
    const int job = blockIdx.z, kind = j.kind[job];
    const float *__restrict__ s = j.src[job] + (size_t)blockIdx.y * stride;
    float *__restrict__ d = j.dst[job] + (size_t)blockIdx.y * stride;
    const int y = px / W, x = px - y * W;
    const int nt = kTapCount[kind], half = nt >> 1;
    double acc = 0.0;
    for (int k = 0; k < nt; ++k) {
        int xx = x, yy = y;
        if (horizontal) { xx = x + k - half; xx = xx < 0 ? 0 : (xx > W - 1 ? W - 1 : xx); }
        else { yy = y + k - half; yy = yy < 0 ? 0 : (yy > H - 1 ? H - 1 : yy); }
        acc = acc + (double)s[(size_t)yy * W + xx] * kTaps[kind][k];
    }
    d[px] = (float)acc;
}

// 2 x 2 block mean in float32, (((a + b) + c) + d) / 4; W, H: the SOURCE size, sstride / dstride: floats between images
__global__ __launch_bounds__(kOdoThreads) void downsample_kernel(ImageJobs j, size_t sstride, size_t dstride, int W, int H)
{
    const int w2 = W >> 1, h2 = H >> 1;
    const int px = blockIdx.x * kOdoThreads + threadIdx.x;
    if (px >= w2 * h2) return;
    const int job = blockIdx.z;
    const float *__restrict__ s = j.src[job] + (size_t)blockIdx.y * sstride;
    float *__restrict__ d = j.dst[job] + (size_t)blockIdx.y * dstride;
    const int y = px / w2, x = px - y * w2;
    const float *r0 = s + (size_t)(2 * y) * W + 2 * x, *r1 = r0 + W;
    d[px] = (((r0[0] + r0[1]) + r1[0]) + r1[1]) / 4.0f;
}

int filter_pass(const ImageJobs &j, int njobs, int count, size_t stride, int W, int H, bool horizontal, hipStream_t st)
{
    hipLaunchKernelGGL(filter_pass_kernel, dim3((unsigned)cdiv((int64_t)W * H, kOdoThreads), count, njobs), dim3(kOdoThreads), 0, st, j, stride, W, H,
                       horizontal ? 1 : 0);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

// ---- odometry state ---------------------------------------------------------------------------------------------------------------
struct OdoState {                               // one per pair, zeroed at the start of every call
    double scale[2];                            // NormalizeIntensity's factors (source, target)
    unsigned ticket, count;
    int failed, pad;
};

struct OdoLevel {                               // pair p's images start p * stride floats further on
    const float *Is, *Ds, *It, *Dt, *dIx, *dIy, *dDx, *dDy;
    size_t stride;
    int W, H;
    double fx, fy, cx, cy;
};

// c = a b with c_ij = (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j
__device__ __forceinline__ void mat3_mul(const double a[9], const double b[9], double c[9])
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) c[3 * i + k] = (a[3 * i] * b[k] + a[3 * i + 1] * b[3 + k]) + a[3 * i + 2] * b[6 + k];
}

template <bool RAW>
__global__ __launch_bounds__(kOdoThreads) void odo_prepare_kernel(const void *ds, const void *cs, const void *dt, const void *ct, const uint8_t *ms,
                                                                  const uint8_t *mt, float scale, float trunc, double dmin, double dmax,
                                                                  float *planes, size_t stride, int npx)
{
    const int px = blockIdx.x * kOdoThreads + threadIdx.x;
    if (px >= npx) return;
    const int which = blockIdx.z;
    const size_t at = (size_t)blockIdx.y * npx + px;
    const void *dep = which ? dt : ds, *col = which ? ct : cs;
    const uint8_t *mask = which ? mt : ms;
    float d, I;
    if (RAW) {
        d = (float)((const uint16_t *)dep)[at] / scale;
        if (d > trunc) d = 0.0f;
        if (mask && mask[at]) d = 0.0f;
        const uint8_t *c = (const uint8_t *)col + 3 * at;
        I = ((0.2990f * (float)c[0] + 0.5870f * (float)c[1]) + 0.1140f * (float)c[2]) / 255.0f;
    } else {
        d = ((const float *)dep)[at];
        I = ((const float *)col)[at];
    }
    if ((double)d < dmin || (double)d > dmax || d <= 0.0f) d = __builtin_nanf("");
    float *p = planes + (size_t)blockIdx.y * stride;
    p[(size_t)(8 + 2 * which) * npx + px] = I;
    p[(size_t)(9 + 2 * which) * npx + px] = d;
}

__global__ __launch_bounds__(kOdoThreads) void odo_scale_kernel(float *planes, size_t stride, int npx, const OdoState *__restrict__ st)
{
    const int px = blockIdx.x * kOdoThreads + threadIdx.x;
    if (px >= npx) return;
    const int which = blockIdx.z;
    float *p = planes + (size_t)blockIdx.y * stride + (size_t)(2 * which) * npx + px;
    *p = (float)((double)*p * st[blockIdx.y].scale[which]);
}

// a thread per source pixel; pose: f64 [pairs][16]
__global__ __launch_bounds__(kOdoThreads) void odo_corr_kernel(OdoLevel L, const OdoState *__restrict__ st, const double *__restrict__ pose,
                                                               unsigned long long *__restrict__ keymap, size_t kstride, double diff_max)
{
    __shared__ double sM[12];
    const int pair = blockIdx.y;
    if (st[pair].failed) return;                        // (uniform: the flag was written by an earlier launch)
    if (threadIdx.x == 0) {
        const double *T = pose + 16 * (size_t)pair;
        const double K[9] = { L.fx, 0.0, L.cx, 0.0, L.fy, L.cy, 0.0, 0.0, 1.0 };
        const double Ki[9] = { 1.0 / L.fx, 0.0, -L.cx / L.fx, 0.0, 1.0 / L.fy, -L.cy / L.fy, 0.0, 0.0, 1.0 };
        const double R[9] = { T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10] };
        double A[9], M[9];
        mat3_mul(K, R, A);
        mat3_mul(A, Ki, M);
        for (int i = 0; i < 9; ++i) sM[i] = M[i];
        for (int i = 0; i < 3; ++i) sM[9 + i] = (K[3 * i] * T[3] + K[3 * i + 1] * T[7]) + K[3 * i + 2] * T[11];
    }
    __syncthreads();
    const int npx = L.W * L.H;
    const int px = blockIdx.x * kOdoThreads + threadIdx.x;
    if (px >= npx) return;
    const float df = L.Ds[(size_t)pair * L.stride + px];
    if (!isfinite(df)) return;
    const int vs = px / L.W, us = px - vs * L.W;
    const double d = (double)df, u = (double)us, v = (double)vs;
    const double qx = d * ((sM[0] * u + sM[1] * v) + sM[2]) + sM[9];
    const double qy = d * ((sM[3] * u + sM[4] * v) + sM[5]) + sM[10];
    const double qz = d * ((sM[6] * u + sM[7] * v) + sM[8]) + sM[11];
    if (!(qz > 0.0)) return;
    const double fu = qx / qz + 0.5, fv = qy / qz + 0.5;
    if (!(fu > -1.0 && fu < (double)L.W && fv > -1.0 && fv < (double)L.H)) return;      // (int) truncates: (-1, 0) lands on pixel 0
    const int ut = (int)fu, vt = (int)fv;
    const int tpx = vt * L.W + ut;
    const float dtf = L.Dt[(size_t)pair * L.stride + tpx];
    if (!isfinite(dtf)) return;
    if (!(fabs(qz - (double)dtf) <= diff_max)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint((float)qz) << 32) | (unsigned)px;
    atomicMin(&keymap[(size_t)pair * kstride + tpx], key);
}

// v += the upper triangle of (w J)^T (w J), (w J)^T (w r) and (w r)^2
__device__ __forceinline__ void add_row(double v[kSums], const double J[6], double r, double w)
{
    double Jw[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) Jw[i] = w * J[i];
    const double rw = w * r;
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int c = i; c < 6; ++c) v[k++] += Jw[i] * Jw[c];
#pragma unroll
    for (int i = 0; i < 6; ++i) v[21 + i] += Jw[i] * rw;
    v[27] += rw * rw;
}

__device__ __forceinline__ double grad(const float *__restrict__ g, size_t at)
{
    const float f = g[at];
    return isfinite(f) ? kSobelScale * (double)f : 0.0;
}

// a thread per target pixel.  slab: f64 [pairs][kSums][slab_blocks], column b = the totals of block b (every block of a launch writes
// its column, so nothing is cleared).  results: f64 [pairs][KPX_ODOMETRY_RESULT_DOUBLES] (kModeInfo); dbg: f64 [KPX_ODOMETRY_ITERATION_DOUBLES]
// of pair 0 or null (the iteration modes)
template <int MODE>
__global__ __launch_bounds__(kOdoThreads) void odo_gather_kernel(OdoLevel L, OdoState *__restrict__ st, double *__restrict__ pose,
                                                                 unsigned long long *__restrict__ keymap, size_t kstride, double *slab, int slab_blocks,
                                                                 double *__restrict__ results, double *__restrict__ dbg)
{
    constexpr int NS = MODE == kModeNormalise ? 2 : (MODE == kModeInfo ? 21 : kSums);
    __shared__ double part[kOdoWaves][kSums];
    __shared__ unsigned cnt[kOdoWaves];
    __shared__ double tot[kSums];
    __shared__ int last;
    const int pair = blockIdx.y;
    OdoState &S = st[pair];
    const size_t img = (size_t)pair * L.stride;
    const int npx = L.W * L.H;
    const int tpx = blockIdx.x * kOdoThreads + threadIdx.x;
    double v[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) v[k] = 0.0;
    unsigned c = 0;
    unsigned long long key = kEmpty;
    if (tpx < npx) {
        key = keymap[(size_t)pair * kstride + tpx];
        if (key != kEmpty) keymap[(size_t)pair * kstride + tpx] = kEmpty;
    }
    if (key != kEmpty) {
        c = 1;
        const int spx = (int)(unsigned)(key & 0xFFFFFFFFull);
        if (MODE == kModeNormalise) {
            v[0] = (double)L.Is[img + spx];
            v[1] = (double)L.It[img + tpx];
        } else if (MODE == kModeInfo) {
            const int vt = tpx / L.W, ut = tpx - vt * L.W;
            const double z = (double)L.Dt[img + tpx];
            const double x = (((double)ut - L.cx) * z) / L.fx, y = (((double)vt - L.cy) * z) / L.fy;
            const double G0[6] = { 0.0, z, -y, 1.0, 0.0, 0.0 }, G1[6] = { -z, 0.0, x, 0.0, 1.0, 0.0 }, G2[6] = { y, -x, 0.0, 0.0, 0.0, 1.0 };
            add_row(v, G0, 0.0, 1.0);
            add_row(v, G1, 0.0, 1.0);
            add_row(v, G2, 0.0, 1.0);
        } else {
            const double *T = pose + 16 * (size_t)pair;
            const int vs = spx / L.W, us = spx - vs * L.W;
            const double z = (double)L.Ds[img + spx];
            const double x = (((double)us - L.cx) * z) / L.fx, y = (((double)vs - L.cy) * z) / L.fy;
            const double p0 = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
            const double p1 = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
            const double p2 = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
            const double invz = 1.0 / p2;
            const double c0 = (grad(L.dIx, img + tpx) * L.fx) * invz, c1 = (grad(L.dIy, img + tpx) * L.fy) * invz;
            const double c2 = (-(c0 * p0 + c1 * p1)) * invz;
            const double rp = (double)L.It[img + tpx] - (double)L.Is[img + spx];
            const double Jp[6] = { -p2 * c1 + p1 * c2, p2 * c0 - p0 * c2, -p1 * c0 + p0 * c1, c0, c1, c2 };
            if (MODE == kModeColor) {
                add_row(v, Jp, rp, 1.0);
            } else {
                const double d0 = (grad(L.dDx, img + tpx) * L.fx) * invz, d1 = (grad(L.dDy, img + tpx) * L.fy) * invz;
                const double d2 = (-(d0 * p0 + d1 * p1)) * invz;
                const double rg = (double)L.Dt[img + tpx] - p2;
                const double Jg[6] = { (-p2 * d1 + p1 * d2) - p1, (p2 * d0 - p0 * d2) + p0, -p1 * d0 + p0 * d1, d0, d1, d2 - 1.0 };
                add_row(v, Jp, rp, sqrt(1.0 - kLambda));
                add_row(v, Jg, rg, sqrt(kLambda));
            }
        }
    }
    // the block's totals: shuffle tree, then the waves in order
    const int wave = wave_id(), lane = lane_id();
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const double s = wave_sum(v[k]);
        if (lane == 0) part[wave][k] = s;
    }
    const unsigned cw = wave_sum(c);
    if (lane == 0) cnt[wave] = cw;
    __syncthreads();
    double *col = slab + (size_t)pair * kSums * slab_blocks;
    if (threadIdx.x < NS) {
        const int k = threadIdx.x;
        // (a device-scope store: written through to where every other compute die reads it)
        __hip_atomic_store(&col[(size_t)k * slab_blocks + blockIdx.x], ((part[0][k] + part[1][k]) + part[2][k]) + part[3][k], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
    if (threadIdx.x == 0) {
        const unsigned cb = ((cnt[0] + cnt[1]) + cnt[2]) + cnt[3];
        if (cb) atomicAdd(&S.count, cb);
    }
    // hand-off to the block of the last ticket: every wave drains its stores, the block meets, one lane releases and takes the ticket
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(&S.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = t == gridDim.x - 1 ? 1 : 0;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!last) return;
    // behind lane 0's acquire and the barrier: the columns in a fixed order -- thread t takes blocks t, t + 256, ..., then the tree again
    const int nblocks = (int)gridDim.x;
#pragma unroll 1
    for (int k = 0; k < NS; ++k) {
        double a = 0.0;
        for (int b = threadIdx.x; b < nblocks; b += kOdoThreads)
            a += __hip_atomic_load(&col[(size_t)k * slab_blocks + b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a = wave_sum(a);
        if (lane == 0) part[wave][k] = a;
    }
    __syncthreads();
    if (threadIdx.x < NS) tot[threadIdx.x] = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
    __syncthreads();
    if (threadIdx.x != 0) return;
    const unsigned count = __hip_atomic_exchange(&S.count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bool bad = false;
    for (int k = 0; k < NS; ++k) bad = bad || !isfinite(tot[k]);
    __hip_atomic_store(&S.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    double *T = pose + 16 * (size_t)pair;
    if (MODE == kModeNormalise) {
        double ss = 1.0, stt = 1.0;
        if (count > 0 && !bad) {
            const double ms = tot[0] / (double)count, mt = tot[1] / (double)count;
            if (ms > 0.0 && mt > 0.0) { ss = 0.5 / ms; stt = 0.5 / mt; }
        }
        S.scale[0] = ss;
        S.scale[1] = stt;
        return;
    }
    if (MODE == kModeInfo) {
        double *out = results + (size_t)KPX_ODOMETRY_RESULT_DOUBLES * pair;
        const bool ok = !S.failed && !bad;
        out[0] = ok ? 1.0 : 0.0;
        out[1] = ok ? (double)count : 0.0;
        for (int i = 0; i < 16; ++i) out[2 + i] = ok ? T[i] : (i % 5 == 0 ? 1.0 : 0.0);
        int k = 0;
        for (int i = 0; i < 6; ++i)
            for (int cidx = i; cidx < 6; ++cidx) {
                const double a = ok ? tot[k] : (i == cidx ? 1.0 : 0.0);
                ++k;
                out[18 + 6 * i + cidx] = a;
                out[18 + 6 * cidx + i] = a;
            }
        return;
    }
    int solved = 0;
    if (!S.failed) {
        if (count == 0 || bad) {
            S.failed = 1;
        } else {
            double A[36], b[6], x[6], U[16], Tn[12];
            int k = 0;
            for (int i = 0; i < 6; ++i)
                for (int cidx = i; cidx < 6; ++cidx) { A[6 * i + cidx] = tot[k]; A[6 * cidx + i] = tot[k]; ++k; }
            for (int i = 0; i < 6; ++i) b[i] = -tot[21 + i];
            if (!solve6_ldlt_ranked(A, b, x, kRankTol)) {
                S.failed = 1;
            } else {
                euler_update(x, U);
                for (int i = 0; i < 3; ++i)
                    for (int cidx = 0; cidx < 4; ++cidx) {
                        double a = (U[4 * i] * T[cidx] + U[4 * i + 1] * T[4 + cidx]) + U[4 * i + 2] * T[8 + cidx];
                        if (cidx == 3) a = a + U[4 * i + 3];
                        Tn[4 * i + cidx] = a;
                    }
                for (int i = 0; i < 12; ++i) T[i] = Tn[i];
                solved = 1;
            }
        }
    }
    if (dbg) {
        for (int i = 0; i < kSums; ++i) dbg[i] = tot[i];
        dbg[28] = (double)count;
        dbg[29] = (double)solved;
        for (int i = 0; i < 16; ++i) dbg[30 + i] = T[i];
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
struct OdoWs {
    OdoState *state;
    double *pose;
    unsigned long long *keymap;
    double *slab;
    int slab_blocks;
    float *planes[KPX_ODOMETRY_MAX_LEVELS];
    int32_t *counts;
    int W[KPX_ODOMETRY_MAX_LEVELS], H[KPX_ODOMETRY_MAX_LEVELS];
};

void odo_carve(Arena &a, int pairs, int width, int height, int levels, bool images, OdoWs *w)
{
    w->state = a.get<OdoState>((size_t)pairs);
    w->pose = a.get<double>((size_t)pairs * 16);
    w->keymap = a.get<unsigned long long>((size_t)pairs * width * height);
    w->counts = a.get<int32_t>((size_t)compact_ws_ints((int64_t)width * height));
    w->slab_blocks = (int)cdiv((int64_t)width * height, kOdoThreads);
    w->slab = a.get<double>((size_t)pairs * kSums * w->slab_blocks);
    for (int l = 0; l < levels; ++l) {
        w->W[l] = l ? w->W[l - 1] >> 1 : width;
        w->H[l] = l ? w->H[l - 1] >> 1 : height;
        w->planes[l] = images ? a.get<float>((size_t)pairs * kPlanes * w->W[l] * w->H[l]) : nullptr;
    }
}

inline bool odo_size_ok(int pairs, int width, int height, int levels)
{
    if (pairs < 1 || pairs > 65535 || width < 1 || height < 1 || (int64_t)width * height >= ((int64_t)1 << 30)) return false;
    if (levels < 1 || levels > KPX_ODOMETRY_MAX_LEVELS) return false;
    return (width >> (levels - 1)) >= 1 && (height >> (levels - 1)) >= 1;
}

int odo_begin(const OdoWs &w, int pairs, int npx, const double *h_pose, hipStream_t st)
{
    KPX_HIP(hipMemsetAsync(w.state, 0, sizeof(OdoState) * (size_t)pairs, st));
    KPX_HIP(hipMemsetAsync(w.keymap, 0xFF, sizeof(unsigned long long) * (size_t)pairs * npx, st));
    KPX_HIP(hipMemcpyAsync(w.pose, h_pose, sizeof(double) * 16 * (size_t)pairs, hipMemcpyHostToDevice, st));
    return KPX_OK;
}

OdoLevel odo_level(const float *planes, int W, int H, const double *K, int level)
{
    OdoLevel L;
    const size_t n = (size_t)W * H;
    L.Is = planes; L.Ds = planes + n; L.It = planes + 2 * n; L.Dt = planes + 3 * n;
    L.dIx = planes + 4 * n; L.dIy = planes + 5 * n; L.dDx = planes + 6 * n; L.dDy = planes + 7 * n;
    L.stride = kPlanes * n;
    L.W = W; L.H = H;
    const double s = (double)(1 << level);           // a power of two: the division is exact
    L.fx = K[0] / s; L.fy = K[1] / s; L.cx = K[2] / s; L.cy = K[3] / s;
    return L;
}

struct ComprPred {
    const unsigned long long *keymap;
    __device__ bool operator()(int64_t i, int) const { return keymap[i] != kEmpty; }
};
struct ComprEmit {
    const unsigned long long *keymap;
    int32_t *out;
    int W;
    __device__ void operator()(int64_t i, int, int32_t dst) const
    {
        const int spx = (int)(unsigned)(keymap[i] & 0xFFFFFFFFull), tpx = (int)i;
        const int vs = spx / W, vt = tpx / W;
        out[4 * (size_t)dst] = spx - vs * W; out[4 * (size_t)dst + 1] = vs; out[4 * (size_t)dst + 2] = tpx - vt * W; out[4 * (size_t)dst + 3] = vt;
    }
};

inline bool intrinsic_ok(const double *K) { return K && K[0] > 0.0 && K[1] > 0.0; }

}  // namespace
}  // namespace kpx

using namespace kpx;

KPX_EXPORT size_t kpx_image_workspace_bytes(int32_t count, int32_t width, int32_t height)
{
    if (count < 1 || width < 1 || height < 1) return 0;
    Arena a(nullptr, 0);
    a.get<float>((size_t)count * width * height);
    return a.off;
}

KPX_EXPORT int kpx_image_filter(const float *src, float *dst, int32_t count, int32_t width, int32_t height, int32_t filter_type, void *ws,
                                size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(filter_type >= KPX_IMAGE_GAUSSIAN3 && filter_type <= KPX_IMAGE_SOBEL3DY, "kpx_image_filter: unknown filter type %d", filter_type);
    KPX_REQUIRE(count >= 1 && count <= 65535 && width >= 1 && height >= 1 && (int64_t)width * height < ((int64_t)1 << 30), "kpx_image_filter: bad image size or count");
    KPX_REQUIRE(src && dst && ws && src != dst, "kpx_image_filter: null pointer or dst aliases src");
    Arena a(ws, ws_bytes);
    float *tmp = a.get<float>((size_t)count * width * height);
    KPX_ARENA_CHECK(a);
    int kh = filter_type, kv = filter_type;
    if (filter_type == KPX_IMAGE_SOBEL3DX) { kh = kTapDiff; kv = kTapSmooth; }
    if (filter_type == KPX_IMAGE_SOBEL3DY) { kh = kTapSmooth; kv = kTapDiff; }
    ImageJobs j;
    memset(&j, 0, sizeof j);
    const size_t stride = (size_t)width * height;
    j.src[0] = src; j.dst[0] = tmp; j.kind[0] = kh;
    if (int rc = filter_pass(j, 1, count, stride, width, height, true, (hipStream_t)stream)) return rc;
    j.src[0] = tmp; j.dst[0] = dst; j.kind[0] = kv;
    return filter_pass(j, 1, count, stride, width, height, false, (hipStream_t)stream);
}

KPX_EXPORT int kpx_image_downsample(const float *src, float *dst, int32_t count, int32_t width, int32_t height, void *stream)
{
    KPX_REQUIRE(count >= 1 && count <= 65535 && width >= 2 && height >= 2 && (int64_t)width * height < ((int64_t)1 << 30), "kpx_image_downsample: bad image size or count");
    KPX_REQUIRE(src && dst, "kpx_image_downsample: null pointer");
    ImageJobs j;
    memset(&j, 0, sizeof j);
    j.src[0] = src; j.dst[0] = dst;
    const int w2 = width >> 1, h2 = height >> 1;
    hipLaunchKernelGGL(downsample_kernel, dim3((unsigned)cdiv((int64_t)w2 * h2, kOdoThreads), count, 1), dim3(kOdoThreads), 0, (hipStream_t)stream, j,
                       (size_t)width * height, (size_t)w2 * h2, width, height);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT size_t kpx_odometry_workspace_bytes(int32_t pairs, int32_t width, int32_t height, int32_t levels)
{
    if (!odo_size_ok(pairs, width, height, levels)) return 0;
    Arena a(nullptr, 0);
    OdoWs w;
    odo_carve(a, pairs, width, height, levels, true, &w);
    return a.off;
}

KPX_EXPORT int kpx_odometry_correspondence(const float *depth_s, const float *depth_t, int32_t width, int32_t height, const double *h_intrinsic,
                                           const double *h_extrinsic, double depth_diff_max, int32_t *corres, int32_t *d_count, void *ws,
                                           size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(odo_size_ok(1, width, height, 1), "kpx_odometry_correspondence: bad image size");
    KPX_REQUIRE(depth_s && depth_t && h_extrinsic && corres && d_count && ws, "kpx_odometry_correspondence: null pointer");
    KPX_REQUIRE(intrinsic_ok(h_intrinsic), "kpx_odometry_correspondence: the focal lengths must be positive");
    Arena a(ws, ws_bytes);
    OdoWs w;
    odo_carve(a, 1, width, height, 1, false, &w);
    KPX_ARENA_CHECK(a);
    hipStream_t st = (hipStream_t)stream;
    const int npx = width * height;
    if (int rc = odo_begin(w, 1, npx, h_extrinsic, st)) return rc;
    OdoLevel L;
    memset(&L, 0, sizeof L);
    L.Ds = depth_s; L.Dt = depth_t; L.stride = 0; L.W = width; L.H = height;
    L.fx = h_intrinsic[0]; L.fy = h_intrinsic[1]; L.cx = h_intrinsic[2]; L.cy = h_intrinsic[3];
    hipLaunchKernelGGL(odo_corr_kernel, dim3((unsigned)cdiv(npx, kOdoThreads), 1), dim3(kOdoThreads), 0, st, L, (const OdoState *)w.state,
                       (const double *)w.pose, w.keymap, (size_t)npx, depth_diff_max);
    KPX_LAUNCH_CHECK();
    ComprPred pred{ w.keymap };
    ComprEmit emit{ w.keymap, corres, width };
    return compact(pred, emit, (int64_t)npx, 1, w.counts, d_count, st);
}

KPX_EXPORT int kpx_odometry_iteration(const float *color_s, const float *depth_s, const float *color_t, const float *depth_t, const float *color_dx,
                                      const float *color_dy, const float *depth_dx, const float *depth_dy, int32_t width, int32_t height,
                                      const double *h_intrinsic, const double *h_extrinsic, int32_t jacobian, double depth_diff_max, double *d_out,
                                      void *ws, size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(odo_size_ok(1, width, height, 1), "kpx_odometry_iteration: bad image size");
    KPX_REQUIRE(jacobian == KPX_ODOMETRY_COLOR || jacobian == KPX_ODOMETRY_HYBRID, "kpx_odometry_iteration: unknown jacobian %d", jacobian);
    KPX_REQUIRE(color_s && depth_s && color_t && depth_t && color_dx && color_dy && h_extrinsic && d_out && ws, "kpx_odometry_iteration: null pointer");
    KPX_REQUIRE(jacobian == KPX_ODOMETRY_COLOR || (depth_dx && depth_dy), "kpx_odometry_iteration: the hybrid term needs the depth gradients");
    KPX_REQUIRE(intrinsic_ok(h_intrinsic), "kpx_odometry_iteration: the focal lengths must be positive");
    Arena a(ws, ws_bytes);
    OdoWs w;
    odo_carve(a, 1, width, height, 1, false, &w);
    KPX_ARENA_CHECK(a);
    hipStream_t st = (hipStream_t)stream;
    const int npx = width * height;
    if (int rc = odo_begin(w, 1, npx, h_extrinsic, st)) return rc;
    OdoLevel L;
    L.Is = color_s; L.Ds = depth_s; L.It = color_t; L.Dt = depth_t; L.dIx = color_dx; L.dIy = color_dy; L.dDx = depth_dx; L.dDy = depth_dy;
    L.stride = 0; L.W = width; L.H = height;
    L.fx = h_intrinsic[0]; L.fy = h_intrinsic[1]; L.cx = h_intrinsic[2]; L.cy = h_intrinsic[3];
    const dim3 grid((unsigned)cdiv(npx, kOdoThreads), 1);
    hipLaunchKernelGGL(odo_corr_kernel, grid, dim3(kOdoThreads), 0, st, L, (const OdoState *)w.state, (const double *)w.pose, w.keymap, (size_t)npx,
                       depth_diff_max);
    if (jacobian == KPX_ODOMETRY_COLOR)
        hipLaunchKernelGGL(odo_gather_kernel<kModeColor>, grid, dim3(kOdoThreads), 0, st, L, w.state, w.pose, w.keymap, (size_t)npx, w.slab, w.slab_blocks, (double *)nullptr, d_out);
    else
        hipLaunchKernelGGL(odo_gather_kernel<kModeHybrid>, grid, dim3(kOdoThreads), 0, st, L, w.state, w.pose, w.keymap, (size_t)npx, w.slab, w.slab_blocks, (double *)nullptr, d_out);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT int kpx_rgbd_odometry(int32_t pairs, const void *depth_s, const void *color_s, const void *depth_t, const void *color_t, int32_t raw,
                                 const uint8_t *mask_s, const uint8_t *mask_t, double depth_scale, double depth_trunc, int32_t width, int32_t height,
                                 const double *h_intrinsic, const double *h_init, int32_t jacobian, int32_t levels, const int32_t *h_iterations,
                                 double depth_diff_max, double depth_min, double depth_max, double *d_results, void *ws, size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(odo_size_ok(pairs, width, height, levels), "kpx_rgbd_odometry: bad pair count, image size or level count (at most %d levels, the coarsest at least 1 x 1)", KPX_ODOMETRY_MAX_LEVELS);
    KPX_REQUIRE(jacobian == KPX_ODOMETRY_COLOR || jacobian == KPX_ODOMETRY_HYBRID, "kpx_rgbd_odometry: unknown jacobian %d", jacobian);
    KPX_REQUIRE(depth_s && color_s && depth_t && color_t && h_init && h_iterations && d_results && ws, "kpx_rgbd_odometry: null pointer");
    KPX_REQUIRE(intrinsic_ok(h_intrinsic), "kpx_rgbd_odometry: the focal lengths must be positive");
    KPX_REQUIRE(!raw || depth_scale > 0.0, "kpx_rgbd_odometry: depth_scale must be positive");
    KPX_REQUIRE(raw || (!mask_s && !mask_t), "kpx_rgbd_odometry: masks go with raw frames");
    for (int l = 0; l < levels; ++l) KPX_REQUIRE(h_iterations[l] >= 0, "kpx_rgbd_odometry: negative iteration count");
    Arena a(ws, ws_bytes);
    OdoWs w;
    odo_carve(a, pairs, width, height, levels, true, &w);
    KPX_ARENA_CHECK(a);
    hipStream_t st = (hipStream_t)stream;
    const int npx = width * height;
    if (int rc = odo_begin(w, pairs, npx, h_init, st)) return rc;
    const dim3 blk(kOdoThreads);
    auto plane = [&](int l, int p) { return w.planes[l] + (size_t)p * w.W[l] * w.H[l]; };
    auto stride = [&](int l) { return (size_t)kPlanes * w.W[l] * w.H[l]; };
    auto jobs4 = [&](int l, const int src[4], const int dst[4], const int kind[4]) {
        ImageJobs j;
        for (int k = 0; k < 4; ++k) { j.src[k] = plane(l, src[k]); j.dst[k] = plane(l, dst[k]); j.kind[k] = kind[k]; }
        return j;
    };
    // preprocess: conversion and depth range -> planes 8..11, Gaussian3 -> planes 0..3
    {
        const dim3 grid((unsigned)cdiv(npx, kOdoThreads), pairs, 2);
        if (raw)
            hipLaunchKernelGGL(odo_prepare_kernel<true>, grid, blk, 0, st, depth_s, color_s, depth_t, color_t, mask_s, mask_t, (float)depth_scale,
                               (float)depth_trunc, depth_min, depth_max, w.planes[0], stride(0), npx);
        else
            hipLaunchKernelGGL(odo_prepare_kernel<false>, grid, blk, 0, st, depth_s, color_s, depth_t, color_t, mask_s, mask_t, 1.0f, 0.0f, depth_min,
                               depth_max, w.planes[0], stride(0), npx);
        KPX_LAUNCH_CHECK();
        const int g3[4] = { kTapGauss3, kTapGauss3, kTapGauss3, kTapGauss3 };
        const int s0[4] = { 8, 9, 10, 11 }, t0[4] = { 12, 13, 14, 15 }, f0[4] = { 0, 1, 2, 3 };
        if (int rc = filter_pass(jobs4(0, s0, t0, g3), 4, pairs, stride(0), width, height, true, st)) return rc;
        if (int rc = filter_pass(jobs4(0, t0, f0, g3), 4, pairs, stride(0), width, height, false, st)) return rc;
    }
    // NormalizeIntensity: full-resolution correspondences at the initial pose, 0.5 / mean over them
    const OdoLevel L0 = odo_level(w.planes[0], width, height, h_intrinsic, 0);
    {
        const dim3 grid((unsigned)cdiv(npx, kOdoThreads), pairs);
        hipLaunchKernelGGL(odo_corr_kernel, grid, blk, 0, st, L0, (const OdoState *)w.state, (const double *)w.pose, w.keymap, (size_t)npx, depth_diff_max);
        hipLaunchKernelGGL(odo_gather_kernel<kModeNormalise>, grid, blk, 0, st, L0, w.state, w.pose, w.keymap, (size_t)npx, w.slab, w.slab_blocks, (double *)nullptr,
                           (double *)nullptr);
        hipLaunchKernelGGL(odo_scale_kernel, dim3(grid.x, pairs, 2), blk, 0, st, w.planes[0], stride(0), npx, (const OdoState *)w.state);
        KPX_LAUNCH_CHECK();
    }
    // pyramids (colour: Gaussian3 then 2 x 2 mean; depth: 2 x 2 mean) and the target's Sobel images
    for (int l = 0; l < levels; ++l) {
        if (l > 0) {
            const int m = l - 1;
            ImageJobs j;
            memset(&j, 0, sizeof j);
            j.src[0] = plane(m, 0); j.dst[0] = plane(m, 12); j.kind[0] = kTapGauss3;
            j.src[1] = plane(m, 2); j.dst[1] = plane(m, 14); j.kind[1] = kTapGauss3;
            if (int rc = filter_pass(j, 2, pairs, stride(m), w.W[m], w.H[m], true, st)) return rc;
            j.src[0] = plane(m, 12); j.dst[0] = plane(m, 8);
            j.src[1] = plane(m, 14); j.dst[1] = plane(m, 10);
            if (int rc = filter_pass(j, 2, pairs, stride(m), w.W[m], w.H[m], false, st)) return rc;
            ImageJobs d;
            const int ds_[4] = { 8, 1, 10, 3 };
            for (int k = 0; k < 4; ++k) { d.src[k] = plane(m, ds_[k]); d.dst[k] = plane(l, k); d.kind[k] = 0; }
            hipLaunchKernelGGL(downsample_kernel, dim3((unsigned)cdiv((int64_t)w.W[l] * w.H[l], kOdoThreads), pairs, 4), blk, 0, st, d, stride(m), stride(l),
                               w.W[m], w.H[m]);
            KPX_LAUNCH_CHECK();
        }
        const int sh[4] = { 2, 2, 3, 3 }, th[4] = { 12, 13, 14, 15 }, kh[4] = { kTapDiff, kTapSmooth, kTapDiff, kTapSmooth };
        const int dv[4] = { 4, 5, 6, 7 }, kv[4] = { kTapSmooth, kTapDiff, kTapSmooth, kTapDiff };
        if (int rc = filter_pass(jobs4(l, sh, th, kh), 4, pairs, stride(l), w.W[l], w.H[l], true, st)) return rc;
        if (int rc = filter_pass(jobs4(l, th, dv, kv), 4, pairs, stride(l), w.W[l], w.H[l], false, st)) return rc;
    }
    // coarse to fine: two launches per iteration
    for (int l = levels - 1; l >= 0; --l) {
        const OdoLevel L = odo_level(w.planes[l], w.W[l], w.H[l], h_intrinsic, l);
        const dim3 grid((unsigned)cdiv((int64_t)w.W[l] * w.H[l], kOdoThreads), pairs);
        for (int it = 0; it < h_iterations[levels - 1 - l]; ++it) {
            hipLaunchKernelGGL(odo_corr_kernel, grid, blk, 0, st, L, (const OdoState *)w.state, (const double *)w.pose, w.keymap, (size_t)npx, depth_diff_max);
            if (jacobian == KPX_ODOMETRY_COLOR)
                hipLaunchKernelGGL(odo_gather_kernel<kModeColor>, grid, blk, 0, st, L, w.state, w.pose, w.keymap, (size_t)npx, w.slab, w.slab_blocks, (double *)nullptr, (double *)nullptr);
            else
                hipLaunchKernelGGL(odo_gather_kernel<kModeHybrid>, grid, blk, 0, st, L, w.state, w.pose, w.keymap, (size_t)npx, w.slab, w.slab_blocks, (double *)nullptr, (double *)nullptr);
        }
        KPX_LAUNCH_CHECK();
    }
    // the information matrix from the full-resolution correspondences at the final pose, and the results
    {
        const dim3 grid((unsigned)cdiv(npx, kOdoThreads), pairs);
        hipLaunchKernelGGL(odo_corr_kernel, grid, blk, 0, st, L0, (const OdoState *)w.state, (const double *)w.pose, w.keymap, (size_t)npx, depth_diff_max);
        hipLaunchKernelGGL(odo_gather_kernel<kModeInfo>, grid, blk, 0, st, L0, w.state, w.pose, w.keymap, (size_t)npx, w.slab, w.slab_blocks, d_results, (double *)nullptr);
        KPX_LAUNCH_CHECK();
    }
    return KPX_OK;
}
