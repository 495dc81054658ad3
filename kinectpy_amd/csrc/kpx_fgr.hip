// kpx_fgr.hip -- Fast Global Registration (Zhou, Park, Koltun 2016; Open3D's registration_fgr_based_on_feature_matching /
// ..._based_on_correspondence with a FastGlobalRegistrationOption).  tests/fgr_ref.py is the pinned float64 statement.
//   tuple test    100 nc trials of three correspondences (Philox, stream word 2), kept when the three edge lengths agree within
//                 tuple_scale on both sides; the first maximum_tuple_count passing trials, in trial order, give 3 pairs each
//   normalise     both clouds to their own mean (128-bit fixed-point sums: order-free) and the largest radius over both
//   optimise      iteration_number Gauss-Newton rounds on T (target -> source) under the Geman-McClure weight
//                 (par / (|r|^2 + par))^2, par annealed by division_factor every fourth round down to
//                 maximum_correspondence_distance -- ONE launch of ONE block (a round is a few microseconds of arithmetic: 64
//                 launches with a host solve between them would be all latency)
// A round's 6x6 system has 16 distinct sums (the translation block of J^T J is (sum s) I, the mixed block is the cross matrix of
// sum s q); each thread keeps those in fp64 registers, a wave folds them with cross-lane adds, the eight waves' rows are added
// in wave order by sixteen lanes (one per sum), lane 0 solves (solve6_ldlt_ranked, euler_update) and publishes T and par in LDS.
#include <vector>

#include "kpx_compact.h"
#include "kpx_fixed.h"
#include "kpx_linalg.h"

namespace kpx {

constexpr int kFgrBatch = 32768;           // trials per launch: RANSAC's batch (kpx_fpfh.hip)
constexpr int kFgrTrialsPerCorres = 100;   // [O3D] AdvancedMatching: number_of_trial = ncorr * 100
constexpr int kFgrThreads = 512;           // 8 waves, two per SIMD, 256 VGPRs each: 1024 threads cap a thread at 128 and the inlined solve spills
constexpr int kFgrWaves = kFgrThreads / 64;
constexpr int kFgrSums = 16;
constexpr double kFgrRankTol = 1e-12;      // solve6_ldlt_ranked: a collinear correspondence set leaves pivots of ~1e-16

// sums of the coordinates (source x y z, target x y z) as 128-bit fixed-point words, and the bits of the largest squared radius
struct FgrNorm {
    unsigned long long sum[6][2];
    unsigned long long max_d2_bits;
    unsigned long long pad;
};

// any index outside its cloud -> *bad = 1
__global__ __launch_bounds__(256) void fgr_range_kernel(const int32_t *__restrict__ corres, int64_t nc, int64_t n_src, int64_t n_tgt,
                                                        int32_t *__restrict__ bad)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nc) return;
    const int64_t i = corres[2 * c], j = corres[2 * c + 1];
    if (i < 0 || i >= n_src || j < 0 || j >= n_tgt) *bad = 1;
}

// ---- tuple test -------------------------------------------------------------------------------------------------
__device__ __forceinline__ void fgr_draw(uint32_t trial, int64_t nc, uint32_t seed_lo, uint32_t seed_hi, int64_t pick[3])
{
    uint32_t out[4];
    philox4x32_10(0u, trial, 2u, 0u, seed_lo, seed_hi, out);
#pragma unroll
    for (int q = 0; q < 3; ++q) pick[q] = (int64_t)(((uint64_t)out[q] * (uint64_t)nc) >> 32);
}
// one thread per trial t0 + t: pass[t] = 1 when the three edges agree within tuple_scale
__global__ __launch_bounds__(256) void fgr_trial_kernel(const float *__restrict__ src, const float *__restrict__ tgt,
                                                        const int32_t *__restrict__ corres, int64_t nc, int32_t t0, int32_t count,
                                                        uint32_t seed_lo, uint32_t seed_hi, double tuple_scale, uint8_t *__restrict__ pass)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    int64_t pick[3];
    fgr_draw((uint32_t)(t0 + t), nc, seed_lo, seed_hi, pick);
    double sp[3][3], tp[3][3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const float *s = src + 3 * (int64_t)corres[2 * pick[q]], *g = tgt + 3 * (int64_t)corres[2 * pick[q] + 1];
#pragma unroll
        for (int a = 0; a < 3; ++a) { sp[q][a] = s[a]; tp[q][a] = g[a]; }
    }
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {                     // edges 0-1, 1-2, 2-0
        const int u = k, v = (k + 1) % 3;
        const double dx = sp[u][0] - sp[v][0], dy = sp[u][1] - sp[v][1], dz = sp[u][2] - sp[v][2];
        const double ex = tp[u][0] - tp[v][0], ey = tp[u][1] - tp[v][1], ez = tp[u][2] - tp[v][2];
        const double l = sqrt(dx * dx + dy * dy + dz * dz), m = sqrt(ex * ex + ey * ey + ez * ez);
        ok = ok && (l * tuple_scale < m) && (m < l / tuple_scale);
    }
    pass[t] = ok ? 1 : 0;
}
struct FgrPassPred {
    const uint8_t *pass;
    __device__ bool operator()(int64_t i, int) const { return pass[i] != 0; }
};
struct FgrPassEmit {
    int32_t *list;
    __device__ void operator()(int64_t i, int, int32_t dst) const { list[dst] = (int32_t)i; }
};
// the three pairs of the first `take` passing trials of a batch behind the `found` tuples of the batches before it
__global__ __launch_bounds__(256) void fgr_emit_kernel(const int32_t *__restrict__ corres, int64_t nc, int32_t t0, const int32_t *__restrict__ list,
                                                       int32_t take, int32_t found, uint32_t seed_lo, uint32_t seed_hi,
                                                       int32_t *__restrict__ pairs, int32_t *__restrict__ d_count)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k == 0) *d_count = 3 * (found + take);
    if (k >= take) return;
    int64_t pick[3];
    fgr_draw((uint32_t)(t0 + list[k]), nc, seed_lo, seed_hi, pick);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int64_t o = 2 * (3 * (int64_t)(found + k) + q);
        pairs[o] = corres[2 * pick[q]];
        pairs[o + 1] = corres[2 * pick[q] + 1];
    }
}

// ---- normalisation ----------------------------------------------------------------------------------------------
// blockIdx.y: 0 the source, 1 the target
__global__ __launch_bounds__(256) void fgr_sum_kernel(const float *__restrict__ src, int64_t n_src, const float *__restrict__ tgt, int64_t n_tgt,
                                                      FgrNorm *__restrict__ nm)
{
    const int cl = blockIdx.y;
    const float *p = cl ? tgt : src;
    const int64_t n = cl ? n_tgt : n_src;
    unsigned long long lo[3] = { 0ull, 0ull, 0ull }, hi[3] = { 0ull, 0ull, 0ull };
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            unsigned long long l, h;
            fixed_split((double)p[3 * i + a], l, h);
            fixed_accumulate(lo[a], hi[a], l, h);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const unsigned long long l = __shfl_down(lo[a], o, 64), h = __shfl_down(hi[a], o, 64);
            fixed_accumulate(lo[a], hi[a], l, h);
        }
    }
    if (lane_id() == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) fixed_add_words(&nm->sum[3 * cl + a][0], lo[a], hi[a]);
    }
}
__device__ __forceinline__ void fgr_means(const FgrNorm *nm, int64_t n_src, int64_t n_tgt, double ms[3], double mt[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        ms[a] = fixed_value(nm->sum[a][0], nm->sum[a][1]) / (double)n_src;
        mt[a] = fixed_value(nm->sum[3 + a][0], nm->sum[3 + a][1]) / (double)n_tgt;
    }
}
// largest |p - mean|^2 over both clouds (a maximum: order-free; non-negative doubles order as their bit patterns)
__global__ __launch_bounds__(256) void fgr_radius_kernel(const float *__restrict__ src, int64_t n_src, const float *__restrict__ tgt, int64_t n_tgt,
                                                         FgrNorm *__restrict__ nm)
{
    const int cl = blockIdx.y;
    const float *p = cl ? tgt : src;
    const int64_t n = cl ? n_tgt : n_src;
    double ms[3], mt[3];
    fgr_means(nm, n_src, n_tgt, ms, mt);
    const double mx = cl ? mt[0] : ms[0], my = cl ? mt[1] : ms[1], mz = cl ? mt[2] : ms[2];
    double best = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double dx = (double)p[3 * i] - mx, dy = (double)p[3 * i + 1] - my, dz = (double)p[3 * i + 2] - mz;
        const double d2 = dx * dx + dy * dy + dz * dz;
        best = d2 > best ? d2 : best;
    }
    best = wave_max(best);
    if (lane_id() == 0) atomicMax(&nm->max_d2_bits, (unsigned long long)__double_as_longlong(best));
}

// ---- optimisation -----------------------------------------------------------------------------------------------
// P: f64 [6][nc], the normalised source (rows 0-2) and target (rows 3-5) point of every correspondence; a thread reads back only
// what it wrote itself.  result: T source -> target in the clouds' units (16) | par | rounds | failed solves | largest radius.
__global__ __launch_bounds__(kFgrThreads) void fgr_optimize_kernel(const float *__restrict__ src, const float *__restrict__ tgt,
                                                                   const int32_t *__restrict__ corres, int64_t nc, const FgrNorm *__restrict__ nm,
                                                                   int64_t n_src, int64_t n_tgt, int use_absolute_scale, int decrease_mu,
                                                                   double division_factor, double max_corr_dist, int iterations,
                                                                   double *__restrict__ P, double *__restrict__ result)
{
    __shared__ double sT[16];
    __shared__ double s_par;
    __shared__ double part[kFgrWaves][kFgrSums];
    __shared__ double acc[kFgrSums];
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    double ms[3], mt[3];
    fgr_means(nm, n_src, n_tgt, ms, mt);
    const double scale = sqrt(__longlong_as_double((long long)nm->max_d2_bits));
    const bool flat = !(scale > 0.0);                   // every point of both clouds on its cloud's mean: nothing to normalise by
    const double scale_global = (use_absolute_scale || flat) ? 1.0 : scale;
    const double par0 = (use_absolute_scale && !flat) ? scale : 1.0;
    for (int64_t c = tid; c < nc; c += kFgrThreads) {
        const float *s = src + 3 * (int64_t)corres[2 * c], *g = tgt + 3 * (int64_t)corres[2 * c + 1];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            P[a * nc + c] = ((double)s[a] - ms[a]) / scale_global;
            P[(3 + a) * nc + c] = ((double)g[a] - mt[a]) / scale_global;
        }
    }
    if (tid < 16) sT[tid] = (tid % 5 == 0) ? 1.0 : 0.0;
    if (tid == 0) s_par = par0;
    __syncthreads();
    const int rounds = nc > 0 ? iterations : 0;
    int failed = 0;                                      // thread 0's
    for (int itr = 0; itr < rounds; ++itr) {
        double T[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = sT[k];
        const double par = s_par;
        double a[kFgrSums];
#pragma unroll
        for (int k = 0; k < kFgrSums; ++k) a[k] = 0.0;
        for (int64_t c = tid; c < nc; c += kFgrThreads) {
            const double px = P[c], py = P[nc + c], pz = P[2 * nc + c];
            const double x = P[3 * nc + c], y = P[4 * nc + c], z = P[5 * nc + c];
            const double qx = T[0] * x + T[1] * y + T[2] * z + T[3];
            const double qy = T[4] * x + T[5] * y + T[6] * z + T[7];
            const double qz = T[8] * x + T[9] * y + T[10] * z + T[11];
            const double rx = px - qx, ry = py - qy, rz = pz - qz;
            const double w = par / (rx * rx + ry * ry + rz * rz + par), s = w * w;
            // J^T J = sum s (rows (0, -qz, qy, -1, 0, 0), (qz, 0, -qx, 0, -1, 0), (-qy, qx, 0, 0, 0, -1))^T (the same), J^T r likewise
            a[0] += s * (qy * qy + qz * qz);
            a[1] += s * (qx * qx + qz * qz);
            a[2] += s * (qx * qx + qy * qy);
            a[3] += s * (qx * qy);
            a[4] += s * (qx * qz);
            a[5] += s * (qy * qz);
            a[6] += s * qx;
            a[7] += s * qy;
            a[8] += s * qz;
            a[9] += s;
            a[10] += s * (qz * ry - qy * rz);
            a[11] += s * (qx * rz - qz * rx);
            a[12] += s * (qy * rx - qx * ry);
            a[13] += s * rx;
            a[14] += s * ry;
            a[15] += s * rz;
        }
#pragma unroll
        for (int k = 0; k < kFgrSums; ++k) {
            const double v = wave_sum(a[k]);
            if (lane == 0) part[wave][k] = v;
        }
        __syncthreads();
        if (wave == 0) {
            if (lane < kFgrSums) {
                double v = 0.0;
#pragma unroll
                for (int w2 = 0; w2 < kFgrWaves; ++w2) v += part[w2][lane];
                acc[lane] = v;
            }
            wave_lds_fence();
            if (lane == 0) {
                double A[36], b[6], xs[6], U[16], Tc[16], Tn[16];
#pragma unroll
                for (int k = 0; k < 36; ++k) A[k] = 0.0;
                A[0] = acc[0]; A[7] = acc[1]; A[14] = acc[2];
                A[1] = A[6] = -acc[3]; A[2] = A[12] = -acc[4]; A[8] = A[13] = -acc[5];
                A[4] = A[24] = -acc[8]; A[5] = A[30] = acc[7];
                A[9] = A[19] = acc[8];  A[11] = A[31] = -acc[6];
                A[15] = A[20] = -acc[7]; A[16] = A[26] = acc[6];
                A[21] = A[28] = A[35] = acc[9];
                b[0] = -acc[10]; b[1] = -acc[11]; b[2] = -acc[12]; b[3] = acc[13]; b[4] = acc[14]; b[5] = acc[15];
#pragma unroll
                for (int k = 0; k < 16; ++k) { U[k] = (k % 5 == 0) ? 1.0 : 0.0; Tc[k] = sT[k]; }
                if (solve6_ldlt_ranked(A, b, xs, kFgrRankTol)) euler_update(xs, U); else ++failed;
                for (int r = 0; r < 3; ++r)                                   // T = delta T (the last row stays 0 0 0 1)
                    for (int c = 0; c < 4; ++c) {
                        double v = 0.0;
                        for (int k = 0; k < 4; ++k) v += U[4 * r + k] * Tc[4 * k + c];
                        Tn[4 * r + c] = v;
                    }
#pragma unroll
                for (int k = 0; k < 12; ++k) sT[k] = Tn[k];
                if (decrease_mu && itr % 4 == 0 && par > max_corr_dist) s_par = par / division_factor;
            }
        }
        __syncthreads();
    }
    if (tid) return;
    // T maps target -> source in normalised coordinates: back to the clouds' units, then the rigid inverse
#pragma unroll
    for (int k = 0; k < 16; ++k) result[k] = (k % 5 == 0) ? 1.0 : 0.0;
    if (rounds > 0) {
        double tp[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            tp[r] = -(sT[4 * r] * mt[0] + sT[4 * r + 1] * mt[1] + sT[4 * r + 2] * mt[2]) + sT[4 * r + 3] * scale_global + ms[r];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) result[4 * r + c] = sT[4 * c + r];
            result[4 * r + 3] = -(sT[r] * tp[0] + sT[4 + r] * tp[1] + sT[8 + r] * tp[2]);
        }
    }
    result[16] = s_par; result[17] = (double)rounds; result[18] = (double)failed; result[19] = scale;
}

struct FgrBuffers {
    uint8_t *pass;
    int32_t *list, *counts, *n_pass, *bad;
    FgrNorm *norm;
    double *P, *result;
};
static void fgr_carve(int64_t n_corres, Arena &a, FgrBuffers *b)
{
    b->pass = a.get<uint8_t>(kFgrBatch);
    b->list = a.get<int32_t>(kFgrBatch);
    b->counts = a.get<int32_t>((size_t)compact_ws_ints(kFgrBatch));
    b->n_pass = a.get<int32_t>(1);
    b->bad = a.get<int32_t>(1);
    b->norm = a.get<FgrNorm>(1);
    b->P = a.get<double>((size_t)6 * (size_t)(n_corres > 0 ? n_corres : 1));
    b->result = a.get<double>(20);
}
// KPX_ERR_RANGE before any point is read through an index that lies outside its cloud (one small launch and a 4-byte read-back)
static int fgr_check_range(const int32_t *corres, int64_t nc, int64_t n_src, int64_t n_tgt, int32_t *d_bad, const char *who, hipStream_t st)
{
    if (nc == 0) return KPX_OK;
    int32_t bad = 0;
    KPX_HIP(hipMemsetAsync(d_bad, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(fgr_range_kernel, dim3((unsigned)cdiv(nc, 256)), dim3(256), 0, st, corres, nc, n_src, n_tgt, d_bad);
    KPX_LAUNCH_CHECK();
    KPX_HIP(hipMemcpyAsync(&bad, d_bad, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    KPX_HIP(hipStreamSynchronize(st));
    if (bad) return fail(KPX_ERR_RANGE, "%s: correspondence index out of range (source has %lld points, target %lld)", who, (long long)n_src, (long long)n_tgt);
    return KPX_OK;
}

}  // namespace kpx

using namespace kpx;

KPX_EXPORT size_t kpx_fgr_workspace_bytes(int64_t n_corres)
{
    Arena a(nullptr, 0);
    FgrBuffers b;
    fgr_carve(n_corres, a, &b);
    return a.off;
}

KPX_EXPORT int kpx_fgr_tuple_test(const float *src, int64_t n_src, const float *tgt, int64_t n_tgt, const int32_t *corres, int64_t n_corres,
                                  double tuple_scale, int32_t maximum_tuple_count, uint64_t seed, int32_t *d_pairs, int32_t *d_count,
                                  void *ws, size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(n_src >= 0 && n_tgt >= 0 && n_corres >= 0 && maximum_tuple_count >= 0, "kpx_fgr_tuple_test: negative size");
    KPX_REQUIRE(n_corres * kFgrTrialsPerCorres < ((int64_t)1 << 31), "kpx_fgr_tuple_test: %d trials per correspondence must stay below 2^31", kFgrTrialsPerCorres);
    KPX_REQUIRE(d_count && ws && (n_corres == 0 || (src && tgt && corres)), "kpx_fgr_tuple_test: null pointer");
    hipStream_t st = (hipStream_t)stream;
    Arena a(ws, ws_bytes);
    FgrBuffers b;
    fgr_carve(n_corres, a, &b);
    KPX_ARENA_CHECK(a);
    int rc = fgr_check_range(corres, n_corres, n_src, n_tgt, b.bad, "kpx_fgr_tuple_test", st);
    if (rc) return rc;
    KPX_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), st));
    const int32_t trials = (int32_t)(n_corres * kFgrTrialsPerCorres);
    KPX_REQUIRE(trials == 0 || maximum_tuple_count == 0 || d_pairs, "kpx_fgr_tuple_test: null output");
    int32_t found = 0;
    // per batch: trials -> passing trials compacted in trial order -> ONE read-back (their number) -> the pairs of as many as are
    // still wanted; the next batch is issued only while the count is short
    for (int32_t t0 = 0; t0 < trials && found < maximum_tuple_count; t0 += kFgrBatch) {
        const int32_t count = trials - t0 < kFgrBatch ? trials - t0 : kFgrBatch;
        hipLaunchKernelGGL(fgr_trial_kernel, dim3((unsigned)cdiv(count, 256)), dim3(256), 0, st, src, tgt, corres, n_corres, t0, count,
                           (uint32_t)seed, (uint32_t)(seed >> 32), tuple_scale, b.pass);
        rc = compact(FgrPassPred{ b.pass }, FgrPassEmit{ b.list }, count, 1, b.counts, b.n_pass, st);
        if (rc) return rc;
        int32_t n_pass = 0;
        KPX_HIP(hipMemcpyAsync(&n_pass, b.n_pass, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        KPX_HIP(hipStreamSynchronize(st));
        const int32_t take = n_pass < maximum_tuple_count - found ? n_pass : maximum_tuple_count - found;
        if (take > 0) {
            hipLaunchKernelGGL(fgr_emit_kernel, dim3((unsigned)cdiv(take, 256)), dim3(256), 0, st, corres, n_corres, t0, b.list, take, found,
                               (uint32_t)seed, (uint32_t)(seed >> 32), d_pairs, d_count);
            KPX_LAUNCH_CHECK();
        }
        found += take;
    }
    return KPX_OK;
}

// h_result (host) f64 [20]: T source -> target (16) | final par | rounds run | failed solves | largest radius
KPX_EXPORT int kpx_fgr_optimize(const float *src, int64_t n_src, const float *tgt, int64_t n_tgt, const int32_t *corres, int64_t n_corres,
                                double division_factor, int32_t use_absolute_scale, int32_t decrease_mu, double maximum_correspondence_distance,
                                int32_t iteration_number, double *h_result, void *ws, size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(h_result, "kpx_fgr_optimize: null result");
    KPX_REQUIRE(n_src >= 0 && n_tgt >= 0 && n_corres >= 0 && iteration_number >= 0, "kpx_fgr_optimize: negative size");
    KPX_REQUIRE(division_factor > 0.0, "kpx_fgr_optimize: division_factor must be positive");
    KPX_REQUIRE(ws && (n_corres == 0 || (src && tgt && corres)), "kpx_fgr_optimize: null pointer");
    hipStream_t st = (hipStream_t)stream;
    Arena a(ws, ws_bytes);
    FgrBuffers b;
    fgr_carve(n_corres, a, &b);
    KPX_ARENA_CHECK(a);
    int rc = fgr_check_range(corres, n_corres, n_src, n_tgt, b.bad, "kpx_fgr_optimize", st);
    if (rc) return rc;
    if (n_src == 0 || n_tgt == 0) {                       // (then n_corres == 0) nothing to normalise: the identity, par as without a scale
        for (int k = 0; k < 20; ++k) h_result[k] = (k < 16 && k % 5 == 0) ? 1.0 : 0.0;
        h_result[16] = 1.0;
        return KPX_OK;
    }
    KPX_HIP(hipMemsetAsync(b.norm, 0, sizeof(FgrNorm), st));
    const int64_t n_max = n_src > n_tgt ? n_src : n_tgt;
    const dim3 grid((unsigned)(cdiv(n_max, 256) < 256 ? cdiv(n_max, 256) : 256), 2);
    hipLaunchKernelGGL(fgr_sum_kernel, grid, dim3(256), 0, st, src, n_src, tgt, n_tgt, b.norm);
    hipLaunchKernelGGL(fgr_radius_kernel, grid, dim3(256), 0, st, src, n_src, tgt, n_tgt, b.norm);
    hipLaunchKernelGGL(fgr_optimize_kernel, dim3(1), dim3(kFgrThreads), 0, st, src, tgt, corres, n_corres, (const FgrNorm *)b.norm, n_src, n_tgt,
                       (int)(use_absolute_scale != 0), (int)(decrease_mu != 0), division_factor, maximum_correspondence_distance,
                       (int)iteration_number, b.P, b.result);
    KPX_LAUNCH_CHECK();
    double r[20];
    KPX_HIP(hipMemcpyAsync(r, b.result, sizeof(r), hipMemcpyDeviceToHost, st));
    KPX_HIP(hipStreamSynchronize(st));
    memcpy(h_result, r, sizeof(r));
    return KPX_OK;
}
