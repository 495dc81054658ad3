// kpx_fps.hip -- PointCloud.farthest_point_down_sample(k, start_index) ([O3D] PointCloud::FarthestPointDownSample).
// Each sample is a global arg-max over the running distances, which depend on every earlier sample:
//   dist[j] = min(dist[j], d2(p[j], p[far]))       d2 = AC3 (fp64 differences of the float32 coordinates)
//   next    = the smallest j among the largest dist[j]; when that largest dist is 0 the previous index repeats
// The arg-max is taken in the total order "larger d, then smaller index", so no result depends on the reduction shape.
// Forms ("Farthest-point sampling"):
//   block  one block per cloud, a batch of clouds in one launch (clouds up to KPX_FPS_BLOCK_MAX_N points; in a batch of several
//          larger clouds, up to KPX_FPS_BATCH_BLOCK_MAX_N); a thread's points and their dist live in registers, then LDS,
//          then (beyond the on-chip caps) in global memory; one barrier per sample (wave partials double-buffered by parity)
//   chain  one large cloud: launch t reduces the candidates of launch t - 1 (every block, redundantly), block 0 records sample t,
//          then every block updates its slice of dist (global, L2/MALL-resident) and writes its candidate; candidates and the
//          recorded sample are double-buffered by the parity of t; stream order is the only synchronisation
#include "kpx_common.h"

namespace kpx {

namespace {

constexpr int kFpsThreads = KPX_FPS_BLOCK_THREADS;
constexpr int kFpsWaves = kFpsThreads / 64;
constexpr int kFpsReg = KPX_FPS_REG_N / kFpsThreads;                          // points per thread in registers
constexpr int kFpsLds = (KPX_FPS_LDS_N - KPX_FPS_REG_N) / kFpsThreads;        // points per thread in LDS
static_assert(kFpsReg * kFpsThreads == KPX_FPS_REG_N && (kFpsReg + kFpsLds) * kFpsThreads == KPX_FPS_LDS_N, "FPS caps");
static_assert(kFpsLds * kFpsThreads * 20 + 2 * kFpsWaves * 32 <= 160 * 1024, "FPS LDS tier exceeds the CU's LDS");
constexpr int kFpsBatch = 64;               // clouds per block-form launch (their descriptors travel as kernel arguments)
constexpr int kChainThreads = 256;
constexpr int kChainWaves = kChainThreads / 64;
constexpr int kChainMaxBlocks = 1024;       // candidate slots per parity
constexpr int kChainPerThread = 4;          // points per thread at which the chain stops adding blocks
constexpr int32_t kNoIdx = 0x7FFFFFFF;

// a (d, idx) candidate with the coordinates of its point, so that the next sample needs no global read
struct alignas(16) Cand {
    double d;
    int32_t idx;
    float x, y, z;
};
static_assert(sizeof(Cand) == 32, "Cand layout");
struct alignas(16) ChainState {           // the sample recorded by a chain launch (the all-zero rule keeps it)
    int32_t far;
    float x, y, z;
};

__device__ __forceinline__ bool better(double da, int32_t ia, double db, int32_t ib) { return da > db || (da == db && ia < ib); }

__device__ __forceinline__ double ac3(float x, float y, float z, double sx, double sy, double sz)
{
    const double dx = (double)x - sx, dy = (double)y - sy, dz = (double)z - sz;
    return fma(dz, dz, fma(dy, dy, dx * dx));
}

// arg-max over groups of W lanes (W = 64: the wave); every lane of a group ends with the group's winner
template <int W> __device__ __forceinline__ void group_argmax(double &d, int32_t &i)
{
#pragma unroll
    for (int o = 1; o < W; o <<= 1) {
        const double od = __shfl_xor(d, o, 64);
        const int32_t oi = __shfl_xor(i, o, 64);
        if (better(od, oi, d, i)) { d = od; i = oi; }
    }
}

// Block arg-max of one candidate per thread (W waves).  The lane that holds its wave's winner publishes the whole candidate in
// sh[wave]; after the barrier every wave reduces the W partials (lane l reads partial l mod W) and reads the winner back from LDS.
// sh is reused two calls later at the earliest, behind another barrier, so one barrier per call suffices.  All threads call.
template <int W> __device__ __forceinline__ Cand block_argmax(const Cand &mine, Cand *sh)
{
    double d = mine.d;
    int32_t i = mine.idx;
    group_argmax<64>(d, i);
    const unsigned long long hit = __ballot(mine.idx == i);      // a point's index is held by one lane; an empty wave: every lane
    if (lane_id() == __builtin_ctzll(hit)) sh[wave_id()] = mine;
    __syncthreads();
    const Cand e = sh[lane_id() & (W - 1)];
    d = e.d;
    i = e.idx;
    group_argmax<W>(d, i);
    const unsigned long long h2 = __ballot(e.idx == i);
    return sh[__builtin_ctzll(h2) & (W - 1)];
}

__device__ __forceinline__ Cand no_cand() { return Cand{ -1.0, kNoIdx, 0.f, 0.f, 0.f }; }

struct FpsCloud {
    const float *pts;
    double *dist;          // running distances of the points beyond KPX_FPS_LDS_N
    int32_t *sel;
    double *cover;         // nullable
    int32_t n;
    int32_t pad;
};
struct FpsBatchArgs {
    FpsCloud c[kFpsBatch];
};

// ---- block form: one block per cloud ------------------------------------------------------------------------------------
// Thread t owns points r * T + t: r < kFpsReg in registers, then kFpsLds in LDS (SoA, slot l * T + t: conflict-free), then every
// T-th point from KPX_FPS_LDS_N on in global memory.  Its points are visited in ascending index, so a strict > keeps the smallest
// index among its equal distances.
__global__ __launch_bounds__(kFpsThreads) void fps_block_kernel(FpsBatchArgs args, int32_t k, int32_t start)
{
    __shared__ float lx[kFpsLds * kFpsThreads], ly[kFpsLds * kFpsThreads], lz[kFpsLds * kFpsThreads];
    __shared__ double ld[kFpsLds * kFpsThreads];
    __shared__ Cand part[2][kFpsWaves];
    const FpsCloud c = args.c[blockIdx.x];
    const int32_t n = c.n, t = threadIdx.x;
    const double inf = __builtin_huge_val();
    float rx[kFpsReg], ry[kFpsReg], rz[kFpsReg];
    double rd[kFpsReg];
#pragma unroll
    for (int r = 0; r < kFpsReg; ++r) {
        const int32_t j = r * kFpsThreads + t;
        rx[r] = ry[r] = rz[r] = 0.f;
        rd[r] = inf;
        if (j < n) { rx[r] = c.pts[3 * (int64_t)j]; ry[r] = c.pts[3 * (int64_t)j + 1]; rz[r] = c.pts[3 * (int64_t)j + 2]; }
    }
#pragma unroll
    for (int l = 0; l < kFpsLds; ++l) {
        const int32_t j = KPX_FPS_REG_N + l * kFpsThreads + t;
        if (j < n) {
            lx[l * kFpsThreads + t] = c.pts[3 * (int64_t)j];
            ly[l * kFpsThreads + t] = c.pts[3 * (int64_t)j + 1];
            lz[l * kFpsThreads + t] = c.pts[3 * (int64_t)j + 2];
            ld[l * kFpsThreads + t] = inf;
        }
    }
    for (int64_t j = (int64_t)KPX_FPS_LDS_N + t; j < n; j += kFpsThreads) c.dist[j - KPX_FPS_LDS_N] = inf;
    int32_t far = start;
    double sx = c.pts[3 * (int64_t)start], sy = c.pts[3 * (int64_t)start + 1], sz = c.pts[3 * (int64_t)start + 2];
    if (t == 0) c.sel[0] = start;
    for (int32_t i = 0; i < k; ++i) {
        Cand b = no_cand();
#pragma unroll
        for (int r = 0; r < kFpsReg; ++r) {
            const int32_t j = r * kFpsThreads + t;
            if (j < n) {
                const double d = ac3(rx[r], ry[r], rz[r], sx, sy, sz);
                const double m = d < rd[r] ? d : rd[r];
                rd[r] = m;
                if (m > b.d) b = Cand{ m, j, rx[r], ry[r], rz[r] };
            }
        }
#pragma unroll
        for (int l = 0; l < kFpsLds; ++l) {
            const int32_t j = KPX_FPS_REG_N + l * kFpsThreads + t;
            if (j < n) {
                const int s = l * kFpsThreads + t;
                const float x = lx[s], y = ly[s], z = lz[s];
                const double d = ac3(x, y, z, sx, sy, sz);
                const double o = ld[s], m = d < o ? d : o;
                ld[s] = m;
                if (m > b.d) b = Cand{ m, j, x, y, z };
            }
        }
        for (int64_t j = (int64_t)KPX_FPS_LDS_N + t; j < n; j += kFpsThreads) {
            const float x = c.pts[3 * j], y = c.pts[3 * j + 1], z = c.pts[3 * j + 2];
            const double d = ac3(x, y, z, sx, sy, sz);
            const double o = c.dist[j - KPX_FPS_LDS_N], m = d < o ? d : o;
            c.dist[j - KPX_FPS_LDS_N] = m;
            if (m > b.d) b = Cand{ m, (int32_t)j, x, y, z };
        }
        const Cand g = block_argmax<kFpsWaves>(b, part[i & 1]);
        if (g.d > 0.0) { far = g.idx; sx = g.x; sy = g.y; sz = g.z; }     // all dist 0: Open3D keeps the previous index
        if (t == 0) {
            if (c.cover) c.cover[i] = g.d;
            if (i + 1 < k) c.sel[i + 1] = far;
        }
    }
}

// ---- chain form: launch t of k + 1 over one large cloud ----------------------------------------------------------------
// cand: [2][ncand] (parity of t); state: [2].  t == k: the final launch (one block), which only writes cover[k - 1].
__global__ __launch_bounds__(kChainThreads) void fps_chain_kernel(const float *__restrict__ pts, int32_t n, int32_t per_block, int32_t t,
                                                                  int32_t k, int32_t start, double *__restrict__ dist, Cand *__restrict__ cand,
                                                                  int32_t ncand, ChainState *__restrict__ state, int32_t *__restrict__ sel,
                                                                  double *__restrict__ cover)
{
    __shared__ Cand sh_prev[kChainWaves], sh_own[kChainWaves];
    const int tid = threadIdx.x;
    const bool recorder = blockIdx.x == 0 && tid == 0;
    double sx, sy, sz;
    if (t == 0) {
        sx = pts[3 * (int64_t)start]; sy = pts[3 * (int64_t)start + 1]; sz = pts[3 * (int64_t)start + 2];
        if (recorder) { sel[0] = start; state[0] = ChainState{ start, (float)sx, (float)sy, (float)sz }; }
    } else {
        const Cand *prev = cand + (int64_t)((t - 1) & 1) * ncand;
        Cand b = no_cand();
        for (int q = tid; q < ncand; q += kChainThreads) {
            const Cand e = prev[q];
            if (better(e.d, e.idx, b.d, b.idx)) b = e;
        }
        const Cand g = block_argmax<kChainWaves>(b, sh_prev);
        int32_t far;
        if (g.d > 0.0) { far = g.idx; sx = g.x; sy = g.y; sz = g.z; }
        else {                                                            // all dist 0: the previous sample repeats
            const ChainState p = state[(t - 1) & 1];
            far = p.far; sx = p.x; sy = p.y; sz = p.z;
        }
        if (recorder) {
            if (cover) cover[t - 1] = g.d;
            if (t < k) { sel[t] = far; state[t & 1] = ChainState{ far, (float)sx, (float)sy, (float)sz }; }
        }
        if (t == k) return;                                               // block-uniform
    }
    const int64_t lo = (int64_t)blockIdx.x * per_block, hi = lo + per_block < n ? lo + per_block : n;
    Cand b = no_cand();
    for (int64_t j = lo + tid; j < hi; j += kChainThreads) {
        const float x = pts[3 * j], y = pts[3 * j + 1], z = pts[3 * j + 2];
        const double d = ac3(x, y, z, sx, sy, sz);
        const double m = t == 0 ? d : (d < dist[j] ? d : dist[j]);
        dist[j] = m;
        if (m > b.d) b = Cand{ m, (int32_t)j, x, y, z };
    }
    const Cand w = block_argmax<kChainWaves>(b, sh_own);
    if (tid == 0) cand[(int64_t)(t & 1) * ncand + blockIdx.x] = w;
}

// A/B switch for measurements: KPX_FPS_FORM=block / chain forces one form for every cloud (unset: by n)
int fps_forced_form()
{
    static const int mode = [] {
        const char *e = getenv("KPX_FPS_FORM");
        return !e ? -1 : (strcmp(e, "block") == 0 ? 0 : (strcmp(e, "chain") == 0 ? 1 : -1));
    }();
    return mode;
}
// mid: the batch's number of clouds with KPX_FPS_BLOCK_MAX_N < n <= KPX_FPS_BATCH_BLOCK_MAX_N (header: dispatch)
bool fps_use_block(int64_t n, int32_t mid)
{
    const int m = fps_forced_form();
    if (m >= 0) return m == 0;
    return n <= KPX_FPS_BLOCK_MAX_N || (mid >= KPX_FPS_BATCH_MIN_CLOUDS && n <= KPX_FPS_BATCH_BLOCK_MAX_N);
}

int chain_blocks()
{
    static const int cus = [] {
        int dev = 0, c = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c < 1) c = 256;
        return c;
    }();
    return cus < kChainMaxBlocks ? cus : kChainMaxBlocks;
}

size_t dist_stride(int64_t n_max) { return ((size_t)(n_max > 0 ? n_max : 1) + 31) & ~(size_t)31; }

int fps_impl(int32_t count, const float *const *h_pts, const int64_t *h_n, int64_t n_max, int32_t k, int32_t start, int32_t *const *h_sel,
             double *const *h_cover, Arena &a, hipStream_t st)
{
    double *dist = a.get<double>((size_t)(count > 0 ? count : 1) * dist_stride(n_max));
    Cand *cand = a.get<Cand>(2 * kChainMaxBlocks);
    ChainState *state = a.get<ChainState>(2);
    if (a.dry) return KPX_OK;
    KPX_ARENA_CHECK(a);
    const size_t stride = dist_stride(n_max);
    int32_t mid = 0;
    for (int32_t c = 0; c < count; ++c) mid += h_n[c] > KPX_FPS_BLOCK_MAX_N && h_n[c] <= KPX_FPS_BATCH_BLOCK_MAX_N;
    FpsBatchArgs args;
    int nb = 0;
    auto flush = [&]() -> int {
        if (!nb) return KPX_OK;
        hipLaunchKernelGGL(fps_block_kernel, dim3(nb), dim3(kFpsThreads), 0, st, args, k, start);
        nb = 0;
        KPX_LAUNCH_CHECK();
        return KPX_OK;
    };
    for (int32_t c = 0; c < count; ++c) {
        if (!fps_use_block(h_n[c], mid)) continue;
        args.c[nb++] = FpsCloud{ h_pts[c], dist + c * stride, h_sel[c], h_cover ? h_cover[c] : nullptr, (int32_t)h_n[c], 0 };
        if (nb == kFpsBatch) { int rc = flush(); if (rc) return rc; }
    }
    int rc = flush();
    if (rc) return rc;
    for (int32_t c = 0; c < count; ++c) {
        if (fps_use_block(h_n[c], mid)) continue;
        const int64_t n = h_n[c];
        int64_t g = cdiv(n, (int64_t)kChainThreads * kChainPerThread);
        if (g > chain_blocks()) g = chain_blocks();
        const int32_t per_block = (int32_t)cdiv(n, g);
        g = cdiv(n, per_block);
        double *cover = h_cover ? h_cover[c] : nullptr;
        for (int32_t t = 0; t < k; ++t)
            hipLaunchKernelGGL(fps_chain_kernel, dim3((unsigned)g), dim3(kChainThreads), 0, st, h_pts[c], (int32_t)n, per_block, t, k, start,
                               dist + c * stride, cand, (int32_t)g, state, h_sel[c], cover);
        if (cover)
            hipLaunchKernelGGL(fps_chain_kernel, dim3(1), dim3(kChainThreads), 0, st, h_pts[c], (int32_t)n, per_block, k, k, start,
                               dist + c * stride, cand, (int32_t)g, state, h_sel[c], cover);
        KPX_LAUNCH_CHECK();
    }
    return KPX_OK;
}

int fps_check(int32_t count, const float *const *h_pts, const int64_t *h_n, int32_t k, int32_t start, int32_t *const *h_sel, int64_t *n_max)
{
    KPX_REQUIRE(count >= 0 && (count == 0 || h_n), "kpx_farthest_point_sample: bad batch");
    KPX_REQUIRE(k >= 0, "Illegal number of samples: %d", k);
    *n_max = 0;
    for (int32_t c = 0; c < count; ++c) {
        const int64_t n = h_n[c];
        KPX_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "kpx_farthest_point_sample: bad size");
        KPX_REQUIRE(k <= n, "Illegal number of samples: %d, must <= point size: %lld", k, (long long)n);
        KPX_REQUIRE(k == 0 || (start >= 0 && start < n), "Illegal start index: %d, must <= point size: %lld", start, (long long)n);
        if (k) KPX_REQUIRE(h_pts && h_sel && h_pts[c] && h_sel[c], "kpx_farthest_point_sample: null pointer");
        if (n > *n_max) *n_max = n;
    }
    return KPX_OK;
}

}  // namespace

}  // namespace kpx

using namespace kpx;

KPX_EXPORT size_t kpx_fps_workspace_bytes(int32_t count, int64_t n_max)
{
    Arena a(nullptr, 0);
    fps_impl(count, nullptr, nullptr, n_max, 0, 0, nullptr, nullptr, a, nullptr);
    return a.off;
}

KPX_EXPORT int kpx_farthest_point_sample_batch(int32_t count, const float *const *h_pts, const int64_t *h_n, int32_t k, int32_t start_index,
                                               int32_t *const *h_sel, double *const *h_cover, void *ws, size_t ws_bytes, void *stream)
{
    int64_t n_max = 0;
    int rc = fps_check(count, h_pts, h_n, k, start_index, h_sel, &n_max);
    if (rc) return rc;
    if (k == 0 || count == 0) return KPX_OK;
    KPX_REQUIRE(ws, "kpx_farthest_point_sample: null workspace");
    Arena a(ws, ws_bytes);
    return fps_impl(count, h_pts, h_n, n_max, k, start_index, h_sel, h_cover, a, (hipStream_t)stream);
}

KPX_EXPORT int kpx_farthest_point_sample(const float *pts, int64_t n, int32_t k, int32_t start_index, int32_t *sel, double *cover, void *ws,
                                         size_t ws_bytes, void *stream)
{
    return kpx_farthest_point_sample_batch(1, &pts, &n, k, start_index, &sel, &cover, ws, ws_bytes, stream);
}
