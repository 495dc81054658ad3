// kpx_pointnet.hip -- inference of the reference's PointNet joint regressor (models/pointnet.py: create_pointnet) and the
// evaluation metrics of evaluate.py (metrics/metric.py: percentual_correct_keypoints, the mean squared error).  Arithmetic
// contract AC18, DESIGN.md 5.19.
//   trunk:   one kernel template for the three point-wise trunks (tnet(3), tnet(32), the main one).  A wave owns 64 points of one
//            cloud, lane = point.  The narrow layers (3 -> 32, 32 -> 32, 32 -> 64, the per-cloud T3 and T32) run on the vector unit:
//            a lane keeps the accumulators of all output channels of its point in registers, the weights of an input channel are
//            wave-uniform (scalar loads), and the layer's input is read back from the lane's own LDS column with a run-time
//            channel index.  The 64 -> 512 layer (89 % of the arithmetic) runs on v_mfma_f32_32x32x2_f32 with the POINTS on the
//            rows: D[point][channel], so the maximum over the points is a maximum over the 16 accumulator registers of a lane,
//            one exchange between the lane halves, and one integer atomicMax per channel -- nothing of B x N x 512 reaches memory.
//            Trunks 2 and 3 recompute x.T3, 3 -> 32, 32 -> 32 (pn_front) from the raw points.
//   padding: a lane past the end of its cloud loads the cloud's LAST point again: a duplicate cannot change a maximum, a
//            zero-filled row (the point (0,0,0), whose activations are positive) can.
//   head:    one block per cloud: 512 -> 256 -> 128 -> width (9, 1024 or 3 J), K split over thread groups and summed in a fixed order.
//   metrics: counts by 64-bit atomic adds (exact), the squared error by one block in a fixed order.
#include "kpx_common.h"
#include "kpx_pointnet.h"

namespace kpx {

constexpr int kPnHeadThreads = 512;

// out[j] = (b[j]) + sum_k x[k] W[k][j], three input channels held in registers
template <int COUT, bool BIAS, bool RELU>
__device__ __forceinline__ void pn_layer3(const float (&x)[3], const float *__restrict__ W, const float *__restrict__ b, float (&out)[COUT])
{
#pragma unroll
    for (int j = 0; j < COUT; ++j) {
        float v = BIAS ? b[j] : 0.0f;
        v = fmaf(x[0], W[j], v);
        v = fmaf(x[1], W[COUT + j], v);
        v = fmaf(x[2], W[2 * COUT + j], v);
        out[j] = RELU ? pn_relu(v) : v;
    }
}

// the same for CIN input channels read from the lane's LDS column col[k * 64]; W and b are wave-uniform
template <int CIN, int COUT, bool BIAS, bool RELU>
__device__ __forceinline__ void pn_layer(const float *col, const float *__restrict__ W, const float *__restrict__ b, float (&out)[COUT])
{
#pragma unroll
    for (int j = 0; j < COUT; ++j) out[j] = BIAS ? b[j] : 0.0f;
#pragma unroll 2
    for (int k = 0; k < CIN; ++k) {
        const float v = col[k * 64];
        const float *__restrict__ w = W + k * COUT;
#pragma unroll
        for (int j = 0; j < COUT; ++j) out[j] = fmaf(v, w[j], out[j]);
    }
    if (RELU) {
#pragma unroll
        for (int j = 0; j < COUT; ++j) out[j] = pn_relu(out[j]);
    }
}
template <int C> __device__ __forceinline__ void pn_store(float *col, const float (&v)[C])
{
#pragma unroll
    for (int j = 0; j < C; ++j) col[j * 64] = v[j];
}

struct PnTrunkArgs {
    const float *pts;                    // [B][n][3]
    int64_t n;
    int32_t tiles;                       // 64-point tiles per cloud
    int32_t chunks;                      // 32-channel chunks of the last layer per blockIdx.y
    const float *T3, *T32;               // [B][9], [B][1024] (trunks 2, 3 / trunk 3)
    const float *wf1, *bf1, *wf2, *bf2;  // the shared front: 3 -> 32, 32 -> 32
    const float *wa, *ba;                // the trunk's own first layer: 3 -> 32 (trunk 1) or 32 -> 32
    const float *wb, *bb;                // 32 -> 64
    const float *wc, *bc;                // 64 -> 512, in the operand order of the matrix instruction (kinectpx.h)
    int32_t *g;                          // [B][512] bit patterns of the maxima, cleared to +0
};

// x.T3 -> 3 -> 32 -> 32: the 32 features the second T-net and the main trunk start from, left in the lane's LDS column
__device__ __forceinline__ void pn_front(const float (&x)[3], const float *__restrict__ T3, const PnTrunkArgs &a, float *col)
{
    float xt[3], f[32];
    pn_layer3<3, false, false>(x, T3, nullptr, xt);
    pn_layer3<32, true, true>(xt, a.wf1, a.bf1, f);
    pn_store<32>(col, f);
    pn_layer<32, 32, true, true>(col, a.wf2, a.bf2, f);
    pn_store<32>(col, f);
}

// KIND 0: tnet(3) on the raw points; 1: tnet(32) on the front's features; 2: the main trunk on the features times T32
template <int KIND>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void pn_trunk_kernel(PnTrunkArgs a)
{
    __shared__ float lds[32 * 64];
    const int lane = threadIdx.x;
    const int64_t cloud = blockIdx.x / a.tiles;
    const int64_t tile = blockIdx.x % a.tiles;
    float *col = lds + lane;

    int64_t p = tile * 64 + lane;
    if (p >= a.n) p = a.n - 1;                                   // a duplicate of the last point, never a zero row
    const float *src = a.pts + (cloud * a.n + p) * 3;
    const float x[3] = { src[0], src[1], src[2] };

    float h2[64];
    {
        float h1[32];
        if (KIND == 0) {
            pn_layer3<32, true, true>(x, a.wa, a.ba, h1);
        } else {
            pn_front(x, a.T3 + cloud * 9, a, col);
            if (KIND == 2) {
                pn_layer<32, 32, false, false>(col, a.T32 + cloud * 1024, nullptr, h1);
                pn_store<32>(col, h1);
            }
            pn_layer<32, 32, true, true>(col, a.wa, a.ba, h1);
        }
        pn_store<32>(col, h1);
        pn_layer<32, 64, true, true>(col, a.wb, a.bb, h2);
    }

    // A operands of the two 32-point tiles: lane l of tile t holds h2[point 32 t + (l & 31)][k = 2 s + (l >> 5)]
    const bool upper = lane >= 32;
    float a0[32], a1[32];
#pragma unroll
    for (int s = 0; s < 32; ++s) {
        const float lo = h2[2 * s], hi = h2[2 * s + 1];
        const float got = __shfl_xor(upper ? lo : hi, 32, 64);
        a0[s] = upper ? got : lo;
        a1[s] = upper ? hi : got;
    }

    int32_t *g = a.g + cloud * kPnFeat;
    const int c0 = blockIdx.y * a.chunks;
    // B operands of a chunk: eight 16-byte loads per lane; the next chunk's are in flight while this one's products issue
    const float4 *wp = reinterpret_cast<const float4 *>(a.wc) + (int64_t)c0 * 8 * 64 + lane;
    float4 next[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) next[q] = wp[q * 64];
    for (int c = c0; c < c0 + a.chunks; ++c) {
        float bv[32];
#pragma unroll
        for (int q = 0; q < 8; ++q) { bv[4 * q] = next[q].x; bv[4 * q + 1] = next[q].y; bv[4 * q + 2] = next[q].z; bv[4 * q + 3] = next[q].w; }
        if (c + 1 < c0 + a.chunks) {
            wp += 8 * 64;
#pragma unroll
            for (int q = 0; q < 8; ++q) next[q] = wp[q * 64];
        }
        pn_f32x16 acc0 = { 0 }, acc1 = { 0 };
#pragma unroll
        for (int s = 0; s < 32; ++s) {
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], bv[s], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], bv[s], acc1, 0, 0, 0);
        }
        float m = fmaxf(acc0[0], acc1[0]);
#pragma unroll
        for (int r = 1; r < 16; ++r) m = fmaxf(m, fmaxf(acc0[r], acc1[r]));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        // the bias after the maximum: rounding is monotone, so max_p fl(v_p + b) == fl(max_p v_p + b)
        const int ch = 32 * c + (lane & 31);
        const int32_t bits = __float_as_int(pn_relu(m + a.bc[ch]));
        if (!upper && bits > __hip_atomic_load(g + ch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(g + ch, bits);
    }
}

// sum_k in[k] w[k stride], len a multiple of 4: four interleaved chains (k mod 4), summed (0 + 1) + (2 + 3) -- four loads in flight, and
// chains a quarter as long round less
__device__ __forceinline__ float pn_dot4(const float *in, const float *__restrict__ w, int stride, int len)
{
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll 2
    for (int k = 0; k < len; k += 4) {
        a0 = fmaf(in[k], w[(int64_t)k * stride], a0);
        a1 = fmaf(in[k + 1], w[(int64_t)(k + 1) * stride], a1);
        a2 = fmaf(in[k + 2], w[(int64_t)(k + 2) * stride], a2);
        a3 = fmaf(in[k + 3], w[(int64_t)(k + 3) * stride], a3);
    }
    return (a0 + a1) + (a2 + a3);
}

// out[j] = act(b[j] + sum_k in[k] W[k][j]) for COUT <= kPnHeadThreads outputs: kPnHeadThreads / COUT thread groups take a slice of k each,
// the slices are summed in ascending order.  All threads call; in / out / part are LDS.
template <int CIN, int COUT>
__device__ __forceinline__ void pn_dense_relu(const float *in, const float *__restrict__ W, const float *__restrict__ b, float *out, float *part)
{
    constexpr int kSlices = kPnHeadThreads / COUT, kLen = CIN / kSlices;
    const int j = threadIdx.x % COUT, sl = threadIdx.x / COUT;
    part[threadIdx.x] = pn_dot4(in + sl * kLen, W + (int64_t)sl * kLen * COUT + j, COUT, kLen);
    __syncthreads();
    if (threadIdx.x < COUT) {
        float v = part[threadIdx.x];
#pragma unroll
        for (int s = 1; s < kSlices; ++s) v += part[s * COUT + threadIdx.x];
        out[threadIdx.x] = pn_relu(v + b[threadIdx.x]);
    }
    __syncthreads();
}

__global__ __launch_bounds__(kPnHeadThreads) void pn_head_kernel(const int32_t *__restrict__ g, const float *__restrict__ w1, const float *__restrict__ b1,
                                                                 const float *__restrict__ w2, const float *__restrict__ b2, const float *__restrict__ w3,
                                                                 const float *__restrict__ b3, int width, float *__restrict__ out)
{
    __shared__ float s_in[kPnFeat], s_part[kPnHeadThreads], s_h1[256], s_h2[128];
    const int64_t cloud = blockIdx.x;
    s_in[threadIdx.x] = __int_as_float(g[cloud * kPnFeat + threadIdx.x]);
    __syncthreads();
    pn_dense_relu<512, 256>(s_in, w1, b1, s_h1, s_part);
    pn_dense_relu<256, 128>(s_h1, w2, b2, s_h2, s_part);
    for (int j = threadIdx.x; j < width; j += kPnHeadThreads) {
        out[cloud * width + j] = pn_dot4(s_h2, w3 + j, width, 128) + b3[j];
    }
}

// ---- metrics --------------------------------------------------------------------------------------------------------------------------
struct PnThresholds {
    float t[KPX_METRICS_MAX_THRESHOLDS];
};
constexpr int kPnMetricThreads = 1024;
// blockIdx.y < nt: the count of threshold blockIdx.y over this block's grid-stride share; blockIdx.y == nt, blockIdx.x == 0: the squared
// error, thread t summing elements t, t + 1024, ... in ascending order, then the block's fixed-order sum
__global__ __launch_bounds__(kPnMetricThreads) void pn_metrics_kernel(const float *__restrict__ yt, const float *__restrict__ yp, int64_t n, PnThresholds thr,
                                                                      int nt, unsigned long long *__restrict__ counts, double *__restrict__ sum_sq)
{
    if ((int)blockIdx.y == nt) {
        __shared__ double shd[kPnMetricThreads / 64];
        if (blockIdx.x != 0) return;
        double s = 0.0;
        for (int64_t i = threadIdx.x; i < n; i += kPnMetricThreads) {
            const double d = (double)(yp[i] - yt[i]);
            s += d * d;
        }
        s = block_sum(s, shd);
        if (threadIdx.x == 0) *sum_sq = s;
        return;
    }
    __shared__ unsigned long long shc[kPnMetricThreads / 64];
    const float t = thr.t[blockIdx.y];
    unsigned long long c = 0;
    for (int64_t i = (int64_t)blockIdx.x * kPnMetricThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kPnMetricThreads)
        c += fabsf(yp[i] - yt[i]) <= t ? 1ull : 0ull;
    c = block_sum(c, shc);
    if (threadIdx.x == 0 && c) atomicAdd(counts + blockIdx.y, c);
}

struct PnScratch {
    int32_t *g;          // [3][B][512]
    float *T3, *T32;     // [B][9], [B][1024]
};
static void pn_carve(Arena &a, int64_t batch, PnScratch *s)
{
    const size_t b = (size_t)(batch > 0 ? batch : 1);
    s->g = a.get<int32_t>(3 * b * kPnFeat);
    s->T3 = a.get<float>(b * 9);
    s->T32 = a.get<float>(b * 1024);
}

}  // namespace kpx

using namespace kpx;

KPX_EXPORT size_t kpx_pointnet_workspace_bytes(int32_t batch, int64_t n, int32_t joints)
{
    if (batch < 0 || n < 1 || joints < 1 || 3 * (int64_t)joints > KPX_POINTNET_MAX_OUT || (int64_t)batch * n >= ((int64_t)1 << 31) || n >= ((int64_t)1 << 31)) return 0;
    Arena a(nullptr, 0);
    PnScratch s;
    pn_carve(a, batch, &s);
    return a.off;
}

KPX_EXPORT int kpx_pointnet_forward(const float *weights, int64_t weights_floats, const float *pts, int32_t batch, int64_t n, int32_t joints, float *out,
                                    float *T3, float *T32, float *g1, float *g2, float *g3, void *ws, size_t ws_bytes, void *stream)
{
    const int rc = pn_size_check("kpx_pointnet_forward", batch, n, joints);
    if (rc) return rc;
    const PnLayout L = pn_layout(joints);
    KPX_REQUIRE(weights_floats == L.total, "kpx_pointnet_forward: the packed weights of %d joints hold %lld floats, not %lld", (int)joints, (long long)L.total,
                (long long)weights_floats);
    if (batch == 0) return KPX_OK;
    KPX_REQUIRE(weights && pts && out && ws, "kpx_pointnet_forward: null pointer");
    KPX_REQUIRE(((uintptr_t)weights % 16) == 0, "kpx_pointnet_forward: the packed weights must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    Arena a(ws, ws_bytes);
    PnScratch s;
    pn_carve(a, batch, &s);
    KPX_ARENA_CHECK(a);

    const size_t gbytes = (size_t)batch * kPnFeat * sizeof(int32_t);
    int32_t *g[3] = { g1 ? (int32_t *)g1 : s.g, g2 ? (int32_t *)g2 : s.g + (size_t)batch * kPnFeat, g3 ? (int32_t *)g3 : s.g + 2 * (size_t)batch * kPnFeat };
    if (!g1 && !g2 && !g3) {
        KPX_HIP(hipMemsetAsync(s.g, 0, 3 * gbytes, st));
    } else {
        for (int t = 0; t < 3; ++t) KPX_HIP(hipMemsetAsync(g[t], 0, gbytes, st));
    }
    float *t3 = T3 ? T3 : s.T3, *t32 = T32 ? T32 : s.T32;

    PnTrunkArgs ta;
    ta.pts = pts;
    ta.n = n;
    ta.tiles = (int32_t)cdiv(n, 64);
    // Few tiles: the last layer's channel chunks go to several waves, each recomputing the narrow layers (11 % of the work), until
    // every SIMD of the device has a wave.  The split changes who computes a channel, never the channel's value.
    const int64_t waves = (int64_t)ta.tiles * batch;
    int split = 1;
    while (split < 4 && waves * split < 1024) split *= 2;
    ta.chunks = kPnChunks / split;
    ta.T3 = t3;
    ta.T32 = t32;
    ta.wf1 = weights + L.w[6]; ta.bf1 = weights + L.b[6];
    ta.wf2 = weights + L.w[7]; ta.bf2 = weights + L.b[7];
    const dim3 grid((unsigned)waves, (unsigned)split);
    const float *W = weights;
    float *head_out[3] = { t3, t32, out };
    const int head_w[3] = { 9, 1024, 3 * joints };
    for (int t = 0; t < 3; ++t) {
        const int l0 = t == 0 ? 0 : t == 1 ? 8 : 14;                    // the trunk's three layers, then the head's three
        ta.wa = W + L.w[l0]; ta.ba = W + L.b[l0];
        ta.wb = W + L.w[l0 + 1]; ta.bb = W + L.b[l0 + 1];
        ta.wc = W + L.w[l0 + 2]; ta.bc = W + L.b[l0 + 2];
        ta.g = g[t];
        if (t == 0) hipLaunchKernelGGL(pn_trunk_kernel<0>, grid, dim3(64), 0, st, ta);
        else if (t == 1) hipLaunchKernelGGL(pn_trunk_kernel<1>, grid, dim3(64), 0, st, ta);
        else hipLaunchKernelGGL(pn_trunk_kernel<2>, grid, dim3(64), 0, st, ta);
        hipLaunchKernelGGL(pn_head_kernel, dim3((unsigned)batch), dim3(kPnHeadThreads), 0, st, (const int32_t *)g[t], W + L.w[l0 + 3], W + L.b[l0 + 3],
                           W + L.w[l0 + 4], W + L.b[l0 + 4], W + L.w[l0 + 5], W + L.b[l0 + 5], head_w[t], head_out[t]);
    }
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT int kpx_joint_metrics(const float *y_true, const float *y_pred, int64_t n, const double *h_thresholds, int32_t n_thresholds, int64_t *d_counts,
                                 double *d_sum_sq, void *stream)
{
    KPX_REQUIRE(n >= 0, "kpx_joint_metrics: negative size");
    KPX_REQUIRE(n_thresholds >= 0 && n_thresholds <= KPX_METRICS_MAX_THRESHOLDS, "kpx_joint_metrics: %d thresholds: at most %d", (int)n_thresholds,
                KPX_METRICS_MAX_THRESHOLDS);
    KPX_REQUIRE(d_sum_sq && (n_thresholds == 0 || (h_thresholds && d_counts)) && (n == 0 || (y_true && y_pred)), "kpx_joint_metrics: null pointer");
    PnThresholds thr;
    for (int t = 0; t < KPX_METRICS_MAX_THRESHOLDS; ++t) thr.t[t] = t < n_thresholds ? (float)h_thresholds[t] : 0.0f;
    hipStream_t st = (hipStream_t)stream;
    if (n_thresholds) KPX_HIP(hipMemsetAsync(d_counts, 0, (size_t)n_thresholds * sizeof(int64_t), st));
    const int64_t blocks = cdiv(n > 0 ? n : 1, (int64_t)kPnMetricThreads * 8);
    hipLaunchKernelGGL(pn_metrics_kernel, dim3((unsigned)(blocks > 1024 ? 1024 : blocks), (unsigned)n_thresholds + 1), dim3(kPnMetricThreads), 0, st, y_true, y_pred,
                       n, thr, (int)n_thresholds, (unsigned long long *)d_counts, d_sum_sq);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}
