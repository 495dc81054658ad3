// kpx_pointnet_train.hip -- one training step of the reference's PointNet joint regressor (models/pointnet.py under train.py's model.fit):
// train-mode forward, loss, backward and Adam.  Arithmetic contract AC19, DESIGN.md 5.20.
//   Batch statistics put a grid-wide dependency between the layers, so the step is a chain of launches on the caller's stream with no
//   host read-back.  Every cross-point / cross-row sum is per-block partial sums (float32, fixed order inside the block) combined by one
//   thread per output in ascending block order (in float64, rounded once): no floating-point atomics, two runs give the same bits.
//   narrow layers (<= 64 channels): pt_fwd_kernel stores the pre-activations z (B N c floats); batch normalisation and ReLU are applied
//            when the next kernel loads them.  pt_bwd_stats / pt_coef / pt_bwd are the two-sum batch-normalisation backward, dX, and dW / db
//            as per-block partials (pt_reduce).  x T3 and f T32 are the same kernels with a per-cloud W and no batch normalisation.
//   64 -> 512: forward on v_mfma_f32_32x32x2_f32 with the points on the rows (pt_wide_kernel).  Nothing of B N 512 is stored: per channel
//            the kernel leaves the partial sums of z and z^2, and per (cloud, channel) one 64-bit atomicMax of (ordered bits of sign(gamma) z,
//            complemented point index) -- BN + ReLU is monotone in z, so that is the pooled point, lowest index on equal z.
//            Backward: the pooled gradient is non-zero at one point per (cloud, channel), so with dz = S - alpha - beta (z - mean) (S sparse,
//            alpha and beta per channel, z - mean = (h - hbar) W, hbar the mean input row) the dense parts collapse onto the 64 x 64
//            covariance of the layer's input:
//              dW = h^T S - s1 alpha^T - (h^T h - s1 hbar^T) W diag(beta),     dh = S W^T - (h - hbar) (W diag(beta) W^T) - 1 (alpha^T W^T)
//            (s1 = the column sums of h): no 512-wide product is taken in the backward pass at all.
//   heads:   B rows: one thread per output channel walks the rows (hd_dense, hd_bn, hd_bwd_bn), one block per input channel takes dW's row
//            and dX's column (hd_bwd_w); the regulariser and its gradient are one block per row of the (B f) x (B f) Gram matrix.
//   Adam:    one element-wise launch over the trainable buffer, evaluated in float64 and rounded once per stored value.
#include "kpx_common.h"
#include "kpx_pointnet.h"

namespace kpx {

constexpr int kPtThreads = 256;
constexpr int kPtStat = 4 * kPnFeat;            // a layer's statistics block: mean, 1 / sqrt(var + eps), scale = gamma rstd, beta
constexpr double kPtEps = 1e-3;
constexpr float kPtInvKeep = 1.0f / 0.7f;
constexpr uint32_t kPtKeepBelow = 11744051u;    // floor(0.7 2^24)

static inline bool pt_has_bn(int l) { return l != 5 && l != 13 && l != 19; }

struct PtLayout {
    int64_t w[kPnLayers], b[kPnLayers], gamma[kPnLayers], beta[kPnLayers], mean[kPnLayers], var[kPnLayers], trainable, total;
};
static PtLayout pt_layout(int joints)
{
    PtLayout L;
    int64_t off = 0;
    for (int l = 0; l < kPnLayers; ++l) {
        const int64_t co = pn_cout(l, joints);
        L.w[l] = off; off += pn_padded((int64_t)kPnCin[l] * co);
        L.b[l] = off; off += pn_padded(co);
        L.gamma[l] = L.beta[l] = -1;
        if (pt_has_bn(l)) {
            L.gamma[l] = off; off += pn_padded(co);
            L.beta[l] = off; off += pn_padded(co);
        }
    }
    L.trainable = off;
    for (int l = 0; l < kPnLayers; ++l) {
        L.mean[l] = L.var[l] = -1;
        if (pt_has_bn(l)) {
            const int64_t co = pn_cout(l, joints);
            L.mean[l] = off; off += pn_padded(co);
            L.var[l] = off; off += pn_padded(co);
        }
    }
    L.total = off;
    return L;
}

// relu(gamma (z - mean) / sqrt(var + eps) + beta) from a statistics block: the mean is taken off first (z scale + shift cancels when |mean| >> sigma)
__device__ __forceinline__ float pt_act(float z, const float *__restrict__ stat, int j)
{
    return pn_relu(fmaf(z - stat[j], stat[2 * kPnFeat + j], stat[3 * kPnFeat + j]));
}

__device__ __forceinline__ uint32_t pt_mix(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
// the dropout keep decision of (seed, step, layer, row, channel): AC19
__device__ __forceinline__ bool pt_keep(uint32_t seed, uint32_t step, uint32_t layer, uint32_t row, uint32_t channel)
{
    const uint32_t h = pt_mix(pt_mix(pt_mix(pt_mix(seed) ^ step) ^ layer) ^ (row * 512u + channel));
    return (h >> 8) < kPtKeepBelow;
}

// mean / variance -> the statistics block and the moving statistics (momentum 0: moving = batch)
__device__ __forceinline__ void pt_bn_finish(double mean, double var, int j, const float *__restrict__ gamma, const float *__restrict__ beta, float *__restrict__ stat,
                                             float *__restrict__ mov_mean, float *__restrict__ mov_var)
{
    const float fm = (float)mean, fv = (float)(var > 0.0 ? var : 0.0);
    const float rstd = (float)(1.0 / sqrt((double)fv + kPtEps));
    const float scale = gamma[j] * rstd;
    stat[j] = fm;
    stat[kPnFeat + j] = rstd;
    stat[2 * kPnFeat + j] = scale;
    stat[3 * kPnFeat + j] = beta[j];
    mov_mean[j] = fm;
    mov_var[j] = fv;
}

// ---- narrow point-wise layers ----------------------------------------------------------------------------------------------------------
struct PtFwdArgs {
    const float *src;          // [B n][cin]
    const float *in_stat;      // the statistics block of the layer that wrote src (BN + ReLU on load), or null: src as it is
    const float *W;            // [cin][cout], cloud c reads W + c wstride
    int64_t wstride;
    const float *bias;         // [cout] or null
    float *dst;                // [B n][cout]
    const float *in_center;    // [cin] subtracted from the loaded (activated) input, or null
    double *part;              // [B tiles][2][cout] sums of z and z^2 (float64), or null
    int64_t n;
    int32_t tiles, cin, cout;  // cin, cout <= 64
};
// a block takes 64 points of one cloud: the inputs transposed into LDS [k][64], thread (point, channel group) sums over k
__global__ __launch_bounds__(kPtThreads) void pt_fwd_kernel(PtFwdArgs a)
{
    __shared__ float s_in[64 * 64], s_z[64 * 65];
    const int tid = threadIdx.x;
    const int64_t cloud = blockIdx.x / a.tiles, p0 = (int64_t)(blockIdx.x % a.tiles) * 64;
    const int cnt = (int)(a.n - p0 < 64 ? a.n - p0 : 64);
    const int64_t base = cloud * a.n + p0;
    const int cin = a.cin, cout = a.cout;
    for (int e = tid; e < 64 * cin; e += kPtThreads) {
        const int p = e / cin, k = e % cin;
        float v = 0.0f;
        if (p < cnt) {
            v = a.src[base * cin + e];
            if (a.in_stat) v = pt_act(v, a.in_stat, k);
            if (a.in_center) v -= a.in_center[k];
        }
        s_in[k * 64 + p] = v;
    }
    __syncthreads();
    const float *__restrict__ W = a.W + cloud * a.wstride;
    const int p = tid & 63;
    for (int j = tid >> 6; j < cout; j += kPtThreads / 64) {
        float acc = a.bias ? a.bias[j] : 0.0f;
        for (int k = 0; k < cin; ++k) acc = fmaf(s_in[k * 64 + p], W[k * cout + j], acc);
        s_z[j * 65 + p] = acc;
    }
    __syncthreads();
    for (int e = tid; e < cnt * cout; e += kPtThreads) a.dst[base * cout + e] = s_z[(e % cout) * 65 + e / cout];
    if (a.part && tid < cout) {
        double s1 = 0.0, s2 = 0.0;
        for (int q = 0; q < cnt; ++q) {
            const double v = (double)s_z[tid * 65 + q];
            s1 += v;
            s2 += v * v;
        }
        a.part[((int64_t)blockIdx.x * 2) * cout + tid] = s1;
        a.part[((int64_t)blockIdx.x * 2 + 1) * cout + tid] = s2;
    }
}

// The two partial sums per channel of `blocks` blocks, combined in a fixed order: a block takes 64 channels, thread (channel, slice s) adds
// the partials of blocks s, s + 16, ... in ascending order, the 16 slices are added in ascending order.  Valid for tid < 64 (slice 0).
constexpr int kPtSlices = 16;
__device__ __forceinline__ void pt_combine2(const double *__restrict__ part, int32_t blocks, int32_t cout, int j, double *s1, double *s2)
{
    __shared__ double sh[2][kPtSlices][64];
    const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
    double a = 0.0, b = 0.0;
    if (j < cout) {
        for (int64_t q = sl; q < blocks; q += kPtSlices) {
            a += part[(q * 2) * cout + j];
            b += part[(q * 2 + 1) * cout + j];
        }
    }
    sh[0][sl][lane] = a;
    sh[1][sl][lane] = b;
    __syncthreads();
    a = b = 0.0;
    if (sl == 0) {
        for (int q = 0; q < kPtSlices; ++q) {
            a += sh[0][q][lane];
            b += sh[1][q][lane];
        }
    }
    *s1 = a;
    *s2 = b;
}

// the partial sums of z and z^2 -> the layer's statistics
__global__ __launch_bounds__(64 * kPtSlices) void pt_stat_kernel(const double *__restrict__ part, int32_t blocks, int32_t cout, double count, const float *__restrict__ gamma,
                                                                 const float *__restrict__ beta, float *__restrict__ stat, float *__restrict__ mov_mean,
                                                                 float *__restrict__ mov_var)
{
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    double s1, s2;
    pt_combine2(part, blocks, cout, j, &s1, &s2);
    if (threadIdx.x >= 64 || j >= cout) return;
    const double mean = s1 / count;
    pt_bn_finish(mean, s2 / count - mean * mean, j, gamma, beta, stat, mov_mean, mov_var);
}

// upstream gradient of a layer's activation -> dy = [activation > 0] d (in place) and the partial sums of dy and dy xhat
__global__ __launch_bounds__(kPtThreads) void pt_bwd_stats_kernel(const float *__restrict__ z, const float *__restrict__ stat, float *__restrict__ dy, double *__restrict__ part,
                                                                  int64_t n, int32_t tiles, int32_t cout)
{
    __shared__ float s_d[64 * 65], s_x[64 * 65];
    const int tid = threadIdx.x;
    const int64_t cloud = blockIdx.x / tiles, p0 = (int64_t)(blockIdx.x % tiles) * 64;
    const int cnt = (int)(n - p0 < 64 ? n - p0 : 64);
    const int64_t base = (cloud * n + p0) * cout;
    for (int e = tid; e < cnt * cout; e += kPtThreads) {
        const int p = e / cout, j = e % cout;
        const float zv = z[base + e];
        const float d = pt_act(zv, stat, j) > 0.0f ? dy[base + e] : 0.0f;
        dy[base + e] = d;
        s_d[j * 65 + p] = d;
        s_x[j * 65 + p] = d * ((zv - stat[j]) * stat[kPnFeat + j]);
    }
    __syncthreads();
    if (tid < cout) {
        double s1 = 0.0, s2 = 0.0;
        for (int q = 0; q < cnt; ++q) {
            s1 += (double)s_d[tid * 65 + q];
            s2 += (double)s_x[tid * 65 + q];
        }
        part[((int64_t)blockIdx.x * 2) * cout + tid] = s1;
        part[((int64_t)blockIdx.x * 2 + 1) * cout + tid] = s2;
    }
}

// -> d beta, d gamma and the two means the backward needs: coef[j] = d beta / count, coef[512 + j] = d gamma / count
__global__ __launch_bounds__(64 * kPtSlices) void pt_coef_kernel(const double *__restrict__ part, int32_t blocks, int32_t cout, double count, float *__restrict__ g_gamma,
                                                                 float *__restrict__ g_beta, float *__restrict__ coef)
{
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    double s1, s2;
    pt_combine2(part, blocks, cout, j, &s1, &s2);
    if (threadIdx.x >= 64 || j >= cout) return;
    g_beta[j] = (float)s1;
    g_gamma[j] = (float)s2;
    coef[j] = (float)(s1 / count);
    coef[kPnFeat + j] = (float)(s2 / count);
}

struct PtBwdArgs {
    const float *in;           // the layer's input [B n][cin]
    const float *in_stat;      // its producer's statistics (BN + ReLU on load) or null
    const float *z;            // the layer's pre-activations [B n][cout]        (stat != null)
    const float *stat, *coef;  // the layer's statistics and backward means, or null: dz = dy (no batch normalisation)
    const float *dy;           // [B n][cout]
    const float *W;            // [cin][cout] (+ cloud wstride)
    int64_t wstride;
    float *din;                // [B n][cin] gradient of the input, or null
    int32_t din_accum;         // add to din instead of writing it
    float *partW, *partb;      // [B groups][cin cout], [B groups][cout]
    int64_t n;
    int32_t tiles, cin, cout;  // cin cout <= 4096
    int32_t gram;              // 1: dz := the input itself (cout = cin): partW = in^T in, partb = the column sums of in
};
// grid (groups, B): block (g, cloud) walks tiles g, g + groups, ... of its cloud in ascending order; thread e owns dW elements e + 256 q
__global__ __launch_bounds__(kPtThreads) void pt_bwd_kernel(PtBwdArgs a)
{
    __shared__ float s_in[64 * 64], s_dz[64 * 65];
    const int tid = threadIdx.x;
    const int cin = a.cin, cout = a.cout, nw = cin * cout;
    const int64_t cloud = blockIdx.y;
    const float *__restrict__ W = a.W ? a.W + cloud * a.wstride : nullptr;
    float acc[16], accb = 0.0f;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t p0 = tile * 64;
        const int cnt = (int)(a.n - p0 < 64 ? a.n - p0 : 64);
        const int64_t base = cloud * a.n + p0;
        for (int e = tid; e < 64 * cin; e += kPtThreads) {
            const int p = e / cin, k = e % cin;
            float v = 0.0f;
            if (p < cnt) {
                v = a.in[base * cin + e];
                if (a.in_stat) v = pt_act(v, a.in_stat, k);
            }
            s_in[k * 64 + p] = v;
            if (a.gram) s_dz[k * 65 + p] = v;
        }
        if (!a.gram) {
            for (int e = tid; e < 64 * cout; e += kPtThreads) {
                const int p = e / cout, j = e % cout;
                float v = 0.0f;
                if (p < cnt) {
                    v = a.dy[base * cout + e];
                    if (a.stat) {
                        const float xh = (a.z[base * cout + e] - a.stat[j]) * a.stat[kPnFeat + j];
                        v = a.stat[2 * kPnFeat + j] * ((v - a.coef[j]) - xh * a.coef[kPnFeat + j]);
                    }
                }
                s_dz[j * 65 + p] = v;
            }
        }
        __syncthreads();
        if (a.din) {
            const int p = tid & 63;
            for (int k = tid >> 6; k < cin; k += kPtThreads / 64) {
                float s = 0.0f;
                for (int j = 0; j < cout; ++j) s = fmaf(s_dz[j * 65 + p], W[k * cout + j], s);
                if (p < cnt) {
                    float *o = a.din + (base + p) * cin + k;
                    *o = a.din_accum ? *o + s : s;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = tid + kPtThreads * q;
            if (e < nw) {
                const float *si = s_in + (e / cout) * 64, *sd = s_dz + (e % cout) * 65;
                float s = acc[q];
                for (int p = 0; p < 64; ++p) s = fmaf(si[p], sd[p], s);
                acc[q] = s;
            }
        }
        if (tid < cout)
            for (int p = 0; p < 64; ++p) accb += s_dz[tid * 65 + p];
        __syncthreads();
    }
    const int64_t blk = cloud * gridDim.x + blockIdx.x;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int e = tid + kPtThreads * q;
        if (e < nw) a.partW[blk * nw + e] = acc[q];
    }
    if (tid < cout) a.partb[blk * cout + tid] = accb;
}

// out[grp][e] (+)= the sum over the group's `blocks` partials: thread (element, slice s) adds the partials of blocks s, s + 16, ... in
// ascending order in float64, the 16 slices are added in ascending order; grid (ceil(count / 64), groups)
__global__ __launch_bounds__(64 * kPtSlices) void pt_reduce_kernel(const float *__restrict__ part, int32_t blocks, int32_t count, float *__restrict__ out, int32_t accumulate)
{
    __shared__ double sh[kPtSlices][64];
    const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + lane;
    const int64_t grp = blockIdx.y;
    double s = 0.0;
    if (e < count)
        for (int64_t b = sl; b < blocks; b += kPtSlices) s += (double)part[(grp * blocks + b) * count + e];
    sh[sl][lane] = s;
    __syncthreads();
    if (sl != 0 || e >= count) return;
    s = accumulate ? (double)out[grp * count + e] : 0.0;
    for (int q = 0; q < kPtSlices; ++q) s += sh[q][lane];
    out[grp * count + e] = (float)s;
}

// ---- the 64 -> 512 layer ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t pt_ordered(float v)
{
    const uint32_t u = __float_as_uint(v);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float pt_unordered(uint32_t o) { return __uint_as_float((o >> 31) ? (o & 0x7fffffffu) : ~o); }

struct PtWideArgs {
    const float *zb;           // [B n][64] pre-activations of the 32 -> 64 layer
    const float *in_stat;      // its statistics
    const float *W, *bias;     // [64][512], [512]
    const float *gamma;        // [512]: the sign decides whether the largest or the smallest z is pooled
    double *part;              // [B tiles][2][512] (float64)
    unsigned long long *key;   // [B][512], cleared
    int64_t n;
    int32_t tiles, chunks;     // 32-channel chunks per blockIdx.y
};
// a wave owns 64 points of one cloud, lane = point, D[point][channel] as in the inference trunk
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void pt_wide_kernel(PtWideArgs a)
{
    const int lane = threadIdx.x, half = lane >> 5;
    const int64_t cloud = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
    int64_t p = tile * 64 + lane;
    if (p >= a.n) p = a.n - 1;                                   // a duplicate of the last point: masked out of the sums, never wins a tie
    const float4 *src = reinterpret_cast<const float4 *>(a.zb + (cloud * a.n + p) * 64);
    float h2[64];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const float4 v = src[q];
        h2[4 * q] = v.x; h2[4 * q + 1] = v.y; h2[4 * q + 2] = v.z; h2[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int k = 0; k < 64; ++k) h2[k] = pt_act(h2[k], a.in_stat, k);
    const bool upper = half != 0;
    float a0[32], a1[32];
#pragma unroll
    for (int s = 0; s < 32; ++s) {
        const float lo = h2[2 * s], hi = h2[2 * s + 1];
        const float got = __shfl_xor(upper ? lo : hi, 32, 64);
        a0[s] = upper ? got : lo;
        a1[s] = upper ? hi : got;
    }
    const int c0 = blockIdx.y * a.chunks;
    for (int c = c0; c < c0 + a.chunks; ++c) {
        const int ch = 32 * c + (lane & 31);
        const float *__restrict__ wp = a.W + half * kPnFeat + ch;
        pn_f32x16 acc0 = { 0 }, acc1 = { 0 };
#pragma unroll
        for (int s = 0; s < 32; ++s) {
            const float bv = wp[2 * s * kPnFeat];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], bv, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], bv, acc1, 0, 0, 0);
        }
        const float b = a.bias[ch], sg = a.gamma[ch] < 0.0f ? -1.0f : 1.0f;
        double s1 = 0.0, s2 = 0.0;
        float best = -INFINITY;
        int32_t bi = INT32_MAX;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int32_t pt = (int32_t)tile * 64 + 32 * t + 8 * (r >> 2) + 4 * half + (r & 3);
                const float zv = (t ? acc1[r] : acc0[r]) + b;
                if (pt < a.n) {
                    s1 += (double)zv;
                    s2 += (double)zv * (double)zv;
                    const float v = sg * zv;
                    if (v > best) { best = v; bi = pt; }
                }
            }
        }
        const double o1 = __shfl_xor(s1, 32, 64), o2 = __shfl_xor(s2, 32, 64);
        const float ob = __shfl_xor(best, 32, 64);
        const int32_t oi = __shfl_xor(bi, 32, 64);
        if (!upper) {
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
            const int64_t blk = blockIdx.x;
            a.part[(blk * 2) * kPnFeat + ch] = s1 + o1;
            a.part[(blk * 2 + 1) * kPnFeat + ch] = s2 + o2;
            if (bi != INT32_MAX)
                atomicMax(a.key + cloud * kPnFeat + ch, ((unsigned long long)pt_ordered(best) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)bi));
        }
    }
}

// the winners -> pooled activation g, its point index and its pre-activation; a pooled 0 (no gradient) reports index 0
__global__ __launch_bounds__(kPtThreads) void pt_pool_kernel(const unsigned long long *__restrict__ key, const float *__restrict__ stat, const float *__restrict__ gamma,
                                                             int64_t total, int64_t n, float *__restrict__ g, int32_t *__restrict__ idx, float *__restrict__ zsel)
{
    const int64_t e = (int64_t)blockIdx.x * kPtThreads + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % kPnFeat);
    const unsigned long long k = key[e];
    const float zv = (gamma[c] < 0.0f ? -1.0f : 1.0f) * pt_unordered((uint32_t)(k >> 32));
    int64_t i = (int64_t)(0xFFFFFFFFu - (uint32_t)k);
    const float act = pt_act(zv, stat, c);
    if (!(act > 0.0f) || stat[2 * kPnFeat + c] == 0.0f) i = 0;
    if (i > n - 1) i = n - 1;
    g[e] = act;
    idx[e] = (int32_t)i;
    zsel[e] = zv;
}

// per channel: the sparse gradient S = scale dy at the pooled points, alpha, beta of dz = S - alpha - beta (z - mean), and d gamma, d beta, d bias
__global__ __launch_bounds__(64) void wd_prep_kernel(const float *__restrict__ dg, const float *__restrict__ g, const float *__restrict__ zsel, const float *__restrict__ stat,
                                                     int32_t B, double count, float *__restrict__ sp, float *__restrict__ alpha, float *__restrict__ beta,
                                                     float *__restrict__ g_gamma, float *__restrict__ g_beta, float *__restrict__ g_bias)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    const float mean = stat[c], rstd = stat[kPnFeat + c], scale = stat[2 * kPnFeat + c];
    double s1 = 0.0, s2 = 0.0, ss = 0.0;
    for (int64_t b = 0; b < B; ++b) {
        const float d = g[b * kPnFeat + c] > 0.0f ? dg[b * kPnFeat + c] : 0.0f;
        s1 += (double)d;
        s2 += (double)(d * ((zsel[b * kPnFeat + c] - mean) * rstd));
        const float s = scale * d;
        sp[b * kPnFeat + c] = s;
        ss += (double)s;
    }
    const double be = (double)scale * (double)rstd * (s2 / count), al = (double)scale * (s1 / count);
    alpha[c] = (float)al;
    beta[c] = (float)be;
    g_beta[c] = (float)s1;
    g_gamma[c] = (float)s2;
    g_bias[c] = (float)(ss - count * (double)(float)al);                    // the sum of z - mean over the points is zero
}

// negM[k'][k] = -sum_c W[k'][c] beta_c W[k][c] (e < 4096), negu[k] = -sum_c alpha_c W[k][c] and hbar[k] = s1[k] / count (4096 <= e < 4160)
__global__ __launch_bounds__(kPtThreads) void wd_small_kernel(const float *__restrict__ W, const float *__restrict__ s1, double count, const float *__restrict__ alpha,
                                                              const float *__restrict__ beta, float *__restrict__ negM, float *__restrict__ negu, float *__restrict__ hbar)
{
    const int e = blockIdx.x * kPtThreads + threadIdx.x;
    if (e >= 4160) return;
    double s = 0.0;
    if (e < 4096) {
        const float *w1 = W + (e >> 6) * kPnFeat, *w2 = W + (e & 63) * kPnFeat;
        for (int c = 0; c < kPnFeat; ++c) s += (double)w1[c] * (double)beta[c] * (double)w2[c];
        negM[e] = (float)-s;
    } else {
        const float *w = W + (e - 4096) * kPnFeat;
        for (int c = 0; c < kPnFeat; ++c) s += (double)alpha[c] * (double)w[c];
        negu[e - 4096] = (float)-s;
        hbar[e - 4096] = (float)((double)s1[e - 4096] / count);
    }
}

// dW[k][c] = sum_b S[b][c] h[pooled point of (b, c)][k] - s1[k] alpha_c - beta_c sum_k' (G[k][k'] - s1[k] s1[k'] / count) W[k'][c], in float64
__global__ __launch_bounds__(kPtThreads) void wd_dw_kernel(const float *__restrict__ sp, const int32_t *__restrict__ idx, const float *__restrict__ zb,
                                                           const float *__restrict__ in_stat, const float *__restrict__ G, const float *__restrict__ s1,
                                                           const float *__restrict__ W, double count, const float *__restrict__ alpha,
                                                           const float *__restrict__ beta, int32_t B, int64_t n, float *__restrict__ gW)
{
    const int e = blockIdx.x * kPtThreads + threadIdx.x;         // < 64 x 512
    const int k = e / kPnFeat, c = e % kPnFeat;
    double s = 0.0;
    for (int64_t b = 0; b < B; ++b) {
        const float v = sp[b * kPnFeat + c];
        if (v != 0.0f) s += (double)v * (double)pt_act(zb[(b * n + idx[b * kPnFeat + c]) * 64 + k], in_stat, k);
    }
    const double hk = (double)s1[k] / count;
    double t = 0.0;
    for (int q = 0; q < 64; ++q) t += ((double)G[k * 64 + q] - hk * (double)s1[q]) * (double)W[q * kPnFeat + c];
    gW[e] = (float)(s - (double)s1[k] * (double)alpha[c] - (double)beta[c] * t);
}

// dh[pooled point][k] += S[b][c] W[k][c]: one block per cloud, thread = channel.  The (point, channel) pairs with a non-zero S are ranked
// (512 comparisons each, in parallel), so the channels that pooled one point sit side by side in ascending order; the first of a run owns
// the row and takes the run in that order: distinct points in parallel, one owner per row, a fixed order of the additions.
__global__ __launch_bounds__(kPnFeat) void wd_sparse_kernel(const float *__restrict__ sp, const int32_t *__restrict__ idx, const float *__restrict__ W, int64_t n,
                                                            float *__restrict__ dh)
{
    __shared__ int32_t s_idx[kPnFeat], s_ord[kPnFeat];
    __shared__ float s_sp[kPnFeat];
    const int c = threadIdx.x;
    const int64_t cloud = blockIdx.x;
    const float mine = sp[cloud * kPnFeat + c];
    const int32_t p = mine != 0.0f ? idx[cloud * kPnFeat + c] : INT32_MAX;         // the pairs without a gradient go last
    s_sp[c] = mine;
    s_idx[c] = p;
    __syncthreads();
    int rank = 0;
    for (int q = 0; q < kPnFeat; ++q) {
        const int32_t o = s_idx[q];
        rank += (o < p || (o == p && q < c)) ? 1 : 0;
    }
    s_ord[rank] = c;
    __syncthreads();
    const int first = s_ord[c];                                                   // thread c now speaks for sorted position c
    const int32_t pp = s_idx[first];
    if (pp == INT32_MAX || (c > 0 && s_idx[s_ord[c - 1]] == pp)) return;
    float4 *row = reinterpret_cast<float4 *>(dh + (cloud * n + pp) * 64);
    float acc[64];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const float4 v = row[q];
        acc[4 * q] = v.x; acc[4 * q + 1] = v.y; acc[4 * q + 2] = v.z; acc[4 * q + 3] = v.w;
    }
    for (int i = c; i < kPnFeat && s_idx[s_ord[i]] == pp; ++i) {
        const int ch = s_ord[i];
        const float v = s_sp[ch];
#pragma unroll
        for (int k = 0; k < 64; ++k) acc[k] = fmaf(v, W[k * kPnFeat + ch], acc[k]);
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) row[q] = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
}

// ---- heads: B rows ------------------------------------------------------------------------------------------------------------------------
// z[b][j] = bias[j] + sum_k in[b][k] W[k][j] in float64 (a B-row batch normalisation amplifies every rounding behind it): grid (ceil(cout /
// 64), ceil(B / 4)); thread (output channel, slice s) sums k over the s-th sixteenth of the inputs for four rows, the 16 slices are added in
// ascending order.  cin is a multiple of 16.
__global__ __launch_bounds__(64 * kPtSlices) void hd_dense_kernel(const float *__restrict__ in, const float *__restrict__ W, const float *__restrict__ bias, int32_t B,
                                                                  int32_t cin, int32_t cout, float *__restrict__ z)
{
    __shared__ double sh[kPtSlices][4][64];
    const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    const int64_t r0 = (int64_t)blockIdx.y * 4;
    const int len = cin / kPtSlices, k0 = sl * len;
    double acc[4] = { 0.0, 0.0, 0.0, 0.0 };
    if (j < cout) {
        for (int k = k0; k < k0 + len; ++k) {
            const double w = (double)W[(int64_t)k * cout + j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (r0 + i < B) acc[i] = fma((double)in[(r0 + i) * cin + k], w, acc[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) sh[sl][i][lane] = acc[i];
    __syncthreads();
    if (sl < 4 && r0 + sl < B && j < cout) {
        double v = (double)bias[j];
        for (int q = 0; q < kPtSlices; ++q) v += sh[q][sl][lane];
        z[(r0 + sl) * cout + j] = (float)v;
    }
}

// batch normalisation over the B rows (two passes in float64), ReLU, dropout: thread = channel
__global__ __launch_bounds__(64) void hd_bn_kernel(const float *__restrict__ z, int32_t B, int32_t cout, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                   float *__restrict__ stat, float *__restrict__ mov_mean, float *__restrict__ mov_var, int32_t drop_layer, uint32_t seed,
                                                   uint32_t step, float *__restrict__ act)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= cout) return;
    double s = 0.0;
    for (int64_t b = 0; b < B; ++b) s += (double)z[b * cout + j];
    const double mean = s / B;
    double q = 0.0;
    for (int64_t b = 0; b < B; ++b) {
        const double d = (double)z[b * cout + j] - mean;
        q += d * d;
    }
    pt_bn_finish(mean, q / B, j, gamma, beta, stat, mov_mean, mov_var);
    for (int64_t b = 0; b < B; ++b) {
        float v = pt_act(z[b * cout + j], stat, j);
        if (drop_layer >= 0) v = pt_keep(seed, step, (uint32_t)drop_layer, (uint32_t)b, (uint32_t)j) ? v * kPtInvKeep : 0.0f;
        act[b * cout + j] = v;
    }
}

// d (in place): the gradient of the layer's output rows -> dz; d gamma, d beta, d bias.  stat == null: a plain Dense, dz = d.
__global__ __launch_bounds__(64) void hd_bwd_bn_kernel(const float *__restrict__ z, const float *__restrict__ stat, int32_t B, int32_t cout, int32_t drop_layer, uint32_t seed,
                                                       uint32_t step, float *__restrict__ d, float *__restrict__ g_gamma, float *__restrict__ g_beta,
                                                       float *__restrict__ g_bias)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= cout) return;
    double sb = 0.0;
    if (!stat) {
        for (int64_t b = 0; b < B; ++b) sb += (double)d[b * cout + j];
        g_bias[j] = (float)sb;
        return;
    }
    const float mean = stat[j], rstd = stat[kPnFeat + j], scale = stat[2 * kPnFeat + j];
    double s1 = 0.0, s2 = 0.0;
    for (int64_t b = 0; b < B; ++b) {
        const float zv = z[b * cout + j];
        float v = pt_act(zv, stat, j) > 0.0f ? d[b * cout + j] : 0.0f;
        if (drop_layer >= 0) v = pt_keep(seed, step, (uint32_t)drop_layer, (uint32_t)b, (uint32_t)j) ? v * kPtInvKeep : 0.0f;
        d[b * cout + j] = v;
        s1 += (double)v;
        s2 += (double)(v * ((zv - mean) * rstd));
    }
    const float c1 = (float)(s1 / B), c2 = (float)(s2 / B);
    for (int64_t b = 0; b < B; ++b) {
        const float xh = (z[b * cout + j] - mean) * rstd;
        const float v = scale * ((d[b * cout + j] - c1) - xh * c2);
        d[b * cout + j] = v;
        sb += (double)v;
    }
    g_beta[j] = (float)s1;
    g_gamma[j] = (float)s2;
    g_bias[j] = (float)sb;
}

// block = input channel k: dW[k][:] = sum_b in[b][k] dz[b][:] and din[b][k] = sum_j dz[b][j] W[k][j] (lanes over j, a fixed-order wave sum)
__global__ __launch_bounds__(64) void hd_bwd_w_kernel(const float *__restrict__ in, const float *__restrict__ dz, const float *__restrict__ W, int32_t B, int32_t cin,
                                                      int32_t cout, float *__restrict__ gW, float *__restrict__ din)
{
    const int64_t k = blockIdx.x;
    const int lane = threadIdx.x;
    for (int64_t r0 = 0; r0 < B; r0 += 16) {
        double ds[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) ds[i] = 0.0;
        for (int j = lane; j < cout; j += 64) {
            const double w = (double)W[k * cout + j];
            double gw = r0 ? (double)gW[k * cout + j] : 0.0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (r0 + i < B) {
                    const double v = (double)dz[(r0 + i) * cout + j];
                    gw = fma((double)in[(r0 + i) * cin + k], v, gw);
                    ds[i] = fma(v, w, ds[i]);
                }
            }
            gW[k * cout + j] = (float)gw;
        }
        if (din) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const double t = wave_sum(ds[i]);
                if (lane == 0 && r0 + i < B) din[(r0 + i) * cin + k] = (float)t;
            }
        }
    }
}

// OrthogonalRegularizer as written: X = T reshaped (B f, f), G = X X^T seen as (B, f, B, f) and cut into f x f chunks, the identity taken
// from every chunk.  Block = row i of G: part[i] = 0.001 sum_i' E[i][i']^2, dT[i][:] = 0.002 / B sum_i' (E[i][i'] + E[i'][i]) X[i'][:]
__global__ __launch_bounds__(kPtThreads) void reg_kernel(const float *__restrict__ X, int32_t B, int32_t f, float *__restrict__ dT, float *__restrict__ part)
{
    __shared__ float s_e[kPtThreads], s_x[32];
    __shared__ double s_sum[kPtThreads / 64];
    const int tid = threadIdx.x;
    const int64_t i = blockIdx.x, R = (int64_t)B * f;
    if (tid < f) s_x[tid] = X[i * f + tid];
    __syncthreads();
    double lsum = 0.0, acc = 0.0;
    for (int64_t c0 = 0; c0 < R; c0 += kPtThreads) {
        const int64_t i2 = c0 + tid;
        float e = 0.0f;
        if (i2 < R) {
            float gv = 0.0f;
            for (int k = 0; k < f; ++k) gv = fmaf(s_x[k], X[i2 * f + k], gv);
            const float e1 = gv - ((i * B + i2 / f) % f == i2 % f ? 1.0f : 0.0f);
            const float e2 = gv - ((i2 * B + i / f) % f == i % f ? 1.0f : 0.0f);
            lsum += (double)e1 * (double)e1;
            e = e1 + e2;
        }
        s_e[tid] = e;
        __syncthreads();
        if (tid < f) {
            const int64_t lim = R - c0 < kPtThreads ? R - c0 : kPtThreads;
            for (int64_t t = 0; t < lim; ++t) acc += (double)s_e[t] * (double)X[(c0 + t) * f + tid];
        }
        __syncthreads();
    }
    if (tid < f) dT[i * f + tid] = (float)(0.002 / (double)B * acc);
    lsum = block_sum(lsum, s_sum);
    if (tid == 0) part[i] = (float)(0.001 * lsum);
}

// d out = 2 (out - y) / count, loss[0] = mse + reg, loss[1] = mse, loss[2] = reg = (sum part3 + sum part32) / B: one block
__global__ __launch_bounds__(kPtThreads) void loss_kernel(const float *__restrict__ out, const float *__restrict__ y, int64_t count, const float *__restrict__ part3, int32_t n3,
                                                          const float *__restrict__ part32, int32_t n32, int32_t B, float *__restrict__ dout, float *__restrict__ loss)
{
    __shared__ double sh[kPtThreads / 64];
    double s = 0.0, r = 0.0;
    for (int64_t i = threadIdx.x; i < count; i += kPtThreads) {
        const float d = out[i] - y[i];
        dout[i] = 2.0f * d / (float)count;
        s += (double)d * (double)d;
    }
    for (int i = threadIdx.x; i < n3 + n32; i += kPtThreads) r += (double)(i < n3 ? part3[i] : part32[i - n3]);
    s = block_sum(s, sh);
    r = block_sum(r, sh);
    if (threadIdx.x == 0) {
        const float mse = (float)(s / (double)count), reg = (float)(r / B);
        loss[0] = mse + reg;
        loss[1] = mse;
        loss[2] = reg;
    }
}

__global__ __launch_bounds__(kPtThreads) void adam_kernel(float *__restrict__ w, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v, int64_t count,
                                                          double b1, double b2, double eps, double rate)
{
    const int64_t i = (int64_t)blockIdx.x * kPtThreads + threadIdx.x;
    if (i >= count) return;
    const double gv = (double)g[i];
    const double mm = b1 * (double)m[i] + (1.0 - b1) * gv, vv = b2 * (double)v[i] + (1.0 - b2) * gv * gv;
    m[i] = (float)mm;
    v[i] = (float)vv;
    w[i] = (float)((double)w[i] - rate * mm / (sqrt(vv) + eps));
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------
struct PtHead {
    unsigned long long *key;          // [B][512]
    float *g, *zsel;                  // [B][512]
    int32_t *idx;
    float *z1, *a1, *z2, *a2, *out;   // [B][256] x 2, [B][128] x 2, [B][width]
    float *dout, *d2, *d1, *dg;       // gradients of out, a2, a1, g
    float *sp;                        // [B][512]
};
struct PtScratch {
    float *z[kPnLayers];              // pre-activations of the eight narrow point-wise layers [B n][c_out]
    float *xt, *ft;                   // x T3 [B n][3], f T32 [B n][32]
    float *d64, *d32a, *d32b, *d32c;  // gradients of point-wise activations
    float *stat, *coef;               // [20][4][512], [2][512]
    double *part;                     // forward / backward statistics partials [B tiles][2][512]
    float *partW, *partb;             // [B groups][4096], [B groups][64]
    float *gram, *s1, *negM, *negu, *hbar, *alpha, *beta;
    float *reg3, *reg32;              // [B 3], [B 32]
    PtHead h[3];
    int64_t groups;
};
static const int kPtNarrow[8] = { 0, 1, 6, 7, 8, 9, 14, 15 };
static void pt_carve(Arena &a, int64_t batch, int64_t n, int32_t joints, PtScratch *s)
{
    const size_t B = (size_t)(batch > 0 ? batch : 1), P = B * (size_t)n, tiles = (size_t)cdiv(n, 64);
    for (int l = 0; l < kPnLayers; ++l) s->z[l] = nullptr;
    for (int q = 0; q < 8; ++q) s->z[kPtNarrow[q]] = a.get<float>(P * kPnCout[kPtNarrow[q]]);
    s->xt = a.get<float>(P * 3);
    s->ft = a.get<float>(P * 32);
    s->d64 = a.get<float>(P * 64);
    s->d32a = a.get<float>(P * 32);
    s->d32b = a.get<float>(P * 32);
    s->d32c = a.get<float>(P * 32);
    s->stat = a.get<float>((size_t)kPnLayers * kPtStat);
    s->coef = a.get<float>(2 * kPnFeat);
    s->part = a.get<double>(B * tiles * 2 * kPnFeat);
    size_t groups = 512 / B;
    if (groups < 1) groups = 1;
    if (groups > tiles) groups = tiles;
    s->groups = (int64_t)groups;
    s->partW = a.get<float>(B * groups * 4096);
    s->partb = a.get<float>(B * groups * 64);
    s->gram = a.get<float>(4096);
    s->s1 = a.get<float>(64);
    s->negM = a.get<float>(4096);
    s->negu = a.get<float>(64);
    s->hbar = a.get<float>(64);
    s->alpha = a.get<float>(kPnFeat);
    s->beta = a.get<float>(kPnFeat);
    s->reg3 = a.get<float>(B * 3);
    s->reg32 = a.get<float>(B * 32);
    const size_t width[3] = { 9, 1024, 3 * (size_t)joints };
    for (int t = 0; t < 3; ++t) {
        PtHead &h = s->h[t];
        h.key = a.get<unsigned long long>(B * kPnFeat);
        h.g = a.get<float>(B * kPnFeat);
        h.zsel = a.get<float>(B * kPnFeat);
        h.idx = a.get<int32_t>(B * kPnFeat);
        h.z1 = a.get<float>(B * 256);
        h.a1 = a.get<float>(B * 256);
        h.z2 = a.get<float>(B * 128);
        h.a2 = a.get<float>(B * 128);
        h.out = a.get<float>(B * width[t]);
        h.dout = a.get<float>(B * width[t]);
        h.d2 = a.get<float>(B * 128);
        h.d1 = a.get<float>(B * 256);
        h.dg = a.get<float>(B * kPnFeat);
        h.sp = a.get<float>(B * kPnFeat);
    }
}

static int pt_grad(float *params, int64_t params_floats, const float *x, const float *y, int32_t batch, int64_t n, int32_t joints, uint64_t seed64, uint64_t step64,
                   int32_t training_dropout, float *loss, float *grad, float *T3, float *T32, float *g1, int32_t *i1, float *g2, int32_t *i2, float *g3, int32_t *i3,
                   float *out, void *ws, size_t ws_bytes, hipStream_t st, const char *who)
{
    const int rc = pn_size_check(who, batch, n, joints);
    if (rc) return rc;
    const PtLayout L = pt_layout(joints);
    KPX_REQUIRE(params_floats == L.total, "%s: the parameter buffer of %d joints holds %lld floats, not %lld", who, (int)joints, (long long)L.total, (long long)params_floats);
    if (batch == 0) {                                            // nothing to learn from: loss 0, a zero gradient
        if (loss) KPX_HIP(hipMemsetAsync(loss, 0, 3 * sizeof(float), st));
        if (grad) KPX_HIP(hipMemsetAsync(grad, 0, (size_t)L.trainable * sizeof(float), st));
        return KPX_OK;
    }
    KPX_REQUIRE(params && x && y && loss && grad && ws, "%s: null pointer", who);
    KPX_REQUIRE(((uintptr_t)params % 16) == 0 && ((uintptr_t)ws % 256) == 0, "%s: the parameter buffer must be 16-byte and the workspace 256-byte aligned", who);
    Arena ar(ws, ws_bytes);
    PtScratch s;
    pt_carve(ar, batch, n, joints, &s);
    KPX_ARENA_CHECK(ar);
    KPX_HIP(hipMemsetAsync(grad, 0, (size_t)L.trainable * sizeof(float), st));          // the gaps between the arrays stay zero

    const int32_t B = batch, tiles = (int32_t)cdiv(n, 64);
    const int64_t P = (int64_t)B * n;
    const uint32_t seed = (uint32_t)seed64, step = (uint32_t)step64;
    const int32_t blocks = B * tiles, groups = (int32_t)s.groups;
    const float *W = params;
    auto stat = [&](int l) { return s.stat + (size_t)l * kPtStat; };
    auto width = [&](int l) { return (int32_t)pn_cout(l, joints); };

    // z[l] = src W_l + b_l with its statistics.  src_stat: the producer's statistics (BN + ReLU on load)
    auto conv = [&](int l, const float *src, const float *src_stat) {
        PtFwdArgs a = { src, src_stat, W + L.w[l], 0, W + L.b[l], s.z[l], nullptr, s.part, n, tiles, kPnCin[l], kPnCout[l] };
        hipLaunchKernelGGL(pt_fwd_kernel, dim3(blocks), dim3(kPtThreads), 0, st, a);
        hipLaunchKernelGGL(pt_stat_kernel, dim3((unsigned)cdiv(kPnCout[l], 64)), dim3(64 * kPtSlices), 0, st, (const double *)s.part, blocks, kPnCout[l], (double)P, W + L.gamma[l],
                           W + L.beta[l], stat(l), params + L.mean[l], params + L.var[l]);
    };
    auto transform = [&](const float *src, const float *src_stat, const float *T, int f, float *dst) {
        PtFwdArgs a = { src, src_stat, T, (int64_t)f * f, nullptr, dst, nullptr, nullptr, n, tiles, f, f };
        hipLaunchKernelGGL(pt_fwd_kernel, dim3(blocks), dim3(kPtThreads), 0, st, a);
    };
    // the 64 -> 512 layer l on top of z[l - 1], the pooled values, and the head l + 1 .. l + 3
    auto wide_and_head = [&](int t, int l) -> int {
        PtHead &h = s.h[t];
        KPX_HIP(hipMemsetAsync(h.key, 0, (size_t)B * kPnFeat * sizeof(unsigned long long), st));
        int split = 1;
        while (split < 4 && (int64_t)blocks * split < 1024) split *= 2;
        PtWideArgs a = { s.z[l - 1], stat(l - 1), W + L.w[l], W + L.b[l], W + L.gamma[l], s.part, h.key, n, tiles, kPnChunks / split };
        hipLaunchKernelGGL(pt_wide_kernel, dim3(blocks, split), dim3(64), 0, st, a);
        hipLaunchKernelGGL(pt_stat_kernel, dim3(kPnFeat / 64), dim3(64 * kPtSlices), 0, st, (const double *)s.part, blocks, kPnFeat, (double)P, W + L.gamma[l], W + L.beta[l], stat(l),
                           params + L.mean[l], params + L.var[l]);
        hipLaunchKernelGGL(pt_pool_kernel, dim3((unsigned)cdiv((int64_t)B * kPnFeat, kPtThreads)), dim3(kPtThreads), 0, st, (const unsigned long long *)h.key,
                           (const float *)stat(l), W + L.gamma[l], (int64_t)B * kPnFeat, n, h.g, h.idx, h.zsel);
        const float *in = h.g;
        float *zs[2] = { h.z1, h.z2 }, *as[2] = { h.a1, h.a2 };
        for (int q = 0; q < 2; ++q) {
            const int hl = l + 1 + q;
            hipLaunchKernelGGL(hd_dense_kernel, dim3((unsigned)cdiv(kPnCout[hl], 64), (unsigned)cdiv(B, 4)), dim3(64 * kPtSlices), 0, st, in, W + L.w[hl], W + L.b[hl], B, kPnCin[hl], kPnCout[hl], zs[q]);
            hipLaunchKernelGGL(hd_bn_kernel, dim3((unsigned)cdiv(kPnCout[hl], 64)), dim3(64), 0, st, (const float *)zs[q], B, kPnCout[hl], W + L.gamma[hl], W + L.beta[hl],
                               stat(hl), params + L.mean[hl], params + L.var[hl], (t == 2 && training_dropout) ? q : -1, seed, step, as[q]);
            in = as[q];
        }
        hipLaunchKernelGGL(hd_dense_kernel, dim3((unsigned)cdiv(width(l + 3), 64), (unsigned)cdiv(B, 4)), dim3(64 * kPtSlices), 0, st, in, W + L.w[l + 3], W + L.b[l + 3], B, 128, width(l + 3), h.out);
        return KPX_OK;
    };

    // ---- forward
    conv(0, x, nullptr);
    conv(1, s.z[0], stat(0));
    if (int e = wide_and_head(0, 2)) return e;
    transform(x, nullptr, s.h[0].out, 3, s.xt);
    conv(6, s.xt, nullptr);
    conv(7, s.z[6], stat(6));
    conv(8, s.z[7], stat(7));
    conv(9, s.z[8], stat(8));
    if (int e = wide_and_head(1, 10)) return e;
    transform(s.z[7], stat(7), s.h[1].out, 32, s.ft);
    conv(14, s.ft, nullptr);
    conv(15, s.z[14], stat(14));
    if (int e = wide_and_head(2, 16)) return e;

    // ---- loss, and the regularisers' gradients straight into the T-net heads' output gradients
    hipLaunchKernelGGL(reg_kernel, dim3((unsigned)B * 3), dim3(kPtThreads), 0, st, (const float *)s.h[0].out, B, 3, s.h[0].dout, s.reg3);
    hipLaunchKernelGGL(reg_kernel, dim3((unsigned)B * 32), dim3(kPtThreads), 0, st, (const float *)s.h[1].out, B, 32, s.h[1].dout, s.reg32);
    hipLaunchKernelGGL(loss_kernel, dim3(1), dim3(kPtThreads), 0, st, (const float *)s.h[2].out, y, (int64_t)B * 3 * joints, (const float *)s.reg3, B * 3,
                       (const float *)s.reg32, B * 32, B, s.h[2].dout, loss);

    // ---- backward
    auto reduce = [&](int count, int nblocks, int ngroups, float *dst, int accumulate) {
        hipLaunchKernelGGL(pt_reduce_kernel, dim3((unsigned)cdiv(count, 64), (unsigned)ngroups), dim3(64 * kPtSlices), 0, st, (const float *)s.partW, nblocks, count, dst,
                           accumulate);
    };
    // a narrow layer l: dy (the gradient of its activation, masked in place) -> its parameters' gradients and din
    auto conv_bwd = [&](int l, const float *in, const float *in_stat, float *dy, float *din, int din_accum) {
        const int ci = kPnCin[l], co = kPnCout[l];
        hipLaunchKernelGGL(pt_bwd_stats_kernel, dim3(blocks), dim3(kPtThreads), 0, st, (const float *)s.z[l], (const float *)stat(l), dy, s.part, n, tiles, co);
        hipLaunchKernelGGL(pt_coef_kernel, dim3((unsigned)cdiv(co, 64)), dim3(64 * kPtSlices), 0, st, (const double *)s.part, blocks, co, (double)P, grad + L.gamma[l], grad + L.beta[l],
                           s.coef);
        PtBwdArgs a = { in, in_stat, s.z[l], stat(l), s.coef, dy, W + L.w[l], 0, din, din_accum, s.partW, s.partb, n, tiles, ci, co, 0 };
        hipLaunchKernelGGL(pt_bwd_kernel, dim3(groups, B), dim3(kPtThreads), 0, st, a);
        reduce(ci * co, B * groups, 1, grad + L.w[l], 0);
        hipLaunchKernelGGL(pt_reduce_kernel, dim3(1), dim3(64 * kPtSlices), 0, st, (const float *)s.partb, B * groups, co, grad + L.b[l], 0);
    };
    // xt = in T: dT (added to the regulariser's gradient) and din
    auto transform_bwd = [&](const float *in, const float *in_stat, const float *T, int f, const float *dy, float *dT, float *din) {
        PtBwdArgs a = { in, in_stat, nullptr, nullptr, nullptr, dy, T, (int64_t)f * f, din, 0, s.partW, s.partb, n, tiles, f, f, 0 };
        hipLaunchKernelGGL(pt_bwd_kernel, dim3(groups, B), dim3(kPtThreads), 0, st, a);
        reduce(f * f, groups, B, dT, 1);
    };
    // head t behind the wide layer l, then the wide layer: h.dout -> ... -> the gradient of z[l - 1]'s activation in d64
    auto head_and_wide_bwd = [&](int t, int l) {
        PtHead &h = s.h[t];
        const bool drop = t == 2 && training_dropout;
        hipLaunchKernelGGL(hd_bwd_bn_kernel, dim3((unsigned)cdiv(width(l + 3), 64)), dim3(64), 0, st, (const float *)nullptr, (const float *)nullptr, B, width(l + 3), -1, seed,
                           step, h.dout, (float *)nullptr, (float *)nullptr, grad + L.b[l + 3]);
        hipLaunchKernelGGL(hd_bwd_w_kernel, dim3(128), dim3(64), 0, st, (const float *)h.a2, (const float *)h.dout, W + L.w[l + 3], B, 128, width(l + 3), grad + L.w[l + 3], h.d2);
        hipLaunchKernelGGL(hd_bwd_bn_kernel, dim3(2), dim3(64), 0, st, (const float *)h.z2, (const float *)stat(l + 2), B, 128, drop ? 1 : -1, seed, step, h.d2,
                           grad + L.gamma[l + 2], grad + L.beta[l + 2], grad + L.b[l + 2]);
        hipLaunchKernelGGL(hd_bwd_w_kernel, dim3(256), dim3(64), 0, st, (const float *)h.a1, (const float *)h.d2, W + L.w[l + 2], B, 256, 128, grad + L.w[l + 2], h.d1);
        hipLaunchKernelGGL(hd_bwd_bn_kernel, dim3(4), dim3(64), 0, st, (const float *)h.z1, (const float *)stat(l + 1), B, 256, drop ? 0 : -1, seed, step, h.d1,
                           grad + L.gamma[l + 1], grad + L.beta[l + 1], grad + L.b[l + 1]);
        hipLaunchKernelGGL(hd_bwd_w_kernel, dim3(512), dim3(64), 0, st, (const float *)h.g, (const float *)h.d1, W + L.w[l + 1], B, 512, 256, grad + L.w[l + 1], h.dg);
        hipLaunchKernelGGL(wd_prep_kernel, dim3(kPnFeat / 64), dim3(64), 0, st, (const float *)h.dg, (const float *)h.g, (const float *)h.zsel, (const float *)stat(l), B,
                           (double)P, h.sp, s.alpha, s.beta, grad + L.gamma[l], grad + L.beta[l], grad + L.b[l]);
        PtBwdArgs ga = { s.z[l - 1], stat(l - 1), nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, s.partW, s.partb, n, tiles, 64, 64, 1 };
        hipLaunchKernelGGL(pt_bwd_kernel, dim3(groups, B), dim3(kPtThreads), 0, st, ga);
        reduce(4096, B * groups, 1, s.gram, 0);
        hipLaunchKernelGGL(pt_reduce_kernel, dim3(1), dim3(64 * kPtSlices), 0, st, (const float *)s.partb, B * groups, 64, s.s1, 0);
        hipLaunchKernelGGL(wd_small_kernel, dim3((unsigned)cdiv(4160, kPtThreads)), dim3(kPtThreads), 0, st, W + L.w[l], (const float *)s.s1, (double)P, (const float *)s.alpha,
                           (const float *)s.beta, s.negM, s.negu, s.hbar);
        hipLaunchKernelGGL(wd_dw_kernel, dim3(64 * kPnFeat / kPtThreads), dim3(kPtThreads), 0, st, (const float *)h.sp, (const int32_t *)h.idx, (const float *)s.z[l - 1],
                           (const float *)stat(l - 1), (const float *)s.gram, (const float *)s.s1, W + L.w[l], (double)P, (const float *)s.alpha, (const float *)s.beta, B, n,
                           grad + L.w[l]);
        PtFwdArgs da = { s.z[l - 1], stat(l - 1), s.negM, 0, s.negu, s.d64, s.hbar, nullptr, n, tiles, 64, 64 };
        hipLaunchKernelGGL(pt_fwd_kernel, dim3(blocks), dim3(kPtThreads), 0, st, da);
        hipLaunchKernelGGL(wd_sparse_kernel, dim3(B), dim3(kPnFeat), 0, st, (const float *)h.sp, (const int32_t *)h.idx, W + L.w[l], n, s.d64);
    };

    head_and_wide_bwd(2, 16);
    conv_bwd(15, s.z[14], stat(14), s.d64, s.d32a, 0);
    conv_bwd(14, s.ft, nullptr, s.d32a, s.d32b, 0);                                  // d32b = the gradient of f T32
    transform_bwd(s.z[7], stat(7), s.h[1].out, 32, s.d32b, s.h[1].dout, s.d32c);     // d32c = the gradient of f, first part
    head_and_wide_bwd(1, 10);
    conv_bwd(9, s.z[8], stat(8), s.d64, s.d32a, 0);
    conv_bwd(8, s.z[7], stat(7), s.d32a, s.d32c, 1);                                 // ... second part
    conv_bwd(7, s.z[6], stat(6), s.d32c, s.d32a, 0);
    conv_bwd(6, s.xt, nullptr, s.d32a, s.d32b, 0);                                   // d32b = the gradient of x T3 ([B n][3])
    transform_bwd(x, nullptr, s.h[0].out, 3, s.d32b, s.h[0].dout, nullptr);
    head_and_wide_bwd(0, 2);
    conv_bwd(1, s.z[0], stat(0), s.d64, s.d32a, 0);
    conv_bwd(0, x, nullptr, s.d32a, nullptr, 0);

    // ---- stage outputs
    const size_t fb = (size_t)B * kPnFeat * sizeof(float);
    if (T3) KPX_HIP(hipMemcpyAsync(T3, s.h[0].out, (size_t)B * 9 * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (T32) KPX_HIP(hipMemcpyAsync(T32, s.h[1].out, (size_t)B * 1024 * sizeof(float), hipMemcpyDeviceToDevice, st));
    float *gs[3] = { g1, g2, g3 };
    int32_t *is[3] = { i1, i2, i3 };
    for (int t = 0; t < 3; ++t) {
        if (gs[t]) KPX_HIP(hipMemcpyAsync(gs[t], s.h[t].g, fb, hipMemcpyDeviceToDevice, st));
        if (is[t]) KPX_HIP(hipMemcpyAsync(is[t], s.h[t].idx, fb, hipMemcpyDeviceToDevice, st));
    }
    if (out) KPX_HIP(hipMemcpyAsync(out, s.h[2].out, (size_t)B * 3 * joints * sizeof(float), hipMemcpyDeviceToDevice, st));
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

static int pt_adam(float *w, const float *g, float *m, float *v, int64_t count, double lr, double beta1, double beta2, double eps, int64_t t, hipStream_t st)
{
    KPX_REQUIRE(count >= 0 && t >= 1, "kpx_adam_step: count = %lld, t = %lld: need count >= 0 and t >= 1", (long long)count, (long long)t);
    KPX_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "kpx_adam_step: beta_1 and beta_2 must lie in [0, 1)");
    if (count == 0) return KPX_OK;
    KPX_REQUIRE(w && g && m && v, "kpx_adam_step: null pointer");
    const double rate = lr * sqrt(1.0 - pow(beta2, (double)t)) / (1.0 - pow(beta1, (double)t));
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)cdiv(count, kPtThreads)), dim3(kPtThreads), 0, st, w, g, m, v, count, beta1, beta2, eps, rate);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

}  // namespace kpx

using namespace kpx;

KPX_EXPORT int kpx_pointnet_train_floats(int32_t joints, int64_t *total, int64_t *trainable)
{
    KPX_REQUIRE(joints >= 1 && 3 * (int64_t)joints <= KPX_POINTNET_MAX_OUT, "kpx_pointnet_train_floats: joints = %d: need 1 <= joints and 3 joints <= %d", (int)joints,
                KPX_POINTNET_MAX_OUT);
    const PtLayout L = pt_layout(joints);
    if (total) *total = L.total;
    if (trainable) *trainable = L.trainable;
    return KPX_OK;
}

KPX_EXPORT size_t kpx_pointnet_train_workspace_bytes(int32_t batch, int64_t n, int32_t joints)
{
    if (batch < 0 || n < 1 || joints < 1 || 3 * (int64_t)joints > KPX_POINTNET_MAX_OUT || (int64_t)batch * n >= ((int64_t)1 << 31) || n >= ((int64_t)1 << 31)) return 0;
    Arena a(nullptr, 0);
    PtScratch s;
    pt_carve(a, batch, n, joints, &s);
    return a.off;
}

KPX_EXPORT int kpx_pointnet_grad(float *params, int64_t params_floats, const float *x, const float *y, int32_t batch, int64_t n, int32_t joints, uint64_t seed,
                                 uint64_t step, int32_t training_dropout, float *loss, float *grad, float *T3, float *T32, float *g1, int32_t *i1, float *g2, int32_t *i2,
                                 float *g3, int32_t *i3, float *out, void *ws, size_t ws_bytes, void *stream)
{
    return pt_grad(params, params_floats, x, y, batch, n, joints, seed, step, training_dropout, loss, grad, T3, T32, g1, i1, g2, i2, g3, i3, out, ws, ws_bytes,
                   (hipStream_t)stream, "kpx_pointnet_grad");
}

KPX_EXPORT int kpx_adam_step(float *w, const float *g, float *m, float *v, int64_t count, double lr, double beta1, double beta2, double eps, int64_t t, void *stream)
{
    return pt_adam(w, g, m, v, count, lr, beta1, beta2, eps, t, (hipStream_t)stream);
}

KPX_EXPORT int kpx_pointnet_train_step(float *params, int64_t params_floats, const float *x, const float *y, int32_t batch, int64_t n, int32_t joints, uint64_t seed,
                                       uint64_t step, int32_t training_dropout, float *loss, float *grad, float *m, float *v, double lr, double beta1, double beta2,
                                       double eps, int64_t t, void *ws, size_t ws_bytes, void *stream)
{
    const int rc = pt_grad(params, params_floats, x, y, batch, n, joints, seed, step, training_dropout, loss, grad, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                           nullptr, nullptr, nullptr, ws, ws_bytes, (hipStream_t)stream, "kpx_pointnet_train_step");
    if (rc || batch == 0) return rc;
    return pt_adam(params, grad, m, v, pt_layout(joints).trainable, lr, beta1, beta2, eps, t, (hipStream_t)stream);
}
