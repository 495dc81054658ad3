// kpx_icpsolve.h -- the update step of a registration: the 3x3 (Kabsch) / 6x6 (point-to-plane) solve from the update sums, the
// convergence test, LightSkip's motion bookkeeping (icp_finish, icp_finish_wave), the solve kernels of the dense and the culled
// engine, the explicit-pair Kabsch and the exact fixed-point totals the culled engine solves from.
#pragma once
#include "kpx_icpdefs.h"
#include "kpx_linalg.h"
#include "kpx_fixed.h"

namespace kpx {

// ---- update step ------------------------------------------------------------------------------------------
__device__ void mat4_mul(const double A[16], const double B[16], double C[16])
{
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            double v = 0.0;
            for (int k = 0; k < 4; ++k) v += A[4 * r + k] * B[4 * k + c];
            C[4 * r + c] = v;
        }
}
// Umeyama / Kabsch without scale from the sums (Eigen::umeyama, with_scaling = false)
__device__ void update_p2p(const double *acc, double U[16])
{
    for (int k = 0; k < 16; ++k) U[k] = (k % 5 == 0) ? 1.0 : 0.0;
    double cnt = acc[0];
    if (cnt < 1.0) return;
    double mu_s[3], mu_t[3], S[9], R[9];
    for (int k = 0; k < 3; ++k) { mu_s[k] = acc[2 + k] / cnt; mu_t[k] = acc[5 + k] / cnt; }
    for (int p = 0; p < 3; ++p) for (int q = 0; q < 3; ++q) S[3 * p + q] = acc[8 + 3 * p + q] / cnt - mu_t[p] * mu_s[q];
    kabsch_rotation(S, R);
    for (int p = 0; p < 3; ++p) {
        for (int q = 0; q < 3; ++q) U[4 * p + q] = R[3 * p + q];
        U[4 * p + 3] = mu_t[p] - (R[3 * p] * mu_s[0] + R[3 * p + 1] * mu_s[1] + R[3 * p + 2] * mu_s[2]);
    }
}
// point-to-plane: (J^T J) x = -J^T r ; T = [Rz(x2) Ry(x1) Rx(x0) | x3..5]
__device__ void update_p2plane(const double *acc, double U[16])
{
    for (int k = 0; k < 16; ++k) U[k] = (k % 5 == 0) ? 1.0 : 0.0;
    if (acc[0] < 1.0) return;
    double A[36], b[6], x[6];
    int q = 17;
    for (int p = 0; p < 6; ++p) for (int c = p; c < 6; ++c) { A[6 * p + c] = acc[q]; A[6 * c + p] = acc[q]; ++q; }
    for (int p = 0; p < 6; ++p) b[p] = -acc[38 + p];
    if (!solve6_ldlt(A, b, x)) return;
    double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
    // Rz(g) Ry(b) Rx(a)
    U[0] = cg * cb; U[1] = cg * sb * sa - sg * ca; U[2] = cg * sb * ca + sg * sa; U[3] = x[3];
    U[4] = sg * cb; U[5] = sg * sb * sa + cg * ca; U[6] = sg * sb * ca - cg * sa; U[7] = x[4];
    U[8] = -sb;     U[9] = cb * sa;                U[10] = cb * ca;               U[11] = x[5];
}

// fitness / rmse / convergence test / update of T from the accumulated sums (one thread).  k = index of the
// correspondence search the sums come from.
__device__ void icp_finish(const double *acc, int64_t n, int mode, int k, int max_iter, double rel_fit, double rel_rmse, IcpState *st,
                           double *__restrict__ result)
{
    double cnt = acc[0];
    double fit = (n > 0 && cnt > 0) ? cnt / (double)n : 0.0;
    double rmse = cnt > 0 ? sqrt(acc[1] / cnt) : 0.0;
    bool done = false;
    if (k >= 1 && fabs(st->fitness - fit) < rel_fit && fabs(st->rmse - rmse) < rel_rmse) done = true;
    st->fitness = fit; st->rmse = rmse; st->count = cnt; st->iter = k;
    if (k >= max_iter) done = true;
    if (!done) {
        double U[16], Tn[16];
        if (mode == 1) update_p2plane(acc, U); else update_p2p(acc, U);
        mat4_mul(U, st->T, Tn);
        for (int c = 0; c < 16; ++c) st->T[c] = Tn[c];
    }
    if (done) st->done = 1;
    if (result) {
        for (int c = 0; c < 16; ++c) result[c] = st->T[c];
        result[16] = fit; result[17] = rmse; result[18] = (double)k; result[19] = cnt;
    }
}

// The same step done by ONE WAVE (all 64 lanes call it; acc, st and fs in LDS or global memory visible to the wave).  The
// serial version above keeps its 6x6 factors in scratch memory (dynamically indexed arrays): ~5 us of dependent memory
// round trips in front of every block's sweep when the update runs in the iteration kernel's prologue.  Here the 6x6 system
// is solved by Gauss-Jordan elimination on the augmented matrix [J^T J | -J^T r] held in LDS, lane (i, c) owning entry (i, c):
// six rank-1 steps (no pivoting: the matrix is symmetric positive definite, as for Open3D's ldlt), then the three sine /
// cosine pairs on three lanes and the 4x4 product U T on sixteen.  Point-to-point keeps the serial Jacobi/Kabsch on lane 0.
// Mathematically the same update; rounding differs from the LDL^T order at the 1e-16 level (T is tolerance-checked).
// Blocks that provably cannot find a partner are not swept again (icp_iter_body).  A block whose four waves all found NO target
// group within reach records key = motion + g, g = the smallest distance from a wave's box to any group box (> reach).  Every
// later update moves a source point by at most  |U s - s| <= ||R_u - I||_F |s| + |t_u|,  |s| <= max over the corners c of the source's
// box of |T c|  (|.| is convex: holds for any affine T), which
// the update step adds to `motion`; `reach` bounds the square root of any row's search bound under the current T (the clamp of
// max_correspondence_distance plus the rounding margins of nn_local's metric).  While motion + reach < key no row of the block
// can have a target point within its bound, so the sweep would report "no partner" for all of them -- exactly what the rows
// already hold.  The bounds carry relative margins of 1e-9 .. 1e-6: they only delay skipping, never allow a wrong one.
struct LightSkip {
    const double *sbbox;       // bounding box of the ORIGINAL source points (lo xyz, hi xyz); nullptr: no bookkeeping
    double max_d2, t2max;
};
struct FinishScratch {
    double M[6][8];
    double trig[6];
    double U[16];
    double Tn[16];
    int flag;
};
__device__ __forceinline__ void icp_finish_wave(const double *acc, int64_t n, int mode, int k, int max_iter, double rel_fit, double rel_rmse,
                                                IcpState *st, double *__restrict__ result, FinishScratch &fs, int lane, const LightSkip ls = LightSkip{ nullptr, 0.0, 0.0 },
                                                unsigned long long *dbg = nullptr)
{
    auto tick = [&](int slot) { if (dbg && lane == 0) dbg[slot] = wall_clock64(); };
    tick(0);
    // largest |T p| over the source: |.| is convex, so it is attained at a corner of the source's bounding box (any affine T)
    // (every lane of the wave calls it: lane c & 7 takes corner c, the maximum -- exact, order-free -- is folded over the lanes)
    auto reach_of_source = [&](const double *T) {
        const int c = lane & 7;
        const double x = ls.sbbox[(c & 1) ? 3 : 0], y = ls.sbbox[(c & 2) ? 4 : 1], z = ls.sbbox[(c & 4) ? 5 : 2];
        double n2 = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) { const double v = T[4 * r] * x + T[4 * r + 1] * y + T[4 * r + 2] * z + T[4 * r + 3]; n2 += v * v; }
        double m2 = fmax(0.0, n2);
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) m2 = fmax(m2, __shfl_xor(m2, o, 64));
        return sqrt(m2) * (1.0 + 1e-9);
    };
    if (lane == 0) {
        const double cnt = acc[0];
        const double fit = (n > 0 && cnt > 0) ? cnt / (double)n : 0.0;
        const double rmse = cnt > 0 ? sqrt(acc[1] / cnt) : 0.0;
        bool done = false;
        if (k >= 1 && fabs(st->fitness - fit) < rel_fit && fabs(st->rmse - rmse) < rel_rmse) done = true;
        st->fitness = fit; st->rmse = rmse; st->count = cnt; st->iter = k;
        if (k >= max_iter) done = true;
        if (done) st->done = 1;
        fs.flag = done ? 1 : (cnt < 1.0 ? 2 : 0);              // 2: no correspondence -> identity update
    }
    wave_lds_fence();
    tick(1);
    const int flag = fs.flag;
    if (flag == 0) {
        if (lane < 16) fs.U[lane] = (lane % 5 == 0) ? 1.0 : 0.0;
        if (mode == 1) {
            const int i = lane / 7, c = lane % 7;
            if (lane < 42) {
                double v;
                if (c < 6) {
                    const int a = i < c ? i : c, b = i < c ? c : i;           // upper-triangle slot of (a, b): 17 + a(13 - a)/2 + (b - a)
                    v = acc[17 + (a * (13 - a)) / 2 + (b - a)];
                } else {
                    v = -acc[38 + i];
                }
                fs.M[i][c] = v;
            }
            wave_lds_fence();
            tick(2);
            bool ok = true;
#pragma unroll
            for (int jj = 0; jj < 6; ++jj) {
                const double d = fs.M[jj][jj];
                ok = ok && (fabs(d) > 1e-300);
                double v = 0.0;
                const bool mine = lane < 42 && i != jj;
                if (mine) {
                    const double f = fs.M[i][jj] / d;
                    v = c == jj ? 0.0 : fs.M[i][c] - f * fs.M[jj][c];
                }
                wave_lds_fence();
                if (mine && ok) fs.M[i][c] = v;
                wave_lds_fence();
            }
            tick(3);
            if (ok) {
                if (lane < 3) {
                    const double a = fs.M[lane][6] / fs.M[lane][lane];
                    fs.trig[2 * lane] = cos(a);
                    fs.trig[2 * lane + 1] = sin(a);
                } else if (lane < 6) {
                    fs.U[4 * (lane - 3) + 3] = fs.M[lane][6] / fs.M[lane][lane];
                }
                wave_lds_fence();
                if (lane == 0) {
                    const double ca = fs.trig[0], sa = fs.trig[1], cb = fs.trig[2], sb = fs.trig[3], cg = fs.trig[4], sg = fs.trig[5];
                    // Rz(g) Ry(b) Rx(a)
                    fs.U[0] = cg * cb; fs.U[1] = cg * sb * sa - sg * ca; fs.U[2] = cg * sb * ca + sg * sa;
                    fs.U[4] = sg * cb; fs.U[5] = sg * sb * sa + cg * ca; fs.U[6] = sg * sb * ca - cg * sa;
                    fs.U[8] = -sb;     fs.U[9] = cb * sa;                fs.U[10] = cb * ca;
                }
            }
        } else if (lane == 0) {
            double U[16];
            update_p2p(acc, U);
#pragma unroll
            for (int e = 0; e < 16; ++e) fs.U[e] = U[e];
        }
        wave_lds_fence();
        tick(4);
        // the lever arm of this update = the reach of the source under the transform it is applied to: what the previous update left in
        // `smax` (the same function of the same T, bit for bit); the first update of a registration computes it
        double lever = 0.0;
        if (ls.sbbox) lever = st->smax >= 0.0 ? st->smax : reach_of_source(st->T);      // (wave-uniform branch: smax is one LDS / memory word)
        if (ls.sbbox && lane == 0) {                       // bound on the displacement this update gives any source point
            double rot = 0.0;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) { const double d = fs.U[4 * r + c] - (r == c ? 1.0 : 0.0); rot += d * d; }
            const double tu = sqrt(fs.U[3] * fs.U[3] + fs.U[7] * fs.U[7] + fs.U[11] * fs.U[11]);
            const double moved = (sqrt(rot) * lever + tu) * (1.0 + 1e-9) + 1e-9;
            st->motion += moved;
            st->last_motion = moved;
        }
        tick(5);
        if (lane < 16) {
            const int r = lane >> 2, c = lane & 3;
            double v = 0.0;
#pragma unroll
            for (int e = 0; e < 4; ++e) v += fs.U[4 * r + e] * st->T[4 * e + c];
            fs.Tn[lane] = v;
        }
        wave_lds_fence();
        if (lane < 16) st->T[lane] = fs.Tn[lane];
    }
    wave_lds_fence();
    tick(6);
    double smax = 0.0;
    if (ls.sbbox) smax = reach_of_source(st->T);
    if (ls.sbbox && lane == 0) {                           // reach of a row's search under the transform the next sweep uses
        st->smax = smax;
        // upper bound of nn_local's row bound rb = (clamp - 1)(1 + 2^-30) + eps with clamp, eps as in icp_iter_body / sweep_wave
        const double r2 = ls.max_d2 * (1.0 + 3.7252902984619140625e-9) + 3.7252902984619140625e-9 + 1.4551915228366851806640625e-11 * (smax * smax + ls.t2max + 2.0);
        st->reach = sqrt(r2) * (1.0 + 1e-9);
    }
    tick(7);
    if (result) {
        if (lane < 16) result[lane] = st->T[lane];
        if (lane == 0) { result[16] = st->fitness; result[17] = st->rmse; result[18] = (double)k; result[19] = st->count; }
    }
}

// The same behind a CALL (icp_chain_kernel): inlined into that kernel's loop, the literal constants of cos / sin / sqrt are hoisted
// out of the loop into registers the kernel does not have, and spilled around every sweep
__device__ __attribute__((noinline)) void icp_finish_wave_call(const double *acc, int64_t n, int mode, int k, int max_iter, double rel_fit, double rel_rmse,
                                                               IcpState *st, double *result, FinishScratch *fs, int lane, const double *sbbox, double max_d2,
                                                               double t2max, unsigned long long *dbg)
{
    icp_finish_wave(acc, n, mode, k, max_iter, rel_fit, rel_rmse, st, result, *fs, lane, LightSkip{ sbbox, max_d2, t2max }, dbg);
}

// 1024 threads: thread (slot q = t & 63, slice = t >> 6) sums its slice of the per-block partials with eight
// interleaved accumulators (lanes of a wave read consecutive slots of one partial row: coalesced; a row-per-thread
// variant was 3x slower, the single CU's address path saturates), the sixteen slices are then added in order (a
// fixed summation tree: bitwise reproducible), thread 0 does the algebra.  k = index of the search just finished.
constexpr int kSolveThreads = 1024;
__global__ __launch_bounds__(kSolveThreads) void icp_solve_kernel(const double *__restrict__ part_acc, int nblocks, int64_t n, int mode, int k,
                                                                  int max_iter, double rel_fit, double rel_rmse, IcpState *st,
                                                                  double *__restrict__ result)
{
    if (st->done) return;
    __shared__ double part[kSolveThreads / 64][64];
    __shared__ double acc[kAcc];
    const int nacc = mode == 1 ? kAcc : 17;
    const int q = threadIdx.x & 63, slice = threadIdx.x >> 6;
    {
        double u[8] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
        if (q < nacc) {
            const int per = (nblocks + kSolveThreads / 64 - 1) / (kSolveThreads / 64);
            const int b0 = slice * per, b1 = b0 + per < nblocks ? b0 + per : nblocks;
            int b = b0;
            for (; b + 7 < b1; b += 8) {
#pragma unroll
                for (int e = 0; e < 8; ++e) u[e] += part_acc[(int64_t)(b + e) * kAcc + q];
            }
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (b + e < b1) u[e] += part_acc[(int64_t)(b + e) * kAcc + q];
        }
        part[slice][q] = ((u[0] + u[1]) + (u[2] + u[3])) + ((u[4] + u[5]) + (u[6] + u[7]));
    }
    __syncthreads();
    if (threadIdx.x < kAcc) {
        double v = 0.0;
        if ((int)threadIdx.x < nacc)
            for (int sl = 0; sl < kSolveThreads / 64; ++sl) v += part[sl][threadIdx.x];
        acc[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x) return;
    icp_finish(acc, n, mode, k, max_iter, rel_fit, rel_rmse, st, result);
}

__global__ void icp_init_kernel(IcpState *st, Mat16 T0)
{
    if (threadIdx.x || blockIdx.x) return;
    for (int slot = 0; slot < 2; ++slot) {               // both slots (see IcpFuse)
        for (int q = 0; q < 16; ++q) st[slot].T[q] = T0.m[q];
        state_fresh(&st[slot]);
    }
}

// ---- explicit-pair Kabsch (compute_transformation with a correspondence list) ------------------------------
__global__ __launch_bounds__(256) void pairs_acc_kernel(const float *__restrict__ src, const float *__restrict__ tgt,
                                                        const int32_t *__restrict__ corr, int64_t nc, double *__restrict__ part_acc)
{
    __shared__ double sh[4];
    double acc[17];
#pragma unroll
    for (int q = 0; q < 17; ++q) acc[q] = 0.0;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < nc; c += (int64_t)gridDim.x * blockDim.x) {
        const float *sp = src + 3 * (int64_t)corr[2 * c], *tp = tgt + 3 * (int64_t)corr[2 * c + 1];
        double s[3] = { (double)sp[0], (double)sp[1], (double)sp[2] }, t[3] = { (double)tp[0], (double)tp[1], (double)tp[2] };
        acc[0] += 1.0;
        for (int k = 0; k < 3; ++k) { acc[2 + k] += s[k]; acc[5 + k] += t[k]; }
        for (int p = 0; p < 3; ++p) for (int q = 0; q < 3; ++q) acc[8 + 3 * p + q] += t[p] * s[q];
    }
    for (int q = 0; q < 17; ++q) {
        double v = block_sum(acc[q], sh);
        if (threadIdx.x == 0) part_acc[(int64_t)blockIdx.x * kAcc + q] = v;
    }
}
__global__ __launch_bounds__(64) void pairs_solve_kernel(const double *__restrict__ part_acc, int nblocks, double *__restrict__ T)
{
    __shared__ double acc[17];
    if (threadIdx.x < 17) {
        double s = 0.0;
        for (int b = 0; b < nblocks; ++b) s += part_acc[(int64_t)b * kAcc + threadIdx.x];
        acc[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x) return;
    double U[16];
    update_p2p(acc, U);
    for (int q = 0; q < 16; ++q) T[q] = U[q];
}


// ---- exact accumulation of the update sums (culled engine) --------------------------------------------------------
// Every block adds its fp64 partial sums -- the 17 / 29 of the 44 slots that are live in the mode (acc_live, kpx_icpdefs.h) -- to
// 128-bit fixed-point accumulators (kpx_fixed.h): the totals do not depend on the order of the blocks, so the registration stays
// bitwise reproducible with ONE pair of words per sum instead of one partial row per block -- the solve kernel reads 8 pairs per
// live slot instead of N/64 x 44 doubles.
// kAccCopies copies (block & 7) keep the same-address atomic traffic low.
constexpr int kAccCopies = 8;
__device__ __forceinline__ double fixed_total(const unsigned long long *acc, int slot)
{
    unsigned long long lo = 0ull, hi = 0ull;
#pragma unroll
    for (int c = 0; c < kAccCopies; ++c) {
        const unsigned long long l = acc[((int64_t)c * kAcc + slot) * 2], h = acc[((int64_t)c * kAcc + slot) * 2 + 1];
        lo += l;
        hi += h + (lo < l ? 1ull : 0ull);
    }
    return fixed_value(lo, hi);
}
// the same through device-coherent loads (for a reader inside the launch that did the adds: the XCDs' L2s are not coherent)
__device__ __forceinline__ double fixed_total_coherent(unsigned long long *acc, int slot)
{
    unsigned long long l[kAccCopies], h[kAccCopies];
#pragma unroll
    for (int c = 0; c < kAccCopies; ++c) {
        l[c] = __hip_atomic_load(acc + ((int64_t)c * kAcc + slot) * 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        h[c] = __hip_atomic_load(acc + ((int64_t)c * kAcc + slot) * 2 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    unsigned long long lo = 0ull, hi = 0ull;
#pragma unroll
    for (int c = 0; c < kAccCopies; ++c) {
        lo += l[c];
        hi += h[c] + (lo < l[c] ? 1ull : 0ull);
    }
    return fixed_value(lo, hi);
}
// sums -> update step; clears the accumulators for the next iteration (single block: no race)
// progress: optional word in pinned host memory, tag | done << 32 | iterations finished -- the batch driver reads it to keep
// a window of iterations queued per problem without copies or events (system-scope release store by one thread)
__global__ __launch_bounds__(256) void icp_solve_fixed_kernel(unsigned long long *acc, int64_t n, int mode, int k, int max_iter, double rel_fit,
                                                              double rel_rmse, IcpState *st, double *__restrict__ result,
                                                              unsigned long long *progress, unsigned long long tag)
{
    if (st->done) return;
    __shared__ double sums[kAcc];
    if (threadIdx.x < kAcc) sums[threadIdx.x] = acc_live(mode == 1, (int)threadIdx.x) ? fixed_total(acc, threadIdx.x) : 0.0;     // (only live slots were added to)
    __syncthreads();
    for (int e = threadIdx.x; e < kAccCopies * kAcc * kFixedWords; e += 256) acc[e] = 0ull;
    __shared__ FinishScratch fs;
    if (threadIdx.x >= 64) return;
    icp_finish_wave(sums, n, mode, k, max_iter, rel_fit, rel_rmse, st, result, fs, (int)threadIdx.x);
    if (threadIdx.x) return;
    if (progress)
        __hip_atomic_store(progress, tag | ((unsigned long long)(st->done ? 1 : 0) << 32) | (unsigned long long)(unsigned)(k + 1), __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace kpx
