// kpx_icpdefs.h -- what the registration's headers share: tile constants, compile-time knobs, the state of a registration, the
// argument blocks of the iteration kernels and a few device helpers (kpx_nndense.h, kpx_icpsolve.h, kpx_nnlocal.h, kpx_icpiter.h,
// kpx_icprows.h; the map is at the top of kpx_icp.hip).
#pragma once
#include <limits.h>

#include "kpx_internal.h"

namespace kpx {

typedef double d4 __attribute__((ext_vector_type(4)));
#ifndef KPX_ICP_WPE
#define KPX_ICP_WPE 3                            // waves per SIMD the iteration kernels are register-budgeted for
#endif

#ifndef KPX_ICP_WAVES
#define KPX_ICP_WAVES 4
#endif
constexpr int kIWaves = KPX_ICP_WAVES;       // waves (16-row tiles) per block: a block lives as long as its slowest wave, but a wave of
                                             // the block form ends with its own rows (icp_iter_body: the last to arrive closes the block)
constexpr int kIThreads = kIWaves * 64;
constexpr int kRT = 2;                       // 16-row tiles per wave (the sweep below is written for 2)
constexpr int kWaves = 4;
constexpr int kRowsPerBlock = kWaves * kRT * 16;   // 128
constexpr int kCT = 32;                      // 16-column tiles per LDS stage (16 KiB)
constexpr int kStageDoubles = kCT * 64;
#ifndef KPX_SEED_STRIDE
#define KPX_SEED_STRIDE 128                 // round 4, operands in curve order, seed = every n-th POINT of the curve: whole bare search 100k x 100k at
                                            // 8 / 16 / 32 / 64 / 128 / 256 -> 0.42 / 0.47 / 0.49 / 0.51 / 0.515 / 0.52 of the fp64 matrix peak (the
                                            // main sweep no longer cares how loose the bound is: a row reaches only the chunks around it).
                                            // Until round 3 (operands in the caller's order, every n-th TILE): 64 -> 2.60 ms, 16 -> 2.48, 8 -> 2.66
#endif
constexpr int kSeedStride = KPX_SEED_STRIDE;  // the seed sweep visits every kSeedStride-th target tile
constexpr double kSentinel = 1e300;
constexpr int kFRT = 4;                      // f32 screening sweep: 16-row tiles per wave
constexpr int kFRowsPerBlock = kWaves * kFRT * 16; // 256
constexpr int kFCT = 64;                     // f32 tiles per LDS stage (16 KiB)
constexpr int kFStageFloats = kFCT * 64;
constexpr int kCand = 64;                    // candidate slots per source row
constexpr int kAcc = 44;                     // accumulator slots: 0 count, 1 sum d2, 2..4 sum s, 5..7 sum t, 8..16 sum t s^T, 17..37 J^T J (21), 38..43 J^T r (6)
// Which slots a mode's update reads -- and the culled engine's iteration kernels therefore produce, stage, sum, add and read back:
// point-to-point (icp_finish / update_p2p) slots 0..16; point-to-plane (update_p2plane) count, sum d2 and the 27 plane slots, 29 of
// the 44: fitness, rmse, the convergence test, the 6x6 system and LightSkip's bookkeeping use none of slots 2..16.  The slot NUMBERS
// and the accumulators' layout are the same in both modes (the merge kernels and icp_solve_kernel share the numbering; GICP, the
// coloured and the robust modes fill slots 0..16 AND 17..43 there); a slot that is not live stays at the zero the accumulators are
// cleared to, and its total is 0.0 without a load.
// In either mode the live slots are 0, 1 and ONE range [acc_lo, acc_hi): loops over them need no test per slot.
__host__ __device__ constexpr int acc_lo(bool plane) { return plane ? 17 : 2; }
__host__ __device__ constexpr int acc_hi(bool plane) { return plane ? kAcc : 17; }
__host__ __device__ constexpr bool acc_live(bool plane, int slot) { return (slot >= 0 && slot < 2) || (slot >= acc_lo(plane) && slot < acc_hi(plane)); }

struct IcpState {
    double T[16];
    double fitness, rmse;
    double count;
    int32_t iter, done;
    double motion, reach;      // see LightSkip: accumulated bound on how far any source point has moved; reach of a row's search
    double last_motion;        // what the latest update added to `motion` (row certificates: how calm the registration is)
    double smax;               // largest |T p| over the source's bounding box under the CURRENT T (the next update's lever arm); < 0: not known yet
};
// a registration that has not iterated yet: everything but T
__device__ __forceinline__ void state_fresh(IcpState *st)
{
    st->fitness = 0.0; st->rmse = 0.0; st->count = 0.0; st->iter = 0; st->done = 0;
    st->motion = 0.0; st->reach = INFINITY; st->last_motion = INFINITY; st->smax = -1.0;
}

__device__ __forceinline__ void xform_row(const double *__restrict__ T, const float *__restrict__ p, double s[3])
{
    const double x = p[0], y = p[1], z = p[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = fma(T[4 * k], x, fma(T[4 * k + 1], y, fma(T[4 * k + 2], z, T[4 * k + 3])));
}
__device__ __forceinline__ double row_seed(const double s[3]) { return fma(s[0], s[0], fma(s[1], s[1], s[2] * s[2])) + 1.0; }
__device__ __forceinline__ int opaque_i(int v) { asm volatile("" : "+v"(v)); return v; }
// What a row (s, seed) is searched with.  Where it has a previous partner: that partner's AC2 value, by the sweep's own fma chain (the
// bound is then a value the sweep would form itself) ...
__device__ __forceinline__ double partner_bound(const double s[3], double seed, const float *tp)
{
    const double tx = tp[0], ty = tp[1], tz = tp[2];
    const double t2 = fma(tx, tx, fma(ty, ty, tz * tz));
    double d = fma(s[0], -2.0 * tx, seed);
    d = fma(s[1], -2.0 * ty, d);
    d = fma(s[2], -2.0 * tz, d);
    return fma(1.0, t2, d);
}
// ... clamped to the correspondence distance: nothing farther than max_d2 can become a partner; the margins cover the expanded
// metric's rounding at the scale of the row and of the target (t2max = target_t2max, kpx_nnlocal.h).  A row without a bound, or whose
// partner lies beyond the clamp, goes in with bj = INT_MAX.
__device__ __forceinline__ void bound_clamp(double seed, double max_d2, double t2max, double &bv, int32_t &bj)
{
    const double clamp = (max_d2 + 1.0) * (1.0 + 9.31322574615478515625e-10) + ldexp(seed + t2max + 1.0, -38);
    if (!(bv <= clamp)) { bv = clamp; bj = INT_MAX; }
}
// AC3: the direct squared distance of a chosen pair
__device__ __forceinline__ double pair_d2(const double s[3], const double t[3])
{
    const double dx = s[0] - t[0], dy = s[1] - t[1], dz = s[2] - t[2];
    return fma(dz, dz, fma(dy, dy, dx * dx));
}
// the point-to-plane row of a pair with the partner's normal at nrm: J = (s x n, n), returns the residual (s - t) . n
__device__ __forceinline__ double plane_row(const double s[3], const double t[3], const float *nrm, double J[6])
{
    const double nx = nrm[0], ny = nrm[1], nz = nrm[2];
    J[0] = s[1] * nz - s[2] * ny; J[1] = s[2] * nx - s[0] * nz; J[2] = s[0] * ny - s[1] * nx;
    J[3] = nx; J[4] = ny; J[5] = nz;
    return (s[0] - t[0]) * nx + (s[1] - t[1]) * ny + (s[2] - t[2]) * nz;
}
// What a pair within the correspondence distance adds to the update sums, handed to put(slot, value): count and d2, with `point`
// the 15 point-to-point terms (s, t, t s^T: slots 2..16), with `plane` the 27 point-to-plane terms (J^T J upper triangle, J^T r:
// slots 17..43).  Every form of the iteration gets its terms here, which is what keeps them equal to the last bit.  The culled
// engine's kernels ask for the slots that are live in their mode (acc_live: point = !plane); the dense engine's merge kernel, whose
// sums are a partial row per block and not atomics, keeps filling all of them (point = true).
template <class Put>
__device__ __forceinline__ void pair_terms(const double s[3], const double t[3], double d2, bool point, bool plane, const float *nrm, Put put)
{
    put(0, 1.0); put(1, d2);
    if (point) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { put(2 + c, s[c]); put(5 + c, t[c]); }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) put(8 + 3 * a + c, t[a] * s[c]);
    }
    if (plane) {
        double J[6];
        const double res = plane_row(s, t, nrm, J);
        int slot = 17;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c = a; c < 6; ++c) put(slot++, J[a] * J[c]);
#pragma unroll
        for (int a = 0; a < 6; ++a) put(38 + a, J[a] * res);
    }
}
// bits 33..39 of a progress word: the share of the registration's rows the iteration searched, in 1/127ths rounded up (0 = none)
__host__ __device__ __forceinline__ unsigned long long progress_searched(unsigned long long searched, int64_t n)
{
    const unsigned long long cls = n > 0 ? (searched * 127ull + (unsigned long long)n - 1ull) / (unsigned long long)n : 0ull;
    return (cls > 127ull ? 127ull : cls) << 33;
}
// the searched-row counts of a registration: eight words behind its ticket, read (device-coherent) and cleared by the block that drew the
// last ticket; every lane < 8 of the calling wave takes one word, the total comes back in every lane of that wave's first 8-lane group
constexpr int kSearchedWord = 8;
__device__ __forceinline__ unsigned long long searched_take(unsigned long long *ticket, int lane_in_block)
{
    unsigned long long v = 0ull;
    if (lane_in_block < 8) {
        v = __hip_atomic_load(ticket + kSearchedWord + lane_in_block, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(ticket + kSearchedWord + lane_in_block, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (lane_in_block < 64) {                              // (wave 0: an 8-lane butterfly; the other waves of a block do not publish)
        unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) {
            const unsigned ol = (unsigned)__shfl_xor((int)lo, o, 64), oh = (unsigned)__shfl_xor((int)hi, o, 64);
            const unsigned long long sum = (((unsigned long long)hi << 32) | lo) + (((unsigned long long)oh << 32) | ol);
            lo = (unsigned)sum; hi = (unsigned)(sum >> 32);
        }
        v = ((unsigned long long)hi << 32) | lo;
    }
    return v;
}
// balanced tree over 16 adjacent values: (((x0+x1)+(x2+x3))+((x4+x5)+(x6+x7))) + (the same over x8..x15) -- the order in which four
// butterfly steps (lane ^ 1, lane ^ 2, half-row mirror, row mirror) add the 16 lanes of a DPP row (row16_tree_sum, kpx_icprows.h)
__device__ __forceinline__ double tile_tree16(const double *x)
{
    double a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = x[2 * i] + x[2 * i + 1];
    return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}
typedef unsigned u2 __attribute__((ext_vector_type(2)));
// high word of the IEEE pattern as a 32-bit register reference (a shift of the 64-bit pattern makes hipcc
// compare zero-extended 64-bit values, i.e. the slow v_cmp_*_u64 this prefilter exists to avoid)
__device__ __forceinline__ unsigned hi32(double v) { return __builtin_bit_cast(u2, v)[1]; }

// [O3D] RobustKernel.cpp: the loss of a robust registration (kpx_icp_robust and its siblings), kind = KPX_LOSS_*.  weight(r) is what
// Open3D's ComputeJTJandJTr multiplies a residual row with (JTJ += J w J^T, JTr += J w r); written with plain fp64 operations, no pow,
// so that tests/robust_ref.py restates it operation by operation.  Open3D does not check k; the entry points require k > 0 where the
// loss has one.
struct RobustLoss {
    int32_t kind;
    double k;
    __device__ __forceinline__ double weight(double r) const
    {
        switch (kind) {
        case KPX_LOSS_L1: return 1.0 / fabs(r);
        case KPX_LOSS_HUBER: return k / fmax(fabs(r), k);
        case KPX_LOSS_CAUCHY: { const double q = r / k; return 1.0 / (1.0 + q * q); }
        case KPX_LOSS_GM: { const double d = k + r * r; return k / (d * d); }
        case KPX_LOSS_TUKEY: { const double q = fmin(1.0, fabs(r) / k); const double u = 1.0 - q * q; return u * u; }
        default: return 1.0;             // KPX_LOSS_L2
        }
    }
};
// One residual row (Jacobian J, residual r) of a robust registration into accumulator slots 17..43: J^T w J (upper triangle) and
// J^T w r with w = loss.weight(r).
// Deviation: Open3D yields NaN from L1Loss at r == 0 (its weight is infinite, times the zero residual); here a row whose weight is
// not finite adds nothing to slots 17..43.
__device__ __forceinline__ void robust_row(const RobustLoss &loss, const double J[6], double r, double *acc)
{
    const double w = loss.weight(r);
    if (!isfinite(w)) return;
    double wJ[6];
#pragma unroll
    for (int p = 0; p < 6; ++p) wJ[p] = w * J[p];
    int q = 17;
#pragma unroll
    for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int c = p; c < 6; ++c) acc[q++] += wJ[p] * J[c];
#pragma unroll
    for (int p = 0; p < 6; ++p) acc[38 + p] += wJ[p] * r;
}

// centre and radius of the target for the float32 screening operands (nn_aux_kernel, kpx_nndense.h)
struct NnAux {
    double c[3];      // centre used for the f32 operands
    double rt2;       // >= max_j |t_j - c|^2
};

struct Mat16 {
    double m[16];
};
static Mat16 mat16_from(const double *h)
{
    Mat16 m;
    for (int q = 0; q < 16; ++q) m.m[q] = h[q];
    return m;
}

// policy and per-registration arguments of the iteration kernels (kpx_icpiter.h, kpx_icprows.h)
struct CertPolicy {
    float calm, factor, smin, smax;      // KPX_CERT_CALM / _FACTOR / _SKIN_MIN / _SKIN_MAX (fractions of the correspondence distance)
};
struct IcpFuse {
    IcpState *pair;
    unsigned long long *ring;
    int max_iter;
    double rel_fit, rel_rmse;
    double *result;
    unsigned long long *progress, tag;
    unsigned long long *ticket;        // non-null (with pair == nullptr): the LAST block of the launch to deliver its sums performs the update
    double *light_key;                 // with ticket: per block, LightSkip key (0 = sweep); nullptr: every block sweeps
    const double *sbbox;               // with light_key: the source's bounding box
    uint32_t *cert;                    // with light_key: per sorted row, the certificate: L as a float rounded down to 17 mantissa bits | the iteration
                                       // of the search in the low 6 bits (0 = none); nullptr: every row is searched
    double *thist;                     // with cert: the transforms of iterations 0 .. 63, 12 doubles each (the winner writes entry k + 1)
    int cert_check;                    // self-check mode: certified rows are searched anyway and compared (g_cert_check)
    CertPolicy pol;
    double *chain_rec;                 // icp_iter_body<true> only: the registration's records (kChainRecords x kChainRec doubles)
    unsigned long long *stamp;         // icp_iter_body<true>, KPX_ICP_CHAIN_STAMPS=1: this iteration's row of g_chain_stamp
};
// one registration of a batch launch (icp_iter_batch_kernel, icp_chain_kernel, icp_rows_kernel's host side)
constexpr int kIcpBatchMax = 8;
struct IcpProblem {
    const float *src;
    const int32_t *row_of;
    float *src_sorted;
    int32_t *idx_sorted;
    float *ptgt_sorted;
    int32_t *idx_cur;
    double *d2_cur;
    IcpState *pair;
    unsigned long long *ring;
    double *result;
    unsigned long long *progress;
    double *light_key;
    const double *sbbox;
    uint32_t *cert;
    double *thist;
    double *chain_rec;
    int64_t n;
    uint32_t block0, blocks;
    // the target operands, the iteration number and the progress tag of the launch: the same for every problem of a launch (one frame's
    // registrations onto one shared target, all at the same iteration; drive_grouped fills them in).  icp_iter_batch_kernel and
    // icp_rows_kernel read them here; icp_chain_kernel, which iterates by itself, takes them as kernel arguments instead
    const float *tgt, *tn;
    const double *Bs;
    const int32_t *orig;
    const float *tile_box, *group_box;
    const double *tbbox;
    int32_t n_groups, k;
    unsigned long long tag;
};
struct IcpBatchArgs {
    IcpProblem p[kIcpBatchMax];
    int32_t count;
};
// the problem whose block range holds this block (block = blockIdx.x - p[..].block0 within it)
__device__ __forceinline__ int batch_problem(const IcpBatchArgs &args)
{
    int pi = 0;
#pragma unroll
    for (int c = 1; c < kIcpBatchMax; ++c) pi += (c < args.count && blockIdx.x >= args.p[c].block0) ? 1 : 0;
    return pi;
}
struct Mat16x8 {
    double m[kIcpBatchMax][16];
};

}  // namespace kpx
