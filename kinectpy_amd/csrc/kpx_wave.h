// kpx_wave.h -- whole-wave (64 lanes) reductions, scans and broadcasts that stay on the vector ALU: DPP row moves inside a row of 16
// lanes, v_permlane16_swap / v_permlane32_swap across the rows and halves, v_readlane / v_readfirstlane for a wave-uniform result.
// __shfl / __shfl_xor / __shfl_up / __shfl_down compile to ds_bpermute_b32 -- an LDS-crossbar instruction and a wait -- per 32-bit
// word and step; none of the primitives below issues one on gfx950.  Other targets (and the host pass) take the shuffles.
//
// PRECONDITION of every primitive: all 64 lanes of the wave are active (full EXEC mask) -- DPP and the swaps read the registers of
// inactive lanes as they are.  Call them from wave-uniform control flow only.
//
// Exactness: the integer primitives and the maxima are exact in any order.  The floating-point sums fix their association:
// wave_sum_down_* leaves in lane 0 bit for bit what `for (o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64)` leaves there (at
// step o lane i < o adds the value of lane i + o).  Lane 0 of the xor butterfly `v += __shfl_xor(v, o, 64)` holds the same bits:
// the pairs are the same and IEEE addition is commutative.  The other lanes hold no defined value.
//
// NaN: wave_max_f64 is a tree of fmax -- a NaN operand is dropped in favour of the other one, the result is NaN only if all 64
// inputs are; with zeros of both signs as the maximum the sign of the result is unspecified.  No caller feeds either (squared
// distances: >= +0, never NaN).  A NaN in wave_sum_down_* propagates as in the shuffle tree (payloads aside).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#if defined(__HIP_DEVICE_COMPILE__) && defined(__gfx950__)
#if __has_builtin(__builtin_amdgcn_permlane16_swap) && __has_builtin(__builtin_amdgcn_permlane32_swap) && __has_builtin(__builtin_amdgcn_update_dpp)
#define KPX_WAVE_VALU 1
#endif
#endif
#ifndef KPX_WAVE_VALU
#define KPX_WAVE_VALU 0
#endif

namespace kpx {

// DPP controls (row = 16 lanes): row_shl:n lane i reads lane i + n, row_shr:n lane i - n, row_ror:n lane (i - n) mod 16 of its row;
// row_bcast15 / row_bcast31: lane 15 of every row / lane 31 to the lanes of the following row / half.  A lane whose source lies
// outside its row, or that the row / bank mask leaves out, keeps `old`.
constexpr int kDppRowShl = 0x100, kDppRowShr = 0x110, kDppRowRor = 0x120, kDppRowBcast15 = 0x142, kDppRowBcast31 = 0x143;

#if KPX_WAVE_VALU
template <int CTRL, int ROW_MASK = 0xF, int BANK_MASK = 0xF> __device__ __forceinline__ unsigned wave_dpp_u32(unsigned old, unsigned v)
{
    return (unsigned)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, ROW_MASK, BANK_MASK, false);
}
template <int CTRL> __device__ __forceinline__ double wave_dpp_f64(double v)
{
    const unsigned long long p = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = wave_dpp_u32<CTRL>((unsigned)p, (unsigned)p), hi = wave_dpp_u32<CTRL>((unsigned)(p >> 32), (unsigned)(p >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// own: this lane's value; other: the value of lane i ^ 16 (swap16) / i ^ 32 (swap32).  With both operands the same register, the
// swap leaves [rows 0 0 2 2 | rows 1 1 3 3] (16) or [halves 0 0 | halves 1 1] (32): one of the two results is the lane's own value.
__device__ __forceinline__ void wave_swap16_u32(unsigned v, unsigned &r0, unsigned &r1)
{
    const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    r0 = r[0]; r1 = r[1];
}
__device__ __forceinline__ void wave_swap32_u32(unsigned v, unsigned &r0, unsigned &r1)
{
    const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    r0 = r[0]; r1 = r[1];
}
// (a, b) = (value of the lower partner, value of the upper partner) of the pair (i, i ^ 16) / (i, i ^ 32), the same in both lanes
__device__ __forceinline__ void wave_swap16_f64(double v, double &a, double &b)
{
    const unsigned long long p = (unsigned long long)__double_as_longlong(v);
    unsigned l0, l1, h0, h1;
    wave_swap16_u32((unsigned)p, l0, l1); wave_swap16_u32((unsigned)(p >> 32), h0, h1);
    a = __longlong_as_double((long long)(((unsigned long long)h0 << 32) | l0));
    b = __longlong_as_double((long long)(((unsigned long long)h1 << 32) | l1));
}
__device__ __forceinline__ void wave_swap32_f64(double v, double &a, double &b)
{
    const unsigned long long p = (unsigned long long)__double_as_longlong(v);
    unsigned l0, l1, h0, h1;
    wave_swap32_u32((unsigned)p, l0, l1); wave_swap32_u32((unsigned)(p >> 32), h0, h1);
    a = __longlong_as_double((long long)(((unsigned long long)h0 << 32) | l0));
    b = __longlong_as_double((long long)(((unsigned long long)h1 << 32) | l1));
}
#endif

// ---- exact reductions, the result in every lane (gfx950: in a scalar register, so a branch on it is a scalar branch) --------------
template <class Op> __device__ __forceinline__ unsigned wave_reduce_u32(unsigned v, Op op)
{
#if KPX_WAVE_VALU
    v = op(v, wave_dpp_u32<kDppRowRor + 1>(v, v)); v = op(v, wave_dpp_u32<kDppRowRor + 2>(v, v));
    v = op(v, wave_dpp_u32<kDppRowRor + 4>(v, v)); v = op(v, wave_dpp_u32<kDppRowRor + 8>(v, v));      // every lane: its row
    unsigned a, b;
    wave_swap16_u32(v, a, b); v = op(a, b);
    wave_swap32_u32(v, a, b); v = op(a, b);
    return (unsigned)__builtin_amdgcn_readfirstlane((int)v);
#else
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
#endif
}
__device__ __forceinline__ int wave_sum_i32(int v)
{
    return (int)wave_reduce_u32((unsigned)v, [](unsigned a, unsigned b) { return a + b; });      // two's complement: wraps like int
}
__device__ __forceinline__ unsigned wave_min_u32(unsigned v)
{
    return wave_reduce_u32(v, [](unsigned a, unsigned b) { return a < b ? a : b; });
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v)
{
    return wave_reduce_u32(v, [](unsigned a, unsigned b) { return a > b ? a : b; });
}
// the largest high word, then the largest low word among the lanes that hold it
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v)
{
    const unsigned hi = wave_max_u32((unsigned)(v >> 32));
    const unsigned lo = wave_max_u32((unsigned)(v >> 32) == hi ? (unsigned)v : 0u);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ double wave_max_f64(double v)
{
#if KPX_WAVE_VALU
    v = fmax(v, wave_dpp_f64<kDppRowRor + 1>(v)); v = fmax(v, wave_dpp_f64<kDppRowRor + 2>(v));
    v = fmax(v, wave_dpp_f64<kDppRowRor + 4>(v)); v = fmax(v, wave_dpp_f64<kDppRowRor + 8>(v));
    double a, b;
    wave_swap16_f64(v, a, b); v = fmax(a, b);
    wave_swap32_f64(v, a, b); v = fmax(a, b);
    const unsigned long long p = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)p), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(p >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
#else
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
#endif
}

// ---- inclusive scan (the GFX9 DPP scan: inside the rows, then lane 15 of a row into the next row, lane 31 into the upper half) ----
__device__ __forceinline__ int wave_incl_scan_i32(int v)
{
#if KPX_WAVE_VALU
    unsigned t = (unsigned)v;
    t += wave_dpp_u32<kDppRowShr + 1>(0u, (unsigned)v) + wave_dpp_u32<kDppRowShr + 2>(0u, (unsigned)v) + wave_dpp_u32<kDppRowShr + 3>(0u, (unsigned)v);
    t += wave_dpp_u32<kDppRowShr + 4, 0xF, 0xE>(0u, t);
    t += wave_dpp_u32<kDppRowShr + 8, 0xF, 0xC>(0u, t);
    t += wave_dpp_u32<kDppRowBcast15, 0xA>(0u, t);
    t += wave_dpp_u32<kDppRowBcast31, 0xC>(0u, t);
    return (int)t;
#else
    const int l = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(v, o, 64); if (l >= o) v += t; }
    return v;
#endif
}

// ---- broadcast from a wave-uniform lane (an owner found by a ballot, a constant) ---------------------------------------------------
__device__ __forceinline__ int wave_bcast(int v, int uniform_lane)
{
#if KPX_WAVE_VALU
    return __builtin_amdgcn_readlane(v, uniform_lane);
#else
    return __shfl(v, uniform_lane, 64);
#endif
}
__device__ __forceinline__ unsigned wave_bcast(unsigned v, int uniform_lane) { return (unsigned)wave_bcast((int)v, uniform_lane); }

// ---- floating-point sums in the __shfl_down tree, valid in lane 0 only --------------------------------------------------------------
__device__ __forceinline__ double wave_sum_down_f64(double v)
{
#if KPX_WAVE_VALU
    double a, b;
    wave_swap32_f64(v, a, b); v = a + b;                          // lane i < 32: v[i] + v[i + 32]
    wave_swap16_f64(v, a, b); v = a + b;                          // lane i < 16: v[i] + v[i + 16]
    v += wave_dpp_f64<kDppRowShl + 8>(v); v += wave_dpp_f64<kDppRowShl + 4>(v);
    v += wave_dpp_f64<kDppRowShl + 2>(v); v += wave_dpp_f64<kDppRowShl + 1>(v);
    return v;
#else
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
#endif
}
__device__ __forceinline__ float wave_sum_down_f32(float v)
{
#if KPX_WAVE_VALU
    unsigned a, b;
    wave_swap32_u32(__float_as_uint(v), a, b); v = __uint_as_float(a) + __uint_as_float(b);
    wave_swap16_u32(__float_as_uint(v), a, b); v = __uint_as_float(a) + __uint_as_float(b);
    v += __uint_as_float(wave_dpp_u32<kDppRowShl + 8>(__float_as_uint(v), __float_as_uint(v)));
    v += __uint_as_float(wave_dpp_u32<kDppRowShl + 4>(__float_as_uint(v), __float_as_uint(v)));
    v += __uint_as_float(wave_dpp_u32<kDppRowShl + 2>(__float_as_uint(v), __float_as_uint(v)));
    v += __uint_as_float(wave_dpp_u32<kDppRowShl + 1>(__float_as_uint(v), __float_as_uint(v)));
    return v;
#else
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
#endif
}

// Nine sums at once (the raw moments of a neighbourhood), each in the tree of wave_sum_down_f64, valid in lane 0.  Step 32 exchanges
// halves BETWEEN two sums -- afterwards one register carries sum j in lanes < 32 and sum j + 5 in lanes >= 32, each lane i' of a half
// holding v[i'] + v[i' + 32] of its sum -- and step 16 does the same with the rows: 9 -> 5 -> 3 registers, every sum's additions and
// their nesting those of the single tree.  The row steps then run on three registers and six moves bring the sums back to lane 0.
__device__ __forceinline__ void wave_sum_down_f64x9(double c[9])
{
#if KPX_WAVE_VALU
    auto pair32 = [](double p, double q) {                          // lanes < 32: tree step of p; lanes >= 32: of q
        const unsigned long long pp = (unsigned long long)__double_as_longlong(p), qq = (unsigned long long)__double_as_longlong(q);
        const auto l = __builtin_amdgcn_permlane32_swap((unsigned)pp, (unsigned)qq, false, false);
        const auto h = __builtin_amdgcn_permlane32_swap((unsigned)(pp >> 32), (unsigned)(qq >> 32), false, false);
        return __longlong_as_double((long long)(((unsigned long long)h[0] << 32) | l[0])) + __longlong_as_double((long long)(((unsigned long long)h[1] << 32) | l[1]));
    };
    auto pair16 = [](double p, double q) {                          // rows 0, 2: tree step of p's row pair; rows 1, 3: of q's
        const unsigned long long pp = (unsigned long long)__double_as_longlong(p), qq = (unsigned long long)__double_as_longlong(q);
        const auto l = __builtin_amdgcn_permlane16_swap((unsigned)pp, (unsigned)qq, false, false);
        const auto h = __builtin_amdgcn_permlane16_swap((unsigned)(pp >> 32), (unsigned)(qq >> 32), false, false);
        return __longlong_as_double((long long)(((unsigned long long)h[0] << 32) | l[0])) + __longlong_as_double((long long)(((unsigned long long)h[1] << 32) | l[1]));
    };
    // halves: r0 = (c0 | c5), r1 = (c1 | c6), r2 = (c2 | c7), r3 = (c3 | c8), r4 = (c4 | c4)
    const double r0 = pair32(c[0], c[5]), r1 = pair32(c[1], c[6]), r2 = pair32(c[2], c[7]), r3 = pair32(c[3], c[8]), r4 = pair32(c[4], c[4]);
    // rows: t0 = (c0, c1, c5, c6), t1 = (c2, c3, c7, c8), t2 = (c4, c4, c4, c4)
    double t0 = pair16(r0, r1), t1 = pair16(r2, r3), t2 = pair16(r4, r4);
    t0 += wave_dpp_f64<kDppRowShl + 8>(t0); t1 += wave_dpp_f64<kDppRowShl + 8>(t1); t2 += wave_dpp_f64<kDppRowShl + 8>(t2);
    t0 += wave_dpp_f64<kDppRowShl + 4>(t0); t1 += wave_dpp_f64<kDppRowShl + 4>(t1); t2 += wave_dpp_f64<kDppRowShl + 4>(t2);
    t0 += wave_dpp_f64<kDppRowShl + 2>(t0); t1 += wave_dpp_f64<kDppRowShl + 2>(t1); t2 += wave_dpp_f64<kDppRowShl + 2>(t2);
    t0 += wave_dpp_f64<kDppRowShl + 1>(t0); t1 += wave_dpp_f64<kDppRowShl + 1>(t1); t2 += wave_dpp_f64<kDppRowShl + 1>(t2);
    // the sums stand in lanes 0, 16, 32, 48 of t0 / t1 and lane 0 of t2
    auto from = [](double v, int lane) {
        const unsigned long long p = (unsigned long long)__double_as_longlong(v);
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)p, lane), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(p >> 32), lane);
        return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    };
    c[0] = t0; c[1] = from(t0, 16); c[5] = from(t0, 32); c[6] = from(t0, 48);
    c[2] = t1; c[3] = from(t1, 16); c[7] = from(t1, 32); c[8] = from(t1, 48);
    c[4] = t2;
#else
#pragma unroll
    for (int q = 0; q < 9; ++q) c[q] = wave_sum_down_f64(c[q]);
#endif
}

// ---- the same per ROW of 16 lanes: four independent results per wave ------------------------------------------------------------------
// Row r = lanes 16 r .. 16 r + 15.  DPP row controls only: a reduction or a scan ends after the four row steps, no swap16 / swap32 and
// no ds_bpermute.  Same precondition (all 64 lanes active, wave-uniform control flow); other targets take __shfl* of width 16.
template <class Op> __device__ __forceinline__ unsigned row_reduce_u32(unsigned v, Op op)      // the row's result in every lane of the row
{
#if KPX_WAVE_VALU
    v = op(v, wave_dpp_u32<kDppRowRor + 1>(v, v)); v = op(v, wave_dpp_u32<kDppRowRor + 2>(v, v));
    v = op(v, wave_dpp_u32<kDppRowRor + 4>(v, v)); v = op(v, wave_dpp_u32<kDppRowRor + 8>(v, v));
    return v;
#else
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = op(v, (unsigned)__shfl_xor((int)v, o, 16));
    return v;
#endif
}
__device__ __forceinline__ int row_sum_i32(int v)
{
    return (int)row_reduce_u32((unsigned)v, [](unsigned a, unsigned b) { return a + b; });
}
__device__ __forceinline__ unsigned row_min_u32(unsigned v)
{
    return row_reduce_u32(v, [](unsigned a, unsigned b) { return a < b ? a : b; });
}
__device__ __forceinline__ unsigned row_max_u32(unsigned v)
{
    return row_reduce_u32(v, [](unsigned a, unsigned b) { return a > b ? a : b; });
}
__device__ __forceinline__ double row_max_f64(double v)                                     // NaN and signed zeros: as wave_max_f64
{
#if KPX_WAVE_VALU
    v = fmax(v, wave_dpp_f64<kDppRowRor + 1>(v)); v = fmax(v, wave_dpp_f64<kDppRowRor + 2>(v));
    v = fmax(v, wave_dpp_f64<kDppRowRor + 4>(v)); v = fmax(v, wave_dpp_f64<kDppRowRor + 8>(v));
    return v;
#else
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 16));
    return v;
#endif
}
__device__ __forceinline__ int row_incl_scan_i32(int v)
{
#if KPX_WAVE_VALU
    unsigned t = (unsigned)v;
    t += wave_dpp_u32<kDppRowShr + 1>(0u, (unsigned)v) + wave_dpp_u32<kDppRowShr + 2>(0u, (unsigned)v) + wave_dpp_u32<kDppRowShr + 3>(0u, (unsigned)v);
    t += wave_dpp_u32<kDppRowShr + 4, 0xF, 0xE>(0u, t);
    t += wave_dpp_u32<kDppRowShr + 8, 0xF, 0xC>(0u, t);
    return (int)t;
#else
    const int l = threadIdx.x & 15;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) { const int t = __shfl_up(v, o, 16); if (l >= o) v += t; }
    return v;
#endif
}
// the value of lane `lane_in_row` (0 .. 15, the same in all lanes of a row; the rows may name different lanes) in every lane of the row
__device__ __forceinline__ unsigned row_bcast(unsigned v, int lane_in_row)
{
#if KPX_WAVE_VALU
    return row_reduce_u32(((int)(threadIdx.x & 15) == lane_in_row) ? v : 0u, [](unsigned a, unsigned b) { return a | b; });
#else
    return (unsigned)__shfl((int)v, lane_in_row, 16);
#endif
}
__device__ __forceinline__ int row_bcast(int v, int lane_in_row) { return (int)row_bcast((unsigned)v, lane_in_row); }
// The last four steps of wave_sum_down_f64, valid in lane 0 of every row: at step o lane i < o of the row adds the value of lane i + o.
__device__ __forceinline__ double row_sum_down_f64(double v)
{
#if KPX_WAVE_VALU
    v += wave_dpp_f64<kDppRowShl + 8>(v); v += wave_dpp_f64<kDppRowShl + 4>(v);
    v += wave_dpp_f64<kDppRowShl + 2>(v); v += wave_dpp_f64<kDppRowShl + 1>(v);
    return v;
#else
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_down(v, o, 16);
    return v;
#endif
}
__device__ __forceinline__ void row_sum_down_f64x9(double c[9])
{
#pragma unroll
    for (int q = 0; q < 9; ++q) c[q] = row_sum_down_f64(c[q]);
}

}  // namespace kpx
