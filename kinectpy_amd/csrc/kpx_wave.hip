// kpx_wave.hip -- the self-test entry of the wave primitives (kpx_wave.h): one block of four waves, wave w takes rows w, w + 4, ...
// of 64 values and stores what every lane holds afterwards, for tests/test_wave_primitives_gpu.py to compare bit for bit.
#include "kpx_common.h"

namespace kpx {

__global__ __launch_bounds__(256) void wave_selftest_kernel(int kind, const unsigned long long *__restrict__ in, int64_t rows,
                                                            unsigned long long *__restrict__ out)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (kind == KPX_WAVE_SUM_DOWN_F64X9) {                        // groups of nine rows, reduced together; lane 0 alone is defined
        for (int64_t g = wave; 9 * g + 9 <= rows; g += 4) {
            double c[9];
#pragma unroll
            for (int q = 0; q < 9; ++q) c[q] = __longlong_as_double((long long)in[(9 * g + q) * 64 + lane]);
            wave_sum_down_f64x9(c);
#pragma unroll
            for (int q = 0; q < 9; ++q) out[(9 * g + q) * 64 + lane] = lane == 0 ? (unsigned long long)__double_as_longlong(c[q]) : 0ull;
        }
        return;
    }
    for (int64_t r = wave; r < rows; r += 4) {
        const unsigned long long v = in[r * 64 + lane];
        unsigned long long o = 0ull;
        switch (kind) {                                           // block-uniform
        case KPX_WAVE_SUM_I32: o = (unsigned)wave_sum_i32((int)(unsigned)v); break;
        case KPX_WAVE_MIN_U32: o = wave_min_u32((unsigned)v); break;
        case KPX_WAVE_MAX_U32: o = wave_max_u32((unsigned)v); break;
        case KPX_WAVE_MAX_U64: o = wave_max_u64(v); break;
        case KPX_WAVE_MAX_F64: o = (unsigned long long)__double_as_longlong(wave_max_f64(__longlong_as_double((long long)v))); break;
        case KPX_WAVE_INCL_SCAN_I32: o = (unsigned)wave_incl_scan_i32((int)(unsigned)v); break;
        case KPX_WAVE_BCAST: o = wave_bcast((unsigned)v, (int)(r & 63)); break;
        case KPX_WAVE_SUM_DOWN_F64: o = (unsigned long long)__double_as_longlong(wave_sum_down_f64(__longlong_as_double((long long)v))); break;
        case KPX_WAVE_SUM_DOWN_F32: o = __float_as_uint(wave_sum_down_f32(__uint_as_float((unsigned)v))); break;
        default: break;
        }
        out[r * 64 + lane] = o;
    }
}

}  // namespace kpx

using namespace kpx;

KPX_EXPORT int kpx_wave_selftest(int32_t kind, const uint64_t *in, int64_t rows, uint64_t *out, void *stream)
{
    KPX_REQUIRE(kind >= KPX_WAVE_SUM_I32 && kind <= KPX_WAVE_SUM_DOWN_F64X9, "kpx_wave_selftest: unknown kind %d", kind);
    KPX_REQUIRE(rows >= 0 && rows <= 65536, "kpx_wave_selftest: rows must be in [0, 65536]");
    KPX_REQUIRE(kind != KPX_WAVE_SUM_DOWN_F64X9 || rows % 9 == 0, "kpx_wave_selftest: the nine-sum form takes groups of nine rows");
    if (rows == 0) return KPX_OK;
    KPX_REQUIRE(in && out, "kpx_wave_selftest: null pointer");
    hipLaunchKernelGGL(wave_selftest_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (int)kind, (const unsigned long long *)in, rows,
                       (unsigned long long *)out);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}
