// kpx_compact.hip -- the scans of per-tile and per-block counts: non-template kernels, defined here once and reached through the
// launchers that kpx_compact.h declares.
#include "kpx_compact.h"

namespace kpx {

// A round scans 8 counts per thread (one 3-barrier block scan per 8 x blockDim tiles; a 64M-point selection has 31250 tiles).
static __device__ __forceinline__ void compact_scan_body(int32_t *bc, int32_t nblocks, int32_t *d_count_slot)
{
    __shared__ int sh[1024 / 64 + 1];
    int carry = 0;
    for (int32_t b0 = 0; b0 < nblocks; b0 += 8 * (int32_t)blockDim.x) {
        const int32_t b = b0 + 8 * (int32_t)threadIdx.x;
        int v[8], sum = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) { v[k] = b + k < nblocks ? bc[b + k] : 0; sum += v[k]; }
        int tot;
        int run = carry + block_excl_scan(sum, sh, &tot);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (b + k < nblocks) bc[b + k] = run;
            run += v[k];
        }
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0 && d_count_slot) *d_count_slot = carry;
}
static __global__ __launch_bounds__(1024) void compact_scan_kernel(int32_t *block_counts, int32_t nblocks, int32_t *d_count)
{
    compact_scan_body(block_counts + (int64_t)blockIdx.x * nblocks, nblocks, d_count ? d_count + blockIdx.x : nullptr);
}
static __global__ __launch_bounds__(1024) void compact_scan2_kernel(int32_t *counts_a, int32_t *counts_b, int32_t nblocks, int32_t *d_count_a,
                                                                    int32_t *d_count_b)
{
    compact_scan_body(blockIdx.x ? counts_b : counts_a, nblocks, blockIdx.x ? d_count_b : d_count_a);
}

// a contiguous slice per thread
static __device__ __forceinline__ void scan_i64_body(int64_t *__restrict__ offsets, int64_t m)
{
    __shared__ int64_t sh[1024];
    const int64_t per = (m + 1023) / 1024;
    const int64_t b = (int64_t)threadIdx.x * per < m ? (int64_t)threadIdx.x * per : m;
    const int64_t e = b + per < m ? b + per : m;
    int64_t s = 0;
    for (int64_t i = b; i < e; ++i) s += offsets[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int t = 0; t < 1024; ++t) { const int64_t c = sh[t]; sh[t] = run; run += c; }
        offsets[m] = run;
    }
    __syncthreads();
    int64_t run = sh[threadIdx.x];
    for (int64_t i = b; i < e; ++i) { const int64_t c = offsets[i]; offsets[i] = run; run += c; }
}
static __global__ __launch_bounds__(1024) void scan_i64_kernel(int64_t *__restrict__ offsets, int64_t m) { scan_i64_body(offsets, m); }
static __global__ __launch_bounds__(1024) void scan2_i64_kernel(int64_t *__restrict__ a, int64_t *__restrict__ b, int64_t m)
{
    scan_i64_body(blockIdx.x ? b : a, m);
}

void compact_scan(int32_t *counts, int32_t tiles, int32_t frames, int32_t *d_count, hipStream_t st)
{
    hipLaunchKernelGGL(compact_scan_kernel, dim3(frames), dim3(compact_scan_threads(tiles)), 0, st, counts, tiles, d_count);
}
void compact_scan2(int32_t *counts_a, int32_t *counts_b, int32_t tiles, int32_t *d_count_a, int32_t *d_count_b, hipStream_t st)
{
    hipLaunchKernelGGL(compact_scan2_kernel, dim3(2), dim3(compact_scan_threads(tiles)), 0, st, counts_a, counts_b, tiles, d_count_a, d_count_b);
}
void scan_i64(int64_t *offsets, int64_t m, hipStream_t st) { hipLaunchKernelGGL(scan_i64_kernel, dim3(1), dim3(1024), 0, st, offsets, m); }
void scan2_i64(int64_t *a, int64_t *b, int64_t m, hipStream_t st) { hipLaunchKernelGGL(scan2_i64_kernel, dim3(2), dim3(1024), 0, st, a, b, m); }

}  // namespace kpx
