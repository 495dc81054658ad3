// kpx_common.h -- shared host/device helpers of libkinectpx.so (gfx950 only).
#pragma once
#include <stdlib.h>
#include <functional>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/kinectpx.h"
#include "kpx_wave.h"

#define KPX_EXPORT extern "C" __attribute__((visibility("default")))

namespace kpx {

// ---- errors -----------------------------------------------------------------------------------
extern thread_local char g_err[512];
int fail(int code, const char *fmt, ...);

#define KPX_HIP(call)                                                                              \
    do {                                                                                           \
        hipError_t e__ = (call);                                                                   \
        if (e__ != hipSuccess)                                                                     \
            return kpx::fail(KPX_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__),  \
                             __FILE__, __LINE__);                                                  \
    } while (0)
#define KPX_LAUNCH_CHECK() KPX_HIP(hipGetLastError())
#define KPX_REQUIRE(cond, ...)                                                                     \
    do {                                                                                           \
        if (!(cond)) return kpx::fail(KPX_ERR_INVALID, __VA_ARGS__);                               \
    } while (0)

// ---- workspace bump allocator (same carve sequence for the size query and the real call) -------
struct Arena {
    char *base;
    size_t off, cap;
    bool dry;
    explicit Arena(void *p, size_t bytes) : base((char *)p), off(0), cap(bytes), dry(p == nullptr) {}
    template <class T> T *get(size_t count)
    {
        size_t bytes = (count * sizeof(T) + 255) & ~(size_t)255;
        T *r = dry ? nullptr : (T *)(base + off);
        off += bytes;
        return r;
    }
    bool ok() const { return dry || off <= cap; }
};
#define KPX_ARENA_CHECK(a)                                                                         \
    do {                                                                                           \
        if (!(a).ok())                                                                             \
            return kpx::fail(KPX_ERR_WORKSPACE, "workspace too small: need %zu bytes, have %zu",   \
                             (a).off, (a).cap);                                                    \
    } while (0)

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// The vendor primitives' temporary-storage queries (hipcub / rocPRIM called with a null buffer) cost tens of microseconds each when
// several frame threads are inside the runtime, and every operator asked them again on every call while carving its workspace -- a
// 4-sensor frame asked ~20 of them, and its stream sat idle meanwhile (profiles/r05/overlap_timeline_*.txt).  Their answers depend
// only on (what is asked, element count): asked once per process and remembered.  `what` (16 bits) names the primitive as it was
// instantiated, never a call site: kpx_sort.h builds it for the sorts, the grid build's scan is the one other user.
constexpr unsigned kMemoSort = 0x4000u, kMemoGridScan = 0x8000u;
size_t memo_bytes(unsigned what, int64_t n, const std::function<size_t()> &query);

// 16-byte loads / stores of data that is touched once (streaming operators): non-temporal, so that a pass over a cloud does not
// evict what other kernels of the frame keep in L2 / Infinity Cache.  -DKPX_STREAM_PLAIN: ordinary accesses (A/B switch).
typedef unsigned int kpx_u4 __attribute__((ext_vector_type(4)));
template <class V> __device__ __forceinline__ V stream_load16(const V *p)
{
    static_assert(sizeof(V) == 16, "16-byte vectors only");
#ifdef KPX_STREAM_PLAIN
    return *p;
#else
    const kpx_u4 r = __builtin_nontemporal_load(reinterpret_cast<const kpx_u4 *>(p));
    V v;
    __builtin_memcpy(&v, &r, 16);
    return v;
#endif
}
template <class V> __device__ __forceinline__ void stream_store16(const V &v, V *p)
{
    static_assert(sizeof(V) == 16, "16-byte vectors only");
#ifdef KPX_STREAM_PLAIN
    *p = v;
#else
    kpx_u4 r;
    __builtin_memcpy(&r, &v, 16);
    __builtin_nontemporal_store(r, reinterpret_cast<kpx_u4 *>(p));
#endif
}
#define KPX_STREAM_LOAD(p) stream_load16(p)
#define KPX_STREAM_STORE(v, p) stream_store16((v), (p))

// ---- HIP-event profiler (armed by kpx_prof_begin; a no-op otherwise) ----------------------------
bool prof_armed();
struct ProfScope {
    int slot;
    hipStream_t st;
    ProfScope(int kernel_id, double work, hipStream_t stream);
    ~ProfScope();
};

// ---- device helpers ----------------------------------------------------------------------------
constexpr int kWave = 64;

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
__device__ __forceinline__ int wave_id() { return threadIdx.x >> 6; }

// (the shuffle tree; kpx_wave.h has the same sums on the vector ALU for call sites known to run with all 64 lanes active)
template <class T> __device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;   // valid in lane 0
}
template <class T> __device__ __forceinline__ T wave_min(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { T t = __shfl_down(v, o, 64); v = t < v ? t : v; }
    return v;
}
template <class T> __device__ __forceinline__ T wave_max(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { T t = __shfl_down(v, o, 64); v = t > v ? t : v; }
    return v;
}

// wave-level ordering of LDS traffic (the DS unit executes one wave's instructions in order; this only stops the
// compiler from moving accesses across the point)
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Philox-4x32-10 (Salmon et al.): the counter-based generator behind every seeded draw (sampler keys, RANSAC triples)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        uint32_t n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Block-wide sum in a FIXED order (wave-tree, then waves in order): bitwise reproducible run to run.
// All threads must call; result valid in thread 0.  `sh` holds >= blockDim/64 elements of T.
template <class T> __device__ __forceinline__ T block_sum(T v, T *sh)
{
    v = wave_sum(v);
    __syncthreads();
    if (lane_id() == 0) sh[wave_id()] = v;
    __syncthreads();
    T r = T(0);
    if (threadIdx.x == 0) {
        int nw = (blockDim.x + 63) >> 6;
        for (int w = 0; w < nw; ++w) r += sh[w];
    }
    return r;
}

// inclusive scan across the wave
__device__ __forceinline__ int wave_incl_scan(int v)
{
    int l = lane_id();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { int t = __shfl_up(v, o, 64); if (l >= o) v += t; }
    return v;
}
// Block exclusive scan of one int per thread; returns the exclusive prefix, *total = block sum.
// sh: >= blockDim/64 + 1 ints.
__device__ __forceinline__ int block_excl_scan(int v, int *sh, int *total)
{
    int incl = wave_incl_scan(v);
    int nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane_id() == 63) sh[wave_id()] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int w = 0; w < nw; ++w) { int t = sh[w]; sh[w] = run; run += t; }
        sh[nw] = run;
    }
    __syncthreads();
    int base = sh[wave_id()];
    *total = sh[nw];
    return base + incl - v;
}

}  // namespace kpx
