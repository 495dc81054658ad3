// kpx_cloudset.h -- several clouds handled as ONE concatenated index space: the voxel grids of kpx_voxel.hip (batch and fused
// forms) and the batched Morton order of kpx_morton.h.  Holds what those forms share below their host policy: the cloud set with
// its index lookup, the two point sources and the per-cloud bounding boxes.
#pragma once
#include "kpx_box.h"

namespace kpx {

// cloud c owns [off[c], off[c+1]) of the concatenated index space; slots >= count hold off[count] and null pointers
template <int MAX> struct CloudSet {
    static constexpr int kMax = MAX;
    const float *pts[MAX];
    int64_t off[MAX + 1];
    int32_t count;
    // which cloud owns concatenated index i (branch-free: the clouds before i's are counted)
    __device__ __forceinline__ int cloud_of(int64_t i) const
    {
        int c = 0;
#pragma unroll
        for (int k = 1; k < MAX; ++k) c += (k < count && i >= off[k]) ? 1 : 0;
        return c;
    }
};

// ---- point sources: point j of cloud c as fp64 ------------------------------------------------------------------------
// the stored float32 point, widened (exact)
struct StoredPoint {
    template <class Set> __device__ __forceinline__ void operator()(const Set &b, int c, int64_t j, double o[3]) const
    {
        const float *p = b.pts[c] + 3 * j;
        o[0] = (double)p[0]; o[1] = (double)p[1]; o[2] = (double)p[2];
    }
};
// the point moved by the cloud's [R | t] (rows in b.T[c], or in device memory at b.dT[c]): 9 fma, recomputed wherever the moved
// point is needed -- the fused stack is never stored (kpx_voxel.hip)
struct MovedPoint {
    template <class Set> __device__ __forceinline__ void operator()(const Set &b, int c, int64_t j, double o[3]) const
    {
        const float *p = b.pts[c] + 3 * j;
        const double x = p[0], y = p[1], z = p[2];
        const double *T = b.dT[c] ? b.dT[c] : b.T[c];
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = fma(T[4 * k], x, fma(T[4 * k + 1], y, fma(T[4 * k + 2], z, T[4 * k + 3])));
    }
};

// ---- bounding boxes (min / max: exact and order-free, so every fold gives the same bits) -------------------------------
// grid (BLOCKS, count): block x of cloud c folds its share of the cloud -> part[(c * BLOCKS + x) * 6 + 0..5] = (min xyz, max xyz).
// Acc: float for stored points (min / max of float32 values need no more), double for moved ones.
template <class Set, class Src, class Acc, int BLOCKS>
__global__ __launch_bounds__(256) void cloud_bbox_partial_kernel(Set b, double *__restrict__ part)
{
    const int c = blockIdx.y;
    const int64_t n = b.off[c + 1] - b.off[c];
    Acc mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        double q[3];
        Src()(b, c, i, q);
#pragma unroll
        for (int a = 0; a < 3; ++a) { const Acc v = (Acc)q[a]; mn[a] = fmin(mn[a], v); mx[a] = fmax(mx[a], v); }
    }
    box_block_fold<4>(mn, mx, part + ((int64_t)c * BLOCKS + blockIdx.x) * 6);
}
// where the box of cloud c goes; err non-null: the cloud's error word, zeroed with it
struct BoxDst {
    double *box[8];
    int32_t *err;
};
// one wave per cloud: folds the cloud's BLOCKS <= 64 partial boxes -> dst.box[c][0..5]
template <int BLOCKS>
__global__ __launch_bounds__(64) void cloud_bbox_final_kernel(const double *__restrict__ part, BoxDst dst)
{
    static_assert(BLOCKS <= 64, "one lane per partial box");
    const int c = blockIdx.x, lane = lane_id();
    double v[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) v[a] = lane < BLOCKS ? part[((int64_t)c * BLOCKS + lane) * 6 + a] : (a < 3 ? (double)INFINITY : -(double)INFINITY);
    box_wave_fold(v, v + 3);
    if (lane == 0) {
        for (int a = 0; a < 6; ++a) dst.box[c][a] = v[a];
        if (dst.err) dst.err[c] = 0;
    }
}

}  // namespace kpx
