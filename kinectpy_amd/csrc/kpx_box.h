// kpx_box.h -- the folds every bounding-box kernel ends with.  A box is a row of six doubles (min xyz, max xyz); min / max are
// exact and order-free, so every fold gives the same bits.  The kernels keep their own load loops.
#pragma once
#include "kpx_common.h"

namespace kpx {

// the wave's box, valid in lane 0
template <class Acc> __device__ __forceinline__ void box_wave_fold(Acc mn[3], Acc mx[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) { mn[a] = wave_min(mn[a]); mx[a] = wave_max(mx[a]); }
}
// Block fold: every thread of a block of WAVES waves brings its own box; threads 0..5 write the block's box to row[0..5].
// Acc: float for stored float32 points (their min / max need no more), double otherwise.
template <int WAVES, class Acc> __device__ __forceinline__ void box_block_fold(Acc mn[3], Acc mx[3], double *__restrict__ row)
{
    __shared__ Acc sh[6][WAVES];
    box_wave_fold(mn, mx);
    if (lane_id() == 0)
        for (int a = 0; a < 3; ++a) { sh[a][wave_id()] = mn[a]; sh[3 + a][wave_id()] = mx[a]; }
    __syncthreads();
    if (threadIdx.x < 6) {
        Acc v = sh[threadIdx.x][0];
        for (int w = 1; w < WAVES; ++w) v = threadIdx.x < 3 ? fmin(v, sh[threadIdx.x][w]) : fmax(v, sh[threadIdx.x][w]);
        row[threadIdx.x] = (double)v;
    }
}

}  // namespace kpx
