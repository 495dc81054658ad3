// kpx_morton.h -- Morton (Z-curve) ordering of a cloud and point/box distance helpers, shared by the culled
// nearest-neighbour sweep (kpx_nnlocal.h) and the box-hierarchy k-NN of kpx_knn.hip.  Kernels are `static`: the
// header is included by more than one translation unit.
#pragma once
#include "kpx_cloudset.h"
#include "kpx_internal.h"
#include "kpx_sort.h"

namespace kpx {

constexpr float kBoxBig = 3.0e38f;

__device__ __forceinline__ uint32_t morton_spread10(uint32_t v)
{
    v &= 1023u;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
// 30-bit Hilbert index of three 10-bit cell coordinates (Skilling, "Programming the Hilbert curve", 2004: axes -> transpose, the
// transposed words' bits interleaved from the top).  The culled search orders rows and target columns along this curve: its
// consecutive cells are neighbours, the Z-curve's are not, and 16 consecutive points -- a wave's rows, a column tile -- are a third
// more compact (kpx_voxel.hip: voxel_hcode has the numbers).  The order decides which rows share a 16-row tile of the ICP sums, so
// another curve moves the transforms' last bits: the Z-curve form (slower, profiles/r03/exp_curve_hilbert.txt) is gone with its switch.
__device__ __forceinline__ uint32_t hilbert30(uint32_t x, uint32_t y, uint32_t z)
{
    uint32_t X[3] = { x & 1023u, y & 1023u, z & 1023u };
#pragma unroll
    for (uint32_t Q = 512u; Q > 1u; Q >>= 1) {
        const uint32_t P = Q - 1u;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const uint32_t t = (X[0] ^ X[i]) & P;
            const bool up = (X[i] & Q) != 0u;
            X[0] ^= up ? P : t;
            X[i] ^= up ? 0u : t;
        }
    }
    X[1] ^= X[0];
    X[2] ^= X[1];
    uint32_t t = 0u;
#pragma unroll
    for (uint32_t Q = 512u; Q > 1u; Q >>= 1) t ^= (X[2] & Q) ? Q - 1u : 0u;
    X[0] ^= t; X[1] ^= t; X[2] ^= t;
    // X[0]'s bit b is the most significant of the triple: spread and interleave
    return (morton_spread10(X[0]) << 2) | (morton_spread10(X[1]) << 1) | morton_spread10(X[2]);
}
__device__ __forceinline__ uint32_t curve_code30(const uint32_t q[3])
{
    return hilbert30(q[0], q[1], q[2]);
}
// 30-bit curve code of p in the grid of 1024^3 cells over the box bbox (cubic cells sized by the longest side; NaN -> cell 0)
__device__ __forceinline__ uint32_t curve_code_of(const float *__restrict__ p, const double *__restrict__ bbox)
{
    const double ext = fmax(bbox[3] - bbox[0], fmax(bbox[4] - bbox[1], bbox[5] - bbox[2]));
    const double scale = ext > 0.0 ? 1023.0 / ext : 0.0;
    uint32_t q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double v = ((double)p[a] - bbox[a]) * scale;
        q[a] = v >= 0.0 ? (uint32_t)(v < 1023.0 ? v : 1023.0) : 0u;          // NaN -> cell 0
    }
    return curve_code30(q);
}
static __global__ __launch_bounds__(256) void morton_key_kernel(const float *__restrict__ pts, int64_t n, const double *__restrict__ bbox,
                                                         uint32_t *__restrict__ keys, int32_t *__restrict__ vals)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = curve_code_of(pts + 3 * i, bbox);
    vals[i] = (int32_t)i;
}

// squared distance from a point to a box (0 inside) and to the box's farthest corner
__device__ __forceinline__ double pt_gap2(double x, double y, double z, const double lo[3], const double hi[3])
{
    const double gx = fmax(0.0, fmax(lo[0] - x, x - hi[0]));
    const double gy = fmax(0.0, fmax(lo[1] - y, y - hi[1]));
    const double gz = fmax(0.0, fmax(lo[2] - z, z - hi[2]));
    return fma(gz, gz, fma(gy, gy, gx * gx));
}
__device__ __forceinline__ double pt_far2(double x, double y, double z, const double lo[3], const double hi[3])
{
    const double fx = fmax(fabs(hi[0] - x), fabs(x - lo[0]));
    const double fy = fmax(fabs(hi[1] - y), fabs(y - lo[1]));
    const double fz = fmax(fabs(hi[2] - z), fabs(z - lo[2]));
    return fma(fz, fz, fma(fy, fy, fx * fx));
}
__device__ __forceinline__ void load_box(const float *__restrict__ bx, double lo[3], double hi[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = (double)bx[a]; hi[a] = (double)bx[3 + a]; }
}
// Morton order of a cloud: d_perm[r] = original index of the r-th point along the curve.
struct SortScratch {
    DeviceSort<uint32_t> sort;          // vals_out: the caller's d_perm
    double *bbox_part, *bbox;
};
static void sort_carve(Arena &a, int64_t n, SortScratch *s)
{
    SortOptions o;
    o.vals_out = false;
    dsort_carve(a, n, 30, o, &s->sort);
    s->bbox_part = a.get<double>((size_t)kBboxBlocks * 6);
    s->bbox = a.get<double>(8);
}
static int morton_order(const float *pts, int64_t n, const SortScratch &s, int32_t *d_perm, hipStream_t st)
{
    int rc = bbox_f32(pts, n, s.bbox, s.bbox_part, st);
    if (rc) return rc;
    DeviceSort<uint32_t> sort = s.sort;
    sort.vals_out = d_perm;
    hipLaunchKernelGGL(morton_key_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, pts, n, s.bbox, sort.keys_in, sort.vals_in);
    return dsort_run(sort, n, 30, st);
}

// ---- Morton order of several clouds with ONE sort -----------------------------------------------------------------
// A registration batch orders its shared target and every source: four sorts of 20-30k keys are ~60 short launches,
// and the host's launch rate, not the GPU, bounds such chains.  Here the clouds are concatenated, the cloud number sits
// above the 30 Morton bits of the key, and one stable sort orders them all (the ordering inside each cloud is the one
// morton_order produces).
constexpr int kMortonBatchMax = 8;
constexpr int kMortonBatchBboxBlocks = 32;
struct MortonBatch : CloudSet<kMortonBatchMax> {
    int32_t *perm[kMortonBatchMax];       // out: perm[c][r] = original index of the r-th point of cloud c along its curve
    double *bbox[kMortonBatchMax];        // out: (min x,y,z, max x,y,z) of cloud c
};
struct MortonBatchScratch {
    DeviceSort<uint64_t, true, kSortDefault32> sort;
    double *part;
};
static void morton_batch_carve(Arena &a, int64_t total, MortonBatchScratch *s)
{
    dsort_carve(a, total, 34, SortOptions(), &s->sort);
    s->part = a.get<double>((size_t)kMortonBatchMax * kMortonBatchBboxBlocks * 6);
}
static __global__ __launch_bounds__(256) void morton_batch_key_kernel(MortonBatch b, uint64_t *__restrict__ keys, int32_t *__restrict__ vals)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.off[b.count]) return;
    const int c = b.cloud_of(i);
    keys[i] = ((uint64_t)c << 30) | curve_code_of(b.pts[c] + 3 * (i - b.off[c]), b.bbox[c]);
    vals[i] = (int32_t)i;
}
static __global__ __launch_bounds__(256) void morton_batch_split_kernel(MortonBatch b, const int32_t *__restrict__ vals)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.off[b.count]) return;
    const int c = b.cloud_of(i);          // sorted position i lies in cloud c's range
    b.perm[c][i - b.off[c]] = vals[i] - (int32_t)b.off[c];
}
static __global__ __launch_bounds__(256) void morton_batch_iota_kernel(MortonBatch b)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.off[b.count]) return;
    const int c = b.cloud_of(i);
    b.perm[c][i - b.off[c]] = (int32_t)(i - b.off[c]);
}
// presorted: the caller's clouds already lie along a space-filling curve (the frame loop's voxel clouds, kpx_voxel.hip): the boxes
// are computed, the permutations are the identity, and the key / sort / split launches (12 of the 14) are skipped
static int morton_order_batch(const MortonBatch &b, const MortonBatchScratch &s, hipStream_t st, bool presorted = false)
{
    const int64_t total = b.off[b.count];
    BoxDst dst;
    for (int c = 0; c < kMortonBatchMax; ++c) dst.box[c] = b.bbox[c];
    dst.err = nullptr;
    hipLaunchKernelGGL((cloud_bbox_partial_kernel<MortonBatch, StoredPoint, float, kMortonBatchBboxBlocks>), dim3(kMortonBatchBboxBlocks, b.count), dim3(256), 0, st, b, s.part);
    hipLaunchKernelGGL(cloud_bbox_final_kernel<kMortonBatchBboxBlocks>, dim3(b.count), dim3(64), 0, st, (const double *)s.part, dst);
    const unsigned nb = (unsigned)cdiv(total, 256);
    if (presorted) {
        hipLaunchKernelGGL(morton_batch_iota_kernel, dim3(nb), dim3(256), 0, st, b);
        KPX_LAUNCH_CHECK();
        return KPX_OK;
    }
    hipLaunchKernelGGL(morton_batch_key_kernel, dim3(nb), dim3(256), 0, st, b, s.sort.keys_in, s.sort.vals_in);
    const int rc = dsort_run(s.sort, total, 34, st);
    if (rc) return rc;
    hipLaunchKernelGGL(morton_batch_split_kernel, dim3(nb), dim3(256), 0, st, b, s.sort.vals_out);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

}  // namespace kpx
