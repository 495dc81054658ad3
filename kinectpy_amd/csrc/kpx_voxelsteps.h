// kpx_voxelsteps.h -- the steps every voxel grid of the library runs, written once: the contract's cell index, the 63-bit key, the
// stable sort of (key, point id), head compaction and the per-voxel sequential fp64 sums.  kpx_voxel.hip (voxel_down_sample in its
// plain, batch and fused forms) and kpx_voxelgrid.hip (VoxelGrid.create_from_point_cloud) are host policies over them.
#pragma once
#include "kpx_compact.h"
#include "kpx_cloudset.h"
#include "kpx_internal.h"
#include "kpx_sort.h"

namespace kpx {

// ---- the steps every form shares ----------------------------------------------------------------------------------------
// The contract's cell index of q in the grid of the box `bbox`: f = floor((q - (min - v/2)) / v) per axis.  Returns true when an
// index lies outside [0, 2^21) -- the 21 bits an axis has in the 63-bit key -- or is NaN; own: the grid's own extents instead.
constexpr double kVoxelAxisCells = 2097152.0;
// voxel_cell_at: the same index in a grid whose origin is given (VoxelGrid: a caller's min_bound, inclusion queries).
__device__ __forceinline__ bool voxel_cell_at(const double q[3], const double org[3], double voxel, double f[3], const double *own = nullptr)
{
#pragma unroll
    for (int a = 0; a < 3; ++a) f[a] = floor((q[a] - org[a]) / voxel);
    if (!(f[0] >= 0.0) || !(f[1] >= 0.0) || !(f[2] >= 0.0)) return true;
    if (own) return !(f[0] < own[0]) || !(f[1] < own[1]) || !(f[2] < own[2]);
    return f[0] >= kVoxelAxisCells || f[1] >= kVoxelAxisCells || f[2] >= kVoxelAxisCells;
}
__device__ __forceinline__ bool voxel_cell(const double q[3], const double *__restrict__ bbox, double voxel, double f[3], const double *own = nullptr)
{
    const double org[3] = { bbox[0] - voxel * 0.5, bbox[1] - voxel * 0.5, bbox[2] - voxel * 0.5 };
    return voxel_cell_at(q, org, voxel, f, own);
}
// (key, concatenated index) of every point.  Src: the point source; Pack: the form's key layout -- grid() prepares it once per block
// (it may synchronise the block), put() writes the key of point i of cloud c and reports a bad index the form's way.
template <class Set, class Src, class Pack>
__global__ __launch_bounds__(256) void voxel_key_kernel(Set b, const double *__restrict__ bbox, double voxel, Pack pack, int32_t *__restrict__ vals)
{
    const typename Pack::Grid g = pack.grid(b, bbox, voxel);
    const int64_t total = b.off[b.count];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = b.cloud_of(i);
        double q[3];
        Src()(b, c, i - b.off[c], q);
        pack.put(g, bbox, voxel, i, c, q);
        vals[i] = (int32_t)i;
    }
}
// 63-bit fixed fields ix | iy | iz over the box bbox[0..5] (plain and fused form); a bad index sets *err
struct FixedKeys {
    struct Grid {};
    uint64_t *keys;
    int32_t *err;
    template <class Set> __device__ __forceinline__ Grid grid(const Set &, const double *, double) const { return Grid(); }
    __device__ __forceinline__ void put(const Grid &, const double *__restrict__ bbox, double voxel, int64_t i, int, const double q[3]) const
    {
        double f[3];
        if (voxel_cell(q, bbox, voxel, f)) { *err = 1; f[0] = f[1] = f[2] = 0.0; }
        keys[i] = ((uint64_t)f[0] << 42) | ((uint64_t)f[1] << 21) | (uint64_t)f[2];
    }
};

template <class Key> struct HeadPredT {
    const Key *keys;
    __device__ bool operator()(int64_t s, int) const { return s == 0 || keys[s] != keys[s - 1]; }
};
struct HeadEmit {
    int32_t *seg_start;
    __device__ void operator()(int64_t s, int, int32_t dst) const { seg_start[dst] = (int32_t)s; }
};

// Sums of the points at sorted positions [s0, s1) -- one voxel -- in ascending point index (the contract: sequential fp64 adds).
// Only the LOADS of 8 points are issued together: a dense voxel (a wall patch close to the camera holds 50+ points) was a chain
// of 2 dependent global loads per point, and the longest voxel set the kernel's duration.
// Load: the form's loader -- load(p, xyz, colour, normal) of the point with concatenated index p (Coord: float, or double for moved
// points), has_col() whether colours are summed.  NRM: normals are loaded and summed too (plain form only).
template <bool NRM, class Load>
__device__ __forceinline__ void voxel_segment_sum(const int32_t *__restrict__ vals, int64_t s0, int64_t s1, const Load &load, double sp[3],
                                                  double sc[3], double sn[3])
{
    for (int64_t s = s0; s < s1; s += 8) {
        const int cnt = (int)(s1 - s < 8 ? s1 - s : 8);
        int64_t p[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) p[k] = k < cnt ? vals[s + k] : -1;
        typename Load::Coord vp[8][3];
        float vc[8][3], vn[8][3];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (p[k] < 0) continue;
            load(p[k], vp[k], vc[k], vn[k]);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (p[k] < 0) continue;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                sp[a] += (double)vp[k][a];
                if (load.has_col()) sc[a] += (double)vc[k][a];
                if (NRM) sn[a] += (double)vn[k][a];
            }
        }
    }
}
// one row of means; ocol null: no colours
__device__ __forceinline__ void voxel_write_row(const double sp[3], const double sc[3], double cn, float *__restrict__ opts, float *__restrict__ ocol)
{
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        opts[a] = (float)(sp[a] / cn);
        if (ocol) ocol[a] = (float)(sc[a] / cn);
    }
}
// points of one cloud with optional colours and normals (plain form; a cloud of the batch form: base = its first concatenated index)
struct StoredLoad {
    using Coord = float;
    const float *pts, *col, *nrm;
    int64_t base;
    __device__ __forceinline__ bool has_col() const { return col != nullptr; }
    __device__ __forceinline__ void operator()(int64_t p, float v[3], float c[3], float n[3]) const
    {
        const int64_t j = p - base;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            v[a] = pts[3 * j + a];
            if (col) c[a] = col[3 * j + a];
            if (nrm) n[a] = nrm[3 * j + a];
        }
    }
};

// Scratch of a form.  VoxelCarve: what distinguishes the forms' workspaces -- the cloud slots, the blocks of a cloud's partial
// bounding boxes, boxes / error words per cloud (with the batch form's head table) or one for all, whether the form also writes keys
// of at most 32 bits as 32-bit words (sorted through dsort_view32, by the library's own radix sort where that serves), and the
// widest key the form sorts.
using VoxelSort = DeviceSort<uint64_t, true, kSortDefault32>;
struct VoxelScratch {
    int32_t *seg_start, *counts, *err, *head, *d_total;
    double *part, *bbox;
    VoxelSort sort;
    char *counts_end;
};
struct VoxelCarve {
    int clouds, bbox_blocks;
    bool per_cloud, keys32;
    int end_bit;
};
static void voxel_carve(Arena &a, int64_t total, const VoxelCarve &v, VoxelScratch *s)
{
    const size_t nn = (size_t)(total > 0 ? total : 1);
    s->seg_start = a.get<int32_t>(nn);
    s->err = a.get<int32_t>(v.per_cloud ? v.clouds : 1);
    s->head = v.per_cloud ? a.get<int32_t>(v.clouds + 1) : nullptr;
    s->d_total = v.per_cloud ? a.get<int32_t>(1) : nullptr;
    s->part = a.get<double>((size_t)v.clouds * v.bbox_blocks * 6);
    s->bbox = a.get<double>((size_t)(v.per_cloud ? v.clouds : 1) * 8);
    SortOptions o;
    if (v.keys32) { o.radix = kRadixAndVendor; o.tmp_floor = dsort_view32_bytes(total); }
    dsort_carve(a, total, v.end_bit, o, &s->sort);
    s->counts = a.get<int32_t>((size_t)compact_ws_ints(total));          // right behind the sort's cleared histograms: one memset for both
    s->counts_end = reinterpret_cast<char *>(s->counts + (size_t)compact_ws_ints(total));
}

// Stable sort of the (key, index) pairs on key bits [0, end_bit), then the segment heads: seg_start[m] = first sorted position of the
// m-th distinct key, *d_heads = their number.  Key: how the form wrote its keys -- 64-bit words, or 32-bit ones (three 8-bit passes of
// the own radix sort for a frame's ~24 bits, against the vendor's eight passes over 64-bit keys).
template <class Key>
static int voxel_sort_and_heads(const VoxelScratch &s, int64_t total, int end_bit, int32_t *d_heads, hipStream_t st)
{
    const bool narrow = sizeof(Key) == 4;
    const DeviceSortView32 v = dsort_view32(s.sort);
    const bool cleared = narrow && dsort_by_radix(v, total);
    const int rc = narrow ? dsort_run(v, total, end_bit, st, s.counts_end) : dsort_run(s.sort, total, end_bit, st);
    if (rc) return rc;
    return compact(HeadPredT<Key>{ reinterpret_cast<const Key *>(s.sort.keys_out) }, HeadEmit{ s.seg_start }, total, 1, s.counts, d_heads, st, cleared);
}

// the plain form's scratch: one cloud, 63-bit keys, the vendor sort
constexpr VoxelCarve kPlainCarve = { 1, kBboxBlocks, false, false, 63 };

}  // namespace kpx
