// kpx_voxel.hip -- a7: PointCloud.voxel_down_sample (preprocessing/filtering.py:23,
// preprocessing/registration.py:8,100,101).
//   origin = min_bound - v/2 ; index = floor((p - origin)/v)   (fp64, identical to the oracle)
//   63-bit key (21 bits per axis), stable radix sort of (key, point id), one thread per voxel sums
//   its points in ascending original index (fp64, sequential) -> bit-exact means.
// Output order: ascending (ix,iy,iz).
//
// Three forms -- plain (voxel_impl: one cloud, normals), batch (voxel_batch_impl: up to 8 clouds in one pass) and fused
// (fuse_voxel_impl: transform + stack + voxel grid) -- run the same steps: bounding box, cell index, key, stable sort, head
// compaction, per-voxel mean.  Each step is written once, in kpx_voxelsteps.h and kpx_cloudset.h; a form is its host policy -- key layout and
// width, sort, read-back, speculation -- plus a key packer and a point loader.
#include "kpx_voxelsteps.h"

namespace kpx {

// ---- plain form: one cloud, colours and normals -----------------------------------------------------------------------------
template <bool NRM>
__global__ __launch_bounds__(256) void voxel_mean_kernel(StoredLoad load, int64_t n, const int32_t *__restrict__ vals, const int32_t *__restrict__ seg_start,
                                                         int32_t *__restrict__ d_count, const int32_t *__restrict__ err, float *__restrict__ opts,
                                                         float *__restrict__ ocol, float *__restrict__ onrm)
{
    const int32_t m_total = *d_count;
    // index overflow is reported through the count word (the host sees KPX_ERR_RANGE when it reads it); a block that reads
    // the count after this store sees a negative total and does nothing -- the output is invalid in that case anyway
    if (blockIdx.x == 0 && threadIdx.x == 0 && *err) *d_count = KPX_ERR_RANGE;
    for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < m_total; m += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s0 = seg_start[m], s1 = (m + 1 < m_total) ? seg_start[m + 1] : n;
        double sp[3] = { 0, 0, 0 }, sc[3] = { 0, 0, 0 }, sn[3] = { 0, 0, 0 };
        voxel_segment_sum<NRM>(vals, s0, s1, load, sp, sc, sn);
        voxel_write_row(sp, sc, (double)(s1 - s0), opts + 3 * m, (load.col && ocol) ? ocol + 3 * m : nullptr);
        if (NRM && onrm) {
            double nn = sqrt(fma(sn[2], sn[2], fma(sn[1], sn[1], sn[0] * sn[0])));
#pragma unroll
            for (int a = 0; a < 3; ++a) onrm[3 * m + a] = (float)(nn > 0 ? sn[a] / nn : sn[a]);
        }
    }
}
static int voxel_impl(const float *pts, const float *col, const float *nrm, int64_t n, double voxel, float *opts,
                      float *ocol, float *onrm, int32_t *d_count, Arena &a, hipStream_t st)
{
    VoxelScratch s;
    voxel_carve(a, n, kPlainCarve, &s);
    KPX_ARENA_CHECK(a);
    int rc = bbox_f32(pts, n, s.bbox, s.part, st);
    if (rc) return rc;
    KPX_HIP(hipMemsetAsync(s.err, 0, sizeof(int32_t), st));
    int nb = (int)(cdiv(n, 256) > 4096 ? 4096 : cdiv(n, 256));
    CloudSet<1> one;
    one.pts[0] = pts; one.off[0] = 0; one.off[1] = n; one.count = 1;
    hipLaunchKernelGGL((voxel_key_kernel<CloudSet<1>, StoredPoint, FixedKeys>), dim3(nb), dim3(256), 0, st, one, (const double *)s.bbox, voxel,
                       FixedKeys{ s.sort.keys_in, s.err }, s.sort.vals_in);
    rc = voxel_sort_and_heads<uint64_t>(s, n, 63, d_count, st);
    if (rc) return rc;
    const StoredLoad load = { pts, col, nrm, 0 };
    const auto mean_kernel = nrm ? &voxel_mean_kernel<true> : &voxel_mean_kernel<false>;
    hipLaunchKernelGGL(mean_kernel, dim3(nb), dim3(256), 0, st, load, n, (const int32_t *)s.sort.vals_out,
                       (const int32_t *)s.seg_start, d_count, (const int32_t *)s.err, opts, ocol, onrm);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

// ---- several clouds in ONE pass ---------------------------------------------------------------------------------
// A voxel grid of an 85k-point cloud is ~28 short launches (bounding box, keys, the merge passes of the sort, head
// compaction, means), and the pipeline down-samples 4 clouds per frame: queued on four lanes the work overlaps on the
// GPU, but the host cannot issue 112 launches faster than ~0.6 ms.  Here the clouds are handled as one concatenated
// array: per-cloud bounding boxes, the cloud number as the most significant digit of the key -- mixed radix
// ((c DX + ix) DY + iy) DZ + iz with DX, DY, DZ the largest grid extents of the batch, so it fits 64 bits whenever the
// single-cloud key does -- ONE stable sort, ONE head compaction, ONE mean kernel.  Results are identical to the
// single-cloud path: same voxel indices (own origin per cloud), ascending (ix, iy, iz) per cloud, sums in ascending
// point index.
constexpr int kVoxelBatchMax = 8;
constexpr int kVoxelBatchBboxBlocks = 64;
constexpr VoxelCarve kBatchCarve = { kVoxelBatchMax, kVoxelBatchBboxBlocks, true, true, 64 };
struct VoxelBatch : CloudSet<kVoxelBatchMax> {
    const float *col[kVoxelBatchMax];
    float *opts[kVoxelBatchMax];
    float *ocol[kVoxelBatchMax];
    int32_t morton;                       // keys = cloud | curve code of (ix, iy, iz) instead of cloud | (ix, iy, iz) row-major: 1 = along the Hilbert curve
};
// clouds [first, first + count) of the caller's arrays (h_col / h_ocol may be null: no colours)
static VoxelBatch voxel_batch_of(const float *const *h_pts, const float *const *h_col, const int64_t *h_n, float *const *h_opts, float *const *h_ocol,
                                 int first, int count, bool morton)
{
    VoxelBatch b;
    b.count = count;
    b.morton = morton ? 1 : 0;
    b.off[0] = 0;
    for (int i = 0; i < kVoxelBatchMax; ++i) {
        const bool on = i < count;
        b.pts[i] = on ? h_pts[first + i] : nullptr;
        b.col[i] = (on && h_col) ? h_col[first + i] : nullptr;
        b.opts[i] = on ? h_opts[first + i] : nullptr;
        b.ocol[i] = (on && h_col && h_ocol) ? h_ocol[first + i] : nullptr;
        b.off[i + 1] = b.off[i] + (on ? h_n[first + i] : 0);
    }
    return b;
}
// bits per axis: enough for the axis' largest index in the batch.  A Z-curve code (round 2; removed: slower, and another order moves the
// ICP transforms' last bits) interleaves bit q of every axis that still has a bit q, so its width is the SUM of the three widths -- a long axis costs its own extra bits only, not
// three times them (a frame's 26-bit cube code would be a fourth radix pass; 7 + 7 + 8 bits + 2 for the cloud stay within three)
__device__ __forceinline__ void voxel_batch_axis_bits(const double d[3], int bits[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const unsigned long long m = (unsigned long long)d[a] - 1ull;          // largest index
        int n = 1;
        while (n < 21 && (m >> n) != 0ull) ++n;
        bits[a] = n;
    }
}
// Hilbert index of (x, y, z), `bits` bits per axis (Skilling, "Programming the Hilbert curve", 2004: axes -> transpose, then the bits
// of the three transposed words interleaved from the top).  Consecutive cells of the curve are neighbours, which the Z-curve's
// are not: 16 consecutive points of a surface cloud -- a wave's rows, a target tile of the culled ICP sweep (kpx_nnlocal.h) -- span
// 177 instead of 246 mm (median; p99 677 instead of 1255) on the bench's 35 mm clouds, a wave multiplies 2.0 instead of 3.0 tiles
// on average (p99 9 instead of 13; profiles/r03/exp_curve_hilbert.txt).  `bits` >= 1.
// Word: the integer the bit loops run in -- uint64_t, or uint32_t when 3 `bits` <= 32 (a 64-bit shift, and, xor is two or more vector
// instructions per step; the values are the same numbers).
template <class Word> __device__ __forceinline__ Word voxel_hcode(Word x, Word y, Word z, int bits)
{
    Word X[3] = { x, y, z };
    const Word M = (Word)1 << (bits - 1);
    for (Word Q = M; Q > (Word)1; Q >>= 1) {
        const Word P = Q - (Word)1;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (X[i] & Q) X[0] ^= P;
            else { const Word t = (X[0] ^ X[i]) & P; X[0] ^= t; X[i] ^= t; }
        }
    }
    X[1] ^= X[0];
    X[2] ^= X[1];
    Word t = 0;
    for (Word Q = M; Q > (Word)1; Q >>= 1)
        if (X[2] & Q) t ^= Q - (Word)1;
    X[0] ^= t; X[1] ^= t; X[2] ^= t;
    Word k = 0;
    for (int b = bits - 1; b >= 0; --b) {
#pragma unroll
        for (int i = 0; i < 3; ++i) k = (k << 1) | ((X[i] >> b) & (Word)1);
    }
    return k;
}
// Width m of the cube the Hilbert code covers when the axes need ab[0..2] bits: the largest m <= max(ab) whose key -- the axes' bits
// above m, row-major, then the 3 m bits of the cube's code -- takes no more 8-bit sort passes than the Z-code's ab[0] + ab[1] + ab[2]
// bits (cloud number included: cb bits).  m = min(ab) always qualifies; a frame's 7 + 7 + 8 bits give m = 7: two cubes stacked
// along z, one jump of the curve between them, three passes as before.
__device__ __forceinline__ int voxel_hilbert_cube_bits(const int ab[3], int cb)
{
    const int top = ab[0] > ab[1] ? (ab[0] > ab[2] ? ab[0] : ab[2]) : (ab[1] > ab[2] ? ab[1] : ab[2]);
    const int low = ab[0] < ab[1] ? (ab[0] < ab[2] ? ab[0] : ab[2]) : (ab[1] < ab[2] ? ab[1] : ab[2]);
    const int passes = (ab[0] + ab[1] + ab[2] + cb + 7) / 8;
    for (int m = top; m > low; --m) {
        int n = 3 * m + cb;
#pragma unroll
        for (int a = 0; a < 3; ++a) n += ab[a] > m ? ab[a] - m : 0;
        if (n <= 64 && (n + 7) / 8 <= passes) return m;
    }
    return low;
}
__device__ __forceinline__ int voxel_hilbert_key_bits(const int ab[3], int m)
{
    int n = 3 * m;
#pragma unroll
    for (int a = 0; a < 3; ++a) n += ab[a] > m ? ab[a] - m : 0;
    return n;
}
// key of one voxel: [x >> m | y >> m | z >> m] (row-major over the cubes) above the cube's Hilbert code of the low m bits.
// Word = uint32_t: voxel_hilbert_key_bits(ab, m) <= 31 and every axis value below 2^ab[a] (the key and every shift fit the word).
template <class Word> __device__ __forceinline__ Word voxel_hilbert_key(Word x, Word y, Word z, const int ab[3], int m)
{
    const Word mask = ((Word)1 << m) - (Word)1;
    const int ey = ab[1] > m ? ab[1] - m : 0, ez = ab[2] > m ? ab[2] - m : 0;
    const Word hi = (((x >> m) << ey | (y >> m)) << ez) | (z >> m);
    return (hi << (3 * m)) | voxel_hcode<Word>(x & mask, y & mask, z & mask, m);
}
// largest grid extents of the batch (index < floor((max - origin) / v) + 1) and whether count x DX x DY x DZ fits 64 bits
__device__ __forceinline__ void voxel_batch_dims(const VoxelBatch &b, const double *__restrict__ bbox, double voxel, double d[3], int *overflow)
{
    d[0] = d[1] = d[2] = 1.0;
    for (int c = 0; c < b.count; ++c) {
        if (b.off[c + 1] == b.off[c]) continue;
        double f[3];
        (void)voxel_cell(bbox + 8 * c + 3, bbox + 8 * c, voxel, f);      // the cell of the box's far corner
        for (int a = 0; a < 3; ++a) {
            const double e = f[a] + 1.0;
            if (e > d[a] && e < kVoxelAxisCells) d[a] = e;        // out-of-range clouds are flagged per point by the key kernel
        }
    }
    *overflow = ((double)b.count * d[0]) * (d[1] * d[2]) >= 18446744073709551616.0 ? 1 : 0;
}
// bits the keys of this batch occupy: batches above rocPRIM's merge-sort limit are sorted by Onesweep, one pass per 8 bits --
// a 4-sensor frame needs ~24 of the 64
__device__ __forceinline__ int voxel_batch_key_bits(const VoxelBatch &b, const double d[3], int overflow)
{
    int n = 64;
    if (!overflow && b.morton) {
        int cb = 0, ab[3];
        while ((1 << cb) < b.count) ++cb;
        voxel_batch_axis_bits(d, ab);
        n = voxel_hilbert_key_bits(ab, voxel_hilbert_cube_bits(ab, cb)) + cb;
        n = n < 1 ? 1 : (n > 64 ? 64 : n);
    } else if (!overflow) {
        const unsigned long long range = (((unsigned long long)b.count * (unsigned long long)d[0]) * (unsigned long long)d[1]) * (unsigned long long)d[2];
        n = 1;
        while (n < 64 && (range >> n) != 0ull) ++n;
    }
    return n;
}
__global__ void voxel_batch_bits_kernel(VoxelBatch b, const double *__restrict__ bbox, double voxel, int32_t *__restrict__ bits)
{
    double d[3];
    int overflow;
    voxel_batch_dims(b, bbox, voxel, d, &overflow);
    *bits = voxel_batch_key_bits(b, d, overflow);
}
// mixed radix ((c DX + ix) DY + iy) DZ + iz, or cloud | Hilbert key, over the boxes bbox[8 c ..]; a bad index sets err[c].  The
// block's first thread works the layout out once; bits_out: the speculated width's check (the caller compares afterwards)
template <class Key> struct BatchKeys {
    struct Grid {
        uint64_t DX, DY, DZ;
        int overflow, morton, ab[3], m;
        int kb;                             // width of the curve key below the cloud number
        int narrow;                         // the whole key fits 32 bits: cloud | curve key, or count x DX x DY x DZ < 2^32
    };
    Key *keys;
    int32_t *err, *bits_out;
    __device__ __forceinline__ Grid grid(const VoxelBatch &b, const double *__restrict__ bbox, double voxel) const
    {
        __shared__ double dims[3];
        __shared__ int overflow, axis_bits[3], cube_bits, key_bits, narrow;
        if (threadIdx.x == 0) {
            double d[3];
            int ov;
            voxel_batch_dims(b, bbox, voxel, d, &ov);
            if (bits_out && blockIdx.x == 0) *bits_out = voxel_batch_key_bits(b, d, ov);
            dims[0] = d[0]; dims[1] = d[1]; dims[2] = d[2];
            int ab[3], cb = 0;
            voxel_batch_axis_bits(d, ab);
            axis_bits[0] = ab[0]; axis_bits[1] = ab[1]; axis_bits[2] = ab[2];
            while ((1 << cb) < b.count) ++cb;
            cube_bits = voxel_hilbert_cube_bits(ab, cb);
            key_bits = voxel_hilbert_key_bits(ab, cube_bits);
            overflow = (ov || (b.morton && key_bits + cb > 64)) ? 1 : 0;
            // 32-bit words throughout: every value and every shift of the key then fits one (a valid point's index on axis a is below
            // d[a] <= 2^ab[a]; a bad one's is 0).  key_bits <= 31 keeps the cloud number's shift defined when cb = 0.
            if (b.morton) narrow = (!overflow && key_bits + cb <= 32 && key_bits <= 31) ? 1 : 0;
            else narrow = (!ov && ((double)b.count * d[0]) * (d[1] * d[2]) < 4294967296.0) ? 1 : 0;
        }
        __syncthreads();
        return Grid{ (uint64_t)dims[0], (uint64_t)dims[1], (uint64_t)dims[2], overflow, b.morton, { axis_bits[0], axis_bits[1], axis_bits[2] }, cube_bits,
                     key_bits, narrow };
    }
    __device__ __forceinline__ void put(const Grid &g, const double *__restrict__ bbox, double voxel, int64_t i, int c, const double q[3]) const
    {
        double f[3];
        const bool bad = voxel_cell(q, bbox + 8 * c, voxel, f) || g.overflow;
        if (bad) { err[c] = 1; f[0] = f[1] = f[2] = 0.0; }
        if constexpr (sizeof(Key) == 4) {
            if (g.narrow) {                  // block-uniform; the same numbers as the 64-bit form below, which truncates its result to Key
                if (g.morton) keys[i] = ((uint32_t)c << g.kb) | voxel_hilbert_key<uint32_t>((uint32_t)f[0], (uint32_t)f[1], (uint32_t)f[2], g.ab, g.m);
                else keys[i] = (((uint32_t)c * (uint32_t)g.DX + (uint32_t)f[0]) * (uint32_t)g.DY + (uint32_t)f[1]) * (uint32_t)g.DZ + (uint32_t)f[2];
                return;
            }
        }
        if (g.morton) keys[i] = (Key)(((uint64_t)c << g.kb) | voxel_hilbert_key<uint64_t>((uint64_t)f[0], (uint64_t)f[1], (uint64_t)f[2], g.ab, g.m));
        else keys[i] = (Key)((((uint64_t)c * g.DX + (uint64_t)f[0]) * g.DY + (uint64_t)f[1]) * g.DZ + (uint64_t)f[2]);
    }
};
// head[c] = number of voxels (segment heads) before cloud c in the sorted array; d_counts[c] = voxels of cloud c
__global__ __launch_bounds__(64) void voxel_batch_locate_kernel(VoxelBatch b, const int32_t *__restrict__ seg_start, const int32_t *__restrict__ d_total,
                                                                const int32_t *__restrict__ err, int32_t *__restrict__ head, int32_t *__restrict__ d_counts)
{
    __shared__ int32_t h[kVoxelBatchMax + 1];
    const int c = threadIdx.x;
    const int32_t m = *d_total;
    if (c <= b.count) {
        int32_t lo = 0, hi = m;                      // first head position >= off[c]
        const int64_t want = b.off[c];
        while (lo < hi) {
            const int32_t mid = lo + (hi - lo) / 2;
            if (seg_start[mid] < want) lo = mid + 1; else hi = mid;
        }
        h[c] = c == b.count ? m : lo;
        head[c] = h[c];
    }
    __syncthreads();
    if (c < b.count) d_counts[c] = err[c] ? KPX_ERR_RANGE : h[c + 1] - h[c];
}
__global__ __launch_bounds__(256) void voxel_batch_mean_kernel(VoxelBatch b, const int32_t *__restrict__ vals, const int32_t *__restrict__ seg_start,
                                                               const int32_t *__restrict__ d_total, const int32_t *__restrict__ head)
{
    const int32_t m_total = *d_total;
    const int64_t total = b.off[b.count];
    for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < m_total; m += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s0 = seg_start[m], s1 = (m + 1 < m_total) ? seg_start[m + 1] : total;
        const int c = b.cloud_of(s0);                // the sorted array keeps the clouds' ranges: position s0 tells the cloud
        const StoredLoad load = { b.pts[c], b.col[c], nullptr, b.off[c] };
        double sp[3] = { 0, 0, 0 }, sc[3] = { 0, 0, 0 }, sn[3];
        voxel_segment_sum<false>(vals, s0, s1, load, sp, sc, sn);
        const int64_t o = m - head[c];
        voxel_write_row(sp, sc, (double)(s1 - s0), b.opts[c] + 3 * o, (load.col && b.ocol[c]) ? b.ocol[c] + 3 * o : nullptr);
    }
}

// spec_bits > 0 (frame loop): the key width is NOT read back -- the sort covers spec_bits bits and *d_bits receives the width the
// batch really needs; the caller compares the two after its own read-back of the counts and repeats the call with spec_bits = 0
// when the speculation was too narrow (the outputs of that call are garbage).
static int voxel_batch_impl(const VoxelBatch &b, double voxel, int32_t *d_counts, Arena &a, hipStream_t st, int spec_bits = 0,
                            int32_t *d_bits = nullptr)
{
    const int64_t total = b.off[b.count];
    VoxelScratch s;
    voxel_carve(a, total, kBatchCarve, &s);
    KPX_ARENA_CHECK(a);
    BoxDst boxes;
    for (int c = 0; c < kVoxelBatchMax; ++c) boxes.box[c] = s.bbox + 8 * c;
    boxes.err = s.err;
    hipLaunchKernelGGL((cloud_bbox_partial_kernel<VoxelBatch, StoredPoint, float, kVoxelBatchBboxBlocks>), dim3(kVoxelBatchBboxBlocks, b.count), dim3(256), 0, st, b, s.part);
    hipLaunchKernelGGL(cloud_bbox_final_kernel<kVoxelBatchBboxBlocks>, dim3(b.count), dim3(64), 0, st, (const double *)s.part, boxes);
    const int nb = (int)(cdiv(total, 256) > 4096 ? 4096 : cdiv(total, 256));
    int end_bit = 64;
    int32_t *bits_out = nullptr;
    if (spec_bits > 0 && d_bits) {
        bits_out = d_bits;                               // written by the key kernel itself
        end_bit = spec_bits > 64 ? 64 : spec_bits;
    } else if (total > (int64_t)128 * 1024) {
        // reading the key width back (one small round trip; the caller waits for the counts anyway) lets keys of at most 32 bits
        // (a 4-sensor frame needs ~25, a 1M-point room at 10 mm 25) be written, sorted and compared as 32-bit words by the library's
        // own radix sort -- three 8-bit passes instead of the vendor sort's eight over 64-bit keys.  Below ~128k points the vendor's
        // merge sort of a handful of launches is as fast as the round trip.
        int32_t *h_bits = static_cast<int32_t *>(thread_resources().pinned(kPinVoxelBits, sizeof(int32_t)));
        if (!h_bits) return KPX_ERR_HIP;
        hipLaunchKernelGGL(voxel_batch_bits_kernel, dim3(1), dim3(1), 0, st, b, s.bbox, voxel, s.head);
        KPX_HIP(hipMemcpyAsync(h_bits, s.head, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (d_bits) KPX_HIP(hipMemcpyAsync(d_bits, s.head, sizeof(int32_t), hipMemcpyDefault, st));      // d_bits may be pinned host memory (kpx_frame_step)
        KPX_HIP(hipStreamSynchronize(st));
        end_bit = *h_bits < 1 ? 1 : (*h_bits > 64 ? 64 : *h_bits);
    } else if (d_bits) {
        hipLaunchKernelGGL(voxel_batch_bits_kernel, dim3(1), dim3(1), 0, st, b, s.bbox, voxel, d_bits);      // for the caller's next speculation
    }
    int rc;
    if (end_bit <= 32) {
        hipLaunchKernelGGL((voxel_key_kernel<VoxelBatch, StoredPoint, BatchKeys<uint32_t>>), dim3(nb), dim3(256), 0, st, b, (const double *)s.bbox, voxel,
                           BatchKeys<uint32_t>{ reinterpret_cast<uint32_t *>(s.sort.keys_in), s.err, bits_out }, s.sort.vals_in);
        rc = voxel_sort_and_heads<uint32_t>(s, total, end_bit, s.d_total, st);
    } else {
        hipLaunchKernelGGL((voxel_key_kernel<VoxelBatch, StoredPoint, BatchKeys<uint64_t>>), dim3(nb), dim3(256), 0, st, b, (const double *)s.bbox, voxel,
                           BatchKeys<uint64_t>{ s.sort.keys_in, s.err, bits_out }, s.sort.vals_in);
        rc = voxel_sort_and_heads<uint64_t>(s, total, end_bit, s.d_total, st);
    }
    if (rc) return rc;
    hipLaunchKernelGGL(voxel_batch_locate_kernel, dim3(1), dim3(64), 0, st, b, s.seg_start, s.d_total, s.err, s.head, d_counts);
    hipLaunchKernelGGL(voxel_batch_mean_kernel, dim3(nb), dim3(256), 0, st, b, s.sort.vals_out, s.seg_start, s.d_total, s.head);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

// ---- transform + fuse + voxel grid in one pass (preprocessing/data.py:44-61) ----------------------------------------
// Cloud c of the frame is moved by its registration T[c] (identity for the master), the clouds are stacked and the stack is
// down-sampled.  The reference keeps the moved points as float64 arrays; storing them as float32 first would move points
// that lie within 2^-24 |x| of a voxel face into the neighbouring voxel (measured: ~1e-5 of the points,
// oracle/storage_deviation.py).  So the stack is never materialised: the bounding box, the voxel index and the per-voxel
// sums all use the fp64 value p' = AC1(T[c], p), recomputed from the float32 sensor point wherever it is needed (9 fma:
// MovedPoint).  That is also one pass less over HBM and three launches less per sensor than transform -> concat -> voxel.
constexpr int kFuseMax = 16;
constexpr int kFuseBboxBlocks = 32;
constexpr VoxelCarve kFuseCarve = { kFuseMax, kFuseBboxBlocks, false, true, 63 };
struct FuseBatch : CloudSet<kFuseMax> {
    const float *col[kFuseMax];
    double T[kFuseMax][12];               // rows of [R | t]
    const double *dT[kFuseMax];           // non-null: the cloud's 4x4 (row-major, first 12 entries used) is read from device memory instead --
                                          // the frame loop hands over the registrations' results without a host round trip
};
// folds the count x kFuseBboxBlocks partial boxes (min / max: exact, order-free) -> bbox[0..5]; zeroes the error word
__global__ __launch_bounds__(64) void fuse_bbox_final_kernel(const double *__restrict__ part, int rows, double *__restrict__ bbox, int32_t *__restrict__ err)
{
    const int lane = lane_id();
    double v[6] = { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY };
    for (int r = lane; r < rows; r += 64) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { v[a] = fmin(v[a], part[(int64_t)r * 6 + a]); v[3 + a] = fmax(v[3 + a], part[(int64_t)r * 6 + 3 + a]); }
    }
    box_wave_fold(v, v + 3);
    if (lane == 0) {
        for (int a = 0; a < 6; ++a) bbox[a] = v[a];
        *err = 0;
    }
}
// The fused cloud's keys as 32-bit mixed-radix words (ix DY + iy) DZ + iz over the grid's own extent -- the SAME order (ascending ix, iy, iz)
// in as few bits as the fused cloud needs (a person at 10 mm voxels: ~23), for the library's own radix sort: three 8-bit passes of two
// launches each where the vendor's merge sort of the 63-bit keys took seven launches with host work between them (~150 us of a frame
// under load, profiles/r05/overlap_timeline_native_stream.txt).  The width this cloud needs (> 32: the keys written are useless and
// the caller takes the 63-bit path):
__device__ __forceinline__ int fuse_key_bits(const double *__restrict__ bbox, double voxel, double d[3], bool *sane_out)
{
    (void)voxel_cell(bbox + 3, bbox, voxel, d);      // the cell of the box's far corner
#pragma unroll
    for (int a = 0; a < 3; ++a) d[a] += 1.0;
    const bool sane = d[0] >= 1.0 && d[1] >= 1.0 && d[2] >= 1.0 && d[0] < kVoxelAxisCells && d[1] < kVoxelAxisCells && d[2] < kVoxelAxisCells;      // (NaN / empty boxes: not sane)
    int bits = 64;
    if (sane && d[0] * d[1] * d[2] < 18446744073709551616.0) {
        const unsigned long long range = (unsigned long long)d[0] * (unsigned long long)d[1] * (unsigned long long)d[2];
        bits = 1;
        while (bits < 64 && (range >> bits) != 0ull) ++bits;
    }
    *sane_out = sane;
    return bits;
}
__global__ void fuse_bits_kernel(const double *__restrict__ bbox, double voxel, int32_t *__restrict__ bits_out)
{
    double d[3];
    bool sane;
    *bits_out = fuse_key_bits(bbox, voxel, d, &sane);
}
// an index outside the grid's own extent becomes cell 0 and raises nothing: that happens only with *bits_out = 64, and the caller redoes
struct ExtentKeys32 {
    struct Grid {
        double d[3];
        unsigned long long DY, DZ;
    };
    uint32_t *keys;
    int32_t *bits_out;
    template <class Set> __device__ __forceinline__ Grid grid(const Set &, const double *__restrict__ bbox, double voxel) const
    {
        Grid g;
        bool sane;
        const int bits = fuse_key_bits(bbox, voxel, g.d, &sane);
        if (blockIdx.x == 0 && threadIdx.x == 0) *bits_out = bits;
        g.DY = sane ? (unsigned long long)g.d[1] : 1ull;
        g.DZ = sane ? (unsigned long long)g.d[2] : 1ull;
        return g;
    }
    __device__ __forceinline__ void put(const Grid &g, const double *__restrict__ bbox, double voxel, int64_t i, int, const double q[3]) const
    {
        double f[3];
        if (voxel_cell(q, bbox, voxel, f, g.d)) f[0] = f[1] = f[2] = 0.0;
        keys[i] = (uint32_t)(((unsigned long long)f[0] * g.DY + (unsigned long long)f[1]) * g.DZ + (unsigned long long)f[2]);
    }
};
// the moved point with concatenated index p and its colour (0 where its cloud has none)
struct MovedLoad {
    using Coord = double;
    const FuseBatch &b;
    __device__ __forceinline__ bool has_col() const { return true; }
    __device__ __forceinline__ void operator()(int64_t p, double v[3], float c[3], float *) const
    {
        const int cl = b.cloud_of(p);
        const int64_t j = p - b.off[cl];
        MovedPoint()(b, cl, j, v);
        const float *col = b.col[cl];
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = col ? col[3 * j + a] : 0.0f;
    }
};
__global__ __launch_bounds__(256) void fuse_mean_kernel(FuseBatch b, const int32_t *__restrict__ vals, const int32_t *__restrict__ seg_start,
                                                        int32_t *__restrict__ d_count, const int32_t *__restrict__ err, float *__restrict__ opts,
                                                        float *__restrict__ ocol)
{
    const int32_t m_total = *d_count;
    if (blockIdx.x == 0 && threadIdx.x == 0 && *err) *d_count = KPX_ERR_RANGE;      // as voxel_mean_kernel
    const int64_t total = b.off[b.count];
    for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < m_total; m += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s0 = seg_start[m], s1 = (m + 1 < m_total) ? seg_start[m + 1] : total;
        double sp[3] = { 0, 0, 0 }, sc[3] = { 0, 0, 0 }, sn[3];
        voxel_segment_sum<false>(vals, s0, s1, MovedLoad{ b }, sp, sc, sn);
        voxel_write_row(sp, sc, (double)(s1 - s0), opts + 3 * m, ocol ? ocol + 3 * m : nullptr);
    }
}
// spec_bits > 0 (frame loop): the fused cloud's keys are taken to fit `spec_bits` <= 32 bits -- the width its slot's previous frame
// needed -- and sorted as 32-bit words by the library's own radix sort; *d_bits (pinned host memory, written by the key kernel) receives
// the width this frame really needs, and the caller repeats the call with spec_bits = 0 when that is larger (the outputs of the
// speculative call are then garbage).  spec_bits = 0: 63-bit keys and the vendor sort, as exported.
static int fuse_voxel_impl(const FuseBatch &b, double voxel, float *opts, float *ocol, int32_t *d_count, Arena &a, hipStream_t st, int spec_bits = 0,
                           int32_t *d_bits = nullptr)
{
    const int64_t total = b.off[b.count];
    VoxelScratch s;
    voxel_carve(a, total, kFuseCarve, &s);
    KPX_ARENA_CHECK(a);
    hipLaunchKernelGGL((cloud_bbox_partial_kernel<FuseBatch, MovedPoint, double, kFuseBboxBlocks>), dim3(kFuseBboxBlocks, b.count), dim3(256), 0, st, b, s.part);
    hipLaunchKernelGGL(fuse_bbox_final_kernel, dim3(1), dim3(64), 0, st, s.part, b.count * kFuseBboxBlocks, s.bbox, s.err);
    const int nb = (int)(cdiv(total, 256) > 4096 ? 4096 : cdiv(total, 256));
    int rc;
    if (spec_bits > 0 && spec_bits <= 32 && d_bits && total <= kRadixMaxPairs) {
        hipLaunchKernelGGL((voxel_key_kernel<FuseBatch, MovedPoint, ExtentKeys32>), dim3(nb), dim3(256), 0, st, b, (const double *)s.bbox, voxel,
                           ExtentKeys32{ reinterpret_cast<uint32_t *>(s.sort.keys_in), d_bits }, s.sort.vals_in);
        rc = voxel_sort_and_heads<uint32_t>(s, total, spec_bits, d_count, st);
    } else {
        if (d_bits) hipLaunchKernelGGL(fuse_bits_kernel, dim3(1), dim3(1), 0, st, s.bbox, voxel, d_bits);      // for the caller's next speculation
        hipLaunchKernelGGL((voxel_key_kernel<FuseBatch, MovedPoint, FixedKeys>), dim3(nb), dim3(256), 0, st, b, (const double *)s.bbox, voxel,
                           FixedKeys{ s.sort.keys_in, s.err }, s.sort.vals_in);
        rc = voxel_sort_and_heads<uint64_t>(s, total, 63, d_count, st);
    }
    if (rc) return rc;
    hipLaunchKernelGGL(fuse_mean_kernel, dim3(nb), dim3(256), 0, st, b, s.sort.vals_out, s.seg_start, d_count, s.err, opts, ocol);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}
}  // namespace kpx

using namespace kpx;

KPX_EXPORT size_t kpx_fuse_voxel_workspace_bytes(int64_t total)
{
    Arena a(nullptr, 0);
    VoxelScratch s;
    voxel_carve(a, total, kFuseCarve, &s);
    return a.off;
}
KPX_EXPORT int kpx_fuse_voxel_downsample(int32_t count, const float *const *h_pts, const float *const *h_col, const int64_t *h_n,
                                         const double *h_T, double voxel, float *opts, float *ocol, int32_t *d_count, void *ws,
                                         size_t ws_bytes, void *stream)
{
    return kpx::fuse_voxel_downsample_dev(count, h_pts, h_col, h_n, h_T, nullptr, voxel, opts, ocol, d_count, ws, ws_bytes, stream, 0, nullptr);
}
int kpx::fuse_voxel_downsample_dev(int32_t count, const float *const *h_pts, const float *const *h_col, const int64_t *h_n, const double *h_T,
                                   const double *const *h_dT, double voxel, float *opts, float *ocol, int32_t *d_count, void *ws, size_t ws_bytes,
                                   void *stream, int spec_bits, int32_t *d_bits)
{
    KPX_REQUIRE(voxel > 0.0, "voxel_size <= 0");
    KPX_REQUIRE(count >= 1 && count <= kFuseMax, "kpx_fuse_voxel_downsample: 1 .. %d clouds", kFuseMax);
    KPX_REQUIRE(h_pts && h_n && h_T && d_count && ws, "kpx_fuse_voxel_downsample: null pointer");
    hipStream_t st = (hipStream_t)stream;
    FuseBatch b;
    b.count = count;
    b.off[0] = 0;
    bool any_col = false, all_col = true;
    for (int i = 0; i < kFuseMax; ++i) {
        const bool on = i < count;
        if (on) {
            KPX_REQUIRE(h_n[i] >= 0 && (h_n[i] == 0 || h_pts[i]), "kpx_fuse_voxel_downsample: bad cloud %d", i);
            if (h_n[i] > 0) { const bool hc = h_col && h_col[i]; any_col |= hc; all_col &= hc; }
        }
        b.pts[i] = on ? h_pts[i] : nullptr;
        b.col[i] = (on && h_col) ? h_col[i] : nullptr;
        b.off[i + 1] = b.off[i] + (on ? h_n[i] : 0);
        for (int k = 0; k < 12; ++k) b.T[i][k] = on ? h_T[16 * i + k] : 0.0;
        b.dT[i] = (on && h_dT) ? h_dT[i] : nullptr;
    }
    const int64_t total = b.off[count];
    KPX_REQUIRE(total < ((int64_t)1 << 31), "kpx_fuse_voxel_downsample: bad size");
    // [O3D] operator+= keeps colours only when both clouds have them
    KPX_REQUIRE(!ocol || !any_col || all_col, "kpx_fuse_voxel_downsample: colours on some clouds only");
    if (total == 0) { KPX_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), st)); return KPX_OK; }
    KPX_REQUIRE(opts, "kpx_fuse_voxel_downsample: null pointer");
    Arena a(ws, ws_bytes);
    return fuse_voxel_impl(b, voxel, opts, (any_col && all_col) ? ocol : nullptr, d_count, a, st, spec_bits, d_bits);
}

KPX_EXPORT size_t kpx_voxel_workspace_bytes(int64_t n)
{
    return kpx_voxel_batch_workspace_bytes(1, &n);
}
KPX_EXPORT int kpx_voxel_downsample(const float *pts, const float *col, const float *nrm, int64_t n, double voxel,
                                    float *opts, float *ocol, float *onrm, int32_t *d_count, void *ws, size_t ws_bytes,
                                    void *stream)
{
    KPX_REQUIRE(voxel > 0.0, "voxel_size <= 0");                       // [O3D] raises here
    KPX_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "kpx_voxel_downsample: bad size");
    KPX_REQUIRE(d_count && ws, "kpx_voxel_downsample: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) { KPX_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), st)); return KPX_OK; }
    KPX_REQUIRE(pts && opts, "kpx_voxel_downsample: null pointer");
    Arena a(ws, ws_bytes);
    // Without normals a single cloud takes the one-pass batch form too (a batch of one): keys of <= 32 bits whenever the grid allows
    // (a 1M-point room at 10 mm needs 25), sorted by the library's own radix sort and the staged mean kernel -- the 63-bit key +
    // vendor-sort path below remains for clouds with normals.  KPX_VOXEL_SINGLE=0: A/B switch.
    static const bool single_batch = [] { const char *e = getenv("KPX_VOXEL_SINGLE"); return !(e && e[0] == '0'); }();
    if (!nrm && single_batch) {
        return voxel_batch_impl(voxel_batch_of(&pts, &col, &n, &opts, col ? &ocol : nullptr, 0, 1, false), voxel, d_count, a, st);
    }
    return voxel_impl(pts, col, nrm, n, voxel, opts, ocol, onrm, d_count, a, st);
}

KPX_EXPORT size_t kpx_voxel_batch_workspace_bytes(int32_t count, const int64_t *h_n)
{
    if (count < 1 || !h_n) return 0;
    Arena a(nullptr, 0), one(nullptr, 0);        // cloud by cloud on the lanes (plain form), or one pass
    VoxelScratch s;
    int64_t total = 0;
    for (int i = 0; i < count; ++i) {
        voxel_carve(a, h_n[i], kPlainCarve, &s);
        total += h_n[i] > 0 ? h_n[i] : 0;
    }
    voxel_carve(one, total, kBatchCarve, &s);
    return a.off > one.off ? a.off : one.off;
}
KPX_EXPORT int kpx_voxel_downsample_batch(int32_t count, const float *const *h_pts, const float *const *h_col, const int64_t *h_n,
                                          double voxel, float *const *h_opts, float *const *h_ocol, int32_t *d_counts, void *ws,
                                          size_t ws_bytes, void *stream)
{
    return kpx::voxel_downsample_batch_spec(count, h_pts, h_col, h_n, voxel, h_opts, h_ocol, d_counts, ws, ws_bytes, stream, 0, nullptr, false);
}
int kpx::voxel_downsample_batch_spec(int32_t count, const float *const *h_pts, const float *const *h_col, const int64_t *h_n, double voxel,
                                     float *const *h_opts, float *const *h_ocol, int32_t *d_counts, void *ws, size_t ws_bytes, void *stream,
                                     int spec_bits, int32_t *d_bits, bool morton)
{
    KPX_REQUIRE(voxel > 0.0, "voxel_size <= 0");
    KPX_REQUIRE(count >= 1 && count <= 64 && h_pts && h_n && h_opts && d_counts && ws, "kpx_voxel_downsample_batch: bad arguments");
    for (int i = 0; i < count; ++i)
        KPX_REQUIRE(h_n[i] >= 0 && h_n[i] < ((int64_t)1 << 31) && (h_n[i] == 0 || (h_pts[i] && h_opts[i])),
                    "kpx_voxel_downsample_batch: bad cloud %d", i);
    hipStream_t st = (hipStream_t)stream;
    int64_t total = 0;
    for (int i = 0; i < count; ++i) total += h_n[i];
    // (the curve order exists in the one-pass form only; the other forms keep the row-major order -- callers that asked for it only
    // lose locality, never correctness)
    if (count <= kVoxelBatchMax && total > 0 && total < ((int64_t)1 << 31)) {         // one pass over the concatenated clouds
        Arena one(ws, ws_bytes);
        return voxel_batch_impl(voxel_batch_of(h_pts, h_col, h_n, h_opts, h_ocol, 0, count, morton), voxel, d_counts, one, st, spec_bits, d_bits);
    }
    if (d_bits) KPX_HIP(hipMemsetAsync(d_bits, 0, sizeof(int32_t), st));         // the other forms do not speculate: width 0 = "fine"
    if (count > kVoxelBatchMax && total > 0) {
        // more clouds than one pass takes: groups of kVoxelBatchMax, one concatenated pass each, one after the other on `stream`
        // (64 clouds of 1M points: 11 ms cloud by cloud on the lanes -- every cloud its own 8-pass sort -- against eight 8M-key sorts)
        // groups of kVoxelBatchMax consecutive clouds.  (Groups capped at the library's own radix sort -- 4M pairs, four 1M-point
        // clouds -- were measured SLOWER than eight clouds per group on the vendor's Onesweep: 8.4 vs 7.1 ms for 64 x 1M points; at
        // 4M pairs the own sort's four 8-bit passes cost 31 + 9 us each, and half as many groups halve the per-group launches.)
        int gstart[65], ng = 0;
        bool ok = true;
        for (int i = 0; i < count;) {
            gstart[ng++] = i;
            int64_t gt = 0;
            int gc = 0;
            while (i < count && gc < kVoxelBatchMax) { gt += h_n[i]; ++gc; ++i; }
            ok = ok && gt < ((int64_t)1 << 31);
        }
        gstart[ng] = count;
        if (ok) {
            for (int g = 0; g < ng; ++g) {
                const int g0 = gstart[g], gc = gstart[g + 1] - g0;
                int64_t gt = 0;
                for (int i = 0; i < gc; ++i) gt += h_n[g0 + i];
                if (gt == 0) { KPX_HIP(hipMemsetAsync(d_counts + g0, 0, (size_t)gc * sizeof(int32_t), st)); continue; }
                Arena one(ws, ws_bytes);
                const int grc = voxel_batch_impl(voxel_batch_of(h_pts, h_col, h_n, h_opts, h_ocol, g0, gc, false), voxel, d_counts + g0, one, st);
                if (grc) return grc;
            }
            return KPX_OK;
        }
    }
    LaneSet *ln = nullptr;
    int rc = lanes_get(&ln);
    if (rc) return rc;
    const int used = count < kLaneCount ? count : kLaneCount;
    rc = lanes_fork(ln, st, used);
    if (rc) return rc;
    Arena a(ws, ws_bytes);
    for (int i = 0; i < count && !rc; ++i) {
        hipStream_t ls = ln->s[i % kLaneCount];
        if (h_n[i] == 0) { rc = hipMemsetAsync(d_counts + i, 0, sizeof(int32_t), ls) == hipSuccess ? KPX_OK : fail(KPX_ERR_HIP, "memset failed"); continue; }
        rc = voxel_impl(h_pts[i], h_col ? h_col[i] : nullptr, nullptr, h_n[i], voxel, h_opts[i], (h_col && h_ocol) ? h_ocol[i] : nullptr, nullptr,
                        d_counts + i, a, ls);
    }
    const int jrc = lanes_join(ln, st, used);
    return rc ? rc : jrc;
}
