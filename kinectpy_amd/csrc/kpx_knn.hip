// kpx_knn.hip -- exact neighbour searches on a uniform grid:
//   a8  PointCloud.remove_statistical_outlier (filtering.py:24, floor_removal.py:73, utils/processing.py:309)
//       estimate_normals(KDTreeSearchParamHybrid) (preprocessing/registration.py:9-13), estimate_covariances
// The grid build, SOR's block-per-64-queries pass 0 and statistics, and the operators SorOp and MomentsOp: what SOR and the normals do
// with a query's k nearest.  The search itself is shared (kpx_gridknn.h): knn_wave_kernel -- a wave per query selects the k smallest
// squared distances of the surrounding cell block in LDS -- and, for what does not fit its buffer, knn_heap_kernel -- one thread per
// query walks Chebyshev rings of cells and keeps the k smallest in a per-thread max-heap (layout [slot][thread]: bank-conflict free
// when the threads of a wave touch the same slot) -- run in that order by knn_cascade.  Both are exact: a search stops only once
// the k-th best distance is below the distance to the boundary of the covered cube.
// Squared distance (contract AC3): d2 = fma(dz,dz, fma(dy,dy, dx*dx)), differences in fp64.
#include <hipcub/hipcub.hpp>

#include "kpx_compact.h"
#include "kpx_gridknn.h"
#include "kpx_morton.h"
#include "kpx_linalg.h"

// candidates per query the group pass holds (kpx_gridknn.h, knn_group_pass; measured: profiles/r06/exp_knn_group.txt)
#ifndef KPX_KNN_GROUP_CAP_SOR
#define KPX_KNN_GROUP_CAP_SOR 256
#endif
#ifndef KPX_KNN_GROUP_CAP_NORMALS
#define KPX_KNN_GROUP_CAP_NORMALS 192
#endif

namespace kpx {

// ---- grid construction ------------------------------------------------------------------------------
// Cell size of the grid: from the bounding box (volume and area heuristics), then -- refine -- corrected once by the occupancy an
// average POINT saw in the first binning (sum c^2 / n: isolated outliers each own a cell and would drag a per-cell mean down);
// occupancy ~ h^2.3 for surfaces with some thickness.  Pure function of (bbox, n, target, cell_cap, sumsq): every block of the
// binning kernel evaluates it for itself (no parameter kernel in front of it), block 0 stores the result for the later kernels.
__device__ __forceinline__ void grid_dims(const double ext[3], double &h, int32_t cell_cap, int dim[3])
{
    for (;;) {
        double tot = 1.0;
        for (int a = 0; a < 3; ++a) {
            double d = floor(ext[a] / h) + 1.0;
            if (d > 1000000.0) d = 1000000.0;
            dim[a] = (int)d; tot *= d;
        }
        if (tot <= (double)cell_cap) break;
        h *= 1.26;
    }
}
// fixed_h > 0: the caller's cell size instead (ISS: half its larger radius), never below the heuristic's cell of `target` points (a
// radius under the point spacing would ask for more cells than there are points) and without the occupancy feedback.
__device__ __forceinline__ GridParams grid_params_of(const double *__restrict__ bbox, int64_t n, double target, int32_t cell_cap,
                                                     const unsigned long long *__restrict__ sumsq, double fixed_h)
{
    GridParams gp;
    double ext[3], vol = 1.0;
    for (int a = 0; a < 3; ++a) { ext[a] = bbox[3 + a] - bbox[a]; if (!(ext[a] > 1e-9)) ext[a] = 1e-9; vol *= ext[a]; }
    const double nn = (double)(n > 0 ? n : 1);
    const double h3 = cbrt(vol * target / nn);
    const double area = ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2];
    const double h2 = sqrt(area * target / nn) * 0.5;           // clouds are surfaces: size cells by area too
    double h = h3 > h2 ? h3 : h2;
    if (!(h > 0.0)) h = 1.0;
    if (fixed_h > h) h = fixed_h;
    int dim[3];
    grid_dims(ext, h, cell_cap, dim);
    if (sumsq && !(fixed_h > 0.0)) {
        const double occ = (double)*sumsq / nn;
        double f = pow(target / (occ > 1.0 ? occ : 1.0), 1.0 / 2.3);
        f = f < 0.125 ? 0.125 : (f > 8.0 ? 8.0 : f);
        h *= f;
        grid_dims(ext, h, cell_cap, dim);
    }
    gp.h = h;
    for (int a = 0; a < 3; ++a) { gp.org[a] = bbox[a]; gp.dim[a] = dim[a]; }
    gp.ncell = dim[0] * dim[1] * dim[2];
    return gp;
}
__global__ __launch_bounds__(256) void grid_occupancy_kernel(const uint32_t *__restrict__ cell_count, const GridParams *__restrict__ gp,
                                                             unsigned long long *__restrict__ sumsq)
{
    __shared__ unsigned long long sh[4];
    const int ncell = gp->ncell;
    unsigned long long c = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ncell; i += gridDim.x * blockDim.x) {
        unsigned long long v = cell_count[i];
        c += v * v;
    }
    c = block_sum(c, sh);
    if (threadIdx.x == 0 && c) atomicAdd(sumsq, c);
}
__global__ __launch_bounds__(256) void grid_cell_kernel(const float *__restrict__ pts, int64_t n, const double *__restrict__ bbox, double target,
                                                        int32_t cell_cap, const unsigned long long *__restrict__ sumsq, GridParams *gp,
                                                        uint32_t *__restrict__ keys, int32_t *__restrict__ vals, uint32_t *__restrict__ cell_count,
                                                        double fixed_h)
{
    __shared__ GridParams sg;
    if (threadIdx.x == 0) {
        sg = grid_params_of(bbox, n, target, cell_cap, sumsq, fixed_h);
        if (blockIdx.x == 0) *gp = sg;
    }
    __syncthreads();
    const GridParams g = sg;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int cx = cell_coord(pts[3 * i], g.org[0], g.h, g.dim[0]);
        int cy = cell_coord(pts[3 * i + 1], g.org[1], g.h, g.dim[1]);
        int cz = cell_coord(pts[3 * i + 2], g.org[2], g.h, g.dim[2]);
        uint32_t cell = (uint32_t)((cx * g.dim[1] + cy) * g.dim[2] + cz);
        keys[i] = cell;
        vals[i] = (int32_t)i;
        atomicAdd(&cell_count[cell], 1u);
    }
}
__global__ __launch_bounds__(256) void grid_gather_kernel(const float *__restrict__ pts, int64_t n, const int32_t *__restrict__ order,
                                                          float *__restrict__ sorted_pts)
{
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        int64_t i = order[s];
        sorted_pts[3 * s] = pts[3 * i]; sorted_pts[3 * s + 1] = pts[3 * i + 1]; sorted_pts[3 * s + 2] = pts[3 * i + 2];
    }
}
// Cell order without a radix sort (a sort of 30k keys is 9-13 launches; this is 2): every point takes the next free slot of its
// cell's range (atomic cursor: the order inside a cell is whatever the hardware made it) ...
__global__ __launch_bounds__(256) void grid_place_kernel(const uint32_t *__restrict__ cell_of, int64_t n, const uint32_t *__restrict__ cell_start,
                                                         uint32_t *__restrict__ cursor, int32_t *__restrict__ slot_idx)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t c = cell_of[i];
        slot_idx[cell_start[c] + atomicAdd(&cursor[c], 1u)] = (int32_t)i;
    }
}
// ... and one thread per point then finds its rank among the points of its cell (how many of them have a lower index: the
// cell's range is a handful of entries, read by neighbouring threads together) and moves itself there: ascending point index
// inside every cell, i.e. exactly the order a stable sort by cell gives -- deterministic, identical to the sorted build.
__global__ __launch_bounds__(256) void grid_rank_kernel(const float *__restrict__ pts, int64_t n, const uint32_t *__restrict__ cell_of,
                                                        const uint32_t *__restrict__ cell_start, const int32_t *__restrict__ slot_idx,
                                                        int32_t *__restrict__ sorted_idx, float *__restrict__ sorted_pts)
{
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        const int32_t i = slot_idx[s];
        const uint32_t c = cell_of[i];
        const int64_t s0 = cell_start[c], s1 = cell_start[c + 1];
        int rank = 0;
        for (int64_t t = s0; t < s1; ++t) rank += slot_idx[t] < i ? 1 : 0;
        const int64_t d = s0 + rank;
        sorted_idx[d] = i;
        sorted_pts[3 * d] = pts[3 * (int64_t)i]; sorted_pts[3 * d + 1] = pts[3 * (int64_t)i + 1]; sorted_pts[3 * d + 2] = pts[3 * (int64_t)i + 2];
    }
}

// Exclusive prefix sums of the cell counts in ONE launch (decoupled look-back over tiles of 2048 counters, kpx_compact.h) instead of
// the vendor scan's two launches and its host-side set-up: with four frames in flight the frame's stream sat idle 50-65 us in front
// of that scan (profiles/r05/overlap_timeline_native_stream.txt).  states: one cleared 64-bit word per tile.
constexpr int kGridScanItems = 8, kGridScanTile = 256 * kGridScanItems;
constexpr int kGridScanWords = 2 * ((kGridMaxCells + 1 + kGridScanTile - 1) / kGridScanTile) + 2;
__global__ __launch_bounds__(256) void grid_scan_kernel(const uint32_t *__restrict__ counts, int64_t len, uint32_t *__restrict__ out,
                                                        unsigned long long *__restrict__ states)
{
    __shared__ int sh[256 / 64 + 2];
    const int64_t base = (int64_t)blockIdx.x * kGridScanTile + (int64_t)threadIdx.x * kGridScanItems;
    uint32_t v[kGridScanItems];
    int c = 0;
#pragma unroll
    for (int k = 0; k < kGridScanItems; ++k) { v[k] = base + k < len ? counts[base + k] : 0u; c += (int)v[k]; }
    int tot;
    const int ex = block_excl_scan(c, sh, &tot);
    __syncthreads();
    const int before = lookback_exclusive(states, blockIdx.x, tot, sh + 256 / 64 + 1);
    uint32_t run = (uint32_t)(before + ex);
#pragma unroll
    for (int k = 0; k < kGridScanItems; ++k) {
        if (base + k < len) out[base + k] = run;
        run += v[k];
    }
}

int grid_build(const float *pts, int64_t n, double target_per_cell, Arena &a, Grid *g, hipStream_t st, double fixed_h)
{
    const size_t nn = (size_t)(n > 0 ? n : 1);
    g->params = a.get<GridParams>(1);
    // ONE cleared region per build: [16 spare words for the caller's counters | sum of squares | counts of the first binning |
    // counts of the definitive binning] (each binning has its own counters so that nothing is cleared in between)
    uint32_t *zero = a.get<uint32_t>(3 * ((size_t)kGridMaxCells + 1) + 32 + kGridExtraWords + kGridScanWords);
    g->cell_start = a.get<uint32_t>((size_t)kGridMaxCells + 1);
    g->sorted_pts = a.get<float>(nn * 3);
    g->sorted_idx = a.get<int32_t>(nn);
    double *part = a.get<double>((size_t)kBboxBlocks * 6 + 8);
    // the sort build's (cell, point) pairs; the vendor scan of KPX_GRID_SCAN=0 runs in the sort's temporary buffer.  The own radix
    // sort's scratch is carved for every size (capped at the sort's limit): the workspace a caller sized for a worst-case count then
    // also holds any smaller cloud's build -- bytes(n) is monotonic (kpx_frame_step sizes one scratch region from the worst case)
    size_t scan_bytes = memo_bytes(kMemoGridScan, kGridMaxCells + 1, [&] { size_t b = 0; (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, zero, g->cell_start, kGridMaxCells + 1, st); return b; });
    DeviceSort<uint32_t> sort;
    SortOptions o;
    o.vals_out = false;
    o.radix = kRadixAndVendor;
    o.tmp_floor = scan_bytes;
    dsort_carve(a, n, 22, o, &sort);
    sort.vals_out = g->sorted_idx;
    g->sorted_keys = sort.keys_out;
    if (a.dry) return KPX_OK;
    KPX_ARENA_CHECK(a);
    double *bbox = part + (size_t)kBboxBlocks * 6;
    int rc = bbox_f32(pts, n, bbox, part, st);
    if (rc) return rc;
    // The counters and the scan cover every cell the grid may have.  Small clouds get a smaller ceiling than the 4M the
    // workspace holds (16 cells per point, at least 64k): clearing and scanning 16 MB twice per build cost ~50 us, more than
    // the neighbour search of a 30k-point cloud; a grid that would need more cells just gets coarser (results do not depend on h).
    int32_t cell_cap = 65536;
    while (cell_cap < kGridMaxCells && (int64_t)cell_cap < 16 * n) cell_cap <<= 1;
    g->spare = reinterpret_cast<int32_t *>(zero);
    unsigned long long *sumsq = reinterpret_cast<unsigned long long *>(zero + 16);
    g->extra = reinterpret_cast<int32_t *>(zero + 32);
    unsigned long long *scan_states = reinterpret_cast<unsigned long long *>(zero + 32 + kGridExtraWords);
    uint32_t *count1 = zero + 32 + kGridExtraWords + kGridScanWords, *count2 = count1 + (size_t)cell_cap + 1, *cursor = count2 + (size_t)cell_cap + 1;
    KPX_HIP(hipMemsetAsync(zero, 0, (32 + kGridExtraWords + kGridScanWords + 3 * ((size_t)cell_cap + 1)) * sizeof(uint32_t), st));
    int nb = (int)(cdiv(n, 256) > 4096 ? 4096 : cdiv(n, 256));
    // first binning from the bounding-box heuristic, one round of occupancy feedback, then the definitive binning
    hipLaunchKernelGGL(grid_cell_kernel, dim3(nb), dim3(256), 0, st, pts, n, bbox, target_per_cell, cell_cap, (const unsigned long long *)nullptr, g->params,
                       sort.keys_in, sort.vals_in, count1, fixed_h);
    hipLaunchKernelGGL(grid_occupancy_kernel, dim3(1024), dim3(256), 0, st, count1, g->params, sumsq);
    hipLaunchKernelGGL(grid_cell_kernel, dim3(nb), dim3(256), 0, st, pts, n, bbox, target_per_cell, cell_cap, (const unsigned long long *)sumsq, g->params,
                       sort.keys_in, sort.vals_in, count2, fixed_h);
    static const bool vendor_scan = [] { const char *e = getenv("KPX_GRID_SCAN"); return e && e[0] == '0'; }();      // A/B switch
    if (vendor_scan) KPX_HIP(hipcub::DeviceScan::ExclusiveSum(sort.tmp, scan_bytes, count2, g->cell_start, cell_cap + 1, st));
    else
        hipLaunchKernelGGL(grid_scan_kernel, dim3((unsigned)cdiv((int64_t)cell_cap + 1, kGridScanTile)), dim3(256), 0, st, count2, (int64_t)cell_cap + 1, g->cell_start,
                           scan_states);
    // The rank pass reads a cell's whole range per point: quadratic in the cell's population.  Cells are sized for 6-96 points, but
    // exact duplicates cannot be split by any grid, so the counting build is kept to frame-sized clouds (where the launch count is
    // what matters and an all-duplicates input costs at most 65536^2 range reads, ~1 s); larger clouds take the radix sort, whose
    // cost does not depend on the data.  KPX_GRID_SORT=1 forces the sort (A/B runs).
    static const bool force_sort = [] { const char *e = getenv("KPX_GRID_SORT"); return e && e[0] == '1'; }();
    const bool by_sort = force_sort || n > 65536;
    if (by_sort) {
        rc = dsort_run(sort, n, 22, st);
        if (rc) return rc;
        hipLaunchKernelGGL(grid_gather_kernel, dim3(nb), dim3(256), 0, st, pts, n, g->sorted_idx, g->sorted_pts);
    } else {
        hipLaunchKernelGGL(grid_place_kernel, dim3(nb), dim3(256), 0, st, sort.keys_in, n, g->cell_start, cursor, sort.vals_in);
        hipLaunchKernelGGL(grid_rank_kernel, dim3(nb), dim3(256), 0, st, pts, n, sort.keys_in, g->cell_start, sort.vals_in, g->sorted_idx, g->sorted_pts);
    }
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

// ---- a8 SOR ------------------------------------------------------------------------------------------
// The mean distance to the k nearest, as an operator of knn_wave_kernel / knn_heap_kernel (kpx_gridknn.h).  The mean needs no
// identities: sum of sqrt over the selected set, ties at the k-th value counted k - (#smaller) times.
// queries = the cell-sorted positions [q0, q1) (all of them: 0, n; a slab of the grid order for kpx_sor_partial).
// sidx != NULL: avg is indexed by the caller's point index; sidx == NULL: by sorted position relative to q0.
struct SorOp {
    static constexpr bool kPos = false;
    static constexpr int kGroupWavesPerSimd = 5, kGroupTrips = 2; // knn_group_kernel: a register budget of 96, trips of 16 candidates fetched together
    using Heap = HeapD;
    const int32_t *sidx;
    int64_t q0;
    double *avg;
    __device__ double r2max(bool heap_walk) const { return heap_walk ? -1.0 : INFINITY; }      // plain kNN
    __device__ void defer(int64_t) const {}
    __device__ void wave(const WaveKnnScratch &sc, const WaveKnnResult &res, int64_t s, const float *) const
    {
        const int lane = threadIdx.x & 63;
        // The roots, ONE fp64 sqrt sequence per 64 selected candidates instead of one per 64 gathered (a chunk of the buffer holds a
        // handful of selected values, and the sequence ran for each chunk under a divergent test): a ballot per chunk lists the selected
        // positions, lanes 0 .. n-1 take the roots of up to 64 listed positions and store them back NEGATED -- the sign marks a
        // candidate as selected for the sum below (d^2 = 0 gives -0).  Nothing reads the distances after this operator.
        int32_t *list = sc.run_off;                                  // free once the gather is over
        int listed = 0;                                              // wave-uniform
        auto roots = [&](int n) {
            wave_lds_fence();
            if (lane < n) { const int t = list[lane]; sc.vals[t] = -sqrt(sc.vals[t]); }
            wave_lds_fence();
        };
        for (int t0 = 0; t0 < res.m; t0 += 64) {
            const int t = t0 + lane;
            const bool sel = t < res.m && (unsigned long long)__double_as_longlong(sc.vals[t]) <= res.thr;
            const unsigned long long bm = __builtin_amdgcn_ballot_w64(sel);
            const int n = __builtin_popcountll(bm);
            if (listed + n > 64) { roots(listed); listed = 0; }
            if (sel) list[listed + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bm, 0u))] = t;
            listed += n;
        }
        roots(listed);
        // the sum in the order it always had: lane l adds its candidates l, l + 64, ... in turn, then the wave's tree
        double sum = 0.0;
        for (int t = lane; t < res.m; t += 64) {
            const double v = sc.vals[t];
            if (__double_as_longlong(v) < 0) sum += -v;
        }
        sum = wave_sum_down_f64(sum);                                // lane 0
        const double total = sum - (double)(res.cnt - res.kk) * sqrt(res.top);      // ties beyond the k-th slot
        if (lane == 0) avg[sidx ? (int64_t)sidx[s] : s - q0] = res.kk > 0 ? total / (double)res.kk : -1.0;
    }
    // the group form (knn_group_kernel): a query per row of 16 lanes, exactly kk selected (no ties beyond the k-th slot)
    __device__ void row(const RowKnnResult &res, int64_t s, const float *) const
    {
        const int j = threadIdx.x & 15, row = (threadIdx.x & 63) >> 4;
        const uint32_t *w32 = reinterpret_cast<const uint32_t *>(res.vals);
        // the roots as in wave(): the selected positions are listed by ballot (kk <= k of them), lanes take the roots of 16 listed
        // positions at a time and store them back negated
        int listed = 0;                                              // the same in all lanes of the row
        for (int u = 0; u < res.trips16; ++u) {
            const int t = 16 * u + j;
            const bool sel = t < res.m && w32[2 * t + 1] <= res.hi_thr;
            const unsigned bits = (unsigned)(__builtin_amdgcn_ballot_w64(sel) >> (16 * row)) & 0xFFFFu;
            const int at = listed + __builtin_popcount(bits & ((1u << j) - 1u));
            if (sel && at < kKnnRowBuckets / 4) res.list[at] = (uint32_t)t;
            listed += __builtin_popcount(bits);
        }
        wave_lds_fence();
        for (int i0 = 0; i0 < res.k; i0 += 16) {
            const int i = i0 + j;
            if (i < listed) { const int t = (int)res.list[i]; res.vals[t] = -sqrt(res.vals[t]); }
        }
        wave_lds_fence();
        // wave() has lane l add its candidates l, l + 64, ... in turn: accumulator a[q] of lane j is lane j + 16 q of that wave
        double a[4] = { 0.0, 0.0, 0.0, 0.0 };
        for (int u0 = 0; u0 < res.trips16; u0 += 4) {
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                const int t = 16 * (u0 + qd) + j;
                if (t < res.m) { const double v = res.vals[t]; if (__double_as_longlong(v) < 0) a[qd] += -v; }
            }
        }
        const double sum = row_sum_down_f64((a[0] + a[2]) + (a[1] + a[3]));      // steps 32 and 16 of wave_sum_down_f64, then the row's
        if (res.store && j == 0) avg[sidx ? (int64_t)sidx[s] : s - q0] = res.kk > 0 ? sum / (double)res.kk : -1.0;
    }
    __device__ void heap(int64_t s, const HeapD &heap) const
    {
        double sum = 0.0;
        for (int e = 0; e < heap.sz; ++e) sum += sqrt(heap.h[e * heap.stride]);
        avg[sidx ? (int64_t)sidx[s] : s - q0] = heap.sz > 0 ? sum / (double)heap.sz : -1.0;
    }
};

// ---- a8 SOR, the queries of a cell together: a BLOCK per 64 cell-sorted queries ----------------------------------------------------------
// The wave-per-query kernel above re-gathers the 27-cell block for every query -- binary search over the cell runs, loads, 64-lane
// ballots per selection step -- although the queries of a cell share that block.  Here a block takes 64 consecutive cell-sorted queries,
// stages the 27-cell block of each CELL among them ONCE with all 256 threads -- nine contiguous runs of the cell-sorted points, one per
// (x, y) column; the run of a point by a fixed-depth search, so that the loads of a thread's eight points are in flight together -- and its
// four waves answer the cell's queries side by side -- wave w the w-th, (w + 4)-th, ... -- each from the two words of the S squared
// distances a lane holds in REGISTERS (lane l: candidates l, l + 64, ...; AC3, fp64; d^2 >= 0, so the IEEE patterns order like the
// values).  The k-th smallest high word is found by counting into 256 LDS buckets (the window starts at the smallest NON-ZERO high word
// and ends at the cover's; a level ends the search when the k-th is the last of its bucket or the bucket is one value wide), the low
// words are looked at only when several candidates share the k-th high word (bisection).  The selected patterns go into the wave's
// selection buffer in the block's own order (a ballot per row of 64 candidates places them) and the sum of their square roots is a fixed
// tree; ties at the k-th value are counted k - (#smaller) times, as in the wave-per-query kernel.
// Exactness is the ring walk's rule: a query is answered here only if its k-th candidate lies inside the distance the staged block covers
// (block_cover2).  Queries the 3 x 3 x 3 block does not cover get the 5 x 5 x 5 block the same way; everything else -- blocks that do not
// cover, blocks with more than 64 x S points, more than kSorTieRoom ties beyond k -- goes to the wave-per-query passes through a list.
// The staged block, its order (column by column, cell-sorted position inside a column) and with it every sum depend on the query's CELL
// alone, not on how the queries were dealt out: the slab calls of the sharded filter (kpx_sor_partial) give bitwise the values of the
// one-GPU call.
// 36 KB of LDS per block at k = 200 (filter_outliers' default, preprocessing/data.py:61): sixteen waves per CU.  Roof: per query 6 x 64 S
// fp64 flops for the distances and a few 32-bit operations per candidate and counting level -- vector ALU work on LDS-resident operands
// (12 B per candidate, staged once per cell); DESIGN.md section 5.3 has the numbers, also against the wave-per-16-queries form this
// kernel replaced.
// The whole-wave reductions, the scan and the broadcasts are those of kpx_wave.h (result the same in every lane).
__device__ __forceinline__ int wave_sum_i(int v) { return wave_sum_i32(v); }
__device__ __forceinline__ unsigned wave_min_u(unsigned v) { return wave_min_u32(v); }
__device__ __forceinline__ unsigned wave_max_u(unsigned v) { return wave_max_u32(v); }
constexpr int kSorBuckets = 256;              // buckets of the counting selection
constexpr int kSorTieRoom = 32;               // candidates tied with the k-th beyond k the selection buffer still holds
constexpr int kBlkQueries = 64, kBlkWaves = 4;
#ifndef KPX_SOR_BLOCK_MINB
#define KPX_SOR_BLOCK_MINB 4
#endif
template <int S>
__global__ __launch_bounds__(64 * kBlkWaves, KPX_SOR_BLOCK_MINB) void sor_block_kernel(
    const GridParams *__restrict__ gp, const uint32_t *__restrict__ cell_start, const float *__restrict__ spts, const int32_t *__restrict__ sidx,
    int64_t q0, int64_t q1, int k, int kbuf, double *__restrict__ avg, int32_t *__restrict__ fb_list, int32_t *__restrict__ fb_count)
{
    constexpr int CAP = 64 * S, W = kBlkWaves, T = 64 * kBlkWaves;
    extern __shared__ __align__(16) double lds[];
    __shared__ uint32_t run_s0[32];
    __shared__ int32_t run_off[32];
    __shared__ float qf[3][kBlkQueries];
    __shared__ int32_t qc[3][kBlkQueries];
    __shared__ int32_t qcell[kBlkQueries], qsidx[kBlkQueries];
    __shared__ uint8_t qstate[kBlkQueries];              // 0 open, 1 settled, 2 ties beyond the buffer (straight to the list)
    __shared__ int32_t s_m;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float *cand = reinterpret_cast<float *>(lds);                                                   // CAP x 3 floats
    uint32_t *hist = reinterpret_cast<uint32_t *>(lds + (size_t)(CAP * 3) / 2) + (size_t)wave * kSorBuckets;
    double *selbuf = lds + (size_t)(CAP * 3) / 2 + (size_t)W * kSorBuckets / 2 + (size_t)wave * kbuf;
    const GridParams g = *gp;
    const int64_t nq = q1 - q0;
    for (int64_t chunk = blockIdx.x; chunk * kBlkQueries < nq; chunk += gridDim.x) {
        const int64_t base = q0 + chunk * kBlkQueries;
        const int nqc = (int)(q1 - base < kBlkQueries ? q1 - base : kBlkQueries);
        if (tid < nqc) {
            const float *qp = spts + 3 * (base + tid);
            int c[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) { const float v = qp[a]; qf[a][tid] = v; c[a] = cell_coord((double)v, g.org[a], g.h, g.dim[a]); qc[a][tid] = c[a]; }
            qcell[tid] = (int32_t)(((int64_t)c[0] * g.dim[1] + c[1]) * g.dim[2] + c[2]);
            qsidx[tid] = sidx ? sidx[base + tid] : (int32_t)(base + tid - q0);
            qstate[tid] = 0;
        }
        __syncthreads();
        // the chunk's cells: a cell's queries are contiguous (cell-sorted); every wave derives the same mask
        const int mycell = lane < nqc ? qcell[lane] : -1;
        const int prevcell = __shfl_up(mycell, 1, 64);
        unsigned long long segs = __builtin_amdgcn_ballot_w64(lane < nqc && (lane == 0 || mycell != prevcell));
        while (segs != 0ull) {
            const int pos = __builtin_ctzll(segs);
            segs &= segs - 1ull;
            const int len = (segs ? __builtin_ctzll(segs) : nqc) - pos;
            const int cx = qc[0][pos], cy = qc[1][pos], cz = qc[2][pos];
            for (int rad = 1; rad <= 2; ++rad) {
                if (rad == 2 && __builtin_amdgcn_ballot_w64(lane < len && qstate[pos + lane] == 0) == 0ull) break;       // block-uniform: qstate is settled
                const int side = 2 * rad + 1, nruns = side * side;
                if (wave == 0) {                                 // the block's runs, one per (x, y) column, ascending
                    uint32_t s0 = 0u;
                    int ln = 0;
                    if (lane < nruns) {
                        const int x = cx + lane / side - rad, y = cy + lane % side - rad;
                        if (x >= 0 && x < g.dim[0] && y >= 0 && y < g.dim[1]) {
                            const int64_t col = ((int64_t)x * g.dim[1] + y) * g.dim[2];
                            const int za = cz - rad < 0 ? 0 : cz - rad, zb = cz + rad >= g.dim[2] ? g.dim[2] - 1 : cz + rad;
                            s0 = cell_start[col + za];
                            ln = (int)(cell_start[col + zb + 1] - s0);
                        }
                    }
                    const int incl = wave_incl_scan_i32(ln);
                    if (lane < 32) { run_s0[lane] = s0; run_off[lane] = lane < nruns ? incl - ln : INT_MAX; }
                    if (lane == 63) s_m = incl;
                }
                __syncthreads();
                const int m = s_m;
                if (m <= CAP) {
                    // the block's points -> LDS: thread t brings in points t, t + 256, ...; the run of a point by a fixed-depth search
#pragma unroll
                    for (int tr = 0; tr < CAP / T; ++tr) {
                        const int jn = tr * T + tid;
                        if (jn < m) {
                            int r = 0;
#pragma unroll
                            for (int st = 16; st > 0; st >>= 1) { const int cr = r + st; if (cr < nruns && run_off[cr] <= jn) r = cr; }
                            const float *pp = spts + 3 * (int64_t)(run_s0[r] + (uint32_t)(jn - run_off[r]));
                            cand[3 * jn] = pp[0]; cand[3 * jn + 1] = pp[1]; cand[3 * jn + 2] = pp[2];
                        }
                    }
                }
                __syncthreads();
                if (m <= CAP) {
                    const int c[3] = { cx, cy, cz };
                    for (int qi = pos + wave; qi < pos + len; qi += W) {
                        if (qstate[qi] != 0) continue;           // wave-uniform
                        const double q[3] = { (double)qf[0][qi], (double)qf[1][qi], (double)qf[2][qi] };
                        // inside the covered distance: at least kk candidates strictly nearer than the block's cover (the ring walk's rule);
                        // d^2 >= 0, so the IEEE patterns order like the values
                        const double cov2 = block_cover2(g, q, c, rad);
                        const bool whole = cov2 == INFINITY;
                        const unsigned ch = (unsigned)((unsigned long long)__double_as_longlong(cov2) >> 32);
                        unsigned hi[S], lo[S];
                        int cnt = 0, zeros = 0;                  // zeros: distances with a zero high word (the query itself, its duplicates)
                        unsigned vmin = 0xFFFFFFFFu;             // smallest non-zero high word
                        int vmax = -1;                           // largest high word (an empty slot's 0xFFFFFFFF is -1)
#pragma unroll
                        for (int sl = 0; sl < S; ++sl) {
                            hi[sl] = 0xFFFFFFFFu; lo[sl] = 0xFFFFFFFFu;
                            const int jn = sl * 64 + lane;
                            if (sl * 64 < m && jn < m) {
                                const double dx = q[0] - (double)cand[3 * jn], dy = q[1] - (double)cand[3 * jn + 1], dz = q[2] - (double)cand[3 * jn + 2];
                                const double d2 = fma(dz, dz, fma(dy, dy, dx * dx));
                                const unsigned long long pat = (unsigned long long)__double_as_longlong(d2);
                                hi[sl] = (unsigned)(pat >> 32); lo[sl] = (unsigned)pat;
                                cnt += d2 < cov2 ? 1 : 0;
                                zeros += hi[sl] == 0u ? 1 : 0;
                                const unsigned nz = hi[sl] == 0u ? 0xFFFFFFFFu : hi[sl];
                                vmin = nz < vmin ? nz : vmin;
                                vmax = (int)hi[sl] > vmax ? (int)hi[sl] : vmax;
                            }
                        }
                        cnt = wave_sum_i(cnt);
                        zeros = wave_sum_i(zeros);
                        const int kk = whole ? (m < k ? m : k) : k;
                        bool ok = cnt >= kk;                     // wave-uniform from here on
                        // The window of the k-th high word: from the smallest NON-ZERO one (the query is its own nearest candidate: with
                        // zero in the window the first level's buckets are eight binades wide and hold everything else in two or three
                        // of them) up to the largest, or the cover's -- at least kk candidates lie strictly inside the cover
                        unsigned a = wave_min_u(vmin);
                        unsigned b = wave_max_u((unsigned)(vmax < 0 ? 0 : vmax));
                        if (!whole && b > ch) b = ch;
                        bool exact = false;                      // a pivot with exactly kk patterns at or below it was met
                        {
                            constexpr int BPL = kSorBuckets / 64;
                            int need_k = kk - zeros;             // rank of the k-th among the candidates at or above the window's start
                            if (need_k <= 0) a = b = 0u;         // the k-th is one of the zero distances
                            unsigned range = b - a;
                            bool run = ok && a < b;
                            while (run) {
                                const int shift = range >= 256u ? 24 - __builtin_clz(range) : 0;
                                uint4 *hz = reinterpret_cast<uint4 *>(hist + lane * BPL);
                                hz[0] = make_uint4(0u, 0u, 0u, 0u);
                                wave_lds_fence();
#pragma unroll
                                for (int sl = 0; sl < S; ++sl)
                                    if (sl * 64 < m) {
                                        const unsigned rel = hi[sl] - a;
                                        if (rel <= range) __hip_atomic_fetch_add(hist + (rel >> shift), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                                    }
                                wave_lds_fence();
                                const uint4 t4 = hz[0];
                                const int hv[BPL] = { (int)t4.x, (int)t4.y, (int)t4.z, (int)t4.w };
                                const int lsum = hv[0] + hv[1] + hv[2] + hv[3];
                                const int incl = wave_incl_scan_i32(lsum), excl = incl - lsum;
                                const bool mine = need_k > excl && need_k <= incl;
                                int B = -1, cb = 0, hb = 0;
                                if (mine) {
                                    int cum = excl;
#pragma unroll
                                    for (int w = 0; w < BPL; ++w) {
                                        if (B < 0 && need_k <= cum + hv[w]) { B = lane * BPL + w; cb = cum; hb = hv[w]; }
                                        cum += hv[w];
                                    }
                                }
                                const unsigned long long bm = __builtin_amdgcn_ballot_w64(mine);
                                const int owner = bm ? __builtin_ctzll(bm) : 0;
                                B = wave_bcast(B, owner); cb = wave_bcast(cb, owner); hb = wave_bcast(hb, owner);
                                // (the window's end may cut the last bucket -- the cover's high word at the first level: nothing beyond it was counted)
                                const unsigned wend = a + range, bstart = a + ((unsigned)(B < 0 ? 0 : B) << shift), bspan = (1u << shift) - 1u;
                                const unsigned bend = wend - bstart < bspan ? wend : bstart + bspan;
                                if (B < 0) { ok = false; run = false; }                       // cannot happen (cnt >= kk)
                                else if (need_k - cb == hb) { a = bend; exact = true; run = false; }     // the k-th is the last of its bucket
                                else if (shift == 0) { a = bstart; run = false; }                        // one value wide: THE k-th high word
                                else { need_k -= cb; a = bstart; range = bend - bstart; }
                            }
                        }
                        const unsigned P = a;
                        unsigned Q = 0xFFFFFFFFu;
                        int n_le = kk;
                        if (ok && !exact) {
                            int c_less = 0, c_eq = 0;
#pragma unroll
                            for (int sl = 0; sl < S; ++sl) if (sl * 64 < m) { c_less += hi[sl] < P ? 1 : 0; c_eq += hi[sl] == P ? 1 : 0; }
                            c_less = wave_sum_i(c_less); c_eq = wave_sum_i(c_eq);
                            n_le = c_less + c_eq;
                            // several candidates share the k-th high word and not all of them fit: the low words decide
                            const int r2 = kk - c_less;
                            if (n_le > kk) {
                                unsigned lmin = 0xFFFFFFFFu, lmax = 0u;
#pragma unroll
                                for (int sl = 0; sl < S; ++sl) if (hi[sl] == P) { lmin = lo[sl] < lmin ? lo[sl] : lmin; lmax = lo[sl] > lmax ? lo[sl] : lmax; }
                                unsigned a2 = wave_min_u(lmin), b2 = wave_max_u(lmax);
                                while (a2 < b2) {
                                    const unsigned mid = a2 + ((b2 - a2) >> 1);
                                    int c2 = 0;
#pragma unroll
                                    for (int sl = 0; sl < S; ++sl) c2 += (hi[sl] == P && lo[sl] <= mid) ? 1 : 0;
                                    c2 = wave_sum_i(c2);
                                    if (c2 >= r2) b2 = mid; else a2 = mid + 1;
                                }
                                int c3 = 0;
#pragma unroll
                                for (int sl = 0; sl < S; ++sl) c3 += (hi[sl] == P && lo[sl] <= a2) ? 1 : 0;
                                c3 = wave_sum_i(c3);
                                Q = a2; n_le = c_less + c3;
                            }
                        }
                        const bool tied_out = ok && n_le > kk + kSorTieRoom;     // ties far beyond k (duplicates, lattices): the wave-per-query passes
                        if (tied_out) ok = false;
                        if (ok) {
                            // the selected patterns (all <= (P, Q)), lane by lane -> selection buffer -> sum of square roots
                            // in the block's own order (candidate 0, 1, 2, ...): a ballot per row of 64 candidates places them
                            int wbase = 0;
#pragma unroll
                            for (int sl = 0; sl < S; ++sl)
                                if (sl * 64 < m) {
                                    const bool sel = hi[sl] < P || (hi[sl] == P && lo[sl] <= Q);
                                    const unsigned long long bm = __builtin_amdgcn_ballot_w64(sel);
                                    if (sel)
                                        selbuf[wbase + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bm, 0u))] =
                                            __longlong_as_double((long long)(((unsigned long long)hi[sl] << 32) | lo[sl]));
                                    wbase += __builtin_popcountll(bm);
                                }
                            wave_lds_fence();
                            double acc = 0.0;
                            for (int t = lane; t < n_le; t += 64) acc += sqrt(selbuf[t]);
                            acc = wave_sum_down_f64(acc);
                            if (lane == 0) {
                                const double top = __longlong_as_double((long long)(((unsigned long long)P << 32) | Q));
                                const double total = n_le > kk ? acc - (double)(n_le - kk) * sqrt(top) : acc;
                                avg[qsidx[qi]] = kk > 0 ? total / (double)kk : -1.0;
                            }
                            wave_lds_fence();
                        }
                        if (lane == 0 && (ok || tied_out)) qstate[qi] = ok ? 1 : 2;
                    }
                }
                __syncthreads();                                 // the states are written and the staged block may be replaced
            }
        }
        // what neither block settled: ONE counter update per chunk
        if (wave == 0) {
            const bool fb = lane < nqc && qstate[lane] != 1;
            const unsigned long long fm = __builtin_amdgcn_ballot_w64(fb);
            if (fm != 0ull) {
                int fb_base = 0;
                if (lane == 0) fb_base = atomicAdd(fb_count, __builtin_popcountll(fm));
                fb_base = wave_bcast(fb_base, 0);
                if (fb) fb_list[fb_base + __builtin_popcountll(fm & ((1ull << lane) - 1ull))] = (int32_t)(base + lane);
            }
        }
        __syncthreads();
    }
}

// mean / std exactly as [O3D]: mean = sum(avg>0)/n ; std = sqrt(sum_{avg>0}(avg-mean)^2/(n-1))
__global__ __launch_bounds__(256) void sor_sum_kernel(const double *__restrict__ avg, int64_t n, const double *__restrict__ stats,
                                                      int pass, double *__restrict__ part)
{
    __shared__ double sh[4];
    double mean = pass ? stats[0] : 0.0, acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        double v = avg[i];
        if (v > 0.0) acc += pass ? (v - mean) * (v - mean) : v;
    }
    acc = block_sum(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}
__global__ void sor_final_kernel(const double *__restrict__ part, int nb, int64_t n, double std_ratio, int pass, double *stats)
{
    if (threadIdx.x || blockIdx.x) return;
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += part[b];
    if (pass == 0) stats[0] = s / (double)n;
    else { stats[1] = sqrt(s / (double)(n - 1)); stats[2] = stats[0] + std_ratio * stats[1]; }
}
struct SorPred {
    const double *avg; const double *stats;
    __device__ bool operator()(int64_t i, int) const { double v = avg[i]; return v > 0.0 && v < stats[2]; }
};
struct IdxEmit {
    int32_t *idx;
    __device__ void operator()(int64_t i, int, int32_t dst) const { idx[dst] = (int32_t)i; }
};
// keep list AND the kept rows of up to two (n,3) attribute arrays: `cl, ind = remove_statistical_outlier(...)` without a host round trip
struct SorGather {
    const float *a0, *a1;
    float *o0, *o1;
};
// the kept rows, gathered by a launch of its own whose length is read on the DEVICE (the keep list's count): inside the compaction's
// emit the eight items of a thread gathered one after the other (17 us for 23k points against 6 + 4 for compaction + this kernel)
// d_count: in device memory (every thread reads it); count_out: the caller's count word, which may be host-visible pinned memory
__global__ __launch_bounds__(256) void sor_gather_kernel(SorGather g, const int32_t *__restrict__ idx, const int32_t *__restrict__ d_count,
                                                         int32_t *__restrict__ count_out)
{
    const int64_t n = *d_count;
    if (blockIdx.x == 0 && threadIdx.x == 0) *count_out = (int32_t)n;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = idx[k];
        if (g.a0) { g.o0[3 * k] = g.a0[3 * s]; g.o0[3 * k + 1] = g.a0[3 * s + 1]; g.o0[3 * k + 2] = g.a0[3 * s + 2]; }
        if (g.a1) { g.o1[3 * k] = g.a1[3 * s]; g.o1[3 * k + 1] = g.a1[3 * s + 1]; g.o1[3 * k + 2] = g.a1[3 * s + 2]; }
    }
}

static int sor_block_threads(int k)
{
    // k * threads * 8 B of LDS per block; keep >= 2 blocks per CU where k allows
    if (k <= 32) return 256;
    if (k <= 80) return 128;
    return 64;
}

// The four launches below (partial sums, fold, partial squared deviations, fold) as ONE block for clouds it can walk in a few
// microseconds: the same block partition (thread t of virtual block b adds items b*2048 + t, +256, ... in the same order, the
// virtual blocks' sums are folded in the same order), so the statistics are bit-identical to the multi-launch form.
__global__ __launch_bounds__(1024) void sor_stats_small_kernel(const double *__restrict__ avg, int64_t n, int nb, double std_ratio, double *__restrict__ stats)
{
    __shared__ double part[64];               // nb <= 64 virtual blocks of 256 threads x 8 items
    __shared__ double sh[4][4];
    __shared__ double s_mean;
    const int vb = threadIdx.x >> 8, t = threadIdx.x & 255;          // 4 virtual blocks at a time
    for (int pass = 0; pass < 2; ++pass) {
        const double mean = pass ? s_mean : 0.0;
        for (int b0 = 0; b0 < nb; b0 += 4) {
            const int b = b0 + vb;
            double acc = 0.0;
            if (b < nb)
                for (int64_t i0 = (int64_t)b * 256 + t; i0 < n; i0 += 8 * (int64_t)nb * 256) {      // 8 loads in flight, added in the same order
                    double v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int64_t i = i0 + (int64_t)u * nb * 256;
                        v[u] = i < n ? avg[i] : 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        if (v[u] > 0.0) acc += pass ? (v[u] - mean) * (v[u] - mean) : v[u];
                }
            // block_sum of a 256-thread block: wave sums, then the four waves in order
            acc = wave_sum(acc);
            if ((t & 63) == 0) sh[vb][t >> 6] = acc;
            __syncthreads();
            if (t == 0 && b < nb) part[b] = ((sh[vb][0] + sh[vb][1]) + sh[vb][2]) + sh[vb][3];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            double s = 0.0;
            for (int b = 0; b < nb; ++b) s += part[b];
            if (pass == 0) { stats[0] = s / (double)n; s_mean = stats[0]; }
            else { stats[1] = sqrt(s / (double)(n - 1)); stats[2] = stats[0] + std_ratio * stats[1]; }
        }
        __syncthreads();
    }
}

// statistics over avg (caller's point order) + ascending keep list -- shared by kpx_sor and kpx_sor_finish, so that the
// sharded filter folds the very same reduction tree over the very same array as the one-GPU call
static int sor_stats_compact(const double *avg, int64_t n, double std_ratio, double *part, int32_t *counts, int32_t *keep_idx,
                             int32_t *d_count, double *d_stats, hipStream_t st, const SorGather *ga = nullptr, bool state_is_clear = false)
{
    int nb = (int)(cdiv(n, 256 * 8) < 1 ? 1 : (cdiv(n, 256 * 8) > 1024 ? 1024 : cdiv(n, 256 * 8)));
    if (nb <= 64) {
        hipLaunchKernelGGL(sor_stats_small_kernel, dim3(1), dim3(1024), 0, st, avg, n, nb, std_ratio, d_stats);
    } else {
        for (int pass = 0; pass < 2; ++pass) {
            hipLaunchKernelGGL(sor_sum_kernel, dim3(nb), dim3(256), 0, st, avg, n, d_stats, pass, part);
            hipLaunchKernelGGL(sor_final_kernel, dim3(1), dim3(1), 0, st, part, nb, n, std_ratio, pass, d_stats);
        }
    }
    KPX_LAUNCH_CHECK();
    int32_t *dev_count = reinterpret_cast<int32_t *>(part + 1023);              // the gather reads the count on the device
    const int rc = compact(SorPred{ avg, d_stats }, IdxEmit{ keep_idx }, n, 1, counts, ga ? dev_count : d_count, st, state_is_clear);
    if (rc || !ga) return rc;
    const int64_t gb = cdiv(n, 256);
    hipLaunchKernelGGL(sor_gather_kernel, dim3((unsigned)(gb < 1 ? 1 : (gb > 4096 ? 4096 : gb))), dim3(256), 0, st, *ga, keep_idx, dev_count, d_count);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

__global__ __launch_bounds__(256) void sor_unsort_kernel(const double *__restrict__ avg_sorted, const int32_t *__restrict__ order, int64_t n,
                                                         double *__restrict__ avg)
{
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) avg[order[s]] = avg_sorted[s];
}

// q0 <= q1: only the queries at cell-sorted positions [q0, q1) are searched (kpx_sor_partial: avg_out is indexed by sorted
// position - q0 and the statistics / keep list are skipped); full == true: the whole filter (kpx_sor)
static int sor_impl(const float *pts, int64_t n, int k, double std_ratio, int32_t *keep_idx, int32_t *d_count, double *d_stats,
                    double *d_avg, Arena &a, hipStream_t st, bool full = true, int64_t q0 = 0, int64_t q1 = 0, int32_t *d_order = nullptr,
                    const SorGather *ga = nullptr)
{
    Grid g;
    if (full) { q0 = 0; q1 = n; }
    int kk = (int64_t)k < n ? k : (int)(n > 0 ? n : 1);
    // cell occupancy (as seen by a point) ~0.4 k: the 27-cell block then holds ~10 k candidates and usually covers the
    // k-th neighbour
    // (with the cell's queries answered together -- sor_block_kernel -- a query that the 27-cell block does not cover costs a second,
    // wave-per-query search, so the cells are sized to cover the k-th neighbour of nearly every query: r_k ~ sqrt(k / (pi rho)) against
    // h = sqrt(occ / rho) on a surface of density rho)
    static const double occ_factor = [] { const char *e = getenv("KPX_SOR_OCC"); const double v = e ? atof(e) : 0.0; return v > 0.0 ? v : 0.4; }();
    double occ = occ_factor * (double)kk;
    occ = occ < 6.0 ? 6.0 : (occ > 240.0 ? 240.0 : occ);
    int rc = grid_build(pts, n, occ, a, &g, st);
    if (rc) return rc;
    double *avg = a.get<double>((size_t)(n > 0 ? n : 1));
    double *part = a.get<double>(1024);
    int32_t *counts = a.get<int32_t>((size_t)compact_ws_ints(n));
    int32_t *fb_list = a.get<int32_t>((size_t)(n > 0 ? n : 1) + 1);
    int32_t *fb_list2 = a.get<int32_t>((size_t)(n > 0 ? n : 1) + 1);
    int32_t *fb_list0 = a.get<int32_t>((size_t)(n > 0 ? n : 1) + 1);
    int32_t *fb_listg = a.get<int32_t>((size_t)(n > 0 ? n : 1) + 1);      // what the group pass hands on
    // k beyond the LDS heaps (KPX_SOR_LDS_K): the last pass's per-thread heaps live in the workspace
    const KnnHeaps hp = knn_heaps_carve(a, kk, KPX_SOR_LDS_K, false, sor_block_threads(kk));
    if (a.dry) return KPX_OK;
    KPX_ARENA_CHECK(a);
    if (d_avg) avg = d_avg;
    const int32_t *out_idx = full ? g.sorted_idx : nullptr;
    const int64_t nq = q1 - q0;
    int32_t *fb_count0 = g.spare + 2;                             // cleared by the grid build; words 0 and 1: the cascade's passes, word 3: the group pass
    {
        ProfScope prof(KPX_PROF_SOR_KNN, 12.0 * (double)n + 8.0 * (double)n, st);     // read points, write mean distances
        // pass 0: the queries of a cell together (sor_block_kernel<S>: a block per 64 queries, 64 x S candidates at most); what it cannot
        // settle goes to the wave-per-query passes below through fb_list0.
        // Measured (profiles/r05/sor_probe.txt, pass 0 off -> forced on): it wins where a query's candidates are many -- (200, 3.0) on a
        // 221k-point fused cloud 1.91 -> 1.25 ms (sor_block_kernel<32> is 0.94 of that: sor_k200_kernels.txt), (50, 0.30) at 259k points
        // 1.20 -> 0.98 -- and loses at k = 20, where the wave-per-query pass alone is faster (259k points 0.85 -> 0.91 ms, a frame-sized
        // 26k-point cloud 0.14 -> 0.21, 1M raw points 5.35 -> 7.06).  So: KPX_SOR_CELL unset = from k > 32 on, 1 = at every k, 0 = never
        // (every query starts at pass 1); k <= 1024 in every case: the largest block holds 2048 candidates.
        static const int cell_mode = [] { const char *e = getenv("KPX_SOR_CELL"); return e ? (e[0] == '0' ? 0 : 2) : 1; }();
        const bool cell_on = (cell_mode == 2 || (cell_mode == 1 && kk > 32)) && kk <= 1024;
        const int32_t *list0 = nullptr, *count0 = nullptr;
        if (cell_on && nq > 0) {
            const int kbuf = kk + kSorTieRoom;
            const int64_t bchunks = cdiv(nq, kBlkQueries);
            const int S = kk <= 32 ? 4 : (kk <= 64 ? 8 : (kk <= 128 ? 16 : 32));          // rows of 64 candidates a block holds
            const auto kernel = S == 4 ? sor_block_kernel<4> : (S == 8 ? sor_block_kernel<8> : (S == 16 ? sor_block_kernel<16> : sor_block_kernel<32>));
            // LDS: the staged points, a bucket array and a selection buffer per wave
            hipLaunchKernelGGL(kernel, dim3((unsigned)(bchunks > 16384 ? 16384 : bchunks)), dim3(64 * kBlkWaves),
                               ((size_t)(64 * S * 3) / 2 + (size_t)kBlkWaves * kSorBuckets / 2 + (size_t)kBlkWaves * kbuf) * 8, st, g.params, g.cell_start,
                               g.sorted_pts, out_idx, q0, q1, kk, kbuf, avg, fb_list0, fb_count0);
            list0 = fb_list0; count0 = fb_count0;
        }
        // the group pass (knn_group_kernel: four queries per wave) where every query would start at pass 1: it settles the common path and
        // lists the rest for the passes below (profiles/r06/exp_knn_group.txt)
        if (KPX_KNN_GROUP && !cell_on && kk <= 32) {
            rc = knn_group_pass<SorOp, KPX_KNN_GROUP_CAP_SOR>(g, kk, SorOp{ out_idx, q0, avg }, q0, q1, fb_listg, g.spare + 3, st);
            if (rc) return rc;
            if (nq > 0) { list0 = fb_listg; count0 = g.spare + 3; }
        }
        // pass 1: one wave per query, 512- or 1024-candidate buffer (small k: smaller buffers, more waves per CU); k beyond half a
        // buffer skips the pass whose buffer cannot hold k candidates plus their surroundings -- the queries go on through the same lists
        // pass 2: the queries whose block did not fit (isolated points next to a dense sheet), 8192-candidate buffer
        // pass 3: whatever is left: thread-per-query ring walk with a k-heap (in LDS; in the workspace for k > KPX_SOR_LDS_K)
        rc = knn_cascade<SorOp>(g, kk, SorOp{ out_idx, q0, avg }, q0, q1, list0, count0,
                                { knn_wave_pass<SorOp, 4>(kk <= 32 ? 512 : 1024, list0 ? 2048 : 8192, fb_list, kk <= 512),
                                  knn_wave_pass<SorOp, 1>(8192, 2048, fb_list2, kk <= 4096) },
                                g.spare, knn_heap_pass<SorOp>(), hp, st);
        if (rc) return rc;
    }
    if (!full) {
        if (d_order) KPX_HIP(hipMemcpyAsync(d_order, g.sorted_idx, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        KPX_LAUNCH_CHECK();
        return KPX_OK;
    }
    // the grid build cleared g.extra together with its counters: the compaction's tile states live there when they fit
    const bool fits = compact_ws_ints(n) <= kGridExtraWords;
    return sor_stats_compact(avg, n, std_ratio, part, fits ? g.extra : counts, keep_idx, d_count, d_stats, st, ga, fits);
}

// ---- estimate_normals ---------------------------------------------------------------------------------
// the symmetric 3x3 (xx, xy, xz, yy, yz, zz) as 9 row-major doubles; nullptr: the identity ([O3D] estimate_covariances, < 3 neighbours)
__device__ __forceinline__ void store_cov9(double *o, const double *cov)
{
    if (!cov) {
#pragma unroll
        for (int e = 0; e < 9; ++e) o[e] = (e % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    o[0] = cov[0]; o[1] = cov[1]; o[2] = cov[2];
    o[3] = cov[1]; o[4] = cov[3]; o[5] = cov[4];
    o[6] = cov[2]; o[7] = cov[4]; o[8] = cov[5];
}
// nine raw moment sums and their count -> the normal (eigenvector of the smallest eigenvalue), or -- COV: estimate_covariances -- the
// covariance to out_cov [n][9]; < 3 neighbours: (0, 0, 1) / the identity.  me: the query's original index.
template <bool COV>
__device__ __forceinline__ void moments_finish(const double sums[9], double m, int64_t me, float *__restrict__ normals, double *__restrict__ out_cov)
{
    double cov[6], nrm[3] = { 0.0, 0.0, 1.0 };
    const bool enough = m >= 3.0;
    if (enough) cov6_from_moments(sums, m, cov);
    if constexpr (COV) {
        if (enough) store_cov9(out_cov + 9 * me, cov);
        else store_cov9(out_cov + 9 * me, nullptr);
    } else {
        if (enough) sym3_smallest_axis(cov, nrm);
        normals[3 * me] = (float)nrm[0]; normals[3 * me + 1] = (float)nrm[1]; normals[3 * me + 2] = (float)nrm[2];
    }
}
// The raw moments of the hybrid neighbourhood, as an operator of knn_wave_kernel / knn_heap_kernel (kpx_gridknn.h).  Wave form: the
// sums of the selected neighbours go to covbuf [n][10] (nine sums, count; count < 0: the query was handed to the heap walk) -- the 3x3
// eigen-problem is serial work and runs one thread per query in normals_eigen_kernel.  Ties at the k-th distance are resolved like the
// (d^2, index) heap of the heap form: the lowest original indices stay.  Heap form: sums in heap-slot order, finished in place
// (heap: normals, heap_alt: covariances).
struct MomentsOp {
    static constexpr bool kPos = true;
    static constexpr int kGroupWavesPerSimd = 3, kGroupTrips = 4; // knn_group_kernel: a register budget of 168, trips of 16 candidates fetched together
    using Heap = HeapDI;
    const int32_t *sidx;
    const float *pts;
    double r2;
    double *covbuf;
    float *normals;
    double *out_cov;
    __device__ double r2max(bool) const { return r2; }
    __device__ void defer(int64_t s) const { covbuf[10 * s + 9] = -1.0; }
    __device__ void wave(const WaveKnnScratch &sc, const WaveKnnResult &res, int64_t s, const float *__restrict__ spts) const
    {
        const int lane = threadIdx.x & 63;
        const int32_t idx_thr = wave_knn_tie_threshold(sc, res, sidx);
        double c[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
        for (int t = lane; t < res.m; t += 64) {
            if (wave_knn_is_selected(sc, res, sidx, idx_thr, t)) {
                const float *pp = spts + 3 * (int64_t)sc.pos[t];
                const double x = pp[0], y = pp[1], z = pp[2];
                c[0] += x; c[1] += y; c[2] += z;
                c[3] += x * x; c[4] += x * y; c[5] += x * z; c[6] += y * y; c[7] += y * z; c[8] += z * z;
            }
        }
        wave_sum_down_f64x9(c);                                      // lane 0: the tree the xor butterfly left there
        if (lane == 0) {
            double *o = covbuf + 10 * s;
#pragma unroll
            for (int a9 = 0; a9 < 9; ++a9) o[a9] = c[a9];
            o[9] = (double)res.kk;
        }
    }
    // the group form (knn_group_kernel): exactly kk selected, so the index tie rule is never asked.  An accumulator starts at +0 and
    // never becomes -0, so a candidate that is not selected adds zeros -- no branch around the loads
    __device__ void row(const RowKnnResult &res, int64_t s, const float *__restrict__ spts) const
    {
        const int j = threadIdx.x & 15;
        const uint32_t *w32 = reinterpret_cast<const uint32_t *>(res.vals);
        auto acc = [&](int qd, double a[9]) {                       // lane j + 16 qd of wave(): candidates j + 16 qd, + 64, ... in turn
#pragma unroll
            for (int e = 0; e < 9; ++e) a[e] = 0.0;
#pragma unroll 4
            for (int t = 16 * qd + j; t < 16 * res.trips16; t += 64) {
                const bool sel = t < res.m && w32[2 * t + 1] <= res.hi_thr;
                const float *pp = spts + 3 * (sel ? (int64_t)res.pos[t] : s);
                const double x = sel ? (double)pp[0] : 0.0, y = sel ? (double)pp[1] : 0.0, z = sel ? (double)pp[2] : 0.0;
                a[0] += x; a[1] += y; a[2] += z;
                a[3] += x * x; a[4] += x * y; a[5] += x * z; a[6] += y * y; a[7] += y * z; a[8] += z * z;
            }
        };
        // (a0 + a2) + (a1 + a3): steps 32 and 16 of wave_sum_down_f64x9; at most three sets of nine are live
        double c[9], b[9], a[9];
        acc(0, c); acc(2, a);
#pragma unroll
        for (int e = 0; e < 9; ++e) c[e] += a[e];
        acc(1, b); acc(3, a);
#pragma unroll
        for (int e = 0; e < 9; ++e) c[e] += b[e] + a[e];
        row_sum_down_f64x9(c);
        if (res.store && j == 0) {
            double *o = covbuf + 10 * s;
#pragma unroll
            for (int a9 = 0; a9 < 9; ++a9) o[a9] = c[a9];
            o[9] = (double)res.kk;
        }
    }
    template <bool COV> __device__ void heap_finish(int64_t s, const HeapDI &heap) const
    {
        double c[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
        if (heap.sz >= 3)
            for (int e = 0; e < heap.sz; ++e) {
                int64_t j = heap.ix[e * heap.stride];
                double x = pts[3 * j], y = pts[3 * j + 1], z = pts[3 * j + 2];
                c[0] += x; c[1] += y; c[2] += z;
                c[3] += x * x; c[4] += x * y; c[5] += x * z; c[6] += y * y; c[7] += y * z; c[8] += z * z;
            }
        moments_finish<COV>(c, (double)heap.sz, sidx[s], normals, out_cov);
    }
    __device__ void heap(int64_t s, const HeapDI &h) const { heap_finish<false>(s, h); }
    __device__ void heap_alt(int64_t s, const HeapDI &h) const { heap_finish<true>(s, h); }
};
// the wave form's sums -> normal / covariance; one thread per (cell-sorted) query
template <bool COV>
__global__ __launch_bounds__(256) void normals_eigen_kernel(const double *__restrict__ covbuf, const int32_t *__restrict__ sidx, int64_t n,
                                                            float *__restrict__ normals, double *__restrict__ out_cov)
{
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const double *in = covbuf + 10 * s;
    const double m = in[9];
    if (m < 0.0) return;                                         // the heap walk writes this query's result itself
    moments_finish<COV>(in, m, sidx[s], normals, out_cov);
}

// normals != nullptr: estimate_normals; otherwise out_cov [n][9]: estimate_covariances (the same search, the covariance the normal comes from)
static int normals_impl(const float *pts, int64_t n, double radius, int max_nn, float *normals, Arena &a, hipStream_t st,
                        double *out_cov = nullptr)
{
    Grid g;
    int kk = (int64_t)max_nn < n ? max_nn : (int)(n > 0 ? n : 1);
    int rc = grid_build(pts, n, 8.0, a, &g, st);
    if (rc) return rc;
    int32_t *fb_list = a.get<int32_t>((size_t)(n > 0 ? n : 1) + 1);
    double *covbuf = a.get<double>((size_t)(n > 0 ? n : 1) * 10);
    int32_t *fb_listg = a.get<int32_t>((size_t)(n > 0 ? n : 1) + 1);      // what the group pass hands on
    const KnnHeaps hp = knn_heaps_carve(a, kk, KPX_NORMALS_LDS_NN, true, kk <= 48 ? 128 : 64);
    if (a.dry) return KPX_OK;
    KPX_ARENA_CHECK(a);
    // pass 1: one wave per query, 512- or 1024-candidate buffer; pass 2: the few queries that did not fit, thread-per-query heap walk
    // (max_nn > 512: the wave kernel's 1024-candidate buffer cannot hold a neighbourhood and its surroundings -- every query takes the heap walk)
    const bool wave_pass = kk <= 512;
    const MomentsOp op{ g.sorted_idx, pts, radius * radius, covbuf, normals, out_cov };
    // in front of it the group pass (knn_group_kernel: four queries per wave; counter word 3 of Grid::spare): the wave pass then searches
    // only what that one listed
    const int32_t *list0 = nullptr, *count0 = nullptr;
    if (KPX_KNN_GROUP && kk <= 48 && n > 0) {
        rc = knn_group_pass<MomentsOp, KPX_KNN_GROUP_CAP_NORMALS>(g, kk, op, 0, n, fb_listg, g.spare + 3, st);
        if (rc) return rc;
        list0 = fb_listg; count0 = g.spare + 3;
    }
    rc = knn_cascade<MomentsOp>(g, kk, op, 0, n, list0, count0,
                                { knn_wave_pass<MomentsOp, 4>(kk <= 48 ? 512 : 1024, list0 ? 2048 : 8192, fb_list, wave_pass) }, g.spare,
                                out_cov ? knn_heap_pass<MomentsOp, true>() : knn_heap_pass<MomentsOp, false>(), hp, st);
    if (rc) return rc;
    const auto eigen_kernel = out_cov ? normals_eigen_kernel<true> : normals_eigen_kernel<false>;
    if (wave_pass) hipLaunchKernelGGL(eigen_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, covbuf, g.sorted_idx, n, normals, out_cov);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

}  // namespace kpx

using namespace kpx;

KPX_EXPORT size_t kpx_sor_workspace_bytes(int64_t n, int32_t nb_neighbors)
{
    Arena a(nullptr, 0);
    sor_impl(nullptr, n, nb_neighbors < 1 ? 1 : nb_neighbors, 1.0, nullptr, nullptr, nullptr, nullptr, a, nullptr);
    return a.off;
}
KPX_EXPORT int kpx_sor(const float *pts, int64_t n, int32_t nb_neighbors, double std_ratio, int32_t *keep_idx,
                       int32_t *d_count, double *d_stats, double *d_avg, void *ws, size_t ws_bytes, void *stream)
{
    // [O3D] "Illegal input parameters, the number of neighbors and standard deviation ratio must be positive"
    KPX_REQUIRE(nb_neighbors >= 1 && std_ratio > 0.0, "remove_statistical_outlier: nb_neighbors and std_ratio must be positive");
    KPX_REQUIRE(nb_neighbors <= KPX_SOR_MAX_K, "remove_statistical_outlier: nb_neighbors > %d is not supported", KPX_SOR_MAX_K);
    KPX_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "kpx_sor: bad size");
    KPX_REQUIRE(d_count && d_stats && ws, "kpx_sor: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) { KPX_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), st)); return KPX_OK; }
    KPX_REQUIRE(pts && keep_idx, "kpx_sor: null pointer");
    Arena a(ws, ws_bytes);
    return sor_impl(pts, n, nb_neighbors, std_ratio, keep_idx, d_count, d_stats, d_avg, a, st);
}

KPX_EXPORT int kpx_sor_select(const float *pts, const float *attr, int64_t n, int32_t nb_neighbors, double std_ratio, float *out_pts,
                              float *out_attr, int32_t *keep_idx, int32_t *d_count, double *d_stats, void *ws, size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(nb_neighbors >= 1 && std_ratio > 0.0, "remove_statistical_outlier: nb_neighbors and std_ratio must be positive");
    KPX_REQUIRE(nb_neighbors <= KPX_SOR_MAX_K, "remove_statistical_outlier: nb_neighbors > %d is not supported", KPX_SOR_MAX_K);
    KPX_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "kpx_sor_select: bad size");
    KPX_REQUIRE(d_count && d_stats && ws, "kpx_sor_select: null pointer");
    KPX_REQUIRE(!attr || out_attr, "kpx_sor_select: attributes without an output array");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) { KPX_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), st)); return KPX_OK; }
    KPX_REQUIRE(pts && keep_idx && out_pts, "kpx_sor_select: null pointer");
    Arena a(ws, ws_bytes);
    const SorGather ga{ pts, attr, out_pts, out_attr };
    return sor_impl(pts, n, nb_neighbors, std_ratio, keep_idx, d_count, d_stats, nullptr, a, st, true, 0, 0, nullptr, &ga);
}

KPX_EXPORT int kpx_sor_partial(const float *pts, int64_t n, int32_t nb_neighbors, int64_t q_begin, int64_t q_end, double *d_avg_sorted,
                               int32_t *d_order, void *ws, size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(nb_neighbors >= 1, "remove_statistical_outlier: nb_neighbors and std_ratio must be positive");
    KPX_REQUIRE(nb_neighbors <= KPX_SOR_MAX_K, "remove_statistical_outlier: nb_neighbors > %d is not supported", KPX_SOR_MAX_K);
    KPX_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "kpx_sor_partial: bad size");
    KPX_REQUIRE(q_begin >= 0 && q_begin <= q_end && q_end <= n, "kpx_sor_partial: bad query range");
    KPX_REQUIRE(pts && ws && (d_avg_sorted || q_begin == q_end), "kpx_sor_partial: null pointer");
    Arena a(ws, ws_bytes);
    return sor_impl(pts, n, nb_neighbors, 1.0, nullptr, nullptr, nullptr, d_avg_sorted, a, (hipStream_t)stream, false, q_begin, q_end, d_order);
}
// [n] the mean distances in the caller's order, [1024] sor_stats_compact's partial sums, compact()'s tile words
struct SorFinishScratch { double *avg, *part; int32_t *counts; };
static void sor_finish_carve(Arena &a, int64_t n, SorFinishScratch *s)
{
    s->avg = a.get<double>((size_t)(n > 0 ? n : 1));
    s->part = a.get<double>(1024);
    s->counts = a.get<int32_t>((size_t)compact_ws_ints(n));
}
KPX_EXPORT size_t kpx_sor_finish_workspace_bytes(int64_t n)
{
    Arena a(nullptr, 0);
    SorFinishScratch s;
    sor_finish_carve(a, n, &s);
    return a.off;
}
KPX_EXPORT int kpx_sor_finish(const double *d_avg_sorted, const int32_t *d_order, int64_t n, double std_ratio, int32_t *keep_idx,
                              int32_t *d_count, double *d_stats, double *d_avg, void *ws, size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(std_ratio > 0.0, "remove_statistical_outlier: nb_neighbors and std_ratio must be positive");
    KPX_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "kpx_sor_finish: bad size");
    KPX_REQUIRE(d_avg_sorted && d_order && keep_idx && d_count && d_stats && ws, "kpx_sor_finish: null pointer");
    hipStream_t st = (hipStream_t)stream;
    Arena a(ws, ws_bytes);
    SorFinishScratch s;
    sor_finish_carve(a, n, &s);
    KPX_ARENA_CHECK(a);
    double *avg = d_avg ? d_avg : s.avg;
    hipLaunchKernelGGL(sor_unsort_kernel, dim3((unsigned)(cdiv(n, 256) > 4096 ? 4096 : cdiv(n, 256))), dim3(256), 0, st, d_avg_sorted, d_order, n, avg);
    return sor_stats_compact(avg, n, std_ratio, s.part, s.counts, keep_idx, d_count, d_stats, st);
}

// out[0]: the queries the calling thread's last group pass (knn_group_kernel: SOR with k <= 32, normals / covariances with max_nn <= 48) was
// given, out[1]: the ones it handed on to the wave passes -- read back from the pass's counter word, so valid until the workspace of
// that call is used again; waits for the call's stream.  {0, 0}: no such pass yet.
KPX_EXPORT int kpx_knn_group_last(int64_t *out)
{
    KPX_REQUIRE(out, "kpx_knn_group_last: null pointer");
    out[0] = out[1] = 0;
    const ThreadResources &tr = thread_resources();
    if (!tr.knn_group_word) return KPX_OK;
    int32_t handed = 0;
    KPX_HIP(hipStreamSynchronize(tr.knn_group_stream));
    KPX_HIP(hipMemcpy(&handed, tr.knn_group_word, sizeof(int32_t), hipMemcpyDeviceToHost));
    out[0] = tr.knn_group_given; out[1] = handed;
    return KPX_OK;
}

KPX_EXPORT size_t kpx_normals_workspace_bytes(int64_t n, int32_t max_nn)
{
    Arena a(nullptr, 0);
    normals_impl(nullptr, n, 1.0, max_nn < 1 ? 1 : max_nn, nullptr, a, nullptr);
    return a.off;
}
KPX_EXPORT int kpx_estimate_normals(const float *pts, int64_t n, double radius, int32_t max_nn, float *normals, void *ws,
                                    size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(radius > 0.0 && max_nn >= 1, "estimate_normals: radius and max_nn must be positive");
    KPX_REQUIRE(max_nn <= KPX_NORMALS_MAX_NN, "estimate_normals: max_nn > %d is not supported", KPX_NORMALS_MAX_NN);
    KPX_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "kpx_estimate_normals: bad size");
    if (n == 0) return KPX_OK;
    KPX_REQUIRE(pts && normals && ws, "kpx_estimate_normals: null pointer");
    Arena a(ws, ws_bytes);
    return normals_impl(pts, n, radius, max_nn, normals, a, (hipStream_t)stream);
}

// [O3D] PointCloud.estimate_covariances(search_param): per point the covariance of its estimate_normals neighbourhood (same search, same
// ties), E[x x^T] - mu mu^T with divisor m; < 3 neighbours -> the identity.  cov f64 [n][9], symmetric.
KPX_EXPORT size_t kpx_covariances_workspace_bytes(int64_t n, int32_t max_nn) { return kpx_normals_workspace_bytes(n, max_nn); }
KPX_EXPORT int kpx_estimate_covariances(const float *pts, int64_t n, double radius, int32_t max_nn, double *cov, void *ws, size_t ws_bytes,
                                        void *stream)
{
    KPX_REQUIRE(radius > 0.0 && max_nn >= 1, "estimate_covariances: radius and max_nn must be positive");
    KPX_REQUIRE(max_nn <= KPX_NORMALS_MAX_NN, "estimate_covariances: max_nn > %d is not supported", KPX_NORMALS_MAX_NN);
    KPX_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "kpx_estimate_covariances: bad size");
    if (n == 0) return KPX_OK;
    KPX_REQUIRE(pts && cov && ws, "kpx_estimate_covariances: null pointer");
    Arena a(ws, ws_bytes);
    return normals_impl(pts, n, radius, max_nn, nullptr, a, (hipStream_t)stream, cov);
}
