// kpx_internal.h -- functions shared between the translation units of libkinectpx.so.
#pragma once
#include "kpx_common.h"

namespace kpx {

// Per-axis min / max of a float32 (n,3) cloud as doubles: d_bbox6 = (minx,miny,minz,maxx,maxy,maxz).
// Exact (min/max need no rounding).  Scratch: bbox_partials_count(n) * 6 doubles.
constexpr int kBboxBlocks = 1024;
int bbox_f32(const float *pts, int64_t n, double *d_bbox6, double *ws_partials, hipStream_t st);

// ---- uniform grid over a cloud (exact neighbour searches: SOR, normals) --------------------------
struct GridParams {
    double org[3];
    double h;
    int32_t dim[3];
    int32_t ncell;
};
constexpr int32_t kGridMaxCells = 1 << 22;

struct Grid {
    GridParams *params;      // device
    uint32_t *cell_start;    // device [kGridMaxCells + 1]
    float *sorted_pts;       // device [n*3] points in cell order
    int32_t *sorted_idx;     // device [n] original index of each sorted point
    uint32_t *sorted_keys;   // device [n] cell id of each sorted point
    int32_t *spare;          // device [16] words cleared by the build, for the caller's counters
    int32_t *extra;          // device [kGridExtraWords] more cleared words (the tile states of a compaction that follows the search)
};
constexpr int kGridExtraWords = 4104;
// Carves a Grid out of the arena (dry arenas only count bytes) and, when real, builds it on `st`.
// target_per_cell: desired mean occupancy of non-empty cells.  fixed_h > 0: cells of that size instead (coarser where the grid would
// outgrow its cell budget or hold fewer than target_per_cell points per cell); no result of any search depends on the cell size.
int grid_build(const float *pts, int64_t n, double target_per_cell, Arena &a, Grid *g, hipStream_t st, double fixed_h = 0.0);

// ---- library-internal lanes ------------------------------------------------------------------------
// Batched entry points run their independent problems (chains of short, latency-bound kernels) side by side on
// kLaneCount internal streams: lanes_fork makes the lanes wait for everything queued on the caller's stream,
// lanes_join makes the caller's stream wait for everything queued on the lanes.  One set per host thread and device,
// created when a call first forks (lanes_get) and held by the thread's ThreadResources.
constexpr int kLaneCount = 4;
constexpr int kLaneDevices = 16;
struct LaneSet {
    hipStream_t s[kLaneCount];
    hipEvent_t fork, join[kLaneCount];      // (fork is created last: non-null = the set is complete)
};
int lanes_get(LaneSet **out);
int lanes_fork(LaneSet *l, hipStream_t caller, int used);
int lanes_join(LaneSet *l, hipStream_t caller, int used);

// ---- what a host thread holds -----------------------------------------------------------------------
// Every host-side HIP resource the library keeps per calling thread lives in ONE thread_local object (kpx_runtime.hip): the pinned
// read-back blocks of the sites below, the lane sets, and the plain counters and caches that go with them.  Its destructor runs when
// the thread ends (a kpx_stream worker: before kpx_stream_destroy's join returns) and gives everything back, ignoring every error
// code -- a runtime that has already shut down must not turn a normal exit into a failure.  kpx_host_resources sums what all
// threads hold.
enum PinnedSite { kPinFrame, kPinVoxelBits, kPinIcpProgress, kPinIcpStates, kPinnedSites };

// kpx_frame_step's memory of "the previous frame of this host thread"
struct FrameLayout {
    float *full_pts, *mask_pts, *mask_col, *down_pts, *normals, *vox_pts, *vox_col;
    int32_t *vox_cnt, *keep_idx;
    double *icp_res, *sor_stats;
    void *op_ws;
    size_t op_bytes;
};
struct FrameState {
    struct { void *ws; size_t bytes; int S; int64_t n_px; FrameLayout L; } carved;      // the layout is a function of these four
    int spec_bits, fuse_spec;              // speculated sort-key widths: registration grids, fused cloud (0 = none)
};

struct ThreadResources {
    void *pin[kPinnedSites] = {};
    size_t pin_bytes[kPinnedSites] = {};
    LaneSet lanes[kLaneDevices] = {};
    unsigned long long frame_seq = 0;      // kPinFrame's completion word: the value the next wait stores
    unsigned long long icp_generation = 0; // kPinIcpProgress: the last call's tag
    FrameState frame = {};
    int32_t *knn_group_word = nullptr;     // the last group pass of this thread (kpx_gridknn.h): its counter word in the caller's workspace,
    int64_t knn_group_given = 0;           // the queries it was given and the stream it ran on -- kpx_knn_group_last
    hipStream_t knn_group_stream = nullptr;
    bool counted = false;                 // this thread is in the "threads holding any" count

    // the site's block, allocated (and zeroed) at first use; nullptr = the allocation failed (the thread's error is set)
    void *pinned(PinnedSite site, size_t bytes) { return pin[site] ? pin[site] : pinned_alloc(site, bytes); }
    ThreadResources() = default;
    ~ThreadResources();
    ThreadResources(const ThreadResources &) = delete;
    ThreadResources &operator=(const ThreadResources &) = delete;
    void *pinned_alloc(PinnedSite site, size_t bytes);
    void hold();
};
ThreadResources &thread_resources();

// kpx_voxel_downsample_batch with a speculated sort-key width (kpx_frame_step): spec_bits > 0 skips the width's read-back (one host
// round trip per call); *d_bits receives the width the batch needs (0 = the call did not speculate) and the caller repeats the call
// with spec_bits = 0 when that is larger than spec_bits.  spec_bits = 0, d_bits = NULL: the exported behaviour.
// morton: the voxels of every cloud leave along the Hilbert curve of their grid indices instead of ascending (ix, iy, iz) -- same
// voxels, same means; for consumers that only need SOME spatially coherent order (the registration inside kpx_frame_step).
int voxel_downsample_batch_spec(int32_t count, const float *const *h_pts, const float *const *h_col, const int64_t *h_n, double voxel,
                                float *const *h_opts, float *const *h_ocol, int32_t *d_counts, void *ws, size_t ws_bytes, void *stream,
                                int spec_bits, int32_t *d_bits, bool morton = false);

// kpx_fuse_voxel_downsample whose transforms may live in device memory: h_dT[i] non-null = cloud i's row-major 4x4 is read there
// (h_T[16 i ..] is then ignored); h_dT == NULL: the exported behaviour.
int fuse_voxel_downsample_dev(int32_t count, const float *const *h_pts, const float *const *h_col, const int64_t *h_n, const double *h_T,
                              const double *const *h_dT, double voxel, float *opts, float *ocol, int32_t *d_count, void *ws, size_t ws_bytes,
                              void *stream, int spec_bits = 0, int32_t *d_bits = nullptr);
// (spec_bits > 0: the keys are taken to fit that many (<= 32) bits and sorted by the library's own radix sort; *d_bits -- pinned host
// memory -- receives the width the cloud really needs: larger than spec_bits = the outputs are garbage, call again with spec_bits = 0)

// kpx_icp_batch for clouds that already lie along a space-filling curve (presorted = true: no Morton sort inside; the culled
// search's tiles are then 16 consecutive points of the caller's order).  presorted = false: the exported behaviour.
// Host threads of this process that are inside a frame step or an ICP batch right now (each thread counted once).  The one-launch ICP
// chain is a LATENCY form: its resident blocks hold wave slots for the whole chain, most of the time waiting; with other frames in
// flight those slots are worth more to the other frames' kernels (two-sensor rig, four frames in flight: 1320 vs 1570-1620 Mpoints/s
// with the chain, profiles/r04/exp_icp_chain_two_sensors.txt), so a chain is admitted only while the calling thread is alone.
struct BusyScope {
    BusyScope();
    ~BusyScope();
    BusyScope(const BusyScope &) = delete;
    BusyScope &operator=(const BusyScope &) = delete;
    bool counted;
};
int busy_threads();
int icp_chain_abort_take();   // 1 if a one-launch ICP chain gave up waiting since the last call (kpx_icp.hip, icp_chain_kernel)
int icp_batch_ordered(int32_t count, const float *const *h_src, const int64_t *h_n_src, const float *tgt, const float *tgt_normals, int64_t n_tgt,
                      double max_dist, const double *h_init, int32_t mode, int32_t max_iteration, double relative_fitness, double relative_rmse,
                      double *d_results, void *ws, size_t ws_bytes, void *stream, bool presorted);

// Column tiles (16 rows x 16 columns, 2048 flops each) the culled nearest-neighbour sweep has multiplied since the
// last call; resets the device counter (kpx_icp.hip).
double nn_local_take_visits();

}  // namespace kpx
