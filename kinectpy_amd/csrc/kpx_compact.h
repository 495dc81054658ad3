// kpx_compact.h -- order-preserving stream compaction: the decoupled look-back, the generic kernel family and its host driver, and
// the launchers of the count scans (kpx_compact.hip).  Included by the translation units that compact or scan counts, by no other.
#pragma once
#include "kpx_common.h"

namespace kpx {

// ---- decoupled look-back (Merrill & Garland): a tile's exclusive prefix without a scan pass ----------------------------
// One 64-bit word per tile, cleared before the launch: bits 63:62 = 0 nothing yet, 1 the tile's own total, 2 its inclusive
// prefix; bits 31:0 = the value.  Flag and value travel in ONE word, so a relaxed device-scope load / store pair is all the
// ordering there is (no fences, no L2 write-backs).  A tile publishes its total, then its first wave walks back over the
// preceding tiles 64 at a time -- lane l reads tile (pos - l) -- until it meets an inclusive prefix.  Tiles are taken in
// blockIdx order (workgroups are dispatched in linear-id order and a resident block never yields), so every predecessor of
// a running tile is running or finished: the spin terminates.
// All threads of the block call it; sh: one int of LDS.  Returns the exclusive prefix of `tile` within its row of states.
constexpr unsigned long long kTileTotal = 1ull << 62, kTilePrefix = 2ull << 62;
__device__ __forceinline__ int lookback_exclusive(unsigned long long *__restrict__ state, int tile, int tot, int *sh)
{
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        if (lane == 0)
            __hip_atomic_store(&state[tile], (tile == 0 ? kTilePrefix : kTileTotal) | (unsigned long long)(unsigned)tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int excl = 0;
        if (tile > 0) {
            int pos = tile - 1;
            for (;;) {
                const int idx = pos - lane;
                unsigned long long st;
                for (;;) {
                    st = idx >= 0 ? __hip_atomic_load(&state[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : kTilePrefix;
                    if (__ballot((st >> 62) == 0ull) == 0ull) break;
                    __builtin_amdgcn_s_sleep(1);
                }
                const unsigned long long pm = __ballot((st >> 62) == 2ull);
                const int first = pm ? __builtin_ctzll(pm) : 64;
                int v = lane <= first ? (int)(unsigned)(st & 0xFFFFFFFFull) : 0;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                excl += v;
                if (pm) break;
                pos -= 64;
            }
            if (lane == 0)
                __hip_atomic_store(&state[tile], kTilePrefix | (unsigned long long)(unsigned)(excl + tot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane == 0) *sh = excl;
    }
    __syncthreads();
    return *sh;
}

// ---- tiles, workspace and the choice of form ----------------------------------------------------------------------------
constexpr int kCompactThreads = 256;
constexpr int kCompactItems = 8;
constexpr int kCompactTile = kCompactThreads * kCompactItems;

// ws_counts of a compaction: int32 [frames * compact_ws_ints(n)] (8-byte aligned: it holds the 64-bit tile states)
static inline int64_t compact_tiles(int64_t n) { return cdiv(n > 0 ? n : 1, kCompactTile); }
static inline int64_t compact_ws_ints(int64_t n) { return 2 * compact_tiles(n) + 2; }
// One pass or three launches?  Measured on MI355X: on batches that stream hundreds of MB the look-back costs bandwidth (every
// tile holds its registers and LDS through a device-scope round trip: 256 frames of depth -> cloud ran at 2.2 TB/s against 3.0
// with count -> scan -> emit), while a frame-sized problem is a chain of launches whose NUMBER is what matters.  So the one-pass
// form serves problems of at most kOnePassTiles tiles; KPX_ONEPASS=0 / 1 forces either path (A/B runs).
constexpr int64_t kOnePassTiles = 2048;
static inline bool use_onepass(int64_t tiles_total)
{
    static const int mode = [] { const char *e = getenv("KPX_ONEPASS"); return e ? (e[0] == '0' ? 0 : 1) : -1; }();
    return mode < 0 ? tiles_total <= kOnePassTiles : mode != 0;
}
// The form of a call and the grid of its kernels: one function per family returns them (px8_plan, kpx_extract.hip; points_plan, kpx_container.hip)
enum class CompactForm { OnePass, OnePassFrameMajor, ThreeLaunch };
struct CompactPlan { CompactForm form; dim3 grid; };
// The generic family and the tile-major grid: blockIdx.x = tile, blockIdx.y = frame.  A one-pass form spins on the states of earlier
// tiles, so it rests on blocks being dispatched in linear order (x fastest): tile t - 1 of a frame is the block just before tile t.
static inline CompactPlan compact_plan(int32_t tiles, int32_t frames) { return { use_onepass((int64_t)tiles * frames) ? CompactForm::OnePass : CompactForm::ThreeLaunch, dim3(tiles, frames) }; }

// ---- the count scans (kernels in kpx_compact.hip: non-template, so they exist once in the library) -----------------------
// one block per frame: exclusive scan of the frame's per-tile counts in place, total -> d_count[frame] (d_count may be NULL)
static inline int compact_scan_threads(int64_t tiles) { return tiles > 2048 ? 1024 : 256; }
void compact_scan(int32_t *counts, int32_t tiles, int32_t frames, int32_t *d_count, hipStream_t st);
// the two lists of one predicate pass (slab split) in one launch: block 0 scans list A, block 1 list B
void compact_scan2(int32_t *counts_a, int32_t *counts_b, int32_t tiles, int32_t *d_count_a, int32_t *d_count_b, hipStream_t st);
// exclusive scan of m 64-bit counts in place, offsets[m] = total: one block (the radius search's per-query counts, the TSDF
// extractions' per-block counts); scan2: two arrays of the same length in one launch
void scan_i64(int64_t *offsets, int64_t m, hipStream_t st);
void scan2_i64(int64_t *a, int64_t *b, int64_t m, hipStream_t st);

// ---- where an emit kernel takes its tile's offset from --------------------------------------------------------------------
// The last launch of count -> scan -> emit and the one-pass kernel of a family are ONE kernel; an Offsets policy is all they differ in.
//   before(): the number of items the frame keeps in front of this tile, whose own total is tot; all threads call it, sh: kLdsInts ints
//   total():  called by all threads with the frame's count up to and including this tile
struct ScannedOffsets {                          // the per-tile counts after compact_scan
    const int32_t *__restrict__ block_offsets;
    static constexpr int kLdsInts = 0, frame_major = 0;          // frame_major: read by the px8 kernel; a scanned launch is tile-major
    __device__ __forceinline__ int before(int frame, unsigned tile, unsigned tiles, int, int *) const { return block_offsets[(int64_t)frame * tiles + tile]; }
    __device__ __forceinline__ void total(int, unsigned, unsigned, int) const {}
};
struct LookbackOffsets {                         // tile states, 64-bit word per (frame, tile), cleared; a frame's last tile writes its count
    unsigned long long *__restrict__ tile_state;
    int32_t *__restrict__ d_count;               // may be NULL
    static constexpr int kLdsInts = 1;
    __device__ __forceinline__ int before(int frame, unsigned tile, unsigned tiles, int tot, int *sh) const { return lookback_exclusive(tile_state + (int64_t)frame * tiles, tile, tot, sh); }
    __device__ __forceinline__ void total(int frame, unsigned tile, unsigned tiles, int sum) const { if (tile == tiles - 1 && threadIdx.x == 0 && d_count) d_count[frame] = sum; }
};

// ---- the generic family ---------------------------------------------------------------------------------------------------
// A Pred is a device functor  bool operator()(int64_t item, int frame) const
// An Emit is a device functor void operator()(int64_t item, int frame, int32_t dst) const
template <class Pred>
__global__ __launch_bounds__(kCompactThreads) void compact_count_kernel(Pred pred, int64_t n, int32_t *block_counts)
{
    __shared__ int sh[kCompactThreads / 64];
    const int frame = blockIdx.y;
    const int64_t base = (int64_t)blockIdx.x * kCompactTile + (int64_t)threadIdx.x * kCompactItems;
    int c = 0;
#pragma unroll
    for (int k = 0; k < kCompactItems; ++k) {
        int64_t i = base + k;
        if (i < n && pred(i, frame)) ++c;
    }
    c = block_sum(c, sh);
    if (threadIdx.x == 0) block_counts[(int64_t)frame * gridDim.x + blockIdx.x] = c;
}
// ScannedOffsets: the third launch, which evaluates the predicate a second time.  LookbackOffsets: ONE pass, the predicate
// evaluated once and the items emitted in place (count -> scan -> emit reads the input twice and costs three launches).
template <class Pred, class Emit, class Offsets>
__global__ __launch_bounds__(kCompactThreads) void compact_emit_kernel(Pred pred, Emit emit, int64_t n, Offsets off)
{
    __shared__ int sh[kCompactThreads / 64 + 1 + Offsets::kLdsInts];
    const int frame = blockIdx.y;
    const unsigned tile = blockIdx.x, tiles = gridDim.x;
    const int64_t base = (int64_t)tile * kCompactTile + (int64_t)threadIdx.x * kCompactItems;
    unsigned flags = 0;
    int c = 0;
#pragma unroll
    for (int k = 0; k < kCompactItems; ++k) {
        int64_t i = base + k;
        if (i < n && pred(i, frame)) { flags |= 1u << k; ++c; }
    }
    int tot;
    const int ex = block_excl_scan(c, sh, &tot);
    const int before = off.before(frame, tile, tiles, tot, sh + kCompactThreads / 64 + 1);
    off.total(frame, tile, tiles, before + tot);          // ahead of the emits: its operands do not stay live through them
    int32_t dst = before + ex;
#pragma unroll
    for (int k = 0; k < kCompactItems; ++k)
        if (flags & (1u << k)) emit(base + k, frame, dst++);
}

// Host driver.  state_is_clear: the caller cleared ws_counts together with a neighbouring region it had to clear anyway (one memset
// dispatch less per call; a frame is a chain of ~5 us dispatches)
template <class Pred, class Emit>
int compact(Pred pred, Emit emit, int64_t n, int32_t frames, int32_t *ws_counts, int32_t *d_count, hipStream_t st, bool state_is_clear = false)
{
    const int32_t tiles = (int32_t)compact_tiles(n);
    const CompactPlan plan = compact_plan(tiles, frames);
    if (plan.form == CompactForm::OnePass) {
        unsigned long long *state = reinterpret_cast<unsigned long long *>(ws_counts);
        if (!state_is_clear) KPX_HIP(hipMemsetAsync(state, 0, (size_t)tiles * frames * sizeof(unsigned long long), st));
        hipLaunchKernelGGL((compact_emit_kernel<Pred, Emit, LookbackOffsets>), plan.grid, dim3(kCompactThreads), 0, st, pred, emit, n,
                           LookbackOffsets{ state, d_count });
    } else {
        hipLaunchKernelGGL(compact_count_kernel<Pred>, plan.grid, dim3(kCompactThreads), 0, st, pred, n, ws_counts);
        compact_scan(ws_counts, tiles, frames, d_count, st);
        hipLaunchKernelGGL((compact_emit_kernel<Pred, Emit, ScannedOffsets>), plan.grid, dim3(kCompactThreads), 0, st, pred, emit, n,
                           ScannedOffsets{ ws_counts });
    }
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

}  // namespace kpx
