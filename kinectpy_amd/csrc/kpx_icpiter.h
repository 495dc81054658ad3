// kpx_icpiter.h -- one iteration of the culled registration in one kernel: icp_iter_body and the kernels built on it (one
// registration, a batch per launch, the whole chain in one launch), the update kernel of a batch and its init kernel, and the
// profiling words these kernels write.  The __device__ globals live here, so this header belongs to ONE translation unit
// (kpx_icp.hip: the library is built without relocatable device code).
#pragma once
#include "kpx_icpdefs.h"
#include "kpx_fixed.h"
#include "kpx_icpsolve.h"
#include "kpx_nnlocal.h"

namespace kpx {

// ---- one ICP iteration in one kernel (culled engine) -----------------------------------------------------------
// Block = 4 waves x 16 sorted rows.  Prologue: lanes 0..15 of a wave transform their row, seed it and bound it
// with last iteration's partner (clamped to the correspondence distance); the wave sweeps (sweep_wave); lanes 0..15
// then form the chosen pair's direct distance (AC3) and the row's contribution to the update sums, which are added
// in a fixed order per block and added to the exact fixed-point accumulators (a wave ends once its rows' terms are staged; the
// block's last wave to arrive adds them, see s_arrive in icp_iter_body); icp_solve_fixed_kernel performs the
// update step (kpx_icp).  Running the update redundantly in the prologue of the next launch (IcpFuse below) puts the serial
// 6x6 / eigen algebra (~5-8 us) in front of every block's sweep against 5.7 us + 1.9 us for the solve kernel and its
// boundary: for one large registration (100k x 100k: five rounds of blocks per launch) it was 20 % slower, so kpx_icp
// keeps two kernels per iteration; kpx_icp_batch, whose small problems fit one round of blocks and whose chains are
// bound by the host's launch rate, uses the one-launch form.
// ("Last block finishes the job" inside this launch was measured twice and lost both times: with plain stores +
// __threadfence() the release writes back / invalidates the XCD's L2 once per block (10x slower); with write-through
// device-scope stores, a drained vmcnt and a relaxed ticket it still adds ~13 us at 485 blocks -- the same-address
// ticket atomics serialise at ~12 ns each and the last block reads 170 KB through sc1 loads -- against ~11 us for
// the boundary + the 1024-thread solve kernel.)
constexpr int kIRows = kIWaves * kLRows;
// One launch per iteration (used by kpx_icp_batch, whose chains are bound by the host's launch rate once several
// registrations and two frames run side by side): launch k first performs the update of iteration k-1 -- every block
// folds the accumulator set of the previous launch and runs the (deterministic) algebra itself, block 0 publishes the
// state, the result and the progress word -- then sweeps with the new transform.  Three accumulator sets in a ring
// (launch k reads set k-1, adds to set k, block 0 clears set k+1) and two state slots (launch k reads slot k-1, writes
// slot k) keep the launches free of races.  pair == nullptr: two-kernel mode, icp_solve_fixed_kernel does the update.
constexpr int kCertHist = 64;                 // iterations whose transforms are kept for the certificates (6 bits of the word)
// The whole chain in ONE launch (icp_chain_kernel): the blocks of a registration stay resident and iterate; the hand-off between
// iterations is a RECORD per iteration -- the registration's state as the update of iteration k - 1 left it -- whose 23 words the
// winner (the block that drew the last ticket) writes with device-coherent stores and wave 0 of every block polls with
// device-coherent loads, each lane ITS word, until none of them is the "empty" pattern any more (a NaN payload no computation
// produces): every word validates itself, so there is no flag, no release and no second round trip.
constexpr int kChainRec = 32;                 // doubles per record (23 used)
constexpr int kChainRecords = 64;             // records 0 .. max_iteration + 1: the chain form serves max_iteration <= 62
constexpr int kChainWords = 24;                // = sizeof(IcpState) / 8
constexpr unsigned long long kChainEmpty = 0xFFF8C0DEC0DEC0DEull;
constexpr int kAccSet = kAccCopies * kAcc * kFixedWords;
// Phase clock of the iteration kernel (while the profiler is armed): thread 0 of every block stores 100 MHz wall-clock stamps in
// its own row of g_icp_stamp -- [0] block start, [1] after the update prologue, [2] after row preparation, [3] after the culled
// sweep, [4] after the pair epilogue, [5] block end ([4] and [5] of the block form: lane 0 of the wave that closes the block, so [4] is
// the arrival of the block's last wave).  Plain stores to private slots: the clock does not disturb what it times.
// The rows of the LAST launch are read by kpx_prof_icp_phases.
constexpr int kStampBlocks = 4096;
__device__ unsigned long long g_icp_stamp[kStampBlocks][8];
// per WAVE of the last sweep launch: [0] sweep start, [1] sweep end (100 MHz), [2] the packed counters sweep_wave returns, [3] rows
// of the wave that ended with a partner
__device__ unsigned long long g_icp_wave[kStampBlocks * 4][4];
// Certificate self-check (KPX_ICP_CERT_CHECK=1): certified rows are searched all the same and the search's winner is compared with the
// partner the certificate kept.  [0] rows certified, [1] rows searched, [2] certified rows whose search disagreed, [3..7] the first
// disagreement: iteration, sorted row, kept partner, found partner, key as float bits.  Read (and cleared) by kpx_prof_icp_cert.
__device__ unsigned long long g_cert_check[8];
// Clock of the one-launch chain (KPX_ICP_CHAIN_STAMPS=1, first registration of the launch; 100 MHz stamps, one row per iteration):
// block 0: [0] record seen, [1] rows prepared, [2] sweep over, [3] sums added, [4] ticket drawn; over all blocks: [5] latest / [10]
// earliest "record seen", [11] latest "sums added", [6] latest ticket; the winner: [7] totals read, [8] update done, [9] record published.
__device__ unsigned long long g_chain_stamp[64][48];    // [32 ..]: the winner's update step from inside (icp_finish_wave, tick)    // [16 ..]: block 0 wave 0's sweep (sweep_wave, dbg_tick)
__device__ __forceinline__ void chain_tick(unsigned long long *row, int slot, bool on)
{
    if (row && on) row[slot] = wall_clock64();
}
__device__ __forceinline__ void phase_tick(unsigned long long *__restrict__ armed, int slot, unsigned bid)
{
    if (!armed || threadIdx.x || bid >= kStampBlocks) return;
    __builtin_nontemporal_store(wall_clock64(), &g_icp_stamp[bid][slot]);
}
// ... by lane 0 of whichever wave is at that point (the block-end stamps of the block form: the wave that closes the block)
__device__ __forceinline__ void phase_tick_wave(unsigned long long *__restrict__ armed, int slot, unsigned bid, int lane)
{
    if (!armed || lane || bid >= kStampBlocks) return;
    __builtin_nontemporal_store(wall_clock64(), &g_icp_stamp[bid][slot]);
}
// Rows of the sums' staging array `sh` in the block form: only the slots that are live in SOME mode of the culled engine have one,
// by a dense index -- slots 0..16 as they are, the plane slots 17..43 moved down onto the point slots 2..16 they never share a launch
// with.  In either mode the live slots then are the dense rows 0 .. acc_dense_live - 1, in slot order.
constexpr int kAccDense = 2 + (kAcc - 17);    // 29 rows instead of 44
static_assert(kAccDense >= 17, "the point-to-point slots 0..16 fit");
__host__ __device__ constexpr int acc_dense(int slot) { return slot < 17 ? slot : slot - 15; }
__host__ __device__ constexpr int acc_dense_live(bool plane) { return plane ? kAccDense : 17; }
__host__ __device__ constexpr int acc_dense_slot(bool plane, int row) { return row < 2 ? row : row - 2 + acc_lo(plane); }
static_assert(acc_dense(acc_dense_slot(true, 28)) == 28 && acc_dense(acc_dense_slot(false, 16)) == 16 && acc_dense_slot(true, 2) == 17, "dense rows <-> slots");
// Certificates: rows whose partner provably cannot change are not searched again.
// A sweep knows more than the winner: every column it multiplied gives D, every box it culled was farther than the row's culling
// bound.  L = sqrt(min(final culling bound, smallest D - 1 among the multiplied columns OTHER than the winner)) is therefore a lower
// bound of the distance from the row to every other target point.  The row keeps (p_c, L): its position at that search and L.  In a
// later iteration it stands at p, every other target is still >= L - |p - p_c| away (triangle inequality, the row's OWN displacement:
// no global bound), and if the partner's own (exactly evaluated) distance d1 is smaller than that -- d1 + |p - p_c| < L, with margins
// for the float32 copy of p_c and the roundings -- the partner is the STRICT nearest neighbour: an exact search would return it, ties
// and all, so the row keeps it without one.  Rows without a partner use the reach of any row's search in place of d1.  A certificate
// is worth something only if the search looked beyond its partner: once the registration is calm (the last update moved no point by
// more than `calm` x the correspondence distance; IcpState::last_motion, LightSkip's bookkeeping) uncertified rows are searched with a
// skin around their partner, `factor` x that motion (between `smin` and `smax` x the correspondence distance): a few more tiles
// multiplied once, no search at all in the iterations that follow.  Waves whose 16 rows are all certified skip the sweep, the others
// cull with the box and bounds of their uncertified rows only.  Partners, sums and transforms are those of the full search, bit for
// bit.  The policy is CertPolicy, above IcpFuse.  (KPX_ICP_CERT=0 switches the certificates off: test_icp_update_placements_and_light_skip_are_bit_identical; KPX_ICP_CERT_CHECK=1
// searches the certified rows all the same and counts disagreements: test_icp_certificates_never_contradict_the_search).
//
// The pieces every form of the iteration shares (icp_iter_body below, icp_rows_kernel in kpx_icprows.h), one definition each:
// how calm the registration is decides the skin uncertified rows are searched with (0: none)
__device__ __forceinline__ double cert_skin(bool certs, int k, const IcpState *st, double max_d2, const CertPolicy &pol)
{
    double c_skin = 0.0;
    if (certs && k > 0) {
        const double lm = st->last_motion, md = sqrt(max_d2);
        if (lm <= (double)pol.calm * md) c_skin = fmin(fmax((double)pol.factor * lm, (double)pol.smin * md), (double)pol.smax * md);
    }
    return c_skin;
}
// The certificate test of a row: s its position now, src its coordinates, (prev, pt) the partner it came with, bj what row_bound left
// of that partner, cert its certificate word, Th the 12 doubles of the transform of the iteration the word names (read only where the
// word holds an L), c_reach the reach of any row's search.  Returns whether the row is certified, and sets the bound rb0 it is searched
// with: none (-1) for a certified row outside the self-check, else widened by the skin.
__device__ __forceinline__ bool cert_test(const double s[3], const float src[3], int32_t prev, const float pt[3], int32_t bj, uint32_t cert, const double *Th,
                                          double c_reach, double c_skin, int cert_check, double &rb0)
{
    // d1: an upper bound of the distance from the row to its partner (a row without one: the reach of any row's search)
    double d1 = c_reach;
    if (bj != INT_MAX) {
        const double dx = s[0] - (double)pt[0], dy = s[1] - (double)pt[1], dz = s[2] - (double)pt[2];
        d1 = sqrt(fma(dz, dz, fma(dy, dy, dx * dx))) * (1.0 + 1e-12);
    }
    // certified: every other target point was >= L away from p_c, the row has moved by |p - p_c| since (p_c is kept as float32:
    // 2^-24 relative per coordinate, covered by the 1e-6 relative margin on the coordinates' scale), and its partner (or the
    // reach of a row without one) is nearer than what is left of L.  A row that HAD a partner and lost it to the clamp is
    // searched (the certificate says nothing about that partner).
    const bool keeps = (prev >= 0) == (bj != INT_MAX);
    const float Lc = __uint_as_float(cert & ~63u);
    double pc[3] = { 0.0, 0.0, 0.0 };
    if (Lc > 0.0f) {                                     // the row's position at that search: AC1 with that iteration's transform
        const double x = src[0], y = src[1], z = src[2];
#pragma unroll
        for (int a = 0; a < 3; ++a) pc[a] = fma(Th[4 * a], x, fma(Th[4 * a + 1], y, fma(Th[4 * a + 2], z, Th[4 * a + 3])));
    }
    const double ex = s[0] - pc[0], ey = s[1] - pc[1], ez = s[2] - pc[2];
    const double moved = sqrt(fma(ez, ez, fma(ey, ey, ex * ex))) * (1.0 + 1e-12);
    const bool certd = Lc > 0.0f && keeps && (d1 + moved) * (1.0 + 1e-6) + 1e-6 < (double)Lc;
    if (certd && !cert_check) rb0 = -1.0;
    else if (c_skin > 0.0) { const double rr = d1 + c_skin; rb0 = fmax(rb0, rr * rr); }
    return certd;
}
// The new certificate word of a row that was searched in iteration k, from what the sweep left in WaveRows (sec, eps_out, rb_out):
// L^2 = min(final culling bound, runner-up among the multiplied columns), both on d^2; L rounded DOWN to a float with its low six
// mantissa bits cleared; those bits carry the iteration (k < 64: later iterations of a longer chain are searched every time)
__device__ __forceinline__ uint32_t cert_word(unsigned sec, double eps_out, double rb_out, int k)
{
    typedef unsigned uu2 __attribute__((ext_vector_type(2)));
    const uu2 pat = { 0u, sec };
    const double d2nd = sec == 0xFFFFFFFFu ? INFINITY : __builtin_bit_cast(double, pat) - 1.0 - eps_out;
    const double l2 = fmin(rb_out, d2nd);
    const uint32_t lb = l2 > 0.0 && k < kCertHist ? (__float_as_uint(f32_down(sqrt(l2) * (1.0 - 1e-7))) & ~63u) : 0u;
    return lb > 63u ? (lb | (uint32_t)k) : 0u;
}
// Self-check bookkeeping (g_cert_check): the search of a certified row disagreed with the partner its certificate kept -- the first
// such row is recorded
__device__ __forceinline__ void cert_check_disagreement(int k, int64_t row, int32_t kept, int32_t found, uint32_t word)
{
    if (atomicAdd(&g_cert_check[2], 1ull) == 0ull) {
        g_cert_check[3] = (unsigned long long)k; g_cert_check[4] = (unsigned long long)row;
        g_cert_check[5] = (unsigned long long)(unsigned)kept; g_cert_check[6] = (unsigned long long)(unsigned)found;
        g_cert_check[7] = (unsigned long long)(word & ~63u);
    }
}
// ... and per wave of rows the counters (one lane calls); `first`: the registration's first wave, which reports the chain's state
// at its last launch in [3..7] as long as there is no disagreement
__device__ __forceinline__ void cert_check_count(bool first, int k, const IcpState *st, double c_skin, int certified, int searched)
{
    if (first && g_cert_check[2] == 0ull) {
        g_cert_check[3] = (unsigned long long)k; g_cert_check[4] = __builtin_bit_cast(unsigned long long, st->last_motion);
        g_cert_check[5] = __builtin_bit_cast(unsigned long long, st->motion); g_cert_check[6] = __builtin_bit_cast(unsigned long long, c_skin);
    }
    atomicAdd(&g_cert_check[0], (unsigned long long)certified);
    atomicAdd(&g_cert_check[1], (unsigned long long)searched);
}
// IcpFuse of the ticket mode for a problem of a batch: the last block of the registration's sweep performs the update (ticket: first
// word of the second accumulator set).  light: the switch word (icp_light_word, kpx_icp.hip)
__device__ __forceinline__ IcpFuse ticket_fuse(const IcpProblem &P, int max_iter, double rel_fit, double rel_rmse, unsigned long long tag, int light,
                                               CertPolicy pol, double *chain_rec, unsigned long long *stamp)
{
    return IcpFuse{ (IcpState *)nullptr, P.ring, max_iter, rel_fit, rel_rmse, P.result, P.progress, tag, P.ring + kAccSet,
                    (light & 1) ? P.light_key : (double *)nullptr, P.sbbox, (light & 2) ? P.cert : (uint32_t *)nullptr,
                    (light & 2) ? P.thist : (double *)nullptr, (light & 4) ? 1 : 0, pol, chain_rec, stamp };
}
// The winner's step (the block that drew its registration's last ticket, THREADS threads, tix_w the caller's thread number behind an
// opaque move), first part: the coherent totals of the mode's live slots into s_sums (0.0 for the others, without a load), the searched-row count (SEARCHED; returned), then -- the block's
// s_sums complete -- the accumulators cleared and the ticket reset for the next launch.
template <int THREADS, bool SEARCHED>
__device__ __forceinline__ unsigned long long winner_take(unsigned long long *acc, unsigned long long *ticket, bool plane, double *s_sums, int tix_w)
{
    if (tix_w < kAcc) s_sums[tix_w] = acc_live(plane, tix_w) ? fixed_total_coherent(acc, tix_w) : 0.0;
    const unsigned long long n_searched = SEARCHED ? searched_take(ticket, tix_w) : 0ull;
    if (THREADS > 64) __syncthreads(); else wave_lds_fence();
    for (int e = tix_w; e < kAccSet; e += THREADS) __hip_atomic_store(acc + e, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tix_w == 0) __hip_atomic_store(ticket, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return n_searched;
}
// ... last part, by the first 24 lanes of the wave that ran the update on `work` (every form but the one-launch chain, which
// publishes a record instead): the state written back, entry k + 1 of the transforms' history (thist, or nullptr without
// certificates), the progress word.  Plain stores: the readers are the blocks of the NEXT launch, behind the kernel boundary.
__device__ __forceinline__ void winner_publish(IcpState *st, const IcpState *work, double *thist, int k, unsigned long long *progress, unsigned long long tag,
                                               unsigned long long n_searched, int64_t n, int lane)
{
    if (lane < (int)(sizeof(IcpState) / sizeof(double))) reinterpret_cast<double *>(st)[lane] = reinterpret_cast<const double *>(work)[lane];
    if (thist && k + 1 < kCertHist && lane < 12) thist[12 * (k + 1) + lane] = work->T[lane];     // what iteration k + 1 transforms with
    if (lane == 0 && progress)
        __hip_atomic_store(progress, tag | progress_searched(n_searched, n) | ((unsigned long long)(work->done ? 1 : 0) << 32) | (unsigned long long)(unsigned)(k + 1),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// bid / nblocks: this block's index among the blocks of ITS registration (one launch may carry several, see icp_iter_batch_kernel)
template <bool PERSIST = false>
__device__ __forceinline__ void icp_iter_body(const unsigned bid, const unsigned nblocks, const float *__restrict__ src, int64_t n, const float *__restrict__ tgt,
                                                       const float *__restrict__ tn, const double *__restrict__ Bs,
                                                       const int32_t *__restrict__ orig, const float *__restrict__ tile_box,
                                                       const float *__restrict__ group_box, int32_t n_groups,
                                                       const double *__restrict__ tbbox, const int32_t *__restrict__ row_of,
                                                       const float *__restrict__ src_sorted, int32_t *__restrict__ idx_sorted,
                                                       float *__restrict__ ptgt_sorted,
                                                       int32_t *__restrict__ idx_cur, double *__restrict__ d2_cur, double max_d2, int mode,
                                                       int k, const IcpState *__restrict__ st, unsigned long long *acc,
                                                       unsigned long long *__restrict__ tile_visits, IcpFuse fuse)
{
    // (chain form: the thread number behind an opaque move, taken anew in every iteration -- otherwise everything derived from it,
    // LDS addresses first of all, is hoisted out of the chain's loop and held in registers this kernel does not have)
    const unsigned tix = PERSIST ? (unsigned)opaque_i((int)threadIdx.x) : threadIdx.x;
    __shared__ IcpState s_state;
    __shared__ double s_sums[kAcc];
    // PERSIST (icp_chain_kernel: this body runs once per iteration inside ONE launch, `st` is the block's LDS copy of the iteration's
    // record): what a row carries from one iteration to the next -- its coordinates, its partner (index, coordinates, normal), its
    // certificate, the block's LightSkip key -- stays in LDS; nothing but constants is read from memory after iteration 0.
    __shared__ float rowk[kIWaves][16][8];           // what a row carries across the sweep (its previous partner: coordinates, normal, index),
                                                     // parked here: a value in 16 lanes costs a whole register through the multiply loop
    __shared__ float rowsrc[kIWaves][16][3];
    __shared__ uint32_t rowc[kIWaves][16];
    __shared__ int32_t rowi[kIWaves][16][2];         // partner (bound / result), original row
    __shared__ double s_key;
    const int wave = PERSIST ? __builtin_amdgcn_readfirstlane((int)(tix >> 6)) : (int)(tix >> 6), lane = tix & 63, q = lane >> 4, j = lane & 15;
    const int64_t row_base = ((int64_t)bid * kIWaves + wave) * kLRows;
    const int64_t last = n - 1;
    const unsigned long long t_block_start = (tile_visits && tix == 0) ? wall_clock64() : 0ull;
    const double t2max = target_t2max(tbbox);
    // An iteration is a chain of dependent memory round trips, so everything that does not depend on this iteration's
    // transform is requested FIRST -- the wave's rows, their previous partners (index AND coordinates, kept in sorted-row
    // order by the previous launch: no gather through the index), the first 128 group boxes -- and arrives while the update
    // algebra of the previous iteration runs below.
    float my_src[3] = { 0.0f, 0.0f, 0.0f }, my_pt[3] = { 0.0f, 0.0f, 0.0f }, my_nrm[3] = { 0.0f, 0.0f, 0.0f };
    int32_t my_row = 0, my_prev = -1;
    uint32_t my_cert = 0u;
    const bool certs = fuse.ticket && fuse.light_key && fuse.cert;
    if (PERSIST && k > 0) {
        if (lane < 16) {
            my_row = rowi[wave][lane][1];
#pragma unroll
            for (int a = 0; a < 3; ++a) { my_src[a] = rowsrc[wave][lane][a]; my_pt[a] = rowk[wave][lane][a]; my_nrm[a] = rowk[wave][lane][3 + a]; }
            my_prev = __float_as_int(rowk[wave][lane][6]);
            if (certs) my_cert = rowc[wave][lane];
        }
    } else if (lane < 16) {
        const int64_t r = row_base + lane < last ? row_base + lane : last;
        if (idx_cur || d2_cur) my_row = row_of[r];           // only the caller-order outputs need the original row number
#pragma unroll
        for (int a = 0; a < 3; ++a) my_src[a] = src_sorted[3 * r + a];
        if (PERSIST) {
#pragma unroll
            for (int a = 0; a < 3; ++a) rowsrc[wave][lane][a] = my_src[a];
            rowc[wave][lane] = 0u;
        }
        if (k > 0) {
            my_prev = idx_sorted[r];
#pragma unroll
            for (int a = 0; a < 3; ++a) my_pt[a] = ptgt_sorted[3 * r + a];
            if (certs) my_cert = fuse.cert[r];
        }
    }
    // (certificates) the transforms of the iterations so far: a certified row's position at its search is recomputed from them, exactly
    __shared__ double s_thist[kCertHist][12];
    if (PERSIST) {                                        // (the earlier entries are still there; a barrier follows before the rows use them)
        if (certs && k < kCertHist && tix < 12) s_thist[k][tix] = st->T[tix];
    } else if (certs && k > 0)
        for (int e = tix; e < 12 * (k < kCertHist ? k : kCertHist); e += kIThreads) (&s_thist[0][0])[e] = fuse.thist[e];
    GroupPre gpre;
    group_pre_load(gpre, group_box, n_groups, lane);
    if (!PERSIST && mode == 1 && k > 0 && lane < 16) {
        // the previous partner's normal, requested through the index as soon as that has arrived (behind everything that does not
        // depend on anything): it is not needed before the pair epilogue, where an unchanged partner -- the rule in the late
        // iterations -- then costs no round trip at all
        const float *np_ = tn + 3 * (int64_t)(my_prev > 0 ? my_prev : 0);
#pragma unroll
        for (int a = 0; a < 3; ++a) my_nrm[a] = np_[a];
    }
    const double *Tk = st->T;
    // (ticket mode) the registration's state, copied into LDS while everything else loads: the block that draws the last ticket runs the
    // update step on this copy -- fitness / rmse / T / motion were four dependent global round trips inside a step that every launch waits
    // for -- and writes the new state back in one burst
    static_assert(sizeof(IcpState) % sizeof(double) == 0, "IcpState is copied as doubles");
    if (fuse.ticket && tix < sizeof(IcpState) / sizeof(double))
        reinterpret_cast<double *>(&s_state)[tix] = reinterpret_cast<const double *>(st)[tix];
    if (fuse.pair) {
        const IcpState *in = fuse.pair + ((k + 1) & 1);
        IcpState *out = fuse.pair + (k & 1);
        // state and accumulators are read in ONE round trip (the sums of a converged chain are simply not used)
        const unsigned long long *prev = fuse.ring + (int64_t)((k + 2) % 3) * kAccSet;
        if (k > 0 && tix < kAcc) s_sums[tix] = acc_live(mode == 1, (int)tix) ? fixed_total(prev, tix) : 0.0;
        if (tix == 0) s_state = *in;
        __syncthreads();
        if (s_state.done) {                               // converged earlier: hand the state on, nothing else to do
            if (bid == 0 && tix == 0) *out = s_state;
            return;
        }
        __shared__ FinishScratch s_fs;
        if (k > 0 && wave == 0)
            icp_finish_wave(s_sums, n, mode, k - 1, fuse.max_iter, fuse.rel_fit, fuse.rel_rmse, &s_state, bid == 0 ? fuse.result : (double *)nullptr,
                            s_fs, lane);
        __syncthreads();
        if (bid == 0) {
            unsigned long long *next = fuse.ring + (int64_t)((k + 1) % 3) * kAccSet;
            for (int e = tix; e < kAccSet; e += kIThreads) next[e] = 0ull;
            if (tix == 0) {
                *out = s_state;
                if (k > 0 && fuse.progress)
                    __hip_atomic_store(fuse.progress, fuse.tag | ((unsigned long long)(s_state.done ? 1 : 0) << 32) | (unsigned long long)(unsigned)k,
                                       __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        if (s_state.done) return;
        Tk = s_state.T;
        acc = fuse.ring + (int64_t)(k % 3) * kAccSet;
    } else if (st->done) return;
    // LightSkip: nothing of this block can have come within reach since it was last swept -> straight to the ticket
    bool skip = false;
    if (fuse.ticket && fuse.light_key) {
        const double key = PERSIST ? (k > 0 ? s_key : 0.0) : fuse.light_key[bid];
        skip = key > 0.0 && (st->motion + st->reach) * (1.0 + 1e-6) + 1e-6 < key;
    }
    __shared__ double s_light[kIWaves];
    const int nacc = mode == 1 ? kAcc : 17;
    if (tile_visits && tix == 0 && bid < kStampBlocks) { g_icp_stamp[bid][7] = skip ? 1ull : 0ull; g_icp_stamp[bid][6] = (unsigned long long)nblocks; }
    // The block form (!PERSIST; icp_iter_kernel, icp_iter_batch_kernel): a wave ENDS with its 16 rows.  It stages their contributions
    // (sh, s_cnt, s_light) and adds 1 to s_arrive with a returning LDS add; the wave whose add returns kIWaves - 1 -- the last to
    // arrive -- closes the block alone, on its lane number: the tile trees and the exact adds, the LightSkip key, the ticket and, as
    // winner, the update.  The others return there and give their registers and wave slot back while the block's slowest wave still
    // sweeps; nobody waits at a barrier.  The LDS operations of a CU are performed in issue order: behind its own returning add the
    // closing wave sees everything the others staged in front of theirs (wave 0's copy of the state in s_state as well, which is in
    // front of the barrier below).  No barrier may follow the arrival point: the closing wave runs straight-line code.  The uniform
    // early ways out follow the same rule: every wave but one returns, one draws the ticket.
    // The one-launch chain (PERSIST) keeps its four waves and its barriers: its blocks iterate, nothing may leave.
    __shared__ unsigned s_arrive;
    do {
    if (skip) {
        if (!PERSIST && wave != 0) return;
        break;
    }
    __shared__ int32_t lists[kIWaves][kLScratch];
    __shared__ double rowd[kIWaves][16][kRowStride]; // s_x, s_y, s_z, (the sweep's row bound), K, bound / result value
    __shared__ float rowf[kIWaves][16][kRowFStride]; // float32 mirror of the rows for the sweep's culling tests
    constexpr int kShRows = PERSIST ? kAcc : kAccDense;
    __shared__ double sh[kShRows][kIRows + 1];               // (block form: a row per dense index, acc_dense)
    auto sh_row = [](int slot) { return PERSIST ? slot : acc_dense(slot); };
    if (tile_visits && tix == 0 && bid < kStampBlocks) {     // only launches that sweep stamp (not the converged / closing ones)
        g_icp_stamp[bid][0] = t_block_start;
        g_icp_stamp[bid][6] = (unsigned long long)nblocks;
    }
    phase_tick(tile_visits, 1, bid);
    // s_thist was staged by all threads of the block and is read by the rows of every wave (until this barrier was added the
    // per-launch form relied on the waves of a block running in step: a row could read an entry before another wave had written it)
    // (block form: the arrival counter is cleared behind the same barrier, which all waves pass before any of them can arrive)
    if (!PERSIST && kIWaves > 1 && tix == 0) s_arrive = 0u;
    if ((!PERSIST && kIWaves > 1) || (certs && (k > 0 || PERSIST))) __syncthreads();
    if (PERSIST && fuse.stamp && tix == 0) {
        const unsigned long long t = wall_clock64();
        if (bid == 0) fuse.stamp[0] = t;
        atomicMax(&fuse.stamp[5], t);
        atomicMin(&fuse.stamp[10], t);
    }

    // Row certificates (kpx_icp.hip, "Certificates" above icp_iter_body): how calm the registration is decides the skin
    const double c_reach = certs ? st->reach : 0.0;
    const double c_skin = cert_skin(certs, k, st, max_d2, fuse.pol);
    bool my_active = true, my_certd = false;
    if (lane < 16) {
        const int64_t i = my_row;
        double s[3];
        xform_row(Tk, my_src, s);
        const double seed = row_seed(s);
        double bv = INFINITY;
        int32_t bj = INT_MAX;
        if (k > 0 && my_prev >= 0) { bv = partner_bound(s, seed, my_pt); bj = my_prev; }
        bound_clamp(seed, max_d2, t2max, bv, bj);
        double rb0 = bv - 1.0;
        if (certs) {
            const bool certd = cert_test(s, my_src, my_prev, my_pt, bj, my_cert, s_thist[my_cert & 63u], c_reach, c_skin, fuse.cert_check, rb0);
            my_active = (!certd || fuse.cert_check) && row_base + lane <= last;
            my_certd = certd && row_base + lane <= last;
        }
        rowd[wave][lane][0] = s[0]; rowd[wave][lane][1] = s[1]; rowd[wave][lane][2] = s[2];
        rowd[wave][lane][3] = rb0;
        rowd[wave][lane][4] = seed; rowd[wave][lane][5] = bv;
        rowi[wave][lane][0] = bj; rowi[wave][lane][1] = (int32_t)i;
#pragma unroll
        for (int a = 0; a < 3; ++a) { rowk[wave][lane][a] = my_pt[a]; rowk[wave][lane][3 + a] = my_nrm[a]; }
        rowk[wave][lane][6] = __int_as_float(my_prev);
    }
    if (PERSIST && fuse.stamp) {          // who is searched, and why (chain clock: [26] waves, [27] rows, [28] rows without partner, [29] rows without certificate)
        const bool searched = lane < 16 && my_active && !my_certd;
        const unsigned long long sm = __builtin_amdgcn_ballot_w64(searched);
        const unsigned long long np = __builtin_amdgcn_ballot_w64(searched && my_prev < 0);
        const unsigned long long nc = __builtin_amdgcn_ballot_w64(searched && (my_cert & ~63u) == 0u);
        if (lane == 0 && sm) {
            atomicAdd(&fuse.stamp[26], 1ull); atomicAdd(&fuse.stamp[27], (unsigned long long)__builtin_popcountll(sm));
            atomicAdd(&fuse.stamp[28], (unsigned long long)__builtin_popcountll(np)); atomicAdd(&fuse.stamp[29], (unsigned long long)__builtin_popcountll(nc));
        }
    }
    const unsigned act_mask = (unsigned)(__builtin_amdgcn_ballot_w64(lane < 16 && my_active) & 0xFFFFull);
    const unsigned certd_mask = (unsigned)(__builtin_amdgcn_ballot_w64(lane < 16 && my_certd) & 0xFFFFull);
    wave_lds_fence();
    WaveRows w;
    w.a = q < 3 ? rowd[wave][j][q] : 1.0;
    w.rows = &rowd[wave][0][0];
    w.rowsf = &rowf[wave][0][0];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int rr = q + 4 * r;
        w.seed[r] = rowd[wave][rr][4];
        w.best[r] = rowd[wave][rr][5];
        w.bcol[r] = rowi[wave][rr][0];
        w.rb0[r] = rowd[wave][rr][3];
    }
    w.skin = c_skin;
    w.act_mask = act_mask;
    w.light_gap2 = -1.0;
    w.dbg = (PERSIST && fuse.stamp && bid == 0 && wave == 0) ? fuse.stamp + 16 : (unsigned long long *)nullptr;
    phase_tick(tile_visits, 2, bid);
    if (PERSIST) chain_tick(fuse.stamp, 1, bid == 0 && tix == 0);
    const unsigned long long t_sweep = tile_visits ? wall_clock64() : 0ull;
    unsigned long long swept = 0ull;
    int lane_p = 0, wave_p = 0, q_p = 0, j_p = 0;
    int64_t row_base_p = 0;
    auto rederive = [&]() {
        lane_p = opaque_i((int)(threadIdx.x & 63)); wave_p = opaque_i((int)(threadIdx.x >> 6)); q_p = lane_p >> 4; j_p = lane_p & 15;
        row_base_p = ((int64_t)bid * kIWaves + wave_p) * kLRows;
    };
    if (act_mask != 0u) {                                 // (a wave whose 16 rows are all certified keeps what it came with)
        wave_lds_fence();                                 // rowd[..][3] is the sweep's own slot from here on
        swept = sweep_wave<true, true, PERSIST>(w, Bs, orig, tile_box, group_box, n_groups, t2max, lists[wave], &gpre);
        rederive();
        // new keys for the rows that were searched: L^2 = min(final culling bound, runner-up among the multiplied columns), both on d^2
        if (certs && fuse.cert_check && j_p == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rr = q_p + 4 * r;
                if (((certd_mask >> rr) & 1u) != 0u && w.bcol[r] != rowi[wave_p][rr][0])
                    cert_check_disagreement(k, row_base_p + rr, rowi[wave_p][rr][0], w.bcol[r], PERSIST ? rowc[wave_p][rr] : fuse.cert[row_base_p + rr]);
            }
        }
        if (certs && j_p == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rr = q_p + 4 * r;
                if (((act_mask >> rr) & 1u) != 0u && ((certd_mask >> rr) & 1u) == 0u) {
                    const uint32_t cw = cert_word(w.sec[r], w.eps_out, w.rb_out[r], k);
                    if (PERSIST) rowc[wave_p][rr] = cw; else fuse.cert[row_base_p + rr] = cw;
                }
            }
        }
    }
    if (act_mask == 0u) rederive();
    // how much of the registration is still searched: what the host picks the next launches' form by (icp_rows_kernel once most rows
    // carry a certificate).  One returning add per BLOCK into one of eight words behind the ticket (kSearchedWord: same-address atomics
    // serialise at ~12 ns each -- one word per registration cost 20 us per launch), waited for like the sums' adds.
    __shared__ int s_cnt[kIWaves];
    if (lane_p == 0) s_cnt[wave_p] = __builtin_popcount(act_mask & ~certd_mask);
    const unsigned visited = (unsigned)(swept & 0xFFFFu);
    if (certs && fuse.cert_check && lane_p == 0)
        cert_check_count(bid == 0 && wave_p == 0, k, st, c_skin, __builtin_popcount(certd_mask), __builtin_popcount(act_mask & ~certd_mask));
    // (LightSkip speaks for ALL rows of a block: a wave that left certified rows out of its box does not count as light)
    if (lane_p == 0) s_light[wave_p] = act_mask == 0xFFFFu ? w.light_gap2 : -1.0;
    if (tile_visits && lane_p == 0 && bid < kStampBlocks && kIWaves <= 4) {
        unsigned long long *o = g_icp_wave[bid * 4 + wave_p];
        int with = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) with += (w.bcol[r] >= 0 && w.bcol[r] != INT_MAX) ? 1 : 0;      // lane 0: rows 0, 4, 8, 12 (a sample)
        o[0] = t_sweep; o[1] = wall_clock64(); o[2] = swept; o[3] = (unsigned long long)with;
    }
    phase_tick(tile_visits, 3, bid);
    if (PERSIST) chain_tick(fuse.stamp, 2, bid == 0 && lane_p == 0 && wave_p == 0);
    if (PERSIST && fuse.stamp && bid == 0 && lane_p == 0 && wave_p == 0) { fuse.stamp[13] = swept; fuse.stamp[14] = (unsigned long long)act_mask | ((unsigned long long)certd_mask << 16); }
    if (tile_visits && lane_p == 0) atomicAdd(tile_visits + ((bid * kIWaves + wave_p) & (kVisitSlots - 1)), (unsigned long long)visited);
    wave_lds_fence();
    if (j_p == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) rowi[wave_p][q_p + 4 * r][0] = w.bcol[r];
    }
    wave_lds_fence();

    // the chosen pairs: direct distance, contribution to the sums (one row per lane 0..15)
    // (lane / wave numbers re-derived behind an opaque move: the LDS addresses the epilogue needs are then computed HERE instead of being
    // carried through the sweep -- the kernel sits on its 168-register budget and carried addresses were spilled to scratch memory,
    // i.e. to HBM traffic)
    const int lane_e = lane_p, wave_e = wave_p;
    if (lane_e < 16) {
        const int col = wave_e * 16 + lane_e;
        if (PERSIST) {
            sh[0][col] = 0.0; sh[1][col] = 0.0;              // the live slots: 0, 1 and [acc_lo, acc_hi)
            for (int a = acc_lo(mode == 1); a < nacc; ++a) sh[a][col] = 0.0;
        } else
            for (int a = 0; a < acc_dense_live(mode == 1); ++a) sh[a][col] = 0.0;
        if (row_base_p + lane_e <= last) {
            const int32_t bj = rowi[wave_e][lane_e][0];
            const int64_t i = rowi[wave_e][lane_e][1];
            const bool none = bj < 0 || bj == INT_MAX;
            // Partners in the caller's row order (idx_cur / d2_cur: scattered 4- and 8-byte stores) only where a caller asked for
            // them (kpx_icp with idx / d2 outputs); the sorted-order copies the NEXT launch bounds its rows with only when the
            // partner changed -- in the late iterations of a registration almost no row changes its partner.
            const int32_t out_j = none ? -1 : bj;
            const int32_t prev_j = __float_as_int(rowk[wave_e][lane_e][6]);
            const bool changed = k == 0 || out_j != prev_j;
            if (idx_cur) idx_cur[i] = out_j;
            if (PERSIST) rowk[wave_e][lane_e][6] = __int_as_float(out_j);
            else if (changed) idx_sorted[row_base_p + lane_e] = out_j;
            if (none) {
                if (d2_cur) d2_cur[i] = INFINITY;
            } else {
                const double s[3] = { rowd[wave_e][lane_e][0], rowd[wave_e][lane_e][1], rowd[wave_e][lane_e][2] };
                // The partner's coordinates and its normal are gathered through the index only where the partner CHANGED: those of an
                // unchanged partner came at the launch's start (coordinates with the row: ptgt_sorted; the normal through the previous
                // index).  In the late iterations whole waves skip this dependent round trip; both parts of a changed partner are
                // requested together.
                float tf[3] = { rowk[wave_e][lane_e][0], rowk[wave_e][lane_e][1], rowk[wave_e][lane_e][2] }, nf[3] = { rowk[wave_e][lane_e][3], rowk[wave_e][lane_e][4], rowk[wave_e][lane_e][5] };
                if (changed) {
                    const float *tp = tgt + 3 * (int64_t)bj;
#pragma unroll
                    for (int c = 0; c < 3; ++c) tf[c] = tp[c];
                    if (mode == 1) {
                        const float *np_ = tn + 3 * (int64_t)bj;
#pragma unroll
                        for (int c = 0; c < 3; ++c) nf[c] = np_[c];
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) {                                                   // the next iteration bounds this row with it
                        if (PERSIST) { rowk[wave_e][lane_e][c] = tf[c]; rowk[wave_e][lane_e][3 + c] = nf[c]; }
                        else ptgt_sorted[3 * (row_base_p + lane_e) + c] = tf[c];
                    }
                }
                const double t[3] = { (double)tf[0], (double)tf[1], (double)tf[2] };
                const double d2 = pair_d2(s, t);
                if (d2_cur) d2_cur[i] = d2;
                if (d2 < max_d2) pair_terms(s, t, d2, mode != 1, mode == 1, nf, [&](int slot, double v) { sh[sh_row(slot)][col] = v; });
            }
        }
    }
    if constexpr (!PERSIST) {
        if (kIWaves > 1) {
            wave_lds_fence();
            unsigned arrived = 0u;
            if (lane_e == 0) arrived = __hip_atomic_fetch_add(&s_arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (__builtin_amdgcn_readfirstlane((int)arrived) != kIWaves - 1) return;
            wave_lds_fence();
        }
        phase_tick_wave(tile_visits, 4, bid, lane_e);
        // The sums' contract (round 5) as stated below for the chain form; lane = dense row: the mode's live slots in slot order
        const bool plane = mode == 1;
        if (lane_e < acc_dense_live(plane)) {
            const int slot_e = acc_dense_slot(plane, lane_e);
            unsigned long long lo = 0ull, hi = 0ull;
#pragma unroll
            for (int t = 0; t < kIWaves; ++t) {
                unsigned long long l, h;
                fixed_split(tile_tree16(&sh[lane_e][16 * t]), l, h);
                fixed_accumulate(lo, hi, l, h);
            }
            unsigned long long *slot = acc + (((int64_t)(bid & (kAccCopies - 1)) * kAcc + slot_e) * kFixedWords);
            if (fuse.ticket) fixed_add_words_performed(slot, lo, hi); else fixed_add_words(slot, lo, hi);
        } else if (fuse.ticket && lane_e == nacc) {
            int cnt = 0;
#pragma unroll
            for (int wv = 0; wv < kIWaves; ++wv) cnt += s_cnt[wv];
            if (cnt) {
                const unsigned long long back = __hip_atomic_fetch_add(fuse.ticket + kSearchedWord + (bid & 7u), (unsigned long long)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("" ::"v"(back));
            }
        }
        if (fuse.light_key && lane_e == 63) {
            double g2 = INFINITY;
            bool light = true;
#pragma unroll
            for (int wv = 0; wv < kIWaves; ++wv) { light = light && s_light[wv] >= 0.0; g2 = fmin(g2, s_light[wv]); }
            fuse.light_key[bid] = light ? st->motion + sqrt(g2) * (1.0 - 1e-9) : 0.0;
        }
        phase_tick_wave(tile_visits, 5, bid, lane_e);
    } else {
    __syncthreads();
    phase_tick(tile_visits, 4, bid);
    // (the thread number re-derived behind the sweep, like the lane state of the pair epilogue: the accumulator slot's address, a 64-bit
    // value per lane known from the kernel's first instruction, was otherwise computed there and carried -- spilled -- across the sweep;
    // every spilled dword is 256 B of scratch per wave written back to HBM at the end of the launch: 0.5 MB per launch at 31k rows)
    const int tix_e = wave_e * 64 + lane_e;
    if (tix_e < nacc && acc_live(mode == 1, tix_e)) {
        // The sums' contract (round 5), for the slots that are live in the mode (acc_live: 0..16 point-to-point; 0, 1 and 17..43 point-to-plane;
        // a slot that is not live is neither staged in sh nor summed nor added, and the winner takes its total as 0.0): per 16-row TILE a balanced tree over adjacent rows (tile_tree16: what four DPP steps give a
        // wave that holds one row per lane, icp_rows_kernel), the tiles' partials then added EXACTLY in 128-bit fixed point -- so the
        // totals do not depend on how tiles are dealt out to waves, blocks or launches, and every form of the iteration agrees bit for bit.
        unsigned long long lo = 0ull, hi = 0ull;
#pragma unroll
        for (int t = 0; t < kIWaves; ++t) {
            unsigned long long l, h;
            fixed_split(tile_tree16(&sh[tix_e][16 * t]), l, h);
            fixed_accumulate(lo, hi, l, h);
        }
        unsigned long long *slot = acc + (((int64_t)(bid & (kAccCopies - 1)) * kAcc + tix_e) * kFixedWords);
        if (fuse.ticket) fixed_add_words_performed(slot, lo, hi); else fixed_add_words(slot, lo, hi);
    }
    if (fuse.light_key && tix == kIThreads - 1) {      // (after the barrier above: s_light is complete)
        double g2 = INFINITY;
        bool light = true;
#pragma unroll
        for (int wv = 0; wv < kIWaves; ++wv) { light = light && s_light[wv] >= 0.0; g2 = fmin(g2, s_light[wv]); }
        const double nk = light ? st->motion + sqrt(g2) * (1.0 - 1e-9) : 0.0;
        s_key = nk;
    }
    phase_tick(tile_visits, 5, bid);
    }
    } while (false);
    if constexpr (!PERSIST) {
        // One wave is left: the one that closed the block, or wave 0 of a block LightSkip left out.  "The last block finishes the job" as
        // described below, a wave in place of the block: the wave waits for its adds, draws the ticket, and as winner takes the totals
        // and performs the update -- the instantiation and the sequence of icp_rows_kernel (kpx_icprows.h).
        if (!fuse.ticket) return;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        wave_lds_fence();
        const int lane_w = opaque_i((int)(threadIdx.x & 63));
        unsigned tk = 0u;
        if (lane_w == 0) tk = (unsigned)__hip_atomic_fetch_add(fuse.ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tk = (unsigned)__builtin_amdgcn_readfirstlane((int)tk);
        wave_lds_fence();
        if (tk != nblocks - 1u) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");      // the winner only: one per registration and launch
        const unsigned long long n_searched = winner_take<64, true>(acc, fuse.ticket, mode == 1, s_sums, lane_w);
        __shared__ FinishScratch s_tail;
        // (t2max again from the target's box, behind an opaque move of its address: a double every lane would otherwise carry across the sweep)
        const double *tbbox_w = tbbox;
        asm volatile("" : "+s"(tbbox_w));
        const double t2max_w = target_t2max(tbbox_w);
        icp_finish_wave(s_sums, n, mode, k, fuse.max_iter, fuse.rel_fit, fuse.rel_rmse, &s_state, fuse.result, s_tail, lane_w,
                        LightSkip{ fuse.light_key ? fuse.sbbox : (const double *)nullptr, max_d2, t2max_w });
        wave_lds_fence();
        winner_publish(const_cast<IcpState *>(st), &s_state, fuse.cert ? fuse.thist : (double *)nullptr, k, fuse.progress, fuse.tag, n_searched, n, lane_w);
    } else {
    if (PERSIST && fuse.stamp && tix == 0) {
        const unsigned long long t = wall_clock64();
        if (bid == 0) fuse.stamp[3] = t;
        atomicMax(&fuse.stamp[11], t);
    }
    if (!fuse.ticket) return;
    // "The last block finishes the job": every add above has RETURNED (it has been performed at the device's point of coherence),
    // the barrier orders the block's ticket behind them, and the block that draws the last ticket of its registration reads the
    // totals -- 8 pairs of words for each of the mode's 17 / 29 live slots -- with device-coherent loads, clears the whole set for the next launch and performs the update.
    // Only relaxed atomics on the producers' side: no release fence, which on this part writes back the XCD's L2 (measured 10x slower,
    // once per block).  The CONSUMER side is by the book: the winner -- one block per registration and launch -- acquires at agent
    // scope behind its ticket (a single buffer_inv; same-box A/B against none: equal within noise, profiles/r03/exp_icp_acquire_fence.txt).
    // This is the `sc1` form of the valid hand-offs of MI355X_MICROARCH.md ("Correctness boundaries"): the handed-off bytes are
    // produced by atomics (performed at the memory side, never resident in a CU's L1), drained before the ticket because every
    // add RETURNS, and read by the winner with device-coherent (sc1) loads only (fixed_total_coherent) -- no plain load of them
    // anywhere.  It rests on gfx950 behaviour, not on the HIP memory model: KPX_ICP_BATCH_LAUNCH=0 KPX_ICP_FUSE=0 (per-registration chains,
    // update in its own kernel, ordered by the kernel boundary) is the portable fall-back, and
    // test_update_placements_agree_with_four_frames_in_flight compares the two bit for bit under four frames in flight.
    // The state is written with plain stores: its readers are the blocks of the NEXT launch, behind the kernel boundary.
    __shared__ unsigned s_ticket;
    __syncthreads();
    if (tix == 0) s_ticket = (unsigned)__hip_atomic_fetch_add(fuse.ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (PERSIST && fuse.stamp && tix == 0) {
        const unsigned long long t = wall_clock64();
        if (bid == 0) fuse.stamp[4] = t;
        atomicMax(&fuse.stamp[6], t);
    }
    if (s_ticket != nblocks - 1u) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");      // the winner only: one per registration and launch
    // (the winner's thread number behind an opaque move as well: addresses derived from it are then formed here, not in front of the sweep)
    const int tix_w = opaque_i((int)threadIdx.x);
    winner_take<kIThreads, false>(acc, fuse.ticket, mode == 1, s_sums, tix_w);
    chain_tick(fuse.stamp, 7, tix == 0);         // (the clearing stores are issued, not waited for)
    // PERSIST: the blocks that see the next record add to these accumulators at once, so every clearing store (and the ticket's) must
    // have been performed before the record is published: each wave drains its stores, the block meets at a barrier (wave 0 after the
    // update algebra, which hides the drain), then wave 0 publishes
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (wave != 0) {
        __syncthreads();
        return;
    }
    __shared__ FinishScratch s_tail;
    // (t2max again from the target's box, behind an opaque move of its address: a double every lane would otherwise carry across the sweep)
    const double *tbbox_w = tbbox;
    asm volatile("" : "+s"(tbbox_w));
    const double t2max_w = target_t2max(tbbox_w);
    IcpState *work = &s_state;
    icp_finish_wave_call(s_sums, n, mode, k, fuse.max_iter, fuse.rel_fit, fuse.rel_rmse, work, (double *)nullptr, &s_tail, lane,
                         fuse.light_key ? fuse.sbbox : (const double *)nullptr, max_d2, t2max_w, fuse.stamp ? fuse.stamp + 32 : (unsigned long long *)nullptr);
    wave_lds_fence();
    chain_tick(fuse.stamp, 8, lane == 0);
    {
        static_assert(sizeof(IcpState) == kChainWords * sizeof(double), "record layout");
        __syncthreads();
        if (lane < kChainWords)
            __hip_atomic_store(reinterpret_cast<unsigned long long *>(fuse.chain_rec + (size_t)kChainRec * (k + 1)) + lane,
                               reinterpret_cast<const unsigned long long *>(&s_state)[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // the result is written ONCE, by the winner of the last iteration: the winners of a chain sit on different XCDs, and plain stores of
        // several of them to the same words would reach memory in whatever order their L2s are written back at the end of the kernel
        if (work->done && fuse.result) {
            if (lane < 16) fuse.result[lane] = work->T[lane];
            if (lane == 0) { fuse.result[16] = work->fitness; fuse.result[17] = work->rmse; fuse.result[18] = (double)k; fuse.result[19] = work->count; }
        }
        if (lane == 0 && fuse.progress && work->done)
            __hip_atomic_store(fuse.progress, fuse.tag | (1ull << 32) | (unsigned long long)(unsigned)(k + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        chain_tick(fuse.stamp, 9, lane == 0);
        if (fuse.stamp && lane == 0) fuse.stamp[12] = __builtin_amdgcn_s_memtime();      // shader clock (against [9]: the clock the chip runs the chain at)
    }
    }
}


__global__ __launch_bounds__(kIThreads) __attribute__((amdgpu_waves_per_eu(KPX_ICP_WPE, KPX_ICP_WPE))) void icp_iter_kernel(const float *__restrict__ src, int64_t n, const float *__restrict__ tgt,
                                                       const float *__restrict__ tn, const double *__restrict__ Bs,
                                                       const int32_t *__restrict__ orig, const float *__restrict__ tile_box,
                                                       const float *__restrict__ group_box, int32_t n_groups,
                                                       const double *__restrict__ tbbox, const int32_t *__restrict__ row_of,
                                                       const float *__restrict__ src_sorted, int32_t *__restrict__ idx_sorted,
                                                       float *__restrict__ ptgt_sorted,
                                                       int32_t *__restrict__ idx_cur, double *__restrict__ d2_cur, double max_d2, int mode,
                                                       int k, const IcpState *__restrict__ st, unsigned long long *acc,
                                                       unsigned long long *__restrict__ tile_visits, IcpFuse fuse)
{
    icp_iter_body(blockIdx.x, gridDim.x, src, n, tgt, tn, Bs, orig, tile_box, group_box, n_groups, tbbox, row_of, src_sorted, idx_sorted, ptgt_sorted,
                  idx_cur, d2_cur, max_d2, mode, k, st, acc, tile_visits, fuse);
}

// Several registrations onto ONE shared target in one launch per iteration (kpx_icp_batch): block b belongs to the problem
// whose block range holds it.  A frame's three or seven registrations then cost one chain of launches instead of three or
// seven -- every kernel boundary writes back / invalidates the XCDs' L2s for everything else running on the device, so the
// number of launches per frame, not their size, is what the frame rate of the pipeline follows.  A problem that has
// converged keeps its blocks in the later launches: they read its state and return.
__global__ __launch_bounds__(kIThreads) __attribute__((amdgpu_waves_per_eu(KPX_ICP_WPE, KPX_ICP_WPE))) void icp_iter_batch_kernel(IcpBatchArgs args, double max_d2, int mode, int max_iter, double rel_fit,
                                                       double rel_rmse, unsigned long long *__restrict__ tile_visits, int light, CertPolicy pol)
{
    const IcpProblem &P = args.p[batch_problem(args)];
    const unsigned bid = blockIdx.x - P.block0;
    const float *__restrict__ tgt = P.tgt, *__restrict__ tn = P.tn, *__restrict__ tile_box = P.tile_box, *__restrict__ group_box = P.group_box;
    const double *__restrict__ Bs = P.Bs, *__restrict__ tbbox = P.tbbox;
    const int32_t *__restrict__ orig = P.orig;
    const int32_t n_groups = P.n_groups;
    const int k = P.k;
    const IcpFuse fuse = ticket_fuse(P, max_iter, rel_fit, rel_rmse, P.tag, light, pol, nullptr, nullptr);
    icp_iter_body(bid, P.blocks, P.src, P.n, tgt, tn, Bs, orig, tile_box, group_box, n_groups, tbbox, P.row_of, P.src_sorted, P.idx_sorted, P.ptgt_sorted,
                  P.idx_cur, P.d2_cur, max_d2, mode, k, P.pair, P.ring, tile_visits, fuse);
}

// The whole chain of a group of registrations in ONE launch: block b iterates over k on the rows it owns (icp_iter_body<true>), the
// block that draws the last ticket of iteration k performs the update and publishes record k + 1, everybody else waits for it (see
// kChainRec).  No kernel boundary, no host poll, no re-read of the rows: an iteration costs the ticket, the update algebra and one
// coherent round trip instead of a launch.
// REQUIRES every block of the launch to be resident at the same time (a block that is not can never deliver its sums): the host
// launches this form only when the grid fits the device beside every other chain kernel it has in flight (chain_reserve), and every
// wait is bounded -- a block that has waited `limit_ticks` (100 MHz wall clock, counted from ITS start) raises *abort_word (pinned
// host memory), poisons its registration's result and leaves; the others follow on their own clocks.  The library reports a raised
// word at the next call (KPX_ERR_HIP); KPX_ICP_CHAIN=0 selects the launch-per-iteration form.
__global__ __launch_bounds__(kIThreads) __attribute__((amdgpu_waves_per_eu(KPX_ICP_WPE, KPX_ICP_WPE))) void icp_chain_kernel(IcpBatchArgs args, const float *__restrict__ tgt,
                                                       const float *__restrict__ tn, const double *__restrict__ Bs,
                                                       const int32_t *__restrict__ orig, const float *__restrict__ tile_box,
                                                       const float *__restrict__ group_box, int32_t n_groups,
                                                       const double *__restrict__ tbbox, double max_d2, int mode, int max_iter, double rel_fit,
                                                       double rel_rmse, unsigned long long tag, unsigned long long *__restrict__ tile_visits, int light,
                                                       CertPolicy pol, unsigned long long limit_ticks, unsigned long long *abort_word)
{
    const int pi = batch_problem(args);
    const IcpProblem &P = args.p[pi];
    const unsigned bid = blockIdx.x - P.block0;
    __shared__ IcpState s_cur;
    __shared__ int s_abort;
    const unsigned long long t0 = wall_clock64();
    if (threadIdx.x == 0) s_abort = 0;
    __syncthreads();
    for (int k = 0; k <= max_iter; ++k) {
        // (the operands' addresses behind opaque moves, per iteration: their loop-invariant loads -- the first group boxes, the problem's
        // descriptor -- would otherwise be hoisted out of the loop and live in registers across it)
        asm volatile("" : "+s"(tgt), "+s"(tn), "+s"(Bs), "+s"(orig), "+s"(tile_box), "+s"(group_box), "+s"(tbbox));
        asm volatile("" : "+s"(max_d2), "+s"(mode), "+s"(n_groups), "+s"(pol.calm), "+s"(pol.factor), "+s"(pol.smin), "+s"(pol.smax));
        const IcpFuse fuse = ticket_fuse(P, max_iter, rel_fit, rel_rmse, tag, light, pol, P.chain_rec,
                                         ((light & 8) && pi == 0 && k < 64) ? &g_chain_stamp[k][0] : (unsigned long long *)nullptr);
        if (threadIdx.x < kChainWords) {
            const unsigned long long *w = reinterpret_cast<const unsigned long long *>(P.chain_rec + (size_t)kChainRec * k) + threadIdx.x;
            unsigned long long v = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            unsigned spins = 0;
            while (v == kChainEmpty) {
                __builtin_amdgcn_s_sleep(2);
                if ((++spins & 255u) == 0u && wall_clock64() - t0 > limit_ticks) { s_abort = 1; break; }
                v = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            reinterpret_cast<unsigned long long *>(&s_cur)[threadIdx.x] = v;
        }
        __syncthreads();
        if (s_abort) {
            // the abort is reported PER CALL: every result word of the registration is NaN (nothing stale leaks out, and whoever reads the
            // result -- ops.icp_batch, kpx_frame_step*, the exchange header of the sharded step -- sees it for THIS call); the pinned word is
            // the process-wide diagnostic behind it
            if (threadIdx.x == 0) __hip_atomic_store(abort_word, tag | 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (P.result && threadIdx.x < 20) P.result[threadIdx.x] = __builtin_nan("");
            return;
        }
        if (s_cur.done) break;
        icp_iter_body<true>(bid, P.blocks, P.src, P.n, tgt, tn, Bs, orig, tile_box, group_box, n_groups, tbbox, P.row_of, P.src_sorted, P.idx_sorted, P.ptgt_sorted,
                            P.idx_cur, P.d2_cur, max_d2, mode, k, &s_cur, P.ring, tile_visits, fuse);
        __syncthreads();                                     // (the body's early returns meet here before s_cur is written again)
    }
}

// Start of a batch chain in ONE launch: per problem both state slots <- the initial transform, the accumulator ring cleared,
// the rows gathered into Morton order (what icp_init_kernel + a memset + gather_rows_kernel did per problem)
__global__ __launch_bounds__(256) void icp_batch_init_kernel(IcpBatchArgs args, Mat16x8 T0)
{
    const int pi = batch_problem(args);
    const IcpProblem &P = args.p[pi];
    const unsigned bid = blockIdx.x - P.block0;
    const int c = threadIdx.x & 3;
    for (int rr = threadIdx.x >> 2; rr < kIRows; rr += 64) {
        const int64_t r = (int64_t)bid * kIRows + rr;
        if (r < P.n && c < 3) P.src_sorted[3 * r + c] = P.src[3 * (int64_t)P.row_of[r] + c];
    }
    if (threadIdx.x == 0) P.light_key[bid] = 0.0;           // the block's LightSkip key
    if (bid == 0) {
        for (int e = threadIdx.x; e < 3 * kAccSet; e += 256) P.ring[e] = 0ull;
        if (threadIdx.x >= 64 && threadIdx.x < 76) P.thist[threadIdx.x - 64] = T0.m[pi][threadIdx.x - 64];
        if (P.chain_rec) {                                  // the chain form: record 0 = the initial state (below), every other record empty
            unsigned long long *rw = reinterpret_cast<unsigned long long *>(P.chain_rec);
            for (int e = kChainRec + threadIdx.x; e < kChainRecords * kChainRec; e += 256) rw[e] = kChainEmpty;
            IcpState *r0 = reinterpret_cast<IcpState *>(P.chain_rec);
            if (threadIdx.x >= 128 && threadIdx.x < 144) r0->T[threadIdx.x - 128] = T0.m[pi][threadIdx.x - 128];
            if (threadIdx.x == 144) state_fresh(r0);
        }
        if (threadIdx.x < 32) {
            IcpState *st = P.pair + (threadIdx.x >> 4);
            st->T[threadIdx.x & 15] = T0.m[pi][threadIdx.x & 15];
            if ((threadIdx.x & 15) == 0) state_fresh(st);
        }
    }
}

}  // namespace kpx
