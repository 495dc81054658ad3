// kpx_icp.hip -- register stage: registration_icp (preprocessing/registration.py:78-84 point-to-plane,
// manual_pointcloud_registration.py:90-98 point-to-point + Kabsch from picked pairs).
//
// This file is the HOST side and the one translation unit of the registration's device code (the library is built without
// relocatable device code, and the kernels share __device__ globals).  Where things are:
//   kpx_icpdefs.h   tile constants and compile-time knobs, IcpState, the kernels' argument blocks (IcpFuse, IcpProblem, IcpBatchArgs)
//   kpx_nndense.h   the all-pairs search (fp64 MFMA distance GEMM, float32 screening sweep) and nn_merge_kernel; the arithmetic
//                   contract of the correspondence search is stated at its top
//   kpx_icpsolve.h  the update step: Kabsch / point-to-plane solve, convergence, LightSkip's bookkeeping, the solve kernels
//   kpx_nnlocal.h   the culled search (sweep_wave) and a bare search's kernels
//   kpx_icpiter.h   one iteration of the culled registration in one kernel: per registration, per batch, the whole chain in one launch;
//                   above icp_iter_body the pieces every form of the iteration shares (certificate skin / test / word, the self-check's
//                   bookkeeping, the winner's step); the row bound and the pair terms, which the searches use too, are in kpx_icpdefs.h
//   kpx_icprows.h   the same iteration with a wave per 64 rows (the calm iterations), same argument block and shared pieces
//   kpx_icpchain.h  host: which one-launch chains may be resident together
// Below: the switches (IcpSwitches), profiling read-backs, plans and workspace, the search launches, what the entry points share (NnProblem: setup
// and the correspondences' way out; icp_search_solve_loop), the exported entry points, and the batch driver (batch_carve, icp_batch_ordered
// with drive_grouped / drive_windowed / drive_dense_polled).  Each culled driver has one job: drive_grouped runs the registrations of a
// batch the sort ordered (at most seven) in one launch per iteration on the caller's stream, with the update in the last block of every
// registration's sweep; drive_windowed runs a chain per registration on the lanes with the update in the next sweep's prologue, or
// (KPX_ICP_FUSE=0, as kpx_icp does) in its own kernel behind the kernel boundary.
#include <chrono>
#include <limits.h>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>

#include "kpx_internal.h"
#include "kpx_linalg.h"
#include "kpx_fixed.h"
#include "kpx_icpdefs.h"
#include "kpx_nndense.h"
#include "kpx_icpsolve.h"
#include "kpx_nnlocal.h"
#include "kpx_icpiter.h"
#include "kpx_icprows.h"
#include "kpx_icpchain.h"

namespace kpx {

// ---- the switches of the registration ---------------------------------------------------------------------------------------------
// Every environment variable the registration reads, read ONCE (first use).  All of them select between forms that give the same
// results and exist for same-box A/B measurements ("Environment switches of the library").  KPX_NN_ENGINE and
// KPX_ICP_CHAIN are not here: kpx_nn_engine() / kpx_icp_chain() also set them at run time, so the environment only decides at their
// first use (local_engine() below, chain_form_on() in kpx_icpchain.h).
struct IcpSwitches {
    bool nn_screen;            // KPX_NN_SCREEN=0: dense engine without its float32 screening sweep; default on (tools/nn_dense_probe.py)
    bool batch_launch;         // KPX_ICP_BATCH_LAUNCH=0: one launch chain per registration; default one for the batch where one sort orders it, up to 7
    bool fuse;                 // KPX_ICP_FUSE=0: per-registration chains with the update in its own kernel, and no grouped chain; default on
    int window;                // KPX_ICP_WINDOW=1..64: launches of a group queued ahead of the newest progress word; default (and out of range) 3 (profiles/r04/exp_icp_window.txt)
    double stall_seconds;      // KPX_ICP_STALL_SECONDS>0: watchdog of the launch windows; default 60
    bool light_skip;           // KPX_ICP_LIGHT_SKIP=0: sweep every block; default on (test_icp_update_placements_and_light_skip_are_bit_identical)
    bool cert;                 // KPX_ICP_CERT=0: search every row every iteration; default on, ignored (off) without LightSkip (same test)
    bool cert_check;           // KPX_ICP_CERT_CHECK=1: search certified rows all the same and count disagreements; default off (test_icp_certificates_never_contradict_the_search)
    CertPolicy cert_policy;    // KPX_CERT_CALM / _FACTOR / _SKIN_MIN / _SKIN_MAX: the certificates' skin policy; default 0.15 / 3 / 0.02 / 0.2
    int rows;                  // KPX_ICP_ROWS=0|1|2: icp_rows_kernel never / by searched share / always (the grouped driver); default 1 (test_icp_update_placements_and_light_skip_are_bit_identical)
    int rows_share;            // KPX_ICP_ROWS_SHARE=1..127: largest searched share (1/127ths) served by the rows form; default (and out of range) 3 (same test)
    bool chain_alone;          // KPX_ICP_CHAIN_ALONE=0: admit one-launch chains also with other frames in flight; default only alone
    long chain_budget;         // KPX_ICP_CHAIN_BUDGET=blocks the chains in flight may hold; default -1 = (blocks per CU - 1) x CUs (test_icp_chain_that_cannot_be_resident_fails_loudly)
    bool chain_no_lock;        // KPX_ICP_CHAIN_LOCK=0: skip the one-process-per-GPU lock file; default locked (test_icp_update_placements_and_light_skip_are_bit_identical)
    unsigned long long chain_wait_ticks;   // KPX_ICP_CHAIN_WAIT_SECONDS>0: bound of every wait inside a chain, in 100 MHz ticks; default 2 s (test_icp_chain_that_cannot_be_resident_fails_loudly)
    bool chain_stamps;         // KPX_ICP_CHAIN_STAMPS=1: the chain's clock, kpx_prof_icp_chain; default off (tools/icp_chain_clock.py)
    bool chain_dump;           // KPX_ICP_CHAIN_DUMP=1: development aid, the chain's records on stderr; default off
};
static const IcpSwitches &icp_switches()
{
    static const IcpSwitches sw = [] {
        auto text = [](const char *name) { const char *e = getenv(name); return e ? e : ""; };
        auto not0 = [&](const char *name) { return text(name)[0] != '0'; };
        auto is1 = [&](const char *name) { return text(name)[0] == '1'; };
        auto digit = [&](const char *name, char hi, int dflt) { const char c = text(name)[0]; return c >= '0' && c <= hi ? c - '0' : dflt; };
        auto real = [](const char *name, float dflt) { const char *e = getenv(name); return e ? (float)atof(e) : dflt; };
        IcpSwitches w;
        w.nn_screen = not0("KPX_NN_SCREEN");
        w.batch_launch = not0("KPX_ICP_BATCH_LAUNCH");
        w.fuse = not0("KPX_ICP_FUSE");
        const int window = atoi(text("KPX_ICP_WINDOW"));
        w.window = window >= 1 && window <= 64 ? window : 3;
        const double stall = atof(text("KPX_ICP_STALL_SECONDS"));
        w.stall_seconds = stall > 0.0 ? stall : 60.0;
        w.light_skip = not0("KPX_ICP_LIGHT_SKIP");
        w.cert = w.light_skip && not0("KPX_ICP_CERT");        // (the certificates rest on LightSkip's motion bookkeeping)
        w.cert_check = is1("KPX_ICP_CERT_CHECK");
        w.cert_policy = CertPolicy{ real("KPX_CERT_CALM", 0.15f), real("KPX_CERT_FACTOR", 3.0f), real("KPX_CERT_SKIN_MIN", 0.02f), real("KPX_CERT_SKIN_MAX", 0.2f) };
        w.rows = digit("KPX_ICP_ROWS", '2', 1);
        const int share = atoi(text("KPX_ICP_ROWS_SHARE"));
        w.rows_share = share >= 1 && share <= 127 ? share : 3;
        w.chain_alone = not0("KPX_ICP_CHAIN_ALONE");
        const char *budget = getenv("KPX_ICP_CHAIN_BUDGET");
        w.chain_budget = budget ? atol(budget) : -1L;
        w.chain_no_lock = text("KPX_ICP_CHAIN_LOCK")[0] == '0';
        const double wait = atof(text("KPX_ICP_CHAIN_WAIT_SECONDS"));
        w.chain_wait_ticks = (unsigned long long)((wait > 0.0 ? wait : 2.0) * 1e8);
        w.chain_stamps = is1("KPX_ICP_CHAIN_STAMPS");
        w.chain_dump = is1("KPX_ICP_CHAIN_DUMP");
        return w;
    }();
    return sw;
}
// the switch word the iteration kernels take (a kernel argument): bit 0 LightSkip, bit 1 row certificates, bit 2 the certificates'
// self-check, bit 3 the chain's clock
static int icp_light_word(const IcpSwitches &sw)
{
    return (sw.light_skip ? 1 : 0) | (sw.cert ? 2 : 0) | (sw.cert_check ? 4 : 0) | (sw.chain_stamps ? 8 : 0);
}

// tiles multiplied by nn_local_kernel while the profiler is armed (one atomic per wave, spread over kVisitSlots
// addresses: same-address atomics from thousands of waves serialise in L2); read by kpx_prof_end
__device__ unsigned long long g_nn_visits[kVisitSlots];
static unsigned long long *nn_visits_ptr()
{
    static unsigned long long *p = nullptr;
    if (!p && hipGetSymbolAddress((void **)&p, HIP_SYMBOL(g_nn_visits)) != hipSuccess) p = nullptr;
    return p;
}
// -> h_out8 (16 doubles): average us per block in the five phases of the LAST sweep launch, [5] blocks of that launch, [6] dispatch
// ramp (latest block start - earliest block start), [7] span (earliest start -> latest end), [8..12] slowest block per phase,
// [13] longest block lifetime
int icp_phase_take(double *h_out8)
{
    static unsigned long long v[kStampBlocks][8];
    unsigned long long *p = nullptr;
    if (hipGetSymbolAddress((void **)&p, HIP_SYMBOL(g_icp_stamp)) != hipSuccess) return KPX_ERR_HIP;
    if (hipMemcpy(v, p, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return KPX_ERR_HIP;
    for (int q = 0; q < 16; ++q) h_out8[q] = 0.0;
    int blocks = (int)v[0][6];
    if (blocks < 1) return KPX_OK;
    if (blocks > kStampBlocks) blocks = kStampBlocks;
    for (int b = 0; b < blocks; ++b) h_out8[14] += v[b][7] ? 1.0 : 0.0;        // blocks LightSkip left out of the last launch
    unsigned long long s_min = ~0ull, s_max = 0ull, e_max = 0ull;
    int counted = 0;
    for (int b = 0; b < blocks; ++b) {
        if (v[b][7] || !(v[b][5] >= v[b][0]) || v[b][1] < v[b][0]) continue;          // a block of an "already converged" launch stamps nothing new
        for (int q = 0; q < 5; ++q) {
            const double d = (double)(v[b][q + 1] - v[b][q]) * 0.01;
            h_out8[q] += d;
            if (d > h_out8[8 + q]) h_out8[8 + q] = d;                      // [8..12]: the slowest block of each phase
        }
        if ((double)(v[b][5] - v[b][0]) * 0.01 > h_out8[13]) h_out8[13] = (double)(v[b][5] - v[b][0]) * 0.01;   // longest block lifetime
        s_min = v[b][0] < s_min ? v[b][0] : s_min;
        s_max = v[b][0] > s_max ? v[b][0] : s_max;
        e_max = v[b][5] > e_max ? v[b][5] : e_max;
        ++counted;
    }
    if (!counted) return KPX_OK;
    for (int q = 0; q < 5; ++q) h_out8[q] /= (double)counted;
    h_out8[5] = (double)counted;
    h_out8[6] = (double)(s_max - s_min) * 0.01;
    h_out8[7] = (double)(e_max - s_min) * 0.01;
    return KPX_OK;
}
// raw rows of g_icp_wave for the blocks of the last sweep launch -> h_out (4 u64 per wave); returns the number of waves
int64_t icp_wave_take(unsigned long long *h_out, int64_t cap_waves)
{
    unsigned long long *p = nullptr, *ps = nullptr;
    if (hipGetSymbolAddress((void **)&p, HIP_SYMBOL(g_icp_wave)) != hipSuccess) return -1;
    if (hipGetSymbolAddress((void **)&ps, HIP_SYMBOL(g_icp_stamp)) != hipSuccess) return -1;
    unsigned long long first[8];
    if (hipMemcpy(first, ps, sizeof(first), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    int64_t waves = (int64_t)first[6] * kIWaves;
    if (waves > kStampBlocks * 4) waves = kStampBlocks * 4;
    if (waves > cap_waves) waves = cap_waves;
    if (waves > 0 && hipMemcpy(h_out, p, (size_t)waves * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return waves;
}
double nn_local_take_visits()
{
    static unsigned long long v[kVisitSlots], zero[kVisitSlots];
    unsigned long long *p = nn_visits_ptr();
    if (!p || hipMemcpy(v, p, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return 0.0;
    (void)hipMemcpy(p, zero, sizeof(zero), hipMemcpyHostToDevice);
    double sum = 0.0;
    for (int i = 0; i < kVisitSlots; ++i) sum += (double)v[i];
    return sum;
}

static int g_nn_engine = -1;          // KPX_NN_ENGINE_*; -1 = not chosen yet (environment decides at first use)
static bool g_nn_fp64_only = false;   // KPX_NN_ENGINE_DENSE_FP64: the all-pairs engine without its float32 screening sweep
static bool local_engine()
{
    if (g_nn_engine < 0) { const char *e = getenv("KPX_NN_ENGINE"); g_nn_engine = (e && e[0] == 'd') ? KPX_NN_ENGINE_DENSE : KPX_NN_ENGINE_CULLED; }
    return g_nn_engine == KPX_NN_ENGINE_CULLED;
}

struct NnPlan {
    int64_t tiles_pad, seed_tiles_pad, n_src, n_tgt, f_tiles_pad;
    int32_t l_groups;                                       // culled sweep: groups of 256 sorted target columns
    int32_t tiles_per_split, splits, row_blocks;
    int32_t f_tiles_per_split, f_splits, f_row_blocks;     // float32 screening sweep
};
static NnPlan nn_plan(int64_t n, int64_t m)
{
    NnPlan p;
    p.n_src = n; p.n_tgt = m;
    p.l_groups = (int32_t)cdiv(m > 0 ? m : 1, 16 * kLGroupTiles);
    int64_t tiles = cdiv(m > 0 ? m : 1, 16);
    int64_t stages = cdiv(tiles, kCT);
    p.row_blocks = (int32_t)cdiv(n > 0 ? n : 1, kRowsPerBlock);
    int64_t want = cdiv(4096, p.row_blocks);            // aim for >= ~4096 workgroups (16 per CU, 5 resident)
    if (want > stages) want = stages;
    if (want < 1) want = 1;
    if (want > 64) want = 64;
    int64_t stages_per_split = cdiv(stages, want);
    p.splits = (int32_t)cdiv(stages, stages_per_split);
    p.tiles_per_split = (int32_t)(stages_per_split * kCT);
    p.tiles_pad = (int64_t)p.splits * p.tiles_per_split;
    p.seed_tiles_pad = cdiv(cdiv(tiles, kSeedStride), kCT) * kCT;
    {
        int64_t fstages = cdiv(tiles, kFCT);
        p.f_row_blocks = (int32_t)cdiv(n > 0 ? n : 1, kFRowsPerBlock);
        int64_t fwant = cdiv(2048, p.f_row_blocks);
        if (fwant > fstages) fwant = fstages;
        if (fwant < 1) fwant = 1;
        if (fwant > 64) fwant = 64;
        int64_t per = cdiv(fstages, fwant);
        p.f_splits = (int32_t)cdiv(fstages, per);
        p.f_tiles_per_split = (int32_t)(per * kFCT);
        p.f_tiles_pad = (int64_t)p.f_splits * p.f_tiles_per_split;
    }
    return p;
}

// Which sweep serves iteration k: the float32 screening sweep pays off when the cloud barely moved since the
// last search (short candidate lists); after a large update (first iterations) the bound is loose, lists
// overflow and the exact fp64 sweep is cheaper.  The host sees (fitness, rmse) at every poll and uses their
// relative change as the motion proxy.
struct ScreenPolicy {
    double fit = -1.0, rmse = -1.0;
    bool calm = false;
    void observe(double f, double r)
    {
        calm = fit >= 0.0 && fabs(f - fit) <= 0.02 && fabs(r - rmse) <= 0.05 * (rmse > 1e-12 ? rmse : 1e-12);
        fit = f; rmse = r;
    }
    bool allow(int k) const { return k >= 2 && calm; }
};

struct NnBuffers {
    double *B, *Bseed, *part_val, *part_acc, *init_val, *d2_cur, *tbbox, *A64, *K64;
    float *Bf, *A32, *thr32;
    NnAux *aux;
    int32_t *part_idx, *init_idx, *idx_cur, *cand_cnt, *cand, *overflow;
    int32_t *colB, *colSeed;                            // dense engine: original index of every column of B / Bseed (curve-ordered operand)
    IcpState *state;
    double *T0;
    // culled sweep
    double *Bs;
    int32_t *orig_t, *row_of, *idx_sorted;
    float *src_sorted, *ptgt_sorted;                    // rows in Morton order; coordinates of each row's last partner, same order
    unsigned long long *acc_fixed;                      // [3][kAccCopies][kAcc][kFixedWords] exact accumulators
    double *light_key;                                  // per block of the iteration kernel (LightSkip)
    uint32_t *cert_sorted;                              // per sorted row: certificate (icp_iter_body)
    double *thist;                                      // transforms of the iterations so far (certificates)
    double *chain_rec;                                  // records of the one-launch chain (kChainRecords x kChainRec)
    float *tile_box, *group_box;
    SortScratch sort_t, sort_s;
};
static void nn_carve_target(Arena &a, const NnPlan &p, NnBuffers *b)
{
    b->Bs = a.get<double>((size_t)p.l_groups * kLGroupTiles * 64);
    b->orig_t = a.get<int32_t>((size_t)p.l_groups * kLGroupTiles * 16);
    b->tile_box = a.get<float>((size_t)p.l_groups * kLGroupTiles * 6);
    b->group_box = a.get<float>((size_t)p.l_groups * 6);
    sort_carve(a, p.n_tgt, &b->sort_t);
    b->B = a.get<double>((size_t)p.tiles_pad * 64);
    b->Bseed = a.get<double>((size_t)p.seed_tiles_pad * 64);
    b->colB = a.get<int32_t>((size_t)p.tiles_pad * 16);
    b->colSeed = a.get<int32_t>((size_t)p.seed_tiles_pad * 16);
    b->Bf = a.get<float>((size_t)p.f_tiles_pad * 64);
    b->aux = a.get<NnAux>(1);
    b->tbbox = a.get<double>((size_t)kBboxBlocks * 6 + 8);
}
static void nn_carve_source(Arena &a, int64_t n, const NnPlan &p, NnBuffers *b)
{
    const size_t nn = (size_t)(n > 0 ? n : 1);
    b->part_val = a.get<double>((size_t)p.splits * nn);
    b->part_idx = a.get<int32_t>((size_t)p.splits * nn);
    b->part_acc = a.get<double>((size_t)cdiv((int64_t)nn, kMergeThreads) * kAcc);
    b->init_val = a.get<double>(nn);
    b->init_idx = a.get<int32_t>(nn);
    b->idx_cur = a.get<int32_t>(nn);
    b->d2_cur = a.get<double>(nn);
    b->state = a.get<IcpState>(2);                     // two slots: the one-launch-per-iteration mode alternates between them
    b->T0 = a.get<double>(16);
    b->A64 = a.get<double>(nn * 4);
    b->K64 = a.get<double>(nn);
    b->A32 = a.get<float>(nn * 4);
    b->thr32 = a.get<float>(nn * 2);                     // (row constant, threshold) pairs
    b->cand_cnt = a.get<int32_t>(nn + 1);               // [n] counters + number of overflowed rows
    b->cand = a.get<int32_t>(nn * kCand);
    b->overflow = a.get<int32_t>(nn);                   // list of overflowed rows
    b->row_of = a.get<int32_t>(nn);
    b->idx_sorted = a.get<int32_t>(nn);
    b->src_sorted = a.get<float>(nn * 3);
    b->ptgt_sorted = a.get<float>(nn * 3);
    b->acc_fixed = a.get<unsigned long long>((size_t)3 * kAccCopies * kAcc * kFixedWords + 8);      // ring of three sets (icp_iter_kernel, IcpFuse)
    b->light_key = a.get<double>((size_t)cdiv((int64_t)nn, 64));   // per 64 rows: a block of icp_iter_body, a wave of icp_rows_kernel
    b->cert_sorted = a.get<uint32_t>(nn);
    b->thist = a.get<double>((size_t)kCertHist * 12);
    b->chain_rec = a.get<double>((size_t)kChainRecords * kChainRec);
    sort_carve(a, n, &b->sort_s);
}
static void nn_carve(Arena &a, int64_t n, int64_t m, const NnPlan &p, NnBuffers *b)
{
    nn_carve_target(a, p, b);
    nn_carve_source(a, n, p, b);
}

static bool screening_enabled() { return icp_switches().nn_screen && !g_nn_fp64_only; }
static __global__ __launch_bounds__(256) void gather_rows_kernel(const float *__restrict__ src, int64_t n, const int32_t *__restrict__ row_of,
                                                                 float *__restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int64_t i = row_of[r];
    out[3 * r] = src[3 * i]; out[3 * r + 1] = src[3 * i + 1]; out[3 * r + 2] = src[3 * i + 2];
}
// ordered: b.row_of already holds the Morton order (morton_order_batch)
static int nn_prep_source(const float *src, const NnPlan &p, const NnBuffers &b, hipStream_t st, bool ordered = false)
{
    if (!local_engine()) return morton_order(src, p.n_src, b.sort_s, b.row_of, st);       // the all-pairs sweep takes its rows in curve order
    KPX_HIP(hipMemsetAsync(b.acc_fixed, 0, ((size_t)3 * kAccCopies * kAcc * kFixedWords + 8) * sizeof(unsigned long long), st));
    int rc = ordered ? KPX_OK : morton_order(src, p.n_src, b.sort_s, b.row_of, st);
    if (rc) return rc;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)cdiv(p.n_src, 256)), dim3(256), 0, st, src, p.n_src, b.row_of, b.src_sorted);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}
// one ICP iteration (search k + update) of the culled engine: two launches
static void icp_iter_launch(const float *src, const float *tgt, const float *tn, const NnPlan &p, const NnBuffers &b, double max_d2, int mode,
                            int k, int max_iter, double rel_fit, double rel_rmse, double *d_result, hipStream_t st,
                            unsigned long long *progress = nullptr, unsigned long long tag = 0, bool want_pairs = true)
{
    {
        ProfScope prof(KPX_PROF_NN_LOCAL, 0.0, st);
        hipLaunchKernelGGL(icp_iter_kernel, dim3((unsigned)cdiv(p.n_src, kIRows)), dim3(kIThreads), 0, st, src, p.n_src, tgt, tn, b.Bs, b.orig_t,
                           b.tile_box, b.group_box, p.l_groups, b.sort_t.bbox, b.row_of, b.src_sorted, b.idx_sorted, b.ptgt_sorted,
                           want_pairs ? b.idx_cur : (int32_t *)nullptr, want_pairs ? b.d2_cur : (double *)nullptr, max_d2, mode, k, b.state,
                           b.acc_fixed, prof_armed() ? nn_visits_ptr() : (unsigned long long *)nullptr, IcpFuse{});
    }
    hipLaunchKernelGGL(icp_solve_fixed_kernel, dim3(1), dim3(256), 0, st, b.acc_fixed, p.n_src, mode, k, max_iter, rel_fit, rel_rmse, b.state,
                       d_result, progress, tag);
}
// one ICP iteration in ONE launch (IcpFuse): launch k = update of iteration k-1 + search k; k = max_iter + 1 is the closing
// launch (update only: one block)
static void icp_fused_launch(const float *src, const float *tgt, const float *tn, const NnPlan &p, const NnBuffers &b, double max_d2, int mode,
                             int k, int max_iter, double rel_fit, double rel_rmse, double *d_result, hipStream_t st,
                             unsigned long long *progress, unsigned long long tag)
{
    const IcpFuse fuse{ b.state, b.acc_fixed, max_iter, rel_fit, rel_rmse, d_result, progress, tag, nullptr, nullptr, nullptr, nullptr, nullptr, 0, CertPolicy{ 0.0f, 0.0f, 0.0f, 0.0f } };
    const unsigned blocks = k > max_iter ? 1u : (unsigned)cdiv(p.n_src, kIRows);
    ProfScope prof(KPX_PROF_NN_LOCAL, 0.0, st);
    hipLaunchKernelGGL(icp_iter_kernel, dim3(blocks), dim3(kIThreads), 0, st, src, p.n_src, tgt, tn, b.Bs, b.orig_t, b.tile_box, b.group_box,
                       p.l_groups, b.sort_t.bbox, b.row_of, b.src_sorted, b.idx_sorted, b.ptgt_sorted, b.idx_cur, b.d2_cur, max_d2, mode, k, b.state,
                       b.acc_fixed, prof_armed() ? nn_visits_ptr() : (unsigned long long *)nullptr, fuse);
}
// ordered: b.orig_t / b.sort_t.bbox already hold the target's Morton order and bounding box (morton_order_batch)
static int nn_prep(const float *tgt, const NnPlan &p, const NnBuffers &b, hipStream_t st, bool ordered = false)
{
    if (local_engine()) {
        int rc = ordered ? KPX_OK : morton_order(tgt, p.n_tgt, b.sort_t, b.orig_t, st);
        if (rc) return rc;
        hipLaunchKernelGGL(nn_local_prep_kernel, dim3((unsigned)p.l_groups), dim3(256), 0, st, tgt, p.n_tgt, b.Bs, b.orig_t, b.tile_box,
                           b.group_box);
        KPX_LAUNCH_CHECK();
        return KPX_OK;
    }
    // the all-pairs operand in the target's curve order
    int rc = morton_order(tgt, p.n_tgt, b.sort_t, b.orig_t, st);
    if (rc) return rc;
    int64_t work = (p.tiles_pad + p.seed_tiles_pad) * 16;
    hipLaunchKernelGGL(nn_prep_kernel, dim3((unsigned)(cdiv(work, 256) > 2048 ? 2048 : cdiv(work, 256))), dim3(256), 0, st, tgt,
                       p.n_tgt, p.tiles_pad, b.B, p.seed_tiles_pad, b.Bseed, b.orig_t, b.colB, b.colSeed);
    {   // float32 screening operand: centre + radius from the target's bounding box
        double *bbox = b.tbbox + (size_t)kBboxBlocks * 6;
        rc = bbox_f32(tgt, p.n_tgt, bbox, b.tbbox, st);
        if (rc) return rc;
        hipLaunchKernelGGL(nn_aux_kernel, dim3(1), dim3(1), 0, st, bbox, b.aux);
        int64_t fw = p.f_tiles_pad * 16;
        hipLaunchKernelGGL(nn_prep_f32_kernel, dim3((unsigned)(cdiv(fw, 256) > 2048 ? 2048 : cdiv(fw, 256))), dim3(256), 0, st, tgt,
                           p.n_tgt, p.f_tiles_pad, b.aux, b.Bf);
    }
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

// One correspondence search.  have_prev: b.idx_cur holds the partners of the previous search (bound from them),
// otherwise a seed sweep over every 64th target tile provides the bound.
template <class Terms = ColorTerms>
static int nn_search_launch(const float *src, const float *tgt, const float *tn, const NnPlan &p, const NnBuffers &b,
                            const double *T, const int32_t *done, bool have_prev, bool allow_screen, double max_d2, int mode, hipStream_t st,
                            Terms ct = Terms{})
{
    const int64_t n = p.n_src;
    const dim3 thr(256);
    if (local_engine()) {
        hipLaunchKernelGGL(nn_local_rowprep_kernel, dim3((unsigned)cdiv(n, 256)), thr, 0, st, src, n, tgt, T, done, b.row_of,
                           have_prev ? b.idx_cur : (const int32_t *)nullptr, mode >= 0 ? max_d2 : 0.0, b.sort_t.bbox, b.init_val, b.init_idx,
                           b.A64, b.K64);
        {
            ProfScope prof(KPX_PROF_NN_LOCAL, 0.0, st);
            hipLaunchKernelGGL(nn_local_kernel, dim3((unsigned)cdiv(n, kLRows)), dim3(64), 0, st, n, b.Bs, b.orig_t, b.tile_box, b.group_box,
                               p.l_groups, b.sort_t.bbox, done, b.A64, b.K64, b.init_val, b.init_idx, b.row_of, b.part_val, b.part_idx,
                               prof_armed() ? nn_visits_ptr() : (unsigned long long *)nullptr);
        }
        hipLaunchKernelGGL(nn_merge_kernel<Terms>, dim3((unsigned)cdiv(n, kMergeThreads)), dim3(kMergeThreads), 0, st, src, n, tgt, tn, T, done,
                           b.part_val, b.part_idx, 1, max_d2, mode, b.idx_cur, b.d2_cur, (double *)nullptr, b.part_acc,
                           (const int32_t *)nullptr, (const int32_t *)nullptr, ct);
        KPX_LAUNCH_CHECK();
        return KPX_OK;
    }
    const bool screen = have_prev && allow_screen && screening_enabled();
    hipLaunchKernelGGL(nn_rowprep_kernel, dim3((unsigned)cdiv(n, 256)), thr, 0, st, src, n, tgt, T, done,
                       have_prev ? b.idx_cur : (const int32_t *)nullptr, screen ? b.aux : (const NnAux *)nullptr, b.init_val, b.init_idx,
                       b.A64, b.K64, b.A32, b.thr32, b.cand_cnt);
    if (screen) {
        {
            ProfScope prof(KPX_PROF_NN_SCREEN, 8.0 * (double)p.n_src * (double)p.n_tgt, st);   // 4 MAC per (source, target) pair
            hipLaunchKernelGGL((nn_screen_kernel<4, 3>), dim3(p.f_row_blocks, p.f_splits), thr, 0, st, n, b.Bf, p.f_tiles_per_split, done,
                               b.A32, b.thr32, b.init_idx, b.cand_cnt, b.cand, b.overflow);
        }
        hipLaunchKernelGGL(nn_overflow_kernel, dim3(1024), thr, 0, st, src, n, tgt,
                           p.n_tgt, T, done, b.cand_cnt, b.cand, b.overflow);
        hipLaunchKernelGGL(nn_merge_kernel<Terms>, dim3((unsigned)cdiv(n, kMergeThreads)), dim3(kMergeThreads), 0, st, src, n, tgt, tn, T, done, b.init_val, b.init_idx, 1,
                           max_d2, mode, b.idx_cur, b.d2_cur, (double *)nullptr, b.part_acc, b.cand_cnt, b.cand, ct);
        KPX_LAUNCH_CHECK();
        return KPX_OK;
    }
    {
    // (timed as ONE unit: a bare search's seed sweep + its merge belong to the all-pairs sweep they make cheaper -- with bounds from
    // every 16th tile the main sweep alone runs at 38 TFLOP/s, from every 64th at 33, but the seed sweep costs what it saves beyond that)
    ProfScope prof(KPX_PROF_NN_MFMA, 8.0 * (double)p.n_src * (double)p.n_tgt, st);     // 4 MAC per (source, target) pair
    if (!have_prev) {
        hipLaunchKernelGGL(nn_mfma_kernel, dim3(p.row_blocks, 1), thr, 0, st, n, b.Bseed, b.colSeed, (int32_t)p.seed_tiles_pad,
                           done, b.A64, b.K64, (const double *)nullptr, (const int32_t *)nullptr, b.part_val, b.part_idx, b.row_of);
        hipLaunchKernelGGL(nn_merge_kernel<ColorTerms>, dim3((unsigned)cdiv(n, kMergeThreads)), dim3(kMergeThreads), 0, st, src, n, tgt, tn, T, done, b.part_val, b.part_idx, 1,
                           0.0, -2, b.init_idx, (double *)nullptr, b.init_val, b.part_acc, (const int32_t *)nullptr, (const int32_t *)nullptr,
                           ColorTerms{});
    }
    // (b.row_of: nn_prep_source put the rows in the source's curve order)
    hipLaunchKernelGGL(nn_mfma_kernel, dim3(p.row_blocks, p.splits), thr, 0, st, n, b.B, b.colB, p.tiles_per_split, done, b.A64, b.K64,
                       b.init_val, b.init_idx, b.part_val, b.part_idx, b.row_of);
    }
    hipLaunchKernelGGL(nn_merge_kernel<Terms>, dim3((unsigned)cdiv(n, kMergeThreads)), dim3(kMergeThreads), 0, st, src, n, tgt, tn, T, done, b.part_val, b.part_idx,
                       p.splits, max_d2, mode, b.idx_cur, b.d2_cur, (double *)nullptr, b.part_acc, (const int32_t *)nullptr,
                       (const int32_t *)nullptr, ct);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

// What every entry point for one pair of clouds starts with: the workspace carved (`extra` doubles behind the search's buffers), the
// state initialised from h_init (null: a bare search has no state) and both clouds prepared for the engine in use.
struct NnProblem {
    NnPlan p;
    NnBuffers b;
    double *extra;
    void carve(Arena &a, int64_t n_src, int64_t n_tgt, size_t extra_doubles)
    {
        p = nn_plan(n_src, n_tgt);
        nn_carve(a, n_src, n_tgt, p, &b);
        extra = a.get<double>(extra_doubles);
    }
    int setup(const float *src, int64_t n_src, const float *tgt, int64_t n_tgt, const double *h_init, void *ws, size_t ws_bytes, hipStream_t st,
              size_t extra_doubles = 0)
    {
        Arena a(ws, ws_bytes);
        carve(a, n_src, n_tgt, extra_doubles);
        KPX_ARENA_CHECK(a);
        if (h_init) hipLaunchKernelGGL(icp_init_kernel, dim3(1), dim3(1), 0, st, b.state, mat16_from(h_init));
        const int rc = nn_prep(tgt, p, b, st);
        return rc ? rc : nn_prep_source(src, p, b, st);
    }
    // the last search's correspondences, to the callers that asked for them
    int copy_pairs(int32_t *idx, double *d2, hipStream_t st) const
    {
        if (idx) KPX_HIP(hipMemcpyAsync(idx, b.idx_cur, (size_t)p.n_src * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        if (d2) KPX_HIP(hipMemcpyAsync(d2, b.d2_cur, (size_t)p.n_src * sizeof(double), hipMemcpyDeviceToDevice, st));
        return KPX_OK;
    }
};

// When a search of the all-pairs engine may take the float32 screening sweep (the culled engine has none): never; from the third
// search on; or, kByPolicy, as ScreenPolicy finds the registration calm where every iteration is polled and from the third search on
// where not.
enum class Screen { kNever, kFromThird, kByPolicy };
struct IcpCriteria {
    int max_iteration;
    double relative_fitness, relative_rmse;
    int poll_interval;
};
// The registration loop of three launches and more per iteration: the search with the sums of nn_merge_kernel<Terms> (merge_mode),
// then icp_solve_kernel (solve_mode).  Kernels queued behind a raised `done` return at once, so the flag is only read back every
// poll_interval iterations (0 = never); kByPolicy reads the whole tail of the state, for ScreenPolicy.
template <class Terms>
static int icp_search_solve_loop(const float *src, const float *tgt, const float *tn, const NnProblem &q, double md2, int merge_mode, int solve_mode,
                                 Screen screen, const IcpCriteria &c, double *d_result, hipStream_t st, Terms terms = Terms{})
{
    const NnBuffers &b = q.b;
    ScreenPolicy policy;
    for (int k = 0; k <= c.max_iteration; ++k) {
        // (ScreenPolicy judges by the fitness and rmse of every iteration: it has them only where every iteration is polled)
        const bool allow_screen = screen == Screen::kByPolicy && c.poll_interval == 1 ? policy.allow(k) : screen != Screen::kNever && k >= 2;
        const int rc = nn_search_launch<Terms>(src, tgt, tn, q.p, b, b.state->T, &b.state->done, k > 0, allow_screen, md2, merge_mode, st, terms);
        if (rc) return rc;
        hipLaunchKernelGGL(icp_solve_kernel, dim3(1), dim3(kSolveThreads), 0, st, b.part_acc, (int)cdiv(q.p.n_src, kMergeThreads), q.p.n_src, solve_mode,
                           k, c.max_iteration, c.relative_fitness, c.relative_rmse, b.state, d_result);
        if (c.poll_interval > 0 && (k + 1) % c.poll_interval == 0 && k < c.max_iteration) {
            // One copy from the device's state into the same bytes of h_state: everything from `fitness` on where the policy observes,
            // the word `done` alone elsewhere.  Only what was copied is read below.
            const bool tail = screen == Screen::kByPolicy;
            const size_t at = tail ? offsetof(IcpState, fitness) : offsetof(IcpState, done);
            IcpState h_state = {};
            KPX_HIP(hipMemcpyAsync((char *)&h_state + at, (const char *)b.state + at, tail ? sizeof(IcpState) - at : sizeof(int32_t),
                                   hipMemcpyDeviceToHost, st));
            KPX_HIP(hipStreamSynchronize(st));
            if (h_state.done) break;
            if (tail) policy.observe(h_state.fitness, h_state.rmse);
        }
    }
    return KPX_OK;
}

}  // namespace kpx

using namespace kpx;

KPX_EXPORT int kpx_prof_icp_waves(uint64_t *h_out, int64_t cap_waves, int64_t *h_count)
{
    KPX_REQUIRE(h_out && h_count && cap_waves >= 0, "kpx_prof_icp_waves: null pointer or negative capacity");
    *h_count = icp_wave_take((unsigned long long *)h_out, cap_waves);
    return *h_count < 0 ? KPX_ERR_HIP : KPX_OK;
}

KPX_EXPORT int kpx_prof_icp_cert(uint64_t *h_out8)
{
    KPX_REQUIRE(h_out8, "kpx_prof_icp_cert: null pointer");
    unsigned long long *p = nullptr;
    static const unsigned long long zero[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    KPX_HIP(hipGetSymbolAddress((void **)&p, HIP_SYMBOL(g_cert_check)));
    KPX_HIP(hipMemcpy(h_out8, p, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    KPX_HIP(hipMemcpy(p, zero, sizeof(zero), hipMemcpyHostToDevice));
    return KPX_OK;
}
KPX_EXPORT int kpx_icp_chain(int32_t on)
{
    if (on == -2) return __atomic_load_n(&g_chain_launches, __ATOMIC_RELAXED);
    const int cur = chain_form_on() ? 1 : 0;
    if (on >= 0) g_chain_form = on ? 1 : 0;
    return cur;
}
// The chain clock (g_chain_stamp): 64 x 16 words, read and reset ([10], the earliest-block slot, to all ones)
KPX_EXPORT int kpx_prof_icp_chain(uint64_t *h_out3072)
{
    KPX_REQUIRE(h_out3072, "kpx_prof_icp_chain: null pointer");
    unsigned long long *p = nullptr;
    static unsigned long long init[64 * 48];
    for (int i = 0; i < 64 * 48; ++i) init[i] = (i % 48) == 10 ? ~0ull : 0ull;
    KPX_HIP(hipGetSymbolAddress((void **)&p, HIP_SYMBOL(g_chain_stamp)));
    KPX_HIP(hipMemcpy(h_out3072, p, sizeof(init), hipMemcpyDeviceToHost));
    KPX_HIP(hipMemcpy(p, init, sizeof(init), hipMemcpyHostToDevice));
    return KPX_OK;
}
KPX_EXPORT int kpx_prof_icp_phases(double *h_out8)
{
    KPX_REQUIRE(h_out8, "kpx_prof_icp_phases: null pointer");
    return icp_phase_take(h_out8);
}
KPX_EXPORT int kpx_nn_engine(int32_t engine)
{
    const int cur = local_engine() ? KPX_NN_ENGINE_CULLED : (g_nn_fp64_only ? KPX_NN_ENGINE_DENSE_FP64 : KPX_NN_ENGINE_DENSE);
    if (engine < 0) return cur;
    KPX_REQUIRE(engine == KPX_NN_ENGINE_CULLED || engine == KPX_NN_ENGINE_DENSE || engine == KPX_NN_ENGINE_DENSE_FP64, "kpx_nn_engine: unknown engine %d", engine);
    g_nn_engine = engine == KPX_NN_ENGINE_CULLED ? KPX_NN_ENGINE_CULLED : KPX_NN_ENGINE_DENSE;
    g_nn_fp64_only = engine == KPX_NN_ENGINE_DENSE_FP64;
    return cur;
}

KPX_EXPORT size_t kpx_nn_workspace_bytes(int64_t n_src, int64_t n_tgt)
{
    Arena a(nullptr, 0);
    NnBuffers b;
    nn_carve(a, n_src, n_tgt, nn_plan(n_src, n_tgt), &b);
    return a.off;
}
KPX_EXPORT int kpx_nn_search(const float *src, int64_t n_src, const float *tgt, int64_t n_tgt, const double *d_T, int32_t *idx,
                             double *d2, void *ws, size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(n_src >= 0 && n_tgt >= 1, "kpx_nn_search: empty target");
    KPX_REQUIRE(n_src < ((int64_t)1 << 31) && n_tgt < ((int64_t)1 << 31) - 65536, "kpx_nn_search: cloud too large");
    if (n_src == 0) return KPX_OK;
    KPX_REQUIRE(src && tgt && d_T && idx && d2 && ws, "kpx_nn_search: null pointer");
    hipStream_t st = (hipStream_t)stream;
    NnProblem q;
    int rc = q.setup(src, n_src, tgt, n_tgt, nullptr, ws, ws_bytes, st);
    if (rc) return rc;
    rc = nn_search_launch(src, tgt, nullptr, q.p, q.b, d_T, nullptr, false, false, 0.0, -1, st);
    return rc ? rc : q.copy_pairs(idx, d2, st);
}

// ---- evaluate_registration + get_information_matrix_from_point_clouds in one pass ---------------------------------------
// After the correspondence search: over the rows that pass the distance test of the ICP accumulation (d2 < max_dist^2, strict),
// eleven fp64 sums -- count, sum d2, and the moments of the MATCHED TARGET points t = tgt[idx]: sum t (3), sum t t^T (6).
// Rounding: a float32 coordinate converts to fp64 exactly and the product of two of them (<= 48 significant bits) is exact in
// fp64, so the only rounding in the ten moment sums is that of the additions (d2 comes from the search as it is).  Order of the
// additions: a thread's rows in grid-stride order, the 64 lanes by the wave tree (wave_sum), the block's waves in order
// (block_sum), the blocks in order (regeval_finish_kernel) -- fixed by (n, grid), no floating-point atomics, so equal idx / d2
// give equal bits whichever engine searched.
// The gathers of t are n random 12-byte loads; the kernel is a few microseconds beside the search.
constexpr int kEvalSums = 11, kEvalBlocks = 256, kEvalThreads = 256, kEvalPartials = kEvalBlocks * kEvalSums;      // (partials: doubles, NnProblem::extra)
__global__ __launch_bounds__(kEvalThreads) void regeval_acc_kernel(const float *__restrict__ tgt, int64_t n, int64_t m, const int32_t *__restrict__ idx,
                                                                  const double *__restrict__ d2, double max_d2, double *__restrict__ part)
{
    __shared__ double sh[kEvalThreads / 64];
    double acc[kEvalSums];
#pragma unroll
    for (int q = 0; q < kEvalSums; ++q) acc[q] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = idx[i];
        const double d = d2[i];
        if (j < 0 || j >= m || !(d < max_d2)) continue;
        const float *tp = tgt + 3 * j;
        const double x = tp[0], y = tp[1], z = tp[2];
        acc[0] += 1.0; acc[1] += d;
        acc[2] += x; acc[3] += y; acc[4] += z;
        acc[5] += x * x; acc[6] += x * y; acc[7] += x * z;
        acc[8] += y * y; acc[9] += y * z; acc[10] += z * z;
    }
#pragma unroll
    for (int q = 0; q < kEvalSums; ++q) {
        const double v = block_sum(acc[q], sh);
        if (threadIdx.x == 0) part[(int64_t)blockIdx.x * kEvalSums + q] = v;
    }
}
// result f64 [40]: fitness, inlier_rmse, count, sum d2, then the 6x6 information matrix row-major (rotation block first).
// Every entry is one sum, the sum of two (the diagonal of the rotation block, from sum x^2, sum y^2, sum z^2 -- never a
// difference) or a negation.
__global__ __launch_bounds__(64) void regeval_finish_kernel(const double *__restrict__ part, int nblocks, int64_t n, double *__restrict__ res)
{
    __shared__ double S[kEvalSums];
    if (threadIdx.x < kEvalSums) {
        double s = 0.0;
        for (int b = 0; b < nblocks; ++b) s += part[(int64_t)b * kEvalSums + threadIdx.x];
        S[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x >= 40) return;
    const double cnt = S[0], sx = S[2], sy = S[3], sz = S[4], xx = S[5], xy = S[6], xz = S[7], yy = S[8], yz = S[9], zz = S[10];
    const double L[36] = { yy + zz, -xy, -xz, 0.0, -sz, sy,
                           -xy, xx + zz, -yz, sz, 0.0, -sx,
                           -xz, -yz, xx + yy, -sy, sx, 0.0,
                           0.0, sz, -sy, cnt, 0.0, 0.0,
                           -sz, 0.0, sx, 0.0, cnt, 0.0,
                           sy, -sx, 0.0, 0.0, 0.0, cnt };
    const int q = threadIdx.x;
    double v;
    if (q == 0) v = n > 0 ? cnt / (double)n : 0.0;
    else if (q == 1) v = cnt > 0.0 ? sqrt(S[1] / cnt) : 0.0;
    else if (q == 2) v = cnt;
    else if (q == 3) v = S[1];
    else v = L[q - 4] + 0.0;                                   // + 0.0: no negative zeros in the matrix
    res[q] = v;
}

KPX_EXPORT size_t kpx_registration_eval_workspace_bytes(int64_t n_src, int64_t n_tgt)
{
    Arena a(nullptr, 0);
    NnProblem q;
    q.carve(a, n_src, n_tgt, kEvalPartials);
    return a.off;
}
KPX_EXPORT int kpx_registration_eval(const float *src, int64_t n_src, const float *tgt, int64_t n_tgt, const double *d_T,
                                     double max_dist, double *d_result, int32_t *idx, double *d2, void *ws, size_t ws_bytes,
                                     void *stream)
{
    KPX_REQUIRE(max_dist > 0.0, "Invalid max_correspondence_distance.");          // [O3D]
    KPX_REQUIRE(n_src >= 1 && n_tgt >= 1, "kpx_registration_eval: empty cloud");
    KPX_REQUIRE(n_src < ((int64_t)1 << 31) && n_tgt < ((int64_t)1 << 31) - 65536, "kpx_registration_eval: cloud too large");
    KPX_REQUIRE(src && tgt && d_T && d_result && ws, "kpx_registration_eval: null pointer");
    hipStream_t st = (hipStream_t)stream;
    NnProblem q;
    int rc = q.setup(src, n_src, tgt, n_tgt, nullptr, ws, ws_bytes, st, kEvalPartials);      // (the state is not used)
    if (rc) return rc;
    rc = nn_search_launch(src, tgt, nullptr, q.p, q.b, d_T, nullptr, false, false, 0.0, -1, st);      // as kpx_nn_search: the engine kpx_nn_engine selects
    if (rc) return rc;
    double *part = q.extra;
    const int nb = (int)(cdiv(n_src, kEvalThreads) > kEvalBlocks ? kEvalBlocks : cdiv(n_src, kEvalThreads));
    hipLaunchKernelGGL(regeval_acc_kernel, dim3(nb), dim3(kEvalThreads), 0, st, tgt, n_src, n_tgt, q.b.idx_cur, q.b.d2_cur, max_dist * max_dist, part);
    hipLaunchKernelGGL(regeval_finish_kernel, dim3(1), dim3(64), 0, st, part, nb, n_src, d_result);
    KPX_LAUNCH_CHECK();
    return q.copy_pairs(idx, d2, st);
}

static double *kabsch_carve(Arena &a) { return a.get<double>((size_t)256 * kAcc); }      // pairs_acc_kernel's partial sums, one row per block
KPX_EXPORT size_t kpx_kabsch_workspace_bytes(int64_t n_corr)
{
    Arena a(nullptr, 0);
    kabsch_carve(a);
    return a.off;
}
KPX_EXPORT int kpx_kabsch(const float *src, const float *tgt, const int32_t *corr, int64_t n_corr, double *d_T, void *ws,
                          size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(n_corr >= 0 && d_T && ws, "kpx_kabsch: bad arguments");
    KPX_REQUIRE(n_corr == 0 || (src && tgt && corr), "kpx_kabsch: null pointer");
    hipStream_t st = (hipStream_t)stream;
    Arena a(ws, ws_bytes);
    double *part = kabsch_carve(a);
    KPX_ARENA_CHECK(a);
    int nb = (int)(cdiv(n_corr > 0 ? n_corr : 1, 256) > 256 ? 256 : cdiv(n_corr > 0 ? n_corr : 1, 256));
    hipLaunchKernelGGL(pairs_acc_kernel, dim3(nb), dim3(256), 0, st, src, tgt, corr, n_corr, part);
    hipLaunchKernelGGL(pairs_solve_kernel, dim3(1), dim3(64), 0, st, part, nb, d_T);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT size_t kpx_icp_workspace_bytes(int64_t n_src, int64_t n_tgt)
{
    return kpx_nn_workspace_bytes(n_src, n_tgt);
}
// The robust entry points' own checks (Open3D does not check k: a deviation, see include/kinectpx.h).
static int loss_check(int32_t loss, double loss_k)
{
    KPX_REQUIRE(loss >= KPX_LOSS_L2 && loss <= KPX_LOSS_TUKEY, "unknown robust loss kind %d", loss);
    KPX_REQUIRE(loss == KPX_LOSS_L2 || loss == KPX_LOSS_L1 || loss_k > 0.0, "the robust loss's k must be positive");
    return KPX_OK;
}
// kpx_icp (loss == nullptr) and kpx_icp_robust: a robust registration is point-to-plane and takes the three-launch loop with the
// weighted sums of nn_merge_kernel<RobustColorTerms> on BOTH engines -- never the culled engine's one-launch iteration, whose
// fixed-point sums are not sized for unbounded weights.
static int icp_run(const float *src, int64_t n_src, const float *tgt, const float *tgt_normals, int64_t n_tgt,
                   double max_dist, const double *h_init, int32_t mode, int32_t max_iteration, double relative_fitness,
                   double relative_rmse, int32_t poll_interval, double *d_result, int32_t *idx, double *d2, void *ws,
                   size_t ws_bytes, void *stream, const RobustLoss *loss)
{
    KPX_REQUIRE(mode == KPX_ICP_POINT_TO_POINT || mode == KPX_ICP_POINT_TO_PLANE, "kpx_icp: unknown estimation mode");
    KPX_REQUIRE(mode != KPX_ICP_POINT_TO_PLANE || tgt_normals,
                "TransformationEstimationPointToPlane and TransformationEstimationColoredICP require pre-computed normal vectors for target PointCloud.");
    KPX_REQUIRE(max_dist > 0.0, "Invalid max_correspondence_distance.");          // [O3D]
    KPX_REQUIRE(n_src >= 1 && n_tgt >= 1 && max_iteration >= 0, "kpx_icp: empty cloud");
    KPX_REQUIRE(n_src < ((int64_t)1 << 31) && n_tgt < ((int64_t)1 << 31) - 65536, "kpx_icp: cloud too large");
    KPX_REQUIRE(src && tgt && h_init && d_result && ws, "kpx_icp: null pointer");
    hipStream_t st = (hipStream_t)stream;
    NnProblem q;
    int rc = q.setup(src, n_src, tgt, n_tgt, h_init, ws, ws_bytes, st);
    if (rc) return rc;
    const NnPlan &p = q.p;
    const NnBuffers &b = q.b;
    const double md2 = max_dist * max_dist;
    if (loss) {
        rc = icp_search_solve_loop(src, tgt, tgt_normals, q, md2, 1, 1, Screen::kByPolicy,
                                   IcpCriteria{ max_iteration, relative_fitness, relative_rmse, poll_interval }, d_result, st,
                                   RobustColorTerms{ ColorTerms{}, *loss });
        if (rc) return rc;
    } else if (local_engine()) {
        // one launch per iteration; kernels queued behind a raised `done` return at once, so the flag is only read back
        // every poll_interval iterations (0 = never)
        for (int k = 0; k <= max_iteration; ++k) {
            icp_iter_launch(src, tgt, tgt_normals, p, b, md2, mode, k, max_iteration, relative_fitness, relative_rmse, d_result, st, nullptr, 0,
                            idx != nullptr || d2 != nullptr);
            if (poll_interval > 0 && (k + 1) % poll_interval == 0 && k < max_iteration) {
                int32_t h_done = 0;
                KPX_HIP(hipMemcpyAsync(&h_done, &b.state->done, sizeof(int32_t), hipMemcpyDeviceToHost, st));
                KPX_HIP(hipStreamSynchronize(st));
                if (h_done) break;
            }
        }
    } else {
        rc = icp_search_solve_loop<ColorTerms>(src, tgt, tgt_normals, q, md2, mode, mode, Screen::kByPolicy,
                                               IcpCriteria{ max_iteration, relative_fitness, relative_rmse, poll_interval }, d_result, st);
        if (rc) return rc;
    }
    rc = q.copy_pairs(idx, d2, st);
    if (rc) return rc;
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}
KPX_EXPORT int kpx_icp(const float *src, int64_t n_src, const float *tgt, const float *tgt_normals, int64_t n_tgt,
                       double max_dist, const double *h_init, int32_t mode, int32_t max_iteration, double relative_fitness,
                       double relative_rmse, int32_t poll_interval, double *d_result, int32_t *idx, double *d2, void *ws,
                       size_t ws_bytes, void *stream)
{
    return icp_run(src, n_src, tgt, tgt_normals, n_tgt, max_dist, h_init, mode, max_iteration, relative_fitness, relative_rmse, poll_interval,
                   d_result, idx, d2, ws, ws_bytes, stream, nullptr);
}
KPX_EXPORT int kpx_icp_robust(const float *src, int64_t n_src, const float *tgt, const float *tgt_normals, int64_t n_tgt,
                              double max_dist, const double *h_init, int32_t mode, int32_t max_iteration, double relative_fitness,
                              double relative_rmse, int32_t poll_interval, double *d_result, int32_t *idx, double *d2, void *ws,
                              size_t ws_bytes, void *stream, int32_t loss, double loss_k)
{
    KPX_REQUIRE(mode != KPX_ICP_POINT_TO_POINT,
                "kpx_icp_robust: TransformationEstimationPointToPoint takes no robust kernel; use KPX_ICP_POINT_TO_PLANE");
    const int rc = loss_check(loss, loss_k);
    if (rc) return rc;
    const RobustLoss rl{ loss, loss_k };
    return icp_run(src, n_src, tgt, tgt_normals, n_tgt, max_dist, h_init, mode, max_iteration, relative_fitness, relative_rmse, poll_interval,
                   d_result, idx, d2, ws, ws_bytes, stream, &rl);
}

// ---- coloured ICP (preprocessing/registration.py:89-114) -----------------------------------------------------
// [O3D] registration_colored_icp = the registration_icp loop (same correspondences, fitness, inlier rmse and convergence
// test) with TransformationEstimationForColoredICP as the update; the target's colour gradient comes from
// kpx_color_gradient.  Search -> sums -> solve are three launches per iteration (nn_merge_kernel mode 2 + icp_solve_kernel):
// the function is unused in the reference, so this path is built for parity, not for speed.
KPX_EXPORT size_t kpx_colored_icp_workspace_bytes(int64_t n_src, int64_t n_tgt) { return kpx_icp_workspace_bytes(n_src, n_tgt); }
static int colored_icp_run(const float *src, const float *src_colors, int64_t n_src, const float *tgt, const float *tgt_colors,
                           const float *tgt_normals, const double *tgt_gradient, int64_t n_tgt, double max_dist, const double *h_init,
                           double lambda_geometric, int32_t max_iteration, double relative_fitness, double relative_rmse,
                           int32_t poll_interval, double *d_result, void *ws, size_t ws_bytes, void *stream, const RobustLoss *loss)
{
    KPX_REQUIRE(tgt_normals, "TransformationEstimationPointToPlane and TransformationEstimationColoredICP require pre-computed normal vectors for target PointCloud.");
    KPX_REQUIRE(src_colors && tgt_colors && tgt_gradient, "kpx_colored_icp: colours of both clouds and the target's colour gradient are required");
    KPX_REQUIRE(max_dist > 0.0, "Invalid max_correspondence_distance.");
    KPX_REQUIRE(lambda_geometric >= 0.0 && lambda_geometric <= 1.0, "kpx_colored_icp: lambda_geometric must lie in [0, 1]");
    KPX_REQUIRE(n_src >= 1 && n_tgt >= 1 && max_iteration >= 0, "kpx_colored_icp: empty cloud");
    KPX_REQUIRE(n_src < ((int64_t)1 << 31) && n_tgt < ((int64_t)1 << 31) - 65536, "kpx_colored_icp: cloud too large");
    KPX_REQUIRE(src && tgt && h_init && d_result && ws, "kpx_colored_icp: null pointer");
    hipStream_t st = (hipStream_t)stream;
    NnProblem q;
    int rc = q.setup(src, n_src, tgt, n_tgt, h_init, ws, ws_bytes, st);
    if (rc) return rc;
    const ColorTerms ct{ src_colors, tgt_colors, tgt_gradient, sqrt(lambda_geometric), sqrt(1.0 - lambda_geometric) };
    const IcpCriteria crit{ max_iteration, relative_fitness, relative_rmse, poll_interval };
    rc = loss ? icp_search_solve_loop(src, tgt, tgt_normals, q, max_dist * max_dist, 2, 1, Screen::kNever, crit, d_result, st,
                                      RobustColorTerms{ ct, *loss })
              : icp_search_solve_loop(src, tgt, tgt_normals, q, max_dist * max_dist, 2, 1, Screen::kNever, crit, d_result, st, ct);
    if (rc) return rc;
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}
KPX_EXPORT int kpx_colored_icp(const float *src, const float *src_colors, int64_t n_src, const float *tgt, const float *tgt_colors,
                               const float *tgt_normals, const double *tgt_gradient, int64_t n_tgt, double max_dist, const double *h_init,
                               double lambda_geometric, int32_t max_iteration, double relative_fitness, double relative_rmse,
                               int32_t poll_interval, double *d_result, void *ws, size_t ws_bytes, void *stream)
{
    return colored_icp_run(src, src_colors, n_src, tgt, tgt_colors, tgt_normals, tgt_gradient, n_tgt, max_dist, h_init, lambda_geometric,
                           max_iteration, relative_fitness, relative_rmse, poll_interval, d_result, ws, ws_bytes, stream, nullptr);
}
KPX_EXPORT int kpx_colored_icp_robust(const float *src, const float *src_colors, int64_t n_src, const float *tgt, const float *tgt_colors,
                                      const float *tgt_normals, const double *tgt_gradient, int64_t n_tgt, double max_dist,
                                      const double *h_init, double lambda_geometric, int32_t max_iteration, double relative_fitness,
                                      double relative_rmse, int32_t poll_interval, double *d_result, void *ws, size_t ws_bytes,
                                      void *stream, int32_t loss, double loss_k)
{
    const int rc = loss_check(loss, loss_k);
    if (rc) return rc;
    const RobustLoss rl{ loss, loss_k };
    return colored_icp_run(src, src_colors, n_src, tgt, tgt_colors, tgt_normals, tgt_gradient, n_tgt, max_dist, h_init, lambda_geometric,
                           max_iteration, relative_fitness, relative_rmse, poll_interval, d_result, ws, ws_bytes, stream, &rl);
}

// ---- generalized ICP ----------------------------------------------------------------------------------------------------------
// [O3D] registration_generalized_icp = the registration_icp loop (same correspondences, fitness, inlier rmse, convergence test and
// iteration count) with TransformationEstimationForGeneralizedICP as the update (gicp_pair_rows; kpx_generalized_icp_robust weights
// its rows by a robust loss).  Search -> sums ->
// solve per iteration as kpx_colored_icp (nn_merge_kernel<GicpTerms> + icp_solve_kernel in its point-to-plane mode), on whichever
// engine kpx_nn_engine selected; the all-pairs engine screens from the third search on, as kpx_icp does.  The covariances come from
// kpx_estimate_covariances or kpx_gicp_covariances; the source's stay in the original frame and are rotated by the current T per pair.
// An iteration whose 6x6 system is singular takes the identity update (solve6_ldlt), as a pair with a singular M adds nothing.
KPX_EXPORT size_t kpx_generalized_icp_workspace_bytes(int64_t n_src, int64_t n_tgt) { return kpx_icp_workspace_bytes(n_src, n_tgt); }
static int generalized_icp_run(const float *src, const double *src_cov, int64_t n_src, const float *tgt, const double *tgt_cov, int64_t n_tgt,
                               double max_dist, const double *h_init, int32_t max_iteration, double relative_fitness, double relative_rmse,
                               int32_t poll_interval, double *d_result, int32_t *idx, double *d2, void *ws, size_t ws_bytes, void *stream,
                               const RobustLoss *loss)
{
    KPX_REQUIRE(src_cov && tgt_cov, "kpx_generalized_icp: covariances of both clouds are required");
    KPX_REQUIRE(max_dist > 0.0, "Invalid max_correspondence_distance.");          // [O3D]
    KPX_REQUIRE(n_src >= 1 && n_tgt >= 1 && max_iteration >= 0, "kpx_generalized_icp: empty cloud");
    KPX_REQUIRE(n_src < ((int64_t)1 << 31) && n_tgt < ((int64_t)1 << 31) - 65536, "kpx_generalized_icp: cloud too large");
    KPX_REQUIRE(src && tgt && h_init && d_result && ws, "kpx_generalized_icp: null pointer");
    hipStream_t st = (hipStream_t)stream;
    NnProblem q;
    int rc = q.setup(src, n_src, tgt, n_tgt, h_init, ws, ws_bytes, st);
    if (rc) return rc;
    const IcpCriteria crit{ max_iteration, relative_fitness, relative_rmse, poll_interval };
    const GicpTerms gt{ src_cov, tgt_cov };
    rc = loss ? icp_search_solve_loop(src, tgt, nullptr, q, max_dist * max_dist, kModeGicp, 1, Screen::kFromThird, crit, d_result, st,
                                      RobustGicpTerms{ gt, *loss })
              : icp_search_solve_loop(src, tgt, nullptr, q, max_dist * max_dist, kModeGicp, 1, Screen::kFromThird, crit, d_result, st, gt);
    if (rc) return rc;
    rc = q.copy_pairs(idx, d2, st);
    if (rc) return rc;
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}
KPX_EXPORT int kpx_generalized_icp(const float *src, const double *src_cov, int64_t n_src, const float *tgt, const double *tgt_cov, int64_t n_tgt,
                                   double max_dist, const double *h_init, int32_t max_iteration, double relative_fitness, double relative_rmse,
                                   int32_t poll_interval, double *d_result, int32_t *idx, double *d2, void *ws, size_t ws_bytes, void *stream)
{
    return generalized_icp_run(src, src_cov, n_src, tgt, tgt_cov, n_tgt, max_dist, h_init, max_iteration, relative_fitness, relative_rmse,
                               poll_interval, d_result, idx, d2, ws, ws_bytes, stream, nullptr);
}
KPX_EXPORT int kpx_generalized_icp_robust(const float *src, const double *src_cov, int64_t n_src, const float *tgt, const double *tgt_cov,
                                          int64_t n_tgt, double max_dist, const double *h_init, int32_t max_iteration, double relative_fitness,
                                          double relative_rmse, int32_t poll_interval, double *d_result, int32_t *idx, double *d2, void *ws,
                                          size_t ws_bytes, void *stream, int32_t loss, double loss_k)
{
    const int rc = loss_check(loss, loss_k);
    if (rc) return rc;
    const RobustLoss rl{ loss, loss_k };
    return generalized_icp_run(src, src_cov, n_src, tgt, tgt_cov, n_tgt, max_dist, h_init, max_iteration, relative_fitness, relative_rmse,
                               poll_interval, d_result, idx, d2, ws, ws_bytes, stream, &rl);
}

// [O3D] InitializePointCloudForGeneralizedICP, covariances from normals: C = R_x diag(eps, 1, 1) R_x^T with R_x = GetRotationFromE1ToX(n),
// evaluated literally -- v = e1 x n, c = e1 . n; c < -0.99: R_x = I (Open3D's branch, kept); else R_x = I + [v]x + [v]x^2 / (1 + c).
// One thread per point, fp64 from the float32 normal.
__global__ __launch_bounds__(256) void gicp_covariances_kernel(const float *__restrict__ normals, int64_t n, double eps, double *__restrict__ cov)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double nx = normals[3 * i], ny = normals[3 * i + 1], nz = normals[3 * i + 2];
    double R[9] = { 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0 };
    const double c = nx;
    if (!(c < -0.99)) {
        const double v0 = 0.0, v1 = -nz, v2 = ny;                        // e1 x n
        const double S[9] = { 0.0, -v2, v1, v2, 0.0, -v0, -v1, v0, 0.0 };
        const double f = 1.0 / (1.0 + c);
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const double s2 = S[3 * p] * S[q] + S[3 * p + 1] * S[3 + q] + S[3 * p + 2] * S[6 + q];
                R[3 * p + q] = (R[3 * p + q] + S[3 * p + q]) + s2 * f;
            }
    }
    const double dg[3] = { eps, 1.0, 1.0 };
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q)
            cov[9 * i + 3 * p + q] = R[3 * p] * dg[0] * R[3 * q] + R[3 * p + 1] * dg[1] * R[3 * q + 1] + R[3 * p + 2] * dg[2] * R[3 * q + 2];
}
struct Rot9 {
    double r[9];
};
// out = R C R^T per point (PointCloud.transform with covariances); in == out allowed
__global__ __launch_bounds__(256) void rotate_covariances_kernel(const double *__restrict__ cov, int64_t n, Rot9 R, double *out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double C[9], RC[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) C[e] = cov[9 * i + e];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q) RC[3 * p + q] = R.r[3 * p] * C[q] + R.r[3 * p + 1] * C[3 + q] + R.r[3 * p + 2] * C[6 + q];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q) out[9 * i + 3 * p + q] = RC[3 * p] * R.r[3 * q] + RC[3 * p + 1] * R.r[3 * q + 1] + RC[3 * p + 2] * R.r[3 * q + 2];
}
KPX_EXPORT int kpx_gicp_covariances(const float *normals, int64_t n, double epsilon, double *cov, void *stream)
{
    KPX_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "kpx_gicp_covariances: bad size");
    if (n == 0) return KPX_OK;
    KPX_REQUIRE(normals && cov, "kpx_gicp_covariances: null pointer");
    hipLaunchKernelGGL(gicp_covariances_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, normals, n, epsilon, cov);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}
KPX_EXPORT int kpx_rotate_covariances(const double *cov, int64_t n, const double *h_T, double *out, void *stream)
{
    KPX_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "kpx_rotate_covariances: bad size");
    if (n == 0) return KPX_OK;
    KPX_REQUIRE(cov && h_T && out, "kpx_rotate_covariances: null pointer");
    Rot9 R;
    for (int p = 0; p < 3; ++p)
        for (int q = 0; q < 3; ++q) R.r[3 * p + q] = h_T[4 * p + q];
    hipLaunchKernelGGL(rotate_covariances_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, cov, n, R, out);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

// ---- several registrations onto one shared target -----------------------------------------------------------------
// (preprocessing/data.py:144-161 registers every sub device onto the same master cloud.)  The target operand is
// prepared once on the caller's stream; the problems then run side by side on internal lanes (their kernels are
// short and latency-bound: one problem alone leaves most of the chip idle), each with two chunks of iterations in
// flight and its state copied to pinned memory after every chunk, so neither the lanes nor the host wait for a round
// trip.  The caller's stream continues after all lanes have finished.
namespace kpx {
// The workspace of a batch (count <= kBatchMax), carved for the call and counted for the size query by the same lines: the target's
// operands once, padded for the largest split plan and shared by the buffers of every problem; each problem's own; and the scratch
// of the batch sort (ms) where that sort can take the target and the sources together.  -> whether it can
constexpr int kBatchMax = 64;
struct BatchLayout {
    NnPlan plans[kBatchMax], tplan;
    NnBuffers bufs[kBatchMax];
    MortonBatchScratch ms;
};
static bool batch_carve(Arena &a, int32_t count, const int64_t *h_n_src, int64_t n_tgt, BatchLayout *L)
{
    L->tplan = nn_plan(h_n_src[0], n_tgt);
    int64_t total_pts = n_tgt;
    for (int i = 0; i < count; ++i) {
        L->plans[i] = nn_plan(h_n_src[i], n_tgt);
        if (L->plans[i].tiles_pad > L->tplan.tiles_pad) L->tplan.tiles_pad = L->plans[i].tiles_pad;
        if (L->plans[i].f_tiles_pad > L->tplan.f_tiles_pad) L->tplan.f_tiles_pad = L->plans[i].f_tiles_pad;
        total_pts += h_n_src[i];
    }
    NnBuffers shared = {};
    nn_carve_target(a, L->tplan, &shared);
    for (int i = 0; i < count; ++i) {
        L->bufs[i] = shared;
        nn_carve_source(a, h_n_src[i], L->plans[i], &L->bufs[i]);
    }
    const bool can_batch_sort = count + 1 <= kMortonBatchMax && total_pts < ((int64_t)1 << 31);
    if (can_batch_sort) morton_batch_carve(a, total_pts, &L->ms);
    return can_batch_sort;
}
}  // namespace kpx
KPX_EXPORT size_t kpx_icp_batch_workspace_bytes(int32_t count, const int64_t *h_n_src, int64_t n_tgt)
{
    if (count < 1 || count > kBatchMax || !h_n_src) return 0;          // (a batch kpx_icp_batch refuses)
    Arena a(nullptr, 0);
    BatchLayout L;
    batch_carve(a, count, h_n_src, n_tgt, &L);
    return a.off;
}
KPX_EXPORT int kpx_icp_batch(int32_t count, const float *const *h_src, const int64_t *h_n_src, const float *tgt,
                             const float *tgt_normals, int64_t n_tgt, double max_dist, const double *h_init, int32_t mode,
                             int32_t max_iteration, double relative_fitness, double relative_rmse, double *d_results, void *ws,
                             size_t ws_bytes, void *stream)
{
    return kpx::icp_batch_ordered(count, h_src, h_n_src, tgt, tgt_normals, n_tgt, max_dist, h_init, mode, max_iteration, relative_fitness, relative_rmse,
                                  d_results, ws, ws_bytes, stream, false);
}
static int g_busy_threads = 0;
static thread_local int t_busy_depth = 0;
kpx::BusyScope::BusyScope() : counted(t_busy_depth++ == 0) { if (counted) __atomic_fetch_add(&g_busy_threads, 1, __ATOMIC_RELAXED); }
kpx::BusyScope::~BusyScope() { --t_busy_depth; if (counted) __atomic_fetch_sub(&g_busy_threads, 1, __ATOMIC_RELAXED); }
int kpx::busy_threads() { return __atomic_load_n(&g_busy_threads, __ATOMIC_RELAXED); }
// A chain kernel gave up waiting since the last call (see icp_chain_kernel): 1 once, then cleared
int kpx::icp_chain_abort_take()
{
    unsigned long long *w = chain_abort_word();
    if (!w) return 0;
    const unsigned long long v = __atomic_exchange_n(w, 0ull, __ATOMIC_ACQ_REL);
    return v ? 1 : 0;
}

namespace kpx {

// ---- the batch driver ---------------------------------------------------------------------------------------------------------------
// Host side of a launch window (both culled drivers).  Every update step publishes a word in pinned host memory:
//     generation (24 bits) << 40 | searched share in 1/127ths (7 bits) << 33 | converged << 32 | iterations finished (32 bits)
// and the driver keeps a window of launches queued ahead of what the words report.  The pinned block (64 words) belongs to the
// calling thread and is allocated once; a call's words carry its generation, so a late word of an earlier call reads as "nothing yet".
struct ProgressWindow {
    struct Word {
        bool converged;
        int seen;              // iterations finished, as far as the host knows
        int share;             // searched share of the last reported iteration (127 = all rows, also before the first report)
    };
    unsigned long long *words = nullptr, generation = 0;
    double stall_limit = 60.0;
    std::chrono::steady_clock::time_point t_last;

    int open(double stall_seconds)
    {
        ThreadResources &tr = thread_resources();
        words = static_cast<unsigned long long *>(tr.pinned(kPinIcpProgress, 64 * sizeof(unsigned long long)));
        if (!words) return KPX_ERR_HIP;
        generation = tr.icp_generation = (tr.icp_generation + 1) & 0xFFFFFFull;
        stall_limit = stall_seconds;
        t_last = std::chrono::steady_clock::now();
        return KPX_OK;
    }
    unsigned long long tag() const { return generation << 40; }
    void clear(int i) const { __atomic_store_n(&words[i], 0ull, __ATOMIC_RELAXED); }
    Word read(int i) const
    {
        const unsigned long long w = __atomic_load_n(&words[i], __ATOMIC_ACQUIRE);
        const bool mine = (w >> 40) == generation;
        const int seen = mine ? (int)(w & 0xFFFFFFFFull) : 0;
        return Word{ mine && ((w >> 32) & 1ull), seen, mine && seen >= 1 ? (int)((w >> 33) & 127ull) : 127 };
    }
    // after one pass over the problems.  "No progress" = no word advanced and nothing could be queued for `stall_limit` seconds (the
    // clock restarts on every advance: the lanes first wait for whatever the caller already queued on its stream, and a large batch
    // runs long)
    int pass_done(bool advanced, bool pending)
    {
        if (advanced) t_last = std::chrono::steady_clock::now();
        else if (pending) {
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t_last).count() > stall_limit)
                return fail(KPX_ERR_HIP, "kpx_icp_batch: no progress for %.0f s (KPX_ICP_STALL_SECONDS)", stall_limit);
            __builtin_ia32_pause();
        }
        return KPX_OK;
    }
};

// what the three drivers work on: the problems, their plans and buffers, the streams, the criteria
struct BatchCtx {
    int count;
    const float *const *h_src;
    const int64_t *h_n_src;
    const float *tgt, *tgt_normals;
    const double *h_init;
    double md2;
    int mode, max_iteration;
    double relative_fitness, relative_rmse;
    double *d_results;
    const NnPlan *plans, *tplan;
    const NnBuffers *bufs;
    bool ordered;              // clouds and target already lie in curve order (the batch sort)
    hipStream_t st;            // the caller's stream (drive_grouped runs on it: no fork / join events)
    hipStream_t *lanes;        // the per-problem drivers: problem i runs on lane(i)
    hipStream_t lane(int problem) const { return lanes[problem % kLaneCount]; }
};

// development aid (KPX_ICP_CHAIN_DUMP=1): the records of every registration of a one-launch chain, per iteration
static void chain_dump_records(const IcpBatchArgs &A, hipStream_t ls)
{
    (void)hipStreamSynchronize(ls);
    static double rec[kChainRecords * kChainRec];
    for (int c = 0; c < A.count; ++c) {
        (void)hipMemcpy(rec, A.p[c].chain_rec, sizeof(rec), hipMemcpyDeviceToHost);
        for (int k = 0; k < kChainRecords; ++k) {
            const IcpState *r = reinterpret_cast<const IcpState *>(rec + (size_t)kChainRec * k);
            unsigned long long w0;
            memcpy(&w0, r, 8);
            if (w0 == kChainEmpty) { fprintf(stderr, "chain problem %d record %d: empty\n", c, k); break; }
            fprintf(stderr, "chain problem %d record %d: iter %d done %d fitness %.9f rmse %.9f count %.0f T03 %.6f motion %.4f last %.4f reach %.3f\n", c, k, r->iter,
                    r->done, r->fitness, r->rmse, r->count, r->T[3], r->motion, r->last_motion, r->reach);
        }
    }
}

// Culled engine, clouds ordered by the batch sort: ONE chain of launches for all problems of the batch (icp_iter_batch_kernel /
// icp_rows_kernel), or the whole chain in one launch (icp_chain_kernel) where it may be resident; on the caller's stream.
// The batch sort orders the target and the sources together, so what it takes always fits one launch:
static_assert(kMortonBatchMax - 1 <= kIcpBatchMax, "a batch ordered by one sort is one group of launches");
static int drive_grouped(const BatchCtx &x)
{
    KPX_REQUIRE(x.count <= kIcpBatchMax, "kpx_icp_batch: %d registrations in one group of launches", x.count);
    const IcpSwitches &sw = icp_switches();
    ProgressWindow pw;
    int rc = pw.open(sw.stall_seconds);
    if (rc) return rc;
    const unsigned long long tag = pw.tag();
    // Launches kept queued ahead of the newest progress word the host has seen.  Every launch queued beyond the one that turns out to
    // be the last still runs (its blocks read "done" and return: ~4 us each) IN FRONT of whatever the caller queues next, and with
    // several frames in flight those empty launches take dispatch slots from the other frames' chains: 3 instead of round 2's 6,
    // same box, four frames in flight 2556-2600 vs 2441-2448 Mpoints/s, one frame at a time equal (a launch lasts >= 20 us, the
    // progress word reaches the host in a few; 2 starts to starve: profiles/r04/exp_icp_window.txt).  KPX_ICP_WINDOW: A/B switch.
    const int window = sw.window;
    // The update runs in the LAST block of every registration's sweep.  The other placements live in the per-registration drivers: the
    // next sweep's prologue in drive_windowed (icp_fused_launch), its own kernel in kpx_icp and under KPX_ICP_FUSE=0 (icp_iter_launch).
    const int light = icp_light_word(sw);
    const CertPolicy cert_policy = sw.cert_policy;
    // The one-launch chain (icp_chain_kernel) when the records hold the iterations and the
    // group's blocks fit the device beside the chains already in flight; KPX_ICP_CHAIN=0: always a launch per iteration.
    const bool chain_ok = chain_form_on() && x.max_iteration <= kChainRecords - 2 && chain_abort_word() != nullptr &&
                          (!sw.chain_alone || busy_threads() <= 1);
    // KPX_ICP_ROWS=0: the iterations through icp_iter_batch_kernel (a wave per 16-row tile, blocks of four) -- the A/B switch of
    // icp_rows_kernel (a wave per 64 rows)
    // (1, the default: per launch, by how much of the registrations the last reported iteration still searched -- the progress word's
    // bits 33..39: a wave per tile while most rows are searched, a wave per 64 rows once most are certified (KPX_ICP_ROWS_SHARE: the
    // largest searched share, in 1/127ths, at which the rows form is taken); 2: always the rows form.  The forms agree bit for bit,
    // so the choice -- which follows the host's timing -- never shows in a result.)
    const int rows_mode = sw.rows;
    const int rows_share = sw.rows_share;
    const NnBuffers &tb = x.bufs[0];                       // (the target's operands are shared)
    hipStream_t ls = x.st;
    IcpBatchArgs A;
    Mat16x8 T0;
    unsigned b0 = 0;
    for (int c = 0; c < kIcpBatchMax; ++c) {
        const int i = c < x.count ? c : x.count - 1;          // unused slots repeat the last problem (never addressed: count bounds the search)
        const NnBuffers &b = x.bufs[i];
        IcpProblem &P = A.p[c];
        P.src = x.h_src[i]; P.row_of = b.row_of; P.src_sorted = b.src_sorted; P.idx_sorted = b.idx_sorted;
        P.ptgt_sorted = b.ptgt_sorted; P.pair = b.state;
        P.idx_cur = nullptr; P.d2_cur = nullptr;              // a batch reports transforms, not correspondence lists
        P.ring = b.acc_fixed; P.result = x.d_results + 20 * i; P.progress = &pw.words[i]; P.n = x.h_n_src[i];
        P.light_key = b.light_key; P.sbbox = b.sort_s.bbox; P.cert = b.cert_sorted; P.thist = b.thist;
        P.chain_rec = chain_ok ? b.chain_rec : nullptr;
        P.block0 = b0; P.blocks = (unsigned)cdiv(x.h_n_src[i], kIRows);
        P.tgt = x.tgt; P.tn = x.tgt_normals; P.Bs = tb.Bs; P.orig = tb.orig_t; P.tile_box = tb.tile_box; P.group_box = tb.group_box;
        P.tbbox = tb.sort_t.bbox; P.n_groups = x.tplan->l_groups; P.k = 0; P.tag = tag;
        for (int e = 0; e < 16; ++e) T0.m[c][e] = x.h_init[16 * i + e];
        if (c < x.count) { b0 += P.blocks; pw.clear(i); }
    }
    A.count = x.count;
    hipLaunchKernelGGL(icp_batch_init_kernel, dim3(b0), dim3(256), 0, ls, A, T0);
    bool chained = false;
    if (chain_ok) {
        chained = chain_launch_if_fits(b0, ls, sw.chain_budget, sw.chain_no_lock, [&] {
            ProfScope prof(KPX_PROF_NN_LOCAL, 0.0, ls);
            hipLaunchKernelGGL(icp_chain_kernel, dim3(b0), dim3(kIThreads), 0, ls, A, x.tgt, x.tgt_normals, tb.Bs, tb.orig_t, tb.tile_box,
                               tb.group_box, x.tplan->l_groups, tb.sort_t.bbox, x.md2, x.mode, x.max_iteration, x.relative_fitness, x.relative_rmse, tag,
                               prof_armed() ? nn_visits_ptr() : (unsigned long long *)nullptr, light, cert_policy, sw.chain_wait_ticks, chain_abort_word());
        });
        if (chained && sw.chain_dump) chain_dump_records(A, ls);
    }
    int k = 0;                                                 // the next iteration to queue
    for (bool pending = !chained; pending && !rc;) {
        int seen = INT_MAX, share = 0;
        // the launches still to be queued carry only the registrations that have not converged yet (as far as the host
        // knows: the progress words lag by up to `window` launches); a converged problem's blocks in an already queued
        // launch read its state and return
        IcpBatchArgs act;
        act.count = 0;
        unsigned ab = 0;
        for (int c = 0; c < A.count; ++c) {
            const ProgressWindow::Word w = pw.read(c);
            if (w.converged) continue;
            seen = w.seen < seen ? w.seen : seen;
            share = w.share > share ? w.share : share;
            act.p[act.count] = A.p[c];
            act.p[act.count].block0 = ab;
            ab += A.p[c].blocks;
            ++act.count;
        }
        if (act.count == 0) break;                             // every registration has converged
        for (int c = act.count; c < kIcpBatchMax; ++c) act.p[c] = act.p[act.count - 1];
        bool advanced = false;
        for (; k <= x.max_iteration && k - seen < window; ++k) {
            advanced = true;
            ProfScope prof(KPX_PROF_NN_LOCAL, 0.0, ls);
            unsigned long long *visits = prof_armed() ? nn_visits_ptr() : (unsigned long long *)nullptr;
            for (int c = 0; c < kIcpBatchMax; ++c) act.p[c].k = k;
            if (!(rows_mode == 2 || (rows_mode == 1 && share <= rows_share)))
                hipLaunchKernelGGL(icp_iter_batch_kernel, dim3(ab), dim3(kIThreads), 0, ls, act, x.md2, x.mode, x.max_iteration, x.relative_fitness,
                                   x.relative_rmse, visits, light, cert_policy);
            else if (x.mode == 1)                              // one wave per 64 rows (kpx_icprows.h)
                hipLaunchKernelGGL(icp_rows_kernel<1>, dim3(ab), dim3(kRowsBlock), 0, ls, act, x.md2, x.max_iteration, x.relative_fitness, x.relative_rmse,
                                   visits, light, cert_policy);
            else
                hipLaunchKernelGGL(icp_rows_kernel<0>, dim3(ab), dim3(kRowsBlock), 0, ls, act, x.md2, x.max_iteration, x.relative_fitness, x.relative_rmse,
                                   visits, light, cert_policy);
        }
        pending = k <= x.max_iteration;                        // (else everything is queued)
        rc = pw.pass_done(advanced, pending);
    }
    if (hipGetLastError() != hipSuccess && !rc) rc = fail(KPX_ERR_HIP, "kpx_icp_batch: launch failed");
    return rc;
}

// Culled engine, one chain of launches per problem: every update step publishes "iterations finished | converged" in a pinned word
// of its problem.  The driver keeps a window of iterations queued per problem and tops it up as the words advance: no copies, no
// events, and at most `window` launches wasted after a problem converges (they return at once on its flag).
static int drive_windowed(const BatchCtx &x)
{
    ProgressWindow pw;
    int rc = pw.open(icp_switches().stall_seconds);
    if (rc) return rc;
    const unsigned long long tag = pw.tag();
    constexpr int window = 6;
    const bool fused = icp_switches().fuse;                  // A/B switch: 0 = update in its own kernel
    const int last_k = fused ? x.max_iteration + 1 : x.max_iteration;       // the fused chain ends with an update-only launch
    int next_k[64];
    bool fin[64];
    for (int i = 0; i < x.count && !rc; ++i) {
        hipStream_t ls = x.lane(i);
        pw.clear(i);
        hipLaunchKernelGGL(icp_init_kernel, dim3(1), dim3(1), 0, ls, x.bufs[i].state, mat16_from(x.h_init + 16 * i));
        rc = nn_prep_source(x.h_src[i], x.plans[i], x.bufs[i], ls, x.ordered);
        next_k[i] = 0;
        fin[i] = false;
    }
    for (bool pending = true; pending && !rc;) {
        pending = false;
        bool advanced = false;
        for (int i = 0; i < x.count; ++i) {
            if (fin[i]) continue;
            const ProgressWindow::Word w = pw.read(i);
            if (w.converged) { fin[i] = true; continue; }
            hipStream_t ls = x.lane(i);
            while (next_k[i] <= last_k && next_k[i] - w.seen < window) {
                advanced = true;
                if (fused)
                    icp_fused_launch(x.h_src[i], x.tgt, x.tgt_normals, x.plans[i], x.bufs[i], x.md2, x.mode, next_k[i], x.max_iteration, x.relative_fitness,
                                     x.relative_rmse, x.d_results + 20 * i, ls, &pw.words[i], tag);
                else
                    icp_iter_launch(x.h_src[i], x.tgt, x.tgt_normals, x.plans[i], x.bufs[i], x.md2, x.mode, next_k[i], x.max_iteration, x.relative_fitness,
                                    x.relative_rmse, x.d_results + 20 * i, ls, &pw.words[i], tag);
                ++next_k[i];
            }
            if (next_k[i] > last_k) { fin[i] = true; continue; }                        // everything is queued
            pending = true;
        }
        rc = pw.pass_done(advanced, pending);
    }
    if (hipGetLastError() != hipSuccess && !rc) rc = fail(KPX_ERR_HIP, "kpx_icp_batch: launch failed");
    return rc;
}

// All-pairs engine: one iteration (search + solve) of a problem at a time, followed by a copy of its state to a pinned slot and an
// event; the host waits for the event, reads (fitness, rmse) -- the sweep choice of the next iteration follows them (ScreenPolicy)
// -- and queues the next iteration.
static int drive_dense_polled(const BatchCtx &x)
{
    IcpState *h_states = static_cast<IcpState *>(thread_resources().pinned(kPinIcpStates, 64 * 2 * sizeof(IcpState)));   // two poll slots per problem
    if (!h_states) return KPX_ERR_HIP;
    hipEvent_t ev[64][2];
    int made = 0, rc = KPX_OK;
    for (; made < 2 * x.count && !rc; ++made)
        if (hipEventCreateWithFlags(&ev[made / 2][made % 2], hipEventDisableTiming) != hipSuccess) { rc = fail(KPX_ERR_HIP, "kpx_icp_batch: hipEventCreateWithFlags failed"); break; }
    ScreenPolicy policy[64];
    int next_k[64], enq[64], polled[64];
    auto enqueue = [&](int i) -> int {
        hipStream_t ls = x.lane(i);
        const NnBuffers &b = x.bufs[i];
        if (next_k[i] <= x.max_iteration) {
            const int k = next_k[i]++;
            int r = nn_search_launch(x.h_src[i], x.tgt, x.tgt_normals, x.plans[i], b, b.state->T, &b.state->done, k > 0, policy[i].allow(k), x.md2, x.mode, ls);
            if (r) return r;
            hipLaunchKernelGGL(icp_solve_kernel, dim3(1), dim3(kSolveThreads), 0, ls, b.part_acc, (int)cdiv(x.h_n_src[i], kMergeThreads),
                               x.h_n_src[i], x.mode, k, x.max_iteration, x.relative_fitness, x.relative_rmse, b.state, x.d_results + 20 * i);
        }
        const int slot = enq[i] & 1;
        KPX_HIP(hipMemcpyAsync(&h_states[2 * i + slot], b.state, sizeof(IcpState), hipMemcpyDeviceToHost, ls));
        KPX_HIP(hipEventRecord(ev[i][slot], ls));
        ++enq[i];
        return KPX_OK;
    };
    for (int i = 0; i < x.count && !rc; ++i) {
        hipStream_t ls = x.lane(i);
        hipLaunchKernelGGL(icp_init_kernel, dim3(1), dim3(1), 0, ls, x.bufs[i].state, mat16_from(x.h_init + 16 * i));
        rc = nn_prep_source(x.h_src[i], x.plans[i], x.bufs[i], ls);
        next_k[i] = 0; enq[i] = 0; polled[i] = 0;
        if (!rc && next_k[i] <= x.max_iteration) rc = enqueue(i);
    }
    for (bool busy = true; busy && !rc;) {
        busy = false;
        for (int i = 0; i < x.count && !rc; ++i) {
            if (polled[i] >= enq[i]) continue;
            busy = true;
            const int slot = polled[i] & 1;
            if (hipEventSynchronize(ev[i][slot]) != hipSuccess) { rc = fail(KPX_ERR_HIP, "convergence poll failed"); break; }
            const IcpState hs = h_states[2 * i + slot];
            ++polled[i];
            if (hs.done || next_k[i] > x.max_iteration) continue;
            policy[i].observe(hs.fitness, hs.rmse);
            rc = enqueue(i);
        }
    }
    for (int e = 0; e < made; ++e) (void)hipEventDestroy(ev[e / 2][e % 2]);
    return rc;
}
}  // namespace kpx

int kpx::icp_batch_ordered(int32_t count, const float *const *h_src, const int64_t *h_n_src, const float *tgt, const float *tgt_normals, int64_t n_tgt,
                           double max_dist, const double *h_init, int32_t mode, int32_t max_iteration, double relative_fitness, double relative_rmse,
                           double *d_results, void *ws, size_t ws_bytes, void *stream, bool presorted)
{
    KPX_REQUIRE(count >= 1 && count <= kBatchMax && h_src && h_n_src, "kpx_icp_batch: bad batch");
    KPX_REQUIRE(mode == KPX_ICP_POINT_TO_POINT || mode == KPX_ICP_POINT_TO_PLANE, "kpx_icp: unknown estimation mode");
    KPX_REQUIRE(mode != KPX_ICP_POINT_TO_PLANE || tgt_normals,
                "TransformationEstimationPointToPlane and TransformationEstimationColoredICP require pre-computed normal vectors for target PointCloud.");
    KPX_REQUIRE(max_dist > 0.0, "Invalid max_correspondence_distance.");
    KPX_REQUIRE(n_tgt >= 1 && n_tgt < ((int64_t)1 << 31) - 65536 && max_iteration >= 0, "kpx_icp_batch: bad target size");
    KPX_REQUIRE(tgt && h_init && d_results && ws, "kpx_icp_batch: null pointer");
    for (int i = 0; i < count; ++i)
        KPX_REQUIRE(h_src[i] && h_n_src[i] >= 1 && h_n_src[i] < ((int64_t)1 << 31), "kpx_icp_batch: bad source cloud %d", i);
    hipStream_t st = (hipStream_t)stream;
    BusyScope busy;
    // (a one-launch chain that gave up its residency wait poisons ITS OWN results with NaN -- icp_chain_kernel -- and the callers that read
    // results report it for that call; an abort left over from an earlier call is not this call's error)
    (void)icp_chain_abort_take();
    // the problems of a batch are independent chains of short, latency-bound kernels: they run side by side on the
    // library's internal lanes (kpx_internal.h), forked from / joined to the caller's stream by events
    Arena a(ws, ws_bytes);
    BatchLayout L;
    const bool can_batch_sort = batch_carve(a, count, h_n_src, n_tgt, &L);
    KPX_ARENA_CHECK(a);
    const NnPlan *plans = L.plans, &tplan = L.tplan;
    const NnBuffers *bufs = L.bufs;
    // the shared target and every source are ordered along their Morton curves by ONE sort (cloud number above the code)
    const bool ordered = can_batch_sort && local_engine();
    int rc = KPX_OK;
    if (ordered) {
        MortonBatch mb;
        mb.count = count + 1;
        mb.off[0] = 0;
        for (int c = 0; c < kMortonBatchMax; ++c) {
            const bool on = c < mb.count;
            mb.pts[c] = !on ? nullptr : (c == 0 ? tgt : h_src[c - 1]);
            mb.perm[c] = !on ? nullptr : (c == 0 ? bufs[0].orig_t : bufs[c - 1].row_of);
            mb.bbox[c] = !on ? nullptr : (c == 0 ? bufs[0].sort_t.bbox : bufs[c - 1].sort_s.bbox);
            mb.off[c + 1] = mb.off[c] + (!on ? 0 : (c == 0 ? n_tgt : h_n_src[c - 1]));
        }
        rc = morton_order_batch(mb, L.ms, st, presorted);
        if (rc) return rc;
    }
    rc = nn_prep(tgt, tplan, bufs[0], st, ordered);
    if (rc) return rc;
    // One chain of launches for the whole batch (drive_grouped) when the clouds were ordered by the batch sort: it runs on the caller's
    // stream itself (no fork / join events).  KPX_ICP_BATCH_LAUNCH=0 / KPX_ICP_FUSE=0, or a batch too large for one sort: one chain per
    // problem, on the lanes.
    const bool grouped = local_engine() && ordered && icp_switches().batch_launch && icp_switches().fuse;
    const int used_lanes = grouped ? 0 : (count < kLaneCount ? count : kLaneCount);
    LaneSet *ln = nullptr;                          // (the thread's lanes exist only once one of its calls has forked)
    if (used_lanes && (rc = lanes_get(&ln))) return rc;
    const BatchCtx ctx{ count, h_src, h_n_src, tgt, tgt_normals, h_init, max_dist * max_dist, mode, max_iteration, relative_fitness, relative_rmse, d_results,
                        plans, &tplan, bufs, ordered, st, ln ? ln->s : nullptr };
    if (used_lanes) rc = lanes_fork(ln, st, used_lanes);
    if (!rc) rc = grouped ? drive_grouped(ctx) : local_engine() ? drive_windowed(ctx) : drive_dense_polled(ctx);
    if (used_lanes) {
        const int jrc = lanes_join(ln, st, used_lanes);
        rc = rc ? rc : jrc;
    }
    if (rc) for (int l = 0; l < used_lanes; ++l) (void)hipStreamSynchronize(ln->s[l]);     // leave nothing in flight on an error
    if (rc) return rc;
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}
