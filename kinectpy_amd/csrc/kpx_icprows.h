// kpx_icprows.h -- one ICP iteration of SEVERAL registrations, one wave per 64 sorted rows (included by kpx_icp.hip only; round 5).
//
// icp_iter_body gives every 16-row tile a wave and every 64 rows a block of four: right for the first iterations, where every tile
// is searched, and wasteful afterwards -- from iteration ~10 on 95-99.9 % of the rows carry a certificate ("Certificates", kpx_icpiter.h),
// a block then lives ~8.6 us of which the search is 0.3, and only 16 of a wave's 64 lanes do the per-row work (transform, bound,
// certificate test, the 17 / 29 terms of the update sums).  With four frames in flight the chip's wave slots x a block's life time IS the
// frame rate, so here
//   * a block is ONE wave and owns 64 consecutive sorted rows, one row per lane in the prologue (rows, previous partners and their
//     coordinates / normals, certificates: coalesced loads; AC1, the partner's AC2 value, the certificate test) and in the pair epilogue
//     (AC3, the 17 / 29 contributions: the slots that are live in the mode, acc_live in kpx_icpdefs.h);
//   * the wave sweeps only those of its four 16-row tiles that hold an uncertified row, one after the other, through the same
//     sweep_wave (kpx_nnlocal.h) on the tile's row records in LDS -- partners are those of icp_iter_body bit for bit;
//   * the sums follow the contract stated in icp_iter_body: per tile the balanced tree of four DPP butterfly steps
//     (row16_tree_sum == tile_tree16), the four tile partials added exactly in fixed point, one pair of returning atomics per live sum;
//   * the block that draws the registration's last ticket performs the update (icp_finish_wave), as in icp_iter_body's ticket mode;
//   * the launch takes the argument block of icp_iter_batch_kernel (IcpBatchArgs: one frame's registrations onto their shared target,
//     all at iteration p[..].k), and the row prologue, the pair terms and the winner's step are the functions icp_iter_body calls.
#pragma once
#include "kpx_icpiter.h"

namespace kpx {

constexpr int kRowsBlock = 64;
static_assert(kRowsBlock == kIRows, "IcpProblem::block0 / blocks count 64-row blocks for icp_iter_batch_kernel and icp_rows_kernel alike");

constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppHalfMirror = 0x141, kDppMirror = 0x140;
// sum over the 16 lanes of a DPP row, the same value (bit for bit: addition commutes) in all of them: tile_tree16's order
__device__ __forceinline__ double row16_tree_sum(double v)
{
    v += dpp_f64<kDppXor1>(v);
    v += dpp_f64<kDppXor2>(v);
    v += dpp_f64<kDppHalfMirror>(v);
    v += dpp_f64<kDppMirror>(v);
    return v;
}

template <int MODE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(KPX_ICP_WPE, KPX_ICP_WPE))) void icp_rows_kernel(IcpBatchArgs args, double max_d2, int max_iter, double rel_fit,
                                                                                                                     double rel_rmse, unsigned long long *__restrict__ tile_visits,
                                                                                                                     int light, CertPolicy pol)
{
    constexpr int NACC = MODE == 1 ? kAcc : 17;
    // (the descriptor by VALUE: read through a reference into the argument block, field by field where it is used, the kernel came out
    // with 22 / 4 spilled vector registers (MODE 1 / 0) instead of 18 / 2 -- one more double carried through the sweep in scratch memory;
    // measured while MODE 1 still carried the 15 sums point-to-plane does not read: without them it spills 2, like MODE 0)
    const IcpProblem P = args.p[batch_problem(args)];
    const unsigned bid = blockIdx.x - P.block0;
    const int k = P.k;
    IcpState *const st = P.pair;
    if (st->done) return;

    // LDS: 10.3 KB per wave (12 waves per CU).  The sweep's records are COMPACT: slot = the row's rank among the block's rows that are
    // searched; what the pair epilogue needs of every row is parked by lane.
    __shared__ IcpState s_state;
    __shared__ double s_sums[kAcc];
    __shared__ FinishScratch s_tail;
    __shared__ double rowd[kRowsBlock][kRowStride];     // by slot: x, y, z under this iteration's transform, (the sweep's bound), K, bound / result value
    __shared__ float rowf[kLRows][kRowFStride];         // float32 mirror of the 16 rows being swept (written by the sweep)
    __shared__ float rowk[kRowsBlock][11];              // by lane: previous partner's coordinates, normal, index; the row's own coordinates
    __shared__ int32_t rowi[kRowsBlock];                // by slot: partner (bound going in, result coming out)
    __shared__ uint32_t rowc[kRowsBlock];               // by slot: certificate word (the sweep writes the new one)
    __shared__ int32_t rowm[kRowsBlock];                // by slot: 1 = the row is certified (searched only by the self-check)
    __shared__ int32_t lists[kLScratch];                // the sweep's scratch; afterwards the four tile partials of the sums
    static_assert(kLScratch * sizeof(int32_t) >= 4 * kAcc * sizeof(double), "the tile partials reuse the sweep's scratch");
    double (*s_part)[kAcc] = reinterpret_cast<double (*)[kAcc]>(lists);

    const int lane = threadIdx.x;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const int64_t last = P.n - 1;
    const int64_t row = (int64_t)bid * kRowsBlock + lane;
    const bool valid = lane < kRowsBlock && row <= last;    // (the lane test is always true; without it the compiler allocates the kernel's registers differently)
    const int64_t r = valid ? row : last;
    const bool certs = (light & 2) != 0, use_light = (light & 1) != 0, cert_check = (light & 4) != 0;
    const double t2max = target_t2max(P.tbbox);

    // everything that does not depend on this iteration's transform is requested first
    float my_src[3], my_pt[3] = { 0.0f, 0.0f, 0.0f }, my_nrm[3] = { 0.0f, 0.0f, 0.0f };
    int32_t my_prev = -1;
    uint32_t my_cert = 0u;
#pragma unroll
    for (int a = 0; a < 3; ++a) my_src[a] = P.src_sorted[3 * r + a];
    if (k > 0) {
        my_prev = P.idx_sorted[r];
#pragma unroll
        for (int a = 0; a < 3; ++a) my_pt[a] = P.ptgt_sorted[3 * r + a];
        if (certs) my_cert = P.cert[r];
    }
    const double key_in = use_light ? P.light_key[bid] : 0.0;
    if (lane < (int)(sizeof(IcpState) / sizeof(double))) reinterpret_cast<double *>(&s_state)[lane] = reinterpret_cast<const double *>(st)[lane];
    GroupPre gpre;
    group_pre_load(gpre, P.group_box, P.n_groups, lane);
    if (MODE == 1 && k > 0) {
        const float *np_ = P.tn + 3 * (int64_t)(my_prev > 0 ? my_prev : 0);
#pragma unroll
        for (int a = 0; a < 3; ++a) my_nrm[a] = np_[a];
    }
    // (certificates) the transform of the iteration the row was last searched in: its position then is recomputed from it, exactly
    double Th[12];
    const int kc = (int)(my_cert & 63u);
    const float Lc = __uint_as_float(my_cert & ~63u);
    if (certs && k > 0 && Lc > 0.0f) {
#pragma unroll
        for (int e = 0; e < 12; ++e) Th[e] = P.thist[12 * kc + e];
    } else {
#pragma unroll
        for (int e = 0; e < 12; ++e) Th[e] = 0.0;
    }
    const double *Tk = st->T;
    unsigned long long *const ticket = P.ring + kAccSet;

    // LightSkip: nothing of this block can have come within reach since it was last swept -> straight to the ticket
    const bool skip = use_light && key_in > 0.0 && (st->motion + st->reach) * (1.0 + 1e-6) + 1e-6 < key_in;
    unsigned visited_total = 0u;
    if (!skip) {
        const double c_reach = certs ? st->reach : 0.0;
        const double c_skin = cert_skin(certs, k, st, max_d2, pol);
        bool my_active = valid, my_certd = false;
        unsigned long long act64, certd64;
        int n_act;
        {
            double s[3];
            xform_row(Tk, my_src, s);
            const double seed = row_seed(s);
            double bv = INFINITY;
            int32_t bj = INT_MAX;
            if (k > 0 && my_prev >= 0) { bv = partner_bound(s, seed, my_pt); bj = my_prev; }
            bound_clamp(seed, max_d2, t2max, bv, bj);
            double rb0 = bv - 1.0;
            if (certs) {
                const bool certd = cert_test(s, my_src, my_prev, my_pt, bj, my_cert, Th, c_reach, c_skin, cert_check ? 1 : 0, rb0);
                my_active = (!certd || cert_check) && valid;
                my_certd = certd && valid;
            }
            act64 = __builtin_amdgcn_ballot_w64(my_active);
            certd64 = __builtin_amdgcn_ballot_w64(my_certd);
            n_act = __builtin_popcountll(act64);
            if (my_active) {
                const int slot = __builtin_popcountll(act64 & lt);
                rowd[slot][0] = s[0]; rowd[slot][1] = s[1]; rowd[slot][2] = s[2];
                rowd[slot][3] = rb0;
                rowd[slot][4] = seed; rowd[slot][5] = bv;
                rowi[slot] = bj;
                rowc[slot] = my_cert;
                rowm[slot] = my_certd ? 1 : 0;
            }
            if (lane >= n_act) {                               // padding of the last 16-row tile (and beyond): rows that take no part
                rowd[lane][0] = 0.0; rowd[lane][1] = 0.0; rowd[lane][2] = 0.0;
                rowd[lane][3] = -1.0;
                rowd[lane][4] = 1.0; rowd[lane][5] = 2.0;
                rowi[lane] = INT_MAX;
                rowc[lane] = 0u;
                rowm[lane] = 1;
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) { rowk[lane][a] = my_pt[a]; rowk[lane][3 + a] = my_nrm[a]; rowk[lane][7 + a] = my_src[a]; }
            rowk[lane][6] = __int_as_float(my_prev);
        }
        wave_lds_fence();

        // the rows to be searched, 16 at a time (a block whose 64 rows all are: its four tiles as they stand)
        bool light_blk = n_act == kRowsBlock;                 // (LightSkip speaks for ALL rows of the block)
        double gap2_blk = INFINITY;
#pragma unroll 1
        for (int v0 = 0; v0 < n_act; v0 += kLRows) {
            const int left = n_act - v0;
            const unsigned act_mask = left >= kLRows ? 0xFFFFu : ((1u << left) - 1u);
            const int lane_s = opaque_i((int)threadIdx.x), q_s = lane_s >> 4, j_s = lane_s & 15;
            WaveRows w;
            w.rows = &rowd[v0][0];
            w.rowsf = &rowf[0][0];
            w.a = q_s < 3 ? rowd[v0 + j_s][q_s] : 1.0;
#pragma unroll
            for (int rr4 = 0; rr4 < 4; ++rr4) {
                const int rr = v0 + q_s + 4 * rr4;
                w.seed[rr4] = rowd[rr][4];
                w.best[rr4] = rowd[rr][5];
                w.bcol[rr4] = rowi[rr];
                w.rb0[rr4] = rowd[rr][3];
            }
            w.skin = c_skin;
            w.act_mask = act_mask;
            w.light_gap2 = -1.0;
            w.dbg = nullptr;
            wave_lds_fence();                                 // rowd[..][3] is the sweep's own slot from here on
            const unsigned long long swept = sweep_wave<true, true, true>(w, P.Bs, P.orig, P.tile_box, P.group_box, P.n_groups, t2max, lists, &gpre);
            visited_total += (unsigned)(swept & 0xFFFFu);
            const int lane_p = opaque_i((int)threadIdx.x), q_p = lane_p >> 4, j_p = lane_p & 15;
            if (certs && cert_check && j_p == 0) {
#pragma unroll
                for (int rr4 = 0; rr4 < 4; ++rr4) {
                    const int rr = q_p + 4 * rr4;
                    if (((act_mask >> rr) & 1u) != 0u && rowm[v0 + rr] != 0 && w.bcol[rr4] != rowi[v0 + rr])
                        cert_check_disagreement(k, (int64_t)bid * kRowsBlock + v0 + rr, rowi[v0 + rr], w.bcol[rr4], rowc[v0 + rr]);
                }
            }
            wave_lds_fence();
            if (j_p == 0) {
#pragma unroll
                for (int rr4 = 0; rr4 < 4; ++rr4) {
                    const int rr = q_p + 4 * rr4;
                    rowi[v0 + rr] = w.bcol[rr4];
                    // new keys for the rows that were searched
                    if (certs && ((act_mask >> rr) & 1u) != 0u && rowm[v0 + rr] == 0) rowc[v0 + rr] = cert_word(w.sec[rr4], w.eps_out, w.rb_out[rr4], k);
                }
            }
            if (w.light_gap2 >= 0.0) gap2_blk = fmin(gap2_blk, w.light_gap2);
            else light_blk = false;
            wave_lds_fence();
        }
        const int lane_e = opaque_i((int)threadIdx.x);
        const unsigned long long lt_e = (1ull << lane_e) - 1ull;
        if (certs && cert_check && lane_e == 0) cert_check_count(bid == 0, k, st, c_skin, __builtin_popcountll(certd64), __builtin_popcountll(act64 & ~certd64));
        if (tile_visits && lane_e == 0 && visited_total) atomicAdd(tile_visits + (blockIdx.x & (kVisitSlots - 1)), (unsigned long long)visited_total);

        // the chosen pairs: direct distance (AC3), contribution to the sums -- one row per lane.  Only the slots that are live in the mode
        // (acc_live, kpx_icpdefs.h) exist from here on: the others are never formed, summed, parked in s_part or added
        constexpr bool PLANE = MODE == 1;
        double c[NACC];
#pragma unroll
        for (int a = 0; a < NACC; ++a) c[a] = 0.0;
        const int64_t row_e = (int64_t)bid * kRowsBlock + lane_e;
        if (lane_e < kRowsBlock && row_e <= last) {
            const bool was_act = ((act64 >> lane_e) & 1ull) != 0ull;
            const int slot_e = __builtin_popcountll(act64 & lt_e);
            const int32_t prev_j = __float_as_int(rowk[lane_e][6]);
            // a row that was not searched keeps what it came with (certified: its partner, or none)
            const int32_t bj = was_act ? rowi[slot_e] : (prev_j >= 0 ? prev_j : INT_MAX);
            const bool none = bj < 0 || bj == INT_MAX;
            const int32_t out_j = none ? -1 : bj;
            const bool changed = k == 0 || out_j != prev_j;
            if (changed) P.idx_sorted[row_e] = out_j;
            const bool searched = was_act && ((certd64 >> lane_e) & 1ull) == 0ull;
            if (certs && searched) P.cert[row_e] = rowc[slot_e];
            if (!none) {
                const float sf[3] = { rowk[lane_e][7], rowk[lane_e][8], rowk[lane_e][9] };
                double s[3];
                xform_row(Tk, sf, s);
                float tf[3] = { rowk[lane_e][0], rowk[lane_e][1], rowk[lane_e][2] }, nf[3] = { rowk[lane_e][3], rowk[lane_e][4], rowk[lane_e][5] };
                if (changed) {
                    const float *tp = P.tgt + 3 * (int64_t)bj;
#pragma unroll
                    for (int e = 0; e < 3; ++e) tf[e] = tp[e];
                    if (MODE == 1) {
                        const float *np_ = P.tn + 3 * (int64_t)bj;
#pragma unroll
                        for (int e = 0; e < 3; ++e) nf[e] = np_[e];
                    }
#pragma unroll
                    for (int e = 0; e < 3; ++e) P.ptgt_sorted[3 * row_e + e] = tf[e];
                }
                const double t[3] = { (double)tf[0], (double)tf[1], (double)tf[2] };
                const double d2 = pair_d2(s, t);
                if (d2 < max_d2) pair_terms(s, t, d2, !PLANE, PLANE, nf, [&](int slot, double v) { c[slot] = v; });
            }
        }
        // per tile the balanced tree (every lane of the tile's DPP row ends with the tile's partial), then the four partials exactly
#pragma unroll
        for (int a = 0; a < NACC; ++a)
            if (acc_live(PLANE, a)) c[a] = row16_tree_sum(c[a]);
        wave_lds_fence();                                     // (the partials take the place of the sweep's scratch)
        if ((lane_e & 15) == 0) {
#pragma unroll
            for (int a = 0; a < NACC; ++a)
                if (acc_live(PLANE, a)) s_part[lane_e >> 4][a] = c[a];
        }
        wave_lds_fence();
        if (lane_e < NACC && acc_live(PLANE, lane_e)) {
            unsigned long long lo = 0ull, hi = 0ull;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                unsigned long long l, h;
                fixed_split(s_part[t][lane_e], l, h);
                fixed_accumulate(lo, hi, l, h);
            }
            fixed_add_words_performed(P.ring + (((int64_t)(bid & (kAccCopies - 1)) * kAcc + lane_e) * kFixedWords), lo, hi);
        } else if (lane_e == NACC && (act64 & ~certd64) != 0ull) {
            // how much of the registration is still searched (see icp_iter_body): one returning add per block, eight words per registration
            const unsigned long long back = __hip_atomic_fetch_add(ticket + kSearchedWord + (bid & 7u), (unsigned long long)__builtin_popcountll(act64 & ~certd64), __ATOMIC_RELAXED,
                                                                   __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("" ::"v"(back));
        }
        if (use_light && lane_e == 0) P.light_key[bid] = light_blk ? st->motion + sqrt(gap2_blk) * (1.0 - 1e-9) : 0.0;
    }

    // "The last block finishes the job" (icp_iter_body, ticket mode): every add above has RETURNED, the wave waits for all of them, then
    // draws its ticket; the block that draws the registration's last one reads the totals with device-coherent loads, clears them and
    // performs the update.  The state is written with plain stores: its readers are the blocks of the NEXT launch.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned tk = 0u;
    if (threadIdx.x == 0) tk = (unsigned)__hip_atomic_fetch_add(ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tk = (unsigned)__builtin_amdgcn_readfirstlane((int)tk);
    if (tk != P.blocks - 1u) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const int lane_w = opaque_i((int)threadIdx.x);
    const unsigned long long n_searched = winner_take<kRowsBlock, true>(P.ring, ticket, MODE == 1, s_sums, lane_w);
    const double *tbbox_w = P.tbbox;
    asm volatile("" : "+s"(tbbox_w));
    const double t2max_w = target_t2max(tbbox_w);
    icp_finish_wave(s_sums, P.n, MODE, k, max_iter, rel_fit, rel_rmse, &s_state, P.result, s_tail, lane_w,
                    LightSkip{ use_light ? P.sbbox : (const double *)nullptr, max_d2, t2max_w });
    wave_lds_fence();
    winner_publish(st, &s_state, certs ? P.thist : (double *)nullptr, k, P.progress, P.tag, n_searched, P.n, lane_w);
}

}  // namespace kpx
