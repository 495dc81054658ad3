// kpx_nndense.h -- the all-pairs correspondence search (KPX_NN_ENGINE=dense) and the merge step every engine shares.
//
// Correspondence search = all-pairs nearest neighbour as an fp64 MFMA distance GEMM in the K=4 augmented
// form (contract AC2):
//     A[i] = (s_x, s_y, s_z, 1)            s = T . src_i       (fp64 fma chain, contract AC1)
//     B[j] = (-2t_x, -2t_y, -2t_z, |t|^2)  |t|^2 = fma(tx,tx, fma(ty,ty, tz*tz))
//     C[i] = K_i = fma(sx,sx, fma(sy,sy, sz*sz)) + 1
//     D_ij = fma(1,|t|^2, fma(s_z,-2t_z, fma(s_y,-2t_y, fma(s_x,-2t_x, K_i))))  = d_ij^2 + 1 > 0
//            -> argmin_j, ties to the lowest j.
// v_mfma_f64_16x16x4_f64 produces a 16x16 tile of D per instruction (bit-for-bit the k-ordered fma chain
// above, seeded with C).  D > 0, so the IEEE bit pattern orders like an unsigned integer: the running
// argmin behind each MFMA is a 32-bit compare of the HIGH words (hi(D) <= hi(best): a necessary condition
// for an update) and a wave-uniform branch; the exact fp64 (value, column) update runs only in the rare
// wave-iterations where some lane passes.  To make updates rare the sweep starts from a valid upper bound:
// the previous iteration's partner (ICP iterations >= 1) or the winner of a seed sweep over every 64th
// target tile.  fp64 VALU compares contend with the fp64 MFMA pipe on MI355X (measured: 4 v_cmp_f64 per
// MFMA cost 30 % of the MFMA rate), the 32-bit prefilter does not.
// Block = 4 waves x 32 source rows; the B stream is staged through LDS by LDS-DMA (16 KiB stages, double
// buffered) and shared by the waves; the column range is split over gridDim.y, a second kernel merges the
// splits (lexicographic (value, column)), computes the direct squared distance (AC3) of the chosen pair
// and accumulates the sums the update needs.  The ICP loop runs on the device; a small kernel solves the
// 3x3 (Kabsch) or 6x6 (point-to-plane) system, updates T and raises `done`.
#pragma once
#include "kpx_icpdefs.h"
#include "kpx_linalg.h"

namespace kpx {

// ---- target preparation: B tiles, element (k, j) of tile t at B[t*64 + k*16 + j]; Bseed = every 64th tile --
__global__ __launch_bounds__(256) void nn_prep_kernel(const float *__restrict__ tgt, int64_t m, int64_t tiles_pad, double *__restrict__ B,
                                                      int64_t seed_tiles_pad, double *__restrict__ Bseed, const int32_t *__restrict__ perm,
                                                      int32_t *__restrict__ colB, int32_t *__restrict__ colSeed)
{
    // perm (round 4): the columns stand in the target's CURVE order (perm[slot] = the caller's index of the point in column `slot`), so
    // that the 32 columns of a trip are neighbours in space and a row's bound -- however loose -- reaches few trips; colB / colSeed carry
    // every column's ORIGINAL index (INT_MAX in the padding): the sweep reports, and breaks ties by, those.
    const int64_t total = (tiles_pad + seed_tiles_pad) * 16;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
        const bool seed = q >= tiles_pad * 16;
        const int64_t jj = seed ? q - tiles_pad * 16 : q;                 // column slot inside its operand array
        const int64_t j = seed ? jj * kSeedStride : jj;                    // (curve-ordered) target slot it stands for: the seed operand is every
                                                                            // kSeedStride-th POINT of the curve, a spatially uniform sample
        double b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = kSentinel;
        int32_t oj = INT_MAX;
        if (j < m) {
            oj = perm[j];
            double tx = tgt[3 * (int64_t)oj], ty = tgt[3 * (int64_t)oj + 1], tz = tgt[3 * (int64_t)oj + 2];
            b0 = -2.0 * tx; b1 = -2.0 * ty; b2 = -2.0 * tz;
            b3 = fma(tx, tx, fma(ty, ty, tz * tz));
        }
        double *o = (seed ? Bseed : B) + (jj >> 4) * 64 + (jj & 15);
        o[0] = b0; o[16] = b1; o[32] = b2; o[48] = b3;
        (seed ? colSeed : colB)[jj] = oj;
    }
}

// ---- per-row operands of one search: transformed source, row seed, bound from a known partner, f32 screening row --
// One thread per source row, once per search (the sweeps are split over the columns: computing these in their
// prologues would repeat the fp64 work in every split).
//   A64[row] = (s_x, s_y, s_z, 1)   K64[row] = K_i            -> fp64 sweep operands
//   prev != NULL: init_val/init_idx = exact D(i, prev[i]) by the MFMA's fma chain, and its partner
//   aux  != NULL (needs prev): A32[row] = fl32(s - c, 1), thr32[row] = (C_i, round_up((U_i - 1 - |s-c|^2) + C_i + E_i)),
//                              C_i = |s-c|^2 + E_i + 1 makes the f32 metric positive (integer compares)
__global__ __launch_bounds__(256) void nn_rowprep_kernel(const float *__restrict__ src, int64_t n, const float *__restrict__ tgt,
                                                         const double *__restrict__ T, const int32_t *__restrict__ done,
                                                         const int32_t *__restrict__ prev, const NnAux *__restrict__ aux,
                                                         double *__restrict__ init_val, int32_t *__restrict__ init_idx,
                                                         double *__restrict__ A64, double *__restrict__ K64,
                                                         float *__restrict__ A32, float *__restrict__ thr32,
                                                         int32_t *__restrict__ cand_cnt)
{
    if (done && *done) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) cand_cnt[n] = 0;          // number of rows whose candidate list overflowed
    if (i >= n) return;
    cand_cnt[i] = 0;
    double s[3];
    xform_row(T, src + 3 * i, s);
    const double seed = row_seed(s);
    reinterpret_cast<double2 *>(A64)[2 * i] = make_double2(s[0], s[1]);
    reinterpret_cast<double2 *>(A64)[2 * i + 1] = make_double2(s[2], 1.0);
    K64[i] = seed;
    if (!prev) return;
    const int32_t j = prev[i];
    const float *tp = tgt + 3 * (int64_t)j;
    const double tx = tp[0], ty = tp[1], tz = tp[2];
    const double t2 = fma(tx, tx, fma(ty, ty, tz * tz));
    double d = fma(s[0], -2.0 * tx, seed);
    d = fma(s[1], -2.0 * ty, d);
    d = fma(s[2], -2.0 * tz, d);
    d = fma(1.0, t2, d);
    init_val[i] = d;
    init_idx[i] = j;
    if (!aux) return;
    const double ux = s[0] - aux->c[0], uy = s[1] - aux->c[1], uz = s[2] - aux->c[2];
    const double q = fma(ux, ux, fma(uy, uy, uz * uz));
    // E_i bounds |D32 - exact|: operand roundings 2^-24 (6X + Y) + four chain roundings of partial sums <= C + X + Y,
    // X = 2|s-c||t-c| <= 2 sqrt(q rt2), Y = |t-c|^2 <= rt2, C ~ q + E + 1  (10 % and 1e-6 slack for second-order terms)
    const double x = 2.0 * sqrt(q * aux->rt2), y = aux->rt2;
    const double e = 1.1 * 5.9604644775390625e-08 * (10.0 * x + 9.0 * y + 4.0 * (q + 2.0)) * (1.0 + 1e-6) + 1e-6;
    const float cq = __double2float_ru(q + e + 1.0);                 // row constant: D32 = cq + approx >= 1 > 0
    reinterpret_cast<float4 *>(A32)[i] = make_float4((float)ux, (float)uy, (float)uz, 1.0f);
    thr32[2 * i] = cq;
    thr32[2 * i + 1] = __double2float_ru(((d - 1.0 - q) + (double)cq) + e);
}

// ---- float32 screening sweep (ICP iterations >= 1) ------------------------------------------------------------
// With a valid upper bound U_i (the exact D of last iteration's partner under the new transform) the exact
// argmin only needs the columns whose D can be <= U_i.  Those are found by ONE sweep of the f32 MFMA
// (v_mfma_f32_16x16x4_f32, ~3x the fp64 MFMA rate) on centred coordinates:
//     approx_ij = fl32 chain of (s-c) . (-2(t-c)) + |t-c|^2  ~  d_ij^2 - |s_i-c|^2
// with the rigorous error bound  |approx - exact| <= E_i = 2^-24 (12 |s_i-c| R_t + 5 R_t^2)  (two roundings of
// every operand, four chain roundings; R_t >= max |t-c|).  Every column with approx_ij <= (U_i - 1 - |s_i-c|^2) + E_i
// (+10 % and 1e-6 slack) is appended to row i's candidate list; nn_merge_kernel then evaluates the exact fp64
// metric (the same fma chain as the MFMA path / the oracle) for the candidates and the bound's partner and takes
// the lexicographic (value, column) minimum -- the result is bit-identical to the fp64 sweep.  Rows whose list
// overflows are resolved by an exact brute-force scan (nn_overflow_kernel).
typedef float f4 __attribute__((ext_vector_type(4)));

__global__ void nn_aux_kernel(const double *__restrict__ bbox, NnAux *aux)
{
    if (threadIdx.x || blockIdx.x) return;
    double r2 = 0.0;
    for (int a = 0; a < 3; ++a) {
        double c = rint(0.5 * (bbox[a] + bbox[3 + a]));
        aux->c[a] = c;
        double e = fmax(fabs(bbox[a] - c), fabs(bbox[3 + a] - c));
        r2 += e * e;
    }
    aux->rt2 = r2 * (1.0 + 1e-12);
}

// Bf tiles: element (k, j) of tile t at Bf[t*64 + k*16 + j] (float)
__global__ __launch_bounds__(256) void nn_prep_f32_kernel(const float *__restrict__ tgt, int64_t m, int64_t tiles_pad,
                                                          const NnAux *__restrict__ aux, float *__restrict__ Bf)
{
    const double cx = aux->c[0], cy = aux->c[1], cz = aux->c[2];
    const int64_t total = tiles_pad * 16;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (int64_t)gridDim.x * blockDim.x) {
        float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 3.0e38f;
        if (j < m) {
            double ux = (double)tgt[3 * j] - cx, uy = (double)tgt[3 * j + 1] - cy, uz = (double)tgt[3 * j + 2] - cz;
            b0 = (float)(-2.0 * ux); b1 = (float)(-2.0 * uy); b2 = (float)(-2.0 * uz);
            b3 = (float)fma(ux, ux, fma(uy, uy, uz * uz));
        }
        float *o = Bf + (j >> 4) * 64 + (j & 15);
        o[0] = b0; o[16] = b1; o[32] = b2; o[48] = b3;
    }
}

template <int TRIP, int MINW>
__global__ __launch_bounds__(256, MINW) void nn_screen_kernel(int64_t n, const float *__restrict__ Bf, int32_t tiles_per_split,
                                                           const int32_t *__restrict__ done, const float *__restrict__ A32,
                                                           const float *__restrict__ thr32, const int32_t *__restrict__ partner,
                                                           int32_t *__restrict__ cand_cnt, int32_t *__restrict__ cand,
                                                           int32_t *__restrict__ over_rows)
{
    if (done && *done) return;
    __shared__ __align__(16) float lds[2][kFStageFloats];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row_base = (int64_t)blockIdx.x * kFRowsPerBlock + (int64_t)wave * (kFRT * 16);
    const int64_t t0 = (int64_t)blockIdx.y * tiles_per_split;
    const int nstages = tiles_per_split / kFCT;

    // A operands: component k = lane>>4 of centred row (lane&15); thresholds of the rows this lane sees in D
    // (f32 layout: row = 4*(lane>>4) + reg)
    // the bound's own partner always passes the test and is always evaluated by nn_merge_kernel: it is not
    // appended (in steady state it is ~99 % of the hits, and an append costs a returning global atomic)
    float a[kFRT];
    f4 cq[kFRT];
    unsigned thr[kFRT][4];
#pragma unroll
    for (int rt = 0; rt < kFRT; ++rt) {
        const int64_t row = row_base + rt * 16 + (lane & 15);
        a[rt] = row < n ? A32[row * 4 + (lane >> 4)] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t drow = row_base + rt * 16 + 4 * (lane >> 4) + r;
            const float2 ct = drow < n ? reinterpret_cast<const float2 *>(thr32)[drow] : make_float2(1.0f, 0.0f);
            cq[rt][r] = ct.x;
            thr[rt][r] = __float_as_uint(ct.y);          // D32 > 0 and thr >= 0: unsigned order of the patterns
        }
    }

    const float *gB = Bf + t0 * 64;
    auto stage_load = [&](int stage, int buf) {
        const float *g = gB + (int64_t)stage * kFStageFloats;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int piece = wave * 4 + q;      // 16 pieces of 1 KiB (= 4 tiles) per 16 KiB stage
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(g + piece * 256 + lane * 4),
                                             (__attribute__((address_space(3))) void *)(&lds[buf][piece * 256]), 16, 0, 0);
        }
    };
    stage_load(0, 0);
    __syncthreads();

    for (int st = 0; st < nstages; ++st) {
        const int buf = st & 1;
        if (st + 1 < nstages) stage_load(st + 1, buf ^ 1);
        const float *lb = lds[buf] + lane;
        const int32_t tile0 = (int32_t)t0 + st * kFCT;
#pragma unroll 1
        for (int ct = 0; ct < kFCT; ct += TRIP) {
            // TRIP column tiles (TRIP x 4 MFMAs) per trip; per D row the minimum of the TRIP bit patterns
            // (v_min3_u32 / v_min_u32) and one unsigned compare against the row's threshold
            float bq[TRIP];
#pragma unroll
            for (int h = 0; h < TRIP; ++h) bq[h] = lb[(ct + h) * 64];
            f4 c[TRIP][kFRT];
#pragma unroll
            for (int rt = 0; rt < kFRT; ++rt)
#pragma unroll
                for (int h = 0; h < TRIP; ++h) c[h][rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rt], bq[h], cq[rt], 0, 0, 0);
            bool hit = false;
#pragma unroll
            for (int rt = 0; rt < kFRT; ++rt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    unsigned m = __float_as_uint(c[0][rt][r]);
#pragma unroll
                    for (int h = 1; h < TRIP; ++h) m = min(m, __float_as_uint(c[h][rt][r]));
                    hit |= m <= thr[rt][r];
                }
            if (__builtin_amdgcn_ballot_w64(hit) != 0) {          // wave-uniform; a few columns per row per sweep
                const int32_t col0 = (tile0 + ct) * 16 + (lane & 15);
#pragma unroll
                for (int rt = 0; rt < kFRT; ++rt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int64_t row = row_base + rt * 16 + 4 * (lane >> 4) + r;
#pragma unroll
                        for (int h = 0; h < TRIP; ++h)
                            if (__float_as_uint(c[h][rt][r]) <= thr[rt][r] && col0 + h * 16 != partner[row]) {
                                const int slot = atomicAdd(&cand_cnt[row], 1);
                                if (slot < kCand) cand[row * kCand + slot] = col0 + h * 16;
                                else if (slot == kCand) over_rows[atomicAdd(&cand_cnt[n], 1)] = (int32_t)row;   // first overflow of this row
                            }
                    }
            }
        }
        __syncthreads();
    }
}

// rows whose candidate list overflowed (listed by the screening sweep): exact brute-force scan (fp64 fma chain),
// one block per row at a time.  With nothing listed the kernel returns at once.
__global__ __launch_bounds__(256) void nn_overflow_kernel(const float *__restrict__ src, int64_t n, const float *__restrict__ tgt, int64_t m,
                                                          const double *__restrict__ T, const int32_t *__restrict__ done,
                                                          int32_t *__restrict__ cand_cnt, int32_t *__restrict__ cand,
                                                          const int32_t *__restrict__ over_rows)
{
    if (done && *done) return;
    const int total = cand_cnt[n];
    __shared__ double sv[256];
    __shared__ int sj[256];
    for (int e = blockIdx.x; e < total; e += gridDim.x) {
        const int64_t row = over_rows[e];
        double s[3];
        xform_row(T, src + 3 * row, s);
        const double seed = row_seed(s);
        double bv = INFINITY;
        int bj = INT_MAX;
        for (int64_t j = threadIdx.x; j < m; j += 256) {
            const double tx = tgt[3 * j], ty = tgt[3 * j + 1], tz = tgt[3 * j + 2];
            double d = fma(s[0], -2.0 * tx, seed);
            d = fma(s[1], -2.0 * ty, d);
            d = fma(s[2], -2.0 * tz, d);
            d = fma(1.0, fma(tx, tx, fma(ty, ty, tz * tz)), d);
            if (d < bv) { bv = d; bj = (int)j; }           // ascending j per thread: first minimum kept
        }
        sv[threadIdx.x] = bv; sj[threadIdx.x] = bj;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) {
                double ov = sv[threadIdx.x + w]; int oj = sj[threadIdx.x + w];
                if (ov < sv[threadIdx.x] || (ov == sv[threadIdx.x] && oj < sj[threadIdx.x])) { sv[threadIdx.x] = ov; sj[threadIdx.x] = oj; }
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) { cand[row * kCand] = sj[0]; cand_cnt[row] = 1; }
        __syncthreads();
    }
}

// ---- the MFMA nearest-neighbour sweep ------------------------------------------------------------------
// colid: the ORIGINAL target index of every column of B (the full operand or the seed operand: every kSeedStride-th tile), staged in LDS beside the tiles
// One form: every trip is examined behind the prefilter as it comes, whether the bounds are loose (seed sweep, first search) or tight
// (the previous partner under the new transform).  Until round 4 searches with tight bounds took a chunked form -- a hot pass of
// MFMAs + one v_min_u32 per result register over four column tiles, swept again the exact way only when some row's smallest high word
// reached its bound.  With the operands in curve order the prefilter rarely passes and the chunks' bookkeeping is pure overhead: per
// trip 0.545 against chunked 0.532 of the fp64 matrix peak inside a registration, 0.458 against 0.453 in a bare search
// (profiles/r04/nn_dense_sorted.txt), so the chunked form was removed.
__global__ __launch_bounds__(256, 4) void nn_mfma_kernel(int64_t n, const double *__restrict__ B, const int32_t *__restrict__ colid, int32_t tiles_per_split,
                                                         const int32_t *__restrict__ done,
                                                         const double *__restrict__ A64, const double *__restrict__ K64,
                                                         const double *__restrict__ init_val, const int32_t *__restrict__ init_idx,
                                                         double *__restrict__ part_val, int32_t *__restrict__ part_idx, const int32_t *__restrict__ rperm)
{
    // rperm (round 4): block row r is the caller's row rperm[r] -- the source's curve order, so that the 32 rows of a wave are neighbours
    // in space and reach the SAME few trips of the (curve-ordered) columns; operands and results stay indexed by the caller's row
    if (done && *done) return;
    __shared__ __align__(16) double lds[2][kStageDoubles];
    __shared__ __align__(16) int32_t lds_col[2][kCT * 16];           // the stage's ORIGINAL column indices (the operand stands in curve order)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row_base = (int64_t)blockIdx.x * kRowsPerBlock + (int64_t)wave * (kRT * 16);
    const int split = blockIdx.y;
    const int64_t t0 = (int64_t)split * tiles_per_split;
    const int nstages = tiles_per_split / kCT;

    // A operands: lane holds component k = lane>>4 of row (lane&15) of each of its row tiles
    double a[kRT];
#pragma unroll
    for (int rt = 0; rt < kRT; ++rt) {
        const int64_t row = row_base + rt * 16 + (lane & 15);
        a[rt] = row < n ? A64[(int64_t)rperm[row] * 4 + (lane >> 4)] : 0.0;
    }
    // C operands (row seeds K_i), running best and its column: D layout row = (lane>>4) + 4*reg
    d4 seed[kRT];
    double best[kRT][4];
    int32_t bcol[kRT][4];
#pragma unroll
    for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = row_base + rt * 16 + (lane >> 4) + 4 * r;
            double kk = 1.0, bv = INFINITY;
            int32_t bj = INT_MAX;
            if (row < n) {
                const int64_t ri = rperm[row];
                kk = K64[ri];
                if (init_val) { bv = init_val[ri]; bj = init_idx[ri]; }
            }
            seed[rt][r] = kk; best[rt][r] = bv; bcol[rt][r] = bj;
        }

    // B stream: global -> LDS by LDS-DMA (1 KiB per wave-instruction, 16 pieces per 16 KiB stage)
    const double *gB = B + t0 * 64;
    const int32_t *gC = colid + t0 * 16;
    auto stage_load = [&](int stage, int buf) {
        const double *g = gB + (int64_t)stage * kStageDoubles;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int piece = wave * 4 + q;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(g + piece * 128 + lane * 2),
                                             (__attribute__((address_space(3))) void *)(&lds[buf][piece * 128]), 16, 0, 0);
        }
        // 512 column ids = 2 KiB: waves 0 and 1, one 16-byte piece per lane
        if (wave < 2)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(gC + (int64_t)stage * (kCT * 16) + wave * 256 + lane * 4),
                                             (__attribute__((address_space(3))) void *)(&lds_col[buf][wave * 256]), 16, 0, 0);
    };
    stage_load(0, 0);
    __syncthreads();

    for (int st = 0; st < nstages; ++st) {
        const int buf = st & 1;
        if (st + 1 < nstages) stage_load(st + 1, buf ^ 1);
        const double *lb = lds[buf] + lane;
        // One trip = two column tiles x two row tiles = four MFMAs; examine() looks at a trip's 16 result registers: prefilter on the
        // high words (D > 0: the unsigned order of the bit patterns is the numeric order), exact (value, column) update only when
        // some lane passes (wave-uniform, rare once the bound is tight).
        auto examine = [&](const d4 &c00, const d4 &c10, const d4 &c01, const d4 &c11, const int ct) {
            bool pass = false;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned h0 = hi32(best[0][r]), h1 = hi32(best[1][r]);
                pass |= (bool)((int)(min(hi32(c00[r]), hi32(c01[r])) <= h0) | (int)(min(hi32(c10[r]), hi32(c11[r])) <= h1));
            }
            if (__builtin_amdgcn_ballot_w64(pass) == 0) return;
            const int32_t col0 = lds_col[buf][ct * 16 + (lane & 15)], col1 = lds_col[buf][ct * 16 + 16 + (lane & 15)];
            bool anyeq = false;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned h0 = hi32(best[0][r]), h1 = hi32(best[1][r]);
                anyeq |= (bool)((int)(hi32(c00[r]) == h0) | (int)(hi32(c01[r]) == h0) | (int)(hi32(c10[r]) == h1) | (int)(hi32(c11[r]) == h1));
                // two candidates of one row with equal high words: the second must be compared exactly with the first
                // once that has become the running best (found by the random cross-engine test: far-apart line clouds)
                anyeq |= (bool)((int)(hi32(c00[r]) == hi32(c01[r])) | (int)(hi32(c10[r]) == hi32(c11[r])));
            }
            if (__builtin_amdgcn_ballot_w64(anyeq) == 0) {
                // every high word differs from its bound: the high words alone decide "<" (no fp64 op)
#define KPX_NN_HI(ACC, RT, COL)                                                                     \
                _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                    \
                    const bool t = hi32(ACC[r]) < hi32(best[RT][r]);                               \
                    best[RT][r] = t ? ACC[r] : best[RT][r];                                        \
                    bcol[RT][r] = t ? (COL) : bcol[RT][r];                                         \
                }
                KPX_NN_HI(c00, 0, col0) KPX_NN_HI(c01, 0, col1) KPX_NN_HI(c10, 1, col0) KPX_NN_HI(c11, 1, col1)
#undef KPX_NN_HI
            } else {
                // near-ties (equal high words, e.g. the bound's own column): exact lexicographic (value, column)
#define KPX_NN_EXACT(ACC, RT, COL)                                                                  \
                _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                    \
                    const bool t = (int)(ACC[r] < best[RT][r]) | ((int)(ACC[r] == best[RT][r]) & (int)((COL) < bcol[RT][r])); \
                    best[RT][r] = t ? ACC[r] : best[RT][r];                                        \
                    bcol[RT][r] = t ? (COL) : bcol[RT][r];                                         \
                }
                KPX_NN_EXACT(c00, 0, col0) KPX_NN_EXACT(c01, 0, col1) KPX_NN_EXACT(c10, 1, col0) KPX_NN_EXACT(c11, 1, col1)
#undef KPX_NN_EXACT
            }
        };
#define KPX_NN_TRIP(P, CT)                                                                          \
        const double P##b0 = lb[(CT) * 64], P##b1 = lb[(CT) * 64 + 64];                             \
        const d4 P##00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0], P##b0, seed[0], 0, 0, 0);       \
        const d4 P##10 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[1], P##b0, seed[1], 0, 0, 0);       \
        const d4 P##01 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0], P##b1, seed[0], 0, 0, 0);       \
        const d4 P##11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[1], P##b1, seed[1], 0, 0, 0);
#pragma unroll 1
        for (int ct = 0; ct < kCT; ct += 2) {
            KPX_NN_TRIP(p, ct)
            examine(p00, p10, p01, p11, ct);
        }
#undef KPX_NN_TRIP
        __syncthreads();
    }

    // reduce over the 16 lanes that hold the same rows (lexicographic (value, column) minimum)
#pragma unroll
    for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double v = best[rt][r];
            int32_t c = bcol[rt][r];
#pragma unroll
            for (int msk = 1; msk < 16; msk <<= 1) {
                double ov = __shfl_xor(v, msk, 64);
                int32_t oc = __shfl_xor(c, msk, 64);
                bool take = ov < v || (ov == v && oc < c);
                v = take ? ov : v;
                c = take ? oc : c;
            }
            int64_t row = row_base + rt * 16 + (lane >> 4) + 4 * r;
            if ((lane & 15) == 0 && row < n) {
                const int64_t ri = rperm[row];
                part_val[(int64_t)split * n + ri] = v;
                part_idx[(int64_t)split * n + ri] = c;
            }
        }
}

// ---- merge splits, direct distance, accumulation ---------------------------------------------------------
// mode: -2 = write (value, column) as the bound of the next sweep, -1 = correspondences only,
//        0 = point-to-point sums, 1 = + point-to-plane normal equations
//        2 = coloured ICP ([O3D] TransformationEstimationForColoredICP): the normal equations hold a geometric row
//            sqrt(lambda) (s x n, n | (s - t).n) and a photometric row sqrt(1 - lambda) (s x g', g' | I_s - (I_t + g.(s' - t))),
//            s' = s projected onto the target's tangent plane, g the target's colour gradient, g' = -(I - n n^T) g
//        3 = generalized ICP (GicpTerms / RobustGicpTerms: those instantiations only): three rows per pair, see gicp_pair_rows
// The kernel is a template on its pair term: nn_merge_kernel<ColorTerms> serves modes -2..2, nn_merge_kernel<GicpTerms> mode 3 (the
// 3x3 eigen-solve of a GICP pair never enters the instantiation every point-to-point / point-to-plane registration runs).
// Robust registrations (kpx_icp_robust, kpx_colored_icp_robust, kpx_generalized_icp_robust) take instantiations of their own,
// nn_merge_kernel<RobustColorTerms> (modes 1 and 2) and nn_merge_kernel<RobustGicpTerms> (mode 3): every residual row of modes 1..3
// goes through robust_row (kpx_icpdefs.h), weighted by the loss of its own residual -- the one row of point-to-plane, the two SCALED
// rows of coloured ICP (sqrt(lambda) r_G, sqrt(1 - lambda) r_I), the three rows r_i = w_i . d of a GICP pair.  Slots 0..16 (count,
// sum d2, the point-to-point sums) stay unweighted: fitness, inlier rmse, the correspondences and the convergence test do not depend
// on the loss, as in Open3D.  The weighting stands behind `if constexpr`: the two instantiations above compile as they did without it.
struct ColorTerms {
    static constexpr bool kGicp = false, kRobust = false;
    const float *src_col, *tgt_col;
    const double *tgt_grad;
    double sqrt_lg, sqrt_lp;
};
struct GicpTerms {
    static constexpr bool kGicp = true, kRobust = false;
    const double *src_cov, *tgt_cov;       // [n_src][9], [n_tgt][9] row-major, in the ORIGINAL source frame / the target's frame
};
struct RobustColorTerms : ColorTerms {
    static constexpr bool kRobust = true;
    RobustLoss loss;
};
struct RobustGicpTerms : GicpTerms {
    static constexpr bool kRobust = true;
    RobustLoss loss;
};
constexpr int kModeGicp = 3;

// [O3D] TransformationEstimationForGeneralizedICP, one correspondence (s = T src_i in fp64, t its target partner):
//   Cs' = R Cs R^T (R = rotation of the current T: Open3D rotates the source's covariances with every PointCloud::Transform),
//   M = Ct + Cs', W = M^{-1/2} = V diag(lambda^{-1/2}) V^T (sym3_eigen), d = s - t,
//   rows i = 0..2: residual r_i = w_i . d, Jacobian J_i = (s x w_i, w_i) with w_i row i of W,
// accumulated into the point-to-plane slots 17..43 (J^T J upper triangle, J^T r); the update is the point-to-plane solve.
// Deviation: Open3D yields NaN when M is singular (e.g. two exactly flat neighbourhoods with aligned normals, raw covariances);
// here a pair whose smallest eigenvalue of M is <= 0, or whose W is not finite, adds nothing to slots 17..43.
template <class Terms>
__device__ __forceinline__ void gicp_pair_rows(const Terms &ct, const double *__restrict__ T, const double *__restrict__ Cs,
                                               const double *__restrict__ Ct, const double s[3], const double t[3], double acc[kAcc])
{
    double RC[9];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q) RC[3 * p + q] = T[4 * p] * Cs[q] + T[4 * p + 1] * Cs[3 + q] + T[4 * p + 2] * Cs[6 + q];
    double M[6];
    {
        int e = 0;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p; q < 3; ++q)
                M[e++] = (RC[3 * p] * T[4 * q] + RC[3 * p + 1] * T[4 * q + 1] + RC[3 * p + 2] * T[4 * q + 2]) + Ct[3 * p + q];
    }
    double lam[3], V[9];
    sym3_eigen(M, lam, V);
    if (!(lam[0] > 0.0)) return;
    double il[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) il[c] = 1.0 / sqrt(lam[c]);
    double W[9];
    bool finite = true;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            W[3 * p + q] = V[3 * p] * il[0] * V[3 * q] + V[3 * p + 1] * il[1] * V[3 * q + 1] + V[3 * p + 2] * il[2] * V[3 * q + 2];
            finite = finite && isfinite(W[3 * p + q]);
        }
    if (!finite) return;
    const double d[3] = { s[0] - t[0], s[1] - t[1], s[2] - t[2] };
#pragma unroll
    for (int row = 0; row < 3; ++row) {
        const double wx = W[3 * row], wy = W[3 * row + 1], wz = W[3 * row + 2];
        const double r = wx * d[0] + wy * d[1] + wz * d[2];
        const double J[6] = { s[1] * wz - s[2] * wy, s[2] * wx - s[0] * wz, s[0] * wy - s[1] * wx, wx, wy, wz };
        if constexpr (Terms::kRobust) {
            robust_row(ct.loss, J, r, acc);
        } else {
            int q = 17;
#pragma unroll
            for (int p = 0; p < 6; ++p)
#pragma unroll
                for (int c = p; c < 6; ++c) acc[q++] += J[p] * J[c];
#pragma unroll
            for (int p = 0; p < 6; ++p) acc[38 + p] += J[p] * r;
        }
    }
}

constexpr int kMergeThreads = 64;
template <class Terms>
__global__ __launch_bounds__(kMergeThreads) void nn_merge_kernel(const float *__restrict__ src, int64_t n, const float *__restrict__ tgt,
                                                       const float *__restrict__ tn, const double *__restrict__ T,
                                                       const int32_t *__restrict__ done, const double *__restrict__ part_val,
                                                       const int32_t *__restrict__ part_idx, int splits, double max_d2, int mode,
                                                       int32_t *__restrict__ idx_out, double *__restrict__ d2_out,
                                                       double *__restrict__ val_out, double *__restrict__ part_acc,
                                                       const int32_t *__restrict__ cand_cnt, const int32_t *__restrict__ cand, Terms ct)
{
    if (done && *done) return;
    __shared__ double sh[kAcc][kMergeThreads + 1];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double acc[kAcc];
#pragma unroll
    for (int q = 0; q < kAcc; ++q) acc[q] = 0.0;
    if (i < n) {
        double bv = part_val[i];
        int32_t bj = part_idx[i];
        if (cand_cnt) {
            // screening path: (part_val, part_idx) hold the bound (exact D of last iteration's partner); the exact
            // metric of every screened candidate decides, by the same fma chain as the MFMA sweep
            double s[3];
            xform_row(T, src + 3 * i, s);
            const double seed = row_seed(s);
            int c = cand_cnt[i];
            c = c < kCand ? c : kCand;
            for (int e = 0; e < c; ++e) {
                const int32_t j = cand[i * kCand + e];
                const float *tp = tgt + 3 * (int64_t)j;
                const double tx = tp[0], ty = tp[1], tz = tp[2];
                double d = fma(s[0], -2.0 * tx, seed);
                d = fma(s[1], -2.0 * ty, d);
                d = fma(s[2], -2.0 * tz, d);
                d = fma(1.0, fma(tx, tx, fma(ty, ty, tz * tz)), d);
                if (d < bv || (d == bv && j < bj)) { bv = d; bj = j; }
            }
        } else {
            for (int s = 1; s < splits; ++s) {
                double v = part_val[(int64_t)s * n + i];
                int32_t j = part_idx[(int64_t)s * n + i];
                if (v < bv || (v == bv && j < bj)) { bv = v; bj = j; }
            }
        }
        const bool none = bj < 0 || bj == INT_MAX;        // culled sweep inside a registration: nothing within max_dist
        if (idx_out) idx_out[i] = none ? -1 : bj;
        if (mode == -2) {
            val_out[i] = bv;
        } else if (none) {
            if (d2_out) d2_out[i] = INFINITY;
        } else {
            double s[3];
            xform_row(T, src + 3 * i, s);
            const float *tp = tgt + 3 * (int64_t)bj;
            const double t[3] = { (double)tp[0], (double)tp[1], (double)tp[2] };
            const double d2 = pair_d2(s, t);
            if (d2_out) d2_out[i] = d2;
            if (mode >= 0 && d2 < max_d2) {
                // (the plain point-to-plane terms come with the point-to-point ones; GICP, the robust losses and the coloured mode form theirs below)
                const bool plane = !Terms::kGicp && !Terms::kRobust && mode == 1;
                pair_terms(s, t, d2, true, plane, plane ? tn + 3 * (int64_t)bj : (const float *)nullptr, [&](int q, double v) { acc[q] = v; });
                if constexpr (Terms::kGicp) {
                    gicp_pair_rows(ct, T, ct.src_cov + 9 * i, ct.tgt_cov + 9 * (int64_t)bj, s, t, acc);
                } else if (mode == 1) {
                    if constexpr (Terms::kRobust) {
                        double J[6];
                        const double r = plane_row(s, t, tn + 3 * (int64_t)bj, J);
                        robust_row(ct.loss, J, r, acc);
                    }
                } else if (mode == 2) {
                    const float *np_ = tn + 3 * (int64_t)bj;
                    const double nv[3] = { np_[0], np_[1], np_[2] };
                    const double rg = (s[0] - t[0]) * nv[0] + (s[1] - t[1]) * nv[1] + (s[2] - t[2]) * nv[2];
                    const double is = ((double)ct.src_col[3 * i] + (double)ct.src_col[3 * i + 1] + (double)ct.src_col[3 * i + 2]) / 3.0;
                    const float *tc = ct.tgt_col + 3 * (int64_t)bj;
                    const double it = ((double)tc[0] + (double)tc[1] + (double)tc[2]) / 3.0;
                    const double *gp = ct.tgt_grad + 3 * (int64_t)bj;
                    const double g[3] = { gp[0], gp[1], gp[2] };
                    const double sp[3] = { s[0] - rg * nv[0], s[1] - rg * nv[1], s[2] - rg * nv[2] };
                    const double is0 = (g[0] * (sp[0] - t[0]) + g[1] * (sp[1] - t[1]) + g[2] * (sp[2] - t[2])) + it;
                    const double gn = g[0] * nv[0] + g[1] * nv[1] + g[2] * nv[2];
                    const double gm[3] = { -(g[0] - gn * nv[0]), -(g[1] - gn * nv[1]), -(g[2] - gn * nv[2]) };
                    const double JG[6] = { ct.sqrt_lg * (s[1] * nv[2] - s[2] * nv[1]), ct.sqrt_lg * (s[2] * nv[0] - s[0] * nv[2]),
                                           ct.sqrt_lg * (s[0] * nv[1] - s[1] * nv[0]), ct.sqrt_lg * nv[0], ct.sqrt_lg * nv[1], ct.sqrt_lg * nv[2] };
                    const double JI[6] = { ct.sqrt_lp * (s[1] * gm[2] - s[2] * gm[1]), ct.sqrt_lp * (s[2] * gm[0] - s[0] * gm[2]),
                                           ct.sqrt_lp * (s[0] * gm[1] - s[1] * gm[0]), ct.sqrt_lp * gm[0], ct.sqrt_lp * gm[1], ct.sqrt_lp * gm[2] };
                    const double rG = ct.sqrt_lg * rg, rI = ct.sqrt_lp * (is - is0);
                    if constexpr (Terms::kRobust) {
                        robust_row(ct.loss, JG, rG, acc);
                        robust_row(ct.loss, JI, rI, acc);
                    } else {
                        int q = 17;
#pragma unroll
                        for (int p = 0; p < 6; ++p)
#pragma unroll
                            for (int c = p; c < 6; ++c) acc[q++] = JG[p] * JG[c] + JI[p] * JI[c];
#pragma unroll
                        for (int p = 0; p < 6; ++p) acc[38 + p] = JG[p] * rG + JI[p] * rI;
                    }
                }
            }
        }
    }
    if (mode < 0) return;
    // fixed-order block sums through LDS: slot q of lane l at sh[q][l] (row stride 65 doubles: conflict-free
    // column walks), lane q then adds its row in lane order -- no cross-lane shuffles (a 64-lane fp64 shuffle
    // tree for 44 slots costs ~500 ds_bpermutes per wave)
    const int nacc = mode >= 1 ? kAcc : 17;
#pragma unroll
    for (int q = 0; q < kAcc; ++q)
        if (q < 17 || mode >= 1) sh[q][threadIdx.x] = acc[q];
    __syncthreads();
    if ((int)threadIdx.x < nacc) {
        double v = 0.0;
        for (int l = 0; l < kMergeThreads; ++l) v += sh[threadIdx.x][l];
        part_acc[(int64_t)blockIdx.x * kAcc + threadIdx.x] = v;
    }
}

}  // namespace kpx
