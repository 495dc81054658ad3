// kpx_tsdfblocks.hip -- the block-sparse TSDF volume ([O3D] pipelines.integration.ScalableTSDFVolume; arithmetic contract AC16,
// DESIGN.md 3 and 5.17): blocks ("volume units") of R^3 voxels on the world lattice, allocated where a depth image's surface band
// falls.  The storage is the caller's: a pool f32 [capacity][R^3][2] = {tsdf, weight} (and f32 [capacity][R^3][3] colours), voxel
// (x, y, z) of a block at (x R + y) R + z, and a sorted index: keys u64 [B] ascending, key = (bx + 2^20) << 42 | (by + 2^20) << 21 |
// (bz + 2^20), with the pool slot of each.  The library never allocates: the pool grows in the caller.
//
//   touch      the blocks the sampled pixels of up to KPX_TSDF_MAX_SENSORS images touch: a fixed number of key slots per pixel,
//              one 64-bit sort, heads counted and filled per 512 keys -> unique keys, their image masks and pool slots (an unknown
//              key takes slot B + its rank among the unknown ones), {touched, new, range error} at a device count
//   insert     merges the new keys into a second index array (every key finds its place with one binary search) and zeroes the
//              new pool slots
//   integrate  one workgroup per touched block, AC9's update (tsdf_observe) for the images of the block's mask
//   extract / mesh   the uniform volume's count -> scan -> fill over the virtual linear index rank(block) R^3 + local; a
//              27-neighbour table per block, built first with one binary search each, resolves voxels of adjacent blocks
#include "kpx_sort.h"
#include "kpx_tsdfcore.h"
#include "kpx_mccore.h"

#include <math.h>

namespace kpx {
namespace {

constexpr int kBias = 1 << 20;
constexpr uint64_t kNoKey = ~0ull;                  // bit 63 set: sorts behind every key

__device__ __forceinline__ uint64_t blk_pack(int bx, int by, int bz)
{
    return (uint64_t)(uint32_t)(bx + kBias) << 42 | (uint64_t)(uint32_t)(by + kBias) << 21 | (uint64_t)(uint32_t)(bz + kBias);
}
__device__ __forceinline__ void blk_unpack(uint64_t key, int b[3])
{
    b[0] = (int)((key >> 42) & 0x1FFFFFull) - kBias;
    b[1] = (int)((key >> 21) & 0x1FFFFFull) - kBias;
    b[2] = (int)(key & 0x1FFFFFull) - kBias;
}
__device__ __forceinline__ bool blk_in_range(int bx, int by, int bz)
{
    return bx >= -kBias && bx < kBias && by >= -kBias && by < kBias && bz >= -kBias && bz < kBias;
}
// rank of `key` in the ascending keys[0, n), -1 when it is not there
__device__ __forceinline__ int32_t blk_find(const uint64_t *__restrict__ keys, int32_t n, uint64_t key)
{
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < n && keys[lo] == key ? lo : -1;
}
// how many of keys[0, n) are below `key`
__device__ __forceinline__ int32_t blk_lower(const uint64_t *__restrict__ keys, int32_t n, uint64_t key)
{
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- touch ---------------------------------------------------------------------------------------------------------------------
struct TouchArgs {
    double P[KPX_TSDF_MAX_SENSORS][12];        // camera -> world, rows 0..2
    const void *depth[KPX_TSDF_MAX_SENSORS];
    double fx, fy, cx, cy, ul, trunc;
    float scale, dtrunc;
    int32_t W, H, stride, nw, nh, count, nax, u16;
};

// One thread per (image, sampled pixel): nax^3 key slots, slot k of thread t at [k NP + t] (coalesced), kNoKey in the unused ones.
__global__ __launch_bounds__(256) void blk_emit_kernel(TouchArgs a, int64_t np, uint64_t *__restrict__ keys, int32_t *__restrict__ vals, int32_t *__restrict__ err)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= np) return;
    const int32_t nsamp = a.nw * a.nh;
    const int s = (int)(t / nsamp);
    const int q = (int)(t - (int64_t)s * nsamp);
    const int i = (q / a.nw) * a.stride, j = (q % a.nw) * a.stride;
    const int64_t pix = (int64_t)i * a.W + j;
    float d;
    if (a.u16) {
        d = (float)((const uint16_t *)a.depth[s])[pix] / a.scale;
        if (d > a.dtrunc) d = 0.0f;
    } else {
        d = ((const float *)a.depth[s])[pix];
    }
    int lo[3] = { 0, 0, 0 }, n[3] = { 0, 0, 0 };
    if (d > 0.0f) {
        const double z = (double)d;
        const double x = ((double)j - a.cx) * z / a.fx;
        const double y = ((double)i - a.cy) * z / a.fy;
        const double *P = a.P[s];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double p = fma(P[4 * k], x, fma(P[4 * k + 1], y, fma(P[4 * k + 2], z, P[4 * k + 3])));
            const double l = floor((p - a.trunc) / a.ul), h = floor((p + a.trunc) / a.ul);
            if (!(l >= (double)-kBias && h < (double)kBias)) { ok = false; continue; }          // also what is not finite
            lo[k] = (int)l;
            const int span = (int)h - (int)l + 1;
            n[k] = span < a.nax ? span : a.nax;
        }
        if (!ok) {
            *err = 1;
            n[0] = 0;
        }
    }
    int k = 0;
    for (int dx = 0; dx < a.nax; ++dx)
        for (int dy = 0; dy < a.nax; ++dy)
            for (int dz = 0; dz < a.nax; ++dz, ++k) {
                const bool in = n[0] > 0 && dx < n[0] && dy < n[1] && dz < n[2];
                keys[(int64_t)k * np + t] = in ? blk_pack(lo[0] + dx, lo[1] + dy, lo[2] + dz) : kNoKey;
                vals[(int64_t)k * np + t] = s;
            }
}

__global__ __launch_bounds__(kExtractWaves * 64) void blk_heads_count_kernel(const uint64_t *__restrict__ sorted, int64_t n, int64_t nchunks,
                                                                             const uint64_t *__restrict__ index, int32_t nblocks,
                                                                             int64_t *__restrict__ hcount, int64_t *__restrict__ ncount)
{
    const int64_t chunk = (int64_t)blockIdx.x * kExtractWaves + wave_id();
    if (chunk >= nchunks) return;
    int h = 0, nw = 0;
    for (int r = 0; r < kChunkRounds; ++r) {
        const int64_t i = chunk * kChunk + r * 64 + lane_id();
        if (i >= n) continue;
        const uint64_t key = sorted[i];
        if (key == kNoKey || (i > 0 && sorted[i - 1] == key)) continue;
        ++h;
        if (blk_find(index, nblocks, key) < 0) ++nw;
    }
    h = wave_sum(h);
    nw = wave_sum(nw);
    if (lane_id() == 0) {
        hcount[chunk] = h;
        ncount[chunk] = nw;
    }
}

// ukeys / tslot may be the sort's input arrays: nothing reads those after the sort.  tmask is cleared before the launch.
__global__ __launch_bounds__(kExtractWaves * 64) void blk_heads_fill_kernel(const uint64_t *__restrict__ sorted, const int32_t *__restrict__ svals, int64_t n,
                                                                            int64_t nchunks, const uint64_t *__restrict__ index,
                                                                            const int32_t *__restrict__ islots, int32_t nblocks,
                                                                            const int64_t *__restrict__ hoff, const int64_t *__restrict__ noff,
                                                                            uint64_t *__restrict__ ukeys, int32_t *__restrict__ tslot,
                                                                            uint32_t *__restrict__ tmask, uint64_t *__restrict__ newkeys)
{
    const int64_t chunk = (int64_t)blockIdx.x * kExtractWaves + wave_id();
    if (chunk >= nchunks) return;
    const int lane = lane_id();
    const unsigned long long upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull, below = (1ull << lane) - 1ull;
    int64_t hpos = hoff[chunk], npos = noff[chunk];
    for (int r = 0; r < kChunkRounds; ++r) {
        const int64_t i = chunk * kChunk + r * 64 + lane;
        uint64_t key = kNoKey;
        int32_t val = 0, found = -1;
        bool head = false, sub = false;
        if (i < n) {
            key = sorted[i];
            val = svals[i];
            if (key != kNoKey) {
                head = i == 0 || sorted[i - 1] != key;
                sub = head || svals[i - 1] != val;
                if (head) found = blk_find(index, nblocks, key);
            }
        }
        const bool isnew = head && found < 0;
        const unsigned long long hb = __ballot(head), nb = __ballot(isnew);
        const int64_t urank = hpos + __builtin_popcountll(hb & upto) - 1;          // >= 0 for every valid key: a head precedes it
        if (head) {
            ukeys[urank] = key;
            if (isnew) {
                const int64_t nrank = npos + __builtin_popcountll(nb & below);
                newkeys[nrank] = key;
                tslot[urank] = nblocks + (int32_t)nrank;
            } else {
                tslot[urank] = islots[found];
            }
        }
        if (sub) atomicOr(&tmask[urank], 1u << val);
        hpos += __builtin_popcountll(hb);
        npos += __builtin_popcountll(nb);
    }
}

__global__ void blk_touch_done_kernel(const int64_t *__restrict__ hoff, const int64_t *__restrict__ noff, int64_t nchunks, const int32_t *__restrict__ err,
                                      int64_t *__restrict__ out)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        out[0] = hoff[nchunks];
        out[1] = noff[nchunks];
        out[2] = *err;
    }
}

using TouchSort = DeviceSort<uint64_t, true, kSortDefault>;
struct TouchScratch {
    TouchSort sort;
    int64_t *hoff, *noff;
    uint32_t *tmask;
    uint64_t *newkeys;
    int32_t *err;
    uint64_t *ukeys;           // = sort.keys_in
    int32_t *tslot;            // = sort.vals_in
    int64_t np, n, nchunks;
    int32_t nw, nh, nax;
};
// the shape of a touch workspace: what the host knows before the launch
struct TouchShape {
    int32_t count, W, H, stride;
    double ul, trunc;
};
inline bool touch_shape_ok(const TouchShape &s)
{
    return s.count >= 1 && s.count <= KPX_TSDF_MAX_SENSORS && s.W > 0 && s.H > 0 && (int64_t)s.W * s.H < ((int64_t)1 << 31) && s.stride >= 1 && s.ul > 0.0 &&
           s.trunc > 0.0 && s.trunc <= s.ul;
}
// Blocks per axis one pixel can touch: trunc <= ul bounds hi - lo by 2 in exact arithmetic; the two quotients round separately, so
// one more is allowed for where 2 trunc / ul is at or above 1 (a band of a whole block or more).
inline int32_t touch_nax(const TouchShape &s) { return 2.0 * s.trunc / s.ul >= 1.0 ? 4 : 3; }
void touch_carve(Arena &a, const TouchShape &s, TouchScratch *t)
{
    t->nw = (s.W + s.stride - 1) / s.stride;
    t->nh = (s.H + s.stride - 1) / s.stride;
    t->nax = touch_nax(s);
    t->np = (int64_t)s.count * t->nw * t->nh;
    t->n = t->np * t->nax * t->nax * t->nax;
    t->nchunks = cdiv(t->n, kChunk);
    dsort_carve(a, t->n, 64, SortOptions(), &t->sort);
    t->hoff = a.get<int64_t>((size_t)t->nchunks + 1);
    t->noff = a.get<int64_t>((size_t)t->nchunks + 1);
    t->tmask = a.get<uint32_t>((size_t)t->n);
    t->newkeys = a.get<uint64_t>((size_t)t->n);
    t->err = a.get<int32_t>(1);
    t->ukeys = t->sort.keys_in;
    t->tslot = t->sort.vals_in;
}

__global__ __launch_bounds__(256) void blk_merge_kernel(const uint64_t *__restrict__ okeys, const int32_t *__restrict__ oslots, int32_t nold,
                                                        const uint64_t *__restrict__ newkeys, int32_t nnew, uint64_t *__restrict__ keys, int32_t *__restrict__ slots)
{
    const int32_t t = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (t < nold) {
        const uint64_t k = okeys[t];
        const int32_t pos = t + blk_lower(newkeys, nnew, k);
        keys[pos] = k;
        slots[pos] = oslots[t];
    } else if (t < nold + nnew) {
        const int32_t j = t - nold;
        const uint64_t k = newkeys[j];
        const int32_t pos = j + blk_lower(okeys, nold, k);
        keys[pos] = k;
        slots[pos] = nold + j;
    }
}

// ---- integrate -----------------------------------------------------------------------------------------------------------------
// One workgroup per touched block; a thread owns pairs of consecutive-z voxels (16-byte accesses when R^3 is even, so that every
// block starts 16-byte aligned; the last pair of an odd block is a single voxel).  a.org is unused: the block's origin is b ul.
template <bool U16, bool COLOR>
__global__ __launch_bounds__(256) void blk_integrate_kernel(float2 *__restrict__ pool, float *__restrict__ cpool, const uint64_t *__restrict__ ukeys,
                                                            const int32_t *__restrict__ tslot, const uint32_t *__restrict__ tmask, double ul, TsdfIntegrateArgs a)
{
    const int R = a.res, R3 = R * R * R;
    const bool wide = (R3 & 1) == 0;
    int b[3];
    blk_unpack(ukeys[blockIdx.x], b);
    const uint32_t mask = tmask[blockIdx.x];
    float2 *vol = pool + (int64_t)tslot[blockIdx.x] * R3;
    float *col = COLOR ? cpool + 3 * (int64_t)tslot[blockIdx.x] * R3 : nullptr;
    const double org[3] = { (double)b[0] * ul, (double)b[1] * ul, (double)b[2] * ul };
    for (int lin0 = 2 * (int)threadIdx.x; lin0 < R3; lin0 += 512) {
        const bool two = lin0 + 1 < R3;
        double c[2][3];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int l = two ? lin0 + k : lin0;
            const int z = l % R, x = (l / R) / R, y = (l / R) % R;
            c[k][0] = org[0] + ((double)x + 0.5) * a.vl;
            c[k][1] = org[1] + ((double)y + 0.5) * a.vl;
            c[k][2] = org[2] + ((double)z + 0.5) * a.vl;
        }
        float f[2] = { 0.0f, 0.0f }, w[2] = { 0.0f, 0.0f }, cc[2][3] = { { 0.0f, 0.0f, 0.0f }, { 0.0f, 0.0f, 0.0f } };
        bool loaded = false;
        for (int s = 0; s < a.count; ++s) {
            if (!((mask >> s) & 1u)) continue;
            float t[2], rgb[2][3];
            bool upd[2];
            upd[0] = tsdf_observe<U16, COLOR>(a, a.s[s], c[0], &t[0], rgb[0]);
            upd[1] = two && tsdf_observe<U16, COLOR>(a, a.s[s], c[1], &t[1], rgb[1]);
            if (!(upd[0] || upd[1])) continue;
            if (!loaded) {
                loaded = true;
                if (two && wide) {
                    const float4 q = *reinterpret_cast<const float4 *>(vol + lin0);
                    f[0] = q.x; w[0] = q.y; f[1] = q.z; w[1] = q.w;
                } else {
                    const float2 q = vol[lin0];
                    f[0] = q.x; w[0] = q.y;
                    if (two) { const float2 q1 = vol[lin0 + 1]; f[1] = q1.x; w[1] = q1.y; }
                }
                if (COLOR) {
                    if (two && wide) {
                        const float2 *cp = reinterpret_cast<const float2 *>(col + 3 * lin0);        // 24-byte stride: 8-byte aligned
                        const float2 q0 = cp[0], q1 = cp[1], q2 = cp[2];
                        cc[0][0] = q0.x; cc[0][1] = q0.y; cc[0][2] = q1.x; cc[1][0] = q1.y; cc[1][1] = q2.x; cc[1][2] = q2.y;
                    } else {
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) {
                            cc[0][ch] = col[3 * lin0 + ch];
                            if (two) cc[1][ch] = col[3 * lin0 + 3 + ch];
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (!upd[k]) continue;
                const float w1 = w[k] + 1.0f;
                f[k] = (f[k] * w[k] + t[k]) / w1;
                if (COLOR) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) cc[k][ch] = (cc[k][ch] * w[k] + rgb[k][ch]) / w1;
                }
                w[k] = w1;
            }
        }
        if (!loaded) continue;
        if (two && wide) {
            *reinterpret_cast<float4 *>(vol + lin0) = make_float4(f[0], w[0], f[1], w[1]);
        } else {
            vol[lin0] = make_float2(f[0], w[0]);
            if (two) vol[lin0 + 1] = make_float2(f[1], w[1]);
        }
        if (COLOR) {
            if (two && wide) {
                float2 *cp = reinterpret_cast<float2 *>(col + 3 * lin0);
                cp[0] = make_float2(cc[0][0], cc[0][1]);
                cp[1] = make_float2(cc[0][2], cc[1][0]);
                cp[2] = make_float2(cc[1][1], cc[1][2]);
            } else {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    col[3 * lin0 + ch] = cc[0][ch];
                    if (two) col[3 * lin0 + 3 + ch] = cc[1][ch];
                }
            }
        }
    }
}

// ---- the view of the blocks (kpx_tsdfcore.h) ---------------------------------------------------------------------------------------
__device__ __forceinline__ int blk_floordiv(int x, int r) { return x >= 0 ? x / r : -((-x + r - 1) / r); }

// The sweeps run over the virtual linear index rank(block) R^3 + local.  Interpolation works in world coordinates; there is no
// neighbour that the surface leaves out: a voxel in an absent block closes no crossing.
struct BlkView {
    const uint64_t *keys;          // [B] ascending
    const int32_t *slots;          // [B] pool slot
    const int32_t *nbr;            // [B][27] rank of the block at (dx, dy, dz) in {-1, 0, 1}^3, -1 = absent
    const float2 *vol;             // the pool
    const float *col;
    double vl, ul;                 // the fills'
    int32_t B, R, R3;
    struct Cell {
        int32_t rank;
        int l, p[3];               // the voxel in its block: l = (p[0] R + p[1]) R + p[2]
        int b[3];                  // the block's index, once anchored
    };
    __device__ __forceinline__ int64_t size() const { return (int64_t)B * R3; }
    __device__ __forceinline__ Cell split(int64_t vlin) const
    {
        Cell c;
        c.rank = (int32_t)(vlin / R3);
        c.l = (int)(vlin - (int64_t)c.rank * R3);
        c.p[2] = c.l % R;                    // signed, as at()'s: the compiler then takes 1 / R once for all of them
        c.p[0] = (c.l / R) / R;
        c.p[1] = (c.l / R) % R;
        return c;
    }
    // from l, not from p[]: the voxel's load then waits for the rank alone and not for the divisions by R
    __device__ __forceinline__ int64_t self(const Cell &c) const { return (int64_t)slots[c.rank] * R3 + c.l; }
    __device__ __forceinline__ int64_t at(const Cell &c, int ox, int oy, int oz, int64_t *virt) const
    {
        const int x = c.p[0] + ox, y = c.p[1] + oy, z = c.p[2] + oz;
        const int dx = blk_floordiv(x, R), dy = blk_floordiv(y, R), dz = blk_floordiv(z, R);
        int32_t nr = c.rank;
        if (dx | dy | dz) {
            if (dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1 && dz >= -1 && dz <= 1) {
                nr = nbr[(int64_t)c.rank * 27 + (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1)];
            } else {                                  // R = 1: a normal's tap two blocks away
                int b[3];
                blk_unpack(keys[c.rank], b);
                nr = blk_in_range(b[0] + dx, b[1] + dy, b[2] + dz) ? blk_find(keys, B, blk_pack(b[0] + dx, b[1] + dy, b[2] + dz)) : -1;
            }
            if (nr < 0) return -1;
        }
        const int local = ((x - dx * R) * R + (y - dy * R)) * R + (z - dz * R);
        *virt = (int64_t)nr * R3 + local;
        return (int64_t)slots[nr] * R3 + local;
    }
    __device__ __forceinline__ bool surface_neighbour(const Cell &, int) const { return true; }
    __device__ __forceinline__ void anchor(Cell &c) const { blk_unpack(keys[c.rank], c.b); }
    __device__ __forceinline__ double centre(const Cell &c, int k) const { return (double)c.b[k] * ul + ((double)c.p[k] + 0.5) * vl; }
    __device__ __forceinline__ double world(double p, int) const { return p; }
    __device__ __forceinline__ int tap0(const Cell &c, double fl, int k) const { return (int)(fl - (double)c.b[k] * (double)R); }
};

__global__ __launch_bounds__(256) void blk_neighbours_kernel(const uint64_t *__restrict__ keys, int32_t nblocks, int32_t *__restrict__ nbr)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)nblocks * 27) return;
    const int32_t rank = (int32_t)(t / 27);
    const int k = (int)(t - (int64_t)rank * 27);
    int b[3];
    blk_unpack(keys[rank], b);
    const int bx = b[0] + k / 9 - 1, by = b[1] + (k / 3) % 3 - 1, bz = b[2] + k % 3 - 1;
    nbr[t] = k == 13 ? rank : blk_in_range(bx, by, bz) ? blk_find(keys, nblocks, blk_pack(bx, by, bz)) : -1;
}

// marching cubes, sweep 1: a corner in an absent block makes the cube inactive.  Eight loads and little else; it keeps its own form
// because the uniform one (kpx_tsdfmesh.hip) pairs its loads along z, which at() does not let the compiler see.
__global__ __launch_bounds__(256) void blk_mc_code_kernel(BlkView v, uint8_t *__restrict__ codes)
{
    const int64_t vlin = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (vlin >= v.size()) return;
    const BlkView::Cell c = v.split(vlin);
    unsigned code = 0u;
    bool active = true;
#pragma unroll
    for (int dx = 0; dx < 2; ++dx)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dz = 0; dz < 2; ++dz) {
                int64_t virt;
                const int64_t at = v.at(c, dx, dy, dz, &virt);
                if (at < 0) { active = false; continue; }
                const float2 q = v.vol[at];
                active = active && q.y != 0.0f;
                if (q.x < 0.0f) code |= 1u << mc_corner(dx, dy, dz);
            }
    codes[vlin] = (uint8_t)(active ? code : 0u);
}

struct BlkMcFillArgs {
    double vl, ul;
    float *overt, *ocol;
    int32_t *otri;
    int64_t nv, nt;
};

// marching cubes, sweep 3, the blocks' own form like the uniform volume's (kpx_tsdfmesh.hip): vertices and colours by rank,
// triangles by the scanned triangle offsets
__global__ __launch_bounds__(kExtractWaves * 64) void blk_mc_fill_kernel(BlkView v, const uint8_t *__restrict__ codes, int64_t nvox, int64_t nchunks,
                                                                         const McGroup *__restrict__ groups, const int64_t *__restrict__ voff,
                                                                         const int64_t *__restrict__ toff, BlkMcFillArgs a)
{
    const int64_t chunk = (int64_t)blockIdx.x * kExtractWaves + wave_id();
    if (chunk >= nchunks) return;
    const int lane = lane_id();
    const unsigned long long below = (1ull << lane) - 1ull;
    const int64_t vbase = voff[chunk], tbase = toff[chunk];
    if (voff[chunk + 1] == vbase && toff[chunk + 1] == tbase) return;
    for (int r = 0; r < kChunkRounds; ++r) {
        const int64_t g = chunk * kChunkRounds + r, vlin = g * 64 + lane;
        if (g * 64 >= nvox) break;
        const McGroup G = groups[g];
        BlkView::Cell c{};
        if (vlin < nvox) c = v.split(vlin);
        // the vertices of this voxel's three edges
        const unsigned mine = vlin < nvox ? (unsigned)((G.m[0] >> lane) & 1ull) | (unsigned)((G.m[1] >> lane) & 1ull) << 1 | (unsigned)((G.m[2] >> lane) & 1ull) << 2 : 0u;
        if (mine) {
            int64_t dst = vbase + G.vrel + __builtin_popcountll(G.m[0] & below) + __builtin_popcountll(G.m[1] & below) + __builtin_popcountll(G.m[2] & below);
            int b[3];
            blk_unpack(v.keys[c.rank], b);
            const int64_t self = v.self(c);
            const double f0 = fabs((double)v.vol[self].x);
            double p0[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) p0[k] = (double)b[k] * a.ul + ((double)c.p[k] + 0.5) * a.vl;
            for (int i = 0; i < 3; ++i) {
                if (!((mine >> i) & 1u)) continue;
                int64_t virt;
                const int64_t at = v.at(c, i == 0, i == 1, i == 2, &virt);
                if (dst >= a.nv || at < 0) break;                      // never true for the ws the count pass left
                const double f1 = fabs((double)v.vol[at].x);
                double p[3] = { p0[0], p0[1], p0[2] };
                p[i] = p[i] + (f0 * a.vl) / (f0 + f1);
#pragma unroll
                for (int k = 0; k < 3; ++k) a.overt[3 * dst + k] = (float)p[k];
                if (a.ocol) {
                    const float *c0 = v.col + 3 * self, *c1 = v.col + 3 * at;
#pragma unroll
                    for (int k = 0; k < 3; ++k) a.ocol[3 * dst + k] = (float)((f1 * ((double)c0[k] / 255.0) + f0 * ((double)c1[k] / 255.0)) / (f0 + f1));
                }
                ++dst;
            }
        }
        // the triangles of the cube at this voxel
        const unsigned code = vlin < nvox ? codes[vlin] : 0u;
        const int nt = c_mc.ntri[code];
        const int incl = wave_incl_scan(nt);
        int64_t tdst = tbase + G.trel + (incl - nt);
        for (int t = 0; t < nt; ++t, ++tdst) {
            if (tdst >= a.nt) break;
            int32_t idx[3] = { 0, 0, 0 };
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int e = c_mc.tri[code][3 * t + k];
                const signed char *s = c_mc.shift[e];
                int64_t virt = 0;
                if (v.at(c, s[0], s[1], s[2], &virt) >= 0) idx[k] = (int32_t)mc_rank(groups, voff, virt, s[3]);
            }
            a.otri[3 * tdst] = idx[0];
            a.otri[3 * tdst + 1] = idx[2];
            a.otri[3 * tdst + 2] = idx[1];
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
inline bool blk_res_ok(int32_t r) { return r >= 1 && r <= KPX_TSDF_BLOCKS_MAX_RESOLUTION; }
inline int64_t blk_r3(int32_t r) { return (int64_t)r * r * r; }

struct ExtractScratch {
    int32_t *nbr;
    int64_t *offsets;
    uint8_t *codes;             // mesh only
    McGroup *groups;
    int64_t *voff, *toff;
    int64_t nvox, nchunks;
};
void extract_carve(Arena &a, int64_t nblocks, int32_t r, bool mesh, ExtractScratch *s)
{
    s->nvox = nblocks * blk_r3(r);
    s->nchunks = cdiv(s->nvox, kChunk);
    s->nbr = a.get<int32_t>((size_t)(nblocks > 0 ? nblocks : 1) * 27);
    s->offsets = nullptr; s->codes = nullptr; s->groups = nullptr; s->voff = nullptr; s->toff = nullptr;
    if (!mesh) {
        s->offsets = a.get<int64_t>((size_t)s->nchunks + 1);
        return;
    }
    s->codes = a.get<uint8_t>((size_t)(s->nvox > 0 ? s->nvox : 1));
    s->groups = a.get<McGroup>((size_t)(s->nchunks > 0 ? s->nchunks : 1) * kChunkRounds);
    s->voff = a.get<int64_t>((size_t)s->nchunks + 1);
    s->toff = a.get<int64_t>((size_t)s->nchunks + 1);
}
inline BlkView blk_view(const int64_t *keys, const int32_t *slots, int64_t nblocks, const float *pool, const float *cpool, int32_t r, double vl,
                        const int32_t *nbr)
{
    BlkView v;
    v.keys = reinterpret_cast<const uint64_t *>(keys); v.slots = slots; v.nbr = nbr;
    v.vol = reinterpret_cast<const float2 *>(pool); v.col = cpool;
    v.vl = vl; v.ul = vl * (double)r;
    v.B = (int32_t)nblocks; v.R = r; v.R3 = (int32_t)blk_r3(r);
    return v;
}
constexpr int64_t kBlkMaxBlocks = 1 << 22;          // 2^37 voxels at R = 32: every grid and 27 B stay below 2^31

}  // namespace
}  // namespace kpx

using namespace kpx;

KPX_EXPORT size_t kpx_tsdf_blocks_touch_workspace_bytes(int32_t count, int32_t width, int32_t height, int32_t stride, double unit_length, double sdf_trunc)
{
    const TouchShape sh = { count, width, height, stride, unit_length, sdf_trunc };
    if (!touch_shape_ok(sh)) return 0;
    Arena a(nullptr, 0);
    TouchScratch t;
    touch_carve(a, sh, &t);
    return a.off;
}

KPX_EXPORT int kpx_tsdf_blocks_touch(const int64_t *index_keys, const int32_t *index_slots, int64_t n_blocks, int32_t count, const void *const *h_depth,
                                     int32_t depth_u16, double depth_scale, double depth_trunc, int32_t width, int32_t height, const double *h_intrinsic,
                                     const double *h_poses, int32_t stride, double unit_length, double sdf_trunc, int64_t *d_counts, void *ws,
                                     size_t ws_bytes, void *stream)
{
    const TouchShape sh = { count, width, height, stride, unit_length, sdf_trunc };
    KPX_REQUIRE(touch_shape_ok(sh), "kpx_tsdf_blocks_touch: 1 to %d images of a positive size, stride >= 1, 0 < sdf_trunc <= unit_length", KPX_TSDF_MAX_SENSORS);
    KPX_REQUIRE(n_blocks >= 0 && n_blocks <= kBlkMaxBlocks, "kpx_tsdf_blocks_touch: bad block count");
    KPX_REQUIRE(h_depth && h_intrinsic && h_poses && d_counts && ws && (n_blocks == 0 || (index_keys && index_slots)), "kpx_tsdf_blocks_touch: null pointer");
    KPX_REQUIRE(!depth_u16 || depth_scale > 0.0, "kpx_tsdf_blocks_touch: depth_scale must be positive");
    for (int32_t i = 0; i < count; ++i) KPX_REQUIRE(h_depth[i], "kpx_tsdf_blocks_touch: image %d is null", i);
    Arena ar(ws, ws_bytes);
    TouchScratch t;
    touch_carve(ar, sh, &t);
    KPX_ARENA_CHECK(ar);
    TouchArgs a;
    memset(&a, 0, sizeof a);
    for (int32_t i = 0; i < count; ++i) {
        memcpy(a.P[i], h_poses + 16 * (size_t)i, sizeof a.P[i]);
        a.depth[i] = h_depth[i];
    }
    a.fx = h_intrinsic[0]; a.fy = h_intrinsic[1]; a.cx = h_intrinsic[2]; a.cy = h_intrinsic[3];
    a.ul = unit_length; a.trunc = sdf_trunc;
    a.scale = (float)depth_scale; a.dtrunc = (float)depth_trunc;
    a.W = width; a.H = height; a.stride = stride; a.nw = t.nw; a.nh = t.nh; a.count = count; a.nax = t.nax; a.u16 = depth_u16;
    hipStream_t st = (hipStream_t)stream;
    KPX_HIP(hipMemsetAsync(t.err, 0, sizeof(int32_t), st));
    KPX_HIP(hipMemsetAsync(t.tmask, 0, sizeof(uint32_t) * (size_t)t.n, st));
    hipLaunchKernelGGL(blk_emit_kernel, dim3((unsigned)cdiv(t.np, 256)), dim3(256), 0, st, a, t.np, t.sort.keys_in, t.sort.vals_in, t.err);
    KPX_LAUNCH_CHECK();
    const int rc = dsort_run(t.sort, t.n, 64, st);
    if (rc != KPX_OK) return rc;
    const uint64_t *index = reinterpret_cast<const uint64_t *>(index_keys);
    const unsigned grid = (unsigned)cdiv(t.nchunks, kExtractWaves);
    hipLaunchKernelGGL(blk_heads_count_kernel, dim3(grid), dim3(kExtractWaves * 64), 0, st, (const uint64_t *)t.sort.keys_out, t.n, t.nchunks, index,
                       (int32_t)n_blocks, t.hoff, t.noff);
    scan2_i64(t.hoff, t.noff, t.nchunks, st);
    hipLaunchKernelGGL(blk_heads_fill_kernel, dim3(grid), dim3(kExtractWaves * 64), 0, st, (const uint64_t *)t.sort.keys_out, (const int32_t *)t.sort.vals_out, t.n,
                       t.nchunks, index, index_slots, (int32_t)n_blocks, (const int64_t *)t.hoff, (const int64_t *)t.noff, t.ukeys, t.tslot, t.tmask, t.newkeys);
    hipLaunchKernelGGL(blk_touch_done_kernel, dim3(1), dim3(64), 0, st, (const int64_t *)t.hoff, (const int64_t *)t.noff, t.nchunks, (const int32_t *)t.err, d_counts);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT int kpx_tsdf_blocks_insert(const int64_t *index_keys, const int32_t *index_slots, int64_t n_blocks, int64_t n_new, int64_t *out_keys,
                                      int32_t *out_slots, float *pool, float *color_pool, int64_t capacity, int32_t unit_resolution, int32_t count,
                                      int32_t width, int32_t height, int32_t stride, double unit_length, double sdf_trunc, const void *ws, size_t ws_bytes,
                                      void *stream)
{
    const TouchShape sh = { count, width, height, stride, unit_length, sdf_trunc };
    KPX_REQUIRE(touch_shape_ok(sh), "kpx_tsdf_blocks_insert: not the shape of a touch workspace");
    KPX_REQUIRE(blk_res_ok(unit_resolution), "kpx_tsdf_blocks_insert: unit resolution must be in [1, %d]", KPX_TSDF_BLOCKS_MAX_RESOLUTION);
    KPX_REQUIRE(n_blocks >= 0 && n_new >= 0 && n_blocks + n_new <= kBlkMaxBlocks, "kpx_tsdf_blocks_insert: bad block counts");
    KPX_REQUIRE(n_blocks + n_new <= capacity, "kpx_tsdf_blocks_insert: %lld blocks in a pool of %lld", (long long)(n_blocks + n_new), (long long)capacity);
    if (n_blocks + n_new == 0) return KPX_OK;
    KPX_REQUIRE(out_keys && out_slots && pool && ws && (n_blocks == 0 || (index_keys && index_slots)), "kpx_tsdf_blocks_insert: null pointer");
    Arena ar(const_cast<void *>(ws), ws_bytes);
    TouchScratch t;
    touch_carve(ar, sh, &t);
    KPX_ARENA_CHECK(ar);
    KPX_REQUIRE(n_new <= t.n, "kpx_tsdf_blocks_insert: more new blocks than the touch can have left");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(blk_merge_kernel, dim3((unsigned)cdiv(n_blocks + n_new, 256)), dim3(256), 0, st, reinterpret_cast<const uint64_t *>(index_keys), index_slots,
                       (int32_t)n_blocks, (const uint64_t *)t.newkeys, (int32_t)n_new, reinterpret_cast<uint64_t *>(out_keys), out_slots);
    KPX_LAUNCH_CHECK();
    const size_t r3 = (size_t)blk_r3(unit_resolution);
    if (n_new > 0) {
        KPX_HIP(hipMemsetAsync(pool + 2 * r3 * (size_t)n_blocks, 0, sizeof(float) * 2 * r3 * (size_t)n_new, st));
        if (color_pool) KPX_HIP(hipMemsetAsync(color_pool + 3 * r3 * (size_t)n_blocks, 0, sizeof(float) * 3 * r3 * (size_t)n_new, st));
    }
    return KPX_OK;
}

KPX_EXPORT int kpx_tsdf_blocks_integrate(float *pool, float *color_pool, int64_t capacity, int32_t unit_resolution, double voxel_length, double sdf_trunc,
                                         int64_t n_touched, int32_t count, const void *const *h_depth, int32_t depth_u16, double depth_scale,
                                         double depth_trunc, const uint8_t *const *h_rgb, int32_t width, int32_t height, const double *h_intrinsic,
                                         const double *h_extrinsics, int32_t stride, const void *ws, size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(blk_res_ok(unit_resolution), "kpx_tsdf_blocks_integrate: unit resolution must be in [1, %d]", KPX_TSDF_BLOCKS_MAX_RESOLUTION);
    KPX_REQUIRE(voxel_length > 0.0, "kpx_tsdf_blocks_integrate: voxel_length must be positive");
    const double ul = voxel_length * (double)unit_resolution;
    const TouchShape sh = { count, width, height, stride, ul, sdf_trunc };
    KPX_REQUIRE(touch_shape_ok(sh), "kpx_tsdf_blocks_integrate: not the shape of a touch workspace");
    KPX_REQUIRE(n_touched >= 0 && n_touched <= kBlkMaxBlocks && capacity >= 0, "kpx_tsdf_blocks_integrate: bad block counts");
    if (n_touched == 0) return KPX_OK;
    KPX_REQUIRE(pool && ws && h_depth && h_intrinsic && h_extrinsics, "kpx_tsdf_blocks_integrate: null pointer");
    KPX_REQUIRE(!color_pool || h_rgb, "kpx_tsdf_blocks_integrate: a colour volume needs colour images");
    KPX_REQUIRE(((uintptr_t)pool % 16) == 0 && ((uintptr_t)color_pool % 8) == 0, "kpx_tsdf_blocks_integrate: the pool must be 16-byte aligned");
    KPX_REQUIRE(!depth_u16 || depth_scale > 0.0, "kpx_tsdf_blocks_integrate: depth_scale must be positive");
    for (int32_t i = 0; i < count; ++i) KPX_REQUIRE(h_depth[i] && (!color_pool || h_rgb[i]), "kpx_tsdf_blocks_integrate: image %d is null", i);
    Arena ar(const_cast<void *>(ws), ws_bytes);
    TouchScratch t;
    touch_carve(ar, sh, &t);
    KPX_ARENA_CHECK(ar);
    KPX_REQUIRE(n_touched <= t.n, "kpx_tsdf_blocks_integrate: more touched blocks than the touch can have left");
    TsdfIntegrateArgs a;
    memset(&a, 0, sizeof a);
    a.count = count;
    for (int32_t i = 0; i < count; ++i) {
        memcpy(a.s[i].E, h_extrinsics + 16 * (size_t)i, sizeof a.s[i].E);
        a.s[i].depth = h_depth[i];
        a.s[i].rgb = color_pool ? h_rgb[i] : nullptr;
    }
    a.vl = voxel_length; a.trunc = sdf_trunc;
    a.fx = h_intrinsic[0]; a.fy = h_intrinsic[1]; a.cx = h_intrinsic[2]; a.cy = h_intrinsic[3];
    a.scale = (float)depth_scale; a.dtrunc = (float)depth_trunc;
    a.W = width; a.H = height; a.res = unit_resolution;
    float2 *vol = reinterpret_cast<float2 *>(pool);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)n_touched), block(256);
    const uint64_t *uk = t.ukeys;
    const int32_t *ts = t.tslot;
    const uint32_t *tm = t.tmask;
    if (depth_u16) {
        if (color_pool) hipLaunchKernelGGL((blk_integrate_kernel<true, true>), grid, block, 0, st, vol, color_pool, uk, ts, tm, ul, a);
        else hipLaunchKernelGGL((blk_integrate_kernel<true, false>), grid, block, 0, st, vol, color_pool, uk, ts, tm, ul, a);
    } else {
        if (color_pool) hipLaunchKernelGGL((blk_integrate_kernel<false, true>), grid, block, 0, st, vol, color_pool, uk, ts, tm, ul, a);
        else hipLaunchKernelGGL((blk_integrate_kernel<false, false>), grid, block, 0, st, vol, color_pool, uk, ts, tm, ul, a);
    }
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT size_t kpx_tsdf_blocks_extract_workspace_bytes(int64_t n_blocks, int32_t unit_resolution, int32_t mesh)
{
    if (!blk_res_ok(unit_resolution) || n_blocks < 0 || n_blocks > kBlkMaxBlocks) return 0;
    Arena a(nullptr, 0);
    ExtractScratch s;
    extract_carve(a, n_blocks, unit_resolution, mesh != 0, &s);
    return a.off;
}

#define KPX_BLK_COMMON(who)                                                                                                                             \
    KPX_REQUIRE(blk_res_ok(unit_resolution), who ": unit resolution must be in [1, %d]", KPX_TSDF_BLOCKS_MAX_RESOLUTION);                               \
    KPX_REQUIRE(n_blocks >= 0 && n_blocks <= kBlkMaxBlocks, who ": bad block count")

KPX_EXPORT int kpx_tsdf_blocks_extract_count(const int64_t *index_keys, const int32_t *index_slots, int64_t n_blocks, const float *pool,
                                             int32_t unit_resolution, int32_t mode, int64_t *d_count, void *ws, size_t ws_bytes, void *stream)
{
    KPX_BLK_COMMON("kpx_tsdf_blocks_extract_count");
    KPX_REQUIRE(mode == KPX_TSDF_SURFACE || mode == KPX_TSDF_VOXELS, "kpx_tsdf_blocks_extract_count: unknown mode %d", mode);
    KPX_REQUIRE(d_count && ws && (n_blocks == 0 || (index_keys && index_slots && pool)), "kpx_tsdf_blocks_extract_count: null pointer");
    Arena a(ws, ws_bytes);
    ExtractScratch s;
    extract_carve(a, n_blocks, unit_resolution, false, &s);
    KPX_ARENA_CHECK(a);
    hipStream_t st = (hipStream_t)stream;
    if (n_blocks == 0) {
        KPX_HIP(hipMemsetAsync(d_count, 0, sizeof(int64_t), st));
        return KPX_OK;
    }
    const BlkView v = blk_view(index_keys, index_slots, n_blocks, pool, nullptr, unit_resolution, 0.0, s.nbr);
    hipLaunchKernelGGL(blk_neighbours_kernel, dim3((unsigned)cdiv(n_blocks * 27, 256)), dim3(256), 0, st, v.keys, v.B, s.nbr);
    hipLaunchKernelGGL(tsdf_count_kernel<BlkView>, dim3((unsigned)cdiv(s.nchunks, kExtractWaves)), dim3(kExtractWaves * 64), 0, st, v, mode, s.nchunks, s.offsets);
    scan_i64(s.offsets, s.nchunks, st);
    KPX_LAUNCH_CHECK();
    KPX_HIP(hipMemcpyAsync(d_count, s.offsets + s.nchunks, sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    return KPX_OK;
}

KPX_EXPORT int kpx_tsdf_blocks_extract_fill(const int64_t *index_keys, const int32_t *index_slots, int64_t n_blocks, const float *pool,
                                            const float *color_pool, int32_t unit_resolution, double voxel_length, int32_t mode, int64_t total, float *pts,
                                            float *nrm, float *col, void *ws, size_t ws_bytes, void *stream)
{
    KPX_BLK_COMMON("kpx_tsdf_blocks_extract_fill");
    KPX_REQUIRE(mode == KPX_TSDF_SURFACE || mode == KPX_TSDF_VOXELS, "kpx_tsdf_blocks_extract_fill: unknown mode %d", mode);
    KPX_REQUIRE(voxel_length > 0.0 && total >= 0, "kpx_tsdf_blocks_extract_fill: bad voxel_length or total");
    if (total == 0 || n_blocks == 0) return KPX_OK;
    KPX_REQUIRE(index_keys && index_slots && pool && pts && ws, "kpx_tsdf_blocks_extract_fill: null pointer");
    Arena a(ws, ws_bytes);
    ExtractScratch s;
    extract_carve(a, n_blocks, unit_resolution, false, &s);
    KPX_ARENA_CHECK(a);
    const BlkView v = blk_view(index_keys, index_slots, n_blocks, pool, color_pool, unit_resolution, voxel_length, s.nbr);
    const TsdfFillArgs f = { pts, mode == KPX_TSDF_SURFACE ? nrm : nullptr, col, total };
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tsdf_fill_kernel<BlkView>, dim3((unsigned)cdiv(s.nchunks, kExtractWaves)), dim3(kExtractWaves * 64), 0, st, v, mode, s.nchunks,
                       (const int64_t *)s.offsets, f);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}

KPX_EXPORT int kpx_tsdf_blocks_mesh_count(const int64_t *index_keys, const int32_t *index_slots, int64_t n_blocks, const float *pool,
                                          int32_t unit_resolution, int64_t *d_counts, void *ws, size_t ws_bytes, void *stream)
{
    KPX_BLK_COMMON("kpx_tsdf_blocks_mesh_count");
    KPX_REQUIRE(d_counts && ws && (n_blocks == 0 || (index_keys && index_slots && pool)), "kpx_tsdf_blocks_mesh_count: null pointer");
    Arena a(ws, ws_bytes);
    ExtractScratch s;
    extract_carve(a, n_blocks, unit_resolution, true, &s);
    KPX_ARENA_CHECK(a);
    hipStream_t st = (hipStream_t)stream;
    if (n_blocks == 0) {
        KPX_HIP(hipMemsetAsync(d_counts, 0, 2 * sizeof(int64_t), st));
        return KPX_OK;
    }
    const BlkView v = blk_view(index_keys, index_slots, n_blocks, pool, nullptr, unit_resolution, 0.0, s.nbr);
    hipLaunchKernelGGL(blk_neighbours_kernel, dim3((unsigned)cdiv(n_blocks * 27, 256)), dim3(256), 0, st, v.keys, v.B, s.nbr);
    hipLaunchKernelGGL(blk_mc_code_kernel, dim3((unsigned)cdiv(s.nvox, 256)), dim3(256), 0, st, v, s.codes);
    hipLaunchKernelGGL(mc_count_kernel<BlkView>, dim3((unsigned)cdiv(s.nchunks, kExtractWaves)), dim3(kExtractWaves * 64), 0, st, v, (const uint8_t *)s.codes, s.nchunks,
                       s.groups, s.voff, s.toff);
    scan2_i64(s.voff, s.toff, s.nchunks, st);
    KPX_LAUNCH_CHECK();
    KPX_HIP(hipMemcpyAsync(d_counts, s.voff + s.nchunks, sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    KPX_HIP(hipMemcpyAsync(d_counts + 1, s.toff + s.nchunks, sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    return KPX_OK;
}

KPX_EXPORT int kpx_tsdf_blocks_mesh_fill(const int64_t *index_keys, const int32_t *index_slots, int64_t n_blocks, const float *pool,
                                         const float *color_pool, int32_t unit_resolution, double voxel_length, int64_t n_vertices, int64_t n_triangles,
                                         float *out_vertices, float *out_colors, int32_t *out_triangles, void *ws, size_t ws_bytes, void *stream)
{
    KPX_BLK_COMMON("kpx_tsdf_blocks_mesh_fill");
    KPX_REQUIRE(voxel_length > 0.0 && n_vertices >= 0 && n_triangles >= 0, "kpx_tsdf_blocks_mesh_fill: bad voxel_length or counts");
    if (n_vertices > kMeshMax || n_triangles > kMeshMax)
        return fail(KPX_ERR_RANGE, "kpx_tsdf_blocks_mesh_fill: %lld vertices and %lld triangles: a mesh holds fewer than 2^31 of each", (long long)n_vertices,
                    (long long)n_triangles);
    if ((n_vertices == 0 && n_triangles == 0) || n_blocks == 0) return KPX_OK;
    KPX_REQUIRE(index_keys && index_slots && pool && ws && (n_vertices == 0 || out_vertices) && (n_triangles == 0 || out_triangles),
                "kpx_tsdf_blocks_mesh_fill: null pointer");
    KPX_REQUIRE(!out_colors || color_pool, "kpx_tsdf_blocks_mesh_fill: colours need a colour volume");
    Arena a(ws, ws_bytes);
    ExtractScratch s;
    extract_carve(a, n_blocks, unit_resolution, true, &s);
    KPX_ARENA_CHECK(a);
    const BlkView v = blk_view(index_keys, index_slots, n_blocks, pool, color_pool, unit_resolution, voxel_length, s.nbr);
    const BlkMcFillArgs f = { v.vl, v.ul, out_vertices, out_colors, out_triangles, n_vertices, n_triangles };
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(blk_mc_fill_kernel, dim3((unsigned)cdiv(s.nchunks, kExtractWaves)), dim3(kExtractWaves * 64), 0, st, v, (const uint8_t *)s.codes, s.nvox, s.nchunks,
                       (const McGroup *)s.groups, (const int64_t *)s.voff, (const int64_t *)s.toff, f);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}
