// kpx_tsdfcore.h -- AC9 and AC16 once, for the uniform volume (kpx_tsdf.hip) and the block volume (kpx_tsdfblocks.hip): the sensor and
// argument records of an integration launch, the update of one voxel centre by one image, and the point-cloud extractions (count per
// chunk of consecutive voxels -> 64-bit scan -> fill) as kernels over a volume view.  (The two integration kernels keep their own
// running-mean loops: as one inlined function the compiler takes the uniform kernel's 16-byte access apart)
//
// A volume view is a small struct passed by value that says where voxels are; the kernels hold the arithmetic.  A view V has
//   vol, col                     the storage: float2 {tsdf, weight} and float[3] per voxel, indexed by what at() returns
//   size()                       how many (virtual) voxels the sweeps cover; they are numbered 0 .. size() - 1
//   Cell, split(lin)             a voxel of the sweep: its block's rank and its (x, y, z) in the block.  Only for 0 <= lin < size():
//                                a view may tell the compiler so, and any other lin is then undefined, not merely a wrong cell
//   self(c)                      its storage index
//   at(c, dx, dy, dz, &virt)     the storage index of the voxel at an offset from c (any coordinate may leave the block), -1 when
//                                there is none; *virt = its number in the sweep
//   surface_neighbour(c, i)      whether the voxel one step along axis i may close a zero crossing
//   anchor(c)                    readies c for the three below (a block loads its index here, once)
//   centre(c, k)                 coordinate k of the voxel's centre, in the frame the interpolation works in
//   world(p, k)                  coordinate k of an output position, from that frame
//   tap0(c, fl, k)               floor(q / vl - 0.5) = fl as a coordinate counted from c's block
// UniformView is below; BlkView is kpx_tsdfblocks.hip's.
#pragma once
#include "kpx_compact.h"

#include <math.h>

namespace kpx {

struct TsdfSensor {
    double E[12];              // world -> camera, rows 0..2 of the row-major 4x4
    const void *depth;         // f32 or u16 [H W]
    const uint8_t *rgb;        // u8 [H W 3] or null
};
struct TsdfIntegrateArgs {
    TsdfSensor s[KPX_TSDF_MAX_SENSORS];
    double org[3], vl, trunc, fx, fy, cx, cy;
    float scale, dtrunc;
    int32_t W, H, res, count;
};

// AC9 for one voxel centre and one image: true = the voxel is updated with *t (and rgb[3])
template <bool U16, bool COLOR>
__device__ __forceinline__ bool tsdf_observe(const TsdfIntegrateArgs &a, const TsdfSensor &sn, const double c[3], float *t, float rgb[3])
{
    const double *E = sn.E;
    const double pz = fma(E[8], c[0], fma(E[9], c[1], fma(E[10], c[2], E[11])));
    if (pz <= 0.0) return false;
    const double px = fma(E[0], c[0], fma(E[1], c[1], fma(E[2], c[2], E[3])));
    const double py = fma(E[4], c[0], fma(E[5], c[1], fma(E[6], c[2], E[7])));
    const double ax = px * a.fx, ay = py * a.fy;
    // Division-free reject of what projects more than a pixel outside the image (the exact test below decides the rest): whole
    // waves whose z-run misses every image leave here without a division, a gather or a volume access.
    if (ax < (-a.cx - 1.5) * pz || ax > ((double)a.W - a.cx + 0.5) * pz || ay < (-a.cy - 1.5) * pz || ay > ((double)a.H - a.cy + 0.5) * pz) return false;
    const double uf = ax / pz + a.cx + 0.5, vf = ay / pz + a.cy + 0.5;
    if (!(uf >= 0.0001 && uf < (double)a.W - 0.0001 && vf >= 0.0001 && vf < (double)a.H - 0.0001)) return false;
    const int u = (int)uf, v = (int)vf;
    const int64_t pix = (int64_t)v * a.W + u;
    float d;
    if (U16) {
        d = (float)((const uint16_t *)sn.depth)[pix] / a.scale;
        if (d > a.dtrunc) d = 0.0f;
    } else {
        d = ((const float *)sn.depth)[pix];
    }
    if (d <= 0.0f) return false;
    // sdf = dz mult with mult >= 1 (a correctly rounded sqrt of a value >= 1), and rounding is monotonic: dz <= -trunc gives
    // sdf <= -trunc (no update) and dz >= trunc gives sdf / trunc >= 1 (t = 1) whatever mult is.  Only the band between the two --
    // a few voxels either side of the surface -- pays for the two divisions, the square root and the quotient.
    const double dz = (double)d - pz;
    if (dz <= -a.trunc) return false;
    if (dz >= a.trunc) {
        *t = 1.0f;
    } else {
        const double xm = ((double)u - a.cx) / a.fx, ym = ((double)v - a.cy) / a.fy;
        const double mult = sqrt(xm * xm + ym * ym + 1.0);
        const double sdf = dz * mult;
        if (!(sdf > -a.trunc)) return false;
        *t = (float)fmin(1.0, sdf / a.trunc);
    }
    if (COLOR) {
        const uint8_t *p = sn.rgb + 3 * pix;
        rgb[0] = (float)p[0]; rgb[1] = (float)p[1]; rgb[2] = (float)p[2];
    }
    return true;
}

// a voxel the extractions use: observed, and inside Open3D's band
__device__ __forceinline__ bool tsdf_valid(const float2 v) { return v.y != 0.0f && v.x >= -0.98f && v.x < 0.98f; }

// index l of a cube of r^3 voxels, z fastest, to (x, y, z); l < 2^30, so the divisions are 32-bit
__device__ __forceinline__ void tsdf_split(uint32_t l, uint32_t r, int &x, int &y, int &z)
{
    const uint32_t t = l / r;
    z = (int)(l - t * r);
    x = (int)(t / r);
    y = (int)(t - (uint32_t)x * r);
}

namespace {

constexpr int kChunk = KPX_TSDF_COUNT_BLOCK;       // consecutive voxels (or keys) a wave counts and fills
constexpr int kChunkRounds = kChunk / 64;
constexpr int kExtractWaves = 4;

// ---- the view of the uniform volume ([O3D] UniformTSDFVolume) --------------------------------------------------------------------
// One block of res^3 voxels, rank 0, voxel (x, y, z) at (x res + y) res + z; res <= 1024, so an index is below 2^30: it is carried as
// int64 for the byte offsets of the 8 GiB volume.  Interpolation works in volume coordinates; the origin is added last.
struct UniformView {
    const float2 *vol;
    const float *col;
    double org[3], vl;         // the fills'
    int32_t res;
    struct Cell {
        int64_t lin;
        int p[3];
    };
    __device__ __forceinline__ int64_t size() const { return (int64_t)res * res * res; }
    __device__ __forceinline__ Cell split(int64_t lin) const
    {
        Cell c;
        c.lin = lin;
        tsdf_split((uint32_t)lin, (uint32_t)res, c.p[0], c.p[1], c.p[2]);
        __builtin_assume(c.p[0] >= 0 && c.p[0] < res && c.p[1] >= 0 && c.p[1] < res && c.p[2] >= 0 && c.p[2] < res);      // lin < size(): folds at()'s tests
        return c;
    }
    __device__ __forceinline__ int64_t self(const Cell &c) const { return c.lin; }
    __device__ __forceinline__ int64_t at(const Cell &c, int dx, int dy, int dz, int64_t *virt) const
    {
        const uint32_t r = (uint32_t)res;
        if ((uint32_t)(c.p[0] + dx) >= r || (uint32_t)(c.p[1] + dy) >= r || (uint32_t)(c.p[2] + dz) >= r) return -1;
        return *virt = c.lin + ((int64_t)dx * res + dy) * res + dz;
    }
    // Open3D's bound: the last layer of every axis is never a neighbour
    __device__ __forceinline__ bool surface_neighbour(const Cell &c, int i) const { return c.p[i] + 1 < res - 1; }
    __device__ __forceinline__ void anchor(Cell &) const {}
    __device__ __forceinline__ double centre(const Cell &c, int k) const { return ((double)c.p[k] + 0.5) * vl; }
    __device__ __forceinline__ double world(double p, int k) const { return p + org[k]; }
    __device__ __forceinline__ int tap0(const Cell &, double fl, int) const { return (int)fl; }
};
inline UniformView uniform_view(const float *volume, const float *color, int32_t res, double vl, const double *h_origin)
{
    UniformView v;
    v.vol = reinterpret_cast<const float2 *>(volume); v.col = color; v.res = res; v.vl = vl;
    for (int k = 0; k < 3; ++k) v.org[k] = h_origin ? h_origin[k] : 0.0;
    return v;
}

// ---- point-cloud extraction ------------------------------------------------------------------------------------------------------
// what voxel `lin` emits: KPX_TSDF_SURFACE: bit i = a zero crossing towards +e_i; KPX_TSDF_VOXELS: bit 0 = the voxel is valid.
// *self = its storage index, *v0 = the voxel, nbi[i] / nb[i] = the neighbour of a set bit i.
template <class V>
__device__ __forceinline__ unsigned tsdf_emits(const V &v, int64_t lin, int mode, int64_t *self, float2 *v0, float2 nb[3], int64_t nbi[3])
{
    const typename V::Cell c = v.split(lin);
    *self = v.self(c);
    *v0 = v.vol[*self];
    if (!tsdf_valid(*v0)) return 0u;
    if (mode == KPX_TSDF_VOXELS) return 1u;
    unsigned m = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (!v.surface_neighbour(c, i)) continue;
        int64_t virt;
        nbi[i] = v.at(c, i == 0, i == 1, i == 2, &virt);
        if (nbi[i] < 0) continue;
        nb[i] = v.vol[nbi[i]];
        if (tsdf_valid(nb[i]) && (double)v0->x * (double)nb[i].x < 0.0) m |= 1u << i;
    }
    return m;
}

template <class V>
__global__ __launch_bounds__(kExtractWaves * 64) void tsdf_count_kernel(V v, int mode, int64_t nchunks, int64_t *__restrict__ counts)
{
    const int64_t chunk = (int64_t)blockIdx.x * kExtractWaves + wave_id();
    if (chunk >= nchunks) return;
    const int64_t nvox = v.size();
    int c = 0;
    for (int r = 0; r < kChunkRounds; ++r) {
        const int64_t lin = chunk * kChunk + r * 64 + lane_id();
        int64_t self, nbi[3];
        float2 v0, nb[3];
        if (lin < nvox) c += __builtin_popcount(tsdf_emits(v, lin, mode, &self, &v0, nb, nbi));
    }
    c = wave_sum(c);
    if (lane_id() == 0) counts[chunk] = c;
}

// trilinear interpolation of the stored tsdf at q (in the view's frame); taps counted from c's block, a tap that is not there is 0
template <class V>
__device__ __forceinline__ double tsdf_tap(const V &v, const typename V::Cell &c, const double q[3])
{
    double r[3];
    int d0[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double g = q[a] / v.vl - 0.5, fl = floor(g);
        r[a] = g - fl;
        d0[a] = v.tap0(c, fl, a) - c.p[a];
    }
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int dx = t >> 2, dy = (t >> 1) & 1, dz = t & 1;
        const double wx = dx ? r[0] : 1.0 - r[0], wy = dy ? r[1] : 1.0 - r[1], wz = dz ? r[2] : 1.0 - r[2];
        int64_t virt;
        const int64_t at = v.at(c, d0[0] + dx, d0[1] + dy, d0[2] + dz, &virt);
        const float fv = at >= 0 ? v.vol[at].x : 0.0f;
        acc = acc + wx * wy * wz * (double)fv;
    }
    return acc;
}

struct TsdfFillArgs {
    float *pts, *nrm, *ocol;
    int64_t total;
};

template <class V>
__global__ __launch_bounds__(kExtractWaves * 64) void tsdf_fill_kernel(V v, int mode, int64_t nchunks, const int64_t *__restrict__ offsets, TsdfFillArgs a)
{
    const int64_t chunk = (int64_t)blockIdx.x * kExtractWaves + wave_id();
    if (chunk >= nchunks) return;
    const int64_t nvox = v.size();
    const int lane = lane_id();
    const unsigned long long below = (1ull << lane) - 1ull;
    int64_t pos = offsets[chunk];
    if (offsets[chunk + 1] == pos) return;
    for (int r = 0; r < kChunkRounds; ++r) {
        const int64_t lin = chunk * kChunk + r * 64 + lane;
        int64_t self = 0, nbi[3] = { -1, -1, -1 };
        float2 v0, nb[3];
        const unsigned m = lin < nvox ? tsdf_emits(v, lin, mode, &self, &v0, nb, nbi) : 0u;
        const unsigned long long b0 = __ballot((m & 1u) != 0), b1 = __ballot((m & 2u) != 0), b2 = __ballot((m & 4u) != 0);
        if ((b0 | b1 | b2) == 0ull) continue;
        int64_t dst = pos + __builtin_popcountll(b0 & below) + __builtin_popcountll(b1 & below) + __builtin_popcountll(b2 & below);
        pos += __builtin_popcountll(b0) + __builtin_popcountll(b1) + __builtin_popcountll(b2);
        if (m == 0u) continue;
        typename V::Cell c = v.split(lin);
        v.anchor(c);
        const double p0[3] = { v.centre(c, 0), v.centre(c, 1), v.centre(c, 2) };
        if (mode == KPX_TSDF_VOXELS) {
            if (dst >= a.total) continue;
#pragma unroll
            for (int k = 0; k < 3; ++k) a.pts[3 * dst + k] = (float)v.world(p0[k], k);
            if (a.ocol) {
                const float g = (float)(((double)v0.x + 1.0) * 0.5);
                a.ocol[3 * dst] = g; a.ocol[3 * dst + 1] = g; a.ocol[3 * dst + 2] = g;
            }
            continue;
        }
        for (int i = 0; i < 3; ++i) {
            if (!((m >> i) & 1u)) continue;
            if (dst >= a.total) break;
            const double r0 = fabs((double)v0.x), r1 = fabs((double)nb[i].x);
            double p[3] = { p0[0], p0[1], p0[2] };
            p[i] = (p0[i] * r1 + (p0[i] + v.vl) * r0) / (r0 + r1);
#pragma unroll
            for (int k = 0; k < 3; ++k) a.pts[3 * dst + k] = (float)v.world(p[k], k);
            if (a.ocol && v.col) {
                const float *c0 = v.col + 3 * self, *c1 = v.col + 3 * nbi[i];
#pragma unroll
                for (int k = 0; k < 3; ++k) a.ocol[3 * dst + k] = (float)(((double)c0[k] * r1 + (double)c1[k] * r0) / (r0 + r1) / 255.0);
            }
            if (a.nrm) {
                const double gap = 0.99 * v.vl;
                double n[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    double qp[3] = { p[0], p[1], p[2] }, qm[3] = { p[0], p[1], p[2] };
                    qp[k] = p[k] + gap;
                    qm[k] = p[k] - gap;
                    n[k] = tsdf_tap(v, c, qp) - tsdf_tap(v, c, qm);
                }
                const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
#pragma unroll
                for (int k = 0; k < 3; ++k) a.nrm[3 * dst + k] = len == 0.0 ? 0.0f : (float)(n[k] / len);
            }
            ++dst;
        }
    }
}

}  // namespace
}  // namespace kpx
