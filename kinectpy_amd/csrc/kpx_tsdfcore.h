// kpx_tsdfcore.h -- what the uniform volume (kpx_tsdf.hip) and the block volume (kpx_tsdfblocks.hip) share of AC9: the sensor and
// argument records of an integration launch, the update of one voxel centre by one image, and the validity test of the extractions.
#pragma once
#include "kpx_common.h"

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

}  // namespace kpx
