// kpx_pointnet.h -- what the inference (kpx_pointnet.hip, AC18) and the training step (kpx_pointnet_train.hip, AC19) of the PointNet joint
// regressor share: the 20 layers' widths, the packed inference layout and the host-side argument check.
#pragma once
#include "kpx_common.h"

namespace kpx {

constexpr int kPnLayers = 20;
constexpr int kPnFeat = 512;                 // width of every trunk's last layer
constexpr int kPnChunks = kPnFeat / 32;      // 32-channel chunks of that layer (one 32x32 accumulator tile each)
constexpr int kPnPad = 64;                   // every array of a packed buffer starts at a multiple of 64 floats

static const int kPnCin[kPnLayers] = { 3, 32, 64, 512, 256, 128, 3, 32, 32, 32, 64, 512, 256, 128, 32, 32, 64, 512, 256, 128 };
static const int kPnCout[kPnLayers] = { 32, 64, 512, 256, 128, 9, 32, 32, 32, 64, 512, 256, 128, 1024, 32, 64, 512, 256, 128, 0 /* 3 J */ };

static inline int64_t pn_cout(int l, int joints) { return l == kPnLayers - 1 ? 3 * (int64_t)joints : kPnCout[l]; }
static inline int64_t pn_padded(int64_t v) { return cdiv(v, kPnPad) * kPnPad; }

struct PnLayout {
    int64_t w[kPnLayers], b[kPnLayers], total;
};
static PnLayout pn_layout(int joints)
{
    PnLayout L;
    int64_t off = 0;
    for (int l = 0; l < kPnLayers; ++l) {
        const int64_t co = pn_cout(l, joints);
        L.w[l] = off;
        off += pn_padded((int64_t)kPnCin[l] * co);
        L.b[l] = off;
        off += pn_padded(co);
    }
    L.total = off;
    return L;
}

typedef float pn_f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float pn_relu(float v) { return v > 0.0f ? v : 0.0f; }

static int pn_size_check(const char *who, int32_t batch, int64_t n, int32_t joints)
{
    KPX_REQUIRE(joints >= 1 && 3 * (int64_t)joints <= KPX_POINTNET_MAX_OUT, "%s: joints = %d: need 1 <= joints and 3 joints <= %d", who, (int)joints,
                KPX_POINTNET_MAX_OUT);
    KPX_REQUIRE(batch >= 0, "%s: negative batch", who);
    KPX_REQUIRE(n >= 1, "%s: a cloud needs at least one point (n = %lld)", who, (long long)n);
    if ((int64_t)batch * n >= ((int64_t)1 << 31) || n >= ((int64_t)1 << 31))
        return fail(KPX_ERR_RANGE, "%s: batch x n = %lld x %lld reaches 2^31 points", who, (long long)batch, (long long)n);
    return KPX_OK;
}

}  // namespace kpx
