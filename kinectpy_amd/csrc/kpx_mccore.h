// kpx_mccore.h -- what the two marching-cubes extractions (kpx_tsdfmesh.hip over the uniform volume, kpx_tsdfblocks.hip over the
// block volume) share of AC12: the case table with its triangle counts and edge shifts in constant memory, and the corner numbering.
#pragma once
#include "kpx_common.h"
#include "kpx_mctables.h"

namespace kpx {
namespace {

struct McTables {
    signed char tri[256][16];
    unsigned char ntri[256];
    signed char shift[12][4];       // edge -> (dx, dy, dz, axis) of its lower voxel
};
constexpr McTables mc_make_tables()
{
    McTables t{};
    for (int c = 0; c < 256; ++c) {
        int n = 0;
        for (int i = 0; i < 16; ++i) {
            t.tri[c][i] = kMcTriTable[c][i];
            if (kMcTriTable[c][i] >= 0 && n == i) ++n;
        }
        t.ntri[c] = (unsigned char)(n / 3);
    }
    constexpr signed char sh[12][4] = { { 0, 0, 0, 0 }, { 1, 0, 0, 1 }, { 0, 1, 0, 0 }, { 0, 0, 0, 1 }, { 0, 0, 1, 0 }, { 1, 0, 1, 1 },
                                        { 0, 1, 1, 0 }, { 0, 0, 1, 1 }, { 0, 0, 0, 2 }, { 1, 0, 0, 2 }, { 1, 1, 0, 2 }, { 0, 1, 0, 2 } };
    for (int e = 0; e < 12; ++e)
        for (int k = 0; k < 4; ++k) t.shift[e][k] = sh[e][k];
    return t;
}
__constant__ McTables c_mc = mc_make_tables();

// corner number of the cube corner at (dx, dy, dz): 0..3 run round the bottom face, 4..7 round the top
__device__ __forceinline__ constexpr int mc_corner(int dx, int dy, int dz) { return dz * 4 + (dy ? 3 - dx : dx); }

// per 64 consecutive voxels: three ballots (bit l of m[a] = edge (voxel 64 g + l, axis a) carries a vertex) and the group's vertex
// and triangle offsets inside its chunk
struct McGroup {
    unsigned long long m[3];
    uint32_t vrel, trel;
};
static_assert(sizeof(McGroup) == 32, "one group record is 32 bytes");

}  // namespace
}  // namespace kpx
