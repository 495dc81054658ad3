// kpx_mccore.h -- AC12 once, for the two marching-cubes extractions (kpx_tsdfmesh.hip over the uniform volume, kpx_tsdfblocks.hip over
// the block volume): the case table with its triangle counts and edge shifts in constant memory, the corner numbering, the count
// sweep as a kernel over a volume view (kpx_tsdfcore.h), and the rank of an edge's vertex.
#pragma once
#include "kpx_tsdfcore.h"
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

// Sweep 1 is each volume's own kernel: one code byte per voxel, the code of the cube whose corner 0 the voxel is (bit i = corner i
// negative); a corner that is not there or of weight 0 makes the cube inactive (0).

// ---- sweep 2: the group records and the chunks' counts (reads the code bytes only) --------------------------------------------
// bit a: edge (voxel, axis a) carries a vertex: one of the up to four cubes round it has the edge's two corners on different sides
// (an inactive cube has code 0: no difference; a cube behind the voxel may sit in another block, and where that is absent there is
// none).  *own = the code of the cube whose corner 0 the voxel is.
template <class V>
__device__ __forceinline__ unsigned mc_edge_flags(const V &v, const uint8_t *__restrict__ codes, const typename V::Cell &cell, unsigned *own)
{
    unsigned m = 0u;
#pragma unroll
    for (int dx = 0; dx < 2; ++dx)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dz = 0; dz < 2; ++dz) {
                if (dx + dy + dz == 3) continue;                     // that cube holds none of the voxel's three edges
                int64_t virt = 0;
                if (v.at(cell, -dx, -dy, -dz, &virt) < 0) continue;
                const unsigned c = codes[virt];
                if (dx + dy + dz == 0) *own = c;
                const unsigned at = (c >> mc_corner(dx, dy, dz)) & 1u;
                if (dx == 0 && (((c >> mc_corner(1, dy, dz)) & 1u) != at)) m |= 1u;
                if (dy == 0 && (((c >> mc_corner(dx, 1, dz)) & 1u) != at)) m |= 2u;
                if (dz == 0 && (((c >> mc_corner(dx, dy, 1)) & 1u) != at)) m |= 4u;
            }
    return m;
}

template <class V>
__global__ __launch_bounds__(kExtractWaves * 64) void mc_count_kernel(V v, const uint8_t *__restrict__ codes, int64_t nchunks, McGroup *__restrict__ groups,
                                                                      int64_t *__restrict__ vcount, int64_t *__restrict__ tcount)
{
    const int64_t chunk = (int64_t)blockIdx.x * kExtractWaves + wave_id();
    if (chunk >= nchunks) return;
    const int64_t nvox = v.size();
    const int lane = lane_id();
    uint32_t vrun = 0u, trun = 0u;             // trun is lane 0's
    for (int r = 0; r < kChunkRounds; ++r) {
        const int64_t g = chunk * kChunkRounds + r, lin = g * 64 + lane;
        if (g * 64 >= nvox) break;
        unsigned m = 0u, own = 0u;
        if (lin < nvox) m = mc_edge_flags(v, codes, v.split(lin), &own);
        const unsigned long long b0 = __ballot((m & 1u) != 0), b1 = __ballot((m & 2u) != 0), b2 = __ballot((m & 4u) != 0);
        const int nt = wave_sum((int)c_mc.ntri[own]);
        if (lane == 0) {
            McGroup G;
            G.m[0] = b0; G.m[1] = b1; G.m[2] = b2;
            G.vrel = vrun; G.trel = trun;
            groups[g] = G;
            trun += (uint32_t)nt;
        }
        vrun += (uint32_t)(__builtin_popcountll(b0) + __builtin_popcountll(b1) + __builtin_popcountll(b2));
    }
    if (lane == 0) {
        vcount[chunk] = vrun;
        tcount[chunk] = trun;
    }
}

// vertex index of edge (voxel lin, axis a)
__device__ __forceinline__ int64_t mc_rank(const McGroup *__restrict__ groups, const int64_t *__restrict__ voff, int64_t lin, int a)
{
    const int64_t g = lin >> 6;
    const int l = (int)(lin & 63);
    const McGroup G = groups[g];
    const unsigned long long below = (1ull << l) - 1ull;
    int64_t r = voff[g / kChunkRounds] + G.vrel + __builtin_popcountll(G.m[0] & below) + __builtin_popcountll(G.m[1] & below) +
                __builtin_popcountll(G.m[2] & below);
    if (a >= 1) r += (int64_t)((G.m[0] >> l) & 1ull);
    if (a == 2) r += (int64_t)((G.m[1] >> l) & 1ull);
    return r;
}

// Sweep 3 (vertices and colours by rank, triangles by the scanned triangle offsets) is each volume's own kernel: DESIGN.md 5.17.

constexpr int64_t kMeshMax = 2147483647;        // int32 indices

}  // namespace
}  // namespace kpx
