// kpx_tsdfmesh.hip -- marching cubes over a uniform TSDF volume ([O3D] UniformTSDFVolume.extract_triangle_mesh; arithmetic contract
// AC12): the code and fill sweeps of the uniform volume and the host side; the count sweep is kpx_mccore.h's
// over the UniformView.  The operators on the extracted mesh are kpx_mesh.hip's.
//
// Extraction keeps the shape of the point-cloud extraction of kpx_tsdf.hip: count, one host read, fill; no atomics, every output
// slot has one owner.  Workspace, carried from count to fill:
//   codes   u8  [res^3]        the cube code at the cube's corner 0 (bit i = corner i negative), 0 = inactive / no cube there
//   groups  32B [res^3 / 64]   per 64 consecutive voxels: three ballots (bit l of m[a] = edge (voxel 64 g + l, axis a) carries a
//                              vertex) and the group's vertex and triangle offsets inside its chunk of 512 voxels
//   voff, toff  i64 [chunks+1] exclusive scans of the chunks' vertex and triangle counts
// The rank of edge (v, a) -- its vertex index -- is voff[chunk] + group.vrel + popcounts of the three ballots below v's lane + the
// set bits of the lower axes at the lane: the order of extract_point_cloud, ascending (linear index, axis).
#include "kpx_mccore.h"

namespace kpx {
namespace {

// sweep 1, not over the view: one test for the whole cube, then eight loads at fixed strides that the compiler pairs along z
__global__ __launch_bounds__(256) void mc_code_kernel(const float2 *__restrict__ vol, int res, int64_t nvox, uint8_t *__restrict__ codes)
{
    const int64_t lin = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (lin >= nvox) return;
    int x, y, z;
    tsdf_split((uint32_t)lin, (uint32_t)res, x, y, z);
    unsigned code = 0u;
    if (x < res - 1 && y < res - 1 && z < res - 1) {
        const int64_t sx = (int64_t)res * res, sy = res;
        bool active = true;
#pragma unroll
        for (int dx = 0; dx < 2; ++dx)
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dz = 0; dz < 2; ++dz) {
                    const float2 v = vol[lin + dx * sx + dy * sy + dz];
                    active = active && v.y != 0.0f;
                    if (v.x < 0.0f) code |= 1u << mc_corner(dx, dy, dz);
                }
        if (!active) code = 0u;
    }
    codes[lin] = (uint8_t)code;
}

struct McFillArgs {
    double org[3], vl;
    const float *col;
    float *overt, *ocol;
    int32_t *otri;
    int64_t nv, nt;
};

// sweep 3, not over the view (it measured slower there): vertices and colours by rank, triangles by the scanned triangle offsets
__global__ __launch_bounds__(kExtractWaves * 64) void mc_fill_kernel(const float2 *__restrict__ vol, const uint8_t *__restrict__ codes, int res, int64_t nvox,
                                                                     int64_t nchunks, const McGroup *__restrict__ groups, const int64_t *__restrict__ voff,
                                                                     const int64_t *__restrict__ toff, McFillArgs a)
{
    const int64_t chunk = (int64_t)blockIdx.x * kExtractWaves + wave_id();
    if (chunk >= nchunks) return;
    const int lane = lane_id();
    const unsigned long long below = (1ull << lane) - 1ull;
    const int64_t vbase = voff[chunk], tbase = toff[chunk];
    if (voff[chunk + 1] == vbase && toff[chunk + 1] == tbase) return;
    const int64_t step[3] = { (int64_t)res * res, (int64_t)res, 1 };
    for (int r = 0; r < kChunkRounds; ++r) {
        const int64_t g = chunk * kChunkRounds + r, lin = g * 64 + lane;
        if (g * 64 >= nvox) break;
        const McGroup G = groups[g];
        int x = 0, y = 0, z = 0;
        if (lin < nvox) tsdf_split((uint32_t)lin, (uint32_t)res, x, y, z);
        // the vertices of this voxel's three edges
        const unsigned mine = lin < nvox ? (unsigned)((G.m[0] >> lane) & 1ull) | (unsigned)((G.m[1] >> lane) & 1ull) << 1 | (unsigned)((G.m[2] >> lane) & 1ull) << 2 : 0u;
        if (mine) {
            int64_t dst = vbase + G.vrel + __builtin_popcountll(G.m[0] & below) + __builtin_popcountll(G.m[1] & below) + __builtin_popcountll(G.m[2] & below);
            const int ix[3] = { x, y, z };
            const double f0 = fabs((double)vol[lin].x);
            const double p0[3] = { ((double)x + 0.5) * a.vl, ((double)y + 0.5) * a.vl, ((double)z + 0.5) * a.vl };
            for (int i = 0; i < 3; ++i) {
                if (!((mine >> i) & 1u)) continue;
                if (dst >= a.nv || ix[i] + 1 >= res) break;           // never true for the ws the count pass left
                const double f1 = fabs((double)vol[lin + step[i]].x);
                double p[3] = { p0[0], p0[1], p0[2] };
                p[i] = p[i] + (f0 * a.vl) / (f0 + f1);
#pragma unroll
                for (int k = 0; k < 3; ++k) a.overt[3 * dst + k] = (float)(p[k] + a.org[k]);
                if (a.ocol) {
                    const float *c0 = a.col + 3 * lin, *c1 = a.col + 3 * (lin + step[i]);
#pragma unroll
                    for (int k = 0; k < 3; ++k) a.ocol[3 * dst + k] = (float)((f1 * ((double)c0[k] / 255.0) + f0 * ((double)c1[k] / 255.0)) / (f0 + f1));
                }
                ++dst;
            }
        }
        // the triangles of the cube at this voxel
        unsigned code = 0u;
        if (lin < nvox && x < res - 1 && y < res - 1 && z < res - 1) code = codes[lin];
        const int nt = c_mc.ntri[code];
        const int incl = wave_incl_scan(nt);
        int64_t tdst = tbase + G.trel + (incl - nt);
        for (int t = 0; t < nt; ++t, ++tdst) {
            if (tdst >= a.nt) break;
            int32_t idx[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int e = c_mc.tri[code][3 * t + k];
                const signed char *s = c_mc.shift[e];
                idx[k] = (int32_t)mc_rank(groups, voff, lin + s[0] * step[0] + s[1] * step[1] + s[2], s[3]);
            }
            a.otri[3 * tdst] = idx[0];
            a.otri[3 * tdst + 1] = idx[2];
            a.otri[3 * tdst + 2] = idx[1];
        }
    }
}

inline bool mc_res_ok(int32_t res) { return res >= 1 && res <= KPX_TSDF_MAX_RESOLUTION; }

struct McScratch {
    uint8_t *codes;
    McGroup *groups;
    int64_t *voff, *toff;
    int64_t nvox, nchunks;
};
void mc_carve(Arena &a, int32_t res, McScratch *s)
{
    s->nvox = (int64_t)res * res * res;
    s->nchunks = cdiv(s->nvox, kChunk);
    s->codes = a.get<uint8_t>((size_t)s->nvox);
    s->groups = a.get<McGroup>((size_t)s->nchunks * kChunkRounds);
    s->voff = a.get<int64_t>((size_t)s->nchunks + 1);
    s->toff = a.get<int64_t>((size_t)s->nchunks + 1);
}

}  // namespace
}  // namespace kpx

using namespace kpx;

KPX_EXPORT size_t kpx_tsdf_mesh_workspace_bytes(int32_t resolution)
{
    if (!mc_res_ok(resolution)) return 0;
    Arena a(nullptr, 0);
    McScratch s;
    mc_carve(a, resolution, &s);
    return a.off;
}

KPX_EXPORT int kpx_tsdf_mesh_count(const float *volume, int32_t resolution, int64_t *d_counts, void *ws, size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(mc_res_ok(resolution), "kpx_tsdf_mesh_count: resolution must be in [1, %d]", KPX_TSDF_MAX_RESOLUTION);
    KPX_REQUIRE(volume && d_counts && ws, "kpx_tsdf_mesh_count: null pointer");
    Arena a(ws, ws_bytes);
    McScratch s;
    mc_carve(a, resolution, &s);
    KPX_ARENA_CHECK(a);
    const UniformView v = uniform_view(volume, nullptr, resolution, 0.0, nullptr);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mc_code_kernel, dim3((unsigned)cdiv(s.nvox, 256)), dim3(256), 0, st, v.vol, resolution, s.nvox, s.codes);
    hipLaunchKernelGGL(mc_count_kernel<UniformView>, dim3((unsigned)cdiv(s.nchunks, kExtractWaves)), dim3(kExtractWaves * 64), 0, st, v, (const uint8_t *)s.codes,
                       s.nchunks, s.groups, s.voff, s.toff);
    scan2_i64(s.voff, s.toff, s.nchunks, st);
    KPX_LAUNCH_CHECK();
    KPX_HIP(hipMemcpyAsync(d_counts, s.voff + s.nchunks, sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    KPX_HIP(hipMemcpyAsync(d_counts + 1, s.toff + s.nchunks, sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    return KPX_OK;
}

KPX_EXPORT int kpx_tsdf_mesh_fill(const float *volume, const float *color, int32_t resolution, double voxel_length, const double *h_origin,
                                  int64_t n_vertices, int64_t n_triangles, float *out_vertices, float *out_colors, int32_t *out_triangles, void *ws,
                                  size_t ws_bytes, void *stream)
{
    KPX_REQUIRE(mc_res_ok(resolution), "kpx_tsdf_mesh_fill: resolution must be in [1, %d]", KPX_TSDF_MAX_RESOLUTION);
    KPX_REQUIRE(voxel_length > 0.0 && n_vertices >= 0 && n_triangles >= 0, "kpx_tsdf_mesh_fill: bad voxel_length or counts");
    if (n_vertices > kMeshMax || n_triangles > kMeshMax)
        return fail(KPX_ERR_RANGE, "kpx_tsdf_mesh_fill: %lld vertices and %lld triangles: a mesh holds fewer than 2^31 of each", (long long)n_vertices,
                    (long long)n_triangles);
    if (n_vertices == 0 && n_triangles == 0) return KPX_OK;
    KPX_REQUIRE(volume && h_origin && ws && (n_vertices == 0 || out_vertices) && (n_triangles == 0 || out_triangles), "kpx_tsdf_mesh_fill: null pointer");
    KPX_REQUIRE(!out_colors || color, "kpx_tsdf_mesh_fill: colours need a colour volume");
    Arena a(ws, ws_bytes);
    McScratch s;
    mc_carve(a, resolution, &s);
    KPX_ARENA_CHECK(a);
    const McFillArgs f = { { h_origin[0], h_origin[1], h_origin[2] }, voxel_length, color, out_vertices, out_colors, out_triangles, n_vertices, n_triangles };
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mc_fill_kernel, dim3((unsigned)cdiv(s.nchunks, kExtractWaves)), dim3(kExtractWaves * 64), 0, st, reinterpret_cast<const float2 *>(volume),
                       (const uint8_t *)s.codes, resolution, s.nvox, s.nchunks, (const McGroup *)s.groups, (const int64_t *)s.voff, (const int64_t *)s.toff, f);
    KPX_LAUNCH_CHECK();
    return KPX_OK;
}
