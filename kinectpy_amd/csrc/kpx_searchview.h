// kpx_searchview.h -- the layout of a search index (kpx_search_index_build's caller-owned buffer) and the view of it that
// kernels walk: shared by kpx_search.hip, which builds and queries it, and kpx_orient.hip, whose exact nearest-foreign search walks
// the same grid.
#pragma once
#include "kpx_gridknn.h"

namespace kpx {

constexpr unsigned long long kSearchMagic = 0x314843525358504bull;      // "KPXSRCH1"
struct SearchHeader {
    unsigned long long magic;
    int64_t n;
    unsigned long long bytes;      // kpx_search_index_bytes(n)
    int32_t cell_cap, pad;
    GridParams gp;
};
struct SearchLayout { size_t cell_start, pts, idx, bytes; };
// the ceiling grid_build puts on the number of cells of an n-point cloud
static inline int32_t search_cell_cap(int64_t n)
{
    int32_t cell_cap = 65536;
    while (cell_cap < kGridMaxCells && (int64_t)cell_cap < 16 * n) cell_cap <<= 1;
    return cell_cap;
}
static inline SearchLayout search_layout(int64_t n)
{
    const size_t nn = (size_t)(n > 0 ? n : 1);
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    SearchLayout l;
    l.cell_start = up(sizeof(SearchHeader));
    l.pts = l.cell_start + up(((size_t)search_cell_cap(n) + 1) * sizeof(uint32_t));
    l.idx = l.pts + up(nn * 3 * sizeof(float));
    l.bytes = l.idx + up(nn * sizeof(int32_t));
    return l;
}
struct SearchView {
    GridParams g;
    const uint32_t *cell_start;
    const float *spts;
    const int32_t *sidx;
    int64_t n;
};

// The header comes back to the host (one small copy and a stream synchronisation per call): a buffer that is not an index, or is
// shorter than the index it claims to be, must not reach a kernel that would walk it.
static inline int search_open(const void *index, size_t index_bytes, hipStream_t st, SearchView *v)
{
    SearchHeader h;
    KPX_HIP(hipMemcpyAsync(&h, index, sizeof(h), hipMemcpyDeviceToHost, st));
    KPX_HIP(hipStreamSynchronize(st));
    KPX_REQUIRE(h.magic == kSearchMagic && h.n >= 0 && h.n < ((int64_t)1 << 31), "kpx_search: the buffer holds no index (kpx_search_index_build)");
    const SearchLayout l = search_layout(h.n);
    KPX_REQUIRE(h.bytes == l.bytes && h.cell_cap == search_cell_cap(h.n) && h.gp.dim[0] >= 1 && h.gp.dim[1] >= 1 && h.gp.dim[2] >= 1 &&
                    (int64_t)h.gp.dim[0] * h.gp.dim[1] * h.gp.dim[2] == (int64_t)h.gp.ncell && h.gp.ncell <= h.cell_cap && h.gp.h > 0.0,
                "kpx_search: the buffer holds no index (kpx_search_index_build)");
    KPX_REQUIRE(index_bytes >= l.bytes, "kpx_search: index_bytes %zu is smaller than the %zu bytes of an index of %lld points", index_bytes, l.bytes,
                (long long)h.n);
    const char *base = (const char *)index;
    v->g = h.gp;
    v->cell_start = reinterpret_cast<const uint32_t *>(base + l.cell_start);
    v->spts = reinterpret_cast<const float *>(base + l.pts);
    v->sidx = reinterpret_cast<const int32_t *>(base + l.idx);
    v->n = h.n;
    return KPX_OK;
}

}  // namespace kpx
