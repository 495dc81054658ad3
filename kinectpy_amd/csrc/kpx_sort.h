// kpx_sort.h -- the one place a device sort is carved and run: stable sorts of (key, int32 value) pairs or of bare keys on key bits
// [0, end_bit), keys of 32 or 64 bits.  A site keeps a DeviceSort in its scratch, carves it with dsort_carve and runs it with dsort_run:
//   * the library's own radix sort (kpx_radix.h) serves (uint32 key, value) pairs up to kRadixMaxPairs where the site carved its
//     scratch (SortOptions::radix); KPX_RADIX=0: the vendor sort instead, at every such site (A/B switch);
//   * rocPRIM's radix sort serves the rest, in the form the DeviceSort's type names (SortForm).
// The vendor sort reports the size of its temporary buffer when called without one.  Query and run are ONE function template here,
// vendor_sort, and the remembered answer is keyed on its instantiation, so a buffer cannot be sized by one sort and used by another.
// What is still assumed of rocPRIM: the size depends on (instantiation, n, end_bit) alone, not on the pointers, and does not grow when
// end_bit shrinks (of the buffer only the digit histograms depend on it, a row per 8 bits): dsort_run takes any end_bit <= max_end_bit.
#pragma once
#include "kpx_common.h"
#include "kpx_radix.h"

#include <rocprim/rocprim.hpp>
#include <type_traits>

namespace kpx {

// Below 1M keys rocPRIM's default is a merge sort: one block sort plus two launches per doubling (13 launches for 30k keys).  In this
// library's dependent chains the NUMBER of launches is what costs (every boundary also writes back / invalidates the L2s under
// everything else on the device), so keys of at most 32 bits go through Onesweep from 4096 pairs on: histogram + scan + one pass per
// 8 bits (5 launches for the 22-bit cell ids of a grid build).  Same result (both are stable).
using NarrowSortConfig = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config, 4096>;
// rocPRIM takes the width of its offsets -- and with it its kernels and the layout of the temporary buffer -- from the TYPE of the
// count: 32 bits for an int (what hipcub's radix sort, a one-line forward with the default config, hands on), 64 for a size_t.
enum SortForm {
    kSortNarrow,         // NarrowSortConfig, size_t count: the 32-bit keys
    kSortDefault,        // default config, size_t count: the mesh's 64-bit pair keys
    kSortDefault32,      // default config, int count (n < 2^31): voxel keys, batched curve keys, sampler keys
};
bool sort_radix_off();          // KPX_RADIX=0, read once (kpx_runtime.hip)

// tmp == nullptr: bytes receives the temporary size and nothing runs
template <class Key, bool kVals, SortForm kForm>
static inline hipError_t vendor_sort(void *tmp, size_t &bytes, const Key *keys_in, Key *keys_out, const int32_t *vals_in, int32_t *vals_out, int64_t n,
                                     int end_bit, hipStream_t st)
{
    using Config = std::conditional_t<kForm == kSortNarrow, NarrowSortConfig, rocprim::default_config>;
    const std::conditional_t<kForm == kSortDefault32, int, size_t> count = n;
    if constexpr (kVals) return rocprim::radix_sort_pairs<Config>(tmp, bytes, keys_in, keys_out, vals_in, vals_out, count, 0u, (unsigned)end_bit, st);
    // (the bare keys' kernels have been instantiated on a plain pointer from the start, and the iterator type is part of their names)
    else return rocprim::radix_sort_keys<Config>(tmp, bytes, const_cast<Key *>(keys_in), keys_out, count, 0u, (unsigned)end_bit, st);
}
// vendor_sort's size query, asked once per process (memo_bytes) under a key made of the instantiation, end_bit and n
template <class Key, bool kVals, SortForm kForm>
static inline size_t sort_tmp_bytes(int64_t n, int end_bit)
{
    const unsigned what = kMemoSort | (unsigned)end_bit << 4 | (unsigned)kForm << 2 | (kVals ? 2u : 0u) | (sizeof(Key) == 8 ? 1u : 0u);
    return memo_bytes(what, n, [&] { size_t b = 0; (void)vendor_sort<Key, kVals, kForm>(nullptr, b, nullptr, nullptr, nullptr, nullptr, n, end_bit, nullptr); return b; });
}

enum SortRadix {
    kVendorOnly,         // no scratch of the own radix sort
    kRadixAndVendor,     // both carved at every size, the radix scratch for at most kRadixMaxPairs: bytes(n) stays monotonic
    kRadixOrVendor,      // only what the sort that serves n needs
};
struct SortOptions {
    bool keys_in = true, keys_out = true, vals_in = true, vals_out = true;      // false: the caller's own array, set before the run
    SortRadix radix = kVendorOnly;
    size_t tmp_floor = 0;          // tmp holds at least this much: what else runs in it (a scan, dsort_view32)
};
template <class Key, bool kVals = true, SortForm kForm = (sizeof(Key) == 4 ? kSortNarrow : kSortDefault)>
struct DeviceSort {
    Key *keys_in, *keys_out;
    int32_t *vals_in, *vals_out;          // null without values
    char *tmp;
    size_t tmp_bytes;
    int max_end_bit;
    bool has_radix;
    RadixScratch rx;                      // carved last: its group histograms are the DeviceSort's last words
};
// whether dsort_run(s, n, ...) takes the own radix sort (and so clears up to clear_end)
template <class Key, bool kVals, SortForm kForm>
static inline bool dsort_by_radix(const DeviceSort<Key, kVals, kForm> &s, int64_t n)
{
    return sizeof(Key) == 4 && kVals && s.has_radix && n <= kRadixMaxPairs && !sort_radix_off();
}
template <class Key, bool kVals, SortForm kForm>
static void dsort_carve(Arena &a, int64_t n, int max_end_bit, const SortOptions &o, DeviceSort<Key, kVals, kForm> *s)
{
    const size_t nn = (size_t)(n > 0 ? n : 1);
    s->keys_in = o.keys_in ? a.get<Key>(nn) : nullptr;
    s->keys_out = o.keys_out ? a.get<Key>(nn) : nullptr;
    s->vals_in = kVals && o.vals_in ? a.get<int32_t>(nn) : nullptr;
    s->vals_out = kVals && o.vals_out ? a.get<int32_t>(nn) : nullptr;
    s->max_end_bit = max_end_bit;
    s->has_radix = o.radix != kVendorOnly;
    if (o.radix == kRadixOrVendor) s->has_radix = dsort_by_radix(*s, (int64_t)nn);
    const size_t need = o.radix == kRadixOrVendor && s->has_radix ? 0 : sort_tmp_bytes<Key, kVals, kForm>((int64_t)nn, max_end_bit);
    s->tmp_bytes = need > o.tmp_floor ? need : o.tmp_floor;
    s->tmp = a.get<char>(s->tmp_bytes);
    s->rx = RadixScratch();
    if (s->has_radix) radix_carve(a, (int64_t)nn <= kRadixMaxPairs ? (int64_t)nn : kRadixMaxPairs, &s->rx);
}
// keys_out (and vals_out) receive the n keys (pairs) of keys_in (and vals_in) in ascending order of key bits [0, end_bit), stable;
// the inputs are only read.  clear_end: the end of a region carved right behind the DeviceSort that the own radix sort's one memset
// clears too (radix_sort_pairs_u32); the vendor sort clears nothing of the caller's.
template <class Key, bool kVals, SortForm kForm>
static int dsort_run(const DeviceSort<Key, kVals, kForm> &s, int64_t n, int end_bit, hipStream_t st, const void *clear_end = nullptr)
{
    KPX_REQUIRE(end_bit >= 1 && end_bit <= s.max_end_bit, "device sort: end_bit %d outside [1, %d]", end_bit, s.max_end_bit);
    if constexpr (sizeof(Key) == 4 && kVals)
        if (dsort_by_radix(s, n)) return radix_sort_pairs_u32(s.rx, s.keys_in, s.keys_out, s.vals_in, s.vals_out, n, end_bit, st, clear_end);
    size_t bytes = s.tmp_bytes;
    const size_t need = sort_tmp_bytes<Key, kVals, kForm>(n, s.max_end_bit);
    KPX_REQUIRE(need <= bytes, "device sort: %zu temporary bytes carved, this sort needs %zu", bytes, need);
    KPX_HIP((vendor_sort<Key, kVals, kForm>(s.tmp, bytes, s.keys_in, s.keys_out, s.vals_in, s.vals_out, n, end_bit, st)));
    return KPX_OK;
}
// The voxel grids write keys of at most 32 bits as 32-bit words into the buffers of their 64-bit sort: the same scratch read that way.
// Its vendor sort is another instantiation with a size of its own, so the owner carves with tmp_floor = dsort_view32_bytes(n).
using DeviceSortView32 = DeviceSort<uint32_t, true, kSortDefault32>;
static inline size_t dsort_view32_bytes(int64_t n) { return sort_tmp_bytes<uint32_t, true, kSortDefault32>(n > 0 ? n : 1, 32); }
static inline DeviceSortView32 dsort_view32(const DeviceSort<uint64_t, true, kSortDefault32> &s)
{
    return { reinterpret_cast<uint32_t *>(s.keys_in), reinterpret_cast<uint32_t *>(s.keys_out), s.vals_in, s.vals_out, s.tmp, s.tmp_bytes,
             s.max_end_bit < 32 ? s.max_end_bit : 32, s.has_radix, s.rx };
}

}  // namespace kpx
