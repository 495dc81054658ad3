// kpx_runtime.hip -- the library's host runtime, no kernels: the per-thread error text, the HIP-event profiler, the memo of the
// vendor primitives' size queries, the KPX_RADIX switch, and what a host thread holds (pinned blocks, lanes).
#include <stdarg.h>

#include <atomic>
#include <mutex>
#include <unordered_map>

#include "kpx_internal.h"

namespace kpx {

thread_local char g_err[512] = "";
int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// ---- profiler -------------------------------------------------------------------------------------
static struct {
    bool on = false;
    int stride = 1;                          // time every stride-th launch of a kernel id
    long long total[KPX_PROF_KERNELS] = {};  // launches seen while armed, timed or not
    int cap = 0, used = 0;
    hipEvent_t *e0 = nullptr, *e1 = nullptr;
    int *kid = nullptr;
    double *work = nullptr;
} g_prof;

bool prof_armed() { return g_prof.on; }
static std::mutex g_prof_mutex;         // launches may come from several host threads
ProfScope::ProfScope(int kernel_id, double w, hipStream_t stream) : slot(-1), st(stream)
{
    if (!g_prof.on) return;
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    if ((g_prof.total[kernel_id]++ % g_prof.stride) != 0 || g_prof.used >= g_prof.cap) return;
    slot = g_prof.used++;
    g_prof.kid[slot] = kernel_id;
    g_prof.work[slot] = w;
    (void)hipEventRecord(g_prof.e0[slot], st);
}
ProfScope::~ProfScope()
{
    if (slot >= 0) (void)hipEventRecord(g_prof.e1[slot], st);
}

// ---- size-query memo (kpx_common.h) and the sorts' KPX_RADIX switch (kpx_sort.h) ---------------------
static std::mutex g_memo_mu;
static std::unordered_map<unsigned long long, size_t> g_memo;
size_t memo_bytes(unsigned what, int64_t n, const std::function<size_t()> &query)
{
    const unsigned long long key = ((unsigned long long)what << 48) ^ (unsigned long long)n;
    {
        std::lock_guard<std::mutex> lock(g_memo_mu);
        auto it = g_memo.find(key);
        if (it != g_memo.end()) return it->second;
    }
    const size_t bytes = query();
    std::lock_guard<std::mutex> lock(g_memo_mu);
    return g_memo[key] = bytes;
}
bool sort_radix_off()
{
    static const bool off = [] { const char *e = getenv("KPX_RADIX"); return e && e[0] == '0'; }();
    return off;
}

// ---- what a host thread holds (kpx_internal.h) -------------------------------------------------------------------
// process-wide sums over the threads' owners: [0] pinned bytes, [1] streams, [2] events, [3] threads holding any
static std::atomic<uint64_t> g_held[4];
ThreadResources &thread_resources()
{
    static thread_local ThreadResources mine;
    return mine;
}
void ThreadResources::hold()
{
    if (!counted) g_held[3].fetch_add(1, std::memory_order_relaxed);
    counted = true;
}
void *ThreadResources::pinned_alloc(PinnedSite site, size_t bytes)
{
    void *p = nullptr;
    const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e != hipSuccess) {
        fail(KPX_ERR_HIP, "hipHostMalloc of %zu bytes: %s", bytes, hipGetErrorString(e));
        return nullptr;
    }
    memset(p, 0, bytes);
    pin[site] = p;
    pin_bytes[site] = bytes;
    g_held[0].fetch_add(bytes, std::memory_order_relaxed);
    hold();
    return p;
}
ThreadResources::~ThreadResources()
{
    for (int i = 0; i < kPinnedSites; ++i)
        if (pin[i]) {
            (void)hipHostFree(pin[i]);
            g_held[0].fetch_sub(pin_bytes[i], std::memory_order_relaxed);
        }
    for (LaneSet &set : lanes) {
        for (int l = 0; l < kLaneCount; ++l) {
            if (set.s[l]) { (void)hipStreamDestroy(set.s[l]); g_held[1].fetch_sub(1, std::memory_order_relaxed); }
            if (set.join[l]) { (void)hipEventDestroy(set.join[l]); g_held[2].fetch_sub(1, std::memory_order_relaxed); }
        }
        if (set.fork) { (void)hipEventDestroy(set.fork); g_held[2].fetch_sub(1, std::memory_order_relaxed); }
    }
    if (counted) g_held[3].fetch_sub(1, std::memory_order_relaxed);
}
int lanes_get(LaneSet **out)
{
    // one set per host thread and device: the fork / join events belong to one call at a time, and streams belong to
    // the device that was current when they were created
    int dev = 0;
    KPX_HIP(hipGetDevice(&dev));
    KPX_REQUIRE(dev >= 0 && dev < kLaneDevices, "lanes_get: device ordinal %d out of range", dev);
    ThreadResources &tr = thread_resources();
    LaneSet &set = tr.lanes[dev];
    if (!set.fork) {                       // (what an earlier, failed attempt did create is kept and counted)
        tr.hold();
        for (int l = 0; l < kLaneCount; ++l) {
            if (!set.s[l]) { KPX_HIP(hipStreamCreateWithFlags(&set.s[l], hipStreamNonBlocking)); g_held[1].fetch_add(1, std::memory_order_relaxed); }
            if (!set.join[l]) { KPX_HIP(hipEventCreateWithFlags(&set.join[l], hipEventDisableTiming)); g_held[2].fetch_add(1, std::memory_order_relaxed); }
        }
        KPX_HIP(hipEventCreateWithFlags(&set.fork, hipEventDisableTiming));
        g_held[2].fetch_add(1, std::memory_order_relaxed);
    }
    *out = &set;
    return KPX_OK;
}
int lanes_fork(LaneSet *l, hipStream_t caller, int used)
{
    KPX_HIP(hipEventRecord(l->fork, caller));
    for (int i = 0; i < used && i < kLaneCount; ++i) KPX_HIP(hipStreamWaitEvent(l->s[i], l->fork, 0));
    return KPX_OK;
}
int lanes_join(LaneSet *l, hipStream_t caller, int used)
{
    for (int i = 0; i < used && i < kLaneCount; ++i) {
        KPX_HIP(hipEventRecord(l->join[i], l->s[i]));
        KPX_HIP(hipStreamWaitEvent(caller, l->join[i], 0));
    }
    return KPX_OK;
}

}  // namespace kpx

using namespace kpx;

KPX_EXPORT const char *kpx_last_error(void) { return g_err; }
KPX_EXPORT int kpx_version(void) { return KPX_VERSION; }

KPX_EXPORT int kpx_host_resources(uint64_t *h_out4)
{
    KPX_REQUIRE(h_out4, "kpx_host_resources: null pointer");
    for (int i = 0; i < 4; ++i) h_out4[i] = g_held[i].load(std::memory_order_relaxed);
    return KPX_OK;
}

KPX_EXPORT int kpx_prof_begin(int32_t capacity)
{
    KPX_REQUIRE(capacity > 0 && capacity <= (1 << 20), "kpx_prof_begin: bad capacity");
    if (g_prof.cap < capacity) {
        for (int i = 0; i < g_prof.cap; ++i) { (void)hipEventDestroy(g_prof.e0[i]); (void)hipEventDestroy(g_prof.e1[i]); }
        delete[] g_prof.e0; delete[] g_prof.e1; delete[] g_prof.kid; delete[] g_prof.work;
        g_prof.e0 = new hipEvent_t[capacity]; g_prof.e1 = new hipEvent_t[capacity];
        g_prof.kid = new int[capacity]; g_prof.work = new double[capacity];
        for (int i = 0; i < capacity; ++i) { KPX_HIP(hipEventCreate(&g_prof.e0[i])); KPX_HIP(hipEventCreate(&g_prof.e1[i])); }
        g_prof.cap = capacity;
    }
    g_prof.used = 0;
    for (int k = 0; k < KPX_PROF_KERNELS; ++k) g_prof.total[k] = 0;
    g_prof.on = true;
    (void)nn_local_take_visits();
    return KPX_OK;
}
KPX_EXPORT int kpx_prof_stride(int32_t stride)
{
    KPX_REQUIRE(stride >= 1, "kpx_prof_stride: stride must be >= 1");
    g_prof.stride = stride;
    return KPX_OK;
}
KPX_EXPORT int kpx_prof_end(double *h_ms, int64_t *h_launches, double *h_work)
{
    KPX_REQUIRE(h_ms && h_launches && h_work, "kpx_prof_end: null pointer");
    g_prof.on = false;
    for (int k = 0; k < KPX_PROF_KERNELS; ++k) { h_ms[k] = 0.0; h_launches[k] = 0; h_work[k] = 0.0; }
    for (int i = 0; i < g_prof.used; ++i) {
        KPX_HIP(hipEventSynchronize(g_prof.e1[i]));
        float ms = 0.f;
        KPX_HIP(hipEventElapsedTime(&ms, g_prof.e0[i], g_prof.e1[i]));
        int k = g_prof.kid[i];
        h_ms[k] += ms; h_launches[k] += 1; h_work[k] += g_prof.work[i];
    }
    g_prof.used = 0;
    // flops actually issued (16 x 16 x 4 MAC per tile), scaled to the timed share of the launches
    h_work[KPX_PROF_NN_LOCAL] = 2048.0 * nn_local_take_visits() * (g_prof.total[KPX_PROF_NN_LOCAL] > 0
                                    ? (double)h_launches[KPX_PROF_NN_LOCAL] / (double)g_prof.total[KPX_PROF_NN_LOCAL] : 0.0);
    return KPX_OK;
}
