// kpx_icpchain.h (host) -- the one-launch chain: who may be resident
// icp_chain_kernel needs all its blocks resident together, so the host admits a chain only while the blocks of every chain kernel it
// has in flight on the device (this process: the deployment is one process per GPU) plus the new ones fit a budget below what the
// device holds (blocks per CU by the occupancy API minus one -- MI355X_MICROARCH.md, "Correctness boundaries": the API can be one
// block per CU high -- times the CUs).  A chain that does not fit runs in the launch-per-iteration form: nothing ever waits for
// another chain.  Finished chains are retired by querying the event recorded behind them.
#pragma once
#include <fcntl.h>
#include <mutex>
#include <stdio.h>
#include <stdlib.h>
#include <sys/file.h>
#include <unistd.h>

#include "kpx_icpiter.h"

namespace kpx {

// the one-launch chain: on unless KPX_ICP_CHAIN=0; kpx_icp_chain() switches it at run time (A/B measurements inside one process)
static int g_chain_form = -1;
static int g_chain_launches = 0;                // chains launched by this process (kpx_icp_chain(-2): tests check that the form they test ran)
static bool chain_form_on()
{
    if (g_chain_form < 0) { const char *e = getenv("KPX_ICP_CHAIN"); g_chain_form = (e && e[0] == '0') ? 0 : 1; }
    return g_chain_form != 0;
}

struct ChainSlot {
    hipEvent_t ev;
    unsigned blocks;
    bool busy, made;
};
struct ChainBook {
    std::mutex mu;
    ChainSlot slot[16] = {};
    long budget = -1;                                    // blocks; -1 = not asked yet
};
static ChainBook g_chain_book[16];
static unsigned long long *g_chain_abort = nullptr;             // pinned: raised by a chain block that gave up waiting
static std::once_flag g_chain_abort_once;
static unsigned long long *chain_abort_word()
{
    std::call_once(g_chain_abort_once, [] {
        if (hipHostMalloc((void **)&g_chain_abort, 64, hipHostMallocDefault) != hipSuccess) g_chain_abort = nullptr;
        else *g_chain_abort = 0ull;
    });
    return g_chain_abort;
}
// forced_budget >= 0: KPX_ICP_CHAIN_BUDGET; no_lock: KPX_ICP_CHAIN_LOCK=0, the caller vouches for being alone (both read by icp_switches, kpx_icp.hip)
template <class F> static bool chain_launch_if_fits(unsigned blocks, hipStream_t st, long forced_budget, bool no_lock, F &&launch)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return false;
    ChainBook &bk = g_chain_book[dev];
    std::lock_guard<std::mutex> lock(bk.mu);
    if (bk.budget < 0) {
        int per_cu = 0, cus = 0;
        // ONE process per GPU may run chains: two processes each admitting chains against the whole device could leave blocks of both
        // waiting for wave slots the other holds (ended only by the timeout).  The first process to take the device's lock file keeps
        // it for its lifetime; the others (ranks sharing a GPU in a rehearsal, a second service on the same card) run a launch per
        // iteration.  No lock (no writable /tmp, no bus id) = no chains.
        bool mine = no_lock;
        char bus[64] = { 0 };
        if (!mine && hipDeviceGetPCIBusId(bus, (int)sizeof(bus), dev) == hipSuccess) {
            char path[128];
            for (char *c = bus; *c; ++c) if (!((*c >= '0' && *c <= '9') || (*c >= 'a' && *c <= 'f') || (*c >= 'A' && *c <= 'F'))) *c = '_';
            // (per user, never through a planted symlink, not inherited across exec; containers that share a GPU but not /dev/shm each
            // believe they are alone: such deployments set KPX_ICP_CHAIN=0 -- INTEGRATION.md)
            snprintf(path, sizeof(path), "/dev/shm/kpx_chain_%u_%s.lock", (unsigned)getuid(), bus);
            const int fd = open(path, O_CREAT | O_RDWR | O_CLOEXEC | O_NOFOLLOW, 0600);
            if (fd >= 0) {
                if (flock(fd, LOCK_EX | LOCK_NB) == 0) mine = true;        // (kept open: the lock lives as long as the process)
                else close(fd);
            }
        }
        if (!mine) bk.budget = 0;
        else if (forced_budget >= 0) bk.budget = forced_budget;
        else if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)icp_chain_kernel, kIThreads, 0) == hipSuccess &&
                 hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && per_cu > 1)
            bk.budget = (long)(per_cu - 1) * cus;
        else bk.budget = 0;
    }
    long used = 0;
    int free_slot = -1;
    for (int i = 0; i < 16; ++i) {
        ChainSlot &c = bk.slot[i];
        if (c.busy && hipEventQuery(c.ev) == hipSuccess) c.busy = false;
        if (c.busy) used += c.blocks;
        else if (free_slot < 0) free_slot = i;
    }
    if (free_slot < 0 || used + (long)blocks > bk.budget) return false;
    ChainSlot &c = bk.slot[free_slot];
    if (!c.made) {
        if (hipEventCreateWithFlags(&c.ev, hipEventDisableTiming) != hipSuccess) return false;
        c.made = true;
    }
    launch();
    __atomic_fetch_add(&g_chain_launches, 1, __ATOMIC_RELAXED);
    if (hipEventRecord(c.ev, st) != hipSuccess) return true;     // launched all the same; the slot just is not booked
    c.blocks = blocks;
    c.busy = true;
    return true;
}

}  // namespace kpx
