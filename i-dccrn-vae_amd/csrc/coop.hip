// Per-device process state and the launch path of the cooperative (spin-synchronised) recurrences (coop.hpp).
//
// Two cooperative launches must never share the chip: each needs ALL its workgroups resident (it spins on its siblings), and
// two half-resident launches on different streams would wait for each other until the spin bound poisons both.  Launches
// from different streams of one device are therefore chained through an event (other kernels may still overlap them).
#include <cstdlib>
#include <mutex>
#include "common.hpp"
#include "coop.hpp"
#include "../../include/idccrn_hip.h"

static std::mutex g_pers_mu;
static hipEvent_t g_pers_done[16] = {};
static hipStream_t g_pers_stream[16] = {};
static int g_max_wg[16] = {};                 // 0: not queried yet
static unsigned* g_status_host[16] = {};      // host-mapped sticky status words
static unsigned* g_status_dev[16] = {};
static bool g_status_tried[16] = {};

static int cur_dev() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return -1;
    return dev;
}

extern "C" int idv_coop_max_workgroups(void) {
    // no device visible (sizing queries in the build container): the MI355X figure, 256 CUs - 16
    const int dev = cur_dev();
    if (dev < 0) { (void)hipGetLastError(); return 240; }
    std::lock_guard<std::mutex> lk(g_pers_mu);
    if (g_max_wg[dev] == 0) {
        hipDeviceProp_t pr;
        if (hipGetDeviceProperties(&pr, dev) != hipSuccess || pr.multiProcessorCount <= 0) {
            (void)hipGetLastError();
            g_max_wg[dev] = 240;
        } else {
            // one workgroup per CU (every cooperative launch requests > half a CU's LDS); 1/16 of the CUs stay free so that a
            // kernel of another stream still finds a CU and never delays the start of a sibling workgroup indefinitely
            const int cu = pr.multiProcessorCount;
            int n = cu - cu / 16;
            const char* e = getenv("IDV_COOP_MAX_WG");              // experiments / CU-masked devices
            if (e && atoi(e) > 0 && atoi(e) < n) n = atoi(e);
            g_max_wg[dev] = n;
        }
    }
    return g_max_wg[dev];
}

// device pointer of the current device's sticky status word (nullptr if it cannot be allocated: the kernels then only poison)
static unsigned* idv_coop_status_word() {
    const int dev = cur_dev();
    if (dev < 0) return nullptr;
    std::lock_guard<std::mutex> lk(g_pers_mu);
    if (!g_status_tried[dev]) {
        g_status_tried[dev] = true;
        void* h = nullptr;
        void* d = nullptr;
        if (hipHostMalloc(&h, 256, hipHostMallocMapped) == hipSuccess) {
            *(volatile unsigned*)h = 0u;
            if (hipHostGetDevicePointer(&d, h, 0) == hipSuccess) {
                g_status_host[dev] = (unsigned*)h;
                g_status_dev[dev] = (unsigned*)d;
            } else {
                (void)hipHostFree(h);
            }
        }
        (void)hipGetLastError();
    }
    return g_status_dev[dev];
}

// IDV_ECOOP if a cooperative kernel of the current device has timed out since the status was last cleared (its outputs are
// NaN-poisoned); clear != 0 acknowledges and resets it -- until then every cooperative entry of the device refuses with IDV_ECOOP.  The word is written by the device when the kernel aborts, so a launch that is
// still queued is not covered: synchronise the stream first for a definite answer.
extern "C" int idv_coop_last_status(int clear) {
    const int dev = cur_dev();
    if (dev < 0) return IDV_ELAUNCH;
    (void)idv_coop_status_word();
    std::lock_guard<std::mutex> lk(g_pers_mu);
    volatile unsigned* w = g_status_host[dev];
    if (!w || !*w) return IDV_OK;
    if (clear) *w = 0u;
    return IDV_ECOOP;
}

namespace {

// The launch chain of the current device, held for the duration of one cooperative launch on `st`.  The constructor takes the
// lock and makes `st` wait for the previous cooperative launch of the device; it leaves a non-zero rc -- lock NOT held, status
// NOT cleared -- when it refuses.  The destructor of a chain that is held records the launch and releases the lock, and leaves
// IDV_ELAUNCH in rc if the launch could not be recorded.
class CoopChain {
public:
    CoopChain(hipStream_t st, int& rc) : st_(st), dev_(cur_dev()), rc_(rc) {
        if (dev_ < 0) { rc_ = IDV_ELAUNCH; return; }
        std::unique_lock<std::mutex> lk(g_pers_mu);
        volatile unsigned* w = g_status_host[dev_];
        // an earlier cooperative launch timed out and nobody has acknowledged it: refuse, like a sticky device error, until
        // idv_coop_last_status(1) -- the status is NOT consumed here, so an unrelated caller cannot swallow it
        if (w && *w) { rc_ = IDV_ECOOP; return; }
        if (g_pers_done[dev_] && g_pers_stream[dev_] != st_ && hipStreamWaitEvent(st_, g_pers_done[dev_], 0) != hipSuccess) {
            rc_ = IDV_ELAUNCH;
            return;
        }
        rc_ = IDV_OK;
        lk_ = std::move(lk);
    }
    ~CoopChain() {
        if (!lk_.owns_lock()) return;
        if (!g_pers_done[dev_] && hipEventCreateWithFlags(&g_pers_done[dev_], hipEventDisableTiming) != hipSuccess) rc_ = IDV_ELAUNCH;
        else if (hipEventRecord(g_pers_done[dev_], st_) != hipSuccess) rc_ = IDV_ELAUNCH;
        else g_pers_stream[dev_] = st_;
    }
    CoopChain(const CoopChain&) = delete;
    CoopChain& operator=(const CoopChain&) = delete;

private:
    hipStream_t st_;
    int dev_;
    int& rc_;
    std::unique_lock<std::mutex> lk_;
};

}  // namespace

int idv_coop_launch_raw(const void* kernel, dim3 grid, size_t smem, hipStream_t st, void* work, size_t sync_bytes, CoopSync* cs,
                        void** params) {
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess) return IDV_ELAUNCH;
    // only the polled words are zeroed: every row of the exchange buffer a step reads was written by the step before
    if (hipMemsetAsync(work, 0, sync_bytes, st) != hipSuccess) return IDV_ELAUNCH;
    cs->sync = (unsigned*)work;
    cs->status = idv_coop_status_word();
    { const char* e = getenv("IDV_COOP_FAULT"); cs->fault = (e && e[0] == '1') ? 1 : 0; }
    int rc;
    {
        CoopChain chain(st, rc);
        if (!rc) (void)hipLaunchKernel(kernel, grid, dim3(256), params, smem, st);      // its error: idv_launch_status() below
    }
    return rc ? rc : idv_launch_status();
}
