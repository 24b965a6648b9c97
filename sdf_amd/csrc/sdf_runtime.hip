// sdf_runtime.hip -- the one definition of the host runtime (sdf_runtime.h): last error, spin-then-block waits, the allocation
// hook, the device-block pool and the cache of pinned host blocks.  No kernels.
#include "sdf_runtime.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "../../include/sdf_hip.h"

namespace sdfk {

thread_local std::string g_err;
int fail(const std::string &m) { g_err = m; return 1; }

hipError_t set_device(int device) {
    const hipError_t e = hipSetDevice(device);
    (void)hipGetLastError();
    return e;
}

long g_spin_us = [] { const char *e = getenv("SDF_WAIT_SPIN_US"); return e ? atol(e) : 100000L; }();
template <typename Query, typename Block>
static hipError_t spin_then_block(Query query, Block block) {
    if (g_spin_us > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned n = 0;; n++) {
            const hipError_t e = query();
            if (e != hipErrorNotReady) return e;
            if ((n & 63u) == 63u &&
                std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > g_spin_us)
                break;
            __builtin_ia32_pause();
        }
    }
    return block();
}
hipError_t stream_wait(hipStream_t s) {
    return spin_then_block([&] { return hipStreamQuery(s); }, [&] { return hipStreamSynchronize(s); });
}
hipError_t event_wait(hipEvent_t ev) {
    return spin_then_block([&] { return hipEventQuery(ev); }, [&] { return hipEventSynchronize(ev); });
}

static int g_fail_alloc_in = 0;      // > 0: the g_fail_alloc_in-th allocation from now fails once
static bool g_alloc_hook_hit = false;
static bool alloc_fails_now() { g_alloc_hook_hit = g_fail_alloc_in > 0 && --g_fail_alloc_in == 0; return g_alloc_hook_hit; }
hipError_t dev_malloc(void **p, size_t bytes) { if (alloc_fails_now()) { *p = nullptr; return hipErrorOutOfMemory; } return hipMalloc(p, bytes); }
hipError_t host_malloc(void **p, size_t bytes) { if (alloc_fails_now()) { *p = nullptr; return hipErrorOutOfMemory; } return hipHostMalloc(p, bytes, hipHostMallocDefault); }

const bool g_pool_trace = getenv("SDF_POOL_TRACE") != nullptr;
DevPool g_pool;

void *DevPool::take(size_t need, int device, size_t *got) {
    std::lock_guard<std::mutex> g(mu);
    int best = -1;
    for (int i = 0; i < (int)free_list.size(); i++) {
        const Blk &b = free_list[i];
        if (b.device != device || b.bytes < need || b.bytes > std::max<size_t>(4 * need, 1 << 16)) continue;
        if (best < 0 || b.bytes < free_list[best].bytes) best = i;
    }
    if (best < 0) return nullptr;
    void *p = free_list[best].p;
    *got = free_list[best].bytes;
    free_list.erase(free_list.begin() + best);
    return p;
}
void DevPool::give(void *p, size_t bytes, int device) {
    std::lock_guard<std::mutex> g(mu);
    // (up to eight calls in flight x up to twelve buffers each come back at once: a list shorter than that evicts -- hipFree, a
    // device synchronisation -- blocks the very next call allocates again)
    if (free_list.size() >= 160) {   // evict the oldest block
        if (g_pool_trace) fprintf(stderr, "[sdf pool] evict %zu bytes (hipFree)\n", free_list.front().bytes);
        (void)hipFree(free_list.front().p);
        free_list.erase(free_list.begin());
    }
    free_list.push_back({p, bytes, device});
}
void DevPool::drop_device(int device) {
    std::lock_guard<std::mutex> g(mu);
    for (size_t i = 0; i < free_list.size();) {
        if (free_list[i].device == device) { (void)hipFree(free_list[i].p); free_list.erase(free_list.begin() + i); }
        else i++;
    }
}

int DevBuf::grow(size_t need) {
    release();
    int dev = 0;
    (void)hipGetDevice(&dev);
    const size_t want = align256(std::max(need, (size_t)256));
    size_t got = 0;
    if (void *q = g_pool.take(want, dev, &got)) { p = q; bytes = got; device = dev; return 0; }
    if (g_pool_trace) fprintf(stderr, "[sdf pool] miss %zu bytes (hipMalloc)\n", want);
    hipError_t e = dev_malloc(&p, want);
    if (e != hipSuccess && !g_alloc_hook_hit) {   // give the cached blocks back to the driver and retry once
        g_pool.drop_device(dev);
        e = dev_malloc(&p, want);
    }
    if (e != hipSuccess) { p = nullptr; return fail(std::string("hipMalloc(") + std::to_string(want) + "): " + hipGetErrorString(e)); }
    bytes = want; device = dev;
    return 0;
}

hipError_t mem_fits(size_t bytes, bool *fits, size_t *free_b) {
    size_t total_b = 0;
    const hipError_t e = hipMemGetInfo(free_b, &total_b);
    *fits = e == hipSuccess && bytes <= *free_b / 10 * 9;
    return e;
}

// ---- pinned host memory for results ----
// A device-to-host copy into fresh pageable memory runs at ~10 GB/s (page faults + the runtime's staging);
// into pinned memory it runs at the link rate.  Pinning is expensive (tens of ms for 200 MB), so the
// blocks are recycled: sdf_host_free hands a block back to a small free list, sdf_host_alloc takes the
// smallest block there that is large enough (and not more than twice the request) before pinning new
// memory.  The host side wraps a block as an ndarray whose owner frees it (sdf_amd/engine.py).
struct HostBlock { void *p; size_t bytes; };
static std::mutex g_host_mu;
static std::vector<HostBlock> g_host_free, g_host_live;
static size_t g_host_cached = 0;

}  // namespace sdfk

using namespace sdfk;

extern "C" {

const char *sdf_last_error(void) { return g_err.c_str(); }

int sdf_test_fail_alloc(int nth) { g_fail_alloc_in = nth > 0 ? nth : 0; return 0; }

int sdf_host_alloc(size_t bytes, void **out) {
    if (!out) return fail("sdf_host_alloc: NULL argument");
    *out = nullptr;
    const size_t want = std::max<size_t>((bytes + 4095) & ~(size_t)4095, 4096);
    {
        std::lock_guard<std::mutex> g(g_host_mu);
        int best = -1;
        for (size_t i = 0; i < g_host_free.size(); i++)
            if (g_host_free[i].bytes >= want && g_host_free[i].bytes <= 2 * want &&
                (best < 0 || g_host_free[i].bytes < g_host_free[(size_t)best].bytes))
                best = (int)i;
        if (best >= 0) {
            const HostBlock b = g_host_free[(size_t)best];
            g_host_free.erase(g_host_free.begin() + best);
            g_host_cached -= b.bytes;
            g_host_live.push_back(b);
            *out = b.p;
            return 0;
        }
    }
    void *p = nullptr;
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e != hipSuccess) {   // give the cached blocks back and retry once
        std::vector<HostBlock> drop;
        { std::lock_guard<std::mutex> g(g_host_mu); drop.swap(g_host_free); g_host_cached = 0; }
        for (auto &b : drop) (void)hipHostFree(b.p);
        e = hipHostMalloc(&p, want, hipHostMallocDefault);
    }
    if (e != hipSuccess) return fail(std::string("hipHostMalloc(") + std::to_string(want) + "): " + hipGetErrorString(e));
    std::lock_guard<std::mutex> g(g_host_mu);
    g_host_live.push_back({p, want});
    *out = p;
    return 0;
}

int sdf_host_free(void *p) {
    if (!p) return 0;
    HostBlock b{nullptr, 0};
    std::vector<HostBlock> drop;
    {
        std::lock_guard<std::mutex> g(g_host_mu);
        for (size_t i = 0; i < g_host_live.size(); i++)
            if (g_host_live[i].p == p) { b = g_host_live[i]; g_host_live.erase(g_host_live.begin() + (long)i); break; }
        if (!b.p) return fail("sdf_host_free: not a block of sdf_host_alloc");
        g_host_free.push_back(b);
        g_host_cached += b.bytes;
        // keep at most 8 blocks / 2 GiB cached: the oldest go back to the system
        while (g_host_free.size() > 8 || g_host_cached > ((size_t)2 << 30)) {
            drop.push_back(g_host_free.front());
            g_host_cached -= g_host_free.front().bytes;
            g_host_free.erase(g_host_free.begin());
        }
    }
    for (auto &d : drop) (void)hipHostFree(d.p);
    return 0;
}

}  // extern "C"
