// sdf_runtime.h -- the host runtime every translation unit of libsdf_hip.so shares (defined once, in sdf_runtime.hip): the last-error
// slot behind sdf_last_error, waiting without going to sleep, the allocation hook of the tests, the pool of device blocks, and the
// small tools of a feature call -- a scratch block (Scratch), the owner of a block the call leaves behind (DevBlock), the checked
// launch of a 256-lane kernel (launch_rows, launch_grid), the memory guard, an event-pair timer (EventTimer).  The fifth tool of a
// reader unit, number_flags, has device code behind it and lives in sdf_prims.h; what the readers' KERNELS share -- box keys, a
// workgroup's sums and boxes, the float64 tree -- is sdf_block.h, for units of flag class `plain` only.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

namespace sdfk {

// ---- errors: the message goes into this thread's slot (sdf_last_error reads it), the call returns 1 ----
extern thread_local std::string g_err;
int fail(const std::string &m);
// a failed HIP call ends the function; what it holds goes back through destructors (DevBuf's owners, Scratch, DevBlock, EventTimer)
#define HIPCHK_MSG(prefix, x)                                                                       \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) return sdfk::fail(std::string(prefix) + hipGetErrorString(e_));       \
    } while (0)
#define HIPCHK(x) HIPCHK_MSG(#x ": ", x)
#define HIPCHK_FN(x) HIPCHK_MSG(std::string(__func__) + ": " #x ": ", x)   // ... named after the entry point it is in

// Entering the library: select the context's device and DROP whatever error another library left in this thread's
// "last error" slot (hipGetLastError is sticky per thread: a failed probe inside RCCL or torch -- seen after
// destroy_process_group: "invalid device ordinal" -- would otherwise be reported by our next launch check)
hipError_t set_device(int device);

// Waiting for the device WITHOUT going to sleep.  hipStreamSynchronize / hipEventSynchronize block on an interrupt
// after a short active wait; on a virtualised host the wake-up costs milliseconds (BENCH_r02: a synchronous 512^3 call
// took 2.2 ms on the driver's box against 0.4 ms of device work).  The calls of this library last 0.3 - 40 ms, so the
// host polls the completion signal (hipStreamQuery / hipEventQuery read it directly) for up to g_spin_us microseconds
// and only then falls back to the blocking wait.  SDF_WAIT_SPIN_US=0 restores the blocking behaviour.
extern long g_spin_us;
hipError_t stream_wait(hipStream_t s);
hipError_t event_wait(hipEvent_t ev);

// Every allocation of the library goes through these two, so that the tests can make the n-th one fail
// (sdf_test_fail_alloc) and check that every error path hands back what it had taken.
hipError_t dev_malloc(void **p, size_t bytes);
hipError_t host_malloc(void **p, size_t bytes);

// Device allocations are recycled through a small per-device free list: hipMalloc / hipFree cost
// tens of microseconds each (and hipFree synchronises), which at ~1 ms per generate call was 10 %
// of the step when every mesh allocated and freed its seven buffers.
extern const bool g_pool_trace;   // SDF_POOL_TRACE: every hipMalloc / hipFree behind the pool, to stderr
struct DevPool {
    struct Blk { void *p; size_t bytes; int device; };
    std::vector<Blk> free_list;
    std::mutex mu;
    void *take(size_t need, int device, size_t *got);
    void give(void *p, size_t bytes, int device);
    void drop_device(int device);
};
extern DevPool g_pool;

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    int device = -1;
    int ensure(size_t need) { return need <= bytes ? 0 : grow(need); }
    int grow(size_t need);
    void release() { if (p) g_pool.give(p, bytes, device); p = nullptr; bytes = 0; }
};

static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// The device scratch of ONE call: a single hooked allocation, not pooled, carved into 256-byte-aligned parts.  part() names every
// part once -- `bytes` is then the size to ask the memory guard about -- and alloc() sets the pointers.  The block is freed when
// the call leaves, on every path, after the stream that worked in it has drained.
struct Scratch {
    explicit Scratch(hipStream_t st) : stream(st) {}
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch() { if (base) { (void)stream_wait(stream); (void)hipFree(base); } }
    template <typename T> void part(T **p, size_t count) {
        parts.push_back({reinterpret_cast<void **>(p), bytes});
        bytes += align256(count * sizeof(T));
    }
    hipError_t alloc() {
        const hipError_t e = dev_malloc((void **)&base, bytes);
        for (size_t k = 0; k < parts.size() && e == hipSuccess; k++) *parts[k].p = base + parts[k].off;
        return e;
    }
    size_t bytes = 0;
private:
    struct Part { void **p; size_t off; };
    std::vector<Part> parts;
    char *base = nullptr;
    hipStream_t stream;
};

// A device block that OUTLIVES the call that made it (the weld, the normals and the shells a mesh keeps): one hooked allocation, not
// pooled, move-only.  It is freed with its owner or by reset(), after the stream that worked in it has drained -- so a producer
// fills a local DevBlock and moves it out only when it has succeeded, and every other path hands the block back.
struct DevBlock {
    DevBlock() = default;
    DevBlock(DevBlock &&o) noexcept : p(o.p), stream(o.stream) { o.p = nullptr; }
    DevBlock &operator=(DevBlock &&o) noexcept {
        if (this != &o) { reset(); p = o.p; stream = o.stream; o.p = nullptr; }
        return *this;
    }
    ~DevBlock() { reset(); }
    hipError_t alloc(size_t bytes, hipStream_t st) { reset(); stream = st; return dev_malloc(&p, bytes); }
    void reset() { if (p) { (void)stream_wait(stream); (void)hipFree(p); p = nullptr; } }
    template <typename T> T *as() const { return static_cast<T *>(p); }
    explicit operator bool() const { return p != nullptr; }
private:
    void *p = nullptr;
    hipStream_t stream = nullptr;
};

// The launch of a kernel of 256-lane workgroups, checked: HIPCHK_MSG(who, launch_rows(k_x, n, st, ...)).  launch_rows gives each of n
// rows a lane and launches nothing when there are none; launch_grid takes the grid as it is (a capped grid whose workgroups stride).
// The arguments are converted to the kernel's parameter types, so a pointer to const or a nullptr needs no cast where it is passed.
static inline unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }
template <typename... P, typename... A>
hipError_t launch_grid(void (*kernel)(P...), unsigned grid, hipStream_t st, A &&...args) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, st, static_cast<P>(args)...);
    return hipGetLastError();
}
template <typename... P, typename... A>
hipError_t launch_rows(void (*kernel)(P...), long long n, hipStream_t st, A &&...args) {
    return n < 1 ? hipSuccess : launch_grid(kernel, blocks_of(n), st, static_cast<A &&>(args)...);
}

// the memory guard of the calls that size their scratch from their arguments: do `bytes` fit in 90 % of what is free now?
// (*free_b: for the caller's message)
hipError_t mem_fits(size_t bytes, bool *fits, size_t *free_b);

// a pair of events around device work on one stream: start(), the work, stop(), and ms() once the stream has been waited for
struct EventTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventTimer() = default;
    EventTimer(const EventTimer &) = delete;
    EventTimer &operator=(const EventTimer &) = delete;
    ~EventTimer() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    hipError_t start(hipStream_t st) {
        hipError_t e = hipEventCreate(&e0);
        if (e == hipSuccess) e = hipEventCreate(&e1);
        return e == hipSuccess ? hipEventRecord(e0, st) : e;
    }
    hipError_t stop(hipStream_t st) { return hipEventRecord(e1, st); }
    hipError_t ms(double *out) {
        float f = 0.f;
        const hipError_t e = hipEventElapsedTime(&f, e0, e1);
        if (e == hipSuccess) *out = (double)f;
        return e;
    }
};

}  // namespace sdfk
