// Host-side runtime layer shared by the library's modules: the error path, the device check, the handle stream that carries out
// the stream rule of include/orbx.h ("Streams and threads"), grow-only buffers, the workspace lease pool and the phase tracer.
// Internal: everything here is a macro, a class or inline inside an anonymous namespace, so it adds no exported symbol.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/orbx.h"

// orbx_api.hip owns the thread-local text behind orbx_last_error(); returns `code`
int orbx_set_error(int code, const std::string &msg);

// More than 64 KB of dynamic LDS has to be requested per kernel AND per device (the attribute belongs to the device's code
// object).  orbx_lds_opt_in (orbx_api.hip) keeps the largest size configured so far per (kernel, device of the calling thread)
// under a mutex, raises it when `bytes` is larger, and returns the runtime's answer -- a handle on a second GPU of the process
// gets its own opt-in, and a failed one is reported instead of being found out by a launch error later.
hipError_t orbx_lds_opt_in(const void *kernel, size_t bytes);

// a failed HIP call returns ORBX_E_NO_DEVICE from the entry point, naming the call
#define ORB_TRY(expr)                                                                                                   \
    do {                                                                                                                \
        hipError_t e_ = (expr);                                                                                         \
        if (e_ != hipSuccess) return orbx_set_error(ORBX_E_NO_DEVICE, std::string(#expr ": ") + hipGetErrorString(e_)); \
    } while (0)

// launches `grid` workgroups of a kernel that ends in flush_counts (orb_device.h), or in its like; eight zeros first unless exactly one
// workgroup writes them
#define LAUNCH_COUNTED(kernel, grid, threads, s, result, ...)                                           \
    do {                                                                                                \
        if ((grid) != 1) hipLaunchKernelGGL(k_counters_clear<>, dim3(1), dim3(64), 0, s, result);       \
        if ((grid) > 0) hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), 0, s, __VA_ARGS__);       \
        ORB_TRY(hipGetLastError());                                                                     \
    } while (0)

namespace {

// Fails without a HIP device.  With `device`, also resolves a handle's ordinal: < 0 is the calling thread's current device.
inline int orb_need_device(int *device = nullptr)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1)
        return orbx_set_error(ORBX_E_NO_DEVICE, "no HIP device available (this library has no CPU path)");
    if (!device) return ORBX_OK;
    if (*device < 0 && hipGetDevice(device) != hipSuccess) *device = 0;
    if (*device >= n) return orbx_set_error(ORBX_E_ARG, "device ordinal out of range");
    return ORBX_OK;
}

// A handle's device, its own stream and the one coupling the library adds to stream 0 (include/orbx.h, "Streams and threads").
// The stream serves the host-pointer entry points only and is NON-BLOCKING: such a call uploads, computes, downloads and waits
// on it, so nothing of it is ordered with the legacy stream or with another thread's handle.  A handle whose host-pointer calls
// lease streams of their own (orbv) never calls create().
struct HandleStream {
    int device = 0;
    hipStream_t stream = nullptr;
    bool null_pending = false; // a device call was enqueued on stream 0 (NULL) since the last host-side wait
    hipError_t create() { return hipStreamCreateWithFlags(&stream, hipStreamNonBlocking); }
    // start of a host-pointer call: NULL-stream device calls of this handle may still be using its scratch
    hipError_t host_call()
    {
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess && null_pending) { e = hipStreamSynchronize((hipStream_t)0); null_pending = false; }
        return e;
    }
    // a device entry point enqueues on `s`; NULL is stream 0 itself, which the next host call and destroy() wait for
    hipError_t device_call(hipStream_t s)
    {
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess && !s) null_pending = true;
        return e;
    }
    // everything the handle enqueued has finished; the calling thread stays on the handle's device
    void destroy()
    {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        if (null_pending) (void)hipStreamSynchronize((hipStream_t)0);
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr;
        null_pending = false;
    }
};

// Grow-only device (PINNED = false) or page-locked host (true) block, owned: the destructor frees it and a copy does not
// compile.  need() keeps the block when `bytes` fit and otherwise replaces it with one of `alloc` bytes (a pinned one with
// hipHostMalloc's `flags`): the growth policy is the caller's, and so is the wait for whatever may still use the old block.
// Never in an object of static storage duration: its destructor would run after the HIP runtime is gone (orbba.hip, g_work).
template <bool PINNED> struct GrowBuf {
    void *p = nullptr;
    size_t cap = 0;
    GrowBuf() = default;
    GrowBuf(const GrowBuf &) = delete;
    GrowBuf &operator=(const GrowBuf &) = delete;
    ~GrowBuf() { release(); }
    hipError_t need(size_t bytes, size_t alloc, unsigned flags = hipHostMallocDefault)
    {
        if (bytes <= cap) return hipSuccess;
        release();
        hipError_t e = PINNED ? hipHostMalloc(&p, alloc, flags) : hipMalloc(&p, alloc);
        if (e == hipSuccess) cap = alloc; else p = nullptr;
        return e;
    }
    void release()
    {
        if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
    template <typename T> T *as() const { return static_cast<T *>(p); }
};
typedef GrowBuf<false> DevBuf;
typedef GrowBuf<true> PinBuf;

// Workspaces (a non-blocking stream and scratch, W::init() makes them) of the calls that must not share a stream or scratch:
// the handle-less BA entry points and orbv_transform on a shared vocabulary.  A call leases one of its device for its duration;
// when the lease returns, the stream the call ran on is synchronised first -- an error return may leave work in flight, and the
// next lessee must not meet it.  That stream is the workspace's own unless the call sets `stream` to another behind acquire(): a
// device-pointer call that borrows the scratch but enqueues on its caller's stream.  The pool never frees a workspace; its owner
// does, if at all.
template <typename W> struct LeasePool {
    std::mutex mu;
    std::vector<W *> idle;
};
template <typename W> struct Lease {
    LeasePool<W> &pool;
    W *w = nullptr;
    hipStream_t stream = nullptr; // the stream the call runs on
    explicit Lease(LeasePool<W> &p) : pool(p) {}
    Lease(const Lease &) = delete;
    Lease &operator=(const Lease &) = delete;
    ~Lease()
    {
        if (!w) return;
        (void)hipStreamSynchronize(stream);
        std::lock_guard<std::mutex> lock(pool.mu);
        pool.idle.push_back(w);
    }
    hipError_t acquire(int device)
    {
        {
            std::lock_guard<std::mutex> lock(pool.mu);
            for (size_t i = pool.idle.size(); i-- > 0;)
                if (pool.idle[i]->device == device) {
                    w = pool.idle[i];
                    stream = w->stream;
                    pool.idle.erase(pool.idle.begin() + (long)i);
                    return hipSuccess;
                }
        }
        W *n = new W();
        n->device = device;
        hipError_t e = n->init();
        if (e != hipSuccess) { delete n; return e; }
        w = n;
        stream = w->stream;
        return hipSuccess;
    }
};

// host time stamps of the phases of a call on stderr, when the environment variable `env` is set
struct PhaseTrace {
    const char *tag;
    bool on;
    std::chrono::steady_clock::time_point t0;
    PhaseTrace(const char *tag_, const char *env) : tag(tag_), on(getenv(env) != nullptr), t0(std::chrono::steady_clock::now()) {}
    void mark(const char *what)
    {
        if (!on) return;
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[%s] %-24s %8.1f us\n", tag, what, std::chrono::duration<double, std::micro>(t - t0).count());
        t0 = t;
    }
};

} // namespace
