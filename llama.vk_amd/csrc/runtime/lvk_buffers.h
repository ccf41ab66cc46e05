// lvk_buffers.h -- move-only owners of what the runtime takes from HIP: device, page-locked and
// host-mapped allocations, the stream, events, captured graphs, and a scratch list for one-off
// operator calls.  (Buffers from Model::alloc are not owned here: the model's arena frees them.)
#pragma once
#include "lvk_model.h"

#include <memory>
#include <new>
#include <type_traits>

namespace lvk {

struct DevFree { void operator()(void * p) const { (void) hipFree(p); } };
struct HostFree { void operator()(void * p) const { (void) hipHostFree(p); } };
template <class T> using DevPtr = std::unique_ptr<T[], DevFree>;     // hipMalloc
template <class T> using HostPtr = std::unique_ptr<T[], HostFree>;   // hipHostMalloc, page-locked or mapped

// a failed allocation throws `what` (nullptr: HIP's own text) and leaves no sticky error behind
inline void alloc_check(hipError_t e, const char * what) {
    if (e == hipSuccess) return;
    (void) hipGetLastError();
    throw Error(what ? std::string(what) : std::string("llama.vk_amd: allocation failed: ") + hipGetErrorString(e));
}
template <class T> DevPtr<T> dev_alloc(size_t n, const char * what = nullptr) {
    void * p = nullptr;
    alloc_check(hipMalloc(&p, n * sizeof(T)), what);
    return DevPtr<T>((T *) p);
}
template <class T> HostPtr<T> host_alloc(size_t n, unsigned flags, const char * what) {
    void * p = nullptr;
    alloc_check(hipHostMalloc(&p, n * sizeof(T), flags), what);
    return HostPtr<T>((T *) p);
}
template <class T> HostPtr<T> pinned_alloc(size_t n, const char * what = nullptr) {
    return host_alloc<T>(n, hipHostMallocDefault, what);
}
// host memory the device writes straight into (coherent); device_address is the kernels' view of it
template <class T> HostPtr<T> mapped_alloc(size_t n, const char * what = nullptr) {
    return host_alloc<T>(n, hipHostMallocMapped | hipHostMallocCoherent, what);
}
template <class T> T * device_address(const HostPtr<T> & p) {
    T * d = nullptr;
    LVK_HIP(hipHostGetDevicePointer((void **) &d, p.get(), 0));
    return d;
}

// page-locked host storage: the per-token logits D2H copy runs as one DMA instead of
// being staged through a driver bounce buffer
template <class T>
struct PinnedAlloc {
    using value_type = T;
    PinnedAlloc() = default;
    template <class U>
    PinnedAlloc(const PinnedAlloc<U> &) {}
    T * allocate(size_t n) {
        void * p = nullptr;
        if (hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault) != hipSuccess) throw std::bad_alloc();
        return (T *) p;
    }
    void deallocate(T * p, size_t) { HostFree{}(p); }
    template <class U>
    bool operator==(const PinnedAlloc<U> &) const { return true; }
    template <class U>
    bool operator!=(const PinnedAlloc<U> &) const { return false; }
};

struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream & operator=(const Stream &) = delete;
    ~Stream() { if (s) (void) hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};

struct HandleFree {
    void operator()(hipEvent_t e) const { (void) hipEventDestroy(e); }
    void operator()(hipGraph_t g) const { (void) hipGraphDestroy(g); }
    void operator()(hipGraphExec_t g) const { (void) hipGraphExecDestroy(g); }
};
template <class H> using Handle = std::unique_ptr<std::remove_pointer_t<H>, HandleFree>;
using Event = Handle<hipEvent_t>;
inline Event make_event() {
    hipEvent_t e = nullptr;
    LVK_HIP(hipEventCreate(&e));
    return Event(e);
}

// a captured graph and its executable: both or neither
struct Graph {
    Handle<hipGraph_t> graph;
    Handle<hipGraphExec_t> exec;      // declared last: destroyed first
    void reset() { exec.reset(); graph.reset(); }
    explicit operator bool() const { return (bool) exec; }
    hipError_t launch(hipStream_t s) const { return hipGraphLaunch(exec.get(), s); }
};

// g = what fn enqueues on s, captured (thread-local mode) and instantiated.  If fn throws, the
// capture is ended and the partial graph destroyed before the error propagates; if the capture
// or the instantiation fails, g is left empty: nothing leaks and the next call captures afresh.
template <class F> void capture(hipStream_t s, Graph & g, F && fn) {
    g.reset();
    LVK_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    hipGraph_t raw = nullptr;
    try {
        fn();
    } catch (...) {
        (void) hipStreamEndCapture(s, &raw);
        Handle<hipGraph_t> partial(raw);
        throw;
    }
    LVK_HIP(hipStreamEndCapture(s, &raw));
    g.graph.reset(raw);
    hipGraphExec_t exec = nullptr;
    const hipError_t e = hipGraphInstantiate(&exec, raw, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        g.reset();
        LVK_HIP(e);
    }
    g.exec.reset(exec);
}

// device scratch of one operator call: everything handed out is freed when the list goes
struct Scratch {
    std::vector<DevPtr<char>> bufs;
    void * get(size_t n) {
        bufs.push_back(dev_alloc<char>(n ? n : 16));
        return bufs.back().get();
    }
    template <class T> T * up(const T * h, size_t n) {
        T * d = (T *) get(n * sizeof(T));
        LVK_HIP(hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice));
        return d;
    }
};

}  // namespace lvk
