// fhx_devmem.hpp - how the host code owns device memory, and what every handle behind the C ABI has in common.  The only file
// of the library that calls hipMalloc or hipFree.
//
//   dev_malloc / dev_free   the two doors; they count the live blocks and bytes of the process (fhx_debug_device_blocks)
//   raw members             a handle's long-lived blocks stay plain pointers: dev_malloc'ed where they are sized, dev_free'd
//                           (which nulls them) where they are replaced and in the handle's destroy
//   DeviceScratch           the blocks of one call: freed on every return path, or earlier with drop(); grow() for an array
//                           sized per batch, grow_keep() for one that accumulates over the batches
//   GrowBuf<T>              a handle's grow-only buffer: steady-state calls allocate nothing
//   Handle                  device, stream, error text; FHX_HIP_ON / fail() store the message and return the code
//   StageClock              host seconds per stage of a call
//   upload<T>               a host table -> one of a handle's long-lived blocks
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <mutex>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/fithic_mi355x.h"

namespace fhx {

// ---- errors ----------------------------------------------------------------------------------------------------------------
// store the message in whatever handle has an `err`, return the code
template <typename H>
inline auto fail(H* h, int code, const std::string& msg) -> decltype((void)h->err, int()) {
    if (h) h->err = msg;
    return code;
}

#define FHX_HIP_ON(h, call)                                                                                         \
    do {                                                                                                            \
        hipError_t e_ = (call);                                                                                     \
        if (e_ != hipSuccess) return fhx::fail(h, FHX_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)
// the handle each group of entry points names by convention
#define FHX_HIP(call) FHX_HIP_ON(ctx, call)
#define KR_HIP(call) FHX_HIP_ON(kr, call)
#define CN_HIP(call) FHX_HIP_ON(cn, call)
#define TH_HIP(h, call) FHX_HIP_ON(h, call)

// ---- the two doors ---------------------------------------------------------------------------------------------------------
// Live device blocks and bytes of the process.  Atomic: the side workers and the emit drainer allocate beside the calling
// thread.  dev_free is not told a block's size, so the sizes are kept here (never destroyed: handles may outlive statics).
struct DevLive {
    std::atomic<int64_t> blocks{0}, bytes{0};
    std::mutex mu;
    std::unordered_map<const void*, size_t> size_of;
};
inline DevLive& dev_live() {
    static DevLive* live = new DevLive();
    return *live;
}

template <typename T>
inline hipError_t dev_malloc(T** p, size_t bytes) {
    const hipError_t e = hipMalloc((void**)p, bytes);
    if (e == hipSuccess && *p) {
        DevLive& live = dev_live();
        {
            std::lock_guard<std::mutex> g(live.mu);
            live.size_of[(const void*)*p] = bytes;
        }
        live.blocks += 1;
        live.bytes += (int64_t)bytes;
    }
    return e;
}

// free and null
template <typename T>
inline void dev_free(T*& p) {
    if (p) {
        DevLive& live = dev_live();
        size_t bytes = 0;
        {
            std::lock_guard<std::mutex> g(live.mu);
            const auto it = live.size_of.find((const void*)p);
            if (it != live.size_of.end()) {
                bytes = it->second;
                live.size_of.erase(it);
            }
        }
        live.blocks -= 1;
        live.bytes -= (int64_t)bytes;
        (void)hipFree((void*)p);
    }
    p = nullptr;
}

// ---- the blocks of one call ------------------------------------------------------------------------------------------------
// Device blocks kept between the batches of one call: allocating and freeing GBs per batch stalls behind the other thread's
// hipFree (a batch of the device writer waited up to 0.5 s in its allocations); a block goes back here instead and the next
// batch, which asks for the same sizes in the same order, takes it again.  Freed when the pool goes out of scope.
struct ScratchPool {
    std::mutex mu;
    std::vector<std::pair<void*, size_t>> idle;
    ~ScratchPool() {
        for (auto& b : idle) dev_free(b.first);
    }
    void* take(size_t bytes, size_t* real) {           // the smallest idle block that is large enough, or nullptr
        std::lock_guard<std::mutex> g(mu);
        size_t best = idle.size();
        for (size_t i = 0; i < idle.size(); ++i)
            if (idle[i].second >= bytes && (best == idle.size() || idle[i].second < idle[best].second)) best = i;
        if (best == idle.size()) return nullptr;
        void* p = idle[best].first;
        *real = idle[best].second;
        idle.erase(idle.begin() + (long)best);
        return p;
    }
    void give(void* p, size_t bytes) {
        std::lock_guard<std::mutex> g(mu);
        idle.emplace_back(p, bytes);
    }
};

// temporary device allocations of one call: freed on every return path (the *_HIP macros return early on errors)
struct DeviceScratch {
    std::vector<std::pair<void*, size_t>> v;
    ScratchPool* pool = nullptr;                       // where the blocks go at the end instead of being freed
    DeviceScratch() = default;
    explicit DeviceScratch(ScratchPool* p) : pool(p) {}
    DeviceScratch(const DeviceScratch&) = delete;
    DeviceScratch& operator=(const DeviceScratch&) = delete;
    ~DeviceScratch() {
        for (auto& b : v) release(b);
    }
    template <typename T>
    hipError_t get(T** p, size_t bytes) {
        bytes = std::max<size_t>(bytes, 16);
        if (pool) {
            size_t real = 0;
            if (void* q = pool->take(bytes, &real)) {
                *p = (T*)q;
                v.emplace_back(q, real);
                return hipSuccess;
            }
        }
        const hipError_t e = dev_malloc(p, bytes);
        if (e == hipSuccess) v.emplace_back((void*)*p, bytes);
        return e;
    }
    template <typename T>
    hipError_t get_n(T** p, size_t count) {            // `count` elements of T
        return get(p, count * sizeof(T));
    }
    // a block that is done before the call is: peak memory depends on it
    void drop(void* p) {
        for (size_t i = 0; i < v.size(); ++i)
            if (v[i].first == p) {
                release(v[i]);
                v.erase(v.begin() + (long)i);
                return;
            }
    }
    // an array that grows to what a batch needs; its old contents are not kept
    template <typename T>
    hipError_t grow(T** p, int64_t* capacity, int64_t need) {
        if (need <= *capacity) return hipSuccess;
        if (*p) drop(*p);
        *p = nullptr;
        *capacity = 0;
        const hipError_t e = get_n(p, (size_t)need);
        if (e == hipSuccess) *capacity = need;
        return e;
    }
    // an array that grows to `need` elements and KEEPS its first `used` ones (at least doubling, so that a file of many batches
    // moves its records a logarithmic number of times); the stream is idle afterwards
    template <typename T>
    hipError_t grow_keep(T** p, int64_t* capacity, int64_t used, int64_t need, hipStream_t stream) {
        if (need <= *capacity) return hipSuccess;
        const int64_t want = std::max<int64_t>(need, *capacity * 2);
        T* bigger = nullptr;
        hipError_t e = get_n(&bigger, (size_t)want);
        if (e == hipSuccess && used > 0) e = hipMemcpyAsync(bigger, *p, (size_t)used * sizeof(T), hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return e;                 // `bigger` goes with the call's other blocks
        if (*p) drop(*p);
        *p = bigger;
        *capacity = want;
        return hipSuccess;
    }

  private:
    void release(std::pair<void*, size_t>& b) {
        if (pool)
            pool->give(b.first, b.second);
        else
            dev_free(b.first);
    }
};

// ---- a handle's grow-only buffer -------------------------------------------------------------------------------------------
// need(n) leaves room for at least n elements, old contents not kept.  `exact`: cap is n itself (fhx_kr strides by cap);
// otherwise an eighth of slack, so that sizes that creep up from pass to pass do not reallocate every time.
template <typename T>
struct GrowBuf {
    T* p = nullptr;
    size_t cap = 0;
    GrowBuf() = default;
    GrowBuf(const GrowBuf&) = delete;
    GrowBuf& operator=(const GrowBuf&) = delete;
    ~GrowBuf() { release(); }                          // every owner is deleted on its device, in its destroy
    hipError_t need(size_t n, bool exact = false) {
        if (n <= cap) return hipSuccess;
        release();
        const size_t want = exact ? n : n + n / 8 + 64;
        const hipError_t e = dev_malloc(&p, want * sizeof(T));
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        dev_free(p);
        cap = 0;
    }
};

// ---- what every handle but the engine's has in common ----------------------------------------------------------------------
struct Handle {
    int device = -1;
    hipStream_t stream = nullptr;
    std::string err;
};

// a new H (derived from Handle) on `device`, with a non-blocking stream; what H owns beyond that is made by the caller, who
// destroys the handle if that fails
template <typename H>
int handle_create(int device, H** out) {
    if (!out) return FHX_ERR_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return FHX_ERR_NO_DEVICE;
    H* h = new H();
    h->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return FHX_ERR_HIP;
    }
    *out = h;
    return FHX_OK;
}

// drop() frees what H owns beyond the base, on the handle's device and with its stream idle
template <typename H, typename Drop>
void handle_destroy(H* h, Drop drop) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    drop();
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

inline const char* handle_last_error(const Handle* h) { return h ? h->err.c_str() : "null context"; }

// host seconds per stage of a call (FHX_TIMING, the *_stage_seconds entry points); the stream is idle at every mark
struct StageClock {
    double* seconds;
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
    void mark(int k) {
        const auto now = std::chrono::steady_clock::now();
        seconds[k] += std::chrono::duration<double>(now - last).count();
        last = now;
    }
};

// a host table of n elements as one of the handle's long-lived blocks (at least one element is allocated); the copy is in
// flight on the handle's stream when this returns
template <typename H, typename T>
int upload(H* h, T** d, const T* src, size_t n) {
    FHX_HIP_ON(h, dev_malloc(d, std::max<size_t>(n, 1) * sizeof(T)));
    if (n) FHX_HIP_ON(h, hipMemcpyAsync(*d, src, n * sizeof(T), hipMemcpyHostToDevice, h->stream));
    return FHX_OK;
}

}  // namespace fhx
