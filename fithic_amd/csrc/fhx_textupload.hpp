// fhx_textupload.hpp - the host side that the device text paths share (fhx_hicpro.hip, fhx_validpairs.hip, fhx_sigselect.hip):
// the handle base with its stream and error text, the device temporaries of one call, the stage clock, and the way a text file
// (fhx_textfile.hpp) reaches HBM: host threads fill one of two pinned buffers while the copy engine drains the other, in batches
// cut at the last newline and padded with blanks as fhx_textlines.hpp's 16-byte loads need it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fithic_mi355x.h"
#include "fhx_textfile.hpp"
#include "fhx_textlines.hpp"

namespace fhx {

// what fhx_hp, fhx_vp and fhx_ms have in common
struct TextHandle {
    int device = -1;
    hipStream_t stream = nullptr;
    std::string err;
    // the upload path: made on first use
    static constexpr size_t kChunk = (size_t)32 << 20;
    void* pinned[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};

    int fail(int code, const std::string& msg) {
        err = msg;
        return code;
    }
};

#define TH_HIP(h, call)                                                                                          \
    do {                                                                                                         \
        hipError_t e_ = (call);                                                                                  \
        if (e_ != hipSuccess) return (h)->fail(FHX_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

// a new H (derived from TextHandle) on `device`, with a non-blocking stream
template <typename H>
int text_handle_create(int device, H** out) {
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
void text_handle_destroy(H* h, Drop drop) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    drop();
    for (int k = 0; k < 2; ++k) {
        if (h->pinned[k]) (void)hipHostFree(h->pinned[k]);
        if (h->ev[k]) (void)hipEventDestroy(h->ev[k]);
    }
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

// device temporaries of one call
struct Scratch {
    std::vector<void*> ptrs;
    ~Scratch() {
        for (void* p : ptrs) (void)hipFree(p);
    }
    template <typename T>
    hipError_t get(T** p, size_t count) {
        hipError_t e = hipMalloc((void**)p, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) ptrs.push_back(*p);
        return e;
    }
    void drop(void* p) {
        auto it = std::find(ptrs.begin(), ptrs.end(), p);
        if (it != ptrs.end()) {
            (void)hipFree(p);
            ptrs.erase(it);
        }
    }
};

// host seconds per stage of a call; the stream is idle at every mark
struct StageClock {
    double* seconds;
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
    void mark(int k) {
        const auto now = std::chrono::steady_clock::now();
        seconds[k] += std::chrono::duration<double>(now - last).count();
        last = now;
    }
};

// the bytes of a batch: the environment variable `env` overrides 256 MB (tests put a batch edge inside a small file), at least
// two lines of the longest kind, at most `upper`, and no more than the text has
inline int64_t batch_bytes_for(const char* env, int64_t upper, int64_t text_bytes) {
    int64_t b = (int64_t)256 << 20;
    if (const char* e = std::getenv(env)) b = std::atoll(e);
    b = std::max<int64_t>(2 * fhxlines::MAX_LINE, std::min<int64_t>(b, upper));
    return std::min(b, std::max<int64_t>(text_bytes, 2 * fhxlines::MAX_LINE));
}

// one batch of a text in HBM
struct TextBatch {
    int64_t len = 0;                              // bytes
    int64_t n_blocks = 0;                         // of fhxlines::BLOCK_BYTES
    bool ends_in_newline = false;
    int64_t lines(unsigned long long newlines) const { return (int64_t)newlines + (ends_in_newline ? 0 : 1); }
};

// Bytes [off, off + len) of the text -> d_text[0, len), len > 0, the stream left idle.  A range that does not reach the end of
// the text ends after its last newline (without one its single line is longer than MAX_LINE, and the path's parse kernel says
// so).  Then blanks up to whole blocks + 64: d_text holds (len + BLOCK_BYTES - 1) / BLOCK_BYTES * BLOCK_BYTES + 64.
// An I/O error reads "reading the <what> file: ...".
inline int upload_batch(TextHandle* h, const TextFile& src, const char* what, int64_t off, int64_t len, unsigned char* d_text,
                        TextBatch* batch) {
    for (int k = 0; k < 2; ++k) {
        if (!h->pinned[k]) TH_HIP(h, hipHostMalloc(&h->pinned[k], TextHandle::kChunk, hipHostMallocDefault));
        if (!h->ev[k]) TH_HIP(h, hipEventCreateWithFlags(&h->ev[k], hipEventDisableTiming));
    }
    bool used[2] = {false, false};
    int turn = 0;
    int64_t last_newline = -1;
    for (int64_t done = 0; done < len; done += (int64_t)TextHandle::kChunk, turn ^= 1) {
        const int64_t now = std::min<int64_t>((int64_t)TextHandle::kChunk, len - done);
        if (used[turn]) TH_HIP(h, hipEventSynchronize(h->ev[turn]));          // the copy engine has drained this buffer
        char* dst = (char*)h->pinned[turn];
        int64_t nl = -1;
        if (const int io_errno = src.read(off + done, now, dst, &nl)) {
            (void)hipStreamSynchronize(h->stream);
            return h->fail(FHX_ERR_ARG, std::string("reading the ") + what + " file: " + std::strerror(io_errno));
        }
        if (nl >= 0) last_newline = done + nl;
        TH_HIP(h, hipMemcpyAsync(d_text + done, dst, (size_t)now, hipMemcpyHostToDevice, h->stream));
        TH_HIP(h, hipEventRecord(h->ev[turn], h->stream));
        used[turn] = true;
    }
    if (off + len < src.size() && last_newline >= 0) len = last_newline + 1;
    batch->len = len;
    batch->n_blocks = (len + fhxlines::BLOCK_BYTES - 1) / fhxlines::BLOCK_BYTES;
    batch->ends_in_newline = last_newline == len - 1;
    TH_HIP(h, hipMemsetAsync(d_text + len, ' ', (size_t)(batch->n_blocks * fhxlines::BLOCK_BYTES + 64 - len), h->stream));
    TH_HIP(h, hipStreamSynchronize(h->stream));                               // the pinned buffers are free again
    return FHX_OK;
}

}  // namespace fhx
