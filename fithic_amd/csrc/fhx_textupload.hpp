// fhx_textupload.hpp - the host side that the device text paths share (fhx_hicpro.hip, fhx_validpairs.hip, fhx_fragpairs.hip,
// fhx_digest.hip, fhx_juicer.hip, fhx_sigselect.hip with fhx_sigtrack.inc and fhx_sigsplit.inc): the text handle (fhx_devmem.hpp's Handle plus the pinned
// upload buffers) and the way a text file (fhx_textfile.hpp) reaches HBM: host threads fill one of two
// pinned buffers while the copy engine drains the other, in batches cut at the last newline and padded with blanks as
// fhx_textlines.hpp's 16-byte loads need it.  TextBatches is the loop over such batches with the newline layer run on each;
// refused_line turns a kernel's error word into what the caller is told.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fithic_mi355x.h"
#include "fhx_devmem.hpp"
#include "fhx_textfile.hpp"
#include "fhx_textlines.hpp"

namespace fhx {

// what fhx_hp, fhx_vp, fhx_fp, fhx_dg, fhx_jc and fhx_ms have in common beyond fhx::Handle: the upload path, made on first use
struct TextHandle : Handle {
    static constexpr size_t kChunk = (size_t)32 << 20;
    void* pinned[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
};

// drop() frees what H (derived from TextHandle) owns beyond it, on the handle's device and with its stream idle
template <typename H, typename Drop>
void text_handle_destroy(H* h, Drop drop) {
    handle_destroy(h, [&] {
        drop();
        for (int k = 0; k < 2; ++k) {
            if (h->pinned[k]) (void)hipHostFree(h->pinned[k]);
            if (h->ev[k]) (void)hipEventDestroy(h->ev[k]);
        }
    });
}

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
            return fail(h, FHX_ERR_ARG, std::string("reading the ") + what + " file: " + std::strerror(io_errno));
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

// A text file, batch by batch, with the newline layer run on every batch:
//
//     fhx::TextBatches in;
//     if (const int rc = in.open(h, &tmp, &clock, path, "dump", "FHX_JC_BATCH_BYTES", upper)) return rc;
//     for (; in.more(); in.advance()) {
//         if (const int rc = in.next<Bytes>()) return rc;
//         ... the path's kernels over in.d_text[0, in.len), in.n_blocks blocks, in.d_block_off, in.lines lines ...
//     }
//
// next() leaves the stream idle and has marked slot 0 of the clock after the upload and slot 1 after the scan.
struct TextBatches {
    TextFile src;                                 // the file itself, or its inflated bytes when it starts with the gzip magic
    int64_t batch_bytes = 0, max_blocks = 0;
    unsigned char* d_text = nullptr;              // max_blocks * BLOCK_BYTES + 64
    unsigned int* d_block_nl = nullptr;
    unsigned long long* d_block_off = nullptr;    // scan_tiles' exclusive scan: what fhxlines::block_lines takes
    // the current batch
    int64_t off = 0;                              // of its first byte in the text
    int64_t line_base = 0;                        // lines of the earlier batches
    int64_t len = 0, n_blocks = 0, lines = 0;
    bool refused_bytes = false;                   // scan_text<Bytes> saw a byte its policy refuses

    int open(TextHandle* handle, DeviceScratch* scratch, StageClock* stage_clock, const char* path, const char* what_word, const char* env,
             int64_t upper) {
        h = handle;
        tmp = scratch;
        clock = stage_clock;
        what = what_word;
        if (const int rc = src.open(path, /*allow_gzip=*/true, &h->err)) return rc;
        batch_bytes = batch_bytes_for(env, upper, src.size());
        max_blocks = (batch_bytes + fhxlines::BLOCK_BYTES - 1) / fhxlines::BLOCK_BYTES;
        TH_HIP(h, tmp->get_n(&d_text, (size_t)max_blocks * fhxlines::BLOCK_BYTES + 64));
        TH_HIP(h, tmp->get_n(&d_block_nl, (size_t)max_blocks));
        TH_HIP(h, tmp->get_n(&d_block_off, (size_t)max_blocks));
        TH_HIP(h, tmp->get_n(&d_scan, 1));
        return FHX_OK;
    }

    bool more() const { return off < src.size(); }

    template <typename Bytes>
    int next() {
        TH_HIP(h, hipMemsetAsync(d_scan, 0, sizeof(ScanWords), h->stream));
        TextBatch b;
        if (const int rc = upload_batch(h, src, what, off, std::min(batch_bytes, src.size() - off), d_text, &b)) return rc;
        len = b.len;
        n_blocks = b.n_blocks;
        clock->mark(0);
        hipLaunchKernelGGL(fhxlines::scan_text<Bytes>, dim3((unsigned)n_blocks), dim3(fhxlines::WG), 0, h->stream, (const unsigned char*)d_text, len,
                           d_block_nl, &d_scan->flags);
        hipLaunchKernelGGL(fhxscan::scan_tiles, dim3(1), dim3(fhxscan::THREADS), 0, h->stream, (const unsigned int*)d_block_nl, n_blocks, d_block_off,
                           &d_scan->newlines);
        TH_HIP(h, hipGetLastError());
        ScanWords scan;
        TH_HIP(h, hipMemcpyAsync(&scan, d_scan, sizeof(scan), hipMemcpyDeviceToHost, h->stream));
        TH_HIP(h, hipStreamSynchronize(h->stream));
        clock->mark(1);
        lines = b.lines(scan.newlines);
        refused_bytes = scan.flags != 0;
        return FHX_OK;
    }

    void advance() {
        off += len;
        line_base += lines;
    }

    // after the last batch: the text leaves HBM and the inflated bytes leave the host
    void close() {
        tmp->drop(d_text);
        d_text = nullptr;
        src.release();
    }

  private:
    struct ScanWords {
        unsigned long long newlines;              // scan_tiles' total
        unsigned int flags, pad;                  // scan_text's flag word
    };
    TextHandle* h = nullptr;
    DeviceScratch* tmp = nullptr;
    StageClock* clock = nullptr;
    const char* what = "";
    ScanWords* d_scan = nullptr;
};

// Where a refusal of a call goes: the caller's why / bad_line (fhx_coarsen.hip: bad row), the handle's message, and the code
// to return.
struct Refusal {
    Handle* h;
    int32_t* why;
    int64_t* bad_line;
    int operator()(int rc, int32_t w, int64_t line, const std::string& msg) const {
        *why = w;
        *bad_line = line;
        return fail(h, rc, msg);
    }
    // a kernel's first_error word (fhxlines::error_word); `internal` is the path's reason for kernels that disagree with each other
    int word(unsigned long long first_error, int32_t internal) const {
        const int32_t w = fhxlines::error_why(first_error);
        const int64_t line = fhxlines::error_line(first_error);
        if (w == internal) return (*this)(FHX_ERR_INTERNAL, w, line, "the kernels of the call disagree about line " + std::to_string(line));
        return (*this)(FHX_ERR_UNSUPPORTED, w, line, "line " + std::to_string(line) + " is outside the device grammar (reason " + std::to_string(w) + ")");
    }
};

}  // namespace fhx
