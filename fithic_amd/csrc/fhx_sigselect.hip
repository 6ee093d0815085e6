// fhx_sigselect.hip - the FDR subset of a Fit-Hi-C significances file on MI355X (gfx950)
// (reference: fithic/utils/merge-filter.sh:22, `awk '{if(NR!=1){print $0}}' | awk -v q="$fdr" '{if($7<=q){print $0}}'`).
//
// The text goes through HBM in BATCHES cut at the last newline (two pinned buffers filled by pread, drained by the copy engine:
// fhx_textupload.hpp); only the kept lines come back.  Per batch:
//
//   scan_text, scan_tiles    the newline layer (fhx_textlines.hpp) with this grammar's byte policy: the line number of every
//                  block's first line, and one flag for the batch when a byte outside the grammar is seen (ms_select looks at
//                  bytes one by one only then)
//   ms_select      the lines that begin in a block, one per lane.  One walk along the line (fhx_sigline.hpp) splits it on blanks and finds field 7;
//                  the field is taken only in the shape C's %e writes, D.DDDDDDe[+-]XX[X], and is then
//                    zero     every digit 0: the number 0, kept when 0 <= fdr (0 < fdr when strict) - the host says which
//                    numeric  [2.225074e-308, 9.999999e+307]: awk compares numbers, and strtod is monotone in the integer key
//                             (exponent, 7-digit mantissa): ONE integer compare with the bound the host found by bisection
//                    string   a non-zero value below 2.225074e-308 or an exponent of 309 and more: awk's strtod flags ERANGE and
//                             the field is compared bytewise with the text of fdr (memcmp, then length)
//                  File line 1 is dropped unparsed when skip_first_line is set.  Per line: its kept length (0: dropped); per
//                  block: kept bytes and kept lines.
//   scan_tiles     kept bytes per block -> the block's offset in the subset
//   ms_gather      the kept lines, verbatim and in file order, into a dense buffer: 256 lines per round, their lengths scanned
//                  into LDS, lanes assigned by OUTPUT byte (gather_round: a binary search in the 256 prefixes), so stores are
//                  coalesced at 1 % kept and at 100 %.  A final line without its newline gets one, as awk's print gives it.
//
// The subset of each batch is copied to the host and appended.  The UCSC interact track of the same selection (strict, no line
// skipped) is made by the kernels of fhx_sigtrack.inc, the per-chromosome subsets of merge-filter-parallelized.sh by those of
// fhx_sigsplit.inc, both included at the end of this file.  No device-side strtod, no atomics per line: a refused line
// costs one atomicMin (line << 8 | reason), so the smallest offending line is reported whatever the launch order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fithic_mi355x.h"
#include "fhx_namerule.hpp"
#include "fhx_score.hpp"
#include "fhx_sigkey.hpp"
#include "fhx_sigline.hpp"
#include "fhx_textupload.hpp"
#include "fhx_trackline.hpp"

namespace msd {

using namespace fhxlines;

// the words the kernels of one call share
struct Words {
    unsigned long long first_error;            // smallest (line << 8 | reason)
    unsigned long long kept_bytes;             // scan_tiles' total of the current batch
    unsigned long long kept_lines;             // of the current batch
};

// ---- pass 2: keep or drop every line --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void ms_select(const unsigned char* __restrict__ text, int64_t T, const unsigned long long* __restrict__ block_off,
                                                int64_t n_lines_batch, int64_t line_base, Fdr fdr, unsigned long long key_bound, int zero_kept,
                                                int strict, int skip_first_line, int check_bytes, unsigned short* __restrict__ keep_len,
                                                unsigned int* __restrict__ block_bytes, Words* __restrict__ words) {
    __shared__ unsigned short lstart[LSTART_ENTRIES];
    const BlockLines B = block_lines(text, T, block_off, lstart);
    unsigned int my_bytes = 0, my_lines = 0;
    for (int e = threadIdx.x; e < B.n_lines; e += WG) {
        const int64_t r = B.row0 + e;
        const int64_t start = B.b0 + lstart[e];
        const bool header = skip_first_line && line_base + r == 0;
        Line L;
        walk</*Tokens=*/false>(text, T, start, check_bytes, L);
        int why = L.why;
        bool keep = false;
        if (!why && r >= n_lines_batch) why = FHX_MS_INTERNAL;                // the scan and this kernel disagree about the lines
        if (!why && !header) {
            if (L.tok < 7) why = FHX_MS_TOKENS;
            else {
                unsigned long long key = 0;
                const int cls = classify(text, start + L.fb, L.fn, &key);
                why = decide(cls, key, key_bound, zero_kept, strict, text, start + L.fb, L.fn, fdr, &keep);
            }
        }
        if (why) atomicMin(&words->first_error, error_word(line_base + r + 1, why));
        const unsigned int len = (keep && !why) ? (unsigned int)L.len + 1u : 0u;            // with its newline, present or not
        if (r < n_lines_batch) keep_len[r] = (unsigned short)len;             // at most MAX_LINE + 1
        my_bytes += len;
        my_lines += len ? 1u : 0u;
    }
    unsigned int total_bytes, total_lines;
    fhxscan::block_exclusive_scan(my_bytes, &total_bytes);                    // every lane of the block arrives here
    fhxscan::block_exclusive_scan(my_lines, &total_lines);
    if (threadIdx.x == 0) {
        block_bytes[blockIdx.x] = total_bytes;
        if (total_lines) atomicAdd(&words->kept_lines, (unsigned long long)total_lines);
    }
}

// ---- pass 3: the kept lines, dense and in file order ----------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void ms_gather(const unsigned char* __restrict__ text, int64_t T, const unsigned long long* __restrict__ block_off,
                                                int64_t n_lines_batch, const unsigned short* __restrict__ keep_len,
                                                const unsigned long long* __restrict__ out_off, unsigned char* __restrict__ out, int64_t out_capacity) {
    __shared__ unsigned short lstart[LSTART_ENTRIES];
    __shared__ unsigned int pre[WG + 1];                    // round-local exclusive prefix of the kept lengths; pre[WG] = their sum
    const BlockLines B = block_lines(text, T, block_off, lstart);
    int64_t at = (int64_t)out_off[blockIdx.x];
    for (int base = 0; base < B.n_lines; base += WG) {      // n_lines is the same for every lane: the scan sees whole blocks
        const Round q = round_of(base, B.n_lines, B.row0, n_lines_batch);
        const unsigned int len = q.valid ? (unsigned int)keep_len[q.r] : 0u;
        unsigned int total;
        pre[threadIdx.x] = fhxscan::block_exclusive_scan(len, &total);
        if (threadIdx.x == 0) pre[WG] = total;
        __syncthreads();
        gather_round<WG>(text, T, pre, total, [&](int t) { return B.b0 + lstart[base + t]; }, at, out, out_capacity);
        at += total;
        __syncthreads();                                    // pre is written again in the next round
    }
}

}  // namespace msd

// ===================================================================================================================
struct fhx_ms : fhx::TextHandle {
    // the last selection
    std::vector<char> subset;
    int64_t n_lines = 0, n_kept = 0;
    double seconds[FHX_MS_STAGES] = {0, 0, 0, 0, 0};
    // the last interact track (fhx_sigtrack.inc)
    std::vector<char> track;
    int64_t t_lines = 0, t_kept = 0, t_deferred = 0;
    double t_seconds[FHX_MS_TRACK_STAGES] = {0, 0, 0, 0, 0, 0};
    // the last per-chromosome split (fhx_sigsplit.inc): one entry per name of field 1, in slot order
    struct SplitName {
        std::string name;
        std::vector<char> text;
        int64_t lines = 0;
    };
    std::vector<SplitName> split;
    int64_t s_lines = 0;
    double s_seconds[FHX_MS_SPLIT_STAGES] = {0, 0, 0, 0, 0};
    fhx_ctx* sorter = nullptr;                 // made by the first split call: selections and tracks do not pay for it
};

namespace {

void drop_subset(fhx_ms* ms) {
    std::vector<char>().swap(ms->subset);
    ms->n_lines = ms->n_kept = 0;
}

// the threshold as the kernels take it; `noun` is what the message calls it
int make_fdr(fhx_ms* ms, const char* fdr_text, int32_t fdr_len, const char* noun, msd::Fdr* fdr, int32_t* why) {
    if (msd::fdr_of(fdr_text, fdr_len, fdr)) return FHX_OK;
    *why = FHX_MS_FDR;
    return fhx::fail(ms, FHX_ERR_UNSUPPORTED, std::string("the text of ") + noun + " must have 1 to " + std::to_string(FHX_MS_FDR_BYTES) + " bytes");
}

// fhx_ms_select_file behind its argument check; whatever it returns but FHX_OK, the caller drops the subset
int select_file(fhx_ms* ms, const char* path, const char* fdr_text, int32_t fdr_len, uint64_t key_bound, int32_t zero_kept, int32_t strict,
                int32_t skip_first_line, int64_t* n_bytes, int32_t* why, int64_t* bad_line) {
    using namespace msd;
    TH_HIP(ms, hipSetDevice(ms->device));
    TH_HIP(ms, hipStreamSynchronize(ms->stream));
    drop_subset(ms);
    for (double& s : ms->seconds) s = 0;
    Fdr fdr;
    if (const int rc = make_fdr(ms, fdr_text, fdr_len, "fdr", &fdr, why)) return rc;
    fhx::StageClock clock{ms->seconds};
    fhx::DeviceScratch tmp;
    fhx::TextBatches in;
    if (const int rc = in.open(ms, &tmp, &clock, path, "significances", "FHX_MS_BATCH_BYTES", (int64_t)1 << 31)) return rc;
    const int64_t out_capacity = in.batch_bytes + 1;                          // every line kept, and the newline the last one lacked
    unsigned char* d_out = nullptr;
    unsigned int* d_block_bytes = nullptr;
    unsigned long long* d_out_off = nullptr;
    unsigned short* d_keep_len = nullptr;
    int64_t keep_capacity = 0;
    Words* d_words = nullptr;
    TH_HIP(ms, tmp.get_n(&d_out, (size_t)out_capacity));
    TH_HIP(ms, tmp.get_n(&d_block_bytes, (size_t)in.max_blocks));
    TH_HIP(ms, tmp.get_n(&d_out_off, (size_t)in.max_blocks));
    TH_HIP(ms, tmp.get_n(&d_words, 1));
    Words words;
    const fhx::Refusal refuse{ms, why, bad_line};
    int64_t kept = 0;
    for (; in.more(); in.advance()) {
        std::memset(&words, 0, sizeof(words));
        words.first_error = NO_ERROR;
        TH_HIP(ms, hipMemcpyAsync(d_words, &words, sizeof(words), hipMemcpyHostToDevice, ms->stream));
        if (const int rc = in.next<GrammarBytes>()) return rc;
        const int64_t n = in.lines;
        TH_HIP(ms, tmp.grow(&d_keep_len, &keep_capacity, n));                 // one length per line of the batch
        hipLaunchKernelGGL(ms_select, dim3((unsigned)in.n_blocks), dim3(WG), 0, ms->stream, (const unsigned char*)in.d_text, in.len,
                           (const unsigned long long*)in.d_block_off, n, in.line_base, fdr, (unsigned long long)key_bound, (int)zero_kept,
                           (int)strict, (int)skip_first_line, (int)in.refused_bytes, d_keep_len, d_block_bytes, d_words);
        hipLaunchKernelGGL(fhxscan::scan_tiles, dim3(1), dim3(fhxscan::THREADS), 0, ms->stream, (const unsigned int*)d_block_bytes, in.n_blocks,
                           d_out_off, &d_words->kept_bytes);
        TH_HIP(ms, hipGetLastError());
        TH_HIP(ms, hipMemcpyAsync(&words, d_words, sizeof(words), hipMemcpyDeviceToHost, ms->stream));
        TH_HIP(ms, hipStreamSynchronize(ms->stream));
        clock.mark(2);
        if (words.first_error != NO_ERROR) return refuse.word(words.first_error, FHX_MS_INTERNAL);      // earlier batches hold the smaller line numbers
        const int64_t bytes = (int64_t)words.kept_bytes;
        if (bytes > out_capacity || (int64_t)words.kept_lines > n) return refuse(FHX_ERR_INTERNAL, FHX_MS_INTERNAL, 0, "more kept bytes than text");
        if (bytes > 0) {
            hipLaunchKernelGGL(ms_gather, dim3((unsigned)in.n_blocks), dim3(WG), 0, ms->stream, (const unsigned char*)in.d_text, in.len,
                               (const unsigned long long*)in.d_block_off, n, (const unsigned short*)d_keep_len, (const unsigned long long*)d_out_off,
                               d_out, out_capacity);
            TH_HIP(ms, hipGetLastError());
            TH_HIP(ms, hipStreamSynchronize(ms->stream));
        }
        clock.mark(3);
        if (bytes > 0) {
            const size_t had = ms->subset.size();
            ms->subset.resize(had + (size_t)bytes);
            TH_HIP(ms, hipMemcpyAsync(ms->subset.data() + had, d_out, (size_t)bytes, hipMemcpyDeviceToHost, ms->stream));
            TH_HIP(ms, hipStreamSynchronize(ms->stream));
        }
        clock.mark(4);
        kept += (int64_t)words.kept_lines;
    }
    ms->n_lines = in.line_base;
    ms->n_kept = kept;
    *n_bytes = (int64_t)ms->subset.size();
    if (std::getenv("FHX_TIMING"))
        std::fprintf(stderr, "FDR subset on the device (%s): %lld lines, %lld kept (%lld bytes): read + upload %.6f s; scan %.6f s; select %.6f s; "
                     "gather %.6f s; copy out %.6f s\n", path, (long long)in.line_base, (long long)kept, (long long)ms->subset.size(), ms->seconds[0],
                     ms->seconds[1], ms->seconds[2], ms->seconds[3], ms->seconds[4]);
    return FHX_OK;
}

}  // namespace

extern "C" {

int fhx_ms_create(int device, fhx_ms** out) { return fhx::handle_create(device, out); }

void fhx_ms_destroy(fhx_ms* ms) {
    fhx::text_handle_destroy(ms, [&] {
        if (ms->sorter) fhx_destroy(ms->sorter);
    });
}

const char* fhx_ms_last_error(const fhx_ms* ms) { return fhx::handle_last_error(ms); }

int fhx_ms_select_file(fhx_ms* ms, const char* path, const char* fdr_text, int32_t fdr_len, uint64_t key_bound, int32_t zero_kept, int32_t strict,
                       int32_t skip_first_line, int64_t* n_bytes, int32_t* why, int64_t* bad_line) {
    if (!ms || !path || !fdr_text || !n_bytes || !why || !bad_line) return FHX_ERR_ARG;
    *n_bytes = 0;
    *why = FHX_MS_OK;
    *bad_line = 0;
    const int rc = select_file(ms, path, fdr_text, fdr_len, key_bound, zero_kept, strict, skip_first_line, n_bytes, why, bad_line);
    if (rc != FHX_OK) drop_subset(ms);                                        // the one exit of a failed call, whatever failed
    return rc;
}

int fhx_ms_counts(const fhx_ms* ms, int64_t* n_lines, int64_t* n_kept, int64_t* n_bytes) {
    if (!ms) return FHX_ERR_ARG;
    if (n_lines) *n_lines = ms->n_lines;
    if (n_kept) *n_kept = ms->n_kept;
    if (n_bytes) *n_bytes = (int64_t)ms->subset.size();
    return FHX_OK;
}

int fhx_ms_stage_seconds(const fhx_ms* ms, double* seconds) {
    if (!ms || !seconds) return FHX_ERR_ARG;
    for (int k = 0; k < FHX_MS_STAGES; ++k) seconds[k] = ms->seconds[k];
    return FHX_OK;
}

int fhx_ms_copy_subset(const fhx_ms* ms, void* dst, int64_t capacity) {
    if (!ms || capacity < (int64_t)ms->subset.size() || (!dst && !ms->subset.empty())) return FHX_ERR_ARG;
    if (!ms->subset.empty()) std::memcpy(dst, ms->subset.data(), ms->subset.size());
    return FHX_OK;
}

}  // extern "C"

#include "fhx_sigtrack.inc"
#include "fhx_sigsplit.inc"
