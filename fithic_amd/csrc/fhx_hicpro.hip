// fhx_hicpro.hip - a HiC-Pro `.matrix` turned into Fit-Hi-C's contact columns and per-bin totals on MI355X (gfx950)
// (reference: fithic/utils/HiCPro2FitHiC.py:33-53, the per-line loop).
//
// The reference walks the matrix in Python: `i, j, cc = line.split()`, two dict lookups, `fragDic[i][3] += cc;
// fragDic[j][3] += cc`, five str() and a gzip write per line.  Here the file goes to HBM as it is (two pinned buffers filled
// by pread, drained by the copy engine: fhx_textupload.hpp) and kernels do everything that is per line:
//
// The five columns of the result are an fhx::CellColumns (fhx_cells.hpp).
//
//   scan_text, scan_tiles    the newline layer (fhx_textlines.hpp) with the text-mode byte policy: the row number of every
//                  block's first line, and a flag for NUL, non-ASCII and a \r that is not followed by \n
//   hp_parse       the lines that begin in a block, one per lane: three tokens, (chr, mid) of i and j gathered from the dense
//                  bin table (8 B per index, L2-resident), five int32 columns stored coalesced in file order, the count added
//                  to the totals of bin i and of bin j (a diagonal line `i i c` adds 2c, :40-41) as 64-bit INTEGER atomics:
//                  exact, so the order of the additions does not matter.  A HiC-Pro matrix is sorted by i, so a wave's 64
//                  lines mostly share one i: runs of equal bins are summed inside the wave first (ballot of the run heads +
//                  segmented shuffle) and each run posts one atomic - without that every lane of the chip hits one address.
//   hp_max_total   the largest total: at 2^53 or more the reference's float sum would have rounded
//
// ONLY THE REGULAR FILE IS TAKEN: ASCII, exactly three tokens per line (separated by str.split()'s ASCII blanks), i and j =
// [+-]?digits (at most 10 digits, within int32), count = digits[.digits] (at most 15 digits, integer part within int32) whose
// fraction digits are all 0 - the reference prints such a count as the integer (:42).  \r\n line ends and a last line without a
// newline are fine.  Everything else is REFUSED with the smallest offending line number (one 64-bit word, atomicMin: the same
// answer whatever the launch order) and a reason; nothing stays loaded.  No line is ever parsed "approximately".
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/fithic_mi355x.h"
#include "fhx_cells.hpp"

namespace hpd {

using namespace fhxlines;

constexpr unsigned long long TOTAL_LIMIT = 1ull << 53;

__device__ inline bool is_space(int c) { return c == ' ' || (c >= '\t' && c <= '\r') || (c >= 0x1c && c <= 0x1f); }

// one lane's walk along its line; `why` keeps the first thing that was wrong with it
struct Cursor {
    const unsigned char* text;
    int64_t T, p, limit;
    int why;
    __device__ int at() const { return p < T ? (int)text[p] : '\n'; }          // the end of the text ends the line
    __device__ bool fail(int w) {
        if (!why) why = w;
        return false;
    }
    // to the next token of the line; false at the end of the line
    __device__ bool next_token() {
        for (;;) {
            const int c = at();
            if (c == '\n') return false;
            if (p >= limit) return fail(FHX_HP_LONG_LINE);
            if (!is_space(c)) return true;
            if (c == '\r' && (p + 1 >= T || text[p + 1] != '\n')) return fail(FHX_HP_BYTES);
            ++p;
        }
    }
    // a token ended where it should not: say whether by a byte no line of this path may hold
    __device__ bool bad_token(int c, int w) { return fail(c == 0 || c >= 0x80 ? FHX_HP_BYTES : w); }
    // int(text) of [+-]?digits: at most 10 digits, within int32
    __device__ bool integer(long long* out) {
        int c = at();
        bool neg = false;
        if (c == '+' || c == '-') {
            neg = c == '-';
            ++p;
        }
        long long v = 0;
        int nd = 0;
        for (;;) {
            c = at();
            if (c < '0' || c > '9') break;
            if (++nd > 10) return fail(FHX_HP_INDEX);
            v = v * 10 + (c - '0');
            ++p;
        }
        if (nd == 0 || !is_space(c)) return bad_token(c, FHX_HP_INDEX);       // "1_000", "1.0", "1e3", "0x10"
        if (neg) v = -v;
        if (v < -2147483648ll || v > 2147483647ll) return fail(FHX_HP_INDEX);
        *out = v;
        return true;
    }
    // float(text) of digits[.digits] (either side of the point may be empty, not both), every fraction digit 0: the value is
    // the integer part as written, the reference prints it with str(int(cc)).  Signs, exponents, underscores, inf/nan and a
    // fraction that is not zero are refused.
    __device__ bool count(int* out) {
        long long v = 0;
        int ni = 0, nf = 0, c;
        bool frac = false;
        for (;;) {
            c = at();
            if (c < '0' || c > '9') break;
            if (++ni > 10) return fail(FHX_HP_COUNT);
            v = v * 10 + (c - '0');
            ++p;
        }
        if (c == '.') {
            ++p;
            for (;;) {
                c = at();
                if (c < '0' || c > '9') break;
                if (++nf > 15) return fail(FHX_HP_COUNT);
                frac |= c != '0';
                ++p;
            }
        }
        if (ni + nf == 0 || !is_space(c)) return bad_token(c, FHX_HP_COUNT);
        if (ni + nf > 15 || v > 2147483647ll) return fail(FHX_HP_COUNT);
        if (frac) return fail(FHX_HP_FRACTION);
        *out = (int)v;
        return true;
    }
};

// Sum of `v` over each run of consecutive lanes that hold the same bin, one atomic per run (posted by the run's first lane).
// Every lane of the wave calls it; a lane without a line passes slot = -1 and is a run of its own that posts nothing.
__device__ inline void add_runs(long long slot, unsigned long long v, unsigned long long* __restrict__ totals) {
    const int lane = threadIdx.x & 63;
    const long long prev = __shfl_up(slot, 1, 64);
    const bool head = lane == 0 || prev != slot;
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    const int end = above ? lane + 1 + (__ffsll((long long)above) - 1) : 64;   // first lane of the next run
    for (int s = 1; s < 64; s <<= 1) {                                         // suffix sums that stop at the run's end
        const unsigned long long other = __shfl_down(v, s, 64);
        if (lane + s < end) v += other;
    }
    if (head && slot >= 0) atomicAdd(totals + slot, v);
}

__global__ __launch_bounds__(WG) void hp_parse(const unsigned char* __restrict__ text, int64_t T, const unsigned long long* __restrict__ block_off,
                                               const int2* __restrict__ bins, long long index_base, long long n_slots, int64_t n_rows,
                                               int32_t* __restrict__ chr1, int32_t* __restrict__ mid1, int32_t* __restrict__ chr2,
                                               int32_t* __restrict__ mid2, int32_t* __restrict__ count, unsigned long long* __restrict__ totals,
                                               unsigned long long* __restrict__ first_error, unsigned long long* __restrict__ absent_index) {
    __shared__ unsigned short lstart[LSTART_ENTRIES];
    const BlockLines B = block_lines(text, T, block_off, lstart);
    for (int base = 0; base < B.n_lines; base += WG) {      // n_lines is the same for every lane: the shuffles below see whole waves
        const int e = base + threadIdx.x;
        long long si = -1, sj = -1;
        int cnt = 0;
        if (e < B.n_lines) {
            const int64_t r = B.row0 + e;
            Cursor c{text, T, B.b0 + lstart[e], 0, 0};
            c.limit = c.p + MAX_LINE;
            long long i = 0, j = 0, absent = 0;
            bool ok = (c.next_token() && c.integer(&i) && c.next_token() && c.integer(&j) && c.next_token() && c.count(&cnt)) ||
                      c.fail(FHX_HP_TOKENS);                                  // the line ended early (or next_token said why not)
            if (ok && (c.next_token() || c.why)) ok = c.fail(FHX_HP_TOKENS);  // a fourth token
            int2 bi = make_int2(-1, 0), bj = make_int2(-1, 0);
            if (ok) {
                si = i - index_base;
                sj = j - index_base;
                if (si >= 0 && si < n_slots) bi = bins[si];
                if (sj >= 0 && sj < n_slots) bj = bins[sj];
                if (bi.x < 0 || bj.x < 0) {                                   // outside the table, or a slot the bed does not fill
                    absent = bi.x < 0 ? i : j;                                // the reference looks i up first (:40)
                    ok = c.fail(FHX_HP_ABSENT);
                }
            }
            if (ok && r >= n_rows) ok = c.fail(FHX_HP_INTERNAL);              // the scan and this kernel disagree about the lines
            if (ok) {
                chr1[r] = bi.x;
                mid1[r] = bi.y;
                chr2[r] = bj.x;
                mid2[r] = bj.y;
                count[r] = cnt;
            } else {
                si = sj = -1;
                atomicMin(first_error, error_word(r + 1, c.why));
                if (c.why == FHX_HP_ABSENT) atomicMin(absent_index, ((unsigned long long)(r + 1) << 32) | (unsigned int)(int)absent);
            }
        }
        add_runs(si, (unsigned long long)cnt, totals);
        add_runs(sj, (unsigned long long)cnt, totals);
    }
}

__global__ __launch_bounds__(WG) void hp_max_total(const unsigned long long* __restrict__ totals, long long n_slots, unsigned long long* __restrict__ out) {
    unsigned long long m = 0;
    for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < n_slots; s += (long long)gridDim.x * blockDim.x) m = max(m, totals[s]);
    for (int s = 32; s >= 1; s >>= 1) m = max(m, (unsigned long long)__shfl_down(m, s, 64));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

}  // namespace hpd

// ===================================================================================================================
struct fhx_hp : fhx::TextHandle {
    // the bin table: slot = index - index_base
    bool have_bins = false;
    int64_t index_base = 0, n_slots = 0;
    int2* d_bins = nullptr;
    unsigned long long* d_totals = nullptr;
    // the last parsed matrix
    fhx::CellColumns cols;
};

namespace {

void drop_rows(fhx_hp* hp) { hp->cols.drop(); }

}  // namespace

extern "C" {

int fhx_hp_create(int device, fhx_hp** out) { return fhx::handle_create(device, out); }

void fhx_hp_destroy(fhx_hp* hp) {
    fhx::text_handle_destroy(hp, [&] {
        drop_rows(hp);
        fhx::dev_free(hp->d_bins);
        fhx::dev_free(hp->d_totals);
    });
}

const char* fhx_hp_last_error(const fhx_hp* hp) { return fhx::handle_last_error(hp); }

int fhx_hp_load_bins(fhx_hp* hp, int64_t index_base, const int32_t* chr_id, const int32_t* mid, int64_t n_slots) {
    if (!hp || n_slots < 0 || (n_slots > 0 && (!chr_id || !mid))) return FHX_ERR_ARG;
    if (n_slots > ((int64_t)1 << 27)) return fhx::fail(hp, FHX_ERR_UNSUPPORTED, "a bin table of more than 2^27 slots");
    if (index_base < -((int64_t)1 << 31) || index_base + n_slots > ((int64_t)1 << 31))
        return fhx::fail(hp, FHX_ERR_UNSUPPORTED, "bin indices outside int32");
    TH_HIP(hp, hipSetDevice(hp->device));
    TH_HIP(hp, hipStreamSynchronize(hp->stream));
    drop_rows(hp);
    fhx::dev_free(hp->d_bins);
    fhx::dev_free(hp->d_totals);
    hp->have_bins = false;
    std::vector<int2> table((size_t)n_slots);
    for (int64_t s = 0; s < n_slots; ++s) table[(size_t)s] = make_int2(chr_id[s] < 0 ? -1 : chr_id[s], mid[s]);
    const size_t slots = (size_t)std::max<int64_t>(n_slots, 1);
    TH_HIP(hp, fhx::dev_malloc(&hp->d_bins, slots * sizeof(int2)));
    TH_HIP(hp, fhx::dev_malloc(&hp->d_totals, slots * sizeof(unsigned long long)));
    if (n_slots) TH_HIP(hp, hipMemcpyAsync(hp->d_bins, table.data(), (size_t)n_slots * sizeof(int2), hipMemcpyHostToDevice, hp->stream));
    TH_HIP(hp, hipMemsetAsync(hp->d_totals, 0, slots * sizeof(unsigned long long), hp->stream));
    TH_HIP(hp, hipStreamSynchronize(hp->stream));                                 // `table` goes out of scope
    hp->index_base = index_base;
    hp->n_slots = n_slots;
    hp->have_bins = true;
    return FHX_OK;
}

int fhx_hp_parse_matrix(fhx_hp* hp, const char* path, int64_t* n_rows, int32_t* why, int64_t* bad_line, int64_t* bad_index) {
    using namespace hpd;
    if (!hp || !path || !n_rows || !why || !bad_line || !bad_index) return FHX_ERR_ARG;
    *n_rows = 0;
    *why = FHX_HP_OK;
    *bad_line = 0;
    *bad_index = 0;
    if (!hp->have_bins) return fhx::fail(hp, FHX_ERR_ARG, "fhx_hp_load_bins has not been called");
    TH_HIP(hp, hipSetDevice(hp->device));
    TH_HIP(hp, hipStreamSynchronize(hp->stream));
    drop_rows(hp);
    const size_t slots = (size_t)std::max<int64_t>(hp->n_slots, 1);
    TH_HIP(hp, hipMemsetAsync(hp->d_totals, 0, slots * sizeof(unsigned long long), hp->stream));
    fhx::TextFile src;
    if (const int rc = src.open(path, /*allow_gzip=*/false, &hp->err)) return rc;
    const int64_t T = src.size();
    if (T == 0) {                                                             // no lines: no rows, all totals zero
        TH_HIP(hp, hipStreamSynchronize(hp->stream));
        return FHX_OK;
    }
    const int64_t n_blocks = (T + BLOCK_BYTES - 1) / BLOCK_BYTES;
    if (n_blocks > 0x7fffffffll) return fhx::fail(hp, FHX_ERR_UNSUPPORTED, "a matrix file of more than 32 TB");
    const bool timing = std::getenv("FHX_TIMING") != nullptr;
    double t_stage[3] = {0, 0, 0};
    fhx::StageClock clock{t_stage};
    fhx::DeviceScratch tmp;
    unsigned char* d_text = nullptr;
    unsigned int* d_block_nl = nullptr;
    unsigned long long *d_block_off = nullptr, *d_words = nullptr;
    TH_HIP(hp, tmp.get_n(&d_text, (size_t)n_blocks * BLOCK_BYTES + 64));
    TH_HIP(hp, tmp.get_n(&d_block_nl, (size_t)n_blocks));
    TH_HIP(hp, tmp.get_n(&d_block_off, (size_t)n_blocks));
    // d_words: [0] newlines in all, [1] smallest (line << 8 | reason), [2] smallest (line << 32 | index) among the absent-index
    // lines, [3] the largest total, [4] bytes-not-taken flag of the scan
    TH_HIP(hp, tmp.get_n(&d_words, 5));
    fhx::TextBatch whole;                                                     // the whole file is resident: one batch
    if (const int rc = fhx::upload_batch(hp, src, "matrix", 0, T, d_text, &whole)) return rc;
    const unsigned long long init[5] = {0ull, NO_ERROR, NO_ERROR, 0ull, 0ull};
    TH_HIP(hp, hipMemcpyAsync(d_words, init, sizeof(init), hipMemcpyHostToDevice, hp->stream));
    TH_HIP(hp, hipStreamSynchronize(hp->stream));                             // `init` may go
    clock.mark(0);
    hipLaunchKernelGGL(scan_text<TextModeBytes>, dim3((unsigned)n_blocks), dim3(WG), 0, hp->stream, (const unsigned char*)d_text, T, d_block_nl,
                       (unsigned int*)(d_words + 4));
    hipLaunchKernelGGL(fhxscan::scan_tiles, dim3(1), dim3(fhxscan::THREADS), 0, hp->stream, (const unsigned int*)d_block_nl, n_blocks, d_block_off,
                       d_words);
    TH_HIP(hp, hipGetLastError());
    unsigned long long n_newlines = 0;
    TH_HIP(hp, hipMemcpyAsync(&n_newlines, d_words, sizeof(n_newlines), hipMemcpyDeviceToHost, hp->stream));
    TH_HIP(hp, hipStreamSynchronize(hp->stream));
    clock.mark(1);
    const int64_t n = whole.lines(n_newlines);
    if (n > 0x7fffffffll) return fhx::fail(hp, FHX_ERR_UNSUPPORTED, "a matrix of more than 2^31 - 1 lines");
    TH_HIP(hp, hp->cols.alloc(n));
    const fhx::CellColumns& C = hp->cols;
    hipLaunchKernelGGL(hp_parse, dim3((unsigned)n_blocks), dim3(WG), 0, hp->stream, (const unsigned char*)d_text, T,
                       (const unsigned long long*)d_block_off, (const int2*)hp->d_bins, (long long)hp->index_base, (long long)hp->n_slots, n, C.col(0),
                       C.col(1), C.col(2), C.col(3), C.col(4), hp->d_totals, d_words + 1, d_words + 2);
    hipLaunchKernelGGL(hp_max_total, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((hp->n_slots + WG - 1) / WG, 1024))), dim3(WG), 0,
                       hp->stream, (const unsigned long long*)hp->d_totals, (long long)hp->n_slots, d_words + 3);
    TH_HIP(hp, hipGetLastError());
    unsigned long long words[5] = {0, 0, 0, 0, 0};
    TH_HIP(hp, hipMemcpyAsync(words, d_words, sizeof(words), hipMemcpyDeviceToHost, hp->stream));
    TH_HIP(hp, hipStreamSynchronize(hp->stream));
    clock.mark(2);
    if (timing)
        std::fprintf(stderr, "hicpro matrix on the device (%s): %lld lines, %lld bytes: upload %.6f s; scan %.6f s; parse + accumulate %.6f s\n",
                     path, (long long)n, (long long)T, t_stage[0], t_stage[1], t_stage[2]);
    const fhx::Refusal refused{hp, why, bad_line};
    auto forget = [&] {                                                       // nothing stays loaded
        drop_rows(hp);
        (void)hipMemsetAsync(hp->d_totals, 0, slots * sizeof(unsigned long long), hp->stream);
        (void)hipStreamSynchronize(hp->stream);
    };
    auto refuse = [&](int rc, int32_t w, int64_t line, int64_t index, const std::string& msg) {
        forget();
        *bad_index = index;
        return refused(rc, w, line, msg);
    };
    if (words[1] != NO_ERROR) {
        const int64_t line = error_line(words[1]);
        if (error_why(words[1]) != FHX_HP_ABSENT) {
            forget();
            return refused.word(words[1], FHX_HP_INTERNAL);
        }
        if ((int64_t)(words[2] >> 32) != line) return refuse(FHX_ERR_INTERNAL, FHX_HP_INTERNAL, line, 0, "error words disagree about the first bad line");
        const int64_t index = (int64_t)(int32_t)(unsigned int)(words[2] & 0xFFFFFFFFull);
        return refuse(FHX_ERR_REFERENCE_EXIT, FHX_HP_ABSENT, line, index, "line " + std::to_string(line) + ": index " + std::to_string(index) + " is not in the bed file");
    }
    if (words[4]) return refuse(FHX_ERR_INTERNAL, FHX_HP_INTERNAL, 0, 0, "the scan saw a byte this path does not take, the parse kernel did not");
    if (words[3] >= TOTAL_LIMIT)
        return refuse(FHX_ERR_UNSUPPORTED, FHX_HP_TOTAL, 0, 0, "a bin's total contact count reaches 2^53: the reference's float sum would round");
    *n_rows = n;
    return FHX_OK;
}

int fhx_hp_totals(fhx_hp* hp, int64_t* tcc) {
    if (!hp || (hp->n_slots > 0 && !tcc)) return FHX_ERR_ARG;
    if (!hp->have_bins) return fhx::fail(hp, FHX_ERR_ARG, "fhx_hp_load_bins has not been called");
    TH_HIP(hp, hipSetDevice(hp->device));
    if (hp->n_slots) TH_HIP(hp, hipMemcpyAsync(tcc, hp->d_totals, (size_t)hp->n_slots * sizeof(int64_t), hipMemcpyDeviceToHost, hp->stream));
    TH_HIP(hp, hipStreamSynchronize(hp->stream));
    return FHX_OK;
}

int fhx_hp_fetch_rows(fhx_hp* hp, int32_t* chr1, int32_t* mid1, int32_t* chr2, int32_t* mid2, int32_t* count) {
    return hp ? hp->cols.fetch(hp, {chr1, mid1, chr2, mid2, count}) : FHX_ERR_ARG;
}

void* fhx_hp_device_ptr(fhx_hp* hp, int32_t which) { return hp ? hp->cols.ptr(which) : nullptr; }

void* fhx_hp_stream(fhx_hp* hp) { return hp ? (void*)hp->stream : nullptr; }

}  // extern "C"
