// fhx_juicer.hip - the text `juicer_tools dump` / `straw` prints for one chromosome pair (`binX binY count` per record) turned into
// Fit-Hi-C's contact counts on MI355X (gfx950)
// (reference: fithic/utils/createFitHiCContacts-hic_old.sh:6, one awk printf per line, and fithic/utils/createFitHiCContacts-hic.py:93,
// one print per record).
//
// Every input line gives exactly one output line, row number = line number: nothing is compacted and no good line costs an atomic.
// The text goes through HBM in batches cut at the last newline (fhx_textupload.hpp).  Per batch:
//
//   scan_text<JcBytes>, scan_tiles   the newline layer (fhx_textlines.hpp): the line number of every block's first line, and whether
//                  any byte of the batch is refused
//   jc_parse       the lines that begin in a block, one per lane, one walk: where tokens 1-3 lie.  VERBATIM mode (resolution 0)
//                  takes any line and only adds up the bytes of `CHR1 \t $1 \t CHR2 \t $2 \t $3 \n`.  MIDPOINT mode applies the grammar
//                  (exactly three tokens, bins of 1-10 digits on the grid, a whole count up to 2^24) and stores the five int32
//                  columns at row = line number, lanes on consecutive rows.  Per line: the output length (2 bytes).  Per block: bytes.
//   scan_tiles     block bytes -> the block's 64-bit offset in the output
//   jc_format      256 lines per round, their lengths scanned; every lane writes its line into a 16 KB window of LDS (a round can be
//                  256 x 4227 bytes: a lane writes only what falls into the current window), and the window goes out 16 bytes a lane
//                  where it is whole, its start moved back to a 16-byte boundary of the output.  Midpoint lines are made from the
//                  columns, verbatim ones from the text.  What a lane wrote is compared with what jc_parse measured.
//
// An output line can be 131 times its input line (an empty line between two 63-byte names), so nothing is sized by the input: the
// output buffer grows to what the scan found and every store is checked against it.  Anything outside the grammar is REFUSED with
// the smallest offending line number (atomicMin over line << 8 | reason) and nothing stays loaded.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fithic_mi355x.h"
#include "fhx_fmt.hpp"
#include "fhx_pairline.hpp"
#include "fhx_textupload.hpp"

namespace jcd {

using namespace fhxlines;

constexpr int NAME_BYTES = FHX_JC_NAME_BYTES;  // `chr` + 63
constexpr int NAME_SLOT = 80;                  // bytes per name in the device copy
constexpr int WINDOW = 16384;                  // LDS bytes of jc_format
constexpr int BIN_DIGITS = 10, COUNT_DIGITS = 15;
constexpr long long COUNT_MAX = 1ll << 24;     // hicstraw's records are binary32: every whole number up to here is one

struct Words {
    unsigned long long first_error;            // smallest (line << 8 | reason)
    unsigned long long out_bytes;              // scan_tiles' total of the block bytes
};

__device__ inline bool refused_byte(unsigned int c) { return c < 0x20u ? (c != '\t' && c != '\n') : c >= 0x7fu; }

struct JcBytes {                               // scan_text's policy
    static __device__ void check(bool& bad, unsigned int c, const unsigned char*, int64_t, int64_t) { bad |= refused_byte(c); }
};

using fhxpair::is_digit;

// one line split at runs of blank and tab: tokens 1 to 3 relative to the line's first byte (length 0: the token is missing)
struct Line {
    int why, tok;
    int b1, n1, b2, n2, b3, n3;
};

__device__ inline void walk(const unsigned char* __restrict__ text, int64_t T, int64_t start, int check_bytes, Line& L) {
    L.why = 0;
    L.b1 = L.n1 = L.b2 = L.n2 = L.b3 = L.n3 = 0;
    int tok = 0, begin = 0, k = 0;
    bool in_tok = false;
    auto close = [&](int end) {
        const int n = end - begin;
        if (tok == 1) { L.b1 = begin; L.n1 = n; }
        else if (tok == 2) { L.b2 = begin; L.n2 = n; }
        else if (tok == 3) { L.b3 = begin; L.n3 = n; }
    };
    for (;; ++k) {
        const int64_t p = start + k;
        const int c = p < T ? (int)text[p] : '\n';                            // the end of the text ends the line
        if (c == '\n') break;
        if (k >= MAX_LINE) {
            L.why = FHX_JC_LONG_LINE;
            break;
        }
        if (check_bytes && refused_byte((unsigned int)c)) {
            L.why = FHX_JC_BYTES;
            break;
        }
        const bool blank = c == ' ' || c == '\t';
        if (!blank && !in_tok) {
            in_tok = true;
            ++tok;
            begin = k;
        } else if (blank && in_tok) {
            in_tok = false;
            close(k);
        }
    }
    if (in_tok) close(k);
    L.tok = tok;
}

// 1 to 10 digits at t[0, n) -> their value; false for anything else
__device__ inline bool bin_value(const unsigned char* __restrict__ t, int n, long long* out) {
    if (n < 1 || n > BIN_DIGITS) return false;
    long long v = 0;
    for (int k = 0; k < n; ++k) {
        if (!is_digit(t[k])) return false;
        v = v * 10 + (t[k] - '0');
    }
    *out = v;
    return true;
}

__device__ inline bool same_word(const unsigned char* __restrict__ t, int n, const char* word) {      // ASCII letters in any case
    int k = 0;
    for (; k < n && word[k]; ++k)
        if ((t[k] | 0x20) != word[k]) return false;
    return k == n && !word[k];
}

// The count at t[0, n), n >= 1: `digits`, or `digits.` and one or more `0` -> 0 and its value; FHX_JC_COUNT for more than 15
// digits, a value above 2^24 or a token that is no number; FHX_JC_FRACTION for what a normalised dump holds (a fraction, an
// exponent, a sign, nan, inf: every byte one of 0-9 . + - e E, or one of the three words behind an optional sign).
__device__ inline int count_value(const unsigned char* __restrict__ t, int n, long long* out) {
    int k = 0, digits = 0;
    long long v = 0;
    for (; k < n && is_digit(t[k]); ++k, ++digits)
        if (digits < COUNT_DIGITS) v = v * 10 + (t[k] - '0');
    bool whole = digits >= 1 && k == n;
    if (digits >= 1 && k < n && t[k] == '.' && k + 1 < n) {
        whole = true;
        for (int j = k + 1; j < n; ++j) whole &= t[j] == '0';
    }
    if (whole) {
        if (digits > COUNT_DIGITS || v > COUNT_MAX) return FHX_JC_COUNT;
        *out = v;
        return 0;
    }
    const int s = (t[0] == '+' || t[0] == '-') ? 1 : 0;
    if (same_word(t + s, n - s, "nan") || same_word(t + s, n - s, "inf") || same_word(t + s, n - s, "infinity")) return FHX_JC_FRACTION;
    for (int j = 0; j < n; ++j) {
        const int c = t[j];
        if (!(is_digit(c) || c == '.' || c == '+' || c == '-' || c == 'e' || c == 'E')) return FHX_JC_COUNT;
    }
    return FHX_JC_FRACTION;
}

__device__ inline unsigned int digits_of(long long v) {                       // v >= 0
    unsigned int n = 1;
    for (unsigned long long u = (unsigned long long)v; u >= 10ull; u /= 10ull) ++n;
    return n;
}

// ---- the grammar, the columns and the length of every output line --------------------------------------------------------------
__global__ __launch_bounds__(WG) void jc_parse(const unsigned char* __restrict__ text, int64_t T, const unsigned long long* __restrict__ block_off,
                                               int64_t n_lines_batch, int64_t line_base, long long res, int name_bytes, int id1, int id2,
                                               int check_bytes, int32_t* __restrict__ chr1, int32_t* __restrict__ mid1,
                                               int32_t* __restrict__ chr2, int32_t* __restrict__ mid2, int32_t* __restrict__ count,
                                               unsigned short* __restrict__ info, unsigned int* __restrict__ block_bytes,
                                               Words* __restrict__ words) {
    __shared__ unsigned short lstart[LSTART_ENTRIES];
    const BlockLines B = block_lines(text, T, block_off, lstart);
    unsigned int my_bytes = 0;
    for (int e = threadIdx.x; e < B.n_lines; e += WG) {
        const int64_t r = B.row0 + e;
        const int64_t start = B.b0 + lstart[e];
        Line L;
        walk(text, T, start, check_bytes, L);
        int why = L.why;
        unsigned int len = 0;
        if (!why && res == 0) len = (unsigned int)(name_bytes + L.n1 + L.n2 + L.n3 + 5);
        else if (!why) {
            long long x = 0, y = 0, c = 0;
            if (L.tok != 3) why = FHX_JC_TOKENS;
            else if (!bin_value(text + start + L.b1, L.n1, &x) || !bin_value(text + start + L.b2, L.n2, &y)) why = FHX_JC_BIN;
            else if (x % res != 0 || y % res != 0) why = FHX_JC_GRID;
            else if (x + res / 2 > 2147483647ll || y + res / 2 > 2147483647ll) why = FHX_JC_RANGE;
            else why = count_value(text + start + L.b3, L.n3, &c);
            if (!why && r < n_lines_batch) {
                const long long m1 = x + res / 2, m2 = y + res / 2;
                chr1[r] = id1;
                mid1[r] = (int32_t)m1;
                chr2[r] = id2;
                mid2[r] = (int32_t)m2;
                count[r] = (int32_t)c;
                len = (unsigned int)name_bytes + digits_of(m1) + digits_of(m2) + digits_of(c) + 2u + 5u;       // `.0`, four tabs, the newline
            }
        }
        if (!why && r >= n_lines_batch) why = FHX_JC_INTERNAL;                // the scan and this kernel disagree about the lines
        if (why) atomicMin(&words->first_error, error_word(line_base + r + 1, why));
        if (r < n_lines_batch) info[r] = (unsigned short)(why ? 0u : len);
        my_bytes += why ? 0u : len;
    }
    unsigned int total;
    fhxscan::block_exclusive_scan(my_bytes, &total);                          // every lane of the block arrives here
    if (threadIdx.x == 0) block_bytes[blockIdx.x] = total;
}

// ---- the output lines, dense and in file order -----------------------------------------------------------------------------------
// what a lane writes of its line: the bytes that fall into the window [w0, w0 + WINDOW) of the round
struct WindowSink {
    unsigned char* lds;
    unsigned int pos, w0;
    __device__ void put(int c) {
        const unsigned int at = pos++ - w0;                                   // wraps to a huge value below the window
        if (at < (unsigned int)WINDOW) lds[at] = (unsigned char)c;
    }
    __device__ void bytes(const unsigned char* __restrict__ src, int n) {
        for (int k = 0; k < n; ++k) put(src[k]);
    }
    __device__ void number(long long v) {
        char tmp[24];
        const int n = fhx::fmt::put_i64(tmp, v);
        for (int k = 0; k < n; ++k) put(tmp[k]);
    }
};

__global__ __launch_bounds__(WG) void jc_format(const unsigned char* __restrict__ text, int64_t T, const unsigned long long* __restrict__ block_off,
                                                int64_t n_lines_batch, int64_t line_base, long long res, const unsigned char* __restrict__ names,
                                                int len1, int len2, const int32_t* __restrict__ mid1, const int32_t* __restrict__ mid2,
                                                const int32_t* __restrict__ count, const unsigned short* __restrict__ info,
                                                const unsigned long long* __restrict__ out_off, unsigned char* __restrict__ out,
                                                int64_t out_capacity, Words* __restrict__ words) {
    __shared__ unsigned short lstart[LSTART_ENTRIES];
    __shared__ __attribute__((aligned(16))) unsigned char window[WINDOW];
    const BlockLines B = block_lines(text, T, block_off, lstart);
    int64_t at = (int64_t)out_off[blockIdx.x];
    for (int base = 0; base < B.n_lines; base += WG) {      // n_lines is the same for every lane
        const int e = base + (int)threadIdx.x;
        const int64_t r = B.row0 + e;
        const bool valid = e < B.n_lines && r < n_lines_batch;
        const unsigned int len = valid ? (unsigned int)info[r] : 0u;
        unsigned int total;
        const unsigned int pre = fhxscan::block_exclusive_scan(len, &total);
        // the line's pieces, once for all its windows
        const unsigned char* line = text + B.b0 + (len ? (int64_t)lstart[e] : 0);
        Line L;
        L.b1 = L.n1 = L.b2 = L.n2 = L.b3 = L.n3 = 0;
        long long m1 = 0, m2 = 0, c = 0;
        if (len && res == 0) walk(text, T, B.b0 + lstart[e], 0, L);
        else if (len) {
            m1 = mid1[r];
            m2 = mid2[r];
            c = count[r];
        }
        // the window starts on a 16-byte boundary of the output: the round's bytes lie `mis` bytes into its first one
        const unsigned int mis = (unsigned int)(at & 15);
        const unsigned int vpre = mis + pre, vend = mis + total;
        for (unsigned int w0 = 0; total != 0 && w0 < vend; w0 += WINDOW) {
            if (len && vpre < w0 + WINDOW && vpre + len > w0) {
                WindowSink s{window, vpre, w0};
                s.bytes(names, len1);
                s.put('\t');
                if (res == 0) s.bytes(line + L.b1, L.n1);
                else s.number(m1);
                s.put('\t');
                s.bytes(names + NAME_SLOT, len2);
                s.put('\t');
                if (res == 0) {
                    s.bytes(line + L.b2, L.n2);
                    s.put('\t');
                    s.bytes(line + L.b3, L.n3);
                } else {
                    s.number(m2);
                    s.put('\t');
                    s.number(c);
                    s.put('.');
                    s.put('0');
                }
                s.put('\n');
                // what was written is what jc_parse counted, or nothing of this call is kept
                if (s.pos - vpre != len) atomicMin(&words->first_error, error_word(line_base + r + 1, FHX_JC_INTERNAL));
            }
            __syncthreads();
            const unsigned int lo = max(w0, mis) - w0, hi = min(w0 + (unsigned int)WINDOW, vend) - w0;      // the window's bytes that are output
            const int64_t g = at - (int64_t)mis + (int64_t)w0;                                              // of the window's first byte: 16 | g
            for (unsigned int j = threadIdx.x * 16u; j < hi; j += WG * 16u) {
                if (j >= lo && j + 16u <= hi && g + (int64_t)j + 16 <= out_capacity) {
                    *reinterpret_cast<uint4*>(out + g + j) = *reinterpret_cast<const uint4*>(window + j);
                } else {
                    for (unsigned int k = j; k < j + 16u; ++k)
                        if (k >= lo && k < hi && g + (int64_t)k < out_capacity) out[g + k] = window[k];
                }
            }
            __syncthreads();                                // the window is written again
        }
        at += total;
    }
}

}  // namespace jcd

// ===================================================================================================================
struct fhx_jc : fhx::TextHandle {
    // the rows kept so far (midpoint mode): five columns that grow together
    int32_t* d_col[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int64_t col_capacity = 0, n_rows = 0, n_lines = 0;
    std::vector<char> text;                       // the output text kept so far
    double seconds[FHX_JC_STAGES] = {0, 0, 0, 0, 0};
};

namespace {

void drop_all(fhx_jc* jc) {
    for (int32_t*& p : jc->d_col) fhx::dev_free(p);
    jc->col_capacity = jc->n_rows = jc->n_lines = 0;
    std::vector<char>().swap(jc->text);
}

// room for `need` rows in the five columns, the first `keep` of them kept
hipError_t grow_columns(fhx_jc* jc, int64_t keep, int64_t need) {
    if (need <= jc->col_capacity) return hipSuccess;
    const int64_t want = std::max<int64_t>(need, jc->col_capacity * 2);
    for (int32_t*& p : jc->d_col) {
        int32_t* bigger = nullptr;
        hipError_t e = fhx::dev_malloc(&bigger, (size_t)want * sizeof(int32_t));
        if (e != hipSuccess) return e;
        if (keep > 0) e = hipMemcpyAsync(bigger, p, (size_t)keep * sizeof(int32_t), hipMemcpyDeviceToDevice, jc->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(jc->stream);
        fhx::dev_free(p);
        p = bigger;                               // a failed copy leaves the handle consistent: the caller drops everything
        if (e != hipSuccess) return e;
    }
    jc->col_capacity = want;
    return hipSuccess;
}

bool name_ok(const char* s) {
    const size_t n = s ? std::strlen(s) : 0;
    if (n < 1 || n > (size_t)FHX_JC_NAME_BYTES) return false;
    for (size_t k = 0; k < n; ++k) {
        const unsigned char c = (unsigned char)s[k];
        if (!((c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || (c >= '0' && c <= '9') || c == '_' || c == '.' || c == '-')) return false;
    }
    return true;
}

// d_out[0, bytes) appended to jc->text through the two pinned buffers: the copy engine fills one while the host empties the other
int copy_out(fhx_jc* jc, const unsigned char* d_out, int64_t bytes) {
    for (int k = 0; k < 2; ++k) {
        if (!jc->pinned[k]) TH_HIP(jc, hipHostMalloc(&jc->pinned[k], fhx::TextHandle::kChunk, hipHostMallocDefault));
        if (!jc->ev[k]) TH_HIP(jc, hipEventCreateWithFlags(&jc->ev[k], hipEventDisableTiming));
    }
    const int64_t chunk = (int64_t)fhx::TextHandle::kChunk;
    const size_t had = jc->text.size();
    jc->text.resize(had + (size_t)bytes);
    int64_t issued = 0, drained = 0;
    int n_issued = 0, n_drained = 0;                                          // chunk k travels through buffer k & 1
    while (drained < bytes) {
        for (; issued < bytes && n_issued - n_drained < 2; ++n_issued) {
            const int64_t now = std::min(chunk, bytes - issued);
            TH_HIP(jc, hipMemcpyAsync(jc->pinned[n_issued & 1], d_out + issued, (size_t)now, hipMemcpyDeviceToHost, jc->stream));
            TH_HIP(jc, hipEventRecord(jc->ev[n_issued & 1], jc->stream));
            issued += now;
        }
        const int64_t now = std::min(chunk, bytes - drained);
        TH_HIP(jc, hipEventSynchronize(jc->ev[n_drained & 1]));
        std::memcpy(jc->text.data() + had + drained, jc->pinned[n_drained & 1], (size_t)now);
        drained += now;
        ++n_drained;
    }
    TH_HIP(jc, hipStreamSynchronize(jc->stream));
    return FHX_OK;
}

// fhx_jc_convert_file behind its argument checks; whatever it returns but FHX_OK, the caller drops everything
int convert_file(fhx_jc* jc, const char* path, const char* name1, const char* name2, int64_t resolution, int32_t id1, int32_t id2,
                 int32_t keep_text, int32_t keep_rows, int64_t* n_lines, int32_t* why, int64_t* bad_line) {
    using namespace jcd;
    TH_HIP(jc, hipSetDevice(jc->device));
    TH_HIP(jc, hipStreamSynchronize(jc->stream));
    fhx::StageClock clock{jc->seconds};
    fhx::DeviceScratch tmp;
    fhx::TextBatches in;
    if (const int rc = in.open(jc, &tmp, &clock, path, "dump", "FHX_JC_BATCH_BYTES", (int64_t)1 << 31)) return rc;
    const int len1 = (int)std::strlen(name1), len2 = (int)std::strlen(name2);
    unsigned char *d_out = nullptr, *d_names = nullptr;
    unsigned int* d_block_bytes = nullptr;
    unsigned long long* d_out_off = nullptr;
    unsigned short* d_info = nullptr;
    int64_t info_capacity = 0, out_capacity = 0;
    Words* d_words = nullptr;
    TH_HIP(jc, tmp.get_n(&d_block_bytes, (size_t)in.max_blocks));
    TH_HIP(jc, tmp.get_n(&d_out_off, (size_t)in.max_blocks));
    TH_HIP(jc, tmp.get_n(&d_names, (size_t)2 * NAME_SLOT));
    TH_HIP(jc, tmp.get_n(&d_words, 1));
    unsigned char names[2 * NAME_SLOT];
    std::memset(names, 0, sizeof(names));
    std::memcpy(names, name1, (size_t)len1);
    std::memcpy(names + NAME_SLOT, name2, (size_t)len2);
    TH_HIP(jc, hipMemcpyAsync(d_names, names, sizeof(names), hipMemcpyHostToDevice, jc->stream));
    TH_HIP(jc, hipStreamSynchronize(jc->stream));
    Words words;
    const fhx::Refusal refuse{jc, why, bad_line};
    for (; in.more(); in.advance()) {
        std::memset(&words, 0, sizeof(words));
        words.first_error = NO_ERROR;
        TH_HIP(jc, hipMemcpyAsync(d_words, &words, sizeof(words), hipMemcpyHostToDevice, jc->stream));
        if (const int rc = in.next<JcBytes>()) return rc;
        const int64_t n = in.lines;
        const int64_t row_base = jc->n_rows;                                  // a call that keeps no rows writes every batch over the last
        TH_HIP(jc, tmp.grow(&d_info, &info_capacity, n));
        if (resolution != 0) TH_HIP(jc, grow_columns(jc, row_base, row_base + n));
        int32_t* col[5];
        for (int k = 0; k < 5; ++k) col[k] = jc->d_col[k] ? jc->d_col[k] + row_base : nullptr;
        hipLaunchKernelGGL(jc_parse, dim3((unsigned)in.n_blocks), dim3(WG), 0, jc->stream, (const unsigned char*)in.d_text, in.len,
                           (const unsigned long long*)in.d_block_off, n, in.line_base, (long long)resolution, len1 + len2, (int)id1, (int)id2,
                           (int)in.refused_bytes, col[0], col[1], col[2], col[3], col[4], d_info, d_block_bytes, d_words);
        hipLaunchKernelGGL(fhxscan::scan_tiles, dim3(1), dim3(fhxscan::THREADS), 0, jc->stream, (const unsigned int*)d_block_bytes, in.n_blocks,
                           d_out_off, &d_words->out_bytes);
        TH_HIP(jc, hipGetLastError());
        TH_HIP(jc, hipMemcpyAsync(&words, d_words, sizeof(words), hipMemcpyDeviceToHost, jc->stream));
        TH_HIP(jc, hipStreamSynchronize(jc->stream));
        clock.mark(2);
        if (words.first_error != NO_ERROR) return refuse.word(words.first_error, FHX_JC_INTERNAL);      // earlier batches hold the smaller line numbers
        const int64_t bytes = (int64_t)words.out_bytes;
        if (keep_text && bytes > 0) {
            TH_HIP(jc, tmp.grow(&d_out, &out_capacity, (bytes + 15) / 16 * 16));
            hipLaunchKernelGGL(jc_format, dim3((unsigned)in.n_blocks), dim3(WG), 0, jc->stream, (const unsigned char*)in.d_text, in.len,
                               (const unsigned long long*)in.d_block_off, n, in.line_base, (long long)resolution, (const unsigned char*)d_names, len1,
                               len2, (const int32_t*)col[1], (const int32_t*)col[3], (const int32_t*)col[4], (const unsigned short*)d_info,
                               (const unsigned long long*)d_out_off, d_out, bytes, d_words);
            TH_HIP(jc, hipGetLastError());
            TH_HIP(jc, hipMemcpyAsync(&words, d_words, sizeof(words), hipMemcpyDeviceToHost, jc->stream));
            TH_HIP(jc, hipStreamSynchronize(jc->stream));
            clock.mark(3);
            if (words.first_error != NO_ERROR) return refuse.word(words.first_error, FHX_JC_INTERNAL);
            if (const int rc = copy_out(jc, d_out, bytes)) return rc;
            clock.mark(4);
        }
        if (keep_rows) jc->n_rows += n;
    }
    jc->n_lines += in.line_base;
    *n_lines = in.line_base;
    if (std::getenv("FHX_TIMING"))
        std::fprintf(stderr, "juicer dump on the device (%s): %lld lines, %lld bytes of output so far: read + upload %.6f s; scan %.6f s; parse %.6f s; "
                     "format %.6f s; copy out %.6f s\n", path, (long long)in.line_base, (long long)jc->text.size(), jc->seconds[0], jc->seconds[1],
                     jc->seconds[2], jc->seconds[3], jc->seconds[4]);
    return FHX_OK;
}

}  // namespace

extern "C" {

int fhx_jc_create(int device, fhx_jc** out) { return fhx::handle_create(device, out); }

void fhx_jc_destroy(fhx_jc* jc) {
    fhx::text_handle_destroy(jc, [&] { drop_all(jc); });
}

const char* fhx_jc_last_error(const fhx_jc* jc) { return fhx::handle_last_error(jc); }

int fhx_jc_reset(fhx_jc* jc) {
    if (!jc) return FHX_ERR_ARG;
    TH_HIP(jc, hipSetDevice(jc->device));
    TH_HIP(jc, hipStreamSynchronize(jc->stream));
    drop_all(jc);
    for (double& s : jc->seconds) s = 0;
    return FHX_OK;
}

int fhx_jc_convert_file(fhx_jc* jc, const char* path, const char* name1, const char* name2, int64_t resolution, int32_t id1, int32_t id2,
                        int32_t keep_text, int32_t keep_rows, int64_t* n_lines, int32_t* why, int64_t* bad_line) {
    if (!jc || !path || !n_lines || !why || !bad_line) return FHX_ERR_ARG;
    *n_lines = 0;
    *why = FHX_JC_OK;
    *bad_line = 0;
    if (!name_ok(name1) || !name_ok(name2)) return fhx::fail(jc, FHX_ERR_ARG, "a chromosome name must be 1 to 66 bytes of [A-Za-z0-9_.-]");
    if (resolution < 0 || resolution > 0x7fffffffll) return fhx::fail(jc, FHX_ERR_ARG, "the resolution must be 1 to 2^31 - 1 (0: verbatim mode)");
    if (keep_rows && resolution == 0) return fhx::fail(jc, FHX_ERR_ARG, "verbatim mode has no rows to keep");
    const int rc = convert_file(jc, path, name1, name2, resolution, id1, id2, keep_text, keep_rows, n_lines, why, bad_line);
    if (rc != FHX_OK) drop_all(jc);                                           // the one exit of a failed conversion, whatever failed
    return rc;
}

int fhx_jc_counts(const fhx_jc* jc, int64_t* n_lines, int64_t* n_rows, int64_t* n_bytes) {
    if (!jc) return FHX_ERR_ARG;
    if (n_lines) *n_lines = jc->n_lines;
    if (n_rows) *n_rows = jc->n_rows;
    if (n_bytes) *n_bytes = (int64_t)jc->text.size();
    return FHX_OK;
}

int fhx_jc_stage_seconds(const fhx_jc* jc, double* seconds) {
    if (!jc || !seconds) return FHX_ERR_ARG;
    for (int k = 0; k < FHX_JC_STAGES; ++k) seconds[k] = jc->seconds[k];
    return FHX_OK;
}

int fhx_jc_copy_text(const fhx_jc* jc, void* dst, int64_t capacity) {
    if (!jc || capacity < (int64_t)jc->text.size() || (!dst && !jc->text.empty())) return FHX_ERR_ARG;
    if (!jc->text.empty()) std::memcpy(dst, jc->text.data(), jc->text.size());
    return FHX_OK;
}

int fhx_jc_fetch_rows(fhx_jc* jc, int32_t* chr1, int32_t* mid1, int32_t* chr2, int32_t* mid2, int32_t* count) {
    if (!jc) return FHX_ERR_ARG;
    if (jc->n_rows > 0 && (!chr1 || !mid1 || !chr2 || !mid2 || !count)) return FHX_ERR_ARG;
    TH_HIP(jc, hipSetDevice(jc->device));
    int32_t* out[5] = {chr1, mid1, chr2, mid2, count};
    for (int k = 0; k < 5 && jc->n_rows > 0; ++k)
        TH_HIP(jc, hipMemcpyAsync(out[k], jc->d_col[k], (size_t)jc->n_rows * sizeof(int32_t), hipMemcpyDeviceToHost, jc->stream));
    TH_HIP(jc, hipStreamSynchronize(jc->stream));
    return FHX_OK;
}

void* fhx_jc_device_ptr(fhx_jc* jc, int32_t which) {
    if (!jc || which < 0 || which > 4 || jc->n_rows == 0) return nullptr;
    return jc->d_col[which];
}

void* fhx_jc_stream(fhx_jc* jc) { return jc ? (void*)jc->stream : nullptr; }

}  // extern "C"
