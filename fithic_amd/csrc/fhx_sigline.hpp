// fhx_sigline.hpp - one line of a significances file on the device, as the kernels of fhx_sigselect.hip, fhx_sigtrack.inc and
// fhx_sigsplit.inc read it: the bytes the grammar refuses, the walk that splits a line on blanks, the rounds of WG lines a block
// is worked in, and the gather that copies kept lines with lanes on consecutive OUTPUT bytes.  The decision on field 7 is
// fhx_sigkey.hpp's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/fithic_mi355x.h"
#include "fhx_textlines.hpp"

namespace msd {

__device__ inline bool refused_byte(unsigned int c) { return c < 0x20u ? (c != '\t' && c != '\n') : c >= 0x7fu; }

struct GrammarBytes {                          // scan_text's policy
    static __device__ void check(bool& bad, unsigned int c, const unsigned char*, int64_t, int64_t) { bad |= refused_byte(c); }
};

// one line split on blanks: tokens 1 to 4 and field 7, relative to the line's first byte
struct Line {
    int why, tok, len;                         // len: without the newline
    int b1, n1, b2, n2, b3, n3, b4, n4, fb, fn;
};

// check_bytes: scan_text saw a refused byte in the batch, so the bytes are looked at one by one.  Tokens = false records field 7
// only (b1 ... n4 stay 0): with all five recorded the compiler keeps L in scratch memory (44 bytes a lane, also when the caller
// never reads tokens 1 to 4), and ms_select, which reads nothing but field 7, does not pay for that
// (profiles/r12/text_paths_resources.txt).
template <bool Tokens = true>
__device__ inline void walk(const unsigned char* __restrict__ text, int64_t T, int64_t start, int check_bytes, Line& L) {
    L.why = 0;
    L.b1 = L.n1 = L.b2 = L.n2 = L.b3 = L.n3 = L.b4 = L.n4 = L.fb = L.fn = 0;
    int tok = 0, begin = 0, k = 0;
    bool in_tok = false;
    auto close = [&](int end) {
        const int n = end - begin;
        if (Tokens && tok == 1) { L.b1 = begin; L.n1 = n; }
        else if (Tokens && tok == 2) { L.b2 = begin; L.n2 = n; }
        else if (Tokens && tok == 3) { L.b3 = begin; L.n3 = n; }
        else if (Tokens && tok == 4) { L.b4 = begin; L.n4 = n; }
        else if (tok == 7) { L.fb = begin; L.fn = n; }
    };
    for (;; ++k) {
        const int64_t p = start + k;
        const int c = p < T ? (int)text[p] : '\n';                            // the end of the text ends the line
        if (c == '\n') break;
        if (k >= fhxlines::MAX_LINE) {
            L.why = FHX_MS_LONG_LINE;
            break;
        }
        if (check_bytes && refused_byte((unsigned int)c)) {
            L.why = FHX_MS_BYTES;
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
    L.len = k;
}

// the lines of a block in rounds of WG: entry e of the round's lane, its line number in the batch, whether both exist
struct Round {
    int e;
    int64_t r;
    bool valid;
};
__device__ inline Round round_of(int base, int n_lines, int64_t row0, int64_t n_lines_batch) {
    Round q;
    q.e = base + (int)threadIdx.x;
    q.r = row0 + q.e;
    q.valid = q.e < n_lines && q.r < n_lines_batch;
    return q;
}

// The kept bytes of one round of N entries (N = the workgroup's lanes) -> out[at, at + total), dense and in order.  pre[t] is the
// exclusive prefix of the entries' kept lengths and pre[N] = total their sum (in LDS, written before a barrier); start_of(t) is where
// entry t begins in the text.  Lanes are assigned by OUTPUT byte and find their entry by a binary search in the prefixes, so
// stores are coalesced at 1 % kept and at 100 %.  A final line without its newline gets one, as awk's print gives it.
template <int N, typename StartOf>
__device__ inline void gather_round(const unsigned char* __restrict__ text, int64_t T, const unsigned int* pre, unsigned int total,
                                    StartOf start_of, int64_t at, unsigned char* __restrict__ out, int64_t out_capacity) {
    for (unsigned int j = threadIdx.x; j < total; j += N) {
        int lo = 0, hi = N;                                 // the last t with pre[t] <= j: an entry that keeps nothing shares its prefix
        while (hi - lo > 1) {                               // with the next one, so the last of equals is the entry that holds byte j
            const int mid = (lo + hi) >> 1;
            if (pre[mid] <= j) lo = mid;
            else hi = mid;
        }
        const int64_t src = start_of(lo) + (int64_t)(j - pre[lo]);
        const unsigned char c = src < T ? text[src] : (unsigned char)'\n';   // the newline the last line lacked
        if (at + j < out_capacity) out[at + j] = c;
    }
}

}  // namespace msd
