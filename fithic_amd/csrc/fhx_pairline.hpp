// fhx_pairline.hpp - the device side of one allValidPairs line (`read chr1 pos1 strand1 chr2 pos2 ...`, split on blanks), shared
// by fhx_validpairs.hip (vp_parse) and fhx_fragpairs.hip (fp_parse); is_digit also serves fhx_juicer.hip and fhx_sigkey.hpp.
//
//   Line       what one pass over a line finds: how many tokens it holds and where tokens 2, 3, 5 and 6 lie
//   walk       that pass (fp_parse), with why it stopped early, if it did.  vp_parse carries its `chrM` search in the same pass and
//              has the loop written out in place over a Line: called as a function - with the search as a per-byte hook, by
//              value, through a reference or inlined by force - the walk cost vp_parse 4 to 5 % of its stage and fp_parse
//              nothing (profiles/r14/cells_layer_resources.txt, cells_layer_ab.txt).  A change to the grammar of a line is
//              made in both.
//   position   1 to 10 digits -> the value
//
// What a path makes of a stop (its own reason code, its own way of reporting the error word) stays with the path.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fhx_textlines.hpp"

namespace fhxpair {

__device__ inline bool is_digit(int c) { return c >= '0' && c <= '9'; }

// digits (1..10 of them) at text[b, b + len) -> the value; false for anything else
__device__ inline bool position(const unsigned char* __restrict__ text, int64_t b, int len, long long* out) {
    if (len < 1 || len > 10) return false;
    long long v = 0;
    for (int k = 0; k < len; ++k) {
        const int c = text[b + k];
        if (!is_digit(c)) return false;
        v = v * 10 + (c - '0');
    }
    *out = v;
    return true;
}

enum Stop { STOP_NONE = 0, STOP_LONG_LINE, STOP_BYTES };   // why walk() left the line before its end

struct Line {
    int tok = 0;                                            // tokens seen
    Stop stop = STOP_NONE;
    int64_t tb[4] = {0, 0, 0, 0}, te[4] = {0, 0, 0, 0};     // tokens 2, 3, 5, 6: text[tb, te)
    __device__ int len(int k) const { return (int)(te[k] - tb[k]); }
};

// The line that begins at text[start]: it ends at \n, \r\n or the end of the text; MAX_LINE bytes without an end, or a NUL,
// a control byte but tab (a lone \r among them), DEL or a non-ASCII byte stop the walk.
__device__ inline Line walk(const unsigned char* __restrict__ text, int64_t T, int64_t start) {
    Line L;
    bool in_tok = false;
    int64_t p = start;
    for (;; ++p) {
        const int c = p < T ? (int)text[p] : '\n';                    // the end of the text ends the line
        if (c == '\n') break;
        if (p - start >= fhxlines::MAX_LINE) {
            L.stop = STOP_LONG_LINE;
            break;
        }
        if (c == '\r' && p + 1 < T && text[p + 1] == '\n') break;     // \r\n
        if (c < 0x20 ? c != '\t' : c >= 0x7f) {
            L.stop = STOP_BYTES;
            break;
        }
        const bool blank = c == ' ' || c == '\t';
        if (!blank && !in_tok) {
            in_tok = true;
            ++L.tok;
            if (L.tok == 2) L.tb[0] = p;
            if (L.tok == 3) L.tb[1] = p;
            if (L.tok == 5) L.tb[2] = p;
            if (L.tok == 6) L.tb[3] = p;
        } else if (blank && in_tok) {
            in_tok = false;
            if (L.tok == 2) L.te[0] = p;
            if (L.tok == 3) L.te[1] = p;
            if (L.tok == 5) L.te[2] = p;
            if (L.tok == 6) L.te[3] = p;
        }
    }
    if (in_tok) {
        if (L.tok == 2) L.te[0] = p;
        if (L.tok == 3) L.te[1] = p;
        if (L.tok == 5) L.te[2] = p;
        if (L.tok == 6) L.te[3] = p;
    }
    return L;
}

}  // namespace fhxpair
