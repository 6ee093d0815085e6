// fhx_namerule.hpp - the chromosome names the per-chromosome split takes (reference: fithic/utils/merge-filter-parallelized.sh:21-25,
// where a name is a shell word, a directory and one side of awk's `$1 == c`): mergefilter_parallel.name_refusal on the device side.
// Shared by the file route (fhx_sigsplit.inc: mp_select applies it to tokens 1 and 3 of every line) and the resident route
// (fhx_sigresident_split.inc: the names are known before any kernel runs, so the host applies it once per chromosome id and the
// kernels look the reason up), so that the two refuse the same names for the same reason.
#pragma once
#include "../../include/fithic_mi355x.h"
#include "fhx_fmt.hpp"

namespace fhx {
namespace namerule {

constexpr int NAME_STRIDE = FHX_MS_SPLIT_NAME_BYTES;       // a name of up to 63 bytes, and room for its length

FHX_HD bool digit(int c) { return c >= '0' && c <= '9'; }
FHX_HD bool letter(int c) { return (c | 0x20) >= 'a' && (c | 0x20) <= 'z'; }

// A name awk compares with another accepted name as STRINGS, and a shell word takes as it is: 0 or the reason.  Precedence: the
// length, then the bytes, then what strtod might make of a name that starts with a digit.
FHX_HD int name_grammar(const unsigned char* s, int n) {
    if (n > NAME_STRIDE - 1) return FHX_MS_NAME;
    bool all_digits = true, certain = false;                                  // certain: strtod cannot consume the name whole
    for (int k = 0; k < n; ++k) {
        const int c = s[k];
        const bool l = letter(c), d = digit(c);
        if (!l && !d && c != '_' && c != '.' && c != '-') return FHX_MS_NAME_BYTES;
        if (k == 0 && !l && !d && c != '_') return FHX_MS_NAME_BYTES;
        all_digits &= d;
        if (c == '_') certain = true;
        if (l) {
            const int lower = c | 0x20;
            if (!(lower >= 'a' && lower <= 'f') && lower != 'x' && lower != 'p') certain = true;
        }
    }
    if (n < 1) return FHX_MS_NAME_BYTES;
    if (!digit(s[0])) return 0;
    if (all_digits) return (n <= 15 && (n == 1 || s[0] != '0')) ? 0 : FHX_MS_NAME_NUMERIC;
    return certain ? 0 : FHX_MS_NAME_NUMERIC;
}

}  // namespace namerule
}  // namespace fhx
