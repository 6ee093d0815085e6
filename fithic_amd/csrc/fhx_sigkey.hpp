// fhx_sigkey.hpp - the decision merge-filter.sh makes on the TEXT of field 7 (`$7 <= q` under mawk 1.3.4, LC_ALL=C), shared by the
// file route (fhx_sigselect.hip, fhx_sigtrack.inc, fhx_sigsplit.inc: ms_select, ut_select and mp_select read the field from the
// file's bytes) and the resident route (fhx_sigresident.hip: sr_decide formats q with fmt_e6 and reads the field from registers).
// All four kernels call classify() and decide(), and both routes make the threshold with fdr_of(), so the two cannot drift apart.
//
// A field in the shape C's %e writes, D.DDDDDDe[+-]XX[X], is
//   zero     every digit 0: the number 0, kept when 0 <= fdr (0 < fdr when strict) - the host says which
//   numeric  [2.225074e-308, 9.999999e+307]: awk compares numbers, and strtod is monotone in the integer key
//            (exponent, 7-digit mantissa): ONE integer compare with the bound the host found by bisection
//   string   a non-zero value below 2.225074e-308 or an exponent of 309 and more: awk's strtod flags ERANGE and
//            the field is compared bytewise with the text of fdr (memcmp, then length)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../include/fithic_mi355x.h"
#include "fhx_pairline.hpp"

namespace msd {

constexpr unsigned long long KEY_EXP = 10000000ull;      // key = (exponent + 308) * 10^7 + the seven digits

// the threshold as the shell passes it: its bytes for the string class, by value
struct Fdr {
    unsigned char text[FHX_MS_FDR_BYTES];
    int len;
};

// fdr_text[0, fdr_len) as the kernels take it; false, and *fdr untouched, unless it has 1 to FHX_MS_FDR_BYTES bytes
static inline bool fdr_of(const char* fdr_text, int32_t fdr_len, Fdr* fdr) {
    if (fdr_len < 1 || fdr_len > FHX_MS_FDR_BYTES) return false;
    std::memset(fdr, 0, sizeof(*fdr));
    std::memcpy(fdr->text, fdr_text, (size_t)fdr_len);
    fdr->len = fdr_len;
    return true;
}

using fhxpair::is_digit;

// Field 7 at text[b, b + len): 0 = not the %e shape (or one the classes leave out), 1 = zero, 2 = numeric (*key set), 3 = string.
__device__ inline int classify(const unsigned char* __restrict__ text, int64_t b, int len, unsigned long long* key) {
    if (len != 12 && len != 13) return 0;
    const int d0 = text[b];
    if (!is_digit(d0) || text[b + 1] != '.' || text[b + 8] != 'e') return 0;
    unsigned long long mant = (unsigned long long)(d0 - '0');
    for (int k = 2; k < 8; ++k) {
        const int c = text[b + k];
        if (!is_digit(c)) return 0;
        mant = mant * 10 + (unsigned long long)(c - '0');
    }
    const int sign = text[b + 9];
    if (sign != '+' && sign != '-') return 0;
    int ex = 0;
    for (int k = 10; k < len; ++k) {
        const int c = text[b + k];
        if (!is_digit(c)) return 0;
        ex = ex * 10 + (c - '0');
    }
    if (mant == 0) return 1;
    if (d0 == '0') return 0;                                                  // 0.000001e-03: not what %e writes
    if (sign == '-') ex = -ex;
    if (ex == 308) return 0;                                                  // numeric up to 1.797693e+308, a string above: left out
    if (ex > 308) return 3;
    if (ex < -308 || (ex == -308 && mant < 2225074ull)) return 3;
    *key = (unsigned long long)(ex + 308) * KEY_EXP + mant;
    return 2;
}

// awk's string comparison of the field with the text of fdr: memcmp over the common length, then the lengths
__device__ inline int compare_text(const unsigned char* __restrict__ text, int64_t b, int len, const Fdr& fdr) {
    const int common = len < fdr.len ? len : fdr.len;
    for (int k = 0; k < common; ++k) {
        const int a = text[b + k], q = fdr.text[k];
        if (a != q) return a < q ? -1 : 1;
    }
    return len < fdr.len ? -1 : (len > fdr.len ? 1 : 0);
}

// The decision on the field at text[b, b + len) that classify put into class cls with `key`: *keep set and 0, or FHX_MS_FIELD for
// class 0.  strict: `$7 < q` (the track) instead of `$7 <= q`; the host has made key_bound and zero_kept for the same operator.
__device__ inline int decide(int cls, unsigned long long key, unsigned long long key_bound, int zero_kept, int strict,
                             const unsigned char* __restrict__ text, int64_t b, int len, const Fdr& fdr, bool* keep) {
    if (cls == 0) return FHX_MS_FIELD;
    if (cls == 1) *keep = zero_kept != 0;
    else if (cls == 2) *keep = key <= key_bound;
    else {
        const int cmp = compare_text(text, b, len, fdr);
        *keep = strict ? cmp < 0 : cmp <= 0;
    }
    return 0;
}

}  // namespace msd
