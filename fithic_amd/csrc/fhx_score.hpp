// fhx_score.hpp - the two score fields of a UCSC interact line, `int(-log($7)/log(10))` and `-log($7)/log(10)` as mawk 1.3.4
// prints them (reference: fithic/utils/visualize-UCSC.sh:18), usable on the host AND in a kernel (csrc/fhx_sigtrack.inc).
//
// awk computes  v_awk = fl( fl(-log(strtod(field))) / fl(log 10) )  with the host's libm and prints a number as "%d" when it is
// integral and below 2^31 in magnitude, through "%.6g" otherwise; int() truncates toward zero and -0 prints as 0.  The text
// depends on libm to the last bit wherever v_awk lies next to an integer or next to a rounding boundary of %.6g, so a kernel
// never guesses: certified() writes the two fields from an approximation T only when every value within eps(T) of T prints
// the same bytes, and returns 0 otherwise - the row is then DEFERRED to host_fields(), which makes mawk's own calls.
//
// eps: the field is D.DDDDDDe[+-]XX = m * 10^(x-6) with the integer 10^6 <= m < 10^7, and t = -log10 of that decimal is
// (6 - x) - log10(m).  The kernel computes  T = fl( (6 - x) - fl_dev(log10(m)) ):
//   * m and 6 - x are exact doubles.  log10(m) lies in [6, 7), where one ulp is 8.9e-16; HIP's math reference gives the device's
//     double log10 a maximal error of 1 ulp, and 4 ulp are assumed here:                            |.| <= 3.6e-15
//   * the subtraction rounds once:                                                                  |.| <= 2^-53 |T|
// and awk's value differs from t by
//   * strtod: the nearest double of the decimal, a relative 2^-53 in q, which is an ABSOLUTE 2^-53 in log q and 2^-53 / ln 10 in
//     the score - for q next to 1 (9.999999e-01, t = 4.3e-8) that is a relative 1e-9 of the score, which is why it is kept as
//     an absolute term:                                                                             |.| <= 4.9e-17
//   * libm's log, below 1 ulp:                                                                      |.| <= 2^-52 |t|
//   * log 10 rounded to a double (2^-53), and the division rounded once (2^-53):                    |.| <= 2^-52 |t|
// Together |T - v_awk| <= 3.7e-15 + 5.6e-16 |T|.  EPS_ABS and EPS_REL are 27 and 17 times those: generosity only costs
// deferrals, about 2 eps / (the width of a %.6g cell) per row, 1e-7 and less for the scores of a Fit-Hi-C run.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fhx_fmt.hpp"

namespace fhx {
namespace score {

constexpr double EPS_ABS = 1e-13;
constexpr double EPS_REL = 1e-14;
constexpr int MAX_TEXT = 24;                   // "-323 -4.34295e-08" and the like, both fields and the blank between them

// "%.6g" of +-(D / 10^5) * 10^e10 for a six-digit D (100000..999999) and -9 <= e10 <= 5: C's rules - scientific when the
// exponent is below -4, trailing zeros and a bare point dropped
FHX_HD int put_g6(char* dst, bool neg, int D, int e10) {
    char d[6];
    for (int k = 5; k >= 0; --k) {
        d[k] = (char)('0' + D % 10);
        D /= 10;
    }
    int nd = 6;
    while (nd > 1 && d[nd - 1] == '0') --nd;
    int n = 0;
    if (neg) dst[n++] = '-';
    if (e10 < -4) {
        dst[n++] = d[0];
        if (nd > 1) dst[n++] = '.';
        for (int k = 1; k < nd; ++k) dst[n++] = d[k];
        dst[n++] = 'e';
        dst[n++] = '-';
        dst[n++] = (char)('0' + (-e10) / 10);
        dst[n++] = (char)('0' + (-e10) % 10);
    } else if (e10 >= 0) {
        for (int k = 0; k <= e10; ++k) dst[n++] = d[k];
        if (nd > e10 + 1) dst[n++] = '.';
        for (int k = e10 + 1; k < nd; ++k) dst[n++] = d[k];
    } else {
        dst[n++] = '0';
        dst[n++] = '.';
        for (int k = 1; k < -e10; ++k) dst[n++] = '0';
        for (int k = 0; k < nd; ++k) dst[n++] = d[k];
    }
    return n;
}

// The two fields and the blank between them for a score known as T +- (EPS_ABS + EPS_REL |T|), into dst (MAX_TEXT bytes);
// 0 when the interval is not inside one cell of the truncation and one cell of %.6g, or T is outside [1e-8, 1000) in magnitude.
FHX_HD int certified(char* dst, double T) {
    const double x = std::fabs(T);
    if (!(x >= 1e-8 && x < 1000.0)) return 0;                                 // a nan fails the comparison
    const double eps = EPS_ABS + EPS_REL * x;
    const double whole = std::floor(x);
    if (x - eps <= whole || x + eps >= whole + 1.0) return 0;                 // an integer, 0 included, lies within reach
    // 10^e10 <= x < 10^(e10 + 1), and scale = 10^(5 - e10), an exact double.  A power of ten that is no integer is itself
    // rounded here: next to it either choice of e10 gives the same text, and the cell check below holds for both
    int e10;
    double scale;
    if (x >= 100.0) { e10 = 2; scale = 1e3; }
    else if (x >= 10.0) { e10 = 1; scale = 1e4; }
    else if (x >= 1.0) { e10 = 0; scale = 1e5; }
    else if (x >= 1e-1) { e10 = -1; scale = 1e6; }
    else if (x >= 1e-2) { e10 = -2; scale = 1e7; }
    else if (x >= 1e-3) { e10 = -3; scale = 1e8; }
    else if (x >= 1e-4) { e10 = -4; scale = 1e9; }
    else if (x >= 1e-5) { e10 = -5; scale = 1e10; }
    else if (x >= 1e-6) { e10 = -6; scale = 1e11; }
    else if (x >= 1e-7) { e10 = -7; scale = 1e12; }
    else { e10 = -8; scale = 1e13; }
    const double s = x * scale;                                               // one rounding, s < 10^6 + 1
    const double r = std::floor(s + 0.5);
    if (r < 100000.0 || r > 1000000.0) return 0;
    // the cell of r at this scale is (r - 1/2, r + 1/2); below 10^e10 the digits are ten times as fine, so the cell of 100000
    // reaches down only 1/20
    const double reach = eps * scale + s * 2.3e-16;
    const double below = r == 100000.0 ? 0.05 : 0.5;
    if (s - reach <= r - below || s + reach >= r + 0.5) return 0;
    int D = (int)r;
    if (D == 1000000) {
        D = 100000;
        ++e10;
    }
    int n = 0;
    if (T < 0 && whole > 0) dst[n++] = '-';                                   // int() of (-1, 0) is -0, which prints as 0
    n += fmt::put_u64(dst + n, (unsigned long long)whole);
    dst[n++] = ' ';
    return n + put_g6(dst + n, T < 0, D, e10);
}

// T of a numeric-class field: the seven digits as one integer m (10^6 <= m < 10^7) and the decimal exponent x
FHX_HD double approximate(unsigned long long m, int x) { return (double)(6 - x) - ::log10((double)m); }

// a number as mawk's print writes it
inline int put_awk_number(char* dst, double d) {
    if (d > -2147483648.0 && d < 2147483648.0 && d == (double)(long long)d) return std::snprintf(dst, 16, "%lld", (long long)d);
    return std::snprintf(dst, 16, "%.6g", d);
}

// The deferred route: the two fields and the blank between them for the field text (at most 15 bytes), with the calls mawk makes -
// strtod, log, the division by log(10), the truncation, its number printing.  `ten` is volatile so that log(10) is libm's at run
// time, not the compiler's.
inline int host_fields(const char* field, int len, char* dst) {
    char buf[16];
    len = len < 0 ? 0 : (len > 15 ? 15 : len);
    std::memcpy(buf, field, (size_t)len);
    buf[len] = 0;
    const double q = std::strtod(buf, nullptr);
    volatile double ten = 10.0;
    const double v = -std::log(q) / std::log(ten);
    int n = put_awk_number(dst, v >= 0 ? std::floor(v) : std::ceil(v));
    dst[n++] = ' ';
    return n + put_awk_number(dst + n, v);
}
}  // namespace score
}  // namespace fhx
