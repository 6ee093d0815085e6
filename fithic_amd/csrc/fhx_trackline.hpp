// fhx_trackline.hpp - one line of the UCSC interact track (reference: fithic/utils/visualize-UCSC.sh:18), from its pieces:
// (name 1, midpoint 1, name 2, midpoint 2, the class and key of field 7, NR) ->
//   $1 ($2-1) ($4+1) NR int(-log($7)/log(10)) -log($7)/log(10) EXP 0 $1 ($2-1) ($2+1) SOURCE_NAME . $3 ($4-1) ($4+1) TARGET_NAME +
// Shared by the file route (fhx_sigtrack.inc: the pieces are tokens of a line of text) and the resident route (fhx_sigresident.hip:
// the pieces are a row's identity and the %e text of its q), so that the two give the same bytes by construction: the grammar
// beyond field 7 and its precedence, the length of a line, the DEFERRED marking, the round trip of a deferred score through
// fhx::score::host_fields and the writer of the line exist here and nowhere else.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "fhx_fmt.hpp"
#include "fhx_score.hpp"
#include "fhx_sigkey.hpp"

namespace fhx {
namespace trackline {

constexpr int NAME_BYTES = 63;                 // tokens 1 and 3
constexpr int MID_DIGITS = 9;                  // tokens 2 and 4: v + 1 stays below 2^31, where awk prints integers as integers
constexpr int MID_LIMIT = 1000000000;          // the values MID_DIGITS digits reach
constexpr int DEFER_IN = 16, DEFER_OUT = 32;   // bytes per deferred line, to the host and back (byte 0: the length)
constexpr unsigned int DEFERRED = 0x8000u;     // in a line's info word; the low 15 bits are a length (0: dropped)
constexpr int FIXED_BYTES = 45;                // 16 blanks and the newline, EXP 0 SOURCE_NAME . TARGET_NAME +
// the longest line of two names of `name_bytes` each: three names, -1 / +1 of two nine-digit midpoints (ten digits at most for
// a +1, three of them), NR below 2^31, the longest score
constexpr int max_line(int name_bytes) { return FIXED_BYTES + 3 * name_bytes + 3 * 9 + 3 * 10 + 10 + score::MAX_TEXT; }

const char HEAD[] =
    "track type=interact name=\"Your_Fit-Hi-C_Interactions\" description=\"Fit-Hi-C_Interactions\" interactDirectional=true useScore=on "
    "maxHeightPixels=50:100:200 visibility=full\n"
    "#chrom  chromStart  chromEnd  name  score  value  exp  color  sourceChrom  sourceStart  sourceEnd  sourceName  sourceStrand  targetChrom  "
    "targetStart  targetEnd  targetName  targetStrand\n";

// 1 to 9 digits -> their value, -1 otherwise
__device__ inline int midpoint(const unsigned char* __restrict__ text, int64_t b, int n) {
    if (n < 1 || n > MID_DIGITS) return -1;
    int v = 0;
    for (int k = 0; k < n; ++k) {
        const int c = text[b + k];
        if (!msd::is_digit(c)) return -1;
        v = v * 10 + (c - '0');
    }
    return v;
}

// the same rule for a midpoint held as a number: what %d prints of it is 1 to 9 digits without a sign
__device__ inline bool midpoint_ok(int v) { return v >= 0 && v < MID_LIMIT; }

__device__ inline int digits_of(long long v) {                                // of the decimal text, a minus sign included
    int n = v < 0 ? 2 : 1;
    unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
    while (u >= 10ull) {
        u /= 10ull;
        ++n;
    }
    return n;
}

// The reason a parsed line is refused for, 0 for none.  A line with several faults reports the first of: field 7 outside the
// classes, a midpoint, a name.
__device__ inline int refusal(int cls, bool midpoints_ok, int n1, int n3) {
    if (cls == 0) return FHX_MS_FIELD;
    if (!midpoints_ok) return FHX_MS_MIDPOINT;
    if (n1 > NAME_BYTES || n3 > NAME_BYTES) return FHX_MS_NAME;
    return 0;
}

// The two score fields of a kept line into score (score::MAX_TEXT bytes) -> their length; 0: the line is DEFERRED.  The zero
// class is `inf inf`; a numeric field is written where the error bound certifies it; the string class always goes to the host.
__device__ inline int score_text(int cls, unsigned long long key, char* score) {
    if (cls == 2) return score::certified(score, score::approximate(key % msd::KEY_EXP, (int)(key / msd::KEY_EXP) - 308));
    if (cls == 3) return 0;
    score[0] = score[4] = 'i', score[1] = score[5] = 'n', score[2] = score[6] = 'f', score[3] = ' ';
    return 7;
}

// a kept line's info word: its length without NR (and, when DEFERRED, without its score)
__device__ inline unsigned int line_word(int n1, int n3, int v2, int v4, int score_len) {
    const unsigned int word = (unsigned int)(FIXED_BYTES + 2 * n1 + n3 + 2 * digits_of((long long)v2 - 1) + digits_of((long long)v2 + 1) +
                                             digits_of((long long)v4 - 1) + 2 * digits_of((long long)v4 + 1) + score_len);
    return score_len == 0 ? word | DEFERRED : word;
}

// field 7 of a deferred line into its slot for the host
__device__ inline void defer_field(unsigned char* __restrict__ fields, int64_t slot, const unsigned char* __restrict__ field, int fn) {
    for (int k = 0; k < DEFER_IN; ++k) fields[slot * DEFER_IN + k] = k < fn && k < DEFER_IN - 1 ? field[k] : (unsigned char)0;
}

// the info word completed: + the digits of NR, + the host's score bytes of a deferred line
__device__ inline unsigned int final_word(unsigned int word, long long nr, const unsigned char* __restrict__ scores, int64_t slot, int64_t n_slots) {
    unsigned int len = (word & ~DEFERRED) + (unsigned int)digits_of(nr);
    if ((word & DEFERRED) && slot < n_slots) len += scores[slot * DEFER_OUT];
    return len | (word & DEFERRED);
}

// the host's answer for a deferred line into score -> its length
__device__ inline int host_score(const unsigned char* __restrict__ scores, int64_t slot, int64_t n_slots, char* score) {
    int n = 0;
    if (slot < n_slots) {
        n = min((int)scores[slot * DEFER_OUT], DEFER_OUT - 1);
        for (int k = 0; k < n && k < score::MAX_TEXT; ++k) score[k] = (char)scores[slot * DEFER_OUT + 1 + k];
    }
    return min(n, score::MAX_TEXT);
}

// The line through sink.put(byte), newline included.
template <typename Sink>
__device__ inline void put_bytes(Sink& s, const unsigned char* __restrict__ src, int n) {
    for (int k = 0; k < n; ++k) s.put(src[k]);
}
template <typename Sink>
__device__ inline void put_literal(Sink& s, const char* t) {
    for (; *t; ++t) s.put(*t);
}
template <typename Sink>
__device__ inline void put_number(Sink& s, long long v) {
    char tmp[24];
    const int n = fhx::fmt::put_i64(tmp, v);
    for (int k = 0; k < n; ++k) s.put(tmp[k]);
}
template <typename Sink>
__device__ inline void write_line(Sink& s, const unsigned char* __restrict__ name1, int n1, int v2, const unsigned char* __restrict__ name3, int n3,
                                  int v4, long long nr, const char* score, int score_len) {
    put_bytes(s, name1, n1);
    s.put(' ');
    put_number(s, (long long)v2 - 1);
    s.put(' ');
    put_number(s, (long long)v4 + 1);
    s.put(' ');
    put_number(s, nr);
    s.put(' ');
    put_bytes(s, (const unsigned char*)score, score_len);
    put_literal(s, " EXP 0 ");
    put_bytes(s, name1, n1);
    s.put(' ');
    put_number(s, (long long)v2 - 1);
    s.put(' ');
    put_number(s, (long long)v2 + 1);
    put_literal(s, " SOURCE_NAME . ");
    put_bytes(s, name3, n3);
    s.put(' ');
    put_number(s, (long long)v4 - 1);
    s.put(' ');
    put_number(s, (long long)v4 + 1);
    put_literal(s, " TARGET_NAME +\n");
}

// The host's half of the round trip: for n_slots fields of DEFER_IN bytes the two score fields as mawk's own calls make them,
// DEFER_OUT bytes a slot (byte 0: the length).  False when a field has no score text.
inline bool answer_deferred(const unsigned char* fields, int64_t n_slots, std::vector<unsigned char>* scores) {
    scores->assign((size_t)(n_slots * DEFER_OUT), 0);
    for (int64_t k = 0; k < n_slots; ++k) {
        const char* f = (const char*)fields + k * DEFER_IN;
        char text[score::MAX_TEXT + 8];
        const int got = score::host_fields(f, (int)strnlen(f, DEFER_IN - 1), text);
        if (got < 3 || got > score::MAX_TEXT) return false;
        (*scores)[(size_t)(k * DEFER_OUT)] = (unsigned char)got;
        std::memcpy(scores->data() + k * DEFER_OUT + 1, text, (size_t)got);
    }
    return true;
}

}  // namespace trackline
}  // namespace fhx
