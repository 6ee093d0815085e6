// fhx_k1key.hpp - one 32-bit key per contact row: all that k1_classify_hist needs of a row (inter-chromosomal or not, the distance
// in slots, the count) where the row's three int32 columns hold it in 12 bytes.  Written by k0_slots next to the columns, read by
// K1 in every pass.  Host and device code; no dependency but <cstdint> (tests/native/k1_key_check.cpp includes it alone).
//
//   bit 31      escape: the row does not fit - K1 loads its three columns as before.  Nothing is approximated.
//   bits 30..13 d = |loc1 - loc2| in slots (18 bits); all ones: an inter-chromosomal row (loc2 < 0)
//   bits 12..0  count (13 bits)
//
// A row escapes when its count is negative or >= 8192, or when it is an intra row with d >= 0x3FFFF (the all-ones pattern belongs
// to the inter rows).  5 kb bins put 49 847 slots on the longest human chromosome, and a Hi-C count of 8192 in one bin pair is a
// handful of rows next to the diagonal: both fields are generous for the data, and the escape keeps the rest exact.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FHX_K1KEY_FN __host__ __device__ inline
#else
#define FHX_K1KEY_FN inline
#endif

namespace fhx {
namespace k1key {

constexpr int COUNT_BITS = 13;
constexpr int D_BITS = 18;
constexpr uint32_t COUNT_LIMIT = 1u << COUNT_BITS;            // counts 0 .. 8191 are inline
constexpr uint32_t D_INTER = (1u << D_BITS) - 1u;             // 0x3FFFF: the d field of an inter row; intra d 0 .. 0x3FFFE are inline
constexpr uint32_t ESCAPE = 1u << 31;
static_assert(COUNT_BITS + D_BITS == 31, "31 payload bits under the escape bit");

struct Row {
    bool escape;      // the key holds nothing else: read the wide columns
    bool inter;
    int32_t d;        // intra rows only
    int32_t count;
};

// inter: the row is inter-chromosomal (d is ignored); d >= 0
FHX_K1KEY_FN uint32_t pack(bool inter, int64_t d, int32_t count) {
    if (count < 0 || (uint32_t)count >= COUNT_LIMIT) return ESCAPE;
    if (inter) return (D_INTER << COUNT_BITS) | (uint32_t)count;
    if (d < 0 || d >= (int64_t)D_INTER) return ESCAPE;
    return ((uint32_t)d << COUNT_BITS) | (uint32_t)count;
}

FHX_K1KEY_FN Row unpack(uint32_t key) {
    Row r;
    r.escape = (key & ESCAPE) != 0u;
    const uint32_t d = (key >> COUNT_BITS) & D_INTER;
    r.inter = d == D_INTER;
    r.d = (int32_t)d;
    r.count = (int32_t)(key & (COUNT_LIMIT - 1u));
    return r;
}

// the key of a row as the slot columns hold it: loc2 < 0 marks an inter row (k0_slots stores ~slot2)
FHX_K1KEY_FN uint32_t pack_row(int32_t loc1, int32_t loc2, int32_t count) {
    const int64_t diff = (int64_t)loc1 - (int64_t)loc2;
    return pack(loc2 < 0, diff < 0 ? -diff : diff, count);
}

}  // namespace k1key
}  // namespace fhx
