// k1_key_check.cpp - stand-alone check of fithic_amd/csrc/fhx_k1key.hpp (tests/test_k1_key_host.py compiles and runs it, with
// -fsanitize=undefined,address): for every (inter, d, count) tried, the key either carries the escape bit or unpacks to exactly
// what was packed; and whether it escapes is what the header's rule says, no more and no less.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "fhx_k1key.hpp"

namespace k = fhx::k1key;

static long long g_checked = 0, g_escaped = 0;

static bool must_escape(bool inter, int64_t d, int32_t count) {
    return count < 0 || count >= 8192 || (!inter && d >= 0x3FFFF);
}

static void fail(const char* what, bool inter, int64_t d, int32_t count, uint32_t key) {
    std::fprintf(stderr, "k1_key_check: %s: inter=%d d=%lld count=%d key=0x%08x\n", what, (int)inter, (long long)d, (int)count, key);
    std::exit(1);
}

static void check(bool inter, int64_t d, int32_t count) {
    const uint32_t key = k::pack(inter, d, count);
    const k::Row r = k::unpack(key);
    ++g_checked;
    if (r.escape != must_escape(inter, d, count)) fail("escape rule", inter, d, count, key);
    if (r.escape) {
        ++g_escaped;
        return;
    }
    if (r.inter != inter) fail("inter flag", inter, d, count, key);
    if (r.count != count) fail("count", inter, d, count, key);
    if (!inter && (int64_t)r.d != d) fail("distance", inter, d, count, key);
}

// the same through the slot columns: loc2 < 0 marks an inter row
static void check_row(int32_t loc1, int32_t loc2, int32_t count) {
    const uint32_t key = k::pack_row(loc1, loc2, count);
    const bool inter = loc2 < 0;
    const int64_t diff = (int64_t)loc1 - (int64_t)loc2, d = diff < 0 ? -diff : diff;
    if (key != k::pack(inter, d, count)) fail("pack_row", inter, d, count, key);
    check(inter, d, count);
}

int main() {
    const int32_t counts[] = {-1, 0, 1, 8190, 8191, 8192, 8193, INT32_MAX, INT32_MIN};
    const int64_t dists[] = {0, 1, 0x3FFFE, 0x3FFFF, 0x40000, 0x40001, INT32_MAX};
    for (int32_t c : counts) {
        for (int64_t d : dists) {
            check(false, d, c);
            check(true, d, c);                                   // an inter row's d is ignored
        }
    }
    // inter rows with small and large counts, as the columns hold them (loc2 = ~slot)
    for (int32_t c : {0, 1, 7, 8191, 8192, 100000, INT32_MAX}) {
        check_row(0, ~0, c);
        check_row(5, ~123456, c);
        check_row(INT32_MAX, ~INT32_MAX, c);
        check_row(0, INT32_MIN, c);
    }
    // the widest intra rows
    check_row(0, INT32_MAX, 1);
    check_row(INT32_MAX, 0, 1);
    check_row(INT32_MAX, INT32_MAX, 8191);
    // 10^6 random triples (xorshift64*): raw 32-bit patterns, and rows shaped like Hi-C rows so that most of them stay inline
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto next = [&]() {
        s ^= s >> 12;
        s ^= s << 25;
        s ^= s >> 27;
        return s * 0x2545F4914F6CDD1Dull;
    };
    for (int i = 0; i < 1000000; ++i) {
        const uint64_t a = next(), b = next();
        if (i & 1) {
            check_row((int32_t)(uint32_t)a, (int32_t)(uint32_t)(a >> 32), (int32_t)(uint32_t)b);
        } else {
            const int32_t l1 = (int32_t)(a % 3000000u), span = (int32_t)((a >> 32) % 300000u), c = (int32_t)(b % 9000u);
            const bool inter = ((b >> 40) & 7u) == 0u;
            check_row(l1 + span, inter ? ~l1 : l1, c);
        }
    }
    if (g_escaped == 0 || g_escaped == g_checked) {
        std::fprintf(stderr, "k1_key_check: %lld of %lld escaped: the cases do not cover both sides\n", g_escaped, g_checked);
        return 1;
    }
    std::printf("k1_key_check ok: %lld triples, %lld escaped\n", g_checked, g_escaped);
    return 0;
}
