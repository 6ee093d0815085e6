// fhx_inflate.inc - gzip members inflated ON THE GPU (included by fhx_device.hip inside its extern "C" block, which is closed
// here and reopened by fhx_ingest.inc; used by fhx_ingest_contacts_file).
//
// A deflate stream is serial, a file of many members is not: the library's own writers cut a table into members of 2^18 rows
// (1 MB compressed, 8 MB of text) and bgzip into 64 KB blocks, each carrying its size.  The host inflates such a file with one
// zlib per core - 0.5 s for the 4.6 GB of C3 on the 16 cores the GPU box grants, then 0.1 s to copy the text to HBM and 0.2 s to
// give the pages back.  Here the COMPRESSED file (0.6 GB) is uploaded and one wave per member decodes it into the text buffer
// the parser kernels read; several hundred members are in flight at once.
//
//   gz_inflate   one 64-lane workgroup per member.  Control flow is wave-uniform: every lane carries the same bit buffer and
//                decodes the same symbol (table entries pass through readfirstlane, so the decoder state lives in scalar
//                registers); what the lanes share out is the data movement - the stream is held 64 words at a time in one
//                vector register (a refill is a v_readlane), a match of up to 258 bytes is copied by all lanes at once out of a
//                32 KB window kept in LDS, and the window leaves for HBM 16 KB at a time as 16-byte stores.  Huffman tables
//                (RFC 1951: stored, fixed and dynamic blocks) live in LDS: one read of a 1024-entry table resolves a
//                literal/length code of up to 10 bits together with its base value and extra-bit count (longer codes: the
//                canonical count walk of zlib's puff.c), and the read for the next symbol is issued before the bytes of the
//                current one move.
//   gz_crc       CRC-32 of every member's text (256 threads per member, each a contiguous span; spans are combined with the
//                x^(8n) mod p algebra the writer uses, fhx_deflate.hpp) compared with the member's trailer.
//
// Every malformed stream ends in an error code, never in a wild store: output and input positions are bounded before each
// write / refill, distances are checked against the bytes produced.  Any error, a CRC or a size mismatch makes the caller fall
// back to zlib on the host, which reports what the reference's gzip module would.

}  // extern "C"

namespace fhx {
namespace gzdev {

constexpr int WIN = 32768;
constexpr int FLUSH = 16384;
constexpr int FAST_L = 10;
constexpr int FAST_D = 8;

struct Job {
    unsigned long long src;          // byte offset of the deflate stream in the uploaded file
    unsigned long long dst;          // byte offset of the member's text in the text buffer
    unsigned int src_len;            // deflate stream bytes (member minus header and the 8-byte trailer)
    unsigned int dst_len;            // ISIZE
    unsigned int crc;                // CRC-32 of the trailer
    unsigned int pad;
};

enum : int { E_NONE = 0, E_BLOCK_TYPE = 1, E_STORED = 2, E_TABLE = 3, E_SYMBOL = 4, E_DISTANCE = 5, E_OUTPUT = 6, E_INPUT = 7, E_SIZE = 8, E_CRC = 9 };

// Table entries (one LDS read resolves a code AND what follows it):
//   literal/length: bits 0-3 code length (0 = longer than FAST_L bits), 4-7 extra bits, 8-9 kind (0 literal, 1 length, 2 end of
//                   block, 3 not a symbol of the alphabet), 16-31 the byte or the length base
//   distance:       bits 0-3 code length, 4-7 extra bits, 8-9 kind (0 distance, 3 not a symbol), 16-31 the distance base
struct Lds {
    __attribute__((aligned(16))) unsigned char win[WIN];
    unsigned int lit_fast[1 << FAST_L];
    unsigned int dist_fast[1 << FAST_D];
    unsigned short lit_sym[288], dist_sym[32];   // symbols ordered by code (puff.c's `symbol`)
    unsigned short lit_cnt[16], dist_cnt[16];    // codes per length
    unsigned short offs[16];
    unsigned char lens[320];
};

__device__ inline unsigned int uni(unsigned int v) { return (unsigned int)__builtin_amdgcn_readfirstlane((int)v); }

__device__ const unsigned short kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__device__ const unsigned char kLenBits[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__device__ const unsigned short kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
                                                 4097, 6145, 8193, 12289, 16385, 24577};
__device__ const unsigned char kDistBits[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__device__ const unsigned char kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

enum : int { ALPHA_RAW = 0, ALPHA_LIT = 1, ALPHA_DIST = 2 };
__device__ inline unsigned int entry_of(int alphabet, unsigned int s, unsigned int len) {
    if (alphabet == ALPHA_LIT) {
        if (s < 256) return (s << 16) | len;
        if (s == 256) return (2u << 8) | len;
        if (s >= 286) return (3u << 8) | len;
        return ((unsigned int)kLenBase[s - 257] << 16) | (1u << 8) | ((unsigned int)kLenBits[s - 257] << 4) | len;
    }
    if (alphabet == ALPHA_DIST) {
        if (s >= 30) return (3u << 8) | len;
        return ((unsigned int)kDistBase[s] << 16) | ((unsigned int)kDistBits[s] << 4) | len;
    }
    return (s << 16) | len;
}

// The bit reader: wave-uniform, 128 bits of the stream in scalar registers.  The stream itself is held 64 words at a time in a
// vector register (lane l = word l of the chunk, one coalesced load) with the next chunk already on its way: appending a word
// is a v_readlane, not a trip to memory.
typedef unsigned __int128 u128;
struct Bits {
    const unsigned int* words;       // 4-byte aligned start at or before the stream
    long long wi, wend;              // next word, one past the last word that may be read
    u128 buf;
    int cnt;
    unsigned int cur, nxt;           // words [wi & ~63, +64) and the 64 after them, one per lane
    __device__ unsigned int load_chunk(long long base) const {
        const long long i = base + threadIdx.x;
        return i < wend ? words[i] : 0u;
    }
    __device__ void start(unsigned int skew) {
        cur = load_chunk(0);
        nxt = load_chunk(64);
        buf = (u128)((unsigned int)__builtin_amdgcn_readlane((int)cur, 0) >> (8 * skew));
        cnt = 32 - 8 * (int)skew;
        wi = 1;
    }
    __device__ void append() {
        const unsigned int w = (unsigned int)__builtin_amdgcn_readlane((int)cur, (int)(wi & 63));
        buf |= (u128)w << cnt;
        cnt += 32;
        ++wi;
        if ((wi & 63) == 0) {
            cur = nxt;
            nxt = load_chunk(wi + 64);
        }
    }
    __device__ void refill() {       // more than 96 bits afterwards (zeros past the end, see starved())
        while (cnt <= 96) append();
    }
    __device__ unsigned int get(int n) {
        const unsigned int v = (unsigned int)buf & (unsigned int)((1ull << n) - 1ull);
        buf >>= n;
        cnt -= n;
        return v;
    }
    __device__ void skip(int n) {    // n < 128
        buf >>= n;
        cnt -= n;
    }
    __device__ unsigned int peek(int at, int n) const { return (unsigned int)(buf >> at) & (unsigned int)((1ull << n) - 1ull); }
    // words past `wend` read as zeros (load_chunk); having consumed any of them is an error, found when a block ends
    __device__ bool starved() const { return 32 * wi - cnt > 32 * wend; }
};

// puff.c construct(): counts per length, symbols in code order; returns the code space left (< 0 over-subscribed, 0 complete)
__device__ inline int construct(const unsigned char* lens, int n, unsigned short* cnt, unsigned short* sym, unsigned short* offs) {
    for (int l = 0; l < 16; ++l) cnt[l] = 0;
    for (int s = 0; s < n; ++s) cnt[uni(lens[s])] += 1;
    int left = 1;
    for (int l = 1; l < 16; ++l) {
        left <<= 1;
        left -= (int)uni(cnt[l]);
        if (left < 0) return left;
    }
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (unsigned short)(uni(offs[l]) + uni(cnt[l]));
    for (int s = 0; s < n; ++s) {
        const unsigned int l = uni(lens[s]);
        if (l) {
            const unsigned int o = uni(offs[l]);
            sym[o] = (unsigned short)s;
            offs[l] = (unsigned short)(o + 1);
        }
    }
    return left;
}

// the one-read table for codes of up to `bits` bits: fast[reversed code | k << len] = entry_of(symbol, len)
__device__ inline void fill_fast(const unsigned short* cnt, const unsigned short* sym, unsigned int* fast, int bits, int alphabet) {
    const int lane = threadIdx.x;
    for (int i = lane; i < (1 << bits); i += 64) fast[i] = 0;
    unsigned int code = 0, index = 0;
    for (int l = 1; l <= bits; ++l) {
        const unsigned int c = uni(cnt[l]);
        for (unsigned int j = 0; j < c; ++j) {
            const unsigned int s = uni(sym[index + j]);
            const unsigned int rev = __brev(code + j) >> (32 - l);
            const unsigned int e = entry_of(alphabet, s, (unsigned int)l);
            for (int k = lane; k < (1 << (bits - l)); k += 64) fast[rev | ((unsigned int)k << l)] = e;
        }
        index += c;
        code = (code + c) << 1;
    }
}

// a code longer than the fast table: the canonical walk over the lengths (puff.c decode()); 0 = no such code
__device__ inline unsigned int decode_slow(const Bits& B, int at, const unsigned short* cnt, const unsigned short* sym, int alphabet) {
    unsigned long long b = (unsigned long long)(B.buf >> at);
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= 15; ++l) {
        code |= (int)(b & 1ull);
        b >>= 1;
        const int c = (int)uni(cnt[l]);
        if (code - c < first) return entry_of(alphabet, uni(sym[index + (code - first)]), (unsigned int)l);
        index += c;
        first += c;
        first <<= 1;
        code <<= 1;
    }
    return 0;
}

typedef unsigned int u4_any __attribute__((ext_vector_type(4), aligned(1)));
typedef unsigned int u4_lds __attribute__((ext_vector_type(4), aligned(16)));

// window bytes [from, from + FLUSH) -> the text; `from` is a multiple of FLUSH, the destination is wherever the member begins
__device__ inline void flush_window(const Lds& L, unsigned char* dst, unsigned int from) {
    for (int k = threadIdx.x * 16; k < FLUSH; k += 64 * 16)
        *reinterpret_cast<u4_any*>(dst + from + k) = *reinterpret_cast<const u4_lds*>(&L.win[(from + k) & (WIN - 1)]);
}

__global__ __launch_bounds__(64) void gz_inflate(const unsigned char* __restrict__ gz, const Job* __restrict__ jobs, unsigned char* __restrict__ text,
                                                 int* __restrict__ status, unsigned int* __restrict__ any_error) {
    __shared__ Lds L;
    const int lane = threadIdx.x;
    const Job J = jobs[blockIdx.x];
    unsigned char* dst = text + J.dst;
    const unsigned int out_len = J.dst_len;
    Bits B;
    B.words = reinterpret_cast<const unsigned int*>(gz + (J.src & ~3ull));
    const unsigned int skew = (unsigned int)(J.src & 3ull);
    B.wend = ((long long)skew + J.src_len + 8 + 3) / 4;                    // the 8 trailer bytes may be looked at, never past them
    B.start(skew);
    unsigned int pos = 0, flushed = 0;
    int err = E_NONE;
    bool last = false;
    while (!last && err == E_NONE) {
        B.refill();
        last = B.get(1) != 0;
        const unsigned int type = B.get(2);
        if (type == 0) {                                                   // stored
            B.get(B.cnt & 7);
            B.refill();
            const unsigned int len = B.get(16);
            B.refill();
            const unsigned int nlen = B.get(16);
            if ((len ^ 0xffffu) != nlen) {
                err = E_STORED;
                break;
            }
            if (len > out_len - pos) {
                err = E_OUTPUT;
                break;
            }
            for (unsigned int i = 0; i < len; ++i) {
                B.refill();
                const unsigned int b = B.get(8);
                if (lane == 0) L.win[pos & (WIN - 1)] = (unsigned char)b;
                ++pos;
                if (pos - flushed >= FLUSH) {
                    flush_window(L, dst, flushed);
                    flushed += FLUSH;
                }
            }
            if (B.starved()) err = E_INPUT;
            continue;
        }
        if (type == 3) {
            err = E_BLOCK_TYPE;
            break;
        }
        int n_lit, n_dist;
        if (type == 1) {                                                   // fixed codes
            for (int s = lane; s < 288; s += 64) L.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
            for (int s = lane; s < 32; s += 64) L.lens[288 + s] = 5;
            n_lit = 288;
            n_dist = 32;                                                   // 30 and 31 fill the code space and are never valid
        } else {                                                           // dynamic: the code length code first
            B.refill();
            n_lit = (int)B.get(5) + 257;
            n_dist = (int)B.get(5) + 1;
            const int n_cl = (int)B.get(4) + 4;
            if (n_lit > 286 || n_dist > 30) {
                err = E_TABLE;
                break;
            }
            for (int s = lane; s < 19; s += 64) L.lens[s] = 0;
            for (int k = 0; k < n_cl; ++k) {
                B.refill();
                const unsigned int v = B.get(3);
                if (lane == 0) L.lens[kClOrder[k]] = (unsigned char)v;
            }
            if (construct(L.lens, 19, L.lit_cnt, L.lit_sym, L.offs) != 0) {  // the code length code must be complete
                err = E_TABLE;
                break;
            }
            fill_fast(L.lit_cnt, L.lit_sym, L.lit_fast, 7, ALPHA_RAW);
            int at = 0;
            unsigned int prev = 0;
            const int total = n_lit + n_dist;
            // the lengths go into lens[] from its start: the code length code's own 19 lengths are no longer needed
            while (at < total && err == E_NONE) {
                B.refill();
                unsigned int e = uni(L.lit_fast[(unsigned int)B.buf & 127u]);            // codes of at most 7 bits: always in the table
                if ((e & 15u) == 0) {
                    err = E_TABLE;
                    break;
                }
                B.get((int)(e & 15u));
                const int s = (int)(e >> 16);
                if (s < 16) {
                    if (lane == 0) L.lens[at] = (unsigned char)s;
                    prev = (unsigned int)s;
                    ++at;
                } else {
                    unsigned int v = 0, rep;
                    if (s == 16) {
                        if (at == 0) {
                            err = E_TABLE;
                            break;
                        }
                        v = prev;
                        rep = 3 + B.get(2);
                    } else if (s == 17) {
                        rep = 3 + B.get(3);
                    } else {
                        rep = 11 + B.get(7);
                    }
                    if (at + (int)rep > total) {
                        err = E_TABLE;
                        break;
                    }
                    for (int k = lane; k < (int)rep; k += 64) L.lens[at + k] = (unsigned char)v;
                    at += (int)rep;
                    prev = v;
                }
            }
            if (err != E_NONE) break;
            if (uni(L.lens[256]) == 0) {                                   // no end-of-block code
                err = E_TABLE;
                break;
            }
            // the distance lengths follow the literal/length ones: to their own place (one instruction: every lane reads its
            // byte before any lane writes), then the literal/length tail is cleared
            {
                const unsigned char v = lane < n_dist ? L.lens[n_lit + lane] : (unsigned char)0;
                if (lane < 32) L.lens[288 + lane] = v;
            }
            for (int s = n_lit + lane; s < 288; s += 64) L.lens[s] = 0;
        }
        {
            // zlib's (and puff.c's) rule: an incomplete code is accepted only when it is a single code of length 1 - or, for the
            // distances, no code at all (RFC 1951 3.2.7: a block of literals only; zlib's inflate_table `max == 0`).  The
            // literal/length set always holds end-of-block.  With no distance code dist_fast is all zeros and decode_slow finds
            // nothing, so a length symbol in such a block ends in E_SYMBOL.
            const int left_l = construct(L.lens, 288, L.lit_cnt, L.lit_sym, L.offs);
            if (left_l < 0 || (left_l > 0 && !(288 - (int)uni(L.lit_cnt[0]) == 1 && uni(L.lit_cnt[1]) == 1))) {
                err = E_TABLE;
                break;
            }
            const int left_d = construct(L.lens + 288, 32, L.dist_cnt, L.dist_sym, L.offs);
            const int used_d = 32 - (int)uni(L.dist_cnt[0]);
            if (left_d < 0 || (left_d > 0 && !(used_d == 0 || (used_d == 1 && uni(L.dist_cnt[1]) == 1)))) {
                err = E_TABLE;
                break;
            }
            fill_fast(L.lit_cnt, L.lit_sym, L.lit_fast, FAST_L, ALPHA_LIT);
            fill_fast(L.dist_cnt, L.dist_sym, L.dist_fast, FAST_D, ALPHA_DIST);
        }
        // The symbols of the block.  Lane k decodes the WHOLE symbol that would begin k bits ahead - literal/length entry, extra
        // bits, distance entry, extra bits: two dependent LDS reads for 64 candidate positions at once - and the wave then
        // walks from symbol to symbol with v_readlane (the bit position after a symbol picks the lane that holds the next one)
        // instead of two dependent trips to LDS and some forty scalar instructions per symbol.  A symbol spans at most
        // 15 + 5 + 15 + 13 = 48 bits, which the 64-bit view of a lane covers; the walk goes on while that many valid bits lie
        // beyond a symbol's start.  Codes longer than the one-read tables send that symbol down the scalar path.
        bool end_of_block = false;
        while (!end_of_block && err == E_NONE) {
            B.refill();
            const unsigned long long lo = (unsigned long long)B.buf, hi = (unsigned long long)(B.buf >> 64);
            const unsigned long long v0 = lane ? (lo >> lane) | (hi << (64 - lane)) : lo;
            const unsigned int le = L.lit_fast[(unsigned int)v0 & ((1u << FAST_L) - 1u)];
            const unsigned int cl = le & 15u, xl = (le >> 4) & 15u, kind = (le >> 8) & 3u;
            const unsigned long long v1 = v0 >> cl;
            const unsigned int len_x = (unsigned int)v1 & ((1u << xl) - 1u);
            const unsigned long long v2 = v1 >> xl;
            const unsigned int de = L.dist_fast[(unsigned int)v2 & ((1u << FAST_D) - 1u)];
            const unsigned int cd = de & 15u, xd = (de >> 4) & 15u;
            const unsigned int dist_x = (unsigned int)(v2 >> cd) & ((1u << xd) - 1u);
            const bool whole = cl != 0 && (kind != 1 || (cd != 0 && ((de >> 8) & 3u) == 0));
            // what the walk reads: bits 0-5 the symbol's span, 6-7 its kind, 8 decoded here, 16-31 the byte or the length
            const unsigned int head = (kind == 1 ? cl + xl + cd + xd : cl) | (kind << 6) | (whole ? 256u : 0u) | (((le >> 16) + (kind == 1 ? len_x : 0u)) << 16);
            const unsigned int far = (de >> 16) + dist_x;
            int p = 0;
            while (p < 64 && p + 48 <= B.cnt) {
                unsigned int h = (unsigned int)__builtin_amdgcn_readlane((int)head, p);
                unsigned int dist = (unsigned int)__builtin_amdgcn_readlane((int)far, p);
                if ((h & 256u) == 0) {                                     // a long code somewhere in this symbol: the scalar path
                    unsigned int e = uni(L.lit_fast[B.peek(p, FAST_L)]);
                    if ((e & 15u) == 0) e = decode_slow(B, p, L.lit_cnt, L.lit_sym, ALPHA_LIT);
                    if (e == 0) {
                        err = E_SYMBOL;
                        break;
                    }
                    int q = p + (int)(e & 15u);
                    const unsigned int k = (e >> 8) & 3u;
                    unsigned int value = e >> 16;
                    if (k == 1) {
                        const int x = (int)((e >> 4) & 15u);
                        value += B.peek(q, x);
                        q += x;
                        unsigned int d = uni(L.dist_fast[B.peek(q, FAST_D)]);
                        if ((d & 15u) == 0) d = decode_slow(B, q, L.dist_cnt, L.dist_sym, ALPHA_DIST);
                        if (d == 0 || ((d >> 8) & 3u)) {
                            err = E_SYMBOL;
                            break;
                        }
                        q += (int)(d & 15u);
                        const int y = (int)((d >> 4) & 15u);
                        dist = (d >> 16) + B.peek(q, y);
                        q += y;
                    }
                    h = (unsigned int)(q - p) | (k << 6) | (value << 16);
                }
                p += (int)(h & 63u);
                const unsigned int k = (h >> 6) & 3u;
                if (k == 0) {                                              // a literal
                    if (pos >= out_len) {
                        err = E_OUTPUT;
                        break;
                    }
                    if (lane == 0) L.win[pos & (WIN - 1)] = (unsigned char)(h >> 16);
                    ++pos;
                } else if (k == 1) {                                       // a match
                    const unsigned int len = h >> 16;
                    if (dist > pos) {
                        err = E_DISTANCE;
                        break;
                    }
                    if (len > out_len - pos) {
                        err = E_OUTPUT;
                        break;
                    }
                    // bytes pos .. pos + len - 1 = the `dist` bytes before pos, repeated: all reads come before all writes
                    const unsigned int from = pos - dist;
                    if (len <= 64 && dist >= len) {
                        unsigned char b = 0;
                        if ((unsigned int)lane < len) b = L.win[(from + lane) & (WIN - 1)];
                        if ((unsigned int)lane < len) L.win[(pos + lane) & (WIN - 1)] = b;
                    } else {
                        unsigned char b[5];
#pragma unroll
                        for (int i5 = 0; i5 < 5; ++i5) {
                            const unsigned int i = (unsigned int)lane + 64u * i5;
                            if (i < len) b[i5] = L.win[(from + (dist >= len ? i : i % dist)) & (WIN - 1)];
                        }
#pragma unroll
                        for (int i5 = 0; i5 < 5; ++i5) {
                            const unsigned int i = (unsigned int)lane + 64u * i5;
                            if (i < len) L.win[(pos + i) & (WIN - 1)] = b[i5];
                        }
                    }
                    pos += len;
                } else if (k == 2) {                                       // end of block
                    end_of_block = true;
                    break;
                } else {
                    err = E_SYMBOL;
                    break;
                }
                if (pos - flushed >= FLUSH) {
                    flush_window(L, dst, flushed);
                    flushed += FLUSH;
                }
            }
            B.skip(p);                                                     // the bits walked over leave the buffer (at most 63 + 48)
        }
        if (err == E_NONE && B.starved()) err = E_INPUT;
    }
    if (err == E_NONE) {
        for (unsigned int k = flushed + lane; k < pos; k += 64) dst[k] = L.win[k & (WIN - 1)];
        const long long consumed = 32 * B.wi - 8 * (long long)skew - B.cnt;
        if (pos != out_len) err = E_SIZE;
        else if (B.starved() || consumed > 8ll * J.src_len) err = E_INPUT;
    }
    if (lane == 0) {
        status[blockIdx.x] = err;
        if (err != E_NONE) atomicOr(any_error, 1u);
    }
}

// CRC-32 of each member's text against its trailer
__global__ __launch_bounds__(256) void gz_crc(const unsigned char* __restrict__ text, const Job* __restrict__ jobs, const unsigned int* __restrict__ crc_table,
                                              const unsigned int* __restrict__ x2n_table, int* __restrict__ status, unsigned int* __restrict__ any_error) {
    __shared__ unsigned int tab[4][256];                               // slicing-by-4: tab[k][b] = CRC of byte b followed by k zero bytes
    __shared__ unsigned int wxor[4];
    for (int k = 0; k < 4; ++k) tab[k][threadIdx.x] = crc_table[k * 256 + threadIdx.x];
    __syncthreads();
    const Job J = jobs[blockIdx.x];
    const unsigned char* p = text + J.dst;
    const unsigned long long n = J.dst_len;
    const unsigned long long span = ((n + 255) / 256 + 15) & ~15ull;
    const unsigned long long b = span * threadIdx.x, e = b + span < n ? b + span : n;
    unsigned int part = 0;
    if (b < n) {
        unsigned int c = 0xffffffffu;
        unsigned long long i = b;
        for (; i < e && ((uintptr_t)(p + i) & 3u); ++i) c = tab[0][(c ^ p[i]) & 0xffu] ^ (c >> 8);
        for (; i + 4 <= e; i += 4) {                                    // four table reads that do not wait for each other
            c ^= *reinterpret_cast<const unsigned int*>(p + i);
            c = tab[3][c & 0xffu] ^ tab[2][(c >> 8) & 0xffu] ^ tab[1][(c >> 16) & 0xffu] ^ tab[0][c >> 24];
        }
        for (; i < e; ++i) c = tab[0][(c ^ p[i]) & 0xffu] ^ (c >> 8);
        c ^= 0xffffffffu;
        unsigned long long after = n - e;                                 // advance by the bytes that follow: x^(8 after) mod p
        unsigned int op = 1u << 31, k = 3;
        while (after) {
            if (after & 1ull) op = fhx::emit::crc_multmodp(x2n_table[k & 31u], op);
            after >>= 1;
            ++k;
        }
        part = fhx::emit::crc_multmodp(op, c);
    }
    for (int s = 32; s >= 1; s >>= 1) part ^= __shfl_xor(part, s, 64);
    if ((threadIdx.x & 63) == 0) wxor[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int crc = wxor[0] ^ wxor[1] ^ wxor[2] ^ wxor[3];
        if (status[blockIdx.x] == E_NONE && crc != J.crc) {
            status[blockIdx.x] = E_CRC;
            atomicOr(any_error, 1u);
        }
    }
}

}  // namespace gzdev
}  // namespace fhx

namespace {

// the CRC-32 byte table and x^(2^k) mod p, as the writer builds them
void crc_tables(unsigned int* tab /* 4 x 256: slicing-by-4 */, unsigned int* x2n) {
    for (unsigned int i = 0; i < 256; ++i) {
        unsigned int c = i;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
        tab[i] = c;
    }
    for (int k = 1; k < 4; ++k)
        for (unsigned int i = 0; i < 256; ++i) tab[k * 256 + i] = (tab[(k - 1) * 256 + i] >> 8) ^ tab[tab[(k - 1) * 256 + i] & 0xffu];
    unsigned int p = 1u << 30;
    x2n[0] = p;
    for (int k = 1; k < 32; ++k) x2n[k] = p = fhx::emit::crc_multmodp(p, p);
}

// host bytes -> device, through two pinned 64 MB buffers filled by the host threads (pageable memory is not DMA-able)
int upload_spans(fhx_ctx* ctx, const std::vector<std::pair<const char*, size_t>>& spans, unsigned char* d_dst, int n_threads) {
    hipError_t pin_err;
    EmitPinned* pinned_ptr = pinned_pair(ctx, &pin_err);
    FHX_HIP(pin_err);
    EmitPinned& pinned = *pinned_ptr;
    const size_t chunk = EmitPinned::kChunk;
    std::vector<int64_t> span_off(spans.size() + 1, 0);
    for (size_t k = 0; k < spans.size(); ++k) span_off[k + 1] = span_off[k] + (int64_t)spans[k].second;
    const int64_t T = span_off.back();
    size_t piece = 0;
    int turn = 0;
    bool used[2] = {false, false};
    for (int64_t off = 0; off < T; off += (int64_t)chunk, turn ^= 1) {
        const int64_t len = std::min<int64_t>((int64_t)chunk, T - off);
        if (used[turn]) FHX_HIP(hipEventSynchronize(pinned.ev[turn]));
        struct Slice {
            const char* src;
            char* dst;
            size_t n;
        };
        std::vector<Slice> slices;
        for (int64_t o = off; o < off + len;) {
            while (span_off[piece + 1] <= o) ++piece;
            const int64_t n = std::min<int64_t>({off + len - o, span_off[piece + 1] - o, (int64_t)4 << 20});
            slices.push_back(Slice{spans[piece].first + (o - span_off[piece]), (char*)pinned.p[turn] + (o - off), (size_t)n});
            o += n;
        }
        std::atomic<size_t> next{0};
        auto work = [&]() {
            for (;;) {
                const size_t i = next.fetch_add(1);
                if (i >= slices.size()) return;
                std::memcpy(slices[i].dst, slices[i].src, slices[i].n);
            }
        };
        const int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_threads, slices.size()));
        std::vector<std::thread> pool;
        for (int k = 1; k < nt; ++k) pool.emplace_back(work);
        work();
        for (auto& th : pool) th.join();
        FHX_HIP(hipMemcpyAsync(d_dst + off, pinned.p[turn], (size_t)len, hipMemcpyHostToDevice, ctx->stream));
        FHX_HIP(hipEventRecord(pinned.ev[turn], ctx->stream));
        used[turn] = true;
    }
    FHX_HIP(hipStreamSynchronize(ctx->stream));                          // the pinned buffers are free for the next user
    return FHX_OK;
}

// offset of the deflate stream inside a gzip member (RFC 1952 header), 0 = not a header this path reads
size_t gz_payload_offset(const unsigned char* m, size_t size) {
    if (size < 18 || m[0] != 0x1f || m[1] != 0x8b || m[2] != 8 || (m[3] & 0xe0)) return 0;
    const unsigned int flg = m[3];
    size_t o = 10;
    if (flg & 4) {
        if (o + 2 > size) return 0;
        o += 2 + (m[o] | ((size_t)m[o + 1] << 8));
    }
    for (int name = 0; name < 2; ++name)
        if (flg & (name == 0 ? 8u : 16u)) {
            while (o < size && m[o]) ++o;
            ++o;
        }
    if (flg & 2) o += 2;
    return o + 8 <= size ? o : 0;
}

// A file of size-tagged gzip members -> its text in HBM (*d_text, allocated in tmp, padded for the parser kernels).
// FHX_ERR_UNSUPPORTED + why: not such a file, or a stream the device decoder refuses - the host's zlib is the judge then.
int device_inflate(fhx_ctx* ctx, DeviceScratch& tmp, const fhx::FileBytes& gz, int n_threads, size_t pad_to, unsigned char** d_text, int64_t* T,
                   int64_t* n_members, std::string& why) {
    using namespace fhx::gzdev;
    std::vector<fhx::GzMember> members;
    if (!fhx::io_scan_members(gz.data(), gz.size(), members)) {
        why = "not a file of size-tagged gzip members (one plain gzip stream is inflated by the host cores, fhx_gunzip.cpp)";
        return FHX_ERR_UNSUPPORTED;
    }
    std::vector<Job> jobs(members.size());
    unsigned long long total = 0;
    for (size_t i = 0; i < members.size(); ++i) {
        const unsigned char* m = gz.data() + members[i].off;
        const size_t o = gz_payload_offset(m, members[i].size);
        if (o == 0 || members[i].isize > ((size_t)64 << 20)) {
            why = o == 0 ? "a gzip member header this path does not read" : "a gzip member of more than 64 MB of text (one wave per member would crawl)";
            return FHX_ERR_UNSUPPORTED;
        }
        const unsigned char* tail = m + members[i].size - 8;
        jobs[i].src = members[i].off + o;
        jobs[i].src_len = (unsigned int)(members[i].size - o - 8);
        jobs[i].dst = total;
        jobs[i].dst_len = (unsigned int)members[i].isize;
        jobs[i].crc = tail[0] | ((unsigned int)tail[1] << 8) | ((unsigned int)tail[2] << 16) | ((unsigned int)tail[3] << 24);
        jobs[i].pad = 0;
        total += members[i].isize;
    }
    const size_t text_bytes = ((size_t)total + pad_to - 1) / pad_to * pad_to + 64;
    unsigned char* d_gz = nullptr;
    Job* d_jobs = nullptr;
    int* d_status = nullptr;
    unsigned int *d_err = nullptr, *d_tab = nullptr, *d_x2n = nullptr;
    DeviceScratch own;                                                     // the compressed bytes are dropped on return
    FHX_HIP(own.get(&d_gz, gz.size() + 64));
    FHX_HIP(own.get(&d_jobs, jobs.size() * sizeof(Job)));
    FHX_HIP(own.get(&d_status, jobs.size() * sizeof(int)));
    FHX_HIP(own.get(&d_err, sizeof(unsigned int)));
    FHX_HIP(own.get(&d_tab, 4 * 256 * 4));
    FHX_HIP(own.get(&d_x2n, 32 * 4));
    FHX_HIP(tmp.get(d_text, text_bytes));
    {
        const int rc = upload_spans(ctx, {{(const char*)gz.data(), gz.size()}}, d_gz, n_threads);
        if (rc != FHX_OK) return rc;
    }
    unsigned int tab[4 * 256], x2n[32];
    crc_tables(tab, x2n);
    FHX_HIP(hipMemsetAsync(d_gz + gz.size(), 0, 64, ctx->stream));
    FHX_HIP(hipMemcpyAsync(d_jobs, jobs.data(), jobs.size() * sizeof(Job), hipMemcpyHostToDevice, ctx->stream));
    FHX_HIP(hipMemcpyAsync(d_tab, tab, sizeof(tab), hipMemcpyHostToDevice, ctx->stream));
    FHX_HIP(hipMemcpyAsync(d_x2n, x2n, sizeof(x2n), hipMemcpyHostToDevice, ctx->stream));
    FHX_HIP(hipMemsetAsync(d_err, 0, sizeof(unsigned int), ctx->stream));
    FHX_HIP(hipMemsetAsync(*d_text + total, ' ', text_bytes - (size_t)total, ctx->stream));
    const bool timing = std::getenv("FHX_TIMING") != nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    if (timing)
        for (auto& e : ev) FHX_HIP(hipEventCreate(&e));
    if (timing) FHX_HIP(hipEventRecord(ev[0], ctx->stream));
    hipLaunchKernelGGL(gz_inflate, dim3((unsigned)jobs.size()), dim3(64), 0, ctx->stream, (const unsigned char*)d_gz, (const Job*)d_jobs, *d_text, d_status,
                       d_err);
    if (timing) FHX_HIP(hipEventRecord(ev[1], ctx->stream));
    hipLaunchKernelGGL(gz_crc, dim3((unsigned)jobs.size()), dim3(256), 0, ctx->stream, (const unsigned char*)*d_text, (const Job*)d_jobs,
                       (const unsigned int*)d_tab, (const unsigned int*)d_x2n, d_status, d_err);
    if (timing) FHX_HIP(hipEventRecord(ev[2], ctx->stream));
    unsigned int any = 0;
    FHX_HIP(hipMemcpyAsync(&any, d_err, sizeof(any), hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipStreamSynchronize(ctx->stream));
    if (timing) {
        float ms_inflate = 0, ms_crc = 0;
        (void)hipEventElapsedTime(&ms_inflate, ev[0], ev[1]);
        (void)hipEventElapsedTime(&ms_crc, ev[1], ev[2]);
        std::fprintf(stderr, "device_inflate: %zu members, %.1f MB -> %.1f MB: gz_inflate %.2f ms, gz_crc %.2f ms\n", jobs.size(), gz.size() / 1e6,
                     (double)total / 1e6, ms_inflate, ms_crc);
        for (auto& e : ev) (void)hipEventDestroy(e);
    }
    if (any) {
        std::vector<int> status(jobs.size());
        FHX_HIP(hipMemcpy(status.data(), d_status, status.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < status.size(); ++i)
            if (status[i]) {
                static const char* const what[] = {"", "reserved block type", "stored block length", "Huffman table", "symbol", "distance beyond the start",
                                                   "more text than ISIZE", "stream ends early", "ISIZE", "CRC-32"};
                why = "gzip member " + std::to_string(i) + ": " + what[status[i] < 10 ? status[i] : 0] + " (device decoder)";
                break;
            }
        return FHX_ERR_UNSUPPORTED;
    }
    *T = (int64_t)total;
    *n_members = (int64_t)jobs.size();
    return FHX_OK;
}

}  // namespace
