// fhx_textlines.hpp - the newline layer of every device text path: fhx_ingest.inc (contact counts), fhx_hicpro.hip (HiC-Pro
// matrix), fhx_validpairs.hip and fhx_fragpairs.hip (allValidPairs; their line walk is fhx_pairline.hpp), fhx_digest.hip (FASTA),
// fhx_juicer.hip (Juicer dump) and fhx_sigselect.hip with fhx_sigtrack.inc and fhx_sigsplit.inc (significances).  A text lies in HBM, padded with blanks to whole blocks plus 64 bytes (fhx_textupload.hpp
// upload_batch); a workgroup of WG lanes owns BLOCK_BYTES of it, SEG bytes per lane read as 16-byte loads.
//
//   scan_text<Bytes>   newlines per block, and bit REFUSED_BYTES in a flag word when a byte the path's policy refuses is seen
//   scan_tiles         exclusive scan of the block counts = the line number of every block's first line          (fhx_scan.hpp)
//   block_lines        called by the path's own per-line kernels: where the lines that begin in its block start, and the line
//                      number of the first of them
//
// A refused line is reported as ONE 64-bit word, error_word(line, reason), kept with atomicMin: the smallest offending line
// whatever the launch order.  The grammars (what a line may hold) stay with the paths.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fhx_scan.hpp"

namespace fhxlines {

constexpr int WG = 256;
constexpr int BLOCK_BYTES = 16384;             // text per workgroup
constexpr int SEG = BLOCK_BYTES / WG;          // 64 bytes per lane in the newline passes
constexpr int MAX_LINE = 4096;                 // a longer line is not a regular one
constexpr int LSTART_ENTRIES = BLOCK_BYTES + 2; // of block_lines' LDS array: block 0 needs BLOCK_BYTES + 1 (the implicit first line +
                                               // one per newline byte), rounded up to an even count
constexpr unsigned long long NO_ERROR = ~0ull;
constexpr unsigned int REFUSED_BYTES = 1u;     // the bit scan_text raises

// (1-based line << 8) | reason: the smaller line wins an atomicMin, and NO_ERROR loses to every line
__host__ __device__ inline unsigned long long error_word(int64_t line, int why) { return ((unsigned long long)line << 8) | (unsigned long long)why; }
inline int32_t error_why(unsigned long long word) { return (int32_t)(word & 0xFFu); }
inline int64_t error_line(unsigned long long word) { return (int64_t)(word >> 8); }

// ---- byte policies of scan_text: check() sets `bad` when byte c at text[p] is one the path does not take --------------------
struct AnyByte {
    static __device__ void check(bool&, unsigned int, const unsigned char*, int64_t, int64_t) {}
};
// what Python's text mode would not hand over unchanged: NUL, non-ASCII, a \r that is not followed by \n (it would end the line)
struct TextModeBytes {
    static __device__ void check(bool& bad, unsigned int c, const unsigned char* text, int64_t p, int64_t T) {
        bad |= c == 0 || c >= 0x80;
        if (c == '\r') bad |= p + 1 >= T || text[p + 1] != '\n';
    }
};

// ---- pass 1 over a text: newlines per block, refused bytes anywhere (at most one flag write per lane) ----------------------
template <typename Bytes>
__global__ __launch_bounds__(WG) void scan_text(const unsigned char* __restrict__ text, int64_t T, unsigned int* __restrict__ block_nl,
                                                unsigned int* __restrict__ flags) {
    const int64_t p0 = (int64_t)blockIdx.x * BLOCK_BYTES + (int64_t)threadIdx.x * SEG;
    unsigned int nl = 0;
    bool bad = false;
    if (p0 < T) {
        const uint4* src = reinterpret_cast<const uint4*>(text + p0);        // the allocation is padded to whole blocks
        for (int v = 0; v < SEG / 16; ++v) {
            const uint4 w = src[v];
            const unsigned int word[4] = {w.x, w.y, w.z, w.w};
            for (int k = 0; k < 16; ++k) {
                const unsigned int c = (word[k >> 2] >> (8 * (k & 3))) & 0xFFu;
                const int64_t p = p0 + v * 16 + k;
                const bool inside = p < T;                                    // no early exit: the 64 bytes are handled as straight-line code
                nl += (c == '\n' && inside) ? 1u : 0u;
                if (inside) Bytes::check(bad, c, text, p, T);
            }
        }
    }
    unsigned int total;
    fhxscan::block_exclusive_scan(nl, &total);
    if (threadIdx.x == 0) block_nl[blockIdx.x] = total;
    if (bad) atomicOr(flags, REFUSED_BYTES);
}

// The lines that BEGIN after a newline of this block (and line 0 in block 0): their start offsets relative to the block, in
// order, in LDS (lstart has LSTART_ENTRIES entries) -> their number.
__device__ inline int block_lines(const unsigned char* __restrict__ text, int64_t T, unsigned short* lstart) {
    const int64_t p0 = (int64_t)blockIdx.x * BLOCK_BYTES + (int64_t)threadIdx.x * SEG;
    unsigned long long mask = 0;                                              // bit k: byte k of the segment is a newline
    if (p0 < T) {
        const uint4* src = reinterpret_cast<const uint4*>(text + p0);
        for (int v = 0; v < SEG / 16; ++v) {
            const uint4 w = src[v];
            const unsigned int word[4] = {w.x, w.y, w.z, w.w};
            for (int k = 0; k < 16; ++k) {
                const unsigned int c = (word[k >> 2] >> (8 * (k & 3))) & 0xFFu;
                if (c == '\n' && p0 + v * 16 + k + 1 < T) mask |= 1ull << (v * 16 + k);        // a newline that ends the text starts no line
            }
        }
    }
    const unsigned int first = (blockIdx.x == 0 && T > 0) ? 1u : 0u;
    unsigned int total;
    unsigned int rank = fhxscan::block_exclusive_scan((unsigned int)__popcll(mask), &total) + first;
    if (first && threadIdx.x == 0) lstart[0] = 0;
    while (mask) {
        const int k = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        lstart[rank++] = (unsigned short)(threadIdx.x * SEG + k + 1);         // 16384 for a line that starts the next block
    }
    __syncthreads();
    return (int)(total + first);
}

// What a per-line kernel knows of its block: entry e < n_lines begins at text[b0 + lstart[e]] and is line row0 + e of the text
// (block_off is scan_tiles' exclusive scan of the blocks' newlines: e in block 0, block_off[block] + 1 + e elsewhere).
struct BlockLines {
    int n_lines;
    int64_t b0, row0;
};
__device__ inline BlockLines block_lines(const unsigned char* __restrict__ text, int64_t T, const unsigned long long* __restrict__ block_off,
                                         unsigned short* lstart) {
    BlockLines B;
    B.n_lines = block_lines(text, T, lstart);
    B.b0 = (int64_t)blockIdx.x * BLOCK_BYTES;
    B.row0 = blockIdx.x == 0 ? 0 : (int64_t)block_off[blockIdx.x] + 1;
    return B;
}

}  // namespace fhxlines
