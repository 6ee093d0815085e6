// fhx_validpairs.hip - HiC-Pro's allValidPairs (one line per read pair) binned into Fit-Hi-C's contact counts on MI355X (gfx950)
// (reference: fithic/utils/validPairs2FitHiC-fixedSize.sh:33-40, the pipeline of five awk, grep, sort, uniq -c and sed).
//
// The text goes through HBM in BATCHES cut at the last newline (two pinned buffers filled by pread, drained by the copy engine:
// fhx_textupload.hpp), so a 100 GB file never has to be resident: only 16 bytes per kept pair accumulate.  Per batch:
//
//   scan_text, scan_tiles    the newline layer (fhx_textlines.hpp), no byte refused there: the line number of every block's
//                  first line
//   vp_parse       the lines that begin in a block, one per lane.  One walk along the line (fhx_pairline.hpp's, in place) splits it on
//                  blanks, keeps where tokens 2, 3, 5, 6 lie and looks for `chrM` anywhere (grep -v chrM, :34); then the name-length filter (:34),
//                  the distance filter (pos1-pos2)^2 > 2*res (:35 - the comparison sits INSIDE the sqrt), the bins
//                  int(pos/res) (:36) and the order of the two ends (:37).  A name of <= 5 bytes is 40 bits, big-endian and
//                  zero-padded: its integer order is its byte order.  The distinct names go into a 2048-slot table in HBM
//                  (one load per name once it is there, a compare-and-swap only for a new one); a kept pair becomes the record
//                  (slot1 << 32 | bin1, slot2 << 32 | bin2), stored compacted (fhx::block_append: a block scan of the
//                  keep flags and ONE atomicAdd per 256 lines; r04_w_atomic_rate: same-address atomics run at 0.09e9/s).
//
// After the last batch the host ranks the names bytewise (sort runs under LC_ALL=C, :38) and
//
//   vp_text_keys   for every bin index k up to the largest seen: the decimal string of k*res as a sortable word
//                  (digits left-aligned, then the length: "100000" < "20000", and "1000" < "10000" because the tab after the
//                  shorter one is smaller than '0'); fhx_sort_u64 + vp_invert give t[k] = the TEXT rank of bin k
//   vp_keys        record -> one 64-bit key  rank1 | t[bin1] | rank2 | t[bin2], bit widths fitted to the data
//   fhx_sort_u64   the stable radix sort; equal keys are the duplicates uniq -c counts
//   fhx::run_heads, vp_cells    run heads (fhx_cells.hpp: count_heads / scan_tiles / head_positions) -> cells (chr1, mid1, chr2,
//                  mid2, count) in the script's text order; a count is the distance between two heads (64-bit), never a walk
//                  along the run
//
// ONLY THE REGULAR FILE IS TAKEN (the header lists the grammar); anything else is REFUSED with the smallest offending line number
// (one 64-bit word, atomicMin over line << 8 | reason: the same answer whatever the launch order) and nothing stays loaded.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fithic_mi355x.h"
#include "fhx_cells.hpp"
#include "fhx_pairline.hpp"

namespace vpd {

using namespace fhxlines;

constexpr int NAME_SLOTS = 2048;               // the device name table (open addressing, at most half full)
constexpr int MAX_NAMES = 1024;

// the words the kernels of one call share
struct Words {
    unsigned long long first_error = NO_ERROR; // smallest (line << 8 | reason)
    unsigned long long n_records = 0;          // kept pairs so far
    unsigned long long max_bin = 0;            // largest bin index among them
    unsigned long long n_names = 0;            // distinct names in the table
    unsigned long long n_cells = 0;            // scan_tiles' total of the heads
    unsigned long long max_count = 0;          // largest cell count
    unsigned long long names_overflow = 0;     // 1: a pair named a name the full table could not take
};

using fhxpair::is_digit;
using fhxpair::position;
__device__ inline bool is_alpha(int c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'); }

// A name of 1..5 bytes at text[b, b + len) -> its 40-bit word, or 0 for a name awk would compare as a number (or might): the
// grammar takes a name that starts with a letter or `_` (but not with inf / nan in any case), and a plain digit string without
// a leading zero.
__device__ inline unsigned long long pack_name(const unsigned char* __restrict__ text, int64_t b, int len) {
    unsigned long long w = 0;
    bool all_digits = true;
    int c[5] = {0, 0, 0, 0, 0};
    for (int k = 0; k < 5; ++k) {
        if (k < len) {
            c[k] = text[b + k];
            all_digits &= is_digit(c[k]);
        }
        w = (w << 8) | (unsigned long long)c[k];
    }
    if (is_digit(c[0])) return (all_digits && (len == 1 || c[0] != '0')) ? w : 0ull;
    if (!is_alpha(c[0]) && c[0] != '_') return 0ull;
    if (len >= 3) {
        const int l0 = c[0] | 0x20, l1 = c[1] | 0x20, l2 = c[2] | 0x20;
        if ((l0 == 'i' && l1 == 'n' && l2 == 'f') || (l0 == 'n' && l1 == 'a' && l2 == 'n')) return 0ull;
    }
    return w;
}

// awk's `a < b` for two names of the grammar (:37): numeric when both are digit strings (no leading zeros: the longer one is the
// larger, equal lengths compare as bytes), bytewise otherwise - the packed words compare as the bytes do.
__device__ inline bool name_less(unsigned long long a, int la, unsigned long long b, int lb) {
    const bool da = is_digit((int)(a >> 32)), db = is_digit((int)(b >> 32));
    if (da && db && la != lb) return la < lb;
    return a < b;
}

// the slot of `name` in the table, inserting it when it is new; -1 when the table holds MAX_NAMES other names already
__device__ inline int intern_name(unsigned long long* __restrict__ table, unsigned long long* __restrict__ n_names, unsigned long long name) {
    unsigned int h = (unsigned int)((name * 0x9E3779B97F4A7C15ull) >> 53);    // 11 bits
    for (int probe = 0; probe < NAME_SLOTS; ++probe, h = (h + 1) & (NAME_SLOTS - 1)) {
        unsigned long long v = __atomic_load_n(table + h, __ATOMIC_RELAXED);
        if (v == name) return (int)h;
        if (v != 0) continue;
        if (__atomic_load_n(n_names, __ATOMIC_RELAXED) >= (unsigned long long)MAX_NAMES) return -1;
        v = atomicCAS(table + h, 0ull, name);
        if (v == 0) {
            atomicAdd(n_names, 1ull);
            return (int)h;
        }
        if (v == name) return (int)h;
    }
    return -1;
}

__global__ __launch_bounds__(WG) void vp_parse(const unsigned char* __restrict__ text, int64_t T, const unsigned long long* __restrict__ block_off,
                                               int64_t n_lines_batch, int64_t line_base, long long res, unsigned long long* __restrict__ names,
                                               ulonglong2* __restrict__ records, unsigned long long capacity, Words* __restrict__ words) {
    __shared__ unsigned short lstart[LSTART_ENTRIES];
    const BlockLines B = block_lines(text, T, block_off, lstart);
    unsigned long long max_bin = 0;
    for (int base = 0; base < B.n_lines; base += WG) {      // n_lines is the same for every lane: the scans below see whole blocks
        const int e = base + threadIdx.x;
        bool keep = false;
        ulonglong2 rec = make_ulonglong2(0ull, 0ull);
        if (e < B.n_lines) {
            const int64_t r = B.row0 + e;
            // fhxpair::walk written out in place, with the `chrM` search (grep -v chrM, :34) in the same pass: called as a function
            // the walk cost this kernel 4 to 5 % of the parse stage (profiles/r14/cells_layer_ab.txt), fp_parse nothing
            const int64_t start = B.b0 + lstart[e];
            int why = 0, m = 0;
            bool in_tok = false, has_chrM = false;
            fhxpair::Line L;
            int64_t p = start;
            for (;; ++p) {
                const int c = p < T ? (int)text[p] : '\n';                    // the end of the text ends the line
                if (c == '\n') break;
                if (p - start >= MAX_LINE) {
                    why = FHX_VP_LONG_LINE;
                    break;
                }
                if (c == '\r' && p + 1 < T && text[p + 1] == '\n') break;     // \r\n
                if (c < 0x20 ? c != '\t' : c >= 0x7f) {                       // NUL, controls (a lone \r among them), DEL, non-ASCII
                    why = FHX_VP_BYTES;
                    break;
                }
                m = c == "chrM"[m] ? m + 1 : (c == 'c' ? 1 : 0);
                if (m == 4) {
                    has_chrM = true;
                    m = 0;
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
            if (!why && L.tok < 6) why = FHX_VP_TOKENS;
            if (!why && r >= n_lines_batch) why = FHX_VP_INTERNAL;           // the scan and this kernel disagree about the lines
            const int l1 = L.len(0), l2 = L.len(2);
            // :34 - a line with a longer name, or with chrM anywhere, is dropped whatever else it holds
            if (!why && l1 <= 5 && l2 <= 5 && !has_chrM) {
                unsigned long long n1 = pack_name(text, L.tb[0], l1), n2 = pack_name(text, L.tb[2], l2);
                long long p1 = 0, p2 = 0;
                if (n1 == 0 || n2 == 0) why = FHX_VP_NAME;
                else if (!position(text, L.tb[1], L.len(1), &p1) || !position(text, L.tb[3], L.len(3), &p2)) why = FHX_VP_POSITION;
                else {
                    long long k1 = p1 / res, k2 = p2 / res;                   // :36
                    if (k1 * res + res / 2 > 2147483647ll || k2 * res + res / 2 > 2147483647ll) why = FHX_VP_RANGE;
                    else {
                        const long long d = p1 - p2;                          // below 2^31: d * d is exact
                        if (n1 != n2 || d * d > 2 * res) {                    // :35
                            const bool as_is = n1 == n2 ? k1 <= k2 : name_less(n1, l1, n2, l2);        // :37
                            if (!as_is) {
                                const unsigned long long tn = n1;
                                n1 = n2;
                                n2 = tn;
                                const long long tk = k1;
                                k1 = k2;
                                k2 = tk;
                            }
                            const int s1 = intern_name(names, &words->n_names, n1);
                            const int s2 = n2 == n1 ? s1 : intern_name(names, &words->n_names, n2);
                            // which line meets the full table depends on the launch order: no line is reported for it
                            if (s1 < 0 || s2 < 0) __atomic_store_n(&words->names_overflow, 1ull, __ATOMIC_RELAXED);
                            else {
                                keep = true;
                                rec = make_ulonglong2(((unsigned long long)s1 << 32) | (unsigned long long)k1,
                                                      ((unsigned long long)s2 << 32) | (unsigned long long)k2);
                                max_bin = max(max_bin, (unsigned long long)max(k1, k2));
                            }
                        }
                    }
                }
            }
            if (why) atomicMin(&words->first_error, error_word(line_base + r + 1, why));
        }
        const unsigned long long pos = fhx::block_append(keep, &words->n_records, capacity);
        if (keep) {
            if (pos != fhx::APPEND_OVER) records[pos] = rec;
            else atomicMin(&words->first_error, error_word(line_base + B.row0 + e + 1, FHX_VP_INTERNAL));
        }
        __syncthreads();                                    // block_append's LDS word is written again in the next round
    }
    for (int s = 32; s >= 1; s >>= 1) max_bin = max(max_bin, (unsigned long long)__shfl_down(max_bin, s, 64));
    if ((threadIdx.x & 63) == 0 && max_bin) atomicMax(&words->max_bin, max_bin);
}

// ---- the text order of the bin starts ------------------------------------------------------------------------------------
// keys[k] = the decimal string of k*res (below 2^31: at most 10 digits) as a word that sorts like the string followed by a tab
__global__ __launch_bounds__(WG) void vp_text_keys(long long res, int64_t n_bins, unsigned long long* __restrict__ keys) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_bins; k += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long v = (unsigned long long)(k * res);
        int len = 1;
        unsigned long long aligned = v;
        for (unsigned long long t = 10; t <= v; t *= 10) ++len;
        for (int d = len; d < 10; ++d) aligned *= 10;
        keys[k] = (aligned << 4) | (unsigned long long)len;
    }
}

// perm[i] = the bin at text rank i  ->  text_rank[bin] = i
__global__ __launch_bounds__(WG) void vp_invert(const unsigned int* __restrict__ perm, int64_t n_bins, unsigned int* __restrict__ text_rank) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_bins; i += (int64_t)gridDim.x * blockDim.x) text_rank[perm[i]] = (unsigned int)i;
}

__global__ __launch_bounds__(WG) void vp_keys(const ulonglong2* __restrict__ records, int64_t n, const int* __restrict__ slot_rank,
                                              const unsigned int* __restrict__ text_rank, int bin_bits, int name_bits,
                                              unsigned long long* __restrict__ keys) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const ulonglong2 r = records[i];
        const unsigned long long e1 = ((unsigned long long)slot_rank[r.x >> 32] << bin_bits) | text_rank[r.x & 0xFFFFFFFFull];
        const unsigned long long e2 = ((unsigned long long)slot_rank[r.y >> 32] << bin_bits) | text_rank[r.y & 0xFFFFFFFFull];
        keys[i] = (e1 << (bin_bits + name_bits)) | e2;
    }
}

// cell c = the run that starts at head_at[c]: its key decoded, its count = the distance to the next head
__global__ __launch_bounds__(WG) void vp_cells(const unsigned long long* __restrict__ keys, int64_t n, const unsigned long long* __restrict__ head_at,
                                               int64_t n_cells, const unsigned int* __restrict__ bin_at_rank, int bin_bits, int name_bits,
                                               long long res, int32_t* __restrict__ chr1, int32_t* __restrict__ mid1, int32_t* __restrict__ chr2,
                                               int32_t* __restrict__ mid2, int32_t* __restrict__ count, unsigned long long* __restrict__ max_count) {
    unsigned long long biggest = 0;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_cells; c += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long at = head_at[c];
        const unsigned long long cnt = (c + 1 < n_cells ? head_at[c + 1] : (unsigned long long)n) - at;
        const unsigned long long key = keys[at];
        const unsigned long long bin_mask = (1ull << bin_bits) - 1, name_mask = (1ull << name_bits) - 1;
        const unsigned long long e1 = key >> (bin_bits + name_bits), e2 = key & ((1ull << (bin_bits + name_bits)) - 1);
        chr1[c] = (int32_t)((e1 >> bin_bits) & name_mask);
        mid1[c] = (int32_t)((long long)bin_at_rank[e1 & bin_mask] * res + res / 2);
        chr2[c] = (int32_t)((e2 >> bin_bits) & name_mask);
        mid2[c] = (int32_t)((long long)bin_at_rank[e2 & bin_mask] * res + res / 2);
        count[c] = (int32_t)min(cnt, 0x7fffffffull);
        biggest = max(biggest, cnt);
    }
    for (int s = 32; s >= 1; s >>= 1) biggest = max(biggest, (unsigned long long)__shfl_down(biggest, s, 64));
    if ((threadIdx.x & 63) == 0 && biggest) atomicMax(max_count, biggest);
}

}  // namespace vpd

// ===================================================================================================================
struct fhx_vp : fhx::TextHandle {
    fhx_ctx* sorter = nullptr;
    // the last binned file
    std::vector<std::string> names;               // bytewise order: a cell's chr column is an index into it
    int64_t n_lines = 0, n_pairs = 0;
    fhx::CellColumns cols;
    double seconds[FHX_VP_STAGES] = {0, 0, 0, 0, 0, 0};
};

namespace {

void drop_cells(fhx_vp* vp) {
    vp->cols.drop();
    vp->names.clear();
    vp->n_lines = vp->n_pairs = 0;
}

int bits_for(unsigned long long largest) {                                    // bits that hold 0..largest, at least 1
    int b = 1;
    while (b < 64 && (largest >> b)) ++b;
    return b;
}

// fhx_vp_bin_file behind its argument check; whatever it returns but FHX_OK, the caller drops the cells
int bin_file(fhx_vp* vp, const char* path, int64_t res, int64_t* n_cells, int32_t* why, int64_t* bad_line) {
    using namespace vpd;
    TH_HIP(vp, hipSetDevice(vp->device));
    TH_HIP(vp, hipStreamSynchronize(vp->stream));
    drop_cells(vp);
    for (double& s : vp->seconds) s = 0;
    if (res < 2 || (res & 1) || res > 0x7fffffffll) {
        *why = FHX_VP_RES;
        return fhx::fail(vp, FHX_ERR_UNSUPPORTED, "the resolution must be an even number from 2 to 2^31 - 2");
    }
    fhx::StageClock clock{vp->seconds};
    fhx::DeviceScratch tmp;
    fhx::TextBatches in;                                                      // a gzip file is read as zcat -f reads it (:33)
    if (const int rc = in.open(vp, &tmp, &clock, path, "validPairs", "FHX_VP_BATCH_BYTES", (int64_t)1 << 32)) return rc;
    unsigned long long* d_names = nullptr;
    Words* d_words = nullptr;
    ulonglong2* d_records = nullptr;
    int64_t capacity = 0;
    TH_HIP(vp, tmp.get_n(&d_names, (size_t)NAME_SLOTS));
    TH_HIP(vp, tmp.get_n(&d_words, 1));
    TH_HIP(vp, hipMemsetAsync(d_names, 0, NAME_SLOTS * sizeof(unsigned long long), vp->stream));
    Words words;                                                              // running totals: set once, not per batch
    TH_HIP(vp, hipMemcpyAsync(d_words, &words, sizeof(words), hipMemcpyHostToDevice, vp->stream));
    TH_HIP(vp, hipStreamSynchronize(vp->stream));
    const fhx::Refusal refuse{vp, why, bad_line};
    int64_t pairs = 0;
    for (; in.more(); in.advance()) {
        if (const int rc = in.next<AnyByte>()) return rc;                     // this path's policy refuses no byte
        const int64_t n = in.lines;
        if (pairs + n >= ((int64_t)1 << 32)) return refuse(FHX_ERR_UNSUPPORTED, FHX_VP_PAIRS, 0, "2^32 or more pairs may be kept: the sort does not take them");
        TH_HIP(vp, tmp.grow_keep(&d_records, &capacity, pairs, pairs + n, vp->stream));        // room for every line of the batch to be kept
        hipLaunchKernelGGL(vp_parse, dim3((unsigned)in.n_blocks), dim3(WG), 0, vp->stream, (const unsigned char*)in.d_text, in.len,
                           (const unsigned long long*)in.d_block_off, n, in.line_base, (long long)res, d_names, d_records,
                           (unsigned long long)capacity, d_words);
        TH_HIP(vp, hipGetLastError());
        TH_HIP(vp, hipMemcpyAsync(&words, d_words, sizeof(words), hipMemcpyDeviceToHost, vp->stream));
        TH_HIP(vp, hipStreamSynchronize(vp->stream));
        clock.mark(2);
        if (words.first_error != NO_ERROR) return refuse.word(words.first_error, FHX_VP_INTERNAL);      // earlier batches hold the smaller line numbers
        pairs = (int64_t)words.n_records;
        if (pairs > capacity) return refuse(FHX_ERR_INTERNAL, FHX_VP_INTERNAL, 0, "more records than lines");
    }
    const int64_t lines = in.line_base;
    in.close();
    if (words.names_overflow || words.n_names > (unsigned long long)MAX_NAMES)       // after every line has been checked: a line error wins
        return refuse(FHX_ERR_UNSUPPORTED, FHX_VP_NAMES, 0, "more than " + std::to_string(MAX_NAMES) + " distinct chromosome names among the kept pairs");
    vp->n_lines = lines;
    vp->n_pairs = pairs;
    if (pairs == 0) {
        clock.mark(3);
        return FHX_OK;
    }
    // ---- names: ranked bytewise on the host (the packed words compare as the bytes do) --------------------------------------
    std::vector<unsigned long long> table((size_t)NAME_SLOTS);
    TH_HIP(vp, hipMemcpy(table.data(), d_names, NAME_SLOTS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    std::vector<std::pair<unsigned long long, int>> present;
    for (int s = 0; s < NAME_SLOTS; ++s)
        if (table[(size_t)s]) present.emplace_back(table[(size_t)s], s);
    std::sort(present.begin(), present.end());
    std::vector<int> slot_rank((size_t)NAME_SLOTS, 0);
    for (size_t k = 0; k < present.size(); ++k) {
        slot_rank[(size_t)present[k].second] = (int)k;
        std::string name;
        for (int b = 4; b >= 0; --b)
            if (const char c = (char)((present[k].first >> (8 * b)) & 0xFF)) name.push_back(c);
        vp->names.push_back(name);
    }
    const int64_t n_bins = (int64_t)words.max_bin + 1;
    const int bin_bits = bits_for(words.max_bin), name_bits = bits_for(present.size() - 1);
    if (2 * (bin_bits + name_bits) > 64)
        return refuse(FHX_ERR_UNSUPPORTED, FHX_VP_NAMES, 0,
                      std::to_string(present.size()) + " distinct names and bin indices up to " + std::to_string(words.max_bin) + " need " +
                          std::to_string(2 * (bin_bits + name_bits)) + " key bits, the sort key has 64");
    int* d_slot_rank = nullptr;
    unsigned int *d_text_rank = nullptr, *d_bin_at_rank = nullptr, *d_perm = nullptr;
    unsigned long long *d_keys = nullptr, *d_sorted = nullptr;
    TH_HIP(vp, tmp.get_n(&d_slot_rank, (size_t)NAME_SLOTS));
    TH_HIP(vp, hipMemcpyAsync(d_slot_rank, slot_rank.data(), NAME_SLOTS * sizeof(int), hipMemcpyHostToDevice, vp->stream));
    TH_HIP(vp, tmp.get_n(&d_text_rank, (size_t)n_bins));
    TH_HIP(vp, tmp.get_n(&d_bin_at_rank, (size_t)n_bins));
    {
        unsigned long long *d_bin_keys = nullptr, *d_bin_sorted = nullptr;
        TH_HIP(vp, tmp.get_n(&d_bin_keys, (size_t)n_bins));
        TH_HIP(vp, tmp.get_n(&d_bin_sorted, (size_t)n_bins));
        const unsigned grid = (unsigned)std::min<int64_t>((n_bins + WG - 1) / WG, 4096);
        hipLaunchKernelGGL(vp_text_keys, dim3(grid), dim3(WG), 0, vp->stream, (long long)res, n_bins, d_bin_keys);
        TH_HIP(vp, hipGetLastError());
        TH_HIP(vp, hipStreamSynchronize(vp->stream));                             // the sorter has a stream of its own
        const int rc = fhx_sort_u64(vp->sorter, d_bin_keys, n_bins, d_bin_sorted, d_bin_at_rank);
        if (rc != FHX_OK) return fhx::fail(vp, rc, std::string("sort of the bin starts: ") + fhx_last_error(vp->sorter));
        hipLaunchKernelGGL(vp_invert, dim3(grid), dim3(WG), 0, vp->stream, (const unsigned int*)d_bin_at_rank, n_bins, d_text_rank);
        TH_HIP(vp, hipGetLastError());
        TH_HIP(vp, hipStreamSynchronize(vp->stream));
        tmp.drop(d_bin_keys);
        tmp.drop(d_bin_sorted);
    }
    TH_HIP(vp, tmp.get_n(&d_keys, (size_t)pairs));
    {
        const unsigned grid = (unsigned)std::min<int64_t>((pairs + WG - 1) / WG, 8192);
        hipLaunchKernelGGL(vp_keys, dim3(grid), dim3(WG), 0, vp->stream, (const ulonglong2*)d_records, pairs, (const int*)d_slot_rank,
                           (const unsigned int*)d_text_rank, bin_bits, name_bits, d_keys);
        TH_HIP(vp, hipGetLastError());
        TH_HIP(vp, hipStreamSynchronize(vp->stream));
    }
    tmp.drop(d_records);
    d_records = nullptr;
    clock.mark(3);
    TH_HIP(vp, tmp.get_n(&d_sorted, (size_t)pairs));
    TH_HIP(vp, tmp.get_n(&d_perm, (size_t)pairs));
    {
        const int rc = fhx_sort_u64(vp->sorter, d_keys, pairs, d_sorted, d_perm);
        if (rc != FHX_OK) return fhx::fail(vp, rc, std::string("sort: ") + fhx_last_error(vp->sorter));
    }
    tmp.drop(d_keys);
    tmp.drop(d_perm);
    clock.mark(4);
    // ---- run heads -> cells --------------------------------------------------------------------------------------------------
    fhx::Heads heads;
    if (const int rc = fhx::run_heads(refuse, FHX_VP_INTERNAL, tmp, d_sorted, pairs, &d_words->n_cells, /*positions=*/true, &heads)) return rc;
    const int64_t cells = heads.cells;
    TH_HIP(vp, vp->cols.alloc(cells));
    const fhx::CellColumns& C = vp->cols;
    hipLaunchKernelGGL(vp_cells, dim3((unsigned)std::min<int64_t>((cells + WG - 1) / WG, 8192)), dim3(WG), 0, vp->stream,
                       (const unsigned long long*)d_sorted, pairs, (const unsigned long long*)heads.d_head_at, cells,
                       (const unsigned int*)d_bin_at_rank, bin_bits, name_bits, (long long)res, C.col(0), C.col(1), C.col(2), C.col(3), C.col(4),
                       &d_words->max_count);
    TH_HIP(vp, hipGetLastError());
    unsigned long long max_count = 0;
    TH_HIP(vp, hipMemcpyAsync(&max_count, &d_words->max_count, sizeof(max_count), hipMemcpyDeviceToHost, vp->stream));
    TH_HIP(vp, hipStreamSynchronize(vp->stream));
    clock.mark(5);
    if (max_count > 0x7fffffffull) return refuse(FHX_ERR_UNSUPPORTED, FHX_VP_COUNT, 0, "a cell is hit by more than 2^31 - 1 pairs: the count column is int32");
    *n_cells = cells;
    if (std::getenv("FHX_TIMING"))
        std::fprintf(stderr, "validPairs on the device (%s): %lld lines, %lld kept pairs, %lld cells: read + upload %.6f s; scan %.6f s; parse %.6f s; "
                     "names + keys %.6f s; sort %.6f s; cells %.6f s\n", path, (long long)lines, (long long)pairs, (long long)cells, vp->seconds[0],
                     vp->seconds[1], vp->seconds[2], vp->seconds[3], vp->seconds[4], vp->seconds[5]);
    return FHX_OK;
}

}  // namespace

extern "C" {

int fhx_vp_create(int device, fhx_vp** out) { return fhx::handle_create_with_sorter(device, out); }

void fhx_vp_destroy(fhx_vp* vp) {
    fhx::text_handle_destroy(vp, [&] {
        drop_cells(vp);
        fhx::drop_sorter(vp);
    });
}

const char* fhx_vp_last_error(const fhx_vp* vp) { return fhx::handle_last_error(vp); }

int fhx_vp_bin_file(fhx_vp* vp, const char* path, int64_t res, int64_t* n_cells, int32_t* why, int64_t* bad_line) {
    using namespace vpd;
    if (!vp || !path || !n_cells || !why || !bad_line) return FHX_ERR_ARG;
    *n_cells = 0;
    *why = FHX_VP_OK;
    *bad_line = 0;
    const int rc = bin_file(vp, path, res, n_cells, why, bad_line);
    if (rc != FHX_OK) drop_cells(vp);                                         // the one exit of a failed call, whatever failed
    return rc;
}

int fhx_vp_counts(const fhx_vp* vp, int64_t* n_lines, int64_t* n_pairs, int64_t* n_cells, int32_t* n_names) {
    if (!vp) return FHX_ERR_ARG;
    if (n_lines) *n_lines = vp->n_lines;
    if (n_pairs) *n_pairs = vp->n_pairs;
    if (n_cells) *n_cells = vp->cols.n;
    if (n_names) *n_names = (int32_t)vp->names.size();
    return FHX_OK;
}

const char* fhx_vp_name(const fhx_vp* vp, int32_t i) { return (vp && i >= 0 && i < (int32_t)vp->names.size()) ? vp->names[(size_t)i].c_str() : nullptr; }

int fhx_vp_stage_seconds(const fhx_vp* vp, double* seconds) {
    if (!vp || !seconds) return FHX_ERR_ARG;
    for (int k = 0; k < FHX_VP_STAGES; ++k) seconds[k] = vp->seconds[k];
    return FHX_OK;
}

int fhx_vp_fetch_cells(fhx_vp* vp, int32_t* chr1, int32_t* mid1, int32_t* chr2, int32_t* mid2, int32_t* count) {
    return vp ? vp->cols.fetch(vp, {chr1, mid1, chr2, mid2, count}) : FHX_ERR_ARG;
}

void* fhx_vp_device_ptr(fhx_vp* vp, int32_t which) { return vp ? vp->cols.ptr(which) : nullptr; }

void* fhx_vp_stream(fhx_vp* vp) { return vp ? (void*)vp->stream : nullptr; }

}  // extern "C"
