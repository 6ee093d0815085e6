// fhx_fragpairs.hip - HiC-Pro's allValidPairs (one line per read pair) binned to RESTRICTION FRAGMENTS on MI355X (gfx950): the
// contact counts that go with the fragments file of fithic_amd.digest for `fithic -r 0`.  The reference ships no script for
// this; the semantics are the project's own.  Parse, key, sort, count as in fhx_validpairs.hip, over the same
// shared layers (fhx_pairline.hpp, fhx_cells.hpp), with the grid division replaced by a search over the cut sites:
//
//   scan_text, scan_tiles    the newline layer (fhx_textlines.hpp) over batches cut at the last newline (fhx_textupload.hpp)
//   fp_parse       the lines that begin in a block, one per lane, one walk along the line (fhx_pairline.hpp): tokens 2, 3, 5, 6.  A
//                  name is hashed (64-bit FNV-1a) and probed in a 16384-slot table the host made of the table's names and the
//                  dropped ones; a hit counts only when the bytes equal the slot's text.  A position p lies in the fragment
//                  k = bisect_left(E_c, p) of its contig (the bed is 0-based and half-open, p is 1-based: start < p <= end),
//                  E_c being the contig's ascending fragment ends in HBM.  The pair becomes ONE word g1 << 32 | g2, g = the
//                  row of the fragment in the fragments file, g1 < g2, stored compacted (fhx::block_append: one atomicAdd per
//                  256 lines).  The two drop counts and the smallest bad line are reduced per wave first.
//   fhx_sort_u64   the stable radix sort; equal words are the pairs of one cell
//   fhx::run_heads, fp_cells    run heads (fhx_cells.hpp) -> cells (contig1, end1, contig2, end2, count); the contig of a
//                  row is found by bisection over the contigs' first rows, a count is the distance between two heads
//
// Nothing is approximated: a line outside the grammar (the header lists it) is REFUSED with the smallest offending line number
// (atomicMin over line << 8 | reason: the same answer whatever the launch order) and nothing stays loaded.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fithic_mi355x.h"
#include "fhx_cells.hpp"
#include "fhx_pairline.hpp"

namespace fpd {

using namespace fhxlines;

constexpr int SLOTS = 16384;                   // the name table (open addressing, at most half full)
constexpr int MAX_NAMES = FHX_FP_MAX_CONTIGS * 2;      // the table's names and the dropped ones that are none of them
constexpr int NAME_BYTES = FHX_FP_NAME_BYTES;  // a name's text, zero-padded: at most 63 bytes of name
constexpr int NOT_FOUND = -2, DROPPED = -1;    // what a name gives when it is no contig (0 .. n_contigs - 1)

// the words the kernels of one call share
struct Words {
    unsigned long long first_error = NO_ERROR; // smallest (line << 8 | reason)
    unsigned long long n_records = 0;          // kept pairs so far
    unsigned long long n_dropped_name = 0;     // lines dropped for a name of the drop list
    unsigned long long n_same_fragment = 0;    // lines whose two ends lie in one fragment
    unsigned long long n_cells = 0;            // scan_tiles' total of the heads
    unsigned long long max_count = 0;          // largest cell count
};

// what the kernels read of the fragment table, all of it in HBM
struct Table {
    const unsigned long long* slot_hash;       // SLOTS words, 0 = empty
    const int32_t* slot_name;                  // SLOTS: the name of the slot
    const unsigned char* name_text;            // n_names x NAME_BYTES
    const int32_t* name_contig;                // n_names: the contig, or DROPPED
    const int32_t* first;                      // n_contigs + 1: the row of every contig's first fragment, then n_frags
    const int32_t* ends;                       // n_frags: E, ascending within a contig
    int32_t n_contigs;
};

constexpr unsigned long long FNV_OFFSET = 0xcbf29ce484222325ull, FNV_PRIME = 0x100000001b3ull;
__host__ __device__ inline unsigned long long fnv1a(const unsigned char* s, int len) {
    unsigned long long h = FNV_OFFSET;
    for (int k = 0; k < len; ++k) h = (h ^ (unsigned long long)s[k]) * FNV_PRIME;
    return h ? h : 1ull;                       // 0 marks an empty slot
}
__host__ __device__ inline unsigned int slot_of(unsigned long long h) { return (unsigned int)((h ^ (h >> 32)) & (SLOTS - 1)); }

using fhxpair::position;

// the contig named by text[b, b + len), DROPPED, or NOT_FOUND.  An equal hash is no hit until the bytes are.
__device__ inline int lookup(const Table& t, const unsigned char* __restrict__ text, int64_t b, int len) {
    if (len < 1 || len >= NAME_BYTES) return NOT_FOUND;
    const unsigned long long h = fnv1a(text + b, len);
    unsigned int s = slot_of(h);
    for (int probe = 0; probe < SLOTS; ++probe, s = (s + 1) & (SLOTS - 1)) {
        const unsigned long long v = t.slot_hash[s];
        if (v == 0) return NOT_FOUND;
        if (v != h) continue;
        const int32_t id = t.slot_name[s];
        const unsigned char* name = t.name_text + (size_t)id * NAME_BYTES;
        bool same = name[len] == 0;
        for (int k = 0; k < len && same; ++k) same = name[k] == text[b + k];
        if (same) return t.name_contig[id];
    }
    return NOT_FOUND;
}

// bisect_left(E_c, p) as a row of the whole table; 1 <= p <= the contig's length = its last end, so the answer is a row of c.
// An empty fragment repeats the end before it (or is 0 0): of equal ends the first is taken, and that one is not empty.
__device__ inline int32_t fragment_of(const Table& t, int c, int32_t p) {
    int32_t lo = t.first[c], hi = t.first[c + 1] - 1;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (t.ends[mid] < p) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(WG) void fp_parse(const unsigned char* __restrict__ text, int64_t T, const unsigned long long* __restrict__ block_off,
                                               int64_t n_lines_batch, int64_t line_base, Table table, unsigned long long* __restrict__ records,
                                               unsigned long long capacity, Words* __restrict__ words) {
    __shared__ unsigned short lstart[LSTART_ENTRIES];
    const BlockLines B = block_lines(text, T, block_off, lstart);
    unsigned long long first_error = NO_ERROR;
    unsigned int dropped_name = 0, same_fragment = 0;
    for (int base = 0; base < B.n_lines; base += WG) {      // n_lines is the same for every lane: the scans below see whole blocks
        const int e = base + threadIdx.x;
        bool keep = false;
        unsigned long long rec = 0;
        if (e < B.n_lines) {
            const int64_t r = B.row0 + e;
            const fhxpair::Line L = fhxpair::walk(text, T, B.b0 + lstart[e]);
            int why = L.stop == fhxpair::STOP_LONG_LINE ? FHX_FP_LONG_LINE : L.stop == fhxpair::STOP_BYTES ? FHX_FP_BYTES : 0;
            if (!why && L.tok < 6) why = FHX_FP_TOKENS;
            if (!why && r >= n_lines_batch) why = FHX_FP_INTERNAL;           // the scan and this kernel disagree about the lines
            if (!why) {
                const int l1 = L.len(0), l2 = L.len(2);
                bool same_name = l1 == l2;                                    // most pairs are cis: one lookup then
                for (int k = 0; k < l1 && same_name; ++k) same_name = text[L.tb[0] + k] == text[L.tb[2] + k];
                const int c1 = lookup(table, text, L.tb[0], l1);
                const int c2 = same_name ? c1 : lookup(table, text, L.tb[2], l2);
                long long p1 = 0, p2 = 0;
                if (c1 == DROPPED || c2 == DROPPED) ++dropped_name;           // the line is not read further
                else if (c1 == NOT_FOUND || c2 == NOT_FOUND) why = FHX_FP_NAME;
                else if (!position(text, L.tb[1], L.len(1), &p1) || !position(text, L.tb[3], L.len(3), &p2)) why = FHX_FP_POSITION;
                else if (p1 < 1 || p2 < 1 || p1 > (long long)table.ends[table.first[c1 + 1] - 1] || p2 > (long long)table.ends[table.first[c2 + 1] - 1])
                    why = FHX_FP_RANGE;
                else {
                    const int32_t g1 = fragment_of(table, c1, (int32_t)p1), g2 = fragment_of(table, c2, (int32_t)p2);
                    if (g1 == g2) ++same_fragment;
                    else {
                        keep = true;
                        rec = ((unsigned long long)(unsigned int)min(g1, g2) << 32) | (unsigned long long)(unsigned int)max(g1, g2);
                    }
                }
            }
            if (why) first_error = min(first_error, error_word(line_base + r + 1, why));
        }
        const unsigned long long pos = fhx::block_append(keep, &words->n_records, capacity);
        if (keep) {
            if (pos != fhx::APPEND_OVER) records[pos] = rec;
            else first_error = min(first_error, error_word(line_base + B.row0 + e + 1, FHX_FP_INTERNAL));
        }
        __syncthreads();                                    // block_append's LDS word is written again in the next round
    }
    for (int s = 32; s >= 1; s >>= 1) {
        first_error = min(first_error, (unsigned long long)__shfl_down(first_error, s, 64));
        dropped_name += __shfl_down(dropped_name, s, 64);
        same_fragment += __shfl_down(same_fragment, s, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (first_error != NO_ERROR) atomicMin(&words->first_error, first_error);
        if (dropped_name) atomicAdd(&words->n_dropped_name, (unsigned long long)dropped_name);
        if (same_fragment) atomicAdd(&words->n_same_fragment, (unsigned long long)same_fragment);
    }
}

// the contig of row g: the last c with first[c] <= g (a contig has at least one fragment: first is strictly ascending)
__device__ inline int32_t contig_of(const int32_t* __restrict__ first, int32_t n_contigs, int32_t g) {
    int32_t lo = 0, hi = n_contigs - 1;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo + 1) >> 1);
        if (first[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// cell c = the run that starts at head_at[c]: its key decoded, its count = the distance to the next head
__global__ __launch_bounds__(WG) void fp_cells(const unsigned long long* __restrict__ keys, int64_t n, const unsigned long long* __restrict__ head_at,
                                               int64_t n_cells, const int32_t* __restrict__ first, int32_t n_contigs, int32_t n_frags,
                                               const int32_t* __restrict__ ends, int32_t* __restrict__ chr1, int32_t* __restrict__ end1,
                                               int32_t* __restrict__ chr2, int32_t* __restrict__ end2, int32_t* __restrict__ count,
                                               unsigned long long* __restrict__ max_count) {
    unsigned long long biggest = 0;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_cells; c += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long at = head_at[c];
        const unsigned long long cnt = (c + 1 < n_cells ? head_at[c + 1] : (unsigned long long)n) - at;
        const unsigned long long key = keys[at];
        const unsigned int last = (unsigned int)(n_frags - 1);              // the rows are below n_frags by construction
        const int32_t g1 = (int32_t)min((unsigned int)(key >> 32), last), g2 = (int32_t)min((unsigned int)(key & 0xFFFFFFFFull), last);
        chr1[c] = contig_of(first, n_contigs, g1);
        end1[c] = ends[g1];
        chr2[c] = contig_of(first, n_contigs, g2);
        end2[c] = ends[g2];
        count[c] = (int32_t)min(cnt, 0x7fffffffull);
        biggest = max(biggest, cnt);
    }
    for (int s = 32; s >= 1; s >>= 1) biggest = max(biggest, (unsigned long long)__shfl_down(biggest, s, 64));
    if ((threadIdx.x & 63) == 0 && biggest) atomicMax(max_count, biggest);
}

}  // namespace fpd

// ===================================================================================================================
struct fhx_fp : fhx::TextHandle {
    fhx_ctx* sorter = nullptr;
    // the fragment table (fhx_fp_load_table)
    int32_t n_contigs = 0, n_names = 0;
    int64_t n_frags = 0;
    unsigned long long* d_slot_hash = nullptr;
    int32_t *d_slot_name = nullptr, *d_name_contig = nullptr, *d_first = nullptr, *d_ends = nullptr;
    unsigned char* d_name_text = nullptr;
    double table_seconds = 0;
    // the last binned file
    int64_t n_lines = 0, n_pairs = 0, n_dropped_name = 0, n_same_fragment = 0;
    fhx::CellColumns cols;
    double seconds[FHX_FP_STAGES] = {0, 0, 0, 0, 0, 0};
};

namespace {

void drop_cells(fhx_fp* fp) {
    fp->cols.drop();
    fp->n_lines = fp->n_pairs = fp->n_dropped_name = fp->n_same_fragment = 0;
}

void drop_table(fhx_fp* fp) {
    fhx::dev_free(fp->d_slot_hash);
    fhx::dev_free(fp->d_slot_name);
    fhx::dev_free(fp->d_name_contig);
    fhx::dev_free(fp->d_first);
    fhx::dev_free(fp->d_ends);
    fhx::dev_free(fp->d_name_text);
    fp->n_contigs = fp->n_names = 0;
    fp->n_frags = 0;
}

// fhx_fp_load_table behind its argument check; whatever it returns but FHX_OK, the caller drops the table
int load_table(fhx_fp* fp, const char* name_text, const int32_t* name_contig, int32_t n_names, const int64_t* first, int32_t n_contigs,
               const int32_t* ends, int64_t n_frags) {
    using namespace fpd;
    using fhx::upload;
    if (n_contigs > FHX_FP_MAX_CONTIGS) return fhx::fail(fp, FHX_ERR_UNSUPPORTED, "more than " + std::to_string(FHX_FP_MAX_CONTIGS) + " contigs");
    if (n_names > MAX_NAMES) return fhx::fail(fp, FHX_ERR_UNSUPPORTED, "more than " + std::to_string(MAX_NAMES) + " names, the contigs' and the dropped ones together");
    if (n_frags > 0x7fffffffll) return fhx::fail(fp, FHX_ERR_UNSUPPORTED, "2^31 or more fragments");
    // the rows: every contig has at least one fragment, its ends ascend from 0 upwards
    std::vector<int32_t> first32((size_t)n_contigs + 1);
    if (first[0] != 0 || first[n_contigs] != n_frags) return fhx::fail(fp, FHX_ERR_ARG, "first[0] is not 0, or first[n_contigs] is not n_frags");
    for (int32_t c = 0; c < n_contigs; ++c) {
        if (first[c + 1] <= first[c] || first[c + 1] > n_frags) return fhx::fail(fp, FHX_ERR_ARG, "contig " + std::to_string(c) + " has no fragment, or rows beyond n_frags");
        first32[(size_t)c] = (int32_t)first[c];
        for (int64_t g = first[c]; g < first[c + 1]; ++g)
            if (ends[g] < 0 || (g > first[c] && ends[g] < ends[g - 1]))
                return fhx::fail(fp, FHX_ERR_ARG, "the fragment ends of contig " + std::to_string(c) + " do not ascend from 0 upwards");
    }
    first32[(size_t)n_contigs] = (int32_t)n_frags;
    // the names: 1 to 63 bytes each, no two equal; every contig is named once
    std::vector<unsigned long long> slot_hash((size_t)SLOTS, 0ull);
    std::vector<int32_t> slot_name((size_t)SLOTS, 0);
    for (int32_t k = 0; k < n_names; ++k) {
        const unsigned char* name = (const unsigned char*)name_text + (size_t)k * NAME_BYTES;
        int len = 0;
        while (len < NAME_BYTES && name[len]) ++len;
        if (len < 1 || len >= NAME_BYTES) return fhx::fail(fp, FHX_ERR_UNSUPPORTED, "name " + std::to_string(k) + " is empty or longer than 63 bytes");
        for (int b = len; b < NAME_BYTES; ++b)
            if (name[b]) return fhx::fail(fp, FHX_ERR_ARG, "name " + std::to_string(k) + " is not zero-padded");
        if (name_contig[k] < DROPPED || name_contig[k] >= n_contigs) return fhx::fail(fp, FHX_ERR_ARG, "name " + std::to_string(k) + " names no contig of the table");
        const unsigned long long h = fnv1a(name, len);
        unsigned int s = slot_of(h);
        for (; slot_hash[s]; s = (s + 1) & (SLOTS - 1))                        // at most half full: an empty slot is met
            if (slot_hash[s] == h && std::memcmp(name_text + (size_t)slot_name[s] * NAME_BYTES, name, NAME_BYTES) == 0)
                return fhx::fail(fp, FHX_ERR_ARG, "name " + std::to_string(k) + " is given twice");
        slot_hash[s] = h;
        slot_name[s] = k;
    }
    TH_HIP(fp, hipSetDevice(fp->device));
    if (const int rc = upload(fp, &fp->d_slot_hash, slot_hash.data(), (size_t)SLOTS)) return rc;
    if (const int rc = upload(fp, &fp->d_slot_name, slot_name.data(), (size_t)SLOTS)) return rc;
    if (const int rc = upload(fp, &fp->d_name_text, (const unsigned char*)name_text, (size_t)n_names * NAME_BYTES)) return rc;
    if (const int rc = upload(fp, &fp->d_name_contig, name_contig, (size_t)n_names)) return rc;
    if (const int rc = upload(fp, &fp->d_first, first32.data(), first32.size())) return rc;
    if (const int rc = upload(fp, &fp->d_ends, ends, (size_t)n_frags)) return rc;
    TH_HIP(fp, hipStreamSynchronize(fp->stream));                             // the host arrays go out of scope
    fp->n_contigs = n_contigs;
    fp->n_names = n_names;
    fp->n_frags = n_frags;
    return FHX_OK;
}

// fhx_fp_bin_file behind its argument check; whatever it returns but FHX_OK, the caller drops the cells
int bin_file(fhx_fp* fp, const char* path, int64_t* n_cells, int32_t* why, int64_t* bad_line) {
    using namespace fpd;
    TH_HIP(fp, hipSetDevice(fp->device));
    TH_HIP(fp, hipStreamSynchronize(fp->stream));
    drop_cells(fp);
    for (double& s : fp->seconds) s = 0;
    fp->seconds[5] = fp->table_seconds;
    if (fp->n_contigs < 1) return fhx::fail(fp, FHX_ERR_ARG, "no fragment table is loaded (fhx_fp_load_table)");
    const Table table{fp->d_slot_hash, fp->d_slot_name, fp->d_name_text, fp->d_name_contig, fp->d_first, fp->d_ends, fp->n_contigs};
    fhx::StageClock clock{fp->seconds};
    fhx::DeviceScratch tmp;
    fhx::TextBatches in;                                                      // a gzip file is inflated on the host first
    if (const int rc = in.open(fp, &tmp, &clock, path, "validPairs", "FHX_FP_BATCH_BYTES", (int64_t)1 << 32)) return rc;
    Words* d_words = nullptr;
    unsigned long long* d_records = nullptr;
    int64_t capacity = 0;
    TH_HIP(fp, tmp.get_n(&d_words, 1));
    Words words;                                                              // running totals: set once, not per batch
    TH_HIP(fp, hipMemcpyAsync(d_words, &words, sizeof(words), hipMemcpyHostToDevice, fp->stream));
    TH_HIP(fp, hipStreamSynchronize(fp->stream));
    const fhx::Refusal refuse{fp, why, bad_line};
    int64_t pairs = 0;
    for (; in.more(); in.advance()) {
        if (const int rc = in.next<AnyByte>()) return rc;                     // this path's policy refuses no byte: fp_parse names the line
        const int64_t n = in.lines;
        if (pairs + n >= ((int64_t)1 << 32)) return refuse(FHX_ERR_UNSUPPORTED, FHX_FP_PAIRS, 0, "2^32 or more pairs may be kept: the sort does not take them");
        TH_HIP(fp, tmp.grow_keep(&d_records, &capacity, pairs, pairs + n, fp->stream));        // room for every line of the batch to be kept
        hipLaunchKernelGGL(fp_parse, dim3((unsigned)in.n_blocks), dim3(WG), 0, fp->stream, (const unsigned char*)in.d_text, in.len,
                           (const unsigned long long*)in.d_block_off, n, in.line_base, table, d_records, (unsigned long long)capacity, d_words);
        TH_HIP(fp, hipGetLastError());
        TH_HIP(fp, hipMemcpyAsync(&words, d_words, sizeof(words), hipMemcpyDeviceToHost, fp->stream));
        TH_HIP(fp, hipStreamSynchronize(fp->stream));
        clock.mark(2);
        if (words.first_error != NO_ERROR) return refuse.word(words.first_error, FHX_FP_INTERNAL);      // earlier batches hold the smaller line numbers
        pairs = (int64_t)words.n_records;
        if (pairs > capacity) return refuse(FHX_ERR_INTERNAL, FHX_FP_INTERNAL, 0, "more records than lines");
    }
    const int64_t lines = in.line_base;
    in.close();
    if ((unsigned long long)lines != words.n_records + words.n_dropped_name + words.n_same_fragment)
        return refuse(FHX_ERR_INTERNAL, FHX_FP_INTERNAL, 0, "the kept and the dropped lines do not add up to the lines read");
    fp->n_lines = lines;
    fp->n_pairs = pairs;
    fp->n_dropped_name = (int64_t)words.n_dropped_name;
    fp->n_same_fragment = (int64_t)words.n_same_fragment;
    if (pairs == 0) return FHX_OK;
    // ---- the records are the sort keys ------------------------------------------------------------------------------------------
    unsigned long long* d_sorted = nullptr;
    unsigned int* d_perm = nullptr;
    TH_HIP(fp, tmp.get_n(&d_sorted, (size_t)pairs));
    TH_HIP(fp, tmp.get_n(&d_perm, (size_t)pairs));
    {
        const int rc = fhx_sort_u64(fp->sorter, d_records, pairs, d_sorted, d_perm);      // the sorter has a stream of its own; this one is idle
        if (rc != FHX_OK) return fhx::fail(fp, rc, std::string("sort: ") + fhx_last_error(fp->sorter));
    }
    tmp.drop(d_records);
    tmp.drop(d_perm);
    clock.mark(3);
    // ---- run heads -> cells --------------------------------------------------------------------------------------------------
    fhx::Heads heads;
    if (const int rc = fhx::run_heads(refuse, FHX_FP_INTERNAL, tmp, d_sorted, pairs, &d_words->n_cells, /*positions=*/true, &heads)) return rc;
    const int64_t cells = heads.cells;
    TH_HIP(fp, fp->cols.alloc(cells));
    const fhx::CellColumns& C = fp->cols;
    hipLaunchKernelGGL(fp_cells, dim3((unsigned)std::min<int64_t>((cells + WG - 1) / WG, 8192)), dim3(WG), 0, fp->stream,
                       (const unsigned long long*)d_sorted, pairs, (const unsigned long long*)heads.d_head_at, cells, (const int32_t*)fp->d_first,
                       fp->n_contigs, (int32_t)fp->n_frags, (const int32_t*)fp->d_ends, C.col(0), C.col(1), C.col(2), C.col(3), C.col(4),
                       &d_words->max_count);
    TH_HIP(fp, hipGetLastError());
    unsigned long long max_count = 0;
    TH_HIP(fp, hipMemcpyAsync(&max_count, &d_words->max_count, sizeof(max_count), hipMemcpyDeviceToHost, fp->stream));
    TH_HIP(fp, hipStreamSynchronize(fp->stream));
    clock.mark(4);
    if (max_count > 0x7fffffffull) return refuse(FHX_ERR_UNSUPPORTED, FHX_FP_COUNT, 0, "a cell is hit by more than 2^31 - 1 pairs: the count column is int32");
    *n_cells = cells;
    if (std::getenv("FHX_TIMING"))
        std::fprintf(stderr, "validPairs to fragments on the device (%s): %lld lines, %lld kept pairs, %lld cells: read + upload %.6f s; scan %.6f s; "
                     "parse %.6f s; sort %.6f s; cells %.6f s\n", path, (long long)lines, (long long)pairs, (long long)cells, fp->seconds[0],
                     fp->seconds[1], fp->seconds[2], fp->seconds[3], fp->seconds[4]);
    return FHX_OK;
}

}  // namespace

extern "C" {

int fhx_fp_create(int device, fhx_fp** out) { return fhx::handle_create_with_sorter(device, out); }

void fhx_fp_destroy(fhx_fp* fp) {
    fhx::text_handle_destroy(fp, [&] {
        drop_cells(fp);
        drop_table(fp);
        fhx::drop_sorter(fp);
    });
}

const char* fhx_fp_last_error(const fhx_fp* fp) { return fhx::handle_last_error(fp); }

int fhx_fp_load_table(fhx_fp* fp, const char* name_text, const int32_t* name_contig, int32_t n_names, const int64_t* first, int32_t n_contigs,
                      const int32_t* ends, int64_t n_frags) {
    if (!fp || !name_text || !name_contig || !first || !ends || n_names < 1 || n_contigs < 1 || n_frags < 1) return FHX_ERR_ARG;
    const auto t0 = std::chrono::steady_clock::now();
    if (hipSetDevice(fp->device) == hipSuccess) (void)hipStreamSynchronize(fp->stream);
    drop_cells(fp);
    drop_table(fp);
    const int rc = load_table(fp, name_text, name_contig, n_names, first, n_contigs, ends, n_frags);
    if (rc != FHX_OK) drop_table(fp);
    fp->table_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

int fhx_fp_bin_file(fhx_fp* fp, const char* path, int64_t* n_cells, int32_t* why, int64_t* bad_line) {
    if (!fp || !path || !n_cells || !why || !bad_line) return FHX_ERR_ARG;
    *n_cells = 0;
    *why = FHX_FP_OK;
    *bad_line = 0;
    const int rc = bin_file(fp, path, n_cells, why, bad_line);
    if (rc != FHX_OK) drop_cells(fp);                                         // the one exit of a failed call, whatever failed
    return rc;
}

int fhx_fp_counts(const fhx_fp* fp, int64_t* n_lines, int64_t* n_pairs, int64_t* n_dropped_name, int64_t* n_same_fragment, int64_t* n_cells) {
    if (!fp) return FHX_ERR_ARG;
    if (n_lines) *n_lines = fp->n_lines;
    if (n_pairs) *n_pairs = fp->n_pairs;
    if (n_dropped_name) *n_dropped_name = fp->n_dropped_name;
    if (n_same_fragment) *n_same_fragment = fp->n_same_fragment;
    if (n_cells) *n_cells = fp->cols.n;
    return FHX_OK;
}

int fhx_fp_stage_seconds(const fhx_fp* fp, double* seconds) {
    if (!fp || !seconds) return FHX_ERR_ARG;
    for (int k = 0; k < FHX_FP_STAGES; ++k) seconds[k] = fp->seconds[k];
    return FHX_OK;
}

int fhx_fp_fetch_cells(fhx_fp* fp, int32_t* chr1, int32_t* end1, int32_t* chr2, int32_t* end2, int32_t* count) {
    return fp ? fp->cols.fetch(fp, {chr1, end1, chr2, end2, count}) : FHX_ERR_ARG;
}

void* fhx_fp_device_ptr(fhx_fp* fp, int32_t which) { return fp ? fp->cols.ptr(which) : nullptr; }

void* fhx_fp_stream(fhx_fp* fp) { return fp ? (void*)fp->stream : nullptr; }

}  // extern "C"
