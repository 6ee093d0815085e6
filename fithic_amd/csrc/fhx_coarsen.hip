// fhx_coarsen.hip - contact rows that sit in HBM summed onto N-fold coarser loci on MI355X (gfx950): a fixed-size map at R taken
// to N*R, or the single fragments of a digest taken to meta-fragments of N, without another pass over the read pairs.  The
// reference has no script for this step; the semantics are the project's own.  The host makes the
// PLAN (fithic_amd/coarsen.py: which coarse locus every fine locus belongs to); the rows are re-keyed, sorted and summed here:
//
//   cz_keys        one row per lane: each end (chr, mid) is found in the fine table by bisection over its chromosome's ascending
//                  mids (fp_parse's layout: first[n_chr + 1] and one ascending column), group_of gives the coarse rows g1, g2,
//                  swapped to g1 <= g2.  The row becomes ONE word g1 << 32 | g2 and its count, both stored compacted (a
//                  diagonal row may be dropped; fhx::block_append: one atomicAdd per 256 rows).  The smallest bad row and the
//                  diagonal count are reduced per wave first.
//   fhx_sort_u64   the stable radix sort; its permutation says which count belongs to a sorted key
//   fhx::run_heads              the number of run heads of the sorted keys (fhx_cells.hpp, up to the count)
//   cz_tile_sums / scan_tiles / cz_heads    the 64-bit ordered scan of the permuted counts: per-tile sums, their exclusive
//                  scan (fhx_scan.hpp's, on 64-bit values), then every head's position and the exclusive prefix of the counts in front of it.  No loop over a run:
//                  one cell may hold every row of the input.  2^31 rows of 2^31 - 1 fit 63 bits.
//   cz_cells       one cell per lane: its sum is the difference of the prefixes at two heads; five int32 columns, lanes on
//                  consecutive cells; the largest sum and the first cell above 2^31 - 1 are reduced per wave
//
// A row whose end is no locus of the table or whose count is negative REFUSES the call with the smallest such 0-based row
// (atomicMin over row << 8 | reason: the same answer whatever the launch order) and nothing stays loaded.
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

namespace czd {

constexpr int WG = 256;
constexpr unsigned long long NO_ERROR = ~0ull;
constexpr unsigned long long INT32_TOP = 0x7fffffffull;

// the words the kernels of one call share
struct Words {
    unsigned long long first_error = NO_ERROR; // smallest (row << 8 | reason)
    unsigned long long n_records = 0;          // kept rows
    unsigned long long n_diagonal = 0;         // rows dropped as diagonal
    unsigned long long n_cells = 0;            // scan_tiles' total of the heads
    unsigned long long total = 0;              // scan_tiles' total of the counts
    unsigned long long max_sum = 0;            // largest cell sum
    unsigned long long first_big = NO_ERROR;   // smallest (cell << 8 | FHX_CZ_SUM)
};

// what cz_keys reads of the plan, all of it in HBM
struct Plan {
    const int32_t* first;                      // n_chr + 1: the row of every chromosome id's first locus, then n_fine
    const int32_t* mids;                       // n_fine: ascending within a chromosome
    const int32_t* group_of;                   // n_fine: the coarse row
    int32_t n_chr;
};

// the row of (chr, mid) in the fine table, -1 when it is no locus of it
__device__ inline int32_t locus_of(const Plan& p, int32_t chr, int32_t mid) {
    if (chr < 0 || chr >= p.n_chr) return -1;
    int32_t lo = p.first[chr];
    const int32_t end = p.first[chr + 1];
    int32_t hi = end;
    while (lo < hi) {
        const int32_t m = lo + ((hi - lo) >> 1);
        if (p.mids[m] < mid) lo = m + 1;
        else hi = m;
    }
    return lo < end && p.mids[lo] == mid ? lo : -1;
}

__global__ __launch_bounds__(WG) void cz_keys(const int32_t* __restrict__ chr1, const int32_t* __restrict__ mid1, const int32_t* __restrict__ chr2,
                                              const int32_t* __restrict__ mid2, const int32_t* __restrict__ count, int64_t n, Plan plan, int keep_diagonal,
                                              unsigned long long* __restrict__ keys, int32_t* __restrict__ kept_count, Words* __restrict__ words) {
    const int64_t r = (int64_t)blockIdx.x * WG + threadIdx.x;
    unsigned long long first_error = NO_ERROR, key = 0;
    unsigned int diagonal = 0;
    bool keep = false;
    int32_t cnt = 0;
    if (r < n) {
        const int32_t f1 = locus_of(plan, chr1[r], mid1[r]), f2 = locus_of(plan, chr2[r], mid2[r]);
        cnt = count[r];
        if (f1 < 0 || f2 < 0) first_error = ((unsigned long long)r << 8) | FHX_CZ_LOCUS;
        else if (cnt < 0) first_error = ((unsigned long long)r << 8) | FHX_CZ_COUNT;
        else {
            const int32_t a = plan.group_of[f1], b = plan.group_of[f2];
            if (a == b && !keep_diagonal) diagonal = 1;
            else {
                keep = true;
                key = ((unsigned long long)(unsigned int)min(a, b) << 32) | (unsigned long long)(unsigned int)max(a, b);
            }
        }
    }
    const unsigned long long pos = fhx::block_append(keep, &words->n_records, (unsigned long long)n);
    if (keep) {
        if (pos != fhx::APPEND_OVER) {                       // room for every row: n words were allocated
            keys[pos] = key;
            kept_count[pos] = cnt;
        } else first_error = min(first_error, ((unsigned long long)r << 8) | FHX_CZ_INTERNAL);
    }
    for (int s = 32; s >= 1; s >>= 1) {
        first_error = min(first_error, (unsigned long long)__shfl_down(first_error, s, 64));
        diagonal += __shfl_down(diagonal, s, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (first_error != NO_ERROR) atomicMin(&words->first_error, first_error);
        if (diagonal) atomicAdd(&words->n_diagonal, (unsigned long long)diagonal);
    }
}

// the counts in the order of the sorted keys, and their sum per tile of fhxscan::TILE
__global__ __launch_bounds__(fhxscan::THREADS) void cz_tile_sums(const unsigned int* __restrict__ perm, const int32_t* __restrict__ kept_count, int64_t n,
                                                                 int32_t* __restrict__ sorted_count, unsigned long long* __restrict__ tile_sums) {
    const int64_t base = (int64_t)blockIdx.x * fhxscan::TILE + (int64_t)threadIdx.x * fhxscan::SCAN_ITEMS;
    unsigned long long s = 0;
    for (int k = 0; k < fhxscan::SCAN_ITEMS; ++k)
        if (base + k < n) {
            const int64_t from = (int64_t)perm[base + k];                          // a permutation of 0 .. n - 1 by construction
            const int32_t v = kept_count[from < n ? from : n - 1];
            sorted_count[base + k] = v;
            s += (unsigned long long)(unsigned int)v;                              // cz_keys kept no negative count
        }
    unsigned long long total;
    fhxscan::block_exclusive_scan(s, &total);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// the run heads of the sorted keys, in order: where each run starts and the sum of the counts in front of it
__global__ __launch_bounds__(fhxscan::THREADS) void cz_heads(const unsigned long long* __restrict__ keys, const int32_t* __restrict__ sorted_count,
                                                             int64_t n, const unsigned long long* __restrict__ tile_offsets,
                                                             const unsigned long long* __restrict__ tile_prefix, int64_t n_cells,
                                                             unsigned long long* __restrict__ head_at, unsigned long long* __restrict__ prefix_at) {
    const int64_t base = (int64_t)blockIdx.x * fhxscan::TILE + (int64_t)threadIdx.x * fhxscan::SCAN_ITEMS;
    unsigned int c = 0;
    unsigned long long s = 0;
    bool head[fhxscan::SCAN_ITEMS];
    unsigned int value[fhxscan::SCAN_ITEMS];
    for (int k = 0; k < fhxscan::SCAN_ITEMS; ++k) {
        const bool in = base + k < n;
        head[k] = in && fhxscan::is_head(keys, base + k);
        value[k] = in ? (unsigned int)sorted_count[base + k] : 0u;
        c += head[k] ? 1u : 0u;
        s += value[k];
    }
    unsigned int heads;
    unsigned long long sum;
    unsigned long long pos = tile_offsets[blockIdx.x] + fhxscan::block_exclusive_scan(c, &heads);
    unsigned long long before = tile_prefix[blockIdx.x] + fhxscan::block_exclusive_scan(s, &sum);
    for (int k = 0; k < fhxscan::SCAN_ITEMS; ++k) {
        if (head[k] && (int64_t)pos < n_cells) {
            head_at[pos] = (unsigned long long)(base + k);
            prefix_at[pos] = before;
            ++pos;
        }
        before += value[k];
    }
}

// cell c = the run that starts at head_at[c]: its key decoded to the two coarse loci, its sum = the distance between two prefixes
__global__ __launch_bounds__(WG) void cz_cells(const unsigned long long* __restrict__ keys, int64_t n, const unsigned long long* __restrict__ head_at,
                                               const unsigned long long* __restrict__ prefix_at, int64_t n_cells,
                                               const int32_t* __restrict__ coarse_chr, const int32_t* __restrict__ coarse_mid, int32_t n_coarse,
                                               int32_t* __restrict__ chr1, int32_t* __restrict__ mid1, int32_t* __restrict__ chr2,
                                               int32_t* __restrict__ mid2, int32_t* __restrict__ count, Words* __restrict__ words) {
    const int64_t c = (int64_t)blockIdx.x * WG + threadIdx.x;
    unsigned long long biggest = 0, first_big = NO_ERROR;
    if (c < n_cells) {
        const unsigned long long at = min(head_at[c], (unsigned long long)(n - 1));       // below n by construction
        const unsigned long long sum = (c + 1 < n_cells ? prefix_at[c + 1] : words->total) - prefix_at[c];
        const unsigned long long key = keys[at];
        const unsigned int last = (unsigned int)(n_coarse - 1);                          // the rows are below n_coarse by construction
        const int32_t g1 = (int32_t)min((unsigned int)(key >> 32), last), g2 = (int32_t)min((unsigned int)(key & 0xFFFFFFFFull), last);
        chr1[c] = coarse_chr[g1];
        mid1[c] = coarse_mid[g1];
        chr2[c] = coarse_chr[g2];
        mid2[c] = coarse_mid[g2];
        count[c] = (int32_t)min(sum, INT32_TOP);
        biggest = sum;
        if (sum > INT32_TOP) first_big = ((unsigned long long)c << 8) | FHX_CZ_SUM;
    }
    for (int s = 32; s >= 1; s >>= 1) {
        biggest = max(biggest, (unsigned long long)__shfl_down(biggest, s, 64));
        first_big = min(first_big, (unsigned long long)__shfl_down(first_big, s, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        if (biggest) atomicMax(&words->max_sum, biggest);
        if (first_big != NO_ERROR) atomicMin(&words->first_big, first_big);
    }
}

}  // namespace czd

// ===================================================================================================================
struct fhx_cz : fhx::Handle {
    fhx_ctx* sorter = nullptr;
    // the plan (fhx_cz_load_plan)
    int32_t n_chr = 0;
    int64_t n_fine = 0, n_coarse = 0;
    int32_t *d_first = nullptr, *d_mids = nullptr, *d_group_of = nullptr, *d_coarse_chr = nullptr, *d_coarse_mid = nullptr;
    double plan_seconds = 0;
    // the last coarsened rows
    int64_t n_rows = 0, n_diagonal = 0;
    fhx::CellColumns cols;
    double seconds[FHX_CZ_STAGES] = {0, 0, 0, 0, 0, 0};
};

namespace {

void drop_cells(fhx_cz* cz) {
    cz->cols.drop();
    cz->n_rows = cz->n_diagonal = 0;
}

void drop_plan(fhx_cz* cz) {
    fhx::dev_free(cz->d_first);
    fhx::dev_free(cz->d_mids);
    fhx::dev_free(cz->d_group_of);
    fhx::dev_free(cz->d_coarse_chr);
    fhx::dev_free(cz->d_coarse_mid);
    cz->n_chr = 0;
    cz->n_fine = cz->n_coarse = 0;
}

// fhx_cz_load_plan behind its argument check; whatever it returns but FHX_OK, the caller drops the plan
int load_plan(fhx_cz* cz, const int64_t* first, int32_t n_chr, const int32_t* fine_mid, const int32_t* group_of, int64_t n_fine,
              const int32_t* coarse_chr, const int32_t* coarse_mid, int64_t n_coarse) {
    using fhx::upload;
    if (n_fine > 0x7fffffffll) return fhx::fail(cz, FHX_ERR_UNSUPPORTED, "2^31 or more loci");
    if (n_coarse > n_fine) return fhx::fail(cz, FHX_ERR_ARG, "more coarse loci than fine ones");
    if (first[0] != 0 || first[n_chr] != n_fine) return fhx::fail(cz, FHX_ERR_ARG, "first[0] is not 0, or first[n_chr] is not n_fine");
    std::vector<int32_t> first32((size_t)n_chr + 1);
    for (int32_t c = 0; c < n_chr; ++c) {                                     // an id without loci has an empty range
        if (first[c + 1] < first[c] || first[c + 1] > n_fine) return fhx::fail(cz, FHX_ERR_ARG, "first does not ascend up to n_fine at chromosome id " + std::to_string(c));
        first32[(size_t)c] = (int32_t)first[c];
        for (int64_t g = first[c] + 1; g < first[c + 1]; ++g)
            if (fine_mid[g] <= fine_mid[g - 1]) return fhx::fail(cz, FHX_ERR_ARG, "the mids of chromosome id " + std::to_string(c) + " do not strictly ascend");
    }
    first32[(size_t)n_chr] = (int32_t)n_fine;
    for (int64_t g = 0; g < n_fine; ++g)
        if (group_of[g] < 0 || group_of[g] >= n_coarse) return fhx::fail(cz, FHX_ERR_ARG, "group_of[" + std::to_string(g) + "] is no coarse row");
    TH_HIP(cz, hipSetDevice(cz->device));
    if (const int rc = upload(cz, &cz->d_first, first32.data(), first32.size())) return rc;
    if (const int rc = upload(cz, &cz->d_mids, fine_mid, (size_t)n_fine)) return rc;
    if (const int rc = upload(cz, &cz->d_group_of, group_of, (size_t)n_fine)) return rc;
    if (const int rc = upload(cz, &cz->d_coarse_chr, coarse_chr, (size_t)n_coarse)) return rc;
    if (const int rc = upload(cz, &cz->d_coarse_mid, coarse_mid, (size_t)n_coarse)) return rc;
    TH_HIP(cz, hipStreamSynchronize(cz->stream));                             // the host arrays go out of scope
    cz->n_chr = n_chr;
    cz->n_fine = n_fine;
    cz->n_coarse = n_coarse;
    return FHX_OK;
}

// the rows d[0..4][0, n) -> the cells; the stream is idle on entry.  Whatever it returns but FHX_OK, the caller drops the cells.
int coarsen_rows(fhx_cz* cz, fhx::DeviceScratch& tmp, fhx::StageClock& clock, const int32_t* const* d, int64_t n, int keep_diagonal,
                 int64_t* n_cells, int32_t* why, int64_t* bad_row) {
    using namespace czd;
    if (cz->n_fine < 1) return fhx::fail(cz, FHX_ERR_ARG, "no plan is loaded (fhx_cz_load_plan)");
    if (n > 0x7fffffffll) return fhx::fail(cz, FHX_ERR_UNSUPPORTED, "2^31 or more rows");
    const fhx::Refusal refuse{cz, why, bad_row};
    cz->n_rows = n;
    if (n == 0) return FHX_OK;
    const Plan plan{cz->d_first, cz->d_mids, cz->d_group_of, cz->n_chr};
    Words* d_words = nullptr;
    unsigned long long* d_keys = nullptr;
    int32_t* d_kept_count = nullptr;
    TH_HIP(cz, tmp.get_n(&d_words, 1));
    TH_HIP(cz, tmp.get_n(&d_keys, (size_t)n));
    TH_HIP(cz, tmp.get_n(&d_kept_count, (size_t)n));
    Words words;
    TH_HIP(cz, hipMemcpyAsync(d_words, &words, sizeof(words), hipMemcpyHostToDevice, cz->stream));
    hipLaunchKernelGGL(cz_keys, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, cz->stream, d[0], d[1], d[2], d[3], d[4], n, plan, keep_diagonal,
                       d_keys, d_kept_count, d_words);
    TH_HIP(cz, hipGetLastError());
    TH_HIP(cz, hipMemcpyAsync(&words, d_words, sizeof(words), hipMemcpyDeviceToHost, cz->stream));
    TH_HIP(cz, hipStreamSynchronize(cz->stream));
    clock.mark(1);
    if (words.first_error != NO_ERROR) {
        const int32_t w = (int32_t)(words.first_error & 0xff);
        const int64_t r = (int64_t)(words.first_error >> 8);
        if (w == FHX_CZ_INTERNAL) return refuse(FHX_ERR_INTERNAL, w, r, "more kept rows than rows at row " + std::to_string(r));
        return refuse(FHX_ERR_UNSUPPORTED, w, r, "row " + std::to_string(r) + (w == FHX_CZ_LOCUS ? " has an end that is no locus of the fragments table" : " has a negative count"));
    }
    const int64_t kept = (int64_t)words.n_records;
    if (kept + (int64_t)words.n_diagonal != n) return refuse(FHX_ERR_INTERNAL, FHX_CZ_INTERNAL, 0, "the kept and the dropped rows do not add up to the rows given");
    cz->n_diagonal = (int64_t)words.n_diagonal;
    if (kept == 0) return FHX_OK;
    // ---- the words are the sort keys ---------------------------------------------------------------------------------------------
    unsigned long long* d_sorted = nullptr;
    unsigned int* d_perm = nullptr;
    TH_HIP(cz, tmp.get_n(&d_sorted, (size_t)kept));
    TH_HIP(cz, tmp.get_n(&d_perm, (size_t)kept));
    {
        const int rc = fhx_sort_u64(cz->sorter, d_keys, kept, d_sorted, d_perm);          // the sorter has a stream of its own; this one is idle
        if (rc != FHX_OK) return fhx::fail(cz, rc, std::string("sort: ") + fhx_last_error(cz->sorter));
    }
    tmp.drop(d_keys);
    clock.mark(2);
    // ---- run heads, and the prefix of the counts at every head ---------------------------------------------------------------------
    const int64_t tiles = (kept + fhxscan::TILE - 1) / fhxscan::TILE;
    unsigned long long *d_tile_sum = nullptr, *d_tile_prefix = nullptr, *d_head_at = nullptr, *d_prefix_at = nullptr;
    int32_t* d_sorted_count = nullptr;
    TH_HIP(cz, tmp.get_n(&d_tile_sum, (size_t)tiles));
    TH_HIP(cz, tmp.get_n(&d_tile_prefix, (size_t)tiles));
    TH_HIP(cz, tmp.get_n(&d_sorted_count, (size_t)kept));
    hipLaunchKernelGGL(cz_tile_sums, dim3((unsigned)tiles), dim3(fhxscan::THREADS), 0, cz->stream, (const unsigned int*)d_perm,
                       (const int32_t*)d_kept_count, kept, d_sorted_count, d_tile_sum);
    hipLaunchKernelGGL(fhxscan::scan_tiles, dim3(1), dim3(fhxscan::THREADS), 0, cz->stream, (const unsigned long long*)d_tile_sum, tiles, d_tile_prefix,
                       &d_words->total);
    fhx::Heads heads;                                                         // its read of the count leaves the stream idle
    if (const int rc = fhx::run_heads(refuse, FHX_CZ_INTERNAL, tmp, d_sorted, kept, &d_words->n_cells, /*positions=*/false, &heads)) return rc;
    const int64_t cells = heads.cells;
    tmp.drop(d_perm);
    tmp.drop(d_kept_count);
    TH_HIP(cz, tmp.get_n(&d_head_at, (size_t)cells));
    TH_HIP(cz, tmp.get_n(&d_prefix_at, (size_t)cells));
    hipLaunchKernelGGL(cz_heads, dim3((unsigned)tiles), dim3(fhxscan::THREADS), 0, cz->stream, (const unsigned long long*)d_sorted,
                       (const int32_t*)d_sorted_count, kept, (const unsigned long long*)heads.d_tile_off, (const unsigned long long*)d_tile_prefix,
                       cells, d_head_at, d_prefix_at);
    TH_HIP(cz, hipGetLastError());
    TH_HIP(cz, hipStreamSynchronize(cz->stream));
    clock.mark(3);
    // ---- cells ---------------------------------------------------------------------------------------------------------------------
    TH_HIP(cz, cz->cols.alloc(cells));
    const fhx::CellColumns& C = cz->cols;
    hipLaunchKernelGGL(cz_cells, dim3((unsigned)((cells + WG - 1) / WG)), dim3(WG), 0, cz->stream, (const unsigned long long*)d_sorted, kept,
                       (const unsigned long long*)d_head_at, (const unsigned long long*)d_prefix_at, cells, (const int32_t*)cz->d_coarse_chr,
                       (const int32_t*)cz->d_coarse_mid, (int32_t)cz->n_coarse, C.col(0), C.col(1), C.col(2), C.col(3), C.col(4), d_words);
    TH_HIP(cz, hipGetLastError());
    TH_HIP(cz, hipMemcpyAsync(&words, d_words, sizeof(words), hipMemcpyDeviceToHost, cz->stream));
    TH_HIP(cz, hipStreamSynchronize(cz->stream));
    if (words.first_big != NO_ERROR) {                                        // the cell goes back in place of a row: g1 << 32 | g2
        const int64_t cell = (int64_t)(words.first_big >> 8);
        unsigned long long at = 0, key = 0;
        TH_HIP(cz, hipMemcpy(&at, d_head_at + cell, sizeof(at), hipMemcpyDeviceToHost));
        TH_HIP(cz, hipMemcpy(&key, d_sorted + std::min<unsigned long long>(at, (unsigned long long)kept - 1), sizeof(key), hipMemcpyDeviceToHost));
        clock.mark(4);
        return refuse(FHX_ERR_UNSUPPORTED, FHX_CZ_SUM, (int64_t)key, "the counts of a cell sum to more than 2^31 - 1 (the largest sum is " +
                      std::to_string(words.max_sum) + "): the count column is int32");
    }
    clock.mark(4);
    *n_cells = cells;
    if (std::getenv("FHX_TIMING"))
        std::fprintf(stderr, "coarsen on the device: %lld rows, %lld dropped as diagonal, %lld cells: upload %.6f s; keys %.6f s; sort %.6f s; "
                     "heads + sums %.6f s; cells %.6f s\n", (long long)n, (long long)cz->n_diagonal, (long long)cells, cz->seconds[0], cz->seconds[1],
                     cz->seconds[2], cz->seconds[3], cz->seconds[4]);
    return FHX_OK;
}

// both entry points: the stream idle, the last cells dropped, the clocks at zero
int begin_call(fhx_cz* cz) {
    TH_HIP(cz, hipSetDevice(cz->device));
    TH_HIP(cz, hipStreamSynchronize(cz->stream));
    drop_cells(cz);
    for (double& s : cz->seconds) s = 0;
    cz->seconds[5] = cz->plan_seconds;
    return FHX_OK;
}

}  // namespace

extern "C" {

int fhx_cz_create(int device, fhx_cz** out) { return fhx::handle_create_with_sorter(device, out); }

void fhx_cz_destroy(fhx_cz* cz) {
    fhx::handle_destroy(cz, [&] {
        drop_cells(cz);
        drop_plan(cz);
        fhx::drop_sorter(cz);
    });
}

const char* fhx_cz_last_error(const fhx_cz* cz) { return fhx::handle_last_error(cz); }

int fhx_cz_reset(fhx_cz* cz) {
    if (!cz) return FHX_ERR_ARG;
    return begin_call(cz);
}

int fhx_cz_load_plan(fhx_cz* cz, const int64_t* first, int32_t n_chr, const int32_t* fine_mid, const int32_t* group_of, int64_t n_fine,
                     const int32_t* coarse_chr, const int32_t* coarse_mid, int64_t n_coarse) {
    if (!cz || !first || !fine_mid || !group_of || !coarse_chr || !coarse_mid || n_chr < 1 || n_fine < 1 || n_coarse < 1) return FHX_ERR_ARG;
    const auto t0 = std::chrono::steady_clock::now();
    if (hipSetDevice(cz->device) == hipSuccess) (void)hipStreamSynchronize(cz->stream);
    drop_cells(cz);
    drop_plan(cz);
    const int rc = load_plan(cz, first, n_chr, fine_mid, group_of, n_fine, coarse_chr, coarse_mid, n_coarse);
    if (rc != FHX_OK) drop_plan(cz);
    cz->plan_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

int fhx_cz_coarsen_device(fhx_cz* cz, const void* d_chr1, const void* d_mid1, const void* d_chr2, const void* d_mid2, const void* d_count, int64_t n,
                          void* stream, int32_t keep_diagonal, int64_t* n_cells, int32_t* why, int64_t* bad_row) {
    if (!cz || !n_cells || !why || !bad_row || n < 0 || (n > 0 && (!d_chr1 || !d_mid1 || !d_chr2 || !d_mid2 || !d_count))) return FHX_ERR_ARG;
    *n_cells = 0;
    *why = FHX_CZ_OK;
    *bad_row = 0;
    if (const int rc = begin_call(cz)) return rc;
    TH_HIP(cz, hipStreamSynchronize((hipStream_t)stream));                    // the producer's kernels have written the rows
    fhx::StageClock clock{cz->seconds};
    fhx::DeviceScratch tmp;
    const int32_t* d[5] = {(const int32_t*)d_chr1, (const int32_t*)d_mid1, (const int32_t*)d_chr2, (const int32_t*)d_mid2, (const int32_t*)d_count};
    const int rc = coarsen_rows(cz, tmp, clock, d, n, keep_diagonal, n_cells, why, bad_row);
    if (rc != FHX_OK) drop_cells(cz);                                         // the one exit of a failed call, whatever failed
    return rc;
}

int fhx_cz_coarsen_host(fhx_cz* cz, const int32_t* chr1, const int32_t* mid1, const int32_t* chr2, const int32_t* mid2, const int32_t* count, int64_t n,
                        int32_t keep_diagonal, int64_t* n_cells, int32_t* why, int64_t* bad_row) {
    if (!cz || !n_cells || !why || !bad_row || n < 0 || (n > 0 && (!chr1 || !mid1 || !chr2 || !mid2 || !count))) return FHX_ERR_ARG;
    *n_cells = 0;
    *why = FHX_CZ_OK;
    *bad_row = 0;
    if (const int rc = begin_call(cz)) return rc;
    fhx::StageClock clock{cz->seconds};
    fhx::DeviceScratch tmp;
    const int32_t* h[5] = {chr1, mid1, chr2, mid2, count};
    int32_t* d[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < 5 && n > 0; ++k) {
        TH_HIP(cz, tmp.get_n(&d[k], (size_t)n));
        TH_HIP(cz, hipMemcpyAsync(d[k], h[k], (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, cz->stream));
    }
    TH_HIP(cz, hipStreamSynchronize(cz->stream));
    clock.mark(0);
    const int rc = coarsen_rows(cz, tmp, clock, d, n, keep_diagonal, n_cells, why, bad_row);
    if (rc != FHX_OK) drop_cells(cz);
    return rc;
}

int fhx_cz_counts(const fhx_cz* cz, int64_t* n_rows, int64_t* n_diagonal, int64_t* n_cells) {
    if (!cz) return FHX_ERR_ARG;
    if (n_rows) *n_rows = cz->n_rows;
    if (n_diagonal) *n_diagonal = cz->n_diagonal;
    if (n_cells) *n_cells = cz->cols.n;
    return FHX_OK;
}

int fhx_cz_stage_seconds(const fhx_cz* cz, double* seconds) {
    if (!cz || !seconds) return FHX_ERR_ARG;
    for (int k = 0; k < FHX_CZ_STAGES; ++k) seconds[k] = cz->seconds[k];
    return FHX_OK;
}

int fhx_cz_fetch_cells(fhx_cz* cz, int32_t* chr1, int32_t* mid1, int32_t* chr2, int32_t* mid2, int32_t* count) {
    return cz ? cz->cols.fetch(cz, {chr1, mid1, chr2, mid2, count}) : FHX_ERR_ARG;
}

void* fhx_cz_device_ptr(fhx_cz* cz, int32_t which) { return cz ? cz->cols.ptr(which) : nullptr; }

void* fhx_cz_stream(fhx_cz* cz) { return cz ? (void*)cz->stream : nullptr; }

}  // extern "C"
