// fhx_cells.hpp - what lies between "kept records" and "five resident int32 columns" in the paths that bin to contact cells:
// fhx_validpairs.hip, fhx_fragpairs.hip and fhx_coarsen.hip (all of it), fhx_hicpro.hip (CellColumns) and fhx_digest.hip (the
// handle with a sorter).  A path keeps its grammar and filters, its key and its decode kernel, its tables and its messages.
//
//   block_append     device: a workgroup's kept records -> consecutive places behind one running counter
//   run_heads        sorted keys -> the number of cells, and where every cell's run starts        (the kernels: fhx_scan.hpp)
//   CellColumns      the five columns of a result in HBM: alloc, drop, fetch, ptr
//   handle_create_with_sorter / drop_sorter    a handle that owns an engine context for fhx_sort_u64
//
// The record array that grows from batch to batch is DeviceScratch::grow_keep, a table upload is upload<T> (fhx_devmem.hpp), a
// refusal is fhx::Refusal (fhx_textupload.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/fithic_mi355x.h"
#include "fhx_textupload.hpp"

namespace fhx {

// ---- device: the compacted append ------------------------------------------------------------------------------------------
constexpr unsigned long long APPEND_OVER = ~0ull;

// Every lane of the workgroup calls it in every round; the lanes with `keep` get consecutive places behind *n_records in lane
// order, at the cost of ONE atomicAdd per round (same-address atomics run at 0.09e9/s: never one per record).  A place at or
// beyond `capacity` comes back as APPEND_OVER: the caller reports its path's INTERNAL word for that record.  The places are
// handed out through one LDS word: a caller that loops has a __syncthreads() between two rounds.
__device__ inline unsigned long long block_append(bool keep, unsigned long long* __restrict__ n_records, unsigned long long capacity) {
    __shared__ unsigned long long out_base;
    unsigned int total;
    const unsigned int at = fhxscan::block_exclusive_scan(keep ? 1u : 0u, &total);
    if (threadIdx.x == 0) out_base = total ? atomicAdd(n_records, (unsigned long long)total) : 0ull;
    __syncthreads();
    const unsigned long long pos = out_base + at;
    return pos < capacity ? pos : APPEND_OVER;
}

// ---- host: sorted keys -> cells ---------------------------------------------------------------------------------------------
struct Heads {
    int64_t tiles = 0, cells = 0;
    unsigned long long* d_tile_off = nullptr;     // [tiles]: the heads in front of every tile
    unsigned long long* d_head_at = nullptr;      // [cells]: where every run starts, when positions were asked for
};

// d_sorted[0, n), n > 0 -> out.  d_n_cells is a device word of the call for scan_tiles' total.  The stream is idle when the
// count is known; head_positions is left in flight.  Heads that do not match the keys refuse the call with the path's
// `internal` reason.
inline int run_heads(const Refusal& refuse, int32_t internal, DeviceScratch& tmp, const unsigned long long* d_sorted, int64_t n,
                     unsigned long long* d_n_cells, bool positions, Heads* out) {
    Handle* h = refuse.h;
    out->tiles = (n + fhxscan::TILE - 1) / fhxscan::TILE;
    const unsigned grid = (unsigned)out->tiles;
    unsigned int* d_tile_cnt = nullptr;
    TH_HIP(h, tmp.get_n(&d_tile_cnt, (size_t)out->tiles));
    TH_HIP(h, tmp.get_n(&out->d_tile_off, (size_t)out->tiles));
    hipLaunchKernelGGL(fhxscan::count_heads, dim3(grid), dim3(fhxscan::THREADS), 0, h->stream, d_sorted, n, d_tile_cnt);
    hipLaunchKernelGGL(fhxscan::scan_tiles, dim3(1), dim3(fhxscan::THREADS), 0, h->stream, (const unsigned int*)d_tile_cnt, out->tiles, out->d_tile_off,
                       d_n_cells);
    TH_HIP(h, hipGetLastError());
    unsigned long long cells = 0;
    TH_HIP(h, hipMemcpyAsync(&cells, d_n_cells, sizeof(cells), hipMemcpyDeviceToHost, h->stream));
    TH_HIP(h, hipStreamSynchronize(h->stream));
    if (cells == 0 || cells > (unsigned long long)n) return refuse(FHX_ERR_INTERNAL, internal, 0, "the run heads do not match the keys");
    out->cells = (int64_t)cells;
    if (!positions) return FHX_OK;
    TH_HIP(h, tmp.get_n(&out->d_head_at, (size_t)cells));
    hipLaunchKernelGGL(fhxscan::head_positions, dim3(grid), dim3(fhxscan::THREADS), 0, h->stream, d_sorted, n,
                       (const unsigned long long*)out->d_tile_off, out->cells, out->d_head_at);
    TH_HIP(h, hipGetLastError());
    return FHX_OK;
}

// ---- host: the five-column result -------------------------------------------------------------------------------------------
struct CellColumns {
    int32_t* d_cols = nullptr;                    // five columns of `stride` elements
    int64_t stride = 0, n = 0;

    // room for n_cells rows; every column starts on a 256-byte boundary, and a result without rows still has a block
    hipError_t alloc(int64_t n_cells) {
        drop();
        const int64_t s = (n_cells + 63) / 64 * 64;
        const hipError_t e = dev_malloc(&d_cols, (size_t)std::max<int64_t>(s, 64) * 5 * sizeof(int32_t));
        if (e == hipSuccess) {
            stride = s;
            n = n_cells;
        }
        return e;
    }
    void drop() {
        dev_free(d_cols);
        stride = n = 0;
    }
    int32_t* col(int k) const { return d_cols + k * stride; }
    void* ptr(int32_t which) const { return (which < 0 || which > 4 || !d_cols) ? nullptr : (void*)col(which); }
    // the n rows to the host, on the handle's stream, which is idle afterwards
    int fetch(Handle* h, int32_t* const (&out)[5]) const {
        for (int k = 0; k < 5; ++k)
            if (n > 0 && !out[k]) return FHX_ERR_ARG;
        TH_HIP(h, hipSetDevice(h->device));
        for (int k = 0; k < 5 && n > 0; ++k) TH_HIP(h, hipMemcpyAsync(out[k], col(k), (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        TH_HIP(h, hipStreamSynchronize(h->stream));
        return FHX_OK;
    }
};

// ---- host: a handle with a sorter ---------------------------------------------------------------------------------------------
// H has `fhx_ctx* sorter`; its destroy calls drop_sorter among what it drops
template <typename H>
int handle_create_with_sorter(int device, H** out) {
    const int rc = handle_create(device, out);
    if (rc == FHX_OK && fhx_create(device, &(*out)->sorter) != FHX_OK) {
        handle_destroy(*out, [] {});              // a new handle owns nothing else yet
        *out = nullptr;
        return FHX_ERR_HIP;
    }
    return rc;
}

template <typename H>
void drop_sorter(H* h) {
    if (h->sorter) fhx_destroy(h->sorter);
    h->sorter = nullptr;
}

}  // namespace fhx
