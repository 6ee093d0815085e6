// fhx_scan.hpp - ordered scan helpers shared by the sort-and-segment stages (fhx_kr.hip, fhx_cni.hip, and through fhx_cells.hpp
// fhx_validpairs.hip, fhx_fragpairs.hip and fhx_coarsen.hip), by fhx_digest.hip and by the newline layer of the text paths
// (fhx_textlines.hpp: fhx_ingest.inc, fhx_hicpro.hip, fhx_validpairs.hip, fhx_fragpairs.hip, fhx_juicer.hip, fhx_sigselect.hip):
// run heads of a sorted u64 key array -> per-tile counts -> exclusive tile offsets -> where every run starts, and the block scan
// under all of them.  Tiles of 1024 keys, 256 threads x 4 consecutive keys.  The scans take unsigned int (counts) or
// unsigned long long (fhx_coarsen.hip's sums of counts) values.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace fhxscan {

constexpr int TILE = 1024;
constexpr int THREADS = 256;
constexpr int SCAN_ITEMS = 4;

// ordered block-wide exclusive scan of one value per thread
template <typename V>
static __device__ inline V block_exclusive_scan(V v, V* total) {
    __shared__ V wsum[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    V inc = v;
    for (int s = 1; s < 64; s <<= 1) {
        const V up = __shfl_up(inc, s, 64);
        if (lane >= s) inc += up;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    V base = 0, all = 0;
    for (int k = 0; k < 4; ++k) {
        if (k < w) base += wsum[k];
        all += wsum[k];
    }
    __syncthreads();
    *total = all;
    return base + inc - v;
}

static __device__ inline bool is_head(const unsigned long long* keys, int64_t i) { return i == 0 || keys[i] != keys[i - 1]; }

static __global__ __launch_bounds__(THREADS) void count_heads(const unsigned long long* keys, int64_t N, unsigned int* tile_counts) {
    const int64_t base = (int64_t)blockIdx.x * TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    unsigned int c = 0;
    for (int k = 0; k < SCAN_ITEMS; ++k)
        if (base + k < N && is_head(keys, base + k)) ++c;
    unsigned int total;
    block_exclusive_scan(c, &total);
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = total;
}

// exclusive scan of the tile values (one block, any number of tiles); offsets are 64-bit
template <typename V>
static __global__ __launch_bounds__(THREADS) void scan_tiles(const V* tile_counts, int64_t n_tiles, unsigned long long* tile_offsets,
                                                         unsigned long long* total_out) {
    __shared__ unsigned long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < n_tiles; base += THREADS) {
        const int64_t i = base + threadIdx.x;
        const V v = i < n_tiles ? tile_counts[i] : 0;
        V total;
        const V ex = block_exclusive_scan(v, &total);
        if (i < n_tiles) tile_offsets[i] = carry + ex;
        __syncthreads();
        if (threadIdx.x == 0) carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total_out = carry;
}

// the run heads of the sorted keys, in order: where each run starts (tile_offsets: scan_tiles of count_heads' counts)
static __global__ __launch_bounds__(THREADS) void head_positions(const unsigned long long* __restrict__ keys, int64_t n,
                                                                 const unsigned long long* __restrict__ tile_offsets, int64_t n_cells,
                                                                 unsigned long long* __restrict__ head_at) {
    const int64_t base = (int64_t)blockIdx.x * TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    unsigned int c = 0;
    bool head[SCAN_ITEMS];
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        head[k] = base + k < n && is_head(keys, base + k);
        c += head[k] ? 1u : 0u;
    }
    unsigned int total;
    unsigned long long pos = tile_offsets[blockIdx.x] + block_exclusive_scan(c, &total);
    for (int k = 0; k < SCAN_ITEMS; ++k)
        if (head[k] && (int64_t)pos < n_cells) head_at[pos++] = (unsigned long long)(base + k);
}

}  // namespace fhxscan
