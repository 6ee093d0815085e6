// fhx_onesweep.inc - K3's sort of large survivor sets (included by fhx_k3.hip, namespace fhx).
//
// What it replaces: eight LSD passes of three launches each - rs_count (reads every key again just to count one digit), rs_scan,
// rs_scatter - over all 62 key bits (profiles/r04_z_od1_kernel_stats.txt: 8 x (35 + 5.5 + 108) us for 1.5e7 keys).
//
//  1. ONE histogram launch (os_hist) reads the keys once and counts the digits of every pass.
//  2. A pass is ONE launch (os_scatter): a workgroup takes a tile of 12 288 keys by ticket, ranks it in LDS exactly as rs_scatter
//     does, publishes its 256 digit counts in a descriptor row and finds the tile's global offsets by decoupled look-back over
//     the descriptors of the tiles before it (one thread per digit; a descriptor word carries its own 2-bit state, so no fence
//     and no L2 write-back is needed: relaxed agent-scope loads and stores).  A tile waits only for tiles with lower tickets -
//     workgroups that are already running and publish their counts before they look back themselves - so the launch cannot stall
//     on a workgroup that has not been dispatched.  A pass whose histogram has one occupied digit only copies.
//  3. Only the TOP bits are radix-sorted: P passes over bits [lo, hi) of an image of the key (os_spread, below), lo = hi - 8 P
//     (5 passes = 40 bits for up to 2.5e8 keys).  p-values are continuous: two keys that agree in 40 leading bits are rare
//     (one inversion per ~1 700 keys at 1.5e7), and keys that agree in ALL bits (the ties of a table-driven run) need no order
//     among themselves.  What is left is repaired from a list of the runs that hold an inversion (os_find_runs .. os_fix_long,
//     further down); runs too long for that are sorted as segments of their own, and when even that is no longer an exception
//     all bits are sorted the plain way (eight one-sweep passes, nothing to repair).  The result is the order a full sort gives
//     up to the order of equal keys, which no consumer can see (ks_tile_sort says why).
//
// Descriptor words hold 30-bit counts: more than 2^30 - 1 keys take the three-launch passes (radix_passes).

constexpr int OS_BITS = 8;
constexpr int OS_RADIX = 1 << OS_BITS;
constexpr int OS_ITEMS = 12;                                // keys per thread
constexpr int OS_HIST_THREADS = 512;
constexpr int OS_THREADS = 1024;
constexpr int OS_WAVES = OS_THREADS / 64;
constexpr int OS_TILE = OS_THREADS * OS_ITEMS;              // 12 288 keys: one workgroup of 16 waves per CU, 147 of its 160 KB of LDS.
// A tile pays one ticket, one look-back and one 1 KB descriptor row whatever it holds: K3 as a fraction of round 4's K3 on the
// same box with 512 threads x 8 keys (two workgroups per CU) 0.89-0.92, 1024 x 8 0.84, 1024 x 12 0.82 (1.5e7 keys; at 3.1e7 keys
// 0.70 and 0.68).
constexpr int OS_MAX_PASSES = 8;
constexpr unsigned int OS_AGG = 1u << 30, OS_PREFIX = 2u << 30, OS_VALUE = (1u << 30) - 1u;
constexpr int64_t OS_MAX_KEYS = (int64_t)OS_VALUE;

// control block (32-bit words) in front of the descriptors
constexpr int OSC_TICKET = 0;                               // OS_MAX_PASSES tile counters
constexpr int OSC_FALLBACK = 8;                             // the repair: bit 0 a run whose ends are out of reach, bit 1 a list overflowed
constexpr int OSC_INVERSIONS = 9;                           // statistics of the last repair (fhx_bh_sort_stats)
constexpr int OSC_SMALL_RUNS = 10;
constexpr int OSC_LONG_RUNS = 11;
constexpr int OSC_COPY_PASSES = 12;
constexpr int OSC_LB_STEPS = 13;                            // (unused: look-back steps were counted here while the scatter was tuned)
constexpr int OSC_SEGMENTS = 14;                            // long runs recorded as segments
constexpr int OSC_HIST = 64;                                // OS_MAX_PASSES x OS_RADIX counts
constexpr int OSC_DESC = OSC_HIST + OS_MAX_PASSES * OS_RADIX;

constexpr int OSC_SEG_N = 16;                               // (8-byte slot) key count of a segment sort

inline size_t os_ctrl_words(int64_t n_keys, int passes) {      // control block + descriptors of `passes` passes
    const size_t tiles = (size_t)((n_keys + OS_TILE - 1) / OS_TILE);
    return (size_t)OSC_DESC + (size_t)passes * tiles * OS_RADIX;
}

// The bits that are radix-sorted are those of a monotone image of the key in which the subnormal patterns (exponent field 0: the
// 52 mantissa bits are the whole value) get exponents of their own, as if the format had 52 more binades below its smallest:
// 0 stays 0, a subnormal m becomes (floor(log2 m) + 1) << 52 | its normalised mantissa, every other pattern moves up by 52
// exponents.  Deep maps underflow: thousands of p are exactly 0 and a few stop just above - in the raw pattern they all share
// their leading 40 bits with 0, one long run with inversions at the very start of the order (the first thing the lognormal
// workload met); in the image a subnormal differs from 0 and from its neighbours in its leading bits like any other value.
// Only digits and run heads are taken from the image; the keys that are moved, compared and handed on are the raw patterns.
__device__ __forceinline__ unsigned long long os_spread(unsigned long long k) {
    if (k >= (1ull << 52)) return k + (52ull << 52);
    if (k == 0ull) return 0ull;
    const int e = 63 - __clzll((long long)k);                 // 0..51
    return ((unsigned long long)(e + 1) << 52) | ((k << (52 - e)) & ((1ull << 52) - 1ull));
}

template <int PASSES>
__global__ __launch_bounds__(OS_HIST_THREADS) void os_hist(const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ n_ptr,
                                                      int lo, unsigned int* __restrict__ hist) {
    __shared__ unsigned int h[PASSES * OS_RADIX];
    for (int i = threadIdx.x; i < PASSES * OS_RADIX; i += OS_HIST_THREADS) h[i] = 0u;
    __syncthreads();
    const int64_t n_all = (int64_t)*n_ptr;
    auto one = [&](unsigned long long k) {
        k = os_spread(k) >> lo;
#pragma unroll
        for (int p = 0; p < PASSES; ++p) atomicAdd(&h[p * OS_RADIX + (int)((k >> (p * OS_BITS)) & (OS_RADIX - 1))], 1u);
    };
    // 16-byte loads: a segment of the array may begin on an odd key
    const int odd = (int)((reinterpret_cast<unsigned long long>(keys) >> 3) & 1ull) && n_all > 0;
    if (odd && blockIdx.x == 0 && threadIdx.x == 0) one(keys[0]);
    const int64_t n = n_all - odd;
    const int64_t n2 = n >> 1;
    const ulonglong2* k2 = reinterpret_cast<const ulonglong2*>(keys + odd);
    for (int64_t i = (int64_t)blockIdx.x * OS_HIST_THREADS + threadIdx.x; i < n2; i += (int64_t)gridDim.x * OS_HIST_THREADS) {
        const ulonglong2 k = k2[i];
        one(k.x);
        one(k.y);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1)) one(keys[n_all - 1]);
    __syncthreads();
    for (int i = threadIdx.x; i < PASSES * OS_RADIX; i += OS_HIST_THREADS)
        if (h[i]) atomicAdd(&hist[i], h[i]);
}

__device__ __forceinline__ unsigned int os_desc_load(const unsigned int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void os_desc_store(unsigned int* p, unsigned int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One workgroup per tile.  (Resident workgroups taking tiles by ticket until none is left, holding the next ticket and the next
// tile's keys while the current tile looks back, were measured slower: a ticket reserved a tile-time ahead makes every later tile
// wait for it.)
constexpr int OS_LOOKBACK = 8;                 // descriptors read per look-back step
__global__ __launch_bounds__(OS_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void os_scatter(
    const unsigned long long* __restrict__ keys_in, const unsigned int* __restrict__ vals_in, unsigned long long* __restrict__ keys_out,
    unsigned int* __restrict__ vals_out, const unsigned long long* __restrict__ n_ptr, int shift, const unsigned int* __restrict__ hist,
    unsigned int* __restrict__ desc, unsigned int* __restrict__ ticket, unsigned int* __restrict__ copy_passes) {
    constexpr int RADIX = OS_RADIX, RADIX_BITS = OS_BITS, TILE = OS_TILE;
    static_assert(OS_WAVES * RADIX * 2 <= TILE * 8, "the per-wave counters fit the block that later stages the keys");
    __shared__ __attribute__((aligned(16))) unsigned char stage_raw[TILE * 8];      // per-wave counters, then the tile's keys
    __shared__ unsigned int s_vals[TILE];
    __shared__ unsigned int tile_start[RADIX];                 // first tile-local slot of each digit
    __shared__ unsigned int global_base[RADIX];                // global offset of the tile's first key of each digit
    __shared__ unsigned int digit_start[RADIX];                // tile 0 only: first global slot of each digit
    __shared__ unsigned int wave_tmp[OS_WAVES];
    __shared__ unsigned int s_tile[2], s_single;
    unsigned short (*wave_digit)[RADIX] = reinterpret_cast<unsigned short (*)[RADIX]>(stage_raw);
    unsigned long long* s_keys = reinterpret_cast<unsigned long long*>(stage_raw);
    const int64_t n = (int64_t)*n_ptr;
    const int64_t tiles = (n + TILE - 1) / TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long lane_lt = (1ull << lane) - 1ull;
    if (threadIdx.x == 0) s_tile[0] = atomicAdd(ticket, 1u);   // tiles in ticket order: every tile before mine is already running
    if (threadIdx.x == 64) s_single = 0u;
    unsigned int digit_count = 0;                              // keys of the whole array with digit threadIdx.x
    if ((int)threadIdx.x < RADIX) digit_count = hist[threadIdx.x];
    __syncthreads();
    int64_t tile_id = (int64_t)s_tile[0];
    if (tile_id >= tiles) return;
    // exclusive scan of RADIX entries of `a` (one per thread of the first four waves); two barriers inside
    auto scan_radix = [&](unsigned int* a) {
        const unsigned int mine = (int)threadIdx.x < RADIX ? a[threadIdx.x] : 0u;
        const unsigned int incl = wave_incl_sum_u32(mine);
        if (lane == 63) wave_tmp[wave] = incl;
        __syncthreads();
        unsigned int excl = incl - mine;
        for (int w = 0; w < wave; ++w) excl += wave_tmp[w];
        if ((int)threadIdx.x < RADIX) a[threadIdx.x] = excl;
        __syncthreads();
    };
    if ((int)threadIdx.x < RADIX && (int64_t)digit_count == n) s_single = 1u;
    __syncthreads();
    if (s_single) {                                            // every key has the same digit here: the pass is a copy
        int slot_i = 0;
        while (tile_id < tiles) {
            if (threadIdx.x == 0) s_tile[slot_i ^ 1] = atomicAdd(ticket, 1u);
            const int64_t beg = tile_id * TILE, end = min(n, beg + (int64_t)TILE);
#pragma unroll
            for (int r = 0; r < OS_ITEMS; ++r) {
                const int64_t i = beg + r * OS_THREADS + threadIdx.x;
                if (i < end) {
                    keys_out[i] = keys_in[i];
                    vals_out[i] = vals_in[i];
                }
            }
            if (tile_id == 0 && threadIdx.x == 0) atomicAdd(copy_passes, 1u);
            __syncthreads();
            slot_i ^= 1;
            tile_id = (int64_t)s_tile[slot_i];
        }
        return;
    }
    // The first global slot of each digit (the exclusive scan of the array's digit counts) enters the chain through tile 0,
    // whose published prefix carries it: no other tile scans the histogram.
    if (tile_id == 0) {
        if ((int)threadIdx.x < RADIX) digit_start[threadIdx.x] = digit_count;
        __syncthreads();
        scan_radix(digit_start);
    }
    const int64_t beg = tile_id * TILE;
    const int64_t end = min(n, beg + (int64_t)TILE);
    const int64_t wave_base = beg + (int64_t)wave * (64 * OS_ITEMS);
    unsigned long long key[OS_ITEMS];
    unsigned int val[OS_ITEMS];
#pragma unroll
    for (int r = 0; r < OS_ITEMS; ++r) {
        const int64_t i = wave_base + r * 64 + lane;
        const bool live = i < n;
        key[r] = live ? keys_in[i] : ~0ull;
        val[r] = live ? vals_in[i] : 0u;
    }
    for (int i = threadIdx.x; i < OS_WAVES * RADIX / 2; i += OS_THREADS) reinterpret_cast<unsigned int*>(stage_raw)[i] = 0u;
    unsigned int slot[OS_ITEMS];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < OS_ITEMS; ++r) {
        const bool live = (wave_base + r * 64 + lane) < end;
        const unsigned int digit = (unsigned int)(os_spread(key[r]) >> shift) & (RADIX - 1);
        unsigned long long same = ~0ull;                   // lanes holding the same digit (dead lanes: a group of their own)
        const unsigned int tag = digit | (live ? 0u : RADIX);
#pragma unroll
        for (int b = 0; b <= RADIX_BITS; ++b) {
            const unsigned long long m = __ballot((tag >> b) & 1u);
            same &= ((tag >> b) & 1u) ? m : ~m;
        }
        const unsigned int before = __popcll(same & lane_lt);
        unsigned int old = 0;
        if (live) old = wave_digit[wave][digit];
        slot[r] = old + before;
        __builtin_amdgcn_wave_barrier();
        if (live && before == 0) wave_digit[wave][digit] = (unsigned short)(old + __popcll(same));
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    unsigned int my_count = 0;
    unsigned int lbv[OS_LOOKBACK];
    if ((int)threadIdx.x < RADIX) {                        // per digit: exclusive offsets over the waves, the tile's total
        const int d = threadIdx.x;
        unsigned int acc = 0;
#pragma unroll
        for (int w = 0; w < OS_WAVES; ++w) {
            const unsigned int c = wave_digit[w][d];
            wave_digit[w][d] = (unsigned short)acc;
            acc += c;
        }
        tile_start[d] = acc;
        my_count = acc;
        // the tile's count goes out at once: the tiles behind this one look back at it while this one is still busy
        os_desc_store(desc + (size_t)tile_id * RADIX + d, tile_id == 0 ? (OS_PREFIX | (digit_start[d] + acc)) : (OS_AGG | acc));
        // ... and the first eight descriptors behind this tile are asked for now; they are looked at after the staging
#pragma unroll
        for (int u = 0; u < OS_LOOKBACK; ++u)
            lbv[u] = (tile_id - 1 - u >= 0) ? os_desc_load(desc + (size_t)(tile_id - 1 - u) * RADIX + d) : OS_PREFIX;
    }
    __syncthreads();
    scan_radix(tile_start);
    const int live_in_tile = (int)(end - beg);
#pragma unroll
    for (int r = 0; r < OS_ITEMS; ++r) {
        const unsigned int digit = (unsigned int)(os_spread(key[r]) >> shift) & (RADIX - 1);
        if (wave_base + r * 64 + lane < end) slot[r] += tile_start[digit] + wave_digit[wave][digit];
    }
    __syncthreads();                                       // the counters are dead: their block now stages the keys
#pragma unroll
    for (int r = 0; r < OS_ITEMS; ++r)
        if (wave_base + r * 64 + lane < end) {
            s_keys[slot[r]] = key[r];
            s_vals[slot[r]] = val[r];
        }
    if ((int)threadIdx.x < RADIX) {                        // decoupled look-back, one digit per thread
        const int d = threadIdx.x;
        unsigned int excl = 0;
        if (tile_id == 0) excl = digit_start[d];
        else {
            // Eight predecessors are read per step (independent loads in flight together) and taken in order up to the first
            // that holds a prefix; one that has not published yet is polled.  At the start of a launch some five hundred tiles
            // begin together and the nearest prefix is hundreds of tiles back.
            int64_t j = tile_id - 1;
            bool done = false, have = true;                // the first step's loads were issued before the staging
            while (!done) {
                if (!have) {
#pragma unroll
                    for (int u = 0; u < OS_LOOKBACK; ++u) lbv[u] = (j - u >= 0) ? os_desc_load(desc + (size_t)(j - u) * RADIX + d) : OS_PREFIX;
                }
                have = false;
#pragma unroll
                for (int u = 0; u < OS_LOOKBACK; ++u) {
                    if (done) break;
                    unsigned int w = lbv[u];
                    while ((w >> 30) == 0u) {
                        __builtin_amdgcn_s_sleep(1);
                        w = os_desc_load(desc + (size_t)(j - u) * RADIX + d);
                    }
                    excl += w & OS_VALUE;
                    done = (w >> 30) == 2u;
                }
                j -= OS_LOOKBACK;
            }
            os_desc_store(desc + (size_t)tile_id * RADIX + d, OS_PREFIX | (excl + my_count));
        }
        global_base[d] = excl;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < OS_ITEMS; ++j) {
        const int s = threadIdx.x + j * OS_THREADS;
        if (s < live_in_tile) {
            const unsigned long long k = s_keys[s];
            const unsigned int digit = (unsigned int)(os_spread(k) >> shift) & (RADIX - 1);
            const unsigned int dst = global_base[digit] + (s - tile_start[digit]);
            keys_out[dst] = k;
            vals_out[dst] = s_vals[s];
        }
    }
}

// ---- repair of the low bits ---------------------------------------------------------------------------------------------------
// After the passes the keys are in order by the bits from `lo` up (of their image, os_spread); a RUN is a stretch of keys that
// agree in those bits.  Inversions - a key smaller than the key before it, inside a run - are rare on a real p column (one per
// ~1 700 keys at 1.5e7 keys and 40 sorted bits) and the runs that hold them are short (two keys, nearly always).  Four launches:
//   os_find_runs   streams the keys once (16-byte loads, nothing else) and, for every inversion, walks to the head and to the end
//                  of its run - a few keys - to see whether it is the run's FIRST inversion; if so the run goes on a list: up to
//                  RP_SMALL keys as (start, length), longer ones (the walk gives up after RP_SMALL steps) as the position of the
//                  inversion.  Read-only: who owns a run is settled before anything moves.
//   os_tally       adds the workgroups' counts up for the verdict.
//   os_fix_runs    one thread per listed run: insertion sort of keys and payloads in place.
//   os_long_runs   one workgroup per listed long inversion: scans back to the run's head (is an inversion in between? then
//                  another entry owns the run) and forward to its end, and records (start, end) as a segment.  Read-only.
//   os_fix_long    one workgroup per segment of up to 4096 keys: ranks by counting in LDS.  Longer segments are the host's, which
//                  sees them in the verdict it reads anyway: sorted on their own by the bits below `lo` (tile sorts in LDS, or
//                  one-sweep passes over the segment).
// (The first version held windows of 8192 sorted keys in LDS, masks of heads and inversions, per-window records stitched by the
// host for runs that crossed windows: 106-174 us per launch for 1.5e7 keys, whatever the window - most of a window's time went
// into what follows the first inversion it met, and 85 % of the windows met one.)
constexpr int RP_SMALL = 32;                                    // runs up to this length are sorted by one thread
constexpr int RP_LONG_CAP = 4096;                               // inversions in long runs the list holds
constexpr int RP_SEG_CAP = 64;                                  // segments handed to the host
constexpr int64_t RP_SCAN_CAP = 1ll << 22;                      // how far os_long_runs looks for a run's head / end

constexpr int RP_FIND_WGS = 1024;                               // workgroups of os_find_runs (== RP_FIND_GRID below)
inline size_t os_region_cap(int64_t n) { return (size_t)(n / 4 / RP_FIND_WGS + 64); }       // runs one workgroup can list
// scratch behind the descriptors: run regions (uint2 each) | per-workgroup counts (4 words each) | long list | segments (2 x i64 each)
inline size_t os_repair_words(int64_t n) { return os_region_cap(n) * RP_FIND_WGS * 2 + RP_FIND_WGS * 4 + RP_LONG_CAP + RP_SEG_CAP * 4 + 8; }

// Every workgroup of os_find_runs lists its runs in a region of its own and leaves its three counts in a slot of its own: ten
// thousand additions to ONE counter are ten thousand serialised round trips (11 ns each on this part: the first version of this
// kernel spent 160 of its 190 us in them).  os_tally adds the slots up for the verdict.
constexpr int RP_FIND_GRID = 1024;
struct OsFindCounts {
    unsigned int inversions, runs, pad0, pad1;
};

__global__ __launch_bounds__(256) void os_find_runs(const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ n_ptr, int lo,
                                                    unsigned int* __restrict__ ctrl, uint2* __restrict__ runs, unsigned int region_cap,
                                                    OsFindCounts* __restrict__ counts, unsigned int* __restrict__ longs) {
    __shared__ unsigned int s_runs, s_inv;
    if (threadIdx.x == 0) s_runs = s_inv = 0u;
    __syncthreads();
    uint2* my_runs = runs + (size_t)blockIdx.x * region_cap;
    const int64_t n = (int64_t)*n_ptr;
    const int64_t pairs = (n + 1) >> 1;
    const ulonglong2* k2 = reinterpret_cast<const ulonglong2*>(keys);
    const int lane = threadIdx.x & 63;
    unsigned int n_inv = 0;
    for (int64_t j0 = ((int64_t)blockIdx.x * 256 + (threadIdx.x & ~63)); j0 < pairs; j0 += (int64_t)gridDim.x * 256) {
        const int64_t j = j0 + lane;                            // this lane's pair: keys 2j, 2j + 1
        unsigned long long k0 = 0, k1 = 0;
        bool has0 = false, has1 = false;
        if (2 * j + 1 < n) {
            const ulonglong2 k = k2[j];
            k0 = k.x;
            k1 = k.y;
            has0 = has1 = true;
        } else if (2 * j < n) {
            k0 = keys[2 * j];
            has0 = true;
        }
        unsigned long long prev = __shfl_up(k1, 1, 64);         // the key in front of this pair: the lane before holds it ...
        if (lane == 0) prev = (j > 0 && has0) ? keys[2 * j - 1] : 0ull;      // ... or the wave before
        const unsigned long long t0 = os_spread(k0) >> lo, t1 = os_spread(k1) >> lo, tp = os_spread(prev) >> lo;
        const bool inv0 = has0 && j > 0 && tp == t0 && k0 < prev;
        const bool inv1 = has1 && t0 == t1 && k1 < k0;
        if (!inv0 && !inv1) continue;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (!(h ? inv1 : inv0)) continue;
            ++n_inv;
            const int64_t x = 2 * j + h;                        // an inversion: is it the first of its run, and where does the run end?
            const unsigned long long top = h ? t1 : t0;
            int64_t s = x - 1;                                  // key s is in the run (same top as key x)
            bool first = true, is_long = false;
            for (int step = 0;; ++step) {
                if (s == 0) break;
                const unsigned long long ks = keys[s], kb = keys[s - 1];
                if ((os_spread(kb) >> lo) != top) break;        // s is the head
                if (ks < kb) {                                   // an inversion at s: the run is that entry's
                    first = false;
                    break;
                }
                if (step == RP_SMALL) {
                    is_long = true;
                    break;
                }
                --s;
            }
            if (!first) continue;
            int64_t e = x + 1;
            if (!is_long)
                while (e < n && (os_spread(keys[e]) >> lo) == top) {
                    if (e - s >= RP_SMALL) {
                        is_long = true;
                        break;
                    }
                    ++e;
                }
            if (is_long) {                                      // (rare: one shared list)
                const unsigned int k = atomicAdd(&ctrl[OSC_LONG_RUNS], 1u);
                if (k < (unsigned int)RP_LONG_CAP) longs[k] = (unsigned int)x;
                else atomicOr(&ctrl[OSC_FALLBACK], 2u);
            } else {
                const unsigned int k = atomicAdd(&s_runs, 1u);
                if (k < region_cap) my_runs[k] = make_uint2((unsigned int)s, (unsigned int)(e - s));
                else atomicOr(&ctrl[OSC_FALLBACK], 2u);
            }
        }
    }
    n_inv = (unsigned int)wave_sum_i64((long long)n_inv);
    if (lane == 0 && n_inv) atomicAdd(&s_inv, n_inv);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = OsFindCounts{s_inv, min(s_runs, region_cap), 0u, 0u};
}

__global__ __launch_bounds__(RP_FIND_GRID) void os_tally(const OsFindCounts* __restrict__ counts, unsigned int* __restrict__ ctrl) {
    __shared__ unsigned int a, b;
    if (threadIdx.x == 0) a = b = 0u;
    __syncthreads();
    const OsFindCounts c = counts[threadIdx.x];
    if (c.inversions) atomicAdd(&a, c.inversions);
    if (c.runs) atomicAdd(&b, c.runs);
    __syncthreads();
    if (threadIdx.x == 0) {
        ctrl[OSC_INVERSIONS] = a;
        ctrl[OSC_SMALL_RUNS] = b;
    }
}

// one workgroup per region of os_find_runs
__global__ __launch_bounds__(256) void os_fix_runs(unsigned long long* __restrict__ keys, unsigned int* __restrict__ vals,
                                                   const uint2* __restrict__ runs, unsigned int region_cap, const OsFindCounts* __restrict__ counts) {
    const unsigned int n_runs = counts[blockIdx.x].runs;
    const uint2* my_runs = runs + (size_t)blockIdx.x * region_cap;
    for (unsigned int r = threadIdx.x; r < n_runs; r += 256) {
        const int64_t s = my_runs[r].x;
        const int L = (int)my_runs[r].y;
        unsigned long long* k = keys + s;
        unsigned int* v = vals + s;
        for (int i = 1; i < L; ++i) {                           // insertion sort in place: the run is this thread's alone
            const unsigned long long kx = k[i];
            const unsigned int vx = v[i];
            int y = i - 1;
            while (y >= 0 && k[y] > kx) {
                k[y + 1] = k[y];
                v[y + 1] = v[y];
                --y;
            }
            k[y + 1] = kx;
            v[y + 1] = vx;
        }
    }
}

// One workgroup per listed inversion x of a long run: the run's head s (the last position <= x whose key differs from the key
// before it in the sorted bits) and its end e.  Several inversions of one run may be listed; only the entry with no inversion
// between the head and x - the run's first - records the segment.  Read-only.
__global__ __launch_bounds__(512) void os_long_runs(const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ n_ptr, int lo,
                                                    unsigned int* __restrict__ ctrl, const unsigned int* __restrict__ longs,
                                                    long long* __restrict__ segs) {
    __shared__ long long s_head, s_inv, s_end;
    const int64_t n = (int64_t)*n_ptr;
    const unsigned int n_long = min(ctrl[OSC_LONG_RUNS], (unsigned int)RP_LONG_CAP);
    for (unsigned int q = blockIdx.x; q < n_long; q += gridDim.x) {
        const int64_t x = longs[q];
        const unsigned long long top = os_spread(keys[x]) >> lo;
        if (threadIdx.x == 0) {
            s_head = -1;
            s_inv = -1;
            s_end = -1;
        }
        __syncthreads();
        // backwards from x - 1: the nearest head, and whether an inversion lies between it and x
        int64_t s = -1;
        bool owner = true, give_up = false;
        for (int64_t base = x - 1; base >= 0; base -= 512) {
            const int64_t p = base - threadIdx.x;
            if (p >= 0) {
                const unsigned long long kp = keys[p];
                const bool head = p == 0 || (os_spread(keys[p - 1]) >> lo) != top;
                if (head) atomicMax(&s_head, (long long)p);
                else if (kp < keys[p - 1]) atomicMax(&s_inv, (long long)p);
            }
            __syncthreads();
            const long long h = s_head, iv = s_inv;
            __syncthreads();
            if (iv > h) {                                       // an inversion nearer to x than any head found: not the first
                owner = false;
                break;
            }
            if (h >= 0) {
                s = h;
                break;
            }
            if (x - base > RP_SCAN_CAP) {
                give_up = true;
                break;
            }
        }
        if (!owner) continue;
        if (!give_up) {
            for (int64_t base = x + 1;; base += 512) {          // forwards: the first key of the next run
                const int64_t p = base + threadIdx.x;
                if (p < n && (os_spread(keys[p]) >> lo) != top) atomicMin(reinterpret_cast<unsigned long long*>(&s_end), (unsigned long long)p);
                __syncthreads();
                const long long e = s_end;
                __syncthreads();
                if (e >= 0) break;
                if (base + 512 >= n) {
                    if (threadIdx.x == 0) s_end = n;
                    __syncthreads();
                    break;
                }
                if (base - x > RP_SCAN_CAP) {
                    give_up = true;
                    break;
                }
            }
        }
        if (threadIdx.x == 0) {
            if (give_up) atomicOr(&ctrl[OSC_FALLBACK], 1u);
            else {
                const unsigned int k = atomicAdd(&ctrl[OSC_SEGMENTS], 1u);
                if (k < (unsigned int)RP_SEG_CAP) {
                    segs[2 * k] = s;
                    segs[2 * k + 1] = s_end;
                } else atomicOr(&ctrl[OSC_FALLBACK], 2u);
            }
        }
        __syncthreads();
    }
}

// the recorded segments of up to RP_WG_RUN keys, one workgroup each: ranks by counting over the run in LDS (what is longer is the
// host's: tile sorts or one-sweep passes over the segment)
constexpr int RP_WG_RUN = 4096;
__global__ __launch_bounds__(512) void os_fix_long(unsigned long long* __restrict__ keys, unsigned int* __restrict__ vals,
                                                   const unsigned int* __restrict__ ctrl, const long long* __restrict__ segs) {
    __shared__ unsigned long long sk[RP_WG_RUN];
    constexpr int PER = RP_WG_RUN / 512;
    const unsigned int n_segs = min(ctrl[OSC_SEGMENTS], (unsigned int)RP_SEG_CAP);
    for (unsigned int q = blockIdx.x; q < n_segs; q += gridDim.x) {
        const int64_t s = segs[2 * q];
        const int L = (int)min<long long>(segs[2 * q + 1] - s, RP_WG_RUN + 1);
        if (L > RP_WG_RUN) continue;
        for (int i = threadIdx.x; i < L; i += 512) sk[i] = keys[s + i];
        __syncthreads();
        unsigned long long kx[PER];
        unsigned int vx[PER];
        int rank[PER];
#pragma unroll
        for (int t = 0; t < PER; ++t) {
            const int i = threadIdx.x + t * 512;
            rank[t] = -1;
            if (i < L) {
                kx[t] = sk[i];
                vx[t] = vals[s + i];
                int r = 0;
                for (int y = 0; y < L; ++y) {
                    const unsigned long long ky = sk[y];
                    r += (ky < kx[t] || (ky == kx[t] && y < i)) ? 1 : 0;
                }
                rank[t] = r;
            }
        }
        __syncthreads();                                        // every payload of the run is in a register before one is overwritten
#pragma unroll
        for (int t = 0; t < PER; ++t)
            if (rank[t] >= 0) {
                keys[s + rank[t]] = kx[t];
                vals[s + rank[t]] = vx[t];
            }
        __syncthreads();
    }
}

__global__ void os_set_n(unsigned long long* slot, unsigned long long v) { *slot = v; }
