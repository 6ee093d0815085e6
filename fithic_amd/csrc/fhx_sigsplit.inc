// fhx_sigsplit.inc - the per-chromosome FDR subsets of a significances file on MI355X (gfx950); included by fhx_sigselect.hip
// (reference: fithic/utils/merge-filter-parallelized.sh:21-25, `cut -f1 | sort | uniq` over every line, then once per listed name c
// `awk '{if(NR!=1){print $0}}' | awk -v c=C '{if($1==c && $3==c){print $0}}' | awk -v q=Q '{if($7<=q){print $0}}'`).
//
// ONE read of the file yields every subset.  Per batch, behind scan_text / scan_tiles of the selection:
//
//   mp_names       token 1 of EVERY line (file line 1 too: cut lists it) is interned: its 64-bit FNV-1a hash claims one of 4096
//                  slots by ONE compare-and-swap - nothing is published behind the hash, so no lane ever waits for another - and
//                  an atomicMin keeps the smallest file offset the name was seen at.  A wave posts each DISTINCT name once (its
//                  lanes vote, fhx_ingest.inc's scheme), and the atomics are issued only when a plain load does not already show
//                  the hash with an earlier offset: a sorted file touches the table a few times per wave.  Per line: its slot
//                  (16 bits); per slot: a flag when it was claimed in this batch.
//   mp_copy_names  the text of every newly claimed name, from the offset the table holds, into 64 bytes per slot (byte 63: the
//                  length).  The array outlives the batch; the host reads it once, at the end.
//   mp_select      one line per lane: ms_select's walk and decision (walk of fhx_sigline.hpp, classify and decide of fhx_sigkey.hpp), the name
//                  grammar on tokens 1 and 3, token 3 against token 1 byte by byte (a trans row goes nowhere), and token 1 against
//                  the STORED name of its slot byte by byte - a hash collision is FHX_MS_INTERNAL, never a wrong subset.  Per
//                  line: its kept length; per block: kept lines.
//   scan_tiles     kept lines per block -> the block's first record
//   mp_emit        one 64-bit record per kept line, in file order: slot << 44 | line start in the batch << 13 | kept length
//   fhx_sort_u64   the stable radix sort: by slot, then by offset = file order within a chromosome
//   mp_tile_bytes  bytes of every 256 sorted records; scan_tiles -> where each such round writes
//   mp_gather      256 sorted records per workgroup, their lengths scanned into LDS, lanes assigned by OUTPUT byte (gather_round,
//                  shared with ms_gather); the record that begins a slot's run notes the byte offset and the record index of the run
//
// so the bytes of one chromosome leave the device contiguous and in file order, and the host makes one copy per (batch,
// chromosome) without looking inside a line.  Atomics: none per good line (mp_names' CAS and atomicMin come once per distinct name
// of a wave, and only while the table does not hold the name yet); one atomicMin (line << 8 | reason) per refused line.
namespace mpd {

using namespace fhxlines;
using namespace msd;                      // the line and the decision: fhx_sigline.hpp, fhx_sigkey.hpp
using fhx::namerule::name_grammar;        // what a name may be: fhx_namerule.hpp, shared with the resident route

constexpr int SLOTS = FHX_MS_SPLIT_NAMES;      // 4096 = 2^12: the slot field of a record
constexpr int NAME_STRIDE = fhx::namerule::NAME_STRIDE;      // a name of up to 63 bytes, and its length in byte 63
constexpr unsigned int NO_SLOT = 0xFFFFu;
constexpr int LEN_BITS = 13, START_BITS = 31;  // 4097 < 2^13; a batch has at most 2^31 bytes
constexpr int ROUND = 256;                     // sorted records per workgroup of mp_gather

struct SplitWords {
    unsigned long long first_error;            // smallest (line << 8 | reason)
    unsigned long long kept_lines;             // scan_tiles' totals of the current batch
    unsigned long long out_bytes;
    unsigned long long overflow;               // not 0: a name found no slot (never cleared within a call)
};

__device__ inline bool name_end(int c) { return c == '\t' || c == ' ' || c == '\n'; }

// the table: hash[slot] (0 = empty), off[slot] = the smallest file offset the name was seen at.  -1: no slot is left.
__device__ inline int table_insert(unsigned long long* __restrict__ t_hash, unsigned long long* __restrict__ t_off,
                                   unsigned int* __restrict__ claimed, unsigned long long h, unsigned long long off) {
    unsigned int s = (unsigned int)((h * 0x9e3779b97f4a7c15ull) >> 52) & (SLOTS - 1);
    for (int probes = 0; probes < SLOTS; ++probes) {
        unsigned long long cur = __hip_atomic_load(&t_hash[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            cur = atomicCAS(&t_hash[s], 0ull, h);
            if (cur == 0) {
                cur = h;
                claimed[s] = 1u;                                              // every writer writes the same value
            }
        }
        if (cur == h) {
            if (__hip_atomic_load(&t_off[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > off) atomicMin(&t_off[s], off);
            return (int)s;
        }
        s = (s + 1) & (SLOTS - 1);
    }
    return -1;
}

// ---- token 1 of every line -> its slot ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void mp_names(const unsigned char* __restrict__ text, int64_t T, const unsigned long long* __restrict__ block_off,
                                               int64_t n_lines_batch, int64_t file_off, unsigned short* __restrict__ line_slot,
                                               unsigned long long* __restrict__ t_hash, unsigned long long* __restrict__ t_off,
                                               unsigned int* __restrict__ claimed, SplitWords* __restrict__ words) {
    __shared__ unsigned short lstart[LSTART_ENTRIES];
    const BlockLines B = block_lines(text, T, block_off, lstart);
    const int lane = threadIdx.x & 63;
    for (int base = 0; base < B.n_lines; base += WG) {      // n_lines is the same for every lane: whole waves reach the votes
        const Round q = round_of(base, B.n_lines, B.row0, n_lines_batch);
        unsigned long long h = 0xcbf29ce484222325ull;       // FNV-1a; equal names are confirmed by mp_select
        int64_t start = 0;
        int n = 0;
        if (q.valid) {
            start = B.b0 + lstart[q.e];
            for (; n < NAME_STRIDE; ++n) {
                const int64_t p = start + n;
                const int c = p < T ? (int)text[p] : '\n';
                if (name_end(c)) break;
                h = (h ^ (unsigned long long)c) * 0x100000001b3ull;
            }
        }
        if (h == 0) h = 1;                                  // 0 marks an empty slot
        bool have = q.valid && n >= 1 && n < NAME_STRIDE;   // anything else is mp_select's to refuse
        int slot = -1;
        for (;;) {                                          // one distinct name of the wave at a time, posted by its lowest lane
            const unsigned long long todo = __ballot(have);
            if (!todo) break;
            const int leader = __ffsll((long long)todo) - 1;
            const unsigned long long lh = __shfl(h, leader, 64);
            int s = 0;
            if (lane == leader) s = table_insert(t_hash, t_off, claimed, h, (unsigned long long)(file_off + start));
            s = __shfl(s, leader, 64);
            if (have && h == lh) {
                slot = s;
                have = false;
            }
        }
        if (q.valid) {
            line_slot[q.r] = slot >= 0 ? (unsigned short)slot : (unsigned short)NO_SLOT;
            if (slot < 0 && n >= 1 && n < NAME_STRIDE) words->overflow = 1ull;            // every writer writes the same value
        }
    }
}

// ---- the text of the names claimed in this batch ------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void mp_copy_names(const unsigned char* __restrict__ text, int64_t T, int64_t file_off,
                                                    const unsigned long long* __restrict__ t_off, unsigned int* __restrict__ claimed,
                                                    unsigned char* __restrict__ names) {
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= SLOTS || !claimed[s]) return;
    claimed[s] = 0u;
    const int64_t p = (int64_t)t_off[s] - file_off;
    int n = 0;
    if (p >= 0)
        for (; n < NAME_STRIDE - 1 && p + n < T; ++n) {
            const int c = text[p + n];
            if (name_end(c)) break;
            names[(size_t)s * NAME_STRIDE + n] = (unsigned char)c;
        }
    names[(size_t)s * NAME_STRIDE + NAME_STRIDE - 1] = (unsigned char)n;
}

// ---- keep or drop every line, and say whose it is -----------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void mp_select(const unsigned char* __restrict__ text, int64_t T, const unsigned long long* __restrict__ block_off,
                                                int64_t n_lines_batch, int64_t line_base, Fdr fdr, unsigned long long key_bound, int zero_kept,
                                                int check_bytes, const unsigned short* __restrict__ line_slot,
                                                const unsigned char* __restrict__ names, unsigned short* __restrict__ keep_len,
                                                unsigned int* __restrict__ block_kept, SplitWords* __restrict__ words) {
    __shared__ unsigned short lstart[LSTART_ENTRIES];
    const BlockLines B = block_lines(text, T, block_off, lstart);
    unsigned int my_kept = 0;
    for (int e = threadIdx.x; e < B.n_lines; e += WG) {
        const int64_t r = B.row0 + e;
        const int64_t start = B.b0 + lstart[e];
        const unsigned char* line = text + start;
        const bool header = line_base + r == 0;                               // dropped whatever it holds; cut still lists its field 1
        Line L;
        walk(text, T, start, check_bytes, L);
        int why = L.why;
        bool keep = false;
        if (!why && r >= n_lines_batch) why = FHX_MS_INTERNAL;                // the scan and this kernel disagree about the lines
        if (!why && !header && L.tok < 7) why = FHX_MS_TOKENS;
        if (!why && (L.n1 == 0 || L.b1 != 0 || start + L.n1 >= T || line[L.n1] != '\t')) why = FHX_MS_NAME_TAB;
        if (!why) why = name_grammar(line, L.n1);
        if (!why && !header) why = name_grammar(line + L.b3, L.n3);
        if (!why && !header) {
            unsigned long long key = 0;
            const int cls = classify(text, start + L.fb, L.fn, &key);
            why = decide(cls, key, key_bound, zero_kept, /*strict=*/0, text, start + L.fb, L.fn, fdr, &keep);
            if (keep) {                                                      // $1 == c && $3 == c for some c: $3 is $1, byte for byte
                keep = L.n3 == L.n1;
                for (int k = 0; keep && k < L.n1; ++k) keep = line[L.b3 + k] == line[k];
            }
        }
        unsigned int slot = NO_SLOT;
        if (!why) {                                                           // the slot holds THIS name, or nothing of the call is kept
            slot = line_slot[r];
            if (slot < (unsigned int)SLOTS) {
                const unsigned char* want = names + (size_t)slot * NAME_STRIDE;
                bool same = (int)want[NAME_STRIDE - 1] == L.n1;
                for (int k = 0; same && k < L.n1; ++k) same = want[k] == line[k];
                if (!same) why = FHX_MS_INTERNAL;
            } else if (__hip_atomic_load(&words->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0ull) {
                why = FHX_MS_INTERNAL;                                        // no slot although the table had room
            } else {
                keep = false;                                                 // the call ends with FHX_MS_NAMES
            }
        }
        if (why) atomicMin(&words->first_error, error_word(line_base + r + 1, why));
        const unsigned int len = (keep && !why) ? (unsigned int)L.len + 1u : 0u;          // with its newline, present or not
        if (r < n_lines_batch) keep_len[r] = (unsigned short)len;             // at most MAX_LINE + 1
        my_kept += len ? 1u : 0u;
    }
    unsigned int total;
    fhxscan::block_exclusive_scan(my_kept, &total);                           // every lane of the block arrives here
    if (threadIdx.x == 0) block_kept[blockIdx.x] = total;
}

// ---- one record per kept line, in file order ----------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void mp_emit(const unsigned char* __restrict__ text, int64_t T, const unsigned long long* __restrict__ block_off,
                                              int64_t n_lines_batch, const unsigned short* __restrict__ line_slot,
                                              const unsigned short* __restrict__ keep_len, const unsigned long long* __restrict__ rec_off,
                                              unsigned long long* __restrict__ records, int64_t n_records) {
    __shared__ unsigned short lstart[LSTART_ENTRIES];
    const BlockLines B = block_lines(text, T, block_off, lstart);
    int64_t at = (int64_t)rec_off[blockIdx.x];
    for (int base = 0; base < B.n_lines; base += WG) {
        const Round q = round_of(base, B.n_lines, B.row0, n_lines_batch);
        const unsigned int len = q.valid ? (unsigned int)keep_len[q.r] : 0u;
        unsigned int total;
        const int64_t i = at + fhxscan::block_exclusive_scan(len ? 1u : 0u, &total);
        if (len && i < n_records)
            records[i] = ((unsigned long long)line_slot[q.r] << (START_BITS + LEN_BITS)) |
                         ((unsigned long long)(B.b0 + lstart[q.e]) << LEN_BITS) | (unsigned long long)len;
        at += total;
    }
}

// ---- bytes of every round of sorted records -----------------------------------------------------------------------------------
__global__ __launch_bounds__(ROUND) void mp_tile_bytes(const unsigned long long* __restrict__ sorted, int64_t n_records,
                                                       unsigned int* __restrict__ tile_bytes) {
    const int64_t i = (int64_t)blockIdx.x * ROUND + threadIdx.x;
    const unsigned int len = i < n_records ? (unsigned int)(sorted[i] & ((1ull << LEN_BITS) - 1)) : 0u;
    unsigned int total;
    fhxscan::block_exclusive_scan(len, &total);
    if (threadIdx.x == 0) tile_bytes[blockIdx.x] = total;
}

// ---- the kept lines, chromosome by chromosome, each in file order -----------------------------------------------------------
__global__ __launch_bounds__(ROUND) void mp_gather(const unsigned char* __restrict__ text, int64_t T, const unsigned long long* __restrict__ sorted,
                                                   int64_t n_records, const unsigned long long* __restrict__ tile_off,
                                                   unsigned char* __restrict__ out, int64_t out_capacity,
                                                   unsigned long long* __restrict__ slot_byte, unsigned int* __restrict__ slot_record) {
    __shared__ unsigned int pre[ROUND + 1];                 // exclusive prefix of the lengths; pre[ROUND] = their sum
    __shared__ unsigned int starts[ROUND];
    const int64_t i = (int64_t)blockIdx.x * ROUND + threadIdx.x;
    const unsigned long long rec = i < n_records ? sorted[i] : 0ull;
    const unsigned int len = (unsigned int)(rec & ((1ull << LEN_BITS) - 1));
    const int64_t at = (int64_t)tile_off[blockIdx.x];
    unsigned int total;
    const unsigned int mine = fhxscan::block_exclusive_scan(len, &total);
    pre[threadIdx.x] = mine;
    starts[threadIdx.x] = (unsigned int)((rec >> LEN_BITS) & ((1ull << START_BITS) - 1));
    if (threadIdx.x == 0) pre[ROUND] = total;
    if (i < n_records) {                                    // the head of a slot's run says where the run begins
        const unsigned int slot = (unsigned int)(rec >> (START_BITS + LEN_BITS));
        const bool head = i == 0 || (unsigned int)(sorted[i - 1] >> (START_BITS + LEN_BITS)) != slot;
        if (head && slot < (unsigned int)SLOTS) {
            slot_byte[slot] = (unsigned long long)(at + mine);
            slot_record[slot] = (unsigned int)i;
        }
    }
    __syncthreads();                                        // the absent records of the last round share the sum as their prefix
    gather_round<ROUND>(text, T, pre, total, [&](int t) { return (int64_t)starts[t]; }, at, out, out_capacity);
}

}  // namespace mpd

// ===================================================================================================================
namespace {

void drop_split(fhx_ms* ms) {
    std::vector<fhx_ms::SplitName>().swap(ms->split);
    ms->s_lines = 0;
}

// fhx_ms_split_file behind its argument check; whatever it returns but FHX_OK, the caller drops the split
int split_file(fhx_ms* ms, const char* path, const char* fdr_text, int32_t fdr_len, uint64_t key_bound, int32_t zero_kept, int32_t* n_names,
               int32_t* why, int64_t* bad_line) {
    using namespace mpd;
    TH_HIP(ms, hipSetDevice(ms->device));
    TH_HIP(ms, hipStreamSynchronize(ms->stream));
    drop_split(ms);
    for (double& s : ms->s_seconds) s = 0;
    Fdr fdr;
    if (const int rc = make_fdr(ms, fdr_text, fdr_len, "fdr", &fdr, why)) return rc;
    if (!ms->sorter && fhx_create(ms->device, &ms->sorter) != FHX_OK) {       // only a split pays for it
        ms->sorter = nullptr;
        return fhx::fail(ms, FHX_ERR_HIP, "the sort context could not be made");
    }
    fhx::StageClock clock{ms->s_seconds};
    fhx::DeviceScratch tmp;
    fhx::TextBatches in;
    if (const int rc = in.open(ms, &tmp, &clock, path, "significances", "FHX_MS_BATCH_BYTES", (int64_t)1 << 31)) return rc;
    const int64_t out_capacity = in.batch_bytes + 1;                          // every line kept, and the newline the last one lacked
    unsigned char *d_out = nullptr, *d_names = nullptr;
    unsigned int *d_block_kept = nullptr, *d_claimed = nullptr, *d_tile_bytes = nullptr, *d_perm = nullptr, *d_slot_record = nullptr;
    unsigned long long *d_rec_off = nullptr, *d_hash = nullptr, *d_off = nullptr, *d_records = nullptr, *d_sorted = nullptr, *d_tile_off = nullptr,
                       *d_slot_byte = nullptr;
    unsigned short *d_keep_len = nullptr, *d_line_slot = nullptr;
    int64_t keep_capacity = 0, slot_capacity = 0, rec_capacity = 0, sorted_capacity = 0, perm_capacity = 0, tile_capacity = 0,
            tile_off_capacity = 0;
    SplitWords* d_words = nullptr;
    TH_HIP(ms, tmp.get_n(&d_out, (size_t)out_capacity));
    TH_HIP(ms, tmp.get_n(&d_block_kept, (size_t)in.max_blocks));
    TH_HIP(ms, tmp.get_n(&d_rec_off, (size_t)in.max_blocks));
    TH_HIP(ms, tmp.get_n(&d_hash, (size_t)SLOTS));
    TH_HIP(ms, tmp.get_n(&d_off, (size_t)SLOTS));
    TH_HIP(ms, tmp.get_n(&d_claimed, (size_t)SLOTS));
    TH_HIP(ms, tmp.get_n(&d_names, (size_t)SLOTS * NAME_STRIDE));
    TH_HIP(ms, tmp.get_n(&d_slot_byte, (size_t)SLOTS));
    TH_HIP(ms, tmp.get_n(&d_slot_record, (size_t)SLOTS));
    TH_HIP(ms, tmp.get_n(&d_words, 1));
    TH_HIP(ms, hipMemsetAsync(d_hash, 0, sizeof(unsigned long long) * SLOTS, ms->stream));
    TH_HIP(ms, hipMemsetAsync(d_off, 0xFF, sizeof(unsigned long long) * SLOTS, ms->stream));
    TH_HIP(ms, hipMemsetAsync(d_claimed, 0, sizeof(unsigned int) * SLOTS, ms->stream));
    TH_HIP(ms, hipMemsetAsync(d_names, 0, (size_t)SLOTS * NAME_STRIDE, ms->stream));
    SplitWords words;
    std::vector<std::vector<char>> text_of((size_t)SLOTS);                    // the host appends per slot
    std::vector<int64_t> lines_of((size_t)SLOTS, 0);
    std::vector<unsigned long long> slot_byte((size_t)SLOTS);
    std::vector<unsigned int> slot_record((size_t)SLOTS);
    std::vector<int> present;
    const fhx::Refusal refuse{ms, why, bad_line};
    bool overflow = false;
    for (; in.more(); in.advance()) {
        std::memset(&words, 0, sizeof(words));
        words.first_error = NO_ERROR;
        words.overflow = overflow ? 1ull : 0ull;
        TH_HIP(ms, hipMemcpyAsync(d_words, &words, sizeof(words), hipMemcpyHostToDevice, ms->stream));
        if (const int rc = in.next<GrammarBytes>()) return rc;
        const unsigned char* d_text = in.d_text;
        const unsigned long long* d_block_off = in.d_block_off;
        const int64_t len = in.len, n_blocks = in.n_blocks, n = in.lines;
        TH_HIP(ms, tmp.grow(&d_keep_len, &keep_capacity, n));                 // one length and one slot per line of the batch
        TH_HIP(ms, tmp.grow(&d_line_slot, &slot_capacity, n));
        hipLaunchKernelGGL(mp_names, dim3((unsigned)n_blocks), dim3(WG), 0, ms->stream, d_text, len, d_block_off, n, in.off, d_line_slot, d_hash,
                           d_off, d_claimed, d_words);
        hipLaunchKernelGGL(mp_copy_names, dim3(SLOTS / WG), dim3(WG), 0, ms->stream, d_text, len, in.off, (const unsigned long long*)d_off, d_claimed,
                           d_names);
        hipLaunchKernelGGL(mp_select, dim3((unsigned)n_blocks), dim3(WG), 0, ms->stream, d_text, len, d_block_off, n, in.line_base, fdr,
                           (unsigned long long)key_bound, (int)zero_kept, (int)in.refused_bytes, (const unsigned short*)d_line_slot,
                           (const unsigned char*)d_names, d_keep_len, d_block_kept, d_words);
        hipLaunchKernelGGL(fhxscan::scan_tiles, dim3(1), dim3(fhxscan::THREADS), 0, ms->stream, (const unsigned int*)d_block_kept, n_blocks, d_rec_off,
                           &d_words->kept_lines);
        TH_HIP(ms, hipGetLastError());
        TH_HIP(ms, hipMemcpyAsync(&words, d_words, sizeof(words), hipMemcpyDeviceToHost, ms->stream));
        TH_HIP(ms, hipStreamSynchronize(ms->stream));
        if (words.first_error != NO_ERROR) return refuse.word(words.first_error, FHX_MS_INTERNAL);      // earlier batches hold the smaller line numbers
        overflow = overflow || words.overflow != 0;
        const int64_t n_records = overflow ? 0 : (int64_t)words.kept_lines;   // after an overflow the lines are only checked
        if (n_records > n) return refuse(FHX_ERR_INTERNAL, FHX_MS_INTERNAL, 0, "more kept lines than lines");
        if (n_records > 0) {
            TH_HIP(ms, tmp.grow(&d_records, &rec_capacity, n_records));
            hipLaunchKernelGGL(mp_emit, dim3((unsigned)n_blocks), dim3(WG), 0, ms->stream, d_text, len, d_block_off, n, (const unsigned short*)d_line_slot,
                               (const unsigned short*)d_keep_len, (const unsigned long long*)d_rec_off, d_records, n_records);
            TH_HIP(ms, hipGetLastError());
            TH_HIP(ms, hipStreamSynchronize(ms->stream));                     // the sorter has a stream of its own
        }
        clock.mark(2);
        int64_t bytes = 0;
        if (n_records > 0) {
            const int64_t n_tiles = (n_records + ROUND - 1) / ROUND;
            TH_HIP(ms, tmp.grow(&d_sorted, &sorted_capacity, n_records));
            TH_HIP(ms, tmp.grow(&d_perm, &perm_capacity, n_records));
            TH_HIP(ms, tmp.grow(&d_tile_bytes, &tile_capacity, n_tiles));
            TH_HIP(ms, tmp.grow(&d_tile_off, &tile_off_capacity, n_tiles));
            const int rc = fhx_sort_u64(ms->sorter, d_records, n_records, d_sorted, d_perm);
            if (rc != FHX_OK) return refuse(rc, FHX_MS_INTERNAL, 0, std::string("sort: ") + fhx_last_error(ms->sorter));
            TH_HIP(ms, hipMemsetAsync(d_slot_record, 0xFF, sizeof(unsigned int) * SLOTS, ms->stream));
            hipLaunchKernelGGL(mp_tile_bytes, dim3((unsigned)n_tiles), dim3(ROUND), 0, ms->stream, (const unsigned long long*)d_sorted, n_records,
                               d_tile_bytes);
            hipLaunchKernelGGL(fhxscan::scan_tiles, dim3(1), dim3(fhxscan::THREADS), 0, ms->stream, (const unsigned int*)d_tile_bytes, n_tiles,
                               d_tile_off, &d_words->out_bytes);
            hipLaunchKernelGGL(mp_gather, dim3((unsigned)n_tiles), dim3(ROUND), 0, ms->stream, d_text, len, (const unsigned long long*)d_sorted,
                               n_records, (const unsigned long long*)d_tile_off, d_out, out_capacity, d_slot_byte, d_slot_record);
            TH_HIP(ms, hipGetLastError());
            TH_HIP(ms, hipMemcpyAsync(&words, d_words, sizeof(words), hipMemcpyDeviceToHost, ms->stream));
            TH_HIP(ms, hipMemcpyAsync(slot_byte.data(), d_slot_byte, sizeof(unsigned long long) * SLOTS, hipMemcpyDeviceToHost, ms->stream));
            TH_HIP(ms, hipMemcpyAsync(slot_record.data(), d_slot_record, sizeof(unsigned int) * SLOTS, hipMemcpyDeviceToHost, ms->stream));
            TH_HIP(ms, hipStreamSynchronize(ms->stream));
            bytes = (int64_t)words.out_bytes;
            if (bytes > out_capacity || bytes < n_records) return refuse(FHX_ERR_INTERNAL, FHX_MS_INTERNAL, 0, "more kept bytes than text");
        }
        clock.mark(3);
        if (n_records > 0) {                                                  // one copy per chromosome of the batch: its run of the sorted bytes
            present.clear();
            for (int s = 0; s < SLOTS; ++s)
                if (slot_record[(size_t)s] != 0xFFFFFFFFu) present.push_back(s);              // ascending slots = ascending runs
            for (size_t k = 0; k < present.size(); ++k) {
                const int s = present[k];
                const bool last = k + 1 == present.size();
                const int64_t b_at = (int64_t)slot_byte[(size_t)s], b_end = last ? bytes : (int64_t)slot_byte[(size_t)present[k + 1]];
                const int64_t r_at = (int64_t)slot_record[(size_t)s], r_end = last ? n_records : (int64_t)slot_record[(size_t)present[k + 1]];
                if (b_at < 0 || b_end <= b_at || b_end > bytes || r_end <= r_at || (k == 0 && (b_at != 0 || r_at != 0)))
                    return refuse(FHX_ERR_INTERNAL, FHX_MS_INTERNAL, 0, "the runs of the sorted records do not tile the subset");
                std::vector<char>& dst = text_of[(size_t)s];
                const size_t had = dst.size();
                dst.resize(had + (size_t)(b_end - b_at));
                TH_HIP(ms, hipMemcpyAsync(dst.data() + had, d_out + b_at, (size_t)(b_end - b_at), hipMemcpyDeviceToHost, ms->stream));
                lines_of[(size_t)s] += r_end - r_at;
            }
            TH_HIP(ms, hipStreamSynchronize(ms->stream));
        }
        clock.mark(4);
    }
    if (overflow)
        return refuse(FHX_ERR_UNSUPPORTED, FHX_MS_NAMES, 0, "more than " + std::to_string(SLOTS) + " distinct names in field 1");
    // the names, in slot order; the caller orders them
    std::vector<unsigned long long> hash((size_t)SLOTS);
    std::vector<unsigned char> names((size_t)SLOTS * NAME_STRIDE);
    TH_HIP(ms, hipMemcpyAsync(hash.data(), d_hash, sizeof(unsigned long long) * SLOTS, hipMemcpyDeviceToHost, ms->stream));
    TH_HIP(ms, hipMemcpyAsync(names.data(), d_names, names.size(), hipMemcpyDeviceToHost, ms->stream));
    TH_HIP(ms, hipStreamSynchronize(ms->stream));
    for (int s = 0; s < SLOTS; ++s) {
        if (!hash[(size_t)s]) continue;
        const unsigned char* at = names.data() + (size_t)s * NAME_STRIDE;
        fhx_ms::SplitName one;
        one.name.assign((const char*)at, (size_t)std::min<int>(at[NAME_STRIDE - 1], NAME_STRIDE - 1));
        one.text.swap(text_of[(size_t)s]);
        one.lines = lines_of[(size_t)s];
        ms->split.push_back(std::move(one));
    }
    clock.mark(4);
    ms->s_lines = in.line_base;
    *n_names = (int32_t)ms->split.size();
    if (std::getenv("FHX_TIMING"))
        std::fprintf(stderr, "per-chromosome FDR subsets on the device (%s): %lld lines, %d names: read + upload %.6f s; scan %.6f s; names + select "
                     "%.6f s; sort + gather %.6f s; copy out %.6f s\n", path, (long long)in.line_base, (int)ms->split.size(), ms->s_seconds[0],
                     ms->s_seconds[1], ms->s_seconds[2], ms->s_seconds[3], ms->s_seconds[4]);
    return FHX_OK;
}

}  // namespace

extern "C" {

int fhx_ms_split_file(fhx_ms* ms, const char* path, const char* fdr_text, int32_t fdr_len, uint64_t key_bound, int32_t zero_kept,
                      int32_t* n_names, int32_t* why, int64_t* bad_line) {
    if (!ms || !path || !fdr_text || !n_names || !why || !bad_line) return FHX_ERR_ARG;
    *n_names = 0;
    *why = FHX_MS_OK;
    *bad_line = 0;
    const int rc = split_file(ms, path, fdr_text, fdr_len, key_bound, zero_kept, n_names, why, bad_line);
    if (rc != FHX_OK) drop_split(ms);                                         // the one exit of a failed call, whatever failed
    return rc;
}

int fhx_ms_split_counts(const fhx_ms* ms, int64_t* n_lines, int32_t* n_names, int64_t* kept_lines, int64_t* kept_bytes, int32_t capacity) {
    if (!ms) return FHX_ERR_ARG;
    if (n_lines) *n_lines = ms->s_lines;
    if (n_names) *n_names = (int32_t)ms->split.size();
    if (kept_lines || kept_bytes) {
        if (capacity < (int32_t)ms->split.size()) return FHX_ERR_ARG;
        for (size_t k = 0; k < ms->split.size(); ++k) {
            if (kept_lines) kept_lines[k] = ms->split[k].lines;
            if (kept_bytes) kept_bytes[k] = (int64_t)ms->split[k].text.size();
        }
    }
    return FHX_OK;
}

int fhx_ms_split_names(const fhx_ms* ms, char* dst, int32_t capacity) {
    if (!ms || capacity < (int32_t)ms->split.size() || (!dst && !ms->split.empty())) return FHX_ERR_ARG;
    for (size_t k = 0; k < ms->split.size(); ++k) {
        std::memset(dst + k * FHX_MS_SPLIT_NAME_BYTES, 0, FHX_MS_SPLIT_NAME_BYTES);
        std::memcpy(dst + k * FHX_MS_SPLIT_NAME_BYTES, ms->split[k].name.data(), ms->split[k].name.size());
    }
    return FHX_OK;
}

int fhx_ms_split_stage_seconds(const fhx_ms* ms, double* seconds) {
    if (!ms || !seconds) return FHX_ERR_ARG;
    for (int k = 0; k < FHX_MS_SPLIT_STAGES; ++k) seconds[k] = ms->s_seconds[k];
    return FHX_OK;
}

int fhx_ms_copy_split(const fhx_ms* ms, int32_t index, void* dst, int64_t capacity) {
    if (!ms || index < 0 || index >= (int32_t)ms->split.size()) return FHX_ERR_ARG;
    const std::vector<char>& text = ms->split[(size_t)index].text;
    if (capacity < (int64_t)text.size() || (!dst && !text.empty())) return FHX_ERR_ARG;
    if (!text.empty()) std::memcpy(dst, text.data(), text.size());
    return FHX_OK;
}

}  // extern "C"
