// fhx_ingest.inc - the contact-counts file parsed ON THE GPU (included by fhx_device.hip after fhx_inflate.inc, outside extern "C").
//
// The reference reads the file line by line (fithic/fithic.py:404-417): `ch1, mid1, ch2, mid2, contactCount = line.split()`,
// int(mid), int(float(count)).  fhx_host_read_table does that on the host cores (0.8 s for 1.5e8 rows on 16 of them, then five
// columns to upload and to index); here the inflated text goes to HBM as it is and kernels do the rest:
//
//   scan_text, scan_tiles    the newline layer (fhx_textlines.hpp) with the text-mode byte policy: the row number of every
//                  block's first line, and the bytes this path does not take (see below)
//   ti_parse       the lines that begin in a block, one per thread: two names, two midpoints, the count.  Names go through a
//                  64-bit hash into a 16 384-slot table in HBM; a wave inserts each DISTINCT name once (its lanes vote), and
//                  only when the table does not yet hold it with an earlier position - sorted files touch it a few thousand
//                  times in all.  The table keeps the smallest byte offset a name was seen at = its first appearance.
//   ti_fetch_names the name texts at those offsets -> the host orders them by offset: the reference's order of appearance
//   ti_verify      every row's two names compared byte by byte with the text of its slot (a hash collision cannot pass)
//   ti_map_rows    slot -> the caller's chromosome id; then the rows enter the context like fhx_load_pairs_device's
//
// ONLY THE REGULAR FILE IS TAKEN: ASCII text, no NUL, no \r outside \r\n, five tokens per line, names of 1..63 bytes, midpoints
// [+-]?digits (at most 10 digits, within int32), count = digits[.digits] (at most 15 digits, integer part within int32: the
// reference's int(float(text)) is then the integer part as written; a non-zero digit behind the point is remembered in the
// context, fhx_ctx::counts_integral).  Anything else - an underscore in a number, an exponent,
// a signed count, a sixth token, an empty line, a malformed line whose error the caller must see -
// returns FHX_ERR_UNSUPPORTED before anything is loaded and the caller parses the same inflated text with
// fhx_host_parse_text, whose grammar is Python's.  No row is ever parsed "approximately".

namespace fhx {
namespace ingest {

using namespace fhxlines;

constexpr int TABLE_SLOTS = 16384;
constexpr int MAX_NAMES = 8192;
constexpr int NAME_STRIDE = 64;                // names of up to 63 bytes

enum : unsigned int { F_BYTES = REFUSED_BYTES, F_LINE = 2u, F_TABLE = 4u, F_COLLISION = 8u,
                      F_FRACTION = 16u };      // some count has a non-zero fractional digit: refuses nothing, the context remembers it

__device__ inline bool is_space(int c) { return c == ' ' || (c >= '\t' && c <= '\r') || (c >= 0x1c && c <= 0x1f); }

struct Cursor {
    const unsigned char* text;
    int64_t T, p, limit;
    __device__ int at() const { return p < T ? (int)text[p] : '\n'; }          // the end of the text ends the line
    // to the next token of the line; false at the end of the line (or past the length this path takes)
    __device__ bool next_token() {
        for (;;) {
            const int c = at();
            if (c == '\n' || p >= limit) return false;
            if (!is_space(c)) return true;
            ++p;
        }
    }
    __device__ bool name(unsigned long long* hash, int64_t* off, int* len) {
        *off = p;
        unsigned long long h = 0xcbf29ce484222325ull;                         // FNV-1a; equal names are confirmed by ti_verify
        int n = 0;
        for (;;) {
            const int c = at();
            if (is_space(c)) break;
            if (++n >= NAME_STRIDE) return false;
            h = (h ^ (unsigned long long)c) * 0x100000001b3ull;
            ++p;
        }
        *hash = h ? h : 1;                                                    // 0 marks an empty slot
        *len = n;
        return n > 0;
    }
    __device__ bool skip_token() {
        int n = 0;
        while (!is_space(at())) {
            if (++n > 16) return false;
            ++p;
        }
        return n > 0;
    }
    // int(text) of [+-]?digits: at most 10 digits, within int32
    __device__ bool integer(int* out) {
        int c = at();
        bool neg = false;
        if (c == '+' || c == '-') {
            neg = c == '-';
            ++p;
        }
        long long v = 0;
        int nd = 0;
        for (;;) {
            c = at();
            if (c < '0' || c > '9') break;
            if (++nd > 10) return false;
            v = v * 10 + (c - '0');
            ++p;
        }
        if (nd == 0 || !is_space(c)) return false;                           // "1_000", "1.0", "1e3", "0x10": the host parser's
        if (neg) v = -v;
        if (v < -2147483648ll || v > 2147483647ll) return false;
        *out = (int)v;
        return true;
    }
    // int(float(text)) of digits[.digits] (either side of the point may be empty, not both): with at most 15 digits in all the
    // double nearest the decimal cannot reach the next integer (the gap to it is >= 10^(k-15) for k integer digits, half an ulp
    // is < 1.2 * 10^(k-16)), so the truncation is the integer part as written.  Signs, exponents, inf/nan: the host parser's.
    __device__ bool count(int* out, bool* fraction) {
        long long v = 0;
        int ni = 0, nf = 0, c;
        bool nonzero = false;
        for (;;) {
            c = at();
            if (c < '0' || c > '9') break;
            if (++ni > 10) return false;
            v = v * 10 + (c - '0');
            ++p;
        }
        if (c == '.') {
            ++p;
            for (;;) {
                c = at();
                if (c < '0' || c > '9') break;
                if (++nf > 15) return false;
                nonzero |= c != '0';
                ++p;
            }
        }
        if (ni + nf == 0 || ni + nf > 15 || !is_space(c)) return false;
        if (v > 2147483647ll) return false;
        *out = (int)v;
        *fraction = nonzero;                                                 // "3.0", "3." and "03.000" are integers as written
        return true;
    }
};

// the table: hash[slot] (0 = empty), off[slot] = the smallest text offset the name was seen at
__device__ inline int table_insert(unsigned long long* __restrict__ t_hash, unsigned long long* __restrict__ t_off, unsigned long long h,
                                   unsigned long long off, unsigned int* __restrict__ flags) {
    unsigned int s = (unsigned int)((h * 0x9e3779b97f4a7c15ull) >> 50) & (TABLE_SLOTS - 1);
    for (int probes = 0; probes < TABLE_SLOTS; ++probes) {
        unsigned long long cur = __hip_atomic_load(&t_hash[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            cur = atomicCAS(&t_hash[s], 0ull, h);
            if (cur == 0) cur = h;
        }
        if (cur == h) {
            if (__hip_atomic_load(&t_off[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > off) atomicMin(&t_off[s], off);
            return (int)s;
        }
        s = (s + 1) & (TABLE_SLOTS - 1);
    }
    atomicOr(flags, F_TABLE);
    return 0;
}

// one distinct name of the wave at a time: the lowest lane that still has one inserts it for every lane holding the same hash
// (lanes hold consecutive lines, so that lane's offset is the group's smallest)
__device__ inline int wave_insert(bool have, unsigned long long h, int64_t off, unsigned long long* t_hash, unsigned long long* t_off,
                                  unsigned int* flags) {
    int slot = 0;
    const int lane = threadIdx.x & 63;
    for (;;) {
        const unsigned long long todo = __ballot(have);
        if (!todo) break;
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned long long lh = __shfl(h, leader, 64);
        int s = 0;
        if (lane == leader) s = table_insert(t_hash, t_off, h, (unsigned long long)off, flags);
        s = __shfl(s, leader, 64);
        if (have && h == lh) {
            slot = s;
            have = false;
        }
    }
    return slot;
}

__global__ __launch_bounds__(WG) void ti_parse(const unsigned char* __restrict__ text, int64_t T, const unsigned long long* __restrict__ block_off,
                                               int32_t* __restrict__ mid1, int32_t* __restrict__ mid2, int32_t* __restrict__ count,
                                               unsigned int* __restrict__ slots, unsigned long long* __restrict__ t_hash,
                                               unsigned long long* __restrict__ t_off, unsigned int* __restrict__ flags) {
    __shared__ unsigned short lstart[LSTART_ENTRIES];
    const int n_lines = block_lines(text, T, lstart);
    const int64_t b0 = (int64_t)blockIdx.x * BLOCK_BYTES;
    const int64_t row0 = blockIdx.x == 0 ? 0 : (int64_t)block_off[blockIdx.x] + 1;
    bool bad = false, fraction = false;
    for (int base = 0; base < n_lines; base += WG) {
        const int e = base + threadIdx.x;
        const bool active = e < n_lines;
        unsigned long long h1 = 0, h2 = 0;
        int64_t o1 = 0, o2 = 0;
        int l1, l2, m1 = 0, m2 = 0, cnt = 0;
        bool ok = false, frac = false;
        if (active) {
            Cursor c{text, T, b0 + lstart[e], 0};
            c.limit = c.p + MAX_LINE;
            ok = c.next_token() && c.name(&h1, &o1, &l1) && c.next_token() && c.integer(&m1) && c.next_token() &&
                 c.name(&h2, &o2, &l2) && c.next_token() && c.integer(&m2) && c.next_token() && c.count(&cnt, &frac);
            if (ok) ok = !c.next_token() && c.at() == '\n';                  // a sixth token, or a line longer than this path takes
            bad |= !ok;
            fraction |= ok && frac;
        }
        const int s1 = wave_insert(ok, h1, o1, t_hash, t_off, flags);
        const int s2 = wave_insert(ok, h2, o2, t_hash, t_off, flags);
        if (ok) {
            const int64_t r = row0 + e;
            mid1[r] = m1;
            mid2[r] = m2;
            count[r] = cnt;
            slots[r] = (unsigned int)s1 | ((unsigned int)s2 << 16);
        }
    }
    if (bad) atomicOr(flags, F_LINE);
    if (fraction) atomicOr(flags, F_FRACTION);
}

__global__ void ti_fetch_names(const unsigned char* __restrict__ text, int64_t T, const unsigned long long* __restrict__ offs, int n,
                               unsigned char* __restrict__ pool, int* __restrict__ lens) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int64_t p = (int64_t)offs[i];
    int len = 0;
    while (p < T && !is_space(text[p]) && len < NAME_STRIDE - 1) pool[(size_t)i * NAME_STRIDE + len++] = text[p++];
    lens[i] = len;
}

// every row's names against the text of their slots
__global__ __launch_bounds__(WG) void ti_verify(const unsigned char* __restrict__ text, int64_t T, const unsigned long long* __restrict__ block_off,
                                                const unsigned int* __restrict__ slots, const short* __restrict__ slot_name,
                                                const unsigned char* __restrict__ pool, const int* __restrict__ lens,
                                                unsigned int* __restrict__ flags) {
    __shared__ unsigned short lstart[LSTART_ENTRIES];
    const int n_lines = block_lines(text, T, lstart);
    const int64_t b0 = (int64_t)blockIdx.x * BLOCK_BYTES;
    const int64_t row0 = blockIdx.x == 0 ? 0 : (int64_t)block_off[blockIdx.x] + 1;
    bool bad = false;
    for (int e = threadIdx.x; e < n_lines; e += WG) {
        Cursor c{text, T, b0 + lstart[e], 0};
        c.limit = c.p + MAX_LINE;
        const unsigned int s = slots[row0 + e];
        auto same = [&](unsigned int slot) {
            const int name = slot_name[slot];
            if (name < 0) return false;
            const int len = lens[name];
            const unsigned char* want = pool + (size_t)name * NAME_STRIDE;
            for (int k = 0; k < len; ++k)
                if (c.p + k >= T || text[c.p + k] != want[k]) return false;
            c.p += len;
            return is_space(c.at());
        };
        bool ok = c.next_token() && same(s & 0xFFFFu) && c.next_token() && c.skip_token() && c.next_token() && same(s >> 16);
        bad |= !ok;
    }
    if (bad) atomicOr(flags, F_COLLISION);
}

__global__ void ti_map_rows(const unsigned int* __restrict__ slots, const int32_t* __restrict__ slot_id, int64_t n, int32_t* __restrict__ chr1,
                            int32_t* __restrict__ chr2) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const unsigned int s = slots[r];
        chr1[r] = slot_id[s & 0xFFFFu];
        chr2[r] = slot_id[s >> 16];
    }
}

// the identity columns of loaded rows rebuilt from the resident ones (what em_format's derive branch does): rows == nullptr
// -> rows 0..n-1
__global__ void ti_rebuild_rows(const int64_t* __restrict__ rows, int64_t n, int64_t n_loaded, const int32_t* __restrict__ loc1,
                                const int32_t* __restrict__ loc2, const int32_t* __restrict__ cnt, const int16_t* __restrict__ slot_chr,
                                const int32_t* __restrict__ slot_mid, const fhx::ChrGrid* __restrict__ grid, int32_t res,
                                int32_t* __restrict__ out /* 5 columns of n */, int* __restrict__ bad) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = rows ? rows[i] : i;
        if (r < 0 || r >= n_loaded) {
            *bad = 1;
            continue;
        }
        const int s1 = loc1[r], l2 = loc2[r], s2 = l2 < 0 ? ~l2 : l2;
        const int c1 = slot_chr[s1], c2 = slot_chr[s2];
        out[i] = c1;
        out[n + i] = slot_mid ? slot_mid[s1] : (s1 - grid[c1].base) * res + grid[c1].off;
        out[2 * n + i] = c2;
        out[3 * n + i] = slot_mid ? slot_mid[s2] : (s2 - grid[c2].base) * res + grid[c2].off;
        out[4 * n + i] = cnt[r];
    }
}

}  // namespace ingest
}  // namespace fhx

// what fhx_ingest_contacts_text leaves in the context for fhx_ingest_contacts_commit
struct fhx_ctx::TextIngest {
    int64_t n_rows = 0;
    int32_t *d_mid1 = nullptr, *d_mid2 = nullptr, *d_count = nullptr;
    unsigned int* d_slots = nullptr;
    bool fraction = false;                     // F_FRACTION: d_count holds the integer part of some count that had more
    std::vector<std::string> names;            // order of first appearance
    std::vector<int> name_slot;                // table slot of each
    ~TextIngest() {                            // the only place the four columns go, but for d_slots once the rows are mapped
        dev_free(d_mid1);
        dev_free(d_mid2);
        dev_free(d_count);
        dev_free(d_slots);
    }
};

static void ingest_drop(fhx_ctx* ctx) {
    delete ctx->text_ingest;
    ctx->text_ingest = nullptr;
}

// the stages shared by both entry points: a text resident in HBM (padded with blanks to whole blocks + 64) -> parsed rows and
// names in *st
struct IngestClock {
    fhx_ctx* ctx;
    bool on;
    std::chrono::steady_clock::time_point last;
    std::string report;
    void mark(const char* what) {
        if (!on) return;
        (void)hipStreamSynchronize(ctx->stream);
        const auto now = std::chrono::steady_clock::now();
        char b[96];
        std::snprintf(b, sizeof(b), " %s %.3f s;", what, std::chrono::duration<double>(now - last).count());
        report += b;
        last = now;
    }
};

static int ingest_parse_resident(fhx_ctx* ctx, DeviceScratch& tmp, unsigned char* d_text, int64_t T, const std::string& label, IngestClock& clock,
                                 std::unique_ptr<fhx_ctx::TextIngest>& st, int64_t* n_rows, int32_t* n_names, bool* grammar) {
    using namespace fhx::ingest;
    const int64_t n_blocks = (T + BLOCK_BYTES - 1) / BLOCK_BYTES;
    const bool timing = clock.on;
    std::string& t_report = clock.report;
    auto mark = [&](const char* what) { clock.mark(what); };
    unsigned int *d_block_nl = nullptr, *d_flags = nullptr;
    unsigned long long *d_block_off = nullptr, *d_total = nullptr, *d_t_hash = nullptr, *d_t_off = nullptr;
    FHX_HIP(tmp.get(&d_block_nl, (size_t)n_blocks * sizeof(unsigned int)));
    FHX_HIP(tmp.get(&d_block_off, (size_t)n_blocks * sizeof(unsigned long long)));
    FHX_HIP(tmp.get(&d_total, sizeof(unsigned long long)));
    FHX_HIP(tmp.get(&d_flags, sizeof(unsigned int)));
    FHX_HIP(tmp.get(&d_t_hash, (size_t)TABLE_SLOTS * sizeof(unsigned long long)));
    FHX_HIP(tmp.get(&d_t_off, (size_t)TABLE_SLOTS * sizeof(unsigned long long)));
    FHX_HIP(hipMemsetAsync(d_flags, 0, sizeof(unsigned int), ctx->stream));
    FHX_HIP(hipMemsetAsync(d_t_hash, 0, (size_t)TABLE_SLOTS * sizeof(unsigned long long), ctx->stream));
    FHX_HIP(hipMemsetAsync(d_t_off, 0xFF, (size_t)TABLE_SLOTS * sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(scan_text<TextModeBytes>, dim3((unsigned)n_blocks), dim3(WG), 0, ctx->stream, (const unsigned char*)d_text, T, d_block_nl, d_flags);
    hipLaunchKernelGGL(fhxscan::scan_tiles, dim3(1), dim3(fhxscan::THREADS), 0, ctx->stream, (const unsigned int*)d_block_nl, n_blocks, d_block_off,
                       d_total);
    unsigned long long n_newlines = 0;
    unsigned int flags = 0;
    unsigned char last = 0;
    FHX_HIP(hipMemcpyAsync(&n_newlines, d_total, sizeof(n_newlines), hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipMemcpyAsync(&flags, d_flags, sizeof(flags), hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipMemcpyAsync(&last, d_text + T - 1, 1, hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipStreamSynchronize(ctx->stream));
    mark("newlines");
    auto refuse = [&](const char* why) {
        *grammar = true;
        if (timing) std::fprintf(stderr, "contacts on the device (%s):%s refused: %s\n", label.c_str(), t_report.c_str(), why);
        return fail(ctx, FHX_ERR_UNSUPPORTED, std::string("the contacts text goes to the host parser: ") + why);
    };
    if (flags & F_BYTES) return refuse("a NUL, a non-ASCII byte or a \\r that is not part of \\r\\n");
    const int64_t n = (int64_t)n_newlines + (last == '\n' ? 0 : 1);
    st->n_rows = n;
    FHX_HIP(dev_malloc(&st->d_mid1, (size_t)n * sizeof(int32_t)));
    FHX_HIP(dev_malloc(&st->d_mid2, (size_t)n * sizeof(int32_t)));
    FHX_HIP(dev_malloc(&st->d_count, (size_t)n * sizeof(int32_t)));
    FHX_HIP(dev_malloc(&st->d_slots, (size_t)n * sizeof(unsigned int)));
    hipLaunchKernelGGL(ti_parse, dim3((unsigned)n_blocks), dim3(WG), 0, ctx->stream, (const unsigned char*)d_text, T,
                       (const unsigned long long*)d_block_off, st->d_mid1, st->d_mid2, st->d_count, st->d_slots, d_t_hash, d_t_off, d_flags);
    std::vector<unsigned long long> t_hash(TABLE_SLOTS), t_off(TABLE_SLOTS);
    FHX_HIP(hipMemcpyAsync(&flags, d_flags, sizeof(flags), hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipMemcpyAsync(t_hash.data(), d_t_hash, t_hash.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipMemcpyAsync(t_off.data(), d_t_off, t_off.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipStreamSynchronize(ctx->stream));
    mark("parse");
    if (flags & F_LINE) return refuse("a line that is not `name int name int digits`");
    if (flags & F_TABLE) return refuse("more chromosome names than the device table holds");
    st->fraction = (flags & F_FRACTION) != 0;
    std::vector<std::pair<unsigned long long, int>> seen;                   // (first offset, slot)
    for (int s = 0; s < TABLE_SLOTS; ++s)
        if (t_hash[s]) seen.emplace_back(t_off[s], s);
    if ((int)seen.size() > MAX_NAMES) return refuse("more chromosome names than the device table holds");
    std::sort(seen.begin(), seen.end());
    const int k_names = (int)seen.size();
    std::vector<unsigned long long> offs(std::max(k_names, 1));
    std::vector<short> slot_name(TABLE_SLOTS, (short)-1);
    for (int i = 0; i < k_names; ++i) {
        offs[i] = seen[i].first;
        slot_name[seen[i].second] = (short)i;
    }
    unsigned long long* d_offs = nullptr;
    unsigned char* d_pool = nullptr;
    int* d_lens = nullptr;
    short* d_slot_name = nullptr;
    FHX_HIP(tmp.get(&d_offs, offs.size() * sizeof(unsigned long long)));
    FHX_HIP(tmp.get(&d_pool, offs.size() * NAME_STRIDE));
    FHX_HIP(tmp.get(&d_lens, offs.size() * sizeof(int)));
    FHX_HIP(tmp.get(&d_slot_name, slot_name.size() * sizeof(short)));
    FHX_HIP(hipMemcpyAsync(d_offs, offs.data(), offs.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
    FHX_HIP(hipMemcpyAsync(d_slot_name, slot_name.data(), slot_name.size() * sizeof(short), hipMemcpyHostToDevice, ctx->stream));
    std::vector<unsigned char> pool(offs.size() * NAME_STRIDE);
    std::vector<int> lens(offs.size());
    if (k_names) {
        hipLaunchKernelGGL(ti_fetch_names, dim3((k_names + 63) / 64), dim3(64), 0, ctx->stream, (const unsigned char*)d_text, T,
                           (const unsigned long long*)d_offs, k_names, d_pool, d_lens);
        hipLaunchKernelGGL(ti_verify, dim3((unsigned)n_blocks), dim3(WG), 0, ctx->stream, (const unsigned char*)d_text, T,
                           (const unsigned long long*)d_block_off, (const unsigned int*)st->d_slots, (const short*)d_slot_name,
                           (const unsigned char*)d_pool, (const int*)d_lens, d_flags);
    }
    FHX_HIP(hipMemcpyAsync(pool.data(), d_pool, pool.size(), hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipMemcpyAsync(lens.data(), d_lens, lens.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipMemcpyAsync(&flags, d_flags, sizeof(flags), hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipStreamSynchronize(ctx->stream));
    mark("names + verification");
    if (flags & F_COLLISION) return refuse("two chromosome names with one hash");
    st->names.resize(k_names);
    st->name_slot.resize(k_names);
    for (int i = 0; i < k_names; ++i) {
        st->names[i].assign((const char*)pool.data() + (size_t)i * NAME_STRIDE, (size_t)lens[i]);
        st->name_slot[i] = seen[i].second;
    }
    *n_rows = n;
    *n_names = k_names;
    ctx->text_ingest = st.release();
    if (timing)
        std::fprintf(stderr, "contacts on the device (%s): %lld rows, %d names, %lld bytes of text:%s\n", label.c_str(), (long long)n, k_names,
                     (long long)T, t_report.c_str());
    return FHX_OK;
}


extern "C" {

void fhx_ingest_contacts_discard(fhx_ctx* ctx) {
    if (!ctx || !ctx->text_ingest) return;
    if (ctx->device >= 0) (void)hipSetDevice(ctx->device);
    ingest_drop(ctx);
}

// the spans of host text (T bytes in all) uploaded and parsed
static int ingest_text_spans(fhx_ctx* ctx, const std::vector<std::pair<const char*, size_t>>& spans, int64_t T, const std::string& path,
                             int32_t n_threads, int64_t* n_rows, int32_t* n_names) {
    using namespace fhx::ingest;
    if (ctx->device < 0) return fail(ctx, FHX_ERR_NO_DEVICE, "host-only context");
    FHX_HIP(hipSetDevice(ctx->device));
    ingest_drop(ctx);
    *n_rows = 0;
    *n_names = 0;
    IngestClock clock{ctx, std::getenv("FHX_TIMING") != nullptr, std::chrono::steady_clock::now(), ""};
    std::unique_ptr<fhx_ctx::TextIngest> st(new (std::nothrow) fhx_ctx::TextIngest());
    if (!st) return FHX_ERR_NOMEM;
    if (T == 0) {                                                             // an empty file: no rows, no names
        ctx->text_ingest = st.release();
        return FHX_OK;
    }
    if (n_threads <= 0) n_threads = fhx::usable_cpus();
    const int64_t n_blocks = (T + BLOCK_BYTES - 1) / BLOCK_BYTES;
    if (n_blocks > 0x7fffffffll) return fail(ctx, FHX_ERR_UNSUPPORTED, "text of more than 32 TB");
    DeviceScratch tmp;
    unsigned char* d_text = nullptr;
    FHX_HIP(tmp.get(&d_text, (size_t)n_blocks * BLOCK_BYTES + 64));
    // ---- the text to HBM: host threads fill two pinned 64 MB buffers, the copy engine drains them -------------------------
    {
        const int rc = upload_spans(ctx, spans, d_text, n_threads);
        if (rc != FHX_OK) return rc;
        FHX_HIP(hipMemsetAsync(d_text + T, ' ', (size_t)(n_blocks * BLOCK_BYTES + 64 - T), ctx->stream));
    }
    clock.mark("text to HBM");
    bool grammar = false;
    return ingest_parse_resident(ctx, tmp, d_text, T, path, clock, st, n_rows, n_names, &grammar);
}

int fhx_ingest_contacts_text(fhx_ctx* ctx, const fhx_text* text, int32_t n_threads, int64_t* n_rows, int32_t* n_names) {
    if (!ctx || !text || !n_rows || !n_names) return FHX_ERR_ARG;
    std::vector<std::pair<const char*, size_t>> spans;
    for (const fhx::TextPiece& piece : text->pieces) spans.emplace_back(piece.data(), piece.size());
    return ingest_text_spans(ctx, spans, text->bytes, text->path, n_threads, n_rows, n_names);
}

// Part `part` of `n_parts` of an inflated text (fhx_text_part_bounds) uploaded and parsed.  For sharded runs over a file the device
// does not inflate (plain gzip): every rank inflates it on its host cores, then uploads and parses 1/N of the text.
int fhx_ingest_contacts_text_slice(fhx_ctx* ctx, const fhx_text* text, int32_t n_threads, int32_t part, int32_t n_parts, int64_t* n_rows,
                                   int32_t* n_names) {
    if (!ctx || !text || !n_rows || !n_names) return FHX_ERR_ARG;
    int64_t lo = 0, hi = 0;
    if (fhx_text_part_bounds(text, part, n_parts, &lo, &hi) != FHX_OK) return FHX_ERR_ARG;
    std::vector<std::pair<const char*, size_t>> spans;
    int64_t base = 0;
    for (const fhx::TextPiece& piece : text->pieces) {
        const int64_t n = (int64_t)piece.size(), a = std::max(lo, base), b = std::min(hi, base + n);
        if (b > a) spans.emplace_back(piece.data() + (a - base), (size_t)(b - a));
        base += n;
    }
    return ingest_text_spans(ctx, spans, std::max<int64_t>(0, hi - lo), text->path, n_threads, n_rows, n_names);
}

// A part of a plain gzip stream inflated by this rank (fhx_host_inflate_part / fhx_text_part_resolve): the rows whose first byte
// lies in this text - from byte `skip` on (the head of a text that begins inside a row belongs to the rank before) plus `extra`, the rest
// of the last row (the head of the next rank's text).
int fhx_ingest_contacts_text_own(fhx_ctx* ctx, const fhx_text* text, int32_t n_threads, int64_t skip, const char* extra, int64_t extra_bytes,
                                 int64_t* n_rows, int32_t* n_names) {
    if (!ctx || !text || !n_rows || !n_names || skip < 0 || skip > text->bytes || extra_bytes < 0 || (extra_bytes > 0 && !extra))
        return FHX_ERR_ARG;
    std::vector<std::pair<const char*, size_t>> spans;
    int64_t base = 0;
    for (const fhx::TextPiece& piece : text->pieces) {
        const int64_t n = (int64_t)piece.size(), a = std::max(skip, base);
        if (base + n > a) spans.emplace_back(piece.data() + (a - base), (size_t)(base + n - a));
        base += n;
    }
    if (extra_bytes > 0) spans.emplace_back(extra, (size_t)extra_bytes);
    return ingest_text_spans(ctx, spans, text->bytes - skip + extra_bytes, text->path, n_threads, n_rows, n_names);
}

// The same from the FILE: the compressed bytes are uploaded and the members inflated by the GPU (fhx_inflate.inc), so the
// text exists in HBM only.  *refused: 0 = taken, 1 = the container is not one the device inflates (or a stream it refuses):
// fhx_host_inflate + fhx_ingest_contacts_text may still take the file; 2 = the text is outside the device parser's grammar:
// fhx_host_read_table is the path.
static int ingest_contacts_file_part(fhx_ctx* ctx, const char* path, int32_t n_threads, int32_t part, int32_t n_parts, int64_t* n_rows,
                                     int32_t* n_names, int32_t* refused, int32_t* ends_with_newline);

int fhx_ingest_contacts_file(fhx_ctx* ctx, const char* path, int32_t n_threads, int64_t* n_rows, int32_t* n_names, int32_t* refused) {
    return ingest_contacts_file_part(ctx, path, n_threads, 0, 1, n_rows, n_names, refused, nullptr);
}

// Part `part` of `n_parts` of the file: whole gzip members, the parts cut where the compressed bytes divide evenly - every rank of a
// sharded run takes one, so that the file is inflated and parsed once in all (fhx_ingest_contacts_file by every rank: N times).
// Needs members that carry their size (this library's writers, bgzip) - else *refused = 1 - and rows that do not straddle two
// parts: *ends_with_newline says whether this part's text ends a row (the caller checks it for every part but the last).
int fhx_ingest_contacts_file_slice(fhx_ctx* ctx, const char* path, int32_t n_threads, int32_t part, int32_t n_parts, int64_t* n_rows,
                                   int32_t* n_names, int32_t* refused, int32_t* ends_with_newline) {
    if (n_parts < 1 || part < 0 || part >= n_parts || !ends_with_newline) return FHX_ERR_ARG;
    return ingest_contacts_file_part(ctx, path, n_threads, part, n_parts, n_rows, n_names, refused, ends_with_newline);
}

static int ingest_contacts_file_part(fhx_ctx* ctx, const char* path, int32_t n_threads, int32_t part, int32_t n_parts, int64_t* n_rows,
                                     int32_t* n_names, int32_t* refused, int32_t* ends_with_newline) {
    using namespace fhx::ingest;
    if (!ctx || !path || !n_rows || !n_names || !refused) return FHX_ERR_ARG;
    if (ctx->device < 0) return fail(ctx, FHX_ERR_NO_DEVICE, "host-only context");
    FHX_HIP(hipSetDevice(ctx->device));
    ingest_drop(ctx);
    *n_rows = 0;
    *n_names = 0;
    *refused = 0;
    IngestClock clock{ctx, std::getenv("FHX_TIMING") != nullptr, std::chrono::steady_clock::now(), ""};
    if (n_threads <= 0) n_threads = fhx::usable_cpus();
    fhx::FileBytes gz;
    std::string why;
    {
        const int rc = fhx::io_read_file(path, gz, why);
        if (rc != FHX_OK) return fail(ctx, rc, why);
    }
    std::unique_ptr<fhx_ctx::TextIngest> st(new (std::nothrow) fhx_ctx::TextIngest());
    if (!st) return FHX_ERR_NOMEM;
    fhx::FileBytes view;                                    // (a part: whole members of the mapped file - itself a gzip file)
    if (n_parts > 1) {
        std::vector<fhx::GzMember> members;
        if (!fhx::io_scan_members(gz.data(), gz.size(), members) || members.empty()) {
            *refused = 1;
            return fail(ctx, FHX_ERR_UNSUPPORTED, "the contacts file's gzip members do not carry their sizes: it cannot be cut into parts");
        }
        auto first_at_or_after = [&](size_t byte) {
            size_t k = 0;
            while (k < members.size() && members[k].off < byte) ++k;
            return k;
        };
        const size_t a = first_at_or_after(gz.size() / (size_t)n_parts * (size_t)part + (gz.size() % (size_t)n_parts) * (size_t)part / (size_t)n_parts);
        const size_t b = part + 1 == n_parts ? members.size()
                                             : first_at_or_after(gz.size() / (size_t)n_parts * (size_t)(part + 1) +
                                                                 (gz.size() % (size_t)n_parts) * (size_t)(part + 1) / (size_t)n_parts);
        const size_t off_a = a < members.size() ? members[a].off : gz.size();
        const size_t off_b = b < members.size() ? members[b].off : gz.size();
        view.p = gz.data() + off_a;
        view.n = off_b - off_a;
        if (ends_with_newline) *ends_with_newline = 1;
        if (view.n == 0) {                                  // more parts than members: this one is empty
            ctx->text_ingest = st.release();
            return FHX_OK;
        }
    }
    const fhx::FileBytes& src = n_parts > 1 ? view : gz;
    DeviceScratch tmp;
    unsigned char* d_text = nullptr;
    int64_t T = 0, n_members = 0;
    {
        const int rc = device_inflate(ctx, tmp, src, n_threads, (size_t)BLOCK_BYTES, &d_text, &T, &n_members, why);
        if (rc == FHX_ERR_UNSUPPORTED) {
            *refused = 1;
            if (clock.on) std::fprintf(stderr, "fhx_ingest_contacts_file(%s): refused: %s\n", path, why.c_str());
            return fail(ctx, rc, "the contacts file is inflated on the host: " + why);
        }
        if (rc != FHX_OK) return rc;
    }
    if (clock.on) {
        char b[64];
        std::snprintf(b, sizeof(b), " %lld members:", (long long)n_members);
        clock.report += b;
    }
    clock.mark("file to HBM + inflate + CRC-32");
    if (T == 0) {
        ctx->text_ingest = st.release();
        return FHX_OK;
    }
    if (ends_with_newline) {
        unsigned char last = 0;
        FHX_HIP(hipMemcpyAsync(&last, d_text + T - 1, 1, hipMemcpyDeviceToHost, ctx->stream));
        FHX_HIP(hipStreamSynchronize(ctx->stream));
        *ends_with_newline = last == '\n' ? 1 : 0;
    }
    if ((T + BLOCK_BYTES - 1) / BLOCK_BYTES > 0x7fffffffll) return fail(ctx, FHX_ERR_UNSUPPORTED, "text of more than 32 TB");
    bool grammar = false;
    const int rc = ingest_parse_resident(ctx, tmp, d_text, T, path, clock, st, n_rows, n_names, &grammar);
    if (rc == FHX_ERR_UNSUPPORTED && grammar) *refused = 2;
    return rc;
}

// test hook: a file of size-tagged gzip members inflated by the device decoder, the text copied back (cap bytes at most)
int fhx_debug_inflate_file(fhx_ctx* ctx, const char* path, void* out, int64_t cap, int64_t* n_out) {
    if (!ctx || !path || !n_out || cap < 0 || (cap > 0 && !out)) return FHX_ERR_ARG;
    if (ctx->device < 0) return fail(ctx, FHX_ERR_NO_DEVICE, "host-only context");
    FHX_HIP(hipSetDevice(ctx->device));
    fhx::FileBytes gz;
    std::string why;
    {
        const int rc = fhx::io_read_file(path, gz, why);
        if (rc != FHX_OK) return fail(ctx, rc, why);
    }
    DeviceScratch tmp;
    unsigned char* d_text = nullptr;
    int64_t T = 0, n_members = 0;
    const int rc = device_inflate(ctx, tmp, gz, fhx::usable_cpus(), 16, &d_text, &T, &n_members, why);
    if (rc != FHX_OK) return rc == FHX_ERR_UNSUPPORTED ? fail(ctx, rc, why) : rc;
    *n_out = T;
    if (T > cap) return fail(ctx, FHX_ERR_ARG, "buffer too small for the text");
    if (T) FHX_HIP(hipMemcpy(out, d_text, (size_t)T, hipMemcpyDeviceToHost));
    return FHX_OK;
}

const char* fhx_ingest_contacts_name(const fhx_ctx* ctx, int32_t i) {
    if (!ctx || !ctx->text_ingest || i < 0 || i >= (int32_t)ctx->text_ingest->names.size()) return nullptr;
    return ctx->text_ingest->names[(size_t)i].c_str();
}

static int ingest_contacts_commit_timed(fhx_ctx* ctx, const int32_t* ids, int32_t n_ids, double* t_map, double* t_load);

int fhx_ingest_contacts_commit(fhx_ctx* ctx, const int32_t* ids, int32_t n_ids) {
    const auto t0 = std::chrono::steady_clock::now();
    double t_map = 0, t_load = 0;
    const int rc = ingest_contacts_commit_timed(ctx, ids, n_ids, &t_map, &t_load);       // (its temporaries are freed when it returns)
    if (rc == FHX_OK && std::getenv("FHX_TIMING"))
        std::fprintf(stderr, "fhx_ingest_contacts_commit: names -> ids %.3f s; rows into the engine %.3f s; temporaries freed %.3f s\n", t_map, t_load,
                     std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() - t_map - t_load);
    return rc;
}

static int ingest_contacts_commit_timed(fhx_ctx* ctx, const int32_t* ids, int32_t n_ids, double* t_map, double* t_load) {
    using namespace fhx::ingest;
    const auto t0 = std::chrono::steady_clock::now();
    auto since = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
    if (!ctx) return FHX_ERR_ARG;
    if (!ctx->text_ingest) return fail(ctx, FHX_ERR_ARG, "fhx_ingest_contacts_text has not been called");
    fhx_ctx::TextIngest* st = ctx->text_ingest;
    if (n_ids != (int32_t)st->names.size() || (n_ids > 0 && !ids)) return fail(ctx, FHX_ERR_ARG, "one id per name of the text is required");
    FHX_HIP(hipSetDevice(ctx->device));
    struct Drop {
        fhx_ctx* c;
        ~Drop() { ingest_drop(c); }
    } drop{ctx};
    const int64_t n = st->n_rows;
    const bool fraction = st->fraction;
    std::vector<int32_t> slot_id(TABLE_SLOTS, -1);
    for (int i = 0; i < n_ids; ++i) slot_id[(size_t)st->name_slot[(size_t)i]] = ids[i];
    DeviceScratch tmp;
    int32_t *d_slot_id = nullptr, *d_c1 = nullptr, *d_c2 = nullptr;
    FHX_HIP(tmp.get(&d_slot_id, slot_id.size() * sizeof(int32_t)));
    FHX_HIP(tmp.get(&d_c1, (size_t)std::max<int64_t>(n, 1) * sizeof(int32_t)));
    FHX_HIP(tmp.get(&d_c2, (size_t)std::max<int64_t>(n, 1) * sizeof(int32_t)));
    FHX_HIP(hipMemcpyAsync(d_slot_id, slot_id.data(), slot_id.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    if (n)
        hipLaunchKernelGGL(ti_map_rows, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, (const unsigned int*)st->d_slots,
                           (const int32_t*)d_slot_id, n, d_c1, d_c2);
    FHX_HIP(hipStreamSynchronize(ctx->stream));
    dev_free(st->d_slots);
    *t_map = since();
    // an empty text holds no columns: any valid pointer stands in for them
    const int rc = fhx_load_pairs_device(ctx, d_c1, n ? st->d_mid1 : d_c1, d_c2, n ? st->d_mid2 : d_c1, n ? st->d_count : d_c1, n, nullptr);
    if (rc == FHX_OK) ctx->counts_integral = !fraction;
    *t_load = since() - *t_map;
    return rc;
}

// ---- `fithic --gpus N` without a funnel: every rank parses the file on its own GPU and keeps the rows of its chromosomes ----------
namespace fhx {
namespace ingest {

__global__ __launch_bounds__(256) void ti_slot_counts(const unsigned int* __restrict__ slots, int64_t n, unsigned long long* __restrict__ counts) {
    __shared__ unsigned int h[TABLE_SLOTS];                    // 64 KB: rows by the table slot of their first locus's name
    for (int i = threadIdx.x; i < TABLE_SLOTS; i += 256) h[i] = 0u;
    __syncthreads();
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) atomicAdd(&h[slots[r] & 0xFFFFu], 1u);
    __syncthreads();
    for (int i = threadIdx.x; i < TABLE_SLOTS; i += 256)
        if (h[i]) atomicAdd(&counts[i], (unsigned long long)h[i]);
}

constexpr int SH_TILE = 4096;
// rows kept per tile of SH_TILE rows (keep: the owner of the first locus's name is this rank)
__global__ __launch_bounds__(256) void ti_shard_count(const unsigned int* __restrict__ slots, const unsigned char* __restrict__ slot_mine, int64_t n,
                                                      unsigned int* __restrict__ tile_kept) {
    __shared__ unsigned int acc;
    if (threadIdx.x == 0) acc = 0u;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * SH_TILE;
    unsigned int c = 0;
    for (int i = threadIdx.x; i < SH_TILE; i += 256)
        if (base + i < n && slot_mine[slots[base + i] & 0xFFFFu]) ++c;
    c = (unsigned int)wave_sum_i64((long long)c);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&acc, c);
    __syncthreads();
    if (threadIdx.x == 0) tile_kept[blockIdx.x] = acc;
}

// stable compaction of the kept rows (file order is kept: the significances file is written in it) + their file positions
__global__ __launch_bounds__(256) void ti_shard_compact(const unsigned int* __restrict__ slots, const unsigned char* __restrict__ slot_mine,
                                                        const int32_t* __restrict__ slot_id, const int32_t* __restrict__ mid1,
                                                        const int32_t* __restrict__ mid2, const int32_t* __restrict__ cnt, int64_t n,
                                                        const unsigned long long* __restrict__ tile_off, int32_t* __restrict__ o_c1,
                                                        int32_t* __restrict__ o_m1, int32_t* __restrict__ o_c2, int32_t* __restrict__ o_m2,
                                                        int32_t* __restrict__ o_cnt, long long* __restrict__ o_pos) {
    __shared__ unsigned int wave_base[4];
    __shared__ unsigned int run;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * SH_TILE;
    if (threadIdx.x == 0) run = 0u;
    __syncthreads();
    for (int i0 = 0; i0 < SH_TILE; i0 += 256) {                // 256 consecutive rows per step, in order
        const int64_t r = base + i0 + threadIdx.x;
        unsigned int s = 0;
        bool keep = false;
        if (r < n) {
            s = slots[r];
            keep = slot_mine[s & 0xFFFFu] != 0;
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wave_base[wave] = (unsigned int)__popcll(m);
        __syncthreads();
        unsigned int before = run;
        for (int w = 0; w < wave; ++w) before += wave_base[w];
        const unsigned int total = wave_base[0] + wave_base[1] + wave_base[2] + wave_base[3];
        if (keep) {
            const unsigned long long at = tile_off[blockIdx.x] + before + (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
            o_c1[at] = slot_id[s & 0xFFFFu];
            o_c2[at] = slot_id[s >> 16];
            o_m1[at] = mid1[r];
            o_m2[at] = mid2[r];
            o_cnt[at] = cnt[r];
            o_pos[at] = r;
        }
        __syncthreads();
        if (threadIdx.x == 0) run += total;
        __syncthreads();
    }
}

// starts of the maximal stretches of consecutive file positions among the local rows
__global__ void ti_segment_heads(const long long* __restrict__ pos, int64_t n, unsigned long long* __restrict__ n_heads, long long* __restrict__ heads,
                                 int64_t cap) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        if (i == 0 || pos[i] != pos[i - 1] + 1) {
            const unsigned long long k = atomicAdd(n_heads, 1ull);
            if ((int64_t)k < cap) heads[k] = i;
        }
}

}  // namespace ingest
}  // namespace fhx

int fhx_ingest_contacts_chr_counts(fhx_ctx* ctx, int64_t* counts, int32_t n_names) {
    using namespace fhx::ingest;
    if (!ctx || !counts) return FHX_ERR_ARG;
    if (!ctx->text_ingest) return fail(ctx, FHX_ERR_ARG, "fhx_ingest_contacts_text has not been called");
    fhx_ctx::TextIngest* st = ctx->text_ingest;
    if (n_names != (int32_t)st->names.size()) return fail(ctx, FHX_ERR_ARG, "one count per name of the text is required");
    FHX_HIP(hipSetDevice(ctx->device));
    DeviceScratch tmp;
    unsigned long long* d_counts = nullptr;
    FHX_HIP(tmp.get(&d_counts, (size_t)TABLE_SLOTS * sizeof(unsigned long long)));
    FHX_HIP(hipMemsetAsync(d_counts, 0, (size_t)TABLE_SLOTS * sizeof(unsigned long long), ctx->stream));
    if (st->n_rows)
        hipLaunchKernelGGL(ti_slot_counts, dim3(grid_for(st->n_rows, 256 * 16, 1024)), dim3(256), 0, ctx->stream, (const unsigned int*)st->d_slots,
                           st->n_rows, d_counts);
    FHX_HIP(hipGetLastError());
    std::vector<unsigned long long> h((size_t)TABLE_SLOTS);
    FHX_HIP(hipMemcpyAsync(h.data(), d_counts, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < n_names; ++i) counts[i] = (int64_t)h[(size_t)st->name_slot[(size_t)i]];
    return FHX_OK;
}

int fhx_ingest_contacts_commit_shard(fhx_ctx* ctx, const int32_t* ids, const uint8_t* mine, int32_t n_ids, int64_t* n_kept_out) {
    using namespace fhx::ingest;
    if (!ctx) return FHX_ERR_ARG;
    if (!ctx->text_ingest) return fail(ctx, FHX_ERR_ARG, "fhx_ingest_contacts_text has not been called");
    fhx_ctx::TextIngest* st = ctx->text_ingest;
    if (n_ids != (int32_t)st->names.size() || (n_ids > 0 && (!ids || !mine))) return fail(ctx, FHX_ERR_ARG, "one id and one flag per name of the text is required");
    FHX_HIP(hipSetDevice(ctx->device));
    struct Drop {
        fhx_ctx* c;
        ~Drop() { ingest_drop(c); }
    } drop{ctx};
    const int64_t n = st->n_rows;
    const bool fraction = st->fraction;        // (of any row of the text, kept here or not)
    std::vector<int32_t> slot_id(TABLE_SLOTS, -1);
    std::vector<unsigned char> slot_mine(TABLE_SLOTS, 0);
    for (int i = 0; i < n_ids; ++i) {
        slot_id[(size_t)st->name_slot[(size_t)i]] = ids[i];
        slot_mine[(size_t)st->name_slot[(size_t)i]] = mine[i] ? 1 : 0;
    }
    const int64_t tiles = std::max<int64_t>(1, (n + SH_TILE - 1) / SH_TILE);
    DeviceScratch tmp;
    int32_t* d_slot_id = nullptr;
    unsigned char* d_slot_mine = nullptr;
    unsigned int* d_tile_kept = nullptr;
    unsigned long long* d_tile_off = nullptr;
    FHX_HIP(tmp.get(&d_slot_id, slot_id.size() * sizeof(int32_t)));
    FHX_HIP(tmp.get(&d_slot_mine, slot_mine.size()));
    FHX_HIP(tmp.get(&d_tile_kept, (size_t)tiles * sizeof(unsigned int)));
    FHX_HIP(tmp.get(&d_tile_off, (size_t)tiles * sizeof(unsigned long long)));
    FHX_HIP(hipMemcpyAsync(d_slot_id, slot_id.data(), slot_id.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    FHX_HIP(hipMemcpyAsync(d_slot_mine, slot_mine.data(), slot_mine.size(), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(ti_shard_count, dim3((unsigned int)tiles), dim3(256), 0, ctx->stream, (const unsigned int*)st->d_slots,
                       (const unsigned char*)d_slot_mine, n, d_tile_kept);
    FHX_HIP(hipGetLastError());
    std::vector<unsigned int> kept((size_t)tiles);
    FHX_HIP(hipMemcpyAsync(kept.data(), d_tile_kept, kept.size() * sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<unsigned long long> off((size_t)tiles);
    unsigned long long total = 0;
    for (int64_t t = 0; t < tiles; ++t) {                     // (tens of thousands of tiles: a host loop)
        off[(size_t)t] = total;
        total += kept[(size_t)t];
    }
    const size_t cap = (size_t)std::max<unsigned long long>(total, 1);
    int32_t* o[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    long long* d_pos = nullptr;
    for (int k = 0; k < 5; ++k) FHX_HIP(tmp.get(&o[k], cap * sizeof(int32_t)));
    FHX_HIP(tmp.get(&d_pos, cap * sizeof(long long)));
    FHX_HIP(hipMemcpyAsync(d_tile_off, off.data(), off.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
    if (n)
        hipLaunchKernelGGL(ti_shard_compact, dim3((unsigned int)tiles), dim3(256), 0, ctx->stream, (const unsigned int*)st->d_slots,
                           (const unsigned char*)d_slot_mine, (const int32_t*)d_slot_id, (const int32_t*)st->d_mid1, (const int32_t*)st->d_mid2,
                           (const int32_t*)st->d_count, n, (const unsigned long long*)d_tile_off, o[0], o[1], o[2], o[3], o[4], d_pos);
    FHX_HIP(hipGetLastError());
    FHX_HIP(hipStreamSynchronize(ctx->stream));
    // the parsed text's columns are no longer needed: give them back before the engine allocates its row arrays
    ingest_drop(ctx);
    int rc = fhx_load_pairs_device(ctx, o[0], o[1], o[2], o[3], o[4], (int64_t)total, nullptr);
    if (rc != FHX_OK) return rc;
    ctx->counts_integral = !fraction;
    // file positions: the -p >= 3 semantics (fhx_set_global_rows), the order of the significances file, the outlier line numbers
    dev_free(ctx->d_grow);
    const size_t gcap = std::max<size_t>(4, ((size_t)total + 3) / 4 * 4);
    FHX_HIP(dev_malloc(&ctx->d_grow, gcap * sizeof(long long)));
    FHX_HIP(hipMemsetAsync(ctx->d_grow, 0, gcap * sizeof(long long), ctx->stream));
    if (total) FHX_HIP(hipMemcpyAsync(ctx->d_grow, d_pos, (size_t)total * sizeof(long long), hipMemcpyDeviceToDevice, ctx->stream));
    FHX_HIP(hipStreamSynchronize(ctx->stream));
    if (n_kept_out) *n_kept_out = (int64_t)total;
    return FHX_OK;
}

namespace fhx {
namespace ingest {
__global__ void ti_iota_i64(long long* __restrict__ v, int64_t n, long long first) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) v[i] = first + i;
}
}  // namespace ingest
}  // namespace fhx

// fhx_set_global_rows for a rank whose rows are ONE stretch of the file: positions first, first + 1, ...
int fhx_set_global_rows_range(fhx_ctx* ctx, int64_t first) {
    using namespace fhx::ingest;
    if (!ctx || first < 0) return FHX_ERR_ARG;
    if (ctx->device < 0) return fail(ctx, FHX_ERR_NO_DEVICE, "host-only context");
    FHX_HIP(hipSetDevice(ctx->device));
    dev_free(ctx->d_grow);
    const int64_t n = ctx->n_rows;
    const size_t cap = std::max<size_t>(4, ((size_t)n + 3) / 4 * 4);
    FHX_HIP(dev_malloc(&ctx->d_grow, cap * sizeof(long long)));
    FHX_HIP(hipMemsetAsync(ctx->d_grow, 0, cap * sizeof(long long), ctx->stream));
    if (n) hipLaunchKernelGGL(ti_iota_i64, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, ctx->d_grow, n, (long long)first);
    FHX_HIP(hipGetLastError());
    FHX_HIP(hipStreamSynchronize(ctx->stream));
    return FHX_OK;
}

int fhx_shard_segments(fhx_ctx* ctx, int64_t* local_start, int64_t* file_start, int64_t* length, int64_t cap, int64_t* n_out) {
    using namespace fhx::ingest;
    if (!ctx || !n_out || cap < 0 || (cap > 0 && (!local_start || !file_start || !length))) return FHX_ERR_ARG;
    if (ctx->device < 0) return fail(ctx, FHX_ERR_NO_DEVICE, "host-only context");
    if (!ctx->d_grow) return fail(ctx, FHX_ERR_ARG, "the rows carry no file positions (fhx_set_global_rows / fhx_ingest_contacts_commit_shard)");
    FHX_HIP(hipSetDevice(ctx->device));
    const int64_t n = ctx->n_rows;
    *n_out = 0;
    if (n == 0) return FHX_OK;
    DeviceScratch tmp;
    unsigned long long* d_n = nullptr;
    long long* d_heads = nullptr;
    FHX_HIP(tmp.get(&d_n, sizeof(unsigned long long)));
    FHX_HIP(tmp.get(&d_heads, (size_t)std::max<int64_t>(cap, 1) * sizeof(long long)));
    FHX_HIP(hipMemsetAsync(d_n, 0, sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(ti_segment_heads, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, (const long long*)ctx->d_grow, n, d_n, d_heads, cap);
    FHX_HIP(hipGetLastError());
    unsigned long long k = 0;
    FHX_HIP(hipMemcpyAsync(&k, d_n, sizeof(k), hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipStreamSynchronize(ctx->stream));
    *n_out = (int64_t)k;
    if ((int64_t)k > cap) return FHX_OK;                       // the caller sees n_out > cap: too many stretches (a file not sorted by chromosome)
    std::vector<long long> heads((size_t)k);
    FHX_HIP(hipMemcpy(heads.data(), d_heads, heads.size() * sizeof(long long), hipMemcpyDeviceToHost));
    std::sort(heads.begin(), heads.end());
    std::vector<long long> pos((size_t)k);
    for (size_t i = 0; i < heads.size(); ++i)
        FHX_HIP(hipMemcpy(&pos[i], ctx->d_grow + heads[i], sizeof(long long), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < heads.size(); ++i) {
        local_start[i] = heads[i];
        file_start[i] = pos[i];
        length[i] = (i + 1 < heads.size() ? heads[i + 1] : n) - heads[i];
    }
    return FHX_OK;
}

int fhx_fetch_pairs(fhx_ctx* ctx, const int64_t* rows, int64_t n, int32_t* chr1, int32_t* mid1, int32_t* chr2, int32_t* mid2, int32_t* count) {
    using namespace fhx::ingest;
    if (!ctx || n < 0 || (n > 0 && (!chr1 || !mid1 || !chr2 || !mid2 || !count))) return FHX_ERR_ARG;
    if (ctx->device < 0) return fail(ctx, FHX_ERR_NO_DEVICE, "host-only context");
    if (!rows && n != ctx->n_rows) return fail(ctx, FHX_ERR_ARG, "without a row list, n must be the number of loaded rows");
    if (n == 0) return FHX_OK;
    FHX_HIP(hipSetDevice(ctx->device));
    if (ctx->d_loc1 && (ctx->tables_dirty || !ctx->d_slot_chr)) {                // slot -> chromosome is built with the bias table
        const int rc = build_slot_tables(ctx);
        if (rc != FHX_OK) return rc;
    }
    if (!ctx->d_loc1 || !ctx->d_slot_chr || (!ctx->nonfixed && !ctx->d_grid) || (ctx->nonfixed && !ctx->d_slot_mid))
        return fail(ctx, FHX_ERR_ARG, "no resident rows");
    DeviceScratch tmp;
    int64_t* d_rows = nullptr;
    int32_t* d_out = nullptr;
    int* d_bad = nullptr;
    if (rows) {
        FHX_HIP(tmp.get(&d_rows, (size_t)n * sizeof(int64_t)));
        FHX_HIP(hipMemcpyAsync(d_rows, rows, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    }
    FHX_HIP(tmp.get(&d_out, (size_t)n * 5 * sizeof(int32_t)));
    FHX_HIP(tmp.get(&d_bad, sizeof(int)));
    FHX_HIP(hipMemsetAsync(d_bad, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(ti_rebuild_rows, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, (const int64_t*)d_rows, n, (int64_t)ctx->n_rows,
                       (const int32_t*)ctx->d_loc1, (const int32_t*)ctx->d_loc2, (const int32_t*)ctx->d_count, (const int16_t*)ctx->d_slot_chr,
                       ctx->nonfixed ? (const int32_t*)ctx->d_slot_mid : (const int32_t*)nullptr, (const fhx::ChrGrid*)ctx->d_grid,
                       (int32_t)ctx->prm.resolution, d_out, d_bad);
    int bad = 0;
    int32_t* dst[5] = {chr1, mid1, chr2, mid2, count};
    for (int k = 0; k < 5; ++k)
        FHX_HIP(hipMemcpyAsync(dst[k], d_out + (size_t)k * n, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipStreamSynchronize(ctx->stream));
    if (bad) return fail(ctx, FHX_ERR_ARG, "a row index outside the loaded rows");
    return FHX_OK;
}

// (the extern "C" block stays open for the rest of fhx_device.hip)
