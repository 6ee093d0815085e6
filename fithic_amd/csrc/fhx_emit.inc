// fhx_emit.inc - the significances file written BY THE GPU (included by fhx_device.hip inside its extern "C" block).
//
// Replaces the output loop of fit_Spline (fithic/fithic.py:1167-1213) for large runs: every emitted row
// "%s\t%d\t%s\t%d\t%d\t%e\t%e\t%e\t%e\t%f\n" is formatted on the device (fhx_fmt.hpp: exact integer arithmetic, the same
// characters as C's printf) from p, q (resident), ExpCC and the two biases (recomputed, k2_extras) and the five identity
// columns of the input file, and DEFLATED on the device into the same container the host writer produces: one gzip member
// per 65 536 rows, each carrying its size in the "FH" extra subfield.  The host only builds the per-member Huffman codes from
// the symbol histograms (2 258 members x 316 counters for C3), patches headers / trailers and writes the bytes.
//
// Deflate on the device.  A general LZ77 match search is pointless here - the text is a table: what repeats is the previous
// row.  Tokens of a row = one match for the longest common prefix with the previous row (chromosome, first midpoint ...),
// then per field either a match against the same field of the previous row (same bias, q = 1.000000e+00 ...) or literals.
// Ratio on real output text: 0.31 (zlib level 1: 0.28, Huffman only: 0.48).  Three passes recompute the tokens from the row
// text staged in LDS (histogram -> bit lengths -> bits); offsets come from workgroup-level scans; a row's bits are written
// with plain stores except its first and last 32-bit word (atomicOr into a zeroed buffer); CRC-32 of a member = XOR over its
// rows of crc(row) advanced by the bytes that follow it (x^(8n) mod p, zlib's crc32_combine algebra).
}  // extern "C"

#include "fhx_cpus.hpp"
#include "fhx_deflate.hpp"
#include "fhx_emitrow.hpp"

namespace fhx {
namespace emit {

constexpr int LDS_STRIDE = 196;                 // 49 words (odd): consecutive rows fall into different LDS banks
constexpr int WG = 256;                         // rows per workgroup
constexpr int MEMBER_ROWS = 65536;              // rows per gzip member
constexpr int WG_PER_MEMBER = MEMBER_ROWS / WG;
constexpr int GZ_HEAD = 24, GZ_TAIL = 8;        // 10 fixed + 2 XLEN + 12 "FH" subfield; CRC32 + ISIZE

__global__ __launch_bounds__(WG) void em_format(Cols C, unsigned char* __restrict__ rowtext, unsigned char* __restrict__ rowlen,
                                                unsigned int* __restrict__ wg_len, int* __restrict__ unsupported,
                                                unsigned long long* __restrict__ rows_emitted) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[WG * LDS_STRIDE];
    __shared__ unsigned int wsum[WG / 64];
    const int64_t r = (int64_t)blockIdx.x * WG + threadIdx.x;
    unsigned char* out = lds + threadIdx.x * LDS_STRIDE;
    int len = 0;
    if (r < C.n_rows) {
        const RowId id = row_identity(C, r);
        if (row_emitted(C, id)) {
            char buf[288];
            const int n = row_text(C, r, id, buf);
            if (n == 0) atomicOr(unsupported, 1);
            len = n;
            for (int k = 0; k < n; ++k) out[k] = (unsigned char)buf[k];
        }
        rowlen[r] = (unsigned char)len;
    }
    // workgroup total (text bytes), then the 32 KB of rows leave LDS coalesced
    unsigned int v = (unsigned int)len;
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) wg_len[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    const unsigned long long some = __ballot(len > 0);
    if ((threadIdx.x & 63) == 0 && some) atomicAdd(rows_emitted, (unsigned long long)__popcll(some));
    const int64_t base = (int64_t)blockIdx.x * WG;
    for (int i = threadIdx.x; i < WG * (ROW_STRIDE / 4); i += WG) {
        const int row = i / (ROW_STRIDE / 4), w = i % (ROW_STRIDE / 4);
        if (base + row < C.n_rows)
            reinterpret_cast<unsigned int*>(rowtext + (base + row) * ROW_STRIDE)[w] = reinterpret_cast<const unsigned int*>(lds + row * LDS_STRIDE)[w];
    }
}

// exclusive scan of the 256 workgroup totals of every member; member totals
__global__ __launch_bounds__(WG_PER_MEMBER) void em_scan_members(const unsigned int* __restrict__ wg_total, int64_t n_wg,
                                                                 unsigned int* __restrict__ wg_off, unsigned int* __restrict__ member_total) {
    __shared__ unsigned int wsum[WG_PER_MEMBER / 64];
    const int64_t i = (int64_t)blockIdx.x * WG_PER_MEMBER + threadIdx.x;
    const unsigned int v = i < n_wg ? wg_total[i] : 0u;
    unsigned int inc = v;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned int up = __shfl_up(inc, s, 64);
        if (lane >= s) inc += up;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    unsigned int base = 0, all = 0;
    for (int k = 0; k < WG_PER_MEMBER / 64; ++k) {
        if (k < w) base += wsum[k];
        all += wsum[k];
    }
    if (i < n_wg) wg_off[i] = base + inc - v;
    if (threadIdx.x == 0) member_total[blockIdx.x] = all;
}

struct DeviceMem {
    static __device__ __forceinline__ void add(unsigned int* p, unsigned int v) { atomicAdd(p, v); }
    static __device__ __forceinline__ void bit_or(unsigned int* p, unsigned int v) { atomicOr(p, v); }
};

// the rows of a workgroup (and the row before its first one, if it belongs to the same member) staged in LDS
struct Stage {
    unsigned char* lds;                        // (WG + 1) rows of LDS_STRIDE; row 0 = the row before the workgroup's first
    __device__ __forceinline__ void load(const unsigned char* rowtext, int64_t n_rows) {
        const int64_t base = (int64_t)blockIdx.x * WG - 1;
        const bool has_before = (blockIdx.x % WG_PER_MEMBER) != 0;
        for (int i = threadIdx.x; i < (WG + 1) * (ROW_STRIDE / 4); i += WG) {
            const int row = i / (ROW_STRIDE / 4), w = i % (ROW_STRIDE / 4);
            const int64_t g = base + row;
            unsigned int v = 0;
            if (g >= 0 && g < n_rows && (row > 0 || has_before)) v = reinterpret_cast<const unsigned int*>(rowtext + g * ROW_STRIDE)[w];
            reinterpret_cast<unsigned int*>(lds + row * LDS_STRIDE)[w] = v;
        }
        __syncthreads();
    }
};

// histogram of the member's symbols + CRC-32 of the member's text
__global__ __launch_bounds__(WG) void em_hist_crc(const unsigned char* __restrict__ rowtext, const unsigned char* __restrict__ rowlen,
                                                  int64_t n_rows, const unsigned int* __restrict__ wg_off,
                                                  const unsigned int* __restrict__ member_text, const unsigned int* __restrict__ crc_table,
                                                  const unsigned int* __restrict__ x2n_table, unsigned int* __restrict__ hist,
                                                  unsigned int* __restrict__ member_crc) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[(WG + 1) * LDS_STRIDE];
    __shared__ unsigned int h[N_SYM];
    __shared__ unsigned int tab[256];
    __shared__ unsigned int wsum[WG / 64];
    __shared__ unsigned int wxor[WG / 64];
    for (int i = threadIdx.x; i < N_SYM; i += WG) h[i] = 0;
    tab[threadIdx.x] = crc_table[threadIdx.x];
    Stage st{lds};
    st.load(rowtext, n_rows);
    const int64_t r = (int64_t)blockIdx.x * WG + threadIdx.x;
    const int member = blockIdx.x / WG_PER_MEMBER;
    const int lc = r < n_rows ? rowlen[r] : 0;
    const int lp = (threadIdx.x > 0 || (blockIdx.x % WG_PER_MEMBER) != 0) ? (r >= 1 && r - 1 < n_rows ? rowlen[r - 1] : 0) : 0;
    const unsigned char* cur = lds + (threadIdx.x + 1) * LDS_STRIDE;
    const unsigned char* prev = lds + threadIdx.x * LDS_STRIDE;
    if (lc > 0) {
        HistSink<DeviceMem> S{h};
        tokenise(cur, lc, prev, lp, S);
    }
    // position of the row inside the member's text: workgroup offset + ordered scan of the lengths
    unsigned int inc = (unsigned int)lc;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned int up = __shfl_up(inc, s, 64);
        if (lane >= s) inc += up;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    unsigned int before = wg_off[blockIdx.x] + inc - (unsigned int)lc;
    for (int k = 0; k < w; ++k) before += wsum[k];
    unsigned int part = 0;
    if (lc > 0) {
        unsigned int c = 0xffffffffu;
        for (int k = 0; k < lc; ++k) c = tab[(c ^ cur[k]) & 0xffu] ^ (c >> 8);
        c ^= 0xffffffffu;
        // advance by the bytes that follow this row in the member: multiply by x^(8 n) mod p (zlib x2nmodp(n, 3))
        unsigned long long n = (unsigned long long)member_text[member] - before - (unsigned int)lc;
        unsigned int op = 1u << 31;
        unsigned int k = 3;
        while (n) {
            if (n & 1ull) op = crc_multmodp(x2n_table[k & 31u], op);
            n >>= 1;
            ++k;
        }
        part = crc_multmodp(op, c);
    }
    for (int s = 32; s >= 1; s >>= 1) part ^= __shfl_xor(part, s, 64);
    if (lane == 0) wxor[w] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int x = wxor[0] ^ wxor[1] ^ wxor[2] ^ wxor[3];
        if (x) atomicXor(&member_crc[member], x);
    }
    for (int i = threadIdx.x; i < N_SYM; i += WG)
        if (h[i]) atomicAdd(&hist[(size_t)member * N_SYM + i], h[i]);
}

__global__ __launch_bounds__(WG) void em_bits(const unsigned char* __restrict__ rowtext, const unsigned char* __restrict__ rowlen,
                                              int64_t n_rows, const CodeTab* __restrict__ codes, unsigned int* __restrict__ wg_bits) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[(WG + 1) * LDS_STRIDE];
    __shared__ unsigned char clen[N_SYM];
    __shared__ unsigned int wsum[WG / 64];
    const int member = blockIdx.x / WG_PER_MEMBER;
    for (int i = threadIdx.x; i < N_SYM; i += WG) clen[i] = codes[member].len[i];
    Stage st{lds};
    st.load(rowtext, n_rows);
    const int64_t r = (int64_t)blockIdx.x * WG + threadIdx.x;
    const int lc = r < n_rows ? rowlen[r] : 0;
    const int lp = (threadIdx.x > 0 || (blockIdx.x % WG_PER_MEMBER) != 0) ? (r >= 1 && r - 1 < n_rows ? rowlen[r - 1] : 0) : 0;
    BitsSink S{clen, 0u};
    if (lc > 0) tokenise(lds + (threadIdx.x + 1) * LDS_STRIDE, lc, lds + threadIdx.x * LDS_STRIDE, lp, S);
    unsigned int v = S.bits;
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) wg_bits[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// member_bit0[m] = bit position (in the output buffer) of the first token of member m, i.e. after its gzip header and its
// deflate block header
__global__ __launch_bounds__(WG) void em_encode(const unsigned char* __restrict__ rowtext, const unsigned char* __restrict__ rowlen,
                                                int64_t n_rows, const CodeTab* __restrict__ codes, const unsigned int* __restrict__ wg_bitoff,
                                                const unsigned long long* __restrict__ member_bit0, unsigned int* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[(WG + 1) * LDS_STRIDE];
    __shared__ unsigned short ccode[N_SYM];
    __shared__ unsigned char clen[N_SYM];
    __shared__ unsigned int wsum[WG / 64];
    const int member = blockIdx.x / WG_PER_MEMBER;
    for (int i = threadIdx.x; i < N_SYM; i += WG) {
        ccode[i] = codes[member].code[i];
        clen[i] = codes[member].len[i];
    }
    Stage st{lds};
    st.load(rowtext, n_rows);
    const int64_t r = (int64_t)blockIdx.x * WG + threadIdx.x;
    const int lc = r < n_rows ? rowlen[r] : 0;
    const int lp = (threadIdx.x > 0 || (blockIdx.x % WG_PER_MEMBER) != 0) ? (r >= 1 && r - 1 < n_rows ? rowlen[r - 1] : 0) : 0;
    const unsigned char* cur = lds + (threadIdx.x + 1) * LDS_STRIDE;
    const unsigned char* prev = lds + threadIdx.x * LDS_STRIDE;
    BitsSink B{clen, 0u};
    if (lc > 0) tokenise(cur, lc, prev, lp, B);
    unsigned int inc = B.bits;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned int up = __shfl_up(inc, s, 64);
        if (lane >= s) inc += up;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    unsigned long long at = member_bit0[member] + wg_bitoff[blockIdx.x] + inc - B.bits;
    for (int k = 0; k < w; ++k) at += wsum[k];
    if (lc > 0) {
        EncodeSink<DeviceMem> E{ccode, clen, out, 0ull, (int)(at & 31ull), at >> 5, true};
        tokenise(cur, lc, prev, lp, E);
        E.finish();
    }
}

// per member: the gzip header (with the member's size in the "FH" subfield), the deflate block header (bits prepared by the
// host) in front of the tokens, the end-of-block code behind them, CRC-32 and ISIZE
__device__ __forceinline__ void or_byte(unsigned int* out, unsigned long long byte_at, unsigned int v) {
    if (v) atomicOr(&out[byte_at >> 2], v << (8u * (unsigned int)(byte_at & 3ull)));
}
__global__ void em_frame(int n_members, const unsigned char* __restrict__ hdr_bits, const unsigned int* __restrict__ hdr_off,
                         const unsigned int* __restrict__ hdr_nbits, const unsigned long long* __restrict__ member_bit0,
                         const unsigned int* __restrict__ member_bits, const CodeTab* __restrict__ codes,
                         const unsigned long long* __restrict__ member_start, const unsigned int* __restrict__ member_crc,
                         const unsigned int* __restrict__ member_text, unsigned int* __restrict__ out) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_members || hdr_nbits[m] == 0xFFFFFFFFu) return;            // 0xFFFFFFFF: no emitted row, no member
    const unsigned long long start = member_start[m], size = member_start[m + 1] - start;
    const unsigned char head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 255, 12, 0, 'F', 'H', 8, 0};
    for (int k = 0; k < 16; ++k) or_byte(out, start + k, head[k]);
    for (int k = 0; k < 8; ++k) or_byte(out, start + 16 + k, (unsigned int)((size >> (8 * k)) & 0xFF));
    const unsigned int crc = member_crc[m], isize = member_text[m];
    for (int k = 0; k < 4; ++k) {
        or_byte(out, start + size - 8 + k, (crc >> (8 * k)) & 0xFF);
        or_byte(out, start + size - 4 + k, (isize >> (8 * k)) & 0xFF);
    }
    unsigned long long at = member_bit0[m] - hdr_nbits[m];
    const unsigned char* src = hdr_bits + hdr_off[m];
    for (unsigned int k = 0; k < hdr_nbits[m]; k += 8) {
        const unsigned int nb = hdr_nbits[m] - k < 8 ? hdr_nbits[m] - k : 8;
        const unsigned long long v = (unsigned long long)(src[k >> 3] & ((1u << nb) - 1u)) << (at & 31ull);
        atomicOr(&out[at >> 5], (unsigned int)v);
        if (v >> 32) atomicOr(&out[(at >> 5) + 1], (unsigned int)(v >> 32));
        at += nb;
    }
    at = member_bit0[m] + member_bits[m];
    const unsigned long long v = (unsigned long long)codes[m].code[256] << (at & 31ull);       // end of block
    atomicOr(&out[at >> 5], (unsigned int)v);
    if (v >> 32) atomicOr(&out[(at >> 5) + 1], (unsigned int)(v >> 32));
}

// test hook: the device formatter on arbitrary doubles (32 bytes per value: the characters, zero padded; len < 0 = not covered)
__global__ void em_debug_format(const double* __restrict__ v, int64_t n, int kind, char* __restrict__ text, int* __restrict__ len) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        char buf[400];
        const int w = kind == 0 ? fmt::fmt_e6(v[i], buf) : fmt::fmt_f6(v[i], buf);
        len[i] = w;
        for (int k = 0; k < 32; ++k) text[i * 32 + k] = (w > 0 && k < w) ? buf[k] : (char)0;
    }
}

}  // namespace emit
}  // namespace fhx

// two pinned buffers through which finished members leave the device and the contacts file enters it; pinning 128 MB takes
// tens of milliseconds, so the pair is made once per context (pinned_pair) and freed with it
struct FhxPinnedPair {
    static constexpr size_t kChunk = (size_t)64 << 20;
    void* p[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipError_t init() {
        for (int k = 0; k < 2; ++k) {
            hipError_t e = hipHostMalloc(&p[k], kChunk, hipHostMallocDefault);
            if (e != hipSuccess) return e;
            e = hipEventCreateWithFlags(&ev[k], hipEventDisableTiming);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    ~FhxPinnedPair() {
        for (int k = 0; k < 2; ++k) {
            if (p[k]) (void)hipHostFree(p[k]);
            if (ev[k]) (void)hipEventDestroy(ev[k]);
        }
    }
};
void fhx_pinned_pair_free(FhxPinnedPair* p) { delete p; }

namespace {

typedef FhxPinnedPair EmitPinned;

// the context's pair, made on first use (the caller has selected the device); nullptr + *err on failure
EmitPinned* pinned_pair(fhx_ctx* ctx, hipError_t* err) {
    *err = hipSuccess;
    if (!ctx->pinned) {
        EmitPinned* p = new (std::nothrow) EmitPinned();
        if (!p) {
            *err = hipErrorOutOfMemory;
            return nullptr;
        }
        *err = p->init();
        if (*err != hipSuccess) {
            delete p;
            return nullptr;
        }
        ctx->pinned = p;
    }
    return ctx->pinned;
}

// The copy-out of finished batches, on a thread and a stream of its own: while batch k leaves through the two pinned buffers
// and fwrite, the kernels of batch k + 1 run.  At most one batch waits behind the one in flight.
struct EmitDrainer {
    struct Item {
        unsigned char* d_out;
        size_t bytes, cap;
    };
    ScratchPool* pool;
    fhx_ctx* ctx;
    std::FILE* f;
    EmitPinned* pin;
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Item> q;
    bool closing = false, busy = false;
    int rc = FHX_OK;
    std::string err;
    double seconds = 0;
    EmitDrainer(fhx_ctx* c, std::FILE* file, EmitPinned* p, ScratchPool* sp) : pool(sp), ctx(c), f(file), pin(p) { th = std::thread([this] { run(); }); }
    ~EmitDrainer() { (void)finish(); }
    void fail_with(int code, const std::string& what) {
        std::lock_guard<std::mutex> g(mu);
        if (rc == FHX_OK) {
            rc = code;
            err = what;
        }
    }
    // (Round 6 measured what limits this loop at C5 scale - 41.7 GB in 5.9-6.0 s = 7 GB/s, profiles/r06/cli_c5.txt: not the one
    // thread in fwrite.  Several threads in pwrite() on the one file were slower (10.5 s with 6, 14.4 s with 3: a write holds the
    // file's inode lock for its whole copy); a shared mapping of the batch's stretch of the file filled by 4-16 threads took
    // 5.9-7.3 s (every fresh 4 KB page of a tmpfs file is a fault that allocates and zero-fills it).  Inserting pages into ONE
    // file's page cache is what runs at 7 GB/s on this box, whoever copies; the loop stays the plain one.)
    void drain(const Item& it, hipStream_t stream) {
        const size_t chunk = EmitPinned::kChunk;
        const size_t n_chunks = (it.bytes + chunk - 1) / chunk;
        auto issue = [&](size_t c) -> hipError_t {
            const size_t lo = c * chunk, n = std::min(chunk, it.bytes - lo);
            hipError_t e = hipMemcpyAsync(pin->p[c & 1], it.d_out + lo, n, hipMemcpyDeviceToHost, stream);
            return e != hipSuccess ? e : hipEventRecord(pin->ev[c & 1], stream);
        };
        hipError_t e = n_chunks ? issue(0) : hipSuccess;
        for (size_t c = 0; c < n_chunks && e == hipSuccess; ++c) {
            e = hipEventSynchronize(pin->ev[c & 1]);
            if (e == hipSuccess && c + 1 < n_chunks) e = issue(c + 1);
            const size_t lo = c * chunk, n = std::min(chunk, it.bytes - lo);
            if (e == hipSuccess && std::fwrite(pin->p[c & 1], 1, n, f) != n) {
                fail_with(FHX_ERR_ARG, "write error");
                break;
            }
        }
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) fail_with(FHX_ERR_HIP, std::string("copy of the output to the host: ") + hipGetErrorString(e));
    }
    void run() {
        hipStream_t stream = nullptr;
        if (hipSetDevice(ctx->device) != hipSuccess || hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) {
            fail_with(FHX_ERR_HIP, "no stream for the copy-out");
            stream = nullptr;
        }
        for (;;) {
            Item it;
            {
                std::unique_lock<std::mutex> g(mu);
                cv.wait(g, [&] { return closing || !q.empty(); });
                if (q.empty()) break;
                it = q.front();
                q.pop_front();
                busy = true;
            }
            const auto t0 = std::chrono::steady_clock::now();
            bool ok;
            {
                std::lock_guard<std::mutex> g(mu);
                ok = rc == FHX_OK;
            }
            if (ok && stream) drain(it, stream);
            pool->give(it.d_out, it.cap);
            {
                std::lock_guard<std::mutex> g(mu);
                seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                busy = false;
            }
            cv.notify_all();
        }
        if (stream) (void)hipStreamDestroy(stream);
    }
    // takes ownership of d_out; waits while another batch is already queued
    void push(unsigned char* d_out, size_t bytes, size_t cap) {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return q.empty(); });
        q.push_back(Item{d_out, bytes, cap});
        g.unlock();
        cv.notify_all();
    }
    int finish() {
        if (th.joinable()) {
            {
                std::lock_guard<std::mutex> g(mu);
                closing = true;
            }
            cv.notify_all();
            th.join();
        }
        return rc;
    }
};

// rows [r0, r0 + n_rows) of the context -> gzip members appended to f.  All device buffers of a call are sized by the batch.
static int write_significances_batch(fhx_ctx* ctx, std::FILE* f, const std::vector<char>& blob, const std::vector<int32_t>& name_off,
                                     int32_t n_names, const int32_t* const* h_col /* 5 host columns at r0, or all null */, bool derive,
                                     int64_t r0, int64_t n_rows, EmitDrainer* drainer, ScratchPool* pool, int64_t* rows_acc, int64_t* bytes_acc) {
    using namespace fhx::emit;
    // FHX_TIMING=1: stage clocks on stderr (each mark synchronises the stream, so the run is slightly slower)
    const bool timing = std::getenv("FHX_TIMING") != nullptr;
    auto clock_now = [] { return std::chrono::steady_clock::now(); };
    auto t_last = clock_now();
    std::string t_report;
    auto mark = [&](const char* what) {
        if (!timing) return;
        (void)hipStreamSynchronize(ctx->stream);
        const auto t = clock_now();
        char b[96];
        std::snprintf(b, sizeof(b), " %s %.3f s;", what, std::chrono::duration<double>(t - t_last).count());
        t_report += b;
        t_last = t;
    };

    const int64_t n_wg = (n_rows + WG - 1) / WG;
    const int n_members = (int)((n_rows + MEMBER_ROWS - 1) / MEMBER_ROWS);
    DeviceScratch G(pool);                              // back to the pool on every path
    int32_t* d_col[5];
    double *d_b1 = nullptr, *d_b2 = nullptr, *d_e = nullptr;
    char* d_names = nullptr;
    int32_t* d_name_off = nullptr;
    unsigned char *d_text = nullptr, *d_len = nullptr;
    unsigned int *d_wg_a = nullptr, *d_wg_off = nullptr, *d_member_a = nullptr, *d_hist = nullptr, *d_crc = nullptr, *d_tab = nullptr, *d_x2n = nullptr;
    int* d_flag = nullptr;
    unsigned long long* d_rows = nullptr;
    const size_t bytes8 = (size_t)n_rows * sizeof(double);
    for (int k = 0; k < 5; ++k) {
        d_col[k] = nullptr;
        if (derive) continue;
        FHX_HIP(G.get(&d_col[k], (size_t)n_rows * 4));
        FHX_HIP(hipMemcpyAsync(d_col[k], h_col[k], (size_t)n_rows * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    FHX_HIP(G.get(&d_b1, bytes8));
    FHX_HIP(G.get(&d_b2, bytes8));
    FHX_HIP(G.get(&d_e, bytes8));
    FHX_HIP(G.get(&d_names, blob.size()));
    FHX_HIP(G.get(&d_name_off, name_off.size() * 4));
    FHX_HIP(G.get(&d_text, (size_t)n_wg * WG * ROW_STRIDE));
    FHX_HIP(G.get(&d_len, (size_t)n_wg * WG));
    FHX_HIP(G.get(&d_wg_a, (size_t)n_wg * 4));
    FHX_HIP(G.get(&d_wg_off, (size_t)n_wg * 4));
    FHX_HIP(G.get(&d_member_a, (size_t)n_members * 4));
    FHX_HIP(G.get(&d_hist, (size_t)n_members * N_SYM * 4));
    FHX_HIP(G.get(&d_crc, (size_t)n_members * 4));
    FHX_HIP(G.get(&d_tab, 256 * 4));
    FHX_HIP(G.get(&d_x2n, 32 * 4));
    FHX_HIP(G.get(&d_flag, 4));
    FHX_HIP(G.get(&d_rows, 8));
    FHX_HIP(hipMemcpyAsync(d_names, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream));
    FHX_HIP(hipMemcpyAsync(d_name_off, name_off.data(), name_off.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    FHX_HIP(hipMemsetAsync(d_flag, 0, 4, ctx->stream));
    FHX_HIP(hipMemsetAsync(d_rows, 0, 8, ctx->stream));
    FHX_HIP(hipMemsetAsync(d_len, 0, (size_t)n_wg * WG, ctx->stream));
    FHX_HIP(hipMemsetAsync(d_hist, 0, (size_t)n_members * N_SYM * 4, ctx->stream));
    FHX_HIP(hipMemsetAsync(d_crc, 0, (size_t)n_members * 4, ctx->stream));
    {
        unsigned int tab[256], x2n[32];
        for (unsigned int i = 0; i < 256; ++i) {
            unsigned int c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
            tab[i] = c;
        }
        auto multmodp = [](unsigned int a, unsigned int b) {
            unsigned int m = 1u << 31, p = 0;
            for (;;) {
                if (a & m) {
                    p ^= b;
                    if ((a & (m - 1)) == 0) break;
                }
                m >>= 1;
                b = (b & 1u) ? (b >> 1) ^ 0xedb88320u : b >> 1;
            }
            return p;
        };
        unsigned int p = 1u << 30;                       // x^1
        x2n[0] = p;
        for (int k = 1; k < 32; ++k) x2n[k] = p = multmodp(p, p);
        FHX_HIP(hipMemcpyAsync(d_tab, tab, sizeof(tab), hipMemcpyHostToDevice, ctx->stream));
        FHX_HIP(hipMemcpyAsync(d_x2n, x2n, sizeof(x2n), hipMemcpyHostToDevice, ctx->stream));
        FHX_HIP(hipStreamSynchronize(ctx->stream));      // the stack tables go out of scope
    }
    mark(derive ? "setup" : "upload of the 5 identity columns");
    // ExpCC and the biases as the writer prints them (fithic.py:1075-1078, :1105-1108)
    K2Params P = make_k2_params(ctx);
    P.loc1 += r0;
    P.loc2 += r0;
    P.count += r0;
    P.n = n_rows;
    launch_k2_extras(ctx, P, n_rows, d_e, d_b1, d_b2);
    // the batch's rows of the resident columns; the five identity columns are the uploaded ones unless they are rebuilt (all null)
    Cols C = resident_cols(ctx, d_names, d_name_off, n_names);
    C.chr1 = d_col[0];
    C.mid1 = d_col[1];
    C.chr2 = d_col[2];
    C.mid2 = d_col[3];
    C.count = derive ? ctx->d_count + r0 : d_col[4];
    C.loc1 += r0;
    C.loc2 += r0;
    C.p += r0;
    C.q += r0;
    C.b1 = d_b1;
    C.b2 = d_b2;
    C.expcc = d_e;
    C.n_rows = n_rows;
    hipLaunchKernelGGL(em_format, dim3((unsigned)n_wg), dim3(WG), 0, ctx->stream, C, d_text, d_len, d_wg_a, d_flag, d_rows);
    hipLaunchKernelGGL(em_scan_members, dim3(n_members), dim3(WG_PER_MEMBER), 0, ctx->stream, (const unsigned int*)d_wg_a, n_wg, d_wg_off, d_member_a);
    hipLaunchKernelGGL(em_hist_crc, dim3((unsigned)n_wg), dim3(WG), 0, ctx->stream, (const unsigned char*)d_text, (const unsigned char*)d_len, n_rows,
                       (const unsigned int*)d_wg_off, (const unsigned int*)d_member_a, (const unsigned int*)d_tab, (const unsigned int*)d_x2n, d_hist, d_crc);
    FHX_HIP(hipGetLastError());
    mark("ExpCC/bias + format + histograms/CRC");
    int h_flag = 0;
    std::vector<unsigned int> h_hist((size_t)n_members * N_SYM), h_crc(n_members), h_text(n_members);
    FHX_HIP(hipMemcpyAsync(&h_flag, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipMemcpyAsync(h_hist.data(), d_hist, h_hist.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipMemcpyAsync(h_crc.data(), d_crc, h_crc.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipMemcpyAsync(h_text.data(), d_member_a, h_text.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipStreamSynchronize(ctx->stream));
    if (h_flag)
        return fail(ctx, FHX_ERR_UNSUPPORTED, "a row does not fit the device formatter (name longer than 24 bytes, |ExpCC| >= 2^63, or a row "
                                              "of 192 bytes or more): use the host writer");
    // ---- codes, headers and the layout of the output (host threads over members) --------------------------------------------
    std::vector<CodeTab> codes(n_members);
    std::vector<BitString> hdrs(n_members);
    std::vector<unsigned int> hdr_off(n_members), hdr_nbits(n_members), member_bits(n_members);
    std::vector<unsigned long long> member_bit0(n_members), member_start(n_members + 1);
    {
        const int n_threads = std::min(32, fhx::usable_cpus());
        std::atomic<int> next{0};
        auto work = [&]() {
            std::vector<unsigned long long> lf(N_LIT), df(N_DIST);
            std::vector<unsigned char> ll, dl;
            std::vector<unsigned short> lc, dc;
            for (;;) {
                const int m = next.fetch_add(1);
                if (m >= n_members) return;
                if (h_text[m] == 0) continue;                    // no emitted row in these 65 536 rows: no member at all
                for (int s = 0; s < N_LIT; ++s) lf[s] = h_hist[(size_t)m * N_SYM + s];
                for (int s = 0; s < N_DIST; ++s) df[s] = h_hist[(size_t)m * N_SYM + N_LIT + s];
                lf[256] = 1;                                     // end of block
                package_merge(lf, 15, ll);
                package_merge(df, 15, dl);
                bool any_dist = false;
                for (unsigned char l : dl) any_dist = any_dist || l;
                if (!any_dist) dl[0] = 1;                        // RFC 1951: one distance code of one bit when no match occurs
                canonical_codes(ll, lc);
                canonical_codes(dl, dc);
                for (int s = 0; s < N_LIT; ++s) {
                    codes[m].code[s] = lc[s];
                    codes[m].len[s] = ll[s];
                }
                for (int s = 0; s < N_DIST; ++s) {
                    codes[m].code[N_LIT + s] = dc[s];
                    codes[m].len[N_LIT + s] = dl[s];
                }
                block_header(ll, dl, hdrs[m]);
                unsigned long long bits = 0;
                for (int s = 0; s < 256; ++s) bits += lf[s] * ll[s];
                for (int s = 257; s < N_LIT; ++s) bits += lf[s] * (ll[s] + kLenExtra[s - 257]);
                for (int s = 0; s < N_DIST; ++s) bits += df[s] * (dl[s] + kDistExtra[s]);
                member_bits[m] = (unsigned int)bits;
            }
        };
        std::vector<std::thread> pool;
        for (int t = 1; t < n_threads; ++t) pool.emplace_back(work);
        work();
        for (auto& t : pool) t.join();
    }
    mark("Huffman codes on the host");
    std::vector<unsigned char> hdr_blob;
    unsigned long long at = 0;                           // bytes; members follow each other without gaps: the buffer IS the file
    for (int m = 0; m < n_members; ++m) {
        member_start[m] = at;
        hdr_off[m] = (unsigned int)hdr_blob.size();
        if (h_text[m] == 0) {
            hdr_nbits[m] = 0xFFFFFFFFu;                  // tells em_frame to skip it
            member_bit0[m] = at * 8;
            continue;
        }
        hdr_nbits[m] = hdrs[m].nbits;
        hdr_blob.insert(hdr_blob.end(), hdrs[m].bytes.begin(), hdrs[m].bytes.end());
        member_bit0[m] = (at + GZ_HEAD) * 8 + hdrs[m].nbits;
        const unsigned long long deflate_bits = (unsigned long long)hdrs[m].nbits + member_bits[m] + codes[m].len[256];
        at += GZ_HEAD + (deflate_bits + 7) / 8 + GZ_TAIL;
    }
    member_start[n_members] = at;
    const unsigned long long out_bytes = at;
    if (hdr_blob.empty()) hdr_blob.push_back(0);
    // ---- encode -------------------------------------------------------------------------------------------------------
    CodeTab* d_codes = nullptr;
    unsigned char* d_hdr = nullptr;
    unsigned int *d_hdr_off = nullptr, *d_hdr_nbits = nullptr, *d_member_bits = nullptr, *d_member_bitsum = nullptr, *d_wg_bitoff = nullptr, *d_out = nullptr;
    unsigned long long *d_bit0 = nullptr, *d_start = nullptr;
    FHX_HIP(G.get(&d_codes, codes.size() * sizeof(CodeTab)));
    FHX_HIP(G.get(&d_hdr, hdr_blob.size()));
    FHX_HIP(G.get(&d_hdr_off, (size_t)n_members * 4));
    FHX_HIP(G.get(&d_hdr_nbits, (size_t)n_members * 4));
    FHX_HIP(G.get(&d_member_bits, (size_t)n_members * 4));
    FHX_HIP(G.get(&d_member_bitsum, (size_t)n_members * 4));
    FHX_HIP(G.get(&d_wg_bitoff, (size_t)n_wg * 4));
    FHX_HIP(G.get(&d_bit0, (size_t)n_members * 8));
    FHX_HIP(G.get(&d_start, (size_t)(n_members + 1) * 8));
    size_t out_cap = (size_t)out_bytes + 16;                           // leaves with the drainer, which hands it back to the pool
    {
        size_t real = 0;
        if (void* q = pool->take(out_cap, &real)) {
            d_out = (unsigned int*)q;
            out_cap = real;
        } else {
            out_cap += out_cap / 16;                                       // the next batch's output may be a little larger
            FHX_HIP(dev_malloc(&d_out, out_cap));
        }
    }
    struct OutGuard {
        unsigned int* p;
        size_t cap;
        ScratchPool* pool;
        ~OutGuard() {
            if (p) pool->give(p, cap);
        }
    } out_guard{d_out, out_cap, pool};
    FHX_HIP(hipMemcpyAsync(d_codes, codes.data(), codes.size() * sizeof(CodeTab), hipMemcpyHostToDevice, ctx->stream));
    FHX_HIP(hipMemcpyAsync(d_hdr, hdr_blob.data(), hdr_blob.size(), hipMemcpyHostToDevice, ctx->stream));
    FHX_HIP(hipMemcpyAsync(d_hdr_off, hdr_off.data(), (size_t)n_members * 4, hipMemcpyHostToDevice, ctx->stream));
    FHX_HIP(hipMemcpyAsync(d_hdr_nbits, hdr_nbits.data(), (size_t)n_members * 4, hipMemcpyHostToDevice, ctx->stream));
    FHX_HIP(hipMemcpyAsync(d_member_bits, member_bits.data(), (size_t)n_members * 4, hipMemcpyHostToDevice, ctx->stream));
    FHX_HIP(hipMemcpyAsync(d_bit0, member_bit0.data(), (size_t)n_members * 8, hipMemcpyHostToDevice, ctx->stream));
    FHX_HIP(hipMemcpyAsync(d_start, member_start.data(), (size_t)(n_members + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    FHX_HIP(hipMemsetAsync(d_out, 0, (size_t)out_bytes + 16, ctx->stream));
    hipLaunchKernelGGL(em_bits, dim3((unsigned)n_wg), dim3(WG), 0, ctx->stream, (const unsigned char*)d_text, (const unsigned char*)d_len, n_rows,
                       (const CodeTab*)d_codes, d_wg_a);
    hipLaunchKernelGGL(em_scan_members, dim3(n_members), dim3(WG_PER_MEMBER), 0, ctx->stream, (const unsigned int*)d_wg_a, n_wg, d_wg_bitoff, d_member_bitsum);
    hipLaunchKernelGGL(em_encode, dim3((unsigned)n_wg), dim3(WG), 0, ctx->stream, (const unsigned char*)d_text, (const unsigned char*)d_len, n_rows,
                       (const CodeTab*)d_codes, (const unsigned int*)d_wg_bitoff, (const unsigned long long*)d_bit0, d_out);
    hipLaunchKernelGGL(em_frame, dim3((n_members + 63) / 64), dim3(64), 0, ctx->stream, n_members, (const unsigned char*)d_hdr,
                       (const unsigned int*)d_hdr_off, (const unsigned int*)d_hdr_nbits, (const unsigned long long*)d_bit0,
                       (const unsigned int*)d_member_bits, (const CodeTab*)d_codes, (const unsigned long long*)d_start,
                       (const unsigned int*)d_crc, (const unsigned int*)d_member_a, d_out);
    FHX_HIP(hipGetLastError());
    std::vector<unsigned int> h_bits_check(n_members);
    FHX_HIP(hipMemcpyAsync(h_bits_check.data(), d_member_bitsum, (size_t)n_members * 4, hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipStreamSynchronize(ctx->stream));
    for (int m = 0; m < n_members; ++m)
        if (h_text[m] != 0 && h_bits_check[m] != member_bits[m])
            return fail(ctx, FHX_ERR_HIP, "internal: token bits on the device differ from the histogram's (member " + std::to_string(m) + ")");
    mark("bit lengths + encode + frame");
    // ---- the buffer is the file: it leaves through the drainer (copies into two pinned buffers alternating with fwrite)
    // while the next batch is computed ----------------------------------------------------------------------------------
    out_guard.p = nullptr;
    drainer->push((unsigned char*)d_out, (size_t)out_bytes, out_cap);
    mark("hand-over to the copy-out thread");
    unsigned long long h_rows = 0;
    FHX_HIP(hipMemcpy(&h_rows, d_rows, 8, hipMemcpyDeviceToHost));
    if (timing) std::fprintf(stderr, "fhx_write_significances_device: rows %lld..%lld, %llu bytes:%s\n", (long long)r0, (long long)(r0 + n_rows),
                             out_bytes, t_report.c_str());
    *rows_acc += (int64_t)h_rows;
    *bytes_acc += (int64_t)out_bytes;
    return FHX_OK;
}

}  // namespace

extern "C" {

static int write_significances_rows(fhx_ctx* ctx, const char* path, const char* const* chr_names, int32_t n_names,
                                    const int32_t* chr1, const int32_t* mid1, const int32_t* chr2, const int32_t* mid2,
                                    const int32_t* count, int64_t n_rows, int64_t row_begin, int64_t row_end, bool with_header,
                                    int64_t* rows_written, int64_t* bytes_written);

int fhx_write_significances_device(fhx_ctx* ctx, const char* path, const char* const* chr_names, int32_t n_names,
                                   const int32_t* chr1, const int32_t* mid1, const int32_t* chr2, const int32_t* mid2,
                                   const int32_t* count, int64_t n_rows, int64_t* rows_written, int64_t* bytes_written) {
    return write_significances_rows(ctx, path, chr_names, n_names, chr1, mid1, chr2, mid2, count, n_rows, 0, n_rows, true, rows_written,
                                    bytes_written);
}

// A stretch [row_begin, row_end) of the context's rows as gzip members of their own, with or without the column-header member in
// front: the ranks of a sharded run write the stretches of the file they hold (fhx_shard_segments) and the pieces are put
// together in file order - a concatenation of gzip members is a gzip file.
int fhx_write_significances_device_range(fhx_ctx* ctx, const char* path, const char* const* chr_names, int32_t n_names, int64_t row_begin,
                                         int64_t row_end, int32_t with_header, int64_t* rows_written, int64_t* bytes_written) {
    if (!ctx) return FHX_ERR_ARG;
    if (row_begin < 0 || row_end < row_begin || row_end > ctx->n_rows) return fail(ctx, FHX_ERR_ARG, "row range outside the loaded rows");
    return write_significances_rows(ctx, path, chr_names, n_names, nullptr, nullptr, nullptr, nullptr, nullptr, ctx->n_rows, row_begin, row_end,
                                    with_header != 0, rows_written, bytes_written);
}

static int write_significances_rows(fhx_ctx* ctx, const char* path, const char* const* chr_names, int32_t n_names,
                                    const int32_t* chr1, const int32_t* mid1, const int32_t* chr2, const int32_t* mid2,
                                    const int32_t* count, int64_t n_rows, int64_t row_begin, int64_t row_end, bool with_header,
                                    int64_t* rows_written, int64_t* bytes_written) {
    using namespace fhx::emit;
    if (!ctx || !path || !chr_names || n_names <= 0 || n_rows < 0) return FHX_ERR_ARG;
    const bool derive = !chr1 && !mid1 && !chr2 && !mid2 && !count;       // all five absent: rebuild them from the resident rows
    if (n_rows > 0 && !derive && (!chr1 || !mid1 || !chr2 || !mid2 || !count)) return FHX_ERR_ARG;
    if (ctx->device < 0) return fail(ctx, FHX_ERR_NO_DEVICE, "host-only context");
    if (!ctx->have_p || !ctx->have_q) return fail(ctx, FHX_ERR_ARG, "p and q must have been computed (fhx_pvalues, fhx_bh)");
    if (n_rows != ctx->n_rows) return fail(ctx, FHX_ERR_ARG, "one identity row per loaded contact row is required");
    FHX_HIP(hipSetDevice(ctx->device));
    FHX_HIP(hipStreamSynchronize(ctx->stream));       // K3 is through: had it seen more survivors than it was sized for, say so
    {
        const int rc = check_fault(ctx);
        if (rc != FHX_OK) return rc;
    }
    // The file is produced under a temporary name in the same directory and renamed over `path` only when it is complete and
    // closed: a refusal in a later batch (FHX_ERR_UNSUPPORTED: the caller falls back to the host writer), a HIP or write error or
    // a crash leaves an output of an earlier run untouched.
    // That earlier output is GBs of page cache (or disk extents) which replacing it would give back while this call waits -
    // 0.3 s for 3.8 GB on tmpfs: once the new file is complete the old one is moved aside (a rename) and unlinked by a thread,
    // which is joined before this function returns.
    struct OldFile {
        std::string name;
        std::thread th;
        ~OldFile() {
            if (th.joinable()) th.join();
        }
    } old_file;
    struct TempFile {                                       // declared before the Closer: the stream is closed before the unlink
        std::string name;
        bool keep = false;
        ~TempFile() {
            if (!keep && !name.empty()) (void)::unlink(name.c_str());
        }
    } temp_file;
    // A target that exists and is not a plain file - a symlink, a FIFO, /dev/stdout, /dev/null - is written THROUGH, as
    // fopen(path, "wb") always did: renaming a regular file over it would replace the node itself.
    bool direct = false;
    {
        struct stat lst;
        if (::lstat(path, &lst) == 0 && !S_ISREG(lst.st_mode)) direct = true;
    }
    if (!direct) temp_file.name = std::string(path) + ".fhx-tmp-" + std::to_string((long long)::getpid());
    std::FILE* f = std::fopen(direct ? path : temp_file.name.c_str(), "wb");
    if (!f) {
        temp_file.name.clear();
        return fail(ctx, FHX_ERR_ARG, std::string("cannot open ") + path);
    }
    auto publish = [&]() -> int {                           // the complete, closed temporary file becomes `path`
        if (direct) return FHX_OK;
        struct stat st;
        bool moved = false;
        if (::stat(path, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > ((off_t)64 << 20)) {
            old_file.name = std::string(path) + ".fhx-old-" + std::to_string((long long)::getpid());
            moved = std::rename(path, old_file.name.c_str()) == 0;
        }
        if (std::rename(temp_file.name.c_str(), path) != 0) {
            if (moved) (void)std::rename(old_file.name.c_str(), path);
            return fail(ctx, FHX_ERR_ARG, std::string("cannot rename the finished file to ") + path);
        }
        temp_file.keep = true;
        if (moved) old_file.th = std::thread([name = old_file.name] { (void)::unlink(name.c_str()); });
        return FHX_OK;
    };
    struct Closer {
        std::FILE* f;
        ~Closer() {
            if (f) std::fclose(f);
        }
    } closer{f};
    // the column-header line: its own member, a stored deflate block written by hand
    if (with_header) {
        const char* hdr = "chr1\tfragmentMid1\tchr2\tfragmentMid2\tcontactCount\tp-value\tq-value\tbias1\tbias2\tExpCC\n";
        const unsigned int n = (unsigned int)std::strlen(hdr);
        unsigned int crc = 0xffffffffu;
        for (unsigned int i = 0; i < n; ++i) {
            crc ^= (unsigned char)hdr[i];
            for (int k = 0; k < 8; ++k) crc = (crc & 1u) ? 0xedb88320u ^ (crc >> 1) : crc >> 1;
        }
        crc ^= 0xffffffffu;
        std::vector<unsigned char> mem = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 255, 12, 0, 'F', 'H', 8, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        mem.push_back(1);                                                    // BFINAL = 1, BTYPE = 00 (stored)
        mem.push_back((unsigned char)(n & 0xFF));
        mem.push_back((unsigned char)(n >> 8));
        mem.push_back((unsigned char)(~n & 0xFF));
        mem.push_back((unsigned char)((~n >> 8) & 0xFF));
        mem.insert(mem.end(), hdr, hdr + n);
        for (int k = 0; k < 4; ++k) mem.push_back((unsigned char)((crc >> (8 * k)) & 0xFF));
        for (int k = 0; k < 4; ++k) mem.push_back((unsigned char)((n >> (8 * k)) & 0xFF));
        const unsigned long long total = mem.size();
        for (int k = 0; k < 8; ++k) mem[16 + k] = (unsigned char)((total >> (8 * k)) & 0xFF);
        if (std::fwrite(mem.data(), 1, mem.size(), f) != mem.size()) return fail(ctx, FHX_ERR_ARG, "write error");
    }
    if (rows_written) *rows_written = 0;
    if (bytes_written) *bytes_written = 0;
    if (row_end <= row_begin) {
        std::FILE* f0 = closer.f;
        closer.f = nullptr;
        if (std::fclose(f0) != 0) return fail(ctx, FHX_ERR_ARG, "write error on close");
        return publish();
    }
    if (derive && (!ctx->d_loc1 || !ctx->d_slot_chr || (!ctx->nonfixed && !ctx->d_grid) || (ctx->nonfixed && !ctx->d_slot_mid)))
        return fail(ctx, FHX_ERR_ARG, "no resident rows to rebuild the identity columns from");
    std::vector<char> blob;
    std::vector<int32_t> name_off(n_names + 1, 0);
    for (int i = 0; i < n_names; ++i) {
        const size_t l = std::strlen(chr_names[i]);
        blob.insert(blob.end(), chr_names[i], chr_names[i] + l);
        name_off[i + 1] = (int32_t)blob.size();
    }
    if (blob.empty()) blob.push_back(0);
    // batches of 512 members (3.4e7 rows: 6.4 GB of row text + ~2 GB of buffers on the device), so that a 2e9-row run does not
    // need 192 bytes of HBM per row at once; FHX_EMIT_BATCH_MEMBERS overrides (tests use 1 to cross batch boundaries)
    int64_t batch_members = 512;
    if (const char* e = std::getenv("FHX_EMIT_BATCH_MEMBERS")) batch_members = std::max<long long>(1, std::atoll(e));
    const int64_t batch = batch_members * MEMBER_ROWS;
    int64_t rows_acc = 0, bytes_acc = 0;
    hipError_t pin_err;
    EmitPinned* pinned = pinned_pair(ctx, &pin_err);
    FHX_HIP(pin_err);
    const auto t_all = std::chrono::steady_clock::now();
    ScratchPool pool;                                      // outlives the drainer, whose last act is to hand a buffer back
    {
        EmitDrainer drainer(ctx, f, pinned, &pool);
        for (int64_t r0 = row_begin; r0 < row_end; r0 += batch) {
            const int64_t n_b = std::min<int64_t>(batch, row_end - r0);
            const int32_t* h_col[5] = {derive ? nullptr : chr1 + r0, derive ? nullptr : mid1 + r0, derive ? nullptr : chr2 + r0,
                                       derive ? nullptr : mid2 + r0, derive ? nullptr : count + r0};
            const int rc = write_significances_batch(ctx, f, blob, name_off, n_names, h_col, derive, r0, n_b, &drainer, &pool, &rows_acc, &bytes_acc);
            if (rc != FHX_OK) return rc;                   // the drainer's destructor lets the batch in flight finish
        }
        const int rc = drainer.finish();
        if (rc != FHX_OK) return fail(ctx, rc, drainer.err);
        if (std::getenv("FHX_TIMING"))
            std::fprintf(stderr, "fhx_write_significances_device: %lld bytes in %.3f s, of which the copy-out thread was busy %.3f s\n",
                         (long long)bytes_acc, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_all).count(), drainer.seconds);
    }
    if (rows_written) *rows_written = rows_acc;
    if (bytes_written) *bytes_written = bytes_acc;
    std::FILE* ff = closer.f;
    closer.f = nullptr;
    if (std::fclose(ff) != 0) return fail(ctx, FHX_ERR_ARG, "write error on close");
    return publish();
}

int fhx_debug_format(fhx_ctx* ctx, const double* values, int64_t n, int32_t kind, char* text32, int32_t* len) {
    if (!ctx || !values || !text32 || !len || n < 0 || (kind != 0 && kind != 1)) return FHX_ERR_ARG;
    if (ctx->device < 0) return fail(ctx, FHX_ERR_NO_DEVICE, "host-only context");
    if (n == 0) return FHX_OK;
    FHX_HIP(hipSetDevice(ctx->device));
    DeviceScratch G;
    double* d_v = nullptr;
    char* d_t = nullptr;
    int* d_l = nullptr;
    FHX_HIP(G.get(&d_v, (size_t)n * 8));
    FHX_HIP(G.get(&d_t, (size_t)n * 32));
    FHX_HIP(G.get(&d_l, (size_t)n * 4));
    FHX_HIP(hipMemcpyAsync(d_v, values, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(fhx::emit::em_debug_format, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, (const double*)d_v, n, (int)kind, d_t, d_l);
    FHX_HIP(hipGetLastError());
    FHX_HIP(hipMemcpyAsync(text32, d_t, (size_t)n * 32, hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipMemcpyAsync(len, d_l, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipStreamSynchronize(ctx->stream));
    return FHX_OK;
}
