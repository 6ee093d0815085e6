// fhx_sigselect.hip - the FDR subset of a Fit-Hi-C significances file on MI355X (gfx950)
// (reference: fithic/utils/merge-filter.sh:22, `awk '{if(NR!=1){print $0}}' | awk -v q="$fdr" '{if($7<=q){print $0}}'`).
//
// The text goes through HBM in BATCHES cut at the last newline (two pinned buffers filled by pread, drained by the copy engine);
// only the kept lines come back.  Per batch:
//
//   ms_scan_text   16 KB of text per workgroup, 64 B per lane as 16-byte loads: newlines per block, and one flag for the batch
//                  when a byte outside the grammar is seen (ms_select looks at bytes one by one only then)
//   scan_tiles     exclusive scan of the block counts = the line number of every block's first line             (fhx_scan.hpp)
//   ms_select      the lines that begin in a block, one per lane.  One walk along the line splits it on blanks and finds field 7;
//                  the field is taken only in the shape C's %e writes, D.DDDDDDe[+-]XX[X], and is then
//                    zero     every digit 0: the number 0, kept when 0 <= fdr (0 < fdr when strict) - the host says which
//                    numeric  [2.225074e-308, 9.999999e+307]: awk compares numbers, and strtod is monotone in the integer key
//                             (exponent, 7-digit mantissa): ONE integer compare with the bound the host found by bisection
//                    string   a non-zero value below 2.225074e-308 or an exponent of 309 and more: awk's strtod flags ERANGE and
//                             the field is compared bytewise with the text of fdr (memcmp, then length)
//                  File line 1 is dropped unparsed when skip_first_line is set.  Per line: its kept length (0: dropped); per
//                  block: kept bytes and kept lines.
//   scan_tiles     kept bytes per block -> the block's offset in the subset
//   ms_gather      the kept lines, verbatim and in file order, into a dense buffer: 256 lines per round, their lengths scanned
//                  into LDS, lanes assigned by OUTPUT byte (a binary search in the 256 prefixes), so stores are coalesced at
//                  1 % kept and at 100 %.  A final line without its newline gets one, as awk's print gives it.
//
// The subset of each batch is copied to the host and appended.  No device-side strtod, no atomics per line: a refused line
// costs one atomicMin (line << 8 | reason), so the smallest offending line is reported whatever the launch order.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/fithic_mi355x.h"
#include "fhx_cpus.hpp"
#include "fhx_scan.hpp"

namespace msd {

constexpr int WG = 256;
constexpr int BLOCK_BYTES = 16384;             // text per workgroup
constexpr int SEG = BLOCK_BYTES / WG;          // 64 bytes per lane in the newline passes
constexpr int MAX_LINE = 4096;                 // a longer line is refused
constexpr unsigned long long NO_ERROR = ~0ull;
constexpr unsigned long long KEY_EXP = 10000000ull;      // key = (exponent + 308) * 10^7 + the seven digits

// the threshold as the shell passes it: its bytes for the string class, by value
struct Fdr {
    unsigned char text[FHX_MS_FDR_BYTES];
    int len;
};

// the words the kernels of one call share
struct Words {
    unsigned long long newlines;               // scan_tiles' total of the current batch
    unsigned long long bad_bytes;              // 1: ms_scan_text saw a byte outside the grammar in the current batch
    unsigned long long first_error;            // smallest (line << 8 | reason)
    unsigned long long kept_bytes;             // scan_tiles' total of the current batch
    unsigned long long kept_lines;             // of the current batch
};

__device__ inline bool refused_byte(unsigned int c) { return c < 0x20u ? (c != '\t' && c != '\n') : c >= 0x7fu; }

// ---- pass 1 over a batch: newlines per block, refused bytes anywhere ------------------------------------------------------------
__global__ __launch_bounds__(WG) void ms_scan_text(const unsigned char* __restrict__ text, int64_t T, unsigned int* __restrict__ block_nl,
                                                   Words* __restrict__ words) {
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
                const bool inside = p0 + v * 16 + k < T;
                nl += (c == '\n' && inside) ? 1u : 0u;
                bad |= inside && refused_byte(c);
            }
        }
    }
    unsigned int total;
    fhxscan::block_exclusive_scan(nl, &total);
    if (threadIdx.x == 0) block_nl[blockIdx.x] = total;
    if (bad) __atomic_store_n(&words->bad_bytes, 1ull, __ATOMIC_RELAXED);     // every writer stores the same value
}

// The lines that BEGIN after a newline of this block (and line 0 in block 0): their start offsets relative to the block, in
// order, in LDS.  Line number of entry e within the batch: e in block 0, block_off[block] + 1 + e elsewhere.
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

__device__ inline bool is_digit(int c) { return c >= '0' && c <= '9'; }

// Field 7 at text[b, b + len): 0 = not the %e shape (or one the classes leave out), 1 = zero, 2 = numeric (*key set), 3 = string.
__device__ inline int classify(const unsigned char* __restrict__ text, int64_t b, int len, unsigned long long* key) {
    if (len != 12 && len != 13) return 0;
    const int d0 = text[b];
    if (!is_digit(d0) || text[b + 1] != '.' || text[b + 8] != 'e') return 0;
    unsigned long long mant = (unsigned long long)(d0 - '0');
    for (int k = 2; k < 8; ++k) {
        const int c = text[b + k];
        if (!is_digit(c)) return 0;
        mant = mant * 10 + (unsigned long long)(c - '0');
    }
    const int sign = text[b + 9];
    if (sign != '+' && sign != '-') return 0;
    int ex = 0;
    for (int k = 10; k < len; ++k) {
        const int c = text[b + k];
        if (!is_digit(c)) return 0;
        ex = ex * 10 + (c - '0');
    }
    if (mant == 0) return 1;
    if (d0 == '0') return 0;                                                  // 0.000001e-03: not what %e writes
    if (sign == '-') ex = -ex;
    if (ex == 308) return 0;                                                  // numeric up to 1.797693e+308, a string above: left out
    if (ex > 308) return 3;
    if (ex < -308 || (ex == -308 && mant < 2225074ull)) return 3;
    *key = (unsigned long long)(ex + 308) * KEY_EXP + mant;
    return 2;
}

// awk's string comparison of the field with the text of fdr: memcmp over the common length, then the lengths
__device__ inline int compare_text(const unsigned char* __restrict__ text, int64_t b, int len, const Fdr& fdr) {
    const int common = len < fdr.len ? len : fdr.len;
    for (int k = 0; k < common; ++k) {
        const int a = text[b + k], q = fdr.text[k];
        if (a != q) return a < q ? -1 : 1;
    }
    return len < fdr.len ? -1 : (len > fdr.len ? 1 : 0);
}

// ---- pass 2: keep or drop every line --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void ms_select(const unsigned char* __restrict__ text, int64_t T, const unsigned long long* __restrict__ block_off,
                                                int64_t n_lines_batch, int64_t line_base, Fdr fdr, unsigned long long key_bound, int zero_kept,
                                                int strict, int skip_first_line, int check_bytes, unsigned short* __restrict__ keep_len,
                                                unsigned int* __restrict__ block_bytes, Words* __restrict__ words) {
    __shared__ unsigned short lstart[BLOCK_BYTES + 2];      // block 0: the implicit first line + one per newline byte = BLOCK_BYTES + 1 entries
    const int n_lines = block_lines(text, T, lstart);
    const int64_t b0 = (int64_t)blockIdx.x * BLOCK_BYTES;
    const int64_t row0 = blockIdx.x == 0 ? 0 : (int64_t)block_off[blockIdx.x] + 1;
    unsigned int my_bytes = 0, my_lines = 0;
    for (int e = threadIdx.x; e < n_lines; e += WG) {
        const int64_t r = row0 + e;
        const int64_t start = b0 + lstart[e];
        const bool header = skip_first_line && line_base + r == 0;
        int why = 0, tok = 0;
        bool in_tok = false;
        int64_t fb = 0, fe = 0;                                               // field 7
        int64_t p = start;
        for (;; ++p) {
            const int c = p < T ? (int)text[p] : '\n';                        // the end of the text ends the line
            if (c == '\n') break;
            if (p - start >= MAX_LINE) {
                why = FHX_MS_LONG_LINE;
                break;
            }
            if (check_bytes && refused_byte((unsigned int)c)) {
                why = FHX_MS_BYTES;
                break;
            }
            const bool blank = c == ' ' || c == '\t';
            if (!blank && !in_tok) {
                in_tok = true;
                if (++tok == 7) fb = p;
            } else if (blank && in_tok) {
                in_tok = false;
                if (tok == 7) fe = p;
            }
        }
        if (in_tok && tok == 7) fe = p;
        bool keep = false;
        if (!why && r >= n_lines_batch) why = FHX_MS_INTERNAL;                // the scan and this kernel disagree about the lines
        if (!why && !header) {
            if (tok < 7) why = FHX_MS_TOKENS;
            else {
                unsigned long long key = 0;
                const int cls = classify(text, fb, (int)(fe - fb), &key);
                if (cls == 0) why = FHX_MS_FIELD;
                else if (cls == 1) keep = zero_kept != 0;
                else if (cls == 2) keep = key <= key_bound;
                else {
                    const int cmp = compare_text(text, fb, (int)(fe - fb), fdr);
                    keep = strict ? cmp < 0 : cmp <= 0;
                }
            }
        }
        if (why) atomicMin(&words->first_error, ((unsigned long long)(line_base + r + 1) << 8) | (unsigned long long)why);
        const unsigned int len = (keep && !why) ? (unsigned int)(p - start) + 1u : 0u;      // with its newline, present or not
        if (r < n_lines_batch) keep_len[r] = (unsigned short)len;             // at most MAX_LINE + 1
        my_bytes += len;
        my_lines += len ? 1u : 0u;
    }
    unsigned int total_bytes, total_lines;
    fhxscan::block_exclusive_scan(my_bytes, &total_bytes);                    // every lane of the block arrives here
    fhxscan::block_exclusive_scan(my_lines, &total_lines);
    if (threadIdx.x == 0) {
        block_bytes[blockIdx.x] = total_bytes;
        if (total_lines) atomicAdd(&words->kept_lines, (unsigned long long)total_lines);
    }
}

// ---- pass 3: the kept lines, dense and in file order ----------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void ms_gather(const unsigned char* __restrict__ text, int64_t T, const unsigned long long* __restrict__ block_off,
                                                int64_t n_lines_batch, const unsigned short* __restrict__ keep_len,
                                                const unsigned long long* __restrict__ out_off, unsigned char* __restrict__ out, int64_t out_capacity) {
    __shared__ unsigned short lstart[BLOCK_BYTES + 2];
    __shared__ unsigned int pre[WG + 1];                    // round-local exclusive prefix of the kept lengths; pre[WG] = their sum
    const int n_lines = block_lines(text, T, lstart);
    const int64_t b0 = (int64_t)blockIdx.x * BLOCK_BYTES;
    const int64_t row0 = blockIdx.x == 0 ? 0 : (int64_t)block_off[blockIdx.x] + 1;
    int64_t at = (int64_t)out_off[blockIdx.x];
    for (int base = 0; base < n_lines; base += WG) {        // n_lines is the same for every lane: the scan sees whole blocks
        const int e = base + threadIdx.x;
        const int64_t r = row0 + e;
        const unsigned int len = (e < n_lines && r < n_lines_batch) ? (unsigned int)keep_len[r] : 0u;
        unsigned int total;
        pre[threadIdx.x] = fhxscan::block_exclusive_scan(len, &total);
        if (threadIdx.x == 0) pre[WG] = total;
        __syncthreads();
        for (unsigned int j = threadIdx.x; j < total; j += WG) {
            int lo = 0, hi = WG;                            // the last t with pre[t] <= j: a dropped line shares its prefix with the
            while (hi - lo > 1) {                           // next one, so the last of equals is the line that holds byte j
                const int mid = (lo + hi) >> 1;
                if (pre[mid] <= j) lo = mid;
                else hi = mid;
            }
            const int64_t src = b0 + lstart[base + lo] + (int64_t)(j - pre[lo]);
            const unsigned char c = src < T ? text[src] : (unsigned char)'\n';       // the newline the last line lacked
            if (at + j < out_capacity) out[at + j] = c;
        }
        at += total;
        __syncthreads();                                    // pre is written again in the next round
    }
}

}  // namespace msd

// ===================================================================================================================
struct fhx_ms {
    int device = -1;
    hipStream_t stream = nullptr;
    std::string err;
    // the last selection
    std::vector<char> subset;
    int64_t n_lines = 0, n_kept = 0;
    double seconds[FHX_MS_STAGES] = {0, 0, 0, 0, 0};
    // the upload path
    static constexpr size_t kChunk = (size_t)32 << 20;
    void* pinned[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
};

namespace {

int mfail(fhx_ms* ms, int code, const std::string& msg) {
    if (ms) ms->err = msg;
    return code;
}

#define MS_HIP(call)                                                                                      \
    do {                                                                                                  \
        hipError_t e_ = (call);                                                                           \
        if (e_ != hipSuccess) return mfail(ms, FHX_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

// device temporaries of one call
struct Scratch {
    std::vector<void*> ptrs;
    ~Scratch() {
        for (void* p : ptrs) (void)hipFree(p);
    }
    template <typename T>
    hipError_t get(T** p, size_t count) {
        hipError_t e = hipMalloc((void**)p, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) ptrs.push_back(*p);
        return e;
    }
    void drop(void* p) {
        auto it = std::find(ptrs.begin(), ptrs.end(), p);
        if (it != ptrs.end()) {
            (void)hipFree(p);
            ptrs.erase(it);
        }
    }
};

// the text: a file read with pread, or the inflated bytes of a gzip file
struct Source {
    int fd = -1;
    std::vector<char> inflated;
    int64_t size = 0;
    ~Source() {
        if (fd >= 0) ::close(fd);
    }
};

void drop_subset(fhx_ms* ms) {
    std::vector<char>().swap(ms->subset);
    ms->n_lines = ms->n_kept = 0;
}

// bytes [off, off + len) of the source -> d_text[0, len): host threads fill one of two pinned buffers while the copy engine
// drains the other.  *last_newline = the offset (within the range) of the range's last newline, -1 without one.
int upload_range(fhx_ms* ms, Source& src, int64_t off, int64_t len, unsigned char* d_text, int64_t* last_newline) {
    for (int k = 0; k < 2; ++k) {
        if (!ms->pinned[k]) MS_HIP(hipHostMalloc(&ms->pinned[k], fhx_ms::kChunk, hipHostMallocDefault));
        if (!ms->ev[k]) MS_HIP(hipEventCreateWithFlags(&ms->ev[k], hipEventDisableTiming));
    }
    const int n_threads = std::min(fhx::usable_cpus(), 8);
    bool used[2] = {false, false};
    int turn = 0;
    *last_newline = -1;
    for (int64_t done = 0; done < len; done += (int64_t)fhx_ms::kChunk, turn ^= 1) {
        const int64_t now = std::min<int64_t>((int64_t)fhx_ms::kChunk, len - done);
        if (used[turn]) MS_HIP(hipEventSynchronize(ms->ev[turn]));
        char* dst = (char*)ms->pinned[turn];
        if (src.fd < 0) {
            std::memcpy(dst, src.inflated.data() + off + done, (size_t)now);
        } else {
            const int64_t slice = (int64_t)4 << 20;
            const int64_t n_slices = (now + slice - 1) / slice;
            std::atomic<int64_t> next{0};
            std::atomic<int> io_errno{0};
            auto work = [&]() {
                for (;;) {
                    const int64_t s = next.fetch_add(1);
                    if (s >= n_slices) return;
                    int64_t at = s * slice;
                    const int64_t stop = std::min(now, at + slice);
                    while (at < stop) {
                        const ssize_t got = ::pread(src.fd, dst + at, (size_t)(stop - at), (off_t)(off + done + at));
                        if (got < 0 && errno == EINTR) continue;
                        if (got <= 0) {                                       // an error, or the file shrank under us
                            io_errno = got < 0 ? errno : EIO;
                            return;
                        }
                        at += got;
                    }
                }
            };
            const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(n_threads, n_slices));
            std::vector<std::thread> pool;
            for (int k = 1; k < nt; ++k) pool.emplace_back(work);
            work();
            for (auto& th : pool) th.join();
            if (io_errno) {
                (void)hipStreamSynchronize(ms->stream);
                return mfail(ms, FHX_ERR_ARG, std::string("reading the significances file: ") + std::strerror(io_errno));
            }
        }
        if (const void* nl = ::memrchr(dst, '\n', (size_t)now)) *last_newline = done + ((const char*)nl - dst);
        MS_HIP(hipMemcpyAsync(d_text + done, dst, (size_t)now, hipMemcpyHostToDevice, ms->stream));
        MS_HIP(hipEventRecord(ms->ev[turn], ms->stream));
        used[turn] = true;
    }
    return FHX_OK;
}

}  // namespace

extern "C" {

int fhx_ms_create(int device, fhx_ms** out) {
    if (!out) return FHX_ERR_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return FHX_ERR_NO_DEVICE;
    fhx_ms* ms = new fhx_ms();
    ms->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ms->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ms;
        return FHX_ERR_HIP;
    }
    *out = ms;
    return FHX_OK;
}

void fhx_ms_destroy(fhx_ms* ms) {
    if (!ms) return;
    (void)hipSetDevice(ms->device);
    if (ms->stream) (void)hipStreamSynchronize(ms->stream);
    for (int k = 0; k < 2; ++k) {
        if (ms->pinned[k]) (void)hipHostFree(ms->pinned[k]);
        if (ms->ev[k]) (void)hipEventDestroy(ms->ev[k]);
    }
    if (ms->stream) (void)hipStreamDestroy(ms->stream);
    delete ms;
}

const char* fhx_ms_last_error(const fhx_ms* ms) { return ms ? ms->err.c_str() : "null context"; }

int fhx_ms_select_file(fhx_ms* ms, const char* path, const char* fdr_text, int32_t fdr_len, uint64_t key_bound, int32_t zero_kept, int32_t strict,
                       int32_t skip_first_line, int64_t* n_bytes, int32_t* why, int64_t* bad_line) {
    using namespace msd;
    if (!ms || !path || !fdr_text || !n_bytes || !why || !bad_line) return FHX_ERR_ARG;
    *n_bytes = 0;
    *why = FHX_MS_OK;
    *bad_line = 0;
    MS_HIP(hipSetDevice(ms->device));
    MS_HIP(hipStreamSynchronize(ms->stream));
    drop_subset(ms);
    for (double& s : ms->seconds) s = 0;
    if (fdr_len < 1 || fdr_len > FHX_MS_FDR_BYTES) {
        *why = FHX_MS_FDR;
        return mfail(ms, FHX_ERR_UNSUPPORTED, "the text of fdr must have 1 to " + std::to_string(FHX_MS_FDR_BYTES) + " bytes");
    }
    Fdr fdr;
    std::memset(&fdr, 0, sizeof(fdr));
    std::memcpy(fdr.text, fdr_text, (size_t)fdr_len);
    fdr.len = fdr_len;
    auto t_last = std::chrono::steady_clock::now();
    auto mark = [&](int k) {                                                  // the stream is idle at every call
        const auto now = std::chrono::steady_clock::now();
        ms->seconds[k] += std::chrono::duration<double>(now - t_last).count();
        t_last = now;
    };
    // ---- the source: the file itself, or its inflated bytes when it starts with the gzip magic --------------------------------
    Source src;
    src.fd = ::open(path, O_RDONLY | O_CLOEXEC);
    if (src.fd < 0) return mfail(ms, FHX_ERR_ARG, std::string(path) + ": " + std::strerror(errno));
    struct stat sb;
    if (::fstat(src.fd, &sb) != 0 || !S_ISREG(sb.st_mode)) return mfail(ms, FHX_ERR_ARG, std::string(path) + ": not a regular file");
    src.size = (int64_t)sb.st_size;
    unsigned char magic[2] = {0, 0};
    if (src.size >= 2 && ::pread(src.fd, magic, 2, 0) == 2 && magic[0] == 0x1f && magic[1] == 0x8b) {
        fhx_text* x = nullptr;
        int rc = fhx_host_inflate(path, 0, &x);
        if (rc != FHX_OK) {
            const std::string msg = x ? fhx_text_error(x) : "fhx_host_inflate";
            fhx_text_free(x);
            return mfail(ms, rc, msg);
        }
        src.inflated.resize((size_t)fhx_text_bytes(x));
        rc = fhx_text_copy(x, src.inflated.data(), (int64_t)src.inflated.size());
        fhx_text_free(x);
        if (rc != FHX_OK) return mfail(ms, rc, "fhx_text_copy");
        ::close(src.fd);
        src.fd = -1;
        src.size = (int64_t)src.inflated.size();
    }
    // ---- the batches ---------------------------------------------------------------------------------------------------------
    int64_t batch_bytes = (int64_t)256 << 20;                                 // FHX_MS_BATCH_BYTES overrides (tests put a batch edge inside a small file)
    if (const char* e = std::getenv("FHX_MS_BATCH_BYTES")) batch_bytes = std::atoll(e);
    batch_bytes = std::max<int64_t>(2 * MAX_LINE, std::min<int64_t>(batch_bytes, (int64_t)1 << 31));
    batch_bytes = std::min(batch_bytes, std::max<int64_t>(src.size, 2 * MAX_LINE));
    const int64_t max_blocks = (batch_bytes + BLOCK_BYTES - 1) / BLOCK_BYTES;
    const int64_t out_capacity = batch_bytes + 1;                             // every line kept, and the newline the last one lacked
    Scratch tmp;
    unsigned char *d_text = nullptr, *d_out = nullptr;
    unsigned int *d_block_nl = nullptr, *d_block_bytes = nullptr;
    unsigned long long *d_block_off = nullptr, *d_out_off = nullptr;
    unsigned short* d_keep_len = nullptr;
    int64_t keep_capacity = 0;
    Words* d_words = nullptr;
    MS_HIP(tmp.get(&d_text, (size_t)max_blocks * BLOCK_BYTES + 64));
    MS_HIP(tmp.get(&d_out, (size_t)out_capacity));
    MS_HIP(tmp.get(&d_block_nl, (size_t)max_blocks));
    MS_HIP(tmp.get(&d_block_bytes, (size_t)max_blocks));
    MS_HIP(tmp.get(&d_block_off, (size_t)max_blocks));
    MS_HIP(tmp.get(&d_out_off, (size_t)max_blocks));
    MS_HIP(tmp.get(&d_words, 1));
    Words words;
    auto refuse = [&](int rc, int32_t w, int64_t line, const std::string& msg) {
        drop_subset(ms);
        *why = w;
        *bad_line = line;
        return mfail(ms, rc, msg);
    };
    int64_t lines = 0, kept = 0;
    for (int64_t off = 0; off < src.size;) {
        int64_t len = std::min(batch_bytes, src.size - off), last_nl = -1;
        std::memset(&words, 0, sizeof(words));
        words.first_error = NO_ERROR;
        MS_HIP(hipMemcpyAsync(d_words, &words, sizeof(words), hipMemcpyHostToDevice, ms->stream));
        {
            const int rc = upload_range(ms, src, off, len, d_text, &last_nl);
            if (rc != FHX_OK) return rc;
        }
        // a batch that does not reach the end of the text ends after its last newline; without one its single line is longer than
        // MAX_LINE and the select kernel says so
        if (off + len < src.size && last_nl >= 0) len = last_nl + 1;
        const int64_t n_blocks = (len + BLOCK_BYTES - 1) / BLOCK_BYTES;
        MS_HIP(hipMemsetAsync(d_text + len, ' ', (size_t)(n_blocks * BLOCK_BYTES + 64 - len), ms->stream));
        MS_HIP(hipStreamSynchronize(ms->stream));                             // the pinned buffers are free again
        mark(0);
        hipLaunchKernelGGL(ms_scan_text, dim3((unsigned)n_blocks), dim3(WG), 0, ms->stream, (const unsigned char*)d_text, len, d_block_nl, d_words);
        hipLaunchKernelGGL(fhxscan::scan_tiles, dim3(1), dim3(fhxscan::THREADS), 0, ms->stream, (const unsigned int*)d_block_nl, n_blocks, d_block_off,
                           &d_words->newlines);
        MS_HIP(hipGetLastError());
        MS_HIP(hipMemcpyAsync(&words, d_words, sizeof(words), hipMemcpyDeviceToHost, ms->stream));
        MS_HIP(hipStreamSynchronize(ms->stream));
        mark(1);
        const int64_t n = (int64_t)words.newlines + (last_nl == len - 1 ? 0 : 1);
        if (n > keep_capacity) {                                              // one length per line of the batch
            if (d_keep_len) tmp.drop(d_keep_len);
            d_keep_len = nullptr;
            MS_HIP(tmp.get(&d_keep_len, (size_t)n));
            keep_capacity = n;
        }
        hipLaunchKernelGGL(ms_select, dim3((unsigned)n_blocks), dim3(WG), 0, ms->stream, (const unsigned char*)d_text, len,
                           (const unsigned long long*)d_block_off, n, lines, fdr, (unsigned long long)key_bound, (int)zero_kept, (int)strict,
                           (int)skip_first_line, (int)(words.bad_bytes != 0), d_keep_len, d_block_bytes, d_words);
        hipLaunchKernelGGL(fhxscan::scan_tiles, dim3(1), dim3(fhxscan::THREADS), 0, ms->stream, (const unsigned int*)d_block_bytes, n_blocks, d_out_off,
                           &d_words->kept_bytes);
        MS_HIP(hipGetLastError());
        MS_HIP(hipMemcpyAsync(&words, d_words, sizeof(words), hipMemcpyDeviceToHost, ms->stream));
        MS_HIP(hipStreamSynchronize(ms->stream));
        mark(2);
        if (words.first_error != NO_ERROR) {                                  // earlier batches hold the smaller line numbers
            const int32_t w = (int32_t)(words.first_error & 0xFFu);
            const int64_t line = (int64_t)(words.first_error >> 8);
            if (w == FHX_MS_INTERNAL) return refuse(FHX_ERR_INTERNAL, w, line, "the line count of the scan and the select kernel disagree");
            return refuse(FHX_ERR_UNSUPPORTED, w, line, "line " + std::to_string(line) + " is outside the device grammar (reason " + std::to_string(w) + ")");
        }
        const int64_t bytes = (int64_t)words.kept_bytes;
        if (bytes > out_capacity || (int64_t)words.kept_lines > n) return refuse(FHX_ERR_INTERNAL, FHX_MS_INTERNAL, 0, "more kept bytes than text");
        if (bytes > 0) {
            hipLaunchKernelGGL(ms_gather, dim3((unsigned)n_blocks), dim3(WG), 0, ms->stream, (const unsigned char*)d_text, len,
                               (const unsigned long long*)d_block_off, n, (const unsigned short*)d_keep_len, (const unsigned long long*)d_out_off, d_out,
                               out_capacity);
            MS_HIP(hipGetLastError());
            MS_HIP(hipStreamSynchronize(ms->stream));
        }
        mark(3);
        if (bytes > 0) {
            const size_t had = ms->subset.size();
            ms->subset.resize(had + (size_t)bytes);
            MS_HIP(hipMemcpyAsync(ms->subset.data() + had, d_out, (size_t)bytes, hipMemcpyDeviceToHost, ms->stream));
            MS_HIP(hipStreamSynchronize(ms->stream));
        }
        mark(4);
        lines += n;
        kept += (int64_t)words.kept_lines;
        off += len;
    }
    ms->n_lines = lines;
    ms->n_kept = kept;
    *n_bytes = (int64_t)ms->subset.size();
    if (std::getenv("FHX_TIMING"))
        std::fprintf(stderr, "FDR subset on the device (%s): %lld lines, %lld kept (%lld bytes): read + upload %.6f s; scan %.6f s; select %.6f s; "
                     "gather %.6f s; copy out %.6f s\n", path, (long long)lines, (long long)kept, (long long)ms->subset.size(), ms->seconds[0],
                     ms->seconds[1], ms->seconds[2], ms->seconds[3], ms->seconds[4]);
    return FHX_OK;
}

int fhx_ms_counts(const fhx_ms* ms, int64_t* n_lines, int64_t* n_kept, int64_t* n_bytes) {
    if (!ms) return FHX_ERR_ARG;
    if (n_lines) *n_lines = ms->n_lines;
    if (n_kept) *n_kept = ms->n_kept;
    if (n_bytes) *n_bytes = (int64_t)ms->subset.size();
    return FHX_OK;
}

int fhx_ms_stage_seconds(const fhx_ms* ms, double* seconds) {
    if (!ms || !seconds) return FHX_ERR_ARG;
    for (int k = 0; k < FHX_MS_STAGES; ++k) seconds[k] = ms->seconds[k];
    return FHX_OK;
}

int fhx_ms_copy_subset(const fhx_ms* ms, void* dst, int64_t capacity) {
    if (!ms || capacity < (int64_t)ms->subset.size() || (!dst && !ms->subset.empty())) return FHX_ERR_ARG;
    if (!ms->subset.empty()) std::memcpy(dst, ms->subset.data(), ms->subset.size());
    return FHX_OK;
}

}  // extern "C"
