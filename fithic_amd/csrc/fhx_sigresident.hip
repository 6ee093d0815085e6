// fhx_sigresident.hip - the FDR subset of a pass taken from its RESIDENT columns: what fhx_ms_select_file gives for the file
// fhx_write_significances_device writes, without the file.  The rows merge-filter.sh drops are never formatted, deflated,
// inflated or uploaded.
//
// The decision is the script's, made on the %e TEXT of q (fhx_sigkey.hpp, shared with ms_select), and the kept rows' text is
// the writer's (fhx_emitrow.hpp: row_identity / row_emitted / row_text, shared with em_format).  On the context's stream:
//
//   sr_decide      one loaded row per lane.  The emit predicate; q -> fmt_e6 -> classify -> zero / numeric key / string compare;
//                  one flag byte per row (not emitted, emitted and dropped, kept); per workgroup the emitted and the kept count.
//                  A q whose text the classes leave out (nan, inf, a sign, exponent 308) costs one atomicMin (row << 8 | reason).
//                  fmt_e6 has no text for 2^64 and more: from the first double that prints e+308 on that is the same refusal,
//                  below it the call is FHX_ERR_UNSUPPORTED as the writer's is.
//                  Bracket: every normal q below `lo` is kept and every one above `hi` (and below 1e300) dropped unformatted; lo
//                  and hi are the doubles nearest the %e fields of the key bound and of the key after it, and rounding a double
//                  to seven digits is monotone, so the bracket decides exactly as the text does.  FHX_SR_NO_BRACKET=1 formats all.
//   scan_tiles x2  the workgroup's emitted rank and kept rank
//   sr_rows        the kept rows' numbers compacted, ascending (file order), and their five columns gathered behind them, so
//                  that k2_extras and the formatter run over the kept rows alone
//   k2_extras      ExpCC and the two biases of the kept rows
//   sr_measure     one kept row per lane: the length of its text; per workgroup the bytes
//   scan_tiles     the workgroup's byte offset
//   sr_format      256 kept rows per workgroup: each lane writes its row into an LDS window that starts on a 16-byte boundary
//                  of the output, and the window leaves 16 bytes a lane; only the ragged ends go bytewise.  Every store is
//                  checked against the scanned total; what a lane wrote is compared with what sr_measure counted.
//
// The same front - the state rules, sr_decide, the two rank scans, the refusal with its line, sr_rows - serves the interact track
// (fhx_sigresident_track.inc) and the per-chromosome subsets (fhx_sigresident_split.inc), both included at the end of this file:
// sr_decide is a template over the view, and decide_rows<VIEW> / gather_kept below are what the three C calls share; the subset
// and the split also share what follows the kept rows' columns (kept_extras, format_kept).
#include <cfloat>

#include "fhx_ctx.hpp"
#include "fhx_emitrow.hpp"
#include "fhx_namerule.hpp"
#include "fhx_sigkey.hpp"
#include "fhx_trackline.hpp"

namespace fhx::sigres {

using emit::Cols;
using emit::RowId;

constexpr int WG = 256;
constexpr unsigned char NOT_EMITTED = 0, DROPPED = 1, KEPT = 2;
constexpr unsigned long long NO_BAD_ROW = ~0ull;
constexpr int WINDOW = WG * emit::ROW_STRIDE + 16;      // the longest round, moved up to 15 bytes into its first 16

struct Words {
    unsigned long long first_bad;              // smallest (loaded row << 8 | reason)
    unsigned long long n_emitted, n_kept, n_bytes;      // the three scans' totals
    unsigned long long n_deferred;             // the track's fourth: kept rows whose score the host writes
    unsigned int unsupported;                  // a kept row (or a q) the formatter does not cover
    unsigned int internal;                     // sr_format wrote another length than sr_measure counted
};

struct Decision {
    msd::Fdr fdr;
    unsigned long long key_bound;
    int zero_kept, strict, bracket;
    double lo, hi;
    double e308;                               // the smallest double %e prints with an exponent of 308
};

// two counts of a workgroup from one predicate pair, thread 0 stores them
__device__ __forceinline__ void count_pair(bool a, bool b, unsigned int* out_a, unsigned int* out_b) {
    __shared__ unsigned int wa[WG / 64], wb[WG / 64];
    const unsigned long long ma = __ballot(a), mb = __ballot(b);
    if ((threadIdx.x & 63) == 0) {
        wa[threadIdx.x >> 6] = (unsigned int)__popcll(ma);
        wb[threadIdx.x >> 6] = (unsigned int)__popcll(mb);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        out_a[blockIdx.x] = wa[0] + wa[1] + wa[2] + wa[3];
        out_b[blockIdx.x] = wb[0] + wb[1] + wb[2] + wb[3];
    }
}

// bytes of chromosome c's name (0 for an id the names do not cover: row_text refuses that row)
__device__ __forceinline__ int name_bytes(const Cols& C, int c) { return c >= 0 && c < C.n_names ? C.name_off[c + 1] - C.name_off[c] : 0; }

// What the decision is for.  SUBSET: merge-filter.sh's, and nothing else.
// TRACK: the rules the track's file route applies to every parsed line beyond field 7 - both midpoints 1 to 9 digits, both names
// at most 63 bytes - hold for every emitted row, kept or not, behind the same word and in trackline::refusal's order (field 7
// first: fhx_sigtrack.inc, ut_select, `why = refusal(cls, ...)`).
// SPLIT: the name rules of the per-chromosome split hold for both names of every emitted row, looked up per chromosome id in the
// table the host made with namerule::name_grammar, and they come BEFORE field 7 (fhx_sigsplit.inc, mp_select: name_grammar of
// token 1, of token 3, then classify); a row is kept only when it is cis (`$1 == c && $3 == c`); every emitted row marks its
// first chromosome as listed (`cut -f1`) with a plain store of the same value, skipped where the lane before holds the same id.
enum View { SUBSET = 0, TRACK = 1, SPLIT = 2 };
struct SplitTables {
    const unsigned char* name_why;             // per chromosome id: 0 or the reason its name is refused for
    unsigned char* listed;                     // per chromosome id: set when an emitted row has it as its first chromosome
};

template <int VIEW>
__global__ __launch_bounds__(WG) void sr_decide(Cols C, Decision D, unsigned char* __restrict__ flags, unsigned int* __restrict__ wg_emitted,
                                                unsigned int* __restrict__ wg_kept, Words* __restrict__ words, SplitTables S) {
    const int64_t r = (int64_t)blockIdx.x * WG + threadIdx.x;
    unsigned char flag = NOT_EMITTED;
    int listed_id = -1;
    if (r < C.n_rows) {
        const RowId id = emit::row_identity(C, r);
        if (emit::row_emitted(C, id)) {
            const double q = C.q[r];
            const bool plain = q >= DBL_MIN && q < 1e300;                     // a normal double whose exponent field is not 308
            bool keep = false;
            int why = 0;
            if (D.bracket && plain && q < D.lo) keep = true;
            else if (D.bracket && plain && q > D.hi) keep = false;
            else {
                char field[16];                                               // at most -D.DDDDDDe-XXX
                const int w = fmt::fmt_e6(q, field);
                if (w <= 0 && q >= D.e308) why = FHX_MS_FIELD;                // fmt_e6 stops at 2^64, but this one's exponent is known
                else if (w <= 0) atomicOr(&words->unsupported, 1u);           // 2^64 and more: the writer has no text for it either
                else {
                    unsigned long long key = 0;
                    const int cls = msd::classify((const unsigned char*)field, 0, w, &key);
                    why = msd::decide(cls, key, D.key_bound, D.zero_kept, D.strict, (const unsigned char*)field, 0, w, D.fdr, &keep);
                }
            }
            if constexpr (VIEW == TRACK)
                why = trackline::refusal(why ? 0 : 2, trackline::midpoint_ok(id.m1) && trackline::midpoint_ok(id.m2), name_bytes(C, id.c1),
                                         name_bytes(C, id.c2));
            if constexpr (VIEW == SPLIT) {
                const bool known = id.c1 >= 0 && id.c1 < C.n_names && id.c2 >= 0 && id.c2 < C.n_names;
                const int name_why = !known ? FHX_MS_INTERNAL : (S.name_why[id.c1] ? S.name_why[id.c1] : S.name_why[id.c2]);
                if (name_why) why = name_why;
                keep = keep && id.c1 == id.c2;
                if (known) listed_id = id.c1;
            }
            if (why) atomicMin(&words->first_bad, ((unsigned long long)r << 8) | (unsigned long long)why);
            flag = (keep && !why) ? KEPT : DROPPED;
        }
        flags[r] = flag;
    }
    if constexpr (VIEW == SPLIT) {
        const int before = __shfl_up(listed_id, 1, 64);
        if (listed_id >= 0 && ((threadIdx.x & 63) == 0 || before != listed_id)) S.listed[listed_id] = 1;
    }
    count_pair(flag != NOT_EMITTED, flag == KEPT, wg_emitted, wg_kept);
}

// the kept rows of a workgroup behind its kept rank: row number and the columns the formatter and k2_extras read
__global__ __launch_bounds__(WG) void sr_rows(const unsigned char* __restrict__ flags, int64_t n_rows, const unsigned long long* __restrict__ kept_off,
                                              int64_t n_kept, const int32_t* __restrict__ loc1, const int32_t* __restrict__ loc2,
                                              const int32_t* __restrict__ count, const double* __restrict__ p, const double* __restrict__ q,
                                              int64_t* __restrict__ rows, int32_t* __restrict__ k_loc1, int32_t* __restrict__ k_loc2,
                                              int32_t* __restrict__ k_count, double* __restrict__ k_p, double* __restrict__ k_q) {
    const int64_t r = (int64_t)blockIdx.x * WG + threadIdx.x;
    const bool kept = r < n_rows && flags[r] == KEPT;
    unsigned int total;
    const unsigned int rank = fhxscan::block_exclusive_scan(kept ? 1u : 0u, &total);
    const int64_t k = (int64_t)kept_off[blockIdx.x] + rank;
    if (kept && k < n_kept) {
        rows[k] = r;
        k_loc1[k] = loc1[r];
        k_loc2[k] = loc2[r];
        k_count[k] = count[r];
        k_p[k] = p[r];
        k_q[k] = q[r];
    }
}

// K = the kept rows as a Cols of their own (identity rebuilt from the gathered slots)
__global__ __launch_bounds__(WG) void sr_measure(Cols K, unsigned char* __restrict__ rowlen, unsigned int* __restrict__ wg_bytes,
                                                 Words* __restrict__ words) {
    const int64_t k = (int64_t)blockIdx.x * WG + threadIdx.x;
    unsigned int len = 0;
    if (k < K.n_rows) {
        char buf[288];
        len = (unsigned int)emit::row_text(K, k, emit::row_identity(K, k), buf);
        if (len == 0) atomicOr(&words->unsupported, 1u);
        rowlen[k] = (unsigned char)len;
    }
    unsigned int total;
    fhxscan::block_exclusive_scan(len, &total);
    if (threadIdx.x == 0) wg_bytes[blockIdx.x] = total;
}

// A workgroup's text out of its LDS window, whose byte `mis` is byte `at` of the output (mis = at & 15, so the window starts on a
// 16-byte boundary of the output): one 16-byte store per lane, the ragged ends bytewise, nothing at or past out_bytes
__device__ __forceinline__ void window_out(const unsigned char* window, unsigned int mis, unsigned int total, int64_t at,
                                           unsigned char* __restrict__ out, int64_t out_bytes) {
    const unsigned int lo = mis, hi = mis + total;                            // the window's bytes that are output
    const int64_t g = at - (int64_t)mis;                                      // of the window's first byte: 16 | g
    for (unsigned int j = threadIdx.x * 16u; j < hi; j += WG * 16u) {
        if (j >= lo && j + 16u <= hi && g + (int64_t)j + 16 <= out_bytes) {
            *reinterpret_cast<uint4*>(out + g + j) = *reinterpret_cast<const uint4*>(window + j);
        } else {
            for (unsigned int b = j; b < j + 16u; ++b)
                if (b >= lo && b < hi && g + (int64_t)b < out_bytes) out[g + b] = window[b];
        }
    }
}

__global__ __launch_bounds__(WG) void sr_format(Cols K, const unsigned char* __restrict__ rowlen, const unsigned long long* __restrict__ wg_off,
                                                unsigned char* __restrict__ out, int64_t out_bytes, Words* __restrict__ words) {
    __shared__ __attribute__((aligned(16))) unsigned char window[WINDOW];
    const int64_t k = (int64_t)blockIdx.x * WG + threadIdx.x;
    const unsigned int len = k < K.n_rows ? (unsigned int)rowlen[k] : 0u;
    unsigned int total;
    const unsigned int pre = fhxscan::block_exclusive_scan(len, &total);
    const int64_t at = (int64_t)wg_off[blockIdx.x];
    const unsigned int mis = (unsigned int)(at & 15);                         // the window starts on a 16-byte boundary of the output
    if (len) {
        char buf[288];
        const unsigned int n = (unsigned int)emit::row_text(K, k, emit::row_identity(K, k), buf);
        if (n != len) atomicOr(&words->internal, 1u);
        else
            for (unsigned int j = 0; j < n; ++j) window[mis + pre + j] = (unsigned char)buf[j];     // mis + pre + n <= 15 + 256 * 191
    }
    __syncthreads();
    window_out(window, mis, total, at, out, out_bytes);
}

// the doubles nearest the %e field of `key` (0: below every numeric field) and of the key after it (none: +inf)
inline void bracket_of(uint64_t key, double* lo, double* hi) {
    auto field_value = [](uint64_t k) {
        char text[32];
        std::snprintf(text, sizeof(text), "%llu.%06llue%+03d", (unsigned long long)(k % msd::KEY_EXP / 1000000ull),
                      (unsigned long long)(k % 1000000ull), (int)(k / msd::KEY_EXP) - 308);
        return std::strtod(text, nullptr);
    };
    const uint64_t lowest = 0ull * msd::KEY_EXP + 2225074ull, highest = 615ull * msd::KEY_EXP + 9999999ull;      // e-308 ... e+307
    if (key < lowest) {
        *lo = 0.0;
        *hi = field_value(lowest);
        return;
    }
    *lo = field_value(key);
    if (key >= highest) {
        *hi = HUGE_VAL;
        return;
    }
    const uint64_t next = key % msd::KEY_EXP == 9999999ull ? (key / msd::KEY_EXP + 1) * msd::KEY_EXP + 1000000ull : key + 1;
    *hi = field_value(next);
}

// the smallest double that C's %e prints with an exponent of 308 (rounding to seven digits is monotone)
inline double first_e308() {
    auto is_308 = [](double v) {
        char text[32];
        std::snprintf(text, sizeof(text), "%e", v);
        return std::strstr(text, "e+308") != nullptr;
    };
    double v = std::strtod("9.9999995e+307", nullptr);
    while (is_308(v)) v = std::nextafter(v, 0.0);
    while (!is_308(v)) v = std::nextafter(v, HUGE_VAL);
    return v;
}

}  // namespace fhx::sigres

namespace {

const char* const kNotCovered = "a row does not fit the device formatter (name longer than 24 bytes, a value of 2^63 or more, or a row of 192 "
                                "bytes or more): select from the written file";
const char* const kMoreText = "more text than the kept rows can hold";

// One call's state: what the decision over the loaded rows leaves on the device (sr_decide and the two rank scans), what
// format_kept adds, and the host clocks of the stages the call's FHX_TIMING line names.  G owns every block until the call returns.
struct Decided {
    DeviceScratch G;
    fhx::sigres::Words words;                  // the host's copy, as read_words last saw the device's
    fhx::sigres::Words* d_words = nullptr;
    unsigned char* d_flags = nullptr;
    unsigned long long* d_kept_off = nullptr;
    char* d_names = nullptr;
    int32_t* d_name_off = nullptr;
    int32_t n_names = 0;
    unsigned char* d_listed = nullptr;         // SPLIT: one byte per chromosome id
    int64_t n = 0, n_wg = 0, emitted = 0, kept = 0;
    // format_kept: the kept rows' text, its bytes, every row's length and every workgroup's first byte
    unsigned char *d_out = nullptr, *d_len = nullptr;
    unsigned long long* d_wg_off = nullptr;
    int64_t bytes = 0;
    const bool timing = std::getenv("FHX_TIMING") != nullptr;
    double s[6] = {0, 0, 0, 0, 0, 0};
    StageClock T{s};
};

// the device's words into F.words; the stream is idle afterwards
int read_words(fhx_ctx* ctx, Decided& F) {
    FHX_HIP(hipMemcpyAsync(&F.words, F.d_words, sizeof(F.words), hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipStreamSynchronize(ctx->stream));
    return FHX_OK;
}

// a stage boundary the call pays for only under FHX_TIMING: it synchronises the stream
int timed_mark(fhx_ctx* ctx, Decided& F, int stage) {
    if (!F.timing) return FHX_OK;
    FHX_HIP(hipStreamSynchronize(ctx->stream));
    F.T.mark(stage);
    return FHX_OK;
}

// in front of every walk over the caller's names
int require_names(fhx_ctx* ctx, const char* const* chr_names, int32_t n_names) {
    for (int i = 0; i < n_names; ++i)
        if (!chr_names[i]) return fail(ctx, FHX_ERR_ARG, "a chromosome name is missing");
    return FHX_OK;
}

// The kept rows compacted in file order with the columns behind them (sr_rows), and what kept_extras adds
struct KeptRows {
    int64_t* d_rows = nullptr;
    int32_t *d_loc1 = nullptr, *d_loc2 = nullptr, *d_count = nullptr;
    double *d_p = nullptr, *d_q = nullptr, *d_b1 = nullptr, *d_b2 = nullptr, *d_e = nullptr;
};

// The state rules, the decision and its refusals, shared by fhx_significant_select and fhx_significant_track (TRACK: the track's
// rules for midpoints and names on every emitted row; SPLIT: `name_why` holds the reason per chromosome id, and F.d_listed says
// afterwards which ids the file lists).  F.n == 0: the context holds no rows and nothing was launched.
template <int VIEW>
int decide_rows(fhx_ctx* ctx, const char* const* chr_names, int32_t n_names, const char* fdr_text, int32_t fdr_len, uint64_t key_bound,
                int32_t zero_kept, int32_t strict, int32_t* why, int64_t* bad_line, Decided& F,
                const std::vector<unsigned char>* name_why = nullptr) {
    using namespace fhx::sigres;
    StageClock& T = F.T;
    if (ctx->device < 0) return fail(ctx, FHX_ERR_NO_DEVICE, "host-only context");
    if (!ctx->have_p || !ctx->have_q) return fail(ctx, FHX_ERR_ARG, "p and q must have been computed (fhx_pvalues, fhx_bh)");
    if (ctx->outliers_folded) return fail(ctx, FHX_ERR_ARG, "fhx_next_pass has closed the pass: select before it");
    Decision D;
    std::memset(&D, 0, sizeof(D));
    if (!msd::fdr_of(fdr_text, fdr_len, &D.fdr)) {
        *why = FHX_MS_FDR;
        return fail(ctx, FHX_ERR_UNSUPPORTED, "the text of fdr must have 1 to " + std::to_string(FHX_MS_FDR_BYTES) + " bytes");
    }
    if (!ctx->d_loc1 || !ctx->d_slot_chr || (!ctx->nonfixed && !ctx->d_grid) || (ctx->nonfixed && !ctx->d_slot_mid))
        return fail(ctx, FHX_ERR_ARG, "no resident rows to rebuild the identity columns from");
    FHX_HIP(hipSetDevice(ctx->device));
    FHX_HIP(hipStreamSynchronize(ctx->stream));       // K3 is through: had it seen more survivors than it was sized for, say so
    if (const int rc = check_fault(ctx)) return rc;
    const int64_t n = ctx->n_rows;
    F.n = n;
    if (n == 0) return FHX_OK;
    T.last = std::chrono::steady_clock::now();
    D.key_bound = key_bound;
    D.zero_kept = zero_kept;
    D.strict = strict;
    D.bracket = std::getenv("FHX_SR_NO_BRACKET") ? 0 : 1;
    bracket_of(key_bound, &D.lo, &D.hi);
    D.e308 = first_e308();
    if (const int rc = require_names(ctx, chr_names, n_names)) return rc;
    std::vector<char> blob;
    std::vector<int32_t> name_off(n_names + 1, 0);
    for (int i = 0; i < n_names; ++i) {
        const size_t l = std::strlen(chr_names[i]);
        blob.insert(blob.end(), chr_names[i], chr_names[i] + l);
        name_off[i + 1] = (int32_t)blob.size();
    }
    if (blob.empty()) blob.push_back(0);
    const int64_t n_wg = (n + WG - 1) / WG;
    F.n_wg = n_wg;
    DeviceScratch& G = F.G;
    unsigned int *d_wg_emitted = nullptr, *d_wg_kept = nullptr;
    unsigned long long* d_emit_off = nullptr;
    FHX_HIP(G.get(&F.d_flags, (size_t)n));
    FHX_HIP(G.get(&d_wg_emitted, (size_t)n_wg * 4));
    FHX_HIP(G.get(&d_wg_kept, (size_t)n_wg * 4));
    FHX_HIP(G.get(&d_emit_off, (size_t)n_wg * 8));
    FHX_HIP(G.get(&F.d_kept_off, (size_t)n_wg * 8));
    FHX_HIP(G.get(&F.d_words, sizeof(Words)));
    FHX_HIP(G.get(&F.d_names, blob.size()));
    FHX_HIP(G.get(&F.d_name_off, name_off.size() * 4));
    Words& words = F.words;
    std::memset(&words, 0, sizeof(words));
    words.first_bad = NO_BAD_ROW;
    FHX_HIP(hipMemcpyAsync(F.d_words, &words, sizeof(words), hipMemcpyHostToDevice, ctx->stream));
    FHX_HIP(hipMemcpyAsync(F.d_names, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream));
    FHX_HIP(hipMemcpyAsync(F.d_name_off, name_off.data(), name_off.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    F.n_names = n_names;
    // every loaded row: identity from the resident slots, q resident; p, the biases and ExpCC are not read by sr_decide
    const Cols C = fhx::emit::resident_cols(ctx, F.d_names, F.d_name_off, n_names);
    SplitTables S{nullptr, nullptr};
    if (VIEW == SPLIT) {
        if (!name_why || (int32_t)name_why->size() != n_names) return fail(ctx, FHX_ERR_INTERNAL, "the split has no reason per chromosome id");
        unsigned char* d_name_why = nullptr;
        FHX_HIP(G.get(&d_name_why, (size_t)n_names));
        FHX_HIP(G.get(&F.d_listed, (size_t)n_names));
        FHX_HIP(hipMemcpyAsync(d_name_why, name_why->data(), (size_t)n_names, hipMemcpyHostToDevice, ctx->stream));
        FHX_HIP(hipMemsetAsync(F.d_listed, 0, (size_t)n_names, ctx->stream));
        S = SplitTables{d_name_why, F.d_listed};
    }
    hipLaunchKernelGGL(sr_decide<VIEW>, dim3((unsigned)n_wg), dim3(WG), 0, ctx->stream, C, D, F.d_flags, d_wg_emitted, d_wg_kept, F.d_words, S);
    FHX_HIP(hipGetLastError());
    if (const int rc = timed_mark(ctx, F, 0)) return rc;
    hipLaunchKernelGGL(fhxscan::scan_tiles, dim3(1), dim3(fhxscan::THREADS), 0, ctx->stream, (const unsigned int*)d_wg_emitted, n_wg, d_emit_off,
                       &F.d_words->n_emitted);
    hipLaunchKernelGGL(fhxscan::scan_tiles, dim3(1), dim3(fhxscan::THREADS), 0, ctx->stream, (const unsigned int*)d_wg_kept, n_wg, F.d_kept_off,
                       &F.d_words->n_kept);
    FHX_HIP(hipGetLastError());
    if (const int rc = read_words(ctx, F)) return rc;
    T.mark(1);
    if (words.first_bad != NO_BAD_ROW) {
        // the line the row has in the file the pass writes: the header, then the emitted rows before it
        const int64_t bad_row = (int64_t)(words.first_bad >> 8), wg = bad_row / WG;
        unsigned long long before = 0;
        unsigned char head[WG];
        FHX_HIP(hipMemcpyAsync(&before, d_emit_off + wg, 8, hipMemcpyDeviceToHost, ctx->stream));
        FHX_HIP(hipMemcpyAsync(head, F.d_flags + wg * WG, (size_t)(bad_row - wg * WG + 1), hipMemcpyDeviceToHost, ctx->stream));
        FHX_HIP(hipStreamSynchronize(ctx->stream));
        for (int64_t k = 0; k < bad_row - wg * WG; ++k) before += head[k] != NOT_EMITTED;
        *why = (int32_t)(words.first_bad & 0xFFu);
        *bad_line = 2 + (int64_t)before;
        return fail(ctx, FHX_ERR_UNSUPPORTED, "line " + std::to_string(*bad_line) + " of the pass's file (loaded row " + std::to_string(bad_row) +
                                                  ") is outside the device grammar (reason " + std::to_string(*why) + ")");
    }
    if (words.unsupported) return fail(ctx, FHX_ERR_UNSUPPORTED, kNotCovered);
    F.emitted = (int64_t)words.n_emitted;
    F.kept = (int64_t)words.n_kept;
    if (F.emitted > n || F.kept > F.emitted) return fail(ctx, FHX_ERR_INTERNAL, "more kept rows than emitted ones");
    return FHX_OK;
}

// sr_rows over a decision with kept rows; nothing is synchronised
int gather_kept(fhx_ctx* ctx, Decided& F, KeptRows& R) {
    using namespace fhx::sigres;
    const int64_t kept = F.kept;
    FHX_HIP(F.G.get(&R.d_rows, (size_t)kept * 8));
    FHX_HIP(F.G.get(&R.d_loc1, (size_t)kept * 4));
    FHX_HIP(F.G.get(&R.d_loc2, (size_t)kept * 4));
    FHX_HIP(F.G.get(&R.d_count, (size_t)kept * 4));
    FHX_HIP(F.G.get(&R.d_p, (size_t)kept * 8));
    FHX_HIP(F.G.get(&R.d_q, (size_t)kept * 8));
    hipLaunchKernelGGL(sr_rows, dim3((unsigned)F.n_wg), dim3(WG), 0, ctx->stream, (const unsigned char*)F.d_flags, F.n,
                       (const unsigned long long*)F.d_kept_off, kept, (const int32_t*)ctx->d_loc1, (const int32_t*)ctx->d_loc2,
                       (const int32_t*)ctx->d_count, (const double*)ctx->d_p, (const double*)ctx->d_q, R.d_rows, R.d_loc1, R.d_loc2, R.d_count, R.d_p,
                       R.d_q);
    FHX_HIP(hipGetLastError());
    return FHX_OK;
}

// ExpCC and the biases of the rows R as the writer prints them (fithic.py:1075-1078, :1105-1108); nothing is synchronised
int kept_extras(fhx_ctx* ctx, Decided& F, KeptRows& R) {
    FHX_HIP(F.G.get(&R.d_b1, (size_t)F.kept * 8));
    FHX_HIP(F.G.get(&R.d_b2, (size_t)F.kept * 8));
    FHX_HIP(F.G.get(&R.d_e, (size_t)F.kept * 8));
    K2Params P = make_k2_params(ctx);
    P.loc1 = R.d_loc1;
    P.loc2 = R.d_loc2;
    P.count = R.d_count;
    P.n = F.kept;
    launch_k2_extras(ctx, P, F.kept, R.d_e, R.d_b1, R.d_b2);
    FHX_HIP(hipGetLastError());
    return FHX_OK;
}

// the kept rows R as a Cols of their own: identity rebuilt from the gathered slots, the biases and ExpCC null without kept_extras
fhx::emit::Cols kept_cols(const fhx_ctx* ctx, const Decided& F, const KeptRows& R) {
    fhx::emit::Cols K = fhx::emit::resident_cols(ctx, F.d_names, F.d_name_off, F.n_names);
    K.count = R.d_count;
    K.loc1 = R.d_loc1;
    K.loc2 = R.d_loc2;
    K.p = R.d_p;
    K.q = R.d_q;
    K.b1 = R.d_b1;
    K.b2 = R.d_b2;
    K.expcc = R.d_e;
    K.n_rows = F.kept;
    return K;
}

// sr_measure, the byte scan, sr_format: F.d_out, F.bytes, F.d_len, F.d_wg_off.  between() enqueues what a caller wants behind the
// scan; the first read-back follows it, and `internal_before` is the message for an `internal` word it shows (raised by the
// caller's own kernels in front of this call; nullptr: there are none).  The stream is idle afterwards.
template <typename Between>
int format_kept(fhx_ctx* ctx, Decided& F, const fhx::emit::Cols& K, Between between, const char* internal_before) {
    using namespace fhx::sigres;
    const int64_t kept = F.kept, k_wg = (kept + WG - 1) / WG;
    unsigned int* d_wg_bytes = nullptr;
    FHX_HIP(F.G.get(&F.d_len, (size_t)kept));
    FHX_HIP(F.G.get(&d_wg_bytes, (size_t)k_wg * 4));
    FHX_HIP(F.G.get(&F.d_wg_off, (size_t)k_wg * 8));
    hipLaunchKernelGGL(sr_measure, dim3((unsigned)k_wg), dim3(WG), 0, ctx->stream, K, F.d_len, d_wg_bytes, F.d_words);
    hipLaunchKernelGGL(fhxscan::scan_tiles, dim3(1), dim3(fhxscan::THREADS), 0, ctx->stream, (const unsigned int*)d_wg_bytes, k_wg, F.d_wg_off,
                       &F.d_words->n_bytes);
    between();
    FHX_HIP(hipGetLastError());
    if (const int rc = read_words(ctx, F)) return rc;
    if (F.words.unsupported) return fail(ctx, FHX_ERR_UNSUPPORTED, kNotCovered);
    if (internal_before && F.words.internal) return fail(ctx, FHX_ERR_INTERNAL, internal_before);
    F.bytes = (int64_t)F.words.n_bytes;
    if (F.bytes <= 0 || F.bytes > kept * (int64_t)fhx::emit::ROW_STRIDE) return fail(ctx, FHX_ERR_INTERNAL, kMoreText);
    FHX_HIP(F.G.get(&F.d_out, (size_t)F.bytes));
    hipLaunchKernelGGL(sr_format, dim3((unsigned)k_wg), dim3(WG), 0, ctx->stream, K, (const unsigned char*)F.d_len,
                       (const unsigned long long*)F.d_wg_off, F.d_out, F.bytes, F.d_words);
    FHX_HIP(hipGetLastError());
    if (const int rc = read_words(ctx, F)) return rc;
    if (F.words.internal) return fail(ctx, FHX_ERR_INTERNAL, "the formatter wrote another length than it measured");
    return FHX_OK;
}

}  // namespace

extern "C" {

int fhx_significant_select(fhx_ctx* ctx, const char* const* chr_names, int32_t n_names, const char* fdr_text, int32_t fdr_len, uint64_t key_bound,
                           int32_t zero_kept, int32_t strict, int64_t* n_emitted, int64_t* n_kept, int64_t* n_bytes, int32_t* why,
                           int64_t* bad_line) {
    using namespace fhx::sigres;
    if (!ctx || !chr_names || n_names <= 0 || !fdr_text || !n_emitted || !n_kept || !n_bytes || !why || !bad_line) return FHX_ERR_ARG;
    *n_emitted = *n_kept = *n_bytes = 0;
    *why = FHX_MS_OK;
    *bad_line = 0;
    std::vector<char>().swap(ctx->sig_text);
    std::vector<int64_t>().swap(ctx->sig_rows);
    Decided F;                                         // stages: decide, rank scans, rows + ExpCC/bias, measure + format, copy out
    if (const int rc = decide_rows<SUBSET>(ctx, chr_names, n_names, fdr_text, fdr_len, key_bound, zero_kept, strict, why, bad_line, F)) return rc;
    if (F.n == 0) return FHX_OK;
    const int64_t kept = F.kept;
    std::vector<char> text;
    std::vector<int64_t> rows((size_t)kept);
    if (kept > 0) {
        KeptRows R;
        if (const int rc = gather_kept(ctx, F, R)) return rc;
        if (const int rc = kept_extras(ctx, F, R)) return rc;
        if (const int rc = timed_mark(ctx, F, 2)) return rc;
        if (const int rc = format_kept(ctx, F, kept_cols(ctx, F, R), [] {}, nullptr)) return rc;
        F.T.mark(3);
        text.resize((size_t)F.bytes);
        FHX_HIP(hipMemcpyAsync(text.data(), F.d_out, (size_t)F.bytes, hipMemcpyDeviceToHost, ctx->stream));
        FHX_HIP(hipMemcpyAsync(rows.data(), R.d_rows, (size_t)kept * 8, hipMemcpyDeviceToHost, ctx->stream));
        FHX_HIP(hipStreamSynchronize(ctx->stream));
        F.T.mark(4);
    }
    ctx->sig_text.swap(text);
    ctx->sig_rows.swap(rows);
    *n_emitted = F.emitted;
    *n_kept = kept;
    *n_bytes = (int64_t)ctx->sig_text.size();
    if (F.timing)
        std::fprintf(stderr, "fhx_significant_select: %lld rows, %lld emitted, %lld kept (%lld bytes): decide %.6f s; rank scans %.6f s; "
                     "rows + ExpCC/bias %.6f s; measure + format %.6f s; copy out %.6f s\n", (long long)F.n, (long long)F.emitted, (long long)kept,
                     (long long)*n_bytes, F.s[0], F.s[1], F.s[2], F.s[3], F.s[4]);
    return FHX_OK;
}

int fhx_significant_copy_text(fhx_ctx* ctx, void* dst, int64_t capacity) {
    if (!ctx || capacity < (int64_t)ctx->sig_text.size() || (!dst && !ctx->sig_text.empty())) return FHX_ERR_ARG;
    if (!ctx->sig_text.empty()) std::memcpy(dst, ctx->sig_text.data(), ctx->sig_text.size());
    return FHX_OK;
}

int fhx_significant_copy_rows(fhx_ctx* ctx, int64_t* rows, int64_t capacity) {
    if (!ctx || capacity < (int64_t)ctx->sig_rows.size() || (!rows && !ctx->sig_rows.empty())) return FHX_ERR_ARG;
    if (!ctx->sig_rows.empty()) std::memcpy(rows, ctx->sig_rows.data(), ctx->sig_rows.size() * sizeof(int64_t));
    return FHX_OK;
}

}  // extern "C"

#include "fhx_sigresident_track.inc"
#include "fhx_sigresident_split.inc"
