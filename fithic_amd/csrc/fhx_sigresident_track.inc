// fhx_sigresident_track.inc - the UCSC interact track of a pass taken from its RESIDENT columns (included at the end of
// fhx_sigresident.hip, at file scope): what fhx_ms_track_file gives for the file fhx_write_significances_device
// writes, without the file.  The decision is fhx_sigresident.hip's made strict (`$7 < q`), with the track's rules for midpoints
// and names on every emitted row (sr_decide<TRACK>); the line is fhx_trackline.hpp's, shared with the file route.  Line 1 of the
// pass's file is fithic's header, which the file route drops and counts: here it is only counted.  Behind sr_decide, the two rank
// scans and sr_rows (the kept rows compacted in file order; ExpCC and the biases are not in a track line, so k2_extras does not run):
//
//   srt_line       one kept row per lane: q -> fmt_e6 -> classify (a row the bracket decided unformatted gets its text here), the
//                  midpoints and names of its identity, the score certified or the row marked DEFERRED; an info word per row
//                  (the length without NR | DEFERRED).  Per workgroup: deferred rows.
//   scan_tiles     the slot of every workgroup's first deferred row
//   srt_defer      the %e text of q of the deferred rows, 16 bytes a slot; the host answers inside the same C call with
//                  fhx::score::host_fields, 32 bytes a slot
//   srt_measure    NR = kept rank + 1 (the row's place in the compacted order: the scan's, never an atomic); the final length =
//                  + the digits of NR + the host's score bytes.  Per workgroup: bytes.
//   scan_tiles     the workgroup's byte offset
//   srt_format     256 kept rows per workgroup into ONE LDS window sized from the longest line two 24-byte names can give
//                  (trackline::max_line(24) = 208 bytes, against the writer's 192-byte row): 256 * 208 + 16 = 53 264 bytes, which
//                  leaves three workgroups (12 waves) a CU of 160 KB - the same three sr_format's 49 168 bytes leave - instead of
//                  ut_format's loop over 16 KB windows, which formats a line once per window it touches.  The window starts on a
//                  16-byte boundary of the output and goes out by sr_format's scheme (window_out); what a lane wrote is compared
//                  with what srt_measure counted.
// A kept row with a name of 25 to 63 bytes is FHX_ERR_UNSUPPORTED (row_text's cap): the caller takes the file route.
namespace fhx::sigres {

namespace tl = fhx::trackline;

constexpr int TRACK_NAME = 24;                                   // the device identity formatter's cap (emit::row_text)
constexpr int TRACK_STRIDE = tl::max_line(TRACK_NAME);           // 208
constexpr int TRACK_WINDOW = WG * TRACK_STRIDE + 16;
static_assert(TRACK_WINDOW <= 65536, "the window is one workgroup's static LDS");
static_assert(TRACK_STRIDE < (int)tl::DEFERRED, "a length fits the info word");

// the pieces of kept row k as the track line takes them
struct TrackRow {
    const unsigned char *name1, *name3;
    int n1, n3, v2, v4, cls, fn;
    unsigned long long key;
    unsigned char field[16];                   // at most -D.DDDDDDe-XXX
};

// 0: the pieces are there; 1: a name the device formatter does not cover; 2: a q sr_decide should not have kept
__device__ __forceinline__ int track_row(const Cols& K, int64_t k, TrackRow& T) {
    const RowId id = emit::row_identity(K, k);
    T.n1 = name_bytes(K, id.c1);
    T.n3 = name_bytes(K, id.c2);
    if (T.n1 < 1 || T.n3 < 1 || T.n1 > TRACK_NAME || T.n3 > TRACK_NAME) return 1;
    T.name1 = (const unsigned char*)K.names + K.name_off[id.c1];
    T.name3 = (const unsigned char*)K.names + K.name_off[id.c2];
    T.v2 = id.m1;
    T.v4 = id.m2;
    T.key = 0;
    T.fn = fmt::fmt_e6(K.q[k], (char*)T.field);
    T.cls = T.fn > 0 ? msd::classify(T.field, 0, T.fn, &T.key) : 0;
    return T.cls != 0 && tl::midpoint_ok(T.v2) && tl::midpoint_ok(T.v4) ? 0 : 2;
}

__global__ __launch_bounds__(WG) void srt_line(Cols K, unsigned short* __restrict__ info, unsigned int* __restrict__ wg_deferred,
                                               Words* __restrict__ words) {
    const int64_t k = (int64_t)blockIdx.x * WG + threadIdx.x;
    unsigned int word = 0;
    if (k < K.n_rows) {
        TrackRow T;
        const int bad = track_row(K, k, T);
        if (bad == 1) atomicOr(&words->unsupported, 1u);
        else if (bad) atomicOr(&words->internal, 1u);
        else {
            char score[score::MAX_TEXT];
            word = tl::line_word(T.n1, T.n3, T.v2, T.v4, tl::score_text(T.cls, T.key, score));
        }
        info[k] = (unsigned short)word;
    }
    unsigned int total;
    fhxscan::block_exclusive_scan((word & tl::DEFERRED) ? 1u : 0u, &total);
    if (threadIdx.x == 0) wg_deferred[blockIdx.x] = total;
}

__global__ __launch_bounds__(WG) void srt_defer(Cols K, const unsigned short* __restrict__ info, const unsigned long long* __restrict__ deferred_off,
                                                unsigned char* __restrict__ fields, int64_t n_slots) {
    const int64_t k = (int64_t)blockIdx.x * WG + threadIdx.x;
    const bool mine = k < K.n_rows && (info[k] & tl::DEFERRED);
    unsigned int total;
    const int64_t slot = (int64_t)deferred_off[blockIdx.x] + fhxscan::block_exclusive_scan(mine ? 1u : 0u, &total);
    if (mine && slot < n_slots) {
        unsigned char field[16];
        const int fn = fmt::fmt_e6(K.q[k], (char*)field);
        tl::defer_field(fields, slot, field, fn > 0 ? fn : 0);
    }
}

__global__ __launch_bounds__(WG) void srt_measure(int64_t n_kept, unsigned short* __restrict__ info, const unsigned long long* __restrict__ deferred_off,
                                                  const unsigned char* __restrict__ scores, int64_t n_slots, unsigned int* __restrict__ wg_bytes) {
    const int64_t k = (int64_t)blockIdx.x * WG + threadIdx.x;
    const unsigned int word = k < n_kept ? (unsigned int)info[k] : 0u;
    unsigned int total;
    const unsigned int rank = fhxscan::block_exclusive_scan((word & tl::DEFERRED) ? 1u : 0u, &total);
    unsigned int len = 0;
    if (word) {
        const unsigned int done = tl::final_word(word, k + 1, scores, (int64_t)deferred_off[blockIdx.x] + rank, n_slots);
        info[k] = (unsigned short)done;
        len = done & ~tl::DEFERRED;
    }
    fhxscan::block_exclusive_scan(len, &total);
    if (threadIdx.x == 0) wg_bytes[blockIdx.x] = total;
}

// a lane's line into the window: nothing at or past `end`, whatever the writer does
struct LdsSink {
    unsigned char* lds;
    unsigned int pos, end;
    __device__ void put(int c) {
        if (pos < end) lds[pos] = (unsigned char)c;
        ++pos;
    }
};

__global__ __launch_bounds__(WG) void srt_format(Cols K, const unsigned short* __restrict__ info, const unsigned long long* __restrict__ deferred_off,
                                                 const unsigned char* __restrict__ scores, int64_t n_slots,
                                                 const unsigned long long* __restrict__ wg_off, unsigned char* __restrict__ out, int64_t out_bytes,
                                                 Words* __restrict__ words) {
    __shared__ __attribute__((aligned(16))) unsigned char window[TRACK_WINDOW];
    const int64_t k = (int64_t)blockIdx.x * WG + threadIdx.x;
    const unsigned int word = k < K.n_rows ? (unsigned int)info[k] : 0u;
    const bool deferred = (word & tl::DEFERRED) != 0;
    unsigned int len = word & ~tl::DEFERRED;
    if (len > (unsigned int)TRACK_STRIDE) {                                   // srt_measure cannot have counted this
        atomicOr(&words->internal, 1u);
        len = 0;
    }
    unsigned int total;
    const unsigned int rank = fhxscan::block_exclusive_scan(deferred ? 1u : 0u, &total);
    const unsigned int pre = fhxscan::block_exclusive_scan(len, &total);
    const int64_t at = (int64_t)wg_off[blockIdx.x];
    const unsigned int mis = (unsigned int)(at & 15);                         // the window starts on a 16-byte boundary of the output
    if (len) {
        TrackRow T;
        if (track_row(K, k, T)) atomicOr(&words->internal, 1u);
        else {
            char score[score::MAX_TEXT];
            const int score_len = deferred ? tl::host_score(scores, (int64_t)deferred_off[blockIdx.x] + rank, n_slots, score)
                                           : tl::score_text(T.cls, T.key, score);
            LdsSink s{window, mis + pre, mis + pre + len};                     // mis + pre + len <= 15 + 256 * 208
            tl::write_line(s, T.name1, T.n1, T.v2, T.name3, T.n3, T.v4, k + 1, score, score_len);
            if (s.pos != s.end) atomicOr(&words->internal, 1u);
        }
    }
    __syncthreads();
    window_out(window, mis, total, at, out, out_bytes);
}

}  // namespace fhx::sigres

extern "C" {

int fhx_significant_track(fhx_ctx* ctx, const char* const* chr_names, int32_t n_names, const char* fdr_text, int32_t fdr_len, uint64_t key_bound,
                          int32_t zero_kept, int64_t* n_emitted, int64_t* n_kept, int64_t* n_deferred, int64_t* n_bytes, int32_t* why,
                          int64_t* bad_line) {
    using namespace fhx::sigres;
    if (!ctx || !chr_names || n_names <= 0 || !fdr_text || !n_emitted || !n_kept || !n_deferred || !n_bytes || !why || !bad_line) return FHX_ERR_ARG;
    *n_emitted = *n_kept = *n_deferred = *n_bytes = 0;
    *why = FHX_MS_OK;
    *bad_line = 0;
    std::vector<char>().swap(ctx->sig_track);
    Decided F;                                 // stages: decide, rank scans, rows + lines, deferred round trip, measure + format, copy out
    StageClock& T = F.T;
    if (const int rc = decide_rows<TRACK>(ctx, chr_names, n_names, fdr_text, fdr_len, key_bound, zero_kept, /*strict=*/1, why, bad_line, F)) return rc;
    const int64_t kept = F.kept;
    if (kept > (int64_t)INT32_MAX) {
        *why = FHX_MS_KEPT;
        return fail(ctx, FHX_ERR_UNSUPPORTED, "more than 2^31 - 1 rows pass: awk prints NR as an integer only below 2^31");
    }
    std::vector<char> text(tl::HEAD, tl::HEAD + sizeof(tl::HEAD) - 1);         // the script's two fixed lines
    int64_t n_slots = 0;
    if (kept > 0) {
        DeviceScratch& G = F.G;
        Words& words = F.words;
        Words* d_words = F.d_words;
        const int64_t k_wg = (kept + WG - 1) / WG;
        KeptRows R;
        unsigned short* d_info = nullptr;
        unsigned int *d_wg_deferred = nullptr, *d_wg_bytes = nullptr;
        unsigned long long *d_deferred_off = nullptr, *d_wg_off = nullptr;
        unsigned char *d_fields = nullptr, *d_scores = nullptr, *d_out = nullptr;
        FHX_HIP(G.get(&d_info, (size_t)kept * 2));
        FHX_HIP(G.get(&d_wg_deferred, (size_t)k_wg * 4));
        FHX_HIP(G.get(&d_wg_bytes, (size_t)k_wg * 4));
        FHX_HIP(G.get(&d_deferred_off, (size_t)k_wg * 8));
        FHX_HIP(G.get(&d_wg_off, (size_t)k_wg * 8));
        if (const int rc = gather_kept(ctx, F, R)) return rc;
        const Cols K = kept_cols(ctx, F, R);
        hipLaunchKernelGGL(srt_line, dim3((unsigned)k_wg), dim3(WG), 0, ctx->stream, K, d_info, d_wg_deferred, d_words);
        hipLaunchKernelGGL(fhxscan::scan_tiles, dim3(1), dim3(fhxscan::THREADS), 0, ctx->stream, (const unsigned int*)d_wg_deferred, k_wg,
                           d_deferred_off, &d_words->n_deferred);
        FHX_HIP(hipGetLastError());
        if (const int rc = read_words(ctx, F)) return rc;
        T.mark(2);
        if (words.unsupported) return fail(ctx, FHX_ERR_UNSUPPORTED, kNotCovered);
        if (words.internal) return fail(ctx, FHX_ERR_INTERNAL, "a kept row has no track line");
        n_slots = (int64_t)words.n_deferred;
        if (n_slots > kept) return fail(ctx, FHX_ERR_INTERNAL, "more deferred rows than kept ones");
        // a buffer even without deferred rows, so that the kernels are handed no null pointer
        FHX_HIP(G.get(&d_fields, (size_t)std::max<int64_t>(n_slots, 1) * tl::DEFER_IN));
        FHX_HIP(G.get(&d_scores, (size_t)std::max<int64_t>(n_slots, 1) * tl::DEFER_OUT));
        if (n_slots > 0) {                                                    // the deferred round trip
            hipLaunchKernelGGL(srt_defer, dim3((unsigned)k_wg), dim3(WG), 0, ctx->stream, K, (const unsigned short*)d_info,
                               (const unsigned long long*)d_deferred_off, d_fields, n_slots);
            FHX_HIP(hipGetLastError());
            std::vector<unsigned char> fields((size_t)(n_slots * tl::DEFER_IN)), scores;
            FHX_HIP(hipMemcpyAsync(fields.data(), d_fields, fields.size(), hipMemcpyDeviceToHost, ctx->stream));
            FHX_HIP(hipStreamSynchronize(ctx->stream));
            if (!tl::answer_deferred(fields.data(), n_slots, &scores)) return fail(ctx, FHX_ERR_INTERNAL, "a deferred score has no text");
            FHX_HIP(hipMemcpyAsync(d_scores, scores.data(), scores.size(), hipMemcpyHostToDevice, ctx->stream));
            FHX_HIP(hipStreamSynchronize(ctx->stream));                       // `scores` leaves scope
        }
        T.mark(3);
        hipLaunchKernelGGL(srt_measure, dim3((unsigned)k_wg), dim3(WG), 0, ctx->stream, kept, d_info, (const unsigned long long*)d_deferred_off,
                           (const unsigned char*)d_scores, n_slots, d_wg_bytes);
        hipLaunchKernelGGL(fhxscan::scan_tiles, dim3(1), dim3(fhxscan::THREADS), 0, ctx->stream, (const unsigned int*)d_wg_bytes, k_wg, d_wg_off,
                           &d_words->n_bytes);
        FHX_HIP(hipGetLastError());
        if (const int rc = read_words(ctx, F)) return rc;
        const int64_t bytes = (int64_t)words.n_bytes;
        if (bytes <= 0 || bytes > kept * (int64_t)TRACK_STRIDE) return fail(ctx, FHX_ERR_INTERNAL, kMoreText);
        FHX_HIP(G.get(&d_out, (size_t)bytes));
        hipLaunchKernelGGL(srt_format, dim3((unsigned)k_wg), dim3(WG), 0, ctx->stream, K, (const unsigned short*)d_info,
                           (const unsigned long long*)d_deferred_off, (const unsigned char*)d_scores, n_slots, (const unsigned long long*)d_wg_off,
                           d_out, bytes, d_words);
        FHX_HIP(hipGetLastError());
        if (const int rc = read_words(ctx, F)) return rc;
        T.mark(4);
        if (words.internal) return fail(ctx, FHX_ERR_INTERNAL, "the track formatter wrote another length than it measured");
        const size_t head = text.size();
        text.resize(head + (size_t)bytes);
        FHX_HIP(hipMemcpyAsync(text.data() + head, d_out, (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream));
        FHX_HIP(hipStreamSynchronize(ctx->stream));
        T.mark(5);
    }
    ctx->sig_track.swap(text);
    *n_emitted = F.emitted;
    *n_kept = kept;
    *n_deferred = n_slots;
    *n_bytes = (int64_t)ctx->sig_track.size();
    if (F.timing)
        std::fprintf(stderr, "fhx_significant_track: %lld rows, %lld emitted, %lld kept, %lld deferred (%lld bytes): decide %.6f s; rank scans "
                     "%.6f s; rows + lines %.6f s; deferred round trip %.6f s; measure + format %.6f s; copy out %.6f s\n", (long long)F.n,
                     (long long)F.emitted, (long long)kept, (long long)n_slots, (long long)*n_bytes, F.s[0], F.s[1], F.s[2], F.s[3], F.s[4], F.s[5]);
    return FHX_OK;
}

int fhx_significant_copy_track(fhx_ctx* ctx, void* dst, int64_t capacity) {
    if (!ctx || capacity < (int64_t)ctx->sig_track.size() || (!dst && !ctx->sig_track.empty())) return FHX_ERR_ARG;
    if (!ctx->sig_track.empty()) std::memcpy(dst, ctx->sig_track.data(), ctx->sig_track.size());
    return FHX_OK;
}

}  // extern "C"
