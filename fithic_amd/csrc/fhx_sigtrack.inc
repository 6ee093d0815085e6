// fhx_sigtrack.inc - the UCSC interact track of the significant contacts on MI355X (gfx950); included by fhx_sigselect.hip
// (reference: fithic/utils/visualize-UCSC.sh:16-18, `awk -v q=Q '{if($7<q){print $0}}' | awk '{print $1, ($2-1), ($4+1), NR,
// int(-log($7)/log(10)), -log($7)/log(10), "EXP", "0", $1, ($2-1), ($2+1), "SOURCE_NAME", ".", $3, ($4-1), ($4+1),
// "TARGET_NAME", "+"}'` behind two fixed lines).
//
// Per batch, behind scan_text / scan_tiles of the selection:
//
//   ut_select      one line per lane, one walk over its tokens: the grammar, ms_select's decision with `$7 < q` and no line
//                  skipped - but a field 7 that starts with a letter on FILE LINE 1 is a string above every accepted threshold,
//                  and that line is only dropped - and for a kept line the bytes of its track line without NR.  The score comes
//                  from fhx_score.hpp: certified on the device, or the line is flagged DEFERRED and its score bytes are left
//                  out.  Per block: kept lines, deferred lines.
//   scan_tiles x2  -> the number of kept lines before every block (NR is this exclusive scan plus the kept lines of the
//                  earlier batches, never an atomic), and the slot of every block's first deferred line
//   ut_defer       field 7 of the deferred lines, 16 bytes a slot; the host answers with the two fields as mawk's own calls make
//                  them (fhx::score::host_fields), 32 bytes a slot
//   ut_measure     the final length of every track line: + the digits of NR, + the host's score bytes.  Per block: bytes.
//   scan_tiles     -> the offset of every block's lines in the track
//   ut_format      256 lines per round, their lengths scanned; every lane writes its line into a 16 KB window of LDS (a round
//                  longer than that takes several windows; a lane writes only what falls into the current one), and the
//                  window goes out with consecutive lanes on consecutive bytes.  Order is file order.
// What a line is made of - the grammar beyond field 7, its length, the DEFERRED marking, the writer - is fhx_trackline.hpp.
// A track line can be two and a half times its input line, so nothing here is sized by the input: d_out grows to what ut_measure found.
namespace utd {

using namespace fhxlines;
using namespace msd;
using namespace fhx::trackline;           // the line itself: fhx_trackline.hpp, shared with the resident route

constexpr int WINDOW = 16384;                  // LDS bytes of ut_format

struct TrackWords {
    unsigned long long first_error;
    unsigned long long kept_lines;             // scan_tiles' totals of the current batch
    unsigned long long deferred;
    unsigned long long out_bytes;
};

// ---- the selection, the grammar and the length of every kept line without NR ---------------------------------------------------
__global__ __launch_bounds__(WG) void ut_select(const unsigned char* __restrict__ text, int64_t T, const unsigned long long* __restrict__ block_off,
                                                int64_t n_lines_batch, int64_t line_base, Fdr fdr, unsigned long long key_bound, int zero_kept,
                                                int check_bytes, unsigned short* __restrict__ info, unsigned int* __restrict__ block_kept,
                                                unsigned int* __restrict__ block_deferred, TrackWords* __restrict__ words) {
    __shared__ unsigned short lstart[LSTART_ENTRIES];
    const BlockLines B = block_lines(text, T, block_off, lstart);
    unsigned int my_kept = 0, my_deferred = 0;
    for (int e = threadIdx.x; e < B.n_lines; e += WG) {
        const int64_t r = B.row0 + e;
        const int64_t start = B.b0 + lstart[e];
        Line L;
        walk(text, T, start, check_bytes, L);
        int why = L.why, cls = 0, v2 = 0, v4 = 0;
        unsigned long long key = 0;
        bool keep = false;
        if (!why && r >= n_lines_batch) why = FHX_MS_INTERNAL;                // the scan and this kernel disagree about the lines
        if (!why && L.tok < 7) why = FHX_MS_TOKENS;
        const int f0 = why ? 0 : (int)text[start + L.fb] | 0x20;
        const bool header = !why && line_base + r == 0 && f0 >= 'a' && f0 <= 'z';       // `q-value`: a string, and above every q
        if (!why && !header) {
            cls = classify(text, start + L.fb, L.fn, &key);
            v2 = midpoint(text, start + L.b2, L.n2);
            v4 = midpoint(text, start + L.b4, L.n4);
            why = refusal(cls, v2 >= 0 && v4 >= 0, L.n1, L.n3);                 // class 0 first; with a reason nothing of the file is kept
            if (!why) why = decide(cls, key, key_bound, zero_kept, /*strict=*/1, text, start + L.fb, L.fn, fdr, &keep);
        }
        if (why) atomicMin(&words->first_error, error_word(line_base + r + 1, why));
        unsigned int word = 0;
        if (keep && !why) {
            char buf[fhx::score::MAX_TEXT];
            word = line_word(L.n1, L.n3, v2, v4, score_text(cls, key, buf));
            if (word & DEFERRED) ++my_deferred;
            ++my_kept;
        }
        if (r < n_lines_batch) info[r] = (unsigned short)word;
    }
    unsigned int total_kept, total_deferred;
    fhxscan::block_exclusive_scan(my_kept, &total_kept);                      // every lane of the block arrives here
    fhxscan::block_exclusive_scan(my_deferred, &total_deferred);
    if (threadIdx.x == 0) {
        block_kept[blockIdx.x] = total_kept;
        block_deferred[blockIdx.x] = total_deferred;
    }
}

// ---- field 7 of the deferred lines, in file order ------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void ut_defer(const unsigned char* __restrict__ text, int64_t T, const unsigned long long* __restrict__ block_off,
                                               int64_t n_lines_batch, const unsigned short* __restrict__ info,
                                               const unsigned long long* __restrict__ deferred_off, unsigned char* __restrict__ fields,
                                               int64_t n_slots) {
    __shared__ unsigned short lstart[LSTART_ENTRIES];
    const BlockLines B = block_lines(text, T, block_off, lstart);
    int64_t slot0 = (int64_t)deferred_off[blockIdx.x];
    for (int base = 0; base < B.n_lines; base += WG) {
        const Round q = round_of(base, B.n_lines, B.row0, n_lines_batch);
        const bool mine = q.valid && (info[q.r] & DEFERRED);
        unsigned int total;
        const int64_t slot = slot0 + fhxscan::block_exclusive_scan(mine ? 1u : 0u, &total);
        if (mine && slot < n_slots) {
            const int64_t start = B.b0 + lstart[q.e];
            Line L;
            walk(text, T, start, 0, L);
            defer_field(fields, slot, text + start + L.fb, L.fn);
        }
        slot0 += total;
    }
}

// ---- the final length of every track line --------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void ut_measure(const unsigned char* __restrict__ text, int64_t T, const unsigned long long* __restrict__ block_off,
                                                 int64_t n_lines_batch, unsigned short* __restrict__ info,
                                                 const unsigned long long* __restrict__ kept_off, const unsigned long long* __restrict__ deferred_off,
                                                 int64_t kept_base, const unsigned char* __restrict__ scores, int64_t n_slots,
                                                 unsigned int* __restrict__ block_bytes) {
    __shared__ unsigned short lstart[LSTART_ENTRIES];
    const BlockLines B = block_lines(text, T, block_off, lstart);
    int64_t nr0 = kept_base + (int64_t)kept_off[blockIdx.x] + 1, slot0 = (int64_t)deferred_off[blockIdx.x];
    unsigned int my_bytes = 0;
    for (int base = 0; base < B.n_lines; base += WG) {
        const Round q = round_of(base, B.n_lines, B.row0, n_lines_batch);
        const unsigned int word = q.valid ? (unsigned int)info[q.r] : 0u;
        const bool kept = word != 0, deferred = (word & DEFERRED) != 0;
        unsigned int total;                                                   // kept lines in the low half, deferred ones in the high half
        const unsigned int rank = fhxscan::block_exclusive_scan((kept ? 1u : 0u) | (deferred ? 0x10000u : 0u), &total);
        if (kept) {
            const unsigned int done = final_word(word, nr0 + (rank & 0xFFFFu), scores, slot0 + (rank >> 16), n_slots);
            const unsigned int len = done & ~DEFERRED;
            info[q.r] = (unsigned short)done;
            my_bytes += len;
        }
        nr0 += total & 0xFFFFu;
        slot0 += total >> 16;
    }
    unsigned int total_bytes;
    fhxscan::block_exclusive_scan(my_bytes, &total_bytes);
    if (threadIdx.x == 0) block_bytes[blockIdx.x] = total_bytes;
}

// ---- the track lines, dense and in file order ----------------------------------------------------------------------------------
// what a lane writes of its line: the bytes that fall into the window [w0, w0 + WINDOW) of the round
struct WindowSink {
    unsigned char* lds;
    unsigned int pos, w0;
    __device__ void put(int c) {
        const unsigned int at = pos++ - w0;                                   // wraps to a huge value below the window
        if (at < (unsigned int)WINDOW) lds[at] = (unsigned char)c;
    }
};

__global__ __launch_bounds__(WG) void ut_format(const unsigned char* __restrict__ text, int64_t T, const unsigned long long* __restrict__ block_off,
                                                int64_t n_lines_batch, int64_t line_base, const unsigned short* __restrict__ info,
                                                const unsigned long long* __restrict__ kept_off, const unsigned long long* __restrict__ deferred_off,
                                                int64_t kept_base, const unsigned char* __restrict__ scores, int64_t n_slots,
                                                const unsigned long long* __restrict__ out_off, unsigned char* __restrict__ out, int64_t out_capacity,
                                                TrackWords* __restrict__ words) {
    __shared__ unsigned short lstart[LSTART_ENTRIES];
    __shared__ unsigned char window[WINDOW];
    const BlockLines B = block_lines(text, T, block_off, lstart);
    int64_t nr0 = kept_base + (int64_t)kept_off[blockIdx.x] + 1, slot0 = (int64_t)deferred_off[blockIdx.x];
    int64_t at = (int64_t)out_off[blockIdx.x];
    for (int base = 0; base < B.n_lines; base += WG) {      // n_lines is the same for every lane
        const Round q = round_of(base, B.n_lines, B.row0, n_lines_batch);
        const unsigned int word = q.valid ? (unsigned int)info[q.r] : 0u;
        const unsigned int len = word & ~DEFERRED;
        const bool kept = len != 0, deferred = (word & DEFERRED) != 0;
        unsigned int counts, total;
        const unsigned int rank = fhxscan::block_exclusive_scan((kept ? 1u : 0u) | (deferred ? 0x10000u : 0u), &counts);
        const unsigned int pre = fhxscan::block_exclusive_scan(len, &total);
        // the line's pieces, once for all its windows
        const unsigned char* line = text + B.b0 + (kept ? (int64_t)lstart[q.e] : 0);
        Line L;
        char score[fhx::score::MAX_TEXT];
        int score_len = 0, v2 = 0, v4 = 0;
        if (kept) {
            walk(text, T, B.b0 + lstart[q.e], 0, L);
            v2 = midpoint(line, L.b2, L.n2);
            v4 = midpoint(line, L.b4, L.n4);
            unsigned long long key = 0;
            const int cls = classify(line, L.fb, L.fn, &key);
            score_len = deferred ? host_score(scores, slot0 + (rank >> 16), n_slots, score) : score_text(cls, key, score);
        }
        for (unsigned int w0 = 0; w0 < total; w0 += WINDOW) {
            if (kept && pre < w0 + WINDOW && pre + len > w0) {
                WindowSink s{window, pre, w0};
                write_line(s, line + L.b1, L.n1, v2, line + L.b3, L.n3, v4, nr0 + (rank & 0xFFFFu), score, score_len);
                // what was written is what ut_measure counted, or nothing of this call is kept
                if (s.pos - pre != len) atomicMin(&words->first_error, error_word(line_base + q.r + 1, FHX_MS_INTERNAL));
            }
            __syncthreads();
            const unsigned int n = min(total - w0, (unsigned int)WINDOW);
            for (unsigned int j = threadIdx.x; j < n; j += WG)
                if (at + w0 + j < out_capacity) out[at + w0 + j] = window[j];
            __syncthreads();                                // the window is written again
        }
        at += total;
        nr0 += counts & 0xFFFFu;
        slot0 += counts >> 16;
    }
}

}  // namespace utd

// ===================================================================================================================
namespace {

void drop_track(fhx_ms* ms) {
    std::vector<char>().swap(ms->track);
    ms->t_lines = ms->t_kept = ms->t_deferred = 0;
}

// fhx_ms_track_file behind its argument check; whatever it returns but FHX_OK, the caller drops the track
int track_file(fhx_ms* ms, const char* path, const char* fdr_text, int32_t fdr_len, uint64_t key_bound, int32_t zero_kept, int64_t* n_bytes,
               int32_t* why, int64_t* bad_line) {
    using namespace utd;
    TH_HIP(ms, hipSetDevice(ms->device));
    TH_HIP(ms, hipStreamSynchronize(ms->stream));
    drop_track(ms);
    for (double& s : ms->t_seconds) s = 0;
    Fdr fdr;
    if (const int rc = make_fdr(ms, fdr_text, fdr_len, "the threshold", &fdr, why)) return rc;
    fhx::StageClock clock{ms->t_seconds};
    fhx::DeviceScratch tmp;
    fhx::TextBatches in;
    if (const int rc = in.open(ms, &tmp, &clock, path, "significances", "FHX_MS_BATCH_BYTES", (int64_t)1 << 31)) return rc;
    unsigned char *d_out = nullptr, *d_fields = nullptr, *d_scores = nullptr;
    unsigned int *d_block_kept = nullptr, *d_block_deferred = nullptr, *d_block_bytes = nullptr;
    unsigned long long *d_kept_off = nullptr, *d_deferred_off = nullptr, *d_out_off = nullptr;
    unsigned short* d_info = nullptr;
    int64_t info_capacity = 0, out_capacity = 0, fields_capacity = 0, scores_capacity = 0;
    TrackWords* d_words = nullptr;
    TH_HIP(ms, tmp.get_n(&d_block_kept, (size_t)in.max_blocks));
    TH_HIP(ms, tmp.get_n(&d_block_deferred, (size_t)in.max_blocks));
    TH_HIP(ms, tmp.get_n(&d_block_bytes, (size_t)in.max_blocks));
    TH_HIP(ms, tmp.get_n(&d_kept_off, (size_t)in.max_blocks));
    TH_HIP(ms, tmp.get_n(&d_deferred_off, (size_t)in.max_blocks));
    TH_HIP(ms, tmp.get_n(&d_out_off, (size_t)in.max_blocks));
    TH_HIP(ms, tmp.get_n(&d_words, 1));
    TrackWords words;
    std::vector<unsigned char> fields, scores;
    const fhx::Refusal refuse{ms, why, bad_line};
    ms->track.assign(HEAD, HEAD + sizeof(HEAD) - 1);
    int64_t kept = 0, deferred_lines = 0;
    for (; in.more(); in.advance()) {
        std::memset(&words, 0, sizeof(words));
        words.first_error = NO_ERROR;
        TH_HIP(ms, hipMemcpyAsync(d_words, &words, sizeof(words), hipMemcpyHostToDevice, ms->stream));
        if (const int rc = in.next<GrammarBytes>()) return rc;
        const unsigned char* d_text = in.d_text;
        const unsigned long long* d_block_off = in.d_block_off;
        const int64_t len = in.len, n_blocks = in.n_blocks, n = in.lines;
        TH_HIP(ms, tmp.grow(&d_info, &info_capacity, n));
        hipLaunchKernelGGL(ut_select, dim3((unsigned)n_blocks), dim3(WG), 0, ms->stream, d_text, len, d_block_off, n, in.line_base, fdr,
                           (unsigned long long)key_bound, (int)zero_kept, (int)in.refused_bytes, d_info, d_block_kept, d_block_deferred, d_words);
        hipLaunchKernelGGL(fhxscan::scan_tiles, dim3(1), dim3(fhxscan::THREADS), 0, ms->stream, (const unsigned int*)d_block_kept, n_blocks, d_kept_off,
                           &d_words->kept_lines);
        hipLaunchKernelGGL(fhxscan::scan_tiles, dim3(1), dim3(fhxscan::THREADS), 0, ms->stream, (const unsigned int*)d_block_deferred, n_blocks,
                           d_deferred_off, &d_words->deferred);
        TH_HIP(ms, hipGetLastError());
        TH_HIP(ms, hipMemcpyAsync(&words, d_words, sizeof(words), hipMemcpyDeviceToHost, ms->stream));
        TH_HIP(ms, hipStreamSynchronize(ms->stream));
        clock.mark(2);
        if (words.first_error != NO_ERROR) return refuse.word(words.first_error, FHX_MS_INTERNAL);      // earlier batches hold the smaller line numbers
        const int64_t batch_kept = (int64_t)words.kept_lines, n_slots = (int64_t)words.deferred;
        if (batch_kept > n || n_slots > batch_kept) return refuse(FHX_ERR_INTERNAL, FHX_MS_INTERNAL, 0, "more kept lines than lines");
        if (kept + batch_kept > (int64_t)INT32_MAX)
            return refuse(FHX_ERR_UNSUPPORTED, FHX_MS_KEPT, 0, "more than 2^31 - 1 lines pass: awk prints NR as an integer only below 2^31");
        if (n_slots > 0) {                                                    // the deferred round trip
            TH_HIP(ms, tmp.grow(&d_fields, &fields_capacity, n_slots * DEFER_IN));
            TH_HIP(ms, tmp.grow(&d_scores, &scores_capacity, n_slots * DEFER_OUT));
            hipLaunchKernelGGL(ut_defer, dim3((unsigned)n_blocks), dim3(WG), 0, ms->stream, d_text, len, d_block_off, n, (const unsigned short*)d_info,
                               (const unsigned long long*)d_deferred_off, d_fields, n_slots);
            TH_HIP(ms, hipGetLastError());
            fields.resize((size_t)(n_slots * DEFER_IN));
            TH_HIP(ms, hipMemcpyAsync(fields.data(), d_fields, fields.size(), hipMemcpyDeviceToHost, ms->stream));
            TH_HIP(ms, hipStreamSynchronize(ms->stream));
            if (!answer_deferred(fields.data(), n_slots, &scores)) return refuse(FHX_ERR_INTERNAL, FHX_MS_INTERNAL, 0, "a deferred score has no text");
            TH_HIP(ms, hipMemcpyAsync(d_scores, scores.data(), scores.size(), hipMemcpyHostToDevice, ms->stream));
            TH_HIP(ms, hipStreamSynchronize(ms->stream));
        }
        clock.mark(3);
        int64_t bytes = 0;
        if (batch_kept > 0) {
            hipLaunchKernelGGL(ut_measure, dim3((unsigned)n_blocks), dim3(WG), 0, ms->stream, d_text, len, d_block_off, n, d_info,
                               (const unsigned long long*)d_kept_off, (const unsigned long long*)d_deferred_off, kept, (const unsigned char*)d_scores,
                               n_slots, d_block_bytes);
            hipLaunchKernelGGL(fhxscan::scan_tiles, dim3(1), dim3(fhxscan::THREADS), 0, ms->stream, (const unsigned int*)d_block_bytes, n_blocks, d_out_off,
                               &d_words->out_bytes);
            TH_HIP(ms, hipGetLastError());
            TH_HIP(ms, hipMemcpyAsync(&words, d_words, sizeof(words), hipMemcpyDeviceToHost, ms->stream));
            TH_HIP(ms, hipStreamSynchronize(ms->stream));
            bytes = (int64_t)words.out_bytes;
            TH_HIP(ms, tmp.grow(&d_out, &out_capacity, bytes));
            hipLaunchKernelGGL(ut_format, dim3((unsigned)n_blocks), dim3(WG), 0, ms->stream, d_text, len, d_block_off, n, in.line_base,
                               (const unsigned short*)d_info, (const unsigned long long*)d_kept_off, (const unsigned long long*)d_deferred_off, kept,
                               (const unsigned char*)d_scores, n_slots, (const unsigned long long*)d_out_off, d_out, out_capacity, d_words);
            TH_HIP(ms, hipGetLastError());
            TH_HIP(ms, hipMemcpyAsync(&words, d_words, sizeof(words), hipMemcpyDeviceToHost, ms->stream));
            TH_HIP(ms, hipStreamSynchronize(ms->stream));
            if (words.first_error != NO_ERROR) return refuse.word(words.first_error, FHX_MS_INTERNAL);
        }
        clock.mark(4);
        if (bytes > 0) {
            const size_t had = ms->track.size();
            ms->track.resize(had + (size_t)bytes);
            TH_HIP(ms, hipMemcpyAsync(ms->track.data() + had, d_out, (size_t)bytes, hipMemcpyDeviceToHost, ms->stream));
            TH_HIP(ms, hipStreamSynchronize(ms->stream));
        }
        clock.mark(5);
        kept += batch_kept;
        deferred_lines += n_slots;
    }
    ms->t_lines = in.line_base;
    ms->t_kept = kept;
    ms->t_deferred = deferred_lines;
    *n_bytes = (int64_t)ms->track.size();
    if (std::getenv("FHX_TIMING"))
        std::fprintf(stderr, "interact track on the device (%s): %lld lines, %lld kept, %lld deferred (%lld bytes): read + upload %.6f s; scan %.6f s; "
                     "select %.6f s; deferred round trip %.6f s; format %.6f s; copy out %.6f s\n", path, (long long)in.line_base, (long long)kept,
                     (long long)deferred_lines, (long long)ms->track.size(), ms->t_seconds[0], ms->t_seconds[1], ms->t_seconds[2], ms->t_seconds[3],
                     ms->t_seconds[4], ms->t_seconds[5]);
    return FHX_OK;
}

}  // namespace

extern "C" {

int fhx_ms_score_text(const char* field, int32_t len, int32_t certify, char* out, int32_t capacity) {
    if (!field || !out || len < 1 || len > 15 || capacity < fhx::score::MAX_TEXT) return FHX_ERR_ARG;
    if (!certify) return fhx::score::host_fields(field, len, out);
    // the kernel's route with the host's log10: the same cells, the same digits
    int e = 0;
    unsigned long long m = 0;
    if ((len != 12 && len != 13) || field[1] != '.' || field[8] != 'e' || (field[9] != '+' && field[9] != '-')) return FHX_ERR_ARG;
    for (int k = 0; k < 8; ++k)
        if (k != 1) {
            if (field[k] < '0' || field[k] > '9') return FHX_ERR_ARG;
            m = m * 10 + (unsigned long long)(field[k] - '0');
        }
    for (int k = 10; k < len; ++k) {
        if (field[k] < '0' || field[k] > '9') return FHX_ERR_ARG;
        e = e * 10 + (field[k] - '0');
    }
    if (m < 1000000ull || e > 308) return FHX_ERR_ARG;
    return fhx::score::certified(out, fhx::score::approximate(m, field[9] == '-' ? -e : e));
}

int fhx_ms_track_file(fhx_ms* ms, const char* path, const char* fdr_text, int32_t fdr_len, uint64_t key_bound, int32_t zero_kept, int64_t* n_bytes,
                      int32_t* why, int64_t* bad_line) {
    if (!ms || !path || !fdr_text || !n_bytes || !why || !bad_line) return FHX_ERR_ARG;
    *n_bytes = 0;
    *why = FHX_MS_OK;
    *bad_line = 0;
    const int rc = track_file(ms, path, fdr_text, fdr_len, key_bound, zero_kept, n_bytes, why, bad_line);
    if (rc != FHX_OK) drop_track(ms);                                         // the one exit of a failed call, whatever failed
    return rc;
}

int fhx_ms_track_counts(const fhx_ms* ms, int64_t* n_lines, int64_t* n_kept, int64_t* n_deferred, int64_t* n_bytes) {
    if (!ms) return FHX_ERR_ARG;
    if (n_lines) *n_lines = ms->t_lines;
    if (n_kept) *n_kept = ms->t_kept;
    if (n_deferred) *n_deferred = ms->t_deferred;
    if (n_bytes) *n_bytes = (int64_t)ms->track.size();
    return FHX_OK;
}

int fhx_ms_track_stage_seconds(const fhx_ms* ms, double* seconds) {
    if (!ms || !seconds) return FHX_ERR_ARG;
    for (int k = 0; k < FHX_MS_TRACK_STAGES; ++k) seconds[k] = ms->t_seconds[k];
    return FHX_OK;
}

int fhx_ms_copy_track(const fhx_ms* ms, void* dst, int64_t capacity) {
    if (!ms || capacity < (int64_t)ms->track.size() || (!dst && !ms->track.empty())) return FHX_ERR_ARG;
    if (!ms->track.empty()) std::memcpy(dst, ms->track.data(), ms->track.size());
    return FHX_OK;
}

}  // extern "C"
