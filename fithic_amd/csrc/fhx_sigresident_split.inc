// fhx_sigresident_split.inc - the per-chromosome FDR subsets of a pass taken from its RESIDENT columns (included at the end of
// fhx_sigresident.hip, at file scope): what fhx_ms_split_file gives for the file fhx_write_significances_device writes, without
// the file.
//
// The list is field 1 of every line of that file: the literal `chr1` of fithic's header, and the first chromosome of every EMITTED
// row (a trans row of an -x All run lists its first chromosome and goes to no subset).  A row is kept for name c when it is
// emitted, both its chromosomes are c and `$7 <= fdr` holds: sr_decide<SPLIT> (fhx_sigresident.hip) makes that decision, looks
// the name rules up per chromosome id (fhx_namerule.hpp, applied by the host: the names are known before any kernel runs) and
// marks the listed ids.  Behind it, the two rank scans and sr_rows:
//
//   srs_keys       one kept row per lane: (rank of its chromosome's name in bytewise order) << 40 | kept rank
//   fhx_sort_u64   the stable radix sort, on a sort context of this context's own (K3's sort state of the pass is not touched).
//                  The sort was built and not a counting partition: the keys carry the kept rank, so the order inside a run is
//                  file order whatever the sort does with equal keys, nothing is counted per (workgroup, name), and the cost
//                  does not depend on how many of the 4096 possible names there are.
//   srs_permute    the kept rows' columns in sorted order
//   kept_extras, format_kept   fhx_significant_select's own, over the permuted rows: ONE output buffer
//   srs_bounds     behind format_kept's byte scan: the row that begins a name's run notes the run's first row and first byte
//
// so a name's subset is one stretch of the output, in file order.  The host ranks the names (at most FHX_MS_SPLIT_NAMES) and cuts
// the stretches; a listed name without a run has an empty subset.
namespace fhx::sigres {

constexpr int RANK_SHIFT = 40;                 // 12 bits of name rank above 40 bits of kept rank
constexpr unsigned long long RANK_MASK = (1ull << RANK_SHIFT) - 1;
constexpr unsigned long long NO_RUN = ~0ull;

__global__ __launch_bounds__(WG) void srs_keys(const int32_t* __restrict__ k_loc1, const int16_t* __restrict__ slot_chr,
                                               const unsigned short* __restrict__ id_rank, int32_t n_names, int64_t n_kept,
                                               unsigned long long* __restrict__ keys, Words* __restrict__ words) {
    const int64_t k = (int64_t)blockIdx.x * WG + threadIdx.x;
    if (k >= n_kept) return;
    const int c = slot_chr[k_loc1[k]];                                        // a kept row is cis: its second chromosome is the same
    unsigned long long rank = 0;
    if (c >= 0 && c < n_names) rank = id_rank[c];
    else atomicOr(&words->internal, 1u);
    keys[k] = (rank << RANK_SHIFT) | (unsigned long long)k;
}

__global__ __launch_bounds__(WG) void srs_permute(const unsigned long long* __restrict__ sorted, int64_t n_kept, const int32_t* __restrict__ loc1,
                                                  const int32_t* __restrict__ loc2, const int32_t* __restrict__ count,
                                                  const double* __restrict__ p, const double* __restrict__ q, int32_t* __restrict__ s_loc1,
                                                  int32_t* __restrict__ s_loc2, int32_t* __restrict__ s_count, double* __restrict__ s_p,
                                                  double* __restrict__ s_q, Words* __restrict__ words) {
    const int64_t j = (int64_t)blockIdx.x * WG + threadIdx.x;
    if (j >= n_kept) return;
    int64_t k = (int64_t)(sorted[j] & RANK_MASK);
    if (k >= n_kept) {                                                        // not a key srs_keys wrote
        atomicOr(&words->internal, 1u);
        k = 0;
    }
    s_loc1[j] = loc1[k];
    s_loc2[j] = loc2[k];
    s_count[j] = count[k];
    s_p[j] = p[k];
    s_q[j] = q[k];
}

// rowlen and wg_off are sr_measure's and its scan's, over the permuted rows
__global__ __launch_bounds__(WG) void srs_bounds(const unsigned long long* __restrict__ sorted, int64_t n_kept, const unsigned char* __restrict__ rowlen,
                                                 const unsigned long long* __restrict__ wg_off, int32_t n_listed,
                                                 unsigned long long* __restrict__ run_row, unsigned long long* __restrict__ run_byte) {
    const int64_t j = (int64_t)blockIdx.x * WG + threadIdx.x;
    const unsigned int len = j < n_kept ? (unsigned int)rowlen[j] : 0u;
    unsigned int total;
    const unsigned int pre = fhxscan::block_exclusive_scan(len, &total);
    if (j >= n_kept) return;
    const unsigned long long rank = sorted[j] >> RANK_SHIFT;
    const bool head = j == 0 || (sorted[j - 1] >> RANK_SHIFT) != rank;
    if (head && rank < (unsigned long long)n_listed) {
        run_row[rank] = (unsigned long long)j;
        run_byte[rank] = wg_off[blockIdx.x] + pre;
    }
}

}  // namespace fhx::sigres

extern "C" {

int fhx_significant_split(fhx_ctx* ctx, const char* const* chr_names, int32_t n_names, const char* fdr_text, int32_t fdr_len, uint64_t key_bound,
                          int32_t zero_kept, int64_t* n_emitted, int32_t* n_listed, int32_t* why, int64_t* bad_line) {
    using namespace fhx::sigres;
    if (!ctx || !chr_names || n_names <= 0 || !fdr_text || !n_emitted || !n_listed || !why || !bad_line) return FHX_ERR_ARG;
    *n_emitted = 0;
    *n_listed = 0;
    *why = FHX_MS_OK;
    *bad_line = 0;
    std::vector<char>().swap(ctx->sig_split_text);
    std::vector<fhx_ctx::SigRun>().swap(ctx->sig_split);
    if (const int rc = require_names(ctx, chr_names, n_names)) return rc;      // here for name_grammar; decide_rows asks again for its own walk
    std::vector<unsigned char> name_why((size_t)n_names, 0);                  // the name rules, once per chromosome id
    for (int i = 0; i < n_names; ++i)
        name_why[(size_t)i] = (unsigned char)fhx::namerule::name_grammar((const unsigned char*)chr_names[i], (int)std::min<size_t>(
                                                                             std::strlen(chr_names[i]), (size_t)INT32_MAX));
    Decided F;                                 // stages: decide, rank scans, rows + keys + sort, ExpCC/bias + measure + format, copy out
    if (const int rc = decide_rows<SPLIT>(ctx, chr_names, n_names, fdr_text, fdr_len, key_bound, zero_kept, /*strict=*/0, why, bad_line, F, &name_why))
        return rc;
    // the list: `chr1` of the header, and the first chromosome of every emitted row; equal names are one entry
    std::vector<unsigned char> listed((size_t)n_names, 0);
    if (F.n > 0) {
        FHX_HIP(hipMemcpyAsync(listed.data(), F.d_listed, (size_t)n_names, hipMemcpyDeviceToHost, ctx->stream));
        FHX_HIP(hipStreamSynchronize(ctx->stream));
    }
    std::vector<std::string> names{"chr1"};
    for (int i = 0; i < n_names; ++i)
        if (listed[(size_t)i]) names.emplace_back(chr_names[i]);
    auto bytewise = [](const std::string& a, const std::string& b) {          // `sort` under LC_ALL=C
        const int c = std::memcmp(a.data(), b.data(), std::min(a.size(), b.size()));
        return c != 0 ? c < 0 : a.size() < b.size();
    };
    std::sort(names.begin(), names.end(), bytewise);
    names.erase(std::unique(names.begin(), names.end()), names.end());
    if (names.size() > (size_t)FHX_MS_SPLIT_NAMES) {
        *why = FHX_MS_NAMES;
        return fail(ctx, FHX_ERR_UNSUPPORTED, "more than " + std::to_string(FHX_MS_SPLIT_NAMES) + " distinct names in field 1");
    }
    const int32_t listed_n = (int32_t)names.size();
    std::vector<fhx_ctx::SigRun> runs((size_t)listed_n);
    for (int32_t k = 0; k < listed_n; ++k) runs[(size_t)k].name = names[(size_t)k];
    std::vector<char> text;
    const int64_t kept = F.kept;
    if (kept > 0) {
        DeviceScratch& G = F.G;
        Words* d_words = F.d_words;
        const int64_t k_wg = (kept + WG - 1) / WG;
        std::vector<unsigned short> id_rank((size_t)n_names, 0);
        for (int i = 0; i < n_names; ++i)
            if (listed[(size_t)i])
                id_rank[(size_t)i] = (unsigned short)(std::lower_bound(names.begin(), names.end(), std::string(chr_names[i]), bytewise) - names.begin());
        KeptRows R, P;
        unsigned short* d_id_rank = nullptr;
        unsigned long long *d_keys = nullptr, *d_sorted = nullptr, *d_run_row = nullptr, *d_run_byte = nullptr;
        unsigned int* d_perm = nullptr;
        FHX_HIP(G.get(&d_id_rank, (size_t)n_names * 2));
        FHX_HIP(G.get(&d_keys, (size_t)kept * 8));
        FHX_HIP(G.get(&d_sorted, (size_t)kept * 8));
        FHX_HIP(G.get(&d_perm, (size_t)kept * 4));
        FHX_HIP(G.get(&d_run_row, (size_t)listed_n * 8));
        FHX_HIP(G.get(&d_run_byte, (size_t)listed_n * 8));
        FHX_HIP(G.get(&P.d_loc1, (size_t)kept * 4));
        FHX_HIP(G.get(&P.d_loc2, (size_t)kept * 4));
        FHX_HIP(G.get(&P.d_count, (size_t)kept * 4));
        FHX_HIP(G.get(&P.d_p, (size_t)kept * 8));
        FHX_HIP(G.get(&P.d_q, (size_t)kept * 8));
        if (!ctx->sig_sorter && fhx_create(ctx->device, &ctx->sig_sorter) != FHX_OK) {      // only a split pays for it
            ctx->sig_sorter = nullptr;
            return fail(ctx, FHX_ERR_HIP, "the sort context could not be made");
        }
        if (const int rc = gather_kept(ctx, F, R)) return rc;
        FHX_HIP(hipMemcpyAsync(d_id_rank, id_rank.data(), (size_t)n_names * 2, hipMemcpyHostToDevice, ctx->stream));
        FHX_HIP(hipMemsetAsync(d_run_row, 0xFF, (size_t)listed_n * 8, ctx->stream));
        FHX_HIP(hipMemsetAsync(d_run_byte, 0xFF, (size_t)listed_n * 8, ctx->stream));
        hipLaunchKernelGGL(srs_keys, dim3((unsigned)k_wg), dim3(WG), 0, ctx->stream, (const int32_t*)R.d_loc1, (const int16_t*)ctx->d_slot_chr,
                           (const unsigned short*)d_id_rank, n_names, kept, d_keys, d_words);
        FHX_HIP(hipGetLastError());
        FHX_HIP(hipStreamSynchronize(ctx->stream));                           // the sorter has a stream of its own, and `id_rank` leaves scope
        if (const int rc = fhx_sort_u64(ctx->sig_sorter, d_keys, kept, d_sorted, d_perm))  // synchronises its stream
            return fail(ctx, rc, std::string("sort: ") + fhx_last_error(ctx->sig_sorter));
        FHX_HIP(hipSetDevice(ctx->device));
        hipLaunchKernelGGL(srs_permute, dim3((unsigned)k_wg), dim3(WG), 0, ctx->stream, (const unsigned long long*)d_sorted, kept,
                           (const int32_t*)R.d_loc1, (const int32_t*)R.d_loc2, (const int32_t*)R.d_count, (const double*)R.d_p, (const double*)R.d_q,
                           P.d_loc1, P.d_loc2, P.d_count, P.d_p, P.d_q, d_words);
        FHX_HIP(hipGetLastError());
        if (const int rc = timed_mark(ctx, F, 2)) return rc;
        if (const int rc = kept_extras(ctx, F, P)) return rc;
        const auto bounds = [&] {
            hipLaunchKernelGGL(srs_bounds, dim3((unsigned)k_wg), dim3(WG), 0, ctx->stream, (const unsigned long long*)d_sorted, kept,
                               (const unsigned char*)F.d_len, (const unsigned long long*)F.d_wg_off, listed_n, d_run_row, d_run_byte);
        };
        if (const int rc = format_kept(ctx, F, kept_cols(ctx, F, P), bounds, "the sorted keys are not the kept rows")) return rc;
        F.T.mark(3);                                                          // the copies of the runs' bounds count as copy out, with the text
        std::vector<unsigned long long> run_row((size_t)listed_n), run_byte((size_t)listed_n);
        text.resize((size_t)F.bytes);
        FHX_HIP(hipMemcpyAsync(run_row.data(), d_run_row, (size_t)listed_n * 8, hipMemcpyDeviceToHost, ctx->stream));
        FHX_HIP(hipMemcpyAsync(run_byte.data(), d_run_byte, (size_t)listed_n * 8, hipMemcpyDeviceToHost, ctx->stream));
        FHX_HIP(hipMemcpyAsync(text.data(), F.d_out, (size_t)F.bytes, hipMemcpyDeviceToHost, ctx->stream));
        FHX_HIP(hipStreamSynchronize(ctx->stream));
        // ascending ranks are ascending runs: each ends where the next one begins, the last one with the text
        int64_t row_end = kept, byte_end = F.bytes;
        for (int32_t k = listed_n - 1; k >= 0; --k) {
            fhx_ctx::SigRun& run = runs[(size_t)k];
            if (run_row[(size_t)k] == NO_RUN) {
                run.offset = byte_end;
                continue;
            }
            const int64_t r_at = (int64_t)run_row[(size_t)k], b_at = (int64_t)run_byte[(size_t)k];
            if (r_at < 0 || r_at >= row_end || b_at < 0 || b_at >= byte_end)
                return fail(ctx, FHX_ERR_INTERNAL, "the runs of the sorted rows do not tile the subsets");
            run.offset = b_at;
            run.bytes = byte_end - b_at;
            run.rows = row_end - r_at;
            row_end = r_at;
            byte_end = b_at;
        }
        if (row_end != 0 || byte_end != 0) return fail(ctx, FHX_ERR_INTERNAL, "the runs of the sorted rows do not tile the subsets");
        F.T.mark(4);
    }
    ctx->sig_split_text.swap(text);
    ctx->sig_split.swap(runs);
    *n_emitted = F.emitted;
    *n_listed = listed_n;
    if (F.timing)
        std::fprintf(stderr, "fhx_significant_split: %lld rows, %lld emitted, %lld kept (%lld bytes) for %d names: decide %.6f s; rank scans "
                     "%.6f s; rows + keys + sort %.6f s; ExpCC/bias + measure + format %.6f s; copy out %.6f s\n", (long long)F.n, (long long)F.emitted,
                     (long long)kept, (long long)ctx->sig_split_text.size(), (int)listed_n, F.s[0], F.s[1], F.s[2], F.s[3], F.s[4]);
    return FHX_OK;
}

int fhx_significant_split_counts(fhx_ctx* ctx, int64_t* kept_rows, int64_t* kept_bytes, int32_t capacity) {
    if (!ctx || capacity < (int32_t)ctx->sig_split.size()) return FHX_ERR_ARG;
    for (size_t k = 0; k < ctx->sig_split.size(); ++k) {
        if (kept_rows) kept_rows[k] = ctx->sig_split[k].rows;
        if (kept_bytes) kept_bytes[k] = ctx->sig_split[k].bytes;
    }
    return FHX_OK;
}

int fhx_significant_split_names(fhx_ctx* ctx, char* dst, int32_t capacity) {
    if (!ctx || capacity < (int32_t)ctx->sig_split.size() || (!dst && !ctx->sig_split.empty())) return FHX_ERR_ARG;
    for (size_t k = 0; k < ctx->sig_split.size(); ++k) {
        const std::string& name = ctx->sig_split[k].name;                     // an accepted name has at most 63 bytes
        std::memset(dst + k * FHX_MS_SPLIT_NAME_BYTES, 0, FHX_MS_SPLIT_NAME_BYTES);
        std::memcpy(dst + k * FHX_MS_SPLIT_NAME_BYTES, name.data(), std::min<size_t>(name.size(), FHX_MS_SPLIT_NAME_BYTES - 1));
    }
    return FHX_OK;
}

int fhx_significant_copy_split(fhx_ctx* ctx, int32_t index, void* dst, int64_t capacity) {
    if (!ctx || index < 0 || index >= (int32_t)ctx->sig_split.size()) return FHX_ERR_ARG;
    const fhx_ctx::SigRun& run = ctx->sig_split[(size_t)index];
    if (capacity < run.bytes || (!dst && run.bytes > 0)) return FHX_ERR_ARG;
    if (run.offset < 0 || run.offset + run.bytes > (int64_t)ctx->sig_split_text.size()) return FHX_ERR_INTERNAL;
    if (run.bytes > 0) std::memcpy(dst, ctx->sig_split_text.data() + run.offset, (size_t)run.bytes);
    return FHX_OK;
}

}  // extern "C"
