// fhx_kr_resident.inc - the Knight-Ruiz matrix assembled from the rows an engine context already holds in HBM (included at
// the end of fhx_kr.hip, outside extern "C").
//
// The protocol runs HiCKRy.py on the contact counts and then fithic.py with its bias file; a `fithic --kr` run has the counts
// resident as d_loc1 / d_loc2 / d_count (locus slots and int32 counts) from its own ingest.  fhx_kr_load_pairs_resident builds
// HiCKRy's rawMatrix (HiCKRy.py:18-54) from them, so that the contacts file is neither inflated and parsed a second time on the
// host nor uploaded as five columns:
//
//   line_of_slot   host, n entries: the engine names a locus by its slot (fixed size: grid[chr].base + mid / res on the
//                  chromosome's offset; -r 0 and off-grid loci: the rank in h_slot_keys); the matrix names it by its fragment
//                  line.  One int32 per slot, -1 = no fragment line; the last line of a repeated locus wins as in
//                  fhx_kr_load_loci, a fragment line no slot covers stays an empty matrix row
//   krr_keys       per row two table lookups instead of kr_lookup's two binary searches: keys[i] = x*n + y, keys[m+i] = y*n + x
//   assemble_cells (fhx_kr.hip) the same sort, run heads and row pointers as the file route; kr_emit_cells<int32_t> reads the
//                  resident counts through the permutation and widens them - no double column of values exists
//
// ALL rows count: HiCKRy sees the whole file, so rows the skip mask hides from later passes, inter-chromosomal rows under
// -x intraOnly and rows with count 0 (stored zeros) enter the matrix as they do on the file route.

namespace krd {

constexpr int KRR_ROWS = 8;                          // rows per thread
constexpr int KRR_CHUNK = THREADS * KRR_ROWS;        // rows per workgroup: one workgroup per chunk, no resident grid loop

// One workgroup per chunk of KRR_CHUNK rows; thread t takes rows t, t + 256, ... of the chunk, so that every load and store of a
// wave covers consecutive addresses.  Reads 8 B per row here (loc1, loc2; the count is read by kr_emit_cells) and two entries of
// line_of_slot, which has one int32 per locus (a few MB at most: L2 resident); writes 16 B per row.
//
// The CSR that follows is bit-identical to the file route's WHATEVER order the resident rows are in: counts are integers and
// there are fewer than 2^32 of them, so every partial sum of a cell is an integer below 2^53 and exact in any order.  That is
// what lets the tests compare this route with fhx_kr_load_pairs bit for bit.
//
// A row with a locus that has no fragment line is the error path only: the smallest FILE position of such a row (grow[i] where
// the context carries file positions, else i) is what the caller's KeyError names, the row the file route names.
__global__ __launch_bounds__(THREADS) void krr_keys(int64_t m, const int32_t* __restrict__ loc1, const int32_t* __restrict__ loc2,
                                                    const long long* __restrict__ grow, const int32_t* __restrict__ line_of_slot,
                                                    int64_t n_slots, int64_t n, unsigned long long* __restrict__ keys,
                                                    unsigned long long* __restrict__ first_missing) {
    const int64_t base = (int64_t)blockIdx.x * KRR_CHUNK + threadIdx.x;
    int s1[KRR_ROWS], s2[KRR_ROWS];
#pragma unroll
    for (int k = 0; k < KRR_ROWS; ++k) {             // all loads of the thread's rows go out first
        const int64_t i = base + (int64_t)k * THREADS;
        s1[k] = i < m ? loc1[i] : 0;
        const int l2 = i < m ? loc2[i] : 0;
        s2[k] = l2 < 0 ? ~l2 : l2;                   // the sign bit carries "inter-chromosomal" (k0_slots)
    }
    int x[KRR_ROWS], y[KRR_ROWS];
#pragma unroll
    for (int k = 0; k < KRR_ROWS; ++k) {
        x[k] = (int64_t)(unsigned int)s1[k] < n_slots ? line_of_slot[s1[k]] : -1;      // (a slot outside the table: no line)
        y[k] = (int64_t)(unsigned int)s2[k] < n_slots ? line_of_slot[s2[k]] : -1;
    }
#pragma unroll
    for (int k = 0; k < KRR_ROWS; ++k) {
        const int64_t i = base + (int64_t)k * THREADS;
        if (i >= m) continue;
        if (x[k] < 0 || y[k] < 0) {
            atomicMin(first_missing, (unsigned long long)(grow ? grow[i] : (long long)i));
            keys[i] = keys[m + i] = 0;
            continue;
        }
        keys[i] = (unsigned long long)((int64_t)x[k] * n + y[k]);
        keys[m + i] = (unsigned long long)((int64_t)y[k] * n + x[k]);
    }
}

}  // namespace krd

namespace {

// slot -> fragment line for the context's locus grid, from the distinct loci fhx_kr_load_loci kept (their last lines)
std::vector<int32_t> line_of_slot_table(const fhx_kr* kr, const fhx_ctx* ctx) {
    std::vector<int32_t> line((size_t)std::max<int64_t>(ctx->n_slots, 1), -1);
    const int64_t res = ctx->prm.resolution;
    for (size_t k = 0; k < kr->locus_keys.size(); ++k) {
        const unsigned long long key = kr->locus_keys[k];
        const int32_t c = (int32_t)(key >> 32), mid = (int32_t)(key & 0xFFFFFFFFull);
        if (c < 0 || mid < 0) continue;                                   // no contact row can name it (the loaders refuse such rows)
        if (ctx->nonfixed) {                                              // -r 0 / off-grid loci: exact match, as build_slot_tables_nonfixed
            const auto it = std::lower_bound(ctx->h_slot_keys.begin(), ctx->h_slot_keys.end(), key);
            if (it != ctx->h_slot_keys.end() && *it == key) line[(size_t)(it - ctx->h_slot_keys.begin())] = kr->locus_index[k];
            continue;
        }
        if (c >= (int32_t)ctx->grid.size()) continue;                     // as build_slot_tables
        const ChrGrid& g = ctx->grid[(size_t)c];
        if (g.off < 0) continue;                                          // the chromosome has no contact rows
        const int64_t idx = mid / res;
        if (mid - idx * res != g.off || idx >= g.nslots) continue;        // no row can match this exact midpoint
        line[(size_t)g.base + (size_t)idx] = kr->locus_index[k];
    }
    return line;
}

}  // namespace

extern "C" int fhx_kr_load_pairs_resident(fhx_kr* kr, fhx_ctx* ctx, int64_t* first_unknown_row) {
    if (!kr || !ctx) return FHX_ERR_ARG;
    if (first_unknown_row) *first_unknown_row = -1;
    if (ctx->device < 0 || ctx->device != kr->device) return fail(kr, FHX_ERR_ARG, "the engine context is not on this context's device");
    if (!ctx->d_loc1 || !ctx->d_loc2 || !ctx->d_count || !ctx->have_params) return fail(kr, FHX_ERR_ARG, "the engine context holds no contact rows");
    const int64_t n = kr->n_full, m = ctx->n_rows;
    if (n <= 0) return fail(kr, FHX_ERR_ARG, "fhx_kr_load_loci must be called first");
    if (!ctx->counts_integral)
        return fail(kr, FHX_ERR_UNSUPPORTED, "a contact count of the resident rows was not an integer as written: HiCKRy balances float(count), "
                                              "the rows hold int(float(count)) - assemble from the file (fhx_kr_load_pairs)");
    if (2 * m >= (1ll << 32)) return fail(kr, FHX_ERR_UNSUPPORTED, "more than 2^31 rows");
    if (ctx->nonfixed && (int64_t)ctx->h_slot_keys.size() != ctx->n_slots) return fail(kr, FHX_ERR_INTERNAL, "the engine's locus list does not match its slots");
    KR_HIP(hipSetDevice(kr->device));
    KR_HIP(hipStreamSynchronize(ctx->stream));        // whatever the engine has in flight; its rows are only read here
    free_matrix(kr);
    KR_HIP(dev_malloc(&kr->d_indptr, (size_t)(n + 1) * sizeof(int64_t)));
    if (m == 0) {
        KR_HIP(hipMemsetAsync(kr->d_indptr, 0, (size_t)(n + 1) * sizeof(int64_t), kr->stream));
        KR_HIP(dev_malloc(&kr->d_col, (size_t)(1 + krd::KR_PAD) * sizeof(int32_t)));
        KR_HIP(dev_malloc(&kr->d_val, (size_t)(1 + krd::KR_PAD) * sizeof(double)));
        KR_HIP(hipStreamSynchronize(kr->stream));
        kr->n = n;
        return FHX_OK;
    }
    // FHX_TIMING=1: where the call's time goes (each mark behind a stream wait the call makes anyway)
    const bool timing = std::getenv("FHX_TIMING") != nullptr;
    auto t_last = std::chrono::steady_clock::now();
    double t_stage[3] = {0, 0, 0};
    auto mark = [&](int k) {
        const auto t = std::chrono::steady_clock::now();
        t_stage[k] = std::chrono::duration<double>(t - t_last).count();
        t_last = t;
    };
    const std::vector<int32_t> line = line_of_slot_table(kr, ctx);
    mark(0);
    int32_t* d_line = nullptr;
    unsigned long long* keys = nullptr;
    DeviceScratch tmp;
    KR_HIP(tmp.get(&d_line, line.size() * sizeof(int32_t)));
    KR_HIP(tmp.get(&keys, (size_t)(2 * m) * 8));
    KR_HIP(hipMemcpyAsync(d_line, line.data(), line.size() * sizeof(int32_t), hipMemcpyHostToDevice, kr->stream));
    if (!kr->d_counter) KR_HIP(dev_malloc(&kr->d_counter, 4 * sizeof(unsigned long long)));
    const unsigned long long none = ~0ull;
    KR_HIP(hipMemcpyAsync(kr->d_counter, &none, 8, hipMemcpyHostToDevice, kr->stream));
    const int64_t chunks = (m + krd::KRR_CHUNK - 1) / krd::KRR_CHUNK;
    if (timing) KR_HIP(hipEventRecord(kr->ev0, kr->stream));
    hipLaunchKernelGGL(krd::krr_keys, dim3((unsigned)chunks), dim3(krd::THREADS), 0, kr->stream, m, (const int32_t*)ctx->d_loc1,
                       (const int32_t*)ctx->d_loc2, (const long long*)ctx->d_grow, (const int32_t*)d_line, ctx->n_slots, n, keys, kr->d_counter);
    KR_HIP(hipGetLastError());
    if (timing) KR_HIP(hipEventRecord(kr->ev1, kr->stream));
    unsigned long long missing = none;
    KR_HIP(hipMemcpyAsync(&missing, kr->d_counter, 8, hipMemcpyDeviceToHost, kr->stream));
    KR_HIP(hipStreamSynchronize(kr->stream));
    mark(1);
    float keys_ms = 0;
    if (timing) (void)hipEventElapsedTime(&keys_ms, kr->ev0, kr->ev1);
    tmp.drop(d_line);
    if (missing != none) {
        if (first_unknown_row) *first_unknown_row = (int64_t)missing;
        return fail(kr, FHX_ERR_REFERENCE_EXIT, "row " + std::to_string(missing) +
                    " names a locus that is not in the fragments file (the reference raises KeyError, HiCKRy.py:44-45)");
    }
    const int rc = assemble_cells(kr, tmp, keys, (const int32_t*)ctx->d_count, m);     // the counts stay where the engine keeps them
    mark(2);
    if (timing && rc == FHX_OK)
        std::fprintf(stderr, "fhx_kr_load_pairs_resident: %lld rows, %lld loci, %lld cells: slot table (host) %.6f s; allocations + table upload + "
                             "krr_keys %.6f s (the kernel alone %.6f s = %.0f GB/s of its 24 B per row); sort + cells + row pointers %.6f s\n",
                     (long long)m, (long long)n, (long long)kr->nnz_full, t_stage[0], t_stage[1], 1e-3 * keys_ms,
                     keys_ms > 0 ? 24.0 * (double)m / (1e-3 * keys_ms) / 1e9 : 0.0, t_stage[2]);
    return rc;
}
