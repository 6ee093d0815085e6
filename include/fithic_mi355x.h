/*
 * fithic_mi355x.h - C ABI of libfithic_mi355x.so, the MI355X-native Fit-Hi-C significance engine.
 *
 * The reference (ay-lab/fithic 2.0.7) is pure Python and has no FFI / plugin interface
 * (SURVEY.md section 8b); the boundary this library honours is the set of Python call signatures on its
 * hot path.  Each entry point below names the reference lines it replaces:
 *
 *   fhx_load_pairs / fhx_load_fragments / fhx_load_bias
 *        the three tables the reference re-reads from gzip text in every stage
 *        (fithic/fithic.py:406-417, :581-590, :805-832), handed over once as host SoA arrays
 *   fhx_pass_stats      fithic.read_Interactions                      (fithic/fithic.py:389-454)      kernel K1
 *   fhx_fit             fithic.makeBinsFromInteractions               (fithic/fithic.py:463-553)
 *                       fithic.generate_FragPairs (fixed-size branch) (fithic/fithic.py:561-689)
 *                       fithic.calculateProbabilities                 (fithic/fithic.py:843-918)
 *                       fithic.fit_Spline, fit + table part           (fithic/fithic.py:936-968)      host C++
 *   fhx_pvalues         fithic.fit_Spline, per-pair loop              (fithic/fithic.py:1017-1124)    kernel K2
 *                       incl. scipy.special.bdtrc                     (call sites :1070, :1101)
 *   fhx_bh              myStats.benjamini_hochberg_correction         (fithic/myStats.py:24-48)       kernels K3
 *                       and its dispatch                              (fithic/fithic.py:1126-1164)
 *   fhx_fetch           the value lists fit_Spline hands to its writer (fithic/fithic.py:1188-1194)
 *   fhx_next_pass       outlier collection for pass >= 2              (fithic/fithic.py:1215-1217, :408-412, :528-548)
 *
 * Conventions: plain C, no exceptions cross the boundary; every function returns 0 (FHX_OK) or a negative
 * error code; fhx_last_error(ctx) returns a message owned by the context.  One context per GPU (or per
 * host thread for device = -1, host-only: everything except the kernels works).  A context is not
 * thread-safe; different contexts are independent.  Host pointers passed in are copied before return.
 */
#ifndef FITHIC_MI355X_H
#define FITHIC_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FHX_OK 0
#define FHX_ERR_ARG (-1)           /* bad argument / call order */
#define FHX_ERR_NO_DEVICE (-2)     /* kernel entry point called on a host-only context, or no GPU */
#define FHX_ERR_HIP (-3)           /* a HIP runtime call failed */
#define FHX_ERR_UNSUPPORTED (-4)   /* input outside the accelerated path (e.g. loci off the fixed-size grid) */
#define FHX_ERR_REFERENCE_EXIT (-5)/* the reference would sys.exit(2) / raise here (message says where) */
#define FHX_ERR_NOMEM (-6)
#define FHX_ERR_INTERNAL (-7)      /* a device-side consistency check failed (results would be wrong): message says which */

#define FHX_MODE_INTRA_ONLY 0      /* -x intraOnly (default) */
#define FHX_MODE_INTER_ONLY 1      /* -x interOnly */
#define FHX_MODE_ALL 2             /* -x All */

/* How the binomial of fithic/fithic.py:1070,1101 sees a total (observedIntraInRangeSum / observedInterAllSum) that does not fit
 * a C int.  The reference hands Python ints to scipy.special.bdtrc, whose Cephes core takes `int n`: the total is narrowed to
 * 32 bits (2^31 arrives as -2^31 and every such p-value is NaN; 2^32 + 10^6 arrives as 10^6).
 *   FHX_TOTALS_REFERENCE (default)  the same narrowing: the output equals fithic.py's bit for bit, NaNs included
 *   FHX_TOTALS_WIDE                 bdtrc's arithmetic on the true total (no reference computes this; identical below 2^31)
 * Everything else (expCC, the bin probabilities, BH) uses the true totals in both modes, as the reference does. */
#define FHX_TOTALS_REFERENCE 0
#define FHX_TOTALS_WIDE 1

typedef struct fhx_ctx fhx_ctx;

/* The reference's module globals (fithic/fithic.py:203-260) after its "zero means unset" rule. */
typedef struct fhx_params {
    int64_t resolution;            /* -r; 0 = non-fixed-size data (arbitrary midpoints, fithic/fithic.py:691-778) */
    int64_t dist_low;              /* -L, default 0 */
    int64_t dist_up;               /* -U, INT64_MAX for +inf */
    int32_t n_bins;                /* -b, default 100 */
    int32_t mapp_thres;            /* -m, default 1 */
    int32_t mode;                  /* FHX_MODE_* */
    int32_t totals;                /* FHX_TOTALS_* (this field was `reserved`, always 0 = FHX_TOTALS_REFERENCE) */
    double bias_low;               /* -tL, default 0.5 */
    double bias_up;                /* -tU, default 2 */
} fhx_params;

/* What read_Interactions returns (fithic/fithic.py:454) plus the counters it logs (:447-449). */
typedef struct fhx_stats {
    int64_t n_rows;                /* rows on this context (shard) */
    int64_t inter_count;           /* observedInterAllCount */
    int64_t inter_sum;             /* observedInterAllSum */
    int64_t intra_all_count;       /* observedIntraAllCount */
    int64_t intra_all_sum;         /* observedIntraAllSum */
    int64_t in_range_count;        /* observedIntraInRangeCount */
    int64_t in_range_sum;          /* observedIntraInRangeSum */
    int64_t max_count;             /* largest contact count seen (sizes the lbeta tables) */
    int64_t n_dist;                /* length of the distance histogram: index i <-> distance i*resolution */
    int64_t n_skipped;             /* rows skipped as outliers of earlier passes */
} fhx_stats;

/* Scalars of one fitted pass (generate_FragPairs' return tuple, fit_Spline's spline diagnostics). */
typedef struct fhx_fit_info {
    int32_t n_bins_made;           /* len(binStats) */
    int32_t n_knots;               /* FITPACK n */
    int32_t spline_ier;            /* FITPACK ier */
    int32_t spline_restarted;      /* 1 if the nest-too-small continuation call ran */
    int64_t n_table;               /* len(splineX) */
    int64_t n_frags;               /* noOfFrags */
    int64_t possible_intra_in_range; /* possibleIntraInRangeCount (double-counted as the reference does) */
    double possible_inter_all;     /* possibleInterAllCount (float after /= 2) */
    double possible_intra_all;     /* possibleIntraAllCount */
    double max_possible_dist;      /* maxPossibleGenomicDist */
    double inter_chr_prob;         /* interChrProb */
    double baseline_intra_prob;    /* baselineIntraChrProb */
    double spline_s;               /* min(y)^2 */
    double spline_fp;              /* FITPACK fp */
    double residual;               /* sum((y - ius(x))^2), numpy pairwise order */
    double bh_total_tests;         /* N handed to benjamini_hochberg_correction for this mode */
    double outlier_thres;          /* 1/N */
    int32_t totals;                /* FHX_TOTALS_* this pass ran with */
    int32_t totals_narrowed;       /* bit 0: observedIntraInRangeSum >= 2^31, bit 1: observedInterAllSum >= 2^31 - the two modes differ */
    int64_t bdtrc_n_intra;         /* the n bdtrc was given for in-range cis rows (the narrowed value in reference mode) */
    int64_t bdtrc_n_inter;         /* ... and for inter-chromosomal rows */
} fhx_fit_info;

/* Arrays a caller can copy out with fhx_get_array (all caller-allocated). */
enum fhx_array {
    FHX_A_HIST_SUMCC = 0,          /* int64[n_dist]   sum of counts per distance index (mainDic[d][1]) */
    FHX_A_HIST_NPAIRS = 1,         /* int64[n_dist]   rows per distance index (key present iff > 0) */
    FHX_A_BIN_LB = 2,              /* int64[n_bins_made] */
    FHX_A_BIN_UB = 3,              /* int64[n_bins_made] */
    FHX_A_BIN_POSS = 4,            /* int64   binStats[b][1] */
    FHX_A_BIN_SUMCC = 5,           /* int64   binStats[b][2] */
    FHX_A_BIN_SUMDIST = 6,         /* double  binStats[b][3] */
    FHX_A_BIN_POSS7 = 7,           /* int64   binStats[b][7] */
    FHX_A_X = 8,                   /* double[n_bins_made]  calculateProbabilities x (unsorted) */
    FHX_A_Y = 9,                   /* double[n_bins_made] */
    FHX_A_KNOTS = 10,              /* double[n_knots] */
    FHX_A_COEFFS = 11,             /* double[n_knots-4] */
    FHX_A_TABLE_X = 12,            /* int64[n_table]  splineX */
    FHX_A_TABLE_Y0 = 13,           /* double[n_table] splineY (before isotonic regression) */
    FHX_A_TABLE_Y = 14,            /* double[n_table] newSplineY */
    FHX_A_OUTLIER_DIST_HIST = 15,  /* int64[n_dist]   multiset of outlier distances accumulated so far */
    FHX_A_FDR_COUNTS = 16,         /* int64[51]       plot_qvalues' shifted cumulative counts */
    FHX_A_BIN_POSS0 = 17,          /* int64   binStats[b][1] right after makeBinsFromInteractions */
    FHX_A_DIST_KEYS = 18,          /* int64[n_dist]   -r 0 only: the distinct in-range distances the histogram arrays belong to */
    FHX_A_OUTLIER_DISTS = 19       /* int64[...]      -r 0 only: ascending multiset of outlier distances accumulated so far */
};

/* ---- life cycle --------------------------------------------------------------------------------- */
int fhx_create(int device, fhx_ctx** out);      /* device >= 0: HIP device ordinal; -1: host-only */
void fhx_destroy(fhx_ctx* ctx);
const char* fhx_last_error(fhx_ctx* ctx);
const char* fhx_version(void);
/* The HIP runtime and the device's primary context brought up ahead of fhx_create (0.15-0.25 s the first time in a process);
 * a launcher calls it on a thread while it does other start-up work.  Optional: fhx_create does the same when needed. */
int fhx_warmup(int device);
int fhx_set_params(fhx_ctx* ctx, const fhx_params* p);

/* ---- tables (host SoA in, copied) --------------------------------------------------------------- */
/* Chromosome ids are small non-negative ints chosen by the caller, shared by all three tables.
 * chr_sort_rank[id] = position of that chromosome NAME in Python's sorted() order: the reference walks
 * chromosomes in that order (fithic.py:606) and its double accumulators depend on it. */
int fhx_load_fragments(fhx_ctx* ctx, const int32_t* chr, const int32_t* mid, const int32_t* hits, int64_t n,
                       const int32_t* chr_sort_rank, int32_t n_chr);
int fhx_load_bias(fhx_ctx* ctx, const int32_t* chr, const int32_t* mid, const double* bias, int64_t n);
int fhx_load_pairs(fhx_ctx* ctx, const int32_t* chr1, const int32_t* mid1, const int32_t* chr2,
                   const int32_t* mid2, const int32_t* count, int64_t n);
/* Same, but the five arrays already live in this GPU's memory (e.g. written by a generator kernel or
 * received over xGMI).  `stream` = the hipStream_t the arrays were produced on, NULL = the legacy default stream
 * (PyTorch's, unless the caller chose another): the call waits for it before reading the arrays. */
int fhx_load_pairs_device(fhx_ctx* ctx, const void* d_chr1, const void* d_mid1, const void* d_chr2,
                          const void* d_mid2, const void* d_count, int64_t n, void* stream);

/* The contacts file parsed BY THE GPU (csrc/fhx_ingest.inc): the inflated text (fhx_host_inflate) goes to HBM as it is and
 * kernels find the lines, read the five fields (fithic/fithic.py:404-417: ch1, int(mid1), ch2, int(mid2),
 * int(float(contactCount))) and collect the chromosome names in the reference's order of first appearance.  Two calls, because
 * the caller owns the id space the names map into (it is shared with the fragments and bias files):
 *   fhx_ingest_contacts_text    parse; n_rows, n_names out, fhx_ingest_contacts_name(ctx, i) = name i (valid until the commit)
 *   fhx_ingest_contacts_commit  ids[i] = the caller's id of name i; the rows enter the context as fhx_load_pairs would have
 *                               loaded them (fhx_set_params must have been called, as for fhx_load_pairs)
 * Only the regular file is taken - ASCII, five tokens per line, names of at most 63 bytes, [+-]digits midpoints and a
 * digits[.digits] count (15 digits at most) within int32.  For every other file (an exponent, an underscore in a number, a malformed line whose
 * error message must name it, ...) fhx_ingest_contacts_text returns FHX_ERR_UNSUPPORTED with nothing loaded, and the caller
 * gives the same fhx_text to fhx_host_parse_text, whose grammar is Python's.  fhx_ingest_contacts_discard drops a parsed text
 * that will not be committed. */
struct fhx_text;
int fhx_ingest_contacts_text(fhx_ctx* ctx, const struct fhx_text* text, int32_t n_threads, int64_t* n_rows, int32_t* n_names);
const char* fhx_ingest_contacts_name(const fhx_ctx* ctx, int32_t i);
/* The same straight from the FILE, for a file of size-tagged gzip members ("FH" of this library's writers, "BC" of bgzip):
 * the compressed bytes are uploaded and every member is inflated by the GPU (csrc/fhx_inflate.inc: one wave per member, CRC-32
 * and ISIZE checked), so the text exists in HBM only.  FHX_ERR_UNSUPPORTED with *refused = 1: not such a container, or a
 * stream the device decoder does not accept - fhx_host_inflate (zlib; it reports what the reference's gzip module would) and
 * fhx_ingest_contacts_text may still take it; *refused = 2: the text is outside the device parser's grammar -
 * fhx_host_read_table is the path. */
int fhx_ingest_contacts_file(fhx_ctx* ctx, const char* path, int32_t n_threads, int64_t* n_rows, int32_t* n_names, int32_t* refused);
/* test hook: the text of such a file as the device decoder produces it (n_out = its size; cap = room in out) */
int fhx_debug_inflate_file(fhx_ctx* ctx, const char* path, void* out, int64_t cap, int64_t* n_out);
int fhx_ingest_contacts_commit(fhx_ctx* ctx, const int32_t* ids, int32_t n_ids);
/* `fithic --gpus N` without a funnel (every rank parses the file on its own GPU, fithic/fithic.py:404-417 once per rank):
 *   fhx_ingest_contacts_chr_counts    rows of the parsed text per name, counted by the FIRST locus's chromosome (what decides which
 *                                     rank a row belongs to: the ranks agree on the owners because they count the same file)
 *   fhx_ingest_contacts_commit_shard  as fhx_ingest_contacts_commit, but only the rows whose first chromosome has mine[i] != 0
 *                                     enter the context, in file order, with their file positions (fhx_set_global_rows)
 *   fhx_shard_segments                the maximal stretches of consecutive file positions among the loaded rows: local_start,
 *                                     file_start, length of each, ordered; *n_out > cap: too many (nothing filled in)          */
/* The cheaper split (round 5, last step): the ranks cut the FILE, not the genome.  fhx_ingest_contacts_file_slice inflates and
 * parses part `part` of `n_parts` (whole gzip members, cut where the compressed bytes divide evenly; the members must carry their
 * sizes, else *refused = 1; *ends_with_newline: the part's text ends a row - required of every part but the last);
 * fhx_ingest_contacts_commit takes its rows; fhx_set_global_rows_range(first) numbers them first, first + 1, ... (first = the rows of
 * the parts before it).  Nothing in the engine needs a chromosome's rows on one rank. */
int fhx_ingest_contacts_file_slice(fhx_ctx* ctx, const char* path, int32_t n_threads, int32_t part, int32_t n_parts, int64_t* n_rows,
                                   int32_t* n_names, int32_t* refused, int32_t* ends_with_newline);
int fhx_set_global_rows_range(fhx_ctx* ctx, int64_t first);
/* The same for a file the device does not inflate (plain gzip): every rank inflates it (fhx_host_inflate), then uploads and parses
 * only the rows that start in its N-th of the text's bytes - every row in exactly one part. */
int fhx_ingest_contacts_text_slice(fhx_ctx* ctx, const struct fhx_text* text, int32_t n_threads, int32_t part, int32_t n_parts, int64_t* n_rows,
                                   int32_t* n_names);
/* bytes [*lo, *hi) of the text that part takes (host only; parts can be empty) */
int fhx_text_part_bounds(const struct fhx_text* text, int32_t part, int32_t n_parts, int64_t* lo, int64_t* hi);
/* Round 6: the ranks of a sharded run inflate ONE plain gzip stream together - rank r its N-th of the COMPRESSED bytes (1/N of the
 * inflate work and of the text in host memory per rank; with fhx_host_inflate every rank did all of it).  Replaces the one
 * gzip.open of fithic/fithic.py:404 for `fithic --gpus N`.  Protocol (fithic_amd/sharded.py: _ingest_stream_parts):
 *   fhx_host_inflate_part      this rank's chunks decoded without the 32 KB before them (csrc/fhx_gunzip.cpp); FHX_ERR_UNSUPPORTED:
 *                              not one plain stream / too small / a stream the decoder refuses - the caller takes the old route
 *   fhx_text_part_tail         the part's last 32768 symbols in terms of the window before the part (< 256: a byte, 256 + j: byte j
 *                              of that window): the caller chains them rank after rank into every part's window
 *   fhx_text_part_resolve      window -> the part's text as a new fhx_text object - the part object is left empty - and its CRC-32; the caller
 *                              checks fhx_crc32_combine of all parts and the summed lengths against the file's trailer
 *   fhx_text_first_row_end     length of the text's first (partial) row, newline included; -1: no newline in the text
 *   fhx_ingest_contacts_text_own   the text from byte `skip` on + `extra` (the rest of its last row: the head of the next rank's text)
 *                              uploaded and parsed: a row belongs to the rank whose text holds its first byte */
typedef struct fhx_text_part fhx_text_part;
int fhx_host_inflate_part(const char* path, int32_t n_threads, int32_t part, int32_t n_parts, fhx_text_part** out);
int64_t fhx_text_part_bytes(const fhx_text_part* p);
int32_t fhx_text_part_is_last(const fhx_text_part* p);
int fhx_text_part_tail(const fhx_text_part* p, uint16_t* tail, int64_t cap);                   /* cap >= 32768 */
int fhx_text_part_resolve(fhx_text_part* p, const uint8_t* window, int64_t window_bytes, struct fhx_text** text_out, uint32_t* crc32_out);
const char* fhx_text_part_error(const fhx_text_part* p);
void fhx_text_part_free(fhx_text_part* p);
uint32_t fhx_crc32_combine(uint32_t crc_a, uint32_t crc_b, int64_t len_b);
int64_t fhx_text_first_row_end(const struct fhx_text* text, char* row, int64_t cap);            /* row may be NULL */
int32_t fhx_text_ends_with_newline(const struct fhx_text* text);
int fhx_ingest_contacts_text_own(fhx_ctx* ctx, const struct fhx_text* text, int32_t n_threads, int64_t skip, const char* extra,
                                 int64_t extra_bytes, int64_t* n_rows, int32_t* n_names);
int fhx_ingest_contacts_chr_counts(fhx_ctx* ctx, int64_t* counts, int32_t n_names);
int fhx_ingest_contacts_commit_shard(fhx_ctx* ctx, const int32_t* ids, const uint8_t* mine, int32_t n_ids, int64_t* n_kept);
int fhx_shard_segments(fhx_ctx* ctx, int64_t* local_start, int64_t* file_start, int64_t* length, int64_t cap, int64_t* n_out);
void fhx_ingest_contacts_discard(fhx_ctx* ctx);
/* The identity columns of loaded rows, rebuilt from the resident rows (slot -> chromosome id, midpoint): rows = n row
 * numbers, or NULL for all rows in order (n must then be the loaded row count).  What a caller that ingested on the device
 * uses to look at a few rows (the outlier lines) without ever holding the columns on the host. */
int fhx_fetch_pairs(fhx_ctx* ctx, const int64_t* rows, int64_t n, int32_t* chr1, int32_t* mid1, int32_t* chr2, int32_t* mid2,
                    int32_t* count);

/* ---- one spline pass ---------------------------------------------------------------------------- */
int fhx_pass_stats(fhx_ctx* ctx, fhx_stats* out);                       /* K1, then waits for the sums */
int fhx_get_stats(fhx_ctx* ctx, fhx_stats* out);                        /* the statistics the current fit was made from */
/* Distributed runs: replace the local histogram / sums by the all-reduced ones before fhx_fit. */
int fhx_set_global_stats(fhx_ctx* ctx, const fhx_stats* global_stats, const int64_t* hist_sumcc,
                         const int64_t* hist_npairs, int64_t n_dist);
/* -r 0 only (host-side testing / callers that bring their own histogram): the distinct distances of the histogram arrays
 * handed to fhx_set_global_stats, and the ascending multiset of outlier distances of earlier passes. */
int fhx_set_dist_keys(fhx_ctx* ctx, const int64_t* keys, int64_t n);
int fhx_set_outlier_dists(fhx_ctx* ctx, const int64_t* dists, int64_t n);
/* Distributed runs, pass >= 2: replace the local multiset of outlier distances (count per distance index,
 * accumulated over all earlier passes) by the all-reduced one. */
int fhx_set_outlier_dist_hist(fhx_ctx* ctx, const int64_t* hist, int64_t n_dist);
/* makeBinsFromInteractions alone (host): bins are readable through fhx_get_array(FHX_A_BIN_LB/UB/SUMCC/POSS0). */
int fhx_make_bins(fhx_ctx* ctx, int32_t* n_bins_made);
int fhx_fit(fhx_ctx* ctx, fhx_fit_info* out);                           /* host; uploads the tables */
int fhx_pvalues(fhx_ctx* ctx);                                          /* K2 (asynchronous) */
int fhx_bh(fhx_ctx* ctx, double n_total_tests);                         /* K3 (asynchronous); any finite N: N <= 0 gives
                                                                          * q = 0 like the reference's loop (running max from 0) */
/* The four calls above as one: K1 -> host fit -> K2 -> K3 of the current pass (asynchronous like fhx_bh; stats and info may be
 * NULL).  What a driver's loop over passes calls: main() of fithic/fithic.py:317-370 between read_Interactions and the writer. */
int fhx_run_pass(fhx_ctx* ctx, fhx_stats* stats, fhx_fit_info* info);
int fhx_sync(fhx_ctx* ctx);
/* Sharded runs with -p >= 3 only.  The reference stops skipping outlier lines after the first line number that
 * is an outlier in two passes (fithic/fithic.py:408-412 on a SortedList with duplicates); that is a
 * statement about positions in the ONE input file, so a shard must know its rows' file positions
 * (fhx_set_global_rows, ascending not required) and the ranks must agree on the limit (min over ranks of
 * fhx_get_skip_limit, handed back with fhx_set_skip_limit; INT64_MAX = no duplicate yet). */
int fhx_set_global_rows(fhx_ctx* ctx, const int64_t* file_row_of_local_row, int64_t n);
int64_t fhx_get_skip_limit(fhx_ctx* ctx);
int fhx_set_skip_limit(fhx_ctx* ctx, int64_t limit);
int fhx_next_pass(fhx_ctx* ctx, int64_t* n_outliers_total);             /* fold this pass's outliers in */
/* Forget every pass: the outlier line set and distance multiset are emptied, the next fhx_pass_stats is pass 1 again.
 * The reference equivalent is starting main() over on the same input (fithic/fithic.py:317-331 builds fresh
 * SortedLists); the loaded tables stay on the device. */
int fhx_reset_passes(fhx_ctx* ctx);

/* ---- results ------------------------------------------------------------------------------------ */
/* Any pointer may be NULL.  Arrays have n_rows entries in input row order. */
int fhx_fetch(fhx_ctx* ctx, double* p, double* q, double* expcc, double* bias1, double* bias2);
/* Per-row byte flags: outlier[i] = (p_i < 1/N) of the last fhx_pvalues; skip[i] = row is skipped by fhx_pass_stats
 * (outlier of an earlier pass, fithic/fithic.py:408-412).  Either pointer may be NULL. */
int fhx_fetch_flags(fhx_ctx* ctx, uint8_t* outlier, uint8_t* skip);
/* The row numbers (file order, ascending) of the rows fhx_fetch_flags would flag as outliers, compacted on the device.
 * rows == NULL or cap < *n_out: only the count is returned. */
int fhx_fetch_outlier_rows(fhx_ctx* ctx, int64_t* rows, int64_t cap, int64_t* n_out);
int fhx_get_array(fhx_ctx* ctx, int which, void* dst, int64_t capacity_elems, int64_t* n_out);
/* Raw device pointers for plumbing (torch / RCCL exchange): 0 = p, 1 = q, 2 = sorted keys, 3 = sorted idx */
void* fhx_device_ptr(fhx_ctx* ctx, int which);
int64_t fhx_n_sorted(fhx_ctx* ctx);
/* How the last Benjamini-Hochberg call sorted its surviving p-values (diagnostics, tests): out8 = radix passes of the first
 * attempt (0: the small in-LDS sort ran), lowest key bit they covered, what the repair of the lower bits could not list (0 =
 * nothing; bit 0: a run whose ends were out of reach, bit 1: a list overflowed, bit 2: forced by FHX_OS_FORCE_FALLBACK, bit 3:
 * every bit of every key was sorted after all), inversions met, runs sorted by one thread each, inversions found in runs too
 * long for that, such runs sorted as segments of their own, keys in them. */
int fhx_bh_sort_stats(fhx_ctx* ctx, int64_t* out8);
/* Which path the last fhx_bh took through K3 (diagnostics, tests).  Read when asked, never collected inside fhx_bh: the call waits
 * for the stream and copies two device words.  out8 = [0] 0: the dense-q launches (k3_compact<true>, k3_fill_q) were not enqueued,
 * 1: enqueued and the device chose the scattered variant, 2: the device chose the dense variant; [1] rows below the cutoff by the key
 * histogram; [2] the same by the compaction's device counter; [3] tiles per workgroup handed to the scattered compaction; [4] the
 * sort: 0 none (no survivor), 1 the in-LDS tile sorts, 2 the one-sweep passes, 3 the count / scan / scatter passes; [5] 1 when the
 * last pass's survivor count (under a tenth of the rows) kept the dense launches from being enqueued; [6] 1 when the compaction
 * relied on a q column filled with 1.0 behind fhx_pass_stats; [7] 0.  FHX_ERR_ARG before the first fhx_bh. */
int fhx_k3_pass_info(fhx_ctx* ctx, int64_t* out8);
/* One more slot of the same report, read the same way (the call waits for the stream): which kernel compacted the rows below the
 * cutoff in the last fhx_bh when the scattered variant did.  *out = 0: the sparse compaction (k3_compact_sparse) was not enqueued -
 * the q column was not filled with 1.0 behind fhx_pass_stats, or the pass was not the engine's own; 1: enqueued, and the device
 * chose k3_compact<false> (by the key histogram more rows lie below the cutoff than 1024 per workgroup of the compaction); 2: the device chose the
 * sparse compaction.  FHX_ERR_ARG before the first fhx_bh. */
int fhx_k3_compact_variant(fhx_ctx* ctx, int32_t* out);
/* Test hook: per = 1..4 replaces the library's choice of tiles per workgroup in the scattered compaction of this context's later
 * fhx_bh and fhx_bh_local_sort calls (the library itself goes beyond 1 only from 6.7e7 rows on), 0 gives the choice back;
 * anything else is FHX_ERR_ARG.  Results do not depend on it.  Not for production callers. */
int fhx_debug_k3_tiles_per_group(fhx_ctx* ctx, int per);
/* Test hook: the device blocks this process holds through the library, over all handles of every kind, and their bytes as they were
 * asked for.  Either pointer may be null.  Compare two readings; other handles of the process are in the absolute values. */
int fhx_debug_device_blocks(int64_t* blocks, int64_t* bytes);
/* Test hook: on = 1 makes this context's later fhx_pass_stats calls classify the rows from their three int32 columns (12 bytes a
 * row) instead of the 32-bit key column written at load; 0 gives the key column back; anything else is FHX_ERR_ARG.  Results do
 * not depend on it.  Not for production callers. */
int fhx_debug_k1_wide(fhx_ctx* ctx, int on);
/* Seconds the kernels of the last pass took on the context's stream (HIP events): k1, k2, k3. */
int fhx_kernel_seconds(fhx_ctx* ctx, double* k1, double* k2, double* k3);
/* The same summed over the passes since the last reset, without stopping the stream after each of them: sums4 = seconds of K1, K2,
 * K3 and of the heavy K2 launch (fhx_k2_heavy_launch), counts4 = how many passes each sum holds (either may be NULL).  The library
 * reads a pass's events at the next point where it waits for the stream anyway (the statistics of the following pass), this call
 * waits for the stream and reads the rest; reset != 0 clears the sums afterwards.  A timing harness calls it once with reset
 * before and once after its timed passes. */
int fhx_kernel_seconds_total(fhx_ctx* ctx, double* sums4, int64_t* counts4, int reset);
/* Passes whose event pair was recorded again before it could be read (a kernel group run twice with no statistics call and no
 * fhx_kernel_seconds_total in between, while the stream had not yet passed the first pair): dropped4 = K1, K2, K3, heavy launch,
 * since the last reset.  Zero means the sums above cover every pass that ran. */
int fhx_kernel_events_dropped(fhx_ctx* ctx, int64_t* dropped4);
/* Duration (HIP events on the context's stream) and row count of the dominant launch of the last fhx_pvalues: the queue
 * of rows whose continued fraction runs to Cephes' 300-iteration cap (k2_queue<BC_CF_SWAPPED>). */
int fhx_k2_heavy_launch(fhx_ctx* ctx, double* seconds, int64_t* rows);
/* The shader clock (GHz) that launch ran at, sampled by one of its waves (cycle counter over the constant-rate counter): what turns
 * a count of VALU wave-instructions into the milliseconds of an issue-bound launch on THIS box (bench.py: valu_issue_floor_ms). */
int fhx_k2_heavy_clock(fhx_ctx* ctx, double* ghz);
/* Rows the last fhx_pvalues queued per branch class of incbet (the per-pair branch table of fithic/fithic.py:1057-1116 followed
 * into Cephes): out5 = power series, converging incbcf, incbd, swapped incbcf (the 300-iteration class), closed form with
 * prior >= 0.01.  Every other row was finished by the classification launch itself (constants, closed form with a small prior).
 * Measurement aid: per-kernel bytes and rows of bench.py / profiles. */
int fhx_k2_class_rows(fhx_ctx* ctx, int64_t* out5);

/* myStats.benjamini_hochberg_correction(p_values, num_total_tests) on an arbitrary host array (fithic/myStats.py:24-48):
 * copies p to the GPU, runs the K3 kernels, copies q back (input order). */
int fhx_bh_array(fhx_ctx* ctx, const double* p, int64_t n, double n_total_tests, double* q);

/* scipy.special.bdtrc(count - 1, n_total, prior) element-wise on the GPU for integer counts (the only form the
 * reference uses, fithic/fithic.py:1070,1101); host arrays in and out.  Known-answer testing of K2's arithmetic.  An integral
 * n_total is narrowed to a C int as scipy does (FHX_TOTALS_REFERENCE, also for a context without parameters) unless the
 * context's parameters say FHX_TOTALS_WIDE. */
int fhx_bdtrc_array(fhx_ctx* ctx, double n_total, const int32_t* count, const double* prior, int64_t n, double* out);

/* Test hook: the K2 launches of a pass - the classification kernel, the closed form, the class kernels, the count-sorted
 * 300-iteration class with its hand-back - on n rows the caller chose: row i has contact count count[i], prior prior[i] and uses
 * the inter-chromosomal binomial (total n_inter) where is_inter[i] != 0, else the intra one (total n_intra).  The launches are the
 * ones fhx_pvalues makes, planned by the same rules (kernels with Cephes' pow branch when a total is below 171, rows per lane of the
 * heavy kernel by row count or FHX_K2H_ROWS, FHX_K2_LEGACY), without the no-bias table path and with the fused key histogram on;
 * nonfixed = 0: the fixed-size classification kernel, 1: the -r 0 one.  Every prior reaches the kernels bit for bit (the .hip file
 * says how).  Totals are narrowed like fhx_bdtrc_array's.  p_out (n): the p-values, which must equal fhx_bdtrc_array's bit for bit;
 * class_rows5 (optional): as fhx_k2_class_rows; n_redo (optional): rows the uniform heavy kernel handed back to the per-lane loop;
 * top_hist (optional, hist_cap >= 4096 entries): the histogram of key(p) >> 50 that K2 gathered for K3 (p = 1.0 is bin 4092;
 * values the heavy kernel stored may be counted in a lower bin than their own, never a higher one).
 * FHX_ERR_ARG for n > 2^22, a count outside [0, 2^20], a negative prior (NaN is accepted), a total that is negative or not finite.
 * The call DISCARDS the contact rows of the context: afterwards every stage call refuses until rows are loaded again. */
int fhx_debug_k2_rows(fhx_ctx* ctx, double n_intra, double n_inter, const int32_t* count, const double* prior, const uint8_t* is_inter,
                      int64_t n, int32_t nonfixed, double* p_out, int64_t* class_rows5, int64_t* n_redo, int64_t* top_hist,
                      int64_t hist_cap);

/* Test hook: the raw Cephes continued fraction (kind 0 = incbcf, 1 = incbd) of K2 evaluated element-wise on the GPU,
 * either with Cephes' literal convergence test (lazy = 0) or with the division-free test K2 uses (lazy = 1); the two
 * must agree bit for bit.  Host arrays in and out. */
int fhx_debug_contfrac(fhx_ctx* ctx, int kind, int lazy, const double* a, const double* b, const double* x, int64_t n,
                       double* out);

/* Test hook: the branch class K2 assigns to (count, prior) under the binomial total n_total - by the per-count threshold table
 * the classify kernel reads (by_table) and by the predicates of Cephes' incbet evaluated directly (by_arith); the two must agree
 * for every double.  thr5 (optional, n x 5): the thresholds tA, tB, tC, tD, tE of each count. */
int fhx_debug_classify(fhx_ctx* ctx, double n_total, const int32_t* count, const double* prior, int64_t n, int32_t* by_table,
                       int32_t* by_arith, double* thr5);
/* Test hook: out[i] = K2's lean division of n[i] / d[i] (must equal IEEE n/d inside the operand window it is used in). */
int fhx_debug_lean_div(fhx_ctx* ctx, const double* n, const double* d, int64_t len, double* out);
/* Test hook: K2's division by a tabulated reciprocal, as the class kernels do it (an LDS table of refined reciprocals by integer j,
 * built per workgroup).  kind 0: the divisor is j (j + 1), the continued fractions' table; kind 1: the divisor is j, the power
 * series' table.  table_len receives the table's length J; out[(j - 1) * m + i] = num[i] / divisor(j) for 1 <= j < J, so out holds
 * (J - 1) * m doubles (call with m = 0 to learn J).  Must equal IEEE division for numerators that are 0 or in [1e-200, 1e200]. */
int fhx_debug_table_div(fhx_ctx* ctx, int kind, const double* num, int64_t m, double* out, int32_t* table_len);
/* Test hook: the device writer's number formatting on arbitrary doubles - kind 0 "%e", 1 "%f"; text32 receives 32 bytes per value
 * (zero padded), len the character count, or -1 where the device formatter hands the row to the host (|v| >= 2^64 / 2^63). */
int fhx_debug_format(fhx_ctx* ctx, const double* values, int64_t n, int32_t kind, char* text32, int32_t* len);

/* ---- distributed BH building blocks (section 8e): local sort, then rank/scan over a global segment -- */
/* Early cutoff (exact): the reference's q is a FORWARD running max of min(p*N/rank, 1), so every p at or above the first
 * key whose value*N/rank bound reaches 1 has q = 1 and need not be sorted.  fhx_bh computes that key from a coarse
 * histogram of its own p-values; sharded runs all-reduce the 8192-bin histograms (fhx_bh_top_hist) and hand the sum
 * back (fhx_bh_set_cutoff) before fhx_bh_local_sort.  Without either call every p < 1 is sorted. */
int fhx_bh_top_hist(fhx_ctx* ctx, int64_t* hist_out, int64_t capacity);
int fhx_bh_set_cutoff(fhx_ctx* ctx, const int64_t* global_hist, int64_t n_bins, double n_total_tests);
/* The same two steps with the histogram left in HBM: fhx_device_ptr(ctx, 4) is the 8192 x uint64 table; the caller
 * all-reduces it in place between the two calls (no host round trip). */
int fhx_bh_top_hist_device(fhx_ctx* ctx);
int fhx_bh_set_cutoff_device(fhx_ctx* ctx, double n_total_tests);
int fhx_bh_local_sort(fhx_ctx* ctx);                 /* compact p below the cutoff, radix sort (key, row) on this GPU */
int fhx_bh_apply_sorted(fhx_ctx* ctx, const void* d_sorted_keys, int64_t n, int64_t global_rank0,
                        double carry_in, double n_total_tests, void* d_q_sorted, double* block_max_out);
/* sort n 64-bit keys that live on this GPU (ascending, stable); d_perm_out[i] = original position of sorted element i */
int fhx_sort_u64(fhx_ctx* ctx, const void* d_keys_in, int64_t n, void* d_keys_out, void* d_perm_out);
/* q[row of local sorted element i] = d_q_sorted_local[i] for the fhx_n_sorted() elements of fhx_bh_local_sort */
int fhx_bh_scatter(fhx_ctx* ctx, const void* d_q_sorted_local);
/* device-to-device copy on the context's stream, then wait (plumbing between the library's buffers and torch's) */
int fhx_memcpy_d2d(fhx_ctx* ctx, void* dst, const void* src, int64_t bytes);

/* ---- multi-GPU runs behind the boundary (SURVEY 8b last row, 8e) -----------------------------------------------------
 * One process (or thread) per GPU, one fhx_ctx each, the contact rows sharded over the contexts (by chromosome, or any
 * other split: every exchange below is row-order free).  The reference is one process, so what must be global is what its
 * data structures make global: mainDic and the sums of read_Interactions (fithic/fithic.py:434-440) -> ONE all-reduce of
 * [sums | in-range histogram windows] in HBM; the global ascending order of benjamini_hochberg_correction
 * (fithic/myStats.py:27-46) -> sample sort: all-reduced 8192-bin key histogram (exact early cutoff), all-gather of
 * regular samples, splitters, all-to-all of the keys, local sort of the received slice, all-gather of the slice maxima
 * (carry of the running max), all-to-all of q back; the outlier multiset of pass >= 2 (fithic.py:528-548) -> all-reduce.
 * All collectives are enqueued on the context's stream between the kernels; the host waits twice per pass (for the summed
 * statistics the host fit needs, and for the send/receive counts of the key exchange).
 *
 * Transport 1 - RCCL over xGMI (production): rank 0 calls fhx_comm_unique_id, hands the bytes to the other ranks by
 * whatever means started them (environment, file, socket, MPI ...), every rank calls fhx_comm_init.  librccl is loaded at
 * run time (the copy already in the process, e.g. PyTorch's, else the system's), so single-GPU users need no RCCL.
 * Transport 2 - caller-provided collectives on device pointers (tests on a one-GPU box, other fabrics): fhx_comm_init_custom.
 * The library synchronises its stream before each callback; a callback returns when its result is in place. */
#define FHX_UNIQUE_ID_BYTES 128
int fhx_comm_unique_id(void* id_out, int64_t capacity);                 /* ncclGetUniqueId */
int fhx_comm_init(fhx_ctx* ctx, const void* rccl_unique_id, int rank, int nranks);   /* ncclCommInitRank on ctx's device */
typedef struct fhx_transport {
    void* user;
    /* in-place reduction of n int64 values at device address d_buf; op 0 = sum, 1 = max, 2 = min */
    int (*all_reduce_i64)(void* user, void* d_buf, int64_t n, int op);
    /* d_recv[r * bytes .. (r + 1) * bytes) = rank r's d_send[0 .. bytes) */
    int (*all_gather)(void* user, const void* d_send, void* d_recv, int64_t bytes);
    /* counts and offsets in elements of elem_bytes, one entry per rank */
    int (*all_to_all_v)(void* user, const void* d_send, const int64_t* send_counts, const int64_t* send_offsets, void* d_recv,
                        const int64_t* recv_counts, const int64_t* recv_offsets, int elem_bytes);
} fhx_transport;
int fhx_comm_init_custom(fhx_ctx* ctx, const fhx_transport* t, int rank, int nranks);
int fhx_comm_destroy(fhx_ctx* ctx);
/* rank, world size and the RCCL version code (0 for a custom transport) of an initialised communicator */
int fhx_comm_info(fhx_ctx* ctx, int* rank, int* nranks, int* rccl_version);
/* One spline pass over all ranks' rows: K1 -> all-reduce -> host fit (identical on every rank) -> K2 -> global BH; leaves
 * p and q of the LOCAL rows in row order, as fhx_pass_stats + fhx_fit + fhx_pvalues + fhx_bh do on one GPU.
 * Fixed-size loci only (-r 0 runs go through the building blocks above). */
int fhx_run_pass_distributed(fhx_ctx* ctx, fhx_fit_info* out);
/* The same pass stage by stage, for callers that keep the reference's stage order (read_Interactions ... fit_Spline):
 * fhx_pass_stats_distributed (K1 + the one all-reduce; afterwards stats and histograms are the genome-wide ones on every rank)
 * -> fhx_make_bins / fhx_fit / fhx_pvalues on every rank as on one GPU -> fhx_bh_distributed (global ranking). */
int fhx_pass_stats_distributed(fhx_ctx* ctx, fhx_stats* out);
int fhx_bh_distributed(fhx_ctx* ctx, double n_total_tests);
/* fhx_next_pass on every rank + the genome-wide outlier multiset, outlier count and first duplicated line */
int fhx_next_pass_distributed(fhx_ctx* ctx, int64_t* n_outliers_total);
/* host wall seconds per stage of the last fhx_run_pass_distributed: k1 + stats exchange, host fit, K2 launch, cutoff +
 * local sort + splitters (up to the count exchange), key exchange + slice sort + scan + q return */
int fhx_dist_stage_seconds(fhx_ctx* ctx, double* out5);
/* The collectives this context issued since the communicator was made (or since the last call with clear != 0), one text line
 * each: "<step> <kind> <size>" with the step ids, kinds and size units of fithic_amd/csrc/fhx_dist_schedule.def - the one list
 * of what a sharded pass exchanges.  Recorded only when FHX_DIST_TRACE=1 was set at fhx_comm_init(_custom) time.  *n_bytes
 * receives the length of the text; nothing is copied (or cleared) when capacity is smaller. */
int fhx_dist_trace(fhx_ctx* ctx, char* buf, int64_t capacity, int64_t* n_bytes, int clear);
/* plain copies between host and this context's GPU (plumbing for custom transports): kind 0 = host to device,
 * 1 = device to host, 2 = device to device; waits for completion */
int fhx_copy(fhx_ctx* ctx, void* dst, const void* src, int64_t bytes, int kind);

/* ---- host numerics, exported for tests and for callers that only need the host side ------------------ */
int fhx_host_spline_fit(const double* x, const double* y, int32_t m, double s, double* t, double* c,
                        int32_t* n_knots, double* fp, int32_t* ier, int32_t* restarted);
int fhx_host_spline_eval(const double* t, const double* c, int32_t n_knots, const double* xs, int64_t nx, double* out);
int fhx_host_pava_decreasing(const double* y, int64_t n, double* out);
int fhx_host_lbeta_table(double n_total, int64_t max_count, double* lbeta_out, double* inv_beta_out);

/* ---- native text I/O (host only) -------------------------------------------------------------------
 * Reader for the three gzip text tables (fithic/fithic.py:406-417 contacts, :581-590 fragments, :805-808 bias):
 * kind 0 = contacts (chr1 mid1 chr2 mid2 count), 1 = fragments (uses columns 0, 2, 3), 2 = bias (chr mid bias).
 * Chromosome names are interned in order of first appearance.  Columns for fhx_table_copy: 0 chr1, 1 mid1, 2 chr2, 3 mid2,
 * 4 count = int(float(text)) or hits (int32 each); 5 = the float itself / the bias (double).  A malformed line returns
 * FHX_ERR_REFERENCE_EXIT (the reference raises ValueError there); fhx_table_error gives the line number. */
typedef struct fhx_table fhx_table;
#define FHX_TABLE_NO_FLOAT 0x100   /* kind 0 | FHX_TABLE_NO_FLOAT: a contacts table without column 5 (8 B/row less to parse and keep) */
int fhx_host_read_table(const char* path, int32_t kind, int32_t n_threads, fhx_table** out);
int64_t fhx_table_rows(const fhx_table* t);
int32_t fhx_table_n_names(const fhx_table* t);
const char* fhx_table_name(const fhx_table* t, int32_t i);
const char* fhx_table_error(const fhx_table* t);
int fhx_table_copy(const fhx_table* t, int32_t column, void* dst);
/* ids[i] = the caller's id of fhx_table_name(t, i): columns 0 and 2 of later fhx_table_copy calls are in that id space. */
int fhx_table_map_names(fhx_table* t, const int32_t* ids, int32_t n_ids);
void fhx_table_free(fhx_table* t);
/* The two stages of fhx_host_read_table on their own.  fhx_host_inflate: the file read and inflated on the host cores - a file
 * of size-tagged members by one zlib per core, ONE plain gzip stream (what `gzip` writes) by csrc/fhx_gunzip.cpp: block starts
 * found by their headers, chunks decoded in parallel with the unknown 32 KB window as 16-bit symbols, windows resolved down the
 * chain, CRC-32 and ISIZE checked, zlib on one thread whenever any of that does not work out (an
 * object is returned even on failure, for fhx_text_error); fhx_host_parse_text: the table of that text.  The split exists for
 * fhx_ingest_contacts_text below, which parses the text on the GPU and leaves fhx_host_parse_text as the path for the files
 * it does not take. */
typedef struct fhx_text fhx_text;
int fhx_host_inflate(const char* path, int32_t n_threads, fhx_text** out);
int64_t fhx_text_bytes(const fhx_text* x);
int fhx_text_copy(const fhx_text* x, void* dst, int64_t cap);      /* the inflated bytes (cap >= fhx_text_bytes) */
const char* fhx_text_error(const fhx_text* x);
int fhx_host_parse_text(const fhx_text* text, int32_t kind, int32_t n_threads, fhx_table** out);
void fhx_text_free(fhx_text* x);
/* The contacts table written as the reference reads it ("%s\t%d\t%s\t%d\t%d\n", fithic/fithic.py:413-417) on all cores;
 * tooling for synthetic workloads.  Like every file this library writes it is a concatenation of gzip members that carry
 * their compressed size in an "FH" extra subfield - plain gzip to every other reader, inflated in parallel by
 * fhx_host_read_table (which does the same for bgzip's "BC" blocks). */
int fhx_host_write_contacts(const char* path, const char* const* chr_names, int32_t n_names, const int32_t* chr1,
                            const int32_t* mid1, const int32_t* chr2, const int32_t* mid2, const int32_t* count, int64_t n_rows,
                            int32_t gzip_level, int32_t n_threads);
/* Writer of <lib>.spline_passN.resR.significances.txt.gz (fithic/fithic.py:1167-1213): header + one
 * "%s\t%d\t%s\t%d\t%d\t%e\t%e\t%e\t%e\t%f" row per emitted contact (inter rows in All / interOnly mode, in-range intra
 * rows in All / intraOnly mode).  Rows are formatted and deflated in parallel, one gzip member per 65 536 rows; the
 * decompressed bytes equal the reference's.  n_threads <= 0: all host cores. */
int fhx_host_write_significances(const char* path, const char* const* chr_names, int32_t n_names, const int32_t* chr1,
                                 const int32_t* mid1, const int32_t* chr2, const int32_t* mid2, const int32_t* count,
                                 const double* p, const double* q, const double* bias1, const double* bias2,
                                 const double* expcc, int64_t n_rows, int32_t mode, int64_t dist_low, int64_t dist_up,
                                 int32_t gzip_level, int32_t n_threads, int64_t* rows_written);
/* The same file written BY THE GPU, for the p and q a context holds after fhx_pvalues + fhx_bh: rows are formatted in a
 * kernel (exact integer arithmetic: the characters C's printf gives), ExpCC and the biases recomputed there, and deflated in
 * kernels (tokens against the previous row + per-member dynamic Huffman codes built by the host from device histograms);
 * the host receives finished gzip members (same container as above) and only writes them.  The five identity columns are
 * the rows given to fhx_load_pairs (n_rows must equal the loaded row count); pass all five as NULL and they are rebuilt on
 * the device from the resident rows (slot -> chromosome, midpoint), so that nothing but the file leaves the GPU.  Returns FHX_ERR_UNSUPPORTED - nothing usable
 * written - when a row does not fit the device formatter (a chromosome name longer than 24 bytes, a value of 2^63 or more,
 * a row of 192 bytes or more): the caller then fetches the columns and uses fhx_host_write_significances. */
int fhx_write_significances_device(fhx_ctx* ctx, const char* path, const char* const* chr_names, int32_t n_names,
                                   const int32_t* chr1, const int32_t* mid1, const int32_t* chr2, const int32_t* mid2,
                                   const int32_t* count, int64_t n_rows, int64_t* rows_written, int64_t* bytes_written);
/* A stretch [row_begin, row_end) of the loaded rows written the same way (identity columns rebuilt on the device), as gzip members
 * of their own, with or without the column-header member in front.  The ranks of `fithic --gpus N` each write the stretches of the
 * file they hold; concatenated in file order the pieces are the reference's file (fithic/fithic.py:1167-1219). */
int fhx_write_significances_device_range(fhx_ctx* ctx, const char* path, const char* const* chr_names, int32_t n_names, int64_t row_begin,
                                         int64_t row_end, int32_t with_header, int64_t* rows_written, int64_t* bytes_written);
/* The FDR subset of the pass taken from its resident columns: the lines fhx_ms_select_file (below) keeps of the file
 * fhx_write_significances_device writes - the same bytes, or the same refusal - without that file.  Every loaded row gets the
 * writer's emit predicate and merge-filter.sh's decision on the %e text of its q (zero / numeric key <= key_bound / string
 * compare with fdr_text; key_bound, zero_kept and strict as for fhx_ms_select_file, whose line 1 is the header and no candidate);
 * only the kept rows are formatted.  Valid after fhx_bh of a pass and before fhx_next_pass (FHX_ERR_ARG otherwise).
 *   *n_emitted  rows the writer would print (the file has *n_emitted + 1 lines); *n_kept, *n_bytes: the subset.
 * Refused, nothing retrievable: an emitted row whose q is nan, inf, negative (-0.0 too) or prints an exponent of 308 -
 * FHX_ERR_UNSUPPORTED, *why = FHX_MS_FIELD, *bad_line = the line the smallest such row has in the written file (2 + the emitted
 * rows before it); a KEPT row the device formatter does not cover (a name longer than 24 bytes, a row of 192 bytes or more) -
 * FHX_ERR_UNSUPPORTED with *why = 0: select from the written file instead.  FHX_SR_NO_BRACKET=1 formats every emitted q instead of
 * deciding normal doubles outside [lo, hi] by value (the same subset; measurements and tests). */
int fhx_significant_select(fhx_ctx* ctx, const char* const* chr_names, int32_t n_names, const char* fdr_text, int32_t fdr_len,
                           uint64_t key_bound, int32_t zero_kept, int32_t strict, int64_t* n_emitted, int64_t* n_kept, int64_t* n_bytes,
                           int32_t* why, int64_t* bad_line);
int fhx_significant_copy_text(fhx_ctx* ctx, void* dst, int64_t capacity);     /* the n_bytes of the last selection */
int fhx_significant_copy_rows(fhx_ctx* ctx, int64_t* rows, int64_t capacity); /* loaded-row numbers of the kept rows, ascending */
/* The UCSC interact track of the pass taken from its resident columns (csrc/fhx_sigresident_track.inc): the text fhx_ms_track_file
 * (below) makes of the file fhx_write_significances_device writes - the same bytes, the script's two fixed lines included, or the
 * same refusal - without that file.  The decision is fhx_significant_select's with strict = 1 (key_bound and zero_kept as for
 * fhx_ms_track_file); line 1 of that file is fithic's header, which the track drops, so the file route's n_lines is *n_emitted + 1.
 * Same state rules as fhx_significant_select; a context without rows gives the two fixed lines.
 *   *n_kept lines behind the fixed two, *n_deferred of them with a score written by the host, *n_bytes the whole text.
 * Refused, nothing retrievable, FHX_ERR_UNSUPPORTED with *bad_line = the line the smallest such row has in the written file: an
 * EMITTED row, kept or not, whose q is outside the grammar (*why = FHX_MS_FIELD), whose midpoint is outside 0 ... 999 999 999
 * (FHX_MS_MIDPOINT) or whose name has more than 63 bytes (FHX_MS_NAME); a row with several faults reports the first of these.
 * More than 2^31 - 1 kept rows: FHX_MS_KEPT, no line.  A KEPT row with a name of more than 24 bytes: FHX_ERR_UNSUPPORTED with
 * *why = 0 - make the track from the written file instead.  The result of fhx_significant_select is left as it is. */
int fhx_significant_track(fhx_ctx* ctx, const char* const* chr_names, int32_t n_names, const char* fdr_text, int32_t fdr_len,
                          uint64_t key_bound, int32_t zero_kept, int64_t* n_emitted, int64_t* n_kept, int64_t* n_deferred,
                          int64_t* n_bytes, int32_t* why, int64_t* bad_line);
int fhx_significant_copy_track(fhx_ctx* ctx, void* dst, int64_t capacity);    /* the n_bytes of the last track */
/* The per-chromosome FDR subsets of the pass taken from its resident columns (csrc/fhx_sigresident_split.inc): what
 * fhx_ms_split_file (below) makes of the file fhx_write_significances_device writes - the same list, the same bytes per name, or
 * the same refusal - without that file.  The list is field 1 of every line of that file: the literal `chr1` of fithic's header and
 * the first chromosome of every emitted row (trans rows of an -x All or interOnly run included); a row goes to name c when it is
 * emitted, both its chromosomes are c and `$7 <= fdr` holds (the decision of fhx_significant_select with strict = 0).  A listed
 * name without such a row has an empty subset.  Same state rules as fhx_significant_select; a context without rows lists `chr1`.
 *   *n_emitted as for fhx_significant_select; *n_listed names, in bytewise order.
 * Refused, nothing retrievable, FHX_ERR_UNSUPPORTED with *bad_line = the line the smallest such row has in the written file: an
 * EMITTED row, kept or not, one of whose names fhx_ms_split_file would refuse (FHX_MS_NAME, FHX_MS_NAME_BYTES,
 * FHX_MS_NAME_NUMERIC; the first name before the second) or, after the names, whose q is outside the grammar (FHX_MS_FIELD).
 * More than FHX_MS_SPLIT_NAMES listed names: FHX_MS_NAMES, no line.  A KEPT row the device formatter does not cover:
 * FHX_ERR_UNSUPPORTED with *why = 0 - split the written file instead.  The results of fhx_significant_select and
 * fhx_significant_track are left as they are. */
int fhx_significant_split(fhx_ctx* ctx, const char* const* chr_names, int32_t n_names, const char* fdr_text, int32_t fdr_len,
                          uint64_t key_bound, int32_t zero_kept, int64_t* n_emitted, int32_t* n_listed, int32_t* why, int64_t* bad_line);
/* per listed name (capacity entries at least, either array may be NULL) its kept rows and their bytes */
int fhx_significant_split_counts(fhx_ctx* ctx, int64_t* kept_rows, int64_t* kept_bytes, int32_t capacity);
int fhx_significant_split_names(fhx_ctx* ctx, char* dst, int32_t capacity);   /* FHX_MS_SPLIT_NAME_BYTES per name, bytewise order */
int fhx_significant_copy_split(fhx_ctx* ctx, int32_t index, void* dst, int64_t capacity);   /* the subset of name `index` */

/* ---- Knight-Ruiz bias vectors (fithic/utils/HiCKRy.py; SURVEY 8f rank 4, the step before Fit-Hi-C) --------------------
 * One fhx_kr per GPU, independent of fhx_ctx.  Call order: load_loci -> load_pairs (or load_pairs_resident) -> [remove_sparse] ->
 * balance -> bias.
 * Summation orders are fixed by the kernels (csrc/fhx_kr.hip header) and restated by oracle/kr_oracle.c. */
typedef struct fhx_kr fhx_kr;
typedef struct fhx_kr_info {
    int64_t n, nnz;                 /* matrix that was balanced (after row removal) */
    int32_t outer_iterations;       /* `i` of knightRuizAlg's return value (31 = the 30-iteration cap was hit, HiCKRy.py:174) */
    int32_t inner_iterations;       /* `k` of the last outer iteration */
    int64_t matvecs;                /* A.dot calls */
    int64_t boundary_steps;         /* inner loops that ended on the cone boundary (HiCKRy.py:199-212) */
    double residual;                /* rout = |1 - x*(A x)|^2 at exit */
    double spmv_seconds;            /* HIP-event time of the timed SpMV launches */
    int64_t spmv_timed;
    int64_t value_bytes;            /* bytes per value streamed by the SpMV: 8 doubles; 4 binary32 (exact for integer counts), with 4-byte
                                     * columns either way; 2: the 4-byte cell (16-bit count + 16-bit column offset in its row) */
} fhx_kr_info;
int fhx_kr_create(int device, fhx_kr** out);
void fhx_kr_destroy(fhx_kr* kr);
const char* fhx_kr_last_error(const fhx_kr* kr);
/* fragments file, HiCKRy.py:21-33: locus index = line number; a repeated (chr, mid) maps to its last line. */
int fhx_kr_load_loci(fhx_kr* kr, const int32_t* chr, const int32_t* mid, int64_t n);
/* interactions file, HiCKRy.py:34-54: rawMatrix = coo((value,(x,y))) + its transpose, assembled as CSR in HBM.  A row whose
 * locus is not in the fragments file returns FHX_ERR_REFERENCE_EXIT (KeyError) and its row number. */
int fhx_kr_load_pairs(fhx_kr* kr, const int32_t* chr1, const int32_t* mid1, const int32_t* chr2, const int32_t* mid2,
                      const double* value, int64_t m, int64_t* first_unknown_row);
/* The same matrix from the contact rows an engine context holds on the same device (HiCKRy.py:18-54 without a second read of
 * the interactions file; csrc/fhx_kr_resident.inc): fhx_kr_load_loci has run with the fragment lines, whose chromosome ids are
 * the ids the context's rows were loaded with.  Every loaded row enters the matrix, whatever the pass state and the contact
 * type; neither the rows nor the pass state change.  On success the context is in the state fhx_kr_load_pairs leaves for the same
 * rows, bit for bit.  FHX_ERR_ARG: no rows, or another device.  FHX_ERR_REFERENCE_EXIT: as fhx_kr_load_pairs, the row being the
 * file position where the context carries them (fhx_set_global_rows).  FHX_ERR_UNSUPPORTED: some count of the contacts text
 * had a non-zero fractional digit ("3.5"; "3.0" and "3." are integers) - HiCKRy balances float(count), the rows hold
 * int(float(count)): use fhx_kr_load_pairs.  Rows given as int32 arrays (fhx_load_pairs, fhx_load_pairs_device) are integers. */
int fhx_kr_load_pairs_resident(fhx_kr* kr, fhx_ctx* ctx, int64_t* first_unknown_row);
int fhx_kr_shape(const fhx_kr* kr, int64_t* n_full, int64_t* nnz_full, int64_t* n_reduced, int64_t* nnz_reduced);
/* which 0 = raw matrix, 1 = after remove_sparse; any output pointer may be NULL */
int fhx_kr_get_csr(fhx_kr* kr, int32_t which, int64_t* indptr, int32_t* col, double* val);
/* mtx.sum(axis=0), HiCKRy.py:78 */
int fhx_kr_row_sums(fhx_kr* kr, double* out);
/* removeZeroDiagonalCSR, HiCKRy.py:74-101: drops every row/column whose sum is <= the int(perc*n)-th smallest sum. */
int fhx_kr_remove_sparse(fhx_kr* kr, double perc, int64_t* n_removed, double* val_to_remove, int64_t* rem_rows);
int fhx_kr_get_removed(const fhx_kr* kr, int64_t* idx, int64_t capacity, int64_t* n_out);
/* knightRuizAlg, HiCKRy.py:139-243 (tol = 1e-6 in the reference's call) */
int fhx_kr_balance(fhx_kr* kr, double tol, fhx_kr_info* out);
int fhx_kr_get_x(const fhx_kr* kr, double* x);
/* computeBiasVector + addZeroBiases, HiCKRy.py:103-115: n_full values, -1 at the removed rows */
int fhx_kr_bias(fhx_kr* kr, double* bias);
/* test / measurement hooks: y = A x (host vectors), repeated `repeats` times with HIP-event timing; ordered dot product */
int fhx_kr_spmv(fhx_kr* kr, int32_t which, const double* x, double* y, int32_t repeats, double* seconds_per_call);
int fhx_kr_dot(fhx_kr* kr, const double* a, const double* b, int64_t n, double* out);

/* ---- merging of nearby significant contacts (fithic/utils/CombineNearbyInteraction.py; SURVEY 8f rank 4, the step after
 * Fit-Hi-C).  The caller parses the significances table, keeps the rows with chr1 == chr2 (:258-266), numbers the chromosomes
 * in the order they are to be written (byte-sorted names, :204-212) and passes n = int(float(mid) + res/2) (:301-303).
 * All numerators must share one offset modulo the resolution (true for every fixed-size Fit-Hi-C output); -p 0 is refused:
 * its result depends on CPython's set iteration order (:417-437). */
typedef struct fhx_cni fhx_cni;
typedef struct fhx_cni_info {
    int64_t rows, nodes, components, selected, pick_rounds, largest_component;
} fhx_cni_info;
typedef struct fhx_cni_record {        /* one output line (:589-600); bins are n / res */
    int32_t chr, reserved;
    int64_t n_lo, n_hi;                /* the picked cell */
    int64_t cc;
    double p, q;                       /* of the first row of that cell */
    int64_t box_min_lo, box_max_lo, box_min_hi, box_max_hi;   /* bounding box of its component (numerators) */
    int64_t sum_cc;                    /* over the component's cells */
    int64_t box_cells;                 /* cells of the chromosome inside the box (0 when bins are not whole numbers) */
    int64_t component_size;
    int64_t first_row;                 /* input row the cell's values come from */
} fhx_cni_record;
int fhx_cni_create(int device, fhx_cni** out);
void fhx_cni_destroy(fhx_cni* cn);
const char* fhx_cni_last_error(const fhx_cni* cn);
int fhx_cni_load(fhx_cni* cn, const int32_t* chr, const int64_t* n1, const int64_t* n2, const int64_t* cc, const double* p,
                 const double* q, int64_t rows, int64_t bin_size, int64_t* n_nodes);
/* connectivity 8|4 (-c), top_percent 1..100 (-p), neighborhood in bins (-n), sort_order 0|1 (-s) */
int fhx_cni_run(fhx_cni* cn, int32_t connectivity, int32_t top_percent, int32_t neighborhood, int32_t sort_order,
                fhx_cni_info* info);
int fhx_cni_get_records(const fhx_cni* cn, fhx_cni_record* out, int64_t capacity, int64_t* n_out);

/* ---- HiC-Pro matrix -> Fit-Hi-C contact columns and per-bin totals (fithic/utils/HiCPro2FitHiC.py:33-53; csrc/fhx_hicpro.hip).
 * One handle per GPU, independent of fhx_ctx.  The caller reads the bed file (one line per bin) and passes the bins as a dense
 * table over [index_base, index_base + n_slots): chr_id = -1 marks an index the bed does not list.  The matrix file (plain text,
 * `i j count` per line) is uploaded as it is and parsed by kernels; the five contact columns (chr1, mid1, chr2, mid2, count: int32,
 * file order) and the totals (every line adds its count to bin i and to bin j, exact 64-bit integers) stay in HBM.
 * Only the regular file is taken: ASCII, exactly three tokens per line, i and j = [+-]digits (10 digits at most, within int32), count
 * = digits[.digits] (15 digits at most, integer part within int32, every fraction digit 0); \r\n and a last line without newline
 * are fine.  Anything else is refused with nothing left loaded: *why = one of FHX_HP_*, *bad_line = the smallest offending 1-based
 * line number.  Return value: FHX_ERR_REFERENCE_EXIT for FHX_HP_ABSENT (the reference raises KeyError(*bad_index) there),
 * FHX_ERR_UNSUPPORTED for the other reasons. */
#define FHX_HP_OK 0
#define FHX_HP_TOKENS 1            /* not exactly three tokens (an empty line included) */
#define FHX_HP_INDEX 2             /* i or j is not [+-]digits of at most 10 digits within int32 */
#define FHX_HP_COUNT 3             /* the count is not digits[.digits] of at most 15 digits with the integer part within int32 */
#define FHX_HP_FRACTION 4          /* a count with a fraction digit other than 0 */
#define FHX_HP_ABSENT 5            /* an index outside the table or absent from the bed */
#define FHX_HP_BYTES 6             /* a NUL, a non-ASCII byte, a \r that is not followed by \n */
#define FHX_HP_LONG_LINE 7         /* a line of more than 4096 bytes */
#define FHX_HP_TOTAL 8             /* a bin total of 2^53 or more: the reference's float sum would have rounded (no line number) */
#define FHX_HP_INTERNAL 9          /* a device-side consistency check failed */
typedef struct fhx_hp fhx_hp;
int fhx_hp_create(int device, fhx_hp** out);
void fhx_hp_destroy(fhx_hp* hp);
const char* fhx_hp_last_error(const fhx_hp* hp);
int fhx_hp_load_bins(fhx_hp* hp, int64_t index_base, const int32_t* chr_id, const int32_t* mid, int64_t n_slots);
int fhx_hp_parse_matrix(fhx_hp* hp, const char* path, int64_t* n_rows, int32_t* why, int64_t* bad_line, int64_t* bad_index);
int fhx_hp_totals(fhx_hp* hp, int64_t* tcc);                       /* n_slots values */
int fhx_hp_fetch_rows(fhx_hp* hp, int32_t* chr1, int32_t* mid1, int32_t* chr2, int32_t* mid2, int32_t* count);   /* n_rows each */
/* the columns in HBM (which 0..4 = chr1, mid1, chr2, mid2, count) and the stream they were written on, for fhx_load_pairs_device;
 * valid until the next fhx_hp_parse_matrix / fhx_hp_load_bins / fhx_hp_destroy */
void* fhx_hp_device_ptr(fhx_hp* hp, int32_t which);
void* fhx_hp_stream(fhx_hp* hp);

/* ---- HiC-Pro allValidPairs -> Fit-Hi-C contact counts (fithic/utils/validPairs2FitHiC-fixedSize.sh:33-40; csrc/fhx_validpairs.hip).
 * One handle per GPU, independent of fhx_ctx.  The file (plain text, or gzip: it is inflated on the host first, as zcat -f does)
 * goes through HBM in batches cut at the last newline (FHX_VP_BATCH_BYTES overrides the batch size of 256 MB; 8192 at least);
 * kernels split every line on blanks, apply the script's filters - both names of at most 5 bytes, no `chrM` anywhere in the
 * line, different names or (pos1 - pos2)^2 > 2 * res - bin both ends (pos / res), order them as the script's awk does, sort and
 * count.  The cells (chr1, mid1, chr2, mid2, count: int32; mid = bin start + res / 2; chr = index into the names, which are in
 * bytewise order) stay in HBM in the order of the script's `sort` under LC_ALL=C: the lines name1 TAB bin1 TAB name2 TAB bin2
 * compared as text.
 * Taken: printable ASCII and tabs, lines of at most 4096 bytes ending in \n or \r\n (the last one may end with the file), at
 * least 6 tokens per line; on a line the first two filters keep: names that start with a letter or `_` (not with inf / nan in
 * any case) or are decimal digits without a leading zero, positions of 1..10 digits with bin start + res / 2 < 2^31.  res is even
 * and >= 2.  At most 1024 distinct names, and 2 * (bits of the largest bin index + bits of the largest name rank) <= 64.
 * Anything else is refused with nothing left loaded: *why = one of FHX_VP_*, *bad_line = the smallest offending 1-based line
 * number (0 for the reasons that belong to no line).  Return value: FHX_ERR_UNSUPPORTED. */
#define FHX_VP_OK 0
#define FHX_VP_TOKENS 1            /* fewer than six tokens (an empty line included) */
#define FHX_VP_NAME 2              /* a name awk would, or might, compare as a number */
#define FHX_VP_POSITION 3          /* a position that is not 1..10 digits */
#define FHX_VP_RANGE 4             /* bin start + res / 2 >= 2^31: awk prints such a number in %.6g form */
#define FHX_VP_BYTES 5             /* a NUL, another control byte than tab, DEL, a non-ASCII byte, a \r that is not followed by \n */
#define FHX_VP_LONG_LINE 6         /* a line of more than 4096 bytes */
#define FHX_VP_NAMES 7             /* more distinct names, or larger bin indices, than the 64-bit sort key holds (no line number) */
#define FHX_VP_COUNT 8             /* a cell hit by more than 2^31 - 1 pairs (no line number) */
#define FHX_VP_RES 9               /* res is odd or below 2 (no line number) */
#define FHX_VP_INTERNAL 10         /* a device-side consistency check failed */
#define FHX_VP_PAIRS 11            /* 2^32 or more pairs could be kept: the sort does not take them (no line number) */
#define FHX_VP_STAGES 6            /* read + upload, newline scan, parse, names + keys, sort, cells */
typedef struct fhx_vp fhx_vp;
int fhx_vp_create(int device, fhx_vp** out);
void fhx_vp_destroy(fhx_vp* vp);
const char* fhx_vp_last_error(const fhx_vp* vp);
int fhx_vp_bin_file(fhx_vp* vp, const char* path, int64_t res, int64_t* n_cells, int32_t* why, int64_t* bad_line);
int fhx_vp_counts(const fhx_vp* vp, int64_t* n_lines, int64_t* n_pairs, int64_t* n_cells, int32_t* n_names);
const char* fhx_vp_name(const fhx_vp* vp, int32_t i);
int fhx_vp_stage_seconds(const fhx_vp* vp, double* seconds);       /* FHX_VP_STAGES host clocks of the last call */
int fhx_vp_fetch_cells(fhx_vp* vp, int32_t* chr1, int32_t* mid1, int32_t* chr2, int32_t* mid2, int32_t* count);   /* n_cells each */
/* the columns in HBM (which 0..4 = chr1, mid1, chr2, mid2, count) and the stream they were written on, for fhx_load_pairs_device;
 * valid until the next fhx_vp_bin_file / fhx_vp_destroy */
void* fhx_vp_device_ptr(fhx_vp* vp, int32_t which);
void* fhx_vp_stream(fhx_vp* vp);
/* The cells as the script writes them: name1 TAB mid1 TAB name2 TAB mid2 TAB count, the count right-justified to width 7 as
 * uniq -c prints it (:38-39); size-tagged gzip members through the pool of the host writer.  Host only: needs no GPU. */
int fhx_vp_write_contacts(const char* path, const char* const* chr_names, int32_t n_names, const int32_t* chr1,
                          const int32_t* mid1, const int32_t* chr2, const int32_t* mid2, const int32_t* count, int64_t n_rows,
                          int32_t gzip_level, int32_t n_threads);

/* ---- the FDR subset of a significances file (fithic/utils/merge-filter.sh:22; csrc/fhx_sigselect.hip).
 * One handle per GPU, independent of fhx_ctx.  The file (plain text, or gzip: it is inflated on the host first) goes through HBM
 * in batches cut at the last newline (FHX_MS_BATCH_BYTES overrides the batch size of 256 MB; 8192 at least); kernels split every
 * line on blanks, find field 7 and decide `$7 <= fdr` (`$7 < fdr` when strict) as mawk 1.3.4 decides it on the TEXT of the
 * field, and gather the kept lines verbatim, in file order, each ending in a newline.  The subset stays in host memory.
 * Taken: printable ASCII and tabs, lines of at most 4096 bytes ending in \n (the last one may end with the file), at least 7
 * tokens per line, field 7 written as C's %e writes a non-negative finite double: D.DDDDDDe[+-]XX or e[+-]XXX.  Such a field is
 *   zero     every digit 0: kept when zero_kept is set (the caller knows whether 0 <= fdr, or 0 < fdr);
 *   numeric  first digit 1-9 and a value in [2.225074e-308, 9.999999e+307]: kept when its key
 *            (exponent + 308) * 10^7 + the seven digits as one integer  is <= key_bound (0 keeps none): strtod is monotone in
 *            the key, so the caller finds the bound by bisection with its own strtod;
 *   string   a non-zero value below 2.225074e-308, or an exponent of 309 and more (mawk's strtod flags ERANGE there and awk
 *            compares strings): kept when the field's bytes compare <= (< when strict) with fdr_text, memcmp then length.
 * An exponent of exactly 308 is refused: mawk compares numbers up to 1.797693e+308 and strings above.
 * With skip_first_line set, line 1 of the file is dropped without being parsed (the byte and length rules still hold for it).
 * Anything else is refused and no subset is kept: *why = one of FHX_MS_*, *bad_line = the smallest offending 1-based line number
 * (0 for FHX_MS_FDR).  Return value: FHX_ERR_UNSUPPORTED. */
#define FHX_MS_OK 0
#define FHX_MS_TOKENS 1            /* fewer than seven tokens (an empty line included) */
#define FHX_MS_FIELD 2             /* field 7 is not in the %e shape, starts with 0 without being zero, or has exponent 308 */
#define FHX_MS_BYTES 3             /* a NUL, another control byte than tab (\r included), DEL, a non-ASCII byte */
#define FHX_MS_LONG_LINE 4         /* a line of more than 4096 bytes */
#define FHX_MS_FDR 5               /* the text of fdr is empty or longer than FHX_MS_FDR_BYTES (no line number) */
#define FHX_MS_INTERNAL 6          /* a device-side consistency check failed */
#define FHX_MS_FDR_BYTES 32
#define FHX_MS_STAGES 5            /* read + upload, newline scan, select, gather, copy out */
typedef struct fhx_ms fhx_ms;
int fhx_ms_create(int device, fhx_ms** out);
void fhx_ms_destroy(fhx_ms* ms);
const char* fhx_ms_last_error(const fhx_ms* ms);
int fhx_ms_select_file(fhx_ms* ms, const char* path, const char* fdr_text, int32_t fdr_len, uint64_t key_bound, int32_t zero_kept,
                       int32_t strict, int32_t skip_first_line, int64_t* n_bytes, int32_t* why, int64_t* bad_line);
int fhx_ms_counts(const fhx_ms* ms, int64_t* n_lines, int64_t* n_kept, int64_t* n_bytes);
int fhx_ms_stage_seconds(const fhx_ms* ms, double* seconds);       /* FHX_MS_STAGES host clocks of the last call */
int fhx_ms_copy_subset(const fhx_ms* ms, void* dst, int64_t capacity);   /* the n_bytes of the last selection */

/* ---- the UCSC interact track of the significant contacts (fithic/utils/visualize-UCSC.sh:16-18; csrc/fhx_sigtrack.inc,
 * csrc/fhx_score.hpp), on the same handle.  The selection is fhx_ms_select_file's with strict = 1 and no line skipped, plus one
 * rule: on FILE LINE 1 a field 7 that starts with an ASCII letter (`q-value`) is a string above every accepted threshold, and the
 * line is dropped without a refusal (fewer than 7 tokens are refused there too).  Every kept line becomes
 *   $1 ($2-1) ($4+1) NR int(-log($7)/log(10)) -log($7)/log(10) EXP 0 $1 ($2-1) ($2+1) SOURCE_NAME . $3 ($4-1) ($4+1) TARGET_NAME +
 * joined by single blanks, NR counting the kept lines from 1, behind the script's two fixed lines; the whole text stays in host
 * memory.  The two score fields are the bytes mawk 1.3.4 prints: written in the kernel where an error bound certifies them,
 * otherwise DEFERRED - field 7 goes to the host, which makes awk's own libm calls, and the line is completed on the device.
 * Taken beyond fhx_ms_select_file's grammar, on every line that is parsed, kept or not: tokens 2 and 4 are 1 to 9 ASCII digits
 * (leading zeros allowed), tokens 1 and 3 at most 63 bytes. */
#define FHX_MS_MIDPOINT 7          /* token 2 or 4 is not 1 to 9 digits */
#define FHX_MS_NAME 8              /* token 1 or 3 is longer than 63 bytes */
#define FHX_MS_KEPT 9              /* more than 2^31 - 1 lines pass: awk prints NR through %.6g from there (no line number) */
#define FHX_MS_TRACK_STAGES 6      /* read + upload, newline scan, select, deferred round trip, measure + format, copy out */
int fhx_ms_track_file(fhx_ms* ms, const char* path, const char* fdr_text, int32_t fdr_len, uint64_t key_bound, int32_t zero_kept,
                      int64_t* n_bytes, int32_t* why, int64_t* bad_line);
int fhx_ms_track_counts(const fhx_ms* ms, int64_t* n_lines, int64_t* n_kept, int64_t* n_deferred, int64_t* n_bytes);
int fhx_ms_track_stage_seconds(const fhx_ms* ms, double* seconds);  /* FHX_MS_TRACK_STAGES host clocks of the last call */
int fhx_ms_copy_track(const fhx_ms* ms, void* dst, int64_t capacity);    /* the n_bytes of the last track */
/* The two score fields and the blank between them for one field 7 (1 to 15 bytes) into out (24 bytes at least) -> their length.
 * certify = 0: the deferred route (strtod, log, the division, awk's number printing); certify = 1: the kernel's route run on the
 * host, 0 when it would defer.  Host only: needs no GPU. */
int fhx_ms_score_text(const char* field, int32_t len, int32_t certify, char* out, int32_t capacity);

/* ---- the per-chromosome FDR subsets of a significances file (fithic/utils/merge-filter-parallelized.sh:21-25;
 * csrc/fhx_sigsplit.inc), on the same handle.  The script lists field 1 of EVERY line (`cut -f1 | sort | uniq`, line 1 included) and,
 * once per listed name c, keeps the rows with `NR != 1 && $1 == c && $3 == c && $7 <= fdr`.  Here one read of the file gives
 * every subset: the `$7` decision is fhx_ms_select_file's (not strict, line 1 dropped), the names of field 1 are interned on the
 * device (at most FHX_MS_SPLIT_NAMES), the kept lines are sorted by (name, file offset) and gathered so that each name's lines
 * reach the host as one run per batch, verbatim and in file order, each ending in a newline.  A name with no kept line (a name
 * seen only in trans rows or only on line 1) is still listed, with an empty subset.
 * Taken beyond fhx_ms_select_file's grammar, on every line (on line 1: the rules for token 1 only): token 1 starts in column 0
 * and is ended by a tab (cut's field 1 and awk's $1 are then the same bytes); tokens 1 and 3 are 1 to 63 bytes of
 * [A-Za-z0-9_.-] that start with a letter, a digit or `_`; a name that starts with a digit is a decimal integer of at most 15
 * digits without a leading zero, or holds `_` or a letter other than a-f, x, p in either case (strtod cannot consume it whole) -
 * so awk's `$1 == c` between two accepted names is byte equality.  Names are returned in no particular order. */
#define FHX_MS_NAME_TAB 10         /* token 1 does not start in column 0, or is not ended by a tab */
#define FHX_MS_NAME_BYTES 11       /* token 1 or 3 holds a byte outside [A-Za-z0-9_.-] or starts with `.` or `-` */
#define FHX_MS_NAME_NUMERIC 12     /* token 1 or 3 starts with a digit and awk would, or might, compare it as a number */
#define FHX_MS_NAMES 13            /* more than FHX_MS_SPLIT_NAMES distinct names in field 1 (no line number) */
#define FHX_MS_SPLIT_NAMES 4096
#define FHX_MS_SPLIT_NAME_BYTES 64 /* per name in fhx_ms_split_names: the name, then zero bytes */
#define FHX_MS_SPLIT_STAGES 5      /* read + upload, newline scan, names + select, sort + gather, copy out */
int fhx_ms_split_file(fhx_ms* ms, const char* path, const char* fdr_text, int32_t fdr_len, uint64_t key_bound, int32_t zero_kept,
                      int32_t* n_names, int32_t* why, int64_t* bad_line);
/* lines read, names listed, and per name (capacity entries at least, either array may be NULL) its kept lines and their bytes */
int fhx_ms_split_counts(const fhx_ms* ms, int64_t* n_lines, int32_t* n_names, int64_t* kept_lines, int64_t* kept_bytes, int32_t capacity);
int fhx_ms_split_names(const fhx_ms* ms, char* dst, int32_t capacity);   /* FHX_MS_SPLIT_NAME_BYTES per name, capacity names */
int fhx_ms_split_stage_seconds(const fhx_ms* ms, double* seconds);  /* FHX_MS_SPLIT_STAGES host clocks of the last call */
int fhx_ms_copy_split(const fhx_ms* ms, int32_t index, void* dst, int64_t capacity);   /* the subset of name `index` */

/* ---- Juicer dump text -> Fit-Hi-C contact counts (fithic/utils/createFitHiCContacts-hic_old.sh:6 and
 * fithic/utils/createFitHiCContacts-hic.py:93; csrc/fhx_juicer.hip).  The input is what `juicer_tools dump` / `straw` prints for
 * one chromosome pair, `binX binY count` per line, plain or gzipped; it goes through HBM in batches cut at the last newline
 * (FHX_JC_BATCH_BYTES overrides the batch size of 256 MB; 8192 at least).  Every line gives exactly one output line.
 *   resolution == 0, VERBATIM mode (the old script): `name1 \t $1 \t name2 \t $2 \t $3 \n` with awk's fields copied as text - split
 *     at runs of blank and tab, a missing field empty, tokens after the third ignored, a last line without a newline given one.
 *   resolution >= 1, MIDPOINT mode (the .py): `name1 \t binX+int(R/2) \t name2 \t binY+int(R/2) \t count \n`, the count as Python's
 *     str() of a whole float (`17`, `17.0` and `017` give `17.0`); the five int32 columns (id1, mid1, id2, mid2, count) are made
 *     at row = line number.  Grammar: exactly three tokens; the bins 1 to 10 digits without a sign, multiples of R, midpoint at
 *     most 2^31 - 1; the count `digits` or `digits.` and one or more `0`, at most 15 digits, at most 2^24.
 * A name is 1 to FHX_JC_NAME_BYTES bytes of [A-Za-z0-9_.-] (FHX_ERR_ARG otherwise).  keep_text appends the output text to the
 * handle's text, keep_rows (midpoint mode) appends the rows to the handle's columns in HBM: several dumps make one table.
 * Anything else is refused and the handle is left empty (rows and text of earlier calls included): *why = one of FHX_JC_*, checked
 * in this order on a line, *bad_line = the smallest offending 1-based line of this file.  Return value: FHX_ERR_UNSUPPORTED. */
#define FHX_JC_OK 0
#define FHX_JC_BYTES 1             /* a NUL, another control byte than tab (\r included), DEL, a non-ASCII byte */
#define FHX_JC_LONG_LINE 2         /* a line of more than 4096 bytes */
#define FHX_JC_TOKENS 3            /* midpoint mode: not exactly three tokens */
#define FHX_JC_BIN 4               /* binX or binY is not 1 to 10 digits */
#define FHX_JC_GRID 5              /* binX or binY is no multiple of the resolution */
#define FHX_JC_RANGE 6             /* bin + int(R/2) is above 2^31 - 1 */
#define FHX_JC_COUNT 7             /* the count is no number, has more than 15 digits or is above 2^24 */
#define FHX_JC_FRACTION 8          /* a fraction, an exponent, a sign, nan or inf: a raw (NONE) dump is expected */
#define FHX_JC_INTERNAL 9          /* a device-side consistency check failed */
#define FHX_JC_NAME_BYTES 66       /* `chr` + 63 */
#define FHX_JC_STAGES 5            /* read + upload, newline scan, parse, format, copy out: summed over the calls since the last reset */
typedef struct fhx_jc fhx_jc;
int fhx_jc_create(int device, fhx_jc** out);
void fhx_jc_destroy(fhx_jc* jc);
const char* fhx_jc_last_error(const fhx_jc* jc);
int fhx_jc_reset(fhx_jc* jc);                                      /* drops rows, text and stage clocks */
int fhx_jc_convert_file(fhx_jc* jc, const char* path, const char* name1, const char* name2, int64_t resolution, int32_t id1, int32_t id2,
                        int32_t keep_text, int32_t keep_rows, int64_t* n_lines, int32_t* why, int64_t* bad_line);
int fhx_jc_counts(const fhx_jc* jc, int64_t* n_lines, int64_t* n_rows, int64_t* n_bytes);
int fhx_jc_stage_seconds(const fhx_jc* jc, double* seconds);
int fhx_jc_copy_text(const fhx_jc* jc, void* dst, int64_t capacity);      /* the n_bytes kept so far */
int fhx_jc_fetch_rows(fhx_jc* jc, int32_t* chr1, int32_t* mid1, int32_t* chr2, int32_t* mid2, int32_t* count);   /* n_rows each */
/* the kept columns in HBM (which = 0..4: chr1, mid1, chr2, mid2, count; NULL without rows) and the stream that wrote them; valid
 * until the next fhx_jc_convert_file / fhx_jc_reset / fhx_jc_destroy */
void* fhx_jc_device_ptr(fhx_jc* jc, int32_t which);
void* fhx_jc_stream(fhx_jc* jc);

/* ---- a FASTA cut with restriction enzymes -> the fragments file of `fithic -r 0`
 * (fithic/utils/createFitHiCFragments-nonfixedsize.sh: HiC-Pro's digest_genome.py, then the script's loop; csrc/fhx_digest.hip).
 * The FASTA, plain or gzipped, goes through HBM in batches cut at the last newline (FHX_DG_BATCH_BYTES overrides the batch size of
 * 256 MB; 8192 at least).  A line that begins with `>` starts a contig named by the bytes behind `>` up to the first blank, tab or
 * \r; every other line adds its bytes to the contig's sequence, case folded; lines before the first header add to nothing.
 * motifs: n_motifs x FHX_DG_MAX_MOTIF bytes, each motif's lengths[m] letters of acgt in either case first (an N of the site comes
 * expanded), offsets[m] = where the site cuts (0 .. lengths[m]).  Every start s at which the sequence equals a motif gives the site
 * s + offset; overlapping matches count, a motif runs across line ends and never across a header.  Per contig the sites come
 * sorted, equal ones kept.
 * Anything else is refused and the handle is left empty: *why = one of FHX_DG_*, *bad_line = the smallest offending 1-based line
 * (of a contig that is too long: its header's).  Return value: FHX_ERR_UNSUPPORTED. */
#define FHX_DG_OK 0
#define FHX_DG_BYTES 1             /* a NUL, a control byte other than \n and a \r directly before \n, DEL, a non-ASCII byte */
#define FHX_DG_BLANK 2             /* a blank or a tab in a line that is no header */
#define FHX_DG_LONG_LINE 3         /* a line of more than 4096 bytes */
#define FHX_DG_CONTIG_LENGTH 4     /* a contig of more than 2^31 - 1 bases */
#define FHX_DG_EMPTY_NAME 5        /* `>` alone, or `>` followed by a blank or a tab */
#define FHX_DG_NAME_CHARS 6        /* a name that holds one of * ? [ \ */
#define FHX_DG_DUPLICATE 7         /* a name seen before */
#define FHX_DG_NO_HEADER 8         /* no header line in the file (bad_line = 1) */
#define FHX_DG_INTERNAL 9          /* a device-side consistency check failed */
#define FHX_DG_MAX_MOTIF 16        /* bases per motif */
#define FHX_DG_MAX_MOTIFS 64
#define FHX_DG_STAGES 6            /* read + upload, newline scan, class pass, sites, sort, names + fetch: of the last digest */
typedef struct fhx_dg fhx_dg;
int fhx_dg_create(int device, fhx_dg** out);
void fhx_dg_destroy(fhx_dg* dg);
const char* fhx_dg_last_error(const fhx_dg* dg);
int fhx_dg_digest_file(fhx_dg* dg, const char* path, const char* motifs, const int32_t* lengths, const int32_t* offsets, int32_t n_motifs,
                       int32_t* why, int64_t* bad_line);
/* lines read, contigs, their bases in all, cut sites */
int fhx_dg_counts(const fhx_dg* dg, int64_t* n_lines, int64_t* n_contigs, int64_t* seq_bytes, int64_t* n_sites);
const char* fhx_dg_name(const fhx_dg* dg, int64_t contig);         /* NULL outside 0 .. n_contigs - 1; valid until the next digest */
int64_t fhx_dg_contig_length(const fhx_dg* dg, int64_t contig);    /* -1 outside 0 .. n_contigs - 1 */
int fhx_dg_fetch_sites(fhx_dg* dg, int32_t* contig, int32_t* position);   /* n_sites each, ordered by contig, then position */
int fhx_dg_stage_seconds(const fhx_dg* dg, double* seconds);
/* Host side, no GPU: the two files made of a digest.  sites are ordered by (contig, position); a contig with the sites c1 <= ... <= ck
 * has the k + 1 fragments [0, c1], [c1, c2], ..., [ck, length], empty ones included.
 *   fhx_dg_write_fragments: gzip, one line `chr<contig + 1> \t 0 \t end \t 1 \t 1 \n` per fragment - what the script's loop writes
 *   fhx_dg_write_bed: plain text, HiC-Pro's `name \t start \t end \t HIC_<name>_<k> \t 0 \t + \n`, k from 1 within the contig
 * gzip_level outside 0-9 means 6; n_threads <= 0 means every usable CPU. */
int fhx_dg_write_fragments(const char* path, int64_t n_contigs, const int64_t* lengths, const int32_t* site_contig, const int32_t* site_position,
                           int64_t n_sites, int32_t gzip_level, int32_t n_threads);
int fhx_dg_write_bed(const char* path, const char* const* names, int64_t n_contigs, const int64_t* lengths, const int32_t* site_contig,
                     const int32_t* site_position, int64_t n_sites, int32_t n_threads);

/* ---- HiC-Pro allValidPairs -> contact counts between the RESTRICTION FRAGMENTS of a digest, for `fithic -r 0`
 * (csrc/fhx_fragpairs.hip; the reference has no script for it, the semantics are this project's: INTEGRATION.md).
 * One handle per GPU, independent of fhx_ctx.  fhx_fp_load_table gives the fragments: per contig c (0-based, file order) the
 * ascending ends E_c of its fragments - its cut sites with duplicates kept, then its length - as rows first[c] .. first[c + 1] - 1 of
 * `ends` (first[0] = 0, first[n_contigs] = n_frags, every contig has at least one row), and the names a line may use:
 * name_text holds n_names x FHX_FP_NAME_BYTES bytes, each name zero-padded (1 to 63 bytes of name, no two equal), name_contig[k]
 * is the contig that name k stands for or -1 for a name whose lines are dropped.  At most FHX_FP_MAX_CONTIGS contigs, twice as
 * many names, fewer than 2^31 fragments: FHX_ERR_UNSUPPORTED beyond that, FHX_ERR_ARG for a table that is not as described.
 * fhx_fp_bin_file takes the file (plain text, or gzip: it is inflated on the host first) through HBM in batches cut at the last
 * newline (FHX_FP_BATCH_BYTES overrides the batch size of 256 MB; 8192 at least).  A line is split on blanks and tabs; token 2 is
 * name1, token 3 pos1, token 5 name2, token 6 pos2; nothing else is read.  A line with a dropped name is dropped and counted, its
 * positions unread.  A position p (1-based) of contig c lies in the fragment bisect_left(E_c, p): start < p <= end, an empty fragment
 * is never hit.  g = the row of the fragment; the pair is ordered g1 < g2, a pair with g1 == g2 is dropped and counted.  The cells
 * (contig1, E[g1], contig2, E[g2], count: int32) stay in HBM in ascending (g1, g2).
 * Taken: printable ASCII and tabs, lines of at most 4096 bytes ending in \n or \r\n (the last one may end with the file), at
 * least 6 tokens per line, names of the table, positions of 1..10 digits from 1 to the contig's length.  Anything else is refused
 * with nothing left loaded: *why = one of FHX_FP_*, *bad_line = the smallest offending 1-based line number (0 for the reasons that
 * belong to no line).  Return value: FHX_ERR_UNSUPPORTED. */
#define FHX_FP_OK 0
#define FHX_FP_TOKENS 1            /* fewer than six tokens (an empty line included) */
#define FHX_FP_NAME 2              /* a name that is neither a contig of the table nor dropped */
#define FHX_FP_POSITION 3          /* a position that is not 1..10 digits */
#define FHX_FP_RANGE 4             /* position 0, or one above the contig's length */
#define FHX_FP_BYTES 5             /* a NUL, another control byte than tab, DEL, a non-ASCII byte, a \r that is not followed by \n */
#define FHX_FP_LONG_LINE 6         /* a line of more than 4096 bytes */
#define FHX_FP_COUNT 7             /* a cell hit by more than 2^31 - 1 pairs (no line number) */
#define FHX_FP_INTERNAL 8          /* a device-side consistency check failed */
#define FHX_FP_PAIRS 9             /* 2^32 or more pairs could be kept: the sort does not take them (no line number) */
#define FHX_FP_MAX_CONTIGS 4096
#define FHX_FP_NAME_BYTES 64
#define FHX_FP_STAGES 6            /* read + upload, newline scan, parse, sort, cells: of the last file; then the last table's upload */
typedef struct fhx_fp fhx_fp;
int fhx_fp_create(int device, fhx_fp** out);
void fhx_fp_destroy(fhx_fp* fp);
const char* fhx_fp_last_error(const fhx_fp* fp);
int fhx_fp_load_table(fhx_fp* fp, const char* name_text, const int32_t* name_contig, int32_t n_names, const int64_t* first, int32_t n_contigs,
                      const int32_t* ends, int64_t n_frags);
int fhx_fp_bin_file(fhx_fp* fp, const char* path, int64_t* n_cells, int32_t* why, int64_t* bad_line);
/* lines read, pairs kept, lines dropped for a name, lines dropped as same-fragment, cells */
int fhx_fp_counts(const fhx_fp* fp, int64_t* n_lines, int64_t* n_pairs, int64_t* n_dropped_name, int64_t* n_same_fragment, int64_t* n_cells);
int fhx_fp_stage_seconds(const fhx_fp* fp, double* seconds);       /* FHX_FP_STAGES host clocks */
int fhx_fp_fetch_cells(fhx_fp* fp, int32_t* chr1, int32_t* end1, int32_t* chr2, int32_t* end2, int32_t* count);   /* n_cells each */
/* the columns in HBM (which 0..4 = contig1, end1, contig2, end2, count) and the stream they were written on, for
 * fhx_load_pairs_device; valid until the next fhx_fp_bin_file / fhx_fp_load_table / fhx_fp_destroy */
void* fhx_fp_device_ptr(fhx_fp* fp, int32_t which);
void* fhx_fp_stream(fhx_fp* fp);

/* ---- contact rows in HBM summed onto N-fold coarser loci (csrc/fhx_coarsen.hip; the reference has no script for it, the
 * semantics are this project's: INTEGRATION.md section 16).  One handle per GPU, independent of fhx_ctx.
 * fhx_cz_load_plan gives what the host planned (fithic_amd/coarsen.py): the fine loci laid out by chromosome id - rows
 * first[c] .. first[c + 1] - 1 of fine_mid are the strictly ascending mids of chromosome id c (first[0] = 0, first[n_chr] = n_fine,
 * an id without loci has an empty range) -, group_of[row] = the coarse row of that fine locus, and the coarse loci
 * (coarse_chr, coarse_mid), n_coarse <= n_fine of them.  FHX_ERR_ARG for a plan that is not as described.
 * fhx_cz_coarsen_device takes n rows (chr1, mid1, chr2, mid2, count: int32 columns in HBM) after waiting for `stream`, the
 * producer's; fhx_cz_coarsen_host uploads them first.  Each end is looked up in the fine table, the two coarse rows are ordered
 * g1 <= g2, a row with g1 == g2 is kept (keep_diagonal != 0) or dropped and counted, and the counts of the rows with equal
 * (g1, g2) are summed.  The cells (coarse chr1, mid1, chr2, mid2, sum: int32) stay in HBM in ascending (g1, g2); a cell exists
 * when any row maps to it, a sum of zero included.
 * Anything else is refused with nothing left loaded: *why = one of FHX_CZ_*, *bad_row = the smallest offending 0-based row; for
 * FHX_CZ_SUM, which belongs to no row, *bad_row = g1 << 32 | g2 of the first cell above 2^31 - 1.  Return value:
 * FHX_ERR_UNSUPPORTED. */
#define FHX_CZ_OK 0
#define FHX_CZ_LOCUS 1             /* an end (chr, mid) that is no locus of the fine table */
#define FHX_CZ_COUNT 2             /* a negative count */
#define FHX_CZ_SUM 3               /* the counts of a cell sum to more than 2^31 - 1 */
#define FHX_CZ_INTERNAL 4          /* a device-side consistency check failed */
#define FHX_CZ_STAGES 6            /* upload (host rows), keys, sort, heads + sums, cells: of the last call; then the last plan's upload */
typedef struct fhx_cz fhx_cz;
int fhx_cz_create(int device, fhx_cz** out);
void fhx_cz_destroy(fhx_cz* cz);
const char* fhx_cz_last_error(const fhx_cz* cz);
int fhx_cz_reset(fhx_cz* cz);                                      /* drops the cells and the stage clocks; the plan stays */
int fhx_cz_load_plan(fhx_cz* cz, const int64_t* first, int32_t n_chr, const int32_t* fine_mid, const int32_t* group_of, int64_t n_fine,
                     const int32_t* coarse_chr, const int32_t* coarse_mid, int64_t n_coarse);
int fhx_cz_coarsen_device(fhx_cz* cz, const void* d_chr1, const void* d_mid1, const void* d_chr2, const void* d_mid2, const void* d_count, int64_t n,
                          void* stream, int32_t keep_diagonal, int64_t* n_cells, int32_t* why, int64_t* bad_row);
int fhx_cz_coarsen_host(fhx_cz* cz, const int32_t* chr1, const int32_t* mid1, const int32_t* chr2, const int32_t* mid2, const int32_t* count, int64_t n,
                        int32_t keep_diagonal, int64_t* n_cells, int32_t* why, int64_t* bad_row);
/* rows given, rows dropped as diagonal, cells */
int fhx_cz_counts(const fhx_cz* cz, int64_t* n_rows, int64_t* n_diagonal, int64_t* n_cells);
int fhx_cz_stage_seconds(const fhx_cz* cz, double* seconds);       /* FHX_CZ_STAGES host clocks */
int fhx_cz_fetch_cells(fhx_cz* cz, int32_t* chr1, int32_t* mid1, int32_t* chr2, int32_t* mid2, int32_t* count);   /* n_cells each */
/* the columns in HBM (which 0..4 = chr1, mid1, chr2, mid2, count) and the stream they were written on, for
 * fhx_load_pairs_device; valid until the next fhx_cz_coarsen_* / fhx_cz_reset / fhx_cz_load_plan / fhx_cz_destroy */
void* fhx_cz_device_ptr(fhx_cz* cz, int32_t which);
void* fhx_cz_stream(fhx_cz* cz);

#ifdef __cplusplus
}
#endif
#endif /* FITHIC_MI355X_H */
