// fhx_emitrow.hpp - one row of the significances file as text: the columns a row is made from (Cols), who the row is, whether the
// reference's output loop prints it, and its characters.  Shared by the device writer (fhx_emit.inc: em_format) and the views
// taken from a pass's resident columns (fhx_sigresident.hip: sr_decide, sr_measure, sr_format and the track's kernels), so that a
// kept row's text is the writer's.
#pragma once
#include "fhx_ctx.hpp"
#include "fhx_fmt.hpp"

namespace fhx::emit {

constexpr int ROW_STRIDE = 192;                 // bytes reserved per row in HBM (longer rows -> the host writer takes over): two 24-byte
                                                // names, 9-digit midpoints and three-digit exponents everywhere are 154

struct Cols {
    const int32_t *chr1, *mid1, *chr2, *mid2, *count;     // chr1 == nullptr: the identity columns are rebuilt from the resident rows
    const int32_t *loc1, *loc2;                           // slots as ingest stored them (loc2 complemented for inter rows)
    const int16_t* slot_chr;
    const int32_t* slot_mid;                              // -r 0 / off-grid: midpoint per slot; nullptr on the fixed grid
    const fhx::ChrGrid* grid;
    int32_t res;
    const double *p, *q, *b1, *b2, *expcc;
    const char* names;                          // concatenated chromosome names
    const int32_t* name_off;                    // n_names + 1 offsets
    int32_t n_names;
    int64_t n_rows;
    int32_t mode;
    int64_t dist_low, dist_up;
};

// Every loaded row of the context: identity rebuilt from the resident slots, p and q resident, the biases and ExpCC absent.  A
// caller with other rows (the kept ones, a batch of the writer) or its own columns assigns those members by name.
static inline Cols resident_cols(const fhx_ctx* ctx, const char* d_names, const int32_t* d_name_off, int32_t n_names) {
    Cols C;
    C.chr1 = C.mid1 = C.chr2 = C.mid2 = nullptr;
    C.count = ctx->d_count;
    C.loc1 = ctx->d_loc1;
    C.loc2 = ctx->d_loc2;
    C.slot_chr = ctx->d_slot_chr;
    C.slot_mid = ctx->nonfixed ? ctx->d_slot_mid : nullptr;
    C.grid = ctx->d_grid;
    C.res = (int32_t)ctx->prm.resolution;
    C.p = ctx->d_p;
    C.q = ctx->d_q;
    C.b1 = C.b2 = C.expcc = nullptr;
    C.names = d_names;
    C.name_off = d_name_off;
    C.n_names = n_names;
    C.n_rows = ctx->n_rows;
    C.mode = ctx->prm.mode;
    C.dist_low = ctx->prm.dist_low;
    C.dist_up = ctx->prm.dist_up;
    return C;
}

struct RowId {
    int c1, c2, m1, m2;
};

__device__ __forceinline__ RowId row_identity(const Cols& C, int64_t r) {
    RowId id;
    if (C.chr1) {
        id.c1 = C.chr1[r];
        id.c2 = C.chr2[r];
        id.m1 = C.mid1[r];
        id.m2 = C.mid2[r];
    } else {                                           // invert ingest (k0_slots / nf_finish_rows)
        const int s1 = C.loc1[r], l2 = C.loc2[r], s2 = l2 < 0 ? ~l2 : l2;
        id.c1 = C.slot_chr[s1];
        id.c2 = C.slot_chr[s2];
        id.m1 = C.slot_mid ? C.slot_mid[s1] : (s1 - C.grid[id.c1].base) * C.res + C.grid[id.c1].off;
        id.m2 = C.slot_mid ? C.slot_mid[s2] : (s2 - C.grid[id.c2].base) * C.res + C.grid[id.c2].off;
    }
    return id;
}

__device__ __forceinline__ bool row_emitted(const Cols& C, const RowId& id) {
    if (id.c1 != id.c2) return C.mode == FHX_MODE_ALL || C.mode == FHX_MODE_INTER_ONLY;                       // fithic.py:1197
    long long d = (long long)id.m1 - (long long)id.m2;
    d = d < 0 ? -d : d;
    return (C.mode == FHX_MODE_ALL || C.mode == FHX_MODE_INTRA_ONLY) && d >= C.dist_low && d <= C.dist_up;   // :1205-1207
}

// the row's text with its newline into buf (288 bytes); its length, or 0 for a row the formatter does not cover
__device__ __forceinline__ int row_text(const Cols& C, int64_t r, const RowId& id, char* buf) {
    const int c1 = id.c1, c2 = id.c2;
    bool ok = c1 >= 0 && c1 < C.n_names && c2 >= 0 && c2 < C.n_names;
    int n = 0;
    if (ok) {
        const int a0 = C.name_off[c1], a1 = C.name_off[c1 + 1], b0 = C.name_off[c2], b1 = C.name_off[c2 + 1];
        ok = (a1 - a0) <= 24 && (b1 - b0) <= 24;
        if (ok) {
            for (int k = a0; k < a1; ++k) buf[n++] = C.names[k];
            buf[n++] = '\t';
            n += fmt::put_i64(buf + n, id.m1);
            buf[n++] = '\t';
            for (int k = b0; k < b1; ++k) buf[n++] = C.names[k];
            buf[n++] = '\t';
            n += fmt::put_i64(buf + n, id.m2);
            buf[n++] = '\t';
            n += fmt::put_i64(buf + n, C.count[r]);
            buf[n++] = '\t';
            const double vals[4] = {C.p[r], C.q[r], C.b1[r], C.b2[r]};
            for (int k = 0; k < 4 && ok; ++k) {
                const int w = fmt::fmt_e6(vals[k], buf + n);
                ok = w > 0;
                n += ok ? w : 0;
                buf[n++] = '\t';
            }
            if (ok) {
                const int w = fmt::fmt_f6(C.expcc[r], buf + n);
                ok = w > 0 && n + w + 1 < ROW_STRIDE;
                n += ok ? w : 0;
                buf[n++] = '\n';
            }
        }
    }
    return (!ok || n >= ROW_STRIDE) ? 0 : n;
}

}  // namespace fhx::emit
