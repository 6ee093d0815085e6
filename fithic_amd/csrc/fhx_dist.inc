// fhx_dist.inc - sharded runs behind the C ABI (included by fhx_device.hip inside its extern "C" block).
//
// One spline pass over all ranks' rows (SURVEY.md 8e).  What the reference keeps in one process and this file exchanges:
//   * mainDic + the sums of read_Interactions (fithic/fithic.py:434-440): ONE all-reduce(SUM) of
//     [7 sums | one slot per rank for its largest count | sumCC window | row-count window] in HBM, then the summed block
//     goes to every host and every rank runs the same deterministic fit;
//   * the ascending order of benjamini_hochberg_correction (fithic/myStats.py:27-46): sample sort - the 8192-bin key
//     histogram is all-reduced in place (exact early cutoff, k3_cutoff), the local survivors are radix-sorted, regular
//     samples are all-gathered, one workgroup sorts them and picks world-1 splitters, the cut points give the send counts,
//     the count matrix is all-gathered (the one host wait of the BH: buffer sizes and rank offsets), keys travel
//     all-to-all (each GPU sends ~1/world of its keys to each peer: one peer per xGMI link), the received slice is sorted,
//     BH values and their running max are scanned per slice with the lower slices' maxima as carry (all-gather of one
//     double), q travels back all-to-all and is scattered to row order;
//   * the outlier multiset of pass >= 2 (fithic/fithic.py:528-548): all-reduce(SUM) of the distance-index counts.
// Rows whose loci are not on one grid per chromosome (-r 0, or -r N on irregular midpoints) keep mainDic as explicit
// (distance, sum of counts, rows) triples per rank: those are all-gathered (padded to the longest list) and merged by
// distance on every host, the outlier distances of pass >= 2 likewise; when only SOME ranks hold such rows the others
// re-slot their rows the same way first (agreed in the one all-reduce(MAX) that also equalises the histogram lengths).
// Two transports carry the same schedule: RCCL (loaded at run time, collectives enqueued on the context's stream) and
// caller-provided callbacks (stream synchronised around each call).
}  // extern "C"

#include <dlfcn.h>
#include <rccl/rccl.h>
#include <chrono>

namespace fhx {
namespace ingest {      // fhx_ingest.inc (included after this file)
__global__ void ti_rebuild_rows(const int64_t* __restrict__ rows, int64_t n, int64_t n_loaded, const int32_t* __restrict__ loc1,
                                const int32_t* __restrict__ loc2, const int32_t* __restrict__ cnt, const int16_t* __restrict__ slot_chr,
                                const int32_t* __restrict__ slot_mid, const fhx::ChrGrid* __restrict__ grid, int32_t res,
                                int32_t* __restrict__ out, int* __restrict__ bad);
}

constexpr int DIST_MAX_SAMPLES = 8192;                  // world x samples per rank, sorted by one workgroup in LDS
constexpr unsigned long long DIST_SENTINEL = ~0ull;     // sorts after every key (keys are IEEE patterns of p >= 0)

// pack = [inter_count inter_sum intra_all_count intra_all_sum in_range_count in_range_sum n_skipped 0 | max_count of rank r
//         in slot 8 + r | sumCC[a .. a + w) | rows[a .. a + w)]: one SUM all-reduce carries sums, a MAX and both windows
__global__ void kd_pack_stats(const K1Sums* __restrict__ sums, const unsigned long long* __restrict__ hist_cc,
                              const unsigned long long* __restrict__ hist_np, int a, int w, int rank, int world,
                              long long* __restrict__ pack) {
    const int total = 8 + world + 2 * w;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        long long v = 0;
        if (i < 7) {
            v = reinterpret_cast<const long long*>(sums)[i];
        } else if (i >= 8 && i < 8 + world) {
            v = (i - 8 == rank) ? (long long)sums->max_count : 0;
        } else if (i >= 8 + world && i < 8 + world + w) {
            v = (long long)hist_cc[a + (i - 8 - world)];
        } else if (i >= 8 + world + w) {
            v = (long long)hist_np[a + (i - 8 - world - w)];
        }
        pack[i] = v;
    }
}

// s regular samples of this rank's sorted keys (sentinels when it has none)
__global__ void kd_samples(const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ n_ptr, int s,
                           unsigned long long* __restrict__ out) {
    const long long n = (long long)*n_ptr;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < s; j += gridDim.x * blockDim.x) {
        unsigned long long v = DIST_SENTINEL;
        if (n > 0) {
            long long at = ((long long)(j + 1) * n) / (s + 1);
            if (at > n - 1) at = n - 1;
            v = keys[at];
        }
        out[j] = v;
    }
}

// one workgroup: bitonic sort of the gathered samples in LDS, then world-1 splitters at regular positions of the valid ones;
// splitters[world - 1] receives the number of valid samples
__global__ __launch_bounds__(1024) void kd_splitters(const unsigned long long* __restrict__ samples, int total, int world,
                                                     unsigned long long* __restrict__ splitters) {
    __shared__ unsigned long long a[DIST_MAX_SAMPLES];
    __shared__ int n_valid;
    int N = 2;                                                     // the network covers the samples there are, not the capacity
    while (N < total) N <<= 1;
    for (int i = threadIdx.x; i < N; i += 1024) a[i] = i < total ? samples[i] : DIST_SENTINEL;
    if (threadIdx.x == 0) n_valid = 0;
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < N; i += 1024) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long x = a[i], y = a[l];
                    const bool up = (i & k) == 0;
                    if ((x > y) == up) {
                        a[i] = y;
                        a[l] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
    int mine = 0;
    for (int i = threadIdx.x; i < N; i += 1024) mine += a[i] != DIST_SENTINEL;
    if (mine) atomicAdd(&n_valid, mine);
    __syncthreads();
    const int nv = n_valid;
    if ((int)threadIdx.x < world - 1) {
        unsigned long long v = DIST_SENTINEL;
        if (nv > 0) {
            long long pos = ((long long)(threadIdx.x + 1) * nv) / world;
            if (pos > nv - 1) pos = nv - 1;
            v = a[pos];
        }
        splitters[threadIdx.x] = v;
    }
    if (threadIdx.x == 0) splitters[world - 1] = (unsigned long long)nv;
}

// send counts: the local sorted run cut at the splitters (first index with key >= splitter); without valid samples
// nobody holds a key and every count is zero
__global__ void kd_cuts(const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ n_ptr,
                        const unsigned long long* __restrict__ splitters, int world, long long* __restrict__ counts) {
    __shared__ long long cut[65];
    const long long n = (long long)*n_ptr;
    const int r = threadIdx.x;
    if (r < world - 1) {
        const unsigned long long s = splitters[r];
        long long lo = 0, hi = n;
        if (splitters[world - 1] == 0ull) {
            lo = n;
        } else {
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                if (keys[mid] < s)
                    lo = mid + 1;
                else
                    hi = mid;
            }
        }
        cut[r + 1] = lo;
    }
    if (r == 0) {
        cut[0] = 0;
        cut[world] = n;
    }
    __syncthreads();
    if (r < world) counts[r] = cut[r + 1] - cut[r];
}

// The slice a rank receives is `world` sorted runs (every sender's keys between two splitters, in its sorted order): one
// kernel merges them - an element's place is its position in its own run plus, for every other run, the number of elements
// below it (at or below it for runs of lower ranks: ties keep sender order) - instead of six radix passes of three launches.
// off[r] = first element of run r, off[world] = the slice's length; payload = arrival index, as the sort's was.
__global__ void kd_merge_runs(const unsigned long long* __restrict__ keys, const long long* __restrict__ off, int world,
                              unsigned long long* __restrict__ keys_out, unsigned int* __restrict__ arrival_out) {
    const long long m = off[world];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long long)gridDim.x * blockDim.x) {
        int r = 0;
        while (r + 1 < world && i >= off[r + 1]) ++r;                      // (empty runs share their successor's start)
        const unsigned long long k = keys[i];
        long long pos = i - off[r];
        for (int o = 0; o < world; ++o) {
            if (o == r) continue;
            long long lo = off[o], hi = off[o + 1];
            const bool take_equal = o < r;
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                const unsigned long long v = keys[mid];
                if (v < k || (take_equal && v == k))
                    lo = mid + 1;
                else
                    hi = mid;
            }
            pos += lo - off[o];
        }
        keys_out[pos] = k;
        arrival_out[pos] = (unsigned int)i;
    }
}

__global__ void kd_carry(const double* __restrict__ slice_max, int rank, double* __restrict__ carry) {
    double c = 0.0;
    for (int r = 0; r < rank; ++r) c = fmax(c, slice_max[r]);
    *carry = c;
}

struct RcclApi {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*GetVersion)(int*) = nullptr;
    std::string err;
};

// librccl at run time: FHX_RCCL_LIB, else a copy this process already holds (PyTorch ships its own next to the HIP runtime it
// needs), else the system's
static RcclApi* rccl_api() {
    static RcclApi api;
    static bool tried = false;
    if (tried) return api.lib ? &api : nullptr;
    tried = true;
    const char* env = getenv("FHX_RCCL_LIB");
    void* h = nullptr;
    if (env && *env) h = dlopen(env, RTLD_NOW | RTLD_GLOBAL);
    const char* names[] = {"librccl.so", "librccl.so.1"};
    for (int k = 0; k < 2 && !h; ++k) h = dlopen(names[k], RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL);
    for (int k = 1; k >= 0 && !h; --k) h = dlopen(names[k], RTLD_NOW | RTLD_GLOBAL);
    if (!h) {
        api.err = std::string("librccl could not be loaded: ") + (dlerror() ? dlerror() : "?");
        return nullptr;
    }
#define FHX_SYM(field, name)                                           \
    api.field = reinterpret_cast<decltype(api.field)>(dlsym(h, name)); \
    if (!api.field) {                                                  \
        api.err = std::string("librccl lacks ") + name;                \
        return nullptr;                                                \
    }
    FHX_SYM(GetUniqueId, "ncclGetUniqueId")
    FHX_SYM(CommInitRank, "ncclCommInitRank")
    FHX_SYM(CommDestroy, "ncclCommDestroy")
    FHX_SYM(AllReduce, "ncclAllReduce")
    FHX_SYM(AllGather, "ncclAllGather")
    FHX_SYM(Send, "ncclSend")
    FHX_SYM(Recv, "ncclRecv")
    FHX_SYM(GroupStart, "ncclGroupStart")
    FHX_SYM(GroupEnd, "ncclGroupEnd")
    FHX_SYM(GetErrorString, "ncclGetErrorString")
    FHX_SYM(GetVersion, "ncclGetVersion")
#undef FHX_SYM
    api.lib = h;
    return &api;
}

// the rows of fhx_dist_schedule.def: every collective names the one it is
enum DistStep : int {
#define FHX_DIST_STEP(id, kind, size, phase) DS_##id,
#include "fhx_dist_schedule.def"
#undef FHX_DIST_STEP
    DS_COUNT
};
static const char* const kDistStepName[DS_COUNT] = {
#define FHX_DIST_STEP(id, kind, size, phase) #id,
#include "fhx_dist_schedule.def"
#undef FHX_DIST_STEP
};
static const char* const kDistStepKind[DS_COUNT] = {
#define FHX_DIST_STEP(id, kind, size, phase) #kind,
#include "fhx_dist_schedule.def"
#undef FHX_DIST_STEP
};
enum DistKind : int { ALL_REDUCE_SUM = 0, ALL_REDUCE_MAX = 1, ALL_REDUCE_MIN = 2, ALL_GATHER = 3, ALL_TO_ALL_V = 4 };
static const int kDistStepKindId[DS_COUNT] = {
#define FHX_DIST_STEP(id, kind, size, phase) kind,
#include "fhx_dist_schedule.def"
#undef FHX_DIST_STEP
};

struct DistTraceRow {
    int step;
    long long size;                    // int64 elements (all-reduce), bytes per rank (all-gather), 8-byte elements sent (all-to-all)
};

struct DistState {
    bool trace_on = false;             // FHX_DIST_TRACE=1 when the communicator was made
    std::vector<DistTraceRow> trace;
    int rank = 0, world = 1;
    RcclApi* api = nullptr;
    ncclComm_t comm = nullptr;
    fhx_transport cb{};
    bool custom = false;
    int rccl_version = 0;
    GrowBuf<long long> pack, counts, matrix;
    GrowBuf<unsigned long long> samples, all_samples, splitters, xkeys[2], misc;
    GrowBuf<unsigned int> xvals[2];
    GrowBuf<double> q_arrival, q_back, tile_max, slice_max, all_max, carry;
    GrowBuf<unsigned long long> out_hist;
    GrowBuf<long long> run_off;                           // starts of the sorted runs in the received slice (world + 1)
    std::vector<long long> h_run_off;
    GrowBuf<long long> nf_send, nf_recv;                  // -r 0 / off-grid: padded (distance, sum, rows) triples, outlier distance lists
    std::vector<long long> h_pack, h_matrix, h_nf;
    double stage[5] = {0, 0, 0, 0, 0};
};

}  // namespace fhx

namespace {

using fhx::DistState;

#define FHX_NCCL(call)                                                                                              \
    do {                                                                                                            \
        ncclResult_t r_ = (call);                                                                                   \
        if (r_ != ncclSuccess)                                                                                      \
            return fail(ctx, FHX_ERR_HIP, std::string(#call) + ": " + (D->api->GetErrorString ? D->api->GetErrorString(r_) : "rccl error")); \
    } while (0)
#define FHX_CB(call)                                                                                   \
    do {                                                                                               \
        FHX_HIP(hipStreamSynchronize(ctx->stream));                                                    \
        const int r_ = (call);                                                                         \
        if (r_ != 0) return fail(ctx, FHX_ERR_HIP, std::string("transport callback failed: ") + #call); \
    } while (0)

// a collective is about to be issued as step `step` of the schedule: the kind must be the table's.  A wrong label is a bug in this
// file, not a run-time condition - and returning on it would keep THIS rank out of a collective the other ranks are entering
// (the hang the surrounding code avoids everywhere else): the mismatch is remembered (fhx_last_error, stderr once) and the
// collective is issued all the same.  The trace is capped: a caller that never drains it must not grow it for ever.
constexpr size_t DIST_TRACE_MAX_ROWS = 1u << 16;
int dist_note(fhx_ctx* ctx, int step, int kind, long long size) {
    DistState* D = ctx->dist;
    if (step < 0 || step >= fhx::DS_COUNT || fhx::kDistStepKindId[step] != kind) {
        ctx->err = std::string("internal: collective issued as schedule step ") + (step >= 0 && step < fhx::DS_COUNT ? fhx::kDistStepName[step] : "?") +
                   " with another kind than fhx_dist_schedule.def gives it";
        static bool told = false;
        if (!told) std::fprintf(stderr, "fithic_mi355x: %s\n", ctx->err.c_str());
        told = true;
        return FHX_OK;
    }
    if (D->trace_on && D->trace.size() < DIST_TRACE_MAX_ROWS) D->trace.push_back(fhx::DistTraceRow{step, size});
    return FHX_OK;
}

int dist_all_reduce_i64(fhx_ctx* ctx, int step, void* d_buf, int64_t n, int op) {
    DistState* D = ctx->dist;
    if (n <= 0) return FHX_OK;
    {
        const int rc = dist_note(ctx, step, op == 0 ? fhx::ALL_REDUCE_SUM : (op == 1 ? fhx::ALL_REDUCE_MAX : fhx::ALL_REDUCE_MIN), (long long)n);
        if (rc != FHX_OK) return rc;
    }
    if (D->custom) {
        FHX_CB(D->cb.all_reduce_i64(D->cb.user, d_buf, n, op));
        return FHX_OK;
    }
    const ncclRedOp_t rop = op == 0 ? ncclSum : (op == 1 ? ncclMax : ncclMin);
    FHX_NCCL(D->api->AllReduce(d_buf, d_buf, (size_t)n, ncclInt64, rop, D->comm, ctx->stream));
    return FHX_OK;
}

int dist_all_gather(fhx_ctx* ctx, int step, const void* d_send, void* d_recv, int64_t bytes) {
    DistState* D = ctx->dist;
    if (bytes <= 0) return FHX_OK;
    {
        const int rc = dist_note(ctx, step, fhx::ALL_GATHER, (long long)bytes);
        if (rc != FHX_OK) return rc;
    }
    if (D->custom) {
        FHX_CB(D->cb.all_gather(D->cb.user, d_send, d_recv, bytes));
        return FHX_OK;
    }
    FHX_NCCL(D->api->AllGather(d_send, d_recv, (size_t)bytes, ncclChar, D->comm, ctx->stream));
    return FHX_OK;
}

// 8-byte elements
int dist_all_to_all_v(fhx_ctx* ctx, int step, const void* d_send, const int64_t* sc, const int64_t* so, void* d_recv, const int64_t* rc,
                      const int64_t* ro) {
    DistState* D = ctx->dist;
    {
        long long sent = 0;
        for (int r = 0; r < D->world; ++r) sent += sc[r];
        const int rn = dist_note(ctx, step, fhx::ALL_TO_ALL_V, sent);
        if (rn != FHX_OK) return rn;
    }
    if (D->custom) {
        FHX_CB(D->cb.all_to_all_v(D->cb.user, d_send, sc, so, d_recv, rc, ro, 8));
        return FHX_OK;
    }
    FHX_NCCL(D->api->GroupStart());
    // a call that fails inside the group must still close it: the communicator would otherwise take every later call of this
    // process for a member of the open group
    ncclResult_t first_bad = ncclSuccess;
    for (int r = 0; r < D->world && first_bad == ncclSuccess; ++r) {
        if (sc[r] > 0)
            first_bad = D->api->Send(static_cast<const char*>(d_send) + so[r] * 8, (size_t)sc[r], ncclUint64, r, D->comm, ctx->stream);
        if (first_bad == ncclSuccess && rc[r] > 0)
            first_bad = D->api->Recv(static_cast<char*>(d_recv) + ro[r] * 8, (size_t)rc[r], ncclUint64, r, D->comm, ctx->stream);
    }
    const ncclResult_t end = D->api->GroupEnd();
    if (first_bad != ncclSuccess || end != ncclSuccess)
        return fail(ctx, FHX_ERR_HIP, std::string("all-to-all (grouped ncclSend / ncclRecv): ") +
                                          D->api->GetErrorString(first_bad != ncclSuccess ? first_bad : end));
    return FHX_OK;
}

double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// every rank must hold histograms of the same length (the longest chromosome anywhere decides): once per loaded row set.
// The same all-reduce(MAX) carries, in bit 62, whether ANY rank holds rows this schedule does not take (loci off the grid, -r 0:
// ingest decides that per rank, on that rank's rows only): the refusal must be genome-wide, or the ranks that hold regular rows
// would wait in the next collective for one that has already returned.
constexpr long long DIST_NONFIXED_BIT = 1ll << 62;
int dist_agree_n_dist(fhx_ctx* ctx) {
    DistState* D = ctx->dist;
    if (ctx->dist_ndist_agreed) return FHX_OK;
    // The collective runs ONCE per load: its answer is kept, so that a call repeated after a failed growth below (hipMalloc)
    // grows again without a second all-reduce that no other rank would join - and never runs K1 with a short histogram.
    if (ctx->dist_ndist_global < 0) {
        FHX_HIP(D->misc.need(8));
        long long mine = (ctx->nonfixed ? 0 : ctx->n_dist) | (ctx->nonfixed ? DIST_NONFIXED_BIT : 0);
        FHX_HIP(hipMemcpyAsync(D->misc.p, &mine, sizeof(mine), hipMemcpyHostToDevice, ctx->stream));
        int rc = dist_all_reduce_i64(ctx, fhx::DS_NDIST_AGREE, D->misc.p, 1, 1);
        if (rc != FHX_OK) return rc;
        long long answer = 0;
        FHX_HIP(hipMemcpyAsync(&answer, D->misc.p, sizeof(answer), hipMemcpyDeviceToHost, ctx->stream));
        FHX_HIP(hipStreamSynchronize(ctx->stream));
        ctx->dist_ndist_global = answer;
    }
    const long long global = ctx->dist_ndist_global;
    ctx->dist_any_nonfixed = (global & DIST_NONFIXED_BIT) != 0;
    if (ctx->dist_any_nonfixed) {                                  // the caller refuses (or converts), on every rank alike
        ctx->dist_ndist_agreed = true;
        return FHX_OK;
    }
    if (global > ctx->n_dist) {
        unsigned long long* grown[3] = {nullptr, nullptr, nullptr};
        for (auto& g : grown) FHX_HIP(dev_malloc(&g, (size_t)global * sizeof(unsigned long long)));
        FHX_HIP(hipMemsetAsync(grown[2], 0, (size_t)global * sizeof(unsigned long long), ctx->stream));
        FHX_HIP(hipMemcpyAsync(grown[2], ctx->d_out_hist, (size_t)ctx->n_dist * sizeof(unsigned long long), hipMemcpyDeviceToDevice,
                               ctx->stream));
        FHX_HIP(hipStreamSynchronize(ctx->stream));
        dev_free(ctx->d_hist_cc);
        dev_free(ctx->d_hist_np);
        dev_free(ctx->d_out_hist);
        ctx->d_hist_cc = grown[0];
        ctx->d_hist_np = grown[1];
        ctx->d_out_hist = grown[2];
        ctx->n_dist = global;
        ctx->h_out_hist.resize((size_t)global, 0);
    }
    ctx->dist_ndist_agreed = true;
    return FHX_OK;
}

}  // namespace

extern "C" {

int fhx_comm_unique_id(void* id_out, int64_t capacity) {
    if (!id_out || capacity < (int64_t)sizeof(ncclUniqueId)) return FHX_ERR_ARG;
    static_assert(sizeof(ncclUniqueId) <= FHX_UNIQUE_ID_BYTES, "unique id size");
    fhx::RcclApi* api = fhx::rccl_api();
    if (!api) return FHX_ERR_UNSUPPORTED;
    ncclUniqueId id;
    if (api->GetUniqueId(&id) != ncclSuccess) return FHX_ERR_HIP;
    std::memset(id_out, 0, (size_t)capacity);
    std::memcpy(id_out, &id, sizeof(id));
    return FHX_OK;
}

int fhx_comm_destroy(fhx_ctx* ctx) {
    if (!ctx) return FHX_ERR_ARG;
    DistState* D = ctx->dist;
    if (!D) return FHX_OK;
    if (ctx->device >= 0) {
        (void)hipSetDevice(ctx->device);
        if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    }
    if (D->comm && D->api) (void)D->api->CommDestroy(D->comm);
    delete D;                                             // its GrowBufs go with it
    ctx->dist = nullptr;
    return FHX_OK;
}

static int comm_common(fhx_ctx* ctx, int rank, int nranks) {
    if (!ctx) return FHX_ERR_ARG;
    if (ctx->device < 0) return fail(ctx, FHX_ERR_NO_DEVICE, "host-only context");
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(ctx, FHX_ERR_ARG, "bad rank / world size");
    if (nranks > 64) return fail(ctx, FHX_ERR_UNSUPPORTED, "more than 64 ranks");
    (void)fhx_comm_destroy(ctx);
    ctx->dist = new (std::nothrow) DistState();
    if (!ctx->dist) return FHX_ERR_NOMEM;
    ctx->dist->rank = rank;
    ctx->dist->world = nranks;
    const char* tr = getenv("FHX_DIST_TRACE");
    ctx->dist->trace_on = tr && *tr && *tr != '0';
    return FHX_OK;
}

int fhx_comm_init(fhx_ctx* ctx, const void* rccl_unique_id, int rank, int nranks) {
    if (!rccl_unique_id) return FHX_ERR_ARG;
    int rc = comm_common(ctx, rank, nranks);
    if (rc != FHX_OK) return rc;
    DistState* D = ctx->dist;
    D->api = fhx::rccl_api();
    if (!D->api) {
        (void)fhx_comm_destroy(ctx);
        return fail(ctx, FHX_ERR_UNSUPPORTED, "RCCL is not available: librccl.so could not be loaded");
    }
    FHX_HIP(hipSetDevice(ctx->device));
    ncclUniqueId id;
    std::memcpy(&id, rccl_unique_id, sizeof(id));
    const ncclResult_t r = D->api->CommInitRank(&D->comm, nranks, id, rank);
    if (r != ncclSuccess) {
        const std::string msg = std::string("ncclCommInitRank: ") + D->api->GetErrorString(r);
        D->comm = nullptr;
        (void)fhx_comm_destroy(ctx);
        return fail(ctx, FHX_ERR_HIP, msg);
    }
    (void)D->api->GetVersion(&D->rccl_version);
    return FHX_OK;
}

int fhx_comm_init_custom(fhx_ctx* ctx, const fhx_transport* t, int rank, int nranks) {
    if (!t || !t->all_reduce_i64 || !t->all_gather || !t->all_to_all_v) return FHX_ERR_ARG;
    const int rc = comm_common(ctx, rank, nranks);
    if (rc != FHX_OK) return rc;
    ctx->dist->cb = *t;
    ctx->dist->custom = true;
    return FHX_OK;
}

int fhx_comm_info(fhx_ctx* ctx, int* rank, int* nranks, int* rccl_version) {
    if (!ctx) return FHX_ERR_ARG;
    if (!ctx->dist) return fail(ctx, FHX_ERR_ARG, "no communicator: call fhx_comm_init first");
    if (rank) *rank = ctx->dist->rank;
    if (nranks) *nranks = ctx->dist->world;
    if (rccl_version) *rccl_version = ctx->dist->rccl_version;
    return FHX_OK;
}

int fhx_dist_trace(fhx_ctx* ctx, char* buf, int64_t capacity, int64_t* n_bytes, int clear) {
    if (!ctx || !n_bytes || capacity < 0 || (capacity > 0 && !buf)) return FHX_ERR_ARG;
    if (!ctx->dist) return fail(ctx, FHX_ERR_ARG, "no communicator");
    std::string out;
    for (const fhx::DistTraceRow& r : ctx->dist->trace) {
        out += fhx::kDistStepName[r.step];
        out += ' ';
        out += fhx::kDistStepKind[r.step];
        out += ' ';
        out += std::to_string(r.size);
        out += '\n';
    }
    *n_bytes = (int64_t)out.size();
    if (buf && (int64_t)out.size() <= capacity) {
        std::memcpy(buf, out.data(), out.size());
        if (clear) ctx->dist->trace.clear();
    }
    return FHX_OK;
}

int fhx_dist_stage_seconds(fhx_ctx* ctx, double* out5) {
    if (!ctx || !out5) return FHX_ERR_ARG;
    if (!ctx->dist) return fail(ctx, FHX_ERR_ARG, "no communicator");
    for (int k = 0; k < 5; ++k) out5[k] = ctx->dist->stage[k];
    return FHX_OK;
}

int fhx_copy(fhx_ctx* ctx, void* dst, const void* src, int64_t bytes, int kind) {
    if (!ctx || bytes < 0 || kind < 0 || kind > 2 || (bytes > 0 && (!dst || !src))) return FHX_ERR_ARG;
    if (ctx->device < 0) return fail(ctx, FHX_ERR_NO_DEVICE, "host-only context");
    FHX_HIP(hipSetDevice(ctx->device));
    const hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice : (kind == 1 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice);
    if (bytes) FHX_HIP(hipMemcpyAsync(dst, src, (size_t)bytes, k, ctx->stream));
    FHX_HIP(hipStreamSynchronize(ctx->stream));
    return FHX_OK;
}

// entered = this rank may take part in collectives.  Nothing here depends on this rank's OWN rows only: a refusal that one
// rank takes alone leaves the others waiting in the next collective (whether loci are on a grid is agreed over all ranks in
// dist_agree_n_dist, and every rank then follows the same schedule).
static int dist_check(fhx_ctx* ctx) {
    if (!ctx) return FHX_ERR_ARG;
    if (ctx->device < 0) return fail(ctx, FHX_ERR_NO_DEVICE, "host-only context");
    if (!ctx->dist) return fail(ctx, FHX_ERR_ARG, "no communicator: call fhx_comm_init first");
    if (!ctx->d_loc1) return fail(ctx, FHX_ERR_ARG, "no contact rows loaded (an empty shard still loads zero rows)");
    FHX_HIP(hipSetDevice(ctx->device));
    return FHX_OK;
}

// This rank's rows are on a grid but another rank's are not: re-slot them as the -r 0 path does (sorted distinct (chr, mid)
// loci, explicit distances), from the identity columns rebuilt out of the resident rows.  File positions (fhx_set_global_rows)
// survive; everything else is as after a fresh load, which is the state this runs in (first pass of a loaded row set).
static int dist_convert_to_nonfixed(fhx_ctx* ctx) {
    if (ctx->tables_dirty || !ctx->d_slot_chr) {
        const int rc = build_slot_tables(ctx);
        if (rc != FHX_OK) return rc;
    }
    const int64_t n = ctx->n_rows;
    DeviceScratch tmp;
    int32_t* d_cols = nullptr;
    int* d_bad = nullptr;
    FHX_HIP(tmp.get(&d_cols, (size_t)std::max<int64_t>(n, 1) * 5 * sizeof(int32_t)));
    FHX_HIP(tmp.get(&d_bad, sizeof(int)));
    FHX_HIP(hipMemsetAsync(d_bad, 0, sizeof(int), ctx->stream));
    if (n) {
        hipLaunchKernelGGL(fhx::ingest::ti_rebuild_rows, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, (const int64_t*)nullptr, n, n,
                           (const int32_t*)ctx->d_loc1, (const int32_t*)ctx->d_loc2, (const int32_t*)ctx->d_count,
                           (const int16_t*)ctx->d_slot_chr, (const int32_t*)nullptr, (const fhx::ChrGrid*)ctx->d_grid,
                           (int32_t)ctx->prm.resolution, d_cols, d_bad);
        FHX_HIP(hipGetLastError());
    }
    FHX_HIP(hipStreamSynchronize(ctx->stream));
    long long* saved_rows = ctx->d_grow;                           // alloc_row_arrays would free them
    ctx->d_grow = nullptr;
    ctx->offgrid = ctx->nonfixed = true;
    const int rc = ingest_device_rows_nonfixed(ctx, d_cols, d_cols + n, d_cols + 2 * n, d_cols + 3 * n, d_cols + 4 * n, n);
    if (rc != FHX_OK) {
        // the row arrays were freed (and perhaps half re-allocated) on the way: the context holds no rows any more and says so -
        // every later stage call fails with "no contact rows loaded" until the caller loads them again
        dev_free(saved_rows);
        const std::string why = ctx->err;
        dev_free(ctx->d_loc1);
        dev_free(ctx->d_loc2);
        dev_free(ctx->d_count);
        ctx->n_rows = 0;
        ctx->offgrid = false;
        ctx->nonfixed = ctx->have_params && ctx->prm.resolution == 0;
        ctx->have_stats = ctx->have_fit = ctx->have_p = ctx->have_q = false;
        return fail(ctx, rc, "re-slotting this rank's rows for a run with off-grid loci failed (" + why + "); the contact rows must be loaded again");
    }
    ctx->d_grow = saved_rows;
    ctx->dist_ndist_agreed = true;                                 // the reload reset the verdict: it stands
    ctx->dist_any_nonfixed = true;
    return FHX_OK;
}

// all-gather of one variable-length int64 list per rank: h_lists[r] on every host.  `width` values per entry (triples: 3).
static int dist_gather_lists(fhx_ctx* ctx, const long long* h_mine, int64_t n_mine, int width, std::vector<std::vector<long long>>& h_lists) {
    DistState* D = ctx->dist;
    const int world = D->world;
    // lengths first (the one thing every rank must know to size the padded exchange)
    FHX_HIP(D->counts.need((size_t)1));
    FHX_HIP(D->matrix.need((size_t)world));
    const long long mine = (long long)n_mine;
    FHX_HIP(hipMemcpyAsync(D->counts.p, &mine, sizeof(mine), hipMemcpyHostToDevice, ctx->stream));
    int rc = dist_all_gather(ctx, fhx::DS_NF_LENGTHS, D->counts.p, D->matrix.p, 8);
    if (rc != FHX_OK) return rc;
    std::vector<long long> lens((size_t)world, 0);
    FHX_HIP(hipMemcpyAsync(lens.data(), D->matrix.p, (size_t)world * 8, hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipStreamSynchronize(ctx->stream));
    long long longest = 0;
    for (long long v : lens) longest = std::max(longest, v);
    h_lists.assign((size_t)world, std::vector<long long>());
    if (longest == 0) return FHX_OK;
    const size_t slot = (size_t)longest * (size_t)width;
    FHX_HIP(D->nf_send.need(slot));
    FHX_HIP(D->nf_recv.need(slot * (size_t)world));
    FHX_HIP(hipMemsetAsync(D->nf_send.p, 0, slot * 8, ctx->stream));
    if (n_mine) FHX_HIP(hipMemcpyAsync(D->nf_send.p, h_mine, (size_t)n_mine * (size_t)width * 8, hipMemcpyHostToDevice, ctx->stream));
    rc = dist_all_gather(ctx, fhx::DS_NF_LISTS, D->nf_send.p, D->nf_recv.p, (int64_t)slot * 8);
    if (rc != FHX_OK) return rc;
    D->h_nf.resize(slot * (size_t)world);
    FHX_HIP(hipMemcpyAsync(D->h_nf.data(), D->nf_recv.p, slot * (size_t)world * 8, hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipStreamSynchronize(ctx->stream));
    for (int r = 0; r < world; ++r)
        h_lists[(size_t)r].assign(D->h_nf.begin() + (size_t)r * slot, D->h_nf.begin() + (size_t)r * slot + (size_t)lens[(size_t)r] * (size_t)width);
    return FHX_OK;
}

// fhx_pass_stats for rows with explicit distances: the local mainDic (sorted distinct distances with their sums) of every rank,
// merged by distance; the seven sums and the largest count ride in front of the list
static int dist_pass_stats_nonfixed(fhx_ctx* ctx, fhx_stats* out, double t_begin) {
    DistState* D = ctx->dist;
    int rc = pass_stats_nonfixed(ctx, nullptr);                    // local: ctx->stats, h_dist_keys / h_hist_cc / h_hist_np
    if (rc != FHX_OK) return rc;
    const fhx_stats mine = ctx->stats;
    const size_t n_runs = ctx->h_dist_keys.size();
    std::vector<long long> send(3 * (n_runs + 3));
    const long long head[9] = {mine.inter_count, mine.inter_sum, mine.intra_all_count, mine.intra_all_sum, mine.in_range_count,
                               mine.in_range_sum, mine.n_skipped, mine.max_count, 0};
    for (int k = 0; k < 9; ++k) send[(size_t)k] = head[k];
    for (size_t i = 0; i < n_runs; ++i) {
        send[9 + 3 * i] = (long long)ctx->h_dist_keys[i];
        send[9 + 3 * i + 1] = (long long)ctx->h_hist_cc[i];
        send[9 + 3 * i + 2] = (long long)ctx->h_hist_np[i];
    }
    std::vector<std::vector<long long>> all;
    rc = dist_gather_lists(ctx, send.data(), (int64_t)n_runs + 3, 3, all);
    if (rc != FHX_OK) return rc;
    struct Triple {
        long long d, cc, np;
    };
    std::vector<Triple> merged;
    fhx_stats& st = ctx->stats;
    st = fhx_stats{};
    st.n_rows = ctx->n_rows;
    for (const auto& L : all) {
        st.inter_count += L[0];
        st.inter_sum += L[1];
        st.intra_all_count += L[2];
        st.intra_all_sum += L[3];
        st.in_range_count += L[4];
        st.in_range_sum += L[5];
        st.n_skipped += L[6];
        st.max_count = std::max<int64_t>(st.max_count, L[7]);
        const size_t before = merged.size();
        for (size_t i = 9; i + 2 < L.size(); i += 3) merged.push_back(Triple{L[i], L[i + 1], L[i + 2]});
        std::inplace_merge(merged.begin(), merged.begin() + (long)before, merged.end(), [](const Triple& a, const Triple& b) { return a.d < b.d; });
    }
    ctx->h_dist_keys.clear();
    ctx->h_hist_cc.clear();
    ctx->h_hist_np.clear();
    for (const Triple& t : merged) {
        if (!ctx->h_dist_keys.empty() && ctx->h_dist_keys.back() == t.d) {
            ctx->h_hist_cc.back() += t.cc;
            ctx->h_hist_np.back() += t.np;
        } else {
            ctx->h_dist_keys.push_back(t.d);
            ctx->h_hist_cc.push_back(t.cc);
            ctx->h_hist_np.push_back(t.np);
        }
    }
    st.n_dist = (int64_t)ctx->h_dist_keys.size();
    ctx->have_stats = true;
    ctx->have_fit = ctx->have_bins = ctx->have_p = ctx->have_q = false;
    if (out) *out = st;
    D->stage[0] = now_s() - t_begin;
    return FHX_OK;
}

// fhx_pass_stats over all ranks' rows: K1, ONE all-reduce, the summed statistics on every host
int fhx_pass_stats_distributed(fhx_ctx* ctx, fhx_stats* out) {
    int rc = dist_check(ctx);
    if (rc != FHX_OK) return rc;
    DistState* D = ctx->dist;
    const int world = D->world, rank = D->rank;
    const double t_begin = now_s();
    rc = dist_agree_n_dist(ctx);
    if (rc != FHX_OK) return rc;
    if (ctx->dist_any_nonfixed) {                                  // explicit distances somewhere: everywhere, then
        if (!ctx->nonfixed) {
            rc = dist_convert_to_nonfixed(ctx);
            if (rc != FHX_OK) return rc;
        }
        return dist_pass_stats_nonfixed(ctx, out, t_begin);
    }

    // ---- K1 + exchange 1 -------------------------------------------------------------------------------------------
    rc = launch_k1(ctx);
    if (rc != FHX_OK) return rc;
    const int64_t res = ctx->prm.resolution;
    const int64_t nd = ctx->n_dist;
    const int64_t a = std::min<int64_t>(std::max<int64_t>(0, ctx->prm.dist_low / res), nd);
    const int64_t b = (ctx->prm.dist_up == INT64_MAX) ? nd : std::max(a, std::min<int64_t>(nd, ctx->prm.dist_up / res + 2));
    const int w = (int)(b - a);
    const int64_t pack_len = 8 + world + 2 * (int64_t)w;
    FHX_HIP(D->pack.need((size_t)pack_len));
    hipLaunchKernelGGL(fhx::kd_pack_stats, dim3(grid_for(pack_len, 256, 64)), dim3(256), 0, ctx->stream, (const K1Sums*)ctx->d_sums,
                       (const unsigned long long*)ctx->d_hist_cc, (const unsigned long long*)ctx->d_hist_np, (int)a, w, rank, world,
                       D->pack.p);
    FHX_HIP(hipGetLastError());
    rc = dist_all_reduce_i64(ctx, fhx::DS_STATS_PACK, D->pack.p, pack_len, 0);
    if (rc != FHX_OK) return rc;
    D->h_pack.resize((size_t)pack_len);
    FHX_HIP(hipMemcpyAsync(D->h_pack.data(), D->pack.p, (size_t)pack_len * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipStreamSynchronize(ctx->stream));                    // host wait 1: the fit needs the summed statistics
    fhx::fold_kernel_events(ctx);
    {
        const long long* P = D->h_pack.data();
        fhx_stats& st = ctx->stats;
        st.n_rows = ctx->n_rows;
        st.inter_count = P[0];
        st.inter_sum = P[1];
        st.intra_all_count = P[2];
        st.intra_all_sum = P[3];
        st.in_range_count = P[4];
        st.in_range_sum = P[5];
        st.n_skipped = P[6];
        long long mc = 0;
        for (int r = 0; r < world; ++r) mc = std::max(mc, P[8 + r]);
        st.max_count = mc;
        st.n_dist = nd;
        ctx->h_hist_cc.assign((size_t)nd, 0);
        ctx->h_hist_np.assign((size_t)nd, 0);
        for (int i = 0; i < w; ++i) {
            ctx->h_hist_cc[(size_t)a + i] = P[8 + world + i];
            ctx->h_hist_np[(size_t)a + i] = P[8 + world + w + i];
        }
        ctx->have_stats = true;
        ctx->have_fit = ctx->have_bins = ctx->have_p = ctx->have_q = false;
    }
    if (out) *out = ctx->stats;
    D->stage[0] = now_s() - t_begin;
    return FHX_OK;
}

// fhx_bh over all ranks' p-values: sample sort across the ranks, q of the local rows in row order
int fhx_bh_distributed(fhx_ctx* ctx, double n_tests) {
    int rc = dist_check(ctx);
    if (rc != FHX_OK) return rc;
    if (!ctx->have_p) return fail(ctx, FHX_ERR_ARG, "fhx_pvalues must run first");
    if (!std::isfinite(n_tests)) return fail(ctx, FHX_ERR_ARG, "number of tests must be finite");
    DistState* D = ctx->dist;
    const int world = D->world, rank = D->rank;
    double t_mark = now_s();
    // ---- exchange 2: global Benjamini-Hochberg ---------------------------------------------------------------------
    before_rerecord(ctx, 2);
    FHX_HIP(hipEventRecord(ctx->ev[4], ctx->stream));
    rc = fill_top_hist(ctx);
    if (rc != FHX_OK) return rc;
    rc = dist_all_reduce_i64(ctx, fhx::DS_TOP_HIST, ctx->d_top_hist, TOP_BINS, 0);
    if (rc != FHX_OK) return rc;
    launch_k3_cutoff(ctx, ctx->d_top_hist, n_tests, &ctx->d_words->bh_cutoff, nullptr, ~0ull, nullptr, CutoffToHost{});
    rc = fhx_bh_local_sort(ctx);                                   // survivors of this rank, sorted: keys + rows; count in bh_kept
    if (rc != FHX_OK) return rc;
    const unsigned long long* d_n = &ctx->d_words->bh_kept;
    const unsigned long long* keys = ctx->d_keys[ctx->sorted_buf];
    // regular samples per rank: 128 cut every slice to within 1/128 of its even share, and the one-workgroup sort of all
    // ranks' samples is 8x shorter than with 1024 (it was 0.1 ms of every pass)
    const int s = std::max(1, std::min(128, fhx::DIST_MAX_SAMPLES / world));
    FHX_HIP(D->samples.need((size_t)s));
    FHX_HIP(D->all_samples.need((size_t)s * world));
    FHX_HIP(D->splitters.need((size_t)world + 1));
    FHX_HIP(D->counts.need((size_t)world));
    FHX_HIP(D->matrix.need((size_t)world * world));
    hipLaunchKernelGGL(fhx::kd_samples, dim3(4), dim3(256), 0, ctx->stream, keys, d_n, s, D->samples.p);
    FHX_HIP(hipGetLastError());
    rc = dist_all_gather(ctx, fhx::DS_SAMPLES, D->samples.p, D->all_samples.p, (int64_t)s * 8);
    if (rc != FHX_OK) return rc;
    hipLaunchKernelGGL(fhx::kd_splitters, dim3(1), dim3(1024), 0, ctx->stream, (const unsigned long long*)D->all_samples.p, s * world,
                       world, D->splitters.p);
    hipLaunchKernelGGL(fhx::kd_cuts, dim3(1), dim3(64), 0, ctx->stream, keys, d_n, (const unsigned long long*)D->splitters.p, world,
                       D->counts.p);
    FHX_HIP(hipGetLastError());
    rc = dist_all_gather(ctx, fhx::DS_COUNT_MATRIX, D->counts.p, D->matrix.p, (int64_t)world * 8);
    if (rc != FHX_OK) return rc;
    D->h_matrix.resize((size_t)world * world);
    FHX_HIP(hipMemcpyAsync(D->h_matrix.data(), D->matrix.p, (size_t)world * world * sizeof(long long), hipMemcpyDeviceToHost,
                           ctx->stream));
    FHX_HIP(hipStreamSynchronize(ctx->stream));                    // host wait 2: buffer sizes and rank offsets
    std::vector<int64_t> sc(world), so(world), rcnt(world), ro(world);
    int64_t n_local = 0, m = 0, rank0 = 0;
    for (int r = 0; r < world; ++r) {
        sc[r] = D->h_matrix[(size_t)rank * world + r];
        so[r] = n_local;
        n_local += sc[r];
        rcnt[r] = D->h_matrix[(size_t)r * world + rank];
        ro[r] = m;
        m += rcnt[r];
    }
    for (int dst = 0; dst < rank; ++dst)
        for (int src = 0; src < world; ++src) rank0 += D->h_matrix[(size_t)src * world + dst];
    ctx->n_sorted = n_local;
    D->stage[3] = now_s() - t_mark;
    t_mark = now_s();
    const size_t mcap = (size_t)std::max<int64_t>(m, 1);
    for (int k = 0; k < 2; ++k) {
        FHX_HIP(D->xkeys[k].need(mcap));
        FHX_HIP(D->xvals[k].need(mcap));
    }
    FHX_HIP(D->q_arrival.need(mcap));
    FHX_HIP(D->q_back.need((size_t)std::max<int64_t>(n_local, 1)));
    FHX_HIP(D->slice_max.need(1));
    FHX_HIP(D->all_max.need((size_t)world));
    FHX_HIP(D->carry.need(1));
    const int tiles = (int)std::max<int64_t>(1, (m + BH_TILE - 1) / BH_TILE);
    FHX_HIP(D->tile_max.need((size_t)tiles + 1));
    // keys to the owners of their slice of the global order
    rc = dist_all_to_all_v(ctx, fhx::DS_KEYS, keys, sc.data(), so.data(), D->xkeys[0].p, rcnt.data(), ro.data());
    if (rc != FHX_OK) return rc;
    int buf = 0;
    if (m > 0) {
        // the received runs are sorted: merge them (one launch)
        D->h_run_off.assign((size_t)world + 1, 0);
        for (int r = 0; r < world; ++r) D->h_run_off[(size_t)r] = (long long)ro[(size_t)r];
        D->h_run_off[(size_t)world] = (long long)m;
        FHX_HIP(D->run_off.need((size_t)world + 1));
        FHX_HIP(hipMemcpyAsync(D->run_off.p, D->h_run_off.data(), ((size_t)world + 1) * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(fhx::kd_merge_runs, dim3(grid_for(m, 256, 2048)), dim3(256), 0, ctx->stream, (const unsigned long long*)D->xkeys[0].p,
                           (const long long*)D->run_off.p, world, D->xkeys[1].p, D->xvals[1].p);
        FHX_HIP(hipGetLastError());
        buf = 1;
        launch_bh_tile_max(ctx, tiles, (const unsigned long long*)D->xkeys[buf].p, (const unsigned long long*)nullptr, m, n_tests, (double)rank0,
                           D->tile_max.p);
        launch_bh_scan_tiles(ctx, D->tile_max.p, (const unsigned long long*)nullptr, m, 0.0, D->slice_max.p, -1, nullptr);
    } else {
        FHX_HIP(hipMemsetAsync(D->slice_max.p, 0, sizeof(double), ctx->stream));
    }
    FHX_HIP(hipGetLastError());
    rc = dist_all_gather(ctx, fhx::DS_SLICE_MAX, D->slice_max.p, D->all_max.p, 8);
    if (rc != FHX_OK) return rc;
    hipLaunchKernelGGL(fhx::kd_carry, dim3(1), dim3(1), 0, ctx->stream, (const double*)D->all_max.p, rank, D->carry.p);
    if (m > 0)                                                     // q in ARRIVAL order: the sort's payload is the arrival index
        launch_bh_apply(ctx, tiles, (const unsigned long long*)D->xkeys[buf].p, (const unsigned int*)D->xvals[buf].p,
                        (const unsigned long long*)nullptr, m, n_tests, (double)rank0, (const double*)D->tile_max.p, (const double*)D->carry.p,
                        D->q_arrival.p, nullptr, nullptr);
    FHX_HIP(hipGetLastError());
    rc = dist_all_to_all_v(ctx, fhx::DS_Q_BACK, D->q_arrival.p, rcnt.data(), ro.data(), D->q_back.p, sc.data(), so.data());
    if (rc != FHX_OK) return rc;
    if (n_local > 0)
        launch_scatter_q(ctx, n_local, (const unsigned int*)ctx->d_vals[ctx->sorted_buf], (const double*)D->q_back.p, d_n, ctx->d_q);
    FHX_HIP(hipGetLastError());
    FHX_HIP(hipEventRecord(ctx->ev[5], ctx->stream));
    ctx->ev_valid[2] = true;
    ctx->ev_folded[2] = false;
    ctx->have_q = true;
    D->stage[4] = now_s() - t_mark;
    return FHX_OK;
}

int fhx_run_pass_distributed(fhx_ctx* ctx, fhx_fit_info* out) {
    int rc = fhx_pass_stats_distributed(ctx, nullptr);
    if (rc != FHX_OK) return rc;
    DistState* D = ctx->dist;
    double t_mark = now_s();
    fhx_fit_info info{};
    rc = fhx_fit(ctx, &info);
    if (rc != FHX_OK) return rc;
    if (out) *out = info;
    D->stage[1] = now_s() - t_mark;
    t_mark = now_s();
    rc = fhx_pvalues(ctx);
    if (rc != FHX_OK) return rc;
    D->stage[2] = now_s() - t_mark;
    return fhx_bh_distributed(ctx, info.bh_total_tests);
}

int fhx_next_pass_distributed(fhx_ctx* ctx, int64_t* n_outliers_total) {
    if (!ctx) return FHX_ERR_ARG;
    DistState* D = ctx->dist;
    if (!D) return fail(ctx, FHX_ERR_ARG, "no communicator: call fhx_comm_init first");
    int64_t local_total = 0;
    int rc = fhx_next_pass(ctx, &local_total);                     // local fold: skip mask, local multiset (device + host copy)
    if (rc != FHX_OK) return rc;
    if (ctx->nonfixed) {
        // explicit distances: every rank's cumulative outlier distance list (ascending), its outlier total and its first
        // duplicated outlier line travel as one list; the merged multiset is what the next pass's binning subtracts
        std::vector<long long> send(2 + ctx->h_outlier_dists.size());
        send[0] = (long long)local_total;
        send[1] = (long long)std::min<int64_t>(ctx->skip_limit, (int64_t)1 << 62);
        std::copy(ctx->h_outlier_dists.begin(), ctx->h_outlier_dists.end(), send.begin() + 2);
        std::vector<std::vector<long long>> all;
        rc = dist_gather_lists(ctx, send.data(), (int64_t)send.size(), 1, all);
        if (rc != FHX_OK) return rc;
        long long total = 0, lim = (long long)1 << 62;
        ctx->h_outlier_dists_global.clear();
        for (const auto& L : all) {
            total += L[0];
            lim = std::min(lim, L[1]);
            const size_t before = ctx->h_outlier_dists_global.size();
            ctx->h_outlier_dists_global.insert(ctx->h_outlier_dists_global.end(), L.begin() + 2, L.end());
            std::inplace_merge(ctx->h_outlier_dists_global.begin(), ctx->h_outlier_dists_global.begin() + (long)before,
                               ctx->h_outlier_dists_global.end());
        }
        ctx->outlier_dists_are_global = true;
        ctx->skip_limit = lim >= ((long long)1 << 62) ? INT64_MAX : (int64_t)lim;
        if (n_outliers_total) *n_outliers_total = (int64_t)total;
        return FHX_OK;
    }
    // genome-wide multiset: reduce a COPY (the device array stays this rank's own cumulative counts)
    const int64_t nd = ctx->n_dist;
    FHX_HIP(D->out_hist.need((size_t)nd + 2));
    FHX_HIP(hipMemcpyAsync(D->out_hist.p, ctx->d_out_hist, (size_t)nd * sizeof(unsigned long long), hipMemcpyDeviceToDevice, ctx->stream));
    const long long tail[1] = {(long long)local_total};
    FHX_HIP(hipMemcpyAsync(D->out_hist.p + nd, tail, sizeof(tail), hipMemcpyHostToDevice, ctx->stream));
    rc = dist_all_reduce_i64(ctx, fhx::DS_OUTLIER_HIST, D->out_hist.p, nd + 1, 0);
    if (rc != FHX_OK) return rc;
    // first duplicated outlier LINE of the whole file (-p >= 3, SURVEY A17): min over ranks, in file positions
    const long long lim = (long long)std::min<int64_t>(ctx->skip_limit, (int64_t)1 << 62);
    FHX_HIP(hipMemcpyAsync(D->out_hist.p + nd + 1, &lim, sizeof(lim), hipMemcpyHostToDevice, ctx->stream));
    rc = dist_all_reduce_i64(ctx, fhx::DS_SKIP_LIMIT, D->out_hist.p + nd + 1, 1, 2);
    if (rc != FHX_OK) return rc;
    ctx->h_out_hist.assign((size_t)nd, 0);
    long long back[2] = {0, 0};
    FHX_HIP(hipMemcpyAsync(ctx->h_out_hist.data(), D->out_hist.p, (size_t)nd * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipMemcpyAsync(back, D->out_hist.p + nd, sizeof(back), hipMemcpyDeviceToHost, ctx->stream));
    FHX_HIP(hipStreamSynchronize(ctx->stream));
    ctx->skip_limit = back[1] >= ((long long)1 << 62) ? INT64_MAX : (int64_t)back[1];
    if (n_outliers_total) *n_outliers_total = (int64_t)back[0];
    return FHX_OK;
}
