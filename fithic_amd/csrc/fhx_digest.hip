// fhx_digest.hip - a FASTA cut with restriction enzymes on MI355X (gfx950): the cut sites of every contig, from which the host
// writes HiC-Pro's fragment bed and the fragments file `fithic -r 0` reads
// (reference: fithic/utils/createFitHiCFragments-nonfixedsize.sh:16, HiC-Pro's digest_genome.py, and :18-33, the loop over its bed).
//
// A coordinate counts sequence bytes only and restarts at every header, and a motif runs across line ends, so nothing here is
// a per-line record.  The text goes through HBM in batches cut at the last newline (fhx_textupload.hpp).  Per batch:
//
//   scan_text<TextModeBytes>, scan_tiles   the newline layer (fhx_textlines.hpp): the line number of every block's first line
//   dg_class       the lines that begin in a block, one per lane, one walk: the grammar (the smallest refused line wins an
//                  atomicMin), and per block the sequence bytes and the header lines
//   scan_tiles x2  S(block) = the sequence bytes before the block's first line, 64 bits; the headers before it
//   dg_walk<COUNT> the same lines in rounds of 256, their sequence bytes and header flags scanned in order: every header's
//                  record (where its name lies, its line, S at the header) at its index, and per block the number of cut sites
//   scan_tiles     where a block's sites go
//   dg_walk<WRITE> every sequence line again: a lane slides a window of 16 four-bit one-hot codes (a c g t = 1 2 4 8, anything
//                  else 0 and so equal to nothing) over its line and up to 15 sequence bytes BEHIND it - line ends skipped, a `>`
//                  after a newline ends the reach, so a window never spans two contigs - and compares it with every motif:
//                  one mask and one compare each.  A hit is contig << 32 | (start + offset), stored where the scan put it: no
//                  atomic, and the order of the buffer is the order of the file.
//
// A window that runs past the end of its batch matches nothing on the device; the host tests those at most 15 start positions
// per batch edge against the bytes of the file (stitch_edge).  The sites of the batches so far stay in one array that grows
// with its contents (DeviceScratch::grow_keep); after the last batch fhx_sort_u64 orders them (several motifs interleave, equal
// sites stay; the handle owns its sorter through fhx_cells.hpp).  Names, their grammar and the duplicate check are the host's: one name per contig.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../include/fithic_mi355x.h"
#include "fhx_cells.hpp"

namespace dgd {

using namespace fhxlines;

constexpr int MAX_MOTIFS = FHX_DG_MAX_MOTIFS;
constexpr int MAX_MOTIF = FHX_DG_MAX_MOTIF;      // bases: one 64-bit window of 4-bit codes
constexpr long long MAX_CONTIG = 2147483647ll;

struct Words {
    unsigned long long first_error;              // smallest (line << 8 | reason)
    unsigned long long seq_bytes, headers, hits; // scan_tiles' totals of the batch
};

struct Motifs {
    unsigned long long pat[MAX_MOTIFS], mask[MAX_MOTIFS];
    int offset[MAX_MOTIFS];
    int n, pad;
};

struct Header {                                  // one per header line, in file order
    unsigned long long S;                        // sequence bytes of the text before it
    long long name_at;                           // offset in the batch of the byte behind `>`
    long long line;                              // 1-based, of the file
    int name_len, pad;
};

__host__ __device__ inline unsigned int code_of(unsigned int c) {
    c |= 0x20u;
    return c == 'a' ? 1u : c == 'c' ? 2u : c == 'g' ? 4u : c == 't' ? 8u : 0u;
}

// what the walks know of a line that dg_class let pass: its bytes up to the newline (or the end of the text), how many of
// them are sequence, whether it is a header
struct Line {
    int raw, n;
    bool header;
};

__device__ inline Line measure(const unsigned char* __restrict__ text, int64_t T, int64_t start) {
    Line L;
    int k = 0;
    for (; k <= MAX_LINE && start + k < T && text[start + k] != '\n'; ++k) {}
    L.raw = k;
    L.header = k > 0 && text[start] == '>';
    const int cr = (k > 0 && text[start + k - 1] == '\r') ? 1 : 0;
    L.n = L.header ? 0 : k - cr;
    return L;
}

// ---- the grammar; sequence bytes and headers per block -------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void dg_class(const unsigned char* __restrict__ text, int64_t T, const unsigned long long* __restrict__ block_off,
                                               int64_t line_base, unsigned int* __restrict__ block_seq, unsigned int* __restrict__ block_hdr,
                                               Words* __restrict__ words) {
    __shared__ unsigned short lstart[LSTART_ENTRIES];
    const BlockLines B = block_lines(text, T, block_off, lstart);
    unsigned int my_seq = 0, my_hdr = 0;
    for (int e = threadIdx.x; e < B.n_lines; e += WG) {
        const int64_t start = B.b0 + lstart[e];
        const bool header = start < T && text[start] == '>';
        int why = 0, n = 0;
        for (int k = 0;; ++k) {
            const int64_t p = start + k;
            const unsigned int c = p < T ? text[p] : '\n';                    // the end of the text ends the line
            if (c == '\n') break;
            if (k >= MAX_LINE) {
                why = FHX_DG_LONG_LINE;
                break;
            }
            if (c == '\r') {
                if (p + 1 >= T || text[p + 1] != '\n') why = FHX_DG_BYTES;
            } else if (c == ' ' || c == '\t') {
                if (!header) why = FHX_DG_BLANK;
            } else if (c < 0x20u || c >= 0x7fu) {
                why = FHX_DG_BYTES;
            } else {
                ++n;
            }
            if (why) break;
        }
        if (why) atomicMin(&words->first_error, error_word(line_base + B.row0 + e + 1, why));
        if (header) ++my_hdr;                                                 // a refused header still has a place among the headers: the host
        else if (!why) my_seq += (unsigned int)n;                             // looks at the names on the lines before the refused one
    }
    unsigned int total;
    fhxscan::block_exclusive_scan(my_seq, &total);                            // every lane of the block arrives here
    if (threadIdx.x == 0) block_seq[blockIdx.x] = total;
    fhxscan::block_exclusive_scan(my_hdr, &total);
    if (threadIdx.x == 0) block_hdr[blockIdx.x] = total;
}

// ---- headers and cut sites -------------------------------------------------------------------------------------------------------
// the codes of up to 15 sequence bytes behind the line that ends at text[p - 1] = '\n' (or at T), first one in the low nibble
__device__ inline unsigned long long reach(const unsigned char* __restrict__ text, int64_t T, int64_t p) {
    unsigned long long ext = 0;
    bool line_start = true;
    for (int got = 0; got < MAX_MOTIF - 1 && p < T; ++p) {
        const unsigned int c = text[p];
        if (line_start && c == '>') break;
        line_start = c == '\n';
        if (c == '\n' || c == '\r') continue;
        ext |= (unsigned long long)code_of(c) << (4 * got);
        ++got;
    }
    return ext;
}

// The sites whose motif starts in the line text[start, start + n): their number; WRITE stores them at out[0, capacity).
template <bool WRITE>
__device__ inline unsigned int line_sites(const unsigned char* __restrict__ text, int64_t T, int64_t start, int n, int raw,
                                          const Motifs* __restrict__ motifs, unsigned long long contig_bits, long long pos0,
                                          unsigned long long* __restrict__ out, int64_t capacity) {
    const unsigned long long ext = reach(text, T, start + raw + 1);
    // code j of the line's stream: its own bytes, then the reach, then nothing
    auto nib = [&](int j) -> unsigned long long {
        if (j < n) return code_of(text[start + j]);
        const int r = j - n;
        return r < MAX_MOTIF - 1 ? (ext >> (4 * r)) & 0xFull : 0ull;
    };
    unsigned long long w = 0;
    for (int j = 0; j < MAX_MOTIF; ++j) w |= nib(j) << (4 * j);
    const int n_motifs = motifs->n;
    unsigned int hits = 0;
    for (int s = 0; s < n; ++s) {
        for (int m = 0; m < n_motifs; ++m) {
            if ((w & motifs->mask[m]) == motifs->pat[m]) {
                if (WRITE && (int64_t)hits < capacity)
                    out[hits] = contig_bits | ((unsigned long long)(pos0 + s + motifs->offset[m]) & 0xFFFFFFFFull);
                ++hits;
            }
        }
        w = (w >> 4) | (nib(s + MAX_MOTIF) << 60);
    }
    return hits;
}

// seq_base, hdr_base: sequence bytes and headers of the earlier batches; carry_S: S at the header in force when the batch
// begins.  COUNT (WRITE = false) fills headers[] and block_hits[]; WRITE stores the sites at hits[hit_off[block] + ...).
template <bool WRITE>
__global__ __launch_bounds__(WG) void dg_walk(const unsigned char* __restrict__ text, int64_t T, const unsigned long long* __restrict__ block_off,
                                              int64_t line_base, const unsigned long long* __restrict__ seq_off,
                                              const unsigned long long* __restrict__ hdr_off, unsigned long long seq_base, long long hdr_base,
                                              unsigned long long carry_S, const Motifs* __restrict__ motifs, Header* __restrict__ headers,
                                              int64_t n_headers, unsigned int* __restrict__ block_hits,
                                              const unsigned long long* __restrict__ hit_off, unsigned long long* __restrict__ hits,
                                              int64_t n_hits) {
    __shared__ unsigned short lstart[LSTART_ENTRIES];
    const BlockLines B = block_lines(text, T, block_off, lstart);
    unsigned long long run_seq = seq_base + seq_off[blockIdx.x];
    long long run_hdr = (long long)hdr_off[blockIdx.x];                       // headers of the batch before the round
    unsigned long long run_hits = WRITE ? hit_off[blockIdx.x] : 0ull;
    for (int base = 0; base < B.n_lines; base += WG) {                        // n_lines is the same for every lane
        const int e = base + (int)threadIdx.x;
        const bool valid = e < B.n_lines;
        const int64_t start = valid ? B.b0 + lstart[e] : 0;
        Line L{0, 0, false};
        if (valid) L = measure(text, T, start);
        unsigned int seq_total, hdr_total, hit_total;
        const unsigned int seq_pre = fhxscan::block_exclusive_scan((unsigned int)L.n, &seq_total);
        const unsigned int hdr_pre = fhxscan::block_exclusive_scan(L.header ? 1u : 0u, &hdr_total);
        const unsigned long long S = run_seq + seq_pre;
        const long long h = run_hdr + hdr_pre;                                // headers of the batch before this line
        if (!WRITE && L.header && h < n_headers) {
            int len = 0;
            for (int k = 1; k < L.raw; ++k, ++len) {
                const unsigned int c = text[start + k];
                if (c == ' ' || c == '\t' || c == '\r') break;
            }
            Header H;
            H.S = S;
            H.name_at = start + 1;
            H.line = line_base + B.row0 + e + 1;
            H.name_len = len;
            H.pad = 0;
            headers[h] = H;
        }
        const long long contig = hdr_base + h - 1;                            // -1: text before the first header belongs to nothing
        // counted in both passes: the scan needs every lane's number before any lane stores
        unsigned int mine = 0;
        if (L.n > 0 && contig >= 0) mine = line_sites<false>(text, T, start, L.n, L.raw, motifs, 0ull, 0ll, nullptr, 0);
        const unsigned int hit_pre = fhxscan::block_exclusive_scan(mine, &hit_total);
        if (WRITE && mine) {
            const unsigned long long at = run_hits + hit_pre;
            const unsigned long long S_header = (h >= 1 && h <= n_headers) ? headers[h - 1].S : carry_S;
            const int64_t room = (int64_t)at < n_hits ? n_hits - (int64_t)at : 0;
            line_sites<true>(text, T, start, L.n, L.raw, motifs, (unsigned long long)contig << 32, (long long)(S - S_header), hits + at, room);
        }
        run_seq += seq_total;
        run_hdr += hdr_total;
        run_hits += hit_total;
    }
    if (!WRITE && threadIdx.x == 0) block_hits[blockIdx.x] = (unsigned int)run_hits;
}

}  // namespace dgd

// ===================================================================================================================
struct fhx_dg : fhx::TextHandle {
    fhx_ctx* sorter = nullptr;
    // the last digested file
    std::vector<std::string> names;
    std::vector<int64_t> lengths;
    unsigned long long* d_sites = nullptr;        // sorted: contig << 32 | position
    int64_t n_sites = 0, n_lines = 0, seq_bytes = 0;
    double seconds[FHX_DG_STAGES] = {0, 0, 0, 0, 0, 0};
};

namespace {

void drop_all(fhx_dg* dg) {
    fhx::dev_free(dg->d_sites);
    dg->n_sites = dg->n_lines = dg->seq_bytes = 0;
    std::vector<std::string>().swap(dg->names);
    std::vector<int64_t>().swap(dg->lengths);
}

// bytes [off, off + len) of the text, or false with the handle's message set
bool read_bytes(fhx_dg* dg, const fhx::TextFile& src, int64_t off, int64_t len, std::vector<char>* out) {
    out->resize((size_t)len);
    int64_t nl;
    if (len > 0)
        if (const int io_errno = src.read(off, len, out->data(), &nl)) {
            (void)fhx::fail(dg, FHX_ERR_ARG, std::string("reading the FASTA file: ") + std::strerror(io_errno));
            return false;
        }
    return true;
}

// The windows that start in the batch [lo, edge) and end behind it: the device saw them cut off.  The last (up to) 15 sequence
// bytes before the edge - they end at a header or where the batch begins: what starts in an earlier batch was stitched at that
// batch's edge - and the first 15 behind it, up to a header; then every motif that lies across the edge.  pos_end: the
// coordinate the first byte behind the edge has.
int stitch_edge(fhx_dg* dg, const fhx::TextFile& src, int64_t lo, int64_t edge, const dgd::Motifs& motifs, const int* motif_len, int64_t contig,
                int64_t pos_end, std::vector<unsigned long long>* found) {
    constexpr int R = dgd::MAX_MOTIF - 1;
    std::vector<char> buf;
    std::vector<unsigned int> tail;                                           // backwards
    bool done = false;
    for (int64_t span = 65536; !done; span *= 4) {
        const int64_t from = std::max(lo, edge - span);
        if (!read_bytes(dg, src, from, edge - from, &buf)) return FHX_ERR_ARG;
        tail.clear();
        int64_t end = (int64_t)buf.size();                                    // buf[end - 1] is a newline: batches are cut behind one
        bool short_of = false;
        while (end > 0 && (int)tail.size() < R) {
            int64_t ls = end - 1;
            while (ls > 0 && buf[(size_t)ls - 1] != '\n') --ls;
            if (ls == 0 && from > lo) {                                       // the line begins before the buffer does
                short_of = true;
                break;
            }
            if (ls < end - 1 && buf[(size_t)ls] == '>') break;                // the contig begins here
            for (int64_t k = end - 2; k >= ls && (int)tail.size() < R; --k)
                if (buf[(size_t)k] != '\r') tail.push_back(dgd::code_of((unsigned char)buf[(size_t)k]));
            end = ls;
        }
        done = !short_of;
    }
    if (tail.empty()) return FHX_OK;
    std::reverse(tail.begin(), tail.end());
    const int t = (int)tail.size();
    std::vector<unsigned int> stream = tail;
    bool line_start = true, ended = false;
    for (int64_t at = edge; !ended && (int)stream.size() < t + R && at < src.size(); at += (int64_t)buf.size()) {
        if (!read_bytes(dg, src, at, std::min<int64_t>(65536, src.size() - at), &buf)) return FHX_ERR_ARG;
        for (size_t k = 0; k < buf.size() && (int)stream.size() < t + R; ++k) {
            const unsigned char c = (unsigned char)buf[k];
            if (line_start && c == '>') {
                ended = true;
                break;
            }
            line_start = c == '\n';
            if (c == '\n' || c == '\r') continue;
            stream.push_back(dgd::code_of(c));
        }
    }
    const int total = (int)stream.size();
    for (int i = 0; i < t; ++i)
        for (int m = 0; m < motifs.n; ++m) {
            const int L = motif_len[m];
            if (i + L <= t || i + L > total) continue;                        // inside the batch: the device has it; or no such window
            bool same = true;
            for (int k = 0; k < L && same; ++k) same = stream[(size_t)(i + k)] == ((motifs.pat[m] >> (4 * k)) & 0xFull);
            if (same) found->push_back(((unsigned long long)contig << 32) | ((unsigned long long)(pos_end - t + i + motifs.offset[m]) & 0xFFFFFFFFull));
        }
    return FHX_OK;
}

// fhx_dg_digest_file behind its argument checks; whatever it returns but FHX_OK, the caller drops everything
int digest_file(fhx_dg* dg, const char* path, const dgd::Motifs& motifs, const int* motif_len, int32_t* why, int64_t* bad_line) {
    using namespace dgd;
    TH_HIP(dg, hipSetDevice(dg->device));
    TH_HIP(dg, hipStreamSynchronize(dg->stream));
    fhx::StageClock clock{dg->seconds};
    fhx::DeviceScratch tmp;
    fhx::TextBatches in;
    if (const int rc = in.open(dg, &tmp, &clock, path, "FASTA", "FHX_DG_BATCH_BYTES", (int64_t)1 << 31)) return rc;
    unsigned int *d_block_seq = nullptr, *d_block_hdr = nullptr, *d_block_hits = nullptr;
    unsigned long long *d_seq_off = nullptr, *d_hdr_off = nullptr, *d_hit_off = nullptr;
    Motifs* d_motifs = nullptr;
    Words* d_words = nullptr;
    Header* d_headers = nullptr;
    int64_t header_capacity = 0;
    unsigned long long* d_hits = nullptr;         // unsorted, in file order, of all batches so far
    int64_t hit_capacity = 0, n_hits = 0;
    TH_HIP(dg, tmp.get_n(&d_block_seq, (size_t)in.max_blocks));
    TH_HIP(dg, tmp.get_n(&d_block_hdr, (size_t)in.max_blocks));
    TH_HIP(dg, tmp.get_n(&d_block_hits, (size_t)in.max_blocks));
    TH_HIP(dg, tmp.get_n(&d_seq_off, (size_t)in.max_blocks));
    TH_HIP(dg, tmp.get_n(&d_hdr_off, (size_t)in.max_blocks));
    TH_HIP(dg, tmp.get_n(&d_hit_off, (size_t)in.max_blocks));
    TH_HIP(dg, tmp.get_n(&d_motifs, 1));
    TH_HIP(dg, tmp.get_n(&d_words, 1));
    TH_HIP(dg, hipMemcpyAsync(d_motifs, &motifs, sizeof(motifs), hipMemcpyHostToDevice, dg->stream));
    TH_HIP(dg, hipStreamSynchronize(dg->stream));
    const fhx::Refusal refuse{dg, why, bad_line};
    const std::string where = std::string(path) + ": ";
    unsigned long long seq_base = 0, carry_S = 0; // sequence bytes so far; S at the header in force
    std::vector<unsigned long long> header_S;     // per contig
    std::vector<int64_t> header_line;
    std::unordered_set<std::string> seen;
    std::vector<unsigned long long> stitched;
    std::vector<Header> headers;
    std::vector<char> name;
    Words words;
    for (; in.more(); in.advance()) {
        std::memset(&words, 0, sizeof(words));
        words.first_error = NO_ERROR;
        TH_HIP(dg, hipMemcpyAsync(d_words, &words, sizeof(words), hipMemcpyHostToDevice, dg->stream));
        if (const int rc = in.next<TextModeBytes>()) return rc;              // its flag is not needed: dg_class names the line
        const unsigned grid = (unsigned)in.n_blocks;
        const unsigned char* text = in.d_text;
        const unsigned long long* block_off = in.d_block_off;
        hipLaunchKernelGGL(dg_class, dim3(grid), dim3(WG), 0, dg->stream, text, in.len, block_off, in.line_base, d_block_seq, d_block_hdr, d_words);
        hipLaunchKernelGGL(fhxscan::scan_tiles, dim3(1), dim3(fhxscan::THREADS), 0, dg->stream, (const unsigned int*)d_block_seq, in.n_blocks, d_seq_off,
                           &d_words->seq_bytes);
        hipLaunchKernelGGL(fhxscan::scan_tiles, dim3(1), dim3(fhxscan::THREADS), 0, dg->stream, (const unsigned int*)d_block_hdr, in.n_blocks, d_hdr_off,
                           &d_words->headers);
        TH_HIP(dg, hipGetLastError());
        TH_HIP(dg, hipMemcpyAsync(&words, d_words, sizeof(words), hipMemcpyDeviceToHost, dg->stream));
        TH_HIP(dg, hipStreamSynchronize(dg->stream));
        clock.mark(2);
        // a refused line does not end the batch yet: a name on a line before it may be refused too, and the smallest line wins
        // (the walk is safe on any bytes; earlier batches hold the smaller line numbers)
        const unsigned long long first_error = words.first_error;
        const int64_t error_at = first_error != NO_ERROR ? error_line(first_error) : INT64_MAX;
        const int64_t n_headers = (int64_t)words.headers;
        const int64_t hdr_base = (int64_t)header_S.size();
        TH_HIP(dg, tmp.grow(&d_headers, &header_capacity, std::max<int64_t>(n_headers, 1)));
        hipLaunchKernelGGL(dg_walk<false>, dim3(grid), dim3(WG), 0, dg->stream, text, in.len, block_off, in.line_base,
                           (const unsigned long long*)d_seq_off, (const unsigned long long*)d_hdr_off, seq_base, (long long)hdr_base, carry_S,
                           (const Motifs*)d_motifs, d_headers, n_headers, d_block_hits, (const unsigned long long*)d_hit_off,
                           (unsigned long long*)nullptr, (int64_t)0);
        hipLaunchKernelGGL(fhxscan::scan_tiles, dim3(1), dim3(fhxscan::THREADS), 0, dg->stream, (const unsigned int*)d_block_hits, in.n_blocks, d_hit_off,
                           &d_words->hits);
        TH_HIP(dg, hipGetLastError());
        TH_HIP(dg, hipMemcpyAsync(&words, d_words, sizeof(words), hipMemcpyDeviceToHost, dg->stream));
        TH_HIP(dg, hipStreamSynchronize(dg->stream));
        const int64_t batch_hits = first_error != NO_ERROR ? 0 : (int64_t)words.hits;
        TH_HIP(dg, tmp.grow_keep(&d_hits, &hit_capacity, n_hits, n_hits + batch_hits, dg->stream));       // the earlier batches' sites are kept
        if (batch_hits > 0) {
            hipLaunchKernelGGL(dg_walk<true>, dim3(grid), dim3(WG), 0, dg->stream, text, in.len, block_off, in.line_base,
                               (const unsigned long long*)d_seq_off, (const unsigned long long*)d_hdr_off, seq_base, (long long)hdr_base, carry_S,
                               (const Motifs*)d_motifs, d_headers, n_headers, (unsigned int*)nullptr, (const unsigned long long*)d_hit_off,
                               d_hits + n_hits, batch_hits);
            TH_HIP(dg, hipGetLastError());
            TH_HIP(dg, hipStreamSynchronize(dg->stream));
        }
        n_hits += batch_hits;
        clock.mark(3);
        // the names, while the host can still say which line they stand on
        headers.resize((size_t)n_headers);
        if (n_headers > 0) TH_HIP(dg, hipMemcpyAsync(headers.data(), d_headers, (size_t)n_headers * sizeof(Header), hipMemcpyDeviceToHost, dg->stream));
        TH_HIP(dg, hipStreamSynchronize(dg->stream));
        for (const Header& H : headers) {
            if (H.line >= error_at) break;
            if (!read_bytes(dg, in.src, in.off + H.name_at, H.name_len, &name)) return FHX_ERR_ARG;
            std::string s(name.begin(), name.end());
            const std::string at = where + "line " + std::to_string(H.line) + ": ";
            if (s.empty()) return refuse(FHX_ERR_UNSUPPORTED, FHX_DG_EMPTY_NAME, H.line, at + "a header without a name");
            if (s.find_first_of("*?[\\") != std::string::npos)
                return refuse(FHX_ERR_UNSUPPORTED, FHX_DG_NAME_CHARS, H.line, at + "a name that holds one of * ? [ \\");
            if (!seen.insert(s).second) return refuse(FHX_ERR_UNSUPPORTED, FHX_DG_DUPLICATE, H.line, at + "the name " + s + " was seen before");
            dg->names.push_back(std::move(s));
            header_S.push_back(H.S);
            header_line.push_back(H.line);
        }
        if (first_error != NO_ERROR) return refuse.word(first_error, FHX_DG_INTERNAL);
        seq_base += words.seq_bytes;
        if (!header_S.empty()) {
            carry_S = header_S.back();
            // the lengths that are final, and the one that is still growing
            for (size_t c = dg->lengths.size(); c < header_S.size(); ++c) {
                const unsigned long long end = c + 1 < header_S.size() ? header_S[c + 1] : seq_base;
                if ((long long)(end - header_S[c]) > MAX_CONTIG)
                    return refuse(FHX_ERR_UNSUPPORTED, FHX_DG_CONTIG_LENGTH, header_line[c],
                                  where + "line " + std::to_string(header_line[c]) + ": a contig of more than 2^31 - 1 bases");
                if (c + 1 < header_S.size()) dg->lengths.push_back((int64_t)(end - header_S[c]));
            }
            if (in.off + in.len < in.src.size())
                if (const int rc = stitch_edge(dg, in.src, in.off, in.off + in.len, motifs, motif_len, (int64_t)header_S.size() - 1,
                                               (int64_t)(seq_base - carry_S), &stitched))
                    return rc;
        }
        clock.mark(5);
    }
    if (header_S.empty()) return refuse(FHX_ERR_UNSUPPORTED, FHX_DG_NO_HEADER, 1, where + "line 1: no header line (`>name`) in the file");
    dg->lengths.push_back((int64_t)(seq_base - header_S.back()));
    dg->seq_bytes = (int64_t)(seq_base - header_S.front());
    dg->n_lines = in.line_base;
    // the sites in order: several motifs interleave and the stitched ones come last
    const int64_t n = n_hits + (int64_t)stitched.size();
    if (n > 0) {
        unsigned long long* d_all = nullptr;
        unsigned int* d_perm = nullptr;
        TH_HIP(dg, tmp.get_n(&d_all, (size_t)n));
        if (n_hits > 0) TH_HIP(dg, hipMemcpyAsync(d_all, d_hits, (size_t)n_hits * sizeof(unsigned long long), hipMemcpyDeviceToDevice, dg->stream));
        if (!stitched.empty())
            TH_HIP(dg, hipMemcpyAsync(d_all + n_hits, stitched.data(), stitched.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, dg->stream));
        TH_HIP(dg, hipStreamSynchronize(dg->stream));                         // the sorter has a stream of its own
        if (d_hits) tmp.drop(d_hits);
        in.close();
        TH_HIP(dg, tmp.get_n(&d_perm, (size_t)n));
        TH_HIP(dg, fhx::dev_malloc(&dg->d_sites, (size_t)n * sizeof(unsigned long long)));
        const int rc = fhx_sort_u64(dg->sorter, d_all, n, dg->d_sites, d_perm);
        if (rc != FHX_OK) return fhx::fail(dg, rc, std::string("sort: ") + fhx_last_error(dg->sorter));
    }
    dg->n_sites = n;
    clock.mark(4);
    if (std::getenv("FHX_TIMING"))
        std::fprintf(stderr, "digest on the device (%s): %lld lines, %lld contigs, %lld bases, %lld sites: read + upload %.6f s; scan %.6f s; "
                     "class %.6f s; sites %.6f s; sort %.6f s; names %.6f s\n", path, (long long)dg->n_lines, (long long)dg->names.size(),
                     (long long)dg->seq_bytes, (long long)dg->n_sites, dg->seconds[0], dg->seconds[1], dg->seconds[2], dg->seconds[3], dg->seconds[4],
                     dg->seconds[5]);
    return FHX_OK;
}

}  // namespace

extern "C" {

int fhx_dg_create(int device, fhx_dg** out) { return fhx::handle_create_with_sorter(device, out); }

void fhx_dg_destroy(fhx_dg* dg) {
    fhx::text_handle_destroy(dg, [&] {
        drop_all(dg);
        fhx::drop_sorter(dg);
    });
}

const char* fhx_dg_last_error(const fhx_dg* dg) { return fhx::handle_last_error(dg); }

int fhx_dg_digest_file(fhx_dg* dg, const char* path, const char* motifs, const int32_t* lengths, const int32_t* offsets, int32_t n_motifs,
                       int32_t* why, int64_t* bad_line) {
    if (!dg || !path || !why || !bad_line) return FHX_ERR_ARG;
    *why = FHX_DG_OK;
    *bad_line = 0;
    if (!motifs || !lengths || !offsets || n_motifs < 1 || n_motifs > FHX_DG_MAX_MOTIFS)
        return fhx::fail(dg, FHX_ERR_ARG, "1 to 64 motifs are expected");
    dgd::Motifs M;
    std::memset(&M, 0, sizeof(M));
    int motif_len[FHX_DG_MAX_MOTIFS];
    for (int m = 0; m < n_motifs; ++m) {
        const int L = lengths[m];
        if (L < 1 || L > FHX_DG_MAX_MOTIF || offsets[m] < 0 || offsets[m] > L)
            return fhx::fail(dg, FHX_ERR_ARG, "a motif has 1 to 16 bases and its cut lies within it");
        for (int k = 0; k < L; ++k) {
            const unsigned long long c = dgd::code_of((unsigned char)motifs[m * FHX_DG_MAX_MOTIF + k]);
            if (!c) return fhx::fail(dg, FHX_ERR_ARG, "a motif holds only the letters a c g t: N comes expanded");
            M.pat[m] |= c << (4 * k);
            M.mask[m] |= 0xFull << (4 * k);
        }
        M.offset[m] = offsets[m];
        motif_len[m] = L;
    }
    M.n = n_motifs;
    for (double& s : dg->seconds) s = 0;
    drop_all(dg);
    const int rc = digest_file(dg, path, M, motif_len, why, bad_line);
    if (rc != FHX_OK) drop_all(dg);                                           // the one exit of a failed digest, whatever failed
    return rc;
}

int fhx_dg_counts(const fhx_dg* dg, int64_t* n_lines, int64_t* n_contigs, int64_t* seq_bytes, int64_t* n_sites) {
    if (!dg) return FHX_ERR_ARG;
    if (n_lines) *n_lines = dg->n_lines;
    if (n_contigs) *n_contigs = (int64_t)dg->names.size();
    if (seq_bytes) *seq_bytes = dg->seq_bytes;
    if (n_sites) *n_sites = dg->n_sites;
    return FHX_OK;
}

const char* fhx_dg_name(const fhx_dg* dg, int64_t contig) {
    return (dg && contig >= 0 && contig < (int64_t)dg->names.size()) ? dg->names[(size_t)contig].c_str() : nullptr;
}

int64_t fhx_dg_contig_length(const fhx_dg* dg, int64_t contig) {
    return (dg && contig >= 0 && contig < (int64_t)dg->lengths.size()) ? dg->lengths[(size_t)contig] : -1;
}

int fhx_dg_fetch_sites(fhx_dg* dg, int32_t* contig, int32_t* position) {
    if (!dg || (dg->n_sites > 0 && (!contig || !position))) return FHX_ERR_ARG;
    if (dg->n_sites == 0) return FHX_OK;
    TH_HIP(dg, hipSetDevice(dg->device));
    fhx::StageClock clock{dg->seconds};
    std::vector<unsigned long long> keys((size_t)dg->n_sites);
    TH_HIP(dg, hipMemcpyAsync(keys.data(), dg->d_sites, keys.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, dg->stream));
    TH_HIP(dg, hipStreamSynchronize(dg->stream));
    for (size_t i = 0; i < keys.size(); ++i) {
        contig[i] = (int32_t)(keys[i] >> 32);
        position[i] = (int32_t)(keys[i] & 0xFFFFFFFFull);
    }
    clock.mark(5);
    return FHX_OK;
}

int fhx_dg_stage_seconds(const fhx_dg* dg, double* seconds) {
    if (!dg || !seconds) return FHX_ERR_ARG;
    for (int k = 0; k < FHX_DG_STAGES; ++k) seconds[k] = dg->seconds[k];
    return FHX_OK;
}

}  // extern "C"
