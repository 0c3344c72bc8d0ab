// fastqparse.hip -- FASTQ text parsed on the device: a chunk of text goes in, an index of its
// records comes out, and ranges of records are gathered into prepared batches (hreads.hip) that keep their names.
//
// Replaces FastaFastqGzParser over kseq (common/io/reads/fasta_fastq_gz_parser.hpp:64-80,113-136; ext/include/kseq/
// kseq.h:170-212), restated for the host in host/fastx.hpp, for input in the four-line form every sequencer writes.  kseq is
// a serial state machine; in that form it has no state to carry: record r is lines 4r .. 4r + 3.  The index therefore
// parses under that assumption and VERIFIES it per record (host/ingest.hpp does the same on the host): the verdict is the
// first record for which kseq would not read the four lines as name, sequence, quality -- the caller hands the input to the
// serial reader from that record on (bbk_fastq_input_text_end is a position between records) -- or whose qualities are
// outside the offset's range.  The strict form (tests/fastq_restated.py states it next to the literal state machine):
//   line 4r      begins with '@'; the name is the rest of it (kseq reads it up to the end of the line, kseq.h:182)
//   line 4r + 1  is empty (kseq skips it and finds the '+') or begins with none of '@' '+' '>' (kseq.h:186-188)
//   line 4r + 2  begins with '+'
//   line 4r + 3  is as long as line 4r + 1; a shorter one makes kseq read on (a multi-line record), a longer one ends its
//                stream (kseq.h:208-212)
// after ks_getuntil2's rule: ONE trailing '\r' is dropped from a field that is longer than one byte.
// Kernels:
//   k_fq_count    one wavefront per tile of 1024 bytes, 16 bytes per lane in one load: the line feeds of a lane as a
//                 popcount, of the tile as five ballots (the bits of the lanes' counts)
//   k_fq_lines    the same tiles behind one scan of their counts: the rank of a lane's first line feed from the same five
//                 ballots below the lane, and the start of the line behind every line feed
//   k_fq_records  one wavefront per record: the four lines against the strict form (the same in every lane), the quality
//                 bytes 64 at a time as a ballot; the field starts and lengths, and ONE 64-bit atomicMin of
//                 record << 2 | kind for a record that fails -- the smallest wins whatever the order
//   k_fq_gather   one wavefront per record of a range: bases (a..z upper-cased, kseq.h:193-194), qualities (offset
//                 subtracted) and name, consecutive bytes in consecutive lanes, to positions that come from the scans of
//                 the field lengths -- no atomics, the same bytes on every run
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>

#include "hammer.h"
#include "select.h"

namespace bbk {

constexpr uint32_t kFqLane = 16, kFqTile = 64 * kFqLane;  // bytes of a lane, of a wavefront's tile
constexpr int kFqMaxQvOffset = 162;                       // 93 + offset must fit a byte (readprint.hip)
constexpr uint32_t kFqMaxQual = 93;
constexpr uint64_t kFqNone = ~0ull;
constexpr uint64_t kFqMaxBases = 1ull << 31, kFqMaxName = 1ull << 30, kFqMaxChunk = 1ull << 40;

// The line feeds among text[p, p + 16) as a 16-bit mask; nothing at or beyond n_bytes.  p is a multiple of 16 below
// n_bytes, and the buffer holds 16 bytes more than the text, so the one load stays inside it.
__device__ inline uint32_t fq_lf_mask(const uint8_t *__restrict__ text, uint64_t n_bytes, uint64_t p) {
    const uint4 v = *reinterpret_cast<const uint4 *>(text + p);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) m |= (((w[j >> 2] >> ((j & 3u) << 3)) & 0xFFu) == (uint32_t)'\n' ? 1u : 0u) << j;
    const uint64_t left = n_bytes - p;
    return left >= 16 ? m : m & ((1u << left) - 1u);
}

__global__ __launch_bounds__(256) void k_fq_count(const uint8_t *__restrict__ text, uint64_t n_bytes, uint64_t n_tiles,
                                                 uint64_t *__restrict__ counts) {
    const uint64_t tile = (BBK_GID()) >> 6;
    if (tile >= n_tiles) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t p = tile * kFqTile + (uint64_t)lane * kFqLane;
    const uint32_t c = p < n_bytes ? (uint32_t)__popc(fq_lf_mask(text, n_bytes, p)) : 0u;
    uint32_t below, all;
    wave_sums<5>(c, lane, &below, &all);  // (the lanes' counts run 0..16)
    if (lane == 0) counts[tile] = all;
}

// base: the scanned counts.  ls[j + 1] = one past line feed j; ls[0] = 0; with tail_at != 0 (an unterminated last line)
// ls[tail_at] = n_bytes + 1, so that every line i is text[ls[i], ls[i + 1] - 1).  n_ls: the entries of ls.
__global__ __launch_bounds__(256) void k_fq_lines(const uint8_t *__restrict__ text, uint64_t n_bytes, uint64_t n_tiles,
                                                 const uint64_t *__restrict__ base, uint64_t n_ls, uint64_t tail_at,
                                                 uint64_t *__restrict__ ls) {
    const uint64_t gid = BBK_GID();
    if (gid == 0) {
        ls[0] = 0;
        if (tail_at != 0 && tail_at < n_ls) ls[tail_at] = n_bytes + 1;
    }
    const uint64_t tile = gid >> 6;
    if (tile >= n_tiles) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t p = tile * kFqTile + (uint64_t)lane * kFqLane;
    uint32_t m = p < n_bytes ? fq_lf_mask(text, n_bytes, p) : 0u;
    uint32_t below, all;
    wave_sums<5>((uint32_t)__popc(m), lane, &below, &all);
    uint64_t j = base[tile] + below + 1;
    while (m) {
        const uint32_t b = (uint32_t)__builtin_ctz(m);
        m &= m - 1u;
        if (j < n_ls) ls[j] = p + b + 1;
        ++j;
    }
}

// ks_getuntil2's rule for a field of `len` bytes at `first`
__device__ inline uint64_t fq_strip_cr(const uint8_t *__restrict__ text, uint64_t first, uint64_t len) {
    return len > 1 && text[first + len - 1] == '\r' ? len - 1 : len;
}

// status[0]: the verdict (record << 2 | kind), status[1]: the first record with a field too long for a batch; both ~0 on
// entry.  blen / nlen: the bases and the name bytes of every record (what the scans read).
__global__ __launch_bounds__(256) void k_fq_records(const uint8_t *__restrict__ text, const uint64_t *__restrict__ ls,
                                                   uint64_t records, uint32_t qvoffset, uint64_t *__restrict__ seq0,
                                                   uint64_t *__restrict__ qual0, uint64_t *__restrict__ name0,
                                                   uint64_t *__restrict__ blen, uint64_t *__restrict__ nlen,
                                                   unsigned long long *__restrict__ status) {
    const uint64_t r = (BBK_GID()) >> 6;
    if (r >= records) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t l0 = ls[4 * r], l1 = ls[4 * r + 1], l2 = ls[4 * r + 2], l3 = ls[4 * r + 3], l4 = ls[4 * r + 4];
    const uint64_t hl = l1 - 1 - l0, pl = l3 - 1 - l2;
    const uint64_t sl = fq_strip_cr(text, l1, l2 - 1 - l1), ql = fq_strip_cr(text, l3, l4 - 1 - l3);
    const uint64_t nl = hl ? fq_strip_cr(text, l0 + 1, hl - 1) : 0;
    bool form = hl >= 1 && text[l0] == '@' && pl >= 1 && text[l2] == '+' && sl == ql;
    if (form && l2 - 1 - l1 != 0) {  // (the first byte of the line as kseq sees it: before the rule)
        const uint8_t c = text[l1];
        form = c != '@' && c != '+' && c != '>';
    }
    bool bad = false;
    if (form) {
        for (uint64_t cb = 0; cb < ql; cb += 64u) {
            const uint64_t p = cb + lane;
            bool b = false;
            if (p < ql) {
                const uint32_t c = text[l3 + p];
                b = c < qvoffset || c > qvoffset + kFqMaxQual;
            }
            if (__ballot(b)) {
                bad = true;
                break;
            }
        }
    }
    if (lane != 0) return;
    seq0[r] = l1;
    qual0[r] = l3;
    name0[r] = l0 + 1;
    blen[r] = sl;
    nlen[r] = nl;
    if (!form) atomicMin(&status[0], (unsigned long long)(r << 2 | BBK_FASTQ_FORM));
    else if (bad) atomicMin(&status[0], (unsigned long long)(r << 2 | BBK_FASTQ_QUALITY));
    if (form && (sl >= kFqMaxBases || nl >= kFqMaxName)) atomicMin(&status[1], (unsigned long long)r);
}

// Records [first, first + n) of the index into a batch: boff / noff are the scanned field lengths of all records
__global__ __launch_bounds__(256) void k_fq_gather(const uint8_t *__restrict__ text, const uint64_t *__restrict__ seq0,
                                                  const uint64_t *__restrict__ qual0, const uint64_t *__restrict__ name0,
                                                  const uint64_t *__restrict__ boff, const uint64_t *__restrict__ noff,
                                                  uint64_t first, uint64_t n, uint32_t qvoffset, uint8_t *__restrict__ bases,
                                                  uint8_t *__restrict__ quals, uint64_t *__restrict__ off,
                                                  uint8_t *__restrict__ names, uint64_t *__restrict__ name_off) {
    const uint64_t i = (BBK_GID()) >> 6;
    if (i >= n) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t r = first + i;
    const uint64_t b0 = boff[r] - boff[first], bl = boff[r + 1] - boff[r];
    const uint64_t n0 = noff[r] - noff[first], nl = noff[r + 1] - noff[r];
    const uint64_t s = seq0[r], q = qual0[r], nm = name0[r];
    for (uint64_t p = lane; p < bl; p += 64u) {
        const uint8_t c = text[s + p];
        bases[b0 + p] = c >= 'a' && c <= 'z' ? (uint8_t)(c - 32) : c;
        quals[b0 + p] = (uint8_t)(text[q + p] - qvoffset);
    }
    for (uint64_t p = lane; p < nl; p += 64u) names[n0 + p] = text[nm + p];
    if (lane != 0) return;
    off[i] = b0;
    name_off[i] = n0;
    if (i + 1 == n) {
        off[n] = b0 + bl;
        name_off[n] = n0 + nl;
    }
}

// The first quality character of record r outside the offset's range, as the serial reader's caller meets it
static int fq_offending_byte(const bbk_fastq_input *in, uint64_t r) {
    bbk_ctx *ctx = in->ctx;
    uint64_t l[2];
    d2h_sync(ctx, l, in->ls.as<uint64_t>() + 4 * r + 3, 16);
    raw_vector<uint8_t> q(l[1] - 1 - l[0]);
    if (!q.empty()) d2h_big(ctx, q.data(), in->text.as<uint8_t>() + l[0], q.size());
    size_t len = q.size();
    if (len > 1 && q[len - 1] == '\r') --len;
    for (size_t p = 0; p < len; ++p)
        if ((int)q[p] < in->qvoffset || (int)q[p] > in->qvoffset + (int)kFqMaxQual) return q[p];
    return -1;
}

static std::unique_ptr<bbk_fastq_input> fq_index(bbk_ctx *ctx, const char *h_text, uint64_t n_bytes, int final, int qvoffset) {
    BBK_HIP(hipSetDevice(ctx->device));
    auto in = std::make_unique<bbk_fastq_input>();
    in->ctx = ctx;
    in->n_bytes = n_bytes;
    in->qvoffset = qvoffset;
    in->text.alloc(n_bytes + kFqLane);
    if (n_bytes) BBK_HIP(hipMemcpyAsync(in->text.p, h_text, n_bytes, hipMemcpyHostToDevice, ctx->stream));
    // ---- the line table ----
    const uint64_t n_tiles = (n_bytes + kFqTile - 1) / kFqTile;
    DevBuf counts((n_tiles + 1) * 8);
    uint64_t feeds = 0;
    if (n_tiles) {
        launch_items_timed(ctx, "k_fq_count", k_fq_count, n_tiles * 64, in->text.as<uint8_t>(), n_bytes, n_tiles,
                           counts.as<uint64_t>());
        feeds = exclusive_scan_u64(ctx, counts.as<uint64_t>(), counts.as<uint64_t>(), n_tiles);  // waits: h_text may go
    }
    const bool tail = final && n_bytes && h_text[n_bytes - 1] != '\n';
    in->lines = feeds + (tail ? 1 : 0);
    in->records = in->lines / 4;
    const uint64_t n_ls = in->lines + 1;
    in->ls.alloc(n_ls * 8);
    launch_items_timed(ctx, "k_fq_lines", k_fq_lines, std::max<uint64_t>(n_tiles, 1) * 64, in->text.as<uint8_t>(), n_bytes, n_tiles,
                       counts.as<uint64_t>(), n_ls, tail ? in->lines : 0ull, in->ls.as<uint64_t>());
    // ---- the records ----
    const uint64_t R = in->records;
    in->seq0.alloc(R * 8);
    in->qual0.alloc(R * 8);
    in->name0.alloc(R * 8);
    in->boff.alloc((R + 1) * 8);
    in->noff.alloc((R + 1) * 8);
    in->h_boff.assign(R + 1, 0);
    unsigned long long status[2] = {kFqNone, kFqNone};
    if (R) {
        DevBuf d_status(16);
        BBK_HIP(hipMemsetAsync(d_status.p, 0xFF, 16, ctx->stream));
        launch_items_timed(ctx, "k_fq_records", k_fq_records, R * 64, in->text.as<uint8_t>(), in->ls.as<uint64_t>(), R,
                           (uint32_t)qvoffset, in->seq0.as<uint64_t>(), in->qual0.as<uint64_t>(), in->name0.as<uint64_t>(),
                           in->boff.as<uint64_t>(), in->noff.as<uint64_t>(), d_status.as<unsigned long long>());
        uint64_t totals[2];
        exclusive_scan2_u64(ctx, in->boff.as<uint64_t>(), in->boff.as<uint64_t>(), in->noff.as<uint64_t>(), in->noff.as<uint64_t>(),
                            R, totals);
        d2h_sync(ctx, status, d_status.p, 16);
        d2h_big(ctx, in->h_boff.data(), in->boff.p, (R + 1) * 8);
    } else {
        BBK_HIP(hipMemsetAsync(in->boff.p, 0, 8, ctx->stream));
        BBK_HIP(hipMemsetAsync(in->noff.p, 0, 8, ctx->stream));
        BBK_HIP(hipStreamSynchronize(ctx->stream));
    }
    in->verdict = status[0];
    in->oversize = status[1];
    if (final && in->lines % 4 != 0 && in->verdict == kFqNone) in->verdict = R << 2 | BBK_FASTQ_FORM;  // leftover lines
    in->usable = in->verdict == kFqNone ? R : in->verdict >> 2;
    if (in->verdict != kFqNone && (in->verdict & 3) == BBK_FASTQ_QUALITY) in->verdict_byte = fq_offending_byte(in.get(), in->usable);
    return in;
}

static std::unique_ptr<bbk_hreads> fq_gather(const bbk_fastq_input *in, uint64_t first, uint64_t n, unsigned k, int trim_quality) {
    const char *fn = "bbk_hreads_from_fastq_input";
    bbk_ctx *ctx = in->ctx;
    BBK_REQUIRE(k >= 1 && k <= 32, BBK_ERR_ARG, "%s: k = %u: one-word k-mers only (1 <= k <= 32)", fn, k);
    BBK_REQUIRE(first <= in->usable && n <= in->usable - first, BBK_ERR_ARG,
                "%s: records [%llu, %llu + %llu): the index has %llu records, %llu before its verdict", fn, (unsigned long long)first,
                (unsigned long long)first, (unsigned long long)n, (unsigned long long)in->records, (unsigned long long)in->usable);
    BBK_REQUIRE(in->oversize == kFqNone || in->oversize >= first + n || in->oversize < first, BBK_ERR_ARG,
                "%s: record %llu has 2^31 bases or a name of 2^30 bytes or more", fn, (unsigned long long)in->oversize);
    BBK_HIP(hipSetDevice(ctx->device));
    auto hr = std::make_unique<bbk_hreads>();
    hr->ctx = ctx;
    hr->k = k;
    hr->trim_quality = trim_quality;
    hr->n = n;
    hr->bytes = in->h_boff[first + n] - in->h_boff[first];
    for (uint64_t r = first; r < first + n; ++r) hr->longest = std::max(hr->longest, in->h_boff[r + 1] - in->h_boff[r]);
    BBK_REQUIRE(hr->bytes < (1ull << 40) && n < (1ull << 40), BBK_ERR_ARG, "%s: %llu bases in %llu records: at most 2^40 of either in one batch",
                fn, (unsigned long long)hr->bytes, (unsigned long long)n);
    uint64_t nb[2] = {0, 0};
    d2h_sync(ctx, &nb[0], in->noff.as<uint64_t>() + first, 8);
    d2h_sync(ctx, &nb[1], in->noff.as<uint64_t>() + first + n, 8);
    hr->name_bytes = nb[1] - nb[0];
    hr->has_names = true;
    hr->bases.alloc(hr->bytes);
    hr->quals.alloc(hr->bytes);
    hr->off.alloc((n + 1) * 8);
    hr->names.alloc(hr->name_bytes);
    hr->name_off.alloc((n + 1) * 8);
    if (n)
        launch_items_timed(ctx, "k_fq_gather", k_fq_gather, n * 64, in->text.as<uint8_t>(), in->seq0.as<uint64_t>(),
                           in->qual0.as<uint64_t>(), in->name0.as<uint64_t>(), in->boff.as<uint64_t>(), in->noff.as<uint64_t>(), first,
                           n, (uint32_t)in->qvoffset, hr->bases.as<uint8_t>(), hr->quals.as<uint8_t>(), hr->off.as<uint64_t>(),
                           hr->names.as<uint8_t>(), hr->name_off.as<uint64_t>());
    else {
        BBK_HIP(hipMemsetAsync(hr->off.p, 0, 8, ctx->stream));
        BBK_HIP(hipMemsetAsync(hr->name_off.p, 0, 8, ctx->stream));
    }
    hreads_prepare(fn, "record", hr.get());  // waits: the index may go
    return hr;
}

}  // namespace bbk

using namespace bbk;

extern "C" {

int bbk_fastq_input_from_host(bbk_ctx *ctx, const char *h_text, uint64_t n_bytes, int final, int qvoffset,
                              bbk_fastq_input **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && out && (h_text || n_bytes == 0), BBK_ERR_ARG, "bbk_fastq_input_from_host: NULL argument");
        BBK_REQUIRE(qvoffset >= 0 && qvoffset <= kFqMaxQvOffset, BBK_ERR_ARG,
                    "bbk_fastq_input_from_host: qvoffset %d is outside [0, %d]: a quality of 93 plus the offset must fit a byte", qvoffset,
                    kFqMaxQvOffset);
        BBK_REQUIRE(n_bytes < kFqMaxChunk, BBK_ERR_ARG, "bbk_fastq_input_from_host: a chunk of %llu bytes: fewer than 2^40 are needed",
                    (unsigned long long)n_bytes);
        *out = fq_index(ctx, h_text, n_bytes, final, qvoffset).release();
    });
}

uint64_t bbk_fastq_input_records(const bbk_fastq_input *in) { return in ? in->records : 0; }

int bbk_fastq_input_verdict(const bbk_fastq_input *in, uint64_t *record, int *kind, int *byte) {
    if (!in || in->verdict == kFqNone) return 0;
    if (record) *record = in->verdict >> 2;
    if (kind) *kind = (int)(in->verdict & 3);
    if (byte) *byte = in->verdict_byte;
    return 1;
}

uint64_t bbk_fastq_input_text_end(const bbk_fastq_input *in, uint64_t n) {
    if (!in || n > in->records) return ~0ull;
    if (n == 0) return 0;
    uint64_t end = ~0ull;
    const int rc = guarded([&] {
        BBK_HIP(hipSetDevice(in->ctx->device));
        d2h_sync(in->ctx, &end, in->ls.as<uint64_t>() + 4 * n, 8);
    });
    if (rc != BBK_OK) return ~0ull;
    return std::min(end, in->n_bytes);  // (an unterminated last line ends at n_bytes + 1 in the table)
}

uint64_t bbk_fastq_input_records_within(const bbk_fastq_input *in, uint64_t first, uint64_t max_bases) {
    if (!in || first >= in->usable) return 0;
    const uint64_t *b = in->h_boff.data();
    const uint64_t target = b[first] + std::min<uint64_t>(max_bases, ~(uint64_t)0 - b[first]);
    const uint64_t *hit = std::lower_bound(b + first + 1, b + in->usable + 1, target);
    return hit == b + in->usable + 1 ? in->usable - first : (uint64_t)(hit - b) - first;
}

void bbk_fastq_input_free(bbk_fastq_input *in) { delete in; }

int bbk_hreads_from_fastq_input(const bbk_fastq_input *in, uint64_t first, uint64_t n, unsigned k, int trim_quality,
                                bbk_hreads **out) {
    return guarded([&] {
        BBK_REQUIRE(in && out, BBK_ERR_ARG, "bbk_hreads_from_fastq_input: NULL argument");
        *out = fq_gather(in, first, n, k, trim_quality).release();
    });
}

}  // extern "C"
