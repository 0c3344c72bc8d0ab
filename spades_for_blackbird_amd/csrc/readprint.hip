// readprint.hip -- the last step of BayesHammer's CorrectAllReads on the device: the outcome of
// every corrected read, the route of every read or pair, and the FASTQ text of Read::print.
//
// Replaces the tag rule of ReadCorrector::CorrectOneRead (projects/hammer/read_corrector.cpp:214-242), Read::print
// (common/io/reads/read.hpp:221-236) and the routing of CorrectReadFile / CorrectPairedReadFiles
// (projects/hammer/hammer_tools.cpp:135-137,178-186).  All three are deterministic per read, so the text is EQUAL to the
// reference's, byte for byte and in its order: every record is placed by a scan, never by an atomic.
// Kernels:
//   k_rp_outcome  one wavefront per record of a corrected batch: the positions where the corrected trimmed read differs
//                 from the resident one, 64 at a time as a ballot and its popcount, and the kind of the record's tag
//   k_rp_size     one thread per record: its stream and the bytes of its text, written to the stream's row of a
//                 (streams x records) table whose other rows stay 0 -- ONE scan of that table is the position of every
//                 record in a buffer that holds the streams one after the other, records in (pair, left before right)
//                 order inside each
//   k_rp_write    one wavefront per record: lane j writes bytes j, j + 64, ... of the record, finding the piece a byte
//                 belongs to (name, tag, padding, bases, digits, qualities) from the piece lengths, which are the same in
//                 all lanes -- so the loads of a piece and the stores of the whole record are consecutive bytes in
//                 consecutive lanes, and nothing is indexed per thread
// Streams: one batch gives 0 good (result true), 1 bad; a pair of batches 0 cor-left, 1 cor-right, 2 unpaired, 3 bad-left,
// 4 bad-right.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstring>
#include <memory>

#include "hammer.h"

namespace bbk {

enum : uint32_t { kRpNone = 0, kRpOk = 1, kRpFailed = 2, kRpChanged = 3 };  // the kind of a tag
constexpr int kRpMaxQvOffset = 162;                                          // 93 + offset must fit a byte
constexpr uint64_t kRpMaxName = 1ull << 30;                                  // a record's text stays below 2^32 bytes

#define BBK_RP_OK " BH:ok"
#define BBK_RP_FAILED " BH:failed"
#define BBK_RP_CHANGED " BH:changed:"
#define BBK_RP_LTRIM " ltrim="
#define BBK_RP_RTRIM " rtrim="
constexpr uint32_t kRpOkLen = sizeof(BBK_RP_OK) - 1, kRpFailedLen = sizeof(BBK_RP_FAILED) - 1,
                   kRpChangedLen = sizeof(BBK_RP_CHANGED) - 1, kRpTrimLen = sizeof(BBK_RP_LTRIM) - 1;

__device__ inline uint32_t rp_dec_len(uint32_t v) {
    uint32_t n = 1;
    while (v >= 10) {
        v /= 10;
        ++n;
    }
    return n;
}
// digit d (0: the first) of v, a number of w digits
__device__ inline uint8_t rp_digit(uint32_t v, uint32_t w, uint32_t d) {
    for (uint32_t i = d + 1; i < w; ++i) v /= 10;
    return (uint8_t)('0' + v % 10);
}

// ---- k_rp_outcome -------------------------------------------------------------------------------------------------
// out / orig: the corrected and the resident trimmed reads in the same layout (toff: n + 1).  The tag (:214-242): a read of
// fewer than k bases never reaches CorrectOneRead; a searched read (where != 0) is changed:<n> or failed; an unsearched one
// is ok exactly when its flag is set (solid_len == read_size), and has no tag otherwise.
__global__ __launch_bounds__(256) void k_rp_outcome(const uint8_t *__restrict__ out, const uint8_t *__restrict__ orig,
                                                   const uint64_t *__restrict__ toff, const uint8_t *__restrict__ res,
                                                   const uint8_t *__restrict__ where, uint64_t n, uint32_t k,
                                                   uint32_t *__restrict__ changed, uint8_t *__restrict__ tag) {
    const uint64_t r = (BBK_GID()) >> 6;
    if (r >= n) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t base = toff[r];
    const uint32_t len = (uint32_t)(toff[r + 1] - base);
    uint32_t diff = 0;
    for (uint32_t cb = 0; cb < len; cb += 64u) {
        const uint32_t p = cb + lane;
        diff += (uint32_t)__popcll(__ballot(p < len && out[base + p] != orig[base + p]));
    }
    if (lane != 0) return;
    changed[r] = diff;
    tag[r] = (uint8_t)(len < k ? kRpNone : where[r] ? (diff ? kRpChanged : kRpFailed) : res[r] ? kRpOk : kRpNone);
}

// ---- the text of a record ---------------------------------------------------------------------------------------------
// What one side (a corrected batch with its names) gives the two kernels below
struct RpSide {
    const uint8_t *bases, *quals;  // the corrected trimmed reads; the trimmed qualities, offset subtracted
    const uint64_t *toff, *off;    // n + 1 each: the trimmed layout; the records as parsed
    const uint32_t *trim;          // n x (start, length)
    const uint8_t *res, *tag;
    const uint32_t *changed;
    const uint8_t *names;
    const uint64_t *name_off;  // n + 1
};
__device__ inline RpSide rp_pick(const RpSide &a, const RpSide &b, bool second) {
    RpSide s;
    s.bases = second ? b.bases : a.bases;
    s.quals = second ? b.quals : a.quals;
    s.toff = second ? b.toff : a.toff;
    s.off = second ? b.off : a.off;
    s.trim = second ? b.trim : a.trim;
    s.res = second ? b.res : a.res;
    s.tag = second ? b.tag : a.tag;
    s.changed = second ? b.changed : a.changed;
    s.names = second ? b.names : a.names;
    s.name_off = second ? b.name_off : a.name_off;
    return s;
}

// The pieces of a record's text; the same values in every lane of its wavefront.
//   @<name><tag>\n  N^lt <bases> N^tail \n  +<name><tag>[ ltrim=<lt>][ rtrim=<tail>]\n  badq^lt <quals + offset> badq^tail \n
struct RpRec {
    uint64_t name0, base0;  // the first byte of the name; of the trimmed read
    uint32_t nl, tl, lt, len, tail;
    uint32_t kind, changed, dl_changed, dl_lt, dl_tail;
    __device__ uint32_t name_tag() const { return nl + tl; }
    __device__ uint32_t body() const { return lt + len + tail; }
    __device__ uint32_t plus_line() const {
        return 1u + name_tag() + (lt ? kRpTrimLen + dl_lt : 0u) + (tail ? kRpTrimLen + dl_tail : 0u) + 1u;
    }
    __device__ uint64_t bytes() const { return (uint64_t)(1u + name_tag() + 1u) + (body() + 1u) + plus_line() + (body() + 1u); }
};

// ltrim_ / rtrim_ of Read::trimLeftRight's bookkeeping (read.hpp:99-122): the ends of what is left, or 0 and the record's
// size when nothing is -- then no padding is printed on either side
__device__ inline RpRec rp_rec(const RpSide &s, uint64_t r, bool tags) {
    RpRec g;
    const uint32_t initial = (uint32_t)(s.off[r + 1] - s.off[r]), start = s.trim[2 * r];
    g.len = s.trim[2 * r + 1];
    g.lt = g.len ? start : 0u;
    g.tail = g.len ? initial - (start + g.len) : 0u;
    g.name0 = s.name_off[r];
    g.nl = (uint32_t)(s.name_off[r + 1] - g.name0);
    g.base0 = s.toff[r];
    g.kind = tags ? s.tag[r] : kRpNone;
    g.changed = s.changed[r];
    g.dl_changed = rp_dec_len(g.changed);
    g.dl_lt = rp_dec_len(g.lt);
    g.dl_tail = rp_dec_len(g.tail);
    g.tl = g.kind == kRpOk ? kRpOkLen : g.kind == kRpFailed ? kRpFailedLen : g.kind == kRpChanged ? kRpChangedLen + g.dl_changed : 0u;
    return g;
}

// byte p of <name><tag>
__device__ inline uint8_t rp_name_tag_byte(const RpSide &s, const RpRec &g, uint32_t p) {
    if (p < g.nl) return s.names[g.name0 + p];
    p -= g.nl;
    if (g.kind == kRpOk) return (uint8_t)BBK_RP_OK[p];
    if (g.kind == kRpFailed) return (uint8_t)BBK_RP_FAILED[p];
    return p < kRpChangedLen ? (uint8_t)BBK_RP_CHANGED[p] : rp_digit(g.changed, g.dl_changed, p - kRpChangedLen);
}

// byte p of the record's text
__device__ inline uint8_t rp_byte(const RpSide &s, const RpRec &g, uint32_t p, uint32_t qvoffset) {
    const uint32_t nt = g.name_tag(), body = g.body();
    if (p == 0) return '@';
    p -= 1u;
    if (p < nt) return rp_name_tag_byte(s, g, p);
    p -= nt;
    if (p == 0) return '\n';
    p -= 1u;
    if (p < body) return p >= g.lt && p < g.lt + g.len ? s.bases[g.base0 + (p - g.lt)] : (uint8_t)'N';
    p -= body;
    if (p == 0) return '\n';
    p -= 1u;
    if (p == 0) return '+';
    p -= 1u;
    if (p < nt) return rp_name_tag_byte(s, g, p);
    p -= nt;
    if (g.lt) {
        if (p < kRpTrimLen) return (uint8_t)BBK_RP_LTRIM[p];
        p -= kRpTrimLen;
        if (p < g.dl_lt) return rp_digit(g.lt, g.dl_lt, p);
        p -= g.dl_lt;
    }
    if (g.tail) {
        if (p < kRpTrimLen) return (uint8_t)BBK_RP_RTRIM[p];
        p -= kRpTrimLen;
        if (p < g.dl_tail) return rp_digit(g.tail, g.dl_tail, p);
        p -= g.dl_tail;
    }
    if (p == 0) return '\n';
    p -= 1u;
    if (p < body) return (uint8_t)(p >= g.lt && p < g.lt + g.len ? s.quals[g.base0 + (p - g.lt)] + qvoffset : qvoffset + 2u);
    return '\n';
}

// Item i of n_items: record i of side a, or -- paired -- record i >> 1 of side a (even i) or b (odd i).
// stream[i]; len[stream * n_items + i] = the bytes of the item's text (the table is zero on entry)
__global__ __launch_bounds__(256) void k_rp_size(RpSide a, RpSide b, int paired, int tags, uint64_t n_items,
                                                uint8_t *__restrict__ stream, uint64_t *__restrict__ len) {
    const uint64_t i = BBK_GID();
    if (i >= n_items) return;
    const bool second = paired && (i & 1ull);
    const uint64_t r = paired ? i >> 1 : i;
    const RpSide s = rp_pick(a, b, second);
    uint32_t st;
    if (!paired) {
        st = a.res[r] ? 0u : 1u;  // hammer_tools.cpp:136
    } else {                      // :179-185
        const bool l = a.res[r] != 0, rr = b.res[r] != 0;
        st = l && rr ? (second ? 1u : 0u) : second ? (rr ? 2u : 4u) : (l ? 2u : 3u);
    }
    stream[i] = (uint8_t)st;
    len[(uint64_t)st * n_items + i] = rp_rec(s, r, tags != 0).bytes();
}

// pos: the scanned table of k_rp_size
__global__ __launch_bounds__(256) void k_rp_write(RpSide a, RpSide b, int paired, int tags, uint32_t qvoffset, uint64_t n_items,
                                                 const uint8_t *__restrict__ stream, const uint64_t *__restrict__ pos,
                                                 uint8_t *__restrict__ text) {
    const uint64_t i = (BBK_GID()) >> 6;
    if (i >= n_items) return;
    const uint32_t lane = threadIdx.x & 63;
    const bool second = paired && (i & 1ull);
    const uint64_t r = paired ? i >> 1 : i;
    const RpSide s = rp_pick(a, b, second);
    const RpRec g = rp_rec(s, r, tags != 0);
    uint8_t *d = text + pos[(uint64_t)stream[i] * n_items + i];
    const uint32_t total = (uint32_t)g.bytes();
    for (uint32_t p = lane; p < total; p += 64u) d[p] = rp_byte(s, g, p, qvoffset);
}

void corrected_outcome(bbk_corrected *cr) {
    if (!cr->n) return;
    const bbk_hreads::Trimmed &t = hreads_trimmed(cr->hr);
    launch_items_timed(cr->ctx, "k_rp_outcome", k_rp_outcome, cr->n * 64, cr->out.as<uint8_t>(), t.bases, t.off,
                       cr->res.as<uint8_t>(), cr->where.as<uint8_t>(), cr->n, (uint32_t)cr->k,
                       cr->changed.as<uint32_t>(), cr->tag.as<uint8_t>());
}

// The names of one side, checked and uploaded
struct RpNames {
    DevBuf blob, off;
};
static void rp_upload_names(bbk_ctx *ctx, const char *what, const char *h_names, const uint64_t *h_off, uint64_t n, RpNames &d,
                            raw_vector<uint64_t> &rel) {
    const uint64_t first = h_off[0];
    for (uint64_t r = 0; r < n; ++r) {
        BBK_REQUIRE(h_off[r] <= h_off[r + 1], BBK_ERR_ARG, "bbk_corrected_print: the offsets of %s name %llu descend", what,
                    (unsigned long long)r);
        BBK_REQUIRE(h_off[r + 1] - h_off[r] < kRpMaxName, BBK_ERR_ARG, "bbk_corrected_print: %s name %llu has %llu bytes: fewer than 2^30 are needed",
                    what, (unsigned long long)r, (unsigned long long)(h_off[r + 1] - h_off[r]));
    }
    const uint64_t bytes = h_off[n] - first;
    BBK_REQUIRE(bytes == 0 || h_names, BBK_ERR_ARG, "bbk_corrected_print: NULL argument");
    if (bytes) {
        const void *nl = memchr(h_names + first, '\n', bytes);
        BBK_REQUIRE(!nl, BBK_ERR_ARG, "bbk_corrected_print: a line feed at byte %llu of the %s names: a name is one line",
                    (unsigned long long)((const char *)nl - h_names), what);
    }
    rel.resize(n + 1);
    for (uint64_t r = 0; r <= n; ++r) rel[r] = h_off[r] - first;
    upload(ctx, d.blob, (const uint8_t *)h_names + first, bytes);
    upload(ctx, d.off, rel.data(), n + 1);
}

static RpSide rp_side(const bbk_corrected *cr, const uint8_t *names, const uint64_t *name_off) {
    const bbk_hreads *hr = cr->hr;
    const bbk_hreads::Trimmed &t = hreads_trimmed(hr);
    RpSide s;
    s.bases = cr->out.as<uint8_t>();
    s.quals = t.quals;
    s.toff = t.off;
    s.off = hr->off.as<uint64_t>();
    s.trim = hr->trim.as<uint32_t>();
    s.res = cr->res.as<uint8_t>();
    s.tag = cr->tag.as<uint8_t>();
    s.changed = cr->changed.as<uint32_t>();
    s.names = names;
    s.name_off = name_off;
    return s;
}

// What both print entries check before they look at their names
static void rp_check(const char *fn, const bbk_corrected *left, const bbk_corrected *right, int qvoffset) {
    BBK_REQUIRE(qvoffset >= 0 && qvoffset <= kRpMaxQvOffset, BBK_ERR_ARG,
                "%s: qvoffset %d is outside [0, %d]: a quality of 93 plus the offset must fit a byte", fn, qvoffset, kRpMaxQvOffset);
    if (right) {
        BBK_REQUIRE(right->ctx == left->ctx, BBK_ERR_ARG, "%s: the two batches belong to different contexts", fn);
        BBK_REQUIRE(right->n == left->n, BBK_ERR_ARG, "%s: %llu left and %llu right reads: a pair is one of each", fn,
                    (unsigned long long)left->n, (unsigned long long)right->n);
    }
}

// The text of one or two corrected batches whose names (blob, n + 1 offsets per side) are on the device; waits for the stream
static bbk_fastq_text *rp_text(const char *fn, const bbk_corrected *left, const bbk_corrected *right, const uint8_t *names_l,
                               const uint64_t *name_off_l, const uint8_t *names_r, const uint64_t *name_off_r, int qvoffset,
                               int tags) {
    bbk_ctx *ctx = left->ctx;
    const uint64_t n = left->n, n_items = right ? 2 * n : n;
    const int streams = right ? 5 : 2;
    auto t = std::make_unique<bbk_fastq_text>();
    t->ctx = ctx;
    t->streams = streams;
    if (n_items == 0) {
        t->text.alloc(0);
        BBK_HIP(hipStreamSynchronize(ctx->stream));  // the (empty) uploads
        return t.release();
    }
    const RpSide a = rp_side(left, names_l, name_off_l), b = right ? rp_side(right, names_r, name_off_r) : a;
    const uint64_t cells = (uint64_t)streams * n_items;
    DevBuf stream(n_items), pos((cells + 1) * 8);
    BBK_HIP(hipMemsetAsync(pos.p, 0, cells * 8, ctx->stream));
    launch_items_timed(ctx, "k_rp_size", k_rp_size, n_items, a, b, right ? 1 : 0, tags ? 1 : 0, n_items, stream.as<uint8_t>(),
                       pos.as<uint64_t>());
    const uint64_t total = exclusive_scan_u64(ctx, pos.as<uint64_t>(), pos.as<uint64_t>(), cells);  // waits: uploaded names are in
    for (int s = 1; s < streams; ++s)
        BBK_HIP(hipMemcpyAsync(&t->start[s], pos.as<uint64_t>() + (uint64_t)s * n_items, 8, hipMemcpyDeviceToHost, ctx->stream));
    t->start[streams] = total;
    t->text.alloc(total + 16);
    launch_items_timed(ctx, "k_rp_write", k_rp_write, n_items * 64, a, b, right ? 1 : 0, tags ? 1 : 0, (uint32_t)qvoffset, n_items,
                       stream.as<uint8_t>(), pos.as<uint64_t>(), t->text.as<uint8_t>());
    BBK_HIP(hipStreamSynchronize(ctx->stream));  // the stream starts are in; the names and the table go now
    for (int s = 0; s < streams; ++s)
        BBK_REQUIRE(t->start[s] <= t->start[s + 1], BBK_ERR_INTERNAL, "%s: stream %d starts at %llu, the next at %llu", fn, s,
                    (unsigned long long)t->start[s], (unsigned long long)t->start[s + 1]);
    return t.release();
}

}  // namespace bbk

using namespace bbk;

extern "C" {

int bbk_corrected_print(const bbk_corrected *left, const bbk_corrected *right, const char *h_names_l,
                        const uint64_t *h_name_off_l, const char *h_names_r, const uint64_t *h_name_off_r, int qvoffset,
                        int tags, bbk_fastq_text **out) {
    return guarded([&] {
        BBK_REQUIRE(left && out && h_name_off_l && (!right || h_name_off_r), BBK_ERR_ARG, "bbk_corrected_print: NULL argument");
        rp_check("bbk_corrected_print", left, right, qvoffset);
        bbk_ctx *ctx = left->ctx;
        BBK_HIP(hipSetDevice(ctx->device));
        const uint64_t n = left->n;
        RpNames nl, nr;
        raw_vector<uint64_t> rel_l, rel_r;  // rp_text waits before they go
        rp_upload_names(ctx, "left", h_names_l, h_name_off_l, n, nl, rel_l);
        if (right) rp_upload_names(ctx, "right", h_names_r, h_name_off_r, n, nr, rel_r);
        *out = rp_text("bbk_corrected_print", left, right, nl.blob.as<uint8_t>(), nl.off.as<uint64_t>(), nr.blob.as<uint8_t>(),
                       nr.off.as<uint64_t>(), qvoffset, tags);
    });
}

int bbk_corrected_print_resident(const bbk_corrected *left, const bbk_corrected *right, int qvoffset, int tags,
                                 bbk_fastq_text **out) {
    return guarded([&] {
        BBK_REQUIRE(left && out, BBK_ERR_ARG, "bbk_corrected_print_resident: NULL argument");
        rp_check("bbk_corrected_print_resident", left, right, qvoffset);
        BBK_REQUIRE(left->hr->has_names && (!right || right->hr->has_names), BBK_ERR_ARG,
                    "bbk_corrected_print_resident: the batch was made from host arrays and holds no names: "
                    "bbk_corrected_print takes them from the host");
        BBK_HIP(hipSetDevice(left->ctx->device));
        *out = rp_text("bbk_corrected_print_resident", left, right, left->hr->names.as<uint8_t>(), left->hr->name_off.as<uint64_t>(),
                       right ? right->hr->names.as<uint8_t>() : nullptr, right ? right->hr->name_off.as<uint64_t>() : nullptr,
                       qvoffset, tags);
    });
}

int bbk_fastq_text_streams(const bbk_fastq_text *t) { return t ? t->streams : 0; }

uint64_t bbk_fastq_text_size(const bbk_fastq_text *t, int stream) {
    return t && stream >= 0 && stream < t->streams ? t->start[stream + 1] - t->start[stream] : 0;
}

int bbk_fastq_text_export(bbk_ctx *ctx, const bbk_fastq_text *t, int stream, char *h_dst) {
    return guarded([&] {
        BBK_REQUIRE(ctx && t, BBK_ERR_ARG, "bbk_fastq_text_export: NULL argument");
        BBK_REQUIRE(stream >= 0 && stream < t->streams, BBK_ERR_ARG, "bbk_fastq_text_export: stream %d: the text has streams 0..%d", stream,
                    t->streams - 1);
        const uint64_t bytes = t->start[stream + 1] - t->start[stream];
        BBK_REQUIRE(bytes == 0 || h_dst, BBK_ERR_ARG, "bbk_fastq_text_export: NULL argument");
        BBK_HIP(hipSetDevice(ctx->device));
        if (bytes) d2h_big(ctx, h_dst, t->text.as<char>() + t->start[stream], bytes);
    });
}

int bbk_fastq_text_write(bbk_ctx *ctx, const bbk_fastq_text *t, int stream, const char *path, int append) {
    return guarded([&] {
        BBK_REQUIRE(ctx && t && path, BBK_ERR_ARG, "bbk_fastq_text_write: NULL argument");
        BBK_REQUIRE(stream >= 0 && stream < t->streams, BBK_ERR_ARG, "bbk_fastq_text_write: stream %d: the text has streams 0..%d", stream,
                    t->streams - 1);
        BBK_HIP(hipSetDevice(ctx->device));
        const uint64_t bytes = t->start[stream + 1] - t->start[stream];
        // positional writes behind what the file holds: O_APPEND would ignore their offsets
        const int fd = open(path, O_WRONLY | O_CREAT | (append ? 0 : O_TRUNC), 0644);
        BBK_REQUIRE(fd >= 0, BBK_ERR_IO, "cannot open %s for writing", path);
        struct stat sb;
        bool ok = fstat(fd, &sb) == 0;
        ok = ok && d2f_big(ctx, fd, append ? (uint64_t)sb.st_size : 0, t->text.as<char>() + t->start[stream], (size_t)bytes);
        const int cl = close(fd);
        BBK_REQUIRE(ok && cl == 0, BBK_ERR_IO, "short write to %s", path);
    });
}

void bbk_fastq_text_free(bbk_fastq_text *t) { delete t; }

}  // extern "C"
