// hreads.hip -- BayesHammer's reads, prepared on the device: what every stage of 4.3c-g needs
// before its first kernel.
//
// Replaces Read::trimNsAndBadQuality / trimLeftRight (common/io/reads/read.hpp:87-122) followed by
// ValidKMerGenerator<K>(read, 2) (projects/hammer/valid_kmer_generator.hpp:147-199) as KMerDataFiller, Expander and
// ReadCorrector apply them (kmer_data.cpp:163-186, expander.cpp:20-29, read_corrector.cpp:160-176), restated for the host in
// host/hammer_reads.hpp.  A batch keeps the records as parsed in HBM, and for every record its trim, the generator's valid
// starts as stretches under both nucleotide predicates (ACGTacgt: the k-mer table; ACGT: the corrector table) and the
// expander-candidate flag.  trim_quality BBK_NO_TRIM (INT_MIN, which until then meant "trim only Ns" and which nobody
// passed: the one addition to the accepted inputs) takes the records as trimmed already: every trim is (0, n), the rest
// follows from it, and the trimmed layout is the batch's own arrays (hreads_trimmed gathers nothing).
//
// The two rules are sequential walks in the reference; here they are a closed form over first / last positions and run
// lengths (tests/hreads_restated.py states it, tests/test_hreads_restated.py holds it against the literal rules):
//   trim       f, l = the first and the last position with base != 'N' and q > trim_quality; nothing is left without one;
//              size = n - f; the right trim (size = l - f + 1) only when l - f + 1 < size and l < size - f - 1 -- the second
//              comparison uses the size AFTER the left erase, so a left trim can suppress the right one (read.hpp:114)
//   generator  over the trimmed read of len bases: pos0 / end_ = the first / one past the last position with q >= 2,
//              T = end_ - k; a window start is an s >= pos0 with [s, s + k) inside [0, len) and all nucleotides; nothing
//              when pos0 > T, otherwise every window start below T and the first one at or above T (the search of Next()
//              runs to len_, not to end_, and does not check what it finds against end_)
// Kernels:
//   k_hr_prepare  one wavefront per record, lanes over the positions in chunks of 64: every predicate is a 64-bit ballot,
//                 and first / last / run information is carried from chunk to chunk in wave-uniform scalars.  A start s is
//                 handled at its window END e = s + k - 1 (run of nucleotides ending at e >= k), so nothing looks ahead;
//                 a stretch is written by the lane one past its last end (a falling edge of the valid-end mask), which
//                 finds the stretch's first end from the zeros of the mask below it.  Runs twice: the count pass writes
//                 the trims, the flags and the stretch counts, one scan gives the offsets (the candidate count rides in
//                 bits 40.. of the k-mer table's counts: one scan, one host wait), the write pass fills the tables.
//   k_hr_ranges   the byte ranges a view is made of: the trimmed read of every record / of every candidate, or every
//                 k-mer stretch
//   k_hr_pack     one wavefront per range: 64 bases -> two ballots (bit 0 and bit 1 of the code) -> two 2-bit words by
//                 bit interleaving; bbk_reads_from_ascii's layout
//   k_hr_copy     one wavefront per range: bytes by range (qualities of a view, the corrector's trimmed reads)
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>

#include "hammer.h"

namespace bbk {

constexpr uint32_t kHrMaxQual = 93;
constexpr unsigned kHrCandShift = 40;  // the candidate count above the stretch count in one scanned word
constexpr uint64_t kHrCountMask = (1ull << kHrCandShift) - 1;
constexpr uint32_t kHrNone = 0xFFFFFFFFu;

__device__ inline bool hr_nucl_kmer(uint8_t c) {  // common/sequence/nucl.hpp:45-62
    const uint8_t u = c & 0xDFu;
    return u == 'A' || u == 'C' || u == 'G' || u == 'T';
}
__device__ inline bool hr_nucl_corrector(uint8_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
__device__ inline uint32_t hr_top_bit(uint64_t m) { return 63u - (uint32_t)__builtin_clzll(m); }  // m != 0

// One table's walk over the window ends of a trimmed read; every member is the same in all lanes.
struct HrWalk {
    uint32_t carry_run = 0;  // nucleotides in a row ending right before the chunk
    uint32_t e0 = 0;         // first end of the open run of valid ends
    uint32_t count = 0;      // stretches closed so far
    uint32_t nvalid = 0;     // valid starts so far
    bool open = false;       // the last end before the chunk was valid
    bool done = false;       // the first window start at or above T has been taken

    // nm: the nucleotides of the 64 positions from cb (0 beyond len).  enabled: pos0 <= T.  E = T + k - 1, the window end of
    // start T.  Returns whether this lane closes a stretch; then *start / *length are the stretch (in the trimmed read) and
    // *slot its number in the record.
    __device__ bool take(uint64_t nm, uint32_t cb, uint32_t lane, uint32_t k, uint32_t len, uint32_t pos0, bool enabled,
                         int64_t E, uint32_t *start, uint32_t *length, uint32_t *slot) {
        const uint64_t z = ~nm & ((2ull << lane) - 1ull);  // non-nucleotides at or below this lane
        const uint32_t run = z ? lane - hr_top_bit(z) : lane + 1u + carry_run;
        const uint32_t e = cb + lane;
        const uint64_t wm = __ballot(e < len && run >= k && e + 1u >= k + pos0);
        uint64_t vm = 0;
        if (enabled) {
            const int64_t below = E - (int64_t)cb;  // ends of the chunk that are below E
            const uint64_t low = below <= 0 ? 0ull : below >= 64 ? ~0ull : (1ull << below) - 1ull;
            vm = wm & low;
            const uint64_t hi = wm & ~low;
            if (!done && hi) {
                vm |= hi & (0ull - hi);
                done = true;
            }
        }
        const uint64_t fm = ((vm << 1) | (open ? 1ull : 0ull)) & ~vm;  // a valid end right before, none here
        const bool falls = (fm >> lane) & 1ull;
        if (falls) {
            const uint64_t zz = ~vm & ((1ull << lane) - 1ull);
            const uint32_t first = zz ? cb + hr_top_bit(zz) + 1u : (open ? e0 : cb);
            *start = first + 1u - k;
            *length = e - first + k - 1u;
            *slot = count + (uint32_t)__popcll(fm & ((1ull << lane) - 1ull));
        }
        count += (uint32_t)__popcll(fm);
        nvalid += (uint32_t)__popcll(vm);
        const bool was_open = open;
        open = (vm >> 63) & 1ull;
        if (open) {
            const uint64_t zz = ~vm;
            e0 = zz ? cb + hr_top_bit(zz) + 1u : (was_open ? e0 : cb);
        }
        const uint64_t zn = ~nm;
        carry_run = zn ? (uint32_t)__builtin_clzll(zn) : carry_run + 64u;
        return falls;
    }
};

// WRITE false: trim, cand, packed[r] = k-mer stretches | candidate << 40, ccount[r] = corrector stretches.
// WRITE true:  packed / ccount hold the scanned values (n + 1 entries); koff / cpos are split out of packed, and the
//              stretches go to kst (starts in the record as parsed) and cst (starts in the trimmed read).
template <bool WRITE>
__global__ __launch_bounds__(256) void k_hr_prepare(const uint8_t *__restrict__ bases, const uint8_t *__restrict__ quals,
                                                   const uint64_t *__restrict__ off, uint64_t n_records, uint32_t k,
                                                   int trim_quality, uint32_t *__restrict__ trim, uint8_t *__restrict__ cand,
                                                   uint64_t *__restrict__ packed, uint64_t *__restrict__ ccount,
                                                   uint64_t *__restrict__ koff, uint64_t *__restrict__ cpos,
                                                   uint32_t *__restrict__ kst, uint32_t *__restrict__ cst) {
    const uint64_t r = (BBK_GID()) >> 6;
    if (r >= n_records) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t base = off[r];
    const uint32_t n = (uint32_t)(off[r + 1] - base);
    // ---- Read::trimNsAndBadQuality ----
    uint32_t first = kHrNone, last = 0;
    const bool whole = trim_quality == BBK_NO_TRIM;  // trimmed already: (0, n)
    for (uint32_t cb = 0; cb < n && !whole; cb += 64u) {
        const uint32_t p = cb + lane;
        bool g = false;
        if (p < n) g = bases[base + p] != 'N' && (int)quals[base + p] > trim_quality;
        const uint64_t m = __ballot(g);
        if (m) {
            if (first == kHrNone) first = cb + (uint32_t)__builtin_ctzll(m);
            last = cb + hr_top_bit(m);
        }
    }
    uint32_t tstart = 0, len = whole ? n : 0;
    if (first != kHrNone) {
        tstart = first;
        len = n - first;
        if (last - first + 1u < len && (int64_t)last < (int64_t)len - (int64_t)first - 1) len = last - first + 1u;
    }
    // ---- TrimBadQuality of the generator: pos0, end_ ----
    const uint64_t tb = base + tstart;
    uint32_t pos0 = kHrNone, end_ = 0;
    for (uint32_t cb = 0; cb < len; cb += 64u) {
        const uint32_t p = cb + lane;
        const uint64_t m = __ballot(p < len && quals[tb + p] >= 2);
        if (m) {
            if (pos0 == kHrNone) pos0 = cb + (uint32_t)__builtin_ctzll(m);
            end_ = cb + hr_top_bit(m) + 1u;
        }
    }
    const bool enabled = pos0 != kHrNone && (int64_t)pos0 <= (int64_t)end_ - (int64_t)k;
    const int64_t E = (int64_t)end_ - 1;
    uint64_t kbase = 0, kend = 0, cbase = 0, cend = 0;
    if (WRITE) {
        kbase = packed[r] & kHrCountMask;
        kend = packed[r + 1] & kHrCountMask;
        cbase = ccount[r];
        cend = ccount[r + 1];
    }
    // ---- the valid starts under both predicates, at their window ends; position len closes an open stretch ----
    HrWalk wk, wc;
    if (len >= k && enabled) {
        for (uint32_t cb = 0; cb <= len; cb += 64u) {
            const uint32_t p = cb + lane;
            uint8_t c = 0;
            if (p < len) c = bases[tb + p];
            const uint64_t nk = __ballot(hr_nucl_kmer(c)), nc = __ballot(hr_nucl_corrector(c));
            uint32_t s = 0, l = 0, j = 0;
            if (wk.take(nk, cb, lane, k, len, pos0, enabled, E, &s, &l, &j) && WRITE && kbase + j < kend) {
                kst[2 * (kbase + j)] = tstart + s;
                kst[2 * (kbase + j) + 1] = l;
            }
            if (wc.take(nc, cb, lane, k, len, pos0, enabled, E, &s, &l, &j) && WRITE && cbase + j < cend) {
                cst[2 * (cbase + j)] = s;
                cst[2 * (cbase + j) + 1] = l;
            }
        }
    }
    if (lane != 0) return;
    if (!WRITE) {
        const bool is_cand = len >= k && wk.nvalid == len - k + 1u;  // every start is valid: one stretch, the trimmed read
        trim[2 * r] = tstart;
        trim[2 * r + 1] = len;
        cand[r] = is_cand ? 1 : 0;
        packed[r] = (uint64_t)wk.count | ((uint64_t)(is_cand ? 1 : 0) << kHrCandShift);
        ccount[r] = wc.count;
    } else {
        koff[r] = kbase;
        cpos[r] = packed[r] >> kHrCandShift;
        if (r + 1 == n_records) {
            koff[n_records] = kend;
            cpos[n_records] = packed[n_records] >> kHrCandShift;
        }
    }
}

// mode 0: the trimmed read of every record; 1: of every candidate; 2: every k-mer stretch.  Range j: its first byte in the
// batch, its length, and the two values the scan of a view reads (packed words, bytes).
__global__ void k_hr_ranges(int mode, const uint64_t *__restrict__ off, const uint32_t *__restrict__ trim,
                            const uint8_t *__restrict__ cand, const uint64_t *__restrict__ cpos,
                            const uint64_t *__restrict__ koff, const uint32_t *__restrict__ kst, uint64_t n_records,
                            uint64_t n_ranges, uint64_t *__restrict__ first, uint32_t *__restrict__ len,
                            uint64_t *__restrict__ words, uint64_t *__restrict__ bytes) {
    const uint64_t r = BBK_GID();
    if (r >= n_records) return;
    uint64_t j = r, j1 = r + 1;
    if (mode == 1) {
        j = cpos[r];
        j1 = j + (cand[r] ? 1 : 0);
    } else if (mode == 2) {
        j = koff[r];
        j1 = koff[r + 1];
    }
    if (j1 > n_ranges) j1 = n_ranges;
    for (; j < j1; ++j) {
        const uint32_t s = mode == 2 ? kst[2 * j] : trim[2 * r], l = mode == 2 ? kst[2 * j + 1] : trim[2 * r + 1];
        first[j] = off[r] + s;
        len[j] = l;
        words[j] = ((uint64_t)l + 31u) >> 5;
        bytes[j] = l;
    }
}

// bit i of x -> bit 2i
__device__ inline uint64_t hr_spread(uint64_t x) {
    x &= 0xFFFFFFFFull;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}

__global__ __launch_bounds__(256) void k_hr_pack(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ first,
                                                const uint32_t *__restrict__ len, const uint64_t *__restrict__ woff,
                                                uint64_t n_ranges, uint64_t *__restrict__ out) {
    const uint64_t j = (BBK_GID()) >> 6;
    if (j >= n_ranges) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t src = first[j], w0 = woff[j];
    const uint32_t l = len[j];
    for (uint32_t cb = 0; cb < l; cb += 64u) {
        const uint32_t p = cb + lane;
        uint32_t code = 0;  // nucl.hpp:120-130 (dignucl): A 0, C 1, G 2, anything else 3; nothing beyond the read
        if (p < l) {
            const uint8_t u = bases[src + p] & 0xDFu;
            code = u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : 3u;
        }
        const uint64_t b0 = __ballot(code & 1u), b1 = __ballot(code & 2u);
        if (lane < 2 && cb + 32u * lane < l) {
            const uint64_t lo = lane ? b0 >> 32 : b0, hi = lane ? b1 >> 32 : b1;
            out[w0 + (cb >> 5) + lane] = hr_spread(lo) | (hr_spread(hi) << 1);
        }
    }
}

__global__ __launch_bounds__(256) void k_hr_copy(const uint8_t *__restrict__ src, const uint64_t *__restrict__ first,
                                                const uint32_t *__restrict__ len, const uint64_t *__restrict__ boff,
                                                uint64_t n_ranges, uint8_t *__restrict__ out) {
    const uint64_t j = (BBK_GID()) >> 6;
    if (j >= n_ranges) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t s = first[j], d = boff[j];
    const uint32_t l = len[j];
    for (uint32_t p = lane; p < l; p += 64u) out[d + p] = src[s + p];
}

// The ranges of one mode with the scans of their words and bytes: first / len of m ranges, woff / boff of m + 1 entries.
struct HrRanges {
    uint64_t m = 0, n_words = 0, n_bytes = 0;
    DevBuf first, len, woff, boff;
};

static void hr_ranges(const bbk_hreads *hr, int mode, HrRanges &g) {
    bbk_ctx *ctx = hr->ctx;
    BBK_HIP(hipSetDevice(ctx->device));
    const uint64_t m = mode == 0 ? hr->n : mode == 1 ? hr->n_cand : hr->n_kst;
    g.m = m;
    g.first.alloc(m * 8);
    g.len.alloc((m + 1) * 4);
    g.woff.alloc((m + 1) * 8);
    g.boff.alloc((m + 1) * 8);
    if (m == 0) {
        BBK_HIP(hipMemsetAsync(g.woff.p, 0, 8, ctx->stream));
        BBK_HIP(hipMemsetAsync(g.boff.p, 0, 8, ctx->stream));
        return;
    }
    launch_items_timed(ctx, "k_hr_ranges", k_hr_ranges, hr->n, mode, hr->off.as<uint64_t>(), hr->trim.as<uint32_t>(),
                       hr->cand.as<uint8_t>(), hr->cpos.as<uint64_t>(), hr->koff.as<uint64_t>(), hr->kst.as<uint32_t>(), hr->n, m,
                       g.first.as<uint64_t>(), g.len.as<uint32_t>(), g.woff.as<uint64_t>(), g.boff.as<uint64_t>());
    uint64_t totals[2] = {0, 0};
    exclusive_scan2_u64(ctx, g.woff.as<uint64_t>(), g.woff.as<uint64_t>(), g.boff.as<uint64_t>(), g.boff.as<uint64_t>(), m, totals);
    g.n_words = totals[0];
    g.n_bytes = totals[1];
    BBK_REQUIRE(g.n_bytes <= hr->bytes, BBK_ERR_INTERNAL, "bbk_hreads: %llu bytes in the ranges of a batch of %llu",
                (unsigned long long)g.n_bytes, (unsigned long long)hr->bytes);
}

// mode 1 or 2: the view's reads, and its qualities when with_quals
static void hr_make_view(const bbk_hreads *hr, int mode, bool with_quals, bbk_hreads::View &v) {
    bbk_ctx *ctx = hr->ctx;
    HrRanges g;
    hr_ranges(hr, mode, g);
    bbk_reads &rd = v.reads;
    rd.ctx = ctx;
    rd.n = g.m;
    rd.n_words = g.n_words;
    rd.bases = g.n_bytes;
    rd.own_words.alloc((g.n_words + 1) * 8);
    BBK_HIP(hipMemsetAsync(rd.own_words.as<uint64_t>() + g.n_words, 0, 8, ctx->stream));
    if (g.m)
        launch_items_timed(ctx, "k_hr_pack", k_hr_pack, g.m * 64, hr->bases.as<uint8_t>(), g.first.as<uint64_t>(),
                           g.len.as<uint32_t>(), g.woff.as<uint64_t>(), g.m, rd.own_words.as<uint64_t>());
    if (with_quals) {
        v.quals.q.alloc(g.n_bytes + 16);
        if (g.m)
            launch_items_timed(ctx, "k_hr_copy", k_hr_copy, g.m * 64, hr->quals.as<uint8_t>(), g.first.as<uint64_t>(),
                               g.len.as<uint32_t>(), g.boff.as<uint64_t>(), g.m, v.quals.q.as<uint8_t>());
        v.quals.reads = &rd;
        v.quals.n = g.m;
        v.quals.bytes = g.n_bytes;
        v.quals.off = std::move(g.boff);
    }
    BBK_HIP(hipStreamSynchronize(ctx->stream));  // g.first goes now
    rd.own_woff = std::move(g.woff);
    rd.own_len = std::move(g.len);
    rd.d_words = rd.own_words.as<uint64_t>();
    rd.d_woff = rd.own_woff.as<uint64_t>();
    rd.d_len = rd.own_len.as<uint32_t>();
    v.made = true;
}

const bbk_hreads::Trimmed &hreads_trimmed(const bbk_hreads *hr) {
    bbk_hreads::Trimmed &t = hr->trimmed;
    if (t.made) return t;
    if (hr->trim_quality == BBK_NO_TRIM) {  // every trim is (0, n): the records as parsed are the layout
        t.bases = hr->bases.as<uint8_t>();
        t.quals = hr->quals.as<uint8_t>();
        t.off = hr->off.as<uint64_t>();
        t.total = hr->bytes;
        t.made = true;
        return t;
    }
    bbk_ctx *ctx = hr->ctx;
    HrRanges g;
    hr_ranges(hr, 0, g);
    t.own_bases.alloc(g.n_bytes);
    t.own_quals.alloc(g.n_bytes);
    if (g.m) {
        KernelTimer timer(ctx, "k_hr_copy");
        launch_items(ctx, "k_hr_copy", k_hr_copy, g.m * 64, hr->bases.as<uint8_t>(), g.first.as<uint64_t>(), g.len.as<uint32_t>(),
                     g.boff.as<uint64_t>(), g.m, t.own_bases.as<uint8_t>());
        launch_items(ctx, "k_hr_copy", k_hr_copy, g.m * 64, hr->quals.as<uint8_t>(), g.first.as<uint64_t>(), g.len.as<uint32_t>(),
                     g.boff.as<uint64_t>(), g.m, t.own_quals.as<uint8_t>());
    }
    BBK_HIP(hipStreamSynchronize(ctx->stream));
    t.own_off = std::move(g.boff);
    t.bases = t.own_bases.as<uint8_t>();
    t.quals = t.own_quals.as<uint8_t>();
    t.off = t.own_off.as<uint64_t>();
    t.total = g.n_bytes;
    t.made = true;
    return t;
}

// The prepare tail both doors share: the count pass, one scan (the one wait: what was queued before it is done with it as
// well), the write pass
void hreads_prepare(const char *fn, const char *unit, bbk_hreads *H) {
    bbk_ctx *ctx = H->ctx;
    const uint64_t n = H->n, bytes = H->bytes;
    const unsigned k = H->k;
    const int trim_quality = H->trim_quality;
    H->trim.alloc(n * 8);
    H->cand.alloc(n);
    H->koff.alloc((n + 1) * 8);
    H->coff.alloc((n + 1) * 8);
    H->cpos.alloc((n + 1) * 8);
    if (n == 0) {
        BBK_HIP(hipMemsetAsync(H->koff.p, 0, 8, ctx->stream));
        BBK_HIP(hipMemsetAsync(H->coff.p, 0, 8, ctx->stream));
        BBK_HIP(hipMemsetAsync(H->cpos.p, 0, 8, ctx->stream));
        H->kst.alloc(0);
        H->cst.alloc(0);
        BBK_HIP(hipStreamSynchronize(ctx->stream));
        return;
    }
    DevBuf packed((n + 1) * 8);
    launch_items_timed(ctx, "k_hr_prepare", k_hr_prepare<false>, n * 64, H->bases.as<uint8_t>(), H->quals.as<uint8_t>(),
                       H->off.as<uint64_t>(), n, (uint32_t)k, trim_quality, H->trim.as<uint32_t>(), H->cand.as<uint8_t>(),
                       packed.as<uint64_t>(), H->coff.as<uint64_t>(), (uint64_t *)nullptr, (uint64_t *)nullptr,
                       (uint32_t *)nullptr, (uint32_t *)nullptr);
    uint64_t totals[2] = {0, 0};  // the one wait: the uploads are done with it as well
    exclusive_scan2_u64(ctx, packed.as<uint64_t>(), packed.as<uint64_t>(), H->coff.as<uint64_t>(), H->coff.as<uint64_t>(), n,
                        totals);
    H->n_kst = totals[0] & kHrCountMask;
    H->n_cand = totals[0] >> kHrCandShift;
    H->n_cst = totals[1];
    BBK_REQUIRE(H->n_kst <= bytes && H->n_cst <= bytes && H->n_cand <= n, BBK_ERR_INTERNAL,
                "%s: %llu + %llu stretches, %llu candidates for %llu bases in %llu %ss", fn,
                (unsigned long long)H->n_kst, (unsigned long long)H->n_cst, (unsigned long long)H->n_cand,
                (unsigned long long)bytes, (unsigned long long)n, unit);
    H->kst.alloc(H->n_kst * 8);
    H->cst.alloc(H->n_cst * 8);
    launch_items_timed(ctx, "k_hr_prepare", k_hr_prepare<true>, n * 64, H->bases.as<uint8_t>(), H->quals.as<uint8_t>(),
                       H->off.as<uint64_t>(), n, (uint32_t)k, trim_quality, (uint32_t *)nullptr, (uint8_t *)nullptr,
                       packed.as<uint64_t>(), H->coff.as<uint64_t>(), H->koff.as<uint64_t>(), H->cpos.as<uint64_t>(),
                       H->kst.as<uint32_t>(), H->cst.as<uint32_t>());
    BBK_HIP(hipStreamSynchronize(ctx->stream));  // `packed` goes now
}

// The offsets, then the qualities, are checked here for every entry that takes records from the host; a record is a `unit`
// in what `fn` refuses
std::unique_ptr<bbk_hreads> hreads_from_host(const char *fn, const char *unit, bbk_ctx *ctx, const char *h_bases,
                                             const uint8_t *h_qual, const uint64_t *h_offsets, uint64_t n, unsigned k,
                                             int trim_quality) {
    BBK_REQUIRE(k >= 1 && k <= 32, BBK_ERR_ARG, "%s: k = %u: one-word k-mers only (1 <= k <= 32)", fn, k);
    const uint64_t first = h_offsets[0];
    uint64_t longest = 0;
    for (uint64_t r = 0; r < n; ++r) {
        BBK_REQUIRE(h_offsets[r] <= h_offsets[r + 1], BBK_ERR_ARG, "%s: the offsets of %s %llu descend", fn, unit,
                    (unsigned long long)r);
        longest = std::max(longest, h_offsets[r + 1] - h_offsets[r]);
    }
    BBK_REQUIRE(longest < (1ull << 31), BBK_ERR_ARG, "%s: a %s of %llu bases: fewer than 2^31 are needed", fn, unit,
                (unsigned long long)longest);
    const uint64_t bytes = h_offsets[n] - first;
    BBK_REQUIRE(bytes == 0 || (h_bases && h_qual), BBK_ERR_ARG, "%s: NULL argument", fn);
    BBK_REQUIRE(bytes <= kHrCountMask && n <= kHrCountMask, BBK_ERR_ARG,
                "%s: %llu bases in %llu %ss: at most 2^%u of either in one batch", fn, (unsigned long long)bytes,
                (unsigned long long)n, unit, kHrCandShift);
    uint8_t worst = 0;
#pragma omp parallel for reduction(max : worst) schedule(static)
    for (int64_t i = 0; i < (int64_t)bytes; ++i) worst = std::max(worst, h_qual[first + i]);
    if (worst > kHrMaxQual)  // say where, like the other entries do
        for (uint64_t i = first; i < first + bytes; ++i)
            BBK_REQUIRE(h_qual[i] <= kHrMaxQual, BBK_ERR_ARG,
                        "%s: the quality at byte %llu is %u: %u at most (the offset is already subtracted)", fn,
                        (unsigned long long)i, (unsigned)h_qual[i], kHrMaxQual);
    BBK_HIP(hipSetDevice(ctx->device));
    auto hr = std::make_unique<bbk_hreads>();
    hr->ctx = ctx;
    hr->k = k;
    hr->trim_quality = trim_quality;
    hr->n = n;
    hr->bytes = bytes;
    hr->longest = longest;
    raw_vector<uint64_t> rel(n + 1);
    for (uint64_t r = 0; r <= n; ++r) rel[r] = h_offsets[r] - first;
    upload(ctx, hr->bases, (const uint8_t *)h_bases + first, bytes);
    upload(ctx, hr->quals, h_qual + first, bytes);
    upload(ctx, hr->off, rel.data(), n + 1);
    hreads_prepare(fn, unit, hr.get());
    return hr;
}

}  // namespace bbk

using namespace bbk;

extern "C" {

int bbk_hreads_from_host(bbk_ctx *ctx, const char *h_bases, const uint8_t *h_qual, const uint64_t *h_offsets, uint64_t n,
                         unsigned k, int trim_quality, bbk_hreads **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && out && h_offsets, BBK_ERR_ARG, "bbk_hreads_from_host: NULL argument");
        *out = hreads_from_host("bbk_hreads_from_host", "record", ctx, h_bases, h_qual, h_offsets, n, k, trim_quality).release();
    });
}

uint64_t bbk_hreads_size(const bbk_hreads *hr) { return hr ? hr->n : 0; }
uint64_t bbk_hreads_kmer_stretches(const bbk_hreads *hr) { return hr ? hr->n_kst : 0; }
uint64_t bbk_hreads_corrector_stretches(const bbk_hreads *hr) { return hr ? hr->n_cst : 0; }
uint64_t bbk_hreads_candidates(const bbk_hreads *hr) { return hr ? hr->n_cand : 0; }

int bbk_hreads_export(bbk_ctx *ctx, const bbk_hreads *hr, uint32_t *h_trim, uint8_t *h_candidate, uint64_t *h_koff,
                      uint32_t *h_kst, uint64_t *h_coff, uint32_t *h_cst) {
    return guarded([&] {
        BBK_REQUIRE(ctx && hr, BBK_ERR_ARG, "bbk_hreads_export: NULL argument");
        BBK_HIP(hipSetDevice(ctx->device));
        if (h_trim && hr->n) d2h_big(ctx, h_trim, hr->trim.p, hr->n * 8);
        if (h_candidate && hr->n) d2h_big(ctx, h_candidate, hr->cand.p, hr->n);
        if (h_koff) d2h_big(ctx, h_koff, hr->koff.p, (hr->n + 1) * 8);
        if (h_kst && hr->n_kst) d2h_big(ctx, h_kst, hr->kst.p, hr->n_kst * 8);
        if (h_coff) d2h_big(ctx, h_coff, hr->coff.p, (hr->n + 1) * 8);
        if (h_cst && hr->n_cst) d2h_big(ctx, h_cst, hr->cst.p, hr->n_cst * 8);
    });
}

uint64_t bbk_hreads_bases(const bbk_hreads *hr) { return hr ? hr->bytes : 0; }
uint64_t bbk_hreads_name_bytes(const bbk_hreads *hr) { return hr ? hr->name_bytes : 0; }

int bbk_hreads_export_records(bbk_ctx *ctx, const bbk_hreads *hr, char *h_bases, uint8_t *h_quals, uint64_t *h_offsets,
                              char *h_names, uint64_t *h_name_off) {
    return guarded([&] {
        BBK_REQUIRE(ctx && hr, BBK_ERR_ARG, "bbk_hreads_export_records: NULL argument");
        BBK_HIP(hipSetDevice(ctx->device));
        if (h_bases && hr->bytes) d2h_big(ctx, h_bases, hr->bases.p, hr->bytes);
        if (h_quals && hr->bytes) d2h_big(ctx, h_quals, hr->quals.p, hr->bytes);
        if (h_offsets) d2h_big(ctx, h_offsets, hr->off.p, (hr->n + 1) * 8);
        if (h_names && hr->name_bytes) d2h_big(ctx, h_names, hr->names.p, hr->name_bytes);
        if (h_name_off) {
            if (hr->has_names) d2h_big(ctx, h_name_off, hr->name_off.p, (hr->n + 1) * 8);
            else memset(h_name_off, 0, (hr->n + 1) * 8);  // a batch made from host arrays: every name is empty
        }
    });
}

int bbk_hreads_stretch_view(const bbk_hreads *hr, const bbk_reads **reads, const bbk_quals **quals) {
    return guarded([&] {
        BBK_REQUIRE(hr && reads, BBK_ERR_ARG, "bbk_hreads_stretch_view: NULL argument");
        if (!hr->stretch_view.made) hr_make_view(hr, 2, true, hr->stretch_view);
        *reads = &hr->stretch_view.reads;
        if (quals) *quals = &hr->stretch_view.quals;
    });
}

int bbk_hreads_candidate_view(const bbk_hreads *hr, const bbk_reads **reads) {
    return guarded([&] {
        BBK_REQUIRE(hr && reads, BBK_ERR_ARG, "bbk_hreads_candidate_view: NULL argument");
        if (!hr->candidate_view.made) hr_make_view(hr, 1, false, hr->candidate_view);
        *reads = &hr->candidate_view.reads;
    });
}

void bbk_hreads_free(bbk_hreads *hr) { delete hr; }

}  // extern "C"
