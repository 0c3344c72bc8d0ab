// kmerstat.hip -- BayesHammer's quality-aware k-mer statistics (KMerData) over a both-strand k-mer set (DESIGN.md f9,
// section 4.3d).
//
// Replaces KMerDataCounter::FillKMerData / KMerDataFiller (projects/hammer/kmer_data.cpp:119-187,369-399): for every
// valid k-mer position of every read, the k-mer and its reverse complement are looked up in the index and a
// KMerStat(1, (float)(1 - cp), q) is merged into the entry under a spin lock (Merge, :119-123): count += 1, total_qual *=
// factor (float), qual[i] = min(63, qual[i] + (q[i] & 63)) (NibbleString::operator+=, kmer_stat.hpp:95-101, whose
// constructor masks and does not saturate, :60-69).  cp is the product of Globals::quality_probs over the window
// (valid_kmer_generator.hpp:164-199; the table is hammer_error_prob, hammer.h).  Which positions are valid -- the trimming of
// Read::trimNsAndBadQuality and the generator's own rule -- is the host's business (host/hammer_reads.hpp): every k-mer
// position of a pushed read is an occurrence.
//
// Here, for k <= 32 and an ascending both-strand set of fewer than 2^32 k-mers:
//   accumulators: one record of 2 + A u64 per k-mer, A = ceil(k / 10): the fixed-point sum of log2(factor), the count,
//     and the quality sums ten to a word (6 bits each, none straddles a word, so one compare-and-swap covers whole sums;
//     the reference's bit-contiguous layout puts sum 10 across words 0 and 1, where two swaps could interleave with
//     another occurrence's).  Everything is added with integer atomics, so the result does not depend on the order of
//     the reads, on how they are split into batches or on scheduling -- byte for byte.
//   k_ks_accum: one wavefront per read, lanes over its k-mer positions (the shape of readfilter.hip: k_median_filter).
//   k_ks_finish: total_qual = (float)exp2(sum * 2^-F), and the sums packed into QualBitSet words (6k bits, bit-contiguous,
//     little-endian, ceil(6k / 64) words, kmer_stat.hpp:49-118).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "hammer.h"
#include "kmer_ops.h"

namespace bbk {

// Fixed-point fraction bits of the log sum.  A quality is at most 93 (bbk_quals_from_host refuses more: '~', the last
// printable character, is 33 + 93).  cp is a product of probabilities, so 1 - cp >= 1 - Prob(q) of any one base of the
// window >= 10^-9.3 > 2^-31, and 1 - cp < 1; rounding to float keeps the factor in [2^-31, 1].  So |log2 factor| <= 31,
// a term is at most 31 * 2^26 in magnitude, and 2^32 - 1 of them (a u32 count) stay below 31 * 2^58 < 2^63: the sum
// cannot overflow.  (F = 27 would: 31 * 2^59 > 2^63.)  Rounding a term moves the exponent by at most 2^-27, the factor
// by a relative 2^-27 * ln 2.
constexpr int kKsFrac = 26;
constexpr uint64_t kKsEven = 0x03F03F03F03F03Full;  // sums 0, 2, 4, 6, 8 of a word
constexpr uint64_t kKsOnes = 0x001001001001001ull;
constexpr uint32_t kKsMaxQual = 93;

// per-field min(63, a + b) of five 6-bit fields 12 bits apart
__host__ __device__ inline uint64_t ks_satadd5(uint64_t a, uint64_t b) {
    const uint64_t s = a + b;  // <= 126 per field: stays inside its 12 bits
    const uint64_t ov = (s >> 6) & kKsOnes;
    return (s | (ov * 0x3Full)) & kKsEven;
}
// the same for the ten sums of an accumulator word
__host__ __device__ inline uint64_t ks_satadd(uint64_t a, uint64_t b) {
    return ks_satadd5(a & kKsEven, b & kKsEven) | (ks_satadd5((a >> 6) & kKsEven, (b >> 6) & kKsEven) << 6);
}

// Merge (kmer_data.cpp:119-123) of one occurrence into record i
template <int A>
__device__ inline void ks_merge(uint64_t *__restrict__ rec, uint64_t i, long long term, const uint64_t (&add)[A]) {
    uint64_t *r = rec + i * (uint64_t)(2 + A);
    atomicAdd(reinterpret_cast<unsigned long long *>(r), (unsigned long long)term);
    atomicAdd(reinterpret_cast<uint32_t *>(r + 1), 1u);
#pragma unroll
    for (int w = 0; w < A; ++w) {
        unsigned long long *p = reinterpret_cast<unsigned long long *>(r + 2 + w);
        unsigned long long old = __atomic_load_n(p, __ATOMIC_RELAXED);
        for (;;) {
            const unsigned long long nw = ks_satadd(old, add[w]);
            if (nw == old) break;  // saturated (or nothing to add): no atomic
            const unsigned long long seen = atomicCAS(p, old, nw);
            if (seen == old) break;
            old = seen;
        }
    }
}

// one wavefront per read, lanes over its k-mer positions
template <int A>
__global__ __launch_bounds__(256) void k_ks_accum(const uint64_t *__restrict__ words, const uint64_t *__restrict__ woff,
                                                 const uint32_t *__restrict__ len, uint64_t n_reads,
                                                 const uint8_t *__restrict__ qual, const uint64_t *__restrict__ qoff, int k,
                                                 const Key<1> *__restrict__ keys, PrefixTable P,
                                                 const double *__restrict__ probs, uint64_t *__restrict__ rec) {
    __shared__ double s_prob[256];
    s_prob[threadIdx.x] = probs[threadIdx.x];
    __syncthreads();
    const uint64_t r = (BBK_GID()) >> 6;
    if (r >= n_reads) return;
    const int lane = threadIdx.x & 63;
    const uint32_t L = len[r];
    if (L < (uint32_t)k) return;
    const uint32_t nk = L - (uint32_t)k + 1u;
    const uint64_t *rw = words + woff[r];
    const uint8_t *rq = qual + qoff[r];
    for (uint32_t p = lane; p < nk; p += 64) {
        const Key<1> f = kmer_extract<1>(rw, p, k);
        const Key<1> rc = kmer_rc<1>(f, k);
        const uint64_t fi = table_find<1>(keys, P, f);
        const uint64_t ri = table_find<1>(keys, P, rc);
        if (fi == kNotFound && ri == kNotFound) continue;  // checking_seq_idx == -1 (kmer_data.cpp:127-129,146-148)
        const uint8_t *q = rq + p;
        double cp = 1.0;
        uint64_t fw[A], rv[A];
#pragma unroll
        for (int w = 0; w < A; ++w) fw[w] = rv[w] = 0ull;
#pragma unroll
        for (int j = 0; j < 10 * A; ++j) {
            if (j < k) {
                const uint32_t a = q[j], b = q[k - 1 - j];
                cp *= s_prob[a];
                fw[j / 10] |= (uint64_t)(a & 63u) << (6 * (j % 10));  // the constructor masks (kmer_stat.hpp:60-69)
                rv[j / 10] |= (uint64_t)(b & 63u) << (6 * (j % 10));  // rcq[K - i - 1] = q[i] (kmer_data.cpp:143-144)
            }
        }
        const float factor = (float)(1.0 - cp);  // KMerStat(1, (float)prob, q), kmer_data.cpp:133,179
        const long long term = __double2ll_rn(log2((double)factor) * (double)(1ull << kKsFrac));
        if (fi != kNotFound) ks_merge<A>(rec, fi, term, fw);
        if (ri != kNotFound) ks_merge<A>(rec, ri, term, rv);
    }
}

template <int A>
__global__ __launch_bounds__(256) void k_ks_finish(const uint64_t *__restrict__ rec, uint64_t n, int k, int qual_words,
                                                  uint32_t *__restrict__ count, float *__restrict__ total_qual,
                                                  uint64_t *__restrict__ qual, uint32_t *__restrict__ status) {
    const uint64_t i = BBK_GID();
    if (i >= n) return;
    const uint64_t *r = rec + i * (uint64_t)(2 + A);
    const long long sum = (long long)r[0];
    const uint32_t c = (uint32_t)r[1];
    count[i] = c;
    if (c >> 31) atomicOr(status, 1u);
    total_qual[i] = (float)exp2((double)sum * (1.0 / (double)(1ull << kKsFrac)));
    uint64_t out[3] = {0ull, 0ull, 0ull};  // 6 * 32 = 192 bits
#pragma unroll
    for (int j = 0; j < 10 * A && j < 32; ++j) {
        if (j < k) {
            const uint64_t v = (r[2 + j / 10] >> (6 * (j % 10))) & 63ull;
            out[(6 * j) >> 6] |= v << ((6 * j) & 63);
            if (((6 * j) & 63) > 58) out[((6 * j) >> 6) + 1] |= v >> (64 - ((6 * j) & 63));
        }
    }
#pragma unroll
    for (int w = 0; w < 3; ++w)
        if (w < qual_words) qual[i * (uint64_t)qual_words + w] = out[w];
}

// the one switch on the accumulator words of a record, ceil(k / 10) in 1..4
template <class F>
static void dispatch_acc(unsigned A, F &&f) {
    switch (A) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        default: BBK_REQUIRE(false, BBK_ERR_INTERNAL, "unsupported accumulator width %u", A);
    }
}

static void ks_finish(bbk_kmerstats *ks) {
    if (ks->finished) return;
    bbk_ctx *ctx = ks->ctx;
    BBK_HIP(hipSetDevice(ctx->device));
    ks->count_overflow = false;
    if (ks->n) {
        DevBuf status(16);
        BBK_HIP(hipMemsetAsync(status.p, 0, 16, ctx->stream));
        dispatch_acc(ks->acc_words, [&](auto a) {
            launch_items_timed(ctx, "k_ks_finish", k_ks_finish<decltype(a)::value>, ks->n, ks->rec.as<uint64_t>(), ks->n,
                               (int)ks->k, (int)ks->qual_words, ks->count.as<uint32_t>(), ks->total_qual.as<float>(),
                               ks->qual.as<uint64_t>(), status.as<uint32_t>());
        });
        uint32_t h_status = 0;
        BBK_HIP(hipMemcpyAsync(&h_status, status.p, 4, hipMemcpyDeviceToHost, ctx->stream));
        BBK_HIP(hipStreamSynchronize(ctx->stream));
        ks->count_overflow = h_status != 0;
    }
    ks->finished = true;
}

// the handle of bbk_kmerstats_begin / _load over a set the stage accepts, with its lookup index
static std::unique_ptr<bbk_kmerstats> ks_new(const char *fn, bbk_ctx *ctx, const bbk_kmerset *set) {
    BBK_REQUIRE(!(set->flags & BBK_CANONICAL), BBK_ERR_ARG,
                "%s: needs a both-strand k-mer set (bbk_count(BBK_BOTH_STRANDS)): this one is canonical only (BBK_CANONICAL)", fn);
    require_hammer_set(fn, set);
    BBK_HIP(hipSetDevice(ctx->device));
    auto ks = std::make_unique<bbk_kmerstats>();
    ks->ctx = ctx;
    ks->set = set;
    ks->k = set->k;
    ks->n = set->n;
    ks->acc_words = (set->k + 9) / 10;
    ks->qual_words = (6 * set->k + 63) / 64;
    if (ks->n) ks->prefix.build(ctx, set->keys.as<uint64_t>(), 1, set->k, set->n);
    return ks;
}

}  // namespace bbk

using namespace bbk;

extern "C" {

int bbk_quals_from_host(bbk_ctx *ctx, const bbk_reads *reads, const uint8_t *h_qual, const uint64_t *h_offsets,
                        uint64_t n_reads, bbk_quals **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && reads && out && (n_reads == 0 || (h_qual && h_offsets)), BBK_ERR_ARG,
                    "bbk_quals_from_host: NULL argument");
        BBK_REQUIRE(n_reads == reads->n, BBK_ERR_ARG, "bbk_quals_from_host: %llu quality strings for %llu reads",
                    (unsigned long long)n_reads, (unsigned long long)reads->n);
        BBK_HIP(hipSetDevice(ctx->device));
        std::vector<uint32_t> len(n_reads);
        if (n_reads) {
            BBK_HIP(hipMemcpyAsync(len.data(), reads->d_len, n_reads * 4, hipMemcpyDeviceToHost, ctx->stream));
            BBK_HIP(hipStreamSynchronize(ctx->stream));
        }
        std::vector<uint64_t> off(n_reads + 1, 0);
        for (uint64_t r = 0; r < n_reads; ++r) {
            BBK_REQUIRE(h_offsets[r + 1] >= h_offsets[r] && h_offsets[r + 1] - h_offsets[r] == len[r], BBK_ERR_ARG,
                        "bbk_quals_from_host: read %llu has %u bases and %llu qualities (the reads must be the stretches "
                        "the qualities were cut for: one run of ACGT each)",
                        (unsigned long long)r, len[r], (unsigned long long)(h_offsets[r + 1] - h_offsets[r]));
            off[r + 1] = off[r] + len[r];
        }
        const uint64_t bytes = off[n_reads];
        const uint8_t *src = n_reads ? h_qual + h_offsets[0] : nullptr;
        for (uint64_t i = 0; i < bytes; ++i)
            BBK_REQUIRE(src[i] <= kKsMaxQual, BBK_ERR_ARG,
                        "bbk_quals_from_host: quality %u (byte %llu): at most %u once the offset is subtracted (is the "
                        "offset right?)",
                        (unsigned)src[i], (unsigned long long)i, kKsMaxQual);
        auto q = std::make_unique<bbk_quals>();
        q->reads = reads;
        q->n = n_reads;
        q->bytes = bytes;
        q->q.alloc(bytes + 16);
        if (bytes) BBK_HIP(hipMemcpyAsync(q->q.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
        upload(ctx, q->off, off.data(), n_reads + 1);
        BBK_HIP(hipStreamSynchronize(ctx->stream));
        *out = q.release();
    });
}

void bbk_quals_free(bbk_quals *q) { delete q; }

int bbk_kmerstats_begin(bbk_ctx *ctx, const bbk_kmerset *set, bbk_kmerstats **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && set && out, BBK_ERR_ARG, "bbk_kmerstats_begin: NULL argument");
        auto ks = ks_new("bbk_kmerstats_begin", ctx, set);
        double probs[256];  // Globals::quality_probs
        for (unsigned q = 0; q < 256; ++q) probs[q] = 1 - hammer_error_prob(q);
        upload(ctx, ks->probs, probs, 256);
        BBK_HIP(hipStreamSynchronize(ctx->stream));  // probs is on this frame
        const size_t rec_bytes = ks->n * (2 + ks->acc_words) * 8;
        ks->rec.alloc(rec_bytes);
        ks->count.alloc(ks->n * 4);
        ks->total_qual.alloc(ks->n * 4);
        ks->qual.alloc(ks->n * ks->qual_words * 8);
        if (ks->n) BBK_HIP(hipMemsetAsync(ks->rec.p, 0, rec_bytes, ctx->stream));
        *out = ks.release();
    });
}

int bbk_kmerstats_push(bbk_kmerstats *ks, const bbk_reads *reads, const bbk_quals *quals) {
    return guarded([&] {
        BBK_REQUIRE(ks && reads && quals, BBK_ERR_ARG, "bbk_kmerstats_push: NULL argument");
        BBK_REQUIRE(quals->reads == reads && quals->n == reads->n, BBK_ERR_ARG,
                    "bbk_kmerstats_push: the qualities were not made for these reads (bbk_quals_from_host)");
        BBK_REQUIRE(!ks->loaded, BBK_ERR_ARG,
                    "bbk_kmerstats_push: these statistics were read from a file (bbk_kmerstats_load): nothing can be added");
        bbk_ctx *ctx = ks->ctx;
        BBK_HIP(hipSetDevice(ctx->device));
        ks->finished = false;
        if (reads->n == 0 || ks->n == 0) return;
        dispatch_acc(ks->acc_words, [&](auto a) {
            launch_items_timed(ctx, "k_ks_accum", k_ks_accum<decltype(a)::value>, reads->n * 64, reads->d_words, reads->d_woff,
                               reads->d_len, reads->n, quals->q.as<uint8_t>(), quals->off.as<uint64_t>(), (int)ks->k,
                               ks->set->keys.as<Key<1>>(), ks->prefix.table(), ks->probs.as<double>(),
                               ks->rec.as<uint64_t>());
        });
        BBK_HIP(hipStreamSynchronize(ctx->stream));  // the caller may free the reads and the qualities
    });
}

int bbk_kmerstats_finish(bbk_kmerstats *ks) {
    return guarded([&] {
        BBK_REQUIRE(ks, BBK_ERR_ARG, "bbk_kmerstats_finish: NULL argument");
        ks_finish(ks);
    });
}

uint64_t bbk_kmerstats_size(const bbk_kmerstats *ks) { return ks ? ks->n : 0; }

int bbk_kmerstats_export(bbk_ctx *ctx, const bbk_kmerstats *ks, uint32_t *h_count, float *h_total_qual,
                         uint64_t *h_qual_words) {
    return guarded([&] {
        BBK_REQUIRE(ctx && ks, BBK_ERR_ARG, "bbk_kmerstats_export: NULL argument");
        BBK_REQUIRE(ks->finished, BBK_ERR_ARG, "bbk_kmerstats_export: call bbk_kmerstats_finish after the last push");
        BBK_HIP(hipSetDevice(ctx->device));
        if (ks->n == 0) return;
        if (h_count) d2h_big(ctx, h_count, ks->count.p, ks->n * 4);
        if (h_total_qual) d2h_big(ctx, h_total_qual, ks->total_qual.p, ks->n * 4);
        if (h_qual_words) d2h_big(ctx, h_qual_words, ks->qual.p, ks->n * ks->qual_words * 8);
    });
}

int bbk_kmerstats_write(bbk_ctx *ctx, const bbk_kmerstats *ks, const char *path) {
    return guarded([&] {
        BBK_REQUIRE(ctx && ks && path, BBK_ERR_ARG, "bbk_kmerstats_write: NULL argument");
        BBK_REQUIRE(ks->finished, BBK_ERR_ARG, "bbk_kmerstats_write: call bbk_kmerstats_finish after the last push");
        write_kmstat(ctx, "bbk_kmerstats_write", path, ks, nullptr, 0);
    });
}

int bbk_kmerstats_load(bbk_ctx *ctx, const bbk_kmerset *set, const char *path, bbk_kmerstats **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && set && path && out, BBK_ERR_ARG, "bbk_kmerstats_load: NULL argument");
        auto ks = ks_new("bbk_kmerstats_load", ctx, set);
        const unsigned qw = ks->qual_words;
        const size_t rsz = kmstat_record_bytes(qw);
        raw_vector<uint64_t> buf;  // a record is a whole number of 64-bit words
        read_u64_file(path, "bbk_kmerstats_load", buf);
        BBK_REQUIRE(buf.size() * 8 == ks->n * rsz, BBK_ERR_ARG,
                    "bbk_kmerstats_load: %s does not hold %llu records of %zu bytes (k = %u), one per k-mer of the set", path,
                    (unsigned long long)ks->n, rsz, ks->k);
        raw_vector<uint32_t> cnt(ks->n);
        raw_vector<float> tq(ks->n);
        raw_vector<uint64_t> qv(ks->n * qw);
        kmstat_unpack(reinterpret_cast<const char *>(buf.data()), qw, ks->n, cnt.data(), tq.data(), qv.data());
        upload(ctx, ks->count, cnt.data(), ks->n);
        upload(ctx, ks->total_qual, tq.data(), ks->n);
        upload(ctx, ks->qual, qv.data(), ks->n * qw);
        if (ks->n) BBK_HIP(hipStreamSynchronize(ctx->stream));  // cnt, tq and qv are on this frame
        ks->finished = ks->loaded = true;
        *out = ks.release();
    });
}

void bbk_kmerstats_free(bbk_kmerstats *ks) { delete ks; }

}  // extern "C"

// Exported for the tests only (not declared in bbk.h): adds delta to the count of k-mer `index` of the accumulators, so
// that a count of 2^31 exists without 2^31 occurrences
extern "C" int bbk_kmerstats_test_add_count(bbk_kmerstats *ks, uint64_t index, uint32_t delta) {
    return guarded([&] {
        BBK_REQUIRE(ks && index < ks->n, BBK_ERR_ARG, "bbk_kmerstats_test_add_count: bad argument");
        BBK_HIP(hipSetDevice(ks->ctx->device));
        uint64_t *slot = ks->rec.as<uint64_t>() + index * (uint64_t)(2 + ks->acc_words) + 1;
        uint64_t v = 0;
        BBK_HIP(hipMemcpyAsync(&v, slot, 8, hipMemcpyDeviceToHost, ks->ctx->stream));
        BBK_HIP(hipStreamSynchronize(ks->ctx->stream));
        v = (uint32_t)((uint32_t)v + delta);
        BBK_HIP(hipMemcpyAsync(slot, &v, 8, hipMemcpyHostToDevice, ks->ctx->stream));
        BBK_HIP(hipStreamSynchronize(ks->ctx->stream));
        ks->finished = false;
    });
}
