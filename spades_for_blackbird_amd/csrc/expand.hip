// expand.hip -- BayesHammer's iterative expansion of the solid k-mers.
//
// Replaces Expander::operator() (projects/hammer/expander.cpp:20-70) and the loop around it
// (projects/hammer/main.cpp:194-222): a read that is covered end to end by good k-mers makes all of its k-mers good, and
// that is repeated until an iteration adds fewer than 10 k-mers or 25 iterations have run.  The reference marks in place
// with six threads, so what an iteration adds -- and, through the stop rule, the final bits -- depends on read order and
// thread timing.  Here an iteration is a SNAPSHOT ROUND over two generations of the good bytes:
//   G_r  (`cur`)  is only read, G_{r+1} (`next`) only written, and next == cur when the round begins;
//   a read is solid in round r when start 0 and start nk - 1 are in the set and good in G_r and no k or more starts in a
//     row are non-good (a start whose k-mer is not in the set is non-good): covered_by_solid all true (:30-51);
//   G_{r+1} = G_r with the forward k-mers, present in the set, of every solid read (:53-67; no reverse complement is
//     looked up, :36);
//   changed_r = |G_{r+1} \ G_r|, counted over the bytes, so a k-mer that several reads mark counts once.
// The result is the same bytes for any order and batching of the reads.  Which reads can take part, and that one such
// read is one stretch, is the host's business (host/hammer_reads.hpp: expander_candidate).
// Kernels: k_ex_round, one wavefront per read, lanes over its k-mer starts in chunks of 64 (the shape of
// readfilter.hip: k_median_filter and kmerstat.hip: k_ks_accum): one table_find<1> and one byte of G_r per start, the
// good starts of a chunk as one 64-bit ballot, the solid test on those masks with the run of non-good starts carried
// from chunk to chunk; k_ex_changed, the count of next & ~cur over the n bytes, which also makes cur = next.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>

#include "hammer.h"
#include "kmer_ops.h"

namespace bbk {

constexpr uint32_t kExNone = 0xFFFFFFFFu;  // nothing to mark at this start (indices stay below 2^32 - 2)
constexpr int kExCached = 4;               // chunks whose lookups stay in registers for the marking: 256 starts

// whether z holds k or more set bits in a row, k in 1..32
__device__ inline bool ex_has_run(uint64_t z, uint32_t k) {
    uint32_t s = 1;
    for (; 2 * s <= k; s *= 2) z &= z >> s;  // bit i: a run of s from i
    if (k > s) z &= z >> (k - s);
    return z != 0;
}

// the solid test over the chunks seen so far
struct ExState {
    uint32_t run = 0;  // non-good starts at the end of what was seen
    bool ok = true, all = true;
    // mask: the good starts of a chunk of m starts (bits m.. are 0)
    __device__ void take(uint64_t mask, uint32_t m, bool first, bool last, uint32_t k) {
        const uint64_t valid = m == 64 ? ~0ull : (1ull << m) - 1ull;
        const uint64_t zeros = ~mask & valid;
        if (first && !(mask & 1ull)) ok = false;
        if (last && !((mask >> (m - 1)) & 1ull)) ok = false;
        if (zeros) all = false;
        if (mask == 0) {
            run += m;
        } else {
            if (run + (uint32_t)__builtin_ctzll(mask) >= k) ok = false;  // the run that straddles the chunk boundary
            run = m - 1u - (63u - (uint32_t)__builtin_clzll(mask));
        }
        if (run >= k || ex_has_run(zeros, k)) ok = false;
    }
};

// the start p of a read: the index of its k-mer when it is in the set and not good (kExNone otherwise); *good: in the set
// and good
__device__ inline uint32_t ex_lookup(const uint64_t *__restrict__ rw, uint32_t p, int k, const Key<1> *__restrict__ keys,
                                     const PrefixTable &P, const uint8_t *__restrict__ cur, bool *good) {
    const uint64_t i = table_find<1>(keys, P, kmer_extract<1>(rw, p, k));
    *good = i != kNotFound && cur[i] != 0;
    return i != kNotFound && !*good ? (uint32_t)i : kExNone;
}

// one wavefront per read, lanes over its k-mer starts in chunks of 64.  status (may be null): 0 not solid, 1 solid,
// 2 every start already good
__global__ __launch_bounds__(256) void k_ex_round(const uint64_t *__restrict__ words, const uint64_t *__restrict__ woff,
                                                 const uint32_t *__restrict__ len, uint64_t n_reads, int k,
                                                 const Key<1> *__restrict__ keys, PrefixTable P,
                                                 const uint8_t *__restrict__ cur, uint8_t *__restrict__ next,
                                                 uint8_t *__restrict__ status) {
    const uint64_t r = (BBK_GID()) >> 6;
    if (r >= n_reads) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t L = len[r];
    if (L < (uint32_t)k) {  // sz < hammer::K (:27-28)
        if (status && lane == 0) status[r] = 0;
        return;
    }
    const uint32_t nk = L - (uint32_t)k + 1u;
    const uint64_t *rw = words + woff[r];
    ExState st;
    uint32_t todo[kExCached];
#pragma unroll
    for (int c = 0; c < kExCached; ++c) {
        todo[c] = kExNone;
        const uint32_t base = 64u * (uint32_t)c;
        if (base < nk && st.ok) {  // once a chunk has failed the read is not solid whatever follows: the rest is skipped
            const uint32_t m = nk - base < 64u ? nk - base : 64u;
            bool g = false;
            if (lane < m) todo[c] = ex_lookup(rw, base + lane, k, keys, P, cur, &g);
            st.take(__ballot(g), m, c == 0, base + m == nk, (uint32_t)k);
        }
    }
    for (uint32_t base = 64u * kExCached; base < nk && st.ok; base += 64u) {
        const uint32_t m = nk - base < 64u ? nk - base : 64u;
        bool g = false;
        if (lane < m) (void)ex_lookup(rw, base + lane, k, keys, P, cur, &g);
        st.take(__ballot(g), m, false, base + m == nk, (uint32_t)k);
    }
    if (status && lane == 0) status[r] = st.ok ? (st.all ? 2 : 1) : 0;
    if (!st.ok || st.all) return;
    // every writer stores the same value: plain byte stores, no atomics
#pragma unroll
    for (int c = 0; c < kExCached; ++c)
        if (todo[c] != kExNone) next[todo[c]] = 1;
    for (uint32_t base = 64u * kExCached + lane; base < nk; base += 64u) {  // beyond the cached chunks: looked up again
        bool g = false;
        const uint32_t i = ex_lookup(rw, base, k, keys, P, cur, &g);
        if (i != kExNone) next[i] = 1;
    }
}

// 16 bytes per lane: *changed += the bytes set in next and not in cur, then cur = next.  Bytes are 0 or 1, so the set
// bits of a word are its set bytes.
__global__ __launch_bounds__(256) void k_ex_changed(uint4 *__restrict__ cur, const uint4 *__restrict__ next, uint64_t nvec,
                                                   unsigned long long *__restrict__ changed) {
    const uint64_t i = BBK_GID();
    uint32_t c = 0;
    if (i < nvec) {
        const uint4 a = cur[i], b = next[i];
        c = (uint32_t)(__popc(b.x & ~a.x) + __popc(b.y & ~a.y) + __popc(b.z & ~a.z) + __popc(b.w & ~a.w));
        cur[i] = b;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(changed, (unsigned long long)c);
}

static uint64_t ex_vectors(uint64_t n) { return (n + 15) / 16; }

static void ex_launch_round(bbk_expander *e, const bbk_reads *reads, uint8_t *d_status) {
    launch_items_timed(e->ctx, "k_ex_round", k_ex_round, reads->n * 64, reads->d_words, reads->d_woff, reads->d_len, reads->n,
                       (int)e->k, e->set->keys.as<Key<1>>(), e->prefix.table(), e->cur.as<uint8_t>(), e->next.as<uint8_t>(),
                       d_status);
}

// changed_r, and G_r <- G_{r+1}: the one host wait of a round
static uint64_t ex_close_round(bbk_expander *e) {
    if (e->n == 0) return 0;
    bbk_ctx *ctx = e->ctx;
    BBK_HIP(hipMemsetAsync(e->changed.p, 0, 8, ctx->stream));
    const uint64_t nvec = ex_vectors(e->n);
    launch_items_timed(ctx, "k_ex_changed", k_ex_changed, nvec, e->cur.as<uint4>(), e->next.as<uint4>(), nvec,
                       e->changed.as<unsigned long long>());
    uint64_t c = 0;
    d2h_sync(ctx, &c, e->changed.p, 8);
    e->good += c;
    return c;
}

// the handle over a set the stage accepts, its lookup index, both generations zeroed; `next` is filled by the caller and
// ex_close_round then counts the good k-mers and copies them into `cur`
static std::unique_ptr<bbk_expander> ex_new(const char *fn, bbk_ctx *ctx, const bbk_kmerset *set) {
    BBK_REQUIRE(!(set->flags & BBK_CANONICAL), BBK_ERR_ARG,
                "%s: needs a both-strand k-mer set (bbk_count(BBK_BOTH_STRANDS)): this one is canonical only (BBK_CANONICAL)", fn);
    require_hammer_set(fn, set);
    BBK_HIP(hipSetDevice(ctx->device));
    auto e = std::make_unique<bbk_expander>();
    e->ctx = ctx;
    e->set = set;
    e->k = set->k;
    e->n = set->n;
    const size_t bytes = ex_vectors(e->n) * 16;
    e->cur.alloc(bytes);
    e->next.alloc(bytes);
    e->changed.alloc(8);
    if (e->n) {
        e->prefix.build(ctx, set->keys.as<uint64_t>(), 1, set->k, set->n);
        BBK_HIP(hipMemsetAsync(e->cur.p, 0, bytes, ctx->stream));
        BBK_HIP(hipMemsetAsync(e->next.p, 0, bytes, ctx->stream));
    }
    return e;
}

}  // namespace bbk

using namespace bbk;

extern "C" {

int bbk_expander_from_subclusters(bbk_ctx *ctx, const bbk_kmerset *set, const bbk_subclusters *sc, bbk_expander **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && set && sc && out, BBK_ERR_ARG, "bbk_expander_from_subclusters: NULL argument");
        BBK_REQUIRE(sc->n == set->n && sc->k == set->k, BBK_ERR_ARG,
                    "bbk_expander_from_subclusters: the set has %llu k-mers of size %u, the subclusters were made for %llu of "
                    "size %u",
                    (unsigned long long)set->n, set->k, (unsigned long long)sc->n, sc->k);
        auto e = ex_new("bbk_expander_from_subclusters", ctx, set);
        if (e->n) BBK_HIP(copy_async(e->next.p, sc->good.p, e->n, hipMemcpyDeviceToDevice, ctx->stream));
        ex_close_round(e.get());
        *out = e.release();
    });
}

int bbk_expander_from_host(bbk_ctx *ctx, const bbk_kmerset *set, const uint8_t *h_good, bbk_expander **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && set && out && (h_good || set->n == 0), BBK_ERR_ARG, "bbk_expander_from_host: NULL argument");
        for (uint64_t i = 0; i < set->n; ++i)
            BBK_REQUIRE(h_good[i] <= 1, BBK_ERR_ARG, "bbk_expander_from_host: byte %llu is %u: a good bit is 0 or 1",
                        (unsigned long long)i, (unsigned)h_good[i]);
        auto e = ex_new("bbk_expander_from_host", ctx, set);
        if (e->n) BBK_HIP(hipMemcpyAsync(e->next.p, h_good, e->n, hipMemcpyHostToDevice, ctx->stream));
        ex_close_round(e.get());  // waits: h_good is the caller's
        *out = e.release();
    });
}

int bbk_expander_round_begin(bbk_expander *e) {
    return guarded([&] {
        BBK_REQUIRE(e, BBK_ERR_ARG, "bbk_expander_round_begin: NULL argument");
        BBK_REQUIRE(!e->in_round, BBK_ERR_ARG, "bbk_expander_round_begin: a round is open: call bbk_expander_round_end first");
        e->in_round = true;  // next == cur already: ex_close_round left them equal
    });
}

int bbk_expander_push(bbk_expander *e, const bbk_reads *reads, uint8_t *h_status) {
    return guarded([&] {
        BBK_REQUIRE(e && reads, BBK_ERR_ARG, "bbk_expander_push: NULL argument");
        BBK_REQUIRE(e->in_round, BBK_ERR_ARG, "bbk_expander_push: no round is open: call bbk_expander_round_begin first");
        if (reads->n == 0) return;
        bbk_ctx *ctx = e->ctx;
        BBK_HIP(hipSetDevice(ctx->device));
        if (e->n == 0) {  // nothing is in the set: no read is solid
            if (h_status) memset(h_status, 0, reads->n);
            return;
        }
        if (!h_status) {
            ex_launch_round(e, reads, nullptr);
            return;
        }
        DevBuf status(reads->n);
        ex_launch_round(e, reads, status.as<uint8_t>());
        d2h_big(ctx, h_status, status.p, reads->n);
    });
}

int bbk_expander_round_end(bbk_expander *e, uint64_t *changed) {
    return guarded([&] {
        BBK_REQUIRE(e, BBK_ERR_ARG, "bbk_expander_round_end: NULL argument");
        BBK_REQUIRE(e->in_round, BBK_ERR_ARG, "bbk_expander_round_end: no round is open: call bbk_expander_round_begin first");
        BBK_HIP(hipSetDevice(e->ctx->device));
        const uint64_t c = ex_close_round(e);
        e->in_round = false;
        if (changed) *changed = c;
    });
}

int bbk_expander_run(bbk_expander *e, const bbk_reads *reads, unsigned max_rounds, uint64_t min_changed, unsigned *rounds,
                     uint64_t *h_changed) {
    return guarded([&] {
        BBK_REQUIRE(e && reads, BBK_ERR_ARG, "bbk_expander_run: NULL argument");
        BBK_REQUIRE(!e->in_round, BBK_ERR_ARG, "bbk_expander_run: a round is open: call bbk_expander_round_end first");
        BBK_REQUIRE(max_rounds > 0, BBK_ERR_ARG, "bbk_expander_run: max_rounds is 0: at least one round is needed");
        BBK_HIP(hipSetDevice(e->ctx->device));
        unsigned r = 0;
        for (;;) {  // main.cpp:198-221
            if (reads->n && e->n) ex_launch_round(e, reads, nullptr);
            const uint64_t c = ex_close_round(e);
            if (h_changed) h_changed[r] = c;
            ++r;
            if (c < min_changed || r == max_rounds) break;
        }
        if (rounds) *rounds = r;
    });
}

uint64_t bbk_expander_good(const bbk_expander *e) { return e ? e->good : 0; }

int bbk_expander_export(bbk_ctx *ctx, const bbk_expander *e, uint8_t *h_good) {
    return guarded([&] {
        BBK_REQUIRE(ctx && e && (h_good || e->n == 0), BBK_ERR_ARG, "bbk_expander_export: NULL argument");
        BBK_HIP(hipSetDevice(ctx->device));
        if (e->n) d2h_big(ctx, h_good, e->cur.p, e->n);
    });
}

int bbk_expander_store(bbk_expander *e, bbk_subclusters *sc) {
    return guarded([&] {
        BBK_REQUIRE(e && sc, BBK_ERR_ARG, "bbk_expander_store: NULL argument");
        BBK_REQUIRE(!e->in_round, BBK_ERR_ARG, "bbk_expander_store: a round is open: call bbk_expander_round_end first");
        BBK_REQUIRE(sc->n == e->n && sc->k == e->k, BBK_ERR_ARG,
                    "bbk_expander_store: the expander holds %llu k-mers of size %u, the subclusters were made for %llu of size %u",
                    (unsigned long long)e->n, e->k, (unsigned long long)sc->n, sc->k);
        bbk_ctx *ctx = e->ctx;
        BBK_HIP(hipSetDevice(ctx->device));
        if (e->n == 0) return;
        BBK_HIP(copy_async(sc->good.p, e->cur.p, e->n, hipMemcpyDeviceToDevice, ctx->stream));
        BBK_HIP(hipStreamSynchronize(ctx->stream));
    });
}

void bbk_expander_free(bbk_expander *e) { delete e; }

}  // extern "C"
