// kmerfilter.hip -- the minimum-multiplicity filter of a count: the accumulated distinct
// canonical records (Key<W>, u32 multiplicity) go in, those whose exported multiplicity reaches `min_count` come out, in
// their order.
//
// Replaces the filtered index build of BayesHammer's count_filter_singletons (KMerDataCounter::BuildKMerIndex,
// projects/hammer/kmer_data.cpp:280-335): there every k-mer and its reverse complement are added to a counting quotient
// filter first and only k-mers it has seen more than once enter the index.  The filter is approximate -- it may
// over-count and let a singleton through; this one is exact on the multiplicities the count carries anyway (the
// divergence is recorded in DESIGN.md 4.3k).
//
// The rule is stated on the multiplicity the finished set reports.  That is the canonical record's count, except for a
// k-mer equal to its own reverse complement (even k) in a both-strand set: both strands of every occurrence are the same
// k-mer, the expansion merges them and its count doubles (count.hip: expand_both_strands), wrapping modulo 2^32 like
// every multiplicity.  `self_rc_doubles` asks for that reading.
// An ordered selection (select.h: no atomics, the same input gives the same bytes) with the rule, McRule, stated once:
//   the count            select_count over McKept, in mask form: the four counts of a lane in one 16-byte load; with
//                        self_rc_doubles also its keys (timing family "k_mc_count")
//   the dropped self-complementary records   a second, count-only selection under self_rc_doubles ("k_mc_self_rc")
//   k_mc_write           the site's own write kernel over the selection's tile bases: counts AND keys of a lane loaded up
//                        front (16-byte loads), the same McRule, the kept records stored at their ranks.  Through
//                        select_write, whose emitter loads the key of a kept record only once the mask is known, the
//                        write measured 21 % slower (profiles/select/README.md), so the kernel stays
#include <hip/hip_runtime.h>

#include "accum.h"
#include "bbk_internal.h"
#include "kmer_ops.h"
#include "select.h"

namespace bbk {

// The keys of records [p, p + 4): 2 W loads of 16 bytes where all four exist (4 W words, 32 W bytes from an aligned p)
template <int W>
__device__ inline void mc_load_keys(const Key<W> *__restrict__ keys, uint64_t n, uint64_t p, Key<W> x[kSelLane]) {
    if (p + kSelLane <= n) {
        const uint4 *q = reinterpret_cast<const uint4 *>(keys + p);
        uint4 v[2 * W];
#pragma unroll
        for (int i = 0; i < 2 * W; ++i) v[i] = q[i];
#pragma unroll
        for (uint32_t b = 0; b < kSelLane; ++b)
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const int j = (int)b * W + i;
                const uint4 t = v[j >> 1];
                x[b].w[i] = (j & 1) ? ((uint64_t)t.w << 32 | t.z) : ((uint64_t)t.y << 32 | t.x);
            }
    } else {
#pragma unroll
        for (uint32_t b = 0; b < kSelLane; ++b) {
#pragma unroll
            for (int i = 0; i < W; ++i) x[b].w[i] = 0;
            if (p + b < n) x[b] = key_load<W>(&keys[p + b]);
        }
    }
}

// The rule, stated once
template <int W>
struct McRule {
    const Key<W> *__restrict__ keys;
    const uint32_t *__restrict__ counts;
    uint32_t min_count;
    int self_rc_doubles, k;
    // The kept records among [p, p + 4) as a mask, from their counts c and (read only with self_rc_doubles) their keys x;
    // *own_rc: those that are their own reverse complement (none without self_rc_doubles)
    __device__ uint32_t decide(const uint32_t c[kSelLane], const Key<W> x[kSelLane], uint64_t p, uint64_t n,
                               uint32_t *own_rc) const {
        uint32_t m = 0, o = 0;
#pragma unroll
        for (uint32_t b = 0; b < kSelLane; ++b) {
            const bool own = self_rc_doubles && key_eq<W>(kmer_rc<W>(x[b], k), x[b]);
            const uint32_t mult = own ? c[b] + c[b] : c[b];  // (u32: wraps as the merged count does)
            m |= (p + b < n && mult >= min_count ? 1u : 0u) << b;
            o |= (p + b < n && own ? 1u : 0u) << b;
        }
        *own_rc = o;
        return m;
    }
    // ... loading what the rule reads: the plain rule reads no key
    __device__ uint32_t kept(uint64_t p, uint64_t n, uint32_t *own_rc) const {
        uint32_t c[kSelLane];
        Key<W> x[kSelLane];
        load4_u32(counts, n, p, c);
        if (self_rc_doubles) mc_load_keys<W>(keys, n, p, x);  // (uniform)
        return decide(c, x, p, n, own_rc);
    }
};

template <int W>
struct McKept {
    McRule<W> rule;
    __device__ uint32_t operator()(uint64_t p, uint64_t n) const {
        uint32_t own;
        return rule.kept(p, n, &own);
    }
};

// own reverse complement and not kept
template <int W>
struct McDroppedSelfRc {
    McRule<W> rule;
    __device__ uint32_t operator()(uint64_t p, uint64_t n) const {
        uint32_t own;
        const uint32_t kept = rule.kept(p, n, &own);
        return own & ~kept;
    }
};

// base: the tile bases of the selection on McKept{rule}.  n_kept: its total, the records the outputs hold
template <int W>
__global__ __launch_bounds__(256) void k_mc_write(McRule<W> rule, uint64_t n, uint64_t n_tiles,
                                                 const uint64_t *__restrict__ base, uint64_t n_kept,
                                                 Key<W> *__restrict__ out_keys, uint32_t *__restrict__ out_counts) {
    const uint64_t tile = (BBK_GID()) >> 6;
    if (tile >= n_tiles) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t p = tile * kSelTile + (uint64_t)lane * kSelLane;
    uint32_t c[kSelLane];
    Key<W> x[kSelLane];
    load4_u32(rule.counts, n, p, c);
    mc_load_keys<W>(rule.keys, n, p, x);
    uint32_t own;
    const uint32_t m = rule.decide(c, x, p, n, &own);
    uint32_t below, all;
    wave_sums<3>((uint32_t)__popc(m), lane, &below, &all);
    uint64_t j = base[tile] + below;
#pragma unroll
    for (uint32_t b = 0; b < kSelLane; ++b) {
        if (((m >> b) & 1u) && j < n_kept) {
            key_store<W>(&out_keys[j], x[b]);
            out_counts[j] = c[b];
            ++j;
        }
    }
}

uint64_t filter_min_count(bbk_ctx *ctx, unsigned k, bool self_rc_doubles, uint32_t min_count, DevBuf &keys, DevBuf &vals,
                          uint64_t n, uint64_t *dropped_self_rc) {
    *dropped_self_rc = 0;
    if (n == 0) return 0;
    const int W = (int)words_of(k);
    const size_t rec = (size_t)W * 8;
    uint64_t n_kept = n;
    dispatch_w((unsigned)W, [&](auto w) {
        constexpr int W_ = decltype(w)::value;
        const McRule<W_> rule{(const Key<W_> *)keys.p, vals.as<uint32_t>(), min_count, self_rc_doubles ? 1 : 0, (int)k};
        const Selection sel = select_count(ctx, "k_mc_count", n, McKept<W_>{rule});
        n_kept = sel.kept;
        if (self_rc_doubles) *dropped_self_rc = select_count(ctx, "k_mc_self_rc", n, McDroppedSelfRc<W_>{rule}).kept;
        if (n_kept == n) return;  // nothing to drop: the records stay where they are
        DevBuf ok(n_kept * rec + 16), ov(n_kept * 4 + 16);
        if (n_kept) {
            launch_items_timed(ctx, "k_mc_write", k_mc_write<W_>, sel.n_tiles * 64, rule, n, sel.n_tiles,
                               sel.base.as<uint64_t>(), n_kept, (Key<W_> *)ok.p, ov.as<uint32_t>());
            stream_wait(ctx);  // the tile bases go back to the pool with this frame
        }
        keys = std::move(ok);
        vals = std::move(ov);
    });
    return n_kept;
}

}  // namespace bbk
