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
// Kernels (an order-preserving compaction, no atomics: the same input gives the same bytes):
//   k_mc_count   one wavefront per tile of 256 records, four per lane: the four counts in one 16-byte load, the kept
//                records of a lane as a 4-bit mask, of the tile as three ballots (the bits of the lanes' totals); with
//                self_rc_doubles also the keys, and the dropped self-complementary records of the tile
//   k_mc_write   the same tiles behind one scan of their totals: the rank of a lane's first kept record from the same
//                ballots below the lane, keys (16-byte loads) and counts stored at their ranks
#include <hip/hip_runtime.h>

#include "accum.h"
#include "bbk_internal.h"
#include "kmer_ops.h"

namespace bbk {

constexpr uint32_t kMcLane = 4, kMcTile = 64 * kMcLane;  // records of a lane, of a wavefront's tile

// The counts of records [p, p + 4): one load where all four exist (p is a multiple of 4: 16-byte aligned), 0 beyond n
__device__ inline void mc_load_counts(const uint32_t *__restrict__ counts, uint64_t n, uint64_t p, uint32_t c[kMcLane]) {
    if (p + kMcLane <= n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(counts + p);
        c[0] = v.x;
        c[1] = v.y;
        c[2] = v.z;
        c[3] = v.w;
    } else {
#pragma unroll
        for (uint32_t b = 0; b < kMcLane; ++b) c[b] = p + b < n ? counts[p + b] : 0u;
    }
}

// The keys of records [p, p + 4): 2 W loads of 16 bytes where all four exist (4 W words, 32 W bytes from an aligned p)
template <int W>
__device__ inline void mc_load_keys(const Key<W> *__restrict__ keys, uint64_t n, uint64_t p, Key<W> x[kMcLane]) {
    if (p + kMcLane <= n) {
        const uint4 *q = reinterpret_cast<const uint4 *>(keys + p);
        uint4 v[2 * W];
#pragma unroll
        for (int i = 0; i < 2 * W; ++i) v[i] = q[i];
#pragma unroll
        for (uint32_t b = 0; b < kMcLane; ++b)
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const int j = (int)b * W + i;
                const uint4 t = v[j >> 1];
                x[b].w[i] = (j & 1) ? ((uint64_t)t.w << 32 | t.z) : ((uint64_t)t.y << 32 | t.x);
            }
    } else {
#pragma unroll
        for (uint32_t b = 0; b < kMcLane; ++b) {
#pragma unroll
            for (int i = 0; i < W; ++i) x[b].w[i] = 0;
            if (p + b < n) x[b] = key_load<W>(&keys[p + b]);
        }
    }
}

// The kept records among [p, p + 4) as a mask; *self_rc: the dropped ones that are their own reverse complement
template <int W>
__device__ inline uint32_t mc_kept(const uint32_t c[kMcLane], const Key<W> x[kMcLane], uint64_t n, uint64_t p,
                                   uint32_t min_count, bool self_rc_doubles, int k, uint32_t *self_rc) {
    uint32_t m = 0, s = 0;
#pragma unroll
    for (uint32_t b = 0; b < kMcLane; ++b) {
        const bool own = self_rc_doubles && key_eq<W>(kmer_rc<W>(x[b], k), x[b]);
        const uint32_t mult = own ? c[b] + c[b] : c[b];  // (u32: wraps as the merged count does)
        const bool keep = p + b < n && mult >= min_count;
        m |= (keep ? 1u : 0u) << b;
        s |= (p + b < n && own && !keep ? 1u : 0u) << b;
    }
    *self_rc = s;
    return m;
}

// The totals t (0..4) of the lanes of a wavefront: their sum over the lanes below this one, and over all lanes
__device__ inline void mc_wave_sums(uint32_t t, uint32_t lane, uint32_t *below, uint32_t *all) {
    const uint64_t lt = (1ull << lane) - 1ull;
    uint32_t b = 0, a = 0;
#pragma unroll
    for (uint32_t bit = 0; bit < 3; ++bit) {
        const uint64_t m = __ballot((t >> bit) & 1u);
        b += (uint32_t)__popcll(m & lt) << bit;
        a += (uint32_t)__popcll(m) << bit;
    }
    *below = b;
    *all = a;
}

// kept[tile]: the records of the tile that stay; self_rc[tile] (with self_rc_doubles): its dropped self-complementary ones
template <int W>
__global__ __launch_bounds__(256) void k_mc_count(const Key<W> *__restrict__ keys, const uint32_t *__restrict__ counts,
                                                 uint64_t n, uint64_t n_tiles, uint32_t min_count, int self_rc_doubles,
                                                 int k, uint64_t *__restrict__ kept, uint64_t *__restrict__ self_rc) {
    const uint64_t tile = (BBK_GID()) >> 6;
    if (tile >= n_tiles) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t p = tile * kMcTile + (uint64_t)lane * kMcLane;
    uint32_t c[kMcLane];
    Key<W> x[kMcLane];
    mc_load_counts(counts, n, p, c);
    if (self_rc_doubles) mc_load_keys<W>(keys, n, p, x);  // (uniform) the plain rule reads no key
    else
#pragma unroll
        for (uint32_t b = 0; b < kMcLane; ++b)
#pragma unroll
            for (int i = 0; i < W; ++i) x[b].w[i] = 0;
    uint32_t s;
    const uint32_t m = mc_kept<W>(c, x, n, p, min_count, self_rc_doubles != 0, k, &s);
    uint32_t below, all;
    mc_wave_sums((uint32_t)__popc(m), lane, &below, &all);
    if (lane == 0) kept[tile] = all;
    if (self_rc_doubles) {
        mc_wave_sums((uint32_t)__popc(s), lane, &below, &all);
        if (lane == 0) self_rc[tile] = all;
    }
}

// base: the scanned totals of k_mc_count.  n_kept: their sum, the records the outputs hold
template <int W>
__global__ __launch_bounds__(256) void k_mc_write(const Key<W> *__restrict__ keys, const uint32_t *__restrict__ counts,
                                                 uint64_t n, uint64_t n_tiles, uint32_t min_count, int self_rc_doubles,
                                                 int k, const uint64_t *__restrict__ base, uint64_t n_kept,
                                                 Key<W> *__restrict__ out_keys, uint32_t *__restrict__ out_counts) {
    const uint64_t tile = (BBK_GID()) >> 6;
    if (tile >= n_tiles) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t p = tile * kMcTile + (uint64_t)lane * kMcLane;
    uint32_t c[kMcLane];
    Key<W> x[kMcLane];
    mc_load_counts(counts, n, p, c);
    mc_load_keys<W>(keys, n, p, x);
    uint32_t s;
    const uint32_t m = mc_kept<W>(c, x, n, p, min_count, self_rc_doubles != 0, k, &s);
    uint32_t below, all;
    mc_wave_sums((uint32_t)__popc(m), lane, &below, &all);
    uint64_t j = base[tile] + below;
#pragma unroll
    for (uint32_t b = 0; b < kMcLane; ++b) {
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
    const uint64_t n_tiles = (n + kMcTile - 1) / kMcTile;
    DevBuf d_kept((n_tiles + 1) * 8), d_self((n_tiles + 1) * 8);
    const int own = self_rc_doubles ? 1 : 0;
    dispatch_w((unsigned)W, [&](auto w) {
        constexpr int W_ = decltype(w)::value;
        launch_items_timed(ctx, "k_mc_count", k_mc_count<W_>, n_tiles * 64, (const Key<W_> *)keys.p, vals.as<uint32_t>(), n,
                           n_tiles, min_count, own, (int)k, d_kept.as<uint64_t>(), d_self.as<uint64_t>());
    });
    uint64_t n_kept = 0;
    if (self_rc_doubles) {
        uint64_t totals[2] = {0, 0};
        exclusive_scan2_u64(ctx, d_kept.as<uint64_t>(), d_kept.as<uint64_t>(), d_self.as<uint64_t>(), d_self.as<uint64_t>(),
                            n_tiles, totals);
        n_kept = totals[0];
        *dropped_self_rc = totals[1];
    } else {
        n_kept = exclusive_scan_u64(ctx, d_kept.as<uint64_t>(), d_kept.as<uint64_t>(), n_tiles);
    }
    BBK_REQUIRE(n_kept <= n, BBK_ERR_INTERNAL, "minimum-count filter: %llu of %llu records kept",
                (unsigned long long)n_kept, (unsigned long long)n);
    if (n_kept == n) return n;  // nothing to drop: the records stay where they are
    DevBuf ok(n_kept * rec + 16), ov(n_kept * 4 + 16);
    if (n_kept) {
        dispatch_w((unsigned)W, [&](auto w) {
            constexpr int W_ = decltype(w)::value;
            launch_items_timed(ctx, "k_mc_write", k_mc_write<W_>, n_tiles * 64, (const Key<W_> *)keys.p, vals.as<uint32_t>(),
                               n, n_tiles, min_count, own, (int)k, d_kept.as<uint64_t>(), n_kept, (Key<W_> *)ok.p,
                               ov.as<uint32_t>());
        });
        stream_wait(ctx);  // the tile bases go back to the pool with this frame
    }
    keys = std::move(ok);
    vals = std::move(ov);
    return n_kept;
}

}  // namespace bbk
