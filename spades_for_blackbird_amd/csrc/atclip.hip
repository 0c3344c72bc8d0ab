// atclip.hip -- early poly-A/T (low-complexity) clipping on the extension index.
//
// Replaces EarlyLowComplexityClipperProcessor::RemoveATEdges / RemoveATTips
// (common/assembly_graph/construction/early_simplification.hpp:163-344), which the main pipeline runs on the extension
// index before the early tip clipper (stages/construction.cpp:320-331, ratio 0.8, min_len 10, max_len 200).
//   edges: a junction k-mer s whose most frequent nucleotide fills at least k * ratio of it (math::ls, 4 ULPs) loses
//          every outgoing link to a junction (a dead end counts as one);
//   tips:  a dead end with a unique incoming edge is walked back to the first junction (at most max_len k-mers); a tip
//          of low complexity over max(|tip|, min_len) bases (the missing bases taken from the junction) is isolated and
//          the junction drops its links to it (RemoveInconsistentForwardLinks, :20-35).
// The reference runs both with OpenMP threads changing the masks in place.  Here the work is collected against a
// snapshot of the masks, applied, and the links are fixed against the applied masks (as in tipclip.hip); the result is
// that of the sequential in-place order because
//   - k is odd, so no k-mer is its own reverse complement: the two orientations of a stored k-mer are distinct walk
//     states;
//   - every tip k-mer but the dead end is a non-junction with a unique incoming and a unique outgoing edge.  A walk is
//     therefore determined by any of its k-mers, so two walks cannot share a k-mer, and a walk that reaches a k-mer of
//     another tip (in either orientation) stops at a dead start or runs past max_len, which it would also do after that
//     tip was isolated (an isolated k-mer is a junction and a dead start): isolating one tip changes no other walk;
//   - in the edge pass only junctions lose bits, and the reference collects every edge before it removes any; removing
//     a collected link clears the same two bits from whichever of its two orientations comes first.
// tests/atclip_restated.py restates the sequential order; the GPU tests compare against it.
#include <hip/hip_runtime.h>

#include <cmath>

#include "bbk_internal.h"
#include "extwalk.h"
#include "kmer_ops.h"

namespace bbk {

// math::ls (math/xmath.h:163,218-226,251-268,300-305): a < b unless the two lie within 4 ULPs of each other
__host__ __device__ inline uint64_t ulp_biased(double v) {
    const uint64_t s = __builtin_bit_cast(uint64_t, v);
    return (s >> 63) ? ~s + 1 : s | (1ull << 63);
}
__host__ __device__ inline bool math_ls(double a, double b) {
    const uint64_t x = ulp_biased(a), y = ulp_biased(b);
    return (x >= y ? x - y : y - x) > 4 && a < b;
}

// nucleotide counts of bases [lo, hi) of x, added to a/c/g/t: popcounts of the two bit planes (A = neither bit)
template <int W>
__device__ inline void count_bases(const Key<W> &x, int lo, int hi, uint32_t &a, uint32_t &c, uint32_t &g, uint32_t &t) {
#pragma unroll
    for (int i = 0; i < W; ++i) {
        const int l = min(max(lo - 32 * i, 0), 32), h = min(max(hi - 32 * i, 0), 32);
        const uint64_t below_h = h >= 32 ? ~0ull : (1ull << (2 * h)) - 1ull;
        const uint64_t below_l = l >= 32 ? ~0ull : (1ull << (2 * l)) - 1ull;
        const uint64_t sel = below_h & ~below_l & 0x5555555555555555ull;
        const uint64_t p0 = x.w[i] & sel, p1 = (x.w[i] >> 1) & sel;
        a += (uint32_t)__popcll(sel & ~(p0 | p1));
        c += (uint32_t)__popcll(p0 & ~p1);
        g += (uint32_t)__popcll(p1 & ~p0);
        t += (uint32_t)__popcll(p0 & p1);
    }
}

__device__ inline uint32_t max4(uint32_t a, uint32_t c, uint32_t g, uint32_t t) { return max(max(a, c), max(g, t)); }

template <int W>
__device__ inline uint32_t max_count(const Key<W> &x, int k) {
    uint32_t a = 0, c = 0, g = 0, t = 0;
    count_bases<W>(x, 0, k, a, c, g, t);
    return max4(a, c, g, t);
}

__device__ inline uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- RemoveATEdges (:183-257) ----------------------------------------------------------------------------------------
// One thread per (stored k-mer, orientation), masks read-only.  lc_min: the smallest maximal nucleotide count with
// !math::ls(count, k * ratio).  clear: per stored k-mer the mask bits to drop, a byte in a 32-bit word for atomicOr.
// ctr[0] = collected (s, c) pairs; ctr[1] = the reference's removed_links: 2 per distinct link.  A collected link
// s -> s<<c is also collected from its other orientation rc(s<<c) -> rc(s) exactly when s<<c is of low complexity too
// (junction(s<<c) and junction(s) hold already); each orientation then adds 1.  A link that is its own reverse
// complement (s<<c == rc(s)) is one mask bit and adds 2, as the reference's `removed_links += 2` does.
template <int W>
__global__ __launch_bounds__(256) void k_at_edges_find(TipTable T, uint32_t lc_min, uint32_t *__restrict__ clear,
                                                      unsigned long long *__restrict__ ctr) {
    const uint64_t t = BBK_GID();
    uint64_t edges = 0, links = 0;
    if (t < 2 * T.n) {
        const uint64_t i = t >> 1;
        const bool rc_side = t & 1;
        const uint32_t stored = T.masks[i];
        const uint32_t mask = rc_side ? rev8(stored) : stored;
        if (!(unique4(mask) && unique4(mask >> 4))) {  // IsJunction
            const Key<W> canon = key_load<W>(&reinterpret_cast<const Key<W> *>(T.keys)[i]);
            if (max_count<W>(canon, T.k) >= lc_min) {  // a k-mer and its reverse complement have the same maximum
                const Key<W> rc = kmer_rc<W>(canon, T.k);
                const Key<W> key = key_select<W>(rc_side, rc, canon);
                const Key<W> anti = key_select<W>(rc_side, canon, rc);
                const uint32_t first = (uint32_t)(key.w[0] & 3ull);
                for (uint32_t c = 0; c < 4; ++c) {
                    if (!(mask & (1u << c))) continue;
                    const Key<W> nk = kmer_shl<W>(key, T.k, c);
                    Oriented<W> nx;
                    if (!tt_orient<W>(T, nk, nx)) continue;
                    const uint32_t nm = tt_mask<W>(T.masks, nx);
                    if (unique4(nm) && unique4(nm >> 4)) continue;  // the edge is longer than one (k+1)-mer
                    ++edges;
                    links += (max_count<W>(nk, T.k) >= lc_min && !key_eq<W>(nk, anti)) ? 1u : 2u;
                    // DeleteOutgoing(s, c), DeleteIncoming(s << c, s[0]) on the stored bytes
                    const uint64_t j = nx.idx;
                    const uint32_t bi = rc_side ? 7u - c : c;
                    const uint32_t bj = nx.minimal ? 4u + first : 3u - first;
                    atomicOr(&clear[i >> 2], 1u << (8 * (uint32_t)(i & 3) + bi));
                    atomicOr(&clear[j >> 2], 1u << (8 * (uint32_t)(j & 3) + bj));
                }
            }
        }
    }
    edges = wave_sum(edges);
    links = wave_sum(links);
    if ((threadIdx.x & 63) == 0 && edges) {
        atomicAdd(&ctr[0], (unsigned long long)edges);
        atomicAdd(&ctr[1], (unsigned long long)links);
    }
}

__global__ void k_at_edges_apply(uint8_t *__restrict__ masks, const uint8_t *__restrict__ clear, uint64_t n) {
    const uint64_t i = BBK_GID();
    if (i >= n) return;
    const uint32_t c = clear[i];
    if (c) masks[i] = (uint8_t)(masks[i] & ~c);
}

// ---- RemoveATTips (:269-333) -----------------------------------------------------------------------------------------
// The walk of :290-294 back from the dead end `cur` (mask m, stored at idx): returns the tip size (0 when a predecessor
// is missing from the table, which a consistent index never has); x / xm = the k-mer it stopped at and its mask; a/c/g/t
// += the last base of every tip k-mer.  MARK: flag the k-mers of the tip.
template <int W, bool MARK>
__device__ inline uint32_t at_walk(const TipTable &T, Key<W> cur, uint32_t m, uint64_t idx, uint32_t max_len,
                                   Oriented<W> &x, uint32_t &xm, uint32_t &a, uint32_t &c, uint32_t &g, uint32_t &t,
                                   uint8_t *flag) {
    const uint32_t lastshift = (uint32_t)(((T.k + 31) & 31) << 1);  // base k-1 lives in word W-1
    uint32_t n = 0;
    do {
        if (MARK) flag[idx] = 1;
        ++n;
        const uint32_t b = (uint32_t)(cur.w[W - 1] >> lastshift) & 3u;
        a += b == 0;
        c += b == 1;
        g += b == 2;
        t += b == 3;
        cur = kmer_shr<W>(cur, T.k, (uint32_t)__builtin_ctz((m >> 4) & 15u));  // GetUniqueIncoming
        if (!tt_orient<W>(T, cur, x)) return 0;
        m = tt_mask<W>(T.masks, x);
        idx = x.idx;
    } while (n < max_len && unique4(m) && unique4(m >> 4));
    xm = m;
    return n;
}

// one thread per (stored k-mer, orientation), masks read-only: mark the dead ends whose tip is clipped (start[t]) and
// the orientation of its junction (tipped[2 i + side], the layout k_tips_links reads).  The k-mers of the tip are
// flagged by a second walk in k_at_tips_mark: with both walks in one kernel, hipcc evaluated the lane mask of
// the "narrow prefix table" branch of the second walk's lookups under the exec mask of the first walk's last iteration,
// so lanes that had left the first walk early took the 64-bit-entry path on a 32-bit table and read out of bounds.
template <int W>
__global__ __launch_bounds__(256) void k_at_tips_find(TipTable T, double ratio, uint32_t min_len, uint32_t max_len,
                                                     uint8_t *__restrict__ start, uint8_t *__restrict__ tipped,
                                                     unsigned long long *__restrict__ removed) {
    const uint64_t t = BBK_GID();
    uint64_t rm = 0;
    if (t < 2 * T.n) {
        const uint64_t i = t >> 1;
        const bool rc_side = t & 1;
        const uint32_t stored = T.masks[i];
        const uint32_t mask = rc_side ? rev8(stored) : stored;
        if ((mask & 15u) == 0 && unique4(mask >> 4)) {  // IsDeadEnd && CheckUniqueIncoming
            const Key<W> canon = key_load<W>(&reinterpret_cast<const Key<W> *>(T.keys)[i]);
            const Key<W> key = key_select<W>(rc_side, kmer_rc<W>(canon, T.k), canon);
            Oriented<W> x;
            uint32_t xm = 0, a = 0, c = 0, g = 0, tt = 0;
            const uint32_t n = at_walk<W, false>(T, key, mask, i, max_len, x, xm, a, c, g, tt, nullptr);
            // bail out at dead starts and where the walk stopped inside an unbranching path (:299-300)
            if (n && (xm >> 4) != 0 && !(unique4(xm) && unique4(xm >> 4))) {
                // a short tip: the complexity over min_len bases, bases k-1-i of the junction for i in [n-1, min_len)
                if (n - 1 < min_len) count_bases<W>(x.key, T.k - (int)min_len, T.k - (int)n + 1, a, c, g, tt);
                const double thr = (double)(n > min_len ? n : min_len) * ratio;
                if (!math_ls((double)max4(a, c, g, tt), thr)) {
                    start[t] = 1;
                    tipped[2 * x.idx + (x.minimal ? 0 : 1)] = 1;
                    rm = n;
                }
            }
        }
    }
    rm = wave_sum(rm);
    if ((threadIdx.x & 63) == 0 && rm) atomicAdd(removed, (unsigned long long)rm);
}

// the walk again from every start k_at_tips_find marked, flagging the k-mers of the tip (IsolateVertex, :314-316)
template <int W>
__global__ __launch_bounds__(256) void k_at_tips_mark(TipTable T, uint32_t max_len, const uint8_t *__restrict__ start,
                                                     uint8_t *__restrict__ flag) {
    const uint64_t t = BBK_GID();
    if (t >= 2 * T.n || !start[t]) return;
    const uint64_t i = t >> 1;
    const bool rc_side = t & 1;
    const uint32_t stored = T.masks[i];
    const Key<W> canon = key_load<W>(&reinterpret_cast<const Key<W> *>(T.keys)[i]);
    Oriented<W> x;
    uint32_t xm = 0, a = 0, c = 0, g = 0, tt = 0;
    (void)at_walk<W, true>(T, key_select<W>(rc_side, kmer_rc<W>(canon, T.k), canon), rc_side ? rev8(stored) : stored, i,
                           max_len, x, xm, a, c, g, tt, flag);
}

template <int W>
static void at_edges_impl(bbk_ctx *ctx, bbk_extindex *x, double ratio, uint64_t *edges, uint64_t *links) {
    uint32_t lc_min = 0;
    while (lc_min <= x->k && math_ls((double)lc_min, (double)x->k * ratio)) ++lc_min;  // k + 1: nothing qualifies
    const uint64_t nwords = (x->n + 3) / 4;
    DevBuf clear(4 * nwords + 16), ctr(16);
    BBK_HIP(hipMemsetAsync(clear.p, 0, 4 * nwords + 16, ctx->stream));
    BBK_HIP(hipMemsetAsync(ctr.p, 0, 16, ctx->stream));
    const TipTable T = tip_table(x);
    {
        KernelTimer t(ctx, "at_edges_find", (double)x->n * (1 + 8 * W));  // one read of masks + keys
        launch_items(ctx, "k_at_edges_find", k_at_edges_find<W>, 2 * x->n, T, lc_min, clear.as<uint32_t>(),
                     ctr.as<unsigned long long>());
    }
    launch_items(ctx, "k_at_edges_apply", k_at_edges_apply, x->n, x->masks.as<uint8_t>(), clear.as<uint8_t>(), x->n);
    unsigned long long h[2] = {0, 0};
    BBK_HIP(hipMemcpyAsync(h, ctr.p, 16, hipMemcpyDeviceToHost, ctx->stream));
    BBK_HIP(hipStreamSynchronize(ctx->stream));
    *edges = h[0];
    *links = h[1];
}

template <int W>
static void at_tips_impl(bbk_ctx *ctx, bbk_extindex *x, double ratio, uint32_t min_len, uint32_t max_len,
                         uint64_t *removed, uint64_t *links) {
    DevBuf start(2 * x->n + 16), flag(x->n + 16), tipped(2 * x->n + 16), m2(x->n + 16), m3(x->n + 16), ctr(16);
    BBK_HIP(hipMemsetAsync(start.p, 0, 2 * x->n + 16, ctx->stream));
    BBK_HIP(hipMemsetAsync(flag.p, 0, x->n + 16, ctx->stream));
    BBK_HIP(hipMemsetAsync(tipped.p, 0, 2 * x->n + 16, ctx->stream));
    BBK_HIP(hipMemsetAsync(ctr.p, 0, 16, ctx->stream));
    TipTable T = tip_table(x);
    {
        KernelTimer t(ctx, "at_tips_find", 0.0);  // both walks
        launch_items(ctx, "k_at_tips_find", k_at_tips_find<W>, 2 * x->n, T, ratio, min_len, max_len,
                     start.as<uint8_t>(), tipped.as<uint8_t>(), ctr.as<unsigned long long>());
        launch_items(ctx, "k_at_tips_mark", k_at_tips_mark<W>, 2 * x->n, T, max_len, start.as<uint8_t>(),
                     flag.as<uint8_t>());
    }
    launch_items(ctx, "k_tips_apply", k_tips_apply, x->n, x->masks.as<uint8_t>(), flag.as<uint8_t>(), x->n,
                 m2.as<uint8_t>());
    T.masks = m2.as<uint8_t>();
    launch_items(ctx, "k_tips_links", k_tips_links<W>, x->n, T, tipped.as<uint8_t>(), m3.as<uint8_t>(),
                 ctr.as<unsigned long long>() + 1);
    unsigned long long h[2] = {0, 0};
    BBK_HIP(hipMemcpyAsync(h, ctr.p, 16, hipMemcpyDeviceToHost, ctx->stream));
    BBK_HIP(hipStreamSynchronize(ctx->stream));
    x->masks = std::move(m3);
    *removed = h[0];
    *links = h[1];
}

// the checks both passes share
static void at_require(const char *fn, bbk_ctx *ctx, bbk_extindex *x, double ratio, const void *out1, const void *out2) {
    BBK_REQUIRE(ctx && x && out1 && out2, BBK_ERR_ARG, "%s: NULL argument", fn);
    BBK_REQUIRE(std::isfinite(ratio) && ratio > 0, BBK_ERR_ARG, "%s: ratio %g is not a finite positive number", fn, ratio);
    BBK_REQUIRE(x->k % 2 == 1, BBK_ERR_ARG, "%s: k = %u is even (a k-mer could be its own reverse complement)", fn, x->k);
    BBK_REQUIRE(x->n < (1ull << 37), BBK_ERR_ARG, "%s: %llu k-mers exceed the launch grid", fn, (unsigned long long)x->n);
}

}  // namespace bbk

using namespace bbk;

extern "C" int bbk_extindex_remove_at_edges(bbk_ctx *ctx, bbk_extindex *x, double ratio, uint64_t *removed_edges,
                                            uint64_t *removed_links) {
    return guarded([&] {
        at_require("bbk_extindex_remove_at_edges", ctx, x, ratio, removed_edges, removed_links);
        BBK_HIP(hipSetDevice(ctx->device));
        *removed_edges = 0;
        *removed_links = 0;
        if (x->n == 0) return;
        dispatch_w(x->W, [&](auto w) {
            at_edges_impl<decltype(w)::value>(ctx, x, ratio, removed_edges, removed_links);
        });
    });
}

extern "C" int bbk_extindex_remove_at_tips(bbk_ctx *ctx, bbk_extindex *x, double ratio, uint32_t min_len,
                                           uint32_t max_len, uint64_t *removed_kmers, uint64_t *clipped_links) {
    return guarded([&] {
        at_require("bbk_extindex_remove_at_tips", ctx, x, ratio, removed_kmers, clipped_links);
        BBK_REQUIRE(max_len > 0, BBK_ERR_ARG, "bbk_extindex_remove_at_tips: max_len is 0");
        BBK_REQUIRE(min_len <= x->k, BBK_ERR_ARG, "bbk_extindex_remove_at_tips: min_len %u exceeds k = %u", min_len,
                    x->k);
        BBK_HIP(hipSetDevice(ctx->device));
        *removed_kmers = 0;
        *clipped_links = 0;
        if (x->n == 0) return;
        dispatch_w(x->W, [&](auto w) {
            at_tips_impl<decltype(w)::value>(ctx, x, ratio, min_len, max_len, removed_kmers, clipped_links);
        });
    });
}
