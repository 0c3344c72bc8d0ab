// tipclip.hip -- early tip clipping on the extension index.
//
// Replaces EarlyTipClipperProcessor::ClipTips + RemoveInconsistentForwardLinks
// (common/assembly_graph/construction/early_simplification.hpp:20-35,37-160), the step the main SPAdes
// pipeline runs between the extension index and the unitig compaction.  Mask-only work:
//   for every stored k-mer and its reverse complement with >= 2 outgoing edges: walk every outgoing branch
//   (FindForward :107-118: unique-in/unique-out k-mers up to length_bound, ending in a dead end = a tip); tips
//   shorter than the junction's longest outgoing branch (a branch that is not a tip counts as infinitely long) are
//   isolated (mask := 0); afterwards the junctions that lost a tip drop their links to the isolated k-mers.
// The reference does this with OpenMP threads modifying the masks in place.  The k-mers of a tip are reachable from
// exactly one junction in one orientation (unique incoming edge), so isolating them cannot change what any other walk
// sees; here the marks are therefore collected first (k_tips_find, masks read-only), applied (k_tips_apply), and the
// links fixed against that snapshot (k_tips_links).  Parity is checked against the sequential CPU oracle.
#include <hip/hip_runtime.h>

#include <memory>

#include "bbk_internal.h"
#include "extwalk.h"
#include "kmer_ops.h"

namespace bbk {

// FindForward (:107-118): size of the tip that starts at `start`, 0 if the branch is not a tip.  MARK: set the flag
// of every k-mer of the tip (only called for branches already known to be tips).
template <int W, bool MARK>
__device__ inline uint32_t tip_walk(const TipTable &T, Key<W> cur, uint32_t length_bound, uint8_t *flag) {
    uint32_t n = 0;
    Oriented<W> o;
    uint32_t m = 0;
    for (;;) {
        if (!tt_orient<W>(T, cur, o)) return 0;
        m = tt_mask<W>(T.masks, o);
        if (!(n < length_bound && unique4(m >> 4) && unique4(m))) break;
        if (MARK) flag[o.idx] = 1;
        ++n;
        cur = kmer_shl<W>(cur, T.k, (uint32_t)__builtin_ctz(m & 15u));
    }
    if (MARK) flag[o.idx] = 1;
    ++n;
    if (!unique4(m >> 4) || (m & 15u) != 0) return 0;  // branching or too long
    return n;
}

// one thread per (stored k-mer, orientation)
template <int W>
__global__ __launch_bounds__(256) void k_tips_find(TipTable T, uint32_t length_bound, uint8_t *__restrict__ flag,
                                                  uint8_t *__restrict__ tipped, unsigned long long *__restrict__ removed) {
    const uint64_t t = BBK_GID();
    if (t >= 2 * T.n) return;
    const uint64_t i = t >> 1;
    const bool rc_side = t & 1;
    const Key<W> canon = key_load<W>(&reinterpret_cast<const Key<W> *>(T.keys)[i]);
    const Key<W> key = key_select<W>(rc_side, kmer_rc<W>(canon, T.k), canon);
    Oriented<W> kh;
    if (!tt_orient<W>(T, key, kh)) return;
    const uint32_t mask = tt_mask<W>(T.masks, kh);
    if (__builtin_popcount(mask & 15u) < 2) return;
    // RemoveForward (:136-149)
    uint32_t len[4] = {0, 0, 0, 0};
    uint32_t mx = 0;
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) {
        if (!(mask & (1u << c))) continue;
        len[c] = tip_walk<W, false>(T, kmer_shl<W>(key, T.k, c), length_bound, nullptr);
        const uint32_t l = len[c] ? len[c] : 0xFFFFFFFFu;
        mx = l > mx ? l : mx;
    }
    uint32_t rm = 0;
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) {
        if (len[c] && len[c] < mx) {
            (void)tip_walk<W, true>(T, kmer_shl<W>(key, T.k, c), length_bound, flag);
            rm += len[c];
        }
    }
    if (rm) {
        tipped[t] = 1;
        atomicAdd(removed, (unsigned long long)rm);
    }
}

// k_tips_apply and k_tips_links (RemoveInconsistentForwardLinks): extwalk.h, shared with atclip.hip

template <int W>
static void clip_tips_impl(bbk_ctx *ctx, bbk_extindex *x, uint32_t length_bound, uint64_t *removed, uint64_t *links) {
    DevBuf flag(x->n + 16), tipped(2 * x->n + 16), m2(x->n + 16), m3(x->n + 16), ctr(16);
    BBK_HIP(hipMemsetAsync(flag.p, 0, x->n + 16, ctx->stream));
    BBK_HIP(hipMemsetAsync(tipped.p, 0, 2 * x->n + 16, ctx->stream));
    BBK_HIP(hipMemsetAsync(ctr.p, 0, 16, ctx->stream));
    TipTable T = tip_table(x);
    {
        KernelTimer t(ctx, "tip_find", 0.0);
        launch_items(ctx, "k_tips_find", k_tips_find<W>, 2 * x->n, T, length_bound, flag.as<uint8_t>(),
                     tipped.as<uint8_t>(), ctr.as<unsigned long long>());
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
    if (removed) *removed = h[0];
    if (links) *links = h[1];
}

}  // namespace bbk

using namespace bbk;

extern "C" int bbk_extindex_clip_tips(bbk_ctx *ctx, bbk_extindex *x, uint32_t length_bound, uint64_t *removed_kmers,
                                      uint64_t *removed_links) {
    return guarded([&] {
        BBK_REQUIRE(ctx && x, BBK_ERR_ARG, "bbk_extindex_clip_tips: NULL argument");
        BBK_REQUIRE(x->n < (1ull << 37), BBK_ERR_ARG, "bbk_extindex_clip_tips: %llu k-mers exceed the launch grid",
                    (unsigned long long)x->n);
        BBK_HIP(hipSetDevice(ctx->device));
        if (removed_kmers) *removed_kmers = 0;
        if (removed_links) *removed_links = 0;
        if (x->n == 0) return;
        dispatch_w(x->W, [&](auto w) {
            clip_tips_impl<decltype(w)::value>(ctx, x, length_bound, removed_kmers, removed_links);
        });
    });
}
