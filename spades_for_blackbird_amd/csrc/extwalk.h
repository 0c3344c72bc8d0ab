// extwalk.h -- walking the extension index on the device: oriented lookups of k-mers and their masks, and the two
// kernels the early simplifications share (isolate flagged k-mers, drop the links that point at them).
// Used by tipclip.hip (EarlyTipClipperProcessor) and atclip.hip (EarlyLowComplexityClipperProcessor).  The kernels
// have internal linkage: every translation unit that includes this header gets its own copy.
#pragma once

#include <hip/hip_runtime.h>

#include "bbk_internal.h"
#include "kmer_ops.h"

namespace bbk {

template <int W>
struct Oriented {
    Key<W> key;    // the k-mer as oriented
    uint64_t idx;  // table index of its canonical form
    bool minimal;  // key is the canonical form
};

struct TipTable {
    const void *keys;
    const uint8_t *masks;
    PrefixTable P;
    int k;
    uint64_t n;
};

inline TipTable tip_table(const bbk_extindex *x) {
    return TipTable{x->keys.p, x->masks.as<uint8_t>(), x->prefix.table(), (int)x->k, x->n};
}

template <int W>
__device__ inline uint64_t tt_find(const TipTable &T, const Key<W> &q) {
    return table_find<W>(reinterpret_cast<const Key<W> *>(T.keys), T.P, q);
}

// InvertableKeyWithHash (utils/ph_map/key_with_hash.hpp:108-207)
template <int W>
__device__ inline bool tt_orient(const TipTable &T, const Key<W> &key, Oriented<W> &o) {
    const Key<W> rc = kmer_rc<W>(key, T.k);
    o.key = key;
    o.minimal = !kmer_less_nucl<W>(rc, key);  // IsMinimal (rtseq.hpp:407-415)
    o.idx = tt_find<W>(T, key_select<W>(o.minimal, key, rc));
    return o.idx != kNotFound;
}

// InvertableStoring::get_value (storing_traits.hpp:30-68)
template <int W>
__device__ inline uint32_t tt_mask(const uint8_t *masks, const Oriented<W> &o) {
    const uint32_t m = masks[o.idx];
    return o.minimal ? m : rev8(m);
}

__device__ inline bool unique4(uint32_t nib) { return __builtin_popcount(nib & 15u) == 1; }

static __global__ void k_tips_apply(const uint8_t *__restrict__ masks, const uint8_t *__restrict__ flag, uint64_t n,
                                    uint8_t *__restrict__ out) {
    const uint64_t i = BBK_GID();
    if (i < n) out[i] = flag[i] ? (uint8_t)0 : masks[i];  // IsolateVertex
}

// RemoveInconsistentForwardLinks (:20-35) for both orientations of stored k-mer i; T.masks = the masks after
// k_tips_apply (read-only here), `out` the final masks
template <int W>
static __global__ __launch_bounds__(256) void k_tips_links(TipTable T, const uint8_t *__restrict__ tipped,
                                                          uint8_t *__restrict__ out, unsigned long long *__restrict__ links) {
    const uint64_t i = BBK_GID();
    if (i >= T.n) return;
    uint32_t stored = T.masks[i];
    if (tipped[2 * i] | tipped[2 * i + 1]) {
        const Key<W> canon = key_load<W>(&reinterpret_cast<const Key<W> *>(T.keys)[i]);
        uint32_t cnt = 0;
        for (int side = 0; side < 2; ++side) {
            if (!tipped[2 * i + side]) continue;
            const Key<W> key = key_select<W>(side == 1, kmer_rc<W>(canon, T.k), canon);
            Oriented<W> kh;
            if (!tt_orient<W>(T, key, kh)) continue;
            const uint32_t mask = kh.minimal ? stored : rev8(stored);
            const uint32_t first = kmer_base<W>(key, 0);
            for (uint32_t c = 0; c < 4; ++c) {
                if (!(mask & (1u << c))) continue;
                Oriented<W> nx;
                if (!tt_orient<W>(T, kmer_shl<W>(key, T.k, c), nx)) continue;
                if (!(tt_mask<W>(T.masks, nx) & (1u << (4 + first)))) {
                    // DeleteOutgoing: bit c of the oriented mask = bit (as_is ? c : 7 - c) of the stored byte
                    stored &= ~(1u << (kh.minimal ? c : 7u - c));
                    ++cnt;
                }
            }
        }
        if (cnt) atomicAdd(links, (unsigned long long)cnt);
    }
    out[i] = (uint8_t)stored;
}

}  // namespace bbk
