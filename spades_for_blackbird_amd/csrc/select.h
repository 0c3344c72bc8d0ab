// select.h -- the one ordered selection: "keep the items that pass a test, in their order" (DESIGN.md 4.3l).
//
// A wavefront takes a tile of kSelTile consecutive items, kSelLane per lane.  The predicate is asked once per lane, in
// MASK FORM: uint32_t pred(p, n) -- bit b says item p + b is kept; p is a multiple of kSelLane below n, and an item at or
// beyond n is never kept.  A site whose test reads one item at a time wraps it with per_item(f); a site with tuned loads
// (load4_u32: four u32 values of a lane in one 16-byte load -- U32AtLeast, kmerfilter.hip) writes the mask itself.  The
// kept items of a tile are three ballots (the bits of the lanes' totals 0..4); one scan of the tile totals gives the tile bases, and the write
// kernel asks the SAME predicate object again, ranks a lane's first kept item from the ballots below it and hands every
// kept item to the emitter: void emit(i, rank).  The test is stated once, n / 32 bytes of device memory carry the
// offsets, and there are no atomics: the same input gives the same bytes.
//
// Host side: select_count runs the count kernel and the scan (ONE host wait) and returns the Selection; select_write
// queues the write behind it and does not wait.  n == 0 launches nothing, kept == 0 launches no write.
// Predicates and emitters are plain structs passed by value.
#pragma once

#include "bbk_internal.h"

namespace bbk {

constexpr uint32_t kSelLane = 4, kSelTile = 64 * kSelLane;  // items of a lane, of a wavefront's tile

// The totals t (below 1 << BITS) of the lanes of a wavefront as BITS ballots (the bits of t): their sum over the lanes
// below this one, and over all lanes
template <uint32_t BITS>
__device__ inline void wave_sums(uint32_t t, uint32_t lane, uint32_t *below, uint32_t *all) {
    const uint64_t lt = (1ull << lane) - 1ull;
    uint32_t b = 0, a = 0;
#pragma unroll
    for (uint32_t bit = 0; bit < BITS; ++bit) {
        const uint64_t m = __ballot((t >> bit) & 1u);
        b += (uint32_t)__popcll(m & lt) << bit;
        a += (uint32_t)__popcll(m) << bit;
    }
    *below = b;
    *all = a;
}

// The mask form of a test on one item: bool f(i), asked for the items of the lane that exist
template <class F>
struct PerItem {
    F f;
    __device__ uint32_t operator()(uint64_t p, uint64_t n) const {
        uint32_t m = 0;
#pragma unroll
        for (uint32_t b = 0; b < kSelLane; ++b) m |= (p + b < n && f(p + b) ? 1u : 0u) << b;
        return m;
    }
};
template <class F>
PerItem<F> per_item(F f) {
    return PerItem<F>{f};
}

// Four consecutive u32 values for a predicate in mask form: one 16-byte load where all four exist (p is a multiple of 4
// and v is 16-byte aligned, as every device buffer is), 0 beyond n
__device__ inline void load4_u32(const uint32_t *__restrict__ v, uint64_t n, uint64_t p, uint32_t c[kSelLane]) {
    if (p + kSelLane <= n) {
        const uint4 q = *reinterpret_cast<const uint4 *>(v + p);
        c[0] = q.x;
        c[1] = q.y;
        c[2] = q.z;
        c[3] = q.w;
    } else {
#pragma unroll
        for (uint32_t b = 0; b < kSelLane; ++b) c[b] = p + b < n ? v[p + b] : 0u;
    }
}

// vals[i] >= min in mask form (vals: the start of a device buffer)
struct U32AtLeast {
    const uint32_t *__restrict__ vals;
    uint32_t min;
    __device__ uint32_t operator()(uint64_t p, uint64_t n) const {
        uint32_t c[kSelLane], m = 0;
        load4_u32(vals, n, p, c);
#pragma unroll
        for (uint32_t b = 0; b < kSelLane; ++b) m |= (p + b < n && c[b] >= min ? 1u : 0u) << b;
        return m;
    }
};

// total[tile]: the kept items of the tile
template <class Pred>
__global__ __launch_bounds__(256) void k_select_count(Pred pred, uint64_t n, uint64_t n_tiles, uint64_t *__restrict__ total) {
    const uint64_t tile = (BBK_GID()) >> 6;
    if (tile >= n_tiles) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t p = tile * kSelTile + (uint64_t)lane * kSelLane;
    const uint32_t m = p < n ? pred(p, n) : 0u;
    uint32_t below, all;
    wave_sums<3>((uint32_t)__popc(m), lane, &below, &all);
    if (lane == 0) total[tile] = all;
}

// base: the scanned totals of k_select_count.  n_kept: their sum, the ranks the emitter may be handed
template <class Pred, class Emit>
__global__ __launch_bounds__(256) void k_select_write(Pred pred, Emit emit, uint64_t n, uint64_t n_tiles,
                                                     const uint64_t *__restrict__ base, uint64_t n_kept) {
    const uint64_t tile = (BBK_GID()) >> 6;
    if (tile >= n_tiles) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t p = tile * kSelTile + (uint64_t)lane * kSelLane;
    const uint32_t m = p < n ? pred(p, n) : 0u;
    uint32_t below, all;
    wave_sums<3>((uint32_t)__popc(m), lane, &below, &all);
    uint64_t j = base[tile] + below;
#pragma unroll
    for (uint32_t b = 0; b < kSelLane; ++b) {
        if (((m >> b) & 1u) && j < n_kept) {
            emit(p + b, j);
            ++j;
        }
    }
}

struct Selection {
    uint64_t n = 0, n_tiles = 0;
    uint64_t kept = 0;  // the items that pass
    DevBuf base;        // [n_tiles] kept items before the tile
};

// Counts the items of [0, n) that pass `pred`; waits for the stream once (the scan's wait)
template <class Pred>
Selection select_count(bbk_ctx *ctx, const char *family, uint64_t n, Pred pred) {
    Selection s;
    s.n = n;
    s.n_tiles = (n + kSelTile - 1) / kSelTile;
    if (n == 0) return s;
    s.base.alloc(s.n_tiles * 8);
    uint64_t *base = s.base.as<uint64_t>();
    launch_items_timed(ctx, family, k_select_count<Pred>, s.n_tiles * 64, pred, n, s.n_tiles, base);
    s.kept = exclusive_scan_u64(ctx, base, base, s.n_tiles);
    BBK_REQUIRE(s.kept <= n, BBK_ERR_INTERNAL, "%s: %llu of %llu items selected", family, (unsigned long long)s.kept,
                (unsigned long long)n);
    return s;
}

// Queues emit(i, rank) for every item that passes `pred` -- the predicate select_count was given; does not wait
template <class Pred, class Emit>
void select_write(bbk_ctx *ctx, const char *family, const Selection &s, Pred pred, Emit emit) {
    if (s.kept == 0) return;
    launch_items_timed(ctx, family, k_select_write<Pred, Emit>, s.n_tiles * 64, pred, emit, s.n, s.n_tiles,
                       s.base.as<uint64_t>(), s.kept);
}

}  // namespace bbk
