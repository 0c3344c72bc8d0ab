// msd_narrow_a.h -- stage A's 4-byte records (reads, 17 <= k <= 21, hash slots): level 1 from reads, level 2, the
// LDS dedup and the widening back to 8-byte keys.  Launched by Pass::level1, level2_scatter, launch_buckets, overflow
// and compact (msd.hip) when Plan::narrow is set.
#pragma once

#include "msd_mark_tail.h"

namespace bbk {

// ---- narrow records (stage A, 17 <= k <= 21) ---------------------------------------------------------------
// A k-mer of 2k <= 42 bits is (hi: 2k - 32 = hb bits, lo: 32 bits = its first 16 bases).  With t = mix(lo), level 1
// sends it to segment
//   bin1 = (t >> 22) ^ (hi << (10 - hb))      (the top ten hash bits of lo, hi folded into the upper hb of them)
// and stores ONLY lo: inside a segment lo determines hi (= (bin1 ^ t >> 22) >> (10 - hb)), so 4-byte records are exact --
// equal lo <=> equal k-mer.  Level 2 and the in-LDS dedup work on lo alone (their bins / slots are other bits of the
// same mix), the dedup kernel rebuilds the 8-byte key from (segment, lo) when it writes the distinct records.  The
// canonical stream -- 1.3 G records at BASELINE configs[1], 8.3x the distinct set -- travels as 4 bytes per record
// instead of 8 through its three passes (level-1 write, level-2 read + write, dedup read).
constexpr int kNwBins1 = 1024;
__device__ inline uint32_t nw_mix(uint32_t lo) {
    uint32_t t = lo * 0x9E3779B1u;
    t ^= t >> 15;
    t *= 0x85EBCA6Bu;
    t ^= t >> 13;
    return t;
}
__device__ inline uint32_t nw_slot(uint32_t t) { return (t * 0x27D4EB2Fu) >> 19; }  // 13 bits for the LDS table
__device__ inline uint32_t nw_bin1(uint32_t hi, uint32_t t, int hb) { return (t >> 22) ^ (hi << (10 - hb)); }
// prefix for level 2: the bits of the mix that level 1 has not used (top-aligned)
__device__ inline uint32_t nw_p2(uint32_t t) { return t << 10; }
// level-2 bin of a record among the nb <= 1024 bins of its segment: __umulhi(nw_p2(t), nb) = ((t & 0x3FFFFF) * nb) >> 22
// exactly, and both factors lie below 2^24 (the product below 2^32): one full-rate 24-bit multiply
__device__ inline uint32_t nw_bin2(uint32_t t, uint32_t nb) {
#ifdef BBK_AB_NW_BIN2_MULHI  // (A/B: the 32 x 32 -> high-word multiply, as before round 11)
    return __umulhi(nw_p2(t), nb);
#else
    return __umul24(t & 0x3FFFFFu, nb) >> 22;
#endif
}
__device__ inline uint64_t nw_key(uint32_t bin1, uint32_t lo, int hb) {
    const uint32_t hi = (bin1 ^ (nw_mix(lo) >> 22)) >> (10 - hb);
    return ((uint64_t)hi << 32) | lo;
}

// ------------------------------------------------------------------------------------------
// narrow stage A kernels (4-byte records, see "narrow records" above): level 1 from reads, level 2, dedup
// ------------------------------------------------------------------------------------------
constexpr int kNwThreads = 1024;
#ifndef BBK_NW_ROUNDS  // (experiments: -DBBK_NW_ROUNDS=4 -DBBK_NW_CHUNKS=3840 -DBBK_NW_WAVES=4 is one workgroup per CU with a 120 KB stage)
#define BBK_NW_ROUNDS 2
#define BBK_NW_CHUNKS 1920
#define BBK_NW_WAVES 8
#endif
constexpr int kNwRounds = BBK_NW_ROUNDS;  // consecutive chunks of 8 k-mer positions per lane (the last 64 lanes of a full tile idle)
constexpr int kNwChunks = BBK_NW_CHUNKS;  // chunks of a level-1 tile: 15360 records = 60 KB staged, runs of ~15 per bin;
                                  // (x 8 records) with the tables 78 KB of LDS: two workgroups per CU
// with a payload (one mask byte per record: the extension index) the same tile would take 94 KB = ONE workgroup per CU
// (measured 8.4 ms against 3.8 ms without payload); 1536 chunks = 12 288 records x 5 bytes + tables = 78 KB
template <bool HAS_VAL>
struct NwCfg {
    static constexpr int ROUNDS = HAS_VAL ? 1 : kNwRounds;       // with the mask extraction two rounds need 72 VGPRs:
    static constexpr int CHUNKS = HAS_VAL ? 1024 : kNwChunks;    // one workgroup of 1024 per CU.  One round: 8192 records
    static constexpr int TILE = CHUNKS * 8;
};

// Eight consecutive k-mer positions of one read from ONE 64-bit window (narrow k: 8 + k + 1 <= 30 bases fit).  With
// F = bases p .. p+31 (base p in the low bits) and NR = ~rev2(F) (the complement of base p at the top),
//   a_i = F  << (64 - 2k - 2i)   is k-mer i top-aligned (its last base in the top bits, other bases of the read below),
//   b_i = NR << 2i               is its reverse complement laid out the same way,
// and the canonical k-mer (base-lexicographic minimum of the two, rtseq.hpp:407-415) is min(a_i, b_i) >> (64 - 2k):
// comparing a k-mer x with rc(x) from the last base down decides like comparing them from the first base up (the first
// difference from the start, x[j] against ~x[k-1-j], is also the first one from the end, ~x[j] against x[k-1-j]).
// Two shifts, one compare, two selects per k-mer -- no carried state, against ~20 operations of the rolled form.
template <bool HAS_VAL>
__device__ __forceinline__ void nw_chunk(const uint64_t *rw, uint32_t p, uint32_t cnt, uint32_t len, uint32_t k_, int hb,
                                         uint32_t *lhist, uint32_t (&lo)[8], uint32_t (&bins)[3], uint32_t (&masks)[2]) {
    constexpr int CH = 8;
    const uint32_t pad = 64u - 2u * k_;  // 22 .. 30
    uint64_t F = 0, NR = 0;
    uint32_t pb = 0;
    if (cnt) {
        F = bases_from(rw, p, (len - 1u) >> 5);
        NR = ~rev2(F);
        if (HAS_VAL) pb = p ? base_at(rw, p - 1u) : 0u;
    }
    bins[0] = bins[1] = bins[2] = 0;
    masks[0] = masks[1] = 0;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        // (computed for idle positions too -- values, not branches: only the LDS atomic is conditional)
        const uint64_t a = F << (pad - 2u * (uint32_t)i);
        uint64_t b = NR << (2 * i);
        // a palindrome counts as minimal (only the mask bits can tell): the unused low bits of b are set
        if (HAS_VAL) b |= (1ull << pad) - 1ull;
        const bool minimal = a <= b;
        const uint64_t key = (minimal ? a : b) >> pad;
        const uint32_t klo = (uint32_t)key;
        const uint32_t bin = nw_bin1((uint32_t)(key >> 32), nw_mix(klo), hb);  // key < 4^k: bin < 1024
        if (HAS_VAL) {
            const uint32_t q = p + (uint32_t)i;
            const uint32_t nextc = (uint32_t)(F >> (2u * ((uint32_t)i + k_))) & 3u;  // base q + k (i + k <= 28)
            const uint32_t prevc = i == 0 ? pb : (uint32_t)(F >> (2 * (i > 0 ? i - 1 : 0))) & 3u;  // base q - 1
            uint32_t m = 0;
            if (q + k_ < len) m |= 1u << (minimal ? nextc : 7u - nextc);
            if (q >= 1) m |= 1u << (minimal ? 4u + prevc : 3u - prevc);
            masks[i >> 2] |= m << (8 * (i & 3));
        }
        if ((uint32_t)i < cnt) atomicAdd(&lhist[bin], 1u);  // count only: the place inside the bin is taken after the scan
        lo[i] = klo;
        bins[i / 3] |= bin << (10 * (i % 3));  // three 10-bit bins per register
        // with the mask arithmetic eight interleaved positions need more registers than two workgroups per CU leave
        if (HAS_VAL) __builtin_amdgcn_sched_barrier(0);
    }
}

// read (relative to the tile's first read) that owns chunk c of the tile: rel[r] <= c < rel[r + 1].  Reads are about
// equally long: the interpolated guess is right or off by one nearly always; otherwise a binary search.
__device__ __forceinline__ uint32_t nw_read_of(const int32_t *s_rel, uint32_t nr, int32_t c, int32_t rel0, float scale) {
    uint32_t g = (uint32_t)((float)(c - rel0) * scale);
    g = g < nr ? g : nr - 1u;
    if (s_rel[g] > c) --g;               // s_rel[0] <= 0 <= c: g stays >= 0
    else if (s_rel[g + 1] <= c) ++g;     // s_rel[nr] > c for every chunk of the tile: g stays < nr
    if (s_rel[g] > c || s_rel[g + 1] <= c) g = last_le(s_rel, nr, c);
    return g;
}

// A lane extracts ROUNDS consecutive chunks (usually of one read: the owner of the first is looked up, the next ones
// follow from it).
template <bool FAST, bool HAS_VAL>
__device__ __forceinline__ void nw_extract(const ReadSrc &S, const PartLevel &L, uint32_t k_, uint32_t tid, uint32_t nch,
                                           uint64_t c0, uint32_t r0, uint32_t nr, const int32_t *s_rel,
                                           const int32_t *s_wrel, const uint32_t *s_len, const uint64_t *s_words,
                                           uint32_t *lhist, uint32_t (&lo)[8 * NwCfg<HAS_VAL>::ROUNDS],
                                           uint32_t (&bins)[3 * NwCfg<HAS_VAL>::ROUNDS],
                                           uint32_t (&masks)[2 * NwCfg<HAS_VAL>::ROUNDS], uint32_t &cnts) {
    constexpr int CH = 8, R = NwCfg<HAS_VAL>::ROUNDS;
    cnts = 0;  // records of round r in bits 4r .. 4r+3
    const int hb = L.narrow_hb;
    const uint32_t ci0 = tid * (uint32_t)R;
    uint32_t ri = 0, p = 0, len = 0, nk = 0;
    const uint64_t *rw = FAST ? s_words : S.words;
    auto rel = [&](uint32_t i) -> int64_t {  // first chunk of read r0 + i, relative to the tile
        return FAST ? (int64_t)s_rel[i] : (int64_t)(S.coff[(uint64_t)r0 + i] - c0);
    };
    auto enter = [&](uint32_t i) {  // per-read values
        if (FAST) {
            len = s_len[i];
            rw = s_words + s_wrel[i];
        } else {
            len = S.len[(uint64_t)r0 + i];
            rw = S.words + S.woff[(uint64_t)r0 + i];
        }
        nk = len - k_ + 1u;
    };
    if (ci0 < nch) {
        if (FAST) {
            const int32_t rel0 = s_rel[0];
            const float scale = (float)nr / (float)(s_rel[nr] - rel0);
            ri = nw_read_of(s_rel, nr, (int32_t)ci0, rel0, scale);
        } else {
            uint32_t a = 0, b = nr;  // largest i with rel(i) <= ci0
            while (b - a > 1) {
                const uint32_t mid = (a + b) >> 1;
                if (rel(mid) <= (int64_t)ci0) a = mid;
                else b = mid;
            }
            ri = a;
        }
        enter(ri);
        p = (uint32_t)((int64_t)ci0 - rel(ri)) * CH;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t ci = ci0 + (uint32_t)r;
        uint32_t cnt = 0;
        if (ci < nch) {
            if (r > 0) {
                p += CH;
                if (p >= nk) {  // the next read that has chunks (rel(nr) lies beyond the tile: the walk ends)
                    do ++ri;
                    while (rel(ri + 1u) <= (int64_t)ci);
                    enter(ri);
                    p = 0;
                }
            }
            cnt = nk - p < (uint32_t)CH ? nk - p : (uint32_t)CH;
        }
        uint32_t l8[CH], b3[3], m2[2];
        nw_chunk<HAS_VAL>(rw, p, cnt, len, k_, hb, lhist, l8, b3, m2);
#pragma unroll
        for (int i = 0; i < CH; ++i) lo[r * CH + i] = l8[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) bins[r * 3 + i] = b3[i];
        masks[r * 2] = m2[0];
        masks[r * 2 + 1] = m2[1];
        cnts |= cnt << (4 * r);
    }
}

// Level 1: fused extraction + partition into 1024 segments.  The bin of a staged record cannot be recomputed from lo
// alone, and a per-record side array would cost as much LDS as the stage itself: the staged order is bin-major, so
// one bit per position marks where a non-empty bin starts and the r-th non-empty bin owns position pos when
// r = #marks below pos (a 64-position word of marks is exactly what a wave handles per step).  What a store needs
// of its bin sits in one 8-byte entry indexed by r.  The tail is msd_mark_tail.h's, shared with stage B's late tag.
template <bool HAS_VAL>
__global__ __launch_bounds__(kNwThreads) __attribute__((amdgpu_waves_per_eu(BBK_NW_WAVES, BBK_NW_WAVES))) void k_part_reads_narrow(ReadSrc S, PartLevel L, uint32_t ntiles,
                                                                 const RdTile *__restrict__ tiles_arg,  // = S.tiles: as an
                                                                 // argument of its own the descriptor is a scalar load
                                                                 uint32_t *__restrict__ cursor,
                                                                 uint32_t *__restrict__ out, uint32_t *__restrict__ vout) {
    constexpr int NT = kNwThreads, CH = 8, MAXB = kNwBins1, ITEMS = CH * NwCfg<HAS_VAL>::ROUNDS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const MarkLds ML = mark_lds<NwCfg<HAS_VAL>::TILE>(smem);  // counts, table, marks | then the read tables, later the stage
    uint32_t *lhist = ML.lhist;
    unsigned char *U = reinterpret_cast<unsigned char *>(ML.stage);
    int32_t *s_rel = reinterpret_cast<int32_t *>(U);
    int32_t *s_wrel = s_rel + (kRdSlots + 2);
    uint32_t *s_len = reinterpret_cast<uint32_t *>(s_wrel + (kRdSlots + 2));
    uint64_t *s_words = reinterpret_cast<uint64_t *>(s_len + (kRdSlots + 2));

    uint32_t tid = threadIdx.x;
    const uint32_t k_ = (uint32_t)S.k;
    const int hb = L.narrow_hb;
    uint32_t xcc = 0;  // the XCD this workgroup runs on (placement is for speed only: any value gives a correct result)
    if (L.xcd_shift) {
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        xcc &= (1u << L.xcd_shift) - 1u;
    }
#ifdef BBK_PHASE_PROF
    unsigned long long t_prev = clock64();
#else
    const unsigned long long t_prev = 0;
    (void)t_prev;
#endif

    // A workgroup walks tiles blockIdx.x, + gridDim.x, ... (normally one: grid = tiles) and loads what the NEXT tile
    // needs (its read tables and packed words: two dependent round trips to memory after the descriptor) into registers
    // while it stores the current one.  One table entry and two words per thread: a tile with more reads or words than
    // that takes the global-memory path (as does one not laid out in read order).
    struct Pre {
        uint64_t coff, woff, w0, w1;
        uint32_t len;
    };
    auto staged_ok = [&](const RdTile &T) { return T.wspan != 0xFFFFFFFFu && T.nr < (uint32_t)NT && T.wspan <= 2u * NT; };
    auto prefetch = [&](const RdTile &T, Pre &Q) {
        Q = Pre{0, 0, 0, 0, 0};  // (the previous tile's values end here: they must not stay alive through the loop)
        if (!staged_ok(T)) return;  // (uniform)
        // unconditional loads, indices clamped into the tile's tables (a staged tile has >= 1 read and >= 1 word)
        const uint32_t i0 = tid < T.nr ? tid : T.nr, i1 = tid < T.nr ? tid : T.nr - 1u;
        const uint32_t j0 = tid < T.wspan ? tid : T.wspan - 1u, j1 = tid + NT < T.wspan ? tid + NT : T.wspan - 1u;
        Q.coff = S.coff[(uint64_t)T.r0 + i0];
        Q.woff = S.woff[(uint64_t)T.r0 + i1];
        Q.len = S.len[(uint64_t)T.r0 + i1];
        Q.w0 = S.words[T.wbase + j0];
        Q.w1 = S.words[T.wbase + j1];
    };

#ifdef BBK_NW_TILES_VIA_STRUCT  // (A/B: the descriptor through the pointer inside S -- a vector load + readfirstlane)
    const RdTile *tiles = S.tiles;
    (void)tiles_arg;
#else
    const RdTile *__restrict__ tiles = tiles_arg;
#endif
    uint32_t tile = blockIdx.x;
    if (tile >= ntiles) return;
    RdTile T = tiles[tile];
    Pre Q{0, 0, 0, 0, 0};
    prefetch(T, Q);
    for (;;) {
        // (the thread index is made opaque per iteration: the compiler otherwise computes every address that depends on
        // it -- 16 stage positions, table slots ... -- once before the loop and keeps ~45 registers alive through it,
        // which is one workgroup per CU instead of two)
        asm volatile("" : "+v"(tid));
        const uint32_t tile_next = tile + gridDim.x;
        const bool more = tile_next < ntiles;  // uniform: every wave of the workgroup leaves the loop together
        RdTile Tn = T;
        if (more) Tn = tiles[tile_next];

        const uint64_t c0 = (uint64_t)tile * NwCfg<HAS_VAL>::CHUNKS;
        const uint64_t left = S.n_chunks - c0;
        const uint32_t nch = left < (uint64_t)NwCfg<HAS_VAL>::CHUNKS ? (uint32_t)left : (uint32_t)NwCfg<HAS_VAL>::CHUNKS;
        const uint32_t r0 = T.r0, nr = T.nr;
        const uint64_t wbase = T.wbase;
        const bool fast = staged_ok(T);
        mark_clear<NwCfg<HAS_VAL>::TILE>(ML, tid);  // NT == MAXB
        if (fast) {  // (a staged tile's reads lie inside its window of words: k_tile_reads)
            if (tid <= nr) s_rel[tid] = (int32_t)(int64_t)(Q.coff - c0);
            if (tid < nr) {
                s_wrel[tid] = (int32_t)(int64_t)(Q.woff - wbase);
                s_len[tid] = Q.len;
            }
            if (tid < T.wspan) s_words[tid] = Q.w0;
            if (tid + NT < T.wspan) s_words[tid + NT] = Q.w1;
        }
        __syncthreads();
        BBK_PH(5, 0, t_prev);  // read tables + words into LDS

        uint32_t lo[ITEMS], bins[3 * NwCfg<HAS_VAL>::ROUNDS], masks[2 * NwCfg<HAS_VAL>::ROUNDS], cnts;
        // (two instantiations: the address space of the packed words -- LDS or global -- must be static, a pointer that
        // may be either compiles to flat loads)
        if (fast) nw_extract<true, HAS_VAL>(S, L, k_, tid, nch, c0, r0, nr, s_rel, s_wrel, s_len, s_words, lhist, lo, bins, masks, cnts);
        else nw_extract<false, HAS_VAL>(S, L, k_, tid, nch, c0, r0, nr, s_rel, s_wrel, s_len, s_words, lhist, lo, bins, masks, cnts);
        __syncthreads();  // histogram complete; the read tables may be overwritten by the stage
        BBK_PH(5, 1, t_prev);  // extraction + LDS ranking

        // scan, reservation, reorder, mark prefix, stores and spills: the shared tail (msd_mark_tail.h)
        const uint64_t slot_end = L.xcd_shift ? (uint64_t)tid * L.slot_stride + (uint64_t)(xcc + 1u) * L.sub_cap
                                              : (uint64_t)tid * L.slot_stride + L.slot_cap;
        mark_tail<NwCfg<HAS_VAL>::TILE, ITEMS, HAS_VAL>(
            ML, lo, tid, (uint32_t)MAXB, &cursor[(tid << L.xcd_shift) + xcc], slot_end, 0u, L, out, vout,
            [&](int i) {
                const int r = i / CH, j = i % CH;
                return (uint32_t)j < ((cnts >> (4 * r)) & 15u) ? (bins[r * 3 + j / 3] >> (10 * (j % 3))) & 1023u : 0xFFFFFFFFu;
            },
            [&](int i) { return masks[(i / CH) * 2 + ((i % CH) >> 2)] >> (8 * (i & 3)); },
            [&](uint32_t bin, uint32_t rec) { return nw_key(bin, rec, hb); },
            [&]() {
                BBK_PH(5, 3, t_prev);  // scans + reservation + reorder into LDS + mark prefix
                if (more) prefetch(Tn, Q);  // in flight during the stores
                else Q = Pre{0, 0, 0, 0, 0};   // (the old values end here either way: they must not stay alive through the loop)
            });
        BBK_PH(5, 4, t_prev);  // store issue
#ifdef BBK_PHASE_PROF
        if (threadIdx.x == 0) atomicAdd(&g_phase[5][7], 1ull);
#endif
        if (!more) break;
        __syncthreads();  // the stage and the tables have been read: the next tile may overwrite them
        tile = tile_next;
        T = Tn;
    }
}

static size_t part_reads_narrow_smem(bool has_val) {
    const size_t tables = sizeof(uint32_t) * 3 * (kRdSlots + 2) + sizeof(uint64_t) * (kRdWords + 1 + 2);
    const size_t tile = has_val ? NwCfg<true>::TILE : NwCfg<false>::TILE;
    const size_t stage = tile * (has_val ? 5 : 4);
    return mark_smem(tile) + std::max(tables, stage);
}

// Level 2: one tile (<= 12288 records) of one segment -> the bucket slots of that segment.  Everything derives from lo.
constexpr int kNw2Threads = 1024;  // == kMaxBins: one bin per thread in the scans
// records per lane: 12 without payload (two workgroups of 1024 per CU; with 16 the kernel needed 72 registers and ran
// one: 3.2 -> 2.6 ms at BASELINE configs[1]), 8 with a payload (the mask byte of level 1: the extension index)
template <bool HAS_VAL>
struct Nw2Cfg {
    static constexpr int ITEMS = HAS_VAL ? 8 : 12;
    static constexpr int TILE = kNw2Threads * ITEMS;
};

// The contiguous records of a tile, four per load.  Item i of a lane is record tile_item4(i, tid) of the tile: group
// i / 4 of the lane is records 4 * ((i / 4) * NT + tid) .. + 3, one 16-byte load.  Which lane holds which record is
// free -- the staged order is by bin.  The loads stay unconditional: a lane past the tile's last group re-reads that
// group (one address for all of them), so up to three words behind the tile's last record are read and never used;
// the level-1 buffer has that slack behind its last slot.  Tile starts are 4-byte aligned only (an odd
// Plan::sub_cap), hence the vector type of alignment 4.  (k_part_lt2 was measured with these loads and did not move:
// profiles/level2_tail.)
typedef uint32_t TileRow4 __attribute__((ext_vector_type(4), aligned(4)));
template <int NT>
__device__ __forceinline__ uint32_t tile_item4(int i, uint32_t tid) {
    return 4u * ((uint32_t)(i >> 2) * NT + tid) + (uint32_t)(i & 3);
}
template <int NT, int ITEMS>
__device__ __forceinline__ void tile_rows4(const uint32_t *__restrict__ in, uint32_t begin, uint32_t count, uint32_t tid,
                                           uint32_t (&rec)[ITEMS]) {
    static_assert(ITEMS % 4 == 0, "whole groups of four");
    const uint32_t last = (count - 1u) & ~3u;
#pragma unroll
    for (int r = 0; r < ITEMS / 4; ++r) {
        const uint32_t p = 4u * ((uint32_t)r * NT + tid);
        const TileRow4 q = *reinterpret_cast<const TileRow4 *>(in + begin + (p < last ? p : last));
        rec[4 * r] = q.x, rec[4 * r + 1] = q.y, rec[4 * r + 2] = q.z, rec[4 * r + 3] = q.w;
    }
}

// The histogram's atomic returns a record's place inside its bin, kept beside the bin (sixteen bits each); the scan,
// reservation, reorder, stores and spills are the shared tail's (msd_mark_tail.h) in its RANKED form: the reorder adds
// the place to the bin's start, and the bin of a staged record is not computed a second time.  (Counting first and
// taking the place with a second returning atomic after the scan, as the tail's other users do, was measured slower
// than the kernel's former own tail: profiles/level2_tail.)  The payload of every caller is level 1's mask byte.
template <bool HAS_VAL>
__global__ __launch_bounds__(kNw2Threads) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_part_narrow2(
    const uint32_t *__restrict__ in, const uint32_t *__restrict__ vin, const uint4 *__restrict__ desc, PartLevel L,
    uint32_t *__restrict__ cursor, uint32_t *__restrict__ out, uint32_t *__restrict__ vout) {
    constexpr int NT = kNw2Threads, ITEMS = Nw2Cfg<HAS_VAL>::ITEMS, TILE = Nw2Cfg<HAS_VAL>::TILE;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const MarkLds S = mark_lds<TILE>(smem);
    const uint32_t tid = threadIdx.x;
    const int hb = L.narrow_hb;
    const uint4 d = desc[blockIdx.x];  // first record, records, bins of the segment | segment << 16, flat index of bin 0
    const uint32_t begin = d.x, count = d.y, nb = d.z & 0xFFFFu, seg = d.z >> 16, gbin0 = d.w;
    if (count == 0) return;  // an unused place of the XCD-wise order (k_tile_desc)
    mark_clear<TILE>(S, tid);  // NT == kMaxBins
    __syncthreads();
    uint32_t lo[ITEMS], vals[ITEMS];
    tile_rows4<NT, ITEMS>(in, begin, count, tid, lo);  // all loads first
    if (HAS_VAL) tile_rows4<NT, ITEMS>(vin, begin, count, tid, vals);
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        asm volatile("" : "+v"(lo[i]));
        if (HAS_VAL) asm volatile("" : "+v"(vals[i]));
    }
    uint32_t binrank[ITEMS];
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        binrank[i] = 0xFFFFFFFFu;
        if (tile_item4<NT>(i, tid) < count) {
            const uint32_t b = nw_bin2(nw_mix(lo[i]), nb);
            binrank[i] = (b << 16) | atomicAdd(&S.lhist[b], 1u);
        }
    }
    __syncthreads();
    const uint64_t slot_end = (uint64_t)(gbin0 + tid) * L.slot_stride + L.slot_cap;
    mark_tail<TILE, ITEMS, HAS_VAL, true>(
        S, lo, tid, nb, &cursor[gbin0 + tid], slot_end, 0u, L, out, vout, [&](int i) { return binrank[i]; },
        [&](int i) { return vals[i]; }, [&](uint32_t, uint32_t rec) { return nw_key(seg, rec, hb); }, []() {});
}

static size_t part_narrow2_smem(bool has_val) {
    const size_t tile = has_val ? Nw2Cfg<true>::TILE : Nw2Cfg<false>::TILE;
    return mark_smem(tile) + tile * (has_val ? 5 : 4);
}

// Dedup of one bucket of 4-byte records in an LDS table (32-bit ds_cmpst); the distinct records leave as 8-byte keys
// rebuilt from (segment of the bucket, lo).  The all-ones record (16 x T) is the table's empty marker and is counted
// on the side.
constexpr int kNwHashThreads = 512;
constexpr int kNwHashItems = 16;  // 8192 records per bucket
constexpr uint32_t kNwHashSlots = 8192;
constexpr uint32_t kNwEmpty = 0xFFFFFFFFu;

// Table slot of a record: the top 13 bits of the FIRST product of nw_mix.  Segment and level-2 bin fix about 18 bits of
// nw_mix(lo) inside a bucket; the top bits of lo * 0x9E3779B1 are not among them, and linear probing on them needs
// the same number of extra probes as on a third multiply of the mix (tests/test_hash32_slot.py) -- one multiply per
// record instead of three.
__device__ inline uint32_t nw_hslot(uint32_t lo) {
#ifdef BBK_AB_HASH32_OLD  // (A/B: the third multiply of the mix, as before round 11)
    return nw_slot(nw_mix(lo)) & (kNwHashSlots - 1);
#else
    return (lo * 0x9E3779B1u) >> 19;
#endif
}

template <int OP>
__device__ __forceinline__ void nw_pay(uint32_t *at, uint32_t v) {
    if (OP == 1) atomicAdd(at, 1u);
    else if (OP == 2) atomicAdd(at, v);
    else if (OP == 3) atomicOr(at, v);
}

// Linear probing behind a slot that held another key: walks on from slot + 1 until the key is in the table (`first`:
// this call put it there) or more than max_probes slots were tried, which raises the give-up flag.  `probes` counts
// the slots tried before (0xFFFFFFFF with slot - 1: the walk starts at the slot itself).  Returns the slot it ended on.
__device__ __forceinline__ uint32_t nw_walk(uint32_t *tab, uint32_t *scan_tmp, uint32_t key, uint32_t slot, uint32_t probes,
                                            uint32_t max_probes, bool &first) {
    for (;;) {
        slot = (slot + 1) & (kNwHashSlots - 1);
        if (++probes > max_probes) {
            scan_tmp[14] = 1;
            break;
        }
        const uint32_t old = atomicCAS(&tab[slot], kNwEmpty, key);
        if (old == kNwEmpty) first = true;
        if (old == kNwEmpty || old == key) break;
    }
    return slot;
}

// One row of a bucket: NR records per lane (k[j] is record p0 + j), `full` (uniform): every record of the row lies
// below n.  The first probes of the row are straight-line -- NR ds_cmpst in flight, one wait, no per-record branch, and
// in a full row no per-record predicate; the lanes that met another key walk on behind ONE wave-uniform test.  A row
// that holds the all-ones record (or, past n, whatever the slot held before) goes record by record: at k <= 21 a
// canonical record is never all ones.  Returns bit j = record j was the first of its key in the table.
template <int OP, int NR>
__device__ __forceinline__ uint32_t nw_insert_row(uint32_t *tab, uint32_t *pay, uint32_t *scan_tmp, const uint32_t *k,
                                                  const uint32_t *v, uint32_t p0, bool full, uint32_t n,
                                                  uint32_t max_probes) {
    constexpr uint32_t ALL = (1u << NR) - 1u;
    const uint32_t left = p0 < n ? n - p0 : 0u;
    const uint32_t valid = full || left >= (uint32_t)NR ? ALL : (1u << left) - 1u;
    uint32_t mx = k[0], first = 0;
#pragma unroll
    for (int j = 1; j < NR; ++j) mx = k[j] > mx ? k[j] : mx;
    if (__any(mx == kNwEmpty)) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            if (!((valid >> j) & 1u)) continue;
            if (k[j] == kNwEmpty) {
                scan_tmp[13] = 1;
                nw_pay<OP>(&scan_tmp[12], v[j]);
                continue;
            }
            bool f = false;
            const uint32_t slot = nw_walk(tab, scan_tmp, k[j], nw_hslot(k[j]) - 1u, 0xFFFFFFFFu, max_probes, f);
            first |= (f ? 1u : 0u) << j;
            if (OP != 0) nw_pay<OP>(&pay[slot], v[j]);
        }
        return first;
    }
    uint32_t slot[NR], old[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) slot[j] = nw_hslot(k[j]);
    if (full) {
#pragma unroll
        for (int j = 0; j < NR; ++j) old[j] = atomicCAS(&tab[slot[j]], kNwEmpty, k[j]);
    } else {
#pragma unroll
        for (int j = 0; j < NR; ++j) old[j] = (valid >> j) & 1u ? atomicCAS(&tab[slot[j]], kNwEmpty, k[j]) : k[j];
    }
    uint32_t miss = 0;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        first |= (old[j] == kNwEmpty ? 1u : 0u) << j;
        miss |= (old[j] != kNwEmpty && old[j] != k[j] ? 1u : 0u) << j;
    }
    if (__any(miss != 0)) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            if ((miss >> j) & 1u) {
                bool f = false;
                slot[j] = nw_walk(tab, scan_tmp, k[j], slot[j], 0u, max_probes, f);
                first |= (f ? 1u : 0u) << j;
            }
        }
    }
    if (OP != 0) {
#pragma unroll
        for (int j = 0; j < NR; ++j)
            if ((valid >> j) & 1u) nw_pay<OP>(&pay[slot[j]], v[j]);
    }
    return first;
}

// Front half of k_bucket_hash32 (every OP): the bucket's records into registers, the table cleared, the records
// inserted row by row.  A row is NR records per lane: 4 in slot mode, where every bucket starts on a 256-byte boundary
// (Plan::stride2) and a lane loads four uint4 -- records 4 * (r * 512 + tid) .. + 3 of row r; 1 with the dense layout,
// whose buckets start anywhere (dword loads, record r * 512 + tid).  n is uniform: a row past n costs one scalar
// branch, a row below n runs unpredicated, only the last one tests its records.  Leaves kk[i] and returns bit i =
// record i was the first of its key.
template <int OP, int NR>
__device__ __forceinline__ uint32_t nw_hash32_rows(const uint32_t *__restrict__ buf, const uint32_t *__restrict__ vals,
                                                   uint32_t *tab, uint32_t *pay, uint32_t *scan_tmp, uint32_t start,
                                                   uint32_t n, uint32_t max_probes, uint32_t (&kk)[kNwHashItems],
                                                   unsigned long long &t_prev) {
    constexpr bool IN_VAL = OP >= 2;
    constexpr int ROWS = kNwHashItems / NR;
    constexpr uint32_t ROW = (uint32_t)kNwHashThreads * NR;
    const uint32_t tid = threadIdx.x;
    uint32_t vv[kNwHashItems];
    if constexpr (NR == 4) {
        // (a lane past the bucket's last group of four re-reads that group: one address for all of them, and the loads
        // stay unconditional -- with a branch around a load every insertion waits for ALL loads, profiles/r09)
        const uint32_t last = (n - 1u) & ~3u;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const uint32_t p = (uint32_t)r * ROW + tid * 4u;
            const uint32_t at = start + (p < last ? p : last);
            const uint4 q = *reinterpret_cast<const uint4 *>(buf + at);
            kk[4 * r] = q.x, kk[4 * r + 1] = q.y, kk[4 * r + 2] = q.z, kk[4 * r + 3] = q.w;
            if (IN_VAL) {
                const uint4 w = *reinterpret_cast<const uint4 *>(vals + at);
                vv[4 * r] = w.x, vv[4 * r + 1] = w.y, vv[4 * r + 2] = w.z, vv[4 * r + 3] = w.w;
            } else {
                vv[4 * r] = vv[4 * r + 1] = vv[4 * r + 2] = vv[4 * r + 3] = 0u;
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < kNwHashItems; ++i) {
            const uint32_t p = (uint32_t)i * ROW + tid;
            const uint32_t at = start + (p < n ? p : n - 1u);
            kk[i] = buf[at];
            vv[i] = IN_VAL ? vals[at] : 0u;
        }
    }
    // (the loads are in flight while the table is cleared; four ds_write_b128 per thread instead of this loop were
    // measured and did not move the kernel: profiles/r11)
    for (uint32_t s = tid; s < kNwHashSlots; s += kNwHashThreads) {
        tab[s] = kNwEmpty;
        if (OP != 0) pay[s] = 0;
    }
    if (tid < 4) scan_tmp[12 + tid] = 0;
    __syncthreads();
    BBK_PH(4, 0, t_prev);  // table cleared
#ifdef BBK_PHASE_PROF
#pragma unroll
    for (int i = 0; i < kNwHashItems; ++i) asm volatile("" : "+v"(kk[i]));
    BBK_PH(4, 1, t_prev);  // records loaded
#endif
    uint32_t firsts = 0;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        if ((uint32_t)r * ROW < n)
            firsts |= nw_insert_row<OP, NR>(tab, pay, scan_tmp, kk + r * NR, vv + r * NR, (uint32_t)r * ROW + tid * NR,
                                            (uint32_t)(r + 1) * ROW <= n, n, max_probes)
                      << (r * NR);
    }
    return firsts;
}

#ifdef BBK_AB_HASH32_OLD  // (A/B: the front half as before round 11 -- sixteen clamped dword loads, a cleared-slot loop,
                          // every record inserted under its own predicates and probe loop, nw_slot(nw_mix(lo)))
template <int OP>
__device__ __forceinline__ uint32_t nw_hash32_records(const uint32_t *__restrict__ buf, const uint32_t *__restrict__ vals,
                                                      uint32_t *tab, uint32_t *pay, uint32_t *scan_tmp, uint32_t start,
                                                      uint32_t n, uint32_t max_probes, uint32_t (&kk)[kNwHashItems],
                                                      unsigned long long &t_prev) {
    constexpr bool IN_VAL = OP >= 2;
    constexpr uint32_t EMPTY = kNwEmpty;
    const uint32_t tid = threadIdx.x;
    uint32_t vv[kNwHashItems];
#pragma unroll
    for (int i = 0; i < kNwHashItems; ++i) {  // (the loads are in flight while the table is cleared)
        const uint32_t p = (uint32_t)(i * kNwHashThreads) + tid;
        const uint32_t at = start + (p < n ? p : n - 1u);
        kk[i] = buf[at];
        vv[i] = IN_VAL ? vals[at] : 0u;
    }
    for (uint32_t s = tid; s < kNwHashSlots; s += kNwHashThreads) {
        tab[s] = EMPTY;
        if (OP != 0) pay[s] = 0;
    }
    if (tid < 4) scan_tmp[12 + tid] = 0;
    __syncthreads();
    BBK_PH(4, 0, t_prev);  // table cleared
#ifdef BBK_PHASE_PROF
#pragma unroll
    for (int i = 0; i < kNwHashItems; ++i) asm volatile("" : "+v"(kk[i]));
    BBK_PH(4, 1, t_prev);  // records loaded
#endif
    uint32_t firsts = 0;  // bit i: record i of this lane was the first of its key in the table
#pragma unroll
    for (int i = 0; i < kNwHashItems; ++i) {
        const uint32_t p = (uint32_t)(i * kNwHashThreads) + tid;
        if (p < n) {
            if (kk[i] == EMPTY) {
                scan_tmp[13] = 1;
                nw_pay<OP>(&scan_tmp[12], vv[i]);
                continue;
            }
            uint32_t slot = nw_hslot(kk[i]);
            uint32_t probes = 0;
            for (;;) {
                const uint32_t old = atomicCAS(&tab[slot], EMPTY, kk[i]);
                if (old == EMPTY) firsts |= 1u << i;
                if (old == EMPTY || old == kk[i]) break;
                slot = (slot + 1) & (kNwHashSlots - 1);
                if (++probes > max_probes) {
                    scan_tmp[14] = 1;
                    break;
                }
            }
            if (OP != 0) nw_pay<OP>(&pay[slot], vv[i]);
        }
    }
    return firsts;
}
#endif

template <int OP>
__global__ __launch_bounds__(kNwHashThreads) void k_bucket_hash32(uint32_t *__restrict__ buf,
                                                                 uint32_t *__restrict__ vals, BucketArgs A,
                                                                 const uint16_t *__restrict__ bucket_seg, int hb) {
    constexpr uint32_t EMPTY = kNwEmpty;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *tab = reinterpret_cast<uint32_t *>(smem);
    uint32_t *pay = tab + kNwHashSlots;
    uint32_t *scan_tmp = pay + (OP != 0 ? kNwHashSlots : 0);  // [0..7] wave totals, [12] payload of the all-ones record,
                                                              // [13] its presence, [14] give-up flag, [15] output base
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t b = blockIdx.x;
#ifdef BBK_PHASE_PROF
    unsigned long long t_prev = clock64();
#else
    unsigned long long t_prev = 0;
    (void)t_prev;
#endif
    uint32_t start, n;
    bucket_range(A, b, &start, &n);
    if (n == 0) {
        if (tid == 0) A.dcount[b] = 0;
        return;
    }
    if (n > (uint32_t)(kNwHashThreads * kNwHashItems)) {
        if (tid == 0) A.dcount[b] = 0xFFFFFFFFu;
        return;
    }
    uint32_t kk[kNwHashItems];
    uint32_t firsts;  // bit i: record kk[i] of this lane was the first of its key in the table
#ifdef BBK_AB_HASH32_OLD
    firsts = nw_hash32_records<OP>(buf, vals, tab, pay, scan_tmp, start, n, A.max_probes, kk, t_prev);
#else
    if (A.slot_cap) firsts = nw_hash32_rows<OP, 4>(buf, vals, tab, pay, scan_tmp, start, n, A.max_probes, kk, t_prev);
    else firsts = nw_hash32_rows<OP, 1>(buf, vals, tab, pay, scan_tmp, start, n, A.max_probes, kk, t_prev);
#endif
    __syncthreads();
    BBK_PH(4, 2, t_prev);  // inserted
    if (scan_tmp[14]) {  // the table is (nearly) full: nothing has been written, the caller takes over
        if (tid == 0) A.dcount[b] = 0xFFFFFFFFu;
        return;
    }
    constexpr int SPT = kNwHashSlots / kNwHashThreads;
    uint32_t cnt = 0;
    if constexpr (OP == 0 && kHashDirectOut) {
        cnt = (uint32_t)__popc(firsts);  // no payload to fetch: whoever put a key into the table writes it out -- no walk
    } else {                             // over the 8192 slots
#pragma unroll
        for (int j = 0; j < SPT; ++j) cnt += tab[j * kNwHashThreads + tid] != EMPTY ? 1u : 0u;
    }
    uint32_t incl = cnt;
    incl = wave_scan_incl(incl);
    if (lane == 63) scan_tmp[wave] = incl;
    __syncthreads();
    uint32_t wbase, total;
    wave_totals<kNwHashThreads / 64>(scan_tmp, lane, wave, wbase, total);
    const uint32_t extra = scan_tmp[13] ? 1u : 0u;
    // The distinct records (4 bytes, still without their segment) go back to the head of the bucket's own slot; a
    // pass over the bucket counts gives the offsets of the dense result and k_compact_narrow widens them into it.
    // (Until round 3 every bucket reserved its place in the result with an atomicAdd on ONE counter: 227 210 buckets at
    // BASELINE configs[1], served one after the other at ~11 ns each -- 2.6 ms of the kernel's 2.8,
    // tools/probes/single_counter_probe.hip.)  Every record of the bucket has been loaded AND used before the barrier
    // that follows the insertions: nothing is overwritten before it has been read.
    uint32_t o = start + wbase + incl - cnt;
    if constexpr (OP == 0 && kHashDirectOut) {
        // (the loaded records are awaited here by every lane: the insertion loop used them under `p < n` only, and the
        // compiler would otherwise wait for them -- vmcnt 0 -- in front of every store below)
#pragma unroll
        for (int i = 0; i < kNwHashItems; ++i) asm volatile("" : "+v"(kk[i]));
#pragma unroll
        for (int i = 0; i < kNwHashItems; ++i) {
            if (firsts & (1u << i)) buf[o++] = kk[i];
        }
    } else {
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            const uint32_t rec = tab[j * kNwHashThreads + tid];
            if (rec != EMPTY) {
                buf[o] = rec;
                if (OP != 0) vals[o] = pay[j * kNwHashThreads + tid];
                ++o;
            }
        }
    }
    BBK_PH(4, 3, t_prev);  // compaction + output
#ifdef BBK_PHASE_PROF
    if (threadIdx.x == 0) atomicAdd(&g_phase[4][7], 1ull);
#endif
    if (tid == 0) {
        if (extra) {
            buf[start + total] = EMPTY;
            if (OP != 0) vals[start + total] = scan_tmp[12];
        }
        A.dcount[b] = total + extra;
    }
}

// one wave per bucket of the narrow path: the distinct 4-byte records at the head of every bucket slot -> 8-byte keys
// (nw_key: the segment gives the high bits) at their place in the dense result
template <bool HAS_VAL>
__global__ __launch_bounds__(256) void k_compact_narrow(const uint32_t *__restrict__ buf, const uint32_t *__restrict__ vals,
                                                       const uint32_t *__restrict__ dcount, const uint64_t *__restrict__ doff,
                                                       uint32_t nbuckets, uint32_t slot_stride,
                                                       const uint16_t *__restrict__ bucket_seg, int hb,
                                                       uint64_t *__restrict__ out, uint32_t *__restrict__ vout) {
    const uint32_t b = (uint32_t)((BBK_GID()) >> 6);
    if (b >= nbuckets) return;
    const int lane = threadIdx.x & 63;
    uint32_t c = dcount[b];
    if (c == 0xFFFFFFFFu) c = 0;  // left to the caller (reprocessed with the spill list)
    const uint32_t s = b * slot_stride, seg = bucket_seg[b];
    const uint64_t d = doff[b];
    for (uint32_t i = lane; i < c; i += 64) {
        out[d + i] = nw_key(seg, buf[s + i], hb);
        if (HAS_VAL) vout[d + i] = vals[s + i];
    }
}

template <int OP>
static size_t bucket_hash32_smem() {
    return sizeof(uint32_t) * kNwHashSlots * (OP != 0 ? 2 : 1) + sizeof(uint32_t) * 16;
}

// 4-byte records of one segment -> 8-byte keys (overflowing slots are reprocessed by the exact path on a key array)
__global__ void k_nw_widen(const uint32_t *__restrict__ in, uint32_t n, uint32_t seg, int hb, uint64_t *__restrict__ out) {
    const uint32_t i = (uint32_t)BBK_GID();  // cnt is a 32-bit count
    if (i < n) out[i] = nw_key(seg, in[i], hb);
}

}  // namespace bbk
