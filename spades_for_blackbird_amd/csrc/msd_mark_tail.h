// msd_mark_tail.h -- the mark-bit scatter tail of k_part_reads_narrow, k_part_narrow2 (msd_narrow_a.h), k_part_view_lt
// and k_part_lt2 (msd_stage_b.h), and the rank-of-a-position helper that k_part_view_lt also uses to find the bucket of a key.
// The layout and the index arithmetic are plain functions, so that the host can run them too
// (tests/mark_tail_check.cpp); the tail itself is device code and needs msd_part.h in front of it.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BBK_MARK_HD __host__ __device__
#else
#define BBK_MARK_HD
#endif

namespace bbk {

// ---- rank of a position among runs ------------------------------------------------------------------------
// Positions 0 .. n-1 are cut into consecutive runs; position 0 always starts one.  Bit p of the mark set says "a run
// starts at position p + 1", so the rank of the run that owns position pos is the number of marks BELOW bit pos: an
// exclusive count, which for pos = 64 * w + lane is what v_mbcnt gives for the word w of a wave, on top of the marks of
// the words before it.  One 16-byte entry per 64 positions holds the word and that prefix: one LDS read per wave step.
struct alignas(16) MarkWord {
    uint32_t lo, hi;  // marks of positions 64 w + 1 .. 64 w + 64 (bit p: a run starts at 64 w + p + 1)
    uint32_t before;  // marks in the words below w
    uint32_t pad;
};

BBK_MARK_HD inline uint32_t mark_words(uint32_t positions) { return (positions + 63u) >> 6; }
// a run that starts at `start` > 0: where its mark lies in the entries seen as 32-bit words (four per entry), and the bit
BBK_MARK_HD inline uint32_t mark_slot32(uint32_t start) {
    const uint32_t s = start - 1u;
    return ((s >> 6) << 2) | ((s >> 5) & 1u);
}
BBK_MARK_HD inline uint32_t mark_bit32(uint32_t start) { return 1u << ((start - 1u) & 31u); }
BBK_MARK_HD inline uint32_t mark_count(uint32_t lo, uint32_t hi) {
    return (uint32_t)__builtin_popcount(lo) + (uint32_t)__builtin_popcount(hi);
}
// rank of the run of position 64 w + lane, from the entry of word w.  On the device `lane` must be the lane that asks
// (two v_mbcnt, the prefix rides in as their addend); the host form takes any lane < 64.
BBK_MARK_HD inline uint32_t mark_rank(uint32_t lo, uint32_t hi, uint32_t before, uint32_t lane) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)lane;
    return __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, before));
#else
    const uint32_t mlo = lane >= 32u ? 0xFFFFFFFFu : (1u << lane) - 1u;
    const uint32_t mhi = lane <= 32u ? 0u : (1u << (lane - 32u)) - 1u;
    return before + mark_count(lo & mlo, hi & mhi);
#endif
}

// ---- the buckets of a tile of the bucket view (k_part_view_lt) ---------------------------------------------
// A tile covers the dense positions c0 .. c0 + n - 1; bucket i of its span starts at off_i (off_0 <= c0 < off_1: the
// span's first bucket is the last one that starts at or before c0).  Buckets that start where the next one starts are
// empty and take no part: they would collide in the bit set, and no position is theirs.
BBK_MARK_HD inline uint32_t view_run_start(uint64_t off_i, uint64_t c0) { return off_i > c0 ? (uint32_t)(off_i - c0) : 0u; }
BBK_MARK_HD inline bool view_bucket_live(uint32_t i, uint32_t span, uint64_t off_i, uint64_t off_next) {
    return i + 1u == span || off_next != off_i;
}

#if defined(__HIPCC__)

// ---- the tail ----------------------------------------------------------------------------------------------
// The staged order is bin-major, a mark per position says where a non-empty bin starts (above), and what a store needs
// of its bin sits in one 8-byte entry indexed by the rank r of its run: the bin of a staged record is never computed
// twice.  kMaxBins threads, one bin per thread in the scans.
typedef __attribute__((address_space(1))) uint32_t MarkGlobalWord;

struct MarkLds {
    uint32_t *lhist;          // counts; later, with the 4 KB behind it:
    unsigned long long *tab;  // r -> byte address of staged position 0 in the run's slot (no overflow in the tile), or
                              //      (global offset - staged start, first staged position past the slot)
    uint32_t *lstart, *scan_tmp;
    MarkWord *mw;             // marks and their prefixes
    uint16_t *nz;             // the r-th non-empty bin
    uint32_t *stage;
    uint8_t *vstage;          // payload bytes (the extension index), behind the stage
};
template <int TILE>
__device__ __forceinline__ MarkLds mark_lds(unsigned char *smem) {
    MarkLds S;
    S.lhist = reinterpret_cast<uint32_t *>(smem);
    S.tab = reinterpret_cast<unsigned long long *>(smem);
    S.lstart = S.lhist + 2 * kMaxBins;
    S.scan_tmp = S.lstart + kMaxBins;  // 64 entries: [0, 16) wave totals, [32] some run of the tile overflows its slot
    S.mw = reinterpret_cast<MarkWord *>(S.scan_tmp + 64);
    S.nz = reinterpret_cast<uint16_t *>(S.mw + TILE / 64);
    S.stage = reinterpret_cast<uint32_t *>(S.nz + kMaxBins);
    S.vstage = reinterpret_cast<uint8_t *>(S.stage + TILE);
    return S;
}
static size_t mark_smem(size_t tile) {
    return sizeof(uint32_t) * (3 * kMaxBins + 64) + (tile / 64) * sizeof(MarkWord) + (size_t)kMaxBins * 2;
}
// before the histogram: counts and marks to zero (a barrier follows at the caller)
template <int TILE>
__device__ __forceinline__ void mark_clear(const MarkLds &S, uint32_t tid) {
    static_assert(4 * (TILE / 64) <= kMaxBins, "one 32-bit word of the marks per thread");
    S.lhist[tid] = 0;
    if (tid < 4u * (TILE / 64)) reinterpret_cast<uint32_t *>(S.mw)[tid] = 0u;
}

// one wave: the prefixes of n words of marks (lane l owns words WPL * l .. WPL * l + WPL - 1)
template <int MW>
__device__ __forceinline__ void mark_prefix(MarkWord *mw, int lane) {
    constexpr int WPL = (MW + 63) / 64;
    uint32_t pw[WPL], tot = 0;
#pragma unroll
    for (int j = 0; j < WPL; ++j) {
        const int idx = lane * WPL + j;
        pw[j] = tot;
        if (idx < MW) {
            const uint2 m = *reinterpret_cast<const uint2 *>(&mw[idx]);
            tot += mark_count(m.x, m.y);
        }
    }
    uint32_t inc2 = tot;
    inc2 = wave_scan_incl(inc2);
    const uint32_t lb = inc2 - tot;
#pragma unroll
    for (int j = 0; j < WPL; ++j) {
        const int idx = lane * WPL + j;
        if (idx < MW) mw[idx].before = lb + pw[j];
    }
}

// rank of the run of staged position i * kMaxBins + tid: the wave's word of step i
template <int NT>
__device__ __forceinline__ uint32_t mark_rank_at(const MarkWord *wmw, int i, int lane) {
    const uint4 m = *reinterpret_cast<const uint4 *>(&wmw[i * (NT / 64)]);
    return mark_rank(m.x, m.y, m.z, (uint32_t)lane);
}

// On entry lhist[b] = records of bin b in this tile and bin_of_item(i) = the bin of item i (0xFFFFFFFF: no record);
// the place inside the bin is taken here, with a second atomic after the scan.  RANKED: the caller's counting atomic
// has returned that place already and bin_of_item(i) = bin << 16 | place (k_part_narrow2, whose bins and places fit
// sixteen bits each).  lo[i] is the item's record, val_of(i) its payload byte (HAS_VAL).  cur / slot_end: cursor and end of
// the slot of bin `tid`.  The stored record is lo | rec_or.  before_stores() runs between the last barrier and the
// stores (k_part_reads_narrow starts the next tile's loads there).
//
// Whether every run of the tile fits its slot is known when the bin threads write the table (room >= count) and
// travels through the barrier that is there anyway, as one LDS word.  If all fit -- the rule: spills are rare -- an
// entry is the byte address out + 4 * (reservation - staged start) and a store is that plus 4 * position: no limit, no
// second exec region.  Otherwise the bin threads rewrite their entries as (offset, limit) and the tile takes the loop
// with the limit test and the spill loop behind it.  Both loops store the same records to the same places.
template <int TILE, int ITEMS, bool HAS_VAL, bool RANKED = false, class BinOf, class ValOf, class KeyOf, class Hook>
__device__ __forceinline__ void mark_tail(const MarkLds &S, const uint32_t (&lo)[ITEMS], uint32_t tid, uint32_t nb,
                                          uint32_t *__restrict__ cur, uint64_t slot_end, uint32_t rec_or, const PartLevel &L,
                                          uint32_t *__restrict__ out, uint32_t *__restrict__ vout, BinOf bin_of_item,
                                          ValOf val_of, KeyOf key_of, Hook before_stores) {
    constexpr int NT = kMaxBins, MW = TILE / 64;  // TILE: the staged positions the LDS layout was made for
    static_assert(ITEMS <= 32 && TILE <= NT * ITEMS && NT * ITEMS < 65536, "one bit per item, 16-bit positions");
    const int lane = tid & 63, wave = tid >> 6;
    const uint32_t c = tid < nb ? S.lhist[tid] : 0u;
    uint32_t incl = c;
    incl = wave_scan_incl(incl);
    const unsigned long long nzb = __ballot(c != 0);
    if (lane == 63) S.scan_tmp[wave] = incl | ((uint32_t)__popcll(nzb) << 16);  // records < 2^16, non-empty bins <= 1024
    if (tid == 0) S.scan_tmp[32] = 0;
    __syncthreads();
    uint32_t before, total;
    wave_totals<NT / 64>(S.scan_tmp, lane, wave, before, total);
    const uint32_t staged = total & 0xFFFFu;
    const uint32_t ex = (before & 0xFFFFu) + incl - c;
    const uint32_t myr = (before >> 16) + (uint32_t)__popcll(nzb & ((1ull << lane) - 1ull));
    S.lstart[tid] = ex;
    uint32_t greserve = 0;
    if (c) {
        greserve = atomicAdd(cur, c);  // issued now, consumed after the LDS reorder
        S.nz[myr] = (uint16_t)tid;
        if (ex) atomicOr(&reinterpret_cast<uint32_t *>(S.mw)[mark_slot32(ex)], mark_bit32(ex));
    }
    __syncthreads();  // (every thread has read its count: lhist may become the table)
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t bin = bin_of_item(i);
        if (bin != 0xFFFFFFFFu) {
            // (lstart ends as the bins' end offsets; nothing reads it again.  RANKED: it stays, bin << 16 | place)
            const uint32_t pos = RANKED ? S.lstart[bin >> 16] + (bin & 0xFFFFu) : atomicAdd(&S.lstart[bin], 1u);
            S.stage[pos] = lo[i];
            if (HAS_VAL) S.vstage[pos] = (uint8_t)val_of(i);
        }
    }
    asm volatile("" : "+v"(greserve));  // awaited by every lane here, not inside the store loop's conditional blocks
    int64_t room = 0;
    if (c) {
        room = (int64_t)slot_end - (int64_t)greserve;
        S.tab[myr] = (unsigned long long)(uintptr_t)out + 4ull * (unsigned long long)((int64_t)greserve - (int64_t)ex);
        if (room < (int64_t)c) S.scan_tmp[32] = 1;
    }
    if (wave == 0) mark_prefix<MW>(S.mw, lane);
    __syncthreads();
    before_stores();
    const MarkWord *wmw = S.mw + wave;  // pos = i * NT + tid: the 64 lanes of a wave cover word i * (NT / 64) + wave
#ifdef BBK_AB_NO_MARK_FAST  // (A/B: every tile takes the loop with the limit test)
    const bool over = true;
#else
    const bool over = __builtin_amdgcn_readfirstlane((int)S.scan_tmp[32]) != 0;  // uniform
#endif
    if (!over) {
        const unsigned long long vdelta = (unsigned long long)((uintptr_t)vout - (uintptr_t)out);
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            // (one row per predicated region.  Full rows in groups of 4 to 7 without a predicate, their LDS reads sent
            // out together, were measured: the stores then leave in bursts and both stage-A level 1 and k_part_lt2 get
            // slower -- profiles/mark_tail)
            const uint32_t pos = (uint32_t)i * NT + tid;
            if (pos < staged) {
                const uint32_t r = mark_rank_at<NT>(wmw, i, lane);
                const unsigned long long a = S.tab[r] + ((unsigned long long)pos << 2);
                *reinterpret_cast<MarkGlobalWord *>(a) = S.stage[pos] | rec_or;
                if (HAS_VAL) *reinterpret_cast<MarkGlobalWord *>(a + vdelta) = S.vstage[pos];
            }
        }
        return;
    }
    if (c) {  // (no thread reads the table in its first form on this path)
        // first staged position of this bin that no longer fits its slot
        S.tab[myr] = (unsigned long long)(greserve - ex) |
                     ((unsigned long long)((uint32_t)(int32_t)(room < -(int64_t)0x7FFF0000 ? -(int64_t)0x7FFF0000 : room) + ex) << 32);
    }
    __syncthreads();
    uint32_t full = 0;  // items whose slot is full (handled after the stores so that no atomic sits between them)
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t pos = (uint32_t)i * NT + tid;
        if (pos < staged) {
            const uint32_t r = mark_rank_at<NT>(wmw, i, lane);
            unsigned long long e = S.tab[r];
            const uint32_t rec = S.stage[pos];
            asm volatile("" : "+v"(e));  // one 8-byte LDS read (otherwise: the limit, a branch, then the offset)
            if ((int32_t)pos >= (int32_t)(uint32_t)(e >> 32)) {
                full |= 1u << i;
            } else {
                const uint32_t g = (uint32_t)e + pos;
                out[g] = rec | rec_or;
                if (HAS_VAL) vout[g] = S.vstage[pos];
            }
        }
    }
    if (full) {
#pragma unroll 1
        for (int i = 0; i < ITEMS; ++i) {
            if ((full >> i) & 1u) {
                const uint32_t pos = (uint32_t)i * NT + tid;
                const uint32_t r = mark_rank_at<NT>(wmw, i, lane);
                const uint32_t sp = atomicAdd(L.spill_count, 1u);
                if (sp < L.spill_cap) {
                    reinterpret_cast<uint64_t *>(L.spill_keys)[sp] = key_of((uint32_t)S.nz[r], S.stage[pos]);
                    if (HAS_VAL) L.spill_vals[sp] = S.vstage[pos];
                }
            }
        }
    }
}

#endif  // __HIPCC__

}  // namespace bbk
