// msd.hip -- the fast sort-and-count path: two MSD radix-partition levels in HBM, then one
// workgroup per bucket deduplicates / sorts + reduces its keys entirely in LDS.
//
// Why: the LSD path (primitives.hip) moves every record 3x per 8-bit pass (k=21: 6 passes, ~19 N*W
// bytes).  Here a record is written by the (fused) extraction+partition, read and written once
// more by the second partition level and read once by the bucket kernel, independent of the key
// length, and the duplicate-heavy k-mer stream (50x coverage) collapses inside LDS.
//
//   k_part_reads : fused k-mer extraction (chunks of one read per lane, rolled) + level-1 partition:
//                  LDS histogram with returning ds_add = local rank, one global atomicAdd per
//                  (tile, non-empty bin) reserves the output run, keys reordered in LDS so that a
//                  wave stores contiguous per-bin runs (unstable: the buckets get sorted later)
//   k_part       : the same over a key array (levels 1 and 2); <HIST> variants only count
//   k_bucket_hash / k_bucket_hashidx : one bucket in an LDS open-addressing table: dedup + reduce
//                  (HASH prefix: the order does not matter)
//   k_bucket_dist: one bucket sorted in LDS by one distribution pass + in-bin ranking, head flags +
//                  segmented reduce (count / sum / OR); k_bucket (ballot-ranked LSD radix) is the
//                  second chance for crowded bins and oversized buckets
//   k_compact    : buckets -> dense output
//
// Two modes (MsdRunner::run): the exact mode counts every level first (histogram kernels, dense
// layout); the slot mode (HASH prefix) gives segments and buckets fixed slots and sends what does
// not fit to a spill list that the exact mode finishes -- no histogram passes.
//
// The partition digit comes from a 32-bit "prefix" p(key): HASH (multiplicative mix: uniform whatever
// the sequence composition; used when only the distinct set matters), KEYS (the key's own top bits:
// output globally ascending) or REF (XXH3 bucket of 16, then key bits: the final_kmers order,
// reference kmer_buckets.hpp:28-33 + kmer_index_builder.hpp:168-181).  Level 2 maps the
// remaining prefix bits monotonically onto nb2 bins, so bucket order == prefix order.
// Buckets larger than CAP (a k-mer repeated thousands of times, skewed composition in KEYS mode)
// are finished by the LSD path, per bucket; if too much overflows the caller falls back entirely.
// Environment knobs (tests / diagnostics): MsdKnobs lists them all; -DBBK_PHASE_PROF builds per-phase shader clocks
// into the kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <type_traits>
#include <vector>

#include "bbk_internal.h"
#include "kmer_ops.h"
#include "msd.h"

namespace bbk {

// Partition tile of a key array: 8192 records of 8 B (4096 of 16 B) staged in LDS, 512 threads x 16
// (x 8) items so the loads stay wide.  Reads are partitioned by k_part_reads (own geometry below).
#ifndef BBK_KEYS_TILE
#define BBK_KEYS_TILE 8192
#endif
#ifndef BBK_KEYS_THREADS
#define BBK_KEYS_THREADS 512
#endif
template <int W>
struct PartCfg {
    static constexpr int TILE = (W == 1) ? BBK_KEYS_TILE : (W == 2 ? 4096 : 2048);  // 64 KB / 48 KB / 64 KB of LDS
    static constexpr int THREADS = BBK_KEYS_THREADS;
    static constexpr int ITEMS = TILE / THREADS;
};
// Fused extraction + level-1 partition: a lane owns one CHUNK of up to CH consecutive k-mer positions of
// ONE read (8-byte keys: 8, rolled base by base; wider keys: 4), a workgroup 1024 chunks.
constexpr int kRdThreads = 1024;      // scatter: big tiles, long per-bin runs
constexpr int kRdHistThreads = 512;   // histogram: nothing is staged, four workgroups per CU hide the prologues
constexpr int kRdSlots = 1024;  // reads of one tile whose cursor tables fit LDS
constexpr int kRdWords = 2048;  // packed read words of one tile staged in LDS (150 bp reads need ~330)
template <int W>
struct RdCfg {
    static constexpr int CH = (W == 1) ? 8 : (W == 2 ? 4 : 2);  // records of a tile: 64 KB (48 KB for 24-byte keys)
    static constexpr int TILE = kRdThreads * CH;
};
constexpr int kMaxBins = 1024;

// 32-bit partition prefix: bucket order == prefix order (only ~20 top bits are ever consumed)
template <int W>
__device__ inline uint32_t prefix_of(const Key<W> &key, int dmode, int w0bits) {
    if (dmode == MSD_HASH) return part_hash32<W>(key);
    const uint64_t top = (w0bits >= 64) ? key.w[0] : (key.w[0] << (64 - w0bits));
    if (dmode == MSD_KEYS) return (uint32_t)(top >> 32);
    const uint32_t b = (uint32_t)__umul64hi(xxh3_64<W>(key), 16ull);
    return (b << 28) | (uint32_t)(top >> 36);
}

struct PartLevel {
    int level;        // 1 or 2
    int b1;           // log2(nb1)
    uint32_t nb1;
    int dmode;
    int w0bits;
    // level 2: every level-1 segment gets its own bin count (sized from its record count, so a
    // skewed prefix distribution still gives buckets of the target size) and flat bin base
    const uint32_t *seg_nb2;
    const uint32_t *seg_bin_start;
    // range pass (inputs above one device batch): only records whose prefix lies in [sel_lo, sel_lo + sel_span)
    // take part (sel_span == 0: all of them); the prefix inside the range, (p - sel_lo) << sel_shl, drives the bins.
    // HASH prefix: 2^b equal hash ranges; KEYS / REF prefix: ranges of the key space sized from a histogram, so the
    // concatenated passes are in prefix order.
    uint32_t sel_lo;
    uint32_t sel_span;
    int sel_shl;
    uint32_t sel_mul;  // stretches (p - sel_lo) << sel_shl, which only reaches span << shl, over the whole 32 bits
    // slot mode (histogram-free HASH path): bin g of this level owns the fixed range [g*slot_cap, (g+1)*slot_cap) of
    // the output and `cursor[g]` starts at g*slot_cap; records that do not fit are appended to the spill list
    uint32_t slot_cap;     // 0: dense layout from an exact histogram
    uint32_t slot_stride;  // distance between slots (>= slot_cap; padded so that slots do not alias in HBM channels)
    void *spill_keys;      // Key<W>[spill_cap]
    uint32_t *spill_vals;  // payloads alongside (records with a payload)
    uint32_t *spill_count; // records appended (may run past spill_cap: the host checks)
    uint32_t spill_cap;
    // narrow stage A (8-byte keys, 2k - 32 = narrow_hb in [1, 10]): 4-byte records between the levels, see "narrow" below
    int narrow_hb;
    // narrow level 1: every segment slot is cut into 2^xcd_shift sub-slots of sub_cap records, one per XCD, with a
    // cursor each (cursor[(bin << xcd_shift) + xcc]).  A (tile, bin) run is ~60 bytes and starts wherever the last one
    // ended; with one fill front per bin a 128-byte line is filled by workgroups on different XCDs, i.e. through
    // different L2s, which is slow (see the call site).  With a fill front per (bin, XCD) every line is one XCD's.  Level 2
    // reads the sub-slots as segments of their own and sends them to the buckets of the parent segment.
    int xcd_shift;
    uint32_t sub_cap;
};

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
__device__ inline uint64_t nw_key(uint32_t bin1, uint32_t lo, int hb) {
    const uint32_t hi = (bin1 ^ (nw_mix(lo) >> 22)) >> (10 - hb);
    return ((uint64_t)hi << 32) | lo;
}

// applies the range selection: false = the record belongs to another pass; p loses the selection bits
__device__ inline bool select_prefix(uint32_t &p, const PartLevel &L) {
    if (L.sel_span == 0) return true;
    const uint32_t d = p - L.sel_lo;
    if (d >= L.sel_span) return false;
    // a span that is not a power of two would leave the top of the prefix space (up to half of the bins) empty and
    // crowd the rest: scale by 2^32 / (span << shl) in (1, 2], monotone (bucket order = prefix order is kept)
    p = d << L.sel_shl;
    p += __umulhi(p, L.sel_mul);
    return true;
}

// bin of this level inside its segment (nb = bins of the segment at level 2)
__device__ inline uint32_t bin_of(uint32_t p, const PartLevel &L, uint32_t nb) {
    if (L.level == 1) return L.b1 == 0 ? 0u : (p >> (32 - L.b1));
    const uint32_t rest = L.b1 == 0 ? p : (p << L.b1);
    return __umulhi(rest, nb);
}

struct ReadSrc {
    const uint64_t *words;
    const uint64_t *woff;
    const uint32_t *len;
    const uint64_t *coff;       // exclusive scan of chunks per read (n_reads + 1)
    const struct RdTile *tiles;  // per tile: its reads and the window of packed words to stage (k_tile_reads)
    uint64_t n_reads;
    uint64_t n_chunks;
    int k;
};

// largest r in [0, nr) with s_rel[r] <= c
__device__ inline uint32_t read_of(const int32_t *s_rel, uint32_t nr, int32_t c) {
    uint32_t lo = 0, hi = nr;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s_rel[mid] <= c) lo = mid;
        else hi = mid;
    }
    return lo;
}

// What a workgroup of k_part_reads needs to start on a tile, precomputed so that its prologue is ONE scalar load
// followed by the coalesced table/word copies instead of three dependent global round trips.
struct RdTile {
    uint64_t wbase;  // first packed word of the staged window
    uint32_t r0;     // read holding the tile's first chunk
    uint32_t nr;     // reads r0 .. r0+nr-1 own chunks of (or lie inside) the tile
    uint32_t wspan;  // words of the window; 0xFFFFFFFF: does not fit LDS / not in read order (global-memory path)
    uint32_t pad;
};

// largest r in [0, n_reads) with off[r] <= j
__device__ inline uint64_t read_at(const uint64_t *__restrict__ off, uint64_t n_reads, uint64_t j) {
    uint64_t lo = 0, hi = n_reads;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (off[mid] <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}

// one thread per tile of `tile` chunks (a chunk = ch k-mer positions of one read).  Two tilings of the same reads in
// one launch: threads [0, n_tiles) describe the tiles of `tile` chunks into out, the next n_tiles_b threads those of
// tile_b chunks into out_b (the scatter and the histogram kernels of level 1 have different workgroup sizes).
__global__ void k_tile_reads(const uint64_t *__restrict__ coff, const uint64_t *__restrict__ woff,
                             const uint32_t *__restrict__ len, uint64_t n_reads, uint64_t n_tiles, uint32_t tile,
                             RdTile *__restrict__ out, uint64_t n_tiles_b, uint32_t tile_b, RdTile *__restrict__ out_b,
                             uint32_t ch, uint32_t k, uint32_t max_reads, uint32_t max_words,
                             const uint32_t *__restrict__ unordered) {
    uint64_t t = BBK_GID();
    if (t >= n_tiles) {
        t -= n_tiles;
        if (t >= n_tiles_b) return;
        tile = tile_b;
        out = out_b;
    }
    const uint64_t c0 = t * (uint64_t)tile;
    const uint64_t r0 = read_at(coff, n_reads, c0), r1 = read_at(coff, n_reads, c0 + tile);
    // staged word window: from the word of the first base this tile touches in r0 (one base before the chunk,
    // for the incoming-edge bit) to the last word it can touch in r1
    const uint32_t p0 = (uint32_t)(c0 - coff[r0]) * ch;
    const uint64_t wbase = woff[r0] + ((p0 ? p0 - 1u : 0u) >> 5);
    const uint32_t len1 = len[r1];
    const uint64_t span1 = (c0 + tile - coff[r1]) * ch + k;  // base index the tile can reach in r1
    const uint32_t lastb1 = len1 ? (uint32_t)(span1 < (uint64_t)(len1 - 1u) ? span1 : (uint64_t)(len1 - 1u)) : 0u;
    const uint64_t wend = woff[r1] + (len1 ? (lastb1 >> 5) + 1u : 0u);
    const uint64_t nr = r1 - r0 + 1;
    // words in read order (checked once for all reads): every read of the tile then lies inside [wbase, wend)
    const bool fast = *unordered == 0 && nr <= (uint64_t)max_reads && wend >= wbase && wend - wbase <= (uint64_t)max_words;
    RdTile T;
    T.wbase = wbase;
    T.r0 = (uint32_t)r0;
    T.nr = (uint32_t)nr;
    T.wspan = fast ? (uint32_t)(wend - wbase) : 0xFFFFFFFFu;
    T.pad = 0;
    out[t] = T;
}

// Tile -> (segment, range).  Level 1: tile t covers records [t*TILE, ...).  Level 2: tiles never
// straddle a level-1 bin: seg_tile_start[b] = first tile of bin b (nb1 + 1 entries).
struct TileMap {
    const uint32_t *seg_tile_start;  // null for level 1
    const uint32_t *seg_off;         // record offset of every level-1 bin (nb1 + 1), level 2 only
    const uint32_t *seg_size;        // records of every level-1 bin; null: seg_off[s + 1] - seg_off[s] (dense)
    uint32_t nseg;
    uint64_t n;
    uint32_t ntiles;  // tiles of the level
    uint32_t group;   // histogram kernels: consecutive tiles one workgroup walks
    const uint4 *desc;  // level 2: per tile (first record, records, bins of its segment, flat index of bin 0),
                        // precomputed so that a workgroup starts with one load instead of a binary search
    // level 1 over a CANONICAL key array that is expanded on the fly: record 2c is key c, record 2c+1 its reverse
    // complement (the both-strand set of spades-kmercount; M.n counts records); expand_tag: the XXH3 bucket of 16
    // goes into bits 2k..2k+3 of either (final_kmers order by one ascending sort, see count.hip)
    int expand_k;  // 0: the array holds the records themselves
    int expand_tag;
};

// level 2: tile -> descriptor (one thread per tile)
__global__ void k_tile_desc(TileMap M, const uint32_t *__restrict__ seg_nb2, const uint32_t *__restrict__ seg_bin_start,
                            uint32_t tile_size, int sub_shift, const uint32_t *__restrict__ xstart,
                            uint4 *__restrict__ desc) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= M.ntiles) return;
    uint32_t lo = 0, hi = M.nseg;  // largest s with seg_tile_start[s] <= t
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (M.seg_tile_start[mid] <= t) lo = mid;
        else hi = mid;
    }
    const uint32_t b = M.seg_off[lo] + (t - M.seg_tile_start[lo]) * tile_size;
    const uint32_t e = M.seg_size ? M.seg_off[lo] + M.seg_size[lo] : M.seg_off[lo + 1];
    // M's entries are the level-1 segments or their per-XCD sub-slots (sub_shift); xstart: the tiles of a segment go to
    // the workgroups of one XCD (see k_tile_desc_narrow)
    const uint32_t seg = lo >> sub_shift;
    const uint32_t at = xstart ? 8u * (xstart[lo] + (t - M.seg_tile_start[lo])) + (seg & 7u) : t;
    desc[at] = make_uint4(b, (e - b) < tile_size ? (e - b) : tile_size, seg_nb2[seg], seg_bin_start[seg]);
}

struct TileInfo {
    uint64_t begin;
    uint32_t count, nb;
    uint64_t gbin0;
};

__device__ inline TileInfo tile_info(const TileMap &M, const PartLevel &L, uint32_t tile, uint32_t tile_size) {
    TileInfo T;
    if (M.desc) {
        const uint4 d = M.desc[tile];
        T.begin = d.x;
        T.count = d.y;
        T.nb = d.z;
        T.gbin0 = d.w;
    } else {  // level 1: one segment, tile t covers records [t * tile_size, ...)
        T.begin = (uint64_t)tile * tile_size;
        const uint64_t rem = M.n - T.begin;
        T.count = rem < (uint64_t)tile_size ? (uint32_t)rem : tile_size;
        T.nb = L.nb1;
        T.gbin0 = 0;
    }
    return T;
}

#ifdef BBK_PHASE_PROF
// phase clocks of the scatter kernels (diagnostic build only): [kernel kind][phase] summed shader cycles of
// thread 0 of every workgroup, [..][7] = workgroups
__device__ unsigned long long g_phase[6][8];
#define BBK_PH(kind, ph, t_prev)                                                   \
    do {                                                                           \
        if (threadIdx.x == 0) {                                                    \
            const unsigned long long t_now = clock64();                            \
            atomicAdd(&g_phase[kind][ph], t_now - t_prev);                         \
            t_prev = t_now;                                                        \
        }                                                                          \
    } while (0)
#else
#define BBK_PH(kind, ph, t_prev) \
    do {                         \
    } while (0)
#endif

// Common tail of the scatter kernels.  On entry lhist[b] = records of bin b in this tile and binrank[i] =
// bin << 16 | rank-in-bin (0xFFFFFFFF: no record).  One global atomicAdd per non-empty bin reserves the
// tile's run in that bin; the records are reordered through LDS (stage) so that a wave stores contiguous
// per-bin runs.  NOUT (narrow stage B, 8-byte keys): the output holds only the keys' low words (spills stay 8-byte).
// Inclusive prefix sum over the 64 lanes of a wave with DPP row shifts and row broadcasts: six v_add with a DPP operand.
// (__shfl_up goes through ds_bpermute: an address register per distance, an LDS-pipe operation and a select per step.)
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);  // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);  // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);  // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1, 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2, 3
    return v;
}

// Per-wave totals (nw <= 64 values in LDS, written before the last barrier) -> the sum of the waves before `wave` and
// the grand total.  Every wave scans the few values itself: log2(nw) shuffle steps instead of a loop of nw LDS reads
// per thread (which was ~80 vector instructions per thread in a workgroup of 16 waves).
template <int NW>
__device__ __forceinline__ void wave_totals(const uint32_t *tmp, int lane, int wave, uint32_t &before, uint32_t &total) {
    static_assert(NW <= 16, "one DPP row");
    const uint32_t v = lane < NW ? tmp[lane] : 0u;
    uint32_t inc = v;
    if (NW > 1) inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x111, 0xf, 0xf, false);
    if (NW > 2) inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x112, 0xf, 0xf, false);
    if (NW > 4) inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x114, 0xf, 0xf, false);
    if (NW > 8) inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x118, 0xf, 0xf, false);
    total = (uint32_t)__builtin_amdgcn_readlane((int)inc, NW - 1);
    before = (uint32_t)__builtin_amdgcn_readlane((int)(inc - v), __builtin_amdgcn_readfirstlane(wave));
}

template <int W, int ITEMS, int THREADS, int MAXB, bool HAS_VAL, bool NOUT = false>
__device__ __forceinline__ void part_tail(const Key<W> (&keys)[ITEMS], const uint32_t (&vals)[ITEMS],
                                          const uint32_t (&binrank)[ITEMS], uint32_t *lhist, uint32_t *lstart,
                                          uint32_t *goff, uint32_t *scan_tmp, Key<W> *stage, uint32_t *vstage,
                                          uint32_t nb, uint64_t gbin0, const PartLevel &L,
                                          uint32_t *__restrict__ cursor, Key<W> *__restrict__ out,
                                          uint32_t *__restrict__ vout, int prof_kind = 0,
                                          unsigned long long t_prev = 0) {
    const int tid = threadIdx.x;
    (void)prof_kind;
    (void)t_prev;
    uint32_t staged = 0;
    // level 1 in slot mode: one fill front (cursor and sub-slot) per (segment, XCD), see PartLevel::xcd_shift
    uint32_t xcc = 0;
    if (L.xcd_shift) {
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        xcc &= (1u << L.xcd_shift) - 1u;
    }
    constexpr int BPT = (MAXB + THREADS - 1) / THREADS;
    uint32_t greserve[BPT], cq[BPT], ex0 = 0;
    {
        uint32_t c[BPT];
        uint32_t v = 0;
#pragma unroll
        for (int q = 0; q < BPT; ++q) {
            const uint32_t bq = BPT * tid + q;
            c[q] = bq < nb ? lhist[bq] : 0;
            cq[q] = c[q];
            v += c[q];
        }
        const int lane = tid & 63, wave = tid >> 6;
        uint32_t incl = v;
        incl = wave_scan_incl(incl);
        if (lane == 63) scan_tmp[wave] = incl;
        __syncthreads();
        uint32_t wbase, all;
        wave_totals<THREADS / 64>(scan_tmp, lane, wave, wbase, all);
        staged = all;  // records of this tile that take part
        ex0 = wbase + incl - v;
        uint32_t ex = ex0;
#pragma unroll
        for (int q = 0; q < BPT; ++q) {
            const uint32_t bq = BPT * tid + q;
            if (bq < nb) lstart[bq] = ex;
            // the reservation is issued now and consumed after the LDS reorder: its latency overlaps that phase
            greserve[q] = (bq < nb && c[q]) ? atomicAdd(&cursor[((gbin0 + bq) << L.xcd_shift) + xcc], c[q]) : 0u;
            ex += c[q];
        }
    }
    __syncthreads();
    BBK_PH(prof_kind, 2, t_prev);  // scan (+ reservation issue)

#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        if (binrank[i] != 0xFFFFFFFFu) {
            const uint32_t pos = lstart[binrank[i] >> 16] + (binrank[i] & 0xFFFFu);
            key_store<W>(&stage[pos], keys[i]);
            if (HAS_VAL) vstage[pos] = vals[i];
        }
    }
    // the reservations' results are awaited HERE, by every lane: the compiler otherwise puts the wait for them (vmcnt 0)
    // into the conditional blocks of the store loop below, where it makes every store wait for the one before
#pragma unroll
    for (int q = 0; q < BPT; ++q) asm volatile("" : "+v"(greserve[q]));
    {
        uint32_t ex = ex0;
#pragma unroll
        for (int q = 0; q < BPT; ++q) {
            const uint32_t bq = BPT * tid + q;
            if (bq < nb) {
                goff[bq] = greserve[q] - ex;
                if (L.slot_cap) {
                    // first staged position of this bin that no longer fits its slot (lhist is free by now)
                    const uint64_t slot_end = (gbin0 + bq) * (uint64_t)L.slot_stride +
                                              (L.xcd_shift ? (uint64_t)(xcc + 1u) * L.sub_cap : (uint64_t)L.slot_cap);
                    const int64_t room = (int64_t)slot_end - (int64_t)greserve[q];
                    lhist[bq] = (uint32_t)(int32_t)(room < -(int64_t)0x7FFF0000 ? -(int64_t)0x7FFF0000 : room) + ex;
                }
            }
            ex += cq[q];
        }
    }
    __syncthreads();
    BBK_PH(prof_kind, 3, t_prev);  // reorder into LDS

    // A bin whose slot is full (a k-mer repeated far beyond the coverage, a crowded bucket) spills.  Rare, and handled
    // after the stores: the spill counter's atomic returns a value, and a wait for it between the stores would make
    // every store wait for the one before.
    uint32_t full = 0;
    static_assert(ITEMS <= 32, "one bit per item");
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t pos = (uint32_t)(i * THREADS + tid);
        if (pos < staged) {
            const Key<W> key = key_load<W>(&stage[pos]);
            uint32_t pfx = prefix_of<W>(key, L.dmode, L.w0bits);
            (void)select_prefix(pfx, L);
            const uint32_t b = bin_of(pfx, L, nb);
            const uint32_t g = goff[b] + pos;
            if (L.slot_cap && (int32_t)pos >= (int32_t)lhist[b]) {
                full |= 1u << i;
            } else {
                if constexpr (NOUT) reinterpret_cast<uint32_t *>(out)[g] = (uint32_t)key.w[0];
                else key_store<W>(&out[g], key);
                if (HAS_VAL) vout[g] = vstage[pos];
            }
        }
    }
    if (full) {
#pragma unroll 1
        for (int i = 0; i < ITEMS; ++i) {
            if ((full >> i) & 1u) {
                const uint32_t pos = (uint32_t)(i * THREADS + tid);
                const uint32_t sp = atomicAdd(L.spill_count, 1u);
                if (sp < L.spill_cap) {
                    key_store<W>(&reinterpret_cast<Key<W> *>(L.spill_keys)[sp], key_load<W>(&stage[pos]));
                    if (HAS_VAL) L.spill_vals[sp] = vstage[pos];
                }
            }
        }
    }
    BBK_PH(prof_kind, 4, t_prev);  // store issue
#ifdef BBK_PHASE_PROF
    if (threadIdx.x == 0) atomicAdd(&g_phase[prof_kind][7], 1ull);
#endif
}

// Record of item i of a lane inside its tile.  8-byte keys: the items come in adjacent pairs, so that a full tile is
// read with 16-byte loads (global_load_dwordx4: half the load instructions of the 8-byte striping); the order of
// the records inside a tile is irrelevant (the scatter is unstable, the histogram a sum).
template <int W, int THREADS>
__device__ __forceinline__ uint32_t tile_local(int i, int tid) {
    if (W == 1) return (uint32_t)((((i >> 1) * THREADS + tid) << 1) | (i & 1));
    return (uint32_t)(i * THREADS + tid);
}

typedef uint64_t KeyPair __attribute__((ext_vector_type(2), aligned(8)));  // 16 bytes, 8-byte aligned

// all ITEMS records of a lane; every load is issued before the first use (a load inside a `local < count` branch
// would be waited for before the next one is issued: one memory latency per record)
template <int W, int ITEMS, int THREADS, bool HAS_VAL>
__device__ __forceinline__ void tile_load(const Key<W> *__restrict__ in, const uint32_t *__restrict__ vin, uint64_t begin,
                                          uint32_t count, int tid, Key<W> (&keys)[ITEMS], uint32_t (&vals)[ITEMS],
                                          int expand_k = 0, int expand_tag = 0) {
    if (expand_k) {  // uniform: record r of the tile = canonical key r/2 (even r) or its reverse complement (odd r)
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const uint32_t local = tile_local<W, THREADS>(i, tid);
            const uint64_t rec = begin + (local < count ? local : count - 1u);  // clamped into the tile
            const uint64_t at = rec >> 1;
            Key<W> x = key_load<W>(&in[at]);
            if (rec & 1) x = kmer_rc<W>(x, expand_k);
            if (W == 1 && expand_tag) x.w[0] |= __umul64hi(xxh3_64<W>(x), 16ull) << (2 * expand_k);
            keys[i] = x;
            vals[i] = HAS_VAL ? vin[at] : 0u;
        }
    } else if constexpr (W == 1) {
        if (count == (uint32_t)(ITEMS * THREADS)) {  // full tile (uniform): pairs
            const uint64_t *base = reinterpret_cast<const uint64_t *>(in) + begin;
#pragma unroll
            for (int i = 0; i < ITEMS; i += 2) {
                const uint32_t local = tile_local<W, THREADS>(i, tid);
                const KeyPair p = *reinterpret_cast<const KeyPair *>(base + local);
                keys[i].w[0] = p.x;
                keys[i + 1].w[0] = p.y;
                vals[i] = HAS_VAL ? vin[begin + local] : 0u;
                vals[i + 1] = HAS_VAL ? vin[begin + local + 1] : 0u;
            }
        } else {
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) {
                const uint32_t local = tile_local<W, THREADS>(i, tid);
                const uint64_t at = begin + (local < count ? local : count - 1u);  // clamped into the tile
                keys[i] = key_load<W>(&in[at]);
                vals[i] = HAS_VAL ? vin[at] : 0u;
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const uint32_t local = tile_local<W, THREADS>(i, tid);
            const uint64_t at = begin + (local < count ? local : count - 1u);  // clamped into the tile
            keys[i] = key_load<W>(&in[at]);
            vals[i] = HAS_VAL ? vin[at] : 0u;
        }
    }
}

// One partition level over a key array.  HIST_ONLY: accumulate the level histogram; else scatter.
// LVL1: level-1 kernels have at most 512 bins (smaller LDS tables: two workgroups per CU)
// NOUT: 4-byte output records (the keys' low words; level 2 of narrow stage B, see k_bucket_dist_nb)
template <int W, bool HAS_VAL, bool HIST_ONLY, bool LVL1, bool NOUT = false>
__global__ __launch_bounds__(PartCfg<W>::THREADS) void k_part(const Key<W> *__restrict__ in,
                                                              const uint32_t *__restrict__ vin, TileMap M, PartLevel L,
                                                              uint32_t *__restrict__ ghist,   // HIST_ONLY: [nseg * nb]
                                                              uint32_t *__restrict__ cursor,  // scatter: running offsets
                                                              Key<W> *__restrict__ out, uint32_t *__restrict__ vout) {
    constexpr int kPartItems = PartCfg<W>::ITEMS, kPartTile = PartCfg<W>::TILE, kPartThreads = PartCfg<W>::THREADS;
    constexpr int MAXB = LVL1 ? 512 : kMaxBins;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // layout: lhist[MAXB] | lstart[MAXB] | goff[MAXB] | scan[32] | stage | vstage
    uint32_t *lhist = reinterpret_cast<uint32_t *>(smem);
    uint32_t *lstart = lhist + MAXB;
    uint32_t *goff = lstart + MAXB;
    uint32_t *scan_tmp = goff + MAXB;
    unsigned char *after = reinterpret_cast<unsigned char *>(scan_tmp + 32);
    Key<W> *stage = reinterpret_cast<Key<W> *>(after);
    uint32_t *vstage = reinterpret_cast<uint32_t *>(after + sizeof(Key<W>) * kPartTile);

    const int tid = threadIdx.x;
    if constexpr (HIST_ONLY) {
        // a workgroup walks `group` consecutive tiles and adds its LDS histogram to the global one when the
        // level-1 segment changes and at the end: one global atomic per (workgroup, bin), not per (tile, bin)
        const uint32_t t0 = blockIdx.x * M.group;
        const uint32_t t1 = t0 + M.group < M.ntiles ? t0 + M.group : M.ntiles;
        uint32_t nb = 0;
        uint64_t gbin0 = ~0ull;  // doubles as the identity of the current segment
        for (uint32_t t = t0; t < t1; ++t) {
            const TileInfo T = tile_info(M, L, t, (uint32_t)kPartTile);
            const uint64_t begin = T.begin;
            const uint32_t count = T.count;
            if (T.gbin0 != gbin0) {
                __syncthreads();
                for (uint32_t b = tid; b < nb; b += kPartThreads) {
                    const uint32_t c = lhist[b];
                    if (c) atomicAdd(&ghist[gbin0 + b], c);
                }
                __syncthreads();
                nb = T.nb;
                gbin0 = T.gbin0;
                for (uint32_t b = tid; b < nb; b += kPartThreads) lhist[b] = 0;
                __syncthreads();
            }
            Key<W> keys[kPartItems];
            uint32_t unused[kPartItems];
            tile_load<W, kPartItems, kPartThreads, false>(in, nullptr, begin, count, tid, keys, unused, M.expand_k,
                                                          M.expand_tag);
#pragma unroll
            for (int i = 0; i < kPartItems; ++i) {
                const uint32_t local = tile_local<W, kPartThreads>(i, tid);
                if (local < count) {
                    uint32_t pfx = prefix_of<W>(keys[i], L.dmode, L.w0bits);
                    if (select_prefix(pfx, L)) atomicAdd(&lhist[bin_of(pfx, L, nb)], 1u);
                }
            }
        }
        __syncthreads();
        for (uint32_t b = tid; b < nb; b += kPartThreads) {
            const uint32_t c = lhist[b];
            if (c) atomicAdd(&ghist[gbin0 + b], c);
        }
        return;
    }
#ifdef BBK_PHASE_PROF
    unsigned long long t_prev = clock64();
    const int prof_kind = LVL1 ? 1 : 2;
#else
    const unsigned long long t_prev = 0;
    const int prof_kind = 0;
#endif
    const TileInfo T = tile_info(M, L, blockIdx.x, (uint32_t)kPartTile);
    const uint64_t begin = T.begin, gbin0 = T.gbin0;  // gbin0: flat index of bin 0 in the cursor array
    const uint32_t count = T.count, nb = T.nb;
    if (count == 0) return;  // an unused place of the XCD-wise order of level-2 tiles (k_tile_desc)

    for (uint32_t b = tid; b < nb; b += kPartThreads) lhist[b] = 0;
    __syncthreads();
    BBK_PH(prof_kind, 0, t_prev);  // tile lookup

    Key<W> keys[kPartItems];
    uint32_t vals[kPartItems];
    uint32_t binrank[kPartItems];  // bin << 16 | rank (rank < 8192 fits 13 bits; bins < 1024)
    tile_load<W, kPartItems, kPartThreads, HAS_VAL>(in, vin, begin, count, tid, keys, vals, M.expand_k, M.expand_tag);
    // keep the records in registers: otherwise hipcc re-loads them from (restrict, read-only) memory for the LDS
    // reorder, which doubles the L2 traffic and, vmcnt being in-order, puts the reservation atomics issued in
    // between back on the critical path
#pragma unroll
    for (int i = 0; i < kPartItems; ++i) {
#pragma unroll
        for (int w = 0; w < W; ++w) asm volatile("" : "+v"(keys[i].w[w]));
        if (HAS_VAL) asm volatile("" : "+v"(vals[i]));
    }
#pragma unroll
    for (int i = 0; i < kPartItems; ++i) {
        const uint32_t local = tile_local<W, kPartThreads>(i, tid);
        binrank[i] = 0xFFFFFFFFu;
        if (local < count) {
            uint32_t pfx = prefix_of<W>(keys[i], L.dmode, L.w0bits);
            if (select_prefix(pfx, L)) {
                const uint32_t b = bin_of(pfx, L, nb);
                const uint32_t rank = atomicAdd(&lhist[b], 1u);
                binrank[i] = (b << 16) | rank;
            }
        }
    }
    __syncthreads();
    BBK_PH(prof_kind, 1, t_prev);  // load + LDS ranking
    static_assert(!NOUT || (W == 1 && !HIST_ONLY), "4-byte output records: 8-byte keys, scatter only");
    part_tail<W, kPartItems, kPartThreads, MAXB, HAS_VAL, NOUT>(keys, vals, binrank, lhist, lstart, goff, scan_tmp, stage, vstage,
                                                        nb, gbin0, L, cursor, out, vout, prof_kind, t_prev);
}

static size_t part_smem(int W, int tile, bool has_val, bool hist_only, bool lvl1) {
    size_t s = sizeof(uint32_t) * (3 * (lvl1 ? 512 : kMaxBins) + 32);
    if (!hist_only) s += (size_t)W * 8 * tile + (has_val ? 4 * (size_t)tile : 0);
    return s;
}

// ------------------------------------------------------------------------------------------
// fused k-mer extraction + level-1 partition over packed reads (HASH prefix)
// ------------------------------------------------------------------------------------------
// Instance space = chunks: read r contributes ceil(nk_r / CH) chunks of CH consecutive k-mer positions
// (the last one shorter); a lane owns one chunk, so it never crosses a read: one extraction, then (8-byte
// keys) every further k-mer is ROLLED from its predecessor -- with R = rev2(fwd) kept alongside one step is
// fwd = fwd>>2 | b<<2(k-1), R = R<<2 | b<<2(32-k), the reverse complement is (~R)>>pad and the canonical
// test is R <= (~fwd)<<pad: ~15 integer ops instead of a fresh extraction + bit reversal.
// The tile's reads (cursor tables + packed words, one coalesced copy) are staged in LDS first, so the lanes'
// dependent lookups (read of the chunk -> word offset -> words) cost LDS, not HBM, latency.  A tile whose
// reads do not fit (thousands of reads shorter than k in a row, words not laid out in read order) takes
// the same code over the global arrays.
struct ChunkWords {
    const uint64_t *rw;  // words of the chunk's read (LDS or global)
    uint32_t p;          // first k-mer position of the chunk
    uint32_t cnt;        // k-mers of the chunk (0: idle lane)
    uint32_t len;        // read length
};

// 64 bits of the packed read starting at base p (bases p .. p+31; words past `lastw` are not touched)
__device__ __forceinline__ uint64_t bases_from(const uint64_t *rw, uint32_t p, uint32_t lastw) {
    uint32_t wi = p >> 5;
    wi = wi <= lastw ? wi : lastw;
    const uint32_t sh = (p & 31u) << 1;
    const uint64_t lo = rw[wi];
    const uint64_t hi = rw[wi + 1 <= lastw ? wi + 1 : lastw];
    return (lo >> sh) | ((hi << 1) << (63u - sh));
}

template <int W, int CH, bool HAS_VAL>
__device__ __forceinline__ void chunk_records(const ChunkWords C, uint32_t k_, const PartLevel &L, uint32_t nb,
                                              uint32_t *lhist, Key<W> (&keys)[CH], uint32_t (&vals)[CH],
                                              uint32_t (&binrank)[CH]) {
    const uint64_t *rw = C.rw;
    // 8-byte keys, all state top-aligned so that every per-step shift is by a constant:
    //   Ft = fwd << pad (base 0 at bit pad, base k-1 at bits 62..63), Rv = rev2(fwd) (base 0 at the top)
    //   step: Ft = (Ft >> 2) & himask | b << 62,  Rv = Rv << 2 | b << pad
    //   canonical test (base-lexicographic fwd <= rc, rtseq.hpp:407-415): Rv <= ~Ft & himask
    // 16-byte keys (k = 33..64): the same with 128-bit state {hi, lo} -- Ft = F << pad (pad = 128 - 2k < 64, only
    // the low word has padding), Rv = {rev2(w0), rev2(w1)}; ~50 VALU per step against ~135 for a fresh extraction,
    // reverse complement and base-order comparison.
    const uint32_t pad = W == 1 ? 64u - 2u * k_ : (W == 2 ? 128u - 2u * k_ : 0u);
    const uint64_t himask = ~0ull << pad;
    uint64_t Ft = 0, Rv = 0;      // 8-byte keys; low words of the 128-bit state
    uint64_t FtH = 0, RvH = 0;    // high words (16-byte keys)
    uint32_t inb = 0;    // bases p+k, p+k+1, ...: the ones that enter (and the outgoing-edge bases)
    uint32_t prevb = 0;  // bases p-1, p, ...: the incoming-edge bases
    if (W == 1 && C.cnt) {
        const uint32_t lastw = (C.len - 1u) >> 5;
        const uint64_t f = bases_from(rw, C.p, lastw);
        Ft = f << pad;
        Rv = rev2(Ft >> pad);
        inb = (uint32_t)bases_from(rw, C.p + k_, lastw);
        if (HAS_VAL) prevb = ((uint32_t)f << 2) | (C.p ? base_at(rw, C.p - 1u) : 0u);
    }
    if (W == 2 && C.cnt) {
        const uint32_t lastw = (C.len - 1u) >> 5;
        const uint64_t w0 = bases_from(rw, C.p, lastw);                                   // bases p .. p+31
        const uint64_t w1 = (bases_from(rw, C.p + 32u, lastw) << pad) >> pad;              // bases p+32 .. p+k-1
        // F << pad as {hi, lo}
        FtH = pad ? (w1 << pad) | (w0 >> (64u - pad)) : w1;
        Ft = w0 << pad;
        RvH = rev2(w0);
        Rv = rev2(w1);
        inb = (uint32_t)bases_from(rw, C.p + k_, lastw);
        if (HAS_VAL) prevb = ((uint32_t)w0 << 2) | (C.p ? base_at(rw, C.p - 1u) : 0u);
    }
#pragma unroll
    for (int i = 0; i < CH; ++i) {
#pragma unroll
        for (int w = 0; w < W; ++w) keys[i].w[w] = 0;
        vals[i] = 0;
        binrank[i] = 0xFFFFFFFFu;
        if ((uint32_t)i < C.cnt) {
            const uint32_t p = C.p + (uint32_t)i;
            bool minimal;
            uint32_t nextc, prevc;  // HAS_VAL: bases p+k and p-1
            if constexpr (W == 1) {
                if (i > 0) {
                    const uint64_t b = (inb >> (2 * (i - 1))) & 3u;
                    Ft = ((Ft >> 2) & himask) | (b << 62);
                    Rv = (Rv << 2) | (b << pad);
                }
                minimal = Rv <= (~Ft & himask);
                keys[i].w[0] = (minimal ? Ft : ~Rv) >> pad;
                nextc = (inb >> (2 * i)) & 3u;
                prevc = (prevb >> (2 * i)) & 3u;
            } else if constexpr (W == 2) {
                if (i > 0) {
                    const uint64_t b = (inb >> (2 * (i - 1))) & 3u;
                    Ft = ((Ft >> 2) | (FtH << 62)) & himask;
                    FtH = (FtH >> 2) | (b << 62);
                    RvH = (RvH << 2) | (Rv >> 62);
                    Rv = (Rv << 2) | (b << pad);
                }
                // canonical test: Rv <= ~Ft & himask128 as 128-bit numbers
                const uint64_t cH = ~FtH, cL = ~Ft & himask;
                minimal = RvH < cH || (RvH == cH && Rv <= cL);
                const uint64_t xH = minimal ? FtH : ~RvH, xL = minimal ? Ft : ~Rv;
                keys[i].w[0] = pad ? (xL >> pad) | (xH << (64u - pad)) : xL;
                keys[i].w[1] = xH >> pad;
                nextc = (inb >> (2 * i)) & 3u;
                prevc = (prevb >> (2 * i)) & 3u;
            } else {
                const Key<W> f = kmer_extract<W>(rw, p, (int)k_);
                const Key<W> rc = kmer_rc<W>(f, (int)k_);
                minimal = !kmer_less_nucl<W>(rc, f);
                keys[i] = key_select<W>(minimal, f, rc);
                if (HAS_VAL) {
                    nextc = p + k_ < C.len ? base_at(rw, p + k_) : 0u;
                    prevc = p >= 1 ? base_at(rw, p - 1) : 0u;
                }
            }
            if (HAS_VAL) {
                uint32_t m = 0;
                if (p + k_ < C.len) m |= 1u << (minimal ? nextc : 7u - nextc);
                if (p >= 1) m |= 1u << (minimal ? 4u + prevc : 3u - prevc);
                vals[i] = m;
            }
            uint32_t pfx = part_hash32<W>(keys[i]);
            if (select_prefix(pfx, L)) {
                const uint32_t b = L.b1 == 0 ? 0u : (pfx >> (32 - L.b1));
                const uint32_t rank = atomicAdd(&lhist[b], 1u);
                binrank[i] = (b << 16) | rank;
            }
        }
    }
}

template <int W, bool HAS_VAL, bool HIST_ONLY>
__global__ __launch_bounds__(HIST_ONLY ? kRdHistThreads : kRdThreads) void k_part_reads(ReadSrc S, PartLevel L, uint32_t *__restrict__ ghist,
                                                           uint32_t *__restrict__ cursor, Key<W> *__restrict__ out,
                                                           uint32_t *__restrict__ vout) {
    constexpr int NT = HIST_ONLY ? kRdHistThreads : kRdThreads;  // chunks per tile = threads
    constexpr int CH = RdCfg<W>::CH, TILE = RdCfg<W>::TILE, MAXB = 512;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // layout: lhist | lstart | goff | scan[32] | U, where U is the read tables while extracting
    // (rel[kRdSlots+2] | wrel[kRdSlots+2] | nk[kRdSlots+2] | words[kRdWords+W+2]) and the stage afterwards
    uint32_t *lhist = reinterpret_cast<uint32_t *>(smem);
    uint32_t *lstart = lhist + MAXB;
    uint32_t *goff = lstart + MAXB;
    uint32_t *scan_tmp = goff + MAXB;
    unsigned char *U = reinterpret_cast<unsigned char *>(scan_tmp + 32);
    int32_t *s_rel = reinterpret_cast<int32_t *>(U);  // first chunk of read r0+i, relative to the tile's first chunk
    int32_t *s_wrel = s_rel + (kRdSlots + 2);         // first word of read r0+i, relative to the staged window
    uint32_t *s_len = reinterpret_cast<uint32_t *>(s_wrel + (kRdSlots + 2));
    uint64_t *s_words = reinterpret_cast<uint64_t *>(s_len + (kRdSlots + 2));
    Key<W> *stage = reinterpret_cast<Key<W> *>(U);
    uint32_t *vstage = reinterpret_cast<uint32_t *>(U + sizeof(Key<W>) * TILE);

    const uint32_t tid = threadIdx.x;
    const uint32_t k_ = (uint32_t)S.k;
    const uint32_t nb = L.nb1;
    const uint32_t ntiles = (uint32_t)((S.n_chunks + NT - 1) / NT);
    for (uint32_t b = tid; b < nb; b += NT) lhist[b] = 0;
#ifdef BBK_PHASE_PROF
    unsigned long long t_prev = clock64();
#else
    const unsigned long long t_prev = 0;
#endif

    // scatter: one tile per workgroup (grid == tiles).  Histogram: a workgroup walks many tiles and adds
    // its LDS histogram to the global one once (512 atomics per workgroup instead of per tile).
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t c0 = (uint64_t)tile * NT;  // first chunk of the tile
    const uint64_t left = S.n_chunks - c0;
    const uint32_t nch = left < (uint64_t)NT ? (uint32_t)left : (uint32_t)NT;
    const RdTile T = S.tiles[tile];
    const uint32_t r0 = T.r0, nr = T.nr;  // reads r0 .. r0+nr-1
    const uint64_t wbase = T.wbase;
    bool fast = T.wspan != 0xFFFFFFFFu;
    const uint32_t wspan = fast ? T.wspan : 0u;
    const uint64_t wend = wbase + wspan;
    if (fast) {
        bool bad = false;
        for (uint32_t i = tid; i <= nr; i += NT) {
            const uint64_t rr = (uint64_t)r0 + i;  // <= n_reads (coff holds n_reads + 1 entries)
            s_rel[i] = (int32_t)(int64_t)(S.coff[rr] - c0);
            if (i < nr) {
                const uint64_t wo = S.woff[rr];
                const uint32_t ln = S.len[rr];
                s_wrel[i] = (int32_t)(int64_t)(wo - wbase);
                s_len[i] = ln;
                // words must be laid out in read order: every read starts inside the window and all but
                // the last end inside it
                if (i > 0 && wo < wbase) bad = true;
                if (i + 1 < nr && wo + ((ln + 31u) >> 5) > wend) bad = true;
            }
        }
        for (uint32_t i = tid; i < wspan; i += NT) s_words[i] = S.words[wbase + i];
        fast = !__syncthreads_or(bad);
    } else {
        __syncthreads();
    }
    if (!HIST_ONLY) BBK_PH(0, 0, t_prev);  // read tables + words into LDS

    Key<W> keys[CH];
    uint32_t vals[CH];
    uint32_t binrank[CH];  // bin << 16 | rank (rank < 8192 fits 13 bits; bins < 512)
    if (fast) {
        ChunkWords C{s_words, 0, 0, 0};
        if (tid < nch) {
            const uint32_t ri = read_of(s_rel, nr, (int32_t)tid);
            C.p = (uint32_t)((int32_t)tid - s_rel[ri]) * CH;
            C.len = s_len[ri];
            const uint32_t nk = C.len - k_ + 1u;  // the read owns a chunk, so len >= k
            C.cnt = nk - C.p < (uint32_t)CH ? nk - C.p : (uint32_t)CH;
            C.rw = s_words + s_wrel[ri];
        }
        chunk_records<W, CH, HAS_VAL>(C, k_, L, nb, lhist, keys, vals, binrank);
    } else {
        ChunkWords C{S.words, 0, 0, 0};
        if (tid < nch) {
            const uint64_t c = c0 + tid;
            uint64_t lo = r0, hi = (uint64_t)r0 + nr;  // largest r with coff[r] <= c
            while (hi - lo > 1) {
                const uint64_t mid = (lo + hi) >> 1;
                if (S.coff[mid] <= c) lo = mid;
                else hi = mid;
            }
            C.p = (uint32_t)(c - S.coff[lo]) * CH;
            C.len = S.len[lo];
            const uint32_t nk = C.len - k_ + 1u;
            C.cnt = nk - C.p < (uint32_t)CH ? nk - C.p : (uint32_t)CH;
            C.rw = S.words + S.woff[lo];
        }
        chunk_records<W, CH, HAS_VAL>(C, k_, L, nb, lhist, keys, vals, binrank);
    }
    __syncthreads();  // histogram complete / the read tables may be overwritten

    if constexpr (!HIST_ONLY) {
        BBK_PH(0, 1, t_prev);  // extraction + LDS ranking
        part_tail<W, CH, NT, MAXB, HAS_VAL>(keys, vals, binrank, lhist, lstart, goff, scan_tmp, stage, vstage, nb,
                                                    0ull, L, cursor, out, vout, 0, t_prev);
        return;
    }
    }
    if (HIST_ONLY) {
        for (uint32_t b = tid; b < nb; b += NT) {
            const uint32_t c = lhist[b];
            if (c) atomicAdd(&ghist[b], c);
        }
    }
}

static size_t part_reads_smem(int W, bool has_val, bool hist_only) {
    const size_t tables = sizeof(uint32_t) * 3 * (kRdSlots + 2) + sizeof(uint64_t) * (kRdWords + W + 2);
    const size_t tile = (size_t)kRdThreads * (W == 1 ? 8 : (W == 2 ? 4 : 2));
    const size_t stage = hist_only ? 0 : (size_t)W * 8 * tile + (has_val ? 4 * tile : 0);
    return sizeof(uint32_t) * (3 * 512 + 32) + std::max(tables, stage);
}

// ------------------------------------------------------------------------------------------
// bucket kernel
// ------------------------------------------------------------------------------------------
__device__ inline uint64_t match8(uint32_t d, bool valid) {
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const uint64_t m = __ballot(bit);
        peers &= bit ? m : ~m;
    }
    return peers;
}

struct BucketArgs {
    const uint32_t *boff;        // nbuckets + 1 record offsets
    uint32_t *dcount;            // distinct per bucket; 0xFFFFFFFF = overflow (left untouched)
    const uint32_t *bucket_ids;  // null: bucket = blockIdx.x; else the list of buckets to process
    int k;
    uint32_t *dbg;               // optional counters (BBK_VERBOSE): [0] buckets that took the all-words fallback
    // slot mode: bucket b lies at [b*slot_cap, b*slot_cap + min(reserved, slot_cap)), reserved = cursor[b] - b*slot_cap;
    // a bucket that reserved more than its slot is left alone (dcount = 0xFFFFFFFF): the host reprocesses it together
    // with the spill list
    uint32_t slot_cap, slot_stride;
    const uint32_t *cursor;
    // (the hash-dedup kernels write the distinct records back to the head of their bucket; until round 3 they could also
    // reserve a place in the dense result with an atomicAdd on one counter -- 2.6 ms for the 227 210 buckets of BASELINE
    // configs[1], tools/probes/single_counter_probe.hip)
    // sorting kernels, input known to hold (almost certainly) no duplicates: bucket b's records go straight to
    // sorted_keys[boff[b] ...] (the dense result: same offsets as the input when nothing is removed), word 0 masked
    // with strip_mask; a bucket that did remove a duplicate raises *dup_flag and the caller redoes the pass in place
    void *sorted_keys;
    uint32_t *sorted_vals;
    uint32_t *dup_flag;
    uint64_t strip_mask;
    // hash-dedup kernels: a probe sequence longer than this means the table is (nearly) full and the bucket is left to
    // the caller (kHashMaxProbes; tests lower it through BBK_HASH_MAX_PROBES to force that path on half-empty slots)
    uint32_t max_probes;
    // sorting kernels reading slots (stage B without histograms): bucket b's sorted records go to sorted_keys[out_off[b]
    // ...] (exclusive scan of the slot fills); null: the dense layout, output offset = input offset
    const uint32_t *out_off;
};

// first record and record count of bucket b (count 0xFFFFFFFF: the slot overflowed)
__device__ inline void bucket_range(const BucketArgs &A, uint32_t b, uint32_t *start, uint32_t *n) {
    if (A.slot_cap) {
        *start = b * A.slot_stride;
        const uint32_t reserved = A.cursor[b] - *start;
        *n = reserved > A.slot_cap ? 0xFFFFFFFFu : reserved;
    } else {
        *start = A.boff[b];
        *n = A.boff[b + 1] - *start;
    }
}

// OP: 0 unique only, 1 COUNT (run length), 2 SUM of vals, 3 OR of vals.  NT threads, CAP = NT * ITEMS.
// Heads + segmented reduce of a bucket that lies sorted in LDS (skeys[0, n), svals alongside when the records
// carry a payload); the distinct records are written back in place at buf[start ...], their reduced payloads
// to vals, the count to dcount[b].  Blocked ownership: thread t owns [t*ITEMS, (t+1)*ITEMS).
template <int W, int NT, int ITEMS, int OP>
__device__ __forceinline__ void bucket_reduce(Key<W> *skeys, uint32_t *svals, uint32_t *scan_tmp, uint32_t n, uint32_t start,
                                              uint32_t b, Key<W> *__restrict__ buf, uint32_t *__restrict__ vals,
                                              const BucketArgs &A) {
    constexpr int NWAVES = NT / 64;
    constexpr bool IN_VAL = OP >= 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t ostart = (A.sorted_keys && A.out_off) ? A.out_off[b] : start;  // where the sorted records go
    Key<W> mine[ITEMS];
    uint32_t mv[ITEMS];
    const uint32_t p0 = (uint32_t)tid * ITEMS;
    Key<W> prev;
#pragma unroll
    for (int j = 0; j < W; ++j) prev.w[j] = ~0ull;  // cannot equal a real key: unused high bits are 0
    if (p0 > 0 && p0 - 1 < n) prev = key_load<W>(&skeys[p0 - 1]);
    uint32_t nheads = 0;
    uint32_t headbits = 0;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
#pragma unroll
        for (int j = 0; j < W; ++j) mine[i].w[j] = 0;
        mv[i] = 0;
        if (p0 + i < n) {
            mine[i] = key_load<W>(&skeys[p0 + i]);
            if (IN_VAL) mv[i] = svals[p0 + i];
            const bool h = (i == 0) ? !key_eq<W>(mine[0], prev) : !key_eq<W>(mine[i], mine[i - 1]);
            if (h) {
                headbits |= 1u << i;
                ++nheads;
            }
        }
    }
    uint32_t excl, total;
    {
        uint32_t incl = nheads;
        incl = wave_scan_incl(incl);
        __syncthreads();  // everyone has its keys in registers: skeys may be reused below
        if (lane == 63) scan_tmp[wave] = incl;
        __syncthreads();
        uint32_t wbase, tot;
        wave_totals<NWAVES>(scan_tmp, lane, wave, wbase, tot);
        excl = wbase + incl - nheads;
        total = tot;
        // the loaded offset is awaited HERE by every lane: left to the compiler, the wait (vmcnt 0) lands in the
        // conditional blocks of the store loop below and makes every store wait for the one before
        asm volatile("" : "+v"(ostart));
    }
#ifndef BBK_AB_BLOCKED_REDUCE  // (A/B: -DBBK_AB_BLOCKED_REDUCE stores straight from the blocked ownership, as before round 3)
    if constexpr (OP == 0) {
        // No payload: the distinct keys go back into LDS at their place in the result (a place at or before the thread's
        // own records, all of which are in registers by now) and leave it with coalesced stores -- 512 contiguous bytes
        // per wave instruction.  Straight from the blocked ownership every lane stored its ITEMS keys 8 ITEMS bytes from
        // its neighbour's: 64 separate pieces per instruction.
        int seg = (int)excl - 1;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            if (p0 + i < n && (headbits & (1u << i))) {
                ++seg;
                Key<W> kx = mine[i];
                if (A.sorted_keys) kx.w[0] &= A.strip_mask;
                key_store<W>(&skeys[seg], kx);
            }
        }
        __syncthreads();
        Key<W> *dstk = A.sorted_keys ? reinterpret_cast<Key<W> *>(A.sorted_keys) + ostart : buf + start;
        for (uint32_t s = tid; s < total; s += NT) key_store<W>(&dstk[s], key_load<W>(&skeys[s]));
        if (tid == 0 && A.sorted_keys && total != n) atomicOr(A.dup_flag, 1u);
        if (tid == 0) A.dcount[b] = total;
        return;
    }
#endif
    uint32_t *acc = reinterpret_cast<uint32_t *>(skeys);  // CAP u32 fit in the key buffer
    if (OP != 0) {
        for (uint32_t s = tid; s < total; s += NT) acc[s] = 0;
        __syncthreads();
    }
    {
        int seg = (int)excl - 1;  // segment of the records before my first head
        uint32_t a = 0;
        bool any = false;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            if (p0 + i < n) {
                if (headbits & (1u << i)) {
                    if (OP != 0 && any) {
                        if (OP == 3) atomicOr(&acc[seg], a);
                        else atomicAdd(&acc[seg], a);
                    }
                    ++seg;
                    a = 0;
                    if (A.sorted_keys) {
                        Key<W> kx = mine[i];
                        kx.w[0] &= A.strip_mask;
                        key_store<W>(&reinterpret_cast<Key<W> *>(A.sorted_keys)[ostart + (uint32_t)seg], kx);
                    } else {
                        key_store<W>(&buf[start + (uint32_t)seg], mine[i]);  // distinct keys, in place
                    }
                }
                any = true;
                if (OP == 1) a += 1;
                else if (OP == 2) a += mv[i];
                else if (OP == 3) a |= mv[i];
            }
        }
        if (OP != 0 && any) {
            if (OP == 3) atomicOr(&acc[seg], a);
            else atomicAdd(&acc[seg], a);
        }
    }
    if (OP != 0) {
        __syncthreads();
        uint32_t *vdst = A.sorted_keys ? A.sorted_vals : vals;
        const uint32_t vstart = A.sorted_keys ? ostart : start;
        for (uint32_t s = tid; s < total; s += NT) vdst[vstart + s] = acc[s];
    }
    if (tid == 0 && A.sorted_keys && total != n) atomicOr(A.dup_flag, 1u);
    if (tid == 0) A.dcount[b] = total;
}

template <int W, int NT, int ITEMS, int OP>
__global__ __launch_bounds__(NT) void k_bucket(Key<W> *__restrict__ buf, uint32_t *__restrict__ vals, BucketArgs A) {
    constexpr int CAP = NT * ITEMS;
    constexpr int NWAVES = NT / 64;
    constexpr bool IN_VAL = OP >= 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // layout: wave_cnt[NWAVES][256] | dstart[256] | scan[32] | skeys[CAP] | svals[CAP] (IN_VAL)
    uint32_t(*wave_cnt)[256] = reinterpret_cast<uint32_t(*)[256]>(smem);
    uint32_t *dstart = reinterpret_cast<uint32_t *>(smem) + NWAVES * 256;
    uint32_t *scan_tmp = dstart + 256;
    Key<W> *skeys = reinterpret_cast<Key<W> *>(scan_tmp + 32);
    uint32_t *svals = reinterpret_cast<uint32_t *>(reinterpret_cast<unsigned char *>(skeys) + sizeof(Key<W>) * CAP);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t b = A.bucket_ids ? A.bucket_ids[blockIdx.x] : blockIdx.x;
    uint32_t start, n;
    bucket_range(A, b, &start, &n);
    if (n == 0) {
        if (tid == 0) A.dcount[b] = 0;
        return;
    }
    if (n > (uint32_t)CAP) {
        if (tid == 0) A.dcount[b] = 0xFFFFFFFFu;
        return;
    }
    {
        // all loads first (unconditional, index clamped into the bucket), then the LDS stores: a load inside the
        // `p < n` branch is waited for before the next one is issued -- one memory latency per record
        Key<W> rk[ITEMS];
        uint32_t rv[ITEMS];
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const uint32_t p = (uint32_t)(i * NT + tid);
            const uint32_t at = start + (p < n ? p : n - 1u);
            rk[i] = key_load<W>(&buf[at]);
            rv[i] = IN_VAL ? vals[at] : 0u;
        }
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const uint32_t p = (uint32_t)(i * NT + tid);
            if (p < n) {
                key_store<W>(&skeys[p], rk[i]);
                if (IN_VAL) svals[p] = rv[i];
            }
        }
    }
    __syncthreads();

    // ---- LSD radix sort inside LDS.  Only word 0 is radix-sorted, and only over the bits in which the
    // bucket's keys differ (keys of a KEYS-mode bucket share their top ~16 bits): subtract the bucket
    // minimum, sort the bits of (max - min).  Wider keys then order the (short) runs of equal word 0 by
    // their remaining words with an insertion sort; a bucket with a long run (> 48 keys sharing 32
    // bases) falls back to radix passes over every word.
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    const int lastbits = 2 * A.k - 64 * (W - 1);
    uint64_t kmin = 0;
    int sortbits = (W == 1) ? lastbits : 64;
    {
        uint64_t mn = ~0ull, mx = 0;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const uint32_t p = (uint32_t)(i * NT + tid);
            if (p < n) {
                const uint64_t x = skeys[p].w[0];
                mn = x < mn ? x : mn;
                mx = x > mx ? x : mx;
            }
        }
#pragma unroll
        for (int dd = 32; dd >= 1; dd >>= 1) {
            const uint64_t a = __shfl_xor(mn, dd, 64), c = __shfl_xor(mx, dd, 64);
            mn = a < mn ? a : mn;
            mx = c > mx ? c : mx;
        }
        uint64_t *mm = reinterpret_cast<uint64_t *>(wave_cnt);  // counters are not live yet
        if (lane == 0) {
            mm[2 * wave] = mn;
            mm[2 * wave + 1] = mx;
        }
        __syncthreads();
        mn = ~0ull;
        mx = 0;
        for (int j = 0; j < NWAVES; ++j) {
            mn = mm[2 * j] < mn ? mm[2 * j] : mn;
            mx = mm[2 * j + 1] > mx ? mm[2 * j + 1] : mx;
        }
        __syncthreads();
        kmin = mn;
        sortbits = 64 - __builtin_clzll((mx - mn) | 1ull);
    }
    // stable radix passes over bits [0, nbits) of (word `wsel` - base)
    auto radix_passes = [&](int wsel, uint64_t base, int nbits) {
        for (int shift = 0; shift < nbits; shift += 8) {
            Key<W> keys[ITEMS];
            uint32_t v[ITEMS];
            uint32_t dr[ITEMS];  // digit << 16 | rank-in-wave
            if (tid < 256) {
#pragma unroll
                for (int j = 0; j < NWAVES; ++j) wave_cnt[j][tid] = 0;
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) {
                const uint32_t p = (uint32_t)(wave * (ITEMS * 64) + i * 64 + lane);
                const bool valid = p < n;
                uint32_t d = 0;
#pragma unroll
                for (int j = 0; j < W; ++j) keys[i].w[j] = 0;
                v[i] = 0;
                if (valid) {
                    keys[i] = key_load<W>(&skeys[p]);
                    if (IN_VAL) v[i] = svals[p];
                    const uint64_t word = (W == 1) ? keys[i].w[0]
                                                   : reinterpret_cast<const uint64_t *>(&skeys[p])[wsel];
                    d = (uint32_t)((word - base) >> shift) & 0xFFu;
                }
                const uint64_t peers = match8(d, valid);
                const uint32_t pre = wave_cnt[wave][d];
                dr[i] = (d << 16) | (pre + (uint32_t)__popcll(peers & lt_mask));
                if (valid && (peers >> lane) == 1ull) wave_cnt[wave][d] = pre + (uint32_t)__popcll(peers);
            }
            __syncthreads();
            {
                uint32_t tot = 0, incl = 0;
                if (tid < 256) {
#pragma unroll
                    for (int j = 0; j < NWAVES; ++j) {
                        const uint32_t c = wave_cnt[j][tid];
                        wave_cnt[j][tid] = tot;
                        tot += c;
                    }
                    incl = tot;
                    incl = wave_scan_incl(incl);
                    if (lane == 63) scan_tmp[wave] = incl;
                }
                __syncthreads();
                if (tid < 256) {
                    uint32_t wbase = 0;
                    for (int j = 0; j < wave; ++j) wbase += scan_tmp[j];
                    dstart[tid] = wbase + incl - tot;
                }
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) {
                const uint32_t p = (uint32_t)(wave * (ITEMS * 64) + i * 64 + lane);
                if (p < n) {
                    const uint32_t d = dr[i] >> 16;
                    const uint32_t pos = dstart[d] + wave_cnt[wave][d] + (dr[i] & 0xFFFFu);
                    key_store<W>(&skeys[pos], keys[i]);
                    if (IN_VAL) svals[pos] = v[i];
                }
            }
            __syncthreads();
        }
    };
    radix_passes(0, kmin, sortbits);
    if (W >= 2) {
        // runs of equal word 0: the thread that owns a run's first record orders the run by words 1..W-1
        bool bad = false;
        const uint32_t q0 = (uint32_t)tid * ITEMS;
        for (uint32_t p = q0; p < q0 + ITEMS && p < n; ++p) {
            const uint64_t w0 = skeys[p].w[0];
            if (p > 0 && skeys[p - 1].w[0] == w0) continue;  // not a run start
            uint32_t e = p + 1;
            while (e < n && skeys[e].w[0] == w0) ++e;
            if (e - p <= 1) continue;
            if (e - p > 48) {
                bad = true;
                continue;
            }
            for (uint32_t x = p + 1; x < e; ++x) {
                const Key<W> kx = key_load<W>(&skeys[x]);
                const uint32_t vx = IN_VAL ? svals[x] : 0u;
                uint32_t y = x;
                while (y > p) {
                    const Key<W> ky = key_load<W>(&skeys[y - 1]);
                    if (!key_less_words<W>(kx, ky)) break;
                    key_store<W>(&skeys[y], ky);
                    if (IN_VAL) svals[y] = svals[y - 1];
                    --y;
                }
                key_store<W>(&skeys[y], kx);
                if (IN_VAL) svals[y] = vx;
            }
        }
        if (__syncthreads_or(bad)) {
            if (A.dbg && tid == 0) atomicAdd(&A.dbg[0], 1u);
            for (int w = W - 1; w >= 0; --w) radix_passes(w, 0ull, (w == W - 1) ? lastbits : 64);
        }
    }

    bucket_reduce<W, NT, ITEMS, OP>(skeys, svals, scan_tmp, n, start, b, buf, vals, A);
}

// ---- first-choice bucket kernel: ONE distribution pass instead of ballot-ranked radix passes.
// The records of a bucket are spread evenly over its key range (KEYS/REF mode: a contiguous range of k-mers
// of a genome), so DistBins::N bins over the top bits of (word 0 - bucket minimum) hold about one record
// each: count with LDS atomics, scan, scatter with returning atomics (the order inside a bin is arbitrary),
// then the owner of a bin puts it in order by insertion on the whole key.  A bin above kDistMaxBin (skewed
// keys, a k-mer repeated hundreds of times in an unreduced stream) marks the bucket as overflowing and the
// host hands it to k_bucket, which takes any distribution.
// 4096 bins; wide keys WITH a payload: 2048, so that keys + payloads + bins stay below 80 KB and TWO workgroups fit a CU
// (16-byte keys: 57 + 14 + 8 KB).  With 4096 bins the sort of an extension index of 16-byte keys (k-mer + edge mask) ran
// one workgroup per CU: 8.1 ms against 5.0 ms for 257 M records.  (8-byte keys with a payload stay at 4096 bins and
// one workgroup per CU: with 5632 records per bucket the fuller bins cost more than the second workgroup gains.)
template <int W, int OP>
struct DistBins {
    static constexpr int N = (W >= 2 && OP >= 2) ? 2048 : 4096;
    static constexpr int LOG = (W >= 2 && OP >= 2) ? 11 : 12;
};
constexpr uint32_t kDistMaxBin = 96;  // equal keys insert in linear time; only distinct keys cost n^2

template <int W, int NT, int ITEMS, int OP>
__global__ __launch_bounds__(NT) void k_bucket_dist(Key<W> *__restrict__ buf, uint32_t *__restrict__ vals, BucketArgs A) {
    constexpr int CAP = NT * ITEMS;
    constexpr int NWAVES = NT / 64;
    constexpr int DB = DistBins<W, OP>::N;
    constexpr int BPT = DB / NT;
    constexpr bool IN_VAL = OP >= 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // layout: bins[DB] | scan[32] | mm[2 * NWAVES] (u64) | skeys[CAP] | svals[CAP] (IN_VAL)
    uint32_t *bins = reinterpret_cast<uint32_t *>(smem);
    uint32_t *scan_tmp = bins + DB;
    uint64_t *mm = reinterpret_cast<uint64_t *>(scan_tmp + 32);
    Key<W> *skeys = reinterpret_cast<Key<W> *>(mm + 2 * NWAVES);
    uint32_t *svals = reinterpret_cast<uint32_t *>(reinterpret_cast<unsigned char *>(skeys) + sizeof(Key<W>) * CAP);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t b = A.bucket_ids ? A.bucket_ids[blockIdx.x] : blockIdx.x;
    uint32_t start, n;
    bucket_range(A, b, &start, &n);
    if (n == 0) {
        if (tid == 0) A.dcount[b] = 0;
        return;
    }
    if (n > (uint32_t)CAP) {
        if (tid == 0) A.dcount[b] = 0xFFFFFFFFu;
        return;
    }
    for (uint32_t q = tid; q < (uint32_t)DB; q += NT) bins[q] = 0;
#ifdef BBK_PHASE_PROF
    unsigned long long t_prev = clock64();
#endif

    // records of this thread (striped over the bucket); all loads issued before the first use
    Key<W> keys[ITEMS];
    uint32_t v[IN_VAL ? ITEMS : 1];
    uint64_t mn = ~0ull, mx = 0;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t p = (uint32_t)(i * NT + tid);
        const uint32_t at = start + (p < n ? p : n - 1u);
        keys[i] = key_load<W>(&buf[at]);
        if (IN_VAL) v[i] = vals[at];
    }
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {  // clamped duplicates do not change min / max
        const uint64_t x = keys[i].w[0];
        mn = x < mn ? x : mn;
        mx = x > mx ? x : mx;
    }
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) {
        const uint64_t a = __shfl_xor(mn, dd, 64), c = __shfl_xor(mx, dd, 64);
        mn = a < mn ? a : mn;
        mx = c > mx ? c : mx;
    }
    if (lane == 0) {
        mm[2 * wave] = mn;
        mm[2 * wave + 1] = mx;
    }
    __syncthreads();  // bins zeroed, min / max of every wave visible
    mn = ~0ull;
    mx = 0;
#pragma unroll
    for (int j = 0; j < NWAVES; ++j) {
        mn = mm[2 * j] < mn ? mm[2 * j] : mn;
        mx = mm[2 * j + 1] > mx ? mm[2 * j + 1] : mx;
    }
    BBK_PH(3, 0, t_prev);  // loads + min/max
    const uint64_t kmin = mn;
    const int rbits = 64 - __builtin_clzll((mx - mn) | 1ull);
    const int sh = rbits > DistBins<W, OP>::LOG ? rbits - DistBins<W, OP>::LOG : 0;  // digit = (word 0 - min) >> sh < bins

#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t p = (uint32_t)(i * NT + tid);
        if (p < n) atomicAdd(&bins[(uint32_t)((keys[i].w[0] - kmin) >> sh)], 1u);
    }
    __syncthreads();
    BBK_PH(3, 1, t_prev);  // count
    // exclusive scan of the bins; thread t owns bins [t*BPT, (t+1)*BPT)
    uint32_t c[BPT];
    uint32_t sum = 0;
    bool big = false;
#pragma unroll
    for (int q = 0; q < BPT; ++q) {
        c[q] = bins[tid * BPT + q];
        sum += c[q];
        big = big || c[q] > kDistMaxBin;
    }
    uint32_t incl = sum;
    incl = wave_scan_incl(incl);
    if (lane == 63) scan_tmp[wave] = incl;
    if (__syncthreads_or(big)) {  // nothing has been written: the second-chance kernel takes the bucket
        if (tid == 0) A.dcount[b] = 0xFFFFFFFFu;
        return;
    }
    uint32_t first = incl - sum;
    for (int j = 0; j < wave; ++j) first += scan_tmp[j];
    {
        uint32_t ex = first;
#pragma unroll
        for (int q = 0; q < BPT; ++q) {
            bins[tid * BPT + q] = ex;
            ex += c[q];
        }
    }
    __syncthreads();
    BBK_PH(3, 2, t_prev);  // scan
    uint32_t pos_of[ITEMS];  // where the scatter put the record (breaks ties between equal keys)
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t p = (uint32_t)(i * NT + tid);
        pos_of[i] = 0;
        if (p < n) {
            const uint32_t pos = atomicAdd(&bins[(uint32_t)((keys[i].w[0] - kmin) >> sh)], 1u);
            key_store<W>(&skeys[pos], keys[i]);
            pos_of[i] = pos;
        }
    }
    __syncthreads();
    BBK_PH(3, 3, t_prev);  // scatter
    // order inside the bins, record-parallel: a record's final place is its bin's start plus the number of
    // records of the bin that go before it (smaller key; equal key: scattered to a lower position).  After the
    // scatter bins[d] is the END of bin d, so bin d = [bins[d-1], bins[d]).
    // Batched so that the LDS reads of several records are in flight together (one record at a time is three
    // dependent LDS round trips: bin bounds, candidates, compare): RB records per round, the first four candidates
    // of every bin read unconditionally; the rare fuller bins finish in a loop.
    uint32_t dest[ITEMS];
    if constexpr (W == 1) {
        constexpr int RB = 6;
    #pragma unroll
        for (int i0 = 0; i0 < ITEMS; i0 += RB) {
            uint32_t sb[RB], e[RB];
    #pragma unroll
            for (int u = 0; u < RB; ++u) {
                const int i = i0 + u;
                sb[u] = e[u] = 0;
                if (i < ITEMS) {
                    const uint32_t p = (uint32_t)(i * NT + tid);
                    if (p < n) {
                        const uint32_t d = (uint32_t)((keys[i].w[0] - kmin) >> sh);
                        sb[u] = d ? bins[d - 1] : 0u;
                        e[u] = bins[d];
                    }
                }
            }
            Key<W> o[RB][4];
    #pragma unroll
            for (int u = 0; u < RB; ++u) {
    #pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const uint32_t y = sb[u] + c;
                    o[u][c] = key_load<W>(&skeys[y < e[u] ? y : (e[u] ? e[u] - 1u : 0u)]);
                }
            }
    #pragma unroll
            for (int u = 0; u < RB; ++u) {
                const int i = i0 + u;
                if (i < ITEMS) {
                    dest[i] = 0xFFFFFFFFu;
                    const uint32_t p = (uint32_t)(i * NT + tid);
                    if (p < n) {
                        uint32_t before = 0;
    #pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const uint32_t y = sb[u] + c;
                            if (y < e[u]) {
                                const bool lt = key_less_words<W>(o[u][c], keys[i]);
                                const bool eq = key_eq<W>(o[u][c], keys[i]);
                                before += (lt || (eq && y < pos_of[i])) ? 1u : 0u;
                            }
                        }
                        for (uint32_t y = sb[u] + 4; y < e[u]; ++y) {  // bins above four records
                            const Key<W> ok = key_load<W>(&skeys[y]);
                            const bool lt = key_less_words<W>(ok, keys[i]);
                            const bool eq = key_eq<W>(ok, keys[i]);
                            before += (lt || (eq && y < pos_of[i])) ? 1u : 0u;
                        }
                        dest[i] = sb[u] + before;
                    }
                }
            }
        }
    } else {
        // wider keys: one record at a time, four candidates in flight (the batched form costs more registers than
        // it saves: measured 8 % slower for 16-byte keys)
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const uint32_t p = (uint32_t)(i * NT + tid);
            dest[i] = 0xFFFFFFFFu;
            if (p < n) {
                const uint32_t d = (uint32_t)((keys[i].w[0] - kmin) >> sh);
                const uint32_t sb = d ? bins[d - 1] : 0u, e = bins[d];
                uint32_t before = 0;
                if (e - sb > 1) {
                    for (uint32_t y = sb; y < e; y += 4) {
                        Key<W> o[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) o[u] = key_load<W>(&skeys[y + u < e ? y + u : e - 1]);
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            if (y + u < e) {
                                const bool lt = key_less_words<W>(o[u], keys[i]);
                                const bool eq = key_eq<W>(o[u], keys[i]);
                                before += (lt || (eq && y + u < pos_of[i])) ? 1u : 0u;
                            }
                        }
                    }
                }
                dest[i] = sb + before;
            }
        }
    }
    __syncthreads();  // every rank is computed from the scattered order: only now overwrite it
    BBK_PH(3, 4, t_prev);  // rank
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        if (dest[i] != 0xFFFFFFFFu) {
            key_store<W>(&skeys[dest[i]], keys[i]);
            if (IN_VAL) svals[dest[i]] = v[i];
        }
    }
    __syncthreads();
    BBK_PH(3, 5, t_prev);  // write
    bucket_reduce<W, NT, ITEMS, OP>(skeys, svals, scan_tmp, n, start, b, buf, vals, A);
    BBK_PH(3, 6, t_prev);  // heads + reduce + output
#ifdef BBK_PHASE_PROF
    if (threadIdx.x == 0) atomicAdd(&g_phase[3][7], 1ull);
#endif
}

template <int W, int NT, int ITEMS, int OP>
static size_t bucket_dist_smem() {
    return sizeof(uint32_t) * (DistBins<W, OP>::N + 32) + sizeof(uint64_t) * 2 * (NT / 64) + (size_t)W * 8 * NT * ITEMS +
           (OP >= 2 ? 4 * NT * ITEMS : 0);
}

template <int W, int NT, int ITEMS, int OP>
static size_t bucket_smem() {
    return sizeof(uint32_t) * ((NT / 64) * 256 + 256 + 32) + (size_t)W * 8 * NT * ITEMS + (OP >= 2 ? 4 * NT * ITEMS : 0);
}

// ---- narrow stage B (8-byte keys, key slots, no payload): 4-byte records from level 2 on
// The KEYS prefix is the key's top 32 bits, p = key >> (w0bits - 32).  Bucket g = bin j of the nb bins of segment s holds
// exactly the keys whose prefix lies in [s*P + q_j, s*P + q_(j+1)), with P = 2^(32 - b1) and q_j = ceil(j * P / nb): the
// inverse of bin_of, whose bin is umulhi(q << b1, nb) = floor(q * nb / P) for the low 32 - b1 prefix bits q.  Its smallest
// key is base[g] = (s*P + q_j) << (w0bits - 32).  When no bucket spans more than 2^32 keys (ceil(P / nb) << (w0bits - 32)
// <= 2^32 for every non-empty segment: the host checks) a key of bucket g is base[g] + (uint32_t)(lo - (uint32_t)base[g]),
// lo being its low word.  So level 2 stores lo only (k_part<..., NOUT>) and k_bucket_dist_nb sorts the 32-bit offsets
// lo - (uint32_t)base[g] and widens them on the way out.  (w0bits <= 32: the key is its low word, base 0.)
__global__ void k_bucket_base(const uint32_t *__restrict__ seg_nb2, const uint32_t *__restrict__ seg_bin, uint32_t nseg,
                              uint32_t nbuckets, int b1, int w0bits, uint64_t *__restrict__ base) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nbuckets) return;
    uint32_t lo = 0, hi = nseg;  // largest s with seg_bin[s] <= g (every segment has at least one bin)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (seg_bin[mid] <= g) lo = mid;
        else hi = mid;
    }
    const uint64_t P = 1ull << (32 - b1), nb = seg_nb2[lo], j = g - seg_bin[lo];
    const uint64_t p = lo * P + (j * P + nb - 1) / nb;
    base[g] = w0bits > 32 ? p << (w0bits - 32) : 0ull;
}

// k_bucket_dist (OP 0, sorted result written directly) on those 4-byte records: the same distribution sort and in-bin
// ranking over 32-bit offsets, with half the LDS (38 KB against 61 KB) and at most 80 registers (76: four records per
// ranking round instead of six), so that three workgroups fit a CU instead of two.  A bucket it turns down, a duplicate or a spill
// sends the call back to the exact mode, as on the 8-byte key slots, so no second-chance kernel needs this form.
template <int NT, int ITEMS>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(6, 6))) void k_bucket_dist_nb(const uint32_t *__restrict__ buf, const uint64_t *__restrict__ base,
                                                       BucketArgs A) {
    constexpr int CAP = NT * ITEMS;
    constexpr int NWAVES = NT / 64;
    constexpr int DB = DistBins<1, 0>::N;
    constexpr int BPT = DB / NT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // layout: bins[DB] | scan[32] | mm[2 * NWAVES] | skeys[CAP] (offsets from the bucket's base)
    uint32_t *bins = reinterpret_cast<uint32_t *>(smem);
    uint32_t *scan_tmp = bins + DB;
    uint32_t *mm = scan_tmp + 32;
    uint32_t *skeys = mm + 2 * NWAVES;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t b = A.bucket_ids ? A.bucket_ids[blockIdx.x] : blockIdx.x;
    uint32_t start, n;
    bucket_range(A, b, &start, &n);
    if (n == 0) {
        if (tid == 0) A.dcount[b] = 0;
        return;
    }
    if (n > (uint32_t)CAP) {
        if (tid == 0) A.dcount[b] = 0xFFFFFFFFu;
        return;
    }
    for (uint32_t q = tid; q < (uint32_t)DB; q += NT) bins[q] = 0;
#ifdef BBK_PHASE_PROF
    unsigned long long t_prev = clock64();
#endif

    const uint64_t kbase = base[b];
    uint32_t keys[ITEMS];  // offsets from the base: the key order
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t p = (uint32_t)(i * NT + tid);
        keys[i] = buf[start + (p < n ? p : n - 1u)];
    }
    uint32_t mn = ~0u, mx = 0;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {  // clamped duplicates do not change min / max
        keys[i] -= (uint32_t)kbase;
        mn = keys[i] < mn ? keys[i] : mn;
        mx = keys[i] > mx ? keys[i] : mx;
    }
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) {
        const uint32_t a = __shfl_xor(mn, dd, 64), c = __shfl_xor(mx, dd, 64);
        mn = a < mn ? a : mn;
        mx = c > mx ? c : mx;
    }
    if (lane == 0) {
        mm[2 * wave] = mn;
        mm[2 * wave + 1] = mx;
    }
    __syncthreads();  // bins zeroed, min / max of every wave visible
    mn = ~0u;
    mx = 0;
#pragma unroll
    for (int j = 0; j < NWAVES; ++j) {
        mn = mm[2 * j] < mn ? mm[2 * j] : mn;
        mx = mm[2 * j + 1] > mx ? mm[2 * j + 1] : mx;
    }
    BBK_PH(3, 0, t_prev);  // loads + min/max
    const uint32_t kmin = mn;
    const int rbits = 32 - __builtin_clz((mx - mn) | 1u);
    const int sh = rbits > DistBins<1, 0>::LOG ? rbits - DistBins<1, 0>::LOG : 0;  // digit = (offset - min) >> sh < bins

#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t p = (uint32_t)(i * NT + tid);
        if (p < n) atomicAdd(&bins[(keys[i] - kmin) >> sh], 1u);
    }
    __syncthreads();
    BBK_PH(3, 1, t_prev);  // count
    uint32_t c[BPT];
    uint32_t sum = 0;
    bool big = false;
#pragma unroll
    for (int q = 0; q < BPT; ++q) {
        c[q] = bins[tid * BPT + q];
        sum += c[q];
        big = big || c[q] > kDistMaxBin;
    }
    uint32_t incl = sum;
    incl = wave_scan_incl(incl);
    if (lane == 63) scan_tmp[wave] = incl;
    if (__syncthreads_or(big)) {
        if (tid == 0) A.dcount[b] = 0xFFFFFFFFu;
        return;
    }
    uint32_t first = incl - sum;
    for (int j = 0; j < wave; ++j) first += scan_tmp[j];
    {
        uint32_t ex = first;
#pragma unroll
        for (int q = 0; q < BPT; ++q) {
            bins[tid * BPT + q] = ex;
            ex += c[q];
        }
    }
    __syncthreads();
    BBK_PH(3, 2, t_prev);  // scan
    uint32_t at[ITEMS];  // where the scatter put the record (breaks ties between equal offsets), then its final place
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t p = (uint32_t)(i * NT + tid);
        at[i] = 0xFFFFFFFFu;
        if (p < n) {
            const uint32_t pos = atomicAdd(&bins[(keys[i] - kmin) >> sh], 1u);
            skeys[pos] = keys[i];
            at[i] = pos;
        }
    }
    __syncthreads();
    BBK_PH(3, 3, t_prev);  // scatter
    // in-bin ranking as in k_bucket_dist: bin d = [bins[d-1], bins[d]) after the scatter, RB records per round with the
    // first four candidates of every bin read unconditionally (one array for both places saves eleven registers)
    constexpr int RB = 4;  // (6 as in k_bucket_dist: 93 registers, two workgroups per CU)
#pragma unroll
    for (int i0 = 0; i0 < ITEMS; i0 += RB) {
        uint32_t sb[RB], e[RB];
#pragma unroll
        for (int u = 0; u < RB; ++u) {
            const int i = i0 + u;
            sb[u] = e[u] = 0;
            if (i < ITEMS) {
                const uint32_t p = (uint32_t)(i * NT + tid);
                if (p < n) {
                    const uint32_t d = (keys[i] - kmin) >> sh;
                    sb[u] = d ? bins[d - 1] : 0u;
                    e[u] = bins[d];
                }
            }
        }
        uint32_t o[RB][4];
#pragma unroll
        for (int u = 0; u < RB; ++u) {
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                const uint32_t y = sb[u] + c4;
                o[u][c4] = skeys[y < e[u] ? y : (e[u] ? e[u] - 1u : 0u)];
            }
        }
#pragma unroll
        for (int u = 0; u < RB; ++u) {
            const int i = i0 + u;
            if (i < ITEMS) {
                const uint32_t p = (uint32_t)(i * NT + tid);
                if (p < n) {
                    uint32_t before = 0;
#pragma unroll
                    for (int c4 = 0; c4 < 4; ++c4) {
                        const uint32_t y = sb[u] + c4;
                        if (y < e[u]) before += (o[u][c4] < keys[i] || (o[u][c4] == keys[i] && y < at[i])) ? 1u : 0u;
                    }
                    for (uint32_t y = sb[u] + 4; y < e[u]; ++y) {  // bins above four records
                        const uint32_t ok = skeys[y];
                        before += (ok < keys[i] || (ok == keys[i] && y < at[i])) ? 1u : 0u;
                    }
                    at[i] = sb[u] + before;
                }
            }
        }
    }
    __syncthreads();  // every rank is computed from the scattered order: only now overwrite it
    BBK_PH(3, 4, t_prev);  // rank
#pragma unroll
    for (int i = 0; i < ITEMS; ++i)
        if (at[i] != 0xFFFFFFFFu) skeys[at[i]] = keys[i];
    __syncthreads();
    BBK_PH(3, 5, t_prev);  // write

    // heads (blocked ownership: thread t owns [t*ITEMS, (t+1)*ITEMS)), the distinct offsets compacted in LDS, then
    // widened and stored coalesced at the bucket's place in the result.  Every offset is a possible value: the first
    // record of the bucket is a head by position, not by comparison with a sentinel.
    uint32_t ostart = A.out_off ? A.out_off[b] : start;
    const uint32_t p0 = (uint32_t)tid * ITEMS;
    const uint32_t prev = (p0 > 0 && p0 - 1 < n) ? skeys[p0 - 1] : 0u;
    uint32_t mine[ITEMS];
    uint32_t nheads = 0, headbits = 0;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        mine[i] = 0;
        if (p0 + i < n) {
            mine[i] = skeys[p0 + i];
            const bool h = (i == 0) ? (p0 == 0 || mine[0] != prev) : mine[i] != mine[i - 1];
            if (h) {
                headbits |= 1u << i;
                ++nheads;
            }
        }
    }
    uint32_t excl, total;
    {
        uint32_t hincl = wave_scan_incl(nheads);
        __syncthreads();  // everyone has its offsets in registers: skeys may be reused below
        if (lane == 63) scan_tmp[wave] = hincl;
        __syncthreads();
        uint32_t wbase, tot;
        wave_totals<NWAVES>(scan_tmp, lane, wave, wbase, tot);
        excl = wbase + hincl - nheads;
        total = tot;
        asm volatile("" : "+v"(ostart));  // awaited here, not inside the store loop (see bucket_reduce)
    }
    int seg = (int)excl - 1;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i)
        if (p0 + i < n && (headbits & (1u << i))) skeys[++seg] = mine[i];
    __syncthreads();
    uint64_t *dst = reinterpret_cast<uint64_t *>(A.sorted_keys) + ostart;
    for (uint32_t s = tid; s < total; s += NT) dst[s] = (kbase + skeys[s]) & A.strip_mask;
    if (tid == 0 && total != n) atomicOr(A.dup_flag, 1u);
    if (tid == 0) A.dcount[b] = total;
    BBK_PH(3, 6, t_prev);  // heads + output
#ifdef BBK_PHASE_PROF
    if (threadIdx.x == 0) atomicAdd(&g_phase[3][7], 1ull);
#endif
}

template <int NT, int ITEMS>
static size_t bucket_dist_nb_smem() {
    return sizeof(uint32_t) * (DistBins<1, 0>::N + 32 + 2 * (NT / 64) + (size_t)NT * ITEMS);
}

// ---- dedup by an LDS hash table (8-byte keys): when the caller only needs the distinct set (the
// hash-partitioned first stage: a second stage sorts the survivors anyway) the bucket does not have
// to be sorted.  Records are streamed from HBM straight into an open-addressing table with 64-bit
// ds_cmpst; with 50x coverage ~8 of 9 records find their key already there on the first probe.
// ~30 instructions per record instead of 6 radix passes.  The distinct keys (+ reduced payload)
// are written back in place in table order.
#ifdef BBK_AB_TABLE_WALK  // (A/B: the distinct keys always collected by a walk over the table's slots, as before round 3)
constexpr bool kHashDirectOut = false;
#else
constexpr bool kHashDirectOut = true;
#endif
constexpr int kHashThreads = 512;
#ifndef BBK_HASH_ITEMS
#define BBK_HASH_ITEMS 16
#endif
constexpr int kHashItems = BBK_HASH_ITEMS;          // 512 x 16 = 8192 records per bucket (x 12: 2 % slower, and the
                                                    // fullest bucket of a 10 M-read batch then overflows its slot)
constexpr uint32_t kHashSlots = 8192;               // distinct keys of a bucket: ~n / multiplicity, far below the slots
                                                    // for read data; all-distinct input fills ~0.7 of them
constexpr uint32_t kHashMaxProbes = 256;            // a probe sequence this long means the table is (nearly) full: the
                                                    // bucket holds more distinct keys than slots -> left to the caller

template <int OP>
__global__ __launch_bounds__(kHashThreads) void k_bucket_hash(Key<1> *__restrict__ buf, uint32_t *__restrict__ vals,
                                                             BucketArgs A) {
    constexpr bool IN_VAL = OP >= 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long *tab = reinterpret_cast<unsigned long long *>(smem);
    uint32_t *pay = reinterpret_cast<uint32_t *>(smem + sizeof(unsigned long long) * kHashSlots);
    uint32_t *scan_tmp = pay + (OP != 0 ? kHashSlots : 0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t b = A.bucket_ids ? A.bucket_ids[blockIdx.x] : blockIdx.x;
    uint32_t start, n;
    bucket_range(A, b, &start, &n);
    if (n == 0) {
        if (tid == 0) A.dcount[b] = 0;
        return;
    }
    if (n > (uint32_t)(kHashThreads * kHashItems)) {
        if (tid == 0) A.dcount[b] = 0xFFFFFFFFu;
        return;
    }
    constexpr unsigned long long EMPTY = ~0ull;
#ifdef BBK_PHASE_PROF
    unsigned long long t_prev = clock64();
#endif
    uint64_t kk[kHashItems];
    uint32_t vv[kHashItems];
#pragma unroll
    for (int i = 0; i < kHashItems; ++i) {  // all loads first: independent, in flight together -- and while the table
        const uint32_t p = (uint32_t)(i * kHashThreads + tid);  // is cleared below
        kk[i] = EMPTY;
        vv[i] = 0;
        if (p < n) {
            kk[i] = buf[start + p].w[0];
            if (IN_VAL) vv[i] = vals[start + p];
        }
    }
    for (uint32_t s = tid; s < kHashSlots; s += kHashThreads) {
        tab[s] = EMPTY;
        if (OP != 0) pay[s] = 0;
    }
    if (tid == 0) scan_tmp[14] = 0;
    __syncthreads();
    BBK_PH(4, 0, t_prev);  // table init
    uint32_t firsts = 0;  // bit i: record i of this lane was the first of its key in the table
    static_assert(kHashItems <= 32, "one bit per record of a lane");
#pragma unroll
    for (int i = 0; i < kHashItems; ++i) {
        if (kk[i] != EMPTY) {
            // 32-bit mix with multipliers of its own (the partition levels consumed the top bits of part_hash32)
            uint32_t h = ((uint32_t)kk[i] ^ 0x7F4A7C15u) * 0x2C1B3C6Du;
            h ^= h >> 15;
            h += (uint32_t)(kk[i] >> 32) * 0x297A2D39u;
            h ^= h >> 14;
            h *= 0x9E3779B1u;
            uint32_t slot = (h >> 19) & (kHashSlots - 1);
            // (probing all records of a lane in rounds, 12 ds_cmpst in flight, was measured 15 % slower)
            uint32_t probes = 0;
            for (;;) {
                const unsigned long long old = atomicCAS(&tab[slot], EMPTY, (unsigned long long)kk[i]);
                if (old == EMPTY) firsts |= 1u << i;
                if (old == EMPTY || old == kk[i]) break;
                slot = (slot + 1) & (kHashSlots - 1);
                if (kHashItems * kHashThreads > (int)(kHashSlots * 3 / 4) && ++probes > A.max_probes) {
                    scan_tmp[14] = 1;  // give up on this bucket (benign race: everyone writes 1)
                    break;
                }
            }
            if (OP == 1) atomicAdd(&pay[slot], 1u);
            else if (OP == 2) atomicAdd(&pay[slot], vv[i]);
            else if (OP == 3) atomicOr(&pay[slot], vv[i]);
        }
    }
    __syncthreads();
    if (scan_tmp[14]) {  // more distinct keys than the table takes: nothing has been written, the caller takes over
        if (tid == 0) A.dcount[b] = 0xFFFFFFFFu;
        return;
    }
    BBK_PH(4, 1, t_prev);  // loads + insert
    // compaction of the occupied slots: thread t owns slots t, t + 512, ... (consecutive lanes read
    // consecutive 8-byte slots: no LDS bank conflicts; the output order is free, the set is unsorted)
    constexpr int SPT = kHashSlots / kHashThreads;
    uint32_t cnt = 0;
    if constexpr (OP == 0 && kHashDirectOut) {
        cnt = (uint32_t)__popc(firsts);  // no payload to fetch: whoever put a key into the table writes it out
    } else {
#pragma unroll
        for (int j = 0; j < SPT; ++j) cnt += tab[j * kHashThreads + tid] != EMPTY ? 1u : 0u;
    }
    uint32_t incl = cnt;
    incl = wave_scan_incl(incl);
    if (lane == 63) scan_tmp[wave] = incl;
    __syncthreads();
    uint32_t wbase, total;
    wave_totals<kHashThreads / 64>(scan_tmp, lane, wave, wbase, total);
    Key<1> *obuf = buf;  // back to the head of the bucket (every record has been read before the barrier above)
    uint32_t *ovals = vals;
    const uint32_t obase = start;
    uint32_t o = obase + wbase + incl - cnt;
    if constexpr (OP == 0 && kHashDirectOut) {
#pragma unroll
        for (int i = 0; i < kHashItems; ++i) {
            if (firsts & (1u << i)) obuf[o++].w[0] = kk[i];
        }
    } else {
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            const unsigned long long key = tab[j * kHashThreads + tid];
            if (key != EMPTY) {
                obuf[o].w[0] = key;
                if (OP != 0) ovals[o] = pay[j * kHashThreads + tid];
                ++o;
            }
        }
    }
    BBK_PH(4, 2, t_prev);  // compaction + output
#ifdef BBK_PHASE_PROF
    if (threadIdx.x == 0) atomicAdd(&g_phase[4][7], 1ull);
#endif
    if (tid == 0) A.dcount[b] = total;
}

// Same idea for wider keys: the bucket's keys are staged in LDS and the table holds record INDICES
// (32-bit ds_cmpst); a probe that finds a different index compares the two keys.  All keys are in
// LDS before the first insertion, so there is no partially written slot to race with.
constexpr int kHashIdxThreads = 512;
// 16-byte keys: 512 x 8 = 4096 records per bucket, 8192 slots; 24/32-byte keys: 512 x 4 = 2048 records, 4096 slots
// (keys + table + payload table must fit the 160 KB of LDS)
template <int W>
struct HashIdxCfg {
    static constexpr int ITEMS = (W <= 2) ? 8 : 4;
    static constexpr uint32_t CAP = kHashIdxThreads * ITEMS;
    static constexpr uint32_t SLOTS = 2 * CAP;
};

template <int W, int OP>
__global__ __launch_bounds__(kHashIdxThreads) void k_bucket_hashidx(Key<W> *__restrict__ buf,
                                                                   uint32_t *__restrict__ vals, BucketArgs A) {
    constexpr int kHashIdxItems = HashIdxCfg<W>::ITEMS;
    constexpr uint32_t kHashIdxCap = HashIdxCfg<W>::CAP, kHashIdxSlots = HashIdxCfg<W>::SLOTS;
    constexpr bool IN_VAL = OP >= 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *tab = reinterpret_cast<uint32_t *>(smem);
    uint32_t *pay = tab + kHashIdxSlots;
    uint32_t *scan_tmp = pay + (OP != 0 ? kHashIdxSlots : 0);
    Key<W> *skeys = reinterpret_cast<Key<W> *>(scan_tmp + 32);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t b = A.bucket_ids ? A.bucket_ids[blockIdx.x] : blockIdx.x;
    uint32_t start, n;
    bucket_range(A, b, &start, &n);
    if (n == 0) {
        if (tid == 0) A.dcount[b] = 0;
        return;
    }
    if (n > kHashIdxCap) {
        if (tid == 0) A.dcount[b] = 0xFFFFFFFFu;
        return;
    }
    constexpr uint32_t EMPTY = 0xFFFFFFFFu;
    for (uint32_t s = tid; s < kHashIdxSlots; s += kHashIdxThreads) {
        tab[s] = EMPTY;
        if (OP != 0) pay[s] = 0;
    }
    uint32_t vv[kHashIdxItems];
    {
        // loads first, unconditional (see k_bucket)
        Key<W> rk[kHashIdxItems];
#pragma unroll
        for (int i = 0; i < kHashIdxItems; ++i) {
            const uint32_t p = (uint32_t)(i * kHashIdxThreads + tid);
            const uint32_t at = start + (p < n ? p : n - 1u);
            rk[i] = key_load<W>(&buf[at]);
            vv[i] = IN_VAL ? vals[at] : 0u;
        }
#pragma unroll
        for (int i = 0; i < kHashIdxItems; ++i) {
            const uint32_t p = (uint32_t)(i * kHashIdxThreads + tid);
            if (p < n) key_store<W>(&skeys[p], rk[i]);
            else vv[i] = 0;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kHashIdxItems; ++i) {
        const uint32_t p = (uint32_t)(i * kHashIdxThreads + tid);
        if (p < n) {
            const Key<W> key = key_load<W>(&skeys[p]);
            // bits of the hash other than the ones the partition consumed (its top ~20)
            uint32_t slot = (part_hash32<W>(key) * 0x9E3779B1u >> 7) & (kHashIdxSlots - 1);
            for (;;) {
                const uint32_t old = atomicCAS(&tab[slot], EMPTY, p);
                if (old == EMPTY) break;
                if (key_eq<W>(key_load<W>(&skeys[old]), key)) break;
                slot = (slot + 1) & (kHashIdxSlots - 1);
            }
            if (OP == 1) atomicAdd(&pay[slot], 1u);
            else if (OP == 2) atomicAdd(&pay[slot], vv[i]);
            else if (OP == 3) atomicOr(&pay[slot], vv[i]);
        }
    }
    __syncthreads();
    constexpr int SPT = kHashIdxSlots / kHashIdxThreads;
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < SPT; ++j) cnt += tab[j * kHashIdxThreads + tid] != EMPTY ? 1u : 0u;  // no bank conflicts
    uint32_t incl = cnt;
    incl = wave_scan_incl(incl);
    if (lane == 63) scan_tmp[wave] = incl;
    __syncthreads();
    uint32_t wbase, total;
    wave_totals<kHashIdxThreads / 64>(scan_tmp, lane, wave, wbase, total);
    Key<W> *obuf = buf;  // back to the head of the bucket (every record has been read before the barrier above)
    uint32_t *ovals = vals;
    const uint32_t obase = start;
    uint32_t o = obase + wbase + incl - cnt;
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
        const uint32_t idx = tab[j * kHashIdxThreads + tid];
        if (idx != EMPTY) {
            key_store<W>(&obuf[o], key_load<W>(&skeys[idx]));
            if (OP != 0) ovals[o] = pay[j * kHashIdxThreads + tid];
            ++o;
        }
    }
    if (tid == 0) A.dcount[b] = total;
}

template <int W, int OP>
static size_t bucket_hashidx_smem() {
    return 4 * HashIdxCfg<W>::SLOTS + (OP != 0 ? 4 * HashIdxCfg<W>::SLOTS : 0) + 128 + (size_t)W * 8 * HashIdxCfg<W>::CAP;
}

template <int OP>
static size_t bucket_hash_smem() {
    return sizeof(unsigned long long) * kHashSlots + (OP != 0 ? 4 * kHashSlots : 0) + 64;
}

// one wave per bucket: dense output
template <int W, bool HAS_VAL>
__global__ __launch_bounds__(256) void k_compact(const Key<W> *__restrict__ buf, const uint32_t *__restrict__ vals,
                                                const uint32_t *__restrict__ boff, const uint32_t *__restrict__ dcount,
                                                const uint64_t *__restrict__ doff, uint32_t nbuckets,
                                                Key<W> *__restrict__ out, uint32_t *__restrict__ vout,
                                                uint64_t mask0,  // cleared from word 0 (sort tag), else ~0
                                                uint32_t slot_cap) {  // boff == null: bucket b starts at b*slot_cap
    const uint32_t b = (uint32_t)((BBK_GID()) >> 6);
    if (b >= nbuckets) return;
    const int lane = threadIdx.x & 63;
    uint32_t c = dcount[b];
    if (c == 0xFFFFFFFFu) c = 0;  // left to the caller (reprocessed with the spill list)
    const uint32_t s = boff ? boff[b] : b * slot_cap;
    const uint64_t d = doff[b];
    for (uint32_t i = lane; i < c; i += 64) {
        Key<W> key = key_load<W>(&buf[s + i]);
        key.w[0] &= mask0;
        key_store<W>(&out[d + i], key);
        if (HAS_VAL) vout[d + i] = vals[s + i];
    }
}

// ids of the buckets the first-pass kernel left alone (dcount == 0xFFFFFFFF); *count may run past cap
__global__ void k_flagged(const uint32_t *__restrict__ dcount, uint32_t n, uint32_t *__restrict__ ids, uint32_t cap,
                          uint32_t *__restrict__ count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && dcount[i] == 0xFFFFFFFFu) {
        const uint32_t at = atomicAdd(count, 1u);
        if (at < cap) ids[at] = i;
    }
}

// slot mode, one thread per bucket: its cursor starts at its slot; bucket_seg (narrow path, else null) gets the level-1
// segment the bucket belongs to, the largest s in [0, nseg) with seg_bin[s] <= bucket
__global__ void k_bucket_init(uint32_t *__restrict__ cursor, uint32_t n, uint32_t stride,
                              const uint32_t *__restrict__ seg_bin, uint32_t nseg, uint16_t *__restrict__ bucket_seg) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    cursor[i] = i * stride;
    if (bucket_seg) {
        uint32_t lo = 0, hi = nseg;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (seg_bin[mid] <= i) lo = mid;
            else hi = mid;
        }
        bucket_seg[i] = (uint16_t)lo;
    }
}

__global__ void k_u32_to_u64(const uint32_t *__restrict__ in, uint64_t n, uint64_t *__restrict__ out, uint32_t clampv) {
    const uint64_t i = BBK_GID();
    if (i < n) out[i] = in[i] == 0xFFFFFFFFu ? (uint64_t)clampv : (uint64_t)in[i];
}

// d_total (optional): the total is still on the device
__global__ void k_scan_to_u32(const uint64_t *__restrict__ in, uint64_t n, uint64_t total,
                              const uint64_t *__restrict__ d_total, uint32_t *__restrict__ out) {
    const uint64_t i = BBK_GID();
    if (i < n) out[i] = (uint32_t)in[i];
    if (i == n) out[n] = (uint32_t)(d_total ? *d_total : total);
}

// k-mers and chunks (of ch k-mer positions) of every read; *unordered is set when the packed words of the reads do not
// lie one after the other in read order (then no tile stages its window of words in LDS: k_tile_reads)
__global__ void k_kmers_per_read2(const uint32_t *__restrict__ len, const uint64_t *__restrict__ woff, uint64_t n,
                                  uint32_t k, uint32_t ch, uint64_t *__restrict__ nk, uint64_t *__restrict__ nch,
                                  uint32_t *__restrict__ unordered) {
    const uint64_t i = BBK_GID();
    if (i < n) {
        const uint32_t L = len[i];
        const uint64_t c = L >= k ? (uint64_t)(L - k + 1) : 0ull;
        nk[i] = c;
        nch[i] = (c + ch - 1) / ch;
        if (i + 1 < n && woff[i + 1] < woff[i] + ((L + 31u) >> 5)) *unordered = 1u;
    }
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
                                  // (x 8 records) with the tables 77 KB of LDS: two workgroups per CU
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
    if (s_rel[g] > c || s_rel[g + 1] <= c) g = read_of(s_rel, nr, c);
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
// r = #marks at or before pos - 1 (a 64-position word of marks is exactly what a wave handles per step).  What a
// store needs of its bin -- global offset and room left in the slot -- sits in one 8-byte entry indexed by r.
template <bool HAS_VAL>
__global__ __launch_bounds__(kNwThreads) __attribute__((amdgpu_waves_per_eu(BBK_NW_WAVES, BBK_NW_WAVES))) void k_part_reads_narrow(ReadSrc S, PartLevel L, uint32_t ntiles,
                                                                 const RdTile *__restrict__ tiles_arg,  // = S.tiles: as an
                                                                 // argument of its own the descriptor is a scalar load
                                                                 uint32_t *__restrict__ cursor,
                                                                 uint32_t *__restrict__ out, uint32_t *__restrict__ vout) {
    constexpr int NT = kNwThreads, CH = 8, MAXB = kNwBins1, ITEMS = CH * NwCfg<HAS_VAL>::ROUNDS;
    constexpr int MW = NwCfg<HAS_VAL>::TILE / 64;  // 64-bit mark words
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *lhist = reinterpret_cast<uint32_t *>(smem);                   // counts; later, with the next array:
    uint2 *tab = reinterpret_cast<uint2 *>(smem);                           // r -> (global offset - staged start, limit)
    uint32_t *lstart = lhist + 2 * MAXB;
    uint32_t *scan_tmp = lstart + MAXB;                                     // 64 entries
    unsigned long long *mark = reinterpret_cast<unsigned long long *>(scan_tmp + 64);  // MW words
    uint16_t *mbase = reinterpret_cast<uint16_t *>(mark + MW);              // marks before every word
    uint16_t *nz = mbase + MW;                                              // r-th non-empty bin
    unsigned char *U = reinterpret_cast<unsigned char *>(nz + MAXB);
    int32_t *s_rel = reinterpret_cast<int32_t *>(U);
    int32_t *s_wrel = s_rel + (kRdSlots + 2);
    uint32_t *s_len = reinterpret_cast<uint32_t *>(s_wrel + (kRdSlots + 2));
    uint64_t *s_words = reinterpret_cast<uint64_t *>(s_len + (kRdSlots + 2));
    uint32_t *stage = reinterpret_cast<uint32_t *>(U);
    uint8_t *vstage = reinterpret_cast<uint8_t *>(stage + NwCfg<HAS_VAL>::TILE);  // payloads of this path are 8 mask bits

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
        const int lane = tid & 63, wave = tid >> 6;
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
        lhist[tid] = 0;  // NT == MAXB
        if (tid < 2 * MW) reinterpret_cast<uint32_t *>(mark)[tid] = 0u;
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

        // scan of the 1024 bin counts (one bin per thread) and of the non-empty flags; reservation of the tile's run
        const uint32_t c = lhist[tid];
        uint32_t incl = c;
        incl = wave_scan_incl(incl);
        const unsigned long long nzb = __ballot(c != 0);
        if (lane == 63) scan_tmp[wave] = incl | ((uint32_t)__popcll(nzb) << 16);  // records < 2^16, non-empty bins <= 1024
        __syncthreads();
        uint32_t before, total;
        wave_totals<NT / 64>(scan_tmp, lane, wave, before, total);
        const uint32_t staged = total & 0xFFFFu;
        const uint32_t ex = (before & 0xFFFFu) + incl - c;
        const uint32_t myr = (before >> 16) + (uint32_t)__popcll(nzb & ((1ull << lane) - 1ull));
        lstart[tid] = ex;
        uint32_t greserve = 0;
        if (c) {
            greserve = atomicAdd(&cursor[(tid << L.xcd_shift) + xcc], c);
            nz[myr] = (uint16_t)tid;
            atomicOr(&mark[ex >> 6], 1ull << (ex & 63u));
        }
        __syncthreads();  // (every thread has read its count: lhist may become the table)
        BBK_PH(5, 2, t_prev);  // scans + reservation issue + marks
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const int r = i / CH, j = i % CH;
            if ((uint32_t)j < ((cnts >> (4 * r)) & 15u)) {
                const uint32_t bin = (bins[r * 3 + j / 3] >> (10 * (j % 3))) & 1023u;
                const uint32_t pos = atomicAdd(&lstart[bin], 1u);  // (lstart ends as the bins' end offsets; nothing reads it again)
                stage[pos] = lo[i];
                if (HAS_VAL) vstage[pos] = (uint8_t)(masks[r * 2 + (j >> 2)] >> (8 * (j & 3)));
            }
        }
        asm volatile("" : "+v"(greserve));  // awaited by every lane here, not inside the store loop's conditional blocks
        if (c) {
            // first staged position of this bin that no longer fits its slot
            const uint64_t slot_end = L.xcd_shift ? (uint64_t)tid * L.slot_stride + (uint64_t)(xcc + 1u) * L.sub_cap
                                                  : (uint64_t)tid * L.slot_stride + L.slot_cap;
            const int64_t room = (int64_t)slot_end - (int64_t)greserve;
            tab[myr] = make_uint2(greserve - ex,
                                  (uint32_t)(int32_t)(room < -(int64_t)0x7FFF0000 ? -(int64_t)0x7FFF0000 : room) + ex);
        }
        if (wave == 0) {  // marks before every 64-position word: lane l owns words WPL*l .. WPL*l + WPL-1
            constexpr int WPL = (MW + 63) / 64;
            uint32_t pw[WPL], tot = 0;
#pragma unroll
            for (int j = 0; j < WPL; ++j) {
                const int idx = lane * WPL + j;
                pw[j] = tot;
                tot += idx < MW ? (uint32_t)__popcll(mark[idx]) : 0u;
            }
            uint32_t inc2 = tot;
            inc2 = wave_scan_incl(inc2);
            const uint32_t lb = inc2 - tot;
#pragma unroll
            for (int j = 0; j < WPL; ++j) {
                const int idx = lane * WPL + j;
                if (idx < MW) mbase[idx] = (uint16_t)(lb + pw[j]);
            }
        }
        __syncthreads();
        BBK_PH(5, 3, t_prev);  // reorder into LDS + mark prefix
        if (more) prefetch(Tn, Q);  // in flight during the stores below
        else Q = Pre{0, 0, 0, 0, 0};   // (the old values end here either way: they must not stay alive through the loop)
        const unsigned long long upto = (2ull << lane) - 1ull;  // this lane and the ones below
        // pos = i * NT + tid: the 64 lanes of a wave cover mark word i * (NT / 64) + wave
        const unsigned long long *wmark = mark + wave;
        const uint16_t *wmbase = mbase + wave;
        uint32_t full = 0;  // items whose slot is full (rare; handled after the stores so that no atomic sits between them)
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const uint32_t pos = (uint32_t)i * NT + tid;
            if (pos < staged) {
                const uint32_t r = (uint32_t)wmbase[i * (NT / 64)] + (uint32_t)__popcll(wmark[i * (NT / 64)] & upto) - 1u;
                unsigned long long e = reinterpret_cast<const unsigned long long *>(tab)[r];
                const uint32_t rec = stage[pos];
                asm volatile("" : "+v"(e));  // one 8-byte LDS read (otherwise: the limit, a branch, then the offset)
                if ((int32_t)pos >= (int32_t)(uint32_t)(e >> 32)) {
                    full |= 1u << i;
                } else {
                    const uint32_t g = (uint32_t)e + pos;
                    out[g] = rec;
                    if (HAS_VAL) vout[g] = vstage[pos];
                }
            }
        }
        if (full) {
#pragma unroll 1
            for (int i = 0; i < ITEMS; ++i) {
                if ((full >> i) & 1u) {
                    const uint32_t pos = (uint32_t)i * NT + tid;
                    const uint32_t r = (uint32_t)wmbase[i * (NT / 64)] + (uint32_t)__popcll(wmark[i * (NT / 64)] & upto) - 1u;
                    const uint32_t sp = atomicAdd(L.spill_count, 1u);
                    if (sp < L.spill_cap) {
                        reinterpret_cast<uint64_t *>(L.spill_keys)[sp] = nw_key(nz[r], stage[pos], hb);
                        if (HAS_VAL) L.spill_vals[sp] = vstage[pos];
                    }
                }
            }
        }
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
    const size_t fixed = sizeof(uint32_t) * (3 * kNwBins1 + 64) + (tile / 64) * (8 + 2) + (size_t)kNwBins1 * 2;
    return fixed + std::max(tables, stage);
}

// Level 2: one tile (<= 16384 records) of one segment -> the bucket slots of that segment.  Everything derives from lo.
constexpr int kNw2Threads = 1024;
// records per lane: 12 without payload (60 VGPRs: two workgroups of 1024 per CU; with 16 the kernel needed 72 and ran
// one: 3.2 -> 2.6 ms at BASELINE configs[1]), 8 with a payload (the mask array costs the registers of four records)
template <bool HAS_VAL>
struct Nw2Cfg {
    static constexpr int ITEMS = HAS_VAL ? 8 : 12;
    static constexpr int TILE = kNw2Threads * ITEMS;
};

template <bool HAS_VAL>
__global__ __launch_bounds__(kNw2Threads) void k_part_narrow2(const uint32_t *__restrict__ in, const uint32_t *__restrict__ vin,
                                                             const uint4 *__restrict__ desc, PartLevel L,
                                                             uint32_t *__restrict__ cursor, uint32_t *__restrict__ out,
                                                             uint32_t *__restrict__ vout) {
    constexpr int NT = kNw2Threads, ITEMS = Nw2Cfg<HAS_VAL>::ITEMS, MAXB = kMaxBins;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *lhist = reinterpret_cast<uint32_t *>(smem);
    uint32_t *lstart = lhist + MAXB;
    uint32_t *goff = lstart + MAXB;
    uint32_t *scan_tmp = goff + MAXB;
    uint32_t *stage = scan_tmp + 32;
    uint32_t *vstage = stage + Nw2Cfg<HAS_VAL>::TILE;
    const uint32_t tid = threadIdx.x;
    const int hb = L.narrow_hb;
    const uint4 d = desc[blockIdx.x];  // first record, records, bins of the segment | segment << 16, flat index of bin 0
    const uint32_t begin = d.x, count = d.y, nb = d.z & 0xFFFFu, seg = d.z >> 16, gbin0 = d.w;
    if (count == 0) return;  // an unused place of the XCD-wise order (k_tile_desc_narrow)
    lhist[tid] = 0;  // NT == MAXB
    __syncthreads();
    uint32_t lo[ITEMS], vals[ITEMS], binrank[ITEMS];
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {  // all loads first (index clamped into the tile)
        const uint32_t local = (uint32_t)i * NT + tid;
        const uint32_t at = begin + (local < count ? local : count - 1u);
        lo[i] = in[at];
        vals[i] = HAS_VAL ? vin[at] : 0u;
    }
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        asm volatile("" : "+v"(lo[i]));
        if (HAS_VAL) asm volatile("" : "+v"(vals[i]));
    }
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t local = (uint32_t)i * NT + tid;
        binrank[i] = 0xFFFFFFFFu;
        if (local < count) {
            const uint32_t b = __umulhi(nw_p2(nw_mix(lo[i])), nb);
            const uint32_t rank = atomicAdd(&lhist[b], 1u);
            binrank[i] = (b << 16) | rank;
        }
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    const uint32_t c = tid < nb ? lhist[tid] : 0u;
    uint32_t incl = c;
    incl = wave_scan_incl(incl);
    if (lane == 63) scan_tmp[wave] = incl;
    __syncthreads();
    uint32_t wb, staged;
    wave_totals<NT / 64>(scan_tmp, lane, wave, wb, staged);
    const uint32_t ex = wb + incl - c;
    if (tid < nb) lstart[tid] = ex;
    uint32_t greserve = c ? atomicAdd(&cursor[gbin0 + tid], c) : 0u;
    __syncthreads();
    // the reservation's result is awaited HERE, by every lane: the compiler otherwise puts the wait for it (vmcnt 0) into
    // the conditional blocks of the store loop below, where it makes every store wait for the one before
    asm volatile("" : "+v"(greserve));
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        if (binrank[i] != 0xFFFFFFFFu) {
            const uint32_t pos = lstart[binrank[i] >> 16] + (binrank[i] & 0xFFFFu);
            stage[pos] = lo[i];
            if (HAS_VAL) vstage[pos] = vals[i];
        }
    }
    if (tid < nb) {
        goff[tid] = greserve - ex;
        const int64_t room = (int64_t)((uint64_t)(gbin0 + tid) * L.slot_stride + L.slot_cap) - (int64_t)greserve;
        lhist[tid] = (uint32_t)(int32_t)(room < -(int64_t)0x7FFF0000 ? -(int64_t)0x7FFF0000 : room) + ex;
    }
    __syncthreads();
    // (records whose slot is full are rare and handled after the stores: the spill counter's atomic returns a value, and
    // a wait for it between the stores would make every store wait for the one before)
    uint32_t full = 0;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t pos = (uint32_t)i * NT + tid;
        if (pos < staged) {
            const uint32_t rec = stage[pos];
            const uint32_t b = __umulhi(nw_p2(nw_mix(rec)), nb);
            if ((int32_t)pos >= (int32_t)lhist[b]) {
                full |= 1u << i;
            } else {
                const uint32_t g = goff[b] + pos;
                out[g] = rec;
                if (HAS_VAL) vout[g] = vstage[pos];
            }
        }
    }
    if (full) {
#pragma unroll 1
        for (int i = 0; i < ITEMS; ++i) {
            if ((full >> i) & 1u) {
                const uint32_t pos = (uint32_t)i * NT + tid;
                const uint32_t sp = atomicAdd(L.spill_count, 1u);
                if (sp < L.spill_cap) {
                    reinterpret_cast<uint64_t *>(L.spill_keys)[sp] = nw_key(seg, stage[pos], hb);
                    if (HAS_VAL) L.spill_vals[sp] = vstage[pos];
                }
            }
        }
    }
}

static size_t part_narrow2_smem(bool has_val) {
    return sizeof(uint32_t) * (3 * kMaxBins + 32) + (size_t)(has_val ? Nw2Cfg<true>::TILE : Nw2Cfg<false>::TILE) * 4 * (has_val ? 2 : 1);
}

// level-2 tile descriptors of the narrow path: like k_tile_desc, with the segment id beside the bin count
// xstart (optional): the tiles of level-1 segment s are dealt to the workgroups that run on XCD s % 8 (workgroup b runs on
// XCD b % 8): tile i of M-entry e becomes workgroup 8 * (xstart[e] + i) + s % 8.  All tiles that fill the buckets of one
// segment then write through ONE L2 (lines filled from several XCDs are what makes a scatter slow, see the level-1 call
// site), and few segments are in flight per XCD at a time.  Unused places keep a zero descriptor (no records).
__global__ void k_tile_desc_narrow(TileMap M, const uint32_t *__restrict__ seg_nb2, const uint32_t *__restrict__ seg_bin_start,
                                   uint32_t tile_size, int sub_shift, const uint32_t *__restrict__ xstart,
                                   uint4 *__restrict__ desc) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= M.ntiles) return;
    uint32_t lo = 0, hi = M.nseg;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (M.seg_tile_start[mid] <= t) lo = mid;
        else hi = mid;
    }
    const uint32_t b = M.seg_off[lo] + (t - M.seg_tile_start[lo]) * tile_size;
    const uint32_t e = M.seg_off[lo] + M.seg_size[lo];
    const uint32_t seg = lo >> sub_shift;  // M's entries are the per-XCD sub-slots of the level-1 segments
    const uint32_t at = xstart ? 8u * (xstart[lo] + (t - M.seg_tile_start[lo])) + (seg & 7u) : t;
    desc[at] = make_uint4(b, (e - b) < tile_size ? (e - b) : tile_size, seg_nb2[seg] | (seg << 16), seg_bin_start[seg]);
}

// Dedup of one bucket of 4-byte records in an LDS table (32-bit ds_cmpst); the distinct records leave as 8-byte keys
// rebuilt from (segment of the bucket, lo).  The all-ones record (16 x T) is the table's empty marker and is counted
// on the side.
constexpr int kNwHashThreads = 512;
constexpr int kNwHashItems = 16;  // 8192 records per bucket
constexpr uint32_t kNwHashSlots = 8192;

template <int OP>
__global__ __launch_bounds__(kNwHashThreads) void k_bucket_hash32(uint32_t *__restrict__ buf,
                                                                 uint32_t *__restrict__ vals, BucketArgs A,
                                                                 const uint16_t *__restrict__ bucket_seg, int hb) {
    constexpr bool IN_VAL = OP >= 2;
    constexpr uint32_t EMPTY = 0xFFFFFFFFu;
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
    const unsigned long long t_prev = 0;
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
    uint32_t kk[kNwHashItems], vv[kNwHashItems];
#pragma unroll
    for (int i = 0; i < kNwHashItems; ++i) {  // (the loads are in flight while the table is cleared)
        const uint32_t p = (uint32_t)(i * kNwHashThreads + tid);
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
        const uint32_t p = (uint32_t)(i * kNwHashThreads + tid);
        if (p < n) {
            if (kk[i] == EMPTY) {
                scan_tmp[13] = 1;
                if (OP == 1) atomicAdd(&scan_tmp[12], 1u);
                else if (OP == 2) atomicAdd(&scan_tmp[12], vv[i]);
                else if (OP == 3) atomicOr(&scan_tmp[12], vv[i]);
                continue;
            }
            uint32_t slot = nw_slot(nw_mix(kk[i])) & (kNwHashSlots - 1);
            uint32_t probes = 0;
            for (;;) {
                const uint32_t old = atomicCAS(&tab[slot], EMPTY, kk[i]);
                if (old == EMPTY) firsts |= 1u << i;
                if (old == EMPTY || old == kk[i]) break;
                slot = (slot + 1) & (kNwHashSlots - 1);
                if (++probes > A.max_probes) {
                    scan_tmp[14] = 1;
                    break;
                }
            }
            if (OP == 1) atomicAdd(&pay[slot], 1u);
            else if (OP == 2) atomicAdd(&pay[slot], vv[i]);
            else if (OP == 3) atomicOr(&pay[slot], vv[i]);
        }
    }
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

// ------------------------------------------------------------------------------------------
// stage B's level 1 straight from stage A's buckets (BucketView, msd.h)
// ------------------------------------------------------------------------------------------
// Tile t of the both-strand records covers the canonical keys c in [t * TILE/2, (t+1) * TILE/2) of the dense order:
// record 2c is key c, record 2c+1 its reverse complement, as in tile_load's expand_k branch.  Key c is the 4-byte word
// slots[b * stride + c - off[b]] of the bucket b with off[b] <= c < off[b + 1], widened with the bucket's segment.
// A tile spans ~6 buckets of ~690 keys at the flagship size; their offsets and segments are staged in LDS.
constexpr int kViewSpan = 64;  // buckets of one tile staged in LDS (more: the lanes search the global table)

// largest b in [lo, hi) with off[b] <= c (off[lo] <= c)
__device__ inline uint32_t view_bucket(const uint64_t *__restrict__ off, uint32_t lo, uint32_t hi, uint64_t c) {
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (off[mid] <= c) lo = mid;
        else hi = mid;
    }
    return lo;
}

// one thread per tile: the buckets of its first and last key
__global__ void k_view_tile_desc(const uint64_t *__restrict__ off, uint32_t nbuckets, uint64_t D, uint32_t keys_per_tile,
                                 uint32_t ntiles, uint2 *__restrict__ desc) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntiles) return;
    const uint64_t c0 = (uint64_t)t * keys_per_tile;
    const uint64_t c1 = (c0 + keys_per_tile < D ? c0 + keys_per_tile : D) - 1u;
    const uint32_t b0 = view_bucket(off, 0, nbuckets, c0);
    desc[t] = make_uint2(b0, view_bucket(off, b0, nbuckets, c1));
}

// k_part (8-byte keys, level-1 scatter, no payload) whose tile comes from the view.  TAG: the XXH3 bucket of 16 above
// the k-mer (M.expand_tag).  Each lane loads a key once and emits it and its reverse complement as its adjacent pair.
template <bool TAG>
__global__ __launch_bounds__(PartCfg<1>::THREADS) void k_part_view(const uint32_t *__restrict__ slots,
                                                                   const uint64_t *__restrict__ off,
                                                                   const uint16_t *__restrict__ seg,
                                                                   const uint2 *__restrict__ vdesc, uint32_t stride,
                                                                   int hb, TileMap M, PartLevel L,
                                                                   uint32_t *__restrict__ cursor,
                                                                   Key<1> *__restrict__ out) {
    constexpr int kItems = PartCfg<1>::ITEMS, kTile = PartCfg<1>::TILE, kThreads = PartCfg<1>::THREADS, MAXB = 512;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // layout: k_part's (lhist | lstart | goff | scan | stage) | toff[kViewSpan] | tseg[kViewSpan]
    uint32_t *lhist = reinterpret_cast<uint32_t *>(smem);
    uint32_t *lstart = lhist + MAXB;
    uint32_t *goff = lstart + MAXB;
    uint32_t *scan_tmp = goff + MAXB;
    Key<1> *stage = reinterpret_cast<Key<1> *>(scan_tmp + 32);
    uint32_t *toff = reinterpret_cast<uint32_t *>(stage + kTile);
    uint16_t *tseg = reinterpret_cast<uint16_t *>(toff + kViewSpan);
    uint32_t *vals_unused = nullptr;

    const int tid = threadIdx.x;
    const TileInfo T = tile_info(M, L, blockIdx.x, (uint32_t)kTile);
    const uint32_t count = T.count, nb = T.nb;  // count: records, even
    const uint2 d = vdesc[blockIdx.x];
    const uint32_t b0 = d.x, span = d.y - d.x + 1u;
    const bool staged = span <= (uint32_t)kViewSpan;  // uniform
    for (uint32_t b = tid; b < nb; b += kThreads) lhist[b] = 0;
    if (staged && tid < (int)span) {
        toff[tid] = (uint32_t)off[b0 + tid];  // key offsets < 2^32: one pass holds fewer records
        tseg[tid] = seg[b0 + tid];
    }
    __syncthreads();

    // item pair j of a lane = records 2c, 2c+1 of local key j * THREADS + tid (tile_local's pairs)
    const uint32_t c0 = (uint32_t)(T.begin >> 1), nkeys = count >> 1;
    uint32_t lo[kItems / 2], sg[kItems / 2];
#pragma unroll
    for (int j = 0; j < kItems / 2; ++j) {
        const uint32_t cl = (uint32_t)(j * kThreads + tid);
        const uint32_t c = c0 + (cl < nkeys ? cl : nkeys - 1u);  // clamped into the tile
        uint32_t b, base;
        if (staged) {
            uint32_t i = 0, hi = span;
            while (hi - i > 1) {
                const uint32_t mid = (i + hi) >> 1;
                if (toff[mid] <= c) i = mid;
                else hi = mid;
            }
            b = b0 + i;
            base = toff[i];
            sg[j] = tseg[i];
        } else {
            b = view_bucket(off, b0, d.y + 1u, c);
            base = (uint32_t)off[b];
            sg[j] = seg[b];
        }
        lo[j] = slots[(size_t)b * stride + (c - base)];
    }
    Key<1> keys[kItems];
    uint32_t binrank[kItems];
#pragma unroll
    for (int j = 0; j < kItems / 2; ++j) {
        Key<1> x, r;
        x.w[0] = nw_key(sg[j], lo[j], hb);
        r = kmer_rc<1>(x, M.expand_k);
        if (TAG) {
            x.w[0] |= __umul64hi(xxh3_64<1>(x), 16ull) << (2 * M.expand_k);
            r.w[0] |= __umul64hi(xxh3_64<1>(r), 16ull) << (2 * M.expand_k);
        }
        keys[2 * j] = x;
        keys[2 * j + 1] = r;
    }
    // in registers through the LDS reorder (see k_part)
#pragma unroll
    for (int i = 0; i < kItems; ++i) asm volatile("" : "+v"(keys[i].w[0]));
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
        const uint32_t local = tile_local<1, kThreads>(i, tid);
        binrank[i] = 0xFFFFFFFFu;
        if (local < count) {
            uint32_t pfx = prefix_of<1>(keys[i], L.dmode, L.w0bits);
            if (select_prefix(pfx, L)) {
                const uint32_t b = bin_of(pfx, L, nb);
                const uint32_t rank = atomicAdd(&lhist[b], 1u);
                binrank[i] = (b << 16) | rank;
            }
        }
    }
    __syncthreads();
    uint32_t vals[kItems] = {};
    part_tail<1, kItems, kThreads, MAXB, false, false>(keys, vals, binrank, lhist, lstart, goff, scan_tmp, stage,
                                                       vals_unused, nb, T.gbin0, L, cursor, out, nullptr, 0, 0ull);
}

static size_t part_view_smem() {
    return part_smem(1, PartCfg<1>::TILE, false, false, true) + (size_t)kViewSpan * (4 + 2);
}

// A key-slot give-up after the view's slots were released: the canonical keys again, from the level-1 records
// (both strands of every key, tag above bit 2k; odd k, so exactly one of a pair is canonical), in any order.  One
// workgroup per level-1 sub-slot; cap bounds the writes.
__global__ void k_view_recanon(const uint64_t *__restrict__ in, const uint32_t *__restrict__ seg_off,
                               const uint32_t *__restrict__ seg_size, int k, uint64_t *__restrict__ out, uint64_t cap,
                               uint32_t *__restrict__ count) {
    const uint32_t o = seg_off[blockIdx.x], n = seg_size[blockIdx.x];
    const uint64_t mask = (1ull << (2 * k)) - 1ull;
    const int lane = threadIdx.x & 63;
    for (uint32_t i0 = 0; i0 < n; i0 += blockDim.x) {  // uniform trip count: the ballot sees whole waves
        const uint32_t i = i0 + threadIdx.x;
        Key<1> x;
        x.w[0] = 0;
        bool keep = false;
        if (i < n) {
            x.w[0] = in[o + i] & mask;
            keep = !kmer_less_nucl<1>(kmer_rc<1>(x, k), x);
        }
        const uint64_t bal = __ballot(keep);
        uint32_t base = 0;
        if (lane == 0 && bal) base = atomicAdd(count, (uint32_t)__popcll(bal));
        base = __shfl(base, 0);
        const uint64_t at = (uint64_t)base + __popcll(bal & ((1ull << lane) - 1ull));
        if (keep && at < cap) out[at] = x.w[0];
    }
}

// ------------------------------------------------------------------------------------------
// stage B with the tag taken late (tagged sort of the both-strand set, fed from a BucketView, k <= 21)
// ------------------------------------------------------------------------------------------
// The tagged key is (tag: XXH3 bucket of 16) << 2k | k-mer, and the tag is a function of the k-mer.  Level 1 above
// bins by the top bits of the TAGGED key, so its records keep 37 of the 46 bits: 8 bytes each.  Here level 1 bins by the
// top ten bits of the k-mer alone (1024 segments, kMaxBins) and stores the remaining lobits = 2k - 10 <= 32 bits: 4-byte
// records, as in narrow stage A.  Level 2 knows the whole k-mer (segment, lo), takes the tag there and sends the record
// to bin tag * nsub + sub of its segment (sub: the next bits of lo, monotone, as bin_of).  Buckets then lie in memory
// as (segment, tag, sub) while the result is ordered (tag, segment, sub): the dense offsets come from a scan of the
// bucket fills gathered in that order (k_bucket_base_lt's perm).  A bucket holds lo in [q_j, q_(j+1)) of one segment
// and one tag, q_j = ceil(j * 2^lobits / nsub): fewer than 2^32 keys by construction, so level 2 stores the k-mer's low
// word and k_bucket_dist_nb sorts and widens it against base = tag << 2k | segment << lobits | q_j, unchanged.
// Both kernels share one tail, the one of k_part_reads_narrow: the staged order is bin-major, a bit per position
// marks where a non-empty bin starts, and what a store needs of its bin is one 8-byte LDS entry -- the bin of a
// staged record (ten dropped bits at level 1, a hash at level 2) is never computed twice.
constexpr int kLtThreads = 1024;  // == kMaxBins: one bin per thread in the scans
// records per lane.  Level 1: 14 336 records = 56 KB staged, 73 KB of LDS with the tables: two workgroups per CU (16
// records per lane would be 81.1 KB, one workgroup); a (tile, bin) run is 14 records = 56 bytes.  Level 2: as
// k_part_narrow2.
constexpr int kLt1Items = 14;
constexpr int kLt2Items = 12;

struct LtLds {
    uint32_t *lhist;           // counts; later, with the 4 KB behind it:
    uint2 *tab;                // r -> (global offset - staged start, first staged position past the slot)
    uint32_t *lstart, *scan_tmp;
    unsigned long long *mark;  // bit per staged position: a non-empty bin starts here
    uint16_t *mbase, *nz;      // marks before every 64-position word; the r-th non-empty bin
    uint32_t *stage;
};
template <int ITEMS>
__device__ __forceinline__ LtLds lt_lds(unsigned char *smem) {
    constexpr int MW = kLtThreads * ITEMS / 64;
    LtLds S;
    S.lhist = reinterpret_cast<uint32_t *>(smem);
    S.tab = reinterpret_cast<uint2 *>(smem);
    S.lstart = S.lhist + 2 * kMaxBins;
    S.scan_tmp = S.lstart + kMaxBins;
    S.mark = reinterpret_cast<unsigned long long *>(S.scan_tmp + 64);
    S.mbase = reinterpret_cast<uint16_t *>(S.mark + MW);
    S.nz = S.mbase + MW;
    S.stage = reinterpret_cast<uint32_t *>(S.nz + kMaxBins);
    return S;
}
static size_t lt_smem(int items, size_t more) {
    const size_t tile = (size_t)kLtThreads * items;
    return sizeof(uint32_t) * (3 * kMaxBins + 64) + (tile / 64) * (8 + 2) + (size_t)kMaxBins * 2 + tile * 4 + more;
}

// the tagged key of (segment, lo): what the spill list and the give-up path need
__device__ inline uint64_t lt_tagged(uint32_t seg, uint32_t lo, int lobits, int k) {
    Key<1> x;
    x.w[0] = ((uint64_t)seg << lobits) | lo;
    return x.w[0] | (__umul64hi(xxh3_64<1>(x), 16ull) << (2 * k));
}

// On entry lhist[b] = records of bin b in this tile (counted, not ranked), lo[i] / bin of item i (two bins per register,
// 0xFFFF: no record).  cur / slot_end: cursor and end of the slot of bin `tid`.  The stored record is lo | rec_or.
template <int ITEMS, class KeyOf>
__device__ __forceinline__ void lt_tail(const LtLds &S, const uint32_t (&lo)[ITEMS], const uint32_t (&bins)[ITEMS / 2],
                                        uint32_t nb, uint32_t *__restrict__ cur, uint64_t slot_end, uint32_t rec_or,
                                        const PartLevel &L, uint32_t *__restrict__ out, KeyOf key_of) {
    constexpr int NT = kLtThreads, MW = NT * ITEMS / 64;
    static_assert(ITEMS % 2 == 0 && ITEMS <= 32 && NT * ITEMS < 65536, "packed bins, one bit per item, 16-bit positions");
    const uint32_t tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const uint32_t c = tid < nb ? S.lhist[tid] : 0u;
    uint32_t incl = c;
    incl = wave_scan_incl(incl);
    const unsigned long long nzb = __ballot(c != 0);
    if (lane == 63) S.scan_tmp[wave] = incl | ((uint32_t)__popcll(nzb) << 16);
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
        atomicOr(&S.mark[ex >> 6], 1ull << (ex & 63u));
    }
    __syncthreads();  // (every thread has read its count: lhist may become the table)
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t bin = (bins[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
        if (bin != 0xFFFFu) {
            const uint32_t pos = atomicAdd(&S.lstart[bin], 1u);  // (lstart ends as the bins' end offsets; nothing reads it again)
            S.stage[pos] = lo[i];
        }
    }
    asm volatile("" : "+v"(greserve));  // awaited by every lane here, not inside the store loop's conditional blocks
    if (c) {
        const int64_t room = (int64_t)slot_end - (int64_t)greserve;
        S.tab[myr] = make_uint2(greserve - ex, (uint32_t)(int32_t)(room < -(int64_t)0x7FFF0000 ? -(int64_t)0x7FFF0000 : room) + ex);
    }
    if (wave == 0) {  // marks before every 64-position word: lane l owns words WPL*l .. WPL*l + WPL-1
        constexpr int WPL = (MW + 63) / 64;
        uint32_t pw[WPL], tot = 0;
#pragma unroll
        for (int j = 0; j < WPL; ++j) {
            const int idx = lane * WPL + j;
            pw[j] = tot;
            tot += idx < MW ? (uint32_t)__popcll(S.mark[idx]) : 0u;
        }
        uint32_t inc2 = tot;
        inc2 = wave_scan_incl(inc2);
        const uint32_t lb = inc2 - tot;
#pragma unroll
        for (int j = 0; j < WPL; ++j) {
            const int idx = lane * WPL + j;
            if (idx < MW) S.mbase[idx] = (uint16_t)(lb + pw[j]);
        }
    }
    __syncthreads();
    const unsigned long long upto = (2ull << lane) - 1ull;  // this lane and the ones below
    // pos = i * NT + tid: the 64 lanes of a wave cover mark word i * (NT / 64) + wave
    const unsigned long long *wmark = S.mark + wave;
    const uint16_t *wmbase = S.mbase + wave;
    uint32_t full = 0;  // items whose slot is full (rare; handled after the stores so that no atomic sits between them)
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t pos = (uint32_t)i * NT + tid;
        if (pos < staged) {
            const uint32_t r = (uint32_t)wmbase[i * (NT / 64)] + (uint32_t)__popcll(wmark[i * (NT / 64)] & upto) - 1u;
            unsigned long long e = reinterpret_cast<const unsigned long long *>(S.tab)[r];
            const uint32_t rec = S.stage[pos];
            asm volatile("" : "+v"(e));  // one 8-byte LDS read (otherwise: the limit, a branch, then the offset)
            if ((int32_t)pos >= (int32_t)(uint32_t)(e >> 32)) full |= 1u << i;
            else out[(uint32_t)e + pos] = rec | rec_or;
        }
    }
    if (full) {
#pragma unroll 1
        for (int i = 0; i < ITEMS; ++i) {
            if ((full >> i) & 1u) {
                const uint32_t pos = (uint32_t)i * NT + tid;
                const uint32_t r = (uint32_t)wmbase[i * (NT / 64)] + (uint32_t)__popcll(wmark[i * (NT / 64)] & upto) - 1u;
                const uint32_t sp = atomicAdd(L.spill_count, 1u);
                if (sp < L.spill_cap) reinterpret_cast<uint64_t *>(L.spill_keys)[sp] = key_of((uint32_t)S.nz[r], S.stage[pos]);
            }
        }
    }
}

// Level 1.  Tile t covers the canonical keys [t * KPT, (t + 1) * KPT) of the view's dense order (DENSE: of a key array,
// the view's overflow records); a lane loads a key once and emits it and its reverse complement.  No tag here.
template <bool DENSE>
__global__ __launch_bounds__(kLtThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_part_view_lt(
    const uint32_t *__restrict__ slots, const uint64_t *__restrict__ off, const uint16_t *__restrict__ seg,
    const uint2 *__restrict__ vdesc, uint32_t stride, int hb, const uint64_t *__restrict__ dense, uint64_t nkeys_all, int k,
    PartLevel L, uint32_t *__restrict__ cursor, uint32_t *__restrict__ out) {
    constexpr int NT = kLtThreads, ITEMS = kLt1Items, KPT = NT * ITEMS / 2, MW = NT * ITEMS / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const LtLds S = lt_lds<ITEMS>(smem);
    uint32_t *toff = S.stage + NT * ITEMS;
    uint16_t *tseg = reinterpret_cast<uint16_t *>(toff + kViewSpan);
    const uint32_t tid = threadIdx.x;
    uint32_t xcc = 0;  // the XCD this workgroup runs on (placement is for speed only: any value gives a correct result)
    if (L.xcd_shift) {
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        xcc &= (1u << L.xcd_shift) - 1u;
    }
    const int lobits = 2 * k - 10;
    const uint32_t lomask = lobits >= 32 ? 0xFFFFFFFFu : (1u << lobits) - 1u;
    const uint64_t c0 = (uint64_t)blockIdx.x * KPT;
    const uint64_t left = nkeys_all - c0;
    const uint32_t nkeys = left < (uint64_t)KPT ? (uint32_t)left : (uint32_t)KPT;
    uint32_t b0 = 0, span = 0;
    bool staged_tab = false;
    if (!DENSE) {
        const uint2 d = vdesc[blockIdx.x];
        b0 = d.x;
        span = d.y - d.x + 1u;
        staged_tab = span <= (uint32_t)kViewSpan;  // uniform
        if (staged_tab && tid < span) {
            toff[tid] = (uint32_t)off[b0 + tid];  // key offsets < 2^32: one pass holds fewer records
            tseg[tid] = seg[b0 + tid];
        }
    }
    S.lhist[tid] = 0;  // NT == kMaxBins
    if (tid < 2 * MW) reinterpret_cast<uint32_t *>(S.mark)[tid] = 0u;
    __syncthreads();

    // all loads first (index clamped into the tile)
    uint64_t x[ITEMS / 2];
    if (DENSE) {
#pragma unroll
        for (int j = 0; j < ITEMS / 2; ++j) {
            const uint32_t cl = (uint32_t)(j * NT) + tid;
            x[j] = dense[c0 + (cl < nkeys ? cl : nkeys - 1u)];
        }
    } else {
        uint32_t w[ITEMS / 2], sg[ITEMS / 2];
#pragma unroll
        for (int j = 0; j < ITEMS / 2; ++j) {
            const uint32_t cl = (uint32_t)(j * NT) + tid;
            const uint32_t c = (uint32_t)c0 + (cl < nkeys ? cl : nkeys - 1u);
            uint32_t b, base;
            if (staged_tab) {
                uint32_t i = 0, hi = span;
                while (hi - i > 1) {
                    const uint32_t mid = (i + hi) >> 1;
                    if (toff[mid] <= c) i = mid;
                    else hi = mid;
                }
                b = b0 + i;
                base = toff[i];
                sg[j] = tseg[i];
            } else {
                b = view_bucket(off, b0, b0 + span, c);
                base = (uint32_t)off[b];
                sg[j] = seg[b];
            }
            w[j] = slots[(size_t)b * stride + (c - base)];
        }
#pragma unroll
        for (int j = 0; j < ITEMS / 2; ++j) x[j] = nw_key(sg[j], w[j], hb);
    }
    uint32_t lo[ITEMS], bins[ITEMS / 2];
#pragma unroll
    for (int j = 0; j < ITEMS / 2; ++j) {
        Key<1> a;
        a.w[0] = x[j];
        const uint64_t r = kmer_rc<1>(a, k).w[0];
        const uint32_t ba = (uint32_t)(x[j] >> lobits), br = (uint32_t)(r >> lobits);  // k-mers < 4^k: bins < 1024
        lo[2 * j] = (uint32_t)x[j] & lomask;
        lo[2 * j + 1] = (uint32_t)r & lomask;
        bins[j] = 0xFFFFFFFFu;
        if ((uint32_t)(j * NT) + tid < nkeys) {
            bins[j] = ba | (br << 16);
            atomicAdd(&S.lhist[ba], 1u);  // count only: the place inside the bin is taken after the scan
            atomicAdd(&S.lhist[br], 1u);
        }
    }
    __syncthreads();
    const uint64_t slot_end = (uint64_t)tid * L.slot_stride + (L.xcd_shift ? (uint64_t)(xcc + 1u) * L.sub_cap : (uint64_t)L.slot_cap);
    lt_tail<ITEMS>(S, lo, bins, (uint32_t)kMaxBins, &cursor[(tid << L.xcd_shift) + xcc], slot_end, 0u, L, out,
                   [&](uint32_t bin, uint32_t rec) { return lt_tagged(bin, rec, lobits, k); });
}

// Level 2: one tile of one segment's sub-slot (k_tile_desc_narrow's descriptors) -> the buckets of that segment.  The
// tag is taken here, once per record.
__global__ __launch_bounds__(kLtThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_part_lt2(
    const uint32_t *__restrict__ in, const uint4 *__restrict__ desc, int k, PartLevel L, uint32_t *__restrict__ cursor,
    uint32_t *__restrict__ out) {
    constexpr int NT = kLtThreads, ITEMS = kLt2Items, MW = NT * ITEMS / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const LtLds S = lt_lds<ITEMS>(smem);
    const uint32_t tid = threadIdx.x;
    const uint4 d = desc[blockIdx.x];  // first record, records, bins of the segment | segment << 16, flat index of bin 0
    const uint32_t begin = d.x, count = d.y, nb = d.z & 0xFFFFu, sgm = d.z >> 16, gbin0 = d.w;
    if (count == 0) return;  // an unused place of the XCD-wise order (k_tile_desc_narrow)
    const int lobits = 2 * k - 10;
    const uint32_t nsub = nb >> 4;
    const uint64_t segbits = (uint64_t)sgm << lobits;
    S.lhist[tid] = 0;  // NT == kMaxBins
    if (tid < 2 * MW) reinterpret_cast<uint32_t *>(S.mark)[tid] = 0u;
    __syncthreads();
    uint32_t lo[ITEMS], bins[ITEMS / 2];
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {  // all loads first (index clamped into the tile)
        const uint32_t local = (uint32_t)i * NT + tid;
        lo[i] = in[begin + (local < count ? local : count - 1u)];
    }
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) asm volatile("" : "+v"(lo[i]));
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        Key<1> x;
        x.w[0] = segbits | lo[i];
        const uint32_t tag = (uint32_t)__umul64hi(xxh3_64<1>(x), 16ull);
        const uint32_t b = tag * nsub + __umulhi(lo[i] << (32 - lobits), nsub);
        const bool valid = (uint32_t)i * NT + tid < count;
        if (valid) atomicAdd(&S.lhist[b], 1u);
        const uint32_t b16 = valid ? b : 0xFFFFu;
        if (i & 1) bins[i >> 1] |= b16 << 16;
        else bins[i >> 1] = b16;
    }
    __syncthreads();
    const uint64_t slot_end = (uint64_t)(gbin0 + tid) * L.slot_stride + L.slot_cap;
    lt_tail<ITEMS>(S, lo, bins, nb, &cursor[gbin0 + tid], slot_end, (uint32_t)segbits, L, out,
                   [&](uint32_t, uint32_t rec) { return lt_tagged(sgm, rec, lobits, k); });
}

// one thread per bucket g = bin tag * nsub + j of segment s: its smallest tagged key, and its place in the order of the
// result, (tag, segment, sub) -- the segments' bin counts are multiples of 16, so a tag owns nbuckets / 16 places
__global__ void k_bucket_base_lt(const uint32_t *__restrict__ seg_nb2, const uint32_t *__restrict__ seg_bin, uint32_t nseg,
                                 uint32_t nbuckets, int lobits, int k, uint64_t *__restrict__ base,
                                 uint32_t *__restrict__ perm) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nbuckets) return;
    uint32_t lo = 0, hi = nseg;  // largest s with seg_bin[s] <= g (every segment has at least one bin)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (seg_bin[mid] <= g) lo = mid;
        else hi = mid;
    }
    const uint32_t nsub = seg_nb2[lo] >> 4, r = g - seg_bin[lo], tag = r / nsub, j = r - tag * nsub;
    const uint64_t q = (((uint64_t)j << lobits) + nsub - 1u) / nsub;
    base[g] = ((uint64_t)tag << (2 * k)) | ((uint64_t)lo << lobits) | q;
    perm[g] = tag * (nbuckets >> 4) + (seg_bin[lo] >> 4) + j;
}

// the slot fills (as SCAN_SLOT_FILL reads them from the cursors) in the order of the result
__global__ void k_lt_fill_perm(const uint32_t *__restrict__ cursor, const uint32_t *__restrict__ perm, uint32_t n,
                               uint32_t stride, uint32_t cap, uint32_t *__restrict__ fill) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const uint32_t c = cursor[g] - g * stride;
    fill[perm[g]] = c < cap ? c : cap;
}

// ... and their exclusive scan back at the buckets
__global__ void k_lt_unperm(const uint64_t *__restrict__ scanned, const uint32_t *__restrict__ perm, uint32_t n,
                            uint32_t *__restrict__ out_off) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < n) out_off[g] = (uint32_t)scanned[perm[g]];
}

// k_view_recanon over the 4-byte level-1 records: the segment comes from the sub-slot, lo from the record
__global__ void k_view_recanon_lt(const uint32_t *__restrict__ in, const uint32_t *__restrict__ seg_off,
                                  const uint32_t *__restrict__ seg_size, int sub_shift, int k, uint64_t *__restrict__ out,
                                  uint64_t cap, uint32_t *__restrict__ count) {
    const uint32_t o = seg_off[blockIdx.x], n = seg_size[blockIdx.x];
    const uint64_t segbits = (uint64_t)(blockIdx.x >> sub_shift) << (2 * k - 10);
    const int lane = threadIdx.x & 63;
    for (uint32_t i0 = 0; i0 < n; i0 += blockDim.x) {  // uniform trip count: the ballot sees whole waves
        const uint32_t i = i0 + threadIdx.x;
        Key<1> x;
        x.w[0] = 0;
        bool keep = false;
        if (i < n) {
            x.w[0] = segbits | in[o + i];
            keep = !kmer_less_nucl<1>(kmer_rc<1>(x, k), x);
        }
        const uint64_t bal = __ballot(keep);
        uint32_t base = 0;
        if (lane == 0 && bal) base = atomicAdd(count, (uint32_t)__popcll(bal));
        base = __shfl(base, 0);
        const uint64_t at = (uint64_t)base + __popcll(bal & ((1ull << lane) - 1ull));
        if (keep && at < cap) out[at] = x.w[0];
    }
}

void BucketView::materialise(bbk_ctx *ctx) {
    if (!live()) return;
    keys.alloc(n() * 8 + 16);
    if (nbuckets) {
        KernelTimer t(ctx, "compact", (double)D * (4 + 8));
        hipLaunchKernelGGL(k_compact_narrow<false>, dim3((unsigned)(((uint64_t)nbuckets * 64 + 255) / 256)), dim3(256), 0,
                           ctx->stream, slots.as<uint32_t>(), nullptr, dcount.as<uint32_t>(), off.as<uint64_t>(), nbuckets,
                           stride, seg.as<uint16_t>(), hb, keys.as<uint64_t>(), nullptr);
        check_launch("compact");
    }
    if (n_extra)
        BBK_HIP(bbk::copy_async(keys.as<uint64_t>() + D, extra.p, n_extra * 8, hipMemcpyDeviceToDevice, ctx->stream));
    stream_wait(ctx);
    release_slots();
}

// ------------------------------------------------------------------------------------------
// host orchestration
// ------------------------------------------------------------------------------------------
// ODD on purpose: in the blocked phases thread t reads records t*ITEMS + i, i.e. lanes are ITEMS*W*2
// dwords apart; with an even ITEMS that stride is a multiple of 16 dwords and a wave hits 2-4 LDS banks
// (16- to 32-way conflicts); with an odd ITEMS the ds_read_b64/b128 of a lane group are conflict-free.
// First pass (k_bucket_dist): 512 threads x 11 records of 8 bytes (CAP 5632), x 7 of 16 bytes (CAP 3584) -- two
// workgroups per CU and few records per lane (the kernel is issue-bound: 256 x 23 was 20 % slower, 512 x 11
// records of 16 bytes, one workgroup per CU, 75 % slower).  Second chance (k_bucket, radix): 512 x 23 / 512 x 11.
template <int W>
struct BktCfg {
#ifndef BBK_BKT_NT
#define BBK_BKT_NT 512
#define BBK_BKT_ITEMS 11
#endif
#ifndef BBK_BKT2_NT
#define BBK_BKT2_NT 512
#define BBK_BKT2_ITEMS 7
#endif
    static constexpr int NT = (W == 1) ? BBK_BKT_NT : BBK_BKT2_NT;
    static constexpr int ITEMS = (W == 1) ? BBK_BKT_ITEMS : (W == 2 ? BBK_BKT2_ITEMS : (W == 3 ? 5 : 3));
    static constexpr uint32_t CAP = NT * ITEMS;
    static constexpr int NT2 = 512;                               // second-chance kernel
    static constexpr int ITEMS2 = (W == 1) ? 23 : (W == 2 ? 11 : (W == 3 ? 7 : 5));
    static constexpr uint32_t CAP2 = NT2 * ITEMS2;
};
// mean bucket = 0.70 CAP: a bucket holds ~100 distinct genomic k-mers x their multiplicity (~40 at 50x
// coverage), so its size varies far more than Poisson on the record count would suggest
constexpr double kBucketFill = 0.70;

static double wall() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// Environment knobs of this file (tests, diagnostics and A/B switches); this is where all of them are read.
struct MsdKnobs {
    // Read once per process: the tests that change them start a fresh process.
    struct PerProcess {
        bool no_dist = getenv("BBK_NO_DIST") != nullptr;  // first bucket pass by the radix kernel, not k_bucket_dist
        // tests: force the LDS table give-up on half-empty slots
        uint32_t hash_max_probes = (uint32_t)env_u64(getenv("BBK_HASH_MAX_PROBES"), kHashMaxProbes);
        uint64_t pass_limit = env_u64(getenv("BBK_PASS_LIMIT"), 0);  // records of one pass (0: from the bucket capacity);
                                                                     // tests force range passes on small inputs
        bool no_narrow = getenv("BBK_NO_NARROW") != nullptr;      // 8-byte records between the levels of stage A
        bool xcd_slots = env_u64(getenv("BBK_XCD_SLOTS"), 1) != 0;  // 0: one level-1 fill front per segment, not per XCD
        bool xcd_tiles = env_u64(getenv("BBK_XCD_TILES"), 1) != 0;  // 0: level-2 workgroups in plain tile order
        bool no_narrow_b = getenv("BBK_NO_NARROW_B") != nullptr;  // 8-byte records after level 1 of stage B
        bool no_late_tag = getenv("BBK_NO_LATE_TAG") != nullptr;  // tagged stage B takes the tag at level 1 (8-byte records there)
        // stage A hands stage B the dense 8-byte array, not its buckets (BucketView)
        bool no_bucket_handoff = getenv("BBK_NO_BUCKET_HANDOFF") != nullptr;
        // k_part_reads_narrow as that many persistent workgroups per CU (0: one workgroup per tile)
        uint32_t nw_wgs_per_cu = (uint32_t)env_u64(getenv("BBK_NW_WGS_PER_CU"), 0);
    };
    const PerProcess &once = *[] {
        static const PerProcess p;
        return &p;
    }();
    // Read on every call: tests change them inside one process.
    bool no_slots = getenv("BBK_NO_SLOTS") != nullptr;    // no histogram-free slot mode (HASH prefix)
    bool no_kslots = getenv("BBK_NO_KSLOTS") != nullptr;  // no key slots (ordering pass of a distinct key array)
    uint64_t slots_min = env_u64(getenv("BBK_SLOTS_MIN"), 1ull << 22);  // records below which neither slot mode runs
    bool verbose = getenv("BBK_VERBOSE") != nullptr;      // "[bbk] msd ..." lines on stderr
    bool no_direct = getenv("BBK_NO_DIRECT") != nullptr;  // no sorted output written by the bucket kernels (nor key slots)
    bool no_level0 = getenv("BBK_NO_LEVEL0") != nullptr;  // key ranges selected from the whole input, no level-0 pass
    bool no_part_kslots = getenv("BBK_NO_PART_KSLOTS") != nullptr;  // no key slots for the ranges level 0 materialised
};

// How one pass (MsdRunner::run) ended
enum class Outcome {
    Declined,        // not an input for this path: the caller uses the LSD path
    Done,
    TooBig,          // more records than one pass takes: run_all splits the input into ranges of the prefix space
    SlotsGaveUp,     // the hash slot mode overflowed: exact histograms
    KeySlotsGaveUp,  // the key slots of the ordering pass did not hold (skewed key space): exact histograms
    NeedDense,       // the input is a BucketView and the pass cannot read it in place: materialise it, run again
};

// Records of a call: reads (rd, see msd_sort_reduce) or a key array (keys[, vals], n)
struct MsdInput {
    const bbk_reads *rd;
    const void *keys;
    const uint32_t *vals;
    uint64_t n;
    bool with_mask;
    BucketView *view = nullptr;  // keys == nullptr: the canonical keys of an expanded input, left in stage A's buckets
};

// f(std::integral_constant<int, OP>) for the runtime reduce op
template <class F>
static void with_op(int op, F &&f) {
    switch (op) {
        case MSD_OP_NONE: f(std::integral_constant<int, MSD_OP_NONE>()); break;
        case MSD_OP_COUNT: f(std::integral_constant<int, MSD_OP_COUNT>()); break;
        case MSD_OP_SUM: f(std::integral_constant<int, MSD_OP_SUM>()); break;
        case MSD_OP_OR: f(std::integral_constant<int, MSD_OP_OR>()); break;
        default: BBK_REQUIRE(false, BBK_ERR_ARG, "bad reduce op");
    }
}

template <int W>
struct MsdRunner {
    static constexpr size_t rec = (size_t)W * 8;
    static constexpr uint32_t kPartTileK = PartCfg<W>::TILE;
    bbk_ctx *ctx;
    unsigned k;
    int dmode;
    int op;  // MSD_OP_*
    uint64_t strip_mask = ~0ull;  // tagged sort: bits of word 0 that survive in the output
    bool assume_distinct = false;  // caller's hint (key arrays, KEYS / REF prefix): duplicates are not expected
    unsigned expand_k = 0;         // key-array input holds CANONICAL k-mers of this length: both strands are generated
    bool expand_tag = false;       // ... with the XXH3 bucket tag above the k-mer (the runner's k is then k + 2)
    MsdKnobs knobs;
    bool slots_ok = !knobs.no_slots;    // histogram-free slot mode allowed (HASH prefix)
    bool kslots_ok = !knobs.no_kslots;  // ... and for the ordering pass of a distinct key array
    bool never_decline = false;  // finish whatever overflows bucket by bucket on the LSD path instead of declining
    bool even_part = false;      // the call sorts a materialised range of an expanded input (run_level0): key slots apply

    int w0bits() const { return (W == 1) ? (int)(2 * k) : 64; }

    template <class K, class... Args>
    void launch(K fn, const char *name, double bytes, uint32_t grid, uint32_t threads, size_t lds, Args... args) {
        launch_timed(ctx, fn, name, bytes, grid, threads, lds, args...);
    }

    // Partition pass over a key array at level 1 (LVL1; also the level-0 and planning passes) or 2: HIST only counts the
    // bins into ghist, otherwise the records go to `cursor`, with their payloads when HAS_VAL
    template <bool HAS_VAL, bool HIST, bool LVL1, bool NOUT = false>
    void launch_part(const char *fam, double bytes, uint32_t ntiles, const Key<W> *in, const uint32_t *vin, TileMap M,
                     PartLevel L, uint32_t *ghist, uint32_t *cursor, Key<W> *out, uint32_t *vout) {
        if (ntiles == 0) return;
        M.ntiles = ntiles;
        M.group = HIST ? 16u : 1u;
        const uint32_t grid = (ntiles + M.group - 1) / M.group;
        launch(k_part<W, HAS_VAL, HIST, LVL1, NOUT>, fam, bytes, grid, PartCfg<W>::THREADS,
               part_smem(W, PartCfg<W>::TILE, HAS_VAL, HIST, LVL1), in, vin, M, L, ghist, cursor, out, vout);
    }

    // scatter of a key array, with the payloads when has_val
    template <bool LVL1>
    void scatter_keys(bool has_val, const char *fam, double bytes, uint32_t ntiles, const Key<W> *in, const uint32_t *vin,
                      TileMap M, PartLevel L, uint32_t *cursor, Key<W> *out, uint32_t *vout) {
        if (has_val) launch_part<true, false, LVL1>(fam, bytes, ntiles, in, vin, M, L, nullptr, cursor, out, vout);
        else launch_part<false, false, LVL1>(fam, bytes, ntiles, in, nullptr, M, L, nullptr, cursor, out, nullptr);
    }

    // level-1 histogram (HIST, no payload) or scatter of reads
    template <bool HIST>
    void launch_part_reads(const char *fam, double bytes, uint32_t ntiles, bool has_val, ReadSrc S, PartLevel L,
                           uint32_t *ghist, uint32_t *cursor, Key<W> *out, uint32_t *vout) {
        if (ntiles == 0) return;
        auto fn = HIST ? k_part_reads<W, false, true> : has_val ? k_part_reads<W, true, false> : k_part_reads<W, false, false>;
        // histogram: ~8 resident-workgroup rounds, each workgroup walks its tiles and flushes once
        const uint32_t grid = HIST ? std::min<uint32_t>(ntiles, 8192u) : ntiles;
        launch(fn, fam, bytes, grid, HIST ? kRdHistThreads : kRdThreads, part_reads_smem(W, has_val, HIST), S, L, ghist,
               cursor, out, has_val ? vout : nullptr);
    }

    // unsorted dedup is enough when a later stage sorts the distinct records (HASH mode)
    bool use_hash_dedup() const { return W == 1 && dmode == MSD_HASH && 2 * k < 64; }
    bool use_hashidx_dedup() const { return W >= 2 && dmode == MSD_HASH; }
    // records a first-pass bucket kernel can hold
    uint32_t bucket_cap() const {
        if (use_hashidx_dedup()) return HashIdxCfg<W>::CAP;
        if (use_hash_dedup()) return (uint32_t)(kHashThreads * kHashItems);
        return BktCfg<W>::CAP;
    }

    // One workgroup per bucket: the LDS hash dedup (HASH prefix, allow_hash), else the sort -- first pass: the one-pass
    // distribution sort; second chance (SECOND): ballot-ranked radix passes, which take any key distribution and twice
    // the records
    template <bool SECOND>
    void bucket_dispatch(uint32_t nblocks, Key<W> *buf, uint32_t *vals, BucketArgs A, double bytes,
                         bool allow_hash = true) {
        with_op(op, [&](auto o) {
            constexpr int OP = decltype(o)::value;
            if (nblocks == 0) return;
            if (allow_hash && use_hashidx_dedup()) {
                if constexpr (W >= 2)
                    launch(k_bucket_hashidx<W, OP>, "k_bucket_hashidx", bytes, nblocks, kHashIdxThreads,
                           bucket_hashidx_smem<W, OP>(), buf, vals, A);
            } else if (allow_hash && use_hash_dedup()) {
                if constexpr (W == 1)
                    launch(k_bucket_hash<OP>, "k_bucket_hash", bytes, nblocks, kHashThreads, bucket_hash_smem<OP>(), buf,
                           vals, A);
            } else {
                constexpr int NT = SECOND ? BktCfg<W>::NT2 : BktCfg<W>::NT;
                constexpr int IT = SECOND ? BktCfg<W>::ITEMS2 : BktCfg<W>::ITEMS;
                const bool dist = !SECOND && !knobs.once.no_dist;
                launch(dist ? k_bucket_dist<W, NT, IT, OP> : k_bucket<W, NT, IT, OP>, dist ? "k_bucket_dist" : "k_bucket",
                       bytes, nblocks, NT, dist ? bucket_dist_smem<W, NT, IT, OP>() : bucket_smem<W, NT, IT, OP>(), buf,
                       vals, A);
            }
        });
    }

    // records two partition levels can take in one pass (bins <= 512 x ~768 of 0.7 CAP records)
    // mean bucket fill the bin plan aims at.  Key arrays deduplicated through the LDS hash table (merge of received
    // shards / pushed batches: multiplicity 1..few) are nearly all distinct: keep the table's load around 0.5 there
    double plan_fill(bool from_reads) const { return (!from_reads && use_hash_dedup()) ? 0.52 : kBucketFill; }
    uint64_t pass_limit(bool from_reads) const {
        if (knobs.once.pass_limit) return knobs.once.pass_limit;
        return (uint64_t)(plan_fill(from_reads) * 512 * 0.75 * kMaxBins * bucket_cap() * 0.98);
    }

    // One range of a range pass: prefixes in [lo, lo + span) (span == 0: everything), est = planning estimate of
    // the records it holds (exact for KEYS / REF ranges, which come from a histogram).
    struct Sel {
        uint32_t lo = 0, span = 0;
        int shl = 0;
        uint32_t mul = 0;
        uint64_t est = 0;
        // shl and mul from span: (d << shl) + mulhi(d << shl, mul) maps [0, span) monotonically onto [0, 2^32)
        void finish() {
            shl = __builtin_clz(span - 1u);
            const uint64_t S = (uint64_t)span << shl;  // in (2^31, 2^32]
            mul = S >= (1ull << 32) ? 0u : (uint32_t)((((1ull << 32) - S) << 32) / S);
        }
    };
    // Where the dense result of an exact-mode pass goes when the caller has already allocated it (range passes
    // write one after the other into the final array: no concatenation copy of a 100 GB result).
    struct Dst {
        void *keys = nullptr;
        uint32_t *vals = nullptr;
    };

    // What a pass decides before its first launch
    struct Plan {
        uint64_t N;     // records of the pass (a range: the planning estimate of its share)
        uint64_t Ntot;  // instance space of the level-1 tiles
        double target;  // bucket size the bin plan aims at
        uint32_t nb1 = 1;  // level-1 bins, 2^b1
        int b1 = 0;
        bool too_deep;  // would need a third level: declined
        int nw_hb;      // key bits above the low word (8-byte keys)
        bool narrow, hslots, kslots, slots;
        bool late_tag = false;  // stage B from a BucketView, k <= 21: 4-byte records from level 1, tag taken at level 2
        uint32_t rd_tile, ntiles1, ntiles1h;  // chunks of a read tile; level-1 tiles (scatter, reads histogram)
        int xs;         // log2 of the level-1 sub-slots per segment (one per XCD)
        uint32_t nsub, sub_cap, seg_cap, cap2, stride2, spill_cap;
        size_t rec_ab;  // record width between the levels
    };

    // The bin plan and the mode of a pass of N records (n_chunks read chunks).  No HIP calls.
    Plan plan(uint64_t N, uint64_t n_chunks, bool from_reads, bool has_val, const Sel &sel, bool has_dst,
              bool from_view = false) const {
        Plan P;
        const bool ranged = sel.span != 0;
        P.Ntot = N;
        P.N = N = ranged ? sel.est : N;
        // record offsets inside one pass are 32-bit; the input of a call may hold more (range passes walk the
        // 64-bit instance space once per range)
        BBK_REQUIRE(N < (1ull << 32) - kPartTileK, BBK_ERR_ARG,
                    "batch holds %llu records%s; one pass is limited to 2^32-1 (split the input)",
                    (unsigned long long)N, ranged ? " in one range of the prefix space" : "");

        // ---- bin plan: nb1 (power of two) level-1 bins; level-2 bin counts are chosen per segment later
        const double fill = plan_fill(from_reads);
        P.target = fill * bucket_cap();
        const double want = std::max(1.0, std::ceil((double)N / P.target));
        while (P.nb1 < 512 && (double)P.nb1 * P.nb1 < want) {
            P.nb1 <<= 1;
            ++P.b1;
        }
        // REF prefix: the 4 XXH3 bucket bits must be consumed before the buckets (a bucket is sorted by key alone
        // and may not hold records of two XXH3 buckets) -- by the range selection (a range inside one XXH3 bucket
        // shifts them all out: shl >= 4; run_all only makes wider ranges as aligned groups of 2^j whole buckets,
        // shl = 4 - j) and, for what is left, by level 1
        const int ref_bits = dmode == MSD_REF ? std::max(0, 4 - (ranged ? sel.shl : 0)) : 0;
        if (P.b1 < ref_bits) {
            P.b1 = ref_bits;
            P.nb1 = 1u << P.b1;
        }
        const bool u32_slots = (double)N / fill * 1.1 + (double)N < 4.2e9;  // slot offsets stay 32-bit
        // narrow stage A: reads, 8-byte keys of 33..42 bits, slot mode, one pass -> 4-byte records between the levels
        // (1024 level-1 segments whatever the size: the segment carries the key bits the record drops)
        P.nw_hb = (int)(2 * k) - 32;
        P.narrow = W == 1 && from_reads && !ranged && !has_dst && P.nw_hb >= 1 && P.nw_hb <= 10 && slots_ok &&
                   dmode == MSD_HASH && use_hash_dedup() && N >= knobs.slots_min && !knobs.once.no_narrow && u32_slots &&
                   (double)N / kNwBins1 / P.target < 0.75 * kMaxBins;
        if (P.narrow) {
            P.b1 = 10;
            P.nb1 = kNwBins1;
        }
        P.too_deep = want / P.nb1 > 0.75 * kMaxBins;
        if (P.too_deep) return P;

        // level-1 tiles cover the whole instance space; a range pass keeps its share of every tile.  Reads:
        // a tile is `threads` chunks, so the histogram (512 threads) and the scatter (1024) have their own tables
        P.rd_tile = P.narrow ? (uint32_t)(has_val ? NwCfg<true>::CHUNKS : NwCfg<false>::CHUNKS) : (uint32_t)kRdThreads;
        P.ntiles1 = from_reads ? (uint32_t)((n_chunks + P.rd_tile - 1) / P.rd_tile)
                               : (uint32_t)((P.Ntot + kPartTileK - 1) / kPartTileK);
        P.ntiles1h = (uint32_t)((n_chunks + kRdHistThreads - 1) / kRdHistThreads);

        // ---- slot mode (HASH prefix + LDS hash dedup): no histogram passes.  The hash spreads the records evenly,
        // so every level-1 segment gets a fixed slot of the mean size + 1 % and every bucket a slot of the dedup
        // kernel's capacity; the scatter kernels reserve space with the same per-(tile, bin) atomics, records
        // that do not fit their slot go to a spill list, and whatever overflowed (spill list + the contents of the
        // overflowing segments / buckets, i.e. every record of the affected keys) is reprocessed by the exact path
        // on a key array.  Heavy repeats therefore cost a second pass over a small part of the data.
        P.hslots = slots_ok && !has_dst && dmode == MSD_HASH && (use_hash_dedup() || use_hashidx_dedup()) && P.nb1 > 1 &&
                   N >= knobs.slots_min && u32_slots;
        // Stage B (ordering a distinct key array, KEYS / REF prefix, sorted result written directly): the same slots
        // instead of the two histogram passes.  The prefix is the key itself, so the spread is only as even as the
        // data: ANY record that misses its slot, any bucket the sort kernel turns down, any duplicate sends the call
        // back to the exact path (the slots cannot be patched up in key order the way the hash slots can).
        // (only for EXPANDED input: both strands of a set spread evenly over the key space; a canonical set does not --
        // its last base is A four times as often as T -- and 119 of 512 segments overflowed their slots in every
        // extension-index build: 3.8 ms of a 30 ms build spent on an attempt that never holds)
        // (even_part: a materialised range of an expanded input -- run_level0 -- is as evenly spread, holds exactly
        // sel.est records and writes into its place of the final array)
        P.kslots = kslots_ok && slots_ok && (even_part || (!has_dst && !ranged && expand_k != 0)) && !from_reads &&
                   assume_distinct && (dmode == MSD_KEYS || dmode == MSD_REF) && P.nb1 > 1 && N >= knobs.slots_min &&
                   !knobs.no_direct && u32_slots;
        P.slots = P.hslots || P.kslots;
        BBK_REQUIRE(!P.narrow || P.slots, BBK_ERR_INTERNAL, "narrow records need the slot mode");
        // Late tag (see k_part_view_lt): everything narrow stage B asks for, a tagged expansion read from stage A's
        // buckets, and 2k - 10 <= 32.  Narrow stage B's span check (no bucket of the 512-segment plan wider than 2^32
        // keys) can only be taken on level 1's fills; here it is taken on the even fills the key slots are sized for, so
        // that a call too small for 4-byte records keeps the 8-byte route as a whole.
        P.late_tag = false;
        if (W == 1 && from_view && P.kslots && expand_tag && !even_part && !ranged && !has_dst && !has_val &&
            op == MSD_OP_NONE && dmode == MSD_KEYS && !knobs.once.no_narrow_b && !knobs.once.no_late_tag && expand_k >= 17 &&
            2 * expand_k <= 42) {
            const double nb2 = std::min<double>(kMaxBins, std::max(1.0, std::ceil((double)N / P.nb1 / P.target)));
            const uint64_t Q = 1ull << (32 - P.b1), q = (Q + (uint64_t)nb2 - 1) / (uint64_t)nb2;
            const int wb = w0bits();
            P.late_tag = (wb > 32 ? q << (wb - 32) : q >> (32 - wb)) <= (1ull << 32);
        }
        if (P.late_tag) {
            P.b1 = 10;
            P.nb1 = kMaxBins;
        }
        // narrow level 1: one sub-slot (and cursor) per XCD inside every segment slot (PartLevel::xcd_shift); the XCDs do
        // not take exactly equal shares of the tiles, so the sub-slots get 6 % + 2048 records of slack.
        // A 128-byte line of a segment that workgroups on DIFFERENT XCDs fill (their ~60-byte runs are adjacent) is
        // what makes this kernel's store pattern slow: tools/probes/reserve_scatter_probe.hip replays the pattern
        // without any arithmetic -- 3.8 ms with one fill front per segment, 2.1 ms with one per (segment, XCD), 6.4 ms
        // when adjacent runs ALWAYS come from different XCDs.  The kernel itself: 3.64 -> 2.94 ms (same call, round 3;
        // in round 2 its arithmetic took as long as the stores and hid the gain: 3.96 -> 3.79).
        P.xs = (P.slots && knobs.once.xcd_slots && ctx->num_xcds == 8) ? 3 : 0;
        P.nsub = P.nb1 << P.xs;  // level-1 cursors = level-2 input segments
        P.sub_cap = P.xs ? ((uint32_t)((double)N / P.nsub * 1.06) + 2048u) | 1u : 0u;
        P.seg_cap = !P.slots ? 0u
                    : P.xs   ? P.sub_cap << P.xs
                             : ((uint32_t)((double)N / P.nb1 * (P.kslots ? 1.06 : 1.01)) + 8192u) | 1u;
        P.cap2 = P.narrow ? (uint32_t)(kNwHashThreads * kNwHashItems) : bucket_cap();
        // bucket slots 256 B further apart than their capacity: with a power-of-two-ish stride every bucket's
        // fill front sits in the same HBM channel (level-2 scatter measured 10 % slower)
        P.rec_ab = (P.narrow || P.late_tag) ? 4 : rec;
        P.stride2 = P.cap2 + (uint32_t)(256 / P.rec_ab);
        P.spill_cap = P.slots ? (uint32_t)(N / 8 + 65536) : 0u;
        return P;
    }

    // One pass: the buffers and host arrays that cross its phases.  The host arrays are also the sources of
    // asynchronous copies and must live until a later synchronisation, so they live as long as the pass.
    struct Pass {
        static constexpr uint32_t kFlagCap = 65536;  // flagged buckets the first pass can list
        MsdRunner &R;
        bbk_ctx *ctx;
        const MsdInput &in;
        MsdOutput &out;
        const Sel sel;
        const Dst dst;
        const bool from_reads, has_val, ranged, has_dst, out_vals, need_vbuf, verbose;
        Plan P{};
        uint64_t N = 0, n_chunks = 0;  // records of the pass (a range: exact once level 1 has counted them); read chunks
        DevBuf coff, tile_read, tiles_h;
        // The pass's small device counters in one block, cleared by one fill when the pass starts and read back by one
        // copy (fetch_flags).  u32 words: [0..3] spill counters ([0] spilled records [1] unused [2] buckets left to the
        // caller), [4] reads not in word order, [8] duplicate seen by the direct pass, [12] flagged buckets (exact
        // mode), [16..31] debug counters (BBK_VERBOSE), [32..35] two u64 scan totals
        enum { kCtlSpill = 0, kCtlUnordered = 4, kCtlDup = 8, kCtlFlagN = 12, kCtlDbg = 16, kCtlTotal = 32, kCtlWords = 40 };
        DevBuf ctl;
        uint32_t h_ctl[kCtlWords] = {};
        uint32_t *ctl_at(int w) const { return ctl.as<uint32_t>() + w; }
        uint64_t *ctl_total() const { return reinterpret_cast<uint64_t *>(ctl_at(kCtlTotal)); }
        uint64_t h_total() const {  // the scan total fetch_flags brought back
            uint64_t t;
            memcpy(&t, h_ctl + kCtlTotal, 8);
            return t;
        }
        ReadSrc S{}, Sh{};
        TileMap M1{}, M2{};
        PartLevel L1{}, L2{};
        DevBuf spill_k, spill_v;
        // level 1 (off1 / tstart / hsub are per level-1 CURSOR: per segment, or per (segment, XCD) sub-slot on the
        // narrow path)
        DevBuf hist1, cur1, bufA, valA;
        uint32_t n32 = 0;
        std::vector<uint32_t> h1, off1, tstart, snb2, sbin, hsub, fill1;
        std::vector<uint32_t> over_seg;  // slot mode: segments that ran over (reprocessed as a whole)
        // level 2
        uint32_t nbuckets = 0, ntiles2 = 0, nwg2 = 0;
        bool narrow_b = false;
        // the layout arrays: one pinned host block (stage; its head is the source of the level-1 cursors), one copy, one
        // device block
        uint32_t *stage = nullptr;
        DevBuf layout_d;
        uint32_t *seg_tile = nullptr, *seg_off = nullptr, *seg_nb2 = nullptr, *seg_bin = nullptr, *seg_size = nullptr,
                 *xstart_d = nullptr;
        DevBuf desc2, desc2h, hist2, boff, bufB, valB;
        std::vector<uint32_t> xstart;
        // buckets
        DevBuf dcount, slot_off, bseg, bbase, flag_ids;  // bbase: narrow stage B, smallest key of a bucket
        DevBuf bperm, pfill;  // late tag: place of every bucket in the order of the result; the fills in that order
        // scans whose totals come back with the flags (fetch_flags): c64 = key slots, exclusive scan of the slot fills;
        // d64 = hash slots, exclusive scan of the distinct counts.  scan_keep: their scratch, alive until the pass ends
        DevBuf c64, d64;
        bool d64_scanned = false;
        std::vector<DevBuf> scan_keep;
        BucketArgs A{};
        bool direct = false;
        uint32_t ctr[4] = {0, 0, 0, 0};  // spilled, direct, flagged, duplicates seen by the direct pass
        std::vector<uint32_t> flagged, hd, hb;  // exact mode with flagged buckets (or verbose): per-bucket counts / offsets
        std::vector<uint32_t> big;
        uint32_t hbo[2] = {0, 0};
        MsdOutput extra;  // slot mode: distinct records of everything that overflowed
        uint64_t novf = 0;

        Pass(MsdRunner &r, const MsdInput &i, MsdOutput &o, const Sel &s, Dst d)
            : R(r), ctx(r.ctx), in(i), out(o), sel(s), dst(d), from_reads(i.rd != nullptr),
              has_val(i.with_mask || i.vals != nullptr), ranged(s.span != 0), has_dst(d.keys != nullptr),
              out_vals(r.op != MSD_OP_NONE), need_vbuf(has_val || out_vals), verbose(r.knobs.verbose) {}

        double rec_bytes(uint64_t n) const { return (double)n * (rec + (has_val ? 4 : 0)); }
        uint32_t *vals_or_null(DevBuf &b) const { return has_val ? b.as<uint32_t>() : nullptr; }

        // n_records: the whole input may be split into ranges; TooBig then gives its record count
        Outcome run(uint64_t *n_records = nullptr) {
            ctl.alloc(kCtlWords * 4);
            BBK_HIP(hipMemsetAsync(ctl.p, 0, kCtlWords * 4, ctx->stream));
            count_instances();
            out.instances = N;
            out.n = 0;
            if (N == 0) return empty();
            if (!ranged && n_records && N > R.pass_limit(from_reads)) {
                *n_records = N;
                return Outcome::TooBig;
            }
            P = R.plan(N, n_chunks, from_reads, has_val, sel, has_dst, in.view != nullptr);
            N = P.N;
            if (in.view && !view_level1()) return Outcome::NeedDense;
            if (P.too_deep) {  // leave to the LSD path
                if (verbose) fprintf(stderr, "[bbk] msd declines: N=%llu needs more than two levels\n", (unsigned long long)N);
                return Outcome::Declined;
            }
            level1_tiles();
            if (auto r = level1()) return *r;
            level2_layout();
            level2_scatter();
            if (auto r = first_pass()) return *r;
            if (auto r = overflow()) return *r;
            compact();
            return Outcome::Done;
        }

        // the key-slot level 1 reads a BucketView in place (every other pass takes the dense array)
        bool view_level1() const {
            return W == 1 && !P.too_deep && P.kslots && R.expand_k && !ranged && !has_dst && !R.even_part && !has_val;
        }

        Outcome empty() {
            if (!has_dst) {
                out.keys.alloc(16);
                out.vals.alloc(16);
            }
            return Outcome::Done;
        }

        // ---- instance space (reads: k-mers for the sizes, chunks for the level-1 tiles)
        void count_instances() {
            N = (R.expand_k && !from_reads) ? 2 * in.n : in.n;
            if (!from_reads) return;
            const bbk_reads *rd = in.rd;
            BBK_REQUIRE(R.dmode == MSD_HASH, BBK_ERR_INTERNAL, "reads are partitioned by hash prefix only");
            DevBuf nk((rd->n + 1) * sizeof(uint64_t));
            coff.alloc((rd->n + 1) * sizeof(uint64_t));
            if (rd->n) {
                hipLaunchKernelGGL(k_kmers_per_read2, bbk::grid_blocks((rd->n + 255) / 256), dim3(256), 0, ctx->stream,
                                   rd->d_len, rd->d_woff, rd->n, R.k, (uint32_t)RdCfg<W>::CH, nk.as<uint64_t>(),
                                   coff.as<uint64_t>(), ctl_at(kCtlUnordered));
                check_launch("k_kmers_per_read2");
            }
            // both scans in the same launches, both totals in one wait; coff[n] = n_chunks is written by the scan
            uint64_t tot[2] = {0, 0};
            exclusive_scan2_u64(ctx, nk.as<uint64_t>(), nk.as<uint64_t>(), coff.as<uint64_t>(), coff.as<uint64_t>(), rd->n,
                                tot);
            N = tot[0];
            n_chunks = tot[1];
        }

        // ---- level-1 tiles (reads) and the slot layout
        void level1_tiles() {
            L1 = PartLevel{1, P.b1, P.nb1, R.dmode, R.w0bits(), nullptr, nullptr, sel.lo, sel.span, sel.shl, sel.mul};
            if (from_reads) {
                const bbk_reads *rd = in.rd;
                tile_read.alloc(((size_t)P.ntiles1 + 1) * sizeof(RdTile));
                tiles_h.alloc(((size_t)P.ntiles1h + 1) * sizeof(RdTile));
                if (P.ntiles1) {
                    hipLaunchKernelGGL(k_tile_reads, dim3(((uint64_t)P.ntiles1 + P.ntiles1h + 255) / 256), dim3(256), 0,
                                       ctx->stream, coff.as<uint64_t>(), rd->d_woff, rd->d_len, rd->n, (uint64_t)P.ntiles1,
                                       P.rd_tile, tile_read.as<RdTile>(), (uint64_t)P.ntiles1h, (uint32_t)kRdHistThreads,
                                       tiles_h.as<RdTile>(), (uint32_t)RdCfg<W>::CH, R.k, (uint32_t)kRdSlots,
                                       (uint32_t)kRdWords, ctl_at(kCtlUnordered));
                    check_launch("k_tile_reads");
                }
                S = ReadSrc{rd->d_words, rd->d_woff, rd->d_len, coff.as<uint64_t>(), tile_read.as<RdTile>(), rd->n,
                            n_chunks, (int)R.k};
                Sh = S;
                Sh.tiles = tiles_h.as<RdTile>();
            }
            M1 = TileMap{nullptr, nullptr, nullptr, 1, P.Ntot, 0, 1, nullptr, (int)R.expand_k, R.expand_tag ? 1 : 0};
            if (P.slots) {
                spill_k.alloc((size_t)P.spill_cap * rec);
                if (has_val) spill_v.alloc((size_t)P.spill_cap * 4);
                use_slots(L1, P.seg_cap, P.seg_cap);
                L1.xcd_shift = P.xs;
                L1.sub_cap = P.sub_cap;
            }
        }

        // slot mode: the bins of level L own slots of `cap` records, `stride` apart; what misses its slot is spilled
        void use_slots(PartLevel &L, uint32_t cap, uint32_t stride) {
            L.slot_cap = cap;
            L.slot_stride = stride;
            L.spill_keys = spill_k.p;
            L.spill_vals = spill_v.as<uint32_t>();
            L.spill_count = ctl_at(kCtlSpill);
            L.spill_cap = P.spill_cap;
            L.narrow_hb = P.narrow ? P.nw_hb : 0;
        }

        // ---- level 1: histogram (exact mode) or slot offsets, scatter
        std::optional<Outcome> level1() {
            const uint32_t nb1 = P.nb1, nsub = P.nsub;
            hist1.alloc((size_t)nb1 * 4 + 16);
            cur1.alloc((size_t)nsub * 4 + 16);
            h1.resize(nb1);
            off1.resize(nsub + 1);
            tstart.resize(nsub + 1);
            snb2.resize(nb1);
            sbin.resize(nb1 + 1);
            hsub.resize(nsub);
            fill1.resize(nsub);
            if (!P.slots) {
                BBK_HIP(hipMemsetAsync(hist1.p, 0, (size_t)nb1 * 4 + 16, ctx->stream));
                if (nb1 > 1 || ranged) {
                    const double hb = from_reads ? (double)in.rd->n_words * 8 : (double)N * rec;
                    if (from_reads)
                        R.template launch_part_reads<true>("k_part_reads_hist", hb, P.ntiles1h, false, Sh, L1,
                                                           hist1.as<uint32_t>(), nullptr, nullptr, nullptr);
                    else
                        R.template launch_part<false, true, true>("k_part_hist1", hb, P.ntiles1, (const Key<W> *)in.keys, nullptr,
                                                            M1, L1, hist1.as<uint32_t>(), nullptr, nullptr, nullptr);
                } else {
                    n32 = (uint32_t)N;
                    BBK_HIP(hipMemcpyAsync(hist1.p, &n32, 4, hipMemcpyHostToDevice, ctx->stream));
                }
                BBK_HIP(hipMemcpyAsync(h1.data(), hist1.p, (size_t)nb1 * 4, hipMemcpyDeviceToHost, ctx->stream));
                stream_wait(ctx);
                off1[0] = 0;
                for (uint32_t b = 0; b < nb1; ++b) off1[b + 1] = off1[b] + h1[b];
                if (ranged) {
                    N = off1[nb1];  // the records of this range
                    out.instances = N;
                }
                BBK_REQUIRE(off1[nb1] == (uint32_t)N, BBK_ERR_INTERNAL, "level-1 histogram does not add up (%u vs %llu)",
                            off1[nb1], (unsigned long long)N);
                if (N == 0) return empty();
            } else {
                BBK_REQUIRE((uint64_t)nb1 * P.seg_cap + N < (1ull << 32), BBK_ERR_INTERNAL,
                            "slot layout exceeds 32-bit offsets");
                for (uint32_t s2 = 0; s2 <= nsub; ++s2)
                    off1[s2] = P.xs ? (s2 >> P.xs) * P.seg_cap + (s2 & ((1u << P.xs) - 1u)) * P.sub_cap : s2 * P.seg_cap;
            }
            // (the pinned block: sized here for the cursors AND the level-2 layout, so that it is never replaced while the
            // cursors' copy is in flight; both parts are written after a wait that followed the last copy out of them)
            stage = (uint32_t *)plan_staging(ctx, (layout_words(nullptr) + pad4(nsub)) * 4);
            memcpy(stage, off1.data(), (size_t)nsub * 4);
            BBK_HIP(hipMemcpyAsync(cur1.p, stage, (size_t)nsub * 4, hipMemcpyHostToDevice, ctx->stream));

            const uint64_t nA = P.slots ? (uint64_t)nb1 * P.seg_cap : N;  // records bufA holds (slot layout has gaps)
            bufA.alloc(nA * P.rec_ab);
            if (has_val) valA.alloc(nA * 4);
            if (P.narrow) {
                if constexpr (W == 1) {
                    const double pbn = (double)in.rd->n_words * 8 + (double)N * (4 + (has_val ? 4 : 0));
                    // One tile per workgroup.  The kernel can also run as persistent workgroups that walk every grid-th
                    // tile and load the next tile's tables during the stores of the current one
                    // (BBK_NW_WGS_PER_CU=2): measured slower in the same call, 3.38-3.46 ms against 2.94 -- the wait
                    // for the loaded tables at the top of the loop is also a wait for the tile's stores, and the
                    // hardware dispatcher balances the tiles better than a static stride.
                    const uint32_t per_cu = R.knobs.once.nw_wgs_per_cu;
                    const uint32_t grid = per_cu ? std::min<uint32_t>(P.ntiles1, (uint32_t)ctx->num_cus * per_cu) : P.ntiles1;
                    R.launch(has_val ? k_part_reads_narrow<true> : k_part_reads_narrow<false>, "k_part_reads_narrow", pbn,
                             grid, kNwThreads, part_reads_narrow_smem(has_val), S, L1, P.ntiles1, S.tiles,
                             cur1.as<uint32_t>(), bufA.as<uint32_t>(), vals_or_null(valA));
                }
            } else {
                const double pb = (from_reads ? (double)in.rd->n_words * 8 : rec_bytes(N)) + rec_bytes(N);
                if (from_reads)
                    R.template launch_part_reads<false>("k_part_reads", pb, P.ntiles1, has_val, S, L1, nullptr,
                                                        cur1.as<uint32_t>(), bufA.as<Key<W>>(), valA.as<uint32_t>());
                else if (in.view)
                    level1_from_view();
                else
                    R.template scatter_keys<true>(has_val, "k_part_l1", pb, P.ntiles1, (const Key<W> *)in.keys, in.vals, M1, L1,
                                   cur1.as<uint32_t>(), bufA.as<Key<W>>(), valA.as<uint32_t>());
            }
            if (!P.slots) return std::nullopt;
            auto r = slot_fills();
            if (in.view && !r) {  // level 1 holds: the buckets are no longer needed (a later give-up: rebuild_view)
                in.view->release_slots();
                if (verbose) fprintf(stderr, "[bbk] msd key slots: level 1 read stage A's buckets (%llu + %llu keys)\n",
                                     (unsigned long long)in.view->D, (unsigned long long)in.view->n_extra);
            }
            return r;
        }

        // level 1 of the key slots over a BucketView: the buckets' keys, then the overflow path's (dense) into the same
        // slots and cursors
        void level1_from_view() {
            if constexpr (W == 1) {
                BucketView &v = *in.view;
                if (P.late_tag) {
                    level1_late_tag(v);
                    return;
                }
                const uint32_t half = kPartTileK / 2;
                const uint32_t nt = (uint32_t)((v.D + half - 1) / half);
                if (nt) {
                    DevBuf vdesc((size_t)nt * sizeof(uint2) + 16);
                    hipLaunchKernelGGL(k_view_tile_desc, dim3((nt + 255) / 256), dim3(256), 0, ctx->stream,
                                       v.off.as<uint64_t>(), v.nbuckets, v.D, half, nt, vdesc.as<uint2>());
                    check_launch("k_view_tile_desc");
                    TileMap Mv = M1;
                    Mv.n = 2 * v.D;
                    Mv.ntiles = nt;
                    R.launch(R.expand_tag ? k_part_view<true> : k_part_view<false>, "k_part_view",
                             (double)v.D * 4 + 2.0 * (double)v.D * rec, nt, PartCfg<1>::THREADS, part_view_smem(),
                             v.slots.as<uint32_t>(), v.off.as<uint64_t>(), v.seg.as<uint16_t>(), vdesc.as<uint2>(),
                             v.stride, v.hb, Mv, L1, cur1.as<uint32_t>(), bufA.as<Key<1>>());
                }
                if (v.n_extra) {
                    TileMap Me = M1;
                    Me.n = 2 * v.n_extra;
                    const uint32_t nte = (uint32_t)((Me.n + kPartTileK - 1) / kPartTileK);
                    R.template scatter_keys<true>(false, "k_part_l1", rec_bytes(v.n_extra) + rec_bytes(Me.n), nte,
                                                  v.extra.as<Key<W>>(), nullptr, Me, L1, cur1.as<uint32_t>(),
                                                  bufA.as<Key<W>>(), nullptr);
                }
            }
        }

        // level 1 with the tag taken late: 4-byte records into 1024 key-prefix segments (k_part_view_lt), from the
        // buckets and from the overflow path's dense keys
        void level1_late_tag(BucketView &v) {
            if constexpr (W == 1) {
                constexpr uint32_t kpt = (uint32_t)kLtThreads * kLt1Items / 2;
                const size_t lds = lt_smem(kLt1Items, (size_t)kViewSpan * (4 + 2));
                const uint32_t nt = (uint32_t)((v.D + kpt - 1) / kpt);
                ctx->add_stat("stat_late_tag", (double)N);
                if (nt) {
                    DevBuf vdesc((size_t)nt * sizeof(uint2) + 16);
                    hipLaunchKernelGGL(k_view_tile_desc, dim3((nt + 255) / 256), dim3(256), 0, ctx->stream,
                                       v.off.as<uint64_t>(), v.nbuckets, v.D, kpt, nt, vdesc.as<uint2>());
                    check_launch("k_view_tile_desc");
                    R.launch(k_part_view_lt<false>, "k_part_view", (double)v.D * 4 + 2.0 * (double)v.D * 4, nt, kLtThreads, lds,
                             v.slots.as<uint32_t>(), v.off.as<uint64_t>(), v.seg.as<uint16_t>(), vdesc.as<uint2>(), v.stride,
                             v.hb, (const uint64_t *)nullptr, v.D, (int)R.expand_k, L1, cur1.as<uint32_t>(),
                             bufA.as<uint32_t>());
                }
                if (v.n_extra) {
                    const uint32_t nte = (uint32_t)((v.n_extra + kpt - 1) / kpt);
                    R.launch(k_part_view_lt<true>, "k_part_l1", (double)v.n_extra * 8 + 2.0 * (double)v.n_extra * 4, nte,
                             kLtThreads, lds, (const uint32_t *)nullptr, (const uint64_t *)nullptr, (const uint16_t *)nullptr,
                             (const uint2 *)nullptr, 0u, 0, v.extra.as<uint64_t>(), v.n_extra, (int)R.expand_k, L1,
                             cur1.as<uint32_t>(), bufA.as<uint32_t>());
                }
            }
        }

        // a key-slot give-up after level 1 released the view's buckets: the canonical keys again, from level 1's records
        Outcome give_up_key_slots() {
            if constexpr (W == 1) {
                if (in.view && !in.view->live() && !in.view->keys.p) {
                    BucketView &v = *in.view;
                    const uint64_t n = v.n();
                    v.keys.alloc(n * rec + 16);
                    DevBuf cnt(16);
                    BBK_HIP(hipMemsetAsync(cnt.p, 0, 16, ctx->stream));
                    if (P.late_tag) {
                        ctx->add_stat("stat_late_tag_recanon", (double)n);
                        hipLaunchKernelGGL(k_view_recanon_lt, dim3(P.nsub), dim3(256), 0, ctx->stream, bufA.as<uint32_t>(),
                                           seg_off, seg_size, P.xs, (int)R.expand_k, v.keys.as<uint64_t>(), n,
                                           cnt.as<uint32_t>());
                    } else {
                        hipLaunchKernelGGL(k_view_recanon, dim3(P.nsub), dim3(256), 0, ctx->stream, bufA.as<uint64_t>(),
                                           seg_off, seg_size, (int)R.expand_k, v.keys.as<uint64_t>(), n,
                                           cnt.as<uint32_t>());
                    }
                    check_launch("k_view_recanon");
                    uint32_t got = 0;
                    BBK_HIP(hipMemcpyAsync(&got, cnt.p, 4, hipMemcpyDeviceToHost, ctx->stream));
                    stream_wait(ctx);
                    BBK_REQUIRE(got == n, BBK_ERR_INTERNAL, "canonical keys rebuilt from level 1: %u of %llu", got,
                                (unsigned long long)n);
                }
            }
            return Outcome::KeySlotsGaveUp;
        }

        // slot mode: the level-1 cursors tell what every segment received
        std::optional<Outcome> slot_fills() {
            const uint32_t nsub = P.nsub, xs = P.xs;
            std::vector<uint32_t> c1(nsub);
            BBK_HIP(hipMemcpyAsync(c1.data(), cur1.p, (size_t)nsub * 4, hipMemcpyDeviceToHost, ctx->stream));
            stream_wait(ctx);
            uint64_t got = 0;
            const uint32_t cap1 = xs ? P.sub_cap : P.seg_cap;
            for (uint32_t b = 0; b < P.nb1; ++b) {
                bool over = false;
                uint32_t tot = 0;
                for (uint32_t s2 = b << xs; s2 < (b + 1) << xs; ++s2) {
                    const uint32_t reserved = c1[s2] - off1[s2];
                    got += reserved;
                    over = over || reserved > cap1;
                    fill1[s2] = std::min(reserved, cap1);  // what the slot really holds
                    tot += fill1[s2];
                }
                if (over) over_seg.push_back(b);
                // an overflowing segment is kept out of level 2 as a whole: every record of a key must meet in one bucket
                h1[b] = over ? 0u : tot;
                for (uint32_t s2 = b << xs; s2 < (b + 1) << xs; ++s2) hsub[s2] = over ? 0u : fill1[s2];
            }
            if (got > P.Ntot) {  // cannot be: every instance reserves one place.  Say what was read before failing
                std::vector<uint32_t> c2(nsub);
                BBK_HIP(hipMemcpyAsync(c2.data(), cur1.p, (size_t)nsub * 4, hipMemcpyDeviceToHost, ctx->stream));
                stream_wait(ctx);
                uint32_t shown = 0, differ = 0;
                for (uint32_t b = 0; b < nsub; ++b) differ += c1[b] != c2[b];
                for (uint32_t b = 0; b < nsub && shown < 8; ++b)
                    if (c1[b] - off1[b] > 2 * P.seg_cap) {
                        fprintf(stderr, "[bbk] level-1 cursor %u: start %u now %u (second read %u), slot capacity %u\n", b,
                                off1[b], c1[b], c2[b], P.seg_cap);
                        ++shown;
                    }
                fprintf(stderr, "[bbk] level-1 cursors: %u of %u differ between two reads; cur1 at %p\n", differ, nsub, cur1.p);
                BBK_REQUIRE(false, BBK_ERR_INTERNAL, "level-1 reservations exceed the instance space (%llu vs %llu)",
                            (unsigned long long)got, (unsigned long long)P.Ntot);
            }
            if (ranged) {
                N = got;
                out.instances = N;
            }
            BBK_REQUIRE(got == N, BBK_ERR_INTERNAL, "level-1 reservations do not add up (%llu vs %llu)",
                        (unsigned long long)got, (unsigned long long)N);
            if (N == 0) return empty();
            if (P.kslots && !over_seg.empty()) {
                if (verbose) fprintf(stderr, "[bbk] msd key slots: %zu segments overflow, exact mode\n", over_seg.size());
                return Outcome::KeySlotsGaveUp;
            }
            return std::nullopt;
        }

        static size_t pad4(size_t words) { return (words + 7) & ~(size_t)3; }  // 16-byte steps, 16 spare bytes at least
        // words of the layout block; off_w (optional): where seg_tile, seg_off, seg_nb2, seg_bin, seg_size, xstart begin
        size_t layout_words(uint32_t *off_w) const {
            const size_t len[6] = {(size_t)P.nsub + 1, (size_t)P.nsub + 1, P.nb1, (size_t)P.nb1 + 1, P.nsub, P.nsub};
            size_t at = 0;
            for (int i = 0; i < 6; ++i) {
                if (off_w) off_w[i] = (uint32_t)at;
                at += pad4(len[i]);
            }
            return at;
        }

        // ---- level-2 layout: bins per segment, tile descriptors
        void level2_layout() {
            const uint32_t nb1 = P.nb1, nsub = P.nsub, xs = P.xs;
            if (!P.slots)
                for (uint32_t b = 0; b < nb1; ++b) hsub[b] = h1[b];  // exact mode: one dense run per segment
            tstart[0] = 0;
            sbin[0] = 0;
            const uint32_t tile2 = P.late_tag ? (uint32_t)(kLtThreads * kLt2Items)
                                   : P.narrow   ? (uint32_t)(has_val ? Nw2Cfg<true>::TILE : Nw2Cfg<false>::TILE)
                                                : kPartTileK;
            for (uint32_t s2 = 0; s2 < nsub; ++s2) tstart[s2 + 1] = tstart[s2] + (hsub[s2] + tile2 - 1) / tile2;
            for (uint32_t b = 0; b < nb1; ++b) {
                // (late tag: 16 tags x nsub key ranges per segment)
                snb2[b] = P.late_tag ? 16u * (uint32_t)std::min<double>(kMaxBins / 16, std::max(1.0, std::ceil((double)h1[b] / (16.0 * P.target))))
                                     : (uint32_t)std::min<double>(kMaxBins, std::max(1.0, std::ceil((double)h1[b] / P.target)));
                sbin[b + 1] = sbin[b] + snb2[b];
            }
            nbuckets = sbin[nb1];

            // narrow stage B (see k_bucket_base): key slots (which imply the direct output), one whole pass, no payload,
            // KEYS prefix, and no bucket spanning more than 2^32 keys -- then only the keys' low words travel after level 1
            const int w0bits = R.w0bits();
            uint64_t span_b = 0;  // widest bucket, in keys
            for (uint32_t b = 0; b < nb1; ++b)
                if (h1[b]) {
                    const uint64_t Q = 1ull << (32 - P.b1), q = (Q + snb2[b] - 1) / snb2[b];
                    span_b = std::max(span_b, w0bits > 32 ? q << (w0bits - 32) : q >> (32 - w0bits));
                }
            narrow_b = W == 1 && P.kslots && !R.even_part && !ranged && !has_dst && !has_val && R.op == MSD_OP_NONE &&
                       R.dmode == MSD_KEYS && span_b <= (1ull << 32) && !R.knobs.once.no_narrow_b;
            if (P.late_tag) narrow_b = true;  // a bucket is one tag and part of one segment: below 2^32 keys by construction
            if (P.late_tag && verbose)
                fprintf(stderr, "[bbk] msd key slots: 4-byte records from level 1, tag taken at level 2 (%u buckets)\n", nbuckets);
            else if (P.kslots && verbose)
                fprintf(stderr, "[bbk] msd key slots: %s records from level 2 (widest bucket 2^%.1f keys)\n",
                        narrow_b ? "4-byte" : "8-byte", std::log2((double)std::max<uint64_t>(span_b, 1)));

            ntiles2 = tstart[nsub];
            // narrow level 2: workgroups dealt to the XCDs by segment (k_tile_desc_narrow); BBK_XCD_TILES=0: A/B
            nwg2 = ntiles2;  // workgroups of the level-2 kernel
            if (R.knobs.once.xcd_tiles && ntiles2) {  // (exact mode too: its histogram pass keeps the plain order, see desc2h)
                xstart.resize(nsub);
                uint32_t per_xcd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                for (uint32_t s2 = 0; s2 < nsub; ++s2) {
                    uint32_t &c = per_xcd[(s2 >> xs) & 7u];
                    xstart[s2] = c;
                    c += tstart[s2 + 1] - tstart[s2];
                }
                nwg2 = 8u * *std::max_element(per_xcd, per_xcd + 8);
            }
            // the six arrays into the pinned block behind the cursors' part, one copy, one device block
            uint32_t off_w[6];
            const size_t words = layout_words(off_w);
            layout_d.alloc(words * 4);
            uint32_t *h = stage + pad4(nsub), *d = layout_d.as<uint32_t>();
            memcpy(h + off_w[0], tstart.data(), ((size_t)nsub + 1) * 4);
            memcpy(h + off_w[1], off1.data(), ((size_t)nsub + 1) * 4);
            memcpy(h + off_w[2], snb2.data(), (size_t)nb1 * 4);
            memcpy(h + off_w[3], sbin.data(), ((size_t)nb1 + 1) * 4);
            memcpy(h + off_w[4], hsub.data(), (size_t)nsub * 4);
            if (!xstart.empty()) memcpy(h + off_w[5], xstart.data(), (size_t)nsub * 4);
            BBK_HIP(hipMemcpyAsync(d, h, words * 4, hipMemcpyHostToDevice, ctx->stream));
            seg_tile = d + off_w[0];
            seg_off = d + off_w[1];
            seg_nb2 = d + off_w[2];
            seg_bin = d + off_w[3];
            seg_size = d + off_w[4];
            xstart_d = xstart.empty() ? nullptr : d + off_w[5];
            L2 = PartLevel{2, P.b1, nb1, R.dmode, w0bits, seg_nb2, seg_bin, sel.lo, sel.span, sel.shl, sel.mul};
            M2 = TileMap{seg_tile, seg_off, seg_size, nsub, N, ntiles2, 1, nullptr, 0, 0};
            desc2.alloc((size_t)nwg2 * sizeof(uint4) + 16);
            if (ntiles2) {
                if (xstart_d) BBK_HIP(hipMemsetAsync(desc2.p, 0, (size_t)nwg2 * sizeof(uint4), ctx->stream));
                hipLaunchKernelGGL((P.narrow || P.late_tag) ? k_tile_desc_narrow : k_tile_desc, dim3((ntiles2 + 255) / 256), dim3(256), 0,
                                   ctx->stream, M2, seg_nb2, seg_bin, tile2, xs, (const uint32_t *)xstart_d,
                                   desc2.as<uint4>());
                check_launch("k_tile_desc");
            }
            M2.desc = desc2.as<uint4>();
            // exact mode: the histogram kernel walks 16 consecutive tiles per workgroup and wants them in plain order
            if (!P.slots && xstart_d && !P.narrow) {
                desc2h.alloc((size_t)ntiles2 * sizeof(uint4) + 16);
                hipLaunchKernelGGL(k_tile_desc, dim3((ntiles2 + 255) / 256), dim3(256), 0, ctx->stream, M2, seg_nb2, seg_bin,
                                   kPartTileK, xs, (const uint32_t *)nullptr, desc2h.as<uint4>());
                check_launch("k_tile_desc");
            }
        }

        // ---- level 2: bucket offsets (exact histogram, or the slots' cursors), scatter
        void level2_scatter() {
            hist2.alloc((size_t)nbuckets * 4 + 16);
            boff.alloc(((size_t)nbuckets + 1) * 4 + 16);
            const uint64_t nB = P.slots ? (uint64_t)nbuckets * P.stride2 : N;
            if (P.slots) BBK_REQUIRE(nB + N < (1ull << 32), BBK_ERR_INTERNAL, "slot layout exceeds 32-bit offsets");
            bufB.alloc(nB * (narrow_b ? 4 : P.rec_ab));
            if (need_vbuf) valB.alloc(nB * 4);
            if (!P.slots) {
                BBK_HIP(hipMemsetAsync(hist2.p, 0, (size_t)nbuckets * 4 + 16, ctx->stream));
                TileMap M2h = M2;
                if (desc2h.p) M2h.desc = desc2h.as<uint4>();
                R.template launch_part<false, true, false>("k_part_hist2", (double)N * rec, ntiles2, bufA.as<Key<W>>(), nullptr,
                                                    M2h, L2, hist2.as<uint32_t>(), nullptr, nullptr, nullptr);
                DevBuf h64(((size_t)nbuckets + 1) * 8);
                hipLaunchKernelGGL(k_u32_to_u64, dim3((nbuckets + 255) / 256), dim3(256), 0, ctx->stream,
                                   hist2.as<uint32_t>(), (uint64_t)nbuckets, h64.as<uint64_t>(), 0u);
                check_launch("k_u32_to_u64");
                const uint64_t tot = exclusive_scan_u64(ctx, h64.as<uint64_t>(), h64.as<uint64_t>(), nbuckets);
                BBK_REQUIRE(tot == N, BBK_ERR_INTERNAL, "level-2 histogram does not add up");
                hipLaunchKernelGGL(k_scan_to_u32, dim3((nbuckets + 1 + 255) / 256), dim3(256), 0, ctx->stream,
                                   h64.as<uint64_t>(), (uint64_t)nbuckets, tot, (const uint64_t *)nullptr,
                                   boff.as<uint32_t>());
                check_launch("k_scan_to_u32");
                BBK_HIP(bbk::copy_async(hist2.p, boff.p, (size_t)nbuckets * 4, hipMemcpyDeviceToDevice, ctx->stream));
                stream_wait(ctx);
            } else {
                // cursor of bucket g starts at its slot; narrow path: the segment of every bucket, for the dedup kernel
                if (P.narrow) bseg.alloc(((size_t)nbuckets + 1) * 2);
                hipLaunchKernelGGL(k_bucket_init, dim3((nbuckets + 255) / 256), dim3(256), 0, ctx->stream,
                                   hist2.as<uint32_t>(), nbuckets, P.stride2, (const uint32_t *)seg_bin, P.nb1,
                                   P.narrow ? bseg.as<uint16_t>() : (uint16_t *)nullptr);
                check_launch("k_bucket_init");
                use_slots(L2, P.cap2, P.stride2);
            }
            if (P.narrow) {
                if (ntiles2)
                    R.launch(has_val ? k_part_narrow2<true> : k_part_narrow2<false>, "k_part_narrow2",
                             2.0 * (double)N * (4 + (has_val ? 4 : 0)), nwg2, kNw2Threads, part_narrow2_smem(has_val),
                             bufA.as<uint32_t>(), vals_or_null(valA), desc2.as<uint4>(), L2, hist2.as<uint32_t>(),
                             bufB.as<uint32_t>(), vals_or_null(valB));
            } else if (P.late_tag) {
                if constexpr (W == 1)
                    if (ntiles2)
                        R.launch(k_part_lt2, "k_part_l2", 2.0 * (double)N * 4, nwg2, kLtThreads, lt_smem(kLt2Items, 0),
                                 bufA.as<uint32_t>(), desc2.as<uint4>(), (int)R.expand_k, L2, hist2.as<uint32_t>(),
                                 bufB.as<uint32_t>());
            } else if (narrow_b) {
                if constexpr (W == 1)
                    R.template launch_part<false, false, false, true>("k_part_l2", (double)N * (rec + 4), nwg2,
                                                                        bufA.as<Key<W>>(), nullptr, M2, L2, nullptr,
                                                                        hist2.as<uint32_t>(), bufB.as<Key<W>>(), nullptr);
            } else {
                R.template scatter_keys<false>(has_val, "k_part_l2", 2.0 * rec_bytes(N), nwg2, bufA.as<Key<W>>(), valA.as<uint32_t>(), M2,
                               L2, hist2.as<uint32_t>(), bufB.as<Key<W>>(), valB.as<uint32_t>());
            }
        }

        // ---- buckets in LDS: the first pass; the direct output's result, give-up or in-place redo
        std::optional<Outcome> first_pass() {
            dcount.alloc((size_t)nbuckets * 4 + 16);
            // (slot mode: the dedup kernels leave the distinct records at the head of every bucket slot, like the exact
            // mode in its dense buckets; the compaction makes the result.  BucketArgs::out_keys / out_total -- every
            // bucket reserving its place in the result with an atomicAdd on one counter -- is no longer used: the counter
            // served the 227 210 buckets of BASELINE configs[1] one after the other, 2.6 ms of 2.8.)
            A = BucketArgs{boff.as<uint32_t>(), dcount.as<uint32_t>(), nullptr, (int)R.k,
                           verbose ? ctl_at(kCtlDbg) : nullptr, P.slots ? P.cap2 : 0u, P.slots ? P.stride2 : 0u,
                           hist2.as<uint32_t>(), nullptr, nullptr, nullptr, ~0ull, R.knobs.once.hash_max_probes, nullptr};
            // Sorted output of a key array that should hold no duplicates (both strands of a distinct canonical set, odd
            // k): the dense result has the offsets of the input, so the sorting kernels write it directly -- no
            // compaction pass.  Should a bucket remove a duplicate after all, or be left to the second chance, the pass
            // is redone in place (the direct pass does not touch the buckets).
            direct = (!P.slots || P.kslots) && R.assume_distinct && (R.dmode == MSD_KEYS || R.dmode == MSD_REF) &&
                     !R.knobs.no_direct;
            if (P.kslots) {
                // dense output offsets = exclusive scan of the slot fills (read from the cursors by the scan itself).  A
                // total below N means a record missed its slot: the host learns it with the flags, after the buckets have
                // run -- such a record also counts in ctr[0], and offsets from a total below N stay inside out.keys
                c64.alloc(((size_t)nbuckets + 1) * 8);
                uint64_t *const so = c64.as<uint64_t>();
                slot_off.alloc(((size_t)nbuckets + 1) * 4 + 16);
                if (P.late_tag) {
                    // buckets lie as (segment, tag, sub), the result is ordered (tag, segment, sub): the fills are
                    // gathered in that order, scanned, and the offsets brought back to the buckets
                    const dim3 gb((nbuckets + 255) / 256);
                    bbase.alloc(((size_t)nbuckets + 1) * 8);
                    bperm.alloc(((size_t)nbuckets + 1) * 4);
                    pfill.alloc(((size_t)nbuckets + 1) * 4);
                    hipLaunchKernelGGL(k_bucket_base_lt, gb, dim3(256), 0, ctx->stream, (const uint32_t *)seg_nb2,
                                       (const uint32_t *)seg_bin, P.nb1, nbuckets, 2 * (int)R.expand_k - 10, (int)R.expand_k,
                                       bbase.as<uint64_t>(), bperm.as<uint32_t>());
                    check_launch("k_bucket_base_lt");
                    hipLaunchKernelGGL(k_lt_fill_perm, gb, dim3(256), 0, ctx->stream, hist2.as<uint32_t>(),
                                       bperm.as<uint32_t>(), nbuckets, P.stride2, P.cap2, pfill.as<uint32_t>());
                    check_launch("k_lt_fill_perm");
                    const ScanSrc src{pfill.p, SCAN_U32_FLAGGED, 0u, 0u};
                    exclusive_scan_enqueue(ctx, 1, &src, &so, nbuckets, ctl_total(), false, scan_keep);
                    hipLaunchKernelGGL(k_lt_unperm, gb, dim3(256), 0, ctx->stream, c64.as<uint64_t>(), bperm.as<uint32_t>(),
                                       nbuckets, slot_off.as<uint32_t>());
                    check_launch("k_lt_unperm");
                } else {
                    const ScanSrc src{hist2.p, SCAN_SLOT_FILL, P.stride2, P.cap2};
                    exclusive_scan_enqueue(ctx, 1, &src, &so, nbuckets, ctl_total(), false, scan_keep);
                    hipLaunchKernelGGL(k_scan_to_u32, dim3((nbuckets + 1 + 255) / 256), dim3(256), 0, ctx->stream,
                                       c64.as<uint64_t>(), (uint64_t)nbuckets, 0ull, (const uint64_t *)ctl_total(),
                                       slot_off.as<uint32_t>());
                    check_launch("k_scan_to_u32");
                }
                A.out_off = slot_off.as<uint32_t>();
            }
            if (direct) {
                if (!has_dst) {
                    out.keys.alloc(N * rec + 16);
                    if (out_vals) out.vals.alloc(N * 4 + 16);
                }
                A.sorted_keys = has_dst ? dst.keys : out.keys.p;
                A.sorted_vals = has_dst ? dst.vals : out.vals.as<uint32_t>();
                A.dup_flag = ctl_at(kCtlDup);
                A.strip_mask = R.strip_mask;
            }
            launch_buckets();
            // buckets the first pass left alone: listed on the device, only the (short) list comes to the host
            flag_ids.alloc((size_t)kFlagCap * 4);
            // hash slots: the scan of the distinct counts (the dense offsets; D) rides on the same wait.  The buckets a
            // flagged list excludes count 0 in it already, so it does not depend on the host's look at the flags
            if (P.hslots && !direct) {
                d64.alloc(((size_t)nbuckets + 1) * 8);
                const ScanSrc src{dcount.p, SCAN_U32_FLAGGED, 0u, 0u};
                uint64_t *const so = d64.as<uint64_t>();
                exclusive_scan_enqueue(ctx, 1, &src, &so, nbuckets, ctl_total(), false, scan_keep);
                d64_scanned = true;
            }
            fetch_flags();
            if (P.kslots && h_total() != N) {
                if (verbose) fprintf(stderr, "[bbk] msd key slots: %llu of %llu records placed, exact mode\n",
                                     (unsigned long long)h_total(), (unsigned long long)N);
                out.keys.release();
                out.vals.release();
                return give_up_key_slots();
            }
            if (!direct) return std::nullopt;
            if (ctr[2] == 0 && ctr[3] == 0 && (!P.kslots || ctr[0] == 0)) {  // every bucket sorted, nothing removed or
                out.n = N;                                                    // spilled: the result is complete
                out.nbuckets = 0;
                out.overflow_buckets = 0;
                if (P.kslots && verbose)
                    fprintf(stderr, "[bbk] msd key slots N=%llu buckets=%u: ordered without histograms\n",
                            (unsigned long long)N, nbuckets);
                return Outcome::Done;
            }
            if (P.kslots) {
                if (verbose) fprintf(stderr, "[bbk] msd key slots given up (spill=%u flagged=%u dup=%u), exact mode\n", ctr[0],
                                     ctr[2], ctr[3]);
                out.keys.release();
                out.vals.release();
                return give_up_key_slots();
            }
            if (verbose) fprintf(stderr, "[bbk] msd direct output withdrawn (flagged=%u dup=%u): in-place pass\n", ctr[2], ctr[3]);
            if (!has_dst) {
                out.keys.release();
                out.vals.release();
            }
            A.sorted_keys = nullptr;
            A.sorted_vals = nullptr;
            A.dup_flag = nullptr;
            A.strip_mask = ~0ull;
            R.template bucket_dispatch<false>(nbuckets, bufB.as<Key<W>>(), valB.as<uint32_t>(), A, rec_bytes(N));
            fetch_flags();
            return std::nullopt;
        }

        // the first-pass bucket kernel of the mode
        void launch_buckets() {
            if (P.narrow) {
                if constexpr (W == 1) {
                    if (nbuckets)
                        with_op(R.op, [&](auto o) {
                            constexpr int OP = decltype(o)::value;
                            R.launch(k_bucket_hash32<OP>, "k_bucket_hash32", (double)N * (4 + (has_val ? 4 : 0)), nbuckets,
                                     kNwHashThreads, bucket_hash32_smem<OP>(), bufB.as<uint32_t>(), valB.as<uint32_t>(), A,
                                     bseg.as<uint16_t>(), P.nw_hb);
                        });
                }
            } else if (narrow_b) {
                if constexpr (W == 1) {
                    BBK_REQUIRE(direct, BBK_ERR_INTERNAL, "4-byte stage-B records need the direct output");
                    if (!P.late_tag) bbase.alloc(((size_t)nbuckets + 1) * 8);  // (late tag: k_bucket_base_lt, with the offsets)
                    if (nbuckets) {
                        if (!P.late_tag) {
                            hipLaunchKernelGGL(k_bucket_base, dim3((nbuckets + 255) / 256), dim3(256), 0, ctx->stream,
                                               (const uint32_t *)seg_nb2, (const uint32_t *)seg_bin, P.nb1, nbuckets, P.b1,
                                               R.w0bits(), bbase.as<uint64_t>());
                            check_launch("k_bucket_base");
                        }
                        constexpr int NT = BktCfg<1>::NT, IT = BktCfg<1>::ITEMS;
                        R.launch(k_bucket_dist_nb<NT, IT>, "k_bucket_dist", (double)N * (4 + rec), nbuckets, NT,
                                 bucket_dist_nb_smem<NT, IT>(), bufB.as<uint32_t>(), bbase.as<uint64_t>(), A);
                    }
                }
            } else {
                R.template bucket_dispatch<false>(nbuckets, bufB.as<Key<W>>(), valB.as<uint32_t>(), A, rec_bytes(N));
            }
        }

        void fetch_flags() {
            uint32_t *d_flag_n = P.slots ? ctl_at(kCtlSpill) + 2 : ctl_at(kCtlFlagN);
            if (!P.slots) BBK_HIP(hipMemsetAsync(d_flag_n, 0, 16, ctx->stream));  // (a withdrawn direct pass counts again)
            hipLaunchKernelGGL(k_flagged, dim3((nbuckets + 255) / 256), dim3(256), 0, ctx->stream, dcount.as<uint32_t>(),
                               nbuckets, flag_ids.as<uint32_t>(), kFlagCap, d_flag_n);
            check_launch("k_flagged");
            // the whole control block in one copy: spill / flag / duplicate counters and the scan total that rode along
            BBK_HIP(hipMemcpyAsync(h_ctl, ctl.p, kCtlWords * 4, hipMemcpyDeviceToHost, ctx->stream));
            stream_wait(ctx);
            if (P.slots) memcpy(ctr, h_ctl + kCtlSpill, 12);
            else ctr[2] = h_ctl[kCtlFlagN];
            if (direct) ctr[3] = h_ctl[kCtlDup];
        }

        // ---- what the first pass left: the slot mode's overflow, or the exact mode's oversized buckets
        std::optional<Outcome> overflow() {
            const uint32_t n_flag = ctr[2];
            if (n_flag > kFlagCap) {  // tens of thousands of overflowing buckets: not an input for this path
                if (verbose) fprintf(stderr, "[bbk] msd: %u buckets overflow\n", n_flag);
                return P.slots ? Outcome::SlotsGaveUp : Outcome::Declined;
            }
            flagged.resize(n_flag);
            if (n_flag) {
                BBK_HIP(hipMemcpyAsync(flagged.data(), flag_ids.p, (size_t)n_flag * 4, hipMemcpyDeviceToHost, ctx->stream));
                stream_wait(ctx);
                std::sort(flagged.begin(), flagged.end());
            }
            const bool exact_check = !P.slots && (n_flag || verbose);
            if (exact_check) {
                hd.resize(nbuckets);
                hb.resize((size_t)nbuckets + 1);
                BBK_HIP(hipMemcpyAsync(hd.data(), dcount.p, (size_t)nbuckets * 4, hipMemcpyDeviceToHost, ctx->stream));
                BBK_HIP(hipMemcpyAsync(hb.data(), boff.p, ((size_t)nbuckets + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
                stream_wait(ctx);
            }
            if (P.slots)
                if (auto r = slot_overflow()) return r;
            bufA.release();
            valA.release();
            if (exact_check)
                if (auto r = exact_overflow()) return r;
            out.overflow_buckets = novf;
            return std::nullopt;
        }

        // slot mode: every record of the affected keys -- the spill list, the overflowing segments' and buckets'
        // slots -- is gathered and reduced on its own; its distinct records go to `extra`
        std::optional<Outcome> slot_overflow() {
            const uint32_t n_spill = ctr[0];
            if (n_spill > P.spill_cap) {  // more than an eighth of the input overflowed: not an input for this mode
                if (verbose) fprintf(stderr, "[bbk] msd slots: spill list overflow (%u), exact mode\n", n_spill);
                return Outcome::SlotsGaveUp;
            }
            const std::vector<uint32_t> &over_bkt = flagged;
            const uint32_t xs = P.xs;
            // records a flagged bucket's slot really holds: a bucket is also flagged when its LDS table gives up on a
            // slot that is NOT full (more distinct keys than the table takes), and the rest of such a slot is stale
            // pool memory -- never copy more than the level-2 cursor says was written
            std::vector<uint32_t> bkt_fill(over_bkt.size(), P.cap2);
            if (!over_bkt.empty()) {
                std::vector<uint32_t> cur2(nbuckets);
                BBK_HIP(hipMemcpyAsync(cur2.data(), hist2.p, (size_t)nbuckets * 4, hipMemcpyDeviceToHost, ctx->stream));
                stream_wait(ctx);
                for (size_t i = 0; i < over_bkt.size(); ++i) {
                    const uint32_t g = over_bkt[i];
                    bkt_fill[i] = std::min<uint32_t>(P.cap2, cur2[g] - g * P.stride2);
                }
            }
            uint64_t n_extra = (uint64_t)n_spill;
            for (uint32_t b : over_seg)
                for (uint32_t s2 = b << xs; s2 < (b + 1) << xs; ++s2) n_extra += fill1[s2];
            for (uint32_t f : bkt_fill) n_extra += f;
            if (verbose)
                fprintf(stderr, "[bbk] msd slots%s N=%llu nb1=%u seg_cap=%u buckets=%u spill=%u over_seg=%zu over_bkt=%zu\n",
                        P.narrow ? " (narrow records)" : "", (unsigned long long)N, P.nb1, P.seg_cap, nbuckets, n_spill,
                        over_seg.size(), over_bkt.size());
            ctx->add_stat("stat_slot_records", (double)N);
            ctx->add_stat("stat_slot_spilled", (double)n_spill);
            ctx->add_stat("stat_slot_overflow_segments", (double)over_seg.size());
            ctx->add_stat("stat_slot_overflow_buckets", (double)over_bkt.size());
            ctx->add_stat("stat_slot_reprocessed", (double)n_extra);
            if (n_extra > N / 2) {  // most of the input overflowed (a handful of distinct k-mers): not for this mode
                if (verbose) fprintf(stderr, "[bbk] msd slots: %llu of %llu records overflowed, exact mode\n",
                                     (unsigned long long)n_extra, (unsigned long long)N);
                return Outcome::SlotsGaveUp;
            }
            novf = over_bkt.size() + over_seg.size();
            if (n_extra == 0) return std::nullopt;
            const bool tiny = n_extra <= (uint64_t)BktCfg<W>::CAP2;  // fits one workgroup of the radix kernel
            DevBuf ek(n_extra * rec), ev;
            if (has_val || (tiny && out_vals)) ev.alloc(n_extra * 4 + 16);
            uint64_t o = 0;
            // narrow path: slots hold 4-byte records, widened with the segment they belong to (seg < 0: 8-byte keys)
            auto put = [&](const void *ksrc, const uint32_t *vsrc, uint64_t first, uint64_t cnt, int seg = -1) {
                if (!cnt) return;
                if (seg >= 0) {
                    hipLaunchKernelGGL(k_nw_widen, bbk::grid_blocks((cnt + 255) / 256), dim3(256), 0, ctx->stream,
                                       (const uint32_t *)ksrc + first, (uint32_t)cnt, (uint32_t)seg, P.nw_hb,
                                       ek.as<uint64_t>() + o);
                    check_launch("k_nw_widen");
                } else {
                    BBK_HIP(bbk::copy_async(ek.as<char>() + o * rec, (const char *)ksrc + first * rec, cnt * rec,
                                           hipMemcpyDeviceToDevice, ctx->stream));
                }
                if (has_val)
                    BBK_HIP(bbk::copy_async(ev.as<uint32_t>() + o, vsrc + first, cnt * 4, hipMemcpyDeviceToDevice,
                                           ctx->stream));
                o += cnt;
            };
            put(spill_k.p, spill_v.as<uint32_t>(), 0, n_spill);
            for (uint32_t b : over_seg)  // the written part of its slot (of every per-XCD sub-slot on the narrow path)
                for (uint32_t s2 = b << xs; s2 < (b + 1) << xs; ++s2)
                    put(bufA.p, valA.as<uint32_t>(), (uint64_t)off1[s2], fill1[s2], P.narrow ? (int)b : -1);
            for (size_t i = 0; i < over_bkt.size(); ++i)
                put(bufB.p, valB.as<uint32_t>(), (uint64_t)over_bkt[i] * P.stride2, bkt_fill[i],
                    P.narrow ? (int)(std::upper_bound(sbin.begin(), sbin.end(), over_bkt[i]) - sbin.begin()) - 1 : -1);
            if (tiny) {
                // the usual case (one or two crowded buckets): ONE workgroup sorts + reduces all of it in LDS,
                // instead of a whole partition pipeline for a few thousand records
                DevBuf tb(16), tc(16);
                hbo[1] = (uint32_t)n_extra;
                BBK_HIP(hipMemcpyAsync(tb.p, hbo, 8, hipMemcpyHostToDevice, ctx->stream));
                BucketArgs At{tb.as<uint32_t>(), tc.as<uint32_t>(), nullptr, (int)R.k, nullptr, 0u, 0u,
                              nullptr, nullptr, nullptr, nullptr, ~0ull, R.knobs.once.hash_max_probes, nullptr};
                MsdRunner<W> sorter = R;
                sorter.dmode = MSD_KEYS;  // picks the sorting kernels in bucket_dispatch
                sorter.expand_k = 0;
                sorter.template bucket_dispatch<true>(1u, ek.as<Key<W>>(), ev.as<uint32_t>(), At, rec_bytes(n_extra),
                                                      /*allow_hash=*/false);
                uint32_t d = 0;
                BBK_HIP(hipMemcpyAsync(&d, tc.p, 4, hipMemcpyDeviceToHost, ctx->stream));
                stream_wait(ctx);
                BBK_REQUIRE(d != 0xFFFFFFFFu && d <= n_extra, BBK_ERR_INTERNAL, "overflow pass: bad count");
                extra.n = d;
                extra.keys = std::move(ek);
                if (out_vals) extra.vals = std::move(ev);
                return std::nullopt;
            }
            stream_wait(ctx);
            // The records were selected BY their hash bucket, so the same hash would pile them up again:
            // partition them by key instead (the order of the result does not matter), and never decline --
            // a k-mer with a million instances is finished by the per-bucket LSD fallback.
            MsdRunner<W> exact = R;
            exact.slots_ok = false;
            exact.dmode = MSD_KEYS;
            exact.never_decline = true;
            exact.expand_k = 0;
            // declined (e.g. one k-mer makes up most of it): so does this call, the caller takes the LSD path
            if (!exact.run_all(MsdInput{nullptr, ek.p, has_val ? ev.as<uint32_t>() : nullptr, n_extra, false}, extra))
                return Outcome::Declined;
            extra.bucket_off.release();
            return std::nullopt;
        }

        // ---- exact mode, buckets above CAP: a second pass with 512-thread workgroups (2 x CAP); what still does not
        // fit (a k-mer repeated > 12 k times in one bucket) is finished by the LSD path, one by one
        std::optional<Outcome> exact_overflow() {
            uint64_t big_rec = 0, ovf_rec = 0;
            // second chance: the ballot-ranked radix kernel with 512 threads -- buckets above the first pass's
            // capacity (8-byte keys: 2 x CAP; wider keys: more than the 4096-record hash kernel) and buckets the
            // distribution sort turned down for a crowded bin
            const uint32_t cap2nd = BktCfg<W>::CAP2;
            for (uint32_t b = 0; b < nbuckets; ++b)
                if (hd[b] == 0xFFFFFFFFu && hb[b + 1] - hb[b] <= cap2nd) {
                    big.push_back(b);
                    big_rec += hb[b + 1] - hb[b];
                }
            if (!big.empty()) {
                DevBuf ids(big.size() * 4);
                BBK_HIP(hipMemcpyAsync(ids.p, big.data(), big.size() * 4, hipMemcpyHostToDevice, ctx->stream));
                BucketArgs A2{boff.as<uint32_t>(), dcount.as<uint32_t>(), ids.as<uint32_t>(), (int)R.k, nullptr, 0u, 0u,
                              nullptr, nullptr, nullptr, nullptr, ~0ull, R.knobs.once.hash_max_probes, nullptr};
                R.template bucket_dispatch<true>((uint32_t)big.size(), bufB.as<Key<W>>(), valB.as<uint32_t>(), A2,
                                                 rec_bytes(big_rec), /*allow_hash=*/false);
                BBK_HIP(hipMemcpyAsync(hd.data(), dcount.p, (size_t)nbuckets * 4, hipMemcpyDeviceToHost, ctx->stream));
                stream_wait(ctx);
            }
            for (uint32_t b = 0; b < nbuckets; ++b)
                if (hd[b] == 0xFFFFFFFFu) {
                    ++novf;
                    ovf_rec += hb[b + 1] - hb[b];
                }
            if (verbose) {
                uint32_t mx = 0;
                for (uint32_t b = 0; b < nbuckets; ++b) mx = std::max(mx, hb[b + 1] - hb[b]);
                uint32_t hdbg[2] = {0, 0};
                BBK_HIP(hipMemcpyAsync(hdbg, ctl_at(kCtlDbg), 8, hipMemcpyDeviceToHost, ctx->stream));
                stream_wait(ctx);
                fprintf(stderr, "[bbk] msd all-words-fallback buckets=%u\n", hdbg[0]);
                fprintf(stderr, "[bbk] msd mode=%d N=%llu nb1=%u buckets=%u max_bucket=%u cap=%u big=%zu lsd=%llu (%llu rec)\n",
                        R.dmode, (unsigned long long)N, P.nb1, nbuckets, mx, R.bucket_cap(), big.size(),
                        (unsigned long long)novf, (unsigned long long)ovf_rec);
            }
            if (!R.never_decline && (novf > 256 || ovf_rec > N / 4)) {
                if (verbose)
                    fprintf(stderr, "[bbk] msd declines: N=%llu, %llu records in %llu buckets above the bucket kernels\n",
                            (unsigned long long)N, (unsigned long long)ovf_rec, (unsigned long long)novf);
                return Outcome::Declined;
            }
            if (novf == 0) return std::nullopt;
            const int op = R.op;
            const ReduceOp rop = op == MSD_OP_OR ? REDUCE_OR : (op == MSD_OP_SUM ? REDUCE_SUM : REDUCE_COUNT);
            for (uint32_t b = 0; b < nbuckets; ++b) {
                if (hd[b] != 0xFFFFFFFFu) continue;
                const uint64_t cnt = hb[b + 1] - hb[b];
                Key<W> *kb = bufB.as<Key<W>>() + hb[b];
                uint32_t *vb = need_vbuf ? valB.as<uint32_t>() + hb[b] : nullptr;
                DevBuf tk(cnt * rec), tv(cnt * 4), ok(cnt * rec), ov(cnt * 4);
                sort_records(ctx, W, kb, tk.p, has_val ? vb : nullptr, has_val ? tv.as<uint32_t>() : nullptr, cnt,
                             key_passes(R.k));
                const uint64_t d = unique_records(ctx, W, kb, has_val ? vb : nullptr, cnt, ok.p,
                                                  out_vals ? ov.as<uint32_t>() : nullptr, rop, false);
                BBK_HIP(bbk::copy_async(kb, ok.p, d * rec, hipMemcpyDeviceToDevice, ctx->stream));
                if (out_vals) BBK_HIP(bbk::copy_async(vb, ov.p, d * 4, hipMemcpyDeviceToDevice, ctx->stream));
                stream_wait(ctx);
                hd[b] = (uint32_t)d;
            }
            BBK_HIP(hipMemcpyAsync(dcount.p, hd.data(), (size_t)nbuckets * 4, hipMemcpyHostToDevice, ctx->stream));
            return std::nullopt;
        }

        // Narrow stage A whose caller asked for a BucketView: the buckets stay where they are, no compaction.  Not when
        // the device could not hold the slots beside stage B's buffers (they take ~4x the dense array).
        bool hand_off_view(uint64_t D, DevBuf &d64) {
            if (!out.want_view) return false;
            const char *why = nullptr;
            if (W != 1 || !P.narrow || out_vals || has_dst || ranged) why = "not a narrow pass";
            else if (R.knobs.once.no_bucket_handoff) why = "BBK_NO_BUCKET_HANDOFF";
            const size_t more = bufB.bytes > D * rec ? bufB.bytes - D * rec : 0;
            // (the driver is asked once per context and again only after the arena has mapped or trimmed)
            if (!why && more > device_free_cached(ctx)) why = "device memory";
            if (verbose)
                fprintf(stderr, "[bbk] msd hand-off to stage B: %s (%llu keys, buckets %.0f MB, dense %.0f MB)%s%s\n",
                        why ? "dense array" : "bucket view", (unsigned long long)out.n, bufB.bytes / 1e6, out.n * rec / 1e6,
                        why ? ": " : "", why ? why : "");
            if (why) return false;
            BucketView &v = out.view;
            v.slots = std::move(bufB);
            v.dcount = std::move(dcount);
            v.off = std::move(d64);
            v.seg = std::move(bseg);
            v.nbuckets = nbuckets;
            v.stride = P.stride2;
            v.hb = P.nw_hb;
            v.D = D;
            v.n_extra = extra.n;
            if (extra.n) v.extra = std::move(extra.keys);
            out.nbuckets = 0;
            return true;  // no wait: everything the queued kernels use has moved into the view, which outlives the call
        }

        // ---- dense output: scan of the bucket counts + compaction.  (Slot mode: overflowing buckets wrote nothing and
        // count 0 here; their records are in `extra`, appended.)  Exact HASH mode also gets the bucket table.
        void compact() {
            uint64_t D = 0;
            if (d64_scanned) {  // scanned before fetch_flags' wait, the total came back with the flags
                D = h_total();
            } else {  // exact mode: the overflow passes have rewritten counts since the flags were read
                d64.alloc(((size_t)nbuckets + 1) * 8);
                const ScanSrc src{dcount.p, SCAN_U32_FLAGGED, 0u, 0u};
                uint64_t *const so = d64.as<uint64_t>();
                exclusive_scan_enqueue(ctx, 1, &src, &so, nbuckets, ctl_total(), false, scan_keep);
                BBK_HIP(hipMemcpyAsync(&D, ctl_total(), 8, hipMemcpyDeviceToHost, ctx->stream));
                stream_wait(ctx);
            }
            if (P.slots) BBK_REQUIRE(D + extra.n <= N, BBK_ERR_INTERNAL, "more distinct records than records");
            out.n = D + (P.slots ? extra.n : 0);
            if (hand_off_view(D, d64)) return;
            if (!has_dst) {
                out.keys.alloc(out.n * rec + 16);
                if (out_vals) out.vals.alloc(out.n * 4 + 16);
            }
            Key<W> *ck = has_dst ? (Key<W> *)dst.keys : out.keys.as<Key<W>>();
            uint32_t *cv = !out_vals ? nullptr : has_dst ? dst.vals : out.vals.as<uint32_t>();
            const uint32_t *vb = out_vals ? valB.as<uint32_t>() : nullptr;
            const uint32_t *cboff = P.slots ? nullptr : boff.as<uint32_t>();  // slot mode: bucket b starts at b * stride2
            const unsigned blocks = (unsigned)(((uint64_t)nbuckets * 64 + 255) / 256);
            if (P.narrow) {
                if constexpr (W == 1)
                    R.launch(out_vals ? k_compact_narrow<true> : k_compact_narrow<false>, "compact",
                             (double)D * (4 + 8 + (out_vals ? 8 : 0)), blocks, 256, 0, bufB.as<uint32_t>(), vb,
                             dcount.as<uint32_t>(), d64.as<uint64_t>(), nbuckets, P.stride2, bseg.as<uint16_t>(), P.nw_hb,
                             reinterpret_cast<uint64_t *>(ck), cv);
            } else {
                R.launch(out_vals ? k_compact<W, true> : k_compact<W, false>, "compact",
                         2.0 * (double)D * (rec + (out_vals ? 4 : 0)), blocks, 256, 0, bufB.as<Key<W>>(), vb, cboff,
                         dcount.as<uint32_t>(), d64.as<uint64_t>(), nbuckets, ck, cv, R.strip_mask, P.stride2);
            }
            if (extra.n) {
                BBK_HIP(bbk::copy_async(out.keys.as<char>() + D * rec, extra.keys.p, extra.n * rec, hipMemcpyDeviceToDevice,
                                       ctx->stream));
                if (out_vals)
                    BBK_HIP(bbk::copy_async(out.vals.as<uint32_t>() + D, extra.vals.p, extra.n * 4, hipMemcpyDeviceToDevice,
                                           ctx->stream));
            }
            out.nbuckets = P.slots ? 0 : nbuckets;
            if (!P.slots) {
                out.bucket_off.alloc(((size_t)nbuckets + 1) * 4);
                hipLaunchKernelGGL(k_scan_to_u32, dim3((nbuckets + 1 + 255) / 256), dim3(256), 0, ctx->stream,
                                   d64.as<uint64_t>(), (uint64_t)nbuckets, D, (const uint64_t *)nullptr,
                                   out.bucket_off.as<uint32_t>());
                check_launch("k_scan_to_u32");
            }
            stream_wait(ctx);
        }
    };

    // One pass over the input, or over one range of its prefix space (sel), under the retry policy: a slot mode that
    // gave up stays off for the rest of the call, and the pass is rerun with exact histograms.  (The hash slots need
    // the HASH prefix, the key slots KEYS / REF: a pass gives up at most one of them.)
    // A BucketView input that a pass cannot (or no longer) read in place continues as the dense array.
    Outcome run_retrying(const MsdInput &in0, MsdOutput &out, const Sel &sel = Sel(), Dst dst = Dst(),
                         uint64_t *n_records = nullptr) {
        MsdInput in = in0;
        for (;;) {
            const Outcome r = Pass(*this, in, out, sel, dst).run(n_records);
            if (in.view && r != Outcome::Done) {
                if (knobs.verbose) fprintf(stderr, "[bbk] msd: stage A's buckets materialised (outcome %d)\n", (int)r);
                in = dense_of(in);
            }
            if (r == Outcome::NeedDense) continue;
            if (r == Outcome::SlotsGaveUp) slots_ok = false;
            else if (r == Outcome::KeySlotsGaveUp) kslots_ok = false;
            else return r;
        }
    }

    // Histogram of the whole input over the top `bits` bits of the prefix (key arrays, KEYS / REF prefix): the
    // range passes of run_all are sized from it, so a skewed key space still gives passes that fit.
    std::vector<uint64_t> prefix_histogram(const void *d_keys, uint64_t n_records, int bits) {
        const uint32_t nb = 1u << bits;
        DevBuf h((size_t)nb * 4 + 16);
        BBK_HIP(hipMemsetAsync(h.p, 0, (size_t)nb * 4 + 16, ctx->stream));
        PartLevel L{1, bits, nb, dmode, w0bits(), nullptr, nullptr, 0u, 0u, 0, 0u};
        TileMap M{nullptr, nullptr, nullptr, 1, n_records, 0, 1, nullptr, (int)expand_k, expand_tag ? 1 : 0};
        const uint64_t nt = (n_records + kPartTileK - 1) / kPartTileK;
        BBK_REQUIRE(nt < (1ull << 32), BBK_ERR_ARG, "input of %llu records exceeds the tile space", (unsigned long long)n_records);
        launch_part<false, true, true>("k_part_hist0", (double)(expand_k ? n_records / 2 : n_records) * rec, (uint32_t)nt,
                                 (const Key<W> *)d_keys, nullptr, M, L, h.as<uint32_t>(), nullptr, nullptr, nullptr);
        std::vector<uint32_t> h32(nb);
        BBK_HIP(hipMemcpyAsync(h32.data(), h.p, (size_t)nb * 4, hipMemcpyDeviceToHost, ctx->stream));
        stream_wait(ctx);
        std::vector<uint64_t> out(nb);
        uint64_t tot = 0;
        for (uint32_t i = 0; i < nb; ++i) tot += (out[i] = h32[i]);
        // a 32-bit counter that wrapped (one fine range above 2^32 records) shows up here
        BBK_REQUIRE(tot == n_records, BBK_ERR_ARG,
                    "key space too skewed for range passes (%llu of %llu records counted)", (unsigned long long)tot,
                    (unsigned long long)n_records);
        return out;
    }

    // Ranges of the prefix space for an input above one pass.  HASH: 2^b equal hash ranges (uniform whatever the
    // input).  KEYS / REF: consecutive fine ranges (1/512 of the prefix space) grouped up to the pass limit from
    // an exact histogram; REF additionally never lets a range straddle XXH3 buckets except as an aligned group of
    // 2^j whole buckets (see ref_bits in run()).
    bool plan_ranges(const bbk_reads *rd, const void *d_keys, uint64_t N, std::vector<Sel> &ranges) {
        const uint64_t limit = (uint64_t)((double)pass_limit(rd != nullptr) * 0.92);
        const bool verbose = knobs.verbose;
        ranges.clear();
        if (dmode == MSD_HASH) {
            // equal spans of the 32-bit hash space, as few as fit (not a power of two: 9.6 G records of 16-byte keys take
            // 10 passes, not 16 -- every pass re-extracts all k-mers of the reads)
            const uint64_t nr = (N + limit - 1) / limit;
            if (nr > 4096) return false;
            const uint64_t span = ((1ull << 32) + nr - 1) / nr;
            for (uint64_t v = 0; v < nr; ++v) {
                Sel s;
                const uint64_t lo = v * span, hi = std::min<uint64_t>(1ull << 32, lo + span);
                if (lo >= hi) break;
                s.lo = (uint32_t)lo;
                s.span = (uint32_t)(hi - lo);
                s.finish();
                s.est = (uint64_t)((double)N * (double)(hi - lo) / 4294967296.0 * 1.04) + 1;
                ranges.push_back(s);
            }
            if (verbose) fprintf(stderr, "[bbk] msd: %llu records in %zu hash ranges\n", (unsigned long long)N, ranges.size());
            return true;
        }
        BBK_REQUIRE(rd == nullptr, BBK_ERR_INTERNAL, "reads are partitioned by hash prefix only");
        constexpr int FB = 9;  // fine ranges: 512 (the level-1 histogram kernel's bin limit)
        const std::vector<uint64_t> h = prefix_histogram(d_keys, N, FB);
        auto emit = [&](uint32_t f0, uint32_t f1, uint64_t cnt) {  // fine ranges [f0, f1)
            Sel s;
            s.lo = f0 << (32 - FB);
            const uint64_t span = (uint64_t)(f1 - f0) << (32 - FB);
            if (span >= (1ull << 32)) {  // everything (cannot happen for an input above the limit, kept for safety)
                s.span = 0;
                s.shl = 0;
            } else {
                s.span = (uint32_t)span;
                s.finish();
            }
            s.est = cnt;
            if (cnt) ranges.push_back(s);
        };
        auto greedy = [&](uint32_t f0, uint32_t f1) -> bool {  // groups the fine ranges [f0, f1)
            uint32_t g0 = f0;
            uint64_t acc = 0;
            for (uint32_t f = f0; f < f1; ++f) {
                if (h[f] > limit) return false;
                if (acc + h[f] > limit) {
                    emit(g0, f, acc);
                    g0 = f;
                    acc = 0;
                }
                acc += h[f];
            }
            emit(g0, f1, acc);
            return true;
        };
        bool ok = true;
        if (dmode == MSD_KEYS) {
            // equal aligned pieces of the key space when they fit a pass (b0 bits: 2, 4, ... 64 pieces): run_all can then
            // split the input into them with ONE partition pass instead of selecting a piece from the whole input per pass
            int b0 = 0;
            for (int b = 1; b <= 6 && !b0; ++b) {
                const uint32_t per = (1u << FB) >> b;
                bool fits = true;
                for (uint32_t f = 0; f < (1u << FB) && fits; f += per) {
                    uint64_t t = 0;
                    for (uint32_t j = 0; j < per; ++j) t += h[f + j];
                    fits = t <= limit;
                }
                if (fits) b0 = b;
            }
            if (b0) {
                const uint32_t per = (1u << FB) >> b0;
                for (uint32_t f = 0; f < (1u << FB); f += per) {
                    uint64_t t = 0;
                    for (uint32_t j = 0; j < per; ++j) t += h[f + j];
                    Sel sp;  // kept even when empty: the pieces stay equal and aligned
                    sp.lo = f << (32 - FB);
                    sp.span = per << (32 - FB);
                    sp.finish();
                    sp.est = t;
                    ranges.push_back(sp);
                }
            } else {
                ok = greedy(0, 1u << FB);
            }
        } else {  // MSD_REF: fine ranges 32 x b .. 32 x b + 31 make up XXH3 bucket b
            constexpr uint32_t per = (1u << FB) / 16;
            uint64_t bt[16];
            for (int b = 0; b < 16; ++b) {
                bt[b] = 0;
                for (uint32_t f = 0; f < per; ++f) bt[b] += h[b * per + f];
            }
            int g = 8;  // largest aligned group of whole buckets that fits a pass
            for (; g >= 1; g >>= 1) {
                bool fits = true;
                for (int b = 0; b < 16 && fits; b += g) {
                    uint64_t t = 0;
                    for (int j = 0; j < g; ++j) t += bt[b + j];
                    fits = t <= limit;
                }
                if (fits) break;
            }
            if (g >= 1) {
                for (int b = 0; b < 16; b += g) {
                    uint64_t t = 0;
                    for (int j = 0; j < g; ++j) t += bt[b + j];
                    emit((uint32_t)b * per, (uint32_t)(b + g) * per, t);
                }
            } else {
                for (int b = 0; b < 16 && ok; ++b) ok = greedy((uint32_t)b * per, (uint32_t)(b + 1) * per);
            }
        }
        if (verbose) {
            fprintf(stderr, "[bbk] msd: %llu records, prefix mode %d, %zu key ranges%s:", (unsigned long long)N, dmode,
                    ranges.size(), ok ? "" : " (a fine range exceeds one pass)");
            for (const Sel &r : ranges) fprintf(stderr, " %llu", (unsigned long long)r.est);
            fprintf(stderr, "\n");
        }
        return ok;
    }

    // Key-array input in R >= 3 equal, aligned ranges of the prefix space (KEYS: pieces of the key space; REF: groups of
    // XXH3 buckets): selecting one range from the WHOLE input per pass reads -- and for an expanded canonical array
    // regenerates -- everything R times, twice (histogram + scatter), and keeps 1/R of every tile.  Instead a "level 0"
    // partition pass writes the records grouped by range once (the counts are already known from the planning
    // histogram), and every range is then an ordinary key array.  Level 0 runs in chunks of 2^j ranges that stay below
    // the 32-bit record offsets of one pass.  false: not applicable (the caller selects per pass as before).
    bool level0_ranges(const MsdInput &in, const std::vector<Sel> &ranges, MsdOutput &out, uint64_t &D, uint64_t &inst) {
        const size_t R = ranges.size();
        if (R < 3 || (R & (R - 1)) || knobs.no_level0) return false;
        const uint32_t span = ranges[0].span;
        if (span == 0 || (span & (span - 1))) return false;
        for (size_t i = 0; i < R; ++i)
            if (ranges[i].span != span || ranges[i].lo != (uint32_t)(i * (uint64_t)span)) return false;
        if ((uint64_t)span * R != (1ull << 32)) return false;
        const bool verbose = knobs.verbose, has_val = in.vals != nullptr;
        // ranges per chunk: the largest power of two whose chunks all stay below the pass's 32-bit offsets
        size_t m = R;
        for (; m > 1; m >>= 1) {
            bool fits = true;
            for (size_t c = 0; c < R && fits; c += m) {
                uint64_t t = 0;
                for (size_t j = 0; j < m; ++j) t += ranges[c + j].est;
                fits = t < (3500ull << 20);
            }
            if (fits) break;
        }
        if (m < 2) return false;
        int jbits = 0;
        while ((1u << jbits) < m) ++jbits;
        const uint64_t Ntot = expand_k ? 2 * in.n : in.n;  // instance space of the level-0 tiles
        const uint64_t nt = (Ntot + kPartTileK - 1) / kPartTileK;
        if (nt >= (1ull << 32)) return false;
        const unsigned ek = expand_k;
        const bool et = expand_tag;
        // every range: an ordinary key array (its records are what the expansion generated)
        expand_k = 0;
        expand_tag = false;
        for (size_t c = 0; c < R; c += m) {
            std::vector<uint32_t> off(m + 1, 0);
            for (size_t j = 0; j < m; ++j) off[j + 1] = off[j] + (uint32_t)ranges[c + j].est;
            const uint64_t nc = off[m];
            if (nc == 0) continue;
            const double t0 = wall();
            DevBuf buf0(nc * rec + 16), val0, cur(m * 4 + 16);
            if (has_val) val0.alloc(nc * 4 + 16);
            BBK_HIP(hipMemcpyAsync(cur.p, off.data(), m * 4, hipMemcpyHostToDevice, ctx->stream));
            Sel cs;
            cs.lo = ranges[c].lo;
            const uint64_t cspan = (uint64_t)span * m;
            if (cspan < (1ull << 32)) {
                cs.span = (uint32_t)cspan;
                cs.finish();
            }
            PartLevel L0{1, jbits, (uint32_t)m, dmode, w0bits(), nullptr, nullptr, cs.lo, cs.span, cs.shl, cs.mul};
            TileMap M0{nullptr, nullptr, nullptr, 1, Ntot, 0, 1, nullptr, (int)ek, et ? 1 : 0};
            const double pb = (double)(ek ? in.n : Ntot) * (rec + (has_val ? 4 : 0)) + (double)nc * (rec + (has_val ? 4 : 0));
            scatter_keys<true>(has_val, "k_part_l0", pb, (uint32_t)nt, (const Key<W> *)in.keys, in.vals, M0, L0, cur.as<uint32_t>(),
                         buf0.as<Key<W>>(), val0.as<uint32_t>());
            std::vector<uint32_t> end(m);
            BBK_HIP(hipMemcpyAsync(end.data(), cur.p, m * 4, hipMemcpyDeviceToHost, ctx->stream));
            stream_wait(ctx);
            for (size_t j = 0; j < m; ++j)
                BBK_REQUIRE(end[j] == off[j + 1], BBK_ERR_INTERNAL, "level 0: range %zu received %u records, planned %u", c + j,
                            end[j] - off[j], off[j + 1] - off[j]);
            if (verbose) fprintf(stderr, "[bbk] level 0: %llu records into %zu ranges: %.3f s\n", (unsigned long long)nc, m, wall() - t0);
            for (size_t j = 0; j < m; ++j) {
                const Sel &sr = ranges[c + j];
                if (sr.est == 0) continue;
                MsdOutput part;
                Dst dst{out.keys.as<char>() + D * rec, out.vals.p ? out.vals.as<uint32_t>() + D : nullptr};
                const double t1 = wall();
                // ranges of an expanded (both-strand) input spread as evenly as the whole: the key slots of the ordering
                // pass apply (no histogram passes, XCD-local fill fronts); should they not hold, the exact mode redoes it
                even_part = ek != 0 && !knobs.no_part_kslots;
                const MsdInput ri{nullptr, buf0.as<char>() + (size_t)off[j] * rec,
                                  has_val ? val0.as<uint32_t>() + off[j] : nullptr, sr.est, false};
                const Outcome rv = run_retrying(ri, part, sr, dst);
                even_part = false;
                if (verbose) fprintf(stderr, "[bbk] key range (materialised): %.3f s\n", wall() - t1);
                BBK_REQUIRE(rv == Outcome::Done, BBK_ERR_INTERNAL, "a materialised range did not sort (%d)", (int)rv);
                D += part.n;
                inst += part.instances;
            }
        }
        return true;
    }

    // KEYS / REF prefix: the ranges are consecutive in prefix order and every pass writes straight into one array
    // (upper bound: every record distinct, which is the usual case -- stage B sorts a distinct set)
    bool run_key_ranges(const MsdInput &in, uint64_t Nrec, const std::vector<Sel> &ranges, MsdOutput &out) {
        const bool out_vals = op != MSD_OP_NONE;
        out.keys.alloc(Nrec * rec + 16);
        if (out_vals) out.vals.alloc(Nrec * 4 + 16);
        uint64_t D = 0, inst = 0;
        if (!level0_ranges(in, ranges, out, D, inst)) {
            D = 0;
            inst = 0;
            for (const Sel &sr : ranges) {
                if (sr.est == 0) continue;
                MsdOutput part;
                Dst dst{out.keys.as<char>() + D * rec, out_vals ? out.vals.as<uint32_t>() + D : nullptr};
                const double t0 = wall();
                const Outcome rv = Pass(*this, in, part, sr, dst).run();
                if (knobs.verbose) fprintf(stderr, "[bbk] key range: %.3f s\n", wall() - t0);
                if (rv != Outcome::Done) return false;
                D += part.n;
                inst += part.instances;
            }
        }
        BBK_REQUIRE(inst == Nrec, BBK_ERR_INTERNAL, "range passes saw %llu of %llu records", (unsigned long long)inst,
                    (unsigned long long)Nrec);
        out.n = D;
        out.instances = Nrec;
        out.nbuckets = 0;
        return true;
    }

    // HASH prefix: every hash range is deduplicated on its own (disjoint key sets) and the distinct records are
    // concatenated
    bool run_hash_ranges(const MsdInput &in, const std::vector<Sel> &ranges, MsdOutput &out) {
        const bool out_vals = op != MSD_OP_NONE;
        std::vector<MsdOutput> parts(ranges.size());
        uint64_t D = 0, inst = 0;
        for (size_t v = 0; v < ranges.size(); ++v) {
            MsdOutput &pt = parts[v];
            const double t0 = wall();
            const Outcome rv = run_retrying(in, pt, ranges[v]);
            if (knobs.verbose) fprintf(stderr, "[bbk] hash range %zu/%zu: %.3f s\n", v + 1, ranges.size(), wall() - t0);
            if (rv != Outcome::Done) return false;
            D += pt.n;
            inst += pt.instances;
            pt.bucket_off.release();
            // the slot mode sizes a part for the worst case (every record distinct): keep what is used
            if (pt.keys.bytes > pt.n * rec + (64u << 20)) {
                DevBuf ek(pt.n * rec + 16), ev;
                BBK_HIP(bbk::copy_async(ek.p, pt.keys.p, pt.n * rec, hipMemcpyDeviceToDevice, ctx->stream));
                if (out_vals) {
                    ev.alloc(pt.n * 4 + 16);
                    BBK_HIP(bbk::copy_async(ev.p, pt.vals.p, pt.n * 4, hipMemcpyDeviceToDevice, ctx->stream));
                }
                stream_wait(ctx);
                pt.keys = std::move(ek);
                if (out_vals) pt.vals = std::move(ev);
            }
        }
        out.n = D;
        out.instances = inst;
        out.keys.alloc(D * rec + 16);
        if (out_vals) out.vals.alloc(D * 4 + 16);
        uint64_t o = 0;
        for (auto &p : parts) {
            if (p.n) {
                BBK_HIP(bbk::copy_async(out.keys.as<char>() + o * rec, p.keys.p, p.n * rec, hipMemcpyDeviceToDevice,
                                       ctx->stream));
                if (out_vals)
                    BBK_HIP(bbk::copy_async(out.vals.as<uint32_t>() + o, p.vals.p, p.n * 4, hipMemcpyDeviceToDevice,
                                           ctx->stream));
            }
            o += p.n;
            stream_wait(ctx);
            p.keys.release();  // hand the part back before the next copy: peak = result + one part
            p.vals.release();
        }
        out.nbuckets = 0;
        return true;
    }

    // run() plus the split into ranges of the prefix space when the input holds more records than one pass takes
    // (what the reference does with bounded buffers, repeated DumpBuffers rounds and the run merge,
    // kmer_splitter.hpp:73-167, kmer_index_builder.hpp:281-365).
    MsdInput dense_of(const MsdInput &in) {
        if (!in.view) return in;
        in.view->materialise(ctx);  // (no-op once the dense array exists)
        BBK_REQUIRE(in.view->keys.p, BBK_ERR_INTERNAL, "bucket view neither live nor materialised");
        MsdInput d = in;
        d.keys = in.view->keys.p;
        d.view = nullptr;
        return d;
    }

    bool run_all(const MsdInput &in0, MsdOutput &out) {
        uint64_t Nrec = 0;  // records of the whole input, when it is too big for one pass
        const Outcome r = run_retrying(in0, out, Sel(), Dst(), &Nrec);
        if (r != Outcome::TooBig) return r == Outcome::Done;
        const MsdInput in = dense_of(in0);
        std::vector<Sel> ranges;
        if (!plan_ranges(in.rd, in.keys, Nrec, ranges)) return false;
        return dmode == MSD_HASH ? run_hash_ranges(in, ranges, out) : run_key_ranges(in, Nrec, ranges, out);
    }
};

#ifdef BBK_PHASE_PROF
static void dump_phases() {
    unsigned long long h[6][8];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_phase), sizeof(h)) != hipSuccess) return;
    static const char *kinds[6] = {"scatter1_reads", "scatter1_keys", "scatter2", "bucket_dist", "bucket_hash",
                                   "scatter1_narrow"};
    for (int q = 0; q < 6; ++q) {
        if (!h[q][7]) continue;
        fprintf(stderr, "[bbk phase] %-15s wgs=%llu cycles/wg:", kinds[q], h[q][7]);
        for (int p = 0; p < 7; ++p) fprintf(stderr, " p%d=%.0f", p, (double)h[q][p] / (double)h[q][7]);
        fprintf(stderr, "\n");
    }
    memset(h, 0, sizeof(h));
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_phase), h, sizeof(h));
}
#endif

template <int W>
static bool msd_run(bbk_ctx *ctx, unsigned k, int dmode, int op, const MsdInput &in, MsdOutput &out, bool assume_distinct,
                    unsigned expand_k, bool expand_tag = false, uint64_t strip_mask = ~0ull) {
    return MsdRunner<W>{ctx, k, dmode, op, strip_mask, assume_distinct, expand_k, expand_tag}.run_all(in, out);
}

bool msd_sort_reduce(bbk_ctx *ctx, unsigned k, int dmode, int op, const bbk_reads *rd, const void *d_keys,
                     const uint32_t *d_vals, uint64_t n, bool with_mask, MsdOutput &out, unsigned tag_bits,
                     bool assume_distinct, unsigned expand_k, BucketView *view) {
    BBK_REQUIRE(!view || (!d_keys && !d_vals && !rd && expand_k && n == view->n() && (view->live() || view->keys.p)),
                BBK_ERR_INTERNAL, "bucket view input: expanded canonical keys only");
    MsdInput in{rd, d_keys, d_vals, n, with_mask};
    if (view && !view->live()) in.keys = view->keys.p;  // already dense
    else in.view = view;
    if (tag_bits) {
        // the tag sits right above the k-mer (bits [2k, 2k + tag_bits)): sort as a (k + tag_bits/2)-mer, clear the
        // tag on the way out
        BBK_REQUIRE(words_of(k) == 1 && rd == nullptr && dmode == MSD_KEYS && tag_bits % 2 == 0 && 2 * k + tag_bits <= 64 &&
                        (expand_k == 0 || expand_k == k),
                    BBK_ERR_INTERNAL, "tagged sort needs 8-byte keys with %u spare bits", tag_bits);
        return msd_run<1>(ctx, k + tag_bits / 2, dmode, op, in, out, assume_distinct, expand_k, expand_k != 0,
                          (2 * k >= 64) ? ~0ull : ((1ull << (2 * k)) - 1ull));
    }
#ifdef BBK_PHASE_PROF
    struct Dump {
        ~Dump() { dump_phases(); }
    } dump_on_exit;
#endif
    switch (words_of(k)) {
        case 1: return msd_run<1>(ctx, k, dmode, op, in, out, assume_distinct, expand_k);
        case 2: return msd_run<2>(ctx, k, dmode, op, in, out, assume_distinct, expand_k);
        case 3: return msd_run<3>(ctx, k, dmode, op, in, out, assume_distinct, expand_k);
        case 4: return msd_run<4>(ctx, k, dmode, op, in, out, assume_distinct, expand_k);
    }
    return false;
}

}  // namespace bbk
