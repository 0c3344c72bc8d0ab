// msd_part.h -- the wide route's partition levels: tile geometry, prefix / bin helpers, tile descriptors and the
// scatter / histogram kernels over key arrays (k_part) and packed reads (k_part_reads).  Launched by Pass::level1_tiles,
// level1, level2_layout and level2_scatter (msd.hip); the other routes reuse its PartLevel, TileMap and part_tail.
#pragma once

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
    // different L2s, which is slow (MsdRunner::plan, msd.hip).  With a fill front per (bin, XCD) every line is one XCD's.  Level 2
    // reads the sub-slots as segments of their own and sends them to the buckets of the parent segment.
    int xcd_shift;
    uint32_t sub_cap;
};

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

// largest s in [0, n) with start[s] <= x (start ascending, start[0] <= x): the segment, bucket or read that owns item x
template <class T, class I>
__device__ inline I last_le(const T *start, I n, T x) {
    I lo = 0, hi = n;
    while (hi - lo > 1) {
        const I mid = (lo + hi) >> 1;
        if (start[mid] <= x) lo = mid;
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

// one thread per tile of `tile` chunks (a chunk = ch k-mer positions of one read).  Two tilings of the same reads in
// one launch: threads [0, n_tiles) describe the tiles of `tile` chunks into out, the next n_tiles_b threads those of
// tile_b chunks into out_b (the scatter and the histogram kernels of level 1 have different workgroup sizes).
// coff is the ReadPlan's scan (n_chunks = coff[n_reads]); *unordered is its flag: set when the packed words of the reads
// do not lie one after the other in read order (then no tile stages its window of words in LDS).
__global__ void k_tile_reads(const uint64_t *__restrict__ coff, const uint64_t *__restrict__ woff,
                             const uint32_t *__restrict__ len, uint64_t n_reads, uint64_t n_chunks, uint64_t n_tiles,
                             uint32_t tile, RdTile *__restrict__ out, uint64_t n_tiles_b, uint32_t tile_b,
                             RdTile *__restrict__ out_b, uint32_t ch, uint32_t k, uint32_t max_reads, uint32_t max_words,
                             const uint32_t *__restrict__ unordered) {
    uint64_t t = BBK_GID();
    if (t >= n_tiles) {
        t -= n_tiles;
        if (t >= n_tiles_b) return;
        tile = tile_b;
        out = out_b;
    }
    const uint64_t c0 = t * (uint64_t)tile;
    const uint64_t r0 = read_of_unit(coff, n_reads, n_chunks, c0), r1 = read_of_unit(coff, n_reads, n_chunks, c0 + tile);
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

// level 2: tile -> descriptor (one thread per tile).  M's entries are the level-1 segments or their per-XCD sub-slots
// (sub_shift).  SEG_IN_Z (the 4-byte routes, narrow stage A and the late tag: the record no longer says which segment
// it belongs to): the segment id beside the bin count.
// xstart (optional): the tiles of level-1 segment s are dealt to the workgroups that run on XCD s % 8 (workgroup b runs on
// XCD b % 8): tile i of M-entry e becomes workgroup 8 * (xstart[e] + i) + s % 8.  All tiles that fill the buckets of one
// segment then write through ONE L2 (lines filled from several XCDs are what makes a scatter slow, see MsdRunner::plan in
// msd.hip), and few segments are in flight per XCD at a time.  Unused places keep a zero descriptor (no records).
template <bool SEG_IN_Z>
__global__ void k_tile_desc(TileMap M, const uint32_t *__restrict__ seg_nb2, const uint32_t *__restrict__ seg_bin_start,
                            uint32_t tile_size, int sub_shift, const uint32_t *__restrict__ xstart,
                            uint4 *__restrict__ desc) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= M.ntiles) return;
    const uint32_t e = last_le(M.seg_tile_start, M.nseg, t), i = t - M.seg_tile_start[e];
    const uint32_t b = M.seg_off[e] + i * tile_size;
    const uint32_t end = M.seg_size ? M.seg_off[e] + M.seg_size[e] : M.seg_off[e + 1];
    const uint32_t seg = e >> sub_shift;
    const uint32_t at = xstart ? 8u * (xstart[e] + i) + (seg & 7u) : t;
    desc[at] = make_uint4(b, (end - b) < tile_size ? (end - b) : tile_size, seg_nb2[seg] | (SEG_IN_Z ? seg << 16 : 0u),
                          seg_bin_start[seg]);
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
            const uint32_t ri = last_le(s_rel, nr, (int32_t)tid);
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

}  // namespace bbk
