// msd.hip -- the fast sort-and-count path: two MSD radix-partition levels in HBM, then one
// workgroup per bucket deduplicates / sorts + reduces its keys entirely in LDS.
//
// Why: the LSD path (sort.hip) moves every record 3x per 8-bit pass (k=21: 6 passes, ~19 N*W
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
// This file is the path's one translation unit: it holds the host side (MsdKnobs, MsdRunner with Plan / Pass, the range
// passes, the entry points).  The kernels sit in headers that nothing else includes, one per kernel family: msd_part.h
// (partition levels), msd_bucket.h (buckets in LDS, compaction), msd_narrow_a.h (stage A's 4-byte records),
// msd_stage_b.h (stage B: 4-byte records, BucketView level 1, late tag).
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
#include <utility>
#include <vector>

#include "bbk_internal.h"
#include "kmer_ops.h"
#include "msd.h"
#include "msd.h"

#include "msd_part.h"
#include "msd_bucket.h"
#include "msd_narrow_a.h"
#include "msd_stage_b.h"

namespace bbk {

// ------------------------------------------------------------------------------------------
// host orchestration
// ------------------------------------------------------------------------------------------
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

// Records of a call: reads (rd, see MsdRequest) or a key array (keys[, vals], n)
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

// The one launch of k_tile_reads (level1_tiles, and the test export of the read plan): the n_a tiles of tile_a chunks
// into out_a and, where n_b is not 0, the n_b tiles of tile_b chunks into out_b, over the ReadPlan's coff / n_chunks
static void launch_tile_reads(bbk_ctx *ctx, const bbk_reads *rd, const uint64_t *coff, uint64_t n_chunks, uint64_t n_a,
                              uint32_t tile_a, RdTile *out_a, uint64_t n_b, uint32_t tile_b, RdTile *out_b, uint32_t ch,
                              uint32_t k, const uint32_t *unordered) {
    if (n_a + n_b == 0) return;
    launch_items(ctx, "k_tile_reads", k_tile_reads, n_a + n_b, coff, rd->d_woff, rd->d_len, rd->n, n_chunks, n_a, tile_a,
                 out_a, n_b, tile_b, out_b, ch, k, (uint32_t)kRdSlots, (uint32_t)kRdWords, unordered);
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
    // an untimed planning kernel: one thread per item, 256 per workgroup
    template <class K, class... Args>
    void launch_plan(K fn, const char *name, uint64_t n_items, Args... args) {
        hipLaunchKernelGGL(fn, bbk::grid_blocks((n_items + 255) / 256), dim3(256), 0, ctx->stream, args...);
        check_launch(name);
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
            // one fused scan over the read lengths, both totals in one wait; coff[n] = n_chunks is written by the scan
            ReadPlan rp;
            rp.run(ctx, rd, R.k, (unsigned)RdCfg<W>::CH, ctl_at(kCtlUnordered));
            coff = std::move(rp.coff);
            N = rp.kmers;
            n_chunks = rp.units;
        }

        // ---- level-1 tiles (reads) and the slot layout
        void level1_tiles() {
            L1 = PartLevel{1, P.b1, P.nb1, R.dmode, R.w0bits(), nullptr, nullptr, sel.lo, sel.span, sel.shl, sel.mul};
            if (from_reads) {
                const bbk_reads *rd = in.rd;
                // (the histogram tiling is read by the exact mode alone: slot mode has no histogram pass)
                const uint64_t nth = P.slots ? 0 : P.ntiles1h;
                tile_read.alloc(((size_t)P.ntiles1 + 1) * sizeof(RdTile));
                tiles_h.alloc(((size_t)nth + 1) * sizeof(RdTile));
                if (P.ntiles1)
                    launch_tile_reads(ctx, rd, coff.as<uint64_t>(), n_chunks, P.ntiles1, P.rd_tile, tile_read.as<RdTile>(),
                                      nth, (uint32_t)kRdHistThreads, tiles_h.as<RdTile>(), (uint32_t)RdCfg<W>::CH, R.k,
                                      ctl_at(kCtlUnordered));
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
            bufA.alloc(nA * P.rec_ab + 16);  // (+ 16: k_part_narrow2 loads a tile's records four at a time, tile_rows4)
            if (has_val) valA.alloc(nA * 4 + 16);
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
                else if (in.view) {
                    if constexpr (W == 1) level1_from_view();
                } else
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

        // The methods from here to rebuild_view exist for 8-byte keys only: each is called under if constexpr (W == 1).

        // tiles of keys_per_tile canonical keys over the view's buckets: per tile, the buckets of its first and last key
        std::pair<DevBuf, uint32_t> view_tiles(BucketView &v, uint32_t keys_per_tile) {
            const uint32_t nt = (uint32_t)((v.D + keys_per_tile - 1) / keys_per_tile);
            DevBuf desc;
            if (nt) {
                desc.alloc((size_t)nt * sizeof(uint2) + 16);
                R.launch_plan(k_view_tile_desc, "k_view_tile_desc", nt, v.off.as<uint64_t>(), v.nbuckets, v.D, keys_per_tile,
                              nt, desc.as<uint2>());
            }
            return {std::move(desc), nt};
        }

        // level 1 of the key slots over a BucketView: the buckets' keys, then the overflow path's (dense) into the same
        // slots and cursors
        void level1_from_view() {
            BucketView &v = *in.view;
            if (P.late_tag) {
                level1_late_tag(v);
                return;
            }
            const auto [vdesc, nt] = view_tiles(v, kPartTileK / 2);
            if (nt) {
                TileMap Mv = M1;
                Mv.n = 2 * v.D;
                Mv.ntiles = nt;
                R.launch(R.expand_tag ? k_part_view<true> : k_part_view<false>, "k_part_view",
                         (double)v.D * 4 + 2.0 * (double)v.D * rec, nt, PartCfg<1>::THREADS, part_view_smem(),
                         v.slots.as<uint32_t>(), v.off.as<uint64_t>(), v.seg.as<uint16_t>(), vdesc.template as<uint2>(),
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

        // level 1 with the tag taken late: 4-byte records into 1024 key-prefix segments (k_part_view_lt), from the
        // buckets and from the overflow path's dense keys
        void level1_late_tag(BucketView &v) {
            constexpr uint32_t kpt = (uint32_t)kLtThreads * kLt1Items / 2;
            const size_t lds = lt_smem(kLt1Items, lt_view_tables());
            ctx->add_stat("stat_late_tag", (double)N);
            const auto [vdesc, nt] = view_tiles(v, kpt);
            if (nt)
                R.launch(k_part_view_lt<false>, "k_part_l1", (double)v.D * 4 + 2.0 * (double)v.D * 4, nt, kLtThreads, lds,
                         v.slots.as<uint32_t>(), v.off.as<uint64_t>(), v.seg.as<uint16_t>(), vdesc.template as<uint2>(),
                         v.stride, v.hb, (const uint64_t *)nullptr, v.D, (int)R.expand_k, L1, cur1.as<uint32_t>(),
                         bufA.as<uint32_t>());
            if (v.n_extra) {
                const uint32_t nte = (uint32_t)((v.n_extra + kpt - 1) / kpt);
                R.launch(k_part_view_lt<true>, "k_part_l1", (double)v.n_extra * 8 + 2.0 * (double)v.n_extra * 4, nte,
                         kLtThreads, lds, (const uint32_t *)nullptr, (const uint64_t *)nullptr, (const uint16_t *)nullptr,
                         (const uint2 *)nullptr, 0u, 0, v.extra.as<uint64_t>(), v.n_extra, (int)R.expand_k, L1,
                         cur1.as<uint32_t>(), bufA.as<uint32_t>());
            }
        }

        // a key-slot give-up after level 1 released the view's buckets: the canonical keys again, from level 1's records
        Outcome give_up_key_slots() {
            if constexpr (W == 1)
                if (in.view && !in.view->live() && !in.view->keys.p) rebuild_view();
            return Outcome::KeySlotsGaveUp;
        }

        void rebuild_view() {
            BucketView &v = *in.view;
            const uint64_t n = v.n();
            v.keys.alloc(n * rec + 16);
            DevBuf cnt(16);
            BBK_HIP(hipMemsetAsync(cnt.p, 0, 16, ctx->stream));
            // (one workgroup per level-1 sub-slot: not launch_plan's geometry)
            if (P.late_tag) {
                ctx->add_stat("stat_late_tag_recanon", (double)n);
                hipLaunchKernelGGL(k_view_recanon_lt, dim3(P.nsub), dim3(256), 0, ctx->stream, bufA.as<uint32_t>(), seg_off,
                                   seg_size, P.xs, (int)R.expand_k, v.keys.as<uint64_t>(), n, cnt.as<uint32_t>());
            } else {
                hipLaunchKernelGGL(k_view_recanon, dim3(P.nsub), dim3(256), 0, ctx->stream, bufA.as<uint64_t>(), seg_off,
                                   seg_size, (int)R.expand_k, v.keys.as<uint64_t>(), n, cnt.as<uint32_t>());
            }
            check_launch("k_view_recanon");
            uint32_t got = 0;
            BBK_HIP(hipMemcpyAsync(&got, cnt.p, 4, hipMemcpyDeviceToHost, ctx->stream));
            stream_wait(ctx);
            BBK_REQUIRE(got == n, BBK_ERR_INTERNAL, "canonical keys rebuilt from level 1: %u of %llu", got,
                        (unsigned long long)n);
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
            if (P.narrow && verbose) {  // the tiles by size: whole ones, and the last one of a sub-slot by the groups of
                                        // four records per lane (4096 records) it reaches -- what tile_rows4 walks
                uint32_t whole = 0, part[3] = {0, 0, 0}, largest = 0;
                for (uint32_t s2 = 0; s2 < nsub; ++s2) {
                    const uint32_t rest = hsub[s2] % tile2;
                    whole += hsub[s2] / tile2;
                    if (rest) ++part[(rest - 1) / (4u * kNw2Threads)];
                    largest = std::max(largest, hsub[s2]);
                }
                fprintf(stderr, "[bbk] msd level-2 tiles (narrow records): whole=%u groups1=%u groups2=%u groups3=%u largest_sub_slot=%u\n",
                        whole, part[0], part[1], part[2], largest);
            }
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
            // level 2: workgroups dealt to the XCDs by segment (k_tile_desc's xstart); BBK_XCD_TILES=0: A/B
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
                // (the 4-byte records of narrow stage A and of the late tag do not say which segment they belong to)
                R.launch_plan((P.narrow || P.late_tag) ? k_tile_desc<true> : k_tile_desc<false>, "k_tile_desc", ntiles2, M2,
                              seg_nb2, seg_bin, tile2, xs, (const uint32_t *)xstart_d, desc2.as<uint4>());
            }
            M2.desc = desc2.as<uint4>();
            // exact mode: the histogram kernel walks 16 consecutive tiles per workgroup and wants them in plain order
            if (!P.slots && xstart_d && !P.narrow) {
                desc2h.alloc((size_t)ntiles2 * sizeof(uint4) + 16);
                R.launch_plan(k_tile_desc<false>, "k_tile_desc", ntiles2, M2, seg_nb2, seg_bin, kPartTileK, xs,
                              (const uint32_t *)nullptr, desc2h.as<uint4>());
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
                R.launch_plan(k_u32_to_u64, "k_u32_to_u64", nbuckets, hist2.as<uint32_t>(), (uint64_t)nbuckets,
                              h64.as<uint64_t>(), 0u);
                const uint64_t tot = exclusive_scan_u64(ctx, h64.as<uint64_t>(), h64.as<uint64_t>(), nbuckets);
                BBK_REQUIRE(tot == N, BBK_ERR_INTERNAL, "level-2 histogram does not add up");
                R.launch_plan(k_scan_to_u32, "k_scan_to_u32", (uint64_t)nbuckets + 1, h64.as<uint64_t>(), (uint64_t)nbuckets,
                              tot, (const uint64_t *)nullptr, boff.as<uint32_t>());
                BBK_HIP(bbk::copy_async(hist2.p, boff.p, (size_t)nbuckets * 4, hipMemcpyDeviceToDevice, ctx->stream));
                stream_wait(ctx);
            } else {
                // cursor of bucket g starts at its slot; narrow path: the segment of every bucket, for the dedup kernel
                if (P.narrow) bseg.alloc(((size_t)nbuckets + 1) * 2);
                R.launch_plan(k_bucket_init, "k_bucket_init", nbuckets, hist2.as<uint32_t>(), nbuckets, P.stride2,
                              (const uint32_t *)seg_bin, P.nb1, P.narrow ? bseg.as<uint16_t>() : (uint16_t *)nullptr);
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
                    bbase.alloc(((size_t)nbuckets + 1) * 8);
                    bperm.alloc(((size_t)nbuckets + 1) * 4);
                    pfill.alloc(((size_t)nbuckets + 1) * 4);
                    R.launch_plan(k_bucket_base_lt, "k_bucket_base_lt", nbuckets, (const uint32_t *)seg_nb2,
                                  (const uint32_t *)seg_bin, P.nb1, nbuckets, 2 * (int)R.expand_k - 10, (int)R.expand_k,
                                  bbase.as<uint64_t>(), bperm.as<uint32_t>());
                    R.launch_plan(k_lt_fill_perm, "k_lt_fill_perm", nbuckets, hist2.as<uint32_t>(), bperm.as<uint32_t>(),
                                  nbuckets, P.stride2, P.cap2, pfill.as<uint32_t>());
                    const ScanSrc src{pfill.p, SCAN_U32_FLAGGED, 0u, 0u};
                    exclusive_scan_enqueue(ctx, 1, &src, &so, nbuckets, ctl_total(), false, scan_keep);
                    R.launch_plan(k_lt_unperm, "k_lt_unperm", nbuckets, c64.as<uint64_t>(), bperm.as<uint32_t>(), nbuckets,
                                  slot_off.as<uint32_t>());
                } else {
                    const ScanSrc src{hist2.p, SCAN_SLOT_FILL, P.stride2, P.cap2};
                    exclusive_scan_enqueue(ctx, 1, &src, &so, nbuckets, ctl_total(), false, scan_keep);
                    R.launch_plan(k_scan_to_u32, "k_scan_to_u32", (uint64_t)nbuckets + 1, c64.as<uint64_t>(),
                                  (uint64_t)nbuckets, 0ull, (const uint64_t *)ctl_total(), slot_off.as<uint32_t>());
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
                        if (!P.late_tag)
                            R.launch_plan(k_bucket_base, "k_bucket_base", nbuckets, (const uint32_t *)seg_nb2,
                                          (const uint32_t *)seg_bin, P.nb1, nbuckets, P.b1, R.w0bits(), bbase.as<uint64_t>());
                        constexpr int NT = BktCfg<1>::NT, IT = BktCfg<1>::ITEMS;
                        // (16-byte loads of a bucket's rows where every bucket starts on a 16-byte boundary: its slots)
                        const bool wide = A.slot_cap != 0 && A.slot_stride % 4 == 0;
                        R.launch(wide ? k_bucket_dist_nb<NT, IT, true> : k_bucket_dist_nb<NT, IT, false>, "k_bucket_dist",
                                 (double)N * (4 + rec), nbuckets, NT, bucket_dist_nb_smem<NT, IT>(), bufB.as<uint32_t>(),
                                 bbase.as<uint64_t>(), A);
                    }
                }
            } else {
                R.template bucket_dispatch<false>(nbuckets, bufB.as<Key<W>>(), valB.as<uint32_t>(), A, rec_bytes(N));
            }
        }

        void fetch_flags() {
            uint32_t *d_flag_n = P.slots ? ctl_at(kCtlSpill) + 2 : ctl_at(kCtlFlagN);
            if (!P.slots) BBK_HIP(hipMemsetAsync(d_flag_n, 0, 16, ctx->stream));  // (a withdrawn direct pass counts again)
            R.launch_plan(k_flagged, "k_flagged", nbuckets, dcount.as<uint32_t>(), nbuckets, flag_ids.as<uint32_t>(), kFlagCap,
                          d_flag_n);
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
                    R.launch_plan(k_nw_widen, "k_nw_widen", cnt, (const uint32_t *)ksrc + first, (uint32_t)cnt, (uint32_t)seg,
                                  P.nw_hb, ek.as<uint64_t>() + o);
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
                                                  out_vals ? ov.as<uint32_t>() : nullptr, rop);
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
                R.launch_plan(k_scan_to_u32, "k_scan_to_u32", (uint64_t)nbuckets + 1, d64.as<uint64_t>(), (uint64_t)nbuckets, D,
                              (const uint64_t *)nullptr, out.bucket_off.as<uint32_t>());
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

bool msd_sort_reduce(bbk_ctx *ctx, unsigned k, const MsdRequest &rq, MsdOutput &out) {
    BucketView *view = rq.view;
    BBK_REQUIRE(!view || (!rq.keys && !rq.vals && !rq.rd && rq.expand_k && rq.n == view->n() && (view->live() || view->keys.p)),
                BBK_ERR_INTERNAL, "bucket view input: expanded canonical keys only");
    MsdInput in{rq.rd, rq.keys, rq.vals, rq.n, rq.with_mask};
    if (view && !view->live()) in.keys = view->keys.p;  // already dense
    else in.view = view;
    if (rq.tag_bits) {
        // the tag sits right above the k-mer (bits [2k, 2k + tag_bits)): sort as a (k + tag_bits/2)-mer, clear the
        // tag on the way out
        BBK_REQUIRE(words_of(k) == 1 && rq.rd == nullptr && rq.prefix == MSD_KEYS && rq.tag_bits % 2 == 0 &&
                        2 * k + rq.tag_bits <= 64 && (rq.expand_k == 0 || rq.expand_k == k),
                    BBK_ERR_INTERNAL, "tagged sort needs 8-byte keys with %u spare bits", rq.tag_bits);
        return msd_run<1>(ctx, k + rq.tag_bits / 2, rq.prefix, rq.op, in, out, rq.assume_distinct, rq.expand_k,
                          rq.expand_k != 0, (2 * k >= 64) ? ~0ull : ((1ull << (2 * k)) - 1ull));
    }
#ifdef BBK_PHASE_PROF
    struct Dump {
        ~Dump() { dump_phases(); }
    } dump_on_exit;
#endif
    bool done = false;
    dispatch_w(words_of(k), [&](auto w) {
        done = msd_run<decltype(w)::value>(ctx, k, rq.prefix, rq.op, in, out, rq.assume_distinct, rq.expand_k);
    });
    return done;
}

}  // namespace bbk

// Exported for the tests only (not declared in bbk.h).  out[10]: chunk length CH of the level-1 kernels at k, chunks of
// a scatter tile, of a histogram tile, of a narrow tile without / with payload, the super-k-mer segment length at k
// (0: not for that path), segments of a super-k-mer tile, reads and packed words a tile may stage in LDS, 0
extern "C" int bbk_read_plan_geometry(unsigned k, uint32_t *out) {
    return bbk::guarded([&] {
        BBK_REQUIRE(out && k >= 1, BBK_ERR_ARG, "bbk_read_plan_geometry: bad argument");
        uint32_t ch = 0;
        bbk::dispatch_w(bbk::words_of(k), [&](auto w) { ch = (uint32_t)bbk::RdCfg<decltype(w)::value>::CH; });
        const uint32_t g[10] = {ch, (uint32_t)bbk::kRdThreads, (uint32_t)bbk::kRdHistThreads,
                                (uint32_t)bbk::NwCfg<false>::CHUNKS, (uint32_t)bbk::NwCfg<true>::CHUNKS,
                                bbk::superk_segment_len(k), bbk::superk_tile_segments(), (uint32_t)bbk::kRdSlots,
                                (uint32_t)bbk::kRdWords, 0u};
        for (int i = 0; i < 10; ++i) out[i] = g[i];
    });
}

// The ReadPlan of `rd` for k-mers of k in units of C, and its tiles of `tile` units: coff (n + 1 values), totals[2] =
// {k-mers, units}, the unordered flag and the descriptors of the ceil(units / tile) tiles (superk = 0: RdTile of the
// level-1 kernels, 24 bytes each; 1: SkTile, 8 bytes) go to the host; tile_cap: tiles the caller's buffer holds
extern "C" int bbk_read_plan(bbk_ctx *ctx, const bbk_reads *rd, unsigned k, unsigned C, unsigned tile, int superk,
                             uint64_t *coff, uint64_t *totals, uint32_t *unordered, void *tiles, uint64_t tile_cap,
                             uint64_t *n_tiles) {
    using namespace bbk;
    return guarded([&] {
        BBK_REQUIRE(ctx && rd && coff && totals && unordered && tiles && n_tiles && k >= 1 && C >= 1 && tile >= 1, BBK_ERR_ARG,
                    "bbk_read_plan: bad argument");
        BBK_HIP(hipSetDevice(ctx->device));
        DevBuf flag(16), td;
        BBK_HIP(hipMemsetAsync(flag.p, 0, 16, ctx->stream));
        ReadPlan rp;
        rp.run(ctx, rd, k, C, flag.as<uint32_t>());
        const uint64_t nt = (rp.units + tile - 1) / tile;
        BBK_REQUIRE(nt <= tile_cap, BBK_ERR_ARG, "bbk_read_plan: %llu tiles, room for %llu", (unsigned long long)nt,
                    (unsigned long long)tile_cap);
        size_t tile_bytes = sizeof(RdTile);
        if (superk) {
            superk_plan_tiles(ctx, rp.coff.as<uint64_t>(), rd->n, rp.units, tile, nt, td);
            tile_bytes = 8;
        } else {
            td.alloc((size_t)(nt + 1) * sizeof(RdTile));
            launch_tile_reads(ctx, rd, rp.coff.as<uint64_t>(), rp.units, nt, (uint32_t)tile, td.as<RdTile>(), 0, (uint32_t)tile,
                              td.as<RdTile>(), (uint32_t)C, (uint32_t)k, flag.as<uint32_t>());
        }
        totals[0] = rp.kmers;
        totals[1] = rp.units;
        *n_tiles = nt;
        d2h_sync(ctx, coff, rp.coff.p, (size_t)(rd->n + 1) * sizeof(uint64_t));
        d2h_sync(ctx, unordered, flag.p, sizeof(uint32_t));
        if (nt) d2h_sync(ctx, tiles, td.p, (size_t)nt * tile_bytes);
    });
}
