// msd.h -- interface of the MSD-partition + in-LDS sort path (msd.hip).
#pragma once

#include "bbk_internal.h"

namespace bbk {

enum { MSD_HASH = 0, MSD_KEYS = 1, MSD_REF = 2 };                      // partition prefix
enum { MSD_OP_NONE = 0, MSD_OP_COUNT = 1, MSD_OP_SUM = 2, MSD_OP_OR = 3 };  // per-key reduction

// Stage A's narrow distinct set left where the dedup kernel wrote it, instead of the dense 8-byte array
// (MsdOutput::want_view): bucket b's distinct records are the 4-byte low words at the head of its level-2 slot,
// slots[b * stride .. + count), and their high bits come from the bucket's level-1 segment (nw_key).  off is the
// exclusive scan of the counts, so key c of the dense order is in the bucket b with off[b] <= c < off[b + 1].  The
// records of the overflow path (already 8-byte keys) follow as `extra`.  Stage B's level 1 reads it as it stands
// (MsdRequest::expand of the view); every other consumer calls materialise() first.
struct BucketView {
    DevBuf slots;   // u32 [nbuckets * stride]
    DevBuf dcount;  // u32 [nbuckets]: distinct records per bucket (0xFFFFFFFF: none here, see extra)
    DevBuf off;     // u64 [nbuckets + 1]: exclusive scan of dcount
    DevBuf seg;     // u16 [nbuckets]: level-1 segment of every bucket
    DevBuf extra;   // u64 [n_extra]
    uint32_t nbuckets = 0, stride = 0;
    int hb = 0;     // key bits above the low word
    uint64_t D = 0, n_extra = 0;
    DevBuf keys;    // the dense array, once materialised
    bool live() const { return slots.p != nullptr; }
    uint64_t n() const { return D + n_extra; }
    void release_slots() {
        slots.release();
        dcount.release();
        off.release();
        seg.release();
        extra.release();
    }
    // the dense array of n() 8-byte keys into `keys` (what stage A's compaction writes); the slots are released
    void materialise(bbk_ctx *ctx);
};

struct MsdOutput {
    DevBuf keys;        // distinct records: bucket-major in prefix order, ascending inside a bucket
    DevBuf vals;        // reduced payload (op != NONE)
    DevBuf bucket_off;  // nbuckets + 1 offsets into keys
    uint64_t n = 0;
    uint64_t instances = 0;
    uint64_t overflow_buckets = 0;
    uint32_t nbuckets = 0;
    // caller: a narrow stage-A pass may leave its result as `view` (keys then stay empty); the pass decides
    bool want_view = false;
    BucketView view;
};

// What msd_sort_reduce is asked to sort + reduce: the partition prefix, the per-key reduction and ONE input, built by
// the named constructor of that input (so a view never goes with anything but an expanded set); tag_bits and
// assume_distinct are set on the result where they apply.
struct MsdRequest {
    int prefix = MSD_HASH;  // MSD_HASH / MSD_KEYS / MSD_REF; MSD_KEYS output is globally ascending
    int op = MSD_OP_NONE;
    const bbk_reads *rd = nullptr;  // reads: canonical k-mers are extracted on the fly ...
    bool with_mask = false;         // ... with the InOutMask bits of every occurrence as payload
    const void *keys = nullptr;     // a record array: keys[, vals], n
    const uint32_t *vals = nullptr;
    uint64_t n = 0;
    // expand_k = k: the array holds n CANONICAL k-mers and the records are generated on the fly -- 2n of them: every key
    // and its reverse complement, with the tag of tag_bits (the XXH3 bucket of 16) written by the level-1 kernels
    // themselves
    unsigned expand_k = 0;
    // ... or the canonical array is a live BucketView (n = view->n(), no payload).  The key-slot level 1 reads it in
    // place and releases its slots; a pass that needs the dense array materialises it, and a key-slot give-up after the
    // slots are gone rebuilds it from the level-1 records.  view->keys may hold the dense array after the call.
    BucketView *view = nullptr;
    // > 0 (8-byte keys, key array input, MSD_KEYS): bits [2k, 2k + tag_bits) of every key hold a tag that is more
    // significant than the k-mer (the caller put it there, or the expansion does); the records are ordered by
    // (tag, k-mer) and the tag is cleared in the output
    unsigned tag_bits = 0;
    // key array, KEYS / REF prefix: the caller expects no duplicates, so the sorted result is written directly at the
    // offsets of the input (no compaction pass); verified on the fly, redone in place otherwise
    bool assume_distinct = false;

    static MsdRequest reads(int prefix, int op, const bbk_reads *rd, bool with_mask) {
        MsdRequest r;
        r.prefix = prefix, r.op = op, r.rd = rd, r.with_mask = with_mask;
        return r;
    }
    static MsdRequest records(int prefix, int op, const void *keys, const uint32_t *vals, uint64_t n) {
        MsdRequest r;
        r.prefix = prefix, r.op = op, r.keys = keys, r.vals = vals, r.n = n;
        return r;
    }
    static MsdRequest expand(int prefix, int op, unsigned k, const void *canon, const uint32_t *vals,
                             uint64_t n) {
        MsdRequest r = records(prefix, op, canon, vals, n);
        r.expand_k = k;
        return r;
    }
    static MsdRequest expand(int prefix, int op, unsigned k, BucketView &view) {
        MsdRequest r = expand(prefix, op, k, nullptr, nullptr, view.n());
        r.view = &view;
        return r;
    }
};

// Sort + reduce the records of `rq` (k-mer size k).  Returns false when this path declines (key width, size, too much
// overflow): the caller then uses the LSD path.
bool msd_sort_reduce(bbk_ctx *ctx, unsigned k, const MsdRequest &rq, MsdOutput &out);

// superk.hip: stage A of a batch of reads for 16- and 24-byte keys through super-k-mer records (distinct canonical
// k-mers + count / OR of edge masks, in any order).  false: not taken or given up -- use msd_sort_reduce.
bool superk_dedup_reads(bbk_ctx *ctx, const bbk_reads *rd, unsigned k, int op, DevBuf &out_keys, DevBuf &out_vals,
                        uint64_t &n_distinct, uint64_t &n_instances);

// superk.hip, for the test export of the read plan (bbk_read_plan): the segment length the path uses at k (0: k is not
// for it) and the segments of a level-1 tile; superk_plan_tiles is the path's own launch of its tile kernel (SkTile:
// r0, nr, for the n_tiles tiles of `tile` segments over the ReadPlan's coff / n_segs, into `tiles`)
uint32_t superk_segment_len(unsigned k);
uint32_t superk_tile_segments();
void superk_plan_tiles(bbk_ctx *ctx, const uint64_t *coff, uint64_t n_reads, uint64_t n_segs, uint32_t tile,
                       uint64_t n_tiles, DevBuf &tiles);

}  // namespace bbk
