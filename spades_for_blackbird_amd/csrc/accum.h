// accum.h -- accumulator behind the streaming entry points (bbk_count_begin / push / finish,
// bbk_extindex_begin / push / finish); defined in count.hip.
#pragma once

#include <vector>

#include "bbk_internal.h"
#include "msd.h"

namespace bbk {

// What the reference gets from bounded per-thread cells, repeated DumpBuffers rounds (one sorted + uniqued run per
// bucket and round, common/utils/kmer_mph/kmer_splitter.hpp:73-167) and the final loser-tree run merge (MergeKMers,
// kmer_index_builder.hpp:281-365): the input never has to be resident as a whole.  Every pushed batch is
// deduplicated on its own (stage A) and kept as a "run" of distinct canonical records; runs are merge-uniqued into
// the accumulated set whenever they outweigh half of it (the total merge work stays linear in the input), and
// finish orders the set once (stage B).
struct Accum {
    bbk_ctx *ctx = nullptr;
    unsigned k = 0;
    bool with_mask = false;  // payload = InOutMask bits (OR) instead of multiplicities (SUM)
    bool want_vals = false;
    // a count whose first batch may leave its distinct set in stage A's buckets (BucketView): both strands, no payload,
    // odd k (stage B then reads the buckets in place)
    bool want_view = false;
    DevBuf keys, vals;       // the accumulated distinct canonical set (any order)
    BucketView view;         // ... or that set still in stage A's buckets (keys empty)
    uint64_t n = 0;
    struct Run {
        DevBuf keys, vals;
        BucketView view;
        uint64_t n = 0;
    };
    std::vector<Run> runs;
    uint64_t runs_n = 0;
    uint64_t instances = 0;  // k-mer positions seen
    uint64_t batches = 0, merges = 0;

    // a count: the payload its BBK_* flags ask for (BBK_WITH_COUNTS / BBK_WITH_MASKS), the view where they allow it
    Accum(bbk_ctx *ctx, unsigned k, unsigned count_flags);
    // an extension index: canonical k-mers with the OR of their InOutMask bits
    static Accum masks(bbk_ctx *ctx, unsigned k) { return Accum(ctx, k, BBK_CANONICAL | BBK_WITH_MASKS); }

    bool has_vals() const;
    int merge_op() const;
    void push(const bbk_reads *rd);
    // a record array already in HBM (keys + payloads, duplicates allowed) becomes one more run
    void push_records(const void *d_keys, const uint32_t *d_vals, uint64_t n_rec);
    void merge();
    void dense();  // every BucketView of the accumulator -> its dense array in keys
    uint64_t finish_sorted(DevBuf &out_keys, DevBuf &out_vals);
};

// count.hip: canon U rc(canon) of the accumulated canonical records as `flags` ask (BBK_BOTH_STRANDS [|
// BBK_REFERENCE_ORDER]).  consume: the accumulator is left empty; otherwise it keeps its records (the extension index
// is built from them afterwards).  carry_payload: the multiplicities travel with the keys.
bbk_kmerset *finish_both_strands(Accum &acc, unsigned flags, bool consume, bool carry_payload);

// kmerfilter.hip: the distinct records (keys, u32 multiplicities in vals; n of them, any order) whose multiplicity is at
// least min_count, in their order, back into keys / vals; returns how many stay.  self_rc_doubles: a k-mer equal to its
// own reverse complement counts twice its payload (what a both-strand set reports for it at even k);
// *dropped_self_rc receives the dropped records of that kind (0 without self_rc_doubles).  Waits for the stream.
uint64_t filter_min_count(bbk_ctx *ctx, unsigned k, bool self_rc_doubles, uint32_t min_count, DevBuf &keys, DevBuf &vals,
                          uint64_t n, uint64_t *dropped_self_rc);

}  // namespace bbk
