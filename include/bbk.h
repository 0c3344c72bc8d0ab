/*
 * bbk.h -- C ABI of the MI355X k-mer counting / de Bruijn graph construction engine.
 *
 * The reference (SPAdes 3.15.4 fork, /root/reference/assembler/src) has no FFI layer; its
 * boundaries for this path are two argv contracts, a C++ operator API and two file formats
 * (SURVEY.md 8b).  Each entry point below names the reference interface it replaces
 * (paths relative to /root/reference/assembler/src).  All functions return 0 on success or a
 * negative bbk_status; the message is available from bbk_last_error() (thread local).
 * No exceptions cross the ABI.  Handles are opaque.  One context per GPU per host thread;
 * a context is not re-entrant (same contract as KMerSortingSplitter, whose per-thread
 * buffers make Split() one-call-at-a-time: common/utils/kmer_mph/kmer_splitter.hpp:111-118).
 *
 * Pointers named d_* must be device (HBM) pointers, h_* host pointers; `dst` pointers of the
 * export calls may be either (hipMemcpyDefault).
 */
#ifndef BBK_H_
#define BBK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bbk_ctx bbk_ctx;
typedef struct bbk_reads bbk_reads;       /* 2-bit packed reads resident in HBM                     */
typedef struct bbk_kmerset bbk_kmerset;   /* sorted distinct k-mers (+ multiplicities) in HBM       */
typedef struct bbk_extindex bbk_extindex; /* sorted canonical k-mers + InOutMask byte each, in HBM  */
typedef struct bbk_unitigs bbk_unitigs;   /* condensed edges + link records (host + device)         */

enum bbk_status {
    BBK_OK = 0,
    BBK_ERR_ARG = -1,      /* bad argument (k out of [1,128), even k for the graph, ...)            */
    BBK_ERR_HIP = -2,      /* a HIP runtime call failed (FATAL_ERROR analogue, utils/logger/logger.hpp:177-190) */
    BBK_ERR_NOMEM = -3,
    BBK_ERR_INTERNAL = -4, /* a device-side invariant failed (VERIFY analogue, utils/verify.hpp)      */
    BBK_ERR_IO = -5
};

#define BBK_MAX_K 128 /* cmake/options.cmake:55-56 SPADES_MAX_K; k must be < BBK_MAX_K */

/* ---- context ---------------------------------------------------------------------------- */
const char *bbk_last_error(void);
const char *bbk_version(void);
int bbk_ctx_create(int device, bbk_ctx **out);
int bbk_ctx_destroy(bbk_ctx *ctx);
/* Run all kernels of this context on an existing hipStream_t (e.g. torch's current stream). */
int bbk_ctx_set_stream(bbk_ctx *ctx, void *hip_stream);
int bbk_ctx_synchronize(bbk_ctx *ctx);
/* Returns device memory the allocator holds but does not use to the driver -- where that is safe: the block-cache
 * allocator (BBK_NO_VMM=1) frees its cached blocks; the default arena allocator keeps its mapped high-water mark for the
 * life of the process (unmapping and re-mapping chunks faults on this platform, see pool.hip). */
int bbk_ctx_trim(bbk_ctx *ctx);
/* Accumulated HIP-event time (ms) and launch count of one named kernel family since the last
 * reset ("extract", "hist", "scan", "scatter", "unique", "expand", "mask", "walk", ...).
 * Timing is only recorded while profiling is enabled (it serialises nothing: events are
 * recorded on the context's stream around each launch). */
int bbk_ctx_profile_enable(bbk_ctx *ctx, int on);
int bbk_ctx_profile_reset(bbk_ctx *ctx);
int bbk_ctx_profile_get(bbk_ctx *ctx, const char *family, double *ms_total, uint64_t *launches,
                        double *bytes_total);
/* Event counters are read the same way (launches = events, bytes_total = summed value): "stat_slot_records",
 * "stat_slot_spilled", "stat_slot_overflow_segments", "stat_slot_overflow_buckets", "stat_slot_reprocessed" -- what the
 * histogram-free slot mode of stage A placed, spilled and had to reprocess (skewed inputs); "stat_host_waits": the times
 * the counting path made the host wait for the stream (launches = waits). */

/* ---- reads: replaces io::EasyStream(file, followed_by_rc=true, handle_Ns=true)
 *      (common/io/reads/io_helper.cpp:19-32) and the binary read cache
 *      (common/io/reads/binary_converter.cpp:50-113) --------------------------------------- */
/* ASCII reads (concatenated; offsets has n+1 entries).  Applies the LongestValid rule
 * (common/io/reads/longest_valid_wrapper.hpp:15-52), accepts ACGTacgt (common/sequence/nucl.hpp:45-62),
 * packs 2 bits/base (A=0 C=1 G=2 T=3, base i in bits 2(i%32) of word i/32, every read starts on
 * a 64-bit word) and uploads.  Reverse complements are NOT materialised: kernels canonicalise. */
int bbk_reads_from_ascii(bbk_ctx *ctx, const char *h_bases, const uint64_t *h_offsets, uint64_t n_reads,
                         bbk_reads **out);
/* Packed reads in HOST memory (what a parser thread of the host produces): read i occupies ceil(len[i]/32) u64
 * words, the reads follow each other in order, each starting on a 64-bit word (the layout above); bits above a
 * read's last base must be zero.  n_words must equal the sum of the per-read word counts.  Uploads (fastest from
 * bbk_host_alloc memory); the word offsets are computed on the device.  The LongestValid rule has already been
 * applied by the caller (one run of ACGTacgt per record, io/reads/longest_valid_wrapper.hpp:15-52). */
int bbk_reads_from_packed(bbk_ctx *ctx, const uint64_t *h_words, uint64_t n_words, const uint32_t *h_len,
                          uint64_t n_reads, bbk_reads **out);
/* Page-locked host memory for the buffers above (host -> device copies from pageable memory run at a fraction of
 * the link rate). */
int bbk_host_alloc(size_t bytes, void **out);
void bbk_host_free(void *p);
/* Adopt packed reads already in HBM (not copied, not freed): d_words[u64], d_word_off[u64, n+1]
 * (first word of each read), d_len[u32, n] (bases). */
int bbk_reads_from_device(bbk_ctx *ctx, const void *d_words, const void *d_word_off, const void *d_len,
                          uint64_t n_reads, uint64_t n_words, bbk_reads **out);
/* Synthetic reads generated on the device: uniform genome of genome_len bases
 * (seed_genome), uniform start, strand flip p=0.5, substitution rate sub_rate (seed_reads). */
int bbk_reads_synth(bbk_ctx *ctx, uint64_t n_reads, uint32_t read_len, uint64_t genome_len, double sub_rate,
                    uint64_t seed_genome, uint64_t seed_reads, bbk_reads **out);
/* Metagenome-shaped synthetic reads (BASELINE configs[4]): n_genomes random genomes with lengths
 * log-uniform in [min_len, max_len] and abundances log-normal(sigma) (sigma = 2: three decades of coverage skew);
 * a read picks its genome with probability ~ abundance x length; read model as bbk_reads_synth.  h_genome_len /
 * h_abundance (optional, n_genomes entries) receive the drawn community. */
int bbk_reads_synth_meta(bbk_ctx *ctx, uint64_t n_reads, uint32_t read_len, uint32_t n_genomes, uint64_t min_len,
                         uint64_t max_len, double sigma, double sub_rate, uint64_t seed, bbk_reads **out,
                         uint64_t *h_genome_len, double *h_abundance);
/* SPAdes binary read cache of single reads (<prefix>.seq / <prefix>.off, io::BinaryWriter::ToBinary,
 * common/io/reads/binary_converter.cpp:50-113; record layout Sequence::BinWrite, common/sequence/sequence.hpp:410-442).
 * Its 2-bit words are exactly the device layout: records are copied, not re-encoded. */
int bbk_reads_from_spades_binary(bbk_ctx *ctx, const char *seq_path, bbk_reads **out);
int bbk_reads_write_spades_binary(bbk_ctx *ctx, const bbk_reads *r, const char *prefix);
uint64_t bbk_reads_count(const bbk_reads *r);
uint64_t bbk_reads_bases(const bbk_reads *r);
/* Copy read i back as ASCII (tests); dst must hold len+1 bytes; returns the length via *len. */
int bbk_reads_get_ascii(bbk_ctx *ctx, const bbk_reads *r, uint64_t i, char *h_dst, uint32_t cap, uint32_t *len);
/* All reads back as ASCII (h_bases may be NULL to query sizes: h_offsets[n] = total bases). */
int bbk_reads_export_ascii(bbk_ctx *ctx, const bbk_reads *r, char *h_bases, uint64_t *h_offsets, uint64_t cap_bases);
void bbk_reads_free(bbk_reads *r);

/* ---- k-mer counting: replaces kmers::KMerDiskCounter<RtSeq>::Count / CountAll
 *      (common/utils/kmer_mph/kmer_index_builder.hpp:195-217,241-279) over a
 *      KMerSortingSplitter (kmer_splitter.hpp:24-52,73-167) ------------------------------- */
#define BBK_BOTH_STRANDS 1u /* spades-kmercount semantics: k-mers of reads and of rc(reads)
                               (projects/kmercount/main.cpp:64-82,106) */
#define BBK_CANONICAL 2u    /* only IsMinimal k-mers (utils/ph_map/storing_traits.hpp:90-101), as the
                               gbuilder splitters use (kmer_splitters.hpp:25-41) */
#define BBK_WITH_COUNTS 4u  /* keep multiplicities (occurrences over reads + rc(reads)).  Multiplicities are u32 and
                               wrap modulo 2^32 on every path, as the reference's uint32_t += does
                               (common/stages/construction.cpp:29, coverage_hash_map_builder.hpp:34-35): counted
                               instances and counts summed by a merge (bbk_kmerset_from_device*, pushed batches)
                               alike, whichever sort path runs; bbk_unitigs_add_coverage_counts reads these values */
#define BBK_UNSORTED 8u     /* distinct set only, internal (hash-bucket) order: enough for the owner partition,
                               bbk_kmerset_both_strands and a later bbk_kmerset_from_device; skips the sort */
#define BBK_REFERENCE_ORDER 16u /* store the set in the final_kmers order (BBK_ORDER_REFERENCE_BUCKETS16) instead of
                                  ascending: what CountAll(16, ..., merge=true) leaves on disk
                                  (projects/kmercount/main.cpp:214-219).  Exporting in that order is then a plain copy
                                  and bbk_kmerset_keys() is the result itself */
#define BBK_WITH_MASKS 32u /* with BBK_CANONICAL: the payload of every k-mer is the OR of the InOutMask bits of its
                              occurrences (the records of the extension index before they are ordered) instead of a
                              multiplicity; bbk_kmerset_export* hand it out where they hand out counts.  The multi-GPU
                              path exchanges these records by owner and builds each shard of the index from them
                              (bbk_extindex_from_device). */
int bbk_count(bbk_ctx *ctx, const bbk_reads *reads, unsigned k, unsigned flags, bbk_kmerset **out);
/* Streaming count: the input never has to be resident as a whole.  Replaces the bounded-memory contract of
 * KMerSortingSplitter -- per-thread cells of `-b` bytes (PrepareBuffers, common/utils/kmer_mph/kmer_splitter.hpp:73-109),
 * one sorted + uniqued run per bucket every time the cells fill up (DumpBuffers, :120-167), and the loser-tree merge of
 * the runs at the end (KMerDiskCounter::MergeKMers, kmer_index_builder.hpp:281-365).  Every pushed batch is
 * deduplicated on the device and kept as a run of distinct canonical k-mers; runs are merge-uniqued into the
 * accumulated set as they pile up; bbk_count_finish orders the set as `flags` ask (same flags and same result as one
 * bbk_count over the concatenated batches).  Device memory is bounded by the batch and the DISTINCT set, host memory
 * by the batch.  bbk_count_finish releases the counter (also on failure); bbk_count_abort drops it without a result. */
typedef struct bbk_counter bbk_counter;
int bbk_count_begin(bbk_ctx *ctx, unsigned k, unsigned flags, bbk_counter **out);
int bbk_count_push_reads(bbk_counter *c, const bbk_reads *reads);
/* ASCII batch (same arguments and LongestValid rule as bbk_reads_from_ascii) */
int bbk_count_push_ascii(bbk_counter *c, const char *h_bases, const uint64_t *h_offsets, uint64_t n_reads);
int bbk_count_finish(bbk_counter *c, bbk_kmerset **out);
/* bbk_count_finish with a minimum multiplicity: the exact form of BayesHammer's count_filter_singletons
 * (KMerDataCounter::BuildKMerIndex, projects/hammer/kmer_data.cpp:280-335, which keeps the k-mers a counting quotient
 * filter has seen more than once; that filter may over-count and let a singleton through, this one may not).  The
 * counter must have been begun with BBK_WITH_COUNTS (BBK_ERR_ARG otherwise).  The result is record for record what
 * bbk_count_finish of the same counter would give, minus every record whose exported multiplicity is < min_count: order
 * and counts of the others are unchanged, min_count <= 1 is the identity, and *n_dropped receives the number of records
 * of the unfiltered result that are absent.  The rule is on the EXPORTED multiplicity: in a BBK_BOTH_STRANDS set at even
 * k a k-mer equal to its own reverse complement counts twice per occurrence, so a single occurrence of it survives
 * min_count = 2.  The filter runs on the distinct canonical records before they are expanded and ordered: the unfiltered
 * set never exists.  Releases the counter, also on failure. */
int bbk_count_finish_min_count(bbk_counter *c, uint32_t min_count, bbk_kmerset **out, uint64_t *n_dropped);
void bbk_count_abort(bbk_counter *c);
uint64_t bbk_count_pushed_instances(const bbk_counter *c); /* k-mer positions seen so far */
/* Device pointer to the records of the set (size * words u64) in the order it is stored in; valid until
 * bbk_kmerset_free.  *order receives BBK_ORDER_SORTED / BBK_ORDER_REFERENCE_BUCKETS16, or 0xFFFFFFFF for a
 * BBK_UNSORTED set. */
const void *bbk_kmerset_keys(const bbk_kmerset *s, unsigned *order);
/* Sort + unique an array of k-mer records already in HBM (n records of bbk_words(k) u64 each,
 * optional u32 multiplicities that are summed).  Used after the multi-GPU exchange. */
int bbk_kmerset_from_device(bbk_ctx *ctx, const void *d_keys, const void *d_counts, uint64_t n, unsigned k,
                            bbk_kmerset **out);
/* same with flags: BBK_UNSORTED deduplicates only (hash-bucket order) */
int bbk_kmerset_from_device_ex(bbk_ctx *ctx, const void *d_keys, const void *d_counts, uint64_t n, unsigned k,
                               unsigned flags, bbk_kmerset **out);
/* canon U rc(canon): the both-strand set of spades-kmercount from a BBK_CANONICAL set (each rank
 * applies it to its own shard after the multi-GPU exchange). */
int bbk_kmerset_both_strands(bbk_ctx *ctx, const bbk_kmerset *canon, bbk_kmerset **out);
/* same; flags = BBK_REFERENCE_ORDER stores the result in the final_kmers order */
int bbk_kmerset_both_strands_ex(bbk_ctx *ctx, const bbk_kmerset *canon, unsigned flags, bbk_kmerset **out);
unsigned bbk_words(unsigned k); /* RtSeq::GetDataSize (common/sequence/rtseq.hpp:129-131) */
uint64_t bbk_kmerset_size(const bbk_kmerset *s);
unsigned bbk_kmerset_k(const bbk_kmerset *s);
uint64_t bbk_kmerset_instances(const bbk_kmerset *s); /* k-mer instances that entered the sort */
#define BBK_ORDER_SORTED 0u              /* ascending, word 0 most significant (adt/array_vector.hpp:114-123) */
#define BBK_ORDER_REFERENCE_BUCKETS16 1u /* the final_kmers order: XXH3 bucket (16) major, ascending inside
                                            (kmer_buckets.hpp:28-33, kmer_index_builder.hpp:168-181) */
/* dst_keys: size * words u64 (host or device); dst_counts (u32, may be NULL). */
int bbk_kmerset_export(bbk_ctx *ctx, const bbk_kmerset *s, unsigned order, void *dst_keys, void *dst_counts);
/* Multi-GPU owner partition: owner(key) = mulhi(mix(key), nranks).  Writes the
 * records grouped by owner to dst (host or device) and the per-owner record counts to h_counts. */
int bbk_kmerset_export_by_owner(bbk_ctx *ctx, const bbk_kmerset *s, unsigned nranks, void *dst_keys,
                                void *dst_counts, uint64_t *h_counts);
/* The device side of spades-read-filter: io::CoverageFilter / CountMedianMlt
 * (common/io/reads/coverage_filtering_read_wrapper.hpp:22-76, projects/kmercount/read_filter.cpp:76-121): h_keep[i] = 1
 * when the upper median of the multiplicities of read i's k-mers (strands identified) is >= threshold (the tool passes
 * its -c value + 1).  `counts` must be the ascending canonical set with counts of the whole dataset
 * (bbk_count(BBK_CANONICAL | BBK_WITH_COUNTS)).  Reads shorter than k have median 0.  For a pair the tool keeps both
 * mates when either passes (coverage_filtering_read_wrapper.hpp:78-94). */
int bbk_reads_median_filter(bbk_ctx *ctx, const bbk_reads *reads, const bbk_kmerset *counts, unsigned threshold,
                            uint8_t *h_keep, uint64_t *n_kept);
void bbk_kmerset_free(bbk_kmerset *s);
/* VERIFY(std::is_sorted(run)) analogue (KMerDiskCounter::MergeKMers, common/utils/kmer_mph/kmer_index_builder.hpp:297),
 * on the device, for sets too large to download: *n_runs = maximal ascending runs of the stored order (1 for an
 * ascending set, <= 16 for a set in the final_kmers order), *n_equal = equal neighbours (0 for a distinct set);
 * h_run_starts (optional, cap entries): record index where each of the first runs begins. */
int bbk_kmerset_verify_order(bbk_ctx *ctx, const bbk_kmerset *s, uint64_t *n_runs, uint64_t *n_equal,
                             uint64_t *h_run_starts, unsigned cap);
/* records [first, first + count) of the stored order (and their multiplicities, if kept) to host memory */
int bbk_kmerset_get(bbk_ctx *ctx, const bbk_kmerset *s, uint64_t first, uint64_t count, void *h_keys, void *h_counts);
/* Writes <path> in the final_kmers format (raw little-endian records, no header). */
int bbk_kmerset_write_final_kmers(bbk_ctx *ctx, const bbk_kmerset *s, const char *path);

/* ---- extension index: replaces DeBruijnExtensionIndexBuilder::BuildExtensionIndexFromStream
 *      (common/utils/extension_index/kmer_extension_index_builder.hpp:62-106) -------------- */
int bbk_extindex_build(bbk_ctx *ctx, const bbk_reads *reads, unsigned k, bbk_extindex **out);
/* The index of a record array already in HBM: n canonical k-mers (bbk_words(k) u64 each) with u32 mask payloads, in
 * any order, duplicates allowed (their masks are OR-ed).  What a rank builds its shard from after the owner exchange
 * of BBK_WITH_MASKS records, and what the gathered shards are merged with before the unitig stage. */
int bbk_extindex_from_device(bbk_ctx *ctx, const void *d_keys, const void *d_masks_u32, uint64_t n, unsigned k,
                             bbk_extindex **out);
/* masks as u32 (the payload layout of the exchange), dst may be host or device */
int bbk_extindex_export_u32(bbk_ctx *ctx, const bbk_extindex *x, void *dst_keys, void *dst_masks_u32);
/* Streaming build (same contract as bbk_count_begin / push / finish): (canonical k-mer, mask bits) records of every
 * pushed batch are OR-reduced on the device, merged as they pile up, ordered once by bbk_extindex_finish. */
typedef struct bbk_extbuilder bbk_extbuilder;
int bbk_extindex_begin(bbk_ctx *ctx, unsigned k, bbk_extbuilder **out);
int bbk_extindex_push_reads(bbk_extbuilder *b, const bbk_reads *reads);
int bbk_extindex_finish(bbk_extbuilder *b, bbk_extindex **out);
void bbk_extindex_abort(bbk_extbuilder *b);
/* Count + extension index from ONE pass over the reads (BASELINE configs[2]: both are wanted of the same reads): the
 * canonical records the index is built from are also the canonical set of the count -- including the k-mers of reads of
 * length exactly k, which the index drops (they never get an extension bit) and spades-kmercount keeps.
 * set_flags = BBK_BOTH_STRANDS [| BBK_REFERENCE_ORDER].  Results equal bbk_count / bbk_extindex_build run separately. */
int bbk_count_extindex(bbk_ctx *ctx, const bbk_reads *reads, unsigned k, unsigned set_flags, bbk_kmerset **set,
                       bbk_extindex **out);
int bbk_extindex_finish_with_set(bbk_extbuilder *b, unsigned set_flags, bbk_kmerset **set, bbk_extindex **out);
uint64_t bbk_extindex_size(const bbk_extindex *x);
unsigned bbk_extindex_k(const bbk_extindex *x);
/* sorted canonical k-mers (size*words u64) and their InOutMask bytes
 * (kmer_extension_index.hpp:42-196: bits 0-3 outgoing A,C,G,T; bits 4-7 incoming) */
int bbk_extindex_export(bbk_ctx *ctx, const bbk_extindex *x, void *dst_keys, void *dst_masks);
/* Early tip clipping on the index, in place: EarlyTipClipperProcessor(index, length_bound).ClipTips()
 * (common/assembly_graph/construction/early_simplification.hpp:37-160; the main pipeline calls it between the
 * extension index and the unitig extraction, stages/construction.cpp:218-275, with length_bound = read length - k
 * unless configured).  Tips (dead-end branches of at most length_bound k-mers) shorter than the longest outgoing
 * branch of their junction are isolated (mask 0) and the junction's links to them removed.
 * *removed_kmers = isolated k-mers (the count the reference logs), *removed_links = links dropped afterwards. */
int bbk_extindex_clip_tips(bbk_ctx *ctx, bbk_extindex *x, uint32_t length_bound, uint64_t *removed_kmers,
                           uint64_t *removed_links);
/* Early poly-A/T clipping on the index, in place: EarlyLowComplexityClipperProcessor(index, ratio, min_len, max_len)
 * (common/assembly_graph/construction/early_simplification.hpp:163-344; the main pipeline runs RemoveATEdges, then
 * RemoveATTips with ratio 0.8, min_len 10, max_len 200 before the early tip clipper, stages/construction.cpp:320-331).
 * A k-mer is of low complexity when its most frequent nucleotide count c satisfies !math::ls(c, L * ratio) (L = k for
 * edges, max(tip length, min_len) for tips; math::ls treats values within 4 ULPs as equal, math/xmath.h:218-226,300-305).
 * remove_at_edges (:183-257): every junction k-mer of low complexity, in either orientation, loses its outgoing links
 * to junctions (dead ends included).  *removed_edges = collected (k-mer, nucleotide) pairs (both orientations of a link
 * count when both qualify: the number the reference logs as "(k+1)-mers were removed"); *removed_links = 2 per removed
 * link ("Links removed").
 * remove_at_tips (:269-333): every dead end with a unique incoming edge is followed back to a junction over at most
 * max_len k-mers; a low-complexity tip that ends at a junction which is not a dead start is isolated (mask 0) and the
 * junction drops its links to it.  *removed_kmers = isolated k-mers, *clipped_links = links dropped ("Clipped tips").
 * BBK_ERR_ARG: a NULL argument, ratio not finite or <= 0, an even k; for tips also max_len == 0 or min_len > k (the
 * reference reads base k-1-i of the junction for i < min_len). */
int bbk_extindex_remove_at_edges(bbk_ctx *ctx, bbk_extindex *x, double ratio, uint64_t *removed_edges,
                                 uint64_t *removed_links);
int bbk_extindex_remove_at_tips(bbk_ctx *ctx, bbk_extindex *x, double ratio, uint32_t min_len, uint32_t max_len,
                                uint64_t *removed_kmers, uint64_t *clipped_links);
void bbk_extindex_free(bbk_extindex *x);

/* ---- unitigs + graph links: replaces UnbranchingPathExtractor::ExtractUnbranchingPathsAndLoops
 *      and FastGraphFromSequencesConstructor::ConstructGraph
 *      (common/assembly_graph/construction/debruijn_graph_constructor.hpp:182-388,390-518) ----- */
int bbk_unitigs_build(bbk_ctx *ctx, bbk_extindex *x, bbk_unitigs **out);
/* ref_threads > 0: perfect loops are collected in the k-mer FILE order of a reference run with -t ref_threads (10 x t
 * XXH3 buckets, ascending inside: kmer_extension_index_builder.hpp:73, CollectLoops debruijn_graph_constructor.hpp:308-344),
 * which fixes where a loop string starts and which palindromic (k+1)-mer SplitLoop (:248-252) cuts a self-conjugate
 * circle at -- the two things that depend on the thread count in the reference itself.  0 = ascending k-mer order. */
int bbk_unitigs_build_ex(bbk_ctx *ctx, bbk_extindex *x, unsigned ref_threads, bbk_unitigs **out);
/* `-c`: coverage of every condensed edge = sum over its (k+1)-mers of their multiplicity in
 * reads + rc(reads) (CoverageHashMapBuilder, common/utils/ph_map/coverage_hash_map_builder.hpp:15-54;
 * FillCoverageAndFlankingFromPHM, assembly_graph/graph_support/coverage_filling.hpp:44-62).  After this
 * call the GFA carries DP:f:<KC/(len-k)> and KC:i:<KC> (projects/gbuilder/main.cpp:200-211). */
int bbk_unitigs_add_coverage(bbk_ctx *ctx, bbk_unitigs *u, const bbk_reads *reads);
/* same from a table the caller has already counted (streaming input: the reads are gone by now): the ascending
 * canonical (k+1)-mer set with multiplicities, bbk_count*(k + 1, BBK_CANONICAL | BBK_WITH_COUNTS) */
int bbk_unitigs_add_coverage_counts(bbk_ctx *ctx, bbk_unitigs *u, const bbk_kmerset *kp1_counts);
int bbk_unitigs_export_kc(bbk_ctx *ctx, const bbk_unitigs *u, uint64_t *h_kc);
uint64_t bbk_unitigs_count(const bbk_unitigs *u);
uint64_t bbk_unitigs_loops(const bbk_unitigs *u);
uint64_t bbk_unitigs_total_bases(const bbk_unitigs *u);
uint64_t bbk_unitigs_vertices(const bbk_unitigs *u);
uint64_t bbk_unitigs_links(const bbk_unitigs *u);
/* The condensed edges as a read set in HBM (packed on the device, nothing crosses PCIe): what the main pipeline does
 * when it feeds the contigs of the previous K into the construction of the next
 * (common/stages/construction.cpp:117-119,228-236: contigs_streams merged into the read streams), and what the
 * full-size tests use to recount the (k+1)-mers of the graph. */
int bbk_unitigs_to_reads(bbk_ctx *ctx, const bbk_unitigs *u, bbk_reads **out);
/* h_bases: total_bases ASCII bytes (no separators); h_offsets: count+1 entries. */
int bbk_unitigs_export(bbk_ctx *ctx, const bbk_unitigs *u, char *h_bases, uint64_t *h_offsets);
/* links: 4 x u32 per link (from_unitig, from_orient(1='+'), to_unitig, to_orient) */
int bbk_unitigs_export_links(bbk_ctx *ctx, const bbk_unitigs *u, uint32_t *h_links);
/* GFA1 text as GFAWriter::WriteSegmentsAndLinks (common/io/graph/gfa_writer.cpp:18-52), segment
 * ids 3+2i (assembly_graph/core/graph_core.hpp:228,610-624); `--unitigs` FASTA as
 * projects/gbuilder/main.cpp:183-192. */
int bbk_unitigs_write_gfa(bbk_ctx *ctx, const bbk_unitigs *u, const char *path);
int bbk_unitigs_write_fasta(bbk_ctx *ctx, const bbk_unitigs *u, const char *path);
/* FASTG as FastgWriter::WriteSegmentsAndLinks (common/io/graph/fastg_writer.cpp:20-47): every edge and its
 * conjugate, header = EDGE_<id>_length_<len>_cov_<cov>['] : successors ; */
int bbk_unitigs_write_fastg(bbk_ctx *ctx, const bbk_unitigs *u, const char *path);
/* SPAdes binary graph <basename>.grseq + <basename>.cvr as io::binary::BasicGraphIO<Graph>().Save
 * (common/io/binary/basic.hpp:24-27, graph.hpp:27-46, coverage.hpp:24-29; gbuilder --spades,
 * projects/gbuilder/main.cpp:221-222).  Edge ids 3+2i as in the GFA; vertex ids in ascending end-k-mer order (the
 * reference's follow its BooPHF indices; its loader takes any consistent numbering). */
int bbk_unitigs_write_spades(bbk_ctx *ctx, const bbk_unitigs *u, const char *basename);
void bbk_unitigs_free(bbk_unitigs *u);

/* ---- per-sample edge abundance profiles: replaces unitig-coverage (projects/unitig_coverage/main.cpp:40-80):
 *      the EdgeIndex of the (k+1)-mers of a graph (common/assembly_graph/index/edge_index_builders.hpp), the
 *      BasicSequenceMapper that maps each read onto it (common/modules/alignment/sequence_mapper.hpp:288-404) and
 *      EdgeProfileStorage::Fill / Save (projects/unitig_coverage/profile_storage.{hpp,cpp}) ------------------------- */
typedef struct bbk_edgeindex bbk_edgeindex; /* every (k+1)-mer of every segment, canonical, with its place     */
typedef struct bbk_profiles bbk_profiles;   /* raw abundances, segments x samples u64, in HBM                 */
/* GFA1 graph (io/graph/gfa_reader.cpp): S lines are the segments in file order (a segment is the edge of its forward
 * strand plus its conjugate; a palindromic segment is its own conjugate), L lines its links.  BBK_ERR_ARG (with a
 * message) for an even k, a link overlap other than <k>M or one whose bases do not overlap, a segment shorter than
 * k + 1, a base other than ACGT, and a (k+1)-mer held twice by the graph (counting both orientations): the mapping
 * relies on each (k+1)-mer having one place, as the graphs spades-gbuilder writes do. */
int bbk_edgeindex_from_gfa(bbk_ctx *ctx, const char *path, unsigned k, bbk_edgeindex **out);
/* the same from an in-process graph; segment i is named 3 + 2i as bbk_unitigs_write_gfa names it */
int bbk_edgeindex_from_unitigs(bbk_ctx *ctx, const bbk_unitigs *u, bbk_edgeindex **out);
uint64_t bbk_edgeindex_segments(const bbk_edgeindex *ix);
uint64_t bbk_edgeindex_size(const bbk_edgeindex *ix); /* (k+1)-mers indexed */
void bbk_edgeindex_free(bbk_edgeindex *ix);
/* Profiles of n_samples samples over the segments of ix (which must outlive them), all zero.  push_reads maps one
 * batch of reads of one sample: every read and, implicitly, its reverse complement (io::EasyStream followed_by_rc,
 * io/reads/io_helper.cpp:19-32); the reads have gone through LongestValid already (bbk_reads).  raw[segment][sample]
 * += the mapped-range sizes of MapSequence on the segment's edge and its conjugate. */
int bbk_profiles_begin(bbk_ctx *ctx, const bbk_edgeindex *ix, unsigned n_samples, bbk_profiles **out);
int bbk_profiles_push_reads(bbk_profiles *p, unsigned sample, const bbk_reads *reads);
/* h_raw: segments x samples u64, segment-major */
int bbk_profiles_export_raw(bbk_ctx *ctx, const bbk_profiles *p, uint64_t *h_raw);
/* EdgeProfileStorage::Save (profile_storage.cpp:44-52): "<name>\t" then raw / (|seq| - k) of every sample as
 * std::ostream prints a double (%g), each followed by "\t", then "\n"; one line per segment in S-line order. */
int bbk_profiles_write(bbk_ctx *ctx, const bbk_profiles *p, const char *path);
void bbk_profiles_free(bbk_profiles *p);

/* ---- mapping paths: the mapper of spades-gmapper (projects/gmapper/main.cpp:156-247), the MappingPath of every read
 *      (BasicSequenceMapper::MapSequence, modules/alignment/sequence_mapper.hpp:288-404) over the same index ---------- */
typedef struct bbk_paths bbk_paths; /* the ranges of one batch of reads, in HBM */
typedef struct {
    uint64_t edge;                 /* 2 * segment, + 1 on the reverse strand of a segment that is not self-conjugate */
    uint32_t read;                 /* read of the batch */
    uint32_t init_start, init_end; /* (k+1)-mer positions on the read, [start, end) */
    uint32_t map_start, map_end;   /* (k+1)-mer offsets on the oriented edge, [start, end) */
    uint32_t reserved;
} bbk_path_range;
/* Maps every read of the batch as it stands, without its reverse complement; the ranges come in read order and in
 * position order within a read.  The batch has gone through LongestValid, so a caller that cuts reads at N as MapRead
 * does (sequence_mapper.hpp:68-98) passes the pieces as reads. */
int bbk_edgeindex_map_paths(bbk_ctx *ctx, const bbk_edgeindex *ix, const bbk_reads *reads, bbk_paths **out);
uint64_t bbk_paths_reads(const bbk_paths *p);
uint64_t bbk_paths_ranges(const bbk_paths *p);
/* h_read_offsets: reads + 1 entries, the ranges of read r are [off[r], off[r + 1]); h_ranges: one entry per range.
 * Either may be NULL. */
int bbk_paths_export(bbk_ctx *ctx, const bbk_paths *p, uint64_t *h_read_offsets, bbk_path_range *h_ranges);
void bbk_paths_free(bbk_paths *p);
/* bbk_edgeindex_from_gfa that also keeps the graph itself (bases, L lines, KC) for the calls below; the other
 * constructors keep only the segment names */
int bbk_edgeindex_from_gfa_with_graph(bbk_ctx *ctx, const char *path, unsigned k, bbk_edgeindex **out);
/* the graph as the index holds it (parsed once from the GFA): L lines, bases (0 when not kept), segment names */
uint64_t bbk_edgeindex_links(const bbk_edgeindex *ix);
uint64_t bbk_edgeindex_total_bases(const bbk_edgeindex *ix);
const char *bbk_edgeindex_name(const bbk_edgeindex *ix, uint64_t segment); /* NULL past the last segment */
/* Any pointer may be NULL.  h_bases: the segments' bases back to back; h_offsets: segments + 1 entries; h_links: 4 x u32
 * per L line in file order (segment a, 1 if a is '+', segment b, 1 if b is '+'); h_kc: the first KC:i: of every S line
 * as GFAReader reads it (io/graph/gfa_reader.cpp:65-68: an int32), 0 without one.  BBK_ERR_ARG for an index that
 * keeps no graph. */
int bbk_edgeindex_export_graph(const bbk_edgeindex *ix, char *h_bases, uint64_t *h_offsets, uint32_t *h_links,
                               uint32_t *h_kc);

/* h_len: the (k+1)-mers of every segment, |seq| - k, the reference's g.length(e) of its edge and of the conjugate;
 * h_self_conjugate: 1 for a segment that is its own reverse complement (one edge), 0 otherwise (two).  Either may be
 * NULL; segments entries each. */
int bbk_edgeindex_export_segments(const bbk_edgeindex *ix, uint64_t *h_len, uint8_t *h_self_conjugate);

/* ---- paired-read info: the paired-end side of PairInfoCount (projects/spades/pair_info_count.cpp:199-243, 285-324,
 *      328-417) over the mapping paths of the two mates: InsertSizeCounter (common/paired_info/is_counter.hpp:85-115) with
 *      the statistics of insert_size_refiner.hpp:23-166, EdgePairCounterFiller / DEFilter (pair_info_count.cpp:70-137)
 *      and LatePairedIndexFiller (common/paired_info/pair_info_filler.hpp:63-93) into the raw, unclustered paired index
 *      (common/paired_info/paired_info_buffer.hpp:54-57, 103-147).  The reference has the stage only inside spades-core;
 *      parity is with a restatement (tests/pairinfo_restated.py) ------------------------------------------------------ */
typedef struct bbk_pairinfo bbk_pairinfo; /* the reduced runs of the passes in HBM, their results on the host */
/* OrientationChanger (common/io/reads/orientation.hpp:15-41): which mate is reverse-complemented before it is mapped */
#define BBK_ORIENT_FF 0 /* neither */
#define BBK_ORIENT_FR 1 /* the second */
#define BBK_ORIENT_RF 2 /* the first */
#define BBK_ORIENT_RR 3 /* both */
typedef struct bbk_pairinfo_stats {
    uint64_t total, mapped, negative; /* pairs seen; with a positive insert size on one long edge; with one <= 0 there */
    uint64_t edge_pairs;              /* distinct ordered (e1, e2) over path1 x path2: exact, where the reference
                                         estimates it with a HyperLogLog */
    double mean, deviation;           /* find_mean */
    double median, mad;               /* find_median */
    double left_quantile, right_quantile; /* GetISInterval(0.8) of the cropped histogram */
    uint64_t percentiles[19];         /* 5 % ... 95 % of find_mean; 0 where the reference sets none */
    int ok;                           /* CollectLibInformation's verdict: 0 when mapped == 0 (no statistic is computed),
                                         when median < k + 2 (no quantile is), or when the cropped histogram is empty */
} bbk_pairinfo_stats;
/* ix must outlive the result.  min_edge_length: edge_length_threshold of InsertSizeCounter. */
int bbk_pairinfo_begin(bbk_ctx *ctx, const bbk_edgeindex *ix, uint64_t min_edge_length, bbk_pairinfo **out);
/* One batch of pairs: pair p is read p of `first` and read p of `second`, in file orientation; both have gone through
 * LongestValid (bbk_reads).  h_cut: 4 x u32 per pair, the bases LongestValid cut before and after each mate in file
 * orientation (left1, right1, left2, right2: SingleRead's offsets, io/reads/single_read.hpp:247-258); NULL = zeros.  The
 * engine swaps a mate's two values when the orientation reverse-complements it (single_read.hpp:143-147).  Every pair
 * counts in total; its insert size and its edge pairs are reduced on the device.  The result of the pass is the same
 * bytes for any batching of the pairs.  BBK_ERR_ARG: unequal read counts, an orientation out of range, 2^32 pairs or
 * 2^32 edge-pair records in one pass (the device counts are 32 bits wide: nothing wraps silently). */
int bbk_pairinfo_push_estimate(bbk_pairinfo *pi, const bbk_reads *first, const bbk_reads *second, int orientation,
                               const uint32_t *h_cut);
/* Ends (or refreshes, after further pushes) the estimate pass: the statistics in doubles on the host, line by line as
 * the reference computes them. */
int bbk_pairinfo_estimate(bbk_pairinfo *pi, bbk_pairinfo_stats *stats);
/* the insert-size histogram of the estimate pass, ascending; either pointer may be NULL */
uint64_t bbk_pairinfo_hist_size(const bbk_pairinfo *pi);
int bbk_pairinfo_hist_export(const bbk_pairinfo *pi, int32_t *h_is, uint64_t *h_count);
/* The fill pass.  insert_size: the reference passes (size_t) mean_insert_size.  round_distance > 1 rounds every distance
 * to a multiple of it, half away from zero.  filter_threshold t > 0 keeps a pair of edges iff min(c, 3) > t with
 * c = occurrences(e1, e2) + occurrences(conj e2, conj e1) over the estimate pass (the reference's counting Bloom filter
 * has 2-bit cells and may over-count; these counts are exact); t = 0 keeps every pair.  BBK_ERR_ARG: t > 0 without an
 * estimate pass over the same handle; bbk_pairinfo_push_fill before bbk_pairinfo_estimate or before
 * bbk_pairinfo_fill_begin; the errors of bbk_pairinfo_push_estimate. */
int bbk_pairinfo_fill_begin(bbk_pairinfo *pi, uint64_t insert_size, unsigned round_distance, unsigned filter_threshold);
int bbk_pairinfo_push_fill(bbk_pairinfo *pi, const bbk_reads *first, const bbk_reads *second, int orientation,
                           const uint32_t *h_cut);
int bbk_pairinfo_fill_finish(bbk_pairinfo *pi);
/* The index: points (e1, e2, gap, weight) ascending, edges numbered as bbk_path_range.edge, gap = distance - length(e1),
 * stored under the smaller of (e1, e2) and (conj e2, conj e1); a pair with e1 == conj e2 has every weight doubled.
 * Integers, exact.  Any pointer may be NULL. */
uint64_t bbk_pairinfo_points(const bbk_pairinfo *pi);
int bbk_pairinfo_export(const bbk_pairinfo *pi, uint64_t *h_e1, uint64_t *h_e2, int32_t *h_gap, uint64_t *h_weight);
/* <path> in the layout of PairedBuffer::BinWrite (paired_info_buffer.hpp:197-210): the number of first edges; per first
 * edge, ascending, its id, then per stored second edge its id and its histogram as io::binary::BinWrite writes one (the
 * number of points, then per point float gap, float weight: RawPointT::BinWrite, index_point.hpp:195-197), then a 0.
 * Unsigned integers are ULEB128, as io::binary::BinWrite encodes them (io/binary/binary.hpp:109-122).  The reference's
 * edge ids are not reproducible here, so an id is edge + 1 (0 is the terminator).  The file's floats are exact below
 * 2^24; bbk_pairinfo_export is exact always. */
int bbk_pairinfo_write(const bbk_pairinfo *pi, const char *path);
void bbk_pairinfo_free(bbk_pairinfo *pi);

/* ---- distance estimation: the raw paired index clustered on the graph distances between the two edges of every stored
 *      pair (projects/spades/distance_estimation.cpp:137-154: DistanceEstimator, common/paired_info/distance_estimation.cpp,
 *      and PairInfoWeightChecker; csrc/distest.hip).  Left out: RefinePairedInfo (it cannot fire on this output),
 *      PairInfoImprover, the scaffolding index and amb_de.  Parity is with a restatement (tests/distest_restated.py) --- */
typedef struct bbk_clustered bbk_clustered; /* the clustered index on the host */
/* A raw index from host points instead of reads: every point goes under the smaller of (e1, e2) and (conj e2, conj e1)
 * with its gap (the gap is the same under both), the points are sorted, and equal (e1, e2, gap) have their weights
 * added: what bbk_pairinfo_fill_finish leaves.  Weights are stored weights (bbk_pairinfo_export's): nothing is doubled,
 * so an exported index comes back as it was.  BBK_ERR_ARG: an edge the graph does not have. */
int bbk_pairinfo_import(bbk_ctx *ctx, const bbk_edgeindex *ix, uint64_t n, const uint64_t *h_e1, const uint64_t *h_e2,
                        const int32_t *h_gap, const uint64_t *h_weight, bbk_pairinfo **out);
typedef struct bbk_cluster_params { /* estimate_distance (distance_estimation.cpp:137-154) */
    uint64_t insert_size;      /* (size_t) math::round(mean_insert_size) */
    uint64_t read_length;      /* the library's read length */
    uint64_t delta;            /* size_t(deviation) */
    uint64_t linkage_distance; /* size_t(linkage_distance_coeff * deviation); shipped coefficient 0.0 */
    uint64_t max_distance;     /* size_t(max_distance_coeff * deviation); shipped coefficient 2.0 */
    double filter_threshold;   /* clustered_filter_threshold; shipped 2.0 */
} bbk_cluster_params;
/* Clusters the points of a filled (or imported) index.  The index must keep its graph
 * (bbk_edgeindex_from_gfa_with_graph); its vertices and their CSR go to the device with the first call.  A pair whose
 * search would make 500 calls or more, whose ball holds more than 512 vertices, or any pair when insert_size + delta -
 * k - 2 > 2047, is searched on the host by the literal backtracking search (ties by ascending edge number); so is every
 * pair when BBK_NO_DISTEST_DEVICE is set.  BBK_ERR_ARG: before bbk_pairinfo_fill_finish, an index without a graph,
 * insert_size + delta - k - 2 <= 0 (the reference's VERIFY), a distance parameter of 2^24 or more. */
int bbk_pairinfo_cluster(bbk_pairinfo *pi, const bbk_cluster_params *params, bbk_clustered **out);
/* Clusters ascending (e1, e2, centre) under the canonical pair only: centre = the distance (not the gap) as the
 * reference's float, var = 0 (the reference's AddToResult drops ClusterResult's half-span: its buffer holds raw points),
 * weight in half-units (twice the weight; a pair with e1 == conj e2 carries four
 * times its clusters' weight, as the reference's buffer and merge leave it).  Any pointer may be NULL. */
uint64_t bbk_clustered_points(const bbk_clustered *c);
uint64_t bbk_clustered_pairs(const bbk_clustered *c);      /* edge pairs the raw index held */
uint64_t bbk_clustered_host_pairs(const bbk_clustered *c); /* of these, searched on the host */
int bbk_clustered_export(const bbk_clustered *c, uint64_t *h_e1, uint64_t *h_e2, float *h_centre, float *h_var,
                         uint64_t *h_weight);
/* <path> in the layout of bbk_pairinfo_write: a point is float gap = centre - length(e1), float weight (PointT inherits
 * RawPointT::BinWrite, index_point.hpp:195-197, 218-259: 8 bytes, no variance).  Ids are edge + 1. */
int bbk_clustered_write(const bbk_clustered *c, const char *path);
void bbk_clustered_free(bbk_clustered *c);

/* ---- k-mer multiplicity profiles across samples: replaces KmerMultiplicityCounter::FilterCombinedKmers
 *      (projects/mts/kmer_multiplicity_counter.cpp:72-139: one KMC database per sample, sorted and merged under
 *      RtSeq::less3 = BBK_ORDER_SORTED) and, for the lookup, the BooPHF map of BuildKmerIndex (:141-181) -- and contig
 *      abundances over them: ProfileCounter::operator() (projects/mts/contig_abundance.cpp:245-284) with the winsorised
 *      mean of TrivialClusterAnalyzer (:46-78) ---------------------------------------------------------------------- */
typedef struct bbk_kmerprofile_builder bbk_kmerprofile_builder; /* the filtered sets of the samples, in HBM          */
typedef struct bbk_kmerprofile bbk_kmerprofile; /* kept k-mers ascending + one row of n_samples u16 each, in HBM     */
/* ci / cs: KMC's per-sample filter (its defaults are 2 and 255): a k-mer counted fewer than ci times is absent from
 * that sample, the remaining counts are saturated at cs.  BBK_ERR_ARG for ci < 1 and for cs outside 1..65535 (the
 * reference would silently truncate a larger count to the 16 bits of a row, :92,127-129). */
int bbk_kmerprofile_begin(bbk_ctx *ctx, unsigned k, unsigned n_samples, unsigned ci, unsigned cs,
                          bbk_kmerprofile_builder **out);
/* sample in [0, n_samples), each exactly once; the set must be the ascending canonical set with counts of the sample's
 * reads (bbk_count*(k, BBK_CANONICAL | BBK_WITH_COUNTS)) and may be freed after the call: its filtered records (keys
 * + u16 counts) stay in HBM until bbk_kmerprofile_finish.  An empty set is a valid sample. */
int bbk_kmerprofile_add_sample(bbk_kmerprofile_builder *b, unsigned sample, const bbk_kmerset *canonical_counts);
/* The join.  With present = samples holding the k-mer and total = the sum of its counts, a k-mer is kept iff
 * present >= min_samples && (present > 1 || total > min_mult) (:115,125); an absent sample has 0 in the row.  An empty
 * result is valid (min_samples > n_samples gives one).  Releases the builder, also on failure. */
int bbk_kmerprofile_finish(bbk_kmerprofile_builder *b, uint64_t min_samples, uint64_t min_mult, bbk_kmerprofile **out);
void bbk_kmerprofile_abort(bbk_kmerprofile_builder *b);
uint64_t bbk_kmerprofile_size(const bbk_kmerprofile *p);
unsigned bbk_kmerprofile_samples(const bbk_kmerprofile *p);
unsigned bbk_kmerprofile_k(const bbk_kmerprofile *p);
/* dst_keys: size * words u64 ascending; dst_rows: size * samples u16, sample-major inside a row (host or device;
 * either may be NULL) */
int bbk_kmerprofile_export(bbk_ctx *ctx, const bbk_kmerprofile *p, void *dst_keys, void *dst_rows);
/* <prefix>.bpr: the rows as the reference writes them (:94,127-129); <prefix>.kmers: the kept k-mers as RtSeq::BinWrite
 * records (the reference's temporary k-mer file, :126), ascending.  The latter stands in for <prefix>.kmm, the BooPHF
 * serialisation of BuildKmerIndex: here the ascending table is the index. */
int bbk_kmerprofile_write(bbk_ctx *ctx, const bbk_kmerprofile *p, const char *prefix);
/* KmerProfileIndex's constructor (contig_abundance.cpp:189-206).  BBK_ERR_ARG when <prefix>.kmers is not a whole number
 * of k-mer records, when <prefix>.bpr is not records x n_samples x 2 bytes, or when the k-mers do not ascend. */
int bbk_kmerprofile_load(bbk_ctx *ctx, const char *prefix, unsigned k, unsigned n_samples, bbk_kmerprofile **out);
/* Every read is one contig without a character other than ACGT (bbk_reads apply LongestValid).  For contig c:
 * h_positions[c] = its k-mer positions; h_n[c] = those found in the profile, either strand (the "earmarks", :257-271);
 * h_sum / h_sumsq[c * samples + s] = sum and sum of squares of the n values of column s after winsorising:
 * o = ceil(float(n) * 0.05f), lo = sorted[o], hi = sorted[n - o - 1], v -> max(min(v, hi), lo); n = 1 stands as it is.
 * That is WinsoredMeanImpl (:46-59) with its commented-out std::sort; the binary's std::nth_element leaves other
 * elements at those two positions.  Integers only: mean = float(sum) / float(n), variance = float(sumsq) / float(n)
 * - mean * mean and the share test n / (length - k + 1) >= 0.7 (math::ls, :274-281) are the caller's. */
int bbk_kmerprofile_abundance(bbk_ctx *ctx, const bbk_kmerprofile *p, const bbk_reads *contigs, uint64_t *h_n,
                              uint64_t *h_positions, uint64_t *h_sum, uint64_t *h_sumsq);
/* The same for contigs that hold other characters: the caller cuts every contig into its maximal ACGT stretches
 * (SplitOnNs, :172-185) and passes them as reads; contig c is the pieces [h_first_piece[c], h_first_piece[c + 1])
 * (n_contigs + 1 entries, from 0 to the number of pieces; a contig may have none). */
int bbk_kmerprofile_abundance_pieces(bbk_ctx *ctx, const bbk_kmerprofile *p, const bbk_reads *pieces,
                                     const uint64_t *h_first_piece, uint64_t n_contigs, uint64_t *h_n,
                                     uint64_t *h_positions, uint64_t *h_sum, uint64_t *h_sumsq);
void bbk_kmerprofile_free(bbk_kmerprofile *p);

/* ---- Hamming-graph clustering of a k-mer set: replaces TauOneKMerHamClusterer::cluster / ClusterChunk
 *      (projects/hammer/hamcluster.cpp:228-289; BayesHammer's first step, projects/hammer/main.cpp:143-168) over a
 *      dsu::ConcurrentDSU (common/adt/concurrent_dsu.hpp) and ConcurrentDSU::extract_to_file (concurrent_dsu.cpp:17-86) --- */
typedef struct bbk_hamclusters bbk_hamclusters; /* label of every k-mer, members cluster by cluster, sizes: in HBM */
/* set: ascending BBK_BOTH_STRANDS set, k <= 32, fewer than 2^32 - 2 k-mers (the union-find holds u32 parents).  An index
 * is a position in that ascending set.  tau must be 1 (general_tau of configs/hammer/config.info).  K-mers at Hamming
 * distance 1 are united; a cluster is a connected component of that graph unless the component has lock_size members
 * or more: those are replayed on the host by the reference's rule (hamcluster.cpp:235-274: chunks of `chunk` indices
 * in ascending order, the strand with key <= rc(key) of a pair is processed, no union with a locked set
 * (canMerge2, :213-226), sets of >= lock_size members with a member in the chunk are locked after it; unite as
 * concurrent_dsu.hpp:46-96).  lock_size / chunk: 0 = the reference's 2500 (:269) / 65536 (:281).
 * BBK_ERR_ARG: tau != 1, k > 32, a BBK_UNSORTED or BBK_REFERENCE_ORDER set, 2^32 - 2 k-mers or more, a set that is not
 * closed under reverse complement.  An empty set gives zero clusters. */
int bbk_kmerset_hamming_clusters(bbk_ctx *ctx, const bbk_kmerset *set, unsigned tau, uint64_t lock_size, uint64_t chunk,
                                 bbk_hamclusters **out);
uint64_t bbk_hamclusters_count(const bbk_hamclusters *h);    /* clusters (ConcurrentDSU::num_sets, concurrent_dsu.hpp:146-153) */
uint64_t bbk_hamclusters_size(const bbk_hamclusters *h);     /* k-mers */
uint64_t bbk_hamclusters_replayed(const bbk_hamclusters *h); /* k-mers that went through the host replay */
/* h_labels: size entries, the smallest member index of the cluster of every k-mer; h_members: size entries, the member
 * indices cluster by cluster, clusters by ascending label, ascending inside a cluster; h_sizes: count entries.  Any may
 * be NULL.  (The reference lists clusters by DSU root, concurrent_dsu.cpp:54-69.) */
int bbk_hamclusters_export(bbk_ctx *ctx, const bbk_hamclusters *h, uint64_t *h_labels, uint64_t *h_members,
                           uint64_t *h_sizes);
/* <path>: h_members as u64; <path>.idx: h_sizes as u64 -- kmers.hamming / kmers.hamming.idx as
 * ConcurrentDSU::extract_to_file writes them (concurrent_dsu.cpp:63-83) */
int bbk_hamclusters_write(bbk_ctx *ctx, const bbk_hamclusters *h, const char *path);
/* The inverse of bbk_hamclusters_write (a restart with hamming_do 0, projects/hammer/main.cpp:143-168): <path> and
 * <path>.idx for a set of n k-mers.  Clusters may come in any order and members in any order inside a cluster (the
 * reference lists by DSU root); the result is in the documented order.  BBK_ERR_ARG unless <path> holds n members that are
 * a permutation of 0 .. n-1 and the sizes are positive and sum to n. */
int bbk_hamclusters_load(bbk_ctx *ctx, uint64_t n, const char *path, bbk_hamclusters **out);
void bbk_hamclusters_free(bbk_hamclusters *h);

/* ---- quality-aware k-mer statistics: replaces KMerDataCounter::FillKMerData / KMerDataFiller over a KMerData
 *      (projects/hammer/kmer_data.cpp:119-187,369-399): one KMerStat per k-mer (projects/hammer/kmer_stat.hpp:120-149)
 *      -- the occurrence count, total_qual and the saturating 6-bit per-position quality sums (QualBitSet,
 *      kmer_stat.hpp:49-118) that everything BayesHammer does after the clustering reads ------------------------------- */
typedef struct bbk_quals bbk_quals;         /* one quality byte per base of a bbk_reads, in HBM                   */
typedef struct bbk_kmerstats bbk_kmerstats; /* the statistics of every k-mer of a set, in HBM                     */
/* h_qual: the quality of every base with the offset already subtracted (Read's qual_, io/reads/read.hpp), read i at
 * [h_offsets[i], h_offsets[i + 1]) (n_reads + 1 entries).  BBK_ERR_ARG unless n_reads and every length equal those of
 * `reads` -- a read that LongestValid shortened no longer matches -- and for a quality above 93 (33 + 93 is the last
 * printable character; the bound keeps the statistics' sums from overflowing).  `reads` must outlive the result. */
int bbk_quals_from_host(bbk_ctx *ctx, const bbk_reads *reads, const uint8_t *h_qual, const uint64_t *h_offsets,
                        uint64_t n_reads, bbk_quals **out);
void bbk_quals_free(bbk_quals *q);
/* set: ascending BBK_BOTH_STRANDS set, k <= 32, fewer than 2^32 - 2 k-mers; it must outlive the statistics, and an
 * index is a position in it.  BBK_ERR_ARG for a BBK_CANONICAL, BBK_UNSORTED or BBK_REFERENCE_ORDER set and for k > 32.
 * All statistics start as KMerStat() does: count 0, total_qual 1, sums 0. */
int bbk_kmerstats_begin(bbk_ctx *ctx, const bbk_kmerset *set, bbk_kmerstats **out);
/* Every k-mer position p of every read is one occurrence (the reads are free of N; which positions
 * ValidKMerGenerator<K>(read, 2) yields after Read::trimNsAndBadQuality, valid_kmer_generator.hpp:147-199 and
 * io/reads/read.hpp:87-122, is the caller's business: bbk_hreads_stretch_view gives exactly those reads from records as parsed).  With
 * cp = the product over the window of Prob(q) = 1 - (q < 3 ? 0.75 : 10^(-q / 10)) in double (main.cpp:103-105), the
 * k-mer is merged with the qualities q[p .. p + k) and its reverse complement with the same qualities reversed
 * (PushKMer / PushKMerRC, kmer_data.cpp:125-154), each only if it is in the set; Merge (:119-123) is count += 1,
 * total_qual *= (float)(1 - cp), sum[i] = min(63, sum[i] + (q[i] & 63)).  A k-mer that is its own reverse complement
 * is merged twice.  Counts and sums are exact; total_qual is carried as a fixed-point sum of log2 of the factors, so
 * the result is the same bytes for any order and batching of the reads (the reference's float product depends on its
 * thread timing; the difference stays inside that spread).  `quals` must have been made for `reads`. */
int bbk_kmerstats_push(bbk_kmerstats *ks, const bbk_reads *reads, const bbk_quals *quals);
/* after the last push and before an export or a write; pushing again afterwards is allowed and needs another finish */
int bbk_kmerstats_finish(bbk_kmerstats *ks);
uint64_t bbk_kmerstats_size(const bbk_kmerstats *ks);
/* h_count: size u32; h_total_qual: size floats; h_qual_words: size x ceil(6k / 64) u64, the QualBitSet of every k-mer
 * (sum i in bits [6i, 6i + 6) of the 6k-bit little-endian string).  Any pointer may be NULL. */
int bbk_kmerstats_export(bbk_ctx *ctx, const bbk_kmerstats *ks, uint32_t *h_count, float *h_total_qual,
                         uint64_t *h_qual_words);
/* one binary_write(KMerStat) record per k-mer (kmer_stat.hpp:170-175): u32 count << 1 (the good bit is 0, mark_bad), float
 * total_qual, the QualBitSet words: 24 bytes at k = 21.  BBK_ERR_ARG when a count is 2^31 or more. */
int bbk_kmerstats_write(bbk_ctx *ctx, const bbk_kmerstats *ks, const char *path);
/* The inverse of bbk_kmerstats_write: the statistics of every k-mer of `set` from a file of binary_write(KMerStat)
 * records (the good bit is ignored), so that a run can restart after the statistics as the reference does with
 * count_do 0 (projects/hammer/main.cpp:122-141).  The result is finished; bbk_kmerstats_push refuses it.  BBK_ERR_ARG
 * unless the file holds exactly one record of 8 + 8 * ceil(6k / 64) bytes per k-mer of the set. */
int bbk_kmerstats_load(bbk_ctx *ctx, const bbk_kmerset *set, const char *path, bbk_kmerstats **out);
void bbk_kmerstats_free(bbk_kmerstats *ks);

/* ---- Bayesian subclustering of the Hamming clusters: replaces KMerClustering::process / ProcessCluster /
 *      SubClusterSingle / lMeansClustering / ClusterBIC / Consensus / ConsensusWithMask
 *      (projects/hammer/kmer_cluster.cpp:49-633) over ExpandedKMer (projects/hammer/kmer_stat.hpp:205-279) and the
 *      tables of projects/hammer/main.cpp:103-108 -- the step that gives every k-mer its good bit (KMerStat::good(),
 *      kmer_stat.hpp:140-148), the one thing Expander and ReadCorrector read ----------------------------------------- */
typedef struct bbk_subclusters bbk_subclusters; /* the subclusters, the good bits and the new k-mers: in HBM */
typedef struct bbk_subcluster_params {
    double singleton_threshold;    /* bayes_singleton_threshold, 0.995 in configs/hammer/config.info */
    double nonsingleton_threshold; /* bayes_nonsingleton_threshold, 0.9 */
    double correct_threshold;      /* correct_threshold, 0.98 */
    int correct_use_threshold;     /* correct_use_threshold, 1 */
} bbk_subcluster_params;
/* set, hamclusters and kmerstats belong together (k <= 32, the ascending both-strand set, fewer than 2^32 - 2 k-mers, one
 * GPU).  The configuration is config.info's bayes_initial_refine 1, bayes_use_hamming_dist 0, bayes_hammer_mode 0; the
 * other settings of the three are not offered.  p = NULL: the four thresholds of config.info.
 * Every Hamming cluster is processed as ProcessCluster does (:455-577): a singleton by :463-491; any other is ordered
 * by count, split by SubClusterSingle (:261-446: l-means for l = 1, 2, ... scored by ClusterBIC, the merge of duplicate
 * centers, the listing, a consensus that is no member looked up in the set or appended as a new k-mer with count 0 and
 * total_qual 1), and the center of every subcluster is marked good or bad (:503-556).  Exact parity with the literal
 * restatement tests/subcluster_restated.py, the bits of the BIC included (DESIGN.md 4.3e says what that takes).
 * Divergences from the reference: an index is a position in the ascending set; the members of a cluster are ordered by
 * (count descending, index ascending) where the reference's std::sort (:625) is unstable; new k-mers get the indices n,
 * n + 1, ... in the order (cluster by ascending label, subcluster by ascending center number), not deduplicated (the
 * reference appends them in thread-timing order and does not deduplicate either, :429-438); where several subclusters
 * name the same k-mer as their center, the last in that order decides its bit (the reference: the last in time);
 * total_qual is the engine's reproducible value (bbk_kmerstats_push).
 * Clusters of more than 256 k-mers are processed on the host (OpenMP); BBK_SUBCLUSTER_HOST=1 sends all of them there.
 * BBK_ERR_ARG: handles of different sizes or sets, statistics without bbk_kmerstats_finish, a threshold outside [0, 1]. */
int bbk_hamclusters_subcluster(bbk_ctx *ctx, const bbk_kmerset *set, const bbk_hamclusters *hamclusters,
                               const bbk_kmerstats *kmerstats, const bbk_subcluster_params *p, bbk_subclusters **out);
uint64_t bbk_subclusters_count(const bbk_subclusters *s);      /* subclusters (empty lists are dropped, :505) */
uint64_t bbk_subclusters_size(const bbk_subclusters *s);       /* entries of all lists together */
uint64_t bbk_subclusters_new_kmers(const bbk_subclusters *s);  /* "non-read kmers" (:650) */
uint64_t bbk_subclusters_host_kmers(const bbk_subclusters *s); /* k-mers of the clusters that went through the host path */
/* Every pointer may be NULL.  h_good: n + new bytes, KMerStat::good() of every k-mer, the new ones last; h_members: size
 * entries, the k-mers subcluster by subcluster (clusters in their order), the center first (blocksInPlace, :493-510), a
 * new k-mer as n + j; h_sizes: count entries; h_per_cluster: the subclusters of every Hamming cluster (1 for a
 * singleton); h_new_keys: new entries; h_bic: the best BIC (bestLikelihood, :305-328) of every Hamming cluster, -inf
 * for a singleton; h_errs[16]: UpdateErrors (:448-453,564), errs[4 * center[i] + kmer[i]] over all positions of every
 * non-center entry; h_stats[9]: gsingl, tsingl, tcsingl, gcsingl, tcls, gcls, tkmers, tncls, newkmers (:592,650-657). */
int bbk_subclusters_export(bbk_ctx *ctx, const bbk_subclusters *s, uint8_t *h_good, uint64_t *h_members, uint64_t *h_sizes,
                           uint64_t *h_per_cluster, uint64_t *h_new_keys, double *h_bic, uint64_t *h_errs,
                           uint64_t *h_stats);
/* <prefix>.kmstat as bbk_kmerstats_write, with the good bit in bit 0 of the count word and the records of the new k-mers
 * (count 0, total_qual 1, no qualities) after the others (KMerData::push_back, kmer_data.hpp); <prefix>.subclusters /
 * .subclusters.idx: h_members / h_sizes as u64, like <path> / <path>.idx of bbk_hamclusters_write; <prefix>.newkmers:
 * the new k-mers, one u64 record each like <prefix>.kmers of spades-kmerdata. */
int bbk_subclusters_write(bbk_ctx *ctx, const bbk_subclusters *s, const bbk_kmerstats *ks, const char *prefix);
void bbk_subclusters_free(bbk_subclusters *s);

/* ---- expansion of the solid k-mers: replaces Expander::operator() (projects/hammer/expander.cpp:20-70) and the loop
 *      around it (projects/hammer/main.cpp:194-222) -- every read that is covered end to end by good k-mers makes all of
 *      its k-mers good, again and again until little changes; what is left is the kmer.index3 ReadCorrector reads -------- */
typedef struct bbk_expander bbk_expander; /* good bits of a set, two generations, in HBM */
/* set: as for bbk_kmerstats_begin (ascending BBK_BOTH_STRANDS, k <= 32, fewer than 2^32 - 2 k-mers); it must outlive the
 * expander, and the lookup index over it is built here, once.  The bits of the first n k-mers of `sc` (the new k-mers
 * are never found from a read: KMerData::checking_seq_idx, kmer_data.hpp), or h_good: n bytes, 0 or 1.
 * BBK_ERR_ARG: a set the stage refuses, subclusters of another n or k, a byte other than 0 or 1. */
int bbk_expander_from_subclusters(bbk_ctx *ctx, const bbk_kmerset *set, const bbk_subclusters *sc, bbk_expander **out);
int bbk_expander_from_host(bbk_ctx *ctx, const bbk_kmerset *set, const uint8_t *h_good, bbk_expander **out);
/* One iteration of main.cpp:198-221 as a SNAPSHOT ROUND: every read pushed between round_begin and
 * round_end is judged against the bits G_r the round began with, and the marks go to the next generation.  A read of sz
 * bases (one run of ACGT: the caller pushes the reads that can ever be solid, trimmed -- bbk_hreads_candidate_view,
 * or host/hammer_reads.hpp expander_candidate; sz < k: ignored, expander.cpp:27-28) has the starts 0 .. nk - 1, nk = sz - k + 1.  It is solid when
 * start 0 and start nk - 1 are in the set and good in G_r and no two consecutive good starts are more than k apart
 * (covered_by_solid all true, :30-51); only the forward k-mer is looked up (:36), and a start whose k-mer is not in the
 * set neither covers nor is marked (:37,54-55).  G_{r+1} = G_r with every k-mer, present in the set, of every solid read
 * (:53-67); *changed = |G_{r+1} \ G_r|, distinct k-mers (changed_ of one thread, :59-61).  Unlike the reference, where a
 * mark is seen by the reads after it in thread-timing order, the result is the same bytes for any order and batching
 * of the reads; the reference's state after t passes of one thread lies between G_t and the closure, which both reach.
 * h_status (n_reads bytes, or NULL): 0 not solid, 1 solid, 2 every start already good.  push does not wait for the
 * device unless h_status is given, so the reads must stay alive until round_end, which waits once, or a
 * bbk_ctx_synchronize.
 * BBK_ERR_ARG: push or round_end outside a round, round_begin inside one. */
int bbk_expander_round_begin(bbk_expander *e);
int bbk_expander_push(bbk_expander *e, const bbk_reads *reads, uint8_t *h_status /* n_reads bytes or NULL */);
int bbk_expander_round_end(bbk_expander *e, uint64_t *changed);
/* reads resident: rounds until changed < min_changed or max_rounds (expand_max_iterations 25 and the 10 of
 * main.cpp:219); *rounds: how many ran; h_changed: max_rounds entries or NULL, the first *rounds are written.  One host
 * wait per round.  BBK_ERR_ARG: max_rounds 0, a round is open. */
int bbk_expander_run(bbk_expander *e, const bbk_reads *reads, unsigned max_rounds, uint64_t min_changed,
                     unsigned *rounds, uint64_t *h_changed);
uint64_t bbk_expander_good(const bbk_expander *e); /* good k-mers now (at the start of the open round) */
int bbk_expander_export(bbk_ctx *ctx, const bbk_expander *e, uint8_t *h_good); /* n bytes */
/* the n bits back into sc (KMerData is one object: Expander marks the KMerStat the subclustering wrote): afterwards
 * bbk_subclusters_export / _write give the expanded bits for the first n k-mers; the bits of the new k-mers and every
 * other field are untouched.  BBK_ERR_ARG: subclusters of another n or k, a round is open. */
int bbk_expander_store(bbk_expander *e, bbk_subclusters *sc);
void bbk_expander_free(bbk_expander *e);

/* ---- read correction: replaces ReadCorrector::CorrectOneRead / CorrectReadRight (projects/hammer/read_corrector.cpp:49-245)
 *      and CorrectReadsBatch (projects/hammer/hammer_tools.cpp:79-105) -- the consumer of the good bits: every read is
 *      corrected outwards from its longest run of solid k-mers ----------------------------------------------------------- */
typedef struct bbk_corrector bbk_corrector; /* a set's lookup index and a copy of its good bits, in HBM */
/* set: as for bbk_expander_* (ascending BBK_BOTH_STRANDS, k <= 32, fewer than 2^32 - 2 k-mers); it must outlive the
 * corrector.  The bits are those of the expander now (copied: the expander may go on or be freed), or h_good: n bytes.
 * BBK_ERR_ARG: a set the stage refuses, a byte other than 0 or 1, an expander with an open round or of another n or k. */
int bbk_corrector_from_expander(bbk_ctx *ctx, const bbk_kmerset *set, const bbk_expander *e, bbk_corrector **out);
int bbk_corrector_from_host(bbk_ctx *ctx, const bbk_kmerset *set, const uint8_t *h_good, bbk_corrector **out);
/* The fixed capacities of a search on the device: a search whose queue would hold more than *heap_cap
 * states after a flush, or that pops more than *pop_cap states, is done by the host rule instead -- with the same result. */
void bbk_corrector_limits(unsigned *heap_cap, unsigned *pop_cap);
/* CorrectReadsBatch over n_reads TRIMMED reads (what Read::trimNsAndBadQuality left; the generator's own q < 2 trimming
 * is applied here): read i is h_bases[h_offsets[i] .. h_offsets[i + 1]), ASCII, any byte other than A, C, G, T is a
 * non-nucleotide; h_qual holds one quality per base with the offset already subtracted.  h_out (same layout) receives the
 * corrected reads, h_result[i] the flag of CorrectOneRead.  A read shorter than k is copied, gets 0 and is not counted
 * (hammer_tools.cpp:90-95).  Per read (:160-245): the longest run of consecutive valid starts (ValidKMerGenerator, bad
 * quality 2) whose k-mer is in the set and good is the solid island [lleft, lright] -- the earliest of equal runs (:185);
 * with 0 < solid_len < size the read is corrected to the right of lright, then its reverse complement to the right of
 * size - 1 - lleft (:206-208), and the flag is 1; otherwise the flag is solid_len == size.  A search (:66-158) is
 * best-first over std::priority_queue ordered by (penalty, pos): keeping the read's base costs 0 / 1 / 2 / 2 / 3 (good;
 * present with q >= 20 / q < 20; absent with q >= 20 / q < 20) and forgets the positions of earlier corrections (the
 * outer cpos, :70,98,104); no correction is tried after a good base of q >= 20, below a penalty of -15 % of the bases to
 * go, or fewer than 8 bases after the fourth-last correction; a correction must give a good k-mer and costs 5 (q >= 20),
 * 1 (q < 20) or 0 (the read has no nucleotide there); the first state that reaches the last base wins; an empty queue
 * leaves the side as it was and counts its bases as uncorrected.  States of equal (penalty, pos) leave the queue in the
 * order of libstdc++'s push_heap / pop_heap, which the device's heap follows step for step.
 * h_where (n_reads bytes, or NULL): 0 no search, 1 searched on the device, 2 a search of the read went through the host
 * rule (capacities above, or BBK_CORRECTOR_HOST=1 in the environment, which sends every search there).  The call waits.
 * The reads are prepared with BBK_NO_TRIM (below: uploaded, the generator's stretches cut on the device), then the call is
 * bbk_corrector_correct_prepared; its output offsets are h_offsets less h_offsets[0].
 * BBK_ERR_ARG: descending offsets, a quality above 93, a read of more than 65535 bases (positions are 16 bits, :20). */
int bbk_corrector_correct(bbk_corrector *c, const char *h_bases, const uint8_t *h_qual, const uint64_t *h_offsets,
                          uint64_t n_reads, char *h_out, uint8_t *h_result, uint8_t *h_where);
/* summed over the calls so far: changed reads, changed nucleotides, uncorrected nucleotides, total nucleotides
 * (CorrectionStats, hammer_tools.cpp:98-104), and the searches that went through the host rule */
int bbk_corrector_stats(const bbk_corrector *c, uint64_t stats[5]);
void bbk_corrector_free(bbk_corrector *c);

/* ---- prepared reads: replaces Read::trimNsAndBadQuality / trimLeftRight (common/io/reads/read.hpp:87-122) followed by
 *      ValidKMerGenerator<K>(read, 2) (projects/hammer/valid_kmer_generator.hpp:147-199), the step KMerDataFiller
 *      (projects/hammer/kmer_data.cpp:163-186), Expander (projects/hammer/expander.cpp:20-29) and ReadCorrector
 *      (projects/hammer/read_corrector.cpp:160-176) all begin with -- FASTQ records as parsed go in, and what the count,
 *      the statistics, the expansion and the correction consume comes out, resident in HBM --------------------------- */
typedef struct bbk_hreads bbk_hreads; /* a batch of records as parsed, their trims, stretches and candidate flags */
/* Record i is h_bases[h_offsets[i] .. h_offsets[i + 1]) (n + 1 offsets), any byte values; h_qual holds one quality per
 * base with the offset already subtracted (Read's qual_).  Per record the batch keeps, on the device:
 *   the trim    (start, length) of what trimNsAndBadQuality(trim_quality) leaves, in the record as parsed (read.hpp:87-122;
 *               a left trim suppresses the right trim, :114); (0, 0): nothing is left.  Read::print's ltrim_ / rtrim_
 *               (:221-236) are start and start + length, or 0 and the record's size when nothing is left;
 *   two tables  the valid starts of ValidKMerGenerator<k>(trimmed read, 2), consecutive starts a..b as one stretch
 *               (a, b - a + k).  The k-mer table takes ACGTacgt for nucleotides (common/sequence/nucl.hpp:45-62), its
 *               starts are in the record as parsed, and it is empty for a trimmed read of fewer than k bases
 *               (kmer_data.cpp:171): what KMerDataFiller and Expander see.  The corrector table takes ACGT only and its
 *               starts are in the trimmed read: what bbk_corrector_correct computes for the same trimmed reads;
 *   the flag    1 when the k-mer table holds exactly one stretch and that is the whole trimmed read: the records
 *               Expander::operator() can ever find solid (expander.cpp:30-51).
 * trim_quality BBK_NO_TRIM: the records are trimmed already and are taken whole -- every trim is (0, size) -- and the
 * tables and the flag are those of a trimmed read of these bases; the trimmed layout of such a batch is the batch itself,
 * so nothing is gathered for the corrector or the printer.  It is the one value of trim_quality that is not a quality.
 * BBK_ERR_ARG: k outside 1..32, descending offsets, a quality above 93, a record of 2^31 bases or more. */
#define BBK_NO_TRIM (-2147483647 - 1) /* INT_MIN */
int bbk_hreads_from_host(bbk_ctx *ctx, const char *h_bases, const uint8_t *h_qual, const uint64_t *h_offsets, uint64_t n,
                         unsigned k, int trim_quality, bbk_hreads **out);
uint64_t bbk_hreads_size(const bbk_hreads *hr);               /* records */
uint64_t bbk_hreads_kmer_stretches(const bbk_hreads *hr);      /* S_k: stretches of the k-mer table */
uint64_t bbk_hreads_corrector_stretches(const bbk_hreads *hr); /* S_c: stretches of the corrector table */
uint64_t bbk_hreads_candidates(const bbk_hreads *hr);
/* Any pointer may be NULL.  h_trim: 2n u32 (start, length); h_candidate: n bytes; h_koff / h_coff: n + 1 entries, the
 * stretches of record i are [off[i], off[i + 1]); h_kst / h_cst: (start, length) u32 pairs, 2 S_k / 2 S_c values. */
int bbk_hreads_export(bbk_ctx *ctx, const bbk_hreads *hr, uint32_t *h_trim, uint8_t *h_candidate, uint64_t *h_koff,
                      uint32_t *h_kst, uint64_t *h_coff, uint32_t *h_cst);
/* One engine read per stretch of the k-mer table with its qualities (what KMerDataFiller pushes, kmer_data.cpp:172-183):
 * for bbk_count_push_reads and bbk_kmerstats_push.  Packed on the device from the resident bytes on the first call,
 * then cached; the batch owns both, they die with it and must not be freed.  quals may be NULL. */
int bbk_hreads_stretch_view(const bbk_hreads *hr, const bbk_reads **reads, const bbk_quals **quals);
/* The trimmed read of every candidate (expander.cpp:20-29), for bbk_expander_push / bbk_expander_run; owned and cached
 * like the stretch view. */
int bbk_hreads_candidate_view(const bbk_hreads *hr, const bbk_reads **reads);
/* CorrectReadsBatch (hammer_tools.cpp:79-105) over the trimmed reads of the batch: the bases, the qualities and the
 * corrector table are the resident ones (bbk_corrector_correct is this call on a BBK_NO_TRIM batch).  h_out receives the
 * corrected trimmed reads back to back, read i at [h_out_offsets[i], h_out_offsets[i + 1]) (n + 1 entries, from 0; the
 * caller sizes h_out for the bases of the batch, which no trim exceeds); h_result, h_where and the counters are those
 * of bbk_corrector_correct on the same trimmed reads.  h_where may be NULL.
 * BBK_ERR_ARG: a batch made for another k than the corrector's, a record of more than 65535 bases. */
int bbk_corrector_correct_prepared(bbk_corrector *c, const bbk_hreads *hr, char *h_out, uint64_t *h_out_offsets,
                                   uint8_t *h_result, uint8_t *h_where);
void bbk_hreads_free(bbk_hreads *hr);
/* The records of a batch as it holds them.  Any pointer may be NULL.  h_bases / h_quals: bbk_hreads_bases bytes each (the
 * qualities with the offset subtracted); h_offsets: n + 1 entries from 0; h_names: bbk_hreads_name_bytes bytes, name i at
 * [h_name_off[i], h_name_off[i + 1]) (n + 1 entries from 0).  A batch made from host arrays holds no names: 0 bytes, every
 * offset 0. */
uint64_t bbk_hreads_bases(const bbk_hreads *hr);
uint64_t bbk_hreads_name_bytes(const bbk_hreads *hr);
int bbk_hreads_export_records(bbk_ctx *ctx, const bbk_hreads *hr, char *h_bases, uint8_t *h_quals, uint64_t *h_offsets,
                              char *h_names, uint64_t *h_name_off);

/* ---- FASTQ text parsed on the device: replaces FastaFastqGzParser over kseq (common/io/reads/
 *      fasta_fastq_gz_parser.hpp:64-80,113-136; ext/include/kseq/kseq.h:170-212) for input in the four-line form, and says
 *      where the input stops being in that form so that the serial reader can take over there -- text blocks go in (plain
 *      bytes, after any gunzip), prepared batches with their names come out, resident in HBM ------------ */
typedef struct bbk_fastq_input bbk_fastq_input; /* one chunk of FASTQ text on the device, with its index */
#define BBK_FASTQ_FORM 1    /* verdict kind: the record is not in the strict four-line form */
#define BBK_FASTQ_QUALITY 2 /* verdict kind: a quality byte outside [qvoffset, qvoffset + 93] */
/* Uploads h_text[0 .. n_bytes) and indexes it.  Lines end at '\n'; with final == 0 only terminated lines count (the
 * caller carries the rest into its next chunk), with final != 0 a non-empty unterminated tail is the last line.  Record r
 * is lines 4r .. 4r + 3, and there are lines / 4 records.  A record is in the strict form -- exactly then kseq
 * (kseq.h:170-212) reads the four lines as name, sequence and quality -- when line 4r begins with '@', line 4r + 1 is empty or
 * begins with none of '@', '+', '>', line 4r + 2 begins with '+', and the sequence and the quality line are equally long
 * after one trailing '\r' has been dropped from a field of more than one byte (ks_getuntil2; the name, the header line
 * without its first byte, loses it the same way).  The verdict is the smallest record index that is not in the strict
 * form (kind BBK_FASTQ_FORM) or, being in it, holds a quality byte outside [qvoffset, qvoffset + 93] (BBK_FASTQ_QUALITY);
 * with final != 0 leftover lines (lines % 4 != 0) make the record after the last one a BBK_FASTQ_FORM verdict.
 * BBK_ERR_ARG: a NULL argument, qvoffset outside 0..162, a chunk of 2^40 bytes or more. */
int bbk_fastq_input_from_host(bbk_ctx *ctx, const char *h_text, uint64_t n_bytes, int final, int qvoffset,
                              bbk_fastq_input **out);
uint64_t bbk_fastq_input_records(const bbk_fastq_input *in); /* complete records: lines / 4 */
/* Returns 1 and fills *record, *kind and *byte (the first offending quality character of a BBK_FASTQ_QUALITY verdict,
 * otherwise -1) when there is a verdict, 0 when every record is usable; any pointer may be NULL. */
int bbk_fastq_input_verdict(const bbk_fastq_input *in, uint64_t *record, int *kind, int *byte);
/* The byte just past record n - 1 (0 for n == 0; n_bytes for a last record without its line feed): where the caller's next
 * chunk starts, or where the serial reader resumes, between records.  ~0 for n above the record count. */
uint64_t bbk_fastq_input_text_end(const bbk_fastq_input *in, uint64_t n);
/* The block rule of a reader that closes a block with the record at which its bases reach max_bases: the number of
 * records from `first` up to and including that one, or all the usable records behind `first` when they do not get there.
 * Usable records are those before the verdict. */
uint64_t bbk_fastq_input_records_within(const bbk_fastq_input *in, uint64_t first, uint64_t max_bases);
void bbk_fastq_input_free(bbk_fastq_input *in);
/* bbk_hreads_from_host for the records [first, first + n) of the index, gathered on the device: the bases with a..z
 * upper-cased (kseq.h:193-194), the qualities with qvoffset subtracted, and the names, which the batch keeps
 * (bbk_hreads_export_records, bbk_corrected_print_resident).  Every position comes from a scan, so the bytes are the same on
 * every run.  The batch does not borrow the index.
 * BBK_ERR_ARG: k outside 1..32, a range that reaches the verdict or the end of the records, a record of 2^31 bases or a
 * name of 2^30 bytes or more. */
int bbk_hreads_from_fastq_input(const bbk_fastq_input *in, uint64_t first, uint64_t n, unsigned k, int trim_quality,
                                bbk_hreads **out);

/* ---- corrected reads as FASTQ text: replaces the last step of CorrectAllReads (projects/hammer/hammer_tools.cpp:107-193:
 *      CorrectReadFile, CorrectPairedReadFiles), the BH: tags of ReadCorrector::CorrectOneRead
 *      (projects/hammer/read_corrector.cpp:214-242) and Read::print (common/io/reads/read.hpp:221-236) -- the outcome of a
 *      batch stays in HBM, and the text of every output file is formatted there ------------------------------------------ */
typedef struct bbk_corrected bbk_corrected;   /* what CorrectReadsBatch made of a prepared batch, resident */
typedef struct bbk_fastq_text bbk_fastq_text; /* the FASTQ text of one or two corrected batches, stream by stream */
/* bbk_corrector_correct_prepared with the result kept on the device (hammer_tools.cpp:79-105): the corrected trimmed
 * reads in the batch's trimmed layout, the flag of CorrectOneRead and the `where` byte of every read; the counters of
 * the corrector advance as they do there.  A search that goes through the host rule (bbk_corrector_limits, or
 * BBK_CORRECTOR_HOST=1) is copied back into the device's reads before the call returns, the bases it may touch and no
 * others.  The result borrows hr, which must outlive it.  BBK_ERR_ARG: as bbk_corrector_correct_prepared. */
int bbk_corrector_correct_resident(bbk_corrector *c, const bbk_hreads *hr, bbk_corrected **out);
uint64_t bbk_corrected_size(const bbk_corrected *cr); /* records */
/* Any pointer may be NULL.  h_out, h_out_offsets (n + 1), h_result, h_where: as bbk_corrector_correct_prepared gives
 * them; h_changed: n u32, the positions where the corrected read differs from the trimmed read (read_corrector.cpp:210-212);
 * h_tag: n bytes, the tag correct_stats 1 puts behind the read's name (:214-242): 0 none (fewer than k bases are left, or
 * no search ran and the flag is 0), 1 " BH:ok" (no search, flag 1), 2 " BH:failed" (searched, nothing changed),
 * 3 " BH:changed:<h_changed>". */
int bbk_corrected_export(bbk_ctx *ctx, const bbk_corrected *cr, char *h_out, uint64_t *h_out_offsets, uint8_t *h_result,
                         uint8_t *h_where, uint32_t *h_changed, uint8_t *h_tag);
void bbk_corrected_free(bbk_corrected *cr);
/* Read::print (read.hpp:221-236) of every record of `left` -- and of `right`, its mates, when that is not NULL -- routed as
 * CorrectReadFile (hammer_tools.cpp:135-137) or CorrectPairedReadFiles (:178-186) route them.  Record i is
 *   @<name><tag>\n N^ltrim <corrected trimmed read> N^tail \n +<name><tag>[ ltrim=<ltrim>][ rtrim=<tail>]\n
 *   (qvoffset + 2)^ltrim <qualities + qvoffset> (qvoffset + 2)^tail \n
 * with ltrim / tail from the batch's trim table (nothing left: no padding, two empty lines) and the tag only when `tags`
 * is not 0.  Names: h_names_* is a byte blob, name i of a side is [h_name_off[i], h_name_off[i + 1]) (n + 1 offsets);
 * both are copied by the call.  Streams: one batch gives 0 good (flag 1) and 1 bad; a pair gives 0 cor-left and 1 cor-right
 * (both flags 1), 2 unpaired (the mate with flag 1 of any other pair), 3 bad-left, 4 bad-right.  Inside a stream the
 * records keep the order (index, left before right); positions come from a scan, so the bytes are the same on every run.
 * BBK_ERR_ARG: a NULL argument, left and right of different sizes or contexts, descending name offsets, a name of 2^30
 * bytes or more, a line feed inside a name, qvoffset outside 0..162 (93 + qvoffset must fit a byte). */
int bbk_corrected_print(const bbk_corrected *left, const bbk_corrected *right, const char *h_names_l,
                        const uint64_t *h_name_off_l, const char *h_names_r, const uint64_t *h_name_off_r, int qvoffset,
                        int tags, bbk_fastq_text **out);
/* bbk_corrected_print with the names taken from the batches' own blobs (batches made by bbk_hreads_from_fastq_input): nothing
 * is uploaded.  BBK_ERR_ARG also for a batch that holds no names. */
int bbk_corrected_print_resident(const bbk_corrected *left, const bbk_corrected *right, int qvoffset, int tags,
                                 bbk_fastq_text **out);
int bbk_fastq_text_streams(const bbk_fastq_text *t); /* 2 or 5 */
uint64_t bbk_fastq_text_size(const bbk_fastq_text *t, int stream); /* bytes; 0 for a stream the text does not have */
/* stream `stream` into h_dst (bbk_fastq_text_size bytes) / into the file `path` through the context's staged copy: the
 * file is replaced, or with append != 0 the bytes go behind what it holds (std::ofstream of hammer_tools.cpp:206-258,
 * one batch after the other).  BBK_ERR_ARG: a stream index out of range. */
int bbk_fastq_text_export(bbk_ctx *ctx, const bbk_fastq_text *t, int stream, char *h_dst);
int bbk_fastq_text_write(bbk_ctx *ctx, const bbk_fastq_text *t, int stream, const char *path, int append);
void bbk_fastq_text_free(bbk_fastq_text *t);


/* ---- several GPUs of one node in one process (bbk_ctx_create(devices, ndev); 8e: the exchange) --------
 * The reference tools are one process for the whole job with hash buckets owned by worker threads
 * (projects/kmercount/main.cpp:186-228, utils/kmer_mph/kmer_buckets.hpp:28-33); here the owner of a canonical k-mer is a
 * GPU, owner(key) = mulhi(mix(key), ndev).  A group names the devices and holds what they need to talk to each other;
 * every rank is driven by ITS OWN host thread, which creates its context with bbk_ctx_create(bbk_group_device(g, rank))
 * and makes all calls for that rank.  The bbk_group_* calls below that take a rank are COLLECTIVE: every rank's thread
 * calls them once, in the same order (like the grouped ncclSend/ncclRecv they issue).  If a rank fails inside one, the
 * others return BBK_ERR_INTERNAL instead of waiting for ever. */
typedef struct bbk_group bbk_group;
#define BBK_EXCHANGE_RCCL 0u /* one grouped ncclSend/ncclRecv all-to-all over xGMI, messages <= 256 MiB (librccl is loaded
                                at this point, not before; devices must be distinct) */
#define BBK_EXCHANGE_COPY 1u /* the same segments moved by peer copies (hipMemcpyPeerAsync); ranks may share a device:
                                the way to run the N-rank path on one GPU */
int bbk_group_create(const int *devices, int ndev, unsigned exchange, bbk_group **out);
int bbk_group_size(const bbk_group *g);
int bbk_group_device(const bbk_group *g, int rank);
void bbk_group_destroy(bbk_group *g);
/* a rank that cannot reach its next collective call (input error, ...) tells the others */
void bbk_group_abort(bbk_group *g);
/* local: this rank's distinct canonical k-mers in any order (bbk_count*(BBK_CANONICAL | BBK_UNSORTED [| BBK_WITH_COUNTS]))
 * -> *shard: the canonical k-mers this rank owns, merged over all ranks (multiplicities summed);
 * flags: BBK_UNSORTED keeps hash-bucket order (enough for bbk_kmerset_both_strands_ex), 0 sorts ascending. */
int bbk_group_exchange_kmers(bbk_group *g, int rank, bbk_ctx *ctx, const bbk_kmerset *local, unsigned flags,
                             bbk_kmerset **shard);
/* local: BBK_CANONICAL | BBK_UNSORTED | BBK_WITH_MASKS records -> this rank's shard of the extension index (ascending
 * canonical k-mers it owns with their complete InOutMask): "ext records follow their k-mer's owner, no second exchange" */
int bbk_group_exchange_extindex(bbk_group *g, int rank, bbk_ctx *ctx, const bbk_kmerset *local_masks,
                                bbk_extindex **shard);
/* all shards -> one index on rank dst (*full; NULL on the other ranks): the unitig walk crosses owners */
int bbk_group_gather_extindex(bbk_group *g, int rank, bbk_ctx *ctx, const bbk_extindex *shard, int dst,
                              bbk_extindex **full);
/* the same for a sharded set with multiplicities -> one ascending set on rank dst (gbuilder -c: the (k+1)-mer counts) */
int bbk_group_gather_kmers(bbk_group *g, int rank, bbk_ctx *ctx, const bbk_kmerset *shard, int dst, bbk_kmerset **full);

/* Device memory of the allocator: *mapped_now = bytes the calling thread's arenas on the context's device hold mapped;
 * *mapped_total / *map_seconds = bytes mapped, and seconds spent mapping, since the process started, by every thread on
 * every device (growth is what a first call pays: ~30 ms/GiB when the driver has to clear the memory first); and the
 * device's free / total bytes as the driver reports them.  Any pointer may be NULL. */
int bbk_ctx_memory_stats(bbk_ctx *ctx, uint64_t *mapped_now, uint64_t *mapped_total, double *map_seconds,
                         uint64_t *device_free, uint64_t *device_total);
/* What the engine found on the device at bbk_ctx_create: compute units, and the XCDs a probe launch's workgroups were seen
 * on (HW_REG_XCC_ID).  The partition kernels keep one fill front per (segment, XCD) and deal level-2 tiles to the XCDs by
 * segment when that is eight (an MI355X in SPX mode); any other value -- a partitioned device -- switches both off.
 * Placement only: results never depend on it.  (Diagnostics; no reference counterpart.) */
int bbk_ctx_device_info(bbk_ctx *ctx, int *num_cus, int *num_xcds);
/* XXH3 bucket boundaries of a set stored in the final_kmers order: h_offsets[b] = first record of bucket b (b = 0..16,
 * h_offsets[16] = size); what a writer that merges several shards into one final_kmers file needs
 * (KMerDiskStorage::merge, kmer_index_builder.hpp:168-181) */
int bbk_kmerset_bucket_offsets(bbk_ctx *ctx, const bbk_kmerset *s, uint64_t *h_offsets);

#ifdef __cplusplus
}
#endif
#endif /* BBK_H_ */
