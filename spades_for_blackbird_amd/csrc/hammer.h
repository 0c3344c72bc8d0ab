// hammer.h -- what hamclust.hip, kmerstat.hip, subclust.hip, expand.hip, readcorrect.hip, hreads.hip, readprint.hip and
// fastqparse.hip (the BayesHammer stage) share.  Host code only: no device arithmetic, so subclust.hip's `fp contract(off)` scope reaches no other translation unit
// through it.
#pragma once

#include <algorithm>
#include <cmath>
#include <string>

#include "bbk_internal.h"
#include "hammer_files.h"

struct bbk_hamclusters {
    uint64_t n = 0, clusters = 0, replayed = 0;
    bbk::DevBuf labels;   // n u32: smallest member index of the cluster of k-mer i
    bbk::DevBuf members;  // n u32: the indices cluster by cluster
    bbk::DevBuf sizes;    // clusters u64
};

struct bbk_kmerstats {
    bbk_ctx *ctx = nullptr;
    const bbk_kmerset *set = nullptr;  // must outlive the statistics
    unsigned k = 0, acc_words = 0, qual_words = 0;
    uint64_t n = 0;
    bool finished = false, count_overflow = false;
    bool loaded = false;  // read from a file (bbk_kmerstats_load): finished for good, there are no accumulators
    bbk::PrefixIndex prefix;
    bbk::DevBuf probs;       // 256 doubles: Globals::quality_probs
    bbk::DevBuf rec;         // n * (2 + acc_words) u64
    bbk::DevBuf count;       // n u32            \.
    bbk::DevBuf total_qual;  // n f32             > written by finish
    bbk::DevBuf qual;        // n * qual_words u64 /
};

struct bbk_subclusters {
    unsigned k = 0;
    uint64_t n = 0, clusters = 0, subs = 0, listed = 0, new_kmers = 0, host_kmers = 0;
    bbk::DevBuf good;         // n + new_kmers u8
    bbk::DevBuf members;      // listed u64: subcluster by subcluster, the center first; a new k-mer is n + j
    bbk::DevBuf sizes;        // subs u64
    bbk::DevBuf per_cluster;  // clusters u64
    bbk::DevBuf new_keys;     // new_kmers u64
    bbk::DevBuf bic;          // clusters double
    uint64_t errs[16] = {0}, stats[9] = {0};
};

struct bbk_expander {
    bbk_ctx *ctx = nullptr;
    const bbk_kmerset *set = nullptr;  // must outlive the expander
    unsigned k = 0;
    uint64_t n = 0, good = 0;
    bool in_round = false;
    bbk::PrefixIndex prefix;
    bbk::DevBuf cur, next;  // n u8 each, zero-padded to a multiple of 16: G_r and G_{r+1}; equal outside a round
    bbk::DevBuf changed;    // one u64
};

struct bbk_quals {
    const bbk_reads *reads = nullptr;  // the reads these belong to (lengths checked against them)
    uint64_t n = 0, bytes = 0;
    bbk::DevBuf q;    // bytes u8, offset already subtracted
    bbk::DevBuf off;  // n + 1 u64
};

// hreads.hip: the records of a batch as parsed, and what Read::trimNsAndBadQuality and ValidKMerGenerator<K>(read, 2)
// make of them
struct bbk_hreads {
    bbk_ctx *ctx = nullptr;
    unsigned k = 0;
    int trim_quality = 0;
    uint64_t n = 0, bytes = 0;  // records; bases (= qualities) of all of them
    uint64_t longest = 0;       // bases of the longest record
    uint64_t n_kst = 0, n_cst = 0, n_cand = 0;
    bbk::DevBuf bases, quals;  // bytes u8 each, as parsed (quals: offset already subtracted)
    bbk::DevBuf off;           // n + 1 u64
    bbk::DevBuf trim;          // n x (start, length) u32, in the record as parsed; (0, 0): nothing is left
    bbk::DevBuf cand;          // n u8: expander_candidate
    bbk::DevBuf koff, kst;     // n + 1 u64; n_kst x (start, length) u32: the k-mer table, starts in the record as parsed
    bbk::DevBuf coff, cst;     // n + 1 u64; n_cst x (start, length) u32: the corrector table, starts in the trimmed read
    bbk::DevBuf cpos;          // n + 1 u64: candidates before record i
    // a batch gathered from FASTQ text (fastqparse.hip) also keeps the names; a batch made from host arrays has none
    bool has_names = false;
    uint64_t name_bytes = 0;
    bbk::DevBuf names, name_off;  // name_bytes u8 back to back; n + 1 u64
    // made on first request, freed with the batch (mutable: a cache behind a const handle, one host thread per context)
    struct View {
        bool made = false;
        bbk_reads reads;
        bbk_quals quals;
    };
    mutable View stretch_view, candidate_view;
    struct Trimmed {  // the trimmed reads back to back, what the corrector's kernels and the printer read
        bool made = false;
        const uint8_t *bases = nullptr, *quals = nullptr;  // total u8 each
        const uint64_t *off = nullptr;                     // n + 1
        uint64_t total = 0;
        bbk::DevBuf own_bases, own_quals, own_off;  // the gather; empty for a BBK_NO_TRIM batch, whose own arrays are the layout
    };
    mutable Trimmed trimmed;
};

// readcorrect.hip: what CorrectReadsBatch made of a prepared batch, resident
struct bbk_corrected {
    bbk_ctx *ctx = nullptr;
    const bbk_hreads *hr = nullptr;  // borrowed: the trimmed layout, the qualities and the trims are the batch's
    unsigned k = 0;
    uint64_t n = 0, total = 0;  // records; bases of the trimmed reads
    bbk::DevBuf out;            // total u8: the corrected trimmed reads, at the offsets of hr's trimmed layout
    bbk::DevBuf res, where;     // n u8 each: CorrectOneRead's flag; 0 no search, 1 device, 2 host rule
    bbk::DevBuf changed, tag;   // n u32, n u8: readprint.hip's k_rp_outcome
    uint64_t stats[5] = {0, 0, 0, 0, 0};  // what the batch added to the corrector's counters
};

// readprint.hip: the FASTQ text of one or two corrected batches, stream after stream in one buffer
struct bbk_fastq_text {
    bbk_ctx *ctx = nullptr;
    int streams = 0;        // 2 or 5
    uint64_t start[6] = {0, 0, 0, 0, 0, 0};  // stream s is text[start[s], start[s + 1])
    bbk::DevBuf text;
};

// fastqparse.hip: one chunk of FASTQ text on the device with its index.  Line i is
// text[ls[i], ls[i + 1] - 1): ls[i + 1] is one past the line feed, or n_bytes + 1 behind an unterminated last line.
struct bbk_fastq_input {
    bbk_ctx *ctx = nullptr;
    uint64_t n_bytes = 0, lines = 0, records = 0;
    int qvoffset = 0;
    uint64_t usable = 0;             // records before the verdict (all of them without one)
    uint64_t verdict = ~0ull;        // record << 2 | kind, ~0: none
    int verdict_byte = -1;           // the first offending quality character of a quality verdict
    uint64_t oversize = ~0ull;       // the first record of 2^31 bases or with a name of 2^30 bytes or more
    bbk::DevBuf text;                // n_bytes u8
    bbk::DevBuf ls;                  // lines + 1 u64
    bbk::DevBuf seq0, qual0, name0;  // records u64: the first byte of the three fields in text
    bbk::DevBuf boff, noff;          // records + 1 u64: bases / name bytes before record i
    bbk::raw_vector<uint64_t> h_boff;  // boff on the host: the block rule and the limits read it
};

namespace bbk {

// hreads.hip: the prepare tail of a batch whose bases, quals and off are on the device (queued on the context's stream is
// enough): trims, flags and both stretch tables; waits for the stream.  `fn` / `unit` as below
void hreads_prepare(const char *fn, const char *unit, bbk_hreads *hr);
// hreads.hip: fills hr->trimmed on first use (two launches, one scan, one wait; nothing for a BBK_NO_TRIM batch)
const bbk_hreads::Trimmed &hreads_trimmed(const bbk_hreads *hr);
// hreads.hip: bbk_hreads_from_host behind its NULL checks, for the entry `fn`, which calls a record a `unit` in its refusals
std::unique_ptr<bbk_hreads> hreads_from_host(const char *fn, const char *unit, bbk_ctx *ctx, const char *h_bases,
                                             const uint8_t *h_qual, const uint64_t *h_offsets, uint64_t n, unsigned k,
                                             int trim_quality);
// readprint.hip: fills cr->changed and cr->tag from cr->out, res and where (one launch, no wait)
void corrected_outcome(bbk_corrected *cr);

// The k-mer sets of the stage: one-word keys, ascending, k-mer indices in 32 bits with two values to spare.  BBK_CANONICAL
// is not judged here: the statistics refuse a canonical set by its flag, the clustering by its closure check.
inline void require_hammer_count(const char *fn, uint64_t n) {
    BBK_REQUIRE(n < (1ull << 32) - 2, BBK_ERR_ARG, "%s: %llu k-mers: fewer than 2^32 - 2 are needed", fn, (unsigned long long)n);
}
inline void require_hammer_set(const char *fn, const bbk_kmerset *set) {
    BBK_REQUIRE(set->k <= 32, BBK_ERR_ARG, "%s: k = %u: one-word keys only (k <= 32)", fn, set->k);
    BBK_REQUIRE(set->sorted, BBK_ERR_ARG, "%s: the set was built with BBK_UNSORTED: an ascending set is needed", fn);
    BBK_REQUIRE(!set->ref_order, BBK_ERR_ARG, "%s: the set is in the final_kmers order (BBK_REFERENCE_ORDER), not ascending", fn);
    require_hammer_count(fn, set->n);
}

// Globals::quality_probs / quality_rprobs (projects/hammer/main.cpp:103-108): the error probability of a base of quality q.
// Host only; 1 - r (kmerstat.hip), log(1 - r) and log(r) - log(3) (subclust.hip) feed results that are pinned bit for bit.
inline double hammer_error_prob(unsigned q) { return q < 3 ? 0.75 : pow(10.0, -(int)q / 10.0); }

// A host array into a fresh device buffer, asynchronously: the caller waits for the stream before the host memory dies.
template <class T>
void upload(bbk_ctx *ctx, DevBuf &dst, const T *src, uint64_t count) {
    dst.alloc(count * sizeof(T));
    if (count) BBK_HIP(hipMemcpyAsync(dst.p, src, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
}

inline FILE *open_file(const std::string &path, bool writing) {
    FILE *f = fopen(path.c_str(), writing ? "wb" : "rb");
    BBK_REQUIRE(f, BBK_ERR_IO, writing ? "cannot open %s for writing" : "cannot open %s", path.c_str());
    return f;
}
inline void write_u64_file(const std::string &path, const uint64_t *p, uint64_t count) {
    FILE *f = open_file(path, true);
    const bool ok = count == 0 || fwrite(p, 8, count, f) == count, closed = fclose(f) == 0;
    BBK_REQUIRE(ok && closed, BBK_ERR_IO, "writing %s failed", path.c_str());
}
inline void read_u64_file(const std::string &path, const char *fn, raw_vector<uint64_t> &v) {
    FILE *f = open_file(path, false);
    fseek(f, 0, SEEK_END);
    const long long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize(bytes > 0 && bytes % 8 == 0 ? (size_t)bytes / 8 : 0);
    const bool ok = v.empty() || fread(v.data(), 8, v.size(), f) == v.size();
    fclose(f);
    BBK_REQUIRE(bytes >= 0 && bytes % 8 == 0, BBK_ERR_ARG, "%s: %s is not a file of 64-bit values", fn, path.c_str());
    BBK_REQUIRE(ok, BBK_ERR_IO, "reading %s failed", path.c_str());  // both after fclose: a refusal leaves no file open
}

// The KMerStat records of ks, then new_kmers records of new k-mers, into `path`, 2^20 records at a time; good (device,
// n + new_kmers u8, or null) supplies bit 0 of every record.  Refuses a count of 2^31 or more.
inline void write_kmstat(bbk_ctx *ctx, const char *fn, const std::string &path, const bbk_kmerstats *ks, const uint8_t *good,
                         uint64_t new_kmers) {
    BBK_REQUIRE(!ks->count_overflow, BBK_ERR_ARG,
                "%s: a k-mer has 2^31 occurrences or more: the record holds twice the count in 32 bits (kmer_stat.hpp:138-139)", fn);
    BBK_HIP(hipSetDevice(ctx->device));
    const uint64_t block = 1ull << 20, n = ks->n, total = n + new_kmers;
    const unsigned qw = ks->qual_words;
    const size_t rsz = kmstat_record_bytes(qw);
    raw_vector<uint32_t> cnt(std::min(n, block));
    raw_vector<float> tq(cnt.size());
    raw_vector<uint64_t> qv(cnt.size() * qw);
    raw_vector<uint8_t> gd(good ? std::min(total, block) : 0);
    raw_vector<char> buf(std::min(total, block) * rsz);
    FILE *f = open_file(path, true);
    bool ok = true;
    for (uint64_t b = 0; b < total && ok; b += block) {
        const uint64_t m = std::min(total - b, block);              // records of the block
        const uint64_t old = b < n ? std::min(n - b, m) : 0;  // those of them that are k-mers of the set
        if (old) {
            d2h_big(ctx, cnt.data(), ks->count.as<uint32_t>() + b, old * 4);
            d2h_big(ctx, tq.data(), ks->total_qual.as<float>() + b, old * 4);
            d2h_big(ctx, qv.data(), ks->qual.as<uint64_t>() + b * qw, old * qw * 8);
        }
        if (good) d2h_big(ctx, gd.data(), good + b, m);
        kmstat_pack_block(buf.data(), qw, b, m, n, cnt.data(), tq.data(), qv.data(), good ? gd.data() : nullptr);
        ok = fwrite(buf.data(), rsz, m, f) == m;
    }
    const bool closed = fclose(f) == 0;
    BBK_REQUIRE(ok && closed, BBK_ERR_IO, "writing %s failed", path.c_str());
}

}  // namespace bbk
