// spades-kmerdata: BayesHammer's counting phase -- the k-mer set and one KMerStat per k-mer -- on the MI355X engine behind
// the C ABI (include/bbk.h).  Not a drop-in: the reference has this only inside spades-hammer
// (projects/hammer/main.cpp:122-171: KMerDataCounter::BuildKMerIndex, the Hamming clustering, then
// KMerDataCounter::FillKMerData, "Collecting K-mer information, this takes a while"); this tool is that sequence alone.
//   -k/--kmer <int=21>  -t/--threads <int>  -b/--bufsize <bytes>  -o/--output <prefix>  -d/--dataset <yaml>  [input files...]
//   (+ --device <int>, --qvoffset <int=33>, --trim-quality <int=4>, --cluster, --subcluster with --singleton-threshold,
//      --nonsingleton-threshold, --correct-threshold, --no-correct-threshold, --expand with --expand-max-iterations <int=25>,
//      --expand-min-changed <int=10>, --correct, --resident-bytes <bytes=0>)
// The records of every file go to the device as parsed, in blocks of -b bases, and are prepared there (bbk_hreads: the trim
// of input_trim_quality 4 of configs/hammer/config.info, then ValidKMerGenerator's valid starts as stretches); a stretch is
// one read of the engine.  Every pass takes a view of the prepared blocks:
//   pass 1  the stretches through bbk_count_begin / push / finish(BBK_BOTH_STRANDS)
//   pass 2  the same stretches with their qualities through bbk_kmerstats_push
// With --resident-bytes 0 every pass parses the files again; otherwise the blocks of pass 1 stay on the device while their
// bases and qualities total at most that many bytes, and the later passes parse only the blocks behind them.  The output
// files are the same bytes either way.
// Output:
//   <prefix>.kmers        the ascending both-strand k-mers (final_kmers records), as spades-hamcluster writes them: index
//                         i of the other files is record i
//   <prefix>.kmstat       one binary_write(KMerStat) record per k-mer (projects/hammer/kmer_stat.hpp:170-175)
//   <prefix>.hamming, <prefix>.hamming.idx   with --cluster: the Hamming clusters of that set, as spades-hamcluster
//   with --subcluster (KMerClustering::process, projects/hammer/kmer_cluster.cpp:590-659; implies --cluster):
//   <prefix>.kmstat then carries the good bit and the records of the new k-mers, and <prefix>.subclusters,
//   <prefix>.subclusters.idx and <prefix>.newkmers are written (bbk_subclusters_write)
//   with --expand (the solid k-mer expansion, projects/hammer/main.cpp:194-222 and expander.cpp:20-70; implies
//   --subcluster): after the subclustering every round pushes the records the Expander can ever find solid
//   (bbk_hreads_candidate_view), trimmed, block by block through bbk_expander_push, until a
//   round adds fewer than --expand-min-changed k-mers or --expand-max-iterations rounds have run; <prefix>.kmstat then
//   carries the expanded good bits (bbk_expander_store) and every other file is as without --expand
//   with --correct (ReadCorrector, projects/hammer/read_corrector.cpp and hammer_tools.cpp:79-142 CorrectReadFile; implies
//   --expand): after the expansion every input file i is taken once more as a single-read file: every record is trimmed
//   (Read::trimNsAndBadQuality(--trim-quality)), corrected block by block (bbk_corrector_correct_prepared) and printed in
//   the format of Read::print to <prefix>.<i>.cor.fastq (result true) or <prefix>.<i>.bad.fastq
// The records are parsed by one thread (fastx.hpp's next_record, which keeps the quality line); -t is accepted for the
// common interface.
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "common.hpp"

using namespace bbkhost;

static void usage(const char *argv0) {
    printf("SYNOPSIS\n        %s [-k <value>] [-d <file>] [-t <value>] [-b <value>] -o <prefix> [-h] [<input files>]...\n\n"
           "OPTIONS\n"
           "        -k, --kmer <value>      K-mer length (at most 32, default 21)\n"
           "        -d, --dataset <file>    Dataset description (in YAML), input files ignored\n"
           "        -t, --threads <value>   # of threads to use\n"
           "        -b, --bufsize <value>   Bytes of input per block\n"
           "        -o, --output <prefix>   Output prefix\n"
           "        -h, --help              Show help\n"
           "        --device <value>        GPU to use (default 0)\n"
           "        --qvoffset <value>      Quality offset of the input (default 33)\n"
           "        --trim-quality <value>  Ns and bases of at most this quality are trimmed from the ends (default 4)\n"
           "        --cluster               Also cluster the Hamming graph of the k-mers (tau = 1)\n"
           "        --subcluster            Also subcluster the Hamming clusters and mark the solid k-mers (implies --cluster)\n"
           "        --singleton-threshold <value>     bayes_singleton_threshold (default 0.995)\n"
           "        --nonsingleton-threshold <value>  bayes_nonsingleton_threshold (default 0.9)\n"
           "        --correct-threshold <value>       correct_threshold (default 0.98)\n"
           "        --no-correct-threshold            correct_use_threshold 0\n"
           "        --expand                Also expand the solid k-mers over the reads they cover (implies --subcluster)\n"
           "        --expand-max-iterations <value>   expand_max_iterations (default 25)\n"
           "        --expand-min-changed <value>      Stop after an iteration that adds fewer k-mers than this (default 10)\n"
           "        --correct               Also correct the reads with the expanded solid k-mers (implies --expand)\n"
           "        --resident-bytes <value>  Keep the first blocks on the GPU for the later passes while their bases and\n"
           "                                qualities total at most this many bytes (default 0: every pass parses the input)\n\n"
           "DESCRIPTION\n        K-mers of FASTQ reads and their reverse complements with BayesHammer's per-k-mer statistics (MI355X)\n\n"
           "        Output: <prefix>.kmers - the k-mers in ascending order, in the final_kmers record format;\n"
           "        <prefix>.kmstat - per k-mer: 32-bit count << 1, float total_qual, the 6-bit quality sums packed into 64-bit words;\n"
           "        with --cluster <prefix>.hamming and <prefix>.hamming.idx as spades-hamcluster writes them;\n"
           "        with --subcluster the good bit in <prefix>.kmstat, the new k-mers' records after the others, and\n"
           "        <prefix>.subclusters, <prefix>.subclusters.idx, <prefix>.newkmers;\n"
           "        with --expand the good bits in <prefix>.kmstat are those after the expansion;\n"
           "        with --correct <prefix>.<i>.cor.fastq and <prefix>.<i>.bad.fastq: the corrected reads of input file i.\n",
           argv0);
}

// One block of records of one input file, as parsed, and its prepared batch on the device (bbk_hreads: the trims, the
// stretches and the candidates of every record).  A resident block keeps the batch, the names, the qualities and the
// offsets for the later passes -- what Read::print needs besides the corrected bases -- and lets the bases go.
struct Block {
    size_t file = 0;
    std::string bases, quals;  // quals: the offset subtracted
    std::vector<uint64_t> offsets{0};
    std::vector<std::string> names;
    bbk_hreads *hr = nullptr;
    bool resident = false;
    uint64_t size() const { return offsets.size() - 1; }
    uint64_t total() const { return offsets.back(); }
    ~Block() { bbk_hreads_free(hr); }
};

// The records of all files as prepared blocks, in file order, once per pass.  A block holds the records of one file up to
// -b bases, so every pass and every --resident-bytes sees the same blocks.  The blocks of the first pass stay on the
// device while their bases and qualities fit --resident-bytes; the later passes take those as they are and parse the
// files again only for the blocks behind them.
class ReadSource {
public:
    ReadSource(bbk_ctx *ctx, const std::vector<std::string> &files, unsigned k, int qvoffset, int trim_quality, size_t block_bytes,
               uint64_t resident_bytes)
        : ctx_(ctx), files_(files), k_(k), qvoffset_(qvoffset), trim_quality_(trim_quality), block_bytes_(block_bytes),
          budget_(resident_bytes), keeping_(resident_bytes != 0), kept_in_file_(files.size(), 0), whole_file_(files.size(), false) {}

    // fn(block) for every block; returns the number of records
    template <class F>
    uint64_t each(bool announce, F fn) {
        uint64_t records = 0;
        for (const auto &b : resident_) {
            fn(*b);
            records += b->size();
        }
        for (size_t f = 0; f < files_.size(); ++f) {
            if (whole_file_[f]) continue;
            if (announce) info("Processing %s", files_[f].c_str());
            records += parse(f, fn);
        }
        keeping_ = false;
        return records;
    }

    void clear() { resident_.clear(); }  // the resident blocks leave the device

private:
    template <class F>
    uint64_t parse(size_t f, F &fn) {
        FastxReader rd(files_[f]);
        if (!rd.is_open()) fatal("cannot open %s", files_[f].c_str());
        std::unique_ptr<Block> b(new Block);
        std::string name, seq, qual;
        uint64_t records = 0, block_no = 0;
        auto flush = [&] {
            if (block_no++ >= kept_in_file_[f]) {  // the blocks before are resident and have been handed out
                b->file = f;
                check(bbk_hreads_from_host(ctx_, b->bases.data(), reinterpret_cast<const uint8_t *>(b->quals.data()), b->offsets.data(),
                                           b->size(), k_, trim_quality_, &b->hr),
                      "bbk_hreads_from_host");
                fn(*b);
                records += b->size();
                if (keeping_ && held_ + 2 * b->total() <= budget_) {
                    held_ += 2 * b->total();
                    b->resident = true;
                    std::string().swap(b->bases);
                    ++kept_in_file_[f];
                    resident_.push_back(std::move(b));
                } else {
                    keeping_ = false;  // the resident blocks are a prefix of all blocks
                }
            }
            b.reset(new Block);
        };
        while (rd.next_record(name, seq, qual)) {
            if (qual.size() != seq.size())
                fatal("%s: record %llu (%s) has no quality string: the statistics need FASTQ input", files_[f].c_str(),
                      (unsigned long long)records, name.c_str());
            for (char &c : qual) {
                const int q = (unsigned char)c - qvoffset_;
                if (q < 0 || q > 93)
                    fatal("%s: record %llu (%s): quality character '%c' is outside [0, 93] at offset %d", files_[f].c_str(),
                          (unsigned long long)records, name.c_str(), c, qvoffset_);
                c = (char)q;
            }
            b->bases += seq;
            b->quals += qual;
            b->offsets.push_back(b->bases.size());
            b->names.push_back(name);
            if (b->bases.size() >= block_bytes_) flush();
        }
        if (b->size()) flush();
        if (keeping_) whole_file_[f] = true;
        return records;
    }

    bbk_ctx *ctx_;
    const std::vector<std::string> &files_;
    unsigned k_;
    int qvoffset_, trim_quality_;
    size_t block_bytes_;
    uint64_t budget_, held_ = 0;
    bool keeping_;
    std::vector<std::unique_ptr<Block>> resident_;
    std::vector<uint64_t> kept_in_file_;  // resident blocks of every file: its first ones
    std::vector<bool> whole_file_;        // every block of the file is resident
};

// CorrectReadFile (hammer_tools.cpp:107-142) over the blocks of all files: the trimmed reads of a block through the
// corrector, printed as Read::print does (read.hpp:221-236) into the pair of files of the block's input file
struct CorrectedWriter {
    const std::vector<std::string> &files;
    const std::string &prefix;
    bbk_ctx *ctx;
    bbk_corrector *cor;
    int qvoffset;
    size_t open_file = 0;
    bool is_open = false;
    FILE *good = nullptr, *bad = nullptr;
    unsigned buffer_no = 0;
    std::string out, line;
    std::vector<uint64_t> offs;
    std::vector<uint8_t> res;
    std::vector<uint32_t> trims;

    void close() {
        if (is_open && (fclose(good) != 0 || fclose(bad) != 0)) fatal("writing the corrected reads failed");
        is_open = false;
    }
    // the files of input file i, and of every file before it that had no block
    void open_until(size_t i) {
        while (!is_open || open_file < i) {
            if (is_open) {
                close();
                ++open_file;
            }
            if (open_file >= files.size()) return;
            info("Correcting single reads: %s", files[open_file].c_str());
            const std::string base = prefix + "." + std::to_string(open_file);
            const std::string cor_path = base + ".cor.fastq", bad_path = base + ".bad.fastq";
            good = fopen(cor_path.c_str(), "wb");
            bad = fopen(bad_path.c_str(), "wb");
            if (!good || !bad) fatal("cannot open %s for writing", (good ? bad_path : cor_path).c_str());
            is_open = true;
            buffer_no = 0;
        }
    }
    void finish() {
        open_until(files.empty() ? 0 : files.size() - 1);
        close();
    }
    void operator()(const Block &b) {
        open_until(b.file);
        info("Prepared batch %u of %llu reads.", buffer_no, (unsigned long long)b.size());
        out.resize(b.total());
        offs.resize(b.size() + 1);
        res.resize(b.size());
        trims.resize(2 * b.size());
        check(bbk_corrector_correct_prepared(cor, b.hr, &out[0], offs.data(), res.data(), nullptr), "bbk_corrector_correct_prepared");
        check(bbk_hreads_export(ctx, b.hr, trims.data(), nullptr, nullptr, nullptr, nullptr, nullptr), "bbk_hreads_export");
        info("Processed batch %u", buffer_no);
        for (uint64_t i = 0; i < b.size(); ++i) {
            // Read::trimLeftRight's bookkeeping (read.hpp:99-122): ltrim_ / rtrim_ are the ends of what is left, or 0 and
            // the size when nothing is
            const size_t initial = b.offsets[i + 1] - b.offsets[i], start = trims[2 * i], len = trims[2 * i + 1];
            const size_t ltrim = len ? start : 0, rtrim = len ? start + len : initial, tail = initial - rtrim;
            const size_t o = offs[i], q0 = b.offsets[i] + start;
            line.assign("@").append(b.names[i]).append("\n").append(ltrim, 'N').append(out, o, len).append(tail, 'N');
            line.append("\n+").append(b.names[i]);
            if (ltrim > 0) line.append(" ltrim=").append(std::to_string(ltrim));
            if (rtrim < initial) line.append(" rtrim=").append(std::to_string(tail));
            line.append("\n").append(ltrim, (char)(qvoffset + 2));
            for (size_t j = 0; j < len; ++j) line.push_back((char)(b.quals[q0 + j] + qvoffset));
            line.append(tail, (char)(qvoffset + 2)).append("\n");
            if (fwrite(line.data(), 1, line.size(), res[i] ? good : bad) != line.size()) fatal("writing the corrected reads failed");
        }
        info("Written batch %u", buffer_no);
        ++buffer_no;
    }
};

int main(int argc, char **argv) {
    unsigned K = 21, device = 0;
    unsigned long long threads = 0, bufsize = 536870912ull, qvoffset = 33, trim_quality = 4, resident_bytes = 0;
    std::string prefix, dataset;
    std::vector<std::string> input;
    unsigned expand_max_iterations = 25;  // configs/hammer/config.info
    unsigned long long expand_min_changed = 10;  // main.cpp:219
    bool help = false, cluster = false, subcluster = false, expand = false, correct = false;
    bbk_subcluster_params sp = {0.995, 0.9, 0.98, 1};  // configs/hammer/config.info
    Options opt;
    opt.num("-k", "--kmer", &K).num("-t", "--threads", &threads).num("-b", "--bufsize", &bufsize).num("", "--device", &device)
        .num("", "--resident-bytes", &resident_bytes).num("", "--qvoffset", &qvoffset).num("", "--trim-quality", &trim_quality).flag("", "--cluster", &cluster)
        .flag("", "--subcluster", [&] { cluster = subcluster = true; })
        .flag("", "--expand", [&] { cluster = subcluster = expand = true; })
        .flag("", "--correct", [&] { cluster = subcluster = expand = correct = true; })
        .num("", "--expand-max-iterations", &expand_max_iterations, 1u).num("", "--expand-min-changed", &expand_min_changed)
        .flag("", "--no-correct-threshold", [&] { sp.correct_use_threshold = 0; })
        .real("", "--singleton-threshold", &sp.singleton_threshold)
        .real("", "--nonsingleton-threshold", &sp.nonsingleton_threshold).real("", "--correct-threshold", &sp.correct_threshold)
        .str("-d", "--dataset", &dataset).str("-o", "--output", &prefix).flag("-h", "--help", &help).positional(&input);
    if (!opt.parse(argc, argv) || help || (prefix.empty() && !(input.empty() && dataset.empty()))) {
        usage(argv[0]);
        return help ? 0 : 1;
    }
    require_input(input, dataset, usage, argv[0]);
    if (K < 1 || K > 32) fatal("k-mer size %u is out of range [1, 32]", K);
    if (qvoffset > 255 || trim_quality > 93) fatal("--qvoffset / --trim-quality out of range");

    info("Starting k-mer statistics (MI355X, %s)", bbk_version());
    info("K-mer length set to %u", K);
    const std::vector<std::string> files = input_files(input, dataset);
    Run run;
    Phases &ph = run.ph;
    run.create_ctx(device);
    bbk_ctx *ctx = run.ctx;

    // pass 1: the set
    bbk_counter *counter = nullptr;
    check(bbk_count_begin(ctx, K, BBK_BOTH_STRANDS, &counter), "bbk_count_begin");
    uint64_t stretches = 0;
    double t0 = now_s();
    ReadSource src(ctx, files, K, (int)qvoffset, (int)trim_quality, (size_t)bufsize, resident_bytes);
    const uint64_t records = src.each(true, [&](const Block &b) {
        const bbk_reads *r = nullptr;
        check(bbk_hreads_stretch_view(b.hr, &r, nullptr), "bbk_hreads_stretch_view");
        check(bbk_count_push_reads(counter, r), "bbk_count_push_reads");
        stretches += bbk_hreads_kmer_stretches(b.hr);
        ++ph.blocks;
    });
    info("Total %llu reads processed, %llu stretches of valid k-mers", (unsigned long long)records,
         (unsigned long long)stretches);
    bbk_kmerset *set = nullptr;
    check(bbk_count_finish(counter, &set), "bbk_count_finish");
    const uint64_t n = bbk_kmerset_size(set);
    info("K-mer counting done. There are %llu kmers in total.", (unsigned long long)n);

    bbk_hamclusters *hc = nullptr;
    if (cluster) check(bbk_kmerset_hamming_clusters(ctx, set, 1, 0, 0, &hc), "bbk_kmerset_hamming_clusters");

    // pass 2: the statistics
    info("Collecting K-mer information");
    bbk_kmerstats *ks = nullptr;
    check(bbk_kmerstats_begin(ctx, set, &ks), "bbk_kmerstats_begin");
    src.each(false, [&](const Block &b) {
        const bbk_reads *r = nullptr;
        const bbk_quals *q = nullptr;
        check(bbk_hreads_stretch_view(b.hr, &r, &q), "bbk_hreads_stretch_view");
        check(bbk_kmerstats_push(ks, r, q), "bbk_kmerstats_push");
    });
    check(bbk_kmerstats_finish(ks), "bbk_kmerstats_finish");
    ph.device = now_s() - t0;

    t0 = now_s();
    {
        std::vector<uint64_t> buf((size_t)n);  // one word per k-mer (k <= 32)
        check(bbk_kmerset_export(ctx, set, BBK_ORDER_SORTED, buf.data(), nullptr), "bbk_kmerset_export");
        write_u64(prefix + ".kmers", buf.data(), buf.size());
    }
    if (!subcluster) check(bbk_kmerstats_write(ctx, ks, (prefix + ".kmstat").c_str()), "bbk_kmerstats_write");
    if (hc) {
        check(bbk_hamclusters_write(ctx, hc, (prefix + ".hamming").c_str()), "bbk_hamclusters_write");
        info("Clustering done. Total clusters: %llu", (unsigned long long)bbk_hamclusters_count(hc));
    }
    if (subcluster) {
        bbk_subclusters *sc = nullptr;
        check(bbk_hamclusters_subcluster(ctx, set, hc, ks, &sp, &sc), "bbk_hamclusters_subcluster");
        if (expand) {  // main.cpp:194-222
            bbk_expander *ex = nullptr;
            check(bbk_expander_from_subclusters(ctx, set, sc, &ex), "bbk_expander_from_subclusters");
            info("Starting solid k-mers expansion in snapshot rounds.");
            for (unsigned iter = 0; iter < expand_max_iterations; ++iter) {
                check(bbk_expander_round_begin(ex), "bbk_expander_round_begin");
                src.each(false, [&](const Block &b) {
                    const bbk_reads *r = nullptr;
                    check(bbk_hreads_candidate_view(b.hr, &r), "bbk_hreads_candidate_view");
                    check(bbk_expander_push(ex, r, nullptr), "bbk_expander_push");
                    // push does not wait, and a block that is not resident goes now
                    if (!b.resident) check(bbk_ctx_synchronize(ctx), "bbk_ctx_synchronize");
                });
                uint64_t changed = 0;
                check(bbk_expander_round_end(ex, &changed), "bbk_expander_round_end");
                info("Solid k-mers iteration %u produced %llu new k-mers.", iter, (unsigned long long)changed);
                if (changed < expand_min_changed) break;
            }
            info("Solid k-mers finalized");
            check(bbk_expander_store(ex, sc), "bbk_expander_store");
            if (correct) {  // hammer_tools.cpp:218-277, every file as a single-read file
                bbk_corrector *cor = nullptr;
                check(bbk_corrector_from_expander(ctx, set, ex, &cor), "bbk_corrector_from_expander");
                info("Starting read correction.");
                CorrectedWriter w{files, prefix, ctx, cor, (int)qvoffset};
                src.each(false, std::ref(w));
                w.finish();
                uint64_t cs[5];
                check(bbk_corrector_stats(cor, cs), "bbk_corrector_stats");
                info("Correction done. Changed %llu bases in %llu reads.", (unsigned long long)cs[1], (unsigned long long)cs[0]);
                info("Failed to correct %llu bases out of %llu.", (unsigned long long)cs[2], (unsigned long long)cs[3]);
                info("  Searches corrected on the host: %llu", (unsigned long long)cs[4]);
                bbk_corrector_free(cor);
            }
            bbk_expander_free(ex);
        }
        check(bbk_subclusters_write(ctx, sc, ks, prefix.c_str()), "bbk_subclusters_write");
        uint64_t st[9], errs[16];
        check(bbk_subclusters_export(ctx, sc, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, errs, st),
              "bbk_subclusters_export");
        const uint64_t gsingl = st[0], tsingl = st[1], tcsingl = st[2], gcsingl = st[3], tcls = st[4], gcls = st[5],
                       tkmers = st[6], tncls = st[7], newkmers = st[8];
        // kmer_cluster.cpp:650-658
        info("Subclustering done. Total %llu non-read kmers were generated.", (unsigned long long)newkmers);
        info("Subclustering statistics:");
        info("  Total singleton hamming clusters: %llu. Among them %llu (%g%%) are good", (unsigned long long)tsingl,
             (unsigned long long)gsingl, 100.0 * (double)gsingl / (double)tsingl);
        info("  Total singleton subclusters: %llu. Among them %llu (%g%%) are good", (unsigned long long)tcsingl,
             (unsigned long long)gcsingl, 100.0 * (double)gcsingl / (double)tcsingl);
        info("  Total non-singleton subcluster centers: %llu. Among them %llu (%g%%) are good", (unsigned long long)tcls,
             (unsigned long long)gcls, 100.0 * (double)gcls / (double)tcls);
        info("  Average size of non-trivial subcluster: %g kmers", 1.0 * (double)tkmers / (double)tcls);
        info("  Average number of sub-clusters per non-singleton cluster: %g", 1.0 * (double)(tcsingl + tcls) / (double)tncls);
        info("  Total solid k-mers: %llu", (unsigned long long)(gsingl + gcsingl + gcls));
        std::string m;
        for (int r = 0; r < 4; ++r) {
            uint64_t row = 0;
            for (int c = 0; c < 4; ++c) row += errs[4 * r + c];
            for (int c = 0; c < 4; ++c) {
                char b[64];
                snprintf(b, sizeof(b), "%s%g", c ? "," : "", (double)errs[4 * r + c] / (double)row);
                m += b;
            }
            m += r < 3 ? ")," : ")";
            if (r < 3) m += "(";
        }
        info("  Substitution probabilities: [4,4]((%s)", m.c_str());
        info("  K-mers subclustered on the host: %llu", (unsigned long long)bbk_subclusters_host_kmers(sc));
        bbk_subclusters_free(sc);
    }
    if (hc) bbk_hamclusters_free(hc);
    {
        std::vector<uint32_t> cnt((size_t)n);
        check(bbk_kmerstats_export(ctx, ks, cnt.data(), nullptr, nullptr), "bbk_kmerstats_export");
        uint64_t singletons = 0;
        for (uint32_t c : cnt) singletons += c == 1;
        info("There are %llu kmers in total. Among them %llu (%g%%) are singletons.", (unsigned long long)n,
             (unsigned long long)singletons, n ? 100.0 * (double)singletons / (double)n : 0.0);
    }
    src.clear();
    bbk_kmerstats_free(ks);
    bbk_kmerset_free(set);
    ph.write = now_s() - t0;
    run.done("spades-kmerdata");
}
