// spades-kmerdata: BayesHammer's counting phase -- the k-mer set and one KMerStat per k-mer -- on the MI355X engine behind
// the C ABI (include/bbk.h).  Not a drop-in: the reference has this only inside spades-hammer
// (projects/hammer/main.cpp:122-171: KMerDataCounter::BuildKMerIndex, the Hamming clustering, then
// KMerDataCounter::FillKMerData, "Collecting K-mer information, this takes a while"); this tool is that sequence alone.
//   -k/--kmer <int=21>  -t/--threads <int>  -b/--bufsize <bytes>  -o/--output <prefix>  -d/--dataset <yaml>  [input files...]
//   (+ --device <int>, --qvoffset <int=33>, --trim-quality <int=4>, --cluster, --subcluster with --singleton-threshold,
//      --nonsingleton-threshold, --correct-threshold, --no-correct-threshold, --expand with --expand-max-iterations <int=25>,
//      --expand-min-changed <int=10>, --correct)
// Every FASTQ record is cut into the stretches of its valid k-mer starts (hammer_reads.hpp: input_trim_quality 4 of
// configs/hammer/config.info, then ValidKMerGenerator); a stretch is one read of the engine.
//   pass 1  the stretches, in blocks of -b bytes, through bbk_count_begin / push / finish(BBK_BOTH_STRANDS)
//   pass 2  the same files again: the same stretches with their qualities through bbk_kmerstats_push
// Output:
//   <prefix>.kmers        the ascending both-strand k-mers (final_kmers records), as spades-hamcluster writes them: index
//                         i of the other files is record i
//   <prefix>.kmstat       one binary_write(KMerStat) record per k-mer (projects/hammer/kmer_stat.hpp:170-175)
//   <prefix>.hamming, <prefix>.hamming.idx   with --cluster: the Hamming clusters of that set, as spades-hamcluster
//   with --subcluster (KMerClustering::process, projects/hammer/kmer_cluster.cpp:590-659; implies --cluster):
//   <prefix>.kmstat then carries the good bit and the records of the new k-mers, and <prefix>.subclusters,
//   <prefix>.subclusters.idx and <prefix>.newkmers are written (bbk_subclusters_write)
//   with --expand (the solid k-mer expansion, projects/hammer/main.cpp:194-222 and expander.cpp:20-70; implies
//   --subcluster): after the subclustering every round reads the files again and pushes the records the Expander can ever
//   find solid (hammer_reads.hpp: expander_candidate), trimmed, in blocks of -b bytes through bbk_expander_push, until a
//   round adds fewer than --expand-min-changed k-mers or --expand-max-iterations rounds have run; <prefix>.kmstat then
//   carries the expanded good bits (bbk_expander_store) and every other file is as without --expand
//   with --correct (ReadCorrector, projects/hammer/read_corrector.cpp and hammer_tools.cpp:79-142 CorrectReadFile; implies
//   --expand): after the expansion every input file i is read once more as a single-read file: every record is trimmed
//   (Read::trimNsAndBadQuality(--trim-quality)), corrected in blocks of -b bytes (bbk_corrector_correct) and printed in
//   the format of Read::print to <prefix>.<i>.cor.fastq (result true) or <prefix>.<i>.bad.fastq
// The records are parsed by one thread (fastx.hpp's next_record, which keeps the quality line); -t is accepted for the
// common interface.
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include "hammer_reads.hpp"

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
           "        --correct               Also correct the reads with the expanded solid k-mers (implies --expand)\n\n"
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

// one block of stretches: bases and qualities (offset subtracted) back to back, offsets for both
struct Block {
    std::string bases, quals;
    std::vector<uint64_t> offsets{0};
    void clear() {
        bases.clear();
        quals.clear();
        offsets.assign(1, 0);
    }
    uint64_t size() const { return offsets.size() - 1; }
};

// Calls push(block) for every block of at most block_bytes bases of the stretches of all records, in file order; returns
// the number of records.  Both passes go through here, so they see the same stretches in the same blocks.  candidates:
// the rounds of the expansion, which take the trimmed read of every record the Expander can ever find solid instead.
template <class Push>
static uint64_t for_each_block(const std::vector<std::string> &files, unsigned k, int qvoffset, int trim_quality,
                               size_t block_bytes, bool announce, bool candidates, Push push) {
    Block b;
    std::string name, seq, qual;
    std::vector<hammer::Stretch> st;
    uint64_t records = 0;
    for (const std::string &f : files) {
        if (announce) info("Processing %s", f.c_str());
        FastxReader rd(f);
        if (!rd.is_open()) fatal("cannot open %s", f.c_str());
        while (rd.next_record(name, seq, qual)) {
            if (qual.size() != seq.size())
                fatal("%s: record %llu (%s) has no quality string: the statistics need FASTQ input", f.c_str(),
                      (unsigned long long)records, name.c_str());
            for (char &c : qual) {
                const int q = (unsigned char)c - qvoffset;
                if (q < 0 || q > 93)
                    fatal("%s: record %llu (%s): quality character '%c' is outside [0, 93] at offset %d", f.c_str(),
                          (unsigned long long)records, name.c_str(), c, qvoffset);
                c = (char)q;
            }
            ++records;
            st.clear();
            hammer::Stretch whole;
            if (!candidates) hammer::valid_stretches(seq, qual, k, trim_quality, st);
            else if (hammer::expander_candidate(seq, qual, k, trim_quality, &whole)) st.push_back(whole);
            for (const hammer::Stretch &s : st) {
                b.bases.append(seq, s.start, s.length);
                b.quals.append(qual, s.start, s.length);
                b.offsets.push_back(b.bases.size());
            }
            if (b.bases.size() >= block_bytes) {
                push(b);
                b.clear();
            }
        }
    }
    if (b.size()) push(b);
    return records;
}

// CorrectReadFile (hammer_tools.cpp:107-142) over one input file: trimmed records in blocks of block_bytes bases through the
// corrector, printed as Read::print does (read.hpp:221-236)
static void correct_read_file(bbk_corrector *cor, const std::string &file, int qvoffset, int trim_quality, size_t block_bytes,
                              const std::string &cor_path, const std::string &bad_path) {
    FastxReader rd(file);
    if (!rd.is_open()) fatal("cannot open %s", file.c_str());
    FILE *good = fopen(cor_path.c_str(), "wb"), *bad = fopen(bad_path.c_str(), "wb");
    if (!good || !bad) fatal("cannot open %s for writing", (good ? bad_path : cor_path).c_str());
    Block b;
    std::vector<std::string> names;
    std::vector<hammer::Trim> trims;
    std::string out;
    std::vector<uint8_t> res;
    unsigned buffer_no = 0;
    auto flush = [&] {
        info("Prepared batch %u of %llu reads.", buffer_no, (unsigned long long)b.size());
        out.resize(b.bases.size());
        res.resize(b.size());
        check(bbk_corrector_correct(cor, b.bases.data(), reinterpret_cast<const uint8_t *>(b.quals.data()), b.offsets.data(),
                                    b.size(), &out[0], res.data(), nullptr),
              "bbk_corrector_correct");
        info("Processed batch %u", buffer_no);
        std::string line;
        for (uint64_t i = 0; i < b.size(); ++i) {
            const hammer::Trim &t = trims[i];
            const size_t o = b.offsets[i], len = b.offsets[i + 1] - o;
            const int tail = t.initial_size_ - t.rtrim_;
            line.assign("@").append(names[i]).append("\n").append((size_t)t.ltrim_, 'N').append(out, o, len).append((size_t)tail, 'N');
            line.append("\n+").append(names[i]);
            if (t.ltrim_ > 0) line.append(" ltrim=").append(std::to_string(t.ltrim_));
            if (t.rtrim_ < t.initial_size_) line.append(" rtrim=").append(std::to_string(tail));
            line.append("\n").append((size_t)t.ltrim_, (char)(qvoffset + 2));
            for (size_t j = 0; j < len; ++j) line.push_back((char)(b.quals[o + j] + qvoffset));
            line.append((size_t)tail, (char)(qvoffset + 2)).append("\n");
            if (fwrite(line.data(), 1, line.size(), res[i] ? good : bad) != line.size()) fatal("writing the corrected reads failed");
        }
        info("Written batch %u", buffer_no);
        ++buffer_no;
        b.clear();
        names.clear();
        trims.clear();
    };
    std::string name, seq, qual;
    uint64_t records = 0;
    while (rd.next_record(name, seq, qual)) {
        if (qual.size() != seq.size()) fatal("%s: record %llu (%s) has no quality string", file.c_str(), (unsigned long long)records, name.c_str());
        for (char &c : qual) c = (char)((unsigned char)c - qvoffset);  // checked in the first pass
        ++records;
        const hammer::Trim t = hammer::trim_ns_and_bad_quality(seq, qual, trim_quality);
        b.bases.append(seq, t.start, t.length);
        b.quals.append(qual, t.start, t.length);
        b.offsets.push_back(b.bases.size());
        names.push_back(name);
        trims.push_back(t);
        if (b.bases.size() >= block_bytes) flush();
    }
    if (b.size()) flush();
    if (fclose(good) != 0 || fclose(bad) != 0) fatal("writing the corrected reads failed");
}

int main(int argc, char **argv) {
    unsigned K = 21, device = 0;
    unsigned long long threads = 0, bufsize = 536870912ull, qvoffset = 33, trim_quality = 4;
    std::string prefix, dataset;
    std::vector<std::string> input;
    unsigned expand_max_iterations = 25;  // configs/hammer/config.info
    unsigned long long expand_min_changed = 10;  // main.cpp:219
    bool help = false, cluster = false, subcluster = false, expand = false, correct = false;
    bbk_subcluster_params sp = {0.995, 0.9, 0.98, 1};  // configs/hammer/config.info
    Options opt;
    opt.num("-k", "--kmer", &K).num("-t", "--threads", &threads).num("-b", "--bufsize", &bufsize).num("", "--device", &device)
        .num("", "--qvoffset", &qvoffset).num("", "--trim-quality", &trim_quality).flag("", "--cluster", &cluster)
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
    const uint64_t records = for_each_block(files, K, (int)qvoffset, (int)trim_quality, (size_t)bufsize, true, false, [&](const Block &b) {
        check(bbk_count_push_ascii(counter, b.bases.data(), b.offsets.data(), b.size()), "bbk_count_push_ascii");
        stretches += b.size();
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
    for_each_block(files, K, (int)qvoffset, (int)trim_quality, (size_t)bufsize, false, false, [&](const Block &b) {
        bbk_reads *r = nullptr;
        bbk_quals *q = nullptr;
        check(bbk_reads_from_ascii(ctx, b.bases.data(), b.offsets.data(), b.size(), &r), "bbk_reads_from_ascii");
        check(bbk_quals_from_host(ctx, r, reinterpret_cast<const uint8_t *>(b.quals.data()), b.offsets.data(), b.size(), &q),
              "bbk_quals_from_host");
        check(bbk_kmerstats_push(ks, r, q), "bbk_kmerstats_push");
        bbk_quals_free(q);
        bbk_reads_free(r);
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
                for_each_block(files, K, (int)qvoffset, (int)trim_quality, (size_t)bufsize, false, true, [&](const Block &b) {
                    bbk_reads *r = nullptr;
                    check(bbk_reads_from_ascii(ctx, b.bases.data(), b.offsets.data(), b.size(), &r), "bbk_reads_from_ascii");
                    check(bbk_expander_push(ex, r, nullptr), "bbk_expander_push");
                    check(bbk_ctx_synchronize(ctx), "bbk_ctx_synchronize");  // push does not wait, and the reads go now
                    bbk_reads_free(r);
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
                for (size_t i = 0; i < files.size(); ++i) {
                    info("Correcting single reads: %s", files[i].c_str());
                    const std::string base = prefix + "." + std::to_string(i);
                    correct_read_file(cor, files[i], (int)qvoffset, (int)trim_quality, (size_t)bufsize, base + ".cor.fastq",
                                      base + ".bad.fastq");
                }
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
    bbk_kmerstats_free(ks);
    bbk_kmerset_free(set);
    ph.write = now_s() - t0;
    run.done("spades-kmerdata");
}
