// spades-kmerdata: BayesHammer's counting phase -- the k-mer set and one KMerStat per k-mer -- on the MI355X engine behind
// the C ABI (include/bbk.h).  Not a drop-in: the reference has this only inside spades-hammer
// (projects/hammer/main.cpp:122-171: KMerDataCounter::BuildKMerIndex, the Hamming clustering, then
// KMerDataCounter::FillKMerData, "Collecting K-mer information, this takes a while"); this tool is that sequence alone.
// The sequence itself -- the blocks, the passes, the writers -- is host/hammer_run.hpp, which spades-hammer (hammer_main.cpp,
// the drop-in) runs once per iteration; here it runs once, as iteration 0, with every step behind its own option.
//   -k/--kmer <int=21>  -t/--threads <int>  -b/--bufsize <bytes>  -o/--output <prefix>  -d/--dataset <yaml>  [input files...]
//   (+ --device <int>, --qvoffset <int=33>, --trim-quality <int=4>, --cluster, --subcluster with --singleton-threshold,
//      --nonsingleton-threshold, --correct-threshold, --no-correct-threshold, --expand with --expand-max-iterations <int=25>,
//      --expand-min-changed <int=10>, --correct with --correct-stats, --paired and --output-dir <dir>,
//      --resident-bytes <bytes=0>, --device-parse with --parse-chunk <bytes=67108864>, --filter-singletons)
// The records of every file go to the device as parsed, in blocks of -b bases, and are prepared there (bbk_hreads: the trim
// of input_trim_quality 4 of configs/hammer/config.info, then ValidKMerGenerator's valid starts as stretches); a stretch is
// one read of the engine.  Every pass takes a view of the prepared blocks:
//   pass 1  the stretches through bbk_count_begin / push / finish(BBK_BOTH_STRANDS); with --filter-singletons
//           (count_filter_singletons 1, KMerDataCounter::BuildKMerIndex, kmer_data.cpp:280-335) with BBK_WITH_COUNTS and
//           bbk_count_finish_min_count(2): every later step works on the k-mers that occur more than once
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
//   with --correct (CorrectAllReads, projects/hammer/hammer_tools.cpp:79-277, and read_corrector.cpp; implies --expand):
//   after the expansion every block is taken once more: its records are trimmed (Read::trimNsAndBadQuality(--trim-quality)),
//   corrected (bbk_corrector_correct_resident), printed in the format of Read::print on the device (bbk_corrected_print)
//   and every stream of the text goes behind its file (bbk_fastq_text_write).  Input file i is a single-read file
//   (CorrectReadFile): <prefix>.<i>.cor.fastq (result true) and <prefix>.<i>.bad.fastq.
//   --correct-stats: correct_stats 1 of configs/hammer/config.info: the name of a read carries BH:ok, BH:failed or
//   BH:changed:<n> (read_corrector.cpp:214-242).
//   --paired: the positional files two at a time, or with -d every library's left reads[i] and right reads[i], are a
//   pair (CorrectPairedReadFiles, hammer_tools.cpp:144-193): both mates good -> the two .cor.fastq, otherwise a good mate ->
//   <prefix>.<i_left>.unpaired.fastq and a bad one -> its own .bad.fastq.  Both files of a pair are cut into blocks at the
//   same record indices, in every pass; a block ends when either side reaches -b.
//   --output-dir <dir>: the corrected reads under the reference's names instead (hammer_tools.cpp:53-59,206-258:
//   <dir>/<basename>.00.<ilib>_<iread>.cor.fastq, <dir>/<basename>.00.bad.fastq, the unpaired reads under the basename of
//   <largest common prefix>_unpaired.fastq), and <dir>/corrected.yaml, the corrected libraries (main.cpp:254-256).
// The records are parsed by one thread (fastx.hpp's next_record, which keeps the quality line); -t is accepted for the
// common interface.
//   --device-parse: the text of every file (gzread: plain files pass through, decompression stays on the host) goes to the
//   device in chunks of --parse-chunk bytes and is parsed there (bbk_fastq_input_*): the blocks hold the
//   same records (bbk_fastq_input_records_within is the rule above; of a pair, the side that closes its block first), the
//   text behind the last block of a chunk is carried into the next one, and a block keeps nothing on the host -- the
//   corrected reads are printed with the names the batch holds (bbk_corrected_print_resident).  Where the index has a
//   verdict -- a record that is not four lines, or a quality character outside the offset's range -- the group goes on
//   with fastx.hpp's reader from the first record of the block that did not get complete (of a pair: both files), so
//   multi-line records, blank lines, FASTA records, truncated files and every refusal are exactly those of the serial
//   reader; the place is remembered, and the later passes go there without indexing that text again.  Every output file
//   is the same bytes with and without the option.
#include "hammer_run.hpp"

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
           "        --correct-stats         Tag the names of the corrected reads: BH:ok, BH:failed, BH:changed:<n>\n"
           "        --paired                Input files two at a time (with -d: left reads[i] and right reads[i]) are pairs:\n"
           "                                a pair is kept only when both mates are good, a single good mate is unpaired\n"
           "        --output-dir <value>    Write the corrected reads under the names BayesHammer gives them in this\n"
           "                                directory, and corrected.yaml, the dataset description of the corrected reads\n"
           "        --resident-bytes <value>  Keep the first blocks on the GPU for the later passes while their bases and\n"
           "                                qualities total at most this many bytes (default 0: every pass parses the input)\n"
           "        --device-parse          Parse the FASTQ text on the GPU; input that is not in the four-line form goes\n"
           "                                through the serial reader from the first such record on (same output files)\n"
           "        --parse-chunk <value>   Bytes of text per chunk of --device-parse (default 67108864)\n"
           "        --filter-singletons     Keep only the k-mers that occur more than once (count_filter_singletons 1)\n\n"
           "DESCRIPTION\n        K-mers of FASTQ reads and their reverse complements with BayesHammer's per-k-mer statistics (MI355X)\n\n"
           "        Output: <prefix>.kmers - the k-mers in ascending order, in the final_kmers record format;\n"
           "        <prefix>.kmstat - per k-mer: 32-bit count << 1, float total_qual, the 6-bit quality sums packed into 64-bit words;\n"
           "        with --cluster <prefix>.hamming and <prefix>.hamming.idx as spades-hamcluster writes them;\n"
           "        with --subcluster the good bit in <prefix>.kmstat, the new k-mers' records after the others, and\n"
           "        <prefix>.subclusters, <prefix>.subclusters.idx, <prefix>.newkmers;\n"
           "        with --expand the good bits in <prefix>.kmstat are those after the expansion;\n"
           "        with --correct <prefix>.<i>.cor.fastq and <prefix>.<i>.bad.fastq: the corrected reads of input file i;\n"
           "        with --paired also <prefix>.<i>.unpaired.fastq for the left file i of every pair.\n",
           argv0);
}

int main(int argc, char **argv) {
    unsigned device = 0;
    unsigned long long threads = 0, bufsize = 536870912ull, qvoffset = 33, trim_quality = 4, resident_bytes = 0, parse_chunk = 67108864ull;
    std::string dataset;
    std::vector<std::string> input;
    bool help = false, paired = false;
    HammerParams p;  // the thresholds and the iteration limits of configs/hammer/config.info; iteration 0
    Options opt;
    opt.num("-k", "--kmer", &p.K).num("-t", "--threads", &threads).num("-b", "--bufsize", &bufsize).num("", "--device", &device)
        .num("", "--resident-bytes", &resident_bytes).num("", "--qvoffset", &qvoffset).num("", "--trim-quality", &trim_quality).flag("", "--cluster", &p.cluster)
        .flag("", "--subcluster", [&] { p.cluster = p.subcluster = true; })
        .flag("", "--expand", [&] { p.cluster = p.subcluster = p.expand = true; })
        .flag("", "--correct", [&] { p.cluster = p.subcluster = p.expand = p.correct = true; })
        .flag("", "--correct-stats", &p.correct_stats).flag("", "--paired", &paired).flag("", "--device-parse", &p.device_parse)
        .flag("", "--filter-singletons", &p.filter_singletons)
        .num("", "--parse-chunk", &parse_chunk, 1ull).str("", "--output-dir", &p.out_dir)
        .num("", "--expand-max-iterations", &p.expand_max_iterations, 1u).num("", "--expand-min-changed", &p.expand_min_changed)
        .flag("", "--no-correct-threshold", [&] { p.sp.correct_use_threshold = 0; })
        .real("", "--singleton-threshold", &p.sp.singleton_threshold)
        .real("", "--nonsingleton-threshold", &p.sp.nonsingleton_threshold).real("", "--correct-threshold", &p.sp.correct_threshold)
        .str("-d", "--dataset", &dataset).str("-o", "--output", &p.prefix).flag("-h", "--help", &help).positional(&input);
    if (!opt.parse(argc, argv) || help || (p.prefix.empty() && !(input.empty() && dataset.empty()))) {
        usage(argv[0]);
        return help ? 0 : 1;
    }
    require_input(input, dataset, usage, argv[0]);
    if (p.K < 1 || p.K > 32) fatal("k-mer size %u is out of range [1, 32]", p.K);
    if (qvoffset > 255 || trim_quality > 93) fatal("--qvoffset / --trim-quality out of range");
    p.qvoffset = (int)qvoffset;
    p.trim_quality = (int)trim_quality;
    p.block_bytes = (size_t)bufsize;
    p.parse_chunk = (size_t)parse_chunk;
    p.resident_bytes = resident_bytes;

    info("Starting k-mer statistics (MI355X, %s)", bbk_version());
    info("K-mer length set to %u", p.K);
    std::vector<InFile> files;
    std::vector<Group> groups;
    std::vector<DatasetLib> outlibs;
    plan_input(input_libs(input, dataset, paired), paired, files, groups, outlibs);
    if (p.correct && !p.out_dir.empty()) p.out_dir = make_dir_absolute(p.out_dir);
    Run run;
    run.create_ctx(device);
    run_hammer_iteration(run.ctx, run.ph, p, files, groups, outlibs);
    run.done("spades-kmerdata");
}
