// spades-kmer-estimating drop-in: same argv contract and the same result line as the reference tool
// (projects/kmercount/kmer_estimating.cpp:39-58 for the flags, :60-104 for the flow).  The reference feeds a
// symmetric (strand-independent) rolling hash of every k-mer of the reads into a HyperLogLog
// (common/utils/kmer_counting.hpp:18-43,182-263) and prints the ESTIMATE of the number of distinct k-mers, reverse
// complements identified.  The engine counts them exactly (bbk_count, canonical set, dedup only), so the number
// printed here is the exact cardinality the estimate approximates (HLL error is ~1 %).
//   -k/--kmer <int=21>  -d/--dataset <yaml> (required)  -t/--threads <int>  -h/--help     (+ --device <int>, ours)
#include <string>
#include <vector>

#include "common.hpp"

using namespace bbkhost;

static void usage(const char *argv0) {
    printf("SYNOPSIS\n        %s [-k <value>] -d <dir> [-t <value>] [-h]\n\n"
           "OPTIONS\n"
           "        -k, --kmer <value>      K-mer length\n"
           "        -d, --dataset <dir>     Dataset description (in YAML)\n"
           "        -t, --threads <value>   # of threads to use\n"
           "        -h, --help              Show help\n"
           "        --device <value>        GPU to use (default 0)\n\n"
           "DESCRIPTION\n         Kmer number estimating.  Kmers from reverse-complementary reads aren't taken into account.\n",
           argv0);
}

int main(int argc, char **argv) {
    unsigned K = 21, device = 0;
    unsigned long long threads = 0;  // accepted; the parser takes its default
    std::string dataset;
    bool help = false;
    Options opt;
    opt.num("-k", "--kmer", &K).num("-t", "--threads", &threads).num("", "--device", &device).str("-d", "--dataset", &dataset)
        .flag("-h", "--help", &help);
    if (!opt.parse(argc, argv) || help || dataset.empty()) {  // kmer_estimating.cpp:50-57: -d is required
        usage(argv[0]);
        return help ? 0 : 1;
    }
    if (K < 1 || K >= BBK_MAX_K) fatal("k-mer size %u is out of range [1, %d)", K, BBK_MAX_K);

    info("Starting kmer spectra cardinality (MI355X, %s)", bbk_version());
    info("K-mer length set to %u", K);
    const std::vector<std::string> files = input_files({}, dataset);
    Run run;
    run.create_ctx(device);
    info("Estimating kmer cardinality");
    // strand-independent distinct k-mers: the canonical set; hash-bucket order is enough (no sort); streamed block by block
    bbk_kmerset *set = count_files(run.ctx, run.ph, files, K, BBK_CANONICAL | BBK_UNSORTED, 512u << 20, default_threads());
    info("Kmer number estimation: %llu", (unsigned long long)bbk_kmerset_size(set));  // :99, exact here
    bbk_kmerset_free(set);
    run.leave();
}
