// spades-hamcluster: BayesHammer's Hamming-graph clustering (tau = 1) of the k-mers of a read set, on the MI355X engine
// behind the C ABI (include/bbk.h).  Not a drop-in: the reference has this step only inside spades-hammer
// (projects/hammer/main.cpp:143-168: KMerDataCounter, then TauOneKMerHamClusterer::cluster and
// ConcurrentDSU::extract_to_file into kmers.hamming / kmers.hamming.idx); this tool is that step alone.
//   -k/--kmer <int=21>  -t/--threads <int>  -b/--bufsize <bytes>  -o/--output <prefix>  -d/--dataset <yaml>  [input files...]
//   (+ --device <int>, --lock-size <int=2500>, --chunk <int=65536>)
// The reads are streamed through bbk_count_begin / push / finish as in spades-kmercount (same reader, -t and -b), the
// both-strand set is clustered, and three files are written:
//   <prefix>.kmers        the ascending both-strand k-mers (final_kmers records): index i of the other two files is record i
//   <prefix>.hamming      the member indices as u64, cluster by cluster
//   <prefix>.hamming.idx  one u64 size per cluster
#include <cstring>
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
           "        --lock-size <value>     Clusters of this many k-mers are locked (default 2500)\n"
           "        --chunk <value>         Indices per chunk of the locking rule (default 65536)\n\n"
           "DESCRIPTION\n        Hamming-graph clustering (tau = 1) of the k-mers of reads and their reverse complements (MI355X)\n\n"
           "        Output: <prefix>.kmers - the k-mers in ascending order, in the final_kmers record format;\n"
           "        <prefix>.hamming - k-mer indices (64-bit) cluster by cluster; <prefix>.hamming.idx - cluster sizes (64-bit).\n",
           argv0);
}

int main(int argc, char **argv) {
    unsigned K = 21, device = 0;
    unsigned long long threads = 0, bufsize = 536870912ull, lock_size = 0, chunk = 0;
    std::string prefix, dataset;
    std::vector<std::string> input;
    bool help = false;
    Options opt;
    opt.num("-k", "--kmer", &K).num("-t", "--threads", &threads).num("-b", "--bufsize", &bufsize).num("", "--device", &device)
        .num("", "--lock-size", &lock_size).num("", "--chunk", &chunk).str("-d", "--dataset", &dataset)
        .str("-o", "--output", &prefix).flag("-h", "--help", &help).positional(&input);
    if (!opt.parse(argc, argv) || help || (prefix.empty() && !(input.empty() && dataset.empty()))) {
        usage(argv[0]);
        return help ? 0 : 1;
    }
    require_input(input, dataset, usage, argv[0]);
    if (K < 1 || K > 32) fatal("k-mer size %u is out of range [1, 32]", K);

    info("Starting Hamming-graph clustering (MI355X, %s)", bbk_version());
    info("K-mer length set to %u", K);
    const std::vector<std::string> files = input_files(input, dataset);
    Run run;
    Phases &ph = run.ph;
    // the context is created while the first block is being parsed
    bbk_kmerset *set = count_files(run.ctx, ph, files, K, BBK_BOTH_STRANDS, (size_t)bufsize,
                                   threads ? (int)threads : default_threads(), [&] { run.create_ctx(device); });
    bbk_ctx *ctx = run.ctx;
    const uint64_t n = bbk_kmerset_size(set);
    info("K-mer counting done. There are %llu kmers in total.", (unsigned long long)n);
    double t0 = now_s();
    bbk_hamclusters *hc = nullptr;
    check(bbk_kmerset_hamming_clusters(ctx, set, 1, lock_size, chunk, &hc), "bbk_kmerset_hamming_clusters");
    ph.finish += now_s() - t0;

    t0 = now_s();
    std::vector<uint64_t> buf((size_t)n);  // one word per k-mer (k <= 32), then reused for the member indices
    check(bbk_kmerset_export(ctx, set, BBK_ORDER_SORTED, buf.data(), nullptr), "bbk_kmerset_export");
    write_u64(prefix + ".kmers", buf.data(), buf.size());
    bbk_kmerset_free(set);
    const uint64_t clusters = bbk_hamclusters_count(hc);
    std::vector<uint64_t> sizes((size_t)clusters);
    check(bbk_hamclusters_export(ctx, hc, nullptr, buf.data(), sizes.data()), "bbk_hamclusters_export");
    write_u64(prefix + ".hamming", buf.data(), buf.size());
    write_u64(prefix + ".hamming.idx", sizes.data(), sizes.size());
    ph.write = now_s() - t0;
    uint64_t largest = 0;
    for (uint64_t s : sizes) largest = s > largest ? s : largest;
    info("Clustering done. %llu k-mers, %llu clusters, largest cluster %llu, replayed k-mers %llu",
         (unsigned long long)n, (unsigned long long)clusters, (unsigned long long)largest,
         (unsigned long long)bbk_hamclusters_replayed(hc));
    bbk_hamclusters_free(hc);
    run.done("spades-hamcluster");
}
