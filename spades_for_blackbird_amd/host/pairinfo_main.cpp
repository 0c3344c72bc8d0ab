// spades-pairinfo: the paired-end side of spades-core's PairInfoCount stage as a tool of its own (the reference has the
// stage only inside spades-core, projects/spades/pair_info_count.cpp:328-417, so this is a new tool and not a drop-in):
//   <graph (in GFA)> <dataset description (in YAML)> <output prefix> -k <value>
//   [-b <bytes>] [-t <value>] [--device <value>] [--min-edge-length <n>] [--meta] [--filter-threshold <t>]
//   [--max-distance-coeff <x>] [--rounding-coeff <x>] [--rounding-threshold <n>]
//   [--cluster] [--read-length <n>] [--linkage-distance-coeff <x>] [--clustered-filter-threshold <x>]
// Every paired-end library (left reads / right reads in lock step, with its orientation) is read twice: the estimate pass
// (CollectLibInformation, :199-243: insert sizes and edge pairs) and the fill pass (the DEFilter counts of :379-400 come
// from the estimate pass here; ProcessPairedReads, :285-324).  Per library i, counted from 0 over the dataset:
//   <prefix>.<i>.is.hist   "<insert size>\t<count>\n", ascending
//   <prefix>.<i>.lib       "key value" lines: the counters and the statistics, doubles as std::ostream prints them
//   <prefix>.<i>.prd       the raw paired index (bbk_pairinfo_write); absent when the insert size cannot be estimated
//   <prefix>.<i>.clustered.prd   with --cluster: the clustered index of the next stage, DistanceEstimation
//                          (projects/spades/distance_estimation.cpp:137-154; bbk_pairinfo_cluster, bbk_clustered_write),
//                          with the parameters of estimate_distance from the statistics above: insert size
//                          math::round(mean), delta size_t(deviation), linkage and maximal distance their coefficient
//                          times the deviation, read length the longest mate seen or --read-length
// The bound on the edge length is --min-edge-length, or with it the N50 of the graph unless --meta is given (:335-337).
// The defaults are the shipped configuration: raw_filter_threshold 2 (1 in meta_mode.info), max_distance_coeff 2.0,
// rounding_coeff 0.5, rounding_threshold 0 (configs/debruijn/distance_estimation.info), which makes the round bound 0.
// Refused, naming the library: mate-pair libraries and libraries whose reads are shorter than k (the reference maps both
// with BWA), and interlaced libraries.  Long-read, contig and single-read libraries are skipped.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "common.hpp"

using namespace bbkhost;

static void usage(const char *argv0) {
    printf("SYNOPSIS\n        %s <graph (in GFA)> <dataset description (in YAML)> <output prefix> -k <value>\n"
           "           [-b <value>] [-t <value>] [--device <value>] [--min-edge-length <value>] [--meta]\n"
           "           [--filter-threshold <value>] [--max-distance-coeff <value>] [--rounding-coeff <value>]\n"
           "           [--rounding-threshold <value>] [--cluster] [--read-length <value>]\n"
           "           [--linkage-distance-coeff <value>] [--clustered-filter-threshold <value>]\n\n"
           "OPTIONS\n"
           "        -k <value>  k-mer length of the graph\n"
           "        -b <value>  bytes of read sequence per batch\n"
           "        -t, --threads <value>\n                    # of threads to use\n"
           "        --device <value>  GPU to use (default 0)\n"
           "        --min-edge-length <value>\n                    shortest edge an insert size is taken from (default 0)\n"
           "        --meta      metagenomic mode: the bound is not raised to the N50 of the graph, filter threshold 1\n"
           "        --filter-threshold <value>\n                    edge pairs seen at most this often are dropped (default 2; 0: none)\n"
           "        --max-distance-coeff <value>, --rounding-coeff <value>, --rounding-threshold <value>\n"
           "                    distances are rounded to min(max-distance-coeff * deviation * rounding-coeff,\n"
           "                    rounding-threshold) (defaults 2.0, 0.5, 0: no rounding)\n"
           "        --cluster   also estimate distances: write <prefix>.<i>.clustered.prd (the maximal distance is\n"
           "                    max-distance-coeff * deviation)\n"
           "        --read-length <value>\n                    read length of the library (default: the longest mate seen)\n"
           "        --linkage-distance-coeff <value>\n                    graph distances this close (times the deviation) form one cluster (default 0.0)\n"
           "        --clustered-filter-threshold <value>\n                    clusters lighter than this are dropped (default 2.0)\n",
           argv0);
}

// Nx (assembly_graph/core/basic_graph_stats.hpp:97-113) over every edge of the graph: a segment is an edge and its
// conjugate, a self-conjugate segment one edge
static uint64_t graph_nx(const std::vector<uint64_t> &seg_len, const std::vector<uint8_t> &self_conj, double percent) {
    uint64_t sum = 0;
    std::vector<uint64_t> lengths;
    for (size_t s = 0; s < seg_len.size(); ++s)
        for (int c = self_conj[s] ? 1 : 2; c > 0; --c) {
            lengths.push_back(seg_len[s]);
            sum += seg_len[s];
        }
    std::sort(lengths.begin(), lengths.end());
    double len_perc = (1.0 - percent * 0.01) * (double)sum;
    for (size_t i = 0; i < lengths.size(); ++i) {
        if ((double)lengths[i] >= len_perc) return lengths[i];
        len_perc -= (double)lengths[i];
    }
    return 0;
}

// the mates of a batch, cut to their LongestValid stretches, and what was cut (left1, right1, left2, right2 per pair)
struct PairBatch {
    std::string bases[2];
    std::vector<uint64_t> off[2];
    std::vector<uint32_t> cut;
    PairBatch() { clear(); }
    void clear() {
        for (int m = 0; m < 2; ++m) {
            bases[m].clear();
            off[m].assign(1, 0);
        }
        cut.clear();
    }
    uint64_t pairs() const { return off[0].size() - 1; }
    size_t bytes() const { return bases[0].size() + bases[1].size(); }
    void add(int m, const std::string &seq) {
        size_t from, to;
        detail::longest_valid(seq.data(), seq.size(), &from, &to);  // LongestValidCoords (ingest.hpp)
        bases[m].append(seq, from, to - from);
        off[m].push_back(bases[m].size());
        cut.push_back((uint32_t)(to > from ? from : 0));
        cut.push_back((uint32_t)(to > from ? seq.size() - to : 0));
    }
};

// one pass over a library: every batch of pairs goes to push(first, second, h_cut); returns the longest read seen
template <class Push>
static size_t for_each_batch(bbk_ctx *ctx, const DatasetLib &L, size_t batch_bytes, uint64_t &n_pairs, Push push) {
    PairBatch b;
    size_t max_len = 0;
    n_pairs = 0;
    auto flush = [&] {
        if (b.pairs() == 0) return;
        bbk_reads *r[2] = {nullptr, nullptr};
        for (int m = 0; m < 2; ++m)
            check(bbk_reads_from_ascii(ctx, b.bases[m].data(), b.off[m].data(), b.pairs(), &r[m]), "bbk_reads_from_ascii");
        push(r[0], r[1], b.cut.data());
        bbk_reads_free(r[0]);
        bbk_reads_free(r[1]);
        n_pairs += b.pairs();
        b.clear();
    };
    for (size_t i = 0; i < L.v[LIB_LEFT].size(); ++i) {
        FastxReader r1(L.v[LIB_LEFT][i]), r2(L.v[LIB_RIGHT][i]);
        if (!r1.is_open()) fatal("Cannot open %s", L.v[LIB_LEFT][i].c_str());
        if (!r2.is_open()) fatal("Cannot open %s", L.v[LIB_RIGHT][i].c_str());
        info("Processing %s and %s", L.v[LIB_LEFT][i].c_str(), L.v[LIB_RIGHT][i].c_str());
        std::string n1, s1, q1, n2, s2, q2;
        // a pair needs both mates: the stream ends with the shorter file
        while (r1.next_record(n1, s1, q1) && r2.next_record(n2, s2, q2)) {
            max_len = std::max(max_len, std::max(s1.size(), s2.size()));
            b.add(0, s1);
            b.add(1, s2);
            if (b.bytes() >= batch_bytes) flush();
        }
    }
    flush();
    return max_len;
}

static std::string lib_text(const bbk_pairinfo_stats &st) {
    char buf[128];
    std::string o;
    auto u = [&](const char *key, unsigned long long v) { o.append(buf, (size_t)snprintf(buf, sizeof(buf), "%s %llu\n", key, v)); };
    auto d = [&](const char *key, double v) { o.append(buf, (size_t)snprintf(buf, sizeof(buf), "%s %g\n", key, v)); };
    u("total", st.total);
    u("mapped", st.mapped);
    u("negative", st.negative);
    u("edge_pairs", st.edge_pairs);
    d("mean", st.mean);
    d("deviation", st.deviation);
    d("median", st.median);
    d("mad", st.mad);
    d("left_quantile", st.left_quantile);
    d("right_quantile", st.right_quantile);
    for (int i = 0; i < 19; ++i)
        o.append(buf, (size_t)snprintf(buf, sizeof(buf), "percentile_%d %llu\n", 5 * (i + 1), (unsigned long long)st.percentiles[i]));
    u("ok", st.ok ? 1 : 0);
    return o;
}

static int orientation_of(const std::string &o, size_t lib) {
    if (o.empty() || o == "fr") return BBK_ORIENT_FR;  // (the default of a paired-end library, pipeline/library.cpp)
    if (o == "ff") return BBK_ORIENT_FF;
    if (o == "rf") return BBK_ORIENT_RF;
    if (o == "rr") return BBK_ORIENT_RR;
    fatal("library #%zu: unknown orientation \"%s\"", lib, o.c_str());
}

struct Settings {  // (threads: the mates are read in lock step by one thread; accepted as every tool accepts it)
    unsigned k = 0, device = 0, filter_threshold = 2, rounding_thr = 0;
    unsigned long long threads = 0, bufsize = 268435456ull, min_edge_length = 0, read_length = 0;
    double max_distance_coeff = 2.0, rounding_coeff = 0.5, linkage_coeff = 0.0, clustered_threshold = 2.0;
    bool meta = false, cluster = false, read_length_given = false;
};

struct Library {  // one paired-end library on its way through estimate_library, fill_library and cluster_library
    const DatasetLib &L;
    size_t i;  // its number in the dataset
    int orientation;
    std::string base;  // <prefix>.<i>
    bbk_pairinfo *pi = nullptr;
    bbk_pairinfo_stats st{};
    size_t rl = 0;  // the longest read seen
};

// the estimate pass, <base>.is.hist and <base>.lib; false: the insert size cannot be estimated, the library ends here
static bool estimate_library(bbk_ctx *ctx, const bbk_edgeindex *ix, const Settings &s, Library &lib) {
    info("Estimating insert size for library #%zu", lib.i);
    bbk_pairinfo *&pi = lib.pi;
    check(bbk_pairinfo_begin(ctx, ix, s.min_edge_length, &pi), "bbk_pairinfo_begin");
    uint64_t n_pairs = 0;
    const size_t rl = lib.rl = for_each_batch(ctx, lib.L, (size_t)s.bufsize, n_pairs, [&](bbk_reads *a, bbk_reads *b, const uint32_t *cut) {
        check(bbk_pairinfo_push_estimate(pi, a, b, lib.orientation, cut), "bbk_pairinfo_push_estimate");
    });
    if (n_pairs > 0 && rl < s.k)
        fatal("library #%zu: its reads (at most %zu bases) are shorter than K (%u): the reference maps such a library "
              "with BWA, which is not supported", lib.i, rl, s.k);
    bbk_pairinfo_stats &st = lib.st;
    check(bbk_pairinfo_estimate(pi, &st), "bbk_pairinfo_estimate");
    info("Edge pairs: %llu", (unsigned long long)st.edge_pairs);
    info("%llu paired reads (%g%% of all) aligned to long edges", (unsigned long long)st.mapped,
         (double)st.mapped * 100.0 / (double)st.total);
    if (st.negative > 3 * st.mapped)
        info("WARN Too much reads aligned with negative insert size. Is the library orientation set properly?");
    const uint64_t nh = bbk_pairinfo_hist_size(pi);
    std::vector<int32_t> is(nh);
    std::vector<uint64_t> cnt(nh);
    check(bbk_pairinfo_hist_export(pi, is.data(), cnt.data()), "bbk_pairinfo_hist_export");
    std::string text;
    char buf[64];
    for (uint64_t j = 0; j < nh; ++j)
        text.append(buf, (size_t)snprintf(buf, sizeof(buf), "%d\t%llu\n", is[j], (unsigned long long)cnt[j]));
    write_text(lib.base + ".is.hist", text);
    write_text(lib.base + ".lib", lib_text(st));
    if (!st.ok) {  // pair_info_count.cpp:356-367
        info("WARN Unable to estimate insert size for paired library #%zu", lib.i);
        if (rl > 0 && rl <= s.k) info("WARN Maximum read length (%zu) should be greater than K (%u)", rl, s.k);
        else if (rl <= (size_t)s.k * 11 / 10) info("WARN Maximum read length (%zu) is probably too close to K (%u)", rl, s.k);
        else info("WARN None of paired reads aligned properly. Please, check orientation of your read pairs.");
        return false;
    }
    info("  Insert size = %g, deviation = %g, left quantile = %g, right quantile = %g, read length = %zu", st.mean,
         st.deviation, st.left_quantile, st.right_quantile, rl);
    if (st.mean < 1.1 * (double)rl)
        info("WARN Estimated mean insert size %g is very small compared to read length %zu", st.mean, rl);
    return true;
}

// the fill pass and <base>.prd
static void fill_library(bbk_ctx *ctx, const Settings &s, Library &lib) {
    unsigned round_thr = 0;  // pair_info_count.cpp:292-296: no rounding when the filter is off
    if (s.filter_threshold)
        round_thr = (unsigned)std::min(s.max_distance_coeff * lib.st.deviation * s.rounding_coeff, (double)s.rounding_thr);
    info("Left insert size quantile %g, right insert size quantile %g, filtering threshold %u, rounding threshold %u",
         lib.st.left_quantile, lib.st.right_quantile, s.filter_threshold, round_thr);
    info("Mapping library #%zu", lib.i);
    check(bbk_pairinfo_fill_begin(lib.pi, (uint64_t)lib.st.mean, round_thr, s.filter_threshold), "bbk_pairinfo_fill_begin");
    uint64_t n_pairs = 0;
    for_each_batch(ctx, lib.L, (size_t)s.bufsize, n_pairs, [&](bbk_reads *a, bbk_reads *b, const uint32_t *cut) {
        check(bbk_pairinfo_push_fill(lib.pi, a, b, lib.orientation, cut), "bbk_pairinfo_push_fill");
    });
    check(bbk_pairinfo_fill_finish(lib.pi), "bbk_pairinfo_fill_finish");
    info("Paired index: %llu points; saving to %s.prd", (unsigned long long)bbk_pairinfo_points(lib.pi), lib.base.c_str());
    check(bbk_pairinfo_write(lib.pi, (lib.base + ".prd").c_str()), "bbk_pairinfo_write");
}

// estimate_distance (distance_estimation.cpp:137-154) and <base>.clustered.prd
static void cluster_library(const Settings &s, Library &lib) {
    bbk_cluster_params prm;
    prm.insert_size = (uint64_t)std::floor(lib.st.mean + 0.5 + 1e-10);  // math::round (math/xmath.h:324-330)
    prm.read_length = s.read_length_given ? s.read_length : lib.rl;
    prm.delta = (uint64_t)lib.st.deviation;
    prm.linkage_distance = (uint64_t)(s.linkage_coeff * lib.st.deviation);
    prm.max_distance = (uint64_t)(s.max_distance_coeff * lib.st.deviation);
    prm.filter_threshold = s.clustered_threshold;
    info("Estimating distances: insert size %llu, read length %llu, delta %llu, linkage distance %llu, max distance %llu",
         (unsigned long long)prm.insert_size, (unsigned long long)prm.read_length, (unsigned long long)prm.delta,
         (unsigned long long)prm.linkage_distance, (unsigned long long)prm.max_distance);
    bbk_clustered *cl = nullptr;
    check(bbk_pairinfo_cluster(lib.pi, &prm, &cl), "bbk_pairinfo_cluster");
    info("Clustered index: %llu points of %llu edge pairs (%llu searched on the host); saving to %s.clustered.prd",
         (unsigned long long)bbk_clustered_points(cl), (unsigned long long)bbk_clustered_pairs(cl),
         (unsigned long long)bbk_clustered_host_pairs(cl), lib.base.c_str());
    check(bbk_clustered_write(cl, (lib.base + ".clustered.prd").c_str()), "bbk_clustered_write");
    bbk_clustered_free(cl);
}

// what cannot be done is refused before anything is written; paired[i]: library i is a paired-end library to process
static std::vector<int> check_libraries(const std::vector<DatasetLib> &libs) {
    std::vector<int> paired(libs.size(), 0);
    for (size_t i = 0; i < libs.size(); ++i) {
        const DatasetLib &L = libs[i];
        const std::string &t = L.type;
        if (t == "mate-pairs" || t == "hq-mate-pairs" || t == "nxmate")
            fatal("library #%zu: mate-pair libraries (%s) are not supported: the reference maps them with BWA", i, t.c_str());
        if (!t.empty() && t != "paired-end") {
            info("Library #%zu (%s) is not a paired-end library, skipping", i, t.c_str());
            continue;
        }
        if (!L.v[LIB_INTERLACED].empty())
            fatal("library #%zu: interlaced reads are not supported: give the mates as left reads / right reads", i);
        if (L.v[LIB_LEFT].empty() && L.v[LIB_RIGHT].empty()) {
            info("Library #%zu has no paired reads, skipping", i);
            continue;
        }
        if (L.v[LIB_LEFT].size() != L.v[LIB_RIGHT].size())
            fatal("library #%zu: %zu left but %zu right read files", i, L.v[LIB_LEFT].size(), L.v[LIB_RIGHT].size());
        orientation_of(L.orientation, i);
        paired[i] = 1;
    }
    return paired;
}

int main(int argc, char **argv) {
    Settings s;
    std::vector<std::string> pos;
    Options opt;
    opt.num("-k", "", &s.k, 0u, 999u).num("-t", "--threads", &s.threads).num("-b", "", &s.bufsize, 1ull)
        .num("", "--device", &s.device).num("", "--min-edge-length", &s.min_edge_length).flag("", "--meta", &s.meta)
        .num("", "--filter-threshold", &s.filter_threshold).real("", "--max-distance-coeff", &s.max_distance_coeff)
        .real("", "--rounding-coeff", &s.rounding_coeff).num("", "--rounding-threshold", &s.rounding_thr).flag("", "--cluster", &s.cluster)
        .num("", "--read-length", &s.read_length).real("", "--linkage-distance-coeff", &s.linkage_coeff)
        .real("", "--clustered-filter-threshold", &s.clustered_threshold).positional(&pos);
    if (!opt.parse(argc, argv) || pos.size() != 3 || !opt.seen("-k")) {
        usage(argv[0]);
        return 1;
    }
    if (s.meta && !opt.seen("--filter-threshold")) s.filter_threshold = 1;  // raw_filter_threshold of meta_mode.info
    s.read_length_given = opt.seen("--read-length");
    const std::string graph = pos[0], dataset = pos[1], prefix = pos[2];
    const unsigned k = s.k;
    info("Starting paired info counting (MI355X, %s)", bbk_version());
    check_graph_k(k);
    info("K-mer length set to %u", k);
    require_gfa(graph);
    std::vector<DatasetLib> libs;
    std::string err;
    if (!load_dataset_libs(dataset, libs, err)) fatal("%s", err.c_str());
    const std::vector<int> paired = check_libraries(libs);
    Run run;
    run.create_ctx(s.device);
    bbk_ctx *ctx = run.ctx;
    info("Loading de Bruijn graph from %s", graph.c_str());
    bbk_edgeindex *ix = nullptr;
    if (s.cluster) check(bbk_edgeindex_from_gfa_with_graph(ctx, graph.c_str(), k, &ix), "bbk_edgeindex_from_gfa_with_graph");
    else check(bbk_edgeindex_from_gfa(ctx, graph.c_str(), k, &ix), "bbk_edgeindex_from_gfa");
    const uint64_t ns = bbk_edgeindex_segments(ix);
    info("Graph: %llu edges, %llu %u-mers indexed", (unsigned long long)ns, (unsigned long long)bbk_edgeindex_size(ix), k + 1);
    if (!s.meta) {  // the bound is raised to the N50 of the graph
        std::vector<uint64_t> seg_len(ns);
        std::vector<uint8_t> self_conj(ns);
        check(bbk_edgeindex_export_segments(ix, seg_len.data(), self_conj.data()), "bbk_edgeindex_export_segments");
        s.min_edge_length = std::max<unsigned long long>(s.min_edge_length, graph_nx(seg_len, self_conj, 50));
    }
    info("Min edge length for estimation: %llu", s.min_edge_length);

    for (size_t i = 0; i < libs.size(); ++i) {
        if (!paired[i]) continue;
        Library lib{libs[i], i, orientation_of(libs[i].orientation, i), prefix + "." + std::to_string(i)};
        if (estimate_library(ctx, ix, s, lib)) {
            fill_library(ctx, s, lib);
            if (s.cluster) cluster_library(s, lib);
        }
        bbk_pairinfo_free(lib.pi);
    }
    bbk_edgeindex_free(ix);
    info("Paired info counting finished");
    run.done("spades-pairinfo");
}
