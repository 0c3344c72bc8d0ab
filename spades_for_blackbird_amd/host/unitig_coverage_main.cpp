// unitig-coverage drop-in: same argv contract as the reference tool (projects/unitig_coverage/main.cpp:84-119)
//   <dataset description (in YAML)> <graph (in GFA)> <output filename> [-k <int=21>] [-t|--threads <int>] [--tmpdir <dir>]
//   (+ -b <bytes> and --device <int>, ours)
// and the same flow (:40-80): one sample per library of the dataset, in file order; the graph's (k+1)-mer index; every
// read of every sample mapped onto the graph; one abundance profile per edge written as EdgeProfileStorage::Save does.
// Each library is streamed block by block (-b bytes of input text per block, -t parser threads) through
// bbk_profiles_push_reads.  --tmpdir is accepted and unused (there are no temp files).  Only GFA graphs are read: the
// reference's toolchain::LoadGraph also takes a SPAdes binary graph pack, which this tool refuses.
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"

using namespace bbkhost;

static void usage(const char *argv0) {
    printf("SYNOPSIS\n        %s <dataset description (in YAML)> <graph (in GFA)> <output filename> [-k <value>]\n"
           "           [(-t|--threads) <value>] [--tmpdir <dir>]\n\n"
           "OPTIONS\n"
           "        -k <value>  k-mer length to use\n"
           "        -t, --threads <value>\n                    # of threads to use\n"
           "        --tmpdir <dir>\n                    scratch directory to use\n"
           "        -b <value>  bytes of input per streamed block\n"
           "        --device <value>  GPU to use (default 0)\n",
           argv0);
}

int main(int argc, char **argv) {
    unsigned k = 21, device = 0;
    unsigned long long threads = 0, bufsize = 536870912ull;
    std::vector<std::string> pos;
    Options opt;
    opt.num("-k", "", &k, 0u, 999u).num("-t", "--threads", &threads).num("-b", "", &bufsize, 1ull).num("", "--device", &device)
        .ignored("", "--tmpdir").positional(&pos);
    if (!opt.parse(argc, argv) || pos.size() != 3) {  // clipp's man page and exit(1) (:100-104)
        usage(argv[0]);
        return 1;
    }
    const std::string dataset = pos[0], graph = pos[1], outfile = pos[2];

    info("Starting computing unitig coverage profiles across a list of samples (MI355X, %s)", bbk_version());
    check_graph_k(k);
    info("K-mer length set to %u", k);
    require_gfa(graph);

    std::vector<DatasetLib> libs;
    std::string err;
    if (!load_dataset_libs(dataset, libs, err)) fatal("%s", err.c_str());
    const unsigned S = (unsigned)libs.size();

    Run run;
    Phases &ph = run.ph;
    run.create_ctx(device);
    bbk_ctx *ctx = run.ctx;
    info("Loading de Bruijn graph from %s", graph.c_str());
    double t0 = now_s();
    bbk_edgeindex *ix = nullptr;
    check(bbk_edgeindex_from_gfa(ctx, graph.c_str(), k, &ix), "bbk_edgeindex_from_gfa");
    info("Graph: %llu edges, %llu %u-mers indexed", (unsigned long long)bbk_edgeindex_segments(ix),
         (unsigned long long)bbk_edgeindex_size(ix), k + 1);
    bbk_profiles *prof = nullptr;
    check(bbk_profiles_begin(ctx, ix, S, &prof), "bbk_profiles_begin");
    const double t_index = now_s() - t0;

    const int nthreads = threads ? (int)threads : default_threads();
    for (unsigned s = 0; s < S; ++s) {
        std::vector<std::string> files;
        for (int kind = 0; kind < 5; ++kind)  // left, right, interlaced, merged, single (library.hpp:130-137)
            for (const std::string &f : libs[s].v[kind]) files.push_back(f);
        info("Sample %u: %zu file(s)", s, files.size());
        if (files.empty()) continue;
        stream_reads(ctx, files, (size_t)bufsize, nthreads, ph,
                     [&](bbk_reads *r) { check(bbk_profiles_push_reads(prof, s, r), "bbk_profiles_push_reads"); });
    }
    t0 = now_s();
    check(bbk_ctx_synchronize(ctx), "bbk_ctx_synchronize");
    ph.finish = t_index + (now_s() - t0);
    info("Saving profiles to %s", outfile.c_str());
    t0 = now_s();
    check(bbk_profiles_write(ctx, prof, outfile.c_str()), "bbk_profiles_write");
    ph.write = now_s() - t0;
    bbk_profiles_free(prof);
    bbk_edgeindex_free(ix);
    run.report("unitig-coverage");
    info("Computing unitig coverage profiles finished");
    run.leave();
}
