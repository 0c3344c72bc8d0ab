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
    bool bad = false;
    std::vector<std::string> pos;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        unsigned long long v = 0;
        auto need = [&](unsigned long long *x) { return i + 1 < argc && parse_uint(argv[++i], x); };
        if (a == "-k") { if (need(&v) && v < 1000) k = (unsigned)v; else bad = true; }
        else if (a == "-t" || a == "--threads") { if (need(&v)) threads = v; else bad = true; }
        else if (a == "-b") { if (need(&v) && v > 0) bufsize = v; else bad = true; }
        else if (a == "--device") { if (need(&v)) device = (unsigned)v; else bad = true; }
        else if (a == "--tmpdir") { if (i + 1 < argc) ++i; else bad = true; }
        else if (!a.empty() && a[0] == '-' && a.size() > 1) bad = true;
        else pos.push_back(a);
    }
    if (bad || pos.size() != 3) {  // clipp's man page and exit(1) (:100-104)
        usage(argv[0]);
        return 1;
    }
    const std::string dataset = pos[0], graph = pos[1], outfile = pos[2];

    info("Starting computing unitig coverage profiles across a list of samples (MI355X, %s)", bbk_version());
    if (k < 1) fatal("k-mer size %u is too low", k);
    if (k >= BBK_MAX_K) fatal("k-mer size %u is too high, recompile with larger SPADES_MAX_K option", k);
    if (k % 2 == 0) fatal("k-mer size must be odd");
    info("K-mer length set to %u", k);
    if (!ends_with(graph, ".gfa"))
        fatal("graph %s: only a GFA graph (*.gfa) is read; the SPAdes binary graph pack is not supported", graph.c_str());

    std::vector<DatasetLib> libs;
    std::string err;
    if (!load_dataset_libs(dataset, libs, err)) fatal("%s", err.c_str());
    const unsigned S = (unsigned)libs.size();

    Phases ph;
    const double t_start = now_s();
    bbk_ctx *ctx = nullptr;
    double t0 = now_s();
    check(bbk_ctx_create((int)device, &ctx), "bbk_ctx_create");
    ph.ctx = now_s() - t0;
    info("Loading de Bruijn graph from %s", graph.c_str());
    t0 = now_s();
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
    ph.total = now_s() - t_start;
    ph.memory(ctx);
    ph.report("unitig-coverage");
    info("Computing unitig coverage profiles finished");
    finish_process(ctx, 0);
}
