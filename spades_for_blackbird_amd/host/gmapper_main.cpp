// spades-gmapper drop-in: same argv contract as the reference tool (projects/gmapper/main.cpp:65-82)
//   <dataset description (in YAML)> <graph (in GFA)> <output filename> [-k <int=21>] [-t <int>] [--tmp-dir <dir>]
//   (+ -b <bytes> and --device <int>, ours)
// and its flow for contig libraries (:156-247):
//   - the graph as GFAReader::to_graph builds it (io/graph/gfa_reader.cpp:54-148): segment i is edge 2i, its conjugate
//     2i+1 (a palindromic segment is the one self-conjugate edge 2i), one vertex pair created as the end of each edge,
//     then the links applied arc by arc with ConstructionHelper::LinkEdges (construction_helper.hpp:95-99), which MOVES
//     the start of the second edge onto the end of the first.  The arcs are the gfa library's (ext/src/gfa1/gfa.c): one
//     per L line plus the complement of every L line whose complement is not in the file (gfa_fix_symm), grouped by
//     source (segment, orientation) in file order.  That is the library's order when its arc sort is stable: always for
//     up to 64 arcs (insertion sort, ksort.h:181); above, its in-place MSD radix sort may permute the arcs of one
//     source.  Where every junction is complete (a spades-gbuilder graph) the order of the arcs does not change the
//     graph; on a larger GFA with partial junctions the vertices may then differ from the reference's;
//   - every contig cut at N (MapRead, sequence_mapper.hpp:68-98) and its pieces mapped on the GPU in blocks of -b bytes
//     of contig text (bbk_edgeindex_map_paths: MapSequence of every piece, csrc/edgeprof.hip);
//   - GappedPathExtractor (long_read_mapper.cpp:201-326) with TryCloseGap (a bounded Dijkstra and PathProcessor's
//     backward DFS, path_processor.hpp), PathStorage (long_read_storage.hpp:66-265) and GFAPathWriter
//     (bidirectional_path_output.hpp:70-107) after GFAWriter::WriteSegmentsAndLinks (io/graph/gfa_writer.cpp).
// The output is rewritten for every contig library, so the last one wins; without one nothing is written.  Refused:
// trusted-contigs (GappedPathExtractorForTrustedContigs reads cfg::get().ha.trusted_aligner_config, which gmapper never
// loads), long-read libraries (PacbioAlignLibrary is not ported), a graph that is not GFA (the SPAdes binary graph pack
// is not read), and a contig holding a character other than ACGTN after upper-casing (the reference aborts in
// Sequence).  Other library types are skipped with the reference's warning.  --tmp-dir is accepted and unused.
#include <algorithm>
#include <cstring>
#include <map>
#include <queue>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../csrc/gfa_graph.h"
#include "common.hpp"

using namespace bbkhost;

namespace {

constexpr uint64_t kLengthBound = 70;            // MappingPathFixer::LENGTH_BOUND_DEFAULT
constexpr uint64_t kMinMappedLength = 100;       // GappedPathExtractor::MIN_MAPPED_LENGTH
constexpr double kMinMappedRatio = 0.3;          // GappedPathExtractor::MIN_MAPPED_RATIO
constexpr uint64_t kMaxCallCnt = 3000;           // PathProcessor::MAX_CALL_CNT
constexpr uint64_t kMaxDijkstraVertices = 3000;  // PathProcessor::MAX_DIJKSTRA_VERTICES
constexpr uint64_t kUsageThreshold = 500;        // PathProcessor::VERTEX_USAGE_ENABLE_THRESHOLD
constexpr uint64_t kMaxVertexUsage = 5;          // PathProcessor::MAX_VERTEX_USAGE

void warn(const char *msg) {
    const double el = now_s() - t0_ref();
    printf("%3d:%02d:%02d.%03d  WARN  %s\n", (int)(el / 3600), (int)(el / 60) % 60, (int)el % 60,
           (int)((el - (long)el) * 1000), msg);
    fflush(stdout);
}

// math::gr (common/math/xmath.h): a > b and more than 4 ULPs apart
bool gr(double a, double b) {
    auto biased = [](double x) {
        uint64_t u;
        memcpy(&u, &x, 8);
        return (u >> 63) ? ~u + 1 : (u | (1ull << 63));
    };
    const uint64_t x = biased(a), y = biased(b);
    return (x > y ? x - y : y - x) > 4 && a > b;
}

typedef uint32_t Edge;    // 2 * segment, + 1 on the reverse strand; these numbers order as the reference's edge ids
typedef uint32_t Vertex;  // 4 * segment (+ 2: created as the end of edge 2 * segment + 1), + 1: the conjugate

struct Graph {
    unsigned k = 0;
    uint64_t ns = 0;
    std::vector<std::string> names;
    std::string bases;
    std::vector<uint64_t> off;
    std::vector<uint32_t> kc;
    std::vector<uint8_t> selfc;
    std::vector<Vertex> end;       // EdgeEnd of every edge
    std::vector<uint64_t> out_off;  // OutgoingEdges of every vertex, ascending (AddOutgoingEdge, graph_core.hpp:193)
    std::vector<Edge> out_e;

    bool exists(Edge e) const { return !(e & 1) || !selfc[e >> 1]; }
    Edge conj(Edge e) const { return selfc[e >> 1] ? e : e ^ 1u; }
    Vertex start(Edge e) const { return end[conj(e)] ^ 1u; }
    uint64_t length(Edge e) const { return off[(e >> 1) + 1] - off[e >> 1] - k; }
    double coverage(Edge e) const { return (double)kc[e >> 1] / (double)length(e); }
    const Edge *out_begin(Vertex v) const { return out_e.data() + out_off[v]; }
    const Edge *out_end(Vertex v) const { return out_e.data() + out_off[v + 1]; }
    // CanonicalEdgeHelper::EdgeOrientationString with the segment names (MapNamingF)
    void orient(Edge e, const char *delim, std::string &o) const {
        o += names[e >> 1];
        o += delim;
        o += (e & 1) ? '-' : '+';
    }
};

// GFAReader::to_graph over the graph the index has parsed.  Returns the number of one-(k+1)-mer homopolymer edges whose
// loop flag in the index (an L line from the segment to itself) differs from "e is among OutgoingEdges(EdgeEnd(e))"
// here: csrc/edgeprof.hip explains why that changes the cut of ranges only, not this tool's output.
uint64_t build_graph(const bbk_edgeindex *ix, unsigned k, int threads, Graph &g) {
    g.k = k;
    g.ns = bbk_edgeindex_segments(ix);
    const uint64_t ns = g.ns, nx = 2 * ns, nv = 4 * ns;
    if (ns >= (1ull << 30)) fatal("graph: %llu segments, at most 2^30 - 1 are supported", (unsigned long long)ns);
    const uint64_t nl = bbk_edgeindex_links(ix);
    g.names.resize(ns);
    for (uint64_t s = 0; s < ns; ++s) g.names[s] = bbk_edgeindex_name(ix, s);
    g.bases.resize(bbk_edgeindex_total_bases(ix));
    g.off.resize(ns + 1);
    g.kc.resize(ns);
    std::vector<uint32_t> links(4 * nl + 4);
    check(bbk_edgeindex_export_graph(ix, &g.bases[0], g.off.data(), links.data(), g.kc.data()),
          "bbk_edgeindex_export_graph");
    g.selfc.assign(ns, 0);
#pragma omp parallel for schedule(static) num_threads(threads)
    for (int64_t s = 0; s < (int64_t)ns; ++s)
        g.selfc[s] = bbk::segment_is_self_conjugate(g.bases.data() + g.off[s], g.off[s + 1] - g.off[s]);
    g.end.assign(nx, 0);
    for (uint64_t s = 0; s < ns; ++s) {  // LinkIncomingEdge: edge 2s ends at vertex 4s, edge 2s + 1 at 4s + 2
        g.end[2 * s] = (Vertex)(4 * s);
        if (!g.selfc[s]) g.end[2 * s + 1] = (Vertex)(4 * s + 2);
    }
    // arcs over oriented segments x = 2 * segment + (x is '-')
    typedef std::pair<uint32_t, uint32_t> Arc;
    std::vector<Arc> arcs(nl);
    for (uint64_t j = 0; j < nl; ++j)
        arcs[j] = {(uint32_t)(2 * links[4 * j] + (links[4 * j + 1] ? 0 : 1)),
                   (uint32_t)(2 * links[4 * j + 2] + (links[4 * j + 3] ? 0 : 1))};
    std::vector<uint64_t> first, order;
    auto group = [&](const std::vector<Arc> &a) {  // stable by source
        first.assign(nx + 1, 0);
        for (const Arc &x : a) ++first[x.first + 1];
        for (uint64_t v = 0; v < nx; ++v) first[v + 1] += first[v];
        std::vector<uint64_t> fill(first.begin(), first.end() - 1);
        order.resize(a.size());
        for (uint64_t j = 0; j < a.size(); ++j) order[fill[a[j].first]++] = j;
    };
    group(arcs);
    std::vector<uint8_t> is_comp(nl, 0);
    std::vector<Arc> all(arcs);
    for (uint64_t v = 0; v < nx; ++v)  // gfa_fix_symm
        for (uint64_t i = first[v]; i < first[v + 1]; ++i) {
            const uint64_t j = order[i];
            if (is_comp[j]) continue;
            const uint32_t w = arcs[j].second;
            bool found = false;
            for (uint64_t i2 = first[w ^ 1u]; i2 < first[(w ^ 1u) + 1] && !found; ++i2) {
                const uint64_t j2 = order[i2];
                if (!is_comp[j2] && arcs[j2].second == ((uint32_t)v ^ 1u)) {
                    is_comp[j2] = 1;
                    found = true;
                }
            }
            if (!found) all.push_back({w ^ 1u, (uint32_t)v ^ 1u});
        }
    group(all);
    for (uint64_t j : order) {  // LinkEdges(e1, e2): e2 leaves its start for the end of e1
        const Edge e1 = g.selfc[all[j].first >> 1] ? (all[j].first & ~1u) : all[j].first;
        const Edge e2 = g.selfc[all[j].second >> 1] ? (all[j].second & ~1u) : all[j].second;
        g.end[g.conj(e2)] = g.end[e1] ^ 1u;
    }
    g.out_off.assign(nv + 1, 0);
    for (Edge e = 0; e < nx; ++e)
        if (g.exists(e)) ++g.out_off[g.start(e) + 1];
    for (uint64_t v = 0; v < nv; ++v) g.out_off[v + 1] += g.out_off[v];
    g.out_e.resize(g.out_off[nv]);
    std::vector<uint64_t> fill(g.out_off.begin(), g.out_off.end() - 1);
    for (Edge e = 0; e < nx; ++e)
        if (g.exists(e)) g.out_e[fill[g.start(e)]++] = e;
    std::vector<uint8_t> self_linked(ns, 0);
    for (uint64_t j = 0; j < nl; ++j)
        if (links[4 * j] == links[4 * j + 2] && links[4 * j + 1] == links[4 * j + 3]) self_linked[links[4 * j]] = 1;
    uint64_t differ = 0;
    for (uint64_t s = 0; s < ns; ++s) {
        const Edge e = (Edge)(2 * s);
        if (g.length(e) != 1) continue;
        const bool looped = std::find(g.out_begin(g.end[e]), g.out_end(g.end[e]), e) != g.out_end(g.end[e]);
        if (bbk::is_homopolymer_k1(g.bases.data() + g.off[s], k + 1) && looped != (bool)self_linked[s]) ++differ;
    }
    return differ;
}

// MappingPathFixer::TryCloseGap (sequence_mapper.hpp:204-235): the first path ProcessPaths(g, 0, 70, v1, v2) finds
struct GapCloser {
    const Graph &g;
    std::unordered_map<Vertex, uint64_t> dist, usage;
    std::vector<Edge> rev;
    uint64_t len = 0, calls = 0;
    bool found = false;
    Vertex from = 0;
    explicit GapCloser(const Graph &graph) : g(graph) {}

    // DijkstraHelper::CreateBoundedDijkstra(g, 70, 3000).Run(s) (dijkstra_algorithm.hpp:166-200): queue order (distance,
    // vertex, previous vertex, edge) as ReverseDistanceComparator
    void dijkstra(Vertex s) {
        dist.clear();
        typedef std::tuple<uint64_t, int64_t, int64_t, int64_t> El;
        std::priority_queue<El, std::vector<El>, std::greater<El>> q;
        q.emplace(0, (int64_t)s, -1, -1);
        uint64_t n = 0;
        while (!q.empty()) {
            const El t = q.top();
            q.pop();
            const uint64_t d = std::get<0>(t);
            const Vertex v = (Vertex)std::get<1>(t);
            if (!dist.emplace(v, d).second) continue;
            ++n;
            if (n > kMaxDijkstraVertices || !(n < kMaxDijkstraVertices && d <= kLengthBound)) continue;
            for (const Edge *e = g.out_begin(v); e != g.out_end(v); ++e) {
                const Vertex w = g.end[*e];
                const uint64_t nd = d + g.length(*e);
                if (!dist.count(w) && nd <= kLengthBound) q.emplace(nd, (int64_t)w, (int64_t)v, (int64_t)*e);
            }
        }
    }

    // PathProcessor::Traversal::Go (path_processor.hpp:111-150) over incoming edges; true ends the search: the call
    // limit, or the first path found (the reference goes on, but only the first path is used)
    bool go(Vertex v) {
        if (++calls >= kMaxCallCnt) return true;
        if (v == from) {
            found = true;
            return true;
        }
        std::vector<Edge> inc;
        for (const Edge *e = g.out_begin(v ^ 1u); e != g.out_end(v ^ 1u); ++e)
            if (dist.count(g.start(g.conj(*e)))) inc.push_back(g.conj(*e));
        std::stable_sort(inc.begin(), inc.end(), [&](Edge a, Edge b) {  // as libstdc++'s insertion sort of <= 16 items
            const uint64_t da = dist.at(g.start(a)), db = dist.at(g.start(b));
            if (da != db) return da < db;
            return g.coverage(a) > g.coverage(b);
        });
        for (const Edge e : inc) {
            const Vertex s = g.start(e);
            if (dist.at(s) + g.length(e) + len > kLengthBound) continue;
            if (calls >= kUsageThreshold && usage[s] >= kMaxVertexUsage) continue;
            len += g.length(e);
            rev.push_back(e);
            ++usage[s];
            const bool stop = go(s);
            if (stop) return true;  // rev holds the path when found
            --usage[s];
            rev.pop_back();
            len -= g.length(e);
        }
        return false;
    }

    // appends the closing path to out; false when there is none
    bool close(Vertex a, Vertex b, std::vector<Edge> &out) {
        if (a == b) return false;
        dijkstra(a);
        const auto it = dist.find(b);
        if (it == dist.end() || it->second > kLengthBound) return false;
        from = a;
        rev.clear();
        usage.clear();
        usage[b] = 1;
        len = calls = 0;
        found = false;
        go(b);
        if (found) out.insert(out.end(), rev.rbegin(), rev.rend());
        return found;
    }
};

// GappedPathExtractor on one contig's mapping path, given as (edge, initial-range size) per range
void extract_paths(const Graph &g, GapCloser &gc, const std::vector<std::pair<Edge, uint64_t>> &mp,
                   std::vector<std::vector<Edge>> &paths) {
    std::vector<Edge> kept;  // DeleteSameEdges, then FilterBadMappings with CountMappedEdgeSize over each run of an edge
    for (size_t i = 0, j; i < mp.size(); i = j) {
        uint64_t size = 0;
        for (j = i; j < mp.size() && mp[j].first == mp[i].first; ++j) size += mp[j].second;
        const Edge e = mp[i].first;
        if (size > kMinMappedLength || gr((double)size / (double)g.length(e), kMinMappedRatio)) kept.push_back(e);
    }
    if (kept.empty()) return;
    std::vector<Edge> cur{kept[0]};
    for (size_t i = 1; i < kept.size(); ++i) {  // FindReadPathWithGaps
        const Vertex l = g.end[kept[i - 1]], r = g.start(kept[i]);
        if (l != r && !gc.close(l, r, cur)) {
            paths.push_back(std::move(cur));
            cur.clear();
        }
        cur.push_back(kept[i]);
    }
    paths.push_back(std::move(cur));
}

// GFAPathWriter: WriteSegmentsAndLinks (gfa_writer.cpp:18-52), then WritePaths for every stored path
void write_output(const Graph &g, const std::map<std::vector<Edge>, uint64_t> &paths, const std::string &path,
                  int threads) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) fatal("cannot open %s for writing", path.c_str());
    bool fail = false;
    auto put = [&](const std::string &t) {
        if (!t.empty() && fwrite(t.data(), 1, t.size(), f) != t.size()) fail = true;
        return true;  // the failure is reported after the last write
    };
    // items formatted in blocks, 64 blocks at a time.  S lines of the canonical edges: DP = float(raw / length), KC = raw
    bbk::format_blocks(g.ns, threads, 64, put, [&](uint64_t s, std::string &o) {
        char tail[96];
        snprintf(tail, sizeof(tail), "\tDP:f:%g\tKC:i:%u\n", (double)(float)g.coverage((Edge)(2 * s)), g.kc[s]);
        o += "S\t";
        o += g.names[s];
        o += '\t';
        o.append(g.bases, g.off[s], g.off[s + 1] - g.off[s]);
        o += tail;
    });
    const std::string ovl = "\t" + std::to_string(g.k) + "M\n";
    // L lines at canonical vertex 2h: incoming x outgoing
    bbk::format_blocks(2 * g.ns, threads, 64, put, [&](uint64_t h, std::string &o) {
        const Vertex v = (Vertex)(2 * h);
        for (const Edge *a = g.out_begin(v ^ 1u); a != g.out_end(v ^ 1u); ++a)
            for (const Edge *b = g.out_begin(v); b != g.out_end(v); ++b) {
                o += "L\t";
                g.orient(g.conj(*a), "\t", o);
                o += '\t';
                g.orient(*b, "\t", o);
                o += ovl;
            }
    });
    uint64_t idx = 0;
    std::string o;
    for (const auto &pw : paths) {  // a new P line wherever consecutive edges are not adjacent (the reference's spelling)
        const std::vector<Edge> &p = pw.first;
        const std::string name = "P\tPATH_" + std::to_string(++idx) + "_length_" + std::to_string(p.size()) + "_weigth_" +
                                 std::to_string(pw.second) + "_";
        const std::string flags = "\t*\tZ:W:" + std::to_string(pw.second) + "\n";
        uint64_t seg = 1;
        o += name + "1\t";
        for (size_t i = 0; i < p.size(); ++i) {
            g.orient(p[i], "", o);
            if (i + 1 == p.size()) break;
            if (g.end[p[i]] != g.start(p[i + 1])) o += flags + name + std::to_string(++seg) + "\t";
            else o += ',';
        }
        o += flags;
        if (o.size() > (1u << 24)) {
            put(o);
            o.clear();
        }
    }
    put(o);
    if (fclose(f) != 0 || fail) fatal("writing %s failed", path.c_str());
}

void usage(const char *argv0) {
    printf("SYNOPSIS\n        %s <dataset description (in YAML)> <graph (in GFA)> <output filename> [-k <value>]\n"
           "           [-t <value>] [--tmp-dir <dir>]\n\n"
           "OPTIONS\n"
           "        -k <value>  k-mer length to use\n"
           "        -t <value>  # of threads to use\n"
           "        --tmp-dir <dir>\n                    scratch directory to use\n"
           "        -b <value>  bytes of contig text per mapped block\n"
           "        --device <value>  GPU to use (default 0)\n",
           argv0);
}

}  // namespace

int main(int argc, char **argv) {
    unsigned k = 21, device = 0;
    unsigned long long threads = 0, bufsize = 536870912ull;
    std::vector<std::string> pos;
    Options opt;
    opt.num("-k", "", &k, 0u, 999u).num("-t", "", &threads).num("-b", "", &bufsize, 1ull).num("", "--device", &device)
        .ignored("", "--tmp-dir").positional(&pos);
    if (!opt.parse(argc, argv) || pos.size() != 3) {  // clipp's man page and exit(1) (:77-81)
        usage(argv[0]);
        return 1;
    }
    const std::string dataset = pos[0], graph = pos[1], outfile = pos[2];

    info("Starting SPAdes sequence-to-graph mapper (MI355X, %s)", bbk_version());
    check_graph_k(k);
    require_gfa(graph);
    std::vector<DatasetLib> libs;
    std::string err;
    if (!load_dataset_libs(dataset, libs, err)) fatal("%s", err.c_str());
    // library types (common/pipeline/library.cpp:36-48, library.hpp:205-217)
    auto is_contigs = [](const std::string &t) { return t == "untrusted-contigs" || t == "path-extend-contigs"; };
    for (size_t i = 0; i < libs.size(); ++i) {
        const std::string &t = libs[i].type;
        if (t == "trusted-contigs")
            fatal("library #%zu is trusted-contigs: its path extractor (GappedPathExtractorForTrustedContigs) reads the "
                  "trusted aligner settings of a SPAdes configuration, which spades-gmapper never loads; give the contigs "
                  "as untrusted-contigs or path-extend-contigs",
                  i);
        if (t == "pacbio" || t == "sanger" || t == "nanopore" || t == "tslr" || t == "fl-rna")
            fatal("library #%zu is a long-read library (%s): long-read alignment (PacbioAlignLibrary) is not supported",
                  i, t.c_str());
    }

    Run run;
    Phases &ph = run.ph;
    const int nthreads = threads ? (int)std::min<unsigned long long>(threads, 1024) : default_threads();
    run.create_ctx(device);
    bbk_ctx *ctx = run.ctx;
    info("Loading de Bruijn graph from %s", graph.c_str());
    double t0 = now_s();
    bbk_edgeindex *ix = nullptr;
    check(bbk_edgeindex_from_gfa_with_graph(ctx, graph.c_str(), k, &ix), "bbk_edgeindex_from_gfa_with_graph");
    Graph g;
    const uint64_t loops_differ = build_graph(ix, k, nthreads, g);
    ph.finish = now_s() - t0;
    info("Graph loaded. Segments: %llu, links: %llu, %u-mers indexed", (unsigned long long)g.ns,
         (unsigned long long)bbk_edgeindex_links(ix), k + 1);
    if (loops_differ)
        info("%llu one-(k+1)-mer loop edge(s) linked differently from their L lines: their ranges are cut differently, "
             "the paths are the same", (unsigned long long)loops_differ);

    double t_extract = 0;
    uint64_t n_contigs = 0;
    for (size_t li = 0; li < libs.size(); ++li) {
        if (!is_contigs(libs[li].type)) {
            warn("Could only map contigs or long reads so far, skipping the library");
            continue;
        }
        info("Mapping contigs library #%zu", li);
        std::map<std::vector<Edge>, uint64_t> storage;  // PathStorage: by first edge, then by path; AddPath(path, 1)
        PieceBlock blk;  // the contigs cut at N
        double t_flush = 0;
        auto flush = [&] {
            const double tf = now_s();
            const uint64_t np = blk.pieces(), nc = blk.sequences();
            std::vector<uint64_t> roff(np + 1, 0);
            std::vector<bbk_path_range> ranges;
            if (np > 0) {
                double t1 = now_s();
                bbk_reads *r = nullptr;
                check(bbk_reads_from_ascii(ctx, blk.bases.data(), blk.off.data(), np, &r), "bbk_reads_from_ascii");
                ph.upload += now_s() - t1;
                t1 = now_s();
                bbk_paths *pp = nullptr;
                check(bbk_edgeindex_map_paths(ctx, ix, r, &pp), "bbk_edgeindex_map_paths");
                ranges.resize(bbk_paths_ranges(pp));
                check(bbk_paths_export(ctx, pp, roff.data(), ranges.data()), "bbk_paths_export");
                bbk_paths_free(pp);
                bbk_reads_free(r);
                ph.device += now_s() - t1;
                ++ph.blocks;
            }
            const double t1 = now_s();
            std::vector<std::vector<std::vector<Edge>>> found(nc);
#pragma omp parallel num_threads(nthreads)
            {
                GapCloser gc(g);
                std::vector<std::pair<Edge, uint64_t>> mp;
#pragma omp for schedule(dynamic, 16)
                for (int64_t c = 0; c < (int64_t)nc; ++c) {
                    mp.clear();
                    for (uint64_t q = blk.first_piece[c]; q < blk.first_piece[c + 1]; ++q)
                        for (uint64_t x = roff[q]; x < roff[q + 1]; ++x)
                            mp.emplace_back((Edge)ranges[x].edge, (uint64_t)(ranges[x].init_end - ranges[x].init_start));
                    extract_paths(g, gc, mp, found[c]);
                }
            }
            for (auto &v : found)
                for (auto &p : v) storage[std::move(p)] += 1;
            t_extract += now_s() - t1;
            blk = PieceBlock();
            t_flush += now_s() - tf;
        };
        const double tl = now_s();
        for (const std::string &file : libs[li].v[LIB_SINGLE]) {
            FastxReader rd(file);
            if (!rd.is_open()) fatal("cannot open %s", file.c_str());
            std::string name, seq, qual;
            while (rd.next_record(name, seq, qual)) {  // upper-cased by the reader, as kseq does
                const size_t j = seq.find_first_not_of("ACGTN");
                if (j != std::string::npos)
                    fatal("contig %s of %s holds '%c' at position %llu: only A, C, G, T and N are accepted (the "
                          "reference aborts on it)",
                          name.substr(0, name.find_first_of(" \t")).c_str(), file.c_str(), seq[j], (unsigned long long)j);
                blk.add(seq, [](char c) { return c == 'N'; });
                ++n_contigs;
                if (blk.bases.size() >= bufsize) flush();
            }
        }
        flush();
        ph.parse += now_s() - tl - t_flush;
        info("Saving to %s (%zu distinct paths)", outfile.c_str(), storage.size());
        t0 = now_s();
        write_output(g, storage, outfile, nthreads);
        ph.write += now_s() - t0;
    }
    info("%llu contigs mapped; path extraction %.3f s", (unsigned long long)n_contigs, t_extract);
    bbk_edgeindex_free(ix);
    run.done("spades-gmapper");
}
