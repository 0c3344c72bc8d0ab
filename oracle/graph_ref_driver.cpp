// TEST INFRASTRUCTURE ONLY: our driver over the reference's graph-side classes (GFA reader, edge index, sequence mapper,
// insert-size counter, paired index, distance estimator), linked into oracle/_ref/graph_ref by `make -C oracle ref`
// (oracle/_ref/ is git-ignored).  It runs the read-to-graph stages on one GFA graph and one paired-end library at one
// thread and writes every stage's state as one JSON document.  Every edge is named (S-line name, orientation); the
// reference's integer ids appear only in the id tables that go with the BinWrite bytes.
// oracle/record_graph_ref.py turns the document into the fixtures of tests/golden/graph_ref/.
//
//   graph_ref <graph.gfa> <k> <work dir> <settings> <out.json> [reads <left.fastq> <right.fastq>] [points <file>]
//             [seqs <file>]
//
// settings, one `key value...` per line:
//   orientation ff|fr|rf|rr          edge_length_bound N         insert_size N (absent: (size_t) mean of the is stage)
//   fill <filter threshold> <round_thr>                          (any number of lines; the first one feeds `de`)
//   de <mean> <deviation> <read length> <linkage coeff> <max distance coeff> <clustered threshold>   (any number)
// points: `name o name o distance weight` per line, given to PairedIndex::Add as they stand.
// seqs: one sequence per line, mapped with MapSequence.
//
// What is restated here in our own words, because the reference keeps it in an anonymous namespace or behind its
// dataset loader: the FASTQ parsing, the listener loops of DEFilter and EdgePairCounterFiller, the construction of the
// counting Bloom filter, and the parameter arithmetic of estimate_distance.  The pair is presented with the reference's
// own io::LongestValid and io::OrientationChanger, in the order of its binary read conversion: cut, then turn.
#include "assembly_graph/core/graph.hpp"
#include "io/graph/gfa_reader.hpp"
#include "io/reads/longest_valid_wrapper.hpp"
#include "io/reads/orientation.hpp"
#include "io/reads/paired_read.hpp"
#include "modules/alignment/edge_index.hpp"
#include "modules/alignment/kmer_mapper.hpp"
#include "modules/alignment/sequence_mapper.hpp"
#include "paired_info/distance_estimation.hpp"
#include "paired_info/is_counter.hpp"
#include "paired_info/pair_info_filler.hpp"
#include "paired_info/pair_info_filters.hpp"
#include "paired_info/paired_info_helpers.hpp"
#include "utils/logger/log_writers.hpp"
#include "utils/logger/logger.hpp"

#include "adt/bf.hpp"  // after the graph headers: it relies on their <cstddef>
#include "adt/hll.hpp"

#include "llvm/Support/TimeProfiler.h"

#define XXH_INLINE_ALL
#include "xxh/xxhash.h"

#include <omp.h>

#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

// The headers open time-trace scopes; the profiler itself is not linked and stays off.
namespace llvm {
TimeTraceProfiler *getTimeTraceProfilerInstance() { return nullptr; }
void timeTraceProfilerBegin(StringRef, StringRef) {}
void timeTraceProfilerEnd() {}
}  // namespace llvm

namespace {

using debruijn_graph::EdgeId;
using debruijn_graph::Graph;
using omnigraph::MappingPath;
using omnigraph::MappingRange;
using namespace omnigraph::de;
typedef std::pair<EdgeId, EdgeId> EdgePair;
typedef debruijn_graph::EdgeIndex<Graph> Index;
typedef debruijn_graph::BasicSequenceMapper<Graph, Index> Mapper;

[[noreturn]] void die(const std::string &what) {
  fprintf(stderr, "graph_ref: %s\n", what.c_str());
  exit(2);
}

std::string revcomp(const std::string &s) {
  std::string r(s.rbegin(), s.rend());
  for (char &c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c;
  return r;
}

uint32_t fbits(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return u;
}

uint64_t dbits(double x) {
  uint64_t u;
  memcpy(&u, &x, 8);
  return u;
}

std::string hex(const std::string &bytes) {
  static const char *d = "0123456789abcdef";
  std::string s;
  for (unsigned char c : bytes) {
    s += d[c >> 4];
    s += d[c & 15];
  }
  return s;
}

// ---- edge names: the S line whose text is EdgeNucls(e), or whose reverse complement is ------------------------------
struct Names {
  std::map<std::string, std::string> by_seq;
  std::map<std::string, std::string> by_name;

  void read(const std::string &gfa) {
    std::ifstream is(gfa);
    if (!is) die("cannot read " + gfa);
    std::string line;
    while (std::getline(is, line)) {
      if (line.size() < 2 || line[0] != 'S') continue;
      std::istringstream ss(line);
      std::string tag, name, seq;
      ss >> tag >> name >> seq;
      for (char &c : seq) c = (char)toupper(c);
      if (by_seq.count(seq) || by_seq.count(revcomp(seq))) die("two segments with one sequence: " + name);
      by_seq[seq] = name;
      by_name[name] = seq;
    }
  }
};

struct Namer {
  const Graph &g;
  std::map<EdgeId, std::string> text;  // "name","o"
  std::map<std::string, EdgeId> edge;  // name + o

  Namer(const Graph &graph, const Names &names) : g(graph) {
    for (EdgeId e : g.edges()) {
      std::string s = g.EdgeNucls(e).str();
      auto it = names.by_seq.find(s);
      char o = '+';
      if (it == names.by_seq.end()) {
        it = names.by_seq.find(revcomp(s));
        o = '-';
      }
      if (it == names.by_seq.end()) die("an edge of the graph is no segment of the file");
      text[e] = "\"" + it->second + "\",\"" + o + "\"";
      edge[it->second + o] = e;
    }
  }

  const std::string &operator()(EdgeId e) const { return text.at(e); }

  EdgeId find(const std::string &name, const std::string &o) const {
    auto it = edge.find(name + o);
    if (it == edge.end() && o == "-") it = edge.find(name + "+");  // a self-conjugate segment has one orientation
    if (it == edge.end()) die("no edge " + name + o);
    return it->second;
  }

  std::vector<EdgeId> sorted_edges() const {  // by (name, orientation): an order that owes nothing to the ids
    std::vector<EdgeId> v;
    for (const auto &kv : edge) v.push_back(kv.second);
    return v;
  }
};

struct Settings {
  io::LibraryOrientation orientation = io::LibraryOrientation::FR;
  size_t edge_length_bound = 0;
  long insert_size = -1;
  std::vector<std::pair<unsigned, unsigned>> fills;
  struct De {
    double mean, deviation;
    size_t read_length;
    double linkage_coeff, max_distance_coeff, threshold;
  };
  std::vector<De> de;
};

Settings read_settings(const std::string &path) {
  Settings s;
  std::ifstream is(path);
  if (!is) die("cannot read " + path);
  std::string line;
  while (std::getline(is, line)) {
    std::istringstream ss(line);
    std::string key;
    if (!(ss >> key)) continue;
    if (key == "orientation") {
      std::string o;
      ss >> o;
      s.orientation = o == "ff" ? io::LibraryOrientation::FF : o == "fr" ? io::LibraryOrientation::FR :
                      o == "rf" ? io::LibraryOrientation::RF : o == "rr" ? io::LibraryOrientation::RR :
                      io::LibraryOrientation::Undefined;
      if (s.orientation == io::LibraryOrientation::Undefined) die("orientation " + o);
    } else if (key == "edge_length_bound") {
      ss >> s.edge_length_bound;
    } else if (key == "insert_size") {
      ss >> s.insert_size;
    } else if (key == "fill") {
      unsigned t, r;
      ss >> t >> r;
      s.fills.emplace_back(t, r);
    } else if (key == "de") {
      Settings::De d;
      ss >> d.mean >> d.deviation >> d.read_length >> d.linkage_coeff >> d.max_distance_coeff >> d.threshold;
      s.de.push_back(d);
    } else {
      die("unknown setting " + key);
    }
    if (!ss) die("malformed setting " + key);
  }
  return s;
}

std::vector<io::PairedRead> read_pairs(const std::string &left, const std::string &right) {
  std::ifstream a(left), b(right);
  if (!a || !b) die("cannot read the library");
  std::vector<io::PairedRead> out;
  std::string h1, s1, p1, q1, h2, s2, p2, q2;
  while (std::getline(a, h1) && std::getline(a, s1) && std::getline(a, p1) && std::getline(a, q1)) {
    if (!(std::getline(b, h2) && std::getline(b, s2) && std::getline(b, p2) && std::getline(b, q2)))
      die("the right file is shorter");
    // insert size 0 here; the fill pass sets it per pair, as paired_binary_readers hands it down
    out.emplace_back(io::SingleRead(h1.substr(1), s1, 0, 0, /*validate*/ true),
                     io::SingleRead(h2.substr(1), s2, 0, 0, /*validate*/ true), 0);
  }
  return out;
}

struct Json {
  FILE *f;
  explicit Json(const std::string &path) : f(fopen(path.c_str(), "w")) {
    if (!f) die("cannot write " + path);
  }
  ~Json() { fclose(f); }
};

std::string path_json(const Namer &name, const MappingPath<EdgeId> &p) {
  std::string s = "[";
  for (size_t i = 0; i < p.size(); ++i) {
    MappingRange r = p.mapping_at(i);
    char buf[128];
    snprintf(buf, sizeof(buf), ",%zu,%zu,%zu,%zu]", r.initial_range.start_pos, r.initial_range.end_pos,
             r.mapped_range.start_pos, r.mapped_range.end_pos);
    s += std::string(i ? ",[" : "[") + name(p.edge_at(i)) + buf;
  }
  return s + "]";
}

float var_of(const RawPoint &) { return 0; }
float var_of(const Point &p) { return p.var; }

// every stored histogram of a raw index, walked by (name, orientation); half: GetHalf, else Get
template <class IndexT>
void dump_points(FILE *f, const Namer &name, const IndexT &index, bool half, bool with_var) {
  fprintf(f, "[");
  bool first = true;
  for (EdgeId e1 : name.sorted_edges()) {
    auto proxy = half ? index.GetHalf(e1) : index.Get(e1);
    std::map<std::string, std::string> rows;  // second edge's name -> its points
    for (auto entry : proxy) {
      std::string row;
      for (auto p : entry.second) {
        char buf[96];
        if (with_var)
          snprintf(buf, sizeof(buf), ",%u,%u,%u]", fbits((float)p.d), fbits(var_of(p)), fbits((float)p.weight));
        else
          snprintf(buf, sizeof(buf), ",%u,%u]", fbits((float)p.d), fbits((float)p.weight));
        row += std::string(row.empty() ? "[" : ",[") + name(e1) + "," + name(entry.first) + buf;
      }
      if (!row.empty()) rows[name(entry.first)] = row;
    }
    for (const auto &kv : rows) {
      fprintf(f, "%s%s", first ? "" : ",", kv.second.c_str());
      first = false;
    }
  }
  fprintf(f, "]");
}

template <class IndexT>
void dump_prd(FILE *f, const Namer &name, const Graph &g, const IndexT &index) {
  std::ostringstream os;
  index.BinWrite(os);
  fprintf(f, "\"prd\":\"%s\",\"prd_ids\":{", hex(os.str()).c_str());
  bool first = true;
  for (EdgeId e : name.sorted_edges()) {
    fprintf(f, "%s\"%zu\":[%s]", first ? "" : ",", (size_t)g.int_id(e), name(e).c_str());
    first = false;
  }
  fprintf(f, "}");
}

uint64_t pair_hash_counter(const EdgePair &e) {
  uint64_t h1 = e.first.hash();
  return XXH3_64bits_withSeed(&h1, sizeof(h1), e.second.hash());
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 6) die("usage: graph_ref <graph.gfa> <k> <work dir> <settings> <out.json> [reads L R] [points F] [seqs F]");
  omp_set_num_threads(1);
  srand(42);
  srandom(42);
  logging::logger *lg = logging::create_logger("");
  lg->add_writer(std::make_shared<logging::console_writer>());
  logging::attach_logger(lg);

  const std::string gfa_path = argv[1], workdir = argv[3];
  const unsigned k = (unsigned)atoi(argv[2]);
  const Settings settings = read_settings(argv[4]);
  std::string left, right, points_path, seqs_path;
  for (int i = 6; i < argc;) {
    std::string key = argv[i];
    if (key == "reads" && i + 2 < argc) {
      left = argv[i + 1];
      right = argv[i + 2];
      i += 3;
    } else if (key == "points" && i + 1 < argc) {
      points_path = argv[i + 1];
      i += 2;
    } else if (key == "seqs" && i + 1 < argc) {
      seqs_path = argv[i + 1];
      i += 2;
    } else {
      die("argument " + key);
    }
  }

  Names names;
  names.read(gfa_path);
  Graph g(k);
  {
    gfa::GFAReader reader(gfa_path);
    if (!reader.valid()) die("the reference's reader refuses " + gfa_path);
    reader.to_graph(g);
  }
  const Namer name(g, names);

  Index index(g, workdir);
  index.Refill();  // attaches the index as well
  debruijn_graph::KmerMapper<Graph> kmer_mapper(g);
  Mapper mapper(g, index, kmer_mapper);

  Json out(argv[5]);
  FILE *f = out.f;
  fprintf(f, "{\"k\":%u,\"edges\":[", k);
  {
    bool first = true;
    for (EdgeId e : name.sorted_edges()) {
      fprintf(f, "%s[%s,%zu,%d]", first ? "" : ",", name(e).c_str(), g.length(e), (int)(g.conjugate(e) == e));
      first = false;
    }
  }
  fprintf(f, "]");

  // ---- map: extra sequences -----------------------------------------------------------------------------------------
  if (!seqs_path.empty()) {
    std::ifstream is(seqs_path);
    if (!is) die("cannot read " + seqs_path);
    fprintf(f, ",\"map_seqs\":[");
    std::string s;
    bool first = true;
    while (std::getline(is, s)) {
      if (s.empty()) continue;
      fprintf(f, "%s%s", first ? "" : ",", path_json(name, mapper.MapSequence(Sequence(s))).c_str());
      first = false;
    }
    fprintf(f, "]");
  }

  // what `de` clusters: the index of the first `fill` line as the filler left it, or the points given from outside
  std::vector<std::unique_ptr<UnclusteredPairedInfoIndexT<Graph>>> raws;

  if (!left.empty()) {
    // ---- presentation and map: both mates by the reference's mapper ------------------------------------------------
    std::vector<io::PairedRead> pairs = read_pairs(left, right);
    io::OrientationChanger changer(settings.orientation);
    std::vector<MappingPath<EdgeId>> path1, path2;
    fprintf(f, ",\"map\":[");
    for (size_t i = 0; i < pairs.size(); ++i) {
      io::PairedRead &r = pairs[i];
      // the order of the binary conversion that PairInfoCount reads (paired_binary_readers): the mates are cut in file
      // orientation (read_converter.cpp:76-83: use_orientation = false, handle_Ns = true) and turned when they are
      // written (PairedReadBinaryWriter, binary_converter.cpp:41-46; BinWrite(rc) swaps the offsets as operator! does)
      io::LongestValid(r);
      changer(r);
      path1.push_back(mapper.MapRead(r.first()));
      path2.push_back(mapper.MapRead(r.second()));
      fprintf(f, "%s{\"first\":\"%s\",\"second\":\"%s\",\"offsets\":[%d,%d,%d,%d],\"path1\":%s,\"path2\":%s}", i ? "," : "",
              r.first().GetSequenceString().c_str(), r.second().GetSequenceString().c_str(),
              (int)r.first().GetLeftOffset(), (int)r.first().GetRightOffset(), (int)r.second().GetLeftOffset(),
              (int)r.second().GetRightOffset(), path_json(name, path1[i]).c_str(), path_json(name, path2[i]).c_str());
    }
    fprintf(f, "]");

    // ---- is ------------------------------------------------------------------------------------------------------
    debruijn_graph::InsertSizeCounter counter(g, settings.edge_length_bound);
    counter.StartProcessLibrary(1);
    for (size_t i = 0; i < pairs.size(); ++i) counter.ProcessPairedRead(0, pairs[i], path1[i], path2[i]);
    counter.MergeBuffer(0);
    counter.StopProcessLibrary();
    double mean = 0, deviation = 0, median = 0, mad = 0;
    {
      fprintf(f, ",\"is\":{\"total\":%zu,\"mapped\":%zu,\"negative\":%zu,\"hist\":[", counter.total(), counter.mapped(),
              counter.negative());
      bool first = true;
      for (const auto &kv : counter.hist()) {
        fprintf(f, "%s[%d,%zu]", first ? "" : ",", kv.first, kv.second);
        first = false;
      }
      fprintf(f, "]");
      if (counter.mapped() > 0) {
        std::map<size_t, size_t> percentiles;
        omnigraph::HistType distribution;
        counter.FindMean(mean, deviation, percentiles);
        counter.FindMedian(median, mad, distribution);
        fprintf(f, ",\"mean\":\"%016" PRIx64 "\",\"deviation\":\"%016" PRIx64 "\",\"median\":\"%016" PRIx64
                   "\",\"mad\":\"%016" PRIx64 "\",\"percentiles\":[",
                dbits(mean), dbits(deviation), dbits(median), dbits(mad));
        first = true;
        for (const auto &kv : percentiles) {
          fprintf(f, "%s[%zu,%zu]", first ? "" : ",", kv.first, kv.second);
          first = false;
        }
        fprintf(f, "],\"distribution\":[");
        first = true;
        for (const auto &kv : distribution) {
          fprintf(f, "%s[%d,%zu]", first ? "" : ",", kv.first, kv.second);
          first = false;
        }
        fprintf(f, "]");
        if (!distribution.empty()) {
          auto interval = omnigraph::GetISInterval(0.8, distribution);
          fprintf(f, ",\"interval\":[\"%016" PRIx64 "\",\"%016" PRIx64 "\"]", dbits(interval.first), dbits(interval.second));
        }
      }
      fprintf(f, "}");
    }

    // ---- pairs: exact counts next to the reference's cardinality estimate and its counting Bloom filter ------------
    std::map<std::pair<std::string, std::string>, std::pair<EdgePair, size_t>> occ;
    hll::hll_with_hasher<EdgePair> cardinality_counter(pair_hash_counter);
    for (size_t i = 0; i < pairs.size(); ++i)
      for (size_t a = 0; a < path1[i].size(); ++a)
        for (size_t b = 0; b < path2[i].size(); ++b) {
          EdgePair ep(path1[i].edge_at(a), path2[i].edge_at(b));
          cardinality_counter.add(ep);
          auto &slot = occ[{name(ep.first), name(ep.second)}];
          slot.first = ep;
          ++slot.second;
        }
    const size_t edgepairs = size_t(cardinality_counter.cardinality());
    typedef bf::counting_bloom_filter<EdgePair, 2> PairedInfoFilter;
    PairedInfoFilter filter(
        [](const EdgePair &e, uint64_t seed) {
          uint64_t h1 = e.first.hash();
          return XXH3_64bits_withSeed(&h1, sizeof(h1), (e.second.hash() * seed) ^ seed);
        },
        12 * edgepairs);
    for (size_t i = 0; i < pairs.size(); ++i)
      for (size_t a = 0; a < path1[i].size(); ++a)
        for (size_t b = 0; b < path2[i].size(); ++b) {
          EdgeId e1 = path1[i].edge_at(a), e2 = path2[i].edge_at(b);
          filter.add({e1, e2});
          filter.add({g.conjugate(e2), g.conjugate(e1)});
        }
    fprintf(f, ",\"pairs\":{\"cardinality\":%zu,\"exact\":%zu,\"cells\":%zu,\"counts\":[", edgepairs, occ.size(),
            12 * edgepairs);
    {
      bool first = true;
      for (const auto &kv : occ) {
        const EdgePair &ep = kv.second.first;
        EdgePair cj(g.conjugate(ep.second), g.conjugate(ep.first));
        auto it = occ.find({name(cj.first), name(cj.second)});
        size_t conj_count = it == occ.end() ? 0 : it->second.second;
        fprintf(f, "%s[%s,%s,%zu,%zu,%zu]", first ? "" : ",", kv.first.first.c_str(), kv.first.second.c_str(),
                kv.second.second, conj_count, filter.lookup(ep));
        first = false;
      }
    }
    fprintf(f, "]}");

    // ---- raw: LatePairedIndexFiller over all pairs, per (filter threshold, round_thr) -----------------------------
    const size_t insert_size = settings.insert_size >= 0 ? (size_t)settings.insert_size : (size_t)mean;
    for (auto &r : pairs) r.set_orig_insert_size(insert_size);
    fprintf(f, ",\"raw\":[");
    for (size_t n = 0; n < settings.fills.size(); ++n) {
      const unsigned threshold = settings.fills[n].first, round_thr = settings.fills[n].second;
      debruijn_graph::LatePairedIndexFiller::WeightF weight;
      if (threshold)
        weight = [&](const EdgePair &ep, const MappingRange &, const MappingRange &) {
          return filter.lookup(ep) > threshold ? 1. : 0.;
        };
      else
        weight = [&](const EdgePair &, const MappingRange &, const MappingRange &) { return 1.; };
      raws.emplace_back(new UnclusteredPairedInfoIndexT<Graph>(g));
      UnclusteredPairedInfoIndexT<Graph> &raw = *raws.back();
      debruijn_graph::LatePairedIndexFiller filler(g, weight, round_thr, raw);
      filler.StartProcessLibrary(1);
      for (size_t i = 0; i < pairs.size(); ++i) filler.ProcessPairedRead(0, pairs[i], path1[i], path2[i]);
      filler.StopProcessLibrary();
      fprintf(f, "%s{\"threshold\":%u,\"round\":%u,\"insert_size\":%zu,\"size\":%zu,\"half\":", n ? "," : "", threshold,
              round_thr, insert_size, raw.size());
      dump_points(f, name, raw, true, false);
      fprintf(f, ",\"full\":");
      dump_points(f, name, raw, false, false);
      fprintf(f, ",");
      dump_prd(f, name, g, raw);
      fprintf(f, "}");
    }
    fprintf(f, "]");
  }

  // ---- raw points given from outside ------------------------------------------------------------------------------
  if (!points_path.empty()) {
    std::ifstream is(points_path);
    if (!is) die("cannot read " + points_path);
    if (!raws.empty()) die("points and reads exclude each other");
    raws.emplace_back(new UnclusteredPairedInfoIndexT<Graph>(g));
    UnclusteredPairedInfoIndexT<Graph> &first_raw = *raws.back();
    std::string n1, o1, n2, o2;
    double d, w;
    while (is >> n1 >> o1 >> n2 >> o2 >> d >> w)
      first_raw.Add(name.find(n1, o1), name.find(n2, o2), RawPoint((DEDistance)d, (DEWeight)w));
    fprintf(f, ",\"points\":{\"size\":%zu,\"half\":", first_raw.size());
    dump_points(f, name, first_raw, true, false);
    fprintf(f, ",\"full\":");
    dump_points(f, name, first_raw, false, false);
    fprintf(f, ",");
    dump_prd(f, name, g, first_raw);
    fprintf(f, "}");
  }

  // ---- lengths and clustered, per `de` line: the calls of estimate_distance up to the weight filter ----------------
  if (raws.empty()) raws.emplace_back(new UnclusteredPairedInfoIndexT<Graph>(g));
  const UnclusteredPairedInfoIndexT<Graph> &first_raw = *raws.front();
  fprintf(f, ",\"de\":[");
  for (size_t n = 0; n < settings.de.size(); ++n) {
    const Settings::De &s = settings.de[n];
    size_t delta = size_t(s.deviation);
    size_t linkage_distance = size_t(s.linkage_coeff * s.deviation);
    size_t insert = (size_t)math::round(s.mean);
    size_t max_distance = size_t(s.max_distance_coeff * s.deviation);
    GraphDistanceFinder finder(g, insert, s.read_length, delta);
    fprintf(f, "%s{\"insert_size\":%zu,\"read_length\":%zu,\"delta\":%zu,\"linkage_distance\":%zu,\"max_distance\":%zu,"
               "\"threshold\":\"%016" PRIx64 "\",\"lengths\":[",
            n ? "," : "", insert, s.read_length, delta, linkage_distance, max_distance, dbits(s.threshold));
    bool first = true;
    for (EdgeId e1 : name.sorted_edges()) {
      std::map<std::string, std::string> rows;
      for (auto entry : first_raw.GetHalf(e1)) {
        std::string row = "[" + name(e1) + "," + name(entry.first) + ",[";
        bool head = true;
        for (size_t len : finder.GetGraphDistancesLengths(e1, entry.first)) {
          row += (head ? "" : ",") + std::to_string(len);
          head = false;
        }
        rows[name(entry.first)] = row + "]]";
      }
      for (const auto &kv : rows) {
        fprintf(f, "%s%s", first ? "" : ",", kv.second.c_str());
        first = false;
      }
    }
    fprintf(f, "]");

    PairedInfoIndexT<Graph> clustered(g);
    DistanceEstimator estimator(g, first_raw, finder, linkage_distance, max_distance);
    estimator.Estimate(clustered, 1);
    fprintf(f, ",\"size_before\":%zu,\"unfiltered\":", clustered.size());
    dump_points(f, name, clustered, false, true);
    PairInfoWeightChecker<Graph> checker(g, s.threshold);
    PairInfoFilter<Graph>(checker).Filter(clustered);
    fprintf(f, ",\"size_after\":%zu,\"clustered\":", clustered.size());
    dump_points(f, name, clustered, false, true);
    fprintf(f, ",\"clustered_half\":");
    dump_points(f, name, clustered, true, true);
    // the condition RefinePairedInfo looks for (it holds the first cluster of a pair against every later one): here any
    // two clusters of a pair no further apart than their spans
    bool intersect = false;
    for (auto it = pair_begin(clustered); it != pair_end(clustered); ++it) {
      auto infos = it->Unwrap();
      for (auto a = infos.begin(); a != infos.end(); ++a) {
        auto b = a;
        for (++b; b != infos.end(); ++b)
          if (math::le(std::abs(b->d - a->d), b->var + a->var)) intersect = true;
      }
    }
    fprintf(f, ",\"refine_condition\":%s,", intersect ? "true" : "false");
    dump_prd(f, name, g, clustered);
    fprintf(f, "}");
  }
  fprintf(f, "]}\n");
  return 0;
}
