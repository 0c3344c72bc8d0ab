// TEST INFRASTRUCTURE ONLY: our driver over the reference's BayesHammer classes, linked into oracle/_ref/hammer_ref by
// `make -C oracle ref` (oracle/_ref/ is git-ignored).  It runs the stages in the order of the reference's main.cpp on
// one paired FASTQ library, at one thread, and after every stage writes that stage's state as plain data keyed by
// k-mer string -- never by the index of the minimal perfect hash.  oracle/record_hammer_ref.py turns the dump into the
// fixtures of tests/golden/hammer_ref/.
//
//   hammer_ref <config.info> <left.fastq> <right.fastq> <work dir> <output dir> <dump dir>
//
// The dataset is built in code (SequencingLibrary::push_back_paired); the YAML loader of the reference is not linked,
// so the file list that corrected.yaml would hold is dumped from the output dataset itself (stage5_files.tsv).
#include "config_struct_hammer.hpp"
#include "expander.hpp"
#include "globals.hpp"
#include "hammer_tools.hpp"
#include "kmer_cluster.hpp"
#include "kmer_data.hpp"
#include "valid_kmer_generator.hpp"

#include "adt/concurrent_dsu.hpp"
#include "io/reads/ireadstream.hpp"
#include "io/reads/read_processor.hpp"
#include "utils/logger/logger.hpp"
#include "utils/memory_limit.hpp"

#include "llvm/Support/TimeProfiler.h"

#include <omp.h>

#include <algorithm>
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

std::vector<uint32_t> *Globals::subKMerPositions = NULL;
KMerData *Globals::kmer_data = NULL;
int Globals::iteration_no = 0;
char Globals::char_offset = 0;
bool Globals::char_offset_user = true;
double Globals::quality_probs[256] = {0};
double Globals::quality_lprobs[256] = {0};
double Globals::quality_rprobs[256] = {0};
double Globals::quality_lrprobs[256] = {0};

// The k-mer counting headers open time-trace scopes; the profiler itself is not linked and stays off.
namespace llvm {
TimeTraceProfiler *getTimeTraceProfilerInstance() { return nullptr; }
void timeTraceProfilerBegin(StringRef, StringRef) {}
void timeTraceProfilerEnd() {}
}  // namespace llvm

namespace {

struct LineWriter : public logging::writer {
  void write_msg(double, size_t, size_t, logging::level, const char *, size_t, const char *source,
                 const char *msg) override {
    printf("%s: %s\n", source, msg);
  }
};

struct InfoFile {
  std::map<std::string, std::string> kv;
  std::string left, right, work, out;

  const std::string &str(const char *key) const {
    auto it = kv.find(key);
    if (it == kv.end()) {
      fprintf(stderr, "hammer_ref: config.info has no %s\n", key);
      exit(2);
    }
    return it->second;
  }
  long num(const char *key) const { return strtol(str(key).c_str(), NULL, 10); }
  double real(const char *key) const { return strtod(str(key).c_str(), NULL); }
};

// key, whitespace, value; ';' starts a comment; a key without a value has the empty string
InfoFile read_info(const char *path) {
  InfoFile f;
  std::ifstream is(path);
  if (!is) {
    fprintf(stderr, "hammer_ref: cannot read %s\n", path);
    exit(2);
  }
  std::string line;
  while (std::getline(is, line)) {
    size_t semi = line.find(';');
    if (semi != std::string::npos) line.erase(semi);
    std::istringstream ss(line);
    std::string key, value;
    if (!(ss >> key)) continue;
    ss >> value;
    f.kv[key] = value;
  }
  return f;
}

std::string join(const std::vector<std::string> &v, char sep) {
  std::string s;
  for (size_t i = 0; i < v.size(); ++i) {
    if (i) s += sep;
    s += v[i];
  }
  return s.empty() ? "-" : s;
}

std::string real_text(double x) {
  char buf[64];
  snprintf(buf, sizeof(buf), "%.17g", x);
  return buf;
}

FILE *open_dump(const std::string &dir, const char *name) {
  std::string path = dir + "/" + name;
  FILE *f = fopen(path.c_str(), "w");
  if (!f) {
    fprintf(stderr, "hammer_ref: cannot write %s\n", path.c_str());
    exit(2);
  }
  return f;
}

// ---- stage 0: trimming, the valid-k-mer generator, Read::print -------------------------------------------------------
void generator_columns(const Read &r, uint8_t threshold, std::string &starts, std::string &probs) {
  std::vector<std::string> s, p;
  for (ValidKMerGenerator<hammer::K> gen(r, threshold); gen.HasMore(); gen.Next()) {
    s.push_back(std::to_string(gen.pos() - 1));
    p.push_back(real_text(gen.correct_probability()));
  }
  starts = join(s, ',');
  probs = join(p, ',');
}

void dump_stage0(const std::string &dump, const std::string files[2], int offset, int trim_quality) {
  FILE *f = open_dump(dump, "stage0.tsv");
  fprintf(f, "#file\tname\tltrim\trtrim\tinitial_size\tsize\tstarts_q2\tprobs_q2\tstarts_q4\tprobs_q4\n");
  for (int side = 0; side < 2; ++side) {
    std::ofstream printed(dump + "/stage0_print_" + std::to_string(side + 1) + ".fastq");
    // the reference's own reader, so that the dump holds what its stages are given: the whole header line as the name,
    // the sequence in upper case
    ireadstream irs(files[side], offset);
    while (!irs.eof()) {
      Read r;
      irs >> r;
      const std::string name = r.getName();
      size_t sz = r.trimNsAndBadQuality(trim_quality);
      std::string s2, p2, s4, p4;
      generator_columns(r, 2, s2, p2);
      generator_columns(r, 4, s4, p4);
      fprintf(f, "%d\t%s\t%d\t%d\t%d\t%zu\t%s\t%s\t%s\t%s\n", side, name.c_str(), r.ltrim(), r.rtrim(),
              r.initial_size(), sz, s2.c_str(), p2.c_str(), s4.c_str(), p4.c_str());
      r.print(printed, offset);
    }
  }
  fclose(f);
}

// ---- the k-mers in one order that does not depend on the hash: ascending by string, new k-mers after them ------------
struct Order {
  std::vector<size_t> idx;  // position -> index of the reference
  size_t from_reads;
};

Order order_of(const KMerData &data, size_t from_reads) {
  Order o;
  o.from_reads = from_reads;
  for (size_t i = 0; i < data.size(); ++i) o.idx.push_back(i);
  std::vector<std::string> text(data.size());
  for (size_t i = 0; i < data.size(); ++i) text[i] = data.kmer(i).str();
  std::sort(o.idx.begin(), o.idx.begin() + from_reads, [&](size_t a, size_t b) { return text[a] < text[b]; });
  return o;
}

void dump_stage1(const std::string &dump, const KMerData &data, const Order &o) {
  FILE *f = open_dump(dump, "stage1.tsv");
  fprintf(f, "#kmer\tcount\ttotal_qual\ttotal_qual_bits\tqual_word0\tqual_word1\n");
  for (size_t i : o.idx) {
    const KMerStat &st = data[i];
    uint32_t bits;
    memcpy(&bits, &st.total_qual, sizeof(bits));
    static_assert(sizeof(QualBitSet) == 16, "two quality words at K = 21");
    fprintf(f, "%s\t%u\t%.9g\t%08x\t%016" PRIx64 "\t%016" PRIx64 "\n", data.kmer(i).str().c_str(), st.count(),
            (double)st.total_qual, bits, st.qual.data()[0], st.qual.data()[1]);
  }
  fclose(f);
}

class CountGreater {
  const KMerData &data_;

 public:
  explicit CountGreater(const KMerData &data) : data_(data) {}
  bool operator()(size_t a, size_t b) { return data_[a].count() > data_[b].count(); }
};

// The cluster file as the subclustering is about to read it: every cluster in the member order that a count-descending
// std::sort of the file's order gives, which is the order the reference's subclustering sees.  Clusters are written by
// their smallest member.
void dump_stage2(const std::string &dump, const KMerData &data, const std::string &prefix) {
  std::ifstream sizes(prefix + ".idx", std::ios::binary), members(prefix, std::ios::binary);
  std::vector<std::pair<std::string, std::string>> lines;
  size_t n;
  while (sizes.read((char *)&n, sizeof(n))) {
    std::vector<size_t> cluster(n);
    members.read((char *)cluster.data(), n * sizeof(size_t));
    std::sort(cluster.begin(), cluster.end(), CountGreater(data));
    std::vector<std::string> text;
    for (size_t i : cluster) text.push_back(data.kmer(i).str());
    lines.emplace_back(*std::min_element(text.begin(), text.end()), join(text, ' '));
  }
  std::sort(lines.begin(), lines.end());
  FILE *f = open_dump(dump, "stage2.tsv");
  for (const auto &l : lines) fprintf(f, "%s\n", l.second.c_str());
  fclose(f);
}

std::string good_bits(const KMerData &data, const Order &o) {
  std::string s;
  for (size_t i : o.idx) s += data[i].good() ? '1' : '0';
  return s;
}

void dump_stage3(const std::string &dump, const KMerData &data, const Order &o) {
  FILE *f = open_dump(dump, "stage3.tsv");
  fprintf(f, "#kmer\tgood\tcount\tnew\n");
  for (size_t p = 0; p < o.idx.size(); ++p) {
    size_t i = o.idx[p];
    fprintf(f, "%s\t%d\t%u\t%d\n", data.kmer(i).str().c_str(), (int)data[i].good(), data[i].count(),
            (int)(i >= o.from_reads));
  }
  fclose(f);
}

size_t expander_pass(const io::DataSet<> &dataset, int offset) {
  Expander expander(*Globals::kmer_data);
  for (auto I = dataset.reads_begin(), E = dataset.reads_end(); I != E; ++I) {
    ireadstream irs(*I, offset);
    hammer::ReadProcessor rp(1);
    rp.Run(irs, expander);
  }
  return expander.changed();
}

std::string file_name(const std::string &path) {
  size_t slash = path.find_last_of('/');
  return slash == std::string::npos ? path : path.substr(slash + 1);
}

}  // namespace

// config_singl.hpp: create_instance(source) calls load(config, source); this is the overload for our source.
void load(hammer_config &c, const InfoFile &f) {
  io::DataSet<>::Library lib;
  lib.push_back_paired(f.left, f.right);
  c.dataset.push_back(lib);

  c.input_working_dir = f.work;
  c.output_dir = f.out;
  c.input_trim_quality = (int)f.num("input_trim_quality");
  if (!f.str("input_qvoffset").empty()) c.input_qvoffset_opt = (int)f.num("input_qvoffset");

  c.general_do_everything_after_first_iteration = f.num("general_do_everything_after_first_iteration");
  c.general_hard_memory_limit = (int)f.num("general_hard_memory_limit");
  c.general_tau = 1;
  c.general_max_iterations = 1;
  c.general_debug = false;

  c.count_do = f.num("count_do");
  c.count_numfiles = (unsigned)f.num("count_numfiles");
  c.count_split_buffer = (size_t)f.num("count_split_buffer");
  c.count_filter_singletons = false;  // the reference's quotient filter is approximate by design

  c.hamming_do = f.num("hamming_do");
  c.hamming_blocksize_quadratic_threshold = (unsigned)f.num("hamming_blocksize_quadratic_threshold");

  c.bayes_do = f.num("bayes_do");
  c.bayes_singleton_threshold = f.real("bayes_singleton_threshold");
  c.bayes_nonsingleton_threshold = f.real("bayes_nonsingleton_threshold");
  c.bayes_use_hamming_dist = f.num("bayes_use_hamming_dist");
  c.bayes_discard_only_singletons = f.num("bayes_discard_only_singletons");
  c.bayes_debug_output = (unsigned)f.num("bayes_debug_output");
  c.bayes_hammer_mode = f.num("bayes_hammer_mode");
  c.bayes_write_solid_kmers = f.num("bayes_write_solid_kmers");
  c.bayes_write_bad_kmers = f.num("bayes_write_bad_kmers");
  c.bayes_initial_refine = f.num("bayes_initial_refine");

  c.expand_do = f.num("expand_do");
  c.expand_max_iterations = (unsigned)f.num("expand_max_iterations");
  c.expand_write_each_iteration = false;
  c.expand_write_kmers_result = false;

  c.correct_do = f.num("correct_do");
  c.correct_discard_bad = f.num("correct_discard_bad");
  c.correct_use_threshold = f.num("correct_use_threshold");
  c.correct_threshold = f.real("correct_threshold");
  c.correct_readbuffer = (unsigned)f.num("correct_readbuffer");
  c.correct_stats = f.num("correct_stats");

  c.general_max_nthreads = c.count_merge_nthreads = c.bayes_nthreads = c.expand_nthreads = c.correct_nthreads = 1;
}

int main(int argc, char **argv) {
  if (argc != 7) {
    fprintf(stderr, "usage: hammer_ref <config.info> <left.fastq> <right.fastq> <work dir> <output dir> <dump dir>\n");
    return 2;
  }
  srand(42);
  srandom(42);
  omp_set_num_threads(1);

  logging::logger *lg = logging::create_logger("");
  lg->add_writer(std::make_shared<LineWriter>());
  logging::attach_logger(lg);

  InfoFile info = read_info(argv[1]);
  info.left = argv[2];
  info.right = argv[3];
  info.work = argv[4];
  info.out = argv[5];
  const std::string dump = argv[6];
  const std::string files[2] = {info.left, info.right};

  cfg::create_instance(info);
  const size_t GB = 1 << 30;
  utils::limit_memory(cfg::get().general_hard_memory_limit * GB);

  if (!cfg::get().input_qvoffset_opt) {
    int determined = determine_offset(info.left);
    if (determined < 0) {
      fprintf(stderr, "hammer_ref: cannot determine the quality offset\n");
      return 2;
    }
    cfg::get_writable().input_qvoffset = determined;
    Globals::char_offset_user = false;
  } else {
    cfg::get_writable().input_qvoffset = *cfg::get().input_qvoffset_opt;
  }
  const int offset = cfg::get().input_qvoffset;
  Globals::char_offset = (char)offset;

  for (unsigned qual = 0; qual < 256; ++qual) {
    Globals::quality_rprobs[qual] = (qual < 3 ? 0.75 : pow(10.0, -(int)qual / 10.0));
    Globals::quality_probs[qual] = 1 - Globals::quality_rprobs[qual];
    Globals::quality_lprobs[qual] = log(Globals::quality_probs[qual]);
    Globals::quality_lrprobs[qual] = log(Globals::quality_rprobs[qual]);
  }
  hammer::InitializeSubKMerPositions(cfg::get().general_tau);

  dump_stage0(dump, files, offset, cfg::get().input_trim_quality);

  Globals::iteration_no = 0;
  Globals::kmer_data = new KMerData;
  KMerData &data = *Globals::kmer_data;
  const io::DataSet<> input = cfg::get().dataset;

  KMerDataCounter(cfg::get().count_numfiles).BuildKMerIndex(data);
  const size_t from_reads = data.size();

  const std::string hamming = hammer::getFilename(cfg::get().input_working_dir, Globals::iteration_no, "kmers.hamming");
  {
    dsu::ConcurrentDSU uf(data.size());
    TauOneKMerHamClusterer().cluster(
        hammer::getFilename(cfg::get().input_working_dir, Globals::iteration_no, "kmers.hamcls"), data, uf);
    uf.extract_to_file(hamming);
  }

  KMerDataCounter(cfg::get().count_numfiles).FillKMerData(data);
  Order order = order_of(data, from_reads);
  dump_stage1(dump, data, order);
  dump_stage2(dump, data, hamming);

  {
    KMerClustering kmc(data, 1, cfg::get().input_working_dir, false);
    kmc.process(hamming);
  }
  order = order_of(data, from_reads);
  dump_stage3(dump, data, order);

  {
    FILE *f = open_dump(dump, "stage4.tsv");
    fprintf(f, "#round\tadded\tgood bits in the order of stage3.tsv\n");
    for (unsigned round = 0; round < cfg::get().expand_max_iterations; ++round) {
      size_t changed = expander_pass(input, offset);
      fprintf(f, "%u\t%zu\t%s\n", round, changed, good_bits(data, order).c_str());
      if (changed < 10) break;
    }
    fclose(f);
  }

  size_t changed_reads = hammer::CorrectAllReads();
  {
    FILE *f = open_dump(dump, "stage5_files.tsv");
    for (const auto &lib : cfg::get().dataset.libraries()) {
      for (auto I = lib.paired_begin(), E = lib.paired_end(); I != E; ++I) {
        fprintf(f, "left\t%s\n", file_name(I->first).c_str());
        fprintf(f, "right\t%s\n", file_name(I->second).c_str());
      }
      for (auto I = lib.single_begin(), E = lib.single_end(); I != E; ++I)
        fprintf(f, "single\t%s\n", file_name(*I).c_str());
    }
    fprintf(f, "changed_reads\t%zu\n", changed_reads);
    fclose(f);
  }

  {
    // one more pass than the reference runs: 0 added means its in-place result is the closure
    FILE *f = open_dump(dump, "stage4_extra.tsv");
    fprintf(f, "added\t%zu\n", expander_pass(input, offset));
    fclose(f);
  }

  delete Globals::kmer_data;
  return 0;
}
