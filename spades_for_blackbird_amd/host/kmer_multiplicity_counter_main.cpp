// kmer_multiplicity_counter drop-in: the option letters and defaults of the reference tool
// (projects/mts/kmer_multiplicity_counter.cpp:210-241)
//   -k <int> -n <samples> -s <min samples> [-m <min multiplicity of single-sample k-mers = 5>] -o <output prefix>
//   [-t <threads>] -f <files dir>      (+ --ci <int=2>, --cs <int=255>, -b <bytes>, --device <int>, ours)
// and its flow (:188-193): the join of the samples' k-mer counts into <prefix>.bpr.  Where the reference expects one KMC
// database per sample (<dir>/sampleI.kmc_pre / .kmc_suf, I = 1..n), this tool takes the reads themselves: exactly one of
// <dir>/sampleI.{fastq,fq,fasta,fa}[.gz], streamed block by block (-b bytes of input text per block, -t parser threads)
// through the canonical counter; --ci / --cs are the two KMC options that shape the counts of such a database (its
// defaults).  Every read contributes its LongestValid stretch, as in every tool of this engine; KMC counts every N-free
// stretch.  <prefix>.kmers (the kept k-mers, ascending) stands in for the reference's <prefix>.kmm.
#include <sys/stat.h>

#include <string>
#include <vector>

#include "common.hpp"

using namespace bbkhost;

static void usage() {
    printf("Usage: kmer_multiplicity_counter [options] -f files_dir\n"
           "Options:\n"
           "-k - kmer length\n"
           "-n - sample count\n"
           "-o - output file prefix\n"
           "-t - number of threads (default: 1)\n"
           "-s - minimal number of samples to contain kmer\n"
           "-m - minimal multiplicity of single-sample kmers\n"
           "--ci - a k-mer counted fewer times in a sample is absent from it (default: 2)\n"
           "--cs - counts are saturated at this value, at most 65535 (default: 255)\n"
           "-b - bytes of input per streamed block\n"
           "--device - GPU to use (default: 0)\n"
           "files_dir must contain the reads of each sample from 1 to n: exactly one of\n"
           "sampleI.fastq, .fq, .fasta, .fa (or the same with .gz)\n");
}

static bool exists(const std::string &p) {
    struct stat st;
    return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode);
}

int main(int argc, char **argv) {
    unsigned long long k = 0, n = 0, s = 0, m = 5, threads = 1, ci = 2, cs = 255, bufsize = 536870912ull;
    unsigned device = 0;
    std::string out, dir;
    Options opt;
    opt.num("-k", "", &k).num("-n", "", &n).num("-s", "", &s).num("-m", "--min-mult", &m).num("-t", "--threads", &threads)
        .num("", "--ci", &ci).num("", "--cs", &cs).num("-b", "", &bufsize, 1ull).num("", "--device", &device).str("-o", "", &out)
        .str("-f", "", &dir);
    if (!opt.parse(argc, argv) || !opt.seen("-k") || !opt.seen("-n") || !opt.seen("-s") || out.empty() || dir.empty()) {
        usage();  // GetOptEx (:228-231)
        return 1;
    }
    info("Starting k-mer multiplicity counter (MI355X, %s)", bbk_version());
    if (k < 1 || k >= BBK_MAX_K) fatal("k-mer size %llu is out of range [1,%d)", k, BBK_MAX_K);
    if (n < 1 || n > 65535) fatal("sample count %llu is out of range [1,65535]", n);
    if (ci < 1) fatal("--ci must be at least 1");
    if (cs < 1 || cs > 65535) fatal("--cs %llu does not fit the 16-bit multiplicities of the profile (1..65535)", cs);

    static const char *kExt[] = {".fastq", ".fq", ".fasta", ".fa", ".fastq.gz", ".fq.gz", ".fasta.gz", ".fa.gz"};
    std::vector<std::string> files;
    for (unsigned long long i = 1; i <= n; ++i) {
        std::vector<std::string> found;
        for (const char *e : kExt) {
            const std::string p = dir + "/sample" + std::to_string(i) + e;
            if (exists(p)) found.push_back(p);
        }
        if (found.empty())
            fatal("sample %llu: none of %s/sample%llu.{fastq,fq,fasta,fa}[.gz] exists", i, dir.c_str(), i);
        if (found.size() > 1)
            fatal("sample %llu: several read files (%s, %s, ...): exactly one is expected", i, found[0].c_str(),
                  found[1].c_str());
        files.push_back(found[0]);
    }

    Run run;
    Phases &ph = run.ph;
    run.create_ctx(device);
    bbk_ctx *ctx = run.ctx;
    bbk_kmerprofile_builder *b = nullptr;
    check(bbk_kmerprofile_begin(ctx, (unsigned)k, (unsigned)n, (unsigned)ci, (unsigned)cs, &b), "bbk_kmerprofile_begin");
    const int nthreads = (int)std::min<unsigned long long>(std::max<unsigned long long>(threads, 1), 1024);
    for (unsigned i = 0; i < (unsigned)n; ++i) {
        Phases one;  // of this sample: stream_reads sets some fields, the samples add up
        bbk_kmerset *set = count_files(ctx, one, {files[i]}, (unsigned)k, BBK_CANONICAL | BBK_WITH_COUNTS, (size_t)bufsize, nthreads);
        ph.parse += one.parse;
        ph.parse_wait += one.parse_wait;
        ph.upload += one.upload;
        ph.device += one.device + one.finish;
        ph.blocks += one.blocks;
        ph.fallback_blocks += one.fallback_blocks;
        const double t0 = now_s();
        info("Sample %u: %llu distinct canonical %llu-mers", i + 1, (unsigned long long)bbk_kmerset_size(set), k);
        check(bbk_kmerprofile_add_sample(b, i, set), "bbk_kmerprofile_add_sample");
        bbk_kmerset_free(set);
        ph.device += now_s() - t0;
    }
    double t0 = now_s();
    bbk_kmerprofile *p = nullptr;
    check(bbk_kmerprofile_finish(b, s, m, &p), "bbk_kmerprofile_finish");
    ph.finish = now_s() - t0;
    info("Kept %llu k-mers", (unsigned long long)bbk_kmerprofile_size(p));
    t0 = now_s();
    check(bbk_kmerprofile_write(ctx, p, out.c_str()), "bbk_kmerprofile_write");
    ph.write = now_s() - t0;
    info("Saved kmer profiles to %s.bpr, k-mers to %s.kmers", out.c_str(), out.c_str());
    bbk_kmerprofile_free(p);
    run.done("kmer_multiplicity_counter");
}
