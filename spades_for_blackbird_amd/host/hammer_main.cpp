// spades-hammer: BayesHammer as the SPAdes pipeline calls it -- `spades-hammer <config.info>`
// (spades_pipeline/stages/error_correction_stage.py:78-97), which then reads <output_dir>/corrected.yaml -- on the MI355X
// engine behind the C ABI (include/bbk.h).  The sequence is projects/hammer/main.cpp:64-262:
//   the configuration (hammer_config.hpp: the keys of config_struct_hammer.cpp:29-83), the dataset it names
//   the PHRED offset, determined from the first read file when input_qvoffset is absent (fastx.hpp: determine_offset)
//   general_max_iterations iterations of hammer_run.hpp's run_hammer_iteration at K = 21 -- count (filtered with
//   count_filter_singletons 1), cluster, statistics, subcluster, expand, correct -- each writing
//   <output_dir>/<basename>.<ii>.<ilib>_<iread>.cor.fastq, <basename>.<ii>.bad.fastq and the unpaired file of every pair
//   (CorrectAllReads, hammer_tools.cpp:206-272); the corrected libraries are the input of the next iteration (pairs stay
//   pairs, the unpaired file joins the library's single reads, merged stays merged), and an iteration that changed no read
//   is the last (main.cpp:247-250)
//   <output_dir>/corrected.yaml: the libraries of the last iteration that ran
// With general_debug 1 the intermediate files of spades-kmerdata (.kmers, .kmstat, .hamming*, .subclusters*, .newkmers) are
// written under the prefix <input_working_dir>/<ii>; none otherwise.
// Without an argument the configuration is config.info in the current directory.  (The reference's default,
// CONFIG_FILENAME of config_struct_hammer.hpp:27, is a path in a developer's home directory; the pipeline always passes
// the file.)
// Refused before the first HIP call, with a message that names the key (hammer_config.hpp: hammer_config_refused):
// general_tau != 1, bayes_use_hamming_dist / bayes_hammer_mode / bayes_initial_refine off their shipped values, any
// *_do 0 (the kmer.index* files of an earlier run cannot be read here), expand_write_each_iteration 1; and a library with
// interlaced reads.  Accepted and without effect, as in the reference: correct_discard_bad and
// bayes_discard_only_singletons (they reach CorrectOneRead's unnamed parameters, read_corrector.cpp:160-161); the thread
// counts, general_hard_memory_limit, count_numfiles, count_split_buffer, correct_readbuffer and
// hamming_blocksize_quadratic_threshold size host structures this path does not have.
// Keys of this project (optional; the reference ignores them): bbk_device, bbk_bufsize, bbk_resident_bytes,
// bbk_device_parse -- spades-kmerdata's --device, -b, --resident-bytes and --device-parse.
#include <fstream>
#include <sstream>

#include "hammer_config.hpp"
#include "hammer_run.hpp"

using namespace bbkhost;

// mkdir -p, then the absolute name
static std::string make_dirs_absolute(const std::string &dir) {
    for (size_t i = 1; i < dir.size(); ++i)
        if (dir[i] == '/' && mkdir(dir.substr(0, i).c_str(), 0755) != 0 && errno != EEXIST) fatal("cannot create %s", dir.substr(0, i).c_str());
    return make_dir_absolute(dir);
}

int main(int argc, char **argv) {
    const std::string config_file = argc > 1 ? argv[1] : "config.info";
    info("Starting BayesHammer (MI355X, %s)", bbk_version());
    info("Loading config from %s", config_file.c_str());
    HammerConfig cfg;
    {
        std::ifstream in(config_file, std::ios::binary);
        if (!in) fatal("cannot open config file %s", config_file.c_str());
        std::stringstream text;
        text << in.rdbuf();
        std::string err;
        if (!load_hammer_config(text.str(), cfg, err)) fatal("%s: %s", config_file.c_str(), err.c_str());
        const std::string refused = hammer_config_refused(cfg);
        if (!refused.empty()) fatal("%s: %s", config_file.c_str(), refused.c_str());
    }
    info("Maximum # of threads to use (adjusted due to OMP capabilities): %lu", cfg.general_max_nthreads);
    std::vector<DatasetLib> libs;
    {
        std::string err;
        if (!load_dataset_libs(cfg.dataset, libs, err)) fatal("%s", err.c_str());
    }
    for (size_t ilib = 0; ilib < libs.size(); ++ilib)
        if (!libs[ilib].v[LIB_INTERLACED].empty())
            fatal("dataset %s: library %zu has interlaced reads (%s): interlaced libraries are not supported", cfg.dataset.c_str(),
                  ilib, libs[ilib].v[LIB_INTERLACED][0].c_str());

    HammerParams p;
    p.K = 21;  // hammer's K (projects/hammer/kmer_stat.hpp)
    p.sp = {cfg.bayes_singleton_threshold, cfg.bayes_nonsingleton_threshold, cfg.correct_threshold, cfg.correct_use_threshold ? 1 : 0};
    p.expand_max_iterations = (unsigned)cfg.expand_max_iterations;
    p.trim_quality = (int)cfg.input_trim_quality;
    p.block_bytes = (size_t)cfg.bbk_bufsize;
    p.resident_bytes = cfg.bbk_resident_bytes;
    p.device_parse = cfg.bbk_device_parse;
    p.cluster = p.subcluster = p.expand = p.correct = true;
    p.correct_stats = cfg.correct_stats;
    p.filter_singletons = cfg.count_filter_singletons;
    p.save_yaml = false;  // once, behind the last iteration
    if (cfg.has_qvoffset) {
        p.qvoffset = (int)cfg.input_qvoffset;
    } else {  // main.cpp:84-99
        info("Trying to determine PHRED offset");
        std::string first;
        for (const DatasetLib &l : libs)
            for (int kind = 0; kind < 5 && first.empty(); ++kind)
                if (!l.v[kind].empty()) first = l.v[kind][0];
        const int determined = determine_offset(first);
        if (determined == -2) fatal("cannot open %s", first.c_str());
        if (determined < 0) {
            fprintf(stderr, "Failed to determine offset! Specify it manually and restart, please!\n");
            return -1;
        }
        info("Determined value is %d", determined);
        p.qvoffset = determined;
    }
    p.out_dir = make_dirs_absolute(cfg.output_dir);
    const std::string work_dir = make_dirs_absolute(cfg.input_working_dir);

    Run run;
    run.create_ctx((unsigned)cfg.bbk_device);
    for (unsigned iteration = 0; iteration < cfg.general_max_iterations; ++iteration) {
        printf("\n     === ITERATION %u begins ===\n", iteration);
        fflush(stdout);
        std::vector<InFile> files;
        std::vector<Group> groups;
        std::vector<DatasetLib> outlibs;
        plan_input(libs, /*paired=*/true, files, groups, outlibs);
        p.iteration = iteration;
        char ii[16];
        snprintf(ii, sizeof(ii), "%02u", iteration);
        p.prefix = cfg.general_debug ? work_dir + "/" + ii : std::string();  // getFilename(input_working_dir, iteration_no, ...)
        const uint64_t changed_reads = run_hammer_iteration(run.ctx, run.ph, p, files, groups, outlibs);
        libs = outlibs;  // CorrectAllReads: cfg::get_writable().dataset = outdataset
        if (changed_reads < 1) {
            info("Too few reads have changed in this iteration. Exiting.");
            break;
        }
    }
    save_corrected_yaml(p.out_dir, libs);
    info("All done. Exiting.");
    run.done("spades-hammer");
}
