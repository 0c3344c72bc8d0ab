// hammer_config.hpp -- BayesHammer's configuration file (configs/hammer/config.info as the pipeline's error-correction stage
// fills it in, spades_pipeline/stages/error_correction_stage.py:25-43) for spades-hammer.  No HIP, no C ABI: a header a
// stand-alone program can test.
//
// The file is in boost's INFO format (boost::property_tree::read_info, projects/hammer/config_struct_hammer.cpp:22-27).
// The reader takes the subset that file and the stage script produce: one `key<whitespace>value` per line, `;` starts a
// comment, a value may be double-quoted with \" and \\ inside, a key may stand without a value, and the later duplicate of
// a key wins.  Sections ({ }), #include and continuation lines are refused with their line number.
// load() then does what config_struct_hammer.cpp:29-83 does: every key loaded there with load(...) is required and
// converted as ptree's stream translator converts it, input_qvoffset is get_optional<int> (an empty or non-integer value:
// absent), unknown keys are ignored.  refused() names the first setting spades-hammer does not support.
#pragma once

#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

namespace bbkhost {

struct HammerConfig {
    std::map<std::string, std::string> kv;  // every key of the file, the later duplicate on top

    std::string dataset, input_working_dir, output_dir;
    long input_trim_quality = 0;
    bool has_qvoffset = false;
    long input_qvoffset = 0;

    bool general_do_everything_after_first_iteration = false, general_debug = false;
    long general_hard_memory_limit = 0, general_tau = 0;
    unsigned long general_max_nthreads = 0, general_max_iterations = 0;

    bool count_do = false, count_filter_singletons = false;
    unsigned long count_numfiles = 0, count_merge_nthreads = 0, count_split_buffer = 0;

    bool hamming_do = false;
    unsigned long hamming_blocksize_quadratic_threshold = 0;

    bool bayes_do = false, bayes_discard_only_singletons = false, bayes_use_hamming_dist = false, bayes_hammer_mode = false,
         bayes_write_solid_kmers = false, bayes_write_bad_kmers = false, bayes_initial_refine = false;
    unsigned long bayes_nthreads = 0, bayes_debug_output = 0;
    double bayes_singleton_threshold = 0, bayes_nonsingleton_threshold = 0;

    bool expand_do = false, expand_write_each_iteration = false, expand_write_kmers_result = false;
    unsigned long expand_max_iterations = 0, expand_nthreads = 0;

    bool correct_do = false, correct_discard_bad = false, correct_use_threshold = false, correct_stats = false;
    double correct_threshold = 0;
    unsigned long correct_readbuffer = 0, correct_nthreads = 0;

    // keys of this project, absent from the reference's file and ignored by it; the defaults are spades-kmerdata's
    unsigned long bbk_device = 0, bbk_bufsize = 536870912ul, bbk_resident_bytes = 0;
    bool bbk_device_parse = false;
};

namespace hammer_config_detail {

inline bool is_space(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f'; }

// One word of a line from position i on: quoted (escapes \" and \\; any other escaped character stands for itself) or up
// to white space or a comment.  false: an unterminated quote or a section brace.
inline bool read_word(const std::string &line, size_t &i, std::string &out, std::string &why) {
    out.clear();
    if (i < line.size() && line[i] == '"') {
        for (++i; i < line.size(); ++i) {
            if (line[i] == '\\' && i + 1 < line.size()) out += line[++i];
            else if (line[i] == '"') return ++i, true;
            else out += line[i];
        }
        why = "unterminated quote";
        return false;
    }
    for (; i < line.size() && !is_space(line[i]) && line[i] != ';'; ++i) {
        if (line[i] == '{' || line[i] == '}') {
            why = "sections are not supported";
            return false;
        }
        out += line[i];
    }
    return true;
}

inline bool to_long(const std::string &s, long &v) {
    if (s.empty() || is_space(s[0])) return false;
    errno = 0;
    char *end = nullptr;
    v = strtol(s.c_str(), &end, 10);
    return errno == 0 && end != s.c_str() && *end == '\0';
}
inline bool to_ulong(const std::string &s, unsigned long &v) {
    if (s.empty() || is_space(s[0]) || s[0] == '-') return false;
    errno = 0;
    char *end = nullptr;
    v = strtoul(s.c_str(), &end, 10);
    return errno == 0 && end != s.c_str() && *end == '\0';
}
inline bool to_double(const std::string &s, double &v) {
    if (s.empty() || is_space(s[0])) return false;
    errno = 0;
    char *end = nullptr;
    v = strtod(s.c_str(), &end);
    return errno == 0 && end != s.c_str() && *end == '\0';
}
inline bool to_bool(const std::string &s, bool &v) {  // the stream translator: 0 / 1, then boolalpha
    if (s == "0" || s == "false") return v = false, true;
    if (s == "1" || s == "true") return v = true, true;
    return false;
}

}  // namespace hammer_config_detail

// The keys and values of INFO text; false with `err` naming the line
inline bool parse_info(const std::string &text, std::map<std::string, std::string> &kv, std::string &err) {
    using namespace hammer_config_detail;
    size_t pos = 0, line_no = 0;
    while (pos <= text.size()) {
        const size_t nl = text.find('\n', pos);
        const std::string line = text.substr(pos, nl == std::string::npos ? std::string::npos : nl - pos);
        pos = nl == std::string::npos ? text.size() + 1 : nl + 1;
        ++line_no;
        size_t i = 0;
        auto skip = [&] {
            while (i < line.size() && is_space(line[i])) ++i;
        };
        auto fail = [&](const std::string &why) {
            err = "line " + std::to_string(line_no) + ": " + why;
            return false;
        };
        skip();
        if (i == line.size() || line[i] == ';') continue;
        if (line[i] == '#') return fail("#include is not supported");
        std::string key, value, why;
        if (!read_word(line, i, key, why)) return fail(why);
        skip();
        if (i < line.size() && line[i] != ';' && !read_word(line, i, value, why)) return fail(why);
        skip();
        if (i < line.size() && line[i] == '\\') return fail("continuation lines are not supported");
        if (i < line.size() && line[i] != ';') return fail("unexpected text behind the value of " + key);
        kv[key] = value;
    }
    return true;
}

// config_struct_hammer.cpp:29-83 over INFO text; false with `err` naming the key that is missing or does not convert
inline bool load_hammer_config(const std::string &text, HammerConfig &c, std::string &err) {
    using namespace hammer_config_detail;
    if (!parse_info(text, c.kv, err)) return false;
    bool ok = true;
    auto raw = [&](const char *key, bool required) -> const std::string * {
        const auto it = c.kv.find(key);
        if (it != c.kv.end()) return &it->second;
        if (required && ok) {
            ok = false;
            err = std::string("No such node (") + key + ")";  // ptree_bad_path's words
        }
        return nullptr;
    };
    auto bad = [&](const char *key, const std::string &v) {
        if (ok) err = std::string("conversion of data to type failed: ") + key + " = \"" + v + "\"";
        ok = false;
    };
    auto B = [&](bool &dst, const char *key, bool required = true) {
        if (const std::string *v = raw(key, required))
            if (!to_bool(*v, dst)) bad(key, *v);
    };
    auto U = [&](unsigned long &dst, const char *key, bool required = true) {
        if (const std::string *v = raw(key, required))
            if (!to_ulong(*v, dst)) bad(key, *v);
    };
    auto I = [&](long &dst, const char *key) {
        if (const std::string *v = raw(key, true))
            if (!to_long(*v, dst)) bad(key, *v);
    };
    auto D = [&](double &dst, const char *key) {
        if (const std::string *v = raw(key, true))
            if (!to_double(*v, dst)) bad(key, *v);
    };
    auto S = [&](std::string &dst, const char *key) {
        if (const std::string *v = raw(key, true)) dst = *v;
    };
    B(c.general_do_everything_after_first_iteration, "general_do_everything_after_first_iteration");
    I(c.general_hard_memory_limit, "general_hard_memory_limit");
    U(c.general_max_nthreads, "general_max_nthreads");
    I(c.general_tau, "general_tau");
    U(c.general_max_iterations, "general_max_iterations");
    B(c.general_debug, "general_debug");
    B(c.count_do, "count_do");
    U(c.count_numfiles, "count_numfiles");
    U(c.count_merge_nthreads, "count_merge_nthreads");
    U(c.count_split_buffer, "count_split_buffer");
    B(c.count_filter_singletons, "count_filter_singletons");
    B(c.hamming_do, "hamming_do");
    U(c.hamming_blocksize_quadratic_threshold, "hamming_blocksize_quadratic_threshold");
    B(c.bayes_do, "bayes_do");
    U(c.bayes_nthreads, "bayes_nthreads");
    D(c.bayes_singleton_threshold, "bayes_singleton_threshold");
    D(c.bayes_nonsingleton_threshold, "bayes_nonsingleton_threshold");
    B(c.bayes_discard_only_singletons, "bayes_discard_only_singletons");
    U(c.bayes_debug_output, "bayes_debug_output");
    B(c.bayes_use_hamming_dist, "bayes_use_hamming_dist");
    B(c.bayes_hammer_mode, "bayes_hammer_mode");
    B(c.bayes_write_bad_kmers, "bayes_write_bad_kmers");
    B(c.bayes_write_solid_kmers, "bayes_write_solid_kmers");
    B(c.bayes_initial_refine, "bayes_initial_refine");
    B(c.expand_do, "expand_do");
    U(c.expand_max_iterations, "expand_max_iterations");
    U(c.expand_nthreads, "expand_nthreads");
    B(c.expand_write_each_iteration, "expand_write_each_iteration");
    B(c.expand_write_kmers_result, "expand_write_kmers_result");
    B(c.correct_do, "correct_do");
    U(c.correct_nthreads, "correct_nthreads");
    D(c.correct_threshold, "correct_threshold");
    B(c.correct_use_threshold, "correct_use_threshold");
    U(c.correct_readbuffer, "correct_readbuffer");
    B(c.correct_discard_bad, "correct_discard_bad");
    B(c.correct_stats, "correct_stats");
    S(c.dataset, "dataset");
    S(c.input_working_dir, "input_working_dir");
    I(c.input_trim_quality, "input_trim_quality");
    if (const std::string *v = raw("input_qvoffset", false)) c.has_qvoffset = to_long(*v, c.input_qvoffset);  // get_optional<int>
    S(c.output_dir, "output_dir");
    U(c.bbk_device, "bbk_device", false);
    U(c.bbk_bufsize, "bbk_bufsize", false);
    U(c.bbk_resident_bytes, "bbk_resident_bytes", false);
    B(c.bbk_device_parse, "bbk_device_parse", false);
    return ok;
}

// The first setting spades-hammer refuses, as a message that names its key; empty: the configuration is supported.
// (Interlaced libraries are a property of the dataset: the driver refuses them when it has read it.)
inline std::string hammer_config_refused(const HammerConfig &c) {
    if (c.general_tau != 1) return "general_tau " + std::to_string(c.general_tau) + ": only tau = 1 is supported";
    if (c.bayes_use_hamming_dist) return "bayes_use_hamming_dist 1: only the shipped value 0 is supported";
    if (c.bayes_hammer_mode) return "bayes_hammer_mode 1: only the shipped value 0 is supported";
    if (!c.bayes_initial_refine) return "bayes_initial_refine 0: only the shipped value 1 is supported";
    const struct {
        const char *key;
        bool on;
    } steps[] = {{"count_do", c.count_do}, {"hamming_do", c.hamming_do}, {"bayes_do", c.bayes_do},
                 {"expand_do", c.expand_do}, {"correct_do", c.correct_do}};
    for (const auto &s : steps)
        if (!s.on)
            return std::string(s.key) + " 0: a restart from the kmer.index* files of an earlier run is not supported "
                   "(they are BooPHF-indexed and cannot be read here)";
    if (c.expand_write_each_iteration) return "expand_write_each_iteration 1: the per-iteration goodkmers files are not written";
    if (c.input_trim_quality < 0 || c.input_trim_quality > 93) return "input_trim_quality " + std::to_string(c.input_trim_quality) + ": out of range [0, 93]";
    if (c.has_qvoffset && (c.input_qvoffset < 0 || c.input_qvoffset > 162))
        return "input_qvoffset " + std::to_string(c.input_qvoffset) + ": out of range [0, 162]";
    if (c.expand_max_iterations > 0xFFFFFFFFul || c.bbk_device > 0xFFFFFFFFul) return "expand_max_iterations / bbk_device: out of range";
    if (c.bbk_bufsize == 0) return "bbk_bufsize 0: a block holds at least one byte";
    return "";
}

}  // namespace bbkhost
