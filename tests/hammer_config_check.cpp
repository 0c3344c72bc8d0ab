// hammer_config_check <shipped config.info>: host/hammer_config.hpp on the shipped text and on crafted ones (stand-alone,
// built with AddressSanitizer + UBSan by tests/test_hammer_config.py).  Prints HAMMER-CONFIG-CHECK-OK.
#include <cstdio>
#include <fstream>
#include <sstream>

#include "../spades_for_blackbird_amd/host/hammer_config.hpp"

using namespace bbkhost;

static int failures = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                \
        }                                                              \
    } while (0)

static bool has(const std::string &s, const char *word) { return s.find(word) != std::string::npos; }

// the shipped text with the line of `key` replaced by `line` ("" drops it)
static std::string with_line(const std::string &text, const std::string &key, const std::string &line) {
    std::stringstream in(text), out;
    std::string l;
    bool found = false;
    while (std::getline(in, l)) {
        const bool is_key = l.compare(0, key.size(), key) == 0 && l.size() > key.size() && (l[key.size()] == ' ' || l[key.size()] == '\t');
        found = found || is_key;
        if (!is_key) out << l << "\n";
        else if (!line.empty()) out << line << "\n";
    }
    if (!found) fprintf(stderr, "with_line: no line for %s\n", key.c_str()), ++failures;
    return out.str();
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string shipped = ss.str();
    CHECK(!shipped.empty());
    std::string err;

    {  // the shipped text: every key, the values of configs/hammer/config.info
        HammerConfig c;
        CHECK(load_hammer_config(shipped, c, err));
        CHECK(err.empty());
        CHECK(c.dataset == "dataset.yaml" && c.input_working_dir == "./test_dataset/input/corrected/tmp");
        CHECK(c.output_dir == "./test_dataset/input/corrected" && c.input_trim_quality == 4 && !c.has_qvoffset);
        CHECK(c.general_do_everything_after_first_iteration && c.general_hard_memory_limit == 150 && c.general_max_nthreads == 16);
        CHECK(c.general_tau == 1 && c.general_max_iterations == 1 && !c.general_debug);
        CHECK(c.count_do && c.count_numfiles == 16 && c.count_merge_nthreads == 16 && c.count_split_buffer == 0 && !c.count_filter_singletons);
        CHECK(c.hamming_do && c.hamming_blocksize_quadratic_threshold == 50);
        CHECK(c.bayes_do && c.bayes_nthreads == 16 && c.bayes_singleton_threshold == 0.995 && c.bayes_nonsingleton_threshold == 0.9);
        CHECK(!c.bayes_use_hamming_dist && !c.bayes_discard_only_singletons && c.bayes_debug_output == 0 && !c.bayes_hammer_mode);
        CHECK(!c.bayes_write_solid_kmers && !c.bayes_write_bad_kmers && c.bayes_initial_refine);
        CHECK(c.expand_do && c.expand_max_iterations == 25 && c.expand_nthreads == 6 && !c.expand_write_each_iteration && !c.expand_write_kmers_result);
        CHECK(c.correct_do && !c.correct_discard_bad && c.correct_use_threshold && c.correct_threshold == 0.98);
        CHECK(c.correct_nthreads == 4 && c.correct_readbuffer == 100000 && c.correct_stats);
        CHECK(c.bbk_device == 0 && c.bbk_bufsize == 536870912ul && c.bbk_resident_bytes == 0 && !c.bbk_device_parse);
        CHECK(hammer_config_refused(c).empty());
        CHECK(c.kv.count("input_qvoffset") == 1 && c.kv["input_qvoffset"].empty());  // a key without a value
    }
    {  // the format: comments, quotes with escapes, a key without a value, a duplicate, an unknown key, CR LF
        std::map<std::string, std::string> kv;
        const std::string text =
            "; a comment line\n"
            "   ; an indented one\n"
            "\n"
            "plain   value ; a comment behind a value\n"
            "tabbed\t\tvalue2\r\n"
            "quoted  \"a value; with \\\"quotes\\\" and a \\\\ backslash\"   ; and a comment\n"
            "empty_quotes \"\"\n"
            "bare\n"
            "bare_with_comment ; nothing here\n"
            "twice first\n"
            "twice second\n"
            "\"quoted key\" 7\n"
            "last_line_without_newline 1";
        CHECK(parse_info(text, kv, err));
        CHECK(kv.size() == 9);
        CHECK(kv["plain"] == "value" && kv["tabbed"] == "value2");
        CHECK(kv["quoted"] == "a value; with \"quotes\" and a \\ backslash");
        CHECK(kv.count("empty_quotes") && kv["empty_quotes"].empty() && kv.count("bare") && kv["bare"].empty());
        CHECK(kv.count("bare_with_comment") && kv["bare_with_comment"].empty());
        CHECK(kv["twice"] == "second" && kv["quoted key"] == "7" && kv["last_line_without_newline"] == "1");
        kv.clear();
        CHECK(parse_info("", kv, err) && kv.empty());
        CHECK(!parse_info("a 1\nb \"open\n", kv, err) && has(err, "line 2") && has(err, "quote"));
        CHECK(!parse_info("a 1 2\n", kv, err) && has(err, "line 1") && has(err, "a"));
        CHECK(!parse_info("section\n{\n  a 1\n}\n", kv, err) && has(err, "line 2"));
        CHECK(!parse_info("#include \"other.info\"\n", kv, err) && has(err, "line 1"));
        CHECK(!parse_info("a \"one\" \\\n  \"two\"\n", kv, err) && has(err, "continuation"));
    }
    {  // the stage script's substitutions, an unknown key and this project's keys
        HammerConfig c;
        std::string t = with_line(shipped, "dataset", "dataset \"/data/my reads/dataset.yaml\"");
        t = with_line(t, "input_qvoffset", "input_qvoffset 64");
        t = with_line(t, "count_filter_singletons", "count_filter_singletons 1");
        t = with_line(t, "general_max_iterations", "general_max_iterations 3");
        t += "some_future_key 12\nbbk_device 3\nbbk_bufsize 1000\nbbk_resident_bytes 5\nbbk_device_parse 1\ngeneral_debug 1\n";
        CHECK(load_hammer_config(t, c, err));
        CHECK(c.dataset == "/data/my reads/dataset.yaml" && c.has_qvoffset && c.input_qvoffset == 64 && c.count_filter_singletons);
        CHECK(c.general_max_iterations == 3 && c.general_debug);  // (general_debug stands twice: the later one wins)
        CHECK(c.bbk_device == 3 && c.bbk_bufsize == 1000 && c.bbk_resident_bytes == 5 && c.bbk_device_parse);
        CHECK(hammer_config_refused(c).empty());
    }
    {  // every key config_struct_hammer.cpp loads with load(...) is required, and the error names it
        const char *required[] = {"general_do_everything_after_first_iteration", "general_hard_memory_limit", "general_max_nthreads",
                                  "general_tau", "general_max_iterations", "general_debug", "count_do", "count_numfiles",
                                  "count_merge_nthreads", "count_split_buffer", "count_filter_singletons", "hamming_do",
                                  "hamming_blocksize_quadratic_threshold", "bayes_do", "bayes_nthreads", "bayes_singleton_threshold",
                                  "bayes_nonsingleton_threshold", "bayes_discard_only_singletons", "bayes_debug_output",
                                  "bayes_use_hamming_dist", "bayes_hammer_mode", "bayes_write_bad_kmers", "bayes_write_solid_kmers",
                                  "bayes_initial_refine", "expand_do", "expand_max_iterations", "expand_nthreads",
                                  "expand_write_each_iteration", "expand_write_kmers_result", "correct_do", "correct_nthreads",
                                  "correct_threshold", "correct_use_threshold", "correct_readbuffer", "correct_discard_bad",
                                  "correct_stats", "dataset", "input_working_dir", "input_trim_quality", "output_dir"};
        for (const char *key : required) {
            HammerConfig c;
            err.clear();
            CHECK(!load_hammer_config(with_line(shipped, key, ""), c, err));
            CHECK(has(err, (std::string("(") + key + ")").c_str()));
        }
        HammerConfig c;
        CHECK(load_hammer_config(with_line(shipped, "input_qvoffset", ""), c, err) && !c.has_qvoffset);  // optional
        CHECK(!load_hammer_config(with_line(shipped, "general_tau", "general_tau one"), c, err) && has(err, "general_tau"));
        CHECK(!load_hammer_config(with_line(shipped, "count_do", "count_do 2"), c, err) && has(err, "count_do"));
        CHECK(!load_hammer_config(with_line(shipped, "correct_threshold", "correct_threshold 0.9x"), c, err) && has(err, "correct_threshold"));
        CHECK(!load_hammer_config(with_line(shipped, "general_max_nthreads", "general_max_nthreads -1"), c, err) && has(err, "general_max_nthreads"));
    }
    {  // input_qvoffset: get_optional<int>
        const struct {
            const char *line;
            bool has;
            long value;
        } rows[] = {{"input_qvoffset", false, 0},      {"input_qvoffset \"\"", false, 0}, {"input_qvoffset 33", true, 33},
                    {"input_qvoffset 64", true, 64},   {"input_qvoffset x", false, 0},    {"input_qvoffset 33x", false, 0},
                    {"input_qvoffset 3.5", false, 0}};
        for (const auto &r : rows) {
            HammerConfig c;
            CHECK(load_hammer_config(with_line(shipped, "input_qvoffset", r.line), c, err));
            CHECK(c.has_qvoffset == r.has && (!r.has || c.input_qvoffset == r.value));
        }
    }
    {  // what the driver refuses, by key
        const struct {
            const char *key, *line;
        } rows[] = {{"general_tau", "general_tau 2"},
                    {"general_tau", "general_tau 0"},
                    {"bayes_use_hamming_dist", "bayes_use_hamming_dist 1"},
                    {"bayes_hammer_mode", "bayes_hammer_mode 1"},
                    {"bayes_initial_refine", "bayes_initial_refine 0"},
                    {"count_do", "count_do 0"},
                    {"hamming_do", "hamming_do 0"},
                    {"bayes_do", "bayes_do 0"},
                    {"expand_do", "expand_do 0"},
                    {"correct_do", "correct_do 0"},
                    {"expand_write_each_iteration", "expand_write_each_iteration 1"},
                    {"input_trim_quality", "input_trim_quality 94"},
                    {"input_qvoffset", "input_qvoffset 200"}};
        for (const auto &r : rows) {
            HammerConfig c;
            CHECK(load_hammer_config(with_line(shipped, r.key, r.line), c, err));
            const std::string why = hammer_config_refused(c);
            CHECK(!why.empty() && why.compare(0, strlen(r.key), r.key) == 0);
        }
        // accepted whatever they say: they reach CorrectOneRead's unnamed parameters
        HammerConfig c;
        std::string t = with_line(shipped, "correct_discard_bad", "correct_discard_bad 1");
        t = with_line(t, "bayes_discard_only_singletons", "bayes_discard_only_singletons 1");
        CHECK(load_hammer_config(t, c, err) && c.correct_discard_bad && c.bayes_discard_only_singletons && hammer_config_refused(c).empty());
    }
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("HAMMER-CONFIG-CHECK-OK\n");
    return 0;
}
