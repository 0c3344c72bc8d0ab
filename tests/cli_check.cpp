// host-only check of the option table of the host tools (spades_for_blackbird_amd/host/cli.hpp) on fixed argv arrays
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <vector>

#include "../spades_for_blackbird_amd/host/cli.hpp"

using bbkhost::Options;

#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
            exit(1);                                                 \
        }                                                            \
    } while (0)

// parse() over argv[0] = "tool" and the given words, each in storage of exactly its own size (for the sanitizer)
static bool run(Options &o, std::initializer_list<const char *> words) {
    std::vector<std::string> own{"tool"};
    own.insert(own.end(), words.begin(), words.end());
    std::vector<std::vector<char>> store;
    for (const std::string &w : own) store.emplace_back(w.c_str(), w.c_str() + w.size() + 1);
    std::vector<char *> argv;
    for (auto &s : store) argv.push_back(s.data());
    return o.parse((int)argv.size(), argv.data());
}

// one -k <word> into a T with bounds; returns whether it parsed, *out the value
template <class T>
static bool one(const char *word, T *out, T lo = 0, T hi = (T)-1) {
    Options o;
    o.num("-k", "--kmer", out, lo, hi);
    const bool ok = run(o, {"-k", word});
    CHECK(o.seen("-k") == ok && o.seen("--kmer") == ok);
    return ok;
}

int main() {
    unsigned u = 7;
    unsigned long long w = 7;
    // what fits and what does not
    CHECK(one("21", &u) && u == 21);
    CHECK(one("4294967295", &u) && u == 4294967295u);
    CHECK(one("0000000000000000000000000000000000021", &u) && u == 21);
    u = 7;
    CHECK(!one("4294967296", &u) && u == 7);   // 2^32
    CHECK(!one("4294967317", &u) && u == 7);   // 2^32 + 21: used to run as 21
    CHECK(one("4294967296", &w) && w == 4294967296ull);
    CHECK(one("18446744073709551615", &w) && w == 18446744073709551615ull);
    w = 7;
    CHECK(!one("18446744073709551616", &w) && w == 7);  // 2^64
    CHECK(!one("18446744073709551620", &w) && w == 7);
    CHECK(!one("123456789012345678901234567890", &w) && w == 7);
    // digits only
    for (const char *bad : {"", "-5", "+5", " 5", "5 ", "0x10", "1e3", "5.0", "x", "-", "--kmer"}) CHECK(!one(bad, &u) && u == 7);
    // bounds, inclusive on both sides
    CHECK(one("1", &u, 1u, 999u) && u == 1);
    CHECK(one("999", &u, 1u, 999u) && u == 999);
    u = 7;
    CHECK(!one("0", &u, 1u, 999u) && !one("1000", &u, 1u, 999u) && u == 7);
    CHECK(one("4294967295", &w, 0ull, 0xFFFFFFFFull) && !one("4294967296", &w, 0ull, 0xFFFFFFFFull));

    {  // a value missing at the very end; parsing went on before it
        Options o;
        std::string d;
        o.num("-k", "", &u).str("-d", "--dataset", &d);
        CHECK(!run(o, {"--dataset", "x.yaml", "-k"}) && d == "x.yaml" && o.seen("-d") && !o.seen("-k"));
        Options p;
        p.str("-d", "--dataset", &d);
        CHECK(!run(p, {"-d"}) && d == "x.yaml" && !p.seen("--dataset"));
    }
    {  // parsing goes on after an error; a value is taken even if it looks like an option; the last value wins
        Options o;
        std::string d;
        u = 7;
        o.num("-k", "", &u).str("-d", "", &d);
        CHECK(!run(o, {"-k", "x", "-d", "-k", "-k", "5", "-k", "9"}) && d == "-k" && u == 9 && o.seen("-k"));
        Options p;
        p.num("-k", "", &u).str("-d", "", &d);
        CHECK(!run(p, {"-k", "5", "-k", "x"}) && u == 5);  // the bad repeat is an error and leaves the value
    }
    {  // an unknown option with and without positionals; "-" and "" are words; a bare word needs positional()
        std::vector<std::string> pos;
        bool h = false;
        Options o;
        o.flag("-h", "--help", &h).positional(&pos);
        CHECK(!run(o, {"a.fa", "--bogus", "-", "", "-x", "b.fa"}) && !h);
        CHECK(pos == (std::vector<std::string>{"a.fa", "-", "", "b.fa"}));
        Options p;
        bool help = false;
        p.flag("-h", "--help", &help);
        CHECK(!run(p, {"--bogus"}) && !run(p, {"word"}) && !run(p, {"-"}) && !run(p, {""}) && !help && !p.seen("-h"));
        CHECK(run(p, {"--help"}) && help && p.seen("-h") && !p.seen("--bogus") && !p.seen(""));
        CHECK(run(p, {}));
    }
    {  // an ignored value-taking option swallows its value, and needs one
        std::vector<std::string> pos;
        Options o;
        o.ignored("-tmp-dir", "").ignored("", "--tmpdir").positional(&pos);
        CHECK(run(o, {"a", "-tmp-dir", "t", "--tmpdir", "-u", "b"}) && pos == (std::vector<std::string>{"a", "b"}));
        CHECK(o.seen("-tmp-dir") && o.seen("--tmpdir"));
        CHECK(!run(o, {"a", "--tmpdir"}));
    }
    {  // a counted flag: the callback runs each time
        int given = 0, mode = 0;
        Options o;
        o.flag("", "--gfa", [&] { mode = 1, ++given; }).flag("", "--fastg", [&] { mode = 2, ++given; });
        CHECK(run(o, {"--gfa", "--fastg", "--gfa"}) && given == 3 && mode == 1 && o.seen("--gfa") && o.seen("--fastg"));
    }
    {  // real: what strtod reads, all of the word
        double d = 0.25;
        Options o;
        o.real("", "--threshold", &d);
        CHECK(!run(o, {"--threshold", "abc"}) && d == 0.25 && !o.seen("--threshold"));
        CHECK(!run(o, {"--threshold", "0.5x"}) && d == 0.25);
        CHECK(!run(o, {"--threshold", ""}) && d == 0.25);
        CHECK(!run(o, {"--threshold"}) && d == 0.25);
        CHECK(run(o, {"--threshold", "1e-3"}) && d == 1e-3 && o.seen("--threshold"));
        CHECK(run(o, {"--threshold", "0.995"}) && d == 0.995);
    }
    printf("CLI-CHECK-OK\n");
    return 0;
}
