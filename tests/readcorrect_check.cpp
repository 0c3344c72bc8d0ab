// readcorrect_check.cpp -- stand-alone host program of tests/test_readcorrect_host.py: runs csrc/readcorrect_host.hpp over
// a case file and prints what it computed.  No GPU, no engine; the test builds it with AddressSanitizer and
// UndefinedBehaviorSanitizer.
//   case file:  k n_keys n_reads
//               n_keys lines  "<key as decimal u64> <good 0/1>", keys ascending
//               n_reads lines "<length> <bases> <qualities as bytes q + 33>" ("0" alone for an empty read)
//   output:     per read   "read <result> <bases or ->"
//               per search "search <read> <0 right / 1 left> <pops> <largest heap> <failed>"
//               at the end "stats <changed reads> <changed bases> <uncorrected bases> <total bases>"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../spades_for_blackbird_amd/csrc/readcorrect_host.hpp"

namespace rc = bbkhost::readcorrect;

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: readcorrect_check <case file>\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    unsigned k = 0;
    size_t n_keys = 0, n_reads = 0;
    if (!(in >> k >> n_keys >> n_reads) || k < 1 || k > 32) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    std::vector<uint64_t> keys(n_keys);
    std::vector<uint8_t> good(n_keys);
    for (size_t i = 0; i < n_keys; ++i) {
        unsigned g;
        if (!(in >> keys[i] >> g) || g > 1 || (i && keys[i] <= keys[i - 1])) {
            fprintf(stderr, "bad key line %zu\n", i);
            return 2;
        }
        good[i] = (uint8_t)g;
    }
    auto lookup = [&](uint64_t key) -> uint64_t {
        auto it = std::lower_bound(keys.begin(), keys.end(), key);
        return it != keys.end() && *it == key ? (uint64_t)(it - keys.begin()) : rc::kNone;
    };
    rc::Counters cnt;
    for (size_t r = 0; r < n_reads; ++r) {
        size_t len;
        std::string seq, qual;
        if (!(in >> len) || (len && !(in >> seq >> qual)) || seq.size() != len || qual.size() != len) {
            fprintf(stderr, "bad read line %zu\n", r);
            return 2;
        }
        for (char &c : qual) c = (char)(c - 33);
        bool res = false;
        std::vector<rc::SearchFigures> searches;
        if (seq.size() >= k) res = rc::CorrectOneRead(seq, qual, k, lookup, good.data(), cnt, &searches);  // hammer_tools.cpp:90-95
        printf("read %d %s\n", (int)res, seq.empty() ? "-" : seq.c_str());
        for (size_t d = 0; d < searches.size(); ++d)
            printf("search %zu %zu %llu %llu %d\n", r, d, (unsigned long long)searches[d].pops,
                   (unsigned long long)searches[d].max_heap, (int)searches[d].failed);
    }
    printf("stats %llu %llu %llu %llu\n", (unsigned long long)cnt.changed_reads, (unsigned long long)cnt.changed_nucleotides,
           (unsigned long long)cnt.uncorrected_nucleotides, (unsigned long long)cnt.total_nucleotides);
    return 0;
}
