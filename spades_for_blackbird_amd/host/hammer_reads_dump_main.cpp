// bbk-hammer-reads-dump [-k <int=21>] [--qvoffset <int=33>] [--trim-quality <int=4>] [--expander] <file>...: test helper
// for hammer_reads.hpp (no GPU needed).  For every FASTQ record, in file order, one line per stretch of valid k-mer starts:
//   <read index> <start> <length>
// (read index counts the records of all files from 0; a record without a stretch prints nothing).  With --expander: one
// such line for every record the Expander can ever find solid (expander_candidate), the trimmed read, and nothing else.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fastx.hpp"
#include "hammer_reads.hpp"

int main(int argc, char **argv) {
    unsigned k = 21;
    int qvoffset = 33, trim_quality = 4;
    int first = 1;
    bool expander = false;
    while (first < argc && argv[first][0] == '-') {
        if (!strcmp(argv[first], "--expander")) {
            expander = true;
            first += 1;
            continue;
        }
        if (first + 1 >= argc) return 2;
        if (!strcmp(argv[first], "-k")) k = (unsigned)atoi(argv[first + 1]);
        else if (!strcmp(argv[first], "--qvoffset")) qvoffset = atoi(argv[first + 1]);
        else if (!strcmp(argv[first], "--trim-quality")) trim_quality = atoi(argv[first + 1]);
        else return 2;
        first += 2;
    }
    if (k < 1 || first >= argc) return 2;
    unsigned long long index = 0;
    std::string name, seq, qual;
    std::vector<bbkhost::hammer::Stretch> st;
    for (int i = first; i < argc; ++i) {
        bbkhost::FastxReader rd(argv[i]);
        if (!rd.is_open()) {
            fprintf(stderr, "cannot open %s\n", argv[i]);
            return 2;
        }
        while (rd.next_record(name, seq, qual)) {
            if (qual.size() != seq.size()) {
                fprintf(stderr, "record %llu has no quality string\n", index);
                return 2;
            }
            for (char &c : qual) c = (char)(c - qvoffset);
            st.clear();
            bbkhost::hammer::Stretch whole;
            if (!expander) bbkhost::hammer::valid_stretches(seq, qual, k, trim_quality, st);
            else if (bbkhost::hammer::expander_candidate(seq, qual, k, trim_quality, &whole)) st.push_back(whole);
            for (const auto &s : st) printf("%llu %u %u\n", index, s.start, s.length);
            ++index;
        }
    }
    return 0;
}
