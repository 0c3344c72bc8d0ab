// Host-only check of csrc/gfa_graph.h: the GFA1 reader, the segment / link / loop passes of the edge index and the
// block-parallel text writer.
//   gfa_graph_check                   prints GFA-GRAPH-OK and exits 0, or says what differed and exits 1
//   gfa_graph_check dump <file> <k>   the graph as the passes see it, for tests/test_gfa_graph.py:
//                                       S <name> <sequence> <KC> <self-conjugate 0|1> <loop flag 0|1>
//                                       L <segment a> <+|-> <segment b> <+|-> (by segment index), or ERROR <message>
// Every case is a tiny text with its expected values written out here.  The text is parsed from a heap block of its
// exact size, so a read past either end is an AddressSanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../spades_for_blackbird_amd/csrc/gfa_graph.h"

namespace {

using namespace bbk;

int failures = 0;

void check(bool ok, const std::string &what, const std::string &got = "") {
    if (!ok && failures++ < 30) std::fprintf(stderr, "FAILED: %s [%s]\n", what.c_str(), got.c_str());
}

struct Parsed {
    HostGraph g;
    GraphError e;
};

Parsed parse(const std::string &text, unsigned k) {
    Parsed p;
    const std::vector<char> exact(text.begin(), text.end());
    p.e = parse_gfa_text(exact.data(), exact.data() + exact.size(), k, "g.gfa", p.g);
    return p;
}

void refused(const std::string &text, unsigned k, const std::string &msg) {
    const Parsed p = parse(text, k);
    check(p.e && !p.e.io && p.e.msg == msg, "refusal: " + msg, p.e.msg);
}

bool same_link(const HostLink &l, uint32_t a, bool oa, uint32_t b, bool ob) {
    return l.a == a && l.oa == oa && l.b == b && l.ob == ob;
}

void parsing() {
    // line ends: CRLF, LF without a last newline, an empty file
    for (const char *eol : {"\r\n", "\n"})
        for (bool last_newline : {true, false}) {
            const std::string e = eol;
            const Parsed p = parse("S\t3\tACGTA" + e + "S\t5\tGTACC" + e + "L\t3\t+\t5\t-\t3M" + (last_newline ? e : ""), 3);
            check(!p.e, "line ends accepted", p.e.msg);
            check(p.g.names == std::vector<std::string>{"3", "5"} && p.g.bases == "ACGTAGTACC" &&
                      p.g.off == std::vector<uint64_t>{0, 5, 10} && p.g.kc == std::vector<uint32_t>{0, 0},
                  "line ends: segments", p.g.bases);
            check(p.g.links.size() == 1 && same_link(p.g.links[0], 0, true, 1, false), "line ends: link");
        }
    {
        const Parsed p = parse("", 3);
        check(!p.e && p.g.names.empty() && p.g.bases.empty() && p.g.off == std::vector<uint64_t>{0} && p.g.links.empty(),
              "empty file", p.e.msg);
    }
    {  // lower case; H, P and # lines, an S without a tab and an empty line are not records
        const Parsed p = parse("H\tVN:Z:1.0\n# S\t9\tAAAA\nP\tp\t3+\t*\n\nS\nS\tx\tacgTa\n", 3);
        check(!p.e && p.g.names == std::vector<std::string>{"x"} && p.g.bases == "ACGTA", "lower case and ignored lines",
              p.e.msg + p.g.bases);
    }
    refused("S\t3\n", 3, "g.gfa:1: S line without a sequence");
    refused("S\t3\tACGTA\n\nS\t5\tACNTA\n", 3, "g.gfa:3: segment 5 holds a base other than ACGT ('N')");
    refused("S\t3\tACGTA\r\nS\t5\tACG-A\r\n", 3, "g.gfa:2: segment 5 holds a base other than ACGT ('-')");
    {  // KC:i: -- the first tag wins, a negative value wraps, none gives 0, a tag that ends the text is read to its end
        const Parsed p = parse("S\t3\tACGTA\tKC:i:7\tKC:i:9\nS\t5\tACGTA\tLN:i:5\tKC:i:-1\nS\t7\tACGTA\tLN:i:5\nS\t9\tACGTA\tKC:i:12",
                               3);
        check(!p.e && p.g.kc == std::vector<uint32_t>{7, 0xFFFFFFFFu, 0, 12}, "KC:i:", p.e.msg);
    }
    // L lines
    const std::string two = "S\t3\tACGTA\nS\t5\tGTACC\n";
    refused(two + "L\t3\t+\t5\t+\n", 3, "g.gfa:3: malformed L line");
    refused(two + "L\t3\t*\t5\t+\t3M\n", 3, "g.gfa:3: malformed L line");
    refused(two + "L\t3\t+\t5\t+-\t3M\n", 3, "g.gfa:3: malformed L line");
    refused(two + "L\t3\t+\t5\t+\t20M\n", 21, "g.gfa:3: link overlap 20M, only 21M (a k-overlap at k = 21) is supported");
    refused(two + "L\t3\t+\t5\t+\t*\n", 3, "g.gfa:3: link overlap *, only 3M (a k-overlap at k = 3) is supported");
    // names 3, 5, 7: taken by value
    const std::string three = two + "S\t7\tTACCA\n";
    {
        const Parsed p = parse(three + "L\t7\t-\t3\t+\t3M\nL\t5\t+\t7\t+\t3M\tRC:i:4\n", 3);
        check(!p.e && p.g.links.size() == 2 && same_link(p.g.links[0], 2, false, 0, true) &&
                  same_link(p.g.links[1], 1, true, 2, true),
              "links by value", p.e.msg);
    }
    for (const char *name : {"05", "4", "9", "1", "0", "", "3x", "99999999999999999999", "18446744073709551619"}) {
        refused(three + "L\t3\t+\t" + name + "\t+\t3M\n", 3, "g.gfa:4: link to an undefined segment");
        refused(three + "\nL\t" + name + "\t-\t3\t+\t3M\n", 3, "g.gfa:5: link to an undefined segment");
    }
    // any other names: through the map
    {
        const Parsed p = parse("S\tA\tACGTA\nS\t3\tGTACC\nL\t3\t-\tA\t+\t3M\nL\tA\t+\tA\t+\t3M\n", 3);
        check(!p.e && p.g.links.size() == 2 && same_link(p.g.links[0], 1, false, 0, true) &&
                  same_link(p.g.links[1], 0, true, 0, true),
              "links by name", p.e.msg);
    }
    refused("S\tA\tACGTA\nS\tB\tGTACC\nS\tA\tGTACC\n", 3, "g.gfa: segment A defined twice");
    refused("S\tA\tACGTA\nS\tB\tGTACC\nL\tA\t+\tC\t+\t3M\n", 3, "g.gfa:3: link to an undefined segment");
    refused("S\t3\tACGTA\nS\t6\tGTACC\nL\t3\t+\t5\t+\t3M\n", 3, "g.gfa:3: link to an undefined segment");  // 5 is no name here
}

HostGraph graph(const std::vector<std::string> &seqs, const std::vector<HostLink> &links = {}) {
    HostGraph g;
    for (size_t i = 0; i < seqs.size(); ++i) {
        g.names.push_back(std::to_string(3 + 2 * i));
        g.bases += seqs[i];
        g.off.push_back(g.bases.size());
    }
    g.links = links;
    return g;
}

void segments() {
    check(comp_base('A') == 'T' && comp_base('C') == 'G' && comp_base('G') == 'C' && comp_base('T') == 'A', "comp_base");
    {  // k bases are too few, k + 1 are one (k+1)-mer; the first short segment in S-line order is the one named
        const HostGraph g = graph({"ACGG", "ACG", "ACGGT", "AC"});
        SegmentTable t(4);
        const GraphError e = classify_segments(g, 3, t);
        check(e && !e.io && e.msg == "segment 5 is 3 bp: shorter than k + 1 = 4 or too long", "short segment", e.msg);
        SegmentTable t1(1);
        check(!classify_segments(graph({"ACGG"}), 3, t1) && t1.len == std::vector<uint64_t>{1} &&
                  t1.emit == std::vector<uint64_t>{0, 1} && t1.flags == std::vector<uint32_t>{0},
              "a segment of k + 1 bases");
    }
    {  // self-conjugate segments emit (L + 1) / 2 records: L = 1 and 3 at k = 3
        const HostGraph g = graph({"ACGT", "AACCG", "AACGTT", "ACGTA", "TTTAAA"});
        SegmentTable t(5);
        const GraphError e = classify_segments(g, 3, t);
        check(!e, "segments accepted", e.msg);
        check(t.len == std::vector<uint64_t>{1, 2, 3, 2, 3} && t.len32 == std::vector<uint32_t>{1, 2, 3, 2, 3}, "lengths");
        check(t.flags == std::vector<uint32_t>{kEpSelfConj, 0, kEpSelfConj, 0, kEpSelfConj}, "self-conjugate flags");
        check(t.emit == std::vector<uint64_t>{0, 1, 3, 5, 7, 9}, "emit offsets");
    }
    {  // ... and even L, which an odd k never gives a self-conjugate (even-length) segment: k = 2, L = 2 and 4
        const HostGraph g = graph({"ACGT", "AACGTT", "AACGTA"});
        SegmentTable t(3);
        check(!classify_segments(g, 2, t) && t.len == std::vector<uint64_t>{2, 4, 4} &&
                  t.flags == std::vector<uint32_t>{kEpSelfConj, kEpSelfConj, 0} &&
                  t.emit == std::vector<uint64_t>{0, 1, 3, 7},
              "emit offsets at even L");
    }
    // no string of odd length is its own reverse complement: all 4^5 of length 5
    uint32_t odd_self = 0;
    for (uint32_t v = 0; v < 1024; ++v) {
        char q[5];
        for (int i = 0; i < 5; ++i) q[i] = "ACGT"[(v >> (2 * i)) & 3];
        odd_self += segment_is_self_conjugate(q, 5) ? 1 : 0;
    }
    check(odd_self == 0, "odd length is never self-conjugate");
    check(segment_is_self_conjugate("AT", 2) && !segment_is_self_conjugate("AA", 2) && segment_is_self_conjugate("", 0),
          "self-conjugate strings");
    check(is_homopolymer_k1("CCCC", 4) && !is_homopolymer_k1("CCCA", 4) && !is_homopolymer_k1("ACCC", 4) &&
              is_homopolymer_k1("CCCA", 3),
          "is_homopolymer_k1");
}

void links() {
    // k = 3.  a = AACCG ends in CCG, rc(a) = CGGTT ends in GTT; b starts with CCG, rc(c) = CCGAA starts with CCG,
    // d starts with GTT, rc(e) = GTTCC starts with GTT
    const std::vector<std::string> seqs = {"AACCG", "CCGTA", "TTCGG", "GTTAC", "GGAAC"};
    const uint32_t a = 0, b = 1, c = 2, d = 3, e = 4;
    struct Case {
        HostLink l;
        const char *msg;  // empty: the overlap matches
    };
    const Case cases[] = {
        {{a, b, true, true}, ""},
        {{a, d, true, true}, "link 3+ -> 9+: the 3M overlap does not match the sequences"},
        {{a, c, true, false}, ""},
        {{a, e, true, false}, "link 3+ -> 11-: the 3M overlap does not match the sequences"},
        {{a, d, false, true}, ""},
        {{a, b, false, true}, "link 3- -> 5+: the 3M overlap does not match the sequences"},
        {{a, e, false, false}, ""},
        {{a, c, false, false}, "link 3- -> 7-: the 3M overlap does not match the sequences"},
    };
    for (const Case &x : cases) {
        const GraphError err = check_links(graph(seqs, {x.l}), 3);
        check(err.msg == x.msg && !err.io, std::string("one link: ") + x.msg, err.msg);
    }
    check(!check_links(graph(seqs), 3), "no links");
    // the first bad link in file order, among good ones and behind enough links to occupy every thread
    std::vector<HostLink> many(40, HostLink{a, b, true, true});
    many[17] = {a, b, false, true};
    many[23] = {a, d, true, true};
    many[39] = {a, e, true, false};
    const GraphError err = check_links(graph(seqs, many), 3);
    check(err.msg == "link 3- -> 5+: the 3M overlap does not match the sequences", "first bad link", err.msg);
}

std::vector<uint32_t> loop_flags(const std::vector<std::string> &seqs, const std::vector<HostLink> &l) {
    const HostGraph g = graph(seqs, l);
    SegmentTable t(seqs.size());
    check(!classify_segments(g, 3, t), "loop graph accepted");
    flag_loops(g, 3, t);
    return t.flags;
}

void loops() {
    // k = 3: AAAA is one homopolymer (k+1)-mer, AAAAA two of them, AAAC one that is none
    const std::vector<std::string> seqs = {"AAAA", "AAAAA", "AAAC", "CCCC"};
    check(loop_flags(seqs, {{0, 0, true, true}}) == std::vector<uint32_t>{kEpLoop1, 0, 0, 0}, "e+ -> e+ loop");
    check(loop_flags(seqs, {{3, 3, false, false}}) == std::vector<uint32_t>{0, 0, 0, kEpLoop1}, "e- -> e- loop");
    check(loop_flags(seqs, {{0, 0, true, false}, {0, 0, false, true}, {0, 3, true, true}, {3, 0, true, true}}) ==
              std::vector<uint32_t>{0, 0, 0, 0},
          "no link from the edge to itself");
    check(loop_flags(seqs, {{1, 1, true, true}}) == std::vector<uint32_t>{0, 0, 0, 0}, "two (k+1)-mers");
    check(loop_flags(seqs, {{2, 2, true, true}}) == std::vector<uint32_t>{0, 0, 0, 0}, "not a homopolymer");
    check(loop_flags(seqs, {}) == std::vector<uint32_t>{0, 0, 0, 0}, "no links");
}

void blocks() {
    const uint64_t B = 1 << 14;
    auto item = [](uint64_t i, std::string &o) { o += std::to_string(i * 7919) + (i % 3 ? "\n" : "\t\n"); };
    for (uint64_t n : {(uint64_t)0, (uint64_t)1, B - 1, B, B + 1, 3 * B + 5})
        for (uint64_t batch : {1, 2, 64})
            for (int threads : {1, 4}) {
                std::string serial, got;
                for (uint64_t i = 0; i < n; ++i) item(i, serial);
                uint64_t calls = 0;
                const bool ok = format_blocks(n, threads, batch, [&](const std::string &t) { return ++calls, got += t, true; }, item);
                check(ok && got == serial, "format_blocks: bytes at n = " + std::to_string(n));
                check(calls == (n + B - 1) / B, "format_blocks: one sink call per block", std::to_string(calls));
            }
    uint64_t calls = 0;  // a sink that fails stops the writer: 4 blocks, the second write fails
    check(!format_blocks(3 * B + 5, 4, 2, [&](const std::string &) { return ++calls < 2; }, item) && calls == 2,
          "format_blocks stops at a failed write", std::to_string(calls));
}

void files() {
    std::string text = "x";
    const GraphError e = read_whole_file("/nonexistent-dir/g.gfa", "cannot open graph %s", "reading graph %s failed", text);
    check(e && e.io && e.msg == "cannot open graph /nonexistent-dir/g.gfa", "a file that does not open", e.msg);
}

int dump(const char *path, unsigned k) {
    std::string text;
    HostGraph g;
    GraphError e = read_whole_file(path, "cannot open graph %s", "reading graph %s failed", text);
    if (!e) e = parse_gfa_text(text.data(), text.data() + text.size(), k, path, g);
    SegmentTable t(g.names.size());
    if (!e) e = classify_segments(g, k, t);
    if (!e) e = check_links(g, k);
    if (e) return std::printf("ERROR %s\n", e.msg.c_str()), 0;
    flag_loops(g, k, t);
    for (size_t s = 0; s < g.names.size(); ++s)
        std::printf("S %s %s %u %d %d\n", g.names[s].c_str(), std::string(g.seq(s), g.size(s)).c_str(), g.kc[s],
                    (t.flags[s] & kEpSelfConj) ? 1 : 0, (t.flags[s] & kEpLoop1) ? 1 : 0);
    for (const HostLink &l : g.links) std::printf("L %u %c %u %c\n", l.a, l.oa ? '+' : '-', l.b, l.ob ? '+' : '-');
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 4 && std::strcmp(argv[1], "dump") == 0) return dump(argv[2], (unsigned)std::atoi(argv[3]));
    parsing();
    segments();
    links();
    loops();
    blocks();
    files();
    if (failures) return std::fprintf(stderr, "%d check(s) failed\n", failures), 1;
    std::puts("GFA-GRAPH-OK");
    return 0;
}
