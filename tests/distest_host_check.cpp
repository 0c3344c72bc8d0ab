// Stand-alone program over csrc/distest_host.hpp (host code only): reads a graph and queries from stdin, prints what the
// library's host path computes, for tests/test_distest_restated.py to compare with the restatement.
//   in:  k ns nl U nq, then ns x (length self_conjugate kc), nl x (a a_plus b b_plus), nq x (e1 e2 min_len)
//   out: "E <end> <start>" per oriented edge that exists ("E - -" otherwise), then per query
//        "Q <ball> <calls> <length> ..." (walk lengths, ascending)
#include <cstdio>
#include <vector>

#include "../spades_for_blackbird_amd/csrc/distest_host.hpp"

int main() {
    unsigned k;
    unsigned long long ns, nl, U, nq;
    if (scanf("%u %llu %llu %llu %llu", &k, &ns, &nl, &U, &nq) != 5) return 2;
    std::vector<uint32_t> seg(ns), kc(ns), links(4 * nl + 1);
    for (unsigned long long s = 0; s < ns; ++s) {
        unsigned len, sc, c;
        if (scanf("%u %u %u", &len, &sc, &c) != 3) return 2;
        seg[s] = len | (sc ? bbk::kSegSelfConj : 0u);
        kc[s] = c;
    }
    for (unsigned long long j = 0; j < 4 * nl; ++j)
        if (scanf("%u", &links[j]) != 1) return 2;
    bbk::DeGraph g;
    bbk::de_build_graph(k, ns, seg.data(), links.data(), nl, kc.data(), g);
    for (uint32_t e = 0; e < 2 * ns; ++e) {
        if (g.exists(e)) printf("E %u %u\n", g.end[e], g.start[e]);
        else printf("E - -\n");
    }
    bbk::DeSearch s(g);
    long long last = -1;
    std::vector<uint32_t> row((U >> 5) + 1);
    for (unsigned long long q = 0; q < nq; ++q) {
        unsigned e1, e2;
        unsigned long long min_len;
        if (scanf("%u %u %llu", &e1, &e2, &min_len) != 3) return 2;
        if ((long long)e1 != last) s.dijkstra(g.end[e1], U);
        last = e1;
        std::fill(row.begin(), row.end(), 0u);
        const uint64_t calls = s.lengths(g.end[e1], g.start[e2], min_len, row.data());
        printf("Q %zu %llu", s.dist.size(), (unsigned long long)calls);
        for (unsigned long long l = 0; l <= U; ++l)
            if (row[l >> 5] >> (l & 31) & 1) printf(" %llu", l);
        printf("\n");
    }
    printf("DISTEST-HOST-OK\n");
    return 0;
}
