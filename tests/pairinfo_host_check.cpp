// Stand-alone program over csrc/pairinfo_host.hpp and csrc/edge_ops.h (host code only): runs the commands on stdin and
// prints what the library's host arithmetic computes, for tests/test_pairinfo_host.py to compare with the restatements.
//   stats k n, n x (key count)          -> "S <mean> <deviation> <median> <mad> <left> <right> <19 percentiles> <ok>",
//                                          doubles as the hex of their bits
//   round n, n x (d r)                  -> "R <pi_round(d, r)>" each
//   threshold n, n x (hex double)       -> "T <least_half_units>" each
//   graph ns, ns x (length self_conj)   -> sets the segment table of the commands below
//   canon n, n x (e1 e2 gap weight)     -> "P e1 e2 gap weight" per point of canonical_points, then "P end"
//   group n, n x (e1 e2 gap weight)     -> "G pe1 ...", "G pe2 ...", "G ppt ...", "G grp ..." of pair_groups
//   raw n, n x (e1 e2 gap weight)       -> "W <hex bytes>" of write_paired_index with raw_index_point
//   clustered n, n x (e1 e2 centre-bits half-units len1) -> "W <hex bytes>" with clustered_index_point
//   selfconj                            -> "C e1 e2 <pair_is_self_conj>" over every pair of edges that exist
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../spades_for_blackbird_amd/csrc/edge_ops.h"
#include "../spades_for_blackbird_amd/csrc/pairinfo_host.hpp"

using namespace bbk;

struct Stats {
    double mean = 0, deviation = 0, median = 0, mad = 0, left_quantile = 0, right_quantile = 0;
    uint64_t percentiles[19] = {};
    bool ok = false;
};

static unsigned long long bits(double x) {
    uint64_t u;
    memcpy(&u, &x, 8);
    return u;
}

static bool read_points(PairPoints &pt) {
    unsigned long long n;
    if (scanf("%llu", &n) != 1) return false;
    pt.resize(n);
    for (unsigned long long i = 0; i < n; ++i) {
        unsigned long long e1, e2, w;
        int gap;
        if (scanf("%llu %llu %d %llu", &e1, &e2, &gap, &w) != 4) return false;
        pt.e1[i] = e1;
        pt.e2[i] = e2;
        pt.gap[i] = gap;
        pt.weight[i] = w;
    }
    return true;
}

static void print_bytes(const std::string &o) {
    printf("W ");
    for (const char c : o) printf("%02x", (unsigned)(unsigned char)c);
    printf("\n");
}

static void print_row(const char *name, const std::vector<uint32_t> &v) {
    printf("G %s", name);
    for (const uint32_t x : v) printf(" %u", x);
    printf("\n");
}

int main() {
    std::vector<uint32_t> seg;
    char cmd[32];
    while (scanf("%31s", cmd) == 1) {
        const std::string c = cmd;
        if (c == "stats") {
            unsigned k;
            unsigned long long n;
            if (scanf("%u %llu", &k, &n) != 2) return 2;
            HistType hist;
            for (unsigned long long i = 0; i < n; ++i) {
                int key;
                unsigned long long cnt;
                if (scanf("%d %llu", &key, &cnt) != 2) return 2;
                hist[key] = cnt;
            }
            Stats st;
            lib_statistics(hist, k, &st);
            printf("S %016llx %016llx %016llx %016llx %016llx %016llx", bits(st.mean), bits(st.deviation), bits(st.median),
                   bits(st.mad), bits(st.left_quantile), bits(st.right_quantile));
            for (int i = 0; i < 19; ++i) printf(" %llu", (unsigned long long)st.percentiles[i]);
            printf(" %d\n", st.ok ? 1 : 0);
        } else if (c == "round") {
            unsigned long long n;
            if (scanf("%llu", &n) != 1) return 2;
            for (unsigned long long i = 0; i < n; ++i) {
                int d;
                unsigned r;
                if (scanf("%d %u", &d, &r) != 2) return 2;
                printf("R %d\n", pi_round(d, r));
            }
        } else if (c == "threshold") {
            unsigned long long n;
            if (scanf("%llu", &n) != 1) return 2;
            for (unsigned long long i = 0; i < n; ++i) {
                unsigned long long u;
                if (scanf("%llx", &u) != 1) return 2;
                double t;
                memcpy(&t, &u, 8);
                printf("T %llu\n", (unsigned long long)least_half_units(t));
            }
        } else if (c == "graph") {
            unsigned long long ns;
            if (scanf("%llu", &ns) != 1) return 2;
            seg.resize(ns);
            for (unsigned long long s = 0; s < ns; ++s) {
                unsigned len, sc;
                if (scanf("%u %u", &len, &sc) != 2) return 2;
                seg[s] = len | (sc ? kSegSelfConj : 0u);
            }
        } else if (c == "canon") {
            PairPoints in;
            if (!read_points(in)) return 2;
            const PairPoints pt = canonical_points(in.size(), in.e1.data(), in.e2.data(), in.gap.data(), in.weight.data(), seg.data());
            for (uint64_t i = 0; i < pt.size(); ++i)
                printf("P %" PRIu64 " %" PRIu64 " %d %" PRIu64 "\n", pt.e1[i], pt.e2[i], pt.gap[i], pt.weight[i]);
            printf("P end\n");
        } else if (c == "group") {
            PairPoints pt;
            if (!read_points(pt)) return 2;
            const PairGroups g = pair_groups(pt);
            print_row("pe1", g.pe1);
            print_row("pe2", g.pe2);
            print_row("ppt", g.ppt);
            print_row("grp", g.grp);
        } else if (c == "raw") {
            PairPoints pt;
            if (!read_points(pt)) return 2;
            std::string o;
            write_paired_index(o, pt.size(), [&](uint64_t i) { return raw_index_point(pt, i); });
            print_bytes(o);
        } else if (c == "clustered") {
            unsigned long long n;
            if (scanf("%llu", &n) != 1) return 2;
            std::vector<IndexPoint> rows(n);
            for (unsigned long long i = 0; i < n; ++i) {
                unsigned long long e1, e2, w, len1;
                unsigned cb;
                if (scanf("%llu %llu %x %llu %llu", &e1, &e2, &cb, &w, &len1) != 5) return 2;
                float centre;
                memcpy(&centre, &cb, 4);
                rows[i] = clustered_index_point(e1, e2, centre, w, len1);
            }
            std::string o;
            write_paired_index(o, n, [&](uint64_t i) { return rows[i]; });
            print_bytes(o);
        } else if (c == "selfconj") {
            for (uint64_t e1 = 0; e1 < 2 * seg.size(); ++e1)
                for (uint64_t e2 = 0; e2 < 2 * seg.size(); ++e2)
                    if (edge_exists(e1, seg[e1 >> 1]) && edge_exists(e2, seg[e2 >> 1]))
                        printf("C %" PRIu64 " %" PRIu64 " %d\n", e1, e2, pair_is_self_conj(e1, e2, seg.data()) ? 1 : 0);
        } else {
            return 3;
        }
    }
    printf("PAIRINFO-HOST-OK\n");
    return 0;
}
