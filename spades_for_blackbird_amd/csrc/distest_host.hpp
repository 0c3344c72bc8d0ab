// distest_host.hpp -- the host side of the distance-estimation stage (csrc/distest.hip) as plain C++: the graph as the
// reference's reader links it, and the literal search of GraphDistanceFinder for the pairs the device leaves to the host.
// Standard headers only (no HIP, no bbk_internal.h), as readcorrect_host.hpp is for the corrector, so a stand-alone
// program can build it with g++ alone.  The rules of an edge (conjugate, length, existence) and the lower bound of a path
// length are edge_ops.h's; the weight threshold and the grouping of the points are pairinfo_host.hpp's.
//
//   DeGraph / de_build_graph   GFAReader::to_graph (io/graph/gfa_reader.cpp:54-148) over the kept L lines: segment i is
//                              edge 2i and its conjugate 2i + 1 (a self-conjugate segment is the one edge 2i), the numbering
//                              of bbk_path_range.edge; vertex 4i is the end of 2i, 4i + 2 the end of 2i + 1, conj v = v ^ 1;
//                              LinkEdges moves the start of e2 onto the end of e1 (construction_helper.hpp:95-99).  The
//                              rule is Graph.end / start of tests/gmapper_restated.py.
//   DeSearch::dijkstra         DijkstraHelper::CreateBoundedDijkstra(g, U, 3000).Run(EdgeEnd(e1))
//   DeSearch::lengths          PathProcessor::Traversal::Go with DistancesLengthsCallback (path_processor.hpp:56-181,
//                              380-402).  Incoming edges go by ascending (Dijkstra distance, -coverage); ties go by
//                              ascending edge number (stable sort over IncomingEdges order), the declared deviation of
//                              tests/distest_restated.py: the reference's edge ids are not reproducible here.
#pragma once

#include <algorithm>
#include <cstdint>
#include <functional>
#include <queue>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "edge_ops.h"

namespace bbk {

constexpr uint64_t kDeMaxCalls = 3000, kDeMaxVertices = 3000, kDeUsageThreshold = 500, kDeMaxUsage = 5;

struct DeGraph {
    unsigned k = 0;
    uint64_t ns = 0;
    std::vector<uint32_t> seg;             // (k+1)-mers of the segment | kSegSelfConj (edge_ops.h)
    std::vector<uint32_t> kc;              // KC:i: of the segment
    std::vector<uint32_t> end, start;      // per oriented edge (2 * ns; an edge that does not exist holds 0)
    std::vector<uint32_t> out_off, out_e;  // per vertex (4 * ns + 1): the edges that start there, ascending

    bool selfc(uint32_t e) const { return edge_self_conj(seg[e >> 1]); }
    bool exists(uint32_t e) const { return edge_exists(e, seg[e >> 1]); }
    uint32_t conj(uint32_t e) const { return edge_conj(e, seg[e >> 1]); }
    uint64_t length(uint32_t e) const { return edge_length(seg[e >> 1]); }
    double coverage(uint32_t e) const { return (double)kc[e >> 1] / (double)length(e); }
};

// links: 4 x u32 per L line in file order (a, a is '+', b, b is '+')
inline void de_build_graph(unsigned k, uint64_t ns, const uint32_t *seg, const uint32_t *links, uint64_t nl,
                           const uint32_t *kc, DeGraph &g) {
    g.k = k;
    g.ns = ns;
    g.seg.assign(seg, seg + ns);
    g.kc.assign(kc, kc + ns);
    const uint64_t nx = 2 * ns, nv = 4 * ns;
    g.end.assign(nx, 0);
    for (uint64_t s = 0; s < ns; ++s) {
        g.end[2 * s] = (uint32_t)(4 * s);
        if (!g.selfc((uint32_t)(2 * s))) g.end[2 * s + 1] = (uint32_t)(4 * s + 2);
    }
    typedef std::pair<uint32_t, uint32_t> Arc;  // over oriented segments x = 2 * segment + (x is '-')
    std::vector<Arc> arcs(nl);
    for (uint64_t j = 0; j < nl; ++j)
        arcs[j] = {(uint32_t)(2 * links[4 * j] + (links[4 * j + 1] ? 0 : 1)),
                   (uint32_t)(2 * links[4 * j + 2] + (links[4 * j + 3] ? 0 : 1))};
    std::vector<uint64_t> first, order;
    auto group = [&](const std::vector<Arc> &a) {  // stable by source
        first.assign(nx + 1, 0);
        for (const Arc &x : a) ++first[x.first + 1];
        for (uint64_t v = 0; v < nx; ++v) first[v + 1] += first[v];
        std::vector<uint64_t> fill(first.begin(), first.end() - 1);
        order.resize(a.size());
        for (uint64_t j = 0; j < a.size(); ++j) order[fill[a[j].first]++] = j;
    };
    group(arcs);
    std::vector<uint8_t> is_comp(nl, 0);
    std::vector<Arc> all(arcs);
    for (uint64_t v = 0; v < nx; ++v)  // gfa_fix_symm: the complement of every L line that has none in the file
        for (uint64_t i = first[v]; i < first[v + 1]; ++i) {
            const uint64_t j = order[i];
            if (is_comp[j]) continue;
            const uint32_t w = arcs[j].second;
            bool found = false;
            for (uint64_t i2 = first[w ^ 1u]; i2 < first[(w ^ 1u) + 1] && !found; ++i2) {
                const uint64_t j2 = order[i2];
                if (!is_comp[j2] && arcs[j2].second == ((uint32_t)v ^ 1u)) {
                    is_comp[j2] = 1;
                    found = true;
                }
            }
            if (!found) all.push_back({w ^ 1u, (uint32_t)v ^ 1u});
        }
    group(all);
    for (uint64_t j : order) {  // LinkEdges(e1, e2)
        const uint32_t e1 = g.selfc(all[j].first) ? (all[j].first & ~1u) : all[j].first;
        const uint32_t e2 = g.selfc(all[j].second) ? (all[j].second & ~1u) : all[j].second;
        g.end[g.conj(e2)] = g.end[e1] ^ 1u;
    }
    g.start.assign(nx, 0);
    g.out_off.assign(nv + 1, 0);
    for (uint32_t e = 0; e < nx; ++e)
        if (g.exists(e)) {
            g.start[e] = g.end[g.conj(e)] ^ 1u;
            ++g.out_off[g.start[e] + 1];
        }
    for (uint64_t v = 0; v < nv; ++v) g.out_off[v + 1] += g.out_off[v];
    g.out_e.resize(g.out_off[nv]);
    std::vector<uint32_t> fill(g.out_off.begin(), g.out_off.end() - 1);
    for (uint32_t e = 0; e < nx; ++e)
        if (g.exists(e)) g.out_e[fill[g.start[e]]++] = e;
}

struct DeSearch {
    const DeGraph &g;
    std::unordered_map<uint32_t, uint64_t> dist, usage;
    uint64_t len = 0, calls = 0, min_len = 0, bound = 0;
    uint32_t from = 0;
    uint32_t *row = nullptr;
    explicit DeSearch(const DeGraph &graph) : g(graph) {}

    // queue order (distance, vertex, previous vertex, edge) as ReverseDistanceComparator (dijkstra_algorithm.hpp)
    void dijkstra(uint32_t s, uint64_t U) {
        dist.clear();
        bound = U;
        typedef std::tuple<uint64_t, int64_t, int64_t, int64_t> El;
        std::priority_queue<El, std::vector<El>, std::greater<El>> q;
        q.emplace(0, (int64_t)s, -1, -1);
        uint64_t n = 0;
        while (!q.empty()) {
            const El t = q.top();
            q.pop();
            const uint64_t d = std::get<0>(t);
            const uint32_t v = (uint32_t)std::get<1>(t);
            if (!dist.emplace(v, d).second) continue;
            ++n;
            if (n > kDeMaxVertices || !(n < kDeMaxVertices && d <= U)) continue;
            for (uint32_t i = g.out_off[v]; i < g.out_off[v + 1]; ++i) {
                const uint32_t e = g.out_e[i], w = g.end[e];
                const uint64_t nd = d + g.length(e);
                if (!dist.count(w) && nd <= U) q.emplace(nd, (int64_t)w, (int64_t)v, (int64_t)e);
            }
        }
    }

    bool go(uint32_t v) {  // true: the call limit was reached
        if (++calls >= kDeMaxCalls) return true;
        if (v == from && len >= min_len) row[len >> 5] |= 1u << (len & 31);
        std::vector<uint32_t> inc;
        for (uint32_t i = g.out_off[v ^ 1u]; i < g.out_off[(v ^ 1u) + 1]; ++i) {
            const uint32_t e = g.conj(g.out_e[i]);
            if (dist.count(g.start[e])) inc.push_back(e);
        }
        std::stable_sort(inc.begin(), inc.end(), [&](uint32_t a, uint32_t b) {
            const uint64_t da = dist.at(g.start[a]), db = dist.at(g.start[b]);
            if (da != db) return da < db;
            return g.coverage(a) > g.coverage(b);
        });
        for (const uint32_t e : inc) {
            const uint32_t s = g.start[e];
            if (dist.at(s) + g.length(e) + len > bound) continue;
            if (calls >= kDeUsageThreshold && usage[s] >= kDeMaxUsage) continue;
            len += g.length(e);
            ++usage[s];
            const bool stop = go(s);
            --usage[s];
            len -= g.length(e);
            if (stop) return true;
        }
        return false;
    }

    // after dijkstra(EdgeEnd(e1), U): bit l of out_row (zeroed, (U >> 5) + 1 words) for every walk length l the search
    // from EdgeStart(e2) = to finds; returns the calls it made
    uint64_t lengths(uint32_t from_v, uint32_t to, uint64_t min_length, uint32_t *out_row) {
        calls = 0;
        const auto it = dist.find(to);
        if (it == dist.end() || it->second > bound) return 0;
        from = from_v;
        min_len = min_length;
        row = out_row;
        len = 0;
        usage.clear();
        usage[to] = 1;
        go(to);
        return calls;
    }
};

}  // namespace bbk
