// gfa_graph.h -- the graph of the mapping stage as plain host code: the GFA1 reader, the checks the position-local form
// of MapSequence needs (csrc/edgeprof.hip) and the block-parallel text writer.  Standard headers and OpenMP only (no HIP,
// no bbk_internal.h), so tests/gfa_graph_check.cpp builds it with g++ alone; edgeprof.hip turns a GraphError into a
// bbk::Error, host/gmapper_main.cpp takes the predicates and format_blocks, kmerprof.hip the file reader.
#pragma once

#include <sys/stat.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

namespace bbk {

// flags of a segment and of its records in the edge index (EdgePos::flags)
constexpr uint32_t kEpCanonFw = 1u;   // the canonical key is the forward window of the segment (set per record)
constexpr uint32_t kEpSelfConj = 2u;  // segment == its reverse complement
constexpr uint32_t kEpLoop1 = 4u;     // segment is one homopolymer (k+1)-mer linked to itself

// link: segment a in orientation oa (true = '+') followed by segment b in orientation ob
struct HostLink {
    uint32_t a, b;
    bool oa, ob;
};

// the graph on the host: segment names, their ACGT sequences back to back (off: n + 1 entries), links
struct HostGraph {
    std::vector<std::string> names;
    std::string bases;
    std::vector<uint64_t> off{0};
    std::vector<HostLink> links;
    std::vector<uint32_t> kc;  // KC:i: per segment (empty: none known)
    const char *seq(uint64_t s) const { return bases.data() + off[s]; }
    uint64_t size(uint64_t s) const { return off[s + 1] - off[s]; }
};

// why a graph is refused: empty msg = accepted; io = the file could not be read (BBK_ERR_IO, otherwise BBK_ERR_ARG)
struct GraphError {
    std::string msg;
    bool io = false;
    explicit operator bool() const { return !msg.empty(); }
};

template <class... A>
GraphError graph_refuse(bool io, const char *fmt, A... a) {
    char msg[1024];  // as long as the library's error text
    snprintf(msg, sizeof(msg), fmt, a...);
    return {msg, io};
}

inline char comp_base(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A'; }

// q[0, n) == its reverse complement (never at odd n: the middle base would be its own complement)
inline bool segment_is_self_conjugate(const char *q, uint64_t n) {
    for (uint64_t i = 0; i < (n + 1) / 2; ++i)
        if (q[i] != comp_base(q[n - 1 - i])) return false;
    return true;
}

// the (k+1)-mer at q is one base repeated
inline bool is_homopolymer_k1(const char *q, unsigned k1) { return std::count(q, q + k1, q[0]) == (ptrdiff_t)k1; }

// the whole file in one read; the caller's messages for a file that does not open and for a failed read (one %s: the path)
inline GraphError read_whole_file(const char *path, const char *open_msg, const char *read_msg, std::string &text) {
    FILE *f = fopen(path, "rb");
    if (!f) return graph_refuse(true, open_msg, path);
    std::unique_ptr<FILE, int (*)(FILE *)> guard(f, fclose);
    struct stat st;
    if (fstat(fileno(f), &st) != 0) return graph_refuse(true, read_msg, path);
    text.resize((size_t)st.st_size + 1);  // one fread takes a regular file and sees its end; a pipe grows the buffer
    size_t got = 0, m;
    while ((m = fread(&text[got], 1, text.size() - got, f)) > 0)
        if ((got += m) == text.size()) text.resize(2 * got);
    text.resize(got);
    if (ferror(f)) return graph_refuse(true, read_msg, path);
    return {};
}

// GFA1 S and L lines (io/graph/gfa_reader.cpp) of the text [p, end): segment names and sequences in file order,
// links with a kM overlap.  path only names the file in the messages.
inline GraphError parse_gfa_text(const char *p, const char *end, unsigned k, const char *path, HostGraph &g) {
    static const std::array<char, 256> code = [] {
        std::array<char, 256> t{};
        t['A'] = t['a'] = 'A';
        t['C'] = t['c'] = 'C';
        t['G'] = t['g'] = 'G';
        t['T'] = t['t'] = 'T';
        return t;
    }();
    struct RawLink {
        const char *a, *b;
        size_t na, nb;
        bool oa, ob;
        unsigned long long line;
    };
    std::vector<RawLink> raw;
    const std::string kM = std::to_string(k) + "M";
    g.bases.reserve((size_t)(end - p));
    const char *fs[7], *fe[7];
    for (unsigned long long lineno = 1; p < end; ++lineno) {
        const char *nl = static_cast<const char *>(memchr(p, '\n', (size_t)(end - p)));
        const char *le = nl ? nl : end;
        const char *next = nl ? nl + 1 : end;
        while (le > p && le[-1] == '\r') --le;
        if (le - p >= 2 && p[1] == '\t' && (p[0] == 'S' || p[0] == 'L')) {
            int nf = 0;
            for (const char *f = p; nf < 7;) {
                const char *t = static_cast<const char *>(memchr(f, '\t', (size_t)(le - f)));
                fs[nf] = f;
                fe[nf++] = t ? t : le;
                if (!t) break;
                f = t + 1;
            }
            auto fld = [&](int i) { return std::string(fs[i], (size_t)(fe[i] - fs[i])); };
            if (p[0] == 'S') {
                if (nf < 3) return graph_refuse(false, "%s:%llu: S line without a sequence", path, lineno);
                for (const char *c = fs[2]; c < fe[2]; ++c) {
                    const char u = code[(unsigned char)*c];
                    if (!u)
                        return graph_refuse(false, "%s:%llu: segment %s holds a base other than ACGT ('%c')", path, lineno,
                                            fld(1).c_str(), *c);
                    g.bases.push_back(u);
                }
                g.off.push_back(g.bases.size());
                g.names.push_back(fld(1));
                uint32_t kc = 0;  // the first KC:i: tag, read as the gfa library reads it (an int32; gfa_reader.cpp:65-68)
                for (const char *t = fe[2]; t + 6 <= le; ++t)
                    if (t[0] == '\t' && memcmp(t + 1, "KC:i:", 5) == 0) {
                        kc = (uint32_t)(int32_t)strtol(std::string(t + 6, (size_t)(le - t - 6)).c_str(), nullptr, 10);
                        break;
                    }
                g.kc.push_back(kc);
            } else {
                if (!(nf >= 6 && fe[2] - fs[2] == 1 && fe[4] - fs[4] == 1 && (*fs[2] == '+' || *fs[2] == '-') &&
                      (*fs[4] == '+' || *fs[4] == '-')))
                    return graph_refuse(false, "%s:%llu: malformed L line", path, lineno);
                if (fld(5) != kM)
                    return graph_refuse(false, "%s:%llu: link overlap %s, only %s (a k-overlap at k = %u) is supported", path,
                                        lineno, fld(5).c_str(), kM.c_str(), k);
                raw.push_back({fs[1], fs[3], (size_t)(fe[1] - fs[1]), (size_t)(fe[3] - fs[3]), *fs[2] == '+', *fs[4] == '+',
                               lineno});
            }
        }
        p = next;
    }
    // names: spades-gbuilder's are 3 + 2i in S-line order (graph_core.hpp:228,610-624), taken by value; others by map
    const uint64_t ns = g.names.size();
    std::unordered_map<std::string, uint32_t> id;
    bool by_value = true;
    for (uint64_t i = 0; i < ns && by_value; ++i) by_value = g.names[i] == std::to_string(3 + 2 * i);
    if (!by_value) {
        id.reserve(ns);
        for (uint64_t i = 0; i < ns; ++i)
            if (!id.emplace(g.names[i], (uint32_t)i).second)
                return graph_refuse(false, "%s: segment %s defined twice", path, g.names[i].c_str());
    }
    auto resolve = [&](const char *s, size_t n, uint32_t *out) {
        if (by_value) {
            uint64_t v = 0;
            for (size_t i = 0; i < n; ++i) {
                if (s[i] < '0' || s[i] > '9' || v > (1ull << 60)) return false;
                v = v * 10 + (uint64_t)(s[i] - '0');
            }
            if (n == 0 || (n > 1 && s[0] == '0') || v < 3 || (v & 1) == 0 || (v - 3) / 2 >= ns) return false;
            *out = (uint32_t)((v - 3) / 2);
            return true;
        }
        auto it = id.find(std::string(s, n));
        if (it == id.end()) return false;
        *out = it->second;
        return true;
    };
    g.links.resize(raw.size());
    for (size_t j = 0; j < raw.size(); ++j) {
        const RawLink &l = raw[j];
        HostLink &h = g.links[j];
        if (!resolve(l.a, l.na, &h.a) || !resolve(l.b, l.nb, &h.b))
            return graph_refuse(false, "%s:%llu: link to an undefined segment", path, l.line);
        h.oa = l.oa;
        h.ob = l.ob;
    }
    return {};
}

// per segment: len = (k+1)-mers (|seq| - k), flags (kEpSelfConj here, kEpLoop1 by flag_loops); emit = prefix sums (ns + 1
// entries) of the (k+1)-mers the index emits, (len + 1) / 2 of them for a self-conjugate segment
struct SegmentTable {
    std::vector<uint64_t> len, emit;
    std::vector<uint32_t> len32, flags;
    explicit SegmentTable(uint64_t ns) : len(ns), emit(ns + 1), len32(ns), flags(ns) {}
};

// refuses the first segment (S-line order) shorter than k + 1 bases or too long for 32-bit offsets
inline GraphError classify_segments(const HostGraph &g, unsigned k, SegmentTable &t) {
    const uint64_t ns = g.names.size();
    int64_t bad = -1;
#pragma omp parallel for schedule(static) num_threads(16)
    for (int64_t s = 0; s < (int64_t)ns; ++s) {
        const uint64_t n = g.size(s);
        if (n < k + 1 || n - k >= (1ull << 32) - 1) {
#pragma omp critical
            bad = bad < 0 || s < bad ? s : bad;
            continue;
        }
        const uint64_t L = n - k;
        t.len[s] = L;
        t.len32[s] = (uint32_t)L;
        const bool selfc = segment_is_self_conjugate(g.seq(s), n);
        if (selfc) t.flags[s] |= kEpSelfConj;
        t.emit[s + 1] = selfc ? (L + 1) / 2 : L;
    }
    if (bad >= 0)
        return graph_refuse(false, "segment %s is %llu bp: shorter than k + 1 = %u or too long", g.names[bad].c_str(),
                            (unsigned long long)g.size(bad), k + 1);
    for (uint64_t s = 0; s < ns; ++s) t.emit[s + 1] += t.emit[s];
    return {};
}

// a link is a true k-overlap: the last k bases of a (as oriented) are the first k bases of b.  Refuses the first link
// (file order) that is not.  The segments hold at least k bases (classify_segments).
inline GraphError check_links(const HostGraph &g, unsigned k) {
    const int64_t nl = (int64_t)g.links.size();
    int64_t bad = -1;
#pragma omp parallel for schedule(static) num_threads(16)
    for (int64_t j = 0; j < nl; ++j) {
        const HostLink &l = g.links[j];
        const char *A = g.seq(l.a), *B = g.seq(l.b);
        const uint64_t la = g.size(l.a), lb = g.size(l.b);
        bool ok = true;
        for (unsigned i = 0; i < k && ok; ++i)
            ok = (l.oa ? A[la - k + i] : comp_base(A[k - 1 - i])) == (l.ob ? B[i] : comp_base(B[lb - 1 - i]));
        if (!ok) {
#pragma omp critical
            bad = bad < 0 || j < bad ? j : bad;
        }
    }
    if (bad < 0) return {};
    const HostLink &l = g.links[bad];
    return graph_refuse(false, "link %s%c -> %s%c: the %uM overlap does not match the sequences", g.names[l.a].c_str(),
                        l.oa ? '+' : '-', g.names[l.b].c_str(), l.ob ? '+' : '-', k);
}

// kEpLoop1: a link e+ -> e+ (or e- -> e-) on a segment that is one homopolymer (k+1)-mer
inline void flag_loops(const HostGraph &g, unsigned k, SegmentTable &t) {
    for (const HostLink &l : g.links)
        if (l.a == l.b && l.oa == l.ob && t.len[l.a] == 1 && is_homopolymer_k1(g.seq(l.a), k + 1)) t.flags[l.a] |= kEpLoop1;
}

// Text of n items, formatted 2^14 items per task by `threads` threads and handed to sink block by block in item order,
// `batch` blocks at a time (the bytes do not depend on threads or batch).  fmt(i, std::string &) appends item i;
// sink(const std::string &) returns false to stop (a short write), and so does format_blocks then.
template <class Sink, class Fmt>
bool format_blocks(uint64_t n, int threads, uint64_t batch, Sink &&sink, Fmt &&fmt) {
    constexpr uint64_t kBlock = 1 << 14;
    const uint64_t nb = (n + kBlock - 1) / kBlock;
    for (uint64_t b0 = 0; b0 < nb; b0 += batch) {
        const uint64_t b1 = std::min(nb, b0 + batch);
        std::vector<std::string> text(b1 - b0);
#pragma omp parallel for num_threads(threads) schedule(dynamic, 1)
        for (int64_t b = (int64_t)b0; b < (int64_t)b1; ++b)
            for (uint64_t i = (uint64_t)b * kBlock; i < std::min(n, (uint64_t)(b + 1) * kBlock); ++i)
                fmt(i, text[(size_t)(b - (int64_t)b0)]);
        for (const std::string &t : text)
            if (!sink(t)) return false;
    }
    return true;
}

}  // namespace bbk
