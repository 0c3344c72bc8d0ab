// unitigs_write.hip -- a unitig set as a file: GFA (formatted on the device or on the host), FASTG, FASTA and the
// SPAdes binary graph.
//
// Replaces io/graph/gfa_writer.cpp:18-52, io/graph/fastg_writer.cpp:20-47, projects/gbuilder/main.cpp:183-192 and
// io/binary/graph.hpp:27-46 + coverage.hpp:24-29 of the reference.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <omp.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bbk_internal.h"
#include "unitigs.h"

namespace bbk {

// ---- the pieces of the text formats, each spelled once -----------------------------------------------------------
__host__ __device__ inline uint32_t dec_len(uint64_t v) {
    uint32_t n = 1;
    while (v >= 10) {
        v /= 10;
        ++n;
    }
    return n;
}
__host__ __device__ inline void put_dec(char *dst, uint64_t v, uint32_t len) {
    for (uint32_t i = 0; i < len; ++i) {
        dst[len - 1 - i] = (char)('0' + v % 10);
        v /= 10;
    }
}

// Segment i is named 3 + 2i (graph_core.hpp:228; edge i gets min_id + 2i, debruijn_graph_constructor.hpp:457-458).
__host__ __device__ inline uint64_t gfa_id(uint64_t i) { return 3 + 2 * i; }

// "S\t<id>\t": the head of a segment line, followed by the bases and the tail
__host__ __device__ inline uint32_t gfa_s_head_len(uint64_t i) { return 3 + dec_len(gfa_id(i)); }
__host__ __device__ inline void gfa_s_head_put(char *d, uint64_t i, uint32_t head_len) {
    d[0] = 'S';
    d[1] = '\t';
    put_dec(d + 2, gfa_id(i), head_len - 3);
    d[head_len - 1] = '\t';
}
#define BBK_GFA_TAIL0 "\tDP:f:0\tKC:i:0\n"  // the tail without coverage
constexpr uint32_t kGfaTail = sizeof(BBK_GFA_TAIL0) - 1;

// "L\t<e1>\t<+|->\t<e2>\t<+|->\t<k>M\n" of the link (a, b), a = edge << 1 | is '+'; klen = dec_len(k)
__host__ __device__ inline uint64_t gfa_l_len(uint64_t a, uint64_t b, uint32_t klen) {
    return 2 + dec_len(gfa_id(a >> 1)) + 3 + dec_len(gfa_id(b >> 1)) + 3 + klen + 2;
}
__host__ __device__ inline void gfa_l_put(char *d, uint64_t a, uint64_t b, uint32_t k, uint32_t klen) {
    const uint64_t ia = gfa_id(a >> 1), ib = gfa_id(b >> 1);
    const uint32_t la = dec_len(ia), lb = dec_len(ib);
    *d++ = 'L';
    *d++ = '\t';
    put_dec(d, ia, la);
    d += la;
    *d++ = '\t';
    *d++ = (a & 1u) ? '+' : '-';
    *d++ = '\t';
    put_dec(d, ib, lb);
    d += lb;
    *d++ = '\t';
    *d++ = (b & 1u) ? '+' : '-';
    *d++ = '\t';
    put_dec(d, k, klen);
    d += klen;
    *d++ = 'M';
    *d++ = '\n';
}

// ---- GFA text on the device ------------------------------------------------------------------
__global__ void k_gfa_s_len(const uint64_t *__restrict__ uoff, uint64_t nu, uint64_t *__restrict__ len) {
    const uint64_t i = BBK_GID();
    if (i < nu) len[i] = gfa_s_head_len(i) + (uoff[i + 1] - uoff[i]) + kGfaTail;
}

// one wavefront per segment line: "S\t<3+2i>\t<bases>\tDP:f:0\tKC:i:0\n"
__global__ __launch_bounds__(256) void k_gfa_s_write(const char *__restrict__ bases, const uint64_t *__restrict__ uoff,
                                                    const uint64_t *__restrict__ pos, uint64_t nu,
                                                    char *__restrict__ out) {
    const uint64_t i = (BBK_GID()) >> 6;
    if (i >= nu) return;
    const int lane = threadIdx.x & 63;
    char *d = out + pos[i];
    const uint32_t hl = gfa_s_head_len(i);
    if (lane == 0) gfa_s_head_put(d, i, hl);
    const uint64_t b0 = uoff[i], len = uoff[i + 1] - b0;
    char *sq = d + hl;
    for (uint64_t j = lane; j < len; j += 64) sq[j] = bases[b0 + j];
    if (lane < (int)kGfaTail) sq[len + lane] = BBK_GFA_TAIL0[lane];
}

__global__ void k_gfa_l_len(const uint64_t *__restrict__ links, uint64_t nl, uint32_t klen, uint64_t *__restrict__ len) {
    const uint64_t l = BBK_GID();
    if (l < nl) len[l] = gfa_l_len(links[2 * l], links[2 * l + 1], klen);
}

__global__ void k_gfa_l_write(const uint64_t *__restrict__ links, const uint64_t *__restrict__ pos, uint64_t nl,
                              uint32_t k, uint32_t klen, char *__restrict__ out) {
    const uint64_t l = BBK_GID();
    if (l < nl) gfa_l_put(out + pos[l], links[2 * l], links[2 * l + 1], k, klen);
}

// GFA text formatted on the device from the device copy, then streamed to the file in
// pinned chunks (copy of chunk i+1 overlaps the pwrite of chunk i).
static void write_gfa_device(bbk_ctx *ctx, const bbk_unitigs *u, const char *path) {
    BBK_HIP(hipSetDevice(ctx->device));
    const uint64_t nu = u->n, nl = u->n_links;
    DevBuf spos((nu + 1) * 8), lpos((nl + 1) * 8);
    uint64_t sbytes = 0, lbytes = 0;
    if (nu) {
        launch_items(ctx, "k_gfa_s_len", k_gfa_s_len, nu, u->d_uoff.as<uint64_t>(), nu, spos.as<uint64_t>());
        sbytes = exclusive_scan_u64(ctx, spos.as<uint64_t>(), spos.as<uint64_t>(), nu);
    }
    const uint32_t klen = dec_len(u->k);
    if (nl) {
        launch_items(ctx, "k_gfa_l_len", k_gfa_l_len, nl, u->d_links.as<uint64_t>(), nl, klen, lpos.as<uint64_t>());
        lbytes = exclusive_scan_u64(ctx, lpos.as<uint64_t>(), lpos.as<uint64_t>(), nl);
    }
    const uint64_t total = sbytes + lbytes;
    DevBuf text(total + 16);
    {
        KernelTimer t(ctx, "gfa_text", (double)total + (double)u->total_bases);
        if (nu) {
            launch_items(ctx, "k_gfa_s_write", k_gfa_s_write, nu * 64, u->d_bases.as<char>(), u->d_uoff.as<uint64_t>(),
                         spos.as<uint64_t>(), nu, text.as<char>());
        }
        if (nl) {
            launch_items(ctx, "k_gfa_l_write", k_gfa_l_write, nl, u->d_links.as<uint64_t>(), lpos.as<uint64_t>(), nl,
                         (uint32_t)u->k, klen, text.as<char>() + sbytes);
        }
    }
    const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    BBK_REQUIRE(fd >= 0, BBK_ERR_IO, "cannot open %s for writing", path);
    const bool ok = d2f_big(ctx, fd, 0, text.p, (size_t)total);
    const int cl = close(fd);
    BBK_REQUIRE(ok && cl == 0, BBK_ERR_IO, "short write to %s", path);
}

// ---- host side ---------------------------------------------------------------------------------------------------
// host worker threads for text formatting / file writes: the box may expose hundreds of logical CPUs
// of which only a share is ours
static int host_threads() { return std::max(1, std::min(omp_get_max_threads(), 32)); }

// parallel positional writes of one buffer (tmpfs / NVMe scale with writers; a single fwrite of
// 1.5 GB is a third of the whole GFA time otherwise)
static bool pwrite_all(int fd, const char *buf, size_t bytes, off_t base) {
    const size_t chunk = 16ull << 20;
    const size_t nchunks = (bytes + chunk - 1) / chunk;
    bool ok = true;
#pragma omp parallel for schedule(dynamic, 1) num_threads(host_threads())
    for (size_t c = 0; c < nchunks; ++c) {
        size_t off = c * chunk;
        const size_t end = std::min(bytes, off + chunk);
        while (off < end) {
            const ssize_t w = pwrite(fd, buf + off, end - off, base + (off_t)off);
            if (w <= 0) {
#pragma omp atomic write
                ok = false;
                break;
            }
            off += (size_t)w;
        }
    }
    return ok;
}

// line lengths -> offsets (two-level parallel prefix sum): v[i + 1] holds the length of item i on entry and the end of
// item i on return; v[0] = 0
static void prefix_sum(raw_vector<uint64_t> &v, uint64_t cnt) {
    const int T = host_threads();
    std::vector<uint64_t> part((size_t)T + 1, 0);
#pragma omp parallel num_threads(T)
    {
        const int t = omp_get_thread_num();
        const uint64_t lo = cnt * (uint64_t)t / T, hi = cnt * (uint64_t)(t + 1) / T;
        uint64_t sacc = 0;
        for (uint64_t i = lo; i < hi; ++i) sacc += v[i + 1];
        part[(size_t)t + 1] = sacc;
#pragma omp barrier
#pragma omp single
        for (int j = 0; j < T; ++j) part[(size_t)j + 1] += part[(size_t)j];
        uint64_t run = part[(size_t)t];
        for (uint64_t i = lo; i < hi; ++i) {
            run += v[i + 1];
            v[i + 1] = run;
        }
    }
}

// s == rc(s): the edge is its own conjugate
static bool is_self_rc(const char *s, uint64_t len) {
    for (uint64_t a = 0; a < len; ++a)
        if (s[a] != complement(s[len - 1 - a])) return false;
    return true;
}

// a sequence in lines of 60 columns (osequencestream.hpp:22-28)
static bool put_wrapped60(FILE *f, const char *s, uint64_t len) {
    bool ok = true;
    for (uint64_t cur = 0; cur < len && ok; cur += 60) {
        const uint64_t w = std::min<uint64_t>(60, len - cur);
        ok = fwrite(s + cur, 1, w, f) == w && fputc('\n', f) != EOF;
    }
    return ok;
}

static uint64_t unitig_len(const bbk_unitigs *u, uint64_t i) { return u->offsets[i + 1] - u->offsets[i]; }

// The S lines of a host result.  Tail "\tDP:f:<float(KC/(len-k))>\tKC:i:<KC>\n": default ostream formatting of a
// float is %g with 6 significant digits (gfa_writer.cpp:18-25; coverage = raw / length, coverage.hpp:58-64);
// coverage is 0 without -c.
static raw_vector<char> gfa_s_lines_host(const bbk_unitigs *u) {
    const uint64_t n = u->n;
    std::vector<std::string> tails;
    if (u->has_cov) {
        tails.resize(n);
#pragma omp parallel for schedule(static) num_threads(host_threads())
        for (uint64_t i = 0; i < n; ++i) {
            const double cov = (double)u->kc[i] / (double)(unitig_len(u, i) - u->k);
            char b[96];
            snprintf(b, sizeof(b), "\tDP:f:%g\tKC:i:%llu\n", (double)(float)cov, (unsigned long long)u->kc[i]);
            tails[i] = b;
        }
    }
    raw_vector<uint64_t> pos(n + 1);
    pos[0] = 0;
#pragma omp parallel for schedule(static) num_threads(host_threads())
    for (uint64_t i = 0; i < n; ++i)
        pos[i + 1] = gfa_s_head_len(i) + unitig_len(u, i) + (u->has_cov ? tails[i].size() : kGfaTail);
    prefix_sum(pos, n);
    raw_vector<char> buf(pos[n]);
#pragma omp parallel for schedule(static) num_threads(host_threads())
    for (uint64_t i = 0; i < n; ++i) {
        char *d = buf.data() + pos[i];
        const uint32_t hl = gfa_s_head_len(i);
        gfa_s_head_put(d, i, hl);
        const uint64_t len = unitig_len(u, i);
        memcpy(d + hl, u->bases.data() + u->offsets[i], len);
        if (u->has_cov) memcpy(d + hl + len, tails[i].data(), tails[i].size());
        else memcpy(d + hl + len, BBK_GFA_TAIL0, kGfaTail);
    }
    return buf;
}

static raw_vector<char> gfa_l_lines_host(const bbk_unitigs *u) {
    const uint64_t nl = u->n_links;
    const uint32_t kl = dec_len(u->k);
    raw_vector<uint64_t> lpos(nl + 1);
    lpos[0] = 0;
#pragma omp parallel for schedule(static) num_threads(host_threads())
    for (uint64_t l = 0; l < nl; ++l) lpos[l + 1] = gfa_l_len(u->links[2 * l], u->links[2 * l + 1], kl);
    prefix_sum(lpos, nl);
    raw_vector<char> lbuf(lpos[nl]);
#pragma omp parallel for schedule(static) num_threads(host_threads())
    for (uint64_t l = 0; l < nl; ++l) gfa_l_put(lbuf.data() + lpos[l], u->links[2 * l], u->links[2 * l + 1], u->k, kl);
    return lbuf;
}

static void write_gfa_host(bbk_ctx *ctx, const bbk_unitigs *u, const char *path) {
    ensure_host(ctx, u);
    const bool verbose = getenv("BBK_VERBOSE") != nullptr;
    double t_prev = omp_get_wtime();
    auto lap = [&](const char *what) {
        if (verbose) {
            const double t = omp_get_wtime();
            fprintf(stderr, "[bbk] write_gfa %-10s %.3f s\n", what, t - t_prev);
            t_prev = t;
        }
    };
    const raw_vector<char> buf = gfa_s_lines_host(u);
    lap("S-format");
    const raw_vector<char> lbuf = gfa_l_lines_host(u);
    lap("L-format");
    const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    BBK_REQUIRE(fd >= 0, BBK_ERR_IO, "cannot open %s for writing", path);
    bool ok = pwrite_all(fd, buf.data(), buf.size(), 0) && pwrite_all(fd, lbuf.data(), lbuf.size(), (off_t)buf.size());
    const int cl = close(fd);
    lap("pwrite");
    BBK_REQUIRE(ok && cl == 0, BBK_ERR_IO, "short write to %s", path);
}

// FastgWriter::WriteSegmentsAndLinks (common/io/graph/fastg_writer.cpp:20-47): one FASTA record per
// edge AND per conjugate edge; header = name, ':' + comma-separated names of the edges leaving its end
// vertex (a std::set, i.e. sorted as strings), ';'.  Names are BasicNamingF
// (io/utils/edge_namer.hpp:33-38): EDGE_<id>_length_<len>_cov_<to_string(cov)>, a conjugate edge is
// the canonical name + "'" (extended_namer_, fastg_writer.hpp:30).  Record order in the reference
// follows its vertex numbering (BooPHF order); here: edge id order, the edge before its conjugate.
static void write_fastg(bbk_ctx *ctx, const bbk_unitigs *u, const char *path) {
    ensure_host(ctx, u);
    const uint64_t n = u->n;
    std::vector<uint8_t> selfconj(n, 0);
#pragma omp parallel for schedule(static) num_threads(host_threads())
    for (uint64_t i = 0; i < n; ++i) selfconj[i] = is_self_rc(u->bases.data() + u->offsets[i], unitig_len(u, i));
    auto flip = [&](uint64_t t) { return selfconj[t >> 1] ? t : (t ^ 1ull); };
    // adjacency of oriented edges: a stored link x -> y also means rc(y) -> rc(x)
    std::vector<std::pair<uint64_t, uint64_t>> adj;
    adj.reserve(2 * u->n_links);
    for (uint64_t l = 0; l < u->n_links; ++l) {
        const uint64_t x = u->links[2 * l], y = u->links[2 * l + 1];
        adj.emplace_back(x, y);
        adj.emplace_back(flip(y), flip(x));
    }
    std::sort(adj.begin(), adj.end());
    adj.erase(std::unique(adj.begin(), adj.end()), adj.end());
    auto name = [&](uint64_t t) {
        const uint64_t i = t >> 1, len = unitig_len(u, i);
        const double cov = u->has_cov ? (double)u->kc[i] / (double)(len - u->k) : 0.0;
        std::string s = "EDGE_" + std::to_string(gfa_id(i)) + "_length_" + std::to_string(len) + "_cov_" +
                        std::to_string(cov);
        if (!(t & 1ull)) s += "'";
        return s;
    };
    FILE *f = fopen(path, "wb");
    BBK_REQUIRE(f != nullptr, BBK_ERR_IO, "cannot open %s for writing", path);
    bool ok = true;
    std::string seq, hdr;
    for (uint64_t i = 0; i < n && ok; ++i) {
        for (int o = 1; o >= 0 && ok; --o) {
            if (o == 0 && selfconj[i]) continue;
            const uint64_t t = (i << 1) | (uint64_t)o;
            // successors of t: adj is sorted by (from, to); orientation '-' (0) sorts before '+' (1)
            auto lo = std::lower_bound(adj.begin(), adj.end(), std::make_pair(t, (uint64_t)0));
            std::vector<std::string> next;
            for (auto it = lo; it != adj.end() && it->first == t; ++it) next.push_back(name(it->second));
            std::sort(next.begin(), next.end());
            hdr = ">" + name(t);
            const char *delim = ":";
            for (const std::string &nx : next) {
                hdr += delim;
                hdr += nx;
                delim = ",";
            }
            hdr += ";\n";
            const char *sq = u->bases.data() + u->offsets[i];
            seq.assign(sq, sq + unitig_len(u, i));
            if (o == 0) seq = str_rc(seq);
            ok = fwrite(hdr.data(), 1, hdr.size(), f) == hdr.size() && put_wrapped60(f, seq.data(), seq.size());
        }
    }
    const int cl = fclose(f);
    BBK_REQUIRE(ok && cl == 0, BBK_ERR_IO, "short write to %s", path);
}

// >EDGE_<i+1>_length_<len> + 60-column wrapped sequence (projects/gbuilder/main.cpp:183-192,
// io/reads/header_naming.hpp:14-20)
static void write_fasta(bbk_ctx *ctx, const bbk_unitigs *u, const char *path) {
    ensure_host(ctx, u);
    FILE *f = fopen(path, "wb");
    BBK_REQUIRE(f != nullptr, BBK_ERR_IO, "cannot open %s for writing", path);
    bool ok = true;
    for (uint64_t i = 0; i < u->n && ok; ++i) {
        const uint64_t len = unitig_len(u, i);
        ok = fprintf(f, ">EDGE_%llu_length_%llu\n", (unsigned long long)(i + 1), (unsigned long long)len) > 0 &&
             put_wrapped60(f, u->bases.data() + u->offsets[i], len);
    }
    const int cl = fclose(f);
    BBK_REQUIRE(ok && cl == 0, BBK_ERR_IO, "short write to %s", path);
}

// SPAdes binary graph: <basename>.grseq (io::binary::GraphIO::SaveImpl, common/io/binary/graph.hpp:27-46) +
// <basename>.cvr (BaseCoverageIO::SaveImpl, common/io/binary/coverage.hpp:24-29), what `spades-gbuilder --spades`
// writes through BasicGraphIO::Save (common/io/binary/basic.hpp:24-27, projects/gbuilder/main.cpp:221-222).
//   .grseq: u64 vreserved, u64 ereserved, u64 vertex_count; per vertex (id order): u64 id, u64 conjugate id, then per
//           outgoing edge e1 with conj(e1) >= e1: u64 e1, u64 e2 = conj(e1), u64 EdgeEnd(e1), u64 EdgeStart(e2),
//           Sequence (u64 length + ceil(length/32) u64 words, 2 bits per base, Sequence::BinWrite
//           common/sequence/sequence.hpp:431-442); u64 0 ends the vertex.
//   .cvr:   per canonical edge u64 id, u32 raw coverage; u64 0 at the end.
// Ids: edge i (GFA segment 3+2i) and its conjugate 3+2i+1 (a self-conjugate edge is its own), as
// FastGraphFromSequencesConstructor numbers them (debruijn_graph_constructor.hpp:450-465, graph_core.hpp:228,610-624).
// Vertices: one pair per distinct canonical end k-mer, numbered 3+2j / 3+2j+1 in ascending k-mer order -- the
// reference numbers them in BooPHF-index order (:494-515), which no other implementation can reproduce, and its
// loader (LoadImpl :48-96) accepts any consistent numbering; parity is therefore structural (tests rebuild the graph
// from the file and compare it with the GFA).
struct SpadesVertices {
    std::vector<uint64_t> vid;  // [2 nu] vertex of the start (2i) and of the end (2i + 1) of edge i
    uint64_t nv = 0;            // vertex pairs
};
static uint64_t conj_vertex(uint64_t v) { return ((v - 3) ^ 1ull) + 3; }

// vertex pair j for every edge end; vid(end) = 3 + 2j + (k-mer is the reverse complement of the canonical form)
static SpadesVertices spades_vertices(const bbk_unitigs *u) {
    const unsigned k = u->k;
    const uint64_t nu = u->n;
    const int W = (int)words_of(k);
    // end k-mers of every edge in canonical form
    struct End {
        uint64_t w[4];
        uint8_t is_rc;
    };
    std::vector<End> ends(2 * nu);
#pragma omp parallel for schedule(static) num_threads(host_threads())
    for (uint64_t i = 0; i < nu; ++i) {
        const char *s = u->bases.data() + u->offsets[i];
        for (int e = 0; e < 2; ++e) {
            const std::string km(s + (e ? unitig_len(u, i) - k : 0), k);
            const std::string r = str_rc(km);
            const bool minimal = km <= r;  // IsMinimal: base-lexicographic, ties minimal (rtseq.hpp:407-415)
            End &d = ends[2 * i + e];
            memset(d.w, 0, sizeof(d.w));
            pack_kmer((minimal ? km : r).data(), k, d.w, W);
            d.is_rc = minimal ? 0 : 1;
        }
    }
    std::vector<uint32_t> order(2 * nu);
    for (uint64_t i = 0; i < 2 * nu; ++i) order[i] = (uint32_t)i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        for (int w = 0; w < W; ++w)
            if (ends[a].w[w] != ends[b].w[w]) return ends[a].w[w] < ends[b].w[w];
        return a < b;
    });
    SpadesVertices V;
    V.vid.resize(2 * nu);
    for (uint64_t r = 0; r < 2 * nu; ++r) {
        const uint32_t a = order[r];
        if (r > 0 && memcmp(ends[a].w, ends[order[r - 1]].w, sizeof(uint64_t) * W) != 0) ++V.nv;
        V.vid[a] = 3 + 2 * V.nv + ends[a].is_rc;
    }
    if (nu) ++V.nv;
    return V;
}

static void write_spades_grseq(const bbk_unitigs *u, const SpadesVertices &V, const std::string &gpath) {
    const uint64_t nu = u->n, nv = V.nv;
    // outgoing lists: edge i (stored orientation) leaves vid(start of i)
    std::vector<std::vector<uint32_t>> out_of(2 * nv);
    for (uint64_t i = 0; i < nu; ++i) out_of[V.vid[2 * i] - 3].push_back((uint32_t)i);
    FILE *f = fopen(gpath.c_str(), "wb");
    BBK_REQUIRE(f != nullptr, BBK_ERR_IO, "cannot open %s for writing", gpath.c_str());
    bool ok = true;
    auto put64 = [&](uint64_t v) { ok = ok && fwrite(&v, 8, 1, f) == 1; };
    put64(3 + 2 * nv);  // reserved id ranges: every id handed out is below
    put64(3 + 2 * nu);
    put64(2 * nv);
    std::vector<uint64_t> words;
    for (uint64_t v = 0; v < 2 * nv && ok; ++v) {
        put64(3 + v);
        put64(conj_vertex(3 + v));
        for (uint32_t i : out_of[v]) {
            const char *s = u->bases.data() + u->offsets[i];
            const uint64_t len = unitig_len(u, i);
            const uint64_t e1 = gfa_id(i), e2 = is_self_rc(s, len) ? e1 : e1 + 1;  // a self-conjugate edge is its own
            put64(e1);
            put64(e2);
            put64(V.vid[2 * i + 1]);               // EdgeEnd(e1)
            put64(conj_vertex(V.vid[2 * i + 1]));  // EdgeStart(conj e1) = conjugate of EdgeEnd(e1)
            put64(len);
            words.resize((len + 31) / 32);
            pack_kmer(s, len, words.data(), words.size());
            ok = ok && (words.empty() || fwrite(words.data(), 8, words.size(), f) == words.size());
        }
        put64(0);
    }
    const int cl = fclose(f);
    BBK_REQUIRE(ok && cl == 0, BBK_ERR_IO, "short write to %s", gpath.c_str());
}

static void write_spades_cvr(const bbk_unitigs *u, const std::string &cpath) {
    FILE *f = fopen(cpath.c_str(), "wb");
    BBK_REQUIRE(f != nullptr, BBK_ERR_IO, "cannot open %s for writing", cpath.c_str());
    bool ok = true;
    for (uint64_t i = 0; i < u->n && ok; ++i) {
        const uint64_t e1 = gfa_id(i);
        const uint64_t raw = u->has_cov ? u->kc[i] : 0;
        const uint32_t cov = raw > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)raw;
        ok = fwrite(&e1, 8, 1, f) == 1 && fwrite(&cov, 4, 1, f) == 1;
    }
    const uint64_t zero = 0;
    ok = ok && fwrite(&zero, 8, 1, f) == 1;
    const int cl = fclose(f);
    BBK_REQUIRE(ok && cl == 0, BBK_ERR_IO, "short write to %s", cpath.c_str());
}

}  // namespace bbk

using namespace bbk;

extern "C" {

int bbk_unitigs_write_gfa(bbk_ctx *ctx, const bbk_unitigs *u, const char *path) {
    return guarded([&] {
        BBK_REQUIRE(ctx && u && path, BBK_ERR_ARG, "bbk_unitigs_write_gfa: NULL argument");
        // the same bytes either way; KC / DP tails are formatted with the host's printf
        if (u->on_device() && !u->has_cov) write_gfa_device(ctx, u, path);
        else write_gfa_host(ctx, u, path);
    });
}

int bbk_unitigs_write_fastg(bbk_ctx *ctx, const bbk_unitigs *u, const char *path) {
    return guarded([&] {
        BBK_REQUIRE(ctx && u && path, BBK_ERR_ARG, "bbk_unitigs_write_fastg: NULL argument");
        write_fastg(ctx, u, path);
    });
}

int bbk_unitigs_write_fasta(bbk_ctx *ctx, const bbk_unitigs *u, const char *path) {
    return guarded([&] {
        BBK_REQUIRE(ctx && u && path, BBK_ERR_ARG, "bbk_unitigs_write_fasta: NULL argument");
        write_fasta(ctx, u, path);
    });
}

int bbk_unitigs_write_spades(bbk_ctx *ctx, const bbk_unitigs *u, const char *basename) {
    return guarded([&] {
        BBK_REQUIRE(ctx && u && basename, BBK_ERR_ARG, "bbk_unitigs_write_spades: NULL argument");
        ensure_host(ctx, u);
        const SpadesVertices V = spades_vertices(u);
        write_spades_grseq(u, V, std::string(basename) + ".grseq");
        write_spades_cvr(u, std::string(basename) + ".cvr");
    });
}

}  // extern "C"
