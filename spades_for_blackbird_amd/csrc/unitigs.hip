// unitigs.hip -- unbranching-path extraction and graph linking; coverage and the unitigs as reads.  The unitig set
// itself and its residency rule are in unitigs.h, the GFA / FASTG / FASTA / SPAdes-binary writers in unitigs_write.hip.
//
// Replaces (reference common/assembly_graph/construction/debruijn_graph_constructor.hpp):
//   UnbranchingPathExtractor::AddStartDeEdges / StepRightIfPossible / ConstructSequenceWithEdge /
//     CalculateSequences (:201-245,267-286)  -> k_count_starts / k_fill_starts / k_walk (one thread
//     per start edge; the sorted (k-mer, mask) table + prefix table replaces the MPHF)
//   `if (s < !s) continue` (:279)              -> decided in-flight from the two end k-mers (see k_walk)
//   CleanCondensed (:288-304)                  -> a visited byte per canonical k-mer
//   CollectLoops / ConstructLoopFromVertex / SplitLoop (:248-265,308-344) -> the (rare) leftover
//     non-junction k-mers are compacted on the device and walked on the host, sequentially like
//     the reference
//   FastGraphFromSequencesConstructor (:390-518): LinkRecord (:400-430) keyed by the canonical end
//     k-mer's table index, device radix sort, vertices = distinct keys, links = incoming x outgoing
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "bbk_internal.h"
#include "kmer_ops.h"
#include "select.h"
#include "unitigs.h"

namespace bbk {

__device__ __host__ inline bool mask_is_junction(uint32_t m) {
    // InOutMask::IsJunction (kmer_extension_index.hpp:46-58,144-162)
    return __builtin_popcount(m & 15u) != 1 || __builtin_popcount((m >> 4) & 15u) != 1;
}

__global__ void k_count_starts(const uint8_t *__restrict__ masks, uint64_t n, uint64_t *__restrict__ cnt) {
    const uint64_t i = BBK_GID();
    if (i >= n) return;
    const uint32_t m = masks[i];
    // outgoing edges of the k-mer and of its reverse complement (whose outgoing = this one's incoming)
    cnt[i] = mask_is_junction(m) ? (uint64_t)__builtin_popcount(m) : 0ull;
}

// start edge descriptor: idx << 3 | strand << 2 | base   (AddStartDeEdges :214-226: the k-mer's own
// outgoing edges for next = 0..3, then those of its reverse complement)
__global__ void k_fill_starts(const uint8_t *__restrict__ masks, uint64_t n, const uint64_t *__restrict__ off,
                              uint64_t *__restrict__ starts) {
    const uint64_t i = BBK_GID();
    if (i >= n) return;
    const uint32_t m = masks[i];
    if (!mask_is_junction(m)) return;
    uint64_t o = off[i];
    for (uint32_t c = 0; c < 4; ++c)
        if (m & (1u << c)) starts[o++] = (i << 3) | c;
    const uint32_t mr = rev8(m);
    for (uint32_t c = 0; c < 4; ++c)
        if (mr & (1u << c)) starts[o++] = (i << 3) | 4u | c;
}

struct WalkOut {
    // pass 0
    uint64_t *keep;      // [E] 0/1
    uint64_t *ulen;      // [E] k + appended bases if kept else 0
    // pass 1
    const uint64_t *uid;   // exclusive scan of keep
    const uint64_t *boff;  // exclusive scan of ulen
    char *bases;
    uint64_t *uoff;        // [U] base offset of unitig
    uint64_t *rec;         // [2U] link records: (idx<<2 | is_rc<<1 | is_start), ~0 = none
    uint8_t *selfconj;     // [U] the unitig equals its own reverse complement
    uint8_t *visited;      // [n]
    uint32_t *err;
};

// One thread per start edge.  PASS 0: length + keep decision (+ visited marks).  PASS 1: write the
// bases and the link records of kept unitigs.
//
// Keep rule (`if (s < !s) continue`, :279): s = x.c....z ; rc(s) starts with rc(z).  If
// x != rc(z) the first k bases decide.  If x == rc(z) the next base decides: s[k] = c against
// rc(s)[k] = comp(base preceding z in s); if these agree too, s and rc(s) leave the same junction
// by the same edge, the walk is deterministic, hence s == rc(s) (self-conjugate edge): keep.
template <int W, int PASS>
__global__ __launch_bounds__(256) void k_walk(const Key<W> *__restrict__ keys, const uint8_t *__restrict__ masks,
                                             PrefixTable P, uint64_t n, int k,
                                             const uint64_t *__restrict__ starts, uint64_t E, WalkOut o) {
    const uint64_t e = BBK_GID();
    if (e >= E) return;
    if (PASS == 1 && o.keep[e] == 0) return;
    const uint64_t d = starts[e];
    const uint64_t i = d >> 3;
    const bool s_rc = (d >> 2) & 1;
    const uint32_t c0 = (uint32_t)(d & 3);
    const Key<W> canon0 = key_load<W>(&keys[i]);
    const Key<W> x = key_select<W>(s_rc, kmer_rc<W>(canon0, k), canon0);
    // pass 1 writes the unitig's bases: 8 ASCII characters are collected in a register and leave as one 8-byte store
    // (global memory takes unaligned 8-byte stores; one store per base was 8x the store instructions of this
    // latency-bound walk)
    typedef uint64_t __attribute__((aligned(1))) u64_any;
    char *dst = nullptr;
    uint64_t pend = 0;   // characters not yet stored
    uint32_t npend = 0;  // how many (0..7)
    uint64_t wpos = 0;   // characters stored so far
    auto put = [&](uint32_t base) {
        pend |= (uint64_t)(unsigned char)"ACGT"[base] << (8 * npend);
        if (++npend == 8) {
            *reinterpret_cast<u64_any *>(dst + wpos) = pend;
            wpos += 8;
            pend = 0;
            npend = 0;
        }
    };
    if (PASS == 1) {
        dst = o.bases + o.boff[e];
        for (int j = 0; j < k; ++j) put(kmer_base<W>(x, j));
        put(c0);
    }
    Key<W> cur = kmer_shl<W>(x, k, c0);
    uint64_t len = 1;
    uint32_t prev_first = kmer_base<W>(x, 0);
    uint64_t j = kNotFound;
    bool cur_min = true;
    Key<W> rcur = cur;
    for (;;) {
        rcur = kmer_rc<W>(cur, k);
        cur_min = !kmer_less_nucl<W>(rcur, cur);
        const Key<W> q = key_select<W>(cur_min, cur, rcur);
        j = table_find<W>(keys, P, q);
        if (j == kNotFound) {
            atomicOr(o.err, 1u);
            return;
        }
        uint32_t m = masks[j];
        if (!cur_min) m = rev8(m);
        if (mask_is_junction(m)) break;
        if (PASS == 0) o.visited[j] = 1;
        const uint32_t c = (uint32_t)__builtin_ctz(m & 15u);
        prev_first = kmer_base<W>(cur, 0);
        cur = kmer_shl<W>(cur, k, c);
        if (PASS == 1) put(c);
        ++len;
        if (len > n + 2) {  // cannot happen on a consistent index: a start edge never re-enters itself
            atomicOr(o.err, 2u);
            return;
        }
    }
    if (PASS == 0) {
        bool keep;
        if (key_eq<W>(x, rcur)) {
            const uint32_t other = 3u - prev_first;
            keep = c0 >= other;
        } else {
            keep = kmer_less_nucl<W>(rcur, x);  // rc(s) < s
        }
        o.keep[e] = keep ? 1ull : 0ull;
        o.ulen[e] = keep ? (uint64_t)k + len : 0ull;
    } else {
        for (uint32_t j = 0; j < npend; ++j) dst[wpos + j] = (char)(pend >> (8 * j));  // the last 0..7 characters
        const uint64_t u = o.uid[e];
        o.uoff[u] = o.boff[e];
        const bool selfconj = key_eq<W>(x, rcur) && c0 == 3u - prev_first;
        // StartLink / EndLink (:432-448): canonical form of the end k-mers, is_rc = k-mer is not it
        o.rec[2 * u] = (i << 2) | ((uint64_t)(s_rc ? 1 : 0) << 1) | 1ull;
        o.rec[2 * u + 1] = selfconj ? ~0ull : ((j << 2) | ((uint64_t)(cur_min ? 0 : 1) << 1));
        o.selfconj[u] = selfconj ? 1 : 0;
    }
}

// the candidates of perfect loops (an ordered selection, select.h): non-junction k-mers no path went through
struct LoopCandidate {
    const uint8_t *__restrict__ masks, *__restrict__ visited;
    __device__ bool operator()(uint64_t i) const { return !mask_is_junction(masks[i]) && !visited[i]; }
};

struct StoreIndex {
    uint64_t *__restrict__ idx;
    __device__ void operator()(uint64_t i, uint64_t rank) const { idx[rank] = i; }
};

// unitigs -> packed reads (bbk_unitigs_to_reads): words per unitig, then one wavefront per unitig packs 32 bases per lane
__global__ void k_unitig_words(const uint64_t *__restrict__ uoff, uint64_t nu, uint64_t *__restrict__ nw,
                               uint32_t *__restrict__ len, uint32_t *__restrict__ err) {
    const uint64_t i = BBK_GID();
    if (i >= nu) return;
    const uint64_t l = uoff[i + 1] - uoff[i];
    if (l > 0xFFFFFFFFull) atomicOr(err, 1u);
    len[i] = (uint32_t)l;
    nw[i] = (l + 31) >> 5;
}
__global__ __launch_bounds__(256) void k_pack_unitigs(const char *__restrict__ bases, const uint64_t *__restrict__ uoff,
                                                     const uint64_t *__restrict__ woff, uint64_t nu,
                                                     uint64_t *__restrict__ words) {
    const uint64_t i = (BBK_GID()) >> 6;
    if (i >= nu) return;
    const int lane = threadIdx.x & 63;
    const uint64_t b0 = uoff[i], len = uoff[i + 1] - b0, nw = (len + 31) >> 5;
    uint64_t *dst = words + woff[i];
    for (uint64_t w = lane; w < nw; w += 64) {
        const uint64_t lo = w << 5, hi = lo + 32 < len ? lo + 32 : len;
        uint64_t v = 0;
        for (uint64_t j = lo; j < hi; ++j) {
            const char c = bases[b0 + j];
            const uint64_t code = c == 'A' ? 0ull : c == 'C' ? 1ull : c == 'G' ? 2ull : 3ull;
            v |= code << ((j - lo) << 1);
        }
        dst[w] = v;
    }
}

__global__ void k_gather_candidates(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ masks,
                                    const uint64_t *__restrict__ idx, uint64_t nc, int W, uint64_t *__restrict__ out_keys,
                                    uint8_t *__restrict__ out_masks) {
    const uint64_t c = BBK_GID();
    if (c >= nc) return;
    const uint64_t r = idx[c];
    for (int w = 0; w < W; ++w) out_keys[c * W + w] = keys[r * W + w];
    out_masks[c] = masks[r];
}

// XXH3 bucket (of nb) of every gathered candidate k-mer: the reference walks its k-mer file bucket by bucket
// (KMerSegmentPolicy, utils/kmer_mph/kmer_buckets.hpp:28-33; 10 x threads buckets, kmer_extension_index_builder.hpp:73)
template <int W>
__global__ void k_candidate_buckets(const uint64_t *__restrict__ keys, uint64_t nc, uint64_t nb, uint32_t *__restrict__ out) {
    const uint64_t c = BBK_GID();
    if (c >= nc) return;
    Key<W> q;
#pragma unroll
    for (int w = 0; w < W; ++w) q.w[w] = keys[c * W + w];
    out[c] = (uint32_t)__umul64hi(xxh3_64<W>(q), nb);
}

// Links from the sorted link records (vertices = groups of equal canonical k-mer index): for every
// canonical vertex every (incoming, outgoing) pair (GFAWriter::WriteLinks, io/graph/gfa_writer.cpp:43-52,
// over the edge lists ConstructionHelper::LinkIncomingEdge/LinkOutgoingEdge build,
// assembly_graph/core/construction_helper.hpp:80-90).  The group head does the work of its group.
__device__ inline bool rec_incoming(uint64_t key) {
    const bool st = key & 1, rc = (key >> 1) & 1;
    return (!st && !rc) || (st && rc);
}
__device__ inline bool rec_outgoing(uint64_t key) {
    const bool st = key & 1, rc = (key >> 1) & 1;
    return (st && !rc) || (!st && rc);
}

template <bool WRITE>
__global__ __launch_bounds__(256) void k_links(const uint64_t *__restrict__ key, const uint32_t *__restrict__ edge,
                                              uint64_t nrec, const uint8_t *__restrict__ selfconj,
                                              uint64_t *__restrict__ cnt, const uint64_t *__restrict__ off,
                                              uint64_t *__restrict__ links, unsigned long long *__restrict__ nvert) {
    const uint64_t r = BBK_GID();
    if (r >= nrec) return;
    const uint64_t kr = key[r];
    const bool head = kr != ~0ull && (r == 0 || (key[r - 1] >> 2) != (kr >> 2));
    if (!head) {
        if (!WRITE) cnt[r] = 0;
        return;
    }
    uint64_t e = r;
    uint32_t nin = 0, nout = 0;
    while (e < nrec && key[e] != ~0ull && (key[e] >> 2) == (kr >> 2)) {
        nin += rec_incoming(key[e]) ? 1u : 0u;
        nout += rec_outgoing(key[e]) ? 1u : 0u;
        ++e;
    }
    if (!WRITE) {
        cnt[r] = (uint64_t)nin * nout;
        atomicAdd(nvert, 1ull);
        return;
    }
    uint64_t o = off[r];
    for (uint64_t a = r; a < e; ++a) {
        const uint64_t ka = key[a];
        if (!rec_incoming(ka)) continue;
        const uint32_t ea = edge[a];
        const uint32_t oa = (!(ka & 1) || selfconj[ea]) ? 1u : 0u;
        for (uint64_t b = r; b < e; ++b) {
            const uint64_t kb = key[b];
            if (!rec_outgoing(kb)) continue;
            const uint32_t eb = edge[b];
            const uint32_t ob = ((kb & 1) || selfconj[eb]) ? 1u : 0u;
            links[2 * o] = ((uint64_t)ea << 1) | oa;
            links[2 * o + 1] = ((uint64_t)eb << 1) | ob;
            ++o;
        }
    }
}

__global__ void k_edge_ids(uint32_t *__restrict__ ids, uint64_t n2) {
    const uint64_t i = BBK_GID();
    if (i < n2) ids[i] = (uint32_t)(i >> 1);
}

// ---- the loop path's candidate table on the host (rare; plain strings) ---------------------------
struct LoopTable {
    int k, W;
    std::vector<uint64_t> idx;     // index in the full table
    std::vector<uint64_t> keys;    // W words each, ascending
    std::vector<uint8_t> masks;
    std::vector<uint8_t> used;
    std::vector<uint64_t> visit;   // the order CollectLoops takes the candidates in (positions in idx)
    // position of an oriented k-mer's canonical form, -1 if absent
    long find(const std::string &kmer, bool *minimal) const {
        const std::string r = str_rc(kmer);
        *minimal = kmer <= r;
        const std::string &c = *minimal ? kmer : r;
        uint64_t q[4];
        pack_kmer(c.data(), k, q, W);
        size_t lo = 0, hi = idx.size();
        while (lo < hi) {
            const size_t mid = lo + (hi - lo) / 2;
            int cmp = 0;
            for (int i = 0; i < W && cmp == 0; ++i)
                cmp = keys[mid * W + i] < q[i] ? -1 : (keys[mid * W + i] > q[i] ? 1 : 0);
            if (cmp == 0) return (long)mid;
            if (cmp < 0) lo = mid + 1;
            else hi = mid;
        }
        return -1;
    }
};

template <int W>
static void run_walk(bbk_ctx *ctx, int pass, const bbk_extindex *x, const uint64_t *starts, uint64_t E, WalkOut o) {
    if (E == 0) return;
    const PrefixTable P = x->prefix.table();
    // bytes: every non-junction k-mer is stepped over once per orientation; a step is one lookup = 2 prefix-table
    // entries + ~3 key probes + 1 mask byte (latency-bound pointer chase: the figure is for reading the rate, not a
    // roofline claim); pass 1 also writes the bases
    KernelTimer t(ctx, pass == 0 ? "walk0" : "walk1", 2.0 * (double)x->n * (3.0 * x->W * 8 + 8 + 1));
    launch_items(ctx, "k_walk", pass == 0 ? k_walk<W, 0> : k_walk<W, 1>, E, x->keys.as<Key<W>>(),
                 x->masks.as<uint8_t>(), P, x->n, (int)x->k, starts, E, o);
}

static void dispatch_walk(bbk_ctx *ctx, int pass, const bbk_extindex *x, const uint64_t *starts, uint64_t E,
                          WalkOut o) {
    dispatch_w(x->W, [&](auto w) { run_walk<decltype(w)::value>(ctx, pass, x, starts, E, o); });
}

struct LinkRec {
    uint64_t key;
    uint32_t edge;
};

void d2h(bbk_ctx *ctx, void *dst, const void *src, size_t bytes) {
    BBK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    BBK_HIP(hipStreamSynchronize(ctx->stream));
}

void ensure_host(bbk_ctx *ctx, const bbk_unitigs *u) {
    if (u->on_host) return;
    BBK_HIP(hipSetDevice(ctx->device));
    u->bases.resize(u->total_bases);
    u->offsets.resize(u->n + 1);
    u->links.resize(2 * u->n_links);
    if (u->total_bases) d2h_big(ctx, u->bases.data(), u->d_bases.p, u->total_bases);
    d2h_big(ctx, u->offsets.data(), u->d_uoff.p, (u->n + 1) * 8);
    if (u->n_links) d2h_big(ctx, u->links.data(), u->d_links.p, u->n_links * 16);
    u->on_host = true;
}

UnitigView device_view(bbk_ctx *ctx, const bbk_unitigs &u, DevBuf &up_bases, DevBuf &up_off) {
    if (u.on_device()) return {u.d_bases.as<char>(), u.d_uoff.as<uint64_t>(), u.total_bases};
    const uint64_t total = u.bases.size();
    up_bases.alloc(total + 16);
    up_off.alloc((u.n + 1) * 8);
    if (total) BBK_HIP(hipMemcpyAsync(up_bases.p, u.bases.data(), total, hipMemcpyHostToDevice, ctx->stream));
    BBK_HIP(hipMemcpyAsync(up_off.p, u.offsets.data(), (u.n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    return {up_bases.as<char>(), up_off.as<uint64_t>(), total};
}

// ---- build(): its phases ------------------------------------------------------------------------------------------
// Each phase owns its temporaries by scope and hands the next one what it needs.  The pool caches blocks, so the
// high-water mark depends on what is freed BEFORE the next allocation; the comment above each phase says what is live
// in it, on top of what it was handed.

struct StartEdges {
    DevBuf starts;  // [E] descriptors, see k_fill_starts
    uint64_t E = 0;
};

// live: cnt (gone on return, before the walk allocates), starts
static StartEdges start_edges(bbk_ctx *ctx, const bbk_extindex *x) {
    const uint64_t n = x->n;
    StartEdges S;
    DevBuf cnt((n + 1) * 8);
    launch_items(ctx, "k_count_starts", k_count_starts, n, x->masks.as<uint8_t>(), n, cnt.as<uint64_t>());
    S.E = exclusive_scan_u64(ctx, cnt.as<uint64_t>(), cnt.as<uint64_t>(), n);
    BBK_REQUIRE(S.E <= 8 * n, BBK_ERR_INTERNAL, "unitigs: %llu start edges counted for %llu k-mers",
                (unsigned long long)S.E, (unsigned long long)n);
    S.starts.alloc((S.E + 1) * 8);
    launch_items(ctx, "k_fill_starts", k_fill_starts, n, x->masks.as<uint8_t>(), n, cnt.as<uint64_t>(),
                 S.starts.as<uint64_t>());
    return S;
}

struct Paths {
    uint64_t NU = 0, NB = 0;  // unitigs, their bases
    DevBuf bases, uoff;       // [NB] ACGT back to back, [NU + 1] offsets
    DevBuf rec, selfc;        // [2 NU] link records, [NU] self-conjugate flags (WalkOut)
    DevBuf visited;           // [n] the k-mer lies inside a path
};

// The two passes of k_walk.  live: starts, keep, ulen, uid, boff, err (all gone on return, before the loop scan
// allocates) and the result.  `S` is taken by value: the start edges end with this phase.
static Paths walk_paths(bbk_ctx *ctx, const bbk_extindex *x, StartEdges S) {
    const int k = (int)x->k;
    const uint64_t n = x->n, E = S.E;
    Paths P;
    // ---- pass 0: lengths + keep
    DevBuf keep((E + 1) * 8), ulen((E + 1) * 8);
    P.visited.alloc(n + 16);
    DevBuf err(16);
    BBK_HIP(hipMemsetAsync(P.visited.p, 0, n + 16, ctx->stream));
    BBK_HIP(hipMemsetAsync(err.p, 0, 16, ctx->stream));
    WalkOut o{};
    o.keep = keep.as<uint64_t>();
    o.ulen = ulen.as<uint64_t>();
    o.visited = P.visited.as<uint8_t>();
    o.err = err.as<uint32_t>();
    dispatch_walk(ctx, 0, x, S.starts.as<uint64_t>(), E, o);
    uint32_t herr = 0;
    d2h(ctx, &herr, err.p, 4);  // before the scans: a walk that gave up leaves its keep / length entries unwritten
    BBK_REQUIRE(herr == 0, BBK_ERR_INTERNAL, "unitig walk failed (code %u): extension index is inconsistent", herr);
    DevBuf uid((E + 1) * 8), boff((E + 1) * 8);
    const uint64_t NU = P.NU = exclusive_scan_u64(ctx, keep.as<uint64_t>(), uid.as<uint64_t>(), E);
    const uint64_t NB = P.NB = exclusive_scan_u64(ctx, ulen.as<uint64_t>(), boff.as<uint64_t>(), E);
    BBK_REQUIRE(NU <= E && NB <= 2 * n + (uint64_t)(k + 1) * NU, BBK_ERR_INTERNAL,
                "unitig walk: %llu unitigs / %llu bases from %llu start edges, %llu k-mers", (unsigned long long)NU,
                (unsigned long long)NB, (unsigned long long)E, (unsigned long long)n);
    // edge ids travel as the u32 payload of the link-record sort
    BBK_REQUIRE(NU < (1ull << 32) - 1, BBK_ERR_ARG, "%llu unitigs: edge ids are 32-bit", (unsigned long long)NU);

    // ---- pass 1: bases + link records
    P.bases.alloc(NB + 16);
    P.uoff.alloc((NU + 1) * 8);
    P.rec.alloc((2 * NU + 2) * 8);
    P.selfc.alloc(NU + 16);
    o.selfconj = P.selfc.as<uint8_t>();
    o.uid = uid.as<uint64_t>();
    o.boff = boff.as<uint64_t>();
    o.bases = P.bases.as<char>();
    o.uoff = P.uoff.as<uint64_t>();
    o.rec = P.rec.as<uint64_t>();
    dispatch_walk(ctx, 1, x, S.starts.as<uint64_t>(), E, o);
    d2h(ctx, &herr, err.p, 4);
    BBK_REQUIRE(herr == 0, BBK_ERR_INTERNAL, "unitig walk (pass 1) failed (code %u)", herr);
    BBK_HIP(hipMemcpyAsync(P.uoff.as<uint64_t>() + NU, &NB, 8, hipMemcpyHostToDevice, ctx->stream));
    return P;
}

struct LoopCandidates {
    PerItem<LoopCandidate> is;  // the test, over masks and Paths::visited
    Selection sel;              // sel.kept: how many; 0 = no perfect loops.  sel.base: n / 256 tile bases
};

// live: the paths, sel
static LoopCandidates loop_candidates(bbk_ctx *ctx, const bbk_extindex *x, const Paths &P) {
    LoopCandidates C{per_item(LoopCandidate{x->masks.as<uint8_t>(), P.visited.as<uint8_t>()}), {}};
    C.sel = select_count(ctx, "loop_candidates", x->n, C.is);
    return C;
}

struct SortedRecs {
    DevBuf ids;         // [2 NU] edge of every record of Paths::rec, which is sorted by (key, edge) now
    DevBuf rtmp, itmp;  // the sort's other halves: they stay as long as ids does, as they always have
};

// live: the paths, sel, ids, rtmp, itmp
static SortedRecs sort_link_records(bbk_ctx *ctx, uint64_t n, Paths &P) {
    const uint64_t NU = P.NU;
    SortedRecs S;
    S.ids.alloc(2 * NU * 4 + 16);
    S.rtmp.alloc((2 * NU + 2) * 8);
    S.itmp.alloc(2 * NU * 4 + 16);
    launch_items(ctx, "k_edge_ids", k_edge_ids, 2 * NU, S.ids.as<uint32_t>(), 2 * NU);
    int bits = 2;
    while ((1ull << (bits - 2)) < n + 1) ++bits;
    std::vector<PassDesc> passes;
    // keys are either < 2^bits or ~0 (no record): the low `bits` bits order the real records; one
    // final pass on the top byte (0x00 vs 0xFF) moves the "no record" entries to the end
    for (int sft = 0; sft < bits; sft += 8) passes.push_back({0, 0, sft, std::min(8, bits - sft), 0});
    passes.push_back({0, 0, 56, 8, 0});
    sort_records(ctx, 1, P.rec.p, S.rtmp.p, S.ids.as<uint32_t>(), S.itmp.as<uint32_t>(), 2 * NU, passes);
    return S;
}

// No perfect loops: vertices and links from the sorted records, and the result stays on the device (host copies are
// made on demand, ensure_host).  live: the paths, sel, the sorted records, lcnt, nv, dl
static void links_on_device(bbk_ctx *ctx, Paths &P, const SortedRecs &S, bbk_unitigs &U) {
    const uint64_t NU = P.NU;
    KernelTimer t(ctx, "links", 0);
    DevBuf lcnt((2 * NU + 1) * 8), nv(16);
    BBK_HIP(hipMemsetAsync(nv.p, 0, 16, ctx->stream));
    launch_items(ctx, "k_links<count>", k_links<false>, 2 * NU, P.rec.as<uint64_t>(), S.ids.as<uint32_t>(), 2 * NU,
                 P.selfc.as<uint8_t>(), lcnt.as<uint64_t>(), (const uint64_t *)nullptr, (uint64_t *)nullptr,
                 nv.as<unsigned long long>());
    const uint64_t NL = exclusive_scan_u64(ctx, lcnt.as<uint64_t>(), lcnt.as<uint64_t>(), 2 * NU);
    DevBuf dl(NL * 16 + 16);
    launch_items(ctx, "k_links<write>", k_links<true>, 2 * NU, P.rec.as<uint64_t>(), S.ids.as<uint32_t>(), 2 * NU,
                 P.selfc.as<uint8_t>(), (uint64_t *)nullptr, lcnt.as<uint64_t>(), dl.as<uint64_t>(),
                 (unsigned long long *)nullptr);
    unsigned long long hv = 0;
    d2h(ctx, &hv, nv.p, 8);
    U.n = NU;
    U.n_loops = 0;
    U.n_vertices = hv;
    U.n_links = NL;
    U.total_bases = P.NB;
    U.d_bases = std::move(P.bases);
    U.d_uoff = std::move(P.uoff);
    U.d_links = std::move(dl);
}

// Perfect loops are appended on the host: the paths come over first.  live: the paths, sel
static void paths_to_host(bbk_ctx *ctx, const Paths &P, bbk_unitigs &U) {
    U.bases.resize(P.NB);
    U.offsets.resize(P.NU + 1);
    if (P.NB) d2h_big(ctx, U.bases.data(), P.bases.p, P.NB);
    d2h_big(ctx, U.offsets.data(), P.uoff.p, (P.NU + 1) * 8);
}

// the sorted link records without the "no record" entries at their end.  live: the paths, sel, the sorted records
static std::vector<LinkRec> link_records_to_host(bbk_ctx *ctx, uint64_t n, Paths &P) {
    const uint64_t NU = P.NU;
    const SortedRecs S = sort_link_records(ctx, n, P);
    raw_vector<uint64_t> hk(2 * NU);
    raw_vector<uint32_t> he(2 * NU);
    d2h_big(ctx, hk.data(), P.rec.p, 2 * NU * 8);
    d2h_big(ctx, he.data(), S.ids.p, 2 * NU * 4);
    std::vector<LinkRec> recs;
    recs.reserve(2 * NU);
    for (uint64_t r = 0; r < 2 * NU; ++r) {
        if (hk[r] == ~0ull) break;
        recs.push_back({hk[r], he[r]});
    }
    return recs;
}

// The leftover non-junction k-mers with their masks, and the order CollectLoops visits them in.
// live: visited, sel, cidx, and for a moment gk, gm, gb (rec, uoff and bases are gone by now)
static LoopTable load_loop_table(bbk_ctx *ctx, const bbk_extindex *x, const LoopCandidates &C, unsigned ref_threads) {
    const uint64_t NC = C.sel.kept;
    LoopTable T;
    T.k = (int)x->k;
    T.W = (int)x->W;
    T.idx.resize(NC);
    DevBuf cidx(NC * 8 + 16);
    select_write(ctx, "loop_candidates", C.sel, C.is, StoreIndex{cidx.as<uint64_t>()});
    d2h_big(ctx, T.idx.data(), cidx.p, NC * 8);
    T.keys.resize(NC * T.W);
    T.masks.resize(NC);
    T.used.assign(NC, 0);
    std::vector<uint32_t> cand_bucket;
    // gather the candidate rows on the device (they may lie anywhere in a table of billions of k-mers)
    DevBuf gk(NC * T.W * 8 + 16), gm(NC + 16);
    launch_items(ctx, "k_gather_candidates", k_gather_candidates, NC, x->keys.as<uint64_t>(), x->masks.as<uint8_t>(),
                 cidx.as<uint64_t>(), NC, T.W, gk.as<uint64_t>(), gm.as<uint8_t>());
    d2h_big(ctx, T.keys.data(), gk.p, NC * T.W * 8);
    d2h_big(ctx, T.masks.data(), gm.p, NC);
    // CollectLoops (:308-344) takes the first unvisited k-mer in K-MER FILE ORDER, and the file is the
    // concatenation of 10 x threads XXH3 buckets, ascending inside: both the rotation of a loop string and the
    // palindrome SplitLoop cuts a self-conjugate circle at follow from that order.  ref_threads = the -t of the
    // reference run to reproduce (0: plain ascending order)
    if (ref_threads) {
        DevBuf gb(NC * 4 + 16);
        const uint64_t nb = 10ull * ref_threads;
        dispatch_w(x->W, [&](auto w) {
            launch_items(ctx, "k_candidate_buckets", k_candidate_buckets<decltype(w)::value>, NC, gk.as<uint64_t>(), NC,
                         nb, gb.as<uint32_t>());
        });
        cand_bucket.resize(NC);
        d2h_big(ctx, cand_bucket.data(), gb.p, NC * 4);
    }
    // visiting order of the candidates: ascending, or (bucket, ascending) = the reference's file order
    T.visit.resize(NC);
    for (uint64_t c = 0; c < NC; ++c) T.visit[c] = c;
    if (!cand_bucket.empty())
        std::stable_sort(T.visit.begin(), T.visit.end(),
                         [&](uint64_t a, uint64_t b) { return cand_bucket[a] < cand_bucket[b]; });
    return T;
}

// records + storage of one loop piece; CleanCondensed(s) and CleanCondensed(rc s)
static void emit_loop(LoopTable &T, const std::string &s, bbk_unitigs &U, std::vector<LinkRec> &recs) {
    const size_t k = (size_t)T.k;
    const std::string r = str_rc(s);
    const std::string &best = (s < r) ? r : s;  // push max(s, rc s) (:330-334)
    const uint64_t id = U.offsets.size() - 1;
    U.bases.insert(U.bases.end(), best.begin(), best.end());
    U.offsets.push_back(U.bases.size());
    const bool selfconj = best == str_rc(best);
    for (int is_start = 1; is_start >= 0; --is_start) {
        if (!is_start && selfconj) continue;
        const std::string km = is_start ? best.substr(0, k) : best.substr(best.size() - k);
        bool minimal;
        const long pos = T.find(km, &minimal);
        BBK_REQUIRE(pos >= 0, BBK_ERR_INTERNAL, "loop end k-mer missing from the candidate table");
        recs.push_back({(T.idx[(size_t)pos] << 2) | ((uint64_t)(minimal ? 0 : 1) << 1) | (uint64_t)is_start,
                        (uint32_t)id});
    }
    for (const std::string *t : {&s, &r})
        for (size_t p = 0; p + k <= t->size(); ++p) {
            bool minimal;
            const long pos = T.find(t->substr(p, k), &minimal);
            if (pos >= 0) T.used[(size_t)pos] = 1;
        }
    ++U.n_loops;
}

// ConstructLoopFromVertex (:255-265) from the canonical k-mer of candidate c
static std::string walk_loop(const LoopTable &T, uint64_t c) {
    const size_t NC = T.idx.size();
    const std::string x0 = unpack_kmer(&T.keys[c * T.W], T.k);
    std::string s = x0;
    std::string cur = x0;
    uint32_t m = T.masks[c];
    for (;;) {
        const int cb = __builtin_ctz(m & 15u);
        cur = cur.substr(1) + "ACGT"[cb];
        if (cur == x0) {  // edge (prev -> x0) closes the cycle: its base is appended, then stop
            s.push_back("ACGT"[cb]);
            break;
        }
        s.push_back("ACGT"[cb]);
        bool minimal;
        const long pos = T.find(cur, &minimal);
        BBK_REQUIRE(pos >= 0, BBK_ERR_INTERNAL, "loop walk left the candidate set");
        m = minimal ? T.masks[(size_t)pos] : rev8(T.masks[(size_t)pos]);
        BBK_REQUIRE(!mask_is_junction(m), BBK_ERR_INTERNAL, "loop walk reached a junction");
        BBK_REQUIRE(s.size() <= 2 * NC + (size_t)T.k + 1, BBK_ERR_INTERNAL, "loop walk does not close");
    }
    // the reference string ends when the walk is back on its first EDGE: x0 . (cycle bases) with
    // the closing k-mer x0 spelled again minus ... -> length = cycle + k  (:232-241)
    // s currently = x0 + one base per cycle edge (cycle edges = n_cyc) -> length k + n_cyc: equal.
    return s;
}

// Perfect loops: leftover non-junction k-mers (CollectLoops :308-344), walked on the host, sequentially like the
// reference.  Appends the loops to U's host arrays and their records to recs, which it sorts again.  Host only.
static void collect_loops_on_host(LoopTable &T, bbk_unitigs &U, std::vector<LinkRec> &recs) {
    const size_t k = (size_t)T.k;
    for (const uint64_t c : T.visit) {
        if (T.used[c]) continue;
        const std::string s = walk_loop(T, c);
        // SplitLoop (:248-252) on the first (k+1)-mer equal to its own reverse complement
        size_t split = std::string::npos;
        for (size_t p = 0; p + k + 1 <= s.size(); ++p) {
            const std::string e = s.substr(p, k + 1);
            if (e == str_rc(e)) {
                split = p;
                break;
            }
        }
        if (split == std::string::npos) {
            emit_loop(T, s, U, recs);
        } else {
            emit_loop(T, s.substr(split, k + 1), U, recs);
            emit_loop(T, s.substr(split + 1, s.size() - k - (split + 1)) + s.substr(0, split + k), U, recs);
        }
    }
    std::stable_sort(recs.begin(), recs.end(), [](const LinkRec &a, const LinkRec &b) {
        return a.key != b.key ? a.key < b.key : a.edge < b.edge;
    });
}

// vertices + links (gfa_writer.cpp:43-52 over construction_helper.hpp:80-90) of a host result.  Host only.
static void links_on_host(bbk_unitigs &U, const std::vector<LinkRec> &recs) {
    std::vector<uint8_t> selfconj(U.n, 0);
    {
        // an edge with a start record but no end record is self-conjugate
        std::vector<uint8_t> has_end(U.n, 0);
        for (const LinkRec &r : recs)
            if (!(r.key & 1)) has_end[r.edge] = 1;
        for (uint64_t i = 0; i < U.n; ++i) selfconj[i] = !has_end[i];
    }
    uint64_t nv = 0;
    for (size_t p = 0; p < recs.size();) {
        size_t q = p;
        const uint64_t h = recs[p].key >> 2;
        while (q < recs.size() && (recs[q].key >> 2) == h) ++q;
        ++nv;
        for (size_t a = p; a < q; ++a) {
            const bool a_start = recs[a].key & 1, a_rc = (recs[a].key >> 1) & 1;
            if (!((!a_start && !a_rc) || (a_start && a_rc))) continue;  // incoming at the canonical vertex
            const uint32_t ea = recs[a].edge;
            const uint32_t oa = (!a_start || selfconj[ea]) ? 1u : 0u;
            for (size_t b = p; b < q; ++b) {
                const bool b_start = recs[b].key & 1, b_rc = (recs[b].key >> 1) & 1;
                if (!((b_start && !b_rc) || (!b_start && b_rc))) continue;  // outgoing
                const uint32_t eb = recs[b].edge;
                const uint32_t ob = (b_start || selfconj[eb]) ? 1u : 0u;
                U.links.push_back(((uint64_t)ea << 1) | oa);
                U.links.push_back(((uint64_t)eb << 1) | ob);
            }
        }
        p = q;
    }
    U.n_vertices = nv;
    U.n_links = U.links.size() / 2;
}

static void build(bbk_ctx *ctx, const bbk_extindex *x, bbk_unitigs &U, unsigned ref_threads) {
    const uint64_t n = x->n;
    U.k = x->k;
    BBK_REQUIRE(x->k % 2 == 1, BBK_ERR_ARG, "k-mer size must be odd");  // projects/gbuilder/main.cpp:125-126
    // k-mer indices, start edges and link-record keys are 64-bit (KMerIndex::seq_idx is a size_t, kmer_index.hpp:85-90;
    // LinkRecord keys are 64-bit, debruijn_graph_constructor.hpp:400-430); only the launch grid bounds n
    BBK_REQUIRE(n < (1ull << 37), BBK_ERR_ARG, "extension index of %llu k-mers exceeds the launch grid", (unsigned long long)n);
    U.offsets.assign(1, 0);
    if (n == 0) {  // the empty result is a host result
        U.on_host = true;
        return;
    }
    Paths P = walk_paths(ctx, x, start_edges(ctx, x));
    const LoopCandidates C = loop_candidates(ctx, x, P);
    if (C.sel.kept == 0 && P.NU != 0) {  // the common case: no perfect loops, links are made on the device
        const SortedRecs S = sort_link_records(ctx, n, P);
        links_on_device(ctx, P, S, U);
    } else {
        if (C.sel.kept) paths_to_host(ctx, P, U);
        std::vector<LinkRec> recs;
        if (P.NU) recs = link_records_to_host(ctx, n, P);
        P.rec.release();  // the device is done with the paths; the loop walk keeps visited and sel
        P.uoff.release();
        P.bases.release();
        if (C.sel.kept) {
            LoopTable T = load_loop_table(ctx, x, C, ref_threads);
            collect_loops_on_host(T, U, recs);
        }
        U.n = P.NU + U.n_loops;
        U.total_bases = U.bases.size();
        U.on_host = true;
        links_on_host(U, recs);
    }
}

// One thread per unitig: roll the (k+1)-mers of the sequence, look the canonical form up in the
// sorted (k+1)-mer count table, add the multiplicities (GraphCoverageFiller,
// assembly_graph/graph_support/coverage_filling.hpp:44-62).
template <int W>
__global__ __launch_bounds__(256) void k_unitig_kc(const char *__restrict__ bases, const uint64_t *__restrict__ off,
                                                  uint64_t n_unitigs, int k1, const Key<W> *__restrict__ keys,
                                                  const uint32_t *__restrict__ counts, PrefixTable P,
                                                  uint64_t *__restrict__ kc, uint32_t *__restrict__ err) {
    const uint64_t u = BBK_GID();
    if (u >= n_unitigs) return;
    const char *s = bases + off[u];
    const uint64_t len = off[u + 1] - off[u];
    uint64_t sum = 0;
    if (len >= (uint64_t)k1) {
        Key<W> cur;
#pragma unroll
        for (int j = 0; j < W; ++j) cur.w[j] = 0;
        auto code = [](char c) -> uint32_t { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : 3u; };
        for (int i = 0; i < k1 - 1; ++i) cur = kmer_shl<W>(cur, k1, code(s[i]));
        for (uint64_t p = (uint64_t)k1 - 1; p < len; ++p) {
            cur = kmer_shl<W>(cur, k1, code(s[p]));
            const Key<W> rc = kmer_rc<W>(cur, k1);
            const bool minimal = !kmer_less_nucl<W>(rc, cur);
            const Key<W> q = key_select<W>(minimal, cur, rc);
            const uint64_t j = table_find<W>(keys, P, q);
            if (j == kNotFound) atomicOr(err, 4u);
            else sum += counts[j];
        }
    }
    kc[u] = sum;
}

}  // namespace bbk

using namespace bbk;

extern "C" {

// KC of every unitig from a table of canonical (k+1)-mer multiplicities
static void coverage_from_counts(bbk_ctx *ctx, bbk_unitigs *u, const bbk_kmerset *set) {
    const unsigned k1 = u->k + 1;
    BBK_REQUIRE(set->k == k1 && set->has_counts && set->sorted && !set->ref_order && (set->flags & BBK_CANONICAL),
                BBK_ERR_ARG, "coverage needs the ascending canonical %u-mer set with counts "
                "(BBK_CANONICAL | BBK_WITH_COUNTS at k + 1)", k1);
    u->kc.assign(u->n, 0);
    u->has_cov = true;
    if (u->n == 0) return;
    PrefixIndex pref;
    pref.build(ctx, set->keys.as<uint64_t>(), set->W, k1, set->n);
    DevBuf up_bases, up_off;
    const UnitigView v = device_view(ctx, *u, up_bases, up_off);
    DevBuf d_kc(u->n * 8), d_err(16);
    BBK_HIP(hipMemsetAsync(d_err.p, 0, 16, ctx->stream));
    dispatch_w(set->W, [&](auto w) {
        constexpr int W_ = decltype(w)::value;
        KernelTimer t(ctx, "coverage", 0);
        launch_items(ctx, "k_unitig_kc", k_unitig_kc<W_>, u->n, v.bases, v.uoff, u->n, (int)k1,
                     set->keys.as<Key<W_>>(), set->counts.as<uint32_t>(), pref.table(), d_kc.as<uint64_t>(),
                     d_err.as<uint32_t>());
    });
    uint32_t herr = 0;
    d2h(ctx, &herr, d_err.p, 4);
    BBK_REQUIRE(herr == 0, BBK_ERR_INTERNAL, "coverage: a (k+1)-mer of a unitig is missing from the count table");
    d2h(ctx, u->kc.data(), d_kc.p, u->n * 8);
}

int bbk_unitigs_add_coverage(bbk_ctx *ctx, bbk_unitigs *u, const bbk_reads *reads) {
    return guarded([&] {
        BBK_REQUIRE(ctx && u && reads, BBK_ERR_ARG, "bbk_unitigs_add_coverage: NULL argument");
        BBK_HIP(hipSetDevice(ctx->device));
        // multiplicities of the canonical (k+1)-mers over reads + rc(reads)
        // (CoverageHashMapBuilder::FillCoverageFromStream, utils/ph_map/coverage_hash_map_builder.hpp:15-38)
        bbk_kmerset *set = nullptr;
        const int rc = bbk_count(ctx, reads, u->k + 1, BBK_CANONICAL | BBK_WITH_COUNTS, &set);
        if (rc != BBK_OK) throw Error{rc};
        std::unique_ptr<bbk_kmerset, void (*)(bbk_kmerset *)> guard(set, bbk_kmerset_free);
        coverage_from_counts(ctx, u, set);
    });
}

int bbk_unitigs_add_coverage_counts(bbk_ctx *ctx, bbk_unitigs *u, const bbk_kmerset *kp1_counts) {
    return guarded([&] {
        BBK_REQUIRE(ctx && u && kp1_counts, BBK_ERR_ARG, "bbk_unitigs_add_coverage_counts: NULL argument");
        BBK_HIP(hipSetDevice(ctx->device));
        coverage_from_counts(ctx, u, kp1_counts);
    });
}

int bbk_unitigs_export_kc(bbk_ctx *ctx, const bbk_unitigs *u, uint64_t *h_kc) {
    return guarded([&] {
        BBK_REQUIRE(ctx && u && h_kc && u->has_cov, BBK_ERR_ARG, "bbk_unitigs_export_kc: no coverage (call bbk_unitigs_add_coverage)");
        if (u->n) memcpy(h_kc, u->kc.data(), u->n * sizeof(uint64_t));
    });
}

int bbk_unitigs_to_reads(bbk_ctx *ctx, const bbk_unitigs *u, bbk_reads **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && u && out, BBK_ERR_ARG, "bbk_unitigs_to_reads: NULL argument");
        BBK_HIP(hipSetDevice(ctx->device));
        const uint64_t nu = u->n;
        DevBuf up_bases, up_off;
        const UnitigView v = device_view(ctx, *u, up_bases, up_off);
        auto rd = std::make_unique<bbk_reads>();
        rd->ctx = ctx;
        rd->n = nu;
        rd->bases = v.total;
        rd->own_woff.alloc((nu + 1) * sizeof(uint64_t));
        rd->own_len.alloc((nu + 1) * sizeof(uint32_t));
        uint64_t nwords = 0;
        if (nu) {
            DevBuf err(16);
            BBK_HIP(hipMemsetAsync(err.p, 0, 16, ctx->stream));
            launch_items(ctx, "k_unitig_words", k_unitig_words, nu, v.uoff, nu, rd->own_woff.as<uint64_t>(),
                         rd->own_len.as<uint32_t>(), err.as<uint32_t>());
            nwords = exclusive_scan_u64(ctx, rd->own_woff.as<uint64_t>(), rd->own_woff.as<uint64_t>(), nu);
            uint32_t herr = 0;
            d2h(ctx, &herr, err.p, 4);
            BBK_REQUIRE(herr == 0, BBK_ERR_ARG, "bbk_unitigs_to_reads: a unitig is longer than 2^32 - 1 bases");
        }
        BBK_HIP(hipMemcpyAsync(rd->own_woff.as<uint64_t>() + nu, &nwords, 8, hipMemcpyHostToDevice, ctx->stream));
        rd->n_words = nwords;
        rd->own_words.alloc((nwords + 1) * sizeof(uint64_t));
        if (nu) {
            launch_items(ctx, "k_pack_unitigs", k_pack_unitigs, nu * 64, v.bases, v.uoff, rd->own_woff.as<uint64_t>(),
                         nu, rd->own_words.as<uint64_t>());
        }
        BBK_HIP(hipStreamSynchronize(ctx->stream));
        rd->d_words = rd->own_words.as<uint64_t>();
        rd->d_woff = rd->own_woff.as<uint64_t>();
        rd->d_len = rd->own_len.as<uint32_t>();
        *out = rd.release();
    });
}

int bbk_unitigs_build_ex(bbk_ctx *ctx, bbk_extindex *x, unsigned ref_threads, bbk_unitigs **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && x && out, BBK_ERR_ARG, "bbk_unitigs_build: NULL argument");
        BBK_REQUIRE(ref_threads <= (1u << 20), BBK_ERR_ARG, "bbk_unitigs_build_ex: ref_threads %u", ref_threads);
        BBK_HIP(hipSetDevice(ctx->device));
        auto u = std::make_unique<bbk_unitigs>();
        build(ctx, x, *u, ref_threads);
        *out = u.release();
    });
}

int bbk_unitigs_build(bbk_ctx *ctx, bbk_extindex *x, bbk_unitigs **out) { return bbk_unitigs_build_ex(ctx, x, 0, out); }

uint64_t bbk_unitigs_count(const bbk_unitigs *u) { return u ? u->n : 0; }
uint64_t bbk_unitigs_loops(const bbk_unitigs *u) { return u ? u->n_loops : 0; }
uint64_t bbk_unitigs_total_bases(const bbk_unitigs *u) { return u ? u->total_bases : 0; }
uint64_t bbk_unitigs_vertices(const bbk_unitigs *u) { return u ? u->n_vertices : 0; }
uint64_t bbk_unitigs_links(const bbk_unitigs *u) { return u ? u->n_links : 0; }

int bbk_unitigs_export(bbk_ctx *ctx, const bbk_unitigs *u, char *h_bases, uint64_t *h_offsets) {
    return guarded([&] {
        BBK_REQUIRE(ctx && u, BBK_ERR_ARG, "bbk_unitigs_export: NULL argument");
        ensure_host(ctx, u);
        if (h_bases && !u->bases.empty()) memcpy(h_bases, u->bases.data(), u->bases.size());
        if (h_offsets) memcpy(h_offsets, u->offsets.data(), u->offsets.size() * sizeof(uint64_t));
    });
}

int bbk_unitigs_export_links(bbk_ctx *ctx, const bbk_unitigs *u, uint32_t *h_links) {
    return guarded([&] {
        BBK_REQUIRE(ctx && u && (u->n_links == 0 || h_links), BBK_ERR_ARG, "bbk_unitigs_export_links: NULL argument");
        ensure_host(ctx, u);
        for (uint64_t l = 0; l < u->n_links; ++l) {
            h_links[4 * l] = (uint32_t)(u->links[2 * l] >> 1);  // edge ids are below 2^32 - 1 (build)
            h_links[4 * l + 1] = (uint32_t)(u->links[2 * l] & 1u);
            h_links[4 * l + 2] = (uint32_t)(u->links[2 * l + 1] >> 1);
            h_links[4 * l + 3] = (uint32_t)(u->links[2 * l + 1] & 1u);
        }
    });
}

void bbk_unitigs_free(bbk_unitigs *u) { delete u; }

}  // extern "C"
