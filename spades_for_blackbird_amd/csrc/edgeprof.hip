// edgeprof.hip -- per-sample edge abundance profiles: the device side of unitig-coverage.
//
// Replaces (reference projects/unitig_coverage/, common/modules/alignment/sequence_mapper.hpp:288-404):
//   EdgeIndex over the (k+1)-mers of every edge and its conjugate -> k_ep_emit + radix sort + prefix table: one
//     canonical (k+1)-mer per record with (segment, offset on the forward strand, offset on the reverse strand, flags)
//   BasicSequenceMapper::MapSequence (FindKmer / TryThread / ProcessKmer), run read by read on one thread per sample
//     -> k_ep_map: one lane per (k+1)-mer position, each position settled from its own lookup and its predecessor's
//   EdgeProfileStorage::Fill / Save (profile_storage.hpp:71-93, profile_storage.cpp:44-52) -> 64-bit atomics per run of
//     equal segment inside a wave, and a host writer of the reference's text.
//
// Position-local form of MapSequence.  With every (k+1)-mer present once in the graph (both orientations counted) and
// every link a true k-overlap, TryThread succeeds exactly when FindKmer would find the next (k+1)-mer and merge it into
// the current range, so the size the read adds to the range of position i depends only on positions i-1 and i:
//   delta_i = 0                      position i not in the graph
//           = off_i - off_{i-1}      i-1 found on the same oriented edge and off_i >= off_{i-1}
//           = 1                      otherwise
// One exception: a one-(k+1)-mer homopolymer edge c^(k+1) linked to itself.  Inside a run of c there, TryThread leaves
// the end of the edge and re-enters it at offset 0 with a new range of size 1, where the merge rule says 0 (off_i ==
// off_{i-1}).  Such edges carry a flag and take 1 (exact when every junction is an edge end, as in a condensed graph).
// A read and its reverse complement (EasyStream followed_by_rc) map to conjugate edges: contrib(rc r, X) =
// contrib(r, conj X), so one pass over the forward read adds both strands to the segment; a self-conjugate segment gets
// both terms from the same edge and takes every delta twice.
//
// Mapping paths (spades-gmapper, projects/gmapper/main.cpp:156-247): k_gm_paths emits the full MappingPath of every
// read instead, one record per range (read, oriented edge, initial [start, end), mapped [start, end)).  By the same
// argument a position starts a new range exactly where the delta rule does not merge it into its predecessor's:
//   start_i = found_i && !(i-1 found on the same oriented edge && (off_i > off_{i-1} || off_i == off_{i-1} && !kEpLoop1))
// (FindKmer merges on off_i + 1 >= mapped end = off_{i-1} + 1; TryThread extends by one inside an edge, the
// off_i = off_{i-1} + 1 case, and opens a range at offset 0 of an outgoing edge, which differs from FindKmer only on a
// one-(k+1)-mer edge looped to itself).  kEpLoop1 comes from the L lines (a link e+ -> e+); the literal mapper asks
// whether e is among OutgoingEdges(EdgeEnd(e)) in the graph ConstructionHelper::LinkEdges builds, which can differ on a
// GFA with partial junctions.  Where it differs, only the cut of a run on that edge into ranges changes (one range per
// position, or one for the run): the edge sequence and the summed initial sizes that GappedPathExtractor reads
// (DeleteSameEdges, CountMappedEdgeSize) stay the same, so spades-gmapper's output does not depend on it, and
// host/gmapper_main.cpp reports such edges.  Records are written without a shared cursor: a count pass takes one
// ballot per wave, an exclusive scan gives every wave its first record, and a write pass fills them.  A range is closed
// by the position after its last one (or by its last one at the end of a read), which finds the record through the
// range index (range starts up to the position, minus one).
#include <hip/hip_runtime.h>

#include <omp.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "bbk_internal.h"
#include "edgeindex.h"
#include "gfa_graph.h"
#include "kmer_ops.h"
#include "unitigs.h"

namespace bbk {

// ---- index ------------------------------------------------------------------------------------------------------------

// One lane per emitted (k+1)-mer.  A self-conjugate segment holds x at p and rc(x) at len-1-p, one key: only the
// positions p <= len-1-p are emitted (emit_off counts them), so any equal keys left after the sort are duplicates.
template <int W>
__global__ __launch_bounds__(256) void k_ep_emit(const uint64_t *__restrict__ words, const uint64_t *__restrict__ woff,
                                                const uint64_t *__restrict__ emit_off, const uint32_t *__restrict__ seg_len,
                                                const uint32_t *__restrict__ seg_flags, uint64_t n_seg, uint64_t n, int k1,
                                                Key<W> *__restrict__ keys, uint32_t *__restrict__ idx,
                                                EdgePos *__restrict__ pos) {
    const uint64_t j = BBK_GID();
    if (j >= n) return;
    const uint64_t s = last_le(emit_off, n_seg, j);  // the segment that emits record j (segments emit at least one)
    const uint32_t p = (uint32_t)(j - emit_off[s]);
    const Key<W> x = kmer_extract<W>(words + woff[s], p, k1);
    const Key<W> r = kmer_rc<W>(x, k1);
    const bool fw = !kmer_less_nucl<W>(r, x);
    key_store<W>(&keys[j], key_select<W>(fw, x, r));
    idx[j] = (uint32_t)j;
    EdgePos e;
    e.seg = (uint32_t)s;
    e.off_fw = p;
    e.off_rc = seg_len[s] - 1u - p;
    e.flags = seg_flags[s] | (fw ? kEpCanonFw : 0u);
    pos[j] = e;
}

// records in key order; equal neighbours are duplicated (k+1)-mers (the smallest such index is reported)
template <int W>
__global__ __launch_bounds__(256) void k_ep_gather(const Key<W> *__restrict__ keys, const uint32_t *__restrict__ idx,
                                                  const EdgePos *__restrict__ pos, uint64_t n, EdgePos *__restrict__ out,
                                                  unsigned long long *__restrict__ first_dup) {
    const uint64_t i = BBK_GID();
    if (i >= n) return;
    out[i] = pos[idx[i]];
    if (i > 0 && key_eq<W>(key_load<W>(&keys[i]), key_load<W>(&keys[i - 1]))) atomicMin(first_dup, (unsigned long long)i);
}

// ---- mapping ----------------------------------------------------------------------------------------------------------

__global__ void k_ep_npos(const uint32_t *__restrict__ len, uint64_t n, uint32_t k1, uint64_t *__restrict__ npos) {
    const uint64_t r = BBK_GID();
    if (r < n) npos[r] = len[r] >= k1 ? (uint64_t)(len[r] - k1 + 1) : 0ull;
}

constexpr int kMapWaves = 4;     // waves per block
constexpr int kMapStep = 63;     // new positions per wave: lane 0 is the predecessor of lane 1
constexpr uint32_t kNoSeg = ~0u;

// One wave = 63 consecutive (k+1)-mer positions of the concatenated reads (lanes 1..63) plus the position before the
// first (lane 0, looked up only to be the predecessor).  Every lane finds its read in pos_off, extracts and
// canonicalises its (k+1)-mer and looks it up; lane i takes (edge, offset, found) of lane i-1 by a shuffle and settles
// delta_i (header comment).  The deltas are summed per segment inside the wave (peeling one segment at a time: a wave
// usually covers one or two), and one 64-bit atomic per segment adds the sum to raw[segment * S + sample].
template <int W>
__global__ __launch_bounds__(256) void k_ep_map(const uint64_t *__restrict__ words, const uint64_t *__restrict__ woff,
                                               const uint32_t *__restrict__ rlen, const uint64_t *__restrict__ pos_off,
                                               uint64_t n_reads, uint64_t total, int k1, const Key<W> *__restrict__ keys,
                                               const EdgePos *__restrict__ epos, PrefixTable P,
                                               unsigned long long *__restrict__ raw, uint32_t samples, uint32_t sample) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (((uint64_t)blockIdx.y * gridDim.x) + blockIdx.x) * kMapWaves + (threadIdx.x >> 6);
    const uint64_t g0 = wave * kMapStep;
    if (g0 >= total) return;  // wave-uniform
    const int64_t g = (int64_t)g0 + lane - 1;
    const bool valid = g >= 0 && (uint64_t)g < total;

    bool found = false;
    uint32_t seg = kNoSeg, off = 0, flags = 0;
    uint64_t oe = ~0ull;  // oriented edge: 2 * seg + (minus strand of a segment that is not self-conjugate)
    uint32_t p = 0;       // position inside the read
    if (valid) {
        const uint64_t lo = last_le(pos_off, n_reads, (uint64_t)g);  // the read that holds position g
        p = (uint32_t)((uint64_t)g - pos_off[lo]);
        const uint64_t *rw = words + woff[lo];
        bool minimal;
        const Key<W> q = kmer_canon<W>(rw, p, k1, (rlen[lo] - 1u) >> 5, &minimal);
        const uint64_t j = table_find<W>(keys, P, q);
        if (j != kNotFound) {
            const EdgePos e = epos[j];
            found = true;
            seg = e.seg;
            flags = e.flags;
            // the read's (k+1)-mer is the segment's forward window when it is as canonical as the stored one
            const bool minus = minimal != ((e.flags & kEpCanonFw) != 0);
            off = minus ? e.off_rc : e.off_fw;
            oe = 2ull * e.seg + ((minus && !(e.flags & kEpSelfConj)) ? 1u : 0u);
        }
    }
    const uint64_t pred_oe = __shfl_up(oe, 1);
    const uint32_t pred_off = __shfl_up(off, 1);
    const int pred_found = __shfl_up((int)found, 1);
    uint64_t c = 0;
    if (lane > 0 && found) {
        uint64_t d = 1;
        if (p > 0 && pred_found && pred_oe == oe && off >= pred_off)
            d = off > pred_off ? (uint64_t)(off - pred_off) : ((flags & kEpLoop1) ? 1u : 0u);
        c = d << ((flags & kEpSelfConj) ? 1 : 0);
    }
    bool pending = c != 0;
    uint64_t todo = __ballot(pending);
    while (todo) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint32_t s0 = __shfl(seg, leader);
        const bool mine = pending && seg == s0;
        uint64_t v = mine ? c : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == leader) atomicAdd(&raw[(uint64_t)s0 * samples + sample], (unsigned long long)v);
        pending = pending && !mine;
        todo = __ballot(pending);
    }
}

// ---- mapping paths ----------------------------------------------------------------------------------------------------

// k_ep_map's waves and lookups, one record per range of MappingPath (header comment).  WRITE = false: the range starts
// of every wave to wave_cnt[wave]; WRITE = true: wave_cnt holds their exclusive scan, a start writes (edge, read,
// starts) of its record and the position that ends a range writes its ends.
template <int W, bool WRITE>
__global__ __launch_bounds__(256) void k_gm_paths(const uint64_t *__restrict__ words, const uint64_t *__restrict__ woff,
                                                 const uint32_t *__restrict__ rlen, const uint64_t *__restrict__ pos_off,
                                                 uint64_t n_reads, uint64_t total, int k1, const Key<W> *__restrict__ keys,
                                                 const EdgePos *__restrict__ epos, PrefixTable P,
                                                 uint64_t *__restrict__ wave_cnt, bbk_path_range *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (((uint64_t)blockIdx.y * gridDim.x) + blockIdx.x) * kMapWaves + (threadIdx.x >> 6);
    const uint64_t g0 = wave * kMapStep;
    if (g0 >= total) return;  // wave-uniform
    const int64_t g = (int64_t)g0 + lane - 1;
    const bool valid = g >= 0 && (uint64_t)g < total;

    bool found = false;
    uint32_t off = 0, flags = 0;
    uint64_t oe = ~0ull;
    uint32_t p = 0, last = 0, rd = 0;  // position inside the read, the read's last position, the read
    if (valid) {
        const uint64_t lo = last_le(pos_off, n_reads, (uint64_t)g);
        rd = (uint32_t)lo;
        p = (uint32_t)((uint64_t)g - pos_off[lo]);
        last = (uint32_t)(pos_off[lo + 1] - pos_off[lo] - 1);
        const uint64_t *rw = words + woff[lo];
        bool minimal;
        const Key<W> q = kmer_canon<W>(rw, p, k1, (rlen[lo] - 1u) >> 5, &minimal);
        const uint64_t j = table_find<W>(keys, P, q);
        if (j != kNotFound) {
            const EdgePos e = epos[j];
            found = true;
            flags = e.flags;
            const bool minus = minimal != ((e.flags & kEpCanonFw) != 0);
            off = minus ? e.off_rc : e.off_fw;
            oe = 2ull * e.seg + ((minus && !(e.flags & kEpSelfConj)) ? 1u : 0u);
        }
    }
    const uint64_t pred_oe = __shfl_up(oe, 1);
    const uint32_t pred_off = __shfl_up(off, 1);
    const int pred_found = __shfl_up((int)found, 1);
    const bool pred_here = lane > 0 && p > 0 && pred_found;  // the predecessor is on the graph, in the same read
    const bool cont = found && pred_here && pred_oe == oe &&
                      (off > pred_off || (off == pred_off && !(flags & kEpLoop1)));
    const bool start = lane > 0 && found && !cont;
    const uint64_t starts = __ballot(start);
    if constexpr (!WRITE) {
        if (lane == 0) wave_cnt[wave] = (uint64_t)__popcll(starts);
    } else {
        if (lane == 0) return;  // lane 0 is the previous wave's lane 63
        // range starts at positions before g: earlier waves, then lanes 1 .. lane-1 of this one
        const uint64_t before = wave_cnt[wave] + (uint64_t)__popcll(starts & ((1ull << lane) - 1));
        if (start) {
            bbk_path_range &r = out[before];
            r.edge = oe;
            r.read = rd;
            r.init_start = p;
            r.map_start = off;
            r.reserved = 0;
        }
        if (pred_here && !cont) {  // the predecessor ends its range
            bbk_path_range &r = out[before - 1];
            r.init_end = p;
            r.map_end = pred_off + 1;
        }
        if (found && p == last) {  // the read ends on the graph
            bbk_path_range &r = out[before + (start ? 1 : 0) - 1];
            r.init_end = p + 1;
            r.map_end = off + 1;
        }
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------

static void require_graph(const GraphError &e) { BBK_REQUIRE(!e, e.io ? BBK_ERR_IO : BBK_ERR_ARG, "%s", e.msg.c_str()); }

// keep: the index also keeps bases, offsets, links and KC (what spades-gmapper rebuilds the graph from); profiles need none
static void keep_or_drop_graph(bbk_edgeindex *ix, HostGraph &g, bool keep) {
    if (!keep) return std::string().swap(g.bases);
    ix->has_graph = true;
    ix->bases = std::move(g.bases);
    ix->off = std::move(g.off);
    ix->kc = g.kc.empty() ? std::vector<uint32_t>(ix->n_seg, 0) : std::move(g.kc);
    ix->links.reserve(4 * g.links.size());
    for (const HostLink &l : g.links) ix->links.insert(ix->links.end(), {l.a, l.oa ? 1u : 0u, l.b, l.ob ? 1u : 0u});
}

// emit, sort, gather over the segments as a packed read set (one segment per read): keys and records of the index in
// key order.  Returns the smallest index whose key equals its predecessor's (~0: every (k+1)-mer is there once).
static uint64_t build_device_index(bbk_ctx *ctx, bbk_edgeindex *ix, const bbk_reads *sr, const SegmentTable &t) {
    const uint64_t ns = ix->n_seg, n = ix->n;
    const unsigned W = ix->W, k1 = ix->k1;
    DevBuf d_emit((ns + 1) * 8), d_len(ns * 4), d_flags(ns * 4);
    BBK_HIP(hipMemcpyAsync(d_emit.p, t.emit.data(), (ns + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    BBK_HIP(hipMemcpyAsync(d_len.p, t.len32.data(), ns * 4, hipMemcpyHostToDevice, ctx->stream));
    BBK_HIP(hipMemcpyAsync(d_flags.p, t.flags.data(), ns * 4, hipMemcpyHostToDevice, ctx->stream));
    // (length, self-conjugate) of every segment stays on the device: what the paired-info join reads per range
    std::vector<uint32_t> &seg = ix->seg_h;
    seg.resize(ns);
    for (uint64_t s = 0; s < ns; ++s) seg[s] = t.len32[s] | ((t.flags[s] & kEpSelfConj) ? kSegSelfConj : 0u);
    ix->seg.alloc(ns * 4);
    BBK_HIP(hipMemcpyAsync(ix->seg.p, seg.data(), ns * 4, hipMemcpyHostToDevice, ctx->stream));
    DevBuf tmp(n * W * 8), idx(n * 4), idx_tmp(n * 4), pos(n * sizeof(EdgePos)), dup(8);
    ix->keys.alloc(n * W * 8);
    ix->pos.alloc(n * sizeof(EdgePos));
    {
        KernelTimer timer(ctx, "edgeindex", (double)n * (W * 8 + sizeof(EdgePos) + 4));
        dispatch_w(W, [&](auto w) {
            constexpr int W_ = decltype(w)::value;
            launch_items(ctx, "k_ep_emit", k_ep_emit<W_>, n, sr->d_words, sr->d_woff, d_emit.as<uint64_t>(),
                         d_len.as<uint32_t>(), d_flags.as<uint32_t>(), ns, n, (int)k1, ix->keys.as<Key<W_>>(),
                         idx.as<uint32_t>(), pos.as<EdgePos>());
        });
    }
    sort_records(ctx, (int)W, ix->keys.p, tmp.p, idx.as<uint32_t>(), idx_tmp.as<uint32_t>(), n, key_passes(k1));
    BBK_HIP(hipMemsetAsync(dup.p, 0xFF, 8, ctx->stream));
    {
        KernelTimer timer(ctx, "edgeindex", (double)n * (2 * W * 8 + 2 * sizeof(EdgePos) + 4));
        dispatch_w(W, [&](auto w) {
            constexpr int W_ = decltype(w)::value;
            launch_items(ctx, "k_ep_gather", k_ep_gather<W_>, n, ix->keys.as<Key<W_>>(), idx.as<uint32_t>(),
                         pos.as<EdgePos>(), n, ix->pos.as<EdgePos>(), dup.as<unsigned long long>());
        });
    }
    uint64_t first_dup = ~0ull;
    d2h_sync(ctx, &first_dup, dup.p, 8);
    return first_dup;
}

static void report_duplicate(const bbk_edgeindex *ix, uint64_t first_dup) {
    EdgePos two[2];
    BBK_HIP(hipMemcpy(two, ix->pos.as<EdgePos>() + first_dup - 1, sizeof(two), hipMemcpyDeviceToHost));
    BBK_REQUIRE(false, BBK_ERR_ARG,
                "duplicated (k+1)-mer: segment %s offset %u and segment %s offset %u hold the same %u-mer (up to "
                "reverse complement); the mapping needs every (k+1)-mer of the graph once",
                ix->names[two[0].seg].c_str(), two[0].off_fw, ix->names[two[1].seg].c_str(), two[1].off_fw, ix->k1);
}

// the index of a graph held on the host, checked as the position-local form needs (gfa_graph.h): classify, check the
// links, flag the loops, keep or drop the graph, build on the device, report a duplicate, prefix table
static bbk_edgeindex *build_index(bbk_ctx *ctx, unsigned k, HostGraph &g, bool keep_graph) {
    BBK_REQUIRE(k >= 1 && k < BBK_MAX_K && k % 2 == 1, BBK_ERR_ARG, "edge index: k = %u must be odd and < %d", k, BBK_MAX_K);
    const uint64_t ns = g.names.size();
    BBK_REQUIRE(ns > 0, BBK_ERR_ARG, "edge index: the graph has no segments");
    BBK_REQUIRE(ns < (1ull << 32) - 1, BBK_ERR_ARG, "edge index: too many segments (%llu)", (unsigned long long)ns);
    auto ix = std::make_unique<bbk_edgeindex>();
    ix->k = k;
    ix->k1 = k + 1;
    ix->W = words_of(k + 1);
    ix->n_seg = ns;
    SegmentTable t(ns);
    require_graph(classify_segments(g, k, t));
    require_graph(check_links(g, k));
    flag_loops(g, k, t);
    ix->n = t.emit[ns];
    BBK_REQUIRE(ix->n < (1ull << 32), BBK_ERR_ARG, "edge index: %llu (k+1)-mers, at most 2^32 - 1 supported",
                (unsigned long long)ix->n);
    ix->len = std::move(t.len);
    ix->names = std::move(g.names);
    bbk_reads *sr = nullptr;
    int rc = bbk_reads_from_ascii(ctx, g.bases.data(), g.off.data(), ns, &sr);
    if (rc != BBK_OK) throw Error{rc};
    std::unique_ptr<bbk_reads, void (*)(bbk_reads *)> sr_guard(sr, bbk_reads_free);
    keep_or_drop_graph(ix.get(), g, keep_graph);
    const uint64_t first_dup = build_device_index(ctx, ix.get(), sr, t);
    if (first_dup != ~0ull) report_duplicate(ix.get(), first_dup);
    ix->prefix.build(ctx, ix->keys.as<uint64_t>(), ix->W, ix->k1, ix->n);
    return ix.release();
}

// pos_off[r] = (k+1)-mer positions before read r, pos_off[n] = total: npos kernel, scan (one wait), total staged from the
// caller's variable, which lives until the stream is waited for.  Returns total: 0 when there is nothing to map
static uint64_t read_positions(bbk_ctx *ctx, const bbk_edgeindex *ix, const bbk_reads *reads, DevBuf &pos_off,
                               uint64_t &total) {
    const uint64_t n = reads->n;
    if (n == 0 || ix->n == 0) return total = 0;
    pos_off.alloc((n + 1) * 8);
    launch_items(ctx, "k_ep_npos", k_ep_npos, n, reads->d_len, n, ix->k1, pos_off.as<uint64_t>());
    total = exclusive_scan_u64(ctx, pos_off.as<uint64_t>(), pos_off.as<uint64_t>(), n);
    if (total) BBK_HIP(hipMemcpyAsync(pos_off.as<uint64_t>() + n, &total, 8, hipMemcpyHostToDevice, ctx->stream));
    return total;
}

// One launch over waves of 63 positions (k_ep_map, k_gm_paths), timed as `family`; extra are the kernel's own arguments
template <int W, class K, class... Args>
static void launch_map(bbk_ctx *ctx, const char *family, const char *name, K fn, const bbk_reads *r,
                       const DevBuf &pos_off, uint64_t total, const bbk_edgeindex *ix, Args... extra) {
    const uint64_t waves = (total + kMapStep - 1) / kMapStep;
    // bytes the lookups need at the least: one prefix entry, the key and the record per position (each pass runs them)
    KernelTimer t(ctx, family, (double)total * (8.0 * W + sizeof(EdgePos) + 4));
    hipLaunchKernelGGL(fn, grid_blocks((waves + kMapWaves - 1) / kMapWaves), dim3(64 * kMapWaves), 0, ctx->stream, r->d_words,
                       r->d_woff, r->d_len, pos_off.as<uint64_t>(), r->n, total, (int)ix->k1, ix->keys.as<Key<W>>(),
                       ix->pos.as<EdgePos>(), ix->prefix.table(), extra...);
    check_launch(name);
}

}  // namespace bbk

using namespace bbk;

extern "C" {

static int from_gfa(bbk_ctx *ctx, const char *path, unsigned k, bbk_edgeindex **out, bool keep_graph) {
    return guarded([&] {
        BBK_REQUIRE(ctx && path && out, BBK_ERR_ARG, "bbk_edgeindex_from_gfa: NULL argument");
        BBK_REQUIRE(k >= 1 && k < BBK_MAX_K && k % 2 == 1, BBK_ERR_ARG, "bbk_edgeindex_from_gfa: k = %u must be odd and < %d",
                    k, BBK_MAX_K);
        BBK_HIP(hipSetDevice(ctx->device));
        HostGraph g;
        {
            std::string text;
            require_graph(read_whole_file(path, "cannot open graph %s", "reading graph %s failed", text));
            require_graph(parse_gfa_text(text.data(), text.data() + text.size(), k, path, g));
        }
        *out = build_index(ctx, k, g, keep_graph);
    });
}

int bbk_edgeindex_from_gfa(bbk_ctx *ctx, const char *path, unsigned k, bbk_edgeindex **out) {
    return from_gfa(ctx, path, k, out, false);
}

int bbk_edgeindex_from_gfa_with_graph(bbk_ctx *ctx, const char *path, unsigned k, bbk_edgeindex **out) {
    return from_gfa(ctx, path, k, out, true);
}

int bbk_edgeindex_from_unitigs(bbk_ctx *ctx, const bbk_unitigs *u, bbk_edgeindex **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && u && out, BBK_ERR_ARG, "bbk_edgeindex_from_unitigs: NULL argument");
        BBK_HIP(hipSetDevice(ctx->device));
        const uint64_t nu = bbk_unitigs_count(u), nl = bbk_unitigs_links(u);
        HostGraph g;
        g.bases.resize(bbk_unitigs_total_bases(u) + 1);
        g.off.resize(nu + 1);
        std::vector<uint32_t> hl(4 * nl + 1);
        int rc = bbk_unitigs_export(ctx, u, &g.bases[0], g.off.data());
        if (rc == BBK_OK) rc = bbk_unitigs_export_links(ctx, u, hl.data());
        if (rc != BBK_OK) throw Error{rc};
        g.names.resize(nu);
        for (uint64_t i = 0; i < nu; ++i) g.names[i] = std::to_string(3 + 2 * i);  // as bbk_unitigs_write_gfa names them
        g.links.resize(nl);
        for (uint64_t l = 0; l < nl; ++l) g.links[l] = {hl[4 * l], hl[4 * l + 2], hl[4 * l + 1] == 1, hl[4 * l + 3] == 1};
        *out = build_index(ctx, u->k, g, false);
    });
}

uint64_t bbk_edgeindex_segments(const bbk_edgeindex *ix) { return ix ? ix->n_seg : 0; }
uint64_t bbk_edgeindex_size(const bbk_edgeindex *ix) { return ix ? ix->n : 0; }
void bbk_edgeindex_free(bbk_edgeindex *ix) { delete ix; }

int bbk_profiles_begin(bbk_ctx *ctx, const bbk_edgeindex *ix, unsigned n_samples, bbk_profiles **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && ix && out, BBK_ERR_ARG, "bbk_profiles_begin: NULL argument");
        BBK_REQUIRE(n_samples >= 1, BBK_ERR_ARG, "bbk_profiles_begin: no samples");
        BBK_HIP(hipSetDevice(ctx->device));
        auto p = std::make_unique<bbk_profiles>();
        p->ctx = ctx;
        p->ix = ix;
        p->samples = n_samples;
        const size_t bytes = (size_t)ix->n_seg * n_samples * 8;
        p->raw.alloc(bytes);
        BBK_HIP(hipMemsetAsync(p->raw.p, 0, bytes, ctx->stream));
        BBK_HIP(hipStreamSynchronize(ctx->stream));
        *out = p.release();
    });
}

int bbk_profiles_push_reads(bbk_profiles *p, unsigned sample, const bbk_reads *reads) {
    return guarded([&] {
        BBK_REQUIRE(p && reads, BBK_ERR_ARG, "bbk_profiles_push_reads: NULL argument");
        BBK_REQUIRE(sample < p->samples, BBK_ERR_ARG, "bbk_profiles_push_reads: sample %u of %u", sample, p->samples);
        bbk_ctx *ctx = p->ctx;
        BBK_HIP(hipSetDevice(ctx->device));
        DevBuf pos_off;
        uint64_t total;
        if (read_positions(ctx, p->ix, reads, pos_off, total) == 0) return;
        dispatch_w(p->ix->W, [&](auto w) {
            constexpr int W_ = decltype(w)::value;
            launch_map<W_>(ctx, "edgeprof_map", "k_ep_map", k_ep_map<W_>, reads, pos_off, total, p->ix,
                           p->raw.as<unsigned long long>(), (uint32_t)p->samples, (uint32_t)sample);
        });
        BBK_HIP(hipStreamSynchronize(ctx->stream));  // pos_off and the staged total are released on return
    });
}

int bbk_profiles_export_raw(bbk_ctx *ctx, const bbk_profiles *p, uint64_t *h_raw) {
    return guarded([&] {
        BBK_REQUIRE(ctx && p && h_raw, BBK_ERR_ARG, "bbk_profiles_export_raw: NULL argument");
        BBK_HIP(hipSetDevice(ctx->device));
        d2h_sync(ctx, h_raw, p->raw.p, (size_t)p->ix->n_seg * p->samples * 8);
    });
}

// EdgeProfileStorage::Save (profile_storage.cpp:44-52): one line per segment (the canonical edge of each S line), in
// S-line order: name, then raw / length for every sample as std::ostream prints a double (%g), each followed by a tab
int bbk_profiles_write(bbk_ctx *ctx, const bbk_profiles *p, const char *path) {
    return guarded([&] {
        BBK_REQUIRE(ctx && p && path, BBK_ERR_ARG, "bbk_profiles_write: NULL argument");
        BBK_HIP(hipSetDevice(ctx->device));
        const bbk_edgeindex *ix = p->ix;
        const unsigned S = p->samples;
        std::vector<uint64_t> raw((size_t)ix->n_seg * S);
        d2h_sync(ctx, raw.data(), p->raw.p, raw.size() * 8);
        FILE *f = fopen(path, "wb");
        BBK_REQUIRE(f, BBK_ERR_IO, "cannot open %s for writing", path);
        std::unique_ptr<FILE, int (*)(FILE *)> guard(f, fclose);
        const int nt = std::max(1, std::min(omp_get_max_threads(), 16));
        const bool ok = format_blocks(
            ix->n_seg, nt, (uint64_t)nt, [&](const std::string &t) { return fwrite(t.data(), 1, t.size(), f) == t.size(); },
            [&](uint64_t s, std::string &o) {
                char num[32];
                o += ix->names[s];
                o += '\t';
                for (unsigned i = 0; i < S; ++i)
                    o.append(num, (size_t)snprintf(num, sizeof(num), "%g\t", (double)raw[s * S + i] / (double)ix->len[s]));
                o += '\n';
            });
        BBK_REQUIRE(ok, BBK_ERR_IO, "short write to %s", path);
        FILE *fo = guard.release();
        BBK_REQUIRE(fclose(fo) == 0, BBK_ERR_IO, "closing %s failed", path);
    });
}

void bbk_profiles_free(bbk_profiles *p) { delete p; }

int bbk_edgeindex_map_paths(bbk_ctx *ctx, const bbk_edgeindex *ix, const bbk_reads *reads, bbk_paths **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && ix && reads && out, BBK_ERR_ARG, "bbk_edgeindex_map_paths: NULL argument");
        BBK_REQUIRE(reads->n < (1ull << 32), BBK_ERR_ARG, "bbk_edgeindex_map_paths: %llu reads, at most 2^32 - 1 per batch",
                    (unsigned long long)reads->n);
        BBK_HIP(hipSetDevice(ctx->device));
        auto p = std::make_unique<bbk_paths>();
        p->n_reads = reads->n;
        DevBuf pos_off;
        uint64_t total;
        if (read_positions(ctx, ix, reads, pos_off, total) > 0) {
            const uint64_t waves = (total + kMapStep - 1) / kMapStep;
            DevBuf wave_cnt(waves * 8);
            auto run = [&](auto write) {  // one pass of k_gm_paths: count the range starts per wave, or write the ranges
                dispatch_w(ix->W, [&](auto w) {
                    constexpr int W_ = decltype(w)::value;
                    constexpr bool WRITE = decltype(write)::value;
                    launch_map<W_>(ctx, WRITE ? "gmap_write" : "gmap_count", "k_gm_paths", k_gm_paths<W_, WRITE>, reads,
                                   pos_off, total, ix, wave_cnt.as<uint64_t>(), p->ranges.as<bbk_path_range>());
                });
            };
            run(std::false_type{});
            p->n_ranges = exclusive_scan_u64(ctx, wave_cnt.as<uint64_t>(), wave_cnt.as<uint64_t>(), waves);
            p->ranges.alloc(p->n_ranges * sizeof(bbk_path_range));
            if (p->n_ranges) run(std::true_type{});
            BBK_HIP(hipStreamSynchronize(ctx->stream));  // pos_off, wave_cnt and the staged total die here
        }
        *out = p.release();
    });
}

uint64_t bbk_paths_reads(const bbk_paths *p) { return p ? p->n_reads : 0; }
uint64_t bbk_paths_ranges(const bbk_paths *p) { return p ? p->n_ranges : 0; }

int bbk_paths_export(bbk_ctx *ctx, const bbk_paths *p, uint64_t *h_read_offsets, bbk_path_range *h_ranges) {
    return guarded([&] {
        BBK_REQUIRE(ctx && p, BBK_ERR_ARG, "bbk_paths_export: NULL argument");
        BBK_HIP(hipSetDevice(ctx->device));
        std::vector<bbk_path_range> tmp;
        bbk_path_range *r = h_ranges;
        if (!r && h_read_offsets) {
            tmp.resize(p->n_ranges);
            r = tmp.data();
        }
        if (r && p->n_ranges) d2h_sync(ctx, r, p->ranges.p, p->n_ranges * sizeof(bbk_path_range));
        if (h_read_offsets) {  // the ranges are in read order: count them per read
            std::fill(h_read_offsets, h_read_offsets + p->n_reads + 1, 0ull);
            for (uint64_t i = 0; i < p->n_ranges; ++i) ++h_read_offsets[r[i].read + 1];
            for (uint64_t i = 0; i < p->n_reads; ++i) h_read_offsets[i + 1] += h_read_offsets[i];
        }
    });
}

void bbk_paths_free(bbk_paths *p) { delete p; }

uint64_t bbk_edgeindex_links(const bbk_edgeindex *ix) { return ix ? ix->links.size() / 4 : 0; }
uint64_t bbk_edgeindex_total_bases(const bbk_edgeindex *ix) { return ix ? ix->bases.size() : 0; }
const char *bbk_edgeindex_name(const bbk_edgeindex *ix, uint64_t segment) {
    return ix && segment < ix->n_seg ? ix->names[segment].c_str() : nullptr;
}

int bbk_edgeindex_export_segments(const bbk_edgeindex *ix, uint64_t *h_len, uint8_t *h_self_conjugate) {
    return guarded([&] {
        BBK_REQUIRE(ix, BBK_ERR_ARG, "bbk_edgeindex_export_segments: NULL index");
        if (h_len) std::copy(ix->len.begin(), ix->len.end(), h_len);
        if (h_self_conjugate)
            for (uint64_t s = 0; s < ix->n_seg; ++s) h_self_conjugate[s] = edge_self_conj(ix->seg_h[s]) ? 1 : 0;
    });
}

int bbk_edgeindex_export_graph(const bbk_edgeindex *ix, char *h_bases, uint64_t *h_offsets, uint32_t *h_links,
                               uint32_t *h_kc) {
    return guarded([&] {
        BBK_REQUIRE(ix, BBK_ERR_ARG, "bbk_edgeindex_export_graph: NULL index");
        BBK_REQUIRE(ix->has_graph, BBK_ERR_ARG,
                    "bbk_edgeindex_export_graph: the index keeps no graph (load it with bbk_edgeindex_from_gfa_with_graph)");
        if (h_bases) memcpy(h_bases, ix->bases.data(), ix->bases.size());
        if (h_offsets) memcpy(h_offsets, ix->off.data(), ix->off.size() * 8);
        if (h_links) memcpy(h_links, ix->links.data(), ix->links.size() * 4);
        if (h_kc) memcpy(h_kc, ix->kc.data(), ix->kc.size() * 4);
    });
}

}  // extern "C"
