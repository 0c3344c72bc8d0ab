// distest.hip -- DistanceEstimation for a paired-end library: the raw paired index of pairinfo.hip clustered on the graph
// distances between the two edges of every stored pair (reference projects/spades/distance_estimation.cpp:137-154:
// DistanceEstimator and the weight filter; RefinePairedInfo cannot fire on this output and PairInfoImprover is a
// follow-up).
//
// Replaces, per stored (canonical) edge pair of the index:
//   GraphDistanceFinder::FillGraphDistancesLengths (common/paired_info/distance_estimation.cpp:17-45): the bounded Dijkstra
//   from EdgeEnd(e1) and PathProcessor::Traversal with DistancesLengthsCallback
//   (assembly_graph/paths/path_processor.hpp:56-181, 380-402)                                             -> k_de_walk
//   DistanceEstimator::EstimateEdgePairDistances (:97-150), ClusterResult (:51-67), the fourfold weight of a pair that is
//   its own conjugate (AddMany into the thread's buffer, Merge into the result: paired_info_buffer.hpp:63-68, 103-133)
//   and PairInfoWeightChecker (pair_info_filters.hpp:42-56)                                               -> k_de_estimate
//
// The order-free rule.  Go(v) is called once per walk that runs backwards from EdgeStart(e2), every prefix of which passes
// dist(start) + length <= U: B[v][l] of the recurrence in tests/distest_restated.py counts them, and their number is the
// sum of B.  The limits of the search are 3000 calls, and from call 500 on 5 uses of a vertex: below 500 calls neither
// fires, so the set of lengths found does not depend on the order the incoming edges are tried in, as long as the
// Dijkstra stayed below its limit of 3000 vertices (it stops expanding at 2999).  k_de_walk enumerates exactly these
// walks, one worklist item per call, so its item count IS the call count: 500 items or more and the pair is left to the
// host, which runs the literal search (distest_host.hpp).  One pass gives the lengths and the proof that they are
// order-free.  (The recurrence is evaluated sparsely: a pair the device keeps has fewer than 500 non-zero B in all, where
// the dense table has |ball| x (U + 1) cells.)
//
// Shape.  The raw points are ascending (e1, e2, gap), so the pairs of one first edge are consecutive.  k_de_walk runs one
// wave per first edge: the ball (the vertices within U of EdgeEnd(e1), with their distances) is built once in LDS as an
// open-addressing table by synchronous relaxation rounds to a fixed point (a slot whose distance dropped in round r is
// relaxed in round r + 1), then the second edges take turns at the walk, 64 items at a time.  The lengths of a pair leave
// as a bitmap of U + 1 bits, which is also how the host hands back the pairs it searched; k_de_estimate, one lane per
// pair, streams the set bits in ascending order against the ascending points, so it holds no list of either.
// Capacities, fixed so that the tables stay in LDS at 14 KB a wave (11 waves a CU): kDeBallCap = 512 vertices in a ball
// (1024 slots: the table stays at most 56 % full with 64 claims in flight), kDeUCap = 2047 for U (64 bitmap words).  A
// ball of 513 vertices or more, or a U of 2048 or more, goes to the host, as does everything under BBK_NO_DISTEST_DEVICE.
//
// Weights are integer half-units in u64 (an exact tie gives half of a point's weight to each neighbour), so the result
// is exact and independent of order; the reference sums floats, equal while a sum stays below 2^23.  Distances are
// integers; the reference holds them as floats and compares within 4 ULPs, the same below 2^21.
//
// Where the rest lives.  The rules of an edge and the lower bound of a path length: edge_ops.h.  The point table, its
// grouping into pairs and first edges, the weight threshold in half-units, the import's canonicalise-sort-merge and the
// writer of the file: pairinfo_host.hpp.  bbk_pairinfo_cluster is a sequence of phases, each a function below:
// cluster_params, group_pairs + upload_pairs, walk_on_device, search_on_host, estimate_clusters.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "bbk_internal.h"
#include "distest_host.hpp"
#include "edgeindex.h"

namespace bbk {

constexpr uint32_t kDeBallCap = 512, kDeSlots = 1024, kDeUCap = 2047, kDeWords = 64, kDeItems = 512;
constexpr uint32_t kDeEmpty = 0xFFFFFFFFu, kDeNone = 0xFFFFFFFFu;
static_assert(kDeSlots >= kDeBallCap + 64 + 1, "a probe must always reach an empty slot");
static_assert(kDeItems >= kDeUsageThreshold && (kDeUCap >> 5) + 1 == kDeWords, "worklist and bitmap sizes");

// the graph on the device: the CSR of the edges that start at a vertex, and both vertices of every oriented edge
struct DeDeviceGraph {
    DeGraph h;
    DevBuf out_off, out_e, e_end, e_start;
};

struct DeGraphView {
    const uint32_t *__restrict__ out_off, *__restrict__ out_e, *__restrict__ e_end, *__restrict__ e_start;
    const uint32_t *__restrict__ seg;
};

struct DeRec {  // one cluster
    uint64_t e1, e2;
    float centre, var;
    uint64_t weight;  // half-units
};

struct DeParams {
    uint32_t k, U, words;  // words = (U >> 5) + 1 per bitmap row
    int64_t gap;           // int(insert_size - 2 * read_length)
    uint64_t delta, linkage, max_distance, min_weight;  // min_weight: the least half-units that pass the filter
};

__device__ inline uint32_t de_slot(uint32_t v) { return (v * 2654435761u) >> 22; }  // 10 bits: kDeSlots

__device__ inline uint32_t de_lookup(const uint32_t *key, const uint32_t *dist, uint32_t v) {
    uint32_t s = de_slot(v);
    for (uint32_t probe = 0; probe < kDeSlots; ++probe) {
        const uint32_t x = key[s];
        if (x == v) return dist[s];
        if (x == kDeEmpty) return kDeNone;
        s = (s + 1) & (kDeSlots - 1);
    }
    return kDeNone;
}

// dist(v) = min(dist(v), nd), v entering the table when it is new; a lowered distance marks the slot for the next round
__device__ inline void de_relax(uint32_t *key, uint32_t *dist, uint8_t *mark, uint32_t *count, uint32_t *overflow,
                                uint32_t v, uint32_t nd) {
    uint32_t s = de_slot(v);
    for (uint32_t probe = 0; probe < kDeSlots; ++probe) {
        uint32_t x = __hip_atomic_load(&key[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (x == kDeEmpty) {
            if (__hip_atomic_load(count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= kDeBallCap) {
                *overflow = 1;  // (at most 64 lanes pass this check together: the table never holds more than cap + 64)
                return;
            }
            x = atomicCAS(&key[s], kDeEmpty, v);
            if (x == kDeEmpty) {
                atomicAdd(count, 1u);
                x = v;
            }
        }
        if (x == v) {
            if (nd < atomicMin(&dist[s], nd)) mark[s] = 1;
            return;
        }
        s = (s + 1) & (kDeSlots - 1);
    }
    *overflow = 1;
}

// One wave per first edge (header comment).  grp[g] .. grp[g + 1]: its pairs; rows: words u32 per pair, bit l set for a
// walk length l in [min_len, U] from EdgeEnd(e1) to EdgeStart(e2); hard[p] = 1: left to the host (the row is zero).
__global__ __launch_bounds__(64) void k_de_walk(uint64_t ng, const uint32_t *__restrict__ grp,
                                                const uint32_t *__restrict__ pair_e1, const uint32_t *__restrict__ pair_e2,
                                                DeGraphView G, DeParams P, uint32_t *__restrict__ rows,
                                                uint32_t *__restrict__ hard) {
    __shared__ uint32_t key[kDeSlots], dist[kDeSlots];
    __shared__ uint8_t mark[2][kDeSlots];
    __shared__ uint32_t wl_v[kDeItems], wl_l[kDeItems], bits[kDeWords];
    __shared__ uint32_t count, overflow, tail;
    const uint64_t g = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (g >= ng) return;
    const uint32_t lane = threadIdx.x, p0 = grp[g], p1 = grp[g + 1];
    const uint32_t e1 = pair_e1[p0], s0 = G.e_end[e1], len1 = edge_length(G.seg[e1 >> 1]);
    for (uint32_t s = lane; s < kDeSlots; s += 64) {
        key[s] = kDeEmpty;
        dist[s] = kDeNone;
        mark[0][s] = mark[1][s] = 0;
    }
    if (lane == 0) overflow = 0;
    __syncthreads();
    if (lane == 0) {
        const uint32_t s = de_slot(s0);
        key[s] = s0;
        dist[s] = 0;
        mark[0][s] = 1;
        count = 1;
    }
    __syncthreads();
    for (int cur = 0;; cur ^= 1) {  // relaxation rounds to the fixed point
        bool took = false;
        for (uint32_t s = lane; s < kDeSlots; s += 64) {
            if (!mark[cur][s]) continue;
            mark[cur][s] = 0;
            took = true;
            const uint32_t v = key[s], d = __hip_atomic_load(&dist[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            for (uint32_t i = G.out_off[v]; i < G.out_off[v + 1]; ++i) {
                const uint32_t e = G.out_e[i];
                const uint64_t nd = (uint64_t)d + edge_length(G.seg[e >> 1]);
                if (nd <= P.U) de_relax(key, dist, mark[cur ^ 1], &count, &overflow, G.e_end[e], (uint32_t)nd);
            }
        }
        if (!__syncthreads_or(took)) break;
    }
    const bool too_big = overflow != 0 || count > kDeBallCap;

    for (uint32_t p = p0; p < p1; ++p) {
        const uint32_t e2 = pair_e2[p], t = G.e_start[e2], len2 = edge_length(G.seg[e2 >> 1]);
        // no walk is longer than U: a bound beyond it is as good as U + 1, which fits the worklist's 32-bit lengths
        const uint64_t lb = path_length_lower_bound(P.k, len1, len2, P.gap, P.delta);
        const uint32_t min_len = lb > P.U ? P.U + 1 : (uint32_t)lb;
        bits[lane] = 0;
        bool is_hard = too_big;
        const bool reached = !too_big && de_lookup(key, dist, t) != kDeNone;
        if (lane == 0) {
            wl_v[0] = t;
            wl_l[0] = 0;
            tail = reached ? 1 : 0;
        }
        __syncthreads();
        for (uint32_t head = 0;;) {
            const uint32_t tl = tail;
            __syncthreads();  // every lane has read the tail before a lane moves it
            if (tl >= kDeUsageThreshold) {
                is_hard = true;
                break;
            }
            if (head >= tl) break;
            const uint32_t n = min(64u, tl - head);
            if (lane < n) {
                const uint32_t v = wl_v[head + lane], l = wl_l[head + lane];
                if (v == s0 && l >= min_len) atomicOr(&bits[l >> 5], 1u << (l & 31));
                // IncomingEdges(v): the conjugates of the edges that start at conj v
                for (uint32_t i = G.out_off[v ^ 1u]; i < G.out_off[(v ^ 1u) + 1]; ++i) {
                    const uint32_t ec = G.out_e[i], sv = G.e_end[ec] ^ 1u;
                    const uint64_t ln = edge_length(G.seg[ec >> 1]);
                    const uint32_t d = de_lookup(key, dist, sv);
                    if (d == kDeNone || (uint64_t)d + ln + l > P.U) continue;
                    const uint32_t at = atomicAdd(&tail, 1u);
                    if (at < kDeItems) {
                        wl_v[at] = sv;
                        wl_l[at] = l + (uint32_t)ln;
                    }
                }
            }
            head += n;
            __syncthreads();
        }
        if (lane < P.words) rows[(uint64_t)p * P.words + lane] = is_hard ? 0u : bits[lane];
        if (lane == 0) hard[p] = is_hard ? 1u : 0u;
        __syncthreads();
    }
}

// rows of the pairs the host searched, into their places
__global__ __launch_bounds__(256) void k_de_scatter(uint64_t n_words, uint32_t words, const uint32_t *__restrict__ idx,
                                                   const uint32_t *__restrict__ src, uint32_t *__restrict__ rows) {
    const uint64_t i = BBK_GID();
    if (i < n_words) rows[(uint64_t)idx[i / words] * words + i % words] = src[i];
}

__device__ inline bool de_near(int64_t f, int64_t d, int64_t md) { return (f > d ? f - d : d - f) <= md; }

// the kept graph lengths of a pair in ascending order: 0 for e1 == e2, then len1 + l for every set bit l, each within
// [lo, hi] (EstimateEdgePairDistances keeps a length iff minD - max_distance <= length <= maxD + max_distance)
struct DeLengths {
    const uint32_t *row;
    uint32_t words, word_at;
    uint32_t cur;  // the unread bits of word word_at
    int64_t len1, lo, hi;
    bool zero;
    __device__ bool next(int64_t &out) {
        if (zero) {
            zero = false;
            if (lo <= 0 && 0 <= hi) {
                out = 0;
                return true;
            }
        }
        for (;;) {
            while (cur == 0) {
                if (++word_at >= words) return false;
                cur = row[word_at];
            }
            const uint32_t b = (uint32_t)__ffs((int)cur) - 1u;
            cur &= cur - 1;
            const int64_t L = len1 + (int64_t)word_at * 32 + b;
            if (L > hi) return false;
            if (L >= lo) {
                out = L;
                return true;
            }
        }
    }
};

// ClusterResult over the estimated (length, weight) pairs as they arrive, then the fourfold weight and the filter
template <bool WRITE>
struct DeClusters {
    int64_t left = 0, last = 0, linkage;
    uint64_t weight = 0, times, min_weight, n = 0, e1, e2;
    bool open = false;
    DeRec *out;
    __device__ void flush() {
        if (!open) return;
        const uint64_t w = weight * times;
        if (w >= min_weight) {
            if constexpr (WRITE) {
                DeRec r;
                r.e1 = e1;
                r.e2 = e2;
                r.centre = (float)((double)(left + last) * 0.5);
                // ClusterResult computes (last - left) / 2, and AddToResult loses it: the thread's buffer holds raw points
                // (PairedInfoBuffer has RawPointTraits, paired_info.hpp:711-712), so AddMany slices the variance off and
                // Merge restores it as 0 (index_point.hpp:228-229).  Every cluster of the reference has variance 0
                r.var = 0.0f;
                r.weight = w;
                out[n] = r;
            }
            ++n;
        }
        open = false;
    }
    __device__ void add(int64_t f, uint64_t w) {
        if (open && f - last <= linkage) {
            last = f;
            weight += w;
            return;
        }
        flush();
        open = true;
        left = last = f;
        weight = w;
    }
};

// One lane per pair: its points pt[pair_pt[p] .. pair_pt[p + 1]) (ascending gap) against its lengths.  WRITE = false: the
// clusters that pass to cnt[p]; WRITE = true: cnt holds their exclusive scan and the clusters are written from there.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_de_estimate(uint64_t np, const uint32_t *__restrict__ pair_e1,
                                                    const uint32_t *__restrict__ pair_e2, const uint32_t *__restrict__ pair_pt,
                                                    const int32_t *__restrict__ pt_gap, const uint64_t *__restrict__ pt_w,
                                                    const uint32_t *__restrict__ seg, DeParams P,
                                                    const uint32_t *__restrict__ rows, uint64_t *__restrict__ cnt,
                                                    DeRec *__restrict__ out) {
    const uint64_t p = BBK_GID();
    if (p >= np) return;
    const uint32_t e1 = pair_e1[p], e2 = pair_e2[p], a = pair_pt[p], b = pair_pt[p + 1];
    const uint32_t s1 = seg[e1 >> 1], s2 = seg[e2 >> 1];
    const int64_t len1 = edge_length(s1), len2 = edge_length(s2), md = (int64_t)P.max_distance;
    DeClusters<WRITE> cl;
    cl.linkage = (int64_t)P.linkage;
    cl.times = pair_is_self_conj(e1, e2, seg) ? 4 : 1;
    cl.min_weight = P.min_weight;
    cl.e1 = e1;
    cl.e2 = e2;
    cl.out = WRITE ? out + cnt[p] : nullptr;
    DeLengths it;
    it.row = rows + p * P.words;
    it.words = P.words;
    it.word_at = 0;
    it.cur = it.row[0];
    it.len1 = len1;
    it.lo = (int64_t)pt_gap[a] + len1 - md;
    it.hi = (int64_t)pt_gap[b - 1] + len1 + md;
    it.zero = e1 == e2;
    int64_t f_cur, f_next = 0;
    if (it.next(f_cur)) {
        uint64_t w_cur = 0;
        bool has_next = it.next(f_next);
        auto shift = [&] {
            cl.add(f_cur, w_cur);
            f_cur = f_next;
            w_cur = 0;
            has_next = it.next(f_next);
        };
        for (uint32_t i = a; i < b; ++i) {
            const int64_t d = (int64_t)pt_gap[i] + len1;
            const uint64_t w = 2 * pt_w[i];
            if (2 * d + len2 < len1) continue;
            while (has_next && f_next < d) shift();
            if (has_next && f_next - d < d - f_cur) {
                shift();
                if (de_near(f_cur, d, md)) w_cur += w;
            } else if (has_next && f_next - d == d - f_cur) {
                if (de_near(f_cur, d, md)) w_cur += w / 2;
                shift();
                if (de_near(f_cur, d, md)) w_cur += w / 2;
            } else if (de_near(f_cur, d, md)) {
                w_cur += w;
            }
        }
        cl.add(f_cur, w_cur);
        while (has_next) {
            cl.add(f_next, 0);
            has_next = it.next(f_next);
        }
        cl.flush();
    }
    if constexpr (!WRITE) cnt[p] = cl.n;
}

// ---- host ---------------------------------------------------------------------------------------------------------------

// a host array to the device on the stream; the array stays until the stream has been waited for
template <class T>
static void upload(bbk_ctx *ctx, DevBuf &d, const std::vector<T> &v) {
    d.alloc(v.size() * sizeof(T));
    if (!v.empty()) BBK_HIP(hipMemcpyAsync(d.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
}

static std::shared_ptr<DeDeviceGraph> device_graph(bbk_ctx *ctx, const bbk_edgeindex *ix) {
    std::lock_guard<std::mutex> lock(ix->de_mutex);
    if (ix->de_graph) return ix->de_graph;
    BBK_REQUIRE(ix->n_seg < (1ull << 30), BBK_ERR_ARG, "bbk_pairinfo_cluster: %llu segments, at most 2^30 - 1 are supported",
                (unsigned long long)ix->n_seg);
    auto g = std::make_shared<DeDeviceGraph>();
    de_build_graph(ix->k, ix->n_seg, ix->seg_h.data(), ix->links.data(), ix->links.size() / 4, ix->kc.data(), g->h);
    upload(ctx, g->out_off, g->h.out_off);
    upload(ctx, g->out_e, g->h.out_e);
    upload(ctx, g->e_end, g->h.end);
    upload(ctx, g->e_start, g->h.start);
    BBK_HIP(hipStreamSynchronize(ctx->stream));
    ix->de_graph = g;
    return g;
}

// ---- the phases of bbk_pairinfo_cluster ---------------------------------------------------------------------------------

// the checks on the parameters of a call and the integers every phase reads
static DeParams cluster_params(const bbk_edgeindex *ix, const bbk_cluster_params *prm) {
    BBK_REQUIRE(ix->has_graph, BBK_ERR_ARG,
                "bbk_pairinfo_cluster: the index keeps no graph (load it with bbk_edgeindex_from_gfa_with_graph)");
    // PairInfoPathLengthUpperBound's VERIFY (pair_info_bounds.hpp:16-21)
    BBK_REQUIRE(prm->insert_size + prm->delta > (uint64_t)ix->k + 2, BBK_ERR_ARG,
                "bbk_pairinfo_cluster: insert_size %llu + delta %llu - k %u - 2 is not positive",
                (unsigned long long)prm->insert_size, (unsigned long long)prm->delta, ix->k);
    const uint64_t U = prm->insert_size + prm->delta - ix->k - 2;
    BBK_REQUIRE(U < (1ull << 24) && prm->insert_size < (1ull << 24) && prm->read_length < (1ull << 24) &&
                    prm->max_distance < (1ull << 24) && prm->linkage_distance < (1ull << 24),
                BBK_ERR_ARG, "bbk_pairinfo_cluster: a distance parameter of 2^24 or more");
    BBK_REQUIRE(!std::isnan(prm->filter_threshold), BBK_ERR_ARG, "bbk_pairinfo_cluster: filter_threshold is not a number");
    DeParams P{};
    P.k = ix->k;
    P.U = (uint32_t)U;
    P.words = (uint32_t)(U >> 5) + 1;
    P.gap = (int64_t)prm->insert_size - 2 * (int64_t)prm->read_length;
    P.delta = prm->delta;
    P.linkage = prm->linkage_distance;
    P.max_distance = prm->max_distance;
    P.min_weight = least_half_units(prm->filter_threshold);
    return P;
}

// the pairs and the first edges of the ascending points (pair_groups, pairinfo_host.hpp) and what the kernels read of
// them; the host arrays live as long as their copies may be in flight
struct DePairs {
    PairGroups h;
    uint64_t n = 0, np = 0, ng = 0;  // points, pairs, first edges
    DevBuf pe1, pe2, ppt, grp, gap, w;
};

static DePairs group_pairs(const PairPoints &pt) {
    DePairs d;
    d.n = pt.size();
    BBK_REQUIRE(d.n < (1ull << 32) - 1, BBK_ERR_ARG, "bbk_pairinfo_cluster: 2^32 - 1 points or more");
    d.h = pair_groups(pt);
    d.np = d.h.pairs();
    d.ng = d.h.firsts();
    return d;
}

static void upload_pairs(bbk_ctx *ctx, const PairPoints &pt, DePairs &d) {
    upload(ctx, d.pe1, d.h.pe1);
    upload(ctx, d.pe2, d.h.pe2);
    upload(ctx, d.ppt, d.h.ppt);
    upload(ctx, d.grp, d.h.grp);
    upload(ctx, d.gap, pt.gap);
    upload(ctx, d.w, pt.weight);
}

// k_de_walk over every first edge: the rows of the pairs it finished; returns hard[p] = 1 for those it left to the host,
// which is every pair under the A/B switch BBK_NO_DISTEST_DEVICE or with U beyond the bitmap
static std::vector<uint32_t> walk_on_device(bbk_ctx *ctx, const bbk_edgeindex *ix, const DeDeviceGraph &G, const DePairs &d,
                                            const DeParams &P, DevBuf &rows) {
    std::vector<uint32_t> hard(d.np, 1);
    if (getenv("BBK_NO_DISTEST_DEVICE") != nullptr || P.U > kDeUCap) return hard;
    DevBuf d_hard(d.np * 4);
    const DeGraphView V{G.out_off.as<uint32_t>(), G.out_e.as<uint32_t>(), G.e_end.as<uint32_t>(), G.e_start.as<uint32_t>(),
                        ix->seg.as<uint32_t>()};
    {
        KernelTimer t(ctx, "distest_walk", (double)d.np * P.words * 4);
        hipLaunchKernelGGL(k_de_walk, grid_blocks(d.ng), dim3(64), 0, ctx->stream, d.ng, d.grp.as<uint32_t>(),
                           d.pe1.as<uint32_t>(), d.pe2.as<uint32_t>(), V, P, rows.as<uint32_t>(), d_hard.as<uint32_t>());
        check_launch("k_de_walk");
    }
    d2h_sync(ctx, hard.data(), d_hard.p, d.np * 4);
    return hard;
}

// the host's pairs: one Dijkstra per first edge that has any, the literal search per pair (distest_host.hpp), and their
// rows scattered into their places; returns how many there were
static uint64_t search_on_host(bbk_ctx *ctx, const DeGraph &g, const DePairs &d, const DeParams &P,
                               const std::vector<uint32_t> &hard, DevBuf &rows) {
    const std::vector<uint32_t> &pe1 = d.h.pe1, &pe2 = d.h.pe2;
    std::vector<uint32_t> hidx;
    for (uint64_t p = 0; p < d.np; ++p)
        if (hard[p]) hidx.push_back((uint32_t)p);
    const uint64_t nh = hidx.size();
    if (nh == 0) return 0;
    std::vector<uint32_t> hrows(nh * P.words, 0);
    std::vector<uint64_t> first;  // where the pairs of a first edge begin in hidx
    for (uint64_t i = 0; i < nh; ++i)
        if (!i || pe1[hidx[i]] != pe1[hidx[i - 1]]) first.push_back(i);
    first.push_back(nh);
#pragma omp parallel num_threads(16)
    {
        DeSearch s(g);
#pragma omp for schedule(dynamic, 1)
        for (int64_t f = 0; f < (int64_t)first.size() - 1; ++f) {
            const uint32_t e1 = pe1[hidx[first[f]]];
            s.dijkstra(g.end[e1], P.U);
            for (uint64_t i = first[f]; i < first[f + 1]; ++i) {
                const uint32_t e2 = pe2[hidx[i]];
                s.lengths(g.end[e1], g.start[e2], path_length_lower_bound(P.k, g.length(e1), g.length(e2), P.gap, P.delta),
                          &hrows[i * P.words]);
            }
        }
    }
    DevBuf d_hidx, d_hrows;
    upload(ctx, d_hidx, hidx);
    upload(ctx, d_hrows, hrows);
    launch_items(ctx, "k_de_scatter", k_de_scatter, nh * P.words, nh * P.words, P.words, d_hidx.as<uint32_t>(),
                 d_hrows.as<uint32_t>(), rows.as<uint32_t>());
    BBK_HIP(hipStreamSynchronize(ctx->stream));  // the host vectors leave scope
    return nh;
}

// count, scan and write of k_de_estimate, then the clusters on the host
static std::vector<DeRec> estimate_clusters(bbk_ctx *ctx, const bbk_edgeindex *ix, const DePairs &d, const DeParams &P,
                                            const DevBuf &rows) {
    DevBuf cnt(d.np * 8), rec;
    auto estimate = [&](auto write, DeRec *o) {
        KernelTimer t(ctx, "distest_estimate", (double)d.n * 12 + (double)d.np * P.words * 4);
        launch_items(ctx, "k_de_estimate", k_de_estimate<decltype(write)::value>, d.np, d.np, d.pe1.as<uint32_t>(),
                     d.pe2.as<uint32_t>(), d.ppt.as<uint32_t>(), d.gap.as<int32_t>(), d.w.as<uint64_t>(),
                     ix->seg.as<uint32_t>(), P, rows.as<uint32_t>(), cnt.as<uint64_t>(), o);
    };
    estimate(std::false_type{}, nullptr);
    const uint64_t total = exclusive_scan_u64(ctx, cnt.as<uint64_t>(), cnt.as<uint64_t>(), d.np);
    std::vector<DeRec> recs(total);
    if (total) {
        rec.alloc(total * sizeof(DeRec));
        estimate(std::true_type{}, rec.as<DeRec>());
        d2h_big(ctx, recs.data(), rec.p, total * sizeof(DeRec));
    }
    BBK_HIP(hipStreamSynchronize(ctx->stream));
    return recs;
}

}  // namespace bbk

using namespace bbk;

struct bbk_clustered {
    const bbk_edgeindex *ix = nullptr;
    std::vector<DeRec> recs;  // as k_de_estimate wrote them: ascending (e1, e2, centre)
    uint64_t pairs = 0, host_pairs = 0;
};

extern "C" {

int bbk_pairinfo_import(bbk_ctx *ctx, const bbk_edgeindex *ix, uint64_t n, const uint64_t *h_e1, const uint64_t *h_e2,
                        const int32_t *h_gap, const uint64_t *h_weight, bbk_pairinfo **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && ix && out && (n == 0 || (h_e1 && h_e2 && h_gap && h_weight)), BBK_ERR_ARG,
                    "bbk_pairinfo_import: NULL argument");
        bbk_pairinfo *made = nullptr;
        const int rc = bbk_pairinfo_begin(ctx, ix, 0, &made);
        if (rc != BBK_OK) throw Error{rc};
        std::unique_ptr<bbk_pairinfo> pi(made);
        for (uint64_t i = 0; i < n; ++i)
            for (const uint64_t e : {h_e1[i], h_e2[i]})
                BBK_REQUIRE(e < 2 * ix->n_seg && edge_exists(e, ix->seg_h[e >> 1]), BBK_ERR_ARG,
                            "bbk_pairinfo_import: point %llu names edge %llu, which the graph does not have",
                            (unsigned long long)i, (unsigned long long)e);
        pi->points = canonical_points(n, h_e1, h_e2, h_gap, h_weight, ix->seg_h.data());
        pi->filled = true;
        *out = pi.release();
    });
}

int bbk_pairinfo_cluster(bbk_pairinfo *pi, const bbk_cluster_params *prm, bbk_clustered **out) {
    return guarded([&] {
        BBK_REQUIRE(pi && prm && out, BBK_ERR_ARG, "bbk_pairinfo_cluster: NULL argument");
        BBK_REQUIRE(pi->filled, BBK_ERR_ARG, "bbk_pairinfo_cluster: before bbk_pairinfo_fill_finish");
        const bbk_edgeindex *ix = pi->ix;
        const DeParams P = cluster_params(ix, prm);
        bbk_ctx *ctx = pi->ctx;
        BBK_HIP(hipSetDevice(ctx->device));
        const std::shared_ptr<DeDeviceGraph> G = device_graph(ctx, ix);

        DePairs d = group_pairs(pi->points);
        auto res = std::make_unique<bbk_clustered>();
        res->ix = ix;
        res->pairs = d.np;
        if (d.np == 0) {
            *out = res.release();
            return;
        }
        BBK_REQUIRE(d.np * (uint64_t)P.words < (1ull << 32), BBK_ERR_ARG,
                    "bbk_pairinfo_cluster: %llu pairs at %u length words each: 2^32 words or more", (unsigned long long)d.np,
                    P.words);
        upload_pairs(ctx, pi->points, d);
        DevBuf rows(d.np * P.words * 4);  // per pair the bitmap of its walk lengths
        const std::vector<uint32_t> hard = walk_on_device(ctx, ix, *G, d, P, rows);
        res->host_pairs = search_on_host(ctx, G->h, d, P, hard, rows);
        res->recs = estimate_clusters(ctx, ix, d, P, rows);
        *out = res.release();
    });
}

uint64_t bbk_clustered_points(const bbk_clustered *c) { return c ? c->recs.size() : 0; }
uint64_t bbk_clustered_pairs(const bbk_clustered *c) { return c ? c->pairs : 0; }
uint64_t bbk_clustered_host_pairs(const bbk_clustered *c) { return c ? c->host_pairs : 0; }

int bbk_clustered_export(const bbk_clustered *c, uint64_t *h_e1, uint64_t *h_e2, float *h_centre, float *h_var,
                         uint64_t *h_weight) {
    return guarded([&] {
        BBK_REQUIRE(c, BBK_ERR_ARG, "bbk_clustered_export: NULL argument");
        for (size_t i = 0; i < c->recs.size(); ++i) {
            const DeRec &r = c->recs[i];
            if (h_e1) h_e1[i] = r.e1;
            if (h_e2) h_e2[i] = r.e2;
            if (h_centre) h_centre[i] = r.centre;
            if (h_var) h_var[i] = r.var;  // the stored 0 (DeClusters::flush)
            if (h_weight) h_weight[i] = r.weight;
        }
    });
}

// the clustered index in the layout of write_paired_index; what a cluster is in the file: clustered_index_point
// (pairinfo_host.hpp)
int bbk_clustered_write(const bbk_clustered *c, const char *path) {
    return guarded([&] {
        BBK_REQUIRE(c && path, BBK_ERR_ARG, "bbk_clustered_write: NULL argument");
        std::string o;
        write_paired_index(o, c->recs.size(), [&](uint64_t i) {
            const DeRec &r = c->recs[i];
            return clustered_index_point(r.e1, r.e2, r.centre, r.weight, c->ix->len[r.e1 >> 1]);
        });
        write_index_file(path, o);
    });
}

void bbk_clustered_free(bbk_clustered *c) { delete c; }

}  // extern "C"
