// pairinfo.hip -- paired-read info over the mapping paths of the two mates: the device side of PairInfoCount for
// paired-end libraries (reference projects/spades/pair_info_count.cpp:199-243, 285-324, 328-417).
//
// Replaces, per pair of a batch whose mates bbk_edgeindex_map_paths has mapped (k_gm_paths, edgeprof.hip):
//   InsertSizeCounter::ProcessPairedRead (common/paired_info/is_counter.hpp:85-115)      -> k_pi_is
//   EdgePairCounterFiller / DEFilter (pair_info_count.cpp:70-80, 123-133)                  -> k_pi_pairs<*, false>
//   LatePairedIndexFiller::ProcessPairedRead (common/paired_info/pair_info_filler.hpp:63-93) with
//   PairedBufferBase::Add / InsertWithConj (common/paired_info/paired_info_buffer.hpp:54-57, 103-147)
//                                                                                          -> k_pi_pairs<*, true>
// The host arithmetic of the stage is pairinfo_host.hpp's: the insert-size statistics in doubles (lib_statistics), the
// rounding of a distance (pi_round), the point table (PairPoints) and PairedBuffer::BinWrite (write_paired_index).  The
// conjugate of an edge and the canonical form of a pair are edge_ops.h's.
//
// A pair as presented.  OrientationChanger (common/io/reads/orientation.hpp:15-41) reverse-complements a mate before it
// is mapped.  The paths of the file-orientation mates are what the batch holds; the path of a reverse complement is
// derived from them, not mapped again: the rule by which k_gm_paths lets a position continue its predecessor's range
// (same oriented edge, larger offset, or the same offset off a looped one-(k+1)-mer edge) reads the same from either
// end of the read once every edge is replaced by its conjugate and every offset o by length - 1 - o, so
//   path(rc s)[j] = (conj e, npos - init_end, npos - init_start, length(e) - map_end, length(e) - map_start)
//   of path(s)[ranges - 1 - j], with npos = |s| - k,
// which the tests hold against MapSequence of the reverse-complemented string.  The cut offsets of LongestValid
// (longest_valid_wrapper.hpp:15-57, single_read.hpp:247-258) swap with the mate (single_read.hpp:143-147).
//
// Shape.  One lane per pair: a path holds one or two ranges nearly always, so a pair is a handful of integer operations
// on two 32-byte ranges per mate, and more lanes per pair would idle.  Records are written without a shared cursor, as
// k_gm_paths and k_rp_size do: a count pass (|path1| x |path2| records that pass the filter), one exclusive scan, a
// write pass.  A record is a 16-byte key; sort.hip and unique.hip reduce them by key:
//   insert size      word 0 = is (a pair that does not count holds 0xFFFFFFFF, the last key, dropped after the reduce)
//   ordered pair     word 0 = e1, word 1 = e2
//   point            word 0 = e1 << 31 | e2 >> 2, word 1 = (e2 & 3) << 32 | (gap ^ 2^31): ascending (e1, e2, gap)
// (edges are 2 * segment + strand with u32 segments: 33 bits).  The filter is a binary search of the pair and of its
// conjugate in the reduced, ascending pair table of the estimate pass: that table holds one entry per distinct edge pair,
// far fewer than there are records, so the searches stay in cache, where a join would sort every record once more.
// A batch leaves reduced runs (key, count); estimate / fill_finish concatenate the runs and reduce once more, so the
// result does not depend on how the pairs were batched.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "bbk_internal.h"
#include "edgeindex.h"
#include "kmer_ops.h"

namespace bbk {

constexpr uint64_t kIsNone = 0xFFFFFFFFull;  // the insert-size key of a pair that does not count (is is a positive int)

// the ranges of one mate of every pair: ranges[first[p] .. last[p]) in file orientation (0, 0 for an empty path)
struct PiSide {
    const bbk_path_range *__restrict__ ranges;
    const uint32_t *__restrict__ first, *__restrict__ last;
    const uint32_t *__restrict__ len;  // bases of the mate
    int rc;                            // the mate is presented reverse-complemented
};

struct PiRange {
    uint64_t edge;
    uint32_t is, ie, ms, me;  // initial [start, end), mapped [start, end)
};

// range i of `cnt` of the presented mate (header comment); npos = (k+1)-mer positions of the mate
__device__ inline PiRange pi_range(const PiSide &s, uint32_t first, uint32_t cnt, uint32_t i, uint32_t npos,
                                   const uint32_t *__restrict__ seg) {
    const bbk_path_range x = s.ranges[first + (s.rc ? cnt - 1u - i : i)];
    PiRange o;
    if (!s.rc) {
        o.edge = x.edge;
        o.is = x.init_start;
        o.ie = x.init_end;
        o.ms = x.map_start;
        o.me = x.map_end;
    } else {
        const uint32_t sg = seg[x.edge >> 1], L = edge_length(sg);
        o.edge = edge_conj(x.edge, sg);
        o.is = npos - x.init_end;
        o.ie = npos - x.init_start;
        o.ms = L - x.map_end;
        o.me = L - x.map_start;
    }
    return o;
}

// trim = left_offset(first) + right_offset(second) of the presented mates; cut = left1, right1, left2, right2 of the file
__device__ inline uint32_t pi_trim(const uint32_t *__restrict__ cut, uint64_t p, int rc1, int rc2) {
    if (!cut) return 0;
    const uint4 c = reinterpret_cast<const uint4 *>(cut)[p];
    return (rc1 ? c.y : c.x) + (rc2 ? c.z : c.w);
}

// One lane per range of either path (the ranges of a batch come in read order): where the ranges of every read begin
// and end.  first / last were zeroed: a read without a range keeps (0, 0).
__global__ __launch_bounds__(256) void k_pi_bounds(const bbk_path_range *__restrict__ r1, uint64_t n1,
                                                  const bbk_path_range *__restrict__ r2, uint64_t n2,
                                                  uint32_t *__restrict__ first1, uint32_t *__restrict__ last1,
                                                  uint32_t *__restrict__ first2, uint32_t *__restrict__ last2) {
    uint64_t i = BBK_GID();
    if (i >= n1 + n2) return;
    const bool one = i < n1;
    const bbk_path_range *r = one ? r1 : r2;
    const uint64_t n = one ? n1 : n2;
    if (!one) i -= n1;
    const uint32_t rd = r[i].read;
    if (i == 0 || r[i - 1].read != rd) (one ? first1 : first2)[rd] = (uint32_t)i;
    if (i + 1 == n || r[i + 1].read != rd) (one ? last1 : last2)[rd] = (uint32_t)(i + 1);
}

// InsertSizeCounter::ProcessPairedRead (is_counter.hpp:85-115), one lane per pair: the insert size of a pair that
// qualifies and is positive, kIsNone otherwise; ctr[0] += pairs counted (mapped), ctr[1] += qualifying pairs whose
// insert size is not positive (negative), one atomic per wave and counter.
__global__ __launch_bounds__(256) void k_pi_is(uint64_t n, PiSide a, PiSide b, const uint32_t *__restrict__ seg,
                                              uint32_t k, uint64_t min_len, const uint32_t *__restrict__ cut,
                                              uint64_t *__restrict__ is_key, unsigned long long *__restrict__ ctr) {
    const uint64_t p = BBK_GID();
    bool counted = false, negative = false;
    if (p < n) {
        const uint32_t f1 = a.first[p], c1 = a.last[p] - f1, f2 = b.first[p], c2 = b.last[p] - f2;
        uint64_t key = kIsNone;
        if (c1 == 1 && c2 == 1) {
            const PiRange x = pi_range(a, f1, 1, 0, a.len[p] - k, seg), y = pi_range(b, f2, 1, 0, b.len[p] - k, seg);
            if (x.edge == y.edge && (uint64_t)edge_length(seg[x.edge >> 1]) >= min_len) {
                const int read1_start = (int)x.ms - (int)x.is, read2_start = (int)y.ms - (int)y.is;
                const int is = read2_start - read1_start + (int)b.len[p] + (int)pi_trim(cut, p, a.rc, b.rc);
                counted = is > 0;
                negative = !counted;
                if (counted) key = (uint64_t)(uint32_t)is;
            }
        }
        is_key[p] = key;
    }
    const unsigned long long mc = __ballot(counted), mn = __ballot(negative);
    if ((threadIdx.x & 63) == 0) {
        if (mc) atomicAdd(&ctr[0], (unsigned long long)__popcll(mc));
        if (mn) atomicAdd(&ctr[1], (unsigned long long)__popcll(mn));
    }
}

// the count of `q` in the ascending pair table (0 when absent), as table_find searches a key table
__device__ inline uint32_t pi_pair_count(const Key<2> *__restrict__ tab, const uint32_t *__restrict__ cnt, uint64_t n,
                                         uint64_t e1, uint64_t e2) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        const Key<2> m = tab[mid];
        if (m.w[0] < e1 || (m.w[0] == e1 && m.w[1] < e2)) lo = mid + 1;
        else hi = mid;
    }
    if (lo < n) {
        const Key<2> m = tab[lo];
        if (m.w[0] == e1 && m.w[1] == e2) return cnt[lo];
    }
    return 0;
}

struct PiFill {
    uint32_t insert_size;  // (size_t) mean_insert_size, modulo 2^32: every sum below is taken as an int
    uint32_t round_distance, threshold;
    const Key<2> *__restrict__ tab;  // the pair table of the estimate pass, counts clamped to 3 (the 2-bit cells)
    const uint32_t *__restrict__ tab_cnt;
    uint64_t tab_n;
};

// the parameters of the fill pass and the pair table of the estimate pass, as the handle holds them
static PiFill fill_params(const bbk_pairinfo *pi) {
    PiFill f{};
    f.insert_size = (uint32_t)pi->fill.insert_size;
    f.round_distance = pi->fill.round_distance;
    f.threshold = pi->fill.threshold;
    if (!pi->est.pair_runs.empty()) {
        f.tab = pi->est.pair_runs[0].keys.as<Key<2>>();
        f.tab_cnt = pi->est.pair_runs[0].vals.as<uint32_t>();
        f.tab_n = pi->est.pair_runs[0].n;
    }
    return f;
}

// One lane per pair over path1 x path2.  FILL = false (estimate pass): a record is the ordered edge pair.  FILL = true:
// a pair of edges passes the filter when min(c, 3) > threshold with c = occurrences(e1, e2) + occurrences(conj e2,
// conj e1) (DEFilter, pair_info_count.cpp:70-80; PairedInfoFilter's cells are 2 bits wide, adt/bf.hpp:50-97); its record
// is the point of pair_info_filler.hpp:76-88 as the buffer stores it (paired_info_buffer.hpp:54-57, 103-147): gap =
// distance - length(e1) under the smaller of (e1, e2) and (conj e2, conj e1).  WRITE = false: the records of pair p to
// cnt[p]; WRITE = true: cnt holds their exclusive scan and the records are written from there.
template <bool WRITE, bool FILL>
__global__ __launch_bounds__(256) void k_pi_pairs(uint64_t n, PiSide a, PiSide b, const uint32_t *__restrict__ seg,
                                                 uint32_t k, const uint32_t *__restrict__ cut, PiFill f,
                                                 uint64_t *__restrict__ cnt, Key<2> *__restrict__ out) {
    const uint64_t p = BBK_GID();
    if (p >= n) return;
    const uint32_t f1 = a.first[p], c1 = a.last[p] - f1, f2 = b.first[p], c2 = b.last[p] - f2;
    if constexpr (!WRITE && !FILL) {
        cnt[p] = (uint64_t)c1 * c2;
        return;
    }
    if (c1 == 0 || c2 == 0) {
        if constexpr (!WRITE) cnt[p] = 0;
        return;
    }
    const uint32_t np1 = a.len[p] - k, np2 = b.len[p] - k;
    uint32_t read_distance = 0;
    if constexpr (FILL) read_distance = f.insert_size - pi_trim(cut, p, a.rc, b.rc) - b.len[p];
    uint64_t w = 0;  // records so far
    uint64_t at = 0;
    if constexpr (WRITE) at = cnt[p];
    for (uint32_t i = 0; i < c1; ++i) {
        const PiRange x = pi_range(a, f1, c1, i, np1, seg);
        for (uint32_t j = 0; j < c2; ++j) {
            const PiRange y = pi_range(b, f2, c2, j, np2, seg);
            if constexpr (!FILL) {
                Key<2> r;
                r.w[0] = x.edge;
                r.w[1] = y.edge;
                out[at + w++] = r;
            } else {
                const uint64_t cy = edge_conj(y.edge, seg[y.edge >> 1]), cx = edge_conj(x.edge, seg[x.edge >> 1]);
                if (f.threshold > 0) {
                    const uint32_t c = pi_pair_count(f.tab, f.tab_cnt, f.tab_n, x.edge, y.edge) +
                                       pi_pair_count(f.tab, f.tab_cnt, f.tab_n, cy, cx);
                    if (!(min(c, 3u) > f.threshold)) continue;
                }
                if constexpr (WRITE) {
                    const uint32_t kmer_distance = read_distance + y.ie - x.is;
                    int32_t d = (int32_t)(kmer_distance + x.ms - y.me);
                    if (f.round_distance > 1) d = pi_round(d, f.round_distance);
                    const uint32_t gap = (uint32_t)d - edge_length(seg[x.edge >> 1]);
                    uint64_t e1, e2;
                    canonical_pair(x.edge, y.edge, seg, &e1, &e2);
                    Key<2> r;
                    r.w[0] = (e1 << 31) | (e2 >> 2);
                    r.w[1] = ((e2 & 3ull) << 32) | (uint64_t)(gap ^ 0x80000000u);
                    out[at + w] = r;
                }
                ++w;
            }
        }
    }
    if constexpr (!WRITE) cnt[p] = w;
}

__global__ __launch_bounds__(256) void k_pi_clamp(uint32_t *__restrict__ v, uint64_t n, uint32_t cap) {
    const uint64_t i = BBK_GID();
    if (i < n) v[i] = min(v[i], cap);
}

// ---- reduce by key ----------------------------------------------------------------------------------------------------

static void add_bits(std::vector<PassDesc> &p, int word, int lo, int hi) {
    for (int s = lo; s < hi; s += 8) p.push_back({0, word, s, std::min(8, hi - s), 0u});
}
static std::vector<PassDesc> is_passes() {
    std::vector<PassDesc> p;
    add_bits(p, 0, 0, 32);
    return p;
}
static std::vector<PassDesc> pair_passes(int eb) {  // least significant first: e2, then e1
    std::vector<PassDesc> p;
    add_bits(p, 1, 0, eb);
    add_bits(p, 0, 0, eb);
    return p;
}
static std::vector<PassDesc> point_passes(int eb) {  // gap and the low bits of e2, the rest of e2, e1
    std::vector<PassDesc> p;
    add_bits(p, 1, 0, 34);
    add_bits(p, 0, 0, std::max(eb - 2, 0));
    add_bits(p, 0, 31, 31 + eb);
    return p;
}

using Run = bbk_pairinfo::Run;

// n unordered records (consumed) -> ascending distinct keys with their number of occurrences
static Run reduce_records(bbk_ctx *ctx, int W, DevBuf &rec, uint64_t n, const std::vector<PassDesc> &passes) {
    Run r;
    if (n == 0) return r;
    DevBuf tmp(n * W * 8);
    sort_records(ctx, W, rec.p, tmp.p, nullptr, nullptr, n, passes);
    r.vals.alloc(n * 4);
    r.n = unique_records(ctx, W, rec.p, nullptr, n, tmp.p, r.vals.as<uint32_t>(), REDUCE_COUNT);
    r.keys = std::move(tmp);
    rec.release();
    return r;
}

// the runs (consumed) -> one run: keys ascending and distinct, counts of equal keys added
static void merge_runs(bbk_ctx *ctx, int W, std::vector<Run> &runs, const std::vector<PassDesc> &passes) {
    runs.erase(std::remove_if(runs.begin(), runs.end(), [](const Run &r) { return r.n == 0; }), runs.end());
    if (runs.size() <= 1) return;
    uint64_t n = 0;
    for (const Run &r : runs) n += r.n;
    BBK_REQUIRE(n < (1ull << 32), BBK_ERR_ARG, "paired info: %llu reduced records, at most 2^32 - 1 supported",
                (unsigned long long)n);
    DevBuf keys(n * W * 8), vals(n * 4), ktmp(n * W * 8), vtmp(n * 4);
    uint64_t at = 0;
    for (const Run &r : runs) {
        BBK_HIP(copy_async(keys.as<char>() + at * W * 8, r.keys.p, r.n * W * 8, hipMemcpyDeviceToDevice, ctx->stream));
        BBK_HIP(copy_async(vals.as<uint32_t>() + at, r.vals.p, r.n * 4, hipMemcpyDeviceToDevice, ctx->stream));
        at += r.n;
    }
    sort_records(ctx, W, keys.p, ktmp.p, vals.as<uint32_t>(), vtmp.as<uint32_t>(), n, passes);  // waits: the copies are done
    runs.clear();
    Run out;
    out.n = unique_records(ctx, W, keys.p, vals.as<uint32_t>(), n, ktmp.p, vtmp.as<uint32_t>(), REDUCE_SUM);
    out.keys = std::move(ktmp);
    out.vals = std::move(vtmp);
    runs.push_back(std::move(out));
}

constexpr size_t kMaxRuns = 16;  // runs kept before they are merged: bounds the memory the runs of many batches hold

static void keep_run(bbk_ctx *ctx, int W, std::vector<Run> &runs, Run &&r, const std::vector<PassDesc> &passes) {
    if (r.n) runs.push_back(std::move(r));
    if (runs.size() >= kMaxRuns) merge_runs(ctx, W, runs, passes);
}

// ---- a batch ----------------------------------------------------------------------------------------------------------

struct PathsGuard {
    bbk_paths *p = nullptr;
    ~PathsGuard() { bbk_paths_free(p); }
};

// the two mates mapped and the bounds of every read's ranges
struct Batch {
    PathsGuard p1, p2;
    DevBuf bounds, cut;
    uint64_t n = 0;
    PiSide a{}, b{};
    const uint32_t *d_cut = nullptr;
};

static void map_batch(bbk_pairinfo *pi, const char *who, const bbk_reads *first, const bbk_reads *second, int orientation,
                      const uint32_t *h_cut, Batch &bt) {
    BBK_REQUIRE(first && second, BBK_ERR_ARG, "%s: NULL argument", who);
    BBK_REQUIRE(first->n == second->n, BBK_ERR_ARG, "%s: %llu first mates and %llu second mates", who,
                (unsigned long long)first->n, (unsigned long long)second->n);
    BBK_REQUIRE(orientation >= BBK_ORIENT_FF && orientation <= BBK_ORIENT_RR, BBK_ERR_ARG,
                "%s: orientation %d is none of BBK_ORIENT_FF, _FR, _RF, _RR", who, orientation);
    bbk_ctx *ctx = pi->ctx;
    BBK_HIP(hipSetDevice(ctx->device));
    const uint64_t n = bt.n = first->n;
    if (n == 0) return;
    int rc = bbk_edgeindex_map_paths(ctx, pi->ix, first, &bt.p1.p);
    if (rc == BBK_OK) rc = bbk_edgeindex_map_paths(ctx, pi->ix, second, &bt.p2.p);
    if (rc != BBK_OK) throw Error{rc};
    const uint64_t n1 = bt.p1.p->n_ranges, n2 = bt.p2.p->n_ranges;
    BBK_REQUIRE(n1 < (1ull << 32) && n2 < (1ull << 32), BBK_ERR_ARG, "%s: more than 2^32 - 1 ranges in a batch", who);
    bt.bounds.alloc(4 * n * 4);
    BBK_HIP(hipMemsetAsync(bt.bounds.p, 0, 4 * n * 4, ctx->stream));
    uint32_t *bd = bt.bounds.as<uint32_t>();
    if (n1 + n2) {
        KernelTimer t(ctx, "pairinfo_join", (double)(n1 + n2) * sizeof(bbk_path_range));
        launch_items(ctx, "k_pi_bounds", k_pi_bounds, n1 + n2, bt.p1.p->ranges.as<bbk_path_range>(), n1,
                     bt.p2.p->ranges.as<bbk_path_range>(), n2, bd, bd + n, bd + 2 * n, bd + 3 * n);
    }
    if (h_cut) {
        bt.cut.alloc(n * 16);
        BBK_HIP(hipMemcpyAsync(bt.cut.p, h_cut, n * 16, hipMemcpyHostToDevice, ctx->stream));
        bt.d_cut = bt.cut.as<uint32_t>();
    }
    const bool rc1 = orientation == BBK_ORIENT_RF || orientation == BBK_ORIENT_RR;
    const bool rc2 = orientation == BBK_ORIENT_FR || orientation == BBK_ORIENT_RR;
    bt.a = {bt.p1.p->ranges.as<bbk_path_range>(), bd, bd + n, first->d_len, rc1};
    bt.b = {bt.p2.p->ranges.as<bbk_path_range>(), bd + 2 * n, bd + 3 * n, second->d_len, rc2};
}

// count pass, scan, write pass of k_pi_pairs, then the reduce of the records: the run of the batch
template <bool FILL>
static Run pair_records(bbk_pairinfo *pi, const Batch &bt, const PiFill &f, uint64_t &records) {
    bbk_ctx *ctx = pi->ctx;
    const uint64_t n = bt.n;
    const uint32_t *seg = pi->ix->seg.as<uint32_t>();
    DevBuf cnt(n * 8), rec;
    const double bytes = (double)(bt.p1.p->n_ranges + bt.p2.p->n_ranges) * sizeof(bbk_path_range) + (double)n * 24;
    {
        KernelTimer t(ctx, "pairinfo_join", bytes);
        launch_items(ctx, "k_pi_pairs", k_pi_pairs<false, FILL>, n, n, bt.a, bt.b, seg, (uint32_t)pi->ix->k, bt.d_cut, f,
                     cnt.as<uint64_t>(), (Key<2> *)nullptr);
    }
    const uint64_t total = exclusive_scan_u64(ctx, cnt.as<uint64_t>(), cnt.as<uint64_t>(), n);
    records += total;
    BBK_REQUIRE(records < (1ull << 32), BBK_ERR_ARG,
                "paired info: %llu edge-pair records in one pass, at most 2^32 - 1 supported (the counts are 32 bits wide)",
                (unsigned long long)records);
    if (total == 0) return Run();
    rec.alloc(total * 16);
    {
        KernelTimer t(ctx, "pairinfo_join", bytes + (double)total * 16);
        launch_items(ctx, "k_pi_pairs", k_pi_pairs<true, FILL>, n, n, bt.a, bt.b, seg, (uint32_t)pi->ix->k, bt.d_cut, f,
                     cnt.as<uint64_t>(), rec.as<Key<2>>());
    }
    return reduce_records(ctx, 2, rec, total, FILL ? point_passes(pi->edge_bits) : pair_passes(pi->edge_bits));
}

void write_index_file(const char *path, const std::string &bytes) {
    FILE *f = fopen(path, "wb");
    BBK_REQUIRE(f, BBK_ERR_IO, "cannot open %s for writing", path);
    const bool ok = fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    BBK_REQUIRE((fclose(f) == 0) && ok, BBK_ERR_IO, "short write to %s", path);
}

}  // namespace bbk

using namespace bbk;

extern "C" {

int bbk_pairinfo_begin(bbk_ctx *ctx, const bbk_edgeindex *ix, uint64_t min_edge_length, bbk_pairinfo **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && ix && out, BBK_ERR_ARG, "bbk_pairinfo_begin: NULL argument");
        for (uint64_t s = 0; s < ix->n_seg; ++s)
            BBK_REQUIRE(ix->len[s] < (1ull << 31), BBK_ERR_ARG, "bbk_pairinfo_begin: segment %s holds 2^31 (k+1)-mers or more",
                        ix->names[s].c_str());
        auto pi = std::make_unique<bbk_pairinfo>();
        pi->ctx = ctx;
        pi->ix = ix;
        pi->min_edge_length = min_edge_length;
        while ((1ull << pi->edge_bits) < 2 * ix->n_seg) ++pi->edge_bits;
        *out = pi.release();
    });
}

int bbk_pairinfo_push_estimate(bbk_pairinfo *pi, const bbk_reads *first, const bbk_reads *second, int orientation,
                               const uint32_t *h_cut) {
    return guarded([&] {
        BBK_REQUIRE(pi, BBK_ERR_ARG, "bbk_pairinfo_push_estimate: NULL argument");
        BBK_REQUIRE(!pi->filling && !pi->filled, BBK_ERR_ARG, "bbk_pairinfo_push_estimate: the fill pass has begun");
        Batch bt;
        map_batch(pi, "bbk_pairinfo_push_estimate", first, second, orientation, h_cut, bt);
        const uint64_t n = bt.n;
        bbk_pairinfo::EstimatePass &est = pi->est;
        BBK_REQUIRE(est.total + n < (1ull << 32), BBK_ERR_ARG,
                    "bbk_pairinfo_push_estimate: 2^32 pairs or more in one estimate pass (the counts are 32 bits wide)");
        pi->estimated = false;
        est.total += n;
        if (n == 0) return;
        bbk_ctx *ctx = pi->ctx;
        DevBuf is_key(n * 8), ctr(16);
        BBK_HIP(hipMemsetAsync(ctr.p, 0, 16, ctx->stream));
        {
            KernelTimer t(ctx, "pairinfo_join", (double)n * 40);
            launch_items(ctx, "k_pi_is", k_pi_is, n, n, bt.a, bt.b, pi->ix->seg.as<uint32_t>(), (uint32_t)pi->ix->k,
                         pi->min_edge_length, bt.d_cut, is_key.as<uint64_t>(), ctr.as<unsigned long long>());
        }
        uint64_t c[2];
        d2h_sync(ctx, c, ctr.p, 16);
        est.mapped += c[0];
        est.negative += c[1];
        Run r = reduce_records(ctx, 1, is_key, n, is_passes());
        if (c[0] < n) --r.n;  // the last key is kIsNone
        keep_run(ctx, 1, est.is_runs, std::move(r), is_passes());
        Run pr = pair_records<false>(pi, bt, PiFill{}, est.records);
        keep_run(ctx, 2, est.pair_runs, std::move(pr), pair_passes(pi->edge_bits));
    });
}

int bbk_pairinfo_estimate(bbk_pairinfo *pi, bbk_pairinfo_stats *st) {
    return guarded([&] {
        BBK_REQUIRE(pi && st, BBK_ERR_ARG, "bbk_pairinfo_estimate: NULL argument");
        bbk_ctx *ctx = pi->ctx;
        BBK_HIP(hipSetDevice(ctx->device));
        bbk_pairinfo::EstimatePass &est = pi->est;
        if (!pi->estimated) {
            merge_runs(ctx, 1, est.is_runs, is_passes());
            merge_runs(ctx, 2, est.pair_runs, pair_passes(pi->edge_bits));
            if (!est.pair_runs.empty()) {  // what the filter reads: min(c, 3) = min(min(a, 3) + min(b, 3), 3)
                Run &t = est.pair_runs[0];
                launch_items(ctx, "k_pi_clamp", k_pi_clamp, t.n, t.vals.as<uint32_t>(), t.n, 3u);
            }
            const uint64_t nh = est.is_runs.empty() ? 0 : est.is_runs[0].n;
            std::vector<uint64_t> keys(nh);
            std::vector<uint32_t> cnt(nh);
            if (nh) {
                BBK_HIP(hipMemcpyAsync(keys.data(), est.is_runs[0].keys.p, nh * 8, hipMemcpyDeviceToHost, ctx->stream));
                BBK_HIP(hipMemcpyAsync(cnt.data(), est.is_runs[0].vals.p, nh * 4, hipMemcpyDeviceToHost, ctx->stream));
            }
            BBK_HIP(hipStreamSynchronize(ctx->stream));
            est.hist_is.resize(nh);
            est.hist_count.resize(nh);
            for (uint64_t i = 0; i < nh; ++i) {
                est.hist_is[i] = (int32_t)(uint32_t)keys[i];
                est.hist_count[i] = cnt[i];
            }
            pi->estimated = true;
        }
        memset(st, 0, sizeof(*st));
        st->total = est.total;
        st->mapped = est.mapped;
        st->negative = est.negative;
        st->edge_pairs = est.pair_runs.empty() ? 0 : est.pair_runs[0].n;
        if (est.mapped == 0) return;  // CollectLibInformation (pair_info_count.cpp:227-230)
        HistType hist;
        for (size_t i = 0; i < est.hist_is.size(); ++i) hist[est.hist_is[i]] = est.hist_count[i];
        lib_statistics(hist, pi->ix->k, st);
    });
}

uint64_t bbk_pairinfo_hist_size(const bbk_pairinfo *pi) { return pi && pi->estimated ? pi->est.hist_is.size() : 0; }

int bbk_pairinfo_hist_export(const bbk_pairinfo *pi, int32_t *h_is, uint64_t *h_count) {
    return guarded([&] {
        BBK_REQUIRE(pi, BBK_ERR_ARG, "bbk_pairinfo_hist_export: NULL argument");
        BBK_REQUIRE(pi->estimated, BBK_ERR_ARG, "bbk_pairinfo_hist_export: before bbk_pairinfo_estimate");
        if (h_is) std::copy(pi->est.hist_is.begin(), pi->est.hist_is.end(), h_is);
        if (h_count) std::copy(pi->est.hist_count.begin(), pi->est.hist_count.end(), h_count);
    });
}

int bbk_pairinfo_fill_begin(bbk_pairinfo *pi, uint64_t insert_size, unsigned round_distance, unsigned filter_threshold) {
    return guarded([&] {
        BBK_REQUIRE(pi, BBK_ERR_ARG, "bbk_pairinfo_fill_begin: NULL argument");
        BBK_REQUIRE(filter_threshold == 0 || pi->estimated, BBK_ERR_ARG,
                    "bbk_pairinfo_fill_begin: filter_threshold %u needs the edge-pair counts of an estimate pass "
                    "(bbk_pairinfo_push_estimate, bbk_pairinfo_estimate) over the same handle", filter_threshold);
        pi->filling = true;
        pi->filled = false;
        pi->fill = {};  // the runs of an earlier fill pass go
        pi->fill.insert_size = insert_size;
        pi->fill.round_distance = round_distance;
        pi->fill.threshold = filter_threshold;
    });
}

int bbk_pairinfo_push_fill(bbk_pairinfo *pi, const bbk_reads *first, const bbk_reads *second, int orientation,
                           const uint32_t *h_cut) {
    return guarded([&] {
        BBK_REQUIRE(pi, BBK_ERR_ARG, "bbk_pairinfo_push_fill: NULL argument");
        BBK_REQUIRE(pi->estimated, BBK_ERR_ARG, "bbk_pairinfo_push_fill: before bbk_pairinfo_estimate");
        BBK_REQUIRE(pi->filling, BBK_ERR_ARG, "bbk_pairinfo_push_fill: before bbk_pairinfo_fill_begin");
        Batch bt;
        map_batch(pi, "bbk_pairinfo_push_fill", first, second, orientation, h_cut, bt);
        if (bt.n == 0) return;
        pi->filled = false;
        Run r = pair_records<true>(pi, bt, fill_params(pi), pi->fill.records);
        keep_run(pi->ctx, 2, pi->fill.point_runs, std::move(r), point_passes(pi->edge_bits));
    });
}

int bbk_pairinfo_fill_finish(bbk_pairinfo *pi) {
    return guarded([&] {
        BBK_REQUIRE(pi, BBK_ERR_ARG, "bbk_pairinfo_fill_finish: NULL argument");
        BBK_REQUIRE(pi->filling, BBK_ERR_ARG, "bbk_pairinfo_fill_finish: before bbk_pairinfo_fill_begin");
        bbk_ctx *ctx = pi->ctx;
        BBK_HIP(hipSetDevice(ctx->device));
        std::vector<Run> &runs = pi->fill.point_runs;
        merge_runs(ctx, 2, runs, point_passes(pi->edge_bits));
        const uint64_t n = runs.empty() ? 0 : runs[0].n;
        std::vector<uint64_t> keys(2 * n);
        std::vector<uint32_t> cnt(n);
        if (n) {
            BBK_HIP(hipMemcpyAsync(keys.data(), runs[0].keys.p, n * 16, hipMemcpyDeviceToHost, ctx->stream));
            BBK_HIP(hipMemcpyAsync(cnt.data(), runs[0].vals.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        }
        BBK_HIP(hipStreamSynchronize(ctx->stream));
        PairPoints &pt = pi->points;
        pt.resize(n);
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t w0 = keys[2 * i], w1 = keys[2 * i + 1];
            const uint64_t e1 = w0 >> 31, e2 = ((w0 & 0x7FFFFFFFull) << 2) | (w1 >> 32);
            pt.e1[i] = e1;
            pt.e2[i] = e2;
            pt.gap[i] = (int32_t)((uint32_t)w1 ^ 0x80000000u);
            // a pair that is its own conjugate gets every point twice (paired_info_buffer.hpp:106-115)
            pt.weight[i] = (uint64_t)cnt[i] * (pair_is_self_conj(e1, e2, pi->ix->seg_h.data()) ? 2 : 1);
        }
        pi->filled = true;
    });
}

uint64_t bbk_pairinfo_points(const bbk_pairinfo *pi) { return pi && pi->filled ? pi->points.size() : 0; }

int bbk_pairinfo_export(const bbk_pairinfo *pi, uint64_t *h_e1, uint64_t *h_e2, int32_t *h_gap, uint64_t *h_weight) {
    return guarded([&] {
        BBK_REQUIRE(pi, BBK_ERR_ARG, "bbk_pairinfo_export: NULL argument");
        BBK_REQUIRE(pi->filled, BBK_ERR_ARG, "bbk_pairinfo_export: before bbk_pairinfo_fill_finish");
        const PairPoints &pt = pi->points;
        if (h_e1) std::copy(pt.e1.begin(), pt.e1.end(), h_e1);
        if (h_e2) std::copy(pt.e2.begin(), pt.e2.end(), h_e2);
        if (h_gap) std::copy(pt.gap.begin(), pt.gap.end(), h_gap);
        if (h_weight) std::copy(pt.weight.begin(), pt.weight.end(), h_weight);
    });
}

// the raw index in the layout of write_paired_index (pairinfo_host.hpp): a point is the float gap and the float weight
int bbk_pairinfo_write(const bbk_pairinfo *pi, const char *path) {
    return guarded([&] {
        BBK_REQUIRE(pi && path, BBK_ERR_ARG, "bbk_pairinfo_write: NULL argument");
        BBK_REQUIRE(pi->filled, BBK_ERR_ARG, "bbk_pairinfo_write: before bbk_pairinfo_fill_finish");
        const PairPoints &pt = pi->points;
        std::string o;
        write_paired_index(o, pt.size(), [&](uint64_t i) { return raw_index_point(pt, i); });
        write_index_file(path, o);
    });
}

void bbk_pairinfo_free(bbk_pairinfo *pi) { delete pi; }

}  // extern "C"
