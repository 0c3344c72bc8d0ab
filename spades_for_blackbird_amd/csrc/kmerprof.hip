// kmerprof.hip -- k-mer multiplicity profiles across samples and contig abundances.
//
// Join: replaces KmerMultiplicityCounter::FilterCombinedKmers (projects/mts/kmer_multiplicity_counter.cpp:72-139): the
// reference sorts one record file per sample and merges them sequentially under RtSeq::less3; every distinct k-mer held
// by `present` samples with summed count `total` is kept iff present >= min_samples && (present > 1 || total >
// min_mult), and its N counts become one uint16_t row of <prefix>.bpr.  Here every sample's canonical counted set is
// filtered (count >= ci, saturated at cs) and kept on the device as keys + u16 counts; finish() concatenates the key
// arrays, merge-uniques them with the engine's own sort (bbk_kmerset_from_device_ex), scatters every sample's counts
// into rows[union position * N + sample] through the prefix table + binary search, applies the keep rule per union
// k-mer and moves the kept keys and rows with the ordered selection of select.h.
//
// Abundance: replaces ProfileCounter::operator() (projects/mts/contig_abundance.cpp:245-284) with the winsorised mean
// of TrivialClusterAnalyzer (:46-78).  A contig is the run of pieces (maximal ACGT stretches) the caller cut it into.
//   pass 1 (k_ab_collect): one wavefront per contig, a loop over its pieces and 64 positions at a time; each lane takes
//     the canonical k-mer at its position, looks it up and the wave appends the found row indices (ballot + prefix
//     popcount) to the contig's slice of one index buffer.  A long contig is a longer loop of the same wave.
//   pass 2 (k_ab_reduce): one wavefront per (contig, sample).  lo = sorted[o], hi = sorted[n - o - 1] with
//     o = ceil(float(n) * 0.05f) are found by radix selection over 256-bin LDS histograms (high byte, then low byte;
//     the high-byte pass is skipped when no row value exceeds 255), then sum and sum of squares of
//     max(min(v, hi), lo) are taken in u64.  For n = 2 (lo > hi) that order of the two clamps is what the reference's
//     in-place loop over a sorted vector gives; n = 1 is left as it is.
// The device returns integers only; every float operation (share test, mean, variance, formatting) is the host's.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <unistd.h>

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "bbk_internal.h"
#include "gfa_graph.h"
#include "kmer_ops.h"
#include "select.h"

struct bbk_kmerprofile {
    unsigned k = 0, W = 0, N = 0;
    uint64_t n = 0;          // kept k-mers
    uint32_t max_value = 0;  // upper bound of every row value (cs, or the maximum of a loaded file)
    bbk::DevBuf keys;        // n * W u64, ascending canonical k-mers
    bbk::DevBuf rows;        // n * N u16, sample-major inside a row
    bbk::PrefixIndex prefix;  // over keys
};

struct bbk_kmerprofile_builder {
    bbk_ctx *ctx = nullptr;
    unsigned k = 0, W = 0, N = 0, ci = 0, cs = 0;
    struct Sample {
        bbk::DevBuf keys, vals;  // n * W u64 ascending, n u16
        uint64_t n = 0;
        bool set = false;
    };
    std::vector<Sample> samples;
};

namespace bbk {

// ---- join ---------------------------------------------------------------------------------------------------------------

// per-sample filter (an ordered selection on U32AtLeast{counts, ci}, select.h): a k-mer counted fewer than ci times is
// absent from the sample, and the remaining counts are saturated at cs (<= 65535) and narrowed to u16
template <int W>
struct KpStoreSample {
    const Key<W> *__restrict__ keys;
    const uint32_t *__restrict__ counts;
    uint32_t cs;
    Key<W> *__restrict__ out_keys;
    uint16_t *__restrict__ out_vals;
    __device__ void operator()(uint64_t i, uint64_t rank) const {
        const uint32_t c = counts[i];
        key_store<W>(&out_keys[rank], key_load<W>(&keys[i]));
        out_vals[rank] = (uint16_t)(c < cs ? c : cs);
    }
};

// one lane per record of sample s: its place in the union, its count into the row
template <int W>
__global__ __launch_bounds__(256) void k_kp_scatter(const Key<W> *__restrict__ skeys, const uint16_t *__restrict__ svals,
                                                   uint64_t n, const Key<W> *__restrict__ ukeys, PrefixTable P, unsigned N,
                                                   unsigned s, uint16_t *__restrict__ rows, uint32_t *__restrict__ err) {
    const uint64_t i = BBK_GID();
    if (i >= n) return;
    const uint64_t pos = table_find<W>(ukeys, P, key_load<W>(&skeys[i]));
    if (pos == kNotFound) {
        atomicOr(err, 1u);
        return;
    }
    rows[pos * (uint64_t)N + s] = svals[i];
}

// one lane per union k-mer: present = samples holding it, total = sum of its counts (:115-125); the rule over a row is
// stated here only: the selection reads the keep byte
__global__ __launch_bounds__(256) void k_kp_keep(const uint16_t *__restrict__ rows, uint64_t n, unsigned N,
                                                uint64_t min_samples, uint64_t min_mult, uint8_t *__restrict__ keep) {
    const uint64_t i = BBK_GID();
    if (i >= n) return;
    const uint16_t *row = rows + i * (uint64_t)N;
    uint64_t present = 0, total = 0;
    for (unsigned s = 0; s < N; ++s) {
        const uint32_t v = row[s];
        present += v != 0 ? 1u : 0u;
        total += v;
    }
    keep[i] = present >= min_samples && (present > 1 || total > min_mult) ? 1 : 0;
}

// (mask form: the four keep bytes of a lane in one load; p is a multiple of 4 and keep holds 16 bytes beyond n)
struct KpKeepByte {
    const uint8_t *__restrict__ keep;
    __device__ uint32_t operator()(uint64_t p, uint64_t n) const {
        const uint32_t v = *reinterpret_cast<const uint32_t *>(keep + p);
        uint32_t m = 0;
#pragma unroll
        for (uint32_t b = 0; b < kSelLane; ++b) m |= (p + b < n && ((v >> (8 * b)) & 0xFFu) ? 1u : 0u) << b;
        return m;
    }
};

template <int W>
struct KpMoveRow {
    const Key<W> *__restrict__ keys;
    const uint16_t *__restrict__ rows;
    unsigned N;
    Key<W> *__restrict__ out_keys;
    uint16_t *__restrict__ out_rows;
    __device__ void operator()(uint64_t i, uint64_t rank) const {
        key_store<W>(&out_keys[rank], key_load<W>(&keys[i]));
        const uint16_t *src = rows + i * (uint64_t)N;
        uint16_t *dst = out_rows + rank * (uint64_t)N;
        for (unsigned s = 0; s < N; ++s) dst[s] = src[s];
    }
};

// ---- abundance ----------------------------------------------------------------------------------------------------------

// one lane per contig: k-mer positions of its pieces (a piece shorter than k has none, :251-252)
__global__ __launch_bounds__(256) void k_ab_positions(const uint32_t *__restrict__ len, const uint64_t *__restrict__ first,
                                                     uint64_t nc, uint32_t k, uint64_t *__restrict__ pos,
                                                     uint32_t *__restrict__ err) {
    const uint64_t c = BBK_GID();
    if (c >= nc) return;
    const uint64_t q0 = first ? first[c] : c, q1 = first ? first[c + 1] : c + 1;
    uint64_t p = 0;
    for (uint64_t q = q0; q < q1; ++q) {
        const uint32_t L = len[q];
        if (L >= k) p += (uint64_t)(L - k) + 1u;
    }
    if (p >> 32) atomicOr(err, 1u);  // the LDS histograms of pass 2 count in u32
    pos[c] = p;
}

// pass 1: one wavefront per contig
template <int W>
__global__ __launch_bounds__(256) void k_ab_collect(const uint64_t *__restrict__ words, const uint64_t *__restrict__ woff,
                                                   const uint32_t *__restrict__ len, const uint64_t *__restrict__ first,
                                                   uint64_t nc, int k, const Key<W> *__restrict__ keys, PrefixTable P,
                                                   const uint64_t *__restrict__ off, uint64_t *__restrict__ found,
                                                   uint64_t *__restrict__ n_out) {
    const uint64_t c = (BBK_GID()) >> 6;
    if (c >= nc) return;
    const int lane = threadIdx.x & 63;
    const uint64_t q0 = first ? first[c] : c, q1 = first ? first[c + 1] : c + 1;
    uint64_t *out = found + off[c];
    uint64_t cnt = 0;
    for (uint64_t q = q0; q < q1; ++q) {
        const uint32_t L = len[q];
        if (L < (uint32_t)k) continue;
        const uint64_t nk = (uint64_t)(L - (uint32_t)k) + 1u;
        const uint64_t *rw = words + woff[q];
        for (uint64_t b = 0; b < nk; b += 64) {  // the whole wave takes every round: the ballot needs all lanes
            const uint64_t p = b + (uint64_t)lane;
            uint64_t i = kNotFound;
            if (p < nk) {
                const Key<W> f = kmer_extract<W>(rw, (uint32_t)p, k);
                const Key<W> rc = kmer_rc<W>(f, k);
                i = table_find<W>(keys, P, key_select<W>(!kmer_less_nucl<W>(rc, f), f, rc));
            }
            const bool hit = i != kNotFound;
            const uint64_t m = __ballot(hit);
            if (hit) out[cnt + (uint64_t)__popcll(m & ((1ull << lane) - 1ull))] = i;
            cnt += (uint64_t)__popcll(m);
        }
    }
    if (lane == 0) n_out[c] = cnt;
}

// Adds 1 to h[bin] for every lane with `valid`.  The values of one contig's column are mostly equal (one coverage), and
// 64 atomics on one LDS address are served one after the other: when every valid lane holds the same bin, one lane adds
// the lane count instead.  h belongs to this wave alone.
__device__ inline void hist_add(uint32_t *h, uint32_t bin, bool valid, int lane) {
    const uint64_t m = __ballot(valid);
    if (m == 0) return;
    const int lead = __ffsll((unsigned long long)m) - 1;
    const uint32_t b0 = (uint32_t)__shfl((int)bin, lead, 64);
    if ((uint64_t)__ballot(valid && bin == b0) == m) {
        if (lane == lead) h[b0] += (uint32_t)__popcll(m);
    } else if (valid) {
        atomicAdd(&h[bin], 1u);
    }
}

// the bin of a 256-bin histogram that holds rank r (0-based, r < total), and r's rank inside that bin
__device__ inline void select_bin(const uint32_t *h, uint32_t r, int lane, uint32_t *bin, uint32_t *rem) {
    const uint32_t c0 = h[4 * lane], c1 = h[4 * lane + 1], c2 = h[4 * lane + 2], c3 = h[4 * lane + 3];
    const uint32_t s = c0 + c1 + c2 + c3;
    uint32_t incl = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, d, 64);
        if (lane >= d) incl += t;
    }
    const uint32_t excl = incl - s;
    const bool mine = r >= excl && r < incl;
    uint32_t b = 4u * (uint32_t)lane, q = r - excl;
    if (mine) {
        if (q >= c0) {
            q -= c0;
            ++b;
            if (q >= c1) {
                q -= c1;
                ++b;
                if (q >= c2) {
                    q -= c2;
                    ++b;
                }
            }
        }
    }
    const uint64_t m = __ballot(mine);
    const int src = m ? __ffsll((unsigned long long)m) - 1 : 0;
    *bin = (uint32_t)__shfl((int)b, src, 64);
    *rem = (uint32_t)__shfl((int)q, src, 64);
}

// pass 2: one wavefront per (contig, sample).  TWO: row values may exceed 255, the high byte is selected first.
template <bool TWO>
__global__ __launch_bounds__(256) void k_ab_reduce(const uint16_t *__restrict__ rows, unsigned N,
                                                  const uint64_t *__restrict__ found, const uint64_t *__restrict__ off,
                                                  const uint64_t *__restrict__ n_arr, uint64_t nc,
                                                  uint64_t *__restrict__ sum_out, uint64_t *__restrict__ sumsq_out) {
    constexpr int NH = TWO ? 3 : 1;
    __shared__ uint32_t hist[4][NH][256];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t g = (BBK_GID()) >> 6;
    // every wave of the block takes the same barriers, with or without work
    const bool active = g < nc * (uint64_t)N;
    const uint64_t c = active ? g / N : 0;
    const unsigned s = active ? (unsigned)(g % N) : 0;
    const uint64_t n = active ? n_arr[c] : 0;
    const uint64_t *idx = found + (active ? off[c] : 0);
    const uint16_t *col = rows + s;
    for (int i = lane; i < NH * 256; i += 64) (&hist[w][0][0])[i] = 0;
    __syncthreads();
    const bool sel = n >= 2;  // n = 1: the value stands as it is
    uint32_t rlo = 0, rhi = 0;
    if (sel) {
        const uint64_t o = (uint64_t)ceilf(__fmul_rn((float)n, 0.05f));  // one rounded multiply: nothing to contract
        rlo = (uint32_t)o;
        rhi = (uint32_t)(n - o - 1);
    }
    uint32_t hb_lo = 0, hb_hi = 0;
    if constexpr (TWO) {
        for (uint64_t b = 0; b < n && sel; b += 64) {
            const uint64_t j = b + (uint64_t)lane;
            const bool valid = j < n;
            const uint32_t v = valid ? col[idx[j] * (uint64_t)N] : 0u;
            hist_add(hist[w][0], v >> 8, valid, lane);
        }
        __syncthreads();
        if (sel) {
            select_bin(hist[w][0], rlo, lane, &hb_lo, &rlo);
            select_bin(hist[w][0], rhi, lane, &hb_hi, &rhi);
        }
    }
    for (uint64_t b = 0; b < n && sel; b += 64) {
        const uint64_t j = b + (uint64_t)lane;
        const bool valid = j < n;
        const uint32_t v = valid ? col[idx[j] * (uint64_t)N] : 0u;
        if constexpr (TWO) {
            hist_add(hist[w][NH - 2], v & 255u, valid && (v >> 8) == hb_lo, lane);
            hist_add(hist[w][NH - 1], v & 255u, valid && (v >> 8) == hb_hi, lane);
        } else {
            hist_add(hist[w][0], v & 255u, valid, lane);
        }
    }
    __syncthreads();
    uint32_t lo = 0, hi = 65535;
    if (sel) {
        uint32_t bl, bh, r_;
        select_bin(hist[w][TWO ? NH - 2 : 0], rlo, lane, &bl, &r_);
        select_bin(hist[w][TWO ? NH - 1 : 0], rhi, lane, &bh, &r_);
        lo = (hb_lo << 8) | bl;
        hi = (hb_hi << 8) | bh;
    }
    uint64_t sum = 0, sq = 0;
    for (uint64_t j = lane; j < n; j += 64) {
        uint32_t v = col[idx[j] * (uint64_t)N];
        v = v < hi ? v : hi;
        v = v > lo ? v : lo;
        sum += v;
        sq += (uint64_t)v * v;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        sum += (uint64_t)__shfl_xor((unsigned long long)sum, d, 64);
        sq += (uint64_t)__shfl_xor((unsigned long long)sq, d, 64);
    }
    if (active && lane == 0) {
        sum_out[g] = sum;
        sumsq_out[g] = sq;
    }
}

static void build_profile_index(bbk_ctx *ctx, bbk_kmerprofile *p) {
    p->prefix.build(ctx, p->keys.as<uint64_t>(), p->W, p->k, p->n);
}

static void check_sample_set(const bbk_kmerset *s, const char *who) {
    BBK_REQUIRE((s->flags & BBK_CANONICAL) && s->has_counts && s->sorted && !s->ref_order, BBK_ERR_ARG,
                "%s: needs an ascending canonical k-mer set with counts (bbk_count(BBK_CANONICAL | BBK_WITH_COUNTS))", who);
}

static void add_sample(bbk_kmerprofile_builder *b, unsigned sample, const bbk_kmerset *s) {
    bbk_ctx *ctx = b->ctx;
    check_sample_set(s, "bbk_kmerprofile_add_sample");
    BBK_REQUIRE(s->k == b->k, BBK_ERR_ARG, "bbk_kmerprofile_add_sample: the set holds %u-mers, the profile %u-mers", s->k,
                b->k);
    BBK_REQUIRE(sample < b->N, BBK_ERR_ARG, "bbk_kmerprofile_add_sample: sample %u of %u", sample, b->N);
    bbk_kmerprofile_builder::Sample &S = b->samples[sample];
    BBK_REQUIRE(!S.set, BBK_ERR_ARG, "bbk_kmerprofile_add_sample: sample %u was added before", sample);
    BBK_HIP(hipSetDevice(ctx->device));
    S.set = true;
    S.n = 0;
    if (s->n == 0) return;
    const size_t rec = (size_t)b->W * 8;
    const U32AtLeast counted{s->counts.as<uint32_t>(), (uint32_t)b->ci};
    const Selection sel = select_count(ctx, "kp_filter", s->n, counted);
    const uint64_t kept = sel.kept;
    if (kept == 0) return;
    S.keys.alloc(kept * rec);
    S.vals.alloc(kept * 2);
    dispatch_w(b->W, [&](auto w) {
        constexpr int W_ = decltype(w)::value;
        select_write(ctx, "kp_filter", sel, counted,
                     KpStoreSample<W_>{s->keys.as<Key<W_>>(), s->counts.as<uint32_t>(), (uint32_t)b->cs, S.keys.as<Key<W_>>(),
                                       S.vals.as<uint16_t>()});
    });
    BBK_HIP(hipStreamSynchronize(ctx->stream));
    S.n = kept;
}

static bbk_kmerprofile *finish_profile(bbk_kmerprofile_builder *b, uint64_t min_samples, uint64_t min_mult) {
    bbk_ctx *ctx = b->ctx;
    BBK_HIP(hipSetDevice(ctx->device));
    for (unsigned s = 0; s < b->N; ++s)
        BBK_REQUIRE(b->samples[s].set, BBK_ERR_ARG, "bbk_kmerprofile_finish: sample %u was never added", s);
    auto p = std::make_unique<bbk_kmerprofile>();
    p->k = b->k;
    p->W = b->W;
    p->N = b->N;
    p->max_value = b->cs;
    const unsigned N = b->N, W = b->W;
    const size_t rec = (size_t)W * 8;
    uint64_t total = 0;
    for (const auto &S : b->samples) total += S.n;
    // the union of the N ascending key arrays: one merge-unique of the engine's own sort
    DevBuf ukeys;
    uint64_t U = 0;
    if (total) {
        DevBuf cat(total * rec);
        uint64_t o = 0;
        for (const auto &S : b->samples) {
            if (!S.n) continue;
            BBK_HIP(copy_async(cat.as<char>() + o * rec, S.keys.p, S.n * rec, hipMemcpyDeviceToDevice, ctx->stream));
            o += S.n;
        }
        BBK_HIP(hipStreamSynchronize(ctx->stream));
        bbk_kmerset *u = nullptr;
        const int rc = bbk_kmerset_from_device_ex(ctx, cat.p, nullptr, total, b->k, 0, &u);
        if (rc != BBK_OK) throw Error{rc};
        U = u->n;
        ukeys = std::move(u->keys);
        bbk_kmerset_free(u);
    }
    if (U == 0) {
        p->keys.alloc(16);
        p->rows.alloc(16);
        build_profile_index(ctx, p.get());
        return p.release();
    }
    PrefixIndex uprefix;
    uprefix.build(ctx, ukeys.as<uint64_t>(), W, b->k, U);
    const PrefixTable UP = uprefix.table();
    DevBuf rows(U * (uint64_t)N * 2 + 16), err(16);
    BBK_HIP(hipMemsetAsync(rows.p, 0, U * (uint64_t)N * 2, ctx->stream));
    BBK_HIP(hipMemsetAsync(err.p, 0, 4, ctx->stream));
    for (unsigned s = 0; s < N; ++s) {
        auto &S = b->samples[s];
        if (!S.n) continue;
        dispatch_w(W, [&](auto w) {
            constexpr int W_ = decltype(w)::value;
            launch_items_timed(ctx, "kp_scatter", k_kp_scatter<W_>, S.n, S.keys.as<Key<W_>>(), S.vals.as<uint16_t>(),
                               S.n, ukeys.as<Key<W_>>(), UP, N, s, rows.as<uint16_t>(), err.as<uint32_t>());
        });
    }
    uint32_t h_err = 0;
    d2h_sync(ctx, &h_err, err.p, 4);
    BBK_REQUIRE(h_err == 0, BBK_ERR_INTERNAL, "bbk_kmerprofile_finish: a sample k-mer is missing from the union");
    for (auto &S : b->samples) {
        S.keys.release();
        S.vals.release();
    }
    DevBuf keep(U + 16);
    launch_items_timed(ctx, "kp_keep", k_kp_keep, U, rows.as<uint16_t>(), U, N, min_samples, min_mult, keep.as<uint8_t>());
    const KpKeepByte kept_byte{keep.as<uint8_t>()};
    const Selection sel = select_count(ctx, "kp_keep", U, kept_byte);
    const uint64_t kept = sel.kept;
    p->n = kept;
    p->keys.alloc(kept * rec);
    p->rows.alloc(kept * (uint64_t)N * 2);
    if (kept) {
        dispatch_w(W, [&](auto w) {
            constexpr int W_ = decltype(w)::value;
            select_write(ctx, "kp_compact", sel, kept_byte,
                         KpMoveRow<W_>{ukeys.as<Key<W_>>(), rows.as<uint16_t>(), N, p->keys.as<Key<W_>>(), p->rows.as<uint16_t>()});
        });
        BBK_HIP(hipStreamSynchronize(ctx->stream));
    }
    build_profile_index(ctx, p.get());
    return p.release();
}

static void abundance(bbk_ctx *ctx, const bbk_kmerprofile *p, const bbk_reads *pieces, const uint64_t *h_first, uint64_t nc,
                      uint64_t *h_n, uint64_t *h_positions, uint64_t *h_sum, uint64_t *h_sumsq) {
    BBK_HIP(hipSetDevice(ctx->device));
    if (nc == 0) return;
    const unsigned N = p->N;
    DevBuf first;
    if (h_first) {
        BBK_REQUIRE(h_first[0] == 0 && h_first[nc] == pieces->n, BBK_ERR_ARG,
                    "bbk_kmerprofile_abundance_pieces: first_piece must run from 0 to the number of pieces");
        for (uint64_t c = 0; c < nc; ++c)
            BBK_REQUIRE(h_first[c] <= h_first[c + 1], BBK_ERR_ARG,
                        "bbk_kmerprofile_abundance_pieces: first_piece must not decrease");
        first.alloc((nc + 1) * 8);
        BBK_HIP(hipMemcpyAsync(first.p, h_first, (nc + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    const uint64_t *d_first = h_first ? first.as<uint64_t>() : nullptr;
    DevBuf pos(nc * 8 + 16), off(nc * 8 + 16), err(16);
    BBK_HIP(hipMemsetAsync(err.p, 0, 4, ctx->stream));
    launch_items_timed(ctx, "ab_collect", k_ab_positions, nc, pieces->d_len, d_first, nc, (uint32_t)p->k,
                       pos.as<uint64_t>(), err.as<uint32_t>());
    uint32_t h_err = 0;
    BBK_HIP(hipMemcpyAsync(h_positions, pos.p, nc * 8, hipMemcpyDeviceToHost, ctx->stream));
    BBK_HIP(hipMemcpyAsync(&h_err, err.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    const uint64_t total = exclusive_scan_u64(ctx, pos.as<uint64_t>(), off.as<uint64_t>(), nc);
    BBK_REQUIRE(h_err == 0, BBK_ERR_ARG, "bbk_kmerprofile_abundance: a contig holds 2^32 k-mer positions or more");
    memset(h_n, 0, nc * 8);
    memset(h_sum, 0, nc * (size_t)N * 8);
    memset(h_sumsq, 0, nc * (size_t)N * 8);
    if (p->n == 0 || total == 0) return;
    DevBuf found(total * 8 + 16), dn(nc * 8 + 16), dsum(nc * (uint64_t)N * 8 + 16), dsq(nc * (uint64_t)N * 8 + 16);
    dispatch_w(p->W, [&](auto w) {
        constexpr int W_ = decltype(w)::value;
        launch_items_timed(ctx, "ab_collect", k_ab_collect<W_>, nc * 64, pieces->d_words, pieces->d_woff, pieces->d_len,
                           d_first, nc, (int)p->k, p->keys.as<Key<W_>>(), p->prefix.table(), off.as<uint64_t>(),
                           found.as<uint64_t>(), dn.as<uint64_t>());
    });
    const uint64_t waves = nc * (uint64_t)N;
    launch_items_timed(ctx, "ab_reduce", p->max_value > 255 ? k_ab_reduce<true> : k_ab_reduce<false>, waves * 64,
                       p->rows.as<uint16_t>(), N, found.as<uint64_t>(), off.as<uint64_t>(), dn.as<uint64_t>(), nc,
                       dsum.as<uint64_t>(), dsq.as<uint64_t>());
    BBK_HIP(hipMemcpyAsync(h_n, dn.p, nc * 8, hipMemcpyDeviceToHost, ctx->stream));
    BBK_HIP(hipMemcpyAsync(h_sum, dsum.p, waves * 8, hipMemcpyDeviceToHost, ctx->stream));
    BBK_HIP(hipMemcpyAsync(h_sumsq, dsq.p, waves * 8, hipMemcpyDeviceToHost, ctx->stream));
    BBK_HIP(hipStreamSynchronize(ctx->stream));
}

static void write_device(bbk_ctx *ctx, const std::string &path, const void *src, size_t bytes) {
    const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    BBK_REQUIRE(fd >= 0, BBK_ERR_IO, "cannot open %s for writing", path.c_str());
    const bool ok = bytes == 0 || d2f_big(ctx, fd, 0, src, bytes);
    const bool closed = close(fd) == 0;
    BBK_REQUIRE(ok && closed, BBK_ERR_IO, "writing %s failed", path.c_str());
}

static void read_file(const std::string &path, std::string &out) {
    const GraphError e = read_whole_file(path.c_str(), "cannot open %s", "short read of %s", out);
    BBK_REQUIRE(!e, BBK_ERR_IO, "%s", e.msg.c_str());
}

}  // namespace bbk

using namespace bbk;

extern "C" {

int bbk_kmerprofile_begin(bbk_ctx *ctx, unsigned k, unsigned n_samples, unsigned ci, unsigned cs,
                          bbk_kmerprofile_builder **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && out, BBK_ERR_ARG, "bbk_kmerprofile_begin: NULL argument");
        BBK_REQUIRE(k >= 1 && k < BBK_MAX_K, BBK_ERR_ARG, "k-mer size %u out of range [1,%d)", k, BBK_MAX_K);
        BBK_REQUIRE(n_samples >= 1 && n_samples <= 65535, BBK_ERR_ARG,
                    "bbk_kmerprofile_begin: %u samples, 1..65535 are supported", n_samples);
        BBK_REQUIRE(ci >= 1, BBK_ERR_ARG, "bbk_kmerprofile_begin: ci must be at least 1");
        BBK_REQUIRE(cs >= 1 && cs <= 65535, BBK_ERR_ARG,
                    "bbk_kmerprofile_begin: cs = %u does not fit the 16-bit rows of the profile (1..65535)", cs);
        auto b = std::make_unique<bbk_kmerprofile_builder>();
        b->ctx = ctx;
        b->k = k;
        b->W = words_of(k);
        b->N = n_samples;
        b->ci = ci;
        b->cs = cs;
        b->samples.resize(n_samples);
        *out = b.release();
    });
}

int bbk_kmerprofile_add_sample(bbk_kmerprofile_builder *b, unsigned sample, const bbk_kmerset *canonical_counts) {
    return guarded([&] {
        BBK_REQUIRE(b && canonical_counts, BBK_ERR_ARG, "bbk_kmerprofile_add_sample: NULL argument");
        add_sample(b, sample, canonical_counts);
    });
}

int bbk_kmerprofile_finish(bbk_kmerprofile_builder *b, uint64_t min_samples, uint64_t min_mult, bbk_kmerprofile **out) {
    std::unique_ptr<bbk_kmerprofile_builder> own(b);  // released on every path
    return guarded([&] {
        BBK_REQUIRE(b && out, BBK_ERR_ARG, "bbk_kmerprofile_finish: NULL argument");
        *out = finish_profile(b, min_samples, min_mult);
    });
}

void bbk_kmerprofile_abort(bbk_kmerprofile_builder *b) { delete b; }

uint64_t bbk_kmerprofile_size(const bbk_kmerprofile *p) { return p ? p->n : 0; }
unsigned bbk_kmerprofile_samples(const bbk_kmerprofile *p) { return p ? p->N : 0; }
unsigned bbk_kmerprofile_k(const bbk_kmerprofile *p) { return p ? p->k : 0; }

int bbk_kmerprofile_export(bbk_ctx *ctx, const bbk_kmerprofile *p, void *dst_keys, void *dst_rows) {
    return guarded([&] {
        BBK_REQUIRE(ctx && p, BBK_ERR_ARG, "bbk_kmerprofile_export: NULL argument");
        BBK_HIP(hipSetDevice(ctx->device));
        if (p->n == 0) return;
        if (dst_keys)
            BBK_HIP(hipMemcpyAsync(dst_keys, p->keys.p, p->n * (size_t)p->W * 8, hipMemcpyDefault, ctx->stream));
        if (dst_rows)
            BBK_HIP(hipMemcpyAsync(dst_rows, p->rows.p, p->n * (size_t)p->N * 2, hipMemcpyDefault, ctx->stream));
        BBK_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int bbk_kmerprofile_write(bbk_ctx *ctx, const bbk_kmerprofile *p, const char *prefix) {
    return guarded([&] {
        BBK_REQUIRE(ctx && p && prefix, BBK_ERR_ARG, "bbk_kmerprofile_write: NULL argument");
        BBK_HIP(hipSetDevice(ctx->device));
        write_device(ctx, std::string(prefix) + ".kmers", p->keys.p, p->n * (size_t)p->W * 8);
        write_device(ctx, std::string(prefix) + ".bpr", p->rows.p, p->n * (size_t)p->N * 2);
    });
}

int bbk_kmerprofile_load(bbk_ctx *ctx, const char *prefix, unsigned k, unsigned n_samples, bbk_kmerprofile **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && prefix && out, BBK_ERR_ARG, "bbk_kmerprofile_load: NULL argument");
        BBK_REQUIRE(k >= 1 && k < BBK_MAX_K, BBK_ERR_ARG, "k-mer size %u out of range [1,%d)", k, BBK_MAX_K);
        BBK_REQUIRE(n_samples >= 1 && n_samples <= 65535, BBK_ERR_ARG,
                    "bbk_kmerprofile_load: %u samples, 1..65535 are supported", n_samples);
        BBK_HIP(hipSetDevice(ctx->device));
        const std::string kp = std::string(prefix) + ".kmers", rp = std::string(prefix) + ".bpr";
        std::string kb, rb;
        read_file(kp, kb);
        read_file(rp, rb);
        const unsigned W = words_of(k);
        const size_t rec = (size_t)W * 8;
        BBK_REQUIRE(kb.size() % rec == 0, BBK_ERR_ARG, "%s: %zu bytes are not a whole number of %zu-byte %u-mer records",
                    kp.c_str(), kb.size(), rec, k);
        const uint64_t n = kb.size() / rec;
        BBK_REQUIRE(rb.size() == n * (size_t)n_samples * 2, BBK_ERR_ARG,
                    "%s: %zu bytes, %llu k-mers x %u samples x 2 bytes were expected", rp.c_str(), rb.size(),
                    (unsigned long long)n, n_samples);
        const uint64_t *kw = reinterpret_cast<const uint64_t *>(kb.data());
        for (uint64_t i = 1; i < n; ++i) {
            bool less = false;
            for (unsigned j = 0; j < W; ++j) {
                const uint64_t a = kw[(i - 1) * W + j], b = kw[i * W + j];
                if (a != b) {
                    less = a < b;
                    break;
                }
            }
            BBK_REQUIRE(less, BBK_ERR_ARG, "%s: record %llu is not above its predecessor (the k-mers must ascend)",
                        kp.c_str(), (unsigned long long)i);
        }
        const uint16_t *rv = reinterpret_cast<const uint16_t *>(rb.data());
        uint32_t mx = 0;
        for (uint64_t i = 0; i < n * n_samples; ++i) mx = rv[i] > mx ? rv[i] : mx;
        auto p = std::make_unique<bbk_kmerprofile>();
        p->k = k;
        p->W = W;
        p->N = n_samples;
        p->n = n;
        p->max_value = mx;
        p->keys.alloc(kb.size());
        p->rows.alloc(rb.size());
        if (n) {
            BBK_HIP(hipMemcpyAsync(p->keys.p, kb.data(), kb.size(), hipMemcpyHostToDevice, ctx->stream));
            BBK_HIP(hipMemcpyAsync(p->rows.p, rb.data(), rb.size(), hipMemcpyHostToDevice, ctx->stream));
            BBK_HIP(hipStreamSynchronize(ctx->stream));
        }
        build_profile_index(ctx, p.get());
        *out = p.release();
    });
}

int bbk_kmerprofile_abundance_pieces(bbk_ctx *ctx, const bbk_kmerprofile *p, const bbk_reads *pieces,
                                     const uint64_t *h_first_piece, uint64_t n_contigs, uint64_t *h_n,
                                     uint64_t *h_positions, uint64_t *h_sum, uint64_t *h_sumsq) {
    return guarded([&] {
        BBK_REQUIRE(ctx && p && pieces && h_first_piece, BBK_ERR_ARG, "bbk_kmerprofile_abundance_pieces: NULL argument");
        BBK_REQUIRE(n_contigs == 0 || (h_n && h_positions && h_sum && h_sumsq), BBK_ERR_ARG,
                    "bbk_kmerprofile_abundance_pieces: NULL output");
        abundance(ctx, p, pieces, h_first_piece, n_contigs, h_n, h_positions, h_sum, h_sumsq);
    });
}

int bbk_kmerprofile_abundance(bbk_ctx *ctx, const bbk_kmerprofile *p, const bbk_reads *contigs, uint64_t *h_n,
                              uint64_t *h_positions, uint64_t *h_sum, uint64_t *h_sumsq) {
    return guarded([&] {
        BBK_REQUIRE(ctx && p && contigs, BBK_ERR_ARG, "bbk_kmerprofile_abundance: NULL argument");
        BBK_REQUIRE(contigs->n == 0 || (h_n && h_positions && h_sum && h_sumsq), BBK_ERR_ARG,
                    "bbk_kmerprofile_abundance: NULL output");
        abundance(ctx, p, contigs, nullptr, contigs->n, h_n, h_positions, h_sum, h_sumsq);
    });
}

void bbk_kmerprofile_free(bbk_kmerprofile *p) { delete p; }

}  // extern "C"
