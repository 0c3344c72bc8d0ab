// count.hip -- k-mer extraction + counting on the device, and the bbk_kmerset part of the C ABI.
//
// Replaces, for one batch of reads resident in HBM:
//   BufferFiller::operator()            reference projects/kmercount/main.cpp:64-82
//   DeBruijnKMerSplitter::FillBufferFromSequence  common/utils/kmer_mph/kmer_splitters.hpp:25-41
//   KMerSortingSplitter::DumpBuffers    common/utils/kmer_mph/kmer_splitter.hpp:120-167 (sort + unique)
//   KMerDiskCounter::Count / MergeKMers common/utils/kmer_mph/kmer_index_builder.hpp:241-267,281-365
//   KMerDiskStorage::merge              kmer_index_builder.hpp:168-181 (the final_kmers order)
// The reference materialises both strands (RCWrap) and filters with IsMinimal; here every read
// position yields ONE canonical key (min(kmer, rc) in base order, rtseq.hpp:407-415) and the
// both-strand set of spades-kmercount is recovered from the distinct canonical keys as
// canon U rc(canon)  (SURVEY.md 7.4).
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "bbk_internal.h"
#include "kmer_ops.h"
#include "msd.h"
#include "accum.h"

namespace bbk {

// BBK_DISABLE_MSD=1 forces the LSD path (A/B timing, and tests that cover both paths)
static bool msd_enabled() {
    const char *e = getenv("BBK_DISABLE_MSD");
    return !(e && e[0] == '1');
}

// One wavefront per read, lanes over k-mer positions: stores of one wave are 64 consecutive
// records.  MODE 0: canonical key.  MODE 1: canonical key + InOutMask bits of this occurrence
// (kmer_extension_index.hpp:67-69,92-106: a non-minimal k-mer stores position 7-pos).
template <int W, int MODE>
__global__ __launch_bounds__(256) void k_extract(const uint64_t *__restrict__ words,
                                                const uint64_t *__restrict__ woff,
                                                const uint32_t *__restrict__ len,
                                                const uint64_t *__restrict__ koff, uint64_t n_reads, int k,
                                                Key<W> *__restrict__ out, uint32_t *__restrict__ out_val) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (BBK_GID()) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t r = wave; r < n_reads; r += nwaves) {
        const uint32_t L = len[r];
        if (L < (uint32_t)k) continue;
        const uint32_t nk = L - (uint32_t)k + 1;
        const uint64_t *rw = words + woff[r];
        const uint64_t base = koff[r];
        for (uint32_t p = lane; p < nk; p += 64) {
            const Key<W> fwd = kmer_extract<W>(rw, p, k);
            const Key<W> rc = kmer_rc<W>(fwd, k);
            const bool minimal = !kmer_less_nucl<W>(rc, fwd);  // fwd <= rc (palindrome -> minimal)
            out[base + p] = key_select<W>(minimal, fwd, rc);
            if (MODE == 1) {
                uint32_t m = 0;
                if (p + (uint32_t)k < L) {  // (k+1)-mer starting at p: outgoing base of this k-mer
                    const uint32_t c = base_at(rw, p + (uint32_t)k);
                    m |= 1u << (minimal ? c : 7u - c);
                }
                if (p >= 1) {  // (k+1)-mer starting at p-1: incoming base
                    const uint32_t c = base_at(rw, p - 1);
                    m |= 1u << (minimal ? 4u + c : 3u - c);
                }
                out_val[base + p] = m;
            }
        }
    }
}

// out[2i] = key, out[2i+1] = rc(key): the both-strand set of spades-kmercount
// TAG (8-byte keys with >= 4 spare bits): the XXH3 bucket of 16 (KMerSegmentPolicy, kmer_buckets.hpp:28-33) is
// put right above the k-mer (bits 2k..2k+3), so that one ascending sort of the tagged keys yields the
// final_kmers order
template <int W, bool TAG>
__global__ __launch_bounds__(256) void k_expand_rc(const Key<W> *__restrict__ in, const uint32_t *__restrict__ cin,
                                                  uint64_t n, int k, Key<W> *__restrict__ out,
                                                  uint32_t *__restrict__ cout) {
    const uint64_t i = BBK_GID();
    if (i >= n) return;
    Key<W> x = in[i];
    Key<W> y = kmer_rc<W>(x, k);
    if (TAG) {
        x.w[0] |= __umul64hi(xxh3_64<W>(x), 16ull) << (2 * k);
        y.w[0] |= __umul64hi(xxh3_64<W>(y), 16ull) << (2 * k);
    }
    out[2 * i] = x;
    out[2 * i + 1] = y;
    if (cin) {
        const uint32_t c = cin[i];
        cout[2 * i] = c;
        cout[2 * i + 1] = c;
    }
}

// neighbours of the stored order: out[0] += strict descents (key[i+1] < key[i] in word order), out[1] += equal
// neighbours, out[2..] = the first positions i of a descent (out[2 + 32] of them at most)
template <int W>
__global__ __launch_bounds__(256) void k_order_check(const Key<W> *__restrict__ keys, uint64_t n,
                                                    unsigned long long *__restrict__ out) {
    const uint64_t i = BBK_GID();
    if (i + 1 >= n) return;
    const Key<W> a = key_load<W>(&keys[i]), b = key_load<W>(&keys[i + 1]);
    if (key_less_words<W>(b, a)) {
        const unsigned long long at = atomicAdd(&out[0], 1ull);
        if (at < 32) out[2 + at] = i;
    } else if (key_eq<W>(a, b)) {
        atomicAdd(&out[1], 1ull);
    }
}

// one thread per bucket boundary b = 0..16 of a set in the final_kmers order (XXH3 bucket ids never decrease):
// out[b] = first record whose bucket is >= b
template <int W>
__global__ void k_bucket_bounds(const Key<W> *__restrict__ keys, uint64_t n, unsigned long long *__restrict__ out) {
    const uint32_t b = threadIdx.x;
    if (b > 16) return;
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        const uint32_t bm = (uint32_t)__umul64hi(xxh3_64<W>(key_load<W>(&keys[mid])), 16ull);
        if (bm < b) lo = mid + 1;
        else hi = mid;
    }
    out[b] = lo;
}

template <int W>
static void launch_extract(bbk_ctx *ctx, const bbk_reads *rd, const uint64_t *koff, int k, void *out, uint32_t *vals,
                           uint64_t n_inst) {
    const unsigned blocks = (unsigned)std::min<uint64_t>((rd->n + 3) / 4, (uint64_t)ctx->num_cus * 32);
    KernelTimer t(ctx, "extract", (double)rd->n_words * 8 + (double)n_inst * (sizeof(Key<W>) + (vals ? 4 : 0)));
    if (vals)
        hipLaunchKernelGGL((k_extract<W, 1>), dim3(blocks ? blocks : 1), dim3(256), 0, ctx->stream, rd->d_words,
                           rd->d_woff, rd->d_len, koff, rd->n, k, (Key<W> *)out, vals);
    else
        hipLaunchKernelGGL((k_extract<W, 0>), dim3(blocks ? blocks : 1), dim3(256), 0, ctx->stream, rd->d_words,
                           rd->d_woff, rd->d_len, koff, rd->n, k, (Key<W> *)out, (uint32_t *)nullptr);
    check_launch("k_extract");
}

template <int W>
static void launch_expand(bbk_ctx *ctx, const void *in, const uint32_t *cin, uint64_t n, int k, void *out,
                          uint32_t *cout, bool tag) {
    if (n == 0) return;
    KernelTimer t(ctx, "expand", 3.0 * (double)n * sizeof(Key<W>));
    launch_items(ctx, "k_expand_rc", tag ? k_expand_rc<W, true> : k_expand_rc<W, false>, n, (const Key<W> *)in, cin, n,
                 k, (Key<W> *)out, cout);
}

// the result of a call that found no record: 16-byte buffers, so that a set's pointers are never null
static void empty_result(DevBuf &keys, DevBuf *vals) {
    keys.alloc(16);
    if (vals) vals->alloc(16);
}

// ---- the general (LSD) path: what every MSD call that declines falls back to ------------------------------------
// Owns the scratch of one radix sort of n records: a key pair and, with a payload, a payload pair.  The records come
// in either from a producer kernel that writes keys.p / vals.p itself (extract, expand) or as a copy of a const
// device array (load); sort() orders them in place, unique() reduces them into buffers of the caller.  n < 2^32: the
// callers refuse larger inputs with a message of their own.
struct LsdSort {
    bbk_ctx *ctx;
    unsigned k;
    uint64_t n;
    int W;
    size_t rec;
    DevBuf keys, tmp, vals, vtmp;
    LsdSort(bbk_ctx *c, unsigned k_, uint64_t n_, bool payload)
        : ctx(c), k(k_), n(n_), W((int)words_of(k_)), rec((size_t)W * 8), keys(n_ * rec), tmp(n_ * rec) {
        if (payload) {
            vals.alloc(n * 4);
            vtmp.alloc(n * 4);
        }
    }
    void load(const void *d_keys, const uint32_t *d_vals) {
        BBK_HIP(bbk::copy_async(keys.p, d_keys, n * rec, hipMemcpyDeviceToDevice, ctx->stream));
        if (vals.p) BBK_HIP(bbk::copy_async(vals.p, d_vals, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    }
    void sort() { sort_records(ctx, W, keys.p, tmp.p, vals.as<uint32_t>(), vtmp.as<uint32_t>(), n, key_passes(k)); }
    // The distinct records of the sorted array into out_keys and, when out_vals is given, their payloads reduced with
    // `op` (REDUCE_COUNT without a payload: the run lengths) into *out_vals: exact size + 16 bytes of slack.  The
    // distinct records land in the scratch's second half (sized for the worst case) first; one wait, at the end.
    uint64_t unique(ReduceOp op, DevBuf &out_keys, DevBuf *out_vals) {
        if (out_vals && !vtmp.p) vtmp.alloc(n * 4);
        uint32_t *rv = out_vals ? vtmp.as<uint32_t>() : nullptr;
        const uint64_t D = unique_records(ctx, W, keys.p, vals.as<uint32_t>(), n, tmp.p, rv, op);
        keys.release();
        vals.release();
        out_keys.alloc(D * rec + 16);
        BBK_HIP(bbk::copy_async(out_keys.p, tmp.p, D * rec, hipMemcpyDeviceToDevice, ctx->stream));
        if (rv) {
            out_vals->alloc(D * 4 + 16);
            BBK_HIP(bbk::copy_async(out_vals->p, rv, D * 4, hipMemcpyDeviceToDevice, ctx->stream));
        }
        stream_wait(ctx);
        return D;
    }
};

// ---- stage A: distinct canonical records (+ reduced payload) of one batch of reads, in ANY order ------------
// payload: with_mask -> OR of the InOutMask bits of every occurrence; want_vals -> multiplicity.
// MSD path (hash-partitioned dedup in LDS, hash-range passes above one device pass); LSD fallback = extract, sort,
// unique (its output happens to be ascending).
// view: the caller takes the result as a BucketView where the narrow MSD pass leaves one (out_keys then stays empty)
void dedup_reads(bbk_ctx *ctx, const bbk_reads *rd, unsigned k, bool with_mask, bool want_vals, DevBuf &out_keys,
                 DevBuf &out_vals, uint64_t &n_distinct, uint64_t &n_instances, BucketView *view = nullptr) {
    n_distinct = 0;
    n_instances = 0;
    if (msd_enabled()) {
        const int op1 = with_mask ? MSD_OP_OR : (want_vals ? MSD_OP_COUNT : MSD_OP_NONE);
        if (superk_dedup_reads(ctx, rd, k, op1, out_keys, out_vals, n_distinct, n_instances)) return;
        n_distinct = 0;
        n_instances = 0;
        MsdOutput a;
        a.want_view = view != nullptr;
        if (msd_sort_reduce(ctx, k, MsdRequest::reads(MSD_HASH, op1, rd, with_mask), a)) {
            n_instances = a.instances;
            n_distinct = a.n;
            if (a.view.live()) *view = std::move(a.view);
            out_keys = std::move(a.keys);
            if (op1 != MSD_OP_NONE) out_vals = std::move(a.vals);
            return;
        }
    }
    ReadPlan rp;  // units of one k-mer: the scan of the k-mers per read, straight from the lengths
    rp.run(ctx, rd, k, 1u, nullptr);
    const DevBuf &koff = rp.coff;
    const uint64_t N = rp.kmers;
    n_instances = N;
    if (N == 0) return empty_result(out_keys, &out_vals);
    BBK_REQUIRE(N < (1ull << 32), BBK_ERR_ARG,
                "batch holds %llu k-mer instances; the LSD path is limited to 2^32-1 per batch (push the reads in "
                "smaller batches)",
                (unsigned long long)N);
    LsdSort t(ctx, k, N, with_mask);  // the extraction writes straight into the scratch
    dispatch_w(t.W, [&](auto w) {
        launch_extract<decltype(w)::value>(ctx, rd, koff.as<uint64_t>(), (int)k, t.keys.p, t.vals.as<uint32_t>(), N);
    });
    t.sort();
    n_distinct =
        t.unique(with_mask ? REDUCE_OR : REDUCE_COUNT, out_keys, (with_mask || want_vals) ? &out_vals : nullptr);
}

// LSD sort + unique of a record array: the fallback of the three callers below
static uint64_t lsd_sort_unique(bbk_ctx *ctx, unsigned k, const void *d_keys, const uint32_t *d_vals, uint64_t n,
                                ReduceOp rop, DevBuf &out_keys, DevBuf &out_vals) {
    LsdSort t(ctx, k, n, d_vals != nullptr);
    t.load(d_keys, d_vals);
    t.sort();
    return t.unique(rop, out_keys, d_vals ? &out_vals : nullptr);
}

// Distinct records of a record array (payloads reduced with the MSD_OP_* `op`), hash-bucket order (prefix MSD_HASH) or
// ascending (MSD_KEYS).  The general path orders either way.
static uint64_t reduce_records(bbk_ctx *ctx, unsigned k, MsdRequest rq, DevBuf &out_keys, DevBuf &out_vals) {
    if (rq.n == 0) {
        empty_result(out_keys, rq.vals ? &out_vals : nullptr);
        return 0;
    }
    if (msd_enabled()) {
        MsdOutput m;
        if (msd_sort_reduce(ctx, k, rq, m)) {
            out_keys = std::move(m.keys);
            if (rq.op != MSD_OP_NONE) out_vals = std::move(m.vals);
            return m.n;
        }
    }
    BBK_REQUIRE(rq.n < (1ull << 32), BBK_ERR_ARG, "%llu records exceed the LSD path's 2^32-1",
                (unsigned long long)rq.n);
    const ReduceOp rop = rq.op == MSD_OP_OR ? REDUCE_OR : REDUCE_SUM;
    return lsd_sort_unique(ctx, k, rq.keys, rq.vals, rq.n, rop, out_keys, out_vals);
}

// Distinct records of a record array (payloads summed / OR-ed), in ANY order: the merge step of the streaming
// count (MergeKMers analogue, kmer_index_builder.hpp:281-365) and of the multi-GPU exchange.
static uint64_t dedup_keys(bbk_ctx *ctx, unsigned k, const void *d_keys, const uint32_t *d_vals, uint64_t n, int op,
                           DevBuf &out_keys, DevBuf &out_vals) {
    return reduce_records(ctx, k, MsdRequest::records(MSD_HASH, op, d_keys, d_vals, n), out_keys, out_vals);
}

// ---- stage B: a distinct set -> ascending (word 0 most significant, adt/array_vector.hpp:114-123) ---------------
static uint64_t sort_distinct(bbk_ctx *ctx, unsigned k, const void *d_keys, const uint32_t *d_vals, uint64_t n, int op,
                              DevBuf &out_keys, DevBuf &out_vals) {
    // the input is distinct: stage B only orders it (assume_distinct: the sorted result is written directly)
    MsdRequest rq = MsdRequest::records(MSD_KEYS, d_vals ? op : MSD_OP_NONE, d_keys, d_vals, n);
    rq.assume_distinct = true;
    return reduce_records(ctx, k, rq, out_keys, out_vals);
}

// ---- accumulator of the streaming entry points -----------------------------------------------------------------
// What the reference gets from bounded per-thread cells, repeated DumpBuffers rounds (one sorted + uniqued run per
// bucket and round, kmer_splitter.hpp:73-167) and the final loser-tree run merge (MergeKMers,
// kmer_index_builder.hpp:281-365): the input never has to be resident as a whole.  Here every pushed batch is
// deduplicated on its own (stage A) and kept as a "run" of distinct canonical records; runs are merge-uniqued into
// the accumulated set whenever they outweigh half of it (so the total merge work stays linear in the input), and
// finish() orders the set once.

// a count whose stage B may read stage A's buckets in place: both strands without payload, 8-byte keys, odd k (the
// ordering pass takes the key slots only for a distinct expanded set)
static bool view_wanted(unsigned k, unsigned flags) {
    return (flags & BBK_BOTH_STRANDS) && !(flags & (BBK_WITH_COUNTS | BBK_WITH_MASKS)) && words_of(k) == 1 && (k & 1);
}

Accum::Accum(bbk_ctx *c, unsigned k_, unsigned count_flags)
    : ctx(c),
      k(k_),
      with_mask((count_flags & BBK_WITH_MASKS) != 0),
      want_vals((count_flags & BBK_WITH_COUNTS) != 0),
      want_view(view_wanted(k_, count_flags)) {}

bool Accum::has_vals() const { return with_mask || want_vals; }
int Accum::merge_op() const { return with_mask ? MSD_OP_OR : (want_vals ? MSD_OP_SUM : MSD_OP_NONE); }

void Accum::push(const bbk_reads *rd) {
    dense();  // a second batch: the first one's set is an ordinary run
    auto one = [&](const bbk_reads *part, bool may_view) {
        Run r;
        uint64_t inst = 0;
        dedup_reads(ctx, part, k, with_mask, want_vals, r.keys, r.vals, r.n, inst, may_view ? &r.view : nullptr);
        instances += inst;
        if (r.n == 0) return;
        runs_n += r.n;
        runs.push_back(std::move(r));
    };
    // 8-byte keys: one call above one pass of stage A (1.6 G instances with narrow records) would run in hash ranges,
    // and every range re-extracts every k-mer of the reads (100 M x 150 bp, k = 21: 7 ranges, 525 of 615 ms).  The
    // reads are cut into pieces of one pass each instead -- what a caller that pushes blocks gets anyway -- and the runs
    // are merged once.  (Wider keys go through super-k-mer records, which never re-extract.)
    const char *ec = getenv("BBK_READ_CHUNK");  // tests: bases per piece
    const uint64_t piece = ec ? strtoull(ec, nullptr, 10) : 1500000000ull;
    if (words_of(k) == 1 && rd->n >= 2 && rd->bases > piece && msd_enabled()) {
        const uint64_t np = (rd->bases + piece - 1) / piece, per = (rd->n + np - 1) / np;
        if (getenv("BBK_VERBOSE"))
            fprintf(stderr, "[bbk] count: %llu reads in %llu pieces of %llu\n", (unsigned long long)rd->n,
                    (unsigned long long)((rd->n + per - 1) / per), (unsigned long long)per);
        for (uint64_t r0 = 0; r0 < rd->n; r0 += per) {
            bbk_reads v;  // a view: owns nothing
            v.ctx = rd->ctx;
            v.n = std::min<uint64_t>(per, rd->n - r0);
            v.n_words = rd->n_words;
            v.bases = (uint64_t)((double)rd->bases * (double)v.n / (double)rd->n);
            v.d_words = rd->d_words;
            v.d_woff = rd->d_woff + r0;
            v.d_len = rd->d_len + r0;
            one(&v, false);
        }
    } else {
        one(rd, want_view && !has_vals() && batches == 0 && n == 0 && runs.empty());
    }
    ++batches;
    static const char *e = getenv("BBK_MERGE_MIN");  // tests force a merge after every push
    const uint64_t floor_n = e ? strtoull(e, nullptr, 10) : (32ull << 20);
    if ((runs.size() > 1 || n) && runs_n >= n / 2 + floor_n) merge();
}

void Accum::push_records(const void *d_keys, const uint32_t *d_vals, uint64_t n_rec) {
    if (n_rec == 0) return;
    Run r;
    r.n = dedup_keys(ctx, k, d_keys, has_vals() ? d_vals : nullptr, n_rec, merge_op(), r.keys, r.vals);
    instances += n_rec;
    ++batches;
    runs_n += r.n;
    runs.push_back(std::move(r));
}

// accumulated set + runs -> accumulated set
void Accum::dense() {
    auto one = [&](BucketView &v, DevBuf &kb) {
        if (!v.live()) return;
        v.materialise(ctx);
        kb = std::move(v.keys);
    };
    one(view, keys);
    for (Run &r : runs) one(r.view, r.keys);
}

void Accum::merge() {
    if (runs.empty()) return;
    if (n == 0 && runs.size() == 1) {  // first batch: adopt
        keys = std::move(runs[0].keys);
        vals = std::move(runs[0].vals);
        view = std::move(runs[0].view);
        n = runs[0].n;
        runs.clear();
        runs_n = 0;
        return;
    }
    dense();
    const size_t rec = (size_t)words_of(k) * 8;
    const uint64_t total = n + runs_n;
    DevBuf ck(total * rec + 16), cv;
    if (has_vals()) cv.alloc(total * 4 + 16);
    uint64_t o = 0;
    auto put = [&](DevBuf &kb, DevBuf &vb, uint64_t cnt) {
        if (!cnt) return;
        BBK_HIP(bbk::copy_async(ck.as<char>() + o * rec, kb.p, cnt * rec, hipMemcpyDeviceToDevice, ctx->stream));
        if (has_vals())
            BBK_HIP(bbk::copy_async(cv.as<uint32_t>() + o, vb.p, cnt * 4, hipMemcpyDeviceToDevice, ctx->stream));
        o += cnt;
        stream_wait(ctx);
        kb.release();
        vb.release();
    };
    put(keys, vals, n);
    for (Run &r : runs) put(r.keys, r.vals, r.n);
    runs.clear();
    runs_n = 0;
    n = dedup_keys(ctx, k, ck.p, cv.as<uint32_t>(), total, merge_op(), keys, vals);
    ++merges;
}

// the accumulated set in ascending order (payloads alongside); the accumulator is left empty
uint64_t Accum::finish_sorted(DevBuf &out_keys, DevBuf &out_vals) {
    merge();
    dense();
    const uint64_t D = sort_distinct(ctx, k, keys.p, has_vals() ? vals.as<uint32_t>() : nullptr, n, merge_op(), out_keys,
                                     out_vals);
    keys.release();
    vals.release();
    n = 0;
    return D;
}

// canon U rc(canon): expand, sort, unique.  A k-mer equal to its own RC (even k) appears twice
// and is merged by unique; its count doubles, as in the reference where both strands of such an
// occurrence are counted.
// want_ref: leave the set in the final_kmers order when that is free (tagged sort / REF prefix); s.ref_order tells.
// view: the canonical set is still in stage A's buckets (ck empty, no payload); stage B's level 1 reads it there
static void expand_both_strands(bbk_ctx *ctx, unsigned k, const DevBuf &ck, const DevBuf *cv, uint64_t D,
                                bbk_kmerset &s, bool want_ref = false, BucketView *view = nullptr) {
    const uint32_t *cvp = cv ? cv->as<uint32_t>() : nullptr;
    const int W = (int)words_of(k);
    if (D == 0) return empty_result(s.keys, cv ? &s.counts : nullptr);
    // (sets above one device pass -- 2^32 records and far less for wide keys -- are sorted in key-range passes inside
    // msd_sort_reduce; only the LSD fallback below keeps the 32-bit limit)
    if (msd_enabled()) {
        // fused: the level-1 partition kernels generate key, reverse complement (and tag) from the canonical array
        // themselves -- the expanded array is never written
        // TAG (8-byte keys with 4 spare bits) or REF prefix (every other key width): the XXH3 bucket above the key bits
        // gives the final_kmers order straight from the sort; BBK_NO_WIDE_REF=1: keys above 16 bytes are sorted
        // ascending and take one more stable pass on the bucket (to_reference_order)
        const bool tag = want_ref && W == 1 && 2 * k + 4 <= 64;
        const bool ref_prefix = want_ref && !tag && (W <= 2 || getenv("BBK_NO_WIDE_REF") == nullptr);
        const int prefix = ref_prefix ? MSD_REF : MSD_KEYS, op = cv ? MSD_OP_SUM : MSD_OP_NONE;
        MsdRequest rq =
            view ? MsdRequest::expand(prefix, op, k, *view) : MsdRequest::expand(prefix, op, k, ck.p, cvp, D);
        rq.tag_bits = tag ? 4u : 0u;
        rq.assume_distinct = (k & 1) != 0;  // odd k has no self-reverse-complementary k-mers
        MsdOutput m;
        if (msd_sort_reduce(ctx, k, rq, m)) {
            s.n = m.n;
            s.keys = std::move(m.keys);
            if (cv) s.counts = std::move(m.vals);
            s.ref_order = tag || ref_prefix;
            return;
        }
    }
    // general path: materialise the expanded array, sort, unique
    BBK_REQUIRE(2 * D < (1ull << 32), BBK_ERR_ARG, "too many distinct k-mers for the LSD path (%llu)", (unsigned long long)D);
    if (view) view->materialise(ctx);
    const void *ckp = view ? view->keys.p : ck.p;
    LsdSort t(ctx, k, 2 * D, cv != nullptr);
    dispatch_w(W, [&](auto w) {
        launch_expand<decltype(w)::value>(ctx, ckp, cvp, D, (int)k, t.keys.p, t.vals.as<uint32_t>(), false);
    });
    t.sort();
    s.n = t.unique(cv ? REDUCE_SUM : REDUCE_COUNT, s.keys, cv ? &s.counts : nullptr);
}

static void check_k(unsigned k) {
    // KMerCounter accepts any k in [1, MAX_K) (projects/kmercount/main.cpp has no parity check)
    BBK_REQUIRE(k >= 1 && k < BBK_MAX_K, BBK_ERR_ARG, "k-mer size %u out of range [1,%d)", k, BBK_MAX_K);
}

static std::unique_ptr<bbk_kmerset> new_kmerset(unsigned k, unsigned flags, bool has_counts, uint64_t instances) {
    auto s = std::make_unique<bbk_kmerset>();
    s->k = k;
    s->W = words_of(k);
    s->flags = flags;
    s->has_counts = has_counts;
    s->instances = instances;
    return s;
}

// CountAll(16, ...) (projects/kmercount/main.cpp:215): the XXH3 bucket of 16 as the digit of one stable pass.  Over an
// ascending set it yields the final_kmers order (KMerDiskStorage::merge, kmer_index_builder.hpp:168-181).
static PassDesc ref_bucket_pass() { return PassDesc{1, 0, 0, 8, 16}; }

// An ascending set -> the final_kmers order, counts alongside (the key widths and paths whose sort did not leave it
// there already).  No-op for a set in that order or without one (BBK_UNSORTED).
static void to_reference_order(bbk_ctx *ctx, bbk_kmerset &s) {
    if (s.ref_order || !s.sorted) return;
    if (s.n) {
        DevBuf nk(s.n * (size_t)s.W * 8), nc;
        if (s.has_counts) nc.alloc(s.n * 4);
        partition_records(ctx, (int)s.W, s.keys.p, nk.p, s.has_counts ? s.counts.as<uint32_t>() : nullptr,
                          nc.as<uint32_t>(), s.n, ref_bucket_pass());
        s.keys = std::move(nk);
        if (s.has_counts) s.counts = std::move(nc);
    }
    s.ref_order = true;
}

// The both-strand set of spades-kmercount from the accumulated canonical set.  consume: the accumulator is left empty
// (a bucket view is read in place); otherwise it keeps its records, dense (bbk_extindex_finish_with_set: the extension
// index is built from them afterwards).  carry_payload: the multiplicities travel with the keys.
bbk_kmerset *finish_both_strands(Accum &acc, unsigned flags, bool consume, bool carry_payload) {
    auto s = new_kmerset(acc.k, flags, carry_payload, 2 * acc.instances);
    acc.merge();
    if (!consume) acc.dense();
    expand_both_strands(acc.ctx, acc.k, acc.keys, carry_payload ? &acc.vals : nullptr, acc.n, *s,
                        (flags & BBK_REFERENCE_ORDER) != 0, acc.view.live() ? &acc.view : nullptr);
    if (consume) {
        acc.keys.release();
        acc.vals.release();
        acc.view = BucketView();
        acc.n = 0;
    }
    if (flags & BBK_REFERENCE_ORDER) to_reference_order(acc.ctx, *s);
    return s.release();
}

// finish of a count: the accumulated distinct canonical set -> the bbk_kmerset the flags ask for
static bbk_kmerset *finish_count(Accum &acc, unsigned flags) {
    const bool wc = (flags & (BBK_WITH_COUNTS | BBK_WITH_MASKS)) != 0;  // a u32 payload travels with the keys
    if (flags & BBK_BOTH_STRANDS) return finish_both_strands(acc, flags, /*consume=*/true, wc);
    auto s = new_kmerset(acc.k, flags, wc, acc.instances);
    acc.merge();
    if (flags & BBK_UNSORTED) {
        s->n = acc.n;
        s->sorted = false;
        s->keys = std::move(acc.keys);
        if (wc) s->counts = std::move(acc.vals);
        if (!s->keys.p) empty_result(s->keys, nullptr);
        acc.n = 0;
    } else {
        s->n = acc.finish_sorted(s->keys, s->counts);
    }
    if (flags & BBK_REFERENCE_ORDER) to_reference_order(acc.ctx, *s);
    return s.release();
}

// finish of a count that keeps only the records whose exported multiplicity reaches min_count (the exact form of
// KMerDataCounter::BuildKMerIndex with count_filter_singletons, projects/hammer/kmer_data.cpp:280-335).  The filter runs on
// the accumulated canonical records, before the expansion and the ordering: a canonical record's count is the
// multiplicity both of its strands will report, and the full both-strand set never exists.  With BBK_WITH_COUNTS the
// accumulator carries payloads, so no bucket view is live here (view_wanted) and the records are dense after merge().
static bbk_kmerset *finish_count_min(Accum &acc, unsigned flags, uint32_t min_count, uint64_t *n_dropped) {
    *n_dropped = 0;
    if (min_count <= 1) return finish_count(acc, flags);
    acc.merge();
    const bool both = (flags & BBK_BOTH_STRANDS) != 0;
    const uint64_t before = acc.n;
    uint64_t self_rc = 0;  // dropped records that are their own reverse complement: one record of the expanded set each
    acc.n = filter_min_count(acc.ctx, acc.k, both && !(acc.k & 1), min_count, acc.keys, acc.vals, acc.n, &self_rc);
    *n_dropped = both ? 2 * (before - acc.n) - self_rc : before - acc.n;
    return finish_count(acc, flags);
}

static void check_count_flags(unsigned flags) {
    const bool both = (flags & BBK_BOTH_STRANDS) != 0, canon = (flags & BBK_CANONICAL) != 0;
    BBK_REQUIRE(both != canon, BBK_ERR_ARG, "bbk_count: pass exactly one of BBK_BOTH_STRANDS / BBK_CANONICAL");
    BBK_REQUIRE(!((flags & BBK_REFERENCE_ORDER) && (flags & BBK_UNSORTED)), BBK_ERR_ARG,
                "bbk_count: BBK_REFERENCE_ORDER and BBK_UNSORTED exclude each other");
    BBK_REQUIRE(!(flags & BBK_WITH_MASKS) || (canon && !(flags & BBK_WITH_COUNTS)), BBK_ERR_ARG,
                "bbk_count: BBK_WITH_MASKS goes with BBK_CANONICAL and without BBK_WITH_COUNTS");
}

}  // namespace bbk

using namespace bbk;

struct bbk_counter {
    bbk::Accum acc;
    unsigned flags;
    bbk_counter(bbk_ctx *ctx, unsigned k, unsigned f) : acc(ctx, k, f), flags(f) {}
};

extern "C" {

int bbk_count_begin(bbk_ctx *ctx, unsigned k, unsigned flags, bbk_counter **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && out, BBK_ERR_ARG, "bbk_count_begin: NULL argument");
        check_k(k);
        check_count_flags(flags);
        *out = new bbk_counter(ctx, k, flags);
    });
}

int bbk_count_push_reads(bbk_counter *c, const bbk_reads *reads) {
    return guarded([&] {
        BBK_REQUIRE(c && reads, BBK_ERR_ARG, "bbk_count_push_reads: NULL argument");
        BBK_HIP(hipSetDevice(c->acc.ctx->device));
        c->acc.push(reads);
    });
}

int bbk_count_push_ascii(bbk_counter *c, const char *h_bases, const uint64_t *h_offsets, uint64_t n_reads) {
    if (!c) {
        set_error("bbk_count_push_ascii: NULL argument");
        return BBK_ERR_ARG;
    }
    bbk_reads *r = nullptr;
    const int rc = bbk_reads_from_ascii(c->acc.ctx, h_bases, h_offsets, n_reads, &r);
    if (rc != BBK_OK) return rc;
    const int rc2 = bbk_count_push_reads(c, r);
    bbk_reads_free(r);
    return rc2;
}

int bbk_count_finish(bbk_counter *c, bbk_kmerset **out) {
    const int rc = guarded([&] {
        BBK_REQUIRE(c && out, BBK_ERR_ARG, "bbk_count_finish: NULL argument");
        BBK_HIP(hipSetDevice(c->acc.ctx->device));
        *out = finish_count(c->acc, c->flags);
    });
    delete c;  // finished or failed: the counter is gone either way
    return rc;
}

int bbk_count_finish_min_count(bbk_counter *c, uint32_t min_count, bbk_kmerset **out, uint64_t *n_dropped) {
    const int rc = guarded([&] {
        BBK_REQUIRE(c && out && n_dropped, BBK_ERR_ARG, "bbk_count_finish_min_count: NULL argument");
        BBK_REQUIRE(c->flags & BBK_WITH_COUNTS, BBK_ERR_ARG,
                    "bbk_count_finish_min_count: the counter was begun without BBK_WITH_COUNTS");
        BBK_HIP(hipSetDevice(c->acc.ctx->device));
        *out = finish_count_min(c->acc, c->flags, min_count, n_dropped);
    });
    delete c;
    return rc;
}

void bbk_count_abort(bbk_counter *c) { delete c; }

uint64_t bbk_count_pushed_instances(const bbk_counter *c) { return c ? c->acc.instances : 0; }

int bbk_count(bbk_ctx *ctx, const bbk_reads *reads, unsigned k, unsigned flags, bbk_kmerset **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && reads && out, BBK_ERR_ARG, "bbk_count: NULL argument");
        check_k(k);
        check_count_flags(flags);
        BBK_HIP(hipSetDevice(ctx->device));
        // one batch through the streaming accumulator: hash-partitioned dedup of the canonical stream (stage A),
        // then expand + sort once (stage B)
        Accum acc(ctx, k, flags);
        acc.push(reads);
        *out = finish_count(acc, flags);
    });
}

const void *bbk_kmerset_keys(const bbk_kmerset *s, unsigned *order) {
    if (!s) return nullptr;
    if (order) *order = !s->sorted ? 0xFFFFFFFFu : (s->ref_order ? BBK_ORDER_REFERENCE_BUCKETS16 : BBK_ORDER_SORTED);
    return s->keys.p;
}

int bbk_kmerset_from_device(bbk_ctx *ctx, const void *d_keys, const void *d_counts, uint64_t n, unsigned k,
                            bbk_kmerset **out) {
    return bbk_kmerset_from_device_ex(ctx, d_keys, d_counts, n, k, 0, out);
}

int bbk_kmerset_from_device_ex(bbk_ctx *ctx, const void *d_keys, const void *d_counts, uint64_t n, unsigned k,
                               unsigned flags, bbk_kmerset **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && out && (n == 0 || d_keys), BBK_ERR_ARG, "bbk_kmerset_from_device: NULL argument");
        check_k(k);
        BBK_HIP(hipSetDevice(ctx->device));
        const uint32_t *d_vals = (const uint32_t *)d_counts;
        auto s = new_kmerset(k, flags, d_vals != nullptr, n);
        const bool unsorted = (flags & BBK_UNSORTED) != 0;
        const MsdRequest rq =
            MsdRequest::records(unsorted ? MSD_HASH : MSD_KEYS, d_vals ? MSD_OP_SUM : MSD_OP_NONE, d_keys, d_vals, n);
        MsdOutput m;
        if (n == 0) {
            empty_result(s->keys, d_vals ? &s->counts : nullptr);
        } else if (msd_enabled() && msd_sort_reduce(ctx, k, rq, m)) {
            s->n = m.n;
            s->sorted = !unsorted;
            s->keys = std::move(m.keys);
            if (d_vals) s->counts = std::move(m.vals);
        } else {  // the general path orders either way
            s->n = lsd_sort_unique(ctx, k, d_keys, d_vals, n, d_vals ? REDUCE_SUM : REDUCE_COUNT, s->keys, s->counts);
        }
        *out = s.release();
    });
}

int bbk_kmerset_both_strands(bbk_ctx *ctx, const bbk_kmerset *canon, bbk_kmerset **out) {
    return bbk_kmerset_both_strands_ex(ctx, canon, 0, out);
}

int bbk_kmerset_both_strands_ex(bbk_ctx *ctx, const bbk_kmerset *canon, unsigned flags, bbk_kmerset **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && canon && out, BBK_ERR_ARG, "bbk_kmerset_both_strands: NULL argument");
        BBK_REQUIRE((flags & ~BBK_REFERENCE_ORDER) == 0, BBK_ERR_ARG,
                    "bbk_kmerset_both_strands_ex: only BBK_REFERENCE_ORDER is accepted");
        BBK_HIP(hipSetDevice(ctx->device));
        auto s = new_kmerset(canon->k, (canon->flags & ~(BBK_CANONICAL | BBK_UNSORTED)) | BBK_BOTH_STRANDS | flags,
                             canon->has_counts, 2 * canon->instances);
        const bool want_ref = (flags & BBK_REFERENCE_ORDER) != 0;
        expand_both_strands(ctx, canon->k, canon->keys, canon->has_counts ? &canon->counts : nullptr, canon->n, *s,
                            want_ref);
        if (want_ref) to_reference_order(ctx, *s);
        *out = s.release();
    });
}

// ---- bbk_kmerset: accessors, export, verification -----------------------------------------------------------------
uint64_t bbk_kmerset_size(const bbk_kmerset *s) { return s ? s->n : 0; }
unsigned bbk_kmerset_k(const bbk_kmerset *s) { return s ? s->k : 0; }
uint64_t bbk_kmerset_instances(const bbk_kmerset *s) { return s ? s->instances : 0; }

static bool is_device_ptr(const void *p) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();  // plain host memory is not an error
        return false;
    }
    return at.type == hipMemoryTypeDevice;
}

static void export_ordered(bbk_ctx *ctx, const bbk_kmerset *s, const PassDesc *pd, void *dst_keys, void *dst_counts,
                           uint64_t *h_counts) {
    BBK_HIP(hipSetDevice(ctx->device));
    // an unsorted set may only be partitioned by owner (order inside a segment is irrelevant there)
    BBK_REQUIRE(s->sorted || (pd && pd->kind == 2), BBK_ERR_ARG,
                "this k-mer set was built with BBK_UNSORTED: it can be owner-partitioned, expanded or re-merged, "
                "not exported in key order");
    const size_t rec = (size_t)s->W * 8;
    if (h_counts && pd) memset(h_counts, 0, pd->nb * sizeof(uint64_t));
    if (s->n == 0) return;
    const bool wc = s->has_counts && dst_counts;
    if (s->ref_order && !pd) {
        // ascending export of a set stored in the final_kmers order: sort a copy (not a hot path)
        LsdSort t(ctx, s->k, s->n, wc);
        t.load(s->keys.p, s->counts.as<uint32_t>());
        t.sort();
        BBK_HIP(bbk::copy_async(dst_keys, t.keys.p, s->n * rec, hipMemcpyDefault, ctx->stream));
        if (wc) BBK_HIP(bbk::copy_async(dst_counts, t.vals.p, s->n * 4, hipMemcpyDefault, ctx->stream));
        stream_wait(ctx);
        return;
    }
    if (!pd || (s->ref_order && pd->kind == 1 && pd->nb == 16)) {  // stored in the requested order: plain copy
        BBK_HIP(bbk::copy_async(dst_keys, s->keys.p, s->n * rec, hipMemcpyDefault, ctx->stream));
        if (wc) BBK_HIP(bbk::copy_async(dst_counts, s->counts.p, s->n * 4, hipMemcpyDefault, ctx->stream));
        stream_wait(ctx);
        return;
    }
    // One stable pass on the bucket digit keeps the ascending order inside each bucket.  It reads the set
    // and writes straight into the caller's buffer when that is device memory (no staging copies).
    const bool kdev = is_device_ptr(dst_keys), cdev = !wc || is_device_ptr(dst_counts);
    DevBuf tk, tc;
    if (!kdev) tk.alloc(s->n * rec);
    if (wc && !cdev) tc.alloc(s->n * 4);
    void *ok = kdev ? dst_keys : tk.p;
    uint32_t *oc = wc ? (cdev ? (uint32_t *)dst_counts : tc.as<uint32_t>()) : nullptr;
    uint64_t hc[256];  // the pass counts the digit values anyway: the per-owner counts come for free
    partition_records(ctx, (int)s->W, s->keys.p, ok, wc ? s->counts.as<uint32_t>() : nullptr, oc, s->n, *pd,
                      h_counts ? hc : nullptr);
    if (h_counts)
        for (unsigned i = 0; i < pd->nb; ++i) h_counts[i] = hc[i];
    if (!kdev) BBK_HIP(hipMemcpyAsync(dst_keys, tk.p, s->n * rec, hipMemcpyDeviceToHost, ctx->stream));
    if (wc && !cdev) BBK_HIP(hipMemcpyAsync(dst_counts, tc.p, s->n * 4, hipMemcpyDeviceToHost, ctx->stream));
    stream_wait(ctx);
}

int bbk_kmerset_export(bbk_ctx *ctx, const bbk_kmerset *s, unsigned order, void *dst_keys, void *dst_counts) {
    return guarded([&] {
        BBK_REQUIRE(ctx && s && (s->n == 0 || dst_keys), BBK_ERR_ARG, "bbk_kmerset_export: NULL argument");
        BBK_REQUIRE(order == BBK_ORDER_SORTED || order == BBK_ORDER_REFERENCE_BUCKETS16, BBK_ERR_ARG,
                    "bbk_kmerset_export: unknown order %u", order);
        if (order == BBK_ORDER_SORTED) {
            export_ordered(ctx, s, nullptr, dst_keys, dst_counts, nullptr);
        } else {
            const PassDesc pd = ref_bucket_pass();
            export_ordered(ctx, s, &pd, dst_keys, dst_counts, nullptr);
        }
    });
}

int bbk_kmerset_export_by_owner(bbk_ctx *ctx, const bbk_kmerset *s, unsigned nranks, void *dst_keys,
                                void *dst_counts, uint64_t *h_counts) {
    return guarded([&] {
        BBK_REQUIRE(ctx && s && h_counts && (s->n == 0 || dst_keys), BBK_ERR_ARG,
                    "bbk_kmerset_export_by_owner: NULL argument");
        BBK_REQUIRE(nranks >= 1 && nranks <= 256, BBK_ERR_ARG, "bbk_kmerset_export_by_owner: nranks %u not in [1,256]",
                    nranks);
        const PassDesc pd{2, 0, 0, 8, nranks};
        export_ordered(ctx, s, &pd, dst_keys, dst_counts, h_counts);
    });
}

void bbk_kmerset_free(bbk_kmerset *s) { delete s; }

int bbk_kmerset_verify_order(bbk_ctx *ctx, const bbk_kmerset *s, uint64_t *n_runs, uint64_t *n_equal,
                             uint64_t *h_run_starts, unsigned cap) {
    return guarded([&] {
        BBK_REQUIRE(ctx && s && n_runs && n_equal, BBK_ERR_ARG, "bbk_kmerset_verify_order: NULL argument");
        BBK_HIP(hipSetDevice(ctx->device));
        *n_runs = s->n ? 1 : 0;
        *n_equal = 0;
        if (h_run_starts && cap) h_run_starts[0] = 0;
        if (s->n < 2) return;
        DevBuf d(8 * 40);
        BBK_HIP(hipMemsetAsync(d.p, 0, 8 * 40, ctx->stream));
        dispatch_w(s->W, [&](auto w) {
            constexpr int W_ = decltype(w)::value;
            launch_items(ctx, "k_order_check", k_order_check<W_>, s->n, (const Key<W_> *)s->keys.p, s->n,
                         (unsigned long long *)d.p);
        });
        unsigned long long h[40];
        BBK_HIP(hipMemcpyAsync(h, d.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
        stream_wait(ctx);
        *n_runs = 1 + h[0];
        *n_equal = h[1];
        if (h_run_starts) {
            const unsigned got = (unsigned)std::min<unsigned long long>(h[0], 32ull);
            std::sort(h + 2, h + 2 + got);
            for (unsigned i = 0; i < got && i + 1 < cap; ++i) h_run_starts[i + 1] = h[2 + i] + 1;
        }
    });
}

int bbk_kmerset_bucket_offsets(bbk_ctx *ctx, const bbk_kmerset *s, uint64_t *h_offsets) {
    return guarded([&] {
        BBK_REQUIRE(ctx && s && h_offsets, BBK_ERR_ARG, "bbk_kmerset_bucket_offsets: NULL argument");
        BBK_REQUIRE(s->ref_order, BBK_ERR_ARG, "bbk_kmerset_bucket_offsets: the set is not in the final_kmers order");
        BBK_HIP(hipSetDevice(ctx->device));
        if (s->n == 0) {
            for (int b = 0; b <= 16; ++b) h_offsets[b] = 0;
            return;
        }
        DevBuf d(17 * 8);
        dispatch_w(s->W, [&](auto w) {
            constexpr int W_ = decltype(w)::value;
            hipLaunchKernelGGL(k_bucket_bounds<W_>, dim3(1), dim3(64), 0, ctx->stream, (const Key<W_> *)s->keys.p, s->n,
                               (unsigned long long *)d.p);
        });
        check_launch("k_bucket_bounds");
        unsigned long long h[17];
        BBK_HIP(hipMemcpyAsync(h, d.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
        stream_wait(ctx);
        for (int b = 0; b <= 16; ++b) h_offsets[b] = h[b];
    });
}

int bbk_kmerset_get(bbk_ctx *ctx, const bbk_kmerset *s, uint64_t first, uint64_t count, void *h_keys, void *h_counts) {
    return guarded([&] {
        BBK_REQUIRE(ctx && s && (count == 0 || h_keys), BBK_ERR_ARG, "bbk_kmerset_get: NULL argument");
        BBK_REQUIRE(first <= s->n && count <= s->n - first, BBK_ERR_ARG, "bbk_kmerset_get: range [%llu, +%llu) outside the set",
                    (unsigned long long)first, (unsigned long long)count);
        BBK_HIP(hipSetDevice(ctx->device));
        if (!count) return;
        const size_t rec = (size_t)s->W * 8;
        BBK_HIP(hipMemcpyAsync(h_keys, s->keys.as<char>() + first * rec, count * rec, hipMemcpyDeviceToHost, ctx->stream));
        if (h_counts && s->has_counts)
            BBK_HIP(hipMemcpyAsync(h_counts, s->counts.as<uint32_t>() + first, count * 4, hipMemcpyDeviceToHost,
                                   ctx->stream));
        stream_wait(ctx);
    });
}

int bbk_kmerset_write_final_kmers(bbk_ctx *ctx, const bbk_kmerset *s, const char *path) {
    return guarded([&] {
        BBK_REQUIRE(ctx && s && path, BBK_ERR_ARG, "bbk_kmerset_write_final_kmers: NULL argument");
        BBK_HIP(hipSetDevice(ctx->device));
        const size_t rec = (size_t)s->W * 8;
        // the records in the final_kmers order on the device (the set itself when it was built in that order),
        // then device -> file through the pinned staging buffers: no host copy of the whole set
        DevBuf tmp;
        const void *src = s->keys.p;
        if (!s->ref_order && s->n) {
            tmp.alloc(s->n * rec);
            const PassDesc pd = ref_bucket_pass();
            export_ordered(ctx, s, &pd, tmp.p, nullptr, nullptr);
            src = tmp.p;
        }
        const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
        BBK_REQUIRE(fd >= 0, BBK_ERR_IO, "cannot open %s for writing", path);
        bool ok = false;
        try {
            ok = d2f_big(ctx, fd, 0, src, s->n * rec);
        } catch (...) {  // a HIP error inside the stream: no descriptor and no full-size, half-written file is left behind
            (void)close(fd);
            (void)unlink(path);
            throw;
        }
        const int cl = close(fd);
        if (!(ok && cl == 0)) (void)unlink(path);
        BBK_REQUIRE(ok && cl == 0, BBK_ERR_IO, "short write to %s", path);
    });
}

}  // extern "C"
