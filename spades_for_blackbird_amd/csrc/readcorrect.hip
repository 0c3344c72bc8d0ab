// readcorrect.hip -- BayesHammer's ReadCorrector: corrected reads from the solid k-mers.
//
// Replaces ReadCorrector::CorrectOneRead / CorrectReadRight (projects/hammer/read_corrector.cpp:49-245) and the batch loop
// around them (projects/hammer/hammer_tools.cpp:79-105).  The reference is deterministic per read, so the result is
// EQUAL to it: every corrected base, every result flag, every counter -- and that includes the order in which
// std::priority_queue pops states of equal (penalty, pos), which is libstdc++'s __push_heap / __adjust_heap.
// Kernels:
//   k_rc_island   one wavefront per read, lanes over the generator's valid starts (the corrector table of the prepared
//                 batch, hreads.hip) in chunks of 64: one table_find<1> and one good byte per start, the good starts of a
//                 chunk as one 64-bit ballot, the longest run of consecutive good starts over those masks with the run
//                 carried from chunk to chunk (the earliest run wins a tie: strict >, :185).  Writes the island and the
//                 result flag of the reads that need no search, and appends (read, direction) work items for the others.
//   k_rc_search   one wavefront per work item: CorrectReadRight as a best-first search whose queue is a binary heap in LDS
//                 that follows __push_heap / __adjust_heap step for step (so does the four-slot candidates heap).  A state
//                 is (last k-mer u64, cpos 4 x u16, pos u16, penalty i16, edit-log node); the corrected string is never
//                 copied: an edit is a node (prev, pos, base) of a parent-linked log and the winner's chain is replayed
//                 onto the output read.  Lane 0 owns the heaps; lanes 0..3 do the up to four lookups of a step.  The left
//                 direction addresses the read reversed and complemented.
// Capacity rule (deterministic, the same for any batching): a search goes to the host rule (readcorrect_host.hpp, OpenMP)
// exactly when `corrections` would hold more than kRcHeapCap states after a flush, when it pops more than kRcPopCap times,
// or when its edit log fills (kRcEditCap = 3 * kRcPopCap nodes: a pop makes three at most, so the pop cap always comes
// first).  Both paths give the same bytes.
// One path (rc_correct) serves every entry, and it runs on a prepared batch (bbk_hreads, hreads.hip): the bases, the
// qualities and the generator's stretches are the resident ones, and the outcome stays resident as well (bbk_corrected: what
// readprint.hip prints).  bbk_corrector_correct_resident is that path; bbk_corrector_correct_prepared is it followed by
// bbk_corrected_export; bbk_corrector_correct, which takes host arrays that are trimmed already, prepares them with
// BBK_NO_TRIM first -- an upload and two k_hr_prepare launches where it used to cut the stretches on the host -- and exports
// into the caller's layout.  The steps: rc_device_pass (island, search), rc_host_tail (the searches beyond the capacities,
// their spans copied back), rc_uncorrected; changed reads and bases are k_rp_outcome's per-read counts.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <memory>

#include "hammer.h"
#include "kmer_ops.h"
#include "readcorrect_host.hpp"

namespace bbk {

constexpr uint32_t kRcHeapCap = 32;
constexpr uint32_t kRcPopCap = 1024;
constexpr uint32_t kRcEditCap = 3 * kRcPopCap;  // node indices fit 12 bits; 0xFFF is "no node"
constexpr uint32_t kRcNoNode = 0xFFFu;
constexpr uint32_t kRcMaxRead = 65535;  // positions are uint16_t in the reference's cpos and in a state here
static_assert(kRcEditCap <= kRcNoNode, "an edit-log node index must fit 12 bits");
static_assert(5 * kRcPopCap < 0x8000, "a penalty must fit 16 bits: a pop costs 5 at most");

enum : uint8_t { kRcNone = 0, kRcDone = 1, kRcFailed = 2, kRcOverflow = 3 };  // what a search came to

// A, C, G, T -> 0..3, anything else 4
__device__ inline uint32_t rc_code(uint8_t c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; }

// ---- k_rc_island --------------------------------------------------------------------------------------------------
// the longest run of good starts seen so far
struct RcRun {
    uint32_t run = 0, run_start = 0, best = 0, best_start = 0;
    // mask: the good starts of m consecutive starts from `first` (bits m.. are 0)
    __device__ void take(uint64_t mask, uint32_t m, uint32_t first) {
        uint32_t p = 0;
        while (p < m) {
            const uint64_t rest = mask >> p;
            if (rest & 1ull) {
                const uint64_t inv = ~rest;
                uint32_t ones = inv ? (uint32_t)__builtin_ctzll(inv) : 64u;
                if (ones > m - p) ones = m - p;
                if (run == 0) run_start = first + p;
                run += ones;
                p += ones;
                if (run > best) {  // strict: the earliest of equal runs stays
                    best = run;
                    best_start = run_start;
                }
            } else {
                uint32_t zeros = rest ? (uint32_t)__builtin_ctzll(rest) : 64u;
                if (zeros > m - p) zeros = m - p;
                run = 0;
                p += zeros;
            }
        }
    }
};

// isl: per read (first start of the longest run, its number of starts); items: read << 1 | direction (0 right, 1 left)
__global__ __launch_bounds__(256) void k_rc_island(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ off,
                                                  uint64_t n_reads, int k, const uint32_t *__restrict__ stretches,
                                                  const uint64_t *__restrict__ st_off, const Key<1> *__restrict__ keys,
                                                  PrefixTable P, const uint8_t *__restrict__ good,
                                                  uint32_t *__restrict__ isl, uint8_t *__restrict__ result,
                                                  unsigned long long *__restrict__ n_items, uint64_t *__restrict__ items) {
    const uint64_t r = (BBK_GID()) >> 6;
    if (r >= n_reads) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t base = off[r];
    const uint32_t size = (uint32_t)(off[r + 1] - base);
    RcRun st;
    for (uint64_t s = st_off[r]; s < st_off[r + 1]; ++s) {
        const uint32_t start = stretches[2 * s], length = stretches[2 * s + 1];
        const uint32_t nk = length >= (uint32_t)k ? length - (uint32_t)k + 1u : 0u;
        st.run = 0;  // two stretches are never adjacent: a start between them is not valid
        for (uint32_t c = 0; c < nk; c += 64u) {
            const uint32_t m = nk - c < 64u ? nk - c : 64u;
            const uint32_t p = start + c + lane;
            bool g = false;
            if (lane < m && p + (uint32_t)k <= size) {
                uint64_t key = 0;
                for (int i = 0; i < k; ++i) key |= (uint64_t)(rc_code(bases[base + p + i]) & 3u) << (2 * i);
                Key<1> q;
                q.w[0] = key;
                const uint64_t i = table_find<1>(keys, P, q);
                g = i != kNotFound && good[i] != 0;
            }
            st.take(__ballot(g), m, start + c);
        }
    }
    if (lane != 0) return;
    isl[2 * r] = st.best_start;
    isl[2 * r + 1] = st.best;
    const uint32_t solid_len = st.best ? st.best + (uint32_t)k - 1u : 0u;
    const bool search = solid_len != 0 && solid_len != size;  // :202
    result[r] = search || (size >= (uint32_t)k && solid_len == size) ? 1 : 0;
    if (!search) return;
    const uint32_t lright = st.best_start + solid_len - 1u;
    const uint32_t n = (lright + 1u < size ? 1u : 0u) + (st.best_start > 0 ? 1u : 0u);  // a search from the last base ends
    const unsigned long long at = atomicAdd(n_items, (unsigned long long)n);            // with its first pop
    uint32_t j = 0;
    if (lright + 1u < size) items[at + j++] = r << 1;
    if (st.best_start > 0) items[at + j] = (r << 1) | 1ull;
}

// ---- k_rc_search --------------------------------------------------------------------------------------------------
// A heap of states in LDS, one array per field.  `key` orders them: (penalty + 0x8000) << 16 | pos, so std::less<state>
// (:41-46: penalty, then pos) is < on the key.  node: the edit-log node of the state's string in bits 0..11; a candidate
// also carries the base it would write in bits 16..18 (4: none).
struct RcHeap {
    uint64_t *last, *cpos;
    uint32_t *key, *node;
    __device__ void move(uint32_t to, uint32_t from) const {
        last[to] = last[from];
        cpos[to] = cpos[from];
        key[to] = key[from];
        node[to] = node[from];
    }
    __device__ void set(uint32_t at, uint64_t l, uint64_t c, uint32_t ky, uint32_t nd) const {
        last[at] = l;
        cpos[at] = c;
        key[at] = ky;
        node[at] = nd;
    }
    // std::__push_heap(first, hole, top = 0, value, less)
    __device__ void push_heap(uint32_t hole, uint32_t top, uint64_t l, uint64_t c, uint32_t ky, uint32_t nd) const {
        while (hole > top) {
            const uint32_t parent = (hole - 1u) / 2u;
            if (!(key[parent] < ky)) break;
            move(hole, parent);
            hole = parent;
        }
        set(hole, l, c, ky, nd);
    }
    // std::__adjust_heap(first, hole = 0, len, value, less)
    __device__ void adjust_heap(uint32_t len, uint64_t l, uint64_t c, uint32_t ky, uint32_t nd) const {
        uint32_t hole = 0, second = 0;
        while ((int)second < ((int)len - 1) / 2) {
            second = 2u * (second + 1u);
            if (key[second] < key[second - 1u]) --second;
            move(hole, second);
            hole = second;
        }
        if ((len & 1u) == 0 && (int)second == ((int)len - 2) / 2) {
            second = 2u * (second + 1u);
            move(hole, second - 1u);
            hole = second - 1u;
        }
        push_heap(hole, 0, l, c, ky, nd);
    }
    // priority_queue::pop of a queue of `size` elements (the top has been read): pop_heap + pop_back
    __device__ void pop(uint32_t size) const {
        if (size > 1) adjust_heap(size - 1u, last[size - 1u], cpos[size - 1u], key[size - 1u], node[size - 1u]);
    }
};

__device__ inline uint32_t rc_key(int penalty, uint32_t pos) { return ((uint32_t)(penalty + 0x8000) << 16) | pos; }

// size_thr: CorrectReadRight's size_t(100 * log2(n)) + 1 for every n up to the longest read, computed by the host
__global__ __launch_bounds__(64) void k_rc_search(const uint8_t *__restrict__ bases, const uint8_t *__restrict__ quals,
                                                 const uint64_t *__restrict__ off, int k, const Key<1> *__restrict__ keys,
                                                 PrefixTable P, const uint8_t *__restrict__ good,
                                                 const uint32_t *__restrict__ isl, const uint64_t *__restrict__ items,
                                                 uint64_t n_items, const uint32_t *__restrict__ size_thr,
                                                 uint8_t *__restrict__ out, uint8_t *__restrict__ sstat) {
    __shared__ uint64_t h_last[kRcHeapCap], h_cpos[kRcHeapCap], c_last[4], c_cpos[4];
    __shared__ uint32_t h_key[kRcHeapCap], h_node[kRcHeapCap], c_key[4], c_node[4];
    __shared__ uint32_t elog[kRcEditCap];
    const uint64_t w = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (w >= n_items) return;
    const uint32_t lane = threadIdx.x;
    const uint64_t r = items[w] >> 1;
    const bool left = (items[w] & 1ull) != 0;
    const uint64_t base = off[r];
    const uint32_t size = (uint32_t)(off[r + 1] - base);
    const uint32_t lleft = isl[2 * r];
    const uint32_t lright = lleft + (uint32_t)k - 1u + isl[2 * r + 1] - 1u;
    // the right search runs on the read from lright, the left one on its reverse complement from size - 1 - lleft (:206-208)
    const uint32_t right_pos = left ? size - 1u - lleft : lright;
    if (right_pos + 1u >= size || right_pos + 1u < (uint32_t)k) return;  // never appended
    const int n = (int)(size - right_pos);
    const uint32_t thr = size_thr[n];
    const RcHeap H{h_last, h_cpos, h_key, h_node}, C{c_last, c_cpos, c_key, c_node};
    const int top_shift = 2 * (k - 1);
    // position p of the string the search runs on: its base code (4: not a nucleotide) and its quality
    auto at = [&](uint32_t p) { return base + (left ? size - 1u - p : p); };
    auto code_at = [&](uint32_t p) {
        const uint32_t d = rc_code(bases[at(p)]);
        return left && d < 4u ? 3u - d : d;
    };

    uint32_t hsize = 0, nlog = 0, pops = 0;  // lane 0's
    if (lane == 0) {
        uint64_t last = 0;  // KMer(seq, right_pos - K + 1, K): the island's last k-mer, all nucleotides
        for (int i = 0; i < k; ++i) last |= (uint64_t)(code_at(right_pos - (uint32_t)k + 1u + (uint32_t)i) & 3u) << (2 * i);
        H.set(0, last, ~0ull, rc_key(0, right_pos), kRcNoNode);
        hsize = 1;
    }
    uint32_t st = kRcNone, winner = kRcNoNode;
    for (;;) {
        uint64_t cl = 0, cc = 0;
        uint32_t ck = 0, cn = 0;
        if (lane == 0) {
            if (hsize == 0) {
                st = kRcFailed;
            } else if (++pops > kRcPopCap) {
                st = kRcOverflow;
            } else {  // state correction = corrections.top(); corrections.pop();
                cl = h_last[0];
                cc = h_cpos[0];
                ck = h_key[0];
                cn = h_node[0];
                H.pop(hsize);
                --hsize;
            }
        }
        st = __shfl(st, 0, 64);
        if (st != kRcNone) break;
        cl = __shfl(cl, 0, 64);
        ck = __shfl(ck, 0, 64);
        const uint32_t pos = (ck & 0xFFFFu) + 1u;
        if (pos == size) {  // return correction.str
            st = kRcDone;
            winner = cn;
            break;
        }
        const uint32_t d = code_at(pos);
        const int q = quals[at(pos)];
        // lane c: correction.last << c
        bool found = false, gd = false;
        if (lane < 4) {
            Key<1> x;
            x.w[0] = (cl >> 2) | ((uint64_t)lane << top_shift);
            const uint64_t i = table_find<1>(keys, P, x);
            found = i != kNotFound;
            gd = found && good[i] != 0;
        }
        const uint32_t fm = (uint32_t)__ballot(found) & 15u, gm = (uint32_t)__ballot(gd) & 15u;
        if (lane == 0) {
            const int pen = (int)(ck >> 16) - 0x8000;
            const bool is_n = d < 4u;
            uint32_t ncand = 0;
            bool extended = false;
            if (is_n) {  // the own nucleotide: the OUTER cpos, all 0xFFFF (:70,98,104)
                const bool f = (fm >> d) & 1u, g = (gm >> d) & 1u;
                const int cost = f ? (g ? 0 : (q >= 20 ? 1 : 2)) : (q >= 20 ? 2 : 3);
                C.push_heap(ncand++, 0, (cl >> 2) | ((uint64_t)d << top_shift), ~0ull, rc_key(pen - cost, pos), cn | (4u << 16));
                extended = g && q >= 20;
            }
            // :109-125: extended, too many corrections, clustered corrections (size_t minus uint16_t: 0xFFFF wraps)
            if (!extended && !(100 * pen < -15 * n) && !((uint64_t)pos - (cc & 0xFFFFull) < 8ull)) {
                const uint64_t ncpos = (cc >> 16) | ((uint64_t)pos << 48);
                const int cost = is_n ? (q >= 20 ? 5 : 1) : 0;
                for (uint32_t c4 = 0; c4 < 4u; ++c4) {
                    if (c4 == d || !((gm >> c4) & 1u)) continue;
                    C.push_heap(ncand++, 0, (cl >> 2) | ((uint64_t)c4 << top_shift), ncpos, rc_key(pen - cost, pos), cn | (c4 << 16));
                }
            }
            // FlushCandidates (:49-64)
            const bool top_only = hsize > thr;
            while (ncand != 0 && st == kRcNone) {
                const uint64_t l = c_last[0], c = c_cpos[0];
                const uint32_t ky = c_key[0];
                uint32_t nd = c_node[0] & 0xFFFu;
                const uint32_t b = c_node[0] >> 16;
                if (hsize == kRcHeapCap || (b < 4u && nlog == kRcEditCap)) {
                    st = kRcOverflow;
                    break;
                }
                if (b < 4u) {  // corrected[pos] = ncc
                    elog[nlog] = nd | (b << 12) | (pos << 16);
                    nd = nlog++;
                }
                H.push_heap(hsize, 0, l, c, ky, nd);
                ++hsize;
                if (top_only) break;
                C.pop(ncand);
                --ncand;
            }
        }
        st = __shfl(st, 0, 64);
        if (st != kRcNone) break;
    }
    if (lane != 0) return;
    if (st == kRcDone) {
        while (winner != kRcNoNode) {
            const uint32_t e = elog[winner];
            const uint32_t b = (e >> 12) & 3u;
            out[at(e >> 16)] = (uint8_t)((0x54474341u >> (8u * (left ? 3u - b : b))) & 0xFFu);  // "ACGT"
            winner = e & 0xFFFu;
        }
    }
    sstat[2 * r + (left ? 1 : 0)] = (uint8_t)st;
}

}  // namespace bbk

struct bbk_corrector {
    bbk_ctx *ctx = nullptr;
    const bbk_kmerset *set = nullptr;  // must outlive the corrector
    unsigned k = 0;
    uint64_t n = 0;
    bbk::PrefixIndex prefix;
    bbk::DevBuf good;  // n u8
    uint64_t stats[5] = {0, 0, 0, 0, 0};
    // the host rule's copy of the set, fetched when a search first needs it
    bbk::raw_vector<uint64_t> h_keys;
    bbk::raw_vector<uint8_t> h_good;
    bool on_host = false;
};

namespace bbk {

static std::unique_ptr<bbk_corrector> rc_new(const char *fn, bbk_ctx *ctx, const bbk_kmerset *set) {
    BBK_REQUIRE(!(set->flags & BBK_CANONICAL), BBK_ERR_ARG,
                "%s: needs a both-strand k-mer set (bbk_count(BBK_BOTH_STRANDS)): this one is canonical only (BBK_CANONICAL)", fn);
    require_hammer_set(fn, set);
    BBK_HIP(hipSetDevice(ctx->device));
    auto c = std::make_unique<bbk_corrector>();
    c->ctx = ctx;
    c->set = set;
    c->k = set->k;
    c->n = set->n;
    c->good.alloc(c->n);
    if (c->n) c->prefix.build(ctx, set->keys.as<uint64_t>(), 1, set->k, set->n);
    return c;
}

static void rc_fetch_set(bbk_corrector *c) {
    if (c->on_host) return;
    c->h_keys.resize(c->n);
    c->h_good.resize(c->n);
    if (c->n) {
        d2h_big(c->ctx, c->h_keys.data(), c->set->keys.p, c->n * 8);
        d2h_big(c->ctx, c->h_good.data(), c->good.p, c->n);
    }
    c->on_host = true;
}

}  // namespace bbk

using namespace bbk;
namespace rch = bbkhost::readcorrect;

static void rc_check(const char *fn, const bbk_corrector *c, const bbk_hreads *hr) {
    BBK_REQUIRE(hr->k == c->k, BBK_ERR_ARG, "%s: the batch was prepared for k = %u, the corrector's set has k = %u", fn, hr->k, c->k);
    BBK_REQUIRE(hr->ctx == c->ctx, BBK_ERR_ARG, "%s: the batch belongs to another context", fn);
    BBK_REQUIRE(hr->longest <= kRcMaxRead, BBK_ERR_ARG,
                "%s: a record has %llu bases: a position is 16 bits (read_corrector.cpp:20), %u at most", fn,
                (unsigned long long)hr->longest, kRcMaxRead);
}

// What the device pass leaves on the host for the tail and the counter
struct RcPass {
    uint64_t n_items = 0;       // searches: none -> the reads stay as they are, and nothing below is filled
    bool host_only = false;     // BBK_CORRECTOR_HOST: no search ran on the device
    raw_vector<uint32_t> isl;   // n_reads x (first start, starts) of the longest run
    raw_vector<uint8_t> sstat;  // n_reads x (right, left): what the search came to
};

// k_rc_island over the batch's corrector table, then k_rc_search for every work item: cr->res, and the searched spans of
// cr->out (a copy of the trimmed reads so far)
static void rc_device_pass(bbk_corrector *c, const bbk_hreads *hr, uint32_t longest, bbk_corrected *cr, RcPass &P) {
    bbk_ctx *ctx = c->ctx;
    const unsigned k = c->k;
    const uint64_t n_reads = hr->n;
    const bbk_hreads::Trimmed &t = hreads_trimmed(hr);
    raw_vector<uint32_t> thr(longest + 1);
    thr[0] = 0;
    for (uint32_t n = 1; n <= longest; ++n) thr[n] = (uint32_t)rch::size_threshold(n);  // the same log2 as the host rule
    DevBuf d_thr, d_isl(n_reads * 8), d_items(n_reads * 16), d_count(8), d_sstat(n_reads * 2);
    upload(ctx, d_thr, thr.data(), (uint64_t)thr.size());
    BBK_HIP(hipMemsetAsync(d_count.p, 0, 8, ctx->stream));
    BBK_HIP(hipMemsetAsync(d_sstat.p, 0, n_reads * 2, ctx->stream));
    launch_items_timed(ctx, "k_rc_island", k_rc_island, n_reads * 64, t.bases, t.off, n_reads, (int)k, hr->cst.as<uint32_t>(),
                       hr->coff.as<uint64_t>(), c->set->keys.as<Key<1>>(), c->prefix.table(), c->good.as<uint8_t>(),
                       d_isl.as<uint32_t>(), cr->res.as<uint8_t>(), d_count.as<unsigned long long>(), d_items.as<uint64_t>());
    d2h_sync(ctx, &P.n_items, d_count.p, 8);
    BBK_REQUIRE(P.n_items <= 2 * n_reads, BBK_ERR_INTERNAL, "bbk_corrector_correct: %llu work items for %llu reads",
                (unsigned long long)P.n_items, (unsigned long long)n_reads);
    const char *env = getenv("BBK_CORRECTOR_HOST");
    P.host_only = env && atoi(env) != 0;
    if (!P.n_items) return;
    if (!P.host_only) {
        KernelTimer timer(ctx, "k_rc_search");
        hipLaunchKernelGGL(k_rc_search, grid_blocks(P.n_items), dim3(64), 0, ctx->stream, t.bases, t.quals, t.off, (int)k,
                           c->set->keys.as<Key<1>>(), c->prefix.table(), c->good.as<uint8_t>(), d_isl.as<uint32_t>(),
                           d_items.as<uint64_t>(), P.n_items, d_thr.as<uint32_t>(), cr->out.as<uint8_t>(), d_sstat.as<uint8_t>());
        check_launch("k_rc_search");
    }
    P.isl.resize(n_reads * 2);
    P.sstat.resize(n_reads * 2);
    d2h_big(ctx, P.isl.data(), d_isl.p, n_reads * 8);
    d2h_big(ctx, P.sstat.data(), d_sstat.p, n_reads * 2);
}

// The searches the device did not finish, by the host rule (readcorrect_host.hpp, OpenMP): their spans are copied back
// into cr->out, and only those; the trimmed bases and qualities come to the host only when there is such a search.  Fills
// `where` (n_reads, zeroed) and returns the number of those searches.
static uint64_t rc_host_tail(bbk_corrector *c, const bbk_hreads *hr, const uint64_t *h_off, RcPass &P, bbk_corrected *cr,
                             uint8_t *where) {
    bbk_ctx *ctx = c->ctx;
    const unsigned k = c->k;
    raw_vector<uint64_t> todo;  // read << 1 | direction
    for (uint64_t r = 0; r < hr->n; ++r) {
        const uint64_t len = h_off[r + 1] - h_off[r];
        const uint32_t run = P.isl[2 * r + 1], solid = run ? run + k - 1 : 0;
        if (!solid || solid == len) continue;
        const uint32_t lleft = P.isl[2 * r], lright = lleft + solid - 1;
        const size_t before = todo.size();
        if (lright + 1 < len && (P.host_only || P.sstat[2 * r] == kRcOverflow)) todo.push_back(r << 1);
        if (lleft > 0 && (P.host_only || P.sstat[2 * r + 1] == kRcOverflow)) todo.push_back((r << 1) | 1);
        where[r] = todo.size() != before ? 2 : 1;
    }
    if (todo.empty()) return 0;
    rc_fetch_set(c);
    const bbk_hreads::Trimmed &t = hreads_trimmed(hr);
    raw_vector<char> h_bases(t.total), h_qual(t.total);
    d2h_big(ctx, h_bases.data(), t.bases, t.total);
    d2h_big(ctx, h_qual.data(), t.quals, t.total);
    const uint64_t *hk = c->h_keys.data();
    const uint8_t *hg = c->h_good.data();
    const uint64_t hn = c->n;
    auto lookup = [hk, hn](uint64_t key) -> uint64_t {
        const uint64_t *it = std::lower_bound(hk, hk + hn, key);
        return it != hk + hn && *it == key ? (uint64_t)(it - hk) : rch::kNone;
    };
    std::vector<std::string> span(todo.size());  // what a search made of the bases it may touch
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t j = 0; j < (int64_t)todo.size(); ++j) {
        const uint64_t r = todo[j] >> 1, o = h_off[r], len = h_off[r + 1] - o;
        const bool left = todo[j] & 1;
        const uint32_t lleft = P.isl[2 * r], lright = lleft + P.isl[2 * r + 1] + k - 2;
        const std::string seq(h_bases.data() + o, len), qual(h_qual.data() + o, len);
        rch::SearchFigures fig;
        if (!left) {
            const std::string s = rch::CorrectReadRight(seq, qual, lright, k, lookup, hg, &fig);
            span[j] = s.substr(lright + 1);  // it touches nothing else
        } else {
            const std::string s = rch::ReverseComplement(
                rch::CorrectReadRight(rch::ReverseComplement(seq), rch::Reverse(qual), len - 1 - lleft, k, lookup, hg, &fig));
            span[j] = s.substr(0, lleft);
        }
        P.sstat[2 * r + left] = fig.failed ? kRcFailed : kRcDone;
    }
    for (size_t j = 0; j < todo.size(); ++j) {  // back into the device's reads: only the spans those searches own
        const uint64_t r = todo[j] >> 1, o = h_off[r];
        const uint64_t at = (todo[j] & 1) ? o : o + P.isl[2 * r] + P.isl[2 * r + 1] + k - 1;
        if (!span[j].empty())
            BBK_HIP(hipMemcpyAsync(cr->out.as<uint8_t>() + at, span[j].data(), span[j].size(), hipMemcpyHostToDevice, ctx->stream));
    }
    BBK_HIP(hipStreamSynchronize(ctx->stream));  // the spans go now
    return todo.size();
}

// the bases of the searches that failed (read_corrector.cpp:206-208)
static uint64_t rc_uncorrected(unsigned k, uint64_t n_reads, const uint64_t *h_off, const RcPass &P, const uint8_t *where) {
    uint64_t uncorrected = 0;
#pragma omp parallel for reduction(+ : uncorrected)
    for (int64_t r = 0; r < (int64_t)n_reads; ++r) {
        if (!where[r]) continue;
        const uint64_t len = h_off[r + 1] - h_off[r];
        const uint32_t lleft = P.isl[2 * r], lright = lleft + P.isl[2 * r + 1] + k - 2;
        if (P.sstat[2 * r] == kRcFailed) uncorrected += len - lright;
        if (P.sstat[2 * r + 1] == kRcFailed) uncorrected += lleft + 1;  // read_size - (read_size - 1 - lleft)
    }
    return uncorrected;
}

// CorrectReadsBatch over the trimmed reads of a prepared batch, the outcome resident: the one path of every entry (fn)
static std::unique_ptr<bbk_corrected> rc_correct(const char *fn, bbk_corrector *c, const bbk_hreads *hr) {
    rc_check(fn, c, hr);
    bbk_ctx *ctx = c->ctx;
    BBK_HIP(hipSetDevice(ctx->device));
    const uint64_t n_reads = hr->n;
    const unsigned k = c->k;
    const bbk_hreads::Trimmed &t = hreads_trimmed(hr);  // the trimmed reads back to back, made once per batch
    raw_vector<uint64_t> h_off(n_reads + 1);
    d2h_big(ctx, h_off.data(), t.off, (n_reads + 1) * 8);
    uint64_t nucleotides = 0;
    uint32_t longest = 0;
    for (uint64_t r = 0; r < n_reads; ++r) {
        const uint64_t len = h_off[r + 1] - h_off[r];
        if (len >= k) nucleotides += len;  // hammer_tools.cpp:90-95
        longest = std::max(longest, (uint32_t)len);
    }
    auto cr = std::make_unique<bbk_corrected>();
    cr->ctx = ctx;
    cr->hr = hr;
    cr->k = k;
    cr->n = n_reads;
    cr->total = t.total;
    cr->out.alloc(t.total);
    cr->res.alloc(n_reads);
    cr->where.alloc(n_reads);
    cr->changed.alloc(n_reads * 4);
    cr->tag.alloc(n_reads);
    uint64_t before[5];
    memcpy(before, c->stats, sizeof(before));
    c->stats[3] += nucleotides;
    BBK_HIP(copy_async(cr->out.p, t.bases, t.total, hipMemcpyDeviceToDevice, ctx->stream));
    RcPass P;
    if (c->n != 0 && nucleotides != 0) rc_device_pass(c, hr, longest, cr.get(), P);
    else BBK_HIP(hipMemsetAsync(cr->res.p, 0, n_reads, ctx->stream));  // no k-mer is good, or no read has k bases: all false
    raw_vector<uint8_t> where;  // 0 no search, 1 device, 2 host rule
    if (P.n_items) {
        where.assign(n_reads, 0);
        c->stats[4] += rc_host_tail(c, hr, h_off.data(), P, cr.get(), where.data());
        c->stats[2] += rc_uncorrected(k, n_reads, h_off.data(), P, where.data());
        BBK_HIP(hipMemcpyAsync(cr->where.p, where.data(), n_reads, hipMemcpyHostToDevice, ctx->stream));
    } else {
        BBK_HIP(hipMemsetAsync(cr->where.p, 0, n_reads, ctx->stream));
    }
    corrected_outcome(cr.get());
    // changed reads, changed nucleotides (read_corrector.cpp:210-219): four bytes per read come back, not the reads; an
    // unsearched read is a copy and counts 0
    raw_vector<uint32_t> changed(n_reads);
    if (n_reads) d2h_big(ctx, changed.data(), cr->changed.p, n_reads * 4);  // waits: `where` goes after it
    else BBK_HIP(hipStreamSynchronize(ctx->stream));
    for (uint64_t r = 0; r < n_reads; ++r) {
        c->stats[0] += changed[r] != 0;
        c->stats[1] += changed[r];
    }
    for (int i = 0; i < 5; ++i) cr->stats[i] = c->stats[i] - before[i];
    return cr;
}

static void rc_export(bbk_ctx *ctx, const bbk_corrected *cr, char *h_out, uint64_t *h_out_offsets, uint8_t *h_result,
                      uint8_t *h_where, uint32_t *h_changed, uint8_t *h_tag) {
    BBK_HIP(hipSetDevice(ctx->device));
    const uint64_t n = cr->n;
    if (h_out && cr->total) d2h_big(ctx, h_out, cr->out.p, cr->total);
    if (h_out_offsets) d2h_big(ctx, h_out_offsets, hreads_trimmed(cr->hr).off, (n + 1) * 8);
    if (h_result && n) d2h_big(ctx, h_result, cr->res.p, n);
    if (h_where && n) d2h_big(ctx, h_where, cr->where.p, n);
    if (h_changed && n) d2h_big(ctx, h_changed, cr->changed.p, n * 4);
    if (h_tag && n) d2h_big(ctx, h_tag, cr->tag.p, n);
}

extern "C" {

int bbk_corrector_from_expander(bbk_ctx *ctx, const bbk_kmerset *set, const bbk_expander *e, bbk_corrector **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && set && e && out, BBK_ERR_ARG, "bbk_corrector_from_expander: NULL argument");
        BBK_REQUIRE(!e->in_round, BBK_ERR_ARG, "bbk_corrector_from_expander: a round is open: call bbk_expander_round_end first");
        BBK_REQUIRE(e->n == set->n && e->k == set->k, BBK_ERR_ARG,
                    "bbk_corrector_from_expander: the set has %llu k-mers of size %u, the expander was made for %llu of size %u",
                    (unsigned long long)set->n, set->k, (unsigned long long)e->n, e->k);
        auto c = rc_new("bbk_corrector_from_expander", ctx, set);
        if (c->n) {
            BBK_HIP(copy_async(c->good.p, e->cur.p, c->n, hipMemcpyDeviceToDevice, ctx->stream));
            BBK_HIP(hipStreamSynchronize(ctx->stream));
        }
        *out = c.release();
    });
}

int bbk_corrector_from_host(bbk_ctx *ctx, const bbk_kmerset *set, const uint8_t *h_good, bbk_corrector **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && set && out && (h_good || set->n == 0), BBK_ERR_ARG, "bbk_corrector_from_host: NULL argument");
        for (uint64_t i = 0; i < set->n; ++i)
            BBK_REQUIRE(h_good[i] <= 1, BBK_ERR_ARG, "bbk_corrector_from_host: byte %llu is %u: a good bit is 0 or 1",
                        (unsigned long long)i, (unsigned)h_good[i]);
        auto c = rc_new("bbk_corrector_from_host", ctx, set);
        if (c->n) {
            BBK_HIP(hipMemcpyAsync(c->good.p, h_good, c->n, hipMemcpyHostToDevice, ctx->stream));
            BBK_HIP(hipStreamSynchronize(ctx->stream));  // h_good is the caller's
        }
        *out = c.release();
    });
}

void bbk_corrector_limits(unsigned *heap_cap, unsigned *pop_cap) {
    if (heap_cap) *heap_cap = kRcHeapCap;
    if (pop_cap) *pop_cap = kRcPopCap;
}

int bbk_corrector_correct(bbk_corrector *c, const char *h_bases, const uint8_t *h_qual, const uint64_t *h_offsets,
                          uint64_t n_reads, char *h_out, uint8_t *h_result, uint8_t *h_where) {
    return guarded([&] {
        BBK_REQUIRE(c && h_offsets && h_result, BBK_ERR_ARG, "bbk_corrector_correct: NULL argument");
        const uint64_t first = h_offsets[0], total = h_offsets[n_reads];
        BBK_REQUIRE(first <= total && (total == first || (h_bases && h_qual && h_out)), BBK_ERR_ARG,
                    "bbk_corrector_correct: NULL argument");
        const char *fn = "bbk_corrector_correct";
        const auto hr = hreads_from_host(fn, "read", c->ctx, h_bases, h_qual, h_offsets, n_reads, c->k, BBK_NO_TRIM);
        const auto cr = rc_correct(fn, c, hr.get());
        rc_export(c->ctx, cr.get(), h_out ? h_out + first : nullptr, nullptr, h_result, h_where, nullptr, nullptr);
    });
}

int bbk_corrector_correct_resident(bbk_corrector *c, const bbk_hreads *hr, bbk_corrected **out) {
    return guarded([&] {
        BBK_REQUIRE(c && hr && out, BBK_ERR_ARG, "bbk_corrector_correct_resident: NULL argument");
        *out = rc_correct("bbk_corrector_correct_resident", c, hr).release();
    });
}

uint64_t bbk_corrected_size(const bbk_corrected *cr) { return cr ? cr->n : 0; }

int bbk_corrected_export(bbk_ctx *ctx, const bbk_corrected *cr, char *h_out, uint64_t *h_out_offsets, uint8_t *h_result,
                         uint8_t *h_where, uint32_t *h_changed, uint8_t *h_tag) {
    return guarded([&] {
        BBK_REQUIRE(ctx && cr, BBK_ERR_ARG, "bbk_corrected_export: NULL argument");
        rc_export(ctx, cr, h_out, h_out_offsets, h_result, h_where, h_changed, h_tag);
    });
}

void bbk_corrected_free(bbk_corrected *cr) { delete cr; }

int bbk_corrector_correct_prepared(bbk_corrector *c, const bbk_hreads *hr, char *h_out, uint64_t *h_out_offsets,
                                   uint8_t *h_result, uint8_t *h_where) {
    return guarded([&] {
        BBK_REQUIRE(c && hr && h_out_offsets && h_result, BBK_ERR_ARG, "bbk_corrector_correct_prepared: NULL argument");
        rc_check("bbk_corrector_correct_prepared", c, hr);
        BBK_HIP(hipSetDevice(c->ctx->device));
        BBK_REQUIRE(hreads_trimmed(hr).total == 0 || h_out, BBK_ERR_ARG, "bbk_corrector_correct_prepared: NULL argument");
        const auto cr = rc_correct("bbk_corrector_correct_prepared", c, hr);
        rc_export(c->ctx, cr.get(), h_out, h_out_offsets, h_result, h_where, nullptr, nullptr);
    });
}

int bbk_corrector_stats(const bbk_corrector *c, uint64_t stats[5]) {
    return guarded([&] {
        BBK_REQUIRE(c && stats, BBK_ERR_ARG, "bbk_corrector_stats: NULL argument");
        memcpy(stats, c->stats, sizeof(c->stats));
    });
}

void bbk_corrector_free(bbk_corrector *c) { delete c; }

}  // extern "C"
