// hamclust.hip -- Hamming-graph clustering of a both-strand k-mer set, tau = 1.
//
// Replaces TauOneKMerHamClusterer::cluster / ClusterChunk (projects/hammer/hamcluster.cpp:228-289), the first thing
// spades-hammer does with its counted 21-mers (projects/hammer/main.cpp:143-168): every k-mer is united in a
// dsu::ConcurrentDSU (adt/concurrent_dsu.hpp) with each of its 3k single-base substitutions that is in the set, unless
// one of the two sets has been locked (>= 2500 members at the end of a 64 Ki-index chunk).
//
// Here, for k <= 32 (one-word keys, base k-1 most significant in the ascending order):
//   rc index (k_hc_rcidx): rcidx[i] = position of rc(key[i]), one table_find per record; a miss is the closure check.
//   block scan (k_hc_scan): with m = k / 2, the records equal on their top m bases are contiguous (a block).  Two
//     k-mers that differ at one base p < k - m share a block; for p >= k - m their reverse complements differ at
//     k - 1 - p < m <= k - m and share one.  So every pair inside every block is compared, and a pair at distance exactly
//     1 unites (a, b) and (rc a, rc b): every Hamming-1 edge of an rc-closed set is found, without a lookup.  A workgroup
//     stages 256 consecutive records in LDS; every lane compares its record with the later records of its block, tile
//     after tile until the block of the workgroup's last record ends.
//   union-find: u32 parents, hooked inside the scan by compare-and-swap on the root with the larger index (a parent is
//     always below its child, so the root of a tree is its smallest member), then pointer jumping in rounds until a
//     round changes nothing (one flag read per round).
//   sizes, the oversize subset, the listing: a histogram of the labels; the members of components of >= lock_size k-mers
//     are compacted (index, key, rc index) and replayed on the host by the reference's chunked rule -- below lock_size nothing
//     is ever locked and a cluster is its component; the LSD sort groups the indices by label (stable: ascending in a cluster).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "hammer.h"
#include "kmer_ops.h"
#include "select.h"

namespace bbk {

constexpr int kHcTile = 256;
constexpr uint64_t kHcLockSize = 2500;    // hamcluster.cpp:269
constexpr uint64_t kHcChunk = 64 * 1024;  // hamcluster.cpp:281

__device__ inline uint32_t hc_load(const uint32_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

// root of x; on the way every visited node is moved to its grandparent (only ever to an ancestor: atomicMin)
__device__ inline uint32_t hc_find(uint32_t *parent, uint32_t x) {
    uint32_t p = hc_load(&parent[x]);
    while (p != x) {
        const uint32_t g = hc_load(&parent[p]);
        if (g != p) atomicMin(&parent[x], g);
        x = p;
        p = g;
    }
    return x;
}

// the root with the larger index goes under the smaller; a lost race starts again from the two roots
__device__ inline void hc_unite(uint32_t *parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = hc_find(parent, a);
        b = hc_find(parent, b);
        if (a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        if (atomicCAS(&parent[hi], hi, lo) == hi) return;
        a = hi;
        b = lo;
    }
}

__global__ __launch_bounds__(256) void k_hc_rcidx(const Key<1> *__restrict__ keys, uint64_t n, int k, PrefixTable P,
                                                 uint32_t *__restrict__ rcidx, uint32_t *__restrict__ parent,
                                                 uint32_t *__restrict__ status) {
    const uint64_t i = BBK_GID();
    if (i >= n) return;
    uint64_t pos = table_find<1>(keys, P, kmer_rc<1>(key_load<1>(&keys[i]), k));
    if (pos == kNotFound) {
        atomicOr(&status[0], 1u);
        pos = i;
    }
    rcidx[i] = (uint32_t)pos;
    parent[i] = (uint32_t)i;
}

// status[1] receives the length of the longest block
__global__ __launch_bounds__(kHcTile) void k_hc_scan(const uint64_t *__restrict__ keys, uint64_t n, int shift,
                                                    const uint32_t *__restrict__ rcidx, uint32_t *__restrict__ parent,
                                                    uint32_t *__restrict__ status) {
    __shared__ uint64_t tile[kHcTile];
    const uint64_t t0 = (((uint64_t)blockIdx.y * gridDim.x) + blockIdx.x) * kHcTile;
    if (t0 >= n) return;
    const int tid = threadIdx.x;
    const uint64_t gi = t0 + (uint64_t)tid;
    const bool valid = gi < n;
    const uint64_t a = valid ? keys[gi] : 0ull;
    const uint64_t ablk = valid ? a >> shift : ~0ull;
    const uint64_t wmax = (uint64_t)__shfl((unsigned long long)ablk, 63, 64);  // block of the wave's last record
    const uint64_t last = t0 + kHcTile - 1 < n ? t0 + kHcTile - 1 : n - 1;
    const uint64_t lastblk = keys[last] >> shift;
    uint32_t later = 0;  // later records of this lane's block
    for (uint64_t ts = t0;;) {
        const uint64_t gl = ts + (uint64_t)tid;
        tile[tid] = gl < n ? keys[gl] : 0ull;
        const int cnt = n - ts < (uint64_t)kHcTile ? (int)(n - ts) : kHcTile;
        __syncthreads();
        // a later tile holds records of this lane's block only if its first record is one
        const bool mine = valid && (ts == t0 || (tile[0] >> shift) == ablk);
        if (__ballot(mine)) {
            for (int j = ts == t0 ? (tid & ~63) + 1 : 0; j < cnt; ++j) {  // every lane reads tile[j]: a broadcast
                const uint64_t b = tile[j];
                const uint64_t bblk = b >> shift;
                if (bblk > wmax) break;  // ascending: nothing further belongs to a block of this wave
                const uint64_t gj = ts + (uint64_t)j;
                if (mine && gj > gi && bblk == ablk) {
                    ++later;
                    if (kmer_hamdist(a, b) == 1) {
                        hc_unite(parent, (uint32_t)gi, (uint32_t)gj);
                        hc_unite(parent, rcidx[gi], rcidx[gj]);
                    }
                }
            }
        }
        __syncthreads();
        ts += kHcTile;
        if (ts >= n || (keys[ts] >> shift) != lastblk) break;
    }
    if (valid && (gi == 0 || (keys[gi - 1] >> shift) != ablk)) atomicMax(&status[1], later + 1u);
}

__global__ __launch_bounds__(256) void k_hc_jump(uint32_t *__restrict__ parent, uint64_t n, uint32_t *__restrict__ changed) {
    const uint64_t i = BBK_GID();
    if (i >= n) return;
    const uint32_t p = hc_load(&parent[i]);
    uint32_t r = p;
    for (uint32_t q = hc_load(&parent[r]); q != r; q = hc_load(&parent[r])) r = q;
    if (r != p) {
        parent[i] = r;
        atomicOr(changed, 1u);
    }
}

__global__ __launch_bounds__(256) void k_hc_count(const uint32_t *__restrict__ label, uint64_t n, uint32_t *__restrict__ cnt) {
    const uint64_t i = BBK_GID();
    if (i < n) atomicAdd(&cnt[label[i]], 1u);
}

// the members of the components of >= lock_size k-mers (an ordered selection, select.h), with their keys and rc indices
struct HcOversize {
    const uint32_t *__restrict__ label, *__restrict__ cnt;
    uint64_t lock_size;
    __device__ bool operator()(uint64_t i) const { return (uint64_t)cnt[label[i]] >= lock_size; }
};

struct HcStoreMember {
    const uint64_t *__restrict__ keys;
    const uint32_t *__restrict__ rcidx;
    uint32_t *__restrict__ out_idx;
    uint64_t *__restrict__ out_key;
    uint32_t *__restrict__ out_rc;
    __device__ void operator()(uint64_t i, uint64_t rank) const {
        out_idx[rank] = (uint32_t)i;
        out_key[rank] = keys[i];
        out_rc[rank] = rcidx[i];
    }
};

__global__ __launch_bounds__(256) void k_hc_relabel(const uint32_t *__restrict__ idx, const uint32_t *__restrict__ lab,
                                                   uint64_t r, uint32_t *__restrict__ label) {
    const uint64_t j = BBK_GID();
    if (j < r) label[idx[j]] = lab[j];
}

// the roots, and the size of each in their order
struct HcRoot {
    const uint32_t *__restrict__ label;
    __device__ bool operator()(uint64_t i) const { return label[i] == (uint32_t)i; }
};

struct HcStoreSize {
    const uint32_t *__restrict__ cnt;
    uint64_t *__restrict__ sizes;
    __device__ void operator()(uint64_t i, uint64_t rank) const { sizes[rank] = cnt[i]; }
};

__global__ __launch_bounds__(256) void k_hc_pairs(const uint32_t *__restrict__ label, uint64_t n, uint64_t *__restrict__ key,
                                                 uint32_t *__restrict__ val) {
    const uint64_t i = BBK_GID();
    if (i >= n) return;
    key[i] = label[i];
    val[i] = (uint32_t)i;
}

// ---- the host replay of the oversize components (hamcluster.cpp:213-276 over adt/concurrent_dsu.hpp:46-133) ----------
namespace {

enum { HC_UNLOCKED = 0, HC_FULLY_LOCKED = 3 };  // hamcluster.cpp:207-211

struct HostDsu {
    std::vector<uint32_t> parent, size;
    std::vector<uint8_t> aux;
    explicit HostDsu(size_t n) : parent(n), size(n, 1), aux(n, HC_UNLOCKED) {
        for (size_t i = 0; i < n; ++i) parent[i] = (uint32_t)i;
    }
    uint32_t find(uint32_t x) {
        uint32_t r = x;
        while (parent[r] != r) r = parent[r];
        while (parent[x] != r) {
            const uint32_t nx = parent[x];
            parent[x] = r;
            x = nx;
        }
        return r;
    }
    // concurrent_dsu.hpp:46-96: the smaller set goes under the larger, of two equal ones the lower index goes under
    // the higher; the merged root keeps the aux of the set that stays root
    void unite(uint32_t x, uint32_t y) {
        x = find(x);
        y = find(y);
        if (x == y) return;
        if (size[x] > size[y] || (size[x] == size[y] && x > y)) std::swap(x, y);
        parent[x] = y;
        size[y] += size[x];
    }
};

}  // namespace

// idx ascending global indices of the members (so key ascends too), rcg the global index of each reverse complement;
// lab[j] receives the smallest global index of the cluster of member j
static void hc_replay(unsigned k, uint64_t lock_size, uint64_t chunk, const std::vector<uint32_t> &idx,
                      const std::vector<uint64_t> &key, const std::vector<uint32_t> &rcg, std::vector<uint32_t> &lab) {
    const size_t R = idx.size();
    std::vector<uint32_t> lrc(R);
    for (size_t j = 0; j < R; ++j) {
        const auto it = std::lower_bound(idx.begin(), idx.end(), rcg[j]);
        BBK_REQUIRE(it != idx.end() && *it == rcg[j], BBK_ERR_INTERNAL,
                    "hamming clusters: the reverse complement of a replayed k-mer is not replayed");
        lrc[j] = (uint32_t)(it - idx.begin());
    }
    HostDsu uf(R);
    for (size_t j = 0; j < R;) {
        const uint64_t c = idx[j] / chunk;
        size_t e = j;
        while (e < R && idx[e] / chunk == c) ++e;
        for (size_t x = j; x < e; ++x) {
            const uint64_t kmer = key[x];
            if (kmer > key[lrc[x]]) continue;  // one strand of a pair is processed
            for (unsigned p = 0; p < k; ++p) {
                const uint64_t cur = (kmer >> (2 * p)) & 3ull;
                for (uint64_t nc = 0; nc < 4; ++nc) {
                    if (nc == cur) continue;
                    const uint64_t cand = (kmer & ~(3ull << (2 * p))) | (nc << (2 * p));
                    const auto it = std::lower_bound(key.begin(), key.end(), cand);
                    if (it == key.end() || *it != cand) continue;
                    const uint32_t y = (uint32_t)(it - key.begin());
                    if (uf.aux[uf.find((uint32_t)x)] == HC_FULLY_LOCKED || uf.aux[uf.find(y)] == HC_FULLY_LOCKED) continue;
                    uf.unite((uint32_t)x, y);
                    uf.unite(lrc[x], lrc[y]);  // no lock check here (hamcluster.cpp:257-260)
                }
            }
        }
        for (size_t x = j; x < e; ++x) {
            const uint32_t r = uf.find((uint32_t)x);
            if (uf.size[r] >= lock_size) uf.aux[r] = HC_FULLY_LOCKED;
        }
        j = e;
    }
    std::vector<uint32_t> low(R, 0xFFFFFFFFu);
    lab.resize(R);
    for (size_t x = 0; x < R; ++x) {
        const uint32_t r = uf.find((uint32_t)x);
        if (low[r] == 0xFFFFFFFFu) low[r] = idx[x];
        lab[x] = low[r];
    }
}

// ---- the driver: three phases over one state -----------------------------------------------------------------------------
struct HcRun {
    bbk_ctx *ctx;
    const bbk_kmerset *s;
    bbk_hamclusters *h;
    uint64_t n, lock_size, chunk;
    uint32_t *label = nullptr;  // h->labels: the parents of the union-find, in the end the labels
    DevBuf rcidx, status;       // n u32; status: [0] an rc is missing, [1] the longest block, [2] a jump round changed something
    DevBuf cnt;                 // k-mers per label

    // the rc index with the closure refusal, the block scan, pointer jumping until a round changes nothing
    void unite() {
        const unsigned k = s->k;
        const uint64_t *keys = s->keys.as<uint64_t>();
        rcidx.alloc(n * 4);
        status.alloc(16);
        uint32_t *st = status.as<uint32_t>(), missing = 0;
        PrefixIndex prefix;
        prefix.build(ctx, keys, 1, k, n);
        h->labels.alloc(n * 4);
        label = h->labels.as<uint32_t>();
        BBK_HIP(hipMemsetAsync(st, 0, 16, ctx->stream));
        launch_items_timed(ctx, "hc_rcidx", k_hc_rcidx, n, s->keys.as<Key<1>>(), n, (int)k, prefix.table(), rcidx.as<uint32_t>(),
                           label, st);
        BBK_HIP(hipMemcpyAsync(&missing, st, 4, hipMemcpyDeviceToHost, ctx->stream));
        BBK_HIP(hipStreamSynchronize(ctx->stream));
        BBK_REQUIRE(missing == 0, BBK_ERR_ARG,
                    "bbk_kmerset_hamming_clusters: the set is not closed under reverse complement (it must be a BBK_BOTH_STRANDS set)");
        prefix.buf.release();
        {
            const int shift = 2 * (int)(k - k / 2);
            KernelTimer t(ctx, "hc_scan");
            hipLaunchKernelGGL(k_hc_scan, grid_blocks((n + kHcTile - 1) / kHcTile), dim3(kHcTile), 0, ctx->stream, keys, n, shift,
                               rcidx.as<uint32_t>(), label, st);
            check_launch("hc_scan");
        }
        uint64_t rounds = 0;  // the device decides, the host reads the flag
        for (uint32_t changed = 1; changed; ++rounds) {
            BBK_HIP(hipMemsetAsync(st + 2, 0, 4, ctx->stream));
            launch_items_timed(ctx, "hc_jump", k_hc_jump, n, label, n, st + 2);
            BBK_HIP(hipMemcpyAsync(&changed, st + 2, 4, hipMemcpyDeviceToHost, ctx->stream));
            BBK_HIP(hipStreamSynchronize(ctx->stream));
        }
        ctx->add_stat("stat_hc_rounds", (double)rounds);
    }

    // the sizes of the components; the members of those of >= lock_size k-mers go through hc_replay; returns how many did
    uint64_t replay_oversize() {
        cnt.alloc(n * 4);
        uint32_t *c = cnt.as<uint32_t>(), h_status[2] = {0, 0};
        BBK_HIP(hipMemsetAsync(c, 0, n * 4, ctx->stream));
        launch_items_timed(ctx, "hc_list", k_hc_count, n, label, n, c);
        BBK_HIP(hipMemcpyAsync(h_status, status.p, 8, hipMemcpyDeviceToHost, ctx->stream));
        const auto oversize = per_item(HcOversize{label, c, lock_size});
        const Selection sel = select_count(ctx, "hc_list", n, oversize);  // waits: h_status has arrived
        const uint64_t R = sel.kept;
        ctx->add_stat("stat_hc_largest_block", (double)h_status[1]);
        if (R) {
            DevBuf oi(R * 4), ok(R * 8), orc(R * 4);
            select_write(ctx, "hc_list", sel, oversize,
                         HcStoreMember{s->keys.as<uint64_t>(), rcidx.as<uint32_t>(), oi.as<uint32_t>(), ok.as<uint64_t>(),
                                       orc.as<uint32_t>()});
            std::vector<uint32_t> h_idx(R), h_rc(R), h_lab;
            std::vector<uint64_t> h_key(R);
            BBK_HIP(hipMemcpyAsync(h_idx.data(), oi.p, R * 4, hipMemcpyDeviceToHost, ctx->stream));
            BBK_HIP(hipMemcpyAsync(h_key.data(), ok.p, R * 8, hipMemcpyDeviceToHost, ctx->stream));
            BBK_HIP(hipMemcpyAsync(h_rc.data(), orc.p, R * 4, hipMemcpyDeviceToHost, ctx->stream));
            BBK_HIP(hipStreamSynchronize(ctx->stream));
            hc_replay(s->k, lock_size, chunk, h_idx, h_key, h_rc, h_lab);
            BBK_HIP(hipMemcpyAsync(orc.p, h_lab.data(), R * 4, hipMemcpyHostToDevice, ctx->stream));
            launch_items_timed(ctx, "hc_list", k_hc_relabel, R, oi.as<uint32_t>(), orc.as<uint32_t>(), R, label);
            BBK_HIP(hipMemsetAsync(c, 0, n * 4, ctx->stream));
            launch_items_timed(ctx, "hc_list", k_hc_count, n, label, n, c);
            BBK_HIP(hipStreamSynchronize(ctx->stream));  // h_lab is read by the copy above
        }
        rcidx.release();
        return R;
    }

    // the roots and their sizes; the listing: (label, index) records sorted by label, stably, so a cluster's members ascend
    void list() {
        const auto root = per_item(HcRoot{label});
        const Selection sel = select_count(ctx, "hc_list", n, root);
        h->clusters = sel.kept;
        h->sizes.alloc(h->clusters * 8);
        select_write(ctx, "hc_list", sel, root, HcStoreSize{cnt.as<uint32_t>(), h->sizes.as<uint64_t>()});
        BBK_HIP(hipStreamSynchronize(ctx->stream));
        cnt.release();
        h->members.alloc(n * 4);
        DevBuf ka(n * 8), kb(n * 8), vb(n * 4);
        launch_items_timed(ctx, "hc_list", k_hc_pairs, n, label, n, ka.as<uint64_t>(), h->members.as<uint32_t>());
        unsigned bits = 1;
        while (bits < 32 && ((n - 1) >> bits)) ++bits;
        sort_records(ctx, 1, ka.p, kb.p, h->members.as<uint32_t>(), vb.as<uint32_t>(), n, key_passes((bits + 1) / 2));
        BBK_HIP(hipStreamSynchronize(ctx->stream));
    }
};

static void hc_export(bbk_ctx *ctx, const bbk_hamclusters *h, uint64_t *h_labels, uint64_t *h_members, uint64_t *h_sizes) {
    BBK_HIP(hipSetDevice(ctx->device));
    if (h->n == 0) return;
    raw_vector<uint32_t> tmp(h->n);
    for (int which = 0; which < 2; ++which) {
        uint64_t *dst = which ? h_members : h_labels;
        if (!dst) continue;
        d2h_big(ctx, tmp.data(), which ? h->members.p : h->labels.p, h->n * 4);
        for (uint64_t i = 0; i < h->n; ++i) dst[i] = tmp[i];
    }
    if (h_sizes) d2h_big(ctx, h_sizes, h->sizes.p, h->clusters * 8);
}

}  // namespace bbk

using namespace bbk;

extern "C" {

int bbk_kmerset_hamming_clusters(bbk_ctx *ctx, const bbk_kmerset *set, unsigned tau, uint64_t lock_size, uint64_t chunk,
                                 bbk_hamclusters **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && set && out, BBK_ERR_ARG, "bbk_kmerset_hamming_clusters: NULL argument");
        BBK_REQUIRE(tau == 1, BBK_ERR_ARG, "bbk_kmerset_hamming_clusters: tau = %u: tau > 1 not built (and tau = 0 unites nothing)",
                    tau);
        require_hammer_set("bbk_kmerset_hamming_clusters", set);
        BBK_HIP(hipSetDevice(ctx->device));
        auto h = std::make_unique<bbk_hamclusters>();
        h->n = set->n;
        for (DevBuf *b : {&h->labels, &h->members, &h->sizes}) b->alloc(16);  // what an empty set keeps
        if (set->n) {
            HcRun r{ctx, set, h.get(), set->n, lock_size ? lock_size : kHcLockSize, chunk ? chunk : kHcChunk};
            r.unite();
            h->replayed = r.replay_oversize();
            r.list();
        }
        *out = h.release();
    });
}

uint64_t bbk_hamclusters_count(const bbk_hamclusters *h) { return h ? h->clusters : 0; }
uint64_t bbk_hamclusters_size(const bbk_hamclusters *h) { return h ? h->n : 0; }
uint64_t bbk_hamclusters_replayed(const bbk_hamclusters *h) { return h ? h->replayed : 0; }

int bbk_hamclusters_export(bbk_ctx *ctx, const bbk_hamclusters *h, uint64_t *h_labels, uint64_t *h_members,
                           uint64_t *h_sizes) {
    return guarded([&] {
        BBK_REQUIRE(ctx && h, BBK_ERR_ARG, "bbk_hamclusters_export: NULL argument");
        hc_export(ctx, h, h_labels, h_members, h_sizes);
    });
}

int bbk_hamclusters_write(bbk_ctx *ctx, const bbk_hamclusters *h, const char *path) {
    return guarded([&] {
        BBK_REQUIRE(ctx && h && path, BBK_ERR_ARG, "bbk_hamclusters_write: NULL argument");
        raw_vector<uint64_t> members(h->n), sizes(h->clusters);
        hc_export(ctx, h, nullptr, members.data(), sizes.data());
        write_u64_file(path, members.data(), h->n);
        write_u64_file(std::string(path) + ".idx", sizes.data(), h->clusters);
    });
}

int bbk_hamclusters_load(bbk_ctx *ctx, uint64_t n, const char *path, bbk_hamclusters **out) {
    return guarded([&] {
        BBK_REQUIRE(ctx && path && out, BBK_ERR_ARG, "bbk_hamclusters_load: NULL argument");
        require_hammer_count("bbk_hamclusters_load", n);
        BBK_HIP(hipSetDevice(ctx->device));
        raw_vector<uint64_t> mem, sz;
        std::vector<uint64_t> sizes;
        std::vector<uint32_t> members, labels;
        read_u64_file(path, "bbk_hamclusters_load", mem);
        read_u64_file(std::string(path) + ".idx", "bbk_hamclusters_load", sz);
        const std::string err = hamclusters_normalise(path, mem.data(), mem.size(), sz.data(), sz.size(), n, members, labels, sizes);
        BBK_REQUIRE(err.empty(), BBK_ERR_ARG, "bbk_hamclusters_load: %s", err.c_str());
        auto h = std::make_unique<bbk_hamclusters>();
        h->n = n;
        h->clusters = sizes.size();
        upload(ctx, h->labels, labels.data(), n);
        upload(ctx, h->members, members.data(), n);
        upload(ctx, h->sizes, sizes.data(), sizes.size());
        if (n) BBK_HIP(hipStreamSynchronize(ctx->stream));  // the three arrays are on this frame
        *out = h.release();
    });
}

void bbk_hamclusters_free(bbk_hamclusters *h) { delete h; }

}  // extern "C"
