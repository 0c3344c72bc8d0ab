// unique.hip -- unique / reduce-by-key over a sorted record array, and the compaction of the pairs with a non-zero
// value, on gfx950.  The std::unique half of what sort.hip replaces (common/utils/kmer_mph/kmer_splitter.hpp:120-167;
// the counts are what the loser-tree merge of kmer_index_builder.hpp:281-365 adds up).  Integer/HBM-bound work: no MFMA.
#include <hip/hip_runtime.h>

#include "bbk_internal.h"
#include "block_scan.h"
#include "kmer_ops.h"
#include "select.h"

namespace bbk {

constexpr int kUniqItems = 8;
constexpr int kUniqTile = kThreads * kUniqItems;

template <int W>
__device__ inline bool is_head(const Key<W> *__restrict__ keys, uint64_t idx) {
    if (idx == 0) return true;
    return !key_eq<W>(keys[idx], keys[idx - 1]);
}

template <int W>
__global__ __launch_bounds__(kThreads) void k_head_count(const Key<W> *__restrict__ keys, uint64_t n,
                                                        uint64_t *__restrict__ bcount) {
    __shared__ uint32_t sm[kWaves];
    const uint64_t base = (uint64_t)blockIdx.x * kUniqTile;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < kUniqItems; ++i) {
        uint64_t idx = base + (uint64_t)i * kThreads + threadIdx.x;
        if (idx < n && is_head<W>(keys, idx)) ++c;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_down(c, d, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < kWaves; ++w) t += sm[w];
        bcount[blockIdx.x] = t;
    }
}

// writes distinct keys and the index of each run head (head_idx has ndistinct+1 entries; the
// last one, = n, is written by the host wrapper)
template <int W>
__global__ __launch_bounds__(kThreads) void k_head_compact(const Key<W> *__restrict__ keys, uint64_t n,
                                                          const uint64_t *__restrict__ boff,
                                                          Key<W> *__restrict__ out_keys,
                                                          uint32_t *__restrict__ head_idx) {
    __shared__ uint32_t scan_tmp[kWaves + 1];
    const uint64_t base = (uint64_t)blockIdx.x * kUniqTile + (uint64_t)threadIdx.x * kUniqItems;
    bool h[kUniqItems];
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < kUniqItems; ++i) {
        h[i] = (base + i < n) && is_head<W>(keys, base + i);
        c += h[i] ? 1u : 0u;
    }
    uint32_t tot;
    uint32_t pre = block_excl_scan(c, scan_tmp, &tot);
    uint64_t pos = boff[blockIdx.x] + pre;
#pragma unroll
    for (int i = 0; i < kUniqItems; ++i) {
        if (h[i]) {
            if (out_keys) out_keys[pos] = keys[base + i];
            head_idx[pos] = (uint32_t)(base + i);
            ++pos;
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_seg_reduce(const uint32_t *__restrict__ head_idx, uint64_t nseg,
                                                        const uint32_t *__restrict__ vals, int op,
                                                        uint32_t *__restrict__ out_vals) {
    const uint64_t s = BBK_GID();
    if (s >= nseg) return;
    const uint32_t a = head_idx[s], b = head_idx[s + 1];
    uint32_t r;
    if (op == REDUCE_COUNT) {
        r = b - a;
    } else if (op == REDUCE_SUM) {  // modulo 2^32, like the MSD bucket kernels (bbk.h: BBK_WITH_COUNTS)
        r = 0;
        for (uint32_t i = a; i < b; ++i) r += vals[i];
    } else {
        r = 0;
        for (uint32_t i = a; i < b; ++i) r |= vals[i];
    }
    out_vals[s] = r;
}

template <int W>
static uint64_t unique_impl(bbk_ctx *ctx, const Key<W> *keys, const uint32_t *vals, uint64_t n, Key<W> *out_keys,
                            uint32_t *out_vals, ReduceOp op) {
    if (n == 0) return 0;
    BBK_REQUIRE(n < (1ull << 32), BBK_ERR_ARG, "unique_records: n=%llu does not fit 32-bit offsets",
                (unsigned long long)n);
    const uint64_t nb = (n + kUniqTile - 1) / kUniqTile;
    DevBuf bcount(nb * sizeof(uint64_t));
    launch_timed(ctx, k_head_count<W>, "unique", (double)n * sizeof(Key<W>), (uint32_t)nb, kThreads, 0, keys, n,
                 bcount.as<uint64_t>());
    const uint64_t nd = exclusive_scan_u64(ctx, bcount.as<uint64_t>(), bcount.as<uint64_t>(), nb);
    DevBuf head((nd + 1) * sizeof(uint32_t));
    launch_timed(ctx, k_head_compact<W>, "unique", (double)n * sizeof(Key<W>) + (double)nd * sizeof(Key<W>), (uint32_t)nb,
                 kThreads, 0, keys, n, bcount.as<uint64_t>(), out_keys, head.as<uint32_t>());
    const uint32_t n32 = (uint32_t)n;
    BBK_HIP(hipMemcpyAsync(head.as<uint32_t>() + nd, &n32, sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    if (out_vals) {
        KernelTimer t(ctx, "reduce", (double)nd * 8 + (vals ? (double)n * 4 : 0));
        launch_items(ctx, "k_seg_reduce", k_seg_reduce, nd, head.as<uint32_t>(), nd, vals, (int)op, out_vals);
    }
    stream_wait(ctx);
    return nd;
}

// ---- ordered selections on a u32 value (select.h) ----------------------------------------------------------------------
struct ValAtLeast {
    const uint32_t *__restrict__ vals;
    uint32_t min;
    __device__ bool operator()(uint64_t i) const { return vals[i] >= min; }
};

template <int W>
struct MovePair {
    const Key<W> *__restrict__ keys;
    const uint32_t *__restrict__ vals;
    Key<W> *__restrict__ out_keys;
    uint32_t *__restrict__ out_vals;
    __device__ void operator()(uint64_t i, uint64_t rank) const {
        out_keys[rank] = keys[i];
        out_vals[rank] = vals[i];
    }
};

struct StoreIndexAndVal {
    const uint32_t *__restrict__ vals;
    uint64_t *__restrict__ out_idx;
    uint32_t *__restrict__ out_vals;
    __device__ void operator()(uint64_t i, uint64_t rank) const {
        out_idx[rank] = i;
        out_vals[rank] = vals[i];
    }
};

// Compacts the (key, val) pairs with val != 0 into out_* (allocated here, only when something is dropped); returns
// how many were kept (if all are kept nothing is allocated or written: the usual case).
uint64_t drop_zero_vals(bbk_ctx *ctx, int W, const void *keys, const uint32_t *vals, uint64_t n, DevBuf &out_keys,
                        DevBuf &out_vals) {
    const U32AtLeast nonzero{vals, 1u};  // (vals is the start of the caller's buffer)
    const Selection sel = select_count(ctx, "drop_zero", n, nonzero);
    if (sel.kept == n) return n;
    out_keys.alloc(sel.kept * (size_t)W * 8 + 16);
    out_vals.alloc(sel.kept * 4 + 16);
    dispatch_w((unsigned)W, [&](auto w) {
        constexpr int W_ = decltype(w)::value;
        select_write(ctx, "drop_zero", sel, nonzero,
                     MovePair<W_>{(const Key<W_> *)keys, vals, out_keys.as<Key<W_>>(), out_vals.as<uint32_t>()});
    });
    stream_wait(ctx);
    return sel.kept;
}

uint64_t unique_records(bbk_ctx *ctx, int W, const void *keys, const uint32_t *vals, uint64_t n, void *out_keys,
                        uint32_t *out_vals, ReduceOp op) {
    uint64_t distinct = 0;
    dispatch_w((unsigned)W, [&](auto w) {
        using K = Key<decltype(w)::value>;
        distinct = unique_impl(ctx, (const K *)keys, vals, n, (K *)out_keys, out_vals, op);
    });
    return distinct;
}

}  // namespace bbk

using namespace bbk;

extern "C" {

int bbk_select_u32(bbk_ctx *ctx, const void *d_vals, uint64_t n, uint32_t min, void *d_idx_out, void *d_val_out,
                   uint64_t *kept) {
    return guarded([&] {
        BBK_REQUIRE(ctx && kept && (n == 0 || (d_vals && d_idx_out && d_val_out)), BBK_ERR_ARG,
                    "bbk_select_u32: NULL argument");
        BBK_HIP(hipSetDevice(ctx->device));
        const uint32_t *vals = (const uint32_t *)d_vals;
        const auto pred = per_item(ValAtLeast{vals, min});
        const Selection sel = select_count(ctx, "select_u32", n, pred);
        select_write(ctx, "select_u32", sel, pred, StoreIndexAndVal{vals, (uint64_t *)d_idx_out, (uint32_t *)d_val_out});
        stream_wait(ctx);
        *kept = sel.kept;
    });
}

}  // extern "C"
