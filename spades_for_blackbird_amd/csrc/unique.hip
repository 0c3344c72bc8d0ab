// unique.hip -- unique / reduce-by-key over a sorted record array, and the compaction of the pairs with a non-zero
// value, on gfx950.  The std::unique half of what sort.hip replaces (common/utils/kmer_mph/kmer_splitter.hpp:120-167;
// the counts are what the loser-tree merge of kmer_index_builder.hpp:281-365 adds up).  Integer/HBM-bound work: no MFMA.
#include <hip/hip_runtime.h>

#include "bbk_internal.h"
#include "block_scan.h"
#include "kmer_ops.h"

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

// compaction of (key, val) pairs with val != 0
template <int W>
__global__ __launch_bounds__(kThreads) void k_nonzero_count(const uint32_t *__restrict__ vals, uint64_t n,
                                                           uint64_t *__restrict__ bcount) {
    __shared__ uint32_t sm[kWaves];
    const uint64_t base = (uint64_t)blockIdx.x * kUniqTile;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < kUniqItems; ++i) {
        uint64_t idx = base + (uint64_t)i * kThreads + threadIdx.x;
        if (idx < n && vals[idx] != 0) ++c;
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

template <int W>
__global__ __launch_bounds__(kThreads) void k_nonzero_compact(const Key<W> *__restrict__ keys,
                                                             const uint32_t *__restrict__ vals, uint64_t n,
                                                             const uint64_t *__restrict__ boff,
                                                             Key<W> *__restrict__ out_keys,
                                                             uint32_t *__restrict__ out_vals) {
    __shared__ uint32_t scan_tmp[kWaves + 1];
    const uint64_t base = (uint64_t)blockIdx.x * kUniqTile + (uint64_t)threadIdx.x * kUniqItems;
    bool h[kUniqItems];
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < kUniqItems; ++i) {
        h[i] = (base + i < n) && vals[base + i] != 0;
        c += h[i] ? 1u : 0u;
    }
    uint32_t tot;
    uint32_t pre = block_excl_scan(c, scan_tmp, &tot);
    uint64_t pos = boff[blockIdx.x] + pre;
#pragma unroll
    for (int i = 0; i < kUniqItems; ++i) {
        if (h[i]) {
            out_keys[pos] = keys[base + i];
            out_vals[pos] = vals[base + i];
            ++pos;
        }
    }
}

template <int W>
static uint64_t unique_impl(bbk_ctx *ctx, const Key<W> *keys, const uint32_t *vals, uint64_t n, Key<W> *out_keys,
                            uint32_t *out_vals, ReduceOp op, bool drop_zero) {
    if (n == 0) return 0;
    BBK_REQUIRE(n < (1ull << 32), BBK_ERR_ARG, "unique_records: n=%llu does not fit 32-bit offsets",
                (unsigned long long)n);
    const uint64_t nb = (n + kUniqTile - 1) / kUniqTile;
    DevBuf bcount(nb * sizeof(uint64_t));
    launch_timed(ctx, k_head_count<W>, "unique", (double)n * sizeof(Key<W>), (uint32_t)nb, kThreads, 0, keys, n,
                 bcount.as<uint64_t>());
    const uint64_t nd = exclusive_scan_u64(ctx, bcount.as<uint64_t>(), bcount.as<uint64_t>(), nb);
    DevBuf head((nd + 1) * sizeof(uint32_t));
    const bool need_tmp = drop_zero && op == REDUCE_OR;
    DevBuf tkeys, tvals;
    Key<W> *dk = out_keys;
    uint32_t *dv = out_vals;
    if (need_tmp) {
        tkeys.alloc(nd * sizeof(Key<W>));
        tvals.alloc(nd * sizeof(uint32_t));
        dk = tkeys.as<Key<W>>();
        dv = tvals.as<uint32_t>();
    }
    launch_timed(ctx, k_head_compact<W>, "unique", (double)n * sizeof(Key<W>) + (double)nd * sizeof(Key<W>), (uint32_t)nb,
                 kThreads, 0, keys, n, bcount.as<uint64_t>(), dk, head.as<uint32_t>());
    const uint32_t n32 = (uint32_t)n;
    BBK_HIP(hipMemcpyAsync(head.as<uint32_t>() + nd, &n32, sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    if (dv) {
        KernelTimer t(ctx, "reduce", (double)nd * 8 + (vals ? (double)n * 4 : 0));
        launch_items(ctx, "k_seg_reduce", k_seg_reduce, nd, head.as<uint32_t>(), nd, vals, (int)op, dv);
    }
    uint64_t result = nd;
    if (need_tmp) {
        const uint64_t nb2 = (nd + kUniqTile - 1) / kUniqTile;
        DevBuf bc2(nb2 * sizeof(uint64_t));
        hipLaunchKernelGGL(k_nonzero_count<W>, dim3((unsigned)nb2), dim3(kThreads), 0, ctx->stream, dv, nd,
                           bc2.as<uint64_t>());
        check_launch("k_nonzero_count");
        result = exclusive_scan_u64(ctx, bc2.as<uint64_t>(), bc2.as<uint64_t>(), nb2);
        hipLaunchKernelGGL(k_nonzero_compact<W>, dim3((unsigned)nb2), dim3(kThreads), 0, ctx->stream, dk, dv, nd,
                           bc2.as<uint64_t>(), out_keys, out_vals);
        check_launch("k_nonzero_compact");
        stream_wait(ctx);
    }
    stream_wait(ctx);
    return result;
}

template <int W>
static uint64_t drop_zero_impl(bbk_ctx *ctx, const Key<W> *keys, const uint32_t *vals, uint64_t n, DevBuf &ok,
                               DevBuf &ov) {
    if (n == 0) return 0;
    const uint64_t nb = (n + kUniqTile - 1) / kUniqTile;
    DevBuf bc(nb * sizeof(uint64_t));
    hipLaunchKernelGGL(k_nonzero_count<W>, dim3((unsigned)nb), dim3(kThreads), 0, ctx->stream, vals, n,
                       bc.as<uint64_t>());
    check_launch("k_nonzero_count");
    const uint64_t kept = exclusive_scan_u64(ctx, bc.as<uint64_t>(), bc.as<uint64_t>(), nb);
    if (kept == n) return n;  // nothing to drop: caller keeps its buffers (the usual case: nothing is allocated)
    ok.alloc(kept * sizeof(Key<W>) + 16);
    ov.alloc(kept * 4 + 16);
    hipLaunchKernelGGL(k_nonzero_compact<W>, dim3((unsigned)nb), dim3(kThreads), 0, ctx->stream, keys, vals, n,
                       bc.as<uint64_t>(), ok.as<Key<W>>(), ov.as<uint32_t>());
    check_launch("k_nonzero_compact");
    stream_wait(ctx);
    return kept;
}

// Compacts the (key, val) pairs with val != 0 into out_* (allocated here, only when something is dropped); returns
// how many were kept (if all are kept nothing is allocated or written).
uint64_t drop_zero_vals(bbk_ctx *ctx, int W, const void *keys, const uint32_t *vals, uint64_t n, DevBuf &out_keys,
                        DevBuf &out_vals) {
    uint64_t kept = 0;
    dispatch_w((unsigned)W, [&](auto w) {
        kept = drop_zero_impl(ctx, (const Key<decltype(w)::value> *)keys, vals, n, out_keys, out_vals);
    });
    return kept;
}

uint64_t unique_records(bbk_ctx *ctx, int W, const void *keys, const uint32_t *vals, uint64_t n, void *out_keys,
                        uint32_t *out_vals, ReduceOp op, bool drop_zero) {
    uint64_t distinct = 0;
    dispatch_w((unsigned)W, [&](auto w) {
        using K = Key<decltype(w)::value>;
        distinct = unique_impl(ctx, (const K *)keys, vals, n, (K *)out_keys, out_vals, op, drop_zero);
    });
    return distinct;
}

}  // namespace bbk
