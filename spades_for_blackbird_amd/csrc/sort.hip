// sort.hip -- stable LSD radix sort of fixed-width k-mer records (+ optional u32 payload) on gfx950, and its single pass
// as a stable partition: LDS-staged digit histograms, wavefront ballot match-any ranking (64-wide) and an LDS reorder so
// that global stores leave the CU as contiguous per-digit runs.  With unique.hip it replaces, on the device, what the
// reference does with libcxx::sort + std::unique per bucket (common/utils/kmer_mph/kmer_splitter.hpp:120-167) and the
// loser-tree merge (kmer_index_builder.hpp:281-365).  Integer/HBM-bound work: no MFMA.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "bbk_internal.h"
#include "block_scan.h"
#include "kmer_ops.h"

namespace bbk {

constexpr int kRadix = 256;

template <int W>
struct SortCfg {
    // tile sized so that static + staged LDS stays below 64 KiB for every key width
    static constexpr int ITEMS = (W == 1) ? 16 : (W <= 3 ? 8 : 4);
    static constexpr int TILE = kThreads * ITEMS;
};

// Digit of a record that sits in memory (global or LDS) at p.  For a key-bit pass the sort word
// is re-read from memory with a dynamic MEMORY index: indexing the register copy with the
// runtime pd.word would push the whole tile to scratch.
template <int W>
__device__ inline uint32_t digit_of(const Key<W> &key, const Key<W> *p, const PassDesc &pd) {
    if (pd.kind == 0) {
        const uint64_t w = (W == 1) ? key.w[0] : reinterpret_cast<const uint64_t *>(p)[pd.word];
        return (uint32_t)(w >> pd.shift) & ((1u << pd.bits) - 1u);
    }
    if (pd.kind == 1) return (uint32_t)__umul64hi(xxh3_64<W>(key), (uint64_t)pd.nb);
    return (uint32_t)__umul64hi(owner_mix<W>(key), (uint64_t)pd.nb);
}

// per-tile digit histogram -> hist[tile][256]
template <int W>
__global__ __launch_bounds__(kThreads) void k_hist(const Key<W> *__restrict__ in, uint64_t n, PassDesc pd,
                                                  uint32_t *__restrict__ hist) {
    constexpr int ITEMS = SortCfg<W>::ITEMS, TILE = SortCfg<W>::TILE;
    __shared__ uint32_t h[kRadix];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * TILE;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        uint64_t idx = base + (uint64_t)i * kThreads + threadIdx.x;
        if (idx < n) {
            const Key<W> key = key_load<W>(&in[idx]);
            atomicAdd(&h[digit_of<W>(key, &in[idx], pd)], 1u);
        }
    }
    __syncthreads();
    hist[(uint64_t)blockIdx.x * kRadix + threadIdx.x] = h[threadIdx.x];
}

// column sums over chunks of kChunk tiles
constexpr int kChunk = 256;
__global__ __launch_bounds__(kRadix) void k_colsum(const uint32_t *__restrict__ hist, uint64_t ntiles,
                                                  uint64_t *__restrict__ chunk_sum) {
    const uint64_t t0 = (uint64_t)blockIdx.x * kChunk;
    const uint64_t t1 = (t0 + kChunk < ntiles) ? t0 + kChunk : ntiles;
    uint64_t s = 0;
    for (uint64_t t = t0; t < t1; ++t) s += hist[t * kRadix + threadIdx.x];
    chunk_sum[(uint64_t)blockIdx.x * kRadix + threadIdx.x] = s;
}

// single block: chunk_sum[c][d] -> exclusive global base of (chunk c, digit d) in digit-major order
__global__ __launch_bounds__(kRadix) void k_scan_chunks(uint64_t *__restrict__ chunk_sum, uint64_t nchunks,
                                                       uint64_t *__restrict__ digit_total) {
    __shared__ uint64_t tot[kRadix];
    const int d = threadIdx.x;
    uint64_t run = 0;
    for (uint64_t c = 0; c < nchunks; ++c) {
        uint64_t v = chunk_sum[c * kRadix + d];
        chunk_sum[c * kRadix + d] = run;
        run += v;
    }
    tot[d] = run;
    if (digit_total) digit_total[d] = run;
    __syncthreads();
    uint64_t base = 0;
    for (int j = 0; j < d; ++j) base += tot[j];
    for (uint64_t c = 0; c < nchunks; ++c) chunk_sum[c * kRadix + d] += base;
}

// hist[t][d] (counts) -> global start offset of (tile t, digit d)
__global__ __launch_bounds__(kRadix) void k_tile_offsets(uint32_t *__restrict__ hist, uint64_t ntiles,
                                                        const uint64_t *__restrict__ chunk_base) {
    const uint64_t t0 = (uint64_t)blockIdx.x * kChunk;
    const uint64_t t1 = (t0 + kChunk < ntiles) ? t0 + kChunk : ntiles;
    // offsets RELATIVE to the chunk's base (a chunk of 256 tiles holds < 2^32 records): the scatter kernel adds the
    // 64-bit base, so that an array of 2^32 records or more (up to the tile limit of sort_scratch) sorts like any other
    uint32_t run = 0;
    for (uint64_t t = t0; t < t1; ++t) {
        uint32_t v = hist[t * kRadix + threadIdx.x];
        hist[t * kRadix + threadIdx.x] = run;
        run += v;
    }
    (void)chunk_base;
}

// wavefront match-any on an 8-bit digit: mask of lanes (among `valid` lanes) holding the same digit
__device__ inline uint64_t match_digit(uint32_t d, bool valid) {
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const uint64_t m = __ballot(bit);
        peers &= bit ? m : ~m;
    }
    return peers;
}

template <int W, bool HAS_VAL>
__global__ __launch_bounds__(kThreads) void k_scatter(const Key<W> *__restrict__ in, Key<W> *__restrict__ out,
                                                     const uint32_t *__restrict__ vin, uint32_t *__restrict__ vout,
                                                     uint64_t n, PassDesc pd,
                                                     const uint32_t *__restrict__ tile_off,
                                                     const uint64_t *__restrict__ chunk_base) {
    constexpr int ITEMS = SortCfg<W>::ITEMS, TILE = SortCfg<W>::TILE;
    __shared__ uint32_t wave_cnt[kWaves][kRadix];
    __shared__ uint32_t digit_start[kRadix];
    __shared__ uint64_t goff[kRadix];
    __shared__ uint32_t scan_tmp[kWaves + 1];
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
    Key<W> *stage = reinterpret_cast<Key<W> *>(dyn_smem);
    uint32_t *vstage = reinterpret_cast<uint32_t *>(dyn_smem + sizeof(Key<W>) * TILE);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t tile = blockIdx.x;
    const uint64_t base = tile * TILE;
    const uint32_t tile_n = (uint32_t)((n - base < (uint64_t)TILE) ? (n - base) : (uint64_t)TILE);

#pragma unroll
    for (int w = 0; w < kWaves; ++w) wave_cnt[w][tid] = 0;
    __syncthreads();

    Key<W> keys[ITEMS];
    uint32_t vals[ITEMS];
    uint32_t dig[ITEMS];
    uint32_t rank[ITEMS];
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t local = (uint32_t)(wave * (ITEMS * 64) + i * 64 + lane);
        const bool valid = local < tile_n;
        uint32_t d = 0;
#pragma unroll
        for (int j = 0; j < W; ++j) keys[i].w[j] = 0;
        vals[i] = 0;
        if (valid) {
            keys[i] = key_load<W>(&in[base + local]);
            if (HAS_VAL) vals[i] = vin[base + local];
            d = digit_of<W>(keys[i], &in[base + local], pd);
        }
        dig[i] = d;
        const uint64_t peers = match_digit(d, valid);
        const uint32_t pre = wave_cnt[wave][d];
        rank[i] = pre + (uint32_t)__popcll(peers & lt_mask);
        // the highest lane of each peer group publishes the new running count
        if (valid && (peers >> lane) == 1ull) wave_cnt[wave][d] = pre + (uint32_t)__popcll(peers);
    }
    __syncthreads();

    // digit tid: exclusive prefix over waves, then exclusive scan over digits
    uint32_t tot = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        uint32_t c = wave_cnt[w][tid];
        wave_cnt[w][tid] = tot;
        tot += c;
    }
    uint32_t tile_total;
    const uint32_t dstart = block_excl_scan(tot, scan_tmp, &tile_total);
    digit_start[tid] = dstart;
    goff[tid] = chunk_base[(tile / kChunk) * kRadix + tid] + tile_off[tile * kRadix + tid] - dstart;  // + pos below
    __syncthreads();

#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t local = (uint32_t)(wave * (ITEMS * 64) + i * 64 + lane);
        if (local < tile_n) {
            const uint32_t pos = digit_start[dig[i]] + wave_cnt[wave][dig[i]] + rank[i];
            key_store<W>(&stage[pos], keys[i]);
            if (HAS_VAL) vstage[pos] = vals[i];
        }
    }
    __syncthreads();

#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t pos = (uint32_t)(i * kThreads + tid);
        if (pos < tile_n) {
            const Key<W> key = key_load<W>(&stage[pos]);
            const uint32_t d = digit_of<W>(key, &stage[pos], pd);
            const uint64_t g = goff[d] + pos;
            key_store<W>(&out[g], key);
            if (HAS_VAL) vout[g] = vstage[pos];
        }
    }
}

std::vector<PassDesc> key_passes(unsigned k) {
    // least significant first: last word (populated low bits only) ... word 0
    std::vector<PassDesc> p;
    const int W = (int)words_of(k);
    for (int w = W - 1; w >= 0; --w) {
        const int bits = (w == W - 1) ? (int)(2 * k - 64 * (W - 1)) : 64;
        for (int s = 0; s < bits; s += 8) {
            const int b = (bits - s < 8) ? bits - s : 8;
            p.push_back({0, w, s, b, 0});
        }
    }
    return p;
}

// one stable counting pass src -> dst on the digit `pd` (hist/chunk: scratch of the caller)
template <int W>
static void sort_pass(bbk_ctx *ctx, const Key<W> *src, Key<W> *dst, const uint32_t *vsrc, uint32_t *vdst, uint64_t n,
                      const PassDesc &pd, DevBuf &hist, DevBuf &chunk, uint64_t *d_digit_totals = nullptr) {
    constexpr int TILE = SortCfg<W>::TILE;
    const uint64_t ntiles = (n + TILE - 1) / TILE;
    const uint64_t nchunks = (ntiles + kChunk - 1) / kChunk;
    const bool hv = vsrc != nullptr;
    const size_t dyn = sizeof(Key<W>) * TILE + (hv ? sizeof(uint32_t) * TILE : 0);
    const double rec_bytes = (double)(sizeof(Key<W>) + (hv ? 4 : 0));
    launch_timed(ctx, k_hist<W>, "hist", (double)n * sizeof(Key<W>), (uint32_t)ntiles, kThreads, 0, src, n, pd,
                 hist.as<uint32_t>());
    {
        KernelTimer t(ctx, "scan", (double)ntiles * kRadix * 4 * 3);
        hipLaunchKernelGGL(k_colsum, dim3((unsigned)nchunks), dim3(kRadix), 0, ctx->stream, hist.as<uint32_t>(), ntiles,
                           chunk.as<uint64_t>());
        hipLaunchKernelGGL(k_scan_chunks, dim3(1), dim3(kRadix), 0, ctx->stream, chunk.as<uint64_t>(), nchunks,
                           d_digit_totals);
        hipLaunchKernelGGL(k_tile_offsets, dim3((unsigned)nchunks), dim3(kRadix), 0, ctx->stream, hist.as<uint32_t>(),
                           ntiles, chunk.as<uint64_t>());
        check_launch("scan kernels");
    }
    {
        KernelTimer t(ctx, "scatter", 2.0 * (double)n * rec_bytes);
        if (hv) {
            hipLaunchKernelGGL((k_scatter<W, true>), dim3((unsigned)ntiles), dim3(kThreads), dyn, ctx->stream, src, dst,
                               vsrc, vdst, n, pd, hist.as<uint32_t>(), chunk.as<uint64_t>());
        } else {
            hipLaunchKernelGGL((k_scatter<W, false>), dim3((unsigned)ntiles), dim3(kThreads), dyn, ctx->stream, src, dst,
                               (const uint32_t *)nullptr, (uint32_t *)nullptr, n, pd, hist.as<uint32_t>(), chunk.as<uint64_t>());
        }
        check_launch("k_scatter");
    }
}

template <int W>
static void sort_scratch(uint64_t n, bool with_vals, DevBuf &hist, DevBuf &chunk) {
    constexpr int TILE = SortCfg<W>::TILE;
    const uint64_t ntiles = (n + TILE - 1) / TILE;
    // k_hist / k_scatter launch one workgroup per tile in x: 2^32 threads or more would be cut short without an error
    // (bbk_internal.h, BBK_GID), i.e. n < 2^24 tiles = 2^36 records (8-byte keys) .. 2^34 (32-byte keys)
    BBK_REQUIRE(ntiles * kThreads < (1ull << 32), BBK_ERR_ARG, "sort_records: n=%llu records exceed %llu tiles",
                (unsigned long long)n, (unsigned long long)((1ull << 32) / kThreads));
    const uint64_t nchunks = (ntiles + kChunk - 1) / kChunk;
    hist.alloc(ntiles * kRadix * sizeof(uint32_t));
    chunk.alloc(nchunks * kRadix * sizeof(uint64_t));
    const size_t dyn = sizeof(Key<W>) * TILE + (with_vals ? sizeof(uint32_t) * TILE : 0);
    if (with_vals) {
        BBK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_scatter<W, true>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
    } else {
        BBK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_scatter<W, false>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
    }
}

template <int W>
static void sort_impl(bbk_ctx *ctx, Key<W> *keys, Key<W> *tmp, uint32_t *vals, uint32_t *vtmp, uint64_t n,
                      const std::vector<PassDesc> &passes) {
    if (n <= 1 || passes.empty()) return;
    DevBuf hist, chunk;
    sort_scratch<W>(n, vals != nullptr, hist, chunk);
    Key<W> *src = keys, *dst = tmp;
    uint32_t *vsrc = vals, *vdst = vtmp;
    for (const PassDesc &pd : passes) {
        sort_pass<W>(ctx, src, dst, vsrc, vdst, n, pd, hist, chunk);
        std::swap(src, dst);
        std::swap(vsrc, vdst);
    }
    if (src != keys) {
        BBK_HIP(bbk::copy_async(keys, src, n * sizeof(Key<W>), hipMemcpyDeviceToDevice, ctx->stream));
        if (vals) BBK_HIP(bbk::copy_async(vals, vsrc, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
    }
    stream_wait(ctx);  // hist/chunk are freed on return
}

template <int W>
static void partition_impl(bbk_ctx *ctx, const Key<W> *src, Key<W> *dst, const uint32_t *vsrc, uint32_t *vdst, uint64_t n,
                           const PassDesc &pd, uint64_t *h_digit_totals) {
    if (h_digit_totals) memset(h_digit_totals, 0, kRadix * sizeof(uint64_t));
    if (n == 0) return;
    DevBuf hist, chunk, tot;
    sort_scratch<W>(n, vsrc != nullptr, hist, chunk);
    if (h_digit_totals) tot.alloc(kRadix * sizeof(uint64_t));
    sort_pass<W>(ctx, src, dst, vsrc, vdst, n, pd, hist, chunk, h_digit_totals ? tot.as<uint64_t>() : nullptr);
    if (h_digit_totals)
        BBK_HIP(hipMemcpyAsync(h_digit_totals, tot.p, kRadix * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    stream_wait(ctx);
}

// one stable pass src -> dst (both on the device, not aliased): records ordered by the digit, input order kept inside
void partition_records(bbk_ctx *ctx, int W, const void *src, void *dst, const uint32_t *vsrc, uint32_t *vdst, uint64_t n,
                       const PassDesc &pd, uint64_t *h_digit_totals) {
    dispatch_w((unsigned)W, [&](auto w) {
        using K = Key<decltype(w)::value>;
        partition_impl(ctx, (const K *)src, (K *)dst, vsrc, vdst, n, pd, h_digit_totals);
    });
}

void sort_records(bbk_ctx *ctx, int W, void *keys, void *keys_tmp, uint32_t *vals, uint32_t *vals_tmp, uint64_t n,
                  const std::vector<PassDesc> &passes) {
    dispatch_w((unsigned)W, [&](auto w) {
        using K = Key<decltype(w)::value>;
        sort_impl(ctx, (K *)keys, (K *)keys_tmp, vals, vals_tmp, n, passes);
    });
}

}  // namespace bbk
