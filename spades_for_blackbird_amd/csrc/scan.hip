// scan.hip -- device-wide exclusive scan of u64 on gfx950: one array, or two arrays of the same length in the same
// launches, and the read plan built on it.  It replaces the running sums the reference keeps on the host while it
// splits reads into buckets (common/utils/kmer_mph/kmer_splitter.hpp).  Integer/HBM-bound work: no MFMA.
#include <hip/hip_runtime.h>

#include <vector>

#include "bbk_internal.h"
#include "block_scan.h"

namespace bbk {

// Reduce-then-apply over tiles of 4096 items: 16 M items take two levels (10 M reads: 2442 block sums, one block).
// The top level is ONE workgroup that scans its (at most kScanTile) items in place and leaves the grand total in device
// memory -- and behind the output array when the caller wants out[n] = total -- so no level needs a copy, a fill or
// the host.
constexpr int kScanItems = 16;
constexpr int kScanTile = kThreads * kScanItems;

struct ScanArrs {
    ScanSrc src[2];
    uint64_t *out[2];
    uint64_t *bsum[2];   // block sums of this level (reduce: written; apply: read, already scanned)
    uint64_t *total[2];  // top level: the grand total goes here ...
    uint64_t *tail[2];   // ... and here when not null
};

__device__ inline uint64_t scan_load(const ScanSrc &s, uint64_t i) {
    if (s.kind == SCAN_U64) return reinterpret_cast<const uint64_t *>(s.p)[i];
    const uint32_t v = reinterpret_cast<const uint32_t *>(s.p)[i];
    if (s.kind == SCAN_U32_FLAGGED) return v == 0xFFFFFFFFu ? 0ull : (uint64_t)v;
    if (s.kind == SCAN_READ_UNITS) {  // v = len: k-mers, in units of cap
        const uint32_t c = v >= s.stride ? v - s.stride + 1u : 0u;
        if (c == 0u) return 0ull;
        // (a uniform choice: the unit lengths in use are powers of two)
        const uint32_t q = (s.cap & (s.cap - 1u)) ? (c - 1u) / s.cap : (c - 1u) >> (__ffs(s.cap) - 1);
        return (uint64_t)q + 1ull;
    }
    const uint32_t c = v - (uint32_t)i * s.stride;  // SCAN_SLOT_FILL
    return c < s.cap ? c : s.cap;
}

// SCAN_READ_UNITS with woff: do the words of read i + 1 start before those of read i end?
// (the callers store the flag once, behind their loop: a store between the loads of two items would make every item
// wait for its own loads)
__device__ inline bool scan_out_of_order(const ScanSrc &s, uint64_t i, uint64_t n) {
    const uint32_t L = reinterpret_cast<const uint32_t *>(s.p)[i];
    return i + 1 < n && s.woff[i + 1] < s.woff[i] + ((L + 31u) >> 5);
}

template <int NA>
__global__ __launch_bounds__(kThreads) void k_scan_reduce(ScanArrs A, uint64_t n) {
    __shared__ uint64_t sm[NA][kWaves];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        uint64_t s = 0;
        const bool check = A.src[a].kind == SCAN_READ_UNITS && A.src[a].woff;
        bool bad = false;
#pragma unroll
        for (int i = 0; i < kScanItems; ++i) {
            const uint64_t idx = base + (uint64_t)i * kThreads + threadIdx.x;
            if (idx < n) {
                s += scan_load(A.src[a], idx);
                if (check) bad |= scan_out_of_order(A.src[a], idx, n);
            }
        }
        if (bad) *A.src[a].unordered = 1u;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
        if ((threadIdx.x & 63) == 0) sm[a][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x < NA) {
        uint64_t t = 0;
        for (int w = 0; w < kWaves; ++w) t += sm[threadIdx.x][w];
        A.bsum[threadIdx.x][blockIdx.x] = t;
    }
}

// TOP: the only workgroup of the last level -- its offset is 0 and it publishes the total; otherwise the workgroup's
// offset is its (scanned) block sum
template <int NA, bool TOP>
__global__ __launch_bounds__(kThreads) void k_scan_apply(ScanArrs A, uint64_t n) {
    __shared__ uint64_t sm[NA][kWaves];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanItems;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        const bool store = A.out[a] != nullptr;  // (uniform) total-only arrays matter at the top level alone
        if (!TOP && !store) continue;
        uint64_t v[kScanItems];
        uint64_t s = 0;
        // (a read source at the top level: n fits one tile and no reduce pass has looked at the word order)
        const bool check = TOP && A.src[a].kind == SCAN_READ_UNITS && A.src[a].woff;
        bool bad = false;
#pragma unroll
        for (int i = 0; i < kScanItems; ++i) {
            v[i] = (base + i < n) ? scan_load(A.src[a], base + i) : 0;
            s += v[i];
            if (check && base + i < n) bad |= scan_out_of_order(A.src[a], base + i, n);
        }
        if (bad) *A.src[a].unordered = 1u;
        uint64_t incl = s;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            uint64_t t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        if (lane == 63) sm[a][wave] = incl;
        __syncthreads();
        uint64_t wbase = 0;
        for (int w = 0; w < wave; ++w) wbase += sm[a][w];
        uint64_t run = (TOP ? 0ull : A.bsum[a][blockIdx.x]) + wbase + incl - s;
#pragma unroll
        for (int i = 0; i < kScanItems; ++i) {
            if (store && base + i < n) A.out[a][base + i] = run;
            run += v[i];
        }
        if (TOP && threadIdx.x == kThreads - 1) {  // run = the sum of everything
            *A.total[a] = run;
            if (A.tail[a]) *A.tail[a] = run;
        }
    }
}

// One level of the scan: block sums, (recursively) their exclusive scan in place, then the blocks.  Nothing waits on the
// host in between: the block-sum buffers of every level live in `keep` until the caller has synchronised.
template <int NA>
static void scan_level(bbk_ctx *ctx, ScanArrs A, uint64_t n, std::vector<DevBuf> &keep) {
    const uint64_t nb = (n + kScanTile - 1) / kScanTile;
    if (nb <= 1) {  // (no items: the totals are 0)
        hipLaunchKernelGGL((k_scan_apply<NA, true>), dim3(1), dim3(kThreads), 0, ctx->stream, A, n);
        check_launch("k_scan_apply");
        return;
    }
    BBK_REQUIRE(nb < (1ull << 31), BBK_ERR_ARG, "scan of %llu items", (unsigned long long)n);
    keep.emplace_back((size_t)NA * (nb + 1) * sizeof(uint64_t));
    uint64_t *bs = keep.back().as<uint64_t>();
    ScanArrs B = A;  // the level above: the block sums, in place
    for (int a = 0; a < NA; ++a) {
        A.bsum[a] = bs + (size_t)a * (nb + 1);
        B.src[a] = ScanSrc{A.bsum[a], SCAN_U64, 0u, 0u};
        B.out[a] = A.bsum[a];  // (total and tail travel up unchanged: the top level writes them)
    }
    hipLaunchKernelGGL((k_scan_reduce<NA>), dim3((unsigned)nb), dim3(kThreads), 0, ctx->stream, A, n);
    check_launch("k_scan_reduce");
    scan_level<NA>(ctx, B, nb, keep);
    hipLaunchKernelGGL((k_scan_apply<NA, false>), dim3((unsigned)nb), dim3(kThreads), 0, ctx->stream, A, n);
    check_launch("k_scan_apply");
}

void exclusive_scan_enqueue(bbk_ctx *ctx, int narr, const ScanSrc *src, uint64_t *const *out, uint64_t n,
                            uint64_t *d_total, bool tail, std::vector<DevBuf> &keep) {
    BBK_REQUIRE(narr == 1 || narr == 2, BBK_ERR_INTERNAL, "scan of %d arrays", narr);
    ScanArrs A{};
    for (int a = 0; a < narr; ++a) {
        A.src[a] = src[a];
        A.out[a] = out[a];
        A.total[a] = d_total + a;
        A.tail[a] = (tail && out[a]) ? out[a] + n : nullptr;
    }
    if (narr == 1) scan_level<1>(ctx, A, n, keep);
    else scan_level<2>(ctx, A, n, keep);
}

uint64_t exclusive_scan_u64(bbk_ctx *ctx, const uint64_t *in, uint64_t *out, uint64_t n) {
    if (n == 0) return 0;
    std::vector<DevBuf> keep;
    keep.reserve(4);  // levels: log_{tile}(n)
    DevBuf dt(16);
    const ScanSrc src{in, SCAN_U64, 0u, 0u};
    exclusive_scan_enqueue(ctx, 1, &src, &out, n, dt.as<uint64_t>(), false, keep);
    uint64_t total = 0;
    BBK_HIP(hipMemcpyAsync(&total, dt.p, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    stream_wait(ctx);  // one wait per scan: the buffers go back now
    return total;
}

void exclusive_scan2_u64(bbk_ctx *ctx, const uint64_t *in0, uint64_t *out0, const uint64_t *in1, uint64_t *out1,
                         uint64_t n, uint64_t totals[2]) {
    std::vector<DevBuf> keep;
    keep.reserve(4);
    DevBuf dt(16);
    const ScanSrc src[2] = {{in0, SCAN_U64, 0u, 0u}, {in1, SCAN_U64, 0u, 0u}};
    uint64_t *const out[2] = {out0, out1};
    exclusive_scan_enqueue(ctx, 2, src, out, n, dt.as<uint64_t>(), true, keep);
    BBK_HIP(hipMemcpyAsync(totals, dt.p, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    stream_wait(ctx);
}

void ReadPlan::run(bbk_ctx *ctx, const bbk_reads *rd, unsigned k, unsigned C, uint32_t *d_unordered) {
    BBK_REQUIRE(k >= 1 && C >= 1, BBK_ERR_INTERNAL, "read plan: k = %u, C = %u", k, C);
    const uint64_t n = rd->n;
    coff.alloc((n + 1) * sizeof(uint64_t));
    std::vector<DevBuf> keep;
    keep.reserve(4);
    DevBuf dt(16);
    // [0] the k-mers (total only), [1] the units; at C = 1 they are the same array
    const ScanSrc src[2] = {{rd->d_len, SCAN_READ_UNITS, k, 1u},
                            {rd->d_len, SCAN_READ_UNITS, k, C, d_unordered ? rd->d_woff : nullptr, d_unordered}};
    uint64_t *const out[2] = {nullptr, coff.as<uint64_t>()};
    const int first = C == 1 ? 1 : 0;
    exclusive_scan_enqueue(ctx, 2 - first, src + first, out + first, n, dt.as<uint64_t>(), true, keep);
    uint64_t tot[2] = {0, 0};
    BBK_HIP(hipMemcpyAsync(tot, dt.p, (2 - first) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    stream_wait(ctx);
    kmers = tot[0];
    units = tot[1 - first];
}

}  // namespace bbk

extern "C" {

int bbk_scan2_u64(bbk_ctx *ctx, void *d_a, void *d_b, uint64_t n, uint64_t *totals) {
    return bbk::guarded([&] {
        BBK_REQUIRE(ctx && d_a && d_b && totals, BBK_ERR_ARG, "bbk_scan2_u64: NULL argument");
        BBK_HIP(hipSetDevice(ctx->device));
        bbk::exclusive_scan2_u64(ctx, (const uint64_t *)d_a, (uint64_t *)d_a, (const uint64_t *)d_b, (uint64_t *)d_b, n,
                                 totals);
    });
}

}  // extern "C"
