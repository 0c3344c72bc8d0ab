// block_scan.h -- the workgroup shape (256 threads, four waves) and the block-wide scan that scan.hip, sort.hip and
// unique.hip share.  Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace bbk {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

// ------------------------------------------------------------------------------------------
// block-wide exclusive scan of one u32 per thread (256 threads), wave shuffles + LDS
// ------------------------------------------------------------------------------------------
__device__ inline uint32_t wave_incl_scan(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// returns the exclusive prefix of v over the block; *total receives the block sum.
__device__ inline uint32_t block_excl_scan(uint32_t v, uint32_t *smem_waves /*[kWaves+1]*/, uint32_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = wave_incl_scan(v);
    if (lane == 63) smem_waves[wave] = incl;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        uint32_t s = smem_waves[w];
        if (w < wave) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + incl - v;
}

}  // namespace bbk
