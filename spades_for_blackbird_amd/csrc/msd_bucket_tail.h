// msd_bucket_tail.h -- the copy-out step of k_bucket_dist_nb (msd_stage_b.h) over plain arrays, so that the host can
// run it too (tests/bucket_tail_check.cpp).  No HIP types: includable from a plain C++ translation unit.
#pragma once

#include <cstdint>

#include "host_device.h"

namespace bbk {

// Position s < n of a bucket whose n 32-bit offsets lie sorted in `sorted`: the key (base + offset) & mask goes to
// dst[s], the place it has in a bucket without duplicates.  Returns whether s and s - 1 hold the same offset (a
// duplicate: the caller discards the whole output, so what a bucket with one stores is of no consequence).
BBK_HOST_DEVICE inline bool dist_tail_at(const uint32_t *sorted, uint32_t s, uint64_t base, uint64_t mask, uint64_t *dst) {
    const uint32_t x = sorted[s];
    dst[s] = (base + x) & mask;
    return s > 0 && sorted[s - 1] == x;
}

// The rows a workgroup of nt lanes walks for n records (record p = row * nt + lane): rows in use, ceil(n / nt).
BBK_HOST_DEVICE inline uint32_t bucket_rows(uint32_t n, uint32_t nt) { return (n + nt - 1u) / nt; }

}  // namespace bbk
