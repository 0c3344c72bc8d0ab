// hammer_files.h -- the two file formats of the BayesHammer stage as plain host code: the binary_write(KMerStat) record
// and the order of a cluster listing.  Standard headers only (no HIP, no bbk_internal.h), so tests/hammer_files_check.cpp
// builds it with g++ alone; hammer.h brings it to hamclust.hip / kmerstat.hip / subclust.hip.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace bbk {

// ---- binary_write(KMerStat), kmer_stat.hpp:170-175 ------------------------------------------------------------------
// count_with_lock (u32: twice the count, the good bit in bit 0 -- 0 after mark_bad), float total_qual, the QualBitSet
// words.  A count of 2^31 or more does not fit: the callers refuse it before they come here.
inline size_t kmstat_record_bytes(unsigned qual_words) { return 8 + 8 * (size_t)qual_words; }

// Records [first, first + m) of a file of n k-mers followed by new k-mers (KMerStat(0, 1.0, NULL)), into out.  count, total_qual,
// qual (read for records below n only) and good (may be null: every bit 0) are the block's slices: entry i is record first + i.
inline void kmstat_pack_block(char *out, unsigned qual_words, uint64_t first, uint64_t m, uint64_t n, const uint32_t *count,
                              const float *total_qual, const uint64_t *qual, const uint8_t *good) {
    const size_t rsz = kmstat_record_bytes(qual_words);
    for (uint64_t i = 0; i < m; ++i) {
        char *o = out + i * rsz;
        const bool old = first + i < n;
        const uint32_t c2 = (old ? count[i] << 1 : 0u) | (good ? good[i] & 1u : 0u);
        const float tq = old ? total_qual[i] : 1.0f;
        memcpy(o, &c2, 4);
        memcpy(o + 4, &tq, 4);
        if (old) memcpy(o + 8, qual + i * qual_words, 8 * (size_t)qual_words);
        else memset(o + 8, 0, 8 * (size_t)qual_words);
    }
}

// The inverse for n records; the good bit is not part of the statistics and is dropped.
inline void kmstat_unpack(const char *in, unsigned qual_words, uint64_t n, uint32_t *count, float *total_qual, uint64_t *qual) {
    const size_t rsz = kmstat_record_bytes(qual_words);
    for (uint64_t i = 0; i < n; ++i) {
        const char *r = in + i * rsz;
        uint32_t c2;
        memcpy(&c2, r, 4);
        count[i] = c2 >> 1;
        memcpy(&total_qual[i], r + 4, 4);
        memcpy(qual + i * qual_words, r + 8, 8 * (size_t)qual_words);
    }
}

// ---- a cluster listing (<path>: members, <path>.idx: sizes) into the documented order ---------------------------------
// mem (n_mem values, sorted in place cluster by cluster) and sz (C values) as read from the two files of `path`, n the
// k-mers of the set.  Leaves members / labels (n u32) and sizes (C u64) with the members ascending inside a cluster and the
// clusters by ascending smallest member (their label; the reference lists clusters by DSU root, concurrent_dsu.cpp:54-69).
// Returns the empty string, or why the files are refused.
inline std::string hamclusters_normalise(const char *path, uint64_t *mem, size_t n_mem, const uint64_t *sz, size_t C, uint64_t n,
                                         std::vector<uint32_t> &members, std::vector<uint32_t> &labels,
                                         std::vector<uint64_t> &sizes) {
    char msg[1024];
    auto refuse = [&](const char *fmt, auto... a) { return snprintf(msg, sizeof(msg), fmt, a...), std::string(msg); };
    if (n_mem != n) return refuse("%s lists %zu members, the set has %llu k-mers", path, n_mem, (unsigned long long)n);
    uint64_t sum = 0;
    for (size_t c = 0; c < C; ++c) {
        if (sz[c] < 1 || sz[c] > n - sum)
            return refuse("%s.idx: the cluster sizes are not positive numbers that sum to %llu", path, (unsigned long long)n);
        sum += sz[c];
    }
    if (sum != n)
        return refuse("%s.idx: the cluster sizes sum to %llu, not to %llu", path, (unsigned long long)sum, (unsigned long long)n);
    std::vector<uint8_t> seen(n, 0);
    for (size_t i = 0; i < n_mem; ++i) {
        const uint64_t m = mem[i];
        if (m >= n || seen[m])
            return refuse("%s: the members are not a permutation of 0 .. %llu (index %llu is %s)", path, (unsigned long long)n,
                          (unsigned long long)m, m < n ? "listed twice" : "out of range");
        seen[m] = 1;
    }
    std::vector<uint64_t> start(C + 1, 0);
    for (size_t c = 0; c < C; ++c) {
        start[c + 1] = start[c] + sz[c];
        std::sort(mem + start[c], mem + start[c + 1]);
    }
    std::vector<size_t> order(C);
    for (size_t c = 0; c < C; ++c) order[c] = c;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return mem[start[a]] < mem[start[b]]; });
    members.resize(n);
    labels.resize(n);
    sizes.resize(C);
    uint64_t o = 0;
    for (size_t c = 0; c < C; ++c) {
        const size_t src = order[c];
        sizes[c] = sz[src];
        for (uint64_t j = 0; j < sz[src]; ++j) {
            const uint32_t m = (uint32_t)mem[start[src] + j];
            members[o++] = m;
            labels[m] = (uint32_t)mem[start[src]];
        }
    }
    return std::string();
}

}  // namespace bbk
