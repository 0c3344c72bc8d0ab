// Host-only check of the copy-out step of k_bucket_dist_nb (csrc/msd_bucket_tail.h: dist_tail_at, bucket_rows), walked
// the way the kernel walks it: NT lanes, row i of lane t is position i * NT + t, rows bounded by bucket_rows(n, NT).
//   bucket_tail_check          prints TAIL-CHECK-OK and exits 0, or says what differed and exits 1
// Sorted buckets of n in {1, 2, 511, 512, 513, 4096, 5631, 5632} offsets, without a duplicate and with one duplicate
// pair at the first, a middle and the last position: the verdict must be raised exactly when a pair exists, and without
// one every dst[s], s < n, must be (base + key[s]) & mask, with nothing stored outside [0, n).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../spades_for_blackbird_amd/csrc/msd_bucket_tail.h"

namespace {

constexpr uint32_t NT = 512, ITEMS = 11;
constexpr uint64_t kGuard = 0xA5A5A5A5A5A5A5A5ull;

int failures = 0;

void fail(const char *what, uint32_t n, int dup_at, uint64_t a, uint64_t b) {
    if (failures++ < 20) std::fprintf(stderr, "n=%u dup_at=%d: %s (%llx vs %llx)\n", n, dup_at, what, (unsigned long long)a, (unsigned long long)b);
}

// strictly ascending offsets that reach the top of the 32-bit range (the sum base + offset then carries into bit 32)
std::vector<uint32_t> ascending(uint32_t n, uint64_t seed) {
    std::vector<uint32_t> v(n);
    const uint64_t step = (0xFFFFFFFFull - 7) / (n ? n : 1);
    uint64_t x = 0;
    for (uint32_t i = 0; i < n; ++i) {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        x += 1 + (step > 1 ? (seed >> 33) % step : 0);
        v[i] = (uint32_t)x;
    }
    if (n) v[n - 1] = 0xFFFFFFFFu;  // every offset is a possible value
    return v;
}

void run_case(uint32_t n, int dup_at, uint64_t base, uint64_t mask) {
    std::vector<uint32_t> keys = ascending(n, 17 * n + 3);
    if (dup_at >= 0) keys[dup_at + 1] = keys[dup_at];  // the pair (dup_at, dup_at + 1); the order stays ascending
    // LDS holds CAP words: whatever lies past n is not the bucket's and must not be looked at
    std::vector<uint32_t> lds(NT * ITEMS, 0xDEADBEEFu);
    for (uint32_t i = 0; i < n; ++i) lds[i] = keys[i];
    if (n < NT * ITEMS && n > 0) lds[n] = keys[n - 1];  // a stale equal word right behind the bucket is no duplicate
    std::vector<uint64_t> dst((size_t)n + 2, kGuard);   // dst[0] and dst[n + 1] are guards
    const uint32_t rows = bbk::bucket_rows(n, NT);
    if (rows != (n + NT - 1) / NT || rows > ITEMS) fail("rows", n, dup_at, rows, (n + NT - 1) / NT);
    bool verdict = false;
    uint32_t visited = 0;
    for (uint32_t tid = 0; tid < NT; ++tid)
        for (uint32_t i = 0; i < ITEMS; ++i)
            if (i < rows) {
                const uint32_t s = i * NT + tid;
                if (s < n) {
                    verdict = bbk::dist_tail_at(lds.data(), s, base, mask, dst.data() + 1) || verdict;
                    ++visited;
                }
            }
    if (visited != n) fail("positions visited", n, dup_at, visited, n);
    if (verdict != (dup_at >= 0)) fail("verdict", n, dup_at, verdict, dup_at >= 0);
    if (dst[0] != kGuard || dst[(size_t)n + 1] != kGuard) fail("store outside [0, n)", n, dup_at, dst[0], dst[(size_t)n + 1]);
    if (dup_at < 0)
        for (uint32_t s = 0; s < n; ++s)
            if (dst[s + 1] != ((base + keys[s]) & mask)) fail("dst[s]", n, dup_at, dst[s + 1], (base + keys[s]) & mask);
}

}  // namespace

int main() {
    const uint32_t sizes[] = {1, 2, 511, 512, 513, 4096, 5631, 5632};
    // (base, mask): a tagged k = 17 key space (tag above bit 34, stripped on the way out), and no mask at all
    const uint64_t forms[][2] = {{(5ull << 34) | 0x2FFFFFF00ull, (1ull << 34) - 1}, {0x123456789ABCull, ~0ull}, {0, ~0ull}};
    int cases = 0;
    for (uint32_t n : sizes)
        for (const auto &f : forms) {
            run_case(n, -1, f[0], f[1]);
            ++cases;
            if (n < 2) continue;
            const int at[] = {0, (int)(n / 2) - 1 < 0 ? 0 : (int)(n / 2) - 1, (int)n - 2};
            for (int d : at) {
                run_case(n, d, f[0], f[1]);
                ++cases;
            }
        }
    if (failures) {
        std::fprintf(stderr, "%d failures in %d cases\n", failures, cases);
        return 1;
    }
    std::printf("TAIL-CHECK-OK %d cases\n", cases);
    return 0;
}
