// Host-only check of the rank-of-a-position helper of the mark-bit scatter tail (csrc/msd_mark_tail.h: MarkWord,
// mark_slot32, mark_bit32, mark_count, mark_rank, view_run_start, view_bucket_live), walked the way the kernels walk it:
// NT lanes, step i of lane t is position i * NT + t, whose word of marks is i * (NT / 64) + wave.
//   mark_tail_check          prints MARK-CHECK-OK and exits 0, or says what differed and exits 1
// Tail form: run tables (records per bin, empty bins among them) -> marks, prefixes, and for EVERY position the rank
// against a naive scan.  View form: bucket offsets with empty buckets -> the bucket of every key position of a tile
// against the largest b with off[b] <= c.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../spades_for_blackbird_amd/csrc/msd_mark_tail.h"

namespace {

constexpr uint32_t NT = 1024;
int failures = 0, cases = 0;

void fail(const char *name, const char *what, uint64_t at, uint64_t a, uint64_t b) {
    if (failures++ < 20) std::fprintf(stderr, "%s: %s at %llu (%llu vs %llu)\n", name, what, (unsigned long long)at, (unsigned long long)a, (unsigned long long)b);
}

// what one wave does after the marks are set: the prefix of every word
void prefixes(std::vector<bbk::MarkWord> &mw) {
    uint32_t before = 0;
    for (auto &w : mw) {
        w.before = before;
        before += bbk::mark_count(w.lo, w.hi);
    }
}

void set_mark(std::vector<bbk::MarkWord> &mw, uint32_t start) {
    uint32_t *w32 = reinterpret_cast<uint32_t *>(mw.data());
    const uint32_t slot = bbk::mark_slot32(start);
    if (slot >= 4 * mw.size() || (slot & 3u) > 1u) {
        fail("set_mark", "slot outside the words", start, slot, 4 * mw.size());
        return;
    }
    w32[slot] |= bbk::mark_bit32(start);
}

// counts[b] records in bin b, staged bin-major; `tile` positions have words (the kernel's LDS layout), staged <= tile
void tail_case(const char *name, const std::vector<uint32_t> &counts, uint32_t tile) {
    ++cases;
    std::vector<uint32_t> owner;  // naive: rank of the non-empty bin that owns each position
    std::vector<bbk::MarkWord> mw(tile / 64, bbk::MarkWord{0, 0, 0, 0xDEADBEEFu});
    uint32_t ex = 0, r = 0;
    for (uint32_t c : counts) {
        if (!c) continue;
        if (ex) set_mark(mw, ex);  // what the bin's thread does: position 0 starts a run without a mark
        owner.insert(owner.end(), c, r++);
        ex += c;
    }
    const uint32_t staged = ex;
    if (staged > tile) {
        fail(name, "case larger than its tile", 0, staged, tile);
        return;
    }
    prefixes(mw);
    uint32_t visited = 0;
    for (uint32_t tid = 0; tid < NT; ++tid) {
        const uint32_t lane = tid & 63u, wave = tid >> 6;
        for (uint32_t i = 0; i * NT + tid < staged; ++i) {
            const uint32_t pos = i * NT + tid;
            const bbk::MarkWord &w = mw.at(i * (NT / 64) + wave);
            const uint32_t got = bbk::mark_rank(w.lo, w.hi, w.before, lane);
            if (got != owner[pos]) fail(name, "rank", pos, got, owner[pos]);
            ++visited;
        }
    }
    if (visited != staged) fail(name, "positions visited", 0, visited, staged);
    if (bbk::mark_words(staged) > mw.size()) fail(name, "mark_words", staged, bbk::mark_words(staged), mw.size());
}

// off[b] = first dense position of bucket b (non-decreasing, off[0] = 0); tile of kpt positions from c0, D keys in all
void view_case(const char *name, const std::vector<uint64_t> &off, uint64_t D, uint64_t c0, uint32_t kpt) {
    ++cases;
    const uint32_t nb = (uint32_t)off.size();
    auto bucket_of = [&](uint64_t c) {
        uint32_t b = 0;
        for (uint32_t q = 0; q < nb; ++q)
            if (off[q] <= c) b = q;
        return b;
    };
    const uint32_t n = (uint32_t)(D - c0 < kpt ? D - c0 : kpt);
    const uint32_t b0 = bucket_of(c0), b1 = bucket_of(c0 + n - 1), span = b1 - b0 + 1;
    std::vector<bbk::MarkWord> mw(kpt / 64, bbk::MarkWord{0, 0, 0, 0xDEADBEEFu});
    std::vector<uint32_t> list;  // the r-th live bucket of the span
    for (uint32_t i = 0; i < span; ++i) {
        const uint64_t o = off[b0 + i], on = i + 1 < span ? off[b0 + i + 1] : 0;
        if (!bbk::view_bucket_live(i, span, o, on)) continue;
        list.push_back(i);
        const uint32_t start = bbk::view_run_start(o, c0);
        if (start) set_mark(mw, start);
        else if (i) fail(name, "a later bucket starts at 0", i, o, c0);
    }
    prefixes(mw);
    for (uint32_t cl = 0; cl < kpt; ++cl) {  // every lane of the tile, the ones past its last key included
        const bbk::MarkWord &w = mw.at(cl >> 6);
        const uint32_t r = bbk::mark_rank(w.lo, w.hi, w.before, cl & 63u);
        if (r >= list.size()) {
            fail(name, "rank past the list", cl, r, list.size());
            continue;
        }
        const uint32_t want = bucket_of(c0 + (cl < n ? cl : n - 1));
        if (b0 + list[r] != want) fail(name, "bucket", cl, b0 + list[r], want);
    }
}

std::vector<uint32_t> repeat(std::initializer_list<uint32_t> pattern, uint32_t total) {
    std::vector<uint32_t> v;
    uint32_t sum = 0;
    while (sum < total)
        for (uint32_t c : pattern) {
            if (sum + c > total) c = total - sum;
            if (c) v.push_back(c);
            sum += c;
            if (sum == total) break;
        }
    return v;
}

}  // namespace

int main() {
    const uint32_t T = 14336;  // 1024 lanes x 14 records: 224 words
    tail_case("single run", {T}, T);
    tail_case("single record", {1}, T);
    tail_case("1024 runs of one record", std::vector<uint32_t>(1024, 1), T);
    tail_case("1024 runs of one record, empty bins between", repeat({1, 0, 0}, 1024), T);
    tail_case("a run starts at 64 w for every w", repeat({64}, T), T);
    tail_case("runs end at 64 w - 1 and start inside the word", repeat({10, 54}, T), T);
    tail_case("a run starts at 64 w + 1 for every w", repeat({1, 64}, T), T);
    tail_case("a run starts at 64 w - 1 for every w", repeat({63, 64}, T), T);
    tail_case("runs of 65 and 129: words without a mark", repeat({65, 129, 3, 200, 1}, T), T);
    tail_case("one run longer than 128 between short ones", {5, 0, 300, 7, 0, 0, 1000, 2}, T);
    tail_case("last word filled to 1", repeat({14}, 64 * 100 + 1), T);
    tail_case("last word filled to 63", repeat({14}, 64 * 100 + 63), T);
    tail_case("last word filled to 1 by a run of its own", {6400, 1}, T);
    tail_case("runs of 14 (the flagship's)", repeat({14}, T), T);
    tail_case("the narrow tile: 15360 positions in 240 words", repeat({15}, 15360), 15360);
    tail_case("the payload tile: 8192 positions", repeat({8, 1, 120}, 8192), 8192);

    const uint32_t KPT = 7168;  // the keys of a level-1 tile of stage B: 112 words
    // ~700 keys per bucket, as at the flagship size
    std::vector<uint64_t> plain;
    for (uint64_t o = 0; o < 40000; o += 690) plain.push_back(o);
    for (uint64_t c0 = 0; c0 < 40000; c0 += KPT) view_case("plain buckets", plain, 40000, c0, KPT);
    view_case("plain buckets, a last tile of one key", plain, 5 * (uint64_t)KPT + 1, 5 * (uint64_t)KPT, KPT);
    // empty buckets at the front (of the table and of a tile), in the middle, doubled and at the end
    const std::vector<uint64_t> holes = {0, 0, 0, 500, 900, 900, 1300, 1300, 1300, 2000, 7168, 7168, 7200, 9000, 9000, 14336, 14336, 14400, 14400, 14400};
    view_case("empty buckets, tile 0", holes, 14400, 0, KPT);
    view_case("empty buckets, tile 1 starts on a doubled offset", holes, 14400, KPT, KPT);
    view_case("empty buckets, last tile of 64 keys", holes, 14400, 2 * (uint64_t)KPT, KPT);
    view_case("one bucket for the whole tile", {0, 0, 100000}, 50000, KPT, KPT);
    std::vector<uint64_t> crowded;  // 64 live buckets in one tile, starts on and around word boundaries
    for (uint64_t i = 0; i < 64; ++i) crowded.push_back(i * 112 + (i % 3 == 0 ? 0 : i % 3 == 1 ? 63 : 1) * (i > 0));
    view_case("64 buckets in a tile", crowded, 7168, 0, KPT);
    std::vector<uint64_t> ones = {0};  // buckets of one key each at the tile's head, then the rest
    for (uint64_t i = 1; i < 40; ++i) ones.push_back(i);
    view_case("buckets of one key", ones, 7000, 0, KPT);

    if (failures) {
        std::fprintf(stderr, "%d failures in %d cases\n", failures, cases);
        return 1;
    }
    std::printf("MARK-CHECK-OK %d cases\n", cases);
    return 0;
}
