// Host-only check of csrc/hammer_files.h: the binary_write(KMerStat) record codec and the order a cluster listing is
// brought into.
//   hammer_files_check         prints HAMMER-FILES-OK and exits 0, or says what differed and exits 1
// Codec, for 1, 2 and 3 quality words (k = 10, 11/21, 22/32): 7 records and 2 new k-mers packed in blocks of 1, 4 and 9
// are the bytes of one block of 9; one record of each kind equals a layout written out here by hand; unpacking gives the
// statistics back without the good bit.  Normaliser: one listing of three clusters in two cluster orders with unsorted
// members comes out the same; n = 0 passes; every refusal returns its message.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../spades_for_blackbird_amd/csrc/hammer_files.h"

namespace {

int failures = 0;

void check(bool ok, const char *what, unsigned a = 0, unsigned b = 0) {
    if (!ok && failures++ < 20) std::fprintf(stderr, "%s (%u, %u)\n", what, a, b);
}

void put32(std::vector<char> &v, uint32_t x) {
    for (int i = 0; i < 4; ++i) v.push_back((char)(x >> (8 * i)));  // little-endian, as every target of the library
}
void put64(std::vector<char> &v, uint64_t x) {
    for (int i = 0; i < 8; ++i) v.push_back((char)(x >> (8 * i)));
}

void codec(unsigned qw) {
    const uint64_t n = 7, news = 2, total = n + news;
    const size_t rsz = bbk::kmstat_record_bytes(qw);
    check(rsz == 8 + 8 * qw, "record size", qw);
    std::vector<uint32_t> count(n);
    std::vector<float> tq(n);
    std::vector<uint64_t> qual(n * qw);
    std::vector<uint8_t> good(total);
    for (uint64_t i = 0; i < n; ++i) {
        count[i] = i == 3 ? 0x7FFFFFFFu : (uint32_t)(1000 * i + 1);  // the largest count that fits
        tq[i] = 1.0f / (float)(i + 2);
        for (unsigned w = 0; w < qw; ++w) qual[i * qw + w] = 0x0123456789ABCDEFull * (i + 1) + w;
    }
    for (uint64_t i = 0; i < total; ++i) good[i] = (uint8_t)((i * 5 + 1) % 3 == 0);
    good[n] = 1;  // a good new k-mer, then a bad one
    good[n + 1] = 0;

    std::vector<char> whole(total * rsz, (char)0x5A);
    bbk::kmstat_pack_block(whole.data(), qw, 0, total, n, count.data(), tq.data(), qual.data(), good.data());
    for (uint64_t block : {1, 4, 9}) {
        std::vector<char> parts;
        for (uint64_t b = 0; b < total; b += block) {
            const uint64_t m = total - b < block ? total - b : block;
            const uint64_t old = b < n ? (n - b < m ? n - b : m) : 0;
            // the block's slices, exactly as long as the block reads them: a read past one is AddressSanitizer's to report
            std::vector<uint32_t> c(count.begin() + (b < n ? b : n), count.begin() + (b < n ? b : n) + old);
            std::vector<float> t(tq.begin() + (b < n ? b : n), tq.begin() + (b < n ? b : n) + old);
            std::vector<uint64_t> q(qual.begin() + (b < n ? b : n) * qw, qual.begin() + ((b < n ? b : n) + old) * qw);
            std::vector<uint8_t> g(good.begin() + b, good.begin() + b + m);
            std::vector<char> out(m * rsz, (char)0xA5);
            bbk::kmstat_pack_block(out.data(), qw, b, m, n, c.data(), t.data(), q.data(), g.data());
            parts.insert(parts.end(), out.begin(), out.end());
        }
        check(parts == whole, "blocks differ from one block", qw, (unsigned)block);
    }

    // by hand: record 3 (an old k-mer, good or not as drawn), record 7 (a good new k-mer), record 8 (a bad one)
    std::vector<char> hand;
    put32(hand, (count[3] << 1) | good[3]);
    uint32_t fbits;
    std::memcpy(&fbits, &tq[3], 4);
    put32(hand, fbits);
    for (unsigned w = 0; w < qw; ++w) put64(hand, qual[3 * qw + w]);
    check(std::memcmp(hand.data(), whole.data() + 3 * rsz, rsz) == 0 && hand.size() == rsz, "record of a k-mer", qw);
    check((unsigned char)whole[3 * rsz + 3] == 0xFF, "count 2^31 - 1 fills the word", qw);
    for (uint64_t i = n; i < total; ++i) {
        hand.clear();
        put32(hand, good[i]);         // count 0
        put32(hand, 0x3F800000u);     // 1.0f
        for (unsigned w = 0; w < qw; ++w) put64(hand, 0);
        check(std::memcmp(hand.data(), whole.data() + i * rsz, rsz) == 0, "record of a new k-mer", qw, (unsigned)i);
    }
    // no good bits given: every bit 0 is clear
    std::vector<char> plain(n * rsz);
    bbk::kmstat_pack_block(plain.data(), qw, 0, n, n, count.data(), tq.data(), qual.data(), nullptr);
    for (uint64_t i = 0; i < n; ++i) {
        check((plain[i * rsz] & 1) == 0, "good bit without good bits", qw, (unsigned)i);
        check(std::memcmp(plain.data() + i * rsz + 1, whole.data() + i * rsz + 1, rsz - 1) == 0, "bytes besides the good bit", qw);
    }

    std::vector<uint32_t> c2(n, 77);
    std::vector<float> t2(n, -1.0f);
    std::vector<uint64_t> q2(n * qw, 99);
    bbk::kmstat_unpack(whole.data(), qw, n, c2.data(), t2.data(), q2.data());
    check(c2 == count, "unpacked counts", qw);
    check(std::memcmp(t2.data(), tq.data(), n * 4) == 0, "unpacked total_qual", qw);
    check(q2 == qual, "unpacked quality words", qw);
}

struct Listing {
    std::vector<uint32_t> members, labels;
    std::vector<uint64_t> sizes;
};

std::string normalise(std::vector<uint64_t> mem, const std::vector<uint64_t> &sz, uint64_t n, Listing &out) {
    return bbk::hamclusters_normalise("f", mem.data(), mem.size(), sz.data(), sz.size(), n, out.members, out.labels, out.sizes);
}

void refused(const std::vector<uint64_t> &mem, const std::vector<uint64_t> &sz, uint64_t n, const char *want, const char *also = "") {
    Listing l;
    const std::string err = normalise(mem, sz, n, l);
    if (err.find(want) == std::string::npos || err.find(also) == std::string::npos) {
        std::fprintf(stderr, "expected a refusal with '%s' '%s', got '%s'\n", want, also, err.c_str());
        ++failures;
    }
    check(l.members.empty() && l.labels.empty() && l.sizes.empty(), "a refusal wrote its outputs");
}

void normaliser() {
    // clusters {0, 4, 5}, {1, 3, 6, 7}, {2} of n = 8
    Listing a, b;
    check(normalise({5, 0, 4, 7, 1, 6, 3, 2}, {3, 4, 1}, 8, a).empty(), "first order refused");
    check(normalise({2, 3, 6, 1, 7, 4, 5, 0}, {1, 4, 3}, 8, b).empty(), "second order refused");
    const std::vector<uint32_t> members = {0, 4, 5, 1, 3, 6, 7, 2}, labels = {0, 1, 2, 1, 0, 0, 1, 1};
    const std::vector<uint64_t> sizes = {3, 4, 1};
    for (const Listing *l : {&a, &b}) {
        check(l->members == members, "members");
        check(l->labels == labels, "labels");
        check(l->sizes == sizes, "sizes");
    }
    Listing e;
    check(normalise({}, {}, 0, e).empty() && e.members.empty() && e.labels.empty() && e.sizes.empty(), "n = 0");

    const std::vector<uint64_t> mem = {0, 1, 2, 3, 4};
    refused(mem, {2, 0, 3}, 5, "not positive numbers");                       // a size of 0
    refused(mem, {2, 2}, 5, "sum to 4, not to 5");                            // short
    refused(mem, {2, 2, 2}, 5, "sum to");                                     // long
    refused({0, 1, 2, 1, 4}, {2, 3}, 5, "not a permutation", "listed twice");  // a duplicate
    refused({0, 1, 5, 3, 4}, {2, 3}, 5, "not a permutation", "out of range");  // a member equal to n
    refused(mem, {2, 3}, 6, "lists 5 members");                               // another member count
    refused(mem, {2, 3}, 4, "lists 5 members");
}

}  // namespace

int main() {
    for (unsigned qw : {1u, 2u, 3u}) codec(qw);
    normaliser();
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::puts("HAMMER-FILES-OK");
    return 0;
}
