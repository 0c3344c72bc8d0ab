// readcorrect_host.hpp -- BayesHammer's ReadCorrector restated literally for the host: no
// HIP, no engine.  It is the path of readcorrect.hip for the searches that outgrow the device's fixed capacities, and what
// the CPU tests hold against tests/readcorrect_restated.py.
//   state, std::less<state>, FlushCandidates   projects/hammer/read_corrector.cpp:22-64
//   ReadCorrector::CorrectReadRight            projects/hammer/read_corrector.cpp:66-158
//   ReadCorrector::CorrectOneRead              projects/hammer/read_corrector.cpp:160-245
// The queues are std::priority_queue with the reference's comparator: which of two states of equal (penalty, pos) comes
// out first is libstdc++'s push_heap / pop_heap, and it decides the corrected read.  Penalties are sums of small
// integers, kept in int: `penalty < -(n * 15.0 / 100)` is `100 * penalty < -15 * n`.
// A k-mer is the engine's one-word key (base i in bits [2i, 2i + 2), A=0 C=1 G=2 T=3, k <= 32); `lookup(key)` gives its
// index in the set or kNone, good[index] its good byte.  A byte other than A, C, G, T is a non-nucleotide.  qual: one
// byte per base, the offset already subtracted.
#pragma once

#include <array>
#include <cmath>
#include <cstdint>
#include <queue>
#include <string>
#include <vector>

#include "../host/hammer_reads.hpp"

namespace bbkhost {
namespace readcorrect {

constexpr uint64_t kNone = ~0ull;

inline bool is_nucl(char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
inline unsigned dignucl(char c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : 3u; }
inline char nucl(unsigned d) { return "ACGT"[d]; }
inline char nucl_complement(char c) { return is_nucl(c) ? nucl(3u - dignucl(c)) : c; }  // N stays N

inline std::string ReverseComplement(const std::string &s) {
    std::string r(s.size(), 0);
    for (size_t i = 0; i < s.size(); ++i) r[s.size() - 1 - i] = nucl_complement(s[i]);
    return r;
}
inline std::string Reverse(const std::string &s) { return std::string(s.rbegin(), s.rend()); }

// KMer(seq, start, k, raw) and operator<<
inline uint64_t kmer_at(const std::string &s, size_t start, unsigned k) {
    uint64_t v = 0;
    for (unsigned i = 0; i < k; ++i) v |= (uint64_t)dignucl(s[start + i]) << (2 * i);
    return v;
}
inline uint64_t kmer_shift(uint64_t last, unsigned c, unsigned k) { return (last >> 2) | ((uint64_t)c << (2 * (k - 1))); }

// CorrectReadRight's size_thr for n = read_size - right_pos
inline size_t size_threshold(size_t n) { return size_t(100 * log2((double)n)) + 1; }

using positions_t = std::array<uint16_t, 4>;

struct state {
    state(size_t p, std::string s, int pen, uint64_t l, positions_t c) : pos(p), str(std::move(s)), penalty(pen), last(l), cpos(c) {}
    size_t pos;
    std::string str;
    int penalty;
    uint64_t last;
    positions_t cpos;
};

struct state_less {
    bool operator()(const state &lhs, const state &rhs) const {
        return lhs.penalty < rhs.penalty || (lhs.penalty == rhs.penalty && lhs.pos < rhs.pos);
    }
};
using queue_t = std::priority_queue<state, std::vector<state>, state_less>;

struct Counters {
    uint64_t changed_reads = 0, changed_nucleotides = 0, uncorrected_nucleotides = 0, total_nucleotides = 0;
};

// what a search took: the figures of the device's capacity rule
struct SearchFigures {
    uint64_t pops = 0, max_heap = 1;
    bool failed = false;
};

inline void FlushCandidates(queue_t &corrections, queue_t &candidates, size_t size_limit, SearchFigures &fig) {
    if (candidates.empty()) return;

    if (corrections.size() > size_limit) {
        corrections.emplace(candidates.top());
    } else {
        while (!candidates.empty()) {
            corrections.emplace(candidates.top());
            candidates.pop();
        }
    }
    if (corrections.size() > fig.max_heap) fig.max_heap = corrections.size();

    queue_t().swap(candidates);
}

// the corrected read, or seq itself when the search fails (fig->failed; the caller adds read_size - right_pos to
// uncorrected_nucleotides)
template <class Lookup>
std::string CorrectReadRight(const std::string &seq, const std::string &qual, size_t right_pos, unsigned K, Lookup &&lookup,
                             const uint8_t *good, SearchFigures *figures) {
    SearchFigures local, &fig = figures ? *figures : local;
    fig = SearchFigures();
    const size_t read_size = seq.size();
    queue_t corrections, candidates;
    positions_t cpos{{(uint16_t)-1, (uint16_t)-1U, (uint16_t)-1U, (uint16_t)-1U}};

    const size_t size_thr = size_threshold(read_size - right_pos);
    const long long n = (long long)(read_size - right_pos);
    const size_t pos_thr = 8;

    corrections.emplace(right_pos, seq, 0, kmer_at(seq, right_pos - K + 1, K), cpos);
    while (!corrections.empty()) {
        state correction = corrections.top();
        corrections.pop();
        ++fig.pops;
        size_t pos = correction.pos + 1;
        if (pos == read_size) return correction.str;

        char c = correction.str[pos];
        const int q = (unsigned char)qual[pos];

        // See, whether it's enough to perform single nucl extension
        bool extended = false;
        if (is_nucl(c)) {
            uint64_t last = kmer_shift(correction.last, dignucl(c), K);
            uint64_t idx = lookup(last);
            if (idx != kNone) {
                const bool g = good[idx] != 0;
                candidates.emplace(pos, correction.str, correction.penalty - (g ? 0 : (q >= 20 ? 1 : 2)), last, cpos);
                if (g && q >= 20) extended = true;
            } else {
                candidates.emplace(pos, correction.str, correction.penalty - (q >= 20 ? 2 : 3), last, cpos);
            }
        }

        // Ok, it's possible to extend using solely solid k-mer, do not try any other corrections.
        if (extended) {
            FlushCandidates(corrections, candidates, size_thr, fig);
            continue;
        }

        // Do not allow too many corrections
        if (100ll * correction.penalty < -15ll * n) {
            FlushCandidates(corrections, candidates, size_thr, fig);
            continue;
        }

        // Do not allow clustered corrections
        if (pos - correction.cpos.front() < pos_thr) {
            FlushCandidates(corrections, candidates, size_thr, fig);
            continue;
        }

        // Try corrections (this cpos shadows the outer one, as in the reference)
        {
            positions_t cpos = correction.cpos;
            std::copy(cpos.begin() + 1, cpos.end(), cpos.begin());
            cpos.back() = (uint16_t)pos;
            for (unsigned cc = 0; cc < 4; ++cc) {
                char ncc = nucl(cc);
                if (c == ncc) continue;

                uint64_t last = kmer_shift(correction.last, cc, K);
                uint64_t idx = lookup(last);
                if (idx == kNone) continue;

                if (good[idx] != 0) {
                    std::string corrected = correction.str;
                    corrected[pos] = ncc;
                    int penalty = correction.penalty - (is_nucl(c) ? (q >= 20 ? 5 : 1) : 0);
                    candidates.emplace(pos, corrected, penalty, last, cpos);
                }
            }
        }

        FlushCandidates(corrections, candidates, size_thr, fig);
    }

    fig.failed = true;
    return seq;
}

// The longest solid island of CorrectOneRead (:167-196) over the generator's valid starts, given as stretches of the
// read: solid_len 0 when no start is good.
template <class Lookup>
void solid_island(const std::string &seq, const std::vector<hammer::Stretch> &stretches, unsigned K, Lookup &&lookup,
                  const uint8_t *good, size_t *lleft, size_t *lright, size_t *solid_len_out) {
    size_t lleft_pos = -1ULL, lright_pos = -1ULL, solid_len = 0;
    size_t left_pos = 0, right_pos = 0;
    for (const hammer::Stretch &st : stretches) {
        for (size_t read_pos = st.start; read_pos + K <= (size_t)st.start + st.length; ++read_pos) {
            uint64_t idx = lookup(kmer_at(seq, read_pos, K));
            if (idx != kNone && good[idx] != 0) {
                if (read_pos != right_pos - K + 2) {
                    left_pos = read_pos;
                    right_pos = left_pos + K - 1;
                } else
                    right_pos += 1;

                if (right_pos - left_pos + 1 > solid_len) {
                    lleft_pos = left_pos;
                    lright_pos = right_pos;
                    solid_len = right_pos - left_pos + 1;
                }
            }
        }
    }
    *lleft = lleft_pos;
    *lright = lright_pos;
    *solid_len_out = solid_len;
}

// CorrectOneRead on a read of K bases or more: seq is replaced by the corrected read; returns the result flag.
// searches (may be null): the figures of the right and of the left search, when they ran.
template <class Lookup>
bool CorrectOneRead(std::string &seq_io, const std::string &qual, unsigned K, Lookup &&lookup, const uint8_t *good,
                    Counters &cnt, std::vector<SearchFigures> *searches = nullptr) {
    const std::string seq = seq_io;
    const size_t read_size = seq.size();

    std::vector<hammer::Stretch> stretches;
    hammer::generator_stretches(seq.data(), qual.data(), read_size, K, 0, stretches, is_nucl);
    size_t lleft_pos, lright_pos, solid_len;
    solid_island(seq, stretches, K, lookup, good, &lleft_pos, &lright_pos, &solid_len);

    cnt.total_nucleotides += read_size;

    if (solid_len && solid_len != read_size) {
        SearchFigures fr, fl;
        std::string newseq = CorrectReadRight(seq, qual, lright_pos, K, lookup, good, &fr);
        if (fr.failed) cnt.uncorrected_nucleotides += read_size - lright_pos;
        newseq = ReverseComplement(
            CorrectReadRight(ReverseComplement(newseq), Reverse(qual), read_size - 1 - lleft_pos, K, lookup, good, &fl));
        if (fl.failed) cnt.uncorrected_nucleotides += read_size - (read_size - 1 - lleft_pos);
        if (searches) {
            searches->push_back(fr);
            searches->push_back(fl);
        }

        unsigned corrected = 0;
        for (size_t i = 0; i < read_size; ++i) corrected += seq[i] != newseq[i];

        if (corrected) {
            cnt.changed_reads += 1;
            cnt.changed_nucleotides += corrected;
        }
        seq_io = newseq;
        return true;
    }
    return solid_len == read_size;
}

}  // namespace readcorrect
}  // namespace bbkhost
