// hammer_reads.hpp -- which k-mer positions of a read BayesHammer's KMerDataFiller pushes (host side of
// spades-kmerdata; no GPU needed).  The two rules are restated literally, quirks included, without the probabilities
// (those are the device's):
//   Read::trimNsAndBadQuality / trimLeftRight   common/io/reads/read.hpp:87-122
//   ValidKMerGenerator<K>(read, 2)              projects/hammer/valid_kmer_generator.hpp:147-199
//   KMerDataFiller::operator()                  projects/hammer/kmer_data.cpp:163-186
// Consecutive valid starts a..b are handed out as one stretch [a, b + k) of the read: a stretch holds no character other
// than ACGT (every window the generator yields is checked base by base), and its k-mer positions are exactly the valid
// starts a..b -- so one stretch is one read of the engine, for bbk_count_push_* and bbk_kmerstats_push alike.
//   Read::print's ltrim_ / rtrim_ (trim_ns_and_bad_quality), for spades-kmerdata --correct   common/io/reads/read.hpp:221-236
//   Expander::operator()                        projects/hammer/expander.cpp:20-51
// A read can pass the Expander's coverage test only when the windows the generator yields cover the whole trimmed read
// [0, sz): every window is free of non-ACGT, and a start is skipped only in the search branch, which a non-nucleotide
// enters -- so the read is ONE stretch that is the trimmed read itself (expander_candidate).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace bbkhost {
namespace hammer {

inline bool is_nucl(char c) {  // common/sequence/nucl.hpp:45-62
    switch (c) {
        case 'A': case 'C': case 'G': case 'T':
        case 'a': case 'c': case 'g': case 't':
            return true;
        default:
            return false;
    }
}

struct Stretch {
    uint32_t start, length;  // in the read as parsed
};

// Read::trimNsAndBadQuality(threshold) with the bookkeeping Read::print needs (read.hpp:87-122, 221-236): the read that is
// left is [start, start + length) of the read as parsed (length 0: nothing is left, and ltrim_ / rtrim_ stay 0 /
// initial_size_ as trimLeftRight leaves them when it empties the read).
struct Trim {
    uint32_t start = 0, length = 0;
    int ltrim_ = 0, rtrim_ = 0, initial_size_ = 0;
};
inline Trim trim_ns_and_bad_quality(const std::string &seq_, const std::string &qual_, int threshold) {
    Trim t;
    t.rtrim_ = t.initial_size_ = (int)seq_.size();
    int start = 0;
    for (; start < (int)seq_.size(); ++start) {
        if (seq_[start] != 'N' && (int)qual_[start] > threshold) break;
    }
    int end = 0;
    for (end = (int)seq_.size() - 1; end > -1; --end) {
        if (seq_[end] != 'N' && (int)qual_[end] > threshold) break;
    }
    const int ltrim = start, rtrim = end;
    if (ltrim >= (int)seq_.size() || rtrim < 0 || rtrim < ltrim) return t;
    int size = (int)seq_.size();
    if (ltrim > 0) {
        t.ltrim_ += ltrim;
        size -= ltrim;
    }
    if (rtrim - ltrim + 1 < size && rtrim < size - ltrim - 1) {  // `size` after the left erase: the bad tail can stay
        t.rtrim_ -= size - (rtrim - ltrim + 1);
        size = rtrim - ltrim + 1;
    }
    t.start = (uint32_t)ltrim;
    t.length = (uint32_t)size;
    return t;
}

// ValidKMerGenerator<k>(seq, qual, len, 2) over a read that is trimmed already: the valid k-mer starts, consecutive ones as
// one stretch, appended to out with `origin` added to every start; returns how many stretches.  is_nucleotide: which bytes
// the generator takes for nucleotides.  (Trimming twice is not the same as trimming once -- a bad tail that a left trim
// kept would go -- so a caller that holds trimmed reads, as ReadCorrector does, uses this and not trimmed_stretches.)
template <class IsNucl>
inline size_t generator_stretches(const char *seq_, const char *qual_, size_t len_, unsigned k, uint32_t origin,
                                  std::vector<Stretch> &out, IsNucl is_nucleotide) {
    // ---- Reset = TrimBadQuality + Next ----
    const uint8_t bad_quality_threshold_ = 2;
    auto GetQual = [&](uint32_t pos) -> uint8_t { return pos >= len_ ? 2 : (uint8_t)qual_[pos]; };
    size_t pos_ = 0, end_ = 0;
    for (; pos_ < len_; ++pos_) {
        if (GetQual((uint32_t)pos_) >= bad_quality_threshold_) break;
    }
    end_ = len_;
    for (; end_ > pos_; --end_) {
        if (GetQual((uint32_t)(end_ - 1)) >= bad_quality_threshold_) break;
    }
    bool has_more_ = true, first = true;
    size_t kmer_start = 0;  // start of the current k-mer: pos() - 1
    auto Next = [&] {
        if (pos_ + k > end_) {
            has_more_ = false;
        } else if (first || !is_nucleotide(seq_[pos_ + k - 1])) {
            // looks for a new k-mer up to len_ (not end_) and does not check the window it finds against end_
            uint32_t start_hypothesis = (uint32_t)pos_;
            uint32_t i = (uint32_t)pos_;
            for (; i < len_; ++i) {
                if (i == k + start_hypothesis) break;
                if (!is_nucleotide(seq_[i])) start_hypothesis = i + 1;
            }
            if (i == k + start_hypothesis) {
                kmer_start = start_hypothesis;
                pos_ = start_hypothesis + 1;
            } else {
                has_more_ = false;
            }
        } else {
            kmer_start = pos_;
            ++pos_;
        }
        first = false;
    };
    Next();
    size_t added = 0;
    bool open = false;
    while (has_more_) {
        const uint32_t s = (uint32_t)(origin + kmer_start);
        if (open && out.back().start + out.back().length - k + 1 == s) {
            ++out.back().length;
        } else {
            out.push_back({s, k});
            open = true;
            ++added;
        }
        Next();
    }
    return added;
}

// seq / qual: the read as parsed, qualities with the offset already subtracted (Read's qual_ is a string of char).
// Appends the stretches of the read to out; returns how many.  *trimmed (may be null): the read trimNsAndBadQuality
// leaves, as a range of the read as parsed -- written only when it has k bases or more (the generator ran).
inline size_t trimmed_stretches(const std::string &seq_in, const std::string &qual_in, unsigned k, int trim_quality,
                                std::vector<Stretch> &out, Stretch *trimmed) {
    // ---- Read::trimNsAndBadQuality(trim_quality) on a copy (kmer_data.cpp:167-171) ----
    std::string seq_ = seq_in, qual_ = qual_in;
    int start = 0;
    for (; start < (int)seq_.size(); ++start) {
        if (seq_[start] != 'N' && (int)qual_[start] > trim_quality) break;
    }
    int end = 0;
    for (end = (int)seq_.size() - 1; end > -1; --end) {
        if (seq_[end] != 'N' && (int)qual_[end] > trim_quality) break;
    }
    {  // trimLeftRight(ltrim = start, rtrim = end)
        const int ltrim = start, rtrim = end;
        if (ltrim >= (int)seq_.size() || rtrim < 0 || rtrim < ltrim) return 0;  // nothing left
        if (ltrim > 0) {
            seq_.erase(0, ltrim);
            qual_.erase(0, ltrim);
        }
        // seq_.size() is the size AFTER the left erase: with ltrim > 0 the second test can fail for an rtrim that is
        // before the end, and the bad tail stays
        if (rtrim - ltrim + 1 < (int)seq_.size() && rtrim < (int)seq_.size() - ltrim - 1) {
            seq_.erase(rtrim - ltrim + 1, std::string::npos);
            qual_.erase(rtrim - ltrim + 1, std::string::npos);
        }
    }
    if (seq_.size() < k) return 0;  // sz < hammer::K
    if (trimmed) *trimmed = {(uint32_t)start, (uint32_t)seq_.size()};
    // ---- ValidKMerGenerator<k>(cr, 2), starts back in the read as parsed ----
    return generator_stretches(seq_.data(), qual_.data(), seq_.size(), k, (uint32_t)start, out, is_nucl);
}

inline size_t valid_stretches(const std::string &seq, const std::string &qual, unsigned k, int trim_quality,
                              std::vector<Stretch> &out) {
    return trimmed_stretches(seq, qual, k, trim_quality, out, nullptr);
}

// Whether Expander::operator() can ever find the read solid: its valid k-mer starts are consecutive from the first base
// of the trimmed read to its last k-mer.  *stretch is then the trimmed read, one read of the engine for
// bbk_expander_push.  Every other read returns before it marks anything, whatever the good bits are: one with an interior
// N, one whose q < 2 tail survived the trimming (end_ stops before sz), one with fewer than k bases left.
inline bool expander_candidate(const std::string &seq, const std::string &qual, unsigned k, int trim_quality,
                               Stretch *stretch) {
    std::vector<Stretch> st;
    Stretch trimmed = {0, 0};
    if (trimmed_stretches(seq, qual, k, trim_quality, st, &trimmed) != 1) return false;
    if (st[0].start != trimmed.start || st[0].length != trimmed.length) return false;
    *stretch = trimmed;
    return true;
}

}  // namespace hammer
}  // namespace bbkhost
