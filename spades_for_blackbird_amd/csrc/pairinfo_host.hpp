// pairinfo_host.hpp -- the host arithmetic of the paired stage (csrc/pairinfo.hip, csrc/distest.hip) as plain C++, next to
// the kernels as distest_host.hpp and readcorrect_host.hpp are: standard headers only (no HIP, no bbk_internal.h), so a
// stand-alone program builds it with g++ alone (tests/pairinfo_host_check.cpp).
//
//   lib_statistics             find_mean / find_median / GetISInterval (common/paired_info/insert_size_refiner.hpp:23-166)
//                              in doubles, line by line, in the order CollectLibInformation calls them
//                              (projects/spades/pair_info_count.cpp:227-242)
//   pi_round                   the rounding of pair_info_filler.hpp:84-85, shared with k_pi_pairs
//   math_ge, least_half_units  PairInfoWeightChecker's comparison (pair_info_filters.hpp:42-56) as a threshold in half-units
//   PairPoints                 the raw point table of a library: ascending (e1, e2, gap), equal points summed
//   canonical_points           what bbk_pairinfo_import leaves of host points
//   pair_groups                the pairs and the first edges of the ascending points
//   uleb128, write_paired_index  PairedBuffer::BinWrite (paired_info_buffer.hpp:197-210), the one writer of both indices
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "edge_ops.h"

namespace bbk {

// ---- statistics (doubles; insert_size_refiner.hpp line by line) ---------------------------------------------------------

typedef std::map<int, uint64_t> HistType;

inline double get_median(const HistType &hist) {
    double S = 0;
    for (auto it = hist.begin(); it != hist.end(); ++it) S += (double)it->second;
    double sum = S;
    for (auto it = hist.begin(); it != hist.end(); ++it) {
        sum -= (double)it->second;
        if (sum <= S / 2) return it->first;
    }
    return -1;
}

// math::round_to_zero (math/xmath.h:330-340); the medians it is given are histogram keys
inline int round_to_zero(double t) {
    const int res = (int)std::floor(std::fabs(t) + 0.5);
    return t < 0 ? -res : res;
}

inline double get_mad(const HistType &hist, double median) {
    HistType hist2;
    for (auto it = hist.begin(); it != hist.end(); ++it) hist2[std::abs(it->first - round_to_zero(median))] = it->second;
    return get_median(hist2);
}

inline void hist_crop(const HistType &hist, double low, double high, HistType &res) {
    for (auto it = hist.begin(); it != hist.end(); ++it)
        if (it->first >= low && it->first <= high) res.insert(*it);
}

inline std::pair<double, double> get_is_interval(double quantile, const HistType &is_hist) {
    double S = 0;
    for (const auto &kv : is_hist) S += (double)kv.second;
    const double lval = S * (1 - quantile) / 2, rval = S * (1 + quantile) / 2;
    double is_min = is_hist.begin()->first, is_max = is_hist.rbegin()->first;
    double cS = 0;
    for (const auto &kv : is_hist) {
        if (cS <= lval) is_min = kv.first;
        else if (cS <= rval) is_max = kv.first;
        cS += (double)kv.second;
    }
    return {is_min, is_max};
}

inline void find_median(const HistType &hist, double &median, double &mad, HistType &cropped) {
    median = get_median(hist);
    mad = get_mad(hist, median);
    const double low = median - 5. * 1.4826 * mad;
    const double high = median + 5. * 1.4826 * mad;
    hist_crop(hist, low, high, cropped);
    median = get_median(cropped);
    mad = get_mad(cropped, median);
}

inline void moments(const HistType &hist, double low, double high, uint64_t &n, double &mean, double &delta) {
#ifdef __clang__  // (g++ knows no such pragma; it has no fused multiply-add to contract to on plain x86-64)
#pragma STDC FP_CONTRACT OFF
#endif
    n = 0;
    double sum = 0., sum2 = 0.;
    for (auto it = hist.begin(); it != hist.end(); ++it) {
        if (it->first < low || it->first > high) continue;
        n += it->second;
        sum += (double)it->second * 1. * (double)it->first;
        sum2 += (double)it->second * 1. * (double)it->first * (double)it->first;
    }
    mean = sum / (double)n;
    delta = sqrt(sum2 / (double)n - mean * mean);
}

inline void find_mean(const HistType &hist, double &mean, double &delta, uint64_t percentiles[19]) {
#ifdef __clang__  // (g++ knows no such pragma; it has no fused multiply-add to contract to on plain x86-64)
#pragma STDC FP_CONTRACT OFF
#endif
    const double median = get_median(hist);
    const double mad = get_mad(hist, median);
    double low = median - 5. * 1.4826 * mad;
    double high = median + 5. * 1.4826 * mad;
    uint64_t n;
    moments(hist, low, high, n, mean, delta);
    low = mean - 5 * delta;
    high = mean + 5 * delta;
    moments(hist, low, high, n, mean, delta);
    uint64_t m = 0;
    for (auto it = hist.begin(); it != hist.end(); ++it) {
        if (it->first < low || it->first > high) continue;
        const uint64_t mm = m + it->second;
        for (unsigned i = 0; i < 19; ++i) {
            const uint64_t scaled = (uint64_t)((double)(5 * (i + 1)) / 100. * (double)n);
            if (m < scaled && mm >= scaled) percentiles[i] = (uint64_t)it->first;
        }
        m = mm;
    }
}

// CollectLibInformation (pair_info_count.cpp:231-242) over a histogram that is not empty, into the zeroed fields of *st
// (bbk_pairinfo_stats, or a stand-alone program's own struct of the same names)
template <class Stats>
inline void lib_statistics(const HistType &hist, unsigned k, Stats *st) {
    HistType cropped;
    find_mean(hist, st->mean, st->deviation, st->percentiles);
    find_median(hist, st->median, st->mad, cropped);
    if (st->median < (double)(k + 2)) return;
    std::tie(st->left_quantile, st->right_quantile) = get_is_interval(0.8, cropped);
    st->ok = !cropped.empty();
}

// ---- points -------------------------------------------------------------------------------------------------------------

// int(std::round(d / double(r))) * r (pair_info_filler.hpp:84-85) in integers: half away from zero
BBK_HOST_DEVICE inline int32_t pi_round(int32_t d, uint32_t r) {
    const uint64_t ad = d < 0 ? (uint64_t)(-(int64_t)d) : (uint64_t)d;
    const uint32_t q = (uint32_t)((2 * ad + r) / (2 * (uint64_t)r));
    const uint32_t m = q * r;
    return (int32_t)(d < 0 ? 0u - m : m);
}

// the raw paired index of a library: ascending (e1, e2, gap), every pair under its canonical form, equal points summed
struct PairPoints {
    std::vector<uint64_t> e1, e2;
    std::vector<int32_t> gap;
    std::vector<uint64_t> weight;
    uint64_t size() const { return e1.size(); }
    void resize(uint64_t n) {
        e1.resize(n);
        e2.resize(n);
        gap.resize(n);
        weight.resize(n);
    }
};

// host points (edges that exist) -> the table: canonicalise, sort, merge equal points
inline PairPoints canonical_points(uint64_t n, const uint64_t *e1, const uint64_t *e2, const int32_t *gap, const uint64_t *weight,
                                   const uint32_t *seg) {
    struct Pt {
        uint64_t e1, e2;
        int32_t gap;
        uint64_t w;
    };
    std::vector<Pt> pts(n);
    for (uint64_t i = 0; i < n; ++i) {
        pts[i].gap = gap[i];
        pts[i].w = weight[i];
        canonical_pair(e1[i], e2[i], seg, &pts[i].e1, &pts[i].e2);
    }
    std::sort(pts.begin(), pts.end(), [](const Pt &a, const Pt &b) {
        return std::tie(a.e1, a.e2, a.gap) < std::tie(b.e1, b.e2, b.gap);
    });
    PairPoints o;
    for (const Pt &p : pts) {
        if (!o.e1.empty() && o.e1.back() == p.e1 && o.e2.back() == p.e2 && o.gap.back() == p.gap) {
            o.weight.back() += p.w;
            continue;
        }
        o.e1.push_back(p.e1);
        o.e2.push_back(p.e2);
        o.gap.push_back(p.gap);
        o.weight.push_back(p.w);
    }
    return o;
}

// The pairs and the first edges of the ascending points (fewer than 2^32 - 1 of them): pair p is (pe1[p], pe2[p]) with
// the points ppt[p] .. ppt[p + 1]; first edge g has the pairs grp[g] .. grp[g + 1].
struct PairGroups {
    std::vector<uint32_t> pe1, pe2, ppt, grp;
    uint64_t pairs() const { return pe1.size(); }
    uint64_t firsts() const { return grp.size() - 1; }
};

inline PairGroups pair_groups(const PairPoints &pt) {
    PairGroups o;
    const uint64_t n = pt.size();
    for (uint64_t i = 0; i < n; ++i) {
        if (i && pt.e1[i] == pt.e1[i - 1] && pt.e2[i] == pt.e2[i - 1]) continue;
        if (!i || pt.e1[i] != pt.e1[i - 1]) o.grp.push_back((uint32_t)o.pe1.size());
        o.pe1.push_back((uint32_t)pt.e1[i]);
        o.pe2.push_back((uint32_t)pt.e2[i]);
        o.ppt.push_back((uint32_t)i);
    }
    o.ppt.push_back((uint32_t)n);
    o.grp.push_back((uint32_t)o.pe1.size());
    return o;
}

// ---- the weight filter --------------------------------------------------------------------------------------------------

// math::ge(weight, threshold) on doubles (math/xmath.h:210-322): not (weight < threshold and more than 4 ULPs apart)
inline bool math_ge(double a, double b) {
    auto biased = [](double x) {
        uint64_t u;
        memcpy(&u, &x, 8);
        return (u >> 63) ? ~u + 1 : u | (1ull << 63);
    };
    const uint64_t x = biased(a), y = biased(b);
    const bool eq = !std::isnan(a) && !std::isnan(b) && (x >= y ? x - y : y - x) <= 4;
    return eq || !(a < b);
}

// the least weight in half-units with math::ge(weight, threshold); threshold is a number.  A threshold that no weight of
// 64 bits reaches gives 2^64 - 1 (the search below would not end there)
inline uint64_t least_half_units(double threshold) {
    if (!(threshold > 0)) return 0;
    if (!math_ge(9223372036854775808.0, threshold)) return ~0ull;  // 2^63: half of the largest weight, as a double
    const double twice = std::min(2 * threshold, 18446744073709549568.0);  // the last double below 2^64
    uint64_t w = (uint64_t)std::floor(twice);
    w = w > 2 ? w - 2 : 0;
    while (!math_ge((double)w / 2.0, threshold)) ++w;
    return w;
}

// ---- the file -----------------------------------------------------------------------------------------------------------

inline void uleb128(std::string &o, uint64_t v) {  // io::binary::BinWrite of an unsigned integer (binary.hpp:109-122)
    do {
        uint8_t b = v & 0x7f;
        v >>= 7;
        if (v) b |= 0x80;
        o.push_back((char)b);
    } while (v);
}

// PairedBuffer::BinWrite (paired_info_buffer.hpp:197-210) appended to `o`: the number of first edges; per first edge its
// id, per stored second edge its id and the histogram (the number of points, then RawPointT::BinWrite of each,
// index_point.hpp:195-197: float gap, float weight), and a 0.  io::binary::BinWrite writes an unsigned integer as ULEB128
// (binary.hpp:109-122, 136-139) and a float raw.  Ids are edge + 1 (bbk.h).  The n points are ascending (e1, e2);
// point_of(i) is point i as the file has it, which is all that the raw and the clustered index differ in.
struct IndexPoint {
    uint64_t e1, e2;
    float gap, weight;
};

// raw: the gap and the weight as floats
inline IndexPoint raw_index_point(const PairPoints &pt, uint64_t i) {
    return {pt.e1[i], pt.e2[i], (float)pt.gap[i], (float)pt.weight[i]};
}

// clustered: PointT inherits RawPointT::BinWrite (index_point.hpp:195-197, 218-259), which writes sizeof(RawPointT) = 8
// bytes, so a point is the float gap = d - length(e1) (PointTraits::Shrink, :296-299, a float subtraction) and the float
// weight (held in half-units); the variance is not in the file
inline IndexPoint clustered_index_point(uint64_t e1, uint64_t e2, float centre, uint64_t half_units, uint64_t len1) {
    return {e1, e2, centre - (float)len1, (float)((double)half_units / 2.0)};
}

template <class PointOf>
inline void write_paired_index(std::string &o, uint64_t n, PointOf point_of) {
    uint64_t firsts = 0;
    for (uint64_t i = 0; i < n; ++i) firsts += i == 0 || point_of(i).e1 != point_of(i - 1).e1;
    uleb128(o, firsts);
    for (uint64_t i = 0; i < n;) {
        const uint64_t e1 = point_of(i).e1;
        uleb128(o, e1 + 1);
        while (i < n && point_of(i).e1 == e1) {
            const uint64_t e2 = point_of(i).e2;
            uint64_t j = i;
            while (j < n && point_of(j).e1 == e1 && point_of(j).e2 == e2) ++j;
            uleb128(o, e2 + 1);
            uleb128(o, j - i);
            for (; i < j; ++i) {
                const IndexPoint p = point_of(i);
                const float pt[2] = {p.gap, p.weight};
                o.append(reinterpret_cast<const char *>(pt), 8);
            }
        }
        uleb128(o, 0);
    }
}

}  // namespace bbk
