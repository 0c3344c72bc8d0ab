"""Sequential restatement of the paired-read side of PairInfoCount (pure Python, test infrastructure), pair by pair as
the reference runs it, over tests/gmapper_restated.py (Graph, map_sequence).

  - presentation: LongestValid (io/reads/longest_valid_wrapper.hpp:15-57) with the offsets of SingleRead::Substr
    (io/reads/single_read.hpp:247-258), OrientationChanger (io/reads/orientation.hpp:15-41), operator! swapping the
    two offsets (single_read.hpp:143-147); both mates mapped with MapSequence (sequence_mapper_notifier.cpp:43-56)
  - InsertSizeCounter::ProcessPairedRead (paired_info/is_counter.hpp:85-115)
  - get_median, get_mad, hist_crop, GetISInterval, find_median, find_mean (paired_info/insert_size_refiner.hpp:23-166)
    and CollectLibInformation's order of calls (projects/spades/pair_info_count.cpp:199-243), in doubles
  - EdgePairCounterFiller / DEFilter (pair_info_count.cpp:70-80, 123-133) with exact counts where the reference has a
    HyperLogLog and a counting Bloom filter of 2-bit cells (adt/bf.hpp:50-97)
  - LatePairedIndexFiller::ProcessPairedRead (paired_info/pair_info_filler.hpp:63-93)
  - PairedBufferBase::Add / InsertWithConj (paired_info/paired_info_buffer.hpp:54-57, 103-147)
  - Nx (assembly_graph/core/basic_graph_stats.hpp:97-113) and the bounds of PairInfoCount::run and ProcessPairedReads
    (pair_info_count.cpp:335-337, 292-296)
  - PairedBuffer::BinWrite (paired_info_buffer.hpp:197-210) over io::binary::BinWrite (io/binary/binary.hpp: unsigned
    integers go out as ULEB128, floats raw) and RawPointT::BinWrite (paired_info/index_point.hpp:195-197)
"""
import math
import struct

from tests.gmapper_restated import map_sequence
from tests.helpers import rc

FF, FR, RF, RR = 0, 1, 2, 3
_ACGT = set("ACGTacgt")


def longest_valid(s):
    """LongestValidCoords + Substr: (stretch, left_offset, right_offset); the first of equally long stretches"""
    best_len, best_pos, pos = 0, None, None
    for i in range(len(s) + 1):
        if i < len(s) and s[i] in _ACGT:
            if pos is None:
                pos = i
        else:
            if pos is not None and i - pos > best_len:
                best_len, best_pos = i - pos, pos
            pos = None
    if best_len == 0:
        return "", 0, 0
    return s[best_pos:best_pos + best_len].upper(), best_pos, len(s) - best_pos - best_len


def present(first, second, orientation):
    """((seq, left, right) of the first mate, the same of the second) as the listeners see the pair"""
    a, b = longest_valid(first), longest_valid(second)
    flip = lambda m: (rc(m[0]), m[2], m[1])  # noqa: E731
    if orientation in (RF, RR):
        a = flip(a)
    if orientation in (FR, RR):
        b = flip(b)
    return a, b


def map_pair(g, first, second, orientation):
    """(path1, path2, |second|, trim): trim = left_offset(first) + right_offset(second)"""
    a, b = present(first, second, orientation)
    return map_sequence(g, a[0]), map_sequence(g, b[0]), len(b[0]), a[1] + b[2]


def i32(x):
    return ((x + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


# ---- insert sizes -------------------------------------------------------------------------------------------------------

class InsertSizeCounter:
    def __init__(self, g, min_edge_length):
        self.g, self.thr = g, min_edge_length
        self.hist, self.total, self.mapped, self.negative = {}, 0, 0, 0

    def process(self, path1, path2, read2_size, is_delta):
        self.total += 1
        if (len(path1) == 1 and len(path2) == 1 and path1[0][0] == path2[0][0] and
                self.g.length(path1[0][0]) >= self.thr):
            r1, r2 = path1[0][1], path2[0][1]
            read1_start = r1[2] - r1[0]
            read2_start = r2[2] - r2[0]
            is_ = read2_start - read1_start + read2_size + is_delta
            if is_ > 0:
                self.hist[is_] = self.hist.get(is_, 0) + 1
                self.mapped += 1
            else:
                self.negative += 1


def round_to_zero(t):
    """math::round_to_zero (math/xmath.h:330-340); its argument here is always a histogram key"""
    res = int(math.floor(abs(t) + 0.5))
    return -res if t < 0 else res


def get_median(hist):
    S = 0.0
    for k in sorted(hist):
        S += float(hist[k])
    s = S
    for k in sorted(hist):
        s -= float(hist[k])
        if s <= S / 2:
            return float(k)
    raise AssertionError("empty histogram")


def get_mad(hist, median):
    hist2 = {}
    for k in sorted(hist):
        hist2[abs(k - round_to_zero(median))] = hist[k]  # an assignment, as the reference has it
    return get_median(hist2)


def hist_crop(hist, low, high):
    return {k: v for k, v in hist.items() if low <= k <= high}


def get_is_interval(quantile, hist):
    S = 0.0
    for k in sorted(hist):
        S += float(hist[k])
    lval, rval = S * (1 - quantile) / 2, S * (1 + quantile) / 2
    keys = sorted(hist)
    is_min, is_max = float(keys[0]), float(keys[-1])
    cS = 0.0
    for k in keys:
        if cS <= lval:
            is_min = float(k)
        elif cS <= rval:
            is_max = float(k)
        cS += float(hist[k])
    return is_min, is_max


def find_median(hist):
    """(median, mad, cropped histogram)"""
    median = get_median(hist)
    mad = get_mad(hist, median)
    low = median - 5. * 1.4826 * mad
    high = median + 5. * 1.4826 * mad
    cropped = hist_crop(hist, low, high)
    median = get_median(cropped)
    mad = get_mad(cropped, median)
    return median, mad, cropped


def find_mean(hist):
    """(mean, deviation, {5 * i: value} of the percentiles that were set)"""
    median = get_median(hist)
    mad = get_mad(hist, median)
    low = median - 5. * 1.4826 * mad
    high = median + 5. * 1.4826 * mad

    def moments(low, high):
        n, s, s2 = 0, 0., 0.
        for k in sorted(hist):
            if k < low or k > high:
                continue
            n += hist[k]
            s += float(hist[k]) * 1. * float(k)
            s2 += float(hist[k]) * 1. * float(k) * float(k)
        mean = s / float(n)
        return n, mean, math.sqrt(s2 / float(n) - mean * mean)

    n, mean, delta = moments(low, high)
    low = mean - 5 * delta
    high = mean + 5 * delta
    n, mean, delta = moments(low, high)
    percentiles, m = {}, 0
    for k in sorted(hist):
        if k < low or k > high:
            continue
        mm = m + hist[k]
        for q in range(5, 100, 5):
            scaled = int(float(q) / 100. * float(n))
            if m < scaled <= mm:
                percentiles[q] = k
        m = mm
    return mean, delta, percentiles


def estimate(counter, k, edge_pairs):
    """CollectLibInformation: the statistics as the engine reports them"""
    st = dict(total=counter.total, mapped=counter.mapped, negative=counter.negative, edge_pairs=edge_pairs, mean=0.0,
              deviation=0.0, median=0.0, mad=0.0, left_quantile=0.0, right_quantile=0.0, percentiles=[0] * 19, ok=False)
    if counter.mapped == 0:
        return st
    st["mean"], st["deviation"], pc = find_mean(counter.hist)
    st["percentiles"] = [pc.get(q, 0) for q in range(5, 100, 5)]
    st["median"], st["mad"], cropped = find_median(counter.hist)
    if st["median"] < k + 2:
        return st
    st["left_quantile"], st["right_quantile"] = get_is_interval(0.8, cropped)
    st["ok"] = len(cropped) > 0
    return st


# ---- edge pairs and the filter ------------------------------------------------------------------------------------------

class PairCounts:
    """occurrences of every ordered edge pair over path1 x path2"""

    def __init__(self, g):
        self.g, self.occ = g, {}

    def process(self, path1, path2):
        for e1, _ in path1:
            for e2, _ in path2:
                self.occ[(e1, e2)] = self.occ.get((e1, e2), 0) + 1

    def edge_pairs(self):
        return len(self.occ)

    def c(self, e1, e2):
        """the filter's count: DEFilter adds {e1, e2} and {conj e2, conj e1} for every occurrence"""
        cj = (self.g.conj[e2], self.g.conj[e1])
        return self.occ.get((e1, e2), 0) + self.occ.get(cj, 0)

    def passes(self, e1, e2, threshold):
        return threshold == 0 or min(self.c(e1, e2), 3) > threshold


# ---- points and storage -------------------------------------------------------------------------------------------------

def round_distance_double(d, r):
    """int(std::round(d / double(r))) * r"""
    x = d / float(r)
    q = math.floor(abs(x) + 0.5)  # std::round: half away from zero
    return i32(int(-q if x < 0 else q) * r)


def round_distance_int(d, r):
    """the device's form: (2 |d| + r) / (2 r) with the sign of d, times r"""
    q = (2 * abs(d) + r) // (2 * r)
    return i32((-q if d < 0 else q) * r)


class PairedIndex:
    """the unclustered index: {(e1, e2): {gap: weight}} under the smaller of a pair and its conjugate"""

    def __init__(self, g):
        self.g, self.store = g, {}
        self.under_conjugate = 0  # points stored under the conjugate of the pair they were added with

    def add(self, e1, e2, d, w=1):
        gap = i32(d - self.g.length(e1))
        cj = (self.g.conj[e2], self.g.conj[e1])
        key = min((e1, e2), cj)
        self.under_conjugate += key != (e1, e2)
        if e1 == self.g.conj[e2]:
            w *= 2
        h = self.store.setdefault(key, {})
        h[gap] = h.get(gap, 0) + w

    def points(self):
        return [(e1, e2, gap, w) for (e1, e2) in sorted(self.store) for gap, w in sorted(self.store[(e1, e2)].items())]


def fill_pair(index, counts, path1, path2, read2_size, trim, insert_size, round_distance, threshold):
    read_distance = i32(insert_size - trim) - read2_size
    for e1, r1 in path1:
        for e2, r2 in path2:
            if not counts.passes(e1, e2, threshold):
                continue
            kmer_distance = read_distance + r2[1] - r1[0]
            d = i32(i32(kmer_distance) + r1[2] - r2[3])
            if round_distance > 1:
                d = round_distance_double(d, round_distance)
            index.add(e1, e2, d)


def uleb128(v):
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | 0x80 if v else b)
        if not v:
            return bytes(out)


def prd_bytes(points):
    """BinWrite of the index with ids edge + 1: the number of first edges, then per first edge its id, per stored second
    edge its id, the number of points and the (float gap, float weight) points, and a 0"""
    by_e1 = {}
    for e1, e2, gap, w in points:
        by_e1.setdefault(e1, {}).setdefault(e2, []).append((gap, w))
    out = [uleb128(len(by_e1))]
    for e1 in sorted(by_e1):
        out.append(uleb128(e1 + 1))
        for e2 in sorted(by_e1[e1]):
            pts = by_e1[e1][e2]
            out.append(uleb128(e2 + 1) + uleb128(len(pts)))
            out += [struct.pack("<ff", float(gap), float(w)) for gap, w in pts]
        out.append(uleb128(0))
    return b"".join(out)


# ---- a library ----------------------------------------------------------------------------------------------------------

class Library:
    """the two (three with a filter) passes of PairInfoCount over one paired library held as (first, second, cut)"""

    def __init__(self, g, min_edge_length=0):
        self.g = g
        self.is_counter = InsertSizeCounter(g, min_edge_length)
        self.counts = PairCounts(g)
        self.index = PairedIndex(g)
        self.max_product = 0

    def push_estimate(self, pairs, orientation):
        for first, second in pairs:
            p1, p2, n2, trim = map_pair(self.g, first, second, orientation)
            self.max_product = max(self.max_product, len(p1) * len(p2))
            self.is_counter.process(p1, p2, n2, trim)
            self.counts.process(p1, p2)

    def estimate(self):
        return estimate(self.is_counter, self.g.k, self.counts.edge_pairs())

    def hist(self):
        return sorted(self.is_counter.hist.items())

    def push_fill(self, pairs, orientation, insert_size, round_distance, threshold):
        for first, second in pairs:
            p1, p2, n2, trim = map_pair(self.g, first, second, orientation)
            fill_pair(self.index, self.counts, p1, p2, n2, trim, insert_size, round_distance, threshold)

    def points(self):
        return self.index.points()


def nx(g, percent):
    """Nx (assembly_graph/core/basic_graph_stats.hpp:97-113) over every edge, conjugates included"""
    lengths = sorted(g.length(e) for e in g.seq)
    len_perc = (1.0 - percent * 0.01) * float(sum(lengths))
    for x in lengths:
        if float(x) >= len_perc:
            return x
        len_perc -= float(x)
    return 0


def round_bound(deviation, threshold, max_distance_coeff=2.0, rounding_coeff=0.5, rounding_thr=0):
    """ProcessPairedReads (pair_info_count.cpp:292-296): no rounding when the filter is off"""
    return int(min(max_distance_coeff * deviation * rounding_coeff, rounding_thr)) if threshold else 0


def fmt_double(x):
    """std::ostream << double"""
    return "%g" % x


def lib_text(st):
    """the <prefix>.<i>.lib file of spades-pairinfo"""
    lines = ["%s %d" % (key, st[key]) for key in ("total", "mapped", "negative", "edge_pairs")]
    lines += ["%s %s" % (key, fmt_double(st[key])) for key in ("mean", "deviation", "median", "mad", "left_quantile",
                                                               "right_quantile")]
    lines += ["percentile_%d %d" % (5 * (i + 1), v) for i, v in enumerate(st["percentiles"])]
    lines.append("ok %d" % st["ok"])
    return "".join(x + "\n" for x in lines)
