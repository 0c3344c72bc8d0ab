"""BayesHammer's KMerData fill restated line for line in Python (no GPU, no engine): the checker of the k-mer statistics.

Restated from the reference (paths under assembler/src):
  Read::trimLeftRight / trimNsAndBadQuality      common/io/reads/read.hpp:87-122
  ValidKMerGenerator (TrimBadQuality, Next)      projects/hammer/valid_kmer_generator.hpp:147-199
  Globals::quality_probs                         projects/hammer/main.cpp:103-105
  NibbleString / QualBitSet / KMerStat           projects/hammer/kmer_stat.hpp:49-149
  Merge, PushKMer, PushKMerRC, KMerDataFiller    projects/hammer/kmer_data.cpp:119-187

A read is (seq, qual): the sequence as the parser leaves it (upper case) and the qualities with the offset already
subtracted, as Read holds them.  Nothing here is "what the rule obviously means": the quirks are kept.
"""
import math
from fractions import Fraction

import numpy as np

MASK64 = (1 << 64) - 1

# main.cpp:103-105
QUALITY_PROBS = [1 - (0.75 if q < 3 else math.pow(10.0, -q / 10.0)) for q in range(256)]


def is_nucl(c):  # common/sequence/nucl.hpp:45-62
    return c in "ACGTacgt"


def trim_left_right(seq, qual, ltrim, rtrim):
    """Read::trimLeftRight: (seq, qual, ok).  The right trim is applied only when rtrim < size_after_left_erase -
    ltrim - 1, which after a left trim is not "rtrim is before the end"."""
    if ltrim >= len(seq) or rtrim < 0 or rtrim < ltrim:
        return "", [], False
    if ltrim > 0:
        seq = seq[ltrim:]
        qual = qual[ltrim:]
    if rtrim - ltrim + 1 < len(seq) and rtrim < len(seq) - ltrim - 1:
        seq = seq[:rtrim - ltrim + 1]
        qual = qual[:rtrim - ltrim + 1]
    return seq, qual, True


def trim_ns_and_bad_quality(seq, qual, threshold):
    """Read::trimNsAndBadQuality: (seq, qual, ltrim); an empty seq when nothing is left"""
    start = 0
    while start < len(seq):
        if seq[start] != "N" and qual[start] > threshold:
            break
        start += 1
    end = len(seq) - 1
    while end > -1:
        if seq[end] != "N" and qual[end] > threshold:
            break
        end -= 1
    s, q, ok = trim_left_right(seq, list(qual), start, end)
    if not ok:
        return "", [], 0
    return s, q, start


class ValidKMerGenerator:
    """valid_kmer_generator.hpp, with K a run-time value"""

    def __init__(self, seq, qual, k, bad_quality_threshold=2):
        self.k = k
        self.seq_, self.qual_ = seq, qual
        self.pos_ = -1
        self.end_ = -1
        self.len_ = len(seq)
        self.correct_probability_ = 1.0
        self.bad_quality_threshold_ = bad_quality_threshold
        self.has_more_ = True
        self.first = True
        self.start_ = None  # start of kmer_ in seq
        self._trim_bad_quality()
        self.next()

    def _get_qual(self, pos):
        return 2 if pos >= self.len_ else self.qual_[pos] & 0xFF

    def _trim_bad_quality(self):
        self.pos_ = 0
        while self.pos_ < self.len_:
            if self._get_qual(self.pos_) >= self.bad_quality_threshold_:
                break
            self.pos_ += 1
        self.end_ = self.len_
        while self.end_ > self.pos_:
            if self._get_qual(self.end_ - 1) >= self.bad_quality_threshold_:
                break
            self.end_ -= 1

    def has_more(self):
        return self.has_more_

    def pos(self):
        return self.pos_

    def next(self):
        k = self.k
        if self.pos_ + k > self.end_:
            self.has_more_ = False
        elif self.first or not is_nucl(self.seq_[self.pos_ + k - 1]):
            # the search branch: scans up to len_, not end_, and does not check what it finds against end_
            self.correct_probability_ = 1.0
            start_hypothesis = self.pos_
            i = self.pos_
            while i < self.len_:
                if i == k + start_hypothesis:
                    break
                self.correct_probability_ *= QUALITY_PROBS[self._get_qual(i)]
                if not is_nucl(self.seq_[i]):
                    start_hypothesis = i + 1
                    self.correct_probability_ = 1.0
                i += 1
            if i == k + start_hypothesis:
                self.start_ = start_hypothesis
                self.pos_ = start_hypothesis + 1
            else:
                self.has_more_ = False
        else:
            # the shift branch: the probability is rolled with a multiply and a divide
            self.start_ += 1
            self.correct_probability_ *= QUALITY_PROBS[self._get_qual(self.pos_ + k - 1)]
            self.correct_probability_ /= QUALITY_PROBS[self._get_qual(self.pos_ - 1)]
            self.pos_ += 1
        self.first = False


class NibbleString:
    """NibbleString<N, 6, uint64_t> with the original set / operator[] arithmetic"""
    BITS = 6
    MAX_VALUE = (1 << 6) - 1

    def __init__(self, n, data=None):
        self.n = n
        self.K = (self.BITS * n + 63) // 64
        self.storage_ = [0] * self.K
        if data is not None:
            for i in range(n):
                self.set(i, data[i])  # masks with MaxValue, does not saturate

    def set(self, n, value):
        value &= 0xFF  # uint8_t
        idx = n * self.BITS // 64
        offset = n * self.BITS - idx * 64
        self.storage_[idx] = ((self.storage_[idx] & ~(self.MAX_VALUE << offset)) |
                              ((value & self.MAX_VALUE) << offset)) & MASK64
        if offset + self.BITS >= 64:
            rbits = 64 - offset
            mask = self.MAX_VALUE >> rbits
            remaining = ((value >> rbits) & mask) & 0xFF
            # at offset + bits == 64 the mask is 0 and the reference rewrites storage_[idx + 1] with itself -- for the
            # last sum of k = 32 that word is one past the array; nothing to restate there
            if mask:
                self.storage_[idx + 1] = (self.storage_[idx + 1] & ~mask & MASK64) | remaining

    def __getitem__(self, n):
        idx = n * self.BITS // 64
        offset = n * self.BITS - idx * 64
        if offset + self.BITS < 64:
            return (self.storage_[idx] >> offset) & self.MAX_VALUE
        rbits = 64 - offset
        mask = self.MAX_VALUE >> rbits
        hi = ((self.storage_[idx + 1] & mask) << rbits) if mask else 0
        return ((self.storage_[idx] >> offset) | hi) & 0xFF

    def iadd(self, other):
        mv = self.MAX_VALUE
        for i in range(self.n):
            self.set(i, min(mv, other[i] + self[i]))

    def words(self):
        return list(self.storage_)

    def values(self):
        return [self[i] for i in range(self.n)]


class KMerStat:
    def __init__(self, k, cnt=0, kquality=1.0, quality=None):
        self.count = cnt
        self.total_qual = np.float32(kquality)
        self.qual = NibbleString(k, quality)
        self.factors = []  # the float32 factor of every merged occurrence, in merge order


def merge(lhs, rhs):  # kmer_data.cpp:119-123
    lhs.count = (lhs.count + rhs.count) & 0x7FFFFFFF  # set_count keeps 31 bits
    lhs.total_qual = np.float32(lhs.total_qual * rhs.total_qual)
    lhs.qual.iadd(rhs.qual)
    lhs.factors.append(rhs.total_qual)


_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(s):
    return "".join(_COMP[c] for c in reversed(s.upper()))


def kmer_key(s):
    """the engine's one-word record of a k-mer: base i in bits [2i, 2i + 2), A=0 C=1 G=2 T=3"""
    v = 0
    for i, c in enumerate(s.upper()):
        v |= "ACGT".index(c) << (2 * i)
    return v


def valid_kmers(seq, qual, k, trim_quality=4):
    """What KMerDataFiller::operator() pushes for one read: [(start in the ORIGINAL read, k-mer, its k qualities,
    correct_probability)]."""
    s, q, ltrim = trim_ns_and_bad_quality(seq, qual, trim_quality)
    if len(s) < k:
        return []
    out = []
    gen = ValidKMerGenerator(s, q, k)
    while gen.has_more():
        st = gen.pos() - 1  # kq = q + gen.pos() - 1
        out.append((ltrim + st, s[st:st + k].upper(), q[st:st + k], gen.correct_probability_))
        gen.next()
    return out


def valid_starts(seq, qual, k, trim_quality=4):
    return [v[0] for v in valid_kmers(seq, qual, k, trim_quality)]


def coalesce(starts, k):
    """consecutive valid starts a..b -> one stretch (a, b + k - a): [(start, length)]"""
    out = []
    for s in starts:
        if out and out[-1][0] + out[-1][1] - k + 1 == s:
            out[-1] = (out[-1][0], out[-1][1] + 1)
        else:
            out.append((s, k))
    return out


def fill_kmer_data(reads, k, kmer_set=None, trim_quality=4):
    """KMerDataCounter::FillKMerData over `reads` ((seq, qual) pairs): {k-mer: KMerStat}.  kmer_set: the k-mers of the
    index (others are skipped: checking_seq_idx == -1); None = every k-mer and reverse complement pushed."""
    data = {}

    def push(kmer, q, prob):
        if kmer_set is not None and kmer not in kmer_set:
            return
        if kmer not in data:
            data[kmer] = KMerStat(k)
        merge(data[kmer], KMerStat(k, 1, np.float32(prob), q))

    for seq, qual in reads:
        for _, kmer, kq, cp in valid_kmers(seq, qual, k, trim_quality):
            push(kmer, kq, 1 - cp)
            push(revcomp(kmer), kq[::-1], 1 - cp)
    return data


def pack_le(values, bits=6):
    """independent statement of the QualBitSet layout: value i in bits [bits * i, bits * i + bits) of one little-endian
    bit string, cut into u64 words"""
    v = 0
    for i, x in enumerate(values):
        v |= (x & ((1 << bits) - 1)) << (bits * i)
    nw = (bits * len(values) + 63) // 64
    return [(v >> (64 * w)) & MASK64 for w in range(nw)]


def total_qual_bound(factors):
    """(P, bound): the exact product of the float32 factors and the accepted |device - P| (the issue's derivation:
    (n + 1) * 2^-22 * P + n * 2^-149)"""
    p = Fraction(1)
    for f in factors:
        p *= Fraction(float(f))
    n = len(factors)
    return p, (n + 1) * Fraction(1, 2 ** 22) * p + n * Fraction(1, 2 ** 149)


def min_window_complement(reads, k, trim_quality=4):
    """the smallest 1 - cp over every pushed window: the tolerance's condition is >= 2^-10"""
    m = 1.0
    for seq, qual in reads:
        for _, _, _, cp in valid_kmers(seq, qual, k, trim_quality):
            m = min(m, 1 - cp)
    return m


def crafted_reads(k, rng):
    """[(what, seq, qual)]: reads that take every corner of the two rules at this k (rng: numpy Generator for the bases)"""
    def bases(n):
        return "".join(rng.choice(list("ACGT"), n))

    out = []
    # a left trim suppresses the right trim: 3 bad bases in front, 2 bases of quality 3 at the end, which then stay
    # (and are not below the generator's threshold 2 either): the last k-mer ends at the last base
    n = k + 12
    out.append(("left trim keeps the q=3 tail", bases(n), [2] * 3 + [30] * (n - 5) + [3] * 2))
    # the same with a tail of quality 1: it survives the trimming, the generator's end_ stops before it
    out.append(("left trim keeps the q=1 tail", bases(n), [4] * 3 + [30] * (n - 5) + [1] * 2))
    # without a left trim the right trim is applied
    out.append(("right trim alone", bases(n), [30] * (n - 4) + [4, 3, 0, 2]))
    # both ends at the thresholds: 4 is trimmed, 5 is not
    out.append(("thresholds", bases(n), [5] + [30] * (n - 2) + [5]))
    # the search branch emits a window that ends beyond end_: after the left trim of 2 the read is k + 4 long with an N
    # at 3 and two q < 2 bases at the end (kept by the quirk above), so end_ = k + 2 and the window [4, k + 4) is found
    s = bases(2) + bases(3) + "N" + bases(k)
    out.append(("window beyond end_", s, [3] * 2 + [30] * (k + 2) + [1, 0]))
    # N-splitting: runs of k + 3, k - 1, k and 2 * k bases
    s = bases(k + 3) + "N" + bases(k - 1) + "NN" + bases(k) + "N" + bases(2 * k)
    out.append(("N-splitting", s, [int(x) for x in rng.integers(5, 42, len(s))]))
    # an N next to the ends and a low-quality base in the middle (which trims nothing)
    s = "N" + bases(k + 5) + "N"
    out.append(("N at the ends", s, [30] * 5 + [0] + [30] * (len(s) - 6)))
    out.append(("all N", "N" * (k + 7), [30] * (k + 7)))
    out.append(("exactly k", bases(k), [int(x) for x in rng.integers(5, 42, k)]))
    out.append(("shorter than k after trimming", bases(k + 1), [2, 4] + [30] * (k - 1)))
    out.append(("shorter than k", bases(k - 1), [30] * (k - 1)))
    out.append(("all bad", bases(k + 3), [2] * (k + 3)))
    return out


def fill_kmer_data_fast(reads, k, kmer_set=None, trim_quality=4):
    """The same statistics for inputs too large for the line-for-line classes: {k-mer: (count, [sums], [factors])}.  The
    valid k-mers and their rolled probabilities still come from the restated generator; the saturating sums are taken
    as min(63, sum of q & 63), which a test holds against NibbleString's += on small inputs."""
    acc = {}

    def push(kmer, q, f):
        if kmer_set is not None and kmer not in kmer_set:
            return
        e = acc.get(kmer)
        if e is None:
            e = acc[kmer] = [0, np.zeros(k, dtype=np.int64), []]
        e[0] += 1
        e[1] += q
        e[2].append(f)

    for seq, qual in reads:
        for _, kmer, kq, cp in valid_kmers(seq, qual, k, trim_quality):
            q = np.array(kq, dtype=np.int64) & 63
            f = np.float32(1 - cp)
            push(kmer, q, f)
            push(revcomp(kmer), q[::-1], f)
    return {km: (e[0], [int(x) for x in np.minimum(e[1], 63)], e[2]) for km, e in acc.items()}
