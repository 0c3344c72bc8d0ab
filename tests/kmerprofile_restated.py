"""Literal sequential restatement (pure Python, no GPU, no reference code) of the two profile steps of the reference's
binning flow, for the tests of the k-mer profile engine:

  * KmerMultiplicityCounter::FilterCombinedKmers (projects/mts/kmer_multiplicity_counter.cpp:72-139): the N-way merge
    of the samples' sorted (k-mer, count) records under RtSeq::less3 (word 0 most significant) with its keep rule;
  * ProfileCounter::operator() / WinsoredMeanImpl / Variance (projects/mts/contig_abundance.cpp:46-78,245-284) and the
    output loop of Runner::Run (projects/mts/contig_abundance_counter.cpp:18-44).

One place is restated, not copied in behaviour: WinsoredMeanImpl selects with std::nth_element and then reads v[o] and
v[n - o - 1], which after that call are whatever introselect left there.  Here the vector is sorted (the reference's
commented-out std::sort line) and the same in-place loop runs over it; for n = 1 (where the reference reads past the
vector) the value stands.  One more: a contig of exactly k - 1 characters makes the reference divide 0 by 0 and then
fail its VERIFY on an empty profile list; here it gets no line.
"""
import math
import struct

import numpy as np

_COMP = str.maketrans("ACGT", "TGCA")
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def rc(s):
    return s[::-1].translate(_COMP)


def words(k):
    return (k + 31) // 32


def encode(kmer):
    """RtSeq words: base i in bits 2(i % 32) of word i / 32"""
    w = [0] * words(len(kmer))
    for i, c in enumerate(kmer):
        w[i >> 5] |= _CODE[c] << (2 * (i & 31))
    return tuple(w)


def decode(key, k):
    return "".join("ACGT"[(int(key[i >> 5]) >> (2 * (i & 31))) & 3] for i in range(k))


def canonical(kmer):
    """the strand a canonical count keeps: the k-mer unless its reverse complement is smaller base by base"""
    r = rc(kmer)
    return r if r < kmer else kmer


# ---- join ---------------------------------------------------------------------------------------------------------------

def filter_sample(keys, counts, ci=2, cs=255):
    """KMC's -ci / -cs on one sample's ascending (key words, count) records"""
    return [(tuple(int(x) for x in key), min(int(c), cs)) for key, c in zip(keys, counts) if int(c) >= ci]


def join(samples, min_samples, min_mult):
    """samples: per sample its ascending [(key tuple, count)].  Returns (kept keys, rows) in merge order."""
    n = len(samples)
    nxt = [0] * n
    top = [None] * n
    alive = [False] * n

    def read(i):
        if nxt[i] < len(samples[i]):
            top[i] = samples[i][nxt[i]]
            nxt[i] += 1
            return True
        return False

    for i in range(n):
        alive[i] = read(i)
    keys, rows = [], []
    while True:
        min_kmer = None
        cnt_min = 0
        for i in range(n):
            if alive[i]:
                cur = top[i][0]
                if min_kmer is None or cur < min_kmer:  # less3: tuples compare word 0 first
                    min_kmer = cur
                    cnt_min = 0
                if cur == min_kmer:
                    cnt_min += 1
        if min_kmer is None:
            break
        if cnt_min >= min_samples:
            cnt_vector = [0] * n
            total_cnt = 0
            for i in range(n):
                if alive[i] and top[i][0] == min_kmer:
                    cnt_vector[i] = top[i][1]
                    total_cnt += top[i][1]
            if cnt_min > 1 or total_cnt > min_mult:
                keys.append(min_kmer)
                rows.append([c & 0xFFFF for c in cnt_vector])  # sizeof(Mpl) bytes of each count
        for i in range(n):
            if alive[i] and top[i][0] == min_kmer:
                alive[i] = read(i)
    return keys, rows


def kmers_bytes(keys):
    """RtSeq::BinWrite of every kept k-mer"""
    return b"".join(struct.pack("<%dQ" % len(k), *k) for k in keys)


def bpr_bytes(rows):
    return b"".join(struct.pack("<%dH" % len(r), *r) for r in rows)


# ---- abundance ----------------------------------------------------------------------------------------------------------

def _biased(v):
    u = struct.unpack("<Q", struct.pack("<d", v))[0]
    return ((~u + 1) & 0xFFFFFFFFFFFFFFFF) if u >> 63 else (u | (1 << 63))


def ls(a, b):
    """math::ls (common/math/xmath.h): a < b and more than 4 ULPs apart (NaN is never almost equal)"""
    if not (math.isnan(a) or math.isnan(b)) and abs(_biased(a) - _biased(b)) <= 4:
        return False
    return a < b


def split_on_ns(seq):
    """SplitOnNs: the maximal stretches of ACGT (either case)"""
    out, cur = [], []
    for c in seq:
        if c in "ACGTacgt":
            cur.append(c.upper())
        elif cur:
            out.append("".join(cur))
            cur = []
    if cur:
        out.append("".join(cur))
    return out


def winsor_offset(n):
    return int(math.ceil(float(np.float32(np.uint64(n)) * np.float32(0.05))))


def winsorised(values):
    """the vector WinsoredMeanImpl sums, with std::sort in the place of std::nth_element"""
    v = sorted(int(x) for x in values)
    n = len(v)
    if n < 2:
        return v
    o = winsor_offset(n)
    for i in range(o):
        v[i] = v[o]
        v[n - i - 1] = v[n - o - 1]
    return v


def earmarks(contig, k, table):
    """(rows found in contig order, k-mer positions of the ACGT stretches); table: canonical k-mer string -> row"""
    found, positions = [], 0
    for seq in split_on_ns(contig):
        if len(seq) < k:
            continue
        for j in range(len(seq) - k + 1):
            positions += 1
            row = table.get(canonical(seq[j:j + k]))
            if row is not None:
                found.append(row)
    return found, positions


def abundance_ints(contig, k, table, n_samples):
    """what the device returns: (n, positions, [sum per sample], [sum of squares per sample])"""
    found, positions = earmarks(contig, k, table)
    sums, sqs = [], []
    for s in range(n_samples):
        v = winsorised([row[s] for row in found])
        sums.append(sum(v))
        sqs.append(sum(x * x for x in v))
    return len(found), positions, sums, sqs


def f32(x):
    return np.uint64(x).astype(np.float32)


def fixed2(x):
    """std::fixed << std::setprecision(2) of a float (printed as the double it widens to)"""
    return "%.2f" % float(np.float32(x))


def profile_line(name, length, k, n, sums, sqs, var=False):
    """the line Runner::Run writes for one contig, or None (too few earmarks)"""
    denom = (length - k + 1) & 0xFFFFFFFFFFFFFFFF  # size_t
    if denom == 0:
        return None
    if ls(float(n) / float(denom), 0.7):
        return None
    out = [name, "\t"]
    for s in range(len(sums)):
        mean = f32(sums[s]) / f32(n)
        if var:
            variance = f32(sqs[s]) / f32(n) - mean * mean
            out.append(fixed2(mean) + "\t" + fixed2(variance))
        else:
            out.append(fixed2(mean))
        out.append("\t")
    out.append("\n")
    return "".join(out)


def run(contigs, k, table, n_samples, min_len=0, var=False):
    """contigs: [(name, sequence)] in file order.  The first contig shorter than min_len ENDS the run."""
    text = []
    for name, seq in contigs:
        if len(seq) < min_len:
            break
        n, _, sums, sqs = abundance_ints(seq, k, table, n_samples)
        line = profile_line(name, len(seq), k, n, sums, sqs, var)
        if line is not None:
            text.append(line)
    return "".join(text)
