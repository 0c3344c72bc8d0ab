"""The prepared read batch (csrc/hreads.hip) stated in Python: no GPU, no engine.

Two things live here:
  * the CLOSED FORM of Read::trimNsAndBadQuality and ValidKMerGenerator<K>(read, 2) that k_hr_prepare implements
    (closed_trim, closed_starts): first / last positions and run lengths, nothing sequential;
  * the LITERAL generator with the predicate as a parameter (literal_starts), because tests/kmerdata_restated.py has it
    for ACGTacgt only and the read corrector takes ACGT alone (csrc/readcorrect_host.hpp: is_nucl).
The literal rules stay the oracle: tests/test_hreads_restated.py holds the closed form against them, the GPU tests hold
the kernels against the literal rules.

A record is (seq, qual): any characters, qualities with the offset already subtracted.
"""
from tests import kmerdata_restated as KR


def is_nucl_kmer(c):  # common/sequence/nucl.hpp:45-62 -- the count, the statistics, the expansion
    return c in "ACGTacgt"


def is_nucl_corrector(c):  # csrc/readcorrect_host.hpp: is_nucl -- the read corrector
    return c in "ACGT"


PREDICATES = {"kmer": is_nucl_kmer, "corrector": is_nucl_corrector}


# ---- literal ---------------------------------------------------------------------------------------------------------
def literal_trim(seq, qual, threshold):
    """(start, length) of what Read::trimNsAndBadQuality leaves, in the record as parsed; (0, 0): nothing"""
    s, _, ltrim = KR.trim_ns_and_bad_quality(seq, list(qual), threshold)
    return (ltrim, len(s)) if len(s) else (0, 0)


def literal_starts(seq, qual, k, is_nucleotide):
    """ValidKMerGenerator<k>(seq, qual, 2) over a read that is trimmed already (valid_kmer_generator.hpp:147-199, as
    host/hammer_reads.hpp generator_stretches walks it): the valid starts"""
    len_ = len(seq)

    def get_qual(pos):
        return 2 if pos >= len_ else qual[pos] & 0xFF

    pos_ = 0
    while pos_ < len_:
        if get_qual(pos_) >= 2:
            break
        pos_ += 1
    end_ = len_
    while end_ > pos_:
        if get_qual(end_ - 1) >= 2:
            break
        end_ -= 1
    out = []
    first = True
    start = None
    while True:
        if pos_ + k > end_:
            break
        if first or not is_nucleotide(seq[pos_ + k - 1]):
            start_hypothesis = pos_
            i = pos_
            while i < len_:
                if i == k + start_hypothesis:
                    break
                if not is_nucleotide(seq[i]):
                    start_hypothesis = i + 1
                i += 1
            if i != k + start_hypothesis:
                break
            start = start_hypothesis
            pos_ = start_hypothesis + 1
        else:
            start = pos_
            pos_ += 1
        first = False
        out.append(start)
    return out


def identity_trim(seq, qual, threshold=None):
    """the trim of a record that is trimmed already (BBK_NO_TRIM): all of it"""
    return 0, len(seq)


# ---- closed form -----------------------------------------------------------------------------------------------------
def closed_trim(seq, qual, threshold):
    n = len(seq)
    good = [i for i in range(n) if seq[i] != "N" and qual[i] > threshold]
    if not good:
        return 0, 0
    f, l = good[0], good[-1]
    size = n - f  # after the left erase (f == 0: nothing erased)
    if l - f + 1 < size and l < size - f - 1:  # the two comparisons of trimLeftRight: `size` is the size AFTER the left erase
        size = l - f + 1
    return f, size


def closed_starts(seq, qual, k, is_nucleotide):
    """the valid starts over a trimmed read: every window start below T = end_ - k and the first one at or above it"""
    n = len(seq)
    ok = [i for i in range(n) if qual[i] >= 2]
    if not ok:
        return []
    pos0, end_ = ok[0], ok[-1] + 1
    T = end_ - k
    if pos0 > T:
        return []
    out = []
    run = 0  # nucleotides in a row ending at e
    for e in range(n):
        run = run + 1 if is_nucleotide(seq[e]) else 0
        s = e - k + 1
        if run >= k and s >= pos0:  # a window start
            out.append(s)
            if s >= T:
                break
    return out


# ---- the batch -------------------------------------------------------------------------------------------------------
def prepare(records, k, trim_quality, trim=literal_trim, starts=literal_starts):
    """What a bbk_hreads holds for `records`: (trims, kmer stretches per record, corrector stretches per record,
    candidate flags).  k-mer stretches are in the record as parsed, corrector stretches relative to the trimmed read."""
    trims, kst, cst, cand = [], [], [], []
    for seq, qual in records:
        t0, tl = trim(seq, qual, trim_quality)
        s, q = seq[t0:t0 + tl], list(qual[t0:t0 + tl])
        trims.append((t0, tl))
        if tl >= k:
            a = [(x + t0, y) for x, y in KR.coalesce(starts(s, q, k, is_nucl_kmer), k)]
            b = KR.coalesce(starts(s, q, k, is_nucl_corrector), k)
        else:
            a, b = [], []
        kst.append(a)
        cst.append(b)
        cand.append(1 if len(a) == 1 and a[0] == (t0, tl) else 0)  # hammer_reads.hpp: expander_candidate
    return trims, kst, cst, cand


def prepare_closed(records, k, trim_quality):
    return prepare(records, k, trim_quality, closed_trim, closed_starts)


def random_records(rng, n, k=None, max_len=None, odd=0.15):
    """the issue's random reads: lengths 0..max_len, `odd` of the characters from a set with N, n and ., qualities from
    {0..5, 30}"""
    if max_len is None:
        max_len = 3 * k + 10
    quals = [0, 1, 2, 3, 4, 5, 30]
    out = []
    for _ in range(n):
        ln = int(rng.integers(0, max_len + 1))
        pick = rng.random(ln) < odd
        a = rng.choice(list("ACGT"), ln)
        b = rng.choice(list("Nn.acgtN"), ln)
        seq = "".join(str(y) if p else str(x) for x, y, p in zip(a, b, pick))
        # long runs of good quality with bad ends now and then, so that trims and q < 2 tails both occur
        mode = rng.integers(0, 3)
        if mode == 0:
            q = [int(x) for x in rng.choice(quals, ln)]
        else:
            q = [30] * ln
            for side in (0, 1):
                m = int(rng.integers(0, 6))
                for j in range(min(m, ln)):
                    q[j if side == 0 else ln - 1 - j] = int(rng.choice(quals))
        out.append((seq, q))
    return out


def boundary_records(rng):
    """every event of the two rules at a chunk boundary: positions 62..65 and 126..129 in records of 63..200 bases"""
    out = []
    for n in (63, 64, 65, 127, 128, 129, 200):
        seq = "".join(rng.choice(list("ACGT"), n))
        for p in (62, 63, 64, 65, 126, 127, 128, 129):
            if p >= n:
                continue
            out.append((seq, [3] * p + [30] * (n - p)))                        # the first good base
            out.append((seq, [30] * (p + 1) + [3] * (n - p - 1)))              # the last good base (right trim)
            out.append((seq, [3] + [30] * p + [1] * (n - p - 1)))              # ... after a left trim: the tail stays,
            out.append((seq, [0] + [30] * p + [1] * (n - p - 1)))              #     and end_ is at the boundary
            out.append((seq, [1] * p + [30] * (n - p)))                        # the first q >= 2 (at trim quality 0)
            out.append((seq, [1] * p + [30] + [1] * (n - p - 1)))              # both at the same base
            for c in "Nn.a":
                out.append((seq[:p] + c + seq[p + 1:], [30] * n))              # an N, a lower-case base, a '.'
                out.append((seq[:p] + c + seq[p + 1:], [0] + [30] * (n - 3) + [1] * 2))
            out.append((seq[:p] + "N" * (n - p), [30] * n))                    # nothing but N from there on
            out.append(("N" * p + seq[p:], [30] * n))
    return out
