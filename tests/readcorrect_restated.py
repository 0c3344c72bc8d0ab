"""BayesHammer's ReadCorrector restated in Python (no GPU, no engine): the checker of csrc/readcorrect.hip and of
csrc/readcorrect_host.hpp.

Restated line for line from the reference (paths under assembler/src):
  state, std::less<state>, FlushCandidates      projects/hammer/read_corrector.cpp:22-64
  ReadCorrector::CorrectReadRight               projects/hammer/read_corrector.cpp:66-158
  ReadCorrector::CorrectOneRead                 projects/hammer/read_corrector.cpp:160-245
  CorrectReadsBatch                             projects/hammer/hammer_tools.cpp:79-105
  Read::print                                   common/io/reads/read.hpp:221-236
over tests/kmerdata_restated.py's ValidKMerGenerator and revcomp, and over an explicit model of the heap algorithms of
libstdc++ (bits/stl_heap.h: __push_heap, __adjust_heap, __pop_heap) under std::priority_queue: which of two states of
equal (penalty, pos) is popped first is decided there, and it decides the corrected read.

A read is (seq, qual): the TRIMMED read of CorrectReadsBatch, qualities with the offset subtracted.  `index` maps a k-mer
string to its position in the set, `good` is a list of 0 / 1.  A byte other than A, C, G, T is a non-nucleotide.

Not from the reference: every search reports its pops, the largest size of `corrections` after a flush and whether two
states of equal (penalty, pos) ever sat in a heap together -- the figures the engine's capacity rule is stated in.
"""
import math

from tests import kmerdata_restated as KR

NUCL = "ACGT"
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def is_nucl(c):
    return c in NUCL


def reverse_complement(s):  # sequence_tools.hpp ReverseComplement: nucl_complement leaves N as it is
    return "".join(_COMP.get(c, c) for c in reversed(s))


class State:
    __slots__ = ("pos", "str", "penalty", "last", "cpos")

    def __init__(self, pos, s, penalty, last, cpos):
        self.pos, self.str, self.penalty, self.last, self.cpos = pos, s, penalty, last, cpos


def state_less(lhs, rhs):  # :41-46
    return lhs.penalty < rhs.penalty or (lhs.penalty == rhs.penalty and lhs.pos < rhs.pos)


class PriorityQueue:
    """std::priority_queue<T, std::vector<T>, less> of libstdc++: push = push_back + push_heap, pop = pop_heap + pop_back,
    with the sifting of bits/stl_heap.h restated step for step"""

    def __init__(self, less):
        self.c, self.less = [], less
        self.tie = False  # not in the library: two elements that compared equivalent met in a sift

    def _cmp(self, a, b):
        r = self.less(a, b)
        if not r and not self.less(b, a):
            self.tie = True
        return r

    def _push_heap(self, hole, top, value):  # __push_heap
        c = self.c
        parent = (hole - 1) // 2
        while hole > top and self._cmp(c[parent], value):
            c[hole] = c[parent]
            hole = parent
            parent = (hole - 1) // 2
        c[hole] = value

    def _adjust_heap(self, hole, length, value):  # __adjust_heap
        c = self.c
        top = hole
        second = hole
        while second < (length - 1) // 2:
            second = 2 * (second + 1)
            if self._cmp(c[second], c[second - 1]):
                second -= 1
            c[hole] = c[second]
            hole = second
        if (length & 1) == 0 and second == (length - 2) // 2:
            second = 2 * (second + 1)
            c[hole] = c[second - 1]
            hole = second - 1
        self._push_heap(hole, top, value)

    def push(self, value):
        self.c.append(value)
        self._push_heap(len(self.c) - 1, 0, value)

    def top(self):
        return self.c[0]

    def pop(self):
        c = self.c
        if len(c) > 1:  # pop_heap: __pop_heap(first, last - 1, last - 1)
            value = c[-1]
            c[-1] = c[0]
            self._adjust_heap(0, len(c) - 1, value)
        c.pop()

    def empty(self):
        return not self.c

    def size(self):
        return len(self.c)


class SearchInfo:
    def __init__(self):
        self.pops = 0       # corrections.pop() calls, the one that ends the search included
        self.max_heap = 1   # largest corrections.size() after a flush (1: the start state)
        self.tie = False
        self.failed = False
        self.flush_top_only = 0  # flushes that took the size > size_thr branch
        self.labels = set()  # the branches of the rule the search took (names in correct_read_right)


def _flush_candidates(corrections, candidates, size_limit, info):  # :49-64
    if candidates.empty():
        return candidates
    if corrections.size() > size_limit:
        corrections.push(candidates.top())
        info.flush_top_only += 1
        info.labels.add("flush-top")
    else:
        while not candidates.empty():
            corrections.push(candidates.top())
            candidates.pop()
    info.tie = info.tie or candidates.tie
    info.max_heap = max(info.max_heap, corrections.size())
    return PriorityQueue(state_less)


class ReadCorrector:
    def __init__(self, index, good, k):
        self.index_, self.good_, self.K = index, good, k
        self.changed_reads_ = self.changed_nucleotides_ = self.uncorrected_nucleotides_ = self.total_nucleotides_ = 0
        self.own_candidate_keeps_cpos = False  # NOT the reference: the rule without its outer-cpos quirk, for one test
        self.searches = []  # (read number of the batch or None, direction 0 right / 1 left, SearchInfo)
        self._read = None

    def stats(self):
        return [self.changed_reads_, self.changed_nucleotides_, self.uncorrected_nucleotides_, self.total_nucleotides_]

    def correct_read_right(self, seq, qual, right_pos, direction=0):  # :66-158
        K = self.K
        info = SearchInfo()
        self.searches.append((self._read, direction, info))
        read_size = len(seq)
        corrections, candidates = PriorityQueue(state_less), PriorityQueue(state_less)
        outer_cpos = (0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF)

        size_thr = int(100 * math.log2(read_size - right_pos)) + 1
        # penalty < -(n * 15.0 / 100) with an integer penalty: 100 * penalty < -15 * n
        n = read_size - right_pos
        pos_thr = 8

        corrections.push(State(right_pos, seq, 0, seq[right_pos - K + 1:right_pos + 1], outer_cpos))
        while not corrections.empty():
            correction = corrections.top()
            corrections.pop()
            info.pops += 1
            pos = correction.pos + 1
            if pos == read_size:
                info.tie = info.tie or corrections.tie
                return correction.str

            c = correction.str[pos]

            extended = False
            own_cpos = correction.cpos if self.own_candidate_keeps_cpos else outer_cpos  # the OUTER cpos (:70,98,104)
            if is_nucl(c):
                last = correction.last[1:] + c
                idx = self.index_.get(last, -1)
                if idx != -1:
                    g = self.good_[idx]
                    info.labels.add("own-good" if g else "own-bad-hi" if qual[pos] >= 20 else "own-bad-lo")
                    candidates.push(State(pos, correction.str,
                                          correction.penalty - (0 if g else (1 if qual[pos] >= 20 else 2)),
                                          last, own_cpos))
                    if g and qual[pos] >= 20:
                        extended = True
                else:
                    info.labels.add("own-absent-hi" if qual[pos] >= 20 else "own-absent-lo")
                    candidates.push(State(pos, correction.str, correction.penalty - (2 if qual[pos] >= 20 else 3),
                                          last, own_cpos))

            if extended:
                info.labels.add("flush-extended")
                candidates = _flush_candidates(corrections, candidates, size_thr, info)
                continue

            if 100 * correction.penalty < -15 * n:
                info.labels.add("flush-penalty")
                candidates = _flush_candidates(corrections, candidates, size_thr, info)
                continue

            # size_t pos minus a uint16_t: 0xFFFF in front wraps to a huge value
            if ((pos - correction.cpos[0]) & KR.MASK64) < pos_thr:
                info.labels.add("flush-cluster")
                candidates = _flush_candidates(corrections, candidates, size_thr, info)
                continue

            cpos = correction.cpos[1:] + (pos & 0xFFFF,)
            for cc in range(4):
                ncc = NUCL[cc]
                if c == ncc:
                    continue
                last = correction.last[1:] + ncc
                idx = self.index_.get(last, -1)
                if idx == -1:
                    continue
                if self.good_[idx]:
                    corrected = correction.str[:pos] + ncc + correction.str[pos + 1:]
                    penalty = correction.penalty - ((5 if qual[pos] >= 20 else 1) if is_nucl(c) else 0)
                    info.labels.add(("alt-hi" if qual[pos] >= 20 else "alt-lo") if is_nucl(c) else "alt-N")
                    candidates.push(State(pos, corrected, penalty, last, cpos))

            candidates = _flush_candidates(corrections, candidates, size_thr, info)

        info.tie = info.tie or corrections.tie
        info.failed = True
        self.uncorrected_nucleotides_ += read_size - right_pos
        return seq

    def island(self, seq, qual):
        """the longest solid island of :167-196: (lleft_pos, lright_pos, solid_len); solid_len 0 when there is none"""
        K = self.K
        lleft_pos = lright_pos = -1
        solid_len = 0
        gen = KR.ValidKMerGenerator(seq, qual, K)
        left_pos = right_pos = 0
        while gen.has_more():
            read_pos = gen.pos() - 1
            kmer = seq[read_pos:read_pos + K]
            idx = self.index_.get(kmer, -1)
            if idx != -1 and self.good_[idx]:
                if read_pos != right_pos - K + 2:  # size_t arithmetic: never equal while right_pos is 0
                    left_pos = read_pos
                    right_pos = left_pos + K - 1
                else:
                    right_pos += 1
                if right_pos - left_pos + 1 > solid_len:
                    lleft_pos, lright_pos = left_pos, right_pos
                    solid_len = right_pos - left_pos + 1
            gen.next()
        return lleft_pos, lright_pos, solid_len

    def correct_one_read(self, seq, qual):
        """(result, sequence): :160-245 without the read-name tags"""
        read_size = len(seq)
        lleft_pos, lright_pos, solid_len = self.island(seq, qual)
        self.total_nucleotides_ += read_size
        if solid_len and solid_len != read_size:
            newseq = self.correct_read_right(seq, qual, lright_pos, 0)
            newseq = reverse_complement(self.correct_read_right(reverse_complement(newseq), qual[::-1],
                                                                read_size - 1 - lleft_pos, 1))
            corrected = sum(1 for a, b in zip(seq, newseq) if a != b)
            if corrected:
                self.changed_reads_ += 1
                self.changed_nucleotides_ += corrected
            return True, newseq
        return solid_len == read_size, seq

    def correct_batch(self, reads):
        """CorrectReadsBatch: ([sequence], [result])"""
        out, res = [], []
        for i, (seq, qual) in enumerate(reads):
            self._read = i
            if len(seq) >= self.K:
                r, s = self.correct_one_read(seq, list(qual))
            else:
                r, s = False, seq
            out.append(s)
            res.append(int(r))
        self._read = None
        return out, res

    def maxima(self, n_reads):
        """per read of the last batches: (largest heap, most pops) over its searches that look at a base at all (a
        search that starts at the last base ends with its first pop); (0, 0) without one"""
        m = [(0, 0)] * n_reads
        for r, _, info in self.searches:
            if r is not None and info.pops > 1:
                m[r] = (max(m[r][0], info.max_heap), max(m[r][1], info.pops))
        return m


def read_print(name, seq, qual, ltrim, rtrim, initial_size, offset):
    """Read::print (read.hpp:221-236) of a read whose trimmed sequence is seq"""
    tail = initial_size - rtrim
    out = "@" + name + "\n" + "N" * ltrim + seq + "N" * tail + "\n+" + name
    if ltrim > 0:
        out += " ltrim=%d" % ltrim
    if rtrim < initial_size:
        out += " rtrim=%d" % tail
    badq = chr(offset + 2)
    return out + "\n" + badq * ltrim + "".join(chr(q + offset) for q in qual) + badq * tail + "\n"


def trim_read(seq, qual, threshold):
    """Read::trimNsAndBadQuality with the bookkeeping print needs: (seq, qual, ltrim_, rtrim_, initial_size_)"""
    initial = len(seq)
    start = 0
    while start < len(seq) and not (seq[start] != "N" and qual[start] > threshold):
        start += 1
    end = len(seq) - 1
    while end > -1 and not (seq[end] != "N" and qual[end] > threshold):
        end -= 1
    ltrim, rtrim = start, end
    if ltrim >= len(seq) or rtrim < 0 or rtrim < ltrim:
        return "", [], 0, initial, initial
    ltrim_, rtrim_ = 0, initial
    s, q = seq, list(qual)
    if ltrim > 0:
        ltrim_ += ltrim
        s, q = s[ltrim:], q[ltrim:]
    if rtrim - ltrim + 1 < len(s) and rtrim < len(s) - ltrim - 1:
        rtrim_ -= len(s) - (rtrim - ltrim + 1)
        s, q = s[:rtrim - ltrim + 1], q[:rtrim - ltrim + 1]
    return s, q, ltrim_, rtrim_, initial


# ---- cases -----------------------------------------------------------------------------------------------------------
def genome(n, seed, k):
    """n random bases whose k-mers, reverse complements included, are all different"""
    import numpy as np
    rng = np.random.default_rng(seed)
    while True:
        g = "".join(rng.choice(list(NUCL), n))
        km = [g[i:i + k] for i in range(n - k + 1)]
        if len(set(km) | {KR.revcomp(x) for x in km}) == 2 * len(km):
            return g


def make_index(good_kmers, bad_kmers=()):
    """(index, keys, good) of the ascending both-strand set that holds good_kmers and their reverse complements as good,
    bad_kmers and theirs as present and not good"""
    good_kmers = set(good_kmers)
    good_kmers |= {KR.revcomp(x) for x in good_kmers}
    allk = good_kmers | set(bad_kmers)
    allk |= {KR.revcomp(x) for x in allk}
    order = sorted(allk, key=KR.kmer_key)
    return ({x: i for i, x in enumerate(order)}, [KR.kmer_key(x) for x in order],
            [1 if x in good_kmers else 0 for x in order])


def kmers_of(s, k):
    return [s[i:i + k] for i in range(len(s) - k + 1)]


def branching_read(k, length, seed=5, step=2):
    """The crafted read of the capacity tests: a good true path of `length` bases whose first k + 4 bases are the island
    (the read's bases at k + 4, 2 k + 4, ... are wrong, so no start behind the island is good), then a branch point at every `step`-th base: two good
    alternatives that lead nowhere.  Every quality is 10.  Returns (read, qual, good k-mers)."""
    true = genome(length, seed, k)
    good = set(kmers_of(true, k))
    isl = k + 4
    read = list(true)
    for p in range(isl, length, k):  # an error right after the island, and one in every k-mer from there on
        read[p] = NUCL[(NUCL.index(true[p]) + 3) % 4]
    for p in range(isl + 2, length, step):
        ctx = true[p - k + 1:p]
        for d in (1, 2):
            good.add(ctx + NUCL[(NUCL.index(true[p]) + d) % 4])
    return "".join(read), [10] * length, good
