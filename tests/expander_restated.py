"""BayesHammer's expansion of the solid k-mers restated in Python (no GPU, no engine): the checker of csrc/expand.hip.

Restated line for line from the reference (paths under assembler/src):
  Expander::operator()                      projects/hammer/expander.cpp:20-70
  the loop around it                        projects/hammer/main.cpp:198-221
over tests/kmerdata_restated.py's trim_ns_and_bad_quality and ValidKMerGenerator.  Marks are visible at once, as in the
reference, and the read order is an argument: one thread, any order.

Next to it, and NOT from the reference: the engine's snapshot rounds and the rule for the reads that can
ever be solid (host/hammer_reads.hpp: expander_candidate).

A read is (seq, qual) as in kmerdata_restated.  `index` maps a k-mer string to its position in the set (the first n
k-mers only: what KMerData::checking_seq_idx finds); `good` is a list of 0 / 1, one per k-mer of the set.
"""
import numpy as np

from tests import kmerdata_restated as KR


class Expander:
    """expander.hpp / expander.cpp; good is marked in place"""

    def __init__(self, index, good, k, trim_quality=4):
        self.index_, self.data_good_, self.k, self.trim_quality = index, good, k, trim_quality
        self.changed_ = 0
        self.passed_coverage_ = False  # not in the reference: whether the last call got past :49-51

    def changed(self):
        return self.changed_

    def __call__(self, seq, qual):
        K = self.k
        self.passed_coverage_ = False
        cr_seq, cr_qual, _ = KR.trim_ns_and_bad_quality(seq, qual, self.trim_quality)
        sz = len(cr_seq)

        if sz < K:
            return False

        covered_by_solid = [False] * sz
        kmer_indices = [-1] * sz

        gen = KR.ValidKMerGenerator(cr_seq, cr_qual, K)
        while gen.has_more():
            kmer = cr_seq[gen.start_:gen.start_ + K].upper()
            idx = self.index_.get(kmer, -1)
            if idx != -1:
                read_pos = gen.pos() - 1

                kmer_indices[read_pos] = idx
                if self.data_good_[idx]:
                    for j in range(read_pos, read_pos + K):
                        covered_by_solid[j] = True
            gen.next()

        for j in range(sz):
            if not covered_by_solid[j]:
                return False
        self.passed_coverage_ = True

        for j in range(sz):
            if kmer_indices[j] == -1:
                continue

            if not self.data_good_[kmer_indices[j]]:
                self.changed_ += 1
                self.data_good_[kmer_indices[j]] = 1

        return False


def expand_pass(reads, k, index, good, order=None, trim_quality=4):
    """one iteration of main.cpp:198-221 with one thread: good is marked in place; returns expander.changed()"""
    expander = Expander(index, good, k, trim_quality)
    for i in (range(len(reads)) if order is None else order):
        expander(*reads[i])
    return expander.changed()


def expand_loop(reads, k, index, good, order=None, max_iterations=25, min_changed=10, trim_quality=4):
    """main.cpp:198-221: (good, [changed of every iteration])"""
    good = list(good)
    counts = []
    for _ in range(max_iterations):
        changed = expand_pass(reads, k, index, good, order, trim_quality)
        counts.append(changed)
        if changed < min_changed:
            break
    return good, counts


class _Everything(dict):
    """an index that holds every k-mer, all as k-mer 0"""

    def get(self, key, default=None):
        return 0


def can_ever_be_solid(seq, qual, k, trim_quality=4):
    """whether Expander::operator() can get past its coverage test for this read at all: it does when every k-mer is in
    the set and good, and more good k-mers never uncover a position"""
    e = Expander(_Everything(), [1], k, trim_quality)
    e(seq, qual)
    return e.passed_coverage_


# ---- the engine's side: candidates and snapshot rounds ----------------------------------------------------------------
def candidate(seq, qual, k, trim_quality=4):
    """(start, length) in the read as parsed when the valid k-mer starts are consecutive from the first base of the
    trimmed read to its last k-mer -- the one stretch equal to the whole trimmed read; None otherwise"""
    s, _, ltrim = KR.trim_ns_and_bad_quality(seq, qual, trim_quality)
    if len(s) < k:
        return None
    st = KR.coalesce(KR.valid_starts(seq, qual, k, trim_quality), k)
    return (ltrim, len(s)) if st == [(ltrim, len(s))] else None


def candidates(reads, k, trim_quality=4):
    """[(read index, start, length)] of the candidates, what `bbk-hammer-reads-dump --expander` prints"""
    out = []
    for i, (seq, qual) in enumerate(reads):
        c = candidate(seq, qual, k, trim_quality)
        if c:
            out.append((i, c[0], c[1]))
    return out


def candidate_reads(reads, k, trim_quality=4):
    """the candidates as the strings the engine is given"""
    return [reads[i][0][s:s + n].upper() for i, s, n in candidates(reads, k, trim_quality)]


def read_status(read, k, index, good):
    """(status, [index of every start, -1 when not in the set]): 0 not solid, 1 solid, 2 every start already good"""
    if len(read) < k:
        return 0, []
    nk = len(read) - k + 1
    idx = [index.get(read[p:p + k], -1) for p in range(nk)]
    g = [i != -1 and bool(good[i]) for i in idx]
    gs = [p for p in range(nk) if g[p]]
    solid = g[0] and g[nk - 1] and all(b - a <= k for a, b in zip(gs, gs[1:]))
    return (2 if all(g) else 1) if solid else 0, idx


def snapshot_round(cands, k, index, good):
    """(G_{r+1}, changed_r, statuses) from G_r = good over the candidate strings"""
    nxt = list(good)
    status = []
    for read in cands:
        s, idx = read_status(read, k, index, good)
        status.append(s)
        if s:
            for i in idx:
                if i != -1:
                    nxt[i] = 1
    return nxt, sum(nxt) - sum(good), status


def snapshot_rounds(cands, k, index, good, max_rounds=25, min_changed=10):
    """(final good, [changed_r], [G_0, G_1, ...]): stops after the first round with changed < min_changed or after
    max_rounds (None: no limit)"""
    states, counts = [list(good)], []
    while max_rounds is None or len(counts) < max_rounds:
        nxt, c, _ = snapshot_round(cands, k, index, states[-1])
        states.append(nxt)
        counts.append(c)
        if c < min_changed:
            break
    return states[-1], counts, states


def covered(read_len, k, good_starts):
    """covered_by_solid of expander.cpp:30-51 as a list, from the good starts"""
    c = [False] * read_len
    for p in good_starts:
        for j in range(p, p + k):
            c[j] = True
    return c


# ---- sets and cases -------------------------------------------------------------------------------------------------
def both_strand_index(kmers):
    """{k-mer: position} of the ascending both-strand set of these k-mers (ascending by the engine's key), and its keys"""
    allk = set(kmers) | {KR.revcomp(x) for x in kmers}
    order = sorted(allk, key=KR.kmer_key)
    return {x: i for i, x in enumerate(order)}, [KR.kmer_key(x) for x in order]


def index_of_reads(reads, k, trim_quality=4):
    """the both-strand set of every valid k-mer of the reads, as spades-kmerdata counts it"""
    kmers = set()
    for seq, qual in reads:
        kmers.update(v[1] for v in KR.valid_kmers(seq, qual, k, trim_quality))
    return both_strand_index(kmers)


def chain_case(k, seed=7, n_reads=30, step=3, extra=10):
    """The chain of overlapping reads: read i is G[step * i, step * i + k + extra) of a random genome; good at first are
    the k-mer at 0 and the last k-mer of every read.  Returns (reads as (seq, qual), index, keys, good)."""
    rng = np.random.default_rng(seed)
    glen = step * (n_reads - 1) + k + extra
    while True:
        genome = "".join(rng.choice(list("ACGT"), glen))
        fwd = [genome[p:p + k] for p in range(glen - k + 1)]
        if len(set(fwd) | {KR.revcomp(x) for x in fwd}) == 2 * len(fwd):  # all distinct, none its own or another's rc
            break
    reads = [(genome[step * i:step * i + k + extra], [30] * (k + extra)) for i in range(n_reads)]
    index, keys = both_strand_index(fwd)
    good = [0] * len(keys)
    good[index[fwd[0]]] = 1
    for i in range(n_reads):
        good[index[fwd[step * i + extra]]] = 1
    return reads, index, keys, good
