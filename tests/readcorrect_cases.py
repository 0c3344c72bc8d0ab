"""Crafted inputs of the read-corrector tests, shared by the CPU and the GPU files: the unit cases of the rule (one read
each), the reads that pin the island search, and the golden reads with seeded errors.  Every case states what the
restatement (tests/readcorrect_restated.py) must do with it; the expected bytes always come from the restatement run over
the set that is actually used."""
import gzip
import os

import numpy as np

from tests import kmerdata_restated as KR
from tests import readcorrect_restated as R

NUCL = R.NUCL


def _sub(s, p, d=1):
    return s[:p] + NUCL[(NUCL.index(s[p]) + d) % 4] + s[p + 1:]


class Case:
    """one read: `labels` are branches of the rule its searches must take, `corrected`: the sequence the restatement must
    give (None: not stated), `island`: the (lleft, lright) it must find (None: not stated)"""

    def __init__(self, what, seq, qual, good, bad=(), labels=(), corrected=None, island=None, failed=None, result=1):
        self.what, self.seq, self.qual, self.good, self.bad = what, seq, list(qual), set(good), set(bad)
        self.labels, self.corrected, self.island, self.failed, self.result = set(labels), corrected, island, failed, result


def unit_cases(k, seed=100):
    """every branch of CorrectReadRight and of the island rule at this k, one read each"""
    out = []
    nxt = [seed]

    def G(n):
        nxt[0] += 1
        return R.genome(n, nxt[0], k)

    L = 3 * k + 20
    # one substitution near the right end, so that the island is on its left; its k-mers absent or present and not good
    for q, present in ((30, False), (10, False), (30, True), (10, True)):
        g = G(L)
        p = L - 8
        read = _sub(g, p)
        qual = [30] * L
        qual[p] = q
        own = ("own-bad-" if present else "own-absent-") + ("hi" if q >= 20 else "lo")
        out.append(Case("error q=%d, its k-mers %s" % (q, "present" if present else "absent"), read, qual, R.kmers_of(g, k),
                        [x for x in R.kmers_of(read, k) if x not in R.kmers_of(g, k)] if present else (),
                        {own, "alt-hi" if q >= 20 else "alt-lo", "own-good", "flush-extended"}, g, (0, p - 1)))
    # the own-nucleotide candidate carries the OUTER cpos: corrections at p, p+1, p+3, p+4, p+6 all go through, because
    # the good bases at p+2 and p+5 forget the positions before them (with the popped state's cpos the fifth would be
    # 6 < 8 behind the first and refused)
    L2 = 5 * k
    g = G(L2)
    p = L2 - 30
    read = g
    for d in (0, 1, 3, 4, 6):
        read = _sub(read, p + d)
    out.append(Case("outer cpos", read, [10] * L2, R.kmers_of(g, k), (), {"alt-lo", "own-good"}, g, (0, p - 1)))
    # five wrong bases in a row: the fifth correction is 4 < 8 behind the first
    g = G(L2)
    read = g
    for d in range(5):
        read = _sub(read, p + d)
    out.append(Case("five wrong bases in a row", read, [10] * L2, R.kmers_of(g, k), (), {"flush-cluster"}, None, (0, p - 1)))
    # the penalty threshold: n = 4 allows -0.6; after one correction at q = 30 (-5) no other is tried, that state ends at
    # -7, and the state that corrected nothing (-2 -2 -2) wins
    g = G(L)
    read = _sub(_sub(g, L - 3), L - 1)
    out.append(Case("penalty threshold", read, [30] * L, R.kmers_of(g, k), (), {"flush-penalty", "alt-hi"}, read, (0, L - 4)))
    # N corrected at cost 0
    g = G(L)
    read = g[:L - 8] + "N" + g[L - 7:]
    out.append(Case("N corrected", read, [30] * L, R.kmers_of(g, k), (), {"alt-N"}, g, (0, L - 9)))
    # N without a good alternative: the search fails
    g = G(L)
    read = g[:L - 8] + "N" + g[L - 7:]
    out.append(Case("N without alternative", read, [30] * L, R.kmers_of(read[:L - 8], k), (), (), read, (0, L - 9), failed=1))
    # an error in the last base: at q >= 20 keeping it (-2) beats correcting it (-5), at q < 20 it is corrected (-1, -3)
    g = G(L)
    out.append(Case("error in the last base, q=30", _sub(g, L - 1), [30] * L, R.kmers_of(g, k), (), {"alt-hi"},
                    _sub(g, L - 1), (0, L - 2)))
    g = G(L)
    out.append(Case("error in the last base, q=10", _sub(g, L - 1), [30] * (L - 1) + [10], R.kmers_of(g, k), (), {"alt-lo"}, g,
                    (0, L - 2)))
    # left only, and both sides
    g = G(L)
    out.append(Case("left only", _sub(g, 5), [30] * L, R.kmers_of(g, k), (), {"alt-hi"}, g, (6, L - 1)))
    g = G(L + 20)
    out.append(Case("both sides", _sub(_sub(g, 5, 2), L + 20 - 6, 3), [30] * (L + 20), R.kmers_of(g, k), (), {"alt-hi"}, g,
                    (6, L + 20 - 7)))
    # two equal islands: the first wins
    c = 2 * k
    g = G(2 * c + 1)
    out.append(Case("equal islands", _sub(g, c), [30] * (2 * c + 1), R.kmers_of(g, k), (), {"alt-hi"}, g, (0, c - 1)))
    # nothing to do, and nothing possible
    g = G(L)
    out.append(Case("every start good", g, [30] * L, R.kmers_of(g, k), (), (), g, (0, L - 1)))
    g = G(L)
    out.append(Case("no start good", g, [30] * L, (), R.kmers_of(g, k), (), g, None, result=0))
    return out


def size_thr_case(k, seed=300):
    """the size > size_thr branch of FlushCandidates: an island of k + 4 bases, then NNNA NNNA ... with every k-mer the
    search asks for good: `corrections` grows by three states per N until it passes 100 * log2(n) + 1"""
    g = R.genome(k + 4, seed, k)
    read = g + "NNNA" * 110
    qual = [30] * len(read)

    class Recording(dict):
        def get(self, key, default=None):
            self.setdefault(key, len(self))
            return self[key]

    rec = Recording()
    R.ReadCorrector(rec, _AllGood(), k).correct_batch([(read, qual)])
    return Case("size_thr", read, qual, list(rec), (), {"flush-top", "alt-N"}, None, (0, k + 3))


class _AllGood:
    def __getitem__(self, i):
        return 1


def build(cases):
    """(index, keys, good, reads) of the cases together; a k-mer may not be good for one case and bad for another"""
    good = set().union(*[c.good for c in cases])
    bad = set().union(*[c.bad for c in cases])
    assert not good & bad
    index, keys, gd = R.make_index(good, bad)
    return index, keys, gd, [(c.seq, c.qual) for c in cases]


def island_cases(k, seed=500):
    """[(what, read, good starts, absent starts)]: one read each; `absent`: starts whose k-mer is left out of the set"""
    nxt = [seed]

    def G(nk):
        nxt[0] += 1
        return R.genome(nk + k - 1, nxt[0], k)

    out = [("every start good", G(40), list(range(40)), []),
           ("none good", G(40), [], []),
           ("length k, good", G(1), [0], []),
           ("length k, not good", G(1), [], []),
           ("shorter than k", G(1)[:-1], [], []),
           ("run across starts 63 | 64", G(140), list(range(50, 80)) + list(range(100, 120)), []),
           ("run across starts 127 | 128", G(200), list(range(3, 30)) + list(range(120, 150)), []),
           ("run over three chunks", G(200), list(range(60, 135)) + list(range(140, 199)), []),
           ("two equal runs", G(100), list(range(10, 30)) + list(range(50, 70)), []),
           ("two equal runs, the second across 63 | 64", G(100), list(range(10, 30)) + list(range(55, 75)), []),
           ("the later run longer by one", G(100), list(range(10, 30)) + list(range(50, 71)), []),
           ("absent k-mer splitting a run", G(100), [p for p in range(20, 70) if p != 50], [50]),
           ("300 bases", G(300 - k + 1), list(range(5, 100)) + list(range(130, 280 - k)), [110, 290 - k])]
    # an interior N: the starts that cover it are not valid, the run ends there
    g = G(120)
    n_at = 70
    out.append(("interior N", g[:n_at] + "N" + g[n_at + 1:], [p for p in range(120) if not n_at - k < p <= n_at], []))
    return out


def build_islands(k, cases):
    """(index, keys, good, reads): q = 30 everywhere"""
    kmers, good_kmers, absent = set(), set(), set()
    for what, read, good_starts, absent_starts in cases:
        nk = max(len(read) - k + 1, 0)
        assert all(0 <= p < nk for p in good_starts + absent_starts), what
        for p in range(nk):
            x = read[p:p + k]
            if "N" in x:
                continue
            (absent if p in absent_starts else kmers).add(x)
            if p in good_starts:
                good_kmers.add(x)
    assert not kmers & absent
    index, keys, good = R.make_index(good_kmers, kmers - good_kmers)
    assert not any(x in index for x in absent)
    return index, keys, good, [(read, [30] * len(read)) for _, read, _, _ in cases]


def golden_reads(golden_dir, files=(1, 2)):
    reads = []
    for i in files:
        with gzip.open(os.path.join(golden_dir, "ecoli_1K_%d.fq.gz" % i), "rt") as f:
            lines = f.read().split("\n")
        reads += [(lines[j + 1], [ord(c) - 33 for c in lines[j + 3]]) for j in range(0, len(lines) - 3, 4)]
    return reads


def seeded_errors(reads, rate, seed, n_rate=0.1):
    """substitutions at `rate` per base, a tenth of them an N"""
    rng = np.random.default_rng(seed)
    out = []
    for seq, qual in reads:
        s = list(seq)
        for p in np.nonzero(rng.random(len(s)) < rate)[0]:
            if s[p] in NUCL:
                s[p] = "N" if rng.random() < n_rate else NUCL[(NUCL.index(s[p]) + int(rng.integers(1, 4))) % 4]
        out.append(("".join(s), qual))
    return out


def golden_case(golden_dir, k=21, rate=0.02, seed=2024, trim_quality=4, files=(1, 2)):
    """(index, keys, good, trimmed mutated reads): every k-mer of the original reads is good; the new k-mers of the
    mutated reads of every other read are present and not good"""
    orig = golden_reads(golden_dir, files)
    mut = seeded_errors(orig, rate, seed)
    good_kmers = set()
    for seq, qual in orig:
        good_kmers.update(v[1] for v in KR.valid_kmers(seq, qual, k, trim_quality))
    bad = set()
    for seq, qual in mut[::2]:
        bad.update(v[1] for v in KR.valid_kmers(seq, qual, k, trim_quality))
    index, keys, good = R.make_index(good_kmers, bad - good_kmers)
    trimmed = []
    for seq, qual in mut:
        s, q, _, _, _ = R.trim_read(seq, qual, trim_quality)
        trimmed.append((s, q))
    return index, keys, good, trimmed
