"""The inputs of the reference-recorded BayesHammer fixtures (tests/golden/hammer_ref/, oracle/record_hammer_ref.py) and
the reader of those fixtures.  Pure Python; no GPU, no engine, no reference tree.

Two paired libraries:
  crafted   a 1000-base genome under paired 100-base reads, with seeded substitutions of low quality, `N`s, ends of
            quality 2 and of quality <= 4, an inverted repeat (a 21-mer and its reverse complement on one strand: at odd
            k no k-mer is its own reverse complement, this is the nearest thing), reads of exactly k and of k - 1 bases
            after trimming, one pair whose right mate is all bad, a lower-case read, and a hot spot where 25-base reads
            carry one or two substitutions each so that one Hamming cluster grows past 64 k-mers, and a cluster whose
            consensus no read holds;
  ecoli     the first ECOLI_PAIRS pairs of tests/golden/ecoli_1K_{1,2}.fq.gz.
"""
import gzip
import hashlib
import json
import os

import numpy as np

from tests import kmerdata_restated as KR
from tests import readcorrect_restated as R

K = 21
READ_LEN = 100
GENOME_LEN = 1000
ECOLI_PAIRS = 120
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
FIXTURES = os.path.join(GOLDEN, "hammer_ref")
CASES = ("crafted", "ecoli")
STAGES = ("stage0", "stage1", "stage2", "stage3", "stage4", "stage5")


def _subst(base, step):
    return R.NUCL[(R.NUCL.index(base) + step) % 4]


def crafted_genome(seed=20):
    """the genome: random, all k-mers of both strands different, then an inverted repeat written over [600, 660)"""
    g = R.genome(GENOME_LEN, seed, K)
    arm = g[600:625]
    g = g[:600] + arm + g[625:635] + KR.revcomp(arm) + g[660:]
    return g


def crafted_pair(seed=20):
    """(left, right): lists of (name, seq, qual) with qual a list of integers (offset subtracted)"""
    rng = np.random.default_rng(seed)
    g = crafted_genome(seed)
    left, right = [], []
    n_pairs = 100
    insert = 260
    for i in range(n_pairs):
        st = int(rng.integers(0, GENOME_LEN - insert + 1))
        a = list(g[st:st + READ_LEN])
        b = list(KR.revcomp(g[st + insert - READ_LEN:st + insert]))
        qa = [int(x) for x in rng.integers(28, 41, READ_LEN)]
        qb = [int(x) for x in rng.integers(28, 41, READ_LEN)]
        for s, q in ((a, qa), (b, qb)):
            if rng.random() < 0.30:  # one substitution of low quality
                p = int(rng.integers(0, READ_LEN))
                s[p] = _subst(s[p], 1 + int(rng.integers(0, 3)))
                q[p] = int(rng.integers(5, 15))
            if rng.random() < 0.06:  # a substitution that the quality does not give away
                p = int(rng.integers(0, READ_LEN))
                s[p] = _subst(s[p], 1 + int(rng.integers(0, 3)))
            if rng.random() < 0.08:
                s[int(rng.integers(0, READ_LEN))] = "N"
            if rng.random() < 0.15:  # an end of quality 2
                n = int(rng.integers(1, 30))
                q[READ_LEN - n:] = [2] * n
            if rng.random() < 0.10:  # ends of quality <= 4 on both sides
                n, m = int(rng.integers(1, 8)), int(rng.integers(1, 12))
                q[:n] = [int(x) for x in rng.integers(0, 5, n)]
                q[READ_LEN - m:] = [int(x) for x in rng.integers(3, 5, m)]
        left.append(("p%d/1" % i, "".join(a), qa))
        right.append(("p%d/2" % i, "".join(b), qb))

    def put(i, side, seq=None, qual=None):
        lst = left if side == 0 else right
        name, s, q = lst[i]
        lst[i] = (name, s if seq is None else seq, q if qual is None else qual)

    put(3, 1, qual=[2] * READ_LEN)  # the right mate is all bad
    # exactly k and k - 1 bases after trimming.  (Good bases in the middle would not do: after a left trim the reference
    # cuts the right end only when the last good base lies in the left half of what is left, read.hpp:101.)
    put(5, 0, seq=g[100:200], qual=[35] * K + [4] * (READ_LEN - K))
    put(6, 0, seq=g[120:220], qual=[35] * (K - 1) + [3] * (READ_LEN - K + 1))
    put(12, 1, seq=g[400:500], qual=[3] * (READ_LEN - K) + [35] * K)
    put(13, 0, seq=g[500:600], qual=[3] * 40 + [35] * K + [4] * (READ_LEN - 40 - K))  # the right end stays: 60 bases
    put(7, 1, seq="N" * READ_LEN)
    put(8, 0, seq=left[8][1].lower())
    s9 = list(left[9][1])
    for p in (10, 31, 52, 73):  # an N every k bases: no valid k-mer, the read cannot be corrected
        s9[p] = "N"
    put(9, 0, seq="".join(s9), qual=[30] * READ_LEN)
    put(10, 1, seq=R.genome(READ_LEN, seed + 1, K), qual=[12] * READ_LEN)  # a read of another genome
    s11 = list(left[11][1])
    s11[50] = _subst(s11[50], 2)  # a wrong base of good quality in a read of quality 40
    put(11, 0, seq="".join(s11), qual=[40] * READ_LEN)

    # the hot spot: 25-base reads over [300, 325), whose window at 2 holds every wrong base.  63 reads carry one wrong
    # base (every position of that window, every other base), 20 carry one of those and a second one.
    hot, span = 300, 25
    n = len(left)
    singles = [(p, step) for p in range(2, 2 + K) for step in (1, 2, 3)]
    doubles = [(singles[3 * j], ((singles[3 * j][0] - 2 + 5 + j) % K + 2, 1 + j % 3)) for j in range(20)]
    for j, errs in enumerate([(e,) for e in singles] + doubles):
        s, q = list(g[hot:hot + span]), [30] * span
        for p, step in errs:
            s[p] = _subst(g[hot + p], step)
            q[p] = 6
        mate = KR.revcomp(g[hot + 150:hot + 150 + span])
        left.append(("h%d/1" % j, "".join(s), q))
        right.append(("h%d/2" % j, mate, [34] * span))
    assert len(left) == len(right) == n + 83

    # a centre that no read holds: reads of exactly k bases around a 21-mer c of another genome, five each of c with one
    # wrong base of quality 6 at 3, at 10 and at 17, and one each of the two k-mers that chain them into one cluster
    c = R.genome(K, seed + 2, K)
    e = {p: _subst(c[p], 1) for p in (3, 10, 17)}
    variants = [((3,), 5), ((3, 10), 1), ((10,), 5), ((10, 17), 1), ((17,), 5)]
    j = 0
    for ps, copies in variants:
        s = "".join(e[p] if p in ps else c[p] for p in range(K))
        for _ in range(copies):
            left.append(("c%d/1" % j, s, [6 if p in ps else 30 for p in range(K)]))
            right.append(("c%d/2" % j, KR.revcomp(g[700:700 + K]), [34] * K))
            j += 1
    return left, right


def ecoli_pair(n_pairs=ECOLI_PAIRS):
    """the first n_pairs records of the two golden files as (header line without '@', seq, quality text)"""
    out = []
    for i in (1, 2):
        with gzip.open(os.path.join(GOLDEN, "ecoli_1K_%d.fq.gz" % i), "rt", encoding="latin-1") as f:
            lines = [next(f).rstrip("\n") for _ in range(4 * n_pairs)]
        out.append([(lines[j][1:], lines[j + 1], lines[j + 3]) for j in range(0, len(lines), 4)])
    return out


def fastq_text(records, offset=33):
    """records with integer qualities or with quality text"""
    return "".join("@%s\n%s\n+\n%s\n" % (n, s, q if isinstance(q, str) else "".join(chr(x + offset) for x in q))
                   for n, s, q in records)


def case_texts(case):
    """(left FASTQ text, right FASTQ text, base names of the two files) of a case"""
    if case == "crafted":
        left, right = crafted_pair()
        return fastq_text(left), fastq_text(right), ("crafted_1.fastq", "crafted_2.fastq")
    if case == "ecoli":
        left, right = ecoli_pair()
        return fastq_text(left), fastq_text(right), ("ecoli_sub_1.fastq", "ecoli_sub_2.fastq")
    raise KeyError(case)


def parsed(text, offset=33):
    """FASTQ text -> [(the whole header line as the name, seq, [quality - offset])], what the reference's parser hands on
    (its kseq reads the name to the end of the line and puts the sequence into upper case)"""
    lines = text.split("\n")
    return [(lines[j][1:], lines[j + 1].upper(), [ord(c) - offset for c in lines[j + 3]])
            for j in range(0, len(lines) - 3, 4)]


def md5(text):
    return hashlib.md5(text.encode("latin-1")).hexdigest()


def load(case, stage):
    """one fixture as the recorder wrote it; stage0 lies in one file per side and comes back joined"""
    if stage == "stage0":
        a, b = load(case, "stage0_1"), load(case, "stage0_2")
        return dict(reads=a["reads"] + b["reads"], printed=[a["printed"], b["printed"]], _provenance=a["_provenance"])
    with gzip.open(os.path.join(FIXTURES, "%s_%s.json.gz" % (case, stage)), "rt", encoding="latin-1") as f:
        return json.load(f)
