"""CPU: the restatement of BayesHammer's KMerData fill (tests/kmerdata_restated.py) pinned against independent
statements -- the plain bit layout, hand-worked trimming and generator cases -- and the tolerance the GPU tests use for
total_qual shown to hold for the reference's own order-dependent float product."""
import random
from fractions import Fraction

import numpy as np
import pytest

from tests import kmerdata_restated as R


@pytest.mark.parametrize("k", [10, 11, 21, 22, 32])
def test_nibble_string_is_plain_little_endian_packing(k):
    rng = random.Random(k)
    for _ in range(20):
        vals = [rng.randrange(64) for _ in range(k)]
        ns = R.NibbleString(k, vals)
        assert ns.K == (6 * k + 63) // 64
        assert ns.words() == R.pack_le(vals)
        assert ns.values() == vals
        # set() over a non-zero string replaces, bit for bit
        other = [rng.randrange(64) for _ in range(k)]
        for i in rng.sample(range(k), k):
            ns.set(i, other[i])
        assert ns.words() == R.pack_le(other)
    if k >= 11:  # sum 10 lies in bits 60..65: words 0 and 1
        ns = R.NibbleString(k)
        ns.set(10, 0b101101)
        assert ns.words()[0] == 0b1101 << 60 and ns.words()[1] == 0b10
    if k >= 22:  # sum 21 lies in bits 126..131: words 1 and 2
        ns = R.NibbleString(k)
        ns.set(21, 0b110110)
        assert ns.words()[1] == 0b10 << 62 and ns.words()[2] == 0b1101


def test_constructor_masks_and_sums_saturate():
    k = 21
    st = R.KMerStat(k, 1, 0.5, [70] * k)
    assert st.qual.values() == [6] * k  # 70 & 63, not min(63, 70)
    acc = R.KMerStat(k)
    for n in range(1, 5):
        R.merge(acc, R.KMerStat(k, 1, 0.5, [40] * 10 + [70] * 11))
        assert acc.qual.values() == [min(63, 40 * n)] * 10 + [min(63, 6 * n)] * 11
    assert acc.count == 4 and acc.total_qual == np.float32(0.0625)
    for _ in range(20):
        R.merge(acc, R.KMerStat(k, 1, 1.0, [1] * k))
    assert acc.qual.values() == [63] * 10 + [44] * 11


def test_probability_table():
    assert R.QUALITY_PROBS[0] == R.QUALITY_PROBS[2] == 0.25
    assert R.QUALITY_PROBS[3] == 1 - 10 ** -0.3 and R.QUALITY_PROBS[10] == 0.9 and R.QUALITY_PROBS[40] == 1 - 1e-4


def test_trimming():
    seq = "ACGTACGTAC"
    good = [30] * 10
    # nothing to trim
    assert R.trim_ns_and_bad_quality(seq, good, 4) == (seq, good, 0)
    # right trim alone: applied
    assert R.trim_ns_and_bad_quality(seq, [30] * 8 + [4, 2], 4) == (seq[:8], [30] * 8, 0)
    # left trim alone
    assert R.trim_ns_and_bad_quality(seq, [4, 0] + [30] * 8, 4) == (seq[2:], [30] * 8, 2)
    # a left trim of 3 suppresses the right trim: rtrim = 7 is not < 7 - 3 - 1
    q = [2, 2, 2] + [30] * 5 + [3, 3]
    assert R.trim_ns_and_bad_quality(seq, q, 4) == (seq[3:], q[3:], 3)
    # ... but a short enough right end is still cut: size 20, ltrim 1, rtrim 9 < 19 - 1 - 1
    s20 = "ACGT" * 5
    q20 = [0] + [30] * 9 + [1] * 10
    assert R.trim_ns_and_bad_quality(s20, q20, 4) == (s20[1:10], [30] * 9, 1)
    # N counts as bad whatever its quality; all N and all bad leave nothing
    assert R.trim_ns_and_bad_quality("NNACGTACNN", good, 4) == ("ACGTACNN", [30] * 8, 2)
    assert R.trim_ns_and_bad_quality("N" * 10, good, 4) == ("", [], 0)
    assert R.trim_ns_and_bad_quality(seq, [4] * 10, 4) == ("", [], 0)


def test_generator_cases():
    k = 5
    # plain read: every position
    assert R.valid_starts("ACGTACGTAC", [30] * 10, k) == list(range(6))
    # shorter than k, all N
    assert R.valid_starts("ACGT", [30] * 4, k) == []
    assert R.valid_starts("NNNNNNNN", [30] * 8, k) == []
    # N-splitting: runs of 6, 4 and 5 bases
    s = "ACGTAC" + "N" + "ACGT" + "N" + "ACGTA"
    assert R.valid_starts(s, [30] * len(s), k) == [0, 1, 12]
    assert R.coalesce([0, 1, 12], k) == [(0, 6), (12, 5)]
    # the tail kept by the trimming quirk, at quality 3: part of the last k-mers; at quality 1: cut by end_
    s = "ACGTACGTACGT"
    assert R.valid_starts(s, [2] * 3 + [30] * 7 + [3] * 2, k) == [3, 4, 5, 6, 7]
    assert R.valid_starts(s, [2] * 3 + [30] * 7 + [1] * 2, k) == [3, 4, 5]
    # the search branch goes beyond end_: trimmed read = ACGNACGTA (9 = k + 4), N at 3, end_ = 7; the window [4, 9) is
    # emitted although it ends at 9 > end_, and nothing after it
    s = "TT" + "ACGNACGTA"
    q = [3, 3] + [30] * 7 + [1, 0]
    assert R.trim_ns_and_bad_quality(s, q, 4)[0] == "ACGNACGTA"
    got = R.valid_kmers(s, q, k)
    assert [(g[0], g[1], g[2]) for g in got] == [(6, "ACGTA", [30, 30, 30, 1, 0])]
    assert got[0][3] == (1 - 1e-3) ** 3 * 0.25 * 0.25
    # without the N the same read stops at end_: starts 0..2 of the trimmed read
    assert R.valid_starts("TT" + "ACGTACGTA", q, k) == [2, 3, 4]


def test_rolled_probability_is_the_window_product_to_the_last_bits():
    rng = random.Random(5)
    s = "".join(rng.choice("ACGT") for _ in range(200))
    q = [rng.randrange(5, 42) for _ in s]
    for start, _, kq, cp in R.valid_kmers(s, q, 21):
        direct = 1.0
        for x in kq:
            direct *= R.QUALITY_PROBS[x]
        assert abs(cp - direct) <= 2 ** -45 * direct


def test_fill_pushes_both_strands_and_skips_foreign_kmers():
    k = 4
    data = R.fill_kmer_data([("ACGTT", [10, 20, 30, 40, 41])], k)
    # ACGT is its own reverse complement: merged twice, once with the qualities reversed
    assert data["ACGT"].count == 2 and data["ACGT"].qual.values() == [50, 50, 50, 50]
    assert data["CGTT"].count == 1 and data["CGTT"].qual.values() == [20, 30, 40, 41]
    assert data["AACG"].count == 1 and data["AACG"].qual.values() == [41, 40, 30, 20]
    assert sorted(data) == ["AACG", "ACGT", "CGTT"]
    only = R.fill_kmer_data([("ACGTT", [10, 20, 30, 40, 41])], k, kmer_set={"AACG"})
    assert sorted(only) == ["AACG"] and only["AACG"].count == 1
    f = np.float32(1 - 0.9 * 0.99 * 0.999 * 0.9999)
    assert data["ACGT"].factors == [f, f] and data["ACGT"].total_qual == np.float32(f * f)
    assert R.kmer_key("ACGT") == 0b11100100 and R.revcomp("AACG") == "CGTT"


@pytest.mark.parametrize("lo,hi", [(2, 41), (30, 41)])
def test_reference_float_product_is_inside_the_tolerance(lo, hi):
    """any order of float32 multiplications -- the reference's own spread -- stays inside the bound the GPU tests use"""
    rng = random.Random(lo)
    k = 21
    worst = Fraction(0)
    for _ in range(300):
        n = rng.randrange(1, 101)
        factors = []
        for _ in range(n):
            cp = 1.0
            for _ in range(k):
                cp *= R.QUALITY_PROBS[rng.randrange(lo, hi + 1)]
            assert 1 - cp >= 2 ** -10
            factors.append(np.float32(1 - cp))
        p, bound = R.total_qual_bound(factors)
        for _ in range(3):
            rng.shuffle(factors)
            t = np.float32(1.0)
            for f in factors:
                t = np.float32(t * f)
            err = abs(Fraction(float(t)) - p)
            assert err <= bound
            worst = max(worst, err / bound)
    assert worst < Fraction(1, 2)


def test_crafted_reads_take_the_corners():
    for k in (10, 11, 21, 22, 32):
        reads = {w: (s, q) for w, s, q in R.crafted_reads(k, np.random.default_rng(k))}
        n = k + 12
        assert R.valid_starts(*reads["left trim keeps the q=3 tail"], k) == list(range(3, n - k + 1))
        assert R.valid_starts(*reads["left trim keeps the q=1 tail"], k) == list(range(3, n - 2 - k + 1))
        assert R.valid_starts(*reads["right trim alone"], k) == list(range(0, n - 4 - k + 1))
        assert R.valid_starts(*reads["thresholds"], k) == list(range(0, n - k + 1))
        assert R.valid_starts(*reads["window beyond end_"], k) == [6]
        assert R.coalesce(R.valid_starts(*reads["N-splitting"], k), k) == [(0, k + 3), (k + 3 + 1 + k - 1 + 2, k),
                                                                          (3 * k + 6, 2 * k)]
        assert R.valid_starts(*reads["N at the ends"], k) == list(range(1, 7))
        assert R.valid_starts(*reads["exactly k"], k) == [0]
        for w in ("all N", "shorter than k after trimming", "shorter than k", "all bad"):
            assert R.valid_starts(*reads[w], k) == []


def test_fast_form_equals_the_line_for_line_form():
    rng = np.random.default_rng(9)
    k = 11
    genome = "".join(rng.choice(list("ACGT"), 120))
    reads = [(s, q) for _, s, q in R.crafted_reads(k, rng)]
    for st in rng.integers(0, 80, 150):
        s = genome[st:st + 40]
        s = R.revcomp(s) if rng.random() < 0.5 else s
        reads.append((s, [int(x) for x in rng.integers(2, 42, 40)]))
    slow = R.fill_kmer_data(reads, k)
    fast = R.fill_kmer_data_fast(reads, k)
    assert sorted(slow) == sorted(fast)
    assert max(st.count for st in slow.values()) > 20 and any(63 in st.qual.values() for st in slow.values())
    for km, st in slow.items():
        assert (st.count, st.qual.values(), st.factors) == fast[km]
