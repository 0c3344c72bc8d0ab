"""CPU: the sequential restatement of EarlyLowComplexityClipperProcessor (tests/atclip_restated.py) on small indices
whose outcome is worked out by hand.  The GPU parity tests (tests/test_gpu_atclip.py) compare against this restatement,
so it is pinned here first.  The indices come from the oracle's extension-index builder."""
import random

import pytest

from oracle import oracle as O
from tests import atclip_restated as R


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _index(reads, k):
    return R.Index.from_oracle(O.ExtIndex(reads, k, 1))


def _diff(before, ix):
    """{k-mer: (mask before, mask after)} of the stored k-mers that changed"""
    return {s: (a, b) for s, a, b in zip(ix.kmers, before, ix.masks) if a != b}


def _canon(s):
    return min(s, R.rc(s))


def test_ls_is_almost_equal_aware():
    one_ulp = 2.0 ** -52
    assert not R.ls(1.0, 1.0)
    assert not R.ls(1.0, 1.0 + 4 * one_ulp)  # within 4 ULPs: equal
    assert R.ls(1.0, 1.0 + 5 * one_ulp)
    assert R.ls(19.0, 20.0) and not R.ls(20.0, 20.0) and not R.ls(21.0, 20.0)
    assert 25 * 0.8 == 20.0 and 10 * 0.8 == 8.0  # the integral thresholds the boundary tests rely on


def test_kmer_strings_roundtrip():
    for k in (5, 21, 33, 77):
        s = _rand(random.Random(k), k)
        assert R.kmer_strings([O.kmer_words(s)], k) == [s]


def test_poly_a_junction_edge_removed():
    """P1|P2 -> A^21 -> C -> G...|T...: J1 = A^21 (two incoming) links to J2 = A^20 C (two outgoing), both junctions
    of low complexity (21 and 20 A >= 21 * 0.8): the link J1 -> J2 is collected from
    both of its orientations (2 edges) and removed once (2 links).  Nothing else is a junction of low complexity."""
    rng = random.Random(1)
    k = 21
    p1, p2 = _rand(rng, 30) + "G", _rand(rng, 30) + "T"
    s1, s2 = "G" + _rand(rng, 30), "T" + _rand(rng, 30)
    reads = [p1 + "A" * 21 + "C" + s1, p2 + "A" * 21 + "C" + s2]
    ix = _index(reads, k)
    j1, j2 = "A" * 21, "A" * 20 + "C"
    assert R.junction(ix.get(j1)) and R.junction(ix.get(j2))
    before = list(ix.masks)
    assert R.remove_at_edges(ix, 0.8) == (2, 2)
    d = _diff(before, ix)
    assert set(d) == {_canon(j1), _canon(j2)}
    assert ix.get(j1) == 0b11000000  # out C gone; in G and T kept
    assert ix.get(j2) == 0b00001100  # in A gone; out G and T kept
    assert R.remove_at_edges(ix, 0.8) == (0, 0)  # non-junctions are never touched: a second pass finds nothing


def _tip_reads(rng, tip, k=21):
    """main path M (complex, 80 bp) and a read leaving it after base 39 into `tip` (M[40] is not tip[0])"""
    m = _rand(rng, 40)
    m += "G" if tip[0] != "G" else "C"
    m += _rand(rng, 39)
    return m, [m, m[:40] + tip]


def test_short_poly_a_tip_isolated_with_junction_bases():
    """A tip of 6 A's off the complex junction x = M[19:40] (min_len 10): the counts take the 6 tip bases plus
    min_len - |tip| + 1 = 5 bases of x, x[k-1-i] for i = 5..9 = M[34..30].  With two A's there the maximal count is
    8 >= 10 * 0.8: the tip is isolated and x drops its link into it; with none it stays (6 < 8)."""
    k = 21
    for junction_a, expect in ((2, True), (0, False)):
        rng = random.Random(7)
        while True:
            m, reads = _tip_reads(rng, "A" * 6)
            if m[30:35].count("A") == junction_a and m[35:40].count("A") < 2 and m[39] != "A":
                break
        ix = _index(reads, k)
        x = m[19:40]
        assert R._POP[ix.get(x) & 15] == 2
        before = list(ix.masks)
        removed, links = R.remove_at_tips(ix, 0.8, 10, 200)
        if expect:
            tip = [(m[:40] + "A" * 6)[i:i + k] for i in range(20, 26)]
            assert (removed, links) == (6, 1)
            assert all(ix.get(t) == 0 for t in tip)
            assert ix.get(x) & 15 == 1 << R.IDX[m[40]]
            assert set(_diff(before, ix)) == {_canon(s) for s in tip + [x]}
        else:
            assert (removed, links) == (0, 0) and ix.masks == before


@pytest.mark.parametrize("tip,max_len,expect", [
    ("A" * 10, 200, 10),         # 10 A (+1 junction base): 10 >= 8, isolated
    ("AAGAAACAAT", 200, 0),      # 70 % A: 7 (+ at most 1 from the junction, which is no A) < 8, kept
    ("A" * 10, 5, 0),            # longer than max_len: the walk stops inside the tip, kept
])
def test_tip_composition_and_length(tip, max_len, expect):
    k = 21
    rng = random.Random(11)
    while True:
        m, reads = _tip_reads(rng, tip)
        if m[30] != "A" and m[39] != "A":
            break
    ix = _index(reads, k)
    before = list(ix.masks)
    removed, links = R.remove_at_tips(ix, 0.8, 10, max_len)
    assert removed == expect
    if expect:
        assert links == 1 and sum(1 for v in ix.masks if v == 0) == expect
    else:
        assert links == 0 and ix.masks == before


def test_short_isolated_edge_from_dead_start_kept():
    """An isolated read of 4 k-mers, nearly all A: its dead end walks back to a dead start, which is no tip."""
    k = 21
    ix = _index(["A" * 15 + "C" + "A" * 8], k)
    assert len(ix.kmers) == 4
    before = list(ix.masks)
    assert R.remove_at_tips(ix, 0.8, 10, 200) == (0, 0)
    assert R.remove_at_edges(ix, 0.8) == (0, 0)  # the junctions (dead start / dead end) lead to non-junctions
    assert ix.masks == before


@pytest.mark.parametrize("n_a,expect", [(20, (1, 2)), (19, (0, 0))])
def test_ls_boundary_at_integral_threshold(n_a, expect):
    """k = 25, ratio 0.8: the threshold is exactly 20.  J1 = A^n_a + a complex rest, joined by two branches on each
    side to J2 = J1 << G (two outgoing): with 20 A's J1 qualifies (ls(20, 20) is false) and its link to J2 goes; J2
    has 19 A's at most, so the reverse orientation is not collected: 1 edge, 2 links.  With 19 A's nothing goes."""
    k = 25
    rng = random.Random(25)
    rest = "CGTCGTCGTC"[:k - n_a]
    j1 = "A" * n_a + rest
    j2 = j1[1:] + "G"
    assert max(j2.count(c) for c in "ACGT") < 20
    p1, p2 = _rand(rng, 30) + "C", _rand(rng, 30) + "T"
    reads = [p1 + j1 + "G" + "A" + _rand(rng, 30), p2 + j1 + "G" + "T" + _rand(rng, 30)]
    ix = _index(reads, k)
    assert R.junction(ix.get(j1)) and R.junction(ix.get(j2))
    before = list(ix.masks)
    assert R.remove_at_edges(ix, 0.8) == expect
    if expect[0]:
        assert set(_diff(before, ix)) == {_canon(j1), _canon(j2)}
        assert not ix.get(j1) & (1 << R.IDX["G"]) and not ix.get(j2) & (1 << (4 + R.IDX["A"]))
    else:
        assert ix.masks == before
