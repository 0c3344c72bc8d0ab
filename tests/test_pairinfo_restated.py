"""CPU: the restatement of the paired-info stage (tests/pairinfo_restated.py) against answers derived by hand."""
import math
import random
import struct

from tests import gmapper_restated as G
from tests import pairinfo_restated as P
from tests.helpers import rc

K = 21


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _one_segment(seed=1, n=700):
    seg = _rand(random.Random(seed), n)
    return seg, G.Graph(K, ["3"], [seg], [])


def _chain(seed=2, n=900, cut=400):
    genome = _rand(random.Random(seed), n)
    return genome, G.Graph(K, ["3", "5"], [genome[:cut], genome[cut - K:]], [(0, "+", 1, "+")])


def _fragment_pair(genome, a, F, l1, l2):
    """the mates of the fragment genome[a:a + F) as a sequencer writes an fr library"""
    return genome[a:a + l1], rc(genome[a + F - l2:a + F])


def _run(g, pairs, orientation, insert_size, round_distance=0, threshold=0):
    lib = P.Library(g)
    lib.push_estimate(pairs, orientation)
    lib.push_fill(pairs, orientation, insert_size, round_distance, threshold)
    return lib


def test_one_segment_fragment_gives_is_and_distance():
    seg, g = _one_segment()
    L = g.length(0)
    for a, F, l1, l2, I in [(50, 400, 150, 150, 380), (10, 300, 100, 140, 300), (200, 250, 60, 90, 410), (5, 180, 150, 150, 200)]:
        lib = _run(g, [_fragment_pair(seg, a, F, l1, l2)], P.FR, I)
        assert lib.hist() == [(F, 1)]
        assert (lib.is_counter.total, lib.is_counter.mapped, lib.is_counter.negative) == (1, 1, 0)
        # one point with d = insert_size - F; it is stored with gap = d - length(e1).  Both mates lie on edge 0, whose
        # pair (0, 0) is smaller than its conjugate (1, 1)
        assert lib.points() == [(0, 0, I - F - L, 1)]


def test_chain_pair_spanning_the_link():
    genome, g = _chain()
    a, F, l1, l2, I = 200, 420, 150, 150, 400  # the first mate ends at 350 < 400; the second starts at 470 >= 400 - k
    lib = _run(g, [_fragment_pair(genome, a, F, l1, l2)], P.FR, I)
    assert lib.hist() == [] and lib.is_counter.mapped == 0  # the mates lie on different edges
    assert lib.counts.edge_pairs() == 1
    # d = length(e1) + insert_size - F, so gap = insert_size - F; (0, 2) < (conj 2, conj 0) = (3, 1)
    assert lib.points() == [(0, 2, I - F, 1)]
    # the same pair from the other strand is the pair (3, 1): stored under its conjugate (0, 2), same gap
    first, second = _fragment_pair(genome, a, F, l1, l2)
    lib2 = _run(g, [(second, first)], P.FR, I)
    assert lib2.points() == [(0, 2, I - F, 1)] and lib2.index.under_conjugate == 1


def test_pair_on_edge_and_its_conjugate_weighs_two():
    seg, g = _one_segment()
    # ff: the second mate is read from the reverse strand, so path2 lies on edge 1 = conj 0
    first, second = seg[100:250], rc(seg[300:450])
    lib = _run(g, [(first, second)], P.FF, 400)
    (e1, e2, _, w), = lib.points()
    assert (e1, e2, w) == (0, 1, 2)
    assert lib.hist() == []  # different edges: no insert size
    # the filter counts such a pair twice per occurrence: c = 2 passes threshold 1 but not 2
    assert lib.counts.c(0, 1) == 2
    assert _run(g, [(first, second)], P.FF, 400, threshold=1).points() == lib.points()
    assert _run(g, [(first, second)], P.FF, 400, threshold=2).points() == []


def test_cut_before_first_mate_moves_is():
    seg, g = _one_segment()
    first, second = _fragment_pair(seg, 50, 400, 150, 150)
    assert _run(g, [(first, second)], P.FR, 400).hist() == [(400, 1)]
    lib = _run(g, [("NNN" + first, second)], P.FR, 400)
    assert P.present("NNN" + first, second, P.FR)[0] == (first, 3, 0)
    assert lib.hist() == [(403, 1)]
    # a cut after the second mate in the file is a cut before it once fr has turned it: it does not enter the trim
    assert _run(g, [(first, second + "N")], P.FR, 400).hist() == [(400, 1)]
    assert _run(g, [(first, "NN" + second)], P.FR, 400).hist() == [(402, 1)]
    # rf turns the first mate: its right cut becomes the left offset
    a, b = P.present(first + "NNNN", second, P.RF)
    assert a == (rc(first), 4, 0) and b == (second, 0, 0)


def test_orientations_present_the_mates():
    a, b = "ACGTTGCA" + "A", "GGGTTTCC" + "C"
    assert [P.present(a, b, o)[0][0] for o in (P.FF, P.FR, P.RF, P.RR)] == [a, a, rc(a), rc(a)]
    assert [P.present(a, b, o)[1][0] for o in (P.FF, P.FR, P.RF, P.RR)] == [b, rc(b), b, rc(b)]
    assert P.longest_valid("NNACGNACGTN") == ("ACGT", 6, 1)
    assert P.longest_valid("ACGNACG") == ("ACG", 0, 4)  # the first of two equally long stretches
    assert P.longest_valid("NNN") == ("", 0, 0)


def test_statistics_by_hand():
    # {100: 1}: the median is 100 (the sum left after 100 is 0 <= 1 / 2), the deviations are {0: 1}, so mad = 0 and
    # the crop keeps [100, 100].  mean = 100, deviation = sqrt(10000 - 10000) = 0; n = 1 makes every scaled quantile
    # int(q / 100) = 0, and no percentile is set.  S = 1: the first key has cS = 0 <= lval, so the interval is (100, 100)
    h1 = {100: 1}
    assert P.find_median(h1) == (100.0, 0.0, {100: 1})
    assert P.find_mean(h1) == (100.0, 0.0, {})
    assert P.get_is_interval(0.8, h1) == (100.0, 100.0)
    # {10: 1, 20: 2, 30: 1}: S = 4; after 10 the sum is 3 > 2, after 20 it is 1 <= 2: median 20.  Deviations: 10 -> 1,
    # 0 -> 2, then 10 -> 1 again (the reference assigns): {0: 2, 10: 1}, S = 3, after 0 the sum is 1 <= 1.5: mad 0.  The
    # crop keeps {20: 2}.  mean 20, deviation 0, n = 2: int(q / 100 * 2) is 0 below 50 and 1 from 50 on; the key 20 takes
    # m from 0 to 2, so the percentiles 50 .. 95 are 20
    h2 = {10: 1, 20: 2, 30: 1}
    assert P.get_median(h2) == 20.0 and P.get_mad(h2, 20.0) == 0.0
    assert P.find_median(h2) == (20.0, 0.0, {20: 2})
    assert P.find_mean(h2) == (20.0, 0.0, {q: 20 for q in range(50, 100, 5)})
    # {100: 3, 110: 2, 120: 3, 1000: 1}: S = 9; 6, then 4 <= 4.5: median 110.  Deviations {10: 3, 0: 2, 890: 1} (10 is
    # assigned twice), S = 6; 4 > 3, then 1 <= 3: mad 10.  The crop is 110 -+ 74.13: {100: 3, 110: 2, 120: 3}, whose
    # median is 110 (S = 8: 5, then 3 <= 4) and whose mad is 10 ({0: 2, 10: 3}: 3 > 2.5, then 0).
    # Mean over the same crop: n = 8, sum = 880, mean 110; sum2 = 97400, 97400 / 8 - 12100 = 75: deviation sqrt(75);
    # 110 -+ 5 sqrt(75) keeps the same keys.  int(q / 100 * 8) = 0 0 1 1 2 2 2 3 3 4 4 4 5 5 6 6 6 7 7; 100 takes m from 0
    # to 3 (the quantiles scaled to 1, 2, 3), 110 to 5 (4, 5), 120 to 8 (6, 7); 5 and 10 scale to 0 and stay unset.
    # Interval: S = 8, lval = 0.8, rval = 7.2: 100 (cS 0) sets the minimum, 110 (cS 3) and 120 (cS 5) the maximum
    h3 = {100: 3, 110: 2, 120: 3, 1000: 1}
    crop = {100: 3, 110: 2, 120: 3}
    assert P.find_median(h3) == (110.0, 10.0, crop)
    mean, dev, pc = P.find_mean(h3)
    assert (mean, dev) == (110.0, math.sqrt(75.0))
    assert [pc.get(q, 0) for q in range(5, 100, 5)] == [0, 0] + [100] * 7 + [110] * 5 + [120] * 5
    assert P.get_is_interval(0.8, crop) == (100.0, 120.0)
    # CollectLibInformation: ok needs mapped > 0 and median >= k + 2
    c = P.InsertSizeCounter(None, 0)
    assert not P.estimate(c, K, 0)["ok"]
    c.hist, c.mapped, c.total = dict(h3), 9, 9
    st = P.estimate(c, K, 5)
    assert st["ok"] and (st["left_quantile"], st["right_quantile"], st["edge_pairs"]) == (100.0, 120.0, 5)
    c.hist = {K + 1: 4}
    assert not P.estimate(c, K, 0)["ok"] and P.estimate(c, K, 0)["median"] == K + 1


def test_integer_rounding_equals_the_double_form():
    for r in (2, 3, 4, 5, 8):
        for d in range(-3 * r, 3 * r + 1):
            assert P.round_distance_int(d, r) == P.round_distance_double(d, r), (d, r)
    assert [P.round_distance_double(d, 2) for d in (-3, -1, 1, 3)] == [-4, -2, 2, 4]  # half away from zero
    assert [P.round_distance_double(d, 5) for d in (-8, -7, 7, 8)] == [-10, -5, 5, 10]


def test_filter_counts_both_orientations():
    genome, g = _chain()
    first, second = _fragment_pair(genome, 200, 420, 150, 150)
    # one occurrence of (0, 2) and one of (3, 1), its conjugate: c = 2 for either
    lib = _run(g, [(first, second), (second, first)], P.FR, 400, threshold=1)
    assert lib.counts.edge_pairs() == 2 and lib.counts.c(0, 2) == 2 and lib.counts.c(3, 1) == 2
    assert lib.points() == [(0, 2, -20, 2)]
    assert _run(g, [(first, second), (second, first)], P.FR, 400, threshold=2).points() == []
    # three occurrences saturate the 2-bit cell: threshold 2 passes, threshold 3 never does
    three = [(first, second)] * 3
    assert _run(g, three, P.FR, 400, threshold=2).points() == [(0, 2, -20, 3)]
    assert _run(g, three * 4, P.FR, 400, threshold=3).points() == []


def test_prd_bytes():
    f = lambda gap, w: struct.pack("<ff", gap, w)  # noqa: E731
    pts = [(0, 2, 5, 1), (0, 2, 7, 3), (4, 4, -1, 2)]
    assert P.prd_bytes(pts) == (b"\x02" + b"\x01" + b"\x03\x02" + f(5, 1) + f(7, 3) + b"\x00" +
                                b"\x05" + b"\x05\x01" + f(-1, 2) + b"\x00")
    assert P.prd_bytes([]) == b"\x00"
    assert P.uleb128(300) == b"\xac\x02"  # an id above 127 takes two bytes
