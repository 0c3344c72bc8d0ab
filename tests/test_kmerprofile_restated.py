"""CPU: pins tests/kmerprofile_restated.py (the restatement the GPU tests of the k-mer profile engine compare with) on
cases worked out by hand from the reference's source."""
import struct

import numpy as np

from tests import kmerprofile_restated as R


def test_encoding_and_canonical_strand():
    assert R.encode("ACGT") == (0 | 1 << 2 | 2 << 4 | 3 << 6,)
    k33 = "A" * 32 + "T"
    assert R.encode(k33) == (0, 3) and R.decode(R.encode(k33), 33) == k33
    assert R.canonical("CGT") == "ACG" and R.canonical("ACG") == "ACG" and R.canonical("ACGT") == "ACGT"
    assert R.kmers_bytes([(1, 2)]) == struct.pack("<QQ", 1, 2)
    assert R.bpr_bytes([[1, 0, 65535]]) == struct.pack("<HHH", 1, 0, 65535)


def test_sample_filter():
    keys = [(1,), (2,), (3,), (4,)]
    assert R.filter_sample(keys, [1, 2, 255, 300]) == [((2,), 2), ((3,), 255), ((4,), 255)]
    assert R.filter_sample(keys, [1, 2, 255, 300], ci=1, cs=1000) == [((1,), 1), ((2,), 2), ((3,), 255), ((4,), 300)]


def test_keep_rule_boundaries():
    a = [((1,), 5), ((2,), 6), ((3,), 1)]
    b = [((3,), 1), ((4,), 5)]
    # total == min_mult in one sample is dropped, min_mult + 1 is kept; two samples keep any total
    assert R.join([a, b], 1, 5) == ([(2,), (3,)], [[6, 0], [1, 1]])
    assert R.join([a, b], 2, 5) == ([(3,)], [[1, 1]])
    assert R.join([a, b], 3, 5) == ([], [])
    assert R.join([a, b], 0, 4) == ([(1,), (2,), (3,), (4,)], [[5, 0], [6, 0], [1, 1], [0, 5]])
    assert R.join([a, []], 1, 0) == ([(1,), (2,), (3,)], [[5, 0], [6, 0], [1, 0]])
    assert R.join([[], []], 0, 0) == ([], [])
    # word 0 is the most significant one
    assert R.join([[((1, 0), 9)], [((0, 5), 9)]], 1, 5)[0] == [(0, 5), (1, 0)]


def test_winsor_offset_steps():
    assert [R.winsor_offset(n) for n in (1, 2, 3, 20, 21, 40, 41, 100, 101)] == [1, 1, 1, 1, 2, 2, 3, 5, 6]


def test_winsorised_vectors():
    assert R.winsorised([7]) == [7]
    assert R.winsorised([9, 3]) == [9, 9]  # v[0] = v[1], then v[1] = v[0]
    assert R.winsorised([9, 1, 5]) == [5, 5, 5]
    v20 = R.winsorised(range(1, 21))
    assert v20 == [2] + list(range(2, 20)) + [19] and sum(v20) == 210
    v21 = R.winsorised(range(21, 0, -1))
    assert v21 == [3, 3] + list(range(3, 20)) + [19, 19] and sum(v21) == 231
    assert R.winsorised([4] * 10) == [4] * 10
    assert R.winsorised([1, 4, 4, 4, 4, 4, 4, 4, 4, 9]) == [4] * 10
    # for n >= 3 the in-place loop is a clamp to [sorted[o], sorted[n - o - 1]]
    rng = np.random.default_rng(1)
    for n in (3, 19, 20, 21, 64, 65, 200):
        v = [int(x) for x in rng.integers(0, 300, n)]
        s, o = sorted(v), R.winsor_offset(n)
        assert R.winsorised(v) == sorted(max(min(x, s[n - o - 1]), s[o]) for x in v)


def test_ls_is_four_ulps_wide():
    x = 0.7
    near = x
    for _ in range(4):
        near = float(np.nextafter(near, 0.0))
    assert not R.ls(near, x) and R.ls(float(np.nextafter(near, 0.0)), x)
    assert not R.ls(x, x) and not R.ls(0.8, x) and R.ls(0.0, x)
    assert not R.ls(float("nan"), x)


def test_fixed_precision_two_of_float32():
    assert R.fixed2(np.float32(2.675)) == "2.67"  # 2.67499995...
    assert R.fixed2(0.125) == "0.12" and R.fixed2(0.375) == "0.38"  # exact ties go to even, as printf does
    assert R.fixed2(np.float32(1) / np.float32(3)) == "0.33"
    assert R.fixed2(-0.001) == "-0.00"
    assert R.fixed2(R.f32(16777217)) == "16777216.00"  # the sum is rounded to float32 before the division


def test_profile_line_share_and_values():
    # 10 positions: a share of exactly 0.7 is not "less"
    assert R.profile_line("c", 30, 21, 7, [7], [7]) == "c\t1.00\t\n"
    assert R.profile_line("c", 30, 21, 6, [6], [6]) is None
    assert R.profile_line("c", 30, 21, 10, [25], [70]) == "c\t2.50\t\n"
    assert R.profile_line("c", 30, 21, 10, [25], [70], var=True) == "c\t2.50\t0.75\t\n"
    assert R.profile_line("n", 30, 21, 10, [25, 1], [70, 1], var=True) == "n\t2.50\t0.75\t0.10\t0.09\t\n"
    assert R.profile_line("short", 20, 21, 0, [0], [0]) is None  # 0 / 0 in the reference
    assert R.profile_line("shorter", 5, 21, 0, [0], [0]) is None  # size_t wraps: a share of 0


def test_abundance_of_a_small_contig():
    table = {"ACG": [5, 0], "AAC": [2, 7]}
    assert R.split_on_ns("acgNNxAC") == ["ACG", "AC"]
    # ACG and CGT (its reverse complement) both find the row; the stretch AC is shorter than k
    assert R.abundance_ints("ACGTNAC", 3, table, 2) == (2, 2, [10, 0], [50, 0])
    assert R.abundance_ints("ACGTTGGG", 3, table, 2) == (3, 6, [15, 0], [75, 0])  # rows [5,0] [5,0] [2,7]: n = 3
    contigs = [("a x", "ACGT"), ("b", "AC"), ("c", "ACGT")]
    assert R.run(contigs, 3, table, 2) == "a x\t5.00\t0.00\t\nc\t5.00\t0.00\t\n"
    assert R.run(contigs, 3, table, 2, min_len=3) == "a x\t5.00\t0.00\t\n"  # b ends the run
    assert R.run([("g", "ACGTTGGG")], 3, table, 2) == ""  # 3 of 6 positions
