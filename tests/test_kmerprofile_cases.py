"""CPU: the crafted inputs of tests/kmerprofile_cases.py really hold the classes they are named after, and the
restatement's integers over them tell a set of deliberately wrong winsorised sums apart from the right ones.  That is
the evidence that tests/test_gpu_kmerprofile_edges.py, which compares the device with the same integers, would notice
a kernel that is wrong in one of these ways."""
import math

import numpy as np
import pytest

from tests import kmerprofile_cases as K
from tests import kmerprofile_restated as R

KS = (21, 33, 65, 127)
COL = {cls: i for i, cls in enumerate(K.CLASSES)}
EXPECT_N = {"n2": 2, "n3": 3, "n19": 19, "n20": 20, "n21": 21, "n63": 63, "n65": 65, "n128": 128, "n1000": 1000,
            "lane63": 1, "alt40": 40, "alt64": 64, "late41": 41, "n127": 127, "short129": 129, "cut257": 257,
            "share70": 70, "share69": 69, "none": 0, "nopiece": 0, "rc127": 127}


def _columns(case):
    """{contig name: the N columns of the rows it finds, in contig order}"""
    out = {}
    for name, seq in case["contigs"]:
        found, _ = R.earmarks(seq, case["k"], case["table"])
        out[name] = [[row[s] for row in found] for s in range(case["N"])]
    return out


def index_bits(n, k):
    """PrefixIndex::build: the bits of word 0 a table of n keys is binned by, and the shift of a lookup"""
    b = 4
    while b < 24 and (1 << (b + 3)) < n:
        b += 1
    w0 = 2 * k if k <= 32 else 64
    bits = min(b, w0)
    return bits, w0 - bits


def _queries(case):
    k = case["k"]
    return [R.canonical(p[j:j + k]) for _, seq in case["contigs"] for p in R.split_on_ns(seq)
            for j in range(len(p) - k + 1)]


@pytest.mark.parametrize("eight", [False, True])
@pytest.mark.parametrize("k", KS)
def test_crafted_classes_are_present(k, eight):
    case = K.crafted(k, eight=eight)
    exp = dict(zip([name for name, _ in case["contigs"]], K.expected(case)))
    assert set(EXPECT_N) | {"mixed"} == set(exp)
    for name, n in EXPECT_N.items():
        assert exp[name][0] == n == case["n"][name], name
    assert {1, 2, 3, 19, 20, 21, 40, 41, 63, 64, 65, 127, 128, 129, 257, 1000} <= {e[0] for e in exp.values()}
    assert 100 < exp["mixed"][0] < 200 and exp["mixed"][1] == 300
    assert exp["share70"][1] == exp["share69"][1] == 100 and exp["lane63"][1] == 70
    assert exp["short129"][1] == 129 and exp["cut257"][1] == 257 and exp["nopiece"][1] == 0 and exp["none"][1] == 100
    assert exp["rc127"] == exp["n127"]
    assert len(R.split_on_ns(dict(case["contigs"])["cut257"])) == 5
    assert [len(p) - k + 1 for p in R.split_on_ns(dict(case["contigs"])["cut257"])] == [1, 63, 64, 65, 64]
    assert len(R.split_on_ns(dict(case["contigs"])["short129"])[1]) < k
    assert (len(case["contigs"]) * case["N"]) % 4 != 0  # the last block of the reduction holds idle waves
    top, t = (255, 70) if eight else (65535, 700)
    assert max(v for row in case["table"].values() for v in row) == top
    big_sq = 0
    for name, cols in _columns(case).items():
        n = len(cols[0])
        if n == 0:
            continue
        o = R.winsor_offset(n)
        assert set(cols[COL["equal"]]) == {30 if eight else 300} and set(cols[COL["zero"]]) == {0}
        assert max(cols[COL["low"]]) < (16 if eight else 256)
        s = sorted(cols[COL["straddle"]])
        if n >= 6:
            if eight:
                assert s[o] < 128 <= s[n - o - 1]
            else:
                assert s[o] < 256 <= s[n - o - 1] and (s[o] >> 8) != (s[n - o - 1] >> 8)
        s = sorted(cols[COL["ties"]])
        if n >= 4:
            assert s[o - 1] < s[o] == t and s[n - o - 1] == t + 1 < s[n - o]
        s = sorted(cols[COL["extremes"]])
        if n >= 3:
            assert s[:o] == [0] * o and s[n - o:] == [top] * o and 0 < s[o] and s[n - o - 1] < top
        if not eight:
            assert set(cols[COL["bytes"]]) <= {255, 256, 511, 512, 767, 768}
            big_sq += exp[name][3][COL["extremes"]] > 1 << 32
            if n == 2 or n >= 40:
                assert exp[name][3][COL["extremes"]] > 1 << 32, name
    assert eight or big_sq >= 10
    # the ties column of the longest contig: 64-lane rounds of one value and mixed rounds
    ties = _columns(case)["n1000"][COL["ties"]]
    rounds = [set(ties[b:b + 64]) for b in range(0, 1000, 64)]
    assert rounds[0] == {t} and rounds[2] == {t + 1} and len(rounds[1]) > 2 and len(rounds[-1]) > 2


@pytest.mark.parametrize("k", KS)
def test_crafted_keys_stress_the_lookup(k):
    case = K.crafted(k)
    keys, rows, kb, bb = K.table_files(case)
    nw = R.words(k)
    assert all(a < b for a, b in zip(keys, keys[1:])) and len(kb) == len(keys) * nw * 8 and len(bb) == len(keys) * 14
    assert [R.decode(key, k) for key in keys] == sorted(case["table"], key=R.encode)
    # the canonical strand is the smaller one base by base (kmer_less_nucl), which word order (key_less_words) contradicts
    # for some keys of more than one word; inside one word the two orders pick the same strand (base i of a k-mer
    # against the complement of base k - 1 - i, read from either end)
    assert any(R.encode(R.rc(km)) < R.encode(km) for km in case["table"]) == (nw > 1)
    queries = _queries(case)
    misses = [q for q in queries if q not in case["table"]]
    assert len(misses) > 400
    if nw > 1:  # misses that equal a key in every word but the last
        heads = {R.encode(q)[:-1] for q in misses}
        assert len(case["near"]) == 24 and all(R.encode(km)[:-1] in heads for km in case["near"])
    for n_keys in (1, 2, 129):
        small = K.restricted(case, n_keys)
        skeys = sorted(R.encode(km) for km in small["table"])
        assert len(skeys) == n_keys and sum(small["n"].values()) >= n_keys
        bits, shift = index_bits(n_keys, k)
        assert bits == (5 if n_keys == 129 else 4) and index_bits(128, k)[0] == 4
        qk = [R.encode(q) for q in queries]
        assert min(qk) < skeys[0] and max(qk) > skeys[-1]
        used = {key[0] >> shift for key in skeys}
        assert {key[0] >> shift for key in qk} - used  # queries into empty bins
        assert max(key[0] >> shift for key in qk) == (1 << bits) - 1  # the last bin reads pref[nbins]


@pytest.mark.parametrize("k", (21, 31, 32) + KS[1:])
def test_clustered_table_sits_in_one_bin(k):
    case = K.clustered(k)
    exp = K.expected(case)
    assert [e[0] for e in exp] == [100, 40] and exp[0][1] == 133 and exp[1][1] >= 40
    bits, shift = index_bits(len(case["table"]), k)
    assert len(case["table"]) == 140 and bits == 5
    assert len({R.encode(q)[0] >> shift for q in _queries(case)} | {R.encode(km)[0] >> shift for km in case["table"]}) == 1
    lo, hi = K.shared_bases(k)
    assert len({km[lo:hi] for km in case["table"]}) == 1 and 2 * (min(k, 32) - lo) == 24
    assert all(m not in case["table"] for m in case["miss"])
    if R.words(k) > 1:
        heads = {R.encode(km)[:-1] for km in case["table"]}
        assert sum(R.encode(m)[:-1] in heads for m in case["miss"]) >= 8
    assert any("N" + R.rc(km) in case["contigs"][1][1] for km in case["table"])  # pieces given as the other strand


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_small_k_tables(k):
    case = K.small_k(k)
    assert len(case["table"]) == {1: 2, 2: 5, 3: 32, 4: 68}[k]
    assert index_bits(len(case["table"]), k) == {1: (2, 0), 2: (4, 0), 3: (4, 2), 4: (4, 4)}[k]  # bits = min(4, 2k)
    exp = K.expected(case)
    assert [e[0] for e in exp] == [case["n"][name] for name, _ in case["contigs"]]
    assert max(e[0] for e in exp) >= 140 and exp[-1][:2] == (0, 0)
    if k % 2 == 0:
        assert any(e[0] < e[1] for e in exp)  # some k-mers are not in the table
    else:
        assert all(e[0] == e[1] for e in exp)


def test_the_tool_lines_of_the_crafted_contigs():
    case = K.crafted(33)
    text = R.run(case["contigs"], 33, case["table"], 7, var=True)
    lines = {line.split("\t")[0]: line.split("\t")[1:] for line in text.split("\n")[:-1]}
    assert "share70" in lines and "share69" not in lines and "none" not in lines and "nopiece" not in lines
    assert not R.ls(70 / 100, 0.7) and R.ls(69 / 100, 0.7)
    # n = 2 of the extremes column: both values become 65535, whose square no float32 holds
    c = 2 * COL["extremes"]
    assert lines["n2"][c] == "65535.00" and float(R.f32(65535 * 65535)) != 65535.0 * 65535.0
    assert lines["n2"][c + 1] == R.fixed2(R.f32(2 * 65535 * 65535) / R.f32(2) - np.float32(65535) * np.float32(65535))
    assert len(lines["n1000"]) == 15 and lines["n1000"][0] == "300.00" and lines["n1000"][1] == "0.00"


# ---- mutants ------------------------------------------------------------------------------------------------------------

def _sums(case, offset=R.winsor_offset, hi_rank=lambda n, o: n - o - 1, hi_first=True, project=lambda v: v, sq_mask=None,
          canon=R.canonical):
    """abundance_ints with the selection written as the device does it (ranks, then two clamps), every step replaceable"""
    k, out = case["k"], []
    for _, seq in case["contigs"]:
        found = []
        for p in R.split_on_ns(seq):
            for j in range(len(p) - k + 1):
                row = case["table"].get(canon(p[j:j + k]))
                if row is not None:
                    found.append(row)
        n, sums, sqs = len(found), [], []
        for s in range(case["N"]):
            v = [row[s] for row in found]
            if n >= 2:
                o = offset(n)
                ranked = sorted(project(x) for x in v)
                lo = ranked[min(max(o, 0), n - 1)]
                hi = ranked[min(max(hi_rank(n, o), 0), n - 1)]
                v = [max(min(x, hi), lo) for x in v] if hi_first else [min(max(x, lo), hi) for x in v]
            sums.append(sum(v))
            sq = sum(x * x for x in v)
            sqs.append(sq if sq_mask is None else sq & sq_mask)
        out.append((n, sums, sqs))
    return out


MUTANTS = {
    "offset o - 1": dict(offset=lambda n: R.winsor_offset(n) - 1),
    "offset o + 1": dict(offset=lambda n: R.winsor_offset(n) + 1),
    "offset in double": dict(offset=lambda n: int(math.ceil(n * float(np.float32(0.05))))),
    "hi = sorted[n - o]": dict(hi_rank=lambda n, o: n - o),
    "clamps in the other order": dict(hi_first=False),
    "selection on the low byte": dict(project=lambda v: v & 255),
    "32-bit sum of squares": dict(sq_mask=0xFFFFFFFF),
    "canonical strand by word order": dict(canon=lambda s: min(s, R.rc(s), key=R.encode)),
}


def _all_cases(k):
    return [K.crafted(k), K.crafted(k, eight=True), K.clustered(k)] + [K.restricted(K.crafted(k), n) for n in (1, 2, 129)]


@pytest.mark.parametrize("k", KS)
def test_clamp_form_equals_the_restatement(k):
    for case in _all_cases(k):
        assert _sums(case) == [(e[0], e[2], e[3]) for e in K.expected(case)]


def test_double_offset_differs_at_multiples_of_twenty():
    bad = [n for n in range(1, 5000) if MUTANTS["offset in double"]["offset"](n) != R.winsor_offset(n)]
    assert len(bad) == 249 and all(n % 20 == 0 for n in bad) and {20, 40, 1000} <= set(bad)


@pytest.mark.parametrize("name", sorted(MUTANTS))
@pytest.mark.parametrize("k", KS)
def test_mutants_are_told_apart(k, name):
    case = K.crafted(k)
    good, bad = _sums(case), _sums(case, **MUTANTS[name])
    names = [c for c, _ in case["contigs"]]
    differ = {(names[i], s) for i in range(len(good)) for s in range(case["N"])
              if (good[i][0], good[i][1][s], good[i][2][s]) != (bad[i][0], bad[i][1][s], bad[i][2][s])}
    if name == "canonical strand by word order" and R.words(k) == 1:
        assert not differ  # one word: both orders pick the same strand
        return
    assert differ, name
    if name == "clamps in the other order":
        assert {c for c, _ in differ} == {"n2"}  # lo > hi only there
    if name == "offset in double":
        assert {c for c, _ in differ} == {"n20", "alt40", "n1000"}
    if name in ("offset o - 1", "hi = sorted[n - o]"):
        assert {c for c, s in differ if s == COL["ties"]} >= {"n20", "n21", "alt64", "n65", "cut257", "n1000"}
    if name == "offset o + 1":  # stays inside the runs of the ties column; the distinct values of the others move
        assert {c for c, s in differ if s == COL["extremes"]} >= {"n20", "n21", "alt64", "n65", "cut257", "n1000"}
    if name == "32-bit sum of squares":
        assert all(s == COL["extremes"] for _, s in differ) or len(differ) > 10
    if name != "selection on the low byte" and name != "32-bit sum of squares":
        eight = K.crafted(k, eight=True)  # the one-pass kernel's profile tells them apart as well
        assert _sums(eight) != _sums(eight, **MUTANTS[name])
