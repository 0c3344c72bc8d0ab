"""CPU: the host arithmetic of the paired stage (csrc/pairinfo_host.hpp, csrc/edge_ops.h), built into a stand-alone program
with AddressSanitizer + UBSan (tests/pairinfo_host_check.cpp; nothing is loaded into python), against the restatements
(tests/pairinfo_restated.py, tests/distest_restated.py) and the values recorded from the reference
(tests/golden/graph_ref/)."""
import os
import struct
import subprocess

import pytest

from tests import distest_cases as Cs
from tests import distest_restated as D
from tests import graph_ref_case as C
from tests import pairinfo_restated as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
K = 21


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("pairinfo") / "pairinfo_host_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", path, os.path.join(ROOT, "tests", "pairinfo_host_check.cpp")])
    return path


def _run(exe, text):
    """the output lines of the program, by their first word"""
    r = subprocess.run([exe], input=text + "\n", capture_output=True, text=True, env=ENV, timeout=60)
    assert r.returncode == 0 and r.stdout.endswith("PAIRINFO-HOST-OK\n"), (r.stdout[-300:], r.stderr[-2000:])
    out = {}
    for ln in r.stdout.splitlines()[:-1]:
        out.setdefault(ln.split()[0], []).append(ln.split()[1:])
    return out


def dbits(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", x))[0]


def _points_text(cmd, pts):
    return "%s %d\n" % (cmd, len(pts)) + "".join("%d %d %d %d\n" % p for p in pts)


def _graph_text(g):
    ns = len(g.names)
    return "graph %d\n" % ns + "".join("%d %d\n" % (g.length(2 * s), g.conj[2 * s] == 2 * s) for s in range(ns))


# ---- statistics ---------------------------------------------------------------------------------------------------------

def _stats(exe, hist, k=K):
    row, = _run(exe, "stats %d %d\n" % (k, len(hist)) + "".join("%d %d\n" % kv for kv in sorted(hist.items())))["S"]
    return dict(mean=row[0], deviation=row[1], median=row[2], mad=row[3], interval=row[4:6],
                percentiles=[int(x) for x in row[6:25]], ok=int(row[25]))


def _restated_stats(hist, k=K):
    c = P.InsertSizeCounter(None, 0)
    c.hist, c.mapped, c.total = dict(hist), sum(hist.values()), sum(hist.values())
    st = P.estimate(c, k, 0)
    return dict(mean=dbits(st["mean"]), deviation=dbits(st["deviation"]), median=dbits(st["median"]), mad=dbits(st["mad"]),
                interval=[dbits(st["left_quantile"]), dbits(st["right_quantile"])], percentiles=st["percentiles"],
                ok=int(st["ok"]))


@pytest.mark.parametrize("case", C.READS)
def test_statistics_equal_the_reference(exe, case):
    fx = C.load(case)
    ref = fx["ref"]["is"]
    got = _stats(exe, {k: v for k, v in ref["hist"]}, fx["k"])
    pc = dict(tuple(x) for x in ref["percentiles"])
    assert (got["mean"], got["deviation"], got["median"], got["mad"]) == (ref["mean"], ref["deviation"], ref["median"], ref["mad"])
    assert got["interval"] == ref["interval"]
    assert got["percentiles"] == [pc.get(q, 0) for q in range(5, 100, 5)]
    assert got["ok"] == 1


# the hand histogram of test_pairinfo_restated.test_statistics_by_hand, then the degenerate ones: one key; two keys with
# equal counts; a median below k + 2 (no interval, not ok); everything but the median's key cropped.  (No histogram has
# every key cropped: the median is a key, and mad >= 0 keeps it inside [median - c * mad, median + c * mad].)
@pytest.mark.parametrize("hist", [{100: 3, 110: 2, 120: 3, 1000: 1}, {10: 1, 20: 2, 30: 1}, {100: 1}, {300: 7}, {200: 4, 260: 4},
                                  {K + 1: 4}, {5: 2, 22: 1, 400: 1}, {250: 9, 1: 1, 90000: 1, 2000000000: 1}])
def test_statistics_equal_the_restatement(exe, hist):
    assert _stats(exe, hist) == _restated_stats(hist)


def test_statistics_by_hand_values(exe):
    got = _stats(exe, {100: 3, 110: 2, 120: 3, 1000: 1})
    assert (got["mean"], got["deviation"], got["median"], got["mad"]) == (dbits(110.0), dbits(75.0 ** 0.5), dbits(110.0), dbits(10.0))
    assert got["interval"] == [dbits(100.0), dbits(120.0)] and got["ok"] == 1
    assert got["percentiles"] == [0, 0] + [100] * 7 + [110] * 5 + [120] * 5
    assert _stats(exe, {K + 1: 4})["ok"] == 0


# ---- rounding, threshold ------------------------------------------------------------------------------------------------

def test_pi_round_equals_the_double_form(exe):
    cases = [(d, r) for r in (1, 2, 5) for d in range(-12, 13)] + [(s * (2 ** 31 - 1), r) for s in (1, -1) for r in (1, 2, 5)]
    got = _run(exe, "round %d\n" % len(cases) + "".join("%d %d\n" % c for c in cases))["R"]
    assert [int(x[0]) for x in got] == [P.round_distance_double(d, r) for d, r in cases]


def test_least_half_unit_weight(exe):
    """the least weight w (half-units) with math::ge(w / 2, t).  At 1e19 no weight of 64 bits passes (2^63 < 1e19 by more
    than 4 ULPs): the smallest w is beyond 2^64, and the library answers 2^64 - 1, the largest threshold a weight can be
    compared with"""
    ts = [0.0, 0.5, 2.0] + [C.ulps_above(2.0, n) for n in (-4, -1, 1, 4)] + [C.ulps_above(2.0, n) for n in (-5, 5)] + [1e19]
    got = _run(exe, "threshold %d\n" % len(ts) + "".join(dbits(t) + "\n" for t in ts))["T"]
    for t, w in zip(ts, got):
        if not D.ge(float(2 ** 64 - 1) / 2, t):
            assert t == 1e19 and int(w[0]) == 2 ** 64 - 1
        else:
            assert int(w[0]) == next(x for x in range(10) if D.ge(x / 2, t)), t
    assert [int(w[0]) for w in got[:3]] == [0, 1, 4]


# ---- points -------------------------------------------------------------------------------------------------------------

def test_canonicalise_and_merge(exe):
    b, (A, Pl, Q) = Cs.hairpin()
    g = b.graph()
    # the hairpin points of test_distest_restated.test_host_search_hand_cases_and_limits, unsorted, with (Pl, conj A) also
    # under its other form (A, Pl), (A, Q) also as (conj Q, conj A), a point given twice, and the self-conjugate Pl
    pts = [(Pl, A + 1, 0, 5), (A, Q, 0, 2), (A, A + 1, 41, 3), (g.conj[Q], g.conj[A], 0, 7), (Pl, Pl, -41, 2), (A, Pl, 0, 5),
           (A, A + 1, 41, 1), (A, Q, -3, 1)]
    got = _run(exe, _graph_text(g) + _points_text("canon", pts))["P"]
    want = D.canonical_points(g, pts)
    assert [tuple(int(x) for x in row) for row in got[:-1]] == want and got[-1] == ["end"]
    assert want == [(A, A + 1, 41, 4), (A, Pl, 0, 10), (A, Q, -3, 1), (A, Q, 0, 9), (Pl, Pl, -41, 2)]


def _grouping(pts):
    pairs = sorted({p[:2] for p in pts})
    firsts = sorted({p[0] for p in pts})
    return ([p[0] for p in pairs], [p[1] for p in pairs], [[q[:2] for q in pts].index(p) for p in pairs] + [len(pts)],
            [[p[0] for p in pairs].index(e) for e in firsts] + [len(pairs)])


@pytest.mark.parametrize("pts", [[], [(4, 6, -1, 2)], [(0, 2, 5, 1), (0, 2, 7, 3), (0, 5, 1, 1), (4, 4, -1, 2)],
                                 [(2 * e, e + 1, g, 1) for e in range(65) for g in range(1 + e % 3)]],
                         ids=["none", "one", "two-pairs-one-first", "65-firsts"])
def test_grouping(exe, pts):
    got = _run(exe, _points_text("group", pts))["G"]
    assert [row[0] for row in got] == ["pe1", "pe2", "ppt", "grp"]
    assert tuple([int(x) for x in row[1:]] for row in got) == _grouping(pts)


# ---- the writer ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pts", [[(0, 2, 5, 1), (0, 2, 7, 3), (4, 4, -1, 2)], [], [(299, 0, -7, 1), (299, 511, 2, 3), (300, 1, 0, 16777216)]],
                         ids=["prd_bytes", "empty", "two-byte-ids"])
def test_raw_writer(exe, pts):
    got, = _run(exe, _points_text("raw", pts))["W"]
    assert bytes.fromhex(got[0] if got else "") == P.prd_bytes(pts)
    if not pts:
        assert got == ["00"]


def _clustered_bytes(exe, c):
    text = "clustered %d\n" % len(c.records) + "".join(
        "%d %d %08x %d %d\n" % (e1, e2, struct.unpack("<I", struct.pack("<f", centre))[0], w, c.g.length(e1))
        for e1, e2, centre, _, w in c.records)
    got, = _run(exe, text)["W"]
    return bytes.fromhex(got[0])


def test_clustered_writer(exe):
    b, (A, M, B) = Cs.single_path()
    g = b.graph()
    c = D.Clustering(g, [(A, B, 48, 3), (A, B, 55, 2)], Cs.params())  # the points of test_file_layout
    assert _clustered_bytes(exe, c) == c.file_bytes() == bytes([1, A + 1, B + 1, 1]) + struct.pack("<ff", 50.0, 5.0) + bytes([0])
    assert _clustered_bytes(exe, D.Clustering(g, [], Cs.params())) == b"\x00"
    # a tie hands an odd weight's halves out: 1.5 a side (the bubble of test_bubble_ties_drops_and_linkage, d = 145)
    b, (A, arms, B) = Cs.bubble()
    c = D.Clustering(b.graph(), [(A, B, 45, 3)], Cs.params(threshold=0.5))
    assert [r[4] for r in c.records] == [3, 3] and _clustered_bytes(exe, c) == c.file_bytes()
    # a larger index; with a linkage distance, centres at .5
    g = Cs.random_graph(0).graph()
    c = D.Clustering(g, Cs.random_points(g, 0), Cs.params(linkage=5, threshold=0.5))
    assert len(c.records) > 50 and any(r[2] != int(r[2]) for r in c.records)
    assert _clustered_bytes(exe, c) == c.file_bytes()


# ---- pair_is_self_conj --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["hairpin", "random"])
def test_pair_is_self_conj(exe, which):
    g = (Cs.hairpin()[0] if which == "hairpin" else Cs.random_graph(2)).graph()
    got = {(int(a), int(b)): int(x) for a, b, x in _run(exe, _graph_text(g) + "selfconj\n")["C"]}
    edges = sorted(g.seq)
    assert sorted(got) == [(a, b) for a in edges for b in edges]
    assert got == {(a, b): int((g.conj[b], g.conj[a]) == (a, b)) for a in edges for b in edges}
    assert sum(got.values()) == len(edges)  # every edge has exactly one partner
    assert any(g.conj[e] == e for e in edges)
