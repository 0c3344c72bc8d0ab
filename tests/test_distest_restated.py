"""CPU: the restatement of the distance-estimation stage (tests/distest_restated.py) against answers derived by hand, its
literal search against the order-free walk-length set, and the library's host search (csrc/distest_host.hpp, built into a
stand-alone program with AddressSanitizer + UBSan; nothing is loaded into python) against the restatement."""
import os
import struct
import subprocess

import pytest

from tests import distest_cases as Cs
from tests import distest_restated as D
from tests import gmapper_restated as G
from tests import pairinfo_restated as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")


def _records(g, points, p, **kw):
    return D.Clustering(g, D.canonical_points(g, points), p, **kw).records


def test_library_params():
    p = D.library_params(399.5, 40.9, 100)
    assert (p.insert_size, p.delta, p.linkage_distance, p.max_distance, p.filter_threshold) == (400, 40, 0, 81, 2.0)
    assert D.library_params(399.49, 40.9, 100, 0.5).insert_size == 399
    assert D.library_params(399.49, 40.9, 100, 0.5).linkage_distance == 20
    assert p.gap == 200 and D.upper_bound(21, 400, 40) == 417 and D.upper_bound(21, 20, 3) is None
    assert D.lower_bound(21, 100, 41, 200, 40) == 42 and D.lower_bound(21, 100, 100, 200, 40) == 0


def test_single_path():
    b, (A, M, B) = Cs.single_path()
    g = b.graph()
    # the one walk from EdgeEnd(A) to EdgeStart(B) is M: distance 100 + 50; both points are within 80 of it
    c = D.Clustering(g, [(A, B, 48, 3), (A, B, 55, 2)], Cs.params())
    assert c.lengths == {(A, B): [150]} and c.calls == {(A, B): 2}
    assert c.records == [(A, B, 150.0, 0.0, 10)]
    # given under the conjugate pair, the points land under the same canonical pair
    assert _records(g, [(g.conj[B], g.conj[A], 48, 3), (A, B, 55, 2)], Cs.params()) == c.records
    # a cluster of weight 1.5 < 2 is filtered, one of weight 2 stays
    assert _records(g, [(A, B, 48, 1)], Cs.params()) == []
    assert _records(g, [(A, B, 48, 2)], Cs.params()) == [(A, B, 150.0, 0.0, 4)]
    assert _records(g, [(A, B, 48, 1)], Cs.params(threshold=0.5)) == [(A, B, 150.0, 0.0, 2)]


def test_bubble_ties_drops_and_linkage():
    b, (A, arms, B) = Cs.bubble()
    g = b.graph()
    # distances 130, 160, 330.  d = 130: 4 to 130.  d = 145: halfway, 1 to each.  d = 158: 3 to 160.  d = 245: halfway
    # between 160 and 330 but 85 > 80 from both: dropped.  d = 420: 90 from 330: dropped; it keeps 330 inside
    # [130 - 80, 420 + 80], so 330 comes out with weight 0 and the filter removes it
    pts = [(A, B, 30, 4), (A, B, 45, 2), (A, B, 58, 3), (A, B, 145, 7), (A, B, 320, 1)]
    c = D.Clustering(g, pts, Cs.params(), keep_unfiltered=True)
    assert c.lengths == {(A, B): [130, 160, 330]}
    assert c.records == [(A, B, 130.0, 0.0, 10), (A, B, 160.0, 0.0, 8), (A, B, 330.0, 0.0, 0)]
    assert _records(g, pts, Cs.params()) == [(A, B, 130.0, 0.0, 10), (A, B, 160.0, 0.0, 8)]
    # linkage_distance 30 joins 130 and 160: centre 145; ClusterResult's half-span 15 does not survive AddToResult (the
    # reference's recorded clusters, tests/golden/graph_ref/bubble.json.gz, all have 0)
    assert D.cluster_result([(130, 10), (160, 8), (330, 0)], 30) == [(145.0, 18, 15.0), (330.0, 0, 0.0)]
    assert _records(g, pts, Cs.params(linkage=30), keep_unfiltered=True) == [(A, B, 145.0, 0.0, 18), (A, B, 330.0, 0.0, 0)]
    assert _records(g, pts, Cs.params(linkage=170)) == [(A, B, 230.0, 0.0, 18)]
    # without the far point 330 is outside [130 - 80, 245 + 80] and is not kept at all
    assert [r[2] for r in _records(g, pts[:4], Cs.params(), keep_unfiltered=True)] == [130.0, 160.0]
    # a point with 2 d + len2 < len1 is skipped: d = -1 (gap -101), which alone would have kept nothing anyway
    assert _records(g, pts + [(A, B, -101, 9)], Cs.params()) == _records(g, pts, Cs.params())


def test_cycle_between_the_edges():
    b, (A, C, B) = Cs.cycle_between()
    g = b.graph()
    c = D.Clustering(g, [(A, B, 0, 3)], Cs.params(max_distance=1000), keep_unfiltered=True)
    # l, l + c, l + 2c, ... up to U = 417: walk lengths 0, 40, ..., 400, one call each
    assert c.lengths == {(A, B): [100 + 40 * j for j in range(11)]} and c.calls == {(A, B): 11}
    assert [r[4] for r in c.records] == [6] + [0] * 10


def test_same_edge_adds_zero():
    b, (A, R) = Cs.cycle_through()
    g = b.graph()
    c = D.Clustering(g, [(A, A, -100, 3)], Cs.params(), keep_unfiltered=True)
    assert c.lengths == {(A, A): [0, 170, 340, 510]}
    assert c.records == [(A, A, 0.0, 0.0, 6)]  # 170 is outside [0 - 80, 0 + 80]


def test_no_path_gives_nothing():
    b, (A, B) = Cs.no_path()
    g = b.graph()
    c = D.Clustering(g, [(A, B, 30, 5)], Cs.params(), keep_unfiltered=True)
    assert c.lengths == {(A, B): []} and c.records == [] and c.calls == {(A, B): 0}


def test_self_conjugate_pairs_carry_four_times_the_weight():
    b, (A, Pl, Q) = Cs.hairpin()
    g = b.graph()
    assert g.conj[Pl] == Pl and g.conj[A] == A + 1
    pts = D.canonical_points(g, [(A, A + 1, 41, 3), (Pl, Pl, -41, 2), (A, Q, 0, 2), (Pl, A + 1, 0, 5), (A, Pl, 0, 5)])
    assert [pt[:2] for pt in pts] == [(A, A + 1), (A, Pl), (A, Q), (Pl, Pl)]  # (Pl, conj A) is stored as (A, Pl)
    c = D.Clustering(g, pts, Cs.params(), keep_unfiltered=True)
    # A -> Pl -> conj A: 100 + 41.  (A, Pl) and (A, Q): the empty walk is shorter than min_len = 183 - l1 - l2
    assert c.lengths == {(A, A + 1): [141], (A, Pl): [], (A, Q): [], (Pl, Pl): [0]}
    assert c.records == [(A, A + 1, 141.0, 0.0, 24), (Pl, Pl, 0.0, 0.0, 16)]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_search_equals_walk_set_where_order_free(seed):
    g = Cs.random_graph(seed).graph()
    pts = Cs.random_points(g, seed)
    s = D.Clustering(g, pts, Cs.params(), keep_unfiltered=True)
    w = D.Clustering(g, pts, Cs.params(), lengths="walks", keep_unfiltered=True)
    free = [pr for pr in s.calls if s.order_free(*pr)]
    assert len(free) > 60
    for pr in s.calls:
        if s.order_free(*pr):
            assert w.lengths[pr] == s.lengths[pr] and w.calls[pr] == s.calls[pr]
        else:
            assert pr not in w.lengths and w.calls[pr] >= 500
    assert [r for r in w.records] == [r for r in s.records if s.order_free(r[0], r[1])]
    assert any(len(v) > 1 for v in s.lengths.values()) and s.records
    # RefinePairedInfo looks for two clusters of a pair with |d2 - d1| <= var1 + var2: there is none, at any linkage
    for linkage in (0, 5, 40):
        recs = D.Clustering(g, pts, Cs.params(linkage=linkage), keep_unfiltered=True).records
        for x, y in zip(recs, recs[1:]):
            if x[:2] == y[:2]:
                assert abs(y[2] - x[2]) > x[3] + y[3]


def test_boundary_chain_calls():
    for calls, shape in Cs.BOUNDARY.items():
        b, (A, B) = Cs.bubble_chain(*shape)
        g = b.graph()
        for mode in ("search", "walks"):
            c = D.Clustering(g, [(A, B, 990, 3)], Cs.boundary_params(), lengths=mode)
            assert c.calls == {(A, B): calls} and c.order_free(A, B) == (calls < 500)
        assert c.hard_pairs(Cs.BALL_CAP, Cs.U_CAP) == ([] if calls < 500 else [(A, B)])


def test_vertex_limit_is_not_order_free():
    gfa, (A, B) = Cs.one_mer_chain(3000)
    g = G.Graph.from_gfa(gfa, Cs.K)
    c = D.Clustering(g, [(A, B, 3000, 3)], Cs.params(insert_size=3100))
    # the Dijkstra takes its 3000th vertex and does not expand it: EdgeStart(B), the 3001st, is never reached
    assert c.ball[A] == 3000 and not c.order_free(A, B) and c.records == []
    short, (A2, B2) = Cs.one_mer_chain(40)
    g2 = G.Graph.from_gfa(short, Cs.K)
    assert D.Clustering(g2, [(A2, B2, 40, 3)], Cs.params()).records == [(A2, B2, 140.0, 0.0, 6)]


def test_file_layout():
    b, (A, M, B) = Cs.single_path()
    g = b.graph()
    c = D.Clustering(g, [(A, B, 48, 3), (A, B, 55, 2)], Cs.params())
    # one first edge; id A + 1; second id B + 1, one point: gap 150 - 100, weight 5; terminator
    assert c.file_bytes() == bytes([1, A + 1, B + 1, 1]) + struct.pack("<ff", 50.0, 5.0) + bytes([0])
    assert D.Clustering(g, [], Cs.params()).file_bytes() == bytes([0])
    assert P.uleb128(300) == bytes([0xAC, 0x02])


# ---- the library's host search ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("distest") / "distest_host_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", path, os.path.join(ROOT, "tests", "distest_host_check.cpp")])
    return path


def _host(exe, g, U, queries):
    """(per edge (end, start) or None, per query (ball, calls, lengths)) of the stand-alone program"""
    ns = len(g.names)
    text = ["%d %d %d %d %d" % (g.k, ns, len(g.links), U, len(queries))]
    text += ["%d %d %d" % (g.length(2 * s), g.conj[2 * s] == 2 * s, g.kc[s]) for s in range(ns)]
    text += ["%d %d %d %d" % (a, oa == "+", b, ob == "+") for a, oa, b, ob in g.links]
    text += ["%d %d %d" % q for q in queries]
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0 and "DISTEST-HOST-OK" in r.stdout, (r.stdout[-300:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    edges = [None if ln == "E - -" else tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("E")]
    qs = [[int(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("Q")]
    return edges, [(q[0], q[1], q[2:]) for q in qs]


def _compare_host(exe, g, pts, p):
    U = D.upper_bound(g.k, p.insert_size, p.delta)
    c = D.Clustering(g, pts, p)
    pairs = sorted(c.calls)
    queries = [(e1, e2, D.lower_bound(g.k, g.length(e1), g.length(e2), p.gap, p.delta)) for e1, e2 in pairs]
    edges, got = _host(exe, g, U, queries)
    assert edges == [(g.end[e], g.start(e)) if e in g.seq else None for e in range(2 * len(g.names))]
    for (e1, e2), (ball, calls, lengths) in zip(pairs, got):
        assert ball == c.ball[e1] and calls == c.calls[(e1, e2)]
        assert [x + g.length(e1) for x in lengths] == [x for x in c.lengths[(e1, e2)] if not (x == 0 and e1 == e2)]
    return c


@pytest.mark.parametrize("seed", [0, 2])
def test_host_search_random_graphs(exe, seed):
    g = Cs.random_graph(seed).graph()
    c = _compare_host(exe, g, Cs.random_points(g, seed), Cs.params())
    assert max(c.calls.values()) >= 500  # the limits fired: the order of the incoming edges mattered


def test_host_search_hand_cases_and_limits(exe):
    b, (A, Pl, Q) = Cs.hairpin()
    g = b.graph()
    _compare_host(exe, g, D.canonical_points(g, [(A, A + 1, 41, 3), (Pl, Pl, -41, 2), (A, Q, 0, 2), (Pl, A + 1, 0, 5)]), Cs.params())
    for shape in Cs.BOUNDARY.values():
        b, (A, B) = Cs.bubble_chain(*shape)
        _compare_host(exe, b.graph(), [(A, B, 990, 3)], Cs.boundary_params())
    gfa, (A, B) = Cs.one_mer_chain(3000)
    c = _compare_host(exe, G.Graph.from_gfa(gfa, Cs.K), [(A, B, 3000, 3)], Cs.params(insert_size=3100))
    assert c.ball[A] == 3000
