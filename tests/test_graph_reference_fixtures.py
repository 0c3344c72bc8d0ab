"""CPU: the Python restatements of the read-to-graph stages (sequence mapping, insert sizes, edge pairs, the raw paired
index, distance estimation) against tests/golden/graph_ref/, the outputs of the reference's own code (recorded by
oracle/record_graph_ref.py through oracle/graph_ref_driver.cpp, one thread).  Every restatement is given the REFERENCE's
recorded output of the stage before it and has to reproduce the reference's recorded output of its own stage, exactly:
paths as integers, doubles and floats by their bits, files through one ULEB128 reader for both byte streams.

Edges are named (S-line name, orientation) in the fixtures; tests/graph_ref_case.py turns names into the restatements'
numbers.  The pairs a fixture lists under `left_out` met a tie of (distance, -coverage) while their search ran into its
limits, which the reference breaks by its own edge ids; they are compared nowhere.

No GPU, no engine, no reference tree: only the last test (the drift guard) runs the reference binary, and skips without it.
"""
import os
import struct

import pytest

from tests import distest_restated as D
from tests import gmapper_restated as G
from tests import graph_ref_case as C
from tests import pairinfo_restated as P

CRAFTED, READS = C.CRAFTED, C.READS
graph, _id_names, _stored, _left_out, _clustered_rows = C.case_graph, C.id_names, C.stored, C.left_out, C.clustered_rows


def dbits(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", x))[0]


def fbits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def path_of(g, rows):
    """a recorded path as the restatements hold one: [(edge, [initial start, initial end, mapped start, mapped end])]"""
    return [(C.edge(g, r[0], r[1]), list(r[2:])) for r in rows]


def named_path(g, path):
    return [C.named(g, e) + list(r) for e, r in path]


def test_the_fixtures_are_the_cases():
    assert C.names() == sorted(CRAFTED + READS)
    for case in C.names():
        assert C.load(case)["_provenance"]["threads"] == dict(omp_set_num_threads=1, listeners=1, estimate=1)


def test_edge_numbers_order_as_the_recorded_graph():
    """every edge of the reference's graph is a segment of the file in one orientation, a self-conjugate one once"""
    for case in CRAFTED + READS:
        g, fx = graph(case), C.load(case)
        got = sorted((C.edge(g, n, o), length, bool(selfconj)) for n, o, length, selfconj in fx["ref"]["edges"])
        assert got == [(e, g.length(e), g.conj[e] == e) for e in sorted(g.seq)], case


# ---- map -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", READS)
def test_map_presentation_and_paths(case):
    g, fx = graph(case), C.load(case)
    o = C.ORIENTATIONS[fx["settings"]["orientation"]]
    seen = set()
    for (first, second), row in zip(fx["pairs"], fx["ref"]["map"]):
        a, b = P.present(first, second, o)
        assert (a[0], b[0]) == (row["first"].upper(), row["second"].upper())
        assert [a[1], a[2], b[1], b[2]] == row["offsets"]
        for mate, rows in ((a[0], row["path1"]), (b[0], row["path2"])):
            assert named_path(g, G.map_sequence(g, mate)) == rows
            assert named_path(g, G.map_read(g, mate)) == rows
            seen.add("short" if 0 < len(mate) < g.k + 1 else "empty" if not mate else "edges>=3" if len(rows) >= 3 else "")
        seen.add("N" if "N" in first + second else "")
        seen.add("lower" if second != second.upper() else "")
    assert len(fx["pairs"]) == len(fx["ref"]["map"])
    assert seen >= {"short", "empty", "N", "lower"} | ({"edges>=3"} if case != "synth_fr" else set())


@pytest.mark.parametrize("case", READS)
def test_map_extra_sequences(case):
    g, fx = graph(case), C.load(case)
    assert len(fx["seqs"]) == len(fx["ref"]["map_seqs"])
    for s, rows in zip(fx["seqs"], fx["ref"]["map_seqs"]):
        assert named_path(g, G.map_sequence(g, s)) == rows
        assert named_path(g, G.map_sequence_local(g, s)) == rows  # the kernel's position-local rule
    assert fx["ref"]["map_seqs"][-1] == [] or case == "synth_fr"  # k bases: shorter than a (k+1)-mer


def test_map_covers_all_four_orientations_by_the_reference():
    """the reverse-complemented mates are mapped by the reference, not derived: in every case some mate that the library's
    orientation turns (the first under rf and rr, the second under fr and rr) has a recorded path of its own, and the
    presented text of such a mate is the reverse complement of its stretch in the file"""
    from tests.helpers import rc
    for case in READS:
        fx = C.load(case)
        o = fx["settings"]["orientation"]
        turned = [key for key, on in (("path1", o in ("rf", "rr")), ("path2", o in ("fr", "rr"))) if on]
        assert (len(turned) > 0) == (o != "ff")
        for key in turned:
            side = 0 if key == "path1" else 1
            mapped = [i for i, row in enumerate(fx["ref"]["map"]) if row[key]]
            assert len(mapped) >= 20, (case, key)
            for i in mapped:
                text = fx["ref"]["map"][i]["first" if side == 0 else "second"]
                assert rc(text).upper() in fx["pairs"][i][side].upper(), (case, i)
    for case in READS[1:]:
        signs = {r[1] for row in C.load(case)["ref"]["map"] for r in row["path1"] + row["path2"]}
        assert signs == {"+", "-"}, case


# ---- is ----------------------------------------------------------------------------------------------------------------------
def _counter(case):
    g, fx = graph(case), C.load(case)
    counter, counts = P.InsertSizeCounter(g, fx["settings"]["edge_length_bound"]), P.PairCounts(g)
    for row in fx["ref"]["map"]:
        p1, p2 = path_of(g, row["path1"]), path_of(g, row["path2"])
        counter.process(p1, p2, len(row["second"]), row["offsets"][0] + row["offsets"][3])
        counts.process(p1, p2)
    return counter, counts


@pytest.mark.parametrize("case", READS)
def test_insert_sizes(case):
    g, ref = graph(case), C.load(case)["ref"]["is"]
    counter, counts = _counter(case)
    assert (counter.total, counter.mapped, counter.negative) == (ref["total"], ref["mapped"], ref["negative"])
    assert sorted(counter.hist.items()) == [tuple(x) for x in ref["hist"]]
    assert counter.mapped > 0
    mean, deviation, percentiles = P.find_mean(counter.hist)
    median, mad, cropped = P.find_median(counter.hist)
    assert (dbits(mean), dbits(deviation), dbits(median), dbits(mad)) == (ref["mean"], ref["deviation"], ref["median"], ref["mad"])
    assert sorted(percentiles.items()) == [tuple(x) for x in ref["percentiles"]]
    assert sorted(cropped.items()) == [tuple(x) for x in ref["distribution"]]
    assert [dbits(x) for x in P.get_is_interval(0.8, cropped)] == ref["interval"]
    st = P.estimate(counter, g.k, counts.edge_pairs())
    assert (dbits(st["left_quantile"]), dbits(st["right_quantile"])) == tuple(ref["interval"]) and st["ok"]
    if case == "synth_fr":
        assert counter.negative > 0 and counter.mapped > 40 and any(row["offsets"][0] + row["offsets"][3] for row in C.load(case)["ref"]["map"])


# ---- pairs -------------------------------------------------------------------------------------------------------------------
def _edge_pairs(case):
    g, ref = graph(case), C.load(case)["ref"]["pairs"]
    _, counts = _counter(case)
    assert counts.edge_pairs() == ref["exact"] == len(ref["counts"])
    selfconj = 0
    for n1, o1, n2, o2, count, conj_count, bloom in ref["counts"]:
        e1, e2 = C.edge(g, n1, o1), C.edge(g, n2, o2)
        assert counts.occ[(e1, e2)] == count
        assert counts.c(e1, e2) == count + conj_count
        # the reference's counting Bloom filter of 2-bit cells said the same as the exact count (a condition of the
        # recording): what passes the engine's exact filter is what passed the reference's
        assert bloom == min(counts.c(e1, e2), 3)
        for threshold in (0, 1):
            assert counts.passes(e1, e2, threshold) == (threshold == 0 or bloom > threshold)
        selfconj += e1 == g.conj[e2]
    assert ref["cells"] == 12 * ref["cardinality"]
    return selfconj


@pytest.mark.parametrize("case", READS)
def test_edge_pair_counts_and_the_filter(case):
    _edge_pairs(case)


def test_self_conjugate_pairs_occur_in_the_read_level_cases():
    assert sum(_edge_pairs(case) for case in READS) >= 3


# ---- raw ---------------------------------------------------------------------------------------------------------------------
def _restated_index(case, raw):
    g, fx = graph(case), C.load(case)
    _, counts = _counter(case)
    index = P.PairedIndex(g)
    for row in fx["ref"]["map"]:
        P.fill_pair(index, counts, path_of(g, row["path1"]), path_of(g, row["path2"]), len(row["second"]),
                    row["offsets"][0] + row["offsets"][3], raw["insert_size"], raw["round"], raw["threshold"])
    return index


@pytest.mark.parametrize("case", READS)
def test_raw_index(case):
    g, fx = graph(case), C.load(case)
    assert [(r["threshold"], r["round"]) for r in fx["ref"]["raw"]] == [(0, 0), (1, 0), (0, 4), (1, 4)]
    sizes = []
    for raw in fx["ref"]["raw"]:
        assert raw["insert_size"] == int(C.f64(fx["ref"]["is"]["mean"]))  # (size_t) mean_insert_size
        points = _restated_index(case, raw).points()
        assert points == C.raw_points(g, raw["half"])  # gaps and weights as exact floats
        # GetHalf presents the canonical pairs only; Get presents each of them and its conjugate couple, the gap unchanged
        full = C.raw_points(g, raw["full"])
        mirrored = [(g.conj[e2], g.conj[e1], gap, w) for e1, e2, gap, w in points if e1 != g.conj[e2]]
        assert full == sorted(points + mirrored)
        assert all((e1, e2) <= (g.conj[e2], g.conj[e1]) for e1, e2, _, _ in points)
        assert raw["size"] == len(points) + len(mirrored)
        # the file: both byte streams through one reader, ids to edges; the streams differ by the id numbering alone
        ref = C.decode_prd(bytes.fromhex(raw["prd"]), _id_names(g, raw["prd_ids"]))
        ours = C.decode_prd(P.prd_bytes(points), {e + 1: e for e in g.seq})
        assert ref == ours and sum(len(v) for v in ours.values()) == len(points)
        assert bytes.fromhex(raw["prd"])[-1] == 0 and P.prd_bytes(points)[-1] == 0
        sizes.append(len(points))
    # the rounding merged points; on the junction graph the filter removed pairs
    assert sizes[2] < sizes[0] and (sizes[1] < sizes[0] or case == "synth_fr")


def test_rounding_is_half_away_from_zero(monkeypatch):
    """round_thr = 4 meets distances halfway between two multiples, positive and negative ones; the restatement's
    std::round reproduces every recorded index (test_raw_index), and rounding such a distance to the even multiple, or
    toward zero, would not"""
    def to_even(d, r):
        return P.i32(int(round(d / float(r))) * r)  # Python rounds half to even

    def toward_zero(d, r):
        q = (2 * abs(d) + r - 1) // (2 * r)
        return P.i32((-q if d < 0 else q) * r)

    for other in (to_even, toward_zero):
        differ = 0
        monkeypatch.setattr(P, "round_distance_double", other)
        for case in READS:
            raw = C.load(case)["ref"]["raw"][2]
            differ += _restated_index(case, raw).points() != C.raw_points(graph(case), raw["half"])
        monkeypatch.undo()
        assert differ == len(READS), other.__name__
    assert [P.round_distance_int(d, r) for r in (2, 4, 5) for d in range(-40, 40)] == \
        [P.round_distance_double(d, r) for r in (2, 4, 5) for d in range(-40, 40)]
    assert P.round_distance_double(-6, 4) == -8 and P.round_distance_double(6, 4) == 8 and to_even(6, 4) == 8 and to_even(-6, 4) == -8
    assert P.round_distance_double(-2, 4) == -4 and to_even(-2, 4) == 0 and toward_zero(6, 4) == 4


# ---- lengths and clustered --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CRAFTED + READS)
def test_library_parameters(case):
    fx = C.load(case)
    for setting, row in zip(fx["settings"]["de"], fx["ref"]["de"]):
        p = D.library_params(*setting)
        assert (p.insert_size, p.read_length, p.delta, p.linkage_distance, p.max_distance, dbits(p.filter_threshold)) == \
            (row["insert_size"], row["read_length"], row["delta"], row["linkage_distance"], row["max_distance"], row["threshold"])


@pytest.mark.parametrize("case", CRAFTED + READS)
def test_lengths(case):
    g, fx = graph(case), C.load(case)
    stored, left = _stored(case), _left_out(case)
    for row in fx["ref"]["de"]:
        c = D.Clustering(g, stored, C.params(row), keep_unfiltered=True)
        ref = {(C.edge(g, r[0], r[1]), C.edge(g, r[2], r[3])): r[4] for r in row["lengths"]}
        assert sorted(ref) == sorted(c.lengths) == sorted({pt[:2] for pt in stored})
        for pair in ref:
            if pair not in left:
                assert c.lengths[pair] == ref[pair], (case, pair)
            else:
                assert not c.order_free(*pair)


@pytest.mark.parametrize("case", CRAFTED + READS)
def test_clustered(case):
    g, fx = graph(case), C.load(case)
    stored, left = _stored(case), _left_out(case)
    for row in fx["ref"]["de"]:
        for key, unfiltered in (("clustered_half", False), ("unfiltered", True)):
            c = D.Clustering(g, stored, C.params(row), keep_unfiltered=unfiltered)
            ref = [r for r in _clustered_rows(g, row[key]) if (r[0], r[1]) <= (g.conj[r[1]], g.conj[r[0]])]
            assert all(C.f32(r[4]) < 1 << 23 and 2 * C.f32(r[4]) == int(2 * C.f32(r[4])) for r in ref)  # half-units are exact
            want = [(e1, e2, fbits(centre), fbits(var), w) for e1, e2, centre, var, w in c.records if (e1, e2) not in left]
            got = [(e1, e2, cb, vb, int(2 * C.f32(wb))) for e1, e2, cb, vb, wb in ref if (e1, e2) not in left]
            assert want == got, (case, key)
        # Get after the filter: every canonical point and its conjugate couple, d' = d + len(e2) - len(e1)
        half, full = _clustered_rows(g, row["clustered_half"]), _clustered_rows(g, row["clustered"])
        mirrored = [(g.conj[e2], g.conj[e1], fbits(C.f32(cb) + g.length(e2) - g.length(e1)), vb, wb)
                    for e1, e2, cb, vb, wb in half if e1 != g.conj[e2]]
        assert full == sorted(half + mirrored, key=lambda r: (r[0], r[1], C.f32(r[2])))
        assert row["size_after"] == len(full) and row["size_before"] >= row["size_after"]
        # the file: RawPointT::BinWrite's 8 bytes per point (gap, weight), no half-span; one reader for both streams
        c = D.Clustering(g, stored, C.params(row))
        ref = C.decode_prd(bytes.fromhex(row["prd"]), _id_names(g, row["prd_ids"]))
        assert sum(len(v) for v in ref.values()) == len(half)
        ours = C.decode_prd(c.file_bytes(), {e + 1: e for e in g.seq})
        assert {k: v for k, v in ref.items() if k not in left} == {k: v for k, v in ours.items() if k not in left}
        # no two clusters of a pair satisfy the condition RefinePairedInfo looks for
        assert row["refine_condition"] is False


def test_share_left_out_under_the_tie_rule():
    for case in CRAFTED + READS:
        left, pairs = _left_out(case), {pt[:2] for pt in _stored(case)}
        assert left <= pairs and len(left) <= (len(pairs) // 10 if case.startswith("random_") else 0), case


def test_limits_are_met_without_a_tie():
    """searches at 500 calls or more, and a ball at the vertex limit, are compared too where no tie decides their order"""
    n = {}
    for case in ("bubble_chain_500", "one_mer_chain_600", "one_mer_chain_3000", "random_0", "random_1", "random_2"):
        g, fx = graph(case), C.load(case)
        c = D.Clustering(g, _stored(case), C.params(fx["ref"]["de"][0]))
        n[case] = len([pr for pr in c.calls if not c.order_free(*pr) and pr not in _left_out(case)])
    assert n["bubble_chain_500"] == n["one_mer_chain_600"] == n["one_mer_chain_3000"] == 1
    assert n["random_0"] + n["random_1"] + n["random_2"] >= 15


# ---- the readings DESIGN 4.3m and 4.3n name, stated from the fixtures alone ---------------------------------------------
def _weights(case, i, key="clustered_half"):
    g = graph(case)
    return [(e1, e2, C.f32(cb), C.f32(wb)) for e1, e2, cb, _, wb in _clustered_rows(g, C.load(case)["ref"]["de"][i][key])
            if (e1, e2) <= (g.conj[e2], g.conj[e1])]


def test_reading_self_conjugate_pair_carries_four_times_its_weight():
    g, (A, Pl, Q) = graph("hairpin"), (0, 2, 4)
    assert g.conj[Pl] == Pl and g.conj[A] == A + 1
    stored = {pt[:2]: pt[3] for pt in _stored("hairpin")}
    assert stored[(A, A + 1)] == 3 and stored[(Pl, Pl)] == 2
    got = {r[:2]: r[2:] for r in _weights("hairpin", 0)}
    assert got[(A, A + 1)] == (141.0, 12.0) and got[(Pl, Pl)] == (0.0, 8.0)


def test_reading_same_edge_has_the_zero_length():
    ref = C.load("cycle_through")["ref"]["de"][0]
    lengths = {tuple(r[:4]): r[4] for r in ref["lengths"]}
    assert lengths[("3", "+", "3", "+")] == [0, 170, 340, 510]
    assert lengths[("3", "+", "3", "-")] == []


def test_reading_vertex_limit_yields_no_record():
    ref = C.load("one_mer_chain_3000")["ref"]["de"][0]
    assert [r[4] for r in ref["lengths"]] == [[]] and ref["unfiltered"] == [] and ref["size_before"] == 0
    ref = C.load("one_mer_chain_600")["ref"]["de"][0]
    assert [r[4] for r in ref["lengths"]] == [[700]] and ref["size_after"] == 2


def test_reading_point_dropped_by_its_distance():
    """cycle_between: the points d = 100 (3), d = 0 (5) and d = -1 (9) all lie within max_distance = 1000 of the length 100
    and nearest to it; 2 d + len2 < len1 drops d = -1 alone"""
    got = _weights("cycle_between", 0, "unfiltered")
    assert (got[0][2], got[0][3]) == (100.0, 8.0)
    assert sum(w for _, _, _, w in got) == 12.0  # 3 + 5 + 4; never the 9


def test_reading_exact_tie_halves_the_weight():
    """bubble: d = 145 (weight 2) lies halfway between 130 and 160: 4 + 1 and 3 + 1"""
    assert [r[2:] for r in _weights("bubble", 0)] == [(130.0, 5.0), (160.0, 4.0)]


def test_reading_weight_filter_has_four_ulps_of_slack():
    ref = C.load("single_path_ulp")["ref"]["de"]
    assert [C.f64(r["threshold"]) > 2.0 for r in ref] == [False, True, True]
    assert [[C.f32(p[6]) for p in r["clustered_half"]] for r in ref] == [[2.0], [2.0], []]


def test_reading_min_len():
    """hairpin: (A, Q) are adjacent, the empty walk has length 0 < min_len = 200 + 23 - 100 - 60 - 40 = 23: no length;
    tree_65 at insert size 300: min_len = max(0, 100 + 23 - 100 - 23 - 40) = 0 and the root's edges have the length 100"""
    lengths = {tuple(r[:4]): r[4] for r in C.load("hairpin")["ref"]["de"][0]["lengths"]}
    assert lengths[("3", "+", "7", "+")] == [] and lengths[("3", "+", "3", "-")] == [141]
    assert sum(r[4] == [100] for r in C.load("tree_65")["ref"]["de"][0]["lengths"]) == 4


def test_reading_longest_valid_cuts_the_mate_in_file_orientation():
    """pair 2 of every read-level case has a first mate of equally long valid stretches.  The binary conversion cuts in file
    orientation and turns at write, so the reference keeps the FIRST stretch of the file's text under all four orientations
    (rf and rr present its reverse complement, the offsets swapped)"""
    from tests.helpers import rc
    for case in READS:
        fx = C.load(case)
        first = fx["pairs"][2][0]
        stretches = [x for x in first.split("N") if x]
        longest = [x for x in stretches if len(x) == max(map(len, stretches))]
        assert len(longest) > 1 and longest[0] != longest[-1]
        turned = fx["settings"]["orientation"] in ("rf", "rr")
        row = fx["ref"]["map"][2]
        assert row["first"] == (rc(longest[0]) if turned else longest[0]), case
        left, right = first.index(longest[0]), len(first) - first.index(longest[0]) - len(longest[0])
        assert row["offsets"][:2] == ([right, left] if turned else [left, right]), case


# ---- the drift guard -------------------------------------------------------------------------------------------------------------
def test_reference_binary_still_gives_the_committed_fixtures(tmp_path):
    from oracle import record_graph_ref as Rec
    if not os.path.exists(Rec.BINARY):
        pytest.skip("oracle/_ref/graph_ref is not built (no reference tree)")
    got = Rec.record(str(tmp_path))
    committed = sorted(f for f in os.listdir(C.FIXTURES) if f.endswith(".json.gz"))
    assert sorted(got) == committed
    for name in committed:
        with open(os.path.join(C.FIXTURES, name), "rb") as f:
            assert f.read() == got[name], name
