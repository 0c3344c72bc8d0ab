"""GPU: the engine and the tools against tests/golden/graph_ref/, the outputs of the reference's own graph-side code
(recorded by oracle/record_graph_ref.py; tests/test_graph_reference_fixtures.py holds the restatements against the same
files on the CPU).  Nothing here looks for the reference or its binary: the fixtures hold the GFA text, the read pairs, the
raw points and every recorded stage.  Every comparison is exact: paths as integers, doubles and floats by their bits,
files decoded by one ULEB128 reader with ids translated to edges.

(a) edgeindex_from_gfa and map_paths against the map stage: every presented mate and every extra sequence.
(b) EdgeIndex.pairinfo: the estimate pass against is and pairs, the fill pass against raw at filter thresholds 0 and 1 and
    round_thr 0 and 4, in one batch and in three uneven ones; the written .prd against the reference's BinWrite bytes.
(c) pairinfo_from_points(...).cluster(...) against clustered for every crafted graph and every read-level one, on the
    device path and with BBK_NO_DISTEST_DEVICE.  Pairs a fixture lists as left out under the tie rule are skipped.
(d) spades-pairinfo --cluster and spades-gmapper on the read-level fixtures."""
import os
import struct
import subprocess

import numpy as np
import pytest

import spades_for_blackbird_amd as B
from spades_for_blackbird_amd import build, build_host
from tests import gmapper_restated as G
from tests import graph_ref_case as C
from tests import pairinfo_cases as PCs
from tests import pairinfo_restated as P

CRAFTED, READS = C.CRAFTED, C.READS
graph, _id_names, _stored, _left_out, _clustered_rows = C.case_graph, C.id_names, C.stored, C.left_out, C.clustered_rows

pytestmark = pytest.mark.gpu

SWITCH = "BBK_NO_DISTEST_DEVICE"


@pytest.fixture(scope="module")
def bins():
    build.build()
    return {os.path.basename(p): p for p in build_host.build()}


@pytest.fixture(scope="module")
def ctx():
    c = B.Context(0)
    yield c
    c.close()


def _index(ctx, tmp_path, case, keep_graph=False):
    path = tmp_path / (case + ".gfa")
    path.write_text(C.load(case)["gfa"])
    return path, ctx.edgeindex_from_gfa(str(path), C.load(case)["k"], keep_graph=keep_graph)


def _recorded_path(g, rows):
    return [(C.edge(g, r[0], r[1]), list(r[2:])) for r in rows]


# ---- (a) map -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", READS)
def test_a_map_paths(ctx, tmp_path, case):
    g, fx = graph(case), C.load(case)
    _, ix = _index(ctx, tmp_path, case)
    seqs, want = [], []
    for row in fx["ref"]["map"]:
        for mate, rows in ((row["first"], row["path1"]), (row["second"], row["path2"])):
            seqs.append(mate)
            want.append(_recorded_path(g, rows))
    for s, rows in zip(fx["seqs"], fx["ref"]["map_seqs"]):
        seqs.append(s)
        want.append(_recorded_path(g, rows))
    off, rec = ix.map_paths(ctx.reads_from_ascii(seqs))
    assert len(off) == len(seqs) + 1 and int(off[-1]) == len(rec) == sum(len(w) for w in want)
    for i in range(len(seqs)):
        got = [(int(x["edge"]), [int(x["init_start"]), int(x["init_end"]), int(x["map_start"]), int(x["map_end"])])
               for x in rec[int(off[i]):int(off[i + 1])]]
        assert got == want[i], (i, seqs[i])
    lens, selfc = ix.segment_lengths()
    assert sorted((C.edge(g, n, o), ln) for n, o, ln, _ in fx["ref"]["edges"] if o == "+") == \
        [(2 * i, int(x)) for i, x in enumerate(lens)]
    assert [bool(x) for x in selfc] == [g.conj[2 * i] == 2 * i for i in range(len(lens))]
    ix.close()


# ---- (b) is, pairs, raw ----------------------------------------------------------------------------------------------------
def _dbits(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", x))[0]


@pytest.mark.parametrize("batches", [None, "three"], ids=["one-batch", "three-batches"])
@pytest.mark.parametrize("case", READS)
def test_b_estimate_and_fill(ctx, tmp_path, case, batches):
    g, fx = graph(case), C.load(case)
    ref, pairs = fx["ref"], [tuple(p) for p in fx["pairs"]]
    o = C.ORIENTATIONS[fx["settings"]["orientation"]]
    _, ix = _index(ctx, tmp_path, case)
    n = len(pairs)
    sizes = None if batches is None else [7, n // 2, n - 7 - n // 2]
    for raw in ref["raw"]:
        prd = str(tmp_path / "x.prd")
        st, hist, points = PCs.engine(ctx, ix, pairs, o, min_edge_length=fx["settings"]["edge_length_bound"],
                                      round_distance=raw["round"], threshold=raw["threshold"], batches=sizes, prd=prd)
        assert (st["total"], st["mapped"], st["negative"]) == (ref["is"]["total"], ref["is"]["mapped"], ref["is"]["negative"])
        assert hist == [tuple(x) for x in ref["is"]["hist"]]
        assert (_dbits(st["mean"]), _dbits(st["deviation"]), _dbits(st["median"]), _dbits(st["mad"])) == \
            (ref["is"]["mean"], ref["is"]["deviation"], ref["is"]["median"], ref["is"]["mad"])
        assert [_dbits(st["left_quantile"]), _dbits(st["right_quantile"])] == ref["is"]["interval"] and st["ok"]
        want_pc = dict((q, v) for q, v in ref["is"]["percentiles"])
        assert st["percentiles"] == [want_pc.get(q, 0) for q in range(5, 100, 5)]
        assert st["edge_pairs"] == ref["pairs"]["exact"]
        assert int(st["mean"]) == raw["insert_size"]
        assert points == C.raw_points(g, raw["half"])
        got = C.decode_prd(open(prd, "rb").read(), {e + 1: e for e in g.seq})
        assert got == C.decode_prd(bytes.fromhex(raw["prd"]), _id_names(g, raw["prd_ids"]))
    ix.close()


# ---- (c) clustered ---------------------------------------------------------------------------------------------------------
def _export(cl):
    e1, e2, c, v, w = cl.export()
    return list(zip(e1.tolist(), e2.tolist(), c.view(np.uint32).tolist(), v.view(np.uint32).tolist(), w.tolist()))


@pytest.mark.parametrize("case", CRAFTED + READS)
def test_c_cluster(ctx, tmp_path, monkeypatch, case):
    g, fx = graph(case), C.load(case)
    stored, left = _stored(case), _left_out(case)
    _, ix = _index(ctx, tmp_path, case, keep_graph=True)
    cols = [np.array([pt[i] for pt in stored], dtype=t) for i, t in enumerate((np.uint64, np.uint64, np.int32, np.uint64))]
    pi = ix.pairinfo_from_points(*cols)
    e1, e2, gap, w = pi.points()
    assert list(zip(e1.tolist(), e2.tolist(), gap.tolist(), w.tolist())) == stored
    for row in fx["ref"]["de"]:
        p = C.params(row)
        want = [(a, b, cb, vb, int(2 * C.f32(wb))) for a, b, cb, vb, wb in _clustered_rows(g, row["clustered_half"])
                if (a, b) not in left]
        assert all(C.f32(r[4]) < 1 << 23 for r in _clustered_rows(g, row["clustered_half"]))
        ref_file = C.decode_prd(bytes.fromhex(row["prd"]), _id_names(g, row["prd_ids"]))
        for on_host in (False, True):
            if on_host:
                monkeypatch.setenv(SWITCH, "1")
            cl = pi.cluster(p.insert_size, p.read_length, p.delta, p.linkage_distance, p.max_distance, p.filter_threshold)
            monkeypatch.delenv(SWITCH, raising=False)
            assert [r for r in _export(cl) if r[:2] not in left] == want, (case, on_host)
            assert cl.pairs == len({pt[:2] for pt in stored})
            out = tmp_path / "x.clustered.prd"
            cl.write(out)
            got = C.decode_prd(out.read_bytes(), {e + 1: e for e in g.seq})
            assert {k: v for k, v in got.items() if k not in left} == {k: v for k, v in ref_file.items() if k not in left}
            cl.close()
    pi.close()
    ix.close()


# ---- (d) the tools -----------------------------------------------------------------------------------------------------------
def _fastq(path, seqs):
    path.write_text("".join("@r%d/x\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(seqs)))
    return path.name


def _ref_stats(ref):
    """the recorded statistics as the engine's dict, for lib_text"""
    pc = dict((q, v) for q, v in ref["is"]["percentiles"])
    return dict(total=ref["is"]["total"], mapped=ref["is"]["mapped"], negative=ref["is"]["negative"],
                edge_pairs=ref["pairs"]["exact"], mean=C.f64(ref["is"]["mean"]), deviation=C.f64(ref["is"]["deviation"]),
                median=C.f64(ref["is"]["median"]), mad=C.f64(ref["is"]["mad"]), left_quantile=C.f64(ref["is"]["interval"][0]),
                right_quantile=C.f64(ref["is"]["interval"][1]), percentiles=[pc.get(q, 0) for q in range(5, 100, 5)], ok=True)


@pytest.mark.parametrize("case", READS)
def test_d_spades_pairinfo_cluster(bins, tmp_path, case):
    g, fx = graph(case), C.load(case)
    ref, pairs = fx["ref"], fx["pairs"]
    gfa = tmp_path / "g.gfa"
    gfa.write_text(fx["gfa"])
    y = tmp_path / "d.yaml"
    y.write_text('- orientation: "%s"\n  type: "paired-end"\n  left reads:\n    - "%s"\n  right reads:\n    - "%s"\n' %
                 (fx["settings"]["orientation"], _fastq(tmp_path / "a_1.fastq", [a for a, _ in pairs]),
                  _fastq(tmp_path / "a_2.fastq", [b for _, b in pairs])))
    ids = {e + 1: e for e in g.seq}
    for i, de in enumerate(fx["settings"]["de"]):
        _, _, read_length, linkage, max_distance, threshold = de
        for raw in ref["raw"][:2] if i == 0 else ref["raw"][:1]:  # round_thr is 0 under the shipped configuration
            prefix = tmp_path / ("out%d_%d" % (i, raw["threshold"]))
            run = subprocess.run([bins["spades-pairinfo"], str(gfa), str(y), str(prefix), "-k", str(fx["k"]), "--meta",
                                  "--min-edge-length", str(fx["settings"]["edge_length_bound"]), "--filter-threshold",
                                  str(raw["threshold"]), "--cluster", "--read-length", str(read_length),
                                  "--linkage-distance-coeff", repr(linkage), "--max-distance-coeff", repr(max_distance),
                                  "--clustered-filter-threshold", repr(threshold)], capture_output=True, text=True)
            assert run.returncode == 0, run.stderr
            assert open("%s.0.is.hist" % prefix).read() == "".join("%d\t%d\n" % tuple(kv) for kv in ref["is"]["hist"])
            assert open("%s.0.lib" % prefix).read() == P.lib_text(_ref_stats(ref))
            got = C.decode_prd(open("%s.0.prd" % prefix, "rb").read(), ids)
            assert got == C.decode_prd(bytes.fromhex(raw["prd"]), _id_names(g, raw["prd_ids"]))
            if raw["threshold"] == 0:  # the recorded clusters are those of the unfiltered raw index
                row = ref["de"][i]
                got = C.decode_prd(open("%s.0.clustered.prd" % prefix, "rb").read(), ids)
                assert got == C.decode_prd(bytes.fromhex(row["prd"]), _id_names(g, row["prd_ids"]))


@pytest.mark.parametrize("case", READS)
def test_d_spades_gmapper(bins, tmp_path, case):
    """the contigs are the presented mates and the extra sequences; the expected file is the restatement's over the
    reference's RECORDED MapSequence paths, not over its own mapper"""
    g, fx = graph(case), C.load(case)
    recorded = {}
    for row in fx["ref"]["map"]:
        recorded[row["first"].upper()] = _recorded_path(g, row["path1"])
        recorded[row["second"].upper()] = _recorded_path(g, row["path2"])
    for s, rows in zip(fx["seqs"], fx["ref"]["map_seqs"]):
        recorded[s] = _recorded_path(g, rows)
    contigs = [s for s in recorded if s]
    gfa = tmp_path / "g.gfa"
    gfa.write_text(fx["gfa"])
    fa = tmp_path / "c.fasta"
    fa.write_text("".join(">c%d\n%s\n" % (i, s) for i, s in enumerate(contigs)))
    y = tmp_path / "d.yaml"
    y.write_text('- type: untrusted-contigs\n  single reads:\n    - "%s"\n' % fa)
    out = tmp_path / "out.gfa"
    run = subprocess.run([bins["spades-gmapper"], str(y), str(gfa), str(out)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert out.read_text() == G.gmapper(g, contigs, mapper=lambda g_, piece: recorded[piece])
    assert sum(line.startswith("P\t") for line in out.read_text().splitlines()) >= 2
