"""Records tests/golden/graph_ref/ from the reference's own graph-side code: `python oracle/record_graph_ref.py`.

TEST INFRASTRUCTURE ONLY.  Runs oracle/_ref/graph_ref (built by `make -C oracle ref` from the reference's sources and
oracle/graph_ref_driver.cpp) on the inputs of tests/graph_ref_case.py and stores each case as <case>.json.gz: the inputs
(GFA text, points or read pairs, settings), the driver's document, the pairs left out under the tie rule, and a
`_provenance` entry.  Recording twice gives the same bytes (gzip without a time stamp, sorted keys), which is what the
drift guard of tests/test_graph_reference_fixtures.py relies on.

Two conditions are checked here, with the restatements alone, and a case that misses one is not written:
  - the reference's counting Bloom filter answers min(count, 3) for every edge pair of a read-level case (the filter is
    probabilistic, the engine exact: a case that falls into a collision is reseeded, not tolerated);
  - a pair whose search runs into its limits (500 calls or more, a ball of 2999 vertices or more) meets no tie of
    (distance, -coverage) in the restatement, or is left out; none may be left out of a crafted case, and at most one
    pair in ten of a random graph.
"""
import gzip
import io
import json
import os
import subprocess
import sys
import tempfile

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
BINARY = os.path.join(_HERE, "_ref", "graph_ref")
THREADS = dict(omp_set_num_threads=1, listeners=1, estimate=1)


def encode(data):
    """the bytes of a fixture file: canonical JSON, gzip with no time stamp and no file name"""
    raw = json.dumps(data, sort_keys=True, separators=(",", ":")).encode("ascii")
    buf = io.BytesIO()
    with gzip.GzipFile(filename="", mode="wb", fileobj=buf, mtime=0, compresslevel=9) as f:
        f.write(raw)
    return buf.getvalue()


def _settings_text(orientation="fr", edge_length_bound=0, insert_size=None, fills=(), de=()):
    lines = ["orientation %s" % orientation, "edge_length_bound %d" % edge_length_bound]
    if insert_size is not None:
        lines.append("insert_size %d" % insert_size)
    lines += ["fill %d %d" % f for f in fills]
    lines += ["de %.17g %.17g %d %.17g %.17g %.17g" % tuple(d) for d in de]
    return "".join(x + "\n" for x in lines)


def _run(d, gfa, k, settings, extra):
    os.makedirs(os.path.join(d, "work"), exist_ok=True)
    paths = {n: os.path.join(d, n) for n in ("g.gfa", "settings", "out.json")}
    with open(paths["g.gfa"], "w") as f:
        f.write(gfa)
    with open(paths["settings"], "w") as f:
        f.write(settings)
    r = subprocess.run([BINARY, paths["g.gfa"], str(k), os.path.join(d, "work"), paths["settings"], paths["out.json"]] + extra,
                       capture_output=True, text=True, errors="replace")
    if r.returncode != 0:
        raise RuntimeError("graph_ref failed (%d):\n%s\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:]))
    with open(paths["out.json"]) as f:
        return json.load(f)


def tied_pairs(g, canon, p):
    """the pairs at their limits that meet a tie in the restatement: [(e1, e2)]"""
    from tests import distest_restated as D
    from tests import gmapper_restated as G
    c = D.Clustering(g, canon, p)
    out = []
    orig = D._sorted_incoming
    for e1, e2 in sorted(c.calls):
        if c.order_free(e1, e2):
            continue
        dist = G.dijkstra(g, g.end[e1], c.U, D.MAX_DIJKSTRA_VERTICES)
        ties = [len(dist) >= D.MAX_DIJKSTRA_VERTICES - 1 and len(set(dist.values())) != len(dist)]

        def spy(g_, dist_, v):
            inc = orig(g_, dist_, v)
            keys = [(dist_[g_.start(e)], -g_.coverage(e)) for e in inc]
            if len(set(keys)) != len(keys):
                ties[0] = True
            return inc

        D._sorted_incoming = spy
        try:
            D.traversal(g, dist, g.end[e1], g.start(e2), D.lower_bound(g.k, g.length(e1), g.length(e2), p.gap, p.delta), c.U)
        finally:
            D._sorted_incoming = orig
        if ties[0]:
            out.append((e1, e2))
    return out, sum(1 for pr in c.calls if not c.order_free(*pr)), len(c.calls)


def _left_out(case, g, canon, doc, cap):
    """the pairs of a case left out under the tie rule, as names; asserts the cap"""
    from tests import graph_ref_case as C
    left, hard_total = set(), 0
    for row in doc["de"]:
        tied, hard, pairs = tied_pairs(g, canon, C.params(row))
        left |= set(tied)
        hard_total = max(hard_total, hard)
    n_pairs = len({pt[:2] for pt in canon})
    print("%-22s %4d pairs, %3d at their limits, %3d left out under the tie rule" % (case, n_pairs, hard_total, len(left)))
    if len(left) > cap * n_pairs:
        raise RuntimeError("%s: %d of %d pairs meet a tie at their limits (cap %g)" % (case, len(left), n_pairs, cap))
    return [C.named(g, e1) + C.named(g, e2) for e1, e2 in sorted(left)]


def record_crafted(case, gfa, points, de, tmp):
    from tests import distest_restated as D
    from tests import gmapper_restated as G
    from tests import graph_ref_case as C
    g = G.Graph.from_gfa(gfa, C.K)
    canon = D.canonical_points(g, points)
    # PairedIndex::Add doubles what it is given for a self-conjugate pair: half the stored weight goes in
    lines = ["%s %s %s %s %d %.17g\n" % tuple(C.named(g, e1) + C.named(g, e2) + [gap + g.length(e1),
                                                                                    w / 2.0 if e1 == g.conj[e2] else w])
             for e1, e2, gap, w in canon]
    d = os.path.join(tmp, case)
    os.makedirs(d)
    with open(os.path.join(d, "points"), "w") as f:
        f.write("".join(lines))
    doc = _run(d, gfa, C.K, _settings_text(de=de), ["points", os.path.join(d, "points")])
    if C.raw_points(g, doc["points"]["half"]) != canon:
        raise RuntimeError("%s: the reference stores other points than the case states" % case)
    left = _left_out(case, g, canon, doc, 0.1 if case.startswith("random_") else 0.0)
    return dict(k=C.K, gfa=gfa, added=[ln.split() for ln in lines], settings=dict(de=[list(x) for x in de]), ref=doc,
                left_out=left, _provenance=_provenance("points"))


def record_reads(case, spec, tmp):
    from tests import gmapper_restated as G
    from tests import graph_ref_case as C
    d = os.path.join(tmp, case)
    os.makedirs(d)
    for side, name in ((0, "left.fastq"), (1, "right.fastq")):
        with open(os.path.join(d, name), "w") as f:
            f.write("".join("@r%d/%d\n%s\n+\n%s\n" % (i, side + 1, p[side], "I" * len(p[side])) for i, p in enumerate(spec["pairs"])))
    with open(os.path.join(d, "seqs"), "w") as f:
        f.write("".join(s + "\n" for s in spec["seqs"]))
    extra = ["reads", os.path.join(d, "left.fastq"), os.path.join(d, "right.fastq"), "seqs", os.path.join(d, "seqs")]
    # a first run for the insert-size statistics: estimate_distance takes its mean and deviation from them
    first = _run(os.path.join(d, "first"), spec["gfa"], C.K, _settings_text(spec["orientation"], spec["edge_length_bound"]), extra)
    if "interval" not in first["is"]:
        raise RuntimeError("%s: the reference cannot estimate the insert size" % case)
    de = [(C.f64(first["is"]["mean"]), C.f64(first["is"]["deviation"])) + tuple(x) for x in spec["de"]]
    doc = _run(d, spec["gfa"], C.K, _settings_text(spec["orientation"], spec["edge_length_bound"], None, spec["fills"], de), extra)
    bad = [row for row in doc["pairs"]["counts"] if row[6] != min(row[4] + row[5], 3)]
    if bad:
        raise RuntimeError("%s: the reference's Bloom filter differs from min(count, 3) on %d pairs: reseed the case" % (case, len(bad)))
    g = G.Graph.from_gfa(spec["gfa"], C.K)
    canon = C.raw_points(g, doc["raw"][0]["half"])
    left = _left_out(case, g, canon, doc, 0.0)
    return dict(k=C.K, gfa=spec["gfa"], pairs=[list(p) for p in spec["pairs"]], seqs=spec["seqs"],
                settings=dict(orientation=spec["orientation"], edge_length_bound=spec["edge_length_bound"],
                              fills=[list(x) for x in spec["fills"]], de=[list(x) for x in de]),
                ref=doc, left_out=left, _provenance=_provenance("reads"))


def _provenance(kind):
    return dict(command="oracle/_ref/graph_ref <gfa> <k> <work> <settings> <out.json> %s" %
                ("points <points>" if kind == "points" else "reads <left.fastq> <right.fastq> seqs <seqs>"),
                recorder="python oracle/record_graph_ref.py", threads=THREADS)


def record(tmp):
    """{file name: bytes} of every fixture"""
    from tests import graph_ref_case as C
    out = {}
    for case, (gfa, points, de) in sorted(C.crafted_cases().items()):
        out[case + ".json.gz"] = encode(record_crafted(case, gfa, points, de, tmp))
    for case, spec in sorted(C.read_cases().items()):
        out[case + ".json.gz"] = encode(record_reads(case, spec, tmp))
    return out


def main():
    from tests import graph_ref_case as C
    if not os.path.exists(BINARY):
        sys.exit("oracle/_ref/graph_ref is not built: run `make -C oracle ref` with the reference tree present")
    os.makedirs(C.FIXTURES, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        for name, data in sorted(record(tmp).items()):
            with open(os.path.join(C.FIXTURES, name), "wb") as f:
                f.write(data)
            print("%-32s %7d bytes" % (name, len(data)))


if __name__ == "__main__":
    sys.path.insert(0, _ROOT)
    main()
