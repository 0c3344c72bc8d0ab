"""GPU: the paired-info stage (csrc/pairinfo.hip, spades-pairinfo) against its restatement (tests/pairinfo_restated.py).
Every comparison is exact: counters, histogram, edge_pairs, every point, the .prd bytes, and the statistics as doubles bit
for bit (they are host code over an equal histogram).

(a) gbuilder graphs of reads_synth(3000 x 150, genome 20 000) at k = 21 and k = 55, pairs cut from the genome with
fragments ~ N(400, 30), all four orientations, with and without substitutions and Ns in the mates.  Two graphs per k:
  - sub 0.003, the graph the stage was specified on.  gbuilder does not simplify, so the 1350 substitutions of the reads
    leave a bubble or a tip each and the genome is cut into some 3000 segments of a few (k+1)-mers: no mate lies on one
    edge (the restatement counts mapped = 0 of 300 at both k), and the paths are long -- up to 480 records per pair at
    k = 21, 49 408 distinct edge pairs.  It carries the conditions on |path1| x |path2| and on conjugate storage.
  - sub 0, the graph of the genome itself: one segment.  Under fr the restatement counts 225 of 300 pairs with a positive
    insert size and 19 with a negative one.  It carries the conditions on mapped, on negative pairs and, again, on
    conjugate storage.
The conditions are computed from the restatement, never from the engine.
(b) edge cases: 0, 1, 63, 64, 65, 255, 256, 257 pairs; a batch where every path is empty; the adversarial graph of
test_gpu_gmapper (homopolymer loop, palindromic segment, circular segment).  (c) one batch against three uneven ones.
(d) filter thresholds 0..3 and round_distance 0, 1, 2, 5.  (e) the tool."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import spades_for_blackbird_amd as B
from spades_for_blackbird_amd import build, build_host
from tests import gmapper_restated as G
from tests import pairinfo_cases as Cs
from tests import pairinfo_restated as P
from tests.helpers import rc

pytestmark = pytest.mark.gpu

N_PAIRS = 300


@pytest.fixture(scope="module")
def bins():
    build.build()
    return {os.path.basename(p): p for p in build_host.build()}


@pytest.fixture(scope="module")
def ctx():
    c = B.Context(0)
    yield c
    c.close()


def _bits(st):
    """the statistics with every double as its bit pattern"""
    return {key: struct.pack("<d", v) if isinstance(v, float) else v for key, v in st.items()}


def _compare(ctx, ix, g, pairs, orientation, tmp_path=None, **kw):
    """engine == restatement for one library; returns the restatement's (statistics, library)"""
    st, hist, points, lib = Cs.restated(g, pairs, orientation, **kw)
    prd = str(tmp_path / "x.prd") if tmp_path is not None else None
    got_st, got_hist, got_points = Cs.engine(ctx, ix, pairs, orientation, prd=prd, **kw)
    assert _bits(got_st) == _bits(st)
    assert got_hist == hist
    assert got_points == points
    if prd is not None:
        assert open(prd, "rb").read() == P.prd_bytes(points)
    return st, lib


@pytest.fixture(scope="module")
def synth_graphs(ctx, tmp_path_factory):
    """get(k, sub_rate) -> (genome, Graph, EdgeIndex) of reads_synth, each built once and freed before the context"""
    made = {}

    def get(k, sub):
        if (k, sub) not in made:
            r = ctx.reads_synth(3000, read_len=150, genome_len=20000, sub_rate=sub, seed_genome=k, seed_reads=k + 1)
            gfa = tmp_path_factory.mktemp("g") / "g.gfa"
            ctx.unitigs(ctx.extindex(r, k)).write_gfa(str(gfa))
            made[(k, sub)] = (Cs.synth_genome(k, 20000), G.Graph.from_gfa(gfa.read_text(), k),
                              ctx.edgeindex_from_gfa(str(gfa), k))
        return made[(k, sub)]

    yield get
    for _, _, ix in made.values():
        ix.close()


@pytest.mark.parametrize("mutated", [False, True], ids=["plain", "mutated"])
@pytest.mark.parametrize("orientation", [P.FF, P.FR, P.RF, P.RR], ids=["ff", "fr", "rf", "rr"])
@pytest.mark.parametrize("k,sub", [(21, 0.003), (21, 0.0), (55, 0.003), (55, 0.0)],
                         ids=["k21-sub", "k21-clean", "k55-sub", "k55-clean"])
def test_a_synth_graphs(ctx, tmp_path, synth_graphs, k, sub, orientation, mutated):
    genome, g, ix = synth_graphs(k, sub)
    rng = random.Random(k)
    pairs = Cs.cut_pairs(rng, genome, N_PAIRS)
    if mutated:  # substitutions split the paths, Ns make LongestValid cut the mates
        pairs = [(Cs.mutate(rng, a, 0.003, 0.004), Cs.mutate(rng, b, 0.003, 0.004)) for a, b in pairs]
        assert Cs.cuts(pairs).any(axis=1).sum() > N_PAIRS // 4
    st, lib = _compare(ctx, ix, g, pairs, orientation, tmp_path)
    assert st["total"] == N_PAIRS and lib.index.under_conjugate >= 1
    if sub > 0:
        assert len(g.names) > 1000 and lib.max_product >= 4
    elif orientation == P.FR:
        # (the substitutions of the mutated mates take a third of the pairs off their edge)
        assert st["mapped"] * (3 if mutated else 2) >= st["total"] and st["negative"] >= 1 and st["ok"]
        assert abs(st["mean"] - 400) < 10
    if sub == 0 and mutated:
        assert lib.max_product >= 4


def _chain_graph(ctx, tmp_path, k=21, seed=5):
    rng = random.Random(seed)
    genome = "".join(rng.choice("ACGT") for _ in range(3000))
    cutpos = [0, 700, 1500, 2200, 3000]
    segs = [genome[max(0, a - k):b] for a, b in zip(cutpos, cutpos[1:])]
    gfa = tmp_path / "chain.gfa"
    gfa.write_text("".join("S\t%d\t%s\n" % (3 + 2 * i, q) for i, q in enumerate(segs)) +
                   "".join("L\t%d\t+\t%d\t+\t%dM\n" % (3 + 2 * i, 5 + 2 * i, k) for i in range(len(segs) - 1)))
    return rng, genome, G.Graph.from_gfa(gfa.read_text(), k), ctx.edgeindex_from_gfa(str(gfa), k)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_b_pair_counts_at_wave_and_block_edges(ctx, tmp_path, n):
    rng, genome, g, ix = _chain_graph(ctx, tmp_path)
    pairs = Cs.cut_pairs(rng, genome, n)
    st, _ = _compare(ctx, ix, g, pairs, P.FR, tmp_path, min_edge_length=700)
    assert st["total"] == n


def test_b_every_path_empty(ctx, tmp_path):
    rng, genome, g, ix = _chain_graph(ctx, tmp_path)
    other = "".join(rng.choice("ACGT") for _ in range(3000))  # not in the graph
    pairs = Cs.cut_pairs(rng, other, 70) + [("ACGT", "ACGTACGTAC"), ("", "N"), ("A" * 21, "C" * 21)]
    st, hist, points, _ = Cs.restated(g, pairs, P.FR)
    assert (st["total"], st["mapped"], st["negative"], st["edge_pairs"], st["ok"]) == (73, 0, 0, 0, False)
    assert hist == [] and points == []
    _compare(ctx, ix, g, pairs, P.FR, tmp_path, insert_size=400)


def test_b_adversarial_graph(ctx, tmp_path):
    """homopolymer loop A^22 between G A^21 and A^21 C, a palindromic segment, a circular segment (test_gpu_gmapper)"""
    rng = random.Random(127)
    k = 21
    x, y = "".join(rng.choice("ACGT") for _ in range(30)), "".join(rng.choice("ACGT") for _ in range(50))
    segs = ["A" * 22, "G" + "A" * 21, "A" * 21 + "C", x + rc(x), y + y[:k]]
    text = ("".join("S\t%d\t%s\n" % (3 + 2 * i, q) for i, q in enumerate(segs)) +
            "L\t3\t+\t3\t+\t21M\nL\t5\t+\t3\t+\t21M\nL\t3\t+\t7\t+\t21M\nL\t11\t+\t11\t+\t21M\n")
    gfa = tmp_path / "adv.gfa"
    gfa.write_text(text)
    g = G.Graph.from_gfa(text, k)
    assert g.conj[6] == 6 and g.loop1(0)
    ix = ctx.edgeindex_from_gfa(str(gfa), k)
    pal = x + rc(x)
    loop = ["G" + "A" * n + "C" for n in (21, 22, 25, 40)] + ["A" * 30, "T" * 30]
    circ = [(y * 5)[i:i + 140] for i in range(0, 50, 7)] + [rc(y * 3)[3:120]]
    mates = loop + circ + [pal, pal[2:50], rc(x)[4:] + x[:9], pal[:40]]
    pairs = [(a, b) for a in mates for b in (mates[::3] + [pal, pal[5:45]])]
    pairs += [(Cs.mutate(rng, a, 0.02, 0.01), Cs.mutate(rng, b, 0.02, 0.01)) for a, b in pairs[::2]]
    for orientation in (P.FF, P.FR, P.RF, P.RR):
        st, lib = _compare(ctx, ix, g, pairs, orientation, tmp_path, insert_size=90, threshold=1)
        # a pair on the palindromic segment is its own conjugate: e1 == conj e2, every weight doubled
        assert lib.counts.occ.get((6, 6), 0) >= 1 and (6, 6) in lib.index.store
        assert all(w % 2 == 0 for w in lib.index.store[(6, 6)].values())
        assert st["mapped"] + st["negative"] >= 1


def test_c_batching_gives_the_same_bytes(ctx, tmp_path):
    rng, genome, g, ix = _chain_graph(ctx, tmp_path)
    pairs = Cs.cut_pairs(rng, genome, 200)
    pairs = [(Cs.mutate(rng, a, 0.003, 0.004), Cs.mutate(rng, b, 0.003, 0.004)) for a, b in pairs]
    one = Cs.engine(ctx, ix, pairs, P.FR, threshold=1, round_distance=2, prd=str(tmp_path / "one.prd"))
    three = Cs.engine(ctx, ix, pairs, P.FR, threshold=1, round_distance=2, batches=[7, 129, 64],
                      prd=str(tmp_path / "three.prd"))
    assert _bits(one[0]) == _bits(three[0]) and one[1:] == three[1:]
    assert (tmp_path / "one.prd").read_bytes() == (tmp_path / "three.prd").read_bytes()
    st, hist, points, _ = Cs.restated(g, pairs, P.FR, threshold=1, round_distance=2)
    assert _bits(one[0]) == _bits(st) and one[1] == hist and one[2] == points and len(points) > 20
    # more batches than runs are kept before a merge
    many = Cs.engine(ctx, ix, pairs, P.FR, threshold=1, round_distance=2, batches=[10] * 20)
    assert _bits(many[0]) == _bits(st) and many[1:] == (hist, points)


@pytest.mark.parametrize("threshold", [0, 1, 2, 3])
def test_d_filter_thresholds(ctx, tmp_path, threshold):
    rng, genome, g, ix = _chain_graph(ctx, tmp_path)
    fp = lambda s, F: (genome[s:s + 100], rc(genome[s + F - 100:s + F]))  # noqa: E731
    # forward-strand pairs inside segment 0 (once), segment 1 (twice) and segment 2 (three times), and one from segment
    # 0 into segment 1: c = 1, 2, 3 and 1
    pairs = [fp(100, 300), fp(800, 300), fp(850, 320), fp(1600, 300), fp(1620, 310), fp(1650, 330), fp(500, 400)]
    st, lib = _compare(ctx, ix, g, pairs, P.FR, tmp_path, threshold=threshold, insert_size=300)
    assert {p: lib.counts.c(*p) for p in lib.counts.occ} == {(0, 0): 1, (2, 2): 2, (4, 4): 3, (0, 2): 1}
    kept = {(e1, e2) for e1, e2, _, _ in lib.points()}
    assert kept == [{(0, 0), (2, 2), (4, 4), (0, 2)}, {(2, 2), (4, 4)}, {(4, 4)}, set()][threshold]


@pytest.mark.parametrize("round_distance", [0, 1, 2, 5])
def test_d_rounding_with_negative_distances(ctx, tmp_path, round_distance):
    rng, genome, g, ix = _chain_graph(ctx, tmp_path)
    pairs = Cs.cut_pairs(rng, genome, 150)
    # insert_size 380 < most fragments: the distances insert_size - F are negative for most pairs, positive for a few
    st, lib = _compare(ctx, ix, g, pairs, P.FR, tmp_path, round_distance=round_distance, insert_size=380)
    # the distances of the points between two edges of one segment (a point stored under the conjugate pair keeps its
    # gap, which was taken with the length of the other edge)
    d = [gap + g.length(e1) for e1, e2, gap, _ in lib.points() if e1 // 2 == e2 // 2]
    assert min(d) < 0 < max(d)
    if round_distance > 1:
        assert all(x % round_distance == 0 for x in d)
    else:
        assert any(x % 5 for x in d)


def test_argument_errors(ctx, tmp_path):
    rng, genome, g, ix = _chain_graph(ctx, tmp_path)
    pairs = Cs.cut_pairs(rng, genome, 4)
    first, second = ctx.reads_from_ascii([a for a, _ in pairs]), ctx.reads_from_ascii([b for _, b in pairs])
    three = ctx.reads_from_ascii([b for _, b in pairs[:3]])
    pi = ix.pairinfo()
    with pytest.raises(B.BBKError, match="4 first mates and 3 second mates"):
        pi.push_estimate(first, three)
    with pytest.raises(B.BBKError, match="orientation 4"):
        pi.push_estimate(first, second, 4)
    with pytest.raises(B.BBKError, match="orientation -1"):
        pi.push_estimate(first, second, -1)
    with pytest.raises(B.BBKError, match="filter_threshold 2 needs"):
        pi.fill_begin(400, 0, 2)
    pi.fill_begin(400, 0, 0)
    with pytest.raises(B.BBKError, match="before bbk_pairinfo_estimate"):
        pi.push_fill(first, second)
    with pytest.raises(ValueError):
        ix.pairinfo().push_estimate(first, second, P.FR, np.zeros((3, 4), dtype=np.uint32))


# ---- (e) the tool -------------------------------------------------------------------------------------------------------

def _fastq(path, seqs):
    path.write_text("".join("@r%d/x\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(seqs)))
    return path.name


def _lib_yaml(tmp_path, name, pairs, orientation="fr", kind="paired-end", interlaced=False):
    left = _fastq(tmp_path / (name + "_1.fastq"), [a for a, _ in pairs])
    right = _fastq(tmp_path / (name + "_2.fastq"), [b for _, b in pairs])
    if interlaced:
        return '- orientation: "%s"\n  type: "%s"\n  interlaced reads:\n    - "%s"\n' % (orientation, kind, left)
    return ('- orientation: "%s"\n  type: "%s"\n  left reads:\n    - "%s"\n  right reads:\n    - "%s"\n' %
            (orientation, kind, left, right))


def _tool(bins, args):
    return subprocess.run([bins["spades-pairinfo"]] + [str(a) for a in args], capture_output=True, text=True)


def _expected_files(g, pairs, orientation, bound, threshold):
    """(is.hist, lib, prd or None) of one library as the tool writes them"""
    lib = P.Library(g, bound)
    lib.push_estimate(pairs, orientation)
    st = lib.estimate()
    hist = "".join("%d\t%d\n" % kv for kv in lib.hist()).encode()
    if not st["ok"]:
        return hist, P.lib_text(st).encode(), None
    lib.push_fill(pairs, orientation, int(st["mean"]), P.round_bound(st["deviation"], threshold), threshold)
    return hist, P.lib_text(st).encode(), P.prd_bytes(lib.points())


def test_e_tool_equals_restatement(ctx, bins, tmp_path):
    rng, genome, g, ix = _chain_graph(ctx, tmp_path)
    gfa = tmp_path / "chain.gfa"
    # the lengths are 679, 800, 700, 800 for a segment and for its conjugate: half of their sum is reached inside the 800s
    assert P.nx(g, 50) == 800 and sorted(g.length(e) for e in g.seq)[0] == 679
    lens, selfc = ix.segment_lengths()
    assert lens.tolist() == [679, 800, 700, 800] and not selfc.any()
    pairs = Cs.cut_pairs(rng, genome, 250)
    pairs = [(Cs.mutate(rng, a, 0.003, 0.004), Cs.mutate(rng, b, 0.003, 0.004)) for a, b in pairs]
    # the second library cannot be estimated: forward-strand fr pairs read as ff leave the mates on different strands
    fwd = [(genome[s:s + 100], rc(genome[s + 200:s + 300])) for s in range(50, 2600, 50)]
    y = tmp_path / "d.yaml"
    y.write_text(_lib_yaml(tmp_path, "a", pairs) + '- type: "single"\n  single reads:\n    - "a_1.fastq"\n' +
                 _lib_yaml(tmp_path, "b", fwd, "ff"))
    for extra, bound, threshold in ([[], 800, 2], [["--meta", "-b", "20000", "-t", "2"], 0, 1],
                                    [["--min-edge-length", "700", "--meta", "--filter-threshold", "0"], 700, 0]):
        prefix = tmp_path / ("out%d" % bound)
        r = _tool(bins, [gfa, y, prefix, "-k", "21"] + extra)
        assert r.returncode == 0, r.stderr
        assert "Min edge length for estimation: %d" % bound in r.stdout
        hist, lib, prd = _expected_files(g, pairs, P.FR, bound, threshold)
        assert prd is not None and len(prd) > 100
        assert open("%s.0.is.hist" % prefix, "rb").read() == hist
        assert open("%s.0.lib" % prefix, "rb").read() == lib
        assert open("%s.0.prd" % prefix, "rb").read() == prd
        assert not os.path.exists("%s.1.lib" % prefix) and "Library #1 (single)" in r.stdout
        hist2, lib2, prd2 = _expected_files(g, fwd, P.FF, bound, threshold)
        assert prd2 is None and hist2 == b"" and b"mapped 0\n" in lib2
        assert open("%s.2.is.hist" % prefix, "rb").read() == hist2
        assert open("%s.2.lib" % prefix, "rb").read() == lib2
        assert not os.path.exists("%s.2.prd" % prefix)
        assert "Unable to estimate insert size for paired library #2" in r.stdout
        assert "None of paired reads aligned properly" in r.stdout
    # the N50 bound keeps the insert sizes of the 679- and 700-long segments out: the two runs differ
    assert open("%s.0.is.hist" % (tmp_path / "out800"), "rb").read() != open("%s.0.is.hist" % (tmp_path / "out0"), "rb").read()


def test_e_tool_refusals(ctx, bins, tmp_path):
    rng, genome, g, ix = _chain_graph(ctx, tmp_path)
    gfa = tmp_path / "chain.gfa"
    pairs = Cs.cut_pairs(rng, genome, 20)
    short = [(a[:15], b[:18]) for a, b in pairs]
    cases = [(_lib_yaml(tmp_path, "m", pairs, "rf", "mate-pairs"), "mate-pair", 0),
             (_lib_yaml(tmp_path, "g", pairs) + _lib_yaml(tmp_path, "i", pairs, interlaced=True), "interlaced", 1),
             (_lib_yaml(tmp_path, "s", short), "shorter than K", 0)]
    for j, (text, word, lib) in enumerate(cases):
        y = tmp_path / ("r%d.yaml" % j)
        y.write_text(text)
        prefix = tmp_path / ("r%d" % j)
        r = _tool(bins, [gfa, y, prefix, "-k", "21"])
        assert r.returncode != 0 and word in r.stderr and "library #%d" % lib in r.stderr, r.stderr
        assert not os.path.exists("%s.%d.prd" % (prefix, lib))
    y = tmp_path / "ok.yaml"
    y.write_text(_lib_yaml(tmp_path, "o", pairs))
    assert _tool(bins, [gfa, y, tmp_path / "x"]).returncode == 1  # -k is required
    assert _tool(bins, [gfa, y, tmp_path / "x", "-k", "21", "--bogus"]).returncode == 1
    r = _tool(bins, [tmp_path / "g.grseq", y, tmp_path / "x", "-k", "21"])
    assert r.returncode != 0 and "GFA" in r.stderr
