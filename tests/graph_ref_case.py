"""The inputs of the reference-recorded graph-side fixtures (tests/golden/graph_ref/, oracle/record_graph_ref.py) and the
reader of those fixtures.  Pure Python; no GPU, no engine, no reference tree.

Crafted graphs (raw points in, lengths and clusters out): the graphs of tests/distest_cases.py with the raw points their
tests use.  Where a search of a case runs into its limits (500 calls or more, a ball of 2999 vertices or more) the KC tags
are rewritten so that every segment has a coverage of its own (`distinct_kc`): the reference then breaks no tie of
(distance, -coverage) by its edge ids, which a fixture could not reproduce.

Read-level graphs (read pairs in; map, is, pairs, raw, lengths, clustered out):
  synth      the 20 000-base genome of Context.reads_synth(seed_genome = 21) as one segment, pairs of an fr library
             with substitutions and Ns, one mate of 15 bases, one mate without a valid base;
  junctions  a Builder graph with a bubble, a one-edge loop, a palindromic segment, a circular segment and two long
             edges; pairs of 100-150 bases cut from walks through it, presented under each of ff, fr, rf and rr.
"""
import gzip
import json
import os
import random

from tests import distest_cases as Cs
from tests import distest_restated as D
from tests import gmapper_restated as G
from tests import pairinfo_cases as PCs
from tests import pairinfo_restated as P
from tests.helpers import rc

K = Cs.K
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = os.path.join(HERE, "golden", "graph_ref")
ORIENTATIONS = {"ff": P.FF, "fr": P.FR, "rf": P.RF, "rr": P.RR}

# (mean, deviation, read length, linkage coeff, max distance coeff, clustered threshold) of estimate_distance;
# deviation 40 with these coefficients gives the integers of distest_cases.params
DEFAULT = (400.0, 40.0, 100, 0.0, 2.0, 2.0)


def de(insert_size=400.0, linkage=0.0, max_distance=2.0, threshold=2.0, deviation=40.0):
    return (float(insert_size), deviation, 100, linkage, max_distance, threshold)


def ulps_above(x, n):
    import struct
    return struct.unpack("<d", struct.pack("<Q", struct.unpack("<Q", struct.pack("<d", x))[0] + n))[0]


def distinct_kc(gfa):
    """every S line's KC:i: rewritten to length * (3 + its number): a coverage of its own per segment"""
    out, i = [], 0
    for line in gfa.splitlines(True):
        f = line.rstrip("\n").split("\t")
        if f[0] == "S":
            f = f[:3] + ["KC:i:%d" % ((len(f[2]) - K) * (3 + i))]
            i += 1
            line = "\t".join(f) + "\n"
        out.append(line)
    return "".join(out)


def crafted_cases():
    """{case: (gfa, host points [(e1, e2, gap, weight)], [de tuples])}"""
    out = {}
    b, (A, M, B) = Cs.single_path()
    out["single_path"] = (b.gfa(), [(A, B, 48, 3), (A, B, 55, 2)],
                          [DEFAULT, de(threshold=0.5), (399.5, 40.9, 100, 0.5, 2.0, 2.0), (399.49, 40.9, 100, 0.5, 2.0, 2.0)])
    # a cluster of weight exactly 2: kept at a threshold 3 ULPs above 2, dropped at 5 ULPs above (math::ge)
    out["single_path_ulp"] = (b.gfa(), [(A, B, 48, 2)],
                              [DEFAULT, de(threshold=ulps_above(2.0, 3)), de(threshold=ulps_above(2.0, 5))])
    b, (A, arms, B) = Cs.bubble()
    out["bubble"] = (b.gfa(), [(A, B, 30, 4), (A, B, 45, 2), (A, B, 58, 3), (A, B, 145, 7), (A, B, 320, 1), (A, B, -101, 9)],
                     [DEFAULT, de(threshold=0.0), de(linkage=0.75, threshold=0.0), de(linkage=4.25)])
    b, (A, C, B) = Cs.cycle_between()
    # d = -1 (gap -101) has 2 d + len2 < len1 and is skipped, though it lies within max_distance = 1000 of the length 100;
    # d = 0 (gap -100) does not and goes to 100
    out["cycle_between"] = (b.gfa(), [(A, B, 0, 3), (A, B, 215, 4), (A, B, -101, 9), (A, B, -100, 5)],
                            [de(max_distance=25.0, threshold=0.0)])
    b, (A, R) = Cs.cycle_through()
    out["cycle_through"] = (b.gfa(), [(A, A, -100, 3), (A, A, 71, 2), (A, A + 1, 0, 1)], [de(threshold=0.0), DEFAULT])
    b, (A, B) = Cs.no_path()
    out["no_path"] = (b.gfa(), [(A, B, 30, 5)], [de(threshold=0.0)])
    b, (A, Pl, Q) = Cs.hairpin()
    out["hairpin"] = (b.gfa(), [(A, A + 1, 41, 3), (Pl, Pl, -41, 2), (A, Q, 0, 2), (Pl, A + 1, 0, 5), (A, Pl, 0, 5),
                                (Q + 1, Pl, 41, 2)], [DEFAULT, de(threshold=0.0)])
    b, (A, edges, depths) = Cs.tree(65)
    out["tree_65"] = (b.gfa(), Cs.pair_points([(A, e) for e in edges], [100 + 23 * d for d in depths]),
                      [de(insert_size=300, threshold=1.0)])
    for calls, shape in sorted(Cs.BOUNDARY.items()):
        b, (A, B) = Cs.bubble_chain(*shape)
        mid = 2 * (len(b.segs) - 2)
        gfa = b.gfa() if calls < 500 else distinct_kc(b.gfa())
        out["bubble_chain_%d" % calls] = (gfa, [(A, B, 990, 3), (A, B, 1013, 2), (A, mid, 970, 2)], [de(insert_size=1200)])
    gfa, (A, B) = Cs.one_mer_chain(600)
    out["one_mer_chain_600"] = (gfa, [(A, B, 600, 3)], [de(insert_size=700)])
    gfa, (A, B) = Cs.one_mer_chain(3000)
    out["one_mer_chain_3000"] = (distinct_kc(gfa), [(A, B, 3000, 3)], [de(insert_size=3100)])
    for seed in (0, 1, 2):
        b = Cs.random_graph(seed)
        out["random_%d" % seed] = (distinct_kc(b.gfa()), Cs.random_points(b.graph(), seed), [de(linkage=(0.0, 0.125, 0.0)[seed])])
    return out


# ---- read-level graphs --------------------------------------------------------------------------------------------------

def spell(g, walk):
    s = g.seq[walk[0]]
    for a, b in zip(walk, walk[1:]):
        assert g.end[a] == g.start(b), (a, b)
        s += g.seq[b][g.k:]
    return s


def junction_graph():
    """(gfa, walks as sequences, {name: edge})"""
    b = Cs.Builder(seed=71)
    v = [b.vertex() for _ in range(7)]
    L = 2 * b.edge(v[0], v[1], 700)
    m1, m2 = 2 * b.edge(v[1], v[2], 30), 2 * b.edge(v[1], v[2], 45)
    e3 = 2 * b.edge(v[2], v[3], 25)
    loop = 2 * b.edge(v[3], v[3], 24)
    e4 = 2 * b.edge(v[3], v[4], 60)
    pal = 2 * b.palindrome(v[4], 41)
    e5 = 2 * b.edge(v[4], v[5], 600)
    circ = 2 * b.edge(v[6], v[6], 120)
    g = b.graph()
    c = lambda e: g.conj[e]  # noqa: E731
    walks = [[L, m1, e3, loop, loop, e4, e5],
             [L, m2, e3, e4, pal, c(e4), c(loop), c(e3), c(m1), c(L)],
             [L, m2, e3, loop, e4, e5],
             [c(e5), c(e4), c(e3), c(m2), c(L)],
             [circ] * 5]
    return b.gfa(), [spell(g, w) for w in walks], dict(L=L, m1=m1, m2=m2, e3=e3, loop=loop, e4=e4, pal=pal, e5=e5, circ=circ)


def cut_from_walks(rng, walks, n, orientation):
    """n pairs whose mates, as the library's orientation presents them, are a forward first mate and a forward second
    mate further along one strand of a walk; every seventh pair is left as an fr pair whatever the orientation"""
    pairs = []
    for i in range(n):
        w = rng.choice(walks)
        la, lb = rng.randint(100, 150), rng.randint(100, 150)
        F = max(la, lb, min(len(w), int(round(rng.gauss(330, 30)))))
        a = rng.randint(0, len(w) - F)
        frag = w[a:a + F]
        if rng.random() < 0.5:
            frag = rc(frag)
        first, second = frag[:la], frag[-lb:]  # both forward
        o = P.FR if i % 7 == 6 else orientation
        if o in (P.RF, P.RR):
            first = rc(first)
        if o in (P.FR, P.RR):
            second = rc(second)
        pairs.append((first, second))
    return pairs


def special_pairs(pairs, rng):
    """Ns, a mate shorter than k + 1, a mate whose longest valid stretch is shorter than k + 1, a mate without a base"""
    pairs = [(PCs.mutate(rng, a, 0.004, 0.003), PCs.mutate(rng, b, 0.004, 0.003)) for a, b in pairs]
    a, b = pairs[1]
    pairs[1] = (a, b[:15])
    a, b = pairs[2]
    pairs[2] = ("".join("N" if i % 20 == 19 else c for i, c in enumerate(a)), b)
    a, b = pairs[3]
    pairs[3] = (a[:60] + "N" + a[61:], "N" * 30)
    a, b = pairs[4]
    pairs[4] = (a[:K + 1], b.lower())
    return pairs


# the seeds of the junction cases' pairs: the first at which the reference's counting Bloom filter answers
# min(count, 3) for every edge pair (its first hash does not see the second edge, so a small case collides easily)
JUNCTION_SEEDS = {"ff": 1, "fr": 0, "rf": 1, "rr": 1}


def read_cases(seeds=None):
    """{case: dict(gfa, pairs, orientation, edge_length_bound, fills, de, seqs)}; a `de` entry is (read length, linkage
    coeff, max distance coeff, clustered threshold): mean and deviation are the reference's own, of its is stage"""
    seeds = seeds or JUNCTION_SEEDS
    out = {}
    genome = PCs.synth_genome(21, 20000)
    rng = random.Random(5)
    pairs = special_pairs(PCs.cut_pairs(rng, genome, 120), rng)
    out["synth_fr"] = dict(gfa="S\tg1\t%s\tKC:i:%d\n" % (genome, 7 * (len(genome) - K)), pairs=pairs, orientation="fr",
                           edge_length_bound=500, fills=[(0, 0), (1, 0), (0, 4), (1, 4)], de=[(150, 0.0, 2.0, 1.5)], seqs=[genome[100:300], rc(genome[5000:5100]), genome[:K]])
    gfa, walks, named = junction_graph()
    g = G.Graph.from_gfa(gfa, K)
    seqs = [walks[0][680:820], walks[1][700:900], g.seq[named["loop"]] + g.seq[named["loop"]][K:], walks[4][60:300],
            g.seq[named["pal"]], walks[0][:K + 1], walks[0][1:K + 1]]
    for name, o in sorted(ORIENTATIONS.items()):
        rng = random.Random(seeds[name])
        out["junctions_" + name] = dict(gfa=gfa, pairs=special_pairs(cut_from_walks(rng, walks, 50, o), rng), orientation=name,
                                        edge_length_bound=100, fills=[(0, 0), (1, 0), (0, 4), (1, 4)],
                                        de=[(150, 0.0, 2.0, 1.0), (150, 0.5, 2.0, 0.0)], seqs=seqs)
    return out


# ---- the fixtures -------------------------------------------------------------------------------------------------------

def names():
    return sorted(f[:-len(".json.gz")] for f in os.listdir(FIXTURES) if f.endswith(".json.gz"))


_CACHE = {}


def load(case):
    if case not in _CACHE:
        with gzip.open(os.path.join(FIXTURES, case + ".json.gz"), "rt") as f:
            _CACHE[case] = json.load(f)
    return _CACHE[case]


def graph(fx):
    return G.Graph.from_gfa(fx["gfa"], fx["k"])


def edge(g, name, o):
    """the restatements' number of a named oriented edge"""
    e = 2 * g.names.index(name)
    return e if o == "+" or g.conj[e] == e else e + 1


def named(g, e):
    return [g.names[e // 2], "-" if e & 1 else "+"]


def f32(bits):
    import struct
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def f64(hexbits):
    import struct
    return struct.unpack("<d", struct.pack("<Q", int(hexbits, 16)))[0]


def raw_points(g, rows):
    """[(e1, e2, gap, weight)] ascending, of dumped rows [n1, o1, n2, o2, d bits, weight bits]: integers, exact"""
    out = []
    for n1, o1, n2, o2, d, w in rows:
        e1, e2 = edge(g, n1, o1), edge(g, n2, o2)
        d, w = f32(d), f32(w)
        assert d == int(d) and w == int(w) and abs(d) < 1 << 23 and w < 1 << 23
        out.append((e1, e2, int(d) - g.length(e1), int(w)))
    return sorted(out)


def params(row):
    """D.Params of a recorded `de` entry, from the integers the reference derived"""
    return D.Params(row["insert_size"], row["read_length"], row["delta"], row["linkage_distance"], row["max_distance"],
                    f64(row["threshold"]))


def uleb(data, at):
    v, shift = 0, 0
    while True:
        b = data[at]
        at += 1
        v |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            return v, at


def decode_prd(data, id_name=None):
    """the one reader of PairedBuffer::BinWrite for both byte streams: the number of first edges, per first edge its id,
    per stored second edge its id, the number of points and 8-byte points, and a 0.  Returns
    {(first, second): [point bytes]} with ids translated by id_name; raises on a framing error or trailing bytes"""
    tr = (lambda x: x) if id_name is None else (lambda x: id_name[x])
    n, at = uleb(data, 0)
    out = {}
    for _ in range(n):
        e1, at = uleb(data, at)
        assert e1 != 0
        while True:
            e2, at = uleb(data, at)
            if e2 == 0:
                break
            cnt, at = uleb(data, at)
            key = (tr(e1), tr(e2))
            assert key not in out and cnt > 0
            out[key] = [bytes(data[at + 8 * j:at + 8 * j + 8]) for j in range(cnt)]
            assert len(out[key][-1]) == 8
            at += 8 * cnt
    assert at == len(data), "trailing bytes"
    return out


# ---- what both test modules read from a fixture --------------------------------------------------------------------------
CRAFTED = ["single_path", "single_path_ulp", "bubble", "cycle_between", "cycle_through", "no_path", "hairpin", "tree_65",
           "bubble_chain_499", "bubble_chain_500", "one_mer_chain_600", "one_mer_chain_3000", "random_0", "random_1", "random_2"]
READS = ["synth_fr", "junctions_ff", "junctions_fr", "junctions_rf", "junctions_rr"]

_G = {}


def case_graph(case):
    if case not in _G:
        _G[case] = graph(load(case))
    return _G[case]


def id_names(g, table):
    return {int(i): edge(g, n, o) for i, (n, o) in table.items()}


def stored(case):
    g, ref = case_graph(case), load(case)["ref"]
    return raw_points(g, (ref["points"] if "points" in ref else ref["raw"][0])["half"])


def left_out(case):
    g = case_graph(case)
    return {(edge(g, r[0], r[1]), edge(g, r[2], r[3])) for r in load(case)["left_out"]}


def clustered_rows(g, rows):
    """[(e1, e2, centre bits, half-span bits, weight bits)] ascending by (e1, e2, centre)"""
    out = [(edge(g, r[0], r[1]), edge(g, r[2], r[3]), r[4], r[5], r[6]) for r in rows]
    return sorted(out, key=lambda r: (r[0], r[1], f32(r[2])))
