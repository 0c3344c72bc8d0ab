"""CPU: the restatement of spades-gmapper (tests/gmapper_restated.py) on hand-built graphs whose outputs are worked out
by hand: gap closing (unique, decided by coverage, decided by tie order, over the 70 bp bound), both filter thresholds,
N-split contigs, duplicate and reverse-complement contigs, a self-conjugate segment, a homopolymer self-loop and a
partial junction where LinkEdges differs from joining vertices; the position-local rule of the kernel against the literal
MapSequence on oracle graphs; and the tool's refusals that need no GPU."""
import os
import random
import subprocess

import pytest

from oracle import oracle as O
from spades_for_blackbird_amd import build, build_host
from tests import gmapper_restated as G
from tests import unitig_profile_restated as U
from tests.helpers import rc

K = 21


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _other(rng, s):
    """a string as long as s that differs from it at every position"""
    return "".join(rng.choice("ACGT".replace(c, "")) for c in s)


def _gfa(segs, links, kc=None):
    """S lines named 3, 5, 7, ... (with KC:i: when given), L lines (i, oi, j, oj) over segment indices"""
    s = "".join("S\t%d\t%s%s\n" % (3 + 2 * i, q, "\tKC:i:%d" % kc[i] if kc else "") for i, q in enumerate(segs))
    return s + "".join("L\t%d\t%s\t%d\t%s\t%dM\n" % (3 + 2 * a, oa, 3 + 2 * b, ob, K) for a, oa, b, ob in links)


def _lines(text, tag):
    return [line for line in text.splitlines() if line.startswith(tag + "\t")]


def _chain(seed, mid):
    """genome p + m + s cut into A = p, B = the last k of p + m + the first k of s, C = s; links A+B+, B+C+"""
    rng = random.Random(seed)
    p, m, s = _rand(rng, 150), _rand(rng, mid), _rand(rng, 200)
    g = G.Graph.from_gfa(_gfa([p, p[-K:] + m + s[:K], s], [(0, "+", 1, "+"), (1, "+", 2, "+")]), K)
    return rng, p, m, s, g


def test_unique_gap_closure():
    rng, p, m, s, g = _chain(1, 20)  # B: 41 (k+1)-mers, within the 70 bp bound
    out = G.gmapper(g, [p + _other(rng, m) + s])  # B itself is not on the contig
    assert _lines(out, "P") == ["P\tPATH_1_length_3_weigth_1_1\t3+,5+,7+\t*\tZ:W:1"]
    assert _lines(out, "L") == ["L\t3\t+\t5\t+\t21M", "L\t5\t+\t7\t+\t21M"]
    assert _lines(out, "S")[0] == "S\t3\t%s\tDP:f:0\tKC:i:0" % p


@pytest.mark.parametrize("kc,closure", [((0, 10, 50, 0), "7+"), ((0, 50, 10, 0), "5+"), ((0, 20, 20, 0), "5+")])
def test_two_closures_by_coverage_then_order(kc, closure):
    """A -> {B1, B2} -> C: both at the same distance; the DFS takes the higher coverage first, on a tie the incoming
    order (B1, the lower id)"""
    rng = random.Random(3)
    p, s, x1, x2 = _rand(rng, 150), _rand(rng, 200), _rand(rng, 10), _rand(rng, 10)
    segs = [p, p[-K:] + x1 + s[:K], p[-K:] + x2 + s[:K], s]
    links = [(0, "+", 1, "+"), (0, "+", 2, "+"), (1, "+", 3, "+"), (2, "+", 3, "+")]
    g = G.Graph.from_gfa(_gfa(segs, links, kc), K)
    junk = "".join(rng.choice([c for c in "ACGT" if c not in (a, b)]) for a, b in zip(x1, x2))
    out = G.gmapper(g, [p + junk + s])
    assert _lines(out, "P") == ["P\tPATH_1_length_3_weigth_1_1\t3+,%s,9+\t*\tZ:W:1" % closure]
    assert _lines(out, "S")[1].endswith("\tDP:f:%s\tKC:i:%d" % ("%g" % (kc[1] / 31), kc[1]))
    assert _lines(out, "L") == ["L\t3\t+\t5\t+\t21M", "L\t3\t+\t7\t+\t21M", "L\t5\t+\t9\t+\t21M", "L\t7\t+\t9\t+\t21M"]


def test_gap_over_the_bound_splits_the_contig():
    rng, p, m, s, g = _chain(4, 60)  # B: 81 (k+1)-mers > 70
    out = G.gmapper(g, [p + _other(rng, m) + s])
    assert _lines(out, "P") == ["P\tPATH_1_length_1_weigth_1_1\t3+\t*\tZ:W:1", "P\tPATH_2_length_1_weigth_1_1\t7+\t*\tZ:W:1"]


def test_filter_thresholds():
    rng = random.Random(5)
    long_seg, short_seg = _rand(rng, 1000 + K), _rand(rng, 50 + K)
    g = G.Graph.from_gfa(_gfa([long_seg, short_seg], []), K)

    def paths(c):
        return _lines(G.gmapper(g, [c]), "P")

    assert paths(long_seg[:101 + K]) == ["P\tPATH_1_length_1_weigth_1_1\t3+\t*\tZ:W:1"]  # 101 > 100, ratio 0.101
    assert paths(long_seg[:100 + K]) == []  # 100: neither threshold
    assert paths(short_seg[:16 + K]) == ["P\tPATH_1_length_1_weigth_1_1\t5+\t*\tZ:W:1"]  # 16 / 50 = 0.32
    assert paths(short_seg[:15 + K]) == []  # 15 / 50 = 0.3 is not greater
    assert not G.gr(0.3, 0.3) and not G.gr(0.30000000000000004, 0.3) and G.gr(0.3000001, 0.3)


def test_n_split_contig():
    rng = random.Random(6)
    seg = _rand(rng, 200)
    g = G.Graph.from_gfa(_gfa([seg], []), K)
    contig = seg[:40] + "NNN" + seg[50:90].lower()
    assert G.pieces(contig) == [(0, seg[:40]), (43, seg[50:90])]
    assert G.map_read(g, contig) == [(0, [0, 19, 0, 19]), (0, [43, 62, 50, 69])]
    # one run of the edge: 38 of 179 (k+1)-mers is below both thresholds
    assert _lines(G.gmapper(g, [contig]), "P") == []
    with pytest.raises(ValueError):
        G.pieces("ACGTRACGT")


def test_duplicate_and_reverse_complement_contigs():
    _, p, m, s, g = _chain(7, 20)
    genome = p + m + s
    assert _lines(G.gmapper(g, [genome, genome]), "P") == ["P\tPATH_1_length_3_weigth_2_1\t3+,5+,7+\t*\tZ:W:2"]
    assert _lines(G.gmapper(g, [genome, rc(genome)]), "P") == ["P\tPATH_1_length_3_weigth_1_1\t3+,5+,7+\t*\tZ:W:1",
                                                                 "P\tPATH_2_length_3_weigth_1_1\t7-,5-,3-\t*\tZ:W:1"]


def test_self_conjugate_segment():
    rng = random.Random(8)
    x = _rand(rng, 30)
    q = x + rc(x)
    g = G.Graph.from_gfa(_gfa([q], []), K)
    assert g.conj[0] == 0 and 1 not in g.seq
    assert G.map_sequence(g, q) == [(0, [0, 39, 0, 39])]
    assert G.map_sequence(g, q[5:50]) == [(0, [0, 24, 5, 29])]
    assert G.map_sequence_local(g, rc(q)[3:44]) == G.map_sequence(g, rc(q)[3:44])
    assert _lines(G.gmapper(g, [q]), "P") == ["P\tPATH_1_length_1_weigth_1_1\t3+\t*\tZ:W:1"]


def test_homopolymer_self_loop():
    """A^22 linked to itself: TryThread re-enters it at every A, one range per position (the index's loop flag)"""
    segs = ["A" * 22, "G" + "A" * 21, "A" * 21 + "C"]
    g = G.Graph.from_gfa(_gfa(segs, [(0, "+", 0, "+"), (1, "+", 0, "+"), (0, "+", 2, "+")]), K)
    contig = "G" + "A" * 25 + "C"
    exp = [(2, [0, 1, 0, 1])] + [(0, [i, i + 1, 0, 1]) for i in range(1, 5)] + [(4, [5, 6, 0, 1])]
    assert G.map_sequence(g, contig) == exp
    assert G.map_sequence_local(g, contig) == exp
    assert g.loop1(0) and g.index_loop1(0)
    assert _lines(G.gmapper(g, [contig]), "P") == ["P\tPATH_1_length_3_weigth_1_1\t5+,3+,7+\t*\tZ:W:1"]


def test_partial_junction_link_edges_moves():
    """A->B, C->D, A->D and no C->B: joining vertices puts all four at one vertex; LinkEdges moves D to the end of C
    and, through the complement arc D- -> A-, A with it, leaving B's start alone"""
    rng = random.Random(9)
    kmer = _rand(rng, K)
    a, c = _rand(rng, 40) + "G" + kmer, _rand(rng, 40) + "T" + kmer
    b, d = kmer + "A" + _rand(rng, 40), kmer + "C" + _rand(rng, 40)
    text = _gfa([a, b, c, d], [(0, "+", 1, "+"), (2, "+", 3, "+"), (0, "+", 3, "+")])
    g = G.Graph.from_gfa(text, K)
    assert g.end[0] == g.end[4] == g.start(6) and g.start(2) != g.end[0]
    assert 2 in U.Graph.from_gfa(text, K).outgoing_of_end(0)  # union-find keeps A -> B
    out = G.write_gfa(g, [])
    assert _lines(out, "L") == ["L\t3\t+\t9\t+\t21M", "L\t7\t+\t9\t+\t21M"]
    # a contig through A and B: no closure from the end of A to B's start (a vertex with no way in)
    assert _lines(G.gmapper(g, [a + b[K:]]), "P") == ["P\tPATH_1_length_1_weigth_1_1\t3+\t*\tZ:W:1",
                                                       "P\tPATH_2_length_1_weigth_1_1\t5+\t*\tZ:W:1"]


def test_gfa_arcs_complements_and_order():
    # an L line and its own complement in the file are one link each way; a missing complement is added after the
    # file's arcs, and arcs are grouped by source with file order kept
    assert G.gfa_arcs([(0, "+", 1, "+"), (1, "-", 0, "-")]) == [(0, 2), (3, 1)]
    assert G.gfa_arcs([(1, "+", 0, "+"), (0, "+", 1, "-")]) == [(0, 3), (1, 3), (2, 0), (2, 1)]


@pytest.mark.parametrize("k,seed", [(5, 1), (7, 2), (21, 3)])
def test_position_local_equals_literal_on_oracle_graphs(k, seed):
    rng = random.Random(seed)
    genome = _rand(rng, 300 if k < 21 else 2000)
    reads = []
    for _ in range(60):
        st = rng.randint(0, len(genome) - 4 * k)
        r = genome[st:st + rng.randint(2 * k, 4 * k)]
        reads.append(rc(r) if rng.random() < 0.5 else r)
    g = G.Graph.from_gfa(O.ExtIndex(reads, k, 1).unitigs().gfa()[0], k)
    for _ in range(80):
        st = rng.randint(0, len(genome) - 60)
        s = "".join(c if rng.random() > 0.02 else rng.choice("ACGT") for c in genome[st:st + rng.randint(k, 120)])
        s = rc(s) if rng.random() < 0.5 else s
        assert G.map_sequence_local(g, s) == G.map_sequence(g, s), s


@pytest.fixture(scope="module")
def gmapper_bin():
    build.build()
    return [p for p in build_host.build() if os.path.basename(p) == "spades-gmapper"][0]


def test_cli_refusals_before_the_gpu(gmapper_bin, tmp_path):
    """argv, library types and the graph format are checked before a device is opened"""
    fa = tmp_path / "c.fasta"
    fa.write_text(">c\nACGT\n")
    gfa = tmp_path / "g.gfa"
    gfa.write_text("S\t3\t%s\n" % ("A" * 30))

    def run(args):
        return subprocess.run([gmapper_bin] + [str(a) for a in args], capture_output=True, text=True)

    assert run([]).returncode == 1
    for typ, word in (("trusted-contigs", "trusted"), ("pacbio", "long-read"), ("nanopore", "long-read")):
        y = tmp_path / ("%s.yaml" % typ)
        y.write_text('- type: %s\n  single reads:\n    - "%s"\n' % (typ, fa))
        r = run([y, gfa, tmp_path / "o.gfa"])
        assert r.returncode > 0 and word in r.stderr, (typ, r.stderr)
    y = tmp_path / "u.yaml"
    y.write_text('- type: untrusted-contigs\n  single reads:\n    - "%s"\n' % fa)
    r = run([y, tmp_path / "g.grseq", tmp_path / "o.gfa"])
    assert r.returncode > 0 and "GFA" in r.stderr
    assert not (tmp_path / "o.gfa").exists()
