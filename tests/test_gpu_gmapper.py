"""GPU: spades-gmapper.  (a) the ranges of bbk_edgeindex_map_paths equal the restated MapSequence
(tests/gmapper_restated.py) for k in {21, 33, 55, 77, 127} on reads with substitutions and Ns, over gbuilder graphs and
over a homopolymer loop, a palindromic segment and a circular segment, and at the wave and block edges of the position
lookup of the two mapping kernels; (b) the CLI on a gbuilder GFA with contigs cut from the genome equals the
restatement byte for byte, and its S/L part equals the input graph up to gfa_canon; (c) every segment as a contig is a
one-edge path of weight 1; (d) consecutive edges of a P line are linked; (e) refusals, the last contig library wins, and
no file without one."""
import os
import random
import subprocess

import numpy as np
import pytest

import spades_for_blackbird_amd as B
from spades_for_blackbird_amd import build, build_host
from spades_for_blackbird_amd.tools import gfa_canon
from tests import gmapper_restated as G
from tests import unitig_profile_restated as R
from tests.helpers import rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bins():
    build.build()
    return {os.path.basename(p): p for p in build_host.build()}


@pytest.fixture(scope="module")
def ctx():
    c = B.Context(0)
    yield c
    c.close()


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _mutate(rng, s, sub=0.01, n=0.004):
    out = []
    for c in s:
        x = rng.random()
        out.append("N" if x < n else rng.choice("ACGT".replace(c, "")) if x < n + sub else c)
    return "".join(out)


def _check_ranges(ctx, ix, g, reads):
    """map_paths of the N-free pieces equals MapSequence piece by piece; returns the number of ranges"""
    pieces = [q for r in reads for _, q in G.pieces(r)]
    off, rec = ix.map_paths(ctx.reads_from_ascii(pieces))
    assert len(off) == len(pieces) + 1 and int(off[-1]) == len(rec)
    for i, q in enumerate(pieces):
        got = [(int(x["edge"]), [int(x["init_start"]), int(x["init_end"]), int(x["map_start"]), int(x["map_end"])])
               for x in rec[int(off[i]):int(off[i + 1])]]
        assert got == G.map_sequence(g, q), (i, q)
        assert all(int(x) == i for x in rec["read"][int(off[i]):int(off[i + 1])])
    return len(rec)


def _cut_genome_gfa(rng, path, k):
    """a random 3 kb genome as four segments that overlap by k, linked in a chain: the graph of a repeat-free genome.
    gbuilder cannot make it at k = 127, where the (k+1)-mers its extension index is built from are no legal k-mers"""
    genome = _rand(rng, 3000)
    cuts = [0, 700, 1500, 2200, 3000]
    segs = [genome[max(0, a - k):b] for a, b in zip(cuts, cuts[1:])]
    path.write_text("".join("S\t%d\t%s\n" % (3 + 2 * i, q) for i, q in enumerate(segs)) +
                    "".join("L\t%d\t+\t%d\t+\t%dM\n" % (3 + 2 * i, 5 + 2 * i, k) for i in range(len(segs) - 1)))
    return genome


@pytest.mark.parametrize("k", [21, 33, 55, 77, 127])
def test_a_ranges_on_gbuilder_graphs(ctx, tmp_path, k):
    # The (k+1)-mers of k = 77 and 127 take three and four key words.  A 150-base read holds few of them and _mutate
    # changes 1.4 % of its bases, so the floor on the number of ranges there comes from the reads left untouched: they
    # map (the graph holds their (k+1)-mers), and 600 x 0.986^150 = 72 are expected; half of that is the floor.
    min_ranges = 600 if k <= 55 else 36
    rng = random.Random(k)
    gfa = tmp_path / "g.gfa"
    if k < 127:
        r = ctx.reads_synth(3000, read_len=150, genome_len=20000, sub_rate=0.003, seed_genome=k, seed_reads=k + 1)
        ctx.unitigs(ctx.extindex(r, k)).write_gfa(str(gfa))
        reads = r.to_list()[:600]
    else:  # no gbuilder graph at the largest k: the cut genome, 150-base reads of both strands
        genome = _cut_genome_gfa(random.Random(k + 1), gfa, k)
        starts = [rng.randint(0, len(genome) - 150) for _ in range(600)]
        reads = [genome[st:st + 150] if i % 2 else rc(genome[st:st + 150]) for i, st in enumerate(starts)]
    g = G.Graph.from_gfa(gfa.read_text(), k)
    ix = ctx.edgeindex_from_gfa(str(gfa), k)
    reads = [_mutate(rng, s) for s in reads] + ["ACGT", "N" * 10, ""]
    assert _check_ranges(ctx, ix, g, reads) > min_ranges


def test_a_ranges_k127_and_adversarial_graphs(ctx, tmp_path):
    rng = random.Random(127)
    k = 127
    gfa = tmp_path / "g127.gfa"
    genome = _cut_genome_gfa(rng, gfa, k)
    reads = []
    for _ in range(300):
        st = rng.randint(0, len(genome) - 400)
        s = _mutate(rng, genome[st:st + rng.randint(150, 400)], 0.003, 0.002)
        reads.append(rc(s) if rng.random() < 0.5 else s)
    _check_ranges(ctx, ctx.edgeindex_from_gfa(str(gfa), k), G.Graph.from_gfa(gfa.read_text(), k), reads)
    # k = 21: a homopolymer loop A^22 between G A^21 and A^21 C, a palindromic segment, a circular segment
    k = 21
    x, y = _rand(rng, 30), _rand(rng, 50)
    segs = ["A" * 22, "G" + "A" * 21, "A" * 21 + "C", x + rc(x), y + y[:k]]
    text = ("".join("S\t%d\t%s\n" % (3 + 2 * i, q) for i, q in enumerate(segs)) +
            "L\t3\t+\t3\t+\t21M\nL\t5\t+\t3\t+\t21M\nL\t3\t+\t7\t+\t21M\nL\t11\t+\t11\t+\t21M\n")
    gfa = tmp_path / "adv.gfa"
    gfa.write_text(text)
    g = G.Graph.from_gfa(text, k)
    assert g.conj[6] == 6 and g.loop1(0)
    reads = ["G" + "A" * n + "C" for n in (21, 22, 25, 40)] + ["A" * 30, "T" * 30, x + rc(x), rc(x)[4:] + x[:9]]
    reads += [(y * 5)[i:i + 140] for i in range(0, 50, 7)] + [rc(y * 3)[3:120], _mutate(rng, y * 4, 0.02, 0.01)]
    _check_ranges(ctx, ctx.edgeindex_from_gfa(str(gfa), k), g, reads)


@pytest.mark.parametrize("k", [21, 33])
def test_a_ranges_at_wave_and_block_edges(ctx, tmp_path, k):
    """The position lookup of k_gm_paths and k_ep_map: a wave takes 63 positions of the concatenated reads in lanes
    1..63 and its lane 0 looks up the position before them; a block takes 4 waves, 252 positions.  One segment with 300
    (k+1)-mers, one and two key words; every batch of reads is its own call and its own sample of the profile."""
    rng = random.Random(k)
    seg = _rand(rng, 300 + k)
    gfa = tmp_path / "one.gfa"
    gfa.write_text("S\t3\t%s\n" % seg)
    g = G.Graph.from_gfa(gfa.read_text(), k)
    ix = ctx.edgeindex_from_gfa(str(gfa), k)
    sub = lambda start, positions: seg[start:start + positions + k]  # a read with that many (k+1)-mer positions
    # one read whose single range ends before, at and after the end of a wave, of two waves, and of the block
    batches = [[sub(5, n)] for n in (62, 63, 64, 126, 127, 252, 253)]
    # the first read fills one wave (two waves): position 0 of the second read is lane 1 of the next wave, and lane 0
    # there holds the first read's last position, on the same edge at a smaller offset.  A new read opens a new range
    batches += [[sub(3, n), sub(3 + n + 20, 40)] for n in (63, 126)]
    # a read shorter than k + 1 has no position: its neighbours follow each other in the concatenation
    batches += [[sub(0, 80), seg[10:10 + k], sub(100, 70)]]
    for reads in batches:
        assert _check_ranges(ctx, ix, g, reads) == sum(len(r) > k for r in reads)  # one range per mapped read
    p = ix.profiles(len(batches))
    for i, reads in enumerate(batches):
        p.push(i, ctx.reads_from_ascii(reads))
    gr = R.Graph.from_gfa(gfa.read_text(), k)
    exp = np.array(R.segment_raw(gr, R.fill_literal(gr, batches)), dtype=np.uint64)
    assert list(exp[0]) == [62, 63, 64, 126, 127, 252, 253, 63 + 40, 126 + 40, 80 + 70]  # every position once
    assert np.array_equal(p.raw(), exp)


def _genome_graph(bins, tmp_path, seed=11, k=21):
    """a 20 kb genome with a repeat, 0.3 % substitutions in 4000 reads: spades-gbuilder --gfa -c"""
    rng = random.Random(seed)
    rep = _rand(rng, 80)
    genome = _rand(rng, 6000) + rep + _rand(rng, 7000) + rep + _rand(rng, 7000)
    reads = []
    for _ in range(4000):
        st = rng.randint(0, len(genome) - 150)
        s = _mutate(rng, genome[st:st + 150], 0.003, 0)
        reads.append(rc(s) if rng.random() < 0.5 else s)
    fa = tmp_path / "reads.fa"
    fa.write_text("".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(reads)))
    gfa = tmp_path / "g.gfa"
    r = subprocess.run([bins["spades-gbuilder"], str(fa), str(gfa), "-k", str(k), "--gfa", "-c"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    return rng, genome, gfa, gfa.read_text()


def _contigs(rng, genome, n):
    out = []
    for _ in range(n):
        ln = rng.randint(200, 3000)
        st = rng.randint(0, len(genome) - ln)
        c = list(_mutate(rng, genome[st:st + ln], 0.002, 0))
        if rng.random() < 0.3:
            p = rng.randint(0, len(c) - 10)
            c[p:p + 6] = "N" * rng.randint(1, 6)
        s = "".join(c)
        out.append(rc(s) if rng.random() < 0.5 else s)
    return out + out[:4] + [out[5].lower()]


def _yaml(path, libs):
    path.write_text("".join('- type: %s\n  single reads:\n    - "%s"\n' % (t, f) for t, f in libs))
    return path


def _fasta(path, seqs):
    path.write_text("".join(">c%d extra words\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    return path


def _run(bins, args):
    return subprocess.run([bins["spades-gmapper"]] + [str(a) for a in args], capture_output=True, text=True)


def test_b_c_d_cli_equals_restatement(bins, tmp_path):
    rng, genome, gfa, text = _genome_graph(bins, tmp_path)
    g = G.Graph.from_gfa(text, 21)
    assert len(g.names) > 20
    contigs = _contigs(rng, genome, 80)
    y = _yaml(tmp_path / "d.yaml", [("untrusted-contigs", _fasta(tmp_path / "c.fasta", contigs))])
    exp = G.gmapper(g, contigs)
    for extra in ([], ["-b", "3000", "-t", "3", "--tmp-dir", str(tmp_path / "tmp")]):
        out = tmp_path / "out.gfa"
        r = _run(bins, [y, gfa, out] + extra)
        assert r.returncode == 0, r.stderr
        got = out.read_text()
        assert got == exp
    assert gfa_canon.canon_text(got) == gfa_canon.canon_text(text)
    # (d) consecutive edges of a P line are linked in the GFA
    links = set()
    for line in got.splitlines():
        f = line.split("\t")
        if f[0] == "L":
            links.add((f[1] + f[2], f[3] + f[4]))
            links.add((f[3] + ("-" if f[4] == "+" else "+"), f[1] + ("-" if f[2] == "+" else "+")))
    p_lines = [line.split("\t") for line in got.splitlines() if line.startswith("P\t")]
    assert len(p_lines) > 20
    multi = 0
    for f in p_lines:
        items = f[2].split(",")
        multi += len(items) > 1
        for a, b in zip(items, items[1:]):
            assert (a, b) in links, (a, b)
    assert multi > 5
    # (c) every segment as a contig: one one-edge path of weight 1 per segment, in S-line order
    y2 = _yaml(tmp_path / "s.yaml", [("path-extend-contigs", _fasta(tmp_path / "segs.fasta", [g.seq[2 * i] for i in range(len(g.names))]))])
    out = tmp_path / "segs.gfa"
    r = _run(bins, [y2, gfa, out])
    assert r.returncode == 0, r.stderr
    assert [line for line in out.read_text().splitlines() if line.startswith("P\t")] == [
        "P\tPATH_%d_length_1_weigth_1_1\t%s+\t*\tZ:W:1" % (i + 1, n) for i, n in enumerate(g.names)]


def test_e_libraries_and_refusals(bins, tmp_path):
    rng, genome, gfa, text = _genome_graph(bins, tmp_path, seed=12)
    g = G.Graph.from_gfa(text, 21)
    first, second = _contigs(rng, genome, 10), _contigs(rng, genome, 12)
    fa1, fa2 = _fasta(tmp_path / "a.fasta", first), _fasta(tmp_path / "b.fasta", second)
    reads = tmp_path / "reads.fa"
    # the last contig library wins; other libraries are skipped
    y = _yaml(tmp_path / "d.yaml", [("untrusted-contigs", fa1), ("single", reads), ("path-extend-contigs", fa2),
                                      ("paired-end", reads)])
    out = tmp_path / "o.gfa"
    r = _run(bins, [y, gfa, out])
    assert r.returncode == 0, r.stderr
    assert out.read_text() == G.gmapper(g, second)
    assert "skipping the library" in r.stdout
    # no contig library: no file
    out2 = tmp_path / "none.gfa"
    r = _run(bins, [_yaml(tmp_path / "n.yaml", [("single", reads)]), gfa, out2])
    assert r.returncode == 0, r.stderr
    assert not out2.exists()
    # refusals
    bad = _fasta(tmp_path / "bad.fasta", [genome[:300], genome[400:500] + "R" + genome[500:600]])
    cases = [([("trusted-contigs", fa1)], gfa, "trusted"), ([("pacbio", fa1)], gfa, "long-read"),
             ([("untrusted-contigs", fa1)], tmp_path / "g.grseq", "GFA"), ([("untrusted-contigs", bad)], gfa, "c1")]
    for i, (libs, graph, word) in enumerate(cases):
        o = tmp_path / ("r%d.gfa" % i)
        r = _run(bins, [_yaml(tmp_path / ("r%d.yaml" % i), libs), graph, o])
        assert r.returncode > 0 and word in r.stderr, (word, r.stderr)
        assert not o.exists()


def test_engine_graph_export(ctx, tmp_path):
    text = "S\t3\t%s\tDP:f:1\tKC:i:7\nS\tx\t%s\nL\t3\t+\tx\t-\t21M\n" % ("A" * 21 + "C", rc("A" * 20 + "CG"))
    gfa = tmp_path / "t.gfa"
    gfa.write_text(text)
    names, seqs, links, kc = ctx.edgeindex_from_gfa(str(gfa), 21, keep_graph=True).graph()
    assert names == ["3", "x"] and seqs == ["A" * 21 + "C", rc("A" * 20 + "CG")]
    assert links == [(0, "+", 1, "-")] and list(kc) == [7, 0]
    with pytest.raises(B.BBKError, match="keeps no graph"):
        ctx.edgeindex_from_gfa(str(gfa), 21).graph()
