"""GPU: unitig-coverage (per-sample edge profiles) against the reference's own DP of the toy graph, against the KC of
the same graph (every read (k+1)-mer on the graph: raw == KC), and against the literal restatement of MapSequence /
EdgeProfileStorage (tests/unitig_profile_restated.py) on reads that leave the graph."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

import spades_for_blackbird_amd as B
from spades_for_blackbird_amd import build, build_host
from tests import unitig_profile_restated as R
from tests.helpers import rc, read_fastq_gz, synth_reads

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


def _gbuilder_gfa(bins, src, out, k=21):
    r = subprocess.run([bins["spades-gbuilder"], str(src), str(out), "-k", str(k), "--gfa"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return open(out).read()


def _run(bins, args):
    return subprocess.run([bins["unitig-coverage"]] + [str(a) for a in args], capture_output=True, text=True)


def test_toy_dp_of_the_reference(bins, golden, golden_dir, tmp_path):
    """(a) every read (k+1)-mer lies on the graph built from the same reads: the printed value is the GFA's DP:f:"""
    g = golden["toy_gbuilder"]["k21"]
    fq = os.path.join(golden_dir, "ecoli_1K_1.fq.gz")
    gfa = tmp_path / "g.gfa"
    _gbuilder_gfa(bins, fq, gfa)
    y = tmp_path / "d.yaml"
    y.write_text('- type: single\n  single reads:\n    - "%s"\n' % fq)
    out = tmp_path / "prof.tsv"
    r = _run(bins, [y, gfa, out, "-k", "21"])
    assert r.returncode == 0, r.stderr
    seqs = {n: s for n, s in zip(*R.parse_gfa(gfa.read_text())[:2])}
    dp_by_len = dict(zip(g["unitig_lengths"], g["DP"]))
    assert len(dp_by_len) == 5
    lines = out.read_text().split("\n")
    assert lines[-1] == "" and len(lines) - 1 == len(seqs) == 5
    for line in lines[:-1]:
        name, val, tail = line.split("\t")
        assert tail == ""
        assert val == dp_by_len[len(seqs[name])], (name, val)


@pytest.mark.parametrize("k,n_reads,read_len", [(21, 1_000_000, 150), (31, 20000, 150), (33, 20000, 150),
                                                (55, 20000, 150), (125, 20000, 250)])
def test_raw_equals_kc(ctx, k, n_reads, read_len):
    """(b) raw == KC of bbk_unitigs_add_coverage on the graph of the same reads.  One known difference: a palindromic
    (k+1)-mer (the middle of a self-conjugate segment) is in a read and in its reverse complement, and MapSequence maps
    both (2 per occurrence), where the count behind KC takes each read position once (1 per occurrence)."""
    genome = max(5000, n_reads * read_len // 60)
    r = ctx.reads_synth(n_reads, read_len=read_len, genome_len=genome, seed_genome=k, seed_reads=k + 1)
    u = ctx.unitigs(ctx.extindex(r, k))
    u.add_coverage(r)
    kc = u.kc()
    ix = ctx.edgeindex_from_unitigs(u)
    assert ix.segments == len(u)
    p = ix.profiles(1)
    p.push(0, r)
    raw = p.raw()
    assert raw.shape == (len(u), 1)
    diff = np.nonzero(raw[:, 0] != kc)[0]
    if len(diff):
        seqs = u.sequences()
        reads = "|".join(r.to_list())
        for i in diff:
            s = seqs[i]
            assert s == rc(s), (i, s, int(raw[i, 0]), int(kc[i]))
            mid = s[(len(s) - k - 1) // 2:][:k + 1]
            assert mid == rc(mid)
            occ = len(re.findall("(?=%s)" % mid, reads))
            assert int(raw[i, 0]) == int(kc[i]) + occ, (i, s, int(raw[i, 0]), int(kc[i]), occ)


def test_k127_equals_restatement(ctx, tmp_path):
    """(b) k = 127 (128-mers, four words): the engine builds graphs up to k = 125 only, so this one is a GFA
    written here (a random sequence cut into four segments that overlap by k), against the restatement"""
    k = 127
    rng = random.Random(127)
    genome = "".join(rng.choice("ACGT") for _ in range(3000))
    cuts = [0, 700, 1500, 2200, 3000]
    segs = [genome[max(0, a - k):b] for a, b in zip(cuts, cuts[1:])]
    gfa = tmp_path / "g127.gfa"
    gfa.write_text("".join("S\t%d\t%s\n" % (3 + 2 * i, q) for i, q in enumerate(segs)) +
                   "".join("L\t%d\t+\t%d\t+\t%dM\n" % (3 + 2 * i, 5 + 2 * i, k) for i in range(len(segs) - 1)))
    reads = []
    for _ in range(600):
        st = rng.randint(0, len(genome) - 300)
        r = list(genome[st:st + rng.randint(100, 300)])
        for j in range(len(r)):
            if rng.random() < 0.003:
                r[j] = rng.choice("ACGTN")
        r = "".join(r)
        reads.append(rc(r) if rng.random() < 0.5 else r)
    ix = ctx.edgeindex_from_gfa(str(gfa), k)
    assert ix.segments == 4 and len(ix) == sum(len(q) - k for q in segs)
    p = ix.profiles(1)
    p.push(0, ctx.reads_from_ascii(reads))
    g = R.Graph.from_gfa(gfa.read_text(), k)
    lit = R.fill_literal(g, [reads])
    assert np.array_equal(p.raw(), np.array(R.segment_raw(g, lit), dtype=np.uint64))
    out = tmp_path / "p.tsv"
    p.write(str(out))
    assert out.read_text() == R.save(g, lit)


def test_three_samples_equal_restatement(ctx, tmp_path):
    """(c) three samples, one of them mostly off the graph (errors and Ns): raw() and the file equal the restatement"""
    k = 21
    base = ctx.reads_synth(1500, read_len=150, genome_len=20000, seed_genome=5, seed_reads=6)
    u = ctx.unitigs(ctx.extindex(base, k))
    gfa = tmp_path / "g.gfa"
    u.write_gfa(str(gfa))
    other = ctx.reads_synth(1200, read_len=150, genome_len=20000, seed_genome=5, seed_reads=7)
    mutated = synth_reads(800, read_len=120, genome_len=20000, sub_rate=0.03, seed=9, n_rate=0.002)
    samples = [base.to_list(), other.to_list(), mutated]
    g = R.Graph.from_gfa(gfa.read_text(), k)
    lit = R.fill_literal(g, samples)
    exp_raw = np.array(R.segment_raw(g, lit), dtype=np.uint64)
    exp_text = R.save(g, lit)
    for ix in (ctx.edgeindex_from_unitigs(u), ctx.edgeindex_from_gfa(str(gfa), k)):
        p = ix.profiles(3)
        p.push(0, base)
        p.push(1, other)
        # a sample in two batches: the profile accumulates
        p.push(2, ctx.reads_from_ascii(mutated[:300]))
        p.push(2, ctx.reads_from_ascii(mutated[300:]))
        assert np.array_equal(p.raw(), exp_raw)
        out = tmp_path / "p.tsv"
        p.write(str(out))
        assert out.read_text() == exp_text
    assert exp_raw[:, 2].sum() < exp_raw[:, 1].sum()  # the mutated sample is not all on the graph


def test_cli_paired_gz_and_fasta_libraries(bins, golden_dir, tmp_path):
    """(d) a paired gz library and a FASTA single library: two samples, equal to the restatement byte for byte"""
    k = 21
    f1, f2 = os.path.join(golden_dir, "ecoli_1K_1.fq.gz"), os.path.join(golden_dir, "ecoli_1K_2.fq.gz")
    gfa = tmp_path / "g.gfa"
    text = _gbuilder_gfa(bins, f1, gfa)
    left, right = read_fastq_gz(f1), read_fastq_gz(f2)
    single = synth_reads(300, read_len=100, genome_len=3000, seed=3, n_rate=0.01) + [left[0][5:90], right[1][:60]]
    fa = tmp_path / "s.fasta"
    fa.write_text("".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(single)))
    y = tmp_path / "d.yaml"
    y.write_text('- type: paired-end\n  orientation: fr\n  left reads:\n    - "%s"\n  right reads:\n    - "%s"\n'
                 '- type: single\n  single reads:\n    - "%s"\n' % (f1, f2, fa))
    g = R.Graph.from_gfa(text, k)
    exp = R.save(g, R.fill_literal(g, [left + right, single]))
    for extra in ([], ["-b", "20000", "-t", "2", "--tmpdir", str(tmp_path / "tmp")]):
        out = tmp_path / "prof.tsv"
        r = _run(bins, [y, gfa, out] + extra)
        assert r.returncode == 0, r.stderr
        assert out.read_text() == exp


def test_cli_refusals(bins, golden_dir, tmp_path):
    """(e) a wrong overlap, a duplicated (k+1)-mer, an even k and a graph that is not GFA: exit != 0 with a message"""
    fq = os.path.join(golden_dir, "ecoli_1K_1.fq.gz")
    gfa = tmp_path / "g.gfa"
    text = _gbuilder_gfa(bins, fq, gfa)
    y = tmp_path / "d.yaml"
    y.write_text('- type: single\n  single reads:\n    - "%s"\n' % fq)
    bad_ovl = tmp_path / "ovl.gfa"
    bad_ovl.write_text(text.replace("\t21M", "\t20M"))
    assert "\t21M" in text
    names, seqs, _ = R.parse_gfa(text)
    dup = tmp_path / "dup.gfa"
    dup.write_text(text + "S\t999\t%s\tDP:f:0\n" % seqs[0][:40])
    notgfa = tmp_path / "g.grseq"
    notgfa.write_text(text)
    cases = [([y, bad_ovl, tmp_path / "o1"], "overlap"), ([y, dup, tmp_path / "o2"], "duplicated"),
             ([y, gfa, tmp_path / "o3", "-k", "20"], "odd"), ([y, notgfa, tmp_path / "o4"], "GFA")]
    for args, word in cases:
        r = _run(bins, args)
        assert r.returncode != 0 and r.returncode > 0, (args, r.returncode)  # an exit, not a signal
        assert word in r.stderr, (word, r.stderr)
    with pytest.raises(B.BBKError, match="overlap"):
        B.Context(0).edgeindex_from_gfa(str(bad_ovl), 21)
