"""GPU parity tests of the extension index, unitig extraction and GFA output (through the C ABI)
against the CPU oracle and the reference's golden vectors.  Bit-exact on the canonical form."""
import hashlib
import os

import numpy as np
import pytest

import spades_for_blackbird_amd as B
from oracle import oracle as O
from spades_for_blackbird_amd.tools import gfa_canon
from tests.helpers import expected_gfa, gfa_bytes, gpu_gfa, rc, read_fastq_gz, synth_reads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = B.Context(0)
    yield c
    c.close()


def oracle_table(reads, k):
    x = O.ExtIndex(reads, k, 1)
    keys, masks = x.kmers, x.masks
    order = np.lexsort([keys[:, j] for j in range(keys.shape[1] - 1, -1, -1)])
    return keys[order], masks[order]


@pytest.mark.parametrize("k", [3, 5, 9, 21, 31, 33, 55, 63, 65, 99])
def test_extindex_vs_oracle(ctx, k):
    reads = synth_reads(300, read_len=120, genome_len=2500, sub_rate=0.01, seed=100 + k, n_rate=0.003)
    reads += ["", "ACGT", "A" * k, "ACGTTGCATT" * 13, "acgtn" * 30]
    ek, em = oracle_table(reads, k)
    x = ctx.extindex(ctx.reads_from_ascii(reads), k)
    gk, gm = x.export()
    assert gk.shape == ek.shape
    assert np.array_equal(gk, ek)
    assert np.array_equal(gm, em)


def test_extindex_toy(ctx, golden, golden_dir):
    g = golden["toy_gbuilder"]
    reads = read_fastq_gz(os.path.join(golden_dir, g["file"]))
    for k, key in ((21, "k21"), (55, "k55")):
        x = ctx.extindex(ctx.reads_from_ascii(reads), k)
        assert len(x) == g[key]["n_k"]
        ek, em = oracle_table(reads, k)
        gk, gm = x.export()
        assert np.array_equal(gk, ek) and np.array_equal(gm, em)


def test_toy_gfa(ctx, golden, golden_dir, tmp_path):
    g = golden["toy_gbuilder"]
    reads = read_fastq_gz(os.path.join(golden_dir, g["file"]))
    txt, u = gpu_gfa(ctx, reads, 21, tmp_path)
    assert len(u) == g["k21"]["n_unitigs"] and u.n_loops == 0
    assert (u.n_vertices, u.n_links) == (g["k21"]["n_vertices"], g["k21"]["n_links"])
    assert sorted(len(s) for s in u.sequences()) == sorted(g["k21"]["unitig_lengths"])
    S = sorted(l.split("\t")[2] for l in txt.splitlines() if l.startswith("S"))
    assert hashlib.md5(("\n".join(S) + "\n").encode()).hexdigest() == g["k21"]["sorted_S_sequences_md5"]
    exp = O.ExtIndex(reads, 21, 1).unitigs().gfa()[0]
    assert gfa_canon.canon_md5(txt) == gfa_canon.canon_md5(exp)
    txt55, u55 = gpu_gfa(ctx, reads, 55, tmp_path, "g55.gfa")
    assert (len(u55), u55.n_vertices) == (g["k55"]["n_unitigs"], g["k55"]["n_vertices"])
    exp55 = O.ExtIndex(reads, 55, 1).unitigs().gfa()[0]
    assert gfa_canon.canon_md5(txt55) == gfa_canon.canon_md5(exp55)


def test_construction_kats(ctx, golden, tmp_path):
    g = golden["construction_unitigs_k5"]
    for c in g["cases"]:
        txt, u = gpu_gfa(ctx, c["reads"], g["k"], tmp_path)
        got = set(u.sequences())
        got |= set(rc(s) for s in got)
        exp = set(c["edges"]) | set(rc(s) for s in c["edges"])
        assert got == exp, c["name"]
        for s in u.sequences():
            assert not (s < rc(s))


def test_loop_and_self_rc_goldens(ctx, golden, tmp_path):
    for name in ("loop_k5", "self_rc_edge_k5", "split_loop_k5"):
        g = golden[name]
        txt, u = gpu_gfa(ctx, g["reads"], g["k"], tmp_path)
        ou = O.ExtIndex(g["reads"], g["k"], 1).unitigs()
        exp = ou.gfa()[0]
        assert (len(u), u.n_loops) == (ou.n, ou.n_loops), name
        if name == "split_loop_k5":
            # which palindrome is split off depends on the start k-mer: compare invariants
            seqs = u.sequences()
            assert sorted(len(s) for s in seqs) == sorted(len(s) for s in g["S"])
            assert any(s == rc(s) and len(s) == g["k"] + 1 for s in seqs)
            assert u.n_links == 1
        else:
            assert gfa_canon.canon_text(txt) == gfa_canon.canon_text(exp), name
    g = golden["self_rc_edge_k5"]
    txt, u = gpu_gfa(ctx, g["reads"], g["k"], tmp_path)
    assert sorted(u.sequences()) == sorted(g["S"])


def test_loops_in_reference_file_order(ctx, golden, tmp_path):
    """End-to-end pin of CollectLoops / SplitLoop (debruijn_graph_constructor.hpp:248-265,308-344): with
    bbk_unitigs_build_ex(ref_threads = T) the engine visits the leftover k-mers in the k-mer file order of a reference
    run with -t T (10 T XXH3 buckets, ascending inside), like the oracle (which reproduces the recorded reference
    output of the SplitLoop golden string for string, tests/test_oracle_golden.py::test_split_loop_golden): the loop
    strings -- where they start, and which palindromic (k+1)-mer a self-conjugate circle is cut at -- are then EQUAL,
    not only equal modulo rotation."""
    cases = [golden["split_loop_k5"]["reads"], golden["loop_k5"]["reads"],
             ["TTTCCTCATGCAATATTGCATGAGGAAA" + "TTTCCTCATGCAAT", "CTTGCTGTGTCCACCCCATCGGAC" * 2, "GGATTACAGGCATGAGCCACC" * 2]]
    seen_loops = 0
    for reads in cases:
        for T in (1, 2, 5):
            r = ctx.reads_from_ascii(reads)
            u = ctx.unitigs(ctx.extindex(r, 5), ref_threads=T)
            ou = O.ExtIndex(reads, 5, T).unitigs()
            got, exp = u.sequences(), ou.seqs
            assert u.n_loops == ou.n_loops
            seen_loops += u.n_loops
            nl = u.n_loops
            assert got[len(got) - nl:] == exp[len(exp) - nl:], (reads, T)      # the loop strings, in order
            assert sorted(got[:len(got) - nl]) == sorted(exp[:len(exp) - nl])  # the paths (their order differs by design)
    assert seen_loops >= 9
    g = golden["split_loop_k5"]
    u = ctx.unitigs(ctx.extindex(ctx.reads_from_ascii(g["reads"]), g["k"]), ref_threads=1)
    assert u.sequences() == g["S"]  # the recorded reference output itself


@pytest.mark.parametrize("k,seed", [(5, 1), (9, 2), (21, 3), (21, 4), (33, 5), (55, 6), (77, 7)])
def test_gfa_vs_oracle_synthetic(ctx, k, seed, tmp_path):
    reads = synth_reads(1500, read_len=100, genome_len=4000 if k > 9 else 600, sub_rate=0.01, seed=seed,
                        n_rate=0.001)
    txt, u = gpu_gfa(ctx, reads, k, tmp_path)
    ox = O.ExtIndex(reads, k, 2)
    ou = ox.unitigs()
    exp, nv, nl = ou.gfa()
    assert (len(u), u.n_loops, u.n_vertices, u.n_links) == (ou.n, ou.n_loops, nv, nl)
    # loops are compared modulo rotation / reverse complement through the canonical form; the one thing
    # it cannot normalise is WHICH palindromic (k+1)-mer SplitLoop cuts a self-conjugate circle at (order-dependent
    # in the reference itself): only then the comparison falls back to segment lengths + counts
    segs = [l.split("\t")[2] for l in exp.splitlines() if l.startswith("S")]
    loops = segs[len(segs) - ou.n_loops:] if ou.n_loops else []
    split = any(s[i:i + k + 1] == rc(s[i:i + k + 1]) for s in loops for i in range(len(s) - k))
    if not split:
        assert gfa_canon.canon_text(txt) == gfa_canon.canon_text(exp)
    else:
        gs, gl = gfa_canon.canon(txt)
        es, el = gfa_canon.canon(exp)
        assert sorted(len(s[0]) for s in gs) == sorted(len(s[0]) for s in es)


def six_circles():
    rng = np.random.default_rng(9)
    reads = []
    for c in range(6):
        circ = "".join("ACGT"[i] for i in rng.integers(0, 4, size=200 + 17 * c))
        dbl = circ + circ
        for s in range(0, len(circ), 7):
            reads.append(dbl[s:s + 60])
    return reads


def test_circular_genomes_loops(ctx, tmp_path):
    """Several perfect loops at once (plasmid-like circles without junctions)."""
    reads = six_circles()
    k = 21
    txt, u = gpu_gfa(ctx, reads, k, tmp_path)
    ou = O.ExtIndex(reads, k, 1).unitigs()
    assert (len(u), u.n_loops) == (ou.n, ou.n_loops)
    assert u.n_loops == 6
    assert gfa_canon.canon_md5(txt) == gfa_canon.canon_md5(ou.gfa()[0])


def test_fasta_and_links_export(ctx, tmp_path):
    reads = synth_reads(200, read_len=80, genome_len=1500, sub_rate=0.01, seed=8)
    r = ctx.reads_from_ascii(reads)
    u = ctx.unitigs(ctx.extindex(r, 21))
    p = str(tmp_path / "u.fa")
    u.write_fasta(p)
    seqs = u.sequences()
    exp = ""
    for i, s in enumerate(seqs):
        exp += ">EDGE_%d_length_%d\n" % (i + 1, len(s))
        exp += "".join(s[j:j + 60] + "\n" for j in range(0, len(s), 60))
    assert open(p).read() == exp
    links = u.links()
    assert links.shape == (u.n_links, 4)
    k = 21
    for a, oa, b, ob in links[:200]:
        sa = seqs[a] if oa else rc(seqs[a])
        sb = seqs[b] if ob else rc(seqs[b])
        assert sa[-k:] == sb[:k]


def test_even_k_rejected(ctx):
    r = ctx.reads_from_ascii(["ACGTACGTTGCA"])
    x = ctx.extindex(r, 4)
    with pytest.raises(B.BBKError):
        ctx.unitigs(x)


def test_coverage_toy_golden(ctx, golden, golden_dir, tmp_path):
    """gbuilder -c on the bundled toy data: KC and DP of the reference run."""
    g = golden["toy_gbuilder"]
    reads = read_fastq_gz(os.path.join(golden_dir, g["file"]))
    r = ctx.reads_from_ascii(reads)
    u = ctx.unitigs(ctx.extindex(r, 21))
    u.add_coverage(r)
    assert sorted(int(x) for x in u.kc()) == sorted(g["k21"]["KC"])
    p = str(tmp_path / "c.gfa")
    u.write_gfa(p)
    txt = open(p).read()
    dp = sorted(l.split("\t")[3][5:] for l in txt.splitlines() if l.startswith("S"))
    assert dp == sorted(g["k21"]["DP"])
    exp = O.ExtIndex(reads, 21, 1).unitigs().gfa(with_cov=True)[0]
    assert gfa_canon.canon_md5(txt, with_kc=True) == gfa_canon.canon_md5(exp, with_kc=True)
    by_seq = {l.split("\t")[2]: l.split("\t", 3)[3] for l in txt.splitlines() if l.startswith("S")}
    exp_by_seq = {l.split("\t")[2]: l.split("\t", 3)[3] for l in exp.splitlines() if l.startswith("S")}
    assert by_seq == exp_by_seq  # identical DP:f / KC:i text per segment


def test_coverage_kat_and_synthetic(ctx, golden, tmp_path):
    g = golden["construction_coverage_k3"]
    r = ctx.reads_from_ascii(g["reads"])
    u = ctx.unitigs(ctx.extindex(r, g["k"]))
    u.add_coverage(r)
    got = {}
    for s, kc in zip(u.sequences(), u.kc()):
        got[s] = int(kc)
        got[rc(s)] = int(kc)
    for e, cov in g["coverage"].items():
        assert got[e] == cov
    for k, seed in ((21, 31), (33, 32), (55, 33)):
        reads = synth_reads(800, read_len=100, genome_len=3000, sub_rate=0.01, seed=seed, n_rate=0.001)
        r = ctx.reads_from_ascii(reads)
        u = ctx.unitigs(ctx.extindex(r, k))
        u.add_coverage(r)
        p = str(tmp_path / ("c%d.gfa" % k))
        u.write_gfa(p)
        exp = O.ExtIndex(reads, k, 2).unitigs().gfa(with_cov=True)[0]
        assert gfa_canon.canon_md5(open(p).read(), with_kc=True) == gfa_canon.canon_md5(exp, with_kc=True)


def test_fastg_structure(ctx, tmp_path):
    """FASTG (gbuilder --fastg): no reference fixture ships for it ("parity unpinned" for the exact
    text); checked structurally against the GFA of the same graph: every edge and its conjugate once,
    successor lists = the link set closed under reverse complement, names per BasicNamingF."""
    reads = synth_reads(600, read_len=100, genome_len=2500, sub_rate=0.01, seed=77)
    k = 21
    r = ctx.reads_from_ascii(reads)
    u = ctx.unitigs(ctx.extindex(r, k))
    p = str(tmp_path / "g.fastg")
    u.write_fastg(p)
    seqs = u.sequences()
    recs = {}
    name = None
    for line in open(p):
        line = line.rstrip("\n")
        if line.startswith(">"):
            assert line.endswith(";")
            head = line[1:-1]
            name, _, succ = head.partition(":")
            recs[name] = [succ.split(",") if succ else [], ""]
        else:
            recs[name][1] += line
    n_self = sum(1 for s in seqs if s == rc(s))
    assert len(recs) == 2 * len(seqs) - n_self

    def nm(i, plus):
        return "EDGE_%d_length_%d_cov_0.000000%s" % (3 + 2 * i, len(seqs[i]), "" if plus else "'")
    for i, s in enumerate(seqs):
        assert recs[nm(i, True)][1] == s
        if s != rc(s):
            assert recs[nm(i, False)][1] == rc(s)
    exp = set()
    for a, oa, b, ob in u.links():
        exp.add((nm(a, oa), nm(b, ob)))
        fa = oa if seqs[a] == rc(seqs[a]) else 1 - oa
        fb = ob if seqs[b] == rc(seqs[b]) else 1 - ob
        exp.add((nm(b, fb), nm(a, fa)))
    got = set((x, y) for x, (succ, _) in recs.items() for y in succ)
    assert got == exp
    for x, y in got:
        assert recs[x][1][-k:] == recs[y][1][:k]
    for x, (succ, _) in recs.items():
        assert succ == sorted(succ)


def test_long_reads_and_long_unitigs(ctx, tmp_path):
    """Contig-sized input records (one partition tile lies inside a single read) and an error-free genome
    (unitigs of thousands of k-mers walked by single threads)."""
    rng = np.random.default_rng(23)
    genome = "".join("ACGT"[i] for i in rng.integers(0, 4, size=60000))
    reads = [genome[:40000], genome[30000:], rc(genome[10000:35000]), "N" * 10 + genome[5000:5100]]
    k = 31
    txt, u = gpu_gfa(ctx, reads, k, tmp_path)
    ou = O.ExtIndex(reads, k, 1).unitigs()
    assert (len(u), u.n_loops) == (ou.n, ou.n_loops)
    assert max(len(s) for s in u.sequences()) > 10000
    assert gfa_canon.canon_md5(txt, k) == gfa_canon.canon_md5(ou.gfa()[0], k)  # an error-free genome has no links
    r = ctx.reads_from_ascii(reads)
    got = ctx.count(r, k, B.BOTH_STRANDS).export(B.ORDER_REFERENCE_BUCKETS16)
    assert np.array_equal(got, O.kmercount(reads, k, 16, 2))


@pytest.mark.parametrize("k,bound", [(21, 129), (21, 10), (33, 117), (55, 95), (77, 20)])
def test_early_tip_clipping(ctx, k, bound):
    """bbk_extindex_clip_tips vs the oracle's restatement of EarlyTipClipperProcessor::ClipTips
    (early_simplification.hpp:37-160): same isolated k-mers, same removed links, identical masks afterwards, and the
    unitigs of the clipped index agree in canonical form.  Sequencing errors near read ends give thousands of tips.
    No reference fixture exists for this step ("parity unpinned": the oracle is the restated algorithm)."""
    reads = synth_reads(2500, read_len=150, genome_len=20000, sub_rate=0.01, seed=31 + k, n_rate=0.001)
    reads += ["ACGT" * 40, "A" * 150]
    ox = O.ExtIndex(reads, k, 1)
    exp_removed, exp_links = ox.clip_tips(bound)
    assert exp_removed > 0
    x = ctx.extindex(ctx.reads_from_ascii(reads), k)
    removed, links = x.clip_tips(bound)
    assert (removed, links) == (exp_removed, exp_links)
    order = np.lexsort([ox.kmers[:, j] for j in range(ox.kmers.shape[1] - 1, -1, -1)])
    gk, gm = x.export()
    assert np.array_equal(gk, ox.kmers[order])
    assert np.array_equal(gm, ox.masks[order])
    # the clipped index still compacts: same unitig multiset as the oracle (orientation-free)
    u = ctx.unitigs(x)
    ou = ox.unitigs()
    got = sorted(min(s, rc(s)) for s in u.sequences())
    exp = sorted(min(s, rc(s)) for s in ou.seqs)
    assert got == exp
    # idempotent on an index without short tips left: a second pass with the same bound removes nothing new only
    # if no new tips arose; the reference makes no such promise, so just check it runs and stays consistent
    removed2, links2 = x.clip_tips(bound)
    assert removed2 >= 0 and links2 >= 0


@pytest.mark.parametrize("k,n_reads", [(21, 10_000_000), (55, 4_000_000), (77, 2_000_000)])
def test_full_size_graph_properties(k, n_reads):
    """The gbuilder path at the full configs[1] size (10 M x 150 bp, k=21; 16- and 24-byte keys at 4 M / 2 M reads)
    through size-independent properties:
    the extension index holds exactly the canonical k-mers of the reads; the unitigs partition the (k+1)-mer set --
    sum(len - k) over the kept unitigs equals the number of canonical (k+1)-mer classes, plus the classes that a
    self-reverse-complementary unitig (one around each palindromic (k+1)-mer) covers twice, a handful at this size;
    coverage: the KC values add up to the (k+1)-mer instance count (every instance lies on exactly one unitig edge,
    self-conjugate unitigs aside)."""
    import torch
    ctx = B.Context(0, stream=torch.cuda.current_stream())
    L = 150
    r = ctx.reads_synth(n_reads, read_len=L, genome_len=n_reads * L // 50, seed_genome=42, seed_reads=43)
    x = ctx.extindex(r, k)
    canon_k = ctx.count(r, k, B.CANONICAL | B.UNSORTED)
    assert len(x) == len(canon_k)                      # every read is longer than k: each k-mer has an edge
    canon_k1 = ctx.count(r, k + 1, B.CANONICAL | B.WITH_COUNTS)
    u = ctx.unitigs(x)
    assert u.n_loops == 0 or u.n_loops < 10
    edges = u.total_bases - len(u) * k                 # sum(len - k)
    extra = edges - len(canon_k1)
    assert 0 <= extra < 1e-5 * len(canon_k1), (edges, len(canon_k1))
    assert u.n_vertices > 0 and u.n_links > 0 and u.n_links < 8 * len(u)
    u.add_coverage(r)
    kc = np.asarray(u.kc(), dtype=np.uint64)
    inst = n_reads * (L - k)                           # (k+1)-mer instances of the reads
    total = int(kc.sum())
    assert inst <= total < inst * (1 + 1e-5)           # self-conjugate unitigs count their instances on both strands
    ctx.close()


def _load_grseq(path):
    """io::binary::GraphIO::LoadImpl (common/io/binary/graph.hpp:48-96) restated: returns (vertices {id: conj id},
    edges {id: (conj id, start vertex, end vertex, sequence)})."""
    import struct
    data = open(path, "rb").read()
    pos = 0

    def u64():
        nonlocal pos
        v = struct.unpack_from("<Q", data, pos)[0]
        pos += 8
        return v
    vres, eres, nvert = u64(), u64(), u64()
    verts, edges = {}, {}
    for _ in range(nvert):
        v, cv = u64(), u64()
        verts[v] = cv
        while True:
            e1 = u64()
            if e1 == 0:
                break
            e2, end1, start2, size = u64(), u64(), u64(), u64()
            nw = (size + 31) // 32
            words = struct.unpack_from("<%dQ" % nw, data, pos)
            pos += 8 * nw
            seq = "".join("ACGT"[(words[i >> 5] >> ((i & 31) << 1)) & 3] for i in range(size))
            edges[e1] = (e2, v, end1, seq)
            assert verts.get(v) == cv and start2 < vres and end1 < vres and e1 < eres and e2 < eres
    assert pos == len(data)
    return verts, edges


@pytest.mark.parametrize("k,seed", [(21, 3), (33, 5), (5, 1)])
def test_spades_binary_graph(ctx, k, seed, tmp_path):
    """gbuilder --spades: <out>.grseq + <out>.cvr.  No reference file exists to compare bytes with and the reference's
    vertex numbering follows BooPHF indices ("parity unpinned"): the file is read back the way the reference's loader
    reads it and the graph it describes must be the graph of the GFA -- same edges under the same ids, a vertex per
    oriented junction k-mer, the same links, the same coverage."""
    import struct
    reads = synth_reads(1500, read_len=100, genome_len=4000 if k > 9 else 600, sub_rate=0.01, seed=seed)
    r = ctx.reads_from_ascii(reads)
    x = ctx.extindex(r, k)
    u = ctx.unitigs(x)
    u.add_coverage(r)
    base = str(tmp_path / "g")
    u.write_spades(base)
    verts, edges = _load_grseq(base + ".grseq")
    seqs = u.sequences()
    assert sorted(edges) == [3 + 2 * i for i in range(len(seqs))]
    vk = {}  # vertex id -> oriented k-mer

    def bind(v, kmer):
        assert vk.setdefault(v, kmer) == kmer, "vertex %d stands for two k-mers" % v
    for i, s in enumerate(seqs):
        e2, vs, ve, seq = edges[3 + 2 * i]
        assert seq == s
        assert e2 == (3 + 2 * i if s == rc(s) else 3 + 2 * i + 1)
        bind(vs, s[:k])
        bind(ve, s[-k:])
        bind(verts[vs], rc(s[:k]))
        bind(verts[ve], rc(s[-k:]))
    assert len(set(vk.values())) == len(vk)                       # one vertex per oriented k-mer
    assert all(verts[verts[v]] == v and verts[v] != v for v in verts)
    assert len(verts) == 2 * u.n_vertices and set(vk) == set(verts)
    # the graph the file describes, written the way GFAWriter::WriteSegmentsAndLinks walks a graph
    # (io/graph/gfa_writer.cpp:35-52: for every canonical vertex, every incoming x outgoing oriented edge; '+' iff the
    # oriented edge is the canonical one), must be the GFA of the same unitigs in canonical form
    conj_e = {}
    start_of, end_of = {}, {}
    for e1, (e2, vs, ve, seq) in edges.items():
        conj_e[e1], conj_e[e2] = e2, e1
        start_of[e1], end_of[e1] = vs, ve
        start_of[e2], end_of[e2] = verts[ve], verts[vs]
    out_e, in_e = {}, {}
    for e in start_of:
        out_e.setdefault(start_of[e], []).append(e)
        in_e.setdefault(end_of[e], []).append(e)
    lines = ["S\t%d\t%s\tDP:f:0\tKC:i:0" % (3 + 2 * i, sq) for i, sq in enumerate(seqs)]
    for v in sorted(verts):
        if v > verts[v]:
            continue
        for a in sorted(in_e.get(v, [])):
            for b in sorted(out_e.get(v, [])):
                lines.append("L\t%d\t%s\t%d\t%s\t%dM" % (min(a, conj_e[a]), "+" if a <= conj_e[a] else "-",
                                                          min(b, conj_e[b]), "+" if b <= conj_e[b] else "-", k))
    gfa_path = str(tmp_path / "g.gfa")
    u.write_gfa(gfa_path)
    assert gfa_canon.canon_text("\n".join(lines) + "\n", k) == gfa_canon.canon_text(open(gfa_path).read(), k)
    # coverage file: (edge id, raw coverage) per canonical edge, zero-terminated
    cv = open(base + ".cvr", "rb").read()
    kc = u.kc()
    assert len(cv) == 12 * len(seqs) + 8
    for i in range(len(seqs)):
        e, c = struct.unpack_from("<QI", cv, 12 * i)
        assert e == 3 + 2 * i and c == kc[i]
    assert struct.unpack_from("<Q", cv, 12 * len(seqs))[0] == 0


# ---- 64-bit graph stage ------------------------------------------------------------------------------------------
# KMerIndex::seq_idx is a size_t (utils/kmer_mph/kmer_index.hpp:85-90) and LinkRecord keys are 64-bit
# (debruijn_graph_constructor.hpp:400-430).  Here the prefix table takes 64-bit entries from 2^32-2 k-mers on;
# BBK_WIDE_INDEX=1 forces them, so that the same code path the >2^32 test (tests/test_gpu_graph64.py) runs is compared
# with the oracle bit for bit at sizes the oracle can do.
@pytest.mark.parametrize("k", [5, 21, 33, 65])
def test_wide_index_gfa_vs_oracle(ctx, monkeypatch, tmp_path, k):
    reads = synth_reads(400, read_len=130, genome_len=3000, sub_rate=0.01, seed=900 + k, n_rate=0.002)
    reads += ["ACGGTCATTGCAGGATCCTA" * 2, "CTTGCTGTGTCCACCCCATCGGAC" * 2]  # a self-conjugate edge, a perfect loop at k = 5
    r = ctx.reads_from_ascii(reads)

    def build(name):
        x = ctx.extindex(r, k)
        u = ctx.unitigs(x)
        p = str(tmp_path / (name + ".gfa"))
        u.write_gfa(p)
        plain = open(p).read()
        u.add_coverage(r)  # KC through the lookup of the (k+1)-mer table
        u.write_gfa(p)
        return plain, open(p).read(), (len(u), u.n_loops, u.n_vertices, u.n_links)
    narrow = build("narrow")
    monkeypatch.setenv("BBK_WIDE_INDEX", "1")
    wide = build("wide")
    assert wide == narrow  # byte for byte: the entry width of the prefix table changes nothing
    exp_txt = O.ExtIndex(reads, k, 1).unitigs().gfa()[0]
    assert gfa_canon.canon_md5(wide[0], k) == gfa_canon.canon_md5(exp_txt, k)


def test_wide_index_tip_clipping_same_as_narrow(ctx, monkeypatch):
    reads = synth_reads(600, read_len=120, genome_len=4000, sub_rate=0.01, seed=77)
    r = ctx.reads_from_ascii(reads)
    x0 = ctx.extindex(r, 21)
    rm0 = x0.clip_tips(42)
    k0, m0 = x0.export()
    monkeypatch.setenv("BBK_WIDE_INDEX", "1")
    x1 = ctx.extindex(r, 21)
    rm1 = x1.clip_tips(42)
    k1, m1 = x1.export()
    assert rm0 == rm1 and np.array_equal(k0, k1) and np.array_equal(m0, m1)


def test_unitigs_to_reads_and_graph_invariants(ctx, tmp_path):
    """The size-independent properties tests/test_gpu_graph64.py relies on, checked where the oracle can confirm them:
    the canonical (k+1)-mers spelled by the segments are pairwise distinct and are exactly the (k+1)-mers of the reads
    (SURVEY 8a "universal invariant"); vertices = junction k-mers with an edge; links = sum over them of in x out."""
    k = 21
    reads = synth_reads(3000, read_len=150, genome_len=9000, sub_rate=0.005, seed=5)
    r = ctx.reads_from_ascii(reads)
    x = ctx.extindex(r, k)
    u = ctx.unitigs(x)
    assert u.n_loops == 0
    ur = u.to_reads()
    assert ur.to_list() == u.sequences()
    e_reads = ctx.count(r, k + 1, B.CANONICAL | B.WITH_COUNTS)
    e_unitigs = ctx.count(ur, k + 1, B.CANONICAL | B.WITH_COUNTS)
    seqs = u.sequences()
    assert len(e_unitigs) == sum(len(s) - k for s in seqs) == len(e_reads)
    ku, cu = e_unitigs.export(with_counts=True)
    kr, _ = e_reads.export(with_counts=True)
    assert np.array_equal(ku, kr) and int(cu.max()) == 1
    _, masks = x.export()
    pop = np.array([bin(i).count("1") for i in range(16)])
    outs, ins = pop[masks & 15], pop[masks >> 4]
    junction = (outs != 1) | (ins != 1)
    assert u.n_vertices == int(junction.sum())
    assert u.n_links == int((outs[junction] * ins[junction]).sum())
    exp = O.ExtIndex(reads, k, 1).unitigs()
    _, nv, nl = exp.gfa()
    assert (len(u), u.n_vertices, u.n_links) == (exp.n, nv, nl)


# ---- where a result lives ------------------------------------------------------------------------------------------
# A unitig set is on the device after a build without perfect loops, on the host after a build with loops (or of an
# empty index), and on both once a host export (sequences(), links(), a host-side writer) has run.  Every consumer
# must give the same answer in each of these states.
RES_K = 21


def residency_reads(loops):
    """600 reads of a 2.5 kb genome: >= 500 unitigs and no perfect loop at k = 9, 21 and 101 (the tests assert it);
    with the six circles of test_circular_genomes_loops appended the result has loops and lives on the host."""
    reads = synth_reads(600, read_len=150, genome_len=2500, sub_rate=0.01, seed=1)
    return reads + six_circles() if loops else reads


@pytest.fixture(scope="module")
def residency_oracle():
    """gfa(with_cov=True) of the oracle for the no-loop and the loop graph at RES_K, computed once"""
    out = {}
    for loops in (False, True):
        ou = O.ExtIndex(residency_reads(loops), RES_K, 1).unitigs()
        out[loops] = (ou.n, ou.n_loops, ou.gfa(with_cov=True)[0])
    return out


def build_unitigs(ctx, reads, k):
    r = ctx.reads_from_ascii(reads)
    return r, ctx.unitigs(ctx.extindex(r, k))


@pytest.mark.parametrize("k", [9, 21, 101])
def test_gfa_text_of_device_result(ctx, k, tmp_path):
    """Written before any host export the text comes from the device formatter: byte for byte the S and L lines of the
    exported sequences and links, with <k>M of 1, 2 and 3 digits and segment ids of 1 to 4 digits; written again after
    the export (both copies present) the file is the same."""
    _, u = build_unitigs(ctx, residency_reads(False), k)
    first = gfa_bytes(u, tmp_path / "first.gfa")
    assert u.n_loops == 0 and len(u) >= 500
    assert first == expected_gfa(u, k)
    assert gfa_bytes(u, tmp_path / "second.gfa") == first


def test_gfa_text_of_host_result(ctx, tmp_path):
    """a result with perfect loops lives on the host and goes through the host formatter: the same bytes"""
    _, u = build_unitigs(ctx, residency_reads(True), RES_K)
    got = gfa_bytes(u, tmp_path / "loops.gfa")
    assert u.n_loops >= 1 and len(u) - u.n_loops >= 500
    assert got == expected_gfa(u, RES_K)


@pytest.mark.parametrize("loops", [True, False])
def test_to_reads_of_host_and_two_copy_result(ctx, loops):
    """to_reads of a host-only result (loops) and of one that is on the device and on the host (sequences() ran first);
    test_unitigs_to_reads_and_graph_invariants covers the device-only state"""
    _, u = build_unitigs(ctx, residency_reads(loops), RES_K)
    assert (u.n_loops >= 1) == loops
    seqs = u.sequences()
    assert u.to_reads().to_list() == seqs


@pytest.mark.parametrize("loops", [True, False])
def test_coverage_of_host_and_two_copy_result(ctx, residency_oracle, loops, tmp_path):
    """add_coverage on a host-only result (loops) and on one whose host copy was made before (sequences() ran first)"""
    n, n_loops, exp = residency_oracle[loops]
    r, u = build_unitigs(ctx, residency_reads(loops), RES_K)
    assert (len(u), u.n_loops) == (n, n_loops) and (n_loops >= 1) == loops
    if not loops:
        u.sequences()
    u.add_coverage(r)
    got = gfa_bytes(u, tmp_path / "cov.gfa").decode()
    assert gfa_canon.canon_md5(got, with_kc=True) == gfa_canon.canon_md5(exp, with_kc=True)


def test_empty_graph(ctx, tmp_path):
    """reads all shorter than k: an index of no k-mers gives an empty result that lives on the host; every export and
    every writer works on it (empty files; the SPAdes binary keeps its three header words and its end mark)"""
    r = ctx.reads_from_ascii(["ACGTACGTAC", "", "TTGACCA" * 2, "ACGTN" * 4])
    x = ctx.extindex(r, RES_K)
    assert len(x) == 0
    u = ctx.unitigs(x)
    assert (len(u), u.n_loops, u.n_vertices, u.n_links, u.total_bases) == (0, 0, 0, 0, 0)
    assert u.sequences() == []
    assert u.links().shape == (0, 4)
    assert u.to_reads().to_list() == []
    sizes = {}
    for fmt in ("gfa", "fasta", "fastg"):
        p = str(tmp_path / ("e." + fmt))
        getattr(u, "write_" + fmt)(p)
        sizes[fmt] = os.path.getsize(p)
    u.write_spades(str(tmp_path / "e"))
    sizes["grseq"] = os.path.getsize(str(tmp_path / "e.grseq"))
    sizes["cvr"] = os.path.getsize(str(tmp_path / "e.cvr"))
    assert sizes == {"gfa": 0, "fasta": 0, "fastg": 0, "grseq": 24, "cvr": 8}
