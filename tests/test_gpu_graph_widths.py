"""GPU: the graph stage (walk, keep rule, link records, perfect loops, self-conjugate edges, GFA, early tip clipper)
against the CPU oracle on both sides of every key-word boundary and in all four key widths: k = 31 | 33 (W = 1 | 2,
the (k+1)-mer fills a word at 31), 63 | 65 (W = 2 | 3), 95 | 97 (W = 3 | 4) and 125 (the widest k the oracle takes).
At these k kmer_shl's last shift is 60 or wraps to 0, kmer_rc shifts by 2 or by 62 bits across words, and the leftover
k-mers of the loop phase are bucketed by all three shapes of xxh3_64<W>.

Every input is tiny; the shape facts a case relies on (how many loops, how many self-conjugate unitigs, that the loop
strings depend on the reference thread count, that the clipper removes something) are asserted from the oracle's own
result before the engine is compared with it, so a change of a generator cannot turn a case into a trivial one."""
import numpy as np
import pytest

import spades_for_blackbird_amd as B
from oracle import oracle as O
from spades_for_blackbird_amd.tools import gfa_canon
from tests import atclip_restated as R
from tests.helpers import expected_gfa, gfa_bytes, polya_reads, rc, synth_reads

pytestmark = pytest.mark.gpu

KS = [31, 33, 63, 65, 95, 97, 125]
TS = (1, 2, 5)


@pytest.fixture(scope="module")
def ctx():
    c = B.Context(0)
    yield c
    c.close()


# ---- 1. crafted loops, hairpins and self-conjugate edges -----------------------------------------------------------
def _bases(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def _windows(circ, length, step):
    rep = circ * 3
    return [rep[s:s + length] for s in range(0, len(circ), step)]


def circles(k, seed):
    """three random circles without junctions: perfect loops"""
    rng = np.random.default_rng(seed)
    reads = []
    for c in range(3):
        reads += _windows(_bases(rng, 2 * k + 40 + 17 * c), k + 40, 7)
    return reads


def hairpin(k, seed):
    """the circle X + rc(X): its own reverse complement, with a palindromic (k+1)-mer around each of the two seams;
    SplitLoop cuts it there into two self-conjugate pieces"""
    x = _bases(np.random.default_rng(seed), k + 30)
    return _windows(x + rc(x), 2 * k + 10, 5)


def selfconj(k, seed):
    """a + rc(a) holds one palindromic (k+1)-mer in its middle; the second read branches off 20 bases into it, so the
    palindromic stretch hangs off a junction: a unitig that is its own reverse complement, with a link to itself"""
    rng = np.random.default_rng(seed)
    a = _bases(rng, (k + 1) // 2 + 40)
    first = a + rc(a)
    return [first, _bases(rng, 30) + first[20:20 + k + 5]]


def combined(k, seed):
    return circles(k, seed) + hairpin(k, seed + 1) + hairpin(k, seed + 2) + selfconj(k, seed + 3)


FAMILIES = {"circles": circles, "hairpin": hairpin, "selfconj": selfconj, "combined": combined}
SEED_OFFSET = {"circles": 0, "hairpin": 1, "selfconj": 3, "combined": 0}


def family_reads(family, k):
    return FAMILIES[family](k, k + SEED_OFFSET[family])


def n_self_rc(seqs):
    return sum(1 for s in seqs if s == rc(s))


def has_palindromic_edge(seqs, k):
    return any(s[i:i + k + 1] == rc(s[i:i + k + 1]) for s in seqs for i in range(len(s) - k))


def oracle_graph(reads, k, T):
    ou = O.ExtIndex(reads, k, T).unitigs()
    txt, nv, nl = ou.gfa()
    return {"n": ou.n, "n_loops": ou.n_loops, "seqs": ou.seqs, "loops": ou.seqs[ou.n - ou.n_loops:],
            "paths": ou.seqs[:ou.n - ou.n_loops], "nv": nv, "nl": nl, "gfa": txt}


def check_links(u, k):
    """every link joins two oriented segments that overlap in k bases (as test_fasta_and_links_export)"""
    seqs = u.sequences()
    links = u.links()
    assert links.shape == (u.n_links, 4)
    for a, oa, b, ob in links.tolist():
        sa = seqs[a] if oa else rc(seqs[a])
        sb = seqs[b] if ob else rc(seqs[b])
        assert sa[-k:] == sb[:k], (a, oa, b, ob)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_crafted_graphs_string_for_string(ctx, family, k, tmp_path):
    """With ref_threads = T the engine visits the leftover k-mers in the k-mer file order of a reference run with -t T
    (10 T XXH3 buckets), like the oracle: the loop strings -- where each starts, and which palindromic (k+1)-mer a
    self-conjugate circle is cut at -- are EQUAL as lists, at every key width and on both sides of a word boundary."""
    reads = family_reads(family, k)
    exp = {T: oracle_graph(reads, k, T) for T in TS}
    # what the oracle alone says about the shape of this input
    for T in TS:
        e = exp[T]
        split = has_palindromic_edge(e["loops"], k)
        if family == "circles":
            assert (e["n"], e["n_loops"]) == (3, 3) and not split
        elif family == "hairpin":
            assert (e["n"], e["n_loops"], e["nv"], e["nl"]) == (2, 2, 1, 1)
            assert n_self_rc(e["loops"]) == 2 and split
        elif family == "selfconj":
            assert (e["n"], e["n_loops"], e["nv"], e["nl"]) == (3, 0, 3, 2)
            assert n_self_rc(e["seqs"]) == 1 and has_palindromic_edge(e["seqs"], k)
        else:
            assert e["n_loops"] == 7 and n_self_rc(e["loops"]) == 4 and n_self_rc(e["paths"]) == 1
    if family == "combined":
        # the visit order over the XXH3 buckets really changes what comes out
        assert len(set(tuple(exp[T]["loops"]) for T in TS)) > 1

    r = ctx.reads_from_ascii(reads)
    for T in TS:
        e = exp[T]
        u = ctx.unitigs(ctx.extindex(r, k), ref_threads=T)
        got = u.sequences()
        assert (len(u), u.n_loops, u.n_vertices, u.n_links) == (e["n"], e["n_loops"], e["nv"], e["nl"]), T
        nl = u.n_loops
        assert got[len(got) - nl:] == e["loops"], T           # the loop strings, in order, not modulo rotation
        assert sorted(got[:len(got) - nl]) == sorted(e["paths"]), T
        if family in ("circles", "selfconj"):
            txt = gfa_bytes(u, tmp_path / ("T%d.gfa" % T)).decode()
            assert gfa_canon.canon_text(txt, k) == gfa_canon.canon_text(e["gfa"], k), T
        if family == "selfconj":
            check_links(u, k)
            for s in got:
                assert not (s < rc(s))


# ---- 2. read-derived graphs ------------------------------------------------------------------------------------------
def read_graph_reads(k, extras):
    reads = synth_reads(600, read_len=k + 80, genome_len=4000, sub_rate=0.01, seed=k, n_rate=0.001)
    if extras:
        reads += ["", "A" * k, "A" * (k + 1), "ACGTTGCATT" * 26, "acgtn" * 60]
    return reads


_READ_GRAPH = {}


def read_graph_oracle(k, extras):
    if (k, extras) not in _READ_GRAPH:
        _READ_GRAPH[k, extras] = oracle_graph(read_graph_reads(k, extras), k, 1)
    return _READ_GRAPH[k, extras]


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("k", KS)
def test_read_graph_vs_oracle(ctx, monkeypatch, k, wide, tmp_path):
    """Hundreds of unitigs from reads with errors and Ns: counts and the canonical GFA against the oracle, once more
    with 64-bit prefix-table entries (BBK_WIDE_INDEX is read per call).  With the fixed extras the graph also holds
    two perfect loops that are not self-conjugate (the poly-A k-mer and a period-10 repeat), which the canonical form
    compares modulo rotation, and the result lives on the host; without them there is no loop, the result stays on the
    device and its GFA text comes from the device formatter, which must equal the text of the host export."""
    if wide:
        monkeypatch.setenv("BBK_WIDE_INDEX", "1")
    for extras in (True, False):
        e = read_graph_oracle(k, extras)
        assert e["n"] >= 500 and e["nl"] > 0 and e["n_loops"] == (2 if extras else 0)
        assert not has_palindromic_edge(e["loops"], k)            # no split loop: the full comparison applies
        r = ctx.reads_from_ascii(read_graph_reads(k, extras))
        u = ctx.unitigs(ctx.extindex(r, k))
        first = gfa_bytes(u, tmp_path / "first.gfa")              # before any host export
        assert (len(u), u.n_loops, u.n_vertices, u.n_links) == (e["n"], e["n_loops"], e["nv"], e["nl"]), extras
        assert gfa_canon.canon_text(first.decode(), k) == gfa_canon.canon_text(e["gfa"], k), extras
        assert first == expected_gfa(u, k), extras
        assert gfa_bytes(u, tmp_path / "second.gfa") == first     # both copies present: the same file


# ---- 3. early tip clipper ------------------------------------------------------------------------------------------
# the input shape of test_early_tip_clipping (errors near read ends give tips) at a smaller size; the bounds were chosen
# with the oracle alone: below k some tips are clipped and longer ones stay, from k on every dead end goes
TIP_BOUND = {63: 40, 65: 85, 97: 20, 125: 125}


def tip_reads(k):
    reads = synth_reads(1000, read_len=k + 60, genome_len=8000, sub_rate=0.01, seed=31 + k, n_rate=0.001)
    return reads + ["ACGT" * 50, "A" * (k + 60)]


_TIPS = {}


def tip_oracle(k):
    """the oracle's clipper and the unitigs of its clipped index, computed once per k"""
    if k not in _TIPS:
        ox = O.ExtIndex(tip_reads(k), k, 1)
        removed, links = ox.clip_tips(TIP_BOUND[k])
        order = np.lexsort([ox.kmers[:, j] for j in range(ox.kmers.shape[1] - 1, -1, -1)])
        keys, masks = ox.kmers[order], ox.masks[order]
        _TIPS[k] = (removed, links, keys, masks, sorted(min(s, rc(s)) for s in ox.unitigs().seqs))
    return _TIPS[k]


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("k", list(TIP_BOUND))
def test_tip_clipping_vs_oracle(ctx, monkeypatch, k, wide):
    """bbk_extindex_clip_tips against the oracle's EarlyTipClipperProcessor::ClipTips with 16-, 24- and 32-byte keys:
    same isolated k-mers, same removed links, identical masks, the same unitigs of the clipped index"""
    exp_removed, exp_links, ekeys, emasks, eseqs = tip_oracle(k)
    assert exp_removed > 0 and exp_links > 0
    if wide:
        monkeypatch.setenv("BBK_WIDE_INDEX", "1")
    x = ctx.extindex(ctx.reads_from_ascii(tip_reads(k)), k)
    assert x.clip_tips(TIP_BOUND[k]) == (exp_removed, exp_links)
    gk, gm = x.export()
    assert np.array_equal(gk, ekeys)
    assert np.array_equal(gm, emasks)
    assert sorted(min(s, rc(s)) for s in ctx.unitigs(x).sequences()) == eseqs


def test_at_clipper_then_tip_clipper_k125(ctx):
    """the early poly-A/T passes, then the tip clipper, then the unitig stage with 32-byte keys: against the restated
    A/T passes written into the oracle's masks and the oracle's own clipper and unitigs"""
    k, bound = 125, 40
    reads = polya_reads()
    ox = O.ExtIndex(reads, k, 1)
    ix = R.Index.from_oracle(ox)
    at_edges = R.remove_at_edges(ix, 0.8)
    at_tips = R.remove_at_tips(ix, 0.8, 10, 200)
    np.ctypeslib.as_array(ox._st.masks, shape=(ox._st.n_k,))[:] = ix.mask_array()
    exp_clip = ox.clip_tips(bound)
    assert at_edges[0] > 0 and at_tips[0] > 0 and exp_clip[0] > 0 and exp_clip[1] > 0
    x = ctx.extindex(ctx.reads_from_ascii(reads), k)
    assert x.remove_at_edges() == at_edges
    assert x.remove_at_tips() == at_tips
    assert x.clip_tips(bound) == exp_clip
    got = sorted(min(s, rc(s)) for s in ctx.unitigs(x).sequences())
    assert got == sorted(min(s, rc(s)) for s in ox.unitigs().seqs)
