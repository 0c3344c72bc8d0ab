"""CPU: the literal restatement of unitig-coverage (MapSequence read by read, each read followed by its reverse
complement) equals the position-local form the GPU kernel applies, on graphs the oracle builds and on the golden
corner-case graphs.  The GPU tests (tests/test_gpu_unitig_coverage.py) compare the engine against the literal form."""
import random

import pytest

from oracle import oracle as O
from tests import unitig_profile_restated as R
from tests.helpers import rc


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _mutate(rng, s):
    """substitutions, insertions, deletions and an occasional N"""
    out = []
    for c in s:
        x = rng.random()
        if x < 0.02:
            out.append(rng.choice("ACGT".replace(c, "")))
        elif x < 0.03:
            out.append(c + rng.choice("ACGT"))
        elif x < 0.04:
            continue
        elif x < 0.045:
            out.append("N")
        else:
            out.append(c)
    return "".join(out)


def _reads_of(rng, genome, n, lo, hi, mutate):
    reads = []
    for _ in range(n):
        ln = rng.randint(lo, hi)
        st = rng.randint(0, max(0, len(genome) - ln))
        r = genome[st:st + ln]
        if rng.random() < 0.5:
            r = rc(r)
        reads.append(_mutate(rng, r) if mutate else r)
    return reads


def _graph(reads, k):
    return R.Graph.from_gfa(O.ExtIndex(reads, k, 1).unitigs().gfa()[0], k)


def _check(g, samples):
    lit = R.fill_literal(g, samples)
    assert R.segment_raw(g, lit) == R.fill_position_local(g, samples)
    # the conjugate edge of a segment gets what its forward edge gets (reads are followed by their reverse complement)
    for e, c in g.conj.items():
        assert lit[e] == lit[c]
    return lit


def test_longest_valid_and_parse():
    assert R.longest_valid("NNACGTNACGTAN") == "ACGTA"
    assert R.longest_valid("acgNNACG") == "ACG"  # the first of equally long runs
    assert R.longest_valid("NNN") == ""
    names, seqs, links = R.parse_gfa("S\t3\tACGTA\tDP:f:0\nS\t5\tTTT\nL\t3\t+\t5\t-\t2M\n")
    assert names == ["3", "5"] and seqs == ["ACGTA", "TTT"] and links == [(0, "+", 1, "-")]


@pytest.mark.parametrize("k,seed", [(5, 1), (5, 2), (7, 3), (9, 4), (21, 5)])
def test_literal_equals_position_local_random(k, seed):
    rng = random.Random(seed)
    genome = _rand(rng, 300 if k < 21 else 2000)
    base = _reads_of(rng, genome, 60, 2 * k, 4 * k + 20, mutate=False)
    g = _graph(base, k)
    samples = [base, _reads_of(rng, genome, 80, 1, 4 * k + 30, mutate=True),
               _reads_of(rng, _rand(rng, 200) + genome[:200], 40, k, 3 * k, mutate=True)]
    lit = _check(g, samples)
    # the reads the graph was built from cover every (k+1)-mer position exactly once per strand
    assert sum(R.segment_raw(g, lit)[i][0] for i in range(len(g.names))) > 0


def test_reads_shorter_than_k_plus_one_and_ns():
    rng = random.Random(7)
    genome = _rand(rng, 200)
    g = _graph(_reads_of(rng, genome, 30, 20, 40, mutate=False), 5)
    lit = _check(g, [["ACGT", "", "NNNN", "ACGTA", genome[10:15] + "N" + genome[16:40]]])
    assert any(v[0] for v in lit.values())


def test_self_rc_edge(golden):
    gk = golden["self_rc_edge_k5"]
    k = gk["k"]
    g = _graph(gk["reads"], k)
    assert sorted(g.seq[2 * i] for i in range(len(g.names))) == sorted(gk["S"])
    selfc = [i for i in range(len(g.names)) if g.conj[2 * i] == 2 * i]
    assert len(selfc) == 1 and g.seq[2 * selfc[0]] == "AGGATCCT"  # holds the palindromic 6-mer GGATCC
    rng = random.Random(11)
    src = gk["reads"][0]
    _check(g, [gk["reads"], [_mutate(rng, src) for _ in range(30)] + ["GGATCC", "AGGATCCTAA", rc(src)]])


def test_loop(golden):
    gk = golden["loop_k5"]
    k = gk["k"]
    g = R.Graph(k, ["3"], gk["S"], [(0, oa, 0, ob) for _, oa, _, ob in gk["L"]])  # the reference's own loop string
    assert g.outgoing_of_end(0) == [0] and g.outgoing_of_end(1) == [1]
    circ = gk["S"][0]
    rng = random.Random(5)
    # reads that go round the circle more than once re-enter the loop edge at offset 0
    _check(g, [gk["reads"], [circ + circ[k:] + circ[k:k + 7], _mutate(rng, circ * 3), rc(circ * 2)]])


def test_homopolymer_loop_edge():
    """A^(k+1) on its own is a one-(k+1)-mer edge linked to itself; inside a run of A TryThread re-enters it with a new
    range of size 1 where the merge rule would give 0: the position-local form carries that case as a flag"""
    rng = random.Random(3)
    k = 5
    genome = _rand(rng, 60) + "A" * 12 + _rand(rng, 60)
    g = _graph(_reads_of(rng, genome, 40, 20, 50, mutate=False) + [genome], k)
    loops = [e for e in g.seq if R.loop1(g, e)]
    assert loops and g.seq[loops[0]] in ("A" * (k + 1), "T" * (k + 1))
    _check(g, [[genome, "C" + "A" * 20 + "G", "A" * 9, "T" * 15], [_mutate(rng, genome) for _ in range(10)]])


def test_save_format():
    g = R.Graph(3, ["3", "5"], ["ACGTTG", "CCCAT"], [])
    raw = {e: [0, 0] for e in g.seq}
    raw[0] = [33220 // 1000, 1]
    raw[2] = [0, 7]
    assert R.save(g, raw) == "3\t11\t0.333333\t\n5\t0\t3.5\t\n"
    assert "%g" % (33220 / (307 - 21)) == "116.154"
