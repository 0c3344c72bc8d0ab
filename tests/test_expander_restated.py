"""CPU: what ties the engine's snapshot rounds to the reference's Expander, on the literal restatement
(tests/expander_restated.py): which reads can ever be solid, G_t within S_t within the closure for one thread in any
read order, equal closures, and the chain of overlapping reads on which the reference's answer depends on the order."""
import gzip
import os

import numpy as np
import pytest

from tests import expander_restated as E
from tests import kmerdata_restated as KR

KS = [10, 11, 21, 22, 32]


def _crafted(k):
    return [(s, q) for _, s, q in KR.crafted_reads(k, np.random.default_rng(100 + k))]


@pytest.fixture(scope="module")
def golden_reads(golden_dir):
    with gzip.open(os.path.join(golden_dir, "ecoli_1K_1.fq.gz"), "rt") as f:
        lines = f.read().split("\n")
    return [(lines[i + 1], [ord(c) - 33 for c in lines[i + 3]]) for i in range(0, len(lines) - 3, 4)]


@pytest.mark.parametrize("k", KS)
def test_candidates_are_the_reads_that_can_ever_be_solid_crafted(k):
    reads = _crafted(k)
    for trim_quality in (4, 2):
        cand = {i for i, _, _ in E.candidates(reads, k, trim_quality)}
        assert cand == {i for i, (s, q) in enumerate(reads) if E.can_ever_be_solid(s, q, k, trim_quality)}
    names = [w for w, _, _ in KR.crafted_reads(k, np.random.default_rng(100 + k))]
    cand = {names[i] for i, _, _ in E.candidates(reads, k)}
    assert cand == {"left trim keeps the q=3 tail", "right trim alone", "thresholds", "exactly k"}
    # the q = 1 tail survives the trimming and end_ stops before it; an interior N; fewer than k bases
    assert not cand & {"left trim keeps the q=1 tail", "N-splitting", "shorter than k after trimming"}


def test_candidates_are_the_reads_that_can_ever_be_solid_golden(golden_reads):
    k = 21
    cand = E.candidates(golden_reads, k)
    assert len(cand) == 2054 == len(golden_reads)
    assert all(E.can_ever_be_solid(s, q, k) for s, q in golden_reads)
    # a candidate is the whole trimmed read
    for i, st, n in cand[:200]:
        s, _, ltrim = KR.trim_ns_and_bad_quality(*golden_reads[i], 4)
        assert (st, n) == (ltrim, len(s))


class _ByStart(dict):
    """a stand-in set in which the p-th lookup of a read finds k-mer p: every start is its own k-mer"""

    def __init__(self):
        self.p = -1

    def get(self, key, default=None):
        self.p += 1
        return self.p


def test_solid_rule_is_full_coverage():
    """the three conditions of a snapshot round are covered_by_solid all true (expander.cpp:30-51)"""
    rng = np.random.default_rng(5)
    for k in (1, 2, 5, 21):
        for _ in range(300):
            nk = int(rng.integers(1, 3 * k + 4))
            g = rng.random(nk) < rng.choice([0.1, 0.5, 0.9])
            read = "A" * (nk + k - 1)
            s, _ = E.read_status(read, k, _ByStart(), [int(x) for x in g])
            assert (s != 0) == all(E.covered(len(read), k, [p for p in range(nk) if g[p]])), (k, g)
            assert (s == 2) == bool(g.all())


def _bracket(reads, cands, k, index, good, order):
    """G_t within S_t within the closure for every t, and equal closures; returns (snapshot counts, literal counts)"""
    closure, snap_counts, states = E.snapshot_rounds(cands, k, index, good, None, 1)
    s = list(good)
    lit_counts = []
    t = 0
    while True:
        c = E.expand_pass(reads, k, index, s, order)
        lit_counts.append(c)
        t += 1
        g = states[min(t, len(states) - 1)]
        assert all(a <= b for a, b in zip(g, s)), t
        assert all(a <= b for a, b in zip(s, closure)), t
        if c == 0:
            break
    assert s == closure
    assert len(lit_counts) <= len(snap_counts)  # marks seen at once never need more passes
    return snap_counts, lit_counts


@pytest.mark.parametrize("k", [21, 32])
def test_chain(k):
    reads, index, keys, good = E.chain_case(k)
    n_fwd = len(keys) // 2
    assert n_fwd == 98 and sum(good) == 31
    cands = E.candidate_reads(reads, k)
    assert cands == [s for s, _ in reads]
    fwd = range(len(reads))
    rev = list(reversed(fwd))
    snap, lit = _bracket(reads, cands, k, index, good, None)
    assert snap == [9] + [6] * 9 + [4, 0]
    assert lit == [67, 0]  # file order: one pass
    snap, lit = _bracket(reads, cands, k, index, good, rev)
    assert lit == [9] + [6] * 9 + [4, 0] == snap  # reverse file order gives exactly the snapshot rounds
    closure, _, _ = E.snapshot_rounds(cands, k, index, good, None, 1)
    assert sum(closure) == 98 and all(closure[index[cands[0][p:p + k]]] for p in range(11))
    assert not any(closure[index[KR.revcomp(cands[0][p:p + k])]] for p in range(11))  # no reverse complement is marked
    # the default stop rule: 9 < 10 ends both after their first round / pass
    g1, counts, _ = E.snapshot_rounds(cands, k, index, good)
    assert counts == [9] and sum(g1) == 40
    assert E.expand_loop(reads, k, index, good, rev)[1] == [9]
    assert E.expand_loop(reads, k, index, good, None)[1] == [67, 0]  # ... and file order goes on to the closure
    assert E.snapshot_rounds(cands, k, index, good, 2, 1)[1] == [9, 6]


@pytest.mark.parametrize("k", KS)
def test_crafted_reads_bracket_and_closure(k):
    reads = _crafted(k)
    index, keys = E.index_of_reads(reads, k)
    cands = E.candidate_reads(reads, k)
    assert len(cands) == 4
    rng = np.random.default_rng(900 + k)
    grew = 0
    for _ in range(6):
        good = [int(x) for x in rng.random(len(keys)) < 0.7]
        for order in (None, list(reversed(range(len(reads))))):
            snap, _ = _bracket(reads, cands, k, index, good, order)
        grew += sum(snap)
    assert grew > 0


def test_golden_reads_bracket_and_closure(golden_reads):
    k = 21
    index, keys = E.index_of_reads(golden_reads, k)
    cands = E.candidate_reads(golden_reads, k)
    good = [int(x) for x in np.random.default_rng(2101).random(len(keys)) < 0.5]
    fwd_idx = {index[c[p:p + k]] for c in cands for p in range(len(c) - k + 1)}
    before = sum(good[i] for i in fwd_idx)
    snap, lit = _bracket(golden_reads, cands, k, index, good, None)
    _bracket(golden_reads, cands, k, index, good, list(reversed(range(len(golden_reads)))))
    assert sum(snap) > 0 and sum(snap) == sum(lit)
    closure = E.snapshot_rounds(cands, k, index, good, None, 1)[0]
    assert sum(closure[i] for i in fwd_idx) == before + sum(snap)
