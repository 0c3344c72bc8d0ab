"""CPU: the restatement of ReadCorrector (tests/readcorrect_restated.py) itself -- its model of libstdc++'s heap against
std::priority_queue of the compiler at hand, and the crafted reads of tests/readcorrect_cases.py, which must take every
branch of the rule and come out as each case states."""
import os
import subprocess

import numpy as np
import pytest

from tests import readcorrect_cases as Cs
from tests import readcorrect_restated as R

HERE = os.path.dirname(os.path.abspath(__file__))
ALL_LABELS = {"own-good", "own-bad-hi", "own-bad-lo", "own-absent-hi", "own-absent-lo", "alt-hi", "alt-lo", "alt-N",
              "flush-extended", "flush-penalty", "flush-cluster", "flush-top"}


@pytest.fixture(scope="module")
def heap_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("heap") / "heap_order_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(HERE, "heap_order_check.cpp")])
    return exe


class _Item:
    def __init__(self, penalty, pos, ident):
        self.penalty, self.pos, self.id = penalty, pos, ident


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_heap_model_pops_in_the_order_of_std_priority_queue(heap_exe, seed):
    rng = np.random.default_rng(seed)
    q = R.PriorityQueue(R.state_less)
    ops, exp = [], []
    for i in range(4000):
        # more pushes than pops at first, then the reverse: the heap grows to a few hundred and drains
        if rng.random() < (0.65 if i < 2000 else 0.35):
            pen, pos = -int(rng.integers(0, 4)), int(rng.integers(0, 4))
            ops.append("push %d %d %d" % (pen, pos, i))
            q.push(_Item(pen, pos, i))
        else:
            ops.append("pop")
            if q.empty():
                exp.append("-")
            else:
                exp.append(str(q.top().id))
                q.pop()
    assert q.tie  # equal (penalty, pos) pairs did meet
    r = subprocess.run([heap_exe], input="\n".join(ops) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == exp


def test_heap_model_is_not_a_stable_queue():
    """what makes the model necessary: among equal elements neither the first nor the last pushed comes out first"""
    q = R.PriorityQueue(R.state_less)
    for i in range(6):
        q.push(_Item(0, 0, i))
    order = []
    while not q.empty():
        order.append(q.top().id)
        q.pop()
    assert order not in (list(range(6)), list(range(5, -1, -1)))


@pytest.mark.parametrize("k", [11, 21, 32])
def test_unit_cases(k):
    cases = Cs.unit_cases(k) + [Cs.size_thr_case(k)]
    index, keys, good, reads = Cs.build(cases)
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    rc = R.ReadCorrector(index, good, k)
    out, res = rc.correct_batch(reads)
    seen = set()
    for i, c in enumerate(cases):
        infos = [inf for r, _, inf in rc.searches if r == i]
        labels = set().union(*[inf.labels for inf in infos]) if infos else set()
        seen |= labels
        assert c.labels <= labels, c.what
        assert res[i] == c.result, c.what
        if c.corrected is not None:
            assert out[i] == c.corrected, c.what
        if c.island is not None:
            assert rc.island(c.seq, c.qual)[:2] == c.island, c.what
        if c.failed is not None:
            assert sum(inf.failed for inf in infos) == c.failed, c.what
        assert len(infos) == (2 if 0 < rc.island(c.seq, c.qual)[2] < len(c.seq) else 0), c.what
    assert seen == ALL_LABELS
    by_name = {c.what: i for i, c in enumerate(cases)}
    # the failed search counts the bases to the right of the island, and only those
    c = cases[by_name["N without alternative"]]
    assert rc.stats()[2] == len(c.seq) - 1 - c.island[1] + 1
    assert rc.stats()[3] == sum(len(c.seq) for c in cases)
    # the size_thr case outgrows 100 * log2(n) + 1
    inf = [inf for r, d, inf in rc.searches if r == by_name["size_thr"] and d == 0][0]
    assert inf.flush_top_only > 0 and inf.max_heap > 100


def test_outer_cpos_quirk_matters():
    """with the popped state's cpos in the own-nucleotide candidate the fifth correction of the 'outer cpos' read would be
    refused: the case is not vacuous"""
    k = 21
    c = [x for x in Cs.unit_cases(k) if x.what == "outer cpos"][0]
    index, keys, good, reads = Cs.build([c])
    rc = R.ReadCorrector(index, good, k)
    out, _ = rc.correct_batch(reads)
    assert out[0] == c.corrected
    n_changed = sum(1 for a, b in zip(out[0], c.seq) if a != b)
    assert n_changed == 5 and rc.stats()[:2] == [1, 5]
    other = R.ReadCorrector(index, good, k)
    other.own_candidate_keeps_cpos = True
    out2, _ = other.correct_batch(reads)
    assert out2[0] != c.corrected and "flush-cluster" in set().union(*[inf.labels for _, _, inf in other.searches])


def test_short_reads_are_not_counted():
    k = 21
    g = R.genome(40, 9, k)
    index, keys, good = R.make_index(R.kmers_of(g, k))
    rc = R.ReadCorrector(index, good, k)
    out, res = rc.correct_batch([(g[:20], [30] * 20), ("", []), (g, [30] * 40)])
    assert res == [0, 0, 1] and out == [g[:20], "", g] and rc.stats() == [0, 0, 0, 40]


def test_branching_reads():
    """the crafted reads of the capacity tests: ties at 60 bases inside the limits the device starts with, far outside
    them at 150"""
    k = 21
    for length, step, inside in ((60, 4, True), (150, 2, False)):
        read, qual, good_kmers = R.branching_read(k, length, step=step)
        index, keys, good = R.make_index(good_kmers)
        rc = R.ReadCorrector(index, good, k)
        out, res = rc.correct_batch([(read, qual)])
        inf = rc.searches[0][2]
        assert res == [1] and inf.tie and not inf.failed
        assert (inf.max_heap <= 32 and inf.pops <= 1024) == inside


def test_read_print():
    s, q, lt, rt, n = R.trim_read("NNACGTACGTNN", [30] * 12, 4)
    assert (s, lt, rt, n) == ("ACGTACGTNN", 2, 12, 12)  # the left trim keeps the bad tail
    assert R.read_print("r", s, q, lt, rt, n, 33) == "@r\nNNACGTACGTNN\n+r ltrim=2\n##" + "?" * 10 + "\n"
    s, q, lt, rt, n = R.trim_read("ACGTACGTNN", [30] * 10, 4)
    assert (s, lt, rt, n) == ("ACGTACGT", 0, 8, 10)
    assert R.read_print("r", s, q, lt, rt, n, 33) == "@r\nACGTACGTNN\n+r rtrim=2\n" + "?" * 8 + "##\n"
    s, q, lt, rt, n = R.trim_read("NNNN", [30] * 4, 4)
    assert (s, lt, rt, n) == ("", 0, 4, 4)
    assert R.read_print("r", s, q, lt, rt, n, 33) == "@r\n\n+r\n\n"
